"""The cases of the kernel-level assignment tests (test_gpu_assign.py, test_assign_host.py), their seeded
inputs, and the launcher conditions that send each case to its kernel instantiation.

Two routes of `lg_assign`: "recomputed" (assign_h3.hip sim_h3_kernel<MODE, RAGGED>, the default eval
route) and "materialised" (assign.hip: stats_fused_kernel / la_fused_kernel<K4>, or the four-read
kernels).  Which instantiation a case runs follows from its shape, its counts and LG_ASSIGN_UNFUSED
alone; test_assign_host.py::test_cases_reach_their_routes -- no GPU -- reads the dispatch constants out
of the sources and recomputes every case's route, so moving a threshold fails there and names the case.

Inputs (build_inputs): md0 ~ a N(0, 1); about half of the md1 rows are noisy copies of md0 rows (real
matches: sim ~ |md0|^2 against N(0, .) elsewhere), the rest random; z ~ 3 N(0, 1) with one +30 and two
-30 per side; one all-zero md0 row; with `ties`, exact duplicates planted in pair 0:
  md1 rows j1 < j2 (and z1) equal, both copies of one md0 row, so that row's two best columns tie;
  md0 rows i1 < i2 (and z0) equal, one md1 row their copy, so that column's two best rows tie.
The index pairs are chosen so that the tied candidates sit in one lane / wave, in two waves of a
workgroup, and in two tiles (recomputed: 64-column wave blocks of a 256 tile; materialised: 4 columns
per lane, 256 per register group, 8 rows per wave, CCH rows per chunk).
`rng`: "one" leaves |md|max about 1; "tiny" scales it to exactly 2^-12 (the planes' low pieces near the
fp16 subnormals; the image is one-sided like the forward's, so the exponent stays 0); "big" draws
a = 1 and plants one element of 64 (exponent 3, |sim| up to a few hundred).
"""
import os
import re

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cs566-project-lightglue_amd", "csrc")
TH = 0.1
J_TIES = [(4, 5), (9, 40), (70, 200), (130, -2)]   # md1 duplicates (negative: from the end)
I_TIES = [(1, 5), (9, 40), (20, 100), (60, -2)]    # md0 duplicates


def _case(name, route, B, M, N, expect, why, counts=None, fixed=0, raw=0, unfused=False, rng="one", ties=False,
          matches=True, seed=1):
    return dict(name=name, route=route, B=B, M=M, N=N, expect=expect, why=why, counts=counts, fixed=fixed, raw=raw,
                unfused=unfused, rng=rng, ties=ties, matches=matches, seed=seed)


R3 = [(272, 528), (37, 300), (1, 1)]
R8 = [(272, 528), (256, 257), (257, 256), (16, 512), (0, 0), (5, 0), (37, 300), (1, 1)]
C3 = [(136, 260), (37, 100), (1, 1)]
Z3 = [(136, 260), (40, 0), (0, 7)]  # one-sided zeros: what width pruning can leave in a ragged batch

CASES = [
    # ---- recomputed: sim_h3_kernel
    _case("h3_one_tile", "recomputed", 1, 16, 16, "h3", "one tile, 15/16 of it masked", matches=False, seed=1),
    _case("h3_tiles", "recomputed", 3, 272, 528, "h3", "ntm = 2, ntn = 3, partial last tiles, B % 8 != 0 (xcd_remap)",
          ties=True, seed=2),
    _case("h3_tiles_tiny", "recomputed", 3, 272, 528, "h3", "the same at |md|max = 2^-12: sim ~ 1e-8, la is decided by "
          "the logits (seed chosen so that each side's one +30 beats the next logit by more than two bars)", rng="tiny",
          matches=False, seed=6),
    _case("h3_tiles_big", "recomputed", 3, 272, 528, "h3", "the same at |md|max = 64: exponent 3, |sim| of hundreds", rng="big",
          ties=True, seed=4),
    _case("h3_pair_per_xcd", "recomputed", 8, 256, 272, "h3", "B % 8 == 0 pair-per-XCD mapping, exact row tile, 16-column "
          "last tile", seed=5),
    _case("h3_ragged3", "recomputed", 3, 272, 528, "h3_ragged", "RAGGED: full, interior and 1 x 1 pairs", counts=R3, fixed=1,
          ties=True, seed=6),
    _case("h3_ragged8", "recomputed", 8, 272, 528, "h3_ragged", "RAGGED under the pair-per-XCD mapping: tiles wholly outside, "
          "counts no multiple of 16, on and one past a tile edge, an empty pair, (5, 0) -> (0, 0)", counts=R8, fixed=1,
          ties=True, seed=7),
    # ---- materialised: fused K4 instantiations and chunk edges
    _case("mat_k4_1_min", "materialised", 1, 1, 4, "K4=1", "M = 1 (one row of one wave), N = 4 (one lane)", matches=False,
          seed=10),
    _case("mat_k4_1", "materialised", 3, 63, 252, "K4=1", "M one short of a chunk, N = 252: the last lane masked", seed=11),
    _case("mat_k4_2", "materialised", 3, 136, 260, "K4=2", "N = 260: one lane of the second register group; three chunks, the "
          "last with one full wave", ties=True, seed=12),
    _case("mat_k4_2_big", "materialised", 3, 136, 260, "K4=2", "the same at |md|max = 64", rng="big", ties=True, seed=13),
    _case("mat_k4_4", "materialised", 1, 64, 1024, "K4=4", "M = CCH exactly", seed=14),
    _case("mat_k4_8", "materialised", 1, 65, 2048, "K4=8", "N = kAsMaxN, M one past a chunk", seed=15),
    # ---- materialised: the four-read kernels
    _case("mat_n1", "materialised", 3, 136, 1, "four_read", "N = 1", matches=False, seed=16),
    _case("mat_n255", "materialised", 1, 65, 255, "four_read", "N % 4 != 0: scalar loads", seed=17),
    _case("mat_n2052", "materialised", 1, 64, 2052, "four_read", "N > kAsMaxN, N % 4 == 0: 16-byte loads", seed=18),
    _case("mat_unfused_260", "materialised", 3, 136, 260, "four_read", "LG_ASSIGN_UNFUSED on a fused shape", unfused=True,
          ties=True, seed=12),
    _case("mat_unfused_2048", "materialised", 1, 65, 2048, "four_read", "LG_ASSIGN_UNFUSED on a fused shape", unfused=True,
          seed=15),
    # ---- materialised with counts
    _case("mat_counts", "materialised", 3, 136, 260, "four_read", "the pruned layout: pair-local [Mb+1][Nb+1] blocks, dustbin "
          "column at Nb, last row at Mb", counts=C3, fixed=0, ties=True, seed=19),
    _case("mat_counts_fixed", "materialised", 3, 136, 260, "four_read", "la_ragged_frame_kernel with the four-read kernels",
          counts=C3, fixed=1, ties=True, seed=20),
    _case("mat_one_sided_zero", "materialised", 3, 136, 260, "four_read", "Mb > 0, Nb = 0 and Mb = 0, Nb > 0 (raw counts): no "
          "index formed from an empty row, no matches", counts=Z3, fixed=0, raw=1, ties=True, seed=21),
    _case("mat_one_sided_zero_fixed", "materialised", 3, 136, 260, "four_read", "the same in the fixed layout", counts=Z3,
          fixed=1, raw=1, ties=True, seed=22),
]
BY_NAME = {c["name"]: c for c in CASES}
assert len(BY_NAME) == len(CASES)


def live_counts(case):
    """[(mb, nb)] per pair as the entry point applies them: clamped; an empty side empties the pair unless raw."""
    B, M, N = case["B"], case["M"], case["N"]
    if case["counts"] is None:
        return [(M, N)] * B
    out = []
    for a, b in case["counts"]:
        a, b = min(max(a, 0), M), min(max(b, 0), N)
        if not case["raw"] and (a == 0 or b == 0):
            a = b = 0
        out.append((a, b))
    return out


def tie_pairs(case):
    """([(j1, j2)], [(i1, i2)]) planted in pair 0."""
    if not case["ties"]:
        return [], []
    M, N = case["M"], case["N"]
    return [(a, b % N) for a, b in J_TIES], [(a, b % M) for a, b in I_TIES]


# ------------------------------------------------------------------------------------ inputs
def build_inputs(case):
    """Seeded fp32 CPU tensors: md0 [B,M,256], md1 [B,N,256], z0 [B,M], z1 [B,N]; rows past a pair's counts zero."""
    g = torch.Generator().manual_seed(4000 + case["seed"])
    rn = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    B, M, N = case["B"], case["M"], case["N"]
    a = 1.0 if case["rng"] == "big" else 0.28
    md0, md1 = a * rn(B, M, 256), a * rn(B, N, 256)
    z0, z1 = 3.0 * rn(B, M), 3.0 * rn(B, N)
    cnt = live_counts(case)
    jt, it = tie_pairs(case)
    t = {"zero_row": None, "jt": [], "it": []}
    for b in range(B):
        mb, nb = cnt[b]
        res0, res1 = set(), set()
        if b == 0 and case["ties"]:
            assert (mb, nb) == (M, N) and M >= 136 and N >= 260
            src_rows, src_cols = [M - 10 - k for k in range(4)], [N - 10 - k for k in range(4)]
            for (j1, j2), i in zip(jt, src_rows):
                md1[0, j1] = md1[0, j2] = md0[0, i] + 0.1 * a * rn(256)
                z1[0, j2] = z1[0, j1]
                t["jt"].append((i, j1, j2))
                res0.add(i), res1.update((j1, j2))
            for (i1, i2), j in zip(it, src_cols):
                md0[0, i2] = md0[0, i1]
                z0[0, i2] = z0[0, i1]
                md1[0, j] = md0[0, i1] + 0.1 * a * rn(256)
                t["it"].append((j, i1, i2))
                res1.add(j), res0.update((i1, i2))
        if b == 0 and mb >= 8:
            t["zero_row"] = mb // 2
            res0.add(mb // 2)
            if case["rng"] == "big":
                res0.add(mb // 2 + 1)
        free0 = torch.tensor([i for i in range(mb) if i not in res0], dtype=torch.long)
        free1 = torch.tensor([j for j in range(nb) if j not in res1], dtype=torch.long)
        k = min(len(free0), len(free1)) // 2
        if k:
            s0 = free0[torch.randperm(len(free0), generator=g)[:k]]
            s1 = free1[torch.randperm(len(free1), generator=g)[:k]]
            md1[b, s1] = md0[b, s0] + 0.1 * a * rn(k, 256)
            if case["matches"]:  # matchable keypoints, so that real matches pass the threshold
                z0[b, s0[: k // 2 + 1]] = z0[b, s0[: k // 2 + 1]].abs() + 1.0
                z1[b, s1[: k // 2 + 1]] = z1[b, s1[: k // 2 + 1]].abs() + 1.0
        for z, n, fr in ((z0, mb, free0), (z1, nb, free1)):
            if n >= 8 and len(fr) >= 3:
                z[b, fr[-1]], z[b, fr[-2]], z[b, fr[-3]] = 30.0, -30.0, -30.0
        if t["zero_row"] is not None and b == 0:
            md0[0, t["zero_row"]] = 0.0
            if case["rng"] == "big":
                md0[0, mb // 2 + 1, 7] = 64.0
        md0[b, mb:], md1[b, nb:] = 0.0, 0.0
    if case["rng"] == "tiny":
        s = 2.0 ** -12 / max(md0.abs().max().item(), md1.abs().max().item())
        md0, md1 = md0 * s, md1 * s
    t.update(md0=md0.contiguous(), md1=md1.contiguous(), z0=z0.contiguous(), z1=z1.contiguous(), counts=cnt)
    return t


# ------------------------------------------------------------------------------------ routes
def _src(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _one(pattern, text, what):
    m = re.search(pattern, text)
    assert m, f"{what}: the source no longer reads as /{pattern}/ -- update tests/assign_cases.py"
    return m


def parsed():
    """The constants of the assignment dispatch, read from the source text."""
    a, h3 = _src("assign.hip"), _src("assign_h3.hip")
    t = {"kSimTile": int(_one(r"constexpr int kSimTile = (\d+);", h3, "kSimTile").group(1)),
         "kAsMaxN": int(_one(r"constexpr int kAsMaxN = (\d+);", a, "kAsMaxN").group(1)),
         "kAsW": int(_one(r"constexpr int kAsW = (\d+);", a, "kAsW").group(1)),
         "CCH": int(_one(r"constexpr int CCH = (\d+);", a, "CCH").group(1))}
    _one(r'const bool fused = LG_ASSIGN_FUSED && !a\.Mb && N % 4 == 0 && N <= kAsMaxN && !getenv\("LG_ASSIGN_UNFUSED"\);', a,
         "fused condition")
    _one(r"const int k4 = \(N \+ 255\) / 256;\n\s*if \(k4 <= 1\) launch_assign_fused<1>\(a, s, nch, psum, st\);\n"
         r"\s*else if \(k4 <= 2\) launch_assign_fused<2>.*\n\s*else if \(k4 <= 4\) launch_assign_fused<4>.*\n"
         r"\s*else launch_assign_fused<8>", a, "K4 dispatch")
    _one(r"bool sim_h3_supported\(int M, int N\) \{ return M % 16 == 0 && N % 16 == 0 &&", h3, "sim_h3_supported")
    _one(r"if \(g\.B % 8 == 0\) \{", h3, "pair-per-XCD mapping")
    _one(r"if \(a\.Mb\) \{\n\s*if \(mode == 0\) hipLaunchKernelGGL\(\(sim_h3_kernel<0, true>\)", h3, "RAGGED dispatch")
    _one(r"\(a\.Mb && !a\.fixed\) \|\| \(!a\.Mb && a\.fixed\) \|\| !sim_h3_supported\(M, N\)", a, "assign_and_filter_h3 rejects")
    return t


def route_of(p, case):
    """The instantiation label a case runs."""
    N, counted = case["N"], case["counts"] is not None
    if case["route"] == "recomputed":
        assert case["M"] % 16 == 0 and N % 16 == 0 and (not counted or case["fixed"])
        return "h3_ragged" if counted else "h3"
    if counted or N % 4 or N > p["kAsMaxN"] or case["unfused"]:
        return "four_read"
    k4 = (N + 255) // 256
    return "K4=%d" % (1 if k4 <= 1 else 2 if k4 <= 2 else 4 if k4 <= 4 else 8)
