"""CPU self-checks of the kernel-level assignment tests (no GPU): lg_assign refuses bad arguments before
touching a device, every case still takes the kernel instantiation it was written for, the float64
reference holds the planted ties and the near-tie cap, a CPU emulation of each route's arithmetic stays
below half of every bar of assign_ref.py, and eight deliberate mistakes miss a bar or an exact check."""
import ctypes
import functools
import os
import subprocess

import pytest
import torch

import assign_cases as ac
import assign_ref as ar
import lgamd  # noqa: F401
from lightglue_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RUNS = [(c["name"], s) for c in ac.CASES for s in (("md",) if c["route"] == "recomputed" else ("sim", "md"))]


@functools.lru_cache(maxsize=None)
def inputs(name):
    return ac.build_inputs(ac.BY_NAME[name])


@functools.lru_cache(maxsize=None)
def prepared(name, src):
    case = ac.BY_NAME[name]
    return case, inputs(name), ar.reference(case, inputs(name), src)


# ---------------------------------------------------------------- 1. argument rejection
FAKE = 0x10000  # never dereferenced: every call below is refused by the argument checks


def _args(route="recomputed", B=2, M=32, N=48, **kw):
    a = _lib.LGAssignArgs()
    a.B, a.M, a.N = B, M, N
    a.route, a.threshold = _lib.ASSIGN_ROUTES[route], 0.1
    for f in ("md0", "md1", "z0", "z1", "m0", "m1", "s0", "s1", "la"):
        setattr(a, f, FAKE)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


@pytest.mark.parametrize("what,args", [
    ("M % 16 on the recomputed route", dict(M=40)),
    ("N % 16 on the recomputed route", dict(N=52)),
    ("counts without fixed on the recomputed route", dict(Mb=FAKE, Nb=FAKE)),
    ("a sim on the recomputed route", dict(sim=FAKE)),
    ("raw counts on the recomputed route", dict(Mb=FAKE, Nb=FAKE, fixed=1, raw_counts=1)),
    ("Mb without Nb", dict(route="materialised", Mb=FAKE)),
    ("fixed without counts", dict(route="materialised", fixed=1)),
    ("raw counts without counts", dict(route="materialised", raw_counts=1)),
    ("no md and no sim", dict(route="materialised", md0=None)),
    ("null z0", dict(route="materialised", z0=None)),
    ("null m1", dict(route="materialised", m1=None)),
    ("B = 0", dict(route="materialised", B=0)),
    ("N = 0", dict(route="materialised", N=0)),
    ("a bad route", dict(route="materialised", _route=7)),
    ("md0 off 16 bytes", dict(route="materialised", md0=FAKE + 4)),
    ("la too large", dict(route="materialised", B=64, M=8192, N=8192)),
])
def test_bad_arguments_are_refused_without_a_gpu(what, args):
    lib = _lib.load()
    bad_route = args.pop("_route", None)
    a = _args(**args)
    if bad_route is not None:
        a.route = bad_route
    assert lib.lg_assign(ctypes.byref(a), FAKE, 1 << 40, None) == _lib.LG_E_INVALID, what
    assert lib.lg_last_error()


def test_workspace_rules_without_a_gpu():
    lib = _lib.load()
    n = ctypes.c_size_t()
    assert lib.lg_assign_workspace_bytes(3, 272, 528, ctypes.byref(n)) == _lib.LG_OK
    rows_pad = (3 * (272 + 528) + 255) // 256 * 256 + 256
    assert n.value >= 2 * rows_pad * 256 * 2 + 3 * 272 * 528 * 4
    assert lib.lg_assign_workspace_bytes(0, 16, 16, ctypes.byref(n)) == _lib.LG_E_INVALID
    assert lib.lg_assign_workspace_bytes(1, 16, 16, None) == _lib.LG_E_INVALID
    lib.lg_assign_workspace_bytes(2, 32, 48, ctypes.byref(n))
    assert lib.lg_assign(ctypes.byref(_args()), FAKE, n.value - 1, None) == _lib.LG_E_WORKSPACE
    assert lib.lg_assign(ctypes.byref(_args()), None, n.value, None) == _lib.LG_E_WORKSPACE
    assert lib.lg_assign(ctypes.byref(_args()), FAKE + 16, n.value, None) == _lib.LG_E_INVALID  # not 256-byte aligned
    assert lib.lg_assign(None, FAKE, n.value, None) == _lib.LG_E_INVALID


def test_assign_args_struct_matches_the_header(tmp_path):
    hdr = os.path.join(ROOT, "include", "lightglue_mi355x.h")
    lines = ["#include <stdio.h>", "#include <stddef.h>", f'#include "{hdr}"', "int main(void) {",
             'printf("size %zu\\n", sizeof(lg_assign_args_t));',
             'printf("sent_f %.17g\\n", (double)LG_ASSIGN_SENTINEL_F);', 'printf("sent_i %d\\n", LG_ASSIGN_SENTINEL_I);',
             'printf("routes %d\\n", LG_ASSIGN_MATERIALISED * 10 + LG_ASSIGN_RECOMPUTED);']
    lines += [f'printf("{f} %zu\\n", offsetof(lg_assign_args_t, {f}));' for f, _ in _lib.LGAssignArgs._fields_]
    lines.append("return 0; }")
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    subprocess.run(["gcc", "-o", str(tmp_path / "layout"), str(src)], check=True)
    got = dict(ln.split() for ln in subprocess.run([str(tmp_path / "layout")], check=True, capture_output=True,
                                                   text=True).stdout.splitlines())
    assert int(got.pop("size")) == ctypes.sizeof(_lib.LGAssignArgs)
    assert float(got.pop("sent_f")) == ar.SENT_F and int(got.pop("sent_i")) == ar.SENT_I == _lib.ASSIGN_SENTINEL_I
    assert int(got.pop("routes")) == _lib.ASSIGN_ROUTES["materialised"] * 10 + _lib.ASSIGN_ROUTES["recomputed"]
    for f, _ in _lib.LGAssignArgs._fields_:
        assert int(got[f]) == getattr(_lib.LGAssignArgs, f).offset, f
    assert {"lg_assign", "lg_assign_workspace_bytes"} <= set(_lib.EXPORTED_SYMBOLS)
    assert _lib.load().lg_abi_version() == 12  # additive: the ABI version does not move


# ---------------------------------------------------------------- 2. routes
def test_cases_reach_their_routes():
    p = ac.parsed()
    T, W, CCH, MAXN = p["kSimTile"], p["kAsW"], p["CCH"], p["kAsMaxN"]
    for c in ac.CASES:
        assert ac.route_of(p, c) == c["expect"], c["name"]
        assert c["B"] * c["M"] * c["N"] <= 8 * 272 * 528, f"{c['name']}: keep the cases small"
    by = ac.BY_NAME
    ntm = lambda c: (c["M"] + T - 1) // T  # noqa: E731
    ntn = lambda c: (c["N"] + T - 1) // T  # noqa: E731
    assert (ntm(by["h3_one_tile"]), ntn(by["h3_one_tile"])) == (1, 1)
    c = by["h3_tiles"]
    assert (ntm(c), ntn(c)) == (2, 3) and c["M"] % T and c["N"] % T and c["B"] % 8
    c = by["h3_pair_per_xcd"]
    assert c["B"] % 8 == 0 and c["M"] % T == 0 and c["N"] % T == 16
    cnt = ac.live_counts(by["h3_ragged8"])
    assert by["h3_ragged8"]["B"] % 8 == 0 and (T, T + 1) in cnt and (T + 1, T) in cnt and (0, 0) in cnt and cnt[5] == (0, 0)
    assert any(mb <= T and nb <= T for mb, nb in cnt if mb) and any(mb % 16 and nb % 16 for mb, nb in cnt)
    assert any(mb % 16 and nb % 16 and mb > 1 for mb, nb in ac.live_counts(by["h3_ragged3"]))
    # the fused instantiations: every K4, the lane edge (N % 256 == 4, 252), N = kAsMaxN
    assert {c["expect"] for c in ac.CASES} >= {"h3", "h3_ragged", "K4=1", "K4=2", "K4=4", "K4=8", "four_read"}
    assert by["mat_k4_8"]["N"] == MAXN and by["mat_n2052"]["N"] > MAXN and by["mat_n2052"]["N"] % 4 == 0
    assert by["mat_n255"]["N"] % 4 and by["mat_n1"]["N"] == 1
    rows = CCH // W
    ms = {c["M"] for c in ac.CASES if c["route"] == "materialised"}
    assert {1, CCH - 1, CCH, CCH + 1, 2 * CCH + rows} <= ms
    # one-sided zeros in both orders, raw
    z = ac.live_counts(by["mat_one_sided_zero"])
    assert any(a and not b for a, b in z) and any(b and not a for a, b in z)
    # the planted ties: same wave block / lane, two waves, two tiles (recomputed); same lane, two lanes, two register
    # groups (fused); same wave, two waves of a chunk, two chunks (column ties)
    jt, it = ac.tie_pairs(by["h3_tiles"])
    blk = lambda j: (j // T, (j % T) // 64)  # noqa: E731
    assert blk(jt[0][0]) == blk(jt[0][1]) and blk(jt[2][0])[0] == blk(jt[2][1])[0] and blk(jt[2][0]) != blk(jt[2][1])
    assert jt[3][0] // T != jt[3][1] // T and it[3][0] // T != it[3][1] // T
    jt, it = ac.tie_pairs(by["mat_k4_2"])
    assert jt[0][0] // 4 == jt[0][1] // 4 and jt[1][0] // 256 == jt[1][1] // 256 and jt[3][0] // 256 != jt[3][1] // 256
    assert it[0][0] // rows == it[0][1] // rows and it[1][0] // CCH == it[1][1] // CCH and it[1][0] // rows != it[1][1] // rows
    assert it[2][0] // CCH != it[2][1] // CCH


# ---------------------------------------------------------------- 3. reference, ties, near-tie cap
@pytest.mark.parametrize("name,src", RUNS)
def test_reference_ties_and_near_tie_cap(name, src):
    case, t, ref = prepared(name, src)
    n = ar.assert_ties_decide(case, t, ref)
    assert n == (8 if case["ties"] else 0)
    assert ref["left_out"] <= 0.02, f"{name}: float64 leaves {ref['left_out']:.3%} of the rows / columns undecided"
    if case["matches"]:
        real = sum(int((p["m0"] > -1).sum()) for p in ref["pairs"])
        assert real >= max(1, min(case["M"], case["N"]) // 16), f"{name}: {real} matches above the threshold"
    E = ref["E"]
    if case["route"] == "recomputed":
        assert E == {"one": 0, "tiny": 0, "big": 3}[case["rng"]]
        mx = max(t["md0"].abs().max().item(), t["md1"].abs().max().item())
        assert {"one": 0.5 < mx < 2.5, "tiny": abs(mx - 2.0 ** -12) < 2.0 ** -30, "big": mx == 64.0}[case["rng"]]
    if t["zero_row"] is not None:
        assert not t["md0"][0, t["zero_row"]].any()


# ---------------------------------------------------------------- 4. the bars are reachable
@pytest.mark.parametrize("name,src", RUNS)
def test_emulation_meets_the_bars(name, src):
    case, t, ref = prepared(name, src)
    got = ar.emulate(case, t, src)
    ratios = ar.check(case, t, ref, got)
    print(f"ASSIGN-EMU {name} {src} " + " ".join(f"{k}={v:.3f}" for k, v in ratios.items()))
    assert max(ratios.values(), default=0.0) <= 0.5, f"{name}/{src}: emulation at {ratios} of the bars"
    if case["ties"]:
        ar.ties_bitwise(t, got)


# ---------------------------------------------------------------- 5. the checks notice mistakes
SENSITIVITY = {
    "drop_low_high": [("h3_tiles", "md")],
    "drop_last_tile": [("h3_tiles", "md")],
    "colstats_next_pair": [("h3_tiles", "md"), ("mat_k4_2", "sim")],
    "dead_cols_in_rowsum": [("h3_ragged3", "md"), ("mat_counts", "sim")],
    "last_index_ties": [("h3_tiles", "md"), ("mat_k4_2", "sim"), ("mat_counts", "md")],
    "merge_ge": [("h3_tiles", "md"), ("mat_k4_2", "sim")],
    "dustbin_at_Nb_fixed": [("h3_ragged3", "md"), ("mat_counts_fixed", "sim")],
    "threshold_ge": [("h3_tiles", "md"), ("mat_k4_2", "sim")],
}


def _caught(case, t, ref, got, **kw):
    try:
        ratios = ar.check(case, t, ref, got, **kw)
    except AssertionError:
        return True
    return max(ratios.values(), default=0.0) > 1.0


@pytest.mark.parametrize("wrong", ar.WRONG)
def test_checks_notice_a_wrong_kernel(wrong):
    assert set(SENSITIVITY) == set(ar.WRONG)
    for name, src in SENSITIVITY[wrong]:
        case, t, ref = prepared(name, src)
        kw = {}
        if wrong == "threshold_ge":  # a score that equals the threshold: > keeps it out, >= lets it in
            good = ar.emulate(case, t, src)
            i = int((good["m0"][0] > -1).nonzero()[0])
            kw = dict(th=float(good["s0"][0, i]), vs64=False)
            right = ar.emulate(case, t, src, th=kw["th"])
            assert right["m0"][0, i] == -1 and not _caught(case, t, ref, right, **kw)
        got = ar.emulate(case, t, src, wrong=wrong, **({"th": kw["th"]} if kw else {}))
        assert _caught(case, t, ref, got, **kw), f"{wrong} on {name}/{src}: the suite would not notice"
