"""The shapes that reach each shape-selected route of the training kernels, and the launcher
conditions that send them there.

The training path has no switches: which kernel runs follows from shape and alignment alone
(csrc/train.h).  The GPU tests (test_gpu_train.py, test_gpu_sg_train.py) take their cases from
here, and test_host.py::test_training_route_cases_reach_their_routes -- no GPU -- reads the
thresholds out of the launchers' source text and checks that every case still lies on the side of
each threshold its comment claims, so moving a threshold fails there and names the case to re-pick.

Measured on an MI355X when the cases were added (worst error / bar of the test that runs them):
  GEMM_CASES, bar 2e-6 sqrt(max(K, 64)) 8: x6_ragged_tile 0.12, x6_similarity 0.09,
    x6_dgrad_transposed_weight 0.16, x6_single_ktile 1e-5, x6_padded_rows 0.12, f32_unaligned_a 0.13,
    f32_beta_half 0.13, f32_dgrad_batched 0.21, f32_batched_beta_one 0.15 (2e4 before tgemm_x6
    declined it: the bf16x6 epilogue added batch 0's C to every batch)
  GEMM_EX, same bar: a1 0.25, b1_split 0.19 (column sums 0.03), b1_whole 0.19 (0.02),
    colsum_scalar 0.08 (0.03), res_x6 0.14, res_f32 0.10
  HEAD_DENSE, spread bar: 0.20 (gd0), 0.14 (final_proj.bias), 0.22 (final_proj.weight), 0.20 (matchability.bias)
  HEAD_NLL, spread bar: 0.22, 0.24 (final_proj.bias); the NLL terms 0.01, 0.05
  TRUNK_MULTIBLOCK, the trunk test's 2e-5 bar: 0.67 (cross_attn.to_qk.bias)
  SG_UNFUSED 0.61 (kenc.encoder.4.weight), SG_NOT_DEFERRED 0.54 (kenc.encoder.0.bias), the ragged test's bar
"""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cs566-project-lightglue_amd", "csrc")


def _gemm(name, route, why, ta, tb, batch, M, N, K, **kw):
    c = dict(name=name, route=route, why=why, ta=ta, tb=tb, batch=batch, M=M, N=N, K=K, alpha=0.75, beta=1.0, bias=True,
             a_offset=0, pad=0, nan_c=False)
    c.update(kw)
    return c


# tgemm through lg_train_gemm.  route: "x6" = gemm.hip's bf16x6 kernel (tgemm_x6 takes it), "f32" =
# tgemm_kernel on the f32 matrix cores (tgemm_x6 declines).
GEMM_CASES = [
    _gemm("x6_ragged_tile", "x6", "ta = 0, K % 16 == 0, aligned, beta = 1; M and N leave a partial 256 x 256 tile "
          "behind a full one", 0, 1, 1, 300, 520, 256),
    _gemm("x6_similarity", "x6", "the heads' md0 md1^T: batched (0, 1), K = 256, beta = 0 -- C must not be read",
          0, 1, 3, 70, 45, 256, alpha=1.0, beta=0.0, bias=False, nan_c=True),
    _gemm("x6_dgrad_transposed_weight", "x6", "(0, 0), batch 1, ldb == N: B is transposed into the workspace first",
          0, 0, 1, 257, 260, 512),
    _gemm("x6_single_ktile", "x6", "K == the k-tile: the pipeline's prologue and one compute step, one output entry",
          0, 1, 1, 1, 1, 16),
    _gemm("x6_padded_rows", "x6", "lda = K + 4, ldc = N + 4 (ld % 4 == 0 keeps the route): C's padding is not written",
          0, 1, 1, 300, 520, 256, pad=4),
    _gemm("f32_unaligned_a", "f32", "A's pointer is 4 bytes past a 16-byte boundary: tgemm_x6's al(A) fails",
          0, 1, 1, 300, 520, 256, a_offset=1),
    _gemm("f32_beta_half", "f32", "beta = 0.5 is neither 0 nor 1: the bf16x6 epilogue only adds a residual",
          0, 1, 1, 300, 520, 256, beta=0.5),
    _gemm("f32_dgrad_batched", "f32", "(0, 0) with batch 2: the workspace transpose is for batch 1 only (beta = 0, so "
          "that this alone decides)", 0, 0, 2, 257, 260, 512, beta=0.0, nan_c=True),
    _gemm("f32_batched_beta_one", "f32", "batch 3 with beta = 1: the bf16x6 epilogue's residual has no batch stride",
          0, 1, 3, 70, 45, 256),
]

# tgemm through lg_train_gemm_ex (the operands only the library's own calls pass)
GEMM_EX = {
    # ffn.0's forward: A = [X | message] read from two sources
    "a1": dict(M=300, N=512, K=512, K0=256),
    # ffn.0's weight gradient: B = [X | message] from two sources, the bias gradient from the same read of dY
    "b1_split": dict(M=512, N=512, K=1180, N0=256),  # tgemm_split: 2 chunks, 592 + 588
    "b1_whole": dict(M=512, N=512, K=300, N0=256),  # K < 1024: no split
    # M % 4 != 0: tgemm_x6t_kernel (the non-vector weight-gradient kernel), no split
    "colsum_scalar": dict(M=37, N=300, K=129),
    "res_x6": dict(M=200, N=136, K=256),  # the bf16x6 epilogue reads R
    "res_f32": dict(M=200, N=136, K=72),  # K % 16 != 0: the f32 route copies R into C first
    "refuse_a1": dict(M=200, N=136, K=72, K0=32),  # the two-source A exists on the bf16x6 route only
    "refuse_b1": dict(M=256, N=256, K=64, N0=100),  # N0 must be a multiple of the 128-wide tile
}

# (B, M, N) of the dense head (lg_head_forward + lg_head_backward) against the float64 oracle
HEAD_DENSE = [
    (2, 70, 1028),  # sim_lse fused QN = 2; 3 blocks of SLF_ROWS, the last partial; la_forward rows kernel
    (1, 40, 2052),  # sim_lse fused QN = 4
    (1, 40, 4100),  # N > 4096, N % 4 == 0: unfused sim_lse with the float4 column pass; la_forward generic
    (1, 40, 4102),  # N % 4 != 0: unfused sim_lse with the scalar column pass; la_forward generic
]
# (B, N) of the NLL head (lg_head_nll_forward + lg_head_nll_backward), M == N
HEAD_NLL = [
    (2, 1028),  # la_nll KC = 8, la_grad_gt IT = 2
    (1, 2052),  # la_nll KC = 16, la_grad_gt IT = 4
]

# the trunk at 1180 rows: every row-blocked reduction has several blocks and a partial last one
TRUNK_MULTIBLOCK = ({"n_layers": 1}, 2, 300, 290)
# (B, Nq, Nk) of the training attention beyond one 256-query block
ATTN_MULTIBLOCK = [(1, 300, 520), (2, 257, 1)]

# (B, M, N, layers, iters) of the SuperGlue training step
SG_UNFUSED = (1, 40, 2112, ["cross"], 5)  # N + 1 > 64 SKF_Q: unfused Sinkhorn forward and backward
SG_NOT_DEFERRED = (2, 33, 40, ["cross"], 130)  # iters > SKA_TMAX: fused, the backward not deferred


# ------------------------------------------------------------------ the launchers' thresholds
def _src(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _body(src, signature):
    """The text of the function whose definition starts with ``signature`` (up to its closing brace
    in column 0)."""
    i = src.index(signature)
    return src[i:src.index("\n}\n", i)]


def _one(pattern, text, what):
    m = re.search(pattern, text)
    assert m, f"{what}: the launcher no longer reads as /{pattern}/ -- update tests/train_route_cases.py"
    return m


def _ladder(body, macro, what):
    """[(bound or None, variant)] of an ``if (.. N <= b) MACRO(v); else if ..; else MACRO(v);`` ladder."""
    steps = [(int(b), int(v)) for b, v in re.findall(r"N <= (\d+)\) " + macro + r"\((\d+)\)", body)]
    last = _one(r"else " + macro + r"\((\d+)\)", body, what)
    assert steps, f"{what}: no N <= bound ladder of {macro} found"
    return steps + [(None, int(last.group(1)))]


def _pick(ladder, n):
    for bound, variant in ladder:
        if bound is None or n <= bound:
            return variant


def thresholds():
    """Every constant and ladder the cases depend on, parsed from train.hip / sg_train.hip / gemm.hip."""
    tr, sg, ge = _src("train.hip"), _src("sg_train.hip"), _src("gemm.hip")
    t = {}
    for name in ("LA_NMAX", "SLF_ROWS", "LSE_ROWS", "LN_ROWS", "PE_ROWS", "HVG_ROWS", "TB_W", "CS_TARGET_WG", "TG_BM",
                 "TG_BN", "X6_BN"):
        t[name] = int(_one(r"constexpr int [^;]*\b" + name + r" = (\d+)", tr, name).group(1))
    t["TG_BK"] = int(_one(r"#define LG_TG_BK (\d+)", tr, "LG_TG_BK").group(1))
    t["TB_KEYS"] = 32 * t["TB_W"]
    _one(r"TB_KEYS = 32 \* TB_W", tr, "TB_KEYS")
    for name in ("SKF_Q", "SKA_TMAX"):
        t[name] = int(_one(r"constexpr int [^;]*\b" + name + r" = (\d+)", sg, name).group(1))
    _one(r"N1 <= 64 \* SKF_Q", _body(sg, "static bool skf_ok("), "skf_ok")
    _one(r"iters <= SKA_TMAX", _body(sg, "static bool sk_defer("), "sk_defer")
    tile = _one(r"#define LG_GEMM_TILE (\d+), (\d+), (\d+)", ge, "LG_GEMM_TILE")
    t["X6_TILE_M"], t["X6_TILE_N"], t["X6_TILE_K"] = (int(v) for v in tile.groups())
    # sim_lse: fused while N % 4 == 0 && N <= bound, QN by the ladder
    b = _body(tr, "hipError_t sim_lse(")
    t["SLF_NMAX"] = int(_one(r"N % 4 == 0 && N <= (\d+)", b, "sim_lse's fused condition").group(1))
    t["SLF_QN"] = _ladder(b, "LG_SLF", "sim_lse")
    _one(r"if \(N % 4 == 0 && [^\n]*\n\s*hipLaunchKernelGGL\(sim_lse_col_part4_kernel", b, "sim_lse's unfused float4 pass")
    t["NLL_KC"] = _ladder(_body(tr, "hipError_t la_nll("), "LG_NLL_ROWS", "la_nll")
    b = _body(tr, "hipError_t la_grad_gt(")
    t["GT_IT"] = _ladder(b, "LG_GT_SIM", "la_grad_gt")
    _one(r"const bool vec = N % 4 == 0", b, "la_grad_gt's vector condition")
    _one(r"if \(N <= LA_NMAX\)\s*\n\s*hipLaunchKernelGGL\(la_forward_rows_kernel", _body(tr, "hipError_t la_forward("),
         "la_forward")
    t["ATTN_QBLOCK"] = int(_one(r"cdiv\(a\.Nq, (\d+)\)", _body(tr, "hipError_t tattn_forward("), "tattn_forward").group(1))
    _one(r"cdiv\(a\.Nk, TB_KEYS\)", _body(tr, "hipError_t tattn_backward("), "tattn_backward")
    # tgemm_x6: ta == 0, K a multiple of the k-tile, beta in {0, 1}, 16-byte-aligned operands, batch 1 residuals
    b = _body(tr, "static bool tgemm_x6(")
    m = _one(r"if \(ta \|\| g\.K < (\d+) \|\| g\.K % (\d+) \|\| \(g\.beta != 0\.f && g\.beta != 1\.f\)\) return false", b,
             "tgemm_x6's first condition")
    t["X6_KMIN"], t["X6_KMOD"] = int(m.group(1)), int(m.group(2))
    m = _one(r"\(uintptr_t\)ptr % (\d+) == 0\) && ld % (\d+) == 0 && sb % (\d+) == 0", b, "tgemm_x6's alignment")
    t["X6_PTR"], t["X6_LD"] = int(m.group(1)), int(m.group(2))
    _one(r"g\.beta != 0\.f && g\.batch != 1 && !g\.R\) return false", b, "tgemm_x6's batched-residual condition")
    _one(r"g\.batch != 1 \|\| g\.ldb != g\.N \|\| !ws", b, "tgemm_x6's transposed-B condition")
    # tgemm_split: split when the output has few tiles and K is long
    b = _body(tr, "int tgemm_split(")
    m = _one(r"tiles < (\d+) && K >= (\d+)", b, "tgemm_split's condition")
    t["SPLIT_TILES"], t["SPLIT_KMIN"] = int(m.group(1)), int(m.group(2))
    m = _one(r"\((\d+) \+ tiles - 1\) / tiles, K / (\d+)\)", b, "tgemm_split's count")
    t["SPLIT_TARGET"], t["SPLIT_KPER"] = int(m.group(1)), int(m.group(2))
    b = _body(tr, "hipError_t tgemm(")
    _one(r"g\.B1 && \(g\.batch != 1 \|\| g\.N0 % X6_BN", b, "tgemm's B1 condition")
    _one(r"const bool vec = g\.M % 4 == 0 && g\.N % 4 == 0", b, "tgemm's vector weight-gradient condition")
    return t


def cdiv(a, b):
    return (a + b - 1) // b


def tgemm_split(t, M, N, K, batch=1):
    """train.hip's tgemm_split on the parsed constants: (splits, chunk length)."""
    tiles = cdiv(M, t["TG_BM"]) * cdiv(N, t["TG_BN"]) * batch
    ks = 1
    if tiles < t["SPLIT_TILES"] and K >= t["SPLIT_KMIN"]:
        ks = max(min(cdiv(t["SPLIT_TARGET"], tiles), K // t["SPLIT_KPER"]), 1)
    kchunk = cdiv(cdiv(K, ks), t["TG_BK"]) * t["TG_BK"]
    return max(cdiv(K, kchunk), 1), kchunk


def colsum_chunks(t, rows, cols):
    """train.hip's cs_chunks: row chunks of the first colsum pass."""
    return max(1, min(cdiv(rows, 16), t["CS_TARGET_WG"] // cdiv(cols, 64)))


def x6_takes(t, c):
    """tgemm_x6's decision for a GEMM_CASES entry (R, A1 absent; the workspace is large enough)."""
    if c["ta"] or c["K"] < t["X6_KMIN"] or c["K"] % t["X6_KMOD"] or c["beta"] not in (0.0, 1.0):
        return False
    if c["beta"] != 0.0 and c["batch"] != 1:
        return False
    if (4 * c["a_offset"]) % t["X6_PTR"] or (c["K"] + c["pad"]) % t["X6_LD"]:
        return False
    if not c["tb"] and c["batch"] != 1:
        return False
    return True


def sim_lse_route(t, N):
    if N % 4 == 0 and N <= t["SLF_NMAX"]:
        return f"fused{_pick(t['SLF_QN'], N)}"
    return "vector" if N % 4 == 0 else "scalar"
