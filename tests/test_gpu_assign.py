"""The assignment head (dual softmax + mutual filter) in isolation, through the C-ABI entry `lg_assign`,
on both routes and against float64 -- needs an MI355X.

The forward goldens see these kernels after nine layers at 1e-3; here every case of assign_cases.CASES
runs alone on seeded md / z / counts, so a failure names the route, the instantiation and the shape.
The recomputed route (assign_h3.hip, the default eval route) runs from md; the materialised route
(assign.hip) runs once on a given fp32 sim (the kernels then see the reference's own input: d = 0, only
the fp32 bar e32 remains) and once from md through the bf16x6 GEMM.  Bars and their derivation:
assign_ref.py (none is taken from a kernel).  Beside the bars, exact checks that near-ties cannot
weaken: oracle.filter_matches on the la actually written reproduces m0 / m1 (scores to the 1-ulp expf
allowance), a run without la, a second run and a zero-padded (unpoisoned) run are bit-identical, planted
duplicates tie bit for bit, everything outside the defined blocks keeps its sentinel, a score equal to
the threshold is no match.  test_assign_host.py shows a CPU emulation of each route stays below half of
every bar and that eight deliberate mistakes are caught.

Measured on an MI355X when the tests were added, worst err / bar (la | dustbins | scores):
recomputed route (fp16x3, from md):
  h3_one_tile                0.191 | 0.111 | 0.019
  h3_tiles                   0.246 | 0.228 | 0.049
  h3_tiles_tiny              0.269 | 0.227 | 0.059
  h3_tiles_big               0.226 | 0.234 | 0.048
  h3_pair_per_xcd            0.243 | 0.219 | 0.070
  h3_ragged3                 0.195 | 0.217 | 0.055
  h3_ragged8                 0.217 | 0.217 | 0.063
materialised route: on a given sim | from md through bf16x6:
  mat_k4_1_min               0.109 | 0.090 | 0.004    0.013 | 0.090 | 0.008
  mat_k4_1                   0.343 | 0.212 | 0.155    0.400 | 0.212 | 0.120
  mat_k4_2                   0.339 | 0.203 | 0.174    0.366 | 0.203 | 0.145
  mat_k4_2_big               0.364 | 0.226 | 0.153    0.508 | 0.226 | 0.127
  mat_k4_4                   0.330 | 0.224 | 0.134    0.401 | 0.224 | 0.094
  mat_k4_8                   0.265 | 0.215 | 0.163    0.574 | 0.215 | 0.090
  mat_n1                     0.181 | 0.210 | 0.018    0.057 | 0.210 | 0.032
  mat_n255                   0.298 | 0.219 | 0.266    0.281 | 0.219 | 0.133
  mat_n2052                  0.280 | 0.216 | 0.122    0.304 | 0.216 | 0.097
  mat_unfused_260            0.404 | 0.203 | 0.365    0.366 | 0.203 | 0.161
  mat_unfused_2048           0.278 | 0.215 | 0.179    0.574 | 0.215 | 0.090
  mat_counts                 0.355 | 0.181 | 0.331    0.358 | 0.181 | 0.102
  mat_counts_fixed           0.346 | 0.211 | 0.305    0.303 | 0.211 | 0.102
  mat_one_sided_zero         0.350 | 0.198 | 0.283    0.340 | 0.198 | 0.098
  mat_one_sided_zero_fixed   0.345 | 0.220 | 0.267    0.619 | 0.220 | 0.105
Plane exponents seen: 0 at |md|max about 1 and at 2^-12 (the image is one-sided), 3 at 64.
Above half a bar: only bf16x6 runs -- mat_k4_2_big 0.51, mat_k4_8 = mat_unfused_2048 (the same similarity) 0.57,
mat_one_sided_zero_fixed 0.62.  That is the format, not the assignment kernels: the same cases on a given sim sit
at 0.27 - 0.36, DESIGN.md section 3 records bf16x6's own maximum over random operands as 3.1e-7 S = 0.65 * 2^-21 S,
and an entry that is no row's or column's match inherits up to 4 d (twice directly, once through each log-sum-exp,
whose weight sits on the match) against a bar of 4 d + e32.  The bars stay as derived.
"""
import ctypes
import functools

import pytest
import torch

import assign_cases as ac
import assign_ref as ar
import lgamd  # noqa: F401
from lightglue_amd import _lib

pytestmark = pytest.mark.gpu

RUNS = [(c["name"], s) for c in ac.CASES for s in (("md",) if c["route"] == "recomputed" else ("sim", "md"))]
NAMES = [c["name"] for c in ac.CASES]


@functools.lru_cache(maxsize=None)
def inputs(name):
    return ac.build_inputs(ac.BY_NAME[name])


@functools.lru_cache(maxsize=None)
def prepared(name, src):
    case = ac.BY_NAME[name]
    return case, inputs(name), ar.reference(case, inputs(name), src)


def _env(case, monkeypatch):
    monkeypatch.delenv("LG_ASSIGN_SIM_X6", raising=False)
    if case["unfused"]:
        monkeypatch.setenv("LG_ASSIGN_UNFUSED", "1")
    else:
        monkeypatch.delenv("LG_ASSIGN_UNFUSED", raising=False)


def run_assign(case, t, src, want_la=True, poison=1, th=ac.TH, override=None):
    """One lg_assign call on sentinel-filled outputs.  Returns (rc, args, outputs on the CPU)."""
    lib = _lib.load()
    B, M, N = case["B"], case["M"], case["N"]
    dev = {k: t[k].cuda() for k in ("md0", "md1", "z0", "z1")}
    a = _lib.LGAssignArgs()
    a.B, a.M, a.N = B, M, N
    a.route, a.threshold, a.poison = _lib.ASSIGN_ROUTES[case["route"]], th, poison
    a.z0, a.z1 = dev["z0"].data_ptr(), dev["z1"].data_ptr()
    if src == "sim":
        dev["sim"] = ar.sim_f32(t).contiguous().cuda()
        a.sim = dev["sim"].data_ptr()
    else:
        a.md0, a.md1 = dev["md0"].data_ptr(), dev["md1"].data_ptr()
    if case["counts"] is not None:  # as the caller states them: the entry point clamps and empties
        dev["Mb"] = torch.tensor([c[0] for c in case["counts"]], dtype=torch.int32).cuda()
        dev["Nb"] = torch.tensor([c[1] for c in case["counts"]], dtype=torch.int32).cuda()
        a.Mb, a.Nb, a.fixed, a.raw_counts = dev["Mb"].data_ptr(), dev["Nb"].data_ptr(), case["fixed"], case["raw"]
    out = dict(la=torch.full((B, M + 1, N + 1), ar.SENT_F, device="cuda") if want_la else None,
               m0=torch.full((B, M), ar.SENT_I, dtype=torch.long, device="cuda"),
               m1=torch.full((B, N), ar.SENT_I, dtype=torch.long, device="cuda"),
               s0=torch.full((B, M), ar.SENT_F, device="cuda"), s1=torch.full((B, N), ar.SENT_F, device="cuda"))
    for k, v in out.items():
        setattr(a, k, v.data_ptr() if v is not None else None)
    for k, v in (override or {}).items():
        setattr(a, k, v)
    nbytes = ctypes.c_size_t()
    _lib.check(lib.lg_assign_workspace_bytes(B, M, N, ctypes.byref(nbytes)), "lg_assign_workspace_bytes")
    ws = torch.empty(nbytes.value, dtype=torch.uint8, device="cuda")
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = lib.lg_assign(ctypes.byref(a), ws.data_ptr(), nbytes.value, stream)
    torch.cuda.synchronize()
    return rc, a, {k: (v.cpu() if v is not None else None) for k, v in out.items()}


def _bits(x):
    return x.view(torch.int32) if x.dtype == torch.float32 else x


def _same(a, b, keys, what):
    for k in keys:
        assert torch.equal(_bits(a[k]), _bits(b[k])), f"{what}: {k} differs"


# ---------------------------------------------------------------- against float64
@pytest.mark.parametrize("name,src", RUNS)
def test_assignment_matches_float64(name, src, monkeypatch):
    case, t, ref = prepared(name, src)
    _env(case, monkeypatch)
    rc, a, got = run_assign(case, t, src)
    _lib.check(rc, "lg_assign")
    ratios = ar.check(case, t, ref, got)
    print(f"ASSIGN {name} {src} " + " ".join(f"{k}={v:.3f}" for k, v in ratios.items()) + f" exp_md={a.exp_md} max_md={a.max_md:.6g}")
    if case["route"] == "recomputed":  # the exponent the bars were computed with is the one the planes carry
        assert a.exp_md == ref["E"] == {"one": 0, "tiny": 0, "big": 3}[case["rng"]]
        assert a.max_md == max(t["md0"].abs().max().item(), t["md1"].abs().max().item())
    else:
        assert a.exp_md == 0 and a.max_md == 0.0
    if case["ties"]:
        ar.ties_bitwise(t, got)
    assert max(ratios.values(), default=0.0) <= 1.0, f"{name}/{src}: {ratios} of the bars"


# ---------------------------------------------------------------- exact invariants
@pytest.mark.parametrize("name", NAMES)
def test_runs_are_bit_identical(name, monkeypatch):
    """la = null, a second run and a zero-padded (unpoisoned) run change no bit of what the contract defines --
    here everything, since the test fills the outputs with the entry point's own sentinels."""
    case, t = ac.BY_NAME[name], inputs(name)
    _env(case, monkeypatch)
    keys = ("m0", "m1", "s0", "s1")
    rc, _, base = run_assign(case, t, "md")
    _lib.check(rc, "lg_assign")
    for what, kw in (("second run", {}), ("zero-padded run", dict(poison=0)), ("la = null", dict(want_la=False))):
        rc, _, other = run_assign(case, t, "md", **kw)
        _lib.check(rc, "lg_assign")
        _same(base, other, keys + (("la",) if other["la"] is not None else ()), f"{name}, {what}")


@pytest.mark.parametrize("name,src", [("h3_tiles", "md"), ("mat_k4_2", "sim"), ("mat_counts", "md")])
def test_threshold_is_strict(name, src, monkeypatch):
    """A score equal to the threshold is no match (lightglue.py:331, `>`); one ulp below, it is."""
    case, t = ac.BY_NAME[name], inputs(name)
    _env(case, monkeypatch)
    rc, _, base = run_assign(case, t, src)
    _lib.check(rc, "lg_assign")
    i = int((base["m0"][0] > -1).nonzero()[0])
    j, th = int(base["m0"][0, i]), float(base["s0"][0, i])
    rc, _, at = run_assign(case, t, src, th=th)
    _lib.check(rc, "lg_assign")
    assert at["m0"][0, i] == -1 and at["m1"][0, j] == -1 and at["s0"][0, i] == base["s0"][0, i]
    keep = base["s0"][0] > th
    assert torch.equal(at["m0"][0][keep], base["m0"][0][keep]) and (at["m0"][0][~keep] <= -1).all()
    below = float(torch.nextafter(torch.tensor(th), torch.tensor(0.0)))
    rc, _, under = run_assign(case, t, src, th=below)
    _lib.check(rc, "lg_assign")
    assert under["m0"][0, i] == j and under["m1"][0, j] == i
    _same(base, at, ("la", "s0", "s1"), f"{name}: the threshold moved a value")


# ---------------------------------------------------------------- refused calls
@pytest.mark.parametrize("what,name,src,override", [
    ("M % 16 on the recomputed route", "h3_one_tile", "md", {"M": 15}),
    ("counts without fixed on the recomputed route", "h3_ragged3", "md", {"fixed": 0}),
    ("a sim on the recomputed route", "h3_one_tile", "md", {"sim": 0x10000}),
    ("fixed without counts", "mat_k4_1", "sim", {"fixed": 1}),
])
def test_refused_calls_write_nothing(what, name, src, override, monkeypatch):
    case, t = ac.BY_NAME[name], inputs(name)
    _env(case, monkeypatch)
    rc, _, got = run_assign(case, t, src, override=override)
    assert rc == _lib.LG_E_INVALID, f"{what}: rc = {rc}"
    assert (got["la"] == torch.tensor(ar.SENT_F)).all() and (got["s0"] == torch.tensor(ar.SENT_F)).all()
    assert (got["m0"] == ar.SENT_I).all() and (got["m1"] == ar.SENT_I).all()
