"""CPU-only checks: the C-ABI library loads and exports what include/*.h declares, the drop-in
module keeps the reference's config keys and state-dict schema, and the host helpers behave."""
import ctypes
import glob
import os
import re

import numpy as np
import pytest
import torch

import lgamd  # noqa: F401
from lightglue_amd import _lib
from lightglue_amd.weights import DEFAULT_CONF, state_dict_schema, synthetic_pair, synthetic_state_dict

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared_symbols():
    syms = set()
    for h in glob.glob(os.path.join(ROOT, "include", "*.h")):
        src = open(h).read()
        src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
        syms |= set(re.findall(r"\b((?:lg|sp|sg)_[a-z_0-9]+)\s*\(", src))
    return syms


def test_library_loads_and_exports_every_declared_symbol():
    lib = _lib.load()
    declared = declared_symbols()
    assert declared, "no declarations found"
    for s in sorted(declared):
        assert hasattr(lib, s), f"{s} declared in include/ but not exported"
    assert declared == set(_lib.EXPORTED_SYMBOLS)
    assert lib.lg_abi_version() == _lib.ABI_VERSION


def test_ctypes_structs_match_header_layout(tmp_path):
    """Every field offset and struct size of the ctypes mirrors equals what a C compiler makes of
    include/lightglue_mi355x.h (gcc on a generated offsetof table)."""
    import subprocess

    structs = {"lg_config_t": _lib.LGConfig, "lg_inputs_t": _lib.LGInputs, "lg_outputs_t": _lib.LGOutputs,
               "sp_config_t": _lib.SPConfig, "sp_inputs_t": _lib.SPInputs, "sp_outputs_t": _lib.SPOutputs,
               "sg_config_t": _lib.SGConfig, "sg_inputs_t": _lib.SGInputs, "sg_outputs_t": _lib.SGOutputs}
    lines = ["#include <stdio.h>", "#include <stddef.h>", f'#include "{os.path.join(ROOT, "include", "lightglue_mi355x.h")}"',
             f'#include "{os.path.join(ROOT, "include", "superpoint_mi355x.h")}"',
             f'#include "{os.path.join(ROOT, "include", "superglue_mi355x.h")}"', "int main(void) {"]
    for cname, py in structs.items():
        lines.append(f'printf("{cname} size %zu\\n", sizeof({cname}));')
        for f, _ in py._fields_:
            lines.append(f'printf("{cname} {f} %zu\\n", offsetof({cname}, {f}));')
    lines += ["return 0; }"]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-o", str(exe), str(src)], check=True)
    got = {}
    for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines():
        c, f, v = line.split()
        got[(c, f)] = int(v)
    for cname, py in structs.items():
        assert got[(cname, "size")] == ctypes.sizeof(py), cname
        for f, _ in py._fields_:
            assert got[(cname, f)] == getattr(py, f).offset, (cname, f)


def test_error_path_without_gpu_reports_message():
    lib = _lib.load()
    b = ctypes.c_size_t()
    assert lib.lg_filter_workspace_bytes(2, 10, 12, ctypes.byref(b)) == 0 and b.value > 0
    rc = lib.lg_filter_matches(None, 1, 1, 1, 0.0, None, None, None, None, None, 0, None)
    assert rc == _lib.LG_E_INVALID
    assert b"null" in lib.lg_last_error()


def test_module_schema_matches_reference_schema():
    from lightglue_amd import LightGlue

    for conf in ({}, {"add_scale_ori": True}, {"input_dim": 128}, {"n_layers": 3}):
        m = LightGlue(conf)
        sd = m.state_dict()
        schema = state_dict_schema(conf)
        assert list(sd.keys()) == [n for n, _ in schema]
        for n, shape in schema:
            assert tuple(sd[n].shape) == tuple(shape), n


def test_default_conf_keys_match_reference():
    # lightglue.py:341-361
    assert set(DEFAULT_CONF) == {
        "name", "input_dim", "add_scale_ori", "descriptor_dim", "n_layers", "num_heads", "flash", "mp",
        "depth_confidence", "width_confidence", "filter_threshold", "checkpointed", "weights",
        "weights_from_version", "loss",
    }


def test_checkpoint_key_renames(tmp_path):
    """Old 'self_attn.{i}' / 'cross_attn.{i}' keys are renamed like lightglue.py:424-429."""
    from lightglue_amd import LightGlue

    sd = synthetic_state_dict({}, seed=3)
    old = {}
    for k, v in sd.items():
        k2 = re.sub(r"^transformers\.(\d+)\.self_attn", r"self_attn.\1", k)
        k2 = re.sub(r"^transformers\.(\d+)\.cross_attn", r"cross_attn.\1", k2)
        old[k2] = torch.from_numpy(v)
    p = tmp_path / "w.pth"
    torch.save(old, p)
    m = LightGlue({"weights": str(p)})
    got = m.state_dict()
    for k, v in sd.items():
        assert torch.equal(got[k], torch.from_numpy(v)), k


def test_forward_refuses_cpu_inputs():
    from lightglue_amd import LightGlue

    m = LightGlue({})
    data = {k: torch.from_numpy(v) for k, v in synthetic_pair(B=1, M=8, seed=0).items()}
    with pytest.raises((RuntimeError, AssertionError)):
        m(data)


def test_assignment_helpers_refuse_cpu():
    from lightglue_amd import filter_matches, log_optimal_transport

    with pytest.raises(RuntimeError):
        filter_matches(torch.zeros(1, 3, 3), 0.1)
    with pytest.raises(RuntimeError):
        log_optimal_transport(torch.zeros(1, 3, 3), 1.0, 3)


def test_synthetic_recipes_are_deterministic():
    a = synthetic_state_dict({}, seed=0)
    b = synthetic_state_dict({}, seed=0)
    assert all(np.array_equal(a[k], b[k]) for k in a)
    p, q = synthetic_pair(B=2, M=20, N=30, seed=1), synthetic_pair(B=2, M=20, N=30, seed=1)
    assert all(np.array_equal(p[k], q[k]) for k in p)
    assert p["keypoints1"].shape == (2, 30, 2)
    np.testing.assert_allclose(np.linalg.norm(p["descriptors1"], axis=-1), 1.0, atol=1e-5)


def test_superpoint_module_schema_matches_reference_schema():
    """lightglue_amd.SuperPoint registers the reference's conv modules (superpoint.py:174-196), so
    its state dict has the recipe schema's keys, order and shapes for every head combination."""
    from lightglue_amd.sp_weights import SP_DEFAULT_CONF, superpoint_schema
    from lightglue_amd.superpoint import SuperPoint

    for conf in ({}, {"has_detector": False, "sparse_outputs": False}, {"has_descriptor": False, "sparse_outputs": False}):
        sd = SuperPoint(conf).state_dict()
        schema = superpoint_schema(conf)
        assert list(sd.keys()) == [n for n, _ in schema]
        for n, shape in schema:
            assert tuple(sd[n].shape) == tuple(shape), n
    assert set(SP_DEFAULT_CONF) == {  # superpoint.py:153-169 + base_model.py:54-59
        "name", "trainable", "freeze_batch_normalization", "timeit", "has_detector", "has_descriptor",
        "descriptor_dim", "sparse_outputs", "dense_outputs", "nms_radius", "refinement_radius",
        "detection_threshold", "max_num_keypoints", "max_num_keypoints_val", "force_num_keypoints",
        "randomize_keypoints_training", "remove_borders", "legacy_sampling"}


def test_superpoint_registered_in_pipeline():
    from lightglue_amd import pipeline
    from lightglue_amd.superpoint import SuperPoint

    for name in ("gluefactory_nonfree.superpoint", "extractors.superpoint", "superpoint"):
        assert pipeline.get_model(name) is SuperPoint


def test_superpoint_cpu_input_raises():
    from lightglue_amd.superpoint import SuperPoint

    with pytest.raises(RuntimeError, match="HIP device"):
        SuperPoint({})({"image": torch.zeros(1, 1, 64, 64)})


def test_superglue_module_schema_matches_reference_schema():
    """The parameter containers' state dict is the reference's (superglue.py:63-139,239-247)."""
    from lightglue_amd import SuperGlue
    from lightglue_amd.sg_weights import superglue_schema

    for conf in ({}, {"use_scores": False, "GNN_layers": ["cross", "self"]}, {"keypoint_encoder": [16, 64]}):
        sd = SuperGlue(conf).state_dict()
        schema = superglue_schema(conf)
        assert list(sd.keys()) == [n for n, _, _ in schema]
        for n, shape, _ in schema:
            assert tuple(sd[n].shape) == tuple(shape), n


def test_superglue_registry_and_cpu_inputs_raise():
    import torch

    from lightglue_amd import SuperGlue
    from lightglue_amd.pipeline import get_model

    assert get_model("gluefactory_nonfree.superglue") is SuperGlue and get_model("superglue") is SuperGlue
    m = SuperGlue({"GNN_layers": ["self"]}).eval()
    view = {"image": torch.zeros(1, 1, 48, 64)}
    data = {"view0": view, "view1": view, "keypoints0": torch.rand(1, 5, 2) * 40,
            "keypoints1": torch.rand(1, 6, 2) * 40, "descriptors0": torch.rand(1, 5, 256),
            "descriptors1": torch.rand(1, 6, 256), "keypoint_scores0": torch.rand(1, 5),
            "keypoint_scores1": torch.rand(1, 6)}
    with pytest.raises(RuntimeError, match="HIP device"):
        m(data)
    # empty view: the reference's early return (superglue.py:257-264), int32 matches
    out = m({**data, "keypoints1": torch.zeros(1, 0, 2), "descriptors1": torch.zeros(1, 0, 256),
             "keypoint_scores1": torch.zeros(1, 0)})
    assert out["matches0"].dtype == torch.int32 and (out["matches0"] == -1).all() and out["matches1"].shape == (1, 0)
    with pytest.raises(ValueError):
        SuperGlue({"GNN_layers": ["self", "both"]})


def test_bench_training_ground_truth_is_one_to_one():
    """bench.py --workload train*: the seeded ground truth of the synthetic pairs is one-to-one,
    consistent across gt_matches0 / gt_matches1 / gt_assignment, and leaves about a third unmatched;
    the training flop model counts the forward linears three times (y, dx, dW)."""
    import bench

    d = bench.gpu_pairs(3, 96, 256, 1, torch.device("cpu"))
    g = bench.gpu_ground_truth(d, 7)
    m0, m1, a = g["gt_matches0"], g["gt_matches1"], g["gt_assignment"]
    b, i = torch.nonzero(m0 > -1, as_tuple=True)
    assert (m1[b, m0[b, i]] == i).all()
    b, j = torch.nonzero(m1 > -1, as_tuple=True)
    assert (m0[b, m1[b, j]] == j).all()
    assert int(a.sum()) == int((m0 > -1).sum()) == int((m1 > -1).sum())
    assert (a.sum(2) <= 1).all() and (a.sum(1) <= 1).all()
    frac = float((m0 > -1).float().mean())
    assert 0.45 < frac < 0.8
    assert bench.train_flops_per_pair(2048) > 3 * 9 * 76 * 2048 * 256 * 256


def test_bench_dump_outputs_formats_budget_and_sample(tmp_path, monkeypatch):
    """bench.py --dump-outputs: every output becomes one <name>.npy in float32 (integers as float64,
    exact); an array over its share of the byte budget is stored as the fixed seeded sample of its
    flattened entries, so two dumps of equal outputs are equal file for file."""
    import bench

    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 4 * 4000)  # 4 outputs -> 1000 float32 entries each
    g = torch.Generator().manual_seed(5)
    big = torch.randn(3, 41, 37, generator=g)
    out = {"matches0": torch.arange(-1, 23).reshape(2, 12), "scores": torch.rand(2, 12, generator=g, dtype=torch.float64),
           "log_assignment": big, "ragged": [big[0, :5, :7], big[1, :3, :2]], "note": "skipped"}
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), out)
    files = sorted(os.listdir(tmp_path / "a"))
    assert files == ["log_assignment.npy", "matches0.npy", "ragged.npy", "scores.npy"]
    a = {f[:-4]: np.load(tmp_path / "a" / f) for f in files}
    assert a["matches0"].dtype == np.float64 and (a["matches0"] == out["matches0"].numpy()).all()
    assert a["scores"].dtype == np.float64 and a["scores"].shape == (2, 12)
    assert a["ragged"].dtype == np.float32 and a["ragged"].shape == (5 * 7 + 3 * 2,)
    idx = bench.dump_sample_indices(big.numel(), 1000)
    assert a["log_assignment"].dtype == np.float32 and a["log_assignment"].shape == (1000,)
    assert (a["log_assignment"] == big.reshape(-1)[idx].numpy()).all()
    assert (idx[1:] >= idx[:-1]).all() and 0 <= int(idx[0]) and int(idx[-1]) < big.numel()
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in files) <= 4 * 4000 + 4 * 128
    for f in files:
        assert (tmp_path / "a" / f).read_bytes() == (tmp_path / "b" / f).read_bytes()


def test_layer_slices_gradient_matches_indexing():
    """lightglue._LayerSlices (loss(): the per-layer head inputs) gives the same slices and the same
    [B, L, M, D] gradient as indexing rd[:, i], including layers whose slice gets no gradient."""
    import torch
    from lightglue_amd.lightglue import _LayerSlices

    g = torch.Generator().manual_seed(3)
    rd = torch.randn(2, 4, 5, 3, generator=g, dtype=torch.float64)
    r = [torch.randn(2, 5, 3, generator=g, dtype=torch.float64) for _ in range(4)]
    a = rd.clone().requires_grad_()
    sl = _LayerSlices.apply(a)
    assert all(s.is_contiguous() and torch.equal(s, rd[:, i]) for i, s in enumerate(sl))
    sum((sl[i] * r[i]).sum() * (i + 1) for i in (0, 1, 3)).backward()  # layer 2 unused
    b = rd.clone().requires_grad_()
    sum((b[:, i] * r[i]).sum() * (i + 1) for i in (0, 1, 3)).backward()
    assert torch.equal(a.grad, b.grad)


def test_env_switches_are_documented():
    """Every environment variable the library reads (getenv("...") in csrc) or the package reads
    (os.environ / os.getenv in its *.py) is a row of DESIGN.md's table "Run-time switches the library
    reads", and the table lists nothing else: an experiment's switch cannot stay behind unrecorded."""
    pkg = os.path.join(ROOT, "cs566-project-lightglue_amd")
    read = set()
    for ext in ("hip", "cpp", "h"):
        for f in glob.glob(os.path.join(pkg, "csrc", "*." + ext)):
            read |= set(re.findall(r'getenv\(\s*"(\w+)"\s*\)', open(f).read()))
    for f in glob.glob(os.path.join(pkg, "*.py")):
        src = open(f).read()
        read |= set(re.findall(r'os\.environ(?:\.get|\.setdefault|\.pop)?[\[(]\s*"(\w+)"', src))
        read |= set(re.findall(r'os\.getenv\(\s*"(\w+)"', src))
        read |= set(re.findall(r'"(\w+)"\s+(?:not\s+)?in\s+os\.environ', src))
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    head = "**Run-time switches the library reads.**"
    assert design.count(head) == 1
    rows = []
    for line in design[design.index(head):].split("\n")[1:]:
        if line.startswith("|"):
            rows.append(line)
        elif rows:
            break  # the table ends at the first line after it that is not a row
    documented = {m.group(1) for m in (re.match(r"\|\s*`(\w+)`\s*\|", r) for r in rows[2:]) if m}
    assert len(documented) == len(rows) - 2, "a row of the table does not start with one `NAME`"
    assert read, "found no environment reads: the patterns no longer match the source"
    assert read == documented, (sorted(read - documented), sorted(documented - read))


def test_training_route_cases_reach_their_routes():
    """The training kernels pick their route by shape alone, so the GPU tests reach a route only
    through their shapes (tests/train_route_cases.py).  This reads every threshold out of the
    launchers' source text and checks that each case lies on the side its comment claims; after a
    threshold moves it fails and names the case to re-pick.  Constants only: no compiled output."""
    import train_route_cases as rc

    t = rc.thresholds()
    # ---- tgemm: the bf16x6 route and its fallbacks
    for c in rc.GEMM_CASES:
        assert rc.x6_takes(t, c) == (c["route"] == "x6"), f"GEMM_CASES {c['name']}: re-pick ({c['why']})"
    by = {c["name"]: c for c in rc.GEMM_CASES}
    c = by["x6_ragged_tile"]
    for dim, tile in ((c["M"], t["X6_TILE_M"]), (c["N"], t["X6_TILE_N"])):
        assert dim > tile and dim % tile, "x6_ragged_tile: M and N need a full tile and a partial one"
    assert by["x6_single_ktile"]["K"] == t["X6_TILE_K"] == t["X6_KMOD"], "x6_single_ktile: K must be one k-tile"
    assert by["x6_padded_rows"]["pad"] % t["X6_LD"] == 0 and by["x6_padded_rows"]["pad"] > 0
    for fb, x6 in (("f32_unaligned_a", "x6_ragged_tile"), ("f32_beta_half", "x6_ragged_tile"),
                   ("f32_dgrad_batched", "x6_dgrad_transposed_weight"), ("f32_batched_beta_one", "x6_similarity")):
        assert [by[fb][k] for k in "MNK"] == [by[x6][k] for k in "MNK"], f"{fb}: same shape as {x6}"
    ex = rc.GEMM_EX
    s = ex["a1"]
    assert s["K"] % t["X6_KMOD"] == 0 and 0 < s["K0"] < s["K"] and s["K0"] % t["X6_KMOD"] == 0, "GEMM_EX a1: off bf16x6"
    s = ex["b1_split"]
    ks, kchunk = rc.tgemm_split(t, s["M"], s["N"], s["K"])
    assert ks >= 2 and s["K"] % kchunk, f"GEMM_EX b1_split: {ks} chunks of {kchunk}: need a split with a partial last chunk"
    nb = ctypes.c_size_t()  # the workspace entry covers the split's partials and their column-sum partials
    assert _lib.load().lg_train_gemm_workspace_bytes(s["M"], s["N"], s["K"], 1, ctypes.byref(nb)) == 0
    assert nb.value >= 4 * ks * s["M"] * (s["N"] + 1)
    assert rc.tgemm_split(t, ex["b1_whole"]["M"], ex["b1_whole"]["N"], ex["b1_whole"]["K"])[0] == 1, "GEMM_EX b1_whole splits"
    for k in ("b1_split", "b1_whole"):
        assert ex[k]["M"] % 4 == 0 and ex[k]["N"] % 4 == 0 and ex[k]["N0"] % t["X6_BN"] == 0, f"GEMM_EX {k}: not the vector kernel"
    assert ex["colsum_scalar"]["M"] % 4 or ex["colsum_scalar"]["N"] % 4, "GEMM_EX colsum_scalar takes the vector kernel"
    assert ex["res_x6"]["K"] % t["X6_KMOD"] == 0 and ex["res_x6"]["K"] >= t["X6_KMIN"], "GEMM_EX res_x6: off bf16x6"
    assert ex["res_f32"]["K"] % t["X6_KMOD"], "GEMM_EX res_f32: on bf16x6"
    assert ex["refuse_a1"]["K"] % t["X6_KMOD"], "GEMM_EX refuse_a1: bf16x6 would take it"
    assert ex["refuse_b1"]["N0"] % t["X6_BN"], "GEMM_EX refuse_b1: the vector kernel would take it"
    # ---- assignment head
    want = ["fused2", "fused4", "vector", "scalar"]
    assert [rc.sim_lse_route(t, n) for _, _, n in rc.HEAD_DENSE] == want, "HEAD_DENSE: sim_lse routes moved"
    assert [n > t["LA_NMAX"] for _, _, n in rc.HEAD_DENSE] == [False, False, True, True], "HEAD_DENSE: la_forward routes moved"
    b, m, n = rc.HEAD_DENSE[0]
    assert m > t["SLF_ROWS"] and m % t["SLF_ROWS"], "HEAD_DENSE[0]: M needs several SLF_ROWS blocks, the last partial"
    assert all(m % t["LSE_ROWS"] for _, m, _ in rc.HEAD_DENSE[2:]), "HEAD_DENSE: unfused cases need a partial LSE_ROWS block"
    r = b * (m + n)
    assert r > t["HVG_ROWS"] and r % t["HVG_ROWS"], "HEAD_DENSE[0]: head_vec_grads needs several blocks, the last partial"
    assert [rc._pick(t["NLL_KC"], n) for _, n in rc.HEAD_NLL] == [8, 16], "HEAD_NLL: la_nll variants moved"
    assert [rc._pick(t["GT_IT"], n) for _, n in rc.HEAD_NLL] == [2, 4], "HEAD_NLL: la_grad_gt variants moved"
    assert all(n % 4 == 0 and n <= t["LA_NMAX"] for _, n in rc.HEAD_NLL), "HEAD_NLL: off the vector kernels"
    # ---- trunk and attention
    conf, b, m, n = rc.TRUNK_MULTIBLOCK
    r = b * (m + n)
    for name in ("LN_ROWS", "PE_ROWS"):
        assert r > 2 * t[name] and r % t[name], f"TRUNK_MULTIBLOCK: {name} needs several blocks, the last partial"
    for out_rows, out_cols in ((768, 256), (256, 256), (512, 512), (256, 512)):  # the trunk's weight gradients
        ks, kchunk = rc.tgemm_split(t, out_rows, out_cols, r)
        assert ks >= 2 and r % kchunk, f"TRUNK_MULTIBLOCK: the {out_rows} x {out_cols} weight gradient is not split unevenly"
    assert rc.colsum_chunks(t, rc.cdiv(r, t["LN_ROWS"]), 512) > 1, "TRUNK_MULTIBLOCK: lngelu_bwd's colsum is one chunk"
    assert min(m, n) > max(t["ATTN_QBLOCK"], t["TB_KEYS"]), "TRUNK_MULTIBLOCK: attention within one block"
    (_, q0, k0), (_, q1, k1) = rc.ATTN_MULTIBLOCK
    assert q0 > t["ATTN_QBLOCK"] and k0 > 2 * t["TB_KEYS"], "ATTN_MULTIBLOCK[0]: within one query / key block"
    assert q1 == t["ATTN_QBLOCK"] + 1 and k1 == 1, "ATTN_MULTIBLOCK[1]: one row into the second query block, one key"
    # ---- SuperGlue training Sinkhorn
    fused_max = 64 * t["SKF_Q"]
    assert rc.SG_UNFUSED[2] + 1 > fused_max, "SG_UNFUSED: still fused"
    assert rc.SG_UNFUSED[4] <= t["SKA_TMAX"]
    assert rc.SG_NOT_DEFERRED[2] + 1 <= fused_max and rc.SG_NOT_DEFERRED[4] > t["SKA_TMAX"], "SG_NOT_DEFERRED: deferred or unfused"
