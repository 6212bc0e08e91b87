"""Shared inputs and CPU references of the ragged SuperGlue / Sinkhorn tests (test_sg_ragged_host.py,
test_gpu_sg_ragged.py).

A ragged case is ``B`` pairs at capacities ``M``, ``N``; pair ``b`` has ``counts[b] = (n0, n1)`` real
points, stored first.  The reference of pair ``b`` is the CPU oracle on that pair alone at its own
sizes (``oracle/superglue_ref.py``, ``oracle.log_optimal_transport``); ``to_capacity`` lays the
per-pair results out in the capacity frame the library returns:

* ``matches0/1`` -1 and ``matching_scores0/1`` 0 on padded points;
* ``sinkhorn_cost`` and the GNN descriptors 0 outside the pair's block;
* ``log_assignment`` [M+1, N+1]: the real block at ``i < n0, j < n1``, the dustbin column at index N
  (``i < n0``), the dustbin row at index M (``j < n1``), the corner [M, N], every other entry -inf;
* a pair with ``n0 == 0`` or ``n1 == 0`` (the reference's empty branch, superglue.py:257-264): no
  matches, zeros, ``log_assignment`` -inf except [M, N] = 0.

Every reference is computed once per process and never modified."""
import functools

import numpy as np
import torch

import lgamd  # noqa: F401

MARGIN = 1e-4  # tests/test_gpu_superglue.py: the near-tie band of a match decision
NEAR_TIE_CAP = 0.02  # at most this share of a case's real points may lie inside the band

# name -> conf, capacities, per-pair counts, weight seed, data seed
SG_CASES = {
    "small": {"conf": {"GNN_layers": ["self", "cross"] * 2, "num_sinkhorn_iterations": 20, "weights": None},
              "M": 96, "N": 80, "counts": ((96, 80), (37, 41), (1, 5), (50, 0)), "wseed": 7, "dseed": 21},
    # the full 18 layers x 50 iterations: more than one attention tile and more than one Sinkhorn row run
    "full": {"conf": {"weights": None}, "M": 300, "N": 260, "counts": ((300, 260), (129, 257)), "wseed": 3, "dseed": 5},
}

# Sinkhorn alone: name -> capacities (M, N), counts, iterations, seed
SK_CASES = {
    "fused_odd": ((33, 257), ((33, 257), (17, 255), (1, 1), (32, 6)), 20, 101),     # ragged last float4 chunk, odd rows
    "four_wave": ((300, 4096), ((300, 4096), (299, 4093)), 10, 102),                # 16 chunks per lane
    "two_read": ((40, 4100), ((40, 4100), (7, 4097)), 10, 103),                     # N > 4096
}
SK_ALPHA = 1.0


def to_capacity(per_pair, M, N, counts, dtype=np.float32):
    """Per-pair oracle outputs (dicts with la [n0+1, n1+1], and optionally cost [n0, n1], m0, m1, s0,
    s1, d0 [n0, D], d1 [n1, D]; None for an empty pair) -> the capacity-layout arrays."""
    B = len(counts)
    out = {"log_assignment": np.full((B, M + 1, N + 1), -np.inf, dtype),
           "matches0": np.full((B, M), -1, np.int64), "matches1": np.full((B, N), -1, np.int64),
           "matching_scores0": np.zeros((B, M), dtype), "matching_scores1": np.zeros((B, N), dtype),
           "sinkhorn_cost": np.zeros((B, M, N), dtype)}
    D = next((p["d0"].shape[-1] for p in per_pair if p is not None and "d0" in p), None)
    if D is not None:
        out["gnn_descriptors0"] = np.zeros((B, M, D), dtype)
        out["gnn_descriptors1"] = np.zeros((B, N, D), dtype)
    for b, (n0, n1) in enumerate(counts):
        p = per_pair[b]
        la = out["log_assignment"][b]
        if n0 == 0 or n1 == 0:
            assert p is None
            la[M, N] = 0.0
            continue
        z = np.asarray(p["la"])
        assert z.shape == (n0 + 1, n1 + 1)
        la[:n0, :n1] = z[:n0, :n1]
        la[:n0, N] = z[:n0, n1]
        la[M, :n1] = z[n0, :n1]
        la[M, N] = z[n0, n1]
        for key, dst, n in (("m0", "matches0", n0), ("m1", "matches1", n1), ("s0", "matching_scores0", n0),
                            ("s1", "matching_scores1", n1)):
            if key in p:
                out[dst][b, :n] = np.asarray(p[key])
        if "cost" in p:
            out["sinkhorn_cost"][b, :n0, :n1] = np.asarray(p["cost"])
        if "d0" in p:
            out["gnn_descriptors0"][b, :n0] = np.asarray(p["d0"])
            out["gnn_descriptors1"][b, :n1] = np.asarray(p["d1"])
    return out


# ---------------------------------------------------------------- Sinkhorn alone
@functools.lru_cache(maxsize=None)
def sk_scores(name):
    (M, N), counts, _, seed = SK_CASES[name]
    g = torch.Generator().manual_seed(seed)
    s = (torch.randn((len(counts), M, N), generator=g) * 2.0).numpy()
    s.setflags(write=False)
    return s


def sk_reference(scores, counts, alpha, iters):
    """The capacity-layout Z of per-pair ``oracle.log_optimal_transport`` runs (fp32, as
    tests/test_gpu_parity.py uses it)."""
    import oracle

    B, M, N = scores.shape
    per = []
    for b, (n0, n1) in enumerate(counts):
        if n0 == 0 or n1 == 0:
            per.append(None)
            continue
        s = torch.from_numpy(np.array(scores[b:b + 1, :n0, :n1]))  # a writable copy
        per.append({"la": oracle.log_optimal_transport(s, alpha, iters)[0].numpy()})
    return to_capacity(per, M, N, counts)["log_assignment"]


@functools.lru_cache(maxsize=None)
def sk_expected(name):
    (M, N), counts, iters, _ = SK_CASES[name]
    z = sk_reference(sk_scores(name), counts, SK_ALPHA, iters)
    z.setflags(write=False)
    return z


def nan_padded(x, counts, side_axis):
    """A copy of x [B, ...] with NaN beyond each pair's counts: side_axis maps an axis of x (after the
    batch axis, 1-based) to the side (0 / 1) whose count bounds it."""
    x = np.array(x, copy=True)
    for b, c in enumerate(counts):
        for axis, side in side_axis.items():
            idx = [slice(None)] * x.ndim
            idx[0] = b
            idx[axis] = slice(c[side], None)
            x[tuple(idx)] = np.nan
    return x


# ---------------------------------------------------------------- SuperGlue
@functools.lru_cache(maxsize=None)
def sg_inputs(name):
    """(state dict, capacity-layout numpy inputs) of a case; the padding holds ordinary values here
    (tests overwrite it with NaN)."""
    from lightglue_amd.sg_weights import superglue_state_dict, synthetic_scores
    from lightglue_amd.weights import synthetic_pair

    c = SG_CASES[name]
    B, M, N = len(c["counts"]), c["M"], c["N"]
    sd = superglue_state_dict(c["conf"], seed=c["wseed"])
    p = synthetic_pair(B, M, N, seed=c["dseed"], width=640, height=480)
    data = {"keypoints0": p["keypoints0"], "keypoints1": p["keypoints1"], "descriptors0": p["descriptors0"],
            "descriptors1": p["descriptors1"], "keypoint_scores0": synthetic_scores(B, M, seed=c["dseed"] + 1),
            "keypoint_scores1": synthetic_scores(B, N, seed=c["dseed"] + 2),
            "image_size": np.tile([[640.0, 480.0]], (B, 1)).astype(np.float32)}
    for v in data.values():
        v.setflags(write=False)
    return sd, data


def sg_pair_data(name, b):
    """Pair b alone at its own sizes (numpy, batch of one)."""
    _, data = sg_inputs(name)
    n0, n1 = SG_CASES[name]["counts"][b]
    out = {}
    for k, v in data.items():
        n = {"0": n0, "1": n1}.get(k[-1])
        out[k] = v[b:b + 1].copy() if k == "image_size" else v[b:b + 1, :n].copy()
    return out


@functools.lru_cache(maxsize=None)
def sg_oracle_pair(name, b):
    """The CPU oracle (float64, as tests/test_gpu_superglue.py::test_superglue_matches_oracle) on pair
    b alone; None for a pair with an empty image."""
    from oracle.superglue_ref import superglue_forward

    n0, n1 = SG_CASES[name]["counts"][b]
    if n0 == 0 or n1 == 0:
        return None
    sd, _ = sg_inputs(name)
    with torch.no_grad():
        ref = superglue_forward(sd, sg_pair_data(name, b), SG_CASES[name]["conf"], dtype=torch.float64)
    return {"la": ref["log_assignment"][0].numpy(), "cost": ref["sinkhorn_cost"][0].numpy(),
            "m0": ref["matches0"][0].numpy(), "m1": ref["matches1"][0].numpy(),
            "s0": ref["matching_scores0"][0].numpy(), "s1": ref["matching_scores1"][0].numpy(),
            "d0": ref["gnn_desc0"][0].transpose(0, 1).numpy(), "d1": ref["gnn_desc1"][0].transpose(0, 1).numpy()}


@functools.lru_cache(maxsize=None)
def sg_expected(name):
    c = SG_CASES[name]
    per = [sg_oracle_pair(name, b) for b in range(len(c["counts"]))]
    out = to_capacity(per, c["M"], c["N"], c["counts"], np.float64)
    for v in out.values():
        v.setflags(write=False)
    return out


def decided(la, th):
    """Rows / columns of a pair's oracle log assignment [n0+1, n1+1] whose match decision lies outside
    the near-tie band: the point's own top-1 / top-2 gap, the threshold distance of its score, and the
    gap of the partner it points at (the mutual check reads that argmax too) all exceed MARGIN."""
    z = np.asarray(la, np.float64)[:-1, :-1]

    def gap(a):  # along the last axis
        if a.shape[-1] < 2:
            return np.full(a.shape[:-1], np.inf)
        s = np.sort(a, axis=-1)
        return s[..., -1] - s[..., -2]

    rg, cg = gap(z), gap(z.T)
    ri, ci = z.argmax(1), z.argmax(0)
    rth = np.abs(np.exp(z.max(1)) - th)
    cth = np.abs(np.exp(z.max(0)) - th)
    rows = (rg > MARGIN) & (rth > MARGIN) & (cg[ri] > MARGIN)
    cols = (cg > MARGIN) & (cth > MARGIN) & (rg[ci] > MARGIN)
    return rows, cols


@functools.lru_cache(maxsize=None)
def sg_decided(name):
    """Capacity-layout masks of the decided real points of a case, and the share of real points
    inside the band."""
    from lightglue_amd.sg_weights import merged_conf

    c = SG_CASES[name]
    th = merged_conf(c["conf"])["filter_threshold"]
    B = len(c["counts"])
    r = np.zeros((B, c["M"]), bool)
    k = np.zeros((B, c["N"]), bool)
    real = 0
    for b, (n0, n1) in enumerate(c["counts"]):
        p = sg_oracle_pair(name, b)
        if p is None:
            continue
        r[b, :n0], k[b, :n1] = decided(p["la"], th)
        real += n0 + n1
    share = 1.0 - (r.sum() + k.sum()) / max(real, 1)
    return r, k, float(share)
