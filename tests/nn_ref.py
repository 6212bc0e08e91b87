"""Torch-CPU restatement of the reference's nearest-neighbour matcher, for the tests only (any dtype).

``nn_forward`` is ``gluefactory/models/matchers/nearest_neighbor_matcher.py:16-72`` (``find_nn``,
``mutual_check`` and ``NearestNeighborMatcher._forward``).  tests/golden/make_nn_golden.py runs the
reference itself; tests/test_nn_golden.py holds this restatement to those fixtures.

Also here: the fixture loader, the fp64 decision margins and the comparison under the near-tie
gating the fixtures record (:func:`check_against_fixture`), shared by the CPU and the GPU tests.

Fixture inputs are stored as int8 codes ``q``; the descriptors are ``q / |q|`` formed in fp64 (an
exact integer sum of squares, one square root, one division) and rounded once to fp32, or ``q / 64``
for the exact fixture, so every host decodes the same bits.
"""
import glob
import json
import os

import numpy as np
import torch

# a directory of their own: tests/golden_util.py takes every tests/golden/*.npz it does not know by
# prefix for a LightGlue forward golden
HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "nn")

# (ratio_thresh, distance_thresh) x mutual_check, in the order of the stored outputs
FLAVOURS = [(r, d, mu) for (r, d) in ((None, None), (0.8, 0.7), (0.95, None), (None, 1.0)) for mu in (True, False)]
# the fp16x3 product's measured maximum error per sum_k |a_k b_k|
H3_ERR = 2.4e-7


def flavour_key(ratio, dist, mutual):
    return f"r{ratio}_d{dist}_m{int(bool(mutual))}"


def find_nn(sim, ratio_thresh, distance_thresh):  # :16-25
    k = 2 if ratio_thresh else 1
    val, ind = sim.topk(k, dim=-1, largest=True)
    dist = 2 * (1 - val)
    keep = torch.ones(ind.shape[:-1], dtype=torch.bool)
    if ratio_thresh:
        keep = keep & (dist[..., 0] <= (ratio_thresh**2) * dist[..., 1])
    if distance_thresh:
        keep = keep & (dist[..., 0] <= distance_thresh**2)
    return torch.where(keep, ind[..., 0], ind.new_tensor(-1))


def mutual_check(m0, m1):  # :28-35
    i0 = torch.arange(m0.shape[-1])
    i1 = torch.arange(m1.shape[-1])
    back0 = torch.gather(m1, -1, m0.clamp(min=0))
    back1 = torch.gather(m0, -1, m1.clamp(min=0))
    return (torch.where((m0 > -1) & (back0 == i0), m0, m0.new_tensor(-1)),
            torch.where((m1 > -1) & (back1 == i1), m1, m1.new_tensor(-1)))


@torch.no_grad()
def nn_forward(desc0, desc1, ratio_thresh=None, distance_thresh=None, mutual=True):  # :52-72
    sim = torch.einsum("bnd,bmd->bnm", desc0, desc1)
    m0 = find_nn(sim, ratio_thresh, distance_thresh)
    m1 = find_nn(sim.transpose(1, 2), ratio_thresh, distance_thresh)
    if mutual:
        m0, m1 = mutual_check(m0, m1)
    b, m, n = sim.shape
    la = sim.new_zeros(b, m + 1, n + 1)
    la[:, :-1, :-1] = torch.log_softmax(sim, -1) + torch.log_softmax(sim, -2)
    return {
        "matches0": m0,
        "matches1": m1,
        "matching_scores0": (m0 > -1).float(),
        "matching_scores1": (m1 > -1).float(),
        "similarity": sim,
        "log_assignment": la,
    }


def nn_forward_ragged(desc0, desc1, counts0, counts1, ratio_thresh=None, distance_thresh=None, mutual=True):
    """Each pair run alone on its own counts, padded back: matches -1 and scores 0 for padded points
    (the dense outputs are not assembled)."""
    B, M = desc0.shape[:2]
    N = desc1.shape[1]
    m0 = torch.full((B, M), -1, dtype=torch.int64)
    m1 = torch.full((B, N), -1, dtype=torch.int64)
    for b in range(B):
        a, c = int(counts0[b]), int(counts1[b])
        if a == 0 or c == 0:
            continue  # nothing to scan
        if ratio_thresh and min(a, c) < 2:  # no second neighbour on one side: that side has no matches
            sim = torch.einsum("bnd,bmd->bnm", desc0[b:b + 1, :a], desc1[b:b + 1, :c])
            r0 = find_nn(sim, ratio_thresh, distance_thresh) if c >= 2 else m0.new_full((1, a), -1)
            r1 = find_nn(sim.transpose(1, 2), ratio_thresh, distance_thresh) if a >= 2 else m1.new_full((1, c), -1)
            if mutual:
                r0, r1 = mutual_check(r0, r1)
            m0[b, :a], m1[b, :c] = r0[0], r1[0]
            continue
        r = nn_forward(desc0[b:b + 1, :a], desc1[b:b + 1, :c], ratio_thresh, distance_thresh, mutual)
        m0[b, :a], m1[b, :c] = r["matches0"][0], r["matches1"][0]
    return {"matches0": m0, "matches1": m1, "matching_scores0": (m0 > -1).float(), "matching_scores1": (m1 > -1).float()}


# ---------------------------------------------------------------------------------------------
# tolerance and margins (computed in fp64; the generator stores them, the GPU tests reuse them on
# their own inputs)
def sim64(desc0, desc1):
    return torch.einsum("bnd,bmd->bnm", torch.as_tensor(np.asarray(desc0)).double(),
                        torch.as_tensor(np.asarray(desc1)).double())


def tol_of(desc0, desc1, sim32=None):
    """(e, S, tol): e = max |fp32 similarity - fp64 similarity| of the torch chain (``sim32``: the
    reference's own fp32 similarity; default this restatement's), S = max over entries of
    sum_k |a_k b_k|, tol = 4 max(e, 2.4e-7 S)."""
    d0, d1 = torch.as_tensor(np.asarray(desc0, np.float32)), torch.as_tensor(np.asarray(desc1, np.float32))
    s64 = sim64(d0, d1)
    if sim32 is None:
        sim32 = torch.einsum("bnd,bmd->bnm", d0, d1)
    e = float((torch.as_tensor(np.asarray(sim32)).double() - s64).abs().max())
    S = float(torch.einsum("bnd,bmd->bnm", d0.double().abs(), d1.double().abs()).max())
    return e, S, 4.0 * max(e, H3_ERR * S)


def margins(desc0, desc1, ratio_thresh, distance_thresh, mutual, tol, counts0=None, counts1=None):
    """Undecidable rows [B,M] and columns [B,N] from the fp64 similarity.  A row (a column likewise) is
    undecidable when a comparison its result depends on has a margin below what ``tol`` allows on its
    two sides: its top-1 / top-2 gap < 2 tol; |dist0 - r^2 dist1| < 2 tol (1 + r^2) with the ratio
    test; |dist0 - d^2| < 2 tol with the distance test; under the mutual check the same for the
    partner it points at.  Padded points of a ragged batch are decided (-1)."""
    s = sim64(desc0, desc1)
    B, M, N = s.shape
    c0 = torch.full((B,), M) if counts0 is None else torch.as_tensor(np.asarray(counts0)).long()
    c1 = torch.full((B,), N) if counts1 is None else torch.as_tensor(np.asarray(counts1)).long()
    live0 = torch.arange(M)[None] < c0[:, None]
    live1 = torch.arange(N)[None] < c1[:, None]
    s = s.masked_fill(~(live0[:, :, None] & live1[:, None, :]), float("-inf"))

    def side(sm, live):  # the scanned side last
        pad = sm.new_full(sm.shape[:-1] + (1,), float("-inf"))  # a single candidate has an infinite gap
        top, ind = torch.cat([sm, pad], -1).topk(2, dim=-1)
        d0, d1 = 2 * (1 - top[..., 0]), 2 * (1 - top[..., 1])
        und = (top[..., 0] - top[..., 1]) < 2 * tol
        if ratio_thresh:
            r2 = float(ratio_thresh) ** 2
            und = und | ((d0 - r2 * d1).abs() < 2 * tol * (1 + r2))
        if distance_thresh:
            und = und | ((d0 - float(distance_thresh) ** 2).abs() < 2 * tol)
        return und & live & torch.isfinite(top[..., 0]), ind[..., 0].clamp(max=sm.shape[-1] - 1)

    ur, argr = side(s, live0)
    uc, argc = side(s.transpose(1, 2), live1)
    if mutual:
        ur, uc = ur | (uc.gather(1, argr) & live0), uc | (ur.gather(1, argc) & live1)
    return {"und_rows": ur.numpy(), "und_cols": uc.numpy()}


def log_assignment64(desc0, desc1):
    s = sim64(desc0, desc1)
    b, m, n = s.shape
    la = s.new_zeros(b, m + 1, n + 1)
    la[:, :-1, :-1] = torch.log_softmax(s, -1) + torch.log_softmax(s, -2)
    return la


# ---------------------------------------------------------------------------------------------
def decode(q, exact):
    """int8 codes -> fp32 descriptors (module docstring)."""
    q = np.asarray(q).astype(np.float64)
    if exact:
        return (q / 64.0).astype(np.float32)
    n2 = (q * q).sum(-1, keepdims=True)  # exact: integers far below 2^53
    return (q / np.sqrt(n2)).astype(np.float32)


def fixture_names():
    return sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(HERE, "nn_*.npz")))


def load_fixture(name):
    """(g, meta): g["descriptors0/1"] fp32, g["counts0/1"] (ragged fixtures), per flavour key k
    g[k + "/matches0"], "/matches1" (int64), "/matching_scores0/1" (fp32), "/und_rows", "/und_cols";
    the exact fixture also "similarity" and "log_assignment" (fp32, the reference's)."""
    z = np.load(os.path.join(HERE, name + ".npz"))
    meta = json.loads(str(z["meta_json"]))
    g = {"descriptors0": decode(z["q0"], meta["exact"]), "descriptors1": decode(z["q1"], meta["exact"])}
    for k in z.files:
        if k in ("meta_json", "q0", "q1"):
            continue
        v = z[k]
        if k.endswith(("/matches0", "/matches1")):
            g[k] = v.astype(np.int64)
            g[k.replace("/matches", "/matching_scores")] = (v > -1).astype(np.float32)
        elif k.endswith(("/und_rows", "/und_cols")):
            g[k] = v.astype(bool)
        else:
            g[k] = v
    return g, meta


def check_against_fixture(got, g, meta, ratio, dist, mutual):
    """``got`` (dict of NumPy arrays) against the fixture's flavour on every decidable item."""
    k = flavour_key(ratio, dist, mutual)
    ok_r, ok_c = ~g[k + "/und_rows"], ~g[k + "/und_cols"]
    for key, ok in (("matches0", ok_r), ("matches1", ok_c), ("matching_scores0", ok_r), ("matching_scores1", ok_c)):
        assert got[key].dtype == g[f"{k}/{key}"].dtype, key
        np.testing.assert_array_equal(got[key][ok], g[f"{k}/{key}"][ok], err_msg=f"{k} {key}")
    for key in ("matching_scores0", "matching_scores1"):  # scores are (m > -1), decidable or not
        np.testing.assert_array_equal(got[key], (got[key.replace("matching_scores", "matches")] > -1).astype(np.float32))
