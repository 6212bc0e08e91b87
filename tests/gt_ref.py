"""Torch-CPU restatement of the reference's homography ground truth, for the tests only (any dtype).

``gt_matches_from_homography`` is ``gluefactory/geometry/gt_generation.py:109-161``;
``warp_points_torch`` is ``geometry/homography.py:161-180`` with ``to_homogeneous`` /
``from_homogeneous`` of ``geometry/utils.py:5-30``.  tests/golden/make_gt_golden.py runs the
reference itself; tests/test_gt_golden.py holds this restatement to those fixtures.

Also here: the fixture loader and the comparison under the near-tie gating the fixtures record
(:func:`check_against_fixture`), shared by the CPU and the GPU tests.
"""
import glob
import json
import os

import numpy as np
import torch

# a directory of their own: tests/golden_util.py takes every tests/golden/*.npz it does not know by
# prefix for a LightGlue forward golden
HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gt")


def warp_points_torch(points, H, inverse=True):  # homography.py:161-180
    points = torch.cat([points, points.new_ones(points.shape[:-1] + (1,))], dim=-1)  # utils.py:12-14
    H_mat = (torch.inverse(H) if inverse else H).transpose(-2, -1)
    warped = torch.einsum("...nj,...ji->...ni", points, H_mat)
    return warped[..., :-1] / (warped[..., -1:] + 1e-5)  # utils.py:30, eps=1e-5


@torch.no_grad()
def gt_matches_from_homography(kp0, kp1, H, pos_th=3, neg_th=6):  # gt_generation.py:109-161
    if kp0.shape[1] == 0 or kp1.shape[1] == 0:  # :111-119
        b_size, n_kp0 = kp0.shape[:2]
        n_kp1 = kp1.shape[1]
        assignment = torch.zeros(b_size, n_kp0, n_kp1, dtype=torch.bool, device=kp0.device)
        m0 = -torch.ones_like(kp0[:, :, 0]).long()
        m1 = -torch.ones_like(kp1[:, :, 0]).long()
        return assignment, m0, m1
    kp0_1 = warp_points_torch(kp0, H, inverse=False)
    kp1_0 = warp_points_torch(kp1, H, inverse=True)

    dist0 = torch.sum((kp0_1.unsqueeze(-2) - kp1.unsqueeze(-3)) ** 2, -1)  # :124-126
    dist1 = torch.sum((kp0.unsqueeze(-2) - kp1_0.unsqueeze(-3)) ** 2, -1)
    dist = torch.max(dist0, dist1)

    reward = (dist < pos_th**2).float() - (dist > neg_th**2).float()  # :128

    min0 = dist.min(-1).indices  # :130-137
    min1 = dist.min(-2).indices
    ismin0 = torch.zeros(dist.shape, dtype=torch.bool, device=dist.device)
    ismin1 = ismin0.clone()
    ismin0.scatter_(-1, min0.unsqueeze(-1), value=1)
    ismin1.scatter_(-2, min1.unsqueeze(-2), value=1)
    positive = ismin0 & ismin1 & (dist < pos_th**2)

    negative0 = dist0.min(-1).values > neg_th**2  # :139-140
    negative1 = dist1.min(-2).values > neg_th**2

    unmatched = min0.new_tensor(-1)  # :145-150
    ignore = min0.new_tensor(-2)
    m0 = torch.where(positive.any(-1), min0, ignore)
    m1 = torch.where(positive.any(-2), min1, ignore)
    m0 = torch.where(negative0, unmatched, m0)
    m1 = torch.where(negative1, unmatched, m1)

    return {
        "assignment": positive,
        "reward": reward,
        "matches0": m0,
        "matches1": m1,
        "matching_scores0": (m0 > -1).float(),
        "matching_scores1": (m1 > -1).float(),
        "proj_0to1": kp0_1,
        "proj_1to0": kp1_0,
    }


# ---------------------------------------------------------------------------------------------
# margins and gating (the issue's definition; computed in fp64 by the generator, reused by the
# end-to-end GPU test on its own inputs)
def margins(kp0, kp1, H, pos_th, neg_th, tau):
    """fp64 run of the chain and the undecidable masks: rows [B,M], columns [B,N], reward entries
    [B,M,N].  A row (a column likewise, with its own quantities) is undecidable if
    |min dist - pos_th^2| < tau, |min dist0 - neg_th^2| < tau, or min dist < pos_th^2 + tau while
    its top-2 gap, or the top-2 gap of its best column, is below tau."""
    kp0, kp1, H = (torch.as_tensor(np.asarray(x)).double() for x in (kp0, kp1, H))
    p01 = warp_points_torch(kp0, H, inverse=False)
    p10 = warp_points_torch(kp1, H, inverse=True)
    d0 = torch.sum((p01.unsqueeze(-2) - kp1.unsqueeze(-3)) ** 2, -1)
    d1 = torch.sum((kp0.unsqueeze(-2) - p10.unsqueeze(-3)) ** 2, -1)
    d = torch.max(d0, d1)
    p2, n2 = float(pos_th) ** 2, float(neg_th) ** 2

    def side(dm, dh):  # dm: dist with the scanned side last; dh: the half whose minimum decides -1
        inf = dm.new_full(dm.shape[:-1] + (1,), float("inf"))  # a single candidate has an infinite gap
        top = torch.cat([dm, inf], -1).topk(2, dim=-1, largest=False).values
        return top[..., 0], top[..., 1] - top[..., 0], dm.argmin(-1), dh.min(-1).values

    rmin, rgap, rarg, rhalf = side(d, d0)
    cmin, cgap, carg, chalf = side(d.transpose(1, 2), d1.transpose(1, 2))
    und_r = ((rmin - p2).abs() < tau) | ((rhalf - n2).abs() < tau) | (
        (rmin < p2 + tau) & ((rgap < tau) | (cgap.gather(1, rarg) < tau)))
    und_c = ((cmin - p2).abs() < tau) | ((chalf - n2).abs() < tau) | (
        (cmin < p2 + tau) & ((cgap < tau) | (rgap.gather(1, carg) < tau)))
    und_e = ((d - p2).abs() < tau) | ((d - n2).abs() < tau)
    return {"und_rows": und_r.numpy(), "und_cols": und_c.numpy(), "und_reward": und_e.numpy(), "dist": d.numpy(),
            "proj_0to1": p01.numpy(), "proj_1to0": p10.numpy()}


def tau_of(kp0, kp1, H, pos_th, neg_th):
    """tau = 4 e as tests/golden/make_gt_golden.py records it, from this restatement's own fp32 and
    fp64 runs: e = max |dist_fp32 - dist_fp64| over entries with dist_fp64 < 4 max(pos_th, neg_th)^2."""
    def dist(k0, k1, h):
        r = gt_matches_from_homography(k0, k1, h, pos_th, neg_th)
        d0 = torch.sum((r["proj_0to1"].unsqueeze(-2) - k1.unsqueeze(-3)) ** 2, -1)
        d1 = torch.sum((k0.unsqueeze(-2) - r["proj_1to0"].unsqueeze(-3)) ** 2, -1)
        return torch.max(d0, d1)

    k0, k1, h = (torch.as_tensor(np.asarray(x, np.float32)) for x in (kp0, kp1, H))
    d32, d64 = dist(k0, k1, h).double(), dist(k0.double(), k1.double(), h.double())
    near = d64 < 4.0 * max(pos_th, neg_th) ** 2
    return 4.0 * float((d32 - d64)[near].abs().max())


def fixture_names():
    return sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(HERE, "gt_*.npz")))


def load_fixture(name):
    z = np.load(os.path.join(HERE, name + ".npz"))
    g = {k: z[k] for k in z.files if k != "meta_json"}
    meta = json.loads(str(z["meta_json"]))
    B, M, N = meta["B"], meta["M"], meta["N"]
    a = np.zeros((B, M, N), bool)
    t = g.pop("assignment_idx")
    a[t[:, 0], t[:, 1], t[:, 2]] = True
    g["assignment"] = a
    g["reward"] = g.pop("reward_i8").astype(np.float32)
    und = np.zeros((B, M, N), bool)
    t = g.pop("und_reward_idx")
    und[t[:, 0], t[:, 1], t[:, 2]] = True
    g["und_reward"] = und
    return g, meta


def check_against_fixture(got, g, meta, reward=True):
    """``got`` (dict of NumPy arrays) against fixture ``g``: the exact case bit for bit in every
    output; the others on every decidable item, projections within the recorded tolerance."""
    if meta["exact"]:
        keys = ["assignment", "matches0", "matches1", "matching_scores0", "matching_scores1", "proj_0to1", "proj_1to0"]
        for k in keys + (["reward"] if reward else []):
            assert got[k].dtype == g[k].dtype, k
            np.testing.assert_array_equal(got[k].view(np.uint8) if got[k].dtype != bool else got[k],
                                          g[k].view(np.uint8) if g[k].dtype != bool else g[k], err_msg=k)
        return
    ok_r, ok_c = ~g["und_rows"], ~g["und_cols"]
    for k, ok in (("matches0", ok_r), ("matches1", ok_c), ("matching_scores0", ok_r), ("matching_scores1", ok_c)):
        np.testing.assert_array_equal(got[k][ok], g[k][ok], err_msg=k)
    # an entry of the assignment is decided when its row and its column are
    ok_a = ok_r[:, :, None] & ok_c[:, None, :]
    np.testing.assert_array_equal(got["assignment"][ok_a], g["assignment"][ok_a], err_msg="assignment")
    if reward:
        ok_e = ~g["und_reward"]
        np.testing.assert_array_equal(got["reward"][ok_e], g["reward"][ok_e], err_msg="reward")
    for k in ("proj_0to1", "proj_1to0"):
        np.testing.assert_allclose(got[k].astype(np.float64), g[k + "_f64"], rtol=0, atol=float(meta["proj_tol"]), err_msg=k)
