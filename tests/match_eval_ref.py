"""Float64 torch restatement of the three match-evaluation metrics (lightglue_amd.match_eval,
csrc/match_eval.hip), written from their formulas, one pair at a time, for the tests.

Inputs are one pair's tensors of any float dtype; everything is computed in float64.  ``num0`` /
``num1`` (optional ints) cut a padded pair down to its real keypoints first.
"""
import math

import torch

HOM_THRESHOLDS = (1.0, 3.0)
EPI_THRESHOLDS = (1e-4, 5e-4, 1e-3)


def live_matches(kpts0, kpts1, matches0, scores0, num0=None, num1=None):
    """Matched point pairs [n,2], [n,2] and their scores [n] in float64."""
    M = kpts0.shape[0] if num0 is None else int(num0)
    N = kpts1.shape[0] if num1 is None else int(num1)
    m = matches0[:M]
    live = (m > -1) & (m < N)
    idx = m[live].long()
    return kpts0[:M][live].double(), kpts1[idx].double(), scores0[:M][live].double()


def _warp(H, p):
    q = torch.cat([p, torch.ones_like(p[:, :1])], 1) @ H.T
    return q[:, :2] / q[:, 2:]


def homography_errors(p0, p1, H):
    """(|hom(H p0) - p1| + |hom(H^-1 p1) - p0|) / 2 per match.  The inverse is the pseudo-inverse of H^T, as
    in the reference: its SVD leaves about cond(H) * 1e-16 in the inverse, which is 1e-9 of an error here,
    so only the same routine reproduces the reference's fp64 errors to 1e-12 (the exact inverse the
    kernel uses is the closer of the two to the true value; the counts are the same either way)."""
    H = H.double().reshape(3, 3)
    return ((_warp(H, p0) - p1).norm(dim=1) + (_warp(torch.linalg.pinv(H.T).T, p1) - p0).norm(dim=1)) / 2


def epipolar_errors(p0, p1, cam0, cam1, T):
    """|p1^T E p0| (1 / sqrt(d0) + 1 / sqrt(d1)) / 2 on normalised image coordinates, E = [t]x R,
    d0 / d1 the squared norms of the first two components of E p0 / E^T p1, clamped at 1e-6.  The triple
    product is one einsum: it cancels to 1e-5 of its terms on a good match, so only the same contraction
    reproduces the reference's fp64 value to 1e-12 relative."""
    cam0, cam1, T = cam0.double().reshape(-1), cam1.double().reshape(-1), T.double().reshape(-1)
    R, t = T[:9].reshape(3, 3), T[9:]
    tx = torch.tensor([[0.0, -t[2], t[1]], [t[2], 0.0, -t[0]], [-t[1], t[0], 0.0]], dtype=torch.float64)
    E = tx @ R
    one = torch.ones_like(p0[:, :1])
    a = torch.cat([(p0 - cam0[4:6]) / cam0[2:4], one], 1)
    b = torch.cat([(p1 - cam1[4:6]) / cam1[2:4], one], 1)
    Ea, Etb = a @ E.T, b @ E
    bEa = torch.einsum("ni,ij,nj->n", b, E, a)  # p1^T E p0
    d0 = (Ea[:, 0] ** 2 + Ea[:, 1] ** 2).clamp(min=1e-6)
    d1 = (Etb[:, 0] ** 2 + Etb[:, 1] ** 2).clamp(min=1e-6)
    return bEa.abs() * (1 / d0.sqrt() + 1 / d1.sqrt()) / 2


def _hartley(p):
    mean = p.mean(0)
    s = math.sqrt(2.0) / ((p - mean).norm(dim=1).mean() + 1e-8)
    T = torch.tensor([[s, 0.0, -s * mean[0]], [0.0, s, -s * mean[1]], [0.0, 0.0, 1.0]], dtype=torch.float64)
    return (p - mean) * s, T


def dlt_homography(p0, p1, w):
    """Score-weighted DLT: the eigenvector of the smallest eigenvalue of A^T W A on Hartley-normalised
    points, de-normalised, divided by H[2,2] + 1e-8.  Fewer than 4 matches: all inf."""
    if p0.shape[0] < 4:
        return torch.full((3, 3), float("inf"), dtype=torch.float64)
    a, T0 = _hartley(p0)
    b, T1 = _hartley(p1)
    x, y, X, Y = a[:, 0], a[:, 1], b[:, 0], b[:, 1]
    o, z = torch.ones_like(x), torch.zeros_like(x)
    rows_x = torch.stack([z, z, z, -x, -y, -o, Y * x, Y * y, Y], 1)
    rows_y = torch.stack([x, y, o, z, z, z, -X * x, -X * y, -X], 1)
    A = torch.cat([rows_x, rows_y], 0)
    ww = torch.cat([w, w], 0)
    _, vec = torch.linalg.eigh(A.T @ (ww[:, None] * A))
    H = torch.linalg.inv(T1) @ vec[:, 0].reshape(3, 3) @ T0
    return H / (H[2, 2] + 1e-8)


def corner_error(H, H_gt, image_size):
    W, Hh = float(image_size[0]), float(image_size[1])
    c = torch.tensor([[0.0, 0.0], [W, 0.0], [W, Hh], [0.0, Hh]], dtype=torch.float64)
    return (_warp(H.double().reshape(3, 3), c) - _warp(H_gt.double().reshape(3, 3), c)).norm(dim=1).mean()


def evaluate_pair(kpts0, kpts1, matches0, scores0, H=None, image_size=None, cam0=None, cam1=None, T=None,
                  num0=None, num1=None):
    """Everything the kernel reports for one pair, as Python numbers / float64 tensors."""
    p0, p1, w = live_matches(kpts0, kpts1, matches0, scores0, num0, num1)
    out = {"n": p0.shape[0]}
    if H is not None:
        err = homography_errors(p0, p1, H)
        out["hom_err"] = err
        out["hom_counts"] = [int((err < t).sum()) for t in HOM_THRESHOLDS]
        if image_size is not None:
            out["H_dlt"] = dlt_homography(p0, p1, w)
            out["H_error_dlt"] = float(corner_error(out["H_dlt"], H, image_size))
    if T is not None:
        err = epipolar_errors(p0, p1, cam0, cam1, T)
        out["epi_err"] = err
        out["epi_counts"] = [int((err < t).sum()) for t in EPI_THRESHOLDS]
    return out
