"""Float64 numpy restatement of the batched LO-RANSAC for homographies, written from the
specification: the counter-based sampler, the projective-basis minimal solver, rounds of 256
hypotheses, the 8-step local optimisation by an unweighted Hartley-normalised DLT (through an SVD
here), the stopping rule and the fp32 result whose mask is its own classification.

Besides the estimator's outputs ``ransac_homography`` returns every field of the kernel's ``info`` row
and the case's ``margin``: the smallest ``|lhs - rhs| / |rhs|`` over every comparison that steers the
run (each residual against ``th`` or ``m * th``, each determinant against ``min_area``, the stop rule).
Two float64 evaluations of the same formula agree to ~1e-12, so a case whose margin is far above that
takes the same path in any of them.
"""
import math

import numpy as np

MASK = (1 << 64) - 1
ROUND = 256
MAX_DRAWS = 64
LO_MULTIPLIERS = (3.0, 2.5, 2.0, 1.5, 1.0, 1.0, 1.0, 1.0)
# the triples of a four-point sample whose determinants are the basis coefficients: p3 replaces p_k
TRIPLES = ((3, 1, 2), (0, 3, 2), (0, 1, 3), (0, 1, 2))


def mix64(z):
    z = (z + 0x9E3779B97F4A7C15) & MASK
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK
    return z ^ (z >> 31)


def sample(seed, t, K):
    """The four distinct match indices of hypothesis t, or None after 64 draws."""
    base = mix64(seed & MASK) + (t << 16)
    got = []
    for d in range(MAX_DRAWS):
        i = ((mix64((base + d) & MASK) >> 32) * K) >> 32
        if i not in got:
            got.append(i)
            if len(got) == 4:
                return got
    return None


def live_matches(kpts0, kpts1, matches0=None, num0=None, num1=None):
    """(rows [K, 4] float64 of x0 y0 x1 y1, their slots) under the kernel's rules."""
    kpts0, kpts1 = np.asarray(kpts0), np.asarray(kpts1)
    n0 = len(kpts0) if num0 is None else min(max(int(num0), 0), len(kpts0))
    n1 = len(kpts1) if num1 is None else min(max(int(num1), 0), len(kpts1))
    m = np.arange(len(kpts0)) if matches0 is None else np.asarray(matches0).astype(np.int64)
    slots = np.array([i for i in range(n0) if 0 <= m[i] < n1], dtype=np.int64)
    if len(slots) == 0:
        return np.zeros((0, 4)), slots
    rows = np.concatenate([kpts0[slots], kpts1[m[slots]]], 1).astype(np.float32).astype(np.float64)
    return rows, slots


class _Margin:
    def __init__(self):
        self.value = math.inf

    def note(self, lhs, rhs):
        lhs = np.asarray(lhs, dtype=np.float64)
        ok = np.isfinite(lhs)
        if ok.any():
            self.value = min(self.value, float(np.min(np.abs(lhs[ok] - rhs) / abs(rhs))))


def residuals(H, pts):
    """Forward transfer distances [..., K] of models [..., 3, 3]; non-finite where w is 0."""
    x, y = pts[:, 0], pts[:, 1]
    H = np.asarray(H, dtype=np.float64)
    with np.errstate(all="ignore"):
        X = H[..., 0, 0, None] * x + H[..., 0, 1, None] * y + H[..., 0, 2, None]
        Y = H[..., 1, 0, None] * x + H[..., 1, 1, None] * y + H[..., 1, 2, None]
        w = H[..., 2, 0, None] * x + H[..., 2, 1, None] * y + H[..., 2, 2, None]
        return np.sqrt((X / w - pts[:, 2]) ** 2 + (Y / w - pts[:, 3]) ** 2)


def _inliers(H, pts, th, margin):
    r = residuals(H, pts)
    margin.note(r, th)
    with np.errstate(invalid="ignore"):
        return np.isfinite(r) & (r < th)


def minimal_solver(quad, min_area, margin):
    """H from four matches [4, 4] by the projective-basis closed form, or None when rejected."""
    hom = lambda p: np.concatenate([p, np.ones((4, 1))], 1)  # noqa: E731
    P, Q = hom(quad[:, :2]), hom(quad[:, 2:])
    d = np.array([np.linalg.det(P[list(t)]) for t in TRIPLES])
    e = np.array([np.linalg.det(Q[list(t)]) for t in TRIPLES])
    margin.note(np.abs(np.concatenate([d, e])), min_area)
    if (np.abs(d) < min_area).any() or (np.abs(e) < min_area).any():
        return None
    same = (d > 0) == (e > 0)
    if not (same.all() or (~same).all()):
        return None
    A = (P[:3] * d[:3, None]).T  # columns d_k p_k
    B = (Q[:3] * e[:3, None]).T
    adj = np.stack([np.cross(A[:, 1], A[:, 2]), np.cross(A[:, 2], A[:, 0]), np.cross(A[:, 0], A[:, 1])])
    return B @ adj


def dlt(pts):
    """Unweighted Hartley-normalised DLT of rows [n, 4]."""
    def frame(p):
        mean = p.mean(0)
        s = math.sqrt(2.0) / np.linalg.norm(p - mean, axis=1).mean()
        return np.array([[s, 0, -s * mean[0]], [0, s, -s * mean[1]], [0, 0, 1.0]])

    T0, T1 = frame(pts[:, :2]), frame(pts[:, 2:])
    u = np.concatenate([pts[:, :2], np.ones((len(pts), 1))], 1) @ T0.T
    v = np.concatenate([pts[:, 2:], np.ones((len(pts), 1))], 1) @ T1.T
    z = np.zeros_like(u)
    rows = np.concatenate([np.concatenate([z, -u, v[:, 1:2] * u], 1), np.concatenate([u, z, -v[:, 0:1] * u], 1)])
    h = np.linalg.svd(rows, full_matrices=len(rows) < 9)[2][-1].reshape(3, 3)
    return np.linalg.inv(T1) @ h @ T0


def local_optimisation(H, count, pts, th, margin):
    for m in LO_MULTIPLIERS:
        sel = _inliers(H, pts, m * th, margin)
        if sel.sum() < 4:
            break
        with np.errstate(all="ignore"):
            fit = dlt(pts[sel])
        c = int(_inliers(fit, pts, th, margin).sum())
        if c >= count:
            H, count = fit, c
    return H, count


def corner_error(H, H_gt, size):
    w, h = float(size[0]), float(size[1])
    c = np.array([[0, 0, 1.0], [w, 0, 1], [w, h, 1], [0, h, 1]])
    a, b = c @ np.asarray(H, dtype=np.float64).T, c @ np.asarray(H_gt, dtype=np.float64).T
    return float(np.linalg.norm(a[:, :2] / a[:, 2:] - b[:, :2] / b[:, 2:], axis=1).mean())


def ransac_homography(pts, th, max_iters=3000, confidence=0.995, seed=0, min_area=1.0):
    """pts [K, 4] (x0, y0, x1, y1).  Returns success, H (fp32 [3, 3]), inliers [K] bool, the info
    fields and the margin."""
    pts = np.asarray(pts, dtype=np.float64).reshape(-1, 4)
    th = float(np.float32(th))
    K = len(pts)
    margin = _Margin()
    out = {"success": 0, "num_matches": K, "num_inliers": 0, "best_t": -1, "best_minimal_count": 0, "rounds": 0,
           "valid_hypotheses": 0, "H": np.eye(3, dtype=np.float32), "inliers": np.zeros(K, dtype=bool)}
    best_min, best_lo, H_lo = -1, -1, None
    done = 0
    while K >= 4 and done < max_iters:
        ts = range(done, min(done + ROUND, max_iters))
        done = ts[-1] + 1
        out["rounds"] += 1
        models, ids = [], []
        for t in ts:
            idx = sample(seed, t, K)
            H = None if idx is None else minimal_solver(pts[idx], min_area, margin)
            if H is not None:
                models.append(H), ids.append(t)
        out["valid_hypotheses"] += len(ids)
        if ids:
            r = residuals(np.stack(models), pts)
            margin.note(r, th)
            with np.errstate(invalid="ignore"):
                counts = (np.isfinite(r) & (r < th)).sum(1)
            k = int(np.argmax(counts))  # the first of equal counts: the lowest t
            if counts[k] > best_min:
                best_min, out["best_t"] = int(counts[k]), ids[k]
                H, c = local_optimisation(models[k], best_min, pts, th, margin)
                if c > best_lo:
                    best_lo, H_lo = c, H
        if best_lo >= 4:
            with np.errstate(divide="ignore"):
                lhs, rhs = done * np.log1p(-((best_lo / K) ** 4)), math.log1p(-confidence)
            margin.note(lhs, rhs)
            if lhs <= rhs:
                break
    out["best_minimal_count"] = max(best_min, 0)
    out["margin"] = margin.value
    if H_lo is None or not np.isfinite(H_lo).all() or not abs(H_lo[2, 2]) > 1e-12 * np.abs(H_lo).max():
        return out
    H32 = (H_lo / H_lo[2, 2]).astype(np.float32)
    inl = _inliers(H32.astype(np.float64), pts, th, margin)
    out["margin"] = margin.value
    if inl.sum() < 4:
        return out
    out.update(success=1, num_inliers=int(inl.sum()), H=H32, inliers=inl)
    return out


INFO_FIELDS = ("success", "num_matches", "num_inliers", "best_t", "best_minimal_count", "rounds", "valid_hypotheses")


def info_row(out):
    return np.array([out[k] for k in INFO_FIELDS] + [0], dtype=np.int32)


def estimate_pair(kpts0, kpts1, matches0, th, num0=None, num1=None, H_gt=None, size=None, **options):
    """One pair in keypoint form: the restatement's outputs in keypoints0 slot order."""
    pts, slots = live_matches(kpts0, kpts1, matches0, num0, num1)
    out = ransac_homography(pts, th, **options)
    mask = np.zeros(len(kpts0), dtype=bool)
    mask[slots] = out["inliers"]
    out["inliers_slots"], out["m_kpts"] = mask, pts.astype(np.float32)
    if H_gt is not None:
        out["H_error"] = corner_error(out["H"], H_gt, size) if out["success"] else math.inf
    return out
