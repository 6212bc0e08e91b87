"""Float64 numpy restatement of the batched five-point LO-RANSAC for relative pose,
written from the specification: §10k's counter-based sampler with five indices, Nistér's five-point
solver, rounds of 256 samples whose every candidate is scored, the 8-step local optimisation by the
linear eight-point fit projected onto the essential manifold, the stop rule with exponent 5, the
cheirality choice among the four decompositions and the fp32 result whose mask is its own
classification.

The solver has two routes to the same candidates:

* ``"kernel"``: the null space by complete-pivot elimination and Gram-Schmidt, Gauss-Jordan with partial
  pivoting on the 10x20 system, a Sturm chain, bisection on the chain's root count and Newton steps:
  what csrc/ransac_relpose.hip does, operation by operation;
* ``"companion"``: the null space from an SVD (brought to the same canonical basis, so that ``z``
  means the same), the 10x10 block through ``numpy.linalg.solve`` and the roots through
  ``numpy.roots``.

Besides the estimator's outputs ``ransac_relpose`` returns every field of the kernel's ``info`` row, a
``trace`` (per round: the candidates' counts in candidate order) and the case's ``margin``: the smallest
relative gap over every comparison that steers the run (the Sampson tests at ``th_n`` and ``m * th_n``
of the candidates that reach the running best count less one and of every local-optimisation model,
ties for the best inside one sample (the gap of the two roots), the stop rule, the cheirality counts and depths).
"""
import math

import numpy as np

from ransac_ref import LO_MULTIPLIERS, MASK, MAX_DRAWS, ROUND, _Margin, live_matches, mix64  # noqa: F401

PIVOT_FLOOR = 1e-12   # relative: a smaller pivot (or Sturm leading coefficient) rejects the sample
BISECTIONS = 48
NEWTONS = 4
INFO_FIELDS = ("success", "num_matches", "num_inliers", "best_t", "best_minimal_count", "rounds", "valid_samples",
               "candidates_scored")

# degree-2 monomials of (x, y, z, 1): the products v_i v_j, i <= j, in lexicographic order
IDX2 = np.zeros((4, 4), dtype=np.int64)
_k = 0
for _i in range(4):
    for _j in range(_i, 4):
        IDX2[_i, _j] = IDX2[_j, _i] = _k
        _k += 1
# degree-3 monomials in Nistér's column order (exponents of x, y, z)
MONO3 = ((3, 0, 0), (0, 3, 0), (2, 1, 0), (1, 2, 0), (2, 0, 1), (2, 0, 0), (0, 2, 1), (0, 2, 0), (1, 1, 1), (1, 1, 0),
         (1, 0, 2), (1, 0, 1), (1, 0, 0), (0, 1, 2), (0, 1, 1), (0, 1, 0), (0, 0, 3), (0, 0, 2), (0, 0, 1), (0, 0, 0))
_EXP1 = ((1, 0, 0), (0, 1, 0), (0, 0, 1), (0, 0, 0))
IDX3 = np.zeros((10, 4), dtype=np.int64)
for _i in range(4):
    for _j in range(_i, 4):
        for _v in range(4):
            e = tuple(a + b + c for a, b, c in zip(_EXP1[_i], _EXP1[_j], _EXP1[_v]))
            IDX3[IDX2[_i, _j], _v] = MONO3.index(e)


def sample5(seed, t, K):
    """The five distinct match indices of sample t, or None after 64 draws."""
    base = mix64(seed & MASK) + (t << 16)
    got = []
    for d in range(MAX_DRAWS):
        i = ((mix64((base + d) & MASK) >> 32) * K) >> 32
        if i not in got:
            got.append(i)
            if len(got) == 5:
                return got
    return None


def normalise(pts, cam0, cam1):
    """Pixel rows [K, 4] (fp32 values) -> normalised rows in float64; cam = (fx, fy, cx, cy)."""
    pts = np.asarray(pts, dtype=np.float32).astype(np.float64).reshape(-1, 4)
    c0 = np.asarray(cam0, dtype=np.float32).astype(np.float64)
    c1 = np.asarray(cam1, dtype=np.float32).astype(np.float64)
    return np.stack([(pts[:, 0] - c0[2]) / c0[0], (pts[:, 1] - c0[3]) / c0[1],
                     (pts[:, 2] - c1[2]) / c1[0], (pts[:, 3] - c1[3]) / c1[1]], 1)


def threshold_n(th, cam0, cam1):
    c0 = np.asarray(cam0, dtype=np.float32).astype(np.float64)
    c1 = np.asarray(cam1, dtype=np.float32).astype(np.float64)
    return float(np.float32(th)) / (((c0[0] + c0[1]) + (c1[0] + c1[1])) / 4.0)


# ---- polynomial pieces, batched over the leading axis -------------------------------------------------
def _mul11(a, b):
    out = np.zeros(a.shape[:-1] + (10,))
    for i in range(4):
        for j in range(4):
            out[..., IDX2[i, j]] += a[..., i] * b[..., j]
    return out


def _mul21(a, b):
    out = np.zeros(a.shape[:-1] + (20,))
    for m in range(10):
        for v in range(4):
            out[..., IDX3[m, v]] += a[..., m] * b[..., v]
    return out


def epipolar_rows(P):
    """[S, 5, 4] -> [S, 5, 9]: the row of x1^T E x0 = 0 for row-major E."""
    x0, y0, x1, y1 = P[..., 0], P[..., 1], P[..., 2], P[..., 3]
    one = np.ones_like(x0)
    return np.stack([x1 * x0, x1 * y0, x1, y1 * x0, y1 * y0, y1, x0, y0, one], -1)


def eliminate5(Q):
    """Gauss-Jordan with complete pivoting on [S, 5, 9].  Returns the reduced rows, the pivot columns
    [S, 5] and ok [S]."""
    Q = Q.copy()
    S = len(Q)
    ar = np.arange(S)
    scale = np.abs(Q).reshape(S, -1).max(1)
    used = np.zeros((S, 9), dtype=bool)
    pc = np.zeros((S, 5), dtype=np.int64)
    ok = np.ones(S, dtype=bool)
    for s in range(5):
        mag = np.abs(Q[:, s:, :])
        mag = np.where(used[:, None, :], -1.0, mag)
        flat = mag.reshape(S, -1).argmax(1)  # the first maximum in row-major order
        r, c = s + flat // 9, flat % 9
        piv = Q[ar, r, c]
        with np.errstate(invalid="ignore"):
            ok &= np.abs(piv) > PIVOT_FLOOR * scale
        tmp = Q[ar, s].copy()
        Q[ar, s] = Q[ar, r]
        Q[ar, r] = tmp
        with np.errstate(all="ignore"):
            Q[ar, s] = Q[ar, s] / piv[:, None]
            for i in range(5):
                if i != s:
                    f = Q[ar, i, c].copy()
                    Q[:, i] = Q[:, i] - f[:, None] * Q[:, s]
        used[ar, c] = True
        pc[:, s] = c
    return Q, pc, ok


def _gram_schmidt(b):
    """Modified Gram-Schmidt over [S, 4, 9], in order."""
    b = b.copy()
    for k in range(4):
        for j in range(k):
            d = (b[:, k] * b[:, j]).sum(1)
            b[:, k] = b[:, k] - d[:, None] * b[:, j]
        n = np.sqrt((b[:, k] * b[:, k]).sum(1))
        with np.errstate(all="ignore"):
            b[:, k] = b[:, k] / n[:, None]
    return b


def free_columns(pc):
    S = len(pc)
    free = np.ones((S, 9), dtype=bool)
    free[np.arange(S)[:, None], pc] = False
    return np.nonzero(free)[1].reshape(S, 4)  # ascending


def null_basis_kernel(Q):
    """The canonical basis (X, Y, Z, W) [S, 4, 9] and ok [S]: the reduced null vectors with the identity
    on the free columns, orthonormalised in order."""
    R, pc, ok = eliminate5(Q)
    S = len(Q)
    ar = np.arange(S)
    F = free_columns(pc)
    b = np.zeros((S, 4, 9))
    for k in range(4):
        b[ar, k, F[:, k]] = 1.0
        for s in range(5):
            b[ar, k, pc[:, s]] = -R[ar, s, F[:, k]]
    return _gram_schmidt(b), ok


def null_basis_svd(Q):
    """The same canonical basis from an SVD null space: N inv(N[F]) has the identity on the free
    columns F; its QR with a positive diagonal is the Gram-Schmidt basis."""
    _, pc, ok = eliminate5(Q)  # the free columns only: a discrete choice, part of what z means
    F = free_columns(pc)
    S = len(Q)
    out = np.zeros((S, 4, 9))
    for i in range(S):
        if not ok[i]:
            continue
        N = np.linalg.svd(Q[i])[2][5:].T  # [9, 4]
        try:
            red = N @ np.linalg.inv(N[F[i]])
        except np.linalg.LinAlgError:
            ok[i] = False
            continue
        q, r = np.linalg.qr(red)
        out[i] = (q * np.sign(np.diag(r))).T
    return out, ok


def constraints(basis):
    """[S, 4, 9] -> the ten cubic constraints [S, 10, 20]: det E, then 2 E E^T E - tr(E E^T) E (halved:
    (E E^T - tr/2 I) E) row-major."""
    S = len(basis)
    E = basis.transpose(0, 2, 1).reshape(S, 3, 3, 4)  # entry (i, j): coefficients of x, y, z, 1
    A = np.zeros((S, 10, 20))
    m = lambda i, j, k, l: _mul11(E[:, i, j], E[:, k, l])  # noqa: E731
    A[:, 0] = (_mul21(m(1, 1, 2, 2) - m(1, 2, 2, 1), E[:, 0, 0]) - _mul21(m(1, 0, 2, 2) - m(1, 2, 2, 0), E[:, 0, 1])
               + _mul21(m(1, 0, 2, 1) - m(1, 1, 2, 0), E[:, 0, 2]))
    G = np.zeros((S, 3, 3, 10))
    for i in range(3):
        for j in range(i, 3):
            G[:, i, j] = G[:, j, i] = m(i, 0, j, 0) + m(i, 1, j, 1) + m(i, 2, j, 2)
    half = 0.5 * (G[:, 0, 0] + G[:, 1, 1] + G[:, 2, 2])
    for i in range(3):
        G[:, i, i] = G[:, i, i] - half
    for i in range(3):
        for j in range(3):
            A[:, 1 + 3 * i + j] = (_mul21(G[:, i, 0], E[:, 0, j]) + _mul21(G[:, i, 1], E[:, 1, j])
                                   + _mul21(G[:, i, 2], E[:, 2, j]))
    return A


def gauss_jordan10(A):
    """Partial pivoting on columns 0..9 of [S, 10, 20]; returns the reduced matrix and ok."""
    A = A.copy()
    S = len(A)
    ar = np.arange(S)
    scale = np.abs(A).reshape(S, -1).max(1)
    ok = np.ones(S, dtype=bool)
    for c in range(10):
        r = c + np.abs(A[:, c:, c]).argmax(1)
        piv = A[ar, r, c]
        with np.errstate(invalid="ignore"):
            ok &= np.abs(piv) > PIVOT_FLOOR * scale
        tmp = A[ar, c].copy()
        A[ar, c] = A[ar, r]
        A[ar, r] = tmp
        with np.errstate(all="ignore"):
            A[:, c] = A[:, c] / piv[:, None]
            for i in range(10):
                if i != c:
                    f = A[:, i, c].copy()
                    A[:, i] = A[:, i] - f[:, None] * A[:, c]
    return A, ok


def _polymul(a, b):
    out = np.zeros(a.shape[:-1] + (a.shape[-1] + b.shape[-1] - 1,))
    for i in range(a.shape[-1]):
        for j in range(b.shape[-1]):
            out[..., i + j] += a[..., i] * b[..., j]
    return out


def z_matrix(T):
    """Rows 4..9 of the reduced system's right half T [S, 10, 10] (columns x z^2, x z, x, y z^2, y z, y,
    z^3, z^2, z, 1) -> B [S, 3, 13]: per row the ascending coefficients of the x (4), y (4) and 1 (5)
    polynomials in z of <e> - z <f>, <g> - z <h>, <i> - z <j>."""
    S = len(T)
    B = np.zeros((S, 3, 13))
    for k in range(3):
        u, v = T[:, 4 + 2 * k], T[:, 5 + 2 * k]
        for o, base in ((0, 0), (4, 3)):  # the x and the y polynomial
            B[:, k, o + 0] = u[:, base + 2]
            B[:, k, o + 1] = u[:, base + 1] - v[:, base + 2]
            B[:, k, o + 2] = u[:, base + 0] - v[:, base + 1]
            B[:, k, o + 3] = -v[:, base + 0]
        B[:, k, 8] = u[:, 9]
        B[:, k, 9] = u[:, 8] - v[:, 9]
        B[:, k, 10] = u[:, 7] - v[:, 8]
        B[:, k, 11] = u[:, 6] - v[:, 7]
        B[:, k, 12] = -v[:, 6]
    return B


def z_determinant(B):
    """det of the 3x3 polynomial matrix: ascending coefficients [S, 11]."""
    bx, by, b1 = B[:, :, 0:4], B[:, :, 4:8], B[:, :, 8:13]
    p0 = _polymul(by[:, 1], b1[:, 2]) - _polymul(b1[:, 1], by[:, 2])
    p1 = _polymul(bx[:, 1], b1[:, 2]) - _polymul(b1[:, 1], bx[:, 2])
    p2 = _polymul(bx[:, 1], by[:, 2]) - _polymul(by[:, 1], bx[:, 2])
    return _polymul(bx[:, 0], p0) - _polymul(by[:, 0], p1) + _polymul(b1[:, 0], p2)


def _horner(p, x, deg):
    v = p[..., deg] + 0.0 * x
    for i in range(deg - 1, -1, -1):
        v = v * x + p[..., i]
    return v


def sturm_chain(c):
    """[S, 11] -> chain [S, 11, 11] (polynomial k has degree 10 - k; each is divided by its largest
    magnitude) and ok [S]."""
    S = len(c)
    ch = np.zeros((S, 11, 11))
    ok = np.ones(S, dtype=bool)

    def norm(p, deg):
        nonlocal ok
        with np.errstate(all="ignore"):
            p = p / np.abs(p).max(1)[:, None]
            ok &= np.abs(p[:, deg]) >= PIVOT_FLOOR  # false for NaN
        return p

    with np.errstate(all="ignore"):
        ch[:, 0] = norm(c, 10)
        d = np.zeros((S, 11))
        for i in range(1, 11):
            d[:, i - 1] = i * ch[:, 0, i]
        ch[:, 1] = norm(d, 9)
        for k in range(2, 11):
            a, b, d = ch[:, k - 2], ch[:, k - 1], 10 - (k - 1)  # b has degree d, a degree d + 1
            q1 = a[:, d + 1] / b[:, d]
            t = a.copy()
            for i in range(1, d + 1):
                t[:, i] = a[:, i] - q1 * b[:, i - 1]
            q0 = t[:, d] / b[:, d]
            r = np.zeros((S, 11))
            for i in range(d):
                r[:, i] = -(t[:, i] - q0 * b[:, i])
            ch[:, k] = norm(r, d - 1)
    return ch, ok


def _variations(ch, x):
    last = np.zeros(len(ch), dtype=np.int64)
    var = np.zeros(len(ch), dtype=np.int64)
    with np.errstate(all="ignore"):
        for k in range(11):
            v = _horner(ch[:, k], x, 10 - k)
            s = (v > 0).astype(np.int64) - (v < 0).astype(np.int64)
            var += (s != 0) & (last != 0) & (s != last)
            last = np.where(s != 0, s, last)
    return var


def roots_kernel(c):
    """Real roots of [S, 11] ascending: z [S, 10], n [S], ok [S]."""
    ch, ok = sturm_chain(c)
    S = len(c)
    p = ch[:, 0]
    with np.errstate(all="ignore"):
        R = 1.0 + np.abs(p[:, :10] / p[:, 10:11]).max(1)
        R = np.where(ok, R, 1.0)
        va = _variations(ch, -R)
        n = np.clip(va - _variations(ch, R), 0, 10)
        n = np.where(ok, n, 0)
        z = np.full((S, 10), np.nan)
        for k in range(int(n.max()) if S else 0):
            lo, hi = -R, R.copy()
            for _ in range(BISECTIONS):
                mid = 0.5 * (lo + hi)
                up = va - _variations(ch, mid) >= k + 1
                hi = np.where(up, mid, hi)
                lo = np.where(up, lo, mid)
            x = 0.5 * (lo + hi)
            for _ in range(NEWTONS):
                v = _horner(p, x, 10)
                d = 10.0 * p[:, 10] + 0.0 * x
                for i in range(9, 0, -1):
                    d = d * x + i * p[:, i]
                xn = x - v / d
                x = np.where(np.isfinite(xn), xn, x)
            z[:, k] = np.where(k < n, x, np.nan)
    return z, n, ok


def back_substitute(B, basis, z):
    """One root per sample (NaN: none) -> E [S, 9] of unit Frobenius norm (non-finite: dropped)."""
    with np.errstate(all="ignore"):
        rows = np.stack([np.stack([_horner(B[:, k, 0:4], z, 3), _horner(B[:, k, 4:8], z, 3),
                                   _horner(B[:, k, 8:13], z, 4)], -1) for k in range(3)], 1)  # [S, 3, 3]
        cr = np.stack([np.cross(rows[:, 0], rows[:, 1]), np.cross(rows[:, 0], rows[:, 2]),
                       np.cross(rows[:, 1], rows[:, 2])], 1)
        pick = np.abs(np.nan_to_num(cr[:, :, 2], nan=-1.0)).argmax(1)
        c = cr[np.arange(len(z)), pick]
        x, y = c[:, 0] / c[:, 2], c[:, 1] / c[:, 2]
        E = x[:, None] * basis[:, 0] + y[:, None] * basis[:, 1] + z[:, None] * basis[:, 2] + basis[:, 3]
        return E / np.sqrt((E * E).sum(1))[:, None]


def essential_5pt(P, route="kernel"):
    """P [S, 5, 4] normalised matches -> (E [S, 10, 9] with NaN rows past count, count [S], z [S, 10]);
    the candidates of a sample are in ascending z of the canonical basis."""
    P = np.asarray(P, dtype=np.float64)
    S = len(P)
    Q = epipolar_rows(P)
    basis, ok = (null_basis_kernel if route == "kernel" else null_basis_svd)(Q)
    basis = np.where(ok[:, None, None], basis, 0.0)
    A = constraints(basis)
    if route == "kernel":
        G, ok2 = gauss_jordan10(A)
        T = G[:, :, 10:]
    else:
        T = np.zeros((S, 10, 10))
        ok2 = ok.copy()
        for i in np.nonzero(ok)[0]:
            try:
                T[i] = np.linalg.solve(A[i, :, :10], A[i, :, 10:])
            except np.linalg.LinAlgError:
                ok2[i] = False
    ok = ok & ok2
    T = np.where(ok[:, None, None], T, 0.0)
    B = z_matrix(T)
    c = z_determinant(B)
    if route == "kernel":
        z, n, ok3 = roots_kernel(np.where(ok[:, None], c, 1.0))
        z[~(ok & ok3)] = np.nan
    else:
        z = np.full((S, 10), np.nan)
        for i in np.nonzero(ok & np.isfinite(c).all(1))[0]:
            r = np.roots(c[i, ::-1])
            r = np.sort(r[r.imag == 0].real)[:10]
            z[i, :len(r)] = r
    out = np.full((S, 10, 9), np.nan)
    zs = np.full((S, 10), np.nan)
    count = np.zeros(S, dtype=np.int32)
    ar = np.arange(S)
    for k in range(10):
        E = back_substitute(B, basis, z[:, k])
        good = np.isfinite(E).all(1)
        out[ar[good], count[good]] = E[good]
        zs[ar[good], count[good]] = z[good, k]
        count[good] += 1
    return out, count, zs


# ---- the estimator -----------------------------------------------------------------------------------
def sampson2(E, pts):
    """Squared Sampson distances [..., K] of models [..., 9] (row-major)."""
    E = np.asarray(E, dtype=np.float64)
    x0, y0, x1, y1 = pts[:, 0], pts[:, 1], pts[:, 2], pts[:, 3]
    e = [E[..., k, None] for k in range(9)]
    with np.errstate(all="ignore"):
        a0, a1, a2 = e[0] * x0 + e[1] * y0 + e[2], e[3] * x0 + e[4] * y0 + e[5], e[6] * x0 + e[7] * y0 + e[8]
        b0, b1 = e[0] * x1 + e[3] * y1 + e[6], e[1] * x1 + e[4] * y1 + e[7]
        num = x1 * a0 + y1 * a1 + a2
        return num * num / (a0 * a0 + a1 * a1 + b0 * b0 + b1 * b1)


def _inl(r2, th, margin=None):
    with np.errstate(all="ignore"):
        if margin is not None:
            margin.note(np.sqrt(r2), th)
        return np.isfinite(r2) & (r2 < th * th)


def eight_point(pts):
    """The unweighted linear fit projected onto the essential manifold, unit Frobenius norm."""
    Q = epipolar_rows(pts[None])[0]
    e = np.linalg.svd(Q, full_matrices=True)[2][8].reshape(3, 3)
    U, _, Vt = np.linalg.svd(e)
    E = U @ np.diag([1.0, 1.0, 0.0]) @ Vt
    return (E / np.linalg.norm(E)).reshape(9)


def local_optimisation(E, count, pts, th, margin):
    for m in LO_MULTIPLIERS:
        sel = _inl(sampson2(E, pts), m * th, margin)
        if sel.sum() < 8:
            break
        with np.errstate(all="ignore"):
            fit = eight_point(pts[sel])
        c = int(_inl(sampson2(fit, pts), th, margin).sum())
        if c >= count:
            E, count = fit, c
    return E, count


def decompose(E):
    """The four (R, t) of an essential matrix in the order (R1, +t), (R1, -t), (R2, +t), (R2, -t)."""
    U, _, Vt = np.linalg.svd(np.asarray(E, dtype=np.float64).reshape(3, 3))
    if np.linalg.det(U) < 0:
        U[:, 2] = -U[:, 2]
    if np.linalg.det(Vt) < 0:
        Vt[2] = -Vt[2]
    W = np.array([[0.0, -1, 0], [1, 0, 0], [0, 0, 1]])
    R1, R2, t = U @ W @ Vt, U @ W.T @ Vt, U[:, 2]
    return [(R1, t), (R1, -t), (R2, t), (R2, -t)]


def depths(R, t, pts):
    """(lambda0, lambda1) [K] of lambda1 x1 = lambda0 R x0 + t by the 2x2 normal equations."""
    X0 = np.concatenate([pts[:, :2], np.ones((len(pts), 1))], 1)
    b = np.concatenate([pts[:, 2:], np.ones((len(pts), 1))], 1)
    a = X0 @ np.asarray(R, dtype=np.float64).T
    aa, bb, ab = (a * a).sum(1), (b * b).sum(1), (a * b).sum(1)
    at, bt = a @ t, b @ t
    with np.errstate(all="ignore"):
        det = aa * bb - ab * ab
        return (ab * bt - at * bb) / det, (aa * bt - ab * at) / det, np.sqrt(aa), np.sqrt(bb)


def _front(R, t, pts, margin=None):
    l0, l1, na, nb = depths(R, t, pts)
    with np.errstate(all="ignore"):
        if margin is not None and len(pts):
            g = np.concatenate([np.abs(l0) * na, np.abs(l1) * nb])  # against the baseline's unit length
            g = g[np.isfinite(g)]
            if len(g):
                margin.value = min(margin.value, float(g.min()))
        return (l0 > 0) & (l1 > 0)


def essential_from(R, t):
    tx = np.array([[0.0, -t[2], t[1]], [t[2], 0.0, -t[0]], [-t[1], t[0], 0.0]])
    return (tx @ R).reshape(9)


def pose_errors(R, t, T_gt):
    """relative_pose_error (geometry/epipolar.py:127-155) in float64; T_gt: the [R|t] row of 12."""
    T = np.asarray(T_gt, dtype=np.float32).astype(np.float64).reshape(12)
    R = np.asarray(R, dtype=np.float64).reshape(3, 3)
    t = np.asarray(t, dtype=np.float64).reshape(3)
    Rg, tg = T[:9].reshape(3, 3), T[9:]
    n = max(np.linalg.norm(t) * np.linalg.norm(tg), 1e-10)
    te = math.degrees(math.acos(min(max(float(t @ tg) / n, -1.0), 1.0)))
    te = min(te, 180.0 - te)
    re = abs(math.degrees(math.acos(min(max((np.trace(R.T @ Rg) - 1.0) / 2.0, -1.0), 1.0))))
    return te, re, max(te, re)


def ransac_relpose(pts_px, cam0, cam1, th, max_iters=2000, confidence=0.9999, seed=0, T_gt=None, route="kernel"):
    """pts_px [K, 4] pixel rows (x0, y0, x1, y1); cam = (fx, fy, cx, cy).  Returns the info fields, R
    (fp32 [3, 3]), t (fp32 [3]), inliers [K] bool, the errors, the trace and the margin."""
    pts = normalise(pts_px, cam0, cam1)
    K = len(pts)
    th = threshold_n(th, cam0, cam1)
    margin = _Margin()
    out = {"success": 0, "num_matches": K, "num_inliers": 0, "best_t": -1, "best_minimal_count": 0, "rounds": 0,
           "valid_samples": 0, "candidates_scored": 0, "R": np.eye(3, dtype=np.float32),
           "t": np.zeros(3, dtype=np.float32), "inliers": np.zeros(K, dtype=bool), "trace": [],
           "t_err": math.inf, "r_err": math.inf, "rel_pose_error": math.inf}
    best_min, best_lo, E_lo = -1, -1, None
    done = 0
    while K >= 5 and done < max_iters:
        ts = list(range(done, min(done + ROUND, max_iters)))
        done = ts[-1] + 1
        out["rounds"] += 1
        idx = [sample5(seed, t, K) for t in ts]
        keep = [i for i, s in enumerate(idx) if s is not None]
        out["valid_samples"] += len(keep)
        cands, ids, zs = np.zeros((0, 9)), [], []
        if keep:
            E, cnt, z = essential_5pt(pts[np.array([idx[i] for i in keep])], route)
            for row, i in enumerate(keep):
                ids += [(ts[i], j) for j in range(cnt[row])]
                zs += z[row, :cnt[row]].tolist()
            cands = np.concatenate([E[row, :cnt[row]] for row in range(len(keep))]) if ids else cands
        out["candidates_scored"] += len(ids)
        if ids:
            r2 = sampson2(cands, pts)
            counts = _inl(r2, th).sum(1)
            out["trace"].append((tuple(ids), tuple(int(c) for c in counts)))
            k = int(np.argmax(counts))  # the first of equal counts: lowest t, then lowest candidate
            near = counts >= max(best_min, int(counts[k])) - 1
            margin.note(np.sqrt(r2[near]), th)
            for o in np.nonzero(counts == counts[k])[0]:
                if o != k and ids[o][0] == ids[k][0] and counts[k] > best_min:
                    # a tie inside one sample hangs on the order of two roots
                    margin.value = min(margin.value, abs(zs[o] - zs[k]) / max(abs(zs[o]), abs(zs[k])))
            if counts[k] > best_min:
                best_min, out["best_t"] = int(counts[k]), ids[k][0]
                E1, c = local_optimisation(cands[k], best_min, pts, th, margin)
                if c > best_lo:
                    best_lo, E_lo = c, E1
        else:
            out["trace"].append(((), ()))
        if best_lo >= 5:
            with np.errstate(divide="ignore"):
                lhs, rhs = done * np.log1p(-((best_lo / K) ** 5)), math.log1p(-confidence)
            margin.note(lhs, rhs)
            if lhs <= rhs:
                break
    out["best_minimal_count"] = max(best_min, 0)
    out["margin"] = margin.value
    if E_lo is None or not np.isfinite(E_lo).all():
        return out
    inl = _inl(sampson2(E_lo, pts), th, margin)
    four = decompose(E_lo)
    front = [int(_front(R, t, pts[inl], margin).sum()) for R, t in four]
    order = sorted(range(4), key=lambda i: -front[i])
    margin.value = min(margin.value, (front[order[0]] - front[order[1]]) / max(front[order[0]], 1))
    out["margin"] = margin.value
    if front[order[0]] == 0:
        return out
    R32, t32 = four[order[0]][0].astype(np.float32), four[order[0]][1].astype(np.float32)
    Rd, td = R32.astype(np.float64), t32.astype(np.float64)
    mask = _inl(sampson2(essential_from(Rd, td), pts), th, margin) & _front(Rd, td, pts, margin)
    out["margin"] = margin.value
    if mask.sum() < 5:
        return out
    out.update(success=1, num_inliers=int(mask.sum()), R=R32, t=t32, inliers=mask)
    if T_gt is not None:
        out["t_err"], out["r_err"], out["rel_pose_error"] = pose_errors(Rd, td, T_gt)
    return out


def info_row(out):
    return np.array([out[k] for k in INFO_FIELDS], dtype=np.int32)


def estimate_pair(kpts0, kpts1, matches0, cam0, cam1, th, num0=None, num1=None, T_gt=None, **options):
    """One pair in keypoint form: the restatement's outputs in keypoints0 slot order."""
    pts, slots = live_matches(kpts0, kpts1, matches0, num0, num1)
    out = ransac_relpose(pts, cam0, cam1, th, T_gt=T_gt, **options)
    mask = np.zeros(len(kpts0), dtype=bool)
    mask[slots] = out["inliers"]
    out["inliers_slots"], out["m_kpts"] = mask, pts.astype(np.float32)
    return out
