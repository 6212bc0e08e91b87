// Batched five-point LO-RANSAC for the relative pose (include/lightglue_mi355x.h: lg_ransac_relpose,
// lg_essential_5pt): what the reference's relative-pose estimators do for
// gluefactory/eval/utils.py:94-129, one workgroup of 256 threads per pair and one launch per batch.
//
//   phase 0   the pair's live matches are compacted in slot order into m_kpts (§10k's ballot prefix
//             scan) and, when they fit, staged in LDS as normalised fp64 rows (x0, y0, x1, y1)
//   rounds    256 samples at a time.  Solve: one sample per thread, Nistér's five-point solver with its
//             10x20 elimination and its Sturm chain in per-thread private arrays; the candidates go to
//             a per-pair workspace and their ids into an LDS list through a workgroup prefix sum.
//             Score: one candidate per thread against every match (all lanes read the same LDS row, a
//             broadcast), so lanes whose sample had few roots do not idle behind one that had ten;
//             the round's best is a workgroup argmax with the candidate index in the key
//   LO        after a round that raised the best minimal count: 8 unweighted linear eight-point fits
//             with shrinking thresholds, by the whole workgroup (45 sums, jacobi9 of dlt_common.h),
//             each projected onto the essential manifold
//   result    the kept E decomposed, the cheirality vote, R and t in fp32, and the mask and the pose
//             errors those fp32 values give in fp64
//
// All arithmetic is fp64 on the fp32 inputs.  Every branch that reaches a barrier is taken on values
// every thread read from LDS or from the call, so it is workgroup-uniform.  No atomics: the same input
// gives the same bits, alone or inside any batch.  The translation unit is built with
// -ffp-contract=off, so a residual is the same number in every pass that classifies with it.
#include <hip/hip_runtime.h>

#include <cmath>

#include "dlt_common.h"
#include "kernels.h"

namespace lg {
namespace {

constexpr int RP_DRAWS = 64;  // a sample whose five indices need more draws is invalid
constexpr int RP_LO_STEPS = 8;
constexpr int RP_BISECTIONS = 48, RP_NEWTONS = 4;
constexpr double RP_FLOOR = 1e-12;  // relative: a smaller pivot or Sturm leading coefficient rejects the sample
constexpr int RP_MAX_CAND = EV_THREADS * 10;

// degree-2 monomials of (x, y, z, 1): v_i v_j, i <= j, in lexicographic order; degree-3 monomials in
// Nistér's column order: x^3 y^3 x^2y xy^2 x^2z x^2 y^2z y^2 xyz xy | xz^2 xz x | yz^2 yz y | z^3 z^2 z 1
__constant__ unsigned char kIdx2[4][4] = {{0, 1, 2, 3}, {1, 4, 5, 6}, {2, 5, 7, 8}, {3, 6, 8, 9}};
__constant__ unsigned char kIdx3[10][4] = {{0, 2, 4, 5},     {2, 3, 8, 9},     {4, 8, 10, 11},   {5, 9, 11, 12},
                                           {3, 1, 6, 7},     {8, 6, 13, 14},   {9, 7, 14, 15},   {10, 13, 16, 17},
                                           {11, 14, 17, 18}, {12, 15, 18, 19}};

struct RpShared {
  double pts[RH_LDS_MATCHES * 4];
  double red[EV_WAVES * 45];
  double jA[81], jV[81];
  double Ekept[9], Efit[9], Ebest[9];
  double pose[24];  // R1, R2 (row-major), t, pad
  unsigned long long key[EV_WAVES];
  int cnt[EV_WAVES], cnt2[EV_WAVES];
  unsigned short list[RP_MAX_CAND];
};

__device__ inline uint64_t rp_mix64(uint64_t z) {  // splitmix64's finaliser
  z += 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// ---- polynomial pieces ------------------------------------------------------------------------------
__device__ inline void mul11(const double* a, const double* b, double* o) {
  for (int k = 0; k < 10; ++k) o[k] = 0.0;
  for (int i = 0; i < 4; ++i)
    for (int j = 0; j < 4; ++j) o[kIdx2[i][j]] += a[i] * b[j];
}
// o = a b - c d
__device__ inline void mul11_diff(const double* a, const double* b, const double* c, const double* d, double* o) {
  double u[10], v[10];
  mul11(a, b, u);
  mul11(c, d, v);
  for (int k = 0; k < 10; ++k) o[k] = u[k] - v[k];
}
__device__ inline void mul21(const double* a, const double* b, double* o) {
  for (int k = 0; k < 20; ++k) o[k] = 0.0;
  for (int m = 0; m < 10; ++m)
    for (int v = 0; v < 4; ++v) o[kIdx3[m][v]] += a[m] * b[v];
}
// o[0 .. na + nb - 2] = a b (ascending coefficients)
__device__ inline void polymul(const double* a, int na, const double* b, int nb, double* o) {
  for (int k = 0; k < na + nb - 1; ++k) o[k] = 0.0;
  for (int i = 0; i < na; ++i)
    for (int j = 0; j < nb; ++j) o[i + j] += a[i] * b[j];
}
__device__ inline double horner(const double* p, int deg, double x) {
  double v = p[deg];
  for (int i = deg - 1; i >= 0; --i) v = v * x + p[i];
  return v;
}

// the chain polynomial divided by its largest magnitude; false when its leading coefficient is
// below the floor (or nothing is finite)
__device__ inline bool sturm_norm(double* p, int deg) {
  double m = 0.0;
  for (int i = 0; i <= deg; ++i) m = fmax(m, fabs(p[i]));
  for (int i = 0; i <= deg; ++i) p[i] = p[i] / m;
  return fabs(p[deg]) >= RP_FLOOR;
}

// sign changes of the chain at x, zeros skipped
__device__ inline int sturm_variations(const double (*ch)[11], double x) {
  int last = 0, var = 0;
  for (int k = 0; k < 11; ++k) {
    const double v = horner(ch[k], 10 - k, x);
    const int s = v > 0.0 ? 1 : v < 0.0 ? -1 : 0;
    if (s != 0) {
      var += (last != 0 && s != last) ? 1 : 0;
      last = s;
    }
  }
  return var;
}

// Nistér's five-point solver.  P: five normalised matches (x0, y0, x1, y1).  Writes
// up to 10 essential matrices (row-major, unit Frobenius norm, ascending z) to out[9 * j] and returns
// their number; nothing past them is written.
__device__ __noinline__ int rp_solve(const double (&P)[5][4], double* out) {
  // 1. the null space of the 5x9 epipolar system: Gauss-Jordan with complete pivoting, the reduced
  //    vectors with the identity on the free columns, modified Gram-Schmidt in order
  double Q[5][9];
  double scale = 0.0;
  for (int i = 0; i < 5; ++i) {
    const double x0 = P[i][0], y0 = P[i][1], x1 = P[i][2], y1 = P[i][3];
    Q[i][0] = x1 * x0, Q[i][1] = x1 * y0, Q[i][2] = x1, Q[i][3] = y1 * x0, Q[i][4] = y1 * y0, Q[i][5] = y1;
    Q[i][6] = x0, Q[i][7] = y0, Q[i][8] = 1.0;
    for (int k = 0; k < 9; ++k) scale = fmax(scale, fabs(Q[i][k]));
  }
  int pc[5];
  unsigned used = 0;
  for (int s = 0; s < 5; ++s) {
    int br = s, bc = 0;
    double bm = -1.0;
    for (int r = s; r < 5; ++r)
      for (int c = 0; c < 9; ++c) {
        const double a = (used >> c & 1u) ? -1.0 : fabs(Q[r][c]);
        if (a > bm) bm = a, br = r, bc = c;  // the first maximum in row-major order
      }
    const double piv = Q[br][bc];
    if (!(fabs(piv) > RP_FLOOR * scale)) return 0;
    for (int k = 0; k < 9; ++k) {
      const double a = Q[s][k];
      Q[s][k] = Q[br][k], Q[br][k] = a;
    }
    for (int k = 0; k < 9; ++k) Q[s][k] = Q[s][k] / piv;
    for (int i = 0; i < 5; ++i) {
      if (i == s) continue;
      const double f = Q[i][bc];
      for (int k = 0; k < 9; ++k) Q[i][k] = Q[i][k] - f * Q[s][k];
    }
    used |= 1u << bc;
    pc[s] = bc;
  }
  double bs[4][9];
  {
    int k = 0;
    for (int f = 0; f < 9; ++f) {
      if (used >> f & 1u) continue;
      for (int e = 0; e < 9; ++e) bs[k][e] = 0.0;
      bs[k][f] = 1.0;
      for (int s = 0; s < 5; ++s) bs[k][pc[s]] = -Q[s][f];
      ++k;
    }
  }
  for (int k = 0; k < 4; ++k) {
    for (int j = 0; j < k; ++j) {
      double d = 0.0;
      for (int e = 0; e < 9; ++e) d += bs[k][e] * bs[j][e];
      for (int e = 0; e < 9; ++e) bs[k][e] = bs[k][e] - d * bs[j][e];
    }
    double n = 0.0;
    for (int e = 0; e < 9; ++e) n += bs[k][e] * bs[k][e];
    n = sqrt(n);
    for (int e = 0; e < 9; ++e) bs[k][e] = bs[k][e] / n;
  }

  // 2. the ten cubic constraints: det E, then (E E^T - tr(E E^T) / 2 I) E row-major
  double A[10][20];
  {
    double Ec[9][4];  // entry e of E: the coefficients of x, y, z, 1
    for (int e = 0; e < 9; ++e)
      for (int k = 0; k < 4; ++k) Ec[e][k] = bs[k][e];
    double d2[10], u[20], v[20], w[20];
    mul11_diff(Ec[4], Ec[8], Ec[5], Ec[7], d2);
    mul21(d2, Ec[0], u);
    mul11_diff(Ec[3], Ec[8], Ec[5], Ec[6], d2);
    mul21(d2, Ec[1], v);
    mul11_diff(Ec[3], Ec[7], Ec[4], Ec[6], d2);
    mul21(d2, Ec[2], w);
    for (int k = 0; k < 20; ++k) A[0][k] = (u[k] - v[k]) + w[k];
    double G[3][3][10];
    for (int i = 0; i < 3; ++i)
      for (int j = i; j < 3; ++j) {
        double a[10], b[10], c[10];
        mul11(Ec[3 * i], Ec[3 * j], a);
        mul11(Ec[3 * i + 1], Ec[3 * j + 1], b);
        mul11(Ec[3 * i + 2], Ec[3 * j + 2], c);
        for (int k = 0; k < 10; ++k) G[i][j][k] = (a[k] + b[k]) + c[k];
      }
    for (int k = 0; k < 10; ++k) {
      const double half = 0.5 * ((G[0][0][k] + G[1][1][k]) + G[2][2][k]);
      G[0][0][k] = G[0][0][k] - half, G[1][1][k] = G[1][1][k] - half, G[2][2][k] = G[2][2][k] - half;
    }
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < i; ++j)
        for (int k = 0; k < 10; ++k) G[i][j][k] = G[j][i][k];
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 3; ++j) {
        mul21(G[i][0], Ec[j], u);
        mul21(G[i][1], Ec[3 + j], v);
        mul21(G[i][2], Ec[6 + j], w);
        for (int k = 0; k < 20; ++k) A[1 + 3 * i + j][k] = (u[k] + v[k]) + w[k];
      }
  }

  // 3. Gauss-Jordan with partial pivoting on columns 0 .. 9
  scale = 0.0;
  for (int i = 0; i < 10; ++i)
    for (int k = 0; k < 20; ++k) scale = fmax(scale, fabs(A[i][k]));
  for (int c = 0; c < 10; ++c) {
    int br = c;
    double bm = fabs(A[c][c]);
    for (int r = c + 1; r < 10; ++r) {
      const double a = fabs(A[r][c]);
      if (a > bm) bm = a, br = r;
    }
    const double piv = A[br][c];
    if (!(fabs(piv) > RP_FLOOR * scale)) return 0;
    for (int k = 0; k < 20; ++k) {
      const double a = A[c][k];
      A[c][k] = A[br][k], A[br][k] = a;
    }
    for (int k = 0; k < 20; ++k) A[c][k] = A[c][k] / piv;
    for (int i = 0; i < 10; ++i) {
      if (i == c) continue;
      const double f = A[i][c];
      for (int k = 0; k < 20; ++k) A[i][k] = A[i][k] - f * A[c][k];
    }
  }

  // 4. <e> - z <f>, <g> - z <h>, <i> - z <j>: per row the x (4), y (4) and 1 (5) polynomials in z,
  //    ascending; their 3x3 determinant, degree 10
  double Bz[3][13];
  for (int k = 0; k < 3; ++k) {
    const double* u = &A[4 + 2 * k][10];
    const double* v = &A[5 + 2 * k][10];
    for (int o = 0; o < 2; ++o) {
      const int base = 3 * o;
      Bz[k][4 * o + 0] = u[base + 2];
      Bz[k][4 * o + 1] = u[base + 1] - v[base + 2];
      Bz[k][4 * o + 2] = u[base + 0] - v[base + 1];
      Bz[k][4 * o + 3] = -v[base + 0];
    }
    Bz[k][8] = u[9];
    Bz[k][9] = u[8] - v[9];
    Bz[k][10] = u[7] - v[8];
    Bz[k][11] = u[6] - v[7];
    Bz[k][12] = -v[6];
  }
  double ch[11][11];
  {
    double a[8], b[8], p0[8], p1[8], p2[8], X[11], Y[11], Z[11];
    polymul(&Bz[1][4], 4, &Bz[2][8], 5, a);
    polymul(&Bz[1][8], 5, &Bz[2][4], 4, b);
    for (int k = 0; k < 8; ++k) p0[k] = a[k] - b[k];
    polymul(&Bz[1][0], 4, &Bz[2][8], 5, a);
    polymul(&Bz[1][8], 5, &Bz[2][0], 4, b);
    for (int k = 0; k < 8; ++k) p1[k] = a[k] - b[k];
    polymul(&Bz[1][0], 4, &Bz[2][4], 4, a);
    polymul(&Bz[1][4], 4, &Bz[2][0], 4, b);
    for (int k = 0; k < 7; ++k) p2[k] = a[k] - b[k];
    polymul(&Bz[0][0], 4, p0, 8, X);
    polymul(&Bz[0][4], 4, p1, 8, Y);
    polymul(&Bz[0][8], 5, p2, 7, Z);
    for (int k = 0; k < 11; ++k) {
      ch[0][k] = (X[k] - Y[k]) + Z[k];
      if (!isfinite(ch[0][k])) return 0;
    }
  }

  // 5. the Sturm chain (polynomial k has degree 10 - k), the real roots by bisection on the chain's
  //    root count and Newton steps
  if (!sturm_norm(ch[0], 10)) return 0;
  for (int i = 1; i < 11; ++i) ch[1][i - 1] = (double)i * ch[0][i];
  if (!sturm_norm(ch[1], 9)) return 0;
  for (int k = 2; k < 11; ++k) {
    const double* a = ch[k - 2];
    const double* b = ch[k - 1];
    const int d = 10 - (k - 1);  // b has degree d, a degree d + 1
    const double q1 = a[d + 1] / b[d];
    double t[11];
    t[0] = a[0];
    for (int i = 1; i <= d; ++i) t[i] = a[i] - q1 * b[i - 1];
    const double q0 = t[d] / b[d];
    for (int i = 0; i < d; ++i) ch[k][i] = -(t[i] - q0 * b[i]);
    if (!sturm_norm(ch[k], d - 1)) return 0;
  }
  double Rb = 0.0;
  for (int i = 0; i < 10; ++i) Rb = fmax(Rb, fabs(ch[0][i] / ch[0][10]));
  Rb = 1.0 + Rb;
  const int va = sturm_variations(ch, -Rb);
  const int nroots = min(max(va - sturm_variations(ch, Rb), 0), 10);
  int count = 0;
  for (int k = 0; k < nroots; ++k) {
    double lo = -Rb, hi = Rb;
    for (int it = 0; it < RP_BISECTIONS; ++it) {
      const double mid = 0.5 * (lo + hi);
      if (va - sturm_variations(ch, mid) >= k + 1) hi = mid;
      else lo = mid;
    }
    double z = 0.5 * (lo + hi);
    for (int it = 0; it < RP_NEWTONS; ++it) {
      const double v = horner(ch[0], 10, z);
      double d = 10.0 * ch[0][10];
      for (int i = 9; i >= 1; --i) d = d * z + (double)i * ch[0][i];
      const double zn = z - v / d;
      if (isfinite(zn)) z = zn;
    }
    // 6. x and y from the cross product of two rows of B(z) with the largest third component
    double rw[3][3];
    for (int r = 0; r < 3; ++r)
      rw[r][0] = horner(&Bz[r][0], 3, z), rw[r][1] = horner(&Bz[r][4], 3, z), rw[r][2] = horner(&Bz[r][8], 4, z);
    double cx = 0.0, cy = 0.0, cz = 0.0, bm = -1.0;
    for (int pr = 0; pr < 3; ++pr) {
      const int i = pr == 2 ? 1 : 0, j = pr == 0 ? 1 : 2;
      const double c0 = rw[i][1] * rw[j][2] - rw[i][2] * rw[j][1];
      const double c1 = rw[i][2] * rw[j][0] - rw[i][0] * rw[j][2];
      const double c2 = rw[i][0] * rw[j][1] - rw[i][1] * rw[j][0];
      if (fabs(c2) > bm) bm = fabs(c2), cx = c0, cy = c1, cz = c2;
    }
    const double x = cx / cz, y = cy / cz;
    double E[9], n = 0.0;
    bool finite = true;
    for (int e = 0; e < 9; ++e) {
      E[e] = ((x * bs[0][e] + y * bs[1][e]) + z * bs[2][e]) + bs[3][e];
      n += E[e] * E[e];
    }
    n = sqrt(n);
    for (int e = 0; e < 9; ++e) E[e] = E[e] / n, finite = finite && isfinite(E[e]);
    if (!finite) continue;
    for (int e = 0; e < 9; ++e) out[9 * count + e] = E[e];
    ++count;
  }
  return count;
}

// ---- the estimator ----------------------------------------------------------------------------------
struct RpCam {
  double fx0, fy0, cx0, cy0, fx1, fy1, cx1, cy1;
};
struct RpPt {
  double x0, y0, x1, y1;
};

__device__ inline RpPt rp_normalise(const RpCam& k, float4 m) {
  return RpPt{((double)m.x - k.cx0) / k.fx0, ((double)m.y - k.cy0) / k.fy0, ((double)m.z - k.cx1) / k.fx1,
              ((double)m.w - k.cy1) / k.fy1};
}
__device__ inline RpPt rp_match(const RpShared& sh, const float4* gm, bool lds, const RpCam& k, int i) {
  if (lds) return RpPt{sh.pts[4 * i], sh.pts[4 * i + 1], sh.pts[4 * i + 2], sh.pts[4 * i + 3]};
  return rp_normalise(k, gm[i]);
}

// squared Sampson distance; a vanishing denominator gives inf or NaN, which no threshold accepts
__device__ inline double rp_resid2(const double (&e)[9], const RpPt& p) {
  const double a0 = e[0] * p.x0 + e[1] * p.y0 + e[2], a1 = e[3] * p.x0 + e[4] * p.y0 + e[5],
               a2 = e[6] * p.x0 + e[7] * p.y0 + e[8];
  const double b0 = e[0] * p.x1 + e[3] * p.y1 + e[6], b1 = e[1] * p.x1 + e[4] * p.y1 + e[7];
  const double num = p.x1 * a0 + p.y1 * a1 + a2;
  return num * num / (a0 * a0 + a1 * a1 + b0 * b0 + b1 * b1);
}

// lambda1 x1 = lambda0 R x0 + t by the 2x2 normal equations: both depths positive
__device__ inline bool rp_front(const double* R, const double* t, const RpPt& p) {
  const double a0 = R[0] * p.x0 + R[1] * p.y0 + R[2], a1 = R[3] * p.x0 + R[4] * p.y0 + R[5],
               a2 = R[6] * p.x0 + R[7] * p.y0 + R[8];
  const double aa = a0 * a0 + a1 * a1 + a2 * a2, bb = p.x1 * p.x1 + p.y1 * p.y1 + 1.0;
  const double ab = a0 * p.x1 + a1 * p.y1 + a2;
  const double at = a0 * t[0] + a1 * t[1] + a2 * t[2], bt = p.x1 * t[0] + p.y1 * t[1] + t[2];
  const double det = aa * bb - ab * ab;
  const double l0 = (ab * bt - at * bb) / det, l1 = (aa * bt - ab * at) / det;
  return l0 > 0.0 && l1 > 0.0;
}

// matches within th of the model in every thread's e (the same model), to every thread
__device__ inline int rp_count(RpShared& sh, const float4* gm, bool lds, const RpCam& cam, int K, const double (&e)[9],
                               double t2) {
  double n[1] = {0.0};
  for (int i = threadIdx.x; i < K; i += EV_THREADS) n[0] += rp_resid2(e, rp_match(sh, gm, lds, cam, i)) < t2 ? 1.0 : 0.0;
  block_sum(n, sh.red);
  return (int)n[0];
}

// symmetric 3x3 eigenproblem by cyclic Jacobi in registers: A's diagonal ends as the eigenvalues, V's
// columns as the eigenvectors (jacobi9's rotations and stopping rules)
__device__ inline void jacobi3(double (&A)[3][3], double (&V)[3][3]) {
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) V[i][j] = i == j ? 1.0 : 0.0;
  for (int sweep = 0; sweep < EV_SWEEPS; ++sweep) {
    if (fabs(A[0][1]) + fabs(A[0][2]) + fabs(A[1][2]) == 0.0) break;
    for (int pr = 0; pr < 3; ++pr) {
      const int p = pr == 2 ? 1 : 0, q = pr == 0 ? 1 : 2, k = 3 - p - q;
      const double apq = A[p][q];
      if (apq == 0.0) continue;
      const double app = A[p][p], aqq = A[q][q], g = 100.0 * fabs(apq);
      if (sweep > 3 && fabs(app) + g == fabs(app) && fabs(aqq) + g == fabs(aqq)) {
        A[p][q] = 0.0, A[q][p] = 0.0;
        continue;
      }
      const double theta = (aqq - app) / (2.0 * apq);
      const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
      const double cs = 1.0 / sqrt(t * t + 1.0), sn = t * cs;
      const double akp = A[k][p], akq = A[k][q];
      A[p][p] = app - t * apq, A[q][q] = aqq + t * apq, A[p][q] = 0.0, A[q][p] = 0.0;
      A[k][p] = cs * akp - sn * akq, A[p][k] = A[k][p];
      A[k][q] = sn * akp + cs * akq, A[q][k] = A[k][q];
      for (int r = 0; r < 3; ++r) {
        const double vp = V[r][p], vq = V[r][q];
        V[r][p] = cs * vp - sn * vq, V[r][q] = sn * vp + cs * vq;
      }
    }
  }
}

// E = u1 s1 v1^T + u2 s2 v2^T + ..: the two leading right singular vectors, u_i = E v_i / s_i and the
// completing u3 = u1 x u2, v3 = v1 x v2 (both determinants positive), through a Jacobi on E^T E
__device__ inline void rp_svd(const double (&E)[9], double (&U)[3][3], double (&Vv)[3][3]) {
  double M[3][3], V[3][3];
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) M[i][j] = (E[i] * E[j] + E[3 + i] * E[3 + j]) + E[6 + i] * E[6 + j];
  jacobi3(M, V);
  int i1 = 0;
  if (M[1][1] > M[i1][i1]) i1 = 1;
  if (M[2][2] > M[i1][i1]) i1 = 2;
  int i2 = i1 == 0 ? 1 : 0;
  for (int k = 0; k < 3; ++k)
    if (k != i1 && M[k][k] > M[i2][i2]) i2 = k;
  const int idx[2] = {i1, i2};
  for (int c = 0; c < 2; ++c) {
    const int s = idx[c];
    const double sg = sqrt(M[s][s]);
    for (int r = 0; r < 3; ++r) {
      Vv[r][c] = V[r][s];
      U[r][c] = ((E[3 * r] * V[0][s] + E[3 * r + 1] * V[1][s]) + E[3 * r + 2] * V[2][s]) / sg;
    }
  }
  U[0][2] = U[1][0] * U[2][1] - U[2][0] * U[1][1];
  U[1][2] = U[2][0] * U[0][1] - U[0][0] * U[2][1];
  U[2][2] = U[0][0] * U[1][1] - U[1][0] * U[0][1];
  Vv[0][2] = Vv[1][0] * Vv[2][1] - Vv[2][0] * Vv[1][1];
  Vv[1][2] = Vv[2][0] * Vv[0][1] - Vv[0][0] * Vv[2][1];
  Vv[2][2] = Vv[0][0] * Vv[1][1] - Vv[1][0] * Vv[0][1];
}

// the projection onto the essential manifold (singular values 1, 1, 0), unit Frobenius norm
__device__ inline void rp_project(const double (&E)[9], double (&o)[9]) {
  double U[3][3], V[3][3];
  rp_svd(E, U, V);
  double n = 0.0;
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) {
      o[3 * i + j] = U[i][0] * V[j][0] + U[i][1] * V[j][1];
      n += o[3 * i + j] * o[3 * i + j];
    }
  n = sqrt(n);
  for (int k = 0; k < 9; ++k) o[k] = o[k] / n;
}

// Local optimisation from the model in sh.Ekept with `kept` inliers; returns the kept count, the kept
// model is left in sh.Ekept.  Called by the whole workgroup.
__device__ inline int rp_local_optimisation(RpShared& sh, const float4* gm, bool lds, const RpCam& cam, int K, double th,
                                            int kept) {
  const int tid = threadIdx.x;
  const double t2 = th * th;
#pragma nounroll
  for (int s = 0; s < RP_LO_STEPS; ++s) {
    const double mult = s == 0 ? 3.0 : s == 1 ? 2.5 : s == 2 ? 2.0 : s == 3 ? 1.5 : 1.0;
    const double tm = mult * th, tm2 = tm * tm;
    double ek[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) ek[k] = sh.Ekept[k];
    // the upper triangle of sum q q^T over the selected matches; its last entry is their number
    double S[45] = {};
    for (int i = tid; i < K; i += EV_THREADS) {
      const RpPt p = rp_match(sh, gm, lds, cam, i);
      if (!(rp_resid2(ek, p) < tm2)) continue;
      const double q[9] = {p.x1 * p.x0, p.x1 * p.y0, p.x1, p.y1 * p.x0, p.y1 * p.y0, p.y1, p.x0, p.y0, 1.0};
      int o = 0;
#pragma unroll
      for (int a = 0; a < 9; ++a)
#pragma unroll
        for (int b = a; b < 9; ++b) S[o++] += q[a] * q[b];
    }
    block_sum(S, sh.red);
    if (S[44] < 8.0) break;  // too few to fit: the optimisation ends with what it kept
    __syncthreads();         // every thread has read the partials
    if (tid == 0)
#pragma unroll
      for (int k = 0; k < 45; ++k) sh.red[k] = S[k];
    __syncthreads();
    if (tid < 81) {
      const int a = min(tid / 9, tid % 9), b = max(tid / 9, tid % 9);
      sh.jA[tid] = sh.red[a * 9 - a * (a - 1) / 2 + (b - a)];
      sh.jV[tid] = tid / 9 == tid % 9 ? 1.0 : 0.0;
    }
    __syncthreads();
    if (tid < 64) {
      jacobi9(sh.jA, sh.jV, tid);
      wave_sync();
      if (tid == 0) {
        int best = 0;
        double ev = sh.jA[0];
        for (int k = 1; k < 9; ++k)
          if (sh.jA[k * 9 + k] < ev) ev = sh.jA[k * 9 + k], best = k;
        double e[9], f[9];
        for (int k = 0; k < 9; ++k) e[k] = sh.jV[k * 9 + best];
        rp_project(e, f);
        for (int k = 0; k < 9; ++k) sh.Efit[k] = f[k];
      }
    }
    __syncthreads();
    double ef[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) ef[k] = sh.Efit[k];
    const int cf = rp_count(sh, gm, lds, cam, K, ef, t2);
    if (cf >= kept) {
      kept = cf;
      __syncthreads();  // every thread has read Ekept
      if (tid < 9) sh.Ekept[tid] = sh.Efit[tid];
      __syncthreads();
    }
  }
  return kept;
}

struct RpState {
  int best_min, best_t, best_lo, rounds, valid, cands;
};

__device__ inline void rp_rounds(RpShared& sh, const float4* gm, bool lds, const RpCam& cam, int K, double th,
                                 int max_iters, double log_fail, uint64_t seed, double* ws, RpState& st) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const double t2 = th * th;
  const uint64_t seed_mix = rp_mix64(seed);
  for (int r = 0;; ++r) {
    // ---- solve: sample t, its candidates into the workspace rows of this thread
    const int t = r * EV_THREADS + tid;
    int n = 0;
    bool valid = false;
    if (t < max_iters) {
      int ix[5] = {-1, -1, -1, -1, -1}, got = 0;
      const uint64_t base = seed_mix + ((uint64_t)(uint32_t)t << 16);
      for (int d = 0; d < RP_DRAWS && got < 5; ++d) {
        const int idx = (int)(((rp_mix64(base + (uint64_t)d) >> 32) * (uint64_t)K) >> 32);
        if (idx == ix[0] || idx == ix[1] || idx == ix[2] || idx == ix[3]) continue;  // unset ones are -1
        ix[got++] = idx;
      }
      valid = got == 5;
      if (valid) {
        double P[5][4];
        for (int k = 0; k < 5; ++k) {
          const RpPt p = rp_match(sh, gm, lds, cam, ix[k]);
          P[k][0] = p.x0, P[k][1] = p.y0, P[k][2] = p.x1, P[k][3] = p.y1;
        }
        n = rp_solve(P, ws + (size_t)tid * 90);
      }
    }
    // ---- the candidates' ids in (sample, root) order: a workgroup exclusive prefix sum of n
    int inc = n;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const int o = __shfl_up(inc, off, 64);
      inc += lane >= off ? o : 0;
    }
    const int nvalid = __popcll(__ballot(valid));
    if (lane == 63) sh.cnt[wave] = inc;
    if (lane == 0) sh.cnt2[wave] = nvalid;
    __syncthreads();
    int off0 = inc - n, total = 0, vsum = 0;
#pragma unroll
    for (int w = 0; w < EV_WAVES; ++w) {
      off0 += w < wave ? sh.cnt[w] : 0;
      total += sh.cnt[w];
      vsum += sh.cnt2[w];
    }
    for (int j = 0; j < n; ++j) sh.list[off0 + j] = (unsigned short)(tid * 16 + j);
    __syncthreads();  // the list and the workspace rows are visible to the workgroup
    // ---- score: one candidate per thread, the division-free form of resid2 < t2
    unsigned long long key = 0ull;
    for (int c = tid; c < total; c += EV_THREADS) {
      const int id = sh.list[c];
      const double* src = ws + ((size_t)(id >> 4) * 10 + (id & 15)) * 9;
      double e[9];
#pragma unroll
      for (int k = 0; k < 9; ++k) e[k] = src[k];
      int count = 0;
      for (int i = 0; i < K; ++i) {
        const RpPt p = rp_match(sh, gm, lds, cam, i);
        const double a0 = e[0] * p.x0 + e[1] * p.y0 + e[2], a1 = e[3] * p.x0 + e[4] * p.y0 + e[5],
                     a2 = e[6] * p.x0 + e[7] * p.y0 + e[8];
        const double b0 = e[0] * p.x1 + e[3] * p.y1 + e[6], b1 = e[1] * p.x1 + e[4] * p.y1 + e[7];
        const double num = p.x1 * a0 + p.y1 * a1 + a2;
        count += num * num < t2 * (a0 * a0 + a1 * a1 + b0 * b0 + b1 * b1) ? 1 : 0;
      }
      // highest count, then lowest sample, then lowest candidate index
      const unsigned long long k2 = ((unsigned long long)(count + 1) << 12) | (unsigned long long)(4095 - id);
      key = k2 > key ? k2 : key;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const unsigned long long o = __shfl_xor(key, off, 64);
      key = o > key ? o : key;
    }
    if (lane == 0) sh.key[wave] = key;
    __syncthreads();
    unsigned long long kmax = sh.key[0];
#pragma unroll
    for (int w = 1; w < EV_WAVES; ++w) kmax = sh.key[w] > kmax ? sh.key[w] : kmax;
    st.valid += vsum;
    st.cands += total;
    st.rounds = r + 1;
    const int done = min((r + 1) * EV_THREADS, max_iters);
    const int rc = (int)(kmax >> 12) - 1, rid = 4095 - (int)(kmax & 4095ull);
    if (kmax != 0ull && rc > st.best_min) {
      st.best_min = rc, st.best_t = r * EV_THREADS + (rid >> 4);
      if (tid < 9) sh.Ekept[tid] = ws[((size_t)(rid >> 4) * 10 + (rid & 15)) * 9 + tid];
      __syncthreads();
      const int kept = rp_local_optimisation(sh, gm, lds, cam, K, th, rc);
      if (kept > st.best_lo) {
        st.best_lo = kept;
        if (tid < 9) sh.Ebest[tid] = sh.Ekept[tid];
      }
    }
    __syncthreads();  // list, key, cnt, Ekept and the workspace are free again; Ebest is visible
    if (done >= max_iters) break;
    if (st.best_lo >= 5) {
      const double q = (double)st.best_lo / (double)K;
      if ((double)done * log1p(-(q * q * q * q * q)) <= log_fail) break;
    }
  }
}

__global__ __launch_bounds__(EV_THREADS) void ransac_relpose_kernel(const RelposeCall c) {
  extern __shared__ __attribute__((aligned(16))) unsigned char rp_smem[];
  RpShared& sh = *reinterpret_cast<RpShared*>(rp_smem);
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int M = c.M, N = c.N;
  int n0 = M, n1 = N;
  if (c.num0) {  // a ragged batch: slots past the counts are padding, whatever they hold
    n0 = min(max(c.num0[b], 0), M);
    n1 = min(max(c.num1[b], 0), N);
  }
  const float* kp0 = c.kp0 + (int64_t)b * M * 2;
  const float* kp1 = c.kp1 + (int64_t)b * N * 2;
  const int64_t* m0 = c.m0 ? c.m0 + (int64_t)b * M : nullptr;
  float4* gm = reinterpret_cast<float4*>(c.m_kpts) + (int64_t)b * M;
  RpCam cam;
  cam.fx0 = c.cam0[4 * b], cam.fy0 = c.cam0[4 * b + 1], cam.cx0 = c.cam0[4 * b + 2], cam.cy0 = c.cam0[4 * b + 3];
  cam.fx1 = c.cam1[4 * b], cam.fy1 = c.cam1[4 * b + 1], cam.cx1 = c.cam1[4 * b + 2], cam.cy1 = c.cam1[4 * b + 3];
  const double th = (double)c.th[b] / (((cam.fx0 + cam.fy0) + (cam.fx1 + cam.fy1)) / 4.0);
  const double t2 = th * th;

  // ---- phase 0: the live matches, in slot order, into m_kpts[b][0 .. K)
  int K = 0;
  for (int64_t base = 0; base < n0; base += EV_THREADS) {
    const int64_t i = base + tid;
    int64_t j = -1;
    if (i < n0) j = m0 ? m0[i] : i;
    const bool live = j >= 0 && j < n1;
    const unsigned long long bal = __ballot(live);
    if (lane == 0) sh.cnt[wave] = __popcll(bal);
    __syncthreads();
    int off = K + __popcll(bal & ((1ull << lane) - 1ull));
#pragma unroll
    for (int w = 0; w < EV_WAVES; ++w) {
      const int cw = sh.cnt[w];
      off += w < wave ? cw : 0;
      K += cw;
    }
    if (live) gm[off] = make_float4(kp0[2 * i], kp0[2 * i + 1], kp1[2 * j], kp1[2 * j + 1]);
    __syncthreads();  // cnt is free again; the rows are visible to the workgroup
  }
  const bool lds = K <= RH_LDS_MATCHES;
  if (lds)
    for (int i = tid; i < K; i += EV_THREADS) {
      const RpPt p = rp_normalise(cam, gm[i]);
      sh.pts[4 * i] = p.x0, sh.pts[4 * i + 1] = p.y0, sh.pts[4 * i + 2] = p.x1, sh.pts[4 * i + 3] = p.y1;
    }
  __syncthreads();

  RpState st = {-1, -1, -1, 0, 0, 0};
  if (K >= 5)
    rp_rounds(sh, gm, lds, cam, K, th, c.max_iters, c.log_fail, c.seed, c.ws + (size_t)b * RP_MAX_CAND * 9, st);

  // ---- result: the kept model's four decompositions, the cheirality vote among its inliers
  bool success = st.best_lo >= 0;
  if (success) {  // uniform
    double eb[9];
    bool finite = true;
#pragma unroll
    for (int k = 0; k < 9; ++k) eb[k] = sh.Ebest[k], finite = finite && isfinite(eb[k]);
    success = finite;
    if (tid == 0 && finite) {
      double U[3][3], V[3][3];
      rp_svd(eb, U, V);
      double n = 0.0;
      for (int i = 0; i < 3; ++i) n += U[i][2] * U[i][2];
      n = sqrt(n);
      for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) {
          const double w = U[i][0] * V[j][1] - U[i][1] * V[j][0], u3 = U[i][2] * V[j][2];
          sh.pose[3 * i + j] = u3 - w;      // U W V^T
          sh.pose[9 + 3 * i + j] = u3 + w;  // U W^T V^T
        }
        sh.pose[18 + i] = U[i][2] / n;
      }
    }
  }
  __syncthreads();
  float Rf[9] = {1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f}, tf[3] = {0.f, 0.f, 0.f};
  if (success) {  // uniform
    double eb[9], tp[3], tn[3];
#pragma unroll
    for (int k = 0; k < 9; ++k) eb[k] = sh.Ebest[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) tp[k] = sh.pose[18 + k], tn[k] = -tp[k];
    double f[4] = {};
    for (int i = tid; i < K; i += EV_THREADS) {
      const RpPt p = rp_match(sh, gm, lds, cam, i);
      if (!(rp_resid2(eb, p) < t2)) continue;
      f[0] += rp_front(sh.pose, tp, p) ? 1.0 : 0.0;
      f[1] += rp_front(sh.pose, tn, p) ? 1.0 : 0.0;
      f[2] += rp_front(sh.pose + 9, tp, p) ? 1.0 : 0.0;
      f[3] += rp_front(sh.pose + 9, tn, p) ? 1.0 : 0.0;
    }
    block_sum(f, sh.red);
    int pick = 0;
#pragma unroll
    for (int k = 1; k < 4; ++k)
      if (f[k] > f[pick]) pick = k;
    if (f[pick] < 1.0) success = false;
    else {
#pragma unroll
      for (int k = 0; k < 9; ++k) Rf[k] = (float)sh.pose[(pick >> 1) * 9 + k];
#pragma unroll
      for (int k = 0; k < 3; ++k) tf[k] = (float)((pick & 1) ? tn[k] : tp[k]);
    }
  }
  // ---- the mask of the fp32 pose: a Sampson inlier of E = [t]x R in front of both cameras
  double Rd[9], td[3], ed[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) Rd[k] = Rf[k];
#pragma unroll
  for (int k = 0; k < 3; ++k) td[k] = tf[k];
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    ed[j] = td[1] * Rd[6 + j] - td[2] * Rd[3 + j];
    ed[3 + j] = td[2] * Rd[j] - td[0] * Rd[6 + j];
    ed[6 + j] = td[0] * Rd[3 + j] - td[1] * Rd[j];
  }
  int ninl = 0;
  if (success) {  // uniform
    double cnt[1] = {0.0};
    for (int i = tid; i < K; i += EV_THREADS) {
      const RpPt p = rp_match(sh, gm, lds, cam, i);
      cnt[0] += (rp_resid2(ed, p) < t2 && rp_front(Rd, td, p)) ? 1.0 : 0.0;
    }
    block_sum(cnt, sh.red);
    ninl = (int)cnt[0];
    if (ninl < 5) success = false;
  }
  uint8_t* inl = c.inliers + (int64_t)b * M;
  for (int64_t i = tid; i < M; i += EV_THREADS) {
    bool in = false;
    if (success && i < n0) {
      const int64_t j = m0 ? m0[i] : i;
      if (j >= 0 && j < n1) {
        const RpPt p = rp_normalise(cam, make_float4(kp0[2 * i], kp0[2 * i + 1], kp1[2 * j], kp1[2 * j + 1]));
        in = rp_resid2(ed, p) < t2 && rp_front(Rd, td, p);
      }
    }
    inl[i] = in ? 1 : 0;
  }
  if (tid == 0) {
    float* Ro = c.R + (int64_t)b * 9;
    float* to = c.t + (int64_t)b * 3;
#pragma unroll
    for (int k = 0; k < 9; ++k) Ro[k] = success ? Rf[k] : (k % 4 == 0 ? 1.f : 0.f);
#pragma unroll
    for (int k = 0; k < 3; ++k) to[k] = success ? tf[k] : 0.f;
    int* o = c.info + (int64_t)b * 8;
    o[0] = success ? 1 : 0, o[1] = K, o[2] = success ? ninl : 0, o[3] = st.best_t, o[4] = max(st.best_min, 0);
    o[5] = st.rounds, o[6] = st.valid, o[7] = st.cands;
    if (c.err) {
      float te = INFINITY, re = INFINITY;
      if (success) {  // relative_pose_error (geometry/epipolar.py:127-155) on the fp32 pose
        const float* T = c.T_gt + (int64_t)b * 12;
        const double deg = 180.0 / 3.14159265358979323846;
        double tr = 0.0, dot = 0.0, nt = 0.0, ng = 0.0;
#pragma unroll
        for (int k = 0; k < 9; ++k) tr += Rd[k] * (double)T[k];
#pragma unroll
        for (int k = 0; k < 3; ++k) dot += td[k] * (double)T[9 + k], nt += td[k] * td[k], ng += (double)T[9 + k] * (double)T[9 + k];
        const double nn = fmax(sqrt(nt) * sqrt(ng), 1e-10);
        double a = acos(fmin(fmax(dot / nn, -1.0), 1.0)) * deg;
        a = fmin(a, 180.0 - a);
        const double r = fabs(acos(fmin(fmax((tr - 1.0) / 2.0, -1.0), 1.0)) * deg);
        te = (float)a, re = (float)r;
      }
      c.err[3 * b] = te, c.err[3 * b + 1] = re, c.err[3 * b + 2] = fmaxf(te, re);
    }
  }
}

__global__ __launch_bounds__(64) void essential_5pt_kernel(const float* pts, int S, double* E, int* count) {
  const int s = blockIdx.x * 64 + threadIdx.x;
  if (s >= S) return;
  double P[5][4];
  for (int k = 0; k < 5; ++k)
    for (int j = 0; j < 4; ++j) P[k][j] = pts[(size_t)s * 20 + 4 * k + j];
  count[s] = rp_solve(P, E + (size_t)s * 90);
}

}  // namespace

size_t ransac_relpose_workspace_bytes(int B) { return (size_t)B * RP_MAX_CAND * 9 * sizeof(double); }

hipError_t ransac_relpose(const RelposeCall& c, hipStream_t st) {
  static_assert(sizeof(RpShared) <= 160 * 1024, "RpShared exceeds a CU's LDS");
  hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(ransac_relpose_kernel),
                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)sizeof(RpShared));
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(ransac_relpose_kernel, dim3(c.B), dim3(EV_THREADS), sizeof(RpShared), st, c);
  return hipGetLastError();
}

hipError_t essential_5pt(const float* pts, int S, double* E, int* count, hipStream_t st) {
  hipLaunchKernelGGL(essential_5pt_kernel, dim3((S + 63) / 64), dim3(64), 0, st, pts, S, E, count);
  return hipGetLastError();
}

}  // namespace lg
