// Galerkin coarse-operator build of the fine Wilson(-clover) level:
// X [Na][Nc][Nc] and Y[0..7] [Na][Nc][Nc] (Nc = 2*Nv, complex double) straight
// from the aggregate-ordered V [Na][B][12][Nv] (ref: kernels/
// coarse_op_kernel.cuh CalculateY/VUV — re-derived for wave64 and LDS).
//
// Conventions (quda_amd/mg/galerkin.py builds the tables and operands):
//   row         ab = a*B + b, the (a, b) order of Transfer.sites_by_agg
//   k12         s*3 + c; chirality 0 = spins 0,1 (k12 < 6)
//   coarse idx  i = chi*Nv + v
//   term        t = 0 the diagonal (1 or the dense clover), t = 1 + d the hop
//               of direction d = 2*mu + fwd
//   nbr  [Na*B][8] int32   row of the d-neighbour
//   bnd  [Na*B]    uint8   bit d: the site lies on the d-face of its block
//   link [Na*B][8][3][3]   U_mu(x) fwd, U_mu(x-mu)^dag bwd
//   clov [Na*B][12][12]    dense site matrix, or null (Wilson: identity)
//   coef [8][4][4]         -kappa * P_d
//
// Every term has the same shape: with the 12 x 12 site matrix
//   D_0(x) = clov(x) or 1,   D_{1+d}(x)[(s,c),(s',c')] = coef_d[s,s'] L_d(x)[c,c']
// and the source row n_t(x) (x itself, or its d-neighbour)
//   W_t(x; k, (chi',v)) = sum_{k' in chi'} D_t(x)[k,k'] V(n_t(x); k', v)
//   M_t[a; (chi,w), (chi',v)] = sum_{x in a} sum_{k in chi} conj(V(x;k,w)) W_t
// i.e. D is applied to the neighbour's 12 x Nv block first, then a rank-6
// update per chirality. A site's hop goes to Y[d] when its bnd bit d is set
// and to X otherwise, so a workgroup handles one (aggregate, part) with
//   part 0      t = 0, all sites            -> scratch[0]
//   part 1..8   t = part, bit clear         -> scratch[part]
//   part 9..16  t = part - 8, bit set       -> Y[part - 9]
// walking only the sites of its part, QA_GK_S at a time, in ascending b. A
// second kernel sums the nine scratch slabs into X in the order t = 0..8. No
// atomics; the order of every sum is fixed by (B, Nv) alone.
#include "common.h"
#include "launchers.h"

namespace {

constexpr int QA_GK_S = 4;    // sites per LDS tile
constexpr int QA_GK_TW = 24;  // rows (w) / columns (v) of one output tile per
                              // chirality pair: 8 x 8 lanes, 3 x 3 each
constexpr int QA_GK_T = 256;  // 4 waves: wave q owns (chi, chi') = (q>>1, q&1)
constexpr int QA_GK_PARTS = 17;

// LDS per site, in doubles: A [12][TW], W [12][2][TW], D [12][12] complex
constexpr int GK_A = 12 * QA_GK_TW * 2;
constexpr int GK_W = 12 * 2 * QA_GK_TW * 2;
constexpr int GK_D = 144 * 2;
static_assert((GK_A + GK_W + GK_D) * QA_GK_S * 8 <= 65536, "static LDS limit");

__device__ __forceinline__ cplx<double> ld2(const double *p) {
  double t[2];
  load_chunk<double, 2>(p, t);
  return {t[0], t[1]};
}

__device__ __forceinline__ void st2(double *p, const cplx<double> &z) {
  chunk16 c;
  double t[2] = {z.re, z.im};
  c = *reinterpret_cast<const chunk16 *>(t);
  *reinterpret_cast<chunk16 *>(p) = c;
}

__global__ void __launch_bounds__(QA_GK_T) k_galerkin_terms(
    double *__restrict__ scratch, double *__restrict__ Y,
    const double *__restrict__ V, const int *__restrict__ nbr,
    const unsigned char *__restrict__ bnd, const double *__restrict__ link,
    const double *__restrict__ clov, const double *__restrict__ coef, long Na,
    int B, int Nv, int ntile) {
  __shared__ alignas(16) double sA[QA_GK_S * GK_A];
  __shared__ alignas(16) double sW[QA_GK_S * GK_W];
  __shared__ alignas(16) double sD[QA_GK_S * GK_D];

  // blockIdx -> (a, part, w tile, v tile); uniform over the workgroup
  long bid = blockIdx.x;
  const int tv = (int)(bid % ntile);
  bid /= ntile;
  const int tw = (int)(bid % ntile);
  bid /= ntile;
  const int part = (int)(bid % QA_GK_PARTS);
  const long a = bid / QA_GK_PARTS;
  if (a >= Na) return;
  const int t = part <= 8 ? part : part - 8;
  const int d = t - 1;
  const int want = part > 8 ? 1 : 0;  // bnd bit wanted (t > 0)
  const int w0 = tw * QA_GK_TW, v0 = tv * QA_GK_TW;
  const long rows = Na * (long)B;
  const long row0 = a * (long)B;
  const int Nc = 2 * Nv;

  const int tid = threadIdx.x;
  const int q = tid >> 6, lane = tid & 63;
  const int chi = q >> 1, chip = q & 1;
  const int ty = lane >> 3, tx = lane & 7;

  cplx<double> acc[3][3];
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 3; ++c) acc[r][c] = {0.0, 0.0};

  int cur = 0;  // next site of the aggregate to look at
  while (cur < B) {
    // the next (up to) QA_GK_S sites of this part, ascending b
    int sb[QA_GK_S];
    int nS = 0;
#pragma unroll
    for (int s = 0; s < QA_GK_S; ++s) sb[s] = 0;
    while (cur < B && nS < QA_GK_S) {
      const bool take = t == 0 || ((bnd[row0 + cur] >> d) & 1) == want;
      if (take) {
#pragma unroll
        for (int s = 0; s < QA_GK_S; ++s)
          if (s == nS) sb[s] = cur;
        ++nS;
      }
      ++cur;
    }
    if (nS == 0) break;

    // stage the conjugate-side panel A[sl][k][w] and the site matrices D
    for (int e = tid; e < QA_GK_S * 12 * QA_GK_TW; e += QA_GK_T) {
      const int w = e % QA_GK_TW;
      const int k = (e / QA_GK_TW) % 12;
      const int sl = e / (12 * QA_GK_TW);
      int b = 0;
#pragma unroll
      for (int s = 0; s < QA_GK_S; ++s)
        if (s == sl) b = sb[s];
      cplx<double> z(0.0, 0.0);
      if (sl < nS && w0 + w < Nv)
        z = ld2(V + (((row0 + b) * 12 + k) * (long)Nv + w0 + w) * 2);
      st2(sA + (long)e * 2, z);
    }
    for (int e = tid; e < QA_GK_S * 144; e += QA_GK_T) {
      const int kp = e % 12;
      const int k = (e / 12) % 12;
      const int sl = e / 144;
      int b = 0;
#pragma unroll
      for (int s = 0; s < QA_GK_S; ++s)
        if (s == sl) b = sb[s];
      cplx<double> z(0.0, 0.0);
      if (sl < nS) {
        const long ab = row0 + b;
        if (t == 0) {
          if (clov != nullptr)
            z = ld2(clov + (ab * 144 + k * 12 + kp) * 2);
          else if (k == kp)
            z = {1.0, 0.0};
        } else {
          const int s = k / 3, c = k - 3 * s, sp = kp / 3, cp = kp - 3 * sp;
          z = ld2(coef + ((d * 4 + s) * 4 + sp) * 2) *
              ld2(link + ((ab * 8 + d) * 9 + c * 3 + cp) * 2);
        }
      }
      st2(sD + (long)e * 2, z);
    }
    __syncthreads();

    // W[sl][k][chi'][v] = sum_{k6} D[sl][k][chi'*6 + k6] * Vsrc[chi'*6 + k6][v]
    for (int e = tid; e < QA_GK_S * 2 * QA_GK_TW; e += QA_GK_T) {
      const int v = e % QA_GK_TW;
      const int cp = (e / QA_GK_TW) & 1;
      const int sl = e / (2 * QA_GK_TW);
      int b = 0;
#pragma unroll
      for (int s = 0; s < QA_GK_S; ++s)
        if (s == sl) b = sb[s];
      long n = -1;
      if (sl < nS && v0 + v < Nv)
        n = t == 0 ? row0 + b : (long)nbr[(row0 + b) * 8 + d];
      const bool ok = n >= 0 && n < rows;
      cplx<double> src[6];
#pragma unroll
      for (int k6 = 0; k6 < 6; ++k6)
        src[k6] = ok ? ld2(V + ((n * 12 + cp * 6 + k6) * (long)Nv + v0 + v) * 2)
                     : cplx<double>(0.0, 0.0);
      const double *dr = sD + ((long)sl * 144 + cp * 6) * 2;
      double *wr = sW + (((long)sl * 12 * 2 + cp) * QA_GK_TW + v) * 2;
#pragma unroll
      for (int k = 0; k < 12; ++k) {
        cplx<double> z(0.0, 0.0);
#pragma unroll
        for (int k6 = 0; k6 < 6; ++k6)
          z = cfma(ld2(dr + (k * 12 + k6) * 2), src[k6], z);
        st2(wr + (long)k * 2 * QA_GK_TW * 2, z);
      }
    }
    __syncthreads();

    // rank-6 update per site: wave (chi, chi'), lane (ty, tx), 3 x 3 each
    for (int sl = 0; sl < nS; ++sl) {
      const double *ap = sA + ((long)sl * 12 + chi * 6) * QA_GK_TW * 2;
      const double *wp = sW + (((long)sl * 12 + chi * 6) * 2 + chip) *
                                  QA_GK_TW * 2;
#pragma unroll
      for (int k6 = 0; k6 < 6; ++k6) {
        cplx<double> av[3], wv[3];
#pragma unroll
        for (int r = 0; r < 3; ++r)
          av[r] = ld2(ap + ((long)k6 * QA_GK_TW + ty + 8 * r) * 2);
#pragma unroll
        for (int c = 0; c < 3; ++c)
          wv[c] = ld2(wp + ((long)k6 * 2 * QA_GK_TW + tx + 8 * c) * 2);
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
          for (int c = 0; c < 3; ++c)
            acc[r][c] = cfma_conj(av[r], wv[c], acc[r][c]);
      }
    }
    __syncthreads();  // the next tile overwrites A, D and W
  }

  double *out = part <= 8 ? scratch + ((long)part * Na + a) * Nc * (long)Nc * 2
                          : Y + ((long)(part - 9) * Na + a) * Nc * (long)Nc * 2;
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    const int w = w0 + ty + 8 * r;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const int v = v0 + tx + 8 * c;
      if (w < Nv && v < Nv)
        st2(out + (((long)chi * Nv + w) * Nc + (long)chip * Nv + v) * 2,
            acc[r][c]);
    }
  }
}

// X = scratch[0] + scratch[1] + ... + scratch[8], in that order
__global__ void k_galerkin_sum(double *__restrict__ X,
                               const double *__restrict__ scratch, long n) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  cplx<double> s = ld2(scratch + i * 2);
  for (int t = 1; t < 9; ++t) s += ld2(scratch + ((long)t * n + i) * 2);
  st2(X + i * 2, s);
}

long gk_ntile(const GalerkinCall &c) {
  return (c.Nv + QA_GK_TW - 1) / QA_GK_TW;
}

}  // namespace

bool qa_galerkin_grid_ok(const GalerkinCall &c) {
  if (!(c.Na > 0 && c.B > 0 && c.Nv > 0)) return false;
  const long nt = gk_ntile(c);
  const long lim = (1L << 31) - 1;
  const long n = c.Na * 4L * c.Nv * c.Nv;  // entries of X
  return c.Na < lim / (QA_GK_PARTS * nt * nt) && n / 256 < lim;
}

void launch_galerkin_build(const GalerkinCall &c, hipStream_t st) {
  const long nt = gk_ntile(c);
  hipLaunchKernelGGL(k_galerkin_terms,
                     dim3((unsigned)(c.Na * QA_GK_PARTS * nt * nt)),
                     dim3(QA_GK_T), 0, st, (double *)c.scratch, (double *)c.Y,
                     (const double *)c.V, c.nbr, c.bnd, (const double *)c.link,
                     (const double *)c.clov, (const double *)c.coef, c.Na, c.B,
                     c.Nv, (int)nt);
  const long n = c.Na * 4L * c.Nv * c.Nv;
  hipLaunchKernelGGL(k_galerkin_sum, dim3((unsigned)((n + 255) / 256)),
                     dim3(256), 0, st, (double *)c.X,
                     (const double *)c.scratch, n);
}
