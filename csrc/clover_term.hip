// Clover-term construction for MI355X (role of the reference's
// computeCloverQuda chain: kernels/field_strength_tensor.cuh +
// clover_compute.cuh + clover_invert.cuh with its trlogA output, rebuilt for
// this project's conventions, see ops/reference.py clover_matrix): from the
// oracle gauge tensor [4][2][Vcb][3][3] (complex double, periodic, single
// rank) one launch writes
//   A      = 1 + coef sum_{mu<nu} sigma_munu (x) F_munu,  coef = kappa csw,
//   A^-1,
// both packed (per chirality block 6 real diagonal entries, then the 15
// lower-triangular complex entries row-major) straight into the chunked
// CloverField layout [2][72/w][Vcb][w], plus per-workgroup partials of
// tr log A and of the number of non-positive pivots, and optionally the six
// F_munu = (Q - Q^dag)/(8i) - trace as [6][2][Vcb][3][3].
//
// A workgroup serves CL_SITES = 32 sites of one parity with 192 threads.
// Stage 1, all 192 lanes: thread t owns (site t / 6, plane t % 6). The plane
// is lane data (hops and link directions are selects, the wrap is applied at
// every hop so extent 2 works). The lane walks the four leaves in the order
// of field_strength; U_mu(x) stays in registers for leaves 1 and 4, and each
// of U_nu(x), U_mu(x-mu), U_nu(x-nu) for the two consecutive leaves that
// share it. The traceless hermitian F goes to LDS as 9 reals (13.5 KB).
// Stage 2, wave 0: lane l owns (site l % 32, chirality l / 32). It forms its
// 6x6 hermitian block from the six F in LDS with the entries of sigma taken
// from generated/sigma.h at compile time, factors it L D L^dag with real
// pivots (sum log|d|, count of d <= 0), inverts through N = L^-1 as
// N^dag D^-1 N and stores 36 + 36 reals as chunk rows: consecutive lanes are
// consecutive sites, so a chunk-row store is 16 contiguous bytes per lane.
// The partials are xor-butterfly sums over the wave: no atomics, bitwise
// reproducible.
//
// VALU fp64, not MFMA, for the reason at the top of clover_force.hip: chained
// 3x3 products at lane-dependent addresses, and a 6x6 factorisation per lane.
#include <hip/hip_runtime.h>

#include "common.h"
#include "launch_setup.h"
#include "launchers.h"
#include "su3_double.h"
#include "generated/sigma.h"

namespace {

constexpr int CL_SITES = 32;
constexpr int CL_BLOCK = 6 * CL_SITES;  // three full waves

struct Site {
  int y0, y1, y2, y3;
  int par;
};

__device__ __forceinline__ int wrap(int v, int n) {
  return v >= n ? v - n : (v < 0 ? v + n : v);
}

// one hop of dlt = +-1 along a lane-dependent direction (as in
// clover_force.hip): selects, no branch; even extents flip the parity
__device__ __forceinline__ Site hop_sel(const Site &w, int dir, int dlt,
                                        const LatDims &d) {
  Site r;
  r.y0 = wrap(w.y0 + (dir == 0 ? dlt : 0), d.X[0]);
  r.y1 = wrap(w.y1 + (dir == 1 ? dlt : 0), d.X[1]);
  r.y2 = wrap(w.y2 + (dir == 2 ? dlt : 0), d.X[2]);
  r.y3 = wrap(w.y3 + (dir == 3 ? dlt : 0), d.X[3]);
  r.par = w.par ^ 1;
  return r;
}

__device__ __forceinline__ void load_at(M3 &L, const cd *__restrict__ g,
                                        const LatDims &d, int dir,
                                        const Site &w) {
  long lex =
      (((long)w.y3 * d.X[2] + w.y2) * d.X[1] + w.y1) * d.X[0] + w.y0;
  load_link(L, g, d.Vcb, dir, w.par, lex >> 1);
}

// Q = sum of the four leaves of plane (mu, nu) at c0, in the leaf order of
// ops/reference.py field_strength
__device__ __forceinline__ void leaf_sum(M3 &Q, const cd *__restrict__ g,
                                         const LatDims &d, const Site &c0,
                                         int mu, int nu) {
  const Site xpm = hop_sel(c0, mu, +1, d), xpn = hop_sel(c0, nu, +1, d);
  const Site xmm = hop_sel(c0, mu, -1, d), xmn = hop_sel(c0, nu, -1, d);
  M3 Um, A, B, T, S;
  load_at(Um, g, d, mu, c0);
  {
    M3 Un;
    load_at(Un, g, d, nu, c0);
    // leaf 1: U_mu(x) U_nu(x+mu) U_mu(x+nu)^d U_nu(x)^d
    load_at(A, g, d, nu, xpm);
    load_at(B, g, d, mu, xpn);
    mat_mul_dag(T, A, B);
    mat_mul(S, Um, T);
    mat_mul_dag(Q, S, Un);
    // leaf 2: U_nu(x) [U_nu(x-mu) U_mu(x-mu+nu)]^d U_mu(x-mu)
    load_at(A, g, d, nu, xmm);
    load_at(B, g, d, mu, hop_sel(xmm, nu, +1, d));
    mat_mul(T, A, B);
    mat_mul_dag(S, Un, T);
  }
  M3 Bm;
  load_at(Bm, g, d, mu, xmm);
  mat_mul(T, S, Bm);
  mat_acc(Q, T);
  // leaf 3: [U_nu(x-mu-nu) U_mu(x-mu)]^d U_mu(x-mu-nu) U_nu(x-nu)
  const Site xmmn = hop_sel(xmm, nu, -1, d);
  load_at(A, g, d, nu, xmmn);
  mat_mul(S, A, Bm);
  M3 Bn;
  load_at(Bn, g, d, nu, xmn);
  load_at(A, g, d, mu, xmmn);
  mat_mul(T, A, Bn);
  mat_dag_mul(B, S, T);
  mat_acc(Q, B);
  // leaf 4: U_nu(x-nu)^d U_mu(x-nu) U_nu(x+mu-nu) U_mu(x)^d
  load_at(A, g, d, mu, xmn);
  load_at(B, g, d, nu, hop_sel(xpm, nu, -1, d));
  mat_mul(T, A, B);
  mat_dag_mul(S, Bn, T);
  mat_mul_dag(T, S, Um);
  mat_acc(Q, T);
}

// entry (a, b) of a hermitian 3x3 held as 3 diagonal reals then the upper
// triangle (0,1), (0,2), (1,2); a and b are compile-time after unrolling
__device__ __forceinline__ cd herm_entry(const double *f, int a, int b) {
  if (a == b) return {f[a], 0.0};
  const int k = 3 + 2 * (a + b - 1);
  return {f[k], a < b ? f[k + 1] : -f[k + 1]};
}

__device__ __forceinline__ cd mul_i_pow(const cd &v, int k) {
  return k == 0 ? v
                : k == 1 ? cd{-v.im, v.re}
                         : k == 2 ? cd{-v.re, -v.im} : cd{v.im, -v.re};
}

// lower triangle, row-major: (1,0), (2,0), (2,1), (3,0), ...
__device__ __forceinline__ constexpr int tri(int i, int j) {
  return i * (i - 1) / 2 + j;
}

// chirality block CHI of 1 + coef sum_P sigma_P (x) F_P: rows and columns
// r = 3 spin + colour, dg the real diagonal, lo the lower triangle
template <int CHI>
__device__ __forceinline__ void clover_block(double (&dg)[6], cd (&lo)[15],
                                             const double *f, double coef) {
#pragma unroll
  for (int k = 0; k < 6; ++k) dg[k] = 0.0;
#pragma unroll
  for (int k = 0; k < 15; ++k) lo[k] = {0.0, 0.0};
#pragma unroll
  for (int p = 0; p < 6; ++p)
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      const int t = SIGMA_COL[p][2 * CHI + s] - 2 * CHI;
      const int ph = SIGMA_PHASE[p][2 * CHI + s];
      if (t > s) continue;  // the upper spin block is the lower one's dagger
#pragma unroll
      for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int b = 0; b < 3; ++b) {
          const int i = 3 * s + a, j = 3 * t + b;
          if (j > i) continue;
          const cd v = mul_i_pow(herm_entry(f + 9 * p, a, b), ph);
          if (i == j)
            dg[i] += v.re;
          else
            lo[tri(i, j)] = cadd(lo[tri(i, j)], v);
        }
    }
#pragma unroll
  for (int k = 0; k < 6; ++k) dg[k] = fma(coef, dg[k], 1.0);
#pragma unroll
  for (int k = 0; k < 15; ++k) lo[k] = {coef * lo[k].re, coef * lo[k].im};
}

// in place A = L D L^dag: dg becomes the real pivots, lo the unit lower L.
// Returns sum log|d|; nbad counts pivots <= 0.
__device__ __forceinline__ double ldl_factor(double (&dg)[6], cd (&lo)[15],
                                             int &nbad) {
  double logdet = 0.0;
  nbad = 0;
#pragma unroll
  for (int j = 0; j < 6; ++j) {
    cd v[6];  // v_k = L_jk d_k
#pragma unroll
    for (int k = 0; k < j; ++k) {
      const cd l = lo[tri(j, k)];
      v[k] = {l.re * dg[k], l.im * dg[k]};
      dg[j] -= l.re * v[k].re + l.im * v[k].im;
    }
    const double dj = dg[j];
    nbad += dj <= 0.0 ? 1 : 0;
    logdet += log(fabs(dj));
    const double rinv = 1.0 / dj;
#pragma unroll
    for (int i = j + 1; i < 6; ++i) {
      cd a = lo[tri(i, j)];
#pragma unroll
      for (int k = 0; k < j; ++k) {
        const cd p = cmulj(lo[tri(i, k)], v[k]);
        a = {a.re - p.re, a.im - p.im};
      }
      lo[tri(i, j)] = {a.re * rinv, a.im * rinv};
    }
  }
  return logdet;
}

// A^-1 = N^dag D^-1 N with N = L^-1 (unit lower), from the factors
__device__ __forceinline__ void ldl_invert(double (&idg)[6], cd (&ilo)[15],
                                           const double (&dg)[6],
                                           const cd (&lo)[15]) {
  cd n[15];
#pragma unroll
  for (int i = 1; i < 6; ++i)
#pragma unroll
    for (int j = 0; j < i; ++j) {
      cd s = lo[tri(i, j)];
#pragma unroll
      for (int k = j + 1; k < i; ++k)
        s = cadd(s, cmul(lo[tri(i, k)], n[tri(k, j)]));
      n[tri(i, j)] = {-s.re, -s.im};
    }
  double r[6];
#pragma unroll
  for (int k = 0; k < 6; ++k) r[k] = 1.0 / dg[k];
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    double s = r[i];
#pragma unroll
    for (int k = i + 1; k < 6; ++k) {
      const cd m = n[tri(k, i)];
      s = fma(r[k], m.re * m.re + m.im * m.im, s);
    }
    idg[i] = s;
#pragma unroll
    for (int j = 0; j < i; ++j) {
      // (N^dag D^-1 N)_ij = sum_{k >= i} conj(N_ki) N_kj / d_k, N_ii = 1
      const cd nij = n[tri(i, j)];
      cd a = {r[i] * nij.re, r[i] * nij.im};
#pragma unroll
      for (int k = i + 1; k < 6; ++k) {
        const cd p = cjmul(n[tri(k, i)], n[tri(k, j)]);
        a = {fma(r[k], p.re, a.re), fma(r[k], p.im, a.im)};
      }
      ilo[tri(i, j)] = a;
    }
  }
}

template <typename R> struct ChunkOf;
template <> struct ChunkOf<double> { using type = double2; };
template <> struct ChunkOf<float> { using type = float4; };

// the 36 packed reals of chirality chi at site i as chunk rows of
// [2][72/w][Vcb][w]; 36 is a multiple of w, so rows never straddle blocks
template <typename R>
__device__ __forceinline__ void store_packed(R *__restrict__ out, long Vcb,
                                             int parity, int chi, long i,
                                             const double (&dg)[6],
                                             const cd (&lo)[15]) {
  using C = typename ChunkOf<R>::type;
  constexpr int W = sizeof(C) / sizeof(R);
  R p[36];
#pragma unroll
  for (int k = 0; k < 6; ++k) p[k] = (R)dg[k];
#pragma unroll
  for (int k = 0; k < 15; ++k) {
    p[6 + 2 * k] = (R)lo[k].re;
    p[7 + 2 * k] = (R)lo[k].im;
  }
  C *rows = reinterpret_cast<C *>(out) +
            ((long)parity * (72 / W) + chi * (36 / W)) * Vcb + i;
#pragma unroll
  for (int c = 0; c < 36 / W; ++c) {
    C v;
    if constexpr (W == 2) {
      v = C{p[2 * c], p[2 * c + 1]};
    } else {
      v = C{p[4 * c], p[4 * c + 1], p[4 * c + 2], p[4 * c + 3]};
    }
    rows[(long)c * Vcb] = v;
  }
}

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) v += __shfl_xor(v, m, 64);
  return v;
}

}  // namespace

// factor == 0 stops after stage 1 (F only; the stage-2 share of the kernel
// time is measured against it)
template <typename R>
__global__ __launch_bounds__(CL_BLOCK) void k_clover_term(
    R *__restrict__ data, R *__restrict__ inv, double *__restrict__ partials,
    cd *__restrict__ fmunu, const cd *__restrict__ g, LatDims d, double coef,
    int nb, int factor) {
  __shared__ double f_lds[CL_BLOCK * 9];
  const int t = threadIdx.x;
  const int parity = (int)blockIdx.x >= nb ? 1 : 0;
  const long base = (long)((int)blockIdx.x - parity * nb) * CL_SITES;
  const long V = d.Vcb;

  {
    const int plane = t % 6;
    const long i = base + t / 6;
    if (i < V) {
      // planes (0,1),(0,2),(0,3),(1,2),(1,3),(2,3)
      const int mu = plane < 3 ? 0 : (plane < 5 ? 1 : 2);
      const int nu = plane < 3 ? plane + 1 : (plane < 5 ? plane - 1 : 3);
      int xc[4];
      coords_from_cb(xc, i, d, parity);
      const Site c0{xc[0], xc[1], xc[2], xc[3], parity};
      M3 Q;
      leaf_sum(Q, g, d, c0, mu, nu);
      // F = (Q - Q^dag)/(8i): F_ab = ((q_ab.im + q_ba.im)
      //                               - i (q_ab.re - q_ba.re)) / 8
      double f[9];
#pragma unroll
      for (int a = 0; a < 3; ++a) f[a] = 0.25 * Q[a][a].im;
      const double tr = ((f[0] + f[1]) + f[2]) / 3.0;
#pragma unroll
      for (int a = 0; a < 3; ++a) f[a] -= tr;
#pragma unroll
      for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = a + 1; b < 3; ++b) {
          f[3 + 2 * (a + b - 1)] = 0.125 * (Q[a][b].im + Q[b][a].im);
          f[4 + 2 * (a + b - 1)] = -0.125 * (Q[a][b].re - Q[b][a].re);
        }
#pragma unroll
      for (int k = 0; k < 9; ++k) f_lds[t * 9 + k] = f[k];
      if (fmunu) {
        M3 F;
#pragma unroll
        for (int a = 0; a < 3; ++a)
#pragma unroll
          for (int b = 0; b < 3; ++b) F[a][b] = herm_entry(f, a, b);
        store_link(fmunu, V, plane, parity, i, F);
      }
    }
  }
  if (!factor) return;  // uniform over the grid
  __syncthreads();
  if (t >= 64) return;  // wave-uniform: stage 2 is wave 0

  const int chi = t >> 5;
  const long i = base + (t & 31);
  double logdet = 0.0;
  int nbad = 0;
  if (i < V) {
    double f[54];
#pragma unroll
    for (int k = 0; k < 54; ++k) f[k] = f_lds[(t & 31) * 54 + k];
    double dg[6], idg[6];
    cd lo[15], ilo[15];
    if (chi == 0)
      clover_block<0>(dg, lo, f, coef);
    else
      clover_block<1>(dg, lo, f, coef);
    store_packed<R>(data, V, parity, chi, i, dg, lo);
    logdet = ldl_factor(dg, lo, nbad);
    ldl_invert(idg, ilo, dg, lo);
    store_packed<R>(inv, V, parity, chi, i, idg, ilo);
  }
  // every lane of wave 0 is here: sites past the tail add zeros
  logdet = wave_sum(logdet);
  const double bad = wave_sum((double)nbad);
  if (t == 0) {
    partials[2 * blockIdx.x] = logdet;
    partials[2 * blockIdx.x + 1] = bad;
  }
}

long clover_term_blocks(long Vcb) { return (Vcb + CL_SITES - 1) / CL_SITES; }

void launch_clover_term(const CloverTermCall &c, hipStream_t st) {
  LatDims d = lat_dims(c.lat);
  const int nb = (int)clover_term_blocks(c.lat.Vcb);
  const dim3 grid(2 * nb), block(CL_BLOCK);
  cd *f = (cd *)c.fmunu;
  const cd *g = (const cd *)c.u;
  const int factor = c.factor ? 1 : 0;
  if (c.prec == 0)
    hipLaunchKernelGGL(k_clover_term<double>, grid, block, 0, st,
                       (double *)c.data, (double *)c.inv, c.partials, f, g, d,
                       c.coef, nb, factor);
  else
    hipLaunchKernelGGL(k_clover_term<float>, grid, block, 0, st,
                       (float *)c.data, (float *)c.inv, c.partials, f, g, d,
                       c.coef, nb, factor);
}
