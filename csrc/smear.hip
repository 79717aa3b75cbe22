// Native link smearing for MI355X: one table-driven level kernel serves APE
// and the three levels of HYP (role of the reference's lib/gauge_ape.cu,
// lib/gauge_hyp.cu and their kernels; re-derived).
//
// Every level has the shape, for output slot o with link direction mu_o,
//   out[o](x) = Proj[ c0 cen[mu_o](x)
//                     + c1 sum_{k < ns_o} staple(src[a_ok], src[b_ok];
//                                                mu_o, eta_ok)(x) ],
//   staple(A, B; mu, eta)(x) = B(x) A(x+eta) B(x+mu)^dag
//                            + B(x-eta)^dag A(x-eta) B(x-eta+mu),
// on complex-double fields in the oracle layout: cen [4][2][Vcb][3][3], src
// [Ns][2][Vcb][3][3] and out [No][2][Vcb][3][3] (a slot is addressed like a
// direction). An output with ns = 0 copies its centre link through,
// unprojected (the t links of spatial APE).
//
// One thread per (site, slot), both parities in one launch, the slots of a
// site in adjacent lanes: the up to 12 outputs of a site read overlapping
// links and meet in the same cache lines. A slot's table entry is one packed
// 64-bit word in the kernel arguments, picked by a select chain over SGPRs,
// so no lane indexes memory for it. For one staple direction the three
// neighbour indices are formed and all six link loads issued before the
// first product. The projection is a template parameter: each kernel
// carries one projection's registers only.
#include <hip/hip_runtime.h>

#include "common.h"
#include "launch_setup.h"
#include "su3_project.h"

namespace {

constexpr int SMEAR_BLOCK = 128;

// word o: bits 0-1 mu, 2-3 ns, then per staple k at 4 + 10 k: eta (2 bits),
// a (4 bits), b (4 bits)
struct SmearWords {
  unsigned long long w[QA_SMEAR_MAX_OUT];
};

// cb index of x + d1 e_m1 + d2 e_m2 (m1 != m2, |d| <= 1), periodic; the
// coordinates stay in registers because every array index is a constant
__device__ __forceinline__ long shifted_cb(const int x[4], int m1, int d1,
                                           int m2, int d2, const LatDims &d) {
  int y[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    int v = x[k] + (k == m1 ? d1 : 0) + (k == m2 ? d2 : 0);
    v = v >= d.X[k] ? v - d.X[k] : v;
    v = v < 0 ? v + d.X[k] : v;
    y[k] = v;
  }
  return cb_from_coords(y, d);
}

}  // namespace

template <int PROJ>
__global__ __launch_bounds__(SMEAR_BLOCK) void k_smear_level(
    cd *__restrict__ out, const cd *__restrict__ src,
    const cd *__restrict__ cen, LatDims d, int No, SmearWords tb, double c0,
    double c1) {
  const long t = (long)blockIdx.x * SMEAR_BLOCK + threadIdx.x;
  const long V = d.Vcb;
  if (t >= 2 * V * No) return;
  const long site = t / No;
  const int o = (int)(t - site * No);
  const int parity = site >= V ? 1 : 0;
  const int op = 1 - parity;
  const long i = site - (long)parity * V;
  unsigned long long w = tb.w[0];
#pragma unroll
  for (int k = 1; k < QA_SMEAR_MAX_OUT; ++k) w = o == k ? tb.w[k] : w;
  const int mu = (int)(w & 3), ns = (int)((w >> 2) & 3);

  M3 M;
  load_link(M, cen, V, mu, parity, i);
  if (ns == 0) {
    store_link(out, V, o, parity, i, M);
    return;
  }
  int xc[4];
  coords_from_cb(xc, i, d, parity);
  const long x_pmu = shifted_cb(xc, mu, +1, -1, 0, d);

  M3 S;
#pragma unroll
  for (int k = 0; k < 9; ++k) S[k / 3][k % 3] = {0.0, 0.0};
#pragma nounroll
  for (int k = 0; k < ns; ++k) {
    const unsigned e = (unsigned)(w >> (4 + 10 * k));
    const int eta = (int)(e & 3), a = (int)((e >> 2) & 15),
              b = (int)((e >> 6) & 15);
    const long x_pe = shifted_cb(xc, eta, +1, -1, 0, d);
    const long x_me = shifted_cb(xc, eta, -1, -1, 0, d);
    const long x_me_pmu = shifted_cb(xc, eta, -1, mu, +1, d);
    M3 b0, a1, b2, b3, a4, b5, tm, st;
    load_link(b0, src, V, b, parity, i);
    load_link(a1, src, V, a, op, x_pe);
    load_link(b2, src, V, b, op, x_pmu);
    load_link(b3, src, V, b, op, x_me);
    load_link(a4, src, V, a, op, x_me);
    load_link(b5, src, V, b, parity, x_me_pmu);
    mat_mul(tm, b0, a1);
    mat_mul_dag(st, tm, b2);
    mat_acc(S, st);
    mat_dag_mul(tm, b3, a4);
    mat_mul(st, tm, b5);
    mat_acc(S, st);
  }
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 3; ++c)
      M[r][c] = {c0 * M[r][c].re + c1 * S[r][c].re,
                 c0 * M[r][c].im + c1 * S[r][c].im};
  if constexpr (PROJ == QA_SMEAR_PROJ_POLAR)
    project_polar(M);
  else
    project_gs(M);
  store_link(out, V, o, parity, i, M);
}

void launch_smear_level(const SmearLevelCall &c, hipStream_t st) {
  LatDims d = lat_dims(c.lat);
  SmearWords tb{};
  for (int o = 0; o < c.No; ++o) {
    unsigned long long w = (unsigned)c.mu[o] | ((unsigned)c.ns[o] << 2);
    for (int k = 0; k < c.ns[o]; ++k)
      w |= (unsigned long long)((unsigned)c.eta[o][k] |
                                ((unsigned)c.a[o][k] << 2) |
                                ((unsigned)c.b[o][k] << 6))
           << (4 + 10 * k);
    tb.w[o] = w;
  }
  const long threads = 2 * c.lat.Vcb * c.No;
  const int grid = (int)((threads + SMEAR_BLOCK - 1) / SMEAR_BLOCK);
  if (c.proj == QA_SMEAR_PROJ_POLAR)
    hipLaunchKernelGGL(k_smear_level<QA_SMEAR_PROJ_POLAR>, dim3(grid),
                       dim3(SMEAR_BLOCK), 0, st, (cd *)c.out,
                       (const cd *)c.src, (const cd *)c.cen, d, c.No, tb, c.c0,
                       c.c1);
  else
    hipLaunchKernelGGL(k_smear_level<QA_SMEAR_PROJ_GS>, dim3(grid),
                       dim3(SMEAR_BLOCK), 0, st, (cd *)c.out,
                       (const cd *)c.src, (const cd *)c.cen, d, c.No, tb, c.c0,
                       c.c1);
}
