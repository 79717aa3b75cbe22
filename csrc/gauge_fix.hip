// Native overrelaxation gauge fixing for MI355X (role of the reference's
// lib/gauge_fix_ovr.cu + gauge_fix_ovr_hit_devf.cuh: checkerboard sweeps of
// overrelaxed SU(2)-subgroup hits, Landau or Coulomb; re-derived).
//
// Works in place on the oracle complex-double tensor [4][2][Vcb][3][3].
//
// k_gauge_fix_ovr: one half-sweep. Eight lanes per site, eight sites per
// wave64: lane l < 4 owns U_l(x), lane l >= 4 owns U_{l-4}(x-mu). A lane
// keeps its link in registers for the whole kernel; a backward lane keeps
// the DAGGER of its link, so that
//     w(x) = sum_{mu<dirs} [U_mu(x) + U_mu(x-mu)^dag]
// is the plain sum of the eight register matrices and W <- r W is the same
// row update on every lane (r U^dag = (U r^dag)^dag: the backward link is
// right-multiplied by r^dag without a second code path). The four real
// numbers of an SU(2) projection are summed over the eight lanes with a
// fixed three-step xor butterfly: no LDS, no barriers, no atomics, and
// every lane ends with the same bits and forms r redundantly. Every link
// has exactly one endpoint of the active parity, so one launch reads and
// writes each of the 4V links once and is race-free.
//
// k_gauge_fix_quality: theta and the functional, one thread per site of
// both parities, per-block partials in fixed order (torch.sum finishes).
#include <hip/hip_runtime.h>

#include "common.h"
#include "launch_setup.h"
#include "reduce.h"
#include "su3_project.h"

namespace {

constexpr int FIX_BLOCK = 256;  // 32 sites of 8 lanes

// sum over the 8 lanes of one site; fp addition commutes, so the two
// partners of every butterfly step hold the same bits afterwards
__device__ __forceinline__ double site_sum(double v) {
  v += __shfl_xor(v, 1, 64);
  v += __shfl_xor(v, 2, 64);
  v += __shfl_xor(v, 4, 64);
  return v;
}

__device__ __forceinline__ void mat_dagger_if(M3 &u, bool on) {
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = i; j < 3; ++j) {
      cd a = u[i][j], b = u[j][i];
      u[i][j] = on ? cd{b.re, -b.im} : a;
      u[j][i] = on ? cd{a.re, -a.im} : b;
    }
}

// one overrelaxed hit on subgroup (P,Q): contributes the lane's matrix to
// the site's SU(2) projection (`weight` 0 for mu >= dirs), forms
//   xb = (omega a0^2 + asq) / (a0^2 + asq),
//   r  = (a0, -xb a1, -xb a2, -xb a3) / sqrt(a0^2 + xb^2 asq)
// and left-multiplies rows (P,Q) by the embedded r
template <int P, int Q>
__device__ __forceinline__ void ovr_hit(M3 &U, double weight, double omega) {
  double a0 = 0.5 * site_sum(weight * (U[P][P].re + U[Q][Q].re));
  double a1 = 0.5 * site_sum(weight * (U[P][Q].im + U[Q][P].im));
  double a2 = 0.5 * site_sum(weight * (U[P][Q].re - U[Q][P].re));
  double a3 = 0.5 * site_sum(weight * (U[P][P].im - U[Q][Q].im));
  double a0sq = a0 * a0;
  double asq = a1 * a1 + a2 * a2 + a3 * a3;
  double xb = (omega * a0sq + asq) / fmax(a0sq + asq, 1e-60);
  double k = fmax(sqrt(a0sq + xb * xb * asq), 1e-30);
  cd ra = {a0 / k, -(xb * a3) / k};
  cd rb = {-(xb * a2) / k, -(xb * a1) / k};
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    cd up = U[P][c], uq = U[Q][c];
    U[P][c] = cadd(cmul(ra, up), cmul(rb, uq));
    U[Q][c] = cadd(cmul(cd{-rb.re, rb.im}, up), cmulj(uq, ra));
  }
}

}  // namespace

// Vcb is a multiple of 8 (all four extents are even; checked on the host),
// so a wave's eight sites are all inside the lattice or all outside it: the
// butterfly below never runs in a partly masked wave, and the tail of the
// last block is masked off in whole waves.
__global__ __launch_bounds__(FIX_BLOCK) void k_gauge_fix_ovr(
    cd *__restrict__ g, LatDims d, int parity, int dirs, double omega,
    int reunit) {
  long t = (long)blockIdx.x * FIX_BLOCK + threadIdx.x;
  long i = t >> 3;
  if (i >= d.Vcb) return;
  const int mu = (int)(t & 3);
  const bool bwd = (t & 4) != 0;
  int xc[4];
  coords_from_cb(xc, i, d, parity);
  const int p = bwd ? 1 - parity : parity;
  const long j = bwd ? neighbor_cb(xc, mu, -1, d) : i;

  M3 U;
  load_link(U, g, d.Vcb, mu, p, j);
  mat_dagger_if(U, bwd);
  const double weight = mu < dirs ? 1.0 : 0.0;
  ovr_hit<0, 1>(U, weight, omega);
  ovr_hit<0, 2>(U, weight, omega);
  ovr_hit<1, 2>(U, weight, omega);
  mat_dagger_if(U, bwd);
  if (reunit) project_gs(U);
  store_link(g, d.Vcb, mu, p, j, U);
}

// re-orthonormalise every link (after the last sweep of a run that did not
// end on a reunitarising launch)
__global__ __launch_bounds__(FIX_BLOCK) void k_gauge_fix_reunit(
    cd *__restrict__ g, long nlinks) {
  long t = (long)blockIdx.x * FIX_BLOCK + threadIdx.x;
  if (t >= nlinks) return;
  M3 U;
  load_link(U, g, nlinks, 0, 0, t);
  project_gs(U);
  store_link(g, nlinks, 0, 0, t, U);
}

// partials[2*block] = sum |Delta(x)|^2, partials[2*block+1] = sum_{mu<dirs}
// Re tr U_mu(x) over the block's sites; Delta = sum_mu [A_mu(x) -
// A_mu(x-mu)], A = U - U^dag - tr(U - U^dag)/3 (no factor 1/2). A is
// linear in U, so the links are summed first and A is taken once.
__global__ __launch_bounds__(FIX_BLOCK) void k_gauge_fix_quality(
    const cd *__restrict__ g, LatDims d, int dirs,
    double *__restrict__ partials) {
  long t = (long)blockIdx.x * FIX_BLOCK + threadIdx.x;
  const long V = d.Vcb;
  double th = 0.0, fn = 0.0;
  if (t < 2 * V) {
    const int parity = t >= V ? 1 : 0;
    const long i = t - (long)parity * V;
    int xc[4];
    coords_from_cb(xc, i, d, parity);
    M3 D;
#pragma unroll
    for (int k = 0; k < 9; ++k) D[k / 3][k % 3] = {0.0, 0.0};
#pragma unroll
    for (int mu = 0; mu < 4; ++mu) {
      if (mu >= dirs) continue;
      M3 a, b;
      load_link(a, g, V, mu, parity, i);
      load_link(b, g, V, mu, 1 - parity, neighbor_cb(xc, mu, -1, d));
      fn += (a[0][0].re + a[1][1].re) + a[2][2].re;
#pragma unroll
      for (int k = 0; k < 9; ++k) {
        const int r = k / 3, c = k % 3;
        D[r][c] = {D[r][c].re + (a[r][c].re - b[r][c].re),
                   D[r][c].im + (a[r][c].im - b[r][c].im)};
      }
    }
    // tr(D - D^dag) = 2i sum Im D_kk
    const double tr3 = 2.0 * ((D[0][0].im + D[1][1].im) + D[2][2].im) / 3.0;
#pragma unroll
    for (int k = 0; k < 9; ++k) {
      const int r = k / 3, c = k % 3;
      double re = D[r][c].re - D[c][r].re;
      double im = D[r][c].im + D[c][r].im - (r == c ? tr3 : 0.0);
      th += re * re + im * im;
    }
  }
  // fixed order: wave shuffle tree, then the four waves in sequence
  __shared__ double part[2][FIX_BLOCK / 64];
  th = wave_reduce(th);
  fn = wave_reduce(fn);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) {
    part[0][wave] = th;
    part[1][wave] = fn;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    partials[2 * (long)blockIdx.x] =
        ((part[0][0] + part[0][1]) + part[0][2]) + part[0][3];
    partials[2 * (long)blockIdx.x + 1] =
        ((part[1][0] + part[1][1]) + part[1][2]) + part[1][3];
  }
}

void launch_gauge_fix_ovr(const GaugeFixCall &c, hipStream_t st) {
  LatDims d = lat_dims(c.lat);
  int grid = (int)((8 * c.lat.Vcb + FIX_BLOCK - 1) / FIX_BLOCK);
  hipLaunchKernelGGL(k_gauge_fix_ovr, dim3(grid), dim3(FIX_BLOCK), 0, st,
                     (cd *)c.u, d, c.parity, c.dirs, c.omega, c.reunit);
}

void launch_gauge_fix_reunit(void *u, long nlinks, hipStream_t st) {
  int grid = (int)((nlinks + FIX_BLOCK - 1) / FIX_BLOCK);
  hipLaunchKernelGGL(k_gauge_fix_reunit, dim3(grid), dim3(FIX_BLOCK), 0, st,
                     (cd *)u, nlinks);
}

long gauge_fix_quality_blocks(long Vcb) {
  return (2 * Vcb + FIX_BLOCK - 1) / FIX_BLOCK;
}

void launch_gauge_fix_quality(const GaugeFixCall &c, double *partials,
                              hipStream_t st) {
  LatDims d = lat_dims(c.lat);
  int grid = (int)gauge_fix_quality_blocks(c.lat.Vcb);
  hipLaunchKernelGGL(k_gauge_fix_quality, dim3(grid), dim3(FIX_BLOCK), 0, st,
                     (const cd *)c.u, d, c.dirs, partials);
}
