// Path-table gauge kernels for MI355X (role of the reference's
// kernels/gauge_force.cuh, gauge_path.cuh and gauge_loop_trace.cuh with
// gauge_path_helper.cuh — re-derived): one kernel walks an arbitrary table
// of signed-direction link paths per (site, direction) and serves the MD
// force (optionally fused with the momentum update), the raw path product
// and, in a second kernel, per-site traces of closed loops.
//
// Operates on the oracle complex-double tensor [4][2][Vcb][3][3], periodic,
// single rank. A step s = +-(nu+1): s > 0 multiplies by U_nu(y) and moves
// y -> y+nu; s < 0 moves y -> y-nu first and multiplies by U_nu(y)^dag.
//
// A path is 8 int8 steps (zero padded) read as ONE 64-bit word through a
// const __restrict__ pointer: the table is wave-uniform, so the word comes
// in by a scalar load, every step is a uniform branch and all lanes walk
// the same path. The step direction is a runtime value; coordinates are
// four scalars updated under a uniform switch and every M3 index is a
// compile-time constant, so nothing is runtime-indexed (no scratch).
#include <hip/hip_runtime.h>

#include "common.h"
#include "launch_setup.h"
#include "su3_double.h"

namespace {

// running site of a path walk: coordinates, all inside the lattice
struct Walker {
  int y0, y1, y2, y3;
  int par;
};

// one hop of dlt = +-1 along `dir` (wave-uniform) with periodic wrap. The
// wrap is applied at every hop, so any accumulated displacement stays in
// range against any extent >= 2; every extent is even, so each hop flips
// the parity, wrapped or not.
__device__ __forceinline__ void hop(Walker &w, int dir, int dlt,
                                    const LatDims &d) {
  switch (dir) {
    case 0: {
      int v = w.y0 + dlt;
      w.y0 = v >= d.X[0] ? v - d.X[0] : (v < 0 ? v + d.X[0] : v);
      break;
    }
    case 1: {
      int v = w.y1 + dlt;
      w.y1 = v >= d.X[1] ? v - d.X[1] : (v < 0 ? v + d.X[1] : v);
      break;
    }
    case 2: {
      int v = w.y2 + dlt;
      w.y2 = v >= d.X[2] ? v - d.X[2] : (v < 0 ? v + d.X[2] : v);
      break;
    }
    default: {
      int v = w.y3 + dlt;
      w.y3 = v >= d.X[3] ? v - d.X[3] : (v < 0 ? v + d.X[3] : v);
      break;
    }
  }
  w.par ^= 1;
}

__device__ __forceinline__ long cb_of(const Walker &w, const LatDims &d) {
  long lex =
      (((long)w.y3 * d.X[2] + w.y2) * d.X[1] + w.y1) * d.X[0] + w.y0;
  return lex >> 1;
}

__device__ __forceinline__ void mat_copy(M3 &o, const M3 &a) {
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) o[i][j] = a[i][j];
}

__device__ __forceinline__ void mat_copy_dag(M3 &o, const M3 &a) {
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) o[i][j] = {a[j][i].re, -a[j][i].im};
}

// step k of the packed path word; a corrupt table can at worst name a wrong
// direction, never leave the lattice
__device__ __forceinline__ int step_of(unsigned long long word, int k) {
  return (int)(signed char)((word >> (8 * k)) & 0xffULL);
}

// P = ordered link product along `word` (len >= 1 steps) starting at w;
// the first link seeds the product
__device__ __forceinline__ void walk_path(M3 &P, Walker w,
                                          unsigned long long word, int len,
                                          const cd *__restrict__ g,
                                          const LatDims &d) {
  const long V = d.Vcb;
  M3 L, T;
  for (int k = 0; k < len; ++k) {
    const int s = step_of(word, k);
    const int dir = ((s < 0 ? -s : s) - 1) & 3;
    if (s > 0) {
      load_link(L, g, V, dir, w.par, cb_of(w, d));
      hop(w, dir, +1, d);
      if (k == 0) {
        mat_copy(P, L);
      } else {
        mat_mul(T, P, L);
        mat_copy(P, T);
      }
    } else {
      hop(w, dir, -1, d);
      load_link(L, g, V, dir, w.par, cb_of(w, d));
      if (k == 0) {
        mat_copy_dag(P, L);
      } else {
        mat_mul_dag(T, P, L);
        mat_copy(P, T);
      }
    }
  }
}

}  // namespace

// out_mu(x) (+)= dt * scale * E[ U_mu(x) sum_p c_p T_p(x+mu) ],
// E = TA (force) or identity (path product); flags bit 0 = TA, bit 1 =
// accumulate into out (the fused momentum update). Each thread owns the
// one link it writes: the accumulate is a plain read-modify-write.
__global__ __launch_bounds__(128) void k_gauge_path(
    cd *__restrict__ out, const cd *__restrict__ g,
    const unsigned long long *__restrict__ steps,
    const int *__restrict__ lens, const double *__restrict__ coefs, int np,
    LatDims d, int mu, double scale, double dt, int flags) {
  long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
  long V = d.Vcb;
  if (t >= 2 * V) return;
  int parity = (int)(t / V);
  long i = t - (long)parity * V;
  int xc[4];
  coords_from_cb(xc, i, d, parity);
  Walker w0{xc[0], xc[1], xc[2], xc[3], parity};
  hop(w0, mu, +1, d);  // every tail starts at x+mu

  M3 S;
#pragma unroll
  for (int k = 0; k < 9; ++k) S[k / 3][k % 3] = {0.0, 0.0};
  for (int p = 0; p < np; ++p) {
    const double c = coefs[p];
    int len = lens[p];
    len = len > 8 ? 8 : len;
    if (len <= 0) {  // empty tail: c * identity
#pragma unroll
      for (int k = 0; k < 3; ++k) S[k][k].re += c;
      continue;
    }
    M3 P;
    walk_path(P, w0, steps[p], len, g, d);
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
      for (int b = 0; b < 3; ++b) {
        S[a][b].re += c * P[a][b].re;
        S[a][b].im += c * P[a][b].im;
      }
  }

  M3 U, W, R;
  load_link(U, g, V, mu, parity, i);
  mat_mul(W, U, S);
  if (flags & 1) {  // TA[W] = (W - W^dag)/2 - tr/3
    cd tr = {0.0, 0.0};
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
      for (int b = 0; b < 3; ++b)
        R[a][b] = {0.5 * (W[a][b].re - W[b][a].re),
                   0.5 * (W[a][b].im + W[b][a].im)};
#pragma unroll
    for (int a = 0; a < 3; ++a) tr = cadd(tr, R[a][a]);
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      R[a][a].re -= tr.re / 3.0;
      R[a][a].im -= tr.im / 3.0;
    }
  } else {
    mat_copy(R, W);
  }
#pragma unroll
  for (int a = 0; a < 3; ++a)
#pragma unroll
    for (int b = 0; b < 3; ++b) {
      R[a][b].re *= scale;
      R[a][b].im *= scale;
    }
  if (flags & 2) {
    M3 O;
    load_link(O, out, V, mu, parity, i);
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
      for (int b = 0; b < 3; ++b) {
        R[a][b].re = O[a][b].re + dt * R[a][b].re;
        R[a][b].im = O[a][b].im + dt * R[a][b].im;
      }
  }
  store_link(out, V, mu, parity, i, R);
}

// tr[l][parity][i] = tr P_l(x) for every closed loop l of a flat table;
// the sum over sites is left to the caller (no reduction, no atomics)
__global__ __launch_bounds__(128) void k_loop_trace(
    cd *__restrict__ tr, const cd *__restrict__ g,
    const unsigned long long *__restrict__ steps,
    const int *__restrict__ lens, int nloops, LatDims d) {
  long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
  long V = d.Vcb;
  if (t >= 2 * V) return;
  int parity = (int)(t / V);
  long i = t - (long)parity * V;
  int xc[4];
  coords_from_cb(xc, i, d, parity);
  const Walker w0{xc[0], xc[1], xc[2], xc[3], parity};
  for (int l = 0; l < nloops; ++l) {
    int len = lens[l];
    len = len > 8 ? 8 : len;
    cd s = {3.0, 0.0};  // empty loop: tr 1
    if (len > 0) {
      M3 P;
      walk_path(P, w0, steps[l], len, g, d);
      s = cadd(cadd(P[0][0], P[1][1]), P[2][2]);
    }
    tr[((long)l * 2 + parity) * V + i] = s;
  }
}

void launch_gauge_path(const GaugePathCall &c, hipStream_t st) {
  LatDims d = lat_dims(c.lat);
  int grid = (int)((2 * c.lat.Vcb + 127) / 128);
  const long off = (long)c.mu * c.np;
  hipLaunchKernelGGL(k_gauge_path, dim3(grid), dim3(128), 0, st, (cd *)c.out,
                     (const cd *)c.u,
                     (const unsigned long long *)c.steps + off, c.lens + off,
                     c.coefs + off, c.np, d, c.mu, c.scale, c.dt,
                     (c.ta ? 1 : 0) | (c.accumulate ? 2 : 0));
}

void launch_loop_trace(const LoopTraceCall &c, hipStream_t st) {
  LatDims d = lat_dims(c.lat);
  int grid = (int)((2 * c.lat.Vcb + 127) / 128);
  hipLaunchKernelGGL(k_loop_trace, dim3(grid), dim3(128), 0, st, (cd *)c.tr,
                     (const cd *)c.u, (const unsigned long long *)c.steps,
                     c.lens, c.nloops, d);
}
