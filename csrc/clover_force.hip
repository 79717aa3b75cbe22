// Wilson-clover pseudofermion force for MI355X (role of the reference's
// kernels/clover_outer_product.cuh + clover_sigma_outer_product.cuh +
// clover_deriv.cuh chain — re-derived for this project's conventions, see
// quda_amd/gauge/fermion_force.py): the MD force of the unpreconditioned
// operator M = A(U) - kappa D for pairs (X_i, Y_i) with real weights c_i,
//
//   F_mu(x) = kappa TA[ U_mu(x) G1 - G2 U_mu(x)^dag
//                       + (i csw / 8) U_mu(x) C_mu(x) ].
//
// Gauge, force and momentum are the oracle complex-double tensor
// [4][2][Vcb][3][3]; X and Y are [n][2][Vcb][4][3]; periodic, single rank.
//
// k_clover_sigma_oprod, one thread per site: the six hermitian traceless
//   H_munu = Ohat + Ohat^dag,  O_ji = sum_i c_i sum_st Y_tj sigma_st X_si^*,
// kept as 9 reals per plane while the pairs are summed. A launch of its
// own: H is read at eight corners per link, fusing it would recompute it.
//
// k_clover_force, all four directions in one launch, eight lanes per
// (site, mu). Lanes 0-5 own one plaquette each, (nu, upper/lower); nu and
// the side are lane data (hops and daggers are selects, not branches). A
// lane walks its plaquette backwards from x and evaluates
//   U (H1 A1 A2 A3 + A1 H2 A2 A3 + A1 A2 H3 A3 + A1 A2 A3 H0)
// as the Horner form U (H1 S1 + A1 (H2 S2 + A2 (H3 A3 + A3 H0))) with the
// suffix products S2 = A2 A3, S1 = A1 S2: nine 3x3 products, not sixteen.
// Lane 6 forms U G1 and lane 7 -G2 U^dag = -(U G2^dag)^dag through the same
// instructions. A three-step xor butterfly sums the eight pre-TA summands;
// lane 0 projects, scales and stores, or adds dt F to the momentum it reads
// once. No LDS, no atomics, a fixed summation order.
//
// VALU fp64, not MFMA: the operands are chained 3x3 complex products at
// data-dependent addresses; v_mfma_f64_16x16x4 would need 16 independent
// 3x3 problems transposed through LDS for every product of the chain (the
// other gauge-sector kernels made the same call).
#include <hip/hip_runtime.h>

#include "common.h"
#include "launch_setup.h"
#include "su3_double.h"
#include "generated/sigma.h"

namespace {

constexpr int CF_BLOCK = 128;  // 16 (site, mu) items of 8 lanes

struct Site {
  int y0, y1, y2, y3;
  int par;
};

__device__ __forceinline__ int wrap(int v, int n) {
  return v >= n ? v - n : (v < 0 ? v + n : v);
}

// one hop of dlt = +-1 along a lane-dependent direction: four selects, no
// branch. The wrap is applied at every hop, so the site stays inside the
// lattice for any extent >= 2; extents are even, so the parity flips.
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

__device__ __forceinline__ long cb_of(const Site &w, const LatDims &d) {
  long lex =
      (((long)w.y3 * d.X[2] + w.y2) * d.X[1] + w.y1) * d.X[0] + w.y0;
  return lex >> 1;
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

__device__ __forceinline__ void mat_zero(M3 &o) {
#pragma unroll
  for (int k = 0; k < 9; ++k) o[k / 3][k % 3] = {0.0, 0.0};
}

// o += a * b
__device__ __forceinline__ void mat_mul_acc(M3 &o, const M3 &a, const M3 &b) {
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      cd s = cadd(o[i][j], cmul(a[i][0], b[0][j]));
      s = cadd(s, cmul(a[i][1], b[1][j]));
      o[i][j] = cadd(s, cmul(a[i][2], b[2][j]));
    }
}

// t = a * t
__device__ __forceinline__ void mat_lmul(M3 &t, const M3 &a) {
  M3 r;
  mat_mul(r, a, t);
#pragma unroll
  for (int k = 0; k < 9; ++k) t[k / 3][k % 3] = r[k / 3][k % 3];
}

// link of direction `dir` at `w`, daggered when `dag`
__device__ __forceinline__ void load_link_at(M3 &L, const cd *__restrict__ g,
                                             const LatDims &d, int dir,
                                             const Site &w, bool dag) {
  load_link(L, g, d.Vcb, dir, w.par, cb_of(w, d));
  mat_dagger_if(L, dag);
}

// a 4-spinor of one site: [4][3] complex
__device__ __forceinline__ void load_spinor(cd (&s)[4][3],
                                            const cd *__restrict__ f, long V,
                                            int k, int par, long i) {
  const cd *b = f + (((long)k * 2 + par) * V + i) * 12;
#pragma unroll
  for (int q = 0; q < 12; ++q) s[q / 3][q % 3] = b[q];
}

// acc += a conj(b) and acc += conj(a) b as explicit fma chains: a product
// is never a value of its own, so the compiler cannot keep the products
// that two planes have in common alive across planes (that spilled)
__device__ __forceinline__ void fma_mulj(cd &acc, const cd &a, const cd &b) {
  acc.re = fma(a.re, b.re, fma(a.im, b.im, acc.re));
  acc.im = fma(a.im, b.re, fma(-a.re, b.im, acc.im));
}
__device__ __forceinline__ void fma_jmul(cd &acc, const cd &a, const cd &b) {
  acc.re = fma(a.re, b.re, fma(a.im, b.im, acc.re));
  acc.im = fma(a.re, b.im, fma(-a.im, b.re, acc.im));
}

// plane P's share of H = O + O^dag from one pair (X already carries c_i):
// O_ji = sum_s (sigma_P Y)_sj conj(X_si). hd holds HALF the real diagonal,
// ho the upper triangle (0,1), (0,2), (1,2).
template <int P>
__device__ __forceinline__ void oprod_plane(double (&hd)[3], cd (&ho)[3],
                                            const cd (&X)[4][3],
                                            const cd (&Y)[4][3]) {
  cd Z[4][3];
  sigma_mul<P>(Z, Y);
#pragma unroll
  for (int s = 0; s < 4; ++s) {
#pragma unroll
    for (int a = 0; a < 3; ++a)
      hd[a] = fma(Z[s][a].re, X[s][a].re, fma(Z[s][a].im, X[s][a].im, hd[a]));
    fma_mulj(ho[0], Z[s][0], X[s][1]);
    fma_jmul(ho[0], Z[s][1], X[s][0]);
    fma_mulj(ho[1], Z[s][0], X[s][2]);
    fma_jmul(ho[1], Z[s][2], X[s][0]);
    fma_mulj(ho[2], Z[s][1], X[s][2]);
    fma_jmul(ho[2], Z[s][2], X[s][1]);
  }
}

// sum over the 8 lanes of one item; fp addition commutes, so both partners
// of a butterfly step hold the same bits afterwards
__device__ __forceinline__ double item_sum(double v) {
  v += __shfl_xor(v, 1, 64);
  v += __shfl_xor(v, 2, 64);
  v += __shfl_xor(v, 4, 64);
  return v;
}

}  // namespace

// h[plane][parity][i] = H_munu(x), planes (0,1),(0,2),(0,3),(1,2),(1,3),(2,3)
__global__ __launch_bounds__(CF_BLOCK) void k_clover_sigma_oprod(
    cd *__restrict__ h, const cd *__restrict__ x, const cd *__restrict__ y,
    const double *__restrict__ coef, int n, long V) {
  long t = (long)blockIdx.x * CF_BLOCK + threadIdx.x;
  if (t >= 2 * V) return;
  const int parity = t >= V ? 1 : 0;
  const long i = t - (long)parity * V;

  // H = O + O^dag: real diagonal, upper triangle (0,1), (0,2), (1,2)
  double hd[6][3];
  cd ho[6][3];
#pragma unroll
  for (int p = 0; p < 6; ++p)
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      hd[p][k] = 0.0;
      ho[p][k] = {0.0, 0.0};
    }
#pragma unroll 1
  for (int k = 0; k < n; ++k) {
    const double c = coef[k];
    cd X[4][3], Y[4][3];
    load_spinor(X, x, V, k, parity, i);
    load_spinor(Y, y, V, k, parity, i);
#pragma unroll
    for (int s = 0; s < 4; ++s)
#pragma unroll
      for (int a = 0; a < 3; ++a) X[s][a] = {c * X[s][a].re, c * X[s][a].im};
    oprod_plane<0>(hd[0], ho[0], X, Y);
    oprod_plane<1>(hd[1], ho[1], X, Y);
    oprod_plane<2>(hd[2], ho[2], X, Y);
    oprod_plane<3>(hd[3], ho[3], X, Y);
    oprod_plane<4>(hd[4], ho[4], X, Y);
    oprod_plane<5>(hd[5], ho[5], X, Y);
  }
#pragma unroll
  for (int p = 0; p < 6; ++p) {
    const double tr = ((hd[p][0] + hd[p][1]) + hd[p][2]) / 3.0;
    M3 H;
#pragma unroll
    for (int a = 0; a < 3; ++a) H[a][a] = {2.0 * (hd[p][a] - tr), 0.0};
    H[0][1] = ho[p][0];
    H[0][2] = ho[p][1];
    H[1][2] = ho[p][2];
    H[1][0] = {ho[p][0].re, -ho[p][0].im};
    H[2][0] = {ho[p][1].re, -ho[p][1].im};
    H[2][1] = {ho[p][2].re, -ho[p][2].im};
    store_link(h, V, p, parity, i, H);
  }
}

// Vcb is a multiple of 8 (even extents; checked on the host), so the 8 Vcb
// items fill whole waves and whole blocks: the butterfly never runs in a
// partly masked wave and mu is uniform over a block.
__global__ __launch_bounds__(CF_BLOCK) void k_clover_force(
    cd *__restrict__ out, const cd *__restrict__ g, const cd *__restrict__ h,
    const cd *__restrict__ x, const cd *__restrict__ y,
    const double *__restrict__ coef, int n, LatDims d, double kappa,
    double csw, double dt, int fused) {
  const long t = (long)blockIdx.x * CF_BLOCK + threadIdx.x;
  const long V = d.Vcb;
  const long item = t >> 3;
  if (item >= 8 * V) return;
  const int lane = (int)(t & 7);
  const int mu = (int)(item / (2 * V));
  const long r = item - (long)mu * 2 * V;
  const int parity = r >= V ? 1 : 0;
  const long i = r - (long)parity * V;
  int xc[4];
  coords_from_cb(xc, i, d, parity);
  const Site c0{xc[0], xc[1], xc[2], xc[3], parity};

  M3 W;
  mat_zero(W);

  if (lane < 6) {
    if (csw != 0.0) {
      const int ni = lane >> 1;
      const int nu = ni + (ni >= mu ? 1 : 0);
      const bool up = (lane & 1) == 0;
      const int s = up ? 1 : -1;
      const int a = mu < nu ? mu : nu, b = mu < nu ? nu : mu;
      const int plane = a * (7 - a) / 2 + b - a - 1;
      // H_munu = -H_numu, and the lower plaquette runs against the plane's
      // orientation
      const double w = (mu < nu ? s : -s) * csw * 0.125;

      const Site c3 = hop_sel(c0, nu, s, d);    // x + s nu
      const Site c2 = hop_sel(c3, mu, +1, d);   // x + mu + s nu
      const Site c1 = hop_sel(c2, nu, -s, d);   // x + mu
      M3 T, S, A, H;
      // A3: c3 -> x, U_nu(x)^dag (upper) or U_nu(x - nu) (lower)
      load_link_at(A, g, d, nu, up ? c0 : c3, up);
      load_link(H, h, V, plane, c0.par, cb_of(c0, d));
      mat_mul(T, A, H);
      load_link(H, h, V, plane, c3.par, cb_of(c3, d));
      mat_mul_acc(T, H, A);
      // A2: c2 -> c3, U_mu(c3)^dag
      M3 B;
      load_link_at(B, g, d, mu, c3, true);
      mat_mul(S, B, A);
      mat_lmul(T, B);
      load_link(H, h, V, plane, c2.par, cb_of(c2, d));
      mat_mul_acc(T, H, S);
      // A1: c1 -> c2, U_nu(x + mu) (upper) or U_nu(c2)^dag (lower)
      load_link_at(A, g, d, nu, up ? c1 : c2, !up);
      mat_lmul(T, A);
      mat_lmul(S, A);
      load_link(H, h, V, plane, c1.par, cb_of(c1, d));
      mat_mul_acc(T, H, S);
      load_link(A, g, V, mu, parity, i);
      mat_mul(S, A, T);
      // W = i w U T
#pragma unroll
      for (int k = 0; k < 9; ++k)
        W[k / 3][k % 3] = {-w * S[k / 3][k % 3].im, w * S[k / 3][k % 3].re};
    }
  } else {
    // lane 6: G1_ca = sum_s [P(-mu) Y](x+mu)_sc conj(X(x))_sa
    // lane 7: G2_cb = sum_s [P(+mu) Y](x)_sc conj(X(x+mu))_sb
    const bool fw = lane == 6;
    const Site c1 = hop_sel(c0, mu, +1, d);
    const Site ys = fw ? c1 : c0, xs = fw ? c0 : c1;
    const long iy = cb_of(ys, d), ix = cb_of(xs, d);
    const double sg = fw ? -0.5 : 0.5;
    M3 G;
    mat_zero(G);
    for (int k = 0; k < n; ++k) {
      const double c = coef[k];
      cd X[4][3], Y[4][3], Z[4][3];
      load_spinor(Y, y, V, k, ys.par, iy);
      load_spinor(X, x, V, k, xs.par, ix);
      gamma_mul(Z, Y, mu);
#pragma unroll
      for (int s = 0; s < 4; ++s)
#pragma unroll
        for (int a = 0; a < 3; ++a) {
          // c P Y = c (Y +- gamma_mu Y) / 2
          const cd p = {c * (0.5 * Y[s][a].re + sg * Z[s][a].re),
                        c * (0.5 * Y[s][a].im + sg * Z[s][a].im)};
#pragma unroll
          for (int b = 0; b < 3; ++b)
            G[a][b] = cadd(G[a][b], cmulj(p, X[s][b]));
        }
    }
    // U G1, or -G2 U^dag = -(U G2^dag)^dag
    M3 U;
    load_link(U, g, V, mu, parity, i);
    mat_dagger_if(G, !fw);
    mat_mul(W, U, G);
    mat_dagger_if(W, !fw);
    const double sw = fw ? 1.0 : -1.0;
#pragma unroll
    for (int k = 0; k < 9; ++k)
      W[k / 3][k % 3] = {sw * W[k / 3][k % 3].re, sw * W[k / 3][k % 3].im};
  }

#pragma unroll
  for (int k = 0; k < 9; ++k) {
    W[k / 3][k % 3].re = item_sum(W[k / 3][k % 3].re);
    W[k / 3][k % 3].im = item_sum(W[k / 3][k % 3].im);
  }
  if (lane != 0) return;

  // F = kappa TA[W], TA[W] = (W - W^dag)/2 - tr/3
  M3 R;
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
#pragma unroll
  for (int k = 0; k < 9; ++k) {
    R[k / 3][k % 3].re *= kappa;
    R[k / 3][k % 3].im *= kappa;
  }
  if (fused) {
    M3 O;
    load_link(O, out, V, mu, parity, i);
#pragma unroll
    for (int k = 0; k < 9; ++k) {
      // one rounding per component
      R[k / 3][k % 3].re = fma(dt, R[k / 3][k % 3].re, O[k / 3][k % 3].re);
      R[k / 3][k % 3].im = fma(dt, R[k / 3][k % 3].im, O[k / 3][k % 3].im);
    }
  }
  store_link(out, V, mu, parity, i, R);
}

void launch_clover_sigma_oprod(const CloverForceCall &c, hipStream_t st) {
  int grid = (int)((2 * c.lat.Vcb + CF_BLOCK - 1) / CF_BLOCK);
  hipLaunchKernelGGL(k_clover_sigma_oprod, dim3(grid), dim3(CF_BLOCK), 0, st,
                     (cd *)c.h, (const cd *)c.x, (const cd *)c.y, c.coefs,
                     c.n, c.lat.Vcb);
}

void launch_clover_force(const CloverForceCall &c, hipStream_t st) {
  LatDims d = lat_dims(c.lat);
  int grid = (int)((64 * c.lat.Vcb + CF_BLOCK - 1) / CF_BLOCK);
  hipLaunchKernelGGL(k_clover_force, dim3(grid), dim3(CF_BLOCK), 0, st,
                     (cd *)c.out, (const cd *)c.u, (const cd *)c.h,
                     (const cd *)c.x, (const cd *)c.y, c.coefs, c.n, d,
                     c.kappa, c.csw, c.dt, c.accumulate ? 1 : 0);
}
