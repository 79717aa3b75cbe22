// Gauge-covariant hop sum on full-parity fields for MI355X (gfx950): the
// kernel under the Laplacian, the covariant displacement, Wuppertal and
// two-link smearing (role of the reference's kernels/laplace.cuh and
// covariant_derivative.cuh; the design is this project's own).
//
//   out(x) = a * sum_{h in hops} T_h in(x) + b * in(x)
//   T_{+mu} in(x) = U_mu(x)          in(x + H mu)
//   T_{-mu} in(x) = U_mu(x - H mu)^d in(x - H mu)
//
// hops is a runtime 8-bit mask, uniform over the grid (bit mu forward, bit
// 4+mu backward); H = 1 or 2 is the shift of the stencil gauge field. The
// -2*ndim diagonal of a Laplacian and smearing normalisations are folded
// into b by the caller: the kernel has no operator-specific branch.
//
// Work split. The unit is a column: the colour 3-vector of one (site, spin).
// A thread owns CPT columns of one site; the NS/CPT threads of a site are
// adjacent lanes and read the same link lines. A column range is a whole
// number of 16-byte chunks (double: any CPT; single: CPT even), so loads and
// stores stay vectorised and no two threads share a chunk. Half needs the
// site maximum for its block-float norm, so a thread owns the whole site.
//
// Links. Both links of a direction come from the site's own slots Q = mu and
// Q = 4+mu of the stencil layout: site-local, coalesced, valid for any H, no
// gauge neighbour index. NBR reads the backward link from the neighbour's
// forward slot instead, as the dslash kernels do (H = 1 only); it is kept as
// a measured variant (profiles/r11_laplace.md).
//
// Schedule. Stencils here are latency- and issue-bound: a round issues the
// raw chunk loads of its direction pairs (links and neighbour columns stay
// in storage format while in flight), then decodes and multiplies. The
// number of pairs per round follows from the registers a pair keeps in
// flight (lap_pairs_per_round); rounds are pinned by the data dependence on
// acc, as in dslash_wilson_body.inl.
#pragma once

#include "common.h"
#include "dslash_staggered.h"  // su3_mul_vec / su3_dagmul_vec

#define QA_LAP_BLOCK 256
// 32-bit registers of raw loads a round may keep in flight
#define QA_LAP_INFLIGHT 128

template <typename Prec, int RECON, int CPT>
constexpr int lap_pairs_per_round() {
  // one direction pair: two links and 2*CPT neighbour columns, counted at
  // working precision (the compiler hoists the half decode up under the
  // loads: counted as stored, half with 4 pairs in flight took 256 VGPRs
  // plus AGPR copies)
  constexpr int per =
      (2 * RECON + 2 * CPT * 6) * (int)sizeof(typename Prec::Real) / 4;
  return 4 * per <= QA_LAP_INFLIGHT ? 4 : 2 * per <= QA_LAP_INFLIGHT ? 2 : 1;
}

// cb index of x + disp*mu, |disp| <= 2 <= X[mu], local periodic wrap
__device__ __forceinline__ long lap_nbr(const int x[4], int mu, int disp,
                                        const LatDims &d) {
  int y[4] = {x[0], x[1], x[2], x[3]};
  int v = y[mu] + disp;
  if (v >= d.X[mu]) v -= d.X[mu];
  if (v < 0) v += d.X[mu];
  y[mu] = v;
  return cb_from_coords(y, d);
}

template <typename Prec, int RECON, int NS, int CPT, bool NBR>
__global__ __launch_bounds__(QA_LAP_BLOCK) void k_laplace(
    SpinorAcc<Prec, 6 * NS> out, SpinorAcc<Prec, 6 * NS> in,
    GaugeAcc<Prec, RECON> g, LatDims d, int hops, int H,
    typename Prec::Real a, typename Prec::Real b, long n_threads) {
  using Acc = SpinorAcc<Prec, 6 * NS>;
  using S = typename Prec::Store;
  using R = typename Prec::Real;
  static_assert(NS % CPT == 0 && (CPT * 6) % Acc::W == 0,
                "a thread's columns are whole chunks");
  constexpr int TPS = NS / CPT;            // threads per site
  constexpr int NCK = CPT * 6 / Acc::W;    // chunks per thread
  constexpr int NRAW = CPT * 6;            // stored reals per thread
  constexpr int LRAW = RECON + 2 * Prec::W;  // bound on a link's raw chunks
  constexpr int PPR = lap_pairs_per_round<Prec, RECON, CPT>();

  long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n_threads) return;
  long gs = t / TPS;  // global site in [0, 2*Vcb)
  int c0 = (int)(t - gs * TPS) * NCK;
  int p = gs >= d.Vcb ? 1 : 0;
  long i = gs - p * d.Vcb;
  int pn = p ^ (H & 1);  // parity of every neighbour
  long noff = pn * d.Vcb;
  // g.data = parity 0 block, g.other = parity 1 block
  const S *gown = p ? g.other : g.data;
  const S *gnbr = pn ? g.other : g.data;
  (void)gnbr;
  int xc[4];
  coords_from_cb(xc, i, d, p);

  S self[NRAW];
  R nself = (R)1;
  in.template load_chunks<NCK>(self, gs, c0);
  if constexpr (Prec::has_norm) nself = in.norm[gs];

  S sf[4][NRAW], sb[4][NRAW], lf[4][LRAW], lb[4][LRAW];
  R nf[4] = {(R)1, (R)1, (R)1, (R)1}, nb[4] = {(R)1, (R)1, (R)1, (R)1};
  cplx<R> acc[CPT][3];
#pragma unroll
  for (int k = 0; k < CPT; ++k)
#pragma unroll
    for (int c = 0; c < 3; ++c) acc[k][c] = {(R)0, (R)0};

#define QA_LGATHER(MU)                                                    \
  if (hops & (1 << MU)) {                                                 \
    long j = lap_nbr(xc, MU, H, d) + noff;                                \
    in.template load_chunks<NCK>(sf[MU], j, c0);                          \
    if constexpr (Prec::has_norm) nf[MU] = in.norm[j];                    \
    g.template load_raw<MU>(gown, lf[MU], i);                             \
  }                                                                       \
  if (hops & (16 << MU)) {                                                \
    long jc = lap_nbr(xc, MU, -H, d);                                     \
    in.template load_chunks<NCK>(sb[MU], jc + noff, c0);                  \
    if constexpr (Prec::has_norm) nb[MU] = in.norm[jc + noff];            \
    if constexpr (NBR)                                                    \
      g.template load_raw<MU>(gnbr, lb[MU], jc);                          \
    else                                                                  \
      g.template load_raw<4 + MU>(gown, lb[MU], i);                       \
  }

#define QA_LMUL(MU)                                                       \
  if (hops & (1 << MU)) {                                                 \
    cplx<R> U[3][3], v[3], w[3];                                          \
    g.template decode_raw<MU>(lf[MU], U);                                 \
    _Pragma("unroll")                                                     \
    for (int k = 0; k < CPT; ++k) {                                       \
      qa_dequantize<Prec, 3>(v, sf[MU] + 6 * k, nf[MU]);                  \
      su3_mul_vec(w, U, v);                                               \
      for (int c = 0; c < 3; ++c) acc[k][c] += w[c];                      \
    }                                                                     \
  }                                                                       \
  if (hops & (16 << MU)) {                                                \
    cplx<R> U[3][3], v[3], w[3];                                          \
    g.template decode_raw<(NBR ? MU : 4 + MU)>(lb[MU], U);                \
    _Pragma("unroll")                                                     \
    for (int k = 0; k < CPT; ++k) {                                       \
      qa_dequantize<Prec, 3>(v, sb[MU] + 6 * k, nb[MU]);                  \
      su3_dagmul_vec(w, U, v);                                            \
      for (int c = 0; c < 3; ++c) acc[k][c] += w[c];                      \
    }                                                                     \
  }

  // Round fence (see dslash_wilson_body.inl): acc is an in/out operand, so
  // the multiplies of a round finish above it, and the memory clobber keeps
  // the next round's loads below it. Emits no instruction.
#define QA_LFENCE()                                                       \
  _Pragma("unroll")                                                       \
  for (int k_ = 0; k_ < CPT; ++k_)                                        \
    asm volatile("" : "+v"(acc[k_][0].re), "+v"(acc[k_][0].im),           \
                      "+v"(acc[k_][1].re), "+v"(acc[k_][1].im),           \
                      "+v"(acc[k_][2].re), "+v"(acc[k_][2].im) :: "memory");

  if constexpr (PPR == 4) {
    QA_LGATHER(0)
    QA_LGATHER(1)
    QA_LGATHER(2)
    QA_LGATHER(3)
    QA_LMUL(0)
    QA_LMUL(1)
    QA_LMUL(2)
    QA_LMUL(3)
  } else if constexpr (PPR == 2) {
    QA_LGATHER(0)
    QA_LGATHER(1)
    QA_LMUL(0)
    QA_LMUL(1)
    QA_LFENCE()
    QA_LGATHER(2)
    QA_LGATHER(3)
    QA_LMUL(2)
    QA_LMUL(3)
  } else {
    QA_LGATHER(0)
    QA_LMUL(0)
    QA_LFENCE()
    QA_LGATHER(1)
    QA_LMUL(1)
    QA_LFENCE()
    QA_LGATHER(2)
    QA_LMUL(2)
    QA_LFENCE()
    QA_LGATHER(3)
    QA_LMUL(3)
  }
#undef QA_LFENCE
#undef QA_LMUL
#undef QA_LGATHER

  cplx<R> res[CPT * 3];
  qa_dequantize<Prec, CPT * 3>(res, self, nself);
#pragma unroll
  for (int k = 0; k < CPT; ++k)
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      cplx<R> &r = res[3 * k + c];
      r = {fma(a, acc[k][c].re, b * r.re), fma(a, acc[k][c].im, b * r.im)};
    }
  S tmp[NRAW];
  R m = qa_quantize<Prec, CPT * 3>(tmp, res);
  if constexpr (Prec::has_norm) {
    static_assert(!Prec::has_norm || NCK == Acc::NCH, "half owns the site");
    out.norm[gs] = m;
  }
  out.template store_chunks<NCK>(tmp, gs, c0);
}
