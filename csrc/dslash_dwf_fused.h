// Fused domain-wall kernel for MI355X (gfx950): the 4-d hop of ALL Ls
// slices plus a per-site dense s-space stage in one launch
// (role of reference include/kernels/dslash_domain_wall_4d_fused_m5.cuh —
//  redesigned: everything between a Dhat and the next B in the Moebius
//  operators is a per-4-d-site linear map in s that never mixes the two
//  chiralities (P± are spin-diagonal in DeGrand-Rossi, see dslash_dwf.h),
//  so the host folds the whole stage into two real Ls x Ls matrices and the
//  kernel applies them from LDS — no in-kernel recursion, no extra HBM
//  round-trip, and in half precision a single block-float rounding).
//
//   out(s,x) = [x(s,x) +] a * sum_s' W_chi[s,s'] (Dhat in)(s',x)
//
// chi = upper block (spins 0,1) / lower block (spins 2,3). Dhat is exactly
// the KT_LOCAL PLAIN stencil of k_dslash_wilson (same projector
// normalisation, dagger convention and fwd-slot backward-link reads).
//
// Thread map: one thread per (x, s). A workgroup owns NS consecutive
// checkerboard sites (16 or 32) times all Ls slices (blockDim = NS*Ls, thread
// t -> site t % NS, slice t / NS), so lanes run over consecutive x at fixed
// s (5-d index i5 = s*Vcb + x: coalesced 16-byte chunk loads) and the Ls
// threads of a 4-d site share their gauge loads through L1.
// LDS: the 24 reals of (Dhat in) as [component][s][site] — consecutive
// sites hit consecutive banks, equal sites at different s broadcast.
// HASW = false (W = identity) skips the LDS stage: a single-launch 5-d hop.
#pragma once

#include "common.h"
#include "generated/proj.h"

template <typename Prec>
struct DwfFusedTile {
  static constexpr int LS_MAX = 16;
  // largest tile: blockDim = NS*Ls <= 512 (single/half) or 256 (double)
  // threads and 24*Ls*NS*sizeof(Real) <= 48 KB of LDS at Ls = 16
  static constexpr int NS_MAX = sizeof(typename Prec::Real) == 8 ? 16 : 32;
  // the launch bound is the largest workgroup of ANY tile: it caps the
  // allocation at 256 VGPRs (2 waves/SIMD) for the smaller tiles too
  static constexpr int MAX_THREADS = NS_MAX * LS_MAX;
};

// NS = sites per workgroup (a tile of NS consecutive cb sites x Ls slices)
template <typename Prec, int RECON, bool DAG, bool XPAY, bool HASW, int NS>
__global__ __launch_bounds__(DwfFusedTile<Prec>::MAX_THREADS) void k_dwf_fused(
    SpinorAcc<Prec> out, SpinorAcc<Prec> in, GaugeAcc<Prec, RECON> g,
    LatDims d, int parity, typename Prec::Real a, SpinorAcc<Prec> x, int Ls,
    const typename Prec::Real *__restrict__ W) {
  using R = typename Prec::Real;
  static_assert(NS <= DwfFusedTile<Prec>::NS_MAX);
  extern __shared__ __attribute__((aligned(16))) char qa_dwf_smem[];
  R *lds = reinterpret_cast<R *>(qa_dwf_smem);  // [24][Ls][NS]

  const int ls = threadIdx.x % NS;
  const int s = threadIdx.x / NS;  // < Ls: blockDim.x == NS * Ls
  const long i = (long)blockIdx.x * NS + ls;
  // tail threads of the last tile skip every load and the store but still
  // reach the barrier below (no early return)
  const bool active = i < d.Vcb;
  // slice s as a pointer offset (a 4-d slice of the 5-d field, exactly the
  // view k_dslash_wilson gets per launch): site indices stay 4-d
  const long soff = (long)s * d.Vcb;
  in.data += soff * SpinorAcc<Prec>::W;
  out.data += soff * SpinorAcc<Prec>::W;
  x.data += soff * SpinorAcc<Prec>::W;
  if constexpr (Prec::has_norm) {
    in.norm += soff;
    out.norm += soff;
    x.norm += soff;
  }

  cplx<R> acc[4][3];
#pragma unroll
  for (int sp = 0; sp < 4; ++sp)
#pragma unroll
    for (int c = 0; c < 3; ++c) acc[sp][c] = {(R)0, (R)0};

  if (active) {
    int xc[4];
    coords_from_cb(xc, i, d, parity);
    cplx<R> p[4][3], h[8][2][3], uh[2][3], U[3][3];
    // proj/recon tables encode 2P (generate_proj.py); the stencil needs P
    const R one = (R)0.5;
    long jm[4];

    // gather + project all 8 neighbors first, then the gauge multiplies
    // (the load-ILP shape of k_dslash_wilson, ROUNDS == 1)
#define QA_GATHER(MU)                                                     \
  {                                                                       \
    long j = neighbor_cb(xc, MU, +1, d);                                  \
    in.load(p, j);                                                        \
    if constexpr (!DAG) proj_##MU##_0(h[2 * MU], p);                      \
    else proj_##MU##_1(h[2 * MU], p);                                     \
    j = neighbor_cb(xc, MU, -1, d);                                       \
    jm[MU] = j;                                                           \
    in.load(p, j);                                                        \
    if constexpr (!DAG) proj_##MU##_1(h[2 * MU + 1], p);                  \
    else proj_##MU##_0(h[2 * MU + 1], p);                                 \
  }
    // fwd link at own site; bwd link from the -mu neighbor's fwd slot
#define QA_MUL(MU)                                                        \
  {                                                                       \
    g.template load<MU>(U, i);                                            \
    su3_mul_half(uh, U, h[2 * MU]);                                       \
    if constexpr (!DAG) recon_##MU##_0(acc, uh, one);                     \
    else recon_##MU##_1(acc, uh, one);                                    \
    g.template load_o<MU>(U, jm[MU]);                                     \
    su3_dagmul_half(uh, U, h[2 * MU + 1]);                                \
    if constexpr (!DAG) recon_##MU##_1(acc, uh, one);                     \
    else recon_##MU##_0(acc, uh, one);                                    \
  }
    QA_GATHER(0)
    QA_GATHER(1)
    QA_GATHER(2)
    QA_GATHER(3)
    QA_MUL(0)
    QA_MUL(1)
    QA_MUL(2)
    QA_MUL(3)
#undef QA_GATHER
#undef QA_MUL
  }

  if constexpr (HASW) {
    const int cstride = Ls * NS;  // one component plane
    R *mine = lds + s * NS + ls;
#pragma unroll
    for (int k = 0; k < 12; ++k) {
      mine[(2 * k) * cstride] = acc[k / 3][k % 3].re;
      mine[(2 * k + 1) * cstride] = acc[k / 3][k % 3].im;
    }
    __syncthreads();
    if (active) {
      R res[24];
#pragma unroll
      for (int k = 0; k < 24; ++k) res[k] = (R)0;
      const R *wu = W + s * Ls;             // row s of the upper block
      const R *wl = W + (Ls + s) * Ls;      // row s of the lower block
      const R *col = lds + ls;
      for (int sp = 0; sp < Ls; ++sp) {
        const R u = wu[sp], l = wl[sp];
        const R *src = col + sp * NS;
#pragma unroll
        for (int k = 0; k < 12; ++k) res[k] = fma(u, src[k * cstride], res[k]);
#pragma unroll
        for (int k = 12; k < 24; ++k) res[k] = fma(l, src[k * cstride], res[k]);
      }
#pragma unroll
      for (int k = 0; k < 12; ++k)
        acc[k / 3][k % 3] = {res[2 * k], res[2 * k + 1]};
    }
  }

  if (active) {
    if constexpr (XPAY) {
      cplx<R> xv[4][3];
      x.load(xv, i);
#pragma unroll
      for (int sp = 0; sp < 4; ++sp)
#pragma unroll
        for (int c = 0; c < 3; ++c) acc[sp][c] = xv[sp][c] + a * acc[sp][c];
    } else {
      if (a != (R)1) {
#pragma unroll
        for (int sp = 0; sp < 4; ++sp)
#pragma unroll
          for (int c = 0; c < 3; ++c) acc[sp][c] = a * acc[sp][c];
      }
    }
    out.store(acc, i);
  }
}
