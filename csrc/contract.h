// Contraction family on full-parity 4-d fields for MI355X (gfx950): per-site
// open-spin / gamma-trace contraction, momentum-projected slice sums and the
// LapH eigenvector sink projection (roles of the reference's
// kernels/contraction.cuh and evec_project.cuh; the design is this project's
// own).
//
//   C[s,t](x)  = sum_c conj(x(s,c)) y(t,c)
//   D[g](x)    = sum_t i^k(g,t) C[col(g,t), t]        (16 monomial gammas)
//   out[p,r,g] = sum_{x : x[rd] = r} phase(p, x) D[g](x)
//   out[i,r,s] = sum_{x : x[rd] = r} sum_c conj(v_i(x,c)) psi(x,s,c)
//
// Fields are read raw through SpinorAcc::load_chunks and decoded straight to
// double (half: double(norm) * double(stored), exact, where load_v would
// round the product to float); every sum runs in double whatever the
// storage. No atomics: each output number has one fixed summation order.
//
// Gamma traces. The table (col, k) comes from Python (ops/contract.py derives
// it from fields/gamma.py); it is uniform, so each of the 64 (g, t) terms is
// a select among the four C[., t], a swap and two sign flips: no multiply.
//
// Slice kernels. A block owns tile k of slice r: NS consecutive sites of the
// slice's enumeration (parity, slice-local cb index). For rd = 3 a tile is a
// contiguous cb range and the loads coalesce; other rd only have to be right.
//
// k_contract_slices, stage 1: thread = site; the 16 traces go to the LDS
// tile, entry g of site s at slot (g + s) & 15 of row s. A row is 256 B, one
// pass over the 64 banks, so unrotated the lanes of a wave would all write
// the same four banks; rotated, 16 adjacent lanes fill 16 distinct 16-byte
// slots. Stage 2: thread = (group h = tid / 16, trace g = tid & 15), group =
// (momentum p0 + h % pcr, site segment h / pcr). The 16 lanes of a group read
// the 16 distinct slots of one row (all 64 banks once), groups on the same
// site share the addresses (broadcast), and the phase is one address per
// group. pcr = min(NS / 16, n_mom rounded up to a power of two) momenta run
// per pass; with few momenta the NS / 16 / pcr segments of a momentum walk
// interleaved sites and are added in segment order, so stage 2 keeps every
// lane busy at n_mom = 1 too. Phases: the separable factors f[p][d][x_d]
// come from the host table; stage 2 needs phase(p, site) for all 16 g, so a
// pass first stores the products of its pcr momenta in LDS [pcr][NS], one
// product per (site, p), rather than keeping the f rows in LDS and
// multiplying in the inner loop of every g. No sincos on the device.
// LDS: NS * (256 + NS + 16) bytes: 51 KB at NS = 128 (the default: two
// blocks per CU overlap stage 1 loads with stage 2), 135 KB at NS = 256
// (profiles/r12_contract.md).
#pragma once

#include "common.h"
#include "reduce.h"

#define QA_CT_BLOCK 256

// word g: nibble t = col | k << 2 of the non-zero entry i^k of row t of G_g
struct GammaTab {
  unsigned w[16];
};

// the slice x[rd] = r enumerated as (parity, slice-local cb index): the other
// dimensions a < b < c in lexicographic order, a halved by the checkerboard
struct SliceGeom {
  int rd, a, b, c;
  int Xah, Xb;   // X[a] / 2, X[b]
  int ob, oc;    // offsets of the b and c factors in a phase row
  int ltot;      // X[a] + X[b] + X[c]: entries per momentum
  int L;         // X[rd]: slices
  long Vs;       // sites per slice
};

__device__ __forceinline__ void ct_set(int x[4], int idx, int v) {
#pragma unroll
  for (int k = 0; k < 4; ++k) x[k] = (k == idx) ? v : x[k];
}

// slice site q in [0, Vs) of slice r -> coordinates and global site index
__device__ __forceinline__ long ct_slice_site(int x[4], int &xa, int &xb,
                                              int &xc, long q, int r,
                                              const LatDims &d,
                                              const SliceGeom &sg) {
  long half = sg.Vs >> 1;
  int p = q >= half ? 1 : 0;
  long j = q - p * half;
  int ha = (int)(j % sg.Xah);
  long t = j / sg.Xah;
  xb = (int)(t % sg.Xb);
  xc = (int)(t / sg.Xb);
  xa = 2 * ha + ((p + d.parity_offset + r + xb + xc) & 1);
  ct_set(x, sg.rd, r);
  ct_set(x, sg.a, xa);
  ct_set(x, sg.b, xb);
  ct_set(x, sg.c, xc);
  return p * d.Vcb + cb_from_coords(x, d);
}

template <typename Prec, int NCOMP>
__device__ __forceinline__ void ct_load(cplx<double> *out,
                                        const SpinorAcc<Prec, NCOMP> &f,
                                        long g) {
  using A = SpinorAcc<Prec, NCOMP>;
  typename Prec::Store tmp[NCOMP];
  f.template load_chunks<A::NCH>(tmp, g, 0);
  double scale = 1.0;
  if constexpr (Prec::has_norm) scale = (double)f.norm[g];
#pragma unroll
  for (int k = 0; k < NCOMP / 2; ++k)
    out[k] = {scale * (double)qa_tor<typename Prec::Real>(tmp[2 * k]),
              scale * (double)qa_tor<typename Prec::Real>(tmp[2 * k + 1])};
}

// C[s][t] = sum_c conj(x(s,c)) y(t,c) of global site gs
template <typename Prec>
__device__ __forceinline__ void ct_open(cplx<double> C[4][4],
                                        const SpinorAcc<Prec, 24> &x,
                                        const SpinorAcc<Prec, 24> &y,
                                        long gs) {
  cplx<double> xv[12], yv[12];
  ct_load(xv, x, gs);
  ct_load(yv, y, gs);
#pragma unroll
  for (int s = 0; s < 4; ++s)
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      cplx<double> acc(0.0, 0.0);
#pragma unroll
      for (int c = 0; c < 3; ++c)
        acc = cfma_conj(xv[3 * s + c], yv[3 * t + c], acc);
      C[s][t] = acc;
    }
}

// by value: a conditional over the array elements themselves is an lvalue,
// i.e. a dynamic address into C, and pushes C to scratch
__device__ __forceinline__ double ct_sel4(unsigned s, double a0, double a1,
                                          double a2, double a3) {
  double lo = (s & 1u) ? a1 : a0, hi = (s & 1u) ? a3 : a2;
  return (s & 2u) ? hi : lo;
}

__device__ __forceinline__ void ct_traces(cplx<double> D[16],
                                          const cplx<double> C[4][4],
                                          const GammaTab &gt) {
#pragma unroll
  for (int g = 0; g < 16; ++g) {
    cplx<double> acc(0.0, 0.0);
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      unsigned e = (gt.w[g] >> (4 * t)) & 15u;
      unsigned s = e & 3u, k = e >> 2;
      double ar = ct_sel4(s, C[0][t].re, C[1][t].re, C[2][t].re, C[3][t].re);
      double ai = ct_sel4(s, C[0][t].im, C[1][t].im, C[2][t].im, C[3][t].im);
      // i^k a: k = 1 (-im, re), k = 2 (-re, -im), k = 3 (im, -re)
      double re = (k & 1u) ? ai : ar, im = (k & 1u) ? ar : ai;
      acc.re += (k == 1u || k == 2u) ? -re : re;
      acc.im += (k >= 2u) ? -im : im;
    }
    D[g] = acc;
  }
}

// ---------------------------------------------------------------------------
// site kernel: 16 numbers per site at the lexicographic index
// ---------------------------------------------------------------------------
template <typename Prec>
__global__ __launch_bounds__(QA_CT_BLOCK) void k_contract_site(
    double2 *out, SpinorAcc<Prec, 24> x, SpinorAcc<Prec, 24> y, LatDims d,
    GammaTab gt, int dr) {
  long gs = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (gs >= 2 * d.Vcb) return;
  int p = gs >= d.Vcb ? 1 : 0;
  int xc[4];
  coords_from_cb(xc, gs - p * d.Vcb, d, p);
  long lex = (((long)xc[3] * d.X[2] + xc[2]) * d.X[1] + xc[1]) * d.X[0] + xc[0];
  cplx<double> C[4][4], D[16];
  ct_open(C, x, y, gs);
  if (dr) {
    ct_traces(D, C, gt);
  } else {
#pragma unroll
    for (int e = 0; e < 16; ++e) D[e] = C[e >> 2][e & 3];
  }
#pragma unroll
  for (int e = 0; e < 16; ++e) out[lex * 16 + e] = make_double2(D[e].re, D[e].im);
}

// ---------------------------------------------------------------------------
// slice-sum kernel: partial[k][p][r][g], grid (tiles, slices), NS threads
// ---------------------------------------------------------------------------
template <typename Prec, int NS>
__global__ __launch_bounds__(NS) void k_contract_slices(
    double2 *partial, SpinorAcc<Prec, 24> x, SpinorAcc<Prec, 24> y, LatDims d,
    SliceGeom sg, GammaTab gt, const double2 *f, int n_mom, int pcr) {
  constexpr int PC = NS / 16;  // groups of 16 lanes
  static_assert(NS % 64 == 0 && (PC & (PC - 1)) == 0, "whole waves");
  __shared__ double2 tile[NS][16];
  __shared__ double2 phs[PC][NS];
  __shared__ double2 red[PC][16];

  const int tid = threadIdx.x, k = blockIdx.x, r = blockIdx.y;
  const long q = (long)k * NS + tid;
  const bool live = q < sg.Vs;
  int xa = 0, xb = 0, xc = 0;
  {
    cplx<double> D[16];
    if (live) {
      int xs[4] = {0, 0, 0, 0};
      long gs = ct_slice_site(xs, xa, xb, xc, q, r, d, sg);
      cplx<double> C[4][4];
      ct_open(C, x, y, gs);
      ct_traces(D, C, gt);
    } else {
#pragma unroll
      for (int g = 0; g < 16; ++g) D[g] = {0.0, 0.0};
    }
#pragma unroll
    for (int g = 0; g < 16; ++g)
      tile[tid][(g + tid) & 15] = make_double2(D[g].re, D[g].im);
  }

  const int h = tid >> 4, g = tid & 15;
  const int segs = PC / pcr;  // pcr is a power of two <= PC
  const int pl = h & (pcr - 1), seg = h / pcr;
  for (int p0 = 0; p0 < n_mom; p0 += pcr) {
    __syncthreads();  // tile complete; the previous pass is done with phs, red
    for (int j = 0; j < pcr; ++j) {
      double2 ph = make_double2(0.0, 0.0);
      if (live && p0 + j < n_mom) {
        const double2 *fp = f + (long)(p0 + j) * sg.ltot;
        double2 fa = fp[xa], fb = fp[sg.ob + xb], fc = fp[sg.oc + xc];
        cplx<double> w = cplx<double>(fa.x, fa.y) * cplx<double>(fb.x, fb.y);
        w = w * cplx<double>(fc.x, fc.y);
        ph = make_double2(w.re, w.im);
      }
      phs[j][tid] = ph;
    }
    __syncthreads();
    cplx<double> acc(0.0, 0.0);
    for (int s = seg; s < NS; s += segs) {
      double2 ph = phs[pl][s], v = tile[s][(g + s) & 15];
      acc = cfma(cplx<double>(ph.x, ph.y), cplx<double>(v.x, v.y), acc);
    }
    red[h][g] = make_double2(acc.re, acc.im);
    __syncthreads();
    if (seg == 0 && p0 + pl < n_mom) {
      double re = 0.0, im = 0.0;
      for (int s = 0; s < segs; ++s) {
        double2 v = red[s * pcr + pl][g];
        re += v.x;
        im += v.y;
      }
      partial[(((long)k * n_mom + p0 + pl) * sg.L + r) * 16 + g] =
          make_double2(re, im);
    }
  }
}

// ---------------------------------------------------------------------------
// eigenvector sink projection: partial[k][i0 + i][r][s], grid (tiles, slices).
// A tile is spt * 256 sites; a thread walks its spt sites with psi of the
// current site in registers (read once per batch of NE eigenvectors) and
// 4 complex accumulators per eigenvector, then the block reduces them: wave
// shuffles, then the waves in order through LDS. The batch's base pointers
// travel as kernel arguments; ne <= NE of them are valid.
// ---------------------------------------------------------------------------
template <int NE>
struct EvecTab {
  const void *data[NE];
  const float *norm[NE];
};

template <typename Prec, int NE>
__global__ __launch_bounds__(QA_CT_BLOCK) void k_evec_project(
    double2 *partial, SpinorAcc<Prec, 24> psi, EvecTab<NE> ev, int ne, int i0,
    int n_ev, LatDims d, SliceGeom sg, int spt) {
  using S = typename Prec::Store;
  __shared__ double wsum[QA_CT_BLOCK / 64][NE * 8];
  const int tid = threadIdx.x, k = blockIdx.x, r = blockIdx.y;
  double acc[NE][8];
#pragma unroll
  for (int i = 0; i < NE; ++i)
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[i][j] = 0.0;

  for (int u = 0; u < spt; ++u) {
    long q = ((long)k * spt + u) * QA_CT_BLOCK + tid;
    if (q >= sg.Vs) break;
    int xs[4] = {0, 0, 0, 0}, xa, xb, xc;
    long gs = ct_slice_site(xs, xa, xb, xc, q, r, d, sg);
    cplx<double> ps[12];
    ct_load(ps, psi, gs);
#pragma unroll
    for (int i = 0; i < NE; ++i) {
      if (i < ne) {
        SpinorAcc<Prec, 6> v{(S *)ev.data[i], (float *)ev.norm[i], d.Vcb};
        cplx<double> vc[3];
        ct_load(vc, v, gs);
#pragma unroll
        for (int s = 0; s < 4; ++s) {
          cplx<double> a(acc[i][2 * s], acc[i][2 * s + 1]);
#pragma unroll
          for (int c = 0; c < 3; ++c) a = cfma_conj(vc[c], ps[3 * s + c], a);
          acc[i][2 * s] = a.re;
          acc[i][2 * s + 1] = a.im;
        }
      }
    }
  }

  const int lane = tid & 63, wave = tid >> 6;
#pragma unroll
  for (int i = 0; i < NE; ++i) {
    if (i < ne) {
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        double w = wave_reduce(acc[i][j]);
        if (lane == 0) wsum[wave][i * 8 + j] = w;
      }
    }
  }
  __syncthreads();
  if (tid < ne * 4) {
    int i = tid >> 2, s = tid & 3;
    double re = 0.0, im = 0.0;
    for (int w = 0; w < QA_CT_BLOCK / 64; ++w) {
      re += wsum[w][i * 8 + 2 * s];
      im += wsum[w][i * 8 + 2 * s + 1];
    }
    partial[(((long)k * n_ev + i0 + i) * sg.L + r) * 4 + s] =
        make_double2(re, im);
  }
}
