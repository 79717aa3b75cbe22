// Multigrid transfer kernels (fine Wilson level <-> first coarse level):
// prolong, restrict and block-orthonormalize, reading and writing the
// chunked-SoA spinor storage directly (ref: kernels/prolongator.cuh,
// restrictor.cuh, block_orthogonalize.cuh — re-derived for wave64).
//
// Conventions (quda_amd/mg/transfer.py builds the tables):
//   fine site   g = parity*Vcb + x   in [0, G), G = 2*Vcb
//   chirality   chi 0 = spins 0,1; chi 1 = spins 2,3; k12 = s*3 + c
//   Vn          [12][Nv][G] complex, site-fastest (k12 = chi*6 + k6): prolong
//   V           [Na][B][12][Nv] complex, aggregate order: restrict, ortho
//   coarse      [Na][2][Nv] complex of the field's real type
//   agg_of_site [G] int32, site_tab [Na][B] int32 (fine site of (a, b))
#include "launch_setup.h"

namespace {

constexpr int QA_TR_MAXT = 256;  // largest workgroup of the reductions

// one complex through a single 8/16-byte load
template <typename R>
__device__ __forceinline__ cplx<R> ld_cplx(const cplx<R> *p) {
  R t[2];
  load_chunk<R, 2>(reinterpret_cast<const R *>(p), t);
  return {t[0], t[1]};
}

template <typename R>
__device__ __forceinline__ R wave_sum(R v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  return v;  // lane 0 holds the sum; fixed pairing order
}

// ---------------------------------------------------------------------------
// prolong: out(g, s, c) = sum_v V(g, s, c, v) * coarse[agg(g), chi(s), v]
// one thread per fine site, both parities
// ---------------------------------------------------------------------------
template <typename Prec>
__global__ void k_transfer_prolong(
    SpinorAcc<Prec> out, const cplx<typename Prec::Real> *__restrict__ coarse,
    const cplx<typename Prec::Real> *__restrict__ Vn,
    const int *__restrict__ agg_of_site, long G, long Na, int Nv) {
  using R = typename Prec::Real;
  long g = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= G) return;
  cplx<R> acc[12];
#pragma unroll
  for (int k = 0; k < 12; ++k) acc[k] = {(R)0, (R)0};
  long a = agg_of_site[g];
  if (a >= 0 && a < Na) {
    const cplx<R> *c0 = coarse + a * 2 * Nv;
    const long rs = (long)Nv * G;  // stride between (chi, k) rows of Vn
    for (int v = 0; v < Nv; ++v) {
      cplx<R> cc[2] = {ld_cplx(c0 + v), ld_cplx(c0 + Nv + v)};
      const cplx<R> *vp = Vn + (long)v * G + g;
#pragma unroll
      for (int k = 0; k < 12; ++k)
        acc[k] = cfma(ld_cplx(vp + (long)k * rs), cc[k / 6], acc[k]);
    }
  }
  out.store_v(acc, g);
}

// ---------------------------------------------------------------------------
// restrict: c[a, chi, v] = sum_{b < B} sum_{k < 6} conj(V) * psi
// reads the aggregate-ordered V[Na][B][4][3][Nv]: for one (a, b, chi) the
// 6*Nv entries are contiguous, so a workgroup per (aggregate, chirality)
// streams its panel with consecutive lanes on consecutive addresses. Thread
// t owns color v = t % Wt and sums the rows r = (b, k) = r0, r0 + q,
// r0 + 2q, ... (r0 = t / Wt) in that order; the q partial sums of each color
// then meet in LDS and are added in the order r0 = 0 .. q-1. The order is
// fixed (it is not the plain row order) and there are no atomics, so the
// result does not depend on scheduling. Colors beyond QA_TR_MAXT are tiled
// over the grid.
// ---------------------------------------------------------------------------
template <typename Prec>
__device__ __forceinline__ cplx<typename Prec::Real> load_comp(
    const SpinorAcc<Prec> &in, long g, int kc) {  // kc = s*3 + c
  using S = typename Prec::Store;
  using R = typename Prec::Real;
  constexpr int W = SpinorAcc<Prec>::W;
  constexpr int CPC = W / 2;  // complexes per chunk
  const int ch = kc / CPC, off = (kc - ch * CPC) * 2;
  S t[2];
  load_chunk<S, 2>(in.data + in.chunk_base(g) + (long)ch * in.V * W + off, t);
  return {(R)t[0], (R)t[1]};
}

template <typename Prec>
__global__ void __launch_bounds__(QA_TR_MAXT) k_transfer_restrict(
    cplx<typename Prec::Real> *__restrict__ coarse, SpinorAcc<Prec> in,
    const cplx<typename Prec::Real> *__restrict__ V,
    const int *__restrict__ site_tab, long G, long Na, int B, int Nv) {
  using R = typename Prec::Real;
  __shared__ R red[QA_TR_MAXT][2];

  const int ntile = (Nv + QA_TR_MAXT - 1) / QA_TR_MAXT;
  const long bid = blockIdx.x;
  const int tile = (int)(bid % ntile);
  const long ac = bid / ntile;
  const int chi = (int)(ac & 1);
  const long a = ac >> 1;
  if (a >= Na) return;  // uniform over the workgroup
  const int v0 = tile * QA_TR_MAXT;
  const int Wt = min(QA_TR_MAXT, Nv - v0);  // colors of this tile
  const int q = (int)blockDim.x / Wt;       // rows in flight
  const int tid = threadIdx.x;
  const int vt = tid % Wt, r0 = tid / Wt;

  cplx<R> acc((R)0, (R)0);
  if (r0 < q) {
    const cplx<R> *panel = V + (a * B * 12 + chi * 6) * (long)Nv + v0 + vt;
    // U rows per trip so the table -> field load chains overlap; the
    // thread's sum keeps its order (an out-of-range row adds an exact zero)
    constexpr int U = 4;
    const int n = 6 * B;
    for (int r = r0; r < n; r += U * q) {
      long g[U];
      int bb[U], kk[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int rr = r + u * q;
        bb[u] = rr / 6;
        kk[u] = rr - 6 * bb[u];
        g[u] = rr < n ? (long)site_tab[a * B + bb[u]] : -1L;
      }
      cplx<R> vv[U], pp[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const bool ok = g[u] >= 0 && g[u] < G;
        vv[u] = ok ? ld_cplx(panel + ((long)bb[u] * 12 + kk[u]) * Nv)
                   : cplx<R>((R)0, (R)0);
        pp[u] = ok ? load_comp(in, g[u], chi * 6 + kk[u])
                   : cplx<R>((R)0, (R)0);
      }
#pragma unroll
      for (int u = 0; u < U; ++u) acc = cfma_conj(vv[u], pp[u], acc);
    }
  }
  red[tid][0] = acc.re;
  red[tid][1] = acc.im;
  __syncthreads();
  if (tid < Wt) {
    R re = (R)0, im = (R)0;
    for (int m = 0; m < q; ++m) {
      re += red[tid + m * Wt][0];
      im += red[tid + m * Wt][1];
    }
    coarse[ac * Nv + v0 + tid] = {re, im};
  }
}

// ---------------------------------------------------------------------------
// block-orthonormalize: per (aggregate, chirality) modified Gram-Schmidt of
// the Nv columns of the [6B x Nv] panel, in place in V[Na][B][4][3][Nv]
// (complex double). Each thread owns the rows r = tid, tid + T, ... for every
// column, so only the reduced scalars cross threads; the panel stays in
// global memory (L2). The update of column j by column i is fused with the
// next dot product (or the norm) so each projection sweeps the column once.
// ---------------------------------------------------------------------------
__device__ __forceinline__ cplx<double> block_sum(cplx<double> v,
                                                  double (*red)[2], int nw) {
  double re = wave_sum(v.re), im = wave_sum(v.im);
  if ((threadIdx.x & 63) == 0) {
    red[threadIdx.x >> 6][0] = re;
    red[threadIdx.x >> 6][1] = im;
  }
  __syncthreads();
  cplx<double> s(0.0, 0.0);
  for (int w = 0; w < nw; ++w) {  // every thread: the same order
    s.re += red[w][0];
    s.im += red[w][1];
  }
  return s;
}

__global__ void __launch_bounds__(QA_TR_MAXT) k_transfer_block_ortho(
    cplx<double> *V, long Na, int B, int Nv, int passes) {
  // two buffers: reduction m+1 writes the buffer last read in reduction
  // m-1, whose readers have all passed the barrier of reduction m
  __shared__ double red[2][QA_TR_MAXT / 64][2];
  const long ac = blockIdx.x;
  const int chi = (int)(ac & 1);
  const long a = ac >> 1;
  if (a >= Na) return;  // uniform over the workgroup
  const int n = 6 * B;
  const int T = blockDim.x;
  const int nw = (T + 63) >> 6;
  cplx<double> *panel = V + (a * B * 12 + chi * 6) * (long)Nv;
  // row r = (b, k): b*12*Nv + k*Nv past the panel base
  auto row = [&](int r) -> cplx<double> * {
    int b = r / 6, k = r - 6 * b;
    return panel + ((long)b * 12 + k) * Nv;
  };
  int m = 0;  // reduction counter (selects the LDS buffer)
  for (int p = 0; p < passes; ++p) {
    for (int j = 0; j < Nv; ++j) {
      cplx<double> acc(0.0, 0.0);
      for (int r = threadIdx.x; r < n; r += T) {
        cplx<double> *w = row(r);
        cplx<double> wj = ld_cplx(w + j);
        if (j == 0)
          acc.re = fma(wj.re, wj.re, fma(wj.im, wj.im, acc.re));
        else
          acc = cfma_conj(ld_cplx(w), wj, acc);
      }
      for (int i = 0; i < j; ++i) {
        cplx<double> c = block_sum(acc, red[m & 1], nw);
        ++m;
        acc = {0.0, 0.0};
        for (int r = threadIdx.x; r < n; r += T) {
          cplx<double> *w = row(r);
          cplx<double> wj = ld_cplx(w + j) - c * ld_cplx(w + i);
          w[j] = wj;
          if (i + 1 < j)
            acc = cfma_conj(ld_cplx(w + i + 1), wj, acc);
          else
            acc.re = fma(wj.re, wj.re, fma(wj.im, wj.im, acc.re));
        }
      }
      double nrm = fmax(sqrt(block_sum(acc, red[m & 1], nw).re), 1e-30);
      ++m;
      for (int r = threadIdx.x; r < n; r += T) {
        cplx<double> *w = row(r);
        cplx<double> wj = ld_cplx(w + j);
        w[j] = {wj.re / nrm, wj.im / nrm};
      }
    }
  }
}

int reduce_block(long n) { return n <= 64 ? 64 : n <= 128 ? 128 : QA_TR_MAXT; }

template <typename Prec>
void prolong_t(const TransferCall &c, hipStream_t st) {
  using R = typename Prec::Real;
  const long G = 2 * c.field.Vcb;
  auto out = spinor_acc<Prec>(c.field);  // double/single: no norm
  const int T = 64;  // one wave per workgroup spreads small lattices widest
  hipLaunchKernelGGL(k_transfer_prolong<Prec>, dim3((unsigned)((G + T - 1) / T)),
                     dim3(T), 0, st, out, (const cplx<R> *)c.coarse,
                     (const cplx<R> *)c.Vn, c.agg_of_site, G, c.Na, c.Nv);
}

template <typename Prec>
void restrict_t(const TransferCall &c, hipStream_t st) {
  using R = typename Prec::Real;
  const long G = 2 * c.field.Vcb;
  auto in = spinor_acc<Prec>(c.field);
  const long ntile = (c.Nv + QA_TR_MAXT - 1) / QA_TR_MAXT;
  hipLaunchKernelGGL(k_transfer_restrict<Prec>,
                     dim3((unsigned)(c.Na * 2 * ntile)), dim3(QA_TR_MAXT), 0,
                     st, (cplx<R> *)c.coarse, in, (const cplx<R> *)c.V,
                     c.site_tab, G, c.Na, c.B, c.Nv);
}

}  // namespace

bool qa_transfer_grid_ok(const TransferCall &c) {
  const long G = 2 * c.field.Vcb;
  const long ntile = (c.Nv + QA_TR_MAXT - 1) / QA_TR_MAXT;
  return c.Na > 0 && c.B > 0 && c.Nv > 0 && G > 0 && G / 64 < (1L << 31) - 1 &&
         c.Na * 2 * ntile < (1L << 31) - 1;
}

void launch_transfer_prolong(const TransferCall &c, hipStream_t st) {
  if (c.prec == 0) prolong_t<PrecDouble>(c, st);
  else prolong_t<PrecSingle>(c, st);
}

void launch_transfer_restrict(const TransferCall &c, hipStream_t st) {
  if (c.prec == 0) restrict_t<PrecDouble>(c, st);
  else restrict_t<PrecSingle>(c, st);
}

void launch_transfer_block_ortho(const BlockOrthoCall &c, hipStream_t st) {
  hipLaunchKernelGGL(k_transfer_block_ortho, dim3((unsigned)(c.Na * 2)),
                     dim3(reduce_block(6L * c.B)), 0, st, (cplx<double> *)c.V,
                     c.Na, c.B, c.Nv, c.passes);
}
