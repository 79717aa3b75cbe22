// Kahler-Dirac block inverse for MI355X (gfx950): the 2^4-hypercube block X of
// the staggered operator, its structured inverse, and the fused apply on
// native staggered storage (role of the reference's staggered_kd_build_xinv
// and staggered_kd_apply_xinv kernels; the design is this project's own).
//
// Structure. Order the 16 corners of a block by corner parity, popcount & 1:
// 8 even corners, then 8 odd ones, 3 colours each. In-block hops connect the
// two classes only, and eta_mu(x + mu) = eta_mu(x), so
//
//   X = [[ 2m,   B ],      B: 24 x 24, tiles +eta_mu(x) U_mu(x) (x even) or
//        [ -B^d, 2m ]]                       -eta_mu(x) U_mu(x)^d (x odd)
//
// X is normal. With E = (4m^2 + B B^d)^-1, O = (4m^2 + B^d B)^-1 (Hermitian
// positive definite for m > 0: Cholesky, no pivoting)
//
//   X^-1 = [[ P,   -G ],   P = 2m E, Q = 2m O, G = E B
//           [ G^d,  Q ]]
//
// and the daggers of X and X^-1 flip the sign of the off-diagonal blocks.
//
// Row order: row = class * 24 + cic * 3 + colour, cic = corner & 7 (the t bit
// of the corner follows from cic and the class), so the three colours of a
// site are adjacent lanes.
//
// Table, per block, in the table type T (double for double fields, float for
// single and half); all build arithmetic is double:
//   PQ  [blk][24/KV][48][KV]  PQ[k][row] = P[row][k] (row < 24) or
//                             Q[row - 24][k]; KV = 16 / sizeof(cplx<T>)
//                             consecutive k share a 16-byte word, and the 48
//                             rows of one k-group are contiguous: a wave's
//                             load is one 768-byte run
//   G   [blk][24][24]         row-major
//   B   [blk][24][24]         row-major, so that apply_X needs no gauge access
// Sections follow each other: PQ at 0, G at 1152 nblk, B at 1728 nblk.
//
// k_kd_build: one wave per block; B, the normal matrix and the inverse of its
// Cholesky factor live in LDS (27 KB).
//
// k_kd_apply: one wave per block, 4 blocks (consecutive in x) per workgroup.
// Lanes 0..47 own one output row each; lanes 48..63 only help staging G: 576
// entries are 9 per lane of 64. A wave per block keeps the colour lanes of a
// site inside one wave (192 threads for 4 blocks would split a site over the
// boundary between waves 0 and 1) at the price of idle lanes in a kernel that
// is bound by the table stream. P and Q stream from global, row-coalesced; G
// (or B) is staged once through LDS, row stride 25, and read by rows for the
// even class and by columns for the odd one. This is a single-right-hand-side
// GEMV at 0.1 flop per table byte: MFMA does not fit.
#include "common.h"
#include "launch_setup.h"

#define QA_KD_BPW 4    // blocks per workgroup of the apply
#define QA_KD_LDG 25   // LDS row stride of the staged G

// corner of (class, cic): low three bits cic, t bit from the class
__device__ __forceinline__ int kd_corner(int cls, int cic) {
  return cic | (((__popc(cic) + cls) & 1) << 3);
}

// parity-major global site of corner `corner` of block `blk` (x-fastest)
__device__ __forceinline__ long kd_site(long blk, int corner, const LatDims &d,
                                        int *par) {
  int bx = d.X[0] >> 1, by = d.X[1] >> 1, bz = d.X[2] >> 1;
  int x[4];
  x[0] = 2 * (int)(blk % bx) + (corner & 1);
  long j = blk / bx;
  x[1] = 2 * (int)(j % by) + ((corner >> 1) & 1);
  j /= by;
  x[2] = 2 * (int)(j % bz) + ((corner >> 2) & 1);
  x[3] = 2 * (int)(j / bz) + ((corner >> 3) & 1);
  *par = (x[0] + x[1] + x[2] + x[3] + d.parity_offset) & 1;
  return cb_from_coords(x, d);
}

template <typename T>
__device__ __forceinline__ long kd_pq_index(long blk, int k, int row) {
  constexpr int KV = 16 / (int)sizeof(cplx<T>);
  return blk * 1152 + ((long)(k / KV) * 48 + row) * KV + (k % KV);
}

// ---------------------------------------------------------------------------
// build
// ---------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(64) void k_kd_build(
    cplx<T> *tab, const cplx<double> *u, LatDims d, long nblk, double mass) {
  using Z = cplx<double>;
  __shared__ Z sB[24 * 24], sA[24 * 24], sW[24 * 24];
  const int lane = threadIdx.x;
  const long blk = blockIdx.x;
  cplx<T> *tPQ = tab, *tG = tab + 1152 * nblk, *tB = tab + 1728 * nblk;
  const double m2 = 2.0 * mass, m4 = 4.0 * mass * mass;

  for (int e = lane; e < 576; e += 64) sB[e] = Z(0.0, 0.0);
  __syncthreads();
  // the 32 in-block links: per mu the 8 corners with c_mu = 0, 9 entries each
  for (int e = lane; e < 288; e += 64) {
    int l = e / 9, ij = e - 9 * l, i = ij / 3, jc = ij - 3 * i;
    int mu = l >> 3, j8 = l & 7;
    int low = j8 & ((1 << mu) - 1);
    int cx = low | ((j8 >> mu) << (mu + 1));  // c_mu = 0
    int cy = cx | (1 << mu);
    int par;
    long cb = kd_site(blk, cx, d, &par);
    Z U = u[(((long)mu * 2 + par) * d.Vcb + cb) * 9 + ij];
    double eta = (__popc(low) & 1) ? -1.0 : 1.0;
    if ((__popc(cx) & 1) == 0)  // x even: row x, column x + mu, +eta U
      sB[((cx & 7) * 3 + i) * 24 + (cy & 7) * 3 + jc] = Z(eta * U.re, eta * U.im);
    else                        // x odd: row x + mu, column x, -eta U^d
      sB[((cy & 7) * 3 + jc) * 24 + (cx & 7) * 3 + i] = Z(-eta * U.re, eta * U.im);
  }
  __syncthreads();
  for (int e = lane; e < 576; e += 64) tB[blk * 576 + e] = cplx<T>((T)sB[e].re, (T)sB[e].im);

  for (int side = 0; side < 2; ++side) {
    // A = 4m^2 + B B^d (even) or 4m^2 + B^d B (odd), lower triangle
    for (int e = lane; e < 576; e += 64) {
      int i = e / 24, j = e - 24 * i;
      if (j > i) continue;
      Z a(i == j ? m4 : 0.0, 0.0);
      for (int k = 0; k < 24; ++k) {
        if (side == 0)
          a = cfma_conj(sB[j * 24 + k], sB[i * 24 + k], a);
        else
          a = cfma_conj(sB[k * 24 + i], sB[k * 24 + j], a);
      }
      sA[e] = a;
    }
    __syncthreads();
    // right-looking Cholesky A = L L^d in place
    for (int j = 0; j < 24; ++j) {
      double dinv = 1.0 / sqrt(sA[j * 24 + j].re);
      __syncthreads();
      if (lane < 24 && lane >= j) {
        Z a = sA[lane * 24 + j];
        sA[lane * 24 + j] = lane == j ? Z(a.re * dinv, 0.0) : Z(a.re * dinv, a.im * dinv);
      }
      __syncthreads();
      for (int e = lane; e < 576; e += 64) {
        int i = e / 24, k = e - 24 * i;
        if (k > j && k <= i) {
          Z lij = sA[i * 24 + j], lkj = sA[k * 24 + j];
          // A[i][k] -= L[i][j] conj(L[k][j])
          sA[e] = cfma_conj(lkj, Z(-lij.re, -lij.im), sA[e]);
        }
      }
      __syncthreads();
    }
    // W = L^-1: lane c solves column c by forward substitution
    if (lane < 24) {
      const int c = lane;
      for (int i = 0; i < c; ++i) sW[i * 24 + c] = Z(0.0, 0.0);
      for (int i = c; i < 24; ++i) {
        Z s(i == c ? 1.0 : 0.0, 0.0);
        for (int k = c; k < i; ++k) {
          Z w = sW[k * 24 + c], l = sA[i * 24 + k];
          s = cfma(Z(-l.re, -l.im), w, s);
        }
        double di = 1.0 / sA[i * 24 + i].re;
        sW[i * 24 + c] = Z(s.re * di, s.im * di);
      }
    }
    __syncthreads();
    // E = W^d W into A (L is no longer needed)
    for (int e = lane; e < 576; e += 64) {
      int i = e / 24, j = e - 24 * i;
      Z a(0.0, 0.0);
      for (int k = (i > j ? i : j); k < 24; ++k)
        a = cfma_conj(sW[k * 24 + i], sW[k * 24 + j], a);
      sA[e] = a;
    }
    __syncthreads();
    for (int e = lane; e < 576; e += 64) {
      int i = e / 24, k = e - 24 * i;
      Z a = sA[e];
      tPQ[kd_pq_index<T>(blk, k, side * 24 + i)] = cplx<T>((T)(m2 * a.re), (T)(m2 * a.im));
      if (side == 0) {  // G = E B
        Z g(0.0, 0.0);
        for (int q = 0; q < 24; ++q) g = cfma(sA[i * 24 + q], sB[q * 24 + k], g);
        tG[blk * 576 + e] = cplx<T>((T)g.re, (T)g.im);
      }
    }
    __syncthreads();
  }
}

// ---------------------------------------------------------------------------
// apply
// ---------------------------------------------------------------------------
template <typename Prec, int KIND, bool DAG>
__global__ __launch_bounds__(64 * QA_KD_BPW) void k_kd_apply(
    StagAcc<Prec> out, StagAcc<Prec> in,
    const cplx<typename Prec::Real> *tab, LatDims d, long nblk,
    typename Prec::Real two_m) {
  using R = typename Prec::Real;
  using S = typename Prec::Store;
  using Acc = StagAcc<Prec>;
  using Zr = cplx<R>;
  constexpr int KV = 16 / (int)sizeof(Zr);
  static_assert(Acc::W == 2 && Acc::NCH == 3, "one colour per chunk");
  __shared__ Zr sv[QA_KD_BPW][48];
  __shared__ Zr sg[QA_KD_BPW][24 * QA_KD_LDG];

  const int lane = threadIdx.x & 63, wb = threadIdx.x >> 6;
  const long blk = (long)blockIdx.x * QA_KD_BPW + wb;
  const bool live = blk < nblk, owner = live && lane < 48;
  const int cls = lane >= 24 ? 1 : 0, r = lane - 24 * cls;
  const int col = r % 3;
  long gs = 0;

  if (live) {
    // G for X^-1, B for X: 576 entries, 9 per lane, coalesced
    const Zr *src = tab + (KIND == 1 ? 1152 : 1728) * nblk + blk * 576;
#pragma unroll
    for (int j = 0; j < 9; ++j) {
      int e = lane + 64 * j;
      sg[wb][(e / 24) * QA_KD_LDG + e % 24] = src[e];
    }
  }
  if (owner) {
    int par;
    long cb = kd_site(blk, kd_corner(cls, r / 3), d, &par);
    gs = par * d.Vcb + cb;
    S raw[2];
    in.template load_chunks<1>(raw, gs, col);
    R scale = (R)1;
    if constexpr (Prec::has_norm) scale = in.norm[gs];
    Zr v;
    qa_dequantize<Prec, 1>(&v, raw, scale);
    sv[wb][lane] = v;
  }
  __syncthreads();

  Zr acc((R)0, (R)0);
  if (owner) {
    const Zr *vd = sv[wb] + 24 * cls, *vx = sv[wb] + 24 * (1 - cls);
    if constexpr (KIND == 1) {
      const Zr *pq = tab + blk * 1152 + (long)lane * KV;
      Zr t[24];
#pragma unroll
      for (int kk = 0; kk < 24 / KV; ++kk)
        *reinterpret_cast<chunk16 *>(t + kk * KV) =
            *reinterpret_cast<const chunk16 *>(pq + (long)kk * 48 * KV);
#pragma unroll
      for (int k = 0; k < 24; ++k) acc = cfma(t[k], vd[k], acc);
    } else {
      acc = two_m * vd[r];
    }
    // upper rows: -/+ G v_o; lower rows: +/- G^d v_e (X: G = -B)
    Zr off((R)0, (R)0);
    const Zr *g = sg[wb];
    if (cls == 0) {
#pragma unroll
      for (int k = 0; k < 24; ++k) off = cfma(g[r * QA_KD_LDG + k], vx[k], off);
    } else {
#pragma unroll
      for (int k = 0; k < 24; ++k) off = cfma_conj(g[k * QA_KD_LDG + r], vx[k], off);
    }
    constexpr bool upper_minus = (KIND == 1) != DAG;
    const bool minus = upper_minus == (cls == 0);
    acc = minus ? acc - off : acc + off;
  }

  if constexpr (Prec::has_norm) {
    // site maximum over the three colour lanes (never split over waves)
    R m = fmax(fabs(acc.re), fabs(acc.im));
    const int base = lane - col;
    R m0 = __shfl(m, base), m1 = __shfl(m, base + 1), m2 = __shfl(m, base + 2);
    m = fmax(m0, fmax(m1, m2));
    if (owner) {
      R inv = m > (R)0 ? (R)1 / m : (R)0;
      S tmp[2] = {qa_tos<S>(acc.re * inv), qa_tos<S>(acc.im * inv)};
      if (col == 0) out.norm[gs] = m;
      store_chunk<S, Acc::W>(
          out.data + out.chunk_base(gs) + (long)col * out.V * Acc::W, tmp);
    }
  } else if (owner) {
    S tmp[2];
    qa_quantize<Prec, 1>(tmp, &acc);
    out.template store_chunks<1>(tmp, gs, col);
  }
}

// ---------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------
bool qa_kd_grid_ok(const KdCall &c) {
  return c.nblk > 0 && c.nblk < (1L << 31) - QA_KD_BPW &&
         16 * c.nblk == 2 * c.lat.Vcb;
}

bool launch_kd_build(const KdCall &c, hipStream_t st) {
  if (!qa_kd_grid_ok(c) || !c.table || !c.gauge) return false;
  LatDims d = lat_dims(c.lat);
  dim3 grid((unsigned)c.nblk), block(64);
  switch (c.table_prec) {
    case 0:
      hipLaunchKernelGGL(k_kd_build<double>, grid, block, 0, st,
                         (cplx<double> *)c.table,
                         (const cplx<double> *)c.gauge, d, c.nblk, c.mass);
      return true;
    case 1:
      hipLaunchKernelGGL(k_kd_build<float>, grid, block, 0, st,
                         (cplx<float> *)c.table,
                         (const cplx<double> *)c.gauge, d, c.nblk, c.mass);
      return true;
  }
  return false;
}

template <typename Prec, int KIND, bool DAG>
static bool kd_launch(const KdCall &c, hipStream_t st) {
  using R = typename Prec::Real;
  unsigned grid = (unsigned)((c.nblk + QA_KD_BPW - 1) / QA_KD_BPW);
  hipLaunchKernelGGL((k_kd_apply<Prec, KIND, DAG>), dim3(grid),
                     dim3(64 * QA_KD_BPW), 0, st, stag_acc<Prec>(c.out),
                     stag_acc<Prec>(c.in), (const cplx<R> *)c.table,
                     lat_dims(c.lat), c.nblk, (R)(2.0 * c.mass));
  return true;
}

template <typename Prec>
static bool kd_kind(const KdCall &c, hipStream_t st) {
  // the table type follows the field: double for double, float otherwise
  if (c.table_prec != (sizeof(typename Prec::Real) == 8 ? 0 : 1)) return false;
  switch (2 * c.kind + (c.dagger ? 1 : 0)) {
    case 0: return kd_launch<Prec, 0, false>(c, st);
    case 1: return kd_launch<Prec, 0, true>(c, st);
    case 2: return kd_launch<Prec, 1, false>(c, st);
    case 3: return kd_launch<Prec, 1, true>(c, st);
  }
  return false;
}

bool launch_kd_apply(const KdCall &c, hipStream_t st) {
  if (!qa_kd_grid_ok(c) || !c.table) return false;
  if (c.out.data == c.in.data) return false;  // in-place stays on the torch path
  switch (c.prec) {
    case 0: return kd_kind<PrecDouble>(c, st);
    case 1: return kd_kind<PrecSingle>(c, st);
    case 2: return kd_kind<PrecHalf>(c, st);
  }
  return false;
}
