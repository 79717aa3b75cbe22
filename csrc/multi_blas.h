// Multi-BLAS family: vector-set dots and block caxpy on the matrix cores
// (role of the reference's multi_reduce cDotProduct, multi_blas caxpy and
// rotateVecs; the design is this project's own).
//
// Double and single chunked-SoA fields are flat runs of complex numbers and
// both operations are position-wise, so a field is just `len` complex
// elements behind a pointer: nothing here knows nspin, parity count or Ls.
// Half adds the per-site norm, found from the chunk index of an element.
//
// A workgroup owns a contiguous segment of E elements of every vector of the
// call. The vectors live in separate allocations, so feeding the MFMA from
// global memory would fetch one 16-byte fragment per allocation; instead
// each vector's piece of the segment is loaded as full coalesced 16-byte
// transactions and written to LDS as rows [vector][element], from where a
// lane reads the operand the instruction wants: vector index along the MFMA
// row (or column), element index along K (dots) or along the column (caxpy).
//
//   k_multi_cdot   G[i,j] += sum_e conj(x_i[e]) y_j[e], always in double
//                  (v_mfma_f64_16x16x4_f64; single and half are decoded to
//                  double while staging, half as double(norm) *
//                  double(stored), which is exact). A 32 x 32 block of G is
//                  four 16 x 16 tiles, one per wave; smaller blocks split K
//                  among the waves instead. The accumulators live across the
//                  grid-stride loop over segments; each workgroup then adds
//                  its waves' pieces in a fixed order and writes one
//                  [N][M] partial. No atomics: the host adds the partials in
//                  block order.
//   k_multi_caxpy  out_i[e] = beta y_i[e] + sum_j A[i,j] x_j[e] in the storage
//                  type (f64 16x16x4, or f32 16x16x4 with two element tiles
//                  interleaved so that a lane owns two adjacent elements and
//                  stores 16 bytes). A block of 32 output rows of A sits in
//                  LDS for the life of the workgroup.
//
// Fragment maps of the 16x16x4 instructions, lane l:
//   A[i = l & 15][k = l >> 4], B[k = l >> 4][j = l & 15]
//   f32 D: rows 4 (l >> 4) + q, f64 D: rows 4 q + (l >> 4); column l & 15
#pragma once
#include <hip/hip_fp16.h>
#include <hip/hip_runtime.h>

#include "launchers.h"

#define QA_MB_BLOCK 256
#define QA_MB_E 64                // k_multi_cdot: elements per segment
#define QA_MB_LD (QA_MB_E + 1)    // its LDS row stride (conflict-free b128)
#define QA_MB_LDA (QA_MB_MAXV + 1)  // k_multi_caxpy: LDS row stride of A

using mb_f64x4 = __attribute__((ext_vector_type(4))) double;
using mb_f32x4 = __attribute__((ext_vector_type(4))) float;

struct MbTab {  // read-only operands of a launch
  const void *data[QA_MB_MAXV];
  const float *norm[QA_MB_MAXV];
};
struct MbPtrs {
  void *p[QA_MB_MAXV];
};
struct MbHalfGeom {  // where the norm of a half element lives
  unsigned cshift;   // log2(complex numbers per chunk)
  unsigned V;        // sites per parity (chunk stride)
  unsigned nchV;     // chunks per parity
};

// complex numbers per 16-byte unit
template <int PREC>
struct MbUnit {
  static constexpr int EPU = PREC == 0 ? 1 : PREC == 1 ? 2 : 4;
};

// elements [e0, e0 + EPU) of one vector as double, zero past len. e0 is a
// multiple of EPU; a unit that straddles the end is read element-wise
template <int PREC>
__device__ __forceinline__ void mb_load_unit(double2 *out, const void *data,
                                             const float *norm,
                                             const MbHalfGeom &hg, long e0,
                                             long len) {
  constexpr int EPU = MbUnit<PREC>::EPU;
  if constexpr (PREC == 0) {
    out[0] = e0 < len ? ((const double2 *)data)[e0] : make_double2(0., 0.);
  } else if constexpr (PREC == 1) {
    const float2 *p = (const float2 *)data + e0;
    float2 v[2] = {{0.f, 0.f}, {0.f, 0.f}};
    if (e0 + 2 <= len) {
      float4 w = *(const float4 *)p;
      v[0] = {w.x, w.y};
      v[1] = {w.z, w.w};
    } else if (e0 < len) {
      v[0] = p[0];
    }
    out[0] = make_double2((double)v[0].x, (double)v[0].y);
    out[1] = make_double2((double)v[1].x, (double)v[1].y);
  } else {
    const unsigned *p = (const unsigned *)data + e0;  // one __half2 each
    unsigned w[4] = {0u, 0u, 0u, 0u};
    if (e0 + 4 <= len) {
      const uint4 u = *(const uint4 *)p;
      w[0] = u.x;
      w[1] = u.y;
      w[2] = u.z;
      w[3] = u.w;
    } else {
#pragma unroll
      for (int n = 0; n < 4; ++n)
        if (e0 + n < len) w[n] = p[n];
    }
    unsigned qprev = 0;
    double scale = 0.;
#pragma unroll
    for (int n = 0; n < EPU; ++n) {
      unsigned q = (unsigned)(e0 + n) >> hg.cshift;
      if ((n == 0 || q != qprev) && e0 + n < len)
        scale = (double)norm[(q / hg.nchV) * hg.V + q % hg.V];
      qprev = q;
      const float2 f = __half22float2(*(const __half2 *)&w[n]);
      out[n] = e0 + n < len
                   ? make_double2(scale * (double)f.x, scale * (double)f.y)
                   : make_double2(0., 0.);
    }
  }
}

// rows [0, rows) of S <- segment seg of vectors v0 .. v0 + nv of tab, rows
// past nv zero. A wave loads one vector's piece (double), two (single) or
// four (half), each piece a run of full 16-byte transactions.
template <int PREC>
__device__ __forceinline__ void mb_stage(double2 *S, const MbTab &tab, int v0,
                                         int nv, int rows, long seg, long len,
                                         const MbHalfGeom &hg) {
  constexpr int EPU = MbUnit<PREC>::EPU;
  constexpr int UPV = QA_MB_E / EPU;       // units per vector piece
  constexpr int VPP = QA_MB_BLOCK / UPV;   // vectors per pass
  const int u = threadIdx.x % UPV;
  const long e0 = seg * QA_MB_E + (long)u * EPU;
  for (int r = threadIdx.x / UPV; r < rows; r += VPP) {
    double2 v[EPU];
#pragma unroll
    for (int n = 0; n < EPU; ++n) v[n] = make_double2(0., 0.);
    if (r < nv)
      mb_load_unit<PREC>(v, tab.data[v0 + r], tab.norm[v0 + r], hg, e0, len);
#pragma unroll
    for (int n = 0; n < EPU; ++n) S[r * QA_MB_LD + u * EPU + n] = v[n];
  }
}

// out: [gridDim.x][N][M]. blockIdx.y names a 32 x 32 block (bx, by) of G;
// with same (y is x, M == N) only bx <= by are launched, a diagonal block
// stages its vectors once, and the lower triangle is written as the
// conjugate of the upper one, so that the result is exactly Hermitian.
template <int PREC>
__global__ __launch_bounds__(QA_MB_BLOCK, 2) void k_multi_cdot(
    double2 *__restrict__ out, MbTab x, MbTab y, int N, int M, int same,
    long len, long nseg, MbHalfGeom hg) {
  __shared__ double2 lds[2 * 32 * QA_MB_LD];
  const int t = threadIdx.x, wave = t >> 6, lane = t & 63;
  int bx, by;
  if (same) {  // (0,0) (0,1) (1,1)
    bx = blockIdx.y == 2;
    by = blockIdx.y != 0;
  } else {
    const int nbx = (N + 31) / 32;
    bx = blockIdx.y % nbx;
    by = blockIdx.y / nbx;
  }
  const int i0 = bx * 32, j0 = by * 32;
  const int nx = min(32, N - i0), ny = min(32, M - j0);
  const int nxt = (nx + 15) / 16, nyt = (ny + 15) / 16;
  const bool diag = same && bx == by;
  double2 *Xs = lds;
  double2 *Ys = diag ? lds : lds + 32 * QA_MB_LD;
  // 1, 2 or 4 tiles: the waves left over split the K range
  const int ntiles = nxt * nyt;
  const int ksteps = (QA_MB_E / 4) / (4 / ntiles);
  const int tile = wave % ntiles, kp = wave / ntiles;
  const int ti = tile % nxt, tj = tile / nxt;
  const int koff = kp * ksteps * 4 + (lane >> 4);
  const double2 *xa = Xs + (ti * 16 + (lane & 15)) * QA_MB_LD + koff;
  const double2 *yb = Ys + (tj * 16 + (lane & 15)) * QA_MB_LD + koff;
  mb_f64x4 Gr = {0., 0., 0., 0.}, Gi = {0., 0., 0., 0.};
  for (long seg = blockIdx.x; seg < nseg; seg += gridDim.x) {
    mb_stage<PREC>(Xs, x, i0, nx, nxt * 16, seg, len, hg);
    if (!diag) mb_stage<PREC>(Ys, y, j0, ny, nyt * 16, seg, len, hg);
    __syncthreads();
    for (int ks = 0; ks < ksteps; ++ks) {
      const double2 a = xa[ks * 4], b = yb[ks * 4];
      // conj(a) b: re = ar br + ai bi, im = ar bi - ai br
      Gr = __builtin_amdgcn_mfma_f64_16x16x4f64(a.x, b.x, Gr, 0, 0, 0);
      Gr = __builtin_amdgcn_mfma_f64_16x16x4f64(a.y, b.y, Gr, 0, 0, 0);
      Gi = __builtin_amdgcn_mfma_f64_16x16x4f64(a.x, b.y, Gi, 0, 0, 0);
      Gi = __builtin_amdgcn_mfma_f64_16x16x4f64(-a.y, b.x, Gi, 0, 0, 0);
    }
    __syncthreads();
  }
  // the waves' pieces, then the 32 x 32 block, both in the staging area
  double2 *part = lds;         // [wave][16][16]
  double2 *Gs = lds + 4 * 256;  // [32][32]
#pragma unroll
  for (int q = 0; q < 4; ++q)
    part[wave * 256 + (4 * q + (lane >> 4)) * 16 + (lane & 15)] =
        make_double2(Gr[q], Gi[q]);
  __syncthreads();
  for (int tl = 0; tl < ntiles; ++tl) {
    double2 s = make_double2(0., 0.);
    for (int k = 0; k < 4 / ntiles; ++k) {  // fixed order
      const double2 p = part[(k * ntiles + tl) * 256 + t];
      s.x += p.x;
      s.y += p.y;
    }
    Gs[((tl % nxt) * 16 + t / 16) * 32 + (tl / nxt) * 16 + t % 16] = s;
  }
  __syncthreads();
  double2 *o = out + (long)blockIdx.x * N * M;
  for (int idx = t; idx < 32 * 32; idx += QA_MB_BLOCK) {
    const int li = idx / 32, lj = idx % 32;
    if (li >= nx || lj >= ny) continue;
    double2 v = Gs[li * 32 + lj];
    if (diag) {
      if (li > lj) {
        v = Gs[lj * 32 + li];
        v.y = -v.y;
      } else if (li == lj) {
        v.y = 0.;
      }
    }
    o[(long)(i0 + li) * M + j0 + lj] = v;
    if (same && !diag)
      o[(long)(j0 + lj) * M + i0 + li] = make_double2(v.x, -v.y);
  }
}

// ---------------------------------------------------------------------------
// block caxpy / basis rotation in the storage type T (double or float)
template <typename T>
struct MbCaxpy;
template <>
struct MbCaxpy<double> {
  using T2 = double2;
  using Acc = mb_f64x4;
  static constexpr int E = 32;    // elements per segment: 2 tiles of 16
  static constexpr int EPU = 1;
};
template <>
struct MbCaxpy<float> {
  using T2 = float2;
  using Acc = mb_f32x4;
  static constexpr int E = 64;    // 2 tile pairs of 32
  static constexpr int EPU = 2;
};

__device__ __forceinline__ mb_f64x4 mb_mfma(double a, double b, mb_f64x4 c) {
  return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0);
}
__device__ __forceinline__ mb_f32x4 mb_mfma(float a, float b, mb_f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}

// A: device [NO][NI] row-major complex of type T. blockIdx.y names 32 output
// vectors. beta = 0 never reads y. No output may be one of the x.
template <typename T>
__global__ __launch_bounds__(QA_MB_BLOCK, 2) void k_multi_caxpy(
    MbPtrs out, MbPtrs y, MbPtrs x, const typename MbCaxpy<T>::T2 *__restrict__ A,
    int NO, int NI, int beta, long len, long nseg) {
  using C = MbCaxpy<T>;
  using T2 = typename C::T2;
  using Acc = typename C::Acc;
  constexpr int E = C::E, EPU = C::EPU, LDX = E + 2;
  constexpr int UPV = E / EPU, VPP = QA_MB_BLOCK / UPV;
  __shared__ __attribute__((aligned(16))) T2 Xs[QA_MB_MAXV * LDX];
  __shared__ __attribute__((aligned(16))) T2 As[32 * QA_MB_LDA];
  const int t = threadIdx.x, wave = t >> 6, lane = t & 63;
  const int io0 = blockIdx.y * 32;
  const int no = min(32, NO - io0);
  const int NI4 = (NI + 3) & ~3;
  for (int idx = t; idx < 32 * NI4; idx += QA_MB_BLOCK) {
    const int i = idx / NI4, j = idx % NI4;
    T2 a = {(T)0, (T)0};
    if (i < no && j < NI) a = A[(long)(io0 + i) * NI + j];
    As[i * QA_MB_LDA + j] = a;
  }
  const int it = wave & 1, et = wave >> 1;
  const int col = lane & 15, kq = lane >> 4;
  const bool active = it * 16 < no;
  const T2 *ap = As + (it * 16 + col) * QA_MB_LDA + kq;
  const T2 *xp = Xs + kq * LDX + et * (E / 2) + col * EPU;
  const int su = t % UPV;
  for (long seg = blockIdx.x; seg < nseg; seg += gridDim.x) {
    const long es = seg * E + (long)su * EPU;
    for (int r = t / UPV; r < NI4; r += VPP) {
      if constexpr (EPU == 1) {
        T2 v = {(T)0, (T)0};
        if (r < NI && es < len) v = ((const T2 *)x.p[r])[es];
        Xs[r * LDX + su] = v;
      } else {
        float4 w = {0.f, 0.f, 0.f, 0.f};
        if (r < NI) {
          const float2 *p = (const float2 *)x.p[r] + es;
          if (es + 2 <= len) {
            w = *(const float4 *)p;
          } else if (es < len) {
            w.x = p[0].x;
            w.y = p[0].y;
          }
        }
        *(float4 *)&Xs[r * LDX + su * 2] = w;
      }
    }
    __syncthreads();
    if (active) {
      // the lane's EPU adjacent elements of output rows irow(q)
      const long e = seg * E + et * (E / 2) + col * EPU;
      Acc Dr[EPU], Di[EPU];
#pragma unroll
      for (int n = 0; n < EPU; ++n)
#pragma unroll
        for (int q = 0; q < 4; ++q) Dr[n][q] = Di[n][q] = (T)0;
      if (beta) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int i = it * 16 + (EPU == 1 ? 4 * q + kq : 4 * kq + q);
          if (i < no && e < len) {
            const T2 *p = (const T2 *)y.p[io0 + i] + e;
            if (EPU == 2 && e + 2 <= len) {
              const float4 v = *(const float4 *)p;
              Dr[0][q] = v.x;
              Di[0][q] = v.y;
              Dr[EPU - 1][q] = v.z;
              Di[EPU - 1][q] = v.w;
            } else {
              const T2 v = p[0];
              Dr[0][q] = v.x;
              Di[0][q] = v.y;
            }
          }
        }
      }
      for (int j = 0; j < NI4; j += 4) {
        const T2 a = ap[j];
        T2 b[EPU];
        if constexpr (EPU == 1) {
          b[0] = xp[j * LDX];
        } else {
          const float4 w = *(const float4 *)&xp[j * LDX];
          b[0] = {w.x, w.y};
          b[1] = {w.z, w.w};
        }
#pragma unroll
        for (int n = 0; n < EPU; ++n) {
          Dr[n] = mb_mfma(a.x, b[n].x, Dr[n]);
          Dr[n] = mb_mfma(-a.y, b[n].y, Dr[n]);
          Di[n] = mb_mfma(a.x, b[n].y, Di[n]);
          Di[n] = mb_mfma(a.y, b[n].x, Di[n]);
        }
      }
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int i = it * 16 + (EPU == 1 ? 4 * q + kq : 4 * kq + q);
        if (i < no && e < len) {
          T2 *p = (T2 *)out.p[io0 + i] + e;
          if (EPU == 2 && e + 2 <= len)
            *(float4 *)p = make_float4((float)Dr[0][q], (float)Di[0][q],
                                       (float)Dr[EPU - 1][q],
                                       (float)Di[EPU - 1][q]);
          else
            p[0] = {Dr[0][q], Di[0][q]};
        }
      }
    }
    __syncthreads();
  }
}
