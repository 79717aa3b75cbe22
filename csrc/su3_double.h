// Complex-double 3x3 helpers shared by the gauge kernels that work on the
// oracle tensor [4][2][Vcb][3][3] (csrc/heatbath.hip, csrc/gauge_path.hip).
// Every M3 index is a compile-time constant, so the matrices live in VGPRs.
#pragma once
#include <hip/hip_runtime.h>

namespace {

struct cd {
  double re, im;
};
__device__ __forceinline__ cd cmul(const cd &a, const cd &b) {
  return {a.re * b.re - a.im * b.im, a.re * b.im + a.im * b.re};
}
__device__ __forceinline__ cd cmulj(const cd &a, const cd &b) {  // a * conj(b)
  return {a.re * b.re + a.im * b.im, a.im * b.re - a.re * b.im};
}
__device__ __forceinline__ cd cjmul(const cd &a, const cd &b) {  // conj(a) * b
  return {a.re * b.re + a.im * b.im, a.re * b.im - a.im * b.re};
}
__device__ __forceinline__ cd cadd(const cd &a, const cd &b) {
  return {a.re + b.re, a.im + b.im};
}

using M3 = cd[3][3];

__device__ __forceinline__ void mat_mul(M3 &o, const M3 &a, const M3 &b) {
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      cd s = cmul(a[i][0], b[0][j]);
      s = cadd(s, cmul(a[i][1], b[1][j]));
      s = cadd(s, cmul(a[i][2], b[2][j]));
      o[i][j] = s;
    }
}

// o = a * b^dag
__device__ __forceinline__ void mat_mul_dag(M3 &o, const M3 &a, const M3 &b) {
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      cd s = cmulj(a[i][0], b[j][0]);
      s = cadd(s, cmulj(a[i][1], b[j][1]));
      s = cadd(s, cmulj(a[i][2], b[j][2]));
      o[i][j] = s;
    }
}

// o = a^dag * b
__device__ __forceinline__ void mat_dag_mul(M3 &o, const M3 &a, const M3 &b) {
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      cd s = cjmul(a[0][i], b[0][j]);
      s = cadd(s, cjmul(a[1][i], b[1][j]));
      s = cadd(s, cjmul(a[2][i], b[2][j]));
      o[i][j] = s;
    }
}

__device__ __forceinline__ void mat_acc(M3 &o, const M3 &a) {
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) o[i][j] = cadd(o[i][j], a[i][j]);
}

// gauge tensor accessor: base + (((mu*2+p)*V + i)*9 + r*3+c)
__device__ __forceinline__ void load_link(M3 &u, const cd *g, long V, int mu,
                                          int p, long i) {
  const cd *b = g + (((long)mu * 2 + p) * V + i) * 9;
#pragma unroll
  for (int k = 0; k < 9; ++k) u[k / 3][k % 3] = b[k];
}

__device__ __forceinline__ void store_link(cd *g, long V, int mu, int p,
                                           long i, const M3 &u) {
  cd *b = g + (((long)mu * 2 + p) * V + i) * 9;
#pragma unroll
  for (int k = 0; k < 9; ++k) b[k] = u[k / 3][k % 3];
}

__device__ __forceinline__ void mat_scale_add_eye(M3 &o, const M3 &a,
                                                  double s) {
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      o[i][j] = {a[i][j].re * s + (i == j ? 1.0 : 0.0), a[i][j].im * s};
    }
}

// exp of a traceless-antihermitian Q by scaling-and-squaring with an
// 8-term Taylor series (scale to 1-norm < 1/4, exact to ~1e-14)
__device__ __forceinline__ void mat_exp_ta(M3 &E, const M3 &Q) {
  // scale Q by 2^-s so its 1-norm < 0.25
  double n = 0.0;
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j)
      n += fabs(Q[i][j].re) + fabs(Q[i][j].im);
  int s = 0;
  double sc = 1.0;
  while (n * sc > 0.25 && s < 40) {
    sc *= 0.5;
    ++s;
  }
  M3 A;
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) A[i][j] = {Q[i][j].re * sc, Q[i][j].im * sc};
  // 8-term Horner Taylor: E = I + A(I + A/2 (I + A/3 (...)))
  M3 T, P;
  mat_scale_add_eye(T, A, 1.0 / 8.0);  // placeholder start: I + A/8
  for (int k = 7; k >= 1; --k) {
    mat_mul(P, A, T);
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        double f = 1.0 / k;
        P[i][j] = {P[i][j].re * f + (i == j ? 1.0 : 0.0), P[i][j].im * f};
      }
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = 0; j < 3; ++j) T[i][j] = P[i][j];
  }
  // square s times
  for (int k = 0; k < s; ++k) {
    mat_mul(P, T, T);
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = 0; j < 3; ++j) T[i][j] = P[i][j];
  }
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) E[i][j] = T[i][j];
}

}  // namespace
