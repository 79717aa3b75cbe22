// SU(3) projections on a register-resident M3 (role of the reference's
// su3_project.cuh; re-derived). Every index is a compile-time constant and
// nothing here needs scratch.
//
// project_gs:    Gram-Schmidt on rows 0 and 1, row 2 = conj(row0 x row1)
//                (fields/gauge.py project_su3). Not gauge covariant.
// project_polar: W / det(W)^(1/3), W the U(3) polar factor of M
//                (fields/gauge.py project_su3_polar). Gauge covariant.
#pragma once
#include "su3_double.h"

namespace {

__device__ __forceinline__ void project_gs(M3 &U) {
  double n = 0.0;
#pragma unroll
  for (int c = 0; c < 3; ++c) n += U[0][c].re * U[0][c].re + U[0][c].im * U[0][c].im;
  n = sqrt(n);
#pragma unroll
  for (int c = 0; c < 3; ++c) U[0][c] = {U[0][c].re / n, U[0][c].im / n};
  cd d = cjmul(U[0][0], U[1][0]);
  d = cadd(d, cjmul(U[0][1], U[1][1]));
  d = cadd(d, cjmul(U[0][2], U[1][2]));
  n = 0.0;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    cd t = cmul(d, U[0][c]);
    U[1][c] = {U[1][c].re - t.re, U[1][c].im - t.im};
    n += U[1][c].re * U[1][c].re + U[1][c].im * U[1][c].im;
  }
  n = sqrt(n);
#pragma unroll
  for (int c = 0; c < 3; ++c) U[1][c] = {U[1][c].re / n, U[1][c].im / n};
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const int a = (c + 1) % 3, b = (c + 2) % 3;
    cd x = cmul(U[0][a], U[1][b]), y = cmul(U[0][b], U[1][a]);
    U[2][c] = {x.re - y.re, -(x.im - y.im)};
  }
}

// cofactor matrix C (adj(X) = C^T, X^-1 = C^T / det) and det X = sum_j
// X_0j C_0j; cyclic indices carry the signs
__device__ __forceinline__ cd mat_cofactors(M3 &C, const M3 &X) {
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const int i1 = (i + 1) % 3, i2 = (i + 2) % 3;
      const int j1 = (j + 1) % 3, j2 = (j + 2) % 3;
      cd p = cmul(X[i1][j1], X[i2][j2]), q = cmul(X[i1][j2], X[i2][j1]);
      C[i][j] = {p.re - q.re, p.im - q.im};
    }
  cd det = cmul(X[0][0], C[0][0]);
  det = cadd(det, cmul(X[0][1], C[0][1]));
  det = cadd(det, cmul(X[0][2], C[0][2]));
  return det;
}

// The polar factor by the scaled Newton iteration on M itself,
//     X <- (z X + (z X)^-dag) / 2,   z = |det X|^(-1/3),
// never through M^dag M (that would square the condition number). The
// inverse is the cofactor one: X^-dag = conj(C / det). The determinant
// scaling makes the singular values of z X multiply to one and tends to 1
// as X becomes unitary. The iteration converges quadratically, so once a
// step moves X by delta = ||X_{k+1} - X_k||_F < 2^-27 the iterate X_{k+1}
// is within delta^2 / 2 < 2^-55 of the limit: a quarter of a rounding.
// POLAR_MAX_ITER caps the trip count; a matrix of condition number 1e12
// needs 9 steps.
constexpr int POLAR_MAX_ITER = 16;
constexpr double POLAR_STOP2 = 0x1p-54;  // delta^2

__device__ __forceinline__ void project_polar(M3 &X) {
#pragma nounroll
  for (int it = 0; it < POLAR_MAX_ITER; ++it) {
    M3 C;
    const cd det = mat_cofactors(C, X);
    const double d2 = det.re * det.re + det.im * det.im;
    const double z = 1.0 / cbrt(sqrt(d2));
    // conj(C / det) / z = conj(C conj(det)) / (|det|^2 z)
    const double hz = 0.5 * z, hw = 0.5 / (d2 * z);
    double delta2 = 0.0;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        const cd w = cmulj(C[i][j], det);  // C conj(det)
        const cd n = {hz * X[i][j].re + hw * w.re, hz * X[i][j].im - hw * w.im};
        const double dr = n.re - X[i][j].re, di = n.im - X[i][j].im;
        delta2 += dr * dr + di * di;
        X[i][j] = n;
      }
    if (delta2 < POLAR_STOP2) break;
  }
  // det(W)^(1/3) on the principal branch: exp(i arg(det W) / 3)
  M3 C;
  const cd det = mat_cofactors(C, X);
  double s, c;
  sincos(atan2(det.im, det.re) / 3.0, &s, &c);
  const cd ph = {c, s};
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) X[i][j] = cmulj(X[i][j], ph);
}

}  // namespace
