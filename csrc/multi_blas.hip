// Multi-BLAS family TU: vector-set dots and block caxpy (multi_blas.h)
#include <algorithm>

#include "multi_blas.h"
#include "table_cache.h"

namespace {

// grid-stride caps: a function of the shape alone, so that the number of
// partials, and with it the summation order, never depends on the device
constexpr long kCdotBlocks = 512;
constexpr long kCaxpyBlocks = 1024;

bool range_ok(const MultiBlasCall &c) {
  return c.nx >= 1 && c.nx <= QA_MB_MAXV && c.ny >= 1 && c.ny <= QA_MB_MAXV &&
         c.len >= 1;
}

template <int PREC>
bool cdot_t(const MultiBlasCall &c, hipStream_t st) {
  MbTab x{}, y{};
  for (int i = 0; i < c.nx; ++i) {
    x.data[i] = c.x[i].data;
    x.norm[i] = (const float *)c.x[i].norm;
  }
  for (int j = 0; j < c.ny; ++j) {
    y.data[j] = c.y[j].data;
    y.norm[j] = (const float *)c.y[j].norm;
  }
  MbHalfGeom hg{};
  if (PREC == 2) {
    if (c.len >= (1L << 31) || c.half_V < 1 || c.half_nchV < c.half_V)
      return false;
    if (c.half_cw != 1 && c.half_cw != 2 && c.half_cw != 4) return false;
    hg.cshift = c.half_cw == 4 ? 2 : c.half_cw == 2 ? 1 : 0;
    hg.V = (unsigned)c.half_V;
    hg.nchV = (unsigned)c.half_nchV;
  }
  const long nseg = (c.len + QA_MB_E - 1) / QA_MB_E;
  const int nbx = (c.nx + 31) / 32, nby = (c.ny + 31) / 32;
  const int pairs = c.same ? nbx * (nbx + 1) / 2 : nbx * nby;
  hipLaunchKernelGGL((k_multi_cdot<PREC>),
                     dim3((unsigned)multi_cdot_blocks(c.len), (unsigned)pairs),
                     dim3(QA_MB_BLOCK), 0, st, (double2 *)c.partial, x, y,
                     c.nx, c.ny, (int)c.same, c.len, nseg, hg);
  return true;
}

template <typename T>
bool caxpy_t(const MultiBlasCall &c, hipStream_t st) {
  using T2 = typename MbCaxpy<T>::T2;
  const auto *A =
      (const T2 *)device_table(c.A, (size_t)c.nx * c.ny * sizeof(T2));
  if (!A) return false;
  MbPtrs out{}, y{}, x{};
  for (int j = 0; j < c.nx; ++j) x.p[j] = c.x[j].data;
  for (int i = 0; i < c.ny; ++i) {
    out.p[i] = c.out[i].data;
    y.p[i] = c.beta ? c.y[i].data : c.out[i].data;
  }
  const long nseg = (c.len + MbCaxpy<T>::E - 1) / MbCaxpy<T>::E;
  hipLaunchKernelGGL((k_multi_caxpy<T>),
                     dim3((unsigned)std::min(nseg, kCaxpyBlocks),
                          (unsigned)((c.ny + 31) / 32)),
                     dim3(QA_MB_BLOCK), 0, st, out, y, x, A, c.ny, c.nx,
                     c.beta, c.len, nseg);
  return true;
}

}  // namespace

long multi_cdot_blocks(long len) {
  return std::min((len + QA_MB_E - 1) / QA_MB_E, kCdotBlocks);
}

bool launch_multi_cdot(const MultiBlasCall &c, hipStream_t st) {
  if (!range_ok(c) || (c.same && c.nx != c.ny)) return false;
  switch (c.prec) {
    case 0: return cdot_t<0>(c, st);
    case 1: return cdot_t<1>(c, st);
    case 2: return cdot_t<2>(c, st);
  }
  return false;
}

bool launch_multi_caxpy(const MultiBlasCall &c, hipStream_t st) {
  if (!range_ok(c) || (c.beta != 0 && c.beta != 1)) return false;
  switch (c.prec) {
    case 0: return caxpy_t<double>(c, st);
    case 1: return caxpy_t<float>(c, st);
  }
  return false;
}
