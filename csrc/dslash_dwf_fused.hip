// Fused domain-wall TU: 4-d hop + dense per-chirality s-stage in one launch
// (double/single/half; recon 18 everywhere, recon 12 for single and half)
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "dslash_dwf_fused.h"
#include "launch_setup.h"

namespace {

// Device copy of the two Ls x Ls blocks, converted to the compute type on
// the host. Operators reuse a handful of matrices for their whole life, so
// the copies are cached by content: a steady-state launch does no
// host-to-device transfer.
template <typename R>
const R *dwf_fused_w(const double *W, int Ls) {
  static std::map<std::string, R *> cache;
  int dev = 0;
  (void)hipGetDevice(&dev);
  const size_t n = (size_t)2 * Ls * Ls;
  std::string key((const char *)&dev, sizeof(dev));
  key.append((const char *)W, n * sizeof(double));
  auto it = cache.find(key);
  if (it != cache.end()) return it->second;
  if (cache.size() >= 256) {  // hipFree waits for in-flight kernels
    for (auto &kv : cache) (void)hipFree(kv.second);
    cache.clear();
  }
  std::vector<R> host(n);
  for (size_t k = 0; k < n; ++k) host[k] = (R)W[k];
  R *dptr = nullptr;
  if (hipMalloc(&dptr, n * sizeof(R)) != hipSuccess) return nullptr;
  if (hipMemcpy(dptr, host.data(), n * sizeof(R), hipMemcpyHostToDevice) !=
      hipSuccess) {
    (void)hipFree(dptr);
    return nullptr;
  }
  cache.emplace(std::move(key), dptr);
  return dptr;
}

template <typename Prec, int RECON, int NS>
bool dwf_fused_t(const DwfFusedCall &c, hipStream_t st) {
  using R = typename Prec::Real;
  // the fields carry the chunk stride Ls*Vcb; c.lat.Vcb is the 4-d volume
  auto out = spinor_acc<Prec>(c.out), in = spinor_acc<Prec>(c.in),
       x = spinor_acc<Prec>(c.x);
  auto g = gauge_acc<Prec, RECON>(c.gauge, c.parity, c.lat.Vcb);
  LatDims d = lat_dims(c.lat);
  const R *W = nullptr;
  if (c.W) {
    W = dwf_fused_w<R>(c.W, c.Ls);
    if (!W) return false;
  }
  const unsigned grid = (unsigned)((c.lat.Vcb + NS - 1) / NS);
  const unsigned blk = (unsigned)(NS * c.Ls);
  const size_t lds = c.W ? (size_t)24 * c.Ls * NS * sizeof(R) : 0;
  const R a = (R)c.a;

#define QA_FUSED(DAG, XPAY, HASW)                                             \
  hipLaunchKernelGGL((k_dwf_fused<Prec, RECON, DAG, XPAY, HASW, NS>), dim3(grid), \
                     dim3(blk), lds, st, out, in, g, d, c.parity, a, x, c.Ls, \
                     W)
#define QA_FUSED_X(DAG, XPAY)                                                 \
  if (c.W) QA_FUSED(DAG, XPAY, true); else QA_FUSED(DAG, XPAY, false)
  if (!c.dagger) {
    if (c.xpay) { QA_FUSED_X(false, true); } else { QA_FUSED_X(false, false); }
  } else {
    if (c.xpay) { QA_FUSED_X(true, true); } else { QA_FUSED_X(true, false); }
  }
#undef QA_FUSED_X
#undef QA_FUSED
  return true;
}

}  // namespace

bool launch_dwf_fused(const DwfFusedCall &c, hipStream_t st) {
  if (c.Ls < 1 || c.Ls > QA_DWF_FUSED_LS_MAX) return false;
  // double always runs the 16-site tile (256 threads at Ls = 16)
  const bool wide = qa_dwf_fused_ns() == 32;
  switch (c.prec * 100 + c.recon) {
    case 18: return dwf_fused_t<PrecDouble, 18, 16>(c, st);
    case 118:
      return wide ? dwf_fused_t<PrecSingle, 18, 32>(c, st)
                  : dwf_fused_t<PrecSingle, 18, 16>(c, st);
    case 112:
      return wide ? dwf_fused_t<PrecSingle, 12, 32>(c, st)
                  : dwf_fused_t<PrecSingle, 12, 16>(c, st);
    case 218:
      return wide ? dwf_fused_t<PrecHalf, 18, 32>(c, st)
                  : dwf_fused_t<PrecHalf, 18, 16>(c, st);
    case 212:
      return wide ? dwf_fused_t<PrecHalf, 12, 32>(c, st)
                  : dwf_fused_t<PrecHalf, 12, 16>(c, st);
  }
  return false;
}
