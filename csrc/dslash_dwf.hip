// DWF/Moebius 5th-dimension TU (all precisions)
#include <type_traits>

#include "dslash_dwf.h"
#include "launch_setup.h"
#include "table_cache.h"

namespace {

// Kernel pairs of the three families. HOP_5D: the hop runs a thread per 5-d
// site (the EOFA hop needs all of s for its rank-1 dot and runs per 4-d
// site, like every inverse).
template <typename Prec>
struct MobiusK {
  static constexpr bool HOP_5D = true;
  template <bool XPAY, bool DAG>
  static auto hop() { return &k_dslash5<Prec, XPAY, DAG>; }
  template <bool XPAY, bool DAG>
  static auto inv() { return &k_m5inv<Prec, XPAY, DAG>; }
};
template <typename Prec>
struct ZMobiusK {  // the dagger lives in the tables
  static constexpr bool HOP_5D = true;
  template <bool XPAY, bool>
  static auto hop() { return &k_zdslash5<Prec, XPAY>; }
  template <bool XPAY, bool>
  static auto inv() { return &k_zm5inv<Prec, XPAY>; }
};
template <typename Prec>
struct EofaK {
  static constexpr bool HOP_5D = false;
  template <bool XPAY, bool DAG>
  static auto hop() { return &k_m5_eofa<Prec, XPAY, DAG>; }
  template <bool XPAY, bool DAG>
  static auto inv() { return &k_m5inv_eofa<Prec, XPAY, DAG>; }
};

// The one launch of the family: picks the grid and the XPAY/DAG
// instantiation; `tail` are the kernel arguments after (out, in, x, Vcb4, Ls).
template <typename Prec, template <typename> class K, typename... Tail>
bool launch5(const Dwf5Call &c, hipStream_t st, Tail... tail) {
  auto out = spinor_acc<Prec>(c.out);
  auto in = spinor_acc<Prec>(c.in);
  auto x = spinor_acc<Prec>(c.x);
  const int blk = 256;
  auto go = [&](auto xpay, auto dag) {
    constexpr bool X = decltype(xpay)::value, D = decltype(dag)::value;
    if (c.kind == 0) {
      long n = K<Prec>::HOP_5D ? c.Vcb4 * c.Ls : c.Vcb4;
      hipLaunchKernelGGL((K<Prec>::template hop<X, D>()),
                         dim3((int)((n + blk - 1) / blk)), dim3(blk), 0, st,
                         out, in, x, c.Vcb4, c.Ls, tail...);
    } else {
      hipLaunchKernelGGL((K<Prec>::template inv<X, D>()),
                         dim3((int)((c.Vcb4 + blk - 1) / blk)), dim3(blk), 0,
                         st, out, in, x, c.Vcb4, c.Ls, tail...);
    }
  };
  std::true_type T;
  std::false_type F;
  if (c.xpay) { if (c.dagger) go(T, T); else go(T, F); }
  else        { if (c.dagger) go(F, T); else go(F, F); }
  return true;
}

template <typename Prec>
bool dwf5_t(const Mobius5Call &c, hipStream_t st) {
  using R = typename Prec::Real;
  return launch5<Prec, MobiusK>(c.f, st, (R)c.f.a, (R)c.alpha, (R)c.beta,
                                (R)c.mf);
}

template <typename Prec>
bool zdwf5_t(const ZDwf5Call &c, hipStream_t st) {
  using R = typename Prec::Real;
  auto *dzc = (const ZCoef *)device_table(c.zc, sizeof(ZCoef));
  if (!dzc) return false;
  return launch5<Prec, ZMobiusK>(c.f, st, (R)c.f.a, (R)c.a_im, dzc);
}

template <typename Prec>
bool eofa5_t(const Eofa5Call &c, hipStream_t st) {
  using R = typename Prec::Real;
  EofaVec ev{};
  for (int s = 0; s < c.f.Ls && s < QA_ZMAX; ++s) {
    ev.u[s] = c.u[s];
    ev.w[s] = c.w[s];
  }
  ev.sh = c.sh;
  ev.pm = c.pm;
  return launch5<Prec, EofaK>(c.f, st, (R)c.f.a, (R)c.alpha, (R)c.beta,
                              (R)c.mf, ev);
}

}  // namespace

bool launch_dwf5(const Mobius5Call &c, hipStream_t st) {
  switch (c.f.prec) {
    case 0: return dwf5_t<PrecDouble>(c, st);
    case 1: return dwf5_t<PrecSingle>(c, st);
    case 2: return dwf5_t<PrecHalf>(c, st);
    case 3: return dwf5_t<PrecQuarter>(c, st);
  }
  return false;
}

// double/single only: k_zm5inv's per-half read-modify-write would re-round
// the other chirality half of a block-float site
bool launch_zdwf5(const ZDwf5Call &c, hipStream_t st) {
  switch (c.f.prec) {
    case 0: return zdwf5_t<PrecDouble>(c, st);
    case 1: return zdwf5_t<PrecSingle>(c, st);
  }
  return false;
}

bool launch_eofa5(const Eofa5Call &c, hipStream_t st) {
  switch (c.f.prec) {
    case 0: return eofa5_t<PrecDouble>(c, st);
    case 1: return eofa5_t<PrecSingle>(c, st);
    case 2: return eofa5_t<PrecHalf>(c, st);
  }
  return false;
}
