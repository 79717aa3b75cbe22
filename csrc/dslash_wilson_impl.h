// Shared runtime->template dispatch for the Wilson dslash TUs.
#pragma once
#include <cstdlib>

#include "dslash_wilson.h"
#include "launch_setup.h"

template <typename Prec, int RECON>
static void dslash_launch_all(const DslashCall &c, hipStream_t st) {
  using R = typename Prec::Real;
  const long Vcb = c.lat.Vcb;  // 4-d cb volume (the fields carry their stride)
  auto out = spinor_acc<Prec>(c.out), in = spinor_acc<Prec>(c.in),
       x = spinor_acc<Prec>(c.x);
  auto g = gauge_acc<Prec, RECON>(c.gauge, c.parity, Vcb);
  CloverAcc<Prec> cl{(const typename Prec::Store *)c.clover, Vcb};
  LatDims d = lat_dims(c.lat);
  auto gh = ghost_acc<GhostAcc<Prec>>(c.halo);
  int blk = qa_dslash_block();
  int grid = (int)((Vcb + blk - 1) / blk);
  R a = (R)c.a;
  R br = (R)c.b_re, bi = (R)c.b_im;
  long n_ext = exterior_threads(c.halo);
  int grid_ext = (int)((n_ext + blk - 1) / blk);

  // double has one form: its 4-round body at the 3-wave cap would spill
  constexpr bool kCapForm = sizeof(R) != 8;
  int waves = kCapForm ? qa_dslash_waves() : 0;
  int grid64 = (int)((Vcb + 63) / 64);

  // fused-epilogue kernels (k_dslash_wilson_clov_out2 / _xpay_dot): dispatched
  // apart from the QA_MODES matrix so only the combinations MdagM uses are
  // instantiated — CLOV_POST x {xpay, no xpay} with out2, dagger PLAIN xpay
  // with dot; kt 0/1, default occupancy form only. The caller checked
  // qa_dslash_epilogue_ok.
  if (c.out2.data || c.y.data) {
    auto out2 = spinor_acc<Prec>(c.out2), y = spinor_acc<Prec>(c.y);
#define QA_EPI_LAUNCH(KERNEL, KT, ...)                                         \
  hipLaunchKernelGGL((KERNEL<Prec, RECON, __VA_ARGS__, KT>), dim3(grid),       \
                     dim3(blk), 0, st, out, in, g, cl, d, c.parity, a, x, gh,  \
                     QA_EPI_TAIL)
    if (c.out2.data) {
#define QA_EPI_TAIL out2
      if (c.kt == 0) {
        if (c.xpay) { QA_EPI_LAUNCH(k_dslash_wilson_clov_out2, KT_LOCAL, false, true); }
        else { QA_EPI_LAUNCH(k_dslash_wilson_clov_out2, KT_LOCAL, false, false); }
      } else {
        if (c.xpay) { QA_EPI_LAUNCH(k_dslash_wilson_clov_out2, KT_FUSED, false, true); }
        else { QA_EPI_LAUNCH(k_dslash_wilson_clov_out2, KT_FUSED, false, false); }
      }
#undef QA_EPI_TAIL
    } else {
#define QA_EPI_TAIL y, c.dot_result, c.dot_slots, c.dot_stride
      if (c.kt == 0) { QA_EPI_LAUNCH(k_dslash_wilson_xpay_dot, KT_LOCAL, true); }
      else { QA_EPI_LAUNCH(k_dslash_wilson_xpay_dot, KT_FUSED, true); }
#undef QA_EPI_TAIL
    }
#undef QA_EPI_LAUNCH
    return;
  }

  // LDS-tiled path (half/quarter, local, 4-d, tile-divisible dims,
  // PLAIN/CLOV_POST/TWIST_POST): see k_dslash_wilson_lds
  if constexpr (Prec::has_norm) {
    const int *X = c.lat.Xdim;
    bool lds_ok = qa_dslash_lds() && c.kt == 0 && c.halo.comm_mask == 0 &&
                  c.in.Vcb == Vcb && c.out.Vcb == Vcb &&
                  (c.mode == PLAIN || c.mode == CLOV_POST ||
                   c.mode == TWIST_POST) &&
                  X[0] % LdsTile::BX == 0 && X[1] % LdsTile::BY == 0 &&
                  X[2] % LdsTile::BZ == 0 && X[3] % LdsTile::BT == 0;
    if (lds_ok) {
      long ntile = ((long)X[0] / LdsTile::BX) * (X[1] / LdsTile::BY) *
                   (X[2] / LdsTile::BZ) * (X[3] / LdsTile::BT);
#define QA_LDS_LAUNCH(DAG, MODE, XPAY)                                         \
  hipLaunchKernelGGL((k_dslash_wilson_lds<Prec, RECON, DAG, MODE, XPAY>),      \
                     dim3((unsigned)ntile), dim3(256), 0, st, out, in, g, cl,  \
                     d, c.parity, a, x, br, bi)
#define QA_LDS_MODES(DAG)                                                      \
  switch (c.mode) {                                                            \
    case PLAIN:                                                                \
      if (c.xpay) QA_LDS_LAUNCH(DAG, PLAIN, true);                             \
      else QA_LDS_LAUNCH(DAG, PLAIN, false);                                   \
      break;                                                                   \
    case CLOV_POST:                                                            \
      if (c.xpay) QA_LDS_LAUNCH(DAG, CLOV_POST, true);                         \
      else QA_LDS_LAUNCH(DAG, CLOV_POST, false);                               \
      break;                                                                   \
    case TWIST_POST:                                                           \
      if (c.xpay) QA_LDS_LAUNCH(DAG, TWIST_POST, true);                        \
      else QA_LDS_LAUNCH(DAG, TWIST_POST, false);                              \
      break;                                                                   \
  }
      if (!c.dagger) { QA_LDS_MODES(false) } else { QA_LDS_MODES(true) }
#undef QA_LDS_MODES
#undef QA_LDS_LAUNCH
      return;
    }
  }

#define QA_LAUNCH(DAG, MODE, XPAY, KT)                                        \
  do {                                                                        \
    if (c.kt == 3) {                                                          \
      hipLaunchKernelGGL((k_dslash_wilson_exterior<Prec, RECON, DAG, MODE, XPAY>), \
                         dim3(grid_ext), dim3(blk), 0, st, out, in, g, cl, d, \
                         c.parity, a, x, gh, n_ext, br, bi);                  \
      break;                                                                  \
    }                                                                         \
    if constexpr (kCapForm) {                                                 \
      if (waves == 3) {                                                       \
        hipLaunchKernelGGL((k_dslash_wilson<Prec, RECON, DAG, MODE, XPAY, KT, 3>), \
                           dim3(grid64), dim3(64), 0, st, out, in, g, cl, d,  \
                           c.parity, a, x, gh, br, bi);                       \
        break;                                                                \
      }                                                                       \
    }                                                                         \
    hipLaunchKernelGGL((k_dslash_wilson<Prec, RECON, DAG, MODE, XPAY, KT>),   \
                       dim3(grid), dim3(blk), 0, st, out, in, g, cl, d,       \
                       c.parity, a, x, gh, br, bi);                           \
  } while (0)

#define QA_MODES(DAG, KT)                                                      \
  switch (c.mode) {                                                            \
    case PLAIN:                                                                \
      if (c.xpay) QA_LAUNCH(DAG, PLAIN, true, KT);                             \
      else QA_LAUNCH(DAG, PLAIN, false, KT);                                   \
      break;                                                                   \
    case CLOV_POST:                                                            \
      if (c.xpay) QA_LAUNCH(DAG, CLOV_POST, true, KT);                         \
      else QA_LAUNCH(DAG, CLOV_POST, false, KT);                               \
      break;                                                                   \
    case CLOV_X: QA_LAUNCH(DAG, CLOV_X, true, KT); break;                      \
    case TWIST_POST:                                                           \
      if (c.xpay) QA_LAUNCH(DAG, TWIST_POST, true, KT);                        \
      else QA_LAUNCH(DAG, TWIST_POST, false, KT);                              \
      break;                                                                   \
    case TWIST_X: QA_LAUNCH(DAG, TWIST_X, true, KT); break;                    \
    case CLOVTW_X: QA_LAUNCH(DAG, CLOVTW_X, true, KT); break;                  \
  }

#define QA_DISPATCH(KT)                                                        \
  if (!c.dagger) { QA_MODES(false, KT) } else { QA_MODES(true, KT) }

  switch (c.kt) {
    case 0: { QA_DISPATCH(KT_LOCAL) } break;
    case 1: { QA_DISPATCH(KT_FUSED) } break;
    case 2: { QA_DISPATCH(KT_INTERIOR) } break;
    case 3: { QA_DISPATCH(KT_LOCAL) } break;  // KT arg unused for exterior
  }
#undef QA_DISPATCH
#undef QA_MODES
#undef QA_LAUNCH
}

template <typename Prec>
static void pack_launch(const PackCall &c, hipStream_t st) {
  auto in = spinor_acc<Prec>(c.in);
  LatDims d = lat_dims(c.lat);
  int blk = 256;
  int grid = (int)((c.Fcb + blk - 1) / blk);
  auto *dst = (typename Prec::Store *)c.dst;

#define QA_PACK(MU, S01, EDGE)                                                 \
  hipLaunchKernelGGL((k_pack_face<Prec, MU, S01, EDGE>), dim3(grid), dim3(blk),\
                     0, st, dst, c.dst_nrm, in, d, c.parity, c.Fcb)
#define QA_PACK_MU(MU)                                                         \
  case MU:                                                                     \
    if (c.s01 == 0) { if (c.edge) QA_PACK(MU, 0, true); else QA_PACK(MU, 0, false); } \
    else            { if (c.edge) QA_PACK(MU, 1, true); else QA_PACK(MU, 1, false); } \
    break;

  switch (c.mu) {
    QA_PACK_MU(0)
    QA_PACK_MU(1)
    QA_PACK_MU(2)
    QA_PACK_MU(3)
  }
#undef QA_PACK_MU
#undef QA_PACK
}
