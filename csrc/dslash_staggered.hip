// staggered dslash TU (all precisions; kernel is small)
#include "dslash_staggered.h"
#include "launch_setup.h"

template <typename Prec, int RECON>
static void stag_launch(const StagDslashCall &c, hipStream_t st) {
  using R = typename Prec::Real;
  auto out = stag_acc<Prec>(c.out), in = stag_acc<Prec>(c.in),
       x = stag_acc<Prec>(c.x);
  auto g = gauge_acc<Prec, RECON>(c.gauge, c.parity, c.lat.Vcb);
  // 3-hop neighbors flip parity too (odd shift): bwd long links also read
  // the other parity block's fwd slots
  auto lng = gauge_acc<Prec, 18>(c.long_gauge, c.parity, c.lat.Vcb);
  LatDims d = lat_dims(c.lat);
  auto gh = ghost_acc<GhostAcc<Prec, 6>>(
      c.halo, c.ghost_depth > 0 ? c.ghost_depth : 1);
  int blk = 256;
  int grid = (int)((c.lat.Vcb + blk - 1) / blk);
  R a = (R)c.a, b = (R)c.b;
  long n_ext = exterior_threads(c.halo);
  int grid_ext = (int)((n_ext + blk - 1) / blk);

#define QA_SLAUNCH(XPAY, KT)                                                   \
  if (c.long_gauge)                                                            \
    hipLaunchKernelGGL((k_dslash_staggered<Prec, RECON, XPAY, KT, true>),      \
                       dim3(grid), dim3(blk), 0, st, out, in, g, lng, d,       \
                       c.parity, a, b, x, gh);                                 \
  else                                                                         \
    hipLaunchKernelGGL((k_dslash_staggered<Prec, RECON, XPAY, KT, false>),     \
                       dim3(grid), dim3(blk), 0, st, out, in, g, lng, d,       \
                       c.parity, a, b, x, gh)
  if (c.kt == 3) {
    hipLaunchKernelGGL((k_dslash_staggered_exterior<Prec, RECON>),
                       dim3(grid_ext), dim3(blk), 0, st, out, in, g, d,
                       c.parity, b, gh, n_ext);
  } else if (c.kt == 0) {
    if (c.xpay) QA_SLAUNCH(true, KT_LOCAL); else QA_SLAUNCH(false, KT_LOCAL);
  } else if (c.kt == 1) {
    if (c.xpay) QA_SLAUNCH(true, KT_FUSED); else QA_SLAUNCH(false, KT_FUSED);
  } else {
    if (c.xpay) QA_SLAUNCH(true, KT_INTERIOR); else QA_SLAUNCH(false, KT_INTERIOR);
  }
#undef QA_SLAUNCH
}

template <typename Prec>
static void stag_recon(const StagDslashCall &c, hipStream_t st) {
  if (c.recon == 12) stag_launch<Prec, 12>(c, st);
  else stag_launch<Prec, 18>(c, st);
}

void launch_dslash_staggered(const StagDslashCall &c, hipStream_t st) {
  switch (c.prec) {
    case 0: stag_recon<PrecDouble>(c, st); break;
    case 1: stag_recon<PrecSingle>(c, st); break;
    case 2: stag_recon<PrecHalf>(c, st); break;
  }
}

template <typename Prec>
static void stag_pack(const PackCall &c, hipStream_t st) {
  auto in = stag_acc<Prec>(c.in);
  LatDims d = lat_dims(c.lat);
  int blk = 256;
  int depth = c.depth > 0 ? c.depth : 1;
  long n = c.Fcb * depth;
  int grid = (int)((n + blk - 1) / blk);
  auto *dst = (typename Prec::Store *)c.dst;
  if (c.edge)
    hipLaunchKernelGGL((k_pack_face_stag<Prec, true>), dim3(grid), dim3(blk),
                       0, st, dst, c.dst_nrm, in, d, c.parity, c.mu, c.Fcb,
                       depth);
  else
    hipLaunchKernelGGL((k_pack_face_stag<Prec, false>), dim3(grid), dim3(blk),
                       0, st, dst, c.dst_nrm, in, d, c.parity, c.mu, c.Fcb,
                       depth);
}

void launch_pack_face_stag(const PackCall &c, hipStream_t st) {
  switch (c.prec) {
    case 0: stag_pack<PrecDouble>(c, st); break;
    case 1: stag_pack<PrecSingle>(c, st); break;
    case 2: stag_pack<PrecHalf>(c, st); break;
  }
}
