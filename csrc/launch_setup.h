// Host-side launch setup shared by the kernel TUs: turns the plain
// descriptors of launchers.h into the device-side accessor structs of
// common.h / halo.h. Host code only.
#pragma once
#include "common.h"
#include "launchers.h"

inline LatDims lat_dims(const LatDesc &l) {
  return LatDims{{l.Xdim[0], l.Xdim[1], l.Xdim[2], l.Xdim[3]}, l.parity_offset,
                 l.Vcb};
}

// BlasField.Vcb carries the CHUNK STRIDE (= Ls*Vcb for a 5-d field whose
// s-slice is addressed via a pointer offset), not the 4-d cb volume
template <typename Prec, int NCOMP = 24>
SpinorAcc<Prec, NCOMP> spinor_acc(const BlasField &f) {
  return {(typename Prec::Store *)f.data, (float *)f.norm, f.Vcb};
}

template <typename Prec>
StagAcc<Prec> stag_acc(const BlasField &f) {
  return spinor_acc<Prec, 6>(f);
}

// stencil-layout gauge [2][NCH][Vcb][W] seen from `parity`: the accessor's
// base is that parity's block, `other` the opposite one. Null stays null.
template <typename Prec, int RECON>
GaugeAcc<Prec, RECON> gauge_acc(const void *base, int parity, long Vcb) {
  const auto *g0 = (const typename Prec::Store *)base;
  if (!g0) return {nullptr, nullptr, Vcb};
  const long gpar = (long)GaugeAcc<Prec, RECON>::NCH * Vcb * Prec::W;
  return {g0 + parity * gpar, g0 + (1 - parity) * gpar, Vcb};
}

// Ghost = GhostAcc<Prec, NCOMP> (halo.h)
template <typename Ghost>
Ghost ghost_acc(const GhostDesc &h, int depth = 1) {
  Ghost gh{};
  gh.mask = h.comm_mask;
  for (int k = 0; k < 8; ++k) {
    gh.buf[k] = (const typename Ghost::S *)h.ghost[k];
    gh.nrm[k] = h.ghost_nrm[k];
  }
  for (int k = 0; k < 4; ++k) gh.Fcb[k] = h.face_cb[k];
  gh.depth = depth;
  return gh;
}

// threads of an exterior kernel: both faces of every partitioned dim
inline long exterior_threads(const GhostDesc &h) {
  long n = 0;
  for (int m = 0; m < 4; ++m)
    if ((h.comm_mask >> m) & 1) n += 2 * h.face_cb[m];
  return n;
}
