// Laplace-family TU: covariant hop sum on full-parity fields (laplace.h)
#include "laplace.h"
#include "launch_setup.h"

template <typename Prec, int RECON, int NS, int CPT>
static bool lap_launch(const LaplaceCall &c, hipStream_t st) {
  using R = typename Prec::Real;
  auto out = spinor_acc<Prec, 6 * NS>(c.out), in = spinor_acc<Prec, 6 * NS>(c.in);
  // seen from parity 0: data = parity 0 block, other = parity 1 block
  auto g = gauge_acc<Prec, RECON>(c.gauge, 0, c.lat.Vcb);
  LatDims d = lat_dims(c.lat);
  long n = 2 * c.lat.Vcb * (NS / CPT);
  int grid = (int)((n + QA_LAP_BLOCK - 1) / QA_LAP_BLOCK);
  R a = (R)c.a, b = (R)c.b;
  if (c.nbr_link) {
    if (c.shift != 1) return false;  // the neighbour's slot holds U(x - mu)
    hipLaunchKernelGGL((k_laplace<Prec, RECON, NS, CPT, true>), dim3(grid),
                       dim3(QA_LAP_BLOCK), 0, st, out, in, g, d, c.hops,
                       c.shift, a, b, n);
  } else {
    hipLaunchKernelGGL((k_laplace<Prec, RECON, NS, CPT, false>), dim3(grid),
                       dim3(QA_LAP_BLOCK), 0, st, out, in, g, d, c.hops,
                       c.shift, a, b, n);
  }
  return true;
}

template <typename Prec, int NS, int CPT>
static bool lap_recon(const LaplaceCall &c, hipStream_t st) {
  if (c.recon == 18) return lap_launch<Prec, 18, NS, CPT>(c, st);
  if (c.recon == 12) return lap_launch<Prec, 12, NS, CPT>(c, st);
  return false;
}

// columns per thread: 0 asks for the measured default of the precision
// (profiles/r11_laplace.md)
static bool lap_double(const LaplaceCall &c, hipStream_t st) {
  if (c.nspin == 1) return c.cpt <= 1 && lap_recon<PrecDouble, 1, 1>(c, st);
  switch (c.cpt ? c.cpt : QA_LAP_CPT_DOUBLE) {
    case 1: return lap_recon<PrecDouble, 4, 1>(c, st);
    case 2: return lap_recon<PrecDouble, 4, 2>(c, st);
    case 4: return lap_recon<PrecDouble, 4, 4>(c, st);
  }
  return false;
}

static bool lap_single(const LaplaceCall &c, hipStream_t st) {
  if (c.nspin == 1) return c.cpt <= 1 && lap_recon<PrecSingle, 1, 1>(c, st);
  switch (c.cpt ? c.cpt : QA_LAP_CPT_SINGLE) {
    case 2: return lap_recon<PrecSingle, 4, 2>(c, st);
    case 4: return lap_recon<PrecSingle, 4, 4>(c, st);
  }
  return false;
}

static bool lap_half(const LaplaceCall &c, hipStream_t st) {
  if (c.nspin == 1) return c.cpt <= 1 && lap_recon<PrecHalf, 1, 1>(c, st);
  if (c.cpt == 0 || c.cpt == 4) return lap_recon<PrecHalf, 4, 4>(c, st);
  return false;
}

bool launch_laplace(const LaplaceCall &c, hipStream_t st) {
  if (c.nspin != 4 && c.nspin != 1) return false;
  if (c.shift != 1 && c.shift != 2) return false;
  if (c.out.data == c.in.data) return false;  // neighbours are read from in
  switch (c.prec) {
    case 0: return lap_double(c, st);
    case 1: return lap_single(c, st);
    case 2: return lap_half(c, st);
  }
  return false;
}
