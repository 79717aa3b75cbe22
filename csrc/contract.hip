// Contraction-family TU: site contraction, momentum slice sums, eigenvector
// sink projection (contract.h)
#include <algorithm>

#include "contract.h"
#include "launch_setup.h"
#include "table_cache.h"

namespace {

SliceGeom slice_geom(const LatDesc &l, int rd) {
  int o[3], n = 0;
  for (int m = 0; m < 4; ++m)
    if (m != rd) o[n++] = m;
  SliceGeom sg{};
  sg.rd = rd;
  sg.a = o[0];
  sg.b = o[1];
  sg.c = o[2];
  sg.Xah = l.Xdim[o[0]] / 2;
  sg.Xb = l.Xdim[o[1]];
  sg.ob = l.Xdim[o[0]];
  sg.oc = sg.ob + l.Xdim[o[1]];
  sg.ltot = sg.oc + l.Xdim[o[2]];
  sg.L = l.Xdim[rd];
  sg.Vs = 2 * l.Vcb / l.Xdim[rd];
  return sg;
}

GammaTab gamma_tab(const ContractCall &c) {
  GammaTab gt;
  for (int g = 0; g < 16; ++g) gt.w[g] = c.gamma[g];
  return gt;
}

int slices_ns(int ns) { return ns ? ns : QA_CT_NS; }
int evec_ne(int ne) { return ne ? ne : QA_CT_NE; }

// sites per thread of the projection: enough blocks to fill the device
// first, then longer tiles; a function of the shape alone
int evec_spt(const LatDesc &l, int rd) {
  long per_thread = 2 * l.Vcb / ((long)QA_CT_BLOCK * 1024);
  return (int)std::min<long>(8, std::max<long>(1, per_thread));
}

template <typename Prec>
bool site_t(const ContractCall &c, hipStream_t st) {
  long n = 2 * c.lat.Vcb;
  hipLaunchKernelGGL((k_contract_site<Prec>),
                     dim3((unsigned)((n + QA_CT_BLOCK - 1) / QA_CT_BLOCK)),
                     dim3(QA_CT_BLOCK), 0, st, (double2 *)c.out,
                     spinor_acc<Prec>(c.x), spinor_acc<Prec>(c.y),
                     lat_dims(c.lat), gamma_tab(c), c.dr);
  return true;
}

template <typename Prec, int NS>
bool slices_t(const ContractCall &c, hipStream_t st) {
  SliceGeom sg = slice_geom(c.lat, c.reduct_dim);
  const auto *f = (const double2 *)device_table(
      c.phases, (size_t)c.n_mom * sg.ltot * sizeof(double2));
  if (!f) return false;
  int pcr = 1;
  while (pcr < NS / 16 && pcr < c.n_mom) pcr *= 2;
  hipLaunchKernelGGL((k_contract_slices<Prec, NS>),
                     dim3((unsigned)contract_slice_tiles(c.lat, c.reduct_dim, NS),
                          (unsigned)sg.L),
                     dim3(NS), 0, st, (double2 *)c.out, spinor_acc<Prec>(c.x),
                     spinor_acc<Prec>(c.y), lat_dims(c.lat), sg, gamma_tab(c),
                     f, c.n_mom, pcr);
  return true;
}

template <typename Prec>
bool slices_ns_t(const ContractCall &c, hipStream_t st) {
  switch (slices_ns(c.ns)) {
    case 128: return slices_t<Prec, 128>(c, st);
    case 256: return slices_t<Prec, 256>(c, st);
  }
  return false;
}

template <typename Prec, int NE>
bool evec_t(const EvecProjectCall &c, hipStream_t st) {
  SliceGeom sg = slice_geom(c.lat, c.reduct_dim);
  int spt = evec_spt(c.lat, c.reduct_dim);
  dim3 grid((unsigned)evec_project_tiles(c.lat, c.reduct_dim), (unsigned)sg.L);
  for (int i0 = 0; i0 < c.n_ev; i0 += NE) {
    EvecTab<NE> tab{};
    int ne = std::min(NE, c.n_ev - i0);
    for (int i = 0; i < ne; ++i) {
      tab.data[i] = c.evecs[i0 + i].data;
      tab.norm[i] = (const float *)c.evecs[i0 + i].norm;
    }
    hipLaunchKernelGGL((k_evec_project<Prec, NE>), grid, dim3(QA_CT_BLOCK), 0,
                       st, (double2 *)c.out, spinor_acc<Prec>(c.psi), tab, ne,
                       i0, c.n_ev, lat_dims(c.lat), sg, spt);
  }
  return true;
}

template <typename Prec>
bool evec_ne_t(const EvecProjectCall &c, hipStream_t st) {
  switch (evec_ne(c.ne)) {
    case 4: return evec_t<Prec, 4>(c, st);
    case 8: return evec_t<Prec, 8>(c, st);
  }
  return false;
}

}  // namespace

long contract_slice_tiles(const LatDesc &l, int reduct_dim, int ns) {
  long Vs = 2 * l.Vcb / l.Xdim[reduct_dim];
  ns = slices_ns(ns);
  return (Vs + ns - 1) / ns;
}

long evec_project_tiles(const LatDesc &l, int reduct_dim) {
  long Vs = 2 * l.Vcb / l.Xdim[reduct_dim];
  long tile = (long)QA_CT_BLOCK * evec_spt(l, reduct_dim);
  return (Vs + tile - 1) / tile;
}

bool launch_contract_site(const ContractCall &c, hipStream_t st) {
  switch (c.prec) {
    case 0: return site_t<PrecDouble>(c, st);
    case 1: return site_t<PrecSingle>(c, st);
    case 2: return site_t<PrecHalf>(c, st);
  }
  return false;
}

bool launch_contract_slices(const ContractCall &c, hipStream_t st) {
  if (c.reduct_dim < 0 || c.reduct_dim > 3 || c.n_mom < 1) return false;
  switch (c.prec) {
    case 0: return slices_ns_t<PrecDouble>(c, st);
    case 1: return slices_ns_t<PrecSingle>(c, st);
    case 2: return slices_ns_t<PrecHalf>(c, st);
  }
  return false;
}

bool launch_evec_project(const EvecProjectCall &c, hipStream_t st) {
  if (c.reduct_dim < 0 || c.reduct_dim > 3 || c.n_ev < 1) return false;
  switch (c.prec) {
    case 0: return evec_ne_t<PrecDouble>(c, st);
    case 1: return evec_ne_t<PrecSingle>(c, st);
    case 2: return evec_ne_t<PrecHalf>(c, st);
  }
  return false;
}
