// C++ launcher API between the HIP kernel TUs and bindings.cpp.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdlib>

// runtime-tunable workgroup size (set by the Python autotuner via the
// set_dslash_block binding; env QUDA_AMD_DSLASH_BLOCK seeds the default)
inline int &qa_dslash_block_ref() {
  static int blk = [] {
    const char *e = getenv("QUDA_AMD_DSLASH_BLOCK");
    int v = e ? atoi(e) : 64;  // 1 wave/WG measures best (see profiles/)
    return (v == 64 || v == 128 || v == 256) ? v : 64;
  }();
  return blk;
}
inline int qa_dslash_block() { return qa_dslash_block_ref(); }

// occupancy experiment: 0 = default (256-thread cap, ~2 waves/SIMD at the
// measured 222 VGPRs), 3 = 64-thread workgroups with __launch_bounds__
// forcing >= 3 waves/SIMD (VGPR cap 168). Only {0,3} are compiled.
// Double has one form (4 gather rounds, ~220 VGPRs, which the cap would
// spill): under 3 it launches its default kernel, and, the switch being
// precision-blind, still goes without the fused epilogues
// (qa_dslash_epilogue_ok), i.e. through the unfused launch sequence.
inline int &qa_dslash_waves_ref() {
  static int w = [] {
    const char *e = getenv("QUDA_AMD_DSLASH_WAVES");
    int v = e ? atoi(e) : 0;
    return v == 3 ? 3 : 0;
  }();
  return w;
}
inline int qa_dslash_waves() { return qa_dslash_waves_ref(); }

// LDS-tiled dslash policy (0 = off, 1 = on where eligible: half/quarter,
// local, 4-d, tile-divisible dims; set_dslash_lds binding / autotuner)
inline int &qa_dslash_lds_ref() {
  static int v = []() {
    const char *e = std::getenv("QUDA_AMD_DSLASH_LDS");
    return e ? std::atoi(e) : 0;
  }();
  return v;
}
inline int qa_dslash_lds() { return qa_dslash_lds_ref(); }

struct BlasField {
  void *data;
  void *norm;  // nullptr unless half
  long Vcb;    // chunk stride (cb volume)
};

enum BlasOp {
  BLAS_AXPY = 0,
  BLAS_AXPY_NORM2,
  BLAS_XPAY,
  BLAS_AXPBY,
  BLAS_CAXPY,
  BLAS_XMY_NORM2,
  BLAS_SCAL,
  BLAS_NORM2,
  BLAS_REDOT,
  BLAS_CDOT,
  BLAS_CAXPBY,
  BLAS_TRIPLE_CG,  // x += a p; r -= a Ap; -> ||r||^2 (ref tripleCGUpdate)
  // same update with alpha = a / result[0] formed on the device (a = the
  // host's r2_old, result[0] = pAp from the fused-dot dslash); ||r||^2 is
  // accumulated into result[1]; `clear` = the next iteration's accumulator
  BLAS_TRIPLE_CG_DEV,
};

struct BlasCall {
  int op;        // BlasOp
  int prec;      // 0 double, 1 single, 2 half
  double a, b;   // scalars (caxpy: a=re, b=im)
  double c, d;   // second complex scalar (caxpby: b=(c,d))
  BlasField x, y;
  BlasField z, w;  // extra operands (TRIPLE_CG: x=p, y=Ap, z=x, w=r)
  long sites;    // npar * Vcb
  int ncomp;     // reals per site: 24 (Wilson) or 6 (staggered)
  bool det;      // deterministic reduce: result = per-block partials
  double *result;  // device ptr (2 doubles, or [grid][2] partials if det)
  // TRIPLE_CG_DEV: pAp = result[0], or, with nslots > 0, the sum of
  // slots[s * slot_stride], s < nslots <= 64 (then also written to
  // result[0]); clear[0..clear_n) is zeroed by the kernel (null = nothing)
  double *clear;
  long clear_n;
  const double *slots;
  int nslots, slot_stride;
};

void launch_blas(const BlasCall &c, hipStream_t st);
void launch_convert(const BlasField &dst, int pdst, const BlasField &src,
                    int psrc, long sites, int ncomp, hipStream_t st);

// ---------------------------------------------------------------------------
// descriptors shared by the stencil-family call structs; launch_setup.h turns
// them into the device-side LatDims / GhostAcc
struct LatDesc {
  int Xdim[4];
  int parity_offset;
  long Vcb;  // cb volume
};

// ghost recv buffers per [2*mu+dir] (dir 1 = from +mu neighbor); null when
// mask bit mu unset. comm_mask==0 => pure-local kernel.
struct GhostDesc {
  const void *ghost[8];
  const float *ghost_nrm[8];
  long face_cb[4];
  int comm_mask;
};

struct DslashCall {
  // single-parity field views (data points at the parity slice)
  BlasField out, in, x;    // x used when xpay / CLOV_X
  const void *gauge;       // [mu][par][nch][Vcb][2]
  const void *clover;      // packed [par][nch][Vcb][W] (A or A^-1 slice)
  LatDesc lat;
  int parity;
  bool dagger;
  int mode;   // CloverMode (csrc/dslash_wilson.h)
  bool xpay;
  double a;
  double b_re, b_im;  // twist scalar for TWIST_*/CLOVTW_* modes
  int recon;  // 18 or 12
  GhostDesc halo;
  int kt;  // 0 local, 1 fused, 2 interior, 3 exterior (csrc/dslash_wilson.h)
  // fused epilogues (kt 0/1 only, never both at once; null = off):
  //   out2       : CLOV_POST, !dagger: out2 = A_clov * (out as stored)
  //   y + result : dagger PLAIN xpay: Re <y, out as stored> is added into
  //                dot_result, workgroup b into word (b % dot_slots) * dot_stride
  BlasField out2, y;
  double *dot_result;
  int dot_slots, dot_stride;
};

// true where the fused-epilogue request in c has a compiled kernel
inline bool qa_dslash_epilogue_ok(const DslashCall &c) {
  if (!c.out2.data && !c.y.data) return true;
  if (c.kt != 0 && c.kt != 1) return false;
  if (qa_dslash_waves() != 0) return false;  // default occupancy form only
  if (c.y.data && (c.dot_slots < 1 || c.dot_stride < 1)) return false;
  if (c.out2.data && c.y.data) return false;
  if (c.out2.data) return c.mode == 1 && !c.dagger;
  if (c.y.data) return c.mode == 0 && c.dagger && c.xpay && c.dot_result;
  return true;
}

void launch_dslash_wilson_double(const DslashCall &c, hipStream_t st);
void launch_dslash_wilson_single(const DslashCall &c, hipStream_t st);
void launch_dslash_wilson_half(const DslashCall &c, hipStream_t st);
void launch_dslash_wilson_quarter(const DslashCall &c, hipStream_t st);

// ---------------------------------------------------------------------------
// multi-RHS Wilson(-clover): NRHS in {2,4} sides share each gauge/clover
// load (csrc/dslash_wilson_mrhs.h). mode PLAIN or CLOV_POST only.
#define QA_MRHS_MAX 4
struct DslashMrhsCall {
  int nrhs;
  BlasField out[QA_MRHS_MAX], in[QA_MRHS_MAX], x[QA_MRHS_MAX];
  const void *gauge;
  const void *clover;
  LatDesc lat;
  int parity;
  bool dagger;
  int mode;
  bool xpay;
  double a;
  int recon;
  GhostDesc halo;  // slice-0 base per face; the kernel offsets by rhs
  int kt;  // 0 local, 1 fused, 2 interior (exterior runs per-RHS)
  int prec;
};
void launch_dslash_wilson_mrhs(const DslashMrhsCall &c, hipStream_t st);

// pack one (mu, s01, edge) face of `in` into dst (see csrc/halo.h)
struct PackCall {
  BlasField in;       // dslash input spinor (single parity view)
  void *dst;
  float *dst_nrm;     // half only
  LatDesc lat;
  int parity;         // parity of `in`
  int mu;
  int s01;            // projector sign index (dir XOR dagger)
  int edge;           // 0: x_mu = 0 face, 1: x_mu = X-1 face
  long Fcb;
  int prec;
  int depth = 1;      // ghost layers (staggered Naik = 3)
};
void launch_pack_face_double(const PackCall &c, hipStream_t st);
void launch_pack_face_single(const PackCall &c, hipStream_t st);
void launch_pack_face_half(const PackCall &c, hipStream_t st);
void launch_pack_face_quarter(const PackCall &c, hipStream_t st);

struct CloverApplyCall {
  BlasField out, in;
  const void *clover;  // full [2][nch][Vcb][W]
  int parity;          // which parity slot of the clover field
  long Vcb;
  long sites;          // = Vcb (single parity)
  int prec;
};
void launch_clover_apply(const CloverApplyCall &c, hipStream_t st);

struct TwistApplyCall {
  BlasField out, in;
  double b_re, b_im;
  long sites;
  long tau3_vcb;  // >0: flavor-doublet g5*tau3 mode (flavor = site/tau3_vcb)
  bool acc;       // accumulate into out instead of overwrite
  int prec;
};
void launch_twist_apply(const TwistApplyCall &c, hipStream_t st);

// ---------------------------------------------------------------------------
struct StagDslashCall {
  BlasField out, in, x;  // single-parity views
  const void *gauge;     // stencil layout, like DslashCall
  const void *long_gauge;  // Naik links (stencil layout, shift=3, recon 18); null = naive
  LatDesc lat;
  int parity;
  bool xpay;
  double a, b;  // out = [a*x +] b*(D in); dagger folds into b
  int recon;
  GhostDesc halo;
  int kt;  // 0 local, 1 fused, 2 interior, 3 exterior
  int prec;
  int ghost_depth;  // 1, or 3 when long links cross rank boundaries
};
void launch_dslash_staggered(const StagDslashCall &c, hipStream_t st);
void launch_pack_face_stag(const PackCall &c, hipStream_t st);

// ---------------------------------------------------------------------------
struct Dwf5Call {
  BlasField out, in, x;  // 5-d single-parity fields (Vcb = chunk stride Ls*Vcb4)
  long Vcb4;
  int Ls;
  bool xpay;
  bool dagger;
  double a, alpha, beta, mf;
  int prec;
  int kind;  // 0 = dslash5 (Ds apply), 1 = m5inv
};
void launch_dwf5(const Dwf5Call &c, hipStream_t st);

// ---------------------------------------------------------------------------
// fused domain-wall kernel (csrc/dslash_dwf_fused.h): for all Ls slices,
//   out = [x +] a * W_chi (Dhat in),  W_chi = dense real Ls x Ls per chirality
#define QA_DWF_FUSED_LS_MAX 16
struct DwfFusedCall {
  BlasField out, in, x;  // 5-d single-parity fields (Vcb = chunk stride Ls*Vcb4)
  const void *gauge;     // stencil layout, like DslashCall
  LatDesc lat;           // Vcb = 4-d cb volume
  int Ls;                // 1..QA_DWF_FUSED_LS_MAX
  int parity;
  bool dagger;
  bool xpay;
  double a;
  int recon;             // 18, or 12 for single/half
  int prec;              // 0 double, 1 single, 2 half
  const double *W;       // HOST [2][Ls][Ls] (upper, lower); null = identity
};
// sites per workgroup for single/half: 16 or 32 (set_dwf_fused_ns binding;
// env QUDA_AMD_DWF_FUSED_NS seeds the default, see profiles/r03_dwf_fused.md)
inline int &qa_dwf_fused_ns_ref() {
  static int ns = [] {
    const char *e = getenv("QUDA_AMD_DWF_FUSED_NS");
    int v = e ? atoi(e) : 16;
    return (v == 16 || v == 32) ? v : 16;
  }();
  return ns;
}
inline int qa_dwf_fused_ns() { return qa_dwf_fused_ns_ref(); }
// false when (prec, recon, Ls) has no instantiation or W staging failed
bool launch_dwf_fused(const DwfFusedCall &c, hipStream_t st);

// ---------------------------------------------------------------------------
// coarse-grid dslash on MFMA (csrc/coarse.hip)
struct CoarseMfmaCall {
  const void *mats;  // [9][Na][Nc][Nc] complex64
  const void *nbr9;  // [Na][9] int64 source sites (>=Na -> ghost rows)
  const void *c;     // [Na + n_ghost][Nc][NR] complex64
  void *out;         // [Na][Nc][NR] complex64
  long Na;
  int Nc;            // multiple of 16
  int NR;            // <= 16
};
void launch_coarse_dslash_mfma(const CoarseMfmaCall &c, hipStream_t st);

// ---------------------------------------------------------------------------
// native heatbath / overrelaxation sweep (csrc/heatbath.hip)
struct HeatbathCall {
  void *u;  // [4][2][Vcb][3][3] complex double (oracle layout)
  LatDesc lat;
  int parity;
  int mu;
  double beta_eff;
  unsigned long long seed;
  int mode;  // 0 heatbath, 1 overrelax
};
void launch_heatbath(const HeatbathCall &c, hipStream_t st);

struct StoutCall {
  void *out;       // [4][2][Vcb][3][3] complex double
  const void *in;
  const void *aux;  // expmul: the combined Z tensor
  LatDesc lat;
  int mu;
  double rho;      // zmat: the eps scale
};
void launch_stout(const StoutCall &c, hipStream_t st);
void launch_zmat(const StoutCall &c, hipStream_t st);    // Z = eps TA[S U^d]
void launch_expmul(const StoutCall &c, hipStream_t st);  // U' = exp(Zc) U

// path-table force / path product and loop traces (csrc/gauge_path.hip).
// A path is QA_PATH_STEPS int8 steps +-(nu+1), zero padded and 8-byte
// aligned; tails hold at most 7 steps, closed loops 8.
#define QA_PATH_STEPS 8
#define QA_PATH_MAX 64
struct GaugePathCall {
  void *out;            // [4][2][Vcb][3][3] complex double; only mu written
  const void *u;        // same shape, never aliases out
  const void *steps;    // [4][np][QA_PATH_STEPS] int8
  const int *lens;      // [4][np]
  const double *coefs;  // [4][np]
  int np;               // tails per direction, <= QA_PATH_MAX
  LatDesc lat;
  int mu;
  double scale;         // force: -beta/6
  double dt;            // accumulate: out += dt * result
  bool ta;              // project traceless-antihermitian (force)
  bool accumulate;      // read-modify-write out (fused momentum update)
};
void launch_gauge_path(const GaugePathCall &c, hipStream_t st);

struct LoopTraceCall {
  void *tr;           // [nloops][2][Vcb] complex double
  const void *u;
  const void *steps;  // [nloops][QA_PATH_STEPS] int8
  const int *lens;    // [nloops]
  int nloops;
  LatDesc lat;
};
void launch_loop_trace(const LoopTraceCall &c, hipStream_t st);

#define QA_ZMAX 32

struct ZCoef {  // host-filled complex coefficient tables (double re/im)
  // zdslash5: out(s)_upper = au[s]*in(s) + wu[s]*in(su[s]); lower likewise
  double au[QA_ZMAX][2], al[QA_ZMAX][2];
  double wu[QA_ZMAX][2], wl[QA_ZMAX][2];
  int su[QA_ZMAX], sl[QA_ZMAX];
  // zm5inv: per chirality a sequence order ord[i] = physical slice of step
  // i and the recursion y[i] = di[i] * (r[i] - e[i] y[i-1]) with di = 1/d;
  // Sherman-Morrison corner weight cw couples step 0 to the LAST step.
  int ord_u[QA_ZMAX], ord_l[QA_ZMAX];
  double diu[QA_ZMAX][2], eu[QA_ZMAX][2], cwu[2];
  double dil[QA_ZMAX][2], el[QA_ZMAX][2], cwl[2];
};

struct ZDwf5Call {
  BlasField out, in, x;
  long Vcb4;
  int Ls;
  bool xpay;
  double a_re, a_im;
  int prec;
  int kind;  // 0 = zdslash5, 1 = zm5inv (double/single only)
  const ZCoef *zc;  // HOST pointer; launcher stages to device
};
void launch_zdwf5(const ZDwf5Call &c, hipStream_t st);

struct EofaVec;  // defined in dslash_dwf.h
struct Eofa5Call {
  BlasField out, in, x;
  long Vcb4;
  int Ls;
  bool xpay;
  bool dagger;
  double a, alpha, beta, mf;
  double u[32], w[32];  // see EofaVec semantics (m5inv: u = B^-1 u, sh/denom)
  double sh;
  int pm;
  int prec;
  int kind;  // 0 = m5_eofa, 1 = m5inv_eofa
};
void launch_eofa5(const Eofa5Call &c, hipStream_t st);

// ---------------------------------------------------------------------------
// multigrid transfer, fine Wilson level (csrc/transfer.hip). Double/single.
struct TransferCall {
  BlasField field;         // full-parity fine field (Vcb = cb volume)
  void *coarse;            // [Na][2][Nv] complex of the field's real type
  const void *Vn;          // [2][6][Nv][2*Vcb] complex, site-fastest (prolong)
  const void *V;           // [Na][B][4][3][Nv] complex (restrict)
  const int *agg_of_site;  // [2*Vcb] aggregate of each fine site (prolong)
  const int *site_tab;     // [Na][B] fine site of each (a, b) (restrict)
  long Na;
  int B;
  int Nv;
  int prec;                // 0 double, 1 single
};
bool qa_transfer_grid_ok(const TransferCall &c);
void launch_transfer_prolong(const TransferCall &c, hipStream_t st);
void launch_transfer_restrict(const TransferCall &c, hipStream_t st);

struct BlockOrthoCall {
  void *V;  // [Na][B][4][3][Nv] complex double, orthonormalized in place
  long Na;
  int B;
  int Nv;
  int passes;
};
void launch_transfer_block_ortho(const BlockOrthoCall &c, hipStream_t st);

// Galerkin coarse-operator build, fine Wilson(-clover) level
// (csrc/galerkin.hip). Complex double throughout; rows ab = a*B + b.
struct GalerkinCall {
  void *X;              // [Na][Nc][Nc], Nc = 2*Nv
  void *Y;              // [8][Na][Nc][Nc]
  void *scratch;        // [9][Na][Nc][Nc] interior part of each term
  const void *V;        // [Na][B][12][Nv]
  const int *nbr;       // [Na*B][8] row of the d-neighbour
  const unsigned char *bnd;  // [Na*B] bit d: site on the d-face of its block
  const void *link;     // [Na*B][8][3][3]
  const void *clov;     // [Na*B][12][12] or null (identity)
  const void *coef;     // [8][4][4] -kappa * P_d
  long Na;
  int B;
  int Nv;
};
bool qa_galerkin_grid_ok(const GalerkinCall &c);
void launch_galerkin_build(const GalerkinCall &c, hipStream_t st);
