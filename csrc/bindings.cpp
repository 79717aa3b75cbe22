// pybind11/torch bindings for the quda_amd HIP kernels (in-tree extension).
#include <torch/extension.h>
#include <c10/hip/HIPStream.h>
#include <hip/hip_runtime.h>

#include "launchers.h"

namespace {

int prec_of(const at::Tensor &t) {
  switch (t.scalar_type()) {
    case at::kDouble: return 0;
    case at::kFloat: return 1;
    case at::kHalf: return 2;
    case at::kFloat8_e4m3fn: return 3;
    default: TORCH_CHECK(false, "unsupported dtype");
  }
}

void *ptr_or_null(const at::Tensor &t) {
  return t.numel() ? t.data_ptr() : nullptr;
}

BlasField field_of(const at::Tensor &data, const at::Tensor &norm, long Vcb) {
  return BlasField{ptr_or_null(data), ptr_or_null(norm), Vcb};
}

int chunk_w_of(const at::Tensor &t) {
  switch (t.scalar_type()) {  // 16B chunks for 24-real sites
    case at::kDouble: return 2;
    case at::kFloat: return 4;
    default: return 8;
  }
}

// field view with a site offset into the chunk-stride dimension
BlasField field_of_off(const at::Tensor &data, const at::Tensor &norm,
                       long v_stride, long s_offset) {
  BlasField f{ptr_or_null(data), ptr_or_null(norm), v_stride};
  if (s_offset && f.data) {
    f.data = (char *)f.data + (long)s_offset * chunk_w_of(data) * data.element_size();
    if (f.norm) f.norm = (float *)f.norm + s_offset;
  }
  return f;
}

hipStream_t stream() {
  return c10::hip::getCurrentHIPStream().stream();
}

void check_launch(const char *what) {
  hipError_t e = hipGetLastError();
  TORCH_CHECK(e == hipSuccess, what, ": ", hipGetErrorString(e));
}

LatDesc lat_of(const std::vector<int64_t> &dims, int64_t parity_offset,
               int64_t Vcb) {
  TORCH_CHECK(dims.size() == 4, "dims must hold the 4 local extents");
  LatDesc l{};
  for (int i = 0; i < 4; ++i) l.Xdim[i] = (int)dims[i];
  l.parity_offset = (int)parity_offset;
  l.Vcb = Vcb;
  return l;
}

// the lists are read only when a dimension is partitioned
GhostDesc ghost_of(const std::vector<at::Tensor> &ghost,
                   const std::vector<at::Tensor> &ghost_nrm,
                   const std::vector<int64_t> &face_cb, int64_t comm_mask) {
  GhostDesc h{};
  h.comm_mask = (int)comm_mask;
  if (comm_mask) {
    TORCH_CHECK(ghost.size() == 8 && ghost_nrm.size() == 8 && face_cb.size() == 4);
    for (int k = 0; k < 8; ++k) {
      h.ghost[k] = ptr_or_null(ghost[k]);
      h.ghost_nrm[k] = (const float *)ptr_or_null(ghost_nrm[k]);
    }
    for (int k = 0; k < 4; ++k) h.face_cb[k] = face_cb[k];
  }
  return h;
}

// the Wilson kernels are split into one TU per precision
auto wilson_launcher(int prec) {
  switch (prec) {
    case 0: return launch_dslash_wilson_double;
    case 1: return launch_dslash_wilson_single;
    case 2: return launch_dslash_wilson_half;
    default: return launch_dslash_wilson_quarter;
  }
}

auto pack_launcher(int prec) {
  switch (prec) {
    case 0: return launch_pack_face_double;
    case 1: return launch_pack_face_single;
    case 2: return launch_pack_face_half;
    default: return launch_pack_face_quarter;
  }
}

}  // namespace

static void dslash_wilson(at::Tensor out, at::Tensor out_n, at::Tensor in,
                          at::Tensor in_n, at::Tensor gauge, at::Tensor clover,
                          at::Tensor x, at::Tensor x_n,
                          std::vector<int64_t> dims, int64_t parity_offset,
                          int64_t Vcb, int64_t parity, bool dagger,
                          int64_t mode, bool xpay, double a, int64_t recon,
                          std::vector<at::Tensor> ghost,
                          std::vector<at::Tensor> ghost_nrm,
                          std::vector<int64_t> face_cb, int64_t comm_mask,
                          int64_t kt, double b_re, double b_im,
                          int64_t v_stride, int64_t s_offset,
                          c10::optional<at::Tensor> out2,
                          c10::optional<at::Tensor> out2_n,
                          c10::optional<at::Tensor> dot_y,
                          c10::optional<at::Tensor> dot_y_n,
                          c10::optional<at::Tensor> dot_result,
                          int64_t dot_slots, int64_t dot_stride) {
  // v_stride: chunk stride of the spinor fields (Ls*Vcb for 5-d fields);
  // s_offset: site offset of the 4-d slice being operated on (s*Vcb)
  // out2 / dot_y + dot_result: fused epilogues (launchers.h DslashCall)
  TORCH_CHECK(out.is_contiguous() && in.is_contiguous() && gauge.is_contiguous());
  if (v_stride == 0) v_stride = Vcb;
  DslashCall c{};
  c.halo = ghost_of(ghost, ghost_nrm, face_cb, comm_mask);
  c.kt = (int)kt;
  c.out = field_of_off(out, out_n, v_stride, s_offset);
  c.in = field_of_off(in, in_n, v_stride, s_offset);
  c.x = field_of_off(x, x_n, v_stride, s_offset);
  c.gauge = gauge.data_ptr();
  c.clover = ptr_or_null(clover);
  c.lat = lat_of(dims, parity_offset, Vcb);
  c.parity = (int)parity;
  c.dagger = dagger;
  c.mode = (int)mode;
  c.xpay = xpay;
  c.a = a;
  c.b_re = b_re;
  c.b_im = b_im;
  c.recon = (int)recon;
  if (out2) {
    TORCH_CHECK(out2_n && out2->is_contiguous() &&
                out2->scalar_type() == out.scalar_type() &&
                out2->numel() == out.numel() &&
                out2->data_ptr() != out.data_ptr() &&
                out2->data_ptr() != in.data_ptr(),
                "dslash_wilson: out2 must be a distinct field shaped like out");
    c.out2 = field_of_off(*out2, *out2_n, v_stride, s_offset);
  }
  if (dot_y) {
    TORCH_CHECK(dot_y_n && dot_result && dot_y->is_contiguous() &&
                dot_y->scalar_type() == out.scalar_type() &&
                dot_y->numel() == out.numel(),
                "dslash_wilson: dot_y must be a field shaped like out");
    TORCH_CHECK(dot_slots >= 1 && dot_stride >= 1 &&
                dot_result->scalar_type() == at::kDouble &&
                dot_result->numel() >= (dot_slots - 1) * dot_stride + 1 &&
                dot_result->is_contiguous() &&
                dot_result->device() == out.device(),
                "dslash_wilson: dot_result must be a float64 tensor on the "
                "fields' device");
    c.y = field_of_off(*dot_y, *dot_y_n, v_stride, s_offset);
    c.dot_result = dot_result->data_ptr<double>();
    c.dot_slots = (int)dot_slots;
    c.dot_stride = (int)dot_stride;
  }
  TORCH_CHECK(qa_dslash_epilogue_ok(c),
              "dslash_wilson: no fused-epilogue kernel for this launch (out2: "
              "CLOV_POST, no dagger; dot: dagger PLAIN xpay; kt 0 or 1; "
              "default occupancy form)");
  wilson_launcher(prec_of(out))(c, stream());
  check_launch("dslash_wilson");
}

static void dslash_wilson_mrhs(
    std::vector<at::Tensor> out, std::vector<at::Tensor> out_n,
    std::vector<at::Tensor> in, std::vector<at::Tensor> in_n,
    at::Tensor gauge, at::Tensor clover, std::vector<at::Tensor> x,
    std::vector<at::Tensor> x_n, std::vector<int64_t> dims,
    int64_t parity_offset, int64_t Vcb, int64_t parity, bool dagger,
    int64_t mode, bool xpay, double a, int64_t recon,
    std::vector<at::Tensor> ghost, std::vector<at::Tensor> ghost_nrm,
    std::vector<int64_t> face_cb, int64_t comm_mask, int64_t kt,
    int64_t v_stride, std::vector<int64_t> s_offsets) {
  // v_stride/s_offsets: address 4-d slices of 5-d fields (domain-wall
  // s-batching — the same tensor appears n times with different offsets)
  int n = (int)out.size();
  TORCH_CHECK(n == 2 || n == 4, "mrhs kernel supports 2 or 4 RHS");
  TORCH_CHECK((int)in.size() == n);
  if (v_stride == 0) v_stride = Vcb;
  DslashMrhsCall c{};
  c.nrhs = n;
  for (int r = 0; r < n; ++r) {
    TORCH_CHECK(out[r].is_contiguous() && in[r].is_contiguous());
    long so = s_offsets.empty() ? 0 : s_offsets[r];
    c.out[r] = field_of_off(out[r], out_n[r], v_stride, so);
    c.in[r] = field_of_off(in[r], in_n[r], v_stride, so);
    if (!x.empty()) c.x[r] = field_of_off(x[r], x_n[r], v_stride, so);
  }
  c.halo = ghost_of(ghost, ghost_nrm, face_cb, comm_mask);
  c.kt = (int)kt;
  c.gauge = gauge.data_ptr();
  c.clover = ptr_or_null(clover);
  c.lat = lat_of(dims, parity_offset, Vcb);
  c.parity = (int)parity;
  c.dagger = dagger;
  c.mode = (int)mode;
  c.xpay = xpay;
  c.a = a;
  c.recon = (int)recon;
  c.prec = prec_of(out[0]);
  launch_dslash_wilson_mrhs(c, stream());
  check_launch("dslash_wilson_mrhs");
}

// shared body of pack_face / pack_face_ptr (dst: tensor or raw peer pointer)
static void pack_face_to(const char *what, void *dst, float *dst_nrm,
                         const at::Tensor &in, const at::Tensor &in_n,
                         const std::vector<int64_t> &dims,
                         int64_t parity_offset, int64_t Vcb, int64_t parity,
                         int64_t mu, int64_t s01, int64_t edge, int64_t Fcb,
                         int64_t v_stride, int64_t s_offset) {
  PackCall c{};
  c.in = field_of_off(in, in_n, v_stride ? v_stride : Vcb, s_offset);
  c.dst = dst;
  c.dst_nrm = dst_nrm;
  c.lat = lat_of(dims, parity_offset, Vcb);
  c.parity = (int)parity;
  c.mu = (int)mu;
  c.s01 = (int)s01;
  c.edge = (int)edge;
  c.Fcb = Fcb;
  c.prec = prec_of(in);
  pack_launcher(c.prec)(c, stream());
  check_launch(what);
}

static void pack_face(at::Tensor dst, at::Tensor dst_nrm, at::Tensor in,
                      at::Tensor in_n, std::vector<int64_t> dims,
                      int64_t parity_offset, int64_t Vcb, int64_t parity,
                      int64_t mu, int64_t s01, int64_t edge, int64_t Fcb,
                      int64_t v_stride = 0, int64_t s_offset = 0) {
  pack_face_to("pack_face", dst.data_ptr(), (float *)ptr_or_null(dst_nrm), in,
               in_n, dims, parity_offset, Vcb, parity, mu, s01, edge, Fcb,
               v_stride, s_offset);
}

static void pack_face_stag(at::Tensor dst, at::Tensor dst_nrm, at::Tensor in,
                           at::Tensor in_n, std::vector<int64_t> dims,
                           int64_t parity_offset, int64_t Vcb, int64_t parity,
                           int64_t mu, int64_t edge, int64_t Fcb,
                           int64_t depth) {
  PackCall c{};
  c.in = field_of(in, in_n, Vcb);
  c.dst = dst.data_ptr();
  c.dst_nrm = (float *)ptr_or_null(dst_nrm);
  c.lat = lat_of(dims, parity_offset, Vcb);
  c.parity = (int)parity;
  c.mu = (int)mu;
  c.edge = (int)edge;
  c.Fcb = Fcb;
  c.prec = prec_of(in);
  c.depth = (int)depth;
  launch_pack_face_stag(c, stream());
  check_launch("pack_face_stag");
}

static void dslash_staggered(at::Tensor out, at::Tensor out_n, at::Tensor in,
                             at::Tensor in_n, at::Tensor gauge,
                             at::Tensor long_gauge, at::Tensor x,
                             at::Tensor x_n, std::vector<int64_t> dims,
                             int64_t parity_offset, int64_t Vcb,
                             int64_t parity, bool xpay, double a, double b,
                             int64_t recon, std::vector<at::Tensor> ghost,
                             std::vector<at::Tensor> ghost_nrm,
                             std::vector<int64_t> face_cb, int64_t comm_mask,
                             int64_t kt, int64_t ghost_depth) {
  TORCH_CHECK(out.is_contiguous() && in.is_contiguous() && gauge.is_contiguous());
  StagDslashCall c{};
  c.out = field_of(out, out_n, Vcb);
  c.in = field_of(in, in_n, Vcb);
  c.x = field_of(x, x_n, Vcb);
  c.gauge = gauge.data_ptr();
  c.long_gauge = ptr_or_null(long_gauge);
  c.lat = lat_of(dims, parity_offset, Vcb);
  c.parity = (int)parity;
  c.xpay = xpay;
  c.a = a;
  c.b = b;
  c.recon = (int)recon;
  c.halo = ghost_of(ghost, ghost_nrm, face_cb, comm_mask);
  c.kt = (int)kt;
  c.prec = prec_of(out);
  c.ghost_depth = (int)ghost_depth;
  launch_dslash_staggered(c, stream());
  check_launch("dslash_staggered");
}

static at::Tensor blas_op(int64_t op, double a, double b, at::Tensor x,
                          at::Tensor x_n, at::Tensor y, at::Tensor y_n,
                          int64_t Vcb, int64_t sites, double c2 = 0.0,
                          double d2 = 0.0, int64_t ncomp = 24,
                          bool deterministic = false,
                          c10::optional<at::Tensor> z = c10::nullopt,
                          c10::optional<at::Tensor> z_n = c10::nullopt,
                          c10::optional<at::Tensor> w = c10::nullopt,
                          c10::optional<at::Tensor> w_n = c10::nullopt) {
  TORCH_CHECK(op != BLAS_TRIPLE_CG_DEV,
              "blas_op: BLAS_TRIPLE_CG_DEV takes a device accumulator — call "
              "triple_cg_dev");
  BlasCall c{};
  c.op = (int)op;
  c.prec = prec_of(x);
  c.a = a;
  c.b = b;
  c.c = c2;
  c.d = d2;
  c.ncomp = (int)ncomp;
  c.det = deterministic;
  c.x = field_of(x, x_n, Vcb);
  c.y = field_of(y, y_n, Vcb);
  if (z) c.z = field_of(*z, *z_n, Vcb);
  if (w) c.w = field_of(*w, *w_n, Vcb);
  c.sites = sites;
  at::Tensor result;
  bool reduction = (op == BLAS_AXPY_NORM2 || op == BLAS_XMY_NORM2 ||
                    op == BLAS_NORM2 || op == BLAS_REDOT || op == BLAS_CDOT ||
                    op == BLAS_TRIPLE_CG);
  if (reduction) {
    if (deterministic) {
      long g = (sites + 255) / 256;
      if (g > 2048) g = 2048;
      result = at::zeros({g, 2}, x.options().dtype(at::kDouble));
    } else {
      result = at::zeros({2}, x.options().dtype(at::kDouble));
    }
    c.result = result.data_ptr<double>();
  }
  launch_blas(c, stream());
  check_launch("blas_op");
  if (reduction && deterministic) result = result.sum(0);
  return result;
}

// x += alpha p; r -= alpha Ap with alpha = r2_old / pAp formed on the
// device; ||r||^2 accumulated into acc[1]; `clear` zeroed whole (see
// k_triple_cg_dev). pAp = acc[0], or with `slots` non-empty the sum of
// slots[s * slot_stride], s < nslots. All float64 on the fields' device.
static void triple_cg_dev(double r2_old, at::Tensor acc, at::Tensor clear,
                          at::Tensor p, at::Tensor p_n, at::Tensor Ap,
                          at::Tensor Ap_n, at::Tensor x, at::Tensor x_n,
                          at::Tensor r, at::Tensor r_n, int64_t Vcb,
                          int64_t sites, int64_t ncomp, at::Tensor slots,
                          int64_t nslots, int64_t slot_stride) {
  auto ok = [&](const at::Tensor &t) {
    return t.scalar_type() == at::kDouble && t.is_contiguous() &&
           t.device() == p.device();
  };
  TORCH_CHECK(ok(acc) && acc.numel() >= 2,
              "triple_cg_dev: acc must hold 2 float64 on the fields' device");
  TORCH_CHECK(clear.numel() == 0 || ok(clear),
              "triple_cg_dev: clear must be empty or float64 on the device");
  if (clear.numel()) {
    auto lo = (const char *)clear.data_ptr(), hi = lo + clear.numel() * 8;
    auto a0 = (const char *)acc.data_ptr();
    TORCH_CHECK(a0 + 16 <= lo || a0 >= hi,
                "triple_cg_dev: clear must not overlap acc");
  }
  TORCH_CHECK(nslots == 0 ||
              (ok(slots) && nslots >= 1 && nslots <= 64 && slot_stride >= 1 &&
               slots.numel() >= (nslots - 1) * slot_stride + 1),
              "triple_cg_dev: slots must hold nslots <= 64 strided float64");
  BlasCall c{};
  c.op = BLAS_TRIPLE_CG_DEV;
  c.prec = prec_of(p);
  c.a = r2_old;
  c.ncomp = (int)ncomp;
  c.x = field_of(p, p_n, Vcb);
  c.y = field_of(Ap, Ap_n, Vcb);
  c.z = field_of(x, x_n, Vcb);
  c.w = field_of(r, r_n, Vcb);
  c.sites = sites;
  c.result = acc.data_ptr<double>();
  c.clear = clear.numel() ? clear.data_ptr<double>() : nullptr;
  c.clear_n = clear.numel();
  c.nslots = (int)nslots;
  c.slot_stride = (int)slot_stride;
  c.slots = nslots ? slots.data_ptr<double>() : nullptr;
  launch_blas(c, stream());
  check_launch("triple_cg_dev");
}

static void convert(at::Tensor dst, at::Tensor dst_n, at::Tensor src,
                    at::Tensor src_n, int64_t Vcb, int64_t sites,
                    int64_t ncomp = 24) {
  launch_convert(field_of(dst, dst_n, Vcb), prec_of(dst),
                 field_of(src, src_n, Vcb), prec_of(src), sites, (int)ncomp,
                 stream());
  check_launch("convert");
}

static void clover_apply(at::Tensor out, at::Tensor out_n, at::Tensor in,
                         at::Tensor in_n, at::Tensor clover, int64_t parity,
                         int64_t Vcb, int64_t v_stride, int64_t s_offset) {
  CloverApplyCall c{};
  c.out = field_of_off(out, out_n, v_stride ? v_stride : Vcb, s_offset);
  c.in = field_of_off(in, in_n, v_stride ? v_stride : Vcb, s_offset);
  c.clover = clover.data_ptr();
  c.parity = (int)parity;
  c.Vcb = Vcb;
  c.sites = Vcb;
  c.prec = prec_of(out);
  launch_clover_apply(c, stream());
  check_launch("clover_apply");
}

static void twist_apply(at::Tensor out, at::Tensor out_n, at::Tensor in,
                        at::Tensor in_n, double b_re, double b_im,
                        int64_t Vcb, int64_t sites, int64_t tau3_vcb = 0,
                        bool acc = false) {
  TwistApplyCall c{};
  c.out = field_of(out, out_n, Vcb);
  c.in = field_of(in, in_n, Vcb);
  c.b_re = b_re;
  c.b_im = b_im;
  c.sites = sites;
  c.tau3_vcb = tau3_vcb;
  c.acc = acc;
  c.prec = prec_of(out);
  launch_twist_apply(c, stream());
  check_launch("twist_apply");
}

static void dwf5(at::Tensor out, at::Tensor out_n, at::Tensor in,
                 at::Tensor in_n, at::Tensor x, at::Tensor x_n,
                 int64_t Vcb4, int64_t Ls, bool xpay, bool dagger, double a,
                 double alpha, double beta, double mf, int64_t kind) {
  Dwf5Call c{};
  long stride = Vcb4 * Ls;
  c.out = field_of(out, out_n, stride);
  c.in = field_of(in, in_n, stride);
  c.x = field_of(x, x_n, stride);
  c.Vcb4 = Vcb4;
  c.Ls = (int)Ls;
  c.xpay = xpay;
  c.dagger = dagger;
  c.a = a;
  c.alpha = alpha;
  c.beta = beta;
  c.mf = mf;
  c.prec = prec_of(out);
  c.kind = (int)kind;
  launch_dwf5(c, stream());
  check_launch("dwf5");
}

// Fused domain-wall kernel (csrc/dslash_dwf_fused.h). Every argument is
// validated here: a bad call raises and nothing is launched.
static void dwf_fused(at::Tensor out, at::Tensor out_n, at::Tensor in,
                      at::Tensor in_n, at::Tensor gauge, at::Tensor x,
                      at::Tensor x_n, c10::optional<at::Tensor> W,
                      std::vector<int64_t> dims, int64_t parity_offset,
                      int64_t Vcb, int64_t Ls, int64_t parity, bool dagger,
                      bool xpay, double a, int64_t recon) {
  TORCH_CHECK(Ls >= 1 && Ls <= QA_DWF_FUSED_LS_MAX, "dwf_fused: Ls = ", Ls,
              " outside 1..", QA_DWF_FUSED_LS_MAX);
  TORCH_CHECK(dims.size() == 4 && Vcb > 0, "dwf_fused: bad lattice");
  TORCH_CHECK(dims[0] > 0 && dims[0] % 2 == 0 && dims[1] > 0 && dims[2] > 0 &&
                  dims[3] > 0 &&
                  dims[0] * dims[1] * dims[2] * dims[3] == 2 * Vcb,
              "dwf_fused: dims do not match Vcb");
  TORCH_CHECK(parity == 0 || parity == 1, "dwf_fused: parity must be 0 or 1");
  TORCH_CHECK(out.is_cuda(), "dwf_fused: fields must live on the GPU");
  const int prec = prec_of(out);
  TORCH_CHECK(prec <= 2, "dwf_fused: double, single or half only");
  TORCH_CHECK(recon == 18 || (recon == 12 && prec != 0),
              "dwf_fused: reconstruct ", recon, " unsupported at this precision");
  const int64_t stride = Ls * Vcb;
  auto check_field = [&](const at::Tensor &t, const at::Tensor &n,
                         const char *name) {
    TORCH_CHECK(t.is_cuda() && t.device() == out.device(), "dwf_fused: ", name,
                " on a different device");
    TORCH_CHECK(t.scalar_type() == out.scalar_type(), "dwf_fused: ", name,
                " dtype differs from out");
    TORCH_CHECK(t.is_contiguous(), "dwf_fused: ", name, " not contiguous");
    TORCH_CHECK(t.dim() == 4 && t.size(0) == 1 && t.size(2) == stride &&
                    t.size(3) == chunk_w_of(t) &&
                    t.size(1) * t.size(3) == 24,
                "dwf_fused: ", name, " is not a single-parity field with "
                "chunk stride Ls*Vcb");
    if (prec == 2) {
      TORCH_CHECK(n.is_cuda() && n.device() == out.device() &&
                      n.scalar_type() == at::kFloat && n.is_contiguous() &&
                      n.numel() == stride,
                  "dwf_fused: ", name, " norm is not float32 [Ls*Vcb]");
    }
  };
  check_field(out, out_n, "out");
  check_field(in, in_n, "in");
  if (xpay) check_field(x, x_n, "x");
  TORCH_CHECK(gauge.is_cuda() && gauge.device() == out.device() &&
                  gauge.scalar_type() == out.scalar_type() &&
                  gauge.is_contiguous() &&
                  gauge.numel() == 2 * 8 * recon * Vcb,
              "dwf_fused: gauge is not a stencil-layout field of this "
              "precision/reconstruct");
  {
    // the stencil reads neighbors of `in` while other workgroups store
    // `out`: their memory must not overlap (out may alias x)
    const char *o0 = (const char *)out.data_ptr(), *o1 = o0 + out.nbytes();
    const char *i0 = (const char *)in.data_ptr(), *i1 = i0 + in.nbytes();
    TORCH_CHECK(o1 <= i0 || i1 <= o0, "dwf_fused: out aliases in");
  }
  const double *Wp = nullptr;
  at::Tensor Wc;
  if (W) {
    TORCH_CHECK(W->device().is_cpu() && W->scalar_type() == at::kDouble,
                "dwf_fused: W must be a float64 host tensor");
    TORCH_CHECK(W->dim() == 3 && W->size(0) == 2 && W->size(1) == Ls &&
                    W->size(2) == Ls,
                "dwf_fused: W must have shape [2, Ls, Ls]");
    Wc = W->contiguous();
    Wp = Wc.data_ptr<double>();
  }
  DwfFusedCall c{};
  c.out = field_of(out, out_n, stride);
  c.in = field_of(in, in_n, stride);
  c.x = xpay ? field_of(x, x_n, stride) : c.out;
  c.gauge = gauge.data_ptr();
  c.lat = lat_of(dims, parity_offset, Vcb);
  c.Ls = (int)Ls;
  c.parity = (int)parity;
  c.dagger = dagger;
  c.xpay = xpay;
  c.a = a;
  c.recon = (int)recon;
  c.prec = prec;
  c.W = Wp;
  TORCH_CHECK(launch_dwf_fused(c, stream()),
              "dwf_fused: no kernel for this configuration");
  check_launch("dwf_fused");
}

static void zdwf5(at::Tensor out, at::Tensor out_n, at::Tensor in,
                  at::Tensor in_n, at::Tensor x, at::Tensor x_n,
                  int64_t Vcb4, int64_t Ls, bool xpay, double a_re,
                  double a_im, int64_t kind,
                  std::vector<double> au, std::vector<double> al,
                  std::vector<double> wu, std::vector<double> wl,
                  std::vector<int64_t> su, std::vector<int64_t> sl,
                  std::vector<int64_t> ord_u, std::vector<int64_t> ord_l,
                  std::vector<double> diu, std::vector<double> eu,
                  std::vector<double> dil, std::vector<double> el,
                  double cwu_re, double cwu_im, double cwl_re, double cwl_im) {
  TORCH_CHECK(Ls <= QA_ZMAX, "zMobius Ls > ", QA_ZMAX);
  ZCoef zc{};
  auto put2 = [&](double dst[][2], const std::vector<double> &v) {
    for (int s = 0; s < (int)Ls && 2 * s + 1 < (int)v.size(); ++s) {
      dst[s][0] = v[2 * s];
      dst[s][1] = v[2 * s + 1];
    }
  };
  put2(zc.au, au); put2(zc.al, al); put2(zc.wu, wu); put2(zc.wl, wl);
  put2(zc.diu, diu); put2(zc.eu, eu); put2(zc.dil, dil); put2(zc.el, el);
  for (int s = 0; s < (int)Ls; ++s) {
    if (s < (int)su.size()) zc.su[s] = (int)su[s];
    if (s < (int)sl.size()) zc.sl[s] = (int)sl[s];
    if (s < (int)ord_u.size()) zc.ord_u[s] = (int)ord_u[s];
    if (s < (int)ord_l.size()) zc.ord_l[s] = (int)ord_l[s];
  }
  zc.cwu[0] = cwu_re; zc.cwu[1] = cwu_im;
  zc.cwl[0] = cwl_re; zc.cwl[1] = cwl_im;
  ZDwf5Call c{};
  long stride = Vcb4 * Ls;
  c.out = field_of(out, out_n, stride);
  c.in = field_of(in, in_n, stride);
  c.x = field_of(x, x_n, stride);
  c.Vcb4 = Vcb4;
  c.Ls = (int)Ls;
  c.xpay = xpay;
  c.a_re = a_re;
  c.a_im = a_im;
  c.prec = prec_of(out);
  c.kind = (int)kind;
  TORCH_CHECK(c.prec != 2, "zdwf5: half precision unsupported");
  c.zc = &zc;
  launch_zdwf5(c, stream());
  check_launch("zdwf5");
}

static void eofa5(at::Tensor out, at::Tensor out_n, at::Tensor in,
                  at::Tensor in_n, at::Tensor x, at::Tensor x_n,
                  int64_t Vcb4, int64_t Ls, bool xpay, bool dagger, double a,
                  double alpha, double beta, double mf,
                  std::vector<double> u, std::vector<double> w, double sh,
                  int64_t pm, int64_t kind) {
  TORCH_CHECK(Ls <= 32, "eofa5: Ls > 32");
  Eofa5Call c{};
  long stride = Vcb4 * Ls;
  c.out = field_of(out, out_n, stride);
  c.in = field_of(in, in_n, stride);
  c.x = field_of(x, x_n, stride);
  c.Vcb4 = Vcb4;
  c.Ls = (int)Ls;
  c.xpay = xpay;
  c.dagger = dagger;
  c.a = a;
  c.alpha = alpha;
  c.beta = beta;
  c.mf = mf;
  for (int s = 0; s < (int)Ls; ++s) {
    if (s < (int)u.size()) c.u[s] = u[s];
    if (s < (int)w.size()) c.w[s] = w[s];
  }
  c.sh = sh;
  c.pm = (int)pm;
  c.prec = prec_of(out);
  c.kind = (int)kind;
  launch_eofa5(c, stream());
  check_launch("eofa5");
}

static void set_dslash_block(int64_t b) {
  if (b == 64 || b == 128 || b == 256) qa_dslash_block_ref() = (int)b;
}

static void set_dslash_waves(int64_t w) {
  if (w == 0 || w == 3) qa_dslash_waves_ref() = (int)w;
}

static void set_dslash_lds(int64_t v) { qa_dslash_lds_ref() = (int)v; }
static int64_t get_dslash_block() { return qa_dslash_block(); }
static int64_t get_dslash_lds() { return qa_dslash_lds(); }
static int64_t get_dslash_waves() { return qa_dslash_waves(); }

static void set_dwf_fused_ns(int64_t v) {
  if (v == 16 || v == 32) qa_dwf_fused_ns_ref() = (int)v;
}

// ---------------------------------------------------------------------------
// HIP-IPC remote-write halos (role of comm_target.cpp:41-134 P2P
// remote-write): export/import device-buffer handles so the pack kernel
// writes directly into the PEER rank's recv buffer over xGMI.
static py::bytes ipc_get_handle(at::Tensor t) {
  // torch's caching allocator suballocates: the IPC handle refers to the
  // BASE allocation, so export (handle, offset-of-tensor-within-it)
  TORCH_CHECK(t.is_cuda() && t.is_contiguous());
  void *base = nullptr;
  size_t sz = 0;
  hipError_t e = hipMemGetAddressRange((hipDeviceptr_t *)&base, &sz,
                                       (hipDeviceptr_t)t.data_ptr());
  TORCH_CHECK(e == hipSuccess, "hipMemGetAddressRange: ",
              hipGetErrorString(e));
  hipIpcMemHandle_t h;
  e = hipIpcGetMemHandle(&h, base);
  TORCH_CHECK(e == hipSuccess, "hipIpcGetMemHandle: ", hipGetErrorString(e));
  uint64_t off = (uint64_t)((char *)t.data_ptr() - (char *)base);
  std::string out(sizeof(h) + sizeof(off), '\0');
  memcpy(&out[0], &h, sizeof(h));
  memcpy(&out[sizeof(h)], &off, sizeof(off));
  return py::bytes(out);
}

static py::tuple ipc_open_handle(py::bytes handle) {
  // returns (tensor_ptr, mapped_base) — close with the BASE
  std::string s = handle;
  TORCH_CHECK(s.size() == sizeof(hipIpcMemHandle_t) + sizeof(uint64_t));
  hipIpcMemHandle_t h;
  uint64_t off;
  memcpy(&h, s.data(), sizeof(h));
  memcpy(&off, s.data() + sizeof(h), sizeof(off));
  void *ptr = nullptr;
  hipError_t e =
      hipIpcOpenMemHandle(&ptr, h, hipIpcMemLazyEnablePeerAccess);
  TORCH_CHECK(e == hipSuccess, "hipIpcOpenMemHandle: ", hipGetErrorString(e));
  return py::make_tuple((int64_t)((uintptr_t)ptr + off),
                        (int64_t)(uintptr_t)ptr);
}

static void ipc_close_handle(int64_t ptr) {
  hipIpcCloseMemHandle((void *)(uintptr_t)ptr);
}

// pack a face directly into a raw (peer) destination pointer
static void pack_face_ptr(int64_t dst, int64_t dst_nrm, at::Tensor in,
                          at::Tensor in_n, std::vector<int64_t> dims,
                          int64_t parity_offset, int64_t Vcb, int64_t parity,
                          int64_t mu, int64_t s01, int64_t edge, int64_t Fcb,
                          int64_t v_stride, int64_t s_offset) {
  pack_face_to("pack_face_ptr", (void *)(uintptr_t)dst,
               (float *)(uintptr_t)dst_nrm, in, in_n, dims, parity_offset, Vcb,
               parity, mu, s01, edge, Fcb, v_stride, s_offset);
}

static void heatbath_sweep_dir(at::Tensor u, std::vector<int64_t> dims,
                               int64_t parity_offset, int64_t Vcb,
                               int64_t parity, int64_t mu, double beta_eff,
                               int64_t seed, int64_t mode) {
  TORCH_CHECK(u.is_contiguous() && u.scalar_type() == at::kComplexDouble);
  HeatbathCall c{};
  c.u = u.data_ptr();
  c.lat = lat_of(dims, parity_offset, Vcb);
  c.parity = (int)parity;
  c.mu = (int)mu;
  c.beta_eff = beta_eff;
  c.seed = (unsigned long long)seed;
  c.mode = (int)mode;
  launch_heatbath(c, stream());
  check_launch("heatbath");
}

static void stout_smear_dir(at::Tensor out, at::Tensor in,
                            std::vector<int64_t> dims,
                            int64_t parity_offset, int64_t Vcb, int64_t mu,
                            double rho) {
  TORCH_CHECK(out.is_contiguous() && in.is_contiguous() &&
              in.scalar_type() == at::kComplexDouble);
  StoutCall c{};
  c.out = out.data_ptr();
  c.in = in.data_ptr();
  c.lat = lat_of(dims, parity_offset, Vcb);
  c.mu = (int)mu;
  c.rho = rho;
  launch_stout(c, stream());
  check_launch("stout");
}

static void flow_zmat_dir(at::Tensor Z, at::Tensor in,
                          std::vector<int64_t> dims, int64_t parity_offset,
                          int64_t Vcb, int64_t mu, double eps) {
  TORCH_CHECK(Z.is_contiguous() && in.is_contiguous());
  StoutCall c{};
  c.out = Z.data_ptr();
  c.in = in.data_ptr();
  c.lat = lat_of(dims, parity_offset, Vcb);
  c.mu = (int)mu;
  c.rho = eps;
  launch_zmat(c, stream());
  check_launch("zmat");
}

static void flow_expmul_dir(at::Tensor out, at::Tensor in, at::Tensor Zc,
                            std::vector<int64_t> dims,
                            int64_t parity_offset, int64_t Vcb, int64_t mu) {
  TORCH_CHECK(out.is_contiguous() && in.is_contiguous() &&
              Zc.is_contiguous());
  StoutCall c{};
  c.out = out.data_ptr();
  c.in = in.data_ptr();
  c.aux = Zc.data_ptr();
  c.lat = lat_of(dims, parity_offset, Vcb);
  c.mu = (int)mu;
  launch_expmul(c, stream());
  check_launch("expmul");
}

// shape checks shared by the two path-table entries: a periodic single-rank
// lattice of even extents whose volume matches the gauge tensor
static void check_path_lattice(const char *what, const at::Tensor &u,
                               const std::vector<int64_t> &dims, int64_t Vcb) {
  TORCH_CHECK(u.is_cuda() && u.is_contiguous() &&
                  u.scalar_type() == at::kComplexDouble,
              what, ": u must be a contiguous complex128 GPU tensor");
  TORCH_CHECK(dims.size() == 4, what, ": dims must hold the 4 extents");
  int64_t vol = 1;
  for (int k = 0; k < 4; ++k) {
    TORCH_CHECK(dims[k] >= 2 && dims[k] % 2 == 0, what,
                ": extents must be even and >= 2");
    vol *= dims[k];
  }
  TORCH_CHECK(Vcb > 0 && vol == 2 * Vcb && vol < (1LL << 31), what,
              ": Vcb does not match dims");
  TORCH_CHECK(u.numel() == 4 * 2 * Vcb * 9, what, ": u is not [4,2,Vcb,3,3]");
}

static void gauge_path_dir(at::Tensor out, at::Tensor u, at::Tensor steps,
                           at::Tensor lens, at::Tensor coefs,
                           std::vector<int64_t> dims, int64_t parity_offset,
                           int64_t Vcb, int64_t mu, double scale, double dt,
                           bool ta, bool accumulate) {
  const char *what = "gauge_path_dir";
  check_path_lattice(what, u, dims, Vcb);
  TORCH_CHECK(out.is_cuda() && out.is_contiguous() &&
                  out.scalar_type() == at::kComplexDouble &&
                  out.numel() == u.numel() && out.device() == u.device() &&
                  out.data_ptr() != u.data_ptr(),
              what, ": out must be a separate tensor shaped like u");
  TORCH_CHECK(steps.is_contiguous() && steps.scalar_type() == at::kChar &&
                  steps.dim() == 3 && steps.size(0) == 4 &&
                  steps.size(2) == QA_PATH_STEPS &&
                  (uintptr_t)steps.data_ptr() % 8 == 0 &&
                  steps.device() == u.device(),
              what, ": steps must be int8 [4][np][8] on u's device");
  const int64_t np = steps.size(1);
  TORCH_CHECK(np >= 1 && np <= QA_PATH_MAX, what, ": np out of range");
  TORCH_CHECK(lens.is_contiguous() && lens.scalar_type() == at::kInt &&
                  lens.numel() == 4 * np && lens.device() == u.device(),
              what, ": lens must be int32 [4][np]");
  TORCH_CHECK(coefs.is_contiguous() && coefs.scalar_type() == at::kDouble &&
                  coefs.numel() == 4 * np && coefs.device() == u.device(),
              what, ": coefs must be float64 [4][np]");
  TORCH_CHECK(mu >= 0 && mu < 4, what, ": mu out of range");
  GaugePathCall c{};
  c.out = out.data_ptr();
  c.u = u.data_ptr();
  c.steps = steps.data_ptr();
  c.lens = lens.data_ptr<int>();
  c.coefs = coefs.data_ptr<double>();
  c.np = (int)np;
  c.lat = lat_of(dims, parity_offset, Vcb);
  c.mu = (int)mu;
  c.scale = scale;
  c.dt = dt;
  c.ta = ta;
  c.accumulate = accumulate;
  launch_gauge_path(c, stream());
  check_launch(what);
}

static void gauge_loop_trace(at::Tensor tr, at::Tensor u, at::Tensor steps,
                             at::Tensor lens, std::vector<int64_t> dims,
                             int64_t parity_offset, int64_t Vcb) {
  const char *what = "gauge_loop_trace";
  check_path_lattice(what, u, dims, Vcb);
  TORCH_CHECK(steps.is_contiguous() && steps.scalar_type() == at::kChar &&
                  steps.dim() == 2 && steps.size(1) == QA_PATH_STEPS &&
                  (uintptr_t)steps.data_ptr() % 8 == 0 &&
                  steps.device() == u.device(),
              what, ": steps must be int8 [nloops][8] on u's device");
  const int64_t nl = steps.size(0);
  TORCH_CHECK(nl >= 1 && nl < (1 << 20), what, ": nloops out of range");
  TORCH_CHECK(lens.is_contiguous() && lens.scalar_type() == at::kInt &&
                  lens.numel() == nl && lens.device() == u.device(),
              what, ": lens must be int32 [nloops]");
  TORCH_CHECK(tr.is_cuda() && tr.is_contiguous() &&
                  tr.scalar_type() == at::kComplexDouble &&
                  tr.numel() == nl * 2 * Vcb && tr.device() == u.device(),
              what, ": tr must be complex128 [nloops][2][Vcb]");
  LoopTraceCall c{};
  c.tr = tr.data_ptr();
  c.u = u.data_ptr();
  c.steps = steps.data_ptr();
  c.lens = lens.data_ptr<int>();
  c.nloops = (int)nl;
  c.lat = lat_of(dims, parity_offset, Vcb);
  launch_loop_trace(c, stream());
  check_launch(what);
}

static void coarse_dslash_mfma(at::Tensor mats, at::Tensor nbr9,
                               at::Tensor c, at::Tensor out, int64_t Na,
                               int64_t Nc, int64_t NR) {
  TORCH_CHECK(mats.scalar_type() == at::kComplexFloat &&
              c.scalar_type() == at::kComplexFloat &&
              out.scalar_type() == at::kComplexFloat);
  TORCH_CHECK(nbr9.scalar_type() == at::kLong);
  TORCH_CHECK(mats.is_contiguous() && nbr9.is_contiguous() &&
              c.is_contiguous() && out.is_contiguous());
  TORCH_CHECK(Nc % 16 == 0 && NR >= 1 && NR <= 16);
  CoarseMfmaCall cc{mats.data_ptr(), nbr9.data_ptr(), c.data_ptr(),
                    out.data_ptr(), Na, (int)Nc, (int)NR};
  launch_coarse_dslash_mfma(cc, stream());
  check_launch("coarse_dslash_mfma");
}

// Multigrid transfer (csrc/transfer.hip). Every shape the kernels index by
// is checked here; the tables' entries are range-checked in the kernels.
static TransferCall transfer_call(const char *what, const at::Tensor &field,
                                  const at::Tensor &coarse,
                                  const at::Tensor &Vn,
                                  const at::Tensor &table, bool table_is_agg) {
  TORCH_CHECK(field.is_cuda() && field.is_contiguous() && field.dim() == 4,
              what, ": field must be a contiguous GPU spinor field");
  const int prec = prec_of(field);
  TORCH_CHECK(prec <= 1, what, ": double or single fields only");
  const int W = chunk_w_of(field);
  const long Vcb = field.size(2);
  TORCH_CHECK(field.size(0) == 2 && field.size(1) * W == 24 &&
                  field.size(3) == W && Vcb > 0,
              what, ": field is not a full-parity nspin=4 field");
  const auto ctype = prec == 0 ? at::kComplexDouble : at::kComplexFloat;
  auto same_dev = [&](const at::Tensor &t, const char *name) {
    TORCH_CHECK(t.is_cuda() && t.device() == field.device() &&
                    t.is_contiguous(),
                what, ": ", name, " must be contiguous on the field's device");
  };
  same_dev(coarse, "coarse");
  same_dev(Vn, "V");
  same_dev(table, "table");
  TORCH_CHECK(coarse.scalar_type() == ctype && Vn.scalar_type() == ctype, what,
              ": coarse and V must be complex of the field's real type");
  TORCH_CHECK(coarse.dim() == 3 && coarse.size(1) == 2, what,
              ": coarse must be [Na, 2, Nv]");
  const long Na = coarse.size(0), Nv = coarse.size(2);
  TORCH_CHECK(table.scalar_type() == at::kInt, what, ": table must be int32");
  TORCH_CHECK(Na > 0 && (2 * Vcb) % Na == 0, what,
              ": Na does not divide the volume");
  const long B = 2 * Vcb / Na;
  if (table_is_agg) {  // prolong: site-fastest V
    TORCH_CHECK(Vn.dim() == 4 && Vn.size(0) == 2 && Vn.size(1) == 6 &&
                    Vn.size(2) == Nv && Vn.size(3) == 2 * Vcb,
                what, ": Vn must be [2, 6, Nv, 2*Vcb]");
    TORCH_CHECK(table.dim() == 1 && table.size(0) == 2 * Vcb, what,
                ": agg_of_site must be [2*Vcb]");
  } else {             // restrict: aggregate-ordered V
    TORCH_CHECK(Vn.dim() == 5 && Vn.size(0) == Na && Vn.size(1) == B &&
                    Vn.size(2) == 4 && Vn.size(3) == 3 && Vn.size(4) == Nv,
                what, ": V must be [Na, B, 4, 3, Nv]");
    TORCH_CHECK(table.dim() == 2 && table.size(0) == Na && table.size(1) == B,
                what, ": site_tab must be [Na, B]");
  }
  TORCH_CHECK(Nv < (1L << 20) && B < (1L << 28), what, ": sizes out of range");
  TransferCall c{};
  c.field = BlasField{field.data_ptr(), nullptr, Vcb};
  c.coarse = coarse.data_ptr();
  c.Vn = table_is_agg ? Vn.data_ptr() : nullptr;
  c.V = table_is_agg ? nullptr : Vn.data_ptr();
  c.agg_of_site = table_is_agg ? table.data_ptr<int>() : nullptr;
  c.site_tab = table_is_agg ? nullptr : table.data_ptr<int>();
  c.Na = Na;
  c.B = (int)B;
  c.Nv = (int)Nv;
  c.prec = prec;
  TORCH_CHECK(qa_transfer_grid_ok(c), what, ": launch grid out of range");
  return c;
}

static void transfer_prolong(at::Tensor out, at::Tensor coarse, at::Tensor Vn,
                             at::Tensor agg_of_site) {
  TransferCall c = transfer_call("transfer_prolong", out, coarse, Vn,
                                 agg_of_site, true);
  launch_transfer_prolong(c, stream());
  check_launch("transfer_prolong");
}

static void transfer_restrict(at::Tensor coarse_out, at::Tensor in,
                              at::Tensor V, at::Tensor site_tab) {
  TransferCall c = transfer_call("transfer_restrict", in, coarse_out, V,
                                 site_tab, false);
  launch_transfer_restrict(c, stream());
  check_launch("transfer_restrict");
}

static void transfer_block_ortho(at::Tensor V, int64_t passes) {
  TORCH_CHECK(V.is_cuda() && V.is_contiguous() &&
                  V.scalar_type() == at::kComplexDouble,
              "transfer_block_ortho: V must be a contiguous complex128 GPU "
              "tensor");
  TORCH_CHECK(V.dim() == 5 && V.size(2) == 4 && V.size(3) == 3,
              "transfer_block_ortho: V must be [Na, B, 4, 3, Nv]");
  TORCH_CHECK(passes >= 0 && passes <= 16, "transfer_block_ortho: passes");
  const long Na = V.size(0), B = V.size(1), Nv = V.size(4);
  TORCH_CHECK(Na > 0 && B > 0 && Nv > 0 && 2 * Na < (1L << 31) - 1 &&
                  6 * B < (1L << 31) - 1 && Nv < (1L << 20),
              "transfer_block_ortho: sizes out of range");
  BlockOrthoCall c{V.data_ptr(), Na, (int)B, (int)Nv, (int)passes};
  launch_transfer_block_ortho(c, stream());
  check_launch("transfer_block_ortho");
}

// Galerkin coarse-operator build (csrc/galerkin.hip): X, Y and the scratch are
// written in full. Shapes are checked here; the neighbour table's entries are
// range-checked in the kernel.
static void galerkin_build(at::Tensor X, at::Tensor Y, at::Tensor scratch,
                           at::Tensor V, at::Tensor nbr, at::Tensor bnd,
                           at::Tensor link, c10::optional<at::Tensor> clov,
                           at::Tensor coef) {
  const char *what = "galerkin_build";
  TORCH_CHECK(V.is_cuda() && V.is_contiguous() &&
                  V.scalar_type() == at::kComplexDouble,
              what, ": V must be a contiguous complex128 GPU tensor");
  TORCH_CHECK(V.dim() == 5 && V.size(2) == 4 && V.size(3) == 3, what,
              ": V must be [Na, B, 4, 3, Nv]");
  const long Na = V.size(0), B = V.size(1), Nv = V.size(4);
  TORCH_CHECK(Na > 0 && B > 0 && Nv > 0 && Nv < (1L << 20) && B < (1L << 28) &&
                  Na * B < (1L << 31) - 1,
              what, ": sizes out of range");
  const long rows = Na * B, Nc = 2 * Nv;
  auto same_dev = [&](const at::Tensor &t, const char *name) {
    TORCH_CHECK(t.is_cuda() && t.device() == V.device() && t.is_contiguous(),
                what, ": ", name, " must be contiguous on V's device");
  };
  auto c128 = [&](const at::Tensor &t, const char *name) {
    same_dev(t, name);
    TORCH_CHECK(t.scalar_type() == at::kComplexDouble, what, ": ", name,
                " must be complex128");
  };
  c128(X, "X");
  c128(Y, "Y");
  c128(scratch, "scratch");
  c128(link, "link");
  c128(coef, "coef");
  TORCH_CHECK(X.dim() == 3 && X.size(0) == Na && X.size(1) == Nc &&
                  X.size(2) == Nc,
              what, ": X must be [Na, 2*Nv, 2*Nv]");
  TORCH_CHECK(Y.dim() == 4 && Y.size(0) == 8 && Y.size(1) == Na &&
                  Y.size(2) == Nc && Y.size(3) == Nc,
              what, ": Y must be [8, Na, 2*Nv, 2*Nv]");
  TORCH_CHECK(scratch.dim() == 4 && scratch.size(0) == 9 &&
                  scratch.size(1) == Na && scratch.size(2) == Nc &&
                  scratch.size(3) == Nc,
              what, ": scratch must be [9, Na, 2*Nv, 2*Nv]");
  same_dev(nbr, "nbr");
  same_dev(bnd, "bnd");
  TORCH_CHECK(nbr.scalar_type() == at::kInt && nbr.dim() == 2 &&
                  nbr.size(0) == rows && nbr.size(1) == 8,
              what, ": nbr must be int32 [Na*B, 8]");
  TORCH_CHECK(bnd.scalar_type() == at::kByte && bnd.dim() == 1 &&
                  bnd.size(0) == rows,
              what, ": bnd must be uint8 [Na*B]");
  TORCH_CHECK(link.dim() == 4 && link.size(0) == rows && link.size(1) == 8 &&
                  link.size(2) == 3 && link.size(3) == 3,
              what, ": link must be [Na*B, 8, 3, 3]");
  TORCH_CHECK(coef.dim() == 3 && coef.size(0) == 8 && coef.size(1) == 4 &&
                  coef.size(2) == 4,
              what, ": coef must be [8, 4, 4]");
  const void *cl = nullptr;
  if (clov.has_value()) {
    c128(*clov, "clov");
    TORCH_CHECK(clov->dim() == 3 && clov->size(0) == rows &&
                    clov->size(1) == 12 && clov->size(2) == 12,
                what, ": clov must be [Na*B, 12, 12]");
    cl = clov->data_ptr();
  }
  GalerkinCall c{X.data_ptr(), Y.data_ptr(), scratch.data_ptr(),
                 V.data_ptr(), nbr.data_ptr<int>(),
                 bnd.data_ptr<unsigned char>(), link.data_ptr(), cl,
                 coef.data_ptr(), Na, (int)B, (int)Nv};
  TORCH_CHECK(qa_galerkin_grid_ok(c), what, ": launch grid out of range");
  launch_galerkin_build(c, stream());
  check_launch(what);
}

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.def("galerkin_build", &galerkin_build,
        "Galerkin coarse operator X, Y[8] from the aggregate-ordered V "
        "(fixed summation order)",
        py::arg("X"), py::arg("Y"), py::arg("scratch"), py::arg("V"),
        py::arg("nbr"), py::arg("bnd"), py::arg("link"), py::arg("clov"),
        py::arg("coef"));
  m.def("transfer_prolong", &transfer_prolong,
        "MG prolongator: fine field = V * coarse, written in native storage",
        py::arg("out"), py::arg("coarse"), py::arg("Vn"),
        py::arg("agg_of_site"));
  m.def("transfer_restrict", &transfer_restrict,
        "MG restrictor: coarse = V^dag * fine field (fixed-order reduction)",
        py::arg("coarse_out"), py::arg("in"), py::arg("V"),
        py::arg("site_tab"));
  m.def("transfer_block_ortho", &transfer_block_ortho,
        "in-place per-(aggregate, chirality) modified Gram-Schmidt of V",
        py::arg("V"), py::arg("passes") = 2);
  m.def("dslash_wilson", &dslash_wilson, "Wilson(-clover/-twisted) dslash",
        py::arg("out"), py::arg("out_n"), py::arg("in"), py::arg("in_n"),
        py::arg("gauge"), py::arg("clover"), py::arg("x"), py::arg("x_n"),
        py::arg("dims"), py::arg("parity_offset"), py::arg("Vcb"),
        py::arg("parity"), py::arg("dagger"), py::arg("mode"),
        py::arg("xpay"), py::arg("a"), py::arg("recon"), py::arg("ghost"),
        py::arg("ghost_nrm"), py::arg("face_cb"), py::arg("comm_mask"),
        py::arg("kt"), py::arg("b_re") = 0.0, py::arg("b_im") = 0.0,
        py::arg("v_stride") = 0, py::arg("s_offset") = 0,
        py::arg("out2") = py::none(), py::arg("out2_n") = py::none(),
        py::arg("dot_y") = py::none(), py::arg("dot_y_n") = py::none(),
        py::arg("dot_result") = py::none(), py::arg("dot_slots") = 1,
        py::arg("dot_stride") = 1);
  m.def("pack_face", &pack_face, "halo face pack (spin-projected)",
        py::arg("dst"), py::arg("dst_nrm"), py::arg("in"), py::arg("in_n"),
        py::arg("dims"), py::arg("parity_offset"), py::arg("Vcb"),
        py::arg("parity"), py::arg("mu"), py::arg("s01"), py::arg("edge"),
        py::arg("Fcb"), py::arg("v_stride") = 0, py::arg("s_offset") = 0);
  m.def("pack_face_stag", &pack_face_stag, "staggered halo face pack");
  m.def("dslash_wilson_mrhs", &dslash_wilson_mrhs,
        "multi-RHS Wilson(-clover) dslash: NRHS sides per gauge load",
        py::arg("out"), py::arg("out_n"), py::arg("in"), py::arg("in_n"),
        py::arg("gauge"), py::arg("clover"), py::arg("x"), py::arg("x_n"),
        py::arg("dims"), py::arg("parity_offset"), py::arg("Vcb"),
        py::arg("parity"), py::arg("dagger"), py::arg("mode"),
        py::arg("xpay"), py::arg("a"), py::arg("recon"), py::arg("ghost"),
        py::arg("ghost_nrm"), py::arg("face_cb"), py::arg("comm_mask"),
        py::arg("kt"), py::arg("v_stride") = 0,
        py::arg("s_offsets") = std::vector<int64_t>{});
  m.def("gauge_path_dir", &gauge_path_dir,
        "path-table force / path product of one direction (fused mom update)");
  m.def("gauge_loop_trace", &gauge_loop_trace,
        "per-site traces of a table of closed loops");
  m.def("flow_zmat_dir", &flow_zmat_dir, "wilson-flow Z = eps TA[S U^d]");
  m.def("flow_expmul_dir", &flow_expmul_dir, "U' = exp(Zc) U");
  m.def("stout_smear_dir", &stout_smear_dir,
        "native stout smear of one direction (exp via scale-and-square)");
  m.def("heatbath_sweep_dir", &heatbath_sweep_dir,
        "SU(2)-subgroup heatbath/overrelax update of one (parity, mu)");
  m.def("coarse_dslash_mfma", &coarse_dslash_mfma,
        "coarse-grid 9-matrix dslash on f32 MFMA tiles");
  m.def("dslash_staggered", &dslash_staggered, "naive staggered dslash");
  m.def("set_dslash_block", &set_dslash_block, "autotuner: dslash workgroup size");
  m.def("set_dslash_waves", &set_dslash_waves,
        "occupancy experiment: 0 default, 3 = 64-thread/3-wave variant "
        "(half/single/quarter; double keeps its default kernel)");
  m.def("set_dslash_lds", &set_dslash_lds,
        "LDS-tiled dslash policy: 1 = stage the in-spinor halo tile in LDS "
        "(half/quarter, local, tile-divisible dims)");
  m.def("get_dslash_block", &get_dslash_block, "current dslash workgroup size");
  m.def("get_dslash_lds", &get_dslash_lds, "current LDS-tiled dslash policy");
  m.def("get_dslash_waves", &get_dslash_waves, "current occupancy variant");
  m.def("ipc_get_handle", &ipc_get_handle, "hipIpcGetMemHandle of a tensor");
  m.def("ipc_open_handle", &ipc_open_handle, "open a peer IPC handle");
  m.def("ipc_close_handle", &ipc_close_handle, "close a peer IPC mapping");
  m.def("pack_face_ptr", &pack_face_ptr,
        "pack a halo face into a raw (IPC peer) pointer");
  m.def("dwf5", &dwf5, "DWF/Moebius 5th-dim ops (Ds apply / M5 inverse)");
  m.def("dwf_fused", &dwf_fused,
        "fused domain-wall kernel: out = [x +] a * W_chi (Dhat in), all Ls "
        "slices in one launch",
        py::arg("out"), py::arg("out_n"), py::arg("in"), py::arg("in_n"),
        py::arg("gauge"), py::arg("x"), py::arg("x_n"), py::arg("W"),
        py::arg("dims"), py::arg("parity_offset"), py::arg("Vcb"),
        py::arg("Ls"), py::arg("parity"), py::arg("dagger"), py::arg("xpay"),
        py::arg("a"), py::arg("recon"));
  m.def("set_dwf_fused_ns", &set_dwf_fused_ns,
        "fused domain-wall kernel: sites per workgroup for single/half "
        "(16 or 32)");
  m.attr("DWF_FUSED_LS_MAX") = (int)QA_DWF_FUSED_LS_MAX;
  m.def("zdwf5", &zdwf5, "zMobius per-slice-complex 5th-dim ops");
  m.def("eofa5", &eofa5, "EOFA rank-1 extended M5 ops");
  m.def("blas_op", &blas_op, "fused blas/reduction",
        py::arg("op"), py::arg("a"), py::arg("b"), py::arg("x"),
        py::arg("x_n"), py::arg("y"), py::arg("y_n"), py::arg("Vcb"),
        py::arg("sites"), py::arg("c2") = 0.0, py::arg("d2") = 0.0,
        py::arg("ncomp") = 24, py::arg("deterministic") = false,
        py::arg("z") = py::none(), py::arg("z_n") = py::none(),
        py::arg("w") = py::none(), py::arg("w_n") = py::none());
  m.def("triple_cg_dev", &triple_cg_dev,
        "fused CG update with alpha = r2_old / acc[0] formed on the device",
        py::arg("r2_old"), py::arg("acc"), py::arg("clear"), py::arg("p"),
        py::arg("p_n"), py::arg("Ap"), py::arg("Ap_n"), py::arg("x"),
        py::arg("x_n"), py::arg("r"), py::arg("r_n"), py::arg("Vcb"),
        py::arg("sites"), py::arg("ncomp"),
        py::arg("slots"), py::arg("nslots"), py::arg("slot_stride"));
  m.def("convert", &convert, "precision conversion copy", py::arg("dst"),
        py::arg("dst_n"), py::arg("src"), py::arg("src_n"), py::arg("Vcb"),
        py::arg("sites"), py::arg("ncomp") = 24);
  m.def("clover_apply", &clover_apply, "clover term apply",
        py::arg("out"), py::arg("out_n"), py::arg("in"), py::arg("in_n"),
        py::arg("clover"), py::arg("parity"), py::arg("Vcb"),
        py::arg("v_stride") = 0, py::arg("s_offset") = 0);
  m.def("twist_apply", &twist_apply, "twisted-mass T(b) apply",
        py::arg("out"), py::arg("out_n"), py::arg("in"), py::arg("in_n"),
        py::arg("b_re"), py::arg("b_im"), py::arg("Vcb"), py::arg("sites"),
        py::arg("tau3_vcb") = 0, py::arg("acc") = false);
  m.attr("BLAS_AXPY") = (int)BLAS_AXPY;
  m.attr("BLAS_AXPY_NORM2") = (int)BLAS_AXPY_NORM2;
  m.attr("BLAS_XPAY") = (int)BLAS_XPAY;
  m.attr("BLAS_AXPBY") = (int)BLAS_AXPBY;
  m.attr("BLAS_CAXPY") = (int)BLAS_CAXPY;
  m.attr("BLAS_XMY_NORM2") = (int)BLAS_XMY_NORM2;
  m.attr("BLAS_SCAL") = (int)BLAS_SCAL;
  m.attr("BLAS_NORM2") = (int)BLAS_NORM2;
  m.attr("BLAS_TRIPLE_CG") = (int)BLAS_TRIPLE_CG;
  m.attr("BLAS_TRIPLE_CG_DEV") = (int)BLAS_TRIPLE_CG_DEV;
  m.attr("BLAS_REDOT") = (int)BLAS_REDOT;
  m.attr("BLAS_CDOT") = (int)BLAS_CDOT;
  m.attr("BLAS_CAXPBY") = (int)BLAS_CAXPBY;
}
