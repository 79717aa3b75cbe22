// Body of the Wilson dslash kernels (csrc/dslash_wilson.h), textually
// included by k_dslash_wilson and its fused-epilogue variants so all of them
// compile the very same stencil. (A shared __device__ function was measured
// to change the register allocation of the existing kernels: 206 VGPRs /
// 2 waves per SIMD became 256 + AGPR copies / 1 wave.)
// In scope at the include: Prec, RECON, DAG, MODE, XPAY, KT, ROUNDS (gather
// rounds of the stencil: 1, 2 or 4, see qa_dslash_rounds), R, the kernel
// arguments out, in, g, clov, d, parity, a, x, gh, br, bi and the
// site index i < d.Vcb. Leaves the finished site in acc[4][3] (not yet
// stored). A kernel that needs the CLOV_POST site matrix afterwards declares
// diag / tri itself and defines QA_DSLASH_CLOVER_DECLARED around the include.
  int xc[4];
  coords_from_cb(xc, i, d, parity);

  cplx<R> acc[4][3];
#pragma unroll
  for (int s = 0; s < 4; ++s)
#pragma unroll
    for (int c = 0; c < 3; ++c) acc[s][c] = {(R)0, (R)0};

  cplx<R> p[4][3], h[8][2][3], uh[2][3], U[3][3];
  // proj/recon tables encode 2P (generate_proj.py); the stencil needs P
  const R one = (R)0.5;

  bool bnd = false;  // interior: site has >=1 hop deferred to EXTERIOR
  if constexpr (KT == KT_INTERIOR) {
#pragma unroll
    for (int m = 0; m < 4; ++m)
      if (gh.active(m) && (xc[m] == 0 || xc[m] == d.X[m] - 1)) bnd = true;
  }
  bool skip[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) skip[k] = false;
  // -mu neighbor index, kept for phase 2: the backward link U_mu(x-mu) is
  // read from the NEIGHBOR's forward slot instead of this site's bwd slot.
  // The stencil layout stores every link twice (fwd slot of x == bwd slot
  // of x+mu); reading only fwd slots halves the dslash's UNIQUE gauge
  // traffic — neighbor fwd-slot lines are shared through L2 exactly like
  // the neighbor spinor loads. Boundary-crossing hops (jm < 0) still read
  // the bwd slot, which holds the -mu RANK's link from the load-time
  // exchange (fields/gauge.py from_complex).
  long jm[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) jm[k] = -1;

  // Phase 1: gather + spin-project all 8 neighbor half-spinors first — the
  // loads are independent, so the wave has 8 spinor fetches in flight
  // instead of a serialized load->project->multiply chain per direction
  // (the dslash is latency-bound at ~30% of HBM peak otherwise; measured
  // FETCH_SIZE is already near-minimal).
#define QA_GATHER(MU)                                                     \
  {                                                                       \
    bool cross_p = KT != KT_LOCAL && gh.active(MU) && xc[MU] == d.X[MU] - 1; \
    if (KT == KT_INTERIOR && cross_p) {                                   \
      skip[2 * MU] = true;                                                \
    } else if (KT == KT_FUSED && cross_p) {                               \
      gh.load(h[2 * MU], MU, 1, ghost_idx(xc, MU, d));                    \
    } else {                                                              \
      long j = neighbor_cb(xc, MU, +1, d);                                \
      in.load(p, j);                                                      \
      if constexpr (!DAG) proj_##MU##_0(h[2 * MU], p);                    \
      else proj_##MU##_1(h[2 * MU], p);                                   \
    }                                                                     \
    bool cross_m = KT != KT_LOCAL && gh.active(MU) && xc[MU] == 0;        \
    if (KT == KT_INTERIOR && cross_m) {                                   \
      skip[2 * MU + 1] = true;                                            \
    } else if (KT == KT_FUSED && cross_m) {                               \
      gh.load(h[2 * MU + 1], MU, 0, ghost_idx(xc, MU, d));                \
    } else {                                                              \
      long j = neighbor_cb(xc, MU, -1, d);                                \
      jm[MU] = j;                                                         \
      in.load(p, j);                                                      \
      if constexpr (!DAG) proj_##MU##_1(h[2 * MU + 1], p);                \
      else proj_##MU##_0(h[2 * MU + 1], p);                               \
    }                                                                     \
  }

  // Phase 2 macro: gauge multiplies + spin reconstruction (fwd link at own
  // site; bwd link from the -mu neighbor's fwd slot, see jm above)
#define QA_MUL(MU)                                                        \
  {                                                                       \
    if (!skip[2 * MU]) {                                                  \
      g.template load<MU>(U, i);                                          \
      su3_mul_half(uh, U, h[2 * MU]);                                     \
      if constexpr (!DAG) recon_##MU##_0(acc, uh, one);                   \
      else recon_##MU##_1(acc, uh, one);                                  \
    }                                                                     \
    if (!skip[2 * MU + 1]) {                                              \
      if (jm[MU] >= 0) g.template load_o<MU>(U, jm[MU]);                  \
      else g.template load<4 + MU>(U, i);                                 \
      su3_dagmul_half(uh, U, h[2 * MU + 1]);                              \
      if constexpr (!DAG) recon_##MU##_1(acc, uh, one);                   \
      else recon_##MU##_0(acc, uh, one);                                  \
    }                                                                     \
  }

  // Round fence. A round is "gather some directions, multiply them into
  // acc"; the fence between two rounds keeps the next round's loads from
  // being issued (and their destinations from being live) before this
  // round's half-spinors and links are dead. It emits no instruction: acc
  // is an in/out operand, so every multiply-add that feeds acc must finish
  // above the fence, and the memory clobber keeps the later loads below it.
  // __builtin_amdgcn_sched_barrier(0) and a bare asm("" ::: "memory") do
  // not do this: both hold the loads in place, but the arithmetic has no
  // memory side effect and no tie to either, so the scheduler sinks all of
  // it below the last barrier and every gathered value is live at once,
  // exactly as in the unsplit form (double: ~750 B/lane of scratch).
  // Four statements of six operands: inline asm takes at most 30 operands.
#define QA_ROUND_FENCE()                                                  \
  _Pragma("unroll")                                                       \
  for (int s_ = 0; s_ < 4; ++s_)                                          \
    asm volatile("" : "+v"(acc[s_][0].re), "+v"(acc[s_][0].im),           \
                      "+v"(acc[s_][1].re), "+v"(acc[s_][1].im),           \
                      "+v"(acc[s_][2].re), "+v"(acc[s_][2].im) :: "memory");

  if constexpr (ROUNDS == 1) {
    // all 8 gathers in flight, then all multiplies (max load ILP; ~210
    // VGPRs -> 2 waves/SIMD at half)
    QA_GATHER(0)
    QA_GATHER(1)
    QA_GATHER(2)
    QA_GATHER(3)
    QA_MUL(0)
    QA_MUL(1)
    QA_MUL(2)
    QA_MUL(3)
  } else if constexpr (ROUNDS == 2) {
    // two 4-neighbor rounds halve the live half-spinor state so the
    // LBW-wave occupancy cap is met without spilling — trades per-wave
    // load ILP for thread-level parallelism
    QA_GATHER(0)
    QA_GATHER(1)
    QA_MUL(0)
    QA_MUL(1)
    QA_ROUND_FENCE()
    QA_GATHER(2)
    QA_GATHER(3)
    QA_MUL(2)
    QA_MUL(3)
  } else {
    // one direction per round: two spinors and two links live at a time
    // (double: the only form that fits the register file, see
    // qa_dslash_rounds)
    static_assert(ROUNDS == 4);
    QA_GATHER(0)
    QA_MUL(0)
    QA_ROUND_FENCE()
    QA_GATHER(1)
    QA_MUL(1)
    QA_ROUND_FENCE()
    QA_GATHER(2)
    QA_MUL(2)
    QA_ROUND_FENCE()
    QA_GATHER(3)
    QA_MUL(3)
  }
#undef QA_ROUND_FENCE
#undef QA_GATHER
#undef QA_MUL

  // boundary sites under CLOV_POST defer the whole epilogue: store raw sum
  if constexpr (KT == KT_INTERIOR && MODE == CLOV_POST) {
    if (bnd) {
      out.store(acc, i);
      return;
    }
  }

  if constexpr (MODE == CLOV_POST) {
#ifndef QA_DSLASH_CLOVER_DECLARED
    R diag[2][6];
    cplx<R> tri[2][15];
#endif
    clov.load(diag, tri, parity, i);
    cplx<R> tmp[4][3];
    clover_mul(tmp, diag, tri, acc);
#pragma unroll
    for (int s = 0; s < 4; ++s)
#pragma unroll
      for (int c = 0; c < 3; ++c) acc[s][c] = tmp[s][c];
  }
  if constexpr (MODE == TWIST_POST) twist_mul(acc, br, bi);

  if constexpr (XPAY || MODE == CLOV_X || MODE == TWIST_X || MODE == CLOVTW_X) {
    cplx<R> xv[4][3];
    x.load(xv, i);
    if constexpr (MODE == CLOV_X || MODE == CLOVTW_X) {
      R diag[2][6];
      cplx<R> tri[2][15];
      clov.load(diag, tri, parity, i);
      cplx<R> Ax[4][3];
      clover_mul(Ax, diag, tri, xv);
      if constexpr (MODE == CLOVTW_X) {
        twist_mul(xv, (R)0, bi);  // i b_im g5 x
#pragma unroll
        for (int s = 0; s < 4; ++s)
#pragma unroll
          for (int c = 0; c < 3; ++c) Ax[s][c] += xv[s][c];
      }
#pragma unroll
      for (int s = 0; s < 4; ++s)
#pragma unroll
        for (int c = 0; c < 3; ++c) acc[s][c] = Ax[s][c] + a * acc[s][c];
    } else if constexpr (MODE == TWIST_X) {
      twist_mul(xv, br, bi);
#pragma unroll
      for (int s = 0; s < 4; ++s)
#pragma unroll
        for (int c = 0; c < 3; ++c) acc[s][c] = xv[s][c] + a * acc[s][c];
    } else {
#pragma unroll
      for (int s = 0; s < 4; ++s)
#pragma unroll
        for (int c = 0; c < 3; ++c) acc[s][c] = xv[s][c] + a * acc[s][c];
    }
  } else {
    if (a != (R)1) {
#pragma unroll
      for (int s = 0; s < 4; ++s)
#pragma unroll
        for (int c = 0; c < 3; ++c) acc[s][c] = a * acc[s][c];
    }
  }

