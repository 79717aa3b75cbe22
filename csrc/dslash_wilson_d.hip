// double-precision Wilson dslash TU (recon 18 only at fp64)
//
// FMA contraction only where one source expression spells a*b+c, not
// wherever the backend finds a multiply next to an add: under the default
// (fast) mode the choice is made per kernel, and with the fenced 4-round
// schedule of the double body k_dslash_wilson and the fused-epilogue kernels
// came out one ulp apart in `out` (same instruction mix, different operands
// fused), which breaks the bitwise relations the CG relies on. With the
// contraction fixed by the source, every kernel that includes the body
// computes the same bits whatever its schedule.
// The pragma stands in front of the include on purpose: it covers the whole
// unit, k_dslash_wilson_exterior (which completes sites the interior kernel
// began, so it must round like the body) and k_pack_face included, and
// every function inlined into them. The build passes no -ffp-contract flag
// that would override it.
#pragma clang fp contract(on)
#include "dslash_wilson_impl.h"

void launch_dslash_wilson_double(const DslashCall &c, hipStream_t st) {
  dslash_launch_all<PrecDouble, 18>(c, st);
}

void launch_pack_face_double(const PackCall &c, hipStream_t st) {
  pack_launch<PrecDouble>(c, st);
}
