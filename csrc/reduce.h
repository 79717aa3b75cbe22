// Block reduction plumbing shared by the BLAS reductions (csrc/blas.hip)
// and the fused dot epilogue of the Wilson dslash (csrc/dslash_wilson.h):
// wave shuffle-reduce -> LDS across waves -> one f64 atomic per block.
#pragma once

#include <hip/hip_runtime.h>

__device__ __forceinline__ double wave_reduce(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  return v;
}

// EVERY thread of the block must reach this call (it holds a
// __syncthreads()); blocks of 64, 128 or 256 threads.
// finish mode: per_block=false -> one f64 atomic per block (fast path);
// per_block=true -> write partial[blockIdx] for a deterministic ordered
// host/torch sum (ref: QUDA_DETERMINISTIC_REDUCE, comm_quda.h:204)
__device__ __forceinline__ void block_atomic_add(double v, double *out,
                                                 bool per_block = false,
                                                 int slot_stride = 1,
                                                 int slot = 0) {
  __shared__ double partial[4];
  int lane = threadIdx.x & 63;
  int wave = threadIdx.x >> 6;
  v = wave_reduce(v);
  if (lane == 0) partial[wave] = v;
  __syncthreads();
  if (wave == 0) {
    double s = (lane < (int)(blockDim.x >> 6)) ? partial[lane] : 0.0;
    s = wave_reduce(s);
    if (lane == 0) {
      if (per_block)
        out[(long)blockIdx.x * slot_stride + slot] = s;
      else
        atomicAdd(out + slot, s);
    }
  }
}
