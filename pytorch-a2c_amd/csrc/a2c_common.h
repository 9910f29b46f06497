// Shared helpers for the gfx950 kernels of liba2c_mi355x.so (not part of the C ABI).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>
#include "../../include/a2c_mi355x.h"

#define A2C_CHECK_LAUNCH()                                   \
  do {                                                       \
    if (hipGetLastError() != hipSuccess) return A2C_ERR_LAUNCH; \
  } while (0)

static inline hipStream_t a2c_s(a2c_stream_t s) { return (hipStream_t)s; }

// Environment switches: the only way the library reads its environment.  Every name, its values and when it is read are
// listed in include/a2c_mi355x.h ("Environment switches"); tests/test_abi.py keeps that list and the sources in step.
static inline bool a2c_env_on(const char* name) {            // set, first character '1'
  const char* v = getenv(name);
  return v != nullptr && v[0] == '1';
}
static inline int a2c_env_int(const char* name, int dflt) {  // unset or empty: dflt
  const char* v = getenv(name);
  return (v != nullptr && v[0] != '\0') ? atoi(v) : dflt;
}

// memory-bound elementwise kernels: cap the grid and grid-stride (guide G11)
static inline int a2c_grid_1d(int64_t n, int block, int max_blocks = 2048) {
  int64_t g = (n + block - 1) / block;
  if (g < 1) g = 1;
  if (g > max_blocks) g = max_blocks;
  return (int)g;
}

// wave64 sum (all lanes get the result)
template <typename T>
__device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// block sum for blockDim.x == 256 (4 waves); result valid in thread 0
template <typename T>
__device__ __forceinline__ T block_sum_256(T v, T* sm /* >= 4 */) {
  v = wave_sum(v);
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) sm[w] = v;
  __syncthreads();
  T r = sm[0] + sm[1] + sm[2] + sm[3];
  __syncthreads();
  return r;
}

// Deterministic grid-wide sum of NV doubles per workgroup (256 threads): every workgroup leaves its partials in its own slot
// of `scratch`, takes a ticket, and the LAST one to arrive adds the slots in workgroup order (fixed tree) and writes out[0..NV).
// No fp64 atomics: the result does not depend on the order in which the workgroups finish.  scratch: A2C_REDUCE_SCRATCH_DOUBLES
// doubles, word 0 = the ticket counter, zero before the first use (the last workgroup resets it); at most A2C_REDUCE_MAX_BLOCKS
// workgroups; kernels that share a scratch must be ordered (same stream).
#define A2C_REDUCE_MAX_BLOCKS 1024
static_assert(A2C_REDUCE_SCRATCH_DOUBLES >= 8 + 3 * A2C_REDUCE_MAX_BLOCKS, "include/a2c_mi355x.h: A2C_REDUCE_SCRATCH_DOUBLES");
template <int NV>
__device__ __forceinline__ void grid_sum_ordered(const double (&v)[NV], double* __restrict__ out, double* __restrict__ scratch,
                                                 double* sm /* >= 4 */) {
  __shared__ unsigned int s_last;
  if (threadIdx.x == 0) {
#pragma unroll
    for (int i = 0; i < NV; ++i) scratch[8 + (long)blockIdx.x * NV + i] = v[i];
    __threadfence();
    s_last = atomicAdd(reinterpret_cast<unsigned int*>(scratch), 1u) == gridDim.x - 1 ? 1u : 0u;
  }
  __syncthreads();
  if (s_last == 0u) return;
  __threadfence();
  const volatile double* part = scratch + 8;
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    double a = 0.0;
    for (unsigned int b = threadIdx.x; b < gridDim.x; b += 256) a += part[(long)b * NV + i];
    a = block_sum_256(a, sm);
    if (threadIdx.x == 0) out[i] = a;
  }
  if (threadIdx.x == 0) *reinterpret_cast<unsigned int*>(scratch) = 0u;
}

// The clipped-ratio (PPO) row rule of a2c_ppo_loss_fwd_bwd / a2c_gauss_ppo_fwd_bwd (ops.ppo_rows_host is its host statement),
// in fp64: d = logp - logp_old, r = e^d, surr = min(r w, clamp(r, 1 - clip, 1 + clip) w), keep = the clip does not bind
// (d surr / d logp != 0 for w != 0), kl = (r - 1) - log r >= 0.  Five partials per workgroup: a grid cap of their own.
#define A2C_PPO_MAX_BLOCKS 512
static_assert(8 + 5 * A2C_PPO_MAX_BLOCKS <= A2C_REDUCE_SCRATCH_DOUBLES, "ppo loss sums: reduce scratch too small");
struct PpoRow {
  double r, surr, kl;
  bool keep;
};
__device__ __forceinline__ PpoRow ppo_row(double d, float w, float clip) {
  PpoRow p;
  const double lo = 1.0 - (double)clip, hi = 1.0 + (double)clip, wd = (double)w;
  p.r = exp(d);
  p.surr = fmin(p.r * wd, fmin(fmax(p.r, lo), hi) * wd);
  p.keep = !((w > 0.f && p.r > hi) || (w < 0.f && p.r < lo));
  p.kl = expm1(d) - d;
  return p;
}

// Small device buffers (error flags, reduction sums; <= 256 B, 4-byte multiples) are cleared by a one-wave kernel,
// not by hipMemsetAsync: as a NODE of a captured hipGraph the memset was observed to leave 0x01010101 in a
// 4-byte flag on some replays (ROCm 7.2, gfx950), which a kernel node never does.
namespace {
__global__ void a2c_zero_words_kernel(unsigned int* p, int n) {
  for (int i = threadIdx.x; i < n; i += 64) p[i] = 0u;
}
}  // namespace
static inline void a2c_zero_async(void* p, size_t bytes, hipStream_t st) {
  hipLaunchKernelGGL(a2c_zero_words_kernel, dim3(1), dim3(64), 0, st, (unsigned int*)p, (int)(bytes / 4));
}

// TD delta of one env step (runner.py:222-232): prev_rew + gamma * val * (1 - prev_done) - prev_val, left to right, every
// operation rounded, never contracted into a fused multiply-add whatever the compiler's flags.  The ONE body of
// record_kernel, post_kernel (rollout_ops.hip) and the fused world kernels, so that they agree bit for bit by construction.
__device__ __forceinline__ float a2c_td_delta(float prev_rew, float prev_done, float gamma, float val, float prev_val) {
  const float gv = __fmul_rn(gamma, val);
  return __fsub_rn(__fadd_rn(prev_rew, __fmul_rn(gv, __fsub_rn(1.f, prev_done))), prev_val);
}
