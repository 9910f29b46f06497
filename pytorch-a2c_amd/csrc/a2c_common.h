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

// ---- a2c_<world>_step_post (snake.hip, pong.hip, breakout.hip): what the three fused world kernels share.
// One workgroup of WORLD_POST_WAVES wavefronts per env (why 4: DESIGN.md section 6e).
constexpr int WORLD_POST_WAVES = 4, WORLD_POST_THREADS = 64 * WORLD_POST_WAVES;

// the launcher's checks of the argument block (HW: floats of one plane of this world)
static inline bool a2c_world_post_ok(const a2c_world_post* p, int64_t HW) {
  if (p == nullptr || p->val == nullptr || p->val_prev == nullptr || p->rewards == nullptr || p->dones == nullptr ||
      p->deltas == nullptr || p->prev == nullptr || p->out == nullptr)
    return false;
  if (p->T < 1 || p->t < 0 || p->t >= p->T || p->C < 1) return false;
  if (p->prev_stride % 4 != 0 || p->out_stride % 4 != 0 || p->prev_stride < p->C * HW || p->out_stride < p->C * HW) return false;
  if ((((uintptr_t)p->out | (uintptr_t)p->prev) & 15u) != 0 || p->out == p->prev) return false;
  return p->h == nullptr || p->hdim >= 1;
}

// the effective done of the step: the world's done, or any non-zero reward for a "Pong" env type
__device__ __forceinline__ float world_post_done(const a2c_world_post& p, float r, float done) {
  return (done != 0.f || (p.pong && r != 0.f)) ? 1.f : 0.f;
}

// One lane: rewards / dones / deltas / val_prev of env b, what record_kernel and post_kernel of rollout_ops.hip do (the
// delta is a2c_td_delta, the body all of them share)
__device__ __forceinline__ void world_post_book(const a2c_world_post& p, int b, float r, float d) {
  const long e = (long)(p.slot0 + b) * p.T + p.t;
  p.rewards[e] = r;
  p.dones[e] = d;
  if (p.done_eff_out != nullptr) p.done_eff_out[b] = d;
  const float v = p.val[(long)b * p.val_stride];
  if (p.t > 0) p.deltas[e - 1] = a2c_td_delta(p.rewards[e - 1], p.dones[e - 1], p.gamma, v, p.val_prev[b]);
  p.val_prev[b] = v;
}

// All WORLD_POST_THREADS lanes: the hidden row of an env whose step closed is zeroed (zero_done_rows_kernel), and planes
// 0 .. C-2 of out[b] = reset ? 0 : planes 1 .. C-1 of prev[b], one contiguous run of (C - 1) * HW floats as 16-byte accesses.
// -> where the world renders plane C - 1
__device__ __forceinline__ float* world_post_planes(const a2c_world_post& p, int b, float d, bool rst, int HW, int tid) {
  if (p.h != nullptr && d != 0.f)
    for (int i = tid; i < p.hdim; i += WORLD_POST_THREADS) p.h[(long)b * p.hdim + i] = 0.f;
  float* __restrict__ o = p.out + (long)b * p.out_stride;
  const int n4 = ((p.C - 1) * HW) >> 2;
  float4* __restrict__ o4 = reinterpret_cast<float4*>(o);
  if (rst) {
    for (int i = tid; i < n4; i += WORLD_POST_THREADS) o4[i] = make_float4(0.f, 0.f, 0.f, 0.f);
  } else {
    const float4* __restrict__ s4 = reinterpret_cast<const float4*>(p.prev + (long)b * p.prev_stride + HW);
#pragma unroll 8
    for (int i = tid; i < n4; i += WORLD_POST_THREADS) o4[i] = s4[i];
  }
  return o + (long)(p.C - 1) * HW;
}
