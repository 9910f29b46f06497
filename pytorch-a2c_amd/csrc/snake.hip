// Snake worlds in device memory: a2c_snake_reset / a2c_snake_step / a2c_snake_step_post (rules: DESIGN.md "Snake"; host twin: a2c_amd/snake.py).
//
// One wavefront per env.  The G x G grid is a time-to-live map (0 free, -1 food, n > 0: occupied for n more steps, the
// head holds the length), kept in HBM between launches and worked on in LDS: a step is one pass over the cells, a food
// placement one ballot/popcount pass that finds the k-th free cell in row-major order (no rejection loop).  The draw and
// step counters are part of the state the kernel advances, so a captured launch plays NEW steps at every replay.  The
// prepped frame row (snake_prep's values) is written as 16-byte stores where the frame-stack kernel reads it.  The draws
// (world_hash) and the a2c_snake_step_post helpers come from world.h; the kernels are this file's own, because the cells live
// in LDS and the step is cooperative.
#include "world.h"

namespace {

constexpr int SNAKE_HDR = 8;        // int32 words in front of the cells: head row, head col, length, draws, steps, episode reward
constexpr int SNAKE_MAX_G = 32;
constexpr int SNAKE_MAX_CELLS = SNAKE_MAX_G * SNAKE_MAX_G;

// food on the k-th free cell in row-major order (k < number of free cells); the whole wave calls it
__device__ __forceinline__ void snake_place_food(int* s, int NC, uint32_t k, int lane) {
  int left = (int)k;
  bool placed = false;
  for (int base = 0; base < NC; base += 64) {
    const int i = base + lane;
    const bool fr = i < NC && s[i] == 0;
    const unsigned long long m = __ballot(fr);
    if (!placed) {
      const int cnt = __popcll(m);
      if (left < cnt) {
        const int rank = __popcll(m & ((1ull << lane) - 1ull));
        if (fr && rank == left) s[i] = -1;
        placed = true;
      } else {
        left -= cnt;
      }
    }
  }
  __syncthreads();
}

// a new episode: heading and head cell from two draws, a snake of length 3 behind the head, n_foods foods
__device__ __forceinline__ void snake_new_episode(int* s, int G, int NC, int n_foods, uint32_t seed, uint32_t env,
                                                  uint32_t& draws, int& hr, int& hc, int& len, int lane) {
  for (int i = lane; i < NC; i += 64) s[i] = 0;
  const int h = (int)(world_hash(seed, env, draws++) & 3u);
  const int k = (int)(world_hash(seed, env, draws++) % (uint32_t)((G - 2) * G));
  const int a = k / G, b = k % G;
  const int dr = h == 0 ? -1 : (h == 2 ? 1 : 0), dc = h == 1 ? 1 : (h == 3 ? -1 : 0);
  hr = h == 0 ? a : (h == 2 ? a + 2 : b);
  hc = h == 1 ? a + 2 : (h == 3 ? a : b);
  len = 3;
  __syncthreads();
  if (lane < 3) s[(hr - lane * dr) * G + (hc - lane * dc)] = 3 - lane;
  __syncthreads();
  for (int i = 0; i < n_foods; ++i)
    snake_place_food(s, NC, world_hash(seed, env, draws++) % (uint32_t)(NC - 3 - i), lane);
}

__device__ __forceinline__ float snake_prep_value(int v, int len) {
  return v == 0 ? 0.0f : (v < 0 ? 0.33f : (v == len ? 1.5f : 1.0f));
}

// frame row (HW floats, HW % 4 == 0) as float4 stores to `frame` and / or `frame2` (either may be null); raw RGB (3*HW
// bytes) as 4-byte words; by `nthreads` lanes
__device__ __forceinline__ void snake_write_frames(const int* s, int G, int unit, int len, float* __restrict__ frame,
                                                   float* __restrict__ frame2, uint8_t* __restrict__ rgb, int tid,
                                                   int nthreads) {
  const int W = G * unit, HW = W * W;
  float4* f4 = reinterpret_cast<float4*>(frame);
  float4* g4 = reinterpret_cast<float4*>(frame2);
  for (int q = tid; q < HW / 4; q += nthreads) {
    float v[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int p = 4 * q + j;
      v[j] = snake_prep_value(s[((p / W) / unit) * G + (p % W) / unit], len);
    }
    if (f4 != nullptr) f4[q] = make_float4(v[0], v[1], v[2], v[3]);
    if (g4 != nullptr) g4[q] = make_float4(v[0], v[1], v[2], v[3]);
  }
  if (rgb != nullptr) {
    uint32_t* w4 = reinterpret_cast<uint32_t*>(rgb);
    for (int q = tid; q < 3 * HW / 4; q += nthreads) {
      uint32_t word = 0u;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int byte = 4 * q + j, p = byte / 3, ch = byte - 3 * p;
        const int v = s[((p / W) / unit) * G + (p % W) / unit];
        // space [0,255,0]  body [1,0,0]  head [255,0,0]  food [0,0,255]
        const uint32_t r = v > 0 ? (v == len ? 255u : 1u) : 0u, g = v == 0 ? 255u : 0u, b = v < 0 ? 255u : 0u;
        word |= (ch == 0 ? r : (ch == 1 ? g : b)) << (8 * j);
      }
      w4[q] = word;
    }
  }
}

// the header words of an env
struct SnakeHead {
  int hr, hc, len;
  uint32_t draws;
  int steps, ep_rew;
};

__device__ __forceinline__ void snake_load_head(const int32_t* st, SnakeHead& h) {
  h.hr = st[0]; h.hc = st[1]; h.len = st[2];
  h.draws = (uint32_t)st[3];
  h.steps = st[4]; h.ep_rew = st[5];
}

// One step of one world by one wave: the cells come from `st` into this wave's LDS copy `s`, the header is in registers.
// Every wave of the workgroup must call it (it holds barriers), each with an `s` of its own.  -> the reward; over: the
// episode ended and the world has been restarted; over_rew: the episode's reward, what such a step adds to ep_stats[1]
__device__ __forceinline__ float snake_advance(int* s, const int32_t* st, SnakeHead& h, int a, uint32_t seed, uint32_t env,
                                               int G, int NC, int n_foods, int lane, bool& over, int& over_rew) {
  for (int i = lane; i < NC; i += 64) s[i] = st[SNAKE_HDR + i];
  __syncthreads();
  const int nr = h.hr + (a == 0 ? -1 : (a == 2 ? 1 : 0)), nc = h.hc + (a == 1 ? 1 : (a == 3 ? -1 : 0));
  const bool inside = nr >= 0 && nr < G && nc >= 0 && nc < G;
  const int v = inside ? s[nr * G + nc] : 1;
  __syncthreads();
  float r = 0.0f;
  over = false;
  ++h.steps;
  if (v > 0) {                       // wall, or a body cell (neck and tail cell included)
    r = -1.0f;
    over = true;
  } else if (v < 0) {                // food: grow by one, nothing is vacated
    r = 1.0f;
    ++h.len;
    h.hr = nr; h.hc = nc;
    if (lane == 0) s[nr * G + nc] = h.len;
    __syncthreads();
    const int n_free = NC - h.len - (n_foods - 1);
    if (n_free == 0) over = true;    // the grid is full
    else snake_place_food(s, NC, world_hash(seed, env, h.draws++) % (uint32_t)n_free, lane);
  } else {                           // plain move: every occupied cell ages, the tail cell is vacated
    for (int i = lane; i < NC; i += 64) {
      const int c = s[i];
      if (c > 0) s[i] = c - 1;
    }
    __syncthreads();
    h.hr = nr; h.hc = nc;
    if (lane == 0) s[nr * G + nc] = h.len;
    __syncthreads();
  }
  h.ep_rew += (int)r;
  over_rew = h.ep_rew;
  if (over) {
    h.ep_rew = 0;
    snake_new_episode(s, G, NC, n_foods, seed, env, h.draws, h.hr, h.hc, h.len, lane);
  }
  return r;
}

// lane 0 of the wave that owns the env: what a step leaves beside the state words
__device__ __forceinline__ void snake_publish(int e, float r, bool over, int over_rew, float* rew, float* done, float* reset,
                                              int32_t* ep_stats) {
  if (over && ep_stats != nullptr) {
    atomicAdd(&ep_stats[0], 1);
    atomicAdd(&ep_stats[1], over_rew);
  }
  rew[e] = r;
  done[e] = over ? 1.0f : 0.0f;
  reset[e] = over ? 1.0f : 0.0f;
}

__device__ __forceinline__ void snake_store(int32_t* st, const int* s, const SnakeHead& h, int NC, int lane) {
  for (int i = lane; i < NC; i += 64) st[SNAKE_HDR + i] = s[i];
  if (lane < SNAKE_HDR) {
    const int hv = lane == 0 ? h.hr : lane == 1 ? h.hc : lane == 2 ? h.len : lane == 3 ? (int)h.draws : lane == 4 ? h.steps
                 : lane == 5 ? h.ep_rew : 0;
    st[lane] = hv;
  }
}

template <bool STEP>
__global__ __launch_bounds__(64) void snake_kernel(int32_t* __restrict__ state, int words, const int64_t* __restrict__ actions,
                                                   int64_t act_stride, int action_shift, int env_id0, uint32_t seed, int G,
                                                   int unit, int n_foods, float* __restrict__ rew, float* __restrict__ done,
                                                   float* __restrict__ reset, float* __restrict__ frames,
                                                   uint8_t* __restrict__ rgb, int32_t* __restrict__ ep_stats) {
  __shared__ int s[SNAKE_MAX_CELLS];
  const int e = blockIdx.x, lane = threadIdx.x;
  const int NC = G * G;
  const uint32_t env = (uint32_t)(env_id0 + e);
  int32_t* st = state + (int64_t)e * words;
  SnakeHead h;
  snake_load_head(st, h);
  const int HW = G * unit * G * unit;
  if (STEP) {
    const int a = (int)((actions[(int64_t)e * act_stride] + (int64_t)action_shift) & 3);
    bool over;
    int over_rew;
    const float r = snake_advance(s, st, h, a, seed, env, G, NC, n_foods, lane, over, over_rew);
    if (lane == 0) snake_publish(e, r, over, over_rew, rew, done, reset, ep_stats);
  } else {
    h.draws = 0u; h.steps = 0; h.ep_rew = 0;
    snake_new_episode(s, G, NC, n_foods, seed, env, h.draws, h.hr, h.hc, h.len, lane);
  }
  __syncthreads();
  snake_store(st, s, h, NC, lane);
  snake_write_frames(s, G, unit, h.len, frames + (int64_t)e * HW, nullptr, rgb == nullptr ? nullptr : rgb + (int64_t)e * 3 * HW,
                     lane, 64);
}

// a2c_snake_step_post: snake_kernel<true> + the step's bookkeeping + the frame stack, WORLD_POST_WAVES waves per env.  Every
// wave plays the same step on an LDS copy of the cells of its own (the step's barriers are the workgroup's: the first one,
// behind the loads of the cells, also keeps wave 0's stores behind every wave's loads); all lanes then render from theirs.
__global__ __launch_bounds__(WORLD_POST_THREADS) void snake_post_kernel(
    int32_t* __restrict__ state, int words, const int64_t* __restrict__ actions, int64_t act_stride, int action_shift,
    int env_id0, uint32_t seed, int G, int unit, int n_foods, float* __restrict__ rew, float* __restrict__ done,
    float* __restrict__ reset, float* __restrict__ frames, uint8_t* __restrict__ rgb, int32_t* __restrict__ ep_stats,
    const a2c_world_post post) {
  __shared__ int s_all[WORLD_POST_WAVES][SNAKE_MAX_CELLS];
  const int e = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
  int* s = s_all[tid >> 6];
  const int NC = G * G;
  const uint32_t env = (uint32_t)(env_id0 + e);
  int32_t* st = state + (int64_t)e * words;
  SnakeHead h;
  snake_load_head(st, h);
  const int HW = G * unit * G * unit;
  const int a = (int)((actions[(int64_t)e * act_stride] + (int64_t)action_shift) & 3);
  bool over;
  int over_rew;
  const float r = snake_advance(s, st, h, a, seed, env, G, NC, n_foods, lane, over, over_rew);
  const float d = world_post_done(post, r, over ? 1.0f : 0.0f);
  if (tid == 0) {
    snake_publish(e, r, over, over_rew, rew, done, reset, ep_stats);
    world_post_book(post, e, r, d);
  }
  __syncthreads();
  if (tid < 64) snake_store(st, s, h, NC, tid);
  float* top = world_post_planes(post, e, d, over, HW, tid);
  snake_write_frames(s, G, unit, h.len, top, frames == nullptr ? nullptr : frames + (int64_t)e * HW,
                     rgb == nullptr ? nullptr : rgb + (int64_t)e * 3 * HW, tid, WORLD_POST_THREADS);
}

bool snake_world_ok(int G, int unit, int n_foods) {
  if (G < 4 || G > SNAKE_MAX_G || unit < 1 || unit > 16) return false;
  if (((G * unit) * (G * unit)) % 4 != 0) return false;
  return n_foods >= 1 && n_foods < G * G - 3;
}

}  // namespace

extern "C" size_t a2c_snake_state_bytes(int G, int n_foods) {
  if (G < 4 || G > SNAKE_MAX_G || n_foods < 1 || n_foods >= G * G - 3) return 0;
  return sizeof(int32_t) * (size_t)(SNAKE_HDR + G * G);
}

extern "C" int a2c_snake_reset(int32_t* state, int B, int env_id0, uint32_t seed, int G, int unit, int n_foods, float* frames,
                               uint8_t* rgb, a2c_stream_t stream) {
  if (B < 0 || env_id0 < 0 || !snake_world_ok(G, unit, n_foods)) return A2C_ERR_ARG;
  if (B == 0) return A2C_OK;
  if (state == nullptr || frames == nullptr) return A2C_ERR_ARG;
  hipLaunchKernelGGL(snake_kernel<false>, dim3(B), dim3(64), 0, a2c_s(stream), state, SNAKE_HDR + G * G,
                     (const int64_t*)nullptr, (int64_t)0, 0, env_id0, seed, G, unit, n_foods, (float*)nullptr, (float*)nullptr,
                     (float*)nullptr, frames, rgb, (int32_t*)nullptr);
  A2C_CHECK_LAUNCH();
  return A2C_OK;
}

extern "C" int a2c_snake_step(int32_t* state, const int64_t* actions, int64_t act_stride, int action_shift, int B, int env_id0,
                              uint32_t seed, int G, int unit, int n_foods, float* rew, float* done, float* reset, float* frames,
                              uint8_t* rgb, int32_t* ep_stats, a2c_stream_t stream) {
  if (B < 0 || env_id0 < 0 || act_stride < 0 || !snake_world_ok(G, unit, n_foods)) return A2C_ERR_ARG;
  if (B == 0) return A2C_OK;
  if (state == nullptr || actions == nullptr || rew == nullptr || done == nullptr || reset == nullptr || frames == nullptr)
    return A2C_ERR_ARG;
  hipLaunchKernelGGL(snake_kernel<true>, dim3(B), dim3(64), 0, a2c_s(stream), state, SNAKE_HDR + G * G, actions, act_stride,
                     action_shift, env_id0, seed, G, unit, n_foods, rew, done, reset, frames, rgb, ep_stats);
  A2C_CHECK_LAUNCH();
  return A2C_OK;
}

extern "C" int a2c_snake_step_post(int32_t* state, const int64_t* actions, int64_t act_stride, int action_shift, int B,
                                   int env_id0, uint32_t seed, int G, int unit, int n_foods, float* rew, float* done,
                                   float* reset, float* frames, uint8_t* rgb, int32_t* ep_stats, const a2c_world_post* post,
                                   a2c_stream_t stream) {
  if (B < 0 || env_id0 < 0 || act_stride < 0 || !snake_world_ok(G, unit, n_foods)) return A2C_ERR_ARG;
  if (!a2c_world_post_ok(post, (int64_t)(G * unit) * (G * unit))) return A2C_ERR_ARG;
  if (B == 0) return A2C_OK;
  if (state == nullptr || actions == nullptr || rew == nullptr || done == nullptr || reset == nullptr) return A2C_ERR_ARG;
  if (frames != nullptr && ((uintptr_t)frames & 15u) != 0) return A2C_ERR_ARG;
  hipLaunchKernelGGL(snake_post_kernel, dim3(B), dim3(WORLD_POST_THREADS), 0, a2c_s(stream), state, SNAKE_HDR + G * G, actions,
                     act_stride, action_shift, env_id0, seed, G, unit, n_foods, rew, done, reset, frames, rgb, ep_stats, *post);
  A2C_CHECK_LAUNCH();
  return A2C_OK;
}
