// The Breakout game of breakout.hip and breakout_rules.hip: the rules of one game frame on BRK_WORDS int32 state words per env,
// the agent step, the 80 x 72 prepped frame row and the kernels of a2c_breakout_reset / _step / _step_post and their _skip
// forms (breakout.hip's first comment; DESIGN.md sections 6d, 6g and 6h).  A header so that the two files compile it into code
// objects of their own (why: DESIGN.md section 6i).
#pragma once
#include "world.h"

namespace {

constexpr int BRK_WORDS = 24;       // paddle x, ball x, ball y, vx, vy, lives, bricks left, draws, steps, episode steps,
                                    // reward since the last done, the 6 brick rows' 18-bit masks, the action of the
                                    // previous game frame (sticky actions; 0 without them), 6 spare
constexpr int BW = 72, BH = 80, BRK_HW = BW * BH;
constexpr int BRICK_ROWS = 6, BRICK_COLS = 18, BRICK_W = 4, BRICK_H = 3, BRICK_TOP = 11;
constexpr int BRICK_BOTTOM = BRICK_TOP + BRICK_ROWS * BRICK_H;
constexpr int FULL_ROW = (1 << BRICK_COLS) - 1, N_BRICKS = BRICK_ROWS * BRICK_COLS;
constexpr int PADDLE_W = 8, PADDLE_H = 2, PADDLE_Y = 77, PADDLE_SPEED = 3, PADDLE_START_X = 32, PADDLE_MAX_X = BW - PADDLE_W;
constexpr int BALL = 2, BALL_MAX_X = BW - BALL, LOST_Y = 78;
constexpr int SERVE_Y = 40, SERVE_X0 = 8, SERVE_SPAN = 56;
constexpr int MAX_LIVES = 5, MAX_EPISODE_STEPS = 1 << 24;
constexpr float LEVEL = 200.0f;     // the paddle and the ball

static_assert(BW == BRICK_COLS * BRICK_W && BRICK_W == 4, "one 16-byte store per brick column");

struct BrkWorld {
  int px, bx, by, vx, vy, lives, left;
  int rows[BRICK_ROWS];
};

// grey level (channel 0 of ALE's brick colours) and points of brick row r, top row first
__device__ __forceinline__ float brk_row_level(int r) {
  return r == 0 ? 200.0f : (r == 1 ? 198.0f : (r == 2 ? 180.0f : (r == 3 ? 162.0f : (r == 4 ? 72.0f : 66.0f))));
}
__device__ __forceinline__ int brk_row_points(int r) { return r < 2 ? 7 : (r < 4 ? 4 : 1); }
__device__ __forceinline__ int brk_row_mask(const BrkWorld& w, int r) {
  return r == 0 ? w.rows[0] : (r == 1 ? w.rows[1] : (r == 2 ? w.rows[2] : (r == 3 ? w.rows[3] : (r == 4 ? w.rows[4] : w.rows[5]))));
}
// the hit table: off = ball x + 1 - paddle x in 0..8 -> vx = {-2,-2,-1,-1,s,1,1,2,2}[off], s = +-1 with the sign vx had
__device__ __forceinline__ int brk_hit_vx(int off, int vx) {
  return off <= 1 ? -2 : (off <= 3 ? -1 : (off == 4 ? (vx > 0 ? 1 : -1) : (off <= 6 ? 1 : 2)));
}

__device__ __forceinline__ void brk_serve(BrkWorld& w, uint32_t d) {
  w.bx = SERVE_X0 + (int)(d % (uint32_t)SERVE_SPAN); w.by = SERVE_Y;
  w.vx = ((d >> 8) & 1u) ? 1 : -1;
  w.vy = -1;
}

__device__ __forceinline__ void brk_new_episode(BrkWorld& w, uint32_t seed, uint32_t env, int lives, uint32_t& draws,
                                                int& ep_steps) {
#pragma unroll
  for (int r = 0; r < BRICK_ROWS; ++r) w.rows[r] = FULL_ROW;
  w.left = N_BRICKS;
  w.lives = lives;
  w.px = PADDLE_START_X;
  ep_steps = 0;
  brk_serve(w, world_hash(seed, env, draws++));
}

// the prepped frame row: BRK_HW floats as float4 stores, the 4 pixels of one brick column in one row each, by `nthreads`
// lanes, to `frame` and / or `frame2` (either may be null)
__device__ __forceinline__ void brk_write_frame(const BrkWorld& w, float* __restrict__ frame, float* __restrict__ frame2,
                                                int tid, int nthreads) {
  float4* f4 = reinterpret_cast<float4*>(frame);
  float4* g4 = reinterpret_cast<float4*>(frame2);
  for (int q = tid; q < BRK_HW / 4; q += nthreads) {
    const int y = q / BRICK_COLS, c = q - y * BRICK_COLS, x0 = BRICK_W * c;
    float base = 0.0f;
    if (y >= BRICK_TOP && y < BRICK_BOTTOM) {
      const int r = (y - BRICK_TOP) / BRICK_H;
      if ((brk_row_mask(w, r) >> c) & 1) base = brk_row_level(r);
    }
    const bool ball_row = y >= w.by && y < w.by + BALL, paddle_row = y >= PADDLE_Y && y < PADDLE_Y + PADDLE_H;
    float v[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int x = x0 + j;
      const bool on = (ball_row && x >= w.bx && x < w.bx + BALL) || (paddle_row && x >= w.px && x < w.px + PADDLE_W);
      v[j] = on ? LEVEL : base;
    }
    if (f4 != nullptr) f4[q] = make_float4(v[0], v[1], v[2], v[3]);
    if (g4 != nullptr) g4[q] = make_float4(v[0], v[1], v[2], v[3]);
  }
}

__device__ __forceinline__ void brk_load(const int32_t* st, BrkWorld& w, WorldCount& c) {
  w.px = st[0]; w.bx = st[1]; w.by = st[2]; w.vx = st[3]; w.vy = st[4]; w.lives = st[5]; w.left = st[6];
  c.draws = (uint32_t)st[7]; c.steps = st[8]; c.ep_steps = st[9]; c.ep_rew = st[10]; c.prev = st[11 + BRICK_ROWS];
#pragma unroll
  for (int r = 0; r < BRICK_ROWS; ++r) w.rows[r] = st[11 + r] & FULL_ROW;
}

__device__ __forceinline__ void brk_store(int32_t* st, const BrkWorld& w, const WorldCount& c, int lane) {
  if (lane < BRK_WORDS) {
    const int hv = lane == 0 ? w.px : lane == 1 ? w.bx : lane == 2 ? w.by : lane == 3 ? w.vx : lane == 4 ? w.vy
                 : lane == 5 ? w.lives : lane == 6 ? w.left : lane == 7 ? (int)c.draws : lane == 8 ? c.steps
                 : lane == 9 ? c.ep_steps : lane == 10 ? c.ep_rew : lane < 11 + BRICK_ROWS ? brk_row_mask(w, lane - 11)
                 : lane == 11 + BRICK_ROWS ? c.prev : 0;
    st[lane] = hv;
  }
}

// One game frame of one world, in registers (wave-uniform; no memory access).  -> the reward; over: the episode ended and the
// world has been restarted; over_rew: the episode's reward, what such a step adds to ep_rew_sum
__device__ __forceinline__ int brk_advance(BrkWorld& w, WorldCount& c, int a, uint32_t seed, uint32_t env, int lives,
                                           int max_episode_steps, bool& over, int& over_rew) {
  ++c.steps;
  ++c.ep_steps;
  // 1. the paddle (0 and 1, ALE's FIRE, leave it where it is)
  w.px = world_clamp(w.px + (a == 2 ? PADDLE_SPEED : (a == 3 ? -PADDLE_SPEED : 0)), 0, PADDLE_MAX_X);
  // 2. the ball, the side walls, the ceiling
  const int y0 = w.by;
  int x = w.bx + w.vx, y = y0 + w.vy;
  if (x < 0) { x = -x; w.vx = -w.vx; }
  else if (x > BALL_MAX_X) { x = 2 * BALL_MAX_X - x; w.vx = -w.vx; }
  if (y < 0) { y = -y; w.vy = -w.vy; }
  // 3. the brick under the leading corner of the new position
  int r = 0;
  const int lx = x + (w.vx > 0 ? 1 : 0), ly = y + (w.vy > 0 ? 1 : 0);
  if (ly >= BRICK_TOP && ly < BRICK_BOTTOM) {
    const int br = (ly - BRICK_TOP) / BRICK_H, bc = lx / BRICK_W;      // 0 <= lx <= 71: bc in 0..17
    if ((brk_row_mask(w, br) >> bc) & 1) {
#pragma unroll
      for (int k = 0; k < BRICK_ROWS; ++k) w.rows[k] &= ~(k == br ? (1 << bc) : 0);
      --w.left;
      r = brk_row_points(br);
      y = y0;
      w.vy = -w.vy;
      if (br < 3) w.vy = w.vy > 0 ? 2 : -2;
    }
  }
  // 4. the paddle
  if (w.vy > 0 && y0 + 1 < PADDLE_Y && y + 1 >= PADDLE_Y && x >= w.px - 1 && x <= w.px + PADDLE_W - 1) {
    const int off = x + 1 - w.px;
    y = PADDLE_Y - BALL;
    w.vy = -w.vy;
    w.vx = brk_hit_vx(off, w.vx);
  }
  w.bx = x; w.by = y;
  // 5. a life
  const bool lost = y > LOST_Y;
  if (lost) --w.lives;
  // 6. the end of the episode, or the serve
  over = w.lives == 0 || w.left == 0 || c.ep_steps >= max_episode_steps;
  c.ep_rew += r;
  over_rew = c.ep_rew;
  if (over) {
    c.ep_rew = 0;
    brk_new_episode(w, seed, env, lives, c.draws, c.ep_steps);
  } else if (lost) {
    brk_serve(w, world_hash(seed, env, c.draws++));
  }
  return r;
}

// One agent step: frame_skip game frames with action a, each keeping the previous frame's action when its sticky draw (taken
// BEFORE the frame itself; none with sticky_num == 0) mod sticky_den is below sticky_num; an episode end drops the
// remaining frames.  -> the summed reward; over, over_rew: as brk_advance
__device__ __forceinline__ int brk_agent_step(BrkWorld& w, WorldCount& c, int a, uint32_t seed, uint32_t env, int lives,
                                              int max_episode_steps, int frame_skip, int sticky_num, int sticky_den, bool& over,
                                              int& over_rew) {
  int R = 0;
  over = false;
  for (int s = 0; s < frame_skip; ++s) {
    int x = a;
    if (sticky_num > 0) {
      if ((int)(world_hash(seed, env, c.draws++) % (uint32_t)sticky_den) < sticky_num) x = c.prev;
      c.prev = x;
    }
    R += brk_advance(w, c, x, seed, env, lives, max_episode_steps, over, over_rew);
    if (over) {
      c.prev = 0;
      break;
    }
  }
  return R;
}

// lane 0 of the wave that owns the env: what a step leaves beside the state words
__device__ __forceinline__ void brk_publish(int e, int r, bool over, int over_rew, float* rew, float* done, float* reset,
                                            int32_t* ep_count, int32_t* ep_rew_sum) {
  if (over) {
    if (ep_count != nullptr) atomicAdd(ep_count, 1);
    if (ep_rew_sum != nullptr) atomicAdd(ep_rew_sum, over_rew);
  }
  rew[e] = (float)r;
  done[e] = over ? 1.0f : 0.0f;
  reset[e] = over ? 1.0f : 0.0f;
}

// REPEAT == false is the (1, 0, .) world with its constants folded: one game frame, no loop, no sticky draw -- the kernel of
// a2c_breakout_step as it was before frame skip (the loop with frame_skip = 1 at run time cost 0.15-0.35 us)
template <bool STEP, bool REPEAT>
__global__ __launch_bounds__(64) void breakout_kernel(int32_t* __restrict__ state, const int64_t* __restrict__ actions,
                                                      int64_t act_stride, int action_shift, int env_id0, uint32_t seed,
                                                      int lives, int max_episode_steps, int frame_skip, int sticky_num,
                                                      int sticky_den, float* __restrict__ frames,
                                                      int64_t frame_ld, float* __restrict__ rew, float* __restrict__ done,
                                                      float* __restrict__ reset, int32_t* __restrict__ ep_count,
                                                      int32_t* __restrict__ ep_rew_sum) {
  const int e = blockIdx.x, lane = threadIdx.x;
  const uint32_t env = (uint32_t)(env_id0 + e);
  int32_t* st = state + (int64_t)e * BRK_WORDS;
  BrkWorld w;
  WorldCount c = {0u, 0, 0, 0, 0};
  if (!REPEAT) {
    frame_skip = 1;
    sticky_num = 0;
    sticky_den = 1;
  }
  if (STEP) {
    brk_load(st, w, c);
    bool over;
    int over_rew;
    const int r = brk_agent_step(w, c, world_action<4>(actions, act_stride, action_shift, e), seed, env, lives, max_episode_steps,
                                 frame_skip, sticky_num, sticky_den, over, over_rew);
    if (lane == 0) brk_publish(e, r, over, over_rew, rew, done, reset, ep_count, ep_rew_sum);
  } else {
    brk_new_episode(w, seed, env, lives, c.draws, c.ep_steps);
  }
  brk_store(st, w, c, lane);
  brk_write_frame(w, frames + (int64_t)e * frame_ld, nullptr, lane, 64);
}

// a2c_breakout_step_post: breakout_kernel<true> + the step's bookkeeping + the frame stack, WORLD_POST_WAVES waves per env.
// Every wave loads the state words and computes the same agent step; the barrier keeps wave 0's stores behind every wave's loads.
template <bool REPEAT>
__global__ __launch_bounds__(WORLD_POST_THREADS) void breakout_post_kernel(
    int32_t* __restrict__ state, const int64_t* __restrict__ actions, int64_t act_stride, int action_shift, int env_id0,
    uint32_t seed, int lives, int max_episode_steps, int frame_skip, int sticky_num, int sticky_den,
    float* __restrict__ frames, int64_t frame_ld, float* __restrict__ rew, float* __restrict__ done, float* __restrict__ reset, int32_t* __restrict__ ep_count, int32_t* __restrict__ ep_rew_sum,
    const a2c_world_post post) {
  if (!REPEAT) {
    frame_skip = 1;
    sticky_num = 0;
    sticky_den = 1;
  }
  const int e = blockIdx.x, tid = threadIdx.x;
  const uint32_t env = (uint32_t)(env_id0 + e);
  int32_t* st = state + (int64_t)e * BRK_WORDS;
  BrkWorld w;
  WorldCount c;
  brk_load(st, w, c);
  const int a = world_action<4>(actions, act_stride, action_shift, e);
  __syncthreads();
  bool over;
  int over_rew;
  const int r = brk_agent_step(w, c, a, seed, env, lives, max_episode_steps, frame_skip, sticky_num, sticky_den, over, over_rew);
  const float d = world_post_done(post, (float)r, over ? 1.0f : 0.0f);
  if (tid == 0) {
    brk_publish(e, r, over, over_rew, rew, done, reset, ep_count, ep_rew_sum);
    world_post_book(post, e, (float)r, d);
  }
  if (tid < 64) brk_store(st, w, c, tid);
  float* top = world_post_planes(post, e, d, over, BRK_HW, tid);
  brk_write_frame(w, top, frames == nullptr ? nullptr : frames + (int64_t)e * frame_ld, tid, WORLD_POST_THREADS);
}

bool brk_world_ok(int lives, int max_episode_steps) {
  return lives >= 1 && lives <= MAX_LIVES && max_episode_steps >= 1 && max_episode_steps <= MAX_EPISODE_STEPS;
}

}  // namespace
