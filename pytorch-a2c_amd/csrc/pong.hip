// Pong worlds in device memory: a2c_pong_reset / a2c_pong_step / a2c_pong_step_post and their _skip forms (rules: DESIGN.md
// sections 6c and 6g; host twin: a2c_amd/pong.py).
//
// One wavefront per env.  The state of an env is PONG_WORDS int32 words in HBM; an agent step is frame_skip (1..8) game
// frames, each a short, loop-free, wave-uniform integer computation (every lane computes the same values from the same
// words; the loop over the frames and its break at an episode end are wave-uniform too), after which lanes 0..PONG_WORDS-1 store
// one word each and all 64 lanes render the 80 x 80 prepped frame row (1 on the two paddles and the ball, 0 elsewhere)
// as 16-byte stores where the frame-stack kernels read it.  The draw, step and episode-step counters are part of the
// state the kernel advances, so a captured launch plays NEW steps at every replay.
#include "a2c_common.h"
#include "pong_rng.h"

namespace {

constexpr int PONG_WORDS = 16;      // agent y, opponent y, ball x, ball y, vx, vy, agent score, opponent score, draws, steps,
                                    // episode steps, reward since the last done, the action of the previous game frame
                                    // (sticky actions; 0 without them), 3 spare
constexpr int PW = 80, PH = 80, PONG_HW = PW * PH;
constexpr int PADDLE_H = 8, PADDLE_W = 2, BALL = 2;
constexpr int OPP_X = 8, AGENT_X = 70;
constexpr int PADDLE_MAX_Y = PH - PADDLE_H, BALL_MAX_Y = PH - BALL;
constexpr int PADDLE_START_Y = 36, SERVE_X = 39, SERVE_Y = 39;
constexpr int MISS_RIGHT = AGENT_X + PADDLE_W, MISS_LEFT = OPP_X - BALL;
constexpr int MAX_POINTS = 21, MAX_EPISODE_STEPS = 1 << 24, MAX_SKILL_DEN = 1 << 16;
constexpr int MAX_FRAME_SKIP = 8, MAX_STICKY_DEN = 1 << 16;

struct PongWorld {
  int ay, oy, bx, by, vx, vy, sa, so;
};

__device__ __forceinline__ int pong_clamp(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }
// the hit table: off = ball y + 1 - paddle y in 0..8 -> vy = {-2,-2,-1,-1,0,1,1,2,2}[off], |vx| = {2,2,1,1,1,1,1,2,2}[off]
__device__ __forceinline__ int pong_hit_vy(int off) { return off <= 1 ? -2 : (off <= 3 ? -1 : (off == 4 ? 0 : (off <= 6 ? 1 : 2))); }
__device__ __forceinline__ int pong_hit_speed(int off) { return (off <= 1 || off >= 7) ? 2 : 1; }

__device__ __forceinline__ void pong_serve(PongWorld& w, uint32_t d, bool towards_agent) {
  w.bx = SERVE_X; w.by = SERVE_Y;
  w.vx = towards_agent ? 1 : -1;
  w.vy = (int)((d >> 1) % 5u) - 2;
}

__device__ __forceinline__ void pong_new_episode(PongWorld& w, uint32_t seed, uint32_t env, uint32_t& draws, int& ep_steps) {
  w.ay = w.oy = PADDLE_START_Y;
  w.sa = w.so = 0;
  ep_steps = 0;
  const uint32_t d = pong_hash(seed, env, draws++);
  pong_serve(w, d, (d & 1u) != 0u);
}

__device__ __forceinline__ bool pong_in(int x, int y, int rx, int ry, int rw, int rh) {
  return x >= rx && x < rx + rw && y >= ry && y < ry + rh;
}

// the prepped frame row: PONG_HW floats as float4 stores, 4 pixels of one row each (PW % 4 == 0), by `nthreads` lanes, to
// `frame` and / or `frame2` (either may be null)
__device__ __forceinline__ void pong_write_frame(const PongWorld& w, float* __restrict__ frame, float* __restrict__ frame2,
                                                 int tid, int nthreads) {
  float4* f4 = reinterpret_cast<float4*>(frame);
  float4* g4 = reinterpret_cast<float4*>(frame2);
  for (int q = tid; q < PONG_HW / 4; q += nthreads) {
    const int y = q / (PW / 4), x0 = 4 * (q - y * (PW / 4));
    float v[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int x = x0 + j;
      const bool on = pong_in(x, y, OPP_X, w.oy, PADDLE_W, PADDLE_H) || pong_in(x, y, AGENT_X, w.ay, PADDLE_W, PADDLE_H) ||
                      pong_in(x, y, w.bx, w.by, BALL, BALL);
      v[j] = on ? 1.0f : 0.0f;
    }
    if (f4 != nullptr) f4[q] = make_float4(v[0], v[1], v[2], v[3]);
    if (g4 != nullptr) g4[q] = make_float4(v[0], v[1], v[2], v[3]);
  }
}

// the counters of an env beside its world
struct PongCount {
  uint32_t draws;
  int steps, ep_steps, ep_rew, prev;
};

__device__ __forceinline__ void pong_load(const int32_t* st, PongWorld& w, PongCount& c) {
  w.ay = st[0]; w.oy = st[1]; w.bx = st[2]; w.by = st[3]; w.vx = st[4]; w.vy = st[5]; w.sa = st[6]; w.so = st[7];
  c.draws = (uint32_t)st[8]; c.steps = st[9]; c.ep_steps = st[10]; c.ep_rew = st[11]; c.prev = st[12];
}

__device__ __forceinline__ void pong_store(int32_t* st, const PongWorld& w, const PongCount& c, int lane) {
  if (lane < PONG_WORDS) {
    const int hv = lane == 0 ? w.ay : lane == 1 ? w.oy : lane == 2 ? w.bx : lane == 3 ? w.by : lane == 4 ? w.vx
                 : lane == 5 ? w.vy : lane == 6 ? w.sa : lane == 7 ? w.so : lane == 8 ? (int)c.draws : lane == 9 ? c.steps
                 : lane == 10 ? c.ep_steps : lane == 11 ? c.ep_rew : lane == 12 ? c.prev : 0;
    st[lane] = hv;
  }
}

// One game frame of one world, in registers (wave-uniform; no memory access).  -> the reward; over: the episode ended and
// the world has been restarted
__device__ __forceinline__ int pong_advance(PongWorld& w, PongCount& c, int a, uint32_t seed, uint32_t env, int points_to_win,
                                            int max_episode_steps, int skill_num, int skill_den, bool& over) {
  ++c.steps;
  ++c.ep_steps;
  // 1. the agent's paddle
  w.ay = pong_clamp(w.ay + (a == 1 ? -2 : (a == 2 ? 2 : 0)), 0, PADDLE_MAX_Y);
  // 2. the opponent's paddle: towards the ball's centre, on the steps the draw allows
  if ((int)(pong_hash(seed, env, c.draws++) % (uint32_t)skill_den) < skill_num) {
    const int cb = w.by + 1, cp = w.oy + PADDLE_H / 2;
    w.oy = pong_clamp(w.oy + (cb < cp ? -1 : (cb > cp ? 1 : 0)), 0, PADDLE_MAX_Y);
  }
  // 3. the ball, the walls
  const int x0 = w.bx;
  int x = x0 + w.vx, y = w.by + w.vy;
  if (y < 0) { y = -y; w.vy = -w.vy; }
  else if (y > BALL_MAX_Y) { y = 2 * BALL_MAX_Y - y; w.vy = -w.vy; }
  // 4. the paddles
  if (w.vx > 0 && x0 + 1 < AGENT_X && x + 1 >= AGENT_X && y >= w.ay - 1 && y <= w.ay + PADDLE_H - 1) {
    const int off = y + 1 - w.ay;
    x = AGENT_X - BALL; w.vx = -pong_hit_speed(off); w.vy = pong_hit_vy(off);
  } else if (w.vx < 0 && x0 > OPP_X + 1 && x <= OPP_X + 1 && y >= w.oy - 1 && y <= w.oy + PADDLE_H - 1) {
    const int off = y + 1 - w.oy;
    x = OPP_X + PADDLE_W; w.vx = pong_hit_speed(off); w.vy = pong_hit_vy(off);
  }
  w.bx = x; w.by = y;
  // 5. a point
  int r = 0;
  if (x >= MISS_RIGHT) { r = -1; ++w.so; }
  else if (x <= MISS_LEFT) { r = 1; ++w.sa; }
  // 6. the end of the episode, or the serve
  over = w.sa >= points_to_win || w.so >= points_to_win || c.ep_steps >= max_episode_steps;
  if (over) pong_new_episode(w, seed, env, c.draws, c.ep_steps);
  else if (r != 0) pong_serve(w, pong_hash(seed, env, c.draws++), r < 0);
  return r;
}

// One agent step: frame_skip game frames with action a, each keeping the previous frame's action when its sticky draw (taken
// BEFORE the frame's own draws; none with sticky_num == 0) mod sticky_den is below sticky_num; an episode end drops the
// remaining frames.  -> the summed reward; over: as pong_advance; closed: the `done` of a "Pong" env type (runner.py:212-214);
// closed_rew: the reward since the last done, what a closed step adds to ep_rew_sum
__device__ __forceinline__ int pong_agent_step(PongWorld& w, PongCount& c, int a, uint32_t seed, uint32_t env, int points_to_win,
                                               int max_episode_steps, int skill_num, int skill_den, int frame_skip,
                                               int sticky_num, int sticky_den, bool& over, bool& closed, int& closed_rew) {
  int R = 0;
  over = false;
  for (int s = 0; s < frame_skip; ++s) {
    int x = a;
    if (sticky_num > 0) {
      if ((int)(pong_hash(seed, env, c.draws++) % (uint32_t)sticky_den) < sticky_num) x = c.prev;
      c.prev = x;
    }
    R += pong_advance(w, c, x, seed, env, points_to_win, max_episode_steps, skill_num, skill_den, over);
    if (over) {
      c.prev = 0;
      break;
    }
  }
  closed = over || R != 0;
  c.ep_rew += R;
  closed_rew = c.ep_rew;
  if (closed) c.ep_rew = 0;
  return R;
}

__device__ __forceinline__ int pong_action(const int64_t* actions, int64_t act_stride, int action_shift, int e) {
  const int64_t a64 = (actions[(int64_t)e * act_stride] + (int64_t)action_shift) % 3;
  return (int)(a64 < 0 ? a64 + 3 : a64);
}

// lane 0 of the wave that owns the env: what a step leaves beside the state words
__device__ __forceinline__ void pong_publish(int e, int r, bool over, bool closed, int closed_rew, float* rew, float* done,
                                             float* reset, int32_t* ep_count, int32_t* ep_rew_sum) {
  if (closed) {
    if (ep_count != nullptr) atomicAdd(ep_count, 1);
    if (ep_rew_sum != nullptr) atomicAdd(ep_rew_sum, closed_rew);
  }
  rew[e] = (float)r;
  done[e] = closed ? 1.0f : 0.0f;
  reset[e] = over ? 1.0f : 0.0f;
}

// REPEAT == false is the (1, 0, .) world with its constants folded: one game frame, no loop, no sticky draw -- the kernel of
// a2c_pong_step as it was before frame skip (the loop with frame_skip = 1 at run time cost 0.15-0.35 us)
template <bool STEP, bool REPEAT>
__global__ __launch_bounds__(64) void pong_kernel(int32_t* __restrict__ state, const int64_t* __restrict__ actions,
                                                  int64_t act_stride, int action_shift, int env_id0, uint32_t seed,
                                                  int points_to_win, int max_episode_steps, int skill_num, int skill_den,
                                                  int frame_skip, int sticky_num, int sticky_den,
                                                  float* __restrict__ frames, int64_t frame_ld, float* __restrict__ rew,
                                                  float* __restrict__ done, float* __restrict__ reset,
                                                  int32_t* __restrict__ ep_count, int32_t* __restrict__ ep_rew_sum) {
  const int e = blockIdx.x, lane = threadIdx.x;
  const uint32_t env = (uint32_t)(env_id0 + e);
  int32_t* st = state + (int64_t)e * PONG_WORDS;
  PongWorld w;
  PongCount c = {0u, 0, 0, 0, 0};
  if (!REPEAT) {
    frame_skip = 1;
    sticky_num = 0;
    sticky_den = 1;
  }
  if (STEP) {
    pong_load(st, w, c);
    bool over, closed;
    int closed_rew;
    const int r = pong_agent_step(w, c, pong_action(actions, act_stride, action_shift, e), seed, env, points_to_win,
                                  max_episode_steps, skill_num, skill_den, frame_skip, sticky_num, sticky_den, over, closed,
                                  closed_rew);
    if (lane == 0) pong_publish(e, r, over, closed, closed_rew, rew, done, reset, ep_count, ep_rew_sum);
  } else {
    pong_new_episode(w, seed, env, c.draws, c.ep_steps);
  }
  pong_store(st, w, c, lane);
  pong_write_frame(w, frames + (int64_t)e * frame_ld, nullptr, lane, 64);
}

// a2c_pong_step_post: pong_kernel<true> + the step's bookkeeping + the frame stack, WORLD_POST_WAVES waves per env.  Every
// wave loads the state words and computes the same agent step; the barrier keeps wave 0's stores behind every wave's loads.
template <bool REPEAT>
__global__ __launch_bounds__(WORLD_POST_THREADS) void pong_post_kernel(
    int32_t* __restrict__ state, const int64_t* __restrict__ actions, int64_t act_stride, int action_shift, int env_id0,
    uint32_t seed, int points_to_win, int max_episode_steps, int skill_num, int skill_den, int frame_skip, int sticky_num,
    int sticky_den, float* __restrict__ frames, int64_t frame_ld, float* __restrict__ rew, float* __restrict__ done, float* __restrict__ reset,
    int32_t* __restrict__ ep_count, int32_t* __restrict__ ep_rew_sum, const a2c_world_post post) {
  if (!REPEAT) {
    frame_skip = 1;
    sticky_num = 0;
    sticky_den = 1;
  }
  const int e = blockIdx.x, tid = threadIdx.x;
  const uint32_t env = (uint32_t)(env_id0 + e);
  int32_t* st = state + (int64_t)e * PONG_WORDS;
  PongWorld w;
  PongCount c;
  pong_load(st, w, c);
  const int a = pong_action(actions, act_stride, action_shift, e);
  __syncthreads();
  bool over, closed;
  int closed_rew;
  const int r = pong_agent_step(w, c, a, seed, env, points_to_win, max_episode_steps, skill_num, skill_den, frame_skip,
                                sticky_num, sticky_den, over, closed, closed_rew);
  const float d = world_post_done(post, (float)r, closed ? 1.0f : 0.0f);
  if (tid == 0) {
    pong_publish(e, r, over, closed, closed_rew, rew, done, reset, ep_count, ep_rew_sum);
    world_post_book(post, e, (float)r, d);
  }
  if (tid < 64) pong_store(st, w, c, tid);
  float* top = world_post_planes(post, e, d, over, PONG_HW, tid);
  pong_write_frame(w, top, frames == nullptr ? nullptr : frames + (int64_t)e * frame_ld, tid, WORLD_POST_THREADS);
}

bool pong_world_ok(int points_to_win, int max_episode_steps, int skill_num, int skill_den) {
  return points_to_win >= 1 && points_to_win <= MAX_POINTS && max_episode_steps >= 1 && max_episode_steps <= MAX_EPISODE_STEPS &&
         skill_den >= 1 && skill_den <= MAX_SKILL_DEN && skill_num >= 0 && skill_num <= skill_den;
}

bool pong_repeat_ok(int frame_skip, int sticky_num, int sticky_den) {
  return frame_skip >= 1 && frame_skip <= MAX_FRAME_SKIP && sticky_den >= 1 && sticky_den <= MAX_STICKY_DEN && sticky_num >= 0 &&
         sticky_num <= sticky_den;
}

bool pong_frames_ok(const float* frames, int64_t frame_ld) {
  return frames != nullptr && ((uintptr_t)frames & 15u) == 0 && frame_ld >= PONG_HW && frame_ld % 4 == 0;
}

}  // namespace

extern "C" size_t a2c_pong_state_bytes(int points_to_win) {
  if (points_to_win < 1 || points_to_win > MAX_POINTS) return 0;
  return sizeof(int32_t) * (size_t)PONG_WORDS;
}

extern "C" int a2c_pong_reset(int32_t* state, int B, int env_id0, uint32_t seed, int points_to_win, int max_episode_steps,
                              int opp_skill_num, int opp_skill_den, float* frames, int64_t frame_ld, a2c_stream_t stream) {
  if (B <= 0 || env_id0 < 0 || !pong_world_ok(points_to_win, max_episode_steps, opp_skill_num, opp_skill_den))
    return A2C_ERR_ARG;
  if (state == nullptr || !pong_frames_ok(frames, frame_ld)) return A2C_ERR_ARG;
  hipLaunchKernelGGL((pong_kernel<false, false>), dim3(B), dim3(64), 0, a2c_s(stream), state, (const int64_t*)nullptr, (int64_t)0, 0,
                     env_id0, seed, points_to_win, max_episode_steps, opp_skill_num, opp_skill_den, 1, 0, 1, frames, frame_ld,
                     (float*)nullptr, (float*)nullptr, (float*)nullptr, (int32_t*)nullptr, (int32_t*)nullptr);
  A2C_CHECK_LAUNCH();
  return A2C_OK;
}

extern "C" int a2c_pong_step_skip(int32_t* state, const int64_t* actions, int64_t act_stride, int action_shift, int B,
                                  int env_id0, uint32_t seed, int points_to_win, int max_episode_steps, int opp_skill_num,
                                  int opp_skill_den, float* frames, int64_t frame_ld, float* rew, float* done, float* reset,
                                  int32_t* ep_count, int32_t* ep_rew_sum, int frame_skip, int sticky_num, int sticky_den,
                                  a2c_stream_t stream) {
  if (B <= 0 || env_id0 < 0 || act_stride < 0 || !pong_world_ok(points_to_win, max_episode_steps, opp_skill_num, opp_skill_den) ||
      !pong_repeat_ok(frame_skip, sticky_num, sticky_den))
    return A2C_ERR_ARG;
  if (state == nullptr || actions == nullptr || rew == nullptr || done == nullptr || reset == nullptr ||
      !pong_frames_ok(frames, frame_ld))
    return A2C_ERR_ARG;
  const auto kernel = (frame_skip == 1 && sticky_num == 0) ? pong_kernel<true, false> : pong_kernel<true, true>;
  hipLaunchKernelGGL(kernel, dim3(B), dim3(64), 0, a2c_s(stream), state, actions, act_stride, action_shift, env_id0,
                     seed, points_to_win, max_episode_steps, opp_skill_num, opp_skill_den, frame_skip, sticky_num, sticky_den,
                     frames, frame_ld, rew, done, reset, ep_count, ep_rew_sum);
  A2C_CHECK_LAUNCH();
  return A2C_OK;
}

extern "C" int a2c_pong_step(int32_t* state, const int64_t* actions, int64_t act_stride, int action_shift, int B, int env_id0,
                             uint32_t seed, int points_to_win, int max_episode_steps, int opp_skill_num, int opp_skill_den,
                             float* frames, int64_t frame_ld, float* rew, float* done, float* reset, int32_t* ep_count,
                             int32_t* ep_rew_sum, a2c_stream_t stream) {
  return a2c_pong_step_skip(state, actions, act_stride, action_shift, B, env_id0, seed, points_to_win, max_episode_steps,
                            opp_skill_num, opp_skill_den, frames, frame_ld, rew, done, reset, ep_count, ep_rew_sum, 1, 0, 1,
                            stream);
}

extern "C" int a2c_pong_step_post_skip(int32_t* state, const int64_t* actions, int64_t act_stride, int action_shift, int B,
                                       int env_id0, uint32_t seed, int points_to_win, int max_episode_steps, int opp_skill_num,
                                       int opp_skill_den, float* frames, int64_t frame_ld, float* rew, float* done,
                                       float* reset, int32_t* ep_count, int32_t* ep_rew_sum, int frame_skip, int sticky_num,
                                       int sticky_den, const a2c_world_post* post, a2c_stream_t stream) {
  if (B <= 0 || env_id0 < 0 || act_stride < 0 || !pong_world_ok(points_to_win, max_episode_steps, opp_skill_num, opp_skill_den) ||
      !pong_repeat_ok(frame_skip, sticky_num, sticky_den))
    return A2C_ERR_ARG;
  if (state == nullptr || actions == nullptr || rew == nullptr || done == nullptr || reset == nullptr ||
      (frames != nullptr && !pong_frames_ok(frames, frame_ld)) || !a2c_world_post_ok(post, PONG_HW))
    return A2C_ERR_ARG;
  const auto kernel = (frame_skip == 1 && sticky_num == 0) ? pong_post_kernel<false> : pong_post_kernel<true>;
  hipLaunchKernelGGL(kernel, dim3(B), dim3(WORLD_POST_THREADS), 0, a2c_s(stream), state, actions, act_stride,
                     action_shift, env_id0, seed, points_to_win, max_episode_steps, opp_skill_num, opp_skill_den, frame_skip,
                     sticky_num, sticky_den, frames, frame_ld, rew, done, reset, ep_count, ep_rew_sum, *post);
  A2C_CHECK_LAUNCH();
  return A2C_OK;
}

extern "C" int a2c_pong_step_post(int32_t* state, const int64_t* actions, int64_t act_stride, int action_shift, int B,
                                  int env_id0, uint32_t seed, int points_to_win, int max_episode_steps, int opp_skill_num,
                                  int opp_skill_den, float* frames, int64_t frame_ld, float* rew, float* done, float* reset,
                                  int32_t* ep_count, int32_t* ep_rew_sum, const a2c_world_post* post, a2c_stream_t stream) {
  return a2c_pong_step_post_skip(state, actions, act_stride, action_shift, B, env_id0, seed, points_to_win, max_episode_steps,
                                 opp_skill_num, opp_skill_den, frames, frame_ld, rew, done, reset, ep_count, ep_rew_sum, 1, 0,
                                 1, post, stream);
}
