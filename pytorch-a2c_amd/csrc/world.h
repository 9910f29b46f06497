// What the worlds in device memory share (snake.hip, pong.hip, breakout.hip; not part of the C ABI): the counter-based draws,
// the a2c_<world>_step_post helpers, and the scaffold of the worlds whose state fits in registers: counters, the frame-skip /
// sticky-action loop, the kernels and their launchers, written once over a game type G (DESIGN.md sections 6h and 6i; Pong runs
// on it, Breakout uses the counters and small helpers and keeps kernels of its own, breakout.hip says why).  A game G supplies
//   WORDS, HW, N_ACTIONS                  int32 state words per env, floats of one frame, actions
//   World, Params, params_ok(Params)      the world in registers; its parameters, plain data, ONE kernel argument
//   load, store, new_episode              state words <-> registers (store: lane i writes word i); reset + first serve
//   frame(w, c, a, gp, seed, env, over, end)   one game frame in registers -> its reward; over: the episode ended, world
//                                         restarted; end: a WorldNoEnd / WorldEnd (below; the picture worlds report nothing)
//   write_frame(w, f, f2, tid, n)         the prepped frame as 16-byte stores by n lanes to f and / or f2 (either may be null)
//   closes(over, R)                       the `done` of an agent step with summed reward R
// The Snake worlds keep kernels of their own (cells in LDS, a cooperative step) and use the first two parts only.
#pragma once
#include "a2c_common.h"

// ---- draws: draw i of env e is world_hash(seed, e, i) (host side: a2c_amd.worlds.hash32).  No state
// besides the counter.
__device__ __forceinline__ uint32_t world_fin(uint32_t x) {       // lowbias32
  x ^= x >> 16; x *= 0x7FEB352Du; x ^= x >> 15; x *= 0x846CA68Bu; x ^= x >> 16;
  return x;
}
__device__ __forceinline__ uint32_t world_hash(uint32_t seed, uint32_t env, uint32_t draw) {
  return world_fin(world_fin(world_fin(seed + 0x9E3779B9u) ^ env) ^ draw);
}

// ---- a2c_<world>_step_post: what the three fused world kernels share.
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

// ---- the scaffold of the register worlds.  One wavefront per env; an agent step is frame_skip (1..8) game frames, each a
// short, loop-free, wave-uniform integer computation (every lane computes the same values from the same words; the loop over
// the frames and its break at an episode end are wave-uniform too), after which lanes 0..WORDS-1 store one word each and all
// lanes render the frame.  The draw, step and episode-step counters are part of the state the kernel advances, so a captured
// launch plays NEW steps at every replay.
constexpr int WORLD_MAX_FRAME_SKIP = 8, WORLD_MAX_STICKY_DEN = 1 << 16;

// the counters of an env beside its world: draws taken, game frames played (in all, in this episode), the reward since the
// last done, the action of the previous game frame (sticky actions; 0 without them)
struct WorldCount {
  uint32_t draws;
  int steps, ep_steps, ep_rew, prev;
};

__device__ __forceinline__ int world_clamp(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// What G::frame hands back about the frame that ENDS an episode, before it restarts the world (time-limit truncation,
// DESIGN.md section 6o): frame calls end.keep(w, limit_alone) with the world as the frame's physics left it; limit_alone: the
// step limit ended the episode and the game's own end condition did not hold at that frame.  WorldNoEnd is the caller that
// asks for nothing: every existing kernel, whose code it leaves as it was.  WorldEnd<World> keeps both in registers.
struct WorldNoEnd {
  template <typename W>
  __device__ __forceinline__ void keep(const W&, bool) {}
};
template <typename W>
struct WorldEnd {
  W w;
  bool limit_alone;
  __device__ __forceinline__ void keep(const W& x, bool l) { w = x; limit_alone = l; }
};

template <int N>
__device__ __forceinline__ int world_action(const int64_t* actions, int64_t act_stride, int action_shift, int e) {
  const int64_t a64 = (actions[(int64_t)e * act_stride] + (int64_t)action_shift) % N;
  return (int)(a64 < 0 ? a64 + N : a64);
}

static inline bool world_repeat_ok(int frame_skip, int sticky_num, int sticky_den) {
  return frame_skip >= 1 && frame_skip <= WORLD_MAX_FRAME_SKIP && sticky_den >= 1 && sticky_den <= WORLD_MAX_STICKY_DEN &&
         sticky_num >= 0 && sticky_num <= sticky_den;
}

static inline bool world_frames_ok(const float* frames, int64_t frame_ld, int HW) {
  return frames != nullptr && ((uintptr_t)frames & 15u) == 0 && frame_ld >= HW && frame_ld % 4 == 0;
}

// One agent step: frame_skip game frames with action a, each keeping the previous frame's action when its sticky draw (taken
// BEFORE the frame's own draws; none with sticky_num == 0) mod sticky_den is below sticky_num; an episode end drops the
// remaining frames.  -> the summed reward R; over: as G::frame; closed = G::closes(over, R): the step's `done`; closed_rew:
// the reward since the last done, what a closed step adds to ep_rew_sum.
// The reward is booked once per agent step.  Where only an episode end closes (real dones only) this equals booking every game
// frame and zeroing at the over: the loop breaks at the frame that ends the episode, so the sum at the over is the old
// ep_rew + R, and the word left behind is 0 after an over and the old ep_rew + R otherwise.
// end: a WorldNoEnd or a WorldEnd (above); the frame that ends the episode fills it.
template <typename G, typename E>
__device__ __forceinline__ int world_agent_step(typename G::World& w, WorldCount& c, int a, const typename G::Params& gp,
                                                uint32_t seed, uint32_t env, int frame_skip, int sticky_num, int sticky_den,
                                                bool& over, bool& closed, int& closed_rew, E& end) {
  int R = 0;
  over = false;
  for (int s = 0; s < frame_skip; ++s) {
    int x = a;
    if (sticky_num > 0) {
      if ((int)(world_hash(seed, env, c.draws++) % (uint32_t)sticky_den) < sticky_num) x = c.prev;
      c.prev = x;
    }
    R += G::frame(w, c, x, gp, seed, env, over, end);
    if (over) {
      c.prev = 0;
      break;
    }
  }
  closed = G::closes(over, R);
  c.ep_rew += R;
  closed_rew = c.ep_rew;
  if (closed) c.ep_rew = 0;
  return R;
}

template <typename G>
__device__ __forceinline__ int world_agent_step(typename G::World& w, WorldCount& c, int a, const typename G::Params& gp,
                                                uint32_t seed, uint32_t env, int frame_skip, int sticky_num, int sticky_den,
                                                bool& over, bool& closed, int& closed_rew) {
  WorldNoEnd none;
  return world_agent_step<G>(w, c, a, gp, seed, env, frame_skip, sticky_num, sticky_den, over, closed, closed_rew, none);
}

// lane 0 of the wave that owns the env: what a step leaves beside the state words
__device__ __forceinline__ void world_publish(int e, int r, bool over, bool closed, int closed_rew, float* rew, float* done,
                                              float* reset, int32_t* ep_count, int32_t* ep_rew_sum) {
  if (closed) {
    if (ep_count != nullptr) atomicAdd(ep_count, 1);
    if (ep_rew_sum != nullptr) atomicAdd(ep_rew_sum, closed_rew);
  }
  rew[e] = (float)r;
  done[e] = closed ? 1.0f : 0.0f;
  reset[e] = over ? 1.0f : 0.0f;
}

// a2c_<world>_reset (STEP == false) and a2c_<world>_step[_skip].  REPEAT == false is the (1, 0, .) world with its constants
// folded: one game frame, no loop, no sticky draw -- the step kernel as it was before frame skip (the
// loop with frame_skip = 1 at run time cost 0.15-0.35 us)
template <typename G, bool STEP, bool REPEAT>
__global__ __launch_bounds__(64) void world_kernel(int32_t* __restrict__ state, const int64_t* __restrict__ actions,
                                                   int64_t act_stride, int action_shift, int env_id0, uint32_t seed,
                                                   const typename G::Params gp, int frame_skip, int sticky_num, int sticky_den,
                                                   float* __restrict__ frames, int64_t frame_ld, float* __restrict__ rew,
                                                   float* __restrict__ done, float* __restrict__ reset,
                                                   int32_t* __restrict__ ep_count, int32_t* __restrict__ ep_rew_sum) {
  const int e = blockIdx.x, lane = threadIdx.x;
  const uint32_t env = (uint32_t)(env_id0 + e);
  int32_t* st = state + (int64_t)e * G::WORDS;
  typename G::World w;
  WorldCount c = {0u, 0, 0, 0, 0};
  if (!REPEAT) {
    frame_skip = 1;
    sticky_num = 0;
    sticky_den = 1;
  }
  if (STEP) {
    G::load(st, w, c);
    bool over, closed;
    int closed_rew;
    const int r = world_agent_step<G>(w, c, world_action<G::N_ACTIONS>(actions, act_stride, action_shift, e), gp, seed, env,
                                      frame_skip, sticky_num, sticky_den, over, closed, closed_rew);
    if (lane == 0) world_publish(e, r, over, closed, closed_rew, rew, done, reset, ep_count, ep_rew_sum);
  } else {
    G::new_episode(w, c, gp, seed, env);
  }
  G::store(st, w, c, lane);
  G::write_frame(w, frames + (int64_t)e * frame_ld, nullptr, lane, 64);
}

// a2c_<world>_step_post[_skip]: world_kernel<G, true, .> + the step's bookkeeping + the frame stack, WORLD_POST_WAVES waves
// per env.  Every wave loads the state words and computes the same agent step; the barrier keeps wave 0's stores behind every
// wave's loads.
template <typename G, bool REPEAT>
__global__ __launch_bounds__(WORLD_POST_THREADS) void world_post_kernel(
    int32_t* __restrict__ state, const int64_t* __restrict__ actions, int64_t act_stride, int action_shift, int env_id0,
    uint32_t seed, const typename G::Params gp, int frame_skip, int sticky_num, int sticky_den, float* __restrict__ frames,
    int64_t frame_ld, float* __restrict__ rew, float* __restrict__ done, float* __restrict__ reset,
    int32_t* __restrict__ ep_count, int32_t* __restrict__ ep_rew_sum, const a2c_world_post post) {
  if (!REPEAT) {
    frame_skip = 1;
    sticky_num = 0;
    sticky_den = 1;
  }
  const int e = blockIdx.x, tid = threadIdx.x;
  const uint32_t env = (uint32_t)(env_id0 + e);
  int32_t* st = state + (int64_t)e * G::WORDS;
  typename G::World w;
  WorldCount c;
  G::load(st, w, c);
  const int a = world_action<G::N_ACTIONS>(actions, act_stride, action_shift, e);
  __syncthreads();
  bool over, closed;
  int closed_rew;
  const int r = world_agent_step<G>(w, c, a, gp, seed, env, frame_skip, sticky_num, sticky_den, over, closed, closed_rew);
  const float d = world_post_done(post, (float)r, closed ? 1.0f : 0.0f);
  if (tid == 0) {
    world_publish(e, r, over, closed, closed_rew, rew, done, reset, ep_count, ep_rew_sum);
    world_post_book(post, e, (float)r, d);
  }
  if (tid < 64) G::store(st, w, c, tid);
  float* top = world_post_planes(post, e, d, over, G::HW, tid);
  G::write_frame(w, top, frames == nullptr ? nullptr : frames + (int64_t)e * frame_ld, tid, WORLD_POST_THREADS);
}

// ---- a2c_<world>_step_rules: the agent step whose number of game frames is drawn.
// The checks of an a2c_world_rules block; flags: the world has episodic_life / clip_rewards (Breakout)
static inline bool world_rules_ok(const a2c_world_rules* r, bool flags) {
  if (r == nullptr || !world_repeat_ok(r->frame_skip, r->sticky_num, r->sticky_den)) return false;
  if (r->frame_skip_max < r->frame_skip || r->frame_skip_max > WORLD_MAX_FRAME_SKIP) return false;
  if ((r->episodic_life | r->clip_rewards) & ~1) return false;
  return flags || (r->episodic_life | r->clip_rewards) == 0;
}

// a block that asks for nothing new: the step is a2c_<world>_step[_post]_skip
static inline bool world_rules_plain(const a2c_world_rules& r) {
  return r.frame_skip_max == r.frame_skip && r.episodic_life == 0 && r.clip_rewards == 0;
}

// the game frames of this agent step: with frame_skip_max > frame_skip ONE draw, taken before the step's first sticky draw
__device__ __forceinline__ int world_draw_skip(WorldCount& c, uint32_t seed, uint32_t env, const a2c_world_rules& r) {
  if (r.frame_skip_max <= r.frame_skip) return r.frame_skip;
  return r.frame_skip + (int)(world_hash(seed, env, c.draws++) % (uint32_t)(r.frame_skip_max - r.frame_skip + 1));
}

// The third instantiation beside REPEAT == false / true, as a kernel of its own that a game instantiates in a file of its
// own (pong_rules.hip), so that those two stay what and where they were in their code object, to the byte (DESIGN.md section
// 6i): world_kernel<G, true, true> (POST == false; `post` is not read) and world_post_kernel<G, true> (POST == true) with the
// k-draw in front of the agent step.  k lives in registers only; every wave of the POST form draws the same k.
template <typename G, bool POST>
__global__ __launch_bounds__(POST ? WORLD_POST_THREADS : 64) void world_rules_kernel(
    int32_t* __restrict__ state, const int64_t* __restrict__ actions, int64_t act_stride, int action_shift, int env_id0,
    uint32_t seed, const typename G::Params gp, const a2c_world_rules rules, float* __restrict__ frames, int64_t frame_ld,
    float* __restrict__ rew, float* __restrict__ done, float* __restrict__ reset, int32_t* __restrict__ ep_count,
    int32_t* __restrict__ ep_rew_sum, const a2c_world_post post) {
  const int e = blockIdx.x, tid = threadIdx.x;
  const uint32_t env = (uint32_t)(env_id0 + e);
  int32_t* st = state + (int64_t)e * G::WORDS;
  typename G::World w;
  WorldCount c;
  G::load(st, w, c);
  const int a = world_action<G::N_ACTIONS>(actions, act_stride, action_shift, e);
  if (POST) __syncthreads();
  bool over, closed;
  int closed_rew;
  const int k = world_draw_skip(c, seed, env, rules);
  const int r = world_agent_step<G>(w, c, a, gp, seed, env, k, rules.sticky_num, rules.sticky_den, over, closed, closed_rew);
  if (tid == 0) world_publish(e, r, over, closed, closed_rew, rew, done, reset, ep_count, ep_rew_sum);
  if (tid < 64) G::store(st, w, c, tid);
  if (POST) {
    const float d = world_post_done(post, (float)r, closed ? 1.0f : 0.0f);
    if (tid == 0) world_post_book(post, e, (float)r, d);
    float* top = world_post_planes(post, e, d, over, G::HW, tid);
    G::write_frame(w, top, frames == nullptr ? nullptr : frames + (int64_t)e * frame_ld, tid, WORLD_POST_THREADS);
  } else {
    G::write_frame(w, frames + (int64_t)e * frame_ld, nullptr, tid, 64);
  }
}

// ---- the launchers: the argument checks of the extern "C" entry points and the launch
template <typename G>
int world_reset(int32_t* state, int B, int env_id0, uint32_t seed, const typename G::Params& gp, float* frames, int64_t frame_ld,
                a2c_stream_t stream) {
  if (B <= 0 || env_id0 < 0 || !G::params_ok(gp)) return A2C_ERR_ARG;
  if (state == nullptr || !world_frames_ok(frames, frame_ld, G::HW)) return A2C_ERR_ARG;
  hipLaunchKernelGGL((world_kernel<G, false, false>), dim3(B), dim3(64), 0, a2c_s(stream), state, (const int64_t*)nullptr,
                     (int64_t)0, 0, env_id0, seed, gp, 1, 0, 1, frames, frame_ld, (float*)nullptr, (float*)nullptr,
                     (float*)nullptr, (int32_t*)nullptr, (int32_t*)nullptr);
  A2C_CHECK_LAUNCH();
  return A2C_OK;
}

template <typename G>
int world_step(int32_t* state, const int64_t* actions, int64_t act_stride, int action_shift, int B, int env_id0, uint32_t seed,
               const typename G::Params& gp, float* frames, int64_t frame_ld, float* rew, float* done, float* reset,
               int32_t* ep_count, int32_t* ep_rew_sum, int frame_skip, int sticky_num, int sticky_den, a2c_stream_t stream) {
  if (B <= 0 || env_id0 < 0 || act_stride < 0 || !G::params_ok(gp) || !world_repeat_ok(frame_skip, sticky_num, sticky_den))
    return A2C_ERR_ARG;
  if (state == nullptr || actions == nullptr || rew == nullptr || done == nullptr || reset == nullptr ||
      !world_frames_ok(frames, frame_ld, G::HW))
    return A2C_ERR_ARG;
  const auto kernel = (frame_skip == 1 && sticky_num == 0) ? world_kernel<G, true, false> : world_kernel<G, true, true>;
  hipLaunchKernelGGL(kernel, dim3(B), dim3(64), 0, a2c_s(stream), state, actions, act_stride, action_shift, env_id0, seed, gp,
                     frame_skip, sticky_num, sticky_den, frames, frame_ld, rew, done, reset, ep_count, ep_rew_sum);
  A2C_CHECK_LAUNCH();
  return A2C_OK;
}

template <typename G>
int world_step_post(int32_t* state, const int64_t* actions, int64_t act_stride, int action_shift, int B, int env_id0,
                    uint32_t seed, const typename G::Params& gp, float* frames, int64_t frame_ld, float* rew, float* done,
                    float* reset, int32_t* ep_count, int32_t* ep_rew_sum, int frame_skip, int sticky_num, int sticky_den,
                    const a2c_world_post* post, a2c_stream_t stream) {
  if (B <= 0 || env_id0 < 0 || act_stride < 0 || !G::params_ok(gp) || !world_repeat_ok(frame_skip, sticky_num, sticky_den))
    return A2C_ERR_ARG;
  if (state == nullptr || actions == nullptr || rew == nullptr || done == nullptr || reset == nullptr ||
      (frames != nullptr && !world_frames_ok(frames, frame_ld, G::HW)) || !a2c_world_post_ok(post, G::HW))
    return A2C_ERR_ARG;
  const auto kernel = (frame_skip == 1 && sticky_num == 0) ? world_post_kernel<G, false> : world_post_kernel<G, true>;
  hipLaunchKernelGGL(kernel, dim3(B), dim3(WORLD_POST_THREADS), 0, a2c_s(stream), state, actions, act_stride, action_shift,
                     env_id0, seed, gp, frame_skip, sticky_num, sticky_den, frames, frame_ld, rew, done, reset, ep_count,
                     ep_rew_sum, *post);
  A2C_CHECK_LAUNCH();
  return A2C_OK;
}

// a2c_<world>_step_rules of a world on the scaffold (no episodic_life / clip_rewards: flags set are A2C_ERR_ARG): post == nullptr
// is the plain step.  A block that asks for nothing new goes to the launchers above and the kernels they launch.
template <typename G>
int world_step_rules(int32_t* state, const int64_t* actions, int64_t act_stride, int action_shift, int B, int env_id0,
                     uint32_t seed, const typename G::Params& gp, float* frames, int64_t frame_ld, float* rew, float* done,
                     float* reset, int32_t* ep_count, int32_t* ep_rew_sum, const a2c_world_rules* rules,
                     const a2c_world_post* post, a2c_stream_t stream) {
  if (!world_rules_ok(rules, false)) return A2C_ERR_ARG;
  if (world_rules_plain(*rules))
    return post == nullptr
               ? world_step<G>(state, actions, act_stride, action_shift, B, env_id0, seed, gp, frames, frame_ld, rew, done, reset,
                               ep_count, ep_rew_sum, rules->frame_skip, rules->sticky_num, rules->sticky_den, stream)
               : world_step_post<G>(state, actions, act_stride, action_shift, B, env_id0, seed, gp, frames, frame_ld, rew, done,
                                    reset, ep_count, ep_rew_sum, rules->frame_skip, rules->sticky_num, rules->sticky_den, post,
                                    stream);
  if (B <= 0 || env_id0 < 0 || act_stride < 0 || !G::params_ok(gp)) return A2C_ERR_ARG;
  if (state == nullptr || actions == nullptr || rew == nullptr || done == nullptr || reset == nullptr) return A2C_ERR_ARG;
  if (post == nullptr) {
    if (!world_frames_ok(frames, frame_ld, G::HW)) return A2C_ERR_ARG;
    hipLaunchKernelGGL((world_rules_kernel<G, false>), dim3(B), dim3(64), 0, a2c_s(stream), state, actions, act_stride,
                       action_shift, env_id0, seed, gp, *rules, frames, frame_ld, rew, done, reset, ep_count, ep_rew_sum,
                       a2c_world_post{});
  } else {
    if ((frames != nullptr && !world_frames_ok(frames, frame_ld, G::HW)) || !a2c_world_post_ok(post, G::HW)) return A2C_ERR_ARG;
    hipLaunchKernelGGL((world_rules_kernel<G, true>), dim3(B), dim3(WORLD_POST_THREADS), 0, a2c_s(stream), state, actions,
                       act_stride, action_shift, env_id0, seed, gp, *rules, frames, frame_ld, rew, done, reset, ep_count,
                       ep_rew_sum, *post);
  }
  A2C_CHECK_LAUNCH();
  return A2C_OK;
}
