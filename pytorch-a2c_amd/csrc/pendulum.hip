// Pendulum worlds in device memory: a2c_pendulum_reset / a2c_pendulum_step (rules: DESIGN.md section 6l; host twin:
// a2c_amd/pendulum.py), the textbook continuous-control world of the Gaussian nets.
//
// The game is pendulum_game.h; the agent step (frame skip, sticky actions, the drawn number of game frames), the counters and
// the bookkeeping of the post form are world.h's.  The kernels are this file's own, on the plan of point.hip and
// cartpole.hip: an env has 12 state words to load, 4 floats to write and some eighty 64-bit integer operations in between,
// so ONE LANE plays an env, 64 envs per wavefront, and everything it touches moves as 16-byte accesses.  The frame-skip loop
// diverges between lanes (no barrier, no LDS: harmless).  The one cooperative part is the hidden rows of closed envs (post
// form, recurrent nets): the closed lanes are balloted and all 64 lanes clear each such row, coalesced.
//
// What differs from the other worlds is the reward: the agent step carries it as an int in units of 2^-8, and everything that
// leaves the kernel as a float (rew[], the post bookkeeping) is that int times 2^-8, exact.  The publishing is therefore
// written out here (pendulum_publish) instead of world_publish: the episode-sum atomic gets WHOLE reward units, the closed
// sum floored, so that B envs closing in the same step (every env of a pool does: only the step cap ends an episode) cannot
// overflow it and episode_stats() stays integers in reward units.
#include "pendulum_game.h"

namespace {

constexpr int PENDULUM_LANES = 64;      // one wavefront per workgroup

enum { PENDULUM_RESET = 0, PENDULUM_STEP = 1, PENDULUM_POST = 2 };

__device__ __forceinline__ void pendulum_load(const int32_t* st, PendulumGame::World& w, WorldCount& c) {
  const int4* s4 = reinterpret_cast<const int4*>(st);
  const int4 a = s4[0], k = s4[1], l = s4[2];
  w.th = a.x; w.thd = a.y;
  c.draws = (uint32_t)k.x; c.steps = k.y; c.ep_steps = k.z; c.ep_rew = k.w;
  c.prev = l.x;
}

__device__ __forceinline__ void pendulum_store(int32_t* st, const PendulumGame::World& w, const WorldCount& c) {
  int4* s4 = reinterpret_cast<int4*>(st);
  s4[0] = make_int4(w.th, w.thd, 0, 0);
  s4[1] = make_int4((int)c.draws, c.steps, c.ep_steps, c.ep_rew);
  s4[2] = make_int4(c.prev, 0, 0, 0);
}

// what a step leaves beside the state words; r and closed_rew in units of 2^-8 -> the step's reward as the float the agent sees
__device__ __forceinline__ float pendulum_publish(int e, int r, bool over, bool closed, int closed_rew, float* rew, float* done,
                                                  float* reset, int32_t* ep_count, int32_t* ep_rew_sum) {
  if (closed) {
    if (ep_count != nullptr) atomicAdd(ep_count, 1);
    if (ep_rew_sum != nullptr) atomicAdd(ep_rew_sum, closed_rew >> PD_REW_FRAC);      // the floor: >> of a negative int
  }
  const float rf = (float)r * (1.f / (float)(1 << PD_REW_FRAC));                      // |r| <= 8 * 4166: exact
  rew[e] = rf;
  done[e] = closed ? 1.0f : 0.0f;
  reset[e] = over ? 1.0f : 0.0f;
  return rf;
}

// MODE == PENDULUM_RESET: a2c_pendulum_reset.  PENDULUM_STEP: the plain step.  PENDULUM_POST: step + bookkeeping + hidden-row
// reset + frame stack (`obs` may be null).  Lane `lane` of workgroup g plays env g * 64 + lane; lanes past B touch no memory
// and own no row.
template <int MODE>
__global__ __launch_bounds__(PENDULUM_LANES) void pendulum_kernel(
    int32_t* __restrict__ state, const float* __restrict__ actions, int64_t act_ld, float action_shift, int B, int env_id0,
    uint32_t seed, const PendulumGame::Params gp, const a2c_world_rules rules, float* __restrict__ obs, int64_t obs_ld,
    float* __restrict__ rew, float* __restrict__ done, float* __restrict__ reset, int32_t* __restrict__ ep_count,
    int32_t* __restrict__ ep_rew_sum, const a2c_world_post post) {
  const int lane = threadIdx.x, e = blockIdx.x * PENDULUM_LANES + lane;
  const bool live = e < B;
  bool zero_row = false;
  if (live) {
    const uint32_t env = (uint32_t)(env_id0 + e);
    int32_t* st = state + (int64_t)e * PENDULUM_WORDS;
    PendulumGame::World w;
    WorldCount c = {0u, 0, 0, 0, 0};
    float4 o;
    if (MODE == PENDULUM_RESET) {
      PendulumGame::new_episode(w, c, gp, seed, env);
      pendulum_store(st, w, c);
      o = PendulumGame::observe(w);
    } else {
      pendulum_load(st, w, c);
      const int a = pendulum_quantise(actions[(int64_t)e * act_ld], action_shift);
      bool over, closed;
      int closed_rew;
      const int k = world_draw_skip(c, seed, env, rules);
      const int r = world_agent_step<PendulumGame>(w, c, a, gp, seed, env, k, rules.sticky_num, rules.sticky_den, over, closed,
                                                   closed_rew);
      const float rf = pendulum_publish(e, r, over, closed, closed_rew, rew, done, reset, ep_count, ep_rew_sum);
      pendulum_store(st, w, c);
      o = PendulumGame::observe(w);
      if (MODE == PENDULUM_POST) {
        const float d = world_post_done(post, rf, closed ? 1.0f : 0.0f);
        world_post_book(post, e, rf, d);
        zero_row = post.h != nullptr && d != 0.f;
        // planes 0 .. C-2 of out[e] = over ? 0 : planes 1 .. C-1 of prev[e]: one quad a plane; the observation is plane C - 1
        float4* __restrict__ o4 = reinterpret_cast<float4*>(post.out + (int64_t)e * post.out_stride);
        const float4* __restrict__ s4 = reinterpret_cast<const float4*>(post.prev + (int64_t)e * post.prev_stride + PENDULUM_HW);
        const int n4 = post.C - 1;
        if (over) {
          for (int i = 0; i < n4; ++i) o4[i] = make_float4(0.f, 0.f, 0.f, 0.f);
        } else {
          for (int i = 0; i < n4; ++i) o4[i] = s4[i];
        }
        o4[n4] = o;
      }
    }
    if (obs != nullptr) *reinterpret_cast<float4*>(obs + (int64_t)e * obs_ld) = o;
  }
  if (MODE == PENDULUM_POST) {
    // the hidden rows of the envs whose step closed (a2c_rollout_record's zeroing): every lane of the wave is here, the
    // closed ones are balloted and the wave clears row after row, 64 floats at a time
    unsigned long long m = __ballot(zero_row);
    while (m != 0ull) {
      const int b = blockIdx.x * PENDULUM_LANES + (__ffsll((long long)m) - 1);
      m &= m - 1ull;
      float* __restrict__ row = post.h + (int64_t)b * post.hdim;
      for (int i = lane; i < post.hdim; i += PENDULUM_LANES) row[i] = 0.f;
    }
  }
}

bool pendulum_obs_ok(const float* obs, int64_t obs_ld) {
  return obs != nullptr && ((uintptr_t)obs & 15u) == 0 && obs_ld >= PENDULUM_HW && obs_ld % 4 == 0;
}

}  // namespace

extern "C" size_t a2c_pendulum_state_bytes(void) { return sizeof(int32_t) * (size_t)PENDULUM_WORDS; }

extern "C" int a2c_pendulum_reset(int32_t* state, int B, int env_id0, uint32_t seed, int max_episode_steps, float* obs,
                                  int64_t obs_ld, a2c_stream_t stream) {
  const PendulumGame::Params gp = {max_episode_steps};
  if (B <= 0 || env_id0 < 0 || !PendulumGame::params_ok(gp)) return A2C_ERR_ARG;
  if (state == nullptr || ((uintptr_t)state & 15u) != 0 || !pendulum_obs_ok(obs, obs_ld)) return A2C_ERR_ARG;
  hipLaunchKernelGGL((pendulum_kernel<PENDULUM_RESET>), dim3((B + PENDULUM_LANES - 1) / PENDULUM_LANES), dim3(PENDULUM_LANES), 0,
                     a2c_s(stream), state, (const float*)nullptr, (int64_t)0, 0.f, B, env_id0, seed, gp,
                     a2c_world_rules{1, 1, 0, 1, 0, 0}, obs, obs_ld, (float*)nullptr, (float*)nullptr, (float*)nullptr,
                     (int32_t*)nullptr, (int32_t*)nullptr, a2c_world_post{});
  A2C_CHECK_LAUNCH();
  return A2C_OK;
}

extern "C" int a2c_pendulum_step(int32_t* state, const float* actions, int64_t act_ld, float action_shift, int B, int env_id0,
                                 uint32_t seed, int max_episode_steps, float* obs, int64_t obs_ld, float* rew, float* done,
                                 float* reset, int32_t* ep_count, int32_t* ep_rew_sum, const a2c_world_rules* rules,
                                 const a2c_world_post* post, a2c_stream_t stream) {
  const PendulumGame::Params gp = {max_episode_steps};
  const a2c_world_rules plain = {1, 1, 0, 1, 0, 0};
  if (rules == nullptr) rules = &plain;
  if (!world_rules_ok(rules, false)) return A2C_ERR_ARG;
  if (B <= 0 || env_id0 < 0 || act_ld < PENDULUM_N_ACT || !PendulumGame::params_ok(gp)) return A2C_ERR_ARG;
  if (state == nullptr || ((uintptr_t)state & 15u) != 0 || actions == nullptr || ((uintptr_t)actions & 3u) != 0 ||
      rew == nullptr || done == nullptr || reset == nullptr)
    return A2C_ERR_ARG;
  const dim3 grid((B + PENDULUM_LANES - 1) / PENDULUM_LANES), block(PENDULUM_LANES);
  if (post == nullptr) {
    if (!pendulum_obs_ok(obs, obs_ld)) return A2C_ERR_ARG;
    hipLaunchKernelGGL((pendulum_kernel<PENDULUM_STEP>), grid, block, 0, a2c_s(stream), state, actions, act_ld, action_shift, B,
                       env_id0, seed, gp, *rules, obs, obs_ld, rew, done, reset, ep_count, ep_rew_sum, a2c_world_post{});
  } else {
    if ((obs != nullptr && !pendulum_obs_ok(obs, obs_ld)) || !a2c_world_post_ok(post, PENDULUM_HW)) return A2C_ERR_ARG;
    hipLaunchKernelGGL((pendulum_kernel<PENDULUM_POST>), grid, block, 0, a2c_s(stream), state, actions, act_ld, action_shift, B,
                       env_id0, seed, gp, *rules, obs, obs_ld, rew, done, reset, ep_count, ep_rew_sum, *post);
  }
  A2C_CHECK_LAUNCH();
  return A2C_OK;
}
