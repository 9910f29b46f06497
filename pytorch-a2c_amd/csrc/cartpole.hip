// CartPole worlds in device memory: a2c_cartpole_reset / a2c_cartpole_step (rules: DESIGN.md section 6k; host twin:
// a2c_amd/cartpole.py), the world of the discrete FC nets.
//
// The game is cartpole_game.h; the agent step (frame skip, sticky actions, the drawn number of game frames), the counters, the
// publishing of rew / done / reset and the bookkeeping of the post form are world.h's.  The kernels are this file's own, on
// the plan of point.hip: an env has 12 state words to load, 4 floats to write and some sixty 64-bit integer operations with
// one division in between, so ONE LANE plays an env, 64 envs per wavefront, and everything it touches moves as 16-byte
// accesses.  The frame-skip loop diverges between lanes (no barrier, no LDS: harmless).  The one cooperative part is the
// hidden rows of closed envs (post form, recurrent nets): the closed lanes are balloted and all 64 lanes clear each such row,
// coalesced.
#include "cartpole_game.h"

namespace {

constexpr int CARTPOLE_LANES = 64;      // one wavefront per workgroup

enum { CARTPOLE_RESET = 0, CARTPOLE_STEP = 1, CARTPOLE_POST = 2 };

__device__ __forceinline__ void cartpole_load(const int32_t* st, CartPoleGame::World& w, WorldCount& c) {
  const int4* s4 = reinterpret_cast<const int4*>(st);
  const int4 a = s4[0], k = s4[1], l = s4[2];
  w.x = a.x; w.xd = a.y; w.th = a.z; w.thd = a.w;
  c.draws = (uint32_t)k.x; c.steps = k.y; c.ep_steps = k.z; c.ep_rew = k.w;
  c.prev = l.x;
}

__device__ __forceinline__ void cartpole_store(int32_t* st, const CartPoleGame::World& w, const WorldCount& c) {
  int4* s4 = reinterpret_cast<int4*>(st);
  s4[0] = make_int4(w.x, w.xd, w.th, w.thd);
  s4[1] = make_int4((int)c.draws, c.steps, c.ep_steps, c.ep_rew);
  s4[2] = make_int4(c.prev, 0, 0, 0);
}

// MODE == CARTPOLE_RESET: a2c_cartpole_reset.  CARTPOLE_STEP: the plain step.  CARTPOLE_POST: step + bookkeeping + hidden-row
// reset + frame stack (`obs` may be null).  Lane `lane` of workgroup g plays env g * 64 + lane; lanes past B touch no memory
// and own no row.
template <int MODE>
__global__ __launch_bounds__(CARTPOLE_LANES) void cartpole_kernel(
    int32_t* __restrict__ state, const int64_t* __restrict__ actions, int64_t act_stride, int action_shift, int B, int env_id0,
    uint32_t seed, const CartPoleGame::Params gp, const a2c_world_rules rules, float* __restrict__ obs, int64_t obs_ld,
    float* __restrict__ rew, float* __restrict__ done, float* __restrict__ reset, int32_t* __restrict__ ep_count,
    int32_t* __restrict__ ep_rew_sum, const a2c_world_post post) {
  const int lane = threadIdx.x, e = blockIdx.x * CARTPOLE_LANES + lane;
  const bool live = e < B;
  bool zero_row = false;
  if (live) {
    const uint32_t env = (uint32_t)(env_id0 + e);
    int32_t* st = state + (int64_t)e * CARTPOLE_WORDS;
    CartPoleGame::World w;
    WorldCount c = {0u, 0, 0, 0, 0};
    float4 o;
    if (MODE == CARTPOLE_RESET) {
      CartPoleGame::new_episode(w, c, gp, seed, env);
      cartpole_store(st, w, c);
      o = CartPoleGame::observe(w);
    } else {
      cartpole_load(st, w, c);
      const int a = world_action<CARTPOLE_N_ACT>(actions, act_stride, action_shift, e);
      bool over, closed;
      int closed_rew;
      const int k = world_draw_skip(c, seed, env, rules);
      const int r = world_agent_step<CartPoleGame>(w, c, a, gp, seed, env, k, rules.sticky_num, rules.sticky_den, over, closed,
                                                   closed_rew);
      world_publish(e, r, over, closed, closed_rew, rew, done, reset, ep_count, ep_rew_sum);
      cartpole_store(st, w, c);
      o = CartPoleGame::observe(w);
      if (MODE == CARTPOLE_POST) {
        const float d = world_post_done(post, (float)r, closed ? 1.0f : 0.0f);
        world_post_book(post, e, (float)r, d);
        zero_row = post.h != nullptr && d != 0.f;
        // planes 0 .. C-2 of out[e] = over ? 0 : planes 1 .. C-1 of prev[e]: one quad a plane; the observation is plane C - 1
        float4* __restrict__ o4 = reinterpret_cast<float4*>(post.out + (int64_t)e * post.out_stride);
        const float4* __restrict__ s4 = reinterpret_cast<const float4*>(post.prev + (int64_t)e * post.prev_stride + CARTPOLE_HW);
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
  if (MODE == CARTPOLE_POST) {
    // the hidden rows of the envs whose step closed (a2c_rollout_record's zeroing): every lane of the wave is here, the
    // closed ones are balloted and the wave clears row after row, 64 floats at a time
    unsigned long long m = __ballot(zero_row);
    while (m != 0ull) {
      const int b = blockIdx.x * CARTPOLE_LANES + (__ffsll((long long)m) - 1);
      m &= m - 1ull;
      float* __restrict__ row = post.h + (int64_t)b * post.hdim;
      for (int i = lane; i < post.hdim; i += CARTPOLE_LANES) row[i] = 0.f;
    }
  }
}

bool cartpole_obs_ok(const float* obs, int64_t obs_ld) {
  return obs != nullptr && ((uintptr_t)obs & 15u) == 0 && obs_ld >= CARTPOLE_HW && obs_ld % 4 == 0;
}

}  // namespace

extern "C" size_t a2c_cartpole_state_bytes(void) { return sizeof(int32_t) * (size_t)CARTPOLE_WORDS; }

extern "C" int a2c_cartpole_reset(int32_t* state, int B, int env_id0, uint32_t seed, int max_episode_steps, float* obs,
                                  int64_t obs_ld, a2c_stream_t stream) {
  const CartPoleGame::Params gp = {max_episode_steps};
  if (B <= 0 || env_id0 < 0 || !CartPoleGame::params_ok(gp)) return A2C_ERR_ARG;
  if (state == nullptr || ((uintptr_t)state & 15u) != 0 || !cartpole_obs_ok(obs, obs_ld)) return A2C_ERR_ARG;
  hipLaunchKernelGGL((cartpole_kernel<CARTPOLE_RESET>), dim3((B + CARTPOLE_LANES - 1) / CARTPOLE_LANES), dim3(CARTPOLE_LANES), 0,
                     a2c_s(stream), state, (const int64_t*)nullptr, (int64_t)0, 0, B, env_id0, seed, gp,
                     a2c_world_rules{1, 1, 0, 1, 0, 0}, obs, obs_ld, (float*)nullptr, (float*)nullptr, (float*)nullptr,
                     (int32_t*)nullptr, (int32_t*)nullptr, a2c_world_post{});
  A2C_CHECK_LAUNCH();
  return A2C_OK;
}

extern "C" int a2c_cartpole_step(int32_t* state, const int64_t* actions, int64_t act_stride, int action_shift, int B,
                                 int env_id0, uint32_t seed, int max_episode_steps, float* obs, int64_t obs_ld, float* rew,
                                 float* done, float* reset, int32_t* ep_count, int32_t* ep_rew_sum, const a2c_world_rules* rules,
                                 const a2c_world_post* post, a2c_stream_t stream) {
  const CartPoleGame::Params gp = {max_episode_steps};
  const a2c_world_rules plain = {1, 1, 0, 1, 0, 0};
  if (rules == nullptr) rules = &plain;
  if (!world_rules_ok(rules, false)) return A2C_ERR_ARG;
  if (B <= 0 || env_id0 < 0 || act_stride < 0 || !CartPoleGame::params_ok(gp)) return A2C_ERR_ARG;
  if (state == nullptr || ((uintptr_t)state & 15u) != 0 || actions == nullptr || rew == nullptr || done == nullptr ||
      reset == nullptr)
    return A2C_ERR_ARG;
  const dim3 grid((B + CARTPOLE_LANES - 1) / CARTPOLE_LANES), block(CARTPOLE_LANES);
  if (post == nullptr) {
    if (!cartpole_obs_ok(obs, obs_ld)) return A2C_ERR_ARG;
    hipLaunchKernelGGL((cartpole_kernel<CARTPOLE_STEP>), grid, block, 0, a2c_s(stream), state, actions, act_stride, action_shift,
                       B, env_id0, seed, gp, *rules, obs, obs_ld, rew, done, reset, ep_count, ep_rew_sum, a2c_world_post{});
  } else {
    if ((obs != nullptr && !cartpole_obs_ok(obs, obs_ld)) || !a2c_world_post_ok(post, CARTPOLE_HW)) return A2C_ERR_ARG;
    hipLaunchKernelGGL((cartpole_kernel<CARTPOLE_POST>), grid, block, 0, a2c_s(stream), state, actions, act_stride, action_shift,
                       B, env_id0, seed, gp, *rules, obs, obs_ld, rew, done, reset, ep_count, ep_rew_sum, *post);
  }
  A2C_CHECK_LAUNCH();
  return A2C_OK;
}
