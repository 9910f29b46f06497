// The scaffold of the worlds where ONE LANE plays an env (point.hip, cartpole.hip, pendulum.hip; not part of the C ABI): the
// kernel in its five modes and the launchers behind a2c_<world>_reset / a2c_<world>_step / a2c_<world>_step_trunc, written once
// over a game type G (DESIGN.md sections 6j - 6l, 6o).  The picture worlds give an env a wavefront or four because a frame has to be rendered
// (world.h); here an env has a dozen state words to load, a few floats to write and some dozens of integer operations in
// between, so one lane plays it, 64 envs per wavefront, and everything it touches moves as 16-byte accesses: the state as
// G::WORDS / 4 int4s, the observation as G::HW / 4 float4s kept in registers.  The frame-skip loop diverges between lanes (no
// barrier, no LDS: harmless).  The one cooperative part is the hidden rows of closed envs (post form, recurrent nets): the
// closed lanes are balloted and all 64 lanes clear each such row, coalesced.  The agent step (frame skip, sticky actions, the
// drawn number of game frames), the counters and the bookkeeping of the post form are world.h's.  A game G supplies
//   WORDS, HW                             int32 state words per env and floats of one observation, both multiples of 4
//   Action, Shift                         the element type of `actions` (int64_t or float) and the type of `action_shift`
//   World, Params, params_ok(Params)      the world in registers; its parameters, plain data, ONE kernel argument
//   load, store, new_episode              state words <-> registers, as int4s; reset
//   action(actions, act_ld, shift, e)     env e's action as the int the game frames take; 0 is what `prev = 0` means
//   frame(w, c, a, gp, seed, env, over, end)   one game frame in registers -> its reward; over: the episode ended, world
//                                         restarted.  Just before it restarts the world the frame calls
//                                         end.keep(w, limit_alone): w as the frame's physics left it, limit_alone = the step
//                                         limit ended the episode and the game's own end condition did not hold (world.h:
//                                         WorldNoEnd keeps nothing, WorldEnd<World> both, for the _TRUNC modes below)
//   closes(over, R)                       the `done` of an agent step with summed reward R
//   observe(w, float4*)                   the observation as HW / 4 quads
//   publish(e, r, over, closed, ...)      rew / done / reset of env e and the episode counters -> the reward as the agent
//                                         sees it, a float (LanePublish: world_publish and (float)r)
//   actions_ok(actions, act_ld)           the launcher's check of a non-null action pointer and its stride
#pragma once
#include <type_traits>
#include "world.h"

namespace {

constexpr int LANE_WORLD_LANES = 64;      // one wavefront per workgroup

// the _TRUNC modes are STEP / POST + the a2c_world_trunc outputs (a2c_<world>_step_trunc)
enum { LANE_WORLD_RESET = 0, LANE_WORLD_STEP = 1, LANE_WORLD_POST = 2, LANE_WORLD_STEP_TRUNC = 3, LANE_WORLD_POST_TRUNC = 4 };

// the kernel's last argument: the post block, and in the _TRUNC modes the trunc block behind it -- so the first three modes
// keep the parameter list, and with it the code, they had before there was a fourth
struct LanePostTrunc {
  a2c_world_post post;
  a2c_world_trunc tr;
};
template <int MODE>
struct LaneTail {
  using type = a2c_world_post;
};
template <>
struct LaneTail<LANE_WORLD_STEP_TRUNC> {
  using type = LanePostTrunc;
};
template <>
struct LaneTail<LANE_WORLD_POST_TRUNC> {
  using type = LanePostTrunc;
};
__device__ __forceinline__ const a2c_world_post& lane_post(const a2c_world_post& t) { return t; }
__device__ __forceinline__ const a2c_world_post& lane_post(const LanePostTrunc& t) { return t.post; }

// the publishing of a game whose reward is the int of its frames: a base of G
struct LanePublish {
  static __device__ __forceinline__ float publish(int e, int r, bool over, bool closed, int closed_rew, float* rew, float* done,
                                                  float* reset, int32_t* ep_count, int32_t* ep_rew_sum) {
    world_publish(e, r, over, closed, closed_rew, rew, done, reset, ep_count, ep_rew_sum);
    return (float)r;
  }
};

// MODE == LANE_WORLD_RESET: a2c_<world>_reset.  LANE_WORLD_STEP: the plain step.  LANE_WORLD_POST: step + bookkeeping +
// hidden-row reset + frame stack (`obs` may be null).  LANE_WORLD_STEP_TRUNC / _POST_TRUNC: those two, and trunc / final_obs of
// the step's env from the WorldEnd the ending frame filled (the observation of the kept world, or the step's own where no
// episode ended): one float and Q quads more per lane, from registers.  Lane `lane` of workgroup g plays env g * 64 + lane;
// lanes past B touch no memory and own no row.
template <typename G, int MODE>
__global__ __launch_bounds__(LANE_WORLD_LANES) void lane_world_kernel(
    int32_t* __restrict__ state, const typename G::Action* __restrict__ actions, int64_t act_ld, typename G::Shift action_shift,
    int B, int env_id0, uint32_t seed, const typename G::Params gp, const a2c_world_rules rules, float* __restrict__ obs,
    int64_t obs_ld, float* __restrict__ rew, float* __restrict__ done, float* __restrict__ reset, int32_t* __restrict__ ep_count,
    int32_t* __restrict__ ep_rew_sum, const typename LaneTail<MODE>::type tail) {
  constexpr int Q = G::HW / 4;      // quads a plane
  constexpr bool POST = MODE == LANE_WORLD_POST || MODE == LANE_WORLD_POST_TRUNC;
  constexpr bool TRUNC = MODE == LANE_WORLD_STEP_TRUNC || MODE == LANE_WORLD_POST_TRUNC;
  const a2c_world_post& post = lane_post(tail);
  const int lane = threadIdx.x, e = blockIdx.x * LANE_WORLD_LANES + lane;
  const bool live = e < B;
  bool zero_row = false;
  if (live) {
    const uint32_t env = (uint32_t)(env_id0 + e);
    int32_t* st = state + (int64_t)e * G::WORDS;
    typename G::World w;
    WorldCount c = {0u, 0, 0, 0, 0};
    float4 o[Q];
    if (MODE == LANE_WORLD_RESET) {
      G::new_episode(w, c, gp, seed, env);
      G::store(st, w, c);
      G::observe(w, o);
    } else {
      G::load(st, w, c);
      const int a = G::action(actions, act_ld, action_shift, e);
      bool over, closed;
      int closed_rew;
      const int k = world_draw_skip(c, seed, env, rules);
      typename std::conditional<TRUNC, WorldEnd<typename G::World>, WorldNoEnd>::type end;
      const int r = world_agent_step<G>(w, c, a, gp, seed, env, k, rules.sticky_num, rules.sticky_den, over, closed, closed_rew,
                                        end);
      const float rf = G::publish(e, r, over, closed, closed_rew, rew, done, reset, ep_count, ep_rew_sum);
      G::store(st, w, c);
      G::observe(w, o);
      if constexpr (TRUNC) {
        float4 fo[Q];
        if (over) {
          G::observe(end.w, fo);
        } else {
#pragma unroll
          for (int q = 0; q < Q; ++q) fo[q] = o[q];
        }
        tail.tr.trunc[(int64_t)e * tail.tr.trunc_stride] = (over && end.limit_alone) ? 1.0f : 0.0f;
        float4* __restrict__ f4 = reinterpret_cast<float4*>(tail.tr.final_obs + (int64_t)e * tail.tr.final_ld);
#pragma unroll
        for (int q = 0; q < Q; ++q) f4[q] = fo[q];
      }
      if (POST) {
        const float d = world_post_done(post, rf, closed ? 1.0f : 0.0f);
        world_post_book(post, e, rf, d);
        zero_row = post.h != nullptr && d != 0.f;
        // planes 0 .. C-2 of out[e] = over ? 0 : planes 1 .. C-1 of prev[e]: Q quads a plane; the observation is plane C - 1
        float4* __restrict__ o4 = reinterpret_cast<float4*>(post.out + (int64_t)e * post.out_stride);
        const float4* __restrict__ s4 = reinterpret_cast<const float4*>(post.prev + (int64_t)e * post.prev_stride + G::HW);
        const int n4 = (post.C - 1) * Q;
        if (over) {
          for (int i = 0; i < n4; ++i) o4[i] = make_float4(0.f, 0.f, 0.f, 0.f);
        } else {
          for (int i = 0; i < n4; ++i) o4[i] = s4[i];
        }
#pragma unroll
        for (int q = 0; q < Q; ++q) o4[n4 + q] = o[q];
      }
    }
    if (obs != nullptr) {
      float4* f4 = reinterpret_cast<float4*>(obs + (int64_t)e * obs_ld);
#pragma unroll
      for (int q = 0; q < Q; ++q) f4[q] = o[q];
    }
  }
  if (POST) {
    // the hidden rows of the envs whose step closed (a2c_rollout_record's zeroing): every lane of the wave is here, the
    // closed ones are balloted and the wave clears row after row, 64 floats at a time
    unsigned long long m = __ballot(zero_row);
    while (m != 0ull) {
      const int b = blockIdx.x * LANE_WORLD_LANES + (__ffsll((long long)m) - 1);
      m &= m - 1ull;
      float* __restrict__ row = post.h + (int64_t)b * post.hdim;
      for (int i = lane; i < post.hdim; i += LANE_WORLD_LANES) row[i] = 0.f;
    }
  }
}

// ---- the launchers: the argument checks of the extern "C" entry points and the launch
template <typename G>
bool lane_obs_ok(const float* obs, int64_t obs_ld) {
  return obs != nullptr && ((uintptr_t)obs & 15u) == 0 && obs_ld >= G::HW && obs_ld % 4 == 0;
}

template <typename G>
int lane_world_reset(int32_t* state, int B, int env_id0, uint32_t seed, const typename G::Params& gp, float* obs, int64_t obs_ld,
                     a2c_stream_t stream) {
  if (B <= 0 || env_id0 < 0 || !G::params_ok(gp)) return A2C_ERR_ARG;
  if (state == nullptr || ((uintptr_t)state & 15u) != 0 || !lane_obs_ok<G>(obs, obs_ld)) return A2C_ERR_ARG;
  hipLaunchKernelGGL((lane_world_kernel<G, LANE_WORLD_RESET>), dim3((B + LANE_WORLD_LANES - 1) / LANE_WORLD_LANES),
                     dim3(LANE_WORLD_LANES), 0, a2c_s(stream), state, (const typename G::Action*)nullptr, (int64_t)0,
                     (typename G::Shift)0, B, env_id0, seed, gp, a2c_world_rules{1, 1, 0, 1, 0, 0}, obs, obs_ld, (float*)nullptr,
                     (float*)nullptr, (float*)nullptr, (int32_t*)nullptr, (int32_t*)nullptr, a2c_world_post{});
  A2C_CHECK_LAUNCH();
  return A2C_OK;
}

// the launcher's checks of a trunc block
template <typename G>
bool lane_trunc_ok(const a2c_world_trunc* tr) {
  return tr != nullptr && tr->trunc != nullptr && tr->trunc_stride >= 1 && tr->final_obs != nullptr &&
         ((uintptr_t)tr->final_obs & 15u) == 0 && tr->final_ld >= G::HW && tr->final_ld % 4 == 0;
}

// post == nullptr is the plain step; `obs` is optional only with a post block.  rules == nullptr is the plain world.
// TRUNC: a2c_<world>_step_trunc, `tr` required; else `tr` is not read
template <typename G, bool TRUNC = false>
int lane_world_step(int32_t* state, const typename G::Action* actions, int64_t act_ld, typename G::Shift action_shift, int B,
                    int env_id0, uint32_t seed, const typename G::Params& gp, float* obs, int64_t obs_ld, float* rew, float* done,
                    float* reset, int32_t* ep_count, int32_t* ep_rew_sum, const a2c_world_rules* rules, const a2c_world_post* post,
                    a2c_stream_t stream, const a2c_world_trunc* tr = nullptr) {
  const a2c_world_rules plain = {1, 1, 0, 1, 0, 0};
  if (rules == nullptr) rules = &plain;
  if (TRUNC && !lane_trunc_ok<G>(tr)) return A2C_ERR_ARG;
  if (!world_rules_ok(rules, false)) return A2C_ERR_ARG;
  if (B <= 0 || env_id0 < 0 || !G::params_ok(gp)) return A2C_ERR_ARG;
  if (state == nullptr || ((uintptr_t)state & 15u) != 0 || actions == nullptr || !G::actions_ok(actions, act_ld) ||
      rew == nullptr || done == nullptr || reset == nullptr)
    return A2C_ERR_ARG;
  const dim3 grid((B + LANE_WORLD_LANES - 1) / LANE_WORLD_LANES), block(LANE_WORLD_LANES);
  LanePostTrunc both = {};      // (the _TRUNC modes' last argument)
  if (TRUNC) {
    if (post != nullptr) both.post = *post;
    both.tr = *tr;
  }
  if (post == nullptr) {
    if (!lane_obs_ok<G>(obs, obs_ld)) return A2C_ERR_ARG;
    if constexpr (TRUNC)
      hipLaunchKernelGGL((lane_world_kernel<G, LANE_WORLD_STEP_TRUNC>), grid, block, 0, a2c_s(stream), state, actions, act_ld,
                         action_shift, B, env_id0, seed, gp, *rules, obs, obs_ld, rew, done, reset, ep_count, ep_rew_sum,
                         both);
    else
      hipLaunchKernelGGL((lane_world_kernel<G, LANE_WORLD_STEP>), grid, block, 0, a2c_s(stream), state, actions, act_ld,
                         action_shift, B, env_id0, seed, gp, *rules, obs, obs_ld, rew, done, reset, ep_count, ep_rew_sum,
                         a2c_world_post{});
  } else {
    if ((obs != nullptr && !lane_obs_ok<G>(obs, obs_ld)) || !a2c_world_post_ok(post, G::HW)) return A2C_ERR_ARG;
    if constexpr (TRUNC)
      hipLaunchKernelGGL((lane_world_kernel<G, LANE_WORLD_POST_TRUNC>), grid, block, 0, a2c_s(stream), state, actions, act_ld,
                         action_shift, B, env_id0, seed, gp, *rules, obs, obs_ld, rew, done, reset, ep_count, ep_rew_sum,
                         both);
    else
      hipLaunchKernelGGL((lane_world_kernel<G, LANE_WORLD_POST>), grid, block, 0, a2c_s(stream), state, actions, act_ld,
                         action_shift, B, env_id0, seed, gp, *rules, obs, obs_ld, rew, done, reset, ep_count, ep_rew_sum, *post);
  }
  A2C_CHECK_LAUNCH();
  return A2C_OK;
}

}  // namespace
