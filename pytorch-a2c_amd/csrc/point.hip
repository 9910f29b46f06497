// Point worlds in device memory: a2c_point_reset / a2c_point_step (rules: DESIGN.md section 6j; host twin: a2c_amd/point.py),
// the continuous-control world of the Gaussian nets.
//
// The game is point_game.h; the agent step (frame skip, sticky actions, the drawn number of game frames), the counters, the
// publishing of rew / done / reset and the bookkeeping of the post form are world.h's.  The kernels are this file's own: the
// picture worlds give an env a wavefront or four because a frame has to be rendered; here an env has 16 state words to load,
// 8 floats to write and a few dozen integer operations in between, so ONE LANE plays an env, 64 envs per wavefront, and
// everything it touches moves as 16-byte accesses.  The frame-skip loop diverges between lanes (no barrier, no LDS: harmless).
// The one cooperative part is the hidden rows of closed envs (post form, recurrent nets): the closed lanes are balloted and
// all 64 lanes clear each such row, coalesced.
#include "point_game.h"

namespace {

constexpr int POINT_LANES = 64;      // one wavefront per workgroup

enum { POINT_RESET = 0, POINT_STEP = 1, POINT_POST = 2 };

__device__ __forceinline__ void point_load(const int32_t* st, PointGame::World& w, WorldCount& c) {
  const int4* s4 = reinterpret_cast<const int4*>(st);
  const int4 a = s4[0], b = s4[1], k = s4[2], l = s4[3];
  w.px = a.x; w.py = a.y; w.vx = a.z; w.vy = a.w;
  w.tx = b.x; w.ty = b.y; w.got = b.z;
  c.draws = (uint32_t)k.x; c.steps = k.y; c.ep_steps = k.z; c.ep_rew = k.w;
  c.prev = l.x;
}

__device__ __forceinline__ void point_store(int32_t* st, const PointGame::World& w, const WorldCount& c) {
  int4* s4 = reinterpret_cast<int4*>(st);
  s4[0] = make_int4(w.px, w.py, w.vx, w.vy);
  s4[1] = make_int4(w.tx, w.ty, w.got, 0);
  s4[2] = make_int4((int)c.draws, c.steps, c.ep_steps, c.ep_rew);
  s4[3] = make_int4(c.prev, 0, 0, 0);
}

// MODE == POINT_RESET: a2c_point_reset.  POINT_STEP: the plain step.  POINT_POST: step + bookkeeping + hidden-row reset + frame
// stack (`obs` may be null).  Lane `lane` of workgroup g plays env g * 64 + lane; lanes past B touch no memory and own no row.
template <int MODE>
__global__ __launch_bounds__(POINT_LANES) void point_kernel(int32_t* __restrict__ state, const float* __restrict__ actions,
                                                            int64_t act_ld, float action_shift, int B, int env_id0,
                                                            uint32_t seed, const PointGame::Params gp,
                                                            const a2c_world_rules rules, float* __restrict__ obs, int64_t obs_ld,
                                                            float* __restrict__ rew, float* __restrict__ done,
                                                            float* __restrict__ reset, int32_t* __restrict__ ep_count,
                                                            int32_t* __restrict__ ep_rew_sum, const a2c_world_post post) {
  const int lane = threadIdx.x, e = blockIdx.x * POINT_LANES + lane;
  const bool live = e < B;
  bool zero_row = false;
  if (live) {
    const uint32_t env = (uint32_t)(env_id0 + e);
    int32_t* st = state + (int64_t)e * POINT_WORDS;
    PointGame::World w;
    WorldCount c = {0u, 0, 0, 0, 0};
    float4 lo, hi;
    if (MODE == POINT_RESET) {
      PointGame::new_episode(w, c, gp, seed, env);
      point_store(st, w, c);
      PointGame::observe(w, lo, hi);
    } else {
      point_load(st, w, c);
      const float* ar = actions + (int64_t)e * act_ld;
      const int a = point_pack(point_quantise(ar[0], action_shift), point_quantise(ar[1], action_shift));
      bool over, closed;
      int closed_rew;
      const int k = world_draw_skip(c, seed, env, rules);
      const int r = world_agent_step<PointGame>(w, c, a, gp, seed, env, k, rules.sticky_num, rules.sticky_den, over, closed,
                                                closed_rew);
      world_publish(e, r, over, closed, closed_rew, rew, done, reset, ep_count, ep_rew_sum);
      point_store(st, w, c);
      PointGame::observe(w, lo, hi);
      if (MODE == POINT_POST) {
        const float d = world_post_done(post, (float)r, closed ? 1.0f : 0.0f);
        world_post_book(post, e, (float)r, d);
        zero_row = post.h != nullptr && d != 0.f;
        // planes 0 .. C-2 of out[e] = over ? 0 : planes 1 .. C-1 of prev[e]: 2 quads a plane; the observation is plane C - 1
        float4* __restrict__ o4 = reinterpret_cast<float4*>(post.out + (int64_t)e * post.out_stride);
        const float4* __restrict__ s4 = reinterpret_cast<const float4*>(post.prev + (int64_t)e * post.prev_stride + POINT_HW);
        const int n4 = (post.C - 1) * (POINT_HW / 4);
        if (over) {
          for (int i = 0; i < n4; ++i) o4[i] = make_float4(0.f, 0.f, 0.f, 0.f);
        } else {
          for (int i = 0; i < n4; ++i) o4[i] = s4[i];
        }
        o4[n4] = lo;
        o4[n4 + 1] = hi;
      }
    }
    if (obs != nullptr) {
      float4* f4 = reinterpret_cast<float4*>(obs + (int64_t)e * obs_ld);
      f4[0] = lo;
      f4[1] = hi;
    }
  }
  if (MODE == POINT_POST) {
    // the hidden rows of the envs whose step closed (a2c_rollout_record's zeroing): every lane of the wave is here, the
    // closed ones are balloted and the wave clears row after row, 64 floats at a time
    unsigned long long m = __ballot(zero_row);
    while (m != 0ull) {
      const int b = blockIdx.x * POINT_LANES + (__ffsll((long long)m) - 1);
      m &= m - 1ull;
      float* __restrict__ row = post.h + (int64_t)b * post.hdim;
      for (int i = lane; i < post.hdim; i += POINT_LANES) row[i] = 0.f;
    }
  }
}

bool point_obs_ok(const float* obs, int64_t obs_ld) {
  return obs != nullptr && ((uintptr_t)obs & 15u) == 0 && obs_ld >= POINT_HW && obs_ld % 4 == 0;
}

}  // namespace

extern "C" size_t a2c_point_state_bytes(void) { return sizeof(int32_t) * (size_t)POINT_WORDS; }

extern "C" int a2c_point_reset(int32_t* state, int B, int env_id0, uint32_t seed, int targets_to_win, int max_episode_steps,
                               float* obs, int64_t obs_ld, a2c_stream_t stream) {
  const PointGame::Params gp = {targets_to_win, max_episode_steps};
  if (B <= 0 || env_id0 < 0 || !PointGame::params_ok(gp)) return A2C_ERR_ARG;
  if (state == nullptr || ((uintptr_t)state & 15u) != 0 || !point_obs_ok(obs, obs_ld)) return A2C_ERR_ARG;
  hipLaunchKernelGGL((point_kernel<POINT_RESET>), dim3((B + POINT_LANES - 1) / POINT_LANES), dim3(POINT_LANES), 0, a2c_s(stream),
                     state, (const float*)nullptr, (int64_t)0, 0.f, B, env_id0, seed, gp, a2c_world_rules{1, 1, 0, 1, 0, 0}, obs,
                     obs_ld, (float*)nullptr, (float*)nullptr, (float*)nullptr, (int32_t*)nullptr, (int32_t*)nullptr,
                     a2c_world_post{});
  A2C_CHECK_LAUNCH();
  return A2C_OK;
}

extern "C" int a2c_point_step(int32_t* state, const float* actions, int64_t act_ld, float action_shift, int B, int env_id0,
                              uint32_t seed, int targets_to_win, int max_episode_steps, float* obs, int64_t obs_ld, float* rew,
                              float* done, float* reset, int32_t* ep_count, int32_t* ep_rew_sum, const a2c_world_rules* rules,
                              const a2c_world_post* post, a2c_stream_t stream) {
  const PointGame::Params gp = {targets_to_win, max_episode_steps};
  const a2c_world_rules plain = {1, 1, 0, 1, 0, 0};
  if (rules == nullptr) rules = &plain;
  if (!world_rules_ok(rules, false)) return A2C_ERR_ARG;
  if (B <= 0 || env_id0 < 0 || act_ld < POINT_N_ACT || !PointGame::params_ok(gp)) return A2C_ERR_ARG;
  if (state == nullptr || ((uintptr_t)state & 15u) != 0 || actions == nullptr || ((uintptr_t)actions & 3u) != 0 ||
      rew == nullptr || done == nullptr || reset == nullptr)
    return A2C_ERR_ARG;
  const dim3 grid((B + POINT_LANES - 1) / POINT_LANES), block(POINT_LANES);
  if (post == nullptr) {
    if (!point_obs_ok(obs, obs_ld)) return A2C_ERR_ARG;
    hipLaunchKernelGGL((point_kernel<POINT_STEP>), grid, block, 0, a2c_s(stream), state, actions, act_ld, action_shift, B,
                       env_id0, seed, gp, *rules, obs, obs_ld, rew, done, reset, ep_count, ep_rew_sum, a2c_world_post{});
  } else {
    if ((obs != nullptr && !point_obs_ok(obs, obs_ld)) || !a2c_world_post_ok(post, POINT_HW)) return A2C_ERR_ARG;
    hipLaunchKernelGGL((point_kernel<POINT_POST>), grid, block, 0, a2c_s(stream), state, actions, act_ld, action_shift, B,
                       env_id0, seed, gp, *rules, obs, obs_ld, rew, done, reset, ep_count, ep_rew_sum, *post);
  }
  A2C_CHECK_LAUNCH();
  return A2C_OK;
}
