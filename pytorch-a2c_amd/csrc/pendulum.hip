// Pendulum worlds in device memory: a2c_pendulum_reset / a2c_pendulum_step (rules: DESIGN.md section 6l; host twin:
// a2c_amd/pendulum.py), the textbook continuous-control world of the Gaussian nets.
//
// The game is pendulum_game.h; the kernels and launchers are lane_world.h's, one lane per env.  This file is what they need
// to know of Pendulum beside the game: 12 state words as three int4s, ONE float action quantised, and an observation of 4
// floats, one quad.
//
// What differs from the other worlds is the reward: the agent step carries it as an int in units of 2^-8, and everything that
// leaves the kernel as a float (rew[], the post bookkeeping) is that int times 2^-8, exact.  The publishing is therefore
// written out here (publish) instead of world_publish: the episode-sum atomic gets WHOLE reward units, the closed sum
// floored, so that B envs closing in the same step (every env of a pool does: only the step cap ends an episode) cannot
// overflow it and episode_stats() stays integers in reward units.
#include "lane_world.h"
#include "pendulum_game.h"

namespace {

struct PendulumLane : PendulumGame {
  using Action = float;
  using Shift = float;

  static __device__ __forceinline__ void load(const int32_t* st, World& w, WorldCount& c) {
    const int4* s4 = reinterpret_cast<const int4*>(st);
    const int4 a = s4[0], k = s4[1], l = s4[2];
    w.th = a.x; w.thd = a.y;
    c.draws = (uint32_t)k.x; c.steps = k.y; c.ep_steps = k.z; c.ep_rew = k.w;
    c.prev = l.x;
  }

  static __device__ __forceinline__ void store(int32_t* st, const World& w, const WorldCount& c) {
    int4* s4 = reinterpret_cast<int4*>(st);
    s4[0] = make_int4(w.th, w.thd, 0, 0);
    s4[1] = make_int4((int)c.draws, c.steps, c.ep_steps, c.ep_rew);
    s4[2] = make_int4(c.prev, 0, 0, 0);
  }

  static __device__ __forceinline__ int action(const float* actions, int64_t act_ld, float shift, int e) {
    return pendulum_quantise(actions[(int64_t)e * act_ld], shift);
  }

  static __device__ __forceinline__ void observe(const World& w, float4* o) { o[0] = PendulumGame::observe(w); }

  // what a step leaves beside the state words; r and closed_rew in units of 2^-8 -> the step's reward as the float the agent
  // sees
  static __device__ __forceinline__ float publish(int e, int r, bool over, bool closed, int closed_rew, float* rew, float* done,
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

  static bool actions_ok(const float* actions, int64_t act_ld) {
    return ((uintptr_t)actions & 3u) == 0 && act_ld >= PENDULUM_N_ACT;
  }
};

}  // namespace

extern "C" size_t a2c_pendulum_state_bytes(void) { return sizeof(int32_t) * (size_t)PENDULUM_WORDS; }

extern "C" int a2c_pendulum_reset(int32_t* state, int B, int env_id0, uint32_t seed, int max_episode_steps, float* obs,
                                  int64_t obs_ld, a2c_stream_t stream) {
  return lane_world_reset<PendulumLane>(state, B, env_id0, seed, {max_episode_steps}, obs, obs_ld, stream);
}

extern "C" int a2c_pendulum_step(int32_t* state, const float* actions, int64_t act_ld, float action_shift, int B, int env_id0,
                                 uint32_t seed, int max_episode_steps, float* obs, int64_t obs_ld, float* rew, float* done,
                                 float* reset, int32_t* ep_count, int32_t* ep_rew_sum, const a2c_world_rules* rules,
                                 const a2c_world_post* post, a2c_stream_t stream) {
  return lane_world_step<PendulumLane>(state, actions, act_ld, action_shift, B, env_id0, seed, {max_episode_steps}, obs, obs_ld,
                                       rew, done, reset, ep_count, ep_rew_sum, rules, post, stream);
}

// a2c_pendulum_step + the a2c_world_trunc outputs (time-limit truncation)
extern "C" int a2c_pendulum_step_trunc(int32_t* state, const float* actions, int64_t act_ld, float action_shift, int B,
                                       int env_id0, uint32_t seed, int max_episode_steps, float* obs, int64_t obs_ld, float* rew,
                                       float* done, float* reset, int32_t* ep_count, int32_t* ep_rew_sum,
                                       const a2c_world_rules* rules, const a2c_world_post* post, const a2c_world_trunc* tr,
                                       a2c_stream_t stream) {
  return lane_world_step<PendulumLane, true>(state, actions, act_ld, action_shift, B, env_id0, seed, {max_episode_steps}, obs,
                                             obs_ld, rew, done, reset, ep_count, ep_rew_sum, rules, post, stream, tr);
}
