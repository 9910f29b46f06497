// CartPole worlds in device memory: a2c_cartpole_reset / a2c_cartpole_step (rules: DESIGN.md section 6k; host twin:
// a2c_amd/cartpole.py), the world of the discrete FC nets.
//
// The game is cartpole_game.h; the kernels and launchers are lane_world.h's, one lane per env.  This file is what they need
// to know of CartPole beside the game: 12 state words as three int4s, an int64 action taken mod 2 as the picture worlds take
// theirs, and an observation of 4 floats, one quad.
#include "lane_world.h"
#include "cartpole_game.h"

namespace {

struct CartPoleLane : CartPoleGame, LanePublish {
  using Action = int64_t;
  using Shift = int;

  static __device__ __forceinline__ void load(const int32_t* st, World& w, WorldCount& c) {
    const int4* s4 = reinterpret_cast<const int4*>(st);
    const int4 a = s4[0], k = s4[1], l = s4[2];
    w.x = a.x; w.xd = a.y; w.th = a.z; w.thd = a.w;
    c.draws = (uint32_t)k.x; c.steps = k.y; c.ep_steps = k.z; c.ep_rew = k.w;
    c.prev = l.x;
  }

  static __device__ __forceinline__ void store(int32_t* st, const World& w, const WorldCount& c) {
    int4* s4 = reinterpret_cast<int4*>(st);
    s4[0] = make_int4(w.x, w.xd, w.th, w.thd);
    s4[1] = make_int4((int)c.draws, c.steps, c.ep_steps, c.ep_rew);
    s4[2] = make_int4(c.prev, 0, 0, 0);
  }

  static __device__ __forceinline__ int action(const int64_t* actions, int64_t act_stride, int shift, int e) {
    return world_action<CARTPOLE_N_ACT>(actions, act_stride, shift, e);
  }

  static __device__ __forceinline__ void observe(const World& w, float4* o) { o[0] = CartPoleGame::observe(w); }

  static bool actions_ok(const int64_t*, int64_t act_stride) { return act_stride >= 0; }
};

}  // namespace

extern "C" size_t a2c_cartpole_state_bytes(void) { return sizeof(int32_t) * (size_t)CARTPOLE_WORDS; }

extern "C" int a2c_cartpole_reset(int32_t* state, int B, int env_id0, uint32_t seed, int max_episode_steps, float* obs,
                                  int64_t obs_ld, a2c_stream_t stream) {
  return lane_world_reset<CartPoleLane>(state, B, env_id0, seed, {max_episode_steps}, obs, obs_ld, stream);
}

extern "C" int a2c_cartpole_step(int32_t* state, const int64_t* actions, int64_t act_stride, int action_shift, int B,
                                 int env_id0, uint32_t seed, int max_episode_steps, float* obs, int64_t obs_ld, float* rew,
                                 float* done, float* reset, int32_t* ep_count, int32_t* ep_rew_sum, const a2c_world_rules* rules,
                                 const a2c_world_post* post, a2c_stream_t stream) {
  return lane_world_step<CartPoleLane>(state, actions, act_stride, action_shift, B, env_id0, seed, {max_episode_steps}, obs,
                                       obs_ld, rew, done, reset, ep_count, ep_rew_sum, rules, post, stream);
}

// a2c_cartpole_step + the a2c_world_trunc outputs (time-limit truncation)
extern "C" int a2c_cartpole_step_trunc(int32_t* state, const int64_t* actions, int64_t act_stride, int action_shift, int B,
                                       int env_id0, uint32_t seed, int max_episode_steps, float* obs, int64_t obs_ld, float* rew,
                                       float* done, float* reset, int32_t* ep_count, int32_t* ep_rew_sum,
                                       const a2c_world_rules* rules, const a2c_world_post* post, const a2c_world_trunc* tr,
                                       a2c_stream_t stream) {
  return lane_world_step<CartPoleLane, true>(state, actions, act_stride, action_shift, B, env_id0, seed, {max_episode_steps}, obs,
                                             obs_ld, rew, done, reset, ep_count, ep_rew_sum, rules, post, stream, tr);
}
