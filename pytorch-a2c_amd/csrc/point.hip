// Point worlds in device memory: a2c_point_reset / a2c_point_step (rules: DESIGN.md section 6j; host twin: a2c_amd/point.py),
// the continuous-control world of the Gaussian nets.
//
// The game is point_game.h; the kernels and launchers are lane_world.h's, one lane per env.  This file is what they need to
// know of Point beside the game: 16 state words as four int4s, two float actions quantised and packed into the one int the
// agent step carries, and an observation of 8 floats, two quads.
#include "lane_world.h"
#include "point_game.h"

namespace {

struct PointLane : PointGame, LanePublish {
  using Action = float;
  using Shift = float;

  static __device__ __forceinline__ void load(const int32_t* st, World& w, WorldCount& c) {
    const int4* s4 = reinterpret_cast<const int4*>(st);
    const int4 a = s4[0], b = s4[1], k = s4[2], l = s4[3];
    w.px = a.x; w.py = a.y; w.vx = a.z; w.vy = a.w;
    w.tx = b.x; w.ty = b.y; w.got = b.z;
    c.draws = (uint32_t)k.x; c.steps = k.y; c.ep_steps = k.z; c.ep_rew = k.w;
    c.prev = l.x;
  }

  static __device__ __forceinline__ void store(int32_t* st, const World& w, const WorldCount& c) {
    int4* s4 = reinterpret_cast<int4*>(st);
    s4[0] = make_int4(w.px, w.py, w.vx, w.vy);
    s4[1] = make_int4(w.tx, w.ty, w.got, 0);
    s4[2] = make_int4((int)c.draws, c.steps, c.ep_steps, c.ep_rew);
    s4[3] = make_int4(c.prev, 0, 0, 0);
  }

  static __device__ __forceinline__ int action(const float* actions, int64_t act_ld, float shift, int e) {
    const float* ar = actions + (int64_t)e * act_ld;
    return point_pack(point_quantise(ar[0], shift), point_quantise(ar[1], shift));
  }

  static __device__ __forceinline__ void observe(const World& w, float4* o) { PointGame::observe(w, o[0], o[1]); }

  static bool actions_ok(const float* actions, int64_t act_ld) { return ((uintptr_t)actions & 3u) == 0 && act_ld >= POINT_N_ACT; }
};

}  // namespace

extern "C" size_t a2c_point_state_bytes(void) { return sizeof(int32_t) * (size_t)POINT_WORDS; }

extern "C" int a2c_point_reset(int32_t* state, int B, int env_id0, uint32_t seed, int targets_to_win, int max_episode_steps,
                               float* obs, int64_t obs_ld, a2c_stream_t stream) {
  return lane_world_reset<PointLane>(state, B, env_id0, seed, {targets_to_win, max_episode_steps}, obs, obs_ld, stream);
}

extern "C" int a2c_point_step(int32_t* state, const float* actions, int64_t act_ld, float action_shift, int B, int env_id0,
                              uint32_t seed, int targets_to_win, int max_episode_steps, float* obs, int64_t obs_ld, float* rew,
                              float* done, float* reset, int32_t* ep_count, int32_t* ep_rew_sum, const a2c_world_rules* rules,
                              const a2c_world_post* post, a2c_stream_t stream) {
  return lane_world_step<PointLane>(state, actions, act_ld, action_shift, B, env_id0, seed, {targets_to_win, max_episode_steps},
                                    obs, obs_ld, rew, done, reset, ep_count, ep_rew_sum, rules, post, stream);
}

// a2c_point_step + the a2c_world_trunc outputs (time-limit truncation)
extern "C" int a2c_point_step_trunc(int32_t* state, const float* actions, int64_t act_ld, float action_shift, int B, int env_id0,
                                    uint32_t seed, int targets_to_win, int max_episode_steps, float* obs, int64_t obs_ld,
                                    float* rew, float* done, float* reset, int32_t* ep_count, int32_t* ep_rew_sum,
                                    const a2c_world_rules* rules, const a2c_world_post* post, const a2c_world_trunc* tr,
                                    a2c_stream_t stream) {
  return lane_world_step<PointLane, true>(state, actions, act_ld, action_shift, B, env_id0, seed,
                                          {targets_to_win, max_episode_steps}, obs, obs_ld, rew, done, reset, ep_count, ep_rew_sum,
                                          rules, post, stream, tr);
}
