// Pong worlds in device memory: a2c_pong_reset / a2c_pong_step / a2c_pong_step_post and their _skip forms (rules: DESIGN.md
// sections 6c and 6g; host twin: a2c_amd/pong.py; a2c_pong_step_rules of section 6i: pong_rules.hip).
//
// The game is pong_game.h: PongGame, the rules of one game frame on PONG_WORDS int32 state words per env and the 80 x 80
// prepped frame row (1 on the two paddles and the ball, 0 elsewhere).  The kernels, the frame-skip / sticky-action loop and
// the launchers are the scaffold of world.h, which states what a game supplies.
#include "pong_game.h"

extern "C" size_t a2c_pong_state_bytes(int points_to_win) {
  if (points_to_win < 1 || points_to_win > MAX_POINTS) return 0;
  return sizeof(int32_t) * (size_t)PONG_WORDS;
}

extern "C" int a2c_pong_reset(int32_t* state, int B, int env_id0, uint32_t seed, int points_to_win, int max_episode_steps,
                              int opp_skill_num, int opp_skill_den, float* frames, int64_t frame_ld, a2c_stream_t stream) {
  return world_reset<PongGame>(state, B, env_id0, seed, {points_to_win, max_episode_steps, opp_skill_num, opp_skill_den}, frames,
                               frame_ld, stream);
}

extern "C" int a2c_pong_step_skip(int32_t* state, const int64_t* actions, int64_t act_stride, int action_shift, int B,
                                  int env_id0, uint32_t seed, int points_to_win, int max_episode_steps, int opp_skill_num,
                                  int opp_skill_den, float* frames, int64_t frame_ld, float* rew, float* done, float* reset,
                                  int32_t* ep_count, int32_t* ep_rew_sum, int frame_skip, int sticky_num, int sticky_den,
                                  a2c_stream_t stream) {
  return world_step<PongGame>(state, actions, act_stride, action_shift, B, env_id0, seed,
                              {points_to_win, max_episode_steps, opp_skill_num, opp_skill_den}, frames, frame_ld, rew, done,
                              reset, ep_count, ep_rew_sum, frame_skip, sticky_num, sticky_den, stream);
}

extern "C" int a2c_pong_step(int32_t* state, const int64_t* actions, int64_t act_stride, int action_shift, int B, int env_id0,
                             uint32_t seed, int points_to_win, int max_episode_steps, int opp_skill_num, int opp_skill_den,
                             float* frames, int64_t frame_ld, float* rew, float* done, float* reset, int32_t* ep_count,
                             int32_t* ep_rew_sum, a2c_stream_t stream) {
  return world_step<PongGame>(state, actions, act_stride, action_shift, B, env_id0, seed,
                              {points_to_win, max_episode_steps, opp_skill_num, opp_skill_den}, frames, frame_ld, rew, done,
                              reset, ep_count, ep_rew_sum, 1, 0, 1, stream);
}

extern "C" int a2c_pong_step_post_skip(int32_t* state, const int64_t* actions, int64_t act_stride, int action_shift, int B,
                                       int env_id0, uint32_t seed, int points_to_win, int max_episode_steps, int opp_skill_num,
                                       int opp_skill_den, float* frames, int64_t frame_ld, float* rew, float* done,
                                       float* reset, int32_t* ep_count, int32_t* ep_rew_sum, int frame_skip, int sticky_num,
                                       int sticky_den, const a2c_world_post* post, a2c_stream_t stream) {
  return world_step_post<PongGame>(state, actions, act_stride, action_shift, B, env_id0, seed,
                                   {points_to_win, max_episode_steps, opp_skill_num, opp_skill_den}, frames, frame_ld, rew,
                                   done, reset, ep_count, ep_rew_sum, frame_skip, sticky_num, sticky_den, post, stream);
}

extern "C" int a2c_pong_step_post(int32_t* state, const int64_t* actions, int64_t act_stride, int action_shift, int B,
                                  int env_id0, uint32_t seed, int points_to_win, int max_episode_steps, int opp_skill_num,
                                  int opp_skill_den, float* frames, int64_t frame_ld, float* rew, float* done, float* reset,
                                  int32_t* ep_count, int32_t* ep_rew_sum, const a2c_world_post* post, a2c_stream_t stream) {
  return world_step_post<PongGame>(state, actions, act_stride, action_shift, B, env_id0, seed,
                                   {points_to_win, max_episode_steps, opp_skill_num, opp_skill_den}, frames, frame_ld, rew,
                                   done, reset, ep_count, ep_rew_sum, 1, 0, 1, post, stream);
}
