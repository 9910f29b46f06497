// a2c_pong_step_rules: the Pong worlds' agent step with its number of game frames drawn -- PongGame on
// world_rules_kernel of world.h's scaffold.  A file, and so a code object, of its own: the kernels of pong.hip stay where they
// were in theirs, byte for byte.
#include "pong_game.h"

extern "C" int a2c_pong_step_rules(int32_t* state, const int64_t* actions, int64_t act_stride, int action_shift, int B,
                                   int env_id0, uint32_t seed, int points_to_win, int max_episode_steps, int opp_skill_num,
                                   int opp_skill_den, float* frames, int64_t frame_ld, float* rew, float* done, float* reset,
                                   int32_t* ep_count, int32_t* ep_rew_sum, const a2c_world_rules* rules,
                                   const a2c_world_post* post, a2c_stream_t stream) {
  return world_step_rules<PongGame>(state, actions, act_stride, action_shift, B, env_id0, seed,
                                    {points_to_win, max_episode_steps, opp_skill_num, opp_skill_den}, frames, frame_ld, rew,
                                    done, reset, ep_count, ep_rew_sum, rules, post, stream);
}
