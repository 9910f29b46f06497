// a2c_breakout_step_rules: the Breakout worlds' agent step with its number of game frames drawn, a lost
// life closing the step (episodic_life) and the reward as a sign (clip_rewards), around the game frame of breakout_game.h.  A
// file, and so a code object, of its own: the kernels of breakout.hip stay where they were in theirs, byte for byte.
#include "breakout_game.h"

namespace {

// brk_agent_step with the number of game frames drawn (world_draw_skip),
// and with episodic_life a game frame that loses a life WITHOUT ending the episode closes the step as an episode end does:
// prev = 0, the remaining frames dropped, the reward since the last close booked and zeroed -- but the world goes on (bricks,
// lives, ep_steps; brk_advance has already served the ball).  -> the summed reward R; over: as brk_advance; closed: over
// or such a life; closed_rew: what a closed step adds to ep_rew_sum (brk_advance leaves it in over_rew on every frame)
__device__ __forceinline__ int brk_rules_step(BrkWorld& w, WorldCount& c, int a, uint32_t seed, uint32_t env, int lives,
                                              int max_episode_steps, const a2c_world_rules& rules, bool& over, bool& closed,
                                              int& closed_rew) {
  const int k = world_draw_skip(c, seed, env, rules);
  int R = 0;
  over = closed = false;
  for (int s = 0; s < k; ++s) {
    int x = a;
    if (rules.sticky_num > 0) {
      if ((int)(world_hash(seed, env, c.draws++) % (uint32_t)rules.sticky_den) < rules.sticky_num) x = c.prev;
      c.prev = x;
    }
    const int lives0 = w.lives;
    R += brk_advance(w, c, x, seed, env, lives, max_episode_steps, over, closed_rew);
    closed = over || (rules.episodic_life != 0 && w.lives < lives0);
    if (closed) {
      c.prev = 0;
      c.ep_rew = 0;
      break;
    }
  }
  return R;
}

// The third instantiation beside REPEAT == false / true: breakout_kernel<true, true> (POST == false; `post` is not read) and
// breakout_post_kernel<true> (POST == true) around brk_rules_step.  rew is the sign of R with clip_rewards; the ep_rew word and ep_rew_sum book R itself.  A life close
// is a done AND a reset: the planes and the hidden row are zeroed as after an episode end.
template <bool POST>
__global__ __launch_bounds__(POST ? WORLD_POST_THREADS : 64) void breakout_rules_kernel(
    int32_t* __restrict__ state, const int64_t* __restrict__ actions, int64_t act_stride, int action_shift, int env_id0,
    uint32_t seed, int lives, int max_episode_steps, const a2c_world_rules rules, float* __restrict__ frames, int64_t frame_ld,
    float* __restrict__ rew, float* __restrict__ done, float* __restrict__ reset, int32_t* __restrict__ ep_count,
    int32_t* __restrict__ ep_rew_sum, const a2c_world_post post) {
  const int e = blockIdx.x, tid = threadIdx.x;
  const uint32_t env = (uint32_t)(env_id0 + e);
  int32_t* st = state + (int64_t)e * BRK_WORDS;
  BrkWorld w;
  WorldCount c;
  brk_load(st, w, c);
  const int a = world_action<4>(actions, act_stride, action_shift, e);
  if (POST) __syncthreads();
  bool over, closed;
  int closed_rew;
  const int R = brk_rules_step(w, c, a, seed, env, lives, max_episode_steps, rules, over, closed, closed_rew);
  const int r = rules.clip_rewards != 0 ? (R > 0) - (R < 0) : R;
  if (tid == 0) brk_publish(e, r, closed, closed_rew, rew, done, reset, ep_count, ep_rew_sum);
  if (tid < 64) brk_store(st, w, c, tid);
  if (POST) {
    const float d = world_post_done(post, (float)r, closed ? 1.0f : 0.0f);
    if (tid == 0) world_post_book(post, e, (float)r, d);
    float* top = world_post_planes(post, e, d, closed, BRK_HW, tid);
    brk_write_frame(w, top, frames == nullptr ? nullptr : frames + (int64_t)e * frame_ld, tid, WORLD_POST_THREADS);
  } else {
    brk_write_frame(w, frames + (int64_t)e * frame_ld, nullptr, tid, 64);
  }
}

}  // namespace

extern "C" int a2c_breakout_step_rules(int32_t* state, const int64_t* actions, int64_t act_stride, int action_shift, int B,
                                       int env_id0, uint32_t seed, int lives, int max_episode_steps, float* frames,
                                       int64_t frame_ld, float* rew, float* done, float* reset, int32_t* ep_count,
                                       int32_t* ep_rew_sum, const a2c_world_rules* rules, const a2c_world_post* post,
                                       a2c_stream_t stream) {
  if (!world_rules_ok(rules, true)) return A2C_ERR_ARG;
  if (world_rules_plain(*rules))      // nothing new is asked for: the launchers above and the kernels they launch
    return post == nullptr
               ? a2c_breakout_step_skip(state, actions, act_stride, action_shift, B, env_id0, seed, lives, max_episode_steps,
                                        frames, frame_ld, rew, done, reset, ep_count, ep_rew_sum, rules->frame_skip,
                                        rules->sticky_num, rules->sticky_den, stream)
               : a2c_breakout_step_post_skip(state, actions, act_stride, action_shift, B, env_id0, seed, lives,
                                             max_episode_steps, frames, frame_ld, rew, done, reset, ep_count, ep_rew_sum,
                                             rules->frame_skip, rules->sticky_num, rules->sticky_den, post, stream);
  if (B <= 0 || env_id0 < 0 || act_stride < 0 || !brk_world_ok(lives, max_episode_steps)) return A2C_ERR_ARG;
  if (state == nullptr || actions == nullptr || rew == nullptr || done == nullptr || reset == nullptr) return A2C_ERR_ARG;
  if (post == nullptr) {
    if (!world_frames_ok(frames, frame_ld, BRK_HW)) return A2C_ERR_ARG;
    hipLaunchKernelGGL((breakout_rules_kernel<false>), dim3(B), dim3(64), 0, a2c_s(stream), state, actions, act_stride,
                       action_shift, env_id0, seed, lives, max_episode_steps, *rules, frames, frame_ld, rew, done, reset,
                       ep_count, ep_rew_sum, a2c_world_post{});
  } else {
    if ((frames != nullptr && !world_frames_ok(frames, frame_ld, BRK_HW)) || !a2c_world_post_ok(post, BRK_HW))
      return A2C_ERR_ARG;
    hipLaunchKernelGGL((breakout_rules_kernel<true>), dim3(B), dim3(WORLD_POST_THREADS), 0, a2c_s(stream), state, actions,
                       act_stride, action_shift, env_id0, seed, lives, max_episode_steps, *rules, frames, frame_ld, rew, done,
                       reset, ep_count, ep_rew_sum, *post);
  }
  A2C_CHECK_LAUNCH();
  return A2C_OK;
}
