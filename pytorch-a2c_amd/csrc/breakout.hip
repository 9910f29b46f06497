// Breakout worlds in device memory: a2c_breakout_reset / a2c_breakout_step / a2c_breakout_step_post and their _skip forms
// (rules: DESIGN.md sections 6d and 6g; host twin: a2c_amd/breakout.py; a2c_breakout_step_rules of section 6i:
// breakout_rules.hip).  The game, its agent step and the kernels are breakout_game.h; here are the launchers.
//
// One wavefront per env.  The state of an env is BRK_WORDS int32 words in HBM; an agent step is frame_skip (1..8) game
// frames, each a short, loop-free, wave-uniform integer computation (every lane computes the same values from the same
// words; the loop over the frames and its break at an episode end are wave-uniform too), after which lanes 0..BRK_WORDS-1 store
// one word each and all 64 lanes render the 80 x 72 prepped frame row (the grey levels breakout_prep hands on, as floats)
// as 16-byte stores where the frame-stack kernels read it.  72 / 4 = 18 = the number of brick columns, so a 16-byte store
// lies in one brick column of one row: its brick test is one shift of one row mask.  The draw, step and episode-step
// counters are part of the state the kernel advances, so a captured launch plays NEW steps at every replay.
//
// These kernels and launchers are NOT on the scaffold of world.h (world_kernel<G, ..>): written over it the same rules
// measured 0.2 us per step slower in the two-launch form and 0.02-0.06 us in step_post_skip, for a cause that was not found
// (DESIGN.md section 6h), so the bodies stay as they were.  From world.h come the draws (world_hash), the counters, the small
// helpers and the a2c_<world>_step_post part.
#include "breakout_game.h"

extern "C" size_t a2c_breakout_state_bytes(int lives) {
  if (lives < 1 || lives > MAX_LIVES) return 0;
  return sizeof(int32_t) * (size_t)BRK_WORDS;
}

extern "C" int a2c_breakout_reset(int32_t* state, int B, int env_id0, uint32_t seed, int lives, int max_episode_steps,
                                  float* frames, int64_t frame_ld, a2c_stream_t stream) {
  if (B <= 0 || env_id0 < 0 || !brk_world_ok(lives, max_episode_steps)) return A2C_ERR_ARG;
  if (state == nullptr || !world_frames_ok(frames, frame_ld, BRK_HW)) return A2C_ERR_ARG;
  hipLaunchKernelGGL((breakout_kernel<false, false>), dim3(B), dim3(64), 0, a2c_s(stream), state, (const int64_t*)nullptr, (int64_t)0,
                     0, env_id0, seed, lives, max_episode_steps, 1, 0, 1, frames, frame_ld, (float*)nullptr, (float*)nullptr,
                     (float*)nullptr, (int32_t*)nullptr, (int32_t*)nullptr);
  A2C_CHECK_LAUNCH();
  return A2C_OK;
}

extern "C" int a2c_breakout_step_skip(int32_t* state, const int64_t* actions, int64_t act_stride, int action_shift, int B,
                                      int env_id0, uint32_t seed, int lives, int max_episode_steps, float* frames,
                                      int64_t frame_ld, float* rew, float* done, float* reset, int32_t* ep_count,
                                      int32_t* ep_rew_sum, int frame_skip, int sticky_num, int sticky_den, a2c_stream_t stream) {
  if (B <= 0 || env_id0 < 0 || act_stride < 0 || !brk_world_ok(lives, max_episode_steps) ||
      !world_repeat_ok(frame_skip, sticky_num, sticky_den))
    return A2C_ERR_ARG;
  if (state == nullptr || actions == nullptr || rew == nullptr || done == nullptr || reset == nullptr ||
      !world_frames_ok(frames, frame_ld, BRK_HW))
    return A2C_ERR_ARG;
  const auto kernel = (frame_skip == 1 && sticky_num == 0) ? breakout_kernel<true, false> : breakout_kernel<true, true>;
  hipLaunchKernelGGL(kernel, dim3(B), dim3(64), 0, a2c_s(stream), state, actions, act_stride, action_shift,
                     env_id0, seed, lives, max_episode_steps, frame_skip, sticky_num, sticky_den, frames, frame_ld, rew, done,
                     reset, ep_count, ep_rew_sum);
  A2C_CHECK_LAUNCH();
  return A2C_OK;
}

extern "C" int a2c_breakout_step(int32_t* state, const int64_t* actions, int64_t act_stride, int action_shift, int B,
                                 int env_id0, uint32_t seed, int lives, int max_episode_steps, float* frames,
                                 int64_t frame_ld, float* rew, float* done, float* reset, int32_t* ep_count,
                                 int32_t* ep_rew_sum, a2c_stream_t stream) {
  return a2c_breakout_step_skip(state, actions, act_stride, action_shift, B, env_id0, seed, lives, max_episode_steps, frames,
                                frame_ld, rew, done, reset, ep_count, ep_rew_sum, 1, 0, 1, stream);
}

extern "C" int a2c_breakout_step_post_skip(int32_t* state, const int64_t* actions, int64_t act_stride, int action_shift, int B,
                                           int env_id0, uint32_t seed, int lives, int max_episode_steps, float* frames,
                                           int64_t frame_ld, float* rew, float* done, float* reset, int32_t* ep_count,
                                           int32_t* ep_rew_sum, int frame_skip, int sticky_num, int sticky_den,
                                           const a2c_world_post* post, a2c_stream_t stream) {
  if (B <= 0 || env_id0 < 0 || act_stride < 0 || !brk_world_ok(lives, max_episode_steps) ||
      !world_repeat_ok(frame_skip, sticky_num, sticky_den))
    return A2C_ERR_ARG;
  if (state == nullptr || actions == nullptr || rew == nullptr || done == nullptr || reset == nullptr ||
      (frames != nullptr && !world_frames_ok(frames, frame_ld, BRK_HW)) || !a2c_world_post_ok(post, BRK_HW))
    return A2C_ERR_ARG;
  const auto kernel = (frame_skip == 1 && sticky_num == 0) ? breakout_post_kernel<false> : breakout_post_kernel<true>;
  hipLaunchKernelGGL(kernel, dim3(B), dim3(WORLD_POST_THREADS), 0, a2c_s(stream), state, actions, act_stride,
                     action_shift, env_id0, seed, lives, max_episode_steps, frame_skip, sticky_num, sticky_den, frames, frame_ld,
                     rew, done, reset, ep_count, ep_rew_sum, *post);
  A2C_CHECK_LAUNCH();
  return A2C_OK;
}

extern "C" int a2c_breakout_step_post(int32_t* state, const int64_t* actions, int64_t act_stride, int action_shift, int B,
                                      int env_id0, uint32_t seed, int lives, int max_episode_steps, float* frames,
                                      int64_t frame_ld, float* rew, float* done, float* reset, int32_t* ep_count,
                                      int32_t* ep_rew_sum, const a2c_world_post* post, a2c_stream_t stream) {
  return a2c_breakout_step_post_skip(state, actions, act_stride, action_shift, B, env_id0, seed, lives, max_episode_steps,
                                     frames, frame_ld, rew, done, reset, ep_count, ep_rew_sum, 1, 0, 1, post, stream);
}
