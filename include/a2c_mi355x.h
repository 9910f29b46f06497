/*
 * a2c_mi355x.h -- C ABI of liba2c_mi355x.so: the MI355X (gfx950 / CDNA4) kernels of
 * the A2C rollout+update hot path of grantsrb/PyTorch-A2C.
 *
 * The reference has no FFI layer (it is pure Python on torch); its boundary is the
 * Python API of a2c/runner.py, a2c/updater.py, a2c/models.py and a2c/utils.py.
 * Each entry point below replaces the arithmetic of one reference call site
 * (cited as file:line into /root/reference/a2c/).  The Python package
 * pytorch-a2c_amd/a2c_amd binds these with ctypes and mirrors the reference API.
 *
 * Conventions
 *   - plain C, no torch types: raw DEVICE pointers into caller-owned memory, sizes,
 *     and the HIP stream (hipStream_t passed as void*; NULL = default stream);
 *   - no allocation, no ownership transfer, no host synchronisation, no global
 *     state: every call only enqueues kernels on `stream` (graph-capturable);
 *     scratch memory is passed in as `ws` / `ws_bytes` and sized by the
 *     matching *_ws_bytes() query;
 *   - all floating-point data is IEEE fp32, row-major, contiguous unless a
 *     leading dimension / stride argument says otherwise; actions are int64;
 *   - return value: 0 = A2C_OK, negative = error (a2c_error_string()).
 */
/*
 * Environment switches
 *
 * The library reads these variables and no others (a2c_env_on / a2c_env_int in csrc/a2c_common.h;
 * tests/test_abi.py checks this list against the sources).  "=1" means the first character is '1'.
 * "per call": read on every call, so a process may flip it; "once": read at the first use.
 * No switch changes a result except by choosing between two tested kernels (or two tested tilings
 * of one kernel, which give bit-identical sums).
 *
 *   A2C_NO_STREAM=1          per call  conv forward / backward: no persistent streaming kernels (A3C conv1 / conv2 class)
 *   A2C_BWD_X6=0             per call  A3C conv2 backward-data: fp32 MFMA streaming kernel instead of the bf16 x 6 one
 *   A2C_WGRAD_X6=0           per call  A3C conv2 weight gradient (and the rank-n head path): fp32 MFMA kernel instead of x 6
 *   A2C_WGRAD_F32=1          per call  conv1 weight gradient from the frame store: fp32 MFMAs instead of the bf16 pipe
 *   A2C_WSB_NO_RING=1        per call  that bf16 kernel: every sample loaded whole (no frame ring in LDS)
 *   A2C_NO_TUNE=1            per call  conv forward / band backward-data: rule-sized tiles, no timed tile search
 *   A2C_BAND_TY=<n>          per call  band backward-data: tile height n (0 = the rule), no timed search
 *   A2C_NO_BAND_GROUPS=1     per call  band backward-data: one workgroup for all channels
 *   A2C_IGEMM_LDS_KB=<kb>    per call  conv forward: LDS budget of the generic kernel (default 64); set: no timed search
 *   A2C_RUN3_LDS_KB=<kb>     per call  conv forward: LDS budget of the run3 kernel (default 80); set: no timed search
 *   A2C_FUSE_W1=1            per call  a2c_conv2d_bwd_data_w1*: the fused band pass (measured slower) instead of two passes
 *   A2C_C3W_D2=1             per call  3x3 weight gradient: round 3's tall-band instances (one chunk of lookahead)
 *   A2C_NO_ODD_BS=1          per call  GRUModel conv4 / conv5 backward-data: the generic band kernel, not the odd-image one
 *   A2C_NO_CHAIN=1           per call  a2c_conv2d_fwd_chain_supported answers 0 (separate launches)
 *   A2C_NO_W1_FRAMES=1       once      a2c_conv2d_bwd_data_w1_frames_supported answers 0
 *   A2C_GEMM_X9=0|1|2        per call  a2c_gemm_f32: 0 or 1 = fp32 MFMA kernels only; 2 = the x 6 kernel from M, N, K >= 256
 *                                      and M N K >= 2.5e8 on; unset = from M, N, K >= 1024 and M N K >= 2e10 on
 *   A2C_NO_GEMM_NT=1         per call  a2c_gemm_f32: not the A B^T split-K kernel
 *   A2C_NO_SKINNY_STREAM=1   per call  a2c_gemm_f32: not the skinny streaming split-K kernel
 *   A2C_GRU_K4=1             per call  GRU cell kernels: four-way K split (bit-identical to the launches they replace)
 *   A2C_NO_RING=1            per call  a2c_a3c_rollout: the per-step body instead of the ring kernel
 *   A2C_RING_BLOCKS=0        per call  a2c_a3c_rollout: no ring kernel when there are more envs than CUs
 *   A2C_RING_F32=1           per call  ring kernel: conv1 on fp32 MFMAs instead of the bf16 pipe
 */
#ifndef A2C_MI355X_H
#define A2C_MI355X_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define A2C_OK 0
#define A2C_ERR_ARG (-1)      /* invalid argument (NULL pointer, bad size, unsupported shape) */
#define A2C_ERR_LAUNCH (-2)   /* hipGetLastError() after the launch was not hipSuccess          */
#define A2C_ERR_WORKSPACE (-3)/* ws_bytes smaller than the matching *_ws_bytes() query          */

typedef void *a2c_stream_t;   /* hipStream_t */

int a2c_version(void);                 /* ABI version, currently 2 */
const char *a2c_error_string(int code);

/* ------------------------------------------------------------------ a5 / a7: scans
 * utils.discount (utils.py:63-79): y[i] = x[i] + g * (dones[i]==1 ? 0 : y[i+1]),
 * evaluated strictly sequentially per row (fp32 multiply then fp32 add, no FMA), so the
 * result is bit-identical to the reference.  The input is n_seg independent rows of
 * length T (row r = elements [r*T, (r+1)*T)); the running sum starts at 0 at each row end.
 * With n_seg == 1 this is exactly utils.discount on a flat array of T elements.
 * When n_seg > 1 the rows are only independent if every row ends with dones == 1
 * (Runner guarantees it: runner.py:223,244).  With err_flag (device int) given, a violation
 * sets it to 1 AND the call recomputes the array as one flat row on the device, so the
 * result is the reference's for any data; with err_flag == NULL the rows are taken as
 * independent without a check.                                                         */
int a2c_discount_scan(const float *x, const float *dones, float *y, int64_t n_seg,
                      int64_t T, float g, int *err_flag, a2c_stream_t stream);
/* updater.py:70-71 + 86-88 fused: advs = discount(deltas, dones, g_adv) and
 * rets = discount(rewards, dones, g_ret) in one pass over the three inputs.            */
int a2c_gae_returns_fused(const float *deltas, const float *rewards, const float *dones,
                          float *advs, float *rets, int64_t n_seg, int64_t T, float g_adv,
                          float g_ret, int *err_flag, a2c_stream_t stream);
/* The three scalar reductions of the update (a2c_moments, a2c_loss_fwd_bwd's loss sums, a2c_gradnorm_sq) are DETERMINISTIC:
 * per-workgroup fp64 partials go to `reduce_scratch` and the last workgroup to finish adds them in workgroup order (no
 * atomics on the sums).  reduce_scratch: A2C_REDUCE_SCRATCH_DOUBLES doubles of device memory, ZERO before its first use
 * (word 0 is a ticket counter the kernels reset); calls that share one scratch must be ordered (same stream).           */
#define A2C_REDUCE_SCRATCH_DOUBLES (8 + 3 * 1024)
/* sums[0] = sum x, sums[1] = sum x*x in double; feeds the
 * mean / unbiased-std normalisations of updater.py:89-98.                              */
int a2c_moments(const float *x, int64_t n, double *sums, double *reduce_scratch, a2c_stream_t stream);
/* y = (x - mean) / (std + eps), mean/std (unbiased) derived from sums (a2c_moments,
 * possibly all-reduced across ranks) over n_global elements: updater.py:98.            */
int a2c_normalize(const float *x, float *y, int64_t n, const double *sums, int64_t n_global,
                  float eps, a2c_stream_t stream);
/* y = a + b (returns = advs + vals.data, updater.py:84)                                */
int a2c_add(const float *a, const float *b, float *y, int64_t n, a2c_stream_t stream);

/* ------------------------------------------------------------------ a1: frame stack
 * utils.next_state (utils.py:26-43) + the state write of runner.py:199, batched over B
 * envs.  out[b] = reset_mask[b] ? [0,..,0, frame_new[b]] : [prev[b][1:], frame_new[b]];
 * C = n_frame_stack planes of HW floats.  prev / out are addressed with a per-env stride
 * in floats so they can point into the rollout buffer `states[idx*T + t]`.              */
int a2c_frame_stack_push(const float *frame_new, const float *reset_mask, const float *prev,
                         int64_t prev_stride, float *out, int64_t out_stride, int B, int C,
                         int HW, a2c_stream_t stream);
/* The same with the new frame as UINT8 pixels (the host pool's transport format: pong_prep,
 * preprocessing.py:11-17, yields uint8; runner.py:199 `FloatTensor(state)` is the expansion):
 * frame_u8[b*frame_stride + i], i < HW, frame_stride in bytes (% 4 == 0); HW % 4 == 0.     */
int a2c_frame_stack_push_u8(const uint8_t *frame_u8, int64_t frame_stride, const float *reset_mask,
                            const float *prev, int64_t prev_stride, float *out, int64_t out_stride,
                            int B, int C, int HW, a2c_stream_t stream);

/* ------------------------------------------------------------------ g1: device relay of the host env pool
 * (a2c_hostpool.h) for the per-step rollout of the models without a persistent kernel.  Replaces, per env step, the
 * host round trip of the memcpy ingest -- D2H of the actions, a2c_pool_post_actions, a2c_pool_wait_frames,
 * a2c_pool_unpack, H2D of the frames block (runner.py:199,207-226 of the reference did the same hand-off one
 * element at a time) -- by two launches that stay on the stream:
 *   a2c_pool_publish_actions   cmd[i] = ((seq_base[0] + seq_off) << 32) | actions[i*act_stride], i < n
 *                              (system-scope 8-byte stores into the device-mapped pinned region)
 *   a2c_pool_ingest            waits until rec[i].seq == seq_base[0] + seq_off (every env, bounded by
 *                              timeout_ticks of the 100 MHz wall clock; on expiry *err = 1 and this and all later
 *                              calls return without waiting), then rew[i], done[i] <- rec[i] and
 *                              frames_out[i*out_stride ..] <- frames[i*frame_stride .. +frame_bytes] (16-byte
 *                              system-scope loads over PCIe).  frame_bytes, strides: multiples of 16.
 * cmd / rec / frames are the DEVICE addresses of the pool's granules of the first env of the block
 * (hipHostGetDevicePointer of the registered region); seq_base lives in device memory so that a captured hipGraph
 * of a segment can be replayed by later rollouts.                                               */
int a2c_pool_publish_actions(uint64_t *cmd, const int64_t *actions, int64_t act_stride, int n,
                             const uint32_t *seq_base, uint32_t seq_off, a2c_stream_t stream);
int a2c_pool_ingest(const uint64_t *rec, const uint8_t *frames, int64_t frame_stride, int frame_bytes, int n,
                    const uint32_t *seq_base, uint32_t seq_off, int64_t timeout_ticks, int *err, float *rew,
                    float *done, uint8_t *frames_out, int64_t out_stride, a2c_stream_t stream);
/* The same for a pool with the PACKED transport (A2C_FRAME_BITS in a2c_hostpool.h: binary preprocessors such as
 * pong_prep, preprocessing.py:15-16, publish one bit per pixel): n_pixels / 8 bytes per env cross the host link and
 * frames_out receives the n_pixels uint8 {0,1} pixels the uint8 kernels expect (n_pixels % 16 == 0).
 * a2c_unpack_bits is the expansion alone, for packed frames a hipMemcpyAsync staged in HBM (memcpy ingest).    */
int a2c_pool_ingest_bits(const uint64_t *rec, const uint8_t *frames, int64_t frame_stride, int n_pixels, int n,
                         const uint32_t *seq_base, uint32_t seq_off, int64_t timeout_ticks, int *err, float *rew,
                         float *done, uint8_t *frames_out, int64_t out_stride, a2c_stream_t stream);
int a2c_unpack_bits(const uint8_t *src, int64_t src_stride, uint8_t *dst, int64_t dst_stride, int n,
                    int n_pixels, a2c_stream_t stream);
/* a2c_pool_ingest / a2c_pool_ingest_bits (packed_bits != 0; frame_elems = uint8 pixels per frame) whose workgroup for env b
 * also does env b's share of a2c_rollout_post_frames for the env step the answer belongs to (runner.py:208-232: rewards /
 * dones / the TD residual of the step before, the valid-plane count of the next state, and for recurrent nets the hidden row
 * of the next step): the same values as the two calls in sequence, one launch.  Arguments after out_stride as in
 * a2c_rollout_post_frames (val = the value head's output of the state the action was sampled from).            */
int a2c_pool_ingest_post(int packed_bits, const uint64_t *rec, const uint8_t *frames, int64_t frame_stride,
                         int frame_elems, int n, const uint32_t *seq_base, uint32_t seq_off,
                         int64_t timeout_ticks, int *err, float *rew, float *done, uint8_t *frames_out,
                         int64_t out_stride, const float *val, int64_t val_stride, float *val_prev,
                         float *rewards, float *dones, float *deltas, int64_t T, int64_t t, int64_t slot0,
                         float gamma, int pong, float *done_eff, float *h, int hdim, float *h_rows,
                         int64_t h_rows_stride, const float *h_src, int *nvalid_rows, int *nvalid_carry,
                         a2c_stream_t stream);

/* ------------------------------------------------------------------ f4: preprocessing on the device, single-frame store
 * a2c_frame_prep_u8 = pong_prep / breakout_prep (preprocessing.py:11-23) on n raw (H, W, C) uint8 frames, raw_stride
 * bytes apart: out[oy][ox] = raw[y0 + oy*step][x0 + ox*step][0] for the crop y0:y1, x0:x1; binarise != 0 applies
 * pong_prep's "144 and 109 -> 0, everything else that is not 0 -> 1" (preprocessing.py:14-16); binarise == 0 keeps the
 * byte (breakout_prep: skimage <= 0.18's rgb2grey returns a 2-D slice unchanged).  pong_prep = (35, 195, 0, W, 2, 1),
 * breakout_prep = (35, 195, 8, W - 8, 2, 0).  Output rows out_stride bytes apart, OW % 4 == 0.                      */
int a2c_frame_prep_u8(const uint8_t *raw, int64_t raw_stride, int H, int W, int C, int y0, int y1, int x0, int x1,
                      int step, int binarise, uint8_t *out, int64_t out_stride, int n, a2c_stream_t stream);
/* Single-frame uint8 store (utils.py:26-43, runner.py:199 behind the boundary): slot r keeps T + C frames of HW bytes,
 * slot_stride bytes apart; state (r, t) = the window frames[r][t .. t+C-1], planes c < C - nvalid are zero (frames from
 * before the env's last reset).  a2c_frame_store_begin: start of a slot -- frames[r][0..C-1] = frames[r][T..T+C-1]
 * (the state the previous slot ended in), nvalid_rows[r*T] = nvalid_carry[r].  a2c_rollout_post_frames: the bookkeeping
 * of a2c_rollout_post[_rec] for env step t WITHOUT a frame-stack copy (the ingest wrote the new frame straight into
 * frames[r][t+C]): rewards / dones / deltas / val_prev [/ hidden-state reset and h_states row], and the valid-plane
 * count of state t+1 (1 after a real done, else min(count + 1, 4): the count saturates at 4 whatever C is -- this entry
 * point is not given C and serves the four-plane store, T + 4 frames per slot, that Runner._frame_store builds only for
 * n_frame_stack == 4) into nvalid_rows[(slot0+b)*T + t+1] (not written when t == T-1) / nvalid_carry.
 * a2c_frames_to_states: the reference's fp32 `states` rows from the store, on demand: state k (< nt) of slot r (< R)
 * -> out + r*out_slot_stride + k*C*HW floats, valid-plane counts nvalid[r*nvalid_slot_stride + k] (NULL: all valid). */
int a2c_frame_store_begin(uint8_t *frame_store, int64_t slot_stride, int64_t T, int C, int HW, int32_t *nvalid_rows,
                          const int32_t *nvalid_carry, int B, a2c_stream_t stream);
int a2c_rollout_post_frames(const float *rew, const float *done, const float *val, int64_t val_stride, float *val_prev,
                            float *rewards, float *dones, float *deltas, int64_t T, int64_t t, int64_t slot0,
                            float gamma, int pong, int B, float *done_eff, float *h, int hdim, float *h_rows,
                            int64_t h_rows_stride, const float *h_src, int32_t *nvalid_rows, int32_t *nvalid_carry,
                            a2c_stream_t stream);
int a2c_frames_to_states(const uint8_t *frame_store, int64_t slot_stride, const int32_t *nvalid,
                         int64_t nvalid_slot_stride, float *out, int64_t out_slot_stride, int R, int nt, int C, int HW,
                         a2c_stream_t stream);

/* ------------------------------------------------------------------ a2: sampler
 * SequentialEnvironment.get_action discrete branch (runner.py:94-97) + utils.sample_action
 * (utils.py:45-60): p = softmax(logits); running fp32 cumsum in index order; first a with
 * cumsum >= u[b]; -1 if none.  actions int64 with element stride act_stride;
 * probs (B,A) optional (may be NULL).                                                   */
int a2c_softmax_sample(const float *logits, int64_t ld_logits, const float *u, int64_t *actions,
                       int64_t act_stride, float *probs, int B, int A, a2c_stream_t stream);
/* utils.sample_action on given probabilities (no softmax); actions as fp32 like the
 * reference's return value.                                                             */
int a2c_sample_probs(const float *probs, const float *u, float *actions, int64_t B, int A,
                     a2c_stream_t stream);

/* ------------------------------------------------------------------ a3: rollout records
 * One env-step of Runner.rollout bookkeeping for B slots (runner.py:212-232): with
 * e = slot*T + t, writes rewards[e] = rew, dones[e] = done_eff where
 * done_eff = done || (pong && rew != 0) (runner.py:213-214), and, when t > 0,
 * deltas[e-1] = rewards[e-1] + (gamma*val[b])*(1-dones[e-1]) - val_prev[b] (runner.py:231);
 * then val_prev[b] = val[b].  If h != NULL (recurrent, hdim columns) rows of h whose
 * done_eff is set are zeroed (runner.py:219-220).                                       */
int a2c_rollout_record(const float *rew, const float *done, const float *val, int64_t val_stride,
                       float *val_prev,
                       float *rewards, float *dones, float *deltas, float *done_eff_out,
                       float *h, int hdim, int B, int64_t T, int64_t t, int64_t slot0,
                       float gamma, int pong, a2c_stream_t stream);
/* a2c_rollout_record (feed-forward nets: no hidden state) and a2c_frame_stack_push of the same
 * env step in ONE launch (one hipGraph node fewer per rollout step).                     */
int a2c_rollout_post(const float *rew, const float *done, const float *val, int64_t val_stride,
                     float *val_prev, float *rewards, float *dones, float *deltas, int64_t T,
                     int64_t t, int64_t slot0, float gamma, int pong, const float *frame_new,
                     const float *reset_mask, const float *prev, int64_t prev_stride, float *out,
                     int64_t out_stride, int B, int C, int HW, a2c_stream_t stream);
int a2c_rollout_post_u8(const float *rew, const float *done, const float *val, int64_t val_stride,
                        float *val_prev, float *rewards, float *dones, float *deltas, int64_t T,
                        int64_t t, int64_t slot0, float gamma, int pong, const uint8_t *frame_u8,
                        int64_t frame_stride, const float *reset_mask, const float *prev,
                        int64_t prev_stride, float *out, int64_t out_stride, int B, int C, int HW,
                        a2c_stream_t stream);
/* The same for recurrent nets, with the hidden-state handling of the step folded into the launch (runner.py:201,
 * 219-221): h[b] = 0 where the env step ended an episode (done, or the Pong override), done_eff_out[b] = that flag,
 * and, when h_rows != NULL, h_rows[b*h_rows_stride ..] = h[b] (the h_states row of the step that follows).
 * h_src (NULL = h): where the previous step's cell left its new hidden rows (B, hdim); h = masked h_src, so a cell
 * that writes h_new somewhere else (e.g. into the update's time-major buffers) needs no copy back.
 * Exactly one of frame_new (fp32) / frame_u8 is given.                                          */
int a2c_rollout_post_rec(const float *rew, const float *done, const float *val, int64_t val_stride,
                         float *val_prev, float *rewards, float *dones, float *deltas, int64_t T,
                         int64_t t, int64_t slot0, float gamma, int pong, const float *frame_new,
                         const uint8_t *frame_u8, int64_t frame_stride, const float *reset_mask,
                         const float *prev, int64_t prev_stride, float *out, int64_t out_stride, int B,
                         int C, int HW, float *done_eff_out, float *h, int hdim, float *h_rows,
                         int64_t h_rows_stride, const float *h_src, a2c_stream_t stream);
/* End of slot (runner.py:236-245): e = slot*T + T-1; if dones[e] == 0:
 * rewards[e] += gamma*val_boot[b], dones[e] = 1; then deltas[e] = rewards[e] - val_prev[b]. */
int a2c_rollout_bootstrap(const float *val_boot, int64_t val_stride, const float *val_prev, float *rewards,
                          float *dones, float *deltas, int B, int64_t T, int64_t slot0,
                          float gamma, a2c_stream_t stream);
/* Evaluation on a device env pool: the FIRST episode of every env, out of the rows a rollout slot left.  Env e (< E) owns
 * rewards / dones [e*T .. e*T + K) (K steps played, rows T >= K apart; dones as the record kernels wrote them, Pong
 * override included).  While active[e] != 0 and t0 + t < max_steps, for t = 0 .. K-1 in order:
 * ep_rew[e] = ep_rew[e] + rewards[e*T+t] (fp32, in step order), ep_len[e] += 1, and a nonzero dones[e*T+t] sets
 * active[e] = 0 -- what the restarted world does afterwards is ignored.  t0 = the global index of step 0 of this chunk.
 * *n_active = the number of envs whose active is still nonzero: overwritten, not added to.  One workgroup, no atomics:
 * deterministic.  An env that enters with active[e] == 0 is not written.                                          */
int a2c_eval_scan(const float *rewards, const float *dones, int64_t T, int64_t K, int E, int64_t t0, int64_t max_steps,
                  float *ep_rew, int32_t *ep_len, int32_t *active, int32_t *n_active, a2c_stream_t stream);
/* One whole rollout step of the A3CModel-shaped policy (models.py:60-90: conv 8x8/s4 -> 16,
 * conv 4x4/s2 -> 32, proj_matrx WITHOUT activation, pi/value heads) in ONE launch, one workgroup
 * per env; replaces, per step of Runner.rollout (runner.py:190-232):
 *   1. (rew != NULL) a2c_rollout_record of the env step that produced this state: step index
 *      t_rec, value read from heads[b*ldh + n_actions] as left by the previous call;
 *   2. the state: frame_new != NULL: a2c_frame_stack_push(prev, frame_new, reset_mask);
 *      frame_new == NULL: the rows of prev as they are.  If out != NULL the state is also written
 *      to out[b*out_stride ..] (the states row of the rollout buffer / the bookmark);
 *   3. the forward pass on that state with the weights prepared for inference:
 *      wfrag1/wfrag2 = a2c_conv2d_prep_weights(kind 0) of the two conv layers,
 *      Wc ((n_actions+1) x F) = [pi.weight; value.weight] . proj_matrx.weight, bc likewise;
 *      heads[b*ldh + 0..n_actions] = [logits | value];
 *   4. (u != NULL) a2c_softmax_sample of the logits into actions[b*act_stride];
 *   5. (bootstrap != 0, t_rec == T-1) a2c_rollout_bootstrap with the value just computed
 *      (runner.py:236-245).
 * Requires C == 4, W % 4 == 0 and the state + activations to fit one CU's LDS
 * (a2c_a3c_step_supported); other shapes use the per-layer entry points.               */
typedef struct {
  int B, C, H, W, n_actions;
  const float *prev; int64_t prev_stride;
  const float *frame_new;          /* (B, H*W) or NULL                                   */
  const float *reset_mask;         /* (B,) or NULL                                       */
  float *out; int64_t out_stride;  /* or NULL                                            */
  const float *wfrag1, *bias1, *wfrag2, *bias2, *Wc, *bc;
  float *heads; int64_t ldh;
  const float *u;                  /* (B,) uniforms or NULL (no sampling)                */
  int64_t *actions; int64_t act_stride;
  const float *rew, *done;         /* (B,) of env step t_rec, or NULL (no bookkeeping)   */
  float *val_prev, *rewards, *dones, *deltas;
  int64_t T, t_rec, slot0;
  float gamma;
  int pong, bootstrap;
  const uint8_t *frame_u8;         /* instead of frame_new: uint8 frame (B, frame_stride bytes), */
  int64_t frame_stride;            /* e.g. the pool's frames block after its H2D copy            */
  /* optional stash of the conv activations of this state (post-ReLU, NCHW): a1 (16, OH1, OW1) and a2
   * (32, OH2, OW2) of env b go to a1_out + b*a1_stride / a2_out + b*a2_stride.  The weights do not change
   * between a rollout and the update that consumes it (training.py:150-165), so Updater.update_model's
   * forward (updater.py:80) would recompute exactly these tensors: it reads the stash instead.
   * The rows are written 16 bytes at a time: A2C_ERR_ARG for a stash when OH1*OW1 is not a multiple of 4, a stride
   * that is not, or a pointer that is not 16-byte aligned (the same for a1_rows / a2_rows of a2c_a3c_rollout).  */
  float *a1_out; int64_t a1_stride;
  float *a2_out; int64_t a2_stride;
  float *heads_out; int64_t heads_out_stride;   /* optional second copy of [logits | value] (same stash) */
} a2c_a3c_step_args;
int a2c_a3c_step_supported(int C, int H, int W, int n_actions);
int a2c_a3c_step(const a2c_a3c_step_args *args, a2c_stream_t stream);

/* A WHOLE rollout slot of the A3CModel-shaped policy -- all n_tsteps iterations of the loop of
 * Runner.rollout (runner.py:198-232) plus the bootstrap (runner.py:236-245) for B envs -- in ONE
 * persistent launch that talks to the host env workers directly through the pinned pool region
 * (include/a2c_hostpool.h), with no host code and no kernel boundary between steps:
 *   iteration t of env b (one workgroup per env, workgroups of several envs take turns):
 *     t > 0: wait for rec[env0+b].seq == seq0+t, read reward/done from the granule and the uint8
 *            frame straight from the pinned frames slot (system-scope loads over PCIe), record env
 *            step t-1 exactly like a2c_a3c_step;  t == 0: the state is bookmark[b];
 *     state -> states[(slot0+b)*T + t] (t == T: -> bookmark[b]); forward; 
 *     t < T: sample with u[t*u_stride + b] -> actions[(slot0+b)*T + t], and publish
 *            cmd[env0+b] = (seq0+t) << 32 | action with one 8-byte system-scope store: the worker
 *            that owns the env steps it as soon as it sees the granule;  t == T: bootstrap.
 * Results are identical to T+1 calls of a2c_a3c_step (see conv1_weight below for the one exception).  Every wait on the host is bounded by
 * timeout_ticks (100 MHz ticks); on a timeout *err is set to 1 and the workgroup stops.
 * Shapes as a2c_a3c_step_supported, uint8 frames, (H*W) % 16 == 0.                          */
typedef struct {
  int B, C, H, W, n_actions;
  float *states;                   /* rollout buffer, rows of S = C*H*W floats                */
  float *bookmark;                 /* (B, S)                                                  */
  const float *wfrag1, *bias1, *wfrag2, *bias2, *Wc, *bc;
  float *heads; int64_t ldh;
  const float *u; int64_t u_stride;
  int64_t *actions;
  float *val_prev, *rewards, *dones, *deltas;
  int64_t T, slot0;
  float gamma;
  int pong;
  uint64_t *cmd;                   /* device-mapped pool arrays (a2c_rollout_buffer_create)   */
  const uint64_t *rec;
  const uint8_t *frames; int64_t frame_stride;
  uint32_t seq0;                   /* env steps every env has taken before this slot          */
  int env0;                        /* pool index of env b is env0 + b                         */
  int *err;                        /* device int                                              */
  int64_t timeout_ticks;
  float *a1_rows, *a2_rows;        /* optional activation stash, row e = (slot0+b)*T + t (see a2c_a3c_step_args) */
  float *heads_rows; int64_t heads_rows_ld;   /* optional [logits | value] of state e, row stride heads_rows_ld */
  /* optional single-frame uint8 store (row f4 of SURVEY.md section 8): slot r keeps T+4 frames of H*W bytes,
   * frame_store_slot_stride bytes apart; the 4 planes of state (r, t) are the CONTIGUOUS window
   * frames[r][t .. t+3] (the newest frame of state t is frames[r][t+3]; frames[r][0..3] are copied from
   * frames[r][T..T+3], the state the previous slot ended in).  nvalid_rows[e] = how many of the 4 planes of state
   * e are real (planes older than the env's last reset are zero, utils.py:37-42); nvalid_carry[b] carries that
   * count of the bookmark state from slot to slot.  Consumer: a2c_conv2d_bwd_weight_frames.              */
  uint8_t *frame_store; int64_t frame_store_slot_stride;
  int32_t *nvalid_rows, *nvalid_carry;
  int frame_bits;                  /* 1: `frames` holds the packed transport (one bit per pixel, frame_stride >= H*W/8) */
  /* optional: the first conv layer's weight tensor (16, 4, 8, 8) as the model stores it.  When given,
   * every env gets a workgroup that keeps its state in LDS for the whole slot (the "ring" kernel) and
   * overlaps the env worker's turn-around with the part of the next forward that does not depend on the new frame
   * (conv1's sum is then ordered plane-major: results equal a2c_a3c_step's up to fp32 re-association).  More envs than
   * CUs: ceil(B / CUs) such launches one after the other, launch k playing the envs b = k (mod that count); with
   * A2C_RING_BLOCKS=0 in the environment ONE launch of the per-step body instead, whose workgroups take several envs in
   * turns (results identical to a2c_a3c_step).                                                                   */
  const float *conv1_weight;
  /* with frame_store, ring kernel only: 1 = do NOT write the fp32 `states` rows (a2c_frames_to_states expands them from
   * the store on demand; the update reads the store: a2c_conv2d_bwd_weight_frames); the bookmark is always written.
   * A2C_ERR_ARG when the launch cannot run as the ring kernel (no conv1_weight, A2C_NO_RING=1, or B > CU count with
   * A2C_RING_BLOCKS=0).                                                                                            */
  int states_lazy;
  /* optional, ring kernel with frame_bits: the pool's SELF-VALIDATING mirror of the packed frames (a2c_hostpool.h:
   * tagged_chunks chunks of 16 bytes per env, tagged_stride bytes apart, every chunk carries the step number's low 16
   * bits).  One wave then fetches poll + frame + reward/done of an env step with ONE 16-byte load per lane -- one PCIe
   * round trip instead of two dependent ones (rec granule, then frame) -- and re-tries until every tag matches.    */
  const uint8_t *tagged; int64_t tagged_stride; int tagged_chunks;
  /* optional, ring kernel only, with a1_rows: the MASK BITS ("lane masks") of the a1 stash rows -- (16*OH1*OW1)/64 64-bit
   * words per state, row e = (slot0+b)*T + t like a1_rows: bit (i & 7) of byte (i >> 3) of the row = (a1[i] > 0), i the flat
   * (c, y, x) index.  Consumer: a2c_conv2d_bwd_data_lanemask (the update's conv2 backward-data reads 800 B per sample instead
   * of the 25.6 KB activation row as its ReLU mask, updater.py:128's autograd).  A2C_ERR_ARG when the launch cannot run as
   * the ring kernel (ask a2c_a3c_ring_supported first) or 16*OH1*OW1 is not a multiple of 256.                         */
  uint64_t *a1_lanemask_rows;
  /* ... and, with a2_rows, the mask bits of the a2 stash rows: F/8 bytes per state (F = 32*OH2*OW2, a multiple of 8), bit
   * (i & 7) of byte (i >> 3) = (a2[i] > 0).  Consumer: a2c_small_n_bwd_data_bits.  Ring kernel only, like the field above. */
  uint8_t *a2_maskbit_rows;
} a2c_a3c_rollout_args;
int a2c_a3c_rollout(const a2c_a3c_rollout_args *args, a2c_stream_t stream);
/* 1 when a2c_a3c_rollout with these shapes, this many envs and this conv1_weight pointer runs the ring kernel (the only
 * body that honours states_lazy: runner.py:199's fp32 row left out), 0 when it would fall back to the per-step persistent
 * body -- same predicate as the launcher's (LDS budget, conv1 output <= 512 pixels, weight alignment, A2C_NO_RING /
 * A2C_RING_BLOCKS read per call).  A caller asks this BEFORE it decides to leave the rows out; a2c_a3c_rollout with
 * states_lazy set on a shape that is not ring-capable returns A2C_ERR_ARG.                                            */
int a2c_a3c_ring_supported(int B, int C, int H, int W, int n_actions, const float *conv1_weight);

/* ------------------------------------------------------------------ b: pinned staging
 * The pool region lives in POSIX shared memory (shm_open name `shm_name`, created by this call)
 * so that env worker processes can map it; it is pinned and mapped into the device's address
 * space with hipHostRegister (no copy): *host_out = the mapping in this process, *dev_out = the
 * address kernels and hipMemcpyAsync use.  Replaces the reference's share_memory_() tensors
 * (training.py:93-101) for the data that crosses the host-device boundary every env step.     */
int a2c_rollout_buffer_create(const char *shm_name, size_t bytes, void **host_out, void **dev_out);
int a2c_rollout_buffer_destroy(const char *shm_name, void *host, size_t bytes);
/* pin + map an existing host range (page aligned) / undo it                                  */
int a2c_pinned_register(void *host, size_t bytes, void **dev_out);
int a2c_pinned_unregister(void *host);
/* Push buffer: fine-grained DEVICE memory that the host writes into directly (large-BAR: *ptr_out is valid on both
 * sides; zero-filled).  The native env worker threads of a pool started with a2c_pool_threads_start_push mirror every
 * answer there (packed / uint8 frame, sfence, rec granule, sfence), and a2c_a3c_rollout / a2c_pool_ingest* given the
 * push addresses poll and fetch from HBM instead of reading host memory over PCIe (training.py:93-101's shared tensors,
 * for the host -> device direction).  A2C_ERR_LAUNCH when the platform refuses the allocation OR the memory is not
 * writable from the host (no large BAR; checked with a guarded probe write that the device reads back).           */
int a2c_push_buffer_alloc(size_t bytes, void **ptr_out);
int a2c_push_buffer_free(void *ptr);
/* host threads waiting in hipStreamSynchronize sleep instead of spinning (hipDeviceScheduleBlockingSync): for
 * nodes where the ranks of a multi-GPU job have fewer CPUs than busy threads.  Call before any other HIP work. */
int a2c_set_blocking_sync(int on);
/* PCI bus id ("0000:c1:00.0") of the current HIP device: the host side places the pinned region and the env
 * workers on the NUMA node the GPU hangs off (/sys/bus/pci/devices/<id>/numa_node)                */
int a2c_device_pci_bus_id(char *out, int len);
/* *dev_ptr = value with one system-scope 4-byte store from the stream (e.g. the phase word of the host pool header,
 * a2c_hostpool.h: the stream itself tells the env workers when a rollout starts and ends, so that they spin only
 * while one is running)                                                                                        */
int a2c_store_u32_system(uint32_t *dev_ptr, uint32_t value, a2c_stream_t stream);
/* hipMemcpyAsync on `stream`: kind 1 = host->device, 2 = device->host, 3 = device->device      */
int a2c_memcpy_async(void *dst, const void *src, size_t bytes, int kind, a2c_stream_t stream);
/* dst[b*dst_stride + j] = src[b*src_stride + j], j < n  (h_states[e] = h, runner.py:201;
 * gathers/scatters of per-step rows of the rollout-major buffers)                       */
int a2c_copy_rows(const float *src, int64_t src_stride, float *dst, int64_t dst_stride, int B,
                  int64_t n, a2c_stream_t stream);
/* x[b, :] *= (1 - dones[b*done_stride])   (hs = hs*(1-dones[:,i]), updater.py:164)      */
int a2c_mask_rows(float *x, int64_t ld, const float *dones, int64_t done_stride, int B, int n,
                  a2c_stream_t stream);
/* dst[(t*R + r)*n + j] = src[(r*T + t)*n + j]: swaps the two leading axes of a (R,T,n) array
 * (rollout-major <-> time-major views of the buffers for the BPTT unroll, updater.py:155-168) */
int a2c_permute_rows(const float *src, float *dst, int64_t R, int64_t T, int64_t n,
                     a2c_stream_t stream);

/* ------------------------------------------------------------------ a8: loss
 * updater.py:100-106,124-127 forward AND backward in one pass over N_local rows:
 *   lsm = log_softmax(logits); log_p = lsm[n, actions[n]];
 *   Entropy = -entr_coef * mean_n sum_a lsm*softmax;  Pi_Loss = -pi_coef * mean(log_p*adv);
 *   ValLoss = val_coef * mean((V-R)^2);  Loss = Pi_Loss + ValLoss - Entropy,
 * means over n_global rows (n_global > n_local when the batch is sharded over GPUs).
 * If adv_sums != NULL the advantages are normalised on the fly as in a2c_normalize
 * (norm_advs, updater.py:97-98) using eps 1e-6.
 * Outputs: dlogits (N, ldd) = dLoss/dlogits, dvals (N) = dLoss/dV,
 * loss_sums[0..2] (double) = sum log_p*adv, sum (V-R)^2, sum_n sum_a p*lsm
 * over the local rows.                                                                  */
int a2c_loss_fwd_bwd(const float *logits, int64_t ld_logits, const float *vals, int64_t val_stride,
                     const int64_t *actions, const float *advs, const float *returns,
                     const double *adv_sums, int64_t n_local, int64_t n_global, int A,
                     float pi_coef, float val_coef, float entr_coef, float *dlogits, int64_t ldd,
                     float *dvals, int64_t dval_stride, double *loss_sums, double *reduce_scratch,
                     a2c_stream_t stream);

/* ------------------------------------------------------------------ a5c: continuous (Gaussian) actions
 * FCModel / GRUFCModel with is_discrete=False (models.py:396-405, 514-524): the heads rows are
 * [mu (n) | raw (n) | value] and sigma = softplus(raw) + 1e-4 (torch threshold 20: raw > 20 gives raw).
 * n (the action dimension) is 1 .. A2C_GAUSS_MAX_N.                                      */
#define A2C_GAUSS_MAX_N 64
/* sigma[b*ld_sigma + j] = sigma (may be NULL); if actions != NULL, actions[b*ld_act + j] = mu + sigma*eps[b*ld_eps + j]
 * rounded like torch's two ops (runner.py:98-104).  B rows of heads with row stride ld_heads (>= 2n).                 */
int a2c_gauss_head(const float *heads, int64_t ld_heads, const float *eps, int64_t ld_eps, float *sigma,
                   int64_t ld_sigma, float *actions, int64_t ld_act, int64_t B, int n, a2c_stream_t stream);
/* a2c_gauss_head that ALSO hands the sampled actions to the env workers of a float-action host pool (a2c_hostpool.h:
 * "CONTINUOUS actions"; runner.py:207-208 env.step(action)) -- same arithmetic, sigma and actions bit-identical.  With
 * s = seq_base[0] + seq_off (modulo 2^32; seq_base in DEVICE memory, so a captured launch replays for later rollouts)
 * the thread that computes action (b, k) stores the granule act[b*act_stride + k] = (s << 32) | float_bits(action) and
 * the thread of k == 0 then the doorbell cmd[b] = (s << 32) | n: system-scope 8-byte stores (act / cmd = device
 * addresses of the registered pinned region).  Every granule carries its own tag, so the worker's acceptance does not
 * depend on the doorbell arriving last.  cmd == NULL: exactly a2c_gauss_head, act / seq_base are not touched.  With
 * cmd != NULL: actions, eps, act, seq_base non-NULL and act_stride >= n.                                         */
int a2c_gauss_head_publish(const float *heads, int64_t ld_heads, const float *eps, int64_t ld_eps, float *sigma,
                           int64_t ld_sigma, float *actions, int64_t ld_act, int64_t B, int n, uint64_t *act,
                           int64_t act_stride, uint64_t *cmd, const uint32_t *seq_base, uint32_t seq_off,
                           a2c_stream_t stream);
/* The reference's Gaussian loss (updater.py:108-117), first of two launches.  With d = mu - a, c = clamp(sigma^2, 1e-3),
 * l = log(clamp(sqrt(2 pi) sigma, 1e-3)) and adv the (optionally normalised, as in a2c_loss_fwd_bwd) advantage:
 * sums[0..5] (double) = sum d^2, sum w/(2c), sum w*l, sum l, sum adv, sum (V-R)^2 over the local rows, where
 * w = adv for n >= 2 and w = 1 for n == 1 (sum adv is only accumulated for n == 1, else 0).  Deterministic (fixed-order
 * grid reduction in reduce_scratch).  When the batch is sharded the six sums are all-reduced before the second launch. */
int a2c_gauss_loss_sums(const float *heads, int64_t ld_heads, const float *vals, int64_t val_stride,
                        const float *actions, int64_t ld_act, const float *advs, const float *returns,
                        const double *adv_sums, int64_t n_local, int64_t n_global, int n, double *sums,
                        double *reduce_scratch, a2c_stream_t stream);
/* Second launch: from the GLOBAL sums (M = n_global*n, mse = sums[0]/M, K and P = sums[1], sums[2], times mean(adv) for
 * n == 1 -- the reference broadcasts (N,1)*(N,) to an N x N product there), writes
 *   dheads[i*ldd + j] = dL/dmu,  dheads[i*ldd + n + j] = dL/draw,  dvals[i*dval_stride] = dL/dV,
 *   loss_sums[0..2] = (-(mse*K + P)/n, sum (V-R)^2, sums[3]/n) * n_local/n_global,
 * so that Updater's host finishing (sum / n_global, summed over the ranks) gives the reference's
 * Pi_Loss = pi_coef*(mse*K + P)/M, ValLoss and Entropy = -entr_coef*sums[3]/M.                                          */
int a2c_gauss_loss_fwd_bwd(const float *heads, int64_t ld_heads, const float *vals, int64_t val_stride,
                           const float *actions, int64_t ld_act, const float *advs, const float *returns,
                           const double *adv_sums, const double *sums, int64_t n_local, int64_t n_global, int n,
                           float pi_coef, float val_coef, float entr_coef, float *dheads, int64_t ldd, float *dvals,
                           int64_t dval_stride, double *loss_sums, a2c_stream_t stream);
/* The per-sample Gaussian log-likelihood loss (hyps["gauss_loss"] = "exact"; NOT the reference's),
 * forward AND backward in ONE launch under the protocol of a2c_loss_fwd_bwd: no batch-wide quantity is needed before the
 * gradients, so a sharded update has no collective here.  With w_i the advantage (normalised as in a2c_loss_fwd_bwd when
 * adv_sums != NULL -- every row its own, for n == 1 too), invN = 1/n_global and, per row i and action dim j,
 *   sigma_ij = softplus(raw_ij) + 1e-4,  u_ij = (a_ij - mu_ij)/sigma_ij,
 *   logp_i = sum_j (-u_ij^2/2 - log sigma_ij - log(2 pi)/2),   H_i = sum_j (1/2 + log(2 pi)/2 + log sigma_ij),
 * it writes
 *   dheads[i*ldd + j]     = dL/dmu_ij  = -pi_coef w_i invN u_ij/sigma_ij,
 *   dheads[i*ldd + n + j] = dL/draw_ij = dL/dsigma_ij * (raw_ij > 20 ? 1 : e^raw/(e^raw + 1)),
 *                           dL/dsigma_ij = -pi_coef w_i invN (u_ij^2 - 1)/sigma_ij - entr_coef invN/sigma_ij,
 *   dvals[i*dval_stride]  = dL/dV_i = val_coef 2 (V_i - R_i) invN,
 *   loss_sums[0..2] (double) = sum_i w_i logp_i, sum_i (V_i - R_i)^2, -sum_i H_i over the local rows,
 * the sums in a2c_loss_fwd_bwd's convention: Pi_Loss = -pi_coef mean(w logp), Entropy = entr_coef mean H and
 * Loss = Pi_Loss + ValLoss - Entropy (the entropy is MAXIMISED, as on the discrete path).  No clamps (sigma >= 1e-4).
 * Deterministic (fixed-order grid reduction in reduce_scratch; at most 1024 workgroups of 256 rows, grid-stride beyond).
 * A2C_ERR_ARG, nothing launched: n outside 1 .. A2C_GAUSS_MAX_N, ld_heads or ldd < 2n, ld_act < n, a NULL pointer;
 * n_local == 0 zeroes loss_sums.                                                                                        */
int a2c_gauss_nll_fwd_bwd(const float *heads, int64_t ld_heads, const float *vals, int64_t val_stride,
                          const float *actions, int64_t ld_act, const float *advs, const float *returns,
                          const double *adv_sums, int64_t n_local, int64_t n_global, int n, float pi_coef,
                          float val_coef, float entr_coef, float *dheads, int64_t ldd, float *dvals,
                          int64_t dval_stride, double *loss_sums, double *reduce_scratch, a2c_stream_t stream);

/* The clipped-ratio (PPO) loss of the multi-epoch update (hyps["ppo_epochs"] >= 2; nothing in the
 * reference): a2c_loss_fwd_bwd (a2c_ppo_loss_fwd_bwd) and a2c_gauss_nll_fwd_bwd (a2c_gauss_ppo_fwd_bwd) with the policy
 * term replaced by the clipped surrogate against the log-probabilities logp_old (n_local doubles) of the policy that
 * collected the rows.  logp_i: lsm[act] (the -1 -> last action rule of a2c_loss_fwd_bwd), or the Gaussian logp_i above,
 * both evaluated in fp64 from the fp32 inputs (the ratio's exponent; the gradients stay the sibling's fp32 formulas);
 * w_i: the advantage, normalised when adv_sums != NULL.
 *   record == 1 (the first epoch: the parameters are the rollout's): logp_old[i] = logp_i is WRITTEN and r_i = 1: dlogits /
 *     dheads, dvals, loss_sums[1] and loss_sums[2] are bit for bit what the sibling writes (the surrogate's gradient at
 *     r = 1 is the policy gradient); loss_sums[0] = sum w_i, loss_sums[3] = loss_sums[4] = 0.
 *   record == 0: logp_old is READ; in fp64 r_i = exp(logp_i - logp_old[i]),
 *     surr_i = min(r_i w_i, clamp(r_i, 1 - clip, 1 + clip) w_i),
 *     keep_i = !((w_i > 0 && r_i > 1 + clip) || (w_i < 0 && r_i < 1 - clip));
 *     the sibling's gradient formulas with g_i = -pi_coef w_i invN replaced by float(g_i r_i) where keep_i and by
 *     exactly 0 where not (a select, not a product: an overflowed r_i on a clipped row makes no NaN); the entropy and value
 *     parts unchanged;  loss_sums[0..4] = sum surr_i, sum (V - R)^2, the sibling's entropy sum, sum (1 - keep_i),
 *     sum ((r_i - 1) - log r_i).  A row with r_i == 1 gets the record-mode outputs bit for bit.
 * Pi_Loss = -pi_coef loss_sums[0] / n_global as for the sibling; loss_sums[3] / n_global is the clipped fraction and
 * loss_sums[4] / n_global an estimate of KL(old || new).  Deterministic (five fp64 partials per workgroup in
 * reduce_scratch: at most 512 workgroups of 256 rows, grid-stride beyond).  A2C_ERR_ARG, nothing launched: whatever the
 * sibling rejects, clip not finite or <= 0, record other than 0 / 1, logp_old == NULL; n_local == 0 zeroes the five
 * loss_sums and writes nothing else.                                                                                    */
int a2c_ppo_loss_fwd_bwd(const float *logits, int64_t ld_logits, const float *vals, int64_t val_stride,
                         const int64_t *actions, const float *advs, const float *returns,
                         const double *adv_sums, int64_t n_local, int64_t n_global, int A,
                         float pi_coef, float val_coef, float entr_coef, float clip, int record, double *logp_old,
                         float *dlogits, int64_t ldd, float *dvals, int64_t dval_stride, double *loss_sums,
                         double *reduce_scratch, a2c_stream_t stream);
int a2c_gauss_ppo_fwd_bwd(const float *heads, int64_t ld_heads, const float *vals, int64_t val_stride,
                          const float *actions, int64_t ld_act, const float *advs, const float *returns,
                          const double *adv_sums, int64_t n_local, int64_t n_global, int n, float pi_coef,
                          float val_coef, float entr_coef, float clip, int record, double *logp_old, float *dheads,
                          int64_t ldd, float *dvals, int64_t dval_stride, double *loss_sums, double *reduce_scratch,
                          a2c_stream_t stream);

/* ------------------------------------------------------------------ a6: dense layers
 * C[M,N] = (accumulate ? C : 0) + opA(A)[M,K] * opB(B)[K,N] (+ bias[N]) ; then optional ReLU ; then optional
 * multiply by (mask[m*ldmask+n] > 0) (the ReLU derivative of the layer below, fused into
 * the producer).  fp32 in / fp32 accumulate on the matrix cores (v_mfma_f32_32x32x2_f32:
 * exact fp32 FMA chain in k order).
 *   transA = 0: A stored [M][lda] (k contiguous);  transA = 1: A stored [K][lda] (m contiguous)
 *   transB = 0: B stored [K][ldb] (n contiguous);  transB = 1: B stored [N][ldb] (k contiguous)
 * splitk > 1 splits K over gridDim.z into partial slabs in ws that a second kernel sums in
 * fixed order (deterministic); ws_bytes >= a2c_gemm_ws_bytes(M,N,splitk).
 * Linear forward  y = x W^T + b  (torch.nn.Linear, models.py:73,84,85 ...): transA=0, transB=1.
 * Linear backward dx = dy W: transA=0, transB=0;  dW = dy^T x: transA=1, transB=0.       */
size_t a2c_gemm_ws_bytes(int64_t M, int64_t N, int splitk);
/* Large products (M, N, K >= 1024 and M N K >= 2e10: ConvModel's 28224 x 2000 layers at update batch, models.py:246-264) run
 * on the BF16 matrix pipe with fp32 results when the workspace also holds a2c_gemm_x9_ws_bytes(M, N, K) bytes BEHIND the
 * a2c_gemm_ws_bytes(M, N, splitk) ones (rounded up to 256): each operand is split, in one pass, into three bf16 images
 * a = a0 + a1 + a2 (exact: 3 x 8 significant bits); the SIX piece products with qa + qb <= 2 are issued (each exact; the
 * three dropped ones are below 2^-24 of |a b|, under the rounding of the fp32 product itself) and every sum is the MFMA's
 * fp32 accumulator's -- nn.Linear's fp32 sum, re-associated, at 6/16 of the fp32 matrix time on paper and 1.7-1.9 x the
 * fp32 kernels measured (DESIGN.md section 4 "bf16 x 6").  A2C_GEMM_X9 moves the threshold (Environment switches).
 * 0: the product does not take that path.  Without the extra bytes a2c_gemm_f32 runs the fp32 MFMA kernels.            */
size_t a2c_gemm_x9_ws_bytes(int64_t M, int64_t N, int64_t K);
int a2c_gemm_f32(int transA, int transB, int64_t M, int64_t N, int64_t K, const float *A,
                 int64_t lda, const float *B, int64_t ldb, float *C, int64_t ldc,
                 const float *bias, int relu, const float *mask, int64_t ldmask, int accumulate,
                 int splitk, void *ws, size_t ws_bytes, a2c_stream_t stream);
/* The same six-product kernel from PREBUILT images (a weight matrix split once per update and used by every step of the
 * rollout: ConvModel's resize_emb at 256 envs, models.py:246): C[M][N] = A[M][K] B[N][K]^T with the epilogue of a2c_gemm_f32.
 *   a2c_gemm_x6_image_bytes  bytes of the image of a rows x K operand (rows padded to 256, K to 16; 16-byte aligned)
 *   a2c_gemm_x6_split        writes it: k_contiguous = 1: src[r * ld + k], 0: src[k * ld + r]; layout
 *                            image[piece][row / 256][k / 16][(k / 8) & 1][row % 256][8] bf16
 *   a2c_gemm_x6_images       the product; splitk = the largest number of K splits allowed (ws_bytes >= splitk * M * N * 4
 *                            when > 1; the kernel takes fewer when the tiles alone fill the chip), slabs summed in fixed order */
size_t a2c_gemm_x6_image_bytes(int64_t rows, int64_t K);
int a2c_gemm_x6_split(const float *src, int64_t ld, int64_t rows, int64_t K, int k_contiguous, void *image,
                      a2c_stream_t stream);
int a2c_gemm_x6_images(int64_t M, int64_t N, int64_t K, const void *image_a, const void *image_b, float *C, int64_t ldc,
                       const float *bias, int relu, const float *mask, int64_t ldmask, int accumulate, int splitk, void *ws,
                       size_t ws_bytes, a2c_stream_t stream);
/* Split-K phase only: writes `a2c_gemm_splits(K, splitk)` partial slabs [split][M][N] (dense,
 * no epilogue) into ws and leaves the fixed-order sum to the consumer (a2c_heads_fused).   */
int a2c_gemm_splits(int64_t K, int splitk);
/* dx[m, k] = (sum_{n < N} dy[m*ldy + n] * W[n*K + k]) * bit(m, k), N <= 8: the skinny input-gradient product of
 * a2c_gemm_f32 (transA = transB = 0, K <= 8 there) with the ReLU mask of the layer below given as ONE BIT per activation
 * -- bit (k & 7) of byte maskbits[m*mask_row_bytes + (k >> 3)] = (act[m][k] > 0) -- instead of the fp32 activation itself
 * (A3CModel's da2 = (dl . Wc[:A]) * (a2 > 0), models.py:73-85 through autograd: 340 MB of mask reads per update become
 * 10 MB).  The same FMA order as a2c_gemm_f32's path: bit-identical results.  K % 8 == 0, ldx % 4 == 0, W and dx 16-byte
 * aligned.  Producer of the bits: a2c_a3c_rollout's ring kernel (a2_maskbit_rows).                                  */
int a2c_small_n_bwd_data_bits(const float *dy, int64_t ldy, const float *W, float *dx, int64_t ldx,
                              const uint8_t *maskbits, int64_t mask_row_bytes, int64_t M, int N, int64_t K,
                              a2c_stream_t stream);
int a2c_gemm_f32_partial(int transA, int transB, int64_t M, int64_t N, int64_t K, const float *A,
                         int64_t lda, const float *B, int64_t ldb, int splitk, void *ws,
                         size_t ws_bytes, a2c_stream_t stream);
/* Fused tail of a forward pass (A3CModel: proj_matrx epilogue + pi/value heads + action sampling,
 * models.py:73,84-85 + runner.py:94-97), one wave per row m:
 *   x[m,:]  = sum_z xs[z*slab_stride + m*ldx + :]  (z < nslab, fixed order) + bias_in  [ReLU]
 *   (optionally stored to emb_out[m*ld_emb + :])
 *   heads[m*ldh + n] = x[m,:] . W[n,:] + b[n]          n < N <= 8, W stored [N][K]
 *   if u != NULL: actions[m*act_stride] = inverse-CDF sample of softmax(heads[m, :n_logits])
 * K % 4 == 0, 16 B aligned rows.                                                          */
int a2c_heads_fused(const float *xs, int nslab, int64_t slab_stride, int64_t ldx,
                    const float *bias_in, int relu_in, float *emb_out, int64_t ld_emb,
                    const float *W, const float *b, float *heads, int64_t ldh, int64_t M, int N,
                    int K, const float *u, int n_logits, int64_t *actions, int64_t act_stride,
                    a2c_stream_t stream);
/* a2c_heads_fused whose sampling thread also hands the action to the env worker (the device relay's
 * a2c_pool_publish_actions, runner.py:129-131 "pipe.send(action)"): with cmd != NULL (needs u)
 *   cmd[m] = ((seq_base[0] + seq_off) << 32) | action[m]       one system-scope 8-byte store per row
 * cmd == NULL is a2c_heads_fused.                                                            */
int a2c_heads_fused_publish(const float *xs, int nslab, int64_t slab_stride, int64_t ldx,
                            const float *bias_in, int relu_in, float *emb_out, int64_t ld_emb,
                            const float *W, const float *b, float *heads, int64_t ldh, int64_t M,
                            int N, int K, const float *u, int n_logits, int64_t *actions,
                            int64_t act_stride, uint64_t *cmd, const uint32_t *seq_base,
                            uint32_t seq_off, a2c_stream_t stream);
int a2c_gemm_f32_nt(int64_t M, int64_t N, int64_t K, const float *A, int64_t lda, const float *B,
                    int64_t ldb, float *C, int64_t ldc, const float *bias, int relu,
                    a2c_stream_t stream);
int a2c_gemm_f32_nn(int64_t M, int64_t N, int64_t K, const float *A, int64_t lda, const float *B,
                    int64_t ldb, float *C, int64_t ldc, const float *mask, int64_t ldmask,
                    a2c_stream_t stream);
int a2c_gemm_f32_tn(int64_t M, int64_t N, int64_t K, const float *A, int64_t lda, const float *B,
                    int64_t ldb, float *C, int64_t ldc, int splitk, void *ws, size_t ws_bytes,
                    a2c_stream_t stream);
/* Inference-only composition of two stacked nn.Linear layers with NO activation in between
 * (A3CModel: emb = proj_matrx(flat), then pi(emb) / value(emb); models.py:73, 84-85):
 *   Wc (N x F) = Wh (N x H) . Wp (H x F)        bc (N) = Wh . bp + bh
 * so that [logits | value] = flat . Wc^T + bc in one skinny layer (a2c_heads_fused / a2c_a3c_step).
 * N <= 8.  Rebuilt after every optimiser step; the update keeps the exact two-layer path.        */
int a2c_compose_heads(const float *Wh, const float *bh, const float *Wp, const float *bp, float *Wc,
                      float *bc, int N, int H, int F, a2c_stream_t stream);
/* out[n] = sum_m x[m*ld + n]   (bias gradients), deterministic two-stage reduction;
 * ws_bytes >= a2c_colsum_ws_bytes(N)                                                    */
size_t a2c_colsum_ws_bytes(int64_t N);
int a2c_colsum(const float *x, int64_t ld, int64_t M, int64_t N, float *out, void *ws,
               size_t ws_bytes, a2c_stream_t stream);

/* ------------------------------------------------------------------ a6: convolutions
 * torch.nn.Conv2d (+ReLU) of the model classes (models.py:98,312,685), NCHW fp32,
 * square kernel ks, stride, zero padding pad.  LDS-staged input tiles, implicit-GEMM inner
 * product on the fp32 matrix cores (v_mfma_f32_16x16x4_f32).
 * `in` samples are addressed with a per-sample stride in floats (so a forward can read
 * states[idx*T+t] straight out of the rollout buffer); planes are contiguous H*W.
 * Constraints: Cin % 4 == 0, Cout % 4 == 0 (true for every reference layer).
 * wprep holds the weights re-laid as matrix-core A fragments; build it with
 * a2c_conv2d_prep_weights after every optimiser step (sizes from a2c_conv2d_prep_floats).
 *   kind 0: forward fragments      kind 1: backward-data fragments                      */
typedef struct {
  int Cin, H, W;      /* input planes and size              */
  int Cout, ks, stride, pad;
  int OH, OW;         /* output size = (H - ks + 2 pad)/stride + 1 */
} a2c_conv_desc;
size_t a2c_conv2d_prep_floats(const a2c_conv_desc *d, int kind);
int a2c_conv2d_prep_weights(const a2c_conv_desc *d, int kind, const float *weight, float *wprep,
                            a2c_stream_t stream);
/* out = relu?(conv(in, W) + bias)                                                       */
int a2c_conv2d_fwd(const a2c_conv_desc *d, const float *in, int64_t in_bstride,
                   const float *wprep_fwd, const float *bias, int relu, float *out,
                   int64_t out_bstride, int B, a2c_stream_t stream);
/* din = conv_transpose(dout, W), then optionally din *= (mask > 0) where mask is the
 * (B,Cin,H,W) activation that fed this conv (the ReLU below it)                          */
int a2c_conv2d_bwd_data(const a2c_conv_desc *d, const float *dout, const float *wprep_bwd,
                        const float *mask, float *din, int B, a2c_stream_t stream);
/* The ReLU mask as SIGN WORDS.  For the 3x3 layers of the conv-stack models the forward can leave, next to `out`, one
 * bit per activation: bit (x & 31) of word signs[b*signs_bstride + (c*OH + y)*ceil(OW/32) + (x >> 5)] = (out[b][c][y][x] > 0).
 * a2c_conv2d_bwd_data_signs of the layer ABOVE takes them in place of the float mask (din *= bit): 1/32 of the mask's
 * HBM reads, same result bit for bit.  a2c_conv2d_sign_words(d) = words per sample of d's output, 0 when d's forward
 * cannot write them (then use a2c_conv2d_fwd and the float mask); a2c_conv2d_bwd_data_signs_supported(d) = 1 when d's
 * backward-data can read the sign words of ITS INPUT ([Cin][H][ceil(W/32)] words per sample); signs == NULL: no mask. */
int64_t a2c_conv2d_sign_words(const a2c_conv_desc *d);
int a2c_conv2d_fwd_signs(const a2c_conv_desc *d, const float *in, int64_t in_bstride, const float *wprep_fwd,
                         const float *bias, int relu, float *out, int64_t out_bstride, uint32_t *signs,
                         int64_t signs_bstride, int B, a2c_stream_t stream);
int a2c_conv2d_bwd_data_signs_supported(const a2c_conv_desc *d);
/* The ReLU mask as one bit per activation, in the layout a wavefront writes without packing work ("lane masks"; the streaming
 * backward-data kernel of the 4x4 / stride-2 layer of A3CModel, models.py:35-37).  lanemask = (B, Cin*H*W/64) 64-bit words =
 * Cin*H*W/8 bytes per sample: bit (i & 7) of byte (i >> 3) = (act[b][i] > 0), i the flat (c, y, x) index -- the four bits of
 * a lane's float4 are one nibble, two neighbouring lanes make a byte.  Producers: a2c_a3c_rollout's ring kernel
 * (a1_lanemask_rows) or a2c_lanemask_from_act over any tensor whose float count is a multiple of 256.
 * din = conv_transpose(dout, W) * bit: the same values as a2c_conv2d_bwd_data with the float mask, bit for bit, for 1/32 of
 * the mask's HBM reads -- at any A2C_BWD_X6 setting: both calls take the same kernel for the layer, batch and switch
 * (the bf16 six-product kernel by default, the fp32 MFMA streaming kernel with A2C_BWD_X6=0), only the mask's encoding
 * differs.  _supported(d, B) = 1 when a2c_conv2d_bwd_data_lanemask can run (layer shape, Cin*H*W % 256 == 0,
 * B large enough for the streaming kernel); otherwise use a2c_conv2d_bwd_data with the float mask.                     */
int a2c_lanemask_from_act(const float *act, uint64_t *lanemask, int64_t n_floats, a2c_stream_t stream);
int a2c_conv2d_bwd_data_lanemask_supported(const a2c_conv_desc *d, int B);
int a2c_conv2d_bwd_data_lanemask(const a2c_conv_desc *d, const float *dout, const float *wprep_bwd, const uint64_t *lanemask,
                                 float *din, int B, a2c_stream_t stream);
/* The same layer below a rank-n_logits head (A3CModel's update: updater.py:128's autograd through pi(emb), proj_matrx and the
 * ReLU of conv2, models.py:35-37, 73, 84): the layer's dOut is never materialised.  With Wc = pi.weight proj_matrx.weight
 * (n_logits x Cout*OH*OW, a2c_compose_heads) and the ReLU mask of the layer's OUTPUT as one bit per activation (maskbits:
 * bit e & 7 of byte e >> 3 of a row of mask_row_bytes bytes, e the flat (co, oy, ox) index; the ring kernel's a2_maskbit_rows),
 *     dOut[b][e] = (act[b][e] > 0) ? sum over n < n_logits of dl[b * ld_dl + n] * Wc[n][e] : 0
 * is formed while a sample is staged -- the sums of a2c_small_n_bwd_data_bits (n ascending, separate multiply and add), so both
 * passes return bit for bit what they return on that entry point's output -- by
 *   a2c_conv2d_bwd_data_lanemask_rank   din = conv_transpose(dOut, W) * bit(lanemask)            (bwd_x6_kernel)
 *   a2c_conv2d_bwd_weight_rank          dW = sum dOut (x) patches(in), db = sum dOut             (wgrad_x6_kernel)
 * both on the bf16 matrix pipe as six exact piece products with fp32 sums.  _supported = 1 for A3CModel's conv2
 * (16 x 20 x 20 -> 32 x 9 x 9, 4 x 4, stride 2) at streaming batch with n_logits <= 4; otherwise form dOut with
 * a2c_small_n_bwd_data_bits and call the plain entry points.                                                            */
int a2c_conv2d_bwd_rank_supported(const a2c_conv_desc *d, int n_logits, int B);
int a2c_conv2d_bwd_data_lanemask_rank(const a2c_conv_desc *d, const float *dl, int64_t ld_dl, int n_logits, const float *Wc,
                                      const uint8_t *maskbits, int64_t mask_row_bytes, const float *wprep_bwd,
                                      const uint64_t *lanemask, float *din, int B, a2c_stream_t stream);
int a2c_conv2d_bwd_weight_rank(const a2c_conv_desc *d, const float *in, int64_t in_bstride, const float *dl, int64_t ld_dl,
                               int n_logits, const float *Wc, const uint8_t *maskbits, int64_t mask_row_bytes, float *dW,
                               float *db, int B, void *ws, size_t ws_bytes, a2c_stream_t stream);
int a2c_conv2d_bwd_data_signs(const a2c_conv_desc *d, const float *dout, const float *wprep_bwd, const uint32_t *signs,
                              int64_t signs_bstride, float *din, int B, a2c_stream_t stream);
/* a2c_conv2d_bwd_data_signs of layer d2 FUSED with a2c_conv2d_bwd_weight_frames of the FIRST layer d1 below it (round 6;
 * GRUModel's conv2 over conv1, models.py:570-590: 16 <- 24 channels at stride 2 on 84 x 84 over 4 -> 16, 3 x 3, stride 1,
 * pad 1).  The first layer's input needs no gradient, so layer 2's masked input gradient (the `din` of the unfused call:
 * 16 x 84 x 84 floats per sample, 14.8 GB at N = 32,768) feeds nothing but d1's weight gradient: the kernel keeps each finished
 * band of it in LDS, splits it into three exact bf16 pieces in registers and multiplies it against the band's rows of the
 * uint8 frames (exact in bf16) on the bf16 matrix pipe -- it is never written to HBM and never read back (the two unfused
 * launches move 29.6 GB for it).  dW1 (16, 4, 3, 3), db1 (16): the sums of a2c_conv2d_bwd_weight_frames over
 * a2c_conv2d_bwd_data_signs's output, re-associated; per-workgroup partials in ws + a fixed-order reduction (deterministic).
 * signs = the sign words of d1's OUTPUT (a2c_conv2d_fwd_signs / a2c_conv2d_fwd_frames), frame_store / nvalid as in
 * a2c_conv2d_bwd_weight_frames.  _ws_bytes returns 0 when the pair of layers has no fused kernel (then use the two calls). */
size_t a2c_conv2d_bwd_data_w1_frames_ws_bytes(const a2c_conv_desc *d2, const a2c_conv_desc *d1, int B);
int a2c_conv2d_bwd_data_w1_frames(const a2c_conv_desc *d2, const float *dout, const float *wprep_bwd, const uint32_t *signs,
                                  int64_t signs_bstride, const a2c_conv_desc *d1, const uint8_t *frame_store,
                                  int64_t slot_stride, int64_t T, const int32_t *nvalid, float *dW1, float *db1, int B,
                                  void *ws, size_t ws_bytes, a2c_stream_t stream);
/* a2c_conv2d_bwd_data of layer d2 FUSED with a2c_conv2d_bwd_weight of the layer d1 below it, for the case where
 * nothing but d1's weight gradient reads d2's input gradient (d1 = first conv of the stack: models.py:196-215, its
 * input needs no gradient): the masked input gradient (the `din` of the call above) is assembled band by band
 * in LDS, multiplied against the band's rows of d1's input x on the matrix cores and dropped -- it is never
 * written to HBM.  dW1 (d1.Cout, d1.Cin, 3, 3), db1 (d1.Cout): the same sums as the two separate calls, per-workgroup
 * partials in ws + fixed-order reduction.  Applies when d1 is 3x3 / stride 1 / pad 1 with d1.Cin*9 <= 48,
 * d1.Cout == d2.Cin <= 16, d2.W % 4 == 0: _ws_bytes returns 0 when it does not (then use the two calls).         */
size_t a2c_conv2d_bwd_data_w1_ws_bytes(const a2c_conv_desc *d2, const a2c_conv_desc *d1, int B);
int a2c_conv2d_bwd_data_w1(const a2c_conv_desc *d2, const float *dout, const float *wprep_bwd,
                           const float *mask, const a2c_conv_desc *d1, const float *x, int64_t x_bstride,
                           float *dW1, float *db1, int B, void *ws, size_t ws_bytes, a2c_stream_t stream);
/* dW (Cout,Cin,ks,ks) and db (Cout) summed over the batch: per-workgroup partial slabs in
 * ws + fixed-order reduction (deterministic).                                            */
size_t a2c_conv2d_bwd_weight_ws_bytes(const a2c_conv_desc *d, int B);
int a2c_conv2d_bwd_weight(const a2c_conv_desc *d, const float *in, int64_t in_bstride,
                          const float *dout, float *dW, float *db, int B, void *ws,
                          size_t ws_bytes, a2c_stream_t stream);
/* The same for the first layer of the A3CModel-shaped nets (8x8 / stride 4 on 4 stacked frames) with the
 * input taken from the single-frame uint8 store a2c_a3c_rollout leaves (stack-on-load: 28 KB of uint8 per
 * sample instead of the 113 KB fp32 state; identical fp32 values, identical summation order): sample
 * n = r*T + t reads frames[r][t .. t+3], planes c < 4 - nvalid[n] are zero.                              */
int a2c_conv2d_bwd_weight_frames(const a2c_conv_desc *d, const uint8_t *frame_store, int64_t slot_stride,
                                 int64_t T, const int32_t *nvalid, const float *dout, float *dW,
                                 float *db, int B, void *ws, size_t ws_bytes, a2c_stream_t stream);
/* A CHAIN of conv + ReLU layers of one rollout step in ONE launch (models.py:648-652: `self.features(x)` of GRUModel,
 * i.e. nn.Sequential over the conv blocks of models.py:570-636): layer i reads layer i-1's output (in / in_bstride for
 * layer 0), writes out[i] (+ b * out_bstride[i] per sample; the rollout passes rows of the update's activation stash) and
 * results are BIT-IDENTICAL to n_layers calls of a2c_conv2d_fwd[_signs] -- same tiles, same summation order; one workgroup
 * walks one sample through all layers, so no launch boundary (fill + tail per launch, 16-58 us each at 256 envs) sits
 * between them.  signs (may be NULL) / signs[i] (may be NULL): sign words of layer i's output (rows of signs_bstride[i]
 * words), as a2c_conv2d_fwd_signs writes them; supported for layer 0, or layers 0 and 1.
 * a2c_conv2d_fwd_chain_supported: 1 for the layer runs that have such a kernel (GRUModel conv2 .. conv5: 16 -> 24 @84,
 * 24 -> 32 @42, 32 -> 48 @21, 48 -> 64 @11, 3x3 / stride 2 / pad 1; A2C_NO_CHAIN=1 switches it off), else the caller
 * launches layer by layer.  wprep_fwd[i]: a2c_conv2d_prep_weights(kind 0) of layer i.                                */
#define A2C_CONV_CHAIN_MAX 8
int a2c_conv2d_fwd_chain_supported(const a2c_conv_desc *d, int n_layers);
int a2c_conv2d_fwd_chain(const a2c_conv_desc *d, int n_layers, const float *in, int64_t in_bstride,
                         const float *const *wprep_fwd, const float *const *bias, int relu, float *const *out,
                         const int64_t *out_bstride, uint32_t *const *signs, const int64_t *signs_bstride, int B,
                         a2c_stream_t stream);
/* ... and, with the same signature, for the first layer of the 3x3 stacks (ConvModel / GRUModel: 4 -> 16 channels at
 * 84 x 84, models.py:201-207, 570-576).  Their FORWARD with the input stacked on load (rollout step: sample b reads the
 * window frame_store + b * sample_stride, T = 1, nvalid[b * nvalid_stride]; in general sample n reads
 * frame_store + (n / T) * sample_stride + (n % T) * H * W): the loader waves of the streaming kernel expand the bytes to
 * the fp32 image, planes c < 4 - nvalid are zero; everything else is a2c_conv2d_fwd[_signs] (signs may be NULL).
 * a2c_conv2d_fwd_frames_supported: 1 when the layer has such a kernel (else: a2c_frames_to_states + a2c_conv2d_fwd).  */
int a2c_conv2d_fwd_frames_supported(const a2c_conv_desc *d);
int a2c_conv2d_fwd_frames(const a2c_conv_desc *d, const uint8_t *frame_store, int64_t sample_stride, int64_t T,
                          const int32_t *nvalid, int64_t nvalid_stride, const float *wprep_fwd, const float *bias,
                          int relu, float *out, int64_t out_bstride, uint32_t *signs, int64_t signs_bstride, int B,
                          a2c_stream_t stream);

/* ------------------------------------------------------------------ a6: GRU cell, LayerNorm
 * models.GRU.forward (models.py:465-476) given the six pre-activation products:
 *   gx = x [Wx0|Wx1|Wx2] (B,3h),  gh = h [Wh0|Wh1] (B,2h),  and, after r is known,
 *   rh_u = (r*h) Wh2 (B,h).  Two elementwise stages around the (r*h) GEMM:
 *   stage1: z = sig(gx0+gh0+b0), r = sig(gx1+gh1+b1), rh = r*h
 *   stage2: c = tanh(gx2 + rh_u + b2), h_new = z*h + (1-z)*c                             */
int a2c_gru_gates(const float *gx, const float *gh, const float *b, const float *h, float *z,
                  float *r, float *rh, int B, int hdim, a2c_stream_t stream);
int a2c_gru_out(const float *gx, const float *rh_u, const float *b, const float *h,
                const float *z, float *c, float *h_new, int B, int hdim, a2c_stream_t stream);
/* The whole cell forward of one rollout step (models.py:465-476 at batch n_envs) in two launches instead of five:
 * x (B, xs; row stride ldx) and h (B, hdim) -> z, r, rh = r*h, c (may be NULL), h_new (may alias h: the in-place rollout
 * step), with WxC = [W_x[0] | W_x[1] | W_x[2]] (xs, 3 hdim), WhC = [W_h[0] | W_h[1]] (hdim, 2 hdim), Wh2 = W_h[2] and
 * b (3 hdim).  gx (B, 3 hdim) is scratch (its candidate columns carry x W_x[2] between the launches).  Bit-identical to
 * a2c_gemm_f32 (x WxC, h WhC) + a2c_gru_gates + a2c_gemm_f32 (rh Wh2) + a2c_gru_out.  hdim % 32 == 0, xs % 8 == 0.    */
int a2c_gru_cell_fwd(const float *x, int64_t ldx, const float *h, const float *WxC, const float *WhC,
                     const float *Wh2, const float *b, float *gx, float *z, float *r, float *rh, float *c,
                     float *h_new, int B, int xs, int hdim, a2c_stream_t stream);
/* backward of stage2: given dh_new (B,h): dc_pre = dh_new*(1-z)*(1-c^2) (B,h) ;
 * dz = dh_new*(h - c) ; dh_direct = dh_new*z                                            */
int a2c_gru_out_bwd(const float *dh_new, const float *h, const float *z, const float *c,
                    float *dc_pre, float *dz, float *dh, int B, int hdim, a2c_stream_t stream);
/* the same inside the BPTT unroll (updater.py:161-166 walked backwards): dh_new is replaced by dh_new + carry * (1 - done[b]),
 * carry (B,h) = the gradient that reached the next step's h_in = h_new * (1 - done) (done[b] = dones[b * done_stride]);
 * one launch instead of mask_rows + add + gru_out_bwd, same values.  carry may be dh (in place).                   */
int a2c_gru_out_bwd_carry(const float *dh_new, const float *carry, const float *dones, int64_t done_stride,
                          const float *h, const float *z, const float *c, float *dc_pre, float *dz, float *dh,
                          int B, int hdim, a2c_stream_t stream);
/* backward of stage1: d_rh (B,h) from the Wh2 GEMM; dz from above:
 * dz_pre = dz*z*(1-z) ; dr = d_rh*h ; dr_pre = dr*r*(1-r) ; dh += d_rh*r               */
int a2c_gru_gates_bwd(const float *d_rh, const float *dz, const float *h, const float *z,
                      const float *r, float *dz_pre, float *dr_pre, float *dh, int B, int hdim,
                      a2c_stream_t stream);
/* One step of the BPTT unroll's backward (updater.py:139-169 differentiated) in two launches instead of five; bit-identical
 * to a2c_gru_out_bwd[_carry] + a2c_gemm_f32 (dc_pre Wh[2]^T) + a2c_gru_gates_bwd + two accumulating a2c_gemm_f32
 * (dz_pre Wh[0]^T, dr_pre Wh[1]^T):  g = dh_new + carry * (1 - dones[b * done_stride]) (carry may be NULL);
 * dc_pre = g (1-z)(1-c^2), dz = g (h - c), d_rh = dc_pre Wh[2]^T, dz_pre = dz z (1-z), dr_pre = d_rh h r (1-r),
 * dh = g z + d_rh r + dz_pre Wh[0]^T + dr_pre Wh[1]^T.  Wh = gru.W_h (3, hdim, hdim); carry must not alias dh.        */
int a2c_gru_cell_bwd(const float *dh_new, const float *carry, const float *dones, int64_t done_stride,
                     const float *h, const float *z, const float *r, const float *c, const float *Wh,
                     float *dc_pre, float *dz, float *dz_pre, float *dr_pre, float *dh, int B, int hdim,
                     a2c_stream_t stream);
/* torch.nn.LayerNorm over the last dim n (eps 1e-5), FCModel value head (models.py:392) */
int a2c_layernorm_fwd(const float *x, const float *w, const float *b, float *y, float *mean,
                      float *rstd, int64_t rows, int n, a2c_stream_t stream);
int a2c_layernorm_bwd(const float *dy, const float *x, const float *w, const float *mean,
                      const float *rstd, float *dx, float *dw_rows, int64_t rows, int n,
                      int accumulate_dx, a2c_stream_t stream);

/* ------------------------------------------------------------------ a9: clip + optimiser
 * sumsq[0] (double, zeroed by the call) = sum g^2 over the flat gradient arena
 * (nn.utils.clip_grad_norm_, updater.py:129).                                           */
int a2c_gradnorm_sq(const float *grads, int64_t n, double *sumsq, double *reduce_scratch, a2c_stream_t stream);
/* clip (coef = min(1, max_norm/(norm+1e-6)), grads scaled in place like torch) and
 * torch.optim.RMSprop step (alpha, eps; momentum 0, not centered): updater.py:131,227-228 */
int a2c_clip_rmsprop(float *params, float *grads, float *square_avg, int64_t n,
                     const double *sumsq, double max_norm, double lr, double alpha, double eps,
                     float *norm_out, a2c_stream_t stream);
/* same with torch.optim.Adam (beta1, beta2, eps, no amsgrad); step = 1-based step count */
int a2c_clip_adam(float *params, float *grads, float *exp_avg, float *exp_avg_sq, int64_t n,
                  const double *sumsq, double max_norm, double lr, double beta1, double beta2,
                  double eps, int64_t step, float *norm_out, a2c_stream_t stream);
/* the same clip fused with the step of the other torch.optim optimisers, torch's defaults for every setting that is
 * not an argument (no momentum, no weight decay apart from AdamW's, no maximize / amsgrad).  One launch each, same
 * validation as a2c_clip_adam: A2C_ERR_ARG on a NULL or non-16-B-aligned array or step < 1, n == 0 is a no-op.
 * Step-dependent scalars are host doubles; `step` is the 1-based step count.                                   */
int a2c_clip_sgd(float *params, float *grads, int64_t n, const double *sumsq, double max_norm, double lr,
                 float *norm_out, a2c_stream_t stream);
/* clr = lr / (1 + (step-1) lr_decay) */
int a2c_clip_adagrad(float *params, float *grads, float *sum, int64_t n, const double *sumsq, double max_norm,
                     double lr, double lr_decay, double eps, int64_t step, float *norm_out, a2c_stream_t stream);
int a2c_clip_adadelta(float *params, float *grads, float *square_avg, float *acc_delta, int64_t n,
                      const double *sumsq, double max_norm, double lr, double rho, double eps, float *norm_out,
                      a2c_stream_t stream);
/* step_size must hold lr before the first step (torch fills it then); grads keep the clipped, UNmasked gradient */
int a2c_clip_rprop(float *params, float *grads, float *prev, float *step_size, int64_t n, const double *sumsq,
                   double max_norm, double etaminus, double etaplus, double step_size_min, double step_size_max,
                   float *norm_out, a2c_stream_t stream);
/* params *= 1 - lr weight_decay, then the Adam step */
int a2c_clip_adamw(float *params, float *grads, float *exp_avg, float *exp_avg_sq, int64_t n,
                   const double *sumsq, double max_norm, double lr, double beta1, double beta2, double eps,
                   double weight_decay, int64_t step, float *norm_out, a2c_stream_t stream);
int a2c_clip_adamax(float *params, float *grads, float *exp_avg, float *exp_inf, int64_t n, const double *sumsq,
                    double max_norm, double lr, double beta1, double beta2, double eps, int64_t step,
                    float *norm_out, a2c_stream_t stream);
/* mu_product = the fp32 state value after this step's mu_product *= mu */
int a2c_clip_nadam(float *params, float *grads, float *exp_avg, float *exp_avg_sq, int64_t n,
                   const double *sumsq, double max_norm, double lr, double beta1, double beta2, double eps,
                   double momentum_decay, int64_t step, double mu_product, float *norm_out,
                   a2c_stream_t stream);
int a2c_clip_radam(float *params, float *grads, float *exp_avg, float *exp_avg_sq, int64_t n,
                   const double *sumsq, double max_norm, double lr, double beta1, double beta2, double eps,
                   int64_t step, float *norm_out, a2c_stream_t stream);
/* eta, mu = the fp32 state values the previous step stored (lr and 1 before the first) */
int a2c_clip_asgd(float *params, float *grads, float *ax, int64_t n, const double *sumsq, double max_norm,
                  double lambd, double eta, double mu, float *norm_out, a2c_stream_t stream);

/* ---- capturable Adam family: step count and step-dependent scalars in device memory (torch's capturable=True).
 * The launchers above take `step` (and NAdam's mu_product, ASGD's eta / mu) as HOST arguments, so a hipGraph replay would
 * repeat the captured step's bias corrections for ever.  Here they live in one per-optimiser device block:
 * a2c_optim_advance increments the step and recomputes the scalars on the device, a2c_clip_step_dev is the same step
 * kernel with its scalars read from the block.  [advance, step] can be captured and replayed; eager runs are the same two
 * launches.  The block is A2C_OPTIM_BLOCK_BYTES of device memory, 16-byte aligned.  To start or restore an optimiser write
 * step, mu_product, eta and mu (a2c_memcpy_async or any copy; zero the rest): a fresh block is step 0, mu_product 1,
 * eta (float)lr, mu 1.  Everything from `rectify` on is overwritten by every advance.
 *
 *   offset  field       written by advance for        meaning
 *    0      step        all (step += 1)               int64, steps taken
 *    8      mu_product  NAdam (*= (float)mu)          running fp32 state, torch's 0-d `mu_product`
 *   12      eta         ASGD                          running fp32 state stored at the END of step `step` (torch's `eta`)
 *   16      mu          ASGD                          running fp32 state stored at the END of step `step` (torch's `mu`)
 *   20      rectify     RAdam                         int32, rho_t > 5
 *   24      mu_is_one   ASGD                          int32, mu_used == 1
 *   28      step_size   Adam, AdamW                   lr / (1 - beta1^step)
 *   32      bc2_sqrt    Adam, AdamW, RAdam            sqrt(1 - beta2^step)
 *   36      neg_clr     Adamax                        -lr / (1 - beta1^step)
 *   40      bc2         NAdam                         1 - beta2^step
 *   44      c_grad      NAdam                         -lr (1 - mu) / (1 - mu_product)
 *   48      c_avg       NAdam                         -lr mu_next / (1 - mu_product mu_next)
 *   52      bc1         RAdam                         1 - beta1^step
 *   56      rect        RAdam                         the rectification term (0 unless rectify)
 *   60      decay       AdamW: 1 - lr weight_decay    ASGD: 1 - lambd eta_used
 *   64      neg_eta     ASGD                          -eta_used   (eta_used / mu_used: what step - 1 stored)
 *   68      mu_used     ASGD
 *   72      lr          all                           the hyper-parameters of the advance, rounded to fp32 as the
 *   76      omb1        all   1 - beta1               launchers above round them
 *   80      beta2       all
 *   84      omb2        all   1 - beta2
 *   88      eps         all
 *   92      (padding)                                                                                                  */
#define A2C_OPTIM_BLOCK_BYTES 96
typedef struct a2c_optim_block {
  int64_t step;
  float mu_product, eta, mu;
  int32_t rectify, mu_is_one;
  float step_size, bc2_sqrt, neg_clr, bc2, c_grad, c_avg, bc1, rect, decay, neg_eta, mu_used;
  float lr, omb1, beta2, omb2, eps;
  float pad_;
} a2c_optim_block;
enum { A2C_OPTIM_ADAM = 0, A2C_OPTIM_ADAMW = 1, A2C_OPTIM_ADAMAX = 2, A2C_OPTIM_NADAM = 3, A2C_OPTIM_RADAM = 4,
       A2C_OPTIM_ASGD = 5 };
/* One launch of one wavefront; one lane does the work in double with the formulas (and their order) of a2c_clip_adam /
 * _adamw / _adamax / _nadam / _radam / _asgd and of torch's fp32 running state (mu_product *= (float)mu; eta, mu).  The
 * hyper-parameters are arguments of THIS launch: a capture fixes them, as it fixes lr for RMSprop.  Arguments a kind does
 * not use are ignored.  A2C_ERR_ARG on a NULL or non-16-B-aligned block or an unknown kind.                          */
int a2c_optim_advance(int kind, void *block, double lr, double beta1, double beta2, double eps, double weight_decay,
                      double momentum_decay, double lambd, double alpha, double t0, a2c_stream_t stream);
/* The clip + step launch of `kind` (same kernel body and element arithmetic as a2c_clip_<kind>, same bytes per parameter)
 * with the rule's scalars read from the block inside the kernel.  state_b is ignored for ASGD.  Validation as
 * a2c_clip_adam (NULL or non-16-B-aligned arrays: A2C_ERR_ARG; n == 0: no-op), plus the block checks of the advance.    */
int a2c_clip_step_dev(int kind, float *params, float *grads, float *state_a, float *state_b, int64_t n,
                      const double *sumsq, double max_norm, const void *block, float *norm_out, a2c_stream_t stream);

/* out5 = [loss_sums[0..2], grad_norm, err]: the five scalars update_model reads back (updater.py:134-136)
 * gathered into ONE device buffer for a single D2H copy                                  */
int a2c_pack_update_scalars(const double *loss_sums, const float *grad_norm, const int *err,
                            double *out5, a2c_stream_t stream);

/* ------------------------------------------------------------------ Snake worlds in device memory (csrc/snake.hip)
 * The reference's third env family (gym-snake; preprocessing.py:25-32 snake_prep) with this project's own rules
 * (DESIGN.md "Snake"; the host twin a2c_amd/snake.py produces the same integers).  A world is G x G cells (4 <= G <= 32)
 * drawn as unit x unit pixel blocks (1 <= unit <= 16, (G*unit)^2 % 4 == 0) with n_foods foods (1 <= n_foods < G*G - 3);
 * anything else returns A2C_ERR_ARG without a launch.  Env e of a launch is world env_id0 + e of `seed`: draw i of a
 * world is hash32(seed, env_id, i).  The state of one env is a2c_snake_state_bytes int32 words: head row, head col,
 * length, draw counter, step counter, episode reward, 2 spare, then the G*G cells (0 free, -1 food, n > 0 occupied for
 * n more steps).  The kernels advance the counters in device memory, so a captured launch plays new steps at each replay.
 * a2c_snake_state_bytes: bytes of ONE env's state, 0 for an unsupported G / n_foods.                                  */
size_t a2c_snake_state_bytes(int G, int n_foods);
/* starts B worlds (counters to 0, then the reset draws): state (B rows of state_bytes), frames (B rows of HW = (G*unit)^2
 * floats: 0 space, 1 body, 1.5 head, 0.33 food) and, when rgb != NULL, the raw frames (B rows of HW*3 bytes, (H, W, 3)).  */
int a2c_snake_reset(int32_t *state, int B, int env_id0, uint32_t seed, int G, int unit, int n_foods, float *frames,
                    uint8_t *rgb, a2c_stream_t stream);
/* one step of B worlds: env e takes (actions[e * act_stride] + action_shift) & 3 (0 up, 1 right, 2 down, 3 left), rew /
 * done / reset (B floats each; reset == done: a finished world has already been restarted and `frames` holds its reset
 * frame, what utils.next_state(reset=True) expects).  ep_stats (may be NULL): two int32 the kernel adds to with atomics --
 * episodes finished, sum of their rewards.                                                                             */
int a2c_snake_step(int32_t *state, const int64_t *actions, int64_t act_stride, int action_shift, int B, int env_id0,
                   uint32_t seed, int G, int unit, int n_foods, float *rew, float *done, float *reset, float *frames,
                   uint8_t *rgb, int32_t *ep_stats, a2c_stream_t stream);

/* ------------------------------------------------------------------ Pong worlds in device memory (csrc/pong.hip)
 * The reference's main env (preprocessing.py:11-17 pong_prep, the "Pong" done override of runner.py:212-214) with this
 * project's own integer rules (the host twin a2c_amd/pong.py produces the same integers; parity with
 * ALE is not claimed).  Field 80 x 80; opponent paddle in columns 8..9, agent paddle in columns 70..71 (2 x 8 each), a
 * 2 x 2 ball; a prepped frame is 6400 floats, 1 on the three rectangles, 0 elsewhere.  World parameters and their bounds
 * (anything else returns A2C_ERR_ARG without a launch): 1 <= points_to_win <= 21, 1 <= max_episode_steps <= 2^24,
 * 1 <= opp_skill_den <= 2^16, 0 <= opp_skill_num <= opp_skill_den (the opponent moves on the steps whose draw mod den is
 * below num).  Also A2C_ERR_ARG: B <= 0, env_id0 < 0, act_stride < 0, a NULL state / actions / frames / rew / done / reset,
 * frames not 16-byte aligned, frame_ld < 6400 or not a multiple of 4.  Env e of a launch is world env_id0 + e of `seed`:
 * draw i of a world is hash32(seed, env_id, i).  The state of one env is 16 int32 words: agent paddle y, opponent paddle
 * y, ball x, ball y, vx, vy, agent score, opponent score, draw counter, step counter, episode-step counter, reward since
 * the last done, the action of the previous game frame (sticky actions, a2c_pong_step_skip; 0 without them), 3 spare.  The
 * kernels advance the counters in device memory: a captured launch plays new steps at each replay.
 * a2c_pong_state_bytes: bytes of ONE env's state, 0 for an unsupported points_to_win.                                  */
size_t a2c_pong_state_bytes(int points_to_win);
/* starts B worlds (counters to 0, scores to 0, paddles centred, then the serve draw): state (B rows of 16 words) and
 * frames (B rows of 6400 floats, frame_ld floats apart).                                                               */
int a2c_pong_reset(int32_t *state, int B, int env_id0, uint32_t seed, int points_to_win, int max_episode_steps,
                   int opp_skill_num, int opp_skill_den, float *frames, int64_t frame_ld, a2c_stream_t stream);
/* one step of B worlds: env e takes (actions[e * act_stride] + action_shift) mod 3 (0 stay, 1 up, 2 down).  rew: +1 the
 * opponent missed, -1 the agent missed, else 0.  reset: 1 when the episode ended (a score reached points_to_win, or
 * max_episode_steps steps): the world has already been restarted and `frames` holds its reset frame, what
 * utils.next_state(reset=True) expects.  done = (rew != 0) or reset, the done of a "Pong" env type.  ep_count /
 * ep_rew_sum (each may be NULL): one int32 each, added to with atomics -- the dones, and the rewards they closed.       */
int a2c_pong_step(int32_t *state, const int64_t *actions, int64_t act_stride, int action_shift, int B, int env_id0,
                  uint32_t seed, int points_to_win, int max_episode_steps, int opp_skill_num, int opp_skill_den,
                  float *frames, int64_t frame_ld, float *rew, float *done, float *reset, int32_t *ep_count,
                  int32_t *ep_rew_sum, a2c_stream_t stream);
/* a2c_pong_step with frame skip and sticky actions: one AGENT step is frame_skip game frames, each
 * the step above.  With a = (action + action_shift) mod 3, game frame s = 0 .. frame_skip-1 runs x = a; when
 * sticky_num > 0 one draw d is taken first (before the frame's opponent draw) and x = the action of the previous game
 * frame (state word 12) if d mod sticky_den < sticky_num; word 12 = x; with sticky_num == 0 no draw is taken and word 12
 * stays 0.  An episode end restarts the world, zeroes word 12 and DROPS the remaining frames.  rew = the sum over the
 * frames run (|rew| <= 1: after a serve the ball needs at least 33 frames to reach a goal line), reset = the episode
 * ended, done = reset or rew != 0, `frames` = the world as the last frame run left it (after an end: the reset frame).  The
 * step and episode-step words, and max_episode_steps, count GAME frames; ep_count / ep_rew_sum count agent-step dones.
 * (1, 0, 1) is a2c_pong_step itself.  A2C_ERR_ARG without a launch, besides what a2c_pong_step rejects: frame_skip outside
 * 1..8, sticky_den outside 1..2^16, sticky_num outside 0..sticky_den.                                                    */
int a2c_pong_step_skip(int32_t *state, const int64_t *actions, int64_t act_stride, int action_shift, int B, int env_id0,
                       uint32_t seed, int points_to_win, int max_episode_steps, int opp_skill_num, int opp_skill_den,
                       float *frames, int64_t frame_ld, float *rew, float *done, float *reset, int32_t *ep_count,
                       int32_t *ep_rew_sum, int frame_skip, int sticky_num, int sticky_den, a2c_stream_t stream);

/* ------------------------------------------------------------------ Breakout worlds in device memory (csrc/breakout.hip)
 * The env of the reference's Breakout runs (preprocessing.py:19-23 breakout_prep: grey frames with more than two levels,
 * real dones only) with this project's own integer rules (the host twin a2c_amd/breakout.py produces
 * the same integers; parity with ALE is not claimed).  Field 72 columns x 80 rows; 6 x 18 bricks of 4 x 3 pixels from row
 * 11 on (grey levels 200, 198, 180, 162, 72, 66 and 7, 7, 4, 4, 1, 1 points by row, top row first), an 8 x 2 paddle in rows
 * 77..78 and a 2 x 2 ball, both of level 200; a prepped frame is 5760 floats holding those levels, 0 elsewhere.  World
 * parameters and their bounds (anything else returns A2C_ERR_ARG without a launch): 1 <= lives <= 5,
 * 1 <= max_episode_steps <= 2^24.  Also A2C_ERR_ARG: B <= 0, env_id0 < 0, act_stride < 0, a NULL state / actions / frames /
 * rew / done / reset, frames not 16-byte aligned, frame_ld < 5760 or not a multiple of 4.  Env e of a launch is world
 * env_id0 + e of `seed`: draw i of a world is hash32(seed, env_id, i); the only draws are serves.  The state of one env is
 * 24 int32 words: paddle x, ball x, ball y, vx, vy, lives left, bricks left, draw counter, step counter, episode-step
 * counter, reward since the last done, the six brick rows' masks (bit c = brick column c alive, top row first), the action
 * of the previous game frame (sticky actions, a2c_breakout_step_skip; 0 without them), 6 spare.
 * The kernels advance the counters in device memory: a captured launch plays new steps at each replay.
 * a2c_breakout_state_bytes: bytes of ONE env's state, 0 for an unsupported lives.                                        */
size_t a2c_breakout_state_bytes(int lives);
/* starts B worlds (counters to 0, all 108 bricks, `lives` lives, the paddle at x = 32, then the serve draw): state (B rows
 * of 24 words) and frames (B rows of 5760 floats, frame_ld floats apart).                                                */
int a2c_breakout_reset(int32_t *state, int B, int env_id0, uint32_t seed, int lives, int max_episode_steps, float *frames,
                       int64_t frame_ld, a2c_stream_t stream);
/* one step of B worlds: env e takes (actions[e * act_stride] + action_shift) mod 4 (0 nothing, 1 = ALE's FIRE: nothing,
 * 2 right, 3 left).  rew: the points of the brick the ball removed, else 0.  done == reset: 1 when the episode ended (no
 * life left, no brick left, or max_episode_steps steps): the world has already been restarted and `frames` holds its reset
 * frame, what utils.next_state(reset=True) expects.  ep_count / ep_rew_sum (each may be NULL): one int32 each, added to
 * with atomics -- the episodes finished, and the sum of their rewards.                                                   */
int a2c_breakout_step(int32_t *state, const int64_t *actions, int64_t act_stride, int action_shift, int B, int env_id0,
                      uint32_t seed, int lives, int max_episode_steps, float *frames, int64_t frame_ld, float *rew,
                      float *done, float *reset, int32_t *ep_count, int32_t *ep_rew_sum, a2c_stream_t stream);
/* a2c_breakout_step with frame skip and sticky actions, by the rules of a2c_pong_step_skip (the previous action is state
 * word 17; the sticky draw comes before the frame): rew = the sum of the bricks' points over the frames run (several
 * bricks may fall in one agent step), done == reset = the episode ended, which drops the remaining frames.  (1, 0, 1) is
 * a2c_breakout_step itself.  A2C_ERR_ARG as there.                                                                        */
int a2c_breakout_step_skip(int32_t *state, const int64_t *actions, int64_t act_stride, int action_shift, int B, int env_id0,
                           uint32_t seed, int lives, int max_episode_steps, float *frames, int64_t frame_ld, float *rew,
                           float *done, float *reset, int32_t *ep_count, int32_t *ep_rew_sum, int frame_skip, int sticky_num,
                           int sticky_den, a2c_stream_t stream);

/* ------------------------------------------------------------------ world step + bookkeeping + frame stack in ONE launch
 * a2c_<world>_step_post(<the arguments of a2c_<world>_step>, post, stream) equals, on the same stream and in this order,
 *   1. a2c_<world>_step;
 *   2. the bookkeeping of env step `t` of slots slot0 .. slot0+B-1 (runner.py:212-232): e = (slot0 + b) * T + t,
 *      rewards[e] = rew[b], dones[e] = done[b] (1 as well when `pong` and rew[b] != 0), done_eff_out[b] = dones[e] (may be
 *      NULL), deltas[e-1] = rewards[e-1] + gamma * val[b * val_stride] * (1 - dones[e-1]) - val_prev[b] when t > 0 (left to
 *      right, every operation rounded: what a2c_rollout_record and a2c_rollout_post both compute), val_prev[b] = val[..];
 *   3. when h != NULL: rows b of h (hdim floats each) with dones[e] != 0 are zeroed, as a2c_rollout_record does;
 *   4. a2c_frame_stack_push: out[b] = reset[b] ? [0, .., 0, frame] : [prev[b][1:], frame] over C planes of the world's HW
 *      floats, rows prev_stride / out_stride floats apart --
 * with every output bit-identical to that sequence.  `frames` may be NULL here: the new frame is then rendered into plane
 * C - 1 of `out` only (rew / done / reset are still written).  One workgroup of 4 wavefronts per env: every wave recomputes
 * the (wave-uniform, deterministic) step, wave 0 alone stores the state words, rew / done / reset, the bookkeeping row and
 * the episode counters, and the C - 1 planes and the rendered frame are split over the 256 lanes as 16-byte loads / stores.
 * A2C_ERR_ARG without a launch: everything a2c_<world>_step rejects (a NULL `frames` excepted), a NULL post / val /
 * val_prev / rewards / dones / deltas / prev / out, T < 1, t outside 0 .. T-1, C < 1, prev_stride or out_stride not a
 * multiple of 4 or below C * HW, out or prev not 16-byte aligned, out == prev, h != NULL with hdim < 1.                   */
typedef struct {
  const float *val;            /* value of the state the action was sampled from: val[b * val_stride]               */
  int64_t val_stride;
  float *val_prev;             /* B floats: the value of the previous step's state, replaced by val                 */
  float *rewards, *dones, *deltas;   /* the rollout buffer's rows, indexed (slot0 + b) * T + t                      */
  int64_t T, t, slot0;
  float gamma;
  int pong;                    /* the "Pong" done override: a non-zero reward closes the step                       */
  const float *prev;           /* state the step was taken from: B rows of C * HW floats, prev_stride floats apart  */
  int64_t prev_stride;
  float *out;                  /* the next state, out_stride floats apart                                           */
  int64_t out_stride;
  int C;                       /* planes of a state (n_frame_stack)                                                 */
  float *done_eff_out;         /* B floats or NULL                                                                  */
  float *h;                    /* recurrent nets: B rows of hdim floats, or NULL                                    */
  int hdim;
} a2c_world_post;

int a2c_snake_step_post(int32_t *state, const int64_t *actions, int64_t act_stride, int action_shift, int B, int env_id0,
                        uint32_t seed, int G, int unit, int n_foods, float *rew, float *done, float *reset, float *frames,
                        uint8_t *rgb, int32_t *ep_stats, const a2c_world_post *post, a2c_stream_t stream);
int a2c_pong_step_post(int32_t *state, const int64_t *actions, int64_t act_stride, int action_shift, int B, int env_id0,
                       uint32_t seed, int points_to_win, int max_episode_steps, int opp_skill_num, int opp_skill_den,
                       float *frames, int64_t frame_ld, float *rew, float *done, float *reset, int32_t *ep_count,
                       int32_t *ep_rew_sum, const a2c_world_post *post, a2c_stream_t stream);
int a2c_breakout_step_post(int32_t *state, const int64_t *actions, int64_t act_stride, int action_shift, int B, int env_id0,
                           uint32_t seed, int lives, int max_episode_steps, float *frames, int64_t frame_ld, float *rew,
                           float *done, float *reset, int32_t *ep_count, int32_t *ep_rew_sum, const a2c_world_post *post,
                           a2c_stream_t stream);
/* the same around a2c_<world>_step_skip: every wave recomputes the whole agent step, so the break at an episode end is
 * uniform over the workgroup; the planes are copied and the frame is rendered once per agent step.                        */
int a2c_pong_step_post_skip(int32_t *state, const int64_t *actions, int64_t act_stride, int action_shift, int B, int env_id0,
                            uint32_t seed, int points_to_win, int max_episode_steps, int opp_skill_num, int opp_skill_den,
                            float *frames, int64_t frame_ld, float *rew, float *done, float *reset, int32_t *ep_count,
                            int32_t *ep_rew_sum, int frame_skip, int sticky_num, int sticky_den, const a2c_world_post *post,
                            a2c_stream_t stream);
int a2c_breakout_step_post_skip(int32_t *state, const int64_t *actions, int64_t act_stride, int action_shift, int B,
                                int env_id0, uint32_t seed, int lives, int max_episode_steps, float *frames, int64_t frame_ld,
                                float *rew, float *done, float *reset, int32_t *ep_count, int32_t *ep_rew_sum, int frame_skip,
                                int sticky_num, int sticky_den, const a2c_world_post *post, a2c_stream_t stream);

/* ------------------------------------------------------------------ random frame skip, episodic life, reward clipping
 * The rest of what Pong-v0 and the usual wrappers do around ALE, as one block and one entry point
 * per world: a2c_<world>_step_rules(<the arguments of a2c_<world>_step>, rules, post, stream).  post == NULL is the step
 * of a2c_<world>_step_skip (frames must be given), else that of a2c_<world>_step_post_skip; with frame_skip_max ==
 * frame_skip and both flags 0 the call IS that entry point: same checks, same kernel.  Otherwise
 *   1. frame_skip_max > frame_skip: the agent step first takes ONE draw d (before its first sticky draw) and plays
 *      k = frame_skip + d mod (frame_skip_max - frame_skip + 1) game frames.  k is not kept anywhere.
 *   2. episodic_life (Breakout): a game frame that loses a life without ending the episode closes the agent step as an
 *      episode end does -- word 17 = 0, the remaining frames dropped, done = reset = 1 (with post: the C - 1 older planes
 *      and the hidden row are zeroed) -- but the world is NOT restarted: bricks, lives, the episode-step word and its
 *      limit carry on, and `frames` shows the ball as just served.  ep_count / ep_rew_sum count these closes too, with the
 *      reward since the previous close (word 10 is zeroed by every close).
 *   3. clip_rewards (Breakout): rew (and, with post, rewards[]) is the sign of the agent step's summed reward; word 10
 *      and ep_rew_sum keep booking the sum itself.
 * A2C_ERR_ARG without a launch, besides what a2c_<world>_step_skip / _step_post_skip reject: a NULL rules,
 * frame_skip_max outside frame_skip .. 8, a flag that is neither 0 nor 1, either flag set for Pong (a point closes every
 * step there already, and |rew| <= 1).                                                                                   */
typedef struct {
  int32_t frame_skip, frame_skip_max;   /* game frames per agent step: frame_skip .. frame_skip_max, drawn per step    */
  int32_t sticky_num, sticky_den;
  int32_t episodic_life, clip_rewards;  /* 0 or 1; Breakout only                                                       */
} a2c_world_rules;

int a2c_pong_step_rules(int32_t *state, const int64_t *actions, int64_t act_stride, int action_shift, int B, int env_id0,
                        uint32_t seed, int points_to_win, int max_episode_steps, int opp_skill_num, int opp_skill_den,
                        float *frames, int64_t frame_ld, float *rew, float *done, float *reset, int32_t *ep_count,
                        int32_t *ep_rew_sum, const a2c_world_rules *rules, const a2c_world_post *post, a2c_stream_t stream);
int a2c_breakout_step_rules(int32_t *state, const int64_t *actions, int64_t act_stride, int action_shift, int B, int env_id0,
                            uint32_t seed, int lives, int max_episode_steps, float *frames, int64_t frame_ld, float *rew,
                            float *done, float *reset, int32_t *ep_count, int32_t *ep_rew_sum, const a2c_world_rules *rules,
                            const a2c_world_post *post, a2c_stream_t stream);

/* ------------------------------------------------------------------ Point worlds in device memory (csrc/point.hip)
 * The continuous-control world of the Gaussian nets (FCModel / GRUFCModel with is_discrete = False): a point mass chasing
 * targets on a 4096 x 4096 integer field, this project's own integer rules (the host twin
 * a2c_amd/point.py produces the same integers).  The state of one env is 16 int32 words: px, py, vx, vy, tx, ty, targets
 * reached, spare, then draw counter, game-frame counter, episode-frame counter, reward since the last done, the packed
 * action of the previous game frame (sticky actions; 0 without them), 3 spare.  An action is TWO floats; each becomes
 * q = 0 for a NaN x, else rint(clamp(x, -1, 1) * 64) (ties to even), x = fp32(a + action_shift): -64 .. 64.  One game frame:
 * d0 = (|px - tx| + |py - ty|) / 64; per axis v = clamp(v + floor(q / 8), -64, 64), p += v, a wall (p < 0, p > 4095) stops
 * the point there with v = 0; d1 likewise; rew = d0 - d1, + 10 and one more target reached when d1 == 0; the episode ends at
 * targets_to_win targets or max_episode_steps frames (the world restarts: two draws place point and target), else a reached
 * target is replaced with one draw.  place(d) = (512 + (d & 0xFFF) % 3072, 512 + ((d >> 12) & 0xFFF) % 3072); draw i of
 * world env_id0 + e is hash32(seed, env_id, i).  done == reset: real dones only.  An observation is 8 floats, each an
 * integer times a power of two: (2 px - 4095) / 4096, (2 py - 4095) / 4096, vx / 64, vy / 64, (tx - px) / 4096,
 * (ty - py) / 4096, got / 8, 1.  World parameters: 1 <= targets_to_win <= 8, 1 <= max_episode_steps <= 2^24.
 * One lane plays one env, 64 envs per wavefront.
 * a2c_point_state_bytes: bytes of ONE env's state.                                                                       */
size_t a2c_point_state_bytes(void);
/* starts B worlds (counters to 0, then the two draws): state (B rows of 16 words) and obs (B rows of 8 floats, obs_ld
 * floats apart).  A2C_ERR_ARG without a launch: B <= 0, env_id0 < 0, a world parameter out of bounds, a NULL state / obs,
 * state or obs not 16-byte aligned, obs_ld < 8 or not a multiple of 4.                                                    */
int a2c_point_reset(int32_t *state, int B, int env_id0, uint32_t seed, int targets_to_win, int max_episode_steps,
                    float *obs, int64_t obs_ld, a2c_stream_t stream);
/* one AGENT step of B worlds by the a2c_world_rules block (NULL: {1, 1, 0, 1, 0, 0}, one game frame): frame_skip ..
 * frame_skip_max game frames with the action of env e, actions[e * act_ld + 0 .. 1], and sticky actions, draws in the order
 * of a2c_<world>_step_rules (the k-draw first, then one sticky draw per frame before the frame's own); rew is the summed
 * reward, an episode end drops the remaining frames.  ep_count / ep_rew_sum as in a2c_pong_step.
 * post == NULL: the plain step; obs is required.  post != NULL: the step + the bookkeeping + the hidden-row reset + the
 * frame stack of the a2c_world_post contract above (HW = 8) in one launch, bit-identical to the plain step followed by
 * a2c_rollout_post (h == NULL) or by a2c_rollout_record + a2c_frame_stack_push (h != NULL); obs may be NULL then.
 * A2C_ERR_ARG without a launch: what a2c_point_reset rejects (a NULL obs excepted with post), act_ld < 2, a NULL actions /
 * rew / done / reset, actions not 4-byte aligned, a rules block a2c_pong_step_rules rejects (either flag set included), a
 * post block a2c_<world>_step_post rejects.                                                                               */
int a2c_point_step(int32_t *state, const float *actions, int64_t act_ld, float action_shift, int B, int env_id0,
                   uint32_t seed, int targets_to_win, int max_episode_steps, float *obs, int64_t obs_ld, float *rew,
                   float *done, float *reset, int32_t *ep_count, int32_t *ep_rew_sum, const a2c_world_rules *rules,
                   const a2c_world_post *post, a2c_stream_t stream);

/* ------------------------------------------------------------------ CartPole worlds in device memory (csrc/cartpole.hip)
 * The world of the discrete FC nets (FCModel / GRUFCModel with is_discrete = True): the pole on a cart, the textbook
 * equations with gym's constants and Euler order in this project's own integer arithmetic (the host
 * twin a2c_amd/cartpole.py produces the same integers; parity with gym is not claimed).  The state of one env is 12 int32
 * words: x, x_dot, theta, theta_dot in Q20 (unit 2^-20), then draw counter, game-frame counter, episode-frame counter,
 * reward since the last done, the action of the previous game frame (sticky actions; 0 without them), 3 spare.  An action
 * is (actions[e * act_stride] + action_shift) mod 2: 0 pushes left, 1 pushes right.  One game frame: sin / cos of theta as
 * polynomials, the two accelerations (every product floored by >> 20, one floor division), x += tau x_dot,
 * x_dot += tau xacc, theta += tau theta_dot, theta_dot += tau thetaacc from the values before the frame, both velocities
 * clamped to +-8; rew = 1; the episode ends when |x| > 2.4, |theta| > 12 degrees or after max_episode_steps frames (the
 * world restarts: four draws d give x, x_dot, theta, theta_dot = d mod 104857 - 52428).  Draw i of world env_id0 + e is
 * hash32(seed, env_id, i).  done == reset: real dones only.  An observation is the 4 state ints times 2^-20, exact in
 * fp32.  World parameter: 1 <= max_episode_steps <= 2^24.  One lane plays one env, 64 envs per wavefront.
 * a2c_cartpole_state_bytes: bytes of ONE env's state.                                                                    */
size_t a2c_cartpole_state_bytes(void);
/* starts B worlds (counters to 0, then the four draws): state (B rows of 12 words) and obs (B rows of 4 floats, obs_ld
 * floats apart).  A2C_ERR_ARG without a launch: B <= 0, env_id0 < 0, max_episode_steps out of bounds, a NULL state / obs,
 * state or obs not 16-byte aligned, obs_ld < 4 or not a multiple of 4.                                                    */
int a2c_cartpole_reset(int32_t *state, int B, int env_id0, uint32_t seed, int max_episode_steps, float *obs, int64_t obs_ld,
                       a2c_stream_t stream);
/* one AGENT step of B worlds by the a2c_world_rules block (NULL: {1, 1, 0, 1, 0, 0}, one game frame), as a2c_point_step:
 * frame_skip .. frame_skip_max game frames with the action of env e and sticky actions, draws in the order of
 * a2c_<world>_step_rules; rew is the summed reward (the game frames played), an episode end drops the remaining frames.
 * ep_count / ep_rew_sum as in a2c_pong_step.
 * post == NULL: the plain step; obs is required.  post != NULL: the step + the bookkeeping + the hidden-row reset + the
 * frame stack of the a2c_world_post contract above (HW = 4) in one launch, bit-identical to the plain step followed by
 * a2c_rollout_post (h == NULL) or by a2c_rollout_record + a2c_frame_stack_push (h != NULL); obs may be NULL then.
 * A2C_ERR_ARG without a launch: what a2c_cartpole_reset rejects (a NULL obs excepted with post), act_stride < 0, a NULL
 * actions / rew / done / reset, a rules block a2c_pong_step_rules rejects (either flag set included), a post block
 * a2c_<world>_step_post rejects.                                                                                          */
int a2c_cartpole_step(int32_t *state, const int64_t *actions, int64_t act_stride, int action_shift, int B, int env_id0,
                      uint32_t seed, int max_episode_steps, float *obs, int64_t obs_ld, float *rew, float *done,
                      float *reset, int32_t *ep_count, int32_t *ep_rew_sum, const a2c_world_rules *rules,
                      const a2c_world_post *post, a2c_stream_t stream);

/* ------------------------------------------------------------------ Pendulum worlds in device memory (csrc/pendulum.hip)
 * The textbook continuous-control world of the Gaussian nets (FCModel / GRUFCModel with is_discrete = False): the pendulum
 * swing-up, the textbook equations with gym's constants and Euler order in this project's own integer arithmetic (DESIGN.md
 * section 6l; the host twin a2c_amd/pendulum.py produces the same integers; parity with gym is not claimed).  The state of
 * one env is 12 int32 words: theta in [-pi, pi) and theta_dot in [-8, 8] in Q20 (unit 2^-20), 2 spare, then draw counter,
 * game-frame counter, episode-frame counter, reward since the last done IN UNITS OF 2^-8, the quantised action of the previous
 * game frame (sticky actions; 0 without them), 3 spare.  The action of env e is ONE float, actions[e * act_ld]:
 * x = fp32(a + action_shift), q = 0 for a NaN, else rint(clamp(x, -2, 2) * 32) with ties to even, the torque u = q / 32.
 * One game frame: cost = theta^2 + 0.1 theta_dot^2 + 0.001 u^2 from the values before the frame;
 * theta_dot = clamp(theta_dot + 0.75 sin theta + 0.15 u, +-8); theta += 0.05 theta_dot (the new one), wrapped once into
 * [-pi, pi); every product floored by >> 20, sin / cos nested-ratio polynomials, no division.  The frame's reward is the
 * int -(cost >> 12) in units of 2^-8 (-4166 .. 0); rew[] and the post bookkeeping get the summed ints times 2^-8 as fp32,
 * exact.  The episode ends after max_episode_steps frames and in no other way (the world restarts: two draws d give
 * theta = d mod 2 pi - pi and theta_dot = d mod (2^21 + 1) - 2^20).  Draw i of world env_id0 + e is
 * hash32(seed, env_id, i).  done == reset: real dones only.  An observation is (cos theta, sin theta, theta_dot) times
 * 2^-20 and a 0, exact in fp32.  World parameter: 1 <= max_episode_steps <= 2^16.  One lane plays one env, 64 envs per
 * wavefront.
 * a2c_pendulum_state_bytes: bytes of ONE env's state.                                                                    */
size_t a2c_pendulum_state_bytes(void);
/* starts B worlds (counters to 0, then the two draws): state (B rows of 12 words) and obs (B rows of 4 floats, obs_ld
 * floats apart).  A2C_ERR_ARG without a launch: B <= 0, env_id0 < 0, max_episode_steps out of bounds, a NULL state / obs,
 * state or obs not 16-byte aligned, obs_ld < 4 or not a multiple of 4.                                                    */
int a2c_pendulum_reset(int32_t *state, int B, int env_id0, uint32_t seed, int max_episode_steps, float *obs, int64_t obs_ld,
                       a2c_stream_t stream);
/* one AGENT step of B worlds by the a2c_world_rules block (NULL: {1, 1, 0, 1, 0, 0}, one game frame), as a2c_point_step:
 * frame_skip .. frame_skip_max game frames with the action of env e and sticky actions, draws in the order of
 * a2c_<world>_step_rules; rew is the summed reward, an episode end drops the remaining frames.  ep_count counts the closed
 * steps; ep_rew_sum gets, per closed step, the reward since the last done FLOORED TO WHOLE reward units (the int >> 8), so
 * the sum of a pool whose envs all close in one step stays inside an int32: less than one unit per episode below the exact sum.
 * post == NULL: the plain step; obs is required.  post != NULL: the step + the bookkeeping + the hidden-row reset + the
 * frame stack of the a2c_world_post contract above (HW = 4) in one launch, bit-identical to the plain step followed by
 * a2c_rollout_post (h == NULL) or by a2c_rollout_record + a2c_frame_stack_push (h != NULL); obs may be NULL then.
 * A2C_ERR_ARG without a launch: what a2c_pendulum_reset rejects (a NULL obs excepted with post), act_ld < 1, a NULL
 * actions / rew / done / reset, actions not 4-byte aligned, a rules block a2c_pong_step_rules rejects (either flag set
 * included), a post block a2c_<world>_step_post rejects.                                                                  */
int a2c_pendulum_step(int32_t *state, const float *actions, int64_t act_ld, float action_shift, int B, int env_id0,
                      uint32_t seed, int max_episode_steps, float *obs, int64_t obs_ld, float *rew, float *done,
                      float *reset, int32_t *ep_count, int32_t *ep_rew_sum, const a2c_world_rules *rules,
                      const a2c_world_post *post, a2c_stream_t stream);

/* ------------------------------------------------------------------ time-limit truncation on the lane worlds
 * An episode that ends because ep_steps reached max_episode_steps, and for no reason of the game's own, was cut short, not
 * lost: its targets bootstrap from the value of the state it ended in (hyps["bootstrap_truncated"]).  That state is gone
 * when the launch returns (the world restarts inside it), so the step reports it:
 * a2c_<world>_step_trunc(<the arguments of a2c_<world>_step, rules and post included>, tr, stream) is a2c_<world>_step --
 * every output of that entry point bit-identical: state words, obs, rew, done, reset, the counters, the post block's
 * bookkeeping, hidden rows and frame stack -- and for env b
 *   trunc[b * trunc_stride] = 1 when the agent step ended an episode at a game frame where ep_steps >= max_episode_steps held
 *     and the game's own end condition did not (CartPole: x or theta out of range; Point: targets_to_win reached; Pendulum
 *     has none), else 0.  Both at the same frame is a terminal end: 0.  With frame skip and sticky actions the frame that
 *     ends the episode decides.
 *   final_obs[b * final_ld + 0 .. HW-1] = the observation of the world as it stood after that frame's physics and before the
 *     restart; where the step ended no episode, the step's own observation.  Every row is written at every launch.
 * A2C_ERR_ARG without a launch: what a2c_<world>_step rejects, a NULL tr / trunc / final_obs, trunc_stride < 1, final_obs
 * not 16-byte aligned, final_ld < HW or not a multiple of 4.                                                               */
typedef struct {
  float *trunc;                /* B floats, trunc_stride floats apart (a row of the rollout buffer: stride T)        */
  int64_t trunc_stride;
  float *final_obs;            /* B rows of HW floats, final_ld floats apart                                          */
  int64_t final_ld;
} a2c_world_trunc;

int a2c_point_step_trunc(int32_t *state, const float *actions, int64_t act_ld, float action_shift, int B, int env_id0,
                         uint32_t seed, int targets_to_win, int max_episode_steps, float *obs, int64_t obs_ld, float *rew,
                         float *done, float *reset, int32_t *ep_count, int32_t *ep_rew_sum, const a2c_world_rules *rules,
                         const a2c_world_post *post, const a2c_world_trunc *tr, a2c_stream_t stream);
int a2c_cartpole_step_trunc(int32_t *state, const int64_t *actions, int64_t act_stride, int action_shift, int B, int env_id0,
                            uint32_t seed, int max_episode_steps, float *obs, int64_t obs_ld, float *rew, float *done,
                            float *reset, int32_t *ep_count, int32_t *ep_rew_sum, const a2c_world_rules *rules,
                            const a2c_world_post *post, const a2c_world_trunc *tr, a2c_stream_t stream);
int a2c_pendulum_step_trunc(int32_t *state, const float *actions, int64_t act_ld, float action_shift, int B, int env_id0,
                            uint32_t seed, int max_episode_steps, float *obs, int64_t obs_ld, float *rew, float *done,
                            float *reset, int32_t *ep_count, int32_t *ep_rew_sum, const a2c_world_rules *rules,
                            const a2c_world_post *post, const a2c_world_trunc *tr, a2c_stream_t stream);
/* the state the net would have seen next had the episode not restarted, for every row of a rollout buffer:
 * out[e] = [planes 1 .. C-1 of states[e], final_obs[e]], rows of C * HW (states, out) and HW (final_obs) floats, dense, as
 * 16-byte accesses.  N == 0 is a no-op.  A2C_ERR_ARG without a launch: N < 0, C < 1, HW < 4 or not a multiple of 4, a NULL
 * or not 16-byte aligned pointer, out == states.                                                                          */
int a2c_final_states(const float *states, const float *final_obs, int C, int HW, int64_t N, float *out, a2c_stream_t stream);
/* the correction of a truncated step's targets, for both arrays x = rewards, deltas:
 *   t = gamma * truncs[e];  x_out[e] = (t != 0) ? x[e] + t * vfin[e] : x[e]
 * in fp32, the product gamma * truncs first, then t * vfin, then the sum, every operation rounded (no FMA): the NumPy
 * statement np.where(t != 0, x + t * vfin, x) over float32 arrays with t = np.float32(gamma) * truncs gives the same bits.
 * A row that was not truncated passes through untouched, whatever vfin[e] holds.  The scans cut at done, so adding
 * gamma * V(final state) to the reward and to the delta of the closing step corrects the discounted return and the GAE
 * advantage alike.  x_out may be x.  N == 0 is a no-op.  A2C_ERR_ARG without a launch: N < 0 or a NULL pointer.            */
int a2c_trunc_bootstrap(const float *rewards, const float *deltas, const float *truncs, const float *vfin, float gamma,
                        int64_t N, float *rewards_out, float *deltas_out, a2c_stream_t stream);

/* ------------------------------------------------------------------ running observation / reward normalisation (csrc/vecnorm.hip)
 * What baselines' VecNormalize does between a vector world and the agent (host twin
 * a2c_amd/vecnorm.py): running mean and variance of the observations and of the discounted return, observations centred and
 * scaled, rewards divided by the return's standard deviation, both clipped.  The statistics live in device memory and advance
 * at every launch, so a captured launch normalises new steps at each replay, as the worlds' counters do.
 * The state block is 4 + 2 L + B_pool doubles: obs count, obs mean[L], obs var[L], return count, return mean, return var,
 * ret[B_pool] (the per-env discounted return accumulators).
 * a2c_vecnorm_state_bytes: bytes of the block, 0 for L outside 1..64 or B_pool < 1.
 * a2c_vecnorm_init: counts = 1e-4, means = 0, vars = 1, ret = 0 (what baselines' RunningMeanStd starts from).  A2C_ERR_ARG
 * without a launch: a NULL block, L outside 1..64, B_pool < 1.
 * a2c_vecnorm_step: one env step of the B envs env0 .. env0+B-1 of a launch, in this order:
 *   1. observations (out != NULL): x[b][j] = out[b * out_stride + (C-1) * L + j], the NEW plane of env b's next state.  With
 *      update != 0 the batch is folded into the running moments, per feature: bm = sum x / B, bv = sum (x - bm)^2 / B (two
 *      passes), delta = bm - mean, tot = count + B, mean += delta * B / tot,
 *      var = (var * count + bv * B + delta * delta * count * B / tot) / tot, count = tot (every product and quotient left to
 *      right).  Then x = fp32(clamp((x - mean) / sqrt(var + eps), -clip_obs, clip_obs)) in place, by the UPDATED moments.  The
 *      older planes are not touched: normalise first, then stack.
 *   2. rewards (rewards != NULL): e = (slot0 + b) * T + t, r = rewards[e]; ret[env0 + b] = ret[env0 + b] * gamma + r, the B
 *      values of ret folded into the return moments by the same rule; rewards[e] = fp32(clamp(r / sqrt(ret_var + eps),
 *      -clip_rew, clip_rew)); then ret[env0 + b] = 0 where dones[e] != 0.
 *   3. update == 0 (evaluation): observations by the moments as they stand, nothing in the block is written; the reward
 *      part must be absent.
 * All arithmetic is fp64 (never contracted), one rounding to fp32 at the store.  ONE workgroup of 256 lanes: lane i sums
 * envs i, i + 256, ... in order, then a halving tree over the lanes (strides 128 .. 1); the same tree for both passes and every
 * feature.  No atomics; the result does not depend on scheduling.
 * A2C_ERR_ARG without a launch: a NULL block or args, B < 1, L outside 1..64, env0 < 0, env0 + B > B_pool, eps <= 0, a clip
 * <= 0, both parts absent; with out: C < 1, out_stride < C * L; with rewards: a NULL dones, T < 1, t outside 0 .. T-1,
 * slot0 < 0, update == 0.                                                                                                */
typedef struct {
  int32_t B, env0, B_pool;     /* the launch's envs inside the pool the block was made for                          */
  int32_t L, C;                /* floats of a plane, planes of a state                                               */
  int32_t update;              /* 0: frozen (evaluation)                                                             */
  float *out;                  /* next-state rows, out_stride floats apart, or NULL: no observation part             */
  int64_t out_stride;
  float *rewards;              /* the rollout buffer's rows, indexed (slot0 + b) * T + t, or NULL: no reward part    */
  const float *dones;
  int64_t T, t, slot0;
  double gamma, eps, clip_obs, clip_rew;
} a2c_vecnorm_args;

size_t a2c_vecnorm_state_bytes(int L, int B_pool);
int a2c_vecnorm_init(double *block, int L, int B_pool, a2c_stream_t stream);
int a2c_vecnorm_step(double *block, const a2c_vecnorm_args *args, a2c_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* A2C_MI355X_H */
