/* Stand-alone stress of the float action granules of the host pool (include/a2c_hostpool.h), meant to be built together
 * with pytorch-a2c_amd/csrc/hostpool.c under -fsanitize=address,undefined and under -fsanitize=thread:
 * one PRODUCER thread plays the GPU process (a2c_pool_post_actions_f32, then waits for the rec granules), one WORKER
 * thread plays an env worker (a2c_pool_take_f32, then a2c_pool_publish).  Every received vector is compared bit for bit
 * with what was posted for that env and step; the reward carries a checksum of it back.  The step counter starts
 * below 2^32 and wraps during the run.  Exit status 0 = every vector arrived intact. */
#include "../../include/a2c_hostpool.h"

#include <pthread.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

enum { N_ENVS = 4, ACT_DIM = 6, ROW = 9 /* a non-dense row stride */, STEPS = 4000, FRAME_BYTES = 16 };
static const uint32_t SEQ0 = 0xfffff800u;
static void *region;
static int failed;

static uint32_t mix(uint32_t seq, uint32_t env, uint32_t k) {
  uint32_t x = seq * 0x9e3779b1u ^ (env + 1u) * 0x85ebca6bu ^ (k + 1u) * 0xc2b2ae35u;
  x ^= x >> 15; x *= 0x2c1b3c6du; x ^= x >> 12; x *= 0x297a2d39u; x ^= x >> 15;
  return x;                      /* any bit pattern: NaNs, infinities and subnormals included */
}
static float checksum(uint32_t seq, uint32_t env) {
  uint32_t s = 0;
  for (uint32_t k = 0; k < ACT_DIM; ++k) s += mix(seq, env, k) >> 8;
  return (float)(s & 0xffffu);
}

static void *worker(void *arg) {
  (void)arg;
  uint32_t next_seq[N_ENVS];
  float frame[FRAME_BYTES / 4] = {0};
  for (int j = 0; j < N_ENVS; ++j) {
    next_seq[j] = SEQ0;
    a2c_pool_publish(region, j, frame, SEQ0, 0.f, 1);
  }
  a2c_pool_worker_ready(region);
  for (;;) {
    float a[ACT_DIM];
    const int i = a2c_pool_take_f32(region, 0, N_ENVS, next_seq, 50000000LL, a);
    if (i == -2) break;
    if (i < 0) continue;
    for (uint32_t k = 0; k < ACT_DIM; ++k) {
      uint32_t got;
      memcpy(&got, a + k, 4);
      if (got != mix(next_seq[i], (uint32_t)i, k)) {
        fprintf(stderr, "env %d step %u component %u: got %08x\n", i, next_seq[i], k, got);
        __atomic_store_n(&failed, 1, __ATOMIC_RELAXED);
      }
    }
    frame[0] = (float)i;
    const float rew = checksum(next_seq[i], (uint32_t)i);
    next_seq[i] += 1u;
    a2c_pool_publish(region, i, frame, next_seq[i], rew, 0);
  }
  return NULL;
}

static void *producer(void *arg) {
  (void)arg;
  float rows[N_ENVS * ROW], rew[N_ENVS], done[N_ENVS];
  if (a2c_pool_wait_frames(region, 0, N_ENVS, SEQ0, 20000000000LL)) {
    __atomic_store_n(&failed, 1, __ATOMIC_RELAXED);
    goto out;
  }
  for (uint32_t t = 0; t < STEPS; ++t) {
    const uint32_t seq = SEQ0 + t;
    for (uint32_t j = 0; j < N_ENVS; ++j)
      for (uint32_t k = 0; k < ROW; ++k) {
        const uint32_t b = k < ACT_DIM ? mix(seq, j, k) : 0xdeadbeefu;
        memcpy(rows + j * ROW + k, &b, 4);
      }
    a2c_pool_post_actions_f32(region, 0, N_ENVS, rows, ROW, seq);
    if (a2c_pool_wait_frames(region, 0, N_ENVS, seq + 1u, 20000000000LL)) {
      fprintf(stderr, "step %u: no answer\n", seq);
      __atomic_store_n(&failed, 1, __ATOMIC_RELAXED);
      break;
    }
    a2c_pool_unpack(region, 0, N_ENVS, rew, done);
    for (uint32_t j = 0; j < N_ENVS; ++j)
      if (rew[j] != checksum(seq, j) || done[j] != 0.f) {
        fprintf(stderr, "step %u env %u: reward %g\n", seq, j, rew[j]);
        __atomic_store_n(&failed, 1, __ATOMIC_RELAXED);
      }
  }
out:
  a2c_pool_set_phase(region, A2C_POOL_SHUTDOWN);
  return NULL;
}

int main(void) {
  const size_t bytes = a2c_pool_bytes_f32(N_ENVS, FRAME_BYTES, ACT_DIM);
  if (!bytes || bytes <= a2c_pool_bytes(N_ENVS, FRAME_BYTES)) return 2;
  region = aligned_alloc(4096, bytes);
  if (!region) return 2;
  memset(region, 0, bytes);
  if (a2c_pool_init(region, bytes, N_ENVS, FRAME_BYTES, A2C_FRAME_F32, 1, -1.0)) return 3;
  a2c_pool_set_seq_start(region, SEQ0);
  if (a2c_pool_enable_actions_f32(region, bytes, ACT_DIM)) return 3;
  if (a2c_pool_enable_actions_f32(region, bytes, ACT_DIM) != -1) return 3;      /* already enabled */
  a2c_pool_set_phase(region, A2C_POOL_ROLLOUT);
  pthread_t tw, tp;
  if (pthread_create(&tw, NULL, worker, NULL) || pthread_create(&tp, NULL, producer, NULL)) return 4;
  pthread_join(tp, NULL);
  pthread_join(tw, NULL);
  free(region);
  if (failed) return 1;
  printf("ok %d steps x %d envs x %d floats\n", STEPS, N_ENVS, ACT_DIM);
  return 0;
}
