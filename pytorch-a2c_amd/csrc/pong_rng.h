// Counter-based draws of the Pong worlds (csrc/pong.hip): draw i of env e is pong_hash(seed, e, i), the mixing function
// DESIGN.md section 6b states for the Snake worlds (host side: a2c_amd.snake.hash32).  No state besides the counter.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

__device__ __forceinline__ uint32_t pong_fin(uint32_t x) {        // lowbias32
  x ^= x >> 16; x *= 0x7FEB352Du; x ^= x >> 15; x *= 0x846CA68Bu; x ^= x >> 16;
  return x;
}
__device__ __forceinline__ uint32_t pong_hash(uint32_t seed, uint32_t env, uint32_t draw) {
  return pong_fin(pong_fin(pong_fin(seed + 0x9E3779B9u) ^ env) ^ draw);
}
