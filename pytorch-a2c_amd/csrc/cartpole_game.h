// The CartPole game of cartpole.hip: CartPoleGame, the pole on a cart in Q20 fixed point, as the game type G of world.h's
// agent step (world_agent_step<G>: World, Params, frame, closes).  The equations are the textbook ones with gym's constants
// and Euler order; every value is an integer of ONE format, every product is followed by an arithmetic right shift (a
// floor), sin and cos are short polynomials, and the one division is a floor division written out (DESIGN.md section 6k
// lists every intermediate with its bound: none reaches 2^50; host twin: a2c_amd/cartpole.py, same integers).
// The observation is 4 floats, so the kernels are lane_world.h's: one LANE per env.
#pragma once
#include "world.h"

namespace {

constexpr int CARTPOLE_WORDS = 12;  // x, x_dot, theta, theta_dot, draws, steps, episode steps, reward since the last done,
                                    // the action of the previous game frame (sticky actions; 0 without them), 3 spare
constexpr int CARTPOLE_HW = 4, CARTPOLE_N_ACT = 2;
constexpr int CARTPOLE_MAX_EPISODE_STEPS = 1 << 24;
constexpr int CP_FRAC = 20;
constexpr int64_t CP_ONE = (int64_t)1 << CP_FRAC;
// the constants as integers of the format, rounded to nearest: g 9.8, force 10, pole mass * half length 0.05, 1 / 1.1,
// 0.1 / 1.1, 0.05 / 1.1, 4 / 3, tau 0.02, 1 / 2, 1 / 6, 1 / 24, 1 / 120
constexpr int64_t CP_G = 10276045, CP_FORCE = 10 * CP_ONE, CP_PML = 52429, CP_INV_TOTAL = 953251, CP_MP_TOTAL = 95325,
                  CP_PML_TOTAL = 47663, CP_FOUR_THIRDS = 1398101, CP_TAU = 20972, CP_HALF = CP_ONE / 2, CP_C6 = 174763,
                  CP_C24 = 43691, CP_C120 = 8738;
constexpr int64_t CP_VMAX = 8 * CP_ONE;
constexpr int CP_X_LIMIT = 2516582;      // floor(2.4 * 2^20)
constexpr int CP_TH_LIMIT = 219613;      // floor(12 degrees * 2^20)
constexpr uint32_t CP_RESET_L = 52428;   // floor(0.05 * 2^20)

// the product of two numbers of the format, floored (>> of a negative int64 is the arithmetic shift)
__device__ __forceinline__ int64_t cp_mul(int64_t a, int64_t b) { return (a * b) >> CP_FRAC; }

// floor(n / d) for d > 0: C's quotient truncates, so one less where a remainder is left below zero
__device__ __forceinline__ int64_t cartpole_floor_div(int64_t n, int64_t d) {
  const int64_t q = n / d;
  return (n - q * d < 0) ? q - 1 : q;
}

__device__ __forceinline__ int64_t cp_clamp(int64_t v, int64_t lo, int64_t hi) { return v < lo ? lo : (v > hi ? hi : v); }

struct CartPoleGame {
  static constexpr int WORDS = CARTPOLE_WORDS, HW = CARTPOLE_HW;
  struct World {
    int x, xd, th, thd;
  };
  struct Params {
    int max_episode_steps;
  };

  static bool params_ok(const Params& p) {
    return p.max_episode_steps >= 1 && p.max_episode_steps <= CARTPOLE_MAX_EPISODE_STEPS;
  }

  static __device__ __forceinline__ int start(uint32_t d) { return (int)(d % (2u * CP_RESET_L + 1u)) - (int)CP_RESET_L; }

  static __device__ __forceinline__ void new_episode(World& w, WorldCount& c, const Params&, uint32_t seed, uint32_t env) {
    w.x = start(world_hash(seed, env, c.draws++));
    w.xd = start(world_hash(seed, env, c.draws++));
    w.th = start(world_hash(seed, env, c.draws++));
    w.thd = start(world_hash(seed, env, c.draws++));
    c.ep_steps = 0;
  }

  // One game frame of one world, in registers (no memory access).  a: 0 pushes left, 1 pushes right.  -> the reward, 1;
  // over: the episode ended and the world has been restarted; end keeps the world that fell or ran out of frames (lane_world.h)
  template <typename E>
  static __device__ __forceinline__ int frame(World& w, WorldCount& c, int a, const Params& p, uint32_t seed, uint32_t env,
                                              bool& over, E& end) {
    ++c.steps;
    ++c.ep_steps;
    const int64_t x = w.x, xd = w.xd, th = w.th, thd = w.thd;
    const int64_t t2 = cp_mul(th, th);
    const int64_t s = th + cp_mul(th, cp_mul(t2, cp_mul(t2, CP_C120) - CP_C6));
    const int64_t co = CP_ONE + cp_mul(t2, cp_mul(t2, CP_C24) - CP_HALF);
    const int64_t temp = cp_mul((a ? CP_FORCE : -CP_FORCE) + cp_mul(CP_PML, cp_mul(cp_mul(thd, thd), s)), CP_INV_TOTAL);
    const int64_t num = cp_mul(CP_G, s) - cp_mul(co, temp);
    const int64_t den = (CP_FOUR_THIRDS - cp_mul(CP_MP_TOTAL, cp_mul(co, co))) >> 1;
    const int64_t thacc = cartpole_floor_div(num * CP_ONE, den);
    const int64_t xacc = temp - cp_mul(CP_PML_TOTAL, cp_mul(thacc, co));
    w.x = (int)(x + cp_mul(CP_TAU, xd));
    w.xd = (int)cp_clamp(xd + cp_mul(CP_TAU, xacc), -CP_VMAX, CP_VMAX);
    w.th = (int)(th + cp_mul(CP_TAU, thd));
    w.thd = (int)cp_clamp(thd + cp_mul(CP_TAU, thacc), -CP_VMAX, CP_VMAX);
    over = abs(w.x) > CP_X_LIMIT || abs(w.th) > CP_TH_LIMIT || c.ep_steps >= p.max_episode_steps;
    if (over) {
      end.keep(w, !(abs(w.x) > CP_X_LIMIT || abs(w.th) > CP_TH_LIMIT));
      new_episode(w, c, p, seed, env);
    }
    return 1;
  }

  // real dones only
  static __device__ __forceinline__ bool closes(bool over, int) { return over; }

  // the observation: the four state ints times 2^-20 -- the int is converted first (exact: |q| < 2^24), then ONE exact
  // multiply by a power of two
  static __device__ __forceinline__ float4 observe(const World& w) {
    constexpr float U = 1.f / 1048576.f;
    return make_float4((float)w.x * U, (float)w.xd * U, (float)w.th * U, (float)w.thd * U);
  }
};

}  // namespace
