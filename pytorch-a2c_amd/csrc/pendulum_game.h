// The Pendulum game of pendulum.hip: PendulumGame, the pendulum swing-up in Q20 fixed point, as the game type G of world.h's
// agent step (world_agent_step<G>: World, Params, frame, closes), and the quantiser that turns the ONE float action of a
// Gaussian net into the int the agent step carries.  The equations are the textbook ones with gym's constants and Euler order;
// every value is an integer of ONE format, every product is followed by an arithmetic right shift (a floor), sin and cos are
// nested-ratio polynomials after a reflection to |x| <= pi / 2, and there is no division (DESIGN.md section 6l bounds every
// intermediate: none reaches 2^49; host twin: a2c_amd/pendulum.py, same integers).
// The int reward of a frame is in units of 2^-8: what leaves the kernel as a float is that int times 2^-8, exact.
// The observation is 4 floats, so the kernels are lane_world.h's: one LANE per env.
#pragma once
#include "world.h"

namespace {

constexpr int PENDULUM_WORDS = 12;  // theta, theta_dot, 2 spare, draws, steps, episode steps, reward since the last done (units
                                    // of 2^-8), the quantised action of the previous game frame (sticky actions; 0 without
                                    // them), 3 spare
constexpr int PENDULUM_HW = 4, PENDULUM_N_ACT = 1;
constexpr int PENDULUM_MAX_EPISODE_STEPS = 1 << 16;      // ep_rew stays below 2^16 * 4166 < 2^29
constexpr int PD_FRAC = 20;
constexpr int64_t PD_ONE = (int64_t)1 << PD_FRAC;
// the constants as integers of the format, rounded to nearest: pi, pi / 2, 3 g / (2 l) dt = 0.75, 3 / (m l^2) dt = 0.15, dt
// 0.05, the cost weights 0.1 and 0.001
constexpr int64_t PD_PI = 3294199, PD_TWO_PI = 2 * PD_PI, PD_HALF_PI = 1647099, PD_C075 = 786432, PD_C015 = 157286,
                  PD_DT = 52429, PD_C01 = 104858, PD_C0001 = 1049;
constexpr int64_t PD_VMAX = 8 * PD_ONE;
constexpr int PD_REW_SHIFT = 12, PD_REW_FRAC = 8;         // reward int = -(cost >> 12): units of 2^-8
constexpr int PD_Q = 32, PD_Q_SHIFT = 15;                 // torque = q / 32 = q << 15 in Q20, q = -64 .. 64

// the product of two numbers of the format, floored (>> of a negative int64 is the arithmetic shift)
__device__ __forceinline__ int64_t pd_mul(int64_t a, int64_t b) { return (a * b) >> PD_FRAC; }

__device__ __forceinline__ int64_t pd_clamp(int64_t v, int64_t lo, int64_t hi) { return v < lo ? lo : (v > hi ? hi : v); }

// one level of a nested series: 1 - x2 * r * p, r the ratio 1 / k as an integer of the format
__device__ __forceinline__ int64_t pd_level(int64_t x2, int64_t r, int64_t p) { return PD_ONE - pd_mul(pd_mul(x2, r), p); }

// sin and cos of th in [-PI, PI): reflected to |x| <= pi / 2 (x = +-PI - th outside, the cosine negated there), then
// sin x = x (1 - x2/6 (1 - x2/20 (1 - x2/42 (1 - x2/72 (1 - x2/110))))) and
// cos x = 1 - x2/2 (1 - x2/12 (1 - x2/30 (1 - x2/56 (1 - x2/90 (1 - x2/132))))): every ratio has full relative precision
__device__ __forceinline__ void pd_sincos(int64_t th, int64_t& s, int64_t& c) {
  const bool out = th > PD_HALF_PI || th < -PD_HALF_PI;
  const int64_t x = out ? (th > 0 ? PD_PI : -PD_PI) - th : th;
  const int64_t x2 = pd_mul(x, x);
  int64_t p = PD_ONE;
  p = pd_level(x2, 9533, p);        // 1 / 110
  p = pd_level(x2, 14564, p);       // 1 / 72
  p = pd_level(x2, 24966, p);       // 1 / 42
  p = pd_level(x2, 52429, p);       // 1 / 20
  p = pd_level(x2, 174763, p);      // 1 / 6
  s = pd_mul(x, p);
  p = PD_ONE;
  p = pd_level(x2, 7944, p);        // 1 / 132
  p = pd_level(x2, 11651, p);       // 1 / 90
  p = pd_level(x2, 18725, p);       // 1 / 56
  p = pd_level(x2, 34953, p);       // 1 / 30
  p = pd_level(x2, 87381, p);       // 1 / 12
  p = pd_level(x2, 524288, p);      // 1 / 2
  c = out ? -p : p;
}

// the action: x = fp32(a + shift), ONE rounded add; NaN -> 0, else rint(clamp(x, -2, 2) * 32), ties to even.  The product is
// exact (a power of two, |x| <= 2), so q is what NumPy's rint gives for the same x: -64 .. 64
__device__ __forceinline__ int pendulum_quantise(float a, float shift) {
  const float x = __fadd_rn(a, shift);
  if (x != x) return 0;
  const float cl = x < -2.f ? -2.f : (x > 2.f ? 2.f : x);
  return (int)rintf(__fmul_rn(cl, 32.f));
}

struct PendulumGame {
  static constexpr int WORDS = PENDULUM_WORDS, HW = PENDULUM_HW;
  struct World {
    int th, thd;
  };
  struct Params {
    int max_episode_steps;
  };

  static bool params_ok(const Params& p) {
    return p.max_episode_steps >= 1 && p.max_episode_steps <= PENDULUM_MAX_EPISODE_STEPS;
  }

  static __device__ __forceinline__ void new_episode(World& w, WorldCount& c, const Params&, uint32_t seed, uint32_t env) {
    w.th = (int)(world_hash(seed, env, c.draws++) % (uint32_t)PD_TWO_PI) - (int)PD_PI;
    w.thd = (int)(world_hash(seed, env, c.draws++) % (uint32_t)(2 * PD_ONE + 1)) - (int)PD_ONE;
    c.ep_steps = 0;
  }

  // One game frame of one world, in registers (no memory access).  a: the quantised torque q, -64 .. 64.  -> the reward in
  // units of 2^-8, -4166 .. 0; over: the episode ended (only the step cap ends one) and the world has been restarted; end
  // keeps the world the cap cut short (lane_world.h): every end here is by the limit alone
  template <typename E>
  static __device__ __forceinline__ int frame(World& w, WorldCount& c, int a, const Params& p, uint32_t seed, uint32_t env,
                                              bool& over, E& end) {
    ++c.steps;
    ++c.ep_steps;
    const int64_t th = w.th, thd = w.thd, u = (int64_t)a * ((int64_t)1 << PD_Q_SHIFT);
    const int64_t cost = pd_mul(th, th) + pd_mul(PD_C01, pd_mul(thd, thd)) + pd_mul(PD_C0001, pd_mul(u, u));
    int64_t s, co;
    pd_sincos(th, s, co);
    const int64_t nthd = pd_clamp(thd + pd_mul(PD_C075, s) + pd_mul(PD_C015, u), -PD_VMAX, PD_VMAX);
    int64_t nth = th + pd_mul(PD_DT, nthd);
    if (nth >= PD_PI) nth -= PD_TWO_PI;
    else if (nth < -PD_PI) nth += PD_TWO_PI;
    w.th = (int)nth;
    w.thd = (int)nthd;
    over = c.ep_steps >= p.max_episode_steps;
    if (over) {
      end.keep(w, true);
      new_episode(w, c, p, seed, env);
    }
    return -(int)(cost >> PD_REW_SHIFT);
  }

  // real dones only
  static __device__ __forceinline__ bool closes(bool over, int) { return over; }

  // the observation: (cos th, sin th, thd) times 2^-20 and a 0 -- the int is converted first (exact: |q| < 2^24), then ONE
  // exact multiply by a power of two
  static __device__ __forceinline__ float4 observe(const World& w) {
    constexpr float U = 1.f / 1048576.f;
    int64_t s, c;
    pd_sincos(w.th, s, c);
    return make_float4((float)(int)c * U, (float)(int)s * U, (float)w.thd * U, 0.f);
  }
};

}  // namespace
