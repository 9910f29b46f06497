// The Point game of point.hip: PointGame, a point mass chasing targets on a 4096 x 4096 integer field, as the game type G of
// world.h's agent step (world_agent_step<G>: World, Params, frame, closes), and the quantiser that turns the two float
// actions of a Gaussian net into the ONE int the agent step carries (host twin: a2c_amd/point.py).
// The observation is 8 floats, not a picture, so the kernels are lane_world.h's: one LANE per env.
#pragma once
#include "world.h"

namespace {

constexpr int POINT_WORDS = 16;     // px, py, vx, vy, tx, ty, got, spare, draws, steps, episode steps, reward since the last done,
                                    // the packed action of the previous game frame (sticky actions; 0 without them), 3 spare
constexpr int POINT_HW = 8, POINT_N_ACT = 2;
constexpr int POINT_P = 4096, POINT_VMAX = 64, POINT_CELL = 64, POINT_REACH_BONUS = 10;
constexpr int POINT_MAX_TARGETS = 8, POINT_MAX_EPISODE_STEPS = 1 << 24;

// one action component: x = fp32(a + shift), ONE rounded add; NaN -> 0, else rint(clamp(x, -1, 1) * 64), ties to even.  The
// product is exact (a power of two, |x| <= 1), so q is what NumPy's rint gives for the same x: -64 .. 64
__device__ __forceinline__ int point_quantise(float a, float shift) {
  const float x = __fadd_rn(a, shift);
  if (x != x) return 0;
  const float cl = x < -1.f ? -1.f : (x > 1.f ? 1.f : x);
  return (int)rintf(__fmul_rn(cl, 64.f));
}

// the pair as the agent step's int: packed 0 is (0, 0), what `prev = 0` after an episode end means
__device__ __forceinline__ int point_pack(int qx, int qy) { return (qx & 0xFF) | ((qy & 0xFF) << 8); }
__device__ __forceinline__ int point_byte(int a, int sh) { return (int)(int8_t)((a >> sh) & 0xFF); }

struct PointGame {
  static constexpr int WORDS = POINT_WORDS, HW = POINT_HW;
  struct World {
    int px, py, vx, vy, tx, ty, got;
  };
  struct Params {
    int targets_to_win, max_episode_steps;
  };

  static bool params_ok(const Params& p) {
    return p.targets_to_win >= 1 && p.targets_to_win <= POINT_MAX_TARGETS && p.max_episode_steps >= 1 &&
           p.max_episode_steps <= POINT_MAX_EPISODE_STEPS;
  }

  static __device__ __forceinline__ void place(uint32_t d, int& x, int& y) {
    x = 512 + (int)((d & 0xFFFu) % 3072u);
    y = 512 + (int)(((d >> 12) & 0xFFFu) % 3072u);
  }

  static __device__ __forceinline__ void new_episode(World& w, WorldCount& c, const Params&, uint32_t seed, uint32_t env) {
    place(world_hash(seed, env, c.draws++), w.px, w.py);
    place(world_hash(seed, env, c.draws++), w.tx, w.ty);
    w.vx = w.vy = w.got = 0;
    c.ep_steps = 0;
  }

  static __device__ __forceinline__ int cells(const World& w) { return (abs(w.px - w.tx) + abs(w.py - w.ty)) / POINT_CELL; }

  // one axis: v = clamp(v + floor(q / 8), -VMAX, VMAX), p += v, the walls stop the point (q >> 3 is the floor: q is signed)
  static __device__ __forceinline__ void axis(int& p, int& v, int q) {
    v = world_clamp(v + (q >> 3), -POINT_VMAX, POINT_VMAX);
    p += v;
    if (p < 0) { p = 0; v = 0; }
    if (p > POINT_P - 1) { p = POINT_P - 1; v = 0; }
  }

  // One game frame of one world, in registers (no memory access).  a: the packed pair.  -> the reward; over: the episode
  // ended and the world has been restarted; end keeps the world that won or ran out of frames (lane_world.h)
  template <typename E>
  static __device__ __forceinline__ int frame(World& w, WorldCount& c, int a, const Params& p, uint32_t seed, uint32_t env,
                                              bool& over, E& end) {
    ++c.steps;
    ++c.ep_steps;
    const int d0 = cells(w);
    axis(w.px, w.vx, point_byte(a, 0));
    axis(w.py, w.vy, point_byte(a, 8));
    const int d1 = cells(w);
    const bool reached = d1 == 0;
    const int r = d0 - d1 + (reached ? POINT_REACH_BONUS : 0);
    w.got += reached;
    over = w.got >= p.targets_to_win || c.ep_steps >= p.max_episode_steps;
    if (over) end.keep(w, w.got < p.targets_to_win);
    if (over) new_episode(w, c, p, seed, env);
    else if (reached) place(world_hash(seed, env, c.draws++), w.tx, w.ty);
    return r;
  }

  // real dones only
  static __device__ __forceinline__ bool closes(bool over, int) { return over; }

  // the observation: 8 floats, each an integer times a power of two (exact in fp32), as two quads
  static __device__ __forceinline__ void observe(const World& w, float4& lo, float4& hi) {
    constexpr float P12 = 1.f / 4096.f, P6 = 1.f / 64.f, P3 = 1.f / 8.f;
    lo = make_float4((float)(2 * w.px - (POINT_P - 1)) * P12, (float)(2 * w.py - (POINT_P - 1)) * P12, (float)w.vx * P6,
                     (float)w.vy * P6);
    hi = make_float4((float)(w.tx - w.px) * P12, (float)(w.ty - w.py) * P12, (float)w.got * P3, 1.f);
  }
};

}  // namespace
