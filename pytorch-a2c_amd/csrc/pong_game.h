// The Pong game of pong.hip and pong_rules.hip: PongGame, the rules of one game frame on PONG_WORDS int32 state words per env and
// the 80 x 80 prepped frame row, as the game type G of world.h's scaffold (DESIGN.md sections 6c and 6h).  A header so that
// the two files compile it into code objects of their own (why: DESIGN.md section 6i).
#pragma once
#include "world.h"

namespace {

constexpr int PONG_WORDS = 16;      // agent y, opponent y, ball x, ball y, vx, vy, agent score, opponent score, draws, steps,
                                    // episode steps, reward since the last done, the action of the previous game frame
                                    // (sticky actions; 0 without them), 3 spare
constexpr int PW = 80, PH = 80, PONG_HW = PW * PH;
constexpr int PADDLE_H = 8, PADDLE_W = 2, BALL = 2;
constexpr int OPP_X = 8, AGENT_X = 70;
constexpr int PADDLE_MAX_Y = PH - PADDLE_H, BALL_MAX_Y = PH - BALL;
constexpr int PADDLE_START_Y = 36, SERVE_X = 39, SERVE_Y = 39;
constexpr int MISS_RIGHT = AGENT_X + PADDLE_W, MISS_LEFT = OPP_X - BALL;
constexpr int MAX_POINTS = 21, MAX_EPISODE_STEPS = 1 << 24, MAX_SKILL_DEN = 1 << 16;

// the hit table: off = ball y + 1 - paddle y in 0..8 -> vy = {-2,-2,-1,-1,0,1,1,2,2}[off], |vx| = {2,2,1,1,1,1,1,2,2}[off]
__device__ __forceinline__ int pong_hit_vy(int off) { return off <= 1 ? -2 : (off <= 3 ? -1 : (off == 4 ? 0 : (off <= 6 ? 1 : 2))); }
__device__ __forceinline__ int pong_hit_speed(int off) { return (off <= 1 || off >= 7) ? 2 : 1; }

__device__ __forceinline__ bool pong_in(int x, int y, int rx, int ry, int rw, int rh) {
  return x >= rx && x < rx + rw && y >= ry && y < ry + rh;
}

struct PongGame {
  static constexpr int WORDS = PONG_WORDS, HW = PONG_HW, N_ACTIONS = 3;
  struct World {
    int ay, oy, bx, by, vx, vy, sa, so;
  };
  struct Params {
    int points_to_win, max_episode_steps, skill_num, skill_den;
  };

  static bool params_ok(const Params& p) {
    return p.points_to_win >= 1 && p.points_to_win <= MAX_POINTS && p.max_episode_steps >= 1 &&
           p.max_episode_steps <= MAX_EPISODE_STEPS && p.skill_den >= 1 && p.skill_den <= MAX_SKILL_DEN && p.skill_num >= 0 &&
           p.skill_num <= p.skill_den;
  }

  static __device__ __forceinline__ void load(const int32_t* st, World& w, WorldCount& c) {
    w.ay = st[0]; w.oy = st[1]; w.bx = st[2]; w.by = st[3]; w.vx = st[4]; w.vy = st[5]; w.sa = st[6]; w.so = st[7];
    c.draws = (uint32_t)st[8]; c.steps = st[9]; c.ep_steps = st[10]; c.ep_rew = st[11]; c.prev = st[12];
  }

  static __device__ __forceinline__ void store(int32_t* st, const World& w, const WorldCount& c, int lane) {
    if (lane < PONG_WORDS) {
      const int hv = lane == 0 ? w.ay : lane == 1 ? w.oy : lane == 2 ? w.bx : lane == 3 ? w.by : lane == 4 ? w.vx
                   : lane == 5 ? w.vy : lane == 6 ? w.sa : lane == 7 ? w.so : lane == 8 ? (int)c.draws : lane == 9 ? c.steps
                   : lane == 10 ? c.ep_steps : lane == 11 ? c.ep_rew : lane == 12 ? c.prev : 0;
      st[lane] = hv;
    }
  }

  static __device__ __forceinline__ void serve(World& w, uint32_t d, bool towards_agent) {
    w.bx = SERVE_X; w.by = SERVE_Y;
    w.vx = towards_agent ? 1 : -1;
    w.vy = (int)((d >> 1) % 5u) - 2;
  }

  static __device__ __forceinline__ void new_episode(World& w, WorldCount& c, const Params&, uint32_t seed, uint32_t env) {
    w.ay = w.oy = PADDLE_START_Y;
    w.sa = w.so = 0;
    c.ep_steps = 0;
    const uint32_t d = world_hash(seed, env, c.draws++);
    serve(w, d, (d & 1u) != 0u);
  }

  // One game frame of one world, in registers (wave-uniform; no memory access).  -> the reward; over: the episode ended and
  // the world has been restarted (the picture worlds report nothing about the frame that ended it: world.h, WorldNoEnd)
  template <typename E>
  static __device__ __forceinline__ int frame(World& w, WorldCount& c, int a, const Params& p, uint32_t seed, uint32_t env,
                                              bool& over, E&) {
    ++c.steps;
    ++c.ep_steps;
    // 1. the agent's paddle
    w.ay = world_clamp(w.ay + (a == 1 ? -2 : (a == 2 ? 2 : 0)), 0, PADDLE_MAX_Y);
    // 2. the opponent's paddle: towards the ball's centre, on the steps the draw allows
    if ((int)(world_hash(seed, env, c.draws++) % (uint32_t)p.skill_den) < p.skill_num) {
      const int cb = w.by + 1, cp = w.oy + PADDLE_H / 2;
      w.oy = world_clamp(w.oy + (cb < cp ? -1 : (cb > cp ? 1 : 0)), 0, PADDLE_MAX_Y);
    }
    // 3. the ball, the walls
    const int x0 = w.bx;
    int x = x0 + w.vx, y = w.by + w.vy;
    if (y < 0) { y = -y; w.vy = -w.vy; }
    else if (y > BALL_MAX_Y) { y = 2 * BALL_MAX_Y - y; w.vy = -w.vy; }
    // 4. the paddles
    if (w.vx > 0 && x0 + 1 < AGENT_X && x + 1 >= AGENT_X && y >= w.ay - 1 && y <= w.ay + PADDLE_H - 1) {
      const int off = y + 1 - w.ay;
      x = AGENT_X - BALL; w.vx = -pong_hit_speed(off); w.vy = pong_hit_vy(off);
    } else if (w.vx < 0 && x0 > OPP_X + 1 && x <= OPP_X + 1 && y >= w.oy - 1 && y <= w.oy + PADDLE_H - 1) {
      const int off = y + 1 - w.oy;
      x = OPP_X + PADDLE_W; w.vx = pong_hit_speed(off); w.vy = pong_hit_vy(off);
    }
    w.bx = x; w.by = y;
    // 5. a point.  Values, not `if (..) { r = -1; ++w.so; } else if (..) { r = 1; ++w.sa; }`: the compiler made of that a
    // run-time-indexed slot in private memory, 12 bytes per lane in every step kernel
    const int r = x >= MISS_RIGHT ? -1 : (x <= MISS_LEFT ? 1 : 0);
    w.so += r < 0;
    w.sa += r > 0;
    // 6. the end of the episode, or the serve
    over = w.sa >= p.points_to_win || w.so >= p.points_to_win || c.ep_steps >= p.max_episode_steps;
    if (over) new_episode(w, c, p, seed, env);
    else if (r != 0) serve(w, world_hash(seed, env, c.draws++), r < 0);
    return r;
  }

  // the `done` of a "Pong" env type (runner.py:212-214): the real done, or a point
  static __device__ __forceinline__ bool closes(bool over, int R) { return over || R != 0; }

  // the prepped frame row: PONG_HW floats as float4 stores, 4 pixels of one row each (PW % 4 == 0), by `nthreads` lanes, to
  // `frame` and / or `frame2` (either may be null)
  static __device__ __forceinline__ void write_frame(const World& w, float* __restrict__ frame, float* __restrict__ frame2,
                                                     int tid, int nthreads) {
    float4* f4 = reinterpret_cast<float4*>(frame);
    float4* g4 = reinterpret_cast<float4*>(frame2);
    for (int q = tid; q < PONG_HW / 4; q += nthreads) {
      const int y = q / (PW / 4), x0 = 4 * (q - y * (PW / 4));
      float v[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int x = x0 + j;
        const bool on = pong_in(x, y, OPP_X, w.oy, PADDLE_W, PADDLE_H) || pong_in(x, y, AGENT_X, w.ay, PADDLE_W, PADDLE_H) ||
                        pong_in(x, y, w.bx, w.by, BALL, BALL);
        v[j] = on ? 1.0f : 0.0f;
      }
      if (f4 != nullptr) f4[q] = make_float4(v[0], v[1], v[2], v[3]);
      if (g4 != nullptr) g4[q] = make_float4(v[0], v[1], v[2], v[3]);
    }
  }
};

}  // namespace
