// Running observation / reward normalisation of the vector worlds: a2c_vecnorm_init / a2c_vecnorm_step (rule: DESIGN.md
// section 6m; host twin: a2c_amd/vecnorm.py), what baselines' VecNormalize does, as one launch behind a step's post launch.
//
// ONE workgroup of 256 lanes per launch: B is a few hundred envs of 4 - 8 floats, and the running moments need one owner.
// The statistics are doubles in device memory and every sum has a fixed order -- lane i adds envs i, i + 256, ... in order,
// then a halving tree over the lanes through LDS (strides 128 .. 1) -- so the block is a pure function of the launches played,
// whatever the scheduling, and the host twin reproduces it bit for bit.  Up to VN_CHUNK features share a tree's barriers
// (each feature's own sums are untouched by that: a tree stage adds the same two partials either way).  All arithmetic is
// fp64, never contracted (the library is built with -ffp-contract=off), and rounded to fp32 once, at the store.
#include "a2c_common.h"

namespace {

constexpr int VN_LANES = 256;
constexpr int VN_CHUNK = 8;       // features reduced together: 16 KiB of LDS
constexpr int VN_MAX_L = 64;

// s[f][lane] holds lane's partial of feature f -> s[f][0] = the sum, by the halving tree; every lane of the workgroup calls
__device__ __forceinline__ void vn_tree(double (*s)[VN_LANES], int nf, int lane) {
  __syncthreads();
  for (int stride = VN_LANES / 2; stride > 0; stride >>= 1) {
    if (lane < stride)
      for (int f = 0; f < nf; ++f) s[f][lane] = s[f][lane] + s[f][lane + stride];
    __syncthreads();
  }
}

__device__ __forceinline__ double vn_clamp(double v, double c) { return v < -c ? -c : (v > c ? c : v); }

// the moment-combination rule for a batch of n values with mean bm and biased variance bv; every operation left to right
__device__ __forceinline__ void vn_fold(double& mean, double& var, double count, double n, double bm, double bv) {
  const double delta = bm - mean;
  const double tot = count + n;
  const double m2 = var * count + bv * n + delta * delta * count * n / tot;
  mean = mean + delta * n / tot;
  var = m2 / tot;
}

__global__ __launch_bounds__(VN_LANES) void vecnorm_kernel(double* block, const a2c_vecnorm_args a) {
  __shared__ double s[VN_CHUNK][VN_LANES];
  __shared__ double s_mean[VN_MAX_L], s_std[VN_MAX_L], s_bm[VN_CHUNK], s_rstd;
  const int lane = threadIdx.x, B = a.B, L = a.L;
  const double n = (double)B;
  double* mean = block + 1;
  double* var = block + 1 + L;
  double* rstat = block + 1 + 2 * L;          // return count, mean, var
  double* ret = block + 4 + 2 * L + a.env0;   // the launch's accumulators

  if (a.out != nullptr) {
    float* plane = a.out + (int64_t)(a.C - 1) * L;
    if (a.update != 0) {
      const double count = block[0];
      for (int j0 = 0; j0 < L; j0 += VN_CHUNK) {
        const int nf = L - j0 < VN_CHUNK ? L - j0 : VN_CHUNK;
        double acc[VN_CHUNK];
#pragma unroll
        for (int f = 0; f < VN_CHUNK; ++f) acc[f] = 0.0;
        for (int b = lane; b < B; b += VN_LANES) {
          const float* x = plane + (int64_t)b * a.out_stride + j0;
#pragma unroll
          for (int f = 0; f < VN_CHUNK; ++f)
            if (f < nf) acc[f] = acc[f] + (double)x[f];
        }
#pragma unroll
        for (int f = 0; f < VN_CHUNK; ++f)
          if (f < nf) s[f][lane] = acc[f];
        vn_tree(s, nf, lane);
        if (lane < nf) s_bm[lane] = s[lane][0] / n;
        __syncthreads();
#pragma unroll
        for (int f = 0; f < VN_CHUNK; ++f) acc[f] = 0.0;
        for (int b = lane; b < B; b += VN_LANES) {
          const float* x = plane + (int64_t)b * a.out_stride + j0;
#pragma unroll
          for (int f = 0; f < VN_CHUNK; ++f)
            if (f < nf) {
              const double d = (double)x[f] - s_bm[f];
              acc[f] = acc[f] + d * d;
            }
        }
#pragma unroll
        for (int f = 0; f < VN_CHUNK; ++f)
          if (f < nf) s[f][lane] = acc[f];
        vn_tree(s, nf, lane);
        if (lane < nf) {
          const int j = j0 + lane;
          double m = mean[j], v = var[j];
          vn_fold(m, v, count, n, s_bm[lane], s[lane][0] / n);
          mean[j] = m;
          var[j] = v;
          s_mean[j] = m;
          s_std[j] = sqrt(v + a.eps);
        }
        __syncthreads();
      }
      if (lane == 0) block[0] = count + n;
    } else {
      if (lane < L) {
        s_mean[lane] = mean[lane];
        s_std[lane] = sqrt(var[lane] + a.eps);
      }
      __syncthreads();
    }
    for (int b = lane; b < B; b += VN_LANES) {
      float* x = plane + (int64_t)b * a.out_stride;
      for (int j = 0; j < L; ++j) x[j] = (float)vn_clamp(((double)x[j] - s_mean[j]) / s_std[j], a.clip_obs);
    }
  }

  if (a.rewards != nullptr) {      // (update != 0: the launcher refuses a frozen reward part)
    float* rw = a.rewards + a.slot0 * a.T + a.t;
    const float* dn = a.dones + a.slot0 * a.T + a.t;
    double acc = 0.0;
    for (int b = lane; b < B; b += VN_LANES) {
      const double g = ret[b] * a.gamma + (double)rw[(int64_t)b * a.T];
      ret[b] = g;
      acc = acc + g;
    }
    s[0][lane] = acc;
    vn_tree(s, 1, lane);
    if (lane == 0) s_bm[0] = s[0][0] / n;
    __syncthreads();
    const double bm = s_bm[0];
    acc = 0.0;
    for (int b = lane; b < B; b += VN_LANES) {
      const double d = ret[b] - bm;
      acc = acc + d * d;
    }
    s[0][lane] = acc;
    vn_tree(s, 1, lane);
    if (lane == 0) {
      const double count = rstat[0];
      double m = rstat[1], v = rstat[2];
      vn_fold(m, v, count, n, bm, s[0][0] / n);
      rstat[0] = count + n;
      rstat[1] = m;
      rstat[2] = v;
      s_rstd = sqrt(v + a.eps);
    }
    __syncthreads();
    const double rstd = s_rstd;
    for (int b = lane; b < B; b += VN_LANES) {
      const int64_t e = (int64_t)b * a.T;
      rw[e] = (float)vn_clamp((double)rw[e] / rstd, a.clip_rew);
      if (dn[e] != 0.f) ret[b] = 0.0;
    }
  }
}

__global__ __launch_bounds__(VN_LANES) void vecnorm_init_kernel(double* block, int L, int B_pool) {
  const int n = 4 + 2 * L + B_pool;
  for (int i = blockIdx.x * VN_LANES + threadIdx.x; i < n; i += gridDim.x * VN_LANES) {
    double v = 0.0;                                           // means, ret
    if (i == 0 || i == 1 + 2 * L) v = 1e-4;                   // the two counts
    else if ((i > L && i <= 2 * L) || i == 3 + 2 * L) v = 1.0;      // the vars
    block[i] = v;
  }
}

bool vn_shape_ok(int L, int B_pool) { return L >= 1 && L <= VN_MAX_L && B_pool >= 1; }

}  // namespace

extern "C" size_t a2c_vecnorm_state_bytes(int L, int B_pool) {
  return vn_shape_ok(L, B_pool) ? sizeof(double) * ((size_t)4 + 2 * (size_t)L + (size_t)B_pool) : 0;
}

extern "C" int a2c_vecnorm_init(double* block, int L, int B_pool, a2c_stream_t stream) {
  if (block == nullptr || !vn_shape_ok(L, B_pool)) return A2C_ERR_ARG;
  hipLaunchKernelGGL(vecnorm_init_kernel, dim3(a2c_grid_1d(4 + 2 * (int64_t)L + B_pool, VN_LANES, 64)), dim3(VN_LANES), 0,
                     a2c_s(stream), block, L, B_pool);
  A2C_CHECK_LAUNCH();
  return A2C_OK;
}

extern "C" int a2c_vecnorm_step(double* block, const a2c_vecnorm_args* args, a2c_stream_t stream) {
  if (block == nullptr || args == nullptr) return A2C_ERR_ARG;
  const a2c_vecnorm_args& a = *args;
  if (a.B < 1 || !vn_shape_ok(a.L, a.B_pool) || a.env0 < 0 || (int64_t)a.env0 + a.B > a.B_pool) return A2C_ERR_ARG;
  if (!(a.eps > 0.0) || !(a.clip_obs > 0.0) || !(a.clip_rew > 0.0)) return A2C_ERR_ARG;
  if (a.out == nullptr && a.rewards == nullptr) return A2C_ERR_ARG;
  if (a.out != nullptr && (a.C < 1 || a.out_stride < (int64_t)a.C * a.L)) return A2C_ERR_ARG;
  if (a.rewards != nullptr &&
      (a.dones == nullptr || a.T < 1 || a.t < 0 || a.t >= a.T || a.slot0 < 0 || a.update == 0))
    return A2C_ERR_ARG;
  hipLaunchKernelGGL(vecnorm_kernel, dim3(1), dim3(VN_LANES), 0, a2c_s(stream), block, a);
  A2C_CHECK_LAUNCH();
  return A2C_OK;
}
