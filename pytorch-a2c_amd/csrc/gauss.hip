// Continuous (Gaussian) action heads of FCModel / GRUFCModel: sigma + sampling, and the reference's Gaussian loss
// (models.py:396-405, runner.py:98-104, updater.py:108-117).  The heads rows are [mu (n) | raw (n) | value]; sigma =
// softplus(raw) + 1e-4 with torch's threshold 20.  The loss needs batch-wide sums (F.mse_loss reduces over the whole
// (N, n) block), so it is two launches: a2c_gauss_loss_sums (fp64 partials, fixed-order grid reduction) and
// a2c_gauss_loss_fwd_bwd (gradients from the -- possibly all-reduced -- sums).  One lane per row; the rows are short
// (n <= A2C_GAUSS_MAX_N), so every launch is latency bound at the reference's sizes.  a2c_gauss_nll_fwd_bwd is the
// per-sample log-likelihood loss (hyps["gauss_loss"] = "exact"): one launch, no batch-wide sums.
#include "a2c_common.h"

namespace {
constexpr float kR2PI = 2.5066282746310002f;     // float(np.sqrt(2*np.pi)) as torch applies it to a float32 tensor
constexpr int kSumsBlocks = 512;                  // 6 partials per workgroup must fit A2C_REDUCE_SCRATCH_DOUBLES
static_assert(8 + 6 * kSumsBlocks <= A2C_REDUCE_SCRATCH_DOUBLES, "gauss loss sums: reduce scratch too small");

// torch.nn.functional.softplus (beta 1, threshold 20) + 1e-4
__device__ __forceinline__ float gauss_sigma(float raw) {
  return __fadd_rn(raw > 20.f ? raw : log1pf(expf(raw)), 1e-4f);
}

struct AdvNorm {
  float mean = 0.f, den = 1.f;
  bool on = false;
};
__device__ __forceinline__ AdvNorm adv_norm(const double* adv_sums, long n_global) {
  AdvNorm a;
  if (adv_sums != nullptr) {       // same statistics as loss_kernel (loss.hip) / a2c_normalize
    const double m = adv_sums[0] / (double)n_global;
    double var = (adv_sums[1] - (double)n_global * m * m) / (double)(n_global - 1);
    if (var < 0.0) var = 0.0;
    a.mean = (float)m;
    a.den = (float)sqrt(var) + 1e-6f;
    a.on = true;
  }
  return a;
}

// PUB: the thread that computes action (b, j) also hands it to env b's worker -- granule (step << 32) | bits, then (j == 0) the
// doorbell; per-lane system-scope 8-byte stores, each granule self-tagged (a2c_hostpool.h), so their order does not matter
template <bool PUB>
__global__ __launch_bounds__(256) void gauss_head_kernel(const float* __restrict__ heads, long ldh, const float* __restrict__ eps,
                                                         long lde, float* __restrict__ sigma, long lds,
                                                         float* __restrict__ actions, long lda, long B, int n,
                                                         unsigned long long* __restrict__ act, long act_stride,
                                                         unsigned long long* __restrict__ cmd,
                                                         const unsigned int* __restrict__ seq_base, unsigned int seq_off) {
  const long total = B * (long)n;
  unsigned long long tag = 0;
  if (PUB) tag = (unsigned long long)(seq_base[0] + seq_off) << 32;
  for (long e = blockIdx.x * 256L + threadIdx.x; e < total; e += gridDim.x * 256L) {
    const long b = e / n;
    const int j = (int)(e - b * n);
    const float* row = heads + b * ldh;
    const float s = gauss_sigma(row[n + j]);
    if (sigma != nullptr) sigma[b * lds + j] = s;
    if (actions != nullptr) {
      const float a = __fadd_rn(row[j], __fmul_rn(s, eps[b * lde + j]));   // mu + (sigma*eps)
      actions[b * lda + j] = a;
      if (PUB) {
        __hip_atomic_store(act + b * act_stride + j, tag | (unsigned long long)__float_as_uint(a), __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_SYSTEM);
        if (j == 0) __hip_atomic_store(cmd + b, tag | (unsigned long long)(unsigned int)n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
      }
    }
  }
}

// sums[0..6) = [sum d^2, sum w/(2c), sum w*l, sum l, sum adv (n == 1), sum (V-R)^2]; w = adv (n >= 2) or 1 (n == 1: the
// batch mean of the advantages multiplies these two sums in the second launch)
__global__ __launch_bounds__(256) void gauss_sums_kernel(const float* __restrict__ heads, long ldh, const float* __restrict__ vals,
                                                         long vstride, const float* __restrict__ actions, long lda,
                                                         const float* __restrict__ advs, const float* __restrict__ returns,
                                                         const double* __restrict__ adv_sums, long n_local, long n_global,
                                                         int n, double* sums, double* scratch) {
  __shared__ double sm[4];
  const AdvNorm an = adv_norm(adv_sums, n_global);
  double s[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (long i = blockIdx.x * 256L + threadIdx.x; i < n_local; i += gridDim.x * 256L) {
    float adv = advs[i];
    if (an.on) adv = (adv - an.mean) / an.den;
    const float w = n == 1 ? 1.f : adv;
    const float* row = heads + i * ldh;
    const float* act = actions + i * lda;
    float sd = 0.f, sk = 0.f, sp = 0.f, sl = 0.f;
    for (int j = 0; j < n; ++j) {
      const float sg = gauss_sigma(row[n + j]);
      const float d = row[j] - act[j];
      const float c = fmaxf(sg * sg, 1e-3f);
      const float l = logf(fmaxf(kR2PI * sg, 1e-3f));
      sd += d * d;
      sk += w / (2.f * c);
      sp += w * l;
      sl += l;
    }
    const float dv = vals[i * vstride] - returns[i];
    s[0] += (double)sd;
    s[1] += (double)sk;
    s[2] += (double)sp;
    s[3] += (double)sl;
    s[4] += n == 1 ? (double)adv : 0.0;
    s[5] += (double)(dv * dv);
  }
#pragma unroll
  for (int k = 0; k < 6; ++k) s[k] = block_sum_256(s[k], sm);
  grid_sum_ordered<6>(s, sums, scratch, sm);
}

__global__ __launch_bounds__(256) void gauss_fwd_bwd_kernel(const float* __restrict__ heads, long ldh,
                                                            const float* __restrict__ vals, long vstride,
                                                            const float* __restrict__ actions, long lda,
                                                            const float* __restrict__ advs, const float* __restrict__ returns,
                                                            const double* __restrict__ adv_sums, const double* __restrict__ sums,
                                                            long n_local, long n_global, int n, float pi_coef, float val_coef,
                                                            float entr_coef, float* __restrict__ dheads, long ldd,
                                                            float* __restrict__ dvals, long dvstride, double* loss_sums) {
  const AdvNorm an = adv_norm(adv_sums, n_global);
  const double M = (double)n_global * (double)n;
  const double adv_mean = sums[4] / (double)n_global;
  const double K = n == 1 ? sums[1] * adv_mean : sums[1];
  const double P = n == 1 ? sums[2] * adv_mean : sums[2];
  const double mse = sums[0] / M;
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    // Updater._finish_host divides every sum by n_global and all-reduces them over the ranks when sharded: each rank
    // writes its share (n_local / n_global) of the global values (the whole value on one GPU)
    const double share = (double)n_local / (double)n_global;
    loss_sums[0] = -(mse * K + P) / (double)n * share;
    loss_sums[1] = sums[5] * share;
    loss_sums[2] = sums[3] / (double)n * share;
  }
  const float g_mu = (float)((double)pi_coef * K / M * 2.0 / M);     // dL/dmu = g_mu * (mu - a)
  const float g_pi = (float)((double)pi_coef / M);
  const float g_en = (float)((double)entr_coef / M);
  const float mse_f = (float)mse;
  const float w1 = (float)adv_mean;
  const float invN = 1.0f / (float)n_global;
  for (long i = blockIdx.x * 256L + threadIdx.x; i < n_local; i += gridDim.x * 256L) {
    float adv = advs[i];
    if (an.on) adv = (adv - an.mean) / an.den;
    const float w = n == 1 ? w1 : adv;
    const float* row = heads + i * ldh;
    const float* act = actions + i * lda;
    float* drow = dheads + i * ldd;
    for (int j = 0; j < n; ++j) {
      const float raw = row[n + j];
      const float sg = gauss_sigma(raw);
      const float s2 = sg * sg;
      const float c = fmaxf(s2, 1e-3f);
      const float q = kR2PI * sg;
      // torch's clamp backward passes the gradient where input >= min
      const float dc = s2 >= 1e-3f ? 2.f * sg : 0.f;
      const float dl = q >= 1e-3f ? kR2PI / q : 0.f;
      const float dsig = g_pi * w * (-mse_f / (2.f * c * c) * dc + dl) + g_en * dl;
      float draw = dsig;
      if (!(raw > 20.f)) {             // softplus backward: g * z / (z + 1), z = exp(raw)
        const float z = expf(raw);
        draw = dsig * z / (z + 1.f);
      }
      drow[j] = g_mu * (row[j] - act[j]);
      drow[n + j] = draw;
    }
    const float dv = vals[i * vstride] - returns[i];
    dvals[i * dvstride] = val_coef * 2.f * dv * invN;
  }
}
// The per-sample Gaussian log-likelihood loss (hyps["gauss_loss"] = "exact"), forward and backward in one pass like
// loss_kernel (loss.hip): every row's gradient needs only that row and the advantage statistics, so there is no first
// launch for batch-wide sums.  The row's two sums over the action dims are kept in fp64 (u^2 reaches 1e8 on a tiny-sigma
// row and would swallow the log sigma terms in fp32); the gradients are fp32.
constexpr double kHalfLog2Pi = 0.91893853320467274178;

// one row's gradients [dmu | draw] from its policy weight gpi (-pi_coef w / N; times the ratio, or 0: gauss_ppo_kernel) and
// gen = entr_coef / N; su2 = sum_j u^2, sls = sum_j log sigma.  The ONE row body of gauss_nll_kernel and gauss_ppo_kernel.
__device__ __forceinline__ void gauss_nll_row(const float* __restrict__ row, const float* __restrict__ act, int n, float gpi,
                                              float gen, float* __restrict__ drow, double& su2, double& sls) {
  su2 = 0.0;
  sls = 0.0;
  for (int j = 0; j < n; ++j) {
    const float raw = row[n + j];
    const float sg = gauss_sigma(raw);
    const float inv_s = 1.f / sg;
    const float u = (act[j] - row[j]) * inv_s;
    const float dsig = (gpi * (u * u - 1.f) - gen) * inv_s;
    float draw = dsig;
    if (!(raw > 20.f)) {               // softplus backward: g * z / (z + 1), z = exp(raw)
      const float z = expf(raw);
      draw = dsig * z / (z + 1.f);
    }
    drow[j] = gpi * u * inv_s;
    drow[n + j] = draw;
    su2 += (double)(u * u);
    sls += (double)logf(sg);
  }
}

// logp of one row before any of its gradients can be written (gauss_ppo_kernel's first pass over the n dims): fp64 from the
// fp32 heads and actions on, sigma included, so that the ratio's exponent carries no fp32 rounding (|logp| reaches 1e3 at
// n = 64, where an fp32 ulp is 1e-4)
__device__ __forceinline__ double gauss_row_logp(const float* __restrict__ row, const float* __restrict__ act, int n) {
  double lp = 0.0;
  for (int j = 0; j < n; ++j) {
    const double raw = (double)row[n + j];
    const double sg = (raw > 20.0 ? raw : log1p(exp(raw))) + 1e-4;
    const double u = ((double)act[j] - (double)row[j]) / sg;
    lp -= 0.5 * u * u + log(sg);
  }
  return lp - (double)n * kHalfLog2Pi;
}

__global__ __launch_bounds__(256) void gauss_nll_kernel(const float* __restrict__ heads, long ldh, const float* __restrict__ vals,
                                                        long vstride, const float* __restrict__ actions, long lda,
                                                        const float* __restrict__ advs, const float* __restrict__ returns,
                                                        const double* __restrict__ adv_sums, long n_local, long n_global, int n,
                                                        float pi_coef, float val_coef, float entr_coef,
                                                        float* __restrict__ dheads, long ldd, float* __restrict__ dvals,
                                                        long dvstride, double* loss_sums, double* scratch) {
  __shared__ double sm[4];
  const AdvNorm an = adv_norm(adv_sums, n_global);
  const float invN = 1.0f / (float)n_global;
  const float gen = entr_coef * invN;
  double s_pi = 0.0, s_val = 0.0, s_ent = 0.0;
  for (long i = blockIdx.x * 256L + threadIdx.x; i < n_local; i += gridDim.x * 256L) {
    float w = advs[i];
    if (an.on) w = (w - an.mean) / an.den;
    const float gpi = -pi_coef * w * invN;
    double su2, sls;                     // sum_j u^2, sum_j log sigma
    gauss_nll_row(heads + i * ldh, actions + i * lda, n, gpi, gen, dheads + i * ldd, su2, sls);
    const float dv = vals[i * vstride] - returns[i];
    dvals[i * dvstride] = val_coef * 2.f * dv * invN;
    s_pi += (double)w * (-0.5 * su2 - sls - (double)n * kHalfLog2Pi);
    s_val += (double)(dv * dv);
    s_ent -= (double)n * (0.5 + kHalfLog2Pi) + sls;
  }
  s_pi = block_sum_256(s_pi, sm);
  s_val = block_sum_256(s_val, sm);
  s_ent = block_sum_256(s_ent, sm);
  const double v3[3] = {s_pi, s_val, s_ent};
  grid_sum_ordered<3>(v3, loss_sums, scratch, sm);       // fixed-order second stage: no fp64 atomics
}

// The clipped-ratio (PPO) loss of the multi-epoch update (hyps["ppo_epochs"] >= 2) on gauss_nll_kernel's
// rows: two passes over a row's n dims (logp first: the ratio scales every gradient of the row), the second one
// gauss_nll_row with the policy weight times r inside the clip range and exactly zero where the clip binds.  RECORD: the
// first epoch, r = 1 -- writes logp_old and gauss_nll_kernel's gradients bit for bit.
template <bool RECORD>
__global__ __launch_bounds__(256) void gauss_ppo_kernel(const float* __restrict__ heads, long ldh, const float* __restrict__ vals,
                                                        long vstride, const float* __restrict__ actions, long lda,
                                                        const float* __restrict__ advs, const float* __restrict__ returns,
                                                        const double* __restrict__ adv_sums, long n_local, long n_global, int n,
                                                        float pi_coef, float val_coef, float entr_coef, float clip,
                                                        double* __restrict__ logp_old, float* __restrict__ dheads, long ldd,
                                                        float* __restrict__ dvals, long dvstride, double* loss_sums,
                                                        double* scratch) {
  __shared__ double sm[4];
  const AdvNorm an = adv_norm(adv_sums, n_global);
  const float invN = 1.0f / (float)n_global;
  const float gen = entr_coef * invN;
  double s[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
  for (long i = blockIdx.x * 256L + threadIdx.x; i < n_local; i += gridDim.x * 256L) {
    float w = advs[i];
    if (an.on) w = (w - an.mean) / an.den;
    float gpi = -pi_coef * w * invN;
    const float* row = heads + i * ldh;
    const float* act = actions + i * lda;
    const double logp = gauss_row_logp(row, act, n);
    if (RECORD) {
      logp_old[i] = logp;
      s[0] += (double)w;
    } else {
      const PpoRow pr = ppo_row(logp - logp_old[i], w, clip);
      gpi = pr.keep ? (float)((double)gpi * pr.r) : 0.f;      // one rounding; r == 1 leaves gpi as it is
      s[0] += pr.surr;
      s[3] += pr.keep ? 0.0 : 1.0;
      s[4] += pr.kl;
    }
    double su2, sls;
    gauss_nll_row(row, act, n, gpi, gen, dheads + i * ldd, su2, sls);
    const float dv = vals[i * vstride] - returns[i];
    dvals[i * dvstride] = val_coef * 2.f * dv * invN;
    s[1] += (double)(dv * dv);
    s[2] -= (double)n * (0.5 + kHalfLog2Pi) + sls;
  }
#pragma unroll
  for (int k = 0; k < 5; ++k) s[k] = block_sum_256(s[k], sm);
  grid_sum_ordered<5>(s, loss_sums, scratch, sm);
}
}  // namespace

extern "C" int a2c_gauss_head_publish(const float* heads, int64_t ld_heads, const float* eps, int64_t ld_eps, float* sigma,
                                      int64_t ld_sigma, float* actions, int64_t ld_act, int64_t B, int n, uint64_t* act,
                                      int64_t act_stride, uint64_t* cmd, const uint32_t* seq_base, uint32_t seq_off,
                                      a2c_stream_t stream) {
  if (B < 0 || n < 1 || n > A2C_GAUSS_MAX_N || ld_heads < 2 * n) return A2C_ERR_ARG;
  if (sigma == nullptr && actions == nullptr) return A2C_ERR_ARG;
  if (sigma != nullptr && ld_sigma < n) return A2C_ERR_ARG;
  if (actions != nullptr && (eps == nullptr || ld_eps < n || ld_act < n)) return A2C_ERR_ARG;
  if (cmd != nullptr && (actions == nullptr || act == nullptr || seq_base == nullptr || act_stride < n)) return A2C_ERR_ARG;
  if (B == 0) return A2C_OK;
  if (heads == nullptr) return A2C_ERR_ARG;
  const dim3 grid(a2c_grid_1d(B * n, 256));
  if (cmd != nullptr)
    hipLaunchKernelGGL(gauss_head_kernel<true>, grid, dim3(256), 0, a2c_s(stream), heads, (long)ld_heads, eps, (long)ld_eps,
                       sigma, (long)ld_sigma, actions, (long)ld_act, (long)B, n, (unsigned long long*)act, (long)act_stride,
                       (unsigned long long*)cmd, seq_base, seq_off);
  else
    hipLaunchKernelGGL(gauss_head_kernel<false>, grid, dim3(256), 0, a2c_s(stream), heads, (long)ld_heads, eps, (long)ld_eps,
                       sigma, (long)ld_sigma, actions, (long)ld_act, (long)B, n, (unsigned long long*)nullptr, 0L,
                       (unsigned long long*)nullptr, (const unsigned int*)nullptr, 0u);
  A2C_CHECK_LAUNCH();
  return A2C_OK;
}

extern "C" int a2c_gauss_head(const float* heads, int64_t ld_heads, const float* eps, int64_t ld_eps, float* sigma,
                              int64_t ld_sigma, float* actions, int64_t ld_act, int64_t B, int n, a2c_stream_t stream) {
  return a2c_gauss_head_publish(heads, ld_heads, eps, ld_eps, sigma, ld_sigma, actions, ld_act, B, n, nullptr, 0, nullptr,
                                nullptr, 0u, stream);
}

extern "C" int a2c_gauss_loss_sums(const float* heads, int64_t ld_heads, const float* vals, int64_t val_stride,
                                   const float* actions, int64_t ld_act, const float* advs, const float* returns,
                                   const double* adv_sums, int64_t n_local, int64_t n_global, int n, double* sums,
                                   double* scratch, a2c_stream_t stream) {
  if (n_local < 0 || n_global < n_local || n_global < 1 || n < 1 || n > A2C_GAUSS_MAX_N || !sums || !scratch)
    return A2C_ERR_ARG;
  if (adv_sums && n_global < 2) return A2C_ERR_ARG;
  if (n_local == 0) {
    a2c_zero_async(sums, 6 * sizeof(double), a2c_s(stream));
    return A2C_OK;
  }
  if (!heads || !vals || !actions || !advs || !returns || ld_heads < 2 * n || ld_act < n) return A2C_ERR_ARG;
  hipLaunchKernelGGL(gauss_sums_kernel, dim3(a2c_grid_1d(n_local, 256, kSumsBlocks)), dim3(256), 0, a2c_s(stream), heads,
                     (long)ld_heads, vals, (long)val_stride, actions, (long)ld_act, advs, returns, adv_sums, (long)n_local,
                     (long)n_global, n, sums, scratch);
  A2C_CHECK_LAUNCH();
  return A2C_OK;
}

extern "C" int a2c_gauss_loss_fwd_bwd(const float* heads, int64_t ld_heads, const float* vals, int64_t val_stride,
                                      const float* actions, int64_t ld_act, const float* advs, const float* returns,
                                      const double* adv_sums, const double* sums, int64_t n_local, int64_t n_global, int n,
                                      float pi_coef, float val_coef, float entr_coef, float* dheads, int64_t ldd,
                                      float* dvals, int64_t dval_stride, double* loss_sums, a2c_stream_t stream) {
  if (n_local < 0 || n_global < n_local || n_global < 1 || n < 1 || n > A2C_GAUSS_MAX_N || !sums || !loss_sums)
    return A2C_ERR_ARG;
  if (adv_sums && n_global < 2) return A2C_ERR_ARG;
  if (n_local == 0) {
    a2c_zero_async(loss_sums, 3 * sizeof(double), a2c_s(stream));
    return A2C_OK;
  }
  if (!heads || !vals || !actions || !advs || !returns || !dheads || !dvals || ld_heads < 2 * n || ld_act < n || ldd < 2 * n)
    return A2C_ERR_ARG;
  hipLaunchKernelGGL(gauss_fwd_bwd_kernel, dim3(a2c_grid_1d(n_local, 256)), dim3(256), 0, a2c_s(stream), heads,
                     (long)ld_heads, vals, (long)val_stride, actions, (long)ld_act, advs, returns, adv_sums, sums,
                     (long)n_local, (long)n_global, n, pi_coef, val_coef, entr_coef, dheads, (long)ldd, dvals,
                     (long)dval_stride, loss_sums);
  A2C_CHECK_LAUNCH();
  return A2C_OK;
}

extern "C" int a2c_gauss_nll_fwd_bwd(const float* heads, int64_t ld_heads, const float* vals, int64_t val_stride,
                                     const float* actions, int64_t ld_act, const float* advs, const float* returns,
                                     const double* adv_sums, int64_t n_local, int64_t n_global, int n, float pi_coef,
                                     float val_coef, float entr_coef, float* dheads, int64_t ldd, float* dvals,
                                     int64_t dval_stride, double* loss_sums, double* scratch, a2c_stream_t stream) {
  if (n_local < 0 || n_global < n_local || n_global < 1 || n < 1 || n > A2C_GAUSS_MAX_N || !loss_sums || !scratch)
    return A2C_ERR_ARG;
  if (adv_sums && n_global < 2) return A2C_ERR_ARG;
  if (n_local == 0) {
    a2c_zero_async(loss_sums, 3 * sizeof(double), a2c_s(stream));
    return A2C_OK;
  }
  if (!heads || !vals || !actions || !advs || !returns || !dheads || !dvals || ld_heads < 2 * n || ld_act < n || ldd < 2 * n)
    return A2C_ERR_ARG;
  hipLaunchKernelGGL(gauss_nll_kernel, dim3(a2c_grid_1d(n_local, 256, A2C_REDUCE_MAX_BLOCKS)), dim3(256), 0, a2c_s(stream),
                     heads, (long)ld_heads, vals, (long)val_stride, actions, (long)ld_act, advs, returns, adv_sums,
                     (long)n_local, (long)n_global, n, pi_coef, val_coef, entr_coef, dheads, (long)ldd, dvals,
                     (long)dval_stride, loss_sums, scratch);
  A2C_CHECK_LAUNCH();
  return A2C_OK;
}

extern "C" int a2c_gauss_ppo_fwd_bwd(const float* heads, int64_t ld_heads, const float* vals, int64_t val_stride,
                                     const float* actions, int64_t ld_act, const float* advs, const float* returns,
                                     const double* adv_sums, int64_t n_local, int64_t n_global, int n, float pi_coef,
                                     float val_coef, float entr_coef, float clip, int record, double* logp_old, float* dheads,
                                     int64_t ldd, float* dvals, int64_t dval_stride, double* loss_sums, double* scratch,
                                     a2c_stream_t stream) {
  if (n_local < 0 || n_global < n_local || n_global < 1 || n < 1 || n > A2C_GAUSS_MAX_N || !loss_sums || !scratch)
    return A2C_ERR_ARG;
  if (adv_sums && n_global < 2) return A2C_ERR_ARG;
  if (!(clip > 0.f) || clip == INFINITY || (record != 0 && record != 1) || !logp_old) return A2C_ERR_ARG;
  if (n_local == 0) {
    a2c_zero_async(loss_sums, 5 * sizeof(double), a2c_s(stream));
    return A2C_OK;
  }
  if (!heads || !vals || !actions || !advs || !returns || !dheads || !dvals || ld_heads < 2 * n || ld_act < n || ldd < 2 * n)
    return A2C_ERR_ARG;
  const dim3 grid(a2c_grid_1d(n_local, 256, A2C_PPO_MAX_BLOCKS));
  if (record)
    hipLaunchKernelGGL(gauss_ppo_kernel<true>, grid, dim3(256), 0, a2c_s(stream), heads, (long)ld_heads, vals, (long)val_stride,
                       actions, (long)ld_act, advs, returns, adv_sums, (long)n_local, (long)n_global, n, pi_coef, val_coef,
                       entr_coef, clip, logp_old, dheads, (long)ldd, dvals, (long)dval_stride, loss_sums, scratch);
  else
    hipLaunchKernelGGL(gauss_ppo_kernel<false>, grid, dim3(256), 0, a2c_s(stream), heads, (long)ld_heads, vals, (long)val_stride,
                       actions, (long)ld_act, advs, returns, adv_sums, (long)n_local, (long)n_global, n, pi_coef, val_coef,
                       entr_coef, clip, logp_old, dheads, (long)ldd, dvals, (long)dval_stride, loss_sums, scratch);
  A2C_CHECK_LAUNCH();
  return A2C_OK;
}
