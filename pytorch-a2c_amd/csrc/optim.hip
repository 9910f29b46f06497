// Gradient clipping + optimiser step over the flat parameter arena (updater.py:129-132,
// 226-229).  All parameters with a gradient live in one contiguous fp32 arena (params, grads,
// optimiser state are parallel arrays), so clip_grad_norm_ + RMSprop/Adam is two memory-bound
// launches: a sum-of-squares reduction and one fused clip+update pass
// (RMSprop: 4 reads... params, grads, square_avg in; params, grads, square_avg out = 24 B/param;
//  Adam: 32 B/param).  The same arena is the RCCL all-reduce buffer on multi-GPU runs.
#include "a2c_common.h"

namespace {

__global__ __launch_bounds__(256) void sumsq_kernel(const float* __restrict__ g, long n, double* out, double* scratch) {
  __shared__ double sm[4];
  double a = 0.0;
  const long n4 = n >> 2;
  const float4* g4 = reinterpret_cast<const float4*>(g);
  for (long i = blockIdx.x * 256L + threadIdx.x; i < n4; i += gridDim.x * 256L) {
    const float4 v = g4[i];
    a += (double)v.x * v.x + (double)v.y * v.y + (double)v.z * v.z + (double)v.w * v.w;
  }
  for (long i = (n4 << 2) + blockIdx.x * 256L + threadIdx.x; i < n; i += gridDim.x * 256L) a += (double)g[i] * g[i];
  a = block_sum_256(a, sm);
  const double v1[1] = {a};
  grid_sum_ordered<1>(v1, out, scratch, sm);       // fixed-order second stage: no fp64 atomics
}

// torch.nn.utils.clip_grad_norm_: coef = max_norm / (total_norm + 1e-6), clamped to 1.0,
// and the gradients are multiplied by it unconditionally.
__device__ __forceinline__ float clip_coef(const double* sumsq, float max_norm, float* norm_out) {
  const float norm = (float)sqrt(sumsq[0]);
  if (norm_out && blockIdx.x == 0 && threadIdx.x == 0) *norm_out = norm;
  const float c = max_norm / (norm + 1e-6f);
  return c > 1.0f ? 1.0f : c;
}

__device__ __forceinline__ void rmsprop1(float& p, float& g, float& sq, float coef, float lr, float alpha,
                                         float oma, float eps) {
  g = g * coef;
  sq = __fadd_rn(__fmul_rn(sq, alpha), __fmul_rn(__fmul_rn(oma, g), g));  // mul_(alpha).addcmul_(g,g,1-alpha)
  const float avg = __fadd_rn(sqrtf(sq), eps);                            // sqrt().add_(eps)
  p = __fadd_rn(p, __fdiv_rn(__fmul_rn(-lr, g), avg));                    // addcdiv_(g, avg, value=-lr)
}

__global__ __launch_bounds__(256) void clip_rmsprop_kernel(float* __restrict__ p, float* __restrict__ g,
                                                           float* __restrict__ sq, long n, const double* sumsq,
                                                           float max_norm, float lr, float alpha, float oma,
                                                           float eps, float* norm_out) {
  const float coef = clip_coef(sumsq, max_norm, norm_out);
  const long n4 = n >> 2;
  float4* p4 = reinterpret_cast<float4*>(p);
  float4* g4 = reinterpret_cast<float4*>(g);
  float4* s4 = reinterpret_cast<float4*>(sq);
  for (long i = blockIdx.x * 256L + threadIdx.x; i < n4; i += gridDim.x * 256L) {
    float4 pv = p4[i], gv = g4[i], sv = s4[i];
    rmsprop1(pv.x, gv.x, sv.x, coef, lr, alpha, oma, eps);
    rmsprop1(pv.y, gv.y, sv.y, coef, lr, alpha, oma, eps);
    rmsprop1(pv.z, gv.z, sv.z, coef, lr, alpha, oma, eps);
    rmsprop1(pv.w, gv.w, sv.w, coef, lr, alpha, oma, eps);
    p4[i] = pv; g4[i] = gv; s4[i] = sv;
  }
  for (long i = (n4 << 2) + blockIdx.x * 256L + threadIdx.x; i < n; i += gridDim.x * 256L)
    rmsprop1(p[i], g[i], sq[i], coef, lr, alpha, oma, eps);
}

__device__ __forceinline__ void adam1(float& p, float& g, float& m, float& v, float coef, float omb1, float beta2,
                                      float omb2, float eps, float step_size, float bc2_sqrt) {
  g = g * coef;
  m = __fadd_rn(m, __fmul_rn(omb1, __fsub_rn(g, m)));                       // exp_avg.lerp_(grad, 1-beta1)
  v = __fadd_rn(__fmul_rn(v, beta2), __fmul_rn(__fmul_rn(omb2, g), g));     // mul_(beta2).addcmul_(g,g,1-beta2)
  const float denom = __fadd_rn(__fdiv_rn(sqrtf(v), bc2_sqrt), eps);       // (sqrt/bc2_sqrt).add_(eps)
  p = __fadd_rn(p, __fdiv_rn(__fmul_rn(-step_size, m), denom));            // addcdiv_(m, denom, -step_size)
}

__global__ __launch_bounds__(256) void clip_adam_kernel(float* __restrict__ p, float* __restrict__ g,
                                                        float* __restrict__ m, float* __restrict__ v, long n,
                                                        const double* sumsq, float max_norm, float omb1, float beta2,
                                                        float omb2, float eps, float step_size, float bc2_sqrt,
                                                        float* norm_out) {
  const float coef = clip_coef(sumsq, max_norm, norm_out);
  const long n4 = n >> 2;
  float4* p4 = reinterpret_cast<float4*>(p);
  float4* g4 = reinterpret_cast<float4*>(g);
  float4* m4 = reinterpret_cast<float4*>(m);
  float4* v4 = reinterpret_cast<float4*>(v);
  for (long i = blockIdx.x * 256L + threadIdx.x; i < n4; i += gridDim.x * 256L) {
    float4 pv = p4[i], gv = g4[i], mv = m4[i], vv = v4[i];
    adam1(pv.x, gv.x, mv.x, vv.x, coef, omb1, beta2, omb2, eps, step_size, bc2_sqrt);
    adam1(pv.y, gv.y, mv.y, vv.y, coef, omb1, beta2, omb2, eps, step_size, bc2_sqrt);
    adam1(pv.z, gv.z, mv.z, vv.z, coef, omb1, beta2, omb2, eps, step_size, bc2_sqrt);
    adam1(pv.w, gv.w, mv.w, vv.w, coef, omb1, beta2, omb2, eps, step_size, bc2_sqrt);
    p4[i] = pv; g4[i] = gv; m4[i] = mv; v4[i] = vv;
  }
  for (long i = (n4 << 2) + blockIdx.x * 256L + threadIdx.x; i < n; i += gridDim.x * 256L)
    adam1(p[i], g[i], m[i], v[i], coef, omb1, beta2, omb2, eps, step_size, bc2_sqrt);
}

// ---- the other torch.optim rules: ONE grid-stride body (float4 groups + scalar tail), one element functor per rule.
// Each functor follows the op order of torch/optim/<name>.py:_single_tensor_<name> (what the reference runs on CPU
// tensors) with correctly rounded fp32 ops.  It sees the already clipped gradient by value: the arena gradient is
// written back clipped and otherwise untouched.  a / b are the rule's state arrays (NS of them are read and written).
struct SgdRule {            // momentum 0: param.add_(grad, alpha=-lr)
  float neg_lr;
  __device__ void operator()(float& p, float g, float&, float&) const { p = __fadd_rn(p, __fmul_rn(neg_lr, g)); }
};

struct AdagradRule {        // a = sum
  float neg_clr, eps;
  __device__ void operator()(float& p, float g, float& a, float&) const {
    a = __fadd_rn(a, __fmul_rn(g, g));                                    // addcmul_(g, g, value=1)
    const float std = __fadd_rn(__fsqrt_rn(a), eps);                       // sqrt().add_(eps)
    p = __fadd_rn(p, __fdiv_rn(__fmul_rn(neg_clr, g), std));              // addcdiv_(g, std, value=-clr)
  }
};

struct AdadeltaRule {       // a = square_avg, b = acc_delta
  float neg_lr, rho, omr, eps;
  __device__ void operator()(float& p, float g, float& a, float& b) const {
    a = __fadd_rn(__fmul_rn(a, rho), __fmul_rn(__fmul_rn(omr, g), g));    // mul_(rho).addcmul_(g, g, 1-rho)
    const float std = __fsqrt_rn(__fadd_rn(a, eps));                       // add(eps).sqrt_()
    float d = __fsqrt_rn(__fadd_rn(b, eps));
    d = __fmul_rn(__fdiv_rn(d, std), g);                                   // div_(std).mul_(g)
    b = __fadd_rn(__fmul_rn(b, rho), __fmul_rn(__fmul_rn(omr, d), d));    // mul_(rho).addcmul_(d, d, 1-rho)
    p = __fadd_rn(p, __fmul_rn(neg_lr, d));                                // add_(delta, alpha=-lr)
  }
};

struct RpropRule {          // a = prev, b = step_size
  float etaminus, etaplus, ss_min, ss_max;
  __device__ void operator()(float& p, float g, float& a, float& b) const {
    const float s = __fmul_rn(g, a);                                       // grad.mul(prev).sign() -> etaplus/etaminus/1
    const float f = s > 0.f ? etaplus : (s < 0.f ? etaminus : 1.f);
    b = fminf(fmaxf(__fmul_rn(b, f), ss_min), ss_max);                     // step_size.mul_(sign).clamp_(min, max)
    const float gm = f == etaminus ? 0.f : g;                              // the masked CLONE of grad
    const float sg = gm > 0.f ? 1.f : (gm < 0.f ? -1.f : 0.f);
    p = __fadd_rn(p, __fmul_rn(-sg, b));                                   // addcmul_(grad.sign(), step_size, value=-1)
    a = gm;                                                                // prev.copy_(grad)
  }
};

struct AdamRule {           // a = exp_avg, b = exp_avg_sq (a2c_clip_adam keeps its own kernel; this is adam1 as a functor)
  float omb1, beta2, omb2, eps, step_size, bc2_sqrt;
  __device__ void operator()(float& p, float g, float& a, float& b) const {
    adam1(p, g, a, b, 1.0f, omb1, beta2, omb2, eps, step_size, bc2_sqrt);
  }
};

struct AdamWRule {          // a = exp_avg, b = exp_avg_sq: param.mul_(1 - lr*wd), then Adam's step
  float decay, omb1, beta2, omb2, eps, step_size, bc2_sqrt;
  __device__ void operator()(float& p, float g, float& a, float& b) const {
    p = __fmul_rn(p, decay);
    adam1(p, g, a, b, 1.0f, omb1, beta2, omb2, eps, step_size, bc2_sqrt);
  }
};

struct AdamaxRule {         // a = exp_avg, b = exp_inf
  float omb1, beta2, eps, neg_clr;
  __device__ void operator()(float& p, float g, float& a, float& b) const {
    a = __fadd_rn(a, __fmul_rn(omb1, __fsub_rn(g, a)));                   // lerp_(grad, 1-beta1)
    b = fmaxf(__fmul_rn(b, beta2), __fadd_rn(fabsf(g), eps));              // maximum(exp_inf.mul_(beta2), |g|.add_(eps))
    p = __fadd_rn(p, __fdiv_rn(__fmul_rn(neg_clr, a), b));                // addcdiv_(exp_avg, exp_inf, value=-clr)
  }
};

struct NAdamRule {          // a = exp_avg, b = exp_avg_sq
  float omb1, beta2, omb2, eps, bc2, c_grad, c_avg;
  __device__ void operator()(float& p, float g, float& a, float& b) const {
    a = __fadd_rn(a, __fmul_rn(omb1, __fsub_rn(g, a)));                   // lerp_(grad, 1-beta1)
    b = __fadd_rn(__fmul_rn(b, beta2), __fmul_rn(__fmul_rn(omb2, g), g)); // mul_(beta2).addcmul_(g, g, 1-beta2)
    const float denom = __fadd_rn(__fsqrt_rn(__fdiv_rn(b, bc2)), eps);    // div(bc2).sqrt().add_(eps)
    p = __fadd_rn(p, __fdiv_rn(__fmul_rn(c_grad, g), denom));             // addcdiv_(grad, denom, -lr(1-mu)/(1-mu_prod))
    p = __fadd_rn(p, __fdiv_rn(__fmul_rn(c_avg, a), denom));              // addcdiv_(exp_avg, denom, ...)
  }
};

struct RAdamRule {          // a = exp_avg, b = exp_avg_sq
  float omb1, beta2, omb2, eps, bc1, lr, bc2_sqrt, rect;
  int rectify;              // rho_t > 5
  __device__ void operator()(float& p, float g, float& a, float& b) const {
    a = __fadd_rn(a, __fmul_rn(omb1, __fsub_rn(g, a)));
    b = __fadd_rn(__fmul_rn(b, beta2), __fmul_rn(__fmul_rn(omb2, g), g));
    float u = __fmul_rn(__fdiv_rn(a, bc1), lr);                            // exp_avg / bc1 * lr
    if (rectify) {
      // bc2**0.5 / (sqrt(v) + eps) is a scalar over a tensor: torch evaluates it as reciprocal(t) * scalar
      const float adaptive = __fmul_rn(__frcp_rn(__fadd_rn(__fsqrt_rn(b), eps)), bc2_sqrt);
      u = __fmul_rn(__fmul_rn(u, adaptive), rect);
    }
    p = __fsub_rn(p, u);                                                   // add_(..., alpha=-1)
  }
};

struct AsgdRule {           // a = ax; eta / mu are the values the PREVIOUS step stored
  float decay, neg_eta, mu;
  int mu_is_one;
  __device__ void operator()(float& p, float g, float& a, float&) const {
    p = __fmul_rn(p, decay);                                               // mul_(1 - lambd*eta)
    p = __fadd_rn(p, __fmul_rn(neg_eta, g));                               // add_(grad, alpha=-eta)
    a = mu_is_one ? p : __fadd_rn(a, __fmul_rn(__fsub_rn(p, a), mu));      // copy_(p) | add_(p.sub(ax).mul_(mu))
  }
};

template <int NS, class Rule>
__device__ __forceinline__ void clip_step_body(float* __restrict__ p, float* __restrict__ g, float* __restrict__ sa,
                                               float* __restrict__ sb, long n, float coef, const Rule& rule) {
  const long n4 = n >> 2;
  float4* p4 = reinterpret_cast<float4*>(p);
  float4* g4 = reinterpret_cast<float4*>(g);
  float4* a4 = reinterpret_cast<float4*>(sa);
  float4* b4 = reinterpret_cast<float4*>(sb);
  for (long i = blockIdx.x * 256L + threadIdx.x; i < n4; i += gridDim.x * 256L) {
    float4 pv = p4[i], gv = g4[i];
    float4 av = make_float4(0.f, 0.f, 0.f, 0.f), bv = av;
    if (NS > 0) av = a4[i];
    if (NS > 1) bv = b4[i];
    gv.x = __fmul_rn(gv.x, coef); gv.y = __fmul_rn(gv.y, coef);
    gv.z = __fmul_rn(gv.z, coef); gv.w = __fmul_rn(gv.w, coef);
    rule(pv.x, gv.x, av.x, bv.x);
    rule(pv.y, gv.y, av.y, bv.y);
    rule(pv.z, gv.z, av.z, bv.z);
    rule(pv.w, gv.w, av.w, bv.w);
    p4[i] = pv; g4[i] = gv;
    if (NS > 0) a4[i] = av;
    if (NS > 1) b4[i] = bv;
  }
  for (long i = (n4 << 2) + blockIdx.x * 256L + threadIdx.x; i < n; i += gridDim.x * 256L) {
    float pv = p[i], gv = __fmul_rn(g[i], coef), av = 0.f, bv = 0.f;
    if (NS > 0) av = sa[i];
    if (NS > 1) bv = sb[i];
    rule(pv, gv, av, bv);
    p[i] = pv; g[i] = gv;
    if (NS > 0) sa[i] = av;
    if (NS > 1) sb[i] = bv;
  }
}

template <int NS, class Rule>
__global__ __launch_bounds__(256) void clip_step_kernel(float* __restrict__ p, float* __restrict__ g,
                                                        float* __restrict__ sa, float* __restrict__ sb, long n,
                                                        const double* sumsq, float max_norm, Rule rule,
                                                        float* norm_out) {
  clip_step_body<NS>(p, g, sa, sb, n, clip_coef(sumsq, max_norm, norm_out), rule);
}

// a2c_clip_adam's validation contract: A2C_ERR_ARG on a NULL or non-16-B-aligned array (NS state arrays), n == 0 a no-op
template <int NS>
int clip_step_args_bad(const float* p, const float* g, const float* sa, const float* sb, int64_t n, const double* sumsq) {
  if (n < 0 || !sumsq) return 1;
  if (n > 0 && (!p || !g || (NS > 0 && !sa) || (NS > 1 && !sb))) return 1;
  return (int)(((uintptr_t)p | (uintptr_t)g | (NS > 0 ? (uintptr_t)sa : 0) | (NS > 1 ? (uintptr_t)sb : 0)) % 16 != 0);
}

template <int NS, class Rule>
int clip_step_launch(float* p, float* g, float* sa, float* sb, int64_t n, const double* sumsq, double max_norm,
                     const Rule& rule, float* norm_out, a2c_stream_t stream) {
  hipLaunchKernelGGL((clip_step_kernel<NS, Rule>), dim3(a2c_grid_1d((n + 3) / 4, 256)), dim3(256), 0, a2c_s(stream),
                     p, g, sa, sb, (long)n, sumsq, (float)max_norm, rule, norm_out);
  A2C_CHECK_LAUNCH();
  return A2C_OK;
}
}  // namespace

namespace {
__global__ void pack_scalars_kernel(const double* __restrict__ loss_sums, const float* __restrict__ norm,
                                    const int* __restrict__ err, double* __restrict__ out) {
  if (threadIdx.x == 0) {
    out[0] = loss_sums[0]; out[1] = loss_sums[1]; out[2] = loss_sums[2];
    out[3] = (double)norm[0];
    out[4] = err ? (double)err[0] : 0.0;
  }
}
}  // namespace

extern "C" {
int a2c_pack_update_scalars(const double* loss_sums, const float* grad_norm, const int* err, double* out5,
                            a2c_stream_t stream) {
  if (!loss_sums || !grad_norm || !out5) return A2C_ERR_ARG;
  hipLaunchKernelGGL(pack_scalars_kernel, dim3(1), dim3(64), 0, a2c_s(stream), loss_sums, grad_norm, err, out5);
  A2C_CHECK_LAUNCH();
  return A2C_OK;
}

int a2c_gradnorm_sq(const float* grads, int64_t n, double* sumsq, double* scratch, a2c_stream_t stream) {
  if (n < 0 || !sumsq || !scratch || (n > 0 && !grads) || ((uintptr_t)grads % 16)) return A2C_ERR_ARG;
  if (n == 0) {
    a2c_zero_async(sumsq, sizeof(double), a2c_s(stream));
    return A2C_OK;
  }
  hipLaunchKernelGGL(sumsq_kernel, dim3(a2c_grid_1d((n + 3) / 4, 256, A2C_REDUCE_MAX_BLOCKS)), dim3(256), 0, a2c_s(stream), grads,
                     (long)n, sumsq, scratch);
  A2C_CHECK_LAUNCH();
  return A2C_OK;
}

int a2c_clip_rmsprop(float* params, float* grads, float* square_avg, int64_t n, const double* sumsq, double max_norm,
                     double lr, double alpha, double eps, float* norm_out, a2c_stream_t stream) {
  if (n < 0 || !sumsq || (n > 0 && (!params || !grads || !square_avg))) return A2C_ERR_ARG;
  if (((uintptr_t)params | (uintptr_t)grads | (uintptr_t)square_avg) % 16) return A2C_ERR_ARG;
  if (n == 0) return A2C_OK;
  const float oma = (float)(1.0 - alpha);
  hipLaunchKernelGGL(clip_rmsprop_kernel, dim3(a2c_grid_1d((n + 3) / 4, 256)), dim3(256), 0, a2c_s(stream), params,
                     grads, square_avg, (long)n, sumsq, (float)max_norm, (float)lr, (float)alpha, oma, (float)eps,
                     norm_out);
  A2C_CHECK_LAUNCH();
  return A2C_OK;
}

int a2c_clip_adam(float* params, float* grads, float* exp_avg, float* exp_avg_sq, int64_t n, const double* sumsq,
                  double max_norm, double lr, double beta1, double beta2, double eps, int64_t step, float* norm_out,
                  a2c_stream_t stream) {
  if (n < 0 || step < 1 || !sumsq || (n > 0 && (!params || !grads || !exp_avg || !exp_avg_sq))) return A2C_ERR_ARG;
  if (((uintptr_t)params | (uintptr_t)grads | (uintptr_t)exp_avg | (uintptr_t)exp_avg_sq) % 16) return A2C_ERR_ARG;
  if (n == 0) return A2C_OK;
  // torch/optim/adam.py (_single_tensor_adam): python-double scalars, rounded when applied
  const double bc1 = 1.0 - pow(beta1, (double)step);
  const double bc2 = 1.0 - pow(beta2, (double)step);
  const float step_size = (float)(lr / bc1);
  const float bc2_sqrt = (float)sqrt(bc2);
  hipLaunchKernelGGL(clip_adam_kernel, dim3(a2c_grid_1d((n + 3) / 4, 256)), dim3(256), 0, a2c_s(stream), params,
                     grads, exp_avg, exp_avg_sq, (long)n, sumsq, (float)max_norm, (float)(1.0 - beta1), (float)beta2,
                     (float)(1.0 - beta2), (float)eps, step_size, bc2_sqrt, norm_out);
  A2C_CHECK_LAUNCH();
  return A2C_OK;
}
}

// ---- the other torch.optim optimisers (torch defaults apart from the arguments).  Step-dependent scalars are computed
// here in double from the host arguments and rounded to fp32 where torch rounds them (python floats -> fp32 scalars).
extern "C" {
int a2c_clip_sgd(float* params, float* grads, int64_t n, const double* sumsq, double max_norm, double lr,
                 float* norm_out, a2c_stream_t stream) {
  if (clip_step_args_bad<0>(params, grads, nullptr, nullptr, n, sumsq)) return A2C_ERR_ARG;
  if (n == 0) return A2C_OK;
  return clip_step_launch<0>(params, grads, nullptr, nullptr, n, sumsq, max_norm, SgdRule{(float)-lr}, norm_out, stream);
}

int a2c_clip_adagrad(float* params, float* grads, float* sum, int64_t n, const double* sumsq, double max_norm,
                     double lr, double lr_decay, double eps, int64_t step, float* norm_out, a2c_stream_t stream) {
  if (step < 1 || clip_step_args_bad<1>(params, grads, sum, nullptr, n, sumsq)) return A2C_ERR_ARG;
  if (n == 0) return A2C_OK;
  const double clr = lr / (1.0 + (double)(step - 1) * lr_decay);
  return clip_step_launch<1>(params, grads, sum, nullptr, n, sumsq, max_norm, AdagradRule{(float)-clr, (float)eps},
                             norm_out, stream);
}

int a2c_clip_adadelta(float* params, float* grads, float* square_avg, float* acc_delta, int64_t n, const double* sumsq,
                      double max_norm, double lr, double rho, double eps, float* norm_out, a2c_stream_t stream) {
  if (clip_step_args_bad<2>(params, grads, square_avg, acc_delta, n, sumsq)) return A2C_ERR_ARG;
  if (n == 0) return A2C_OK;
  const AdadeltaRule r{(float)-lr, (float)rho, (float)(1.0 - rho), (float)eps};
  return clip_step_launch<2>(params, grads, square_avg, acc_delta, n, sumsq, max_norm, r, norm_out, stream);
}

int a2c_clip_rprop(float* params, float* grads, float* prev, float* step_size, int64_t n, const double* sumsq,
                   double max_norm, double etaminus, double etaplus, double step_size_min, double step_size_max,
                   float* norm_out, a2c_stream_t stream) {
  if (clip_step_args_bad<2>(params, grads, prev, step_size, n, sumsq)) return A2C_ERR_ARG;
  if (n == 0) return A2C_OK;
  const RpropRule r{(float)etaminus, (float)etaplus, (float)step_size_min, (float)step_size_max};
  return clip_step_launch<2>(params, grads, prev, step_size, n, sumsq, max_norm, r, norm_out, stream);
}

int a2c_clip_adamw(float* params, float* grads, float* exp_avg, float* exp_avg_sq, int64_t n, const double* sumsq,
                   double max_norm, double lr, double beta1, double beta2, double eps, double weight_decay,
                   int64_t step, float* norm_out, a2c_stream_t stream) {
  if (step < 1 || clip_step_args_bad<2>(params, grads, exp_avg, exp_avg_sq, n, sumsq)) return A2C_ERR_ARG;
  if (n == 0) return A2C_OK;
  const double bc1 = 1.0 - pow(beta1, (double)step);          // as a2c_clip_adam
  const double bc2 = 1.0 - pow(beta2, (double)step);
  const AdamWRule r{(float)(1.0 - lr * weight_decay), (float)(1.0 - beta1), (float)beta2, (float)(1.0 - beta2),
                    (float)eps, (float)(lr / bc1), (float)sqrt(bc2)};
  return clip_step_launch<2>(params, grads, exp_avg, exp_avg_sq, n, sumsq, max_norm, r, norm_out, stream);
}

int a2c_clip_adamax(float* params, float* grads, float* exp_avg, float* exp_inf, int64_t n, const double* sumsq,
                    double max_norm, double lr, double beta1, double beta2, double eps, int64_t step, float* norm_out,
                    a2c_stream_t stream) {
  if (step < 1 || clip_step_args_bad<2>(params, grads, exp_avg, exp_inf, n, sumsq)) return A2C_ERR_ARG;
  if (n == 0) return A2C_OK;
  const double clr = lr / (1.0 - pow(beta1, (double)step));
  const AdamaxRule r{(float)(1.0 - beta1), (float)beta2, (float)eps, (float)-clr};
  return clip_step_launch<2>(params, grads, exp_avg, exp_inf, n, sumsq, max_norm, r, norm_out, stream);
}

int a2c_clip_nadam(float* params, float* grads, float* exp_avg, float* exp_avg_sq, int64_t n, const double* sumsq,
                   double max_norm, double lr, double beta1, double beta2, double eps, double momentum_decay,
                   int64_t step, double mu_product, float* norm_out, a2c_stream_t stream) {
  if (step < 1 || clip_step_args_bad<2>(params, grads, exp_avg, exp_avg_sq, n, sumsq)) return A2C_ERR_ARG;
  if (n == 0) return A2C_OK;
  // mu_product: the fp32 state value AFTER this step's `mu_product *= mu` (the caller keeps the state)
  const double s = (double)step;
  const double mu = beta1 * (1.0 - 0.5 * pow(0.96, s * momentum_decay));
  const double mu_next = beta1 * (1.0 - 0.5 * pow(0.96, (s + 1.0) * momentum_decay));
  const double mu_product_next = mu_product * mu_next;
  const NAdamRule r{(float)(1.0 - beta1), (float)beta2, (float)(1.0 - beta2), (float)eps,
                    (float)(1.0 - pow(beta2, s)), (float)(-lr * (1.0 - mu) / (1.0 - mu_product)),
                    (float)((-lr * mu_next) / (1.0 - mu_product_next))};
  return clip_step_launch<2>(params, grads, exp_avg, exp_avg_sq, n, sumsq, max_norm, r, norm_out, stream);
}

int a2c_clip_radam(float* params, float* grads, float* exp_avg, float* exp_avg_sq, int64_t n, const double* sumsq,
                   double max_norm, double lr, double beta1, double beta2, double eps, int64_t step, float* norm_out,
                   a2c_stream_t stream) {
  if (step < 1 || clip_step_args_bad<2>(params, grads, exp_avg, exp_avg_sq, n, sumsq)) return A2C_ERR_ARG;
  if (n == 0) return A2C_OK;
  const double s = (double)step;
  const double bc1 = 1.0 - pow(beta1, s);
  const double bc2 = 1.0 - pow(beta2, s);
  const double rho_inf = 2.0 / (1.0 - beta2) - 1.0;
  const double rho_t = rho_inf - 2.0 * s * pow(beta2, s) / bc2;
  const int rectify = rho_t > 5.0;
  const double rect =
      rectify ? pow((rho_t - 4.0) * (rho_t - 2.0) * rho_inf / ((rho_inf - 4.0) * (rho_inf - 2.0) * rho_t), 0.5) : 0.0;
  const RAdamRule r{(float)(1.0 - beta1), (float)beta2, (float)(1.0 - beta2), (float)eps, (float)bc1, (float)lr,
                    (float)pow(bc2, 0.5), (float)rect, rectify};   // python's ** 0.5
  return clip_step_launch<2>(params, grads, exp_avg, exp_avg_sq, n, sumsq, max_norm, r, norm_out, stream);
}

int a2c_clip_asgd(float* params, float* grads, float* ax, int64_t n, const double* sumsq, double max_norm,
                  double lambd, double eta, double mu, float* norm_out, a2c_stream_t stream) {
  if (clip_step_args_bad<1>(params, grads, ax, nullptr, n, sumsq)) return A2C_ERR_ARG;
  if (n == 0) return A2C_OK;
  // eta, mu: the fp32 state values the previous step stored (lr and 1 before the first step)
  const AsgdRule r{(float)(1.0 - lambd * eta), (float)-eta, (float)mu, (float)mu == 1.0f};
  return clip_step_launch<1>(params, grads, ax, nullptr, n, sumsq, max_norm, r, norm_out, stream);
}
}

// ---- capturable Adam family: the step count and the step-dependent scalars live in a device block (a2c_optim_block,
// include/a2c_mi355x.h), so a hipGraph replay of [advance, step] steps like an eager run.  optim_advance_kernel is the
// scalar part of the launchers above moved onto the device: the same double formulas in the same order, rounded to fp32
// at the same places; clip_step_dev_kernel is clip_step_body with the functor filled from the block.
namespace {
static_assert(sizeof(a2c_optim_block) == A2C_OPTIM_BLOCK_BYTES, "a2c_optim_block layout");

__global__ __launch_bounds__(64) void optim_advance_kernel(int kind, a2c_optim_block* blk, double lr, double beta1,
                                                           double beta2, double eps, double weight_decay,
                                                           double momentum_decay, double lambd, double alpha,
                                                           double t0) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  a2c_optim_block b = *blk;
  b.step += 1;
  const double s = (double)b.step;
  b.lr = (float)lr;
  b.omb1 = (float)(1.0 - beta1);
  b.beta2 = (float)beta2;
  b.omb2 = (float)(1.0 - beta2);
  b.eps = (float)eps;
  switch (kind) {
    case A2C_OPTIM_ADAM:
    case A2C_OPTIM_ADAMW: {                                   // a2c_clip_adam / a2c_clip_adamw
      const double bc1 = 1.0 - pow(beta1, s);
      const double bc2 = 1.0 - pow(beta2, s);
      b.decay = (float)(1.0 - lr * weight_decay);
      b.step_size = (float)(lr / bc1);
      b.bc2_sqrt = (float)sqrt(bc2);
      break;
    }
    case A2C_OPTIM_ADAMAX: {                                  // a2c_clip_adamax
      const double clr = lr / (1.0 - pow(beta1, s));
      b.neg_clr = (float)-clr;
      break;
    }
    case A2C_OPTIM_NADAM: {                                   // optim.nadam_mu_product, then a2c_clip_nadam
      const double mu = beta1 * (1.0 - 0.5 * pow(0.96, s * momentum_decay));
      b.mu_product = (float)((double)b.mu_product * (double)(float)mu);
      const double mu_product = (double)b.mu_product;
      const double mu_next = beta1 * (1.0 - 0.5 * pow(0.96, (s + 1.0) * momentum_decay));
      const double mu_product_next = mu_product * mu_next;
      b.bc2 = (float)(1.0 - pow(beta2, s));
      b.c_grad = (float)(-lr * (1.0 - mu) / (1.0 - mu_product));
      b.c_avg = (float)((-lr * mu_next) / (1.0 - mu_product_next));
      break;
    }
    case A2C_OPTIM_RADAM: {                                   // a2c_clip_radam
      const double bc1 = 1.0 - pow(beta1, s);
      const double bc2 = 1.0 - pow(beta2, s);
      const double rho_inf = 2.0 / (1.0 - beta2) - 1.0;
      const double rho_t = rho_inf - 2.0 * s * pow(beta2, s) / bc2;
      b.rectify = rho_t > 5.0;
      const double rect = b.rectify ? pow((rho_t - 4.0) * (rho_t - 2.0) * rho_inf /
                                          ((rho_inf - 4.0) * (rho_inf - 2.0) * rho_t), 0.5) : 0.0;
      b.bc1 = (float)bc1;
      b.bc2_sqrt = (float)pow(bc2, 0.5);
      b.rect = (float)rect;
      break;
    }
    default: {                                                // A2C_OPTIM_ASGD: a2c_clip_asgd, then optim.asgd_eta_mu
      const double eta = (double)b.eta, mu = (double)b.mu;    // what the previous step stored
      b.decay = (float)(1.0 - lambd * eta);
      b.neg_eta = (float)-eta;
      b.mu_used = (float)mu;
      b.mu_is_one = (float)mu == 1.0f;
      b.eta = (float)(lr / pow(1.0 + lambd * lr * s, alpha));
      b.mu = (float)(1.0 / fmax(1.0, s - t0));
      break;
    }
  }
  *blk = b;
}

template <class Rule> __device__ __forceinline__ Rule rule_from_block(const a2c_optim_block& b);
template <> __device__ __forceinline__ AdamRule rule_from_block<AdamRule>(const a2c_optim_block& b) {
  return AdamRule{b.omb1, b.beta2, b.omb2, b.eps, b.step_size, b.bc2_sqrt};
}
template <> __device__ __forceinline__ AdamWRule rule_from_block<AdamWRule>(const a2c_optim_block& b) {
  return AdamWRule{b.decay, b.omb1, b.beta2, b.omb2, b.eps, b.step_size, b.bc2_sqrt};
}
template <> __device__ __forceinline__ AdamaxRule rule_from_block<AdamaxRule>(const a2c_optim_block& b) {
  return AdamaxRule{b.omb1, b.beta2, b.eps, b.neg_clr};
}
template <> __device__ __forceinline__ NAdamRule rule_from_block<NAdamRule>(const a2c_optim_block& b) {
  return NAdamRule{b.omb1, b.beta2, b.omb2, b.eps, b.bc2, b.c_grad, b.c_avg};
}
template <> __device__ __forceinline__ RAdamRule rule_from_block<RAdamRule>(const a2c_optim_block& b) {
  return RAdamRule{b.omb1, b.beta2, b.omb2, b.eps, b.bc1, b.lr, b.bc2_sqrt, b.rect, b.rectify};
}
template <> __device__ __forceinline__ AsgdRule rule_from_block<AsgdRule>(const a2c_optim_block& b) {
  return AsgdRule{b.decay, b.neg_eta, b.mu_used, b.mu_is_one};
}

// the block was written by an earlier launch on the stream and is only read here: every thread block sees the same step
template <int NS, class Rule>
__global__ __launch_bounds__(256) void clip_step_dev_kernel(float* __restrict__ p, float* __restrict__ g,
                                                            float* __restrict__ sa, float* __restrict__ sb, long n,
                                                            const double* sumsq, float max_norm,
                                                            const a2c_optim_block* __restrict__ blk, float* norm_out) {
  const Rule rule = rule_from_block<Rule>(*blk);
  clip_step_body<NS>(p, g, sa, sb, n, clip_coef(sumsq, max_norm, norm_out), rule);
}

template <int NS, class Rule>
int clip_step_dev_launch(float* p, float* g, float* sa, float* sb, int64_t n, const double* sumsq, double max_norm,
                         const a2c_optim_block* blk, float* norm_out, a2c_stream_t stream) {
  if (clip_step_args_bad<NS>(p, g, sa, sb, n, sumsq)) return A2C_ERR_ARG;
  if (n == 0) return A2C_OK;
  hipLaunchKernelGGL((clip_step_dev_kernel<NS, Rule>), dim3(a2c_grid_1d((n + 3) / 4, 256)), dim3(256), 0, a2c_s(stream),
                     p, g, sa, sb, (long)n, sumsq, (float)max_norm, blk, norm_out);
  A2C_CHECK_LAUNCH();
  return A2C_OK;
}

bool optim_block_bad(int kind, const void* block) {
  return kind < A2C_OPTIM_ADAM || kind > A2C_OPTIM_ASGD || !block || (uintptr_t)block % 16 != 0;
}
}  // namespace

extern "C" {
int a2c_optim_advance(int kind, void* block, double lr, double beta1, double beta2, double eps, double weight_decay,
                      double momentum_decay, double lambd, double alpha, double t0, a2c_stream_t stream) {
  if (optim_block_bad(kind, block)) return A2C_ERR_ARG;
  hipLaunchKernelGGL(optim_advance_kernel, dim3(1), dim3(64), 0, a2c_s(stream), kind, (a2c_optim_block*)block, lr,
                     beta1, beta2, eps, weight_decay, momentum_decay, lambd, alpha, t0);
  A2C_CHECK_LAUNCH();
  return A2C_OK;
}

int a2c_clip_step_dev(int kind, float* params, float* grads, float* state_a, float* state_b, int64_t n,
                      const double* sumsq, double max_norm, const void* block, float* norm_out, a2c_stream_t stream) {
  if (optim_block_bad(kind, block)) return A2C_ERR_ARG;
  const a2c_optim_block* blk = (const a2c_optim_block*)block;
  switch (kind) {
    case A2C_OPTIM_ADAM:
      return clip_step_dev_launch<2, AdamRule>(params, grads, state_a, state_b, n, sumsq, max_norm, blk, norm_out, stream);
    case A2C_OPTIM_ADAMW:
      return clip_step_dev_launch<2, AdamWRule>(params, grads, state_a, state_b, n, sumsq, max_norm, blk, norm_out, stream);
    case A2C_OPTIM_ADAMAX:
      return clip_step_dev_launch<2, AdamaxRule>(params, grads, state_a, state_b, n, sumsq, max_norm, blk, norm_out, stream);
    case A2C_OPTIM_NADAM:
      return clip_step_dev_launch<2, NAdamRule>(params, grads, state_a, state_b, n, sumsq, max_norm, blk, norm_out, stream);
    case A2C_OPTIM_RADAM:
      return clip_step_dev_launch<2, RAdamRule>(params, grads, state_a, state_b, n, sumsq, max_norm, blk, norm_out, stream);
    default:                    // A2C_OPTIM_ASGD: one state array (ax); state_b is not touched
      return clip_step_dev_launch<1, AsgdRule>(params, grads, state_a, nullptr, n, sumsq, max_norm, blk, norm_out, stream);
  }
}
}
