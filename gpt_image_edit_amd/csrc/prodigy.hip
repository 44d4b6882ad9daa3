// Prodigy (Mishchenko & Defazio, "Prodigy: An Expeditiously Adaptive Parameter-Free Learner") on fp32 masters: the second
// optimiser of the training seam (reference train_denoiser.py:595-624, `optimizer: 'prodigy'`).  The step size d is estimated
// from two sums over ALL trainable elements, so one step is two streaming passes with a scalar update between them:
//
//   fk_prodigy_begin     1 thread   bias correction, dlr = d * lr * bc, d_numerator *= beta3, running sums = 0
//   fk_prodigy_moments   per tensor m, v, s in place; sum g * (p0 - p) and sum |s_new| into the running sums     ~36 B / element
//   fk_prodigy_update_d  1 thread   d_numerator, d_denom, d_hat, d, d_max, k; the skipped flag when d_denom == 0
//   fk_prodigy_apply     per tensor p (and its bf16 copy) with the OLD dlr and the NEW d                          ~18 B / element
//
// Every scalar lives in the caller's fp64 state buffer (FK_PRODIGY_* slots of include/fk.h); nothing is read back to the host.
// Per-tensor scalar factors are formed in double from that buffer and rounded to fp32 ONCE; the element arithmetic is fp32 with
// every operation rounded on its own (tests/prodigy_ref.py emulates this order and derives the bounds from it).
//
// Decomposition of both streaming kernels: with every pointer 16-byte aligned (the bf16 ones 8-byte) thread t of the grid takes
// the 4-element groups t, t + T, t + 2T, ... (T = blocks * 256, at most PR_MAX_BLOCKS blocks) as 16-byte loads and stores, and
// the n % 4 tail elements go one per thread; an unaligned view goes one element per thread throughout.  The sums have a FIXED
// order: per thread its elements in increasing order in double, a wave shuffle tree, the block's 4 waves in order, one partial
// pair per block in ws, then ONE finishing block that adds them onto the running sums.  No floating-point atomics: two runs
// give the same bits, and calls accumulate in call order.
#include "fk_common.h"

namespace {

constexpr int PR_THREADS = 256;
constexpr int PR_MAX_BLOCKS = 2048;

// wave (shuffle) then block (LDS, fixed order) sum of two values; valid in thread 0
FK_DEV void block_sum2(double& a, double& b, double* sh) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    a += __shfl_xor(a, off);
    b += __shfl_xor(b, off);
  }
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  if (lane == 0) {
    sh[2 * wave] = a;
    sh[2 * wave + 1] = b;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    a = b = 0.0;
    for (int i = 0; i < PR_THREADS / 64; ++i) {
      a += sh[2 * i];
      b += sh[2 * i + 1];
    }
  }
}

struct MomentScalars {
  float coef, wd, b1, b2, b3, cm, cv, cs;
};

// adamw_kernel's coefficient arithmetic, then the per-tensor factors: double from the state buffer, one rounding to fp32
FK_DEV MomentScalars moment_scalars(const double* state, const double* grad_sumsq, float max_norm, float grad_scale, float b1,
                                    float b2, float b3, float wd, double d0, int safeguard) {
  MomentScalars k;
  k.coef = grad_scale;
  if (grad_sumsq) {
    const float total = __fmul_rn((float)sqrt(grad_sumsq[0]), grad_scale);
    k.coef = __fmul_rn(fminf(max_norm / (total + 1e-6f), 1.0f), grad_scale);
  }
  const double d = state[FK_PRODIGY_D], dlr = state[FK_PRODIGY_DLR];
  k.wd = wd; k.b1 = b1; k.b2 = b2; k.b3 = b3;
  k.cm = (float)(d * (1.0 - (double)b1));
  k.cv = (float)(d * d * (1.0 - (double)b2));
  k.cs = (float)((d / d0) * (safeguard ? d : dlr));
  return k;
}

// one element of step 2; returns g * (p0 - p) and |s_new| through dot / ab
FK_DEV void moment_element(const MomentScalars& k, int decouple, float graw, float p, float p0, float& m, float& v, float& s,
                           double& dot, double& ab) {
  float g = __fmul_rn(graw, k.coef);
  if (!decouple) g = __fadd_rn(g, __fmul_rn(k.wd, p));
  dot += (double)g * (double)__fsub_rn(p0, p);
  m = __fadd_rn(__fmul_rn(k.b1, m), __fmul_rn(k.cm, g));
  v = __fadd_rn(__fmul_rn(k.b2, v), __fmul_rn(__fmul_rn(k.cv, g), g));
  s = __fadd_rn(__fmul_rn(k.b3, s), __fmul_rn(k.cs, g));
  ab += (double)fabsf(s);
}

template <bool VEC>
__global__ __launch_bounds__(PR_THREADS) void prodigy_moments_kernel(const float* master, const float* p0, const void* grad,
                                                                     int g_is_bf16, float* m, float* v, float* s,
                                                                     const double* state, const double* grad_sumsq,
                                                                     float max_norm, float grad_scale, float b1, float b2,
                                                                     float b3, float wd, double d0, int decouple,
                                                                     int safeguard, int64_t n, double* ws) {
  __shared__ double sh[2 * (PR_THREADS / 64)];
  const MomentScalars k = moment_scalars(state, grad_sumsq, max_norm, grad_scale, b1, b2, b3, wd, d0, safeguard);
  double dot = 0.0, ab = 0.0;
  const int64_t tid = (int64_t)blockIdx.x * PR_THREADS + threadIdx.x, T = (int64_t)gridDim.x * PR_THREADS;
  const int64_t n4 = VEC ? n / 4 : 0;
  for (int64_t q = tid; q < n4; q += T) {
    const f32x4_t pv = ((const f32x4_t*)master)[q], p0v = ((const f32x4_t*)p0)[q];
    f32x4_t mv = ((const f32x4_t*)m)[q], vv = ((const f32x4_t*)v)[q], sv = ((const f32x4_t*)s)[q], gv;
    if (g_is_bf16) {
      const u32x2_t w = ((const u32x2_t*)grad)[q];
      gv = f32x4_t{bf_lo(w[0]), bf_hi(w[0]), bf_lo(w[1]), bf_hi(w[1])};
    } else {
      gv = ((const f32x4_t*)grad)[q];
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      float me = mv[e], ve = vv[e], se = sv[e];
      moment_element(k, decouple, gv[e], pv[e], p0v[e], me, ve, se, dot, ab);
      mv[e] = me; vv[e] = ve; sv[e] = se;
    }
    ((f32x4_t*)m)[q] = mv;
    ((f32x4_t*)v)[q] = vv;
    ((f32x4_t*)s)[q] = sv;
  }
  for (int64_t i = n4 * 4 + tid; i < n; i += T) {
    const float graw = g_is_bf16 ? bf2f(((const bf16_t*)grad)[i]) : ((const float*)grad)[i];
    float me = m[i], ve = v[i], se = s[i];
    moment_element(k, decouple, graw, master[i], p0[i], me, ve, se, dot, ab);
    m[i] = me; v[i] = ve; s[i] = se;
  }
  block_sum2(dot, ab, sh);
  if (threadIdx.x == 0) {
    ws[2 * (int64_t)blockIdx.x] = dot;
    ws[2 * (int64_t)blockIdx.x + 1] = ab;
  }
}

// state[SUM_DOT] += sum of the blocks' dot partials, state[SUM_ABS] += sum of their |s| partials -- one block, fixed order
__global__ __launch_bounds__(PR_THREADS) void prodigy_finish_kernel(const double* ws, int nblk, double* state) {
  __shared__ double sh[2 * (PR_THREADS / 64)];
  double dot = 0.0, ab = 0.0;
  for (int j = threadIdx.x; j < nblk; j += PR_THREADS) {
    dot += ws[2 * j];
    ab += ws[2 * j + 1];
  }
  block_sum2(dot, ab, sh);
  if (threadIdx.x == 0) {
    state[FK_PRODIGY_SUM_DOT] += dot;
    state[FK_PRODIGY_SUM_ABS] += ab;
  }
}

__global__ void prodigy_begin_kernel(double* state, double lr, double beta1, double beta2, double beta3, int bias_correction) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  const double k1 = state[FK_PRODIGY_K] + 1.0;
  const double bc = bias_correction ? sqrt(1.0 - pow(beta2, k1)) / (1.0 - pow(beta1, k1)) : 1.0;
  state[FK_PRODIGY_DLR] = state[FK_PRODIGY_D] * lr * bc;
  state[FK_PRODIGY_D_NUMERATOR] *= beta3;
  state[FK_PRODIGY_SUM_DOT] = 0.0;
  state[FK_PRODIGY_SUM_ABS] = 0.0;
  state[FK_PRODIGY_SKIPPED] = 0.0;
}

__global__ void prodigy_update_d_kernel(double* state, double d0, double d_coef, double growth_rate) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  double d = state[FK_PRODIGY_D];
  const double num = state[FK_PRODIGY_D_NUMERATOR] + (d / d0) * state[FK_PRODIGY_DLR] * state[FK_PRODIGY_SUM_DOT];
  const double den = state[FK_PRODIGY_SUM_ABS];
  state[FK_PRODIGY_D_NUMERATOR] = num;
  state[FK_PRODIGY_D_DENOM] = den;
  if (den == 0.0) {                      // an all-zero gradient so far: parameters, d and k stay; the moments kept their decay
    state[FK_PRODIGY_SKIPPED] = 1.0;
    return;
  }
  const double d_hat = d_coef * num / den;
  double d_max = state[FK_PRODIGY_D_MAX];
  if (d == d0) d = fmax(d, d_hat);
  d_max = fmax(d_max, d_hat);
  d = fmin(d_max, d * growth_rate);
  state[FK_PRODIGY_D_HAT] = d_hat;
  state[FK_PRODIGY_D_MAX] = d_max;
  state[FK_PRODIGY_D] = d;
  state[FK_PRODIGY_K] += 1.0;
}

struct ApplyScalars {
  float dlr, deps, wdf;
};

FK_DEV float apply_element(const ApplyScalars& k, int decouple, float p, float m, float v) {
  if (decouple) p = __fadd_rn(p, __fmul_rn(p, k.wdf));
  const float denom = __fadd_rn(__fsqrt_rn(v), k.deps);
  return __fsub_rn(p, __fmul_rn(k.dlr, __fdiv_rn(m, denom)));
}

template <bool VEC>
__global__ __launch_bounds__(PR_THREADS) void prodigy_apply_kernel(float* master, bf16_t* param_bf16, const float* m,
                                                                   const float* v, const double* state, float eps, float wd,
                                                                   int decouple, int64_t n) {
  if (state[FK_PRODIGY_SKIPPED] != 0.0) return;
  ApplyScalars k;
  const double dlr = state[FK_PRODIGY_DLR];
  k.dlr = (float)dlr;
  k.deps = (float)(state[FK_PRODIGY_D] * (double)eps);
  k.wdf = (float)(-(double)wd * dlr);
  const int64_t tid = (int64_t)blockIdx.x * PR_THREADS + threadIdx.x, T = (int64_t)gridDim.x * PR_THREADS;
  const int64_t n4 = VEC ? n / 4 : 0;
  for (int64_t q = tid; q < n4; q += T) {
    f32x4_t pv = ((const f32x4_t*)master)[q];
    const f32x4_t mv = ((const f32x4_t*)m)[q], vv = ((const f32x4_t*)v)[q];
#pragma unroll
    for (int e = 0; e < 4; ++e) pv[e] = apply_element(k, decouple, pv[e], mv[e], vv[e]);
    ((f32x4_t*)master)[q] = pv;
    if (param_bf16) ((u32x2_t*)param_bf16)[q] = u32x2_t{pack_bf2(pv[0], pv[1]), pack_bf2(pv[2], pv[3])};
  }
  for (int64_t i = n4 * 4 + tid; i < n; i += T) {
    const float p = apply_element(k, decouple, master[i], m[i], v[i]);
    master[i] = p;
    if (param_bf16) param_bf16[i] = f2bf(p);
  }
}

int grid_of(int64_t items) {
  const int64_t g = (items + PR_THREADS - 1) / PR_THREADS;
  return (int)(g < 1 ? 1 : (g < PR_MAX_BLOCKS ? g : PR_MAX_BLOCKS));
}
bool al(const void* p, uintptr_t bytes) { return (uintptr_t)p % bytes == 0; }
bool beta_ok(double b) { return b >= 0.0 && b < 1.0; }

}  // namespace

extern "C" int64_t fk_prodigy_ws_doubles(void) { return 2 * PR_MAX_BLOCKS; }

extern "C" int fk_prodigy_begin(double* state, double lr, double beta1, double beta2, double beta3, int32_t use_bias_correction,
                                fk_stream_t stream) {
  FK_CHECK_ARG(state, "fk_prodigy_begin: NULL state buffer");
  FK_CHECK_ARG(beta_ok(beta1) && beta_ok(beta2) && beta_ok(beta3), "fk_prodigy_begin: betas must lie in [0, 1)");
  hipLaunchKernelGGL(prodigy_begin_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, state, lr, beta1, beta2, beta3,
                     (int)use_bias_correction);
  FK_CHECK_LAUNCH("fk_prodigy_begin");
  return FK_OK;
}

extern "C" int fk_prodigy_moments(const float* master, const float* p0, const void* grad, int32_t grad_is_bf16, float* m, float* v,
                                  float* s, double* state, const double* grad_sumsq, float max_grad_norm, float grad_scale,
                                  float beta1, float beta2, float beta3, float weight_decay, double d0, int32_t decouple,
                                  int32_t safeguard_warmup, int64_t n, double* ws, fk_stream_t stream) {
  FK_CHECK_ARG(master && p0 && grad && m && v && s && state && ws, "fk_prodigy_moments: NULL pointer");
  FK_CHECK_ARG(n > 0, "fk_prodigy_moments: n = %lld", (long long)n);
  FK_CHECK_ARG(grad_scale > 0.f, "fk_prodigy_moments: grad_scale must be positive");
  FK_CHECK_ARG(d0 > 0.0, "fk_prodigy_moments: d0 must be positive");
  FK_CHECK_ARG(beta_ok(beta1) && beta_ok(beta2) && beta_ok(beta3), "fk_prodigy_moments: betas must lie in [0, 1)");
  const bool vec = al(master, 16) && al(p0, 16) && al(m, 16) && al(v, 16) && al(s, 16) && al(grad, grad_is_bf16 ? 8 : 16);
  const int nblk = grid_of(vec ? (n + 3) / 4 : n);
  const hipStream_t st = (hipStream_t)stream;
#define FK_PR_MOMENTS(V)                                                                                                    \
  hipLaunchKernelGGL(prodigy_moments_kernel<V>, dim3(nblk), dim3(PR_THREADS), 0, st, master, p0, grad, (int)grad_is_bf16, m, \
                     v, s, (const double*)state, grad_sumsq, max_grad_norm, grad_scale, beta1, beta2, beta3, weight_decay,  \
                     d0, (int)decouple, (int)safeguard_warmup, n, ws)
  if (vec) FK_PR_MOMENTS(true);
  else FK_PR_MOMENTS(false);
#undef FK_PR_MOMENTS
  FK_CHECK_LAUNCH("fk_prodigy_moments");
  hipLaunchKernelGGL(prodigy_finish_kernel, dim3(1), dim3(PR_THREADS), 0, st, (const double*)ws, nblk, state);
  FK_CHECK_LAUNCH("fk_prodigy_moments (finish)");
  return FK_OK;
}

extern "C" int fk_prodigy_update_d(double* state, double d0, double d_coef, double growth_rate, fk_stream_t stream) {
  FK_CHECK_ARG(state, "fk_prodigy_update_d: NULL state buffer");
  FK_CHECK_ARG(d0 > 0.0, "fk_prodigy_update_d: d0 must be positive");
  hipLaunchKernelGGL(prodigy_update_d_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, state, d0, d_coef, growth_rate);
  FK_CHECK_LAUNCH("fk_prodigy_update_d");
  return FK_OK;
}

extern "C" int fk_prodigy_apply(float* master, void* param_bf16, const float* m, const float* v, const double* state, float eps,
                                float weight_decay, int32_t decouple, int64_t n, fk_stream_t stream) {
  FK_CHECK_ARG(master && m && v && state, "fk_prodigy_apply: NULL pointer");
  FK_CHECK_ARG(n > 0, "fk_prodigy_apply: n = %lld", (long long)n);
  const bool vec = al(master, 16) && al(m, 16) && al(v, 16) && (!param_bf16 || al(param_bf16, 8));
  const int nblk = grid_of(vec ? (n + 3) / 4 : n);
  if (vec)
    hipLaunchKernelGGL(prodigy_apply_kernel<true>, dim3(nblk), dim3(PR_THREADS), 0, (hipStream_t)stream, master,
                       (bf16_t*)param_bf16, m, v, state, eps, weight_decay, (int)decouple, n);
  else
    hipLaunchKernelGGL(prodigy_apply_kernel<false>, dim3(nblk), dim3(PR_THREADS), 0, (hipStream_t)stream, master,
                       (bf16_t*)param_bf16, m, v, state, eps, weight_decay, (int)decouple, n);
  FK_CHECK_LAUNCH("fk_prodigy_apply");
  return FK_OK;
}
