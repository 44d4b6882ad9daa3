// The denoise loop's update of the latent state, every rule and every state type: one HBM-bound pass over the target rows of the
// token buffer, 8 elements (one 16-byte vector) per thread, one launch per step.
//   Euler (scheduler.step on bf16 tensors):  x = bf16(x + bf16(bf16(dsigma) * v))
//   AB2 (scheduler.py: FlowMatchMultistepScheduler, a non-uniform sigma grid):
//     s = x + c_v * v  [+ c_h * h]      fp32, each product and each sum rounded once (no fma: torch restates it op by op)
//     x = bf16(s)                        the one rounding of the update
//     hist <- v                          the same pass: the next step's history
//     The coefficients stay fp32: rounded to bf16 (2^-8 relative) the rule would no longer be second order.
//   Float32 state: either rule with s kept unrounded in `state` from step to step.
// With a mask, the keep-region blend of a masked edit on the rule's value; scale_noise makes the start tokens of an edit that
// begins inside the schedule from the same keep value.  The pieces the kernels share are in step_common.h.
#include <type_traits>

#include "fk_common.h"
#include "step_common.h"

namespace {

template <bool MASK>
__global__ __launch_bounds__(256) void euler_kernel(bf16_t* x, int64_t x_bs, const bf16_t* v, int64_t v_bs, keep_args keep,
                                                    int S_tgt, int C, float dsig_bf, float sb, float omsb) {
  const int b = blockIdx.y;
  const int64_t cvec = C / 8, nvec = (int64_t)S_tgt * cvec;
  bf16_t* xb = x + (int64_t)b * x_bs;
  const bf16_t* vb = v + (int64_t)b * v_bs;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < nvec; i += (int64_t)gridDim.x * 256) {
    float s[8], p[8];
    widen8(s, *(const u32x4_t*)(xb + i * 8));
    widen8(p, *(const u32x4_t*)(vb + i * 8));
#pragma unroll
    for (int j = 0; j < 8; ++j) s[j] += round_bf(dsig_bf * p[j]);
    *(u32x4_t*)(xb + i * 8) = MASK ? blend8_bf16(s, keep, b, i, cvec, sb, omsb) : pack8(s);
  }
}

__global__ __launch_bounds__(256) void scale_noise_kernel(const bf16_t* x0, int64_t x0_bs, const bf16_t* noise,
                                                          int64_t n_bs, bf16_t* out, int64_t o_bs, int S_tgt, int C,
                                                          float sb, float omsb) {
  const int b = blockIdx.y;
  const int64_t nvec = (int64_t)S_tgt * C / 8;
  const bf16_t* x0b = x0 + (int64_t)b * x0_bs;
  const bf16_t* nb = noise + (int64_t)b * n_bs;
  bf16_t* ob = out + (int64_t)b * o_bs;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < nvec; i += (int64_t)gridDim.x * 256) {
    float z[8], n[8];
    widen8(z, *(const u32x4_t*)(x0b + i * 8));
    widen8(n, *(const u32x4_t*)(nb + i * 8));
#pragma unroll
    for (int j = 0; j < 8; ++j) z[j] = keep_f(sb, omsb, n[j], z[j]);
    *(u32x4_t*)(ob + i * 8) = pack8(z);
  }
}

template <bool HIST, bool MASK>
__global__ __launch_bounds__(256) void ab2_kernel(bf16_t* x, int64_t x_bs, const bf16_t* v, int64_t v_bs, bf16_t* hist,
                                                  int64_t h_bs, keep_args keep, int S_tgt, int C, float c_v, float c_h,
                                                  float sb, float omsb) {
  const int b = blockIdx.y;
  const int64_t cvec = C / 8, nvec = (int64_t)S_tgt * cvec;
  bf16_t* xb = x + (int64_t)b * x_bs;
  const bf16_t* vb = v + (int64_t)b * v_bs;
  bf16_t* hb = hist + (int64_t)b * h_bs;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < nvec; i += (int64_t)gridDim.x * 256) {
    const u32x4_t vw = *(const u32x4_t*)(vb + i * 8);
    float s[8];
    widen8(s, *(const u32x4_t*)(xb + i * 8));
    axpy8_rn(s, c_v, vw);
    if (HIST) axpy8_rn(s, c_h, *(const u32x4_t*)(hb + i * 8));   // this thread's h, read before the store below replaces it
    *(u32x4_t*)(hb + i * 8) = vw;
    *(u32x4_t*)(xb + i * 8) = MASK ? blend8_bf16(s, keep, b, i, cvec, sb, omsb) : pack8(s);
  }
}

// ---- host side: the checks the entries share.  FK_CHECK_ARG returns from the function it stands in, so these return the code
// and an entry does `if (int e = ...) return e;` at the place in its own ladder where the check has always stood.
bool sizes_ok(int32_t B, int32_t S_tgt, int32_t C) { return B > 0 && S_tgt > 0 && C > 0 && C % 8 == 0; }

// an entry's bf16 rows -- x, v and hist, which may be NULL (scale_noise: x0, noise, out): 16-byte pointers, strides in whole vectors
int check_rows(const char* name, const void* a, int64_t a_bs, const void* b, int64_t b_bs, const void* c, int64_t c_bs) {
  FK_CHECK_ARG(a_bs % 8 == 0 && b_bs % 8 == 0 && (!c || c_bs % 8 == 0) && ((uintptr_t)a % 16 == 0) &&
                   ((uintptr_t)b % 16 == 0) && ((uintptr_t)c % 16 == 0), "%s: alignment", name);
  return FK_OK;
}

// the operands of a masked step (mask != NULL)
int check_keep(const char* name, const keep_args& k) {
  FK_CHECK_ARG(k.x0 && k.noise, "%s: a mask needs x0 and noise", name);
  FK_CHECK_ARG(k.x0_bs % 8 == 0 && k.n_bs % 8 == 0 && ((uintptr_t)k.x0 % 16 == 0) && ((uintptr_t)k.noise % 16 == 0),
               "%s: alignment of x0 / noise", name);
  FK_CHECK_ARG(k.m_bs % 4 == 0 && ((uintptr_t)k.mask % 8 == 0), "%s: alignment of the mask", name);
  return FK_OK;
}

keep_args keep_of(const void* x0, int64_t x0_bs, const void* noise, int64_t n_bs, const void* mask, int64_t m_bs) {
  return keep_args{(const bf16_t*)x0, x0_bs, (const bf16_t*)noise, n_bs, (const bf16_t*)mask, m_bs};
}

// f(std::bool_constant<HIST>, std::bool_constant<MASK>): the four instantiations of a <HIST, MASK> kernel, chosen once
template <class F>
void with_hist_mask(bool hist, bool mask, F&& f) {
  if (hist && mask) f(std::true_type{}, std::true_type{});
  else if (hist) f(std::true_type{}, std::false_type{});
  else if (mask) f(std::false_type{}, std::true_type{});
  else f(std::false_type{}, std::false_type{});
}

// the unmasked Euler launch: fk_euler_step_bf16, and fk_euler_inpaint_step_bf16 without a mask (a mask of ones)
int euler_launch(const char* name, void* x, int64_t x_bs, const void* v, int64_t v_bs, int32_t B, int32_t S_tgt, int32_t C,
                 float dsigma, fk_stream_t stream) {
  const int64_t nvec = (int64_t)S_tgt * C / 8;
  // host_round_bf: the reference multiplies a 0-dim fp32 tensor into a bf16 tensor, and the scalar is first cast to bf16
  hipLaunchKernelGGL(euler_kernel<false>, dim3(ew_grid(nvec), B), dim3(256), 0, (hipStream_t)stream, (bf16_t*)x, x_bs,
                     (const bf16_t*)v, v_bs, keep_args{}, S_tgt, C, host_round_bf(dsigma), 0.0f, 0.0f);
  FK_CHECK_LAUNCH(name);
  return FK_OK;
}

}  // namespace

extern "C" int fk_euler_step_bf16(void* x, int64_t x_batch_stride, const void* v, int64_t v_batch_stride,
                                  int32_t B, int32_t S_tgt, int32_t C, float dsigma, fk_stream_t stream) {
  FK_CHECK_ARG(x && v && sizes_ok(B, S_tgt, C), "fk_euler_step_bf16: bad sizes");
  if (int e = check_rows("fk_euler_step_bf16", x, x_batch_stride, v, v_batch_stride, nullptr, 0)) return e;
  return euler_launch("fk_euler_step_bf16", x, x_batch_stride, v, v_batch_stride, B, S_tgt, C, dsigma, stream);
}

extern "C" int fk_euler_inpaint_step_bf16(void* x, int64_t x_batch_stride, const void* v, int64_t v_batch_stride,
                                          const void* x0, int64_t x0_batch_stride, const void* noise,
                                          int64_t noise_batch_stride, const void* mask, int64_t mask_batch_stride,
                                          int32_t B, int32_t S_tgt, int32_t C, float dsigma, float sigma_next,
                                          fk_stream_t stream) {
  const char* name = "fk_euler_inpaint_step_bf16";
  FK_CHECK_ARG(x && v && sizes_ok(B, S_tgt, C), "fk_euler_inpaint_step_bf16: bad sizes");
  if (int e = check_rows(name, x, x_batch_stride, v, v_batch_stride, nullptr, 0)) return e;
  // a mask of ones selects the Euler update everywhere: x0 and noise are not looked at (and may be NULL)
  if (!mask) return euler_launch(name, x, x_batch_stride, v, v_batch_stride, B, S_tgt, C, dsigma, stream);
  const keep_args keep = keep_of(x0, x0_batch_stride, noise, noise_batch_stride, mask, mask_batch_stride);
  if (int e = check_keep(name, keep)) return e;
  const float sb = host_round_bf(sigma_next), omsb = host_round_bf(1.0f - sb);
  const int64_t nvec = (int64_t)S_tgt * C / 8;
  hipLaunchKernelGGL(euler_kernel<true>, dim3(ew_grid(nvec), B), dim3(256), 0, (hipStream_t)stream, (bf16_t*)x,
                     x_batch_stride, (const bf16_t*)v, v_batch_stride, keep, S_tgt, C, host_round_bf(dsigma), sb, omsb);
  FK_CHECK_LAUNCH(name);
  return FK_OK;
}

extern "C" int fk_scale_noise_bf16(const void* x0, int64_t x0_batch_stride, const void* noise, int64_t noise_batch_stride,
                                   void* out, int64_t out_batch_stride, int32_t B, int32_t S_tgt, int32_t C, float sigma,
                                   fk_stream_t stream) {
  FK_CHECK_ARG(x0 && noise && out && sizes_ok(B, S_tgt, C), "fk_scale_noise_bf16: bad sizes");
  if (int e = check_rows("fk_scale_noise_bf16", x0, x0_batch_stride, noise, noise_batch_stride, out, out_batch_stride)) return e;
  const float sb = host_round_bf(sigma), omsb = host_round_bf(1.0f - sb);
  const int64_t nvec = (int64_t)S_tgt * C / 8;
  hipLaunchKernelGGL(scale_noise_kernel, dim3(ew_grid(nvec), B), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)x0,
                     x0_batch_stride, (const bf16_t*)noise, noise_batch_stride, (bf16_t*)out, out_batch_stride, S_tgt, C,
                     sb, omsb);
  FK_CHECK_LAUNCH("fk_scale_noise_bf16");
  return FK_OK;
}

extern "C" int fk_ab2_step_bf16(void* x, int64_t x_batch_stride, const void* v, int64_t v_batch_stride, void* hist,
                                int64_t hist_batch_stride, const void* x0, int64_t x0_batch_stride, const void* noise,
                                int64_t noise_batch_stride, const void* mask, int64_t mask_batch_stride, int32_t B,
                                int32_t S_tgt, int32_t C, float c_v, float c_h, int32_t use_hist, float sigma_next,
                                fk_stream_t stream) {
  const char* name = "fk_ab2_step_bf16";
  FK_CHECK_ARG(x && v && hist && sizes_ok(B, S_tgt, C), "fk_ab2_step_bf16: bad sizes");
  FK_CHECK_ARG(hist != v && hist != x, "fk_ab2_step_bf16: hist must be a buffer of its own (it is written while v and x are read)");
  FK_CHECK_ARG(use_hist == 0 || use_hist == 1, "fk_ab2_step_bf16: use_hist=%d is neither 0 nor 1", (int)use_hist);
  if (int e = check_rows(name, x, x_batch_stride, v, v_batch_stride, hist, hist_batch_stride)) return e;
  const keep_args keep = keep_of(x0, x0_batch_stride, noise, noise_batch_stride, mask, mask_batch_stride);
  float sb = 0.0f, omsb = 0.0f;
  if (mask) {
    if (int e = check_keep(name, keep)) return e;
    sb = host_round_bf(sigma_next);
    omsb = host_round_bf(1.0f - sb);
  }
  const int64_t nvec = (int64_t)S_tgt * C / 8;
  const dim3 grid(ew_grid(nvec), B), block(256);
  with_hist_mask(use_hist, mask != nullptr, [&](auto H, auto M) {
    hipLaunchKernelGGL((ab2_kernel<decltype(H)::value, decltype(M)::value>), grid, block, 0, (hipStream_t)stream, (bf16_t*)x,
                       x_batch_stride, (const bf16_t*)v, v_batch_stride, (bf16_t*)hist, hist_batch_stride, keep, S_tgt, C, c_v,
                       c_h, sb, omsb);
  });
  FK_CHECK_LAUNCH(name);
  return FK_OK;
}

namespace {

// The same rule on a float32 state (fk_solver_step_f32): the sum is kept unrounded in `state` from step to step and the token
// rows receive its one rounding to bf16, the model's next input.  The keep-region value and the blend are float32 too
// (blend8_f32).  The vector layout is ab2_kernel's; the state is two 16-byte accesses per vector.  load_state == 0 (the first
// executed step) widens the bf16 token rows instead and never reads `state`; hist == nullptr (Euler) stores no history.
template <bool HIST, bool MASK>
__global__ __launch_bounds__(256) void state_kernel(float* state, int64_t s_bs, bf16_t* x, int64_t x_bs, const bf16_t* v,
                                                    int64_t v_bs, bf16_t* hist, int64_t h_bs, keep_args keep, int S_tgt, int C,
                                                    float c_v, float c_h, int load_state, float sn, float om) {
  const int b = blockIdx.y;
  const int64_t cvec = C / 8, nvec = (int64_t)S_tgt * cvec;
  float* sb = state + (int64_t)b * s_bs;
  bf16_t* xb = x + (int64_t)b * x_bs;
  const bf16_t* vb = v + (int64_t)b * v_bs;
  bf16_t* hb = hist ? hist + (int64_t)b * h_bs : nullptr;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < nvec; i += (int64_t)gridDim.x * 256) {
    const u32x4_t vw = *(const u32x4_t*)(vb + i * 8);
    float s[8];
    if (load_state) {
      const f32x4_t lo = *(const f32x4_t*)(sb + i * 8), hi = *(const f32x4_t*)(sb + i * 8 + 4);
#pragma unroll
      for (int e = 0; e < 4; ++e) s[e] = lo[e], s[4 + e] = hi[e];
    } else {
      widen8(s, *(const u32x4_t*)(xb + i * 8));
    }
    axpy8_rn(s, c_v, vw);
    if (HIST) axpy8_rn(s, c_h, *(const u32x4_t*)(hb + i * 8));   // this thread's h, read before the store below replaces it
    if (hb) *(u32x4_t*)(hb + i * 8) = vw;
    if (MASK) blend8_f32(s, keep, b, i, cvec, sn, om);
    *(f32x4_t*)(sb + i * 8) = f32x4_t{s[0], s[1], s[2], s[3]};
    *(f32x4_t*)(sb + i * 8 + 4) = f32x4_t{s[4], s[5], s[6], s[7]};
    *(u32x4_t*)(xb + i * 8) = pack8(s);
  }
}

}  // namespace

extern "C" int fk_solver_step_f32(float* state, int64_t state_batch_stride, void* x, int64_t x_batch_stride, const void* v,
                                  int64_t v_batch_stride, void* hist, int64_t hist_batch_stride, const void* x0,
                                  int64_t x0_batch_stride, const void* noise, int64_t noise_batch_stride, const void* mask,
                                  int64_t mask_batch_stride, int32_t B, int32_t S_tgt, int32_t C, float c_v, float c_h,
                                  int32_t use_hist, int32_t load_state, float sigma_next, fk_stream_t stream) {
  const char* name = "fk_solver_step_f32";
  FK_CHECK_ARG(state && x && v && sizes_ok(B, S_tgt, C), "fk_solver_step_f32: bad sizes");
  FK_CHECK_ARG(use_hist == 0 || use_hist == 1, "fk_solver_step_f32: use_hist=%d is neither 0 nor 1", (int)use_hist);
  FK_CHECK_ARG(load_state == 0 || load_state == 1, "fk_solver_step_f32: load_state=%d is neither 0 nor 1", (int)load_state);
  FK_CHECK_ARG(hist || !use_hist, "fk_solver_step_f32: use_hist=1 needs a history buffer");
  FK_CHECK_ARG(!hist || (hist != v && hist != x && hist != (void*)state),
               "fk_solver_step_f32: hist must be a buffer of its own (it is written while v, x and state are read)");
  FK_CHECK_ARG((void*)state != x, "fk_solver_step_f32: state must be a buffer of its own (x receives its bf16 rounding)");
  if (int e = check_rows(name, x, x_batch_stride, v, v_batch_stride, hist, hist_batch_stride)) return e;
  FK_CHECK_ARG(state_batch_stride % 4 == 0 && ((uintptr_t)state % 16 == 0), "fk_solver_step_f32: alignment of the state");
  const keep_args keep = keep_of(x0, x0_batch_stride, noise, noise_batch_stride, mask, mask_batch_stride);
  float om = 0.0f;
  if (mask) {
    if (int e = check_keep(name, keep)) return e;
    om = 1.0f - sigma_next;   // float32(1 - sigma_next), formed once: sigma_next itself is not rounded to bf16 here
  }
  const int64_t nvec = (int64_t)S_tgt * C / 8;
  const dim3 grid(ew_grid(nvec), B), block(256);
  with_hist_mask(use_hist, mask != nullptr, [&](auto H, auto M) {
    hipLaunchKernelGGL((state_kernel<decltype(H)::value, decltype(M)::value>), grid, block, 0, (hipStream_t)stream, state,
                       state_batch_stride, (bf16_t*)x, x_batch_stride, (const bf16_t*)v, v_batch_stride, (bf16_t*)hist,
                       hist_batch_stride, keep, S_tgt, C, c_v, c_h, (int)load_state, sigma_next, om);
  });
  FK_CHECK_LAUNCH(name);
  return FK_OK;
}
