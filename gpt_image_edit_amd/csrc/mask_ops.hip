// Pixel arithmetic of a masked edit that works on the masked box and pastes the result back (include/fk.h states each rule):
//   fk_mask_bbox_u8                 bounding box of the mask bytes >= a threshold (per-block partials + a one-block finish)
//   fk_mask_blur_u8                 separable Gaussian feather of the mask, taps added in ascending order
//   fk_pixels_u8_box_to_nhwc_bf16   a box of the picture, bilinear, in front of the VAE encoder
//   fk_image_overlay_u8             the decoded result resampled into the box and alpha-blended over the picture's own bytes
// Four HBM-bound single passes on the elementwise grid.  Every product, sum and division is one operation -- fp32, except the
// crop's, which are fp64 (K3 below says why): the file is built with -ffp-contract=off (Makefile), so a product and a sum stay
// apart.  Every index is clamped before its load; nothing here uses atomics.
#include "pixel_common.h"
#include "step_common.h"   // ew_grid

namespace {

constexpr int BBOX_THREADS = 256;

struct box_t { int x0, y0, x1, y1; };

// ---- K1 ------------------------------------------------------------------------------------------------------------------------
// (min x, min y, max x + 1, max y + 1) of four candidates merged over the block, thread 0 writes the block's four ints
FK_DEV void bbox_block_merge(int lx, int ly, int hx, int hy, int* out4) {
  __shared__ int s[4][BBOX_THREADS];
  const int t = threadIdx.x;
  s[0][t] = lx; s[1][t] = ly; s[2][t] = hx; s[3][t] = hy;
  __syncthreads();
  for (int w = BBOX_THREADS / 2; w > 0; w >>= 1) {
    if (t < w) {
      s[0][t] = min(s[0][t], s[0][t + w]);
      s[1][t] = min(s[1][t], s[1][t + w]);
      s[2][t] = max(s[2][t], s[2][t + w]);
      s[3][t] = max(s[3][t], s[3][t + w]);
    }
    __syncthreads();
  }
  if (t == 0) { out4[0] = s[0][0]; out4[1] = s[1][0]; out4[2] = s[2][0]; out4[3] = s[3][0]; }
}

// VEC: W % 4 == 0 and a 4-byte aligned mask, so a lane's four bytes are one load and lie in one row
template <bool VEC>
__global__ __launch_bounds__(BBOX_THREADS) void bbox_partial_kernel(const uint8_t* mask, int* ws, int64_t total, int H, int W,
                                                                    int thr) {
  int lx = W, ly = H, hx = 0, hy = 0;
  constexpr int PER = VEC ? 4 : 1;
  const int64_t n = total / PER;
  for (int64_t i = (int64_t)blockIdx.x * BBOX_THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * BBOX_THREADS) {
    const int64_t p = i * PER, row = p / W;
    const int x = (int)(p - row * W), y = (int)(row % H);
    uint32_t w;
    if constexpr (VEC) w = *(const uint32_t*)(mask + p);
    else w = mask[p];
#pragma unroll
    for (int e = 0; e < PER; ++e)
      if ((int)((w >> (8 * e)) & 0xffu) >= thr) {
        lx = min(lx, x + e); hx = max(hx, x + e + 1);
        ly = min(ly, y); hy = max(hy, y + 1);
      }
  }
  bbox_block_merge(lx, ly, hx, hy, ws + 4 * blockIdx.x);
}

__global__ __launch_bounds__(BBOX_THREADS) void bbox_finish_kernel(const int* ws, int nblk, int H, int W, int* out4) {
  int lx = W, ly = H, hx = 0, hy = 0;
  for (int i = threadIdx.x; i < nblk; i += BBOX_THREADS) {
    lx = min(lx, ws[4 * i]); ly = min(ly, ws[4 * i + 1]);
    hx = max(hx, ws[4 * i + 2]); hy = max(hy, ws[4 * i + 3]);
  }
  bbox_block_merge(lx, ly, hx, hy, out4);
}

// ---- K2 ------------------------------------------------------------------------------------------------------------------------
// One pass of the separable blur along x (ALONG_X) or y: acc = acc + w[k] * v(clamp(pos + k)), k = -R..R ascending.
// The horizontal pass reads the mask bytes and writes the fp32 plane; the vertical pass reads the plane and writes bytes.
template <bool ALONG_X>
__global__ __launch_bounds__(256) void blur_pass_kernel(const uint8_t* src_u8, const float* src_f, float* dst_f, uint8_t* dst_u8,
                                                        const float* taps, int R, int64_t total, int H, int W) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int64_t row = i / W;
    const int x = (int)(i - row * W), y = (int)(row % H);
    const int64_t plane0 = (row - y) * W;          // first element of this sample's plane
    float acc = 0.f;
    for (int k = -R; k <= R; ++k) {
      float v;
      if constexpr (ALONG_X) v = (float)src_u8[plane0 + (int64_t)y * W + min(max(x + k, 0), W - 1)];
      else v = src_f[plane0 + (int64_t)min(max(y + k, 0), H - 1) * W + x];
      acc = __fadd_rn(acc, __fmul_rn(taps[k + R], v));
    }
    if constexpr (ALONG_X) dst_f[i] = acc;
    else dst_u8[i] = (uint8_t)rintf(fminf(fmaxf(acc, 0.f), 255.f));
  }
}

// ---- the bilinear rule K3 and K4 share ------------------------------------------------------------------------------------------
// Output position X of n_out samples over a source of n_in: s = clamp((X + 0.5) * (n_in / n_out) - 0.5, 0, n_in - 1),
// i0 = floor(s), i1 = min(i0 + 1, n_in - 1), f = s - i0 (exact).  Equal sizes give s = X and f = 0.
// F = float for the overlay, double for the crop (below); the file is built without contraction, so each operator is one operation.
template <typename F>
FK_DEV void bilinear_tap(int X, int n_in, int n_out, int& i0, int& i1, F& f) {
  const F scale = (F)n_in / (F)n_out;
  F s = ((F)X + (F)0.5) * scale - (F)0.5;
  s = s < (F)0 ? (F)0 : (s > (F)(n_in - 1) ? (F)(n_in - 1) : s);
  const F fl = floor(s);
  i0 = min(max((int)fl, 0), n_in - 1);
  i1 = min(i0 + 1, n_in - 1);
  f = s - fl;
}

// (1 - fy) * ((1 - fx) * p00 + fx * p01) + fy * ((1 - fx) * p10 + fx * p11), every operation rounded once
template <typename F>
FK_DEV F bilinear_mix(F p00, F p01, F p10, F p11, F fx, F fy) {
  const F gx = (F)1 - fx, gy = (F)1 - fy;
  const F top = gx * p00 + fx * p01;
  const F bot = gx * p10 + fx * p11;
  return gy * top + fy * bot;
}

// ---- K3 ------------------------------------------------------------------------------------------------------------------------
// The crop is held to 1 bf16 ulp of the rule's exact value on EVERY element.  Float32 cannot give that: where the normalised value
// crosses 0 (u ~ 127.5; with renorm, u ~ 191.25) bf16's spacing falls below float32's rounding of s and u.  So the rule runs in
// float64, operation by operation in the stated order (the gather is HBM-bound; gfx950's float64 rate leaves it so), and the result
// is rounded to float32 and then to bf16.  A sample that lies on a source pixel (fx == fy == 0) takes pixel_norm of that byte in
// float32 instead -- the whole-picture kernel's value, so the whole picture at equal size gives that kernel's bits; for every byte
// and either renorm the two are at most 1 bf16 ulp apart (tests/test_mask_ops_ref.py).
__global__ __launch_bounds__(256) void pixels_box_kernel(const uint8_t* src, bf16_t* dst, int Hin, int Win, box_t box, int Hout,
                                                         int Wout, int Cpad, int renorm) {
  const int b = blockIdx.y;
  const int64_t total = (int64_t)Hout * Wout * Cpad;
  const uint8_t* sb = src + (int64_t)b * Hin * Win * 3;
  bf16_t* db = dst + (int64_t)b * total;
  const int bw = box.x1 - box.x0, bh = box.y1 - box.y0;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int c = (int)(i % Cpad);
    const int64_t pix = i / Cpad;
    float v = 0.f;
    if (c < 3) {
      const int y = (int)(pix / Wout), x = (int)(pix - (int64_t)y * Wout);
      int xa, xb, ya, yb;
      double fx, fy;
      bilinear_tap(x, bw, Wout, xa, xb, fx);
      bilinear_tap(y, bh, Hout, ya, yb, fy);
      const uint8_t* r0 = sb + ((int64_t)(box.y0 + ya) * Win + box.x0) * 3 + c;
      const uint8_t* r1 = sb + ((int64_t)(box.y0 + yb) * Win + box.x0) * 3 + c;
      if (fx == 0.0 && fy == 0.0) {
        v = pixel_norm((float)r0[xa * 3], renorm);
      } else {
        const double u = bilinear_mix((double)r0[xa * 3], (double)r0[xb * 3], (double)r1[xa * 3], (double)r1[xb * 3], fx, fy);
        double w = ((u / 255.0) - 0.5) / 0.5;
        if (renorm) w = 2.0 * w - 1.0;
        v = (float)w;
      }
    }
    db[i] = f2bf(v);
  }
}

// ---- K4 ------------------------------------------------------------------------------------------------------------------------
// grid (blocks, B).  orig_bs / alpha_bs: batch strides in bytes, 0 when one picture / one mask serves the batch.
template <typename T>
__global__ __launch_bounds__(256) void overlay_kernel(const T* img, int h, int w, const uint8_t* orig, int64_t orig_bs,
                                                      const uint8_t* alpha, int64_t alpha_bs, uint8_t* dst, int H, int W,
                                                      box_t box) {
  const int b = blockIdx.y;
  const int64_t total = (int64_t)H * W * 3, hw = (int64_t)h * w;
  const T* ib = img + (int64_t)b * 3 * hw;
  const uint8_t* ob = orig + (int64_t)b * orig_bs;
  const uint8_t* ab = alpha ? alpha + (int64_t)b * alpha_bs : nullptr;
  uint8_t* db = dst + (int64_t)b * total;
  const int bw = box.x1 - box.x0, bh = box.y1 - box.y0;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int c = (int)(i % 3);
    const int64_t pix = i / 3;
    const int Y = (int)(pix / W), X = (int)(pix - (int64_t)Y * W);
    const uint8_t o = ob[i];
    uint8_t out = o;
    if (X >= box.x0 && X < box.x1 && Y >= box.y0 && Y < box.y1) {
      const int a = ab ? (int)ab[pix] : 255;
      if (a != 0) {                                 // a == 0: the original's byte, taken
        int xa, xb, ya, yb;
        float fx, fy;                               // float32: the overlay's bound is derived for it (tests/mask_ops_ref.py)
        bilinear_tap(X - box.x0, w, bw, xa, xb, fx);
        bilinear_tap(Y - box.y0, h, bh, ya, yb, fy);
        const T* r0 = ib + (int64_t)c * hw + (int64_t)ya * w;
        const T* r1 = ib + (int64_t)c * hw + (int64_t)yb * w;
        const float g = bilinear_mix(image_unit(r0[xa]), image_unit(r0[xb]), image_unit(r1[xa]), image_unit(r1[xb]), fx, fy);
        float v = __fmul_rn(g, 255.0f);
        if (a != 255)                               // a == 255: the resampled result, taken
          v = __fdiv_rn(__fadd_rn(__fmul_rn((float)a, v), __fmul_rn((float)(255 - a), (float)o)), 255.0f);
        out = (uint8_t)rintf(fminf(fmaxf(v, 0.f), 255.f));
      }
    }
    db[i] = out;
  }
}

inline bool box_inside(const box_t& b, int H, int W) {
  return b.x0 >= 0 && b.y0 >= 0 && b.x0 < b.x1 && b.y0 < b.y1 && b.x1 <= W && b.y1 <= H;
}

}  // namespace

extern "C" int64_t fk_mask_bbox_ws_ints(void) { return 4 * (int64_t)ew_grid(INT64_MAX / 2); }

extern "C" int fk_mask_bbox_u8(const void* mask, int32_t Bm, int32_t H, int32_t W, int32_t threshold, int32_t* out4,
                               int32_t* ws, int64_t ws_ints, fk_stream_t stream_) {
  FK_CHECK_ARG(mask && out4 && ws && Bm > 0 && H > 0 && W > 0, "fk_mask_bbox_u8: bad arguments");
  FK_CHECK_ARG(threshold >= 0 && threshold <= 255, "fk_mask_bbox_u8: threshold=%d is no byte value", threshold);
  FK_CHECK_ARG(ws_ints >= fk_mask_bbox_ws_ints(), "fk_mask_bbox_u8: workspace of %lld ints, needs fk_mask_bbox_ws_ints() = %lld",
               (long long)ws_ints, (long long)fk_mask_bbox_ws_ints());
  FK_CHECK_ARG((uintptr_t)out4 % 4 == 0 && (uintptr_t)ws % 4 == 0 && (void*)out4 != (void*)ws, "fk_mask_bbox_u8: alignment");
  const int64_t total = (int64_t)Bm * H * W;
  const bool vec = W % 4 == 0 && (uintptr_t)mask % 4 == 0;
  const int nblk = ew_grid(vec ? total / 4 : total);
  hipStream_t s = (hipStream_t)stream_;
  if (vec) hipLaunchKernelGGL(bbox_partial_kernel<true>, dim3(nblk), dim3(BBOX_THREADS), 0, s, (const uint8_t*)mask, ws, total, H, W, threshold);
  else hipLaunchKernelGGL(bbox_partial_kernel<false>, dim3(nblk), dim3(BBOX_THREADS), 0, s, (const uint8_t*)mask, ws, total, H, W, threshold);
  hipLaunchKernelGGL(bbox_finish_kernel, dim3(1), dim3(BBOX_THREADS), 0, s, (const int*)ws, nblk, H, W, out4);
  FK_CHECK_LAUNCH("fk_mask_bbox_u8");
  return FK_OK;
}

extern "C" int fk_mask_blur_u8(const void* src, void* dst, float* plane, const float* taps, int32_t R, int32_t Bm, int32_t H,
                               int32_t W, fk_stream_t stream_) {
  FK_CHECK_ARG(src && dst && plane && taps && Bm > 0 && H > 0 && W > 0, "fk_mask_blur_u8: bad arguments");
  FK_CHECK_ARG(R >= 0 && R <= FK_MASK_BLUR_MAX_RADIUS, "fk_mask_blur_u8: R=%d is outside [0, %d]", R, FK_MASK_BLUR_MAX_RADIUS);
  FK_CHECK_ARG((uintptr_t)plane % 4 == 0 && (uintptr_t)taps % 4 == 0, "fk_mask_blur_u8: alignment");
  FK_CHECK_ARG((void*)plane != src && (void*)plane != dst && (const void*)taps != (const void*)plane,
               "fk_mask_blur_u8: the plane must be a buffer of its own");
  const int64_t total = (int64_t)Bm * H * W;
  const dim3 grid(ew_grid(total)), block(256);
  hipStream_t s = (hipStream_t)stream_;
  hipLaunchKernelGGL(blur_pass_kernel<true>, grid, block, 0, s, (const uint8_t*)src, (const float*)nullptr, plane,
                     (uint8_t*)nullptr, taps, R, total, H, W);
  hipLaunchKernelGGL(blur_pass_kernel<false>, grid, block, 0, s, (const uint8_t*)nullptr, (const float*)plane, (float*)nullptr,
                     (uint8_t*)dst, taps, R, total, H, W);
  FK_CHECK_LAUNCH("fk_mask_blur_u8");
  return FK_OK;
}

extern "C" int fk_pixels_u8_box_to_nhwc_bf16(const void* src, void* dst, int32_t B, int32_t Hin, int32_t Win, int32_t x0,
                                             int32_t y0, int32_t x1, int32_t y1, int32_t Hout, int32_t Wout, int32_t Cpad,
                                             int32_t renorm, fk_stream_t stream_) {
  FK_CHECK_ARG(src && dst && B > 0 && Hin > 0 && Win > 0 && Hout > 0 && Wout > 0 && Cpad >= 3,
               "fk_pixels_u8_box_to_nhwc_bf16: bad arguments");
  const box_t box{x0, y0, x1, y1};
  FK_CHECK_ARG(box_inside(box, Hin, Win), "fk_pixels_u8_box_to_nhwc_bf16: box (%d, %d, %d, %d) is empty or outside the %d x %d picture",
               x0, y0, x1, y1, Win, Hin);
  const dim3 grid(ew_grid((int64_t)Hout * Wout * Cpad), B), block(256);
  hipLaunchKernelGGL(pixels_box_kernel, grid, block, 0, (hipStream_t)stream_, (const uint8_t*)src, (bf16_t*)dst, Hin, Win, box,
                     Hout, Wout, Cpad, renorm);
  FK_CHECK_LAUNCH("fk_pixels_u8_box_to_nhwc_bf16");
  return FK_OK;
}

extern "C" int fk_image_overlay_u8(const void* img, int32_t img_is_fp32, int32_t h, int32_t w, const void* orig, int32_t orig_batch,
                                   const void* alpha, int32_t alpha_batch, void* dst, int32_t B, int32_t H, int32_t W, int32_t x0,
                                   int32_t y0, int32_t x1, int32_t y1, fk_stream_t stream_) {
  FK_CHECK_ARG(img && orig && dst && B > 0 && h > 0 && w > 0 && H > 0 && W > 0, "fk_image_overlay_u8: bad arguments");
  FK_CHECK_ARG(orig_batch == 1 || orig_batch == B, "fk_image_overlay_u8: %d original pictures for a batch of %d", orig_batch, B);
  FK_CHECK_ARG(alpha ? (alpha_batch == 1 || alpha_batch == B) : alpha_batch == 0,
               "fk_image_overlay_u8: alpha_batch=%d is neither 1 nor the batch %d (0 without alpha)", alpha_batch, B);
  const box_t box{x0, y0, x1, y1};
  FK_CHECK_ARG(box_inside(box, H, W), "fk_image_overlay_u8: box (%d, %d, %d, %d) is empty or outside the %d x %d picture", x0, y0,
               x1, y1, W, H);
  FK_CHECK_ARG(dst != orig && dst != alpha && dst != img, "fk_image_overlay_u8: dst must be a buffer of its own");
  FK_CHECK_ARG((uintptr_t)img % (img_is_fp32 ? 4 : 2) == 0, "fk_image_overlay_u8: alignment");
  const int64_t HW = (int64_t)H * W;
  const dim3 grid(ew_grid(HW * 3), B), block(256);
  const int64_t obs = orig_batch == 1 ? 0 : HW * 3, abs_ = alpha_batch == B && B > 1 ? HW : 0;
  hipStream_t s = (hipStream_t)stream_;
  if (img_is_fp32) hipLaunchKernelGGL(overlay_kernel<float>, grid, block, 0, s, (const float*)img, h, w, (const uint8_t*)orig, obs, (const uint8_t*)alpha, abs_, (uint8_t*)dst, H, W, box);
  else hipLaunchKernelGGL(overlay_kernel<bf16_t>, grid, block, 0, s, (const bf16_t*)img, h, w, (const uint8_t*)orig, obs, (const uint8_t*)alpha, abs_, (uint8_t*)dst, H, W, box);
  FK_CHECK_LAUNCH("fk_image_overlay_u8");
  return FK_OK;
}
