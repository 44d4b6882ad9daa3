// Antialiased byte resize and byte paste-back (include/fk.h states both rules):
//   fk_resample_pass_u8   one pass of Pillow's 8-bit resize along one axis: out = clip((2^21 + sum_t kk_t * src[xmin + t]) >> 22)
//   fk_bytes_overlay_u8   the resized result blended over the picture's own bytes inside a box
// Pure integer arithmetic on host-made tables: nothing here can be contracted, and the result does not depend on the order of the
// sum, so the horizontal pass may walk a window in pieces.  Every window is clamped to the axis and to ksize taps before a load,
// whatever the tables hold.
//
// Vertical pass: a block owns one output row's piece of 256 lanes; a lane owns 4 consecutive bytes of the row (one dword; one byte
// when the view is not 4-byte aligned), so a tap is one coalesced row read.  The output row, hence its window and its weights, is
// the same for the whole block: the tap loop is wave-uniform and hipcc reads bounds and weights through the scalar cache.
//
// Horizontal pass: a block owns 256 adjacent outputs of one row; a lane owns one output pixel, all channels.  Adjacent outputs read
// overlapping windows, so the block stages the union of its windows in LDS (dword copies between the 4-byte boundaries of the
// source, bytes at the two ends), in pieces of RS_SPAN_BYTES when the union is longer: a 256-tap window at 1/256 spans far more
// than LDS holds.  The table is tap-major [ksize, n_out]: at tap t adjacent lanes read adjacent weights.
#include "fk_common.h"
#include "step_common.h"   // ew_grid

namespace {

constexpr int RS_BITS = 22;
constexpr int RS_THREADS = 256;
constexpr int RS_MAX_BLOCKS = 8192;       // grid cap; a block strides over the work items beyond it
constexpr int RS_SPAN_BYTES = 8192;       // LDS piece of a horizontal tile's source span

struct box_t { int x0, y0, x1, y1; };

// The empty statement keeps the shift and the clamp apart.  Left together, hipcc fuses two of them into one v_ashr_pk_u8_i32 and
// then ORs further bytes into that register as if its upper half were zero; on the MI355X the instruction leaves the upper half
// as it was (bytes 2 and 3 of every packed dword came out wrong, tests/test_hip_resample_kernels.py).  v_med3_i32 it is.
FK_DEV uint32_t rs_clip(int acc) {
  int v = (acc + (1 << (RS_BITS - 1))) >> RS_BITS;
  asm volatile("" : "+v"(v));
  return (uint32_t)min(max(v, 0), 255);
}

// (xmin, xmax) of output i, made safe: 0 <= xmin <= xmax <= n_in and xmax - xmin <= ksize
FK_DEV void rs_window(const int* bounds, int i, int n_in, int ksize, int& xmin, int& xmax) {
  xmin = min(max(bounds[2 * i], 0), n_in);
  xmax = min(max(bounds[2 * i + 1], xmin), min(n_in, xmin + ksize));
}

// work item = (sample b, output row i, piece of the row); rowbytes = Win * C
template <bool VEC>
__global__ __launch_bounds__(RS_THREADS) void resample_v_kernel(const uint8_t* src, int64_t sbs, int64_t srs, uint8_t* dst, int Hin,
                                                                int rowbytes, int n_out, const int* bounds, const int* kk,
                                                                int ksize, int pieces, int64_t items) {
  constexpr int PER = VEC ? 4 : 1;
  for (int64_t it = blockIdx.x; it < items; it += gridDim.x) {
    const int piece = (int)(it % pieces);
    const int64_t r = it / pieces;
    const int i = (int)(r % n_out);
    const int64_t b = r / n_out;
    int xmin, xmax;
    rs_window(bounds, i, Hin, ksize, xmin, xmax);
    const int col = (piece * RS_THREADS + (int)threadIdx.x) * PER;
    if (col >= rowbytes) continue;            // VEC: rowbytes % 4 == 0, so a lane's dword lies inside the row
    const uint8_t* p = src + b * sbs + (int64_t)xmin * srs + col;
    const int* w = kk + (int64_t)i * ksize;
    int acc[PER] = {};
    for (int t = 0; t < xmax - xmin; ++t, p += srs) {
      const int k = w[t];
      if constexpr (VEC) {
        const uint32_t v = *(const uint32_t*)p;
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[e] += k * (int)((v >> (8 * e)) & 0xffu);
      } else {
        acc[0] += k * (int)*p;
      }
    }
    uint8_t* d = dst + (b * n_out + i) * (int64_t)rowbytes + col;
    if constexpr (VEC) *(uint32_t*)d = rs_clip(acc[0]) | (rs_clip(acc[1]) << 8) | (rs_clip(acc[2]) << 16) | (rs_clip(acc[3]) << 24);
    else *d = (uint8_t)rs_clip(acc[0]);
  }
}

// work item = (sample b, source row y, tile of RS_THREADS outputs)
template <int C>
__global__ __launch_bounds__(RS_THREADS) void resample_h_kernel(const uint8_t* src, int64_t sbs, int64_t srs, uint8_t* dst, int Hin,
                                                                int Win, int n_out, const int* bounds, const int* kkT, int ksize,
                                                                int tiles, int64_t items) {
  __shared__ __attribute__((aligned(16))) uint8_t span[RS_SPAN_BYTES + 4];
  __shared__ int lohi[2];
  constexpr int PIECE = RS_SPAN_BYTES / C;    // source pixels per LDS piece
  const int tid = (int)threadIdx.x;
  for (int64_t it = blockIdx.x; it < items; it += gridDim.x) {
    const int tile = (int)(it % tiles);
    const int64_t r = it / tiles;
    const int y = (int)(r % Hin);
    const int64_t b = r / Hin;
    const int i = tile * RS_THREADS + tid;
    const bool live = i < n_out;
    int xmin = 0, xmax = 0;
    if (live) rs_window(bounds, i, Win, ksize, xmin, xmax);
    if (tid == 0) { lohi[0] = Win; lohi[1] = 0; }
    __syncthreads();
    if (live && xmax > xmin) { atomicMin(&lohi[0], xmin); atomicMax(&lohi[1], xmax); }
    __syncthreads();
    const int lo = lohi[0], hi = lohi[1];     // the union of the tile's windows, the same in every lane
    __syncthreads();                          // ... read by all before the next item resets it
    const uint8_t* row = src + b * sbs + (int64_t)y * srs;
    int acc[C] = {};
    for (int cb = lo; cb < hi; cb += PIECE) {
      const int npx = min(PIECE, hi - cb), nbytes = npx * C;
      const uint8_t* g = row + (int64_t)cb * C;
      // LDS byte off + k holds g[k]: a 4-byte boundary of the source is one of the LDS, and what lies between two is copied as dwords
      const int off = (int)((uintptr_t)g & 3);
      const int head = min((4 - off) & 3, nbytes);
      const int body = (nbytes - head) >> 2;
      const int tail = head + 4 * body;
      if (tid < head) span[off + tid] = g[tid];
      if (body > 0) {
        const uint32_t* g32 = (const uint32_t*)(g + head);
        uint32_t* s32 = (uint32_t*)(span + off + head);
        for (int k = tid; k < body; k += RS_THREADS) s32[k] = g32[k];
      }
      if (tid < nbytes - tail) span[off + tail + tid] = g[tail + tid];
      __syncthreads();
      if (live) {
        const int t0 = max(xmin, cb), t1 = min(xmax, cb + npx);
        const int* w = kkT + (int64_t)(t0 - xmin) * n_out + i;
        const uint8_t* s = span + off + (t0 - cb) * C;
        for (int x = t0; x < t1; ++x, w += n_out, s += C) {
          const int k = *w;
#pragma unroll
          for (int c = 0; c < C; ++c) acc[c] += k * (int)s[c];
        }
      }
      __syncthreads();
    }
    if (live) {
      uint8_t* d = dst + ((b * Hin + y) * (int64_t)n_out + i) * C;
#pragma unroll
      for (int c = 0; c < C; ++c) d[c] = (uint8_t)rs_clip(acc[c]);
    }
  }
}

// grid (blocks, B).  orig_bs / alpha_bs: batch strides in bytes, 0 when one picture / one mask serves the batch.
__global__ __launch_bounds__(256) void bytes_overlay_kernel(const uint8_t* res, const uint8_t* orig, int64_t orig_bs,
                                                            const uint8_t* alpha, int64_t alpha_bs, uint8_t* dst, int H, int W,
                                                            box_t box) {
  const int b = blockIdx.y;
  const int64_t total = (int64_t)H * W * 3;
  const int bw = box.x1 - box.x0, bh = box.y1 - box.y0;
  const uint8_t* rb = res + (int64_t)b * bh * bw * 3;
  const uint8_t* ob = orig + (int64_t)b * orig_bs;
  const uint8_t* ab = alpha ? alpha + (int64_t)b * alpha_bs : nullptr;
  uint8_t* db = dst + (int64_t)b * total;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int c = (int)(i % 3);
    const int64_t pix = i / 3;
    const int Y = (int)(pix / W), X = (int)(pix - (int64_t)Y * W);
    const uint8_t o = ob[i];
    uint8_t out = o;
    if (X >= box.x0 && X < box.x1 && Y >= box.y0 && Y < box.y1) {
      const uint32_t a = ab ? ab[pix] : 255u;
      if (a != 0) {                                 // a == 0: the original's byte, taken
        const uint32_t rv = rb[((int64_t)(Y - box.y0) * bw + (X - box.x0)) * 3 + c];
        out = a == 255 ? (uint8_t)rv                // a == 255: the result's byte, taken
                       : (uint8_t)((2u * (a * rv + (255u - a) * (uint32_t)o) + 255u) / 510u);
      }
    }
    db[i] = out;
  }
}

inline bool box_inside(const box_t& b, int H, int W) {
  return b.x0 >= 0 && b.y0 >= 0 && b.x0 < b.x1 && b.y0 < b.y1 && b.x1 <= W && b.y1 <= H;
}

}  // namespace

extern "C" int fk_resample_pass_u8(const void* src, int64_t src_batch_stride, int64_t src_row_stride, void* dst, int32_t B,
                                   int32_t Hin, int32_t Win, int32_t C, int32_t axis, int32_t n_out, const int32_t* bounds,
                                   const int32_t* kk, int32_t ksize, fk_stream_t stream_) {
  FK_CHECK_ARG(src && dst && bounds && kk, "fk_resample_pass_u8: null pointer");
  FK_CHECK_ARG(C == 1 || C == 3, "fk_resample_pass_u8: C=%d is neither 1 nor 3", C);
  FK_CHECK_ARG(B > 0 && Hin > 0 && Win > 0 && n_out > 0, "fk_resample_pass_u8: sizes must be positive (B=%d, Hin=%d, Win=%d, n_out=%d)",
               B, Hin, Win, n_out);
  FK_CHECK_ARG(axis == 0 || axis == 1, "fk_resample_pass_u8: axis=%d is neither 0 (vertical) nor 1 (horizontal)", axis);
  FK_CHECK_ARG(ksize >= 1, "fk_resample_pass_u8: ksize=%d is below 1", ksize);
  FK_CHECK_ARG(ksize <= FK_RESAMPLE_MAX_KSIZE, "fk_resample_pass_u8: ksize=%d is above FK_RESAMPLE_MAX_KSIZE = %d", ksize,
               FK_RESAMPLE_MAX_KSIZE);
  const int64_t rowbytes = (int64_t)Win * C;
  FK_CHECK_ARG(src_row_stride >= rowbytes && src_batch_stride >= 0,
               "fk_resample_pass_u8: rows of %lld bytes overlap at a row stride of %lld (batch stride %lld)", (long long)rowbytes,
               (long long)src_row_stride, (long long)src_batch_stride);
  FK_CHECK_ARG(rowbytes <= INT32_MAX && (int64_t)n_out * C <= INT32_MAX, "fk_resample_pass_u8: a row is longer than 2^31 bytes");
  FK_CHECK_ARG((uintptr_t)bounds % 4 == 0 && (uintptr_t)kk % 4 == 0, "fk_resample_pass_u8: alignment");
  FK_CHECK_ARG(dst != src, "fk_resample_pass_u8: dst must be a buffer of its own");
  hipStream_t s = (hipStream_t)stream_;
  const uint8_t* sp = (const uint8_t*)src;
  uint8_t* dp = (uint8_t*)dst;
  if (axis == 0) {
    const bool vec = rowbytes % 4 == 0 && (uintptr_t)src % 4 == 0 && (uintptr_t)dst % 4 == 0 && src_row_stride % 4 == 0 &&
                     src_batch_stride % 4 == 0;
    const int per = (vec ? 4 : 1) * RS_THREADS;
    const int pieces = (int)((rowbytes + per - 1) / per);
    const int64_t items = (int64_t)B * n_out * pieces;
    const dim3 grid((unsigned)(items < RS_MAX_BLOCKS ? items : RS_MAX_BLOCKS)), block(RS_THREADS);
    if (vec) hipLaunchKernelGGL(resample_v_kernel<true>, grid, block, 0, s, sp, src_batch_stride, src_row_stride, dp, Hin, (int)rowbytes, n_out, bounds, kk, ksize, pieces, items);
    else hipLaunchKernelGGL(resample_v_kernel<false>, grid, block, 0, s, sp, src_batch_stride, src_row_stride, dp, Hin, (int)rowbytes, n_out, bounds, kk, ksize, pieces, items);
  } else {
    const int tiles = (n_out + RS_THREADS - 1) / RS_THREADS;
    const int64_t items = (int64_t)B * Hin * tiles;
    const dim3 grid((unsigned)(items < RS_MAX_BLOCKS ? items : RS_MAX_BLOCKS)), block(RS_THREADS);
    if (C == 3) hipLaunchKernelGGL(resample_h_kernel<3>, grid, block, 0, s, sp, src_batch_stride, src_row_stride, dp, Hin, Win, n_out, bounds, kk, ksize, tiles, items);
    else hipLaunchKernelGGL(resample_h_kernel<1>, grid, block, 0, s, sp, src_batch_stride, src_row_stride, dp, Hin, Win, n_out, bounds, kk, ksize, tiles, items);
  }
  FK_CHECK_LAUNCH("fk_resample_pass_u8");
  return FK_OK;
}

extern "C" int fk_bytes_overlay_u8(const void* res, const void* orig, int32_t orig_batch, const void* alpha, int32_t alpha_batch,
                                   void* dst, int32_t B, int32_t H, int32_t W, int32_t x0, int32_t y0, int32_t x1, int32_t y1,
                                   fk_stream_t stream_) {
  FK_CHECK_ARG(res && orig && dst && B > 0 && H > 0 && W > 0, "fk_bytes_overlay_u8: bad arguments");
  FK_CHECK_ARG(orig_batch == 1 || orig_batch == B, "fk_bytes_overlay_u8: %d original pictures for a batch of %d", orig_batch, B);
  FK_CHECK_ARG(alpha ? (alpha_batch == 1 || alpha_batch == B) : alpha_batch == 0,
               "fk_bytes_overlay_u8: alpha_batch=%d is neither 1 nor the batch %d (0 without alpha)", alpha_batch, B);
  const box_t box{x0, y0, x1, y1};
  FK_CHECK_ARG(box_inside(box, H, W), "fk_bytes_overlay_u8: box (%d, %d, %d, %d) is empty or outside the %d x %d picture", x0, y0,
               x1, y1, W, H);
  FK_CHECK_ARG(dst != orig && dst != alpha && dst != res, "fk_bytes_overlay_u8: dst must be a buffer of its own");
  const int64_t HW = (int64_t)H * W;
  const dim3 grid(ew_grid(HW * 3), B), block(256);
  const int64_t obs = orig_batch == 1 ? 0 : HW * 3, abs_ = alpha_batch == B && B > 1 ? HW : 0;
  hipLaunchKernelGGL(bytes_overlay_kernel, grid, block, 0, (hipStream_t)stream_, (const uint8_t*)res, (const uint8_t*)orig, obs,
                     (const uint8_t*)alpha, abs_, (uint8_t*)dst, H, W, box);
  FK_CHECK_LAUNCH("fk_bytes_overlay_u8");
  return FK_OK;
}
