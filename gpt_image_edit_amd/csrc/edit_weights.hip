// The edit-region loss weights of a (reference picture, target picture) pair, integer arithmetic only (include/fk.h states each rule):
//   fk_edit_diff_mask_u8        E1  |ref - tgt| per channel -> Pillow's "L" grey -> 255 where grey >= threshold
//   fk_mask_close5_u8           E2  closing with the 5 x 5 ellipse: dilation then erosion, the outside never counted
//   fk_mask_filter_components   E3  8-connected components per plane; one survives iff den * area >= num * white count of the plane
//   fk_mask_and_pool8_u8        E4  AND over a sample's references, white count, all-white fallback, 8 x 8 max pool, E2, white count
//   fk_mask_weight_fill_f32     E5  w[b] where the pooled mask is white, 1.0f elsewhere
// A mask byte is white iff it is >= 128 (the masks these entries write hold 0 or 255).  E3 uses integer atomicMin / atomicAdd: the
// labels it converges to (the least pixel index of each component) and the sums do not depend on their order.  EVERY loop below has
// a bound that comes from the plane's size; a root chase or a union that reaches its bound sets the status word and stops.
#include "step_common.h"   // ew_grid

namespace {

constexpr int TILE = FK_MASK_CLOSE_TILE;   // E2: output tile of one block pass
constexpr int IN_T = TILE + 8;             // the tile's bytes with a halo of 4 (2 for the dilation under 2 for the erosion)
constexpr int DIL_T = TILE + 4;            // the dilated values the tile's erosion reads

FK_DEV bool is_white(uint8_t v) { return v >= 128; }

// ---- E1 ------------------------------------------------------------------------------------------------------------------------
// ref_bs: bytes between the reference pictures (>= H * W * 3: a slice [:, r] of [B, R, H, W, 3] is read where it lies)
__global__ __launch_bounds__(256) void diff_mask_kernel(const uint8_t* ref, int64_t ref_bs, const uint8_t* tgt, uint8_t* dst,
                                                        int64_t total, int64_t HW, int thr) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int64_t n = i / HW;
    const uint8_t* r = ref + n * ref_bs + (i - n * HW) * 3;
    const uint8_t* t = tgt + i * 3;
    const int dr = abs((int)r[0] - (int)t[0]), dg = abs((int)r[1] - (int)t[1]), db = abs((int)r[2] - (int)t[2]);
    const int grey = (19595 * dr + 38470 * dg + 7471 * db + 32768) >> 16;
    dst[i] = grey >= thr ? 255 : 0;
  }
}

// ---- E2 ------------------------------------------------------------------------------------------------------------------------
// the ellipse's rows 00100 / 11111 / 11111 / 11111 / 00100 as (dy, dx) of a [.][stride] byte array around p
template <bool IS_AND>
FK_DEV int ellipse5(const uint8_t* p, int stride) {
  int v = IS_AND ? 1 : 0;
#pragma unroll
  for (int dy = -2; dy <= 2; ++dy) {
    const int r = (dy == -2 || dy == 2) ? 0 : 2;
#pragma unroll
    for (int dx = -r; dx <= r; ++dx) {
      if constexpr (IS_AND) v &= p[dy * stride + dx];
      else v |= p[dy * stride + dx];
    }
  }
  return v;
}

// One block closes one TILE x TILE tile per pass of its loop over (plane, tile row, tile column): the tile's bytes with a halo of 4
// into LDS (outside the plane: black, so it adds nothing to a dilation), the dilation of the tile with a halo of 2 (outside the
// plane: white, so it takes nothing from an erosion), the erosion of the tile.  counts != NULL: the white pixels of plane n are
// added to counts[2 n + 1] (E4).  The loop's bound is the number of tiles, which the plane's size gives.
__global__ __launch_bounds__(256) void close5_kernel(const uint8_t* src, uint8_t* dst, int64_t tiles, int tiles_y, int tiles_x, int H,
                                                     int W, int* counts) {
  __shared__ uint8_t s_in[IN_T][IN_T];
  __shared__ uint8_t s_dil[DIL_T][DIL_T];
  __shared__ int s_white;
  const int t = threadIdx.x;
  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const int tx = (int)(tile % tiles_x);
    const int64_t q = tile / tiles_x;
    const int ty = (int)(q % tiles_y);
    const int64_t n = q / tiles_y;
    const int x0 = tx * TILE, y0 = ty * TILE;
    const uint8_t* sp = src + n * H * W;
    if (t == 0) s_white = 0;
    for (int i = t; i < IN_T * IN_T; i += 256) {
      const int ly = i / IN_T, lx = i - ly * IN_T;
      const int y = y0 - 4 + ly, x = x0 - 4 + lx;
      s_in[ly][lx] = (y >= 0 && y < H && x >= 0 && x < W) ? (is_white(sp[(int64_t)y * W + x]) ? 1 : 0) : 0;
    }
    __syncthreads();
    for (int i = t; i < DIL_T * DIL_T; i += 256) {
      const int ly = i / DIL_T, lx = i - ly * DIL_T;
      const int y = y0 - 2 + ly, x = x0 - 2 + lx;
      s_dil[ly][lx] = (y >= 0 && y < H && x >= 0 && x < W) ? (uint8_t)ellipse5<false>(&s_in[ly + 2][lx + 2], IN_T) : 1;
    }
    __syncthreads();
    int white = 0;
    for (int i = t; i < TILE * TILE; i += 256) {
      const int ly = i / TILE, lx = i - ly * TILE;
      const int y = y0 + ly, x = x0 + lx;
      if (y < H && x < W) {
        const int v = ellipse5<true>(&s_dil[ly + 2][lx + 2], DIL_T);
        dst[n * H * W + (int64_t)y * W + x] = v ? 255 : 0;
        white += v;
      }
    }
    if (counts) {
      if (white) atomicAdd(&s_white, white);
      __syncthreads();
      if (t == 0 && s_white) atomicAdd(&counts[2 * n + 1], s_white);
    }
    __syncthreads();   // the next pass overwrites s_in, s_dil and s_white
  }
}

// ---- E3 ------------------------------------------------------------------------------------------------------------------------
// Workspace (int32): [0] status, [1, 1 + N) white count per plane, then the labels [N * H * W], then the areas [N * H * W].
// A label is a pixel's index in the whole [N, H, W] array (below 2^31), -1 on a black pixel.  L[i] <= i always, and a pixel's parent
// lies in its own plane and component, so a chain of parents is strictly decreasing inside one plane: at most H * W steps.
// Once the status word is set the result is an error whatever the labels hold: a chase looks at the word every 256 steps and a
// union before each try, and both give up, so the bounds of a failing launch do not multiply.
FK_DEV bool failed(const int* status) { return __atomic_load_n(status, __ATOMIC_RELAXED) != 0; }

FK_DEV int find_root(const int* L, int i, int bound, int* status) {
  for (int k = 0; k < bound; ++k) {
    if ((k & 255) == 255 && failed(status)) return i;
    const int p = L[i];
    if (p == i) return i;
    if (p < 0 || p > i) break;      // no label of a white pixel: a bug, reported like a bound
    i = p;
  }
  atomicOr(status, 1);
  return i;
}

// Join the trees of a and b: the larger root is pointed at the smaller with atomicMin.  When the atomic finds that the larger one
// was no root any more it returns that pixel's newer parent, which is smaller: the larger of the two indices in hand falls with every
// retry, so there are at most H * W of them.  The tree's root ends as the least index of the component whatever the order.
FK_DEV void unite(int* L, int a, int b, int bound, int* status) {
  for (int k = 0; k < bound; ++k) {
    if (failed(status)) return;
    a = find_root(L, a, bound, status);
    b = find_root(L, b, bound, status);
    if (a == b) return;
    if (a < b) { const int s = a; a = b; b = s; }
    const int old = atomicMin(&L[a], b);
    if (old == a) return;
    a = old;
  }
  atomicOr(status, 1);
}

// Black: label -1.  The first pixel of a horizontal run of white labels the whole run with its own index (at most W steps), so the
// run is one tree from the start.  Every pixel's area is cleared by its own thread.
__global__ __launch_bounds__(256) void cc_init_kernel(const uint8_t* mask, int* L, int* area, int64_t total, int W) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    area[i] = 0;
    const int x = (int)(i % W);
    if (!is_white(mask[i])) { L[i] = -1; continue; }
    if (x > 0 && is_white(mask[i - 1])) continue;                   // labelled by the run's first pixel
    for (int k = 0; k < W - x; ++k) {
      if (!is_white(mask[i + k])) break;
      L[i + k] = (int)i;
    }
  }
}

// A white pixel joins the run above it: through the pixel straight above when that is white (its white neighbours left and right
// are in the same run), otherwise through the two diagonal ones.
__global__ __launch_bounds__(256) void cc_merge_kernel(const uint8_t* mask, int* L, int64_t total, int H, int W, int* status) {
  const int bound = H * W;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int x = (int)(i % W), y = (int)((i / W) % H);
    if (y == 0 || !is_white(mask[i])) continue;
    const int64_t up = i - W;
    if (is_white(mask[up])) { unite(L, (int)i, (int)up, bound, status); continue; }
    if (x > 0 && is_white(mask[up - 1])) unite(L, (int)i, (int)(up - 1), bound, status);
    if (x + 1 < W && is_white(mask[up + 1])) unite(L, (int)i, (int)(up + 1), bound, status);
  }
}

// Every white pixel takes its root; a reader that meets a pixel before or after its store finds the same root either way.
__global__ __launch_bounds__(256) void cc_flatten_kernel(int* L, int64_t total, int H, int W, int* status) {
  const int bound = H * W;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    if (L[i] < 0) continue;
    L[i] = find_root(L, (int)i, bound, status);
  }
}

// The first pixel of each run adds the run's length (at most W steps) to its root's area and to its plane's white count.
__global__ __launch_bounds__(256) void cc_count_kernel(const int* L, int* area, int* white, int64_t total, int H, int W) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int x = (int)(i % W);
    if (L[i] < 0 || (x > 0 && L[i - 1] >= 0)) continue;
    int len = 0;
    for (int k = 0; k < W - x; ++k) {
      if (L[i + k] < 0) break;
      ++len;
    }
    atomicAdd(&area[L[i]], len);
    atomicAdd(&white[i / ((int64_t)H * W)], len);
  }
}

__global__ __launch_bounds__(256) void cc_filter_kernel(const int* L, const int* area, const int* white, uint8_t* dst, int64_t total,
                                                        int H, int W, int num, int den) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int r = L[i];
    uint8_t v = 0;
    if (r >= 0 && (int64_t)den * area[r] >= (int64_t)num * white[i / ((int64_t)H * W)]) v = 255;
    dst[i] = v;
  }
}

// ---- E4 ------------------------------------------------------------------------------------------------------------------------
// grid (blocks, B): the white pixels of the AND over the R planes of sample b, one global atomicAdd per block
__global__ __launch_bounds__(256) void and_count_kernel(const uint8_t* masks, int R, int HW, int* counts) {
  __shared__ int s_white;
  const int b = blockIdx.y;
  const uint8_t* mb = masks + (int64_t)b * R * HW;
  if (threadIdx.x == 0) s_white = 0;
  __syncthreads();
  int white = 0;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < HW; i += gridDim.x * 256) {
    int v = 1;
    for (int r = 0; r < R; ++r) v &= is_white(mb[(int64_t)r * HW + i]) ? 1 : 0;
    white += v;
  }
  if (white) atomicAdd(&s_white, white);
  __syncthreads();
  if (threadIdx.x == 0 && s_white) atomicAdd(&counts[2 * b], s_white);
}

// grid (blocks, B): 8 x 8 / stride-8 max pool of the AND, floor sizes; counts[2 b] == 0 makes the sample's plane white instead
__global__ __launch_bounds__(256) void and_pool8_kernel(const uint8_t* masks, int R, int H, int W, int h, int w, const int* counts,
                                                        uint8_t* dst) {
  const int b = blockIdx.y;
  const int64_t HW = (int64_t)H * W;
  const uint8_t* mb = masks + (int64_t)b * R * HW;
  const bool all_white = counts[2 * b] == 0;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < h * w; i += gridDim.x * 256) {
    const int oy = i / w, ox = i - oy * w;
    int any = all_white ? 1 : 0;
    for (int dy = 0; dy < 8 && !any; ++dy)
      for (int dx = 0; dx < 8; ++dx) {
        const int64_t p = (int64_t)(oy * 8 + dy) * W + ox * 8 + dx;
        int v = 1;
        for (int r = 0; r < R; ++r) v &= is_white(mb[(int64_t)r * HW + p]) ? 1 : 0;
        any |= v;
      }
    dst[(int64_t)b * h * w + i] = any ? 255 : 0;
  }
}

// a labelling that reached a bound upstream (status word != 0) makes every count -1: the one read-back carries it to the host
__global__ __launch_bounds__(256) void poison_counts_kernel(const int* status, int* counts, int B) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b < B && *status != 0) counts[2 * b] = counts[2 * b + 1] = -1;
}

// ---- E5 ------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void weight_fill_kernel(const uint8_t* mask, const float* w, float* dst, int64_t total, int hw) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256)
    dst[i] = is_white(mask[i]) ? w[i / hw] : 1.0f;
}

// the sizes every entry here takes: 1 <= H, W <= 4096 and N * H * W < 2^31
inline bool sizes_ok(int64_t N, int H, int W) {
  return N >= 1 && H >= 1 && W >= 1 && H <= FK_EDIT_MASK_MAX_SIDE && W <= FK_EDIT_MASK_MAX_SIDE && N * H * W < ((int64_t)1 << 31);
}

int close5_launch(const uint8_t* src, uint8_t* dst, int64_t N, int H, int W, int* counts, hipStream_t s) {
  const int tiles_y = (H + TILE - 1) / TILE, tiles_x = (W + TILE - 1) / TILE;
  const int64_t tiles = N * tiles_y * tiles_x;
  const int grid = (int)(tiles < 65536 ? tiles : 65536);
  hipLaunchKernelGGL(close5_kernel, dim3(grid), dim3(256), 0, s, src, dst, tiles, tiles_y, tiles_x, H, W, counts);
  return grid;
}

}  // namespace

extern "C" int fk_edit_diff_mask_u8(const void* ref, int64_t ref_batch_stride, const void* tgt, void* dst, int32_t N, int32_t H,
                                    int32_t W, int32_t threshold, fk_stream_t stream_) {
  FK_CHECK_ARG(ref && tgt && dst, "fk_edit_diff_mask_u8: bad arguments");
  FK_CHECK_ARG(sizes_ok(N, H, W), "fk_edit_diff_mask_u8: %d planes of %d x %d: sides are 1..%d and N * H * W < 2^31", N, H, W,
               FK_EDIT_MASK_MAX_SIDE);
  FK_CHECK_ARG(threshold >= 0 && threshold <= 256, "fk_edit_diff_mask_u8: threshold=%d is outside [0, 256]", threshold);
  FK_CHECK_ARG(ref_batch_stride >= (int64_t)H * W * 3, "fk_edit_diff_mask_u8: ref_batch_stride=%lld is less than a picture's %lld bytes",
               (long long)ref_batch_stride, (long long)H * W * 3);
  FK_CHECK_ARG(dst != ref && dst != tgt, "fk_edit_diff_mask_u8: dst must be a buffer of its own");
  const int64_t total = (int64_t)N * H * W;
  hipLaunchKernelGGL(diff_mask_kernel, dim3(ew_grid(total)), dim3(256), 0, (hipStream_t)stream_, (const uint8_t*)ref,
                     ref_batch_stride, (const uint8_t*)tgt, (uint8_t*)dst, total, (int64_t)H * W, threshold);
  FK_CHECK_LAUNCH("fk_edit_diff_mask_u8");
  return FK_OK;
}

extern "C" int fk_mask_close5_u8(const void* src, void* dst, int32_t N, int32_t H, int32_t W, fk_stream_t stream_) {
  FK_CHECK_ARG(src && dst, "fk_mask_close5_u8: bad arguments");
  FK_CHECK_ARG(sizes_ok(N, H, W), "fk_mask_close5_u8: %d planes of %d x %d: sides are 1..%d and N * H * W < 2^31", N, H, W,
               FK_EDIT_MASK_MAX_SIDE);
  FK_CHECK_ARG(dst != src, "fk_mask_close5_u8: dst must be a buffer of its own");
  close5_launch((const uint8_t*)src, (uint8_t*)dst, N, H, W, nullptr, (hipStream_t)stream_);
  FK_CHECK_LAUNCH("fk_mask_close5_u8");
  return FK_OK;
}

extern "C" int64_t fk_mask_components_ws_bytes(int32_t N, int32_t H, int32_t W) {
  if (!sizes_ok(N, H, W)) return 0;
  return 4 * (1 + (int64_t)N + 2 * (int64_t)N * H * W);
}

extern "C" int fk_mask_filter_components_u8(const void* src, void* dst, int32_t N, int32_t H, int32_t W, int32_t keep_num,
                                            int32_t keep_den, int32_t* ws, int64_t ws_bytes, fk_stream_t stream_) {
  FK_CHECK_ARG(src && dst && ws, "fk_mask_filter_components_u8: bad arguments");
  FK_CHECK_ARG(sizes_ok(N, H, W), "fk_mask_filter_components_u8: %d planes of %d x %d: sides are 1..%d and N * H * W < 2^31", N, H, W,
               FK_EDIT_MASK_MAX_SIDE);
  FK_CHECK_ARG(keep_num >= 0 && keep_den >= 1, "fk_mask_filter_components_u8: keep %d / %d is no fraction >= 0", keep_num, keep_den);
  FK_CHECK_ARG(ws_bytes >= fk_mask_components_ws_bytes(N, H, W),
               "fk_mask_filter_components_u8: workspace of %lld bytes, needs fk_mask_components_ws_bytes() = %lld", (long long)ws_bytes,
               (long long)fk_mask_components_ws_bytes(N, H, W));
  FK_CHECK_ARG((uintptr_t)ws % 4 == 0, "fk_mask_filter_components_u8: alignment");
  FK_CHECK_ARG((const void*)ws != src && (void*)ws != dst, "fk_mask_filter_components_u8: ws must be a buffer of its own");
  const int64_t total = (int64_t)N * H * W;
  int* status = ws;
  int* white = ws + 1;
  int* L = ws + 1 + N;
  int* area = L + total;
  const dim3 grid(ew_grid(total)), block(256);
  hipStream_t s = (hipStream_t)stream_;
  if (hipMemsetAsync(ws, 0, 4 * (1 + (size_t)N), s) != hipSuccess) {
    fk_set_error("fk_mask_filter_components_u8: cannot clear the workspace: %s", hipGetErrorString(hipGetLastError()));
    return FK_ELAUNCH;
  }
  hipLaunchKernelGGL(cc_init_kernel, grid, block, 0, s, (const uint8_t*)src, L, area, total, W);
  hipLaunchKernelGGL(cc_merge_kernel, grid, block, 0, s, (const uint8_t*)src, L, total, H, W, status);
  hipLaunchKernelGGL(cc_flatten_kernel, grid, block, 0, s, L, total, H, W, status);
  hipLaunchKernelGGL(cc_count_kernel, grid, block, 0, s, (const int*)L, area, white, total, H, W);
  hipLaunchKernelGGL(cc_filter_kernel, grid, block, 0, s, (const int*)L, (const int*)area, (const int*)white, (uint8_t*)dst, total, H,
                     W, keep_num, keep_den);
  FK_CHECK_LAUNCH("fk_mask_filter_components_u8");
  return FK_OK;
}

extern "C" int fk_mask_components_status(const int32_t* ws, fk_stream_t stream_) {
  FK_CHECK_ARG(ws && (uintptr_t)ws % 4 == 0, "fk_mask_components_status: bad arguments");
  int32_t word = 0;
  hipError_t e = hipMemcpyAsync(&word, ws, 4, hipMemcpyDeviceToHost, (hipStream_t)stream_);
  if (e == hipSuccess) e = hipStreamSynchronize((hipStream_t)stream_);
  if (e != hipSuccess) {
    fk_set_error("fk_mask_components_status: cannot read the status word: %s", hipGetErrorString(e));
    return FK_ELAUNCH;
  }
  if (word != 0) {
    fk_set_error("fk_mask_components_status: a root chase or a union of fk_mask_filter_components_u8 reached its bound of H * W steps");
    return FK_EBOUND;
  }
  return FK_OK;
}

extern "C" int fk_mask_and_pool8_u8(const void* masks, int32_t B, int32_t R, int32_t H, int32_t W, void* pooled, void* mask_ds,
                                    int32_t* counts, const int32_t* status, fk_stream_t stream_) {
  FK_CHECK_ARG(masks && pooled && mask_ds && counts && R >= 1, "fk_mask_and_pool8_u8: bad arguments");
  FK_CHECK_ARG(sizes_ok((int64_t)B * R, H, W) && B >= 1 && H >= 8 && W >= 8,
               "fk_mask_and_pool8_u8: %d x %d planes of %d x %d: sides are 8..%d and B * R * H * W < 2^31", B, R, H, W,
               FK_EDIT_MASK_MAX_SIDE);
  FK_CHECK_ARG(B <= 65535, "fk_mask_and_pool8_u8: a batch of %d is more than 65535", B);
  FK_CHECK_ARG((uintptr_t)counts % 4 == 0 && (uintptr_t)status % 4 == 0, "fk_mask_and_pool8_u8: alignment");
  FK_CHECK_ARG(pooled != mask_ds && pooled != masks && mask_ds != masks && (void*)counts != pooled && (void*)counts != mask_ds,
               "fk_mask_and_pool8_u8: pooled and mask_ds must be buffers of their own");
  const int h = H / 8, w = W / 8;
  hipStream_t s = (hipStream_t)stream_;
  if (hipMemsetAsync(counts, 0, 8 * (size_t)B, s) != hipSuccess) {
    fk_set_error("fk_mask_and_pool8_u8: cannot clear the counts: %s", hipGetErrorString(hipGetLastError()));
    return FK_ELAUNCH;
  }
  hipLaunchKernelGGL(and_count_kernel, dim3(ew_grid((int64_t)H * W), B), dim3(256), 0, s, (const uint8_t*)masks, R, H * W, counts);
  hipLaunchKernelGGL(and_pool8_kernel, dim3(ew_grid((int64_t)h * w), B), dim3(256), 0, s, (const uint8_t*)masks, R, H, W, h, w,
                     (const int*)counts, (uint8_t*)pooled);
  close5_launch((const uint8_t*)pooled, (uint8_t*)mask_ds, B, h, w, counts, s);
  if (status) hipLaunchKernelGGL(poison_counts_kernel, dim3((B + 255) / 256), dim3(256), 0, s, status, counts, B);
  FK_CHECK_LAUNCH("fk_mask_and_pool8_u8");
  return FK_OK;
}

extern "C" int fk_mask_weight_fill_f32(const void* mask_ds, const float* w, float* dst, int32_t B, int32_t h, int32_t wd,
                                       fk_stream_t stream_) {
  FK_CHECK_ARG(mask_ds && w && dst, "fk_mask_weight_fill_f32: bad arguments");
  FK_CHECK_ARG(sizes_ok(B, h, wd), "fk_mask_weight_fill_f32: %d planes of %d x %d: sides are 1..%d and B * h * w < 2^31", B, h, wd,
               FK_EDIT_MASK_MAX_SIDE);
  FK_CHECK_ARG((uintptr_t)w % 4 == 0 && (uintptr_t)dst % 4 == 0, "fk_mask_weight_fill_f32: alignment");
  FK_CHECK_ARG((const void*)dst != mask_ds && (const void*)dst != (const void*)w, "fk_mask_weight_fill_f32: dst must be a buffer of its own");
  const int64_t total = (int64_t)B * h * wd;
  hipLaunchKernelGGL(weight_fill_kernel, dim3(ew_grid(total)), dim3(256), 0, (hipStream_t)stream_, (const uint8_t*)mask_ds, w, dst,
                     total, h * wd);
  FK_CHECK_LAUNCH("fk_mask_weight_fill_f32");
  return FK_OK;
}
