// Step cache (residual caching across denoise steps, pipeline.py / step_cache.py): the measure and the two residual passes.
// Four HBM-bound kernels over bf16 [B, R, D] views with contiguous rows, a row stride and a batch stride of their own
// (fk_rows) -- the caller hands over the image part of a joint [B, S_txt + S_img, D] buffer as it is.  The fourth is the
// first-block measure (fk_residual_absdiff_sums_bf16): the residual pass and the sums in one, with the bits of the two.
//
// One decomposition for all of them: a work item is chunk c (elements [8c, 8c + 8) of the row, cut at D) of row m, item
// i = m * cpr + c with cpr = ceil(D / 8); thread g of the grid takes items g, g + T, g + 2T, ... (T = blocks * 256, at most
// SC_MAX_BLOCKS blocks).  A full chunk of a view whose rows are 16-byte aligned is one 16-byte load / store; a cut chunk, or
// any chunk of an unaligned view, goes element by element.  Nothing outside [0, D) of a row is read or written.
//
// The sums have a FIXED order (tests/step_cache_ref.py emulates it and derives the error bound from it):
//   chunk    ((t0 + t1) + (t2 + t3)) + ((t4 + t5) + (t6 + t7)) over the chunk's terms, 0 beyond D            3 additions deep
//   thread   acc += chunk sum, items in increasing order                                                    ceil(N / T)
//   block    LDS halving tree over the 256 accumulators (offsets 128, 64, ..., 1); one partial pair per block          8
//   final    a second launch of ONE block: thread t adds partials t, t + 256, ... in order, then the same tree
// No floating-point atomics and no arrival counters: two launches on the same data give the same bits.
#include "fk_common.h"

namespace {

constexpr int SC_THREADS = 256;
constexpr int SC_MAX_BLOCKS = 1024;

FK_DEV float tree8(const float* t) { return ((t[0] + t[1]) + (t[2] + t[3])) + ((t[4] + t[5]) + (t[6] + t[7])); }

template <bool ALIGNED>
FK_DEV void load_chunk(const bf16_t* row, int c, int D, float* f) {
  if (ALIGNED && c * 8 + 8 <= D) {
    const u32x4_t w = *(const u32x4_t*)(row + c * 8);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      f[2 * e] = bf_lo(w[e]);
      f[2 * e + 1] = bf_hi(w[e]);
    }
  } else {
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int j = c * 8 + e;
      f[e] = j < D ? bf2f(row[j]) : 0.0f;
    }
  }
}

FK_DEV void block_tree(float* sd, float* sb, int t) {
  __syncthreads();
  for (int off = SC_THREADS / 2; off >= 1; off >>= 1) {
    if (t < off) {
      sd[t] += sd[t + off];
      sb[t] += sb[t + off];
    }
    __syncthreads();
  }
}

template <bool ALIGNED>
__global__ __launch_bounds__(SC_THREADS) void absdiff_partials_kernel(const bf16_t* a, fk_rows ra, const bf16_t* b,
                                                                      fk_rows rb, int64_t nitems, int cpr, int D,
                                                                      float* ws) {
  __shared__ float sd[SC_THREADS], sb[SC_THREADS];
  const int t = threadIdx.x;
  float accd = 0.0f, accb = 0.0f;
  for (int64_t i = (int64_t)blockIdx.x * SC_THREADS + t; i < nitems; i += (int64_t)gridDim.x * SC_THREADS) {
    const int64_t m = i / cpr;
    const int c = (int)(i - m * cpr);
    float fa[8], fb[8], td[8], tb[8];
    load_chunk<ALIGNED>(a + fk_row_offset(ra, m), c, D, fa);
    load_chunk<ALIGNED>(b + fk_row_offset(rb, m), c, D, fb);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      td[e] = fabsf(fa[e] - fb[e]);
      tb[e] = fabsf(fb[e]);
    }
    accd += tree8(td);
    accb += tree8(tb);
  }
  sd[t] = accd;
  sb[t] = accb;
  block_tree(sd, sb, t);
  if (t == 0) {
    ws[2 * (int64_t)blockIdx.x] = sd[0];
    ws[2 * (int64_t)blockIdx.x + 1] = sb[0];
  }
}

// The first-block measure as one pass: r = bf16(float(h1) - float(h0)) (residual_kernel<., -1>'s value), optionally stored, then
// the terms |float(r) - float(ref)| and |float(ref)| through absdiff_partials_kernel's decomposition and order -- hence the
// bits of residual_save followed by absdiff_sums.  ALIGNED speaks for every view of the launch, r_out included.
template <bool ALIGNED, bool STORE>
__global__ __launch_bounds__(SC_THREADS) void residual_absdiff_partials_kernel(const bf16_t* h1, fk_rows r1, const bf16_t* h0,
                                                                               fk_rows r0, const bf16_t* ref, fk_rows rf,
                                                                               bf16_t* r_out, fk_rows rr, int64_t nitems,
                                                                               int cpr, int D, float* ws) {
  __shared__ float sd[SC_THREADS], sb[SC_THREADS];
  const int t = threadIdx.x;
  float accd = 0.0f, accb = 0.0f;
  for (int64_t i = (int64_t)blockIdx.x * SC_THREADS + t; i < nitems; i += (int64_t)gridDim.x * SC_THREADS) {
    const int64_t m = i / cpr;
    const int c = (int)(i - m * cpr);
    const bf16_t* xr = h1 + fk_row_offset(r1, m);
    const bf16_t* yr = h0 + fk_row_offset(r0, m);
    float fr[8], fb[8], td[8], tb[8];
    load_chunk<ALIGNED>(ref + fk_row_offset(rf, m), c, D, fb);
    if (ALIGNED && c * 8 + 8 <= D) {
      const u32x4_t xw = *(const u32x4_t*)(xr + c * 8), yw = *(const u32x4_t*)(yr + c * 8);
      u32x4_t ow;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        ow[e] = pack_bf2(bf_lo(xw[e]) - bf_lo(yw[e]), bf_hi(xw[e]) - bf_hi(yw[e]));
        fr[2 * e] = bf_lo(ow[e]);
        fr[2 * e + 1] = bf_hi(ow[e]);
      }
      if (STORE) *(u32x4_t*)(r_out + fk_row_offset(rr, m) + c * 8) = ow;
    } else {
      bf16_t* orow = STORE ? r_out + fk_row_offset(rr, m) : nullptr;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const int j = c * 8 + e;
        fr[e] = 0.0f;
        if (j < D) {
          const bf16_t rv = f2bf(bf2f(xr[j]) - bf2f(yr[j]));
          fr[e] = bf2f(rv);
          if (STORE) orow[j] = rv;
        }
      }
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      td[e] = fabsf(fr[e] - fb[e]);
      tb[e] = fabsf(fb[e]);
    }
    accd += tree8(td);
    accb += tree8(tb);
  }
  sd[t] = accd;
  sb[t] = accb;
  block_tree(sd, sb, t);
  if (t == 0) {
    ws[2 * (int64_t)blockIdx.x] = sd[0];
    ws[2 * (int64_t)blockIdx.x + 1] = sb[0];
  }
}

__global__ __launch_bounds__(SC_THREADS) void absdiff_final_kernel(const float* ws, int nblk, float* out) {
  __shared__ float sd[SC_THREADS], sb[SC_THREADS];
  const int t = threadIdx.x;
  float accd = 0.0f, accb = 0.0f;
  for (int j = t; j < nblk; j += SC_THREADS) {
    accd += ws[2 * j];
    accb += ws[2 * j + 1];
  }
  sd[t] = accd;
  sb[t] = accb;
  block_tree(sd, sb, t);
  if (t == 0) {
    out[0] = sd[0];
    out[1] = sb[0];
  }
}

// o = bf16(float(x) + SIGN * float(y)); o may be x itself (every element is read and written by one thread)
template <bool ALIGNED, int SIGN>
__global__ __launch_bounds__(SC_THREADS) void residual_kernel(const bf16_t* x, fk_rows rx, const bf16_t* y, fk_rows ry,
                                                              bf16_t* o, fk_rows ro, int64_t nitems, int cpr, int D) {
  for (int64_t i = (int64_t)blockIdx.x * SC_THREADS + threadIdx.x; i < nitems; i += (int64_t)gridDim.x * SC_THREADS) {
    const int64_t m = i / cpr;
    const int c = (int)(i - m * cpr);
    const bf16_t* xr = x + fk_row_offset(rx, m);
    const bf16_t* yr = y + fk_row_offset(ry, m);
    bf16_t* orow = o + fk_row_offset(ro, m);
    if (ALIGNED && c * 8 + 8 <= D) {
      const u32x4_t xw = *(const u32x4_t*)(xr + c * 8), yw = *(const u32x4_t*)(yr + c * 8);
      u32x4_t ow;
#pragma unroll
      for (int e = 0; e < 4; ++e)
        ow[e] = SIGN > 0 ? pack_bf2(bf_lo(xw[e]) + bf_lo(yw[e]), bf_hi(xw[e]) + bf_hi(yw[e]))
                         : pack_bf2(bf_lo(xw[e]) - bf_lo(yw[e]), bf_hi(xw[e]) - bf_hi(yw[e]));
      *(u32x4_t*)(orow + c * 8) = ow;
    } else {
      for (int j = c * 8; j < D && j < c * 8 + 8; ++j) {
        const float xv = bf2f(xr[j]), yv = bf2f(yr[j]);
        orow[j] = f2bf(SIGN > 0 ? xv + yv : xv - yv);
      }
    }
  }
}

// ---- host side -----------------------------------------------------------------------------------------------------
bool rows_ok(const fk_rows& r, int D) {
  if (r.ld < D) return false;
  return r.rows_per_batch <= 0 || r.batch_stride >= 0;
}
// rows of an OUTPUT must not overlap one another
bool rows_disjoint(const fk_rows& r, int D) {
  return r.rows_per_batch <= 0 || r.batch_stride >= (r.rows_per_batch - 1) * r.ld + D;
}
bool aligned16(const void* p, const fk_rows& r) {
  return (uintptr_t)p % 16 == 0 && r.ld % 8 == 0 && (r.rows_per_batch <= 0 || r.batch_stride % 8 == 0);
}
// [lo, hi): the bytes from a view's first element to the end of its last row (strides are >= 0: the last row is the farthest)
struct Span { uintptr_t lo, hi; };
Span span_of(const void* p, const fk_rows& r, int64_t M, int D) {
  const uintptr_t lo = (uintptr_t)p;
  int64_t last = (M - 1) * r.ld;                       // fk_row_offset(r, M - 1), on the host
  if (r.rows_per_batch > 0) {
    const int64_t b = (M - 1) / r.rows_per_batch;
    last = b * r.batch_stride + (M - 1 - b * r.rows_per_batch) * r.ld;
  }
  return Span{lo, lo + (uintptr_t)(last + D) * sizeof(bf16_t)};
}
bool overlap(const Span& a, const Span& b) { return a.lo < b.hi && b.lo < a.hi; }
bool same_view(const void* p, const fk_rows& r, const void* q, const fk_rows& s) {
  return p == q && r.ld == s.ld && r.rows_per_batch == s.rows_per_batch && (r.rows_per_batch <= 0 || r.batch_stride == s.batch_stride);
}
int grid_of(int64_t nitems) {
  const int64_t g = (nitems + SC_THREADS - 1) / SC_THREADS;
  return (int)(g < SC_MAX_BLOCKS ? g : SC_MAX_BLOCKS);
}

// out = x + sign * y over the views; `alias_x`: out may be x itself
int residual_launch(const char* name, const void* x, const fk_rows& rx, const void* y, const fk_rows& ry, void* o,
                    const fk_rows& ro, int64_t M, int32_t D, int32_t is_bf16, int sign, bool alias_x, hipStream_t stream) {
  FK_CHECK_ARG(x && y && o, "%s: NULL pointer", name);
  FK_CHECK_ARG(M >= 1 && D >= 1, "%s: needs M >= 1 rows of D >= 1 elements (M = %lld, D = %d)", name, (long long)M, D);
  if (!is_bf16) {
    fk_set_error("%s: bf16 views only", name);
    return FK_EUNSUPPORTED;
  }
  FK_CHECK_ARG(rows_ok(rx, D) && rows_ok(ry, D) && rows_ok(ro, D), "%s: a row stride below D = %d (or a negative batch stride)", name, D);
  FK_CHECK_ARG(rows_disjoint(ro, D), "%s: the output's rows overlap", name);
  const Span sx = span_of(x, rx, M, D), sy = span_of(y, ry, M, D), so = span_of(o, ro, M, D);
  const bool aliased = alias_x && same_view(x, rx, o, ro);
  FK_CHECK_ARG(!overlap(sx, sy), "%s: the two inputs overlap", name);
  FK_CHECK_ARG(!overlap(so, sy) && (aliased || !overlap(so, sx)),
               "%s: the output overlaps an input%s", name, alias_x ? " (it may only BE the first one, same strides)" : "");
  const int cpr = (D + 7) / 8;
  const int64_t nitems = M * cpr;
  const bool al = aligned16(x, rx) && aligned16(y, ry) && aligned16(o, ro);
  const dim3 grid(grid_of(nitems)), block(SC_THREADS);
#define FK_SC_LAUNCH(AL, SG)                                                                                       \
  hipLaunchKernelGGL((residual_kernel<AL, SG>), grid, block, 0, stream, (const bf16_t*)x, rx, (const bf16_t*)y, ry, \
                     (bf16_t*)o, ro, nitems, cpr, (int)D)
  if (al && sign > 0) FK_SC_LAUNCH(true, 1);
  else if (al) FK_SC_LAUNCH(true, -1);
  else if (sign > 0) FK_SC_LAUNCH(false, 1);
  else FK_SC_LAUNCH(false, -1);
#undef FK_SC_LAUNCH
  FK_CHECK_LAUNCH(name);
  return FK_OK;
}

}  // namespace

extern "C" int64_t fk_absdiff_ws_floats(void) { return 2 * SC_MAX_BLOCKS; }

extern "C" int fk_absdiff_sums_bf16(const void* a, fk_rows ra, const void* b, fk_rows rb, int64_t M, int32_t D,
                                    int32_t is_bf16, float* out, float* ws, int64_t ws_floats, fk_stream_t stream) {
  FK_CHECK_ARG(a && b && out && ws, "fk_absdiff_sums_bf16: NULL pointer");
  FK_CHECK_ARG(M >= 1 && D >= 1, "fk_absdiff_sums_bf16: needs M >= 1 rows of D >= 1 elements (M = %lld, D = %d)", (long long)M, D);
  if (!is_bf16) {
    fk_set_error("fk_absdiff_sums_bf16: bf16 views only");
    return FK_EUNSUPPORTED;
  }
  FK_CHECK_ARG(rows_ok(ra, D) && rows_ok(rb, D), "fk_absdiff_sums_bf16: a row stride below D = %d (or a negative batch stride)", D);
  const int cpr = (D + 7) / 8;
  const int64_t nitems = M * cpr;
  const int nblk = grid_of(nitems);
  FK_CHECK_ARG(ws_floats >= 2 * (int64_t)nblk, "fk_absdiff_sums_bf16: the workspace holds %lld floats, %d blocks need %d",
               (long long)ws_floats, nblk, 2 * nblk);
  const hipStream_t st = (hipStream_t)stream;
  if (aligned16(a, ra) && aligned16(b, rb))
    hipLaunchKernelGGL(absdiff_partials_kernel<true>, dim3(nblk), dim3(SC_THREADS), 0, st, (const bf16_t*)a, ra,
                       (const bf16_t*)b, rb, nitems, cpr, (int)D, ws);
  else
    hipLaunchKernelGGL(absdiff_partials_kernel<false>, dim3(nblk), dim3(SC_THREADS), 0, st, (const bf16_t*)a, ra,
                       (const bf16_t*)b, rb, nitems, cpr, (int)D, ws);
  FK_CHECK_LAUNCH("fk_absdiff_sums_bf16");
  hipLaunchKernelGGL(absdiff_final_kernel, dim3(1), dim3(SC_THREADS), 0, st, (const float*)ws, nblk, out);
  FK_CHECK_LAUNCH("fk_absdiff_sums_bf16 (final)");
  return FK_OK;
}

extern "C" int fk_residual_absdiff_sums_bf16(const void* h1, fk_rows r1, const void* h0, fk_rows r0, const void* ref, fk_rows rf,
                                             void* r_out, fk_rows rr, int64_t M, int32_t D, int32_t is_bf16, float* out,
                                             float* ws, int64_t ws_floats, fk_stream_t stream) {
  const char* name = "fk_residual_absdiff_sums_bf16";
  FK_CHECK_ARG(h1 && h0 && ref && out && ws, "%s: NULL pointer", name);
  FK_CHECK_ARG(M >= 1 && D >= 1, "%s: needs M >= 1 rows of D >= 1 elements (M = %lld, D = %d)", name, (long long)M, D);
  if (!is_bf16) {
    fk_set_error("%s: bf16 views only", name);
    return FK_EUNSUPPORTED;
  }
  FK_CHECK_ARG(rows_ok(r1, D) && rows_ok(r0, D) && rows_ok(rf, D) && (!r_out || rows_ok(rr, D)),
               "%s: a row stride below D = %d (or a negative batch stride)", name, D);
  if (r_out) {
    FK_CHECK_ARG(rows_disjoint(rr, D), "%s: r_out's rows overlap", name);
    const Span so = span_of(r_out, rr, M, D);
    FK_CHECK_ARG(!overlap(so, span_of(h1, r1, M, D)) && !overlap(so, span_of(h0, r0, M, D)) && !overlap(so, span_of(ref, rf, M, D)),
                 "%s: r_out overlaps an input", name);
  }
  const int cpr = (D + 7) / 8;
  const int64_t nitems = M * cpr;
  const int nblk = grid_of(nitems);
  FK_CHECK_ARG(ws_floats >= 2 * (int64_t)nblk, "%s: the workspace holds %lld floats, %d blocks need %d", name,
               (long long)ws_floats, nblk, 2 * nblk);
  const hipStream_t st = (hipStream_t)stream;
  const bool al = aligned16(h1, r1) && aligned16(h0, r0) && aligned16(ref, rf) && (!r_out || aligned16(r_out, rr));
  const dim3 grid(nblk), block(SC_THREADS);
#define FK_SC_LAUNCH(AL, ST)                                                                                              \
  hipLaunchKernelGGL((residual_absdiff_partials_kernel<AL, ST>), grid, block, 0, st, (const bf16_t*)h1, r1, (const bf16_t*)h0, \
                     r0, (const bf16_t*)ref, rf, (bf16_t*)r_out, rr, nitems, cpr, (int)D, ws)
  if (al && r_out) FK_SC_LAUNCH(true, true);
  else if (al) FK_SC_LAUNCH(true, false);
  else if (r_out) FK_SC_LAUNCH(false, true);
  else FK_SC_LAUNCH(false, false);
#undef FK_SC_LAUNCH
  FK_CHECK_LAUNCH(name);
  hipLaunchKernelGGL(absdiff_final_kernel, dim3(1), dim3(SC_THREADS), 0, st, (const float*)ws, nblk, out);
  FK_CHECK_LAUNCH("fk_residual_absdiff_sums_bf16 (final)");
  return FK_OK;
}

extern "C" int fk_residual_save_bf16(const void* h_out, fk_rows ro, const void* h0, fk_rows r0, void* r, fk_rows rr, int64_t M,
                                     int32_t D, int32_t is_bf16, fk_stream_t stream) {
  return residual_launch("fk_residual_save_bf16", h_out, ro, h0, r0, r, rr, M, D, is_bf16, -1, false, (hipStream_t)stream);
}

extern "C" int fk_residual_apply_bf16(const void* h0, fk_rows r0, const void* r, fk_rows rr, void* out, fk_rows ro, int64_t M,
                                      int32_t D, int32_t is_bf16, fk_stream_t stream) {
  return residual_launch("fk_residual_apply_bf16", h0, r0, r, rr, out, ro, M, D, is_bf16, +1, true, (hipStream_t)stream);
}
