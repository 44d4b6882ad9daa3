/*
 * fk.h -- C ABI of libfk.so: the MI355X (gfx950) native FLUX-Kontext denoiser hot path.
 *
 * Drop-in boundary.  The reference (wyhlovecpp/GPT-Image-Edit) is 100 %
 * Python and reaches this arithmetic through torch/diffusers module calls; it has no FFI of its
 * own.  Each entry point below therefore names the reference call site / third-party module whose
 * device work it replaces.  A Python maintainer binds these with ctypes (INTEGRATION.md shows the
 * stub); nothing here mentions torch types: plain device pointers (from tensor.data_ptr()),
 * integer sizes/strides in ELEMENTS, scalars, and the hipStream_t to enqueue on.
 *
 * Conventions
 *   - every function returns 0 on success or a negative FK_E* code; fk_last_error() returns a
 *     thread-local message for the last failure.  Nothing throws across the ABI.
 *   - all work is stream-ordered on `stream`; no function synchronises the device or allocates
 *     device memory: the caller (PyTorch caching allocator) owns every buffer incl. workspaces.
 *   - bf16 buffers are raw uint16 storage (torch.bfloat16), row-major, inner dimension contiguous
 *     and 16-byte aligned unless a stride parameter says otherwise.
 *   - re-entrant; no global mutable state.
 */
#ifndef FK_H_
#define FK_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* fk_stream_t; /* hipStream_t */

enum {
  FK_OK = 0,
  FK_EINVAL = -1,  /* bad shape / alignment / null pointer */
  FK_EUNSUPPORTED = -2,
  FK_ELAUNCH = -3, /* hipLaunch / runtime error */
  FK_EBOUND = -4,  /* a device loop reached the bound its plane size gives it (fk_mask_components_status) */
};

/* Epilogues of fk_gemm_bf16 (applied in this order; every stage rounds to bf16 exactly where the
 * reference's bf16 torch graph does):
 *   y = bf16(acc + bias)                                   (nn.Linear output)
 *   FK_EPI_GELU_TANH : y = bf16(gelu_tanh(y))              (FeedForward "gelu-approximate")
 *   FK_EPI_SILU      : y = bf16(silu(y))                   (TimestepEmbedding / PixArtAlphaTextProjection)
 *   FK_EPI_GATE_RES  : y = bf16(res + bf16(gate[b] * y))   (gate_msa.unsqueeze(1) * attn_out; h + ...)
 *   FK_EPI_RES       : y = bf16(res + y)                   (ResnetBlock2D / VAE attention residual)
 *   FK_EPI_SCALE     : y = bf16(alpha * acc)  (no bias)    (attention scores for the VAE mid block)
 *   FK_EPI_QKV       : fused QKV projection of FluxAttnProcessor2_0 (N = 3*H*128 = q | k | v, or 2*H*128 = q | k): the q and k
 *                      thirds get per-head RMSNorm(eps 1e-6, weight) + interleaved RoPE and are written
 *                      head-major to q_out / k_out [B, H, S_total, 128]; the v third is stored like
 *                      FK_EPI_NONE into C (= the qkv buffer the attention kernel reads V from).
 */
enum {
  FK_EPI_NONE = 0,
  FK_EPI_GELU_TANH = 1,
  FK_EPI_SILU = 2,
  FK_EPI_GATE_RES = 3,
  FK_EPI_RES = 4,
  FK_EPI_SCALE = 5,
  FK_EPI_QKV = 6,
};

/* Row addressing used for A, C and the residual: logical row m lives at
 *   base + (m / rows_per_batch) * batch_stride + (m % rows_per_batch) * ld        (elements)
 * so that the text / image streams of a double block can read from and write into slices of one
 * joint [B, S, *] buffer without copies.  rows_per_batch <= 0 means "one batch" (offset = m*ld). */
typedef struct fk_rows {
  int64_t ld;
  int64_t rows_per_batch;
  int64_t batch_stride;
} fk_rows;

/* C[M,N] = epilogue(A[M,K] . W[N,K]^T + bias[N]);  A, W bf16 K-contiguous; fp32 accumulation on MFMA.
 * Replaces every nn.Linear of FluxTransformer2DModel / FeedForward / AutoencoderKL.Attention
 * (diffusers 0.32.2; reached from reference univa/utils/flux_pipeline.py:1067-1077).
 * K % 64 == 0, ldw % 8 == 0, A/W/C row starts 16-byte aligned.  N % 8 == 0 unless out_fp32. */
typedef struct fk_gemm_args {
  const void* A; fk_rows a;
  const void* W; int64_t ldw;
  const void* bias;              /* bf16 [N] or NULL */
  void* C; fk_rows c;            /* bf16, or fp32 when out_fp32 (debug/parity: acc + bias only; out_fp32 = 1: the 128 x 128
                                  * register-staged kernel, 2: the large-tile kernels' own main loops -- 256 x 256, 256 x 128,
                                  * mixed grid, split-K pairs, as the launch plan / fk_gemm_set_variant selects) */
  const void* res; fk_rows r;    /* FK_EPI_GATE_RES / FK_EPI_RES */
  const void* gate;              /* bf16, gate row b at gate + b*gate_batch_stride; b = m / gate_rows_per_batch */
  int64_t gate_batch_stride;
  int64_t gate_rows_per_batch;
  int32_t M, N, K;
  int32_t epilogue;
  int32_t out_fp32;
  float alpha;                   /* FK_EPI_SCALE */
  /* FK_EPI_QKV only (row m of this problem is token s = qkv_s_offset + m % c.rows_per_batch of batch
   * m / c.rows_per_batch; c.rows_per_batch <= 0: one batch): */
  void* q_out; void* k_out;      /* bf16 [B, H, S_total, 128] */
  const void* wq; const void* wk;/* bf16 [128] RMSNorm weights of this stream (norm_q/norm_k or norm_added_*) */
  const float* rope_cs;          /* fp32 [S_total, 64, 2]: (cos, sin) of every rotary pair (FluxPosEmbed repeats each
                                  * value over the two columns of its pair, so the [S,128] cos / sin tables hold
                                  * every number twice; the epilogue reads 512 B per token row instead of 1 KiB) */
  /* Optional split-K workspace (caller-owned, one per stream that issues GEMMs): splitk_slots x 256 KiB of fp32 partial
   * tiles followed by splitk_slots x 2 uint32 control words, the control words zeroed ONCE at allocation (a counter and a
   * flag, each moved by exactly 4 per use of the slot afterwards: never reset, wrap-safe).  With it, a K >= 6144 GEMM whose 256 x 256 tiling fills at most half the CUs runs
   * as two half-K workgroups per tile (deterministic: the two fp32 partials are added once, and fp32 addition
   * commutes).  NULL: never split.  Launches that share a workspace must be ordered (same stream). */
  void* splitk_ws;
  int32_t qkv_s_offset, qkv_s_total, qkv_heads;
  int32_t splitk_slots;
  /* Operand layout (the backward pass's operands as they lie in memory; reference: autograd through nn.Linear,
   * train_denoiser.py:1172):  0 = A [M, K], W [N, K] (above);  1 = W is [K, N] (ldw = its row stride): the data gradient
   * dX = dY W reads the weight as stored;  2 = A is [K, M] as well (a = its K rows, uniformly strided): the weight
   * gradient dW = dY^T X reads both operands token-major.  1 / 2: N % 256 == 0, K % 64 == 0, epilogue none (1: also
   * FK_EPI_RES), 2: M % 256 == 0; same sums, bit for bit, as layout 0 on transposed copies. */
  int32_t layout;
  int32_t f32_flags;         /* out_fp32 = 1 only: bit 0 = bias is fp32 [N]; bit 1 = `res` is an fp32 tensor (rows r) added to C */
  /* Launch controls of the large-tile kernels -- PER CALL: the library keeps no mutable launch state (round 5; rounds 2-4 had
   * process-wide fk_gemm_set_* hooks).  All zero = the defaults.  A grouped launch takes them from its first problem.
   *   variant : 0 = the launch plan chooses per problem; 128 = 256 x 128 tiles, 256 = 256 x 256 tiles, 384 = mixed grid,
   *             512 = split-K pairs, 640 = stream-K ranges -- forced where the form applies (tests, measurement).
   *   plan    : 0 = default (mixed grids and split-K pairs allowed); otherwise FK_GEMM_PLAN_EXPLICIT | allow-bits: bit 0 mixed
   *             grids (bit-identical results), bit 1 split-K pairs (results differ in the last bits from the unsplit sum: with
   *             bit 1 clear a sample's result does not depend on the grid it runs in -- "batch-invariant"), bit 2 stream-K
   *             ranges for long-K launches with a poorly filled last round (measured slower inside the edits: off by default);
   *             optionally one FK_GEMM_PLAN_SPLITK_* bit (below): the exchange of the split-K pairs; optionally
   *             FK_GEMM_PLAN_TILE_PER_WG / FK_GEMM_PLAN_WALK / FK_GEMM_PLAN_WALK_CAP(G) (below): the tile walk.
   *   group_m : 0 = default (8): depth in row tiles of the grouped tile order; >= the row-tile count: every XCD owns a column
   *             range.  Results do not depend on it.
   *   mfma    : 0 = default (16); 16 = v_mfma_f32_16x16x32_bf16, 32 = v_mfma_f32_32x32x16_bf16 (the two differ in the last
   *             bits; every launch form of ONE shape agrees bit for bit with the others).  Layouts 1 / 2 follow it too (round 6; rounds 3-5: always 32). */
  int32_t variant, plan, group_m, mfma;
  /* OUT, optional (NULL: not wanted): which launch form this call used -- 128 = 256 x 128 tiles, 256 = 256 x 256, 384 = mixed
   * grid, 512 = split-K pairs of 256 x 256 tiles, 640 = stream-K ranges, 0 = none of the large-tile kernels (the 128 x 128
   * register-staged kernel).  Written by the host code of the call before it returns (tests, profiling); a grouped launch
   * writes through its first problem's pointer.  Replaces the thread-local fk_gemm_last_variant() of rounds 2-5. */
  int32_t* variant_used;
} fk_gemm_args;
#define FK_GEMM_PLAN_EXPLICIT 8
#define FK_GEMM_PLAN_BATCH_INVARIANT (FK_GEMM_PLAN_EXPLICIT | 1)   /* mixed grids only: no K split of any kind */
/* How the two workgroups of a split-K pair (variant 512) exchange their fp32 partial tiles; at most one bit, with
 * FK_GEMM_PLAN_EXPLICIT; none = the built default.  Every form gives the same bits (fp32 own + other commutes).
 *   WHOLE       : the first to finish writes its whole tile and exits, the second adds it and runs the whole epilogue.
 *   SYMMETRIC   : each writes the 128 rows the other finishes and finishes its own 128 -- where both workgroups are known to be
 *                 on the chip when the first is done; a pair of which one is not falls back to WHOLE by itself.
 *   UNANNOUNCED : tests only -- SYMMETRIC taking its decisions as if the partner had never been seen on the chip: the fallback. */
#define FK_GEMM_PLAN_SPLITK_WHOLE 16
#define FK_GEMM_PLAN_SPLITK_SYMMETRIC 32
#define FK_GEMM_PLAN_SPLITK_UNANNOUNCED 64
/* Tile walk (with FK_GEMM_PLAN_EXPLICIT): a 256 x 256 or mixed grid with more tiles than workgroups may run as one workgroup
 * per CU, each walking tiles g, g + G, ... of the launch's tile order with the next tile's first operands requested in front
 * of the current tile's epilogue.  Same bits as one workgroup per tile; variant_used reports 256 / 384 either way.
 *   TILE_PER_WG : never walk -- one workgroup per tile (A/B runs, the reference side of the tests).
 *   WALK        : walk wherever the grid has more tiles than workgroups, also where the built rule would not.
 *   WALK_CAP(G) : at most G workgroups (1 .. 32767; implies WALK); 0 = one per CU. */
#define FK_GEMM_PLAN_TILE_PER_WG 128
#define FK_GEMM_PLAN_WALK 256
#define FK_GEMM_PLAN_WALK_CAP_SHIFT 16
#define FK_GEMM_PLAN_WALK_CAP(G) ((int32_t)(G) << FK_GEMM_PLAN_WALK_CAP_SHIFT)
#define FK_GEMM_PLAN_WALK_BITS (FK_GEMM_PLAN_TILE_PER_WG | FK_GEMM_PLAN_WALK | FK_GEMM_PLAN_WALK_CAP(0x7fff))
#define FK_SPLITK_SLOT_BYTES (256 * 256 * 4 + 8)

int fk_gemm_bf16(const fk_gemm_args* args, fk_stream_t stream);

/* n (<= FK_MAX_GROUP) independent problems that share N, K and the epilogue in ONE launch: the text- and
 * image-stream linears of a FluxTransformerBlock (different weights, different row counts) fill the GPU
 * together.  args is an array of n fk_gemm_args; bf16 output only. */
#define FK_MAX_GROUP 4
int fk_gemm_bf16_grouped(const fk_gemm_args* args, int32_t n, fk_stream_t stream);

/* ---- MXFP8 (OCP MX v1.0, E4M3 elements, E8M0 block scales) -- opt-in inference format of the block GEMMs ---------------
 * A row of K elements is stored as K e4m3fn bytes (x / 2^e, round-to-nearest-even, saturated to +-448) plus K / 32 E8M0
 * scale bytes (2^(byte - 127)), one per block of 32 consecutive elements:  e = max(floor(log2(amax)) - 8, -127);  an all-zero
 * block has scale byte 127 (2^0); a block holding Inf / NaN has scale byte 0xFF and every element 0x7F (both NaN), so a bad
 * activation surfaces as NaN rows.
 *
 * fk_quantize_mxfp8: x bf16 (rows m of M through xr, K contiguous) -> q [M, K] bytes (row m at q + m * ldq) and scales
 * [M, K / 32] bytes (row m at scales + m * ld_scale).  K % 32 == 0, x rows 16-byte aligned, ldq % 16 == 0.  One pass, the
 * same entry point quantizes weights ([N, K], K-contiguous) once at pack time. */
int fk_quantize_mxfp8(const void* x, fk_rows xr, int64_t M, int32_t K, void* q, int64_t ldq, void* scales,
                      int64_t ld_scale, fk_stream_t stream);

/* C = epilogue(sum_k deq(A)[m, k] * deq(W)[n, k] + bias) on v_mfma_scale_f32_16x16x128_f8f6f4 (e4m3 x e4m3), fp32
 * accumulation.  g carries everything of fk_gemm_args except the operands: shapes, bias, C / res / gate / QKV fields,
 * epilogue (FK_EPI_NONE, GELU_TANH, GATE_RES, QKV; g.out_fp32 = 2: fp32(acc + bias), the parity build), g.variant
 * (0 = launch plan, 128 = 256 x 128 tiles, 256 = 256 x 256 tiles, 512 = split-K pairs) and g.variant_used; g.A / g.W / g.a /
 * g.ldw are unused.  The epilogue arithmetic and rounding points are those of fk_gemm_bf16.  K % 128 == 0, N % 256 == 0, any M;
 * operand rows 16-byte aligned (lda8, ldw8 % 16 == 0), scale rows 4-byte aligned (ld scales % 4 == 0).
 *
 * Split-K pairs (variant 512): two workgroups per 256 x 256 tile, each over half of K, which meet through g.splitk_ws /
 * g.splitk_slots -- the workspace of fk_gemm_args, shared with the bf16 GEMMs of the same stream (same control words, each moved
 * by exactly 4 per use of a slot, never reset), one slot per tile, numbered across the problems of a grouped launch.  Epilogues
 * FK_EPI_NONE (bf16 or out_fp32 = 2) and FK_EPI_GATE_RES.  Handing over the workspace is the opt-in: with g.variant = 0 the
 * launch plan takes the form only when g.splitk_ws is non-NULL, g.plan allows bit 1 (0 = default allows it,
 * FK_GEMM_PLAN_BATCH_INVARIANT forbids it), K >= 6144, K / 128 is even, the pairs fit one round of CUs (2 x tiles <= CUs) and
 * tiles <= g.splitk_slots; otherwise -- and always with g.splitk_ws = NULL -- the launches are those of the unsplit plan.  The
 * split sum differs from the unsplit one in the last bits (two fp32 partials added once; every exchange gives the same bits).
 * g.plan is validated as fk_gemm_bf16 validates it (FK_EINVAL otherwise) and may carry one FK_GEMM_PLAN_SPLITK_* exchange bit
 * (default: symmetric).  A forced g.variant = 512 never falls back: another epilogue, K < 6144 or an odd K / 128 return
 * FK_EUNSUPPORTED, a missing workspace or fewer slots than tiles FK_EINVAL, each with an fk_last_error() text. */
typedef struct fk_gemm_mxfp8_args {
  fk_gemm_args g;
  const void* A8; int64_t lda8;            /* e4m3 [M, K]: row m at A8 + m * lda8 bytes */
  const void* A_scale; int64_t lda_scale;  /* E8M0 [M, K / 32] */
  const void* W8; int64_t ldw8;            /* e4m3 [N, K] */
  const void* W_scale; int64_t ldw_scale;  /* E8M0 [N, K / 32] */
} fk_gemm_mxfp8_args;

int fk_gemm_mxfp8(const fk_gemm_mxfp8_args* args, fk_stream_t stream);
/* n (<= FK_MAX_GROUP) problems with identical N, K and epilogue in one launch (the img + txt pairs of a double block). */
int fk_gemm_mxfp8_grouped(const fk_gemm_mxfp8_args* args, int32_t n, fk_stream_t stream);

/* The same GEMM as a PRODUCER of quantized activations: the result, rounded to bf16 where fk_gemm_mxfp8 rounds it, leaves as
 * MXFP8 -- exactly the bytes fk_quantize_mxfp8 gives for fk_gemm_mxfp8's bf16 output, without that output ever being stored
 * (a.g.C / a.g.c are unused).  Epilogues FK_EPI_NONE and FK_EPI_GELU_TANH.  Row m, column n goes to byte
 * Q + m * ldq + col_offset + n and its block's scale to Q_scale + m * ldq_scale + (col_offset + n) / 32: a GEMM can fill a column
 * window of a wider operand (the single block's MLP-up writes columns [D, 5D) of the [M, 5D] operand of proj_out).
 * Q 16-byte aligned, ldq % 16 == 0; Q_scale 4-byte aligned, ldq_scale % 4 == 0; col_offset % 32 == 0; ldq >= col_offset + N,
 * ldq_scale >= (col_offset + N) / 32.  Launch plan, tile widths (a.g.variant / variant_used) and grouping as fk_gemm_mxfp8, without
 * the split-K pairs: a.g.splitk_ws is ignored and a.g.variant = 512 returns FK_EUNSUPPORTED. */
typedef struct fk_gemm_mxfp8_q_args {
  fk_gemm_mxfp8_args a;
  void* Q; int64_t ldq;                    /* e4m3 [M, ldq] */
  void* Q_scale; int64_t ldq_scale;        /* E8M0 [M, ldq_scale] */
  int64_t col_offset;
} fk_gemm_mxfp8_q_args;
int fk_gemm_mxfp8_q(const fk_gemm_mxfp8_q_args* args, fk_stream_t stream);
int fk_gemm_mxfp8_q_grouped(const fk_gemm_mxfp8_q_args* args, int32_t n, fk_stream_t stream);

/* out = LN(x; eps, no affine) * (1 + scale[b]) + shift[b], rows of width D (=3072), bf16 in/out.
 * Rounds like the reference graph: LN -> bf16, (1+scale) -> bf16, product -> bf16, sum -> bf16.
 * Replaces AdaLayerNormZero / AdaLayerNormZeroSingle / AdaLayerNormContinuous / norm2 (+modulate)
 * of diffusers FluxTransformerBlock.
 * Row m of x / out uses fk_rows addressing; scale/shift row b = m / mod_rows_per_batch at
 * base + b * mod_batch_stride. */
int fk_ln_modulate_bf16(const void* x, fk_rows xr, void* out, fk_rows outr, const void* shift,
                        const void* scale, int64_t mod_batch_stride, int64_t mod_rows_per_batch,
                        int64_t M, int32_t D, float eps, fk_stream_t stream);

/* Same, over a joint [text | image] sequence: rows with (m % rows_per_batch) < split use (shift, scale),
 * the others (shift_b, scale_b) -- both AdaLayerNormZero streams of a FluxTransformerBlock in one launch. */
int fk_ln_modulate2_bf16(const void* x, fk_rows xr, void* out, fk_rows outr, const void* shift,
                         const void* scale, const void* shift_b, const void* scale_b, int64_t split,
                         int64_t mod_batch_stride, int64_t mod_rows_per_batch, int64_t M, int32_t D, float eps,
                         fk_stream_t stream);

/* fk_ln_modulate_bf16 / fk_ln_modulate2_bf16 as PRODUCERS of quantized activations: the same statistics, modulation and bf16
 * rounding points, and the bf16 values then stored as MXFP8 -- exactly the bytes fk_quantize_mxfp8 gives for the bf16 output,
 * which is not written.  Outputs are dense, as fk_gemm_mxfp8 addresses an operand: row m of x at q + m * ldq and
 * scales + m * ld_scale.  The joint form gives each stream its own buffers, batch-major: row r < split of batch b at row
 * b * split + r of (q, scales), row r >= split at row b * (mod_rows_per_batch - split) + r - split of (q_b, scales_b).
 * D % 32 == 0 (512, 1024, 3072); q / q_b 16-byte aligned, ldq >= D, ldq % 16 == 0; scales 4-byte aligned, ld_scale >= D / 32,
 * ld_scale % 4 == 0. */
int fk_ln_modulate_mxfp8(const void* x, fk_rows xr, void* q, int64_t ldq, void* scales, int64_t ld_scale, const void* shift,
                         const void* scale, int64_t mod_batch_stride, int64_t mod_rows_per_batch, int64_t M, int32_t D,
                         float eps, fk_stream_t stream);
int fk_ln_modulate2_mxfp8(const void* x, fk_rows xr, void* q, void* scales, void* q_b, void* scales_b, int64_t ldq,
                          int64_t ld_scale, const void* shift, const void* scale, const void* shift_b, const void* scale_b,
                          int64_t split, int64_t mod_batch_stride, int64_t mod_rows_per_batch, int64_t M, int32_t D, float eps,
                          fk_stream_t stream);

/* QKV post-processing of FluxAttnProcessor2_0: per-head RMSNorm(eps, weight) on q and k
 * (text rows s < s_txt use the *_added weights), interleaved-pair RoPE in fp32, and re-layout:
 *   qkv [B, S, 3*H*128] (q | k | v, head-major inside each)  ->  q_out, k_out [B, H, S, 128] bf16.
 * V is NOT copied: fk_attention_fwd_bf16 reads it in place from the qkv buffer.
 * cos/sin: fp32 [S, 128].  head_dim is fixed at 128. */
int fk_qkv_post_bf16(const void* qkv, void* q_out, void* k_out, const void* wq_img, const void* wk_img,
                     const void* wq_txt, const void* wk_txt, const float* cos, const float* sin, int32_t B,
                     int32_t S, int32_t S_txt, int32_t H, float eps, fk_stream_t stream);

/* O = softmax(Q K^T * scale) V, non-causal, no mask (F.scaled_dot_product_attention as called by
 * FluxAttnProcessor2_0).  q, k: [B, H, S, 128] contiguous; v: token s of batch b, head h at
 * v + b*v_batch_stride + s*v_ld + h*128 (e.g. the V third of the qkv buffer: v_ld = 3*H*128);
 * o: rows (b, s) at o + b*o_batch_stride + s*o_ld, head h at column h*128 -> the [B, S, H*128] layout the
 * next Linear consumes (o_ld lets the single block write straight into its [attn | mlp] buffer). */
int fk_attention_fwd_bf16(const void* q, const void* k, const void* v, void* o, int32_t B, int32_t H,
                          int32_t S, int64_t v_ld, int64_t v_batch_stride, int64_t o_ld,
                          int64_t o_batch_stride, float scale, fk_stream_t stream);
/* The same with a caller-owned stream-K workspace (fk_attention_ws_bytes() bytes, 16-byte aligned, zeroed ONCE at
 * allocation: its control words are monotonic tickets afterwards; launches that share it must be ordered, i.e. one
 * workspace per stream; layout: 16 KiB of (ticket, flag) pairs, then one fp32 partial slot per CU) and an optional lse output ([B, H, S] fp32, log2 domain; NULL: none).  With the workspace, a grid
 * that would leave >= 4 % of its rounds of one-workgroup-per-CU idle (B = 1: S = 8704 is 816 blocks = 3.19 rounds,
 * S = 5632 2.06) runs as a PERSISTENT grid: the KV tiles of all (b, h, 256-row block) items are dealt out as equal
 * contiguous ranges, one per CU, and a block whose keys straddle two CUs is finished by whichever arrives second
 * (fp32 partials through the workspace, agent-scope ticket + flag; deterministic: the merge is symmetric).  Where a block's
 * keys are cut depends on the grid, so the choice comes with the call -- `grid`: 0 = as described, -1 = always one workgroup
 * per block ("batch-invariant"; also what ws = NULL gives), >= 2 = a persistent grid of that many workgroups wherever every
 * block is cut at most once (test hook).  The library keeps no launch state. */
int fk_attention_fwd_ws_bf16(const void* q, const void* k, const void* v, void* o, float* lse, int32_t B, int32_t H,
                             int32_t S, int64_t v_ld, int64_t v_batch_stride, int64_t o_ld, int64_t o_batch_stride,
                             float scale, void* ws, int64_t ws_bytes, int32_t grid, fk_stream_t stream);
int64_t fk_attention_ws_bytes(void);

/* fk_attention_fwd_ws_bf16 as a PRODUCER of quantized activations: the same kernel, grid choice (`grid`, ws, ws_bytes: exactly as
 * above) and lse, the output rounded to bf16 as above and then stored as MXFP8 -- exactly the bytes fk_quantize_mxfp8 gives for
 * the bf16 output, which is not written.  The destination is row-split like fk_ln_modulate2_mxfp8's: token s < split of batch b is
 * the dense row b * split + s of (q, scales), token s >= split the dense row b * (S - split) + s - split of (q_b, scales_b); head h
 * fills bytes [128 h, 128 h + 128) of its row (row stride ldq) and scale bytes [4 h, 4 h + 4) (row stride ldq_scale), so a
 * row may be a window of a wider operand (the single block's [M, 5D] operand of proj_out: ldq = 5D).  split = 0 or S: one stream,
 * (q, scales) alone -- q_b / scales_b may be NULL.  0 <= split <= S; q / q_b 16-byte aligned, ldq % 16 == 0, ldq >= H * 128;
 * scales / scales_b 4-byte aligned, ldq_scale % 4 == 0, ldq_scale >= H * 4: a violation is FK_EINVAL before anything is launched.
 * Only the 4-wave kernel has this form: with FK_ATTN_KERNEL=8 in the environment the call returns FK_EUNSUPPORTED. */
typedef struct fk_attn_mx_out {
  void* q; void* scales;           /* stream A: tokens [0, split) */
  void* q_b; void* scales_b;       /* stream B: tokens [split, S) */
  int64_t split;
  int64_t ldq, ldq_scale;          /* bytes per row, both streams */
} fk_attn_mx_out;
int fk_attention_fwd_ws_mxfp8(const void* q, const void* k, const void* v, float* lse, int32_t B, int32_t H, int32_t S,
                              int64_t v_ld, int64_t v_batch_stride, float scale, const fk_attn_mx_out* out, void* ws,
                              int64_t ws_bytes, int32_t grid, fk_stream_t stream);

/* Parity / debug build of the SAME kernel (same tiling, LDS layouts, softmax, key <-> MFMA k-slot binding): the output
 * is fp32 (o_ld / o_batch_stride in fp32 elements, 16-byte aligned) and every probability enters the PV product as
 * two bf16 terms (hi + lo), so the result can be compared with an fp32 reference at the tolerance BASELINE.json
 * states (rtol 1e-3 / atol 1e-4); ~1.5x slower, never used by the product path. */
int fk_attention_fwd_f32_debug(const void* q, const void* k, const void* v, float* o, int32_t B, int32_t H,
                               int32_t S, int64_t v_ld, int64_t v_batch_stride, int64_t o_ld,
                               int64_t o_batch_stride, float scale, fk_stream_t stream);

/* ---- key-padding mask (padded batches of samples of different sizes) ---------------------------------------------------------
 * kmask: caller-owned device pointer, uint64 [B, ceil(S / 64)], 8-byte aligned.  Bit j of word (b, t) is 1 when key 64 t + j of
 * sample b is VALID; bits at positions >= S are ignored.  One word per 64-key tile of the attention kernels (forward and
 * backward): a wave classifies a tile with one uniform 8-byte load.  The mask is a KEY mask, broadcast over heads and queries
 * (F.scaled_dot_product_attention(attn_mask = mask[:, None, None, :])); every query row, masked token or not, is an ordinary row.
 * PRECONDITION (not checked: it would take a device synchronisation): every sample has at least one valid key, and the K / V
 * rows of masked keys are finite (in the model they come from zero-padded latents).  A sample without a valid key gets NaN
 * rows; a non-finite masked K / V row may reach the output as NaN.  Nothing is read or written out of bounds either way.
 *
 * fk_pack_key_mask: out[b, t] from a byte / bool mask (non-zero = valid), key s of sample b at mask[b * batch_stride + s]. */
int fk_pack_key_mask(const uint8_t* mask, int64_t batch_stride, int32_t B, int32_t S, uint64_t* out, fk_stream_t stream);
/* fk_attention_fwd_lse_bf16 over the valid keys only (lse may be NULL; otherwise the log2-domain log-sum-exp over the valid
 * keys).  The 8-wave kernel on the plain grid, one workgroup per (b, h, 256-row block): no workspace, no `grid`.  A tile whose
 * word is all ones runs the unmasked tile body, an all-zero tile is taken from the K / V ring and not computed, any other gets
 * the per-key select that the ragged last tile has always had (score -1e30, numerator exactly 0).  An all-ones mask therefore
 * gives the bits of fk_attention_fwd_ws_bf16(grid = -1), a prefix mask [0, L) those of a call with S = L. */
int fk_attention_fwd_masked_bf16(const void* q, const void* k, const void* v, void* o, float* lse, const uint64_t* kmask, int32_t B,
                                 int32_t H, int32_t S, int64_t v_ld, int64_t v_batch_stride, int64_t o_ld, int64_t o_batch_stride,
                                 float scale, fk_stream_t stream);
/* The fp32-output parity form (fk_attention_fwd_f32_debug) with the mask. */
int fk_attention_fwd_masked_f32_debug(const void* q, const void* k, const void* v, float* o, const uint64_t* kmask, int32_t B,
                                      int32_t H, int32_t S, int64_t v_ld, int64_t v_batch_stride, int64_t o_ld,
                                      int64_t o_batch_stride, float scale, fk_stream_t stream);

/* ---- block-level entry points ------------------------------------------------------------------------
 * ONE call enqueues every launch of a FluxTransformerBlock / FluxSingleTransformerBlock (diffusers 0.32.2 as the reference
 * reaches it at flux_pipeline.py:1067-1077), or of all blocks of a forward, on the caller's stream -- the same launches, in
 * the same order, with the same arguments as the per-kernel calls above, hence the same bits; what they remove is host work
 * (~5 400 calls per 28-step edit become 28).  All buffers are caller-owned bf16 (PyTorch's allocator), D = H * 128:
 *   s   [B, S, D]   residual stream, text rows [0, S_txt) first, image rows after (S = S_txt + S_img); updated in place
 *   n   [B, S, D]   LN + modulate output                 qkv [B, S, 3D]   fused QKV projection (V is read from it in place)
 *   q,k [B, H, S, 128]                                    o   [B, S, D]    attention output (double blocks)
 *   ff  [B, S, 4D]  MLP hidden (double blocks)            cat [B, S, 5D]   [attention | MLP hidden] (single blocks)
 * rope_cs: fp32 [S, 64, 2] (cos, sin) per rotary pair.  splitk_ws / attn_ws: the optional workspaces of fk_gemm_args /
 * fk_attention_fwd_ws_bf16 (NULL: never split).  mod: bf16 [B, mod_total] with row stride mod_batch_stride (elements), the
 * modulation vectors of every block (Linear(SiLU(temb)) of norm1 / norm1_context / norm); a block's weights struct carries its
 * element offset(s) into a row: double block (shift, scale, gate, shift_mlp, scale_mlp, gate_mlp) x D for the image stream at
 * mod_off_img and for the text stream at mod_off_txt; single block (shift, scale, gate) x D at mod_off. */
typedef struct fk_block_ws {
  void *s, *n, *qkv, *q, *k, *o, *ff, *cat;
  const float* rope_cs;
  void* splitk_ws;
  void* attn_ws;
  int64_t attn_ws_bytes;
  int32_t splitk_slots;
  int32_t B, S_txt, S_img, H;
  float eps;                       /* LayerNorm eps (1e-6) */
  /* launch controls handed to every GEMM / attention launch of the block (all zero = defaults): fk_gemm_args.variant / plan /
   * group_m / mfma and fk_attention_fwd_ws_bf16's `grid` */
  int32_t gemm_variant, gemm_plan, gemm_group_m, gemm_mfma, attn_grid;
  int32_t* gemm_variant_used;      /* OUT, optional: fk_gemm_args.variant_used of every GEMM of the call (the last one stays) */
} fk_block_ws;
typedef struct fk_double_block_weights {   /* bf16; Linear weights [N, K] K-contiguous, fused q|k|v as [3D, D] / [3D] */
  const void *wqkv_img, *bqkv_img, *wqkv_txt, *bqkv_txt;          /* attn.to_{q,k,v} / attn.add_{q,k,v}_proj */
  const void *norm_q, *norm_k, *norm_added_q, *norm_added_k;      /* RMSNorm weights [128] */
  const void *w_out, *b_out, *w_add_out, *b_add_out;              /* attn.to_out.0 / attn.to_add_out */
  const void *w_ff1, *b_ff1, *w_ff1_ctx, *b_ff1_ctx;              /* ff.net.0.proj / ff_context.net.0.proj  [4D, D] */
  const void *w_ff2, *b_ff2, *w_ff2_ctx, *b_ff2_ctx;              /* ff.net.2 / ff_context.net.2            [D, 4D] */
  int64_t mod_off_img, mod_off_txt;
} fk_double_block_weights;
typedef struct fk_single_block_weights {
  const void *wqkv, *bqkv, *norm_q, *norm_k;                      /* attn.to_{q,k,v} fused, attn.norm_{q,k} */
  const void *w_mlp, *b_mlp, *w_out, *b_out;                      /* proj_mlp [4D, D], proj_out [D, 5D] */
  int64_t mod_off;
} fk_single_block_weights;
int fk_double_block_fwd(const fk_block_ws* ws, const fk_double_block_weights* w, const void* mod, int64_t mod_batch_stride,
                        fk_stream_t stream);
int fk_single_block_fwd(const fk_block_ws* ws, const fk_single_block_weights* w, const void* mod, int64_t mod_batch_stride,
                        fk_stream_t stream);
/* All blocks of FluxTransformer2DModel.forward between the embedders and the output head: n_double double blocks, then
 * n_single single blocks (the embedders, the conditioning GEMMs and norm_out / proj_out stay per-kernel calls: 8 launches). */
int fk_mmdit_blocks_fwd(const fk_block_ws* ws, const fk_double_block_weights* dbl, int32_t n_double,
                        const fk_single_block_weights* sgl, int32_t n_single, const void* mod, int64_t mod_batch_stride,
                        fk_stream_t stream);

/* ---- MXFP8 block forward (opt-in inference format; fk_quantize_mxfp8 / fk_gemm_mxfp8 above) -------------------------------
 * The same launches, in the same order, as fk_double_block_fwd / fk_single_block_fwd / fk_mmdit_blocks_fwd, except that every
 * block GEMM becomes fk_quantize_mxfp8 of its activation operand (into the caller's fk_mx_ws) followed by fk_gemm_mxfp8(_grouped)
 * on the pre-quantized weight; biases, RMSNorm weights and the modulation offsets still come from the bf16 weight structs.
 * Weight pairs: e4m3 [N, K] and E8M0 [N, K / 32], both dense (ld = K, K / 32). */
typedef struct fk_mx_pair {
  const void* q;
  const void* s;
} fk_mx_pair;
typedef struct fk_double_block_weights_mx {
  fk_mx_pair qkv_img, qkv_txt, out, add_out, ff1, ff1_ctx, ff2, ff2_ctx;
} fk_double_block_weights_mx;
typedef struct fk_single_block_weights_mx {
  fk_mx_pair qkv, mlp, out;
} fk_single_block_weights_mx;
/* quantized activations of one launch: q >= B * S * 5D bytes (16-byte aligned), s >= B * S * 5D / 32 bytes (4-byte aligned).
 * fused != 0 selects the fused schedule: the producers emit MXFP8 themselves (fk_ln_modulate(2)_mxfp8, fk_gemm_mxfp8_q) and
 * only the attention output goes through fk_quantize_mxfp8 --
 *   double block: LN -> n8, QKV GEMM, attention, quantize o -> o8, out GEMMs, LN -> n8, ff1 GEMMs (GELU) -> ff8, ff2 GEMMs;
 *   single block: LN -> n8 (once), QKV GEMM, attention -> cat[:, :D], quantize -> cat8[:, :D], MLP GEMM (GELU) -> cat8[:, D:],
 *                 out GEMM on cat8;
 * the bf16 n, ff and cat[:, D:] are not written.  Same bits as the unfused schedule (blocks of 32 never straddle a producer).
 * fused is a bit set: bit 0 (1) = the schedule above; bit 1 (2), valid only together with bit 0 (fused = 3; fused = 2 alone is
 * FK_EINVAL) = the attention emits MXFP8 as well (fk_attention_fwd_ws_mxfp8: o8 img rows as stream B and txt rows as stream A with
 * split = S_txt; cat8 columns [0, D) with ldq = 5D) and no fk_quantize_mxfp8 launch is left -- the bf16 o and cat[:, :D] are then
 * not written either.  Same bits again.  Where that entry answers FK_EUNSUPPORTED (FK_ATTN_KERNEL=8), and only then, the block runs
 * the bf16 attention and the quantizer as with fused = 1.
 * The workspace then holds n8 (D bytes per row) AND the block's consumer operand at once: q >= B * S * 5D bytes for a double
 * block (n8 | o8 or ff8), B * S * 6D for a single block (n8 | cat8), s 1/32 of that; too small: FK_EINVAL, nothing launched.
 * splitk != 0 (either schedule): the long-K GEMMs of a block -- ff.net.2 / ff_context.net.2 (K = 4D) and the single block's
 * proj_out (K = 5D) -- get fk_block_ws.splitk_ws / splitk_slots and fk_block_ws.gemm_plan, so fk_gemm_mxfp8's launch plan may run
 * them as split-K pairs (variant 512; last-bit differences against splitk = 0).  0: no MXFP8 GEMM is handed a workspace. */
typedef struct fk_mx_ws {
  void* q;
  void* s;
  int64_t q_bytes, s_bytes;
  int32_t fused;
  int32_t* quantize_launches;   /* OUT, optional (NULL: not wanted): incremented by the host code of the call once per
                                 * fk_quantize_mxfp8 launch it enqueues (tests: 2 per double, 1 per single block when fused) */
  int32_t splitk;               /* 0: today's launches; != 0: split-K pairs allowed for the long-K GEMMs (above) */
} fk_mx_ws;
int fk_double_block_fwd_mx(const fk_block_ws* ws, const fk_mx_ws* mx, const fk_double_block_weights* w,
                           const fk_double_block_weights_mx* wx, const void* mod, int64_t mod_batch_stride, fk_stream_t stream);
int fk_single_block_fwd_mx(const fk_block_ws* ws, const fk_mx_ws* mx, const fk_single_block_weights* w,
                           const fk_single_block_weights_mx* wx, const void* mod, int64_t mod_batch_stride, fk_stream_t stream);
int fk_mmdit_blocks_fwd_mx(const fk_block_ws* ws, const fk_mx_ws* mx, const fk_double_block_weights* dbl,
                           const fk_double_block_weights_mx* dblx, int32_t n_double, const fk_single_block_weights* sgl,
                           const fk_single_block_weights_mx* sglx, int32_t n_single, const void* mod, int64_t mod_batch_stride,
                           fk_stream_t stream);

/* ---- backward pass of the MMDiT (train_denoiser.py:1172 `accelerator.backward(loss)` through diffusers' blocks) ---- */
/* Forward attention that also saves lse[b, h, s] = log2(sum_j exp(q.k_j * scale)) (fp32) for the backward pass. */
int fk_attention_fwd_lse_bf16(const void* q, const void* k, const void* v, void* o, float* lse, int32_t B, int32_t H,
                              int32_t S, int64_t v_ld, int64_t v_batch_stride, int64_t o_ld, int64_t o_batch_stride,
                              float scale, fk_stream_t stream);
/* A [B, H, S, 128] bf16 tensor in any of the layouts the path uses: element (b, h, s, d) at
 * p + b*batch_stride + h*head_stride + s*ld + d   (head-major q / k: ld = 128, head_stride = S*128;
 * token-major slices of a [B, S, n*H*128] buffer: ld = n*H*128, head_stride = 128). */
typedef struct fk_attn_view {
  const void* p;
  int64_t ld, head_stride, batch_stride;
} fk_attn_view;
/* dQ, dK, dV of O = softmax(Q K^T scale) V given dO, the forward's lse and dsum[b, h, s] = sum_d dO * O (fk_rowdot_bf16).
 * Three deterministic passes (no atomics); dq / dk / dv are written, not accumulated. */
int fk_attention_bwd_bf16(const fk_attn_view* q, const fk_attn_view* k, const fk_attn_view* v, const fk_attn_view* dout,
                          const float* lse, const float* dsum, const fk_attn_view* dq, const fk_attn_view* dk,
                          const fk_attn_view* dv, int32_t B, int32_t H, int32_t S, float scale, fk_stream_t stream);
/* The same with the attention forward's stream-K workspace (fk_attention_ws_bytes(); shared with the forward on one stream):
 * the dQ pass then runs as a persistent grid where one workgroup per 256-row block would waste part of a round of CUs
 * (the parts of a cut block ADD their fp32 accumulators through the workspace: symmetric, deterministic). */
int fk_attention_bwd_ws_bf16(const fk_attn_view* q, const fk_attn_view* k, const fk_attn_view* v, const fk_attn_view* dout,
                             const float* lse, const float* dsum, const fk_attn_view* dq, const fk_attn_view* dk,
                             const fk_attn_view* dv, int32_t B, int32_t H, int32_t S, float scale, void* ws, int64_t ws_bytes,
                             int32_t grid, int32_t passes, fk_stream_t stream);
/* grid: as fk_attention_fwd_ws_bf16 (0 default, -1 plain grid, >= 2 forced persistent grid).  passes (measurement / parity):
 * 0 or 2 = two launches, the dQ pass and one pass in which wave pairs produce dK and dV together (7 tile products, default),
 * 3 = three launches (dQ, dV, dK: 8 tile products).  dQ and dV are the same bit for bit in both; dK differs in the last bf16
 * bit (the paired pass forms p (dP - D) from the bf16 p that also enters dV, the three-pass form from the fp32 p). */

/* fk_attention_bwd_bf16 under the key-padding mask of fk_attention_fwd_masked_bf16 (same format, same precondition; lse from
 * the masked forward).  Plain grids; passes as above (0 / 2 or 3).  dQ pass: masked keys weigh 0, all-masked key tiles are not
 * computed.  dK / dV: the rows of masked keys are WRITTEN as exact zeros, and a key block without a valid key streams nothing.
 * Query rows of masked tokens are ordinary rows (in the model their dout is zero: their loss weight is). */
int fk_attention_bwd_masked_bf16(const fk_attn_view* q, const fk_attn_view* k, const fk_attn_view* v, const fk_attn_view* dout,
                                 const float* lse, const float* dsum, const fk_attn_view* dq, const fk_attn_view* dk,
                                 const fk_attn_view* dv, const uint64_t* kmask, int32_t B, int32_t H, int32_t S, float scale,
                                 int32_t passes, fk_stream_t stream);

/* fp32 elements of workspace `ws` the reductions below need (per-workgroup partial sums, fixed-order finalisation). */
int64_t fk_bwd_ws_floats(void);
/* Largest grid (256-thread blocks, 8 elements per thread and trip) of the grid-stride elementwise kernels fk_gelu_bwd_bf16,
 * fk_silu_bwd_bf16, fk_gate_res_fwd_bf16, fk_gelu_tanh_bf16: above 2048 * this many elements their threads loop. */
int64_t fk_bwd_ew_max_blocks(void);
/* Adjoint of fk_ln_modulate_bf16 for one stream (rows [b*rows_per_batch, (b+1)*rows_per_batch) use scale row b):
 *   dx_out = (dx_in ? dx_in : 0) + dLN/dx,   dshift[b] = sum_s dn,   dscale[b] = sum_s dn * LN(x)     (fp32 outputs;
 * dscale must be dshift + D: the (shift, scale) chunk pair of the block's modulation vector, batch stride given). */
int fk_ln_modulate_bwd_bf16(const void* x, fk_rows xr, const void* dn, fk_rows dnr, const void* scale,
                            int64_t mod_batch_stride, int64_t rows_per_batch, const void* dx_in, fk_rows dxi, void* dx_out,
                            fk_rows dxo, float* dshift, float* dscale, int64_t dmod_batch_stride, float* ws, int32_t B,
                            int32_t D, float eps, fk_stream_t stream);
/* Adjoint of the FK_EPI_GATE_RES epilogue out = res + gate[b] * y:  dy = dout * gate[b] (bf16),
 * dgate[b, :] = sum_s dout * y (fp32);  dres = dout. */
int fk_gate_res_bwd_bf16(const void* dout, fk_rows dor, const void* y, fk_rows yr, const void* gate,
                         int64_t gate_batch_stride, int64_t rows_per_batch, void* dy, fk_rows dyr, float* dgate,
                         int64_t dgate_batch_stride, float* ws, int32_t B, int32_t N, fk_stream_t stream);
/* out = df * gelu_tanh'(h) over n elements (h = the Linear's bf16 output before the activation); out may alias df.
 * Accuracy of the activation kernels (fk_gelu_bwd_bf16, fk_silu_bwd_bf16, fk_gelu_tanh_bf16, fk_silu_bf16 and the GEMM
 * epilogues of the same functions), every finite bf16 input: within 1 bf16 ulp of the exact function rounded once, finite
 * wherever it is (the derivative of GELU(tanh) is 1 / 0 at |h| > 1.8e19, where fp32 h^2 overflows).  They form
 * sigmoid(.) in fp32 on the hardware exp2 / rcp, which flush subnormal results: where the exact sigmoid is below 2^-126
 * (h < -87.3 for SiLU, h < -10.05 for GELU(tanh)) the output is +-0, although the exact value -- at most 2^-126 times the
 * factor that multiplies the sigmoid (|h|; |df| (1 + |h| ...) for the derivatives) -- may still be a normal bf16 number. */
int fk_gelu_bwd_bf16(const void* h, const void* df, void* out, int64_t n, fk_stream_t stream);
/* The same for FK_EPI_SILU (the denoise_projector's activation, modeling_univa_denoise_tower.py:36-41; the projector is
 * among the parameters train_denoiser.py:71-119 trains). */
int fk_silu_bwd_bf16(const void* h, const void* df, void* out, int64_t n, fk_stream_t stream);
/* Adjoint of fk_qkv_post_bf16: dq, dk [B, H, S, 128] -> the q and k thirds of dqkv [B, S, 3*H*128] (gradient of the raw
 * projection `qkv`), and dw [2 (q, k)][2 (image, text)][128] fp32 = gradients of the RMSNorm weights. */
int fk_qkv_post_bwd_bf16(const void* dq, const void* dk, const void* qkv, void* dqkv, const void* wq_img, const void* wk_img,
                         const void* wq_txt, const void* wk_txt, const float* cos, const float* sin, float* dw, float* ws,
                         int32_t B, int32_t S, int32_t S_txt, int32_t H, float eps, fk_stream_t stream);
/* Un-fused pieces of the block forward that the recomputation (gradient checkpointing, train_denoiser.py:486) runs so
 * that the pre-gate / pre-activation tensors exist: out = bf16(res + bf16(gate[b] * y)) (the FK_EPI_GATE_RES epilogue on a
 * stored y) and y = bf16(gelu_tanh(x)) (the FK_EPI_GELU_TANH epilogue on a stored x); same rounding points. */
int fk_gate_res_fwd_bf16(const void* res, fk_rows rr, const void* y, fk_rows yr, const void* gate, int64_t gate_batch_stride,
                         int64_t rows_per_batch, void* out, fk_rows orr, int64_t M, int32_t N, fk_stream_t stream);
int fk_gelu_tanh_bf16(const void* x, fk_rows xr, void* y, fk_rows yr, int64_t M, int32_t N, fk_stream_t stream);
/* dst[c, r] (bf16, row length dst_ld >= R, columns r >= R zeroed) = src[r, c] (fp32, row stride src_ld): the fp32
 * modulation-vector gradients [B, n] as the K-padded operand of their weight-gradient GEMM. */
int fk_f32_to_bf16_transposed(const float* src, int64_t src_ld, void* dst, int32_t dst_ld, int32_t R, int32_t C,
                              fk_stream_t stream);
/* out[n] = sum_m x[m, n] (fp32): bias gradients. */
int fk_colsum_bf16(const void* x, fk_rows xr, int64_t M, int32_t N, float* out, float* ws, fk_stream_t stream);
/* out[b, h, s] = sum_d a[b, s, h*128 + d] * c[b, s, h*128 + d] (fp32): the softmax-backward row term. */
int fk_rowdot_bf16(const void* a, int64_t a_ld, int64_t a_batch_stride, const void* c, int64_t c_ld,
                   int64_t c_batch_stride, float* out, int32_t B, int32_t S, int32_t H, fk_stream_t stream);

/* Block-level entry points of the backward pass (the forward's: fk_double_block_fwd / fk_single_block_fwd above): ONE call
 * enqueues the backward of a FluxTransformerBlock / FluxSingleTransformerBlock (diffusers 0.32.2), i.e. what autograd runs for
 * the reference at `accelerator.backward(loss)` (train_denoiser.py:1172), from the activations the training forward stored.
 * Host code only: the same per-kernel calls with the same arguments, in the same order, as the Python adaptor
 * (gpt_image_edit_amd/backward.py) -- bit-identical results.  Data gradients read the stored weights (fk_gemm_args.layout 1),
 * weight gradients both operands token-major (layout 2): B * S_txt and B * S_img must be multiples of 64.
 * Batch: fk_single_block_bwd takes any B (its operands are whole [B, S, *] buffers); double blocks: B == 1 (the stream
 * slices of a joint buffer are not uniformly strided, and the layout-2 GEMM addresses its second operand by one row stride).
 * fk_double_block_bwd with B > 1 returns FK_EUNSUPPORTED before its first launch: nothing has been written.
 * fk_bwd_ws = shapes, scratch shared by every block of a pass, launch controls; caller-owned, nothing is allocated. */
typedef struct fk_bwd_ws {
  int32_t B, S_txt, S_img, H;
  float eps;                               /* LayerNorm / RMSNorm eps (1e-6) */
  int32_t splitk_slots;
  void* g;                                 /* bf16 [B, S, D]: gradient of the residual stream, IN (block output) / OUT (block input) */
  void *dy, *dff, *dn, *d_o, *dqkv;        /* bf16 scratch [B,S,D], [B,S,4D], [B,S,D], [B,S,D], [B,S,3D] */
  void *dq, *dk;                           /* bf16 scratch [B, H, S, 128] */
  float* dsum;                             /* fp32 [B, H, S] */
  float* dmod;                             /* fp32 [B, 12 D] (double block: image 6D | text 6D) / [B, 3 D] (single) */
  void *ff, *cat;                          /* bf16 [B,S,4D] / [B,S,5D]: rebuilt GELU outputs (only when ff.net.2 / proj_out train) */
  const float *cos, *sin;                  /* fp32 [S, 128] rotary tables */
  float* red_ws;                           /* fk_bwd_ws_floats() */
  void* attn_ws; int64_t attn_ws_bytes;    /* fk_attention_ws_bytes(), as the forward's */
  void* splitk_ws;
  const void* mod; int64_t mod_batch_stride;   /* bf16 modulation vectors of the step (all blocks), row stride in elements */
  const void *actT, *onesT;                /* bf16 [D, 64] = silu(temb)^T zero-padded, [64, 64] ones in the first B columns */
  void* dmodT;                             /* bf16 [6 D, 64] scratch */
  int32_t gemm_variant, gemm_plan, gemm_group_m, gemm_mfma, attn_grid, attn_passes;   /* as fk_gemm_args / fk_attention_bwd_ws_bf16 */
  int32_t* gemm_variant_used;              /* OUT, optional */
} fk_bwd_ws;
typedef struct fk_block_saved {            /* what the training forward kept of ONE block (bf16 unless said) */
  const void *x0;                          /* [B,S,D] block input */
  const void *n1, *qkv, *q, *k;            /* LN+modulate output, raw fused projection [B,S,3D], q / k after RMSNorm + RoPE [B,H,S,128] */
  const void *y1, *h1, *o;                 /* pre-gate projection output [B,S,D], pre-GELU MLP hidden [B,S,4D], attention output */
  const float* lse;                        /* fp32 [B, H, S] */
  const void *x1, *n2, *y2;                /* double blocks only: stream after attention, second LN+modulate, pre-gate MLP output */
} fk_block_saved;
/* Gradient outputs: bf16 [N, K] weights as stored, fp32 [N] biases, fp32 [2 (q, k)][2 (image, text)][128] RMSNorm weights (always
 * written), AdaLN linear as bf16 [n, D] + bf16 [n, 64] whose COLUMN 0 is the bias gradient.  NULL weight pointer = frozen. */
typedef struct fk_single_block_grads {
  void* dwqkv; float* dbqkv;               /* attn.to_{q,k,v} fused [3D, D] / [3D] */
  void* dw_mlp; float* db_mlp;             /* proj_mlp [4D, D] */
  void* dw_out; float* db_out;             /* proj_out [D, 5D] */
  float* dnorm;
  void *dw_mod, *db_mod;                   /* norm.linear [3D, D] / [3D, 64] */
} fk_single_block_grads;
typedef struct fk_double_block_grads {
  void* dwqkv_img; float* dbqkv_img; void* dwqkv_txt; float* dbqkv_txt;
  void* dw_out; float* db_out; void* dw_add_out; float* db_add_out;
  void* dw_ff1; float* db_ff1; void* dw_ff1_ctx; float* db_ff1_ctx;       /* ff.net.0.proj / ff_context.net.0.proj [4D, D] */
  void* dw_ff2; float* db_ff2; void* dw_ff2_ctx; float* db_ff2_ctx;       /* ff.net.2 / ff_context.net.2 [D, 4D] */
  float* dnorm;
  void *dw_mod_img, *db_mod_img, *dw_mod_txt, *db_mod_txt;                /* norm1.linear / norm1_context.linear [6D, D] / [6D, 64] */
} fk_double_block_grads;
int fk_single_block_bwd(const fk_bwd_ws* ws, const fk_block_saved* saved, const fk_single_block_weights* w,
                        const fk_single_block_grads* grads, fk_stream_t stream);
int fk_double_block_bwd(const fk_bwd_ws* ws, const fk_block_saved* saved, const fk_double_block_weights* w,
                        const fk_double_block_grads* grads, fk_stream_t stream);

/* Elementwise / tiny kernels ------------------------------------------------------------------ */
/* y = bf16(silu(x)) over n elements (n % 8 == 0). */
int fk_silu_bf16(const void* x, void* y, int64_t n, fk_stream_t stream);
/* out[b, :256] = bf16(cat(cos, sin)(bf16(bf16(v[b]) * 1000) * freqs[k])), k < 128:
 * Timesteps(256, flip_sin_to_cos=True) after the model's `.to(dtype) * 1000`; v bf16 or fp32 [B];
 * freqs = exp(-ln(1e4) * k / 128) as a device fp32[128] table (computed once by the host). */
int fk_timestep_proj(const void* v, int32_t v_is_fp32, const float* freqs, void* out, int32_t B,
                     fk_stream_t stream);
/* out = bf16(bf16(a + b) + c) over n elements: temb = (T + G) + P. */
int fk_add3_bf16(const void* a, const void* b, const void* c, void* out, int64_t n, fk_stream_t stream);
/* True classifier-free guidance, `noise_pred = neg + true_cfg_scale * (noise_pred - neg)`
 * (univa/utils/flux_pipeline.py:1095): out = bf16(neg + bf16(scale * bf16(pos - neg))) over n elements
 * (the python-float scale stays fp32, as on the GPU the reference runs on); out may alias pos or neg. */
int fk_true_cfg_bf16(const void* pos, const void* neg, void* out, float scale, int64_t n, fk_stream_t stream);
/* ---- optimisation step of the denoiser (reference train_denoiser.py:935-1181): the HBM-bound pieces around the MMDiT forward /
 * backward ("backward pass" section above) ---- */
/* Doubles of workspace the two reductions below need. */
int64_t fk_reduce_ws_doubles(void);
/* noisy = (1 - sigma[b]) * x + sigma[b] * noise in fp32 (train_denoiser.py:994), rounded to bf16 and written as the
 * 2x2-packed tokens FluxKontextPipeline.prepare_latents / _pack_latents produce (:1009-1027):
 * x, noise fp32 [B, C, h, w]; tokens bf16, sample b at tokens + b*tokens_batch_stride, [ (h/2)(w/2), 4C ] row-major --
 * the stride lets it land in the target half of the [target | condition] token buffer. */
int fk_flow_noisy_tokens_bf16(const float* x, const float* noise, const float* sigma, void* tokens,
                              int64_t tokens_batch_stride, int32_t B, int32_t C, int32_t h, int32_t w, fk_stream_t stream);
/* Flow-matching loss and its gradient in one pass (train_denoiser.py:1096-1166, unpadded batch):
 *   d = float(pred) - (noise - x)  on the packed bf16 prediction (the `_unpack_latents` index map is applied here),
 *   loss[0] = sum(weight[b] * d^2) / (B*C*h*w)   (weight NULL = ones: the shipped logit_normal scheme),
 *   grad    = bf16(2 * weight[b] * d / (B*C*h*w)) in pred's packed layout (NULL: loss only).
 * ws: fk_reduce_ws_doubles() doubles; fixed-order two-stage sum, bit-identical from run to run. */
int fk_flow_loss_bf16(const void* pred, int64_t pred_batch_stride, const float* x, const float* noise,
                      const float* weight, void* grad, int64_t grad_batch_stride, double* loss, double* ws,
                      int32_t B, int32_t C, int32_t h, int32_t w, fk_stream_t stream);
/* The stage-2 loss AS CONFIGURED (scripts/denoiser/flux_qwen2p5vl_7b_vlm_stage2_1024.yaml:27 `mask_weight_type: 'log'`;
 * train_denoiser.py:1123-1165): per-pixel weights on top of the per-sample one,
 *   weighting[b, y, x] = weight[b] * area_weights[b, 0, y, x] * weight_mask[b, 0, y, x]   (fp32, that order; NULL factor = 1;
 *                        the maps are [B, 1, h, w] contiguous, already nearest-resized to the latent size as :1131-1148 does),
 *   loss[0] = sum(weighting * d^2) / denominator,  grad = bf16(2 * weighting * d / denominator),
 *   denominator = mask_sum[0] * C when mask_sum (a DEVICE scalar holding weight_mask.sum(), :1163-1165) is given, else B*C*h*w
 *   (loss.mean()).  All map arguments NULL: fk_flow_loss_bf16 bit for bit. */
int fk_flow_loss_weighted_bf16(const void* pred, int64_t pred_batch_stride, const float* x, const float* noise,
                               const float* weight, const float* area_weights, const float* weight_mask, const float* mask_sum,
                               void* grad, int64_t grad_batch_stride, double* loss, double* ws,
                               int32_t B, int32_t C, int32_t h, int32_t w, fk_stream_t stream);
/* out[0] = (accumulate ? out[0] : 0) + sum(g^2) over n fp32 (or bf16) elements: the global gradient norm of
 * accelerator.clip_grad_norm_ (train_denoiser.py:1171-1177) accumulated tensor by tensor, in double. */
int fk_sumsq(const void* g, int32_t g_is_bf16, int64_t n, int32_t accumulate, double* out, double* ws, fk_stream_t stream);
/* torch.optim.AdamW's update (single-tensor form) on fp32 master weights, with the clipping coefficient
 * min(1, max_grad_norm / (sqrt(grad_sumsq[0]) + 1e-6)) folded into the gradient read (grad_sumsq NULL: no clipping)
 * and the bf16 copy the forward pass reads written in the same pass (param_bf16 NULL: none).  step counts from 1. */
int fk_adamw_step(float* master, void* param_bf16, const void* grad, int32_t grad_is_bf16, float* exp_avg,
                  float* exp_avg_sq, const double* grad_sumsq, float max_grad_norm, float lr, float beta1, float beta2,
                  float eps, float weight_decay, int32_t step, int64_t n, fk_stream_t stream);
/* The same with gradients that are stored UNSCALED sums: the gradient applied is grad_scale * grad (grad_scale = 1 / world
 * for the sums a ZeRO-2 reduce-scatter leaves), grad_sumsq is the squared norm of the stored sums, and the clipping
 * coefficient becomes grad_scale * min(1, max_grad_norm / (grad_scale * sqrt(grad_sumsq[0]) + 1e-6)) -- one multiply per
 * element either way, no pass of its own for the mean.  grad_scale = 1 is fk_adamw_step bit for bit. */
int fk_adamw_step_scaled(float* master, void* param_bf16, const void* grad, int32_t grad_is_bf16, float* exp_avg,
                         float* exp_avg_sq, const double* grad_sumsq, float max_grad_norm, float grad_scale, float lr,
                         float beta1, float beta2, float eps, float weight_decay, int32_t step, int64_t n,
                         fk_stream_t stream);
/* ---- Prodigy (csrc/prodigy.hip): the reference's second optimiser (train_denoiser.py:595-624, `optimizer: 'prodigy'`) on the
 * same fp32 masters.  One step = fk_prodigy_begin, fk_prodigy_moments per tensor / chunk, [all-reduce of the two running sums
 * under data parallelism], fk_prodigy_update_d, fk_prodigy_apply per tensor / chunk.  Every scalar lives in a caller-owned
 * DEVICE buffer of FK_PRODIGY_STATE_DOUBLES doubles; a step reads nothing back to the host.  Initial contents: D = D_MAX = d0,
 * every other slot 0.  The step (k = state[K], d = state[D]):
 *   begin     bc = use_bias_correction ? sqrt(1 - beta2^(k+1)) / (1 - beta1^(k+1)) : 1;  DLR = d * lr * bc;
 *             D_NUMERATOR *= beta3;  SUM_DOT = SUM_ABS = SKIPPED = 0
 *   moments   g = grad * coef (fk_adamw_step_scaled's clipping / grad_scale coefficient, same arithmetic);  !decouple: g += wd * p;
 *             SUM_DOT += sum g * (p0 - p);  m = beta1 m + d (1 - beta1) g;  v = beta2 v + d^2 (1 - beta2) g^2;
 *             s = beta3 s + (d / d0) (safeguard_warmup ? d : DLR) g;  SUM_ABS += sum |s_new|
 *   update_d  D_NUMERATOR += (d / d0) DLR SUM_DOT;  D_DENOM = SUM_ABS;  D_DENOM == 0: SKIPPED = 1 and nothing else changes; else
 *             D_HAT = d_coef D_NUMERATOR / D_DENOM;  d == d0: d = max(d, D_HAT);  D_MAX = max(D_MAX, D_HAT);
 *             D = min(D_MAX, d * growth_rate);  K += 1
 *   apply     SKIPPED: nothing.  decouple: p += p * (-wd DLR);  p -= DLR * (m / (sqrt(v) + D eps));  bf16 copy of p
 * Element arithmetic is fp32, the scalar factors are formed in double and rounded once, the sums are double.  The sums have a
 * fixed order (per-block partials in ws, one finishing block) and use no atomics: two runs give the same bits, and successive
 * fk_prodigy_moments calls accumulate in call order.  Pointers that are all 16-byte aligned (bf16 ones 8-byte) move as 16-byte
 * vectors with a scalar tail; anything else goes element by element; any n >= 1.  NULL pointers, n <= 0, grad_scale <= 0,
 * d0 <= 0, a beta outside [0, 1): FK_EINVAL, nothing launched. */
enum {
  FK_PRODIGY_D = 0,           /* step-size estimate */
  FK_PRODIGY_D_MAX = 1,
  FK_PRODIGY_D_NUMERATOR = 2,
  FK_PRODIGY_D_DENOM = 3,
  FK_PRODIGY_D_HAT = 4,
  FK_PRODIGY_DLR = 5,         /* d * lr * bias correction of the CURRENT step (what fk_prodigy_apply uses) */
  FK_PRODIGY_K = 6,           /* steps taken (skipped ones do not count) */
  FK_PRODIGY_SKIPPED = 7,     /* 1 after fk_prodigy_update_d met D_DENOM == 0 */
  FK_PRODIGY_SUM_DOT = 8,     /* running sum of g * (p0 - p) of this step */
  FK_PRODIGY_SUM_ABS = 9,     /* running sum of |s| of this step */
  FK_PRODIGY_STATE_DOUBLES = 10
};
/* Doubles of workspace fk_prodigy_moments needs (two partials per block). */
int64_t fk_prodigy_ws_doubles(void);
int fk_prodigy_begin(double* state, double lr, double beta1, double beta2, double beta3, int32_t use_bias_correction,
                     fk_stream_t stream);
int fk_prodigy_moments(const float* master, const float* p0, const void* grad, int32_t grad_is_bf16, float* m, float* v,
                       float* s, double* state, const double* grad_sumsq, float max_grad_norm, float grad_scale, float beta1,
                       float beta2, float beta3, float weight_decay, double d0, int32_t decouple, int32_t safeguard_warmup,
                       int64_t n, double* ws, fk_stream_t stream);
int fk_prodigy_update_d(double* state, double d0, double d_coef, double growth_rate, fk_stream_t stream);
int fk_prodigy_apply(float* master, void* param_bf16, const float* m, const float* v, const double* state, float eps,
                     float weight_decay, int32_t decouple, int64_t n, fk_stream_t stream);

/* FlowMatchEulerDiscreteScheduler.step fused with the pipeline's `noise_pred[:, :S_tgt]` slice:
 *   x[b, s, :] = bf16(float(x) + float(bf16(bf16(dsigma) * v[b, s, :])))   for s < S_tgt
 * x rows at x + b*x_batch_stride + s*C, v rows at v + b*v_batch_stride + s*C.
 * (reference univa/utils/flux_pipeline.py:1078,1099) */
int fk_euler_step_bf16(void* x, int64_t x_batch_stride, const void* v, int64_t v_batch_stride,
                       int32_t B, int32_t S_tgt, int32_t C, float dsigma, fk_stream_t stream);
/* The same step for a masked (inpaint) edit, fused with the keep-region blend of diffusers' inpaint loop; every bf16(...)
 * is one fp32 evaluation rounded once, as torch rounds per bf16 tensor op.  For s < S_tgt, element j of a token:
 *   p    = bf16(x + bf16(bf16(dsigma) * v))                                        (fk_euler_step_bf16)
 *   sb   = bf16(sigma_next)
 *   keep = bf16(bf16(sb * noise) + bf16(bf16(1 - sb) * x0))                        (scale_noise; x0 when sigma_next == 0)
 *   x    = bf16(bf16(bf16(1 - mask[j % 4]) * keep) + bf16(mask[j % 4] * p))
 * mask: bf16 [1 or B, S_tgt, 4], one value per sub-pixel of the 2x2-packed token (element j is channel j / 4, sub-pixel
 * j % 4), 1 = repaint, 0 = keep; mask_batch_stride == 0 broadcasts one mask over the batch.  x0, noise: [B, S_tgt, C] rows
 * at their batch strides.  mask NULL = a mask of ones: the values of fk_euler_step_bf16; x0 and noise are then not read.
 * C % 8 == 0; pointers and batch strides 16-byte aligned, the mask and its stride 8-byte aligned. */
int fk_euler_inpaint_step_bf16(void* x, int64_t x_batch_stride, const void* v, int64_t v_batch_stride,
                               const void* x0, int64_t x0_batch_stride, const void* noise, int64_t noise_batch_stride,
                               const void* mask, int64_t mask_batch_stride, int32_t B, int32_t S_tgt, int32_t C,
                               float dsigma, float sigma_next, fk_stream_t stream);
/* FlowMatchEulerDiscreteScheduler.scale_noise on bf16 tensors -- the start tokens of an edit that begins inside the schedule:
 *   out[b, s, :] = bf16(bf16(bf16(sigma) * noise) + bf16(bf16(1 - bf16(sigma)) * x0))   for s < S_tgt
 * (the `keep` of fk_euler_inpaint_step_bf16, one device function). */
int fk_scale_noise_bf16(const void* x0, int64_t x0_batch_stride, const void* noise, int64_t noise_batch_stride, void* out,
                        int64_t out_batch_stride, int32_t B, int32_t S_tgt, int32_t C, float sigma, fk_stream_t stream);
/* Second-order multistep (Adams-Bashforth 2) step of the denoise loop on a non-uniform sigma grid (csrc/solver_step.hip;
 * scheduler.py: FlowMatchMultistepScheduler.coefficients), in place on rows s < S_tgt of x.  Per element, in fp32 with every
 * product and every sum rounded once (never an fma), and ONE rounding to bf16:
 *   s = x + c_v * v;   if (use_hist) s = s + c_h * hist;   p = bf16(s)
 * c_v and c_h are used as the fp32 numbers they are (not rounded to bf16 as fk_euler_step_bf16 rounds dsigma).  The same pass
 * stores hist <- v; every element's hist is read (use_hist == 1) before it is written, and with use_hist == 0 hist is never
 * read (it may hold anything) and still written.  hist: [B, S_tgt, C] rows at hist_batch_stride, a buffer of its own.
 * mask NULL: x = p; x0, noise and sigma_next are not read.  With a mask (the layout of fk_euler_inpaint_step_bf16):
 *   x = bf16(bf16(bf16(1 - mask[j % 4]) * keep) + bf16(mask[j % 4] * p)),  keep as in fk_euler_inpaint_step_bf16
 * FK_EINVAL, nothing launched: x, v or hist NULL, hist == v or hist == x, B, S_tgt or C < 1, C % 8 != 0, a pointer or batch
 * stride that is not 16-byte aligned (the mask and its stride: 8 bytes), use_hist outside {0, 1}, a mask without x0 and noise. */
int fk_ab2_step_bf16(void* x, int64_t x_batch_stride, const void* v, int64_t v_batch_stride,
                     void* hist, int64_t hist_batch_stride,
                     const void* x0, int64_t x0_batch_stride, const void* noise, int64_t noise_batch_stride,
                     const void* mask, int64_t mask_batch_stride,
                     int32_t B, int32_t S_tgt, int32_t C, float c_v, float c_h, int32_t use_hist,
                     float sigma_next, fk_stream_t stream);
/* The denoise loop's step on a float32 latent state (csrc/solver_step.hip), for the Euler and the AB2 rule alike: the state is
 * carried unrounded from step to step in `state`, fp32 [B, S_tgt, C] rows at state_batch_stride, and rows s < S_tgt of the bf16
 * token buffer x receive its rounding, the model's next input.  Per element, every product and every sum is ONE float32
 * operation (never an fma), and the only rounding to bf16 is the one stored to x:
 *   xs  = load_state ? state : float(x)          load_state == 0 (the first executed step, or the step after the caller
 *                                                replaced the token rows) seeds the state from x: `state` is then NOT read
 *                                                and may hold anything, NaN bits included
 *   s   = xs + c_v * v;   if (use_hist) s = s + c_h * hist          (hist is not read when use_hist == 0)
 *   mask NULL:   out = s                                            (x0, noise and sigma_next are not read)
 *   with a mask: k   = sigma_next * noise + om * x0,  om = float32(1 - sigma_next) formed once on the host
 *                out = (1 - mask[j % 4]) * k + mask[j % 4] * s      (float32: sigma_next, k and the blend are NOT rounded to bf16)
 *   state <- out;   x <- bf16(out);   hist <- v in the same pass when hist is non-NULL
 * A mask value of 1 gives s bit for bit and 0 gives k, which is x0 exactly when sigma_next == 0.  Euler: use_hist = 0, hist NULL,
 * c_v = sigma[i+1] - sigma[i] as the float32 difference it is (fk_euler_step_bf16 rounds it to bf16; this entry does not).  Every
 * element's hist is read (use_hist == 1) before it is written.  mask, x0, noise: the layouts of fk_euler_inpaint_step_bf16.
 * FK_EINVAL, nothing launched: state, x or v NULL, B, S_tgt or C < 1, C % 8 != 0, a bf16 pointer or batch stride that is not
 * 16-byte aligned (the mask and its stride: 8 bytes; the state: a 16-byte aligned pointer and a stride that is a multiple of 4
 * elements), use_hist or load_state outside {0, 1}, use_hist == 1 with hist NULL, hist == x, v or state, state == x, a mask
 * without x0 and noise. */
int fk_solver_step_f32(float* state, int64_t state_batch_stride, void* x, int64_t x_batch_stride,
                       const void* v, int64_t v_batch_stride, void* hist, int64_t hist_batch_stride,
                       const void* x0, int64_t x0_batch_stride, const void* noise, int64_t noise_batch_stride,
                       const void* mask, int64_t mask_batch_stride,
                       int32_t B, int32_t S_tgt, int32_t C, float c_v, float c_h, int32_t use_hist, int32_t load_state,
                       float sigma_next, fk_stream_t stream);
/* ---- step cache: residual caching across denoise steps (csrc/step_cache.hip; gpt_image_edit_amd/step_cache.py) ----
 * All views are bf16 [B, R, D] with contiguous rows, M = B * R rows addressed through fk_rows (strides in elements, >= D and
 * >= 0), e.g. the image part n[:, S_txt:] of a joint buffer.  is_bf16 states the type of the caller's tensors (as fk_sumsq's g_is_bf16
 * does): 0 is FK_EUNSUPPORTED.  NULL pointers, M < 1, D < 1, a row stride below D: FK_EINVAL, nothing launched.  Rows that are
 * 16-byte aligned move as 16-byte vectors, a cut last chunk (D % 8 != 0) and unaligned views element by element; any size.
 *
 * out[0] = sum |float(a) - float(b)|, out[1] = sum |float(b)| over all M * D elements, in fp32 and in a FIXED order: per
 * 8-element chunk a pairwise tree, per thread its chunks in increasing order, a 256-wide halving tree per block, then one
 * finalising block over the per-block partials in ws (a second launch).  No floating-point atomics: two launches on the same
 * data give the same bits.  ws: fk_absdiff_ws_floats() floats owned by the caller (ws_floats says how many there are; fewer
 * than 2 per block of the launch is FK_EINVAL); launches that share one must be ordered. */
int64_t fk_absdiff_ws_floats(void);
int fk_absdiff_sums_bf16(const void* a, fk_rows ra, const void* b, fk_rows rb, int64_t M, int32_t D, int32_t is_bf16,
                         float* out, float* ws, int64_t ws_floats, fk_stream_t stream);
/* r = bf16(float(h_out) - float(h0)): what the blocks added to their input, kept for the steps that skip them.  r must not
 * overlap h_out or h0, nor they each other (tested on the byte range a view spans from its first to its last row: FK_EINVAL). */
int fk_residual_save_bf16(const void* h_out, fk_rows ro, const void* h0, fk_rows r0, void* r, fk_rows rr, int64_t M, int32_t D,
                          int32_t is_bf16, fk_stream_t stream);
/* out = bf16(float(h0) + float(r)).  out may BE h0 (same pointer and strides); any other overlap of the three is FK_EINVAL. */
int fk_residual_apply_bf16(const void* h0, fk_rows r0, const void* r, fk_rows rr, void* out, fk_rows ro, int64_t M, int32_t D,
                           int32_t is_bf16, fk_stream_t stream);
/* The first-block measure of the step cache as one pass over three bf16 views: r = bf16(float(h1) - float(h0)), exactly
 * fk_residual_save_bf16's value, written to r_out when r_out is non-NULL (rr is ignored otherwise), and out[0] = sum |float(r) -
 * float(ref)|, out[1] = sum |float(ref)| with fk_absdiff_sums_bf16's decomposition, summation order and workspace: out holds the
 * bits of fk_residual_save_bf16(h1, h0, r) followed by fk_absdiff_sums_bf16(r, ref).  The inputs may overlap one another; r_out
 * overlapping an input, or r_out rows that overlap each other, is FK_EINVAL, as is everything fk_absdiff_sums_bf16 refuses. */
int fk_residual_absdiff_sums_bf16(const void* h1, fk_rows r1, const void* h0, fk_rows r0, const void* ref, fk_rows rf, void* r_out,
                                  fk_rows rr, int64_t M, int32_t D, int32_t is_bf16, float* out, float* ws, int64_t ws_floats,
                                  fk_stream_t stream);
/* dst[r, c] = src[c, r] for a [R, C] bf16 matrix with leading dimensions lds/ldd (elements);
 * batched over `batch` with the given batch strides. */
int fk_transpose_bf16(const void* src, int64_t lds, int64_t src_batch_stride, void* dst, int64_t ldd,
                      int64_t dst_batch_stride, int32_t R, int32_t C, int32_t batch, fk_stream_t stream);
/* Single-head attention with head dimension 512, fused (flash-style: nothing of size S x S is stored): the mid-block attention
 * of the FLUX AutoencoderKL (diffusers `Attention` in UNetMidBlock2D, heads = 1, dim_head = 512; reference call sites
 * univa/utils/flux_pipeline.py:604-611 encode, :1127-1129 decode).  q, k, v: bf16 [B, S, >= 512] views with a common row
 * stride ld_qkv (e.g. the three column blocks of one fused [B, S, 1536] projection), o: bf16 [B, S, 512] rows ld_o apart;
 * strides in elements, ld_qkv % 8 == 0, ld_o % 4 == 0; any S >= 1.  o = softmax(scale q k^T) v with fp32 scores and sums. */
int fk_attention_hd512_bf16(const void* q, const void* k, const void* v, int64_t ld_qkv, int64_t batch_stride_qkv, void* o,
                            int64_t ld_o, int64_t batch_stride_o, int32_t B, int32_t S, float scale, fk_stream_t stream);
/* y[r, :n] = bf16(softmax(x[r, :n])) with fp32 scores x (row strides ldx / ldy in elements), n % 4 == 0,
 * n <= 32768: the softmax of the VAE mid-block attention (scores kept in fp32 like a fused SDPA). */
int fk_softmax_rows(const float* x, int64_t ldx, void* y, int64_t ldy, int64_t rows, int32_t n,
                    fk_stream_t stream);

/* FLUX AutoencoderKL pieces (diffusers AutoencoderKL; reference flux_pipeline.py:604-611,1127-1129).
 * Activations are NHWC bf16 with C % 32 == 0 (3- and 16-channel inputs are zero padded to 32). */
typedef struct fk_conv_args {
  const void* x;       /* [B, Hin, Win, Cin] bf16 */
  const void* w;       /* [Cout, KH, KW, Cin] bf16 (repacked from OIHW, Cin zero padded) */
  const void* bias;    /* bf16 [Cout] */
  void* y;             /* [B, Hout, Wout, Cout] bf16 */
  const void* res;     /* optional residual, same layout as y: y = bf16(res + y) */
  int32_t B, Hin, Win, Cin, Cout;
  int32_t ksize;       /* 1 or 3 */
  int32_t stride;      /* 1 or 2 */
  int32_t pad;         /* 3x3: 1 = symmetric pad 1; 0 with stride 2 = F.pad(x,(0,1,0,1)) then valid conv */
  int32_t upsample2x;  /* 1: input is nearest-upsampled 2x on the fly (Upsample2D + conv) */
  int32_t Hout, Wout;
} fk_conv_args;
int fk_conv2d_nhwc_bf16(const fk_conv_args* args, fk_stream_t stream);
/* The 3 x 3 / stride 1 / pad 1 convolutions of ResnetBlock2D / Upsample2D (Cin % 64 == 0) as an LDS halo-tiled MFMA kernel:
 * a workgroup stages the 18 x 18 x 64-channel halo of its 16 x 16 output pixels ONCE per channel chunk and reads the nine
 * taps from LDS.  With gn_stats != NULL (fk_groupnorm_stats_nhwc_bf16 of x) the GroupNorm(gn_groups) + optional SiLU that
 * precedes the convolution in the reference graph (conv(act(norm(x)))) is applied while the halo is staged -- same
 * arithmetic and rounding points as fk_groupnorm_apply_nhwc_bf16, zero padding outside the image AFTER the normalisation --
 * so the normalised activation is never written to memory.  args->res: y = bf16(res + y).  args->upsample2x as above. */
int fk_conv3x3_halo_bf16(const fk_conv_args* args, const float* gn_stats, const void* gn_gamma, const void* gn_beta,
                         int32_t gn_groups, int32_t gn_silu, fk_stream_t stream);
/* Parity build of the same kernel: args->y is fp32 [B, Hout, Wout, Cout] = acc + bias (no residual, no output rounding),
 * so that the halo staging / GroupNorm prologue / tap loop can be held to an fp32 reference at rtol 1e-3 / atol 1e-4. */
int fk_conv3x3_halo_f32_debug(const fk_conv_args* args, const float* gn_stats, const void* gn_gamma, const void* gn_beta,
                              int32_t gn_groups, int32_t gn_silu, fk_stream_t stream);

/* GroupNorm(32 groups, eps) statistics: stats[b, g] = (mean, rstd) fp32; ws: fp32 workspace of
 * fk_groupnorm_ws_floats(B, HW, C) floats. */
int64_t fk_groupnorm_ws_floats(int32_t B, int64_t HW, int32_t C);
int fk_groupnorm_stats_nhwc_bf16(const void* x, float* stats, float* ws, int32_t B, int64_t HW,
                                 int32_t C, int32_t groups, float eps, fk_stream_t stream);
/* y = act(bf16((x - mean) * rstd * gamma + beta)); act = SiLU when silu != 0. */
int fk_groupnorm_apply_nhwc_bf16(const void* x, void* y, const float* stats, const void* gamma,
                                 const void* beta, int32_t B, int64_t HW, int32_t C, int32_t groups,
                                 int32_t silu, fk_stream_t stream);
/* Layout changes at the VAE boundary. src NCHW (fp32 or bf16) -> dst NHWC bf16 with C zero padded to Cpad,
 * applying y = bf16(bf16(bf16(x) / div) + add) (latent un-scaling `z / scaling + shift` of
 * flux_pipeline.py:1128; div = 1, add = 0 is the plain `image.to(vae.dtype)` cast). */
int fk_nchw_to_nhwc_bf16(const void* src, int32_t src_is_fp32, void* dst, int32_t B, int32_t C,
                         int32_t Cpad, int32_t H, int32_t W, float div, float add, fk_stream_t stream);
/* src NHWC bf16 (channel stride Cpad) -> dst NCHW (fp32 or bf16), first C channels,
 * y = bf16(bf16(x + add) * mul)  (`(z - shift) * scaling` of flux_pipeline.py:611). */
int fk_nhwc_to_nchw(const void* src, void* dst, int32_t dst_is_fp32, int32_t B, int32_t C, int32_t Cpad,
                    int32_t H, int32_t W, float add, float mul, fk_stream_t stream);

/* ---- fp32-class encoder (reference: train_denoiser.py:458 loads the VAE in fp32 and :887-918 encodes the target and the
 * condition image with it inside every optimisation step).  Activations are fp32 NHWC; a product a . w runs on the bf16
 * MFMA as the K-concatenation [a_hi | a_lo | a_hi] . [w_hi | w_hi | w_lo] with a_hi = bf16(a), a_lo = bf16(a - a_hi) and
 * fp32 accumulation (parts = 3; parts = 2 drops the third term: exact when the weights ARE bf16 numbers).  The term left
 * out, a_lo . w_lo, is ~2^-16 of the product; tests hold the encoder to the fp32 oracle at rtol 1e-3 / atol 1e-4. ---- */
/* y[r, p * part_stride + c] = part p of x[r, c] (fp32, n % 4 == 0); activation order (hi, lo, hi), or weight order
 * (hi, hi, lo) when weight_order != 0; parts = 2: (hi, lo). */
int fk_split_f32_rows(const float* x, int64_t ldx, void* y, int64_t ldy, int64_t part_stride, int64_t rows, int32_t n,
                      int32_t parts, int32_t weight_order, fk_stream_t stream);
/* GroupNorm(32) (+ SiLU, fp32 expf) of fp32 NHWC x with fp32 gamma / beta, written as the bf16 parts of the fp32 result:
 * y_parts [B, HW, parts * C] = [hi | lo | hi] per pixel -- the operand layout of fk_conv2d_nhwc_f32out / fk_gemm_bf16.
 * stats: [B, 32, 2] fp32 scratch, ws: fk_groupnorm_ws_floats(B, HW, C) floats. */
int fk_groupnorm_f32_nhwc(const float* x, void* y_parts, float* stats, float* ws, const float* gamma, const float* beta,
                          int32_t B, int64_t HW, int32_t C, int32_t groups, float eps, int32_t silu, int32_t parts,
                          fk_stream_t stream);
/* Implicit-GEMM convolution (fk_conv2d_nhwc_bf16's kernel) over operand parts: args->x [B, Hin, Win, Cin] and args->w hold
 * the parts side by side along the channel axis (Cin = parts * C), args->bias / res / y are fp32. */
int fk_conv2d_nhwc_f32out(const fk_conv_args* args, fk_stream_t stream);
/* The same for the 3 x 3 / stride 1 / pad 1 convolutions with parts * C % 64 == 0 on the LDS halo-tiled kernel
 * (fk_conv3x3_halo_bf16's main loop, fp32 epilogue): the operand parts are read once per channel chunk instead of nine times. */
int fk_conv3x3_halo_f32out(const fk_conv_args* args, fk_stream_t stream);
/* src NCHW fp32 -> NHWC bf16 parts [B, HW, parts * Cpad], every part zero padded to Cpad channels. */
int fk_nchw_f32_to_nhwc_parts(const float* src, void* dst, int32_t B, int32_t C, int32_t Cpad, int32_t H, int32_t W,
                              int32_t parts, fk_stream_t stream);
/* src NHWC fp32 (channel stride Cpad) -> dst NCHW fp32, first C channels, y = (x + add) * mul in fp32. */
int fk_nhwc_f32_to_nchw(const float* src, float* dst, int32_t B, int32_t C, int32_t Cpad, int32_t H, int32_t W, float add,
                        float mul, fk_stream_t stream);
/* fk_softmax_rows with the fp32 probability written as the three bf16 parts (hi, lo, hi), part_stride columns apart. */
int fk_softmax_rows_parts(const float* x, int64_t ldx, void* y, int64_t ldy, int64_t part_stride, int64_t rows, int32_t n,
                          fk_stream_t stream);

/* Pixels in: uint8 NHWC [B, Hin, Win, 3] (PIL / numpy layout) -> NHWC bf16 [B, Hout, Wout, Cpad] (channels >= 3 zero),
 * fusing the three host steps the reference runs in front of vae.encode:
 *   `(img / 255 - 0.5) / 0.5` in fp32                    (univa/serve/cli.py:106-109),
 *   VaeImageProcessor.resize on a tensor = F.interpolate(mode="nearest"): src = min(floor(dst * in/out), in - 1)
 *   and VaeImageProcessor.preprocess, which normalises (2x - 1) once more iff the tensor has no negative value
 *   (renorm != 0: the caller checks min(u8) >= 128)      (univa/utils/flux_pipeline.py:960-972),
 *   `image.to(dtype)` = bf16                             (flux_pipeline.py prepare_latents). */
int fk_pixels_u8_to_nhwc_bf16(const void* src, void* dst, int32_t B, int32_t Hin, int32_t Win, int32_t Hout,
                              int32_t Wout, int32_t Cpad, int32_t renorm, fk_stream_t stream);
/* Pixels out: decoder output NCHW (bf16 or fp32) -> uint8 NHWC, VaeImageProcessor.postprocess up to the PIL array
 * (flux_pipeline.py:1130): clamp(x / 2 + 0.5, 0, 1) in the tensor dtype, then rint(float * 255). */
int fk_image_to_u8_nhwc(const void* src, int32_t src_is_fp32, void* dst, int32_t B, int32_t C, int32_t H, int32_t W,
                        fk_stream_t stream);

/* ---- Masked edits on the masked box (pipeline.py: padding_mask_crop / mask_blur / overlay; csrc/mask_ops.hip).  The rules are
 * written from the description of diffusers' VaeImageProcessor.get_crop_region / .blur / .apply_overlay; parity with PIL's
 * GaussianBlur is unpinned (its lanczos / bicubic / bilinear resize is pinned byte for byte: fk_resample_pass_u8 below).  Every product, sum and division below is one fp32 operation (the file is built
 * without contraction) -- except in K3, where each is one fp64 operation; every index is clamped before its load; no atomics.  A refused call returns FK_EINVAL with a message and
 * writes nothing.  K3 and K4 point-sample: a box smaller than the model resolution on the way out, larger on the way in, aliases.
 * The antialiased route is fk_resample_pass_u8 + fk_bytes_overlay_u8 below (pipeline.py: resample=).
 *
 * The bilinear rule (K3, K4), per axis, output position X of n_out over a source of n_in samples:
 *   s = clamp((X + 0.5) * (n_in / n_out) - 0.5, 0, n_in - 1),  i0 = floor(s),  i1 = min(i0 + 1, n_in - 1),  f = s - i0
 *   u = (1-fy) * ((1-fx) * p00 + fx * p01) + fy * ((1-fx) * p10 + fx * p11)
 * Equal sizes give s = X, f = 0 and u = p00 exactly. ---- */

/* K1.  mask [Bm, H, W] uint8 -> out4 = (min x, min y, max x + 1, max y + 1) over all samples of the pixels with byte >= threshold
 * (0..255); (W, H, 0, 0) when there are none.  Per-block partials in `ws` (fk_mask_bbox_ws_ints() int32, caller-owned, one per
 * stream of ordered launches) and a one-block finish.  out4 and ws: device int32, 4-byte aligned. */
int64_t fk_mask_bbox_ws_ints(void);
int fk_mask_bbox_u8(const void* mask, int32_t Bm, int32_t H, int32_t W, int32_t threshold, int32_t* out4, int32_t* ws,
                    int64_t ws_ints, fk_stream_t stream);
/* K2.  Separable Gaussian feather of src [Bm, H, W] uint8 into dst (same shape; dst may be src).  taps: device fp32 [2R + 1],
 * made on the host (helpers.gaussian_taps: R = ceil(3 sigma), float64 exp(-k^2 / (2 sigma^2)) divided by their float64 sum,
 * rounded to fp32), 0 <= R <= FK_MASK_BLUR_MAX_RADIUS.  Horizontal pass into `plane` (caller-owned fp32 [Bm, H, W]):
 *   acc = 0;  for k = -R..R ascending: acc = acc + w[k] * float(src[y, clamp(x + k, 0, W-1)])
 * vertical pass: the same over y on that plane; dst = uint8(rint(clamp(v, 0, 255))).  The order of operations is the contract. */
#define FK_MASK_BLUR_MAX_RADIUS 192
int fk_mask_blur_u8(const void* src, void* dst, float* plane, const float* taps, int32_t R, int32_t Bm, int32_t H, int32_t W,
                    fk_stream_t stream);
/* K3.  fk_pixels_u8_to_nhwc_bf16 reading the source box [x0, x1) x [y0, y1) of src [B, Hin, Win, 3] with the bilinear rule
 * (n_in = the box's side, n_out = Wout / Hout) on the bytes, then that kernel's normalisation, `renorm` flag (the caller checks
 * that every byte of the box is >= 128) and bf16 cast.  Every element is within 1 bf16 ulp of the rule's exact value, which fp32
 * cannot give where the normalised value crosses 0: s, f, u, ((u / 255) - 0.5) / 0.5 and 2v - 1 are evaluated in fp64, in this
 * order, and rounded to fp32, then bf16.  A sample on a source pixel (fx == fy == 0) takes that kernel's fp32 value of the byte
 * (at most 1 bf16 ulp from the fp64 one), so a box that is the whole picture at equal size gives that kernel's bits. */
int fk_pixels_u8_box_to_nhwc_bf16(const void* src, void* dst, int32_t B, int32_t Hin, int32_t Win, int32_t x0, int32_t y0,
                                  int32_t x1, int32_t y1, int32_t Hout, int32_t Wout, int32_t Cpad, int32_t renorm,
                                  fk_stream_t stream);
/* K4.  img: decoder output NCHW [B, 3, h, w] (bf16 or fp32); orig: uint8 [orig_batch, H, W, 3], orig_batch 1 or B; alpha: uint8
 * [alpha_batch, H, W], alpha_batch 1 or B, or NULL (alpha_batch 0) meaning 255 everywhere; dst: uint8 [B, H, W, 3], a buffer of
 * its own.  Outside the box [x0, x1) x [y0, y1): the original's bytes.  Inside, with o the original's byte and a the alpha:
 *   t = fk_image_to_u8_nhwc's clamp(x / 2 + 0.5, 0, 1) per decoded pixel,  g = the bilinear rule from (h, w) to the box on t,
 *   c = g * 255;   a == 0: o, taken;   a == 255: c, taken;   otherwise (a * c + (255 - a) * o) / 255
 * then rint(clamp(., 0, 255)).  The whole picture as the box at equal size with alpha 255 or NULL gives fk_image_to_u8_nhwc's bits. */
int fk_image_overlay_u8(const void* img, int32_t img_is_fp32, int32_t h, int32_t w, const void* orig, int32_t orig_batch,
                        const void* alpha, int32_t alpha_batch, void* dst, int32_t B, int32_t H, int32_t W, int32_t x0, int32_t y0,
                        int32_t x1, int32_t y1, fk_stream_t stream);

/* ---- Antialiased byte resize and byte paste-back (pipeline.py: resample=; csrc/resample.hip).  Pillow's 8-bit resize, written from
 * its behaviour: integer arithmetic on tables made on the host (helpers.resample_coeffs, float64), so the kernels are held to
 * EQUALITY with Pillow's bytes (tests/test_resample_ref.py, tests/test_hip_resample_kernels.py), not to a tolerance.
 *
 * Filters (float64): bilinear 1 - |x| on |x| < 1, support 1;  bicubic with a = -0.5, support 2;  lanczos sinc(x) sinc(x / 3) on
 * -3 <= x < 3 with sinc(x) = sin(pi x) / (pi x), support 3.  Per axis, n_in -> n_out:
 *   scale = n_in / n_out,  fs = max(scale, 1),  support = filter_support * fs,  ksize = ceil(support) * 2 + 1
 * and per output index i:
 *   center = (i + 0.5) * scale,  xmin = max(int(center - support + 0.5), 0),  xmax = min(int(center + support + 0.5), n_in)
 *   w_t = filter((t + xmin - center + 0.5) * (1 / fs)) for t < xmax - xmin, summed in ascending t, each divided by the sum when
 *   the sum is nonzero;  kk_t = int(w_t * 2^22 + 0.5) for w_t >= 0, int(w_t * 2^22 - 0.5) otherwise (int truncates).
 * One pass over an axis, per channel, int32 accumulator, arithmetic shift:
 *   out = clip((2^21 + sum_t kk_t * src[xmin + t]) >> 22, 0, 255)
 * The window is clamped BEFORE the weights are made, so the weights of a cut window are renormalised.  A resize is the horizontal
 * pass into a uint8 intermediate [B, Hin, Wout, C] -- that rounding is part of the rule -- then the vertical pass; a pass whose axis
 * keeps its size is skipped, not run with a one-tap table (ops.resample_u8).  A crop is crop-then-resize: the box is an integer
 * sub-view of the source and windows clamp at the box, so the entry takes a strided view and no box.
 *
 * fk_resample_pass_u8: src is a view of uint8 pixels [B, Hin, Win, C], C 1 or 3, pixels of a row contiguous, rows src_row_stride
 * and samples src_batch_stride bytes apart; dst is contiguous, [B, Hin, n_out, C] for axis 1 (horizontal) and [B, n_out, Win, C] for
 * axis 0 (vertical).  bounds: device int32 [n_out, 2] = (xmin, xmax).  kk: device int32, [n_out, ksize] for axis 0 and TAP-MAJOR
 * [ksize, n_out] for axis 1 (adjacent lanes are adjacent outputs), zero past xmax - xmin.  The caller guarantees
 * 255 * sum_t |kk_t| + 2^21 < 2^31 per output (helpers.resample_coeffs checks it).  Whatever the tables hold, every window is
 * clamped to [0, n_in] and to ksize taps before a load.  Refused with FK_EINVAL and a message, nothing written: a null pointer, C
 * not 1 or 3, a size that is not positive, an axis that is not 0 or 1, ksize < 1 or > FK_RESAMPLE_MAX_KSIZE (lanczos down to 1/85,
 * bilinear to 1/256), rows that overlap, tables that are not 4-byte aligned, dst == src. */
#define FK_RESAMPLE_MAX_KSIZE 513
int fk_resample_pass_u8(const void* src, int64_t src_batch_stride, int64_t src_row_stride, void* dst, int32_t B, int32_t Hin,
                        int32_t Win, int32_t C, int32_t axis, int32_t n_out, const int32_t* bounds, const int32_t* kk,
                        int32_t ksize, fk_stream_t stream);
/* fk_image_overlay_u8 on bytes.  res: uint8 [B, y1 - y0, x1 - x0, 3], the result already at the box's size; orig: uint8
 * [orig_batch, H, W, 3], orig_batch 1 or B; alpha: uint8 [alpha_batch, H, W], alpha_batch 1 or B, or NULL (alpha_batch 0) meaning
 * 255 everywhere; dst: uint8 [B, H, W, 3], a buffer of its own.  Outside the box [x0, x1) x [y0, y1): the original's bytes.  Inside,
 * with o the original's byte, r the result's and a the alpha:
 *   a == 0: o, taken;   a == 255: r, taken;   otherwise (2 * (a * r + (255 - a) * o) + 255) / 510 in integers
 * -- the exact quotient (a r + (255 - a) o) / 255 rounded to nearest; a tie cannot occur.  Parity with PIL's compositing is not
 * claimed. */
int fk_bytes_overlay_u8(const void* res, const void* orig, int32_t orig_batch, const void* alpha, int32_t alpha_batch, void* dst,
                        int32_t B, int32_t H, int32_t W, int32_t x0, int32_t y0, int32_t x1, int32_t y1, fk_stream_t stream);

/* ---- Edit-region loss weights (edit_weights.py: edit_region_weights; csrc/edit_weights.hip).  The per-pixel loss map of the
 * reference's `mask_weight_type` configs (univa/utils/get_mask.py: get_weight_mask), from the (reference, target) bytes on the device.
 * Integer arithmetic only, so every stage is held to EQUALITY with its numpy restatement (tests/edit_weights_ref.py,
 * tests/test_hip_edit_weights_kernels.py).  Parity: the grey conversion is pinned to the installed Pillow; the closing and the
 * labelling are written from OpenCV's documented behaviour (ellipse table, default morphology border, connectivity 8) and
 * cross-checked against scipy; OpenCV itself is not available to the tests, so parity with OpenCV is unpinned.
 *
 * Masks are uint8 planes [N, H, W]; the entries write 0 or 255 and read a byte as white iff it is >= 128.  Sizes: 1 <= H, W <=
 * FK_EDIT_MASK_MAX_SIDE and N * H * W < 2^31 (E4: 8 <= H, W and B <= 65535 as well).  A refused call returns FK_EINVAL with the
 * entry's name in the message and writes nothing. ---- */
#define FK_EDIT_MASK_MAX_SIDE 4096
#define FK_MASK_CLOSE_TILE 32

/* E1.  ref, tgt: uint8 NHWC RGB [N, H, W, 3] (rows need no alignment); the reference pictures lie ref_batch_stride >= H * W * 3
 * bytes apart, so a slice [:, r] of [B, R, H, W, 3] is read in place; dst: uint8 [N, H, W], a buffer of its own.  Per pixel
 *   d_c = |ref_c - tgt_c|,  grey = (19595 d_R + 38470 d_G + 7471 d_B + 32768) >> 16,  dst = 255 iff grey >= threshold (0..256)
 * which is ImageChops.difference(ref, tgt).convert("L").point(lambda v: 255 if v >= threshold else 0), byte for byte. */
int fk_edit_diff_mask_u8(const void* ref, int64_t ref_batch_stride, const void* tgt, void* dst, int32_t N, int32_t H, int32_t W,
                         int32_t threshold, fk_stream_t stream);
/* E2.  Closing with the 5 x 5 ellipse whose rows are 00100 / 11111 / 11111 / 11111 / 00100 (OpenCV's MORPH_ELLIPSE (5, 5)):
 * dilation first (white iff any pixel under the element is white), then erosion (white iff every pixel under it is).  Positions
 * outside the plane are not counted in either pass: a border never dilates and never erodes.  One block closes one
 * FK_MASK_CLOSE_TILE-square tile at a time from LDS; dst is a buffer of its own. */
int fk_mask_close5_u8(const void* src, void* dst, int32_t N, int32_t H, int32_t W, fk_stream_t stream);
/* E3.  The white pixels of each plane are labelled by 8-connectivity (planes never connect); a component survives iff
 *   keep_den * area >= keep_num * (white pixels of its plane)        (int64 products; keep_num >= 0, keep_den >= 1)
 * -- the denominator is the plane's WHITE count, not H * W.  For keep 3 / 10 this is the reference's float64 test
 * area >= 0.3 * total: at a tie 0.3 * total rounds to the integer itself and the component is kept (tests/test_edit_weights_ref.py).
 * dst may be src.  ws: fk_mask_components_ws_bytes(N, H, W) bytes, caller-owned, 4-byte aligned, one per stream of ordered
 * launches: int32 [0] the status word, [1, 1 + N) the planes' white counts, then the labels and the areas, N * H * W each.
 * Labelling: the first pixel of every horizontal run labels the run with its own index in [N, H, W]; every white pixel then joins
 * the run above it (straight above, else the two diagonals) by pointing the larger root at the smaller with atomicMin; a pass takes
 * every pixel to its root, which is the least index of its component whatever order the atomics took; areas and white counts are
 * atomicAdd sums of run lengths.  Two launches give the same bytes.  Every loop has a bound from the plane's size: a run W steps,
 * a chain of parents (strictly decreasing inside one plane) H * W, the retries of a union (the larger index in hand falls with each)
 * H * W.  A loop that reaches its bound, or meets a label that is none, sets the status word and stops: never a hang; the loops of
 * the other lanes look at the word (a chase every 256 steps, a union before each try) and give up too.  The entry
 * itself reads nothing back; fk_mask_components_status(ws) waits for the stream, reads the word and returns FK_EBOUND when it is
 * set, and E4 carries it to the host inside its counts. */
int64_t fk_mask_components_ws_bytes(int32_t N, int32_t H, int32_t W);   /* 0 for sizes the entry refuses */
int fk_mask_filter_components_u8(const void* src, void* dst, int32_t N, int32_t H, int32_t W, int32_t keep_num, int32_t keep_den,
                                 int32_t* ws, int64_t ws_bytes, fk_stream_t stream);
int fk_mask_components_status(const int32_t* ws, fk_stream_t stream);
/* E4.  masks: uint8 [B, R, H, W], R >= 1.  Per sample b: the AND over its R planes; counts[b, 0] = its white pixels; when that is
 * 0 the all-white plane takes its place (the reference's "reconstruction data" rule, decided on the device); 8 x 8 / stride-8 max
 * pool with floor sizes (F.max_pool2d) into pooled [B, H / 8, W / 8]; E2 of pooled into mask_ds; counts[b, 1] = the white pixels
 * of mask_ds.  counts: device int32 [B, 2], cleared here.  status: NULL, or E3's workspace: when its status word is set every
 * count is written as -1, so the caller's one read-back of counts shows a labelling that reached a bound.  pooled and mask_ds are
 * caller-owned buffers of their own. */
int fk_mask_and_pool8_u8(const void* masks, int32_t B, int32_t R, int32_t H, int32_t W, void* pooled, void* mask_ds, int32_t* counts,
                         const int32_t* status, fk_stream_t stream);
/* E5.  dst fp32 [B, 1, h, w] = w[b] where mask_ds [B, h, w] is white, 1.0f elsewhere.  w: device fp32 [B]. */
int fk_mask_weight_fill_f32(const void* mask_ds, const float* w, float* dst, int32_t B, int32_t h, int32_t wd, fk_stream_t stream);

/* ---- LoRA merge (transformer.py: load_lora_adapter / set_adapters / set_lora_scale; the reference's pipeline is a
 * FluxLoraLoaderMixin, univa/utils/flux_pipeline.py:195).  Adapters become part of a bf16 weight [N, K]:
 *   out[n, k] = bf16_rne( float(base[n, k]) + sum_t scale_t * acc_t[n, k] ),  acc_t[n, k] = sum_j up_t[n, j] * down_t[j, k]
 * acc_t accumulated in fp32 on the bf16 MFMA, the terms added in ascending t (one fp32 fma each).  Row strides in elements,
 * rows contiguous.  out may BE base (same pointer and row stride: every element is read and written by one lane); otherwise
 * out overlaps nothing.  base, up and down are never written.  A term whose scale is 0 adds nothing: all scales 0 gives
 * base's bits.  Supported: N >= 1; K >= 8, K % 8 == 0; ld_* >= the row length; 1 <= rank <= FK_LORA_MAX_RANK;
 * 1 <= n_terms <= FK_LORA_MAX_TERMS; anything else returns FK_EINVAL / FK_EUNSUPPORTED and writes nothing.  `terms` is a
 * HOST array, copied into the launch by value. ---- */
#define FK_LORA_MAX_TERMS 4
#define FK_LORA_MAX_RANK 128
typedef struct fk_lora_term {
  const void* up;   /* bf16 [N, rank]  (lora_B) */
  int64_t ld_up;
  const void* down; /* bf16 [rank, K]  (lora_A) */
  int64_t ld_down;
  int32_t rank;
  float scale;
} fk_lora_term;
int fk_lora_merge_bf16(const void* base, int64_t ld_base, void* out, int64_t ld_out, int32_t N, int32_t K,
                       const fk_lora_term* terms, int32_t n_terms, fk_stream_t stream);

/* ---- LoRA gradient projection (train_step.py: DenoiserTrainStep(lora=...)).  The chain rule through the merge
 * W = bf16(W_base + scale * up . down), straight through its one bf16 rounding, from the weight gradient dw [N, K]:
 *   d_up  [n, j] = scale * sum_k dw[n, k] * down[j, k]          d_down[j, k] = scale * sum_n up[n, j] * dw[n, k]
 * dw, up [N, rank] (lora_B), down [rank, K] (lora_A): bf16, rows contiguous, row strides in elements (dw may be a row block of a
 * wider buffer).  d_up [N, rank] and d_down [rank, K]: fp32, contiguous.  Products on the bf16 MFMA with fp32 accumulation, the
 * rank zero-padded to 32, the reduction index to the kernel's step; scale multiplies the finished sum once.  No atomics: every
 * output element is written once by a sum whose order is fixed by (N, K, rank) alone (csrc/lora_grad.hip states it).  When a
 * reduction is split over workgroups the unscaled partials go through `ws`, fk_lora_grad_ws_floats(N, K, rank) floats (0 when
 * nothing is split: ws may then be NULL); one workspace per stream of ordered launches.  The inputs are never written; outputs
 * and workspace overlap nothing.  Supported: N >= 1, K >= 1, ld_* >= the row length, 1 <= rank <= FK_LORA_MAX_RANK, a finite
 * scale; anything else returns FK_EINVAL / FK_EUNSUPPORTED and writes nothing. ---- */
int64_t fk_lora_grad_ws_floats(int32_t N, int32_t K, int32_t rank);
int fk_lora_grad_bf16(const void* dw, int64_t ld_dw, const void* up, int64_t ld_up, const void* down, int64_t ld_down,
                      int32_t N, int32_t K, int32_t rank, float scale, float* d_up, float* d_down, float* ws,
                      int64_t ws_floats, fk_stream_t stream);
/* The same projection with a choice of what happens to the outputs (gradient accumulation over micro-batches; train_step.py:
 * DenoiserTrainStep(lora=..., data_parallel=True)).  accumulate = 0: overwrite -- exactly fk_lora_grad_bf16, the outputs are never
 * read (they may hold NaN bits).  accumulate = 1: d_up[n, j] = d_up_old[n, j] + scale * sum_k ..., likewise d_down; the thread
 * that owns an element reads it once and writes it once, where the scaled value is formed (the final store of an unsplit role, the
 * reduction of a split one; partials are never added to).  Still no atomics and an order fixed by (N, K, rank): two identical call
 * sequences give the same bits.  The outputs need only 4-byte alignment (views anywhere inside a flat fp32 buffer).  Any other
 * value of accumulate returns FK_EINVAL and writes nothing. */
int fk_lora_grad_acc_bf16(const void* dw, int64_t ld_dw, const void* up, int64_t ld_up, const void* down, int64_t ld_down,
                          int32_t N, int32_t K, int32_t rank, float scale, float* d_up, float* d_down, int32_t accumulate,
                          float* ws, int64_t ws_floats, fk_stream_t stream);

/* ---- Factored LoRA gradient (train_step.py: DenoiserTrainStep(lora=..., lora_backward="factored")): the same two gradients from
 * the linear's own backward operands, without the weight gradient dw = dy^T x:
 *   d_up[n, j] = scale * sum_m dy[m, n] * T[m, j],  T = x down^T      d_down[j, k] = scale * sum_m U[m, j] * x[m, k],  U = dy up
 * x [B, R, K] and dy [B, R, N]: bf16 views, last dimension contiguous, a row stride ld_* and a batch stride bs_* (>= 0) each, in
 * elements (the image rows of a joint [B, S, *] buffer, a column block of a wider one; M = B * R is any value >= 1).  up [N, rank],
 * down [rank, K]: bf16, rows contiguous.  d_up [N, rank], d_down [rank, K]: fp32, contiguous, 4-byte aligned.  All products on the
 * bf16 MFMA with fp32 accumulation; T and U pass through the workspace as split-bf16 pairs hi = bf16(t), lo = bf16(t - hi)
 * (|t - hi - lo| <= 2^-18 |t|), both multiplied into one accumulator; scale multiplies the finished sum once.  No atomics, the order
 * fixed by (B, R, N, K, rank) alone (csrc/lora_side_grad.hip states it): two launches give the same bits.  accumulate = 0: overwrite,
 * the outputs are never read (they may hold NaN bits); accumulate = 1: the scaled sum is added to the old value, each element read
 * once and written once by its owner; any other value is FK_EINVAL.  ws: fk_lora_side_grad_ws_floats(B, R, N, K, rank) floats
 * (0 for unsupported arguments), 4-byte aligned, one per stream of ordered launches.  Inputs are never written; outputs and
 * workspace overlap nothing.  Supported: 1 <= rank <= FK_LORA_MAX_RANK, ld_* >= the row length, a finite scale; anything else
 * returns FK_EINVAL / FK_EUNSUPPORTED and writes nothing. ---- */
int64_t fk_lora_side_grad_ws_floats(int64_t B, int64_t R, int64_t N, int64_t K, int64_t rank);
int fk_lora_side_grad_bf16(const void* x, int64_t ld_x, int64_t bs_x, const void* dy, int64_t ld_dy, int64_t bs_dy, int64_t B,
                           int64_t R, int64_t N, int64_t K, const void* up, int64_t ld_up, const void* down, int64_t ld_down,
                           int64_t rank, float scale, float* d_up, float* d_down, int accumulate, float* ws, int64_t ws_floats,
                           fk_stream_t stream);

const char* fk_last_error(void);
/* Build identification: "fk <version> gfx950". */
const char* fk_version(void);

#ifdef __cplusplus
}
#endif
#endif /* FK_H_ */
