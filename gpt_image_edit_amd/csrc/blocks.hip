// Block-level entry points of the C ABI (SURVEY.md section 8b lists `fk_double_block_fwd`, `fk_single_block_fwd`,
// `fk_mmdit_fwd` beside the per-kernel calls): ONE call enqueues every launch of a FluxTransformerBlock /
// FluxSingleTransformerBlock (diffusers 0.32.2, reached from reference flux_pipeline.py:1067-1077), or of all the blocks of a
// forward, on the caller's stream.  Host code only: it fills the argument structs of the per-kernel entry points exactly as
// the Python adaptor does (gpt_image_edit_amd/ops.py: `rows_of` addressing of the text / image slices of the joint buffers,
// split-K and stream-K workspaces) and calls them in the adaptor's order, so the launches -- and therefore the results --
// are the same bit for bit (tests/test_hip_mmdit.py::test_block_entry_points_give_the_same_bits).  What it removes is host
// work: ~5 400 ctypes calls per edit become 57 x 28 (per-block form) or 28 (whole-stack form).
#include "fk_common.h"

namespace {

constexpr int HD = 128;

struct Dims {
  int B, S_txt, S_img, S, H, D;
};

// a [B, R, cols] slice (rows [r0, r0 + R) of every batch, columns from c0) of a joint [B, S, ld] buffer
struct View {
  const void* p;
  fk_rows r;
};
View view(const void* base, const Dims& d, int64_t ld, int64_t r0, int64_t R, int64_t c0) {
  return View{(const char*)base + (r0 * ld + c0) * 2, fk_rows{ld, R, (int64_t)d.S * ld}};
}

void set_ws(fk_gemm_args& g, const fk_block_ws& ws) {   // ops._gemm_args: only the shapes the planner may split get the workspace
  if (g.K >= 6144 && g.N % 256 == 0 && (int64_t)g.M <= 256ll * ws.splitk_slots && ws.splitk_ws) {
    g.splitk_ws = ws.splitk_ws;
    g.splitk_slots = ws.splitk_slots;
  }
}

// launch controls of the block's GEMMs (fk_block_ws.gemm_*): a grouped launch reads them from its first problem
void ctl(fk_gemm_args& g, const fk_block_ws& ws) {
  g.variant = ws.gemm_variant; g.plan = ws.gemm_plan; g.group_m = ws.gemm_group_m; g.mfma = ws.gemm_mfma;
  g.variant_used = ws.gemm_variant_used;
}

fk_gemm_args gemm(const View& a, const void* w, const void* bias, const View& c, int M, int N, int K, int epi) {
  fk_gemm_args g = {};
  g.A = a.p; g.a = a.r;
  g.W = w; g.ldw = K;
  g.bias = bias;
  g.C = (void*)c.p; g.c = c.r;
  g.M = M; g.N = N; g.K = K;
  g.epilogue = epi;
  g.alpha = 1.0f;
  return g;
}
void gate_res(fk_gemm_args& g, const View& res, const void* gate, int64_t gate_bs, int64_t rows_per_batch) {
  g.res = res.p; g.r = res.r;
  g.gate = gate; g.gate_batch_stride = gate_bs; g.gate_rows_per_batch = rows_per_batch;
}
void qkv_epi(fk_gemm_args& g, const fk_block_ws& ws, const Dims& d, const void* wq, const void* wk, int s_offset) {
  g.q_out = ws.q; g.k_out = ws.k; g.wq = wq; g.wk = wk; g.rope_cs = ws.rope_cs;
  g.qkv_s_offset = s_offset; g.qkv_s_total = d.S; g.qkv_heads = d.H;
}

int check_ws(const fk_block_ws* ws, Dims& d, const char* who) {
  FK_CHECK_ARG(ws != nullptr, "%s: null workspace", who);
  FK_CHECK_ARG(ws->B > 0 && ws->S_txt >= 0 && ws->S_img > 0 && ws->H > 0, "%s: bad B / S_txt / S_img / H %d %d %d %d", who, ws->B,
               ws->S_txt, ws->S_img, ws->H);
  FK_CHECK_ARG(ws->s && ws->n && ws->qkv && ws->q && ws->k && ws->rope_cs, "%s: null activation buffer", who);
  d = Dims{ws->B, ws->S_txt, ws->S_img, ws->S_txt + ws->S_img, ws->H, ws->H * HD};
  FK_CHECK_ARG((int64_t)d.B * d.S < (1ll << 31), "%s: B * S too large", who);
  return FK_OK;
}

#define FK_TRY(expr)          \
  do {                        \
    const int rc_ = (expr);   \
    if (rc_ != FK_OK) return rc_; \
  } while (0)

// MXFP8 form of a block's launch (fk_*_fwd_mx): the quantized-activation workspace and this launch's weight pairs
struct Mx {
  const fk_mx_ws* ws;
  const fk_mx_pair* w;   // one per problem of the launch
};

// launch controls of one MXFP8 GEMM problem a (a copy of the bf16 problem: set_ws / ctl already applied; g0 = the launch's first
// problem, which carries the controls).  fk_mx_ws.splitk == 0: no workspace, every control zero -- the launches MXFP8 shipped with.
// Otherwise the long-K problems keep the split-K workspace set_ws gave them and the block's plan, so fk_gemm_mxfp8's launch plan
// may split them; the other controls (variant, group_m, mfma) have no MXFP8 meaning and stay zero.
void mx_launch_controls(fk_gemm_args& a, const fk_gemm_args& g0, const fk_mx_ws& m) {
  const bool sk = m.splitk != 0 && a.splitk_ws != nullptr;
  if (!sk) { a.splitk_ws = nullptr; a.splitk_slots = 0; }
  a.variant = 0; a.plan = sk ? g0.plan : 0; a.group_m = 0; a.mfma = 0;
}

// one GEMM launch of a block: the bf16 call as it always was, or (mx) each problem's activation quantized into the workspace,
// the img rows first, then the mxfp8 GEMM on the pre-quantized weights with the same epilogue fields
int block_gemm(fk_gemm_args* g, int n, const Mx* mx, fk_stream_t st) {
  if (!mx) return n == 1 ? fk_gemm_bf16(g, st) : fk_gemm_bf16_grouped(g, n, st);
  fk_gemm_mxfp8_args a[2] = {};
  int64_t qo = 0, so = 0;
  for (int i = 0; i < n; ++i) {
    const int K = g[i].K;
    FK_CHECK_ARG(mx->w[i].q && mx->w[i].s, "fk_*_block_fwd_mx: null quantized weight");
    FK_CHECK_ARG(qo + (int64_t)g[i].M * K <= mx->ws->q_bytes && so + (int64_t)g[i].M * (K / 32) <= mx->ws->s_bytes,
                 "fk_*_block_fwd_mx: quantized-activation workspace too small (%lld / %lld bytes)", (long long)mx->ws->q_bytes,
                 (long long)mx->ws->s_bytes);
    void* q = (char*)mx->ws->q + qo;
    void* s = (char*)mx->ws->s + so;
    FK_TRY(fk_quantize_mxfp8(g[i].A, g[i].a, g[i].M, K, q, K, s, K / 32, st));
    if (mx->ws->quantize_launches) ++*mx->ws->quantize_launches;
    a[i].g = g[i];
    a[i].g.A = nullptr; a[i].g.W = nullptr;
    mx_launch_controls(a[i].g, g[0], *mx->ws);
    a[i].A8 = q; a[i].lda8 = K; a[i].A_scale = s; a[i].lda_scale = K / 32;
    a[i].W8 = mx->w[i].q; a[i].ldw8 = K; a[i].W_scale = mx->w[i].s; a[i].ldw_scale = K / 32;
    qo += (int64_t)g[i].M * K;
    so += (int64_t)g[i].M * (K / 32);
  }
  return fk_gemm_mxfp8_grouped(a, n, st);
}

// ---- fused MXFP8 schedule (fk_mx_ws.fused): the producers emit the quantized operand themselves -------------------------------
// a dense quantized operand in the workspace: rows of K bytes at q, of K / 32 scale bytes at s
struct Q8 {
  uint8_t *q, *s;
  int64_t ld, lds;
};
Q8 q8_at(const fk_mx_ws& m, int64_t byte_off, int64_t ld) {
  return Q8{(uint8_t*)m.q + byte_off, (uint8_t*)m.s + byte_off / 32, ld, ld / 32};
}
Q8 q8_rows(const Q8& a, int64_t row0) { return Q8{a.q + row0 * a.ld, a.s + row0 * a.lds, a.ld, a.lds}; }

// the mxfp8 form of problem g (epilogue fields kept) on the pre-quantized operand a8 and weight pair w
int mx_problem(fk_gemm_mxfp8_args& a, const fk_gemm_args& g, const fk_gemm_args& g0, const fk_mx_ws& m, const Q8& a8,
               const fk_mx_pair& w) {
  FK_CHECK_ARG(w.q && w.s, "fk_*_block_fwd_mx: null quantized weight");
  a = fk_gemm_mxfp8_args{};
  a.g = g;
  a.g.A = nullptr; a.g.W = nullptr;
  mx_launch_controls(a.g, g0, m);
  a.A8 = a8.q; a.lda8 = a8.ld; a.A_scale = a8.s; a.lda_scale = a8.lds;
  a.W8 = w.q; a.ldw8 = g.K; a.W_scale = w.s; a.ldw_scale = g.K / 32;
  return FK_OK;
}
// n problems (img first) on pre-quantized operands; out: their quantized outputs (nullptr: the bf16 epilogue of g)
int mx_gemm(const fk_mx_ws& m, const fk_gemm_args* g, int n, const Q8* a8, const fk_mx_pair* w, const Q8* out, int64_t col_offset,
            fk_stream_t st) {
  if (!out) {
    fk_gemm_mxfp8_args a[2];
    for (int i = 0; i < n; ++i) FK_TRY(mx_problem(a[i], g[i], g[0], m, a8[i], w[i]));
    return fk_gemm_mxfp8_grouped(a, n, st);
  }
  fk_gemm_mxfp8_q_args a[2];
  for (int i = 0; i < n; ++i) {
    FK_TRY(mx_problem(a[i].a, g[i], g[0], m, a8[i], w[i]));
    a[i].a.g.C = nullptr;
    a[i].Q = out[i].q; a[i].ldq = out[i].ld; a[i].Q_scale = out[i].s; a[i].ldq_scale = out[i].lds;
    a[i].col_offset = col_offset;
  }
  return fk_gemm_mxfp8_q_grouped(a, n, st);
}
// the standalone quantizer on a bf16 view (what is left of it in the fused schedule: the attention output)
int quantize_view(const fk_mx_ws& m, const View& x, int64_t M, int K, const Q8& o, fk_stream_t st) {
  FK_TRY(fk_quantize_mxfp8(x.p, x.r, M, K, o.q, o.ld, o.s, o.lds, st));
  if (m.quantize_launches) ++*m.quantize_launches;
  return FK_OK;
}
// fk_mx_ws.fused bit 1: the attention writes the quantized rows itself (stream A = rows [0, split) -> a, stream B = the rest -> b;
// split = 0: everything to a).  FK_EUNSUPPORTED (no MXFP8 form of the selected attention kernel) comes back to the caller, which
// then takes the bf16 attention + quantizer route; nothing has been launched at that point.
int attention_mx(const fk_block_ws& ws, const Dims& d, const Q8& a, const Q8* b, int split, fk_stream_t st) {
  const int D = d.D;
  const fk_attn_mx_out out = {a.q, a.s, b ? b->q : nullptr, b ? b->s : nullptr, split, a.ld, a.lds};
  return fk_attention_fwd_ws_mxfp8(ws.q, ws.k, (const char*)ws.qkv + (int64_t)2 * D * 2, nullptr, d.B, d.H, d.S, 3 * D,
                                   (int64_t)d.S * 3 * D, 0.08838834764831845f, &out, ws.attn_ws, ws.attn_ws_bytes, ws.attn_grid, st);
}
// the workspace holds n8 (D bytes per row) and the block's consumer operand (operand_cols bytes per row) at once
int check_fused_ws(const fk_mx_ws& m, const Dims& d, int operand_cols, const char* who) {
  const int64_t need = (int64_t)d.B * d.S * (d.D + (int64_t)operand_cols);
  FK_CHECK_ARG(m.q_bytes >= need && m.s_bytes >= need / 32,
               "%s: the fused schedule needs a quantized-activation workspace of %lld + %lld bytes (given %lld + %lld)", who,
               (long long)need, (long long)(need / 32), (long long)m.q_bytes, (long long)m.s_bytes);
  return FK_OK;
}

int double_block_fused(const fk_block_ws& ws, const Dims& d, const fk_double_block_weights& w, const void* mod, int64_t mod_bs,
                       fk_stream_t st, const fk_mx_ws& mxws, const fk_double_block_weights_mx& wx) {
  FK_CHECK_ARG(ws.o && d.S_txt > 0, "fk_double_block_fwd_mx: needs the o buffer and a text stream");
  FK_TRY(check_fused_ws(mxws, d, 4 * d.D, "fk_double_block_fwd_mx"));
  const int D = d.D, B = d.B, Mi = B * d.S_img, Mt = B * d.S_txt;
  const char* mi = (const char*)mod + w.mod_off_img * 2;
  const char* mt = (const char*)mod + w.mod_off_txt * 2;
  auto chunk = [&](const char* m, int j) { return (const void*)(m + (int64_t)j * D * 2); };
  const View s_all = view(ws.s, d, D, 0, d.S, 0);
  const View h = view(ws.s, d, D, d.S_txt, d.S_img, 0), cx = view(ws.s, d, D, 0, d.S_txt, 0);
  const View none = View{nullptr, fk_rows{0, 0, 0}};
  const int64_t M = (int64_t)B * d.S;
  // every operand: the img rows first, then the txt rows (each stream dense, batch-major)
  const Q8 n8 = q8_at(mxws, 0, D), o8 = q8_at(mxws, M * D, D), ff8 = q8_at(mxws, M * D, 4 * D);
  const Q8 n8s[2] = {n8, q8_rows(n8, Mi)}, o8s[2] = {o8, q8_rows(o8, Mi)}, ff8s[2] = {ff8, q8_rows(ff8, Mi)};
  FK_TRY(fk_ln_modulate2_mxfp8(s_all.p, s_all.r, n8s[1].q, n8s[1].s, n8s[0].q, n8s[0].s, n8.ld, n8.lds, chunk(mt, 0), chunk(mt, 1),
                               chunk(mi, 0), chunk(mi, 1), d.S_txt, mod_bs, d.S, M, D, ws.eps, st));
  {
    fk_gemm_args g[2];
    g[0] = gemm(none, nullptr, w.bqkv_img, view(ws.qkv, d, 3 * D, d.S_txt, d.S_img, 0), Mi, 3 * D, D, FK_EPI_QKV);
    qkv_epi(g[0], ws, d, w.norm_q, w.norm_k, d.S_txt);
    g[1] = gemm(none, nullptr, w.bqkv_txt, view(ws.qkv, d, 3 * D, 0, d.S_txt, 0), Mt, 3 * D, D, FK_EPI_QKV);
    qkv_epi(g[1], ws, d, w.norm_added_q, w.norm_added_k, 0);
    ctl(g[0], ws); FK_TRY(mx_gemm(mxws, g, 2, n8s, &wx.qkv_img, nullptr, 0, st));
  }
  // o8: txt rows (stream A, split = S_txt) behind the img rows (stream B), from the attention itself or through the quantizer
  const int rc_mx = (mxws.fused & 2) ? attention_mx(ws, d, o8s[1], &o8s[0], d.S_txt, st) : FK_EUNSUPPORTED;
  if (rc_mx != FK_EUNSUPPORTED) FK_TRY(rc_mx);
  else {
    FK_TRY(fk_attention_fwd_ws_bf16(ws.q, ws.k, (const char*)ws.qkv + (int64_t)2 * D * 2, ws.o, nullptr, B, d.H, d.S, 3 * D,
                                    (int64_t)d.S * 3 * D, D, (int64_t)d.S * D, 0.08838834764831845f, ws.attn_ws, ws.attn_ws_bytes, ws.attn_grid, st));
    const View oi = view(ws.o, d, D, d.S_txt, d.S_img, 0), ot = view(ws.o, d, D, 0, d.S_txt, 0);
    FK_TRY(quantize_view(mxws, oi, Mi, D, o8s[0], st));
    FK_TRY(quantize_view(mxws, ot, Mt, D, o8s[1], st));
  }
  {
    fk_gemm_args g[2];
    g[0] = gemm(none, nullptr, w.b_out, h, Mi, D, D, FK_EPI_GATE_RES);
    gate_res(g[0], h, chunk(mi, 2), mod_bs, d.S_img);
    g[1] = gemm(none, nullptr, w.b_add_out, cx, Mt, D, D, FK_EPI_GATE_RES);
    gate_res(g[1], cx, chunk(mt, 2), mod_bs, d.S_txt);
    ctl(g[0], ws); FK_TRY(mx_gemm(mxws, g, 2, o8s, &wx.out, nullptr, 0, st));
  }
  FK_TRY(fk_ln_modulate2_mxfp8(s_all.p, s_all.r, n8s[1].q, n8s[1].s, n8s[0].q, n8s[0].s, n8.ld, n8.lds, chunk(mt, 3), chunk(mt, 4),
                               chunk(mi, 3), chunk(mi, 4), d.S_txt, mod_bs, d.S, M, D, ws.eps, st));
  {
    fk_gemm_args g[2];
    g[0] = gemm(none, nullptr, w.b_ff1, none, Mi, 4 * D, D, FK_EPI_GELU_TANH);
    g[1] = gemm(none, nullptr, w.b_ff1_ctx, none, Mt, 4 * D, D, FK_EPI_GELU_TANH);
    ctl(g[0], ws); FK_TRY(mx_gemm(mxws, g, 2, n8s, &wx.ff1, ff8s, 0, st));
  }
  {
    fk_gemm_args g[2];
    g[0] = gemm(none, nullptr, w.b_ff2, h, Mi, D, 4 * D, FK_EPI_GATE_RES);
    gate_res(g[0], h, chunk(mi, 5), mod_bs, d.S_img);
    g[1] = gemm(none, nullptr, w.b_ff2_ctx, cx, Mt, D, 4 * D, FK_EPI_GATE_RES);
    gate_res(g[1], cx, chunk(mt, 5), mod_bs, d.S_txt);
    set_ws(g[0], ws); set_ws(g[1], ws);
    ctl(g[0], ws); FK_TRY(mx_gemm(mxws, g, 2, ff8s, &wx.ff2, nullptr, 0, st));
  }
  return FK_OK;
}

int single_block_fused(const fk_block_ws& ws, const Dims& d, const fk_single_block_weights& w, const void* mod, int64_t mod_bs,
                       fk_stream_t st, const fk_mx_ws& mxws, const fk_single_block_weights_mx& wx) {
  FK_CHECK_ARG(ws.cat != nullptr, "fk_single_block_fwd_mx: needs the [attn | mlp] buffer");
  FK_TRY(check_fused_ws(mxws, d, 5 * d.D, "fk_single_block_fwd_mx"));
  const int D = d.D, B = d.B;
  const int Ms = B * d.S;
  const char* m0 = (const char*)mod + w.mod_off * 2;     // shift, scale, gate
  auto chunk = [&](int j) { return (const void*)(m0 + (int64_t)j * D * 2); };
  const View s_all = view(ws.s, d, D, 0, d.S, 0);
  const View none = View{nullptr, fk_rows{0, 0, 0}};
  const Q8 n8 = q8_at(mxws, 0, D), cat8 = q8_at(mxws, (int64_t)Ms * D, 5 * D);
  // n8 once: the QKV and the MLP-up GEMM read the same quantized rows
  FK_TRY(fk_ln_modulate_mxfp8(s_all.p, s_all.r, n8.q, n8.ld, n8.s, n8.lds, chunk(0), chunk(1), mod_bs, d.S, (int64_t)Ms, D, ws.eps, st));
  {
    fk_gemm_args g = gemm(none, nullptr, w.bqkv, view(ws.qkv, d, 3 * D, 0, d.S, 0), Ms, 3 * D, D, FK_EPI_QKV);
    qkv_epi(g, ws, d, w.norm_q, w.norm_k, 0);
    ctl(g, ws); FK_TRY(mx_gemm(mxws, &g, 1, &n8, &wx.qkv, nullptr, 0, st));
  }
  // columns [0, D) of cat8 from the attention output (directly, or bf16 cat[:, :D] through the quantizer), columns [D, 5D)
  // straight from the MLP-up GEMM's epilogue
  const int rc_mx = (mxws.fused & 2) ? attention_mx(ws, d, cat8, nullptr, 0, st) : FK_EUNSUPPORTED;
  if (rc_mx != FK_EUNSUPPORTED) FK_TRY(rc_mx);
  else {
    FK_TRY(fk_attention_fwd_ws_bf16(ws.q, ws.k, (const char*)ws.qkv + (int64_t)2 * D * 2, ws.cat, nullptr, B, d.H, d.S, 3 * D,
                                    (int64_t)d.S * 3 * D, 5 * D, (int64_t)d.S * 5 * D, 0.08838834764831845f, ws.attn_ws,
                                    ws.attn_ws_bytes, ws.attn_grid, st));
    const View att = view(ws.cat, d, 5 * D, 0, d.S, 0);
    FK_TRY(quantize_view(mxws, att, Ms, D, cat8, st));
  }
  {
    fk_gemm_args g = gemm(none, nullptr, w.b_mlp, none, Ms, 4 * D, D, FK_EPI_GELU_TANH);
    ctl(g, ws); FK_TRY(mx_gemm(mxws, &g, 1, &n8, &wx.mlp, &cat8, D, st));
  }
  {
    fk_gemm_args g = gemm(none, nullptr, w.b_out, s_all, Ms, D, 5 * D, FK_EPI_GATE_RES);
    gate_res(g, s_all, chunk(2), mod_bs, d.S);
    set_ws(g, ws);
    ctl(g, ws); FK_TRY(mx_gemm(mxws, &g, 1, &cat8, &wx.out, nullptr, 0, st));
  }
  return FK_OK;
}

int double_block(const fk_block_ws& ws, const Dims& d, const fk_double_block_weights& w, const void* mod, int64_t mod_bs,
                 fk_stream_t st, const fk_mx_ws* mxws = nullptr,
                 const fk_double_block_weights_mx* wx = nullptr) {
  if (mxws && wx && mxws->fused) return double_block_fused(ws, d, w, mod, mod_bs, st, *mxws, *wx);
  FK_CHECK_ARG(ws.o && ws.ff && d.S_txt > 0, "fk_double_block_fwd: needs the o / ff buffers and a text stream");
  // the img / txt weight pairs of a launch are adjacent members of fk_double_block_weights_mx (qkv_img | qkv_txt, out | add_out, ...)
  Mx mxc;
  auto mx = [&](const fk_mx_pair* pair) -> const Mx* { if (!pair) return nullptr; mxc = Mx{mxws, pair}; return &mxc; };
  const int D = d.D, B = d.B, Mi = B * d.S_img, Mt = B * d.S_txt;
  const char* mi = (const char*)mod + w.mod_off_img * 2;     // shift, scale, gate, shift_mlp, scale_mlp, gate_mlp: D each
  const char* mt = (const char*)mod + w.mod_off_txt * 2;
  auto chunk = [&](const char* m, int j) { return (const void*)(m + (int64_t)j * D * 2); };
  const View s_all = view(ws.s, d, D, 0, d.S, 0), n_all = view(ws.n, d, D, 0, d.S, 0);
  const View h = view(ws.s, d, D, d.S_txt, d.S_img, 0), cx = view(ws.s, d, D, 0, d.S_txt, 0);
  const View n_img = view(ws.n, d, D, d.S_txt, d.S_img, 0), n_txt = view(ws.n, d, D, 0, d.S_txt, 0);
  const int64_t M = (int64_t)B * d.S;
  // text + image streams share every launch: joint LN + modulate, grouped GEMMs (one grid, two weights)
  FK_TRY(fk_ln_modulate2_bf16(s_all.p, s_all.r, (void*)n_all.p, n_all.r, chunk(mt, 0), chunk(mt, 1), chunk(mi, 0), chunk(mi, 1),
                              d.S_txt, mod_bs, d.S, M, D, ws.eps, st));
  {
    fk_gemm_args g[2];
    g[0] = gemm(n_img, w.wqkv_img, w.bqkv_img, view(ws.qkv, d, 3 * D, d.S_txt, d.S_img, 0), Mi, 3 * D, D, FK_EPI_QKV);
    qkv_epi(g[0], ws, d, w.norm_q, w.norm_k, d.S_txt);
    g[1] = gemm(n_txt, w.wqkv_txt, w.bqkv_txt, view(ws.qkv, d, 3 * D, 0, d.S_txt, 0), Mt, 3 * D, D, FK_EPI_QKV);
    qkv_epi(g[1], ws, d, w.norm_added_q, w.norm_added_k, 0);
    ctl(g[0], ws); FK_TRY(block_gemm(g, 2, mx(wx ? &wx->qkv_img : nullptr), st));
  }
  FK_TRY(fk_attention_fwd_ws_bf16(ws.q, ws.k, (const char*)ws.qkv + (int64_t)2 * D * 2, ws.o, nullptr, B, d.H, d.S, 3 * D,
                                  (int64_t)d.S * 3 * D, D, (int64_t)d.S * D, 0.08838834764831845f, ws.attn_ws, ws.attn_ws_bytes, ws.attn_grid, st));
  {
    fk_gemm_args g[2];
    g[0] = gemm(view(ws.o, d, D, d.S_txt, d.S_img, 0), w.w_out, w.b_out, h, Mi, D, D, FK_EPI_GATE_RES);
    gate_res(g[0], h, chunk(mi, 2), mod_bs, d.S_img);
    g[1] = gemm(view(ws.o, d, D, 0, d.S_txt, 0), w.w_add_out, w.b_add_out, cx, Mt, D, D, FK_EPI_GATE_RES);
    gate_res(g[1], cx, chunk(mt, 2), mod_bs, d.S_txt);
    set_ws(g[0], ws); set_ws(g[1], ws);
    ctl(g[0], ws); FK_TRY(block_gemm(g, 2, mx(wx ? &wx->out : nullptr), st));
  }
  FK_TRY(fk_ln_modulate2_bf16(s_all.p, s_all.r, (void*)n_all.p, n_all.r, chunk(mt, 3), chunk(mt, 4), chunk(mi, 3), chunk(mi, 4),
                              d.S_txt, mod_bs, d.S, M, D, ws.eps, st));
  {
    fk_gemm_args g[2];
    g[0] = gemm(n_img, w.w_ff1, w.b_ff1, view(ws.ff, d, 4 * D, d.S_txt, d.S_img, 0), Mi, 4 * D, D, FK_EPI_GELU_TANH);
    g[1] = gemm(n_txt, w.w_ff1_ctx, w.b_ff1_ctx, view(ws.ff, d, 4 * D, 0, d.S_txt, 0), Mt, 4 * D, D, FK_EPI_GELU_TANH);
    ctl(g[0], ws); FK_TRY(block_gemm(g, 2, mx(wx ? &wx->ff1 : nullptr), st));
  }
  {
    fk_gemm_args g[2];
    g[0] = gemm(view(ws.ff, d, 4 * D, d.S_txt, d.S_img, 0), w.w_ff2, w.b_ff2, h, Mi, D, 4 * D, FK_EPI_GATE_RES);
    gate_res(g[0], h, chunk(mi, 5), mod_bs, d.S_img);
    g[1] = gemm(view(ws.ff, d, 4 * D, 0, d.S_txt, 0), w.w_ff2_ctx, w.b_ff2_ctx, cx, Mt, D, 4 * D, FK_EPI_GATE_RES);
    gate_res(g[1], cx, chunk(mt, 5), mod_bs, d.S_txt);
    set_ws(g[0], ws); set_ws(g[1], ws);
    ctl(g[0], ws); FK_TRY(block_gemm(g, 2, mx(wx ? &wx->ff2 : nullptr), st));
  }
  return FK_OK;
}

int single_block(const fk_block_ws& ws, const Dims& d, const fk_single_block_weights& w, const void* mod, int64_t mod_bs,
                 fk_stream_t st, const fk_mx_ws* mxws = nullptr, const fk_single_block_weights_mx* wx = nullptr) {
  if (mxws && wx && mxws->fused) return single_block_fused(ws, d, w, mod, mod_bs, st, *mxws, *wx);
  Mx mxc;
  auto mx = [&](const fk_mx_pair* pair) -> const Mx* { if (!pair) return nullptr; mxc = Mx{mxws, pair}; return &mxc; };
  FK_CHECK_ARG(ws.cat != nullptr, "fk_single_block_fwd: needs the [attn | mlp] buffer");
  const int D = d.D, B = d.B;
  const int Ms = B * d.S;
  const char* m0 = (const char*)mod + w.mod_off * 2;     // shift, scale, gate
  auto chunk = [&](int j) { return (const void*)(m0 + (int64_t)j * D * 2); };
  const View s_all = view(ws.s, d, D, 0, d.S, 0), n_all = view(ws.n, d, D, 0, d.S, 0);
  FK_TRY(fk_ln_modulate_bf16(s_all.p, s_all.r, (void*)n_all.p, n_all.r, chunk(0), chunk(1), mod_bs, d.S, (int64_t)Ms, D, ws.eps, st));
  {
    fk_gemm_args g = gemm(n_all, w.wqkv, w.bqkv, view(ws.qkv, d, 3 * D, 0, d.S, 0), Ms, 3 * D, D, FK_EPI_QKV);
    qkv_epi(g, ws, d, w.norm_q, w.norm_k, 0);
    ctl(g, ws); FK_TRY(block_gemm(&g, 1, mx(wx ? &wx->qkv : nullptr), st));
  }
  // attention writes columns [0, D) of the [B, S, 5D] buffer, the MLP-up GEMM columns [D, 5D): proj_out reads one operand
  FK_TRY(fk_attention_fwd_ws_bf16(ws.q, ws.k, (const char*)ws.qkv + (int64_t)2 * D * 2, ws.cat, nullptr, B, d.H, d.S, 3 * D,
                                  (int64_t)d.S * 3 * D, 5 * D, (int64_t)d.S * 5 * D, 0.08838834764831845f, ws.attn_ws,
                                  ws.attn_ws_bytes, ws.attn_grid, st));
  {
    fk_gemm_args g = gemm(n_all, w.w_mlp, w.b_mlp, view(ws.cat, d, 5 * D, 0, d.S, D), Ms, 4 * D, D, FK_EPI_GELU_TANH);
    ctl(g, ws); FK_TRY(block_gemm(&g, 1, mx(wx ? &wx->mlp : nullptr), st));
  }
  {
    fk_gemm_args g = gemm(view(ws.cat, d, 5 * D, 0, d.S, 0), w.w_out, w.b_out, s_all, Ms, D, 5 * D, FK_EPI_GATE_RES);
    gate_res(g, s_all, chunk(2), mod_bs, d.S);
    set_ws(g, ws);
    ctl(g, ws); FK_TRY(block_gemm(&g, 1, mx(wx ? &wx->out : nullptr), st));
  }
  return FK_OK;
}

}  // namespace

extern "C" int fk_double_block_fwd(const fk_block_ws* ws, const fk_double_block_weights* w, const void* mod,
                                   int64_t mod_batch_stride, fk_stream_t stream) {
  Dims d;
  FK_TRY(check_ws(ws, d, "fk_double_block_fwd"));
  FK_CHECK_ARG(w && mod, "fk_double_block_fwd: null weights / modulation");
  return double_block(*ws, d, *w, mod, mod_batch_stride, stream);
}

extern "C" int fk_single_block_fwd(const fk_block_ws* ws, const fk_single_block_weights* w, const void* mod,
                                   int64_t mod_batch_stride, fk_stream_t stream) {
  Dims d;
  FK_TRY(check_ws(ws, d, "fk_single_block_fwd"));
  FK_CHECK_ARG(w && mod, "fk_single_block_fwd: null weights / modulation");
  return single_block(*ws, d, *w, mod, mod_batch_stride, stream);
}

extern "C" int fk_mmdit_blocks_fwd(const fk_block_ws* ws, const fk_double_block_weights* dbl, int32_t n_double,
                                   const fk_single_block_weights* sgl, int32_t n_single, const void* mod,
                                   int64_t mod_batch_stride, fk_stream_t stream) {
  Dims d;
  FK_TRY(check_ws(ws, d, "fk_mmdit_blocks_fwd"));
  FK_CHECK_ARG(mod && n_double >= 0 && n_single >= 0 && (n_double == 0 || dbl) && (n_single == 0 || sgl),
               "fk_mmdit_blocks_fwd: null weights / modulation");
  for (int i = 0; i < n_double; ++i) FK_TRY(double_block(*ws, d, dbl[i], mod, mod_batch_stride, stream));
  for (int i = 0; i < n_single; ++i) FK_TRY(single_block(*ws, d, sgl[i], mod, mod_batch_stride, stream));
  return FK_OK;
}

// ---- MXFP8 forms: the same launches with every block GEMM as quantize -> fk_gemm_mxfp8, or (fk_mx_ws.fused) the fused schedule
namespace {
int check_mx(const fk_mx_ws* mx, const char* who) {
  FK_CHECK_ARG(mx && mx->q && mx->s && (uintptr_t)mx->q % 16 == 0 && (uintptr_t)mx->s % 4 == 0,
               "%s: null or misaligned quantized-activation workspace", who);
  FK_CHECK_ARG((mx->fused & 3) != 2,
               "%s: fk_mx_ws.fused = %d: bit 1 (the attention emits MXFP8) is valid only together with bit 0 (the fused schedule)", who,
               (int)mx->fused);
  return FK_OK;
}
}  // namespace

extern "C" int fk_double_block_fwd_mx(const fk_block_ws* ws, const fk_mx_ws* mx, const fk_double_block_weights* w,
                                      const fk_double_block_weights_mx* wx, const void* mod, int64_t mod_batch_stride,
                                      fk_stream_t stream) {
  Dims d;
  FK_TRY(check_ws(ws, d, "fk_double_block_fwd_mx"));
  FK_TRY(check_mx(mx, "fk_double_block_fwd_mx"));
  FK_CHECK_ARG(w && wx && mod, "fk_double_block_fwd_mx: null weights / modulation");
  return double_block(*ws, d, *w, mod, mod_batch_stride, stream, mx, wx);
}

extern "C" int fk_single_block_fwd_mx(const fk_block_ws* ws, const fk_mx_ws* mx, const fk_single_block_weights* w,
                                      const fk_single_block_weights_mx* wx, const void* mod, int64_t mod_batch_stride,
                                      fk_stream_t stream) {
  Dims d;
  FK_TRY(check_ws(ws, d, "fk_single_block_fwd_mx"));
  FK_TRY(check_mx(mx, "fk_single_block_fwd_mx"));
  FK_CHECK_ARG(w && wx && mod, "fk_single_block_fwd_mx: null weights / modulation");
  return single_block(*ws, d, *w, mod, mod_batch_stride, stream, mx, wx);
}

extern "C" int fk_mmdit_blocks_fwd_mx(const fk_block_ws* ws, const fk_mx_ws* mx, const fk_double_block_weights* dbl,
                                      const fk_double_block_weights_mx* dblx, int32_t n_double, const fk_single_block_weights* sgl,
                                      const fk_single_block_weights_mx* sglx, int32_t n_single, const void* mod,
                                      int64_t mod_batch_stride, fk_stream_t stream) {
  Dims d;
  FK_TRY(check_ws(ws, d, "fk_mmdit_blocks_fwd_mx"));
  FK_TRY(check_mx(mx, "fk_mmdit_blocks_fwd_mx"));
  FK_CHECK_ARG(mod && n_double >= 0 && n_single >= 0 && (n_double == 0 || (dbl && dblx)) && (n_single == 0 || (sgl && sglx)),
               "fk_mmdit_blocks_fwd_mx: null weights / modulation");
  if (mx->fused) {   // before the first launch: nothing runs against a workspace that a later block would overrun
    if (n_double > 0) FK_TRY(check_fused_ws(*mx, d, 4 * d.D, "fk_mmdit_blocks_fwd_mx"));
    if (n_single > 0) FK_TRY(check_fused_ws(*mx, d, 5 * d.D, "fk_mmdit_blocks_fwd_mx"));
  }
  for (int i = 0; i < n_double; ++i) FK_TRY(double_block(*ws, d, dbl[i], mod, mod_batch_stride, stream, mx, &dblx[i]));
  for (int i = 0; i < n_single; ++i) FK_TRY(single_block(*ws, d, sgl[i], mod, mod_batch_stride, stream, mx, &sglx[i]));
  return FK_OK;
}
