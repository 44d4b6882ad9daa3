// Block-level entry points of the BACKWARD pass (VERDICT r5 "missing" #3; the forward's are in blocks.hip): ONE call enqueues
// every launch of the backward of a FluxTransformerBlock / FluxSingleTransformerBlock -- what autograd runs for the reference at
// `accelerator.backward(loss)` (train_denoiser.py:1172) -- on the caller's stream.  Host code only: it fills the argument structs
// of the per-kernel entry points exactly as gpt_image_edit_amd/backward.py::_single_backward / _double_backward do (same views,
// same order, the stored-weight K-major GEMM forms of FK_BWD_K_MAJOR = 2) and calls them, so the launches and the results are the
// same bit for bit (tests/test_hip_train_step.py::test_block_level_backward_entry_points_give_the_same_bits).  The ZeRO-2 bucket
// hand-off of a block's gradients stays in Python between two calls.
//
// Scope = the stage-2 step as configured: activations stored by the forward, weight gradients by the layout-2 GEMM (token counts
// that are multiples of 64, uniformly strided views: any B for a single block, B == 1 for a double block, which refuses a
// larger batch with FK_EUNSUPPORTED before its first launch), data gradients on the stored weights (layout 1).  The Python adaptor keeps
// the per-launch route for everything else (recomputation, padded token counts, FK_BWD_K_MAJOR < 2).
#include "fk_common.h"

namespace {

constexpr int HD = 128;

struct Dims {
  int B, S_txt, S_img, S, H, D;
};
struct View {      // a [B, R, cols] slice of a joint [B, S, ld] buffer
  const void* p;
  fk_rows r;
  int R;
};
View view(const void* base, const Dims& d, int64_t ld, int64_t r0, int64_t R, int64_t c0) {
  return View{(const char*)base + (r0 * ld + c0) * 2, fk_rows{ld, R, (int64_t)d.S * ld}, (int)R};
}

#define FK_TRY(expr)              \
  do {                            \
    const int rc_ = (expr);       \
    if (rc_ != FK_OK) return rc_; \
  } while (0)

struct Ctx {
  const fk_bwd_ws& ws;
  Dims d;
  fk_stream_t st;
  void ctl(fk_gemm_args& g) const {
    g.variant = ws.gemm_variant; g.plan = ws.gemm_plan; g.group_m = ws.gemm_group_m; g.mfma = ws.gemm_mfma;
    g.variant_used = ws.gemm_variant_used;
  }
  // data gradient dX = dY W on the stored weight: ops.gemm(dy, out=dx, w=W[:, cols], layout=1[, epilogue=RES, res=dx])
  fk_gemm_args dgrad(const View& dy, const void* w, int64_t ldw, int n_out, int n_in, const View& dx, bool add) const {
    fk_gemm_args g = {};
    g.A = dy.p; g.a = dy.r;
    g.W = w; g.ldw = ldw;
    g.C = (void*)dx.p; g.c = dx.r;
    g.M = d.B * dy.R; g.N = n_in; g.K = n_out;
    g.layout = 1; g.alpha = 1.0f;
    g.epilogue = add ? FK_EPI_RES : FK_EPI_NONE;
    if (add) { g.res = dx.p; g.r = dx.r; }
    ctl(g);
    return g;
  }
  // the layout-2 GEMM addresses W by one row stride (ldw): a [B, R, *] operand must continue from batch to batch
  bool uniform(const View& v) const { return d.B == 1 || v.r.batch_stride == (int64_t)v.R * v.r.ld; }
  // weight gradient dW [N, K] = dY^T X over the tokens of two [B, R, *] views: ops.gemm(dy, x, out=dw, layout=2)
  int wgrad(const View& dy, int n, const View& x, int k, void* dw) const {
    if (!(uniform(x) && uniform(dy))) {   // unreachable from the entry points below (they refuse up front); kept for new callers
      fk_set_error("block backward: weight gradient over views that are not uniformly strided (B = %d)", d.B);
      return FK_EUNSUPPORTED;
    }
    fk_gemm_args g = {};
    const bool one = d.B == 1;       // backward.wgrad: a one-batch view is passed as its [R, N] matrix (any batch stride)
    g.A = dy.p; g.a = one ? fk_rows{dy.r.ld, 0, 0} : dy.r;
    g.W = x.p; g.ldw = x.r.ld;
    g.C = dw; g.c = fk_rows{k, 0, 0};
    g.M = n; g.N = k; g.K = d.B * dy.R;
    g.layout = 2; g.alpha = 1.0f; g.epilogue = FK_EPI_NONE;
    ctl(g);
    return fk_gemm_bf16(&g, st);
  }
  int colsum(const View& x, int n, float* out) const { return fk_colsum_bf16(x.p, x.r, (int64_t)d.B * x.R, n, out, ws.red_ws, st); }
  int gate_res_bwd(const View& dout, const View& y, const void* gate, const View& dy, float* dgate, int64_t dgate_ld) const {
    return fk_gate_res_bwd_bf16(dout.p, dout.r, y.p, y.r, gate, ws.mod_batch_stride, dout.R, (void*)dy.p, dy.r, dgate, dgate_ld,
                                ws.red_ws, d.B, d.D, st);
  }
  int ln_bwd(const View& x, const View& dn, const void* scale, const View& g, float* dshift, int64_t dmod_ld) const {
    return fk_ln_modulate_bwd_bf16(x.p, x.r, dn.p, dn.r, scale, ws.mod_batch_stride, x.R, g.p, g.r, (void*)g.p, g.r, dshift,
                                   dshift + d.D, dmod_ld, ws.red_ws, d.B, d.D, ws.eps, st);
  }
  // AdaLN linear: dW [n, D] = dmod^T silu(temb), db [n] = column 0 of dmod^T ones (backward.py::_mod_grads)
  int mod_grads(const float* dmod, int64_t dmod_ld, int n, void* dw, void* db64) const {
    FK_TRY(fk_f32_to_bf16_transposed(dmod, dmod_ld, ws.dmodT, 64, d.B, n, st));
    for (int which = 0; which < 2; ++which) {
      fk_gemm_args g = {};
      g.A = ws.dmodT; g.a = fk_rows{64, 0, 0};
      g.W = which == 0 ? ws.actT : ws.onesT; g.ldw = 64;
      g.C = which == 0 ? dw : db64; g.c = fk_rows{which == 0 ? d.D : 64, 0, 0};
      g.M = n; g.N = which == 0 ? d.D : 64; g.K = 64;
      g.alpha = 1.0f; g.epilogue = FK_EPI_NONE;
      ctl(g);
      FK_TRY(fk_gemm_bf16(&g, st));
    }
    return FK_OK;
  }
  int attention(const fk_block_saved& sv) const {
    const int D = d.D, S = d.S, B = d.B, H = d.H;
    FK_TRY(fk_rowdot_bf16(ws.d_o, D, (int64_t)S * D, sv.o, D, (int64_t)S * D, ws.dsum, B, S, H, st));
    const fk_attn_view q = {sv.q, HD, (int64_t)S * HD, (int64_t)H * S * HD}, k = {sv.k, HD, (int64_t)S * HD, (int64_t)H * S * HD};
    const fk_attn_view v = {(const char*)sv.qkv + (int64_t)2 * D * 2, 3 * D, HD, (int64_t)S * 3 * D};
    const fk_attn_view dout = {ws.d_o, D, HD, (int64_t)S * D};
    const fk_attn_view dq = {ws.dq, HD, (int64_t)S * HD, (int64_t)H * S * HD}, dk = {ws.dk, HD, (int64_t)S * HD, (int64_t)H * S * HD};
    const fk_attn_view dv = {(char*)ws.dqkv + (int64_t)2 * D * 2, 3 * D, HD, (int64_t)S * 3 * D};
    return fk_attention_bwd_ws_bf16(&q, &k, &v, &dout, sv.lse, ws.dsum, &dq, &dk, &dv, B, H, S, 0.08838834764831845f, ws.attn_ws,
                                    ws.attn_ws_bytes, ws.attn_grid, ws.attn_passes, st);
  }
};

int check(const fk_bwd_ws* ws, const fk_block_saved* sv, Dims& d, const char* who) {
  FK_CHECK_ARG(ws != nullptr && sv != nullptr, "%s: null workspace / saved activations", who);
  FK_CHECK_ARG(ws->B > 0 && ws->S_txt >= 0 && ws->S_img > 0 && ws->H > 0, "%s: bad B / S_txt / S_img / H %d %d %d %d", who, ws->B,
               ws->S_txt, ws->S_img, ws->H);
  d = Dims{ws->B, ws->S_txt, ws->S_img, ws->S_txt + ws->S_img, ws->H, ws->H * HD};
  FK_CHECK_ARG(ws->g && ws->dy && ws->dff && ws->dn && ws->d_o && ws->dqkv && ws->dq && ws->dk && ws->dsum && ws->dmod && ws->cos &&
               ws->sin && ws->red_ws && ws->mod && ws->attn_ws, "%s: null scratch buffer", who);
  FK_CHECK_ARG(sv->x0 && sv->n1 && sv->qkv && sv->q && sv->k && sv->y1 && sv->h1 && sv->o && sv->lse, "%s: null saved activation", who);
  FK_CHECK_ARG((int64_t)d.B * d.S < (1ll << 31), "%s: B * S too large", who);
  return FK_OK;
}

}  // namespace

extern "C" int fk_single_block_bwd(const fk_bwd_ws* wsp, const fk_block_saved* svp, const fk_single_block_weights* wp,
                                   const fk_single_block_grads* gp, fk_stream_t st) {
  Dims d;
  FK_TRY(check(wsp, svp, d, "fk_single_block_bwd"));
  FK_CHECK_ARG(wp && gp && gp->dnorm, "fk_single_block_bwd: null weights / gradient table");
  const fk_bwd_ws& ws = *wsp;
  const fk_block_saved& sv = *svp;
  const fk_single_block_weights& w = *wp;
  const fk_single_block_grads& gr = *gp;
  const Ctx c{ws, d, st};
  const int D = d.D, S = d.S;
  const char* mo = (const char*)ws.mod + w.mod_off * 2;      // shift, scale, gate: D each
  auto ch = [&](int j) { return (const void*)(mo + (int64_t)j * D * 2); };
  const View g = view(ws.g, d, D, 0, S, 0), dy = view(ws.dy, d, D, 0, S, 0), d_o = view(ws.d_o, d, D, 0, S, 0);
  const View dff = view(ws.dff, d, 4 * D, 0, S, 0), dn = view(ws.dn, d, D, 0, S, 0), dqkv = view(ws.dqkv, d, 3 * D, 0, S, 0);
  const View y1 = view(sv.y1, d, D, 0, S, 0), n1 = view(sv.n1, d, D, 0, S, 0), x0 = view(sv.x0, d, D, 0, S, 0);
  float* const dmod = ws.dmod;                                // fp32 [B, 3D]
  const int64_t dml = 3 * D;
  // x' = x + gate * y, y = proj_out([attn | gelu(mlp)])
  FK_TRY(c.gate_res_bwd(g, y1, ch(2), dy, dmod + 2 * D, dml));
  {  // proj_out [D, 5D]: input columns [0, D) -> attention, [D, 5D) -> MLP
    fk_gemm_args a = c.dgrad(dy, w.w_out, 5 * D, D, D, d_o, false);
    FK_TRY(fk_gemm_bf16(&a, st));
    fk_gemm_args b = c.dgrad(dy, (const char*)w.w_out + (int64_t)D * 2, 5 * D, D, 4 * D, dff, false);
    FK_TRY(fk_gemm_bf16(&b, st));
  }
  FK_TRY(fk_gelu_bwd_bf16(sv.h1, ws.dff, ws.dff, (int64_t)d.B * S * 4 * D, st));
  FK_TRY(c.attention(sv));
  FK_TRY(fk_qkv_post_bwd_bf16(ws.dq, ws.dk, sv.qkv, ws.dqkv, w.norm_q, w.norm_k, nullptr, nullptr, ws.cos, ws.sin, gr.dnorm,
                              ws.red_ws, d.B, S, 0, d.H, ws.eps, st));
  {
    fk_gemm_args a = c.dgrad(dqkv, w.wqkv, D, 3 * D, D, dn, false);
    FK_TRY(fk_gemm_bf16(&a, st));
    fk_gemm_args b = c.dgrad(dff, w.w_mlp, D, 4 * D, D, dn, true);
    FK_TRY(fk_gemm_bf16(&b, st));
  }
  if (gr.dwqkv) {
    FK_TRY(c.wgrad(dqkv, 3 * D, n1, D, gr.dwqkv));
    FK_TRY(c.colsum(dqkv, 3 * D, gr.dbqkv));
  }
  if (gr.dw_mlp) {
    FK_TRY(c.wgrad(dff, 4 * D, n1, D, gr.dw_mlp));
    FK_TRY(c.colsum(dff, 4 * D, gr.db_mlp));
  }
  if (gr.dw_out) {   // cat is shared scratch: rebuild [attn | gelu(mlp)] of this block
    FK_CHECK_ARG(ws.cat, "fk_single_block_bwd: proj_out trains but no cat scratch");
    const hipError_t e = hipMemcpy2DAsync(ws.cat, (size_t)5 * D * 2, sv.o, (size_t)D * 2, (size_t)D * 2, (size_t)d.B * S,
                                          hipMemcpyDeviceToDevice, (hipStream_t)st);
    FK_CHECK_ARG(e == hipSuccess, "fk_single_block_bwd: copy of the attention output into cat failed: %s", hipGetErrorString(e));
    const View cat_mlp = view(ws.cat, d, 5 * D, 0, S, D), h1 = view(sv.h1, d, 4 * D, 0, S, 0);
    FK_TRY(fk_gelu_tanh_bf16(h1.p, h1.r, (void*)cat_mlp.p, cat_mlp.r, (int64_t)d.B * S, 4 * D, st));
    FK_TRY(c.wgrad(dy, D, view(ws.cat, d, 5 * D, 0, S, 0), 5 * D, gr.dw_out));
    FK_TRY(c.colsum(dy, D, gr.db_out));
  }
  FK_TRY(c.ln_bwd(x0, dn, ch(1), g, dmod, dml));
  if (gr.dw_mod) FK_TRY(c.mod_grads(dmod, dml, 3 * D, gr.dw_mod, gr.db_mod));
  return FK_OK;
}

extern "C" int fk_double_block_bwd(const fk_bwd_ws* wsp, const fk_block_saved* svp, const fk_double_block_weights* wp,
                                   const fk_double_block_grads* gp, fk_stream_t st) {
  Dims d;
  FK_TRY(check(wsp, svp, d, "fk_double_block_bwd"));
  FK_CHECK_ARG(wp && gp && gp->dnorm && svp->x1 && svp->n2 && svp->y2 && d.S_txt > 0,
               "fk_double_block_bwd: null weights / gradient table / x1, n2, y2, or no text stream");
  if (d.B != 1) {   // before the first launch: the caller's buffers are untouched
    // every weight gradient here runs over the image or the text rows of a joint [B, S, *] buffer: batch stride S * ld, not
    // R * ld, which the layout-2 GEMM cannot address for its second operand (Ctx::uniform)
    fk_set_error("fk_double_block_bwd: B = %d unsupported, double blocks take B == 1 (the stream slices of a joint buffer are "
                 "not uniformly strided)", d.B);
    return FK_EUNSUPPORTED;
  }
  const fk_bwd_ws& ws = *wsp;
  const fk_block_saved& sv = *svp;
  const fk_double_block_weights& w = *wp;
  const fk_double_block_grads& gr = *gp;
  const Ctx c{ws, d, st};
  const int D = d.D, S = d.S, St = d.S_txt, Si = d.S_img;
  const char* mi = (const char*)ws.mod + w.mod_off_img * 2;   // shift, scale, gate, shift_mlp, scale_mlp, gate_mlp: D each
  const char* mt = (const char*)ws.mod + w.mod_off_txt * 2;
  auto ch = [&](const char* m, int j) { return (const void*)(m + (int64_t)j * D * 2); };
  auto img = [&](const void* base, int64_t ld) { return view(base, d, ld, St, Si, 0); };
  auto txt = [&](const void* base, int64_t ld) { return view(base, d, ld, 0, St, 0); };
  float* const dm_i = ws.dmod;                                // fp32 [B, 12D] = [image 6D | text 6D]
  float* const dm_t = ws.dmod + 6 * D;
  const int64_t dml = 12 * D;
  const bool ff2_i = gr.dw_ff2 != nullptr, ff2_t = gr.dw_ff2_ctx != nullptr;
  // -- MLP: x2 = x1 + gate_mlp * y2
  FK_TRY(c.gate_res_bwd(img(ws.g, D), img(sv.y2, D), ch(mi, 5), img(ws.dy, D), dm_i + 5 * D, dml));
  FK_TRY(c.gate_res_bwd(txt(ws.g, D), txt(sv.y2, D), ch(mt, 5), txt(ws.dy, D), dm_t + 5 * D, dml));
  if (ff2_i || ff2_t) {   // ws.ff is shared scratch: this block's GELU output again
    FK_CHECK_ARG(ws.ff, "fk_double_block_bwd: ff.net.2 trains but no ff scratch");
    const View h1 = view(sv.h1, d, 4 * D, 0, S, 0), ff = view(ws.ff, d, 4 * D, 0, S, 0);
    FK_TRY(fk_gelu_tanh_bf16(h1.p, h1.r, (void*)ff.p, ff.r, (int64_t)d.B * S, 4 * D, st));
    if (ff2_i) {
      FK_TRY(c.wgrad(img(ws.dy, D), D, img(ws.ff, 4 * D), 4 * D, gr.dw_ff2));
      FK_TRY(c.colsum(img(ws.dy, D), D, gr.db_ff2));
    }
    if (ff2_t) {
      FK_TRY(c.wgrad(txt(ws.dy, D), D, txt(ws.ff, 4 * D), 4 * D, gr.dw_ff2_ctx));
      FK_TRY(c.colsum(txt(ws.dy, D), D, gr.db_ff2_ctx));
    }
  }
  auto grouped = [&](const fk_gemm_args& a, const fk_gemm_args& b) {
    fk_gemm_args g2[2] = {a, b};
    return fk_gemm_bf16_grouped(g2, 2, st);
  };
  FK_TRY(grouped(c.dgrad(img(ws.dy, D), w.w_ff2, 4 * D, D, 4 * D, img(ws.dff, 4 * D), false),
                 c.dgrad(txt(ws.dy, D), w.w_ff2_ctx, 4 * D, D, 4 * D, txt(ws.dff, 4 * D), false)));
  FK_TRY(fk_gelu_bwd_bf16(sv.h1, ws.dff, ws.dff, (int64_t)d.B * S * 4 * D, st));
  if (gr.dw_ff1) {
    FK_TRY(c.wgrad(img(ws.dff, 4 * D), 4 * D, img(sv.n2, D), D, gr.dw_ff1));
    FK_TRY(c.colsum(img(ws.dff, 4 * D), 4 * D, gr.db_ff1));
  }
  if (gr.dw_ff1_ctx) {
    FK_TRY(c.wgrad(txt(ws.dff, 4 * D), 4 * D, txt(sv.n2, D), D, gr.dw_ff1_ctx));
    FK_TRY(c.colsum(txt(ws.dff, 4 * D), 4 * D, gr.db_ff1_ctx));
  }
  FK_TRY(grouped(c.dgrad(img(ws.dff, 4 * D), w.w_ff1, D, 4 * D, D, img(ws.dn, D), false),
                 c.dgrad(txt(ws.dff, 4 * D), w.w_ff1_ctx, D, 4 * D, D, txt(ws.dn, D), false)));
  FK_TRY(c.ln_bwd(img(sv.x1, D), img(ws.dn, D), ch(mi, 4), img(ws.g, D), dm_i + 3 * D, dml));
  FK_TRY(c.ln_bwd(txt(sv.x1, D), txt(ws.dn, D), ch(mt, 4), txt(ws.g, D), dm_t + 3 * D, dml));
  // -- attention output projection: x1 = x0 + gate_msa * y1
  FK_TRY(c.gate_res_bwd(img(ws.g, D), img(sv.y1, D), ch(mi, 2), img(ws.dy, D), dm_i + 2 * D, dml));
  FK_TRY(c.gate_res_bwd(txt(ws.g, D), txt(sv.y1, D), ch(mt, 2), txt(ws.dy, D), dm_t + 2 * D, dml));
  FK_TRY(grouped(c.dgrad(img(ws.dy, D), w.w_out, D, D, D, img(ws.d_o, D), false),
                 c.dgrad(txt(ws.dy, D), w.w_add_out, D, D, D, txt(ws.d_o, D), false)));
  if (gr.dw_out) {
    FK_TRY(c.wgrad(img(ws.dy, D), D, img(sv.o, D), D, gr.dw_out));
    FK_TRY(c.colsum(img(ws.dy, D), D, gr.db_out));
  }
  if (gr.dw_add_out) {
    FK_TRY(c.wgrad(txt(ws.dy, D), D, txt(sv.o, D), D, gr.dw_add_out));
    FK_TRY(c.colsum(txt(ws.dy, D), D, gr.db_add_out));
  }
  // -- joint attention
  FK_TRY(c.attention(sv));
  FK_TRY(fk_qkv_post_bwd_bf16(ws.dq, ws.dk, sv.qkv, ws.dqkv, w.norm_q, w.norm_k, w.norm_added_q, w.norm_added_k, ws.cos, ws.sin,
                              gr.dnorm, ws.red_ws, d.B, S, St, d.H, ws.eps, st));
  FK_TRY(grouped(c.dgrad(img(ws.dqkv, 3 * D), w.wqkv_img, D, 3 * D, D, img(ws.dn, D), false),
                 c.dgrad(txt(ws.dqkv, 3 * D), w.wqkv_txt, D, 3 * D, D, txt(ws.dn, D), false)));
  if (gr.dwqkv_img) {
    FK_TRY(c.wgrad(img(ws.dqkv, 3 * D), 3 * D, img(sv.n1, D), D, gr.dwqkv_img));
    FK_TRY(c.colsum(img(ws.dqkv, 3 * D), 3 * D, gr.dbqkv_img));
  }
  if (gr.dwqkv_txt) {
    FK_TRY(c.wgrad(txt(ws.dqkv, 3 * D), 3 * D, txt(sv.n1, D), D, gr.dwqkv_txt));
    FK_TRY(c.colsum(txt(ws.dqkv, 3 * D), 3 * D, gr.dbqkv_txt));
  }
  FK_TRY(c.ln_bwd(img(sv.x0, D), img(ws.dn, D), ch(mi, 1), img(ws.g, D), dm_i, dml));
  FK_TRY(c.ln_bwd(txt(sv.x0, D), txt(ws.dn, D), ch(mt, 1), txt(ws.g, D), dm_t, dml));
  if (gr.dw_mod_img) FK_TRY(c.mod_grads(dm_i, dml, 6 * D, gr.dw_mod_img, gr.db_mod_img));
  if (gr.dw_mod_txt) FK_TRY(c.mod_grads(dm_t, dml, 6 * D, gr.dw_mod_txt, gr.db_mod_txt));
  return FK_OK;
}
