// encoder.cpp -- composite: one conformer block enqueued from C++, no host sync.  select_route() checks every argument and picks ONE route (cfm.h cfm_route)
// before anything is launched; each route (run_*) is a straight list of launches built from the shared stages above it: GENERAL (17 launches: separate GEMMs,
// LayerNorm and depthwise kernels), FUSED_FFN (each feed-forward one launch of ffn.hip), CHAIN (4: the row-local chains of rowchain.hip around the attention),
// CHAIN_NEXT (3: the final chain also runs the NEXT block's macaron chain), CHAIN_NEXT_CIN (2: the conv-in chain is that launch's input stage), FFSPLIT (few
// rows at D = 256: feed-forwards split over FF, ffnsplit.hip), PAIR (D = 512: feed-forwards split over workgroup pairs).
//
// Mirrors reference src/encoder_layer.py:49-71:
//   x = x + 1/2 FFNm(LN(x)); x = x + MHSA(LN(x)); x = x + Conv(LN(x)); x = x + 1/2 FFN(LN(x)); out = LN(x)
// with every residual add, bias, activation, GLU and padding mask folded into a GEMM epilogue and the
// residual stream kept in f32.  Layer norms write the GEMM operand dtype directly.
#include <math.h>

#include <stdlib.h>

#include "cfm_common.h"

namespace {

const float kEps = 1e-5f;

inline const void* eoff(const void* p, int64_t elems, int dt) { return (const char*)p + elems * cfm_elt_size(dt); }

struct Ctx {   // the call's arguments, then what select_route derives from them while it checks
    const cfm_layer_weights* w; const cfm_layer_scratch* s; const cfm_layer_io* io; const float* x_in; float* x_out; cfm_stream_t st;
    int M, D, FF, H, dk, adt, w_dt, Tc, Tk, P;
    bool split, has_pos, ring;
    const int32_t* len;   // rows per item behind which the GLU output is zero: io->utt_len (whole utterances) or io->stream_len (streaming windows), else null
};

int& cin_merge_flag() {
    static int flag = getenv("CFM_CIN_MERGE") == nullptr || atoi(getenv("CFM_CIN_MERGE")) != 0;
    return flag;
}

int ffsplit_max_rows() {   // the environment override is for experiments (scripts/bench_small_batch.py)
    static const int rows = getenv("CFM_FFSPLIT_MAX_ROWS") ? atoi(getenv("CFM_FFSPLIT_MAX_ROWS")) : CFM_FFSPLIT_MAX_ROWS;
    return rows;
}

// the depthwise conv can run as the input stage of the pointwise-conv-2 head (15 symmetric taps); otherwise it is a launch of its own
bool taps15(const Ctx& c) { return c.io->ktaps == 15 && !c.io->causal_conv; }

#define CFM_TRY(expr) do { int rc__ = (expr); if (rc__ != CFM_OK) return rc__; } while (0)

// Every argument check of the block and the choice of its route; launches nothing and reads only the three structs and io->next_w.
int select_route(Ctx& c) {
    const cfm_layer_weights* w = c.w; const cfm_layer_scratch* s = c.s; const cfm_layer_io* io = c.io;
    CFM_CHECK_ARG(w && s && io && c.x_in && c.x_out, "cfm_encoder_layer_forward: null pointer");
    CFM_CHECK_ARG(io->B > 0 && io->T > 0 && io->D > 0 && io->H > 0 && io->D % io->H == 0 && io->FF > 0,
                  "cfm_encoder_layer_forward: bad dims B=%d T=%d D=%d H=%d FF=%d", io->B, io->T, io->D, io->H, io->FF);
    CFM_CHECK_ARG(io->D % 16 == 0, "cfm_encoder_layer_forward: D must be a multiple of 16 (GLU interleave)");
    CFM_CHECK_ARG(c.x_in != c.x_out, "cfm_encoder_layer_forward: x_in and x_out must differ (inputs are not mutated)");
    c.M = io->B * io->T; c.D = io->D; c.FF = io->FF; c.H = io->H; c.dk = c.D / c.H; c.adt = io->act_dtype; c.w_dt = io->w_dtype;
    c.split = io->act_dtype == CFM_F32;
    c.has_pos = io->pos_rows > 0 && w->pos_w;
    c.ring = io->kv_ring != nullptr;
    CFM_CHECK_ARG(!c.ring || (io->stream_offset && io->ring_T >= io->T && !io->attn_cache && !io->new_cache),
                  "encoder layer: the K/V ring needs stream_offset and ring_T >= T, and excludes attn_cache / new_cache");
    c.Tc = io->attn_cache ? io->cache_T : 0;
    c.Tk = c.ring ? io->ring_T : c.Tc + io->T;
    c.P = 0;
    if (c.has_pos) {
        CFM_CHECK_ARG((io->pos_embed || io->pos_proj) && (io->pos_shared || io->pos_rows % io->B == 0),
                      "encoder layer: pos_embed rows (%d) must be a multiple of B (%d)", io->pos_rows, io->B);
        c.P = io->pos_shared ? io->pos_rows : io->pos_rows / io->B;
        CFM_CHECK_ARG(!io->pos_shared || c.P == c.Tk, "encoder layer: shared positions need one row per key (%d rows, Tk=%d)", io->pos_rows, c.Tk);
        CFM_CHECK_ARG(c.P == 1 || c.P == c.Tk, "encoder layer: pos_embed gives %d rows per item, need 1 or Tk=%d (attention.py:78-88)", c.P, c.Tk);
    }
    CFM_CHECK_ARG(c.Tc == 0 || io->new_cache, "encoder layer: a KV cache input needs new_cache storage");
    CFM_CHECK_ARG(!io->after_out || (io->after_g && io->after_b), "encoder layer: after_out needs after_g / after_b");
    CFM_CHECK_ARG(!io->utt_len || (!c.ring && !io->attn_cache && !io->causal_conv && !io->pad_valid),
                  "encoder layer: utt_len (a ragged batch of whole utterances) excludes kv_ring, attn_cache, causal_conv and pad_valid");
    CFM_CHECK_ARG(!io->stream_len || (c.ring && !io->utt_len && !io->pad_valid),
                  "encoder layer: stream_len (per-stream window lengths) needs kv_ring and excludes utt_len, attn_cache and pad_valid");
    c.len = io->utt_len ? io->utt_len : io->stream_len;
    const bool chains = !c.split && w->ffm_w1f && w->ffm_w2n && w->ff_w1f && w->ff_w2n && w->qkv_wf && w->out_wf && w->pw1_wf && w->pw2_wf &&
                        cfm_rowchain_supported(c.D, c.FF);
    CFM_CHECK_ARG(!io->macaron_done || chains, "encoder layer: macaron_done needs the chain path");
    if (!chains) {
        CFM_CHECK_ARG(!c.split || (w->ffm_w1_lo && w->ffm_w2_lo && w->ff_w1_lo && w->ff_w2_lo && w->qkv_w_lo && w->out_w_lo && w->pw1_w_lo && w->pw2_w_lo &&
                                   (!c.has_pos || io->pos_proj || w->pos_w_lo)),
                      "encoder layer: split mode needs the *_lo weight planes");
        const bool fused = !c.split && w->ffm_w1f && w->ffm_w2f && w->ff_w1f && w->ff_w2f && (c.D == 144 || c.D == 256) && c.FF % 32 == 0 && c.FF <= 2048;
        return fused ? CFM_ROUTE_FUSED_FFN : CFM_ROUTE_GENERAL;
    }
    // PAIR needs D = 512 (cfm_rowchain_pair_supported) and FFSPLIT D = 256 (cfm_ffn_split_supported): they exclude each other by width
    const bool alone = s->psum && !io->macaron_done && !io->next_w;
    if (alone && s->psum_splits >= 3 && c.M <= CFM_PAIR_MAX_ROWS && cfm_rowchain_pair_supported(c.D, c.FF)) return CFM_ROUTE_PAIR;
    if (alone && c.M <= ffsplit_max_rows() && cfm_ffn_split_supported(c.D, c.FF) && s->psum_splits >= c.FF / 256 && w->pw2_w && io->ktaps == 15)
        return CFM_ROUTE_FFSPLIT;
    if (!io->next_w) return CFM_ROUTE_CHAIN;
    const cfm_layer_weights* nw = io->next_w;
    CFM_CHECK_ARG(taps15(c) && cfm_rowchain_dw_supported(c.D) && !io->after_out && io->next_x_out && io->next_x_out != c.x_out && nw->ffm_w1f && nw->ffm_w2n &&
                      nw->qkv_wf && c.D == 256 && c.FF == 2048,
                  "encoder layer: chaining into the next block needs the fused depthwise stage, no after_out, a distinct next_x_out and the next "
                  "block's fragment-major packs (D = 256, FF = 2048)");
    return cin_merge_flag() ? CFM_ROUTE_CHAIN_NEXT_CIN : CFM_ROUTE_CHAIN_NEXT;   // the merged conv-in stage needs nothing beyond the check above
}

// ---- shared stages -------------------------------------------------------------------------------------------------------------------------------
int gemm(const Ctx& c, const void* A, int a_dt, int64_t lda, const void* W, const void* Wlo, const float* bias, void* C, int c_dt,
         int64_t ldc, int M, int N, int K, int act, const float* res, float alpha, const uint8_t* row_mask) {
    cfm_gemm_desc d = {};
    d.A = A; d.W = W; d.W_lo = c.split ? Wlo : nullptr; d.bias = bias; d.residual = res; d.row_mask = row_mask; d.C = C;
    d.lda = lda; d.ldc = ldc; d.ldr = ldc; d.M = M; d.N = N; d.K = K;
    d.a_dtype = a_dt; d.w_dtype = c.w_dt; d.c_dtype = c_dt; d.act = act; d.alpha = alpha;
    if (act == CFM_ACT_GLU && c.len) { d.row_len = c.len; d.row_T = c.io->T; }   // zeros past each item's end (cfm.h cfm_layer_io.utt_len / stream_len)
    return cfm_gemm(&d, c.st);
}

int layernorm(const Ctx& c, const float* g, const float* b, void* out16, const uint8_t* row_mask) {   // s->xn-style operand of the next GEMM from x_out
    return cfm_layernorm(c.x_out, g, b, nullptr, 0, nullptr, nullptr, out16, c.adt, row_mask, kEps, c.M, c.D, c.st);
}

// after_out where no chain writes it: one more LayerNorm launch at the end (same result, nothing fused)
int after_norm(const Ctx& c) {
    if (!c.io->after_out) return CFM_OK;
    return cfm_layernorm(c.x_out, c.io->after_g, c.io->after_b, c.io->after_out, CFM_F32, nullptr, nullptr, nullptr, 0, nullptr, kEps, c.M, c.D, c.st);
}

// s->qkv -> s->ctx: positional projection unless the driver did it, K/V into the returned cache or the ring (ring_written: the q|k|v launch filled it), attention
int attention(const Ctx& c, bool ring_written = false) {
    const cfm_layer_weights* w = c.w; const cfm_layer_scratch* s = c.s; const cfm_layer_io* io = c.io;
    const int D = c.D, H = c.H, dk = c.dk, adt = c.adt, Tk = c.Tk;
    if (c.has_pos && !io->pos_proj)
        CFM_TRY(gemm(c, io->pos_embed, CFM_F32, D, w->pos_w, w->pos_w_lo, nullptr, s->pos, adt, D, io->pos_rows, D, D, CFM_ACT_NONE, nullptr, 0.f, nullptr));
    const void* kq = eoff(s->qkv, D, adt);
    const void* vq = eoff(s->qkv, 2 * D, adt);
    const int64_t sb = (int64_t)io->T * 3 * D, stt = 3 * D;
    if (io->new_cache)
        CFM_TRY(cfm_kv_cache_pack(io->attn_cache, c.Tc, kq, vq, adt, sb, stt, sb, stt, io->new_cache, io->B, H, io->T, dk, c.st));
    if (c.ring && !ring_written)
        CFM_TRY(cfm_kv_ring_write(kq, vq, adt, sb, stt, sb, stt, io->kv_ring, io->stream_offset, io->stream_len, io->B, H, io->T, dk, io->ring_T, c.st));
    cfm_attn_desc a = {};
    a.q = s->qkv; a.q_sb = sb; a.q_st = stt; a.q_dtype = adt;
    if (c.ring || c.Tc > 0) {   // keys/values in f32: every slot of the ring (the slot mask picks this step's context), or [cache | new] as packed into new_cache
        const float* kv = c.ring ? io->kv_ring : io->new_cache;
        a.k = kv; a.v = kv + dk; a.kv_dtype = CFM_F32;
        a.k_sb = a.v_sb = (int64_t)H * Tk * 2 * dk; a.k_sh = a.v_sh = (int64_t)Tk * 2 * dk; a.k_st = a.v_st = 2 * dk;
    } else {
        a.k = kq; a.v = vq; a.kv_dtype = adt;
        a.k_sb = a.v_sb = sb; a.k_sh = a.v_sh = dk; a.k_st = a.v_st = stt;
    }
    if (c.has_pos) {
        const int64_t pld = io->pos_proj ? io->pos_proj_ld : D;
        a.p = io->pos_proj ? io->pos_proj : s->pos; a.p_dtype = adt; a.p_sb = io->pos_shared ? 0 : (int64_t)c.P * pld; a.p_st = c.P == 1 ? 0 : pld;
        a.bias_u = w->bias_u; a.bias_v = w->bias_v;
    }
    a.mask = io->attn_mask; a.m_sb = io->am_sb; a.m_sq = io->am_sq;
    a.out = s->ctx; a.out_dtype = adt;
    a.B = io->B; a.H = H; a.Tq = io->T; a.Tk = Tk; a.dk = dk;
    a.mma_dtype = c.w_dt; a.split = c.split ? 1 : 0;
    a.scale = 1.0f / sqrtf((float)dk);
    return cfm_attention(&a, c.st);
}

// s->glu -> s->dw: depthwise conv + BatchNorm + SiLU as a launch of its own -- causal with its cache update, or the reference's symmetric one
int depthwise(const Ctx& c) {
    const cfm_layer_weights* w = c.w; const cfm_layer_scratch* s = c.s; const cfm_layer_io* io = c.io;
    if (!io->causal_conv)
        return cfm_dwconv_bn_silu(s->glu, c.adt, w->dw_w, w->dw_b, w->bn_scale, w->bn_shift, s->dw, c.adt, io->B, io->T, c.D, io->ktaps, c.st);
    CFM_TRY(cfm_dwconv_causal_bn_silu(s->glu, c.adt, io->conv_cache, w->dw_w, w->dw_b, w->bn_scale, w->bn_shift, s->dw, c.adt, io->B, io->T, c.D, io->ktaps, c.st));
    if (!io->conv_cache) return CFM_OK;
    return cfm_conv_cache_update(s->glu, c.adt, io->conv_cache, io->stream_len, io->B, io->T, c.D, io->ktaps, c.st);
}

// ---- row-chain descriptors (cfm.h cfm_rowchain_desc) -------------------------------------------------------------------------------------------------
cfm_rowchain_desc chain(const Ctx& c, float alpha) {   // the sizes of every chain; alpha scales its feed-forward (1/2) or its head (1)
    cfm_rowchain_desc d = {};
    d.M = c.M; d.D = c.D; d.FF = c.FF; d.w_dtype = c.w_dt; d.alpha = alpha; d.eps = kEps;
    return d;
}

// LN + feed-forward of a chain on rows x (nullptr: behind a head): the macaron one (LN_ffm) or the block's second (LN_ff)
cfm_rowchain_desc ffn_chain(const Ctx& c, bool macaron, const float* x) {
    const cfm_layer_weights* w = c.w;
    cfm_rowchain_desc d = chain(c, 0.5f);
    d.x = x;
    if (macaron) { d.ln_g = w->ln_ffm_g; d.ln_b = w->ln_ffm_b; d.w1f = w->ffm_w1f; d.w2n = w->ffm_w2n; d.b1 = w->ffm_b1; d.b2 = w->ffm_b2; }
    else { d.ln_g = w->ln_ff_g; d.ln_b = w->ln_ff_b; d.w1f = w->ff_w1f; d.w2n = w->ff_w2n; d.b1 = w->ff_b1; d.b2 = w->ff_b2; }
    return d;
}

void qkv_tail(cfm_rowchain_desc& d, const Ctx& c, const cfm_layer_weights* w) {   // fused q|k|v projection of block w -> s->qkv
    d.tail_w = w->qkv_wf; d.tail_b = w->qkv_b; d.tail_out = c.s->qkv; d.tail_N = 3 * c.D; d.tail_glu = 0;
}

// macaron chain: x_in + 1/2 FFNm -> x_out, LN_mha, q|k|v -- unless the previous block's call already ran it (macaron_done)
int macaron_chain(const Ctx& c) {
    if (c.io->macaron_done) return CFM_OK;
    cfm_rowchain_desc m = ffn_chain(c, true, c.x_in);
    m.ln2_g = c.w->ln_mha_g; m.ln2_b = c.w->ln_mha_b; m.out_f32 = c.x_out;
    qkv_tail(m, c, c.w);
    return cfm_rowchain(&m, c.st);
}

// conv-in chain: out-proj of s->ctx + residual x_out -> rows (in place, or `park` with the tail's columns over a workgroup pair, whose other workgroup still
// reads x_out) -> LN_conv (pad mask) -> pointwise-conv-1 + GLU -> s->glu
int conv_in_chain(const Ctx& c, float* park = nullptr) {
    const cfm_layer_weights* w = c.w;
    cfm_rowchain_desc ci = chain(c, 1.0f);
    ci.head_a = c.s->ctx; ci.head_w = w->out_wf; ci.head_b = w->out_b; ci.head_res = c.x_out; ci.ln_g = w->ln_conv_g; ci.ln_b = w->ln_conv_b;
    ci.ln_mask = c.io->pad_valid; ci.out_f32 = c.x_out; ci.tail_w = w->pw1_wf; ci.tail_b = w->pw1_b; ci.tail_out = c.s->glu; ci.tail_N = 2 * c.D; ci.tail_glu = 1;
    if (park) { ci.tail_pair = 1; ci.out_f32 = park; }
    ci.glu_len = c.len; ci.glu_T = c.io->T;
    return cfm_rowchain(&ci, c.st);
}

// head of a chain: pointwise-conv-2 + pad mask + residual `res`, on s->dw or -- dw_in_head -- on s->glu with the depthwise stage as the head's input stage
void pw2_head(cfm_rowchain_desc& d, const Ctx& c, bool dw_in_head, const float* res) {
    const cfm_layer_weights* w = c.w;
    d.head_a = dw_in_head ? c.s->glu : c.s->dw; d.head_w = w->pw2_wf; d.head_b = w->pw2_b; d.head_res = res; d.head_mask = c.io->pad_valid;
    if (dw_in_head) { d.dw_w = w->dw_w; d.dw_b = w->dw_b; d.dw_scale = w->bn_scale; d.dw_shift = w->bn_shift; d.dw_T = c.io->T; d.dw_K = 15; }
}

// s->glu -> x_out = res + pad mask(pointwise-conv-2(depthwise stage)): one chain launch with the depthwise stage in the head (tail_pair: each workgroup of a pair
// HALF of the output columns -- no LayerNorm behind the head, so half rows are complete results), or the depthwise kernel and a plain product over all CUs
int conv_out(const Ctx& c, bool dw_in_head, const float* res, int tail_pair) {
    if (dw_in_head) {
        cfm_rowchain_desc dh = chain(c, 1.0f);
        pw2_head(dh, c, true, res);
        dh.out_f32 = c.x_out; dh.tail_pair = tail_pair;
        return cfm_rowchain(&dh, c.st);
    }
    CFM_TRY(depthwise(c));
    return gemm(c, c.s->dw, c.adt, c.D, c.w->pw2_w, c.w->pw2_w_lo, c.w->pw2_b, c.x_out, CFM_F32, c.D, c.M, c.D, c.D, CFM_ACT_NONE, res, 1.0f, c.io->pad_valid);
}

// final chain: pointwise-conv-2 head on x_out -> LN_ff -> FFN -> + residual -> LN_final; the route says where the rows go
cfm_rowchain_desc final_chain(const Ctx& c, bool dw_in_head) {
    cfm_rowchain_desc fi = ffn_chain(c, false, nullptr);
    pw2_head(fi, c, dw_in_head, c.x_out);
    fi.ln1_g = c.w->ln_final_g; fi.ln1_b = c.w->ln_final_b;
    return fi;
}

// ... and the next block's macaron chain on the same rows, in the same launch (cfm.h cfm_layer_io.next_w): its residual -> next_x_out, its q|k|v -> s->qkv
void next_macaron(cfm_rowchain_desc& fi, const Ctx& c) {
    const cfm_layer_weights* nw = c.io->next_w;
    fi.s2_ln_g = nw->ln_ffm_g; fi.s2_ln_b = nw->ln_ffm_b; fi.s2_w1f = nw->ffm_w1f; fi.s2_w2n = nw->ffm_w2n; fi.s2_b1 = nw->ffm_b1; fi.s2_b2 = nw->ffm_b2;
    fi.s2_out_f32 = c.io->next_x_out; fi.s2_alpha = 0.5f;
    fi.ln2_g = nw->ln_mha_g; fi.ln2_b = nw->ln_mha_b;
    qkv_tail(fi, c, nw);
}

// ---- split feed-forward descriptors (cfm.h cfm_ffn_split_desc) ---------------------------------------------------------------------------------------
cfm_ffn_split_desc split_desc(const Ctx& c, int mode, const float* x) {
    cfm_ffn_split_desc f = {};
    f.x = x; f.M = c.M; f.D = c.D; f.mode = mode; f.w_dtype = c.w_dt; f.eps = kEps;
    return f;
}

int split_ffn(const Ctx& c, bool macaron, const float* x) {   // LN + feed-forward of rows x as FF / 256 partial slabs in s->psum
    const cfm_layer_weights* w = c.w;
    cfm_ffn_split_desc f = split_desc(c, 2, x);
    if (macaron) { f.ln_g = w->ln_ffm_g; f.ln_b = w->ln_ffm_b; f.w1 = w->ffm_w1f; f.b1 = w->ffm_b1; f.w2 = w->ffm_w2n; }
    else { f.ln_g = w->ln_ff_g; f.ln_b = w->ln_ff_b; f.w1 = w->ff_w1f; f.b1 = w->ff_b1; f.w2 = w->ff_w2n; }
    f.N1 = c.FF; f.act = CFM_ACT_SILU; f.psum_out = c.s->psum;
    return cfm_ffn_split(&f, c.st);
}

cfm_ffn_split_desc split_reduce(const Ctx& c, int mode, const float* x, const float* b2) {   // rows = x + 1/2 (slabs + b2) -> x_out, then what `mode` says
    cfm_ffn_split_desc r = split_desc(c, mode, x);
    r.psum = c.s->psum; r.psum_b2 = b2; r.psum_splits = c.FF / 256; r.psum_alpha = 0.5f; r.rows_out = c.x_out;
    return r;
}

// ---- the routes ------------------------------------------------------------------------------------------------------------------------------------
// steps (2) and (3) of the two routes without chains: s->xn = LN_mha(x_out) in; attention and convolution module, residuals in place on x_out
int attention_and_conv_gemms(const Ctx& c) {
    const cfm_layer_weights* w = c.w; const cfm_layer_scratch* s = c.s;
    const int M = c.M, D = c.D, adt = c.adt;
    CFM_TRY(gemm(c, s->xn, adt, D, w->qkv_w, w->qkv_w_lo, w->qkv_b, s->qkv, adt, 3 * D, M, 3 * D, D, CFM_ACT_NONE, nullptr, 0.f, nullptr));
    CFM_TRY(attention(c));
    CFM_TRY(gemm(c, s->ctx, adt, D, w->out_w, w->out_w_lo, w->out_b, c.x_out, CFM_F32, D, M, D, D, CFM_ACT_NONE, c.x_out, 1.0f, nullptr));
    CFM_TRY(layernorm(c, w->ln_conv_g, w->ln_conv_b, s->xn, c.io->pad_valid));   // mask -> pw1+GLU -> depthwise+BN+SiLU -> pw2 -> mask
    CFM_TRY(gemm(c, s->xn, adt, D, w->pw1_w, w->pw1_w_lo, w->pw1_b, s->glu, adt, D, M, 2 * D, D, CFM_ACT_GLU, nullptr, 0.f, nullptr));
    return conv_out(c, false, c.x_out, 0);
}

// xn_ready: s->xn already holds LN_ffm(x_in); next_g / next_b: also leave the next block's first norm there (cfm.h: read on this route only)
int run_general(const Ctx& c, int xn_ready, const float* next_g, const float* next_b) {
    const cfm_layer_weights* w = c.w; const cfm_layer_scratch* s = c.s;
    const int M = c.M, D = c.D, FF = c.FF, adt = c.adt;
    if (!xn_ready) CFM_TRY(cfm_layernorm(c.x_in, w->ln_ffm_g, w->ln_ffm_b, nullptr, 0, nullptr, nullptr, s->xn, adt, nullptr, kEps, M, D, c.st));
    CFM_TRY(gemm(c, s->xn, adt, D, w->ffm_w1, w->ffm_w1_lo, w->ffm_b1, s->hid, adt, FF, M, FF, D, CFM_ACT_SILU, nullptr, 0.f, nullptr));
    CFM_TRY(gemm(c, s->hid, adt, FF, w->ffm_w2, w->ffm_w2_lo, w->ffm_b2, c.x_out, CFM_F32, D, M, D, FF, CFM_ACT_NONE, c.x_in, 0.5f, nullptr));
    CFM_TRY(layernorm(c, w->ln_mha_g, w->ln_mha_b, s->xn, nullptr));
    CFM_TRY(attention_and_conv_gemms(c));
    CFM_TRY(layernorm(c, w->ln_ff_g, w->ln_ff_b, s->xn, nullptr));
    CFM_TRY(gemm(c, s->xn, adt, D, w->ff_w1, w->ff_w1_lo, w->ff_b1, s->hid, adt, FF, M, FF, D, CFM_ACT_SILU, nullptr, 0.f, nullptr));
    CFM_TRY(gemm(c, s->hid, adt, FF, w->ff_w2, w->ff_w2_lo, w->ff_b2, c.x_out, CFM_F32, D, M, D, FF, CFM_ACT_NONE, c.x_out, 0.5f, nullptr));
    // norm_final in place (+ the next block's first norm chained in registers)
    if (next_g)
        CFM_TRY(cfm_layernorm(c.x_out, w->ln_final_g, w->ln_final_b, c.x_out, CFM_F32, next_g, next_b, s->xn, adt, nullptr, kEps, M, D, c.st));
    else
        CFM_TRY(cfm_layernorm(c.x_out, w->ln_final_g, w->ln_final_b, c.x_out, CFM_F32, nullptr, nullptr, nullptr, 0, nullptr, kEps, M, D, c.st));
    return after_norm(c);
}

// the fused feed-forward kernel (ffn.hip) covers LN + W1 + SiLU + W2 + residual (+ the following norms) in one launch; the second runs in place on x_out
int run_fused_ffn(const Ctx& c) {
    const cfm_layer_weights* w = c.w;
    cfm_ffn_desc d = {};
    d.M = c.M; d.D = c.D; d.FF = c.FF; d.w_dtype = c.w_dt; d.out16_dtype = c.adt; d.act = CFM_ACT_SILU; d.add_x = 1; d.alpha = 0.5f; d.eps = kEps;
    cfm_ffn_desc m = d, f = d;
    m.x = c.x_in; m.ln_g = w->ln_ffm_g; m.ln_b = w->ln_ffm_b; m.w1f = w->ffm_w1f; m.w2f = w->ffm_w2f; m.b1 = w->ffm_b1; m.b2 = w->ffm_b2;
    m.ln2_g = w->ln_mha_g; m.ln2_b = w->ln_mha_b; m.out_f32 = c.x_out; m.out16 = c.s->xn;
    CFM_TRY(cfm_ffn_fused(&m, c.st));
    CFM_TRY(attention_and_conv_gemms(c));
    f.x = c.x_out; f.ln_g = w->ln_ff_g; f.ln_b = w->ln_ff_b; f.w1f = w->ff_w1f; f.w2f = w->ff_w2f; f.b1 = w->ff_b1; f.b2 = w->ff_b2;
    f.ln1_g = w->ln_final_g; f.ln1_b = w->ln_final_b; f.out_f32 = c.x_out;
    CFM_TRY(cfm_ffn_fused(&f, c.st));
    return after_norm(c);
}

int run_chain(const Ctx& c) {
    const bool dw_in_head = taps15(c) && cfm_rowchain_dw_supported(c.D);
    CFM_TRY(macaron_chain(c));
    CFM_TRY(attention(c));
    CFM_TRY(conv_in_chain(c));
    if (!dw_in_head) CFM_TRY(depthwise(c));
    cfm_rowchain_desc fi = final_chain(c, dw_in_head);
    fi.out_f32 = c.x_out;
    if (c.io->after_out) { fi.ln2_g = c.io->after_g; fi.ln2_b = c.io->after_b; fi.out2_f32 = c.io->after_out; }   // encoder.py:74 in the same launch
    return cfm_rowchain(&fi, c.st);
}

int run_chain_next(const Ctx& c) {   // x_out keeps the residual stream before the feed-forward; the block's output exists only in registers
    CFM_TRY(macaron_chain(c));
    CFM_TRY(attention(c));
    CFM_TRY(conv_in_chain(c));
    cfm_rowchain_desc fi = final_chain(c, true);
    next_macaron(fi, c);
    return cfm_rowchain(&fi, c.st);
}

// the conv-in chain as the input stage of the last launch, on each tile's 32 + 14 halo rows (cfm.h cfm_rowchain_desc.cin_*).  Its residual rows go to next_x_out
// (this tile's own rows: read back as the head's residual, overwritten at the end with the next block's residual -- all by the same workgroup); halo rows are
// read from x_out, which this launch does not write
int run_chain_next_cin(const Ctx& c) {
    const cfm_layer_weights* w = c.w;
    CFM_TRY(macaron_chain(c));
    CFM_TRY(attention(c));
    cfm_rowchain_desc fi = final_chain(c, true);
    next_macaron(fi, c);
    fi.cin_a = c.s->ctx; fi.cin_w = w->out_wf; fi.cin_b = w->out_b; fi.cin_res = c.x_out; fi.cin_out = c.io->next_x_out; fi.cin_ln_g = w->ln_conv_g;
    fi.cin_ln_b = w->ln_conv_b; fi.cin_mask = c.io->pad_valid; fi.cin_tail_w = w->pw1_wf; fi.cin_tail_b = w->pw1_b; fi.head_res = c.io->next_x_out;
    fi.glu_len = c.len; fi.glu_T = c.io->T;
    return cfm_rowchain(&fi, c.st);
}

// few rows (a streaming step): both feed-forwards split over FF / 256 workgroups per 32-row tile instead of inside the row chains, where every tile's
// workgroup streams all 2 MB of a feed-forward's weights whatever the row count
int run_ffsplit(const Ctx& c) {
    const cfm_layer_weights* w = c.w; const cfm_layer_io* io = c.io;
    const bool ring_written = c.ring && c.dk % 4 == 0;   // the q|k|v launch also fills the K/V ring
    CFM_TRY(split_ffn(c, true, c.x_in));
    cfm_ffn_split_desc q = split_reduce(c, 1, c.x_in, w->ffm_b2);   // ... then LN_mha and the fused q|k|v projection
    q.ln_g = w->ln_mha_g; q.ln_b = w->ln_mha_b; q.w1 = w->qkv_wf; q.b1 = w->qkv_b; q.N1 = 3 * c.D; q.act = CFM_ACT_NONE; q.out16 = c.s->qkv; q.ldo = 3 * c.D;
    if (ring_written) { q.kv_ring = io->kv_ring; q.ring_offsets = io->stream_offset; q.ring_T = io->ring_T; q.ring_H = c.H; q.ring_Tq = io->T; q.ring_len = io->stream_len; }
    CFM_TRY(cfm_ffn_split(&q, c.st));
    CFM_TRY(attention(c, ring_written));
    CFM_TRY(conv_in_chain(c));
    CFM_TRY(conv_out(c, taps15(c) && cfm_rowchain_dw_supported(c.D), c.x_out, 0));   // in place on x_out
    CFM_TRY(split_ffn(c, false, c.x_out));
    cfm_ffn_split_desc r = split_reduce(c, 0, c.x_out, w->ff_b2);   // ... then norm_final (+ after_norm)
    r.ln1_g = w->ln_final_g; r.ln1_b = w->ln_final_b;
    if (io->after_out) { r.ln2_g = io->after_g; r.ln2_b = io->after_b; r.rows2_out = io->after_out; }
    return cfm_ffn_split(&r, c.st);
}

// D = 512 with at most one row tile per CU pair (config 4: 125 tiles): both feed-forwards split over workgroup pairs, one half of FF each; the halves meet in
// the next launch's row load.  Chains with tail_pair split their tail's columns over the pair instead
int run_pair(const Ctx& c) {
    const cfm_layer_weights* w = c.w; const cfm_layer_scratch* s = c.s;
    float* const park = s->psum + (int64_t)2 * c.M * c.D;   // third slab: the conv-in chain's rows, the residual of pointwise-conv-2
    cfm_rowchain_desc m = ffn_chain(c, true, c.x_in);
    m.psum_out = s->psum;
    CFM_TRY(cfm_rowchain(&m, c.st));
    cfm_rowchain_desc q = chain(c, 1.0f);   // rows = x + 1/2 (half 0 + half 1 + b2) -> x_out, LN_mha, fused q|k|v projection
    q.x = c.x_in; q.psum_in = s->psum; q.psum_b2 = w->ffm_b2; q.psum_alpha = 0.5f; q.out_f32 = c.x_out; q.ln_g = w->ln_mha_g; q.ln_b = w->ln_mha_b; q.tail_pair = 1;
    qkv_tail(q, c, w);
    CFM_TRY(cfm_rowchain(&q, c.st));
    CFM_TRY(attention(c));
    CFM_TRY(conv_in_chain(c, park));
    // causal or not 15 taps: as a chain the 0.5 MB head would be streamed by BOTH workgroups of every pair (+18 us per launch), so it is a plain product
    CFM_TRY(conv_out(c, taps15(c), park, 1));
    cfm_rowchain_desc fa = ffn_chain(c, false, c.x_out);   // LN_ff -> this workgroup's half of the feed-forward
    fa.psum_out = s->psum;
    CFM_TRY(cfm_rowchain(&fa, c.st));
    cfm_rowchain_desc fr = chain(c, 1.0f);   // rows + 1/2 (halves + b2) -> LN_final, in place on x_out (one workgroup per row tile)
    fr.x = c.x_out; fr.psum_in = s->psum; fr.psum_b2 = w->ff_b2; fr.psum_alpha = 0.5f; fr.ln_g = w->ln_final_g; fr.ln_b = w->ln_final_b; fr.out2_f32 = c.x_out;
    CFM_TRY(cfm_rowchain(&fr, c.st));
    return after_norm(c);
}

}  // namespace

extern "C" int32_t cfm_set_cin_merge(int32_t on) {
    const int prev = cin_merge_flag();
    cin_merge_flag() = on != 0;
    return prev;
}

extern "C" int32_t cfm_ffsplit_max_rows(void) { return ffsplit_max_rows(); }

extern "C" int32_t cfm_encoder_layer_route(const cfm_layer_weights* w, const cfm_layer_scratch* s, const cfm_layer_io* io, const float* x_in, const float* x_out) {
    Ctx c = {w, s, io, x_in, const_cast<float*>(x_out), nullptr};
    return select_route(c);
}

extern "C" int cfm_encoder_layer_forward(const cfm_layer_weights* w, const cfm_layer_scratch* s, const cfm_layer_io* io,
                                         const float* x_in, float* x_out, int xn_ready, const float* next_g,
                                         const float* next_b, cfm_stream_t stream) {
    Ctx c = {w, s, io, x_in, x_out, stream};
    const int route = select_route(c);
    switch (route) {
        case CFM_ROUTE_GENERAL: return run_general(c, xn_ready, next_g, next_b);
        case CFM_ROUTE_FUSED_FFN: return run_fused_ffn(c);
        case CFM_ROUTE_CHAIN: return run_chain(c);
        case CFM_ROUTE_CHAIN_NEXT: return run_chain_next(c);
        case CFM_ROUTE_CHAIN_NEXT_CIN: return run_chain_next_cin(c);
        case CFM_ROUTE_FFSPLIT: return run_ffsplit(c);
        case CFM_ROUTE_PAIR: return run_pair(c);
        default: return route;   // a negative cfm_status, cfm_last_error() set
    }
}
