/* cfm.h -- C ABI of libconformer_gfx950.so: the MI355X (gfx950 / CDNA4) conformer-encoder hot path.
 *
 * This is the drop-in boundary described in SURVEY.md section 8(b).  The reference
 * (Lingeng56/conformer-pytorch-lightning) has no native layer at all: its hot path is eager
 * torch.nn ops issued from Python.  Each entry point below therefore names the reference Python
 * call site it replaces (file:line under the reference's src/), and INTEGRATION.md shows the ctypes
 * binding a maintainer of the reference would add.
 *
 * Conventions
 *  - plain pointers and sizes only (no torch types).  Every pointer is a DEVICE pointer on the GPU
 *    that owns `stream`, unless a comment says "host".
 *  - every launch function returns CFM_OK (0) or a negative cfm_status; it never throws, aborts,
 *    allocates device memory or synchronises.  Text of the last error of the calling thread:
 *    cfm_last_error().
 *  - `stream` is a hipStream_t passed as void* (torch.cuda.current_stream().cuda_stream).
 *  - activations are row-major [rows, cols]; "16-bit" means bf16 or fp16 as selected by cfm_dtype.
 *  - all entry points are re-entrant; the only global state is the optional profiling table
 *    (cfm_prof_*), guarded by a mutex.
 */
#ifndef CFM_H_
#define CFM_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CFM_VERSION 307 /* 0.3.7: removed cfm_dwconv_bn_train (cfm_dwconv_bn_train_groups with one group), cfm_dwconv_bn_train_bwd and cfm_dwconv_bn_train_bwd_acc (cfm_dwconv_bn_train_bwd_groups with one group; its accumulate argument) and cfm_layernorm_bwd (cfm_layernorm_bwd_fused with the descriptor's optional fields zero). 0.3.7 (additive, same number): the attention decoder's beam search (cfm_dec_step_attn_desc, cfm_dec_step_attn, cfm_dec_beam_prune_desc, cfm_dec_beam_prune). 0.3.6 (additive): cfm_route, cfm_encoder_layer_route (the route cfm_encoder_layer_forward would take, asked on the host), cfm_ffsplit_max_rows. 0.3.5: removed the attention input stage of the conv-in chain (cfm_rowchain_desc.att_*, cfm_layer_scratch.vt and its row stride) and the transposed-value output of the macaron chain's tail that fed it (three cfm_rowchain_desc fields); psum_out chains take no head. 0.3.4: removed cfm_ctc_nll_train (cfm_ctc_nll_train_groups is the training forward), cfm_ctc_grad requires beta (alpha is no longer overwritten), removed cfm_rnnt_desc.sweep / cfm_rnnt_packed_desc.sweep (the LDS recursion is the only one). 0.3.3: removed cfm_encoder_layer_train_forward / _backward (the stack entry points run a single block), cfm_ffn_train_forward / _supported, cfm_ffn_train_desc, cfm_pack_ffn_fragments, cfm_layer_train_weights.*_w1f / *_w2f, cfm_layer_train_io.B / T / attn_mask / am_sb / am_sq / side_stream and cfm_encoder_train_backward's n_scratch. 0.3.2 (additive, same number): packed RNN-T lattices (cfm_lattice, cfm_rnnt_packed_desc, cfm_rnnt_packed_nll / _grad, cfm_joint_act_packed / _bwd). 0.3.2 (additive, same number): the RNN-T loss (cfm_rnnt_desc, cfm_rnnt_nll, cfm_rnnt_grad) and the transducer joint's activation backward (cfm_joint_act_bwd). 0.3.2: cfm_rowchain_desc.cin_* (the conv-in chain as the input stage of the next launch). 0.3.1: row chains at D = 512, cfm_rowchain_desc.psum_out / psum_in (feed-forward split over workgroup pairs), cfm_conv12_relu at C = 512. 0.3.0: row groups in the train entry points (cfm_train_group, cfm_layer_train_io.n_groups), cfm_gemm_tn_group + deferred weight gradients, cfm_encoder_train_forward / _backward (the whole stack from one host call). 0.2.3: cfm_ffn_split, cfm_layer_scratch.psum (the feed-forward split over FF for few rows). 0.2.2: cfm_ctc_nll_train / cfm_ctc_grad take a beta buffer (both recursions in one launch); GEMM tile ids 9-11 (K groups). 0.2.1: fused front-end (cfm_conv12_relu); attention stage of the conv-in chain (cfm_rowchain_desc.att_*, cfm_layer_scratch.vt). 0.2.0: training entry points */

typedef void* cfm_stream_t;

typedef enum { CFM_F32 = 0, CFM_BF16 = 1, CFM_F16 = 2 } cfm_dtype;

typedef enum {
    CFM_OK = 0,
    CFM_ERR_ARG = -1,         /* bad shape / alignment / null pointer / unsupported combination */
    CFM_ERR_LAUNCH = -2,      /* hipGetLastError() after a launch */
    CFM_ERR_UNSUPPORTED = -3  /* valid request this build has no kernel for */
} cfm_status;

typedef enum {
    CFM_ACT_NONE = 0, CFM_ACT_SILU = 1, CFM_ACT_RELU = 2, CFM_ACT_GLU = 3,
    /* backward epilogues (training): v = alpha * (acc + bias) * f'(aux[m,n]) with aux the forward pre-activation (SiLU) or output (ReLU) */
    CFM_ACT_DSILU = 4, CFM_ACT_DRELU = 5
} cfm_act;

int cfm_version(void);
const char* cfm_last_error(void);
/* 1 when the library was built for gfx950 and a gfx950 device is visible (host query, no launch). */
int cfm_device_ok(void);

/* ------------------------------------------------------------------------------------------------
 * GEMM with fused epilogue:   C = epilogue( A[M,K] . W[N,K]^T )
 *
 * replaces nn.Linear / nn.Conv1d(k=1) / nn.Conv2d(3,stride 2) call sites:
 *   feedforward.py:17-20 (w_1 + SiLU, w_2), attention.py:62-64,78,99 (linear_q/k/v/pos/out),
 *   convolution.py:41-42 (pointwise_conv1 + GLU), :46-48 (pointwise_conv2 + mask),
 *   convolution.py:62-63 (Conv2d(D,D,3,2)+ReLU as implicit GEMM), :74 (out Linear).
 *
 *  A        a_dtype 16-bit or f32 (f32 is rounded to `w_dtype` while staging; or split, below)
 *  W        [N,K] row-major (the nn.Linear weight layout), 16-bit `w_dtype` (bf16|fp16)
 *  W_lo     optional second plane: when non-NULL the product is evaluated as
 *           A_hi.W_hi + A_lo.W_hi + A_hi.W_lo with A split on the fly (A must be f32, w_dtype bf16):
 *           ~16 mantissa bits, the "f32-accurate" mode.
 *  epilogue v = acc + bias[n];  v = act(v)   (GLU: columns are interleaved in blocks of 16 as
 *           [a0..a15 | g0..g15 | a16.. ] and the output has N/2 columns = a * sigmoid(g));
 *           if row_mask && !row_mask[m]: v = 0   (or acc = 0 before the bias, see mask_mode);
 *           if residual: v = residual[m,n] + alpha * v;     store as c_dtype.
 *  conv     when conv_C > 0, A is a channels-last image [B, T1, F1, C] and row m = (b, t2, f2) of the
 *           3x3 stride-2 convolution output [B, T2, F2, N]; K = 9*C ordered (kt, kf, c).
 *
 * constraints: K % 8 == 0, lda % 8 == 0 (elements), ldc % 2 == 0, N % 2 == 0 (residual: both % 4; GLU: N % 32 == 0).
 * N or ldc not a multiple of 4 (a vocabulary of 5002 columns) is written with column-pair stores.
 */
#define CFM_TILE_AUTO_TRAIN (-1) /* cfm_gemm_desc.tile */
typedef struct {
    const void* A;
    const void* W;
    const void* W_lo;
    const float* bias;
    const float* residual;
    const uint8_t* row_mask;
    void* C;
    int64_t lda, ldc, ldr;
    int32_t M, N, K;
    int32_t a_dtype, w_dtype, c_dtype;
    int32_t act;
    float alpha;
    int32_t conv_C, conv_T1, conv_F1, conv_T2, conv_F2; /* conv_C == 0: plain GEMM */
    int32_t tile;                                       /* 0 = auto (every choice keeps the K order: results do not depend on M, a batch shard reproduces the
                                                           batch bit for bit); -1 = CFM_TILE_AUTO_TRAIN: auto, K-group tiles allowed; 1: 128x128, 2: 64x128, 3: 64x64, 4: 128x64, 5: 32x64, 6: 32x128,
                                                           7: 128x128 persistent workgroups (16-bit plain products, K %% 64 == 0),
                                                           8: 256x256 with LDS-DMA staging (csrc/gemm256.hip: 16-bit operands, K %% 64 == 0, bias / SiLU /
                                                              ReLU epilogues; auto when a cost model says its whole rounds beat the 128x128 tiles),
                                                           9 / 11 / 10: 32x64 k2 / 64x64 k2 / 64x64 k4 -- two or four K groups of four wavefronts per tile that meet
                                                              through LDS (16-bit operands, any epilogue; 11 is chosen under tile = -1 for K >= 1024 on <= 512 tiles
                                                              of 64x64: the long-K products of a training micro-batch) */
    int32_t mask_mode;                                  /* 0: row_mask zeroes the OUTPUT row (after act, before residual);
                                                           1: row_mask zeroes the INPUT row (acc = 0, bias/act still apply) */
    /* training: */
    void* C_pre;        /* optional second output [M,N] (row stride ld_pre, pre_dtype): acc + bias BEFORE the activation -- what the
                           backward of SiLU / GLU needs (feedforward.py:18, convolution.py:42).  GLU: all N interleaved columns. */
    int64_t ld_pre;
    int32_t pre_dtype;
    int32_t aux_dtype;  /* CFM_ACT_DSILU / CFM_ACT_DRELU: dtype and row stride of aux [M,N] */
    const void* aux;
    int64_t ld_aux;
    /* dropout on the OUTPUT element (m,n), after the activation and before row_mask / residual (train mode): kept with probability 1-p and
     * scaled by 1/(1-p); the mask is a pure function of (seed, m*N_out + n) (csrc/cfm_common.h cfm_hash32), so the backward passes the same
     * (p, seed) instead of reading a stored mask.  CFM_ACT_DSILU / CFM_ACT_DRELU apply it to acc (the gradient arriving at the dropped activation).
     * drop2: a second, independent mask on the same element (the plain MHSA's extra dropout after linear_out, attention.py:177). */
    float drop_p, drop2_p;
    uint32_t drop_seed, drop2_seed;
    /* ragged batches: rows are [B, row_T] flattened and row m = (b, t) with t >= row_len[b] is treated as row_mask[m] == 0 (mask_mode 0 only: the OUTPUT
     * row is zeroed after the activation -- with CFM_ACT_GLU the depthwise convolution behind it then reads zeros past the utterance's end, as at a tensor
     * edge).  NULL = every row is kept.  M % row_T == 0. */
    const int32_t* row_len;
    int32_t row_T;
} cfm_gemm_desc;

int cfm_gemm(const cfm_gemm_desc* d, cfm_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Weight gradient ("TN" product, csrc/gemm_tn.hip):   C[N,K] (+)= alpha * A[M,N]^T . B[M,K]      (f32 output, MFMA)
 * the d loss / d weight of every nn.Linear / Conv1d(k=1) / Conv2d(3,2) on the path: A = gradient of the layer's output rows,
 * B = the rows the layer consumed (what autograd computes for the `weight` of feedforward.py:17-20, attention.py:62-64,99,
 * convolution.py:41,46,62,74, decoder.py:19).  Both operands are read with the contraction index (the row m) as the SLOW index and
 * transposed on the way out of LDS (ds_read_b64_tr_b16), so no transposed copy of an activation is ever written.
 *  A, B      16-bit (mma_dtype) or f32 (rounded while staging; split = 1: both f32, hi/lo bf16 planes, 3 MFMAs: "f32-accurate")
 *  colsum    optional f32 [N]: (+)= alpha * sum_m A[m,n]     (the gradient of the layer's bias)
 *  row_mask  optional uint8 [M]: rows with 0 contribute nothing (padded frames of convolution.py:47-48)
 *  conv      conv_C > 0: B is a channels-last image [Bt, T1, F1, C] and row m = (b, t2, f2) of its 3x3 stride-2 im2col matrix,
 *            K = 9*C ordered (kt, kf, c) -- the weight gradient of the front-end's second convolution
 *  The M rows are split over `splits` workgroups per output tile (0 = auto) that add their partial products with f32 atomics;
 *  accumulate = 0 zero-fills C / colsum first (same stream).  splits = 1 is bitwise reproducible.
 * constraints: N % 8 == 0, K % 8 == 0, lda/ldb % 8 == 0 (16-bit) or % 4 (f32), ldc % 4 == 0.
 */
typedef struct {
    const void* A;
    const void* B;
    float* C;
    float* colsum;
    const uint8_t* row_mask;
    int64_t lda, ldb, ldc;
    int32_t M, N, K;
    int32_t a_dtype, b_dtype, mma_dtype;
    int32_t split, accumulate, splits;
    float alpha;
    int32_t conv_C, conv_T1, conv_F1, conv_T2, conv_F2;
    /* optional scatter of the output (needs accumulate = 1: the caller has zero-filled the destination): row n of C starts at C + row_off[n]
     * (elements) instead of C + n*ldc, column sum n goes to colsum[colsum_off[n]] -- lets one fused product (q|k|v, the interleaved
     * pointwise-conv-1 pack) write each reference parameter's gradient where it lives in a flat gradient buffer.  int64 [N], device. */
    const int64_t* row_off;
    const int64_t* colsum_off;
    int32_t tile; /* 0 = chosen by the library; 64 or 128: output tile edge (experiments, scripts/bench_gemm_tn_splits.py) */
    /* optional SECOND destination of column sum n: colsum[colsum_off2[n]] (entries < 0: none).  pos_bias_u's gradient is linear_q.bias'
     * gradient (attention.py:81: (q + u) . k^T), so the fused q|k|v product writes both.  int64 [N], device; needs accumulate = 1. */
    const int64_t* colsum_off2;
} cfm_gemm_tn_desc;

int cfm_gemm_tn(const cfm_gemm_tn_desc* d, cfm_stream_t stream);
/* n products in ONE launch (the weight gradients of a conformer block: feedforward.py:17-20 x 2, attention.py:62-64,99, convolution.py:41,46
 * under autograd): each is too small to fill the chip and none feeds the chain of input gradients, so a block's backward defers them to
 * its end.  Grouped when all are 16-bit products of one type without row mask / f32 split / implicit convolution and n <= 12; otherwise
 * one launch each, in order.  Same results as n calls of cfm_gemm_tn up to the order of the atomic sums. */
int cfm_gemm_tn_group(const cfm_gemm_tn_desc* descs, int32_t n, cfm_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Fused feed-forward block (one launch; the [M,FF] hidden activation never reaches memory):
 *     y  = (add_x ? x : 0) + alpha * ( W2 . act( W1 . LN(x; ln_g, ln_b) + b1 ) + b2 )
 *     y1 = ln1_g ? LN(y; ln1_g, ln1_b) : y        -> out_f32 (if non-NULL)
 *     y2 = ln2_g ? LN(y1; ln2_g, ln2_b) : y1      -> out16   (if non-NULL, 16-bit)
 * replaces norm + feed_forward(_macaron) + the residual add of encoder_layer.py:56-58 / :67-69 (and :70 through ln1,
 * the next sub-block's norm through ln2).  ln_g == NULL: no input LayerNorm (feedforward.py:16-21 on its own).
 *  x     f32 [M,D];  D in {144, 256};  FF % 32 == 0, FF <= 2048
 *  w1f   W1 [FF,D] packed fragment-major (see cfm/packing.py pack_ffn_fragments): 16-bit
 *        w1f[((ffb*KS1 + kk)*64 + lane)*8 + j] = W1[ffb*16 + (lane&15)][kk*32 + 8*(lane>>4) + j]   (0 for k >= D)
 *  w2f   W2 [D,FF] packed fragment-major with the k order of each 32-block permuted to accumulator order:
 *        w2f[((fs*(D/16) + nf)*64 + lane)*8 + j] = W2[nf*16 + (lane&15)][fs*32 + (j<4 ? 0 : 16) + 4*(lane>>4) + (j&3)]
 */
typedef struct {
    const float* x;
    const float *ln_g, *ln_b;
    const void *w1f, *w2f;
    const float *b1, *b2;
    const float *ln1_g, *ln1_b, *ln2_g, *ln2_b;
    float* out_f32;
    void* out16;
    int64_t M;
    int32_t D, FF;
    int32_t w_dtype, out16_dtype;
    int32_t act;   /* CFM_ACT_SILU | CFM_ACT_RELU */
    int32_t add_x;
    float alpha, eps;
} cfm_ffn_desc;

int cfm_ffn_fused(const cfm_ffn_desc* d, cfm_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Row-local chain on 32-row tiles, one launch (csrc/rowchain.hip):
 *     x  = head_a ? head_res + mask_out( head_a . Wh^T + head_b ) : x          (head_mask zeroes the product's row)
 *     xn = LN(x; ln_g, ln_b), rows with ln_mask == 0 zeroed
 *     y  = w1f ? x + alpha * FFN(xn) : x                                         (FFN as in cfm_ffn_fused, SiLU)
 *     y1 = ln1_g ? LN(y) : y -> out_f32        (head without FFN: out_f32 receives x, the new residual stream)
 *     y2 = ln2_g ? LN(y1) : xn -> the tail's input; behind a feed-forward with ln2_g also -> out16 (optional; not written otherwise)
 *     t  = tail_w ? y2 . Wt^T + tail_b, tail_glu: value*sigmoid(gate) on 16-column fragment pairs -> tail_out (16 bit)
 * The three chains of a conformer block (encoder_layer.py:56-70):
 *     macaron : x, LN_ffm, FFN_m, ln2 = LN_mha, tail = fused QKV                       (no head)
 *     conv-in : head = out-proj on the attention context + residual, LN_conv + pad mask, tail = pointwise-conv-1 + GLU
 *     final   : head = pointwise-conv-2 (+ pad mask) + residual, LN_ff, FFN, ln1 = LN_final
 * All matrices are 16-bit FRAGMENT-MAJOR: w[((nfrag*KS + kk)*64 + lane)*8 + j] = W[nfrag*16 + (lane&15)][kk*32 + 8*(lane>>4) + j]
 * for every matrix here, W2 included (the feed-forward keeps its hidden activation as a 32 x FF tile in LDS between the two
 * products, so W2 is read in natural k order).  Instances: D in {144, 256, 512} with the FF / tail sizes of those configs.
 */
typedef struct {
    const float* x;
    const void* head_a;
    const void* head_w;
    const float* head_b;
    const float* head_res;
    const uint8_t* head_mask;
    const float *ln_g, *ln_b;
    const uint8_t* ln_mask;
    const void *w1f, *w2n; /* fragment-major W1 [FF,D] and W2 [D,FF] (w2n: NATURAL k order, not cfm_ffn_fused's permuted w2f) */
    const float *b1, *b2;
    const float *ln1_g, *ln1_b, *ln2_g, *ln2_b;
    float* out_f32;
    void* out16;
    const void* tail_w;
    const float* tail_b;
    void* tail_out;
    int64_t M;
    int32_t D, FF, tail_N, tail_glu;
    int32_t w_dtype;
    float alpha, eps;
    float* out2_f32; /* optional f32 [M,D]: y2 = LN2(y1) as well (ln2_g required) -- e.g. the encoder's after_norm (encoder.py:74) applied to
                        the last block's output in the same launch */
    /* optional depthwise input stage of the "final" chain (head + feed-forward, no tail): head_a is the GLU output and
     *   a = SiLU( (DepthwiseConv15(head_a) + dw_b) * dw_scale + dw_shift )      rows [B, dw_T] flattened, zero padding at
     * utterance edges -- exactly cfm_dwconv_bn_silu (convolution.py:43-45) without its launch and its round trip. */
    const float *dw_w, *dw_b, *dw_scale, *dw_shift;
    int32_t dw_T, dw_K;
    /* optional SECOND feed-forward segment on the same rows, kept in registers (final chain of block i + macaron chain of block i+1):
     *     y1 = LN1(y)                       (as above; out_f32 may be NULL then: nothing else reads the block's output)
     *     z  = y1 + s2_alpha * FFN2( LN(y1; s2_ln_g, s2_ln_b) )   -> s2_out_f32
     *     y2 = LN(z; ln2_g, ln2_b) -> out16 / the tail's input;  the tail follows z.
     * Needs w1f (a first feed-forward), ln2_g and the same FF for both. */
    const float *s2_ln_g, *s2_ln_b;
    const void *s2_w1f, *s2_w2n;
    const float *s2_b1, *s2_b2;
    float* s2_out_f32;
    float s2_alpha;
    /* D = 512 (config 4: 3 984 rows are 125 row tiles for 256 CUs): the feed-forward of a chain split over PAIRS of workgroups, one half of FF each.
     *   psum_out  (with w1f, no head, no tail, no ln1 / ln2): the launch runs LN -> this workgroup's half of the feed-forward and leaves the partial
     *             sums psum_out[half][M][D] (f32, without b2 / alpha / residual).  2 x ceil(M/32) workgroups, halves on different XCDs.
     *   psum_in   (a chain without head and feed-forward): the rows are x + psum_alpha * (psum_in[0] + psum_in[1] + psum_b2) -> out_f32, then LN -> the
     *             tail; without a tail the normalised rows go to out2_f32. */
    float* psum_out;
    const float* psum_in;
    const float* psum_b2;
    float psum_alpha;
    /* The conv-in chain of the SAME block as the input stage of the depthwise stage (with dw_w and the second segment, D = 256): out-projection of the
     * attention context cin_a [M,D] (16 bit) + residual cin_res -> cin_out (this tile's rows; == head_res, != cin_res), LN(cin_ln_*; rows with cin_mask == 0
     * zeroed), pointwise-conv-1 + GLU (cin_tail_w: GLU-interleaved, fragment-major) -- computed per tile for its 32 + 14 halo rows, the GLU rows go
     * straight to the depthwise stage (head_a is not read, but stays non-NULL: it is what names the head).  One launch per block less than conv-in chain + this chain. */
    const void *cin_a, *cin_w;
    const float *cin_b, *cin_res;
    float* cin_out;
    const float *cin_ln_g, *cin_ln_b;
    const uint8_t* cin_mask;
    const void* cin_tail_w;
    const float* cin_tail_b;
    int32_t tail_pair; /* D = 512, a chain with a tail and no feed-forward: the tail's columns split over workgroup pairs (rows and LayerNorm computed by
                          both, written by the first); out_f32 must NOT alias head_res then */
    /* ragged batches (whole utterances of different lengths in one batch): rows are [B, glu_T] flattened and the GLU output of row (b, t) with
     * t >= glu_len[b] is written as ZERO -- a select behind the GLU, on the tail (tail_glu) and on the conv-in input stage (cin_*), so that the depthwise
     * stage reads zeros past the utterance's end exactly as it does past a tensor edge.  NULL = no select.  Needs tail_glu or cin_a, M % glu_T == 0. */
    const int32_t* glu_len;
    int32_t glu_T;
} cfm_rowchain_desc;

int cfm_rowchain(const cfm_rowchain_desc* d, cfm_stream_t stream);
/* 1 when cfm_rowchain has instances for all three chains of a block with these sizes (host query) */
int cfm_rowchain_supported(int32_t D, int32_t FF);
/* 1 when the depthwise input stage (dw_w ...) exists at this width; otherwise cfm_dwconv_bn_silu runs in front of the final chain (D = 512) */
int cfm_rowchain_dw_supported(int32_t D);
/* 1 when the pair-split feed-forward (psum_out / psum_in) has instances at this size */
int cfm_rowchain_pair_supported(int32_t D, int32_t FF);

/* ------------------------------------------------------------------------------------------------
 * LayerNorm (eps inside sqrt, biased variance), optionally two chained norms in one pass:
 *   y1 = LN(x; g1, b1);  if out1: out1 = y1 (out1_dtype)
 *   if g2:  y2 = LN(y1; g2, b2) else y2 = y1;  if out2: out2 = row_mask[m] ? y2 : 0  (out2_dtype)
 * replaces nn.LayerNorm at encoder_layer.py:57,60,64,68,70 and encoder.py:74, and the
 * masked_fill of convolution.py:36-37 (row_mask).   x is f32 [M,D]; D % 4 == 0, D <= 2048.
 */
int cfm_layernorm(const float* x, const float* g1, const float* b1, void* out1, int out1_dtype,
                  const float* g2, const float* b2, void* out2, int out2_dtype,
                  const uint8_t* row_mask, float eps, int64_t M, int32_t D, cfm_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Fused attention:  out[b,i,h,:] = softmax_j( scale * ((q_i+u_h).k_j + (q_i+v_h).p_{b,j}) ) . v_j
 * with masked scores = -inf and fully masked rows giving 0 (attention.py:81-96 / :162-172).
 *   q,k,v   element (b,t,h,d) at  base + b*sb + t*st + h*dk + d   (dtype 16-bit or f32)
 *   p       projected positions, element (b,j,h,d) at p + b*p_sb + j*p_st + h*dk + d;
 *           p_st == 0 broadcasts one row over all keys (the reference's batch path);
 *           p == NULL: plain MHSA (no u/v either).
 *   mask    uint8/bool, element (b,i,j) at mask + b*m_sb + i*m_sq + j ; m_sq == 0 broadcasts over
 *           queries; NULL = no mask.
 *   out     [B,Tq,H*dk] row-major, out_dtype.          dk <= 64.
 */
typedef struct {
    const void* q;
    const void* k;
    const void* v;
    const void* p;
    const float* bias_u; /* [H,dk] f32 */
    const float* bias_v; /* [H,dk] f32 */
    const uint8_t* mask;
    void* out;
    int64_t q_sb, q_st, k_sb, k_st, k_sh, v_sb, v_st, v_sh, p_sb, p_st, m_sb, m_sq;
    int32_t B, H, Tq, Tk, dk;
    int32_t q_dtype, kv_dtype, p_dtype, out_dtype, mma_dtype; /* mma_dtype: bf16|fp16 operand type */
    int32_t split;                                            /* 1: hi/lo bf16 split (f32-accurate) */
    float scale;
    float* lse;        /* optional (training): f32 [B,H,Tq], log-sum-exp of each row's scaled masked scores (-inf: fully masked) */
    float drop_p;      /* dropout on the attention probabilities (attention.py:93), element ((b*H+h)*Tq+i)*Tk+j; the softmax normaliser is */
    uint32_t drop_seed;/* that of the undropped row, as torch's softmax -> dropout gives */
} cfm_attn_desc;

int cfm_attention(const cfm_attn_desc* d, cfm_stream_t stream);
/* n attention problems in ONE launch: the micro-batches of a training window (cfm_train_group) differ in B, T and mask, and none fills the
 * chip alone.  Grouped when every problem takes the d_k = 64 fast path without a positional term (16-bit K/V, same mask kind), n <= 8;
 * otherwise one launch each, in order.  Results are those of n calls of cfm_attention. */
int cfm_attention_group(const cfm_attn_desc* descs, int32_t n, cfm_stream_t stream);

/* new_cache[b,h,t,0:dk] = K_t, [dk:2dk] = V_t with rows t < Tc copied from old_cache and rows t >= Tc
 * taken from (k,v) (same addressing as cfm_attn_desc).  f32 output [B,H,Tc+Tn,2dk].
 * replaces torch.split/cat of attention.py:70-76. */
int cfm_kv_cache_pack(const float* old_cache, int32_t Tc, const void* k, const void* v, int32_t kv_dtype,
                      int64_t k_sb, int64_t k_st, int64_t v_sb, int64_t v_st, float* new_cache,
                      int32_t B, int32_t H, int32_t Tn, int32_t dk, cfm_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Depthwise conv (k taps, zero padding at the tensor edges only) + per-channel affine (folded
 * BatchNorm, eval) + SiLU on a channels-last [B,T,D] activation.
 * replaces convolution.py:43-45.   w [D,Ktaps] f32, dw_bias/bn_scale/bn_shift [D] f32.
 *   y = silu( (sum_k w[d,k] x[b,t+k-(Ktaps-1)/2,d] + dw_bias[d]) * bn_scale[d] + bn_shift[d] )
 */
int cfm_dwconv_bn_silu(const void* x, int x_dtype, const float* w, const float* dw_bias,
                       const float* bn_scale, const float* bn_shift, void* y, int y_dtype, int32_t B,
                       int32_t T, int32_t D, int32_t ktaps, cfm_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Front-end first conv: x [B,T,F] f32 -> relu(conv3x3 stride 2) as channels-last [B,T1,F1,C].
 * replaces convolution.py:60-61.  w [9,C] f32 (tap-major), bias [C].  C % 8 == 0.
 * Optional global CMVN folded into the tap loads (cmvn.py:22-33, encoder.py:59-60): every input sample is read as
 * (x[b,t,f] - cmvn_mean[f]) * cmvn_istd[f]  (cmvn_istd NULL: mean only; both NULL: plain) -- the same two f32 operations the
 * reference applies before the convolution, so results are bit-identical to normalising first.
 */
int cfm_conv1_relu(const float* x, const float* w, const float* bias, void* y, int y_dtype, int32_t B,
                   int32_t T, int32_t F, int32_t C, const float* cmvn_mean, const float* cmvn_istd, cfm_stream_t stream);

/* The same convolution on the matrix pipe (csrc/convmod.hip cfm_conv1_mma_kernel): the 9 taps as a K = 32 MFMA contraction.  Inputs
 * (after the optional CMVN, applied in f32) and weights are ROUNDED to the 16-bit type y_dtype (bf16 / f16), products accumulate in
 * f32 on top of the bias; cfm_conv1_relu multiplies in f32.  For the 16-bit precision modes, whose conv1 output is 16-bit anyway.
 * C % 16 == 0, C <= 256.  Same arguments otherwise. */
int cfm_conv1_relu_mma(const float* x, const float* w, const float* bias, void* y, int y_dtype, int32_t B, int32_t T, int32_t F,
                       int32_t C, const float* cmvn_mean, const float* cmvn_istd, cfm_stream_t stream);

/* Both front-end convolutions in one kernel (csrc/frontend.hip): relu(conv3x3 s2 (relu(conv3x3 s2 (x)))) -> y [B,T2,F2,C] channels-last in
 * the 16-bit type y_dtype.  replaces convolution.py:60-63 in eval mode.  The first convolution is recomputed inside the second one's
 * A-operand producer with the operands of cfm_conv1_relu_mma, so its [B,T1,F1,C] output never exists in memory; the result is
 * bit-identical to cfm_conv1_relu_mma followed by cfm_gemm(conv_*, ReLU) on the same packed weights.
 * w1 [9,C] f32 tap-major, b1 [C], w2 [C, 9*C] 16-bit (y_dtype) in K order (kt, kf, ci), b2 [C] f32.  C in {64,128,192,256}.  CMVN as cfm_conv1_relu. */
int cfm_conv12_supported(int32_t C, int32_t y_dtype);
int cfm_conv12_relu(const float* x, const float* w1, const float* b1, const void* w2, const float* b2, void* y, int32_t y_dtype, int32_t B,
                    int32_t T, int32_t F, int32_t C, const float* cmvn_mean, const float* cmvn_istd, cfm_stream_t stream);
/* The row tiles of cfm_conv12_relu are 32 fm rows (fm = 2, 3, 4, 8, 10).  cfm_conv12_plan: the host's choice for M output rows, C channels
 * and a chip of `cus` compute units, without touching a device -- rows on fm_main tiles first (whole rounds of 256-row tiles, or every row
 * on 256- or 320-row tiles in one launch; 0 = no such launch), the remaining rows as one round of fm_tail tiles (0 = none); by a cost
 * model of rounds x K steps x time per step of each tile (csrc/frontend.hip).  cfm_set_conv12_tile(fm): every row on tiles of 32 fm rows
 * whatever the plan says (0 = by the plan, the default; another value leaves the setting alone); returns the previous setting.  Every
 * tile gives the same bits; the switch is host-side and exists for tests and measurements. */
int cfm_conv12_plan(int64_t M, int32_t C, int32_t cus, int32_t* fm_main, int32_t* fm_tail);
int32_t cfm_set_conv12_tile(int32_t fm);

/* ------------------------------------------------------------------------------------------------
 * Masks -- integer/bool, bit-exact with the reference.
 *  cfm_valid_mask     out[b,t] = (t*stride + first) < len[b]     (uint8 0/1), t in [0,T)
 *                     first=0,stride=1: ~make_pad_mask (utils.py:84-93, encoder.py:62);
 *                     first=6,stride=4: the subsampled mask of convolution.py:76 built straight from lengths.
 *  cfm_chunk_mask     out[i,j] = start_i <= j < end_i            (utils.py:96-111)
 *  cfm_attn_mask      out[b,i,j] = valid[b,j] & chunk[i,j]       (utils.py:150-152)
 */
int cfm_valid_mask(const void* lengths, int len_is_i64, uint8_t* out, int32_t B, int32_t T, int32_t first,
                   int32_t stride, cfm_stream_t stream);
int cfm_chunk_mask(uint8_t* out, int32_t size, int32_t chunk, int32_t left, cfm_stream_t stream);
int cfm_attn_mask(const uint8_t* valid, const uint8_t* chunk, uint8_t* out, int32_t B, int32_t T,
                  cfm_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Per-stream state of the batched streaming step (csrc/stream.hip) -- beyond the reference, whose forward_chunk serves one stream at a
 * time (encoder.py:78-123) and rebuilds its cache with cat + slice (:117).  offsets int32 [B] on the device: encoder frames each stream has
 * consumed.  need = chunk * left_chunks cached frames, ring_T >= need + T slots.
 *  cfm_stream_prep     slot_mask u8 [B,ring_T] = slot holds a frame of [offset-min(offset,need), offset+c_b); pos_rows f32 [B,ring_T,D] = pe[that
 *                      frame] (pe f32 [max_len,D], the sinusoid table of attention.py:12-16); abs_rows f32 [B,D] = pe[offset] (optional: the
 *                      absolute encoding's row, attention.py:119-120).  frame_lens NULL (then out_lens NULL too): whole windows, c_b = T.  Else
 *                      per-stream lengths: stream b's window holds frame_lens[b] valid FEATURE frames (left-aligned, 0 .. window), hence
 *                      out_lens[b] = c_b = ((n-1)/2-1)/2 encoder frames (0 for n < 7; capped at T), which it writes: the newest frame is
 *                      offset + c_b - 1, the mask covers the min(offset, need) cached frames and the c_b new ones (c_b = 0: the cached frames only;
 *                      none at offset 0).  The other three take lens = out_lens, and lens[b] = 0 changes nothing of stream b.
 *  cfm_kv_ring_write   K / V rows of the T new frames (addressed like cfm_attn_desc k / v, head h at h*dk) -> ring slots (offset+t) mod ring_T.
 *                      lens NULL: whole windows; else rows t < lens[b] only.
 *  cfm_stream_advance  lens NULL: offset[b] += T for streams with active[b] != 0 (active NULL: all).  Else offset[b] += lens[b] (clamped to 0 .. T; not
 *                      with active) and rows t >= lens[b] of y f32 [B,T,D] (optional, needs lens and D % 4 == 0) are set to zero.
 *  cfm_dwconv_causal_bn_silu  y = SiLU(BN_eval(causal depthwise conv over [cache | x])), cache f32 [B,ktaps-1,D] or NULL (zeros)
 *  cfm_conv_cache_update      cache <- last ktaps-1 frames of [cache | x], in place.  lens NULL: whole windows; else of [cache | x[:lens[b]]] per stream
 */
int cfm_stream_prep(const int32_t* offsets, const int32_t* frame_lens, int32_t* out_lens, int32_t B, int32_t T, int32_t need, int32_t ring_T,
                    const float* pe, int32_t max_len, int32_t D, uint8_t* slot_mask, float* pos_rows, float* abs_rows, cfm_stream_t stream);
int cfm_kv_ring_write(const void* k, const void* v, int32_t kv_dtype, int64_t k_sb, int64_t k_st, int64_t v_sb, int64_t v_st, float* ring,
                      const int32_t* offsets, const int32_t* lens, int32_t B, int32_t H, int32_t T, int32_t dk, int32_t ring_T, cfm_stream_t stream);
int cfm_stream_advance(int32_t* offsets, const uint8_t* active, const int32_t* lens, float* y, int32_t B, int32_t T, int32_t D, cfm_stream_t stream);
int cfm_dwconv_causal_bn_silu(const void* x, int32_t x_dtype, const float* cache, const float* w, const float* dw_bias, const float* bn_scale,
                              const float* bn_shift, void* y, int32_t y_dtype, int32_t B, int32_t T, int32_t D, int32_t ktaps, cfm_stream_t stream);
int cfm_conv_cache_update(const void* x, int32_t x_dtype, float* cache, const int32_t* lens, int32_t B, int32_t T, int32_t D, int32_t ktaps,
                          cfm_stream_t stream);

/* element-wise dtype conversion:  dst = cast(src) */
int cfm_cast(const void* src, int src_dtype, void* dst, int dst_dtype, int64_t n, cfm_stream_t stream);
/* x[r,:] += add[r / group, :]   (f32, in place; the absolute positional encoding of attention.py:119-120,
 * where one table row is added to every frame of a batch item: group = T') */
int cfm_add_rows(float* x, const float* add, int64_t rows, int32_t D, int32_t group, cfm_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Composite: one conformer block / the whole encoder stack, enqueued from C++ so that a forward is
 * ~1 host call instead of ~170 (encoder_layer.py:49-71 and the loop at encoder.py:72-74).
 * Weights are the PACKED device copies the Python side prepares once (see cfm/packing.py).
 */
typedef struct {
    /* layer norms, f32 [D] */
    const float *ln_ffm_g, *ln_ffm_b, *ln_mha_g, *ln_mha_b, *ln_conv_g, *ln_conv_b, *ln_ff_g, *ln_ff_b,
        *ln_final_g, *ln_final_b;
    /* macaron FFN, FFN: W 16-bit [FF,D] / [D,FF] (+ lo planes in split mode), bias f32 */
    const void *ffm_w1, *ffm_w1_lo, *ffm_w2, *ffm_w2_lo;
    const float *ffm_b1, *ffm_b2;
    const void *ff_w1, *ff_w1_lo, *ff_w2, *ff_w2_lo;
    const float *ff_b1, *ff_b2;
    /* optional fragment-major packs for cfm_ffn_fused / cfm_rowchain (NULL: the separate-GEMM path is used) */
    const void *ffm_w1f, *ffm_w2f, *ff_w1f, *ff_w2f;
    const void *ffm_w2n, *ff_w2n; /* W2 fragment-major in natural k order: what cfm_rowchain reads (w2f: cfm_ffn_fused) */
    const void *qkv_wf, *out_wf, *pw1_wf, *pw2_wf;
    /* attention: fused qkv [3D,D], pos [D,D] (NULL for plain MHSA), out [D,D] */
    const void *qkv_w, *qkv_w_lo, *pos_w, *pos_w_lo, *out_w, *out_w_lo;
    const float *qkv_b, *out_b, *bias_u, *bias_v;
    /* conv module: pw1 [2D,D] GLU-interleaved, dw [D,K], folded BN, pw2 [D,D] */
    const void *pw1_w, *pw1_w_lo, *pw2_w, *pw2_w_lo;
    const float *pw1_b, *pw2_b, *dw_w, *dw_b, *bn_scale, *bn_shift;
} cfm_layer_weights;

typedef struct {
    void *xn, *hid, *qkv, *pos, *ctx, *glu, *dw; /* activation-dtype scratch: [M,D],[M,FF],[M,3D],[R,D],[M,D],[M,D],[M,D] */
    float* psum;   /* optional f32 [psum_splits, M, D]: partial slabs of a split feed-forward; null = the block never takes CFM_ROUTE_FFSPLIT / _PAIR.
                      CFM_ROUTE_FFSPLIT: psum_splits >= FF/256, at most cfm_ffsplit_max_rows() rows at D = 256 (cfm_ffn_split_supported) -- both feed-forwards
                      split over FF/256 workgroups per 32-row tile instead of inside the row chains (few rows: a streaming step).  CFM_ROUTE_PAIR:
                      psum_splits >= 3, at most CFM_PAIR_MAX_ROWS rows at D = 512 (cfm_rowchain_pair_supported) -- both feed-forwards split over workgroup
                      PAIRS (two slabs + the parked rows of the final chain): 125 row tiles alone leave half of the CUs idle */
    int32_t psum_splits;
} cfm_layer_scratch;
#define CFM_PAIR_MAX_ROWS 4096    /* 128 row tiles x 2 halves = one workgroup per CU */
#define CFM_FFSPLIT_MAX_ROWS 1536 /* measured crossover against the row chains: 996 rows -21 %, 1992 rows +4 % (scripts/bench_small_batch.py) */

typedef struct {
    int32_t B, T, D, H, FF, ktaps;
    int32_t act_dtype; /* CFM_BF16 | CFM_F16 (16-bit modes) | CFM_F32 (split mode) */
    int32_t w_dtype;   /* CFM_BF16 | CFM_F16 */
    const uint8_t* attn_mask;
    int64_t am_sb, am_sq;     /* see cfm_attn_desc.mask */
    const uint8_t* pad_valid; /* [B*T] or NULL */
    const float* pos_embed;   /* f32 [R,D] rows, R = B*P */
    int32_t pos_rows;         /* R (0: plain MHSA) */
    const void* pos_proj;     /* optional: linear_pos(pos_embed) already projected (act dtype), row stride pos_proj_ld;
                                 lets the driver project the positions of ALL blocks with one GEMM */
    int64_t pos_proj_ld;
    const float* attn_cache;  /* f32 [B,H,Tc,2dk] or NULL */
    int32_t cache_T;
    float* new_cache;         /* f32 [B,H,Tc+T,2dk] or NULL (not materialised) */
    const float *after_g, *after_b; /* optional: ALSO write LN(x_out; after_g, after_b) to after_out (f32 [B*T,D]) -- the encoder's after_norm, fused into the
                                       last block's final launch on CFM_ROUTE_CHAIN / _FFSPLIT, one more LayerNorm launch on the other routes; not with next_w */
    float* after_out;
    /* Batched streaming with PER-STREAM state (csrc/stream.hip; beyond the reference): when kv_ring is set, this layer's keys /
     * values live in a ring buffer f32 [B,H,ring_T,2dk] (frame f of a stream in slot f mod ring_T); the step's T new frames of stream b are
     * frames stream_offset[b] .. +T-1 and are written to their slots, attention runs over all ring_T slots with attn_mask = the (B,1,ring_T)
     * slot mask and pos_rows = B*ring_T positional rows (both from cfm_stream_prep).  attn_cache / new_cache are unused then. */
    float* kv_ring;
    const int32_t* stream_offset;
    int32_t ring_T;
    /* OPT-IN causal depthwise convolution (not in the reference, which has no causal mode and ignores cnn_cache: convolution.py:34-39):
     * taps reach back ktaps-1 frames instead of (ktaps-1)/2 each way; conv_cache f32 [B,ktaps-1,D] (optional) is the left context of this
     * chunk -- the last GLU outputs of the previous one -- and is updated in place.  0 = the reference's symmetric convolution. */
    int32_t causal_conv;
    float* conv_cache;
    int32_t pos_shared;       /* 1: the pos_rows == Tk positional rows are the SAME for every batch item (batched streaming step: all
                                 streams at one offset).  Beyond the reference, whose forward_chunk only works at batch 1
                                 (attention.py:78-88); per item it equals that batch-1 call. */
    /* Chaining consecutive blocks (CFM_ROUTE_CHAIN_NEXT / _CHAIN_NEXT_CIN; needs every chain pack, else next_w is not read): the final chain of this block and the macaron chain of the NEXT block are both
     * row-local, so one launch can run them back to back on rows that stay in registers (cfm_rowchain_desc.s2_*): one launch, one f32
     * read and one f32 write of the residual stream less per block.
     *   next_w != NULL : after norm_final, run the next block's macaron feed-forward + norm_mha + fused QKV projection as well; the
     *                    next block's post-macaron residual goes to next_x_out (f32 [B*T,D]) and its q|k|v rows to s->qkv.  x_out then
     *                    does NOT receive this block's output (it is left holding the residual stream before the feed-forward).
     *   macaron_done   : this block's macaron chain already ran in the previous block's call: x_out holds its residual, s->qkv its
     *                    projections; x_in is not read.  A modifier of the three CFM_ROUTE_CHAIN* routes (it excludes _FFSPLIT and _PAIR); an error elsewhere. */
    const cfm_layer_weights* next_w;
    float* next_x_out;
    int32_t macaron_done;
    /* A ragged batch of WHOLE utterances (beyond the reference, which decodes them at batch 1): int32 [B], item b has utt_len[b] <= T frames and the frames
     * behind them do not exist for the convolution module -- the GLU output of rows t >= utt_len[b] is zero, so the depthwise convolution sees what it
     * sees at a tensor edge (masking in front of pointwise_conv1, as pad_valid does, leaves GLU(bias) there instead).  On every route.  The caller masks
     * the keys t >= utt_len[b] through attn_mask; rows at and past utt_len[b] of x_out hold no defined result.  NULL = today's behaviour.
     * Not with kv_ring, attn_cache, causal_conv or pad_valid. */
    const int32_t* utt_len;
    /* The batched streaming step with PER-STREAM window lengths (needs kv_ring): int32 [B], only the first stream_len[b] <= T rows of stream b are frames
     * of its utterance (a short final chunk, or 0 for an idle stream).  What utt_len does for whole utterances -- the same select behind the GLU, on every
     * route, so the symmetric depthwise convolution of a valid row sees zeros past the stream's end, as the reference's batch-1 forward_chunk on the
     * shorter window does -- plus the streaming state: only rows t < stream_len[b] are written to the K/V ring (cfm_kv_ring_write with lens, or
     * cfm_ffn_split_desc.ring_len on CFM_ROUTE_FFSPLIT) and enter conv_cache (cfm_conv_cache_update with lens); stream_len[b] = 0 leaves both untouched.
     * attn_mask is the slot mask of cfm_stream_prep with frame_lens.  Rows at and past stream_len[b] of x_out hold no defined result (non-finite values included)
     * and reach no valid row.  NULL = every stream has T rows, as before.  Not with utt_len, attn_cache or pad_valid. */
    const int32_t* stream_len;
} cfm_layer_io;

/* The launch sequence of one block.  Every argument is checked and ONE route chosen before anything is launched (csrc/encoder.cpp select_route).
 * chains = all eight fragment-major chain packs (ffm_w1f, ffm_w2n, ff_w1f, ff_w2n, qkv_wf, out_wf, pw1_wf, pw2_wf), a 16-bit act_dtype and
 * cfm_rowchain_supported(D, FF).  Without chains: FUSED_FFN when the *_w1f / *_w2f packs are there, D in {144, 256}, FF % 32 == 0 and FF <= 2048, else
 * GENERAL.  With chains, the first that applies: PAIR and FFSPLIT (cfm_layer_scratch.psum; neither with macaron_done or next_w, FFSPLIT also needs pw2_w
 * and 15 taps; D = 512 against D = 256, so they exclude each other), CHAIN_NEXT_CIN (next_w, cfm_set_cin_merge on), CHAIN_NEXT (next_w), CHAIN. */
typedef enum {
    CFM_ROUTE_GENERAL = 0,        /* separate GEMMs, LayerNorm and depthwise kernels: 17 launches */
    CFM_ROUTE_FUSED_FFN = 1,      /* ... with each feed-forward as one cfm_ffn_fused launch */
    CFM_ROUTE_CHAIN = 2,          /* the three row chains (cfm_rowchain) around the attention: 4 launches */
    CFM_ROUTE_CHAIN_NEXT = 3,     /* ... the final chain also runs the next block's macaron chain: 3 per block */
    CFM_ROUTE_CHAIN_NEXT_CIN = 4, /* ... and the conv-in chain as the input stage of that launch: 2 per block */
    CFM_ROUTE_FFSPLIT = 5,        /* both feed-forwards split over FF (cfm_ffn_split) */
    CFM_ROUTE_PAIR = 6            /* both feed-forwards split over workgroup pairs (cfm_rowchain_desc.psum_out / psum_in) */
} cfm_route;

/* x_in f32 [B*T,D] (not modified) -> x_out f32 [B*T,D] = norm_final(block(x_in)).
 * xn_ready / next_g / next_b are read on CFM_ROUTE_GENERAL only: xn_ready != 0 says s->xn already holds LN_ffm(x_in); if next_g != NULL the call additionally
 * writes LN(x_out; next_g,next_b) to s->xn for the following block. */
int cfm_encoder_layer_forward(const cfm_layer_weights* w, const cfm_layer_scratch* s, const cfm_layer_io* io,
                              const float* x_in, float* x_out, int xn_ready, const float* next_g,
                              const float* next_b, cfm_stream_t stream);
/* The cfm_route that call would take, or its negative cfm_status (cfm_last_error() set) -- the same checks, asked on the host: no launch, no HIP call, and no
 * pointer dereferenced but the three structs and io->next_w, so it also runs where there is no GPU and with made-up addresses. */
int32_t cfm_encoder_layer_route(const cfm_layer_weights* w, const cfm_layer_scratch* s, const cfm_layer_io* io, const float* x_in, const float* x_out);
/* The row limit of CFM_ROUTE_FFSPLIT in force: CFM_FFSPLIT_MAX_ROWS, or the environment variable of that name at first use (experiments). */
int32_t cfm_ffsplit_max_rows(void);

/* ------------------------------------------------------------------------------------------------
 * CTC negative log-likelihood per utterance on top of the vocabulary projection (csrc/ctc.hip):
 * replaces  probs = logits.transpose(0,1).log_softmax(2); nn.CTCLoss(reduction='sum')(probs, labels, enc_lens, label_lens)
 * of CTCDecoder.forward (reference src/decoder.py:20-21; blank = 0, no zero_infinity).  logits f32 [B,T,ld>=V] (from cfm_gemm with
 * ctc_lo.weight / bias), labels int32 [B,Umax] (padding ignored beyond label_lens[b]), work f32 scratch [B,T,2*Umax+2], nll f32 [B];
 * the caller sums nll and divides by Umax as decoder.py:22 does.  Umax <= 255.  An impossible alignment gives +inf, like nn.CTCLoss.
 */
int cfm_ctc_nll(const float* logits, int64_t ld, int32_t B, int32_t T, int32_t V, const int32_t* enc_lens,
                const int32_t* labels, int32_t Umax, const int32_t* label_lens, float* work, float* nll, cfm_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Transducer joint, activation operand (csrc/joint.hip):  replaces
 *     out = enc_out.unsqueeze(2) + pred_out.unsqueeze(1);  out = tanh(out)        (reference src/joint.py:31-37)
 * enc f32 [B*T, ld_e >= J] = enc_ffn(encoder_out), pred f32 [B*U, ld_p >= J] = pred_ffn(predictor_out) (both from cfm_gemm);
 * out [B*T*U, J] row-major in out_dtype (f32 / bf16 / f16), row (b*T + t)*U + u = tanh(enc[b*T+t] + pred[b*U+u]).
 * The vocabulary projection ffn_out is then cfm_gemm over these rows (N = vocab_size may be any multiple of 2).  J % 8 == 0.
 */
int cfm_joint_act(const float* enc, int64_t ld_e, const float* pred, int64_t ld_p, void* out, int32_t out_dtype, int32_t B,
                  int32_t T, int32_t U, int32_t J, cfm_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * RNN-T loss (csrc/rnnt.hip):  replaces
 *     torchaudio.functional.rnnt_loss(joint_out, rnnt_text, encoder_out_lens, rnnt_text_lengths, blank=self.blank, reduction="mean")
 * of Transducer.rnnt_loss (reference src/model.py:107; fused_log_softmax = True), per utterance and with the gradient w.r.t. the logits.
 *  logits       [B, T, U1, ld >= V] (logits_dtype f32 / bf16 / fp16; U1 = U + 1), arithmetic f32
 *  targets      int32 [B, U1-1] (labels y_1..y_U; may be NULL when U1 == 1), logit_lens / target_lens int32 [B] (clamped to [0,T] / [0,U1-1])
 *  lse, lp_blank, lp_label, alpha, beta   f32 [B, T, U1] work arrays (only t < T_b, u <= U_b are written); shift f32 [B, T + U1]
 *  nll          f32 [B]: -log P(y | x) per utterance (+inf when T_b = 0); nll_shifted / ll_alpha f32 [B]: -beta'[0,0] and alpha'[T_b-1,U_b] +
 *               lp_blank' of the shifted recursions (csrc/rnnt.hip) -- equal up to f32 rounding
 * cfm_rnnt_nll  the row pass (log-sum-exp, blank and label log-probabilities per node) and both recursions (2 B workgroups, one barrier per
 *               diagonal); fills the arrays above.  U1 <= 1024, T <= 8192.
 * cfm_rnnt_grad after cfm_rnnt_nll with the same desc: grad [B, T, U1, ld_grad] (grad_dtype) columns 0..grad_cols-1 (V <= grad_cols <= ld_grad) =
 *               s_b * clamp(d nll_b / d logits, +-clamp) (clamp <= 0: none), s_b = gscale * (gscale_dev ? gscale_dev[b * gscale_stride] : 1) (a
 *               DEVICE scale: no host synchronisation); exact zeros outside t < T_b, u <= U_b and in columns V..grad_cols-1.  grad may be the
 *               logits themselves (in place) when ld_grad * sizeof(grad) == ld * sizeof(logits) and the gradient type is no wider than the logits'.
 */
typedef struct {
    const void* logits;
    int64_t ld;
    int32_t logits_dtype;
    int32_t B, T, U1, V, blank;
    const int32_t* targets;
    const int32_t* logit_lens;
    const int32_t* target_lens;
    float *lse, *lp_blank, *lp_label, *alpha, *beta, *shift;
    float *nll, *nll_shifted, *ll_alpha;
    /* cfm_rnnt_grad only: */
    void* grad;
    int64_t ld_grad;
    int32_t grad_dtype, grad_cols;
    float gscale;
    int32_t gscale_stride; /* 0: one scalar for all utterances; 1: gscale_dev[b] (reduction "none") */
    const float* gscale_dev;
    float clamp;
} cfm_rnnt_desc;
int cfm_rnnt_nll(const cfm_rnnt_desc* d, cfm_stream_t stream);
int cfm_rnnt_grad(const cfm_rnnt_desc* d, cfm_stream_t stream);

/* Backward of the joint's activation (csrc/joint.hip), the train path of TransducerJoint.rnnt_loss (reference src/joint.py:31-37 under
 * autograd): a = tanh(enc[b*T+t] + pred[b*U+u]) recomputed from the f32 projections (as cfm_joint_act), dz = dact (1 - a^2) with dact f32
 * [B*T*U, J]; d_enc f32 [B*T, J] = sum_u dz, d_pred f32 [B*U, J] = sum_t dz, both in a fixed order (no atomics).  work: f32 scratch of
 * cfm_joint_act_bwd_ws(B, T, U, J) floats.  J % 8 == 0. */
int64_t cfm_joint_act_bwd_ws(int32_t B, int32_t T, int32_t U, int32_t J);
int cfm_joint_act_bwd(const float* enc, int64_t ld_e, const float* pred, int64_t ld_p, const float* dact, float* d_enc, float* d_pred,
                      float* work, int32_t B, int32_t T, int32_t U, int32_t J, cfm_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Packed ("compact") RNN-T lattices: only the valid nodes of a ragged batch get a row.  Utterance b owns the rows
 * [off[b], off[b] + T[b] (U[b]+1)) of a [M, V] logits matrix, M = off[B]; row off[b] + t (U[b]+1) + u is node (b, t, u).  The encoder row of
 * (b, t) is enc_row0[b] + t and the predictor row of (b, u) is pred_row0[b] + u, so one descriptor covers one padded batch (enc_row0[b] = b T')
 * and the row matrix of an accumulation window whose micro-batches have different T' (ConformerEncoder.forward_window(return_rows=True)).
 * Encoder rows are owned in order: rows [enc_row0[b], enc_row0[b+1]) (the last: up to n_enc) belong to b, the ones with t >= T[b] are padding
 * (likewise the predictor rows with u > U[b]).  Every array is on the device and built by the caller from host lengths (the offsets are a
 * prefix sum): T[b] >= 0 frames, U[b] >= 0 labels, T_max >= max T[b], U1_max >= max U[b] + 1; blk_off[b] = sum_{b' < b} ceil(T[b'] / 8) (U[b'] + 1)
 * (the rows of cfm_joint_act_packed_bwd's per-frame-block partials, blk_off[B] of them).
 */
typedef struct {
    int32_t B, T_max, U1_max;
    int64_t M;                    /* = off[B] */
    const int64_t* off;           /* [B + 1] */
    const int32_t* T;             /* [B] */
    const int32_t* U;             /* [B] */
    const int64_t* enc_row0;      /* [B], nondecreasing */
    const int64_t* pred_row0;     /* [B], nondecreasing */
    int64_t n_enc, n_pred;        /* rows of the encoder / predictor matrices */
    const int64_t* blk_off;       /* [B + 1] */
} cfm_lattice;

/* Joint activation over a packed lattice (csrc/joint.hip): replaces the broadcast of joint.py:31-37 (as cfm_joint_act) for the valid cells only:
 * out [M, J] (out_dtype f32 / bf16 / f16) row off[b] + t (U[b]+1) + u = tanh(enc[enc_row0[b] + t] + pred[pred_row0[b] + u]).  J % 8 == 0.
 * cfm_joint_act_packed_bwd: dz = dact (1 - a^2) over dact f32 [M, J], d_enc f32 [n_enc, J] = sum_u dz, d_pred f32 [n_pred, J] = sum_t dz, both in a
 * fixed order (no atomics), exact zeros in the padding rows; work: f32 scratch of blk_off[B] * J floats. */
int cfm_joint_act_packed(const float* enc, int64_t ld_e, const float* pred, int64_t ld_p, void* out, int32_t out_dtype, const cfm_lattice* lat,
                         int32_t J, cfm_stream_t stream);
int cfm_joint_act_packed_bwd(const float* enc, int64_t ld_e, const float* pred, int64_t ld_p, const float* dact, float* d_enc, float* d_pred,
                             float* work, const cfm_lattice* lat, int32_t J, cfm_stream_t stream);

/* RNN-T loss over a packed lattice (csrc/rnnt.hip): torchaudio.functional.rnnt_loss of Transducer.rnnt_loss (reference src/model.py:107) on the
 * valid nodes only, what cfm_rnnt_nll / cfm_rnnt_grad compute on the same nodes of a padded [B, T, U1, ld] buffer (same per-node code: the
 * costs are the same bits).  logits [M, ld >= V]; targets int32 row b at targets + b * ld_targets (U[b] labels; may be NULL when every U[b] is 0);
 * lse, lp_blank, lp_label, alpha, beta f32 [M]; shift f32 [B, T_max + U1_max]; nll, nll_shifted, ll_alpha f32 [B] (+inf / -inf when T[b] = 0).
 * The gradient fields are those of cfm_rnnt_desc: grad [M, ld_grad] (may be the logits, in place), per-utterance gscale_dev[b * gscale_stride].
 * U1_max <= 1024, T_max <= 8192 (cfm_last_error otherwise). */
typedef struct {
    cfm_lattice lat;
    const void* logits;
    int64_t ld;
    int32_t logits_dtype, V, blank, ld_targets;
    const int32_t* targets;
    float *lse, *lp_blank, *lp_label, *alpha, *beta, *shift;
    float *nll, *nll_shifted, *ll_alpha;
    /* cfm_rnnt_packed_grad only: */
    void* grad;
    int64_t ld_grad;
    int32_t grad_dtype, grad_cols;
    float gscale;
    int32_t gscale_stride;
    const float* gscale_dev;
    float clamp;
} cfm_rnnt_packed_desc;
int cfm_rnnt_packed_nll(const cfm_rnnt_packed_desc* d, cfm_stream_t stream);
int cfm_rnnt_packed_grad(const cfm_rnnt_packed_desc* d, cfm_stream_t stream);

/* cfm_rnnt_align / cfm_rnnt_packed_align: RNN-T forced alignment (csrc/rnnt.hip) -- the best single alignment of each utterance's frames to ITS
 *   labels over the transducer lattice, the max-plus (Viterbi) twin of cfm_rnnt_nll's alpha recursion (as cfm_ctc_align is of cfm_ctc_nll's).  The
 *   reference has nothing of the kind; the algorithm is stated in float64 in tests/rnnt_align_ref.py.  `r` is the loss's descriptor, read exactly
 *   as cfm_rnnt_nll / cfm_rnnt_packed_nll read it (logits, lengths and their clamping, labels clamped into [0, V), blank); r.lse, r.lp_blank
 *   and r.lp_label are required work arrays of the loss's sizes and are filled as the loss fills them; r.shift, r.alpha, r.beta, r.nll,
 *   r.nll_shifted, r.ll_alpha and the gradient fields are not used and may be NULL (the shifts live in LDS; nothing reads them afterwards).
 *   With lb[t,u] = log_softmax(logits[t,u,:V])[blank], ll[t,u] = log_softmax(logits[t,u,:V])[y_{u+1}], Tb = logit_lens[b] clamped to [0, T] and
 *   Ub = target_lens[b] clamped to [0, U1-1] (packed: lat.T[b], lat.U[b]):
 *       delta[0,0] = 0
 *       delta[t,u] = max(delta[t-1,u] + lb[t-1,u]   (the blank move, only where t > 0),
 *                        delta[t,u-1] + ll[t,u-1])  (the label move, only where u > 0)
 *       score      = delta[Tb-1,Ub] + lb[Tb-1,Ub]
 *   Ties: the blank move is taken first; the label move replaces it only if it is STRICTLY greater.  From (Tb-1, Ub) the recorded moves are
 *   followed back to (0, 0).  The recursion runs in f32 on the loss's shifted values (lb[t,u] - max_u lb[t,.], ll[t,u] - max_t ll[.,u]: every
 *   path to a node takes the same offsets, so no decision moves); the offsets are added back to the score in fp64.
 *   score f32 [B]: the path's log-probability; -inf when Tb == 0 (the final blank needs a frame; the loss is +inf there).
 *   frame int32 [B, Umax]: frame[u] is the t of the label move (t,u) -> (t,u+1) that emits label u (0-based); nondecreasing in u, several
 *     labels may share a frame.  token_logp f32 [B, Umax]: ll[frame[u], u].  Entries u >= Ub, and all of an utterance with Tb == 0, are -1 and
 *     -inf.  Umax = U1 - 1 (padded) or lat.U1_max - 1 (packed).
 *   scratch: the recorded moves, scratch_bytes >= cfm_rnnt_align_scratch_bytes(nodes), nodes = B * T * U1 (padded) or lat.M (packed): two
 *     bytes per node (per node the last frame at which its column was entered by a label move, so the trace-back is Ub dependent loads),
 *     rounded up to a multiple of 4; 2-byte aligned (int16 entries).
 *   Two launches (the loss's row pass, then one workgroup per utterance), no host synchronisation, no float atomics: the same inputs give the
 *   same bits on every run, and padded and packed give the same bits on the same nodes.  U1 <= 1024, T <= 8192 (cfm_last_error otherwise). */
typedef struct {
    cfm_rnnt_desc r;
    int32_t* frame;
    float* token_logp;
    float* score;
    void* scratch;
    int64_t scratch_bytes;
} cfm_rnnt_align_desc;
typedef struct {
    cfm_rnnt_packed_desc r;
    int32_t* frame;
    float* token_logp;
    float* score;
    void* scratch;
    int64_t scratch_bytes;
} cfm_rnnt_packed_align_desc;
int64_t cfm_rnnt_align_scratch_bytes(int64_t nodes);
int cfm_rnnt_align(const cfm_rnnt_align_desc* d, cfm_stream_t stream);
int cfm_rnnt_packed_align(const cfm_rnnt_packed_align_desc* d, cfm_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Training (BASELINE config 3: encoder + CTC loss + backward).  Input gradients of the dense layers are cfm_gemm on transposed
 * weight packs (with the CFM_ACT_DSILU / CFM_ACT_DRELU epilogues), weight / bias gradients are cfm_gemm_tn; the rest is below.
 * Every reduction over rows is two-stage through a caller-provided f32 workspace (size from the matching *_ws function, in floats)
 * and bitwise reproducible.
 *
 * cfm_layernorm_bwd_fused: backward of nn.LayerNorm at encoder_layer.py:57,60,64,68,70 and encoder.py:74.   D % 4 == 0, D <= 1024.
 *   x f32 [M,D] (the norm's INPUT; statistics are recomputed), dy [M,D] (dy_dtype), gamma [D];
 *   dx = (dres ? dres : 0) + dLN(dy)   (dx may alias dres: the residual stream's gradient is updated in place);
 *   rows with row_mask == 0 have dy = 0 (the masked norm_conv of convolution.py:36-37);  dgamma, dbeta f32 [D].
 * Every other field of the descriptor is optional and zero in the plain backward; they fold in what a conformer block's backward does right
 * before and after it:
 *   accumulate != 0 : dgamma / dbeta are ADDED to with f32 atomics in the same launch (no workspace pass, ws may be NULL; the caller zero-fills
 *                     them or carries a running sum; summation order varies from run to run) -- 0: two-stage through ws
 *                     (cfm_layernorm_bwd_ws(M, D) floats), overwritten, reproducible;
 *   dx2 != NULL     : also writes dropout(alpha2 * dx) in dx2_dtype -- the next residual branch's gradient as a GEMM operand, exactly
 *                     cfm_dropout_rows(dx, .., alpha2, p1, seed1, p2, seed2) without its launch.  With p1 > 0 or p2 > 0 the dropout counter
 *                     limits the call to M * D < 2^32 elements.
 */
int64_t cfm_layernorm_bwd_ws(int64_t M, int32_t D);
typedef struct {
    const float* x;
    const void* dy;
    const float* gamma;
    const uint8_t* row_mask;
    const float* dres;
    float *dx, *dgamma, *dbeta, *ws;
    void* dx2;
    int64_t M;
    int32_t D, dy_dtype, dx2_dtype, accumulate;
    float eps, alpha2, p1, p2;
    uint32_t seed1, seed2;
    const uint8_t* dx2_row_mask; /* optional: rows of dx2 with mask == 0 are written as zeros (cfm_dropout_rows' row_mask) */
    /* optional CHAINED second norm (needs accumulate = 1): dx = dLN( dres + dLN(dy; x, gamma) ; chain_x, chain_gamma ) -- the backward of two
     * LayerNorms applied one after the other to the same rows (block l's norm_final feeding block l+1's norm_ff_macaron, encoder_layer.py:70,57)
     * in one launch; the intermediate gradient is never stored, dx / dx2 come from the second stage, chain_dgamma / chain_dbeta get its sums. */
    const float *chain_x, *chain_gamma;
    float *chain_dgamma, *chain_dbeta;
} cfm_ln_bwd_desc;
int cfm_layernorm_bwd_fused(const cfm_ln_bwd_desc* d, cfm_stream_t stream);

/* GLU backward (convolution.py:42) on the column-interleaved layout the pointwise-conv-1 GEMM writes through cfm_gemm_desc.C_pre:
 * u [M,2D] (blocks of 16 value columns followed by their 16 gate columns), dg [M,D] -> du [M,2D] same layout.  D % 16 == 0. */
int cfm_glu_bwd(const void* u, int32_t u_dtype, const void* dg, int32_t dg_dtype, void* du, int32_t du_dtype, int64_t M, int32_t D,
                cfm_stream_t stream);

/* One micro-batch of an accumulation window (train.sh:36 accum_grad; src/executor.py:151): B utterances of T frames whose rows start at row0
 * of the window's row matrices.  Groups are contiguous: row0 of group i+1 = row0 of group i + B*T. */
#define CFM_TRAIN_MAX_GROUPS 8
typedef struct {
    int32_t B, T;
    int64_t row0;
    const uint8_t* attn_mask; /* this micro-batch's attention mask, strides as cfm_layer_train_io.am_sb / am_sq */
    int64_t am_sb, am_sq;
} cfm_train_group;

/* Depthwise conv (15 taps) -> BatchNorm1d in TRAINING mode -> SiLU  (convolution.py:43-45 under module.train()), over the micro-batches of a
 * training window (cfm_train_group; csrc/train_layer.cpp; a single batch is a window of one group with row0 = 0).  g / c_out / s_out are the window's
 * [M, D] row matrices, M = the sum of B*T over the groups; every stage is ONE launch for all groups, each group with its own batch statistics:
 *   c = dw(g) + bias            -> c_out f32 [M,D]  (kept for the backward); the taps see zeros before frame 0 and after frame T-1 of each utterance
 *   batch mean / biased variance of each channel over ALL B*T rows of the group, padded frames included
 *   stats f32 [n_groups][4][D] = mean, rstd, scale = gamma*rstd, shift = beta - mean*scale;   s_out = SiLU(c*scale + shift)  (s_dtype)
 *   running_mean / running_var (optional, both or neither) are updated in place with `momentum` and the UNBIASED variance, as torch does, group
 *   after group in the order of the table.
 * cfm_dwconv_bn_train_bwd_groups: ds [M,D] = d loss / d s_out, with c and stats as the forward left them -> dg_out [M,D] = d loss / d g, and the
 * gradients of the taps dw_w [D,15], the conv bias dw_b [D], the BatchNorm gain / bias dgamma, dbeta [D], each summed over the groups.
 *   accumulate != 0: the four parameter gradients are added to what the buffers hold (one writer per element: reproducible) instead of
 *   overwritten -- a gradient buffer shared by the micro-batches of an optimizer step.
 *   glu_u / glu_du (both or neither; dtype = g_dtype = dg_dtype): the GLU backward of convolution.py:42 in the depthwise launch -- u [M,2D] the
 *   pre-GLU columns (cfm_gemm_desc.C_pre layout), du [M,2D] their gradient; dg_out is then not written (may be NULL).  Same values as
 *   cfm_glu_bwd on the rounded dg.
 * dy_ws: f32 [M,D] scratch.  ws (both directions): the sum of cfm_dwconv_bn_ws(B,T,D) floats over the groups.  D % 4 == 0, D <= 512. */
int64_t cfm_dwconv_bn_ws(int32_t B, int32_t T, int32_t D);
int cfm_dwconv_bn_train_groups(const void* g, int32_t g_dtype, const float* w, const float* dw_bias, const float* gamma, const float* beta,
                               float* running_mean, float* running_var, float momentum, float eps, float* c_out, float* stats, void* s_out,
                               int32_t s_dtype, float* ws, const cfm_train_group* groups, int32_t n_groups, int32_t D, int32_t ktaps, cfm_stream_t stream);
int cfm_dwconv_bn_train_bwd_groups(const void* ds, int32_t ds_dtype, const float* c, const float* stats, const void* g, int32_t g_dtype, const float* w,
                                   void* dg_out, int32_t dg_dtype, float* dw_w, float* dw_b, float* dgamma, float* dbeta, float* dy_ws, float* ws,
                                   const cfm_train_group* groups, int32_t n_groups, int32_t D, int32_t ktaps, int32_t accumulate, const void* glu_u,
                                   void* glu_du, cfm_stream_t stream);

/* Front-end backward (convolution.py:60-63).  cfm_col2im_relu_bwd: dcol [B*T2*F2, 9*C] = dh2 . W2 (cfm_gemm on the transposed conv2 pack,
 * K order (kt,kf,c)) -> dh1 [B,T1,F1,C] = ReLU'(h1) * (transposed im2col of dcol).  cfm_conv1_wgrad: dh1 and the fbank input x [B,T,F]
 * (global CMVN folded as in cfm_conv1_relu) -> dw [9,C] tap-major, db [C]. */
int cfm_col2im_relu_bwd(const void* dcol, int32_t dcol_dtype, const void* h1, int32_t h1_dtype, void* dh1, int32_t dh1_dtype, int32_t B, int32_t T1,
                        int32_t F1, int32_t C, cfm_stream_t stream);
int64_t cfm_conv1_wgrad_ws(int32_t B, int32_t T, int32_t C);
int cfm_conv1_wgrad(const void* dh1, int32_t dh1_dtype, const float* x, const float* cmvn_mean, const float* cmvn_istd, float* dw, float* db, float* ws,
                    int32_t B, int32_t T, int32_t F, int32_t C, cfm_stream_t stream);

/* Attention backward (csrc/attention_bwd.hip; attention.py:81-96 under autograd).  cfm_attention with `lse` set also writes the row
 * log-sum-exp of the scaled, masked scores, lse f32 [B,H,Tq] (-inf for a fully masked row).  Given dout [B,Tq,H*dk] the backward
 * recomputes the probabilities tile by tile (nothing of size Tq x Tk reaches memory) and writes grad_q/k/v with the strides of q, k, v.
 * Batch path only (p broadcast over keys or absent: the positional term is then constant along a softmax row and has no gradient;
 * d pos_bias_u = the column sums of dq).  Fully masked rows contribute nothing (the reference's masked_fill(0) makes them constant). */
typedef struct {
    const void *q, *k, *v;          /* element (b,t,h,d) at base + b*sb + t*st + h*dk + d; q already includes pos_bias_u (train mode adds it
                                       through the projection's bias) */
    const uint8_t* mask;
    const void* out;                /* forward output [B,Tq,H*dk] */
    const void* dout;               /* [B,Tq,H*dk] */
    const float* lse;               /* [B,H,Tq] */
    void *grad_q, *grad_k, *grad_v; /* same strides as q, k, v */
    float* delta;                   /* f32 scratch [B,H,Tq] */
    int64_t q_sb, q_st, k_sb, k_st, v_sb, v_st, m_sb, m_sq;
    int32_t B, H, Tq, Tk, dk;
    int32_t io_dtype;               /* dtype of q,k,v,out,dq,dk,dv (16-bit or f32) */
    int32_t dout_dtype;
    int32_t mma_dtype, split;
    float scale;
    float drop_p;                   /* the forward's probability dropout (same p, same seed) */
    uint32_t drop_seed;
} cfm_attn_bwd_desc;
int cfm_attention_bwd(const cfm_attn_bwd_desc* d, cfm_stream_t stream);
/* n backward problems in three launches (delta, dq, dkv over all of them) when every one takes the d_k = 64 / 16-bit kernels; else one by one. */
int cfm_attention_bwd_group(const cfm_attn_bwd_desc* descs, int32_t n, cfm_stream_t stream);
/* d_k = 64 with 16-bit, 16-byte-aligned q / k / v / dO rows takes fast kernels, under any mask kind: none, a key-validity mask (m_sq == 0) or a
 * (B,Tq,Tk) mask (m_sq != 0, the MFULL instances); they are profiled as attn_bwd_{delta,dq,dkv}_fast* (tiles staged as they lie in memory,
 * transposed operands read with ds_read_b64_tr_b16, next tile prefetched) -- bit-identical to the general ones, which this switch forces (tests). */
void cfm_attention_bwd_force_general(int32_t on);
/* Chained blocks (cfm_layer_io.next_w): run the conv-in chain as the input stage of the block's last launch (two launches per block; the default, also
 * switched off by CFM_CIN_MERGE=0 in the environment at first use) or as a launch of its own (three).  The results are bit-identical; bench.py times the
 * narrower launch beside the merged one with it.  Returns the previous setting. */
int32_t cfm_set_cin_merge(int32_t on);

/* Feed-forward for FEW rows, the hidden dimension split across workgroups (csrc/ffnsplit.hip; feedforward.py:17-20 inside encoder_layer.py:55-58,
 * 67-70 when B*T' is a few hundred rows: a streaming step, BASELINE config 5).  One launch = the row-reduce input stage + (by mode) nothing, a
 * projection, or a feed-forward that leaves PARTIAL sums:
 *   rows      x = psum ? x + psum_alpha * (sum_{g < psum_splits} psum[g] + psum_b2) : x;   if ln1: x = LN1(x);   rows_out = x (optional)
 *   mode 0    rows2_out = LN2(x) (optional)
 *   mode 1    out16[:, n] = act(LN(x) . w1[n,:] + b1[n]),  n < N1                       grid = (ceil(M/32), N1/256)
 *   mode 2    psum_out[g] = act(LN(x) . w1[256 g .. 256 g + 255,:]^T + b1) . w2[:, 256 g ..]^T,  g < N1/256 (N1 = FF), to be reduced -- with b2, alpha,
 *             the residual and the next norm(s) -- by the rows stage of the next cfm_ffn_split call (fixed order g = 0,1,..: reproducible)
 * w1: fragment-major [N1/16][D/32][64][8] (packing.pack_frag_major / pack_ffn_fragments' w1f), w2: fragment-major [D/16][FF/32][64][8] (w2n);
 * 16-bit `w_dtype`; f32 rows [M,D]; psum / psum_out f32 [splits][M][D]; rows_out may alias x only when one slice runs (mode 0, or N1 == 256).  D = 256. */
typedef struct {
    const float* x;
    const float* psum;
    const float* psum_b2;
    int32_t psum_splits;
    float psum_alpha;
    const float *ln1_g, *ln1_b, *ln2_g, *ln2_b;
    float *rows_out, *rows2_out;
    const float *ln_g, *ln_b;
    const void* w1;
    const float* b1;
    int32_t N1, act;
    const void* w2;
    float* psum_out;
    void* out16;
    int64_t ldo;
    int32_t M, D, mode, w_dtype;
    float eps;
    /* mode 1 as the fused q|k|v projection of a batched streaming step (N1 = 3 D): when kv_ring is given, the key and value columns are ALSO written,
     * as the 16-bit values widened to f32, into the per-stream ring f32 [B, ring_H, ring_T, 2 dk] at slot (ring_offsets[b] + t) mod ring_T, row
     * m = b * ring_Tq + t -- what cfm_kv_ring_write would copy from out16, without its launch */
    float* kv_ring;
    const int32_t* ring_offsets;
    int32_t ring_T, ring_H, ring_Tq;
    /* optional int32 [B] with kv_ring: only rows t < ring_len[b] of stream b are frames of the stream and go into the ring; later rows touch no slot.
     * out16 still receives every row.  NULL = all ring_Tq rows, as before */
    const int32_t* ring_len;
} cfm_ffn_split_desc;
int cfm_ffn_split(const cfm_ffn_split_desc* d, cfm_stream_t stream);
int cfm_ffn_split_supported(int32_t D, int32_t FF);

/* CTC backward (csrc/ctc.hip).  cfm_ctc_nll_train_groups is cfm_ctc_nll for the micro-batches of a training window that also keeps, per micro-batch,
 * log alpha (alpha f32 [B,T,2*Umax+2]), log(beta / y) (beta, same shape), the per-frame log-sum-exp (lse f32 [B,T]) and nll_shifted f32 [B] (-log P
 * of the per-frame-shifted recursion: the posteriors' normaliser): the per-frame row passes per micro-batch, then BOTH recursions of ALL micro-batches
 * in one launch (each is a serial chain on one CU; 2 * B workgroups per micro-batch).  A single batch is a window of one micro-batch.
 * cfm_ctc_grad takes one micro-batch's arrays and writes d loss / d logits [B,T,ld] = gscale[b] * (softmax - occupancy)
 * for t < enc_lens[b] and 0 elsewhere (pad columns V..ld-1 too) -- what autograd gives for nn.CTCLoss(reduction='sum') on
 * log_softmax(logits) (decoder.py:20-21).  The scale is gscale * (gscale_dev ? *gscale_dev : 1): a host factor (1 / padded label length,
 * decoder.py:22) times an optional DEVICE scalar (the upstream gradient).  alpha and beta are read only.
 * An utterance with no valid alignment (nll = inf) gets a zero gradient (torch's is undefined without zero_infinity).  V <= 8192. */
typedef struct {
    const float* logits;
    int64_t ld;
    int32_t B, T, Umax;
    const int32_t *enc_lens, *labels, *label_lens;
    float *work, *alpha, *lse, *nll, *nll_shifted, *beta;
} cfm_ctc_group;
int cfm_ctc_nll_train_groups(const cfm_ctc_group* groups, int32_t n, int32_t V, cfm_stream_t stream);
int cfm_ctc_grad(const float* logits, int64_t ld, int32_t B, int32_t T, int32_t V, const int32_t* enc_lens, const int32_t* labels, int32_t Umax,
                 const int32_t* label_lens, const float* work, const float* alpha, const float* beta, const float* lse, const float* nll_shifted,
                 float gscale, const float* gscale_dev, float* dlogits, cfm_stream_t stream);

/* Dropout as an elementwise pass:  y[m,n] = keep(seed, m*N + n) ? alpha * x[m,n] / (1-p) : 0, rows with row_mask == 0 zeroed.  The backward of
 * a residual branch x + alpha * dropout(f(..)) needs d f = alpha * mask/(1-p) * dx as a GEMM operand (encoder_layer.py:58,61,64,69); the
 * forward of the same dropout is fused into the producing GEMM's epilogue (cfm_gemm_desc.drop_p), this pass only regenerates its mask.
 * cfm_dropout_mask writes the 0/1 keep mask itself (tests). */
int cfm_dropout_rows(const void* x, int32_t x_dtype, void* y, int32_t y_dtype, const uint8_t* row_mask, float alpha, float p, uint32_t seed,
                     float p2, uint32_t seed2, int64_t M, int32_t N, cfm_stream_t stream);
int cfm_dropout_mask(uint8_t* out, int64_t n, float p, uint32_t seed, cfm_stream_t stream);

/* Weight packs of the training path, any number of matrices in one launch (csrc/train.hip cfm_pack_kernel).  jobs_dev: DEVICE array of
 * n_jobs x 8 int64 -- { rows, N, K, dst, dst_lo, dst_t, dst_t_lo, first_tile }: `rows` a device array of N pointers to f32 source rows of K
 * contiguous values (concatenated or permuted sources are just pointer tables: the fused q|k|v matrix, the GLU-interleaved pointwise
 * conv), dst [N,K] and dst_t [K,N] the 16-bit matrix and its transpose (either may be 0), *_lo the bf16 lo planes when split != 0,
 * first_tile the prefix sum of ceil(N/64) * ceil(K/64) over the preceding jobs; total_tiles the sum over all jobs.  N % 8 == 0, K % 8 == 0.
 * Replaces the per-step torch casts / transposes of cfm/packing.py (what the reference's optimizer step makes necessary: the kernels
 * read 16-bit copies of the f32 master weights). */
int cfm_pack_matrices(const int64_t* jobs_dev, int32_t n_jobs, int64_t total_tiles, int32_t w_dtype, int32_t split, cfm_stream_t stream);
/* out[i] = *a[i] + (b[i] ? *b[i] : 0), i < n: the small f32 vectors of the training packs of a whole block stack in one launch (the fused
 * q|k|v bias with pos_bias_u added to its first third, attention.py:62-64,81; the GLU-interleaved pointwise-conv-1 bias, convolution.py:41-42)
 * as gathers through two device tables of element pointers. */
int cfm_pack_vectors(const float* const* a, const float* const* b, float* out, int64_t n, cfm_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * The conformer blocks in TRAIN mode (csrc/train_layer.cpp): encoder_layer.py:49-71 under module.train() and its
 * backward, the same launches in the same order as the op-by-op composition of cfm/autograd.py's sub-block helpers (tests/train_block_ref.py).
 * A block may lack the conv module's biases or the BatchNorm affine: the kernels write those gradients all the same, so the caller points
 * them at a discard buffer, never at null.  All buffers are the caller's:
 *   weights  the train packs (forward [N,K] and transposed [K,N] 16-bit matrices, + lo planes in the f32-accurate mode; cfm/packing.py)
 *   saved    activations the backward needs, act dtype unless typed: xn1..4 [M,D], z1,z2,h1,h2 [M,FF], qkv [M,3D], ctx [M,D], u [M,2D], glu/s [M,D],
 *            f32 x1..x4 / c [M,D], lse [B,H,T], stats [4,D]
 *   scratch  backward work buffers (dxn f32 [M,D], dz [M,FF], dyb/ds/dglu/dctx [M,D], du [M,2D], dqkv [M,3D], delta f32 [B,H,T],
 *            ln_ws cfm_layernorm_bwd_ws floats, dwbn_ws cfm_dwconv_bn_ws floats, dy_ws f32 [M,D]; dz2 / dyb2..4 with io->defer_wgrad);
 *            the forward uses dwbn_ws only
 *   grads    where each parameter's gradient goes: plain pointers, and for the two fused products (q|k|v, the interleaved pointwise-conv-1
 *            pack) per-row element offsets relative to `slab` (cfm_gemm_tn_desc.row_off).  Weight / bias gradients are ACCUMULATED: the
 *            caller zero-fills; LayerNorm / BatchNorm / depthwise gradients are overwritten.  pos_bias_u receives a copy of q_bias' gradient.
 * Dropout: probabilities per site and one seed (site s uses seed + 0x9E3779B1*s); 0 disables.  deterministic = 1: weight-gradient products
 * run unsplit (no atomics).  Returns like every entry point; nothing is synchronised. */
typedef struct {
    const float *ln_ffm_g, *ln_ffm_b, *ln_mha_g, *ln_mha_b, *ln_conv_g, *ln_conv_b, *ln_ff_g, *ln_ff_b, *ln_final_g, *ln_final_b;
    const void *ffm_w1, *ffm_w1_lo, *ffm_w2, *ffm_w2_lo, *ffm_w1t, *ffm_w1t_lo, *ffm_w2t, *ffm_w2t_lo;
    const float *ffm_b1, *ffm_b2;
    const void *ff_w1, *ff_w1_lo, *ff_w2, *ff_w2_lo, *ff_w1t, *ff_w1t_lo, *ff_w2t, *ff_w2t_lo;
    const float *ff_b1, *ff_b2;
    const void *qkv_w, *qkv_w_lo, *qkv_t, *qkv_t_lo, *out_w, *out_w_lo, *out_t, *out_t_lo;
    const float *qkv_b, *out_b;
    const void *pw1_w, *pw1_w_lo, *pw1_t, *pw1_t_lo, *pw2_w, *pw2_w_lo, *pw2_t, *pw2_t_lo;
    const float *pw1_b, *pw2_b, *dw_w, *dw_b, *bn_gamma, *bn_beta;
    float *bn_running_mean, *bn_running_var;
    float bn_momentum, bn_eps;
} cfm_layer_train_weights;


typedef struct {
    int32_t D, H, FF, ktaps, act_dtype, w_dtype;
    const uint8_t* pad_valid;
    float p_hidden_m, p_hidden, p_branch, p_attn, p_attn_out;
    uint32_t seed;
    int32_t deterministic;
    /* backward only: the gradient slab is a running sum (the optimizer step's flat gradient buffer itself) -- every parameter gradient is ADDED
     * to it and nothing in it is overwritten.  Needs deterministic == 0 (the LayerNorm sums are added with atomics). */
    int32_t grads_accumulate;
    /* ROW GROUPS (n_groups >= 1; one group: a single micro-batch).  The micro-batches of an accumulation window concatenated along the row
     * axis: every row matrix has M = sum B_g*T_g rows, pad_valid has M entries, lse / delta are the groups' [B_g,H,T_g] arrays one after the other, stats is [n_groups][4*D].  Row-local work (dense products, LayerNorm, their backward, the
     * weight gradients) runs once over all rows; attention, the depthwise convolution and BatchNorm run per group, BatchNorm's running
     * statistics updated group after group -- the reference's sequence of forward passes over those micro-batches.  host array. */
    int32_t n_groups;
    const cfm_train_group* groups;
    /* backward: keep the operands of the block's eight weight-gradient products until its last launch and issue them as ONE
     * cfm_gemm_tn_group (needs the dz2 / dyb2..4 scratch buffers and, for pos_bias_u, grads.qkv_bias_off2; 16-bit modes -- ignored in the
     * f32-accurate mode). */
    int32_t defer_wgrad;
} cfm_layer_train_io;

typedef struct {
    void *xn1, *z1, *h1, *xn2, *qkv, *ctx, *xn3, *u, *glu, *s, *xn4, *z2, *h2;
    float *x1, *x2, *x3, *x4, *c, *lse, *stats;
} cfm_layer_train_saved;

typedef struct {
    float* dxn;
    void *dz, *dyb, *ds, *dglu, *du, *dctx, *dqkv;
    float *delta, *ln_ws, *dwbn_ws, *dy_ws;
    void *dz2, *dyb2, *dyb3, *dyb4; /* with io->defer_wgrad: the operands of the deferred weight-gradient products must outlive the sub-block that
                                       made them: second feed-forward's dz, one branch-gradient buffer per sub-block (act dtype, [M,FF] / [M,D]) */
} cfm_layer_train_scratch;

typedef struct {
    float* slab;
    float *ln_ffm_g, *ln_ffm_b, *ln_mha_g, *ln_mha_b, *ln_conv_g, *ln_conv_b, *ln_ff_g, *ln_ff_b, *ln_final_g, *ln_final_b;
    float *ffm_w1, *ffm_b1, *ffm_w2, *ffm_b2, *ff_w1, *ff_b1, *ff_w2, *ff_b2;
    float *out_w, *out_b, *pw2_w, *pw2_b, *dw_w, *dw_b, *bn_g, *bn_b;
    float* pos_bias_u;
    const float* q_bias;
    const int64_t *qkv_row_off, *qkv_bias_off, *pw1_row_off, *pw1_bias_off;
    const int64_t* qkv_bias_off2; /* optional: int64 [3D], entry n < D = offset of pos_bias_u[n] relative to slab, others -1 (cfm_gemm_tn_desc.colsum_off2) */
} cfm_layer_train_grads;

/* The whole block stack in train mode (src/encoder.py:72-73 `for block in self.encoders` under module.train()) from ONE host call each way.
 *   w, sv, g  arrays of n_layers structs; io, t shared by all blocks (layer l's dropout seed is derived from io->seed and l)
 *   xs        n_layers + 1 f32 [M,D] row matrices: xs[0] the stack's input, xs[l+1] block l's output (kept: block l+1's backward reads xs[l+1])
 * backward: dy = gradient of xs[n_layers]; dbuf0 / dbuf1 two f32 [M,D] work buffers, *dx_out is set to the one holding the gradient of xs[0].
 * `done(l, user)` (optional) is called on the host right after block l's backward launches have been enqueued, last block first -- the
 * data-parallel trainer starts that block's gradient bucket all-reduce from it (DDP's reducer hook, executor.py:137-154).
 * With deterministic == 0 block l's last LayerNorm backward (norm_ff_macaron) runs chained in block l-1's first launch, and `done(l)` follows
 * that launch.  One block with one row group is the plain single-block training pass. */
typedef void (*cfm_layer_done_fn)(int32_t layer, void* user);
int cfm_encoder_train_forward(int32_t n_layers, const cfm_layer_train_weights* w, const cfm_layer_train_io* io, const cfm_layer_train_saved* sv,
                              const cfm_layer_train_scratch* t, float* const* xs, cfm_stream_t stream);
int cfm_encoder_train_backward(int32_t n_layers, const cfm_layer_train_weights* w, const cfm_layer_train_io* io, const cfm_layer_train_saved* sv,
                               const cfm_layer_train_scratch* t, const cfm_layer_train_grads* g, float* const* xs, const float* dy,
                               float* dbuf0, float* dbuf1, cfm_layer_done_fn done, void* user, float** dx_out, cfm_stream_t stream);

/* Optimizer step over flat f32 buffers (module.py:140-143 Adam; executor.py:150 gradient_clip_val):  g' = g * (*grad_scale) + wd * p;
 * m = b1 m + (1-b1) g';  v = b2 v + (1-b2) g'^2;  p -= lr/(1-b1^step) * m / (sqrt(v)/sqrt(1-b2^step) + eps)   (torch.optim.Adam).
 * grad_scale: optional DEVICE scalar (the clip coefficient), so nothing synchronises between backward and step.
 * cfm_sumsq: out[0] = sum x^2 (two-stage, n_partials <= 4096 workgroups). */
int cfm_adam_step(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1, float beta2, float eps, float weight_decay,
                  int64_t step, const float* grad_scale, cfm_stream_t stream);
int cfm_sumsq(const float* x, int64_t n, float* partials, int32_t n_partials, float* out, cfm_stream_t stream);
/* cfm_adam_step with the step's scalar glue inside (executor.py:150 gradient_clip_val + Lightning DDP's gradient averaging): the gradient
 * scale is min(1, clip / (sqrt(*sumsq) * inv_world + 1e-6)) * inv_world (clip <= 0: inv_world), computed on the device from cfm_sumsq's result;
 * *norm_out (optional) receives the averaged gradient's norm when sumsq is given (sumsq NULL, allowed with clip <= 0: it is not written);
 * zero_grad != 0 zeroes g as it is read (the next step's accumulation buffer).  A NaN *sumsq under clip > 0 gives a NaN scale, so p, m, v
 * all become NaN (torch's clip_grad_norm_ + Adam); an infinite one gives the scale 0. */
int cfm_adam_clip_step(float* p, float* g, float* m, float* v, int64_t n, float lr, float beta1, float beta2, float eps, float weight_decay,
                       int64_t step, const float* sumsq, float clip, float inv_world, int32_t zero_grad, float* norm_out, cfm_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Profiling table (aux subsystem: tracing).  When enabled, every kernel launch made through this
 * library carries a start and a stop HIP event attached to the dispatch itself (its own begin/end timestamps, the
 * duration a profiler reports); cfm_prof_collect() synchronises those events and accumulates per-kernel-name
 * totals.  Used by bench.py for the live roofline figure.
 */
void cfm_prof_enable(int on);
void cfm_prof_reset(void);
int cfm_prof_collect(void);                 /* returns number of distinct kernel names */
int cfm_prof_entry(int i, char* name, int name_cap, int64_t* calls, double* total_ms, double* flops,
                   double* bytes);

/* ------------------------------------------------------------------------------------------------
 * One step of the batched RNN-T greedy search (reference src/model.py:215-269: predictor step predictor.py:76-86, joint joint.py:20-38,
 * argmax and the loop's bookkeeping) for B <= 64 streams, six launches, everything float32 (csrc/greedy.hip).  All state lives in caller
 * buffers and is updated in place; calling it repeatedly (or replaying a captured graph of calls) runs the search, n_done counts the
 * streams that have reached their last frame.  Weights are f32 row-major [out, in]:
 *   embed [vocab, E];  lstm_w[l] [4H, in_l + H] = [W_ih | W_hh] with ROWS ORDERED [unit][gate i,f,g,o] (not torch's [gate][unit]),
 *   lstm_b[l] [4H] = b_ih + b_hh in the same order;  proj_w [P, H], pf_w [J, P] (pred_ffn), out_w [Vp, J] (ffn_out, rows >= V zero,
 *   out_b there -inf);  enc_proj [B, T, J] = enc_ffn(encoder output).
 *   state: token / t / count / frame_count / lens int64 [B], hyps int64 [B, hyp_ld] (at most hyp_cap + 1 entries used), h / c and the
 *   candidates h_new / c_new f32 [L, B, H], done uint8 [B];  scratch: pred [B, P], act [B, J], pmax / pidx [Vp/16, B]. */
typedef struct {
    const float* embed;
    const float* lstm_w[4];
    const float* lstm_b[4];
    const float *proj_w, *proj_b, *pf_w, *pf_b, *out_w, *out_b;
    const float* enc_proj;
    int64_t *token, *t, *count, *frame_count, *hyps;
    const int64_t* lens;
    float *h, *c, *h_new, *c_new, *pred, *act, *pmax;
    int32_t* pidx;
    uint8_t* done;
    int32_t* n_done;
    int64_t hyp_cap, hyp_ld;
    int32_t B, T, L, E, H, P, J, Vp, blank, n_steps;
} cfm_greedy_desc;
int cfm_greedy_step(const cfm_greedy_desc* d, cfm_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Chunk-lookahead greedy search: the decoder of a batched streaming recogniser (reference src/model.py:178-199 / :126-165 around
 * basic_greedy_search), B <= 64 streams, chunk <= 32 encoder frames per stream and call, everything float32 (csrc/greedy.hip).
 * The state is cfm_greedy_desc's with two differences: t is the frame index INSIDE the current chunk, lens[b] in [0, chunk] the number
 * of the chunk's frames that belong to stream b (0: idle, nothing about the stream changes).
 *   cfm_greedy_chunk_begin  enc_proj = enc_ffn(enc) for the chunk's B * chunk rows (ef_w [J, D], ef_b [J]); t, frame_count <- 0,
 *                           done / n_done from lens, steps <- 0; carry == 0: token <- blank, h, c <- 0 on the streams with frames.
 *   cfm_greedy_chunk_step   one lookahead step: the predictor on (token, h, c), the joint for the frames t_b .. lens_b - 1 of every
 *                           unfinished stream, the first frame whose argmax is not blank emits (none: the stream is done with the
 *                           chunk).  At most 1 + (most emissions of any stream) steps finish a chunk; n_done == B says so.
 * Weights as in cfm_greedy_desc.  Scratch: pred [B, P], pp [B, J], act [B * chunk, J] and rows [B * chunk] (compact: only the rows
 * evaluated this step, row_off / row_cnt [B] per stream, n_rows [1] in all; rows[i] = b * chunk + frame), pmax / pidx [B * chunk, Vp/16]
 * per compact row.  steps [1] counts the steps that began with a live stream, overflow [1] is set when a stream had more than hyp_cap
 * symbols to store (the symbol is counted, not stored).  hyps accumulates across chunks: count is not reset by begin. */
typedef struct {
    const float* embed;
    const float* lstm_w[4];
    const float* lstm_b[4];
    const float *proj_w, *proj_b, *pf_w, *pf_b, *out_w, *out_b, *ef_w, *ef_b;
    const float* enc;            /* [B, chunk, D] encoder output (begin only) */
    float* enc_proj;             /* [B, chunk, J] */
    int64_t *token, *t, *count, *frame_count, *hyps;
    const int64_t* lens;
    float *h, *c, *h_new, *c_new, *pred, *pp, *act, *pmax;
    int32_t *pidx, *rows, *row_off, *row_cnt, *n_rows, *steps, *overflow;
    uint8_t* done;
    int32_t* n_done;
    int64_t hyp_cap, hyp_ld;
    int32_t B, chunk, L, E, H, P, J, D, Vp, blank, n_steps, carry;
} cfm_greedy_chunk_desc;
int cfm_greedy_chunk_begin(const cfm_greedy_chunk_desc* d, cfm_stream_t stream);
int cfm_greedy_chunk_step(const cfm_greedy_chunk_desc* d, cfm_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Kaldi-compatible log-mel filter bank, waveform in, feature rows out, one launch (csrc/fbank.hip): the reference's
 * kaldi.fbank(waveform * (1 << 15), num_mel_bins, frame_length, frame_shift, dither, energy_floor=0, sample_frequency) of
 * src/processor.py:175-193 (compute_fbank) and src/deploy.py:106-146 (preprocess, preprocess_stream) with torchaudio's defaults for the rest.
 * Row r of item b is frame pos + r of its signal: samples [shift r, shift r + win) of the item's sample sequence, minus their mean,
 * pre-emphasised (0.97), times `window`, zero-padded to `padded` (a power of two, 8 .. 512), |rfft|^2, the sparse mel product, log(max(., f32 eps)).
 *   samples   [B, ld] int16 (samples_i16 != 0) or f32, on the int16 scale
 *   twiddle   f64 [padded, 2] = (cos, -sin)(2 pi k / padded);  window f64 [win]  (host tables, float64: the kernel calls no sin / cos for them)
 *   mel_w     f32 [mel_nnz <= 512] packed weights;  mel bin b = sum_i power[mel_start[b] + i] * mel_w[mel_off[b] + i], i < mel_len[b]
 *   out       f32 [B, rows, F]
 *   dither    > 0 adds dither * n(seed, b, pos + r, j), standard normal from cfm_hash32 through Box-Muller: a frame's noise depends on its
 *             ABSOLUTE index, not on how the audio was cut into calls
 * cfm_fbank (offline, deploy.py preprocess): the sequence of item b is samples[b, 0 .. lengths[b]) (clamped to n_cols), pos = 0; rows at or beyond its frame
 *   count 1 + (n - win) / shift (0 when n < win) are written as zeros (the reference's padding() pads features with 0), feats_length [B] receives the count.
 * cfm_fbank_stream (deploy.py preprocess_stream, for B streams): every row is computed.  A stream with fresh_in[b] != 0 reads its `n_first` = (rows - 1) shift + win
 *   samples from samples[b] and has pos = 0; any other stream reads carry_in[b, 0 .. carry_n) followed by `n_next` = n_first - carry_n samples of samples[b],
 *   and pos = pos_in[b].  carry_out[b] <- the last carry_n samples of that sequence, fresh_out[b] <- 0, pos_out[b] <- pos + hop.  The *_in and *_out
 *   buffers must not alias (the caller swaps them between calls).  n_cols >= n_next; the caller, who knows which streams it reset, passes n_first
 *   columns when one is fresh (a read at or past n_cols yields 0, never memory beyond the row).
 * cfm_fbank_stream with n_new != null (audio packets of any size; the fields behind `seed`, which the other two modes leave null / 0 and never read):
 *   the carry is f32 [B, carry_cap] of which carry_len_in[b] samples count (0 for a fresh stream), the sequence of stream b is those followed by
 *   samples[b, 0 .. n_new[b]) (clamped to n_cols; a read at or past n_new[b] yields 0), L samples in all, and with n_first as above:
 *     L >= n_first                 a whole window: m = rows, the sequence loses hop * shift samples at its head, pos + hop
 *     L <  n_first, final[b] != 0  the utterance's short last window: m = 1 + (L - win) / shift (0 when L < win) rows, rows >= m written as zeros;
 *                                  c = ((m - 1) / 2 - 1) / 2 (0 for m < 7, cfm_stream_prep's encoder-frame count), 4 c shift samples lost, pos + 4 c
 *     L <  n_first otherwise       buffering: m = 0, nothing lost, every row zero
 *   carry_out[b] <- what is left of the sequence (at most carry_cap samples: the caller admits L <= n_first + hop * shift - 1, so that n_first - 1
 *   remain at the most; carry_cap >= n_first - 1), carry_len_out[b] <- its length, pos_out, fresh_out <- 0, frame_lens[b] <- m: the device buffer of
 *   window lengths that the length-aware encoder step reads.  carry_n is not read; n_cols may be 0 (samples may then be null). */
typedef struct {
    const void* samples;
    const int32_t* lengths;      /* offline */
    int32_t* feats_length;       /* offline, may be null */
    const float* carry_in;       /* streaming: f32 [B, carry_n] */
    float* carry_out;
    const int32_t *fresh_in, *pos_in;
    int32_t *fresh_out, *pos_out;
    const double* twiddle;
    const double* window;
    const float* mel_w;
    const int32_t *mel_start, *mel_len, *mel_off;
    float* out;
    int64_t ld;
    int32_t B, n_cols, rows, F, win, shift, padded, mel_nnz, samples_i16, carry_n, hop;
    float dither;
    uint32_t seed;
    const int32_t *n_new, *final;    /* ragged packets (cfm_fbank_stream with n_new != null): int32 [B] each */
    const int32_t* carry_len_in;     /* int32 [B] */
    int32_t *carry_len_out, *frame_lens;
    int32_t carry_cap;               /* the carry buffers are f32 [B, carry_cap] */
} cfm_fbank_desc;
int cfm_fbank(const cfm_fbank_desc* d, cfm_stream_t stream);
int cfm_fbank_stream(const cfm_fbank_desc* d, cfm_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * LSTM over whole sequences, forward and backward (csrc/lstm.hip): torch.nn.LSTM(batch_first=True) of the RNN-T predictor's teacher-forced
 * pass (reference src/predictor.py:66-67) -- gate order i, f, g, o, weight_ih_l{k} [4H, in_k], weight_hh_l{k} [4H, H], bias_* [4H] (NULL: no
 * bias), in_0 = in, in_k = H.  Everything is f32; every product runs on the f32 MFMA.
 *   x [B, U, in] dense, h0 / c0 [layers, B, H] (NULL: zeros)  ->  y [B, U, H], hn / cn [layers, B, H]
 *   save[k]   one block of cfm_lstm_save_floats(B, U, H) floats per layer, written by the forward, read by the backward (the layer's
 *             outputs and cells with the initial state in front, and the gates after their activations)
 *   dropout   between layers (not after the last): element e of layer k - 1's time-major [U*B, H] output is kept iff
 *             hash(seed + 0x9E3779B1 * k, e) >= drop_p * 2^32 and scaled by 1 / (1 - drop_p); the backward regenerates the mask from
 *             (drop_p, seed).  drop_p = 0: off (eval mode).
 *   backward  dy [B, U, H] dense, dhn / dcn [layers, B, H] (NULL: zeros)  ->  dx [B, U, in], dw_ih / dw_hh / db_ih / db_hh (overwritten; db_*
 *             may be NULL), dh0 / dc0 [layers, B, H];  work buffers dg [U*B, 4H] and, for layers > 1, dyl [U*B, H]
 * H and in: multiples of 64 up to 512; B >= 1, U >= 1, B*U*4H < 2^31; 1..CFM_LSTM_MAX_LAYERS layers; every pointer 16-byte aligned.
 * A workgroup owns 16 sequences for all U steps and never waits on another one.  All sums run in a fixed order: bitwise reproducible. */
#define CFM_LSTM_MAX_LAYERS 4
typedef struct {
    int32_t B, U, in, H, layers;
    float drop_p;
    uint32_t seed;
    const float* x;
    const float *w_ih[CFM_LSTM_MAX_LAYERS], *w_hh[CFM_LSTM_MAX_LAYERS], *b_ih[CFM_LSTM_MAX_LAYERS], *b_hh[CFM_LSTM_MAX_LAYERS];
    const float *h0, *c0;
    float *y, *hn, *cn;
    float* save[CFM_LSTM_MAX_LAYERS];
    /* backward only */
    const float *dy, *dhn, *dcn;
    float* dx;
    float *dw_ih[CFM_LSTM_MAX_LAYERS], *dw_hh[CFM_LSTM_MAX_LAYERS], *db_ih[CFM_LSTM_MAX_LAYERS], *db_hh[CFM_LSTM_MAX_LAYERS];
    float *dh0, *dc0;
    float *dg, *dyl;
} cfm_lstm_desc;
int64_t cfm_lstm_save_floats(int32_t B, int32_t U, int32_t H);
int cfm_lstm_forward(const cfm_lstm_desc* d, cfm_stream_t stream);
int cfm_lstm_backward(const cfm_lstm_desc* d, cfm_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * CTC decoding on top of the vocabulary projection (csrc/ctc_decode.hip).  logits f32 [B,T,ld>=V] as for cfm_ctc_nll (ld % 4 == 0, columns
 * V..ld never read); lens int32 [B]: the valid frames of each utterance / stream (clamped to [0, T]).  The reference has no CTC decoder;
 * the algorithms are the standard ones, restated in float64 in tests/ctc_decode_ref.py.
 *
 * cfm_ctc_topk: per valid frame lse = log sum_c exp(logits[c]) (max-shifted, f32) and the k largest log-probabilities logits[c] - lse with
 *   their classes, 1 <= k <= min(16, V), in descending order, the lower class first among equal values (torch.argmax's rule for k = 1,
 *   torch.sort(stable=True, descending=True) otherwise).  idx int32 [B*T, k], logp f32 [B*T, k], lse f32 [B*T]; the rows of frames at or
 *   beyond lens[b] are not touched. */
int cfm_ctc_topk(const float* logits, int64_t ld, int32_t B, int32_t T, int32_t V, const int32_t* lens, int32_t k, int32_t* idx, float* logp,
                 float* lse, cfm_stream_t stream);

/* cfm_ctc_greedy: best-path decoding -- the per-frame argmax, repeats collapsed, blanks dropped -- as a streaming step.  idx / logp: the
 *   first column of cfm_ctc_topk's output (row stride ld_k >= 1, so any k serves).  Frame t < lens[b] of stream b emits its class when it
 *   differs from the class of the frame before it and from blank; the frame before frame 0 is prev[b] (int32 [B], -1 at an utterance's start,
 *   left holding the last frame's class: a repeat across two calls collapses).  An emission is appended at hyps[b, count[b]] (int64
 *   [B, hyp_ld], count int64 [B]) together with frames[b, .] = frame_base[b] + t (int32; frame_base int32 [B] may be null: 0, else it is
 *   advanced by lens[b]) and token_logp[b, .] = the class's log-probability (f32), both of hyps' shape.  A stream that already holds hyp_cap
 *   symbols sets overflow[0] = 1; the symbol is counted, not stored.  lens[b] == 0 changes nothing for stream b.  blank in [0, V). */
typedef struct {
    const int32_t* idx;
    const float* logp;
    int64_t ld_k;
    const int32_t* lens;
    int32_t* prev;
    int32_t* frame_base;
    int64_t *hyps, *count;
    int32_t* frames;
    float* token_logp;
    int32_t* overflow;
    int64_t hyp_cap, hyp_ld;
    int32_t B, T, V, blank;
} cfm_ctc_greedy_desc;
int cfm_ctc_greedy(const cfm_ctc_greedy_desc* d, cfm_stream_t stream);

/* cfm_ctc_prefix_beam: CTC prefix beam search, 1 <= beam <= 16 prefixes kept.  idx / logp [B, T, k]: cfm_ctc_topk's output, 1 <= k <= min(16, V), of
 *   which a frame offers its first min(k, beam) classes (k = beam unless the vocabulary has fewer classes than the beam has places).  Every
 *   prefix of the beam carries pb / pnb, the f32 log-probabilities of its alignments that end in blank / in its last token (-inf:
 *   impossible); the empty prefix starts at (0, -inf).  A frame's class (c, p) adds logaddexp(pb, pnb) + p to pb of the prefix itself
 *   (c blank) or to pnb of the prefix extended by c, except that c equal to the prefix's last token adds pnb + p to the prefix's own pnb and
 *   only pb + p to the extension.  Candidates that are the same TOKEN STRING are merged (a prefix that left the beam and returned under a new
 *   trie node meets its surviving extension again): the kernel compares (length, last token, 64-bit incremental hash of the string), see
 *   csrc/ctc_decode.hip for the collision bound.  The `beam` best candidates by logaddexp(pb, pnb) are kept; a score of -inf is no candidate.
 *   The order is total: higher score; then the candidate that continues the better-ranked parent; then the prefix itself before its
 *   extensions; then the lower class (a merged candidate ranks with the better of its two sources).
 *   nodes: scratch, int32 pairs (parent, token), n_nodes >= cfm_ctc_beam_nodes(B, T, beam) = B * beam * (T + 1) pairs.
 *   nbest_tokens int64 [B, beam, T] (entry n holds nbest_len[b, n] tokens, the rest is not touched), nbest_len int32 [B, beam], nbest_score
 *   f32 [B, beam], best first; entries beyond the live prefixes have length 0 and score -inf.  lens[b] == 0: one empty hypothesis, score 0. */
typedef struct {
    const int32_t* idx;
    const float* logp;
    const int32_t* lens;
    int32_t* nodes;
    int64_t n_nodes;
    int64_t* nbest_tokens;
    int32_t* nbest_len;
    float* nbest_score;
    int32_t B, T, V, k, beam, blank;
} cfm_ctc_beam_desc;
int64_t cfm_ctc_beam_nodes(int32_t B, int32_t T, int32_t beam);
int cfm_ctc_prefix_beam(const cfm_ctc_beam_desc* d, cfm_stream_t stream);

/* cfm_ctc_align: CTC forced alignment (csrc/ctc.hip) -- the best single alignment of each utterance's frames to ITS labels, the max-plus
 *   (Viterbi) twin of cfm_ctc_nll's alpha recursion.  The reference has nothing of the kind; the algorithm is stated in float64 in
 *   tests/ctc_align_ref.py.  logits / ld / enc_lens / labels / label_lens / work exactly as for cfm_ctc_nll; blank is 0 as in the loss (an
 *   alignment against a head uses the blank the head was trained with); labels outside [0, V) are clamped as the loss clamps them; Umax <= 255.
 *   With lp[t, c] = log_softmax(logits[t, :V])[c], len = enc_lens[b] clamped to [0, T], U = label_lens[b] clamped to [0, Umax] and the extended
 *   sequence z = (0, y1, 0, ..., yU, 0) of S = 2U + 1 states:
 *       delta_0[s] = lp[0, z_s] for s < 2, -inf otherwise
 *       delta_t[s] = lp[t, z_s] + max(delta_{t-1}[s], delta_{t-1}[s-1], delta_{t-1}[s-2])    the s-2 term only where z_s != 0 and z_s != z_{s-2}
 *   Ties: the candidates are taken in the order stay, s-1, s-2 and a later one replaces an earlier one only if it is STRICTLY greater.  The
 *   path ends in state S-2 (the last label) unless delta_{len-1}[S-1] is strictly greater; with U = 0 it ends in state 0.  From there the
 *   recorded moves are followed back to frame 0.  The recursion runs in f32 on lp[t, .] - max_s lp[t, z_s] (no argmax moves); the per-frame
 *   maxima are added back to the score in fp64.
 *   score f32 [B]: the path's log-probability; -inf when no alignment exists (len < U + the number of adjacent equal labels, or len == 0 < U),
 *     0 for len == 0 and U == 0.
 *   path int32 [B, T]: the state index s_t for t < len, -1 for t >= len and in every frame of an utterance without an alignment.
 *   start / end int32 [B, Umax]: the first and last frame (inclusive) whose state is 2u + 1; token_logp f32 [B, Umax]: the sum over those
 *     frames of lp[t, y_u] (f32, in frame order).  Entries u >= U, and all of an utterance without an alignment, are -1, -1 and -inf.
 *   work: f32 scratch [B, T, 2*Umax + 2] as for cfm_ctc_nll; scratch: the recorded moves, scratch_bytes >= cfm_ctc_align_scratch_bytes(B, T, Umax)
 *     = B * T * ((2*Umax + 1) rounded up to a multiple of 4) bytes (one byte per frame and state), 4-byte aligned.
 *   Two launches, no host synchronisation. */
typedef struct {
    const float* logits;
    int64_t ld;
    const int32_t* enc_lens;
    const int32_t* labels;
    const int32_t* label_lens;
    float* work;
    void* scratch;
    int64_t scratch_bytes;
    int32_t* path;
    float* score;
    int32_t *start, *end;
    float* token_logp;
    int32_t B, T, V, Umax;
} cfm_ctc_align_desc;
int64_t cfm_ctc_align_scratch_bytes(int32_t B, int32_t T, int32_t Umax);
int cfm_ctc_align(const cfm_ctc_align_desc* d, cfm_stream_t stream);

/* cfm_edit_distance: Levenshtein distance of P hypothesis-reference pairs in one launch, with one fixed optimal alignment each
 *   (csrc/edit_distance.hip) -- the device counterpart of the reference's torchmetrics.WordErrorRate; stated in pure Python in
 *   tests/edit_distance_ref.py.  Tokens are int32 and are compared for equality only (any value, negative included).  Pair p is hypothesis
 *   row p, h[0:H] with H = hyp_lens[p] clamped to [0, Hmax], against reference row ref_index[p] (clamped to [0, R); ref_index null: row p,
 *   and P == R), r[0:U] with U = ref_lens[.] clamped to [0, Umax]; columns at and past the lengths are never read.  Hmax, Umax <= 1024.
 *       D[i][0] = i, D[0][j] = j, D[i][j] = min(D[i-1][j-1] + (r[i-1] != h[j-1]), D[i-1][j] + 1, D[i][j-1] + 1);     dist[p] = D[U][H]
 *   The alignment is the backtrace from (U, H) to (0, 0) that takes the FIRST rule that applies: (1) i > 0, j > 0 and
 *   D[i][j] == D[i-1][j-1] + (r[i-1] != h[j-1]): diagonal, a hit when the tokens are equal, a substitution otherwise; (2) i > 0 and
 *   D[i][j] == D[i-1][j] + 1: a deletion (a reference token without a hypothesis token); (3) an insertion.
 *   counts int32 [P, 4] = (S, D, I, hits); ops uint8 [P, Hmax + Umax]: the ops in forward order, 1 hit, 2 substitution, 3 deletion,
 *     4 insertion, 0 from ops_len[p] to the row's end; ops_len int32 [P].  counts may be null together with ops and ops_len (distance
 *     only: no scratch is touched); ops and ops_len may be null on their own, and are null or not together.
 *   scratch: the recorded moves, 2 bits per cell, needed only with counts: scratch_bytes >= cfm_edit_distance_scratch_bytes(P, Hmax, Umax)
 *     = P * Umax * 64 * (1, 2 or 4 bytes for Hmax <= 256, <= 512, <= 1024), 0 when Hmax or Umax is 0; 4-byte aligned.
 *   One launch, one wavefront per pair, no host synchronisation; integer arithmetic, so the result is exact. */
typedef struct {
    const int32_t* hyp;
    const int32_t* hyp_lens;
    const int32_t* ref;
    const int32_t* ref_lens;
    const int32_t* ref_index;
    int32_t* dist;
    int32_t* counts;
    uint8_t* ops;
    int32_t* ops_len;
    void* scratch;
    int64_t scratch_bytes;
    int32_t P, R, Hmax, Umax;
} cfm_edit_distance_desc;
int64_t cfm_edit_distance_scratch_bytes(int32_t P, int32_t Hmax, int32_t Umax);
int cfm_edit_distance(const cfm_edit_distance_desc* d, cfm_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * RNN-T beam search on the transducer head: n-best lists with scores, B utterances at once, 1 <= beam <= 15 hypotheses each, everything
 * float32 (csrc/greedy.hip).  The search is alignment-length synchronous and is stated once, in float64, in tests/rnnt_beam_ref.py (the
 * reference project has no beam search): a hypothesis is (string, frame t, symbols fc emitted on that frame, score = log of the summed
 * probability of the alignments found, the predictor input (token, h, c) as cfm_greedy_desc keeps it).  One step, per live hypothesis:
 * logp = log_softmax over the V real classes of the joint at (t, predictor output); it offers its blank (t + 1, fc = 0, predictor input
 * unchanged) and, unless fc == max_symbols or its length == max_len, its `beam` best non-blank classes (the lower class first among equal
 * values); candidates that are the same TOKEN STRING are merged with logaddexp (compared by length, last token and a 64-bit incremental
 * hash, collision bound in csrc/greedy.hip; only a blank candidate and an extension can meet, the blank candidate's t and state stay);
 * the `beam` best are kept -- higher score, then the better-ranked parent, then the blank before the extensions, then the lower class, a
 * merged candidate with the better of its sources; kept candidates with t == lens[b] are finished and enter the finished set (the `beam`
 * best by score); with that set full, live hypotheses whose score is below its worst are dropped.  An utterance is done when no
 * hypothesis is live, after at most lens[b] + max_len + 1 steps.
 *   cfm_rnnt_beam_begin  the empty hypothesis (score 0, token = blank, zero LSTM state) per utterance; lens[b] <= 0: done at once, the
 *                        empty hypothesis with score 0 is its result.  n_done [1] counts the utterances that are done.
 *   cfm_rnnt_beam_step   one step for every utterance that is not done (L + 5 launches); when n_done == B every launch returns at once.
 *                        The step that empties an utterance's live set writes its result.
 * Rows: hypothesis slot j of utterance b is row b * beam + j, R = B * beam <= 64 rows in all; an utterance's live hypotheses are its
 * first slots in rank order (live [R] int32 1 / 0).  Weights as in cfm_greedy_desc (out_w [Vp, J], rows >= V zero, out_b there -inf),
 * enc_proj [B, T, J], lens int64 [B] (clamped to T).  beam + 1 <= V <= 2^20.
 *   per row [R]: token / t / hash int64, fc / len / node / parent / ext / live int32, score f32; parent and ext say which row of the
 *     previous step the slot continues and whether it extended it.
 *   h / c f32 [2, L, R, H]: a step reads buffer `parity` and writes the new slots' states to the other one, so the caller alternates
 *     parity 0, 1, 0, ... from begin on (steps after the last live one change nothing).  h_new / c_new [L, R, H].
 *   scratch: pred [R, P], act [R, J], logits [R, Vp], topk_idx int32 / topk_logp f32 [R, beam + 1], lse [R]; nodes int32 pairs
 *     (parent, token), n_nodes >= cfm_rnnt_beam_nodes(B, T, max_len, beam) = B * (beam * (T + max_len + 1) + 1) pairs; the finished
 *     set fin_score f32 / fin_node / fin_len int32 [B, beam], n_fin [B]; step int32 [B] the steps an utterance took; done uint8 [B].
 *   result: nbest_tokens int64 [B, beam, max_len] (entry n holds nbest_len[b, n] tokens, the rest is not touched), nbest_len int32
 *     [B, beam], nbest_score f32 [B, beam], best first; entries beyond the finished ones have length 0 and score -inf.  No length
 *     normalisation.
 *   len_by_frames != 0: a hypothesis of utterance b holds at most min(max_len, lens[b]) tokens (the search's default: max_len = T). */
typedef struct {
    const float* embed;
    const float* lstm_w[4];
    const float* lstm_b[4];
    const float *proj_w, *proj_b, *pf_w, *pf_b, *out_w, *out_b;
    const float* enc_proj;
    const int64_t* lens;
    int64_t *token, *t, *hash;
    int32_t *fc, *len, *node, *parent, *ext, *live;
    float* score;
    float *h, *c, *h_new, *c_new, *pred, *act, *logits;
    int32_t* topk_idx;
    float *topk_logp, *lse;
    int32_t* nodes;
    int64_t n_nodes;
    float* fin_score;
    int32_t *fin_node, *fin_len, *n_fin, *step;
    uint8_t* done;
    int32_t* n_done;
    int64_t* nbest_tokens;
    int32_t* nbest_len;
    float* nbest_score;
    int32_t B, T, L, E, H, P, J, V, Vp, beam, blank, max_symbols, max_len, len_by_frames, parity;
} cfm_rnnt_beam_desc;
int64_t cfm_rnnt_beam_nodes(int32_t B, int32_t T, int32_t max_len, int32_t beam);
int cfm_rnnt_beam_begin(const cfm_rnnt_beam_desc* d, cfm_stream_t stream);
int cfm_rnnt_beam_step(const cfm_rnnt_beam_desc* d, cfm_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Streaming RNN-T beam search: the search above with a beam carried across encoder chunks (csrc/greedy.hip; the algorithm is stated in
 * float64 in tests/rnnt_beam_ref_stream.py).  Per stream, avail[b] encoder frames have been fed and final[b] says whether the utterance
 * has ended (n = avail).  Before each step: final set -- the offline step with n = avail; final not set -- the stream steps only if every
 * live hypothesis has t <= avail - 2, else it is PAUSED and the step changes nothing about it.  After a permitted step every t <= avail - 1
 * < n for any n the utterance can still have (a final that arrives with no new frame included), so for every split of an utterance into
 * feeds the steps taken, the live sets and the n-best list are those of cfm_rnnt_beam_step on the whole utterance; the beam trails the
 * encoder by one frame.
 *   `beam` is the offline descriptor with these readings: T = max_frames, enc_proj [B, max_frames, J] is filled as frames arrive (no
 *     ring: a live hypothesis may sit many frames behind avail), lens int64 [B] holds the frames of the chunk being FED (clamped to
 *     0..chunk), n_done [1] counts the streams that are done OR paused ("idle": when it reaches B the launches before the control kernel
 *     return at once; the host reads it once per replay), len_by_frames = 0 (max_len is explicit: n is not known), n_nodes >=
 *     cfm_rnnt_beam_nodes(B, max_frames, max_len, beam).  Limits as offline: B * beam <= 64, 1 <= beam <= 15.
 *   avail int32 [B], final / paused uint8 [B]; feed_final uint8 [B] or null: the streams whose utterance ends with this feed; overflow
 *     int32 [1]: a feed with avail + lens > max_frames sets it and leaves the stream as it was (the host raises).
 *   enc f32 [B, chunk, D] the chunk's encoder output, ef_w [J, D] / ef_b [J] the joint's enc_ffn, chunk_proj f32 [B * chunk, J] scratch.
 *   report: best_tokens int64 [B, max_len], best_len int32 [B], best_score f32 [B] the top-ranked live hypothesis; stable_len int32 [B]
 *     the length of the longest common prefix BY TOKENS of all live hypotheses' strings: it only grows and is a prefix of every entry of the
 *     final n-best list.  Entries of best_tokens below the previous stable_len are not rewritten (they cannot change).
 *   cfm_rnnt_beam_stream_reset   cfm_rnnt_beam_begin's work for the streams with mask[b] != 0 (mask null: all): the empty hypothesis,
 *                                zero state in both buffers, avail = 0, not final, not done, paused; the others are not touched.
 *   cfm_rnnt_beam_stream_feed    enc_ffn of the chunk (one M-tiled product), then one launch that appends lens[b] projected rows at row
 *                                avail[b] of each stream, advances avail, latches final and evaluates the pause rule again.  final with
 *                                avail == 0: done, the result is the empty hypothesis with score 0.  A done stream ignores feeds.
 *   cfm_rnnt_beam_stream_step    the offline step's launches with the streaming instance of the control kernel (L + 5 launches).  h / c
 *                                alternate by the caller's parity as offline; a paused stream's control workgroup copies its live slots'
 *                                state to the other buffer each step, so the step that resumes it finds it whichever parity it has --
 *                                PROVIDED the caller runs an even number of steps between feeds, starting at parity 0.
 *   cfm_rnnt_beam_stream_report  one launch: best / stable of every stream that is not done (a done stream's result is nbest_*).
 * Reads at the frontier: paused and dead rows still pass through the joint on stale inputs; the joint-input launch reads
 * enc_proj[b, min(t, max_frames - 1)], inside the buffer for any t, and a row whose output is used is live in a stepping stream, so
 * t <= avail - 1: rows >= avail, which nobody has written, never reach a result. */
typedef struct {
    cfm_rnnt_beam_desc beam;
    const float *enc, *ef_w, *ef_b;
    float* chunk_proj;
    int32_t* avail;
    uint8_t *final, *paused;
    const uint8_t* feed_final;
    int32_t* overflow;
    int64_t* best_tokens;
    int32_t *best_len, *stable_len;
    float* best_score;
    int32_t chunk, D;
} cfm_rnnt_beam_stream_desc;
int cfm_rnnt_beam_stream_reset(const cfm_rnnt_beam_stream_desc* d, const uint8_t* mask, cfm_stream_t stream);
int cfm_rnnt_beam_stream_feed(const cfm_rnnt_beam_stream_desc* d, cfm_stream_t stream);
int cfm_rnnt_beam_stream_step(const cfm_rnnt_beam_stream_desc* d, cfm_stream_t stream);
int cfm_rnnt_beam_stream_report(const cfm_rnnt_beam_stream_desc* d, cfm_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Sample-rate conversion, waveform in, waveform out, one launch (csrc/resample.hip): torchaudio.transforms.Resample(orig_freq, new_freq) with its
 * defaults (sinc_interp_hann, lowpass_filter_width 6, rolloff 0.99), the first line of the reference's preprocess / preprocess_stream
 * (src/deploy.py:108-110, :129-131) and processor.resample (src/processor.py:49-59).
 *
 * FORMULA.  g = gcd(orig, new), o = orig / g, n = new / g, base = min(o, n) * 0.99, width = ceil(6 o / base).  For phase j < n and tap
 *   k = i + width, i = -width .. width + o - 1 (n_taps = 2 width + o per phase):  t = clamp((-j / n + i / o) base, -6, 6),
 *   h[j][k] = (t == 0 ? 1 : sin(pi t) / (pi t)) cos^2(pi t / 12) base / o.   y[q n + j] = sum_k h[j][k] seq[q o + k].
 * PADDING.  seq is the input with `width` zeros in front of it and zeros behind it (torchaudio pads width on the left, width + o on the right);
 *   the zeros are operands like any other (0.0f in LDS).
 * OUTPUT LENGTH.  ceil(n L / o) samples for an input of L samples.
 * TABLE.  taps f32 [tap_off[n]]: phase j's one run of live taps (|h| >= 2^-60, computed in float64 on the host; the others are the clamped ends
 *   of the window) is taps[tap_off[j] .. tap_off[j + 1]), its first tap is k = tap_first[j]; tap_first int32 [n], tap_off int32 [n + 1].
 *   n <= 1024 and tap_off[n] <= 16384 (64 KiB): the bank and a tile's input span stay in LDS.
 * SUMMATION ORDER (part of the contract).  An output sample is ONE f32 fmaf chain over its live taps in ascending tap order, starting from +0.0f:
 *   acc = fmaf(taps[.], seq[.], acc).  It therefore has the same bits whichever tile, call or mode computed it.
 *   samples   [B, ld] int16 (samples_i16 != 0; exact in f32) or f32;   out f32 [B, ld_out], `cap` columns of each row are written
 *
 * cfm_resample (offline): the input of item b is samples[b, 0 .. lengths[b]) (clamped to n_cols); out_lens[b] <- ceil(n len / o) (clamped to cap), the
 *   columns at or beyond it are written as zeros.
 * cfm_resample_stream (B streams, packets of any size): stream b brings n_new[b] >= 0 samples (clamped to n_cols; what lies behind them in its row is
 *   never read) and final[b] != 0 when its utterance ends with them.  State per stream: counts int64 [B, 2] = (input samples seen c, output blocks
 *   emitted Q) and tail f32 [B, tail_cap]: the input from sample Q o - width on, c - Q o + width samples (the part before sample 0 is the left padding
 *   and reads as zero whatever the buffer holds: clearing counts resets a stream).  EMISSION RULE: a call emits every whole block q >= Q with
 *   (q + 1) o + width <= c -- all of its taps' samples have arrived -- as n samples each, left-aligned in out[b]; a final call emits everything up to
 *   ceil(n c / o) and leaves the stream reset (counts 0, 0).  out_lens[b] <- the samples emitted, the columns behind them are zeros.  A stream with
 *   n_new = 0 that is not final changes nothing.  tail_cap >= 2 width + o (a stream holds back fewer than width + o input samples); *_in and *_out
 *   must not alias (the caller swaps them); cap = 0 is legal (out may then be null), n_cols = 0 too (samples may then be null). */
typedef struct {
    const void* samples;
    const int32_t* lengths;          /* offline */
    const float* taps;
    const int32_t *tap_first, *tap_off;
    float* out;
    int32_t* out_lens;
    int64_t ld, ld_out;
    int32_t B, n_cols, cap, samples_i16, o, n, width, n_live; /* n_live = tap_off[n], the length of `taps` */
    const int32_t *n_new, *final;    /* streaming: int32 [B] each */
    const float* tail_in;            /* f32 [B, tail_cap] */
    float* tail_out;
    const int64_t* counts_in;        /* int64 [B, 2] */
    int64_t* counts_out;
    int32_t tail_cap;
} cfm_resample_desc;
int cfm_resample(const cfm_resample_desc* d, cfm_stream_t stream);
int cfm_resample_stream(const cfm_resample_desc* d, cfm_stream_t stream);
/* Input blocks (o samples in, n out) per workgroup tile for this reduced rate pair; 0 when the pair does not fit in LDS. */
int32_t cfm_resample_tile_blocks(int32_t o, int32_t n, int32_t width);

/* ------------------------------------------------------------------------------------------------
 * Training augmentation on the device: the two stages of the reference's recipe that sit between the waveform and the encoder
 * (exp/data_config.json speed_perturb / spec_aug; src/dataset.py:135-138 and :160-167).
 *
 * cfm_resample_group (csrc/resample.hip): cfm_resample with ONE RATE PAIR PER ITEM, one launch over a batch that mixes up to
 *   CFM_RESAMPLE_MAX_BANKS pairs.  Speed perturbation by a factor s at rate R is torchaudio.functional.speed: resample from int(s R) to R
 *   with the filter above -- at 16 kHz, 0.9 is o = 9, n = 10 and 1.1 is o = 11, n = 10.  (The reference calls sox's `speed` + `rate`,
 *   another filter; the definition here is the specification.)
 *   bank int32 [B] selects the item's bank (clamped to [0, G)); banks[g] is its geometry: the reduced pair o, n, `width`, n_live, where
 *   its part of each concatenated table starts (taps[taps_at ..+ n_live), tap_first[first_at ..+ n), tap_off[off_at ..+ n + 1), offsets
 *   relative to taps_at), and tile_blocks = cfm_resample_tile_blocks(o, n, width) > 0.  n_taps, n_first, n_off are the tables' lengths.
 *   A bank with o == n is the IDENTITY: the item is copied (int16 -> f32 exactly), its other fields are not read, and the tables may be
 *   null when every bank is one.
 *   Contract: out_lens[b] <- ceil(n_b len_b / o_b) (len clamped to n_cols, the result to cap); every column of out [B, cap] is written
 *   exactly once, those at or beyond out_lens[b] as +0.0f; nothing is read at or past an item's own len_b samples.  An output sample is
 *   cfm_resample's f32 fmaf chain (SUMMATION ORDER above): item b equals cfm_resample on that item alone at that pair bit for bit. */
#define CFM_RESAMPLE_MAX_BANKS 8
typedef struct {
    int32_t o, n, width, n_live, taps_at, first_at, off_at, tile_blocks;
} cfm_resample_bank;
typedef struct {
    const void* samples;             /* [B, ld] int16 (samples_i16 != 0) or f32 */
    const int32_t *lengths, *bank;   /* int32 [B] each */
    const float* taps;
    const int32_t *tap_first, *tap_off;
    float* out;                      /* f32 [B, ld_out] */
    int32_t* out_lens;
    int64_t ld, ld_out;
    int32_t B, n_cols, cap, samples_i16, G, n_taps, n_first, n_off;
    cfm_resample_bank banks[CFM_RESAMPLE_MAX_BANKS];
} cfm_resample_group_desc;
int cfm_resample_group(const cfm_resample_group_desc* d, cfm_stream_t stream);

/* cfm_spec_augment (csrc/augment.hip): SpecAugment in place, processor.spec_aug (src/processor.py:151-172) for a ragged batch in one
 *   launch.  feats f32 [B, T_max, F], element (b, t, f) at feats[b item_stride + t row_stride + f]; T = lengths[b] clamped to
 *   [0, T_max]; ids uint32 [B] name the items (null: ids[b] = b).  num_t_mask + num_f_mask <= CFM_SPEC_MAX_MASKS; max_t, max_f >= 1.
 *   DRAWS (part of the contract).  r(b, k) = cfm_hash32(cfm_hash32(seed, ids[b]), k) with
 *       cfm_hash32(s, i): h = (i * 0x9E3779B1) ^ s;  h ^= h >> 16;  h *= 0x85EBCA6B;  h ^= h >> 13;  h *= 0xC2B2AE35;  h ^= h >> 16   (uint32)
 *     and U[0, N - 1] drawn from r is (uint64(r) * N) >> 32 (multiply-high: a value's probability is off 1 / N by at most 2^-32, a
 *     relative bias of at most N / 2^32).  Mask m = 0 .. num_t_mask + num_f_mask - 1, the time masks first, uses k = 2 m for its start
 *     and k = 2 m + 1 for its length:
 *       time mask i   (m = i):               start = U[0, T - 1], len = 1 + U[0, max_t - 1], end = min(T, start + len): rows [start, end) <- 0.0f
 *       freq mask i   (m = num_t_mask + i):  start = U[0, F - 1], len = 1 + U[0, max_f - 1], end = min(F, start + len): columns [start, end)
 *                                            of rows [0, T) <- 0.0f
 *     T == 0 (or F == 0): the item has no masks (the reference would raise); its rows of `masks` are (0, 0).
 *   A step of training enters through the seed: seed + 0x9E3779B1 * step mod 2^32, the dropout sites' convention.
 *   The kernel only STORES +0.0f to masked elements: it never loads from feats and touches neither rows at or past T nor unmasked
 *   elements, so its traffic is the masked area.  masks int32 [B, num_t_mask + num_f_mask, 2] = (start, end), optional. */
#define CFM_SPEC_MAX_MASKS 32
typedef struct {
    float* feats;
    const int32_t* lengths;
    const uint32_t* ids;
    int32_t* masks;
    int64_t item_stride, row_stride;
    int32_t B, T_max, F, num_t_mask, num_f_mask, max_t, max_f;
    uint32_t seed;
} cfm_spec_augment_desc;
int cfm_spec_augment(const cfm_spec_augment_desc* d, cfm_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Attention rescoring of n-best lists (csrc/rescore.hip; the definition is tests/attention_decoder_ref.py in float64, the host side
 * decoder.AttentionRescorer).  P = B * N hypotheses, Lc = Lmax + 1 decoder positions each.
 *
 * cfm_rescore_prep: everything a decoder pass needs from the device n-best buffers of the beam searches, one launch, no host synchronisation.
 *   tokens int32 [B, N, Lmax], nlen int32 [B, N], score f32 [B, N] (the first-pass scores); 1 <= N <= 16, 1 <= Lc <= 1024.  Hypothesis p is
 *   UNUSED when nlen[p] < 0 or score[p] = -inf; otherwise L = min(nlen[p], Lmax), Lcp = L + 1, in = (sos, y_1..y_L), tg = (y_1..y_L, eos).
 *     x0 [P * Lc, D] f32        row (p, i) = embed[in_i] * sqrt(D) + pe[i] for i < Lcp (evaluated in double, rounded once), else 0
 *     targets int32 [P, Lc]     tg_i for i < Lcp, else -1
 *     mask uint8 [P, Lc, Lc]    mask[p][i][j] = (j <= i and j < Lcp): causal and valid; no query row of a used hypothesis is empty
 *   x0_r / targets_r (null, or both with embed_r): the same for the reversed hypothesis, in = (sos, y_L..y_1), tg = (y_L..y_1, eos), through
 *   the right decoder's embedding table embed_r; the mask is shared.  An unused hypothesis is dead throughout: x0 rows 0, targets -1, mask 0.
 *   embed, embed_r f32 [V, D] dense, pe f32 [>= Lc, D] dense (attention._sinusoid_table, indexed by POSITION).  Tokens are clamped into
 *   [0, V) for the gather (the caller's to guarantee).  Plain vector stores only. */
typedef struct {
    const int32_t* tokens;
    const int32_t* nlen;
    const float* score;
    const float* embed;
    const float* embed_r;
    const float* pe;
    float* x0;
    float* x0_r;
    int32_t* targets;
    int32_t* targets_r;
    uint8_t* mask;
    int32_t B, N, Lmax, D, V, sos, eos;
} cfm_rescore_prep_desc;
int cfm_rescore_prep(const cfm_rescore_prep_desc* d, cfm_stream_t stream);

/* cfm_token_logprob: the log-probability of ONE class per row of an output projection, without the logits:
 *     logp[m] = (x_m . w_t + b_t) - logsumexp_{c < V} (x_m . w_c + b_c),  t = target[m];     lse[m] (optional) = that logsumexp
 *   X [M, D] f32 or W's type, rows ldx elements apart (f32 is rounded to W's type first, as cfm_gemm does); W [Vp, D] bf16 / fp16 dense,
 *   bias f32 [Vp], Vp >= V: rows and bias entries V..Vp are never read.  D % 8 == 0, D <= 512; X and W 16-byte aligned, ldx a multiple of 4
 *   (f32) or 8 (16-bit).  The product is 16x16x32 MFMA with f32 accumulation, computed transposed (W . X^T: the vocabulary runs along a
 *   lane's accumulator registers, a lane owns one row); the logsumexp is online in f32 -- a running maximum and a running sum per row,
 *   folded per tile of 32 classes, lanes and wavefronts combined once at the end in a fixed order.  No atomics: the same input gives the
 *   same bits.  A row with target < 0 gives logp = 0 and lse = 0; a tile of 64 rows that holds no other row leaves without reading W;
 *   target >= V gives NaN.
 *   logits != NULL (f32 [M, >= V], rows ld elements apart): the product is skipped (X, W, bias are not read; D is ignored) and only the
 *   reduction and the gather run, one wavefront per row -- the second half of the unfused form (cfm_gemm, then this), which the fp32
 *   precision mode uses (cfm_gemm owns the three-product formula). */
typedef struct {
    const void* X;
    const void* W;
    const float* bias;
    const float* logits;
    const int32_t* target;
    float* logp;
    float* lse;
    int64_t ldx, ld;
    int32_t M, D, V, x_dtype, w_dtype;
} cfm_token_logprob_desc;
int cfm_token_logprob(const cfm_token_logprob_desc* d, cfm_stream_t stream);

/* cfm_rescore_combine: per hypothesis the sum of its Lc token log-probabilities in position order (f32, one add per position), the weighted
 * scores and the ranking of each utterance's N entries, one launch:
 *     left[p] = sum_i logp[p][i]; right[p] likewise over logp_r (0 when logp_r is null: reverse_weight must then be 0)
 *     att = left when reverse_weight = 0, else (1 - reverse_weight) * left + reverse_weight * right;   final = att + first_pass_weight * score
 *   (each product and sum rounded on its own).  An unused hypothesis (nlen < 0 or score = -inf) has final = -inf.  order int32 [B, N]:
 *   entry r is the index of the hypothesis of rank r -- higher final first, on an exact tie (unused entries among themselves included) the
 *   lower index, i.e. the better first-pass rank; a NaN final ranks as -inf.  1 <= N <= 16. */
typedef struct {
    const float* logp;
    const float* logp_r;
    const int32_t* nlen;
    const float* score;
    float* final_score;
    float* left;
    float* right;
    int32_t* order;
    int32_t B, N, Lc;
    float first_pass_weight, reverse_weight;
} cfm_rescore_combine_desc;
int cfm_rescore_combine(const cfm_rescore_combine_desc* d, cfm_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Label-smoothing loss of the attention decoder (csrc/lsm.hip; the reference's label_smoothing_loss.py:52-80; the definition in float64 is
 * tests/attention_loss_ref.py).  Per row m with target t = target[m] >= 0 over V classes, smoothing s, e = s / (V - 1): the target
 * distribution is q_c = 1 - s at c = t and e elsewhere, and the row's loss is the divergence sum_c q_c (log q_c - logp_c), 0 log 0 = 0.
 * With z the logits, lse their logsumexp and S = sum_{c < V} z_c this is
 *     loss[m] = C(s, V) - (1 - s - e) (z_t - lse) - e (S - V lse),     C = (1 - s) log(1 - s) + s log e   (evaluated in double on the host)
 * A row with target < 0 is ignored: loss = 0, lse = 0, dz = 0.  target >= V gives NaN.  0 <= s < 1; s > 0 needs V >= 2.
 *
 * cfm_lsm_loss: the forward.  X, W, bias, D, V, ldx, the dtypes and every limit are cfm_token_logprob's (D % 8 == 0, D <= 512, rows and
 *   bias entries V..Vp never read), and so are the product, the online logsumexp and the target gather: the two kernels include ONE product
 *   loop (csrc/vocab_tile.h).  A running f32 sum of the logits rides along; all combined in a fixed order, no atomics, the same input gives
 *   the same bits.  Writes loss f32 [M] and lse f32 [M] (both required: the backward reads lse).
 *   logits != NULL (f32 [M, >= V], rows ld apart): the product is skipped, one wavefront per row (the fp32 precision mode, and callers that
 *   hold logits). */
typedef struct {
    const void* X;
    const void* W;
    const float* bias;
    const float* logits;
    const int32_t* target;
    float* loss;
    float* lse;
    int64_t ldx, ld;
    int32_t M, D, V, x_dtype, w_dtype;
    float smoothing;
} cfm_lsm_loss_desc;
int cfm_lsm_loss(const cfm_lsm_loss_desc* d, cfm_stream_t stream);

/* cfm_lsm_grad: the backward.  dz[m][c] = g[m] (exp(z_c - lse[m]) - q_c) for c < V and exactly 0 for V <= c < Vk, as [M, Vk] with rows ldz
 *   apart: the operand of the projection's gradient products (dX = cfm_gemm(dz, W^T pack) with K = Vk; dW, db = cfm_gemm_tn(dz, X)).
 *   lse f32 [M] is the forward's; g f32 [M] the per-row scale (the upstream gradient over the denominator; ignored rows write 0 whatever g
 *   holds).  Vk >= V, Vk % 4 == 0, ldz >= Vk, ldz % 4 == 0, dz 16-byte aligned.  The logits are recomputed tile by tile on the forward's
 *   product loop and never stored; dz is of W's type.  Nothing past column Vk of a row, or past row M, is written.  Plain vector stores only.
 *   logits != NULL: elementwise over stored f32 logits; dz_dtype is f32, bf16 or fp16. */
typedef struct {
    const void* X;
    const void* W;
    const float* bias;
    const float* logits;
    const int32_t* target;
    const float* lse;
    const float* g;
    void* dz;
    int64_t ldx, ld, ldz;
    int32_t M, D, V, Vk, x_dtype, w_dtype, dz_dtype;
    float smoothing;
} cfm_lsm_grad_desc;
int cfm_lsm_grad(const cfm_lsm_grad_desc* d, cfm_stream_t stream);

/* cfm_lsm_reduce: out[0] = sum_m loss[m] / denom and out[1] = denom, one workgroup, a fixed order, no host read.  denom = batch when
 *   batch > 0 (the reference's default), else the number of targets >= 0 (normalize_length), at least 1: a call without one valid target
 *   gives 0 where the reference gives 0 / 0 -- the one deliberate difference. */
int cfm_lsm_reduce(const float* loss, const int32_t* target, int32_t M, int32_t batch, float* out, cfm_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Autoregressive beam search with the attention decoder (csrc/attn_search.hip; the definition is tests/attention_search_ref.py in float64, the
 * host side decoder.AttentionBeamSearch).  R = B * K rows: utterance b owns rows b*K .. b*K + K - 1, best hypothesis first.
 *
 * cfm_dec_step_attn: ONE query per (row, head) against keys and values that live in a store addressed through an indirection:
 *     s_j = (q_r,h . K[slot(r, j)]_h) / sqrt(dk),  p = softmax over j < klen(r),  out_r,h = sum_j p_j V[slot(r, j)]_h        (all in f32)
 *   q [R, >= D] rows ldq apart, out [R, D] rows ldo apart, store [slots, 2 D] dense (row s: K | V of one position), all of io_dtype
 *   (f32, bf16 or fp16; the fp32 precision mode keeps the store in f32).  D = H * dk.
 *   slot(r, j): the table form reads slot[r * slot_ld + j] (int32; several rows may name the same slots: shared ancestors); with slot NULL
 *   it is (r / group) * stride + j -- cross-attention over [owners, stride] memory rows, `group` rows per owner.  A slot is clamped into
 *   [0, slots) before it is used, so no table content makes the kernel leave the store.
 *   klen(r): klen[r / klen_group] (int32), or, with klen NULL, step[0] + 1 -- a device step counter, so that a captured graph needs no
 *   host argument per step.  Clamped into [0, cap]; cap is the declared capacity (cap <= slot_ld, resp. cap <= stride).  klen = 0 writes zeros.
 *   kv_new (optional, table form only; [R, 2 D] rows ld_new apart): this step's own K | V.  It is the key of position klen - 1: the kernel
 *   stores it to slot(r, klen - 1) -- exactly that one store row per row r, head slice by head slice -- and attends to it from kv_new itself,
 *   so append and attend are one launch and nothing is read back.  Nothing is stored for a row with klen = 0.
 *   One wavefront per (row, head): scores with one key per lane into LDS, wave maximum and sum, then the context with dk / 4 lanes across a
 *   value row and 64 / (dk / 4) keys in flight, reduced through LDS in a fixed order.  No atomics: the same input gives the same bits.
 *   Limits (CFM_ERR_ARG): D % 8 == 0, dk % 4 == 0, dk <= 128, 1 <= cap <= 2048, ldq, ldo, ld_new multiples of 4, 16-byte aligned bases. */
typedef struct {
    const void* q;
    void* store;
    const int32_t* slot;
    const int32_t* klen;
    const int32_t* step;
    const void* kv_new;
    void* out;
    int64_t ldq, ld_new, ldo, slots;
    int32_t R, H, dk, cap, slot_ld, group, stride, klen_group, io_dtype;
} cfm_dec_step_attn_desc;
int cfm_dec_step_attn(const cfm_dec_step_attn_desc* d, cfm_stream_t stream);

/* cfm_dec_beam_prune: one search step's pruning and bookkeeping, one workgroup per utterance, no host synchronisation.
 *   topk_idx int32 / topk_logp f32 [R, k_ld]: per row its K best classes and their log-probabilities (cfm_ctc_topk on the step's f32 logits:
 *   descending, the lower class first among equal values).  Utterance b at step i = step[b], unless done[b]:
 *     candidates  an unfinished row offers its K classes at score[row] + logp (one f32 add); a finished row (its last token was eos)
 *                 offers itself alone, score unchanged
 *     order       higher score first, then the better-ranked parent, then the lower class; the best K are kept in that order (a row whose
 *                 score is -inf -- an unused beam slot of step 0 -- never beats a real candidate)
 *     per kept    token, score, finished, parent (a global row index), hlen (tokens before eos), klen (the next step's key count),
 *                 tokens int32 [R, Lmax] (the strings, eos included) and slots int32 [R, Lmax] (the ancestry table of cfm_dec_step_attn's
 *                 self-attention store) both reordered by parent IN PLACE, tokens[row][i] = the new token, slots[row][i + 1] =
 *                 (i + 1) * R + row: position j's K | V is written once, to slot j * R + (the row at step j), and never moved
 *     x           f32 [R, D]: the next step's decoder input rows embed[token] * sqrt(D) + pe[i + 1] (in double, rounded once)
 *     done        when every kept hypothesis is finished or i + 1 == max_len[b] (int32 [B], 1 <= max_len[b] <= Lmax): done[b] = 1, n_done += 1,
 *                 all_done[0] = 1 once n_done reaches B, and the n-best buffers nbest_tokens int32 [B, K, Lmax] (eos stripped; only the
 *                 first nbest_len entries are written), nbest_len int32 [B, K], nbest_score f32 [B, K] are written -- once; a kept
 *                 entry of score -inf has length 0
 *   INVARIANT: the rows of a done utterance keep valid indices for every later step a captured graph still runs: parent = the row itself,
 *   step, klen and tokens frozen, x rewritten from the frozen token and position; slots frozen too, but for the entry at the last position i,
 *   which is set to i * R + row when the utterance becomes done (kept siblings share their parent's slot at position i; a frozen row keeps
 *   appending its K | V at that position every later step, so the slot must be its own: no two rows write one slot).  Such a row attends
 *   within its own table; its outputs are ignored.  Plain C++ and vector stores only.
 *   1 <= K <= 16, K <= k_ld, K <= V, 1 <= Lmax <= 1023, B * K <= 1024; embed f32 [V, D], pe f32 [>= Lmax, D]. */
typedef struct {
    const int32_t* topk_idx;
    const float* topk_logp;
    const float* embed;
    const float* pe;
    const int32_t* max_len;
    float* score;
    int32_t* token;
    int32_t* parent;
    uint8_t* finished;
    int32_t* hlen;
    int32_t* klen;
    int32_t* tokens;
    int32_t* slots;
    float* x;
    int32_t* step;
    uint8_t* done;
    int32_t* n_done;
    int32_t* all_done;
    int32_t* nbest_tokens;
    int32_t* nbest_len;
    float* nbest_score;
    int32_t B, K, k_ld, Lmax, D, V, eos;
} cfm_dec_beam_prune_desc;
int cfm_dec_beam_prune(const cfm_dec_beam_prune_desc* d, cfm_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Joint CTC/attention decoding: the CTC prefix scorer of the attention beam search (csrc/ctc_prefix.hip; the definition is
 * tests/ctc_prefix_ref.py in float64, the host side decoder.JointBeamSearch).  x[t, c] = log_softmax(CTC logits of utterance b)[t, c] for
 * t < n = lens[b] (clamped to [0, T]); (+) is logaddexp.  A hypothesis g carries gamma_n[t], gamma_b[t] -- the log-probabilities of the
 * alignments of exactly g to frames 0..t that end in its last token / in blank -- and psi(g), the log-probability that the output starts with
 * g.  The empty g: gamma_n = -inf, gamma_b[t] = sum_{tau <= t} x[tau, blank], psi = 0.  For a candidate c (not blank, not eos), `last` the
 * last token of g:
 *     phi[t]      = gamma_b[t] if c == last, else gamma_n[t] (+) gamma_b[t]
 *     psi(g.c)    = init (+) (+)_{t=1..n-1} (phi[t-1] + x[t, c]),   init = x[0, c] if g is empty, else -inf
 *     gamma_n'[0] = init, gamma_b'[0] = -inf,  gamma_n'[t] = (gamma_n'[t-1] (+) phi[t-1]) + x[t, c],
 *     gamma_b'[t] = (gamma_n'[t-1] (+) gamma_b'[t-1]) + x[t, blank]
 *   psi(g.eos) = gamma_n[n-1] (+) gamma_b[n-1], the CTC log-likelihood of g itself; psi(g.blank) = -inf, and the state of g.blank is -inf
 *   throughout.  The increment delta = psi(g.c) - psi(g) is -inf whenever either term is -inf: no NaN is produced.
 * Layouts: Tp = T rounded up to 4.  x f32 [B, V, Tp], CLASS-major: a candidate's column is contiguous in t.  state f32 [2][R, Tp, 2]: two
 * halves of (gamma_n, gamma_b) pairs, R = B * K rows, utterance b owning rows b*K .. b*K + K - 1 as in cfm_dec_beam_prune; psi f32 [R].
 * The half that holds the hypotheses a step scores is step[b] & 1 (step: the prune's per-utterance counter), so a captured graph needs no
 * host argument per step.  No atomics, fixed reduction orders: the same input gives the same bits.  Plain C++ and vector stores only.
 *
 * cfm_ctc_logprob_t: once per search.  logits f32 [B*T, ld] as for cfm_ctc_topk (ld >= V, ld % 4 == 0); per frame t < lens[b] the
 *   max-shifted f32 log-sum-exp, x[b, c, t] = (logits - max) - log(sum).  Elements at t >= lens[b], the padding t >= T included, are NOT
 *   TOUCHED, and nothing below reads them.  1 <= T <= 2048, B <= 65535, logits and x 16-byte aligned. */
int cfm_ctc_logprob_t(const float* logits, int64_t ld, int32_t B, int32_t T, int32_t V, const int32_t* lens, float* x, cfm_stream_t stream);

/* cfm_ctc_prefix_score: once per step, before the prune, one workgroup per row.  topk_idx int32 / topk_logp f32 [R, P]: the row's P best
 *   attention classes (cfm_ctc_topk with k = P) and their log-probabilities.  Candidate j of an unfinished row of an utterance that is not
 *   done offers  (1 - ctc_weight) * topk_logp[j] + ctc_weight * delta(g . topk_idx[j])  (the attention term is dropped, not multiplied by
 *   zero, at ctc_weight = 1; a NaN offer counts as -inf).  g's last token is token[r], g is empty when hlen[r] <= 0, psi(g) is psi[r].
 *   The K best of the P offers are written in descending order, the lower class first among equal values, as out_idx int32 / out_logp f32
 *   [R, K] -- what cfm_dec_beam_prune takes as its top-k lists -- with cand_psi f32 [R, K] = psi(g.c) of each.  Every row of a finished
 *   hypothesis, of a done utterance or of an utterance without frames is written as (eos, -inf, -inf): the prune ignores it.
 *   A class index read from topk_idx is clamped into [0, V) before use.  One wavefront per candidate reduces over t: the maximum, then the
 *   shifted sum, each lane over t = 1 + lane, 65 + lane, ... and the lanes in wave_sum's order.
 * cfm_ctc_prefix_advance: once per step, after the prune (step[b] then counts the steps taken), one lane per row.  For every kept
 *   unfinished row r of an utterance that is not done: gamma_n', gamma_b' and psi of (parent[r], token[r]) from the parent's state in half
 *   (step[b] + 1) & 1, written to row r of half step[b] & 1 and to psi[r]; frames t >= lens[b] are not touched.  The parent's last token is
 *   tokens[r][hlen[r] - 2] (tokens int32 [R, Lmax], reordered by the prune; hlen[r] >= 1 is the new length, 1: the parent was empty).
 *   parent[r] is clamped into the utterance's rows, token[r] into [0, V), hlen[r] into [1, Lmax].  Finished rows, rows of done utterances and
 *   the half that was read stay bit-unchanged.
 * Limits (CFM_ERR_ARG): 1 <= K <= P <= 16, P <= V, 1 <= T <= 2048, R = B * K <= 1024, eos != blank, both in [0, V), ctc_weight in (0, 1],
 *   x and state 16-byte aligned. */
typedef struct {
    const float* x;
    float* state;
    float* psi;
    const int32_t* topk_idx;
    const float* topk_logp;
    const int32_t* token;
    const int32_t* hlen;
    const uint8_t* finished;
    const int32_t* step;
    const uint8_t* done;
    const int32_t* lens;
    const int32_t* parent;
    const int32_t* tokens;
    int32_t* out_idx;
    float* out_logp;
    float* cand_psi;
    int32_t B, K, P, T, V, Lmax, blank, eos;
    float ctc_weight;
} cfm_ctc_prefix_desc;
int cfm_ctc_prefix_score(const cfm_ctc_prefix_desc* d, cfm_stream_t stream);
int cfm_ctc_prefix_advance(const cfm_ctc_prefix_desc* d, cfm_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* CFM_H_ */
