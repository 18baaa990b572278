// greedy.hip -- the device steps of the two batched RNN-T greedy searches (reference src/model.py:215-269, greedy.py) on f32 weights:
// cfm_greedy_step decides ONE frame per stream and step, cfm_greedy_chunk_begin / cfm_greedy_chunk_step (the streaming recogniser's
// decoder) all remaining frames of a stream's chunk.  A step of either is the same predictor stage, then its own joint and control stage:
//
//   predictor (enqueue_predictor, L + 1 launches), shared
//     LSTM layers   gates = [x | h] . [W_ih | W_hh]^T + (b_ih + b_hh);  c' = sig(f) c + sig(i) tanh(g);  h' = sig(o) tanh(c')
//                   (layer 0's x is the embedding row of the stream's current token: a gather, no launch of its own)
//     projection    pred = h' . Wp^T + bp                                         (predictor.py:83)
//   cfm_greedy_step (3 launches; six in all for L = 2)
//     joint input   a = tanh(enc_proj[b, t_b] + pred . Wpf^T + bpf)               (joint.py:34-36; enc_ffn was applied to all frames once)
//     joint output  z = a . Wout^T + bout, per 16-class tile and stream the (max, first index) pair            (joint.py:37, model.py:254)
//     control       k = argmax over the tiles; the reference's branches as selects on the per-stream state (model.py:255-267)
//   cfm_greedy_chunk_step (4 launches): pred_ffn, the compact row list, the M-tiled vocabulary product, control across the lookahead --
//     described at its section below
//   cfm_rnnt_beam_step (5 launches): the RNN-T beam search, hypotheses as rows of the same predictor and joint launches -- described at its
//     section near the end of the file
//   cfm_rnnt_beam_stream_reset / _feed / _step / _report: that search with the beam carried across encoder chunks -- the last section
//
// The torch-operation form of a single-frame step (greedy.py) is ~45 small launches; the predictor's and the single-frame joint's products
// are "skinny": B <= 64 streams against weight matrices of 0.26-2.5 M elements, i.e. one read of 7.5 M f32 weights per step, spread over
// the chip.  Everything stays f32, so the argmax is the reference's wherever its two best logits are further apart than f32 rounding
// (DESIGN.md's margin rule): the products run on the f32 MFMA (v_mfma_f32_16x16x4_f32: exact f32 multiplies, f32 accumulation) -- one
// wavefront per 16 output columns, the weight rows as the A operand and up to four 16-stream tiles as B operands, both read as 16-byte
// pieces straight from memory (the contraction index is walked in the order lane group g holds k = 16 q + 4 g + r, the same for both
// operands).
//   * the LSTM weight rows are packed [unit][gate] so that the lane that owns output rows 4 g .. 4 g + 3 of a tile holds the four gates
//     (i, f, g, o) of one hidden unit of one stream: the cell update is lane-local;
//   * streams that are finished, or whose step produced a blank, keep their state: the candidates (h', c') go to side buffers and the
//     control launch selects (commit_state);
//   * every argmax follows torch.argmax's rule, the lowest index among equal values (take_better), from the lane to the control kernels.
#include <math.h>

#include "cfm_common.h"

namespace {

// (best, bi) <- (v, i) when v is larger, or equal with the lower index
__device__ __forceinline__ void take_better(float& best, int& bi, float v, int i) {
    if (v > best || (v == best && i < bi)) { best = v; bi = i; }
}

// The best of a 16-class tile of an MFMA product's output, per stream / row: the lane holds classes i0 .. i0 + 3 (v), the tile's other
// twelve are in the lanes 16, 32 and 48 further on; every lane ends up with the tile's pair.
__device__ __forceinline__ void tile_argmax(const f32x4 v, int i0, float& best, int& bi) {
    best = v.x;
    bi = i0;
    if (v.y > best) { best = v.y; bi = i0 + 1; }
    if (v.z > best) { best = v.z; bi = i0 + 2; }
    if (v.w > best) { best = v.w; bi = i0 + 3; }
#pragma unroll
    for (int o = 16; o < 64; o <<= 1) take_better(best, bi, __shfl_xor(best, o, 64), __shfl_xor(bi, o, 64));
}

// the LSTM's candidate state of this step becomes stream b's state (the step emitted); a: either control kernel's arguments
template <class Args>
__device__ __forceinline__ void commit_state(const Args& a, int b, int tid) {
    for (int i = tid; i < a.L * a.H; i += 256) {
        const int l = i / a.H, u = i - l * a.H;
        const int64_t o = ((int64_t)l * a.B + b) * a.H + u;
        a.h[o] = a.h_new[o];
        a.c[o] = a.c_new[o];
    }
}

struct SkinnyArgs {
    const float* W;          // [N, K] f32 row-major (N % 16 == 0, K % 16 == 0)
    const float* bias;       // [N]
    const float* x1;         // first K1 contraction columns: rows at x1 + row(b) * ld1 ...
    const int64_t* x1_rows;  // ... row(b) = x1_rows[b] when given (the embedding gather by token), else b
    int64_t ld1;
    int K1;
    const float* x2;         // remaining K - K1 columns: x2 + b * ld2 (LSTM: the layer's hidden state)
    int64_t ld2;
    int B, N, K;
    // epilogues
    float* out;              // EPI 0: out[b, n] (ld_out)
    int64_t ld_out;
    const float* c_in;       // EPI 1 (LSTM cell, N = 4 H): cell state [B, H]
    float *h_out, *c_out;    //        candidate h', c' [B, H]
    const float* enc;        // EPI 2: enc_proj [B, T, N];  a[b, n] = tanh(enc[b, min(t[b], T-1), n] + acc + bias)
    const int64_t* t_idx;
    int T;
    int enc_div;             //        enc's item of row b is b / enc_div (0: b itself) -- the beam search's rows, `beam` per utterance
    float* pmax;             // EPI 3: per (tile, b): best value / first index of the tile's 16 classes
    int* pidx;
    const int* n_done;       // when given (the chunk-lookahead step): every stream finished (*n_done >= B) -> the launch does nothing
    int done_at;             // ... *n_done >= done_at instead, when not 0 (the beam search counts utterances, B is its rows)
};

__device__ __forceinline__ float sigmoid_acc(float x) { return 1.0f / (1.0f + expf(-x)); }

template <int EPI>
__global__ __launch_bounds__(256) void cfm_skinny_kernel(const SkinnyArgs a) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int l15 = lane & 15, g = lane >> 4;
    const int tile = blockIdx.x * 4 + wave;                 // 16 output columns per wavefront
    if (tile * 16 >= a.N) return;
    if (a.n_done && *a.n_done >= (a.done_at ? a.done_at : a.B)) return;   // uniform: a step captured after the last stream finished costs empty launches only
    const int n0 = tile * 16;
    const int nbt = (a.B + 15) / 16;                        // <= 4 stream tiles
    f32x4 acc[4];
#pragma unroll
    for (int bt = 0; bt < 4; ++bt) acc[bt] = (f32x4){0.f, 0.f, 0.f, 0.f};
    const float* wrow = a.W + (int64_t)(n0 + l15) * a.K + 4 * g;
    const float* xr1[4];
    const float* xr2[4];
#pragma unroll
    for (int bt = 0; bt < 4; ++bt) {
        int b = bt * 16 + l15;
        b = b < a.B ? b : a.B - 1;
        const int64_t r1 = a.x1_rows ? a.x1_rows[b] : (int64_t)b;
        xr1[bt] = a.x1 + r1 * a.ld1 + 4 * g;
        xr2[bt] = a.x2 ? a.x2 + (int64_t)b * a.ld2 + 4 * g : xr1[bt];
    }
    const int nq = a.K / 16, nq1 = a.K1 / 16;
    for (int q = 0; q < nq; ++q) {                          // (unrolling by 4 to batch the requests: no gain, 63 vs 58 us per step)
        const f32x4 wv = *(const f32x4*)(wrow + 16 * q);
        const bool first = q < nq1;                         // uniform
        f32x4 xv[4];
#pragma unroll
        for (int bt = 0; bt < 4; ++bt) {
            if (bt < nbt) xv[bt] = first ? *(const f32x4*)(xr1[bt] + 16 * q) : *(const f32x4*)(xr2[bt] + 16 * (q - nq1));
        }
#pragma unroll
        for (int bt = 0; bt < 4; ++bt) {
            if (bt < nbt) {                                  // uniform
#pragma unroll
                for (int r = 0; r < 4; ++r) acc[bt] = __builtin_amdgcn_mfma_f32_16x16x4f32(wv[r], xv[bt][r], acc[bt], 0, 0, 0);
            }
        }
    }
    // lane (l15, g) holds output rows n0 + 4 g + r (r = 0..3) of stream bt * 16 + l15
    const f32x4 bv = *(const f32x4*)(a.bias + n0 + 4 * g);
#pragma unroll
    for (int bt = 0; bt < 4; ++bt) {
        const int b = bt * 16 + l15;
        if (bt >= nbt) break;
        const f32x4 v = acc[bt] + bv;
        const bool live = b < a.B;
        if constexpr (EPI == 0) {
            if (live) *(f32x4*)(a.out + (int64_t)b * a.ld_out + n0 + 4 * g) = v;
        } else if constexpr (EPI == 1) {                    // rows are [unit][i, f, g, o]: this lane owns unit (n0 >> 2) + g
            if (live) {
                const int H = a.N >> 2, u = (n0 >> 2) + g;
                const float c0 = a.c_in[(int64_t)b * H + u];
                const float c1 = sigmoid_acc(v.y) * c0 + sigmoid_acc(v.x) * tanhf(v.z);
                a.c_out[(int64_t)b * H + u] = c1;
                a.h_out[(int64_t)b * H + u] = sigmoid_acc(v.w) * tanhf(c1);
            }
        } else if constexpr (EPI == 2) {
            if (live) {
                int64_t t = a.t_idx[b];
                t = t < a.T ? t : a.T - 1;
                const int eb = a.enc_div ? b / a.enc_div : b;
                const f32x4 e = *(const f32x4*)(a.enc + ((int64_t)eb * a.T + t) * a.N + n0 + 4 * g);
                *(f32x4*)(a.out + (int64_t)b * a.ld_out + n0 + 4 * g) = (f32x4){tanhf(e.x + v.x), tanhf(e.y + v.y), tanhf(e.z + v.z), tanhf(e.w + v.w)};
            }
        } else {                                            // EPI 3: the tile's best class per stream, [tile, B]
            float best;
            int bi;
            tile_argmax(v, n0 + 4 * g, best, bi);
            if (g == 0 && live) {
                a.pmax[(int64_t)tile * a.B + b] = best;
                a.pidx[(int64_t)tile * a.B + b] = bi;
            }
        }
    }
}

template <int EPI>
int launch_skinny(const SkinnyArgs& a, hipStream_t s, const char* name) {
    const int tiles = a.N / 16;
    CfmProfScope prof(name, s, 2.0 * a.B * (double)a.N * a.K, (double)a.N * a.K * 4);
    CFM_LAUNCH((cfm_skinny_kernel<EPI>), dim3((unsigned)((tiles + 3) / 4)), dim3(256), 0, s, a);
    return cfm_launch_status(name);
}

// what cfm_greedy_desc and cfm_greedy_chunk_desc (Desc) have in common: the limits of the skinny launches, the weights, the per-stream
// state and the scratch both steps use; `who` is the entry point that was called
template <class Desc>
int check_common(const Desc* d, const char* who) {
    CFM_CHECK_ARG(d, "%s: null descriptor", who);
    CFM_CHECK_ARG(d->B > 0 && d->B <= 64 && d->L >= 1 && d->L <= 4 && d->E % 16 == 0 && d->H % 16 == 0 && d->P % 16 == 0 && d->J % 16 == 0 && d->Vp % 16 == 0 &&
                      d->n_steps > 0,
                  "%s: B <= 64 streams, <= 4 LSTM layers, sizes multiples of 16 (B=%d L=%d E=%d H=%d P=%d J=%d Vp=%d)", who, d->B, d->L, d->E, d->H, d->P, d->J, d->Vp);
    CFM_CHECK_ARG(d->embed && d->proj_w && d->proj_b && d->pf_w && d->pf_b && d->out_w && d->out_b && d->enc_proj && d->token && d->t && d->lens && d->count &&
                      d->frame_count && d->hyps && d->h && d->c && d->h_new && d->c_new && d->pred && d->act && d->pmax && d->pidx && d->done && d->n_done,
                  "%s: null pointer", who);
    return 0;
}

// The predictor stage of a step of either search: (token, h, c) -> candidates h_new / c_new [L, B, H] and pred [B, P].  n_done: null, or
// the device counter that turns the launches into empty ones once every stream is finished (SkinnyArgs::n_done).
template <class Desc>
int enqueue_predictor(const Desc* d, const int* n_done, hipStream_t s, const char* who, int done_at = 0) {
    const int B = d->B, H = d->H;
    for (int l = 0; l < d->L; ++l) {
        CFM_CHECK_ARG(d->lstm_w[l] && d->lstm_b[l], "%s: LSTM layer %d has no weights", who, l);
        SkinnyArgs a = {};
        a.W = d->lstm_w[l]; a.bias = d->lstm_b[l]; a.B = B; a.N = 4 * H; a.x2 = d->h + (int64_t)l * B * H; a.ld2 = H;
        if (l == 0) { a.x1 = d->embed; a.x1_rows = d->token; a.ld1 = d->E; a.K1 = d->E; }
        else { a.x1 = d->h_new + (int64_t)(l - 1) * B * H; a.ld1 = H; a.K1 = H; }
        a.K = a.K1 + H;
        a.c_in = d->c + (int64_t)l * B * H; a.h_out = d->h_new + (int64_t)l * B * H; a.c_out = d->c_new + (int64_t)l * B * H; a.n_done = n_done; a.done_at = done_at;
        if (int rc = launch_skinny<1>(a, s, "greedy_lstm")) return rc;
    }
    SkinnyArgs a = {};
    a.W = d->proj_w; a.bias = d->proj_b; a.B = B; a.N = d->P; a.K = a.K1 = H; a.x1 = d->h_new + (int64_t)(d->L - 1) * B * H; a.ld1 = H; a.out = d->pred; a.ld_out = d->P;
    a.n_done = n_done; a.done_at = done_at;
    return launch_skinny<0>(a, s, "greedy_proj");
}

// ---------------------------------------------------------------------------------------------------------------------------------------
// Single frame (cfm_greedy_step): the joint for the one frame each stream is on, the reference's loop body as selects.
// ---------------------------------------------------------------------------------------------------------------------------------------
struct CtlArgs {
    const float* pmax;
    const int* pidx;
    int ntiles, B, L, H, blank, n_steps;
    int64_t *token, *t, *count, *frame_count, *hyps;
    const int64_t* lens;
    int64_t hyp_cap, hyp_ld;
    float *h, *c;                // [L, B, H] state
    const float *h_new, *c_new;  // [L, B, H] candidates of this step
    uint8_t* done;
    int* n_done;                 // number of finished streams after this step (one int)
};

// one workgroup per stream: argmax over the tiles, then model.py:255-267 as selects
__global__ __launch_bounds__(256) void cfm_greedy_control_kernel(const CtlArgs a) {
    __shared__ float smax[256];
    __shared__ int sidx[256];
    __shared__ int s_nb;
    const int b = blockIdx.x, tid = threadIdx.x;
    float best = -INFINITY;
    int bi = 0x7fffffff;
    for (int tl = tid; tl < a.ntiles; tl += 256) {
        take_better(best, bi, a.pmax[(int64_t)tl * a.B + b], a.pidx[(int64_t)tl * a.B + b]);
    }
    smax[tid] = best;
    sidx[tid] = bi;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (tid < s) take_better(smax[tid], sidx[tid], smax[tid + s], sidx[tid + s]);
        __syncthreads();
    }
    const bool was_done = a.done[b] != 0;
    if (tid == 0) {
        const int k = sidx[0];
        const bool nb = k != a.blank && !was_done;
        s_nb = nb ? 1 : 0;
        int64_t fc = a.frame_count[b], t = a.t[b];
        if (nb) {
            const int64_t pos = a.count[b] < a.hyp_cap ? a.count[b] : a.hyp_cap;
            a.hyps[(int64_t)b * a.hyp_ld + pos] = k;
            a.count[b] += 1;
            a.token[b] = k;
            fc += 1;
        }
        const bool adv = (k == a.blank || fc >= a.n_steps) && !was_done;
        if (adv) { t += 1; fc = 0; }
        a.t[b] = t;
        a.frame_count[b] = fc;
        const bool dn = t >= a.lens[b];
        a.done[b] = dn ? 1 : 0;
        if (dn && !was_done) atomicAdd(a.n_done, 1);
    }
    __syncthreads();
    if (s_nb) commit_state(a, b, tid);                      // a non-blank: the LSTM's new state becomes the stream's state
}

}  // namespace

extern "C" int cfm_greedy_step(const cfm_greedy_desc* d, cfm_stream_t stream) {
    if (int rc = check_common(d, "cfm_greedy_step")) return rc;
    CFM_CHECK_ARG(d->T > 0, "cfm_greedy_step: T = %d frames", d->T);
    hipStream_t s = (hipStream_t)stream;
    const int B = d->B, H = d->H;
    if (int rc = enqueue_predictor(d, nullptr, s, "cfm_greedy_step")) return rc;
    {
        SkinnyArgs a = {};
        a.W = d->pf_w; a.bias = d->pf_b; a.B = B; a.N = d->J; a.K = a.K1 = d->P; a.x1 = d->pred; a.ld1 = d->P; a.out = d->act; a.ld_out = d->J; a.enc = d->enc_proj;
        a.t_idx = d->t; a.T = d->T;
        if (int rc = launch_skinny<2>(a, s, "greedy_joint_in")) return rc;
    }
    {
        SkinnyArgs a = {};
        a.W = d->out_w; a.bias = d->out_b; a.B = B; a.N = d->Vp; a.K = a.K1 = d->J; a.x1 = d->act; a.ld1 = d->J; a.pmax = d->pmax; a.pidx = d->pidx;
        if (int rc = launch_skinny<3>(a, s, "greedy_joint_out")) return rc;
    }
    CtlArgs c;
    c.pmax = d->pmax; c.pidx = d->pidx; c.ntiles = d->Vp / 16; c.B = B; c.L = d->L; c.H = H; c.blank = d->blank; c.n_steps = d->n_steps;
    c.token = d->token; c.t = d->t; c.count = d->count; c.frame_count = d->frame_count; c.hyps = d->hyps; c.lens = d->lens; c.hyp_cap = d->hyp_cap;
    c.hyp_ld = d->hyp_ld; c.h = d->h; c.c = d->c; c.h_new = d->h_new; c.c_new = d->c_new; c.done = d->done; c.n_done = d->n_done;
    CfmProfScope prof("greedy_control", s, 0.0, (double)B * (d->Vp / 16) * 8);
    CFM_LAUNCH(cfm_greedy_control_kernel, dim3((unsigned)B), dim3(256), 0, s, c);
    return cfm_launch_status("cfm_greedy_step (control)");
}

// ---------------------------------------------------------------------------------------------------------------------------------------
// Chunk lookahead (cfm_greedy_chunk_begin / cfm_greedy_chunk_step): the streaming recogniser's decoder.  The predictor output is a pure
// function of (token, LSTM state), which change only at an emission; between two emissions the joint is therefore evaluated for ALL
// remaining frames of a stream's chunk against the one current predictor output and the first non-blank frame is found on the device:
// a chunk costs at most 1 + (most emissions of any stream) steps instead of frames + emissions.  One step:
//
//   pred   the predictor stage (enqueue_predictor with n_done), pp = pred_ffn(pred); once every stream is done with the chunk (n_done == B)
//          these launches return at once, so the steps a captured graph holds beyond the chunk's last one cost empty launches only
//   rows   per stream b the frames f = t_b .. lens_b - 1 become rows of a COMPACT activation matrix: act[off_b + i] = tanh(encp[b, t_b + i] + pp[b]);
//          row_off / row_cnt / n_rows describe it (finished streams contribute no row, so they cost no product)
//   mtile  z = act . Wout^T + bout on n_rows rows, reduced to the (max, first index) per row and 16-class tile -- an M-tiled f32 MFMA
//          product: a wavefront holds a 64-row x 32-class tile (4 x 2 MFMA tiles), every weight fragment meets four row tiles from registers
//   ctl    one workgroup per stream: argmax per row, the first row whose class is not blank, model.py:255-267 across the lookahead
//
// cfm_greedy_chunk_begin applies enc_ffn to the chunk's (B chunk, D) encoder rows with the same M-tiled product (plain epilogue) and
// resets the per-chunk control state.
// ---------------------------------------------------------------------------------------------------------------------------------------
namespace {

struct MTileArgs {
    const float* W;          // [N, K] f32 row-major (N % 16 == 0, K % 16 == 0)
    const float* bias;       // [N]
    const float* x;          // [M, K] rows at x + m * ldx
    int64_t ldx;
    int M;                   // rows the launch was sized for ...
    const int* n_rows;       // ... and, when given, the number that exist this time (device side, <= M)
    int N, K;
    float* out;              // EPI 0: out[m, n] (ld_out)
    int64_t ld_out;
    float* pmax;             // EPI 1: per (row, 16-class tile): best value / first index, [M, ntiles]
    int* pidx;
};

// 256 threads = 4 wavefronts side by side along N; a wavefront: rows m0 .. m0 + 63 (blockIdx.y) x two 16-column tiles.  Operands are read
// as 16-byte pieces straight from memory in cfm_skinny_kernel's contraction order (lane group g holds k = 16 q + 4 g + r), the next
// pieces requested before the current ones are multiplied; per 16 k: 6 loads feed 32 MFMAs.
template <int EPI>
__global__ __launch_bounds__(256) void cfm_mtile_kernel(const MTileArgs a) {
    int M = a.M;
    if (a.n_rows) { const int n = *a.n_rows; M = n < M ? n : M; }
    const int m0 = blockIdx.y * 64;
    if (m0 >= M) return;                                    // row tiles that do not exist this step: no product
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int l15 = lane & 15, g = lane >> 4;
    const int ntl = a.N / 16;
    const int nt0 = (blockIdx.x * 4 + wave) * 2;
    if (nt0 >= ntl) return;
    const bool two = nt0 + 1 < ntl;                         // uniform
    const int nmt = (M - m0 + 15) / 16 < 4 ? (M - m0 + 15) / 16 : 4;
    f32x4 acc[2][4];
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) acc[j][mt] = (f32x4){0.f, 0.f, 0.f, 0.f};
    const float* w0 = a.W + (int64_t)(nt0 * 16 + l15) * a.K + 4 * g;
    const float* w1 = two ? w0 + (int64_t)16 * a.K : w0;
    const float* xr[4];
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) {
        int m = m0 + mt * 16 + l15;
        m = m < M ? m : M - 1;
        xr[mt] = a.x + (int64_t)m * a.ldx + 4 * g;
    }
    const int nq = a.K / 16;
    f32x4 wv0 = *(const f32x4*)w0, wv1 = *(const f32x4*)w1, xv[4];
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) xv[mt] = mt < nmt ? *(const f32x4*)xr[mt] : (f32x4){0.f, 0.f, 0.f, 0.f};
    for (int q = 0; q < nq; ++q) {
        const int qn = q + 1 < nq ? q + 1 : q;
        const f32x4 nw0 = *(const f32x4*)(w0 + 16 * qn), nw1 = *(const f32x4*)(w1 + 16 * qn);
        f32x4 nx[4];
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) nx[mt] = mt < nmt ? *(const f32x4*)(xr[mt] + 16 * qn) : (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) {
            if (mt < nmt) {                                  // uniform
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    acc[0][mt] = __builtin_amdgcn_mfma_f32_16x16x4f32(wv0[r], xv[mt][r], acc[0][mt], 0, 0, 0);
                    acc[1][mt] = __builtin_amdgcn_mfma_f32_16x16x4f32(wv1[r], xv[mt][r], acc[1][mt], 0, 0, 0);
                }
            }
        }
        wv0 = nw0; wv1 = nw1;
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) xv[mt] = nx[mt];
    }
    // lane (l15, g) holds output columns n0 + 4 g + r (r = 0..3) of row m0 + 16 mt + l15
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        if (j == 1 && !two) break;
        const int n0 = (nt0 + j) * 16;
        const f32x4 bv = *(const f32x4*)(a.bias + n0 + 4 * g);
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) {
            if (mt >= nmt) break;
            const int m = m0 + mt * 16 + l15;
            const f32x4 v = acc[j][mt] + bv;
            if constexpr (EPI == 0) {
                if (m < M) *(f32x4*)(a.out + (int64_t)m * a.ld_out + n0 + 4 * g) = v;
            } else {                                         // the tile's best class per row, [row, tile]
                float best;
                int bi;
                tile_argmax(v, n0 + 4 * g, best, bi);
                if (g == 0 && m < M) {
                    a.pmax[(int64_t)m * ntl + nt0 + j] = best;
                    a.pidx[(int64_t)m * ntl + nt0 + j] = bi;
                }
            }
        }
    }
}

template <int EPI>
int launch_mtile(const MTileArgs& a, hipStream_t s, const char* name) {
    const int ntl = a.N / 16;
    CfmProfScope prof(name, s, 2.0 * a.M * (double)a.N * a.K, ((double)a.N + a.M) * a.K * 4);
    CFM_LAUNCH((cfm_mtile_kernel<EPI>), dim3((unsigned)((ntl + 7) / 8), (unsigned)((a.M + 63) / 64)), dim3(256), 0, s, a);
    return cfm_launch_status(name);
}

struct ChunkBeginArgs {
    int64_t *token, *t, *frame_count;
    const int64_t* lens;
    float *h, *c;
    uint8_t* done;
    int *n_done, *steps;
    int B, L, H, blank, carry;
};

// one workgroup per stream: frame index and per-frame count to 0 (the reference starts every basic_greedy_search call with
// per_frame_noblk = 0); carry == 0: the predictor restarts from blank / zeros (greedy_search_streaming_eval, model.py:155-161) on the
// streams that have frames; an idle stream (lens == 0) keeps everything
__global__ __launch_bounds__(256) void cfm_chunk_begin_kernel(const ChunkBeginArgs a) {
    const int b = blockIdx.x, tid = threadIdx.x;
    const bool idle = a.lens[b] <= 0;
    if (tid == 0) {
        a.t[b] = 0;
        a.frame_count[b] = 0;
        a.done[b] = idle ? 1 : 0;
        if (!a.carry && !idle) a.token[b] = a.blank;
        if (b == 0) {
            int n = 0;
            for (int i = 0; i < a.B; ++i) n += a.lens[i] <= 0 ? 1 : 0;
            *a.n_done = n;
            *a.steps = 0;
        }
    }
    if (!a.carry && !idle) {
        for (int i = tid; i < a.L * a.H; i += 256) {
            const int l = i / a.H, u = i - l * a.H;
            const int64_t o = ((int64_t)l * a.B + b) * a.H + u;
            a.h[o] = 0.f;
            a.c[o] = 0.f;
        }
    }
}

struct ChunkRowsArgs {
    const float *encp, *pp;
    const int64_t *t, *lens;
    float* act;
    int *rows, *row_off, *row_cnt, *n_rows, *steps;
    int B, chunk, J;
};

// one workgroup per stream: its place in the compact row list (every workgroup sums the <= 64 counts itself), then its rows
__global__ __launch_bounds__(256) void cfm_chunk_rows_kernel(const ChunkRowsArgs a) {
    __shared__ int s_cnt[64];
    __shared__ int s_off, s_tot;
    const int b = blockIdx.x, tid = threadIdx.x;
    if (tid < a.B) {
        int64_t ti = a.t[tid], li = a.lens[tid];
        ti = ti < 0 ? 0 : ti;
        li = li < a.chunk ? li : a.chunk;
        s_cnt[tid] = ti < li ? (int)(li - ti) : 0;
    }
    __syncthreads();
    if (tid == 0) {
        int off = 0, tot = 0;
        for (int i = 0; i < a.B; ++i) {
            if (i < b) off += s_cnt[i];
            tot += s_cnt[i];
        }
        s_off = off;
        s_tot = tot;
        a.row_off[b] = off;
        a.row_cnt[b] = s_cnt[b];
        if (b == 0) {
            *a.n_rows = tot;
            if (tot > 0) *a.steps += 1;                      // a step that began with a live stream
        }
    }
    __syncthreads();
    const int cnt = s_cnt[b], off = s_off;
    if (cnt == 0) return;
    int64_t tb = a.t[b];
    const int t0 = tb < 0 ? 0 : (int)tb;
    for (int i = tid; i < cnt; i += 256) a.rows[off + i] = b * a.chunk + t0 + i;
    const int j4n = a.J / 4;
    for (int i = tid; i < cnt * j4n; i += 256) {
        const int r = i / j4n, j = (i - r * j4n) * 4;
        const f32x4 e = *(const f32x4*)(a.encp + ((int64_t)b * a.chunk + t0 + r) * a.J + j);
        const f32x4 p = *(const f32x4*)(a.pp + (int64_t)b * a.J + j);
        *(f32x4*)(a.act + (int64_t)(off + r) * a.J + j) = (f32x4){tanhf(e.x + p.x), tanhf(e.y + p.y), tanhf(e.z + p.z), tanhf(e.w + p.w)};
    }
}

struct ChunkCtlArgs {
    const float* pmax;
    const int* pidx;
    const int *row_off, *row_cnt;
    int ntiles, B, L, H, blank, n_steps;
    int64_t *token, *t, *count, *frame_count, *hyps;
    const int64_t* lens;
    int64_t hyp_cap, hyp_ld;
    float *h, *c;
    const float *h_new, *c_new;
    uint8_t* done;
    int *n_done, *overflow;
};

// one workgroup per stream: the class of each of its rows (a wavefront per row, torch.argmax's lowest-index rule), then model.py:255-267
// across the lookahead: the first row whose class is not blank emits; the blank rows before it are the frames the reference would have
// stepped over one by one with the same predictor output
__global__ __launch_bounds__(256) void cfm_chunk_control_kernel(const ChunkCtlArgs a) {
    __shared__ int s_k[32];
    __shared__ int s_nb;
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int cnt = a.row_cnt[b], off = a.row_off[b];
    if (cnt == 0) return;                                    // idle or finished: nothing about the stream changes
    for (int r = wave; r < cnt; r += 4) {
        float best = -INFINITY;
        int bi = 0x7fffffff;
        const int64_t base = (int64_t)(off + r) * a.ntiles;
        for (int tl = lane; tl < a.ntiles; tl += 64) take_better(best, bi, a.pmax[base + tl], a.pidx[base + tl]);
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) take_better(best, bi, __shfl_xor(best, o, 64), __shfl_xor(bi, o, 64));
        if (lane == 0) s_k[r] = bi;
    }
    __syncthreads();
    if (tid == 0) {
        int first = -1;
        for (int r = 0; r < cnt; ++r) {
            if (s_k[r] != a.blank) { first = r; break; }
        }
        int64_t t = a.t[b], fc = a.frame_count[b];
        t = t < 0 ? 0 : t;
        const int64_t end = t + cnt;                         // = min(lens, chunk)
        if (first < 0) {
            t = end;
            fc = 0;
        } else {
            const int k = s_k[first];
            const int64_t n = a.count[b];
            if (n < a.hyp_cap) a.hyps[(int64_t)b * a.hyp_ld + n] = k;
            else *a.overflow = 1;                            // the caller sizes the buffer; never the last slot again
            a.count[b] = n + 1;
            a.token[b] = k;
            fc = (first == 0 ? fc : 0) + 1;
            t += first;
            if (fc >= a.n_steps) { t += 1; fc = 0; }
        }
        a.t[b] = t;
        a.frame_count[b] = fc;
        if (t >= end) {
            a.done[b] = 1;
            atomicAdd(a.n_done, 1);
        }
        s_nb = first >= 0 ? 1 : 0;
    }
    __syncthreads();
    if (s_nb) commit_state(a, b, tid);
}

int chunk_check(const cfm_greedy_chunk_desc* d, const char* who) {
    if (int rc = check_common(d, who)) return rc;
    CFM_CHECK_ARG(d->chunk >= 1 && d->chunk <= 32 && d->D % 16 == 0 && d->E > 0 && d->H > 0 && d->P > 0 && d->J > 0 && d->D > 0 && d->Vp > 0 && d->hyp_cap >= 0 &&
                      d->hyp_ld >= d->hyp_cap,
                  "%s: chunk <= 32, sizes positive, D a multiple of 16, 0 <= hyp_cap <= hyp_ld (chunk=%d E=%d H=%d P=%d J=%d D=%d Vp=%d hyp_cap=%lld hyp_ld=%lld)", who,
                  d->chunk, d->E, d->H, d->P, d->J, d->D, d->Vp, (long long)d->hyp_cap, (long long)d->hyp_ld);
    CFM_CHECK_ARG(d->ef_w && d->ef_b && d->pp && d->rows && d->row_off && d->row_cnt && d->n_rows && d->steps && d->overflow, "%s: null pointer", who);
    return 0;
}

}  // namespace

extern "C" int cfm_greedy_chunk_begin(const cfm_greedy_chunk_desc* d, cfm_stream_t stream) {
    if (int rc = chunk_check(d, "cfm_greedy_chunk_begin")) return rc;
    CFM_CHECK_ARG(d->enc, "cfm_greedy_chunk_begin: no encoder output");
    hipStream_t s = (hipStream_t)stream;
    MTileArgs a = {};
    a.W = d->ef_w; a.bias = d->ef_b; a.x = d->enc; a.ldx = d->D; a.M = d->B * d->chunk; a.N = d->J; a.K = d->D; a.out = d->enc_proj; a.ld_out = d->J;
    if (int rc = launch_mtile<0>(a, s, "greedy_chunk_enc_ffn")) return rc;
    ChunkBeginArgs g;
    g.token = d->token; g.t = d->t; g.frame_count = d->frame_count; g.lens = d->lens; g.h = d->h; g.c = d->c; g.done = d->done; g.n_done = d->n_done;
    g.steps = d->steps; g.B = d->B; g.L = d->L; g.H = d->H; g.blank = d->blank; g.carry = d->carry;
    CfmProfScope prof("greedy_chunk_begin", s, 0.0, 0.0);
    CFM_LAUNCH(cfm_chunk_begin_kernel, dim3((unsigned)d->B), dim3(256), 0, s, g);
    return cfm_launch_status("cfm_greedy_chunk_begin");
}

extern "C" int cfm_greedy_chunk_step(const cfm_greedy_chunk_desc* d, cfm_stream_t stream) {
    if (int rc = chunk_check(d, "cfm_greedy_chunk_step")) return rc;
    hipStream_t s = (hipStream_t)stream;
    const int B = d->B, H = d->H;
    if (int rc = enqueue_predictor(d, d->n_done, s, "cfm_greedy_chunk_step")) return rc;
    {
        SkinnyArgs a = {};
        a.W = d->pf_w; a.bias = d->pf_b; a.B = B; a.N = d->J; a.K = a.K1 = d->P; a.x1 = d->pred; a.ld1 = d->P; a.out = d->pp; a.ld_out = d->J; a.n_done = d->n_done;
        if (int rc = launch_skinny<0>(a, s, "greedy_chunk_pred_ffn")) return rc;
    }
    {
        ChunkRowsArgs r;
        r.encp = d->enc_proj; r.pp = d->pp; r.t = d->t; r.lens = d->lens; r.act = d->act; r.rows = d->rows; r.row_off = d->row_off; r.row_cnt = d->row_cnt;
        r.n_rows = d->n_rows; r.steps = d->steps; r.B = B; r.chunk = d->chunk; r.J = d->J;
        CfmProfScope prof("greedy_chunk_rows", s, 0.0, (double)B * d->chunk * d->J * 8);
        CFM_LAUNCH(cfm_chunk_rows_kernel, dim3((unsigned)B), dim3(256), 0, s, r);
        if (int rc = cfm_launch_status("cfm_greedy_chunk_step (rows)")) return rc;
    }
    {
        MTileArgs a = {};
        a.W = d->out_w; a.bias = d->out_b; a.x = d->act; a.ldx = d->J; a.M = B * d->chunk; a.n_rows = d->n_rows; a.N = d->Vp; a.K = d->J; a.pmax = d->pmax; a.pidx = d->pidx;
        if (int rc = launch_mtile<1>(a, s, "greedy_chunk_joint_out")) return rc;
    }
    ChunkCtlArgs c;
    c.pmax = d->pmax; c.pidx = d->pidx; c.row_off = d->row_off; c.row_cnt = d->row_cnt; c.ntiles = d->Vp / 16; c.B = B; c.L = d->L; c.H = H; c.blank = d->blank;
    c.n_steps = d->n_steps; c.token = d->token; c.t = d->t; c.count = d->count; c.frame_count = d->frame_count; c.hyps = d->hyps; c.lens = d->lens;
    c.hyp_cap = d->hyp_cap; c.hyp_ld = d->hyp_ld; c.h = d->h; c.c = d->c; c.h_new = d->h_new; c.c_new = d->c_new; c.done = d->done; c.n_done = d->n_done;
    c.overflow = d->overflow;
    CfmProfScope prof("greedy_chunk_control", s, 0.0, (double)B * d->chunk * (d->Vp / 16) * 8);
    CFM_LAUNCH(cfm_chunk_control_kernel, dim3((unsigned)B), dim3(256), 0, s, c);
    return cfm_launch_status("cfm_greedy_chunk_step (control)");
}

// ---------------------------------------------------------------------------------------------------------------------------------------
// RNN-T beam search (cfm_rnnt_beam_begin / cfm_rnnt_beam_step): n-best lists from the transducer head; the algorithm is stated once, in
// float64, in tests/rnnt_beam_ref.py.  The hypotheses are ROWS of the skinny products: utterance b's `beam` slots are rows b * beam + j,
// R = B * beam <= 64 in all; the live hypotheses of an utterance sit in its first slots in rank order, the other slots are dead (live = 0):
// they run through the products on stale, valid inputs and are never candidates.  All live hypotheses of an utterance have the same
// alignment length t + len, so one step advances every utterance by one lattice diagonal.  One step, L + 5 launches (7 for L = 2; the
// greedy step has 6):
//
//   pred    the predictor stage over R rows (enqueue_predictor; the token gather is per row)
//   act     tanh(enc_proj[row / beam, t_row] + pred_ffn(pred))                       (cfm_skinny_kernel<2> with enc_div = beam)
//   logits  z = act . Wout^T + bout, [R, Vp]; the pad columns V..Vp carry bias -inf  (cfm_skinny_kernel<0>)
//   topk    cfm_ctc_topk over the R rows as R one-frame items, `live` as their lengths (a dead row costs nothing), the V real classes,
//           k = beam + 1: lse and the k best log-probabilities, the lower class first among equal values.  One of them may be the blank, so
//           the other `beam` are the row's best non-blank classes; the blank's own log-probability is logits[blank] - lse
//   ctl     one workgroup per utterance, thread (j, e) = candidate e of parent slot j: e = 0 the blank (t + 1, fc = 0, the unchanged
//           predictor input), e = 1 .. beam the extension by the parent's e-th best non-blank class (not offered at fc == max_symbols or
//           len == max_len).  An extension whose string is the string of a live slot q -- (length, last token, 64-bit hash) equal, as in
//           cfm_ctc_prefix_beam_kernel -- is folded into q's blank candidate with logaddexp and leaves (at equal alignment length no other
//           two candidates can be the same string, and at most one extension meets a given q: its parent is q's string less the last token).
//           Every candidate counts those that rank before it (score; then parent slot, blank before extension, class: c_key; a merged
//           candidate has the smaller key of its sources); rank < beam is kept.  Thread 0 then walks the <= beam kept candidates in rank
//           order: those with t == n enter the finished set F (global memory between the steps, best first, at most beam), the others get
//           the next free live slot unless F is full and their score is below F's worst.  The candidates write their slots' scalars and
//           trie nodes; all threads copy the slots' LSTM states.  An utterance whose live set is empty writes its n-best list and counts in
//           n_done; from then on its workgroup returns at once, and when n_done == B so do the launches before it.
//
// State reorder: a new slot takes (h, c) from its parent slot -- the candidates (h_new, c_new) of this step when it extended, the
// parent's own state when it took the blank -- and the slots of an utterance read each other's state, so it cannot be done in place: h and c
// are two buffers [2, L, R, H], a step reads [parity] and its control launch writes [parity ^ 1].  parity is the caller's (it alternates
// 0, 1, 0, ... from cfm_rnnt_beam_begin on; the steps after the last live one change nothing, so a captured graph of an even number of
// steps keeps it).  No launch of its own: the control workgroup copies at most beam * L * H * 2 floats.
//
// Identity by hash: unequal strings of equal length and last token collide with probability 2^-64 per comparison; a step makes at most
// beam^3 <= 3375 comparisons per utterance, so ~2e-16 per step -- 1e-11 for 64 rows over 1 000 steps, far below what f32 rounding of the
// scores does to the comparison anyway.
//
// Trie: a kept extension of step s in live slot i becomes node 1 + s * beam + i of its utterance ((parent, token) pairs, node 0 the empty
// string); s < T + max_len + 1, so beam (T + max_len + 1) + 1 nodes per utterance (cfm_rnnt_beam_nodes).
// ---------------------------------------------------------------------------------------------------------------------------------------
namespace {

constexpr int RB_W = 16;                                    // candidate slots per parent: the blank and up to 15 extensions

__device__ __forceinline__ uint64_t beam_hash(uint64_t h, int c) {       // ctc_decode.hip's prefix_hash: splitmix64's finaliser per token
    uint64_t z = h + 0x9E3779B97F4A7C15ull * (uint64_t)(unsigned)(c + 1);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

__device__ __forceinline__ float logaddexp_acc(float a, float b) {       // full-precision expf / log1pf: the scores are compared with float64
    const float m = fmaxf(a, b);
    if (m == -INFINITY) return -INFINITY;
    return m + log1pf(expf(-fabsf(a - b)));
}

struct BeamArgs {
    const int64_t* lens;
    int64_t *token, *t, *hash;
    int *fc, *len, *node, *parent, *ext, *live;
    float* score;
    float *h, *c;                // [2, L, R, H]
    const float *h_new, *c_new;  // [L, R, H]
    const float* logits;         // [R, Vp]
    const int* topk_idx;         // [R, k]
    const float *topk_logp, *lse;
    int* nodes;
    float* fin_score;
    int *fin_node, *fin_len, *n_fin, *step;
    uint8_t* done;
    int* n_done;
    int64_t* nbest_tokens;
    int* nbest_len;
    float* nbest_score;
    int B, T, L, H, Vp, beam, blank, max_symbols, max_len, len_by_frames, parity;
};

__device__ __forceinline__ int64_t beam_nodes_per_utt(int T, int max_len, int beam) { return (int64_t)beam * ((int64_t)T + max_len + 1) + 1; }

// what the streaming entry points (cfm_rnnt_beam_stream_*, at the end of the file) add per stream
struct BeamStreamArgs : BeamArgs {
    int* avail;                  // [B] encoder frames fed so far
    uint8_t *final, *paused;     // [B] the utterance has ended (n = avail); the stream waits for frames
};

// utterance b's empty hypothesis in slot 0, zero LSTM state in both buffers, no finished entry; idle (no frames): that is the result
__device__ __forceinline__ void beam_empty_hyp(const BeamArgs& a, int b, int tid, bool idle) {
    const int K = a.beam, R = a.B * K;
    if (tid < K) {
        const int r = b * K + tid;
        a.token[r] = a.blank; a.t[r] = 0; a.hash[r] = 0;
        a.fc[r] = 0; a.len[r] = 0; a.node[r] = 0; a.parent[r] = r; a.ext[r] = 0;
        a.live[r] = (tid == 0 && !idle) ? 1 : 0;
        a.score[r] = tid == 0 ? 0.f : -INFINITY;
        a.fin_score[r] = -INFINITY; a.fin_node[r] = 0; a.fin_len[r] = 0;
        a.nbest_len[r] = 0;
        a.nbest_score[r] = (tid == 0 && idle) ? 0.f : -INFINITY;
    }
    if (tid == 0) {
        a.n_fin[b] = 0;
        a.step[b] = 0;
        a.done[b] = idle ? 1 : 0;
        int* nodes = a.nodes + beam_nodes_per_utt(a.T, a.max_len, K) * 2 * b;
        nodes[0] = -1; nodes[1] = -1;
    }
    const int KH = K * a.H;
    for (int i = tid; i < 2 * a.L * KH; i += 256) {
        const int pl = i / KH, x = i - pl * KH;             // (buffer, layer), (slot, unit)
        const int64_t o = ((int64_t)pl * R + (int64_t)b * K) * a.H + x;
        a.h[o] = 0.f;
        a.c[o] = 0.f;
    }
}

// one workgroup per utterance: the empty hypothesis in slot 0, zero LSTM state in both buffers, no finished entry; n == 0: the result
__global__ __launch_bounds__(256) void cfm_rnnt_beam_begin_kernel(const BeamArgs a) {
    const int b = blockIdx.x, tid = threadIdx.x;
    beam_empty_hyp(a, b, tid, a.lens[b] <= 0);
    if (tid == 0 && b == 0) {
        int n = 0;
        for (int i = 0; i < a.B; ++i) n += a.lens[i] <= 0 ? 1 : 0;
        *a.n_done = n;
    }
}

// STREAM (cfm_rnnt_beam_stream_step): n is known only once `final` is set -- until then nothing finishes; a paused stream carries its
// live slots' LSTM state to the other buffer and changes nothing else; the step that leaves a live hypothesis within one frame of
// `avail` pauses the stream and counts it in n_done (which there counts the streams that are done OR paused)
template <bool STREAM>
__global__ __launch_bounds__(256) void cfm_rnnt_beam_control_kernel(const std::conditional_t<STREAM, BeamStreamArgs, BeamArgs> a) {
    __shared__ float c_score[256];
    __shared__ unsigned c_key[256];
    __shared__ int slot_of[256];                            // the new live slot of a candidate, -1: none
    __shared__ float m_score[RB_W];                         // the extension folded into slot q's blank candidate
    __shared__ unsigned m_key[RB_W];
    __shared__ int kept[RB_W], k_fin[RB_W], k_node[RB_W], k_len[RB_W];   // by rank: candidate, finished?, the string's node and length
    __shared__ float k_score[RB_W];
    __shared__ float f_score[RB_W];                         // F, best first
    __shared__ int f_node[RB_W], f_len[RB_W];
    __shared__ int new_par[RB_W], new_ext[RB_W];            // by new slot
    __shared__ int new_t[RB_W];                             // STREAM: the new slots' frames
    __shared__ int s_nkept, s_nlive, s_nfin;
    const int b = blockIdx.x, tid = threadIdx.x, K = a.beam, R = a.B * K, kk = K + 1;
    if (a.done[b]) return;                                  // uniform
    const int LH = a.L * a.H;
    const int64_t buf = (int64_t)a.L * R * a.H;
    const float *h_in = a.h + a.parity * buf, *c_in = a.c + a.parity * buf;
    float *h_out = a.h + (a.parity ^ 1) * buf, *c_out = a.c + (a.parity ^ 1) * buf;
    int n, avail = 0;
    bool fin = true;
    if constexpr (STREAM) {
        if (a.paused[b]) {                                  // uniform.  The reorder below with new_par = identity, new_ext = 0: the next step
            int nl = 0;                                      // reads the other buffer, and so does the step that resumes the stream
            for (int q = 0; q < K; ++q) nl += a.live[b * K + q] != 0 ? 1 : 0;
            for (int i = tid; i < nl * LH; i += 256) {
                const int sl = i / LH, x = i - sl * LH, l = x / a.H, u = x - l * a.H;
                const int64_t o = ((int64_t)l * R + b * K + sl) * a.H + u;
                h_out[o] = h_in[o];
                c_out[o] = c_in[o];
            }
            return;
        }
        avail = a.avail[b];
        fin = a.final[b] != 0;
        n = fin ? (avail < a.T ? avail : a.T) : 0x7fffffff;  // not final: no candidate finishes (the pause rule keeps every t < avail)
    } else {
        int64_t n64 = a.lens[b];
        n = n64 < a.T ? (int)n64 : a.T;
    }
    const int max_len = a.len_by_frames && n < a.max_len ? n : a.max_len;   // the most tokens of a hypothesis of this utterance
    const int stp = a.step[b];
    const bool overrun = stp >= a.T + a.max_len + 1;        // cannot happen (a step adds one to t + len); would run past the node buffer
    const int j = tid >> 4, e = tid & 15;
    const int row = b * K + (j < K ? j : 0);
    const bool par_live = j < K && e <= K && !overrun && a.live[row] != 0;
    int64_t pt = 0;
    int pfc = 0, plen = 0, pnode = 0, ptok = 0, cls = -1, merge_into = -1;
    uint64_t phash = 0, xh = 0;
    float sc = -INFINITY;
    unsigned key = 0xffffffffu;
    if (par_live) {
        pt = a.t[row]; pfc = a.fc[row]; plen = a.len[row]; pnode = a.node[row]; ptok = (int)a.token[row]; phash = (uint64_t)a.hash[row];
        const float pscore = a.score[row];
        if (e == 0) {
            sc = pscore + (a.logits[(int64_t)row * a.Vp + a.blank] - a.lse[row]);
            key = (unsigned)(2 * j) << 20;
        } else if (pfc < a.max_symbols && plen < max_len) {
            const int* ix = a.topk_idx + (int64_t)row * kk;
            int pb = kk;                                    // where the blank stands among the k best, k: not among them
            for (int q = kk - 1; q >= 0; --q) pb = ix[q] == a.blank ? q : pb;
            const int pos = (e - 1) < pb ? e - 1 : e;       // the e-th best non-blank class; pos <= beam < k
            cls = ix[pos];
            sc = pscore + a.topk_logp[(int64_t)row * kk + pos];
            key = ((unsigned)(2 * j + 1) << 20) | (unsigned)cls;
            xh = beam_hash(phash, cls);
            for (int q = 0; q < K; ++q) {
                const int rq = b * K + q;
                if (a.live[rq] != 0 && a.len[rq] == plen + 1 && (int)a.token[rq] == cls && (uint64_t)a.hash[rq] == xh) merge_into = q;
            }
        }
    }
    if (tid < RB_W) { m_score[tid] = -INFINITY; m_key[tid] = 0xffffffffu; }
    if (tid == 0) s_nkept = 0;
    __syncthreads();
    if (merge_into >= 0) {                                  // at most one extension per slot
        m_score[merge_into] = sc;
        m_key[merge_into] = key;
        sc = -INFINITY;
        key = 0xffffffffu;
    }
    __syncthreads();
    if (par_live && e == 0) {
        sc = logaddexp_acc(sc, m_score[j]);
        key = min(key, m_key[j]);
    }
    c_score[tid] = sc;
    c_key[tid] = key;
    slot_of[tid] = -1;
    __syncthreads();
    if (key != 0xffffffffu) {
        int rank = 0;
        for (int q = 0; q < K; ++q) {
            for (int x = 0; x <= K; ++x) {
                const float s = c_score[q * RB_W + x];
                const unsigned kq = c_key[q * RB_W + x];
                rank += (kq != 0xffffffffu && (s > sc || (s == sc && kq < key))) ? 1 : 0;
            }
        }
        if (rank < K) {
            kept[rank] = tid;
            k_score[rank] = sc;
            k_fin[rank] = (e == 0 && pt + 1 >= n) ? 1 : 0;
            k_node[rank] = pnode;
            k_len[rank] = plen;
            atomicAdd(&s_nkept, 1);
        }
    }
    __syncthreads();
    if (tid == 0) {                                         // <= beam kept candidates in rank order: F, the prune, the new live slots
        int nf = a.n_fin[b], nl = 0;
        int order[RB_W];
        for (int i = 0; i < nf; ++i) { f_score[i] = a.fin_score[b * K + i]; f_node[i] = a.fin_node[b * K + i]; f_len[i] = a.fin_len[b * K + i]; }
        const int nk = s_nkept < K ? s_nkept : K;
        for (int r = 0; r < nk; ++r) {
            if (!k_fin[r]) { order[nl++] = r; continue; }
            int p = nf;
            while (p > 0 && f_score[p - 1] < k_score[r]) --p;       // behind the entries of the same score
            if (p >= K) continue;
            for (int i = (nf < K ? nf : K - 1); i > p; --i) { f_score[i] = f_score[i - 1]; f_node[i] = f_node[i - 1]; f_len[i] = f_len[i - 1]; }
            f_score[p] = k_score[r]; f_node[p] = k_node[r]; f_len[p] = k_len[r];
            nf = nf < K ? nf + 1 : K;
        }
        int nlive = 0;
        for (int i = 0; i < nl; ++i) {
            if (nf == K && k_score[order[i]] < f_score[K - 1]) continue;   // scores only fall: it cannot enter F any more
            slot_of[kept[order[i]]] = nlive++;
        }
        for (int i = 0; i < nf; ++i) { a.fin_score[b * K + i] = f_score[i]; a.fin_node[b * K + i] = f_node[i]; a.fin_len[b * K + i] = f_len[i]; }
        a.n_fin[b] = nf;
        a.step[b] = stp + 1;
        s_nlive = nlive;
        s_nfin = nf;
    }
    __syncthreads();
    const int slot = slot_of[tid], nl = s_nlive;
    if (slot >= 0) {
        const int nr = b * K + slot;
        if (e == 0) {
            a.t[nr] = pt + 1; a.fc[nr] = 0; a.len[nr] = plen; a.hash[nr] = (int64_t)phash; a.token[nr] = ptok; a.node[nr] = pnode;
        } else {
            int* nodes = a.nodes + beam_nodes_per_utt(a.T, a.max_len, K) * 2 * b;
            const int id = 1 + stp * K + slot;
            nodes[2 * id] = pnode;
            nodes[2 * id + 1] = cls;
            a.t[nr] = pt; a.fc[nr] = pfc + 1; a.len[nr] = plen + 1; a.hash[nr] = (int64_t)xh; a.token[nr] = cls; a.node[nr] = id;
        }
        a.score[nr] = sc;
        a.parent[nr] = row;
        a.ext[nr] = e != 0 ? 1 : 0;
        a.live[nr] = 1;
        new_par[slot] = j;
        new_ext[slot] = e != 0 ? 1 : 0;
        if constexpr (STREAM) new_t[slot] = (int)pt + (e == 0 ? 1 : 0);
    }
    if (tid < K && tid >= nl) a.live[b * K + tid] = 0;
    __syncthreads();
    // the new slots' LSTM states, into the other buffer
    for (int i = tid; i < nl * LH; i += 256) {
        const int sl = i / LH, x = i - sl * LH, l = x / a.H, u = x - l * a.H;
        const int64_t src = ((int64_t)l * R + b * K + new_par[sl]) * a.H + u, dst = ((int64_t)l * R + b * K + sl) * a.H + u;
        h_out[dst] = new_ext[sl] ? a.h_new[src] : h_in[src];
        c_out[dst] = new_ext[sl] ? a.c_new[src] : c_in[src];
    }
    if (nl > 0) {                                           // uniform
        if constexpr (STREAM) {
            if (tid == 0 && !fin) {                          // the next step is permitted only with every live t <= avail - 2
                int mt = 0;
                for (int q = 0; q < nl; ++q) mt = new_t[q] > mt ? new_t[q] : mt;
                if (mt > avail - 2) {
                    a.paused[b] = 1;
                    atomicAdd(a.n_done, 1);
                }
            }
        }
        return;
    }
    // the live set is empty: the utterance is done, F is its n-best list (the strings by walking the parent links back)
    if (tid < K) {
        const int64_t o = (int64_t)b * K + tid;
        if (tid < s_nfin) {
            const int* nodes = a.nodes + beam_nodes_per_utt(a.T, a.max_len, K) * 2 * b;
            const int len = f_len[tid];
            a.nbest_len[o] = len;
            a.nbest_score[o] = f_score[tid];
            int node = f_node[tid];
            for (int pos = len - 1; pos >= 0; --pos) {
                a.nbest_tokens[o * a.max_len + pos] = nodes[2 * node + 1];
                node = nodes[2 * node];
            }
        } else {
            a.nbest_len[o] = 0;
            a.nbest_score[o] = -INFINITY;
        }
    }
    if (tid == 0) {
        a.done[b] = 1;
        atomicAdd(a.n_done, 1);
    }
}

// what enqueue_predictor reads of a descriptor, over the R rows
struct BeamRows {
    const float* embed;
    const float* const* lstm_w;
    const float* const* lstm_b;
    const float *proj_w, *proj_b;
    const int64_t* token;
    const float *h, *c;
    float *h_new, *c_new, *pred;
    int B, L, E, H, P;
};

int beam_check(const cfm_rnnt_beam_desc* d, const char* who) {
    CFM_CHECK_ARG(d, "%s: null descriptor", who);
    CFM_CHECK_ARG(d->beam >= 1 && d->beam <= 15 && d->B > 0 && (int64_t)d->B * d->beam <= 64, "%s: 1 <= beam <= 15 and B * beam <= 64 rows (B=%d beam=%d)", who, d->B,
                  d->beam);
    CFM_CHECK_ARG(d->T > 0 && d->L >= 1 && d->L <= 4 && d->E > 0 && d->H > 0 && d->P > 0 && d->J > 0 && d->E % 16 == 0 && d->H % 16 == 0 && d->P % 16 == 0 &&
                      d->J % 16 == 0 && d->Vp % 16 == 0 && d->V > 0 && d->V <= d->Vp && d->V <= (1 << 20),
                  "%s: T > 0, <= 4 LSTM layers, sizes multiples of 16, V <= Vp, V <= 2^20 (T=%d L=%d E=%d H=%d P=%d J=%d V=%d Vp=%d)", who, d->T, d->L, d->E, d->H, d->P,
                  d->J, d->V, d->Vp);
    CFM_CHECK_ARG(d->beam + 1 <= d->V && d->blank >= 0 && d->blank < d->V, "%s: beam + 1 <= V classes, blank in [0, V) (beam=%d V=%d blank=%d)", who, d->beam, d->V,
                  d->blank);
    CFM_CHECK_ARG(d->max_symbols >= 1 && d->max_len >= 0 && d->parity >= 0 && d->parity <= 1, "%s: max_symbols >= 1, max_len >= 0, parity 0 or 1 (%d, %d, %d)", who,
                  d->max_symbols, d->max_len, d->parity);
    CFM_CHECK_ARG((int64_t)d->beam * ((int64_t)d->T + d->max_len + 1) < (1ll << 30), "%s: beam * (T + max_len + 1) nodes per utterance exceed 2^30", who);
    CFM_CHECK_ARG(d->n_nodes >= cfm_rnnt_beam_nodes(d->B, d->T, d->max_len, d->beam), "%s: node buffer of %lld nodes, %lld needed", who, (long long)d->n_nodes,
                  (long long)cfm_rnnt_beam_nodes(d->B, d->T, d->max_len, d->beam));
    CFM_CHECK_ARG(d->embed && d->proj_w && d->proj_b && d->pf_w && d->pf_b && d->out_w && d->out_b && d->enc_proj && d->lens && d->token && d->t && d->hash && d->fc &&
                      d->len && d->node && d->parent && d->ext && d->live && d->score && d->h && d->c && d->h_new && d->c_new && d->pred && d->act && d->logits &&
                      d->topk_idx && d->topk_logp && d->lse && d->nodes && d->fin_score && d->fin_node && d->fin_len && d->n_fin && d->step && d->done && d->n_done &&
                      d->nbest_tokens && d->nbest_len && d->nbest_score,
                  "%s: null pointer", who);
    return 0;
}

BeamArgs beam_args(const cfm_rnnt_beam_desc* d) {
    BeamArgs a;
    a.lens = d->lens; a.token = d->token; a.t = d->t; a.hash = d->hash; a.fc = d->fc; a.len = d->len; a.node = d->node; a.parent = d->parent; a.ext = d->ext;
    a.live = d->live; a.score = d->score; a.h = d->h; a.c = d->c; a.h_new = d->h_new; a.c_new = d->c_new; a.logits = d->logits; a.topk_idx = d->topk_idx;
    a.topk_logp = d->topk_logp; a.lse = d->lse; a.nodes = d->nodes; a.fin_score = d->fin_score; a.fin_node = d->fin_node; a.fin_len = d->fin_len; a.n_fin = d->n_fin;
    a.step = d->step; a.done = d->done; a.n_done = d->n_done; a.nbest_tokens = d->nbest_tokens; a.nbest_len = d->nbest_len; a.nbest_score = d->nbest_score;
    a.B = d->B; a.T = d->T; a.L = d->L; a.H = d->H; a.Vp = d->Vp; a.beam = d->beam; a.blank = d->blank; a.max_symbols = d->max_symbols; a.max_len = d->max_len; a.len_by_frames = d->len_by_frames;
    a.parity = d->parity;
    return a;
}

}  // namespace

extern "C" int64_t cfm_rnnt_beam_nodes(int32_t B, int32_t T, int32_t max_len, int32_t beam) {
    return (int64_t)B * ((int64_t)beam * ((int64_t)T + max_len + 1) + 1);
}

extern "C" int cfm_rnnt_beam_begin(const cfm_rnnt_beam_desc* d, cfm_stream_t stream) {
    if (int rc = beam_check(d, "cfm_rnnt_beam_begin")) return rc;
    hipStream_t s = (hipStream_t)stream;
    const BeamArgs a = beam_args(d);
    CfmProfScope prof("rnnt_beam_begin", s, 0.0, 0.0);
    CFM_LAUNCH(cfm_rnnt_beam_begin_kernel, dim3((unsigned)d->B), dim3(256), 0, s, a);
    return cfm_launch_status("cfm_rnnt_beam_begin");
}

namespace {

// the launches of one step on the rows of d; the control kernel's arguments are the caller's (offline or streaming)
template <bool STREAM, class Args>
int beam_step_launches(const cfm_rnnt_beam_desc* d, const Args& c, cfm_stream_t stream, const char* who) {
    hipStream_t s = (hipStream_t)stream;
    const int R = d->B * d->beam, k = d->beam + 1;
    const int64_t buf = (int64_t)d->L * R * d->H;
    BeamRows rows;
    rows.embed = d->embed; rows.lstm_w = d->lstm_w; rows.lstm_b = d->lstm_b; rows.proj_w = d->proj_w; rows.proj_b = d->proj_b; rows.token = d->token;
    rows.h = d->h + d->parity * buf; rows.c = d->c + d->parity * buf; rows.h_new = d->h_new; rows.c_new = d->c_new; rows.pred = d->pred;
    rows.B = R; rows.L = d->L; rows.E = d->E; rows.H = d->H; rows.P = d->P;
    if (int rc = enqueue_predictor(&rows, d->n_done, s, who, d->B)) return rc;
    {
        SkinnyArgs a = {};
        a.W = d->pf_w; a.bias = d->pf_b; a.B = R; a.N = d->J; a.K = a.K1 = d->P; a.x1 = d->pred; a.ld1 = d->P; a.out = d->act; a.ld_out = d->J; a.enc = d->enc_proj;
        a.t_idx = d->t; a.T = d->T; a.enc_div = d->beam; a.n_done = d->n_done; a.done_at = d->B;
        if (int rc = launch_skinny<2>(a, s, "rnnt_beam_joint_in")) return rc;
    }
    {
        SkinnyArgs a = {};
        a.W = d->out_w; a.bias = d->out_b; a.B = R; a.N = d->Vp; a.K = a.K1 = d->J; a.x1 = d->act; a.ld1 = d->J; a.out = d->logits; a.ld_out = d->Vp;
        a.n_done = d->n_done; a.done_at = d->B;
        if (int rc = launch_skinny<0>(a, s, "rnnt_beam_joint_out")) return rc;
    }
    if (int rc = cfm_ctc_topk(d->logits, d->Vp, R, 1, d->V, d->live, k, d->topk_idx, d->topk_logp, d->lse, stream)) return rc;
    CfmProfScope prof(STREAM ? "rnnt_beam_stream_control" : "rnnt_beam_control", s, 0.0, (double)R * (k * 8 + 64));
    CFM_LAUNCH((cfm_rnnt_beam_control_kernel<STREAM>), dim3((unsigned)d->B), dim3(256), 0, s, c);
    return cfm_launch_status(who);
}

}  // namespace

extern "C" int cfm_rnnt_beam_step(const cfm_rnnt_beam_desc* d, cfm_stream_t stream) {
    if (int rc = beam_check(d, "cfm_rnnt_beam_step")) return rc;
    return beam_step_launches<false>(d, beam_args(d), stream, "cfm_rnnt_beam_step");
}

// ---------------------------------------------------------------------------------------------------------------------------------------
// Streaming RNN-T beam search (cfm_rnnt_beam_stream_reset / _feed / _step / _report): the search above on frames that arrive in pieces;
// the algorithm is stated in tests/rnnt_beam_ref_stream.py.  enc_proj [B, max_frames, J] fills as frames arrive (avail[b] rows are valid);
// a stream whose utterance has not ended (`final` not set) steps only while every live hypothesis has t <= avail - 2, else it is PAUSED:
// after a permitted step every t <= avail - 1 < n for whatever n the utterance turns out to have, so no candidate that should have
// finished is missed and no live hypothesis waits at t == n -- the steps taken, the live sets and the result are the offline search's.
// n_done counts the streams that are done or paused ("idle"): when it reaches B the launches before the control kernel return at once.
//
// State parity: a paused stream resumes, and must find (h, c) in the buffer the resuming step reads.  Its control workgroup copies its
// live slots' state from buffer `parity` to the other one on every step (the reorder with the identity for parents); a decode runs
// whole replays of an even number of steps from parity 0, so whichever step paused the stream, buffer 0 holds its state at the next
// decode.  The predictor launches are the offline ones.
//
// Reads at the frontier: paused and dead rows still run through rnnt_beam_joint_in on stale, valid inputs.  cfm_skinny_kernel<2> reads
// enc_proj[row / beam, min(t, T - 1)] with T = max_frames, inside [B, max_frames, J] whatever t holds; a row that is read for a result is
// live in a stream that steps, hence t <= avail - 1: rows >= avail (not yet written) reach only rows whose outputs the control kernel
// does not read.
// ---------------------------------------------------------------------------------------------------------------------------------------
namespace {

struct StreamFeedArgs {
    const float* chunk_proj;     // [B, chunk, J]
    float* enc_proj;             // [B, T, J]
    const int64_t* lens;         // [B] frames of this chunk
    const uint8_t* feed_final;   // [B] or null
    const int64_t* t;
    int* live;
    int* avail;
    uint8_t *final, *paused, *done;
    int *n_idle, *overflow, *nbest_len;
    float* nbest_score;
    int B, T, J, chunk, beam;
};

// one workgroup per stream: lens[b] projected rows appended at row avail[b] (a ragged destination), avail advanced, final latched, the
// pause rule evaluated again.  avail + lens > max_frames: the overflow flag, nothing about the stream changes.  A done stream ignores feeds.
__global__ __launch_bounds__(256) void cfm_rnnt_beam_stream_feed_kernel(const StreamFeedArgs a) {
    const int b = blockIdx.x, tid = threadIdx.x, K = a.beam;
    if (a.done[b]) return;                                  // uniform
    int64_t n64 = a.lens[b];
    const int n = n64 < 0 ? 0 : (n64 < a.chunk ? (int)n64 : a.chunk);
    const int av = a.avail[b];
    if (av < 0 || av > a.T || n > a.T - av) {               // uniform
        if (tid == 0) *a.overflow = 1;
        return;
    }
    const int j4n = a.J / 4;
    for (int i = tid; i < n * j4n; i += 256) {
        const int r = i / j4n, j = (i - r * j4n) * 4;
        *(f32x4*)(a.enc_proj + ((int64_t)b * a.T + av + r) * a.J + j) = *(const f32x4*)(a.chunk_proj + ((int64_t)b * a.chunk + r) * a.J + j);
    }
    if (tid == 0) {
        const int av2 = av + n;
        const bool fin = a.final[b] != 0 || (a.feed_final && a.feed_final[b] != 0);
        const int was_idle = a.paused[b] != 0 ? 1 : 0;
        int idle;
        a.avail[b] = av2;
        a.final[b] = fin ? 1 : 0;
        if (fin && av2 == 0) {                               // an utterance without frames: the empty hypothesis with score 0 is its result
            a.live[b * K] = 0;
            a.nbest_len[b * K] = 0;
            a.nbest_score[b * K] = 0.f;
            a.done[b] = 1;
            a.paused[b] = 0;
            idle = 1;
        } else {
            int64_t mt = 0;
            for (int q = 0; q < K; ++q) {
                if (a.live[b * K + q] != 0) mt = a.t[b * K + q] > mt ? a.t[b * K + q] : mt;
            }
            idle = (!fin && mt > (int64_t)av2 - 2) ? 1 : 0;
            a.paused[b] = (uint8_t)idle;
        }
        if (idle != was_idle) atomicAdd(a.n_idle, idle - was_idle);
    }
}

struct StreamResetArgs {
    BeamArgs a;
    const uint8_t* mask;         // [B] or null (every stream)
    int* avail;
    uint8_t *final, *paused;
    int *best_len, *stable_len;
    float* best_score;
};

// cfm_rnnt_beam_begin_kernel's work for the masked streams: the empty hypothesis, no frames, not final, not done -- and paused, since
// nothing can step without frames
__global__ __launch_bounds__(256) void cfm_rnnt_beam_stream_reset_kernel(const StreamResetArgs r) {
    const int b = blockIdx.x, tid = threadIdx.x;
    if (b == 0 && tid == 0) {                               // the idle count: a masked stream is idle after this launch, the others are not written by it
        int n = 0;
        for (int i = 0; i < r.a.B; ++i) n += (!r.mask || r.mask[i] || r.a.done[i] != 0 || r.paused[i] != 0) ? 1 : 0;
        *r.a.n_done = n;
    }
    if (r.mask && !r.mask[b]) return;                       // uniform
    beam_empty_hyp(r.a, b, tid, false);
    if (tid == 0) {
        r.avail[b] = 0;
        r.final[b] = 0;
        r.paused[b] = 1;
        r.best_len[b] = 0;
        r.stable_len[b] = 0;
        r.best_score[b] = 0.f;
    }
}

struct StreamReportArgs {
    const int *live, *len, *node, *nodes;
    const float* score;
    const uint8_t* done;
    int64_t* best_tokens;        // [B, max_len]
    int *best_len, *stable_len;
    float* best_score;
    int B, T, max_len, beam;
};

// one workgroup (its first wavefront) per stream that is not done: the best live hypothesis (slot 0: the live slots are in rank order)
// and the length of the longest common prefix, BY TOKENS, of the live hypotheses' strings: lane j walks slot j's string up the trie, first
// to the shallowest live length, then all in lockstep comparing tokens until the node ids coincide (equal nodes have equal ancestors).
// The common prefix only grows and is a prefix of every later best hypothesis, so best_tokens below the previous stable length are
// already there: the backtrace stops at it.
__global__ __launch_bounds__(64) void cfm_rnnt_beam_stream_report_kernel(const StreamReportArgs a) {
    const int b = blockIdx.x, lane = threadIdx.x, K = a.beam;
    if (a.done[b]) return;                                  // uniform: the n-best list is the result
    const int* nodes = a.nodes + beam_nodes_per_utt(a.T, a.max_len, K) * 2 * b;
    const bool lv = lane < K && a.live[b * K + lane] != 0;
    if (!__any(lv)) return;                                 // cannot happen: a stream that is not done has a live hypothesis
    const int len0 = a.len[b * K], node0 = a.node[b * K];  // slot 0 is live
    int len = lv ? a.len[b * K + lane] : len0, node = lv ? a.node[b * K + lane] : node0;   // the other lanes mirror slot 0
    int lmin = len;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const int x = __shfl_xor(lmin, o, 64); lmin = x < lmin ? x : lmin; }
    for (int d = len; d > lmin; --d) node = nodes[2 * node];
    int stable = lmin;
    for (int d = lmin; d >= 1; --d) {
        if (__all(node == __shfl(node, 0, 64))) break;      // uniform
        const int tok = nodes[2 * node + 1];
        if (__any(tok != __shfl(tok, 0, 64))) stable = d - 1;
        node = nodes[2 * node];
    }
    if (lane == 0) {
        int prev = a.stable_len[b];
        prev = prev < 0 ? 0 : (prev < len0 ? prev : len0);
        int nd = node0;
        for (int pos = len0 - 1; pos >= prev; --pos) {
            a.best_tokens[(int64_t)b * a.max_len + pos] = nodes[2 * nd + 1];
            nd = nodes[2 * nd];
        }
        a.best_len[b] = len0;
        a.best_score[b] = a.score[b * K];
        a.stable_len[b] = stable;
    }
}

int stream_check(const cfm_rnnt_beam_stream_desc* d, const char* who) {
    CFM_CHECK_ARG(d, "%s: null descriptor", who);
    if (int rc = beam_check(&d->beam, who)) return rc;
    CFM_CHECK_ARG(d->beam.len_by_frames == 0, "%s: max_len is explicit in streaming (len_by_frames = %d)", who, d->beam.len_by_frames);
    CFM_CHECK_ARG(d->chunk >= 1 && d->D > 0 && d->D % 16 == 0, "%s: chunk >= 1, D a positive multiple of 16 (chunk=%d D=%d)", who, d->chunk, d->D);
    CFM_CHECK_ARG(d->ef_w && d->ef_b && d->chunk_proj && d->avail && d->final && d->paused && d->overflow && d->best_tokens && d->best_len && d->best_score &&
                      d->stable_len,
                  "%s: null pointer", who);
    return 0;
}

BeamStreamArgs stream_args(const cfm_rnnt_beam_stream_desc* d) {
    BeamStreamArgs a;
    static_cast<BeamArgs&>(a) = beam_args(&d->beam);
    a.avail = d->avail; a.final = d->final; a.paused = d->paused;
    return a;
}

}  // namespace

extern "C" int cfm_rnnt_beam_stream_reset(const cfm_rnnt_beam_stream_desc* d, const uint8_t* mask, cfm_stream_t stream) {
    if (int rc = stream_check(d, "cfm_rnnt_beam_stream_reset")) return rc;
    hipStream_t s = (hipStream_t)stream;
    StreamResetArgs r;
    r.a = beam_args(&d->beam); r.mask = mask; r.avail = d->avail; r.final = d->final; r.paused = d->paused; r.best_len = d->best_len; r.stable_len = d->stable_len;
    r.best_score = d->best_score;
    CfmProfScope prof("rnnt_beam_stream_reset", s, 0.0, 0.0);
    CFM_LAUNCH(cfm_rnnt_beam_stream_reset_kernel, dim3((unsigned)d->beam.B), dim3(256), 0, s, r);
    return cfm_launch_status("cfm_rnnt_beam_stream_reset");
}

extern "C" int cfm_rnnt_beam_stream_feed(const cfm_rnnt_beam_stream_desc* d, cfm_stream_t stream) {
    if (int rc = stream_check(d, "cfm_rnnt_beam_stream_feed")) return rc;
    CFM_CHECK_ARG(d->enc, "cfm_rnnt_beam_stream_feed: no encoder output");
    hipStream_t s = (hipStream_t)stream;
    const cfm_rnnt_beam_desc* o = &d->beam;
    MTileArgs m = {};
    m.W = d->ef_w; m.bias = d->ef_b; m.x = d->enc; m.ldx = d->D; m.M = o->B * d->chunk; m.N = o->J; m.K = d->D; m.out = d->chunk_proj; m.ld_out = o->J;
    if (int rc = launch_mtile<0>(m, s, "rnnt_beam_stream_enc_ffn")) return rc;
    StreamFeedArgs f;
    f.chunk_proj = d->chunk_proj; f.enc_proj = const_cast<float*>(o->enc_proj); f.lens = o->lens; f.feed_final = d->feed_final; f.t = o->t; f.live = o->live;
    f.avail = d->avail; f.final = d->final; f.paused = d->paused; f.done = o->done; f.n_idle = o->n_done; f.overflow = d->overflow; f.nbest_len = o->nbest_len;
    f.nbest_score = o->nbest_score; f.B = o->B; f.T = o->T; f.J = o->J; f.chunk = d->chunk; f.beam = o->beam;
    CfmProfScope prof("rnnt_beam_stream_feed", s, 0.0, (double)o->B * d->chunk * o->J * 8);
    CFM_LAUNCH(cfm_rnnt_beam_stream_feed_kernel, dim3((unsigned)o->B), dim3(256), 0, s, f);
    return cfm_launch_status("cfm_rnnt_beam_stream_feed");
}

extern "C" int cfm_rnnt_beam_stream_step(const cfm_rnnt_beam_stream_desc* d, cfm_stream_t stream) {
    if (int rc = stream_check(d, "cfm_rnnt_beam_stream_step")) return rc;
    return beam_step_launches<true>(&d->beam, stream_args(d), stream, "cfm_rnnt_beam_stream_step");
}

extern "C" int cfm_rnnt_beam_stream_report(const cfm_rnnt_beam_stream_desc* d, cfm_stream_t stream) {
    if (int rc = stream_check(d, "cfm_rnnt_beam_stream_report")) return rc;
    hipStream_t s = (hipStream_t)stream;
    const cfm_rnnt_beam_desc* o = &d->beam;
    StreamReportArgs a;
    a.live = o->live; a.len = o->len; a.node = o->node; a.nodes = o->nodes; a.score = o->score; a.done = o->done; a.best_tokens = d->best_tokens;
    a.best_len = d->best_len; a.stable_len = d->stable_len; a.best_score = d->best_score; a.B = o->B; a.T = o->T; a.max_len = o->max_len; a.beam = o->beam;
    CfmProfScope prof("rnnt_beam_stream_report", s, 0.0, 0.0);
    CFM_LAUNCH(cfm_rnnt_beam_stream_report_kernel, dim3((unsigned)o->B), dim3(64), 0, s, a);
    return cfm_launch_status("cfm_rnnt_beam_stream_report");
}
