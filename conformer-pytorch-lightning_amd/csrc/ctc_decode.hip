// ctc_decode.hip -- CTC decoding on top of the vocabulary projection (gfx950): per-frame top-k, best-path collapse, prefix beam search.
//
// The logits [B, T, V] (f32, row stride ld, pad columns V..ld never read) come from cfm_gemm exactly as for cfm_ctc_nll; nothing of size
// rows x V is written again.  Three launches, each usable on its own:
//   topk    one wavefront per frame (b, t < lens[b]), the whole chip busy: lse = log sum_c exp(logits[t, c]) (16-byte loads, max-shifted,
//           f32, the same two passes as cfm_ctc_rows_kernel), then the k <= 16 largest log-probabilities logits - lse with their classes.
//           Every lane keeps the best KC >= k of the classes it has seen in a sorted register list (an unrolled insertion, entered only when
//           a value beats the list's last); the k winners are then drawn one per round by a wavefront argmax over the lanes' list heads.
//           Order: descending value, the lower class first among equal values (torch.argmax for k = 1, torch.sort(stable, descending) else).
//   greedy  best path: one wavefront per utterance / stream, 64 frames per round.  A frame emits when its class differs from the previous
//           frame's and is not blank; the position of an emission in the hypothesis is count + (emissions in lower lanes), a ballot and a
//           population count instead of a serial loop.  prev [B] carries the last frame's class from call to call: a streaming step.
//   beam    CTC prefix beam search, one workgroup per utterance, serial over frames, the beam in LDS -- see its section below.
#include "cfm_common.h"

namespace {

// (v, i) ranks before (w, j): larger value, or equal value with the lower class
__device__ __forceinline__ bool ranks_before(float v, int i, float w, int j) { return v > w || (v == w && i < j); }

constexpr int TOPK_NT = 256;

// grid = ceil(B*T / 4) workgroups of 4 wavefronts, wavefront = one frame.  KC: capacity of a lane's list (>= k)
template <int KC>
__global__ __launch_bounds__(TOPK_NT) void cfm_ctc_topk_kernel(const float* __restrict__ logits, int64_t ld, int B, int T, int V, const int* __restrict__ lens, int k,
                                                               int* __restrict__ idx, float* __restrict__ logp, float* __restrict__ lse_out) {
    const int lane = threadIdx.x & 63;
    const int64_t row_id = (int64_t)blockIdx.x * (TOPK_NT / 64) + (threadIdx.x >> 6);
    if (row_id >= (int64_t)B * T) return;
    const int b = (int)(row_id / T), t = (int)(row_id % T);
    if (t >= min(max(lens[b], 0), T)) return;              // frames past the utterance: output rows untouched
    const float* row = logits + row_id * ld;
    float bv[KC];
    int bi[KC];
#pragma unroll
    for (int j = 0; j < KC; ++j) { bv[j] = -INFINITY; bi[j] = 0x7fffffff; }
    // a lane sees its classes in ascending order, so a strict '>' keeps the lower class first among equal values
    auto offer = [&](float v, int c) {
        if (v > bv[KC - 1]) {
#pragma unroll
            for (int j = 0; j < KC; ++j) {
                if (v > bv[j]) {
                    const float tv = bv[j]; const int ti = bi[j];
                    bv[j] = v; bi[j] = c;
                    v = tv; c = ti;
                }
            }
        }
    };
    float m = -INFINITY;
    for (int c = lane * 4; c < V; c += 256) {
        if (c + 3 < V) {
            const f32x4 v = *(const f32x4*)(row + c);
            m = fmaxf(fmaxf(m, fmaxf(v.x, v.y)), fmaxf(v.z, v.w));
            offer(v.x, c); offer(v.y, c + 1); offer(v.z, c + 2); offer(v.w, c + 3);
        } else {
            for (int e = c; e < V; ++e) { const float v = row[e]; m = fmaxf(m, v); offer(v, e); }
        }
    }
    m = wave_max(m);
    float sum = 0.f;
    for (int c = lane * 4; c < V; c += 256) {              // second pass over a row that is now in L1/L2
        if (c + 3 < V) {
            const f32x4 v = *(const f32x4*)(row + c);
            sum += (expf(v.x - m) + expf(v.y - m)) + (expf(v.z - m) + expf(v.w - m));
        } else {
            for (int e = c; e < V; ++e) sum += expf(row[e] - m);
        }
    }
    const float lse = m + logf(wave_sum(sum));
    if (lane == 0) lse_out[row_id] = lse;
    float myv = 0.f;
    int myi = 0;
    for (int r = 0; r < k; ++r) {                          // uniform
        float best = bv[0];
        int bc = bi[0];
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const float ov = __shfl_xor(best, o, 64);
            const int oc = __shfl_xor(bc, o, 64);
            if (ranks_before(ov, oc, best, bc)) { best = ov; bc = oc; }
        }
        if (lane == r) { myv = best; myi = bc; }
        if (bi[0] == bc) {                                 // the winner's lane (classes are unique): next of its list moves up
#pragma unroll
            for (int j = 0; j + 1 < KC; ++j) { bv[j] = bv[j + 1]; bi[j] = bi[j + 1]; }
            bv[KC - 1] = -INFINITY; bi[KC - 1] = 0x7fffffff;
        }
    }
    if (lane < k) {
        idx[row_id * k + lane] = myi;
        logp[row_id * k + lane] = myv - lse;
    }
}

struct CtcGreedyArgs {
    const int* idx;
    const float* logp;
    int64_t ldk;
    const int* lens;
    int *prev, *frame_base, *frames, *overflow;
    int64_t *hyps, *count;
    float* token_logp;
    int64_t hyp_cap, hyp_ld;
    int T, blank;
};

// grid = B workgroups of one wavefront
__global__ __launch_bounds__(64) void cfm_ctc_greedy_kernel(const CtcGreedyArgs a) {
    const int b = blockIdx.x, lane = threadIdx.x;
    const int len = min(max(a.lens[b], 0), a.T);
    if (len == 0) return;                                  // idle stream: nothing changes
    int carry = a.prev[b];                                 // class of the frame before this round's first
    int64_t n = a.count[b];
    const int base = a.frame_base ? a.frame_base[b] : 0;
    const uint64_t below = lane == 0 ? 0ull : (~0ull >> (64 - lane));
    for (int t0 = 0; t0 < len; t0 += 64) {
        const int t = t0 + lane;
        const bool live = t < len;
        const int64_t row = ((int64_t)b * a.T + (live ? t : len - 1)) * a.ldk;
        const int cls = a.idx[row];
        const int up = __shfl_up(cls, 1, 64);
        const int before = lane == 0 ? carry : up;
        const bool emit = live && cls != before && cls != a.blank;
        const uint64_t votes = __ballot(emit);
        if (emit) {
            const int64_t pos = n + __popcll(votes & below);
            if (pos < a.hyp_cap) {
                const int64_t o = (int64_t)b * a.hyp_ld + pos;
                a.hyps[o] = cls;
                a.frames[o] = base + t;
                a.token_logp[o] = a.logp[row];
            } else {
                *a.overflow = 1;                           // counted, not stored
            }
        }
        n += __popcll(votes);
        carry = __shfl(cls, min(63, len - 1 - t0), 64);    // the round's last valid frame
    }
    if (lane == 0) {
        a.count[b] = n;
        a.prev[b] = carry;
        if (a.frame_base) a.frame_base[b] = base + len;
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------------
// CTC prefix beam search.  A prefix l of the beam carries pb / pnb, the log-probabilities of all alignments of the frames so far that
// collapse to l and end in blank / in l's last token (-inf: impossible).  Frame t offers its min(k, beam) best classes (c, p) from topk:
//     c == blank        l     : pb  (+)= logaddexp(pb, pnb) + p
//     c == last(l)      l     : pnb (+)= pnb + p ;        l + c : pnb (+)= pb + p
//     otherwise         l + c : pnb (+)= logaddexp(pb, pnb) + p
// ((+)= is logaddexp-accumulation), i.e. per beam entry one "self" candidate and up to `beam` extensions: <= beam (beam + 1) candidates.  A
// candidate whose score logaddexp(pb, pnb) is -inf does not exist.  The best `beam` by score survive; equal scores are ordered by the key
// (rank of the parent in the current beam, self before extension, class), a merged candidate taking the smaller key of its two sources.
//
// Prefix identity is the token string.  Two candidates of a frame can be the same string only as the self candidate of entry r' and an
// extension l_r + c = l_r' (two extensions that are equal have the same parent and class, two entries of a beam differ).  That happens when
// l_r left the beam and was re-created under a new trie node while l_r' stayed, so node identity cannot decide it.  Every entry carries
// (length, last token, a 64-bit hash of the string, extended per token by the splitmix64 finaliser); an extension is merged into the entry
// whose three values equal its own.  Unequal strings of equal length and last token collide with probability 2^-64 per comparison: at most
// beam^3 = 4096 comparisons per frame, ~1e-13 per 8 000-frame batch -- not exact, but far below the f32 rounding that the comparison
// of scores is exposed to anyway.  (Walking both parent chains until they meet is exact and costs O(T) dependent global loads per pair.)
//
// Threads 0..255 own the extension candidates (entry r = tid / 16, class slot j = tid % 16), threads 256..271 the self candidates; three
// barriers per frame: contributions | self candidates | ranking (each live candidate counts those that rank before it, all reading the
// same LDS word at a time) and the next beam, double-buffered.  A surviving extension becomes trie node 1 + t * beam + (its new rank) in
// the caller's node buffer ((parent, token) pairs, node 0 the empty prefix): no counter, and at most beam (T + 1) nodes.  The n-best
// strings are written in order by walking the parent links back from each final entry.
// ---------------------------------------------------------------------------------------------------------------------------------------
constexpr int BEAM_MAX = 16;
constexpr int BEAM_NT = 320;
constexpr int BEAM_SLOTS = BEAM_MAX * BEAM_MAX + BEAM_MAX;  // extension slots [0, 256), self slots [256, 272)

__device__ __forceinline__ uint64_t prefix_hash(uint64_t h, int c) {
    uint64_t z = h + 0x9E3779B97F4A7C15ull * (uint64_t)(unsigned)(c + 1);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

struct BeamEntry {
    int node[BEAM_MAX], last[BEAM_MAX], len[BEAM_MAX];
    float pb[BEAM_MAX], pnb[BEAM_MAX];
    uint64_t hash[BEAM_MAX];
};

struct CtcBeamArgs {
    const int* idx;
    const float* logp;
    const int* lens;
    int* nodes;
    int64_t* nbest_tokens;
    int* nbest_len;
    float* nbest_score;
    int T, k, beam, blank;
};

__global__ __launch_bounds__(BEAM_NT) void cfm_ctc_prefix_beam_kernel(const CtcBeamArgs a) {
    __shared__ BeamEntry ent[2];
    __shared__ float c_score[BEAM_SLOTS];
    __shared__ unsigned c_key[BEAM_SLOTS];
    __shared__ float self_pb[BEAM_MAX], self_pnb[BEAM_MAX], merge_pnb[BEAM_MAX];
    __shared__ unsigned merge_key[BEAM_MAX];
    __shared__ int s_live[2];                               // frame t counts into [t & 1]: the other one is still being read
    const int b = blockIdx.x, tid = threadIdx.x, beam = a.beam, T = a.T, k = a.k, nk = min(k, beam);   // nk classes per frame
    const int len = min(max(a.lens[b], 0), T);
    const bool is_ext = tid < BEAM_MAX * BEAM_MAX, is_self = tid >= BEAM_MAX * BEAM_MAX && tid < BEAM_SLOTS;
    const int r = is_ext ? tid >> 4 : tid - BEAM_MAX * BEAM_MAX, j = tid & 15;
    int* nodes = a.nodes + (int64_t)b * beam * (T + 1) * 2;
    if (tid < BEAM_SLOTS) { c_score[tid] = -INFINITY; c_key[tid] = 0xffffffffu; }
    if (tid < BEAM_MAX) { self_pb[tid] = self_pnb[tid] = merge_pnb[tid] = -INFINITY; merge_key[tid] = 0xffffffffu; }
    if (tid == 0) {
        ent[0].node[0] = 0; ent[0].last[0] = -1; ent[0].len[0] = 0; ent[0].pb[0] = 0.f; ent[0].pnb[0] = -INFINITY; ent[0].hash[0] = 0;
        nodes[0] = -1; nodes[1] = -1;
    }
    int cur = 0, n_live = 1;
    const int64_t frame0 = (int64_t)b * T * k;
    int nc = 0;
    float np = -INFINITY;
    if (is_ext && j < nk && len > 0) { nc = a.idx[frame0 + j]; np = a.logp[frame0 + j]; }
    __syncthreads();
    for (int t = 0; t < len; ++t) {
        const BeamEntry& E = ent[cur];
        BeamEntry& N = ent[cur ^ 1];
        const int c = nc;
        const float p = np;
        if (is_ext && j < nk && t + 1 < len) { nc = a.idx[frame0 + (int64_t)(t + 1) * k + j]; np = a.logp[frame0 + (int64_t)(t + 1) * k + j]; }
        // contributions of (entry r, class slot j)
        float x_pnb = -INFINITY;                            // this thread's extension candidate l_r + c
        unsigned x_key = 0xffffffffu;
        uint64_t x_hash = 0;
        if (is_ext) {
            bool alive = false;
            if (r < n_live && j < nk) {
                const float pb = E.pb[r], pnb = E.pnb[r];
                if (c == a.blank) {
                    self_pb[r] = logaddexp_(pb, pnb) + p;
                } else {
                    if (c == E.last[r]) {
                        self_pnb[r] = pnb + p;
                        x_pnb = pb + p;
                    } else {
                        x_pnb = logaddexp_(pb, pnb) + p;
                    }
                    if (x_pnb > -INFINITY) {
                        x_key = ((unsigned)(2 * r + 1) << 20) | (unsigned)c;
                        x_hash = prefix_hash(E.hash[r], c);
                        const int xl = E.len[r] + 1;
                        int same = -1;
                        for (int q = 0; q < n_live; ++q)
                            if (E.len[q] == xl && E.last[q] == c && E.hash[q] == x_hash) same = q;
                        if (same >= 0) {                    // the string of entry `same`: at most one extension per entry
                            merge_pnb[same] = x_pnb;
                            merge_key[same] = x_key;
                        } else {
                            alive = true;
                        }
                    }
                }
            }
            c_score[tid] = alive ? x_pnb : -INFINITY;
            c_key[tid] = x_key;
            if (!alive) x_pnb = -INFINITY;
        }
        if (tid == 0) s_live[t & 1] = 0;
        __syncthreads();
        // self candidates
        float s_pb = -INFINITY, s_pnb = -INFINITY;
        if (is_self) {
            float sc = -INFINITY;
            unsigned key = 0xffffffffu;
            if (r < n_live) {
                s_pb = self_pb[r];
                s_pnb = logaddexp_(self_pnb[r], merge_pnb[r]);
                sc = logaddexp_(s_pb, s_pnb);
                key = min((unsigned)(2 * r) << 20, merge_key[r]);
            }
            c_score[tid] = sc;
            c_key[tid] = key;
            self_pb[r] = self_pnb[r] = merge_pnb[r] = -INFINITY;
            merge_key[r] = 0xffffffffu;
        }
        __syncthreads();
        // ranking and the next beam
        const float my = tid < BEAM_SLOTS ? c_score[tid] : -INFINITY;
        if (my > -INFINITY) {
            const unsigned mk = c_key[tid];
            int rank = 0;
            for (int q = 0; q < n_live; ++q) {
                for (int e = 0; e < nk; ++e) {
                    const float s = c_score[q * BEAM_MAX + e];
                    rank += (s > my || (s == my && c_key[q * BEAM_MAX + e] < mk)) ? 1 : 0;
                }
                const float s = c_score[BEAM_MAX * BEAM_MAX + q];
                rank += (s > my || (s == my && c_key[BEAM_MAX * BEAM_MAX + q] < mk)) ? 1 : 0;
            }
            if (rank < beam) {
                atomicMax(&s_live[t & 1], rank + 1);
                if (is_self) {
                    N.node[rank] = E.node[r]; N.last[rank] = E.last[r]; N.len[rank] = E.len[r]; N.hash[rank] = E.hash[r];
                    N.pb[rank] = s_pb; N.pnb[rank] = s_pnb;
                } else {
                    const int id = 1 + t * beam + rank;
                    nodes[2 * id] = E.node[r];
                    nodes[2 * id + 1] = c;
                    N.node[rank] = id; N.last[rank] = c; N.len[rank] = E.len[r] + 1; N.hash[rank] = x_hash;
                    N.pb[rank] = -INFINITY; N.pnb[rank] = x_pnb;
                }
            }
        }
        __syncthreads();
        n_live = s_live[t & 1];                                    // >= 1 unless every candidate was impossible
        cur ^= 1;
        if (n_live == 0) break;                             // uniform
    }
    __syncthreads();                                        // the node stores of the last frame, before the walk reads them
    const BeamEntry& E = ent[cur];
    if (tid < beam) {
        const int64_t o = (int64_t)b * beam + tid;
        if (tid < n_live) {
            const int L = E.len[tid];
            a.nbest_len[o] = L;
            a.nbest_score[o] = logaddexp_(E.pb[tid], E.pnb[tid]);
            int node = E.node[tid];
            for (int pos = L - 1; pos >= 0; --pos) {
                a.nbest_tokens[o * T + pos] = nodes[2 * node + 1];
                node = nodes[2 * node];
            }
        } else {
            a.nbest_len[o] = 0;
            a.nbest_score[o] = -INFINITY;
        }
    }
}

}  // namespace

extern "C" int cfm_ctc_topk(const float* logits, int64_t ld, int32_t B, int32_t T, int32_t V, const int32_t* lens, int32_t k, int32_t* idx, float* logp,
                            float* lse, cfm_stream_t stream) {
    CFM_CHECK_ARG(logits && lens && idx && logp && lse, "cfm_ctc_topk: null pointer");
    CFM_CHECK_ARG(B > 0 && T > 0 && V > 0, "cfm_ctc_topk: bad shape B=%d T=%d V=%d", B, T, V);
    CFM_CHECK_ARG(k >= 1 && k <= 16, "cfm_ctc_topk: k=%d outside 1..16", k);
    CFM_CHECK_ARG(k <= V, "cfm_ctc_topk: k=%d exceeds the %d classes", k, V);
    CFM_CHECK_ARG(ld >= V && ld % 4 == 0, "cfm_ctc_topk: row stride %lld must be >= V and a multiple of 4", (long long)ld);
    hipStream_t s = (hipStream_t)stream;
    const int64_t rows = (int64_t)B * T;
    const dim3 grid((unsigned)((rows + TOPK_NT / 64 - 1) / (TOPK_NT / 64)));
    CfmProfScope prof("ctc_topk", s, 0.0, (double)rows * V * 4);
    if (k == 1) CFM_LAUNCH(cfm_ctc_topk_kernel<1>, grid, dim3(TOPK_NT), 0, s, logits, ld, B, T, V, lens, k, idx, logp, lse);
    else if (k <= 4) CFM_LAUNCH(cfm_ctc_topk_kernel<4>, grid, dim3(TOPK_NT), 0, s, logits, ld, B, T, V, lens, k, idx, logp, lse);
    else CFM_LAUNCH(cfm_ctc_topk_kernel<16>, grid, dim3(TOPK_NT), 0, s, logits, ld, B, T, V, lens, k, idx, logp, lse);
    return cfm_launch_status("cfm_ctc_topk");
}

extern "C" int cfm_ctc_greedy(const cfm_ctc_greedy_desc* d, cfm_stream_t stream) {
    CFM_CHECK_ARG(d, "cfm_ctc_greedy: null descriptor");
    CFM_CHECK_ARG(d->idx && d->logp && d->lens && d->prev && d->hyps && d->count && d->frames && d->token_logp && d->overflow, "cfm_ctc_greedy: null pointer");
    CFM_CHECK_ARG(d->B > 0 && d->T > 0 && d->V > 0 && d->ld_k >= 1, "cfm_ctc_greedy: bad shape B=%d T=%d V=%d ld_k=%lld", d->B, d->T, d->V, (long long)d->ld_k);
    CFM_CHECK_ARG(d->blank >= 0 && d->blank < d->V, "cfm_ctc_greedy: blank=%d outside [0, %d)", d->blank, d->V);
    CFM_CHECK_ARG(d->hyp_cap >= 0 && d->hyp_ld >= d->hyp_cap, "cfm_ctc_greedy: 0 <= hyp_cap <= hyp_ld (hyp_cap=%lld hyp_ld=%lld)", (long long)d->hyp_cap,
                  (long long)d->hyp_ld);
    CtcGreedyArgs a;
    a.idx = d->idx; a.logp = d->logp; a.ldk = d->ld_k; a.lens = d->lens; a.prev = d->prev; a.frame_base = d->frame_base; a.frames = d->frames;
    a.overflow = d->overflow; a.hyps = d->hyps; a.count = d->count; a.token_logp = d->token_logp; a.hyp_cap = d->hyp_cap; a.hyp_ld = d->hyp_ld;
    a.T = d->T; a.blank = d->blank;
    hipStream_t s = (hipStream_t)stream;
    CfmProfScope prof("ctc_greedy", s, 0.0, (double)d->B * d->T * 8);
    CFM_LAUNCH(cfm_ctc_greedy_kernel, dim3((unsigned)d->B), dim3(64), 0, s, a);
    return cfm_launch_status("cfm_ctc_greedy");
}

extern "C" int64_t cfm_ctc_beam_nodes(int32_t B, int32_t T, int32_t beam) { return (int64_t)B * beam * ((int64_t)T + 1); }

extern "C" int cfm_ctc_prefix_beam(const cfm_ctc_beam_desc* d, cfm_stream_t stream) {
    CFM_CHECK_ARG(d, "cfm_ctc_prefix_beam: null descriptor");
    CFM_CHECK_ARG(d->idx && d->logp && d->lens && d->nodes && d->nbest_tokens && d->nbest_len && d->nbest_score, "cfm_ctc_prefix_beam: null pointer");
    CFM_CHECK_ARG(d->B > 0 && d->T > 0 && d->V > 0 && d->V <= (1 << 20), "cfm_ctc_prefix_beam: bad shape B=%d T=%d V=%d (V <= 2^20)", d->B, d->T, d->V);
    CFM_CHECK_ARG(d->beam >= 1 && d->beam <= BEAM_MAX, "cfm_ctc_prefix_beam: beam=%d outside 1..%d", d->beam, BEAM_MAX);
    CFM_CHECK_ARG(d->k >= 1 && d->k <= 16 && d->k <= d->V, "cfm_ctc_prefix_beam: k=%d outside 1..min(16, V=%d)", d->k, d->V);
    CFM_CHECK_ARG(d->blank >= 0 && d->blank < d->V, "cfm_ctc_prefix_beam: blank=%d outside [0, %d)", d->blank, d->V);
    CFM_CHECK_ARG((int64_t)d->beam * ((int64_t)d->T + 1) < (1ll << 30), "cfm_ctc_prefix_beam: beam * (T + 1) nodes per utterance exceed 2^30");
    CFM_CHECK_ARG(d->n_nodes >= cfm_ctc_beam_nodes(d->B, d->T, d->beam), "cfm_ctc_prefix_beam: node buffer of %lld nodes, B * beam * (T + 1) = %lld needed",
                  (long long)d->n_nodes, (long long)cfm_ctc_beam_nodes(d->B, d->T, d->beam));
    CtcBeamArgs a;
    a.idx = d->idx; a.logp = d->logp; a.lens = d->lens; a.nodes = d->nodes; a.nbest_tokens = d->nbest_tokens; a.nbest_len = d->nbest_len;
    a.nbest_score = d->nbest_score; a.T = d->T; a.k = d->k; a.beam = d->beam; a.blank = d->blank;
    hipStream_t s = (hipStream_t)stream;
    CfmProfScope prof("ctc_prefix_beam", s, 0.0, (double)d->B * d->T * d->k * 8);
    CFM_LAUNCH(cfm_ctc_prefix_beam_kernel, dim3((unsigned)d->B), dim3(BEAM_NT), 0, s, a);
    return cfm_launch_status("cfm_ctc_prefix_beam");
}
