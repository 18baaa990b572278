// attn_search.hip -- autoregressive beam search with the attention decoder (include/cfm.h states the two entry points;
// tests/attention_search_ref.py the definition; decoder.AttentionBeamSearch the host side).
//
//   cfm_dec_step_attn     one query per (row, head) over a K | V store addressed through a slot table (self-attention: the ancestry of a beam
//                         row, position j's K | V written once and never moved) or a base and a stride (cross-attention over the memory).
//                         One wavefront per (row, head), four per workgroup.  Pass 1: one key per lane, the query in LDS, scores to LDS, wave
//                         maximum.  Pass 2: exp and wave sum.  Pass 3: dk / 4 lanes across a value row, 64 / (dk / 4) keys in flight, the
//                         partial contexts folded through LDS in group order.  This step's own K | V is read from kv_new and stored to its slot.
//   cfm_dec_beam_prune    one workgroup of 256 threads per utterance: thread (p, j) is parent p's j-th offer, ranks itself among the K * K
//                         candidates in LDS, the K best are kept; strings and ancestry are reordered in place, 16 columns at a time (all reads
//                         of a column block before its writes); the next input rows, the done flags and, once, the n-best buffers.
#include "cfm_common.h"

#define SA_WAVES 4
#define SA_RED 256                                             // floats: (64 / (dk / 4)) groups * dk <= 256

// ------------------------------------------------------------------------------------------------------------------------------ step attention
static __device__ __forceinline__ int64_t sa_slot(const cfm_dec_step_attn_desc& d, int r, int j) {
    const int64_t s = d.slot ? (int64_t)d.slot[(int64_t)r * d.slot_ld + j] : (int64_t)(r / d.group) * d.stride + j;
    return s < 0 ? 0 : (s >= d.slots ? d.slots - 1 : s);       // never outside the store, whatever the table holds
}

template <typename T>
__global__ __launch_bounds__(SA_WAVES * 64) void cfm_dec_step_attn_kernel(cfm_dec_step_attn_desc d, float scale) {
    extern __shared__ __attribute__((aligned(16))) float sa_smem[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int dk = d.dk, D = d.H * dk, nchunk = dk >> 2, groups = 64 / nchunk;
    const int capr = (d.cap + 3) & ~3;
    float* qs = sa_smem + (size_t)wave * (dk + capr + SA_RED);  // the query [dk], the scores [cap], the partial contexts [groups][dk]
    float* sc = qs + dk;
    float* red = sc + capr;
    const int item = blockIdx.x * SA_WAVES + wave;
    const bool live = item < d.R * d.H;                        // a wavefront past the end runs along with klen = 0 and writes nothing
    const int r = live ? item / d.H : 0, h = live ? item - r * d.H : 0;
    int klen = 0;
    if (live) klen = min(max(d.klen ? d.klen[r / d.klen_group] : d.step[0] + 1, 0), d.cap);
    const int hoff = h * dk;
    const bool append = d.kv_new != nullptr && klen > 0;
    const int64_t new_row = (int64_t)r * d.ld_new + hoff;       // this step's key in kv_new; its value D further

    if (lane < nchunk && live) {
        *(f32x4*)(qs + 4 * lane) = ld4<T>(d.q, (int64_t)r * d.ldq + hoff + 4 * lane);
        if (append) {                                          // the one store row of this row: head h's slice of K and of V
            const int64_t dst = sa_slot(d, r, klen - 1) * 2 * D + hoff + 4 * lane;
            st4<T>(d.store, dst, ld4<T>(d.kv_new, new_row + 4 * lane));
            st4<T>(d.store, dst + D, ld4<T>(d.kv_new, new_row + D + 4 * lane));
        }
    }
    __syncthreads();

    float m = -INFINITY;
    for (int j = lane; j < klen; j += 64) {
        const bool own = append && j == klen - 1;
        const void* base = own ? d.kv_new : (const void*)d.store;
        const int64_t at = own ? new_row : sa_slot(d, r, j) * 2 * D + hoff;
        float acc = 0.f;
        for (int c = 0; c < nchunk; ++c) {
            const f32x4 kv = ld4<T>(base, at + 4 * c), qv = *(const f32x4*)(qs + 4 * c);
            acc += kv.x * qv.x + kv.y * qv.y + kv.z * qv.z + kv.w * qv.w;
        }
        const float s = acc * scale;
        sc[j] = s;
        m = fmaxf(m, s);
    }
    m = wave_max(m);
    __syncthreads();

    float sum = 0.f;
    for (int j = lane; j < klen; j += 64) {
        const float p = __expf(sc[j] - m);
        sc[j] = p;
        sum += p;
    }
    sum = wave_sum(sum);
    __syncthreads();

    const int g = lane / nchunk, c = lane - g * nchunk;
    if (g < groups) {
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        for (int j = g; j < klen; j += groups) {
            const bool own = append && j == klen - 1;
            const void* base = own ? d.kv_new : (const void*)d.store;
            const int64_t at = (own ? new_row : sa_slot(d, r, j) * 2 * D + hoff) + D;
            const f32x4 v = ld4<T>(base, at + 4 * c);
            const float p = sc[j];
            acc.x += p * v.x, acc.y += p * v.y, acc.z += p * v.z, acc.w += p * v.w;
        }
        *(f32x4*)(red + g * dk + 4 * c) = acc;
    }
    __syncthreads();

    if (lane < nchunk && live) {
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        if (klen > 0) {
            for (int gg = 0; gg < groups; ++gg) {
                const f32x4 v = *(const f32x4*)(red + gg * dk + 4 * lane);
                acc.x += v.x, acc.y += v.y, acc.z += v.z, acc.w += v.w;
            }
            const float inv = 1.f / sum;
            acc.x *= inv, acc.y *= inv, acc.z *= inv, acc.w *= inv;
        }
        st4<T>(d.out, (int64_t)r * d.ldo + hoff + 4 * lane, acc);
    }
}

extern "C" int cfm_dec_step_attn(const cfm_dec_step_attn_desc* d, cfm_stream_t stream) {
    CFM_CHECK_ARG(d, "cfm_dec_step_attn: null descriptor");
    const int64_t D = (int64_t)d->H * d->dk;
    CFM_CHECK_ARG(d->R >= 1 && d->H >= 1 && d->dk >= 4 && d->dk % 4 == 0 && d->dk <= 128 && D % 8 == 0 && (int64_t)d->R * d->H < (int64_t)1 << 31,
                  "cfm_dec_step_attn: bad shape R=%d H=%d dk=%d (dk %% 4 == 0, dk <= 128, D = H * dk a multiple of 8)", d->R, d->H, d->dk);
    CFM_CHECK_ARG(d->io_dtype == CFM_F32 || cfm_is16(d->io_dtype), "cfm_dec_step_attn: io_dtype %d", d->io_dtype);
    CFM_CHECK_ARG(d->q && d->store && d->out && (d->klen || d->step), "cfm_dec_step_attn: null pointer (q, store, out, and klen or step)");
    CFM_CHECK_ARG(d->cap >= 1 && d->cap <= 2048 && d->slots >= 1 && d->klen_group >= 1, "cfm_dec_step_attn: capacity %d outside 1..2048, %lld slots, klen_group %d",
                  d->cap, (long long)d->slots, d->klen_group);
    if (d->slot) {
        CFM_CHECK_ARG(d->slot_ld >= d->cap, "cfm_dec_step_attn: a key count up to the capacity %d does not fit the slot table's %d columns", d->cap, d->slot_ld);
    } else {
        CFM_CHECK_ARG(d->group >= 1 && d->stride >= d->cap && (int64_t)((d->R - 1) / d->group) * d->stride + d->cap <= d->slots,
                      "cfm_dec_step_attn: group=%d stride=%d: a key count up to the capacity %d leaves the owner's rows or the %lld slots", d->group, d->stride, d->cap,
                      (long long)d->slots);
        CFM_CHECK_ARG(!d->kv_new, "cfm_dec_step_attn: kv_new (append) needs the slot table form");
    }
    CFM_CHECK_ARG(d->ldq >= D && d->ldq % 4 == 0 && d->ldo >= D && d->ldo % 4 == 0 && (!d->kv_new || (d->ld_new >= 2 * D && d->ld_new % 4 == 0)),
                  "cfm_dec_step_attn: row strides ldq=%lld ldo=%lld ld_new=%lld (multiples of 4, >= D resp. 2 D)", (long long)d->ldq, (long long)d->ldo, (long long)d->ld_new);
    CFM_CHECK_ARG((((uintptr_t)d->q | (uintptr_t)d->store | (uintptr_t)d->out | (uintptr_t)d->kv_new) & 15) == 0, "cfm_dec_step_attn: q, store, out and kv_new must be 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    const int items = d->R * d->H;
    const size_t lds = (size_t)SA_WAVES * (d->dk + ((d->cap + 3) & ~3) + SA_RED) * sizeof(float);
    const float scale = 1.0f / sqrtf((float)d->dk);
    CfmProfScope prof(d->slot ? "dec_step_attn_self" : "dec_step_attn_cross", s, 4.0 * items * d->dk * d->cap, 2.0 * items * d->dk * d->cap * cfm_elt_size(d->io_dtype));
    const dim3 grid((unsigned)((items + SA_WAVES - 1) / SA_WAVES)), block(SA_WAVES * 64);
    cfm_by_dtype(d->io_dtype, [&](auto tag) { CFM_LAUNCH((cfm_dec_step_attn_kernel<decltype(tag)>), grid, block, lds, s, *d, scale); });
    return cfm_launch_status("cfm_dec_step_attn");
}

// ------------------------------------------------------------------------------------------------------------------------------------ prune
// Rows of a done utterance keep VALID indices for every later step of a captured graph: parent = the row itself, step / klen / tokens / slots
// frozen, x rewritten from the frozen token and position -- so a later step never gathers out of range; what such rows compute is ignored.
// The last slot of such a row is made its own (i * R + row) when the utterance becomes done: siblings share their parent's slot at position i,
// and the frozen rows keep appending at that position.
__global__ __launch_bounds__(256) void cfm_dec_beam_prune_kernel(cfm_dec_beam_prune_desc d, double sqrt_d) {
    __shared__ float c_key[256];
    __shared__ int c_cls[256];
    __shared__ unsigned char c_valid[256];
    __shared__ float k_score[16];
    __shared__ int k_parent[16], k_cls[16], k_fin[16], o_hlen[16], n_hlen[16], n_token[16], n_pos[16];
    const int b = blockIdx.x, t = threadIdx.x, K = d.K, Lmax = d.Lmax, R = d.B * K, row0 = b * K;
    const bool was_done = d.done[b] != 0;
    const int i = d.step[b];

    if (!was_done) {                                           // uniform per workgroup
        const int p = t / K, j = t - p * K;
        bool valid = false;
        float key = -INFINITY;
        int cls = d.eos;
        if (t < K * K) {
            const int row = row0 + p;
            const float ps = d.score[row];
            if (d.finished[row]) {
                valid = j == 0;
                key = ps;
            } else {
                valid = true;
                cls = d.topk_idx[(int64_t)row * d.k_ld + j];
                key = ps + d.topk_logp[(int64_t)row * d.k_ld + j];
            }
            if (key != key) key = -INFINITY;                   // a total order: NaN ranks last
        }
        c_key[t] = key, c_cls[t] = cls, c_valid[t] = valid ? 1 : 0;
        if (t < K) {
            k_score[t] = -INFINITY, k_parent[t] = t, k_cls[t] = d.eos, k_fin[t] = 1;       // an unfilled rank (K <= V: there is none): finished, identity parent
            o_hlen[t] = d.hlen[row0 + t];
        }
        __syncthreads();
        int rank = 0;
        if (valid) {
            for (int m = 0; m < K * K; ++m) {
                if (!c_valid[m]) continue;
                const float km = c_key[m];
                const int pm = m / K;
                rank += (km > key || (km == key && (pm < p || (pm == p && c_cls[m] < cls)))) ? 1 : 0;
            }
        }
        __syncthreads();
        if (valid && rank < K) k_score[rank] = key, k_parent[rank] = p, k_cls[rank] = cls, k_fin[rank] = d.finished[row0 + p] ? 1 : 0;
        __syncthreads();

        // strings and ancestry, columns 0 .. i, by parent, in place: a block of 16 columns is read by everyone before anyone writes it
        const int q = t >> 4, cl = t & 15;
        for (int c0 = 0; c0 <= i; c0 += 16) {
            const int col = c0 + cl;
            const bool mine = q < K && col <= i && col < Lmax;
            int tk = 0, sl = 0;
            if (mine) {
                const int64_t src = (int64_t)(row0 + k_parent[q]) * Lmax + col;
                tk = d.tokens[src], sl = d.slots[src];
            }
            __syncthreads();
            if (mine) {
                const int64_t dst = (int64_t)(row0 + q) * Lmax + col;
                d.tokens[dst] = tk, d.slots[dst] = sl;
            }
        }
        __syncthreads();

        bool all_fin = true;
        for (int qq = 0; qq < K; ++qq) all_fin = all_fin && (k_fin[qq] || k_cls[qq] == d.eos);
        const bool now_done = all_fin || i + 1 >= d.max_len[b];
        if (t < K) {
            const int row = row0 + t, cls = k_cls[t];
            const bool fin = k_fin[t] || cls == d.eos;
            const int hl = o_hlen[k_parent[t]] + ((k_fin[t] || cls == d.eos) ? 0 : 1);
            d.token[row] = cls, d.score[row] = k_score[t], d.finished[row] = fin ? 1 : 0, d.parent[row] = row0 + k_parent[t], d.hlen[row] = hl;
            if (i < Lmax) d.tokens[(int64_t)row * Lmax + i] = cls;
            if (!now_done) {
                d.klen[row] = i + 2;
                if (i + 1 < Lmax) d.slots[(int64_t)row * Lmax + i + 1] = (i + 1) * R + row;
            } else if (i < Lmax) {
                d.slots[(int64_t)row * Lmax + i] = i * R + row;   // frozen at klen = i + 1: later steps append here, so the slot is the row's own, not its parent's
            }
            n_token[t] = cls, n_pos[t] = now_done ? i : i + 1;
            n_hlen[t] = hl;
        }
        __syncthreads();
        if (now_done) {
            if (t < K) {
                const float sc = k_score[t];
                const int len = sc == -INFINITY ? 0 : min(n_hlen[t], Lmax);
                d.nbest_len[row0 + t] = len, d.nbest_score[row0 + t] = sc;
            }
            for (int e = t; e < K * Lmax; e += 256) {           // this workgroup's own writes above are visible after the barrier
                const int qq = e / Lmax, col = e - qq * Lmax;
                const int len = k_score[qq] == -INFINITY ? 0 : min(n_hlen[qq], Lmax);
                if (col < len) d.nbest_tokens[(int64_t)(row0 + qq) * Lmax + col] = d.tokens[(int64_t)(row0 + qq) * Lmax + col];
            }
            if (t == 0) {
                d.done[b] = 1;
                if (atomicAdd(d.n_done, 1) + 1 >= d.B) d.all_done[0] = 1;
            }
        } else if (t == 0) {
            d.step[b] = i + 1;
        }
    } else {
        if (t < K) {
            const int row = row0 + t;
            d.parent[row] = row;
            n_token[t] = d.token[row], n_pos[t] = max(d.klen[row] - 1, 0);
        }
        __syncthreads();
    }
    // the next step's decoder input rows (a done utterance: the same rows again, so that they stay finite)
    for (int e = t; e < K * d.D; e += 256) {
        const int qq = e / d.D, k = e - qq * d.D;
        const int tok = min(max(n_token[qq], 0), d.V - 1);
        d.x[(int64_t)(row0 + qq) * d.D + k] = (float)((double)d.embed[(int64_t)tok * d.D + k] * sqrt_d + (double)d.pe[(int64_t)n_pos[qq] * d.D + k]);
    }
}

extern "C" int cfm_dec_beam_prune(const cfm_dec_beam_prune_desc* d, cfm_stream_t stream) {
    CFM_CHECK_ARG(d, "cfm_dec_beam_prune: null descriptor");
    CFM_CHECK_ARG(d->B >= 1 && d->K >= 1 && d->K <= 16 && d->k_ld >= d->K && d->V >= d->K && d->Lmax >= 1 && d->Lmax <= 1023 && d->D >= 1 &&
                      (int64_t)d->B * d->K <= 1024,
                  "cfm_dec_beam_prune: bad shape B=%d K=%d k_ld=%d V=%d Lmax=%d D=%d (1 <= K <= 16, K <= k_ld, K <= V, Lmax <= 1023, B * K <= 1024)", d->B, d->K, d->k_ld, d->V,
                  d->Lmax, d->D);
    CFM_CHECK_ARG(d->eos >= 0 && d->eos < d->V, "cfm_dec_beam_prune: eos=%d outside the vocabulary of %d", d->eos, d->V);
    CFM_CHECK_ARG(d->topk_idx && d->topk_logp && d->embed && d->pe && d->max_len && d->score && d->token && d->parent && d->finished && d->hlen && d->klen && d->tokens &&
                      d->slots && d->x && d->step && d->done && d->n_done && d->all_done && d->nbest_tokens && d->nbest_len && d->nbest_score,
                  "cfm_dec_beam_prune: null pointer");
    hipStream_t s = (hipStream_t)stream;
    CfmProfScope prof("dec_beam_prune", s, 0.0, (double)d->B * d->K * (d->D * 12.0 + d->Lmax * 16.0));
    CFM_LAUNCH(cfm_dec_beam_prune_kernel, dim3((unsigned)d->B), dim3(256), 0, s, *d, sqrt((double)d->D));
    return cfm_launch_status("cfm_dec_beam_prune");
}
