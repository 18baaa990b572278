// ctc_prefix.hip -- the CTC prefix scorer of joint CTC/attention decoding (include/cfm.h states the three entry points;
// tests/ctc_prefix_ref.py the definition in float64; decoder.JointBeamSearch the host side).
//
//   cfm_ctc_logprob_t      once per search: log_softmax of the CTC head's logits, written CLASS-major [B, V, Tp], so that a candidate's column is
//                          contiguous in t.  One workgroup per (utterance, 32 frames): a wavefront per frame for the max-shifted log-sum-exp, then
//                          64-class tiles turned through LDS.
//   cfm_ctc_prefix_score   once per step: one workgroup per beam row.  phi (both forms) is built once per row in LDS; a wavefront per candidate
//                          reduces psi(g.c) = init (+) (+)_t (phi[t-1] + x[t, c]) with lanes over t -- maximum, then the shifted sum, both in a fixed
//                          order --; the P offers are ranked in LDS and the K best written.
//   cfm_ctc_prefix_advance once per step, after the prune: one lane per kept row runs the recursion of (parent, token) over t and writes the
//                          other half of the double-buffered state.
// No atomics, plain C++ and vector stores: the same input gives the same bits.
#include "cfm_common.h"

#define LPT_FRAMES 32                                          // frames per workgroup of cfm_ctc_logprob_t
#define LPT_CLS 64                                             // classes per LDS tile
#define PFX_WAVES 4

// ---------------------------------------------------------------------------------------------------------------- what both step kernels share
// phi[t] of a candidate: the alignments of g to frames 0..t after which the candidate may start -- those ending in blank when it repeats g's
// last token, all of them otherwise; and the first-frame term, which only the empty prefix has.
static __device__ __forceinline__ float pfx_phi(float gn, float gb, bool same) { return same ? gb : logaddexp_(gn, gb); }
static __device__ __forceinline__ float pfx_init(const float* __restrict__ xc, bool empty) { return empty ? xc[0] : -INFINITY; }

static __device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// ------------------------------------------------------------------------------------------------------------------------------- logprob_t
__global__ __launch_bounds__(256) void cfm_ctc_logprob_t_kernel(const float* __restrict__ logits, int64_t ld, int T, int V, int Tp, const int32_t* __restrict__ lens,
                                                                float* __restrict__ x) {
    __shared__ float tile[LPT_CLS][LPT_FRAMES + 1];
    __shared__ float f_max[LPT_FRAMES], f_log[LPT_FRAMES];
    const int b = blockIdx.y, t0 = blockIdx.x * LPT_FRAMES, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int n = clampi(lens[b], 0, T);
    if (t0 >= n) return;                                       // uniform per workgroup
    const int nt = min(LPT_FRAMES, n - t0);
    for (int f = wave; f < nt; f += 4) {                       // a wavefront per frame: maximum, then the shifted sum
        const float* row = logits + ((int64_t)b * T + t0 + f) * ld;
        float m = -INFINITY;
        for (int c = lane; c < V; c += 64) m = fmaxf(m, row[c]);
        m = wave_max(m);
        float s = 0.f;
        for (int c = lane; c < V; c += 64) s += expf(row[c] - m);
        s = wave_sum(s);
        if (lane == 0) f_max[f] = m, f_log[f] = logf(s);
    }
    __syncthreads();
    const int tc = threadIdx.x >> 5, tf = threadIdx.x & 31;
    for (int c0 = 0; c0 < V; c0 += LPT_CLS) {
        for (int f = wave; f < nt; f += 4)                     // read class-contiguous ...
            if (c0 + lane < V) tile[lane][f] = logits[((int64_t)b * T + t0 + f) * ld + c0 + lane];
        __syncthreads();
        for (int cc = tc; cc < LPT_CLS; cc += 8)               // ... write frame-contiguous: (v - max) - log(sum), two roundings at the result's magnitude
            if (c0 + cc < V && tf < nt) x[((int64_t)b * V + c0 + cc) * Tp + t0 + tf] = (tile[cc][tf] - f_max[tf]) - f_log[tf];
        __syncthreads();
    }
}

extern "C" int cfm_ctc_logprob_t(const float* logits, int64_t ld, int32_t B, int32_t T, int32_t V, const int32_t* lens, float* x, cfm_stream_t stream) {
    CFM_CHECK_ARG(logits && lens && x, "cfm_ctc_logprob_t: null pointer");
    CFM_CHECK_ARG(B >= 1 && B <= 65535 && T >= 1 && T <= 2048 && V >= 1, "cfm_ctc_logprob_t: bad shape B=%d T=%d V=%d (1 <= T <= 2048)", B, T, V);
    CFM_CHECK_ARG(ld >= V && ld % 4 == 0, "cfm_ctc_logprob_t: row stride %lld must be >= V and a multiple of 4", (long long)ld);
    CFM_CHECK_ARG((((uintptr_t)logits | (uintptr_t)x) & 15) == 0, "cfm_ctc_logprob_t: logits and x must be 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    const int Tp = (T + 3) & ~3;
    CfmProfScope prof("ctc_logprob_t", s, 0.0, (double)B * T * V * 12.0);
    CFM_LAUNCH(cfm_ctc_logprob_t_kernel, dim3((unsigned)((T + LPT_FRAMES - 1) / LPT_FRAMES), (unsigned)B), dim3(256), 0, s, logits, ld, T, V, Tp, lens, x);
    return cfm_launch_status("cfm_ctc_logprob_t");
}

// ------------------------------------------------------------------------------------------------------------------------------------ score
__global__ __launch_bounds__(PFX_WAVES * 64) void cfm_ctc_prefix_score_kernel(cfm_ctc_prefix_desc d, int Tp) {
    extern __shared__ __attribute__((aligned(16))) float pfx_smem[];
    __shared__ float o_key[16], o_psi[16];
    __shared__ int o_cls[16];
    float* phi_d = pfx_smem;                                   // [Tp] gamma_n (+) gamma_b: a candidate other than the last token
    float* phi_s = pfx_smem + Tp;                              // [Tp] gamma_b alone: the candidate repeats the last token
    const int r = blockIdx.x, K = d.K, P = d.P, b = r / K, t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int n = clampi(d.lens[b], 0, d.T);
    if (d.done[b] || d.finished[r] || n == 0) {                // uniform per workgroup: nothing the prune reads, and no NaN
        if (t < K) d.out_idx[(int64_t)r * K + t] = d.eos, d.out_logp[(int64_t)r * K + t] = -INFINITY, d.cand_psi[(int64_t)r * K + t] = -INFINITY;
        return;
    }
    const int R = d.B * K;
    const float* st = d.state + ((int64_t)(d.step[b] & 1) * R + r) * Tp * 2;
    const int last = d.token[r];
    const bool empty = d.hlen[r] <= 0;
    const float psi_g = d.psi[r];
    for (int tt = t; tt < n; tt += PFX_WAVES * 64) {
        const f32x2 g = *(const f32x2*)(st + 2 * tt);
        phi_d[tt] = pfx_phi(g.x, g.y, false), phi_s[tt] = pfx_phi(g.x, g.y, true);
    }
    __syncthreads();

    for (int j = wave; j < P; j += PFX_WAVES) {                // a wavefront per candidate
        const int c = clampi(d.topk_idx[(int64_t)r * P + j], 0, d.V - 1);
        float psi_c;
        if (c == d.blank) {
            psi_c = -INFINITY;
        } else if (c == d.eos) {
            psi_c = phi_d[n - 1];                              // the CTC likelihood of g itself
        } else {
            const float* xc = d.x + ((int64_t)b * d.V + c) * Tp;
            const float* ph = c == last ? phi_s : phi_d;
            const float init = pfx_init(xc, empty);
            float m = init;
            for (int tt = 1 + lane; tt < n; tt += 64) m = fmaxf(m, ph[tt - 1] + xc[tt]);
            m = wave_max(m);
            psi_c = -INFINITY;
            if (m != -INFINITY) {                              // uniform per wavefront
                float s = lane == 0 ? __expf(init - m) : 0.f;
                for (int tt = 1 + lane; tt < n; tt += 64) s += __expf((ph[tt - 1] + xc[tt]) - m);
                psi_c = m + __logf(wave_sum(s));
            }
        }
        if (lane == 0) {
            const float delta = (psi_c == -INFINITY || psi_g == -INFINITY) ? -INFINITY : psi_c - psi_g;
            const float att = d.ctc_weight < 1.f ? (1.f - d.ctc_weight) * d.topk_logp[(int64_t)r * P + j] : 0.f;
            float key = delta == -INFINITY ? -INFINITY : att + d.ctc_weight * delta;
            if (key != key) key = -INFINITY;                   // a NaN attention score ranks last, as in the prune
            o_key[j] = key, o_psi[j] = psi_c, o_cls[j] = c;
        }
    }
    __syncthreads();
    if (t < P) {                                               // descending, the lower class first among equal values
        const float key = o_key[t];
        const int cls = o_cls[t];
        int rank = 0;
        for (int m = 0; m < P; ++m) {
            const float km = o_key[m];
            rank += (km > key || (km == key && (o_cls[m] < cls || (o_cls[m] == cls && m < t)))) ? 1 : 0;
        }
        if (rank < K) d.out_idx[(int64_t)r * K + rank] = cls, d.out_logp[(int64_t)r * K + rank] = key, d.cand_psi[(int64_t)r * K + rank] = o_psi[t];
    }
}

static int pfx_check(const cfm_ctc_prefix_desc* d, const char* who) {
    CFM_CHECK_ARG(d, "%s: null descriptor", who);
    CFM_CHECK_ARG(d->K >= 1 && d->K <= d->P && d->P <= 16 && d->P <= d->V, "%s: K=%d P=%d V=%d (1 <= K <= P <= 16, P <= V)", who, d->K, d->P, d->V);
    CFM_CHECK_ARG(d->B >= 1 && (int64_t)d->B * d->K <= 1024 && d->T >= 1 && d->T <= 2048, "%s: B=%d K=%d T=%d (R = B * K <= 1024, 1 <= T <= 2048)", who, d->B, d->K, d->T);
    CFM_CHECK_ARG(d->blank >= 0 && d->blank < d->V && d->eos >= 0 && d->eos < d->V && d->eos != d->blank, "%s: blank=%d and eos=%d must differ and lie in [0, %d)", who,
                  d->blank, d->eos, d->V);
    CFM_CHECK_ARG(d->x && d->state && d->psi && d->token && d->hlen && d->finished && d->step && d->done && d->lens, "%s: null pointer", who);
    CFM_CHECK_ARG((((uintptr_t)d->x | (uintptr_t)d->state) & 15) == 0, "%s: x and state must be 16-byte aligned", who);
    return CFM_OK;
}

extern "C" int cfm_ctc_prefix_score(const cfm_ctc_prefix_desc* d, cfm_stream_t stream) {
    if (int rc = pfx_check(d, "cfm_ctc_prefix_score")) return rc;
    CFM_CHECK_ARG(d->topk_idx && d->topk_logp && d->out_idx && d->out_logp && d->cand_psi, "cfm_ctc_prefix_score: null pointer (topk_idx, topk_logp, out_idx, out_logp, cand_psi)");
    CFM_CHECK_ARG(d->ctc_weight > 0.f && d->ctc_weight <= 1.f, "cfm_ctc_prefix_score: ctc_weight=%g outside (0, 1]", (double)d->ctc_weight);
    hipStream_t s = (hipStream_t)stream;
    const int R = d->B * d->K, Tp = (d->T + 3) & ~3;
    CfmProfScope prof("ctc_prefix_score", s, 0.0, (double)R * d->T * (8.0 + 4.0 * d->P));
    CFM_LAUNCH(cfm_ctc_prefix_score_kernel, dim3((unsigned)R), dim3(PFX_WAVES * 64), (size_t)2 * Tp * sizeof(float), s, *d, Tp);
    return cfm_launch_status("cfm_ctc_prefix_score");
}

// ---------------------------------------------------------------------------------------------------------------------------------- advance
// Runs after the prune: step[b] counts the steps taken, so the half the prune's candidates were scored from is (step[b] + 1) & 1 and the new
// state goes to step[b] & 1 -- the half the next score launch reads.  A row's length is hlen[r] >= 1, its token tokens[r][hlen - 1] = token[r],
// its parent's last token tokens[r][hlen - 2] (the prune has reordered the strings by parent already).
__global__ __launch_bounds__(64) void cfm_ctc_prefix_advance_kernel(cfm_ctc_prefix_desc d, int Tp) {
    const int r = blockIdx.x * 64 + threadIdx.x, K = d.K, R = d.B * K;
    if (r >= R) return;
    const int b = r / K;
    const int n = clampi(d.lens[b], 0, d.T);
    if (d.done[b] || d.finished[r] || n == 0) return;          // never read again: left as it is
    const int i = d.step[b];
    const int p = clampi(d.parent[r], b * K, b * K + K - 1);   // a kept row's parent is a row of its own utterance
    const int c = clampi(d.token[r], 0, d.V - 1);
    const int L = clampi(d.hlen[r], 1, d.Lmax);
    const bool empty = L <= 1;
    const bool same = !empty && d.tokens[(int64_t)r * d.Lmax + L - 2] == c;
    const float* src = d.state + ((int64_t)((i + 1) & 1) * R + p) * Tp * 2;
    float* dst = d.state + ((int64_t)(i & 1) * R + r) * Tp * 2;
    const float* xc = d.x + ((int64_t)b * d.V + c) * Tp;
    const float* xb = d.x + ((int64_t)b * d.V + d.blank) * Tp;
    float gn = c == d.blank ? -INFINITY : pfx_init(xc, empty), gb = -INFINITY, psi = gn;
    *(f32x2*)dst = (f32x2){gn, gb};
    if (c == d.blank) {                                        // no hypothesis ends in blank: impossible from here on
        for (int t = 1; t < n; ++t) *(f32x2*)(dst + 2 * t) = (f32x2){-INFINITY, -INFINITY};
    } else {
#pragma unroll 4
        for (int t = 1; t < n; ++t) {
            const f32x2 g = *(const f32x2*)(src + 2 * (t - 1));
            const float ph = pfx_phi(g.x, g.y, same), xt = xc[t];
            const float both = logaddexp_(gn, gb);
            gn = logaddexp_(gn, ph) + xt;
            gb = both + xb[t];
            psi = logaddexp_(psi, ph + xt);
            *(f32x2*)(dst + 2 * t) = (f32x2){gn, gb};
        }
    }
    d.psi[r] = psi;
}

extern "C" int cfm_ctc_prefix_advance(const cfm_ctc_prefix_desc* d, cfm_stream_t stream) {
    if (int rc = pfx_check(d, "cfm_ctc_prefix_advance")) return rc;
    CFM_CHECK_ARG(d->parent && d->tokens && d->Lmax >= 1, "cfm_ctc_prefix_advance: null pointer (parent, tokens) or Lmax=%d", d->Lmax);
    hipStream_t s = (hipStream_t)stream;
    const int R = d->B * d->K, Tp = (d->T + 3) & ~3;
    CfmProfScope prof("ctc_prefix_advance", s, 0.0, (double)R * d->T * 32.0);
    CFM_LAUNCH(cfm_ctc_prefix_advance_kernel, dim3((unsigned)((R + 63) / 64)), dim3(64), 0, s, *d, Tp);
    return cfm_launch_status("cfm_ctc_prefix_advance");
}
