// rescore.hip -- attention rescoring of n-best lists (include/cfm.h states the three entry points; tests/attention_decoder_ref.py the definition).
//
//   cfm_rescore_prep      one workgroup of 64 threads per decoder position (p, i): the embedding gather * sqrt(D) + pe in double, the target, the
//                         mask row -- for the left and, when asked, the reversed hypothesis.
//   cfm_token_logprob     the hot path: log_softmax(x . W^T + b)[target] per row without the logits.  A workgroup owns 64 rows, staged once in LDS
//                         in W's type; its 8 wavefronts deal the vocabulary out in tiles of 32 classes.  The product is computed TRANSPOSED,
//                         C = W_tile . X^T with 16x16x32 MFMA: C's row (the class) runs along a lane's 4 accumulator registers and its column (the
//                         hypothesis row) is lane & 15, so a lane folds its 8 values of a tile into ITS row's running (max, sum) in registers.  The 4
//                         lanes of a row, then the 8 wavefronts, are combined once at the end, in a fixed order.  The second form (logits given) is
//                         one wavefront per row over stored logits.
//                         The product loop lives in vocab_tile.h: the label-smoothing loss (lsm.hip) runs on the same one.
//   cfm_rescore_combine   one wavefront per utterance, lane n sums hypothesis n's rows in position order and ranks itself among the N.
#include "cfm_common.h"
#include "vocab_tile.h"

// ------------------------------------------------------------------------------------------------------------------------------------- prep
__global__ __launch_bounds__(64) void cfm_rescore_prep_kernel(cfm_rescore_prep_desc d, double sqrt_d) {
    const int Lc = d.Lmax + 1;
    const int p = blockIdx.x / Lc, i = blockIdx.x - p * Lc, lane = threadIdx.x;
    const int nl = d.nlen[p];
    const bool used = nl >= 0 && d.score[p] != -INFINITY;
    const int L = min(nl, d.Lmax), Lcp = used ? L + 1 : 0;
    const bool live = i < Lcp;
    const int32_t* y = d.tokens + (int64_t)p * d.Lmax;
    const int64_t row = (int64_t)p * Lc + i;
    // left: in_i = sos, y_0 ..; tg_i = y_0 .., eos.   reversed: in_i = sos, y_{L-1} ..; tg_i = y_{L-1} .., eos
    int in_l = d.sos, tg_l = -1, in_r = d.sos, tg_r = -1;
    if (live) {
        if (i > 0) in_l = y[i - 1], in_r = y[L - i];
        tg_l = i < L ? y[i] : d.eos;
        tg_r = i < L ? y[L - 1 - i] : d.eos;
    }
    if (lane == 0) {
        d.targets[row] = tg_l;
        if (d.targets_r) d.targets_r[row] = tg_r;
    }
    uint8_t* mrow = d.mask + row * Lc;
    for (int j = lane; j < Lc; j += 64) mrow[j] = (uint8_t)(j <= i && j < Lcp ? 1 : 0);
    const float* pe = d.pe + (int64_t)i * d.D;
    const float* el = d.embed + (int64_t)min(max(in_l, 0), d.V - 1) * d.D;
    float* xl = d.x0 + row * d.D;
    for (int k = lane; k < d.D; k += 64) xl[k] = live ? (float)((double)el[k] * sqrt_d + (double)pe[k]) : 0.f;
    if (d.x0_r) {
        const float* er = d.embed_r + (int64_t)min(max(in_r, 0), d.V - 1) * d.D;
        float* xr = d.x0_r + row * d.D;
        for (int k = lane; k < d.D; k += 64) xr[k] = live ? (float)((double)er[k] * sqrt_d + (double)pe[k]) : 0.f;
    }
}

extern "C" int cfm_rescore_prep(const cfm_rescore_prep_desc* d, cfm_stream_t stream) {
    CFM_CHECK_ARG(d, "cfm_rescore_prep: null descriptor");
    CFM_CHECK_ARG(d->B >= 1 && d->N >= 1 && d->N <= 16 && d->Lmax >= 0 && d->Lmax + 1 <= 1024 && d->D >= 1 && d->V >= 1,
                  "cfm_rescore_prep: bad shape B=%d N=%d Lmax=%d D=%d V=%d (1 <= N <= 16, Lmax + 1 <= 1024)", d->B, d->N, d->Lmax, d->D, d->V);
    CFM_CHECK_ARG((int64_t)d->B * d->N * (d->Lmax + 1) < (int64_t)1 << 31, "cfm_rescore_prep: B * N * (Lmax + 1) exceeds 2^31 positions");
    CFM_CHECK_ARG((d->tokens || d->Lmax == 0) && d->nlen && d->score && d->embed && d->pe && d->x0 && d->targets && d->mask, "cfm_rescore_prep: null pointer");
    CFM_CHECK_ARG(!d->x0_r == !d->targets_r && !d->x0_r == !d->embed_r, "cfm_rescore_prep: x0_r, targets_r and embed_r go together");
    CFM_CHECK_ARG(d->sos >= 0 && d->sos < d->V && d->eos >= 0 && d->eos < d->V, "cfm_rescore_prep: sos=%d eos=%d outside the vocabulary of %d", d->sos, d->eos, d->V);
    hipStream_t s = (hipStream_t)stream;
    const int64_t rows = (int64_t)d->B * d->N * (d->Lmax + 1);
    CfmProfScope prof("rescore_prep", s, 0.0, (double)rows * (d->D * 8.0 * (d->x0_r ? 2 : 1) + d->Lmax + 1));
    CFM_LAUNCH(cfm_rescore_prep_kernel, dim3((unsigned)rows), dim3(64), 0, s, *d, sqrt((double)d->D));
    return cfm_launch_status("cfm_rescore_prep");
}

// ---------------------------------------------------------------------------------------------------------------------------- token logprob
template <typename HT, typename XT>
__global__ __launch_bounds__(TL_WAVES * 64) void cfm_token_logprob_kernel(cfm_token_logprob_desc d) {
    extern __shared__ __attribute__((aligned(16))) unsigned char tl_smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int row0 = blockIdx.x * TL_ROWS;
    const int M = d.M, D = d.D, V = d.V;
    int live = 0;
    if (tid < TL_ROWS) live = row0 + tid < M && d.target[row0 + tid] >= 0;
    if (!__syncthreads_or(live)) {                             // a wholly dead tile: nothing of X, W or bias is read
        if (tid < TL_ROWS && row0 + tid < M) {
            d.logp[row0 + tid] = 0.f;
            if (d.lse) d.lse[row0 + tid] = 0.f;
        }
        return;
    }
    tl_stage_rows<HT, XT>(tl_smem, d.X, d.ldx, row0, M, D, tid);

    const int g = lane >> 4, l15 = lane & 15;
    float mx[4], sm[4], tv[4];
    int tg[4];
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        const int r = row0 + s * 16 + l15;
        tg[s] = r < M ? d.target[r] : -1;
        mx[s] = -INFINITY, sm[s] = 0.f, tv[s] = 0.f;
    }
    tl_tiles<HT>(tl_smem, (const u16*)d.W, d.bias, D, V, wave, TL_WAVES, (V + 31) >> 5, lane, [&](int c0, int s, const float (&v)[8]) {
        tl_fold_lse(mx[s], sm[s], v);
        tl_pick_target(tv[s], tg[s], c0, g, v);
    });
    // the four lanes of a row (g = 0..3): xor 16, then xor 32
#pragma unroll
    for (int s = 0; s < 4; ++s) {
#pragma unroll
        for (int o = 16; o <= 32; o <<= 1) {
            const float m2 = __shfl_xor(mx[s], o, 64), s2 = __shfl_xor(sm[s], o, 64), t2 = __shfl_xor(tv[s], o, 64);
            tl_merge(mx[s], sm[s], m2, s2);
            tv[s] += t2;
        }
    }
    __syncthreads();                                           // every wavefront is done with the row image: its memory now takes the partials
    float* part = (float*)tl_smem;                             // [TL_WAVES][3][TL_ROWS]
    if (g == 0) {
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const int r = s * 16 + l15;
            part[(wave * 3 + 0) * TL_ROWS + r] = mx[s];
            part[(wave * 3 + 1) * TL_ROWS + r] = sm[s];
            part[(wave * 3 + 2) * TL_ROWS + r] = tv[s];
        }
    }
    __syncthreads();
    if (tid < TL_ROWS && row0 + tid < M) {
        float m = part[tid], sum = part[TL_ROWS + tid], val = part[2 * TL_ROWS + tid];
        for (int w = 1; w < TL_WAVES; ++w) {
            tl_merge(m, sum, part[(w * 3 + 0) * TL_ROWS + tid], part[(w * 3 + 1) * TL_ROWS + tid]);
            val += part[(w * 3 + 2) * TL_ROWS + tid];
        }
        const int t = d.target[row0 + tid];
        const float lse = m + logf(sum);
        d.logp[row0 + tid] = t < 0 ? 0.f : t >= V ? __builtin_nanf("") : val - lse;
        if (d.lse) d.lse[row0 + tid] = t < 0 ? 0.f : lse;
    }
}

// The logits form: one wavefront per row, lane j takes classes j, j + 64, ..; the lanes' pairs meet in a xor butterfly (tl_merge is symmetric).
__global__ __launch_bounds__(256) void cfm_token_logprob_logits_kernel(cfm_token_logprob_desc d) {
    const int lane = threadIdx.x & 63;
    const int m = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4 + (threadIdx.x >> 6)));
    if (m >= d.M) return;
    const int t = d.target[m];
    if (t < 0) {
        if (lane == 0) {
            d.logp[m] = 0.f;
            if (d.lse) d.lse[m] = 0.f;
        }
        return;
    }
    const float* row = d.logits + (int64_t)m * d.ld;
    float mx = -INFINITY, sm = 0.f;
    for (int c = lane; c < d.V; c += 64) tl_merge(mx, sm, row[c], 1.f);
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const float m2 = __shfl_xor(mx, o, 64), s2 = __shfl_xor(sm, o, 64);
        tl_merge(mx, sm, m2, s2);
    }
    if (lane == 0) {
        const float lse = mx + logf(sm);
        d.logp[m] = t >= d.V ? __builtin_nanf("") : row[t] - lse;
        if (d.lse) d.lse[m] = lse;
    }
}

extern "C" int cfm_token_logprob(const cfm_token_logprob_desc* d, cfm_stream_t stream) {
    CFM_CHECK_ARG(d, "cfm_token_logprob: null descriptor");
    CFM_CHECK_ARG(d->M >= 1 && d->V >= 1, "cfm_token_logprob: bad shape M=%d V=%d", d->M, d->V);
    CFM_CHECK_ARG(d->target && d->logp, "cfm_token_logprob: null pointer");
    hipStream_t s = (hipStream_t)stream;
    if (d->logits) {
        CFM_CHECK_ARG(d->ld >= d->V, "cfm_token_logprob: logits row stride %lld below V=%d", (long long)d->ld, d->V);
        CfmProfScope prof("token_logprob_logits", s, 0.0, (double)d->M * d->V * 4);
        CFM_LAUNCH(cfm_token_logprob_logits_kernel, dim3((unsigned)((d->M + 3) / 4)), dim3(256), 0, s, *d);
        return cfm_launch_status("cfm_token_logprob (logits)");
    }
    CFM_CHECK_ARG(d->X && d->W && d->bias, "cfm_token_logprob: null pointer (X, W and bias, or logits)");
    CFM_CHECK_ARG(d->D >= 8 && d->D % 8 == 0 && d->D <= TL_MAXD, "cfm_token_logprob: D=%d (a multiple of 8, at most %d)", d->D, TL_MAXD);
    CFM_CHECK_ARG(cfm_is16(d->w_dtype), "cfm_token_logprob: W is bf16 or fp16 (the fp32 mode runs cfm_gemm and the logits form)");
    CFM_CHECK_ARG(d->x_dtype == CFM_F32 || d->x_dtype == d->w_dtype, "cfm_token_logprob: X is f32 or of W's type");
    const int xa = d->x_dtype == CFM_F32 ? 4 : 8;
    CFM_CHECK_ARG(d->ldx >= d->D && d->ldx % xa == 0 && ((uintptr_t)d->X & 15) == 0 && ((uintptr_t)d->W & 15) == 0,
                  "cfm_token_logprob: X and W must be 16-byte aligned, ldx=%lld a multiple of %d and >= D", (long long)d->ldx, xa);
    const size_t lds = tl_lds_bytes(d->D, 3);
    const dim3 grid((unsigned)((d->M + TL_ROWS - 1) / TL_ROWS)), block(TL_WAVES * 64);
    CfmProfScope prof("token_logprob", s, 2.0 * d->M * d->V * d->D, (double)d->M * d->D * cfm_elt_size(d->x_dtype) + (double)grid.x * d->V * d->D * 2);
    if (d->w_dtype == CFM_BF16) {
        if (d->x_dtype == CFM_F32) CFM_LAUNCH((cfm_token_logprob_kernel<BF16, float>), grid, block, lds, s, *d);
        else CFM_LAUNCH((cfm_token_logprob_kernel<BF16, BF16>), grid, block, lds, s, *d);
    } else {
        if (d->x_dtype == CFM_F32) CFM_LAUNCH((cfm_token_logprob_kernel<F16, float>), grid, block, lds, s, *d);
        else CFM_LAUNCH((cfm_token_logprob_kernel<F16, F16>), grid, block, lds, s, *d);
    }
    return cfm_launch_status("cfm_token_logprob");
}

// --------------------------------------------------------------------------------------------------------------------------------- combine
__global__ __launch_bounds__(64) void cfm_rescore_combine_kernel(cfm_rescore_combine_desc d) {
#pragma clang fp contract(off)                                  // every product and sum below is rounded on its own: no fused multiply-add
    const int b = blockIdx.x, n = threadIdx.x;
    const int N = d.N, Lc = d.Lc;
    float fin = -INFINITY;
    if (n < N) {
        const int64_t p = (int64_t)b * N + n;
        float l = 0.f, r = 0.f;
        const float* row = d.logp + p * Lc;
        for (int i = 0; i < Lc; ++i) l = __fadd_rn(l, row[i]);
        if (d.logp_r) {
            const float* rr = d.logp_r + p * Lc;
            for (int i = 0; i < Lc; ++i) r = __fadd_rn(r, rr[i]);
        }
        const float sc = d.score[p];
        const bool used = d.nlen[p] >= 0 && sc != -INFINITY;
        const float att = d.reverse_weight == 0.f ? l : __fadd_rn(__fmul_rn(1.f - d.reverse_weight, l), __fmul_rn(d.reverse_weight, r));
        fin = used ? __fadd_rn(att, __fmul_rn(d.first_pass_weight, sc)) : -INFINITY;
        d.final_score[p] = fin;
        d.left[p] = l;
        d.right[p] = r;
    }
    const float key = fin != fin ? -INFINITY : fin;            // a total order: NaN ranks with the unused entries
    int rank = 0;
    for (int m = 0; m < N; ++m) {
        const float km = __shfl(key, m, 64);
        rank += (km > key || (km == key && m < n)) ? 1 : 0;
    }
    if (n < N) d.order[(int64_t)b * N + rank] = n;
}

extern "C" int cfm_rescore_combine(const cfm_rescore_combine_desc* d, cfm_stream_t stream) {
    CFM_CHECK_ARG(d, "cfm_rescore_combine: null descriptor");
    CFM_CHECK_ARG(d->B >= 1 && d->N >= 1 && d->N <= 16 && d->Lc >= 1, "cfm_rescore_combine: bad shape B=%d N=%d Lc=%d (1 <= N <= 16)", d->B, d->N, d->Lc);
    CFM_CHECK_ARG(d->logp && d->nlen && d->score && d->final_score && d->left && d->right && d->order, "cfm_rescore_combine: null pointer");
    CFM_CHECK_ARG(d->reverse_weight >= 0.f && d->reverse_weight <= 1.f, "cfm_rescore_combine: reverse_weight=%g outside [0, 1]", (double)d->reverse_weight);
    CFM_CHECK_ARG(d->logp_r || d->reverse_weight == 0.f, "cfm_rescore_combine: reverse_weight=%g needs logp_r", (double)d->reverse_weight);
    hipStream_t s = (hipStream_t)stream;
    CfmProfScope prof("rescore_combine", s, 0.0, (double)d->B * d->N * d->Lc * 4 * (d->logp_r ? 2 : 1));
    CFM_LAUNCH(cfm_rescore_combine_kernel, dim3((unsigned)d->B), dim3(64), 0, s, *d);
    return cfm_launch_status("cfm_rescore_combine");
}
