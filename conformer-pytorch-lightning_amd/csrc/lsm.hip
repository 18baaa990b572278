// lsm.hip -- the label-smoothing loss of the attention decoder and its gradient (include/cfm.h states the entry points; the definition is
// tests/attention_loss_ref.py in float64).  With z the logits of a row, t its target, s the smoothing, e = s / (V - 1):
//     loss = C(s, V) - (1 - s - e) (z_t - lse) - e (S - V lse),   S = sum_{c < V} z_c,   dz_c = g (exp(z_c - lse) - q_c)
//
//   cfm_lsm_loss     the product, the online logsumexp and the target gather are cfm_token_logprob's (vocab_tile.h); a running f32 sum of the
//                    logits rides along.  The logits form is one wavefront per row over stored logits.
//   cfm_lsm_grad     recomputes the logits tile by tile on the same loop and writes dz in the activation type; the vocabulary is also split
//                    over blockIdx.y (no reduction crosses a tile here).  The logits form is elementwise.
//   cfm_lsm_reduce   sum_m loss_m / denom in one workgroup, a fixed order, and denom itself (the batch size or the count of valid targets).
#include "cfm_common.h"
#include "vocab_tile.h"

namespace {

constexpr unsigned LSM_GRID_TARGET = 256;   // workgroups the backward's grid aims at: the MI355X's compute units (fewer elsewhere only splits finer)

struct LsmCoef {
    float c, wt, e, conf;   // C(s, V); 1 - s - e; e; 1 - s
};

LsmCoef lsm_coef(float smoothing, int V) {
    const double s = smoothing, e = V > 1 ? s / (V - 1) : 0.0, conf = 1.0 - s;
    const double c = (conf > 0.0 ? conf * log(conf) : 0.0) + (e > 0.0 ? (V - 1) * e * log(e) : 0.0);   // 0 log 0 = 0
    return {(float)c, (float)(conf - e), (float)e, (float)conf};
}

__device__ __forceinline__ float lsm_row_loss(const LsmCoef& k, int V, float zt, float lse, float zsum) {
    return k.c - k.wt * (zt - lse) - k.e * (zsum - (float)V * lse);
}

// ------------------------------------------------------------------------------------------------------------------------------ forward
template <typename HT, typename XT>
__global__ __launch_bounds__(TL_WAVES * 64) void cfm_lsm_loss_kernel(cfm_lsm_loss_desc d, LsmCoef k) {
    extern __shared__ __attribute__((aligned(16))) unsigned char tl_smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int row0 = blockIdx.x * TL_ROWS;
    const int M = d.M, D = d.D, V = d.V;
    int live = 0;
    if (tid < TL_ROWS) live = row0 + tid < M && d.target[row0 + tid] >= 0;
    if (!__syncthreads_or(live)) {                             // a wholly ignored tile: nothing of X, W or bias is read
        if (tid < TL_ROWS && row0 + tid < M) d.loss[row0 + tid] = 0.f, d.lse[row0 + tid] = 0.f;
        return;
    }
    tl_stage_rows<HT, XT>(tl_smem, d.X, d.ldx, row0, M, D, tid);

    const int g = lane >> 4, l15 = lane & 15;
    float mx[4], sm[4], tv[4], zs[4];
    int tg[4];
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        const int r = row0 + s * 16 + l15;
        tg[s] = r < M ? d.target[r] : -1;
        mx[s] = -INFINITY, sm[s] = 0.f, tv[s] = 0.f, zs[s] = 0.f;
    }
    tl_tiles<HT>(tl_smem, (const u16*)d.W, d.bias, D, V, wave, TL_WAVES, (V + 31) >> 5, lane, [&](int c0, int s, const float (&v)[8]) {
        tl_fold_lse(mx[s], sm[s], v);
        tl_pick_target(tv[s], tg[s], c0, g, v);
        float add = 0.f;
#pragma unroll
        for (int q = 0; q < 8; ++q) add += c0 + (q >> 2) * 16 + g * 4 + (q & 3) < V ? v[q] : 0.f;
        zs[s] += add;
    });
    // the four lanes of a row (g = 0..3): xor 16, then xor 32
#pragma unroll
    for (int s = 0; s < 4; ++s) {
#pragma unroll
        for (int o = 16; o <= 32; o <<= 1) {
            const float m2 = __shfl_xor(mx[s], o, 64), s2 = __shfl_xor(sm[s], o, 64), t2 = __shfl_xor(tv[s], o, 64), z2 = __shfl_xor(zs[s], o, 64);
            tl_merge(mx[s], sm[s], m2, s2);
            tv[s] += t2;
            zs[s] += z2;
        }
    }
    __syncthreads();                                           // every wavefront is done with the row image: its memory now takes the partials
    float* part = (float*)tl_smem;                             // [TL_WAVES][4][TL_ROWS]
    if (g == 0) {
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const int r = s * 16 + l15;
            part[(wave * 4 + 0) * TL_ROWS + r] = mx[s];
            part[(wave * 4 + 1) * TL_ROWS + r] = sm[s];
            part[(wave * 4 + 2) * TL_ROWS + r] = tv[s];
            part[(wave * 4 + 3) * TL_ROWS + r] = zs[s];
        }
    }
    __syncthreads();
    if (tid < TL_ROWS && row0 + tid < M) {
        float m = part[tid], sum = part[TL_ROWS + tid], val = part[2 * TL_ROWS + tid], zsum = part[3 * TL_ROWS + tid];
        for (int w = 1; w < TL_WAVES; ++w) {
            tl_merge(m, sum, part[(w * 4 + 0) * TL_ROWS + tid], part[(w * 4 + 1) * TL_ROWS + tid]);
            val += part[(w * 4 + 2) * TL_ROWS + tid];
            zsum += part[(w * 4 + 3) * TL_ROWS + tid];
        }
        const int t = d.target[row0 + tid];
        const float lse = m + logf(sum);
        d.loss[row0 + tid] = t < 0 ? 0.f : t >= V ? __builtin_nanf("") : lsm_row_loss(k, V, val, lse, zsum);
        d.lse[row0 + tid] = t < 0 ? 0.f : lse;
    }
}

// The logits form: one wavefront per row, lane j takes classes j, j + 64, ..; the lanes' values meet in a xor butterfly (symmetric: every lane
// ends with the same bits).
__global__ __launch_bounds__(256) void cfm_lsm_loss_logits_kernel(cfm_lsm_loss_desc d, LsmCoef k) {
    const int lane = threadIdx.x & 63;
    const int m = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4 + (threadIdx.x >> 6)));
    if (m >= d.M) return;
    const int t = d.target[m];
    if (t < 0) {
        if (lane == 0) d.loss[m] = 0.f, d.lse[m] = 0.f;
        return;
    }
    const float* row = d.logits + (int64_t)m * d.ld;
    float mx = -INFINITY, sm = 0.f, zs = 0.f;
    for (int c = lane; c < d.V; c += 64) {
        const float z = row[c];
        tl_merge(mx, sm, z, 1.f);
        zs += z;
    }
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const float m2 = __shfl_xor(mx, o, 64), s2 = __shfl_xor(sm, o, 64), z2 = __shfl_xor(zs, o, 64);
        tl_merge(mx, sm, m2, s2);
        zs += z2;
    }
    if (lane == 0) {
        const float lse = mx + logf(sm);
        d.loss[m] = t >= d.V ? __builtin_nanf("") : lsm_row_loss(k, d.V, row[t], lse, zs);
        d.lse[m] = lse;
    }
}

// ----------------------------------------------------------------------------------------------------------------------------- backward
// 4 consecutive classes c .. c + 3 of row `row` (c % 4 == 0, c + 3 < Vk): g (exp(z - lse) - q), exact zeros at and past V and in ignored rows
template <typename ZT>
__device__ __forceinline__ void lsm_store_dz(void* dz, int64_t ldz, int row, int c, const float* z, int V, int t, float lse, float gm, const LsmCoef& k) {
    f32x4 o;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const float q = c + e == t ? k.conf : k.e;
        o[e] = (t >= 0 && c + e < V) ? gm * (__expf(z[e] - lse) - q) : 0.f;
    }
    st4<ZT>(dz, (int64_t)row * ldz + c, o);
}

template <typename HT, typename XT, typename ZT>
__global__ __launch_bounds__(TL_WAVES * 64) void cfm_lsm_grad_kernel(cfm_lsm_grad_desc d, LsmCoef k) {
    extern __shared__ __attribute__((aligned(16))) unsigned char tl_smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int row0 = blockIdx.x * TL_ROWS;
    const int M = d.M, D = d.D, V = d.V, Vk = d.Vk;
    const int ntile = (Vk + 31) >> 5;                          // the tiles cover the zero columns V..Vk too
    const int ct0 = blockIdx.y * TL_WAVES + wave, ctstep = gridDim.y * TL_WAVES;
    int live = 0;
    if (tid < TL_ROWS) live = row0 + tid < M && d.target[row0 + tid] >= 0;
    if (!__syncthreads_or(live)) {                             // a wholly ignored tile: zeros, nothing of X, W or bias is read
        for (int ct = ct0; ct < ntile; ct += ctstep)
            for (int i = lane; i < TL_ROWS * 8; i += 64) {
                const int r = row0 + (i >> 3), c = ct * 32 + (i & 7) * 4;
                if (r < M && c < Vk) st4<ZT>(d.dz, (int64_t)r * d.ldz + c, (f32x4){0.f, 0.f, 0.f, 0.f});
            }
        return;
    }
    tl_stage_rows<HT, XT>(tl_smem, d.X, d.ldx, row0, M, D, tid);

    const int g = lane >> 4, l15 = lane & 15;
    float ls[4], gm[4];
    int tg[4];
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        const int r = row0 + s * 16 + l15;
        tg[s] = r < M ? d.target[r] : -1;
        ls[s] = r < M ? d.lse[r] : 0.f;
        gm[s] = r < M ? d.g[r] : 0.f;
    }
    tl_tiles<HT>(tl_smem, (const u16*)d.W, d.bias, D, V, ct0, ctstep, ntile, lane, [&](int c0, int s, const float (&v)[8]) {
        const int r = row0 + s * 16 + l15;
        if (r >= M) return;
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const int c = c0 + t * 16 + g * 4;                 // Vk % 4 == 0: the four classes lie wholly inside [0, Vk) or wholly outside
            if (c < Vk) lsm_store_dz<ZT>(d.dz, d.ldz, r, c, v + t * 4, V, tg[s], ls[s], gm[s], k);
        }
    });
}

template <typename ZT>
__global__ __launch_bounds__(256) void cfm_lsm_grad_logits_kernel(cfm_lsm_grad_desc d, LsmCoef k) {
    const int nq = d.Vk >> 2;
    const int64_t n = (int64_t)d.M * nq;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const int m = (int)(i / nq), c = (int)(i - (int64_t)m * nq) * 4;
        const int t = d.target[m];
        float z[4] = {0.f, 0.f, 0.f, 0.f};
        if (t >= 0) {
            const float* row = d.logits + (int64_t)m * d.ld;
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (c + e < d.V) z[e] = row[c + e];
        }
        lsm_store_dz<ZT>(d.dz, d.ldz, m, c, z, d.V, t, d.lse[m], d.g[m], k);
    }
}

// ------------------------------------------------------------------------------------------------------------------------------- reduce
// One workgroup: thread i sums rows i, i + 256, .. in order, then a binary tree over the 256 partials.  out[0] = sum / denom, out[1] = denom:
// the batch size when batch > 0, else the number of targets >= 0 (at least 1: no valid target gives loss 0).
__global__ __launch_bounds__(256) void cfm_lsm_reduce_kernel(const float* __restrict__ loss, const int32_t* __restrict__ target, int M, int batch,
                                                             float* __restrict__ out) {
    __shared__ float ssum[256];
    __shared__ int scnt[256];
    const int tid = threadIdx.x;
    float s = 0.f;
    int n = 0;
    for (int m = tid; m < M; m += 256) {
        s += loss[m];
        n += target[m] >= 0 ? 1 : 0;
    }
    ssum[tid] = s, scnt[tid] = n;
    __syncthreads();
    for (int h = 128; h >= 1; h >>= 1) {
        if (tid < h) ssum[tid] += ssum[tid + h], scnt[tid] += scnt[tid + h];
        __syncthreads();
    }
    if (tid == 0) {
        const float denom = batch > 0 ? (float)batch : (float)max(scnt[0], 1);
        out[0] = ssum[0] / denom;
        out[1] = denom;
    }
}

int lsm_check_product(const char* op, const void* X, const void* W, const float* bias, int D, int x_dtype, int w_dtype, int64_t ldx) {
    CFM_CHECK_ARG(X && W && bias, "%s: null pointer (X, W and bias, or logits)", op);
    CFM_CHECK_ARG(D >= 8 && D % 8 == 0 && D <= TL_MAXD, "%s: D=%d (a multiple of 8, at most %d)", op, D, TL_MAXD);
    CFM_CHECK_ARG(cfm_is16(w_dtype), "%s: W is bf16 or fp16 (the fp32 mode runs cfm_gemm and the logits form)", op);
    CFM_CHECK_ARG(x_dtype == CFM_F32 || x_dtype == w_dtype, "%s: X is f32 or of W's type", op);
    const int xa = x_dtype == CFM_F32 ? 4 : 8;
    CFM_CHECK_ARG(ldx >= D && ldx % xa == 0 && ((uintptr_t)X & 15) == 0 && ((uintptr_t)W & 15) == 0,
                  "%s: X and W must be 16-byte aligned, ldx=%lld a multiple of %d and >= D", op, (long long)ldx, xa);
    return 0;
}

int lsm_check_smoothing(const char* op, float s, int V) {
    CFM_CHECK_ARG(s >= 0.f && s < 1.f && (s == 0.f || V >= 2), "%s: smoothing=%g outside [0, 1), or a vocabulary of one class with smoothing", op, (double)s);
    return 0;
}

}  // namespace

extern "C" int cfm_lsm_loss(const cfm_lsm_loss_desc* d, cfm_stream_t stream) {
    CFM_CHECK_ARG(d, "cfm_lsm_loss: null descriptor");
    CFM_CHECK_ARG(d->M >= 1 && d->V >= 1, "cfm_lsm_loss: bad shape M=%d V=%d", d->M, d->V);
    CFM_CHECK_ARG(d->target && d->loss && d->lse, "cfm_lsm_loss: null pointer");
    if (int rc = lsm_check_smoothing("cfm_lsm_loss", d->smoothing, d->V)) return rc;
    const LsmCoef k = lsm_coef(d->smoothing, d->V);
    hipStream_t s = (hipStream_t)stream;
    if (d->logits) {
        CFM_CHECK_ARG(d->ld >= d->V, "cfm_lsm_loss: logits row stride %lld below V=%d", (long long)d->ld, d->V);
        CfmProfScope prof("lsm_loss_logits", s, 0.0, (double)d->M * d->V * 4);
        CFM_LAUNCH(cfm_lsm_loss_logits_kernel, dim3((unsigned)((d->M + 3) / 4)), dim3(256), 0, s, *d, k);
        return cfm_launch_status("cfm_lsm_loss (logits)");
    }
    if (int rc = lsm_check_product("cfm_lsm_loss", d->X, d->W, d->bias, d->D, d->x_dtype, d->w_dtype, d->ldx)) return rc;
    const size_t lds = tl_lds_bytes(d->D, 4);
    const dim3 grid((unsigned)((d->M + TL_ROWS - 1) / TL_ROWS)), block(TL_WAVES * 64);
    CfmProfScope prof("lsm_loss", s, 2.0 * d->M * d->V * d->D, (double)d->M * d->D * cfm_elt_size(d->x_dtype) + (double)grid.x * d->V * d->D * 2);
    if (d->w_dtype == CFM_BF16) {
        if (d->x_dtype == CFM_F32) CFM_LAUNCH((cfm_lsm_loss_kernel<BF16, float>), grid, block, lds, s, *d, k);
        else CFM_LAUNCH((cfm_lsm_loss_kernel<BF16, BF16>), grid, block, lds, s, *d, k);
    } else {
        if (d->x_dtype == CFM_F32) CFM_LAUNCH((cfm_lsm_loss_kernel<F16, float>), grid, block, lds, s, *d, k);
        else CFM_LAUNCH((cfm_lsm_loss_kernel<F16, F16>), grid, block, lds, s, *d, k);
    }
    return cfm_launch_status("cfm_lsm_loss");
}

extern "C" int cfm_lsm_grad(const cfm_lsm_grad_desc* d, cfm_stream_t stream) {
    CFM_CHECK_ARG(d, "cfm_lsm_grad: null descriptor");
    CFM_CHECK_ARG(d->M >= 1 && d->V >= 1, "cfm_lsm_grad: bad shape M=%d V=%d", d->M, d->V);
    CFM_CHECK_ARG(d->target && d->lse && d->g && d->dz, "cfm_lsm_grad: null pointer");
    CFM_CHECK_ARG(d->Vk >= d->V && d->Vk % 4 == 0 && d->ldz >= d->Vk && d->ldz % 4 == 0 && ((uintptr_t)d->dz & 15) == 0,
                  "cfm_lsm_grad: Vk=%d (>= V=%d, a multiple of 4), ldz=%lld (>= Vk, a multiple of 4), dz 16-byte aligned", d->Vk, d->V, (long long)d->ldz);
    CFM_CHECK_ARG(d->dz_dtype >= CFM_F32 && d->dz_dtype <= CFM_F16, "cfm_lsm_grad: bad dz_dtype");
    if (int rc = lsm_check_smoothing("cfm_lsm_grad", d->smoothing, d->V)) return rc;
    const LsmCoef k = lsm_coef(d->smoothing, d->V);
    hipStream_t s = (hipStream_t)stream;
    if (d->logits) {
        CFM_CHECK_ARG(d->ld >= d->V, "cfm_lsm_grad: logits row stride %lld below V=%d", (long long)d->ld, d->V);
        const int64_t n = (int64_t)d->M * (d->Vk / 4);
        const unsigned blocks = (unsigned)(n + 255 < (int64_t)4096 * 256 ? (n + 255) / 256 : 4096);
        CfmProfScope prof("lsm_grad_logits", s, 0.0, (double)d->M * (d->V * 4.0 + (double)d->Vk * cfm_elt_size(d->dz_dtype)));
        if (d->dz_dtype == CFM_F32) CFM_LAUNCH((cfm_lsm_grad_logits_kernel<float>), dim3(blocks), dim3(256), 0, s, *d, k);
        else if (d->dz_dtype == CFM_BF16) CFM_LAUNCH((cfm_lsm_grad_logits_kernel<BF16>), dim3(blocks), dim3(256), 0, s, *d, k);
        else CFM_LAUNCH((cfm_lsm_grad_logits_kernel<F16>), dim3(blocks), dim3(256), 0, s, *d, k);
        return cfm_launch_status("cfm_lsm_grad (logits)");
    }
    if (int rc = lsm_check_product("cfm_lsm_grad", d->X, d->W, d->bias, d->D, d->x_dtype, d->w_dtype, d->ldx)) return rc;
    CFM_CHECK_ARG(d->dz_dtype == d->w_dtype, "cfm_lsm_grad: dz is of W's type in the fused form (it is cfm_gemm's and cfm_gemm_tn's 16-bit operand)");
    const size_t lds = tl_lds_bytes(d->D, 0);
    // no reduction crosses a tile here, so the vocabulary is split over blockIdx.y until the grid holds about one workgroup per CU
    const unsigned gx = (unsigned)((d->M + TL_ROWS - 1) / TL_ROWS);
    const unsigned rounds = (unsigned)(((d->Vk + 31) / 32 + TL_WAVES - 1) / TL_WAVES);
    unsigned gy = LSM_GRID_TARGET / gx;
    gy = gy < 1 ? 1 : gy > rounds ? rounds : gy;
    const dim3 grid(gx, gy), block(TL_WAVES * 64);
    CfmProfScope prof("lsm_grad", s, 2.0 * d->M * d->V * d->D, (double)d->M * d->Vk * 2 + (double)gx * d->V * d->D * 2);
    if (d->w_dtype == CFM_BF16) {
        if (d->x_dtype == CFM_F32) CFM_LAUNCH((cfm_lsm_grad_kernel<BF16, float, BF16>), grid, block, lds, s, *d, k);
        else CFM_LAUNCH((cfm_lsm_grad_kernel<BF16, BF16, BF16>), grid, block, lds, s, *d, k);
    } else {
        if (d->x_dtype == CFM_F32) CFM_LAUNCH((cfm_lsm_grad_kernel<F16, float, F16>), grid, block, lds, s, *d, k);
        else CFM_LAUNCH((cfm_lsm_grad_kernel<F16, F16, F16>), grid, block, lds, s, *d, k);
    }
    return cfm_launch_status("cfm_lsm_grad");
}

extern "C" int cfm_lsm_reduce(const float* loss, const int32_t* target, int32_t M, int32_t batch, float* out, cfm_stream_t stream) {
    CFM_CHECK_ARG(loss && target && out && M >= 1 && batch >= 0, "cfm_lsm_reduce: bad arguments (M >= 1, batch >= 0: 0 counts the valid targets)");
    hipStream_t s = (hipStream_t)stream;
    CfmProfScope prof("lsm_reduce", s, 0.0, (double)M * 8);
    CFM_LAUNCH(cfm_lsm_reduce_kernel, dim3(1), dim3(256), 0, s, loss, target, M, batch, out);
    return cfm_launch_status("cfm_lsm_reduce");
}
