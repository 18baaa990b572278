// lstm.hip -- the RNN-T predictor's LSTM over a whole label matrix, forward and backward (torch.nn.LSTM(batch_first=True): gate order
// i, f, g, o in weight_ih_l{k} [4H, in] / weight_hh_l{k} [4H, H] / bias_* [4H], optional (h0, c0), dropout between layers in train mode).
// Everything is f32 and every product runs on the f32 MFMA (v_mfma_f32_16x16x4_f32: exact f32 multiplies, f32 accumulation), walked as
// greedy.hip walks its skinny products: lane (l15, g) of a wavefront supplies contraction index 16 q + 4 g + r to the r-th MFMA of step q
// and ends up with output rows 4 g + r of column l15.
//
// Inside the library a layer's rows are TIME-major, m = t * B + b: the 16 sequences of a tile are then neighbours at every step, and with
// one extra leading time slot for the initial state the saved outputs serve twice -- ybuf[1 .. U] is the layer's output, ybuf[0 .. U-1]
// is "h of the step before", the operand of dW_hh -- without a shifted copy.  x, y, dy and dx keep torch's [B, U, *] layout: the
// products that touch them remap the row index.
//
//   forward, per layer    mm (gates' input part = drop(x_l) . W_ih^T + b_ih + b_hh, all U*B rows)  ->  recurrence (one launch)
//   backward, per layer   reverse recurrence (d gates)  ->  mm x 3 (dW_ih, dW_hh, dx_l with the dropout mask regenerated)  ->  column sums
//
// Recurrences: a workgroup of 8 wavefronts owns 16 sequences for all U steps and never looks at another workgroup.  A wavefront owns
// groups of 16 hidden units across all four gates (four accumulators), so lane (l15, g) holds i, f, g, o, c of units 4 g .. 4 g + 3 of its
// group for sequence l15 and the cell update is lane-local.  h of the tile lives in LDS (two buffers: one barrier per step), c in
// registers, W_hh is streamed from L2 every step.  The reverse recurrence keeps d h (recurrent part) and d c in the same registers: its
// product d gates . W_hh takes d gates of the tile from LDS and W_hh as the row operand, so the result lands in the owning lane.
#include <math.h>

#include "cfm_common.h"

namespace {

constexpr int LSTM_NW = 8;             // wavefronts per recurrence workgroup
constexpr int LSTM_NT = LSTM_NW * 64;
constexpr int LSTM_MAXG = 4;           // unit groups of 16 per wavefront: H <= 512

__device__ __forceinline__ float sigmoid_acc(float x) { return 1.0f / (1.0f + expf(-x)); }
__device__ __forceinline__ f32x4 mfma4(const f32x4& a, const f32x4& b, f32x4 acc) {
#pragma unroll
    for (int r = 0; r < 4; ++r) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[r], b[r], acc, 0, 0, 0);
    return acc;
}

// ---------------------------------------------------------------------------------------------------------------------------------------
// out[j, i] = sum_k P(i, k) Q(j, k) (+ b1[i] + b2[i]),  P(i, k) = P[i * spi + k * spk],  Q(j, k) = Q[j * sqj + k * sqk],  i contiguous in out.
// I % 64 == 0; J and the contraction length Kc are arbitrary (clamped loads, masked stores / zeroed terms).  A contraction-contiguous
// operand (stride 1) is read as 16-byte pieces, a strided one as four dwords that are contiguous across l15.
// remap: a row index m = t * rB + b of the time-major order addresses row b * rU + t of a [B, U, *] operand.
// drop_on: the dropout mask of the element's offset (relative to the operand's base) is applied to P (1), Q (2) or the output (3).
// ---------------------------------------------------------------------------------------------------------------------------------------
struct MmArgs {
    const float *P, *Q;
    int64_t spi, spk, sqj, sqk, ldo;
    float* out;
    const float *b1, *b2;
    int I, J, Kc;
    int remap_pk, remap_qj, remap_oj, rB, rU;
    int drop_on;
    CfmDrop drop;
};

__device__ __forceinline__ int64_t remap_row(const MmArgs& a, int m) { return (int64_t)(m % a.rB) * a.rU + m / a.rB; }

template <int NJ>
__global__ __launch_bounds__(256) void cfm_lstm_mm_kernel(const MmArgs a) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, l15 = lane & 15, g = lane >> 4;
    const int i0 = (blockIdx.x * 4 + wave) * 16;
    if (i0 >= a.I) return;
    const int jbase = blockIdx.y * (16 * NJ);
    f32x4 acc[NJ];
    int64_t qoff[NJ];
#pragma unroll
    for (int jt = 0; jt < NJ; ++jt) {
        acc[jt] = (f32x4){0.f, 0.f, 0.f, 0.f};
        int j = jbase + jt * 16 + l15;
        j = j < a.J ? j : a.J - 1;
        qoff[jt] = (a.remap_qj ? remap_row(a, j) : (int64_t)j) * a.sqj;
    }
    const int64_t poff = (int64_t)(i0 + l15) * a.spi;
    const bool pvec = a.spk == 1 && !a.remap_pk && a.Kc % 16 == 0, qvec = a.sqk == 1 && a.Kc % 16 == 0;   // uniform
    const int nq = (a.Kc + 15) / 16;
#pragma unroll 2
    for (int q = 0; q < nq; ++q) {
        const int k0 = 16 * q + 4 * g;
        f32x4 pv, qv[NJ];
        if (pvec) {
            pv = ld4<float>(a.P, poff + k0);
            if (a.drop_on == 1) {
#pragma unroll
                for (int r = 0; r < 4; ++r) pv[r] = cfm_drop(a.drop, (unsigned)(poff + k0 + r), pv[r]);
            }
        } else {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int k = k0 + r;
                float v = 0.f;
                if (k < a.Kc) {
                    const int64_t o = poff + (a.remap_pk ? remap_row(a, k) : (int64_t)k) * a.spk;
                    v = ld1<float>(a.P, o);
                    if (a.drop_on == 1) v = cfm_drop(a.drop, (unsigned)o, v);
                }
                pv[r] = v;
            }
        }
#pragma unroll
        for (int jt = 0; jt < NJ; ++jt) {
            if (qvec) {
                qv[jt] = ld4<float>(a.Q, qoff[jt] + k0);
                if (a.drop_on == 2) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) qv[jt][r] = cfm_drop(a.drop, (unsigned)(qoff[jt] + k0 + r), qv[jt][r]);
                }
            } else {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int k = k0 + r;
                    float v = 0.f;
                    if (k < a.Kc) {
                        const int64_t o = qoff[jt] + (int64_t)k * a.sqk;
                        v = ld1<float>(a.Q, o);
                        if (a.drop_on == 2) v = cfm_drop(a.drop, (unsigned)o, v);
                    }
                    qv[jt][r] = v;
                }
            }
        }
#pragma unroll
        for (int jt = 0; jt < NJ; ++jt) acc[jt] = mfma4(pv, qv[jt], acc[jt]);
    }
    // lane (l15, g) holds out[j = jbase + 16 jt + l15][i0 + 4 g + r]
    f32x4 bv = (f32x4){0.f, 0.f, 0.f, 0.f};
    if (a.b1) bv += ld4<float>(a.b1, i0 + 4 * g);
    if (a.b2) bv += ld4<float>(a.b2, i0 + 4 * g);
#pragma unroll
    for (int jt = 0; jt < NJ; ++jt) {
        const int j = jbase + jt * 16 + l15;
        if (j >= a.J) continue;
        const int64_t o = (a.remap_oj ? remap_row(a, j) : (int64_t)j) * a.ldo + i0 + 4 * g;
        f32x4 v = acc[jt] + bv;
        if (a.drop_on == 3) {
#pragma unroll
            for (int r = 0; r < 4; ++r) v[r] = cfm_drop(a.drop, (unsigned)(o + r), v[r]);
        }
        st4<float>(a.out, o, v);
    }
}

int launch_mm(const MmArgs& a, bool narrow, hipStream_t s, const char* name) {
    CfmProfScope prof(name, s, 2.0 * a.I * (double)a.J * a.Kc, 4.0 * ((double)a.I * a.Kc + (double)a.J * a.Kc + (double)a.I * a.J));
    if (narrow) CFM_LAUNCH((cfm_lstm_mm_kernel<1>), dim3((unsigned)(a.I / 64), (unsigned)((a.J + 15) / 16)), dim3(256), 0, s, a);
    else CFM_LAUNCH((cfm_lstm_mm_kernel<4>), dim3((unsigned)(a.I / 64), (unsigned)((a.J + 63) / 64)), dim3(256), 0, s, a);
    return cfm_launch_status(name);
}

// column sums of d gates [M, N] -> one or two bias gradients [N]: 64 columns x 16 row groups per workgroup, summed in a fixed order
__global__ __launch_bounds__(1024) void cfm_lstm_colsum_kernel(const float* __restrict__ dg, int M, int N, float* o1, float* o2) {
    __shared__ float part[16][64];
    const int c = threadIdx.x & 63, rg = threadIdx.x >> 6, n = blockIdx.x * 64 + c;
    float s = 0.f;
    for (int m = rg; m < M; m += 16) s += ld1<float>(dg, (int64_t)m * N + n);
    part[rg][c] = s;
    __syncthreads();
    if (rg == 0) {
        float t = 0.f;
#pragma unroll
        for (int i = 0; i < 16; ++i) t += part[i][c];
        if (o1) st1<float>(o1, n, t);
        if (o2) st1<float>(o2, n, t);
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------------
// Forward recurrence of one layer.  gates [U*B, 4H]: in, the input part of the pre-activations; out, the gates after their
// activations.  ybuf / cbuf [(U+1)*B, H]: slot 0 receives (h0, c0), slot t + 1 the state after step t.
// ---------------------------------------------------------------------------------------------------------------------------------------
struct FwdArgs {
    const float *w_hh, *h0, *c0;   // h0 / c0 [B, H] of this layer or null (zeros)
    float *gates, *ybuf, *cbuf;
    float *y, *hn, *cn;            // y [B, U, H] (last layer only, else null); hn / cn [B, H] of this layer
    int B, U, H;
};

template <int NG>
__global__ __launch_bounds__(LSTM_NT) void cfm_lstm_fwd_kernel(const FwdArgs a) {
    extern __shared__ __attribute__((aligned(16))) float lstm_hs[];   // [2][16][H + 4]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l15 = lane & 15, g = lane >> 4;
    const int B = a.B, U = a.U, H = a.H, ldh = H + 4, ngroups = H >> 4;
    const int b0 = blockIdx.x * 16, b = b0 + l15;
    const bool live = b < B;
    const int bc = live ? b : B - 1;
    const int64_t BH = (int64_t)B * H;
    for (int idx = tid; idx < 16 * H; idx += LSTM_NT) {
        const int sq = idx / H, k = idx - sq * H;
        const int bb = b0 + sq < B ? b0 + sq : B - 1;
        const float v = a.h0 ? ld1<float>(a.h0, (int64_t)bb * H + k) : 0.f;
        lstm_hs[sq * ldh + k] = v;
        if (b0 + sq < B) st1<float>(a.ybuf, (int64_t)bb * H + k, v);
    }
    f32x4 c[NG];
#pragma unroll
    for (int j = 0; j < NG; ++j) {
        const int ug = wave + LSTM_NW * j;
        c[j] = (f32x4){0.f, 0.f, 0.f, 0.f};
        if (ug < ngroups) {
            const int64_t o = (int64_t)bc * H + ug * 16 + 4 * g;
            if (a.c0) c[j] = ld4<float>(a.c0, o);
            if (live) st4<float>(a.cbuf, o, c[j]);
        }
    }
    __syncthreads();
    for (int t = 0; t < U; ++t) {
        const float* hcur = lstm_hs + (t & 1) * 16 * ldh;
        float* hnext = lstm_hs + ((t & 1) ^ 1) * 16 * ldh;
#pragma unroll
        for (int j = 0; j < NG; ++j) {
            const int ug = wave + LSTM_NW * j;
            if (ug >= ngroups) continue;                              // uniform per wavefront
            const int u = ug * 16 + 4 * g;
            f32x4 acc[4];
            const float* wrow[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                acc[k] = (f32x4){0.f, 0.f, 0.f, 0.f};
                wrow[k] = a.w_hh + (int64_t)(k * H + ug * 16 + l15) * H + 4 * g;
            }
            const float* hrow = hcur + l15 * ldh + 4 * g;
#pragma unroll 2
            for (int q = 0; q < (H >> 4); ++q) {
                const f32x4 hv = *(const f32x4*)(hrow + 16 * q);
                f32x4 wv[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) wv[k] = ld4<float>(wrow[k], 16 * q);
#pragma unroll
                for (int k = 0; k < 4; ++k) acc[k] = mfma4(wv[k], hv, acc[k]);
            }
            const int64_t row = (int64_t)t * B + bc;
            const int64_t go = row * 4 * H + u;
            f32x4 vi = acc[0] + ld4<float>(a.gates, go), vf = acc[1] + ld4<float>(a.gates, go + H);
            f32x4 vg = acc[2] + ld4<float>(a.gates, go + 2 * H), vo = acc[3] + ld4<float>(a.gates, go + 3 * H);
            f32x4 hv;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                vi[r] = sigmoid_acc(vi[r]);
                vf[r] = sigmoid_acc(vf[r]);
                vg[r] = tanhf(vg[r]);
                vo[r] = sigmoid_acc(vo[r]);
                c[j][r] = vf[r] * c[j][r] + vi[r] * vg[r];
                hv[r] = vo[r] * tanhf(c[j][r]);
            }
            *(f32x4*)(hnext + l15 * ldh + u) = hv;
            if (live) {
                st4<float>(a.gates, go, vi);
                st4<float>(a.gates, go + H, vf);
                st4<float>(a.gates, go + 2 * H, vg);
                st4<float>(a.gates, go + 3 * H, vo);
                const int64_t so = BH * (t + 1) + (int64_t)b * H + u;
                st4<float>(a.ybuf, so, hv);
                st4<float>(a.cbuf, so, c[j]);
                if (a.y) st4<float>(a.y, ((int64_t)b * U + t) * H + u, hv);
                if (t == U - 1) {
                    st4<float>(a.hn, (int64_t)b * H + u, hv);
                    st4<float>(a.cn, (int64_t)b * H + u, c[j]);
                }
            }
        }
        __syncthreads();
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------------
// Reverse recurrence of one layer: d gates (pre-activation) [U*B, 4H] from dy (element (b, t, k) at b * dy_sb + t * dy_st + k), the saved
// gates and cells, and optional gradients of the final state; d h0 / d c0 [B, H].
// ---------------------------------------------------------------------------------------------------------------------------------------
struct BwdArgs {
    const float *w_hh, *gates, *cbuf, *dy, *dhn, *dcn;
    int64_t dy_sb, dy_st;
    float *dg, *dh0, *dc0;
    int B, U, H;
};

template <int NG>
__global__ __launch_bounds__(LSTM_NT) void cfm_lstm_bwd_kernel(const BwdArgs a) {
    extern __shared__ __attribute__((aligned(16))) float lstm_dg[];   // [16][4H + 4]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l15 = lane & 15, g = lane >> 4;
    const int B = a.B, U = a.U, H = a.H, ldg = 4 * H + 4, ngroups = H >> 4;
    const int b = blockIdx.x * 16 + l15;
    const bool live = b < B;
    const int bc = live ? b : B - 1;
    const int64_t BH = (int64_t)B * H;
    f32x4 dhr[NG], dcc[NG];
#pragma unroll
    for (int j = 0; j < NG; ++j) {
        const int ug = wave + LSTM_NW * j;
        dhr[j] = dcc[j] = (f32x4){0.f, 0.f, 0.f, 0.f};
        if (ug < ngroups) {
            const int64_t o = (int64_t)bc * H + ug * 16 + 4 * g;
            if (a.dhn) dhr[j] = ld4<float>(a.dhn, o);
            if (a.dcn) dcc[j] = ld4<float>(a.dcn, o);
        }
    }
    for (int t = U - 1; t >= 0; --t) {
#pragma unroll
        for (int j = 0; j < NG; ++j) {
            const int ug = wave + LSTM_NW * j;
            if (ug >= ngroups) continue;
            const int u = ug * 16 + 4 * g;
            const int64_t row = (int64_t)t * B + bc;
            const int64_t go = row * 4 * H + u;
            const f32x4 gi = ld4<float>(a.gates, go), gf = ld4<float>(a.gates, go + H), gg = ld4<float>(a.gates, go + 2 * H), gq = ld4<float>(a.gates, go + 3 * H);
            const f32x4 cp = ld4<float>(a.cbuf, BH * t + (int64_t)bc * H + u), ct = ld4<float>(a.cbuf, BH * (t + 1) + (int64_t)bc * H + u);
            const f32x4 dyv = ld4<float>(a.dy, (int64_t)bc * a.dy_sb + (int64_t)t * a.dy_st + u);
            f32x4 di, df, dgg, dq;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float dh = dyv[r] + dhr[j][r];
                const float tc = tanhf(ct[r]);
                const float dc = dcc[j][r] + dh * gq[r] * (1.f - tc * tc);
                di[r] = dc * gg[r] * gi[r] * (1.f - gi[r]);
                df[r] = dc * cp[r] * gf[r] * (1.f - gf[r]);
                dgg[r] = dc * gi[r] * (1.f - gg[r] * gg[r]);
                dq[r] = dh * tc * gq[r] * (1.f - gq[r]);
                dcc[j][r] = dc * gf[r];
            }
            float* ls = lstm_dg + l15 * ldg + u;
            *(f32x4*)ls = di;
            *(f32x4*)(ls + H) = df;
            *(f32x4*)(ls + 2 * H) = dgg;
            *(f32x4*)(ls + 3 * H) = dq;
            if (live) {
                st4<float>(a.dg, go, di);
                st4<float>(a.dg, go + H, df);
                st4<float>(a.dg, go + 2 * H, dgg);
                st4<float>(a.dg, go + 3 * H, dq);
            }
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < NG; ++j) {
            const int ug = wave + LSTM_NW * j;
            if (ug >= ngroups) continue;
            // d h[unit, seq] = sum_n W_hh[n, unit] dg[seq, n]: W_hh column (unit) as the row operand, four dwords per lane and step
            const float* wcol = a.w_hh + ug * 16 + l15;
            const float* drow = lstm_dg + l15 * ldg + 4 * g;
            f32x4 acc = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
            for (int q = 0; q < (H >> 2); ++q) {
                const f32x4 dv = *(const f32x4*)(drow + 16 * q);
                f32x4 wv;
#pragma unroll
                for (int r = 0; r < 4; ++r) wv[r] = ld1<float>(wcol, (int64_t)(16 * q + 4 * g + r) * H);
                acc = mfma4(wv, dv, acc);
            }
            dhr[j] = acc;
        }
        __syncthreads();
    }
    if (live) {
#pragma unroll
        for (int j = 0; j < NG; ++j) {
            const int ug = wave + LSTM_NW * j;
            if (ug >= ngroups) continue;
            const int64_t o = (int64_t)b * H + ug * 16 + 4 * g;
            st4<float>(a.dh0, o, dhr[j]);
            st4<float>(a.dc0, o, dcc[j]);
        }
    }
}

template <int NG>
int launch_fwd_ng(const FwdArgs& a, hipStream_t s) {
    const size_t lds = (size_t)2 * 16 * (a.H + 4) * 4;
    static bool attr_set = false;                           // > 64 KB of dynamic LDS needs the attribute once per process
    if (!attr_set) {
        if (hipFuncSetAttribute((const void*)cfm_lstm_fwd_kernel<NG>, hipFuncAttributeMaxDynamicSharedMemorySize, 2 * 16 * (512 + 4) * 4) != hipSuccess)
            return cfm_fail(CFM_ERR_LAUNCH, "cfm_lstm_forward: cannot raise the dynamic LDS limit");
        attr_set = true;
    }
    CfmProfScope prof("lstm_fwd", s, 8.0 * a.B * (double)a.U * a.H * a.H, 4.0 * ((double)a.U * 4 * a.H * a.H * ((a.B + 15) / 16) + 10.0 * a.B * a.U * a.H));
    CFM_LAUNCH((cfm_lstm_fwd_kernel<NG>), dim3((unsigned)((a.B + 15) / 16)), dim3(LSTM_NT), lds, s, a);
    return cfm_launch_status("cfm_lstm_forward");
}

template <int NG>
int launch_bwd_ng(const BwdArgs& a, hipStream_t s) {
    const size_t lds = (size_t)16 * (4 * a.H + 4) * 4;
    static bool attr_set = false;
    if (!attr_set) {
        if (hipFuncSetAttribute((const void*)cfm_lstm_bwd_kernel<NG>, hipFuncAttributeMaxDynamicSharedMemorySize, 16 * (4 * 512 + 4) * 4) != hipSuccess)
            return cfm_fail(CFM_ERR_LAUNCH, "cfm_lstm_backward: cannot raise the dynamic LDS limit");
        attr_set = true;
    }
    CfmProfScope prof("lstm_bwd", s, 8.0 * a.B * (double)a.U * a.H * a.H, 4.0 * ((double)a.U * 4 * a.H * a.H * ((a.B + 15) / 16) + 11.0 * a.B * a.U * a.H));
    CFM_LAUNCH((cfm_lstm_bwd_kernel<NG>), dim3((unsigned)((a.B + 15) / 16)), dim3(LSTM_NT), lds, s, a);
    return cfm_launch_status("cfm_lstm_backward");
}

int launch_fwd(const FwdArgs& a, hipStream_t s) {
    switch ((a.H + 127) / 128) {
        case 1: return launch_fwd_ng<1>(a, s);
        case 2: return launch_fwd_ng<2>(a, s);
        case 3: return launch_fwd_ng<3>(a, s);
        default: return launch_fwd_ng<LSTM_MAXG>(a, s);
    }
}
int launch_bwd(const BwdArgs& a, hipStream_t s) {
    switch ((a.H + 127) / 128) {
        case 1: return launch_bwd_ng<1>(a, s);
        case 2: return launch_bwd_ng<2>(a, s);
        case 3: return launch_bwd_ng<3>(a, s);
        default: return launch_bwd_ng<LSTM_MAXG>(a, s);
    }
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

int check_desc(const cfm_lstm_desc* d, const char* who) {
    CFM_CHECK_ARG(d, "%s: null descriptor", who);
    CFM_CHECK_ARG(d->B >= 1 && d->U >= 1 && d->layers >= 1 && d->layers <= CFM_LSTM_MAX_LAYERS, "%s: B >= 1, U >= 1, 1..%d layers (B=%d U=%d layers=%d)", who,
                  CFM_LSTM_MAX_LAYERS, d->B, d->U, d->layers);
    CFM_CHECK_ARG(d->H >= 64 && d->H <= 512 && d->H % 64 == 0 && d->in >= 64 && d->in <= 512 && d->in % 64 == 0,
                  "%s: hidden and input size must be multiples of 64 up to 512 (in=%d H=%d)", who, d->in, d->H);
    CFM_CHECK_ARG((int64_t)d->B * d->U * 4 * d->H < (1ll << 31), "%s: B * U * 4H must stay below 2^31 (B=%d U=%d H=%d)", who, d->B, d->U, d->H);
    CFM_CHECK_ARG(d->drop_p >= 0.f && d->drop_p < 1.f, "%s: dropout probability %g outside [0, 1)", who, (double)d->drop_p);
    CFM_CHECK_ARG(d->x && aligned16(d->x), "%s: x is null or not 16-byte aligned", who);
    for (int l = 0; l < d->layers; ++l) {
        CFM_CHECK_ARG(d->w_ih[l] && d->w_hh[l] && d->save[l], "%s: layer %d: null weight or save block", who, l);
        CFM_CHECK_ARG(aligned16(d->w_ih[l]) && aligned16(d->w_hh[l]) && aligned16(d->b_ih[l]) && aligned16(d->b_hh[l]) && aligned16(d->save[l]),
                      "%s: layer %d: weights, biases and the save block must be 16-byte aligned", who, l);
    }
    CFM_CHECK_ARG(aligned16(d->h0) && aligned16(d->c0), "%s: h0 / c0 must be 16-byte aligned", who);
    return 0;
}

// the three parts of a layer's save block
struct SaveParts {
    float *ybuf, *cbuf, *gates;
};
SaveParts save_parts(float* block, int B, int U, int H) {
    const int64_t st = (int64_t)(U + 1) * B * H;
    return {block, block + st, block + 2 * st};
}

// seed of the dropout between layer l - 1 and layer l (the mask is indexed by the element offset in layer l - 1's time-major [U*B, H] output)
unsigned layer_seed(unsigned seed, int l) { return seed + 0x9E3779B1u * (unsigned)l; }

}  // namespace

extern "C" int64_t cfm_lstm_save_floats(int32_t B, int32_t U, int32_t H) { return 2 * (int64_t)(U + 1) * B * H + (int64_t)U * B * 4 * H; }

extern "C" int cfm_lstm_forward(const cfm_lstm_desc* d, cfm_stream_t stream) {
    if (int rc = check_desc(d, "cfm_lstm_forward")) return rc;
    CFM_CHECK_ARG(d->y && d->hn && d->cn && aligned16(d->y) && aligned16(d->hn) && aligned16(d->cn), "cfm_lstm_forward: y / hn / cn null or not 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    const int B = d->B, U = d->U, H = d->H, M = B * U;
    for (int l = 0; l < d->layers; ++l) {
        const SaveParts sv = save_parts(d->save[l], B, U, H);
        const int K = l == 0 ? d->in : H;
        MmArgs m = {};
        m.P = d->w_ih[l]; m.spi = K; m.spk = 1; m.sqj = K; m.sqk = 1; m.out = sv.gates; m.ldo = 4 * H; m.b1 = d->b_ih[l]; m.b2 = d->b_hh[l];
        m.I = 4 * H; m.J = M; m.Kc = K; m.rB = B; m.rU = U;
        if (l == 0) { m.Q = d->x; m.remap_qj = 1; }
        else {
            m.Q = save_parts(d->save[l - 1], B, U, H).ybuf + (int64_t)B * H;
            if (d->drop_p > 0.f) { m.drop_on = 2; m.drop = cfm_make_drop(d->drop_p, layer_seed(d->seed, l)); }
        }
        if (int rc = launch_mm(m, false, s, "lstm_in")) return rc;
        const int64_t so = (int64_t)l * B * H;
        FwdArgs f = {};
        f.w_hh = d->w_hh[l]; f.h0 = d->h0 ? d->h0 + so : nullptr; f.c0 = d->c0 ? d->c0 + so : nullptr;
        f.gates = sv.gates; f.ybuf = sv.ybuf; f.cbuf = sv.cbuf; f.y = l == d->layers - 1 ? d->y : nullptr; f.hn = d->hn + so; f.cn = d->cn + so;
        f.B = B; f.U = U; f.H = H;
        if (int rc = launch_fwd(f, s)) return rc;
    }
    return CFM_OK;
}

extern "C" int cfm_lstm_backward(const cfm_lstm_desc* d, cfm_stream_t stream) {
    if (int rc = check_desc(d, "cfm_lstm_backward")) return rc;
    CFM_CHECK_ARG(d->dy && d->dx && d->dh0 && d->dc0 && d->dg && aligned16(d->dy) && aligned16(d->dx) && aligned16(d->dh0) && aligned16(d->dc0) && aligned16(d->dg) &&
                      aligned16(d->dhn) && aligned16(d->dcn),
                  "cfm_lstm_backward: dy / dx / dh0 / dc0 / dg null, or a gradient not 16-byte aligned");
    CFM_CHECK_ARG(d->layers == 1 || (d->dyl && aligned16(d->dyl)), "cfm_lstm_backward: more than one layer needs the dyl work buffer");
    hipStream_t s = (hipStream_t)stream;
    const int B = d->B, U = d->U, H = d->H, M = B * U, L = d->layers;
    for (int l = L - 1; l >= 0; --l) {
        CFM_CHECK_ARG(d->dw_ih[l] && d->dw_hh[l] && aligned16(d->dw_ih[l]) && aligned16(d->dw_hh[l]), "cfm_lstm_backward: layer %d: weight gradient null or not 16-byte aligned", l);
        const SaveParts sv = save_parts(d->save[l], B, U, H);
        const int K = l == 0 ? d->in : H;
        const int64_t so = (int64_t)l * B * H;
        BwdArgs r = {};
        r.w_hh = d->w_hh[l]; r.gates = sv.gates; r.cbuf = sv.cbuf; r.dhn = d->dhn ? d->dhn + so : nullptr; r.dcn = d->dcn ? d->dcn + so : nullptr;
        if (l == L - 1) { r.dy = d->dy; r.dy_sb = (int64_t)U * H; r.dy_st = H; }
        else { r.dy = d->dyl; r.dy_sb = H; r.dy_st = (int64_t)B * H; }
        r.dg = d->dg; r.dh0 = d->dh0 + so; r.dc0 = d->dc0 + so; r.B = B; r.U = U; r.H = H;
        if (int rc = launch_bwd(r, s)) return rc;
        const bool drop = l > 0 && d->drop_p > 0.f;
        const CfmDrop dr = cfm_make_drop(d->drop_p, layer_seed(d->seed, l));
        const float* xin = l == 0 ? d->x : save_parts(d->save[l - 1], B, U, H).ybuf + (int64_t)B * H;
        // dW_ih[n, k] = sum_m dg[m, n] drop(x)[m, k];  dW_hh[n, k] = sum_m dg[m, n] h_prev[m, k]
        MmArgs w = {};
        w.P = xin; w.spi = 1; w.spk = K; w.Q = d->dg; w.sqj = 1; w.sqk = 4 * H; w.out = d->dw_ih[l]; w.ldo = K; w.I = K; w.J = 4 * H; w.Kc = M; w.rB = B; w.rU = U;
        if (l == 0) w.remap_pk = 1;
        else if (drop) { w.drop_on = 1; w.drop = dr; }
        if (int rc = launch_mm(w, true, s, "lstm_dw_ih")) return rc;
        MmArgs h = {};
        h.P = sv.ybuf; h.spi = 1; h.spk = H; h.Q = d->dg; h.sqj = 1; h.sqk = 4 * H; h.out = d->dw_hh[l]; h.ldo = H; h.I = H; h.J = 4 * H; h.Kc = M; h.rB = B; h.rU = U;
        if (int rc = launch_mm(h, true, s, "lstm_dw_hh")) return rc;
        if (d->db_ih[l] || d->db_hh[l]) {
            CfmProfScope prof("lstm_db", s, 0.0, 4.0 * M * 4 * H);
            CFM_LAUNCH(cfm_lstm_colsum_kernel, dim3((unsigned)(4 * H / 64)), dim3(1024), 0, s, (const float*)d->dg, M, 4 * H, d->db_ih[l], d->db_hh[l]);
            if (int rc = cfm_launch_status("cfm_lstm_backward(bias)")) return rc;
        }
        // dx[m, k] = sum_n dg[m, n] W_ih[n, k]: layer 0 writes torch's [B, U, in]; the others the next reverse recurrence's dy, through the mask
        MmArgs x = {};
        x.P = d->w_ih[l]; x.spi = 1; x.spk = K; x.Q = d->dg; x.sqj = 4 * H; x.sqk = 1; x.ldo = K; x.I = K; x.J = M; x.Kc = 4 * H; x.rB = B; x.rU = U;
        if (l == 0) { x.out = d->dx; x.remap_oj = 1; }
        else {
            x.out = d->dyl;
            if (drop) { x.drop_on = 3; x.drop = dr; }
        }
        if (int rc = launch_mm(x, false, s, "lstm_dx")) return rc;
    }
    return CFM_OK;
}
