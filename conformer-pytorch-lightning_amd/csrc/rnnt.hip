// rnnt.hip -- RNN-T loss (Graves 2012) and its gradient with respect to the joint's logits (gfx950).
//
// replaces torchaudio.functional.rnnt_loss(joint_out, rnnt_text, encoder_out_lens, rnnt_text_lengths, blank, reduction) of
// Transducer.rnnt_loss (reference src/model.py:107) with fused_log_softmax = True: logits [B, T, U+1, ld >= V] (f32 / bf16 / fp16), all
// arithmetic f32, no float atomics (the same inputs give the same bits on every run).
//
// Three launches (cfm_rnnt_nll: rows + recursions; cfm_rnnt_grad: gradient):
//   rows   one wavefront per lattice node (b, t < T_b, u <= U_b): lse = log sum_v exp(L[v]) in ONE pass over the row (online max-shifted
//          sum, 16-byte loads for f32), lp_blank = L[blank] - lse, lp_label = L[y_{u+1}] - lse (u < U_b) -> compact f32 [B, T, U+1];
//   alpha | beta   2 B workgroups, [0, B) forwards, [B, 2B) backwards, one anti-diagonal (d = t + u) per step with thread = u:
//              alpha[t,u] = logaddexp(alpha[t-1,u] + lp_blank[t-1,u], alpha[t,u-1] + lp_label[t,u-1])
//              beta[t,u]  = logaddexp(beta[t+1,u] + lp_blank[t,u], beta[t,u+1] + lp_label[t,u]),  beta[T_b-1,U_b] = lp_blank[T_b-1,U_b]
//          A thread's own column is in a register; the neighbour's value of the previous diagonal comes through an LDS double buffer with
//          one barrier per diagonal (U+1 <= 1024).  The lattice inputs do not
//          depend on alpha / beta and are requested RNNT_AHEAD diagonals before they are used (as ctc.hip does).
//          Shifted recursion (the CTC precedent): every blank of frame t is offset by o_t = max_u lp_blank[t,u] and every emission of label
//          u+1 by q_u = max_t lp_label[t,u].  Each path to (t,u) takes exactly one blank per frame < t and one emission per label <= u, so
//          alpha' = alpha - sum_{t'<t} o - sum_{u'<u} q exactly, and alpha' + beta' - ll' = alpha + beta - ll: the posteriors do not depend
//          on the shift, but alpha' / beta' stay small numbers where the unshifted ones grow by ~log V per step (|alpha| ~ 2500 at config 4,
//          one f32 ulp = 2.4e-4 in the log domain, a 1e-3 error in every posterior).  nll = -(beta'[0,0] + sum o + sum q), the sums in fp64.
//   grad   one wavefront per row over all B T (U+1) rows:
//              g[v] = s_b * clamp( exp(L[v] - lse + alpha + beta - ll) - [v = blank] exp(alpha + lp_blank + beta[t+1,u] - ll)
//                                                                     - [v = y_{u+1}] exp(alpha + lp_label + beta[t,u+1] - ll) )
//          (clamped before the upstream scale, as torchaudio does), exact zeros outside t < T_b, u <= U_b and in the columns V..grad_cols-1.
//          The output may alias the logits: each lane writes only bytes of its row that the wavefront has already read (same element size:
//          the same bytes; a 16-bit gradient over f32 logits: the first half of the row), so the pointers are not declared __restrict__.
//
// Packed lattices (cfm_rnnt_packed_nll / _grad, include/cfm.h cfm_lattice): the same three kernels, instantiated on cfm_rnnt_packed_desc.  Only the
// valid nodes have rows (utterance b: rows off[b] + t (U_b+1) + u), so the row and gradient passes launch over M = sum T_b (U_b+1) rows and find
// their utterance by a binary search over off (B is a few hundred at most: <= 9 probes of an L2-resident array, next to a V-wide row).  The
// per-node code is shared through utt_geo (where utterance b's nodes live): a node's arithmetic, and so each cost, is the same bits either way.
#include "cfm_common.h"

namespace {

constexpr int RNNT_NT = 256;                               // up to 4 columns per thread
constexpr int RNNT_MAXU1 = 1024;                           // U + 1
constexpr int RNNT_MAXT = 8192;                            // o_t lives in LDS
constexpr int RNNT_AHEAD = 4;

__device__ __forceinline__ int label_at(const int* __restrict__ tg, int u, int V) {
    const int y = tg[u];                                   // labels outside [0, V) cannot index a row: clamped (torchaudio would raise)
    return y < 0 ? 0 : (y < V ? y : V - 1);
}

// where utterance b's nodes live: node (t, u) at base + t * ld + u (t < Tb, u <= Ub); o_t at shift[t], q_u at shift[qoff + u]; labels at tg[u]
struct UttGeo {
    int64_t base;
    int ld, Tb, Ub;
    float* shift;
    int qoff;
    const int32_t* tg;
};

__host__ __device__ __forceinline__ int n_utt(const cfm_rnnt_desc& d) { return d.B; }
__host__ __device__ __forceinline__ int n_utt(const cfm_rnnt_packed_desc& d) { return d.lat.B; }

__device__ __forceinline__ UttGeo utt_geo(const cfm_rnnt_desc& d, int b) {
    return {(int64_t)b * d.T * d.U1, d.U1, min(max(d.logit_lens[b], 0), d.T), min(max(d.target_lens[b], 0), d.U1 - 1),
            d.shift + (int64_t)b * (d.T + d.U1), d.T, d.targets + (int64_t)b * (d.U1 - 1)};
}

__device__ __forceinline__ UttGeo utt_geo(const cfm_rnnt_packed_desc& d, int b) {
    const int Ub = d.lat.U[b];
    return {d.lat.off[b], Ub + 1, d.lat.T[b], Ub, d.shift + (int64_t)b * (d.lat.T_max + d.lat.U1_max), d.lat.T_max, d.targets + (int64_t)b * d.ld_targets};
}

// row r -> (b, t, u); padded: every (b, t < T, u < U1) has a row (the caller checks t < Tb, u <= Ub); packed: the last b with off[b] <= r
__device__ __forceinline__ void locate(const cfm_rnnt_desc& d, int64_t r, int& b, int& t, int& u) {
    b = (int)(r / ((int64_t)d.T * d.U1));
    const int rem = (int)(r - (int64_t)b * d.T * d.U1);
    t = rem / d.U1;
    u = rem - t * d.U1;
}

__device__ __forceinline__ void locate(const cfm_rnnt_packed_desc& d, int64_t r, int& b, int& t, int& u) {
    b = last_le(d.lat.off, d.lat.B, r);                    // r >= 0 = off[0]: never -1
    const int U1 = d.lat.U[b] + 1;
    const int rem = (int)(r - d.lat.off[b]);
    t = rem / U1;
    u = rem - t * U1;
}

__host__ __device__ __forceinline__ int64_t n_rows(const cfm_rnnt_desc& d) { return (int64_t)d.B * d.T * d.U1; }
__host__ __device__ __forceinline__ int64_t n_rows(const cfm_rnnt_packed_desc& d) { return d.lat.M; }

// ---- rows: grid = ceil(B T U1 / 4) workgroups of 4 wavefronts, wavefront = one node ----
template <typename D, typename TI, bool VEC>
__global__ __launch_bounds__(256) void cfm_rnnt_rows_kernel(D d) {
    const int lane = threadIdx.x & 63;
    const int64_t row_id = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int V = d.V;
    if (row_id >= n_rows(d)) return;
    int b, t, u;
    locate(d, row_id, b, t, u);
    const UttGeo g = utt_geo(d, b);
    const int Ub = g.Ub;
    if (t >= g.Tb || u > Ub) return;                       // never read by the recursions or the gradient pass (wavefront-uniform)
    const void* row = (const char*)d.logits + row_id * d.ld * (cfm_is_f32<TI> ? 4 : 2);
    float m = -INFINITY, s = 0.f;                          // online log-sum-exp: the row is read once
    if constexpr (VEC) {
        for (int c = lane * 4; c < V; c += 256) {
            if (c + 3 < V) {
                const f32x4 v = ld4<TI>(row, c);
                const float cm = fmaxf(fmaxf(v.x, v.y), fmaxf(v.z, v.w));
                if (cm > m) {
                    s *= __expf(m - cm);
                    m = cm;
                }
                if (m > -INFINITY) s += (__expf(v.x - m) + __expf(v.y - m)) + (__expf(v.z - m) + __expf(v.w - m));
            } else {
                for (int k = c; k < V; ++k) {
                    const float x = ld1<TI>(row, k);
                    if (x > m) {
                        s *= __expf(m - x);
                        m = x;
                    }
                    if (m > -INFINITY) s += __expf(x - m);
                }
            }
        }
    } else {
        for (int c = lane; c < V; c += 64) {
            const float x = ld1<TI>(row, c);
            if (x > m) {
                s *= __expf(m - x);
                m = x;
            }
            if (m > -INFINITY) s += __expf(x - m);
        }
    }
    const float M = wave_max(m);
    const float tot = wave_sum(m == -INFINITY ? 0.f : s * __expf(m - M));
    const float lse = M + __logf(tot);
    if (lane == 0) {
        d.lse[row_id] = lse;
        d.lp_blank[row_id] = ld1<TI>(row, d.blank) - lse;
        d.lp_label[row_id] = u < Ub ? ld1<TI>(row, label_at(g.tg, u, V)) - lse : -INFINITY;
    }
}

// the shifts of one utterance into LDS (no barrier): o_t over the valid columns (a wavefront per frame), q_u over the valid frames (a thread per label)
template <int NT>
__device__ __forceinline__ void rnnt_shifts(const float* lb, const float* ll, const int U1, const int Tb, const int Ub, float* sh_o, float* sh_q) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int t = wave; t < Tb; t += NT / 64) {
        float m = -INFINITY;
        for (int u = lane; u <= Ub; u += 64) m = fmaxf(m, lb[(int64_t)t * U1 + u]);
        m = wave_max(m);
        if (lane == 0) sh_o[t] = m > -INFINITY ? m : 0.f;
    }
    for (int u = tid; u < Ub; u += NT) {
        float m0 = -INFINITY, m1 = -INFINITY, m2 = -INFINITY, m3 = -INFINITY;
        int t = 0;
        for (; t + 3 < Tb; t += 4) {
            m0 = fmaxf(m0, ll[(int64_t)t * U1 + u]);
            m1 = fmaxf(m1, ll[(int64_t)(t + 1) * U1 + u]);
            m2 = fmaxf(m2, ll[(int64_t)(t + 2) * U1 + u]);
            m3 = fmaxf(m3, ll[(int64_t)(t + 3) * U1 + u]);
        }
        for (; t < Tb; ++t) m0 = fmaxf(m0, ll[(int64_t)t * U1 + u]);
        const float m = fmaxf(fmaxf(m0, m1), fmaxf(m2, m3));
        sh_q[u] = m > -INFINITY ? m : 0.f;
    }
}

// ---- alpha | beta: one workgroup per (utterance, direction), PER columns per thread, the neighbour column through LDS ----
template <int NT, int PER, typename Desc>
__device__ __forceinline__ void rnnt_sweep(const Desc& d, const int b, const bool fwd) {
    __shared__ float sh_o[RNNT_MAXT];
    __shared__ float sh_q[RNNT_MAXU1];
    __shared__ float pub[2][RNNT_MAXU1 + 2];
    __shared__ double red[NT];
    const int tid = threadIdx.x;
    const UttGeo g = utt_geo(d, b);
    const int U1 = g.ld, Tb = g.Tb, Ub = g.Ub;
    if (Tb == 0) {                                         // no frame: no alignment (torchaudio rejects it); +inf, zero gradient
        if (tid == 0) {
            if (fwd) d.ll_alpha[b] = -INFINITY;
            else d.nll[b] = d.nll_shifted[b] = INFINITY;
        }
        return;
    }
    const int64_t base = g.base;
    const float* lb = d.lp_blank + base;
    const float* ll = d.lp_label + base;
    rnnt_shifts<NT>(lb, ll, U1, Tb, Ub, sh_o, sh_q);
    for (int i = tid; i < RNNT_MAXU1 + 2; i += NT) pub[0][i] = pub[1][i] = -INFINITY;
    __syncthreads();
    float* shift = g.shift;
    if (fwd) {                                             // the gradient pass reads the shifts from here
        for (int t = tid; t < Tb; t += NT) shift[t] = sh_o[t];
        for (int u = tid; u < Ub; u += NT) shift[g.qoff + u] = sh_q[u];
    }
    float* out = (fwd ? d.alpha : d.beta) + base;
    const int D = Tb + Ub;                                 // diagonals 0 .. Tb-1+Ub
    float self[PER], lbp[PER];
    float nb[RNNT_AHEAD][PER], nl[RNNT_AHEAD][PER];
    auto fetch = [&](int step, int i, float& vb, float& vl) {
        const int u = tid + i * NT, dd = fwd ? step : D - 1 - step, t = dd - u;
        const bool ok = step < D && u <= Ub && t >= 0 && t < Tb;
        vb = ok ? lb[(int64_t)t * U1 + u] - sh_o[t] : 0.f;
        vl = (ok && u < Ub) ? ll[(int64_t)t * U1 + u] - sh_q[u] : -INFINITY;
    };
#pragma unroll
    for (int i = 0; i < PER; ++i) {
        self[i] = -INFINITY;
        lbp[i] = 0.f;
#pragma unroll
        for (int k = 0; k < RNNT_AHEAD; ++k) fetch(k, i, nb[k][i], nl[k][i]);
    }
    for (int s0 = 0; s0 < D; s0 += RNNT_AHEAD) {
#pragma unroll
        for (int k = 0; k < RNNT_AHEAD; ++k) {
            const int step = s0 + k;
            if (step < D) {                                // uniform
                const int dd = fwd ? step : D - 1 - step;
#pragma unroll
                for (int i = 0; i < PER; ++i) {
                    const int u = tid + i * NT, t = dd - u;
                    // the neighbour column's value of the previous diagonal
                    const float nbr = fwd ? pub[(step + 1) & 1][u] : pub[(step + 1) & 1][u + 1];
                    float v = -INFINITY;
                    if (u <= Ub && t >= 0 && t < Tb) {
                        if (fwd) {
                            const float a = (t == 0 && u == 0) ? 0.f : logaddexp_(self[i] + lbp[i], nbr);
                            out[(int64_t)t * U1 + u] = a;
                            self[i] = a;
                            lbp[i] = nb[k][i];
                            v = a + nl[k][i];                              // -inf at u = Ub
                            if (t == Tb - 1 && u == Ub) d.ll_alpha[b] = a + nb[k][i];
                        } else {
                            const float bt = (t == Tb - 1 && u == Ub) ? nb[k][i] : logaddexp_(self[i] + nb[k][i], nbr + nl[k][i]);
                            out[(int64_t)t * U1 + u] = bt;
                            self[i] = bt;
                            v = bt;
                        }
                    }
                    pub[step & 1][fwd ? u + 1 : u] = v;
                    fetch(step + RNNT_AHEAD, i, nb[k][i], nl[k][i]);
                }
                __syncthreads();
            }
        }
    }
    if (fwd) return;
    double part = 0.0;                                     // sum o + sum q in fp64, a fixed order
    for (int t = tid; t < Tb; t += NT) part += (double)sh_o[t];
    for (int u = tid; u < Ub; u += NT) part += (double)sh_q[u];
    red[tid] = part;
    __syncthreads();                                       // also: beta[0,0] (thread 0's column) is final
    if (tid == 0) {
        double tot = 0.0;
        for (int i = 0; i < NT; ++i) tot += red[i];
        const float b00 = self[0];                         // thread 0 owns u = 0; its last value is beta'[0,0]
        d.nll_shifted[b] = -b00;
        d.nll[b] = (float)(-((double)b00 + tot));
    }
}

template <int NT, int PER, typename D>
__global__ __launch_bounds__(NT) void cfm_rnnt_alpha_beta_kernel(D d) {
    const int wg = (int)blockIdx.x, B = n_utt(d);
    if (wg < B) rnnt_sweep<NT, PER>(d, wg, true);
    else rnnt_sweep<NT, PER>(d, wg - B, false);
}

// ---- forced alignment: the max-plus (Viterbi) twin of the forward sweep, one workgroup per utterance ----
// delta'[t,u] = max(delta'[t-1,u] + lp_blank'[t-1,u], delta'[t,u-1] + lp_label'[t,u-1]) on the shifted values of the loss (every path to (t,u)
// takes the same offsets, so no decision moves); the blank move first, the label move only where it is STRICTLY greater (at t = 0 it is the only
// move).  Recorded per node: ent[t,u] = the last frame t' <= t at which column u was entered by a label move -- a column thread's running
// register, stored as int16 (T <= 8192).  The trace-back is then one dependent load per LABEL, not per move: from (Tb-1, Ub),
// frame[u-1] = t = ent[t,u], down to u = 1.  By construction 0 <= ent[t,u] <= t, so the walk cannot leave the lattice.
__host__ __device__ __forceinline__ int align_ld(const cfm_rnnt_desc& d) { return d.U1 - 1; }
__host__ __device__ __forceinline__ int align_ld(const cfm_rnnt_packed_desc& d) { return d.lat.U1_max - 1; }

template <int NT, int PER, typename AD>
__global__ __launch_bounds__(NT) void cfm_rnnt_viterbi_kernel(AD ad) {
    __shared__ float sh_o[RNNT_MAXT];
    __shared__ float sh_q[RNNT_MAXU1];
    __shared__ float pub[2][RNNT_MAXU1 + 2];
    __shared__ double red[NT];
    __shared__ float sh_end;
    const auto& d = ad.r;
    const int tid = threadIdx.x, b = (int)blockIdx.x;
    const UttGeo g = utt_geo(d, b);
    const int U1 = g.ld, Tb = g.Tb, Ub = g.Ub, W = align_ld(d);
    int32_t* frame = ad.frame + (int64_t)b * W;
    float* tlp = ad.token_logp + (int64_t)b * W;
    for (int u = (Tb > 0 ? Ub : 0) + tid; u < W; u += NT) {     // beyond the labels; everything when there is no alignment
        frame[u] = -1;
        tlp[u] = -INFINITY;
    }
    if (Tb == 0) {                                         // the final blank needs a frame
        if (tid == 0) ad.score[b] = -INFINITY;
        return;
    }
    const int64_t base = g.base;
    const float* lb = d.lp_blank + base;
    const float* ll = d.lp_label + base;
    int16_t* ent = (int16_t*)ad.scratch + base;
    rnnt_shifts<NT>(lb, ll, U1, Tb, Ub, sh_o, sh_q);
    for (int i = tid; i < RNNT_MAXU1 + 2; i += NT) pub[0][i] = pub[1][i] = -INFINITY;
    __syncthreads();
    const int D = Tb + Ub;                                 // diagonals 0 .. Tb-1+Ub
    float self[PER], lbp[PER];
    int entered[PER];
    float nb[RNNT_AHEAD][PER], nl[RNNT_AHEAD][PER];
    auto fetch = [&](int step, int i, float& vb, float& vl) {
        const int u = tid + i * NT, t = step - u;
        const bool ok = step < D && u <= Ub && t >= 0 && t < Tb;
        vb = ok ? lb[(int64_t)t * U1 + u] - sh_o[t] : 0.f;
        vl = (ok && u < Ub) ? ll[(int64_t)t * U1 + u] - sh_q[u] : -INFINITY;
    };
#pragma unroll
    for (int i = 0; i < PER; ++i) {
        self[i] = -INFINITY;
        lbp[i] = 0.f;
        entered[i] = 0;
#pragma unroll
        for (int k = 0; k < RNNT_AHEAD; ++k) fetch(k, i, nb[k][i], nl[k][i]);
    }
    for (int s0 = 0; s0 < D; s0 += RNNT_AHEAD) {
#pragma unroll
        for (int k = 0; k < RNNT_AHEAD; ++k) {
            const int step = s0 + k;
            if (step < D) {                                // uniform
#pragma unroll
                for (int i = 0; i < PER; ++i) {
                    const int u = tid + i * NT, t = step - u;
                    const float nbr = pub[(step + 1) & 1][u];                  // delta'[t,u-1] + lp_label'[t,u-1]; -inf at u = 0
                    float v = -INFINITY;
                    if (u <= Ub && t >= 0 && t < Tb) {
                        const float cb = self[i] + lbp[i];
                        const bool label = t == 0 ? u > 0 : nbr > cb;
                        const float a = (t == 0 && u == 0) ? 0.f : (label ? nbr : cb);
                        if (label) entered[i] = t;
                        ent[(int64_t)t * U1 + u] = (int16_t)entered[i];
                        self[i] = a;
                        lbp[i] = nb[k][i];
                        v = a + nl[k][i];                                      // -inf at u = Ub
                        if (t == Tb - 1 && u == Ub) sh_end = a + nb[k][i];
                    }
                    pub[step & 1][u + 1] = v;
                    fetch(step + RNNT_AHEAD, i, nb[k][i], nl[k][i]);
                }
                __syncthreads();
            }
        }
    }
    double part = 0.0;                                     // sum o + sum q in fp64, a fixed order (as the loss)
    for (int t = tid; t < Tb; t += NT) part += (double)sh_o[t];
    for (int u = tid; u < Ub; u += NT) part += (double)sh_q[u];
    red[tid] = part;
    __syncthreads();                                       // the loop's last barrier already ordered sh_end and every ent store
    if (tid != 0) return;
    double tot = 0.0;
    for (int i = 0; i < NT; ++i) tot += red[i];
    ad.score[b] = (float)((double)sh_end + tot);
    int t = Tb - 1;
    for (int u = Ub; u > 0; --u) {                         // Ub dependent loads
        t = ent[(int64_t)t * U1 + u];
        frame[u - 1] = t;
        tlp[u - 1] = ll[(int64_t)t * U1 + u - 1];
    }
}

// ---- gradient: one wavefront per row (b, t, u), all rows ----
template <typename D, typename TI, typename TO, bool VEC>
__global__ __launch_bounds__(256) void cfm_rnnt_grad_kernel(D d) {
    const int lane = threadIdx.x & 63;
    const int64_t row_id = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int V = d.V, ncols = d.grad_cols;
    if (row_id >= n_rows(d)) return;
    int b, t, u;
    locate(d, row_id, b, t, u);
    const UttGeo g = utt_geo(d, b);
    const int U1 = g.ld, Tb = g.Tb, Ub = g.Ub;
    const void* row = (const char*)d.logits + row_id * d.ld * (cfm_is_f32<TI> ? 4 : 2);
    void* grow = (char*)d.grad + row_id * d.ld_grad * (cfm_is_f32<TO> ? 4 : 2);
    const float nls = d.nll_shifted[b];
    if (t >= Tb || u > Ub || !(nls < INFINITY)) {          // outside the lattice (or no alignment): exact zeros
        if constexpr (VEC) {
            for (int c = lane * 4; c < ncols; c += 256) st4<TO>(grow, c, (f32x4){0.f, 0.f, 0.f, 0.f});
        } else {
            for (int c = lane; c < ncols; c += 64) st1<TO>(grow, c, 0.f);
        }
        return;
    }
    const int64_t node = g.base + (int64_t)t * U1 + u;
    const float* shift = g.shift;
    const float ll = -nls, a = d.alpha[node];
    const float lse = d.lse[node];
    const float c0 = lse - (a + d.beta[node] - ll);                  // exp(L[v] - c0) = softmax[v] * posterior of the node
    const float lbs = d.lp_blank[node] - shift[t];                   // the recursion's own shifted values, bit for bit
    const float bnext = t + 1 < Tb ? d.beta[node + U1] : (u == Ub ? 0.f : -INFINITY);
    const float cb = __expf(a + lbs + bnext - ll);
    float cl = 0.f;
    int y = -1;
    if (u < Ub) {
        y = label_at(g.tg, u, V);
        cl = __expf(a + (d.lp_label[node] - shift[g.qoff + u]) + d.beta[node + 1] - ll);
    }
    const int blank = d.blank;
    const float gs = d.gscale * (d.gscale_dev ? d.gscale_dev[(int64_t)b * d.gscale_stride] : 1.f);
    const float cl_ = d.clamp;
    auto g1 = [&](int v, float x) {
        float g = __expf(x - c0) - (v == blank ? cb : 0.f) - (v == y ? cl : 0.f);
        if (cl_ > 0.f) g = fminf(fmaxf(g, -cl_), cl_);
        return gs * g;
    };
    if constexpr (VEC) {
        for (int c = lane * 4; c < ncols; c += 256) {
            f32x4 g;
            if (c + 3 < V) {
                const f32x4 x = ld4<TI>(row, c);
#pragma unroll
                for (int e = 0; e < 4; ++e) g[e] = g1(c + e, x[e]);
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e) g[e] = c + e < V ? g1(c + e, ld1<TI>(row, c + e)) : 0.f;
            }
            st4<TO>(grow, c, g);
        }
    } else {
        for (int c = lane; c < ncols; c += 64) st1<TO>(grow, c, c < V ? g1(c, ld1<TI>(row, c)) : 0.f);
    }
}

// loss: the entries that run the alpha / beta recursions; the alignment reads neither those arrays nor the costs
int rnnt_check(const cfm_rnnt_desc* d, const char* what, const bool loss = true) {
    CFM_CHECK_ARG(d && d->logits && d->logit_lens && d->target_lens && d->lse && d->lp_blank && d->lp_label &&
                  (!loss || (d->alpha && d->beta && d->shift && d->nll && d->nll_shifted)), "%s: null pointer", what);
    CFM_CHECK_ARG(d->B > 0 && d->T > 0 && d->U1 > 0 && d->V > 1, "%s: bad shape B=%d T=%d U+1=%d V=%d", what, d->B, d->T, d->U1, d->V);
    CFM_CHECK_ARG(d->U1 <= RNNT_MAXU1, "%s: U+1 = %d exceeds %d", what, d->U1, RNNT_MAXU1);
    CFM_CHECK_ARG(d->T <= RNNT_MAXT, "%s: T = %d frames exceeds %d", what, d->T, RNNT_MAXT);
    CFM_CHECK_ARG(d->U1 == 1 || d->targets, "%s: targets is null", what);
    CFM_CHECK_ARG(d->blank >= 0 && d->blank < d->V, "%s: blank %d outside [0, %d)", what, d->blank, d->V);
    CFM_CHECK_ARG(d->ld >= d->V, "%s: row stride %lld < V = %d", what, (long long)d->ld, d->V);
    CFM_CHECK_ARG(d->logits_dtype >= CFM_F32 && d->logits_dtype <= CFM_F16, "%s: bad logits dtype", what);
    return CFM_OK;
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

template <typename D, typename TI>
int launch_rows(const D& d, hipStream_t s, CfmProfScope& prof) {
    const int64_t rows = n_rows(d);
    const dim3 grid((unsigned)((rows + 3) / 4));
    const bool vec = d.ld % 4 == 0 && (cfm_is_f32<TI> ? aligned16(d.logits) : ((uintptr_t)d.logits & 7) == 0);
    if (vec) CFM_LAUNCH((cfm_rnnt_rows_kernel<D, TI, true>), grid, dim3(256), 0, s, d);
    else CFM_LAUNCH((cfm_rnnt_rows_kernel<D, TI, false>), grid, dim3(256), 0, s, d);
    return CFM_OK;
}

template <typename D, typename TI, typename TO>
int launch_grad(const D& d, hipStream_t s, CfmProfScope& prof) {
    const int64_t rows = n_rows(d);
    const dim3 grid((unsigned)((rows + 3) / 4));
    const bool in_ok = cfm_is_f32<TI> ? aligned16(d.logits) : ((uintptr_t)d.logits & 7) == 0;
    const bool out_ok = cfm_is_f32<TO> ? aligned16(d.grad) : ((uintptr_t)d.grad & 7) == 0;
    const bool vec = d.ld % 4 == 0 && d.ld_grad % 4 == 0 && d.grad_cols % 4 == 0 && in_ok && out_ok;
    if (vec) CFM_LAUNCH((cfm_rnnt_grad_kernel<D, TI, TO, true>), grid, dim3(256), 0, s, d);
    else CFM_LAUNCH((cfm_rnnt_grad_kernel<D, TI, TO, false>), grid, dim3(256), 0, s, d);
    return CFM_OK;
}

template <typename D, typename TI>
int launch_grad_out(const D& d, hipStream_t s, CfmProfScope& prof) {
    return cfm_by_dtype(d.grad_dtype, [&](auto to) { return launch_grad<D, TI, decltype(to)>(d, s, prof); });
}

int rnnt_packed_check(const cfm_rnnt_packed_desc* d, const char* what, const bool loss = true) {
    CFM_CHECK_ARG(d && d->logits && d->lat.off && d->lat.T && d->lat.U && d->lse && d->lp_blank && d->lp_label &&
                  (!loss || (d->alpha && d->beta && d->shift && d->nll && d->nll_shifted)), "%s: null pointer", what);
    const cfm_lattice& L = d->lat;
    CFM_CHECK_ARG(L.B > 0 && L.M >= 0 && L.T_max >= 0 && L.U1_max > 0 && d->V > 1, "%s: bad shape B=%d M=%lld T_max=%d U1_max=%d V=%d", what, L.B,
                  (long long)L.M, L.T_max, L.U1_max, d->V);
    CFM_CHECK_ARG(L.U1_max <= RNNT_MAXU1, "%s: U+1 = %d exceeds %d", what, L.U1_max, RNNT_MAXU1);
    CFM_CHECK_ARG(L.T_max <= RNNT_MAXT, "%s: T = %d frames exceeds %d", what, L.T_max, RNNT_MAXT);
    CFM_CHECK_ARG(L.U1_max == 1 || (d->targets && d->ld_targets >= L.U1_max - 1), "%s: targets is null or ld_targets < U1_max - 1", what);
    CFM_CHECK_ARG(d->blank >= 0 && d->blank < d->V, "%s: blank %d outside [0, %d)", what, d->blank, d->V);
    CFM_CHECK_ARG(d->ld >= d->V, "%s: row stride %lld < V = %d", what, (long long)d->ld, d->V);
    CFM_CHECK_ARG(d->logits_dtype >= CFM_F32 && d->logits_dtype <= CFM_F16, "%s: bad logits dtype", what);
    return CFM_OK;
}

template <typename D>
int rnnt_rows_launch(const D& d, const char* what, hipStream_t s) {
    const int64_t rows = n_rows(d);
    if (rows == 0) return CFM_OK;                          // a packed lattice may have no node at all (every T_b = 0)
    CfmProfScope prof("rnnt_rows", s, 0.0, (double)rows * d.V * cfm_elt_size(d.logits_dtype));
    int rc = cfm_by_dtype(d.logits_dtype, [&](auto ti) { return launch_rows<D, decltype(ti)>(d, s, prof); });
    if (rc) return rc;
    return cfm_launch_status(what);
}

template <typename D>
int rnnt_nll_launch(const D& d, const char* what, hipStream_t s) {
    const int64_t rows = n_rows(d);
    if (int rc = rnnt_rows_launch(d, what, s)) return rc;
    CfmProfScope prof("rnnt_alpha_beta", s, 0.0, (double)rows * 4 * 6);
    CFM_LAUNCH((cfm_rnnt_alpha_beta_kernel<RNNT_NT, RNNT_MAXU1 / RNNT_NT, D>), dim3(2 * n_utt(d)), dim3(RNNT_NT), 0, s, d);
    return cfm_launch_status(what);
}

template <typename D>
int rnnt_grad_launch(const D& d, const char* what, hipStream_t s) {
    CFM_CHECK_ARG(d.grad, "%s: null gradient", what);
    CFM_CHECK_ARG(d.grad_dtype >= CFM_F32 && d.grad_dtype <= CFM_F16, "%s: bad gradient dtype", what);
    CFM_CHECK_ARG(d.grad_cols >= d.V && d.ld_grad >= d.grad_cols, "%s: grad_cols %d must be in [V, ld_grad] (V = %d, ld_grad = %lld)", what,
                  d.grad_cols, d.V, (long long)d.ld_grad);
    if (d.grad == d.logits)                                // in place: each row's gradient must fit the bytes of its own row
        CFM_CHECK_ARG(d.ld_grad * cfm_elt_size(d.grad_dtype) == d.ld * cfm_elt_size(d.logits_dtype) &&
                      cfm_elt_size(d.grad_dtype) <= cfm_elt_size(d.logits_dtype), "%s: in place needs the same row bytes and a gradient no wider than the logits", what);
    const int64_t rows = n_rows(d);
    if (rows == 0) return CFM_OK;
    CfmProfScope prof("rnnt_grad", s, 0.0, (double)rows * ((double)d.V * cfm_elt_size(d.logits_dtype) + (double)d.grad_cols * cfm_elt_size(d.grad_dtype)));
    int rc = cfm_by_dtype(d.logits_dtype, [&](auto ti) { return launch_grad_out<D, decltype(ti)>(d, s, prof); });
    if (rc) return rc;
    return cfm_launch_status(what);
}

// the alignment's own arguments, after the embedded descriptor passed its check; then the row pass as the loss runs it and the Viterbi launch
template <typename AD>
int rnnt_align_launch(const AD& ad, const char* what, hipStream_t s) {
    const int64_t rows = n_rows(ad.r);
    CFM_CHECK_ARG(ad.score && (align_ld(ad.r) == 0 || (ad.frame && ad.token_logp)) && (rows == 0 || ad.scratch), "%s: null pointer", what);
    CFM_CHECK_ARG(ad.scratch_bytes >= cfm_rnnt_align_scratch_bytes(rows), "%s: scratch of %lld bytes, cfm_rnnt_align_scratch_bytes = %lld needed", what,
                  (long long)ad.scratch_bytes, (long long)cfm_rnnt_align_scratch_bytes(rows));
    CFM_CHECK_ARG(((uintptr_t)ad.scratch & 1) == 0, "%s: scratch must be 2-byte aligned", what);
    if (int rc = rnnt_rows_launch(ad.r, what, s)) return rc;
    CfmProfScope prof("rnnt_viterbi", s, 0.0, (double)rows * (4 * 2 + 2));
    CFM_LAUNCH((cfm_rnnt_viterbi_kernel<RNNT_NT, RNNT_MAXU1 / RNNT_NT, AD>), dim3(n_utt(ad.r)), dim3(RNNT_NT), 0, s, ad);
    return cfm_launch_status(what);
}

}  // namespace

extern "C" int64_t cfm_rnnt_align_scratch_bytes(int64_t nodes) { return nodes <= 0 ? 0 : (2 * nodes + 3) / 4 * 4; }

extern "C" int cfm_rnnt_align(const cfm_rnnt_align_desc* d, cfm_stream_t stream) {
    if (int rc = rnnt_check(d ? &d->r : nullptr, "cfm_rnnt_align", false)) return rc;
    return rnnt_align_launch(*d, "cfm_rnnt_align", (hipStream_t)stream);
}

extern "C" int cfm_rnnt_packed_align(const cfm_rnnt_packed_align_desc* d, cfm_stream_t stream) {
    if (int rc = rnnt_packed_check(d ? &d->r : nullptr, "cfm_rnnt_packed_align", false)) return rc;
    return rnnt_align_launch(*d, "cfm_rnnt_packed_align", (hipStream_t)stream);
}

extern "C" int cfm_rnnt_nll(const cfm_rnnt_desc* d, cfm_stream_t stream) {
    if (int rc = rnnt_check(d, "cfm_rnnt_nll")) return rc;
    CFM_CHECK_ARG(d->ll_alpha, "cfm_rnnt_nll: null pointer");
    return rnnt_nll_launch(*d, "cfm_rnnt_nll", (hipStream_t)stream);
}

extern "C" int cfm_rnnt_grad(const cfm_rnnt_desc* d, cfm_stream_t stream) {
    if (int rc = rnnt_check(d, "cfm_rnnt_grad")) return rc;
    return rnnt_grad_launch(*d, "cfm_rnnt_grad", (hipStream_t)stream);
}

extern "C" int cfm_rnnt_packed_nll(const cfm_rnnt_packed_desc* d, cfm_stream_t stream) {
    if (int rc = rnnt_packed_check(d, "cfm_rnnt_packed_nll")) return rc;
    CFM_CHECK_ARG(d->ll_alpha, "cfm_rnnt_packed_nll: null pointer");
    return rnnt_nll_launch(*d, "cfm_rnnt_packed_nll", (hipStream_t)stream);
}

extern "C" int cfm_rnnt_packed_grad(const cfm_rnnt_packed_desc* d, cfm_stream_t stream) {
    if (int rc = rnnt_packed_check(d, "cfm_rnnt_packed_grad")) return rc;
    return rnnt_grad_launch(*d, "cfm_rnnt_packed_grad", (hipStream_t)stream);
}
