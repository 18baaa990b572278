// joint.hip -- the transducer joint's broadcast-add + tanh (gfx950).
//
// replaces, in TransducerJoint.forward (reference src/joint.py:31-37):
//     out = enc_out.unsqueeze(2) + pred_out.unsqueeze(1);  out = tanh(out)          [B, T, U, J]
// which is the activation operand of the vocabulary projection ffn_out (cfm_gemm, M = B*T*U rows).  Written ONCE as a 16-bit
// (f32 in the accurate mode) row-major [B*T*U, J] operand: 167 MB at BASELINE config 4 (B 16, T' 249, U 41, J 512) next to the
// 3.3 GB of f32 logits the GEMM writes.  Fusing the tanh into the GEMM's A-tile loader instead would evaluate it once per N tile --
// 40 times at V = 5002, ~14 k VALU/transcendental cycles per wavefront against 4 k cycles of MFMA per 128 x 128 x 512 tile -- and the
// XCD-aware tile order of cfm_gemm already makes the 40 N tiles of one M tile read these rows from one L2.
//
// HBM-bound: per output row J*2 bytes written; the projected encoder / predictor rows (B*T*J and B*U*J f32, a few MB) stay in L2.
//
// The packed forms (cfm_joint_act_packed / _bwd) write and read only the valid cells of a ragged batch or accumulation window (include/cfm.h
// cfm_lattice): same per-cell arithmetic, same fixed-order sums, a binary search over the lattice offsets in place of the padded divisions.
#include "cfm_common.h"

namespace {

// tanh(x) = 1 - 2 / (1 + e^{2x}) on v_exp_f32 / v_rcp_f32: absolute error ~1e-7, exact limits at +-inf
__device__ __forceinline__ float tanh_fast(float x) { return 1.0f - 2.0f * __builtin_amdgcn_rcpf(1.0f + __expf(2.0f * x)); }

template <typename OT>
__global__ __launch_bounds__(256) void cfm_joint_act_kernel(const float* __restrict__ enc, int64_t ld_e, const float* __restrict__ pred,
                                                            int64_t ld_p, void* __restrict__ out, int T, int U, int J, int64_t chunks) {
    const int cpr = J >> 3;                                // 8-column chunks per row
    for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < chunks; idx += (int64_t)gridDim.x * 256) {
        const int64_t m = idx / cpr;                       // output row (b, t, u)
        const int c = (int)(idx - m * cpr) * 8;
        const int64_t bt = m / U;                          // encoder row b*T + t
        const int u = (int)(m - bt * U);
        const int64_t b = bt / T;
        const float* e = enc + bt * ld_e + c;
        const float* p = pred + (b * U + u) * ld_p + c;
        const f32x4 e0 = *(const f32x4*)e, e1 = *(const f32x4*)(e + 4);
        const f32x4 p0 = *(const f32x4*)p, p1 = *(const f32x4*)(p + 4);
        f32x4 v0, v1;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            v0[r] = tanh_fast(e0[r] + p0[r]);
            v1[r] = tanh_fast(e1[r] + p1[r]);
        }
        if constexpr (std::is_same<OT, float>::value) {
            float* o = (float*)out + m * J + c;
            *(f32x4*)o = v0;
            *(f32x4*)(o + 4) = v1;
        } else {
            *(u32x4*)((u16*)out + m * J + c) = pack8<OT>(v0, v1);
        }
    }
}

// backward of a = tanh(e[b,t] + p[b,u]) (train path of TransducerJoint.rnnt_loss): dz = dA (1 - a^2) with a recomputed from the f32 projections
// (the same tanh_fast as the forward, not the 16-bit operand), reduced to de[b,t] = sum_u dz and dp[b,u] = sum_t dz in a fixed order, no atomics:
// workgroup (column block, block of JAB_TB frames, b); each thread owns 4 columns, walks u = 0..U-1 and, per u, its JAB_TB frames: de rows are
// complete in registers at the end, dp leaves one partial per (frame block, u) that cfm_joint_act_bwd_sum_kernel adds in frame-block order.
// HBM-bound: dA (f32 [B T U, J]) is read once.
constexpr int JAB_TB = 8;

__global__ __launch_bounds__(64) void cfm_joint_act_bwd_kernel(const float* __restrict__ enc, int64_t ld_e, const float* __restrict__ pred, int64_t ld_p,
                                                               const float* __restrict__ dA, float* __restrict__ de, float* __restrict__ part, int T, int U, int J) {
    const int c = (blockIdx.x * 64 + threadIdx.x) * 4;
    if (c >= J) return;
    const int tb = blockIdx.y, nTB = gridDim.y, b = blockIdx.z, t0 = tb * JAB_TB;
    f32x4 e[JAB_TB], acc[JAB_TB];
#pragma unroll
    for (int k = 0; k < JAB_TB; ++k) {
        e[k] = t0 + k < T ? *(const f32x4*)(enc + ((int64_t)b * T + t0 + k) * ld_e + c) : (f32x4){0.f, 0.f, 0.f, 0.f};
        acc[k] = (f32x4){0.f, 0.f, 0.f, 0.f};
    }
    for (int u = 0; u < U; ++u) {
        const f32x4 p = *(const f32x4*)(pred + ((int64_t)b * U + u) * ld_p + c);
        f32x4 ap = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int k = 0; k < JAB_TB; ++k) {
            if (t0 + k < T) {
                const f32x4 g = *(const f32x4*)(dA + (((int64_t)b * T + t0 + k) * U + u) * J + c);
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float a = tanh_fast(e[k][r] + p[r]);
                    const float dz = g[r] * (1.0f - a * a);
                    acc[k][r] += dz;
                    ap[r] += dz;
                }
            }
        }
        *(f32x4*)(part + (((int64_t)b * nTB + tb) * U + u) * J + c) = ap;
    }
#pragma unroll
    for (int k = 0; k < JAB_TB; ++k)
        if (t0 + k < T) *(f32x4*)(de + ((int64_t)b * T + t0 + k) * J + c) = acc[k];
}

// dp[b,u,:] = sum over frame blocks tb = 0, 1, .. of part[b,tb,u,:]
__global__ __launch_bounds__(256) void cfm_joint_act_bwd_sum_kernel(const float* __restrict__ part, float* __restrict__ dp, int B, int nTB, int U, int J) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;          // one 4-column chunk of dp
    const int cpr = J / 4;
    if (idx >= (int64_t)B * U * cpr) return;
    const int64_t row = idx / cpr;                                       // b*U + u
    const int c = (int)(idx - row * cpr) * 4, b = (int)(row / U), u = (int)(row - (int64_t)b * U);
    f32x4 s = {0.f, 0.f, 0.f, 0.f};
    for (int tb = 0; tb < nTB; ++tb) s += *(const f32x4*)(part + (((int64_t)b * nTB + tb) * U + u) * J + c);
    *(f32x4*)(dp + row * J + c) = s;
}


// ---- packed lattices (include/cfm.h cfm_lattice): only the valid cells (b, t < T_b, u <= U_b) have rows ----

// forward: one wavefront per run of JPK_RUN consecutive packed rows; the run's first row is found by a binary search over off, the rest by
// stepping (b, t, u), so the encoder chunk (shared by U_b+1 consecutive rows) is loaded once per frame of the run.  8 columns per lane.
constexpr int JPK_RUN = 16;

template <typename OT>
__global__ __launch_bounds__(256) void cfm_joint_act_packed_kernel(const float* __restrict__ enc, int64_t ld_e, const float* __restrict__ pred,
                                                                   int64_t ld_p, void* __restrict__ out, cfm_lattice L, int J) {
    const int lane = threadIdx.x & 63;
    const int64_t r0 = ((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * JPK_RUN;
    if (r0 >= L.M) return;
    const int64_t r1 = r0 + JPK_RUN < L.M ? r0 + JPK_RUN : L.M;
    const int b0 = last_le(L.off, L.B, r0);
    const int rem = (int)(r0 - L.off[b0]), U10 = L.U[b0] + 1, t0 = rem / U10, u0 = rem - t0 * U10;
    for (int c = lane * 8; c < J; c += 512) {
        int b = b0, t = t0, u = u0, U1 = U10, Tb = L.T[b0];
        const float* e = enc + (L.enc_row0[b] + t) * ld_e + c;
        f32x4 e0 = *(const f32x4*)e, e1 = *(const f32x4*)(e + 4);
        for (int64_t r = r0; r < r1; ++r) {
            const float* p = pred + (L.pred_row0[b] + u) * ld_p + c;
            const f32x4 p0 = *(const f32x4*)p, p1 = *(const f32x4*)(p + 4);
            f32x4 v0, v1;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                v0[k] = tanh_fast(e0[k] + p0[k]);
                v1[k] = tanh_fast(e1[k] + p1[k]);
            }
            if constexpr (std::is_same<OT, float>::value) {
                float* o = (float*)out + r * J + c;
                *(f32x4*)o = v0;
                *(f32x4*)(o + 4) = v1;
            } else {
                *(u32x4*)((u16*)out + r * J + c) = pack8<OT>(v0, v1);
            }
            if (r + 1 < r1 && ++u == U1) {                 // next row: next frame, or the next utterance that has one
                u = 0;
                if (++t == Tb) {
                    t = 0;
                    do ++b; while (L.T[b] == 0);           // r + 1 < M: some later utterance has a row
                    Tb = L.T[b];
                    U1 = L.U[b] + 1;
                }
                e = enc + (L.enc_row0[b] + t) * ld_e + c;
                e0 = *(const f32x4*)e;
                e1 = *(const f32x4*)(e + 4);
            }
        }
    }
}

// backward, pass 1: workgroup (column block, block of JAB_TB frames, b) as cfm_joint_act_bwd_kernel over utterance b's own T_b x (U_b+1) block:
// d_enc rows complete in registers, one d_pred partial per (frame block, u) at row blk_off[b] + tb (U_b+1) + u of the work array.
__global__ __launch_bounds__(64) void cfm_joint_act_packed_bwd_kernel(const float* __restrict__ enc, int64_t ld_e, const float* __restrict__ pred,
                                                                      int64_t ld_p, const float* __restrict__ dA, float* __restrict__ de,
                                                                      float* __restrict__ part, cfm_lattice L, int J) {
    const int c = (blockIdx.x * 64 + threadIdx.x) * 4;
    const int tb = blockIdx.y, b = blockIdx.z, t0 = tb * JAB_TB;
    const int T = L.T[b];
    if (c >= J || t0 >= T) return;
    const int U = L.U[b] + 1;
    const int64_t er = L.enc_row0[b] + t0, pr = L.pred_row0[b], node0 = L.off[b] + (int64_t)t0 * U, prt = L.blk_off[b] + (int64_t)tb * U;
    f32x4 e[JAB_TB], acc[JAB_TB];
#pragma unroll
    for (int k = 0; k < JAB_TB; ++k) {
        e[k] = t0 + k < T ? *(const f32x4*)(enc + (er + k) * ld_e + c) : (f32x4){0.f, 0.f, 0.f, 0.f};
        acc[k] = (f32x4){0.f, 0.f, 0.f, 0.f};
    }
    for (int u = 0; u < U; ++u) {
        const f32x4 p = *(const f32x4*)(pred + (pr + u) * ld_p + c);
        f32x4 ap = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int k = 0; k < JAB_TB; ++k) {
            if (t0 + k < T) {
                const f32x4 g = *(const f32x4*)(dA + (node0 + (int64_t)k * U + u) * J + c);
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float a = tanh_fast(e[k][r] + p[r]);
                    const float dz = g[r] * (1.0f - a * a);
                    acc[k][r] += dz;
                    ap[r] += dz;
                }
            }
        }
        *(f32x4*)(part + (prt + u) * J + c) = ap;
    }
#pragma unroll
    for (int k = 0; k < JAB_TB; ++k)
        if (t0 + k < T) *(f32x4*)(de + (er + k) * J + c) = acc[k];
}

// backward, pass 2: one 4-column chunk per thread over the n_pred predictor rows then the n_enc encoder rows.  Predictor row (b, u <= U_b) of an
// utterance with frames: the partials of its frame blocks added in block order; every other predictor row and every encoder row outside
// t < T_b (pass 1 wrote those): exact zeros.
__global__ __launch_bounds__(256) void cfm_joint_act_packed_bwd_sum_kernel(const float* __restrict__ part, float* __restrict__ dp, float* __restrict__ de,
                                                                          cfm_lattice L, int J) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int cpr = J / 4;
    const int64_t row = idx / cpr;
    if (row >= L.n_pred + L.n_enc) return;
    const int c = (int)(idx - row * cpr) * 4;
    f32x4 s = {0.f, 0.f, 0.f, 0.f};
    if (row < L.n_pred) {
        const int b = last_le(L.pred_row0, L.B, row);
        if (b >= 0) {
            const int u = (int)(row - L.pred_row0[b]), U = L.U[b] + 1, nTB = (L.T[b] + JAB_TB - 1) / JAB_TB;
            if (u < U) {
                const float* q = part + (L.blk_off[b] + u) * J + c;
                for (int tb = 0; tb < nTB; ++tb) s += *(const f32x4*)(q + (int64_t)tb * U * J);
            }
        }
        *(f32x4*)(dp + row * J + c) = s;
    } else {
        const int64_t r = row - L.n_pred;
        const int b = last_le(L.enc_row0, L.B, r);
        if (b >= 0 && r - L.enc_row0[b] < L.T[b]) return;
        *(f32x4*)(de + r * J + c) = s;
    }
}
}  // namespace

extern "C" int64_t cfm_joint_act_bwd_ws(int32_t B, int32_t T, int32_t U, int32_t J) {
    return (int64_t)B * ((T + JAB_TB - 1) / JAB_TB) * U * J;
}

extern "C" int cfm_joint_act_bwd(const float* enc, int64_t ld_e, const float* pred, int64_t ld_p, const float* dact, float* d_enc, float* d_pred,
                                 float* work, int32_t B, int32_t T, int32_t U, int32_t J, cfm_stream_t stream) {
    CFM_CHECK_ARG(enc && pred && dact && d_enc && d_pred && work, "cfm_joint_act_bwd: null pointer");
    CFM_CHECK_ARG(B > 0 && T > 0 && U > 0 && J > 0 && J % 8 == 0, "cfm_joint_act_bwd: bad shape B=%d T=%d U=%d J=%d (J %% 8 == 0)", B, T, U, J);
    CFM_CHECK_ARG(ld_e >= J && ld_p >= J && ld_e % 4 == 0 && ld_p % 4 == 0, "cfm_joint_act_bwd: row strides must be >= J and multiples of 4");
    hipStream_t s = (hipStream_t)stream;
    const int nTB = (T + JAB_TB - 1) / JAB_TB;
    {
        CfmProfScope prof("joint_act_bwd", s, 0.0, (double)B * T * U * J * 4 + (double)B * nTB * U * J * 4);
        CFM_LAUNCH(cfm_joint_act_bwd_kernel, dim3((unsigned)((J / 4 + 63) / 64), (unsigned)nTB, (unsigned)B), dim3(64), 0, s, enc, ld_e, pred, ld_p, dact,
                   d_enc, work, T, U, J);
        if (int rc = cfm_launch_status("cfm_joint_act_bwd")) return rc;
    }
    const int64_t chunks = (int64_t)B * U * (J / 4);
    CfmProfScope prof("joint_act_bwd_sum", s, 0.0, (double)B * nTB * U * J * 4);
    CFM_LAUNCH(cfm_joint_act_bwd_sum_kernel, dim3((unsigned)((chunks + 255) / 256)), dim3(256), 0, s, (const float*)work, d_pred, B, nTB, U, J);
    return cfm_launch_status("cfm_joint_act_bwd (sum)");
}

extern "C" int cfm_joint_act(const float* enc, int64_t ld_e, const float* pred, int64_t ld_p, void* out, int32_t out_dtype, int32_t B,
                             int32_t T, int32_t U, int32_t J, cfm_stream_t stream) {
    CFM_CHECK_ARG(enc && pred && out, "cfm_joint_act: null pointer");
    CFM_CHECK_ARG(B > 0 && T > 0 && U > 0 && J > 0 && J % 8 == 0, "cfm_joint_act: bad shape B=%d T=%d U=%d J=%d (J %% 8 == 0)", B, T, U, J);
    CFM_CHECK_ARG(ld_e >= J && ld_p >= J && ld_e % 4 == 0 && ld_p % 4 == 0, "cfm_joint_act: row strides must be >= J and multiples of 4");
    CFM_CHECK_ARG(out_dtype >= CFM_F32 && out_dtype <= CFM_F16, "cfm_joint_act: bad out_dtype");
    hipStream_t s = (hipStream_t)stream;
    const int64_t rows = (int64_t)B * T * U, chunks = rows * (J / 8);
    const int64_t want = (chunks + 255) / 256;
    const unsigned grid = (unsigned)(want < 256 * 16 ? want : 256 * 16);      // grid-stride beyond 16 workgroups per CU
    CfmProfScope prof("joint_act", s, 0.0, (double)rows * J * cfm_elt_size(out_dtype));
    cfm_by_dtype(out_dtype, [&](auto ot) {
        CFM_LAUNCH(cfm_joint_act_kernel<decltype(ot)>, dim3(grid), dim3(256), 0, s, enc, ld_e, pred, ld_p, out, T, U, J, chunks);
    });
    return cfm_launch_status("cfm_joint_act");
}

static int lattice_check(const cfm_lattice* L, const char* what) {
    CFM_CHECK_ARG(L && L->off && L->T && L->U && L->enc_row0 && L->pred_row0, "%s: null lattice array", what);
    CFM_CHECK_ARG(L->B > 0 && L->M >= 0 && L->n_enc > 0 && L->n_pred > 0, "%s: bad lattice B=%d M=%lld n_enc=%lld n_pred=%lld", what, L->B,
                  (long long)L->M, (long long)L->n_enc, (long long)L->n_pred);
    return CFM_OK;
}

extern "C" int cfm_joint_act_packed(const float* enc, int64_t ld_e, const float* pred, int64_t ld_p, void* out, int32_t out_dtype, const cfm_lattice* lat,
                                    int32_t J, cfm_stream_t stream) {
    CFM_CHECK_ARG(enc && pred && out, "cfm_joint_act_packed: null pointer");
    if (int rc = lattice_check(lat, "cfm_joint_act_packed")) return rc;
    CFM_CHECK_ARG(J > 0 && J % 8 == 0, "cfm_joint_act_packed: J = %d (J %% 8 == 0)", J);
    CFM_CHECK_ARG(ld_e >= J && ld_p >= J && ld_e % 4 == 0 && ld_p % 4 == 0, "cfm_joint_act_packed: row strides must be >= J and multiples of 4");
    CFM_CHECK_ARG(out_dtype >= CFM_F32 && out_dtype <= CFM_F16, "cfm_joint_act_packed: bad out_dtype");
    if (lat->M == 0) return CFM_OK;
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((unsigned)((lat->M + 4 * JPK_RUN - 1) / (4 * JPK_RUN)));
    CfmProfScope prof("joint_act_packed", s, 0.0, (double)lat->M * J * cfm_elt_size(out_dtype));
    cfm_by_dtype(out_dtype, [&](auto ot) {
        CFM_LAUNCH(cfm_joint_act_packed_kernel<decltype(ot)>, grid, dim3(256), 0, s, enc, ld_e, pred, ld_p, out, *lat, J);
    });
    return cfm_launch_status("cfm_joint_act_packed");
}

extern "C" int cfm_joint_act_packed_bwd(const float* enc, int64_t ld_e, const float* pred, int64_t ld_p, const float* dact, float* d_enc, float* d_pred,
                                        float* work, const cfm_lattice* lat, int32_t J, cfm_stream_t stream) {
    CFM_CHECK_ARG(enc && pred && d_enc && d_pred, "cfm_joint_act_packed_bwd: null pointer");
    if (int rc = lattice_check(lat, "cfm_joint_act_packed_bwd")) return rc;
    CFM_CHECK_ARG(lat->blk_off, "cfm_joint_act_packed_bwd: null blk_off");
    CFM_CHECK_ARG(lat->M == 0 || (dact && work), "cfm_joint_act_packed_bwd: null dact / work");
    CFM_CHECK_ARG(J > 0 && J % 8 == 0, "cfm_joint_act_packed_bwd: J = %d (J %% 8 == 0)", J);
    CFM_CHECK_ARG(ld_e >= J && ld_p >= J && ld_e % 4 == 0 && ld_p % 4 == 0, "cfm_joint_act_packed_bwd: row strides must be >= J and multiples of 4");
    hipStream_t s = (hipStream_t)stream;
    if (lat->M > 0) {
        const int nTB = (lat->T_max + JAB_TB - 1) / JAB_TB;
        CFM_CHECK_ARG(nTB > 0, "cfm_joint_act_packed_bwd: T_max = %d with %lld rows", lat->T_max, (long long)lat->M);
        CfmProfScope prof("joint_act_packed_bwd", s, 0.0, (double)lat->M * J * 4 * (1.0 + 1.0 / JAB_TB));
        CFM_LAUNCH(cfm_joint_act_packed_bwd_kernel, dim3((unsigned)((J / 4 + 63) / 64), (unsigned)nTB, (unsigned)lat->B), dim3(64), 0, s, enc, ld_e, pred,
                   ld_p, dact, d_enc, work, *lat, J);
        if (int rc = cfm_launch_status("cfm_joint_act_packed_bwd")) return rc;
    }
    const int64_t chunks = (lat->n_pred + lat->n_enc) * (J / 4);
    CfmProfScope prof("joint_act_packed_bwd_sum", s, 0.0, (double)lat->M * J * 4 / JAB_TB + (double)(lat->n_pred + lat->n_enc) * J * 4);
    CFM_LAUNCH(cfm_joint_act_packed_bwd_sum_kernel, dim3((unsigned)((chunks + 255) / 256)), dim3(256), 0, s, (const float*)work, d_pred, d_enc, *lat, J);
    return cfm_launch_status("cfm_joint_act_packed_bwd (sum)");
}
