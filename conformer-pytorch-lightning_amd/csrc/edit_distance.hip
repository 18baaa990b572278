// edit_distance.hip -- cfm_edit_distance: batched Levenshtein distance with one fixed optimal alignment per pair (include/cfm.h states the definition
// and the tie rule, tests/edit_distance_ref.py is its pure-Python statement).  Integer arithmetic throughout: the result is exact.
//
// One wavefront per pair, ED_WAVES pairs per workgroup.  Columns 1..H of the table are dealt out in strips of NC = 1, 2, 4, 8 or 16 consecutive columns
// per lane (the smallest that covers H with 64 lanes); column 0 (D[i][0] = i) is no lane's.  The previous row stays in registers.  Per reference token:
//     t[j]   = min(prev[j] + 1, prev[j-1] + (r != h[j-1]))                        prev[j-1] of a strip's first column: one wave shift
//     cur[j] = min over k <= j of t[k] + (j - k)                                  a min-plus prefix scan:
//         inside the strip serially (loc), then over the strips' last values shifted by one lane -- column 0's value i enters at lane 0 -- as a
//         min-scan of (value - first column) in DPP steps: row_shr 1, 2, 4, 8, row_bcast15, row_bcast31.
// With counts or ops wanted every cell's move goes to scratch, 2 bits each (0 hit, 1 substitution, 2 deletion, 3 insertion -- the op code minus one),
// a strip per lane and row in ONE uint8 / uint16 / uint32 (NC <= 4 / 8 / 16), so that no two lanes share a byte.  The backtrace is wave-uniform: the
// wavefront loads a window of WR rows x WE strips around the current cell, one element per lane, and follows the moves by v_readlane until the path
// leaves the window; lane 0 stages the ops in LDS in walk order, and the wavefront writes them out reversed, zero-filled to the row's end.
#include "cfm_common.h"

#define ED_WAVES 4
#define ED_MAXLEN 1024
#define ED_INF 0x3fffffff

template <int NC> struct ed_word { typedef uint8_t type; };
template <> struct ed_word<8> { typedef uint16_t type; };
template <> struct ed_word<16> { typedef uint32_t type; };

// the strip width for a hypothesis of H tokens, and the bytes of one lane's moves in one row at that width (host and device)
__host__ __device__ static inline int ed_strip(int H) {
    const int n = (H + 63) >> 6;
    return n <= 1 ? 1 : n <= 2 ? 2 : n <= 4 ? 4 : n <= 8 ? 8 : 16;
}
__host__ __device__ static inline int ed_lane_bytes(int H) {
    const int nc = ed_strip(H);
    return nc <= 4 ? 1 : nc == 8 ? 2 : 4;
}

// lanes without a source (outside the DPP pattern or masked by ROW_MASK) keep `old`
template <int CTRL, int ROW_MASK = 0xF>
__device__ __forceinline__ int ed_dpp(int old, int v) {
    return __builtin_amdgcn_update_dpp(old, v, CTRL, ROW_MASK, 0xF, false);
}

// inclusive minimum over lanes 0..lane
__device__ __forceinline__ int ed_prefix_min(int v) {
    v = min(v, ed_dpp<0x111>(ED_INF, v));                    // row_shr:1
    v = min(v, ed_dpp<0x112>(ED_INF, v));                    // row_shr:2
    v = min(v, ed_dpp<0x114>(ED_INF, v));                    // row_shr:4
    v = min(v, ed_dpp<0x118>(ED_INF, v));                    // row_shr:8
    v = min(v, ed_dpp<0x142, 0xA>(ED_INF, v));               // row_bcast15 into rows 1 and 3
    v = min(v, ed_dpp<0x143, 0xC>(ED_INF, v));               // row_bcast31 into rows 2 and 3
    return v;
}

// The table's rows 1..U for one pair (H, U >= 1, wave-uniform); returns D[U][H] in every lane.  mv: this pair's moves, [U][64] elements.
template <int NC, bool MOVES>
__device__ __forceinline__ int ed_rows(const int32_t* __restrict__ h, int H, const int32_t* __restrict__ r, int U, typename ed_word<NC>::type* __restrict__ mv,
                                       int lane) {
    typedef typename ed_word<NC>::type word;
    const int c0 = lane * NC;                                  // the strip is columns c0 + 1 .. c0 + NC, compared with h[c0 .. c0 + NC - 1]
    int prev[NC], tok[NC];
#pragma unroll
    for (int k = 0; k < NC; ++k) {
        tok[k] = c0 + k < H ? h[c0 + k] : 0;                   // columns beyond H are computed and never used: nothing flows from right to left
        prev[k] = c0 + k + 1;
    }
    int rnext = lane < U ? r[lane] : 0, rcur = 0;              // 64 reference tokens a lane each, the next 64 in flight
    for (int i = 1; i <= U; ++i) {
        const int q = (i - 1) & 63;
        if (q == 0) {
            rcur = rnext;
            rnext = i + 63 + lane < U ? r[i + 63 + lane] : 0;
        }
        const int rt = __builtin_amdgcn_readlane(rcur, q);
        const int left = ed_dpp<0x138>(i - 1, prev[NC - 1]);   // wave_shr:1 -- D[i-1][c0]; lane 0: column 0
        int loc[NC], dg[NC], cur[NC];
#pragma unroll
        for (int k = 0; k < NC; ++k) {
            dg[k] = (k ? prev[k - 1] : left) + (rt != tok[k] ? 1 : 0);
            const int t = min(prev[k] + 1, dg[k]);
            loc[k] = k ? min(t, loc[k - 1] + 1) : t;
        }
        const int before = ed_dpp<0x138>(i, loc[NC - 1]);      // what reaches column c0 from the strip to the left alone; lane 0: D[i][0] = i
        const int carry = ed_prefix_min(before - c0) + c0;     // D[i][c0]
        unsigned w = 0;
#pragma unroll
        for (int k = 0; k < NC; ++k) {
            cur[k] = min(loc[k], carry + k + 1);
            if (MOVES) {                                       // the tie rule: diagonal first, then deletion, then insertion
                const unsigned m = cur[k] == dg[k] ? (rt != tok[k] ? 1u : 0u) : cur[k] == prev[k] + 1 ? 2u : 3u;
                w |= m << (2 * k);
            }
        }
        if (MOVES) mv[(int64_t)(i - 1) * 64 + lane] = (word)w;
#pragma unroll
        for (int k = 0; k < NC; ++k) prev[k] = cur[k];
    }
    int v = prev[0];
#pragma unroll
    for (int k = 1; k < NC; ++k) v = ((H - 1) % NC) == k ? prev[k] : v;
    return __builtin_amdgcn_readlane(v, (H - 1) / NC);
}

// The backtrace from (U, H): ops in walk order (last op first) into `stage` when it is not null, their number in n[0], (S, D, I, hits) in n[1..4].
// Everything but the window load is wave-uniform.
template <int NC>
__device__ __forceinline__ void ed_trace(const typename ed_word<NC>::type* __restrict__ mv, int H, int U, uint8_t* stage, int lane, int* n) {
    constexpr int WE = NC == 1 ? 8 : NC == 16 ? 2 : 4, WR = 64 / WE;       // the window: WR rows x WE strips, its last row and strip at (i0, e0)
    int i = U, j = H, t = 0, i0 = 0, e0 = 0, nS = 0, nD = 0, nI = 0, nH = 0;
    bool have = false;
    unsigned win = 0;
    while (i > 0 || j > 0) {
        int op;
        if (i == 0) {
            op = 4;
        } else if (j == 0) {
            op = 3;
        } else {
            const int c = j - 1, e = c / NC;
            if (!have || i <= i0 - WR || e <= e0 - WE) {
                i0 = i, e0 = e, have = true;
                const int ri = i0 - lane / WE, el = e0 - (WE - 1) + lane % WE;
                win = ri >= 1 && el >= 0 ? (unsigned)mv[(int64_t)(ri - 1) * 64 + el] : 0u;
            }
            const unsigned w = (unsigned)__builtin_amdgcn_readlane((int)win, (i0 - i) * WE + (e - (e0 - (WE - 1))));
            op = (int)((w >> (2 * (c % NC))) & 3u) + 1;
        }
        if (stage && lane == 0) stage[t] = (uint8_t)op;
        ++t;
        nH += op == 1, nS += op == 2, nD += op == 3, nI += op == 4;
        i -= op != 4;
        j -= op != 3;
    }
    n[0] = t, n[1] = nS, n[2] = nD, n[3] = nI, n[4] = nH;
}

template <bool MOVES>
__global__ __launch_bounds__(ED_WAVES * 64) void cfm_edit_distance_kernel(cfm_edit_distance_desc d, int64_t pair_bytes) {
    __shared__ uint8_t stage_all[ED_WAVES][2 * ED_MAXLEN];
    const int lane = threadIdx.x & 63;
    const int p = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * ED_WAVES + (threadIdx.x >> 6)));
    if (p >= d.P) return;                                      // no barrier below: the wavefronts of a workgroup share nothing
    const int H = __builtin_amdgcn_readfirstlane(min(max(d.hyp_lens[p], 0), d.Hmax));
    const int ri = __builtin_amdgcn_readfirstlane(min(max(d.ref_index ? d.ref_index[p] : p, 0), d.R - 1));
    const int U = __builtin_amdgcn_readfirstlane(min(max(d.ref_lens[ri], 0), d.Umax));
    const int32_t* h = d.hyp + (int64_t)p * d.Hmax;
    const int32_t* r = d.ref + (int64_t)ri * d.Umax;
    uint8_t* scr = MOVES ? (uint8_t*)d.scratch + (int64_t)p * pair_bytes : nullptr;
    const int nc = ed_strip(H);
    int dist = H + U;                                          // an empty side: all insertions or all deletions, no table
    if (H > 0 && U > 0) {
        switch (nc) {
            case 1: dist = ed_rows<1, MOVES>(h, H, r, U, (ed_word<1>::type*)scr, lane); break;
            case 2: dist = ed_rows<2, MOVES>(h, H, r, U, (ed_word<2>::type*)scr, lane); break;
            case 4: dist = ed_rows<4, MOVES>(h, H, r, U, (ed_word<4>::type*)scr, lane); break;
            case 8: dist = ed_rows<8, MOVES>(h, H, r, U, (ed_word<8>::type*)scr, lane); break;
            default: dist = ed_rows<16, MOVES>(h, H, r, U, (ed_word<16>::type*)scr, lane); break;
        }
    }
    if (lane == 0) d.dist[p] = dist;
    if (!MOVES) return;
    __threadfence_block();                                     // the window loads below read what other lanes of this wavefront stored: its stores
                                                               // complete first (workgroup scope is a wait, not an L2 write-back)
    uint8_t* stage = d.ops ? stage_all[threadIdx.x >> 6] : nullptr;
    int n[5];
    switch (H > 0 && U > 0 ? nc : 1) {                         // with an empty side the walk never looks at a move
        case 1: ed_trace<1>((const ed_word<1>::type*)scr, H, U, stage, lane, n); break;
        case 2: ed_trace<2>((const ed_word<2>::type*)scr, H, U, stage, lane, n); break;
        case 4: ed_trace<4>((const ed_word<4>::type*)scr, H, U, stage, lane, n); break;
        case 8: ed_trace<8>((const ed_word<8>::type*)scr, H, U, stage, lane, n); break;
        default: ed_trace<16>((const ed_word<16>::type*)scr, H, U, stage, lane, n); break;
    }
    if (lane < 4) d.counts[(int64_t)p * 4 + lane] = lane == 0 ? n[1] : lane == 1 ? n[2] : lane == 2 ? n[3] : n[4];
    if (!d.ops_len) return;
    if (lane == 0) d.ops_len[p] = n[0];
    __builtin_amdgcn_wave_barrier();                           // lane 0's staged ops are read by every lane (LDS keeps a wavefront's order)
    const int cap = d.Hmax + d.Umax, L = n[0];
    uint8_t* ops = d.ops + (int64_t)p * cap;
    for (int k = lane; k < cap; k += 64) ops[k] = k < L ? stage[L - 1 - k] : (uint8_t)0;
}

extern "C" int64_t cfm_edit_distance_scratch_bytes(int32_t P, int32_t Hmax, int32_t Umax) {
    if (P < 1 || Hmax < 1 || Umax < 1) return 0;
    return (int64_t)P * Umax * 64 * ed_lane_bytes(Hmax);
}

extern "C" int cfm_edit_distance(const cfm_edit_distance_desc* d, cfm_stream_t stream) {
    CFM_CHECK_ARG(d, "cfm_edit_distance: null descriptor");
    CFM_CHECK_ARG(d->P >= 1 && d->R >= 1 && d->Hmax >= 0 && d->Umax >= 0, "cfm_edit_distance: bad shape P=%d R=%d Hmax=%d Umax=%d", d->P, d->R, d->Hmax, d->Umax);
    CFM_CHECK_ARG(d->Hmax <= ED_MAXLEN && d->Umax <= ED_MAXLEN, "cfm_edit_distance: Hmax=%d Umax=%d exceeds %d tokens", d->Hmax, d->Umax, ED_MAXLEN);
    CFM_CHECK_ARG(d->ref_index || d->P == d->R, "cfm_edit_distance: without ref_index P=%d must equal R=%d", d->P, d->R);
    CFM_CHECK_ARG((d->hyp || d->Hmax == 0) && d->hyp_lens && (d->ref || d->Umax == 0) && d->ref_lens && d->dist, "cfm_edit_distance: null pointer");
    CFM_CHECK_ARG(!d->ops == !d->ops_len || (!d->ops && d->Hmax + d->Umax == 0), "cfm_edit_distance: ops and ops_len go together");
    CFM_CHECK_ARG(d->counts || !d->ops_len, "cfm_edit_distance: ops need counts");
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((unsigned)((d->P + ED_WAVES - 1) / ED_WAVES)), block(ED_WAVES * 64);
    const double cells = (double)d->P * d->Hmax * d->Umax;
    if (!d->counts) {
        CfmProfScope prof("edit_distance", s, 0.0, (double)d->P * (d->Hmax + d->Umax) * 4);
        CFM_LAUNCH(cfm_edit_distance_kernel<false>, grid, block, 0, s, *d, (int64_t)0);
        return cfm_launch_status("cfm_edit_distance");
    }
    const int64_t need = cfm_edit_distance_scratch_bytes(d->P, d->Hmax, d->Umax);
    CFM_CHECK_ARG(d->scratch_bytes >= need && (d->scratch || need == 0), "cfm_edit_distance: scratch of %lld bytes, cfm_edit_distance_scratch_bytes = %lld needed",
                  (long long)d->scratch_bytes, (long long)need);
    CFM_CHECK_ARG(((uintptr_t)d->scratch & 3) == 0, "cfm_edit_distance: scratch must be 4-byte aligned");
    CfmProfScope prof("edit_distance_align", s, 0.0, (double)d->P * (d->Hmax + d->Umax) * 5 + cells / 2);
    CFM_LAUNCH(cfm_edit_distance_kernel<true>, grid, block, 0, s, *d, need / d->P);
    return cfm_launch_status("cfm_edit_distance (align)");
}
