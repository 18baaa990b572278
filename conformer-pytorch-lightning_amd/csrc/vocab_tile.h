// vocab_tile.h -- the product loop that the vocabulary kernels share: cfm_token_logprob (rescore.hip), cfm_lsm_loss and cfm_lsm_grad (lsm.hip).
//
// A workgroup of TL_WAVES wavefronts owns TL_ROWS rows of X, staged once in LDS in W's type (tl_stage_rows).  Its wavefronts deal the
// vocabulary out in tiles of 32 classes (tl_tiles).  The product is computed TRANSPOSED, C = W_tile . X^T with 16x16x32 MFMA: C's row (the
// class) runs along a lane's 4 accumulator registers and its column (the row of X) is lane & 15, so a lane holds 8 logits of ONE row per
// 16-row slice and folds them into that row's running values in registers.  What is folded is the caller's: tl_tiles hands every slice's 8
// logits (bias added, -inf at and past V) to a functor.
#pragma once
#include "cfm_common.h"

#define TL_ROWS 64
#define TL_WAVES 8
#define TL_MAXD 512

// One (max, sum) pair takes another in: the sum stays relative to the larger maximum.  Symmetric in its arguments (a float add commutes), so
// two lanes that exchange their pairs end with the same bits.  An empty pair is (-inf, 0).
__device__ __forceinline__ void tl_merge(float& mx, float& sm, float m2, float s2) {
    const float mn = fmaxf(mx, m2);
    if (mn > -INFINITY) sm = sm * __expf(mx - mn) + s2 * __expf(m2 - mn);
    mx = mn;
}

// LDS image of the row tile: row r at r * (Dp * 2) bytes, its 16-byte chunk c (8 values) at chunk slot c ^ (r & swz)
__device__ __forceinline__ int tl_off(int r, int c, int row_bytes, int swz) { return r * row_bytes + ((c ^ (r & swz)) << 4); }

// bytes of LDS a kernel built on this loop needs: the row image, or the `nvals` per-row partials of every wavefront that later take its place
static inline size_t tl_lds_bytes(int D, int nvals) {
    const size_t image = (size_t)TL_ROWS * ((D + 31) / 32) * 64, parts = (size_t)TL_WAVES * nvals * TL_ROWS * sizeof(float);
    return image > parts ? image : parts;
}

// rows row0 .. row0 + TL_ROWS of X (f32 or W's type, rows ldx apart) into the image, zero past M and past D; ends with the barrier
template <typename HT, typename XT>
__device__ __forceinline__ void tl_stage_rows(unsigned char* smem, const void* X, int64_t ldx, int row0, int M, int D, int tid) {
    const int ksteps = (D + 31) >> 5, nchunk = ksteps * 4, row_bytes = nchunk * 16, swz = (nchunk & 7) ? 3 : 7;
    for (int idx = tid; idx < TL_ROWS * nchunk; idx += TL_WAVES * 64) {
        const int r = idx / nchunk, c = idx - r * nchunk, k = c * 8;
        u32x4 v = {0u, 0u, 0u, 0u};
        if (row0 + r < M && k < D) {                           // D % 8 == 0: a chunk lies wholly inside a row or wholly in the zero padding
            if constexpr (cfm_is_f32<XT>) {
                const float* src = (const float*)X + (int64_t)(row0 + r) * ldx + k;
                v = pack8<HT>(*(const f32x4*)src, *(const f32x4*)(src + 4));
            } else {
                v = *(const u32x4*)((const u16*)X + (int64_t)(row0 + r) * ldx + k);
            }
        }
        *(u32x4*)(smem + tl_off(r, c, row_bytes, swz)) = v;
    }
    __syncthreads();
}

// Tiles ct0, ct0 + ctstep, .. below ntile of this wavefront.  fold(c0, s, v): tile base class c0, slice s (the lane's row is s * 16 + (lane & 15)
// of the workgroup's), v[t * 4 + e] = the logit of class c0 + 16 t + 4 (lane >> 4) + e, -inf at and past V.  Rows of W at and past V are
// never read: such classes read row V - 1 and are masked by the bias.
template <typename HT, typename F>
__device__ __forceinline__ void tl_tiles(const unsigned char* smem, const u16* W, const float* bias, int D, int V, int ct0, int ctstep, int ntile, int lane,
                                         F&& fold) {
    const int ksteps = (D + 31) >> 5, nchunk = ksteps * 4, row_bytes = nchunk * 16, swz = (nchunk & 7) ? 3 : 7;
    const int g = lane >> 4, l15 = lane & 15;
    for (int ct = ct0; ct < ntile; ct += ctstep) {
        const int c0 = ct * 32;
        // A operand: lane holds W[class c0 + 16 t + l15][k = 32 ks + 8 g ..+8]; classes at and past V read row V - 1 and are masked below
        const u16* w0 = W + (int64_t)min(c0 + l15, V - 1) * D + g * 8;
        const u16* w1 = W + (int64_t)min(c0 + 16 + l15, V - 1) * D + g * 8;
        f32x4 acc[2][4];
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int s = 0; s < 4; ++s) acc[t][s] = (f32x4){0.f, 0.f, 0.f, 0.f};
        for (int ks = 0; ks < ksteps; ++ks) {
            u32x4 a0 = {0u, 0u, 0u, 0u}, a1 = {0u, 0u, 0u, 0u};
            if (ks * 32 + g * 8 < D) {
                a0 = *(const u32x4*)(w0 + ks * 32);
                a1 = *(const u32x4*)(w1 + ks * 32);
            }
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                const u32x4 b = *(const u32x4*)(smem + tl_off(s * 16 + l15, ks * 4 + g, row_bytes, swz));
                acc[0][s] = HT::mfma(a0, b, acc[0][s]);
                acc[1][s] = HT::mfma(a1, b, acc[1][s]);
            }
        }
        // this lane's 8 classes of the tile: c0 + 16 t + 4 g + e
        float bv[8];                                           // -inf at and past V: the sum with the (finite) product masks the class
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int c = c0 + t * 16 + g * 4 + e;
                bv[t * 4 + e] = c < V ? bias[c] : -INFINITY;
            }
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            float v[8];
#pragma unroll
            for (int t = 0; t < 2; ++t)
#pragma unroll
                for (int e = 0; e < 4; ++e) v[t * 4 + e] = acc[t][s][e] + bv[t * 4 + e];
            fold(c0, s, v);
        }
    }
}

// v's 8 logits into a row's running (max, sum)
__device__ __forceinline__ void tl_fold_lse(float& mx, float& sm, const float (&v)[8]) {
    float tm = v[0];
#pragma unroll
    for (int q = 1; q < 8; ++q) tm = fmaxf(tm, v[q]);
    const float mn = fmaxf(mx, tm);
    if (mn > -INFINITY) {
        float add = 0.f;
#pragma unroll
        for (int q = 0; q < 8; ++q) add += __expf(v[q] - mn);
        sm = sm * __expf(mx - mn) + add;
        mx = mn;
    }
}

// the target's logit, when this lane holds it in this tile: exactly one lane of a row's four, in exactly one tile, does
__device__ __forceinline__ void tl_pick_target(float& tv, int target, int c0, int g, const float (&v)[8]) {
    const int dt = target - c0;
    if (dt >= 0 && dt < 32 && ((dt >> 2) & 3) == g) {
        const int q = (dt >> 4) * 4 + (dt & 3);
        float pick = v[0];
#pragma unroll
        for (int qq = 1; qq < 8; ++qq) pick = q == qq ? v[qq] : pick;
        tv = pick;
    }
}
