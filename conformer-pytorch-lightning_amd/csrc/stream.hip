// stream.hip -- per-stream state for the batched streaming step (beyond the reference, whose forward_chunk
// serves one stream at a time, src/encoder.py:78-123, and rebuilds its attention cache with cat + slice every step, :117).
//
// B independent streams advance together, each at ITS OWN position: stream b has consumed offset[b] encoder frames of its utterance
// (int32 on the device, so a captured HIP graph replays without host-side scalars).  Per layer the keys / values of the last
// `need` frames and of the current chunk live in a ring buffer  kv_ring f32 [B, H, ring_T, 2*dk],  ring_T = need + chunk: frame f of a
// stream sits in slot f mod ring_T, a step writes only its `chunk` new frames, and nothing is ever moved.  Attention runs over all
// ring_T slots with a per-stream slot mask (the softmax is a sum over a SET of keys: their order in memory is irrelevant up to the
// rounding of the running sums) and per-(stream, slot) positional rows, so item b of the result equals the reference's batch-1
// forward_chunk on that stream with that stream's cache and offset (to the precision mode's tolerance).
//
//   cfm_stream_prep     offsets -> slot mask [B, ring_T], positional rows pe[frame in slot] [B, ring_T, D], optional absolute rows [B, D]
//   cfm_kv_ring_write   this step's K / V rows (from the fused QKV projection) -> their slots of the ring
//   cfm_stream_advance  offset[b] += chunk for active streams
//   frame_lens / lens   optional in those three and in cfm_conv_cache_update (NULL: whole windows) -- PER-STREAM lengths: stream b's window holds
//                       frame_lens[b] valid feature frames, hence c_b = ((n - 1) / 2 - 1) / 2 encoder frames (0 below 7: the two un-padded stride-2
//                       convolutions of the front-end); only those enter the mask, the ring, the conv cache and the offset, and c_b = 0 touches no
//                       state at all
//   cfm_dwconv_causal_bn_silu / cfm_conv_cache_update   the OPT-IN causal depthwise convolution with a (ktaps-1)-frame left context per
//                       stream (the reference has no causal mode and ignores its cnn_cache, convolution.py:34-39: off = parity)
#include "cfm_common.h"

namespace {

// the frame held by slot s when the newest frame of the window is `last`: the largest f <= last with f = s (mod ring_T)
__device__ __forceinline__ int slot_frame(int last, int s, int ring_T) {
    int r = (last - s) % ring_T;
    if (r < 0) r += ring_T;
    return last - r;
}

// encoder frames of a window of n feature frames (convolution.py: two 3-tap stride-2 convolutions without padding), at most T
__device__ __forceinline__ int stream_out_len(int n, int T) {
    const int c = n < 7 ? 0 : ((n - 1) / 2 - 1) / 2;
    return c < T ? c : T;
}

// The newest frame of stream b is off + c_b - 1, c_b = T or -- frame_lens set -- stream_out_len(frame_lens[b]), which out_lens[b] receives: the mask covers
// the min(off, need) cached frames and the c_b new ones.  c_b = 0: the newest frame is off - 1, so the mask is the cached frames alone, and at off = 0 no
// slot at all (slot_frame then returns a negative frame)
__global__ void cfm_stream_prep_kernel(const int* __restrict__ offsets, const int* __restrict__ frame_lens, int* __restrict__ out_lens, int B, int T, int need,
                                       int ring_T, const float* __restrict__ pe, int max_len, int D, uint8_t* __restrict__ slot_mask,
                                       float* __restrict__ pos_rows, float* __restrict__ abs_rows) {
    const int b = blockIdx.y, s = blockIdx.x;
    const int off = offsets[b];
    const int c = frame_lens ? stream_out_len(frame_lens[b], T) : T;
    const int cached = off < need ? off : need;
    if (frame_lens && s == 0 && threadIdx.x == 0) out_lens[b] = c;
    if (s < ring_T) {
        const int f = slot_frame(off + c - 1, s, ring_T);
        const bool valid = f >= off - cached && f >= 0;
        if (threadIdx.x == 0) slot_mask[(int64_t)b * ring_T + s] = valid ? 1 : 0;
        // f < max_len is the caller's job (encoder.StreamingBatch extends the table before a stream reaches its end); the clamp only keeps a
        // misuse of the C entry point inside the allocation
        const int row = valid ? (f < max_len ? f : max_len - 1) : 0;
        for (int i = threadIdx.x * 4; i < D; i += blockDim.x * 4)
            *(f32x4*)(pos_rows + ((int64_t)b * ring_T + s) * D + i) = *(const f32x4*)(pe + (int64_t)row * D + i);
    } else if (abs_rows) {                                  // one extra block per stream: the absolute-encoding row pe[offset] (attention.py:119-120)
        const int row = off < max_len ? off : max_len - 1;
        for (int i = threadIdx.x * 4; i < D; i += blockDim.x * 4) *(f32x4*)(abs_rows + (int64_t)b * D + i) = *(const f32x4*)(pe + (int64_t)row * D + i);
    }
}

// ring[b, h, (offset[b] + t) mod ring_T, 0:dk] = K_t, [dk:2dk] = V_t for the T new frames, or -- lens set -- for rows t < lens[b] only.  Later rows touch
// no slot: they are no frames of the stream and may hold anything, non-finite values included, while a masked slot has to stay finite (the attention
// multiplies its values with a probability of zero)
__global__ void cfm_kv_ring_write_kernel(const void* __restrict__ k, const void* __restrict__ v, int dt, int64_t k_sb, int64_t k_st, int64_t v_sb, int64_t v_st,
                                         float* __restrict__ ring, const int* __restrict__ offsets, const int* __restrict__ lens, int B, int H, int T, int dk,
                                         int ring_T) {
    const int64_t n = (int64_t)B * T * H * 2 * dk;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int e = (int)(i % (2 * dk));
        int64_t r = i / (2 * dk);
        const int h = (int)(r % H);
        r /= H;
        const int t = (int)(r % T);
        const int b = (int)(r / T);
        if (lens && t >= lens[b]) continue;
        const int slot = (offsets[b] + t) % ring_T;
        const float val = e < dk ? load_as_f32(k, (int64_t)b * k_sb + (int64_t)t * k_st + h * dk + e, dt)
                                 : load_as_f32(v, (int64_t)b * v_sb + (int64_t)t * v_st + h * dk + (e - dk), dt);
        ring[(((int64_t)b * H + h) * ring_T + slot) * (2 * dk) + e] = val;
    }
}

// offsets[b] += c_b, one workgroup per stream: c_b = T for an active stream and 0 for an inactive one (active NULL: all active), or -- lens set --
// lens[b] clamped to 0 .. T.  Rows t >= c_b of y [B, T, D] (optional, with lens) become zero -- a store, not a product: those rows may hold anything
__global__ void cfm_stream_advance_kernel(int* offsets, const uint8_t* __restrict__ active, const int* __restrict__ lens, float* __restrict__ y, int T, int D) {
    const int b = blockIdx.x;
    int c = T;
    if (lens) c = lens[b] < 0 ? 0 : (lens[b] < T ? lens[b] : T);
    else if (active && !active[b]) c = 0;
    if (y) {
        float* const rows = y + ((int64_t)b * T + c) * D;
        const int n = (T - c) * D;
        for (int i = threadIdx.x * 4; i < n; i += blockDim.x * 4) *(f32x4*)(rows + i) = (f32x4){0.f, 0.f, 0.f, 0.f};
    }
    if (threadIdx.x == 0 && c > 0) offsets[b] += c;
}

// y[b,t,d] = silu( (sum_k w[d,k] xx[b, t+k, d] + bias[d]) * scale[d] + shift[d] ),  xx = [cache (K-1 frames) | x (T frames)]
__global__ void cfm_dwconv_causal_kernel(const void* __restrict__ x, int x_dt, const float* __restrict__ cache, const float* __restrict__ w,
                                         const float* __restrict__ bias, const float* __restrict__ sc, const float* __restrict__ sh, void* __restrict__ y, int y_dt,
                                         int B, int T, int D, int K) {
    const int64_t n = (int64_t)B * T * D;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int d = (int)(i % D);
        const int t = (int)((i / D) % T);
        const int b = (int)(i / ((int64_t)D * T));
        float a = 0.f;
        for (int k = 0; k < K; ++k) {
            const int tt = t + k - (K - 1);                 // position in x; negative: the left context
            float xv;
            if (tt >= 0) xv = load_as_f32(x, ((int64_t)b * T + tt) * D + d, x_dt);
            else xv = cache ? cache[((int64_t)b * (K - 1) + (K - 1 + tt)) * D + d] : 0.f;
            a = fmaf(w[(int64_t)d * K + k], xv, a);
        }
        store_from_f32(y, i, y_dt, siluf_((a + bias[d]) * sc[d] + sh[d]));
    }
}

// cache <- the last K-1 frames of [cache | x[:T_b]], in place; T_b = T, or -- lens set -- min(lens[b], T).  New row j is row j + T_b of [cache | x[:T_b]]:
// old cache row j + T_b while j + T_b < K-1, else x row j + T_b - (K-1) < T_b.  A thread owns one (stream, channel) column and walks j upwards, and for
// T_b > 0 the cache row it reads, j + T_b, lies above every row written so far (<= j); T_b = 0 would read and write row j itself -- the column is left alone
__global__ void cfm_conv_cache_update_kernel(const void* __restrict__ x, int x_dt, float* __restrict__ cache, const int* __restrict__ lens, int B, int T, int D,
                                             int K) {
    const int C = K - 1;
    const int64_t n = (int64_t)B * D;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int d = (int)(i % D);
        const int b = (int)(i / D);
        const int Tb = lens && lens[b] < T ? lens[b] : T;
        if (Tb <= 0) continue;
        for (int j = 0; j < C; ++j) {
            const int tt = j + Tb - C;                      // position in x of new cache row j
            cache[((int64_t)b * C + j) * D + d] = tt >= 0 ? load_as_f32(x, ((int64_t)b * T + tt) * D + d, x_dt) : cache[((int64_t)b * C + (C + tt)) * D + d];
        }
    }
}

inline int blocks_for(int64_t n) {
    const int64_t b = (n + 255) / 256;
    return (int)(b < 1 ? 1 : (b > 4096 ? 4096 : b));
}

}  // namespace

extern "C" int cfm_stream_prep(const int32_t* offsets, const int32_t* frame_lens, int32_t* out_lens, int32_t B, int32_t T, int32_t need, int32_t ring_T,
                               const float* pe, int32_t max_len, int32_t D, uint8_t* slot_mask, float* pos_rows, float* abs_rows, cfm_stream_t stream) {
    CFM_CHECK_ARG(offsets && pe && slot_mask && pos_rows, "cfm_stream_prep: null pointer");
    CFM_CHECK_ARG(!frame_lens == !out_lens, "cfm_stream_prep: frame_lens and out_lens come together");
    CFM_CHECK_ARG(B > 0 && B <= 65535 && T > 0 && need >= 0 && ring_T >= need + T && D > 0 && D % 4 == 0 && max_len > 0,
                  "cfm_stream_prep: bad shape B=%d T=%d need=%d ring_T=%d D=%d (ring_T >= need + T)", B, T, need, ring_T, D);
    hipStream_t s = (hipStream_t)stream;
    CfmProfScope prof("stream_prep", s, 0.0, (double)B * ring_T * D * 8);
    CFM_LAUNCH(cfm_stream_prep_kernel, dim3((unsigned)(ring_T + (abs_rows ? 1 : 0)), (unsigned)B), dim3(64), 0, s, offsets, frame_lens, out_lens, B, T, need, ring_T,
               pe, max_len, D, slot_mask, pos_rows, abs_rows);
    return cfm_launch_status("cfm_stream_prep");
}

extern "C" int cfm_kv_ring_write(const void* k, const void* v, int32_t kv_dtype, int64_t k_sb, int64_t k_st, int64_t v_sb, int64_t v_st, float* ring,
                                 const int32_t* offsets, const int32_t* lens, int32_t B, int32_t H, int32_t T, int32_t dk, int32_t ring_T, cfm_stream_t stream) {
    CFM_CHECK_ARG(k && v && ring && offsets, "cfm_kv_ring_write: null pointer");
    CFM_CHECK_ARG(B > 0 && H > 0 && T > 0 && dk > 0 && ring_T >= T, "cfm_kv_ring_write: bad shape");
    hipStream_t s = (hipStream_t)stream;
    const int64_t n = (int64_t)B * T * H * 2 * dk;
    // the one scope that keeps its length-aware name: tests/test_stream_ragged_gpu.py tells the two ring write sites of a ragged step apart by it
    CfmProfScope prof(lens ? "kv_ring_write_len" : "kv_ring_write", s, 0.0, (double)n * (4 + cfm_elt_size(kv_dtype)));
    CFM_LAUNCH(cfm_kv_ring_write_kernel, dim3((unsigned)blocks_for(n)), dim3(256), 0, s, k, v, kv_dtype, k_sb, k_st, v_sb, v_st, ring, offsets, lens, B, H, T, dk,
               ring_T);
    return cfm_launch_status("cfm_kv_ring_write");
}

extern "C" int cfm_stream_advance(int32_t* offsets, const uint8_t* active, const int32_t* lens, float* y, int32_t B, int32_t T, int32_t D, cfm_stream_t stream) {
    CFM_CHECK_ARG(offsets && B > 0 && T > 0, "cfm_stream_advance: bad arguments");
    CFM_CHECK_ARG(!lens || !active, "cfm_stream_advance: active is not combined with lens");
    CFM_CHECK_ARG(!y || (lens && D > 0 && D % 4 == 0), "cfm_stream_advance: y needs lens and D > 0, a multiple of 4");
    hipStream_t s = (hipStream_t)stream;
    CfmProfScope prof("stream_advance", s, 0.0, (double)B * 8);
    CFM_LAUNCH(cfm_stream_advance_kernel, dim3((unsigned)B), dim3(64), 0, s, offsets, active, lens, y, T, D);
    return cfm_launch_status("cfm_stream_advance");
}

extern "C" int cfm_dwconv_causal_bn_silu(const void* x, int32_t x_dtype, const float* cache, const float* w, const float* dw_bias, const float* bn_scale,
                                         const float* bn_shift, void* y, int32_t y_dtype, int32_t B, int32_t T, int32_t D, int32_t ktaps, cfm_stream_t stream) {
    CFM_CHECK_ARG(x && w && dw_bias && bn_scale && bn_shift && y, "cfm_dwconv_causal_bn_silu: null pointer");
    CFM_CHECK_ARG(B > 0 && T > 0 && D > 0 && ktaps > 0, "cfm_dwconv_causal_bn_silu: bad shape");
    hipStream_t s = (hipStream_t)stream;
    const int64_t n = (int64_t)B * T * D;
    CfmProfScope prof("dwconv_causal", s, 2.0 * n * ktaps, (double)n * (cfm_elt_size(x_dtype) + cfm_elt_size(y_dtype)));
    CFM_LAUNCH(cfm_dwconv_causal_kernel, dim3((unsigned)blocks_for(n)), dim3(256), 0, s, x, x_dtype, cache, w, dw_bias, bn_scale, bn_shift, y, y_dtype, B, T, D, ktaps);
    return cfm_launch_status("cfm_dwconv_causal_bn_silu");
}

extern "C" int cfm_conv_cache_update(const void* x, int32_t x_dtype, float* cache, const int32_t* lens, int32_t B, int32_t T, int32_t D, int32_t ktaps,
                                     cfm_stream_t stream) {
    CFM_CHECK_ARG(x && cache, "cfm_conv_cache_update: null pointer");
    CFM_CHECK_ARG(B > 0 && T > 0 && D > 0 && ktaps > 1, "cfm_conv_cache_update: bad shape");
    hipStream_t s = (hipStream_t)stream;
    CfmProfScope prof("conv_cache_update", s, 0.0, (double)B * (ktaps - 1) * D * 8);
    CFM_LAUNCH(cfm_conv_cache_update_kernel, dim3((unsigned)blocks_for((int64_t)B * D)), dim3(256), 0, s, x, x_dtype, cache, lens, B, T, D, ktaps);
    return cfm_launch_status("cfm_conv_cache_update");
}
