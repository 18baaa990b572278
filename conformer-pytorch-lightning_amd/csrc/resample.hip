// resample.hip -- sample-rate conversion on the device: waveform in, waveform out, one launch.  The reference does it on the host with torchaudio,
// Resample(orig_freq=sample_rate, new_freq=16000)(waveform), as the first line of preprocess / preprocess_stream (src/deploy.py:108-110, :129-131)
// and in processor.resample (src/processor.py:49-59): a polyphase FIR bank, n phases of 2 width + o taps (include/cfm.h has the formula).
//
// One workgroup per tile of tile_blocks(o, n, width) input blocks (o samples in, n samples out each) of one item or stream; a lane produces one output
// sample at a time.  In LDS: the compact bank (each phase's run of live taps, computed in float64 on the host), its two index vectors, and the
// tile's input span tile_blocks * o + 2 width + o samples with the zero padding materialised as 0.0f.  The input sequence of an item is
// `head` samples from the stream's tail buffer (offline: the `width` zeros of the left padding) followed by its new samples, then zeros.
//
// SUMMATION ORDER.  out = one f32 fmaf chain over the phase's live taps in ascending tap order from +0.0f, operands read from LDS: the same
// instruction sequence on the same values whichever tile, call or mode computes the sample, so streaming output equals offline output bit for bit.
// A workgroup past the last tile of its row does the row's bookkeeping: the output length and, streaming, the new tail and counts.
#include "cfm_common.h"

namespace {

constexpr int kThreads = 256, kMaxPhases = 1024, kMaxLive = 16384, kTileOut = 2048, kTileIn = 8192, kMaxLds = 128 * 1024;

// input blocks per tile: about kTileOut output samples, at most about kTileIn input samples, at least one block; 0 when the largest bank
// (kMaxLive taps) and the span exceed kMaxLds -- a function of the rate pair alone, so the answer does not depend on the table
int tile_blocks(int o, int n, int width) {
    if (o < 1 || n < 1 || n > kMaxPhases || width < 1) return 0;
    int tb = kTileOut / n < kTileIn / o ? kTileOut / n : kTileIn / o;
    if (tb < 1) tb = 1;
    const int64_t lds = 4 * ((int64_t)kMaxLive + 2 * n + 1 + (int64_t)tb * o + 2 * (int64_t)width + o);
    return lds <= kMaxLds ? tb : 0;
}

struct Seq {                     // the sample sequence of one item: [0, head) from the tail buffer, [head, head + nn) from its row, zeros behind
    const void* blk;
    const float* tail;           // null: the head is zeros (offline)
    int head, zeros, nn, i16;    // the first `zeros` samples of the head lie before sample 0 of the utterance: the left padding
    __device__ __forceinline__ float at(int64_t v) const {
        if (v < head) return (tail && v >= zeros) ? tail[v] : 0.f;
        v -= head;
        if (v >= nn) return 0.f;                             // never read past the item's own samples
        return i16 ? (float)((const int16_t*)blk)[v] : ((const float*)blk)[v];
    }
};

__global__ __launch_bounds__(kThreads) void cfm_resample_kernel(cfm_resample_desc d, int streaming, int tiles, int tb) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int b = blockIdx.y, tid = threadIdx.x, o = d.o, n = d.n, w = d.width;
    const int K = 2 * w + o, span = tb * o + K;
    float* taps = lds;                                       // [n_live]
    int* first = (int*)(lds + d.n_live);                     // [n]
    int* off = first + n;                                    // [n + 1]
    float* x = (float*)(off + n + 1);                        // [span]

    Seq s;
    s.i16 = d.samples_i16;
    s.blk = (const char*)d.samples + (int64_t)b * d.ld * (d.samples_i16 ? 2 : 4);
    int64_t seen = 0, blocks = 0;
    bool fin = true;
    if (streaming) {
        seen = d.counts_in[2 * b];
        blocks = d.counts_in[2 * b + 1];
        const int64_t held = seen - blocks * o + w;          // the host mirror keeps it in [width, tail_cap]; clamped: never index outside the buffers
        s.head = (int)(held < w ? w : held > d.tail_cap ? d.tail_cap : held);
        s.zeros = blocks == 0 ? w : 0;
        s.tail = d.tail_in + (int64_t)b * d.tail_cap;
        s.nn = min(max(d.n_new[b], 0), d.n_cols);
        fin = d.final[b] != 0;
    } else {
        s.head = s.zeros = w;
        s.tail = nullptr;
        s.nn = min(max(d.lengths[b], 0), d.n_cols);
    }
    const int64_t T = (int64_t)s.head + s.nn;                // the sequence's samples; behind them zeros
    // whole blocks whose every tap has arrived: (q + 1) o + width <= c  <=>  (q - Q + 1) o <= T - 2 width
    const int64_t nb = T >= 2 * w ? (T - 2 * w) / o : 0;
    int64_t emit = fin ? ((T - w) * n + o - 1) / o : nb * n;
    if (emit > d.cap) emit = d.cap;                          // the caller sizes `out` from the host mirror; never write past it

    if ((int)blockIdx.x == tiles) {                          // the row's bookkeeping block
        if (tid == 0) d.out_lens[b] = (int)emit;
        if (!streaming) return;
        const int64_t used = fin ? T : nb * o;             // a final call leaves the stream reset
        const int keep = T - used < d.tail_cap ? (int)(T - used) : d.tail_cap;
        float* to = d.tail_out + (int64_t)b * d.tail_cap;
        for (int v = tid; v < d.tail_cap; v += kThreads) to[v] = v < keep ? s.at(used + v) : 0.f;
        if (tid == 0) {
            d.counts_out[2 * b] = fin ? 0 : seen + s.nn;
            d.counts_out[2 * b + 1] = fin ? 0 : blocks + nb;
        }
        return;
    }

    const int64_t col0 = (int64_t)blockIdx.x * tb * n;       // the tile's first output sample; col0 < cap by the grid
    const int cols = (int64_t)tb * n < d.cap - col0 ? tb * n : (int)(d.cap - col0);
    float* out = d.out + (int64_t)b * d.ld_out + col0;
    if (col0 >= emit) {                                      // nothing but padding here (block-uniform: no barrier is skipped by a part)
        for (int p = tid; p < cols; p += kThreads) out[p] = 0.f;
        return;
    }

    for (int i = tid; i < d.n_live; i += kThreads) taps[i] = d.taps[i];
    for (int i = tid; i < n; i += kThreads) first[i] = d.tap_first[i];
    for (int i = tid; i <= n; i += kThreads) off[i] = d.tap_off[i];
    const int64_t v0 = (int64_t)blockIdx.x * tb * o;
    for (int i = tid; i < span; i += kThreads) x[i] = s.at(v0 + i);
    __syncthreads();

    const int live = emit - col0 < cols ? (int)(emit - col0) : cols;
    for (int p = tid; p < cols; p += kThreads) {
        float acc = 0.f;
        if (p < live) {
            const int q = p / n, j = p - q * n;
            const int a = off[j], len = off[j + 1] - a;
            const float* xs = x + q * o + first[j];          // first[j] + len <= K: inside the span
            for (int i = 0; i < len; ++i) acc = fmaf(taps[a + i], xs[i], acc);
        }
        out[p] = acc;
    }
}

int resample_launch(const cfm_resample_desc* d, int streaming, cfm_stream_t stream, const char* who) {
    CFM_CHECK_ARG(d && d->taps && d->tap_first && d->tap_off && d->out_lens, "%s: null pointer", who);
    CFM_CHECK_ARG(d->B > 0 && d->B <= 65535 && d->cap >= 0 && d->cap < (1 << 30) && (d->out || d->cap == 0) && d->ld_out >= d->cap, "%s: B %d, %d output columns (ld %lld)", who,
                  d->B, d->cap, (long long)d->ld_out);
    CFM_CHECK_ARG(d->n_cols >= 0 && d->n_cols < (1 << 30) && (d->samples || d->n_cols == 0) && d->ld >= d->n_cols, "%s: %d columns (ld %lld)", who, d->n_cols, (long long)d->ld);
    CFM_CHECK_ARG(d->o >= 1 && d->n >= 1 && d->n <= kMaxPhases && d->width >= 1 && d->n_live >= d->n && d->n_live <= kMaxLive,
                  "%s: %d -> %d (reduced rates), width %d, %d live taps: at most %d phases and %d taps", who, d->o, d->n, d->width, d->n_live, kMaxPhases, kMaxLive);
    const int tb = tile_blocks(d->o, d->n, d->width);
    CFM_CHECK_ARG(tb > 0, "%s: %d -> %d (reduced rates), width %d: the bank and one tile's input span exceed %d bytes of LDS", who, d->o, d->n, d->width, kMaxLds);
    if (streaming) {
        CFM_CHECK_ARG(d->n_new && d->final && d->tail_in && d->tail_out && d->counts_in && d->counts_out, "%s: null state pointer", who);
        CFM_CHECK_ARG(d->tail_in != d->tail_out && d->counts_in != d->counts_out, "%s: state in and out alias", who);
        CFM_CHECK_ARG(d->tail_cap >= 2 * d->width + d->o && d->tail_cap < (1 << 24), "%s: a tail of %d samples; a stream holds up to 2 width + o = %d", who, d->tail_cap,
                      2 * d->width + d->o);
    } else {
        CFM_CHECK_ARG(d->lengths, "%s: null lengths", who);
    }
    const int K = 2 * d->width + d->o;
    const size_t lds = 4 * ((size_t)d->n_live + 2 * d->n + 1 + (size_t)tb * d->o + K);
    static bool attr_set = false;                           // > 64 KB of dynamic LDS needs the attribute once per process
    if (!attr_set) {
        if (hipFuncSetAttribute((const void*)cfm_resample_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, kMaxLds) != hipSuccess)
            return cfm_fail(CFM_ERR_LAUNCH, "%s: cannot raise the dynamic LDS limit", who);
        attr_set = true;
    }
    const int64_t tile_out = (int64_t)tb * d->n;
    const int tiles = (int)((d->cap + tile_out - 1) / tile_out);
    hipStream_t s = (hipStream_t)stream;
    CfmProfScope prof(streaming ? "resample_stream" : "resample", s, 2.0 * d->B * d->cap * K,
                      (double)d->B * ((double)d->cap * d->o / d->n * (d->samples_i16 ? 2 : 4) + (double)d->cap * 4));
    CFM_LAUNCH(cfm_resample_kernel, dim3((unsigned)tiles + 1, (unsigned)d->B), dim3(kThreads), lds, s, *d, streaming, tiles, tb);
    return cfm_launch_status(who);
}

// ---------------------------------------------------------------------------------------------
// cfm_resample_group: the offline kernel with one rate pair per item -- speed perturbation of a batch that mixes speeds in one launch.  Item b uses
// bank g = bank[b]; its workgroups load that bank alone into LDS and walk the item in that bank's tiles, so a sample is the same fmaf chain over the
// same LDS operands as in cfm_resample_kernel at that pair.  The grid is sized from the bank with the most tiles; a workgroup past its own item's
// tiles leaves at once.  An identity bank (o == n) copies (int16 -> f32 is exact) in tiles of kTileOut samples and needs no table.
// ---------------------------------------------------------------------------------------------
int group_tile_out(const cfm_resample_bank& k) {              // output samples per tile of this bank; 0: does not fit
    return k.o == k.n ? kTileOut : tile_blocks(k.o, k.n, k.width) * k.n;
}

__global__ __launch_bounds__(kThreads) void cfm_resample_group_kernel(cfm_resample_group_desc d, int tiles) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int b = blockIdx.y, tid = threadIdx.x;
    const int g = min(max(d.bank[b], 0), d.G - 1);
    cfm_resample_bank k = d.banks[0];
#pragma unroll
    for (int i = 1; i < CFM_RESAMPLE_MAX_BANKS; ++i)          // a select per bank: the table stays in scalar registers
        if (i == g) k = d.banks[i];
    const int o = k.o, n = k.n, w = k.width;
    const bool same = o == n;

    Seq s;
    s.i16 = d.samples_i16;
    s.blk = (const char*)d.samples + (int64_t)b * d.ld * (d.samples_i16 ? 2 : 4);
    s.head = s.zeros = same ? 0 : w;
    s.tail = nullptr;
    s.nn = min(max(d.lengths[b], 0), d.n_cols);
    int64_t emit = same ? s.nn : ((int64_t)s.nn * n + o - 1) / o;
    if (emit > d.cap) emit = d.cap;

    if ((int)blockIdx.x == tiles) {                          // the row's bookkeeping block
        if (tid == 0) d.out_lens[b] = (int)emit;
        return;
    }
    const int tb = same ? 0 : k.tile_blocks;
    const int tile_out = same ? kTileOut : tb * n;
    const int64_t col0 = (int64_t)blockIdx.x * tile_out;     // the tile's first output sample
    if (col0 >= d.cap) return;                               // this bank has fewer tiles than the grid (block-uniform)
    const int cols = tile_out < d.cap - col0 ? tile_out : (int)(d.cap - col0);
    float* out = d.out + (int64_t)b * d.ld_out + col0;
    if (col0 >= emit) {                                      // nothing but padding here (block-uniform: no barrier is skipped by a part)
        for (int p = tid; p < cols; p += kThreads) out[p] = 0.f;
        return;
    }
    if (same) {
        for (int p = tid; p < cols; p += kThreads) out[p] = s.at(col0 + p);      // zeros at and past the item's samples
        return;
    }

    const int K = 2 * w + o, span = tb * o + K;
    float* taps = lds;                                       // [n_live]
    int* first = (int*)(lds + k.n_live);                     // [n]
    int* off = first + n;                                    // [n + 1]
    float* x = (float*)(off + n + 1);                        // [span]
    for (int i = tid; i < k.n_live; i += kThreads) taps[i] = d.taps[k.taps_at + i];
    for (int i = tid; i < n; i += kThreads) first[i] = d.tap_first[k.first_at + i];
    for (int i = tid; i <= n; i += kThreads) off[i] = d.tap_off[k.off_at + i];
    const int64_t v0 = (int64_t)blockIdx.x * tb * o;
    for (int i = tid; i < span; i += kThreads) x[i] = s.at(v0 + i);
    __syncthreads();

    const int live = emit - col0 < cols ? (int)(emit - col0) : cols;
    for (int p = tid; p < cols; p += kThreads) {
        float acc = 0.f;
        if (p < live) {
            const int q = p / n, j = p - q * n;
            const int a = off[j], len = off[j + 1] - a;
            const float* xs = x + q * o + first[j];          // first[j] + len <= K: inside the span
            for (int i = 0; i < len; ++i) acc = fmaf(taps[a + i], xs[i], acc);
        }
        out[p] = acc;
    }
}

}  // namespace

extern "C" int cfm_resample_group(const cfm_resample_group_desc* d, cfm_stream_t stream) {
    const char* who = "cfm_resample_group";
    CFM_CHECK_ARG(d && d->lengths && d->bank && d->out_lens, "%s: null pointer", who);
    CFM_CHECK_ARG(d->B > 0 && d->B <= 65535 && d->cap >= 0 && d->cap < (1 << 30) && (d->out || d->cap == 0) && d->ld_out >= d->cap, "%s: B %d, %d output columns (ld %lld)", who,
                  d->B, d->cap, (long long)d->ld_out);
    CFM_CHECK_ARG(d->n_cols >= 0 && d->n_cols < (1 << 30) && (d->samples || d->n_cols == 0) && d->ld >= d->n_cols, "%s: %d columns (ld %lld)", who, d->n_cols, (long long)d->ld);
    CFM_CHECK_ARG(d->G >= 1 && d->G <= CFM_RESAMPLE_MAX_BANKS, "%s: %d banks, 1 .. %d", who, d->G, CFM_RESAMPLE_MAX_BANKS);
    size_t lds = 0;
    int tiles = 0, kmax = 1;                                 // kmax: the longest window, for the profile's operation count
    for (int g = 0; g < d->G; ++g) {
        const cfm_resample_bank& k = d->banks[g];
        CFM_CHECK_ARG(k.o >= 1 && k.n >= 1 && k.n <= kMaxPhases, "%s: bank %d: %d -> %d (reduced rates): at most %d phases", who, g, k.o, k.n, kMaxPhases);
        const int tile_out = group_tile_out(k);
        if (k.o != k.n) {
            CFM_CHECK_ARG(d->taps && d->tap_first && d->tap_off, "%s: null table", who);
            CFM_CHECK_ARG(k.width >= 1 && k.n_live >= k.n && k.n_live <= kMaxLive, "%s: bank %d: width %d, %d live taps for %d phases: at most %d taps", who, g, k.width, k.n_live,
                          k.n, kMaxLive);
            CFM_CHECK_ARG(tile_out > 0 && k.tile_blocks == tile_out / k.n, "%s: bank %d: %d -> %d, width %d: tile_blocks %d, cfm_resample_tile_blocks gives %d (0: the bank and one tile's "
                          "input span exceed %d bytes of LDS)", who, g, k.o, k.n, k.width, k.tile_blocks, tile_out / k.n, kMaxLds);
            CFM_CHECK_ARG(k.taps_at >= 0 && k.first_at >= 0 && k.off_at >= 0 && (int64_t)k.taps_at + k.n_live <= d->n_taps && (int64_t)k.first_at + k.n <= d->n_first &&
                              (int64_t)k.off_at + k.n + 1 <= d->n_off,
                          "%s: bank %d lies outside the tables (%d taps, %d first, %d offsets)", who, g, d->n_taps, d->n_first, d->n_off);
            const size_t need = 4 * ((size_t)k.n_live + 2 * k.n + 1 + (size_t)k.tile_blocks * k.o + 2 * k.width + k.o);
            if (need > lds) lds = need;
            if (2 * k.width + k.o > kmax) kmax = 2 * k.width + k.o;
        }
        const int t = (int)((d->cap + tile_out - 1) / tile_out);
        if (t > tiles) tiles = t;
    }
    static bool attr_set = false;                           // > 64 KB of dynamic LDS needs the attribute once per process
    if (!attr_set) {
        if (hipFuncSetAttribute((const void*)cfm_resample_group_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, kMaxLds) != hipSuccess)
            return cfm_fail(CFM_ERR_LAUNCH, "%s: cannot raise the dynamic LDS limit", who);
        attr_set = true;
    }
    hipStream_t s = (hipStream_t)stream;
    CfmProfScope prof("resample_group", s, 2.0 * d->B * d->cap * kmax, (double)d->B * ((double)d->cap * (d->samples_i16 ? 2 : 4) + (double)d->cap * 4));
    CFM_LAUNCH(cfm_resample_group_kernel, dim3((unsigned)tiles + 1, (unsigned)d->B), dim3(kThreads), lds, s, *d, tiles);
    return cfm_launch_status(who);
}

extern "C" int cfm_resample(const cfm_resample_desc* d, cfm_stream_t stream) { return resample_launch(d, 0, stream, "cfm_resample"); }
extern "C" int cfm_resample_stream(const cfm_resample_desc* d, cfm_stream_t stream) { return resample_launch(d, 1, stream, "cfm_resample_stream"); }
extern "C" int32_t cfm_resample_tile_blocks(int32_t o, int32_t n, int32_t width) {
    return tile_blocks(o, n, width);
}
