// fbank.hip -- Kaldi-compatible log-mel filter bank on the device: waveform in, feature rows out, one launch, nothing in between in HBM.
// The reference computes it on the host with torchaudio: kaldi.fbank(waveform * (1 << 15), num_mel_bins=80, frame_length=25, frame_shift=10,
// dither, energy_floor=0, sample_frequency=16000), src/processor.py:175-193 (compute_fbank), src/deploy.py:106-146 (preprocess, preprocess_stream).
//
// One wavefront per frame, 4 wavefronts per workgroup, FR frames after one another per wavefront (a workgroup = 16 consecutive rows of one item):
//   samples (int16 | f32; a streaming frame may begin in the stream's carry and end in the new block: one index map) -> + dither -> - mean
//   (wavefront reduction) -> pre-emphasis -> povey window -> zero-pad -> the `padded`-point real transform as a padded/2-point complex
//   Stockham FFT (radix 4, one radix-2 stage when the size asks for it) in LDS -> unpack + |.|^2 -> sparse mel product -> logf -> store.
//
// PRECISION.  The frame pipeline up to the power spectrum runs in float64, the mel sum accumulates f32 weights in float64, logf is f32.  The
// parity gate is max |device - float64 reference| <= 2 x (float32 torch restatement's same error), a maximum over cells whose worst one is a
// small mel energy next to a large bin of the same frame: a float32 FFT errs by ~1e-7 of the frame's LARGEST bin whatever its factorisation,
// and restating this kernel's f32 radix-4 arithmetic on the host gave between 0.9 x and 2.3 x the torch error depending on the signal and
// on how products were fused -- a coin toss against a factor 2.  The transform is 9k flops per frame; in float64 it costs nothing
// that shows next to the LDS round trips, and it takes the FFT out of the error budget ("Log-mel fbank").
#include "cfm_common.h"

namespace {

constexpr int kWaves = 4, kFR = 4, kRowsPerBlock = kWaves * kFR, kMaxPad = 512, kMaxT = kMaxPad / 64, kMaxNnz = 512;
constexpr float kEps = 1.1920929e-07f;

struct d2 {
    double x, y;
};
__device__ __forceinline__ d2 operator+(d2 a, d2 b) { return {a.x + b.x, a.y + b.y}; }
__device__ __forceinline__ d2 operator-(d2 a, d2 b) { return {a.x - b.x, a.y - b.y}; }
__device__ __forceinline__ d2 cmul(d2 a, d2 w) { return {a.x * w.x - a.y * w.y, a.x * w.y + a.y * w.x}; }
__device__ __forceinline__ d2 mul_i(d2 a) { return {-a.y, a.x}; }

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// standard normal draw number j of frame `frame` of item b: two 24-bit uniforms from the counter hash, Box-Muller
__device__ __forceinline__ float dither_normal(unsigned key, unsigned j) {
    const unsigned a = cfm_hash32(key, 2u * j), c = cfm_hash32(key, 2u * j + 1u);
    const float u1 = (float)((a >> 8) + 1u) * (1.0f / 16777216.0f);          // (0, 1]
    const float u2 = (float)(c >> 8) * (1.0f / 16777216.0f);                 // [0, 1)
    return sqrtf(-2.0f * logf(u1)) * cosf(6.28318530717958647692f * u2);
}

struct Src {                     // the sample sequence of one item: [0, cn) from the carry, [cn, len) from the block
    const void* blk;
    const float* carry;
    int cn, len, i16, ncols;
    __device__ __forceinline__ float at(int v) const {
        if (v < cn) return carry[v];
        if (v - cn >= ncols) return 0.f;                     // a block narrower than a fresh stream's first read (the host refuses it; never read past the row)
        return i16 ? (float)((const int16_t*)blk)[v - cn] : ((const float*)blk)[v - cn];
    }
};

// kRagged: the streaming mode for audio packets of any size (cfm_fbank_desc.n_new set), its own instantiation: the offline and the whole-block
// streaming mode are the kRagged = false one, whose code does not know the third mode exists.
template <bool kRagged>
__global__ __launch_bounds__(kWaves * 64) void cfm_fbank_kernel(cfm_fbank_desc d, int streaming, int frame_blocks) {
    __shared__ d2 tw[kMaxPad];
    __shared__ double wnd[kMaxPad];
    __shared__ float melw[kMaxNnz];
    __shared__ d2 buf[kWaves][2][kMaxPad / 2];

    const int b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int P = d.padded, N = P >> 1, win = d.win;

    Src s;
    s.i16 = d.samples_i16;
    s.ncols = d.n_cols;
    s.blk = (const char*)d.samples + (int64_t)b * d.ld * (d.samples_i16 ? 2 : 4);
    int pos = 0, m;
    if constexpr (kRagged) {                               // a carry of carry_len_in[b] <= carry_cap samples, n_new[b] new ones, 0 .. rows frames
        const bool fresh = d.fresh_in[b] != 0;
        s.cn = fresh ? 0 : min(max(d.carry_len_in[b], 0), d.carry_cap);
        s.carry = d.carry_in + (int64_t)b * d.carry_cap;
        s.ncols = min(max(d.n_new[b], 0), d.n_cols);       // a read at or past the stream's own count yields 0
        s.len = s.cn + s.ncols;
        pos = fresh ? 0 : d.pos_in[b];
        m = d.rows;                                        // a whole window, the short last one of a finished utterance, or nothing (buffering)
        if (s.len < (d.rows - 1) * d.shift + win) m = d.final[b] == 0 || s.len < win ? 0 : 1 + (s.len - win) / d.shift;
    } else if (streaming) {
        const bool fresh = d.fresh_in[b] != 0;
        s.cn = fresh ? 0 : d.carry_n;
        s.carry = d.carry_in + (int64_t)b * d.carry_n;
        s.len = (d.rows - 1) * d.shift + win;
        pos = fresh ? 0 : d.pos_in[b];
        m = d.rows;
    } else {
        s.cn = 0;
        s.carry = nullptr;
        s.len = min(max(d.lengths[b], 0), d.n_cols);
        m = s.len >= win ? 1 + (s.len - win) / d.shift : 0;
    }

    if ((int)blockIdx.x == frame_blocks) {                 // the item's bookkeeping block
        if constexpr (kRagged) {
            // the sequence loses a hop at its head after a whole window, 4 c frames after a short one of c encoder frames (cfm_stream_prep's count)
            const int adv = m == d.rows ? d.hop : m < 7 ? 0 : 4 * (((m - 1) / 2 - 1) / 2), used = adv * d.shift;
            const int keep = min(s.len - used, d.carry_cap);                          // the host mirror refuses a packet that would overfill the carry
            for (int v = tid; v < keep; v += kWaves * 64) {                           // used + v < s.len: in the carry or the stream's own new samples; B * carry_cap < 2^31 (checked at the launch)
                const int i = used + v - s.cn;
                d.carry_out[b * d.carry_cap + v] = i < 0 ? s.carry[used + v] : s.i16 ? (float)((const int16_t*)s.blk)[i] : ((const float*)s.blk)[i];
            }
            if (tid == 0) {
                d.carry_len_out[b] = keep;
                d.fresh_out[b] = 0;
                d.pos_out[b] = pos + adv;
                d.frame_lens[b] = m;
            }
        } else if (streaming) {
            for (int v = tid; v < d.carry_n; v += kWaves * 64) d.carry_out[(int64_t)b * d.carry_n + v] = s.at(s.len - d.carry_n + v);
            if (tid == 0) {
                d.fresh_out[b] = 0;
                d.pos_out[b] = pos + d.hop;
            }
        } else if (tid == 0 && d.feats_length) {
            d.feats_length[b] = min(m, d.rows);
        }
        return;
    }

    const int row0 = blockIdx.x * kRowsPerBlock;
    float* out = d.out + ((int64_t)b * d.rows + row0) * d.F;
    if (row0 >= m) {                                        // nothing but padding rows here (block-uniform: no barrier is skipped by a part)
        const int n = min(kRowsPerBlock, d.rows - row0) * d.F;
        for (int i = tid; i < n; i += kWaves * 64) out[i] = 0.f;
        return;
    }

    for (int i = tid; i < P; i += kWaves * 64) tw[i] = {d.twiddle[2 * i], d.twiddle[2 * i + 1]};
    for (int i = tid; i < win; i += kWaves * 64) wnd[i] = d.window[i];
    for (int i = tid; i < d.mel_nnz; i += kWaves * 64) melw[i] = d.mel_w[i];
    const unsigned key_b = cfm_hash32(d.seed, (unsigned)b);
    __syncthreads();

    for (int it = 0; it < kFR; ++it) {
        const int r = row0 + wave * kFR + it;
        const bool in_rows = r < d.rows, valid = r < m;     // padding rows run the arithmetic on zeros: every wave meets every barrier
        const int v0 = r * d.shift;
        double* ra = (double*)buf[wave][0];
        double* rb = (double*)buf[wave][1];

        double x[kMaxT], sum = 0.0;
        const unsigned key = cfm_hash32(key_b, (unsigned)(pos + r));
#pragma unroll
        for (int t = 0; t < kMaxT; ++t) {
            const int j = lane + 64 * t;
            float v = 0.f;
            if (valid && j < win) {
                v = s.at(v0 + j);
                if (d.dither > 0.f) v += d.dither * dither_normal(key, (unsigned)j);
            }
            x[t] = (double)v;
            sum += x[t];
        }
        const double mean = wave_sum_f64(sum) / (double)win;
#pragma unroll
        for (int t = 0; t < kMaxT; ++t) {
            const int j = lane + 64 * t;
            if (j < P) ra[j] = x[t] - mean;
        }
        __syncthreads();
#pragma unroll
        for (int t = 0; t < kMaxT; ++t) {
            const int j = lane + 64 * t;
            if (j < P) rb[j] = j < win ? (ra[j] - 0.97 * ra[j > 0 ? j - 1 : 0]) * wnd[j] : 0.0;
        }
        __syncthreads();

        // z[n] = y[2n] + i y[2n+1] is rb read as complex.  Stockham autosort, decimation in frequency: length n, stride st, src -> dst per stage.
        d2* src = buf[wave][1];
        d2* dst = buf[wave][0];
        int n = N, st = 1;
        while (n >= 4) {
            const int n1 = n >> 2, step = P / n;
            for (int i = lane; i < (N >> 2); i += 64) {
                const int p = i / st, q = i - p * st;
                const d2 a = src[q + st * p], bb = src[q + st * (p + n1)], c = src[q + st * (p + 2 * n1)], e = src[q + st * (p + 3 * n1)];
                const d2 apc = a + c, amc = a - c, bpd = bb + e, jbmd = mul_i(bb - e);
                const int k = p * step;
                dst[q + st * (4 * p)] = apc + bpd;
                dst[q + st * (4 * p + 1)] = cmul(amc - jbmd, tw[k]);
                dst[q + st * (4 * p + 2)] = cmul(apc - bpd, tw[2 * k]);
                dst[q + st * (4 * p + 3)] = cmul(amc + jbmd, tw[3 * k]);
            }
            __syncthreads();
            d2* t2 = src; src = dst; dst = t2;
            n >>= 2;
            st <<= 2;
        }
        if (n == 2) {
            for (int i = lane; i < (N >> 1); i += 64) {     // p = 0: the twiddle is 1
                const d2 a = src[i], bb = src[i + st];
                dst[i] = a + bb;
                dst[i + st] = a - bb;
            }
            __syncthreads();
            d2* t2 = src; src = dst; dst = t2;
        }

        // X[k] = (Z[k] + conj Z[N-k]) / 2 - i W_P^k (Z[k] - conj Z[N-k]) / 2,  k < N (the Nyquist bin has mel weight 0);  power -> dst as f64 [N]
        double* pw = (double*)dst;
        for (int k = lane; k < N; k += 64) {
            const d2 z = src[k], zc = src[(N - k) & (N - 1)];
            const d2 ev = {0.5 * (z.x + zc.x), 0.5 * (z.y - zc.y)}, od = {0.5 * (z.x - zc.x), 0.5 * (z.y + zc.y)};
            const d2 t = cmul(od, tw[k]);
            const double xr = ev.x + t.y, xi = ev.y - t.x;
            pw[k] = xr * xr + xi * xi;
        }
        __syncthreads();
        if (in_rows) {
            float* orow = out + (int64_t)(wave * kFR + it) * d.F;
            for (int f = lane; f < d.F; f += 64) {
                float res = 0.f;
                if (valid) {
                    const int k0 = d.mel_start[f], len = d.mel_len[f], o = d.mel_off[f];
                    double acc = 0.0;
                    for (int i = 0; i < len; ++i) acc += pw[k0 + i] * (double)melw[o + i];
                    res = logf(fmaxf((float)acc, kEps));
                }
                orow[f] = res;
            }
        }
        __syncthreads();
    }
}

int fbank_launch(const cfm_fbank_desc* d, int streaming, cfm_stream_t stream, const char* who) {
    CFM_CHECK_ARG(d && (d->samples || (streaming && d->n_new && d->n_cols == 0)) && d->twiddle && d->window && d->mel_w && d->mel_start && d->mel_len && d->mel_off && d->out, "%s: null pointer", who);
    CFM_CHECK_ARG(d->B > 0 && d->B <= 65535 && d->rows > 0 && d->F > 0, "%s: B %d rows %d F %d", who, d->B, d->rows, d->F);
    CFM_CHECK_ARG(d->padded >= 8 && d->padded <= kMaxPad && (d->padded & (d->padded - 1)) == 0 && d->win >= 2 && d->win <= d->padded && d->shift >= 1,
                  "%s: window %d padded to %d, shift %d: the padded window must be a power of two in [8, %d]", who, d->win, d->padded, d->shift, kMaxPad);
    CFM_CHECK_ARG(d->mel_nnz > 0 && d->mel_nnz <= kMaxNnz, "%s: %d packed mel weights (at most %d)", who, d->mel_nnz, kMaxNnz);
    CFM_CHECK_ARG((int64_t)(d->rows - 1) * d->shift + d->win < (1ll << 30), "%s: rows %d: sample index out of range", who, d->rows);
    const int64_t n_first = (int64_t)(d->rows - 1) * d->shift + d->win;
    if (streaming) {
        CFM_CHECK_ARG(d->carry_in && d->carry_out && d->fresh_in && d->fresh_out && d->pos_in && d->pos_out, "%s: null state pointer", who);
        CFM_CHECK_ARG(d->carry_in != d->carry_out && d->fresh_in != d->fresh_out && d->pos_in != d->pos_out, "%s: state in and out alias", who);
    }
    if (streaming && d->n_new) {                           // audio packets of any size
        CFM_CHECK_ARG(d->final && d->carry_len_in && d->carry_len_out && d->frame_lens && d->carry_len_in != d->carry_len_out, "%s: ragged packets: null or aliased length state", who);
        CFM_CHECK_ARG(d->hop > 0 && (int64_t)d->hop * d->shift < n_first && d->carry_cap >= n_first - 1 && d->carry_cap < (1 << 30),
                      "%s: ragged packets: hop %d, a carry of %d samples for a %lld-sample window", who, d->hop, d->carry_cap, (long long)n_first);
        CFM_CHECK_ARG(d->n_cols >= 0 && d->n_cols < (1 << 30) && d->ld >= d->n_cols, "%s: %d columns (ld %lld)", who, d->n_cols, (long long)d->ld);
        CFM_CHECK_ARG((int64_t)d->B * d->carry_cap < (1ll << 31), "%s: ragged packets: %d streams x a carry of %d samples: the carry is indexed in 32 bits", who, d->B, d->carry_cap);
    } else if (streaming) {
        CFM_CHECK_ARG(d->carry_n >= 0 && d->carry_n < n_first && d->hop > 0, "%s: carry %d of a %lld-sample window, hop %d", who, d->carry_n, (long long)n_first, d->hop);
        CFM_CHECK_ARG(d->n_cols >= n_first - d->carry_n && d->ld >= d->n_cols, "%s: %d columns (ld %lld), a stream reads %lld new samples (%lld after a reset)", who, d->n_cols,
                      (long long)d->ld, (long long)(n_first - d->carry_n), (long long)n_first);
    } else {
        CFM_CHECK_ARG(d->lengths && d->n_cols >= 0 && d->ld >= d->n_cols, "%s: lengths / n_cols %d / ld %lld", who, d->n_cols, (long long)d->ld);
    }
    const int frame_blocks = (d->rows + kRowsPerBlock - 1) / kRowsPerBlock;
    hipStream_t s = (hipStream_t)stream;
    const double frames = (double)d->B * d->rows;
    CfmProfScope prof(streaming ? "fbank_stream" : "fbank", s, frames * (5.0 * d->padded * 8 + 2.0 * d->mel_nnz),
                      (double)d->B * ((double)d->rows * d->shift * (d->samples_i16 ? 2 : 4) + (double)d->rows * d->F * 4));
    if (streaming && d->n_new)
        CFM_LAUNCH(cfm_fbank_kernel<true>, dim3((unsigned)frame_blocks + 1, (unsigned)d->B), dim3(kWaves * 64), 0, s, *d, streaming, frame_blocks);
    else
        CFM_LAUNCH(cfm_fbank_kernel<false>, dim3((unsigned)frame_blocks + 1, (unsigned)d->B), dim3(kWaves * 64), 0, s, *d, streaming, frame_blocks);
    return cfm_launch_status(who);
}

}  // namespace

extern "C" int cfm_fbank(const cfm_fbank_desc* d, cfm_stream_t stream) { return fbank_launch(d, 0, stream, "cfm_fbank"); }
extern "C" int cfm_fbank_stream(const cfm_fbank_desc* d, cfm_stream_t stream) { return fbank_launch(d, 1, stream, "cfm_fbank_stream"); }
