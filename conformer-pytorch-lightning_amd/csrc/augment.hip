// augment.hip -- SpecAugment in place on a ragged batch of fbank features, one launch: the reference's processor.spec_aug
// (src/processor.py:151-172; num_t_mask 2, num_f_mask 2, max_t 50, max_f 50 in exp/data_config.json), which runs on the host one utterance
// at a time.  include/cfm.h (cfm_spec_augment) states the draws; tests/spec_augment_ref.py restates them in numpy integers.
//
// Grid: tiles of kRows rows x B items.  Every workgroup recomputes its item's masks into LDS (at most 32 pairs of hashes), then each
// wavefront walks its rows of the tile: a row inside a time mask is zeroed whole, any other row only in the columns of the frequency
// masks.  Nothing is loaded from feats, rows at or past the item's length and unmasked elements are never touched: the traffic is the
// masked area.  (The speed perturbation that precedes the fbank is cfm_resample_group, csrc/resample.hip.)
#include "cfm_common.h"

namespace {

constexpr int kThreads = 256, kWaves = kThreads / 64, kRows = 64;

// U[0, N - 1] from 32 random bits: multiply-high
__device__ __forceinline__ int draw(unsigned r, int N) { return (int)(((unsigned long long)r * (unsigned)N) >> 32); }

__global__ __launch_bounds__(kThreads) void cfm_spec_augment_kernel(cfm_spec_augment_desc d) {
    __shared__ int lo[CFM_SPEC_MAX_MASKS], hi[CFM_SPEC_MAX_MASKS];
    const int b = blockIdx.y, tid = threadIdx.x, nt = d.num_t_mask, nm = d.num_t_mask + d.num_f_mask;
    const int T = min(max(d.lengths[b], 0), d.T_max);
    if (tid < nm) {
        int start = 0, end = 0;
        if (T > 0 && d.F > 0) {
            const unsigned item = cfm_hash32(d.seed, d.ids ? d.ids[b] : (unsigned)b);
            const int N = tid < nt ? T : d.F, most = tid < nt ? d.max_t : d.max_f;
            start = draw(cfm_hash32(item, 2u * tid), N);
            const int len = 1 + draw(cfm_hash32(item, 2u * tid + 1u), most);     // start < 2^30 and len <= 2^30: no overflow
            end = min(N, start + len);
        }
        lo[tid] = start;
        hi[tid] = end;
        if (d.masks && blockIdx.x == 0) {
            d.masks[((int64_t)b * nm + tid) * 2] = start;
            d.masks[((int64_t)b * nm + tid) * 2 + 1] = end;
        }
    }
    __syncthreads();
    const int r0 = blockIdx.x * kRows, r1 = min(r0 + kRows, T);
    float* item = d.feats + (int64_t)b * d.item_stride;
    const int wave = tid >> 6, lane = tid & 63;
    for (int r = r0 + wave; r < r1; r += kWaves) {           // r < T: rows at or past the item's length are never touched
        float* row = item + (int64_t)r * d.row_stride;
        bool whole = false;
        for (int m = 0; m < nt; ++m) whole |= r >= lo[m] && r < hi[m];
        if (whole) {
            for (int c = lane; c < d.F; c += 64) row[c] = 0.f;
            continue;
        }
        for (int m = nt; m < nm; ++m)
            for (int c = lo[m] + lane; c < hi[m]; c += 64) row[c] = 0.f;          // hi <= F; overlapping masks store the same zero twice
    }
}

}  // namespace

extern "C" int cfm_spec_augment(const cfm_spec_augment_desc* d, cfm_stream_t stream) {
    const char* who = "cfm_spec_augment";
    CFM_CHECK_ARG(d && d->lengths, "%s: null pointer", who);
    CFM_CHECK_ARG(d->B > 0 && d->B <= 65535 && d->T_max >= 0 && d->T_max < (1 << 30) && d->F >= 0 && d->F < (1 << 30), "%s: B %d, T_max %d, F %d", who, d->B, d->T_max, d->F);
    CFM_CHECK_ARG(d->feats || d->T_max == 0 || d->F == 0, "%s: null feats", who);
    CFM_CHECK_ARG(d->row_stride >= d->F && d->item_stride >= (int64_t)d->T_max * d->row_stride, "%s: row stride %lld for %d columns, item stride %lld for %d rows", who,
                  (long long)d->row_stride, d->F, (long long)d->item_stride, d->T_max);
    CFM_CHECK_ARG(d->num_t_mask >= 0 && d->num_f_mask >= 0 && d->num_t_mask + d->num_f_mask <= CFM_SPEC_MAX_MASKS, "%s: %d time and %d frequency masks, at most %d in all", who,
                  d->num_t_mask, d->num_f_mask, CFM_SPEC_MAX_MASKS);
    CFM_CHECK_ARG(d->max_t >= 1 && d->max_t <= (1 << 30) && d->max_f >= 1 && d->max_f <= (1 << 30), "%s: max_t %d, max_f %d: mask lengths are drawn from 1 .. max", who, d->max_t,
                  d->max_f);
    const int tiles = d->T_max > 0 ? (d->T_max + kRows - 1) / kRows : 1;      // one workgroup per item at least: it writes the masks table
    hipStream_t s = (hipStream_t)stream;
    CfmProfScope prof("spec_augment", s, 0.0, 0.0);          // stores alone, of a size only the draws know
    CFM_LAUNCH(cfm_spec_augment_kernel, dim3((unsigned)tiles, (unsigned)d->B), dim3(kThreads), 0, s, *d);
    return cfm_launch_status(who);
}
