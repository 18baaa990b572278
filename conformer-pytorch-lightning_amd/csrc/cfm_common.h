// cfm_common.h -- shared device/host helpers for libconformer_gfx950 (gfx950 / CDNA4 only).
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <stdint.h>

#include "../../include/cfm.h"

// ---------------------------------------------------------------------------------------------
// host side: error text + launch check + profiling hooks (abi.cpp)
// ---------------------------------------------------------------------------------------------
int cfm_fail(int code, const char* fmt, ...);

struct CfmProfScope {  // one kernel launch; when profiling is on, CFM_LAUNCH hands its two events to the launch itself
    CfmProfScope(const char* name, hipStream_t s, double flops, double bytes);
    ~CfmProfScope();
    void* rec;
    hipStream_t stream;
    hipEvent_t ev_start, ev_stop;
};

// Launch inside a function that declared `CfmProfScope prof(...)`.  With profiling on, the start/stop events are attached to the
// dispatch itself (hipExtLaunchKernelGGL): they carry the kernel's own begin/end timestamps -- what rocprofv3 reports as its
// duration -- instead of bracketing it with separately recorded events (which adds ~2 us of event processing per launch).
#define CFM_LAUNCH(kernel, grid, block, lds, stream, ...)                                                                     \
    do {                                                                                                                     \
        if (prof.rec) hipExtLaunchKernelGGL(kernel, grid, block, lds, stream, prof.ev_start, prof.ev_stop, 0, __VA_ARGS__);   \
        else hipLaunchKernelGGL(kernel, grid, block, lds, stream, __VA_ARGS__);                                               \
    } while (0)

#define CFM_CHECK_ARG(cond, ...)                                   \
    do {                                                           \
        if (!(cond)) return cfm_fail(CFM_ERR_ARG, __VA_ARGS__);    \
    } while (0)

static inline int cfm_launch_status(const char* what) {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return cfm_fail(CFM_ERR_LAUNCH, "%s: %s", what, hipGetErrorString(e));
    return CFM_OK;
}

static inline int cfm_elt_size(int dt) { return dt == CFM_F32 ? 4 : 2; }
static inline bool cfm_is16(int dt) { return dt == CFM_BF16 || dt == CFM_F16; }

// ---------------------------------------------------------------------------------------------
// device side: 16-bit operand types.  A wavefront is 64 lanes on gfx950; every constant below
// assumes that.
// ---------------------------------------------------------------------------------------------
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
// the same vectors where the address is only known to be dword aligned (rows of a [M, ld] matrix with ld % 4 == 2): global memory needs
// dword alignment only, so an access through these stays ONE global_load / global_store_dwordx4 / dwordx2
typedef float f32x4_a4 __attribute__((ext_vector_type(4), aligned(4)));
typedef float f32x2_a4 __attribute__((ext_vector_type(2), aligned(4)));
typedef unsigned int u32x2_a4 __attribute__((ext_vector_type(2), aligned(4)));
typedef __bf16 bf16x8_t __attribute__((ext_vector_type(8)));
typedef _Float16 f16x8_t __attribute__((ext_vector_type(8)));
typedef unsigned short u16;

struct BF16 {
    static constexpr int kId = CFM_BF16;
    typedef bf16x8_t frag;
    static __device__ __forceinline__ float to_f32(u16 v) { return __uint_as_float(((unsigned)v) << 16); }
    static __device__ __forceinline__ u16 from_f32(float f) {
        __bf16 b = (__bf16)f;  // v_cvt_pk_bf16_f32: RNE, NaN stays NaN
        return __builtin_bit_cast(u16, b);
    }
    static __device__ __forceinline__ f32x4 mfma(const u32x4& a, const u32x4& b, f32x4 c) {
        return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(frag, a), __builtin_bit_cast(frag, b), c,
                                                        0, 0, 0);
    }
};

struct F16 {
    static constexpr int kId = CFM_F16;
    typedef f16x8_t frag;
    static __device__ __forceinline__ float to_f32(u16 v) { return (float)__builtin_bit_cast(_Float16, v); }
    static __device__ __forceinline__ u16 from_f32(float f) {
        _Float16 h = (_Float16)f;
        return __builtin_bit_cast(u16, h);
    }
    static __device__ __forceinline__ f32x4 mfma(const u32x4& a, const u32x4& b, f32x4 c) {
        return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(frag, a), __builtin_bit_cast(frag, b), c,
                                                       0, 0, 0);
    }
};

template <typename HT>
__device__ __forceinline__ unsigned pack2(float lo, float hi) {
    return (unsigned)HT::from_f32(lo) | ((unsigned)HT::from_f32(hi) << 16);
}

// 8 consecutive f32 -> one 16-byte fragment of 16-bit values
template <typename HT>
__device__ __forceinline__ u32x4 pack8(const f32x4& a, const f32x4& b) {
    u32x4 r;
    r.x = pack2<HT>(a.x, a.y);
    r.y = pack2<HT>(a.z, a.w);
    r.z = pack2<HT>(b.x, b.y);
    r.w = pack2<HT>(b.z, b.w);
    return r;
}

// hi/lo bf16 split of 8 f32 values:  x ~= hi + lo  with ~16 mantissa bits
__device__ __forceinline__ void split8(const f32x4& a, const f32x4& b, u32x4& hi, u32x4& lo) {
    float v[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
    unsigned h[8], l[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        u16 hb = BF16::from_f32(v[i]);
        float r = v[i] - BF16::to_f32(hb);
        h[i] = hb;
        l[i] = BF16::from_f32(r);
    }
    hi = (u32x4){h[0] | (h[1] << 16), h[2] | (h[3] << 16), h[4] | (h[5] << 16), h[6] | (h[7] << 16)};
    lo = (u32x4){l[0] | (l[1] << 16), l[2] | (l[3] << 16), l[4] | (l[5] << 16), l[6] | (l[7] << 16)};
}

// v_exp_f32 + v_rcp_f32 (1 ulp): the IEEE divide sequence costs ~10 VALU ops per element in a GEMM epilogue
__device__ __forceinline__ float sigmoidf_(float x) { return __builtin_amdgcn_rcpf(1.0f + __expf(-x)); }
__device__ __forceinline__ float siluf_(float x) { return x * sigmoidf_(x); }
// ReLU of the GEMM epilogues: fmaxf alone returns its other argument for a NaN, which turns an overflowed activation into a clean zero
// (torch.relu keeps the NaN).  Every other value, -0.0 included, keeps the bits fmaxf gives.
__device__ __forceinline__ float reluf_(float x) { return x != x ? x : fmaxf(x, 0.f); }

// ---------------------------------------------------------------------------------------------
// dropout: a counter-based generator -- keep(seed, element index) is a pure function, so the backward regenerates the forward's
// mask instead of reading it from memory (nothing of the size of an activation is stored for dropout).  murmur3's 32-bit finaliser
// over (index * golden ratio) ^ seed: 2 multiplies, 3 shifts, 4 xors per element.  No bit-parity with torch's Philox stream (SURVEY 2.2:
// parity is defined at p = 0); statistics and forward/backward consistency are tested.
// ---------------------------------------------------------------------------------------------
struct CfmDrop {
    unsigned seed, thresh;   // keep iff hash >= thresh;  thresh = p * 2^32 (0: dropout off)
    float scale;             // 1 / (1 - p)
};
__device__ __forceinline__ unsigned cfm_hash32(unsigned seed, unsigned idx) {
    unsigned h = (idx * 0x9E3779B1u) ^ seed;
    h ^= h >> 16;
    h *= 0x85EBCA6Bu;
    h ^= h >> 13;
    h *= 0xC2B2AE35u;
    h ^= h >> 16;
    return h;
}
__device__ __forceinline__ float cfm_drop(const CfmDrop& d, unsigned idx, float v) {
    return cfm_hash32(d.seed, idx) >= d.thresh ? v * d.scale : 0.f;
}
static inline CfmDrop cfm_make_drop(float p, unsigned seed) {
    CfmDrop d;
    d.seed = seed;
    d.thresh = p <= 0.f ? 0u : (p >= 1.f ? 0xFFFFFFFFu : (unsigned)((double)p * 4294967296.0));
    d.scale = p <= 0.f ? 1.f : (p >= 1.f ? 0.f : 1.f / (1.f - p));
    return d;
}

// ---------------------------------------------------------------------------------------------
// typed loads / stores: element i of an array of T as f32 and back.  T is the element type tag `float`, `BF16` or `F16`;
// cfm_elt_t<dtype code> maps a CFM_F32 / CFM_BF16 / CFM_F16 template argument to it, cfm_dtype_of<T> maps back.
//   ld1 / st1    one value
//   ld4 / st4    four consecutive values in one 16-byte (f32) / 8-byte (16-bit) access: i % 4 == 0 and a base aligned to that size
//   st2          two consecutive values (the last column pair of a row with N % 4 == 2)
//   A4 = true    the address is only dword aligned (the *_a4 types above): still one instruction
// load_as_f32 / store_from_f32 / load4 / store4 / store2 are the same by RUN-TIME dtype (a branch per access: edges and epilogues;
// a loop of many loads wants the compile-time forms, see train.hip's depthwise-conv backward).
// ---------------------------------------------------------------------------------------------
template <int DT> struct cfm_elt;
template <> struct cfm_elt<CFM_F32> { typedef float type; };
template <> struct cfm_elt<CFM_BF16> { typedef BF16 type; };
template <> struct cfm_elt<CFM_F16> { typedef F16 type; };
template <int DT> using cfm_elt_t = typename cfm_elt<DT>::type;
template <typename T> inline constexpr int cfm_dtype_of = T::kId;
template <> inline constexpr int cfm_dtype_of<float> = CFM_F32;
template <typename T> constexpr bool cfm_is_f32 = cfm_dtype_of<T> == CFM_F32;

template <typename HT>
__device__ __forceinline__ f32x4 unpack4(u32x2 r) {  // 4 consecutive 16-bit values -> f32
    return (f32x4){HT::to_f32((u16)(r.x & 0xffffu)), HT::to_f32((u16)(r.x >> 16)), HT::to_f32((u16)(r.y & 0xffffu)), HT::to_f32((u16)(r.y >> 16))};
}

template <typename T>
__device__ __forceinline__ float ld1(const void* p, int64_t i) {
    if constexpr (cfm_is_f32<T>) return ((const float*)p)[i];
    else return T::to_f32(((const u16*)p)[i]);
}
template <typename T>
__device__ __forceinline__ void st1(void* p, int64_t i, float v) {
    if constexpr (cfm_is_f32<T>) ((float*)p)[i] = v;
    else ((u16*)p)[i] = T::from_f32(v);
}
template <typename T>
__device__ __forceinline__ f32x4 ld4(const void* p, int64_t i) {
    if constexpr (cfm_is_f32<T>) return *(const f32x4*)((const float*)p + i);
    else return unpack4<T>(*(const u32x2*)((const u16*)p + i));
}
template <typename T, bool A4 = false>
__device__ __forceinline__ void st4(void* p, int64_t i, const f32x4& v) {
    if constexpr (cfm_is_f32<T>) {
        if constexpr (A4) *(f32x4_a4*)((float*)p + i) = v;
        else *(f32x4*)((float*)p + i) = v;
    } else {
        const u32x2 w = {pack2<T>(v.x, v.y), pack2<T>(v.z, v.w)};
        if constexpr (A4) *(u32x2_a4*)((u16*)p + i) = w;
        else *(u32x2*)((u16*)p + i) = w;
    }
}
template <typename T, bool A4 = false>
__device__ __forceinline__ void st2(void* p, int64_t i, const f32x2& v) {
    if constexpr (cfm_is_f32<T>) {
        if constexpr (A4) *(f32x2_a4*)((float*)p + i) = v;
        else *(f32x2*)((float*)p + i) = v;
    } else {
        *(unsigned*)((u16*)p + i) = pack2<T>(v.x, v.y);
    }
}

__device__ __forceinline__ float load_as_f32(const void* p, int64_t i, int dt) {
    if (dt == CFM_F32) return ((const float*)p)[i];
    u16 v = ((const u16*)p)[i];
    return dt == CFM_BF16 ? BF16::to_f32(v) : F16::to_f32(v);
}
__device__ __forceinline__ void store_from_f32(void* p, int64_t i, int dt, float v) {
    if (dt == CFM_F32)
        ((float*)p)[i] = v;
    else
        ((u16*)p)[i] = dt == CFM_BF16 ? BF16::from_f32(v) : F16::from_f32(v);
}
__device__ __forceinline__ f32x4 load4(const void* p, int dt, int64_t i) {
    if (dt == CFM_F32) return ld4<float>(p, i);
    const u32x2 r = *(const u32x2*)((const u16*)p + i);  // one load for both 16-bit types
    return dt == CFM_BF16 ? unpack4<BF16>(r) : unpack4<F16>(r);
}
template <bool A4 = false>
__device__ __forceinline__ void store4(void* p, int dt, int64_t i, const f32x4& v) {
    if (dt == CFM_F32) st4<float, A4>(p, i, v);
    else if (dt == CFM_BF16) st4<BF16, A4>(p, i, v);
    else st4<F16, A4>(p, i, v);
}
template <bool A4 = false>
__device__ __forceinline__ void store2(void* p, int dt, int64_t i, const f32x2& v) {
    if (dt == CFM_F32) st2<float, A4>(p, i, v);
    else if (dt == CFM_BF16) st2<BF16, A4>(p, i, v);
    else st2<F16, A4>(p, i, v);
}

// host: calls f with a value of the element type of a run-time dtype, so that a generic lambda can name the type:
//   cfm_by_dtype(dt, [&](auto tag) { return launch<decltype(tag)>(...); })
// A kernel templated on the dtype code instead takes cfm_dtype_of<decltype(tag)>.  Callers check the code first; any other code selects float.
template <typename F>
static inline decltype(auto) cfm_by_dtype(int dt, F&& f) {
    if (dt == CFM_BF16) return f(BF16());
    if (dt == CFM_F16) return f(F16());
    return f(float());
}

// Sum over the 64 lanes of a wavefront, result in every lane (EXEC must be all ones).  Four DPP adds fold each row of 16
// lanes (quad swaps, then half-row and row mirrors), four v_readlane pick up the row totals: ~40 clk, against six dependent
// ds_bpermute round trips (~60 clk each) for the shuffle version -- LayerNorm calls this twice per row.
template <int CTRL>
__device__ __forceinline__ float dpp_mov_(float v) {
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xF, 0xF, true));
}
__device__ __forceinline__ float wave_sum(float v) {
    v += dpp_mov_<0xB1>(v);                                // quad_perm [1,0,3,2]
    v += dpp_mov_<0x4E>(v);                                // quad_perm [2,3,0,1]
    v += dpp_mov_<0x141>(v);                               // row_half_mirror
    v += dpp_mov_<0x140>(v);                               // row_mirror
    const int b = __builtin_bit_cast(int, v);
    const float r0 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(b, 0)), r1 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(b, 16));
    const float r2 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(b, 32)), r3 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(b, 48));
    return (r0 + r1) + (r2 + r3);
}

// Maximum over the 64 lanes, result in every lane: the six-step xor shuffle (the CTC / RNN-T row passes call it once per row)
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}

// log(exp(a) + exp(b)) on the hardware exp2/log2 units (v_exp_f32 / v_log_f32, ~1 ulp): the CTC and RNN-T recursions are serial chains of
// these, the library expf / log1pf sequences made CTC's 181 us at T' = 249.  1 + e is in (1, 2], where log needs no special care.
__device__ __forceinline__ float logaddexp_(float a, float b) {
    const float m = fmaxf(a, b);
    if (m == -INFINITY) return -INFINITY;
    return m + __logf(1.0f + __expf(-fabsf(a - b)));
}

// the last b with key[b] <= r (keys nondecreasing: a packed lattice's off / enc_row0 / pred_row0), -1 if none: <= 9 probes at B <= 512, all
// lanes of a wavefront at one address
__device__ __forceinline__ int last_le(const int64_t* __restrict__ key, int B, int64_t r) {
    if (key[0] > r) return -1;
    int lo = 0, hi = B - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (key[mid] <= r) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}
