// Device-side primitives shared by the gfx950 kernels: vector types, buffer descriptors, LDS-DMA and store instructions issued through
// inline asm, split-fp16 operand packing, wave reductions and the label rule of the evaluator tail.  Each exists once, here; the kernels keep what is theirs alone.
#pragma once
#include "arseg_common.h"

typedef _Float16 h16x8 __attribute__((ext_vector_type(8)));
typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));

// Buffer offset of a masked-off lane in the CReFF kernels: the last 16-byte slot of the 4 GiB offset range, beyond num_records of every
// descriptor they build (a frame stays below 2 GiB) -- the load returns zeros, the store is dropped.  (The conv kernels mark such lanes
// with 0x80000000, which stays out of range after a tap or chunk offset is added to it: a different value, under their own names.)
constexpr unsigned OOB_TOP16 = 0xFFFFFFF0u;
constexpr float LOG2E = 1.44269504088896340736f;

__device__ __forceinline__ unsigned lds_addr(const void *p) { return (unsigned)(size_t)(__attribute__((address_space(3))) const void *)p; }

// Asynchronous memory traffic is issued through inline asm on purpose.  hipcc (ROCm 7.2) serialises the LDS-DMA builtins
// (a waterfall loop over the M0 base with an s_waitcnt vmcnt(0) in front of every load) and, on gfx9, drains every counter it
// knows about in front of each s_barrier -- so builtin stores would expose the full write latency at the next barrier.
// Loads: invisible to the compiler's s_waitcnt bookkeeping, so waited for explicitly (s_waitcnt vmcnt(0)) before the barrier that
// publishes their LDS image.  Stores: fire and forget (their data registers are read at issue).
__device__ __forceinline__ u32x4 make_rsrc(const void *base, unsigned bytes) {
    const unsigned long long a = (unsigned long long)base;      // wave uniform: pin the descriptor to SGPRs
    return u32x4{(unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)a), (unsigned)__builtin_amdgcn_readfirstlane((int)((unsigned)(a >> 32) & 0xffffu)),
                 (unsigned)__builtin_amdgcn_readfirstlane((int)bytes), 0x00020000u};
}
// LDS[lds_base + lane*16 .. +15] <- buffer[voff .. +15] (LDS-DMA: no staging registers)
__device__ __forceinline__ void dma16_buf(const u32x4 rsrc, unsigned voff, unsigned lds_base) {
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %1\n\ts_nop 0\n\tbuffer_load_dwordx4 %2, %3, 0 offen lds\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep) : "s"(lds_base), "v"(voff), "s"(rsrc) : "memory");
}
// LDS[lds_base + lane*16 .. +15] <- 16 bytes at g
__device__ __forceinline__ void dma16_glb(const void *g, unsigned lds_base) {
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %1\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %2, off\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep) : "s"(lds_base), "v"(g) : "memory");
}
__device__ __forceinline__ void store16_buf(const u32x4 v, const u32x4 rsrc, unsigned voff) {
    // s_nop: a VMEM store of more than 64 bits needs two wait states (gfx940+) before its data VGPRs may be overwritten (the
    // compiler pads this hazard for its own stores, not inside asm)
    asm volatile("buffer_store_dwordx4 %0, %1, %2, 0 offen\n\ts_nop 1" ::"v"(v), "v"(voff), "s"(rsrc) : "memory");
}
__device__ __forceinline__ void store4_buf(unsigned v, const u32x4 rsrc, unsigned voff) {
    asm volatile("buffer_store_dword %0, %1, %2, 0 offen" ::"v"(v), "v"(voff), "s"(rsrc) : "memory");
}

// fp32 x 4 -> split-fp16 halves (arseg_split_f16): {h01, h23}, {l01, l23}
__device__ __forceinline__ void split4(const f32x4 v, u32x2 &hi, u32x2 &lo) {
    unsigned h01, h23, l01, l23;
    arseg_split_f16(v, h01, h23, l01, l23);
    hi = u32x2{h01, h23}; lo = u32x2{l01, l23};
}
// two 4-half groups -> one 8-half MFMA operand
__device__ __forceinline__ h16x8 pack8(const u32x2 a, const u32x2 b) { return __builtin_bit_cast(h16x8, u32x4{a.x, a.y, b.x, b.y}); }
// ds_read_b64_tr_b16, the LDS transpose read: value records go to the matrix cores as an A operand without a transposed copy in LDS
__device__ __forceinline__ u32x2 lds_tr16(const unsigned char *p) {
    return __builtin_bit_cast(u32x2, __builtin_amdgcn_ds_read_tr16_b64_v4i16((s16x4 __attribute__((address_space(3))) *)p));
}
// a * b + c on packed pairs: v_pk_fma_f32 issues 2 FMAs in 4.2 cycles per wave, v_fmac_f32 one in 3.0 (measured on MI355X, 4 waves
// per SIMD) -- the depthwise convolutions are bound by exactly this
__device__ __forceinline__ f32x4 fma4(const f32x4 a, const f32x4 b, const f32x4 c) {
    const f32x2 lo = __builtin_elementwise_fma(__builtin_shufflevector(a, a, 0, 1), __builtin_shufflevector(b, b, 0, 1), __builtin_shufflevector(c, c, 0, 1));
    const f32x2 hi = __builtin_elementwise_fma(__builtin_shufflevector(a, a, 2, 3), __builtin_shufflevector(b, b, 2, 3), __builtin_shufflevector(c, c, 2, 3));
    return __builtin_shufflevector(lo, hi, 0, 1, 2, 3);
}
// reductions over the 4 DPP rows of a wave (lanes l, l^16, l^32, l^48) on the VALU: v_permlane16_swap exchanges the odd rows of its
// first operand with the even rows of the second, v_permlane32_swap the upper half of the first with the lower half of the second --
// fed two copies of x they return the pair (x, partner's x) in every lane.  (__shfl_xor is a ds_bpermute: an LDS round trip that all
// 16 lock-stepped waves of the workgroup wait for.)
__device__ __forceinline__ float rows_max(float x) {
    auto a = __builtin_amdgcn_permlane16_swap(__float_as_uint(x), __float_as_uint(x), false, false);
    x = fmaxf(__uint_as_float(a[0]), __uint_as_float(a[1]));
    auto b = __builtin_amdgcn_permlane32_swap(__float_as_uint(x), __float_as_uint(x), false, false);
    return fmaxf(__uint_as_float(b[0]), __uint_as_float(b[1]));
}
__device__ __forceinline__ float rows_sum(float x) {
    auto a = __builtin_amdgcn_permlane16_swap(__float_as_uint(x), __float_as_uint(x), false, false);
    x = __uint_as_float(a[0]) + __uint_as_float(a[1]);
    auto b = __builtin_amdgcn_permlane32_swap(__float_as_uint(x), __float_as_uint(x), false, false);
    return __uint_as_float(b[0]) + __uint_as_float(b[1]);
}
// The largest 64-bit key of a wave (simplify.hip, simplify_shared.hip: {value, tie-break} packed into one word).
template <int CTRL>
__device__ __forceinline__ unsigned long long dpp_max_u64(unsigned long long k) {
    const unsigned lo = (unsigned)__builtin_amdgcn_update_dpp(0, (int)(unsigned)k, CTRL, 0xf, 0xf, false);
    const unsigned hi = (unsigned)__builtin_amdgcn_update_dpp(0, (int)(unsigned)(k >> 32), CTRL, 0xf, 0xf, false);
    const unsigned long long o = ((unsigned long long)hi << 32) | lo;
    return o > k ? o : k;
}
// The largest key of the wave in every lane: within a row of 16 lanes by DPP (each step pairs every lane with one partner, so all lanes
// end with the row's maximum; quad_perm [1,0,3,2] and [2,3,0,1], row_half_mirror, row_mirror), across the rows by the lane swaps above
// (fed two copies they return {own, partner's} or the reverse -- the same order for both halves of the key).
__device__ __forceinline__ unsigned long long wave_max_u64(unsigned long long k) {
    k = dpp_max_u64<0xB1>(k);
    k = dpp_max_u64<0x4E>(k);
    k = dpp_max_u64<0x141>(k);
    k = dpp_max_u64<0x140>(k);
#pragma unroll
    for (int step = 0; step < 2; ++step) {
        const unsigned lo = (unsigned)k, hi = (unsigned)(k >> 32);
        unsigned l0, l1, h0, h1;
        if (step == 0) {
            auto a = __builtin_amdgcn_permlane16_swap(lo, lo, false, false); l0 = a[0]; l1 = a[1];
            auto b = __builtin_amdgcn_permlane16_swap(hi, hi, false, false); h0 = b[0]; h1 = b[1];
        } else {
            auto a = __builtin_amdgcn_permlane32_swap(lo, lo, false, false); l0 = a[0]; l1 = a[1];
            auto b = __builtin_amdgcn_permlane32_swap(hi, hi, false, false); h0 = b[0]; h1 = b[1];
        }
        const unsigned long long k0 = ((unsigned long long)h0 << 32) | l0, k1 = ((unsigned long long)h1 << 32) | l1;
        k = k0 > k1 ? k0 : k1;
    }
    // uniform from here on: what is decided from the key is decided on the scalar unit
    return ((unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(k >> 32)) << 32) | (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)k);
}

// ------------------------------------------------------------------ non-finite values: the activation of every conv epilogue, the max of the pools
// A NaN or an infinity that reaches an epilogue or a pool leaves it as torch's ReLU / PReLU / identity / max would leave it (DESIGN.md section 2,
// "Non-finite values").  fmaxf / v_max_f32 return the operand that is NOT NaN, so neither a ReLU nor a pool may be written with them: the
// forms below are compares and selects on uniform parameters (v_cmp + v_cndmask, no branch per element; the sigmoid keeps its uniform branch).
struct ArsegAct { float slope; bool relu, sigmoid; };
__device__ __forceinline__ ArsegAct arseg_act(int act, float slope) {
    return ArsegAct{act == ARSEG_ACT_PRELU ? slope : 1.0f, act == ARSEG_ACT_RELU, act == ARSEG_ACT_SIGMOID};      // (NONE / RELU: slope 1)
}
__device__ __forceinline__ float arseg_act_apply(float v, const ArsegAct a) {
    if (a.sigmoid) return 1.0f / (1.0f + __expf(-v));
    const float t = v >= 0.0f ? v : v * a.slope;          // a NaN fails the compare and stays NaN through the product
    return (a.relu && v < 0.0f) ? 0.0f : t;               // a NaN fails this one too: it is not clipped
}
// max that keeps a NaN: the first NaN met wins and stays (m NaN: both compares fail)
__device__ __forceinline__ float max_nan(float m, float f) { return (f > m || f != f) ? f : m; }
__device__ __forceinline__ f32x4 max_nan(const f32x4 m, const f32x4 f) {
    return f32x4{max_nan(m[0], f[0]), max_nan(m[1], f[1]), max_nan(m[2], f[2]), max_nan(m[3], f[3])};
}

// a wave-uniform double pinned to scalar registers (uniform fp64 values are computed on the VALU; left in VGPRs across a kernel's main
// loop they are spilled to scratch and reloaded -- a memory round trip -- in the phase that uses them)
__device__ __forceinline__ double uniform_f64(double x) {
    const unsigned long long u = __builtin_bit_cast(unsigned long long, x);
    unsigned lo, hi;                                 // (asm: the builtin is sunk to the use and the VGPR pair stays live)
    asm volatile("s_nop 1\n\tv_readfirstlane_b32 %0, %2\n\tv_readfirstlane_b32 %1, %3" : "=s"(lo), "=s"(hi) : "v"((unsigned)u), "v"((unsigned)(u >> 32)));
    return __builtin_bit_cast(double, ((unsigned long long)hi << 32) | lo);
}

// ------------------------------------------------------------------ NHWC element storage of the small layers (layers.hip, warp.hip)
// One lane moves a 16-byte channel vector: V = 4 fp32 or 8 fp16 / bf16 channels.  Arithmetic is fp32 in both storages; a 16-bit store rounds
// once, to nearest even.  The pyramid cells and bins take 4 channels per lane in both storages (ld4 / st4: 16 or 8 bytes).
template <int DT>           // enum arseg_dtype: ARSEG_DT_F16 | ARSEG_DT_BF16 (fp32: the specialisation below)
struct ArsegStore {
    static constexpr bool BF = DT == ARSEG_DT_BF16;
    using T = uint16_t;
    static constexpr int V = 8, SH = 3;          // channels per lane, log2 V
    static __device__ __forceinline__ void ld(const T *p, float (&f)[8]) {
        const u32x4 v = *reinterpret_cast<const u32x4 *>(p);
#pragma unroll
        for (int e = 0; e < 4; ++e) { f[2 * e] = arseg_h2f<BF>((uint16_t)(v[e] & 0xffffu)); f[2 * e + 1] = arseg_h2f<BF>((uint16_t)(v[e] >> 16)); }
    }
    static __device__ __forceinline__ void st(T *p, const float (&f)[8]) {
        u32x4 v;
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = (unsigned)arseg_f2h<BF>(f[2 * e]) | ((unsigned)arseg_f2h<BF>(f[2 * e + 1]) << 16);
        *reinterpret_cast<u32x4 *>(p) = v;
    }
    static __device__ __forceinline__ void cp(T *dst, const T *src) { *reinterpret_cast<u32x4 *>(dst) = *reinterpret_cast<const u32x4 *>(src); }     // bits, unconverted
    static __device__ __forceinline__ f32x4 ld4(const T *p) {
        const u32x2 v = *reinterpret_cast<const u32x2 *>(p);
        return f32x4{arseg_h2f<BF>((uint16_t)(v.x & 0xffffu)), arseg_h2f<BF>((uint16_t)(v.x >> 16)), arseg_h2f<BF>((uint16_t)(v.y & 0xffffu)),
                     arseg_h2f<BF>((uint16_t)(v.y >> 16))};
    }
    static __device__ __forceinline__ void st4(T *p, const f32x4 f) {
        *reinterpret_cast<u32x2 *>(p) = u32x2{arseg_f2h<BF>(f[0]) | ((unsigned)arseg_f2h<BF>(f[1]) << 16), arseg_f2h<BF>(f[2]) | ((unsigned)arseg_f2h<BF>(f[3]) << 16)};
    }
};
template <>
struct ArsegStore<ARSEG_DT_F32> {
    using T = float;
    static constexpr int V = 4, SH = 2;
    static __device__ __forceinline__ void ld(const T *p, float (&f)[4]) {
        const f32x4 v = *reinterpret_cast<const f32x4 *>(p);
        f[0] = v[0]; f[1] = v[1]; f[2] = v[2]; f[3] = v[3];
    }
    static __device__ __forceinline__ void st(T *p, const float (&f)[4]) { *reinterpret_cast<f32x4 *>(p) = f32x4{f[0], f[1], f[2], f[3]}; }
    static __device__ __forceinline__ void cp(T *dst, const T *src) { *reinterpret_cast<f32x4 *>(dst) = *reinterpret_cast<const f32x4 *>(src); }
    static __device__ __forceinline__ f32x4 ld4(const T *p) { return *reinterpret_cast<const f32x4 *>(p); }
    static __device__ __forceinline__ void st4(T *p, const f32x4 f) { *reinterpret_cast<f32x4 *>(p) = f; }
};

// ------------------------------------------------------------------ byte spans of the 8-bit output planes (egress.hip, confidence.hip)
typedef unsigned u32x2_a4 __attribute__((ext_vector_type(2), aligned(4)));

// NB consecutive bytes <-> NB values, with the widest accesses the address allows: 8 / 4 bytes on a 4-byte aligned address, 2 bytes on an
// even one, single bytes otherwise.  Exactly the NB bytes are touched: nothing past a row's last sample is read or written.
template <int NB>
__device__ __forceinline__ void span_load(const uint8_t *g, unsigned (&v)[NB]) {
    const unsigned al = (unsigned)reinterpret_cast<uintptr_t>(g);
    if (NB % 4 == 0 && !(al & 3u)) {
#pragma unroll
        for (int q = 0; q < NB / 4; q += 2) {
            unsigned x0, x1 = 0;
            if (q + 1 < NB / 4) { const u32x2_a4 x = *reinterpret_cast<const u32x2_a4 *>(g + 4 * q); x0 = x.x; x1 = x.y; }
            else x0 = *reinterpret_cast<const unsigned *>(g + 4 * q);
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                v[4 * q + b] = (x0 >> (8 * b)) & 0xffu;
                if (q + 1 < NB / 4) v[(4 * q + 4 < NB ? 4 * q + 4 : 0) + b] = (x1 >> (8 * b)) & 0xffu;
            }
        }
    } else if (NB % 2 == 0 && !(al & 1u)) {
#pragma unroll
        for (int q = 0; q < NB / 2; ++q) {
            const unsigned x = *reinterpret_cast<const uint16_t *>(g + 2 * q);
            v[2 * q] = x & 0xffu; v[2 * q + 1] = x >> 8;
        }
    } else {
#pragma unroll
        for (int q = 0; q < NB; ++q) v[q] = g[q];
    }
}
template <int NB>
__device__ __forceinline__ void span_store(uint8_t *g, const unsigned (&v)[NB]) {
    const unsigned al = (unsigned)reinterpret_cast<uintptr_t>(g);
    if (NB % 4 == 0 && !(al & 3u)) {
#pragma unroll
        for (int q = 0; q < NB / 4; q += 2) {
            const unsigned x0 = v[4 * q] | (v[4 * q + 1] << 8) | (v[4 * q + 2] << 16) | (v[4 * q + 3] << 24);
            if (q + 1 < NB / 4) {
                const int o = 4 * q + 4 < NB ? 4 * q + 4 : 0;
                const unsigned x1 = v[o] | (v[o + 1] << 8) | (v[o + 2] << 16) | (v[o + 3] << 24);
                *reinterpret_cast<u32x2_a4 *>(g + 4 * q) = u32x2_a4{x0, x1};
            } else {
                *reinterpret_cast<unsigned *>(g + 4 * q) = x0;
            }
        }
    } else if (NB % 2 == 0 && !(al & 1u)) {
#pragma unroll
        for (int q = 0; q < NB / 2; ++q) *reinterpret_cast<uint16_t *>(g + 2 * q) = (uint16_t)(v[2 * q] | (v[2 * q + 1] << 8));
    } else {
#pragma unroll
        for (int q = 0; q < NB; ++q) g[q] = (uint8_t)v[q];
    }
}

// ------------------------------------------------------------------ the label rule of the evaluator tail and of the egress kernels
// logits NCHW [N,n_cls,h,w] -> the class of one output pixel after the bilinear resize to H x W.  THE one definition: the evaluator tail
// (layers.hip: argmax_pixel / argmax_run, ungrouped and grouped) and the egress kernels (egress.hip) call these, so their labels agree bit for
// bit.  torch.argmax semantics: the first maximum wins, a NaN counts as the maximum (the first NaN wins).  Branch free (the short-circuit
// form compiles to a divergent branch per pixel and class).
//
// Accumulators.  With an accumulator type other than ArsegNoAcc (the default: the tail and egress, nothing is instantiated for it) the rule
// hands every blended class value v_k to *acc, together with the running best before it and the rule's decision: acc->step(r, v, best,
// take) for pixel r of the thread, in class order, BEFORE best / bi are updated.  The accumulator only looks on: the operations that decide
// k* are the same with or without it.

struct ArsegNoAcc {};
template <class Acc> constexpr bool arseg_has_acc = !__is_same(Acc, ArsegNoAcc);

// The softmax of a pixel's blended class values in one pass over the classes (include/arseg_hip.h, arseg_segment_confidence_fwd): running
// maximum m (the rule's own best), Z = sum_k exp(v_k - m) rescaled whenever the maximum moves -- one exp per class either way, since
// exp(-|v - m|) is the rescale factor when v is the new maximum and the new term when it is not -- and the largest value over k != k*.
// A NaN value makes Z NaN for good; infinite maxima are caught in code().  S pixels per thread, no per-class array.
template <int S>
struct ArsegSoftmaxAcc {
    float m[S], Z[S], sec[S];
    __device__ __forceinline__ ArsegSoftmaxAcc() {
#pragma unroll
        for (int r = 0; r < S; ++r) { m[r] = -INFINITY; Z[r] = 0.f; sec[r] = -INFINITY; }
    }
    __device__ __forceinline__ void step(int r, float v, float best, bool take) {
        const float e = v == best ? 1.f : __expf(-fabsf(v - best));          // (equal infinities: their difference would be NaN)
        Z[r] = take ? fmaf(Z[r], e, 1.f) : Z[r] + e;
        sec[r] = take ? best : fmaxf(sec[r], v);
        m[r] = take ? v : m[r];
    }
    // the 8-bit code of pixel r: q = floor(255 c + 0.5), c = p1 = 1 / Z or the margin p1 - p2 = (1 - exp(v_second - m)) / Z; a NaN c
    // (NaN value, +inf maximum, all -inf) -> 0
    __device__ __forceinline__ unsigned code(int r, bool margin) const {
        float c = __builtin_amdgcn_rcpf(Z[r]);
        if (margin) c *= 1.f - __expf(sec[r] - m[r]);
        c = fabsf(m[r]) == INFINITY ? NAN : c;
        const float q = floorf(fmaf(255.f, c, 0.5f));
        return q == q ? (unsigned)fminf(q, 255.f) : 0u;
    }
};

// One output pixel (ox, oy) of frame n on the per-pixel route: `same` (h == H && w == W) reads the logit itself, otherwise the four bilinear
// taps of arseg_src_index (sy / sx = arseg_resize_scale of the two axes, either align_corners).
template <class Acc = ArsegNoAcc>
__device__ __forceinline__ int arseg_label_pixel(const float *__restrict__ logits, int n, int oy, int ox, int n_cls, int h, int w, int align, bool same,
                                                 float sy, float sx, Acc *acc = nullptr) {
    int y0 = oy, y1 = oy, x0 = ox, x1 = ox; float ly = 0.f, lx = 0.f;
    if (!same) {
        arseg_src_index(sy, oy, align != 0, h, y0, y1, ly);
        arseg_src_index(sx, ox, align != 0, w, x0, x1, lx);
        ly = fminf(fmaxf(ly, 0.f), 1.f); lx = fminf(fmaxf(lx, 0.f), 1.f);
    }
    float best = -INFINITY; int bi = 0; bool best_nan = false;
    for (int k = 0; k < n_cls; ++k) {
        const float *b = logits + ((size_t)n * n_cls + k) * h * w;
        float v;
        if (same) v = b[(size_t)oy * w + ox];
        else v = (1.f - ly) * ((1.f - lx) * b[(size_t)y0 * w + x0] + lx * b[(size_t)y0 * w + x1]) +
                 ly * ((1.f - lx) * b[(size_t)y1 * w + x0] + lx * b[(size_t)y1 * w + x1]);
        const bool isn = v != v, take = !best_nan & ((v > best) | isn);
        if constexpr (arseg_has_acc<Acc>) acc->step(0, v, best, take);
        best = take ? v : best; bi = take ? k : bi; best_nan = best_nan | (take & isn);
    }
    return bi;
}

// One run of an exact x S bilinear upsample with align_corners=False, S a power of two: the S output pixels x = S*j + S/2 .. S*j + 3S/2 - 1
// of output row oy all interpolate between the low-resolution columns j and j+1 (src = j + (r + 0.5) / S), j = -1 .. w-1 (the first and the
// last run reach S/2 pixels off the frame: those entries of bi are computed on clamped columns and belong to no pixel).  The 4 taps are
// loaded once per class and the S pixels evaluated from registers -- 4 loads per class and run instead of 4 S.  Same taps and weights as
// arseg_label_pixel (arseg_src_index, sc = 1 / S); the blend is regrouped (see below), so a label may differ from the per-pixel form where
// the top two logits are within fp32 rounding of each other: a caller picks the route by shape, never per pixel.
template <int S, class Acc = ArsegNoAcc>
__device__ __forceinline__ void arseg_label_run(const float *__restrict__ logits, float sc, int n, int oy, int j, int n_cls, int h, int w, int (&bi)[S],
                                                Acc *acc = nullptr) {
    const int W = S * w;
    int y0, y1; float ly;
    arseg_src_index(sc, oy, false, h, y0, y1, ly);
    ly = fminf(fmaxf(ly, 0.f), 1.f);
    const int x0 = max(j, 0), x1 = min(x0 + 1, w - 1), xs = S * j + S / 2;       // first output column of the run (may be negative for j = -1)
    float lx[S];
#pragma unroll
    for (int r = 0; r < S; ++r) {
        int a, b;
        arseg_src_index(sc, min(max(xs + r, 0), W - 1), false, w, a, b, lx[r]);
        lx[r] = fminf(fmaxf(lx[r], 0.f), 1.f);
    }
    float best[S]; bool bn[S];
#pragma unroll
    for (int r = 0; r < S; ++r) { best[r] = -INFINITY; bi[r] = 0; bn[r] = false; }
    const float *b = logits + (size_t)n * n_cls * h * w;
    const size_t o00 = (size_t)y0 * w + x0, o01 = (size_t)y0 * w + x1, o10 = (size_t)y1 * w + x0, o11 = (size_t)y1 * w + x1, cs = (size_t)h * w;
    for (int k0 = 0; k0 < n_cls; k0 += 4) {          // four classes' taps in flight (a class at a time is bound by the load latency)
        float t[4][4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const float *bk = b + (size_t)min(k0 + u, n_cls - 1) * cs;
            if (x1 > x0) {          // the two taps of a row are neighbours: one 8-byte load (the kernel is bound by the number of load instructions)
                // (a 4-byte aligned pair type: the address is odd in floats for every other run -- gfx950 global loads take any dword
                // address, and the reduced alignment makes that a defined access instead of a misaligned float2)
                typedef float f32x2_a4 __attribute__((ext_vector_type(2), aligned(4)));
                const f32x2_a4 a01 = *reinterpret_cast<const f32x2_a4 *>(bk + o00), a11 = *reinterpret_cast<const f32x2_a4 *>(bk + o10);
                t[u][0] = a01.x; t[u][1] = a01.y; t[u][2] = a11.x; t[u][3] = a11.y;
            } else {
                t[u][0] = bk[o00]; t[u][1] = bk[o01]; t[u][2] = bk[o10]; t[u][3] = bk[o11];
            }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            if (k0 + u >= n_cls) break;
            // the bilinear blend is linear in lx along the run: v(r) = a + lx[r] * b -- one FMA per pixel and class (the expanded form,
            // 6 operations, made this kernel VALU bound); same value up to fp32 rounding of the regrouped sum
            const float a = (1.f - ly) * t[u][0] + ly * t[u][2];
            const float b = (1.f - ly) * (t[u][1] - t[u][0]) + ly * (t[u][3] - t[u][2]);
#pragma unroll
            for (int r = 0; r < S; ++r) {
                const float v = fmaf(lx[r], b, a);
                const bool isn = v != v, take = !bn[r] & ((v > best[r]) | isn);
                if constexpr (arseg_has_acc<Acc>) acc->step(r, v, best[r], take);
                best[r] = take ? v : best[r];
                bi[r] = take ? k0 + u : bi[r];
                bn[r] = bn[r] | (take & isn);
            }
        }
    }
}
