// Device-side primitives shared by the gfx950 kernels: vector types, buffer descriptors, LDS-DMA and store instructions issued through
// inline asm, split-fp16 operand packing and wave reductions.  Each exists once, here; the kernels keep what is theirs alone.
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
// a wave-uniform double pinned to scalar registers (uniform fp64 values are computed on the VALU; left in VGPRs across a kernel's main
// loop they are spilled to scratch and reloaded -- a memory round trip -- in the phase that uses them)
__device__ __forceinline__ double uniform_f64(double x) {
    const unsigned long long u = __builtin_bit_cast(unsigned long long, x);
    unsigned lo, hi;                                 // (asm: the builtin is sunk to the use and the VGPR pair stays live)
    asm volatile("s_nop 1\n\tv_readfirstlane_b32 %0, %2\n\tv_readfirstlane_b32 %1, %3" : "=s"(lo), "=s"(hi) : "v"((unsigned)u), "v"((unsigned)(u >> 32)));
    return __builtin_bit_cast(double, ((unsigned long long)hi << 32) | lo);
}
