// conv2d as an implicit GEMM on the gfx950 fp32 matrix cores (v_mfma_f32_32x32x2_f32).
//
// Replaces the nn.Conv2d / BatchNorm2d / ReLU / PReLU stacks of the reference backbones
// (model/extractors.py:35-66,108-158; model/pspnet.py:14-46; model/bisenet.py:31-60,162-399).
//
//   GEMM view      M = N*Ho*Wo output pixels, N = Cout, K = R*S*Cin (k = (r*S+s)*Cin + ci)
//   A (activations) NHWC: the K axis is channel-contiguous, so a 16-byte vector never straddles a
//                   filter tap; im2col is done by address arithmetic in the loader (zero fill for
//                   padding), nothing is materialised.
//   B (weights)     packed [Cout][Kpad] (K contiguous) by arseg_pack_conv_weight_host.
//   Block           256 threads = 4 waves in a 2x2 grid, block tile BM x BN, K step 32.
//   LDS             A and B tiles as [row][32+4] floats (the +4 pad makes the ds_read_b128 of a
//                   32-row fragment conflict free), double buffered; one barrier per K step.
//   Global -> LDS   register staged (16-byte loads issued before the MFMAs of the current step,
//                   written to the other buffer after them) because im2col needs predication.
//   MFMA fragments  lane l = (i = l&31, h = l>>5) reads 4 consecutive k (one ds_read_b128) for row i
//                   at k-offset 8*k8+4*h; the 4 values feed 4 MFMAs.  The MFMA's two k slots (h=0,1)
//                   therefore see k = 8*k8+kk and 8*k8+4+kk -- a permutation of K applied
//                   identically to A and B, which leaves the product unchanged.
//   Epilogue        y = acc*scale[co] + bias[co] (+ residual) -> none/ReLU/PReLU/sigmoid, NHWC store
//                   (32 consecutive channels per half wave = 128-byte segments).
//   Split-K         gridDim.z slices of the K loop write fp32 partials to the workspace; a second
//                   kernel sums them in slice order (deterministic) and applies the epilogue.
//   XCD mapping     the linear block id is remapped so that each of the 8 XCDs (private L2) gets a
//                   contiguous run of tiles that share activation rows.
//
// Two arithmetic back ends share the loader / tiling / epilogue (template parameter MATH):
//   ARSEG_MATH_F32    v_mfma_f32_32x32x2_f32 on fp32 operands (157 TF peak, the fp32 VALU rate).
//   ARSEG_MATH_F16X3  every fp32 operand x is represented as hi + lo, two fp16 numbers (hi = x truncated to 11 significant
//                     bits, lo = fp16(x - hi): 22 bits together), and a.b is evaluated as a_hi.b_hi + a_hi.b_lo + a_lo.b_hi
//                     with three v_mfma_f32_32x32x16_f16 (fp32 accumulate; the dropped lo.lo term is 2^-22 relative).
//                     16x the MFMA rate for 3x the instructions.  Weights are split (and scaled per output channel by a
//                     power of two so that lo stays a normal fp16) once at pack time; activations stay fp32 in HBM and
//                     are split on their way into LDS, whose row layout becomes [32 hi halves | 32 lo halves | pad].
#include "arseg_device.h"
#include "conv_plans.h"
#include <type_traits>
#include <cmath>
#include <cstring>

namespace {

typedef __fp16 fp16x2 __attribute__((ext_vector_type(2)));

constexpr int KALIGN = 32;       // packed K is padded to a multiple of this (one f16x3 weight tile)

struct ConvParams {
    const float *in, *w, *scale, *bias, *res;
    float *out, *ws;
    int N, H, W, Cin, in_ld, log2Cin;
    int Ho, Wo, Cout, out_ld, res_ld;
    int R, S, stride, pad, dil;
    int K, Kpad, M;
    int act;
    float slope;
    int ktiles, ktiles_per_split, nsplit, N_batch;
    int tiles_m, tiles_n;
    int inv_S;                       // 65536/S + 1: r = (rs*inv_S) >> 16 without a division
    int up2;                         // patch kernel: `in` is the low-resolution tensor [N, H/2, W/2, in_ld], convolved after a x2 bilinear upsample
    unsigned *range_flag;            // F16X3: sticky status word (or null): bit 0 is set when an A operand exceeds range_limit in magnitude
    float range_limit;
    unsigned in_bytes, w_bytes;      // extents for the buffer descriptors
    unsigned out_bytes, res_bytes;   // extent of one problem's output / residual if below 2 GiB (branch-free epilogue through buffer stores), else 0
    long long in_bs, w_bs, out_bs;   // batched GEMM mode (blockIdx.y = batch index): element strides between problems
};

// fp32 x4 -> (hi, lo) fp16 x4 each (arseg_common.h: hi = RTZ fp16 of x, lo = fp16 of x - hi; representable range |x| <= 131008)
__device__ __forceinline__ void split_f16x3(const f32x4 v, uint2 &hi, uint2 &lo) {
    unsigned h01, h23, l01, l23;
    arseg_split_f16(v, h01, h23, l01, l23);
    hi = uint2{h01, h23}; lo = uint2{l01, l23};
}

// Operand range watch of the split-fp16 back end (arseg_conv_desc.range_flag): the running maximum |a| of the activations a thread splits.
// Only the workgroups of output-channel tile 0 watch, so every activation is examined once per conv (per tap), not once per N tile; inf / NaN operands are not flagged (they propagate into the output by themselves), the silent case -- finite values the hi/lo
// pair can only clamp -- is.
__device__ __forceinline__ void range_watch(float &vmax, const f32x4 v) {
    vmax = fmaxf(fmaxf(vmax, fmaxf(fabsf(v[0]), fabsf(v[1]))), fmaxf(fabsf(v[2]), fabsf(v[3])));
}
__device__ __forceinline__ void range_report(const ConvParams &p, bool watch, float vmax) {
    if (watch && vmax > p.range_limit) atomicOr(p.range_flag, 1u);
}

// Branch-free epilogue of one accumulator element: scale, bias, residual, activation, store.  The bounds tests become out-of-range
// buffer offsets (loads return 0, stores are dropped), the activation is selects on uniform parameters (arseg_act_apply) -- the per-element
// `continue` / `if (res)` / switch form compiled to ~3 branches and a 64-bit multiply per element (a fifth of a short-K tile's time).
template <bool RES>
__device__ __forceinline__ void epi_store(float v, float sc, float bi, const ArsegAct a, const __amdgpu_buffer_rsrc_t o_rsrc,
                                          const __amdgpu_buffer_rsrc_t r_rsrc, unsigned o_off, unsigned r_off) {
    v = v * sc + bi;
    if constexpr (RES) v += __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r_rsrc, r_off, 0, 0));
    __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, arseg_act_apply(v, a)), o_rsrc, o_off, 0, 0);
}

template <int BM, int BN, int BK, int NBUF, int MATH, int NWM = 2, int NWN = 2>      // NWM x NWN waves, wave tile BM/NWM x BN/NWN
__global__ __launch_bounds__(64 * NWM * NWN) void conv_igemm_kernel(const ConvParams p) {
    constexpr int LDS_LD = BK + 4;                // floats per LDS row (the +4 pad keeps the ds_read_b128 fragments conflict free)
    constexpr int CPR = BK / 4;                   // 16-byte chunks per row of a K step
    constexpr int NT = 64 * NWM * NWN;
    constexpr int RPP = NT / CPR;                 // rows staged per pass of the workgroup
    constexpr int TM = BM / (32 * NWM), TN = BN / (32 * NWN);     // 32x32 MFMA tiles per wave
    constexpr int RA = BM / RPP, RB = BN / RPP;   // rows staged per thread
    constexpr unsigned OOB = 0x80000000u;         // beyond num_records of either buffer: the load returns zeros
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float *As = smem;                              // [NBUF][BM][LDS_LD]
    float *Bs = smem + NBUF * BM * LDS_LD;         // [NBUF][BN][LDS_LD]

    // XCD-aware (bijective) remap of the linear block id: XCD x gets a contiguous chunk of tiles.
    const int nblk = p.tiles_m * p.tiles_n;
    int bid = blockIdx.x;
    {
        const int q = nblk >> 3, r = nblk & 7, xcd = bid & 7, idx = bid >> 3;
        bid = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
    }
    const int tile_m = bid / p.tiles_n, tile_n = bid - tile_m * p.tiles_n;   // n fastest: neighbours share A rows
    const int m0 = tile_m * BM, n0 = tile_n * BN;
    const bool watch = MATH == ARSEG_MATH_F16X3 && p.range_flag != nullptr && tile_n == 0;      // (every split-K slice: each covers its own part of K)
    float vmax = 0.f;
    float *__restrict__ gout = p.out + (size_t)blockIdx.y * p.out_bs;
    // operands through buffer descriptors: a load whose offset is out of range returns zeros, which is how image padding,
    // tile tails and K padding are produced without branches
    const __amdgpu_buffer_rsrc_t a_rsrc =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(p.in + (size_t)blockIdx.y * p.in_bs), 0, (int)p.in_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t b_rsrc =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(p.w + (size_t)blockIdx.y * p.w_bs), 0, (int)p.w_bytes, 0x00020000);

    const int tid = threadIdx.x;
    const int chunk = tid & (CPR - 1);  // which 16-byte vector of the BK-float K step
    const int row0 = tid / CPR;

    // decode the output pixels this thread stages (constant over the K loop)
    int iy0[RA], ix0[RA], rowoff[RA];
#pragma unroll
    for (int i = 0; i < RA; ++i) {
        const int m = m0 + row0 + RPP * i;
        if (m < p.M) {
            const int hw = p.Ho * p.Wo;
            const int n = m / hw, rem = m - n * hw;
            const int oy = rem / p.Wo, ox = rem - oy * p.Wo;
            iy0[i] = oy * p.stride - p.pad;
            ix0[i] = ox * p.stride - p.pad;
            rowoff[i] = ((n * p.H + iy0[i]) * p.W + ix0[i]) * p.in_ld * 4 + chunk * 16;     // bytes; may be negative
        } else {
            iy0[i] = -(1 << 28); ix0[i] = 0; rowoff[i] = 0;     // every tap fails the bounds test
        }
    }
    unsigned woff[RB];
#pragma unroll
    for (int i = 0; i < RB; ++i) {
        const int n = n0 + row0 + RPP * i;
        woff[i] = n < p.Cout ? (unsigned)(n * p.Kpad + chunk * 4) * 4u : OOB;
    }

    const int kt_begin = blockIdx.z * p.ktiles_per_split;
    const int kt_end = min(kt_begin + p.ktiles_per_split, p.ktiles);
    const bool tap_uniform = p.R * p.S > 1 && (p.Cin & (BK - 1)) == 0;    // a whole K step lies inside one filter tap

    struct Regs { u32x4 a[RA], b[RB]; };
    auto load_tile = [&](int kt, Regs &rg) {
        int dy = 0, dx = 0, koff;         // koff: byte offset of this lane's 4 channels relative to rowoff (without the tap)
        bool kvalid;
        if (p.R * p.S == 1) {
            const int k = kt * BK + chunk * 4;
            koff = kt * BK * 4; kvalid = k < p.K;
        } else if (tap_uniform) {          // scalar tap decode
            const int rs = (kt * BK) >> p.log2Cin;
            const int r = (rs * p.inv_S) >> 16, s = rs - r * p.S;
            dy = r * p.dil; dx = s * p.dil;
            koff = ((kt * BK) & (p.Cin - 1)) * 4; kvalid = rs < p.R * p.S;
        } else {                           // narrow Cin (the 3-channel stems): taps differ between lanes
            const int k = kt * BK + chunk * 4;
            const int rs = k >> p.log2Cin;
            const int r = (rs * p.inv_S) >> 16, s = rs - r * p.S;
            dy = r * p.dil; dx = s * p.dil;
            koff = (k & (p.Cin - 1)) * 4 - chunk * 16; kvalid = rs < p.R * p.S;
        }
        const int tapoff = (dy * p.W + dx) * p.in_ld * 4 + koff;
#pragma unroll
        for (int i = 0; i < RA; ++i) {
            const int iy = iy0[i] + dy, ix = ix0[i] + dx;
            const bool ok = kvalid && (unsigned)iy < (unsigned)p.H && (unsigned)ix < (unsigned)p.W;
            rg.a[i] = __builtin_amdgcn_raw_buffer_load_b128(a_rsrc, ok ? (unsigned)(rowoff[i] + tapoff) : OOB, 0, 0);
        }
#pragma unroll
        for (int i = 0; i < RB; ++i) rg.b[i] = __builtin_amdgcn_raw_buffer_load_b128(b_rsrc, woff[i] + (unsigned)(kt * BK * 4), 0, 0);
    };
    auto store_tile = [&](int buf, const Regs &rg) {
        float *a = As + buf * BM * LDS_LD, *b = Bs + buf * BN * LDS_LD;
#pragma unroll
        for (int i = 0; i < RA; ++i) {
            float *row = a + (row0 + RPP * i) * LDS_LD;
            if (MATH == ARSEG_MATH_F16X3) {             // per 32-k tile: halves [0,32) hi, [32,64) lo
                uint2 hi, lo;
                split_f16x3(__builtin_bit_cast(f32x4, rg.a[i]), hi, lo);
                if (watch) range_watch(vmax, __builtin_bit_cast(f32x4, rg.a[i]));
                *reinterpret_cast<uint2 *>(row + (chunk >> 3) * 32 + (chunk & 7) * 2) = hi;
                *reinterpret_cast<uint2 *>(row + (chunk >> 3) * 32 + 16 + (chunk & 7) * 2) = lo;
            } else if (MATH == ARSEG_MATH_F16) {        // plain fp16 operands (round to nearest), the lo halves stay unused
                const f32x4 v = __builtin_bit_cast(f32x4, rg.a[i]);
                typedef _Float16 h16x4 __attribute__((ext_vector_type(4)));
                const h16x4 hv = {(_Float16)v[0], (_Float16)v[1], (_Float16)v[2], (_Float16)v[3]};
                *reinterpret_cast<h16x4 *>(row + (chunk >> 3) * 32 + (chunk & 7) * 2) = hv;
            } else {
                *reinterpret_cast<u32x4 *>(row + chunk * 4) = rg.a[i];
            }
        }
#pragma unroll
        for (int i = 0; i < RB; ++i) *reinterpret_cast<u32x4 *>(b + (row0 + RPP * i) * LDS_LD + chunk * 4) = rg.b[i];
    };

    const int wave = tid >> 6, lane = tid & 63;
    const int wm = wave / NWN, wn = wave % NWN;
    const int li = lane & 31, lh = lane >> 5;

    // f16x3 with a single MFMA tile per wave: a second accumulator for the two cross terms breaks the dependent chain
    constexpr bool DUAL = MATH == ARSEG_MATH_F16X3 && TM * TN == 1;
    f32x16 acc[TM][TN], acc2[1];
#pragma unroll
    for (int a = 0; a < TM; ++a)
#pragma unroll
        for (int b = 0; b < TN; ++b)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.0f;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc2[0][r] = 0.0f;

    auto compute = [&](int cur) {
        if (MATH == ARSEG_MATH_F16) {                  // one fp16 MFMA per product: the hi halves only
            const float *ah = As + cur * BM * LDS_LD + (wm * (BM / NWM) + li) * LDS_LD + 4 * lh;
            const float *bh = Bs + cur * BN * LDS_LD + (wn * (BN / NWN) + li) * LDS_LD + 4 * lh;
#pragma unroll
            for (int ks = 0; ks < BK / 16; ++ks) {
                const int ko = (ks >> 1) * 32 + (ks & 1) * 8;
                h16x8 fa[TM], fb[TN];
#pragma unroll
                for (int t = 0; t < TM; ++t) fa[t] = *reinterpret_cast<const h16x8 *>(ah + t * 32 * LDS_LD + ko);
#pragma unroll
                for (int t = 0; t < TN; ++t) fb[t] = *reinterpret_cast<const h16x8 *>(bh + t * 32 * LDS_LD + ko);
#pragma unroll
                for (int tm = 0; tm < TM; ++tm)
#pragma unroll
                    for (int tn = 0; tn < TN; ++tn) acc[tm][tn] = __builtin_amdgcn_mfma_f32_32x32x16_f16(fa[tm], fb[tn], acc[tm][tn], 0, 0, 0);
            }
        } else if (MATH == ARSEG_MATH_F16X3) {
            // lane (li, lh) holds k = 16*ks + 8*lh + 0..7 of row li: one ds_read_b128 per operand and precision half
            const float *ah = As + cur * BM * LDS_LD + (wm * (BM / NWM) + li) * LDS_LD + 4 * lh;
            const float *bh = Bs + cur * BN * LDS_LD + (wn * (BN / NWN) + li) * LDS_LD + 4 * lh;
#pragma unroll
            for (int ks = 0; ks < BK / 16; ++ks) {
                const int ko = (ks >> 1) * 32 + (ks & 1) * 8;      // float offset of this 16-k slice inside the row
                h16x8 fah[TM], fal[TM], fbh[TN], fbl[TN];
#pragma unroll
                for (int t = 0; t < TM; ++t) {
                    fah[t] = *reinterpret_cast<const h16x8 *>(ah + t * 32 * LDS_LD + ko);
                    fal[t] = *reinterpret_cast<const h16x8 *>(ah + t * 32 * LDS_LD + 16 + ko);
                }
#pragma unroll
                for (int t = 0; t < TN; ++t) {
                    fbh[t] = *reinterpret_cast<const h16x8 *>(bh + t * 32 * LDS_LD + ko);
                    fbl[t] = *reinterpret_cast<const h16x8 *>(bh + t * 32 * LDS_LD + 16 + ko);
                }
                if (DUAL) {
                    acc2[0] = __builtin_amdgcn_mfma_f32_32x32x16_f16(fal[0], fbh[0], acc2[0], 0, 0, 0);
                    acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x16_f16(fah[0], fbh[0], acc[0][0], 0, 0, 0);
                    acc2[0] = __builtin_amdgcn_mfma_f32_32x32x16_f16(fah[0], fbl[0], acc2[0], 0, 0, 0);
                } else {
#pragma unroll
                    for (int tm = 0; tm < TM; ++tm)
#pragma unroll
                        for (int tn = 0; tn < TN; ++tn)
                            acc[tm][tn] = __builtin_amdgcn_mfma_f32_32x32x16_f16(fal[tm], fbh[tn], acc[tm][tn], 0, 0, 0);
#pragma unroll
                    for (int tm = 0; tm < TM; ++tm)
#pragma unroll
                        for (int tn = 0; tn < TN; ++tn)
                            acc[tm][tn] = __builtin_amdgcn_mfma_f32_32x32x16_f16(fah[tm], fbl[tn], acc[tm][tn], 0, 0, 0);
#pragma unroll
                    for (int tm = 0; tm < TM; ++tm)
#pragma unroll
                        for (int tn = 0; tn < TN; ++tn)
                            acc[tm][tn] = __builtin_amdgcn_mfma_f32_32x32x16_f16(fah[tm], fbh[tn], acc[tm][tn], 0, 0, 0);
                }
            }
        } else {
            const float *a = As + cur * BM * LDS_LD + (wm * (BM / NWM) + li) * LDS_LD + 4 * lh;
            const float *b = Bs + cur * BN * LDS_LD + (wn * (BN / NWN) + li) * LDS_LD + 4 * lh;
#pragma unroll
        for (int k8 = 0; k8 < BK / 8; ++k8) {
            f32x4 fa[TM], fb[TN];
#pragma unroll
            for (int t = 0; t < TM; ++t) fa[t] = *reinterpret_cast<const f32x4 *>(a + t * 32 * LDS_LD + k8 * 8);
#pragma unroll
            for (int t = 0; t < TN; ++t) fb[t] = *reinterpret_cast<const f32x4 *>(b + t * 32 * LDS_LD + k8 * 8);
#pragma unroll
            for (int kk = 0; kk < 4; ++kk)
#pragma unroll
                for (int tm = 0; tm < TM; ++tm)
#pragma unroll
                    for (int tn = 0; tn < TN; ++tn)
                        acc[tm][tn] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[tm][kk], fb[tn][kk], acc[tm][tn], 0, 0, 0);
        }
        }
    };

    Regs r0, r1;
    if (kt_begin < kt_end) {
        load_tile(kt_begin, r0);
        store_tile(0, r0);
    }
    if (NBUF == 2) {
        // LDS double buffer + two register stages: the loads of K step kt+2 are issued before the MFMAs of step kt and are
        // written to LDS a whole step later, so they have two compute phases to land; one barrier per step.
        if (kt_begin + 1 < kt_end) load_tile(kt_begin + 1, r0);
        __syncthreads();
        int cur = 0;
        auto step = [&](int kt, Regs &ld, Regs &st) {
            if (kt + 2 < kt_end) load_tile(kt + 2, ld);
            compute(cur);
            if (kt + 1 < kt_end) store_tile(cur ^ 1, st);
            __syncthreads();
            cur ^= 1;
        };
        for (int kt = kt_begin; kt < kt_end; kt += 2) {
            step(kt, r1, r0);
            if (kt + 1 < kt_end) step(kt + 1, r0, r1);
        }
    } else {
        // single LDS buffer: half the LDS per block (more blocks per CU), two barriers per step
        __syncthreads();
        for (int kt = kt_begin; kt < kt_end; ++kt) {
            const bool more = kt + 1 < kt_end;
            if (more) load_tile(kt + 1, r0);
            compute(0);
            __syncthreads();
            if (more) store_tile(0, r0);
            __syncthreads();
        }
    }

    if (DUAL) acc[0][0] += acc2[0];

    range_report(p, watch, vmax);
    // epilogue: C/D layout of the 32x32 MFMA: col = lane&31, row = (r&3) + 8*(r>>2) + 4*(lane>>5)
    if (p.nsplit == 1 && p.out_bytes) {
        constexpr unsigned OOBS = 0x80000000u;
        const __amdgpu_buffer_rsrc_t o_rsrc = __builtin_amdgcn_make_buffer_rsrc(gout, 0, (int)p.out_bytes, 0x00020000);
        const __amdgpu_buffer_rsrc_t r_rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(p.res ? p.res : gout), 0, (int)p.res_bytes, 0x00020000);
        const ArsegAct ea = arseg_act(p.act, p.slope);
        auto run = [&](auto res_tag) {
            constexpr bool RES = decltype(res_tag)::value;
#pragma unroll
            for (int tm = 0; tm < TM; ++tm)
#pragma unroll
                for (int tn = 0; tn < TN; ++tn) {
                    const int n = n0 + wn * (BN / NWN) + tn * 32 + li, nc = min(n, p.Cout - 1);
                    const float sc = p.scale ? p.scale[nc] : 1.0f, bi = p.bias ? p.bias[nc] : 0.0f;
                    const int mb = m0 + wm * (BM / NWM) + tm * 32 + 4 * lh;
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int m = mb + (r & 3) + 8 * (r >> 2);
                        const bool ok = n < p.Cout && m < p.M;
                        epi_store<RES>(acc[tm][tn][r], sc, bi, ea, o_rsrc, r_rsrc, ok ? ((unsigned)m * (unsigned)p.out_ld + (unsigned)n) * 4u : OOBS,
                                       ok ? ((unsigned)m * (unsigned)p.res_ld + (unsigned)n) * 4u : OOBS);
                    }
                }
        };
        if (p.res) run(std::true_type{}); else run(std::false_type{});
        return;
    }
#pragma unroll
    for (int tm = 0; tm < TM; ++tm)
#pragma unroll
        for (int tn = 0; tn < TN; ++tn) {
            const int n = n0 + wn * (BN / NWN) + tn * 32 + li;
            if (n >= p.Cout) continue;
            float sc = 1.0f, bi = 0.0f;
            if (p.nsplit == 1) {
                if (p.scale) sc = p.scale[n];
                if (p.bias) bi = p.bias[n];
            }
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int m = m0 + wm * (BM / NWM) + tm * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
                if (m >= p.M) continue;
                float v = acc[tm][tn][r];
                if (p.nsplit == 1) {
                    v = v * sc + bi;
                    if (p.res) v += p.res[(size_t)m * p.res_ld + n];
                    gout[(size_t)m * p.out_ld + n] = arseg_act_apply(v, arseg_act(p.act, p.slope));
                } else {
                    p.ws[((size_t)blockIdx.z * p.M + m) * p.Cout + n] = v;
                }
            }
        }
}

// ---------------------------------------------------------------------------------------------------------------------
// 3x3 stride-1 convolution with the input patch of a tile resident in LDS (f16x3 only; tile_cfg 13 / 14).
// The implicit-GEMM kernel above re-stages (and re-splits) the activation slice of every filter tap: nine global loads,
// nine hi/lo splits and nine LDS writes per input element.  Here a workgroup owns TH x TW = 128 output pixels of one image
// and, per 32-channel chunk, stages the (TH+2d) x (TW+2d) input patch once, split into [32 hi | 32 lo] halves per pixel;
// the nine taps are A-fragment *address offsets* into that patch.  K order = (chunk, tap), i.e. K tile kt = tap*Cin/32 +
// chunk of the ordinary packed weights.  Per tap only the weight tile is streamed (double buffered, one barrier per tap);
// the next chunk's patch is prefetched into registers under the nine taps of the current one.
//
// UP2: the conv input is the x2 bilinear (align_corners=False) upsample of `p.in` (PSPUpsample, model/pspnet.py:43-46), never
// materialised.  The patch starts at the odd coordinate ty0 - 1: it is a grid of 2 x 2 blocks (rows 2i+1, 2i+2) and each block is a
// blend of exactly ONE 2 x 2 quad of low-resolution pixels (rows i, i+1: weights .75/.25 and .25/.75) -- one 16-byte load per
// upsampled 16-byte piece, a quarter of the bytes of the materialised tensor, and no resize kernel (its 0.25/0.75 arithmetic and
// edge cases, layers.hip upsample2x_nhwc_kernel, are reproduced).  Dilation 1.
template <int BN, int WM, bool UP2>      // WM wave rows of 64 output pixels each: BM = 64*WM pixels, 2*WM waves
__global__ __launch_bounds__(128 * WM, (BN == 64 ? (WM == 2 ? 3 : 4) : 2)) void conv3x3_patch_kernel(const ConvParams p, int TW, int log2TW) {
    constexpr int ROWB = 144;                          // bytes per LDS row: 32 hi + 32 lo halves + pad (conflict-free b128 reads)
    constexpr int NT = 128 * WM, BM = 64 * WM;
    constexpr int TN = BN / 64, TM = 2, RB = (BN * 8 + NT - 1) / NT, RPB = NT / 8;
    constexpr unsigned OOB = 0x80000000u;
    constexpr int MAXI = UP2 ? 1 : (WM == 2 ? 9 : 7);  // patch items (pixel, 16-byte piece) per thread: <= 288 / 448 pixels
    constexpr int MAXU = UP2 ? (WM == 2 ? 3 : 2) : 1;  // UP2: items (2 x 2 block, 16-byte piece) per thread: <= 72 / 112 blocks
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int TH = BM >> log2TW, d = p.dil, PW = TW + 2 * d, PH = TH + 2 * d, npx = PW * PH;
    unsigned char *Ps = reinterpret_cast<unsigned char *>(smem);               // [npx][ROWB]
    unsigned char *Bs = Ps + ((npx * ROWB + 255) & ~255);                        // [2][BN][ROWB]

    // tile decode (n fastest over output-channel tiles, then x, y, image), XCD-contiguous like the GEMM kernel
    const int tiles_x = (p.Wo + TW - 1) >> log2TW, tiles_y = (p.Ho + TH - 1) / TH;
    const int nblk = p.tiles_m * p.tiles_n;
    int bid = blockIdx.x;
    {
        const int q = nblk >> 3, r = nblk & 7, xcd = bid & 7, idx = bid >> 3;
        bid = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
    }
    const int tile_m = bid / p.tiles_n, tile_n = bid - tile_m * p.tiles_n;
    const int img = tile_m / (tiles_x * tiles_y), trem = tile_m - img * (tiles_x * tiles_y);
    const int ty0 = (trem / tiles_x) * TH, tx0 = (trem - (trem / tiles_x) * tiles_x) * TW, n0 = tile_n * BN;
    const bool watch = p.range_flag != nullptr && tile_n == 0;
    float vmax = 0.f;

    const __amdgpu_buffer_rsrc_t a_rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(p.in), 0, (int)p.in_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t b_rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(p.w), 0, (int)p.w_bytes, 0x00020000);
    const int tid = threadIdx.x;

    // patch items of this thread: item i = (pixel i/8, piece i%8); global byte offset without the chunk term, or OOB
    unsigned poff[MAXI];
    if constexpr (!UP2) {
#pragma unroll
        for (int it = 0; it < MAXI; ++it) {
            const int i = tid + it * NT, px = i >> 3, py = px / PW, pxx = px - py * PW;
            const int gy = ty0 - d + py, gx = tx0 - d + pxx;
            const bool ok = px < npx && (unsigned)gy < (unsigned)p.H && (unsigned)gx < (unsigned)p.W;
            poff[it] = ok ? (unsigned)((((img * p.H + gy) * p.W + gx) * p.in_ld) * 4 + (i & 7) * 16) : OOB;
        }
    }
    // UP2 items: block (by, bx) of the patch = upsampled rows 2*iy+1, 2*iy+2 and columns 2*ix+1, 2*ix+2; quad = low-res rows
    // clamp(iy), clamp(iy+1) x columns clamp(ix), clamp(ix+1).  uflag: bit 0/1 row 0/1 inside the image, bit 2/3 column 0/1 inside,
    // bit 4: iy < 0 (row 1 is the image's first row = the low-res row itself), bit 5: ix < 0.
    // TWIN: conv_up2_c64.hip (load_quads / stage) restates the quad addressing, uflag and the blend of store_patch below, operation for
    // operation, so that tile_cfg 23 rounds as these plans do.  Change one and change the other (tests/test_gpu_up2_c64.py compares them).
    unsigned uoff[MAXU][4];
    int upx[MAXU], uflag[MAXU];
    if constexpr (UP2) {
        const int h = p.H >> 1, w = p.W >> 1, BWc = PW >> 1, nblkp = BWc * (PH >> 1);
#pragma unroll
        for (int it = 0; it < MAXU; ++it) {
            const int i = tid + it * NT, b = i >> 3, by = b / BWc, bx = b - by * BWc;
            const int iy = (ty0 >> 1) - 1 + by, ix = (tx0 >> 1) - 1 + bx;
            const int ya = min(max(iy, 0), h - 1), yb = min(max(iy + 1, 0), h - 1), xa = min(max(ix, 0), w - 1), xb = min(max(ix + 1, 0), w - 1);
            const unsigned base = (unsigned)(img * h) * (unsigned)w, q16 = (i & 7) * 16;
            const bool live = b < nblkp;
            uoff[it][0] = live ? ((base + ya * w + xa) * p.in_ld) * 4u + q16 : OOB;
            uoff[it][1] = live ? ((base + ya * w + xb) * p.in_ld) * 4u + q16 : OOB;
            uoff[it][2] = live ? ((base + yb * w + xa) * p.in_ld) * 4u + q16 : OOB;
            uoff[it][3] = live ? ((base + yb * w + xb) * p.in_ld) * 4u + q16 : OOB;
            upx[it] = live ? (2 * by * PW + 2 * bx) : -1;
            uflag[it] = ((iy >= 0 && 2 * iy + 1 < p.H) ? 1 : 0) | ((2 * iy + 2 < p.H) ? 2 : 0) | ((ix >= 0 && 2 * ix + 1 < p.W) ? 4 : 0) |
                        ((2 * ix + 2 < p.W) ? 8 : 0) | (iy < 0 ? 16 : 0) | (ix < 0 ? 32 : 0);
        }
    }
    const int chunk = tid & 7, row0 = tid >> 3;
    unsigned woff[RB];
#pragma unroll
    for (int i = 0; i < RB; ++i) {
        const int n = n0 + row0 + RPB * i;
        woff[i] = (n < p.Cout && row0 + RPB * i < BN) ? (unsigned)(n * p.Kpad + chunk * 4) * 4u : OOB;
    }
    const int nchunk = p.Cin >> 5;

    struct BRegs { u32x4 v[RB]; };
    u32x4 rp[MAXI];
    u32x4 rq[MAXU][4];
    auto load_patch = [&](int ck) {
        if constexpr (UP2) {
#pragma unroll
            for (int it = 0; it < MAXU; ++it)
#pragma unroll
                for (int k = 0; k < 4; ++k) rq[it][k] = __builtin_amdgcn_raw_buffer_load_b128(a_rsrc, uoff[it][k] + (unsigned)(ck * 128), 0, 0);
        } else {
#pragma unroll
            for (int it = 0; it < MAXI; ++it) rp[it] = __builtin_amdgcn_raw_buffer_load_b128(a_rsrc, poff[it] + (unsigned)(ck * 128), 0, 0);
        }
    };
    auto put_px = [&](int px, int piece, const f32x4 v) {
        uint2 hi, lo;
        split_f16x3(v, hi, lo);
        if (watch) range_watch(vmax, v);
        unsigned char *row = Ps + px * ROWB + piece * 8;
        *reinterpret_cast<uint2 *>(row) = hi;
        *reinterpret_cast<uint2 *>(row + 64) = lo;
    };
    auto store_patch = [&]() {
        if constexpr (UP2) {
#pragma unroll
            for (int it = 0; it < MAXU; ++it) {
                if (upx[it] < 0) continue;
                const int piece = (tid + it * NT) & 7, f = uflag[it];
                const f32x4 q00 = __builtin_bit_cast(f32x4, rq[it][0]), q01 = __builtin_bit_cast(f32x4, rq[it][1]);
                const f32x4 q10 = __builtin_bit_cast(f32x4, rq[it][2]), q11 = __builtin_bit_cast(f32x4, rq[it][3]);
                // vertical blend at the two low-res columns (row 2iy+1: .75 / .25; row 2iy+2: .25 / .75, or the row itself at the top edge)
                const f32x4 r0a = 0.75f * q00 + 0.25f * q10, r0b = 0.75f * q01 + 0.25f * q11;
                const f32x4 r1a = (f & 16) ? q10 : 0.25f * q00 + 0.75f * q10, r1b = (f & 16) ? q11 : 0.25f * q01 + 0.75f * q11;
                const f32x4 z = {0.f, 0.f, 0.f, 0.f};
                const f32x4 o00 = 0.75f * r0a + 0.25f * r0b, o01 = (f & 32) ? r0b : 0.25f * r0a + 0.75f * r0b;
                const f32x4 o10 = 0.75f * r1a + 0.25f * r1b, o11 = (f & 32) ? r1b : 0.25f * r1a + 0.75f * r1b;
                put_px(upx[it], piece, (f & 5) == 5 ? o00 : z);
                put_px(upx[it] + 1, piece, (f & 9) == 9 ? o01 : z);
                put_px(upx[it] + PW, piece, (f & 6) == 6 ? o10 : z);
                put_px(upx[it] + PW + 1, piece, (f & 10) == 10 ? o11 : z);
            }
        } else {
#pragma unroll
            for (int it = 0; it < MAXI; ++it) {
                const int i = tid + it * NT, px = i >> 3;
                if (px < npx) put_px(px, i & 7, __builtin_bit_cast(f32x4, rp[it]));
            }
        }
    };
    auto load_b = [&](int ck, int tap, BRegs &r) {
        const unsigned kt = (unsigned)(tap * nchunk + ck) * 128u;
#pragma unroll
        for (int i = 0; i < RB; ++i) r.v[i] = __builtin_amdgcn_raw_buffer_load_b128(b_rsrc, woff[i] + kt, 0, 0);
    };
    auto store_b = [&](int buf, const BRegs &r) {
#pragma unroll
        for (int i = 0; i < RB; ++i)
            if (row0 + RPB * i < BN) *reinterpret_cast<u32x4 *>(Bs + (buf * BN + row0 + RPB * i) * ROWB + chunk * 16) = r.v[i];
    };

    const int wave = tid >> 6, lane = tid & 63, wm = wave >> 1, wn = wave & 1, li = lane & 31, lh = lane >> 5;
    // A rows of this lane: output pixel m = wm*64 + tm*32 + li of the tile (wm < WM) -> patch pixel (ty, tx) (+ tap offset later)
    int arow[TM];
#pragma unroll
    for (int tm = 0; tm < TM; ++tm) {
        const int m = wm * 64 + tm * 32 + li, ty = m >> log2TW, tx = m & (TW - 1);
        arow[tm] = (ty * PW + tx) * ROWB + lh * 16;
    }
    f32x16 acc[TM][TN];
#pragma unroll
    for (int a = 0; a < TM; ++a)
#pragma unroll
        for (int b = 0; b < TN; ++b)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.0f;

    // K steps s = (chunk ck, tap): s = 9*ck + tap.  Weight tiles are requested two steps ahead (two register stages, LDS
    // double buffer): a step of 12-24 MFMAs is shorter than the L2 latency.
    const int nsteps = nchunk * 9;
    BRegs r0, r1;
    load_patch(0);
    load_b(0, 0, r0);
    store_patch();
    store_b(0, r0);
    if (nsteps > 1) load_b(0, 1, r0);
    __syncthreads();
    int cur = 0, ck = 0, tap = 0;              // of the step being computed
    int ck2 = 0, tap2 = 2;                     // of the step two ahead (valid while s + 2 < nsteps; 9 taps >= 3)
    auto step = [&](int s_, BRegs &ld, BRegs &st) {
        if (s_ + 2 < nsteps) load_b(ck2, tap2, ld);
        if (tap == 0 && ck + 1 < nchunk) load_patch(ck + 1);
        const int r3 = (tap * 11) >> 5, s3 = tap - r3 * 3;                 // tap = 3*r3 + s3
        const int toff = (r3 * d * PW + s3 * d) * ROWB;
        const unsigned char *bh = Bs + (cur * BN + wn * (BN / 2) + li) * ROWB + lh * 16;
        // all fragments of the tap first (one exposed LDS latency per tap), then the MFMAs back to back
        h16x8 fah[2][TM], fal[2][TM], fbh[2][TN], fbl[2][TN];
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
#pragma unroll
            for (int t = 0; t < TM; ++t) {
                fah[ks][t] = *reinterpret_cast<const h16x8 *>(Ps + arow[t] + toff + ks * 32);
                fal[ks][t] = *reinterpret_cast<const h16x8 *>(Ps + arow[t] + toff + 64 + ks * 32);
            }
#pragma unroll
            for (int t = 0; t < TN; ++t) {
                fbh[ks][t] = *reinterpret_cast<const h16x8 *>(bh + t * 32 * ROWB + ks * 32);
                fbl[ks][t] = *reinterpret_cast<const h16x8 *>(bh + t * 32 * ROWB + 64 + ks * 32);
            }
        }
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
#pragma unroll
            for (int tm = 0; tm < TM; ++tm)
#pragma unroll
                for (int tn = 0; tn < TN; ++tn) acc[tm][tn] = __builtin_amdgcn_mfma_f32_32x32x16_f16(fal[ks][tm], fbh[ks][tn], acc[tm][tn], 0, 0, 0);
#pragma unroll
            for (int tm = 0; tm < TM; ++tm)
#pragma unroll
                for (int tn = 0; tn < TN; ++tn) acc[tm][tn] = __builtin_amdgcn_mfma_f32_32x32x16_f16(fah[ks][tm], fbl[ks][tn], acc[tm][tn], 0, 0, 0);
#pragma unroll
            for (int tm = 0; tm < TM; ++tm)
#pragma unroll
                for (int tn = 0; tn < TN; ++tn) acc[tm][tn] = __builtin_amdgcn_mfma_f32_32x32x16_f16(fah[ks][tm], fbh[ks][tn], acc[tm][tn], 0, 0, 0);
        }
        if (s_ + 1 < nsteps) store_b(cur ^ 1, st);
        __syncthreads();
        cur ^= 1;
        if (tap == 8 && ck + 1 < nchunk) {     // everybody is past the last tap of this chunk: the patch may be replaced
            store_patch();
            __syncthreads();
        }
        if (++tap == 9) { tap = 0; ++ck; }
        if (++tap2 == 9) { tap2 = 0; ++ck2; }
    };
#pragma unroll 1
    for (int s_ = 0; s_ < nsteps; s_ += 2) {
        step(s_, r1, r0);
        if (s_ + 1 < nsteps) step(s_ + 1, r0, r1);
    }

    range_report(p, watch, vmax);
    // epilogue: C/D layout of the 32x32 MFMA: col = lane&31, row = (r&3) + 8*(r>>2) + 4*(lane>>5)
    if (p.out_bytes) {
        constexpr unsigned OOBS = 0x80000000u;
        const __amdgpu_buffer_rsrc_t o_rsrc = __builtin_amdgcn_make_buffer_rsrc(p.out, 0, (int)p.out_bytes, 0x00020000);
        const __amdgpu_buffer_rsrc_t r_rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(p.res ? p.res : p.out), 0, (int)p.res_bytes, 0x00020000);
        const ArsegAct ea = arseg_act(p.act, p.slope);
        auto run = [&](auto res_tag) {
            constexpr bool RES = decltype(res_tag)::value;
#pragma unroll
            for (int tm = 0; tm < TM; ++tm)
#pragma unroll
                for (int tn = 0; tn < TN; ++tn) {
                    const int n = n0 + wn * (BN / 2) + tn * 32 + li, nc = min(n, p.Cout - 1);
                    const float sc = p.scale ? p.scale[nc] : 1.0f, bi = p.bias ? p.bias[nc] : 0.0f;
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int ml = wm * 64 + tm * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
                        const int oy = ty0 + (ml >> log2TW), ox = tx0 + (ml & (TW - 1));
                        const bool ok = n < p.Cout && oy < p.Ho && ox < p.Wo;
                        const unsigned m = ((unsigned)img * (unsigned)p.Ho + (unsigned)oy) * (unsigned)p.Wo + (unsigned)ox;
                        epi_store<RES>(acc[tm][tn][r], sc, bi, ea, o_rsrc, r_rsrc, ok ? (m * (unsigned)p.out_ld + (unsigned)n) * 4u : OOBS,
                                       ok ? (m * (unsigned)p.res_ld + (unsigned)n) * 4u : OOBS);
                    }
                }
        };
        if (p.res) run(std::true_type{}); else run(std::false_type{});
        return;
    }
#pragma unroll
    for (int tm = 0; tm < TM; ++tm)
#pragma unroll
        for (int tn = 0; tn < TN; ++tn) {
            const int n = n0 + wn * (BN / 2) + tn * 32 + li;
            if (n >= p.Cout) continue;
            const float sc = p.scale ? p.scale[n] : 1.0f, bi = p.bias ? p.bias[n] : 0.0f;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int ml = wm * 64 + tm * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
                const int oy = ty0 + (ml >> log2TW), ox = tx0 + (ml & (TW - 1));
                if (oy >= p.Ho || ox >= p.Wo) continue;
                const size_t m = ((size_t)img * p.Ho + oy) * p.Wo + ox;
                float v = acc[tm][tn][r] * sc + bi;
                if (p.res) v += p.res[m * p.res_ld + n];
                p.out[m * p.out_ld + n] = arseg_act_apply(v, arseg_act(p.act, p.slope));
            }
        }
}

// sums the split-K partials in slice order and applies the epilogue; 4 channels per thread
__global__ __launch_bounds__(256) void conv_splitk_reduce_kernel(const ConvParams p) {
    const int c4 = p.Cout >> 2;
    const long long total = (long long)p.M * c4;
    for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long long)gridDim.x * blockDim.x) {
        const int m = (int)(idx / c4), n = (int)(idx - (long long)m * c4) * 4;
        f32x4 v = *reinterpret_cast<const f32x4 *>(p.ws + (size_t)m * p.Cout + n);
        for (int z = 1; z < p.nsplit; ++z) v += *reinterpret_cast<const f32x4 *>(p.ws + ((size_t)z * p.M + m) * p.Cout + n);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float x = v[j] * (p.scale ? p.scale[n + j] : 1.0f) + (p.bias ? p.bias[n + j] : 0.0f);
            if (p.res) x += p.res[(size_t)m * p.res_ld + n + j];
            p.out[(size_t)m * p.out_ld + n + j] = arseg_act_apply(x, arseg_act(p.act, p.slope));
        }
    }
}

int make_plan(const arseg_conv_desc *d, ConvPlan *pl) {
    if (int e = conv_geometry(d, pl)) return e;
    pl->Kpad = arseg_packed_k(d->Cin, d->R, d->S);
    const ConvPlanRow *row = conv_plan_row(kConvPlans32, d->tile_cfg);
    if (!row) return ARSEG_EINVAL;
    pl->take(*row);
    pl->patch_tw = pl->patch_th = 0; pl->ktiles = (pl->Kpad + pl->bk - 1) / pl->bk; pl->ktiles_per_split = pl->ktiles; pl->split(1, d->Cout);
    if (row->kind == ARSEG_PLAN_UP2_C64) {
        if (!d->upsample2x) return ARSEG_EINVAL;                  // the id exists for convs on an upsampled input only
        if (!conv_up2_c64_shape(d) || (d->out_ld & 3) || conv_up2_c64_in_bytes(d) >= (1ll << 31) || conv_up2_c64_out_bytes(d) >= (1ll << 31)) return ARSEG_EUNSUPPORTED;
        pl->tiles_m = d->N * arseg_cdiv(pl->Ho, 8) * arseg_cdiv(pl->Wo, 16); pl->tiles_n = 1;
        return ARSEG_OK;
    }
    if (row->f16x3_only && d->math != ARSEG_MATH_F16X3) return ARSEG_EUNSUPPORTED;
    if (d->upsample2x && !row->fuses_up2) return ARSEG_EUNSUPPORTED;
    if (!conv_fits_32bit(d, pl->Kpad)) return ARSEG_EUNSUPPORTED;
    if (row->kind == ARSEG_PLAN_PATCH) return conv_patch_plan(d, *row, 31, pl);
    // Tile / split-K choice, fitted to a brute-force sweep of this model family's layer shapes on MI355X
    // (scratch sweep recorded in DESIGN.md): aim for ~512 workgroups (2 per CU); take the largest tile that gets
    // there with a split-K factor that still leaves >= 8 K-steps per slice; shallow GEMMs (< 64 K-steps) are best
    // served by 64x64 tiles.
    const long long M = pl->M;
    const int target = d->batch > 1 ? (512 + d->batch - 1) / d->batch : 512;
    const int max_split = pl->ktiles / 8 > 0 ? (pl->ktiles / 8 > 16 ? 16 : pl->ktiles / 8) : 1;
    int nsplit = 1;
    if (row->kind == ARSEG_PLAN_AUTO) {      // (its K step and single LDS buffer -- more blocks per CU, measured faster -- are the row's)
        const int order_deep[4] = {1, 4, 2, 3}, order_shallow[4] = {3, 3, 3, 3};
        const int *order = pl->ktiles >= 64 ? order_deep : order_shallow;
        pl->bm = pl->bn = 64;
        bool found = false;
        for (int t = 0; t < 4 && !found; ++t) {
            const int tb_m = kConvPlans32[order[t]].bm, tb_n = kConvPlans32[order[t]].bn;
            if (tb_n == 128 && d->Cout <= 64) continue;
            if (tb_m == 128 && M <= 64) continue;
            const long long tiles = (long long)arseg_cdiv(M, tb_m) * arseg_cdiv(d->Cout, tb_n), need = (target + tiles - 1) / tiles;
            if (need <= max_split || order[t] == 3) {
                pl->bm = tb_m; pl->bn = tb_n;
                nsplit = (int)(need < 1 ? 1 : (need > max_split ? max_split : need));
                found = true;
            }
        }
    }
    pl->tiles_m = arseg_cdiv(M, pl->bm); pl->tiles_n = arseg_cdiv(d->Cout, pl->bn);
    if (d->split_k > 0) nsplit = d->split_k;
    else if (row->kind != ARSEG_PLAN_AUTO) {
        const long long tiles = (long long)pl->tiles_m * pl->tiles_n, need = (target + tiles - 1) / tiles;
        nsplit = (int)(need < 1 ? 1 : (need > max_split ? max_split : need));
    }
    if (nsplit > pl->ktiles) nsplit = pl->ktiles;
    if (nsplit > 1 && (d->Cout & 3)) nsplit = 1;   // the reduce kernel is 4-wide
    if (d->batch > 1) nsplit = 1;                   // batched GEMMs bring their own parallelism
    pl->ktiles_per_split = arseg_cdiv(pl->ktiles, nsplit);
    pl->split(arseg_cdiv(pl->ktiles, pl->ktiles_per_split), d->Cout);
    return ARSEG_OK;
}

template <int BM, int BN, int BK, int NBUF, int MATH, int NWM = 2, int NWN = 2>
int launch(const ConvParams &p, const ConvPlan &pl, hipStream_t st) {
    const size_t smem = (size_t)NBUF * (BM + BN) * (BK + 4) * sizeof(float);
    static ArsegSmemAttr attr;
    if (int e = arseg_allow_smem(attr, reinterpret_cast<const void *>(conv_igemm_kernel<BM, BN, BK, NBUF, MATH, NWM, NWN>), smem)) return e;
    dim3 grid(pl.tiles_m * pl.tiles_n, p.in_bs || p.w_bs || p.out_bs ? p.N_batch : 1, pl.nsplit);
    hipLaunchKernelGGL((conv_igemm_kernel<BM, BN, BK, NBUF, MATH, NWM, NWN>), grid, dim3(64 * NWM * NWN), smem, st, p);
    return arseg_launch_status();
}

template <int BK, int NBUF, int MATH>
int launch_tile(const ConvParams &p, const ConvPlan &pl, hipStream_t hs) {
    if (pl.bm == 128 && pl.bn == 128) return launch<128, 128, BK, NBUF, MATH>(p, pl, hs);
    if (pl.bm == 128 && pl.bn == 64) return launch<128, 64, BK, NBUF, MATH>(p, pl, hs);
    if (pl.bm == 64 && pl.bn == 128) return launch<64, 128, BK, NBUF, MATH>(p, pl, hs);
    return launch<64, 64, BK, NBUF, MATH>(p, pl, hs);
}

template <int BN, int WM, bool UP2>
int launch_patch_up(const ConvParams &p, const ConvPlan &pl, int dil, hipStream_t st) {
    const int tw = pl.patch_tw, npx = (pl.patch_th + 2 * dil) * (tw + 2 * dil);
    const size_t smem = (size_t)((npx * 144 + 255) & ~255) + (size_t)2 * BN * 144;
    static ArsegSmemAttr attr;
    if (int e = arseg_allow_smem(attr, reinterpret_cast<const void *>(conv3x3_patch_kernel<BN, WM, UP2>), smem)) return e;
    int l2 = 0;
    while ((1 << l2) < tw) ++l2;
    hipLaunchKernelGGL((conv3x3_patch_kernel<BN, WM, UP2>), dim3(pl.tiles_m * pl.tiles_n), dim3(128 * WM), smem, st, p, tw, l2);
    return arseg_launch_status();
}
template <int BN, int WM>
int launch_patch(const ConvParams &p, const ConvPlan &pl, int dil, hipStream_t st) {
    return p.up2 ? launch_patch_up<BN, WM, true>(p, pl, dil, st) : launch_patch_up<BN, WM, false>(p, pl, dil, st);
}

template <int MATH>
int launch_math(const ConvParams &p, const ConvPlan &pl, hipStream_t hs) {
    if (pl.kind == ARSEG_PLAN_TILE_WIDE) {      // (f16x3 only: make_plan)
        if (pl.bm == 256 && pl.bn == 128) return launch<256, 128, 32, 1, ARSEG_MATH_F16X3, 4, 2>(p, pl, hs);
        if (pl.bm == 128 && pl.bn == 256) return launch<128, 256, 32, 1, ARSEG_MATH_F16X3, 2, 4>(p, pl, hs);
        return launch<256, 256, 32, 1, ARSEG_MATH_F16X3, 4, 4>(p, pl, hs);
    }
    if (pl.bk == 64) return launch_tile<64, 1, MATH>(p, pl, hs);
    return pl.nbuf == 1 ? launch_tile<32, 1, MATH>(p, pl, hs) : launch_tile<32, 2, MATH>(p, pl, hs);
}

}  // namespace

extern "C" int arseg_packed_k(int Cin_pad, int R, int S) {
    const int K = R * S * Cin_pad;
    return (K + KALIGN - 1) / KALIGN * KALIGN;
}

extern "C" int arseg_conv_out_hw(const arseg_conv_desc *d, int *Ho, int *Wo) {
    ConvPlan pl;
    if (int e = make_plan(d, &pl)) return e;
    if (Ho) *Ho = pl.Ho;
    if (Wo) *Wo = pl.Wo;
    return ARSEG_OK;
}

extern "C" int arseg_conv_plan_query(int engine, const arseg_conv_desc *d, arseg_conv_plan_info *info) {
    if (!d || !info || (engine != ARSEG_CONV_ENGINE_F32 && engine != ARSEG_CONV_ENGINE_16)) return ARSEG_EINVAL;
    const bool e16 = engine == ARSEG_CONV_ENGINE_16;
    ConvPlan pl{};
    if (const ConvPlanRow *row = e16 ? conv_plan_row(kConvPlans16, d->tile_cfg) : conv_plan_row(kConvPlans32, d->tile_cfg)) pl.take(*row);
    const int st = e16 ? conv16_plan(d, &pl) : make_plan(d, &pl);
    *info = pl;          // (refused: what the id is; the shape's fields are then without meaning)
    return st;
}

extern "C" size_t arseg_conv2d_workspace_bytes(const arseg_conv_desc *d) {
    arseg_conv_plan_info info;
    return arseg_conv_plan_query(ARSEG_CONV_ENGINE_F32, d, &info) == ARSEG_OK ? info.workspace_bytes : 0;
}

extern "C" int arseg_conv2d_fwd(const arseg_conv_desc *d, const float *in, const float *w_packed, const float *scale,
                                const float *bias, const float *residual, float *out, void *workspace,
                                size_t workspace_bytes, arseg_stream_t stream) {
    ConvPlan pl;
    int st = make_plan(d, &pl);
    if (st != ARSEG_OK) return st;
    ARSEG_CHECK_PTR(in); ARSEG_CHECK_PTR(w_packed); ARSEG_CHECK_PTR(out);
    if (!ARSEG_ALIGNED16(in) || !ARSEG_ALIGNED16(w_packed)) return ARSEG_EINVAL;
    if (residual && d->res_ld < d->Cout) return ARSEG_EINVAL;
    if (pl.kind == ARSEG_PLAN_UP2_C64) return residual ? ARSEG_EUNSUPPORTED : arseg_conv_up2_c64_fwd(d, in, w_packed, scale, bias, out, 0, stream);
    if (pl.nsplit > 1) {
        if (!workspace || workspace_bytes < pl.workspace_bytes) return ARSEG_EWORKSPACE;
        if (!ARSEG_ALIGNED16(workspace)) return ARSEG_EINVAL;
    }
    ConvParams p;
    p.in = in; p.w = w_packed; p.scale = scale; p.bias = bias; p.res = residual; p.out = out;
    p.ws = reinterpret_cast<float *>(workspace);
    p.N = d->N; p.H = d->H; p.W = d->W; p.Cin = d->Cin; p.in_ld = d->in_ld;
    p.log2Cin = 0;
    while ((1 << p.log2Cin) < d->Cin) ++p.log2Cin;
    p.inv_S = 65536 / d->S + 1;
    p.in_bytes = (unsigned)((((long long)d->N * d->H * d->W - 1) * d->in_ld + d->Cin) * 4);
    p.w_bytes = (unsigned)((long long)d->Cout * pl.Kpad * 4);
    {
        const long long ob = (((long long)pl.M - 1) * d->out_ld + d->Cout) * 4, rb = (((long long)pl.M - 1) * d->res_ld + d->Cout) * 4;
        const bool fits = ob < (1ll << 31) && (!residual || rb < (1ll << 31));
        p.out_bytes = fits ? (unsigned)ob : 0u;
        p.res_bytes = fits ? (residual ? (unsigned)rb : (unsigned)ob) : 0u;
    }
    p.Ho = pl.Ho; p.Wo = pl.Wo; p.Cout = d->Cout; p.out_ld = d->out_ld; p.res_ld = d->res_ld;
    p.R = d->R; p.S = d->S; p.stride = d->stride; p.pad = d->pad; p.dil = d->dil;
    p.K = pl.K; p.Kpad = pl.Kpad; p.M = pl.M;
    p.act = d->act; p.slope = d->prelu_slope;
    p.ktiles = pl.ktiles; p.ktiles_per_split = pl.ktiles_per_split; p.nsplit = pl.nsplit;
    p.tiles_m = pl.tiles_m; p.tiles_n = pl.tiles_n;
    p.N_batch = d->batch > 1 ? d->batch : 1;
    p.in_bs = d->batch > 1 ? d->in_batch_stride : 0; p.w_bs = d->batch > 1 ? d->w_batch_stride : 0;
    p.out_bs = d->batch > 1 ? d->out_batch_stride : 0;
    if (d->batch > 1 && (residual || d->batch > 65535 || (d->in_batch_stride & 3) || (d->w_batch_stride & 3))) return ARSEG_EINVAL;
    hipStream_t hs = arseg_stream(stream);
    p.up2 = d->upsample2x ? 1 : 0;
    p.range_flag = d->math == ARSEG_MATH_F16X3 ? reinterpret_cast<unsigned *>(d->range_flag) : nullptr;
    p.range_limit = d->range_limit > 0.0f ? d->range_limit : 65504.0f;
    if (p.range_flag && (reinterpret_cast<uintptr_t>(p.range_flag) & 3)) return ARSEG_EINVAL;
    if (pl.kind == ARSEG_PLAN_PATCH) {
        p.in_bytes = d->upsample2x ? (unsigned)((((long long)d->N * (d->H >> 1) * (d->W >> 1) - 1) * d->in_ld + d->Cin) * 4)
                                   : (unsigned)((((long long)d->N * d->H * d->W - 1) * d->in_ld + d->Cin) * 4);
        if (pl.bm == 256) return pl.bn == 64 ? launch_patch<64, 4>(p, pl, d->dil, hs) : launch_patch<128, 4>(p, pl, d->dil, hs);
        return pl.bn == 64 ? launch_patch<64, 2>(p, pl, d->dil, hs) : launch_patch<128, 2>(p, pl, d->dil, hs);
    }
    st = d->math == ARSEG_MATH_F16X3 ? launch_math<ARSEG_MATH_F16X3>(p, pl, hs)
         : (d->math == ARSEG_MATH_F16 ? launch_math<ARSEG_MATH_F16>(p, pl, hs) : launch_math<ARSEG_MATH_F32>(p, pl, hs));
    if (st != ARSEG_OK) return st;
    if (pl.nsplit > 1) {
        const long long total = (long long)pl.M * (d->Cout >> 2);
        int blocks = arseg_cdiv(total, 256);
        if (blocks > 4096) blocks = 4096;
        hipLaunchKernelGGL(conv_splitk_reduce_kernel, dim3(blocks), dim3(256), 0, hs, p);
        st = arseg_launch_status();
    }
    return st;
}

// ---------------------------------------------------------------------------------------------
// host-side weight packer
// ---------------------------------------------------------------------------------------------
extern "C" int arseg_pack_conv_weight_host(const float *w, int Cout, int Cin, int R, int S, int Cin_pad, float *out) {
    if (!w || !out || Cout <= 0 || Cin <= 0 || R <= 0 || S <= 0 || Cin_pad < Cin || (Cin_pad & 3)) return ARSEG_EINVAL;
    const int Kpad = arseg_packed_k(Cin_pad, R, S);
    for (int co = 0; co < Cout; ++co) {
        float *o = out + (size_t)co * Kpad;
        for (int k = 0; k < Kpad; ++k) o[k] = 0.0f;
        for (int ci = 0; ci < Cin; ++ci)
            for (int r = 0; r < R; ++r)
                for (int s = 0; s < S; ++s) o[(r * S + s) * Cin_pad + ci] = w[(((size_t)co * Cin + ci) * R + r) * S + s];
    }
    return ARSEG_OK;
}

// fp32 packed weights [Cout][Kpad] -> f16x3 operand format: per 32-k tile 32 hi halves then 32 lo halves (same bytes),
// row co pre-multiplied by chan_mul[co] = 2^e with max|w| * 2^e in [16,32) -- exact, undone by chan_mul_inv in the epilogue
// scale -- so that the lo halves of the significant weights are normal fp16 numbers.
static inline uint16_t f32_to_f16_rtz(float f) {
    uint32_t u;
    memcpy(&u, &f, 4);
    const uint32_t sign = (u >> 16) & 0x8000u;
    const int32_t e = (int32_t)((u >> 23) & 0xff) - 127 + 15;
    uint32_t man = u & 0x7fffffu;
    if (((u >> 23) & 0xff) == 0xff) return (uint16_t)(sign | 0x7c00u | (man ? 0x200u : 0));
    if (e >= 31) return (uint16_t)(sign | 0x7bffu);                 // RTZ never reaches infinity
    if (e <= 0) {
        if (e < -10) return (uint16_t)sign;
        man |= 0x800000u;
        return (uint16_t)(sign | (man >> (14 - e)));
    }
    return (uint16_t)(sign | ((uint32_t)e << 10) | (man >> 13));
}
static inline float f16_to_f32(uint16_t h) {
    const uint32_t sign = (uint32_t)(h & 0x8000u) << 16;
    const int e = (h >> 10) & 0x1f;
    const uint32_t man = h & 0x3ffu;
    float r;
    if (e == 0) r = ldexpf((float)man, -24);
    else if (e == 31) r = man ? NAN : INFINITY;
    else r = ldexpf((float)(man | 0x400u), e - 25);
    return sign ? -r : r;
}

extern "C" int arseg_split_weight_f16x3_host(const float *w_packed, int Cout, int Kpad, void *out_host, float *chan_mul_inv) {
    if (!w_packed || !out_host || Cout <= 0 || Kpad <= 0 || (Kpad % KALIGN)) return ARSEG_EINVAL;
    uint16_t *o = reinterpret_cast<uint16_t *>(out_host);
    for (int co = 0; co < Cout; ++co) {
        const float *row = w_packed + (size_t)co * Kpad;
        float mx = 0.0f;
        for (int k = 0; k < Kpad; ++k) mx = fmaxf(mx, fabsf(row[k]));
        int e = 0;
        if (chan_mul_inv && mx > 0.0f && std::isfinite(mx)) {
            int ex;
            frexpf(mx, &ex);          // mx = f * 2^ex, f in [0.5,1)  ->  mx * 2^(5-ex) in [16,32)
            e = 5 - ex;
            if (e > 100) e = 100;
            if (e < -100) e = -100;
        }
        if (chan_mul_inv) chan_mul_inv[co] = ldexpf(1.0f, -e);
        constexpr int BK = KALIGN;
        for (int kt = 0; kt < Kpad / BK; ++kt)
            for (int j = 0; j < BK; ++j) {
                const float x = ldexpf(row[kt * BK + j], e);
                const uint16_t hi = f32_to_f16_rtz(x);
                const uint16_t lo = f32_to_f16_rtz(x - f16_to_f32(hi));
                o[((size_t)co * (Kpad / BK) + kt) * 2 * BK + j] = hi;
                o[((size_t)co * (Kpad / BK) + kt) * 2 * BK + BK + j] = lo;
            }
    }
    return ARSEG_OK;
}

extern "C" int arseg_fold_bn_host(const float *gamma, const float *beta, const float *mean, const float *var, float eps,
                                  const float *conv_bias, int C, float *scale_out, float *bias_out) {
    if (!gamma || !beta || !mean || !var || !scale_out || !bias_out || C <= 0) return ARSEG_EINVAL;
    for (int c = 0; c < C; ++c) {
        const double s = (double)gamma[c] / sqrt((double)var[c] + (double)eps);
        scale_out[c] = (float)s;
        bias_out[c] = (float)((double)beta[c] + ((conv_bias ? (double)conv_bias[c] : 0.0) - (double)mean[c]) * s);
    }
    return ARSEG_OK;
}

extern "C" int arseg_pack_dw3x3_host(const float *w, int C, float *out) {
    if (!w || !out || C <= 0) return ARSEG_EINVAL;
    for (int c = 0; c < C; ++c)
        for (int t = 0; t < 9; ++t) out[(size_t)t * C + c] = w[(size_t)c * 9 + t];
    return ARSEG_OK;
}

// ---------------------------------------------------------------------------------------------------------------------------
// "find": times the launch plans a conv shape admits on the device it will run on and returns the fastest.  The candidate set is
// every tile_cfg the shape supports (5..12 GEMM tiles, 13..16 / 20..22 patch-resident, 17..19 large f16x3 tiles, 23 with a fused upsample) x split-K {1,2,3,4,6,8}
// (K long enough, Cout % 4 == 0, not in batched mode) plus the built-in heuristic (0, 0).  Unlike every other entry point this one
// SYNCHRONISES the stream (hipEvent timing); it writes `out` (and the workspace) with real results of each candidate.
namespace {
struct FindCand { int cfg, sk; };
int find_candidates(const arseg_conv_desc *d, FindCand *c, int cap) {
    int n = 0, ktiles = (d->R * d->S * d->Cin + 31) / 32;
    c[n++] = FindCand{0, 0};
    for (int cfg = 1; cfg < (int)(sizeof(kConvPlans32) / sizeof(kConvPlans32[0])) && n < cap; ++cfg) {
        const ConvPlanRow &row = kConvPlans32[cfg];
        // with a fused upsample only the plans that upsample while they stage; without, not up_3's kernel (it refuses every other shape) and not
        // the double-buffered GEMM tiles (their single-buffered twins measured faster)
        if (d->upsample2x ? !row.fuses_up2 : (row.kind == ARSEG_PLAN_NONE || row.kind == ARSEG_PLAN_UP2_C64 || (row.kind == ARSEG_PLAN_TILE && row.nbuf == 2)))
            continue;
        static const int sks[6] = {1, 2, 3, 4, 6, 8};
        for (int i = 0; i < 6 && n < cap; ++i)
            if (sks[i] == 1 || (row.split_k && d->batch <= 1 && ktiles / sks[i] >= 4 && !(d->Cout & 3))) c[n++] = FindCand{cfg, sks[i]};
    }
    return n;
}
}  // namespace

extern "C" size_t arseg_conv2d_find_workspace_bytes(const arseg_conv_desc *d) {
    if (!d) return 0;
    FindCand c[128];
    const int n = find_candidates(d, c, 128);
    size_t best = 0;
    arseg_conv_desc t = *d;
    for (int i = 0; i < n; ++i) {
        t.tile_cfg = c[i].cfg; t.split_k = c[i].sk;
        const size_t b = arseg_conv2d_workspace_bytes(&t);
        if (b > best) best = b;
    }
    return best;
}

extern "C" int arseg_conv2d_find(const arseg_conv_desc *d, const float *in, const float *w_packed, const float *scale, const float *bias,
                                 const float *residual, float *out, void *workspace, size_t workspace_bytes, int reps, int *tile_cfg,
                                 int *split_k, float *best_us, arseg_stream_t stream) {
    if (!d || !tile_cfg || !split_k) return ARSEG_EINVAL;
    ARSEG_CHECK_PTR(in); ARSEG_CHECK_PTR(w_packed); ARSEG_CHECK_PTR(out);
    if (reps <= 0) reps = 3;
    hipStream_t hs = arseg_stream(stream);
    hipEvent_t e0, e1;
    if (hipEventCreate(&e0) != hipSuccess) return ARSEG_EINVAL;
    if (hipEventCreate(&e1) != hipSuccess) { (void)hipEventDestroy(e0); return ARSEG_EINVAL; }
    FindCand c[128];
    const int n = find_candidates(d, c, 128);
    arseg_conv_desc t = *d;
    float best = -1.0f;
    int first_err = ARSEG_EUNSUPPORTED;
    float tms[128];                                   // per candidate: ms for `reps` launches, < 0 = not launched
    auto time_cand = [&](int i, int nrep, float *ms) -> int {
        t.tile_cfg = c[i].cfg; t.split_k = c[i].sk;
        int st = arseg_conv2d_fwd(&t, in, w_packed, scale, bias, residual, out, workspace, workspace_bytes, stream);      // warm
        if (st != ARSEG_OK) return st;
        (void)hipEventRecord(e0, hs);
        for (int r = 0; r < nrep; ++r) st = arseg_conv2d_fwd(&t, in, w_packed, scale, bias, residual, out, workspace, workspace_bytes, stream);
        (void)hipEventRecord(e1, hs);
        if (hipEventSynchronize(e1) != hipSuccess) { const int e = (int)hipGetLastError(); return e ? e : ARSEG_EINVAL; }
        (void)hipEventElapsedTime(ms, e0, e1);
        *ms /= (float)nrep;
        return st;
    };
    for (int i = 0; i < n; ++i) {
        tms[i] = -1.0f;
        t.tile_cfg = c[i].cfg; t.split_k = c[i].sk;
        if (arseg_conv2d_workspace_bytes(&t) > workspace_bytes) continue;
        float ms = 0.0f;
        const int st = time_cand(i, reps, &ms);
        if (st > 0) { (void)hipEventDestroy(e0); (void)hipEventDestroy(e1); return st; }
        if (st != ARSEG_OK) { if (i == 0) first_err = st; continue; }
        tms[i] = ms;
        if (best < 0.0f || ms < best) { best = ms; *tile_cfg = c[i].cfg; *split_k = c[i].sk; }
    }
    // second look at the candidates within 10 % of the fastest, 4x the repetitions: a single short measurement of a 20 us kernel is
    // noisy enough to pick a plan that is 5-10 % slower in steady state (seen as run-to-run spread of the whole step)
    if (best > 0.0f) {
        const float lim = best * 1.10f;
        float best2 = -1.0f;
        for (int i = 0; i < n; ++i) {
            if (tms[i] < 0.0f || tms[i] > lim) continue;
            float ms = 0.0f;
            if (time_cand(i, 4 * reps, &ms) != ARSEG_OK) continue;
            if (best2 < 0.0f || ms < best2) { best2 = ms; *tile_cfg = c[i].cfg; *split_k = c[i].sk; }
        }
        if (best2 > 0.0f) best = best2;
    }
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    if (best < 0.0f) return first_err;          // nothing could be launched (e.g. the 2 GiB limit of the 32-bit buffer offsets)
    if (best_us) *best_us = best * 1000.0f;
    return ARSEG_OK;
}
