// up_3 of the PSPNet decoder: 3x3 stride-1 pad-1 conv, 64 -> 64 channels, on the x2 bilinear (align_corners=False) upsample of its input
// (PSPUpsample, model/pspnet.py:43-46), split-fp16 arithmetic (ARSEG_MATH_F16X3), folded scale / bias / activation epilogue.  tile_cfg 23 of
// arseg_conv_desc; the general patch-resident kernel (conv_igemm.hip, conv3x3_patch_kernel) serves every other shape.
//
// That kernel spends this layer's time outside the matrix cores: with Cin = 64 a tile has two 32-channel chunks, so the staging of the first
// patch hides under nothing, every one of the 18 taps streams a weight tile through LDS behind its own barrier -- the same 147 KB for every
// tile of the launch -- and all waves stage, then all waves multiply.  Here
//   * the grid is persistent: at most one workgroup of 8 waves per compute unit walks a run of 8 x 16 pixel tiles (XCD-contiguous chunks,
//     the workgroups of an XCD interleaved inside its chunk, so concurrently running tiles share their halo in that XCD's L2);
//   * waves 0..3 multiply (ROLE_MMA).  Wave s owns output channels 16 s .. 16 s + 15 and keeps their hi and lo weight fragments for the nine
//     taps of both chunks in registers (36 fragments = 144 VGPRs), loaded once before its first tile: no weight goes through LDS, no barrier
//     per tap.  v_mfma_f32_16x16x32_f16 with the weights as the A operand and 16 pixels of a tile row as B: a lane ends up with 4 consecutive
//     channels of one pixel = one 16-byte store;
//   * waves 4..7 stage (ROLE_STAGE) the patch of the NEXT tile -- both chunks, the upsample blend, the hi/lo split; the arithmetic of
//     conv3x3_patch_kernel's store_patch, operation for operation -- into the other half of a double-buffered patch, under the 432 MFMAs of
//     the current one.  One barrier per tile.
// K order as in the patch kernel: chunk outer, tap inner, per product a_lo.w_hi + a_hi.w_lo + a_hi.w_hi (a 32-deep MFMA where that kernel
// issues two 16-deep ones).
//
// LDS image of one patch buffer: 4 planes (chunk, hi | lo) of 180 pixel rows of 64 bytes (32 halves = four 16-byte k groups); the k group g
// of patch pixel px sits in slot g ^ ((px >> 1) & 2) of its row.  A ds_read_b128 lane group holds 8 pixels on group g and 8 on g ^ 1; pixel
// rows are consecutive, so with the swizzle the 16 lanes fall on 16 different 16-byte slots of the 256-byte bank row whatever the tap offset.
#include "arseg_device.h"
#include "conv_plans.h"
#include <cmath>

namespace {

constexpr int TH = 8, TW = 16, PH = TH + 2, PW = TW + 2, NPX = PH * PW;      // output tile, staged patch (180 pixels)
constexpr int PLANE = NPX * 64, BUFB = 4 * PLANE;                            // bytes: one (chunk, hi | lo) plane, one patch buffer (46080)
constexpr int BWC = PW / 2, NBLK = (PH / 2) * BWC;                           // 2 x 2 blocks of the patch: 5 x 9
constexpr int NMMA = 256, NSTAGE = 256, NT = NMMA + NSTAGE;
constexpr int MAXU = (NBLK * 16 + NSTAGE - 1) / NSTAGE;                      // items (block, 16-byte piece of the 64 channels) per staging thread: 3
constexpr int KT = 18;                                                       // 32-deep K tiles of the packed weights: kt = 2 * tap + chunk
constexpr unsigned OOB = 0x80000000u;                                        // beyond num_records of every descriptor: loads return 0, stores are dropped
enum { ROLE_MMA = 0, ROLE_STAGE = 1 };

struct Up2Params {
    const float *in, *w, *scale, *bias;
    float *out;
    int H, W, in_ld, out_ld;                 // H, W: the conv's (upsampled) size; `in` is [N, H/2, W/2, in_ld]
    int tiles_x, tiles_y, ntiles;
    int act;
    float slope;
    unsigned *range_flag;
    float range_limit;
    unsigned in_bytes, w_bytes, out_bytes;
};

// The tiles of this workgroup: first, first + stride, ... (count of them).  The tile list is cut into min(8, grid) contiguous chunks, one per
// XCD (workgroup b runs on XCD b % 8); the workgroups of an XCD take the tiles of its chunk in turn.
struct TileRun { int first, stride, count; };
__device__ __forceinline__ TileRun tile_run(int ntiles) {
    const int G = (int)gridDim.x, b = (int)blockIdx.x, nx = G < 8 ? G : 8;
    const int xcd = b % nx, idx = b / nx, wgs = (G - xcd + nx - 1) / nx;
    const int q = ntiles / nx, r = ntiles - q * nx;
    const int start = xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q, cnt = q + (xcd < r ? 1 : 0);
    return TileRun{start + idx, wgs, idx < cnt ? (cnt - idx + wgs - 1) / wgs : 0};
}
struct TilePos { int img, ty0, tx0; };
__device__ __forceinline__ TilePos tile_pos(const Up2Params &p, int t) {
    const int per = p.tiles_x * p.tiles_y, img = t / per, rem = t - img * per, ty = rem / p.tiles_x;
    return TilePos{img, ty * TH, (rem - ty * p.tiles_x) * TW};
}

template <int ROLE>
__device__ __forceinline__ void up2_role(const Up2Params &p, unsigned char *lds) {
    const TileRun run = tile_run(p.ntiles);
    if (run.count == 0) return;                                  // (both roles: no barrier is left waiting)

    if constexpr (ROLE == ROLE_STAGE) {
        const int ptid = (int)threadIdx.x - NMMA;
        const __amdgpu_buffer_rsrc_t a_rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(p.in), 0, (int)p.in_bytes, 0x00020000);
        const bool watch = p.range_flag != nullptr;
        float vmax = 0.f;
        const int h = p.H >> 1, w = p.W >> 1;
        // item it of this thread: block (by, bx) of the patch = upsampled rows 2 iy + 1, 2 iy + 2 x columns 2 ix + 1, 2 ix + 2, channels 4 * p16 .. + 3
        int by[MAXU], bx[MAXU], upx[MAXU];
#pragma unroll
        for (int it = 0; it < MAXU; ++it) {
            const int b = (ptid + it * NSTAGE) >> 4;
            by[it] = b / BWC; bx[it] = b - by[it] * BWC;
            upx[it] = b < NBLK ? 2 * by[it] * PW + 2 * bx[it] : -1;
        }
        const int p16 = ptid & 15;                                 // (NSTAGE % 16 == 0: the same piece for every item)
        u32x4 rq[MAXU][4];
        int uflag[MAXU];
        // TWIN of conv3x3_patch_kernel<.., UP2 = true> (conv_igemm.hip: uoff / uflag / store_patch): same addressing, flags and operation order;
        // keep the two in step.
        // the quad of low-resolution pixels behind each block of tile t: rows clamp(iy), clamp(iy + 1) x columns clamp(ix), clamp(ix + 1).
        // uflag: bit 0 / 1 row 0 / 1 of the block inside the image, bit 2 / 3 column 0 / 1 inside, bit 4: iy < 0 (row 1 is the image's first
        // row = the low-resolution row itself), bit 5: ix < 0
        auto load_quads = [&](int t) {
            const TilePos tp = tile_pos(p, t);
#pragma unroll
            for (int it = 0; it < MAXU; ++it) {
                const int iy = (tp.ty0 >> 1) - 1 + by[it], ix = (tp.tx0 >> 1) - 1 + bx[it];
                const int ya = min(max(iy, 0), h - 1), yb = min(max(iy + 1, 0), h - 1), xa = min(max(ix, 0), w - 1), xb = min(max(ix + 1, 0), w - 1);
                const unsigned base = (unsigned)(tp.img * h) * (unsigned)w, q16 = (unsigned)p16 * 16u;
                const bool live = upx[it] >= 0;
                const unsigned o0 = live ? ((base + ya * w + xa) * p.in_ld) * 4u + q16 : OOB, o1 = live ? ((base + ya * w + xb) * p.in_ld) * 4u + q16 : OOB;
                const unsigned o2 = live ? ((base + yb * w + xa) * p.in_ld) * 4u + q16 : OOB, o3 = live ? ((base + yb * w + xb) * p.in_ld) * 4u + q16 : OOB;
                rq[it][0] = __builtin_amdgcn_raw_buffer_load_b128(a_rsrc, o0, 0, 0);
                rq[it][1] = __builtin_amdgcn_raw_buffer_load_b128(a_rsrc, o1, 0, 0);
                rq[it][2] = __builtin_amdgcn_raw_buffer_load_b128(a_rsrc, o2, 0, 0);
                rq[it][3] = __builtin_amdgcn_raw_buffer_load_b128(a_rsrc, o3, 0, 0);
                uflag[it] = ((iy >= 0 && 2 * iy + 1 < p.H) ? 1 : 0) | ((2 * iy + 2 < p.H) ? 2 : 0) | ((ix >= 0 && 2 * ix + 1 < p.W) ? 4 : 0) |
                            ((2 * ix + 2 < p.W) ? 8 : 0) | (iy < 0 ? 16 : 0) | (ix < 0 ? 32 : 0);
            }
        };
        auto stage = [&](unsigned char *buf) {
            auto put_px = [&](int px, const f32x4 v) {
                u32x2 hi, lo;
                split4(v, hi, lo);
                if (watch) vmax = fmaxf(fmaxf(vmax, fmaxf(fabsf(v[0]), fabsf(v[1]))), fmaxf(fabsf(v[2]), fabsf(v[3])));
                const int piece = p16 & 7;
                unsigned char *row = buf + (p16 >> 3) * 2 * PLANE + px * 64 + (((piece >> 1) ^ ((px >> 1) & 2)) << 4) + (piece & 1) * 8;
                *reinterpret_cast<u32x2 *>(row) = hi;
                *reinterpret_cast<u32x2 *>(row + PLANE) = lo;
            };
#pragma unroll
            for (int it = 0; it < MAXU; ++it) {
                if (upx[it] < 0) continue;
                const int f = uflag[it];
                const f32x4 q00 = __builtin_bit_cast(f32x4, rq[it][0]), q01 = __builtin_bit_cast(f32x4, rq[it][1]);
                const f32x4 q10 = __builtin_bit_cast(f32x4, rq[it][2]), q11 = __builtin_bit_cast(f32x4, rq[it][3]);
                // vertical blend at the two low-res columns (row 2iy+1: .75 / .25; row 2iy+2: .25 / .75, or the row itself at the top edge)
                const f32x4 r0a = 0.75f * q00 + 0.25f * q10, r0b = 0.75f * q01 + 0.25f * q11;
                const f32x4 r1a = (f & 16) ? q10 : 0.25f * q00 + 0.75f * q10, r1b = (f & 16) ? q11 : 0.25f * q01 + 0.75f * q11;
                const f32x4 z = {0.f, 0.f, 0.f, 0.f};
                const f32x4 o00 = 0.75f * r0a + 0.25f * r0b, o01 = (f & 32) ? r0b : 0.25f * r0a + 0.75f * r0b;
                const f32x4 o10 = 0.75f * r1a + 0.25f * r1b, o11 = (f & 32) ? r1b : 0.25f * r1a + 0.75f * r1b;
                put_px(upx[it], (f & 5) == 5 ? o00 : z);
                put_px(upx[it] + 1, (f & 9) == 9 ? o01 : z);
                put_px(upx[it] + PW, (f & 6) == 6 ? o10 : z);
                put_px(upx[it] + PW + 1, (f & 10) == 10 ? o11 : z);
            }
        };
        // tile j + 1 is staged under the MFMAs of tile j; the quads of tile j + 2 are requested right after and land before the barrier.
        // Trip -1 stages the first tile: ONE copy of the blend code, so a tile's values do not depend on its place in a run (two copies
        // contract their multiply-adds differently: 1 ulp)
        load_quads(run.first);
#pragma unroll 1
        for (int j = -1; j < run.count; ++j) {
            if (j + 1 < run.count) {
                stage(lds + ((j + 1) & 1) * BUFB);
                if (j + 2 < run.count) load_quads(run.first + (j + 2) * run.stride);
            }
            __syncthreads();
        }
        if (watch && vmax > p.range_limit) atomicOr(p.range_flag, 1u);
    } else {
        const int lane = (int)threadIdx.x & 63, slice = (int)threadIdx.x >> 6, l15 = lane & 15, kg = lane >> 4;
        // the wave's weights: channel 16 slice + l15, k = 8 kg .. + 7 of each 32-deep K tile, hi and lo halves
        h16x8 wh[KT], wl[KT];
        {
            const __amdgpu_buffer_rsrc_t b_rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(p.w), 0, (int)p.w_bytes, 0x00020000);
            const unsigned wo = (unsigned)((slice * 16 + l15) * KT) * 128u + (unsigned)kg * 16u;
#pragma unroll
            for (int kt = 0; kt < KT; ++kt) {
                wh[kt] = __builtin_bit_cast(h16x8, __builtin_amdgcn_raw_buffer_load_b128(b_rsrc, wo + kt * 128, 0, 0));
                wl[kt] = __builtin_bit_cast(h16x8, __builtin_amdgcn_raw_buffer_load_b128(b_rsrc, wo + kt * 128 + 64, 0, 0));
            }
        }
        const int c0 = slice * 16 + kg * 4;                         // the 4 output channels of this lane (C/D rows 4 kg + r)
        float sc[4], bi[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) { sc[r] = p.scale ? p.scale[c0 + r] : 1.0f; bi[r] = p.bias ? p.bias[c0 + r] : 0.0f; }
        const ArsegAct ea = arseg_act(p.act, p.slope);
        const u32x4 o_rsrc = make_rsrc(p.out, p.out_bytes);
        // byte offset of this lane's fragment in a plane for patch pixel l15 + C, without the 64 C term: by C & 7 (the swizzle looks at bit 2 of the pixel)
        unsigned swz[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) swz[j] = (unsigned)(l15 * 64 + ((kg ^ (((l15 + j) >> 1) & 2)) << 4));

        __syncthreads();
#pragma unroll 1
        for (int j = 0; j < run.count; ++j) {
            const unsigned char *buf = lds + (j & 1) * BUFB;
            const unsigned char *pj[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) pj[i] = buf + swz[i];
            f32x4 acc[TH];
#pragma unroll
            for (int mf = 0; mf < TH; ++mf) acc[mf] = f32x4{0.f, 0.f, 0.f, 0.f};
            // step g = (chunk, tap, pair of tile rows): the fragments of step g + 1 are read under the 6 MFMAs of step g, and no further ahead
            // (the scheduler, left alone, hoists the reads of whole taps and spills the weights)
            h16x8 fh[2][2], fl[2][2];
            auto frags = [&](int g, h16x8 (&h)[2], h16x8 (&l)[2]) {
                const int ck = g / 36, tap = (g % 36) >> 2;
#pragma unroll
                for (int u = 0; u < 2; ++u) {
                    const int C = (2 * (g & 3) + u + tap / 3) * PW + tap % 3;
                    h[u] = *reinterpret_cast<const h16x8 *>(pj[C & 7] + 2 * ck * PLANE + C * 64);
                    l[u] = *reinterpret_cast<const h16x8 *>(pj[C & 7] + (2 * ck + 1) * PLANE + C * 64);
                }
            };
            frags(0, fh[0], fl[0]);
#pragma unroll
            for (int g = 0; g < 72; ++g) {
                if (g + 1 < 72) frags(g + 1, fh[(g + 1) & 1], fl[(g + 1) & 1]);
                const int kt = 2 * ((g % 36) >> 2) + g / 36;
#pragma unroll
                for (int u = 0; u < 2; ++u) {
                    const int mf = 2 * (g & 3) + u;
                    acc[mf] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wh[kt], fl[g & 1][u], acc[mf], 0, 0, 0);
                    acc[mf] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wl[kt], fh[g & 1][u], acc[mf], 0, 0, 0);
                    acc[mf] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wh[kt], fh[g & 1][u], acc[mf], 0, 0, 0);
                }
                __builtin_amdgcn_sched_group_barrier(0x100, 4, 0);      // the 4 reads first, then the 6 MFMAs
                __builtin_amdgcn_sched_group_barrier(0x008, 6, 0);
                __builtin_amdgcn_sched_barrier(0);
            }
            // epilogue: C/D of the 16x16 MFMA: column (pixel) = lane & 15, row (channel) = 4 * (lane >> 4) + r
            const TilePos tp = tile_pos(p, run.first + j * run.stride);
            const int ox = tp.tx0 + l15;
#pragma unroll
            for (int mf = 0; mf < TH; ++mf) {
                const int oy = tp.ty0 + mf;
                f32x4 v;
#pragma unroll
                for (int r = 0; r < 4; ++r) v[r] = arseg_act_apply(acc[mf][r] * sc[r] + bi[r], ea);
                const unsigned m = ((unsigned)tp.img * (unsigned)p.H + (unsigned)oy) * (unsigned)p.W + (unsigned)ox;
                store16_buf(__builtin_bit_cast(u32x4, v), o_rsrc, (oy < p.H && ox < p.W) ? (m * (unsigned)p.out_ld + (unsigned)c0) * 4u : OOB);
            }
            __syncthreads();
        }
    }
}

__global__ __launch_bounds__(NT) void conv_up2_c64_kernel(const Up2Params p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char up2_smem[];      // [2][BUFB]
    if (threadIdx.x < NMMA) up2_role<ROLE_MMA>(p, up2_smem);
    else up2_role<ROLE_STAGE>(p, up2_smem);
}

}  // namespace

extern "C" int arseg_conv_up2_c64_fwd(const arseg_conv_desc *d, const float *in, const float *w_packed, const float *scale, const float *bias, float *out,
                                      int max_wgs, arseg_stream_t stream) {
    if (!d) return ARSEG_EINVAL;
    if (d->N <= 0 || d->H <= 0 || d->W <= 0 || max_wgs < 0) return ARSEG_EINVAL;
    if (!conv_up2_c64_shape(d)) return ARSEG_EUNSUPPORTED;
    if (d->in_ld < 64 || (d->in_ld & 3) || d->out_ld < 64) return ARSEG_EINVAL;
    if (d->out_ld & 3) return ARSEG_EUNSUPPORTED;                // a lane stores its 4 channels as one 16-byte piece
    if (d->act != ARSEG_ACT_NONE && d->act != ARSEG_ACT_RELU && d->act != ARSEG_ACT_PRELU && d->act != ARSEG_ACT_SIGMOID) return ARSEG_EINVAL;
    ARSEG_CHECK_PTR(in); ARSEG_CHECK_PTR(w_packed); ARSEG_CHECK_PTR(out);
    if (!ARSEG_ALIGNED16(in) || !ARSEG_ALIGNED16(w_packed)) return ARSEG_EINVAL;
    if (!ARSEG_ALIGNED16(out)) return ARSEG_EUNSUPPORTED;
    void *rf = d->range_flag;
    if (rf && (reinterpret_cast<uintptr_t>(rf) & 3)) return ARSEG_EINVAL;
    const long long ib = conv_up2_c64_in_bytes(d), ob = conv_up2_c64_out_bytes(d);
    if ((long long)d->N * d->H * d->W > (1ll << 30) || ib >= (1ll << 31) || ob >= (1ll << 31)) return ARSEG_EUNSUPPORTED;      // 32-bit buffer offsets
    Up2Params p;
    p.in = in; p.w = w_packed; p.scale = scale; p.bias = bias; p.out = out;
    p.H = d->H; p.W = d->W; p.in_ld = d->in_ld; p.out_ld = d->out_ld;
    p.tiles_x = arseg_cdiv(d->W, TW); p.tiles_y = arseg_cdiv(d->H, TH); p.ntiles = d->N * p.tiles_x * p.tiles_y;
    p.act = d->act; p.slope = d->prelu_slope;
    p.range_flag = reinterpret_cast<unsigned *>(rf);
    p.range_limit = d->range_limit > 0.0f ? d->range_limit : 65504.0f;
    p.in_bytes = (unsigned)ib; p.w_bytes = (unsigned)(64 * KT * 128); p.out_bytes = (unsigned)ob;
    hipStream_t hs = arseg_stream(stream);
    static ArsegSmemAttr attr;
    if (int e = arseg_allow_smem(attr, reinterpret_cast<const void *>(conv_up2_c64_kernel), 2 * BUFB)) return e;
    const int cus = arseg_cu_count(max_wgs), grid = p.ntiles < cus ? p.ntiles : cus;      // persistent: at most one workgroup per compute unit
    hipLaunchKernelGGL(conv_up2_c64_kernel, dim3(grid), dim3(NT), 2 * BUFB, hs, p);
    return arseg_launch_status();
}
