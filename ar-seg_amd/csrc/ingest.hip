// Fused ingest of decoder frames (include/arseg_hip.h, arseg_frame_ingest_fwd / arseg_frame_ingest_yuv_fwd): interleaved RGB8, NV12, planar
// I420 or 10-bit P010 / I010 (all 4:2:0) in, the conv engine's input out -- fp32 NHWC4 or fp16 / bf16 NHWC8 -- in one pass: colour conversion,
// the evaluator's bilinear align_corners=True downscale (evaluation.py:186-188), ToTensor + Normalize (dataset/camvid.py:503-506).  No
// intermediate tensor.  ONE kernel family: a per-pixel kernel and a row-staged kernel, each a template over <source format, output type>;
// what differs between the five sources is the Src<FMT> row below.
//
// Per output pixel, all in fp32: the (up to) four taps of the downscale (ingest_src_index); at each tap RGB in the 0-255 scale (RGB8: the
// stored bytes; the others: Y, chroma sampled bilinearly on the stored codes of the half-resolution plane at cx = x / 2, cy = y / 2 - 0.25, both
// clamped to the plane, codes scaled to 8 bits, then the matrix of the colour enum, each component clipped to [0, 255], not rounded); the
// taps are blended with the operation order of the other ingest kernels; then v * na[c] + nb[c] with na = 1 / (255 std), nb = -mean / std
// formed in double on the host ((v / 255 - mean) / std in one fma: within 2 ulp of the two-division form).  16-bit outputs round once, at the
// store (arseg_f2h: v_cvt_pk_bf16_f32 for bf16).
//
// Every floating-point expression of the contract sits in a function under `fp contract(off)`, and the two fused operations that belong to
// it are explicit __builtin_fmaf (the tap weight in ingest_src_index, the normalisation): equal sample values give equal fp32 bits in all
// thirty instantiations, whatever the format they arrive in.  (chroma_pos multiplies by 0.5 and subtracts: exact with or without contraction.)
#include <type_traits>

#include "arseg_device.h"

namespace {

// ------------------------------------------------------------------ the colour contract (documented in include/arseg_hip.h)
// R = ky (Y - y0) + rv (Cr - 128);  G = ky (Y - y0) - gu (Cb - 128) - gv (Cr - 128);  B = ky (Y - y0) + bu (Cb - 128), with
//   rv = 2 (1 - Kr) s,  bu = 2 (1 - Kb) s,  gu = 2 Kb (1 - Kb) / Kg s,  gv = 2 Kr (1 - Kr) / Kg s,  Kg = 1 - Kr - Kb,
// limited range: y0 = 16, ky = 255 / 219, s = 255 / 224;  full range: y0 = 0, ky = 1, s = 1.  BT.601: Kr = 0.299, Kb = 0.114;
// BT.709: Kr = 0.2126, Kb = 0.0722.  The ONE place the four matrices are written: index = enum arseg_colour.
struct ColourK { float y0, ky, rv, gu, gv, bu; };
constexpr ColourK colour_k(double Kr, double Kb, bool full) {
    const double Kg = 1.0 - Kr - Kb, s = full ? 1.0 : 255.0 / 224.0;
    return ColourK{full ? 0.f : 16.f, (float)(full ? 1.0 : 255.0 / 219.0), (float)(2.0 * (1.0 - Kr) * s), (float)(2.0 * Kb * (1.0 - Kb) / Kg * s),
                   (float)(2.0 * Kr * (1.0 - Kr) / Kg * s), (float)(2.0 * (1.0 - Kb) * s)};
}
constexpr ColourK COLOURS[4] = {colour_k(0.299, 0.114, false), colour_k(0.299, 0.114, true), colour_k(0.2126, 0.0722, false), colour_k(0.2126, 0.0722, true)};
// ------------------------------------------------------------------ the source formats: index = enum arseg_src_format
// T = stored sample; PX = bytes per plane-0 pixel; NC = chroma rows staged per source row (0: no chroma, 2: interleaved (Cb, Cr) rows k0, k1,
// 4: planar Cb k0, Cb k1, Cr k0, Cr k1); code() = the sample's code of depth n = 8 (uint8_t) or 10 (uint16_t).  With n the colour contract
// reads: chroma is interpolated on the codes, then Y8 = code cs, C8 - 128 = (code - 2^(n-1)) cs with cs = 2^-(n-8) (limited range) or
// 255 / (2^n - 1) (full range), then the matrix of COLOURS.
template <typename T_, int PX_, int NC_>
struct SrcRow {
    typedef T_ T;
    static constexpr int B = (int)sizeof(T_), PX = PX_, NC = NC_;
    static constexpr bool YUV = NC_ > 0, PLANAR = NC_ == 4;
    static constexpr int CE = PLANAR ? B : 2 * B;                          // bytes per chroma column of a chroma row
    static constexpr int PLANES = !YUV ? 1 : PLANAR ? 3 : 2;
    static __device__ __forceinline__ unsigned code(unsigned s) { return s; }          // 8-bit: the byte
};
template <int FMT> struct Src;
template <> struct Src<ARSEG_SRC_RGB8> : SrcRow<uint8_t, 3, 0> {};
template <> struct Src<ARSEG_SRC_NV12> : SrcRow<uint8_t, 1, 2> {};
template <> struct Src<ARSEG_SRC_I420> : SrcRow<uint8_t, 1, 4> {};
template <> struct Src<ARSEG_SRC_P010> : SrcRow<uint16_t, 2, 2> {
    static __device__ __forceinline__ unsigned code(unsigned s) { return s >> 6; }
};
template <> struct Src<ARSEG_SRC_I010> : SrcRow<uint16_t, 2, 4> {
    static __device__ __forceinline__ unsigned code(unsigned s) { return s & 0x3ffu; }
};

struct IngestP {
    const uint8_t *pl[3];            // RGB8: the interleaved frame;  YUV: luma; Cb (planar) or interleaved (Cb, Cr); Cr (planar only)
    void *out;
    long long pitch[3], ns[3];       // bytes per row / per image of each plane
    int N, H, W, h, w, segs;
    float na[3], nb[3];
    float cs, cmid;                  // code -> 8-bit scale, chroma centre code 2^(n-1)
    ColourK k;
};

// Source taps of output index dst (align_corners=True) as the other ingest kernels compute them once hipcc has contracted their
// `scale * dst - i0`: the ROUNDED product picks the taps, the weight is fma(scale, dst, -i0), i.e. taken from the unrounded product.  Written
// out here so that every instantiation of this file agrees with them whatever the compiler would have contracted (half an ulp of the position
// is 6e-5 pixels at x = 1024: 2e-4 of a normalised value between two unrelated bytes).
__device__ __forceinline__ void ingest_src_index(float scale, int dst, int in, int &i0, int &i1, float &l1) {
    const float src = scale * (float)dst;
    i0 = min((int)src, in - 1);
    i1 = i0 + (i0 < in - 1 ? 1 : 0);
    l1 = fminf(fmaxf(__builtin_fmaf(scale, (float)dst, -(float)i0), 0.f), 1.f);
}

// chroma sample position of luma coordinate v along one axis (half = 0.25 vertically, 0 horizontally): plane index pair + weight of the second
__device__ __forceinline__ void chroma_pos(int v, float shift, int n2, int &i0, int &i1, float &l1) {
    const float c = fminf(fmaxf((float)v * 0.5f - shift, 0.f), (float)(n2 - 1));
    i0 = (int)c;
    i1 = min(i0 + 1, n2 - 1);
    l1 = c - (float)i0;
}

template <int OUT>          // enum arseg_dtype
__device__ __forceinline__ void store_px(void *out, size_t pix, const float (&v)[3]) {
    if constexpr (OUT == ARSEG_DT_F32) {
        const f32x4 o = {v[0], v[1], v[2], 0.f};
        *reinterpret_cast<f32x4 *>((float *)out + pix * 4) = o;
    } else {
        constexpr bool BF = OUT == ARSEG_DT_BF16;
        const u32x4 o = {(unsigned)arseg_f2h<BF>(v[0]) | ((unsigned)arseg_f2h<BF>(v[1]) << 16), (unsigned)arseg_f2h<BF>(v[2]), 0u, 0u};
        *reinterpret_cast<u32x4 *>((uint16_t *)out + pix * 8) = o;
    }
}

// stored codes of one tap (luma, the 2 x 2 chroma neighbourhood q[row 0 | 1, column j0 | j1][Cb, Cr]) -> RGB in the 0-255 scale
__device__ __forceinline__ void yuv_rgb(float yc, const float (&q)[4][2], float wy, float wx, const IngestP &p, float (&rgb)[3]) {
#pragma clang fp contract(off)
    const float cb = (((1.f - wy) * ((1.f - wx) * q[0][0] + wx * q[1][0]) + wy * ((1.f - wx) * q[2][0] + wx * q[3][0])) - p.cmid) * p.cs;
    const float cr = (((1.f - wy) * ((1.f - wx) * q[0][1] + wx * q[1][1]) + wy * ((1.f - wx) * q[2][1] + wx * q[3][1])) - p.cmid) * p.cs;
    const float yl = p.k.ky * (yc * p.cs - p.k.y0);
    rgb[0] = fminf(fmaxf(yl + p.k.rv * cr, 0.f), 255.f);
    rgb[1] = fminf(fmaxf(yl - p.k.gu * cb - p.k.gv * cr, 0.f), 255.f);
    rgb[2] = fminf(fmaxf(yl + p.k.bu * cb, 0.f), 255.f);
}

// blend of the four taps (the other ingest kernels' operation order), then the normalisation as ONE fma; at identity size the one tap is normalised
__device__ __forceinline__ void finish(const float (&a)[3], const float (&b)[3], const float (&c)[3], const float (&d)[3], float ly, float lx,
                                       const IngestP &p, float (&v)[3]) {
#pragma clang fp contract(off)
#pragma unroll
    for (int e = 0; e < 3; ++e)
        v[e] = __builtin_fmaf((1.f - ly) * ((1.f - lx) * a[e] + lx * b[e]) + ly * ((1.f - lx) * c[e] + lx * d[e]), p.na[e], p.nb[e]);
}
__device__ __forceinline__ void norm(const float (&a)[3], const IngestP &p, float (&v)[3]) {
#pragma unroll
    for (int e = 0; e < 3; ++e) v[e] = __builtin_fmaf(a[e], p.na[e], p.nb[e]);
}

// One tap: RGB (0-255 scale) of source pixel x.  `row` = its plane-0 row (RGB8: 3 bytes per pixel; YUV: luma); cb0 / cb1 (cr0 / cr1) = the two
// Cb (Cr) rows under it, wy the weight of the second; with interleaved chroma the Cr rows are the Cb rows + one sample (unused when STAGED:
// the pair is one aligned LDS read of 2 sizeof(T) bytes).  Plane-0 pointers are already shifted so that byte index 0 is byte bias_l of the
// full row, chroma pointers byte bias_c.
template <int FMT, bool STAGED>
__device__ __forceinline__ void tap(const uint8_t *row, const uint8_t *cb0, const uint8_t *cb1, const uint8_t *cr0, const uint8_t *cr1, float wy, int x,
                                    int bias_l, int bias_c, const IngestP &p, float (&rgb)[3]) {
    using S = Src<FMT>;
    using T = typename S::T;
    constexpr int B = S::B, CE = S::CE;
    if constexpr (!S::YUV) {
#pragma unroll
        for (int c = 0; c < 3; ++c) rgb[c] = (float)row[3 * x + c - bias_l];
    } else {
        int j0, j1; float wx;
        chroma_pos(x, 0.f, p.W >> 1, j0, j1, wx);
        const int o0 = CE * j0 - bias_c, o1 = CE * j1 - bias_c;
        float q[4][2];
        if constexpr (!S::PLANAR && STAGED) {
            using Pair = std::conditional_t<B == 1, uint16_t, uint32_t>;
            const uint8_t *src[4] = {cb0 + o0, cb0 + o1, cb1 + o0, cb1 + o1};
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const unsigned pr = *reinterpret_cast<const Pair *>(src[t]);
                q[t][0] = (float)S::code(pr & ((1u << 8 * B) - 1u)); q[t][1] = (float)S::code(pr >> 8 * B);
            }
        } else {
            auto ld = [](const uint8_t *g) { return (float)S::code(*reinterpret_cast<const T *>(g)); };
            q[0][0] = ld(cb0 + o0); q[1][0] = ld(cb0 + o1); q[2][0] = ld(cb1 + o0); q[3][0] = ld(cb1 + o1);
            q[0][1] = ld(cr0 + o0); q[1][1] = ld(cr0 + o1); q[2][1] = ld(cr1 + o0); q[3][1] = ld(cr1 + o1);
        }
        const float yc = (float)S::code(*reinterpret_cast<const T *>(row + B * x - bias_l));
        yuv_rgb(yc, q, wy, wx, p, rgb);
    }
}

// ------------------------------------------------------------------ per-pixel form: any shape, any alignment the entry points admit
template <int FMT, int OUT>
__global__ __launch_bounds__(256) void ingest_kernel(const IngestP p) {
    using S = Src<FMT>;
    const long long total = (long long)p.N * p.h * p.w;
    const float sy = arseg_resize_scale(p.H, p.h, true), sx = arseg_resize_scale(p.W, p.w, true);
    const bool same = (p.h == p.H && p.w == p.W);
    const long long cpitch = p.pitch[S::PLANAR ? 2 : 1];                  // pitch of the rows the Cr samples sit in
    for (long long pix = (long long)blockIdx.x * blockDim.x + threadIdx.x; pix < total; pix += (long long)gridDim.x * blockDim.x) {
        const int ox = (int)(pix % p.w), oy = (int)((pix / p.w) % p.h), n = (int)(pix / ((long long)p.w * p.h));
        const uint8_t *b0 = p.pl[0] + (size_t)n * p.ns[0], *b1 = S::YUV ? p.pl[1] + (size_t)n * p.ns[1] : nullptr;
        const uint8_t *b2 = S::PLANAR ? p.pl[2] + (size_t)n * p.ns[2] : S::YUV ? b1 + S::B : nullptr;
        int y0 = oy, y1 = oy, x0 = ox, x1 = ox; float ly = 0.f, lx = 0.f;
        if (!same) {
            ingest_src_index(sy, oy, p.H, y0, y1, ly);
            ingest_src_index(sx, ox, p.W, x0, x1, lx);
        }
        float t[4][3], v[3];
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            if (r == 1 && same) break;
            const int y = r ? y1 : y0;
            int k0 = 0, k1 = 0; float wy = 0.f;
            if constexpr (S::YUV) chroma_pos(y, 0.25f, p.H >> 1, k0, k1, wy);
            const uint8_t *row = b0 + (size_t)y * p.pitch[0], *cb0 = b1 + (size_t)k0 * p.pitch[1], *cb1 = b1 + (size_t)k1 * p.pitch[1];
            const uint8_t *cr0 = b2 + (size_t)k0 * cpitch, *cr1 = b2 + (size_t)k1 * cpitch;
            tap<FMT, false>(row, cb0, cb1, cr0, cr1, wy, x0, 0, 0, p, t[2 * r]);
            if (!same) tap<FMT, false>(row, cb0, cb1, cr0, cr1, wy, x1, 0, 0, p, t[2 * r + 1]);
        }
        if (same) norm(t[0], p, v);
        else finish(t[0], t[1], t[2], t[3], ly, lx, p, v);
        store_px<OUT>(p.out, (size_t)pix, v);
    }
}

// ------------------------------------------------------------------ row-staged form (the twin of frame_to_nhwc_rows_kernel, csrc/layers.hip)
// One workgroup = 256 consecutive output pixels of one output row.  Per source row under it (two; one at identity size) LDS holds the
// plane-0 row over the pixels' x span and, for YUV, its NC chroma rows over columns xa / 2 .. xe1 / 2 + 1, staged with coalesced 4-byte loads
// (a per-pixel gather of 3-byte pixels / chroma samples is not); the taps come from there, every lane stores 16 bytes.  Needs 4-byte aligned
// plane pointers, pitches and image strides and a horizontal scale <= 4.1.
constexpr int IN_SPAN = 1056;                    // staged source pixels per row: 255 * sx + 2 (+3 alignment, +3 chroma reach) <= IN_SPAN
template <int FMT>
struct Stage {
    using S = Src<FMT>;
    static constexpr int LB = S::PX * IN_SPAN + 16;                                   // plane-0 row: <= PX (IN_SPAN - 6) bytes + alignment
    static constexpr int CB = S::PLANAR ? S::B * (IN_SPAN / 2) + 16 : LB;             // chroma row: <= IN_SPAN / 2 - 1 columns of CE bytes + alignment
    static constexpr int SET = LB + S::NC * CB;                                       // one source row's rows
    static constexpr int CR = S::PLANAR ? 2 * CB : 0;                                 // from the Cb rows to the Cr rows (interleaved: the same rows)
};

template <int FMT, int OUT>
__global__ __launch_bounds__(256) void ingest_rows_kernel(const IngestP p) {
    using S = Src<FMT>;
    using G = Stage<FMT>;
    constexpr int PX = S::PX, CE = S::CE, NC = S::NC, LB = G::LB, CB = G::CB, SET = G::SET, CR = G::CR;
    __shared__ __attribute__((aligned(16))) uint8_t st[2 * SET];
    const float sy = arseg_resize_scale(p.H, p.h, true), sx = arseg_resize_scale(p.W, p.w, true);
    const bool same = (p.h == p.H && p.w == p.W);
    const int seg = blockIdx.x % p.segs, oy = (blockIdx.x / p.segs) % p.h, n = blockIdx.x / (p.segs * p.h);
    const int ox0 = seg * 256, ox1 = min(ox0 + 255, p.w - 1);
    int y0 = oy, y1 = oy, xa = ox0, xe1 = ox1, xt; float ly = 0.f, lt;
    if (!same) {
        ingest_src_index(sy, oy, p.H, y0, y1, ly);
        ingest_src_index(sx, ox0, p.W, xa, xt, lt);
        ingest_src_index(sx, ox1, p.W, xt, xe1, lt);
    }
    const int W2 = p.W >> 1, ca = xa >> 1, cl = min((xe1 >> 1) + 1, W2 - 1);          // first / last staged chroma column
    const int lrow = PX * p.W, crow = CE * W2;                                         // bytes of a plane-0 / chroma row
    const int bias_l = (PX * xa) & ~3, bias_c = (CE * ca) & ~3;
    const int nl = (PX * xe1 + PX - 1 - bias_l) / 4 + 1, nc = (CE * cl + CE - 1 - bias_c) / 4 + 1;          // 4-byte chunks (<= LB / 4, CB / 4)
    int ka0 = 0, ka1 = 0, kb0 = 0, kb1 = 0; float wya = 0.f, wyb = 0.f;               // chroma rows under y0 (a) and y1 (b)
    if constexpr (S::YUV) { chroma_pos(y0, 0.25f, p.H >> 1, ka0, ka1, wya); chroma_pos(y1, 0.25f, p.H >> 1, kb0, kb1, wyb); }
    const uint8_t *b0 = p.pl[0] + (size_t)n * p.ns[0], *b1 = S::YUV ? p.pl[1] + (size_t)n * p.ns[1] : nullptr;
    const uint8_t *b2 = S::PLANAR ? p.pl[2] + (size_t)n * p.ns[2] : nullptr;
    const int per = nl + NC * nc, total = (same ? 1 : 2) * per;
    for (int i = threadIdx.x; i < total; i += 256) {
        const int set = i >= per ? 1 : 0;
        int j = i - set * per, off, rb, lo = set * SET;
        const uint8_t *g;
        if (!S::YUV || j < nl) {
            g = b0 + (size_t)(set ? y1 : y0) * p.pitch[0]; off = bias_l + 4 * j; rb = lrow; lo += 4 * j;
        } else {
            j -= nl;
            const int sub = j / nc, ch = j - sub * nc;                                 // sub: Cb k0, Cb k1, Cr k0, Cr k1 (planar) | k0, k1 (interleaved)
            const int kr = (sub & 1) ? (set ? kb1 : ka1) : (set ? kb0 : ka0);
            const bool third = S::PLANAR && sub >= 2;
            g = (third ? b2 : b1) + (size_t)kr * p.pitch[third ? 2 : 1]; off = bias_c + 4 * ch; rb = crow; lo += LB + sub * CB + 4 * ch;
        }
        unsigned v = 0;
        if (off + 4 <= rb) {
            v = *reinterpret_cast<const unsigned *>(g + off);
        } else {                                             // the row's last, partial chunk: never read past the row
            for (int b = 0; b < 4; ++b)
                if (off + b < rb) v |= (unsigned)g[off + b] << (8 * b);
        }
        *reinterpret_cast<unsigned *>(&st[lo]) = v;
    }
    __syncthreads();
    const int ox = ox0 + threadIdx.x;
    if (ox < p.w) {
        float t[4][3], v[3];
        const uint8_t *c = st + LB;
        if (same) {
            tap<FMT, true>(st, c, c + CB, c + CR, c + CR + CB, wya, ox, bias_l, bias_c, p, t[0]);
            norm(t[0], p, v);
        } else {
            int x0, x1; float lx;
            ingest_src_index(sx, ox, p.W, x0, x1, lx);
#pragma unroll
            for (int r = 0; r < 2; ++r) {
                const uint8_t *row = st + r * SET, *cr = c + r * SET;
                tap<FMT, true>(row, cr, cr + CB, cr + CR, cr + CR + CB, r ? wyb : wya, x0, bias_l, bias_c, p, t[2 * r]);
                tap<FMT, true>(row, cr, cr + CB, cr + CR, cr + CR + CB, r ? wyb : wya, x1, bias_l, bias_c, p, t[2 * r + 1]);
            }
            finish(t[0], t[1], t[2], t[3], ly, lx, p, v);
        }
        store_px<OUT>(p.out, ((size_t)n * p.h + oy) * p.w + ox, v);
    }
}

template <int FMT, int OUT>
int launch(const IngestP &p, bool staged, hipStream_t st) {
    if (staged) hipLaunchKernelGGL((ingest_rows_kernel<FMT, OUT>), dim3((unsigned)(p.N * p.h * p.segs)), dim3(256), 0, st, p);
    else hipLaunchKernelGGL((ingest_kernel<FMT, OUT>), dim3(arseg_grid_for((long long)p.N * p.h * p.w)), dim3(256), 0, st, p);
    return arseg_launch_status();
}

// ------------------------------------------------------------------ host: what both entry points take, validated once
struct IngestCall {
    const void *plane[3];
    int64_t pitch[3], ns[3];
    int colour;
    void *out;
    int out_dtype, N, H, W, h, w;
    const float *mean3, *std3;
    arseg_stream_t stream;
};

// Planes past Src<FMT>::PLANES, and colour without chroma, are not looked at.
template <int FMT>
int ingest(const IngestCall &a) {
    using S = Src<FMT>;
    ARSEG_CHECK_PTR(a.out); ARSEG_CHECK_PTR(a.mean3); ARSEG_CHECK_PTR(a.std3);
    ARSEG_CHECK_POS(a.N); ARSEG_CHECK_POS(a.H); ARSEG_CHECK_POS(a.W); ARSEG_CHECK_POS(a.h); ARSEG_CHECK_POS(a.w);
    if (a.out_dtype != ARSEG_DT_F32 && a.out_dtype != ARSEG_DT_F16 && a.out_dtype != ARSEG_DT_BF16) return ARSEG_EINVAL;
    if (a.std3[0] == 0.f || a.std3[1] == 0.f || a.std3[2] == 0.f || !ARSEG_ALIGNED16(a.out)) return ARSEG_EINVAL;
    if (S::YUV && ((a.H & 1) || (a.W & 1) || a.colour < 0 || a.colour > ARSEG_COLOUR_BT709_FULL)) return ARSEG_EINVAL;
    IngestP p = {};
    p.out = a.out; p.N = a.N; p.H = a.H; p.W = a.W; p.h = a.h; p.w = a.w; p.segs = arseg_cdiv(a.w, 256);
    bool staged = a.W >= 8 && 255.f * arseg_resize_scale(a.W, a.w, true) + 8.f <= (float)IN_SPAN && (long long)a.N * a.h * p.segs < (1ll << 31);
    for (int i = 0; i < S::PLANES; ++i) {
        ARSEG_CHECK_PTR(a.plane[i]);
        const int64_t row = i == 0 ? (int64_t)S::PX * a.W : (int64_t)S::CE * (a.W / 2);          // bytes of a row of plane i
        if (a.pitch[i] < row || a.ns[i] < 0) return ARSEG_EINVAL;
        const uintptr_t bits = reinterpret_cast<uintptr_t>(a.plane[i]) | (uintptr_t)a.pitch[i] | (uintptr_t)a.ns[i];
        if (bits & (uintptr_t)(S::B - 1)) return ARSEG_EINVAL;                                     // 16-bit samples: even pointer, pitch, image stride
        staged = staged && (bits & 3u) == 0;
        p.pl[i] = (const uint8_t *)a.plane[i]; p.pitch[i] = a.pitch[i]; p.ns[i] = a.ns[i];
    }
    for (int c = 0; c < 3; ++c) {
        p.na[c] = (float)(1.0 / (255.0 * (double)a.std3[c]));
        p.nb[c] = (float)(-(double)a.mean3[c] / (double)a.std3[c]);
    }
    const int colour = S::YUV ? a.colour : 0;
    const bool full = colour == ARSEG_COLOUR_BT601_FULL || colour == ARSEG_COLOUR_BT709_FULL;
    p.k = COLOURS[colour];
    p.cs = S::B == 1 ? 1.f : full ? (float)(255.0 / 1023.0) : 0.25f;
    p.cmid = S::B == 1 ? 128.f : 512.f;
    hipStream_t st = arseg_stream(a.stream);
    return a.out_dtype == ARSEG_DT_F32 ? launch<FMT, ARSEG_DT_F32>(p, staged, st)
         : a.out_dtype == ARSEG_DT_F16 ? launch<FMT, ARSEG_DT_F16>(p, staged, st) : launch<FMT, ARSEG_DT_BF16>(p, staged, st);
}

int ingest_any(int src_format, const IngestCall &a) {
    switch (src_format) {
    case ARSEG_SRC_RGB8: return ingest<ARSEG_SRC_RGB8>(a);
    case ARSEG_SRC_NV12: return ingest<ARSEG_SRC_NV12>(a);
    case ARSEG_SRC_I420: return ingest<ARSEG_SRC_I420>(a);
    case ARSEG_SRC_P010: return ingest<ARSEG_SRC_P010>(a);
    case ARSEG_SRC_I010: return ingest<ARSEG_SRC_I010>(a);
    default: return ARSEG_EINVAL;
    }
}

}  // namespace

extern "C" int arseg_frame_ingest_fwd(const void *plane0, const void *plane1, int src_format, int64_t pitch0, int64_t pitch1, int64_t n_stride0,
                                      int64_t n_stride1, int colour, void *out, int out_dtype, int N, int H, int W, int h, int w, const float *mean3,
                                      const float *std3, arseg_stream_t stream) {
    if (src_format != ARSEG_SRC_RGB8 && src_format != ARSEG_SRC_NV12) return ARSEG_EINVAL;
    return ingest_any(src_format, {{plane0, plane1, nullptr}, {pitch0, pitch1, 0}, {n_stride0, n_stride1, 0}, colour, out, out_dtype, N, H, W, h, w,
                                   mean3, std3, stream});
}

extern "C" int arseg_frame_ingest_yuv_fwd(const void *plane0, const void *plane1, const void *plane2, int src_format, int64_t pitch0, int64_t pitch1,
                                          int64_t pitch2, int64_t n_stride0, int64_t n_stride1, int64_t n_stride2, int colour, void *out, int out_dtype,
                                          int N, int H, int W, int h, int w, const float *mean3, const float *std3, arseg_stream_t stream) {
    if (src_format != ARSEG_SRC_I420 && src_format != ARSEG_SRC_P010 && src_format != ARSEG_SRC_I010) return ARSEG_EINVAL;
    return ingest_any(src_format, {{plane0, plane1, plane2}, {pitch0, pitch1, pitch2}, {n_stride0, n_stride1, n_stride2}, colour, out, out_dtype, N, H, W,
                                   h, w, mean3, std3, stream});
}
