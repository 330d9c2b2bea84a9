// Fused ingest of 8-bit decoder frames (include/arseg_hip.h, arseg_frame_ingest_fwd): interleaved RGB8 or NV12 (4:2:0) in, the conv
// engine's input out -- fp32 NHWC4 or fp16 / bf16 NHWC8 -- in one pass: colour conversion (NV12), the evaluator's bilinear
// align_corners=True downscale (evaluation.py:186-188), ToTensor + Normalize (dataset/camvid.py:503-506).  No intermediate tensor.
//
// Per output pixel, all in fp32: the (up to) four taps of the downscale (ingest_src_index); at each tap RGB in the 0-255
// scale (RGB8: the stored bytes; NV12: Y, chroma sampled bilinearly from the half-resolution plane at cx = x / 2, cy = y / 2 - 0.25,
// both clamped to the plane, then the matrix of the colour enum, each component clipped to [0, 255], not rounded); the taps are blended
// with the operation order of the other ingest kernels; then v * na[c] + nb[c] with na = 1 / (255 std), nb = -mean / std formed in
// double on the host ((v / 255 - mean) / std in one fma: within 2 ulp of the two-division form).  16-bit outputs round once, at the
// store (arseg_f2h: v_cvt_pk_bf16_f32 for bf16).  Planar I420 and 10-bit P010 / I010 sources (arseg_frame_ingest_yuv_fwd): the second
// kernel family further down, same shapes, same contract with a bit depth.
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

struct IngestP {
    const uint8_t *p0, *p1;          // RGB8: interleaved frame, unused;  NV12: luma plane, interleaved (Cb, Cr) plane
    void *out;
    long long pitch0, pitch1, ns0, ns1;      // bytes per row / per image of each plane
    int N, H, W, h, w, segs;
    float na[3], nb[3];
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

// One tap: RGB (0-255 scale) of source pixel x of one source row.  `row` = that row (RGB8: 3 bytes per pixel; NV12: luma), `c0` / `c1` =
// the two chroma rows under it with wy the weight of c1; all three already shifted so that byte index 0 is byte `bias` of the full row.
template <bool NV12, bool PAIR16>
__device__ __forceinline__ void tap(const uint8_t *row, const uint8_t *c0, const uint8_t *c1, float wy, int x, int bias, int W, const ColourK &k, float (&rgb)[3]) {
    if constexpr (!NV12) {
#pragma unroll
        for (int c = 0; c < 3; ++c) rgb[c] = (float)row[3 * x + c - bias];
    } else {
        int j0, j1; float wx;
        chroma_pos(x, 0.f, W >> 1, j0, j1, wx);
        float q[4][2];                                    // (row 0 | 1, column j0 | j1) x (Cb, Cr)
        const uint8_t *src[4] = {c0 + 2 * j0 - bias, c0 + 2 * j1 - bias, c1 + 2 * j0 - bias, c1 + 2 * j1 - bias};
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            if constexpr (PAIR16) {                       // staged rows: the pair is 2-byte aligned, one 16-bit read
                const unsigned pr = *reinterpret_cast<const uint16_t *>(src[t]);
                q[t][0] = (float)(pr & 0xffu); q[t][1] = (float)(pr >> 8);
            } else {
                q[t][0] = (float)src[t][0]; q[t][1] = (float)src[t][1];
            }
        }
        const float cb = (1.f - wy) * ((1.f - wx) * q[0][0] + wx * q[1][0]) + wy * ((1.f - wx) * q[2][0] + wx * q[3][0]) - 128.f;
        const float cr = (1.f - wy) * ((1.f - wx) * q[0][1] + wx * q[1][1]) + wy * ((1.f - wx) * q[2][1] + wx * q[3][1]) - 128.f;
        const float yl = k.ky * ((float)row[x - bias] - k.y0);
        rgb[0] = fminf(fmaxf(yl + k.rv * cr, 0.f), 255.f);
        rgb[1] = fminf(fmaxf(yl - k.gu * cb - k.gv * cr, 0.f), 255.f);
        rgb[2] = fminf(fmaxf(yl + k.bu * cb, 0.f), 255.f);
    }
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

// blend of the four taps (the other ingest kernels' operation order) + normalisation
__device__ __forceinline__ void finish(const float (&a)[3], const float (&b)[3], const float (&c)[3], const float (&d)[3], float ly, float lx, const IngestP &p,
                                       float (&v)[3]) {
#pragma unroll
    for (int e = 0; e < 3; ++e)
        v[e] = ((1.f - ly) * ((1.f - lx) * a[e] + lx * b[e]) + ly * ((1.f - lx) * c[e] + lx * d[e])) * p.na[e] + p.nb[e];
}

// ------------------------------------------------------------------ per-pixel form: any shape, any alignment (odd RGB8 pitches, tiny frames)
template <bool NV12, int OUT>
__global__ __launch_bounds__(256) void frame_ingest_kernel(const IngestP p) {
    const long long total = (long long)p.N * p.h * p.w;
    const float sy = arseg_resize_scale(p.H, p.h, true), sx = arseg_resize_scale(p.W, p.w, true);
    const bool same = (p.h == p.H && p.w == p.W);
    for (long long pix = (long long)blockIdx.x * blockDim.x + threadIdx.x; pix < total; pix += (long long)gridDim.x * blockDim.x) {
        const int ox = (int)(pix % p.w), oy = (int)((pix / p.w) % p.h), n = (int)(pix / ((long long)p.w * p.h));
        const uint8_t *b0 = p.p0 + (size_t)n * p.ns0, *b1 = NV12 ? p.p1 + (size_t)n * p.ns1 : nullptr;
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
            if constexpr (NV12) chroma_pos(y, 0.25f, p.H >> 1, k0, k1, wy);
            const uint8_t *row = b0 + (size_t)y * p.pitch0, *c0 = NV12 ? b1 + (size_t)k0 * p.pitch1 : nullptr, *c1 = NV12 ? b1 + (size_t)k1 * p.pitch1 : nullptr;
            tap<NV12, false>(row, c0, c1, wy, x0, 0, p.W, p.k, t[2 * r]);
            if (!same) tap<NV12, false>(row, c0, c1, wy, x1, 0, p.W, p.k, t[2 * r + 1]);
        }
        if (same) {
#pragma unroll
            for (int e = 0; e < 3; ++e) v[e] = t[0][e] * p.na[e] + p.nb[e];
        } else {
            finish(t[0], t[1], t[2], t[3], ly, lx, p, v);
        }
        store_px<OUT>(p.out, (size_t)pix, v);
    }
}

// ------------------------------------------------------------------ row-staged form (the 8-bit twin of frame_to_nhwc8_rows_kernel, csrc/layers16.hip)
// One workgroup = 256 consecutive output pixels of one output row.  The source rows under it -- RGB8: the two rows; NV12: the two luma
// rows and the two chroma rows of each -- are staged in LDS over the x span of the 256 pixels with coalesced 4-byte loads (a per-pixel
// gather of 3-byte pixels / 2-byte chroma pairs is not), the taps come from there, every lane stores 16 bytes.  At identity size one
// row set is staged and one tap read.  Needs 4-byte aligned rows (plane pointers, pitches, image strides) and a horizontal scale <= 4.1.
constexpr int IN_SPAN = 1056;                    // staged source pixels per row: 255 * sx + 2 (+3 alignment, +3 chroma reach) <= IN_SPAN
template <bool NV12>
constexpr int stage_bytes() { return (NV12 ? IN_SPAN : 3 * IN_SPAN) + 16; }

template <bool NV12, int OUT>
__global__ __launch_bounds__(256) void frame_ingest_rows_kernel(const IngestP p) {
    constexpr int ROWS = NV12 ? 6 : 2, HALF = ROWS / 2, SB = stage_bytes<NV12>();
    __shared__ __attribute__((aligned(16))) uint8_t st[ROWS][SB];
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
    // staged byte window of a row: RGB8 bytes 3 xa .. 3 xe1 + 2;  NV12 bytes xa .. xe1 of the luma row and the chroma pairs of columns
    // xa / 2 .. xe1 / 2 + 1, i.e. bytes (xa & ~1) .. min(xe1 + 3, W - 1) of a chroma row (both kinds of row are W bytes long)
    const int row_bytes = NV12 ? p.W : 3 * p.W;
    const int bias = (NV12 ? xa : 3 * xa) & ~3;
    const int last = NV12 ? min(xe1 + 3, p.W - 1) : 3 * xe1 + 2;
    const int nch = (last - bias) / 4 + 1;                   // 4-byte chunks per staged row (<= SB / 4 by the host's span check)
    int ka0 = 0, ka1 = 0, kb0 = 0, kb1 = 0; float wya = 0.f, wyb = 0.f;          // chroma rows under y0 (a) and y1 (b)
    if constexpr (NV12) { chroma_pos(y0, 0.25f, p.H >> 1, ka0, ka1, wya); chroma_pos(y1, 0.25f, p.H >> 1, kb0, kb1, wyb); }
    const uint8_t *b0 = p.p0 + (size_t)n * p.ns0, *b1 = NV12 ? p.p1 + (size_t)n * p.ns1 : nullptr;
    const int rows = same ? HALF : ROWS;
    for (int i = threadIdx.x; i < rows * nch; i += 256) {
        const int r = i / nch, ch = i - r * nch, set = r / HALF, sub = r - set * HALF;          // sub 0: RGB / luma row, 1 / 2: chroma rows
        const int kr = set ? (sub == 1 ? kb0 : kb1) : (sub == 1 ? ka0 : ka1);
        const uint8_t *g = sub == 0 ? b0 + (size_t)(set ? y1 : y0) * p.pitch0 : b1 + (size_t)kr * p.pitch1;
        const int off = bias + 4 * ch;
        unsigned v = 0;
        if (off + 4 <= row_bytes) {
            v = *reinterpret_cast<const unsigned *>(g + off);
        } else {                                             // the row's last, partial chunk: never read past the row
            for (int b = 0; b < 4; ++b)
                if (off + b < row_bytes) v |= (unsigned)g[off + b] << (8 * b);
        }
        *reinterpret_cast<unsigned *>(&st[r][4 * ch]) = v;
    }
    __syncthreads();
    const int ox = ox0 + threadIdx.x;
    if (ox < p.w) {
        float t[4][3], v[3];
        if (same) {
            tap<NV12, true>(st[0], st[NV12 ? 1 : 0], st[NV12 ? 2 : 0], wya, ox, bias, p.W, p.k, t[0]);
#pragma unroll
            for (int e = 0; e < 3; ++e) v[e] = t[0][e] * p.na[e] + p.nb[e];
        } else {
            int x0, x1; float lx;
            ingest_src_index(sx, ox, p.W, x0, x1, lx);
#pragma unroll
            for (int r = 0; r < 2; ++r) {
                const uint8_t *row = st[r * HALF], *c0 = st[NV12 ? r * HALF + 1 : 0], *c1 = st[NV12 ? r * HALF + 2 : 0];
                tap<NV12, true>(row, c0, c1, r ? wyb : wya, x0, bias, p.W, p.k, t[2 * r]);
                tap<NV12, true>(row, c0, c1, r ? wyb : wya, x1, bias, p.W, p.k, t[2 * r + 1]);
            }
            finish(t[0], t[1], t[2], t[3], ly, lx, p, v);
        }
        store_px<OUT>(p.out, ((size_t)n * p.h + oy) * p.w + ox, v);
    }
}

template <bool NV12, int OUT>
int launch_ingest(const IngestP &p, bool staged, hipStream_t st) {
    if (staged) hipLaunchKernelGGL((frame_ingest_rows_kernel<NV12, OUT>), dim3((unsigned)(p.N * p.h * p.segs)), dim3(256), 0, st, p);
    else hipLaunchKernelGGL((frame_ingest_kernel<NV12, OUT>), dim3(arseg_grid_for((long long)p.N * p.h * p.w)), dim3(256), 0, st, p);
    return arseg_launch_status();
}
template <bool NV12>
int launch_ingest_dt(const IngestP &p, int out_dtype, bool staged, hipStream_t st) {
    return out_dtype == ARSEG_DT_F32 ? launch_ingest<NV12, ARSEG_DT_F32>(p, staged, st)
         : out_dtype == ARSEG_DT_F16 ? launch_ingest<NV12, ARSEG_DT_F16>(p, staged, st) : launch_ingest<NV12, ARSEG_DT_BF16>(p, staged, st);
}

// ================================================================== planar 4:2:0 and 10-bit sources (arseg_frame_ingest_yuv_fwd)
// I420 / P010 / I010: the two kernel shapes above, generalised over the source side -- plane count, sample width, code extraction.  The
// colour contract gains a bit depth n: chroma is interpolated on the stored codes, then Y8 = code cs, C8 - 128 = (code - 2^(n-1)) cs with
// cs = 2^-(n-8) (limited range) or 255 / (2^n - 1) (full range), then the matrix of COLOURS.  Every floating-point expression of this family
// sits in a function under `fp contract(off)`, the fused operations that belong to the contract are explicit __builtin_fmaf (the tap weight
// in ingest_src_index, the normalisation): equal sample values give equal fp32 bits in all eighteen instantiations.  (chroma_pos multiplies
// by 0.5 and subtracts: exact with or without contraction.)
template <int FMT> struct Src;
template <> struct Src<ARSEG_SRC_I420> {
    typedef uint8_t T; static constexpr bool PLANAR = true;
    static __device__ __forceinline__ unsigned code(unsigned s) { return s; }
};
template <> struct Src<ARSEG_SRC_P010> {
    typedef uint16_t T; static constexpr bool PLANAR = false;
    static __device__ __forceinline__ unsigned code(unsigned s) { return s >> 6; }
};
template <> struct Src<ARSEG_SRC_I010> {
    typedef uint16_t T; static constexpr bool PLANAR = true;
    static __device__ __forceinline__ unsigned code(unsigned s) { return s & 0x3ffu; }
};

struct YuvP {
    const uint8_t *p0, *p1, *p2;     // luma; Cb (planar) or interleaved (Cb, Cr) (P010); Cr (planar only)
    void *out;
    long long pitch0, pitch1, pitch2, ns0, ns1, ns2;      // bytes per row / per image of each plane
    int N, H, W, h, w, segs;
    float na[3], nb[3];
    float cs, cmid;                  // code -> 8-bit scale, chroma centre code 2^(n-1)
    ColourK k;
};

// stored codes of one tap (luma, the 2 x 2 chroma neighbourhood q[row 0 | 1, column j0 | j1][Cb, Cr]) -> RGB in the 0-255 scale
__device__ __forceinline__ void yuv_rgb(float yc, const float (&q)[4][2], float wy, float wx, const YuvP &p, float (&rgb)[3]) {
#pragma clang fp contract(off)
    const float cb = (((1.f - wy) * ((1.f - wx) * q[0][0] + wx * q[1][0]) + wy * ((1.f - wx) * q[2][0] + wx * q[3][0])) - p.cmid) * p.cs;
    const float cr = (((1.f - wy) * ((1.f - wx) * q[0][1] + wx * q[1][1]) + wy * ((1.f - wx) * q[2][1] + wx * q[3][1])) - p.cmid) * p.cs;
    const float yl = p.k.ky * (yc * p.cs - p.k.y0);
    rgb[0] = fminf(fmaxf(yl + p.k.rv * cr, 0.f), 255.f);
    rgb[1] = fminf(fmaxf(yl - p.k.gu * cb - p.k.gv * cr, 0.f), 255.f);
    rgb[2] = fminf(fmaxf(yl + p.k.bu * cb, 0.f), 255.f);
}

// blend of the four taps, then the normalisation as ONE fma
__device__ __forceinline__ void yuv_finish(const float (&a)[3], const float (&b)[3], const float (&c)[3], const float (&d)[3], float ly, float lx,
                                           const YuvP &p, float (&v)[3]) {
#pragma clang fp contract(off)
#pragma unroll
    for (int e = 0; e < 3; ++e)
        v[e] = __builtin_fmaf((1.f - ly) * ((1.f - lx) * a[e] + lx * b[e]) + ly * ((1.f - lx) * c[e] + lx * d[e]), p.na[e], p.nb[e]);
}
__device__ __forceinline__ void yuv_norm(const float (&a)[3], const YuvP &p, float (&v)[3]) {
#pragma unroll
    for (int e = 0; e < 3; ++e) v[e] = __builtin_fmaf(a[e], p.na[e], p.nb[e]);
}

// One tap of source pixel x.  `row` = its luma row; cb0 / cb1 (cr0 / cr1) = the two Cb (Cr) rows under it, wy the weight of the second; for
// P010 the Cr rows are the Cb rows + 2 bytes (unused when STAGED: the pair is one aligned 32-bit LDS read).  Luma pointers are already
// shifted so that byte index 0 is byte bias_l of the full row, chroma pointers byte bias_c.
template <int FMT, bool STAGED>
__device__ __forceinline__ void yuv_tap(const uint8_t *row, const uint8_t *cb0, const uint8_t *cb1, const uint8_t *cr0, const uint8_t *cr1, float wy, int x,
                                        int bias_l, int bias_c, const YuvP &p, float (&rgb)[3]) {
    using S = Src<FMT>;
    using T = typename S::T;
    constexpr int B = (int)sizeof(T), CE = S::PLANAR ? B : 2 * B;          // bytes per luma sample / per chroma column of a chroma row
    int j0, j1; float wx;
    chroma_pos(x, 0.f, p.W >> 1, j0, j1, wx);
    const int o0 = CE * j0 - bias_c, o1 = CE * j1 - bias_c;
    float q[4][2];
    if constexpr (!S::PLANAR && STAGED) {
        const uint8_t *src[4] = {cb0 + o0, cb0 + o1, cb1 + o0, cb1 + o1};
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const unsigned pr = *reinterpret_cast<const unsigned *>(src[t]);
            q[t][0] = (float)S::code(pr & 0xffffu); q[t][1] = (float)S::code(pr >> 16);
        }
    } else {
        auto ld = [](const uint8_t *g) { return (float)S::code(*reinterpret_cast<const T *>(g)); };
        q[0][0] = ld(cb0 + o0); q[1][0] = ld(cb0 + o1); q[2][0] = ld(cb1 + o0); q[3][0] = ld(cb1 + o1);
        q[0][1] = ld(cr0 + o0); q[1][1] = ld(cr0 + o1); q[2][1] = ld(cr1 + o0); q[3][1] = ld(cr1 + o1);
    }
    const float yc = (float)S::code(*reinterpret_cast<const T *>(row + B * x - bias_l));
    yuv_rgb(yc, q, wy, wx, p, rgb);
}

// ---- per-pixel form: any shape, any alignment the entry point admits
template <int FMT, int OUT>
__global__ __launch_bounds__(256) void yuv_ingest_kernel(const YuvP p) {
    using S = Src<FMT>;
    const long long total = (long long)p.N * p.h * p.w;
    const float sy = arseg_resize_scale(p.H, p.h, true), sx = arseg_resize_scale(p.W, p.w, true);
    const bool same = (p.h == p.H && p.w == p.W);
    const long long cpitch = S::PLANAR ? p.pitch2 : p.pitch1;             // pitch of the rows the Cr samples sit in
    for (long long pix = (long long)blockIdx.x * blockDim.x + threadIdx.x; pix < total; pix += (long long)gridDim.x * blockDim.x) {
        const int ox = (int)(pix % p.w), oy = (int)((pix / p.w) % p.h), n = (int)(pix / ((long long)p.w * p.h));
        const uint8_t *b0 = p.p0 + (size_t)n * p.ns0, *b1 = p.p1 + (size_t)n * p.ns1;
        const uint8_t *b2 = S::PLANAR ? p.p2 + (size_t)n * p.ns2 : b1 + sizeof(typename S::T);
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
            int k0, k1; float wy;
            chroma_pos(y, 0.25f, p.H >> 1, k0, k1, wy);
            const uint8_t *row = b0 + (size_t)y * p.pitch0, *cb0 = b1 + (size_t)k0 * p.pitch1, *cb1 = b1 + (size_t)k1 * p.pitch1;
            const uint8_t *cr0 = b2 + (size_t)k0 * cpitch, *cr1 = b2 + (size_t)k1 * cpitch;
            yuv_tap<FMT, false>(row, cb0, cb1, cr0, cr1, wy, x0, 0, 0, p, t[2 * r]);
            if (!same) yuv_tap<FMT, false>(row, cb0, cb1, cr0, cr1, wy, x1, 0, 0, p, t[2 * r + 1]);
        }
        if (same) yuv_norm(t[0], p, v);
        else yuv_finish(t[0], t[1], t[2], t[3], ly, lx, p, v);
        store_px<OUT>(p.out, (size_t)pix, v);
    }
}

// ---- row-staged form.  One workgroup = 256 consecutive output pixels of one output row.  Per source row under it (two; one at identity
// size) LDS holds the luma row over the pixels' x span and its chroma rows over columns xa / 2 .. xe1 / 2 + 1: planar Cb k0, Cb k1, Cr k0,
// Cr k1; P010 the two interleaved rows.  Coalesced 4-byte loads, taps from LDS, 16-byte stores.  Needs 4-byte aligned plane pointers,
// pitches and image strides and the horizontal-scale limit of IN_SPAN.
template <int FMT>
struct YuvStage {
    using S = Src<FMT>;
    static constexpr int B = (int)sizeof(typename S::T), CE = S::PLANAR ? B : 2 * B, NC = S::PLANAR ? 4 : 2;
    static constexpr int LB = B * IN_SPAN + 16;                            // luma row: <= B (IN_SPAN - 6) bytes + alignment
    static constexpr int CB = S::PLANAR ? B * (IN_SPAN / 2) + 16 : LB;     // chroma row: <= IN_SPAN / 2 - 1 columns of CE bytes + alignment
    static constexpr int SET = LB + NC * CB;
};

template <int FMT, int OUT>
__global__ __launch_bounds__(256) void yuv_ingest_rows_kernel(const YuvP p) {
    using S = Src<FMT>;
    using G = YuvStage<FMT>;
    constexpr int B = G::B, CE = G::CE, NC = G::NC, LB = G::LB, CB = G::CB, SET = G::SET;
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
    const int lrow = B * p.W, crow = CE * W2;                                          // bytes of a luma / chroma row
    const int bias_l = (B * xa) & ~3, bias_c = (CE * ca) & ~3;
    const int nl = (B * xe1 + B - 1 - bias_l) / 4 + 1, nc = (CE * cl + CE - 1 - bias_c) / 4 + 1;          // 4-byte chunks (<= LB / 4, CB / 4)
    int ka0, ka1, kb0, kb1; float wya, wyb;                                            // chroma rows under y0 (a) and y1 (b)
    chroma_pos(y0, 0.25f, p.H >> 1, ka0, ka1, wya);
    chroma_pos(y1, 0.25f, p.H >> 1, kb0, kb1, wyb);
    const uint8_t *b0 = p.p0 + (size_t)n * p.ns0, *b1 = p.p1 + (size_t)n * p.ns1, *b2 = S::PLANAR ? p.p2 + (size_t)n * p.ns2 : nullptr;
    const int per = nl + NC * nc, total = (same ? 1 : 2) * per;
    for (int i = threadIdx.x; i < total; i += 256) {
        const int set = i >= per ? 1 : 0;
        int j = i - set * per, off, rb, lo = set * SET;
        const uint8_t *g;
        if (j < nl) {
            g = b0 + (size_t)(set ? y1 : y0) * p.pitch0; off = bias_l + 4 * j; rb = lrow; lo += 4 * j;
        } else {
            j -= nl;
            const int sub = j / nc, ch = j - sub * nc;                                 // sub: Cb k0, Cb k1, Cr k0, Cr k1 (planar) | k0, k1 (P010)
            const int kr = (sub & 1) ? (set ? kb1 : ka1) : (set ? kb0 : ka0);
            const bool third = S::PLANAR && sub >= 2;
            g = (third ? b2 : b1) + (size_t)kr * (third ? p.pitch2 : p.pitch1); off = bias_c + 4 * ch; rb = crow; lo += LB + sub * CB + 4 * ch;
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
            yuv_tap<FMT, true>(st, c, c + CB, c + (NC - 2) * CB, c + (NC - 1) * CB, wya, ox, bias_l, bias_c, p, t[0]);
            yuv_norm(t[0], p, v);
        } else {
            int x0, x1; float lx;
            ingest_src_index(sx, ox, p.W, x0, x1, lx);
#pragma unroll
            for (int r = 0; r < 2; ++r) {
                const uint8_t *row = st + r * SET, *cr = c + r * SET;
                yuv_tap<FMT, true>(row, cr, cr + CB, cr + (NC - 2) * CB, cr + (NC - 1) * CB, r ? wyb : wya, x0, bias_l, bias_c, p, t[2 * r]);
                yuv_tap<FMT, true>(row, cr, cr + CB, cr + (NC - 2) * CB, cr + (NC - 1) * CB, r ? wyb : wya, x1, bias_l, bias_c, p, t[2 * r + 1]);
            }
            yuv_finish(t[0], t[1], t[2], t[3], ly, lx, p, v);
        }
        store_px<OUT>(p.out, ((size_t)n * p.h + oy) * p.w + ox, v);
    }
}

template <int FMT, int OUT>
int launch_yuv(const YuvP &p, bool staged, hipStream_t st) {
    if (staged) hipLaunchKernelGGL((yuv_ingest_rows_kernel<FMT, OUT>), dim3((unsigned)(p.N * p.h * p.segs)), dim3(256), 0, st, p);
    else hipLaunchKernelGGL((yuv_ingest_kernel<FMT, OUT>), dim3(arseg_grid_for((long long)p.N * p.h * p.w)), dim3(256), 0, st, p);
    return arseg_launch_status();
}
template <int FMT>
int launch_yuv_dt(const YuvP &p, int out_dtype, bool staged, hipStream_t st) {
    return out_dtype == ARSEG_DT_F32 ? launch_yuv<FMT, ARSEG_DT_F32>(p, staged, st)
         : out_dtype == ARSEG_DT_F16 ? launch_yuv<FMT, ARSEG_DT_F16>(p, staged, st) : launch_yuv<FMT, ARSEG_DT_BF16>(p, staged, st);
}

}  // namespace

extern "C" int arseg_frame_ingest_yuv_fwd(const void *plane0, const void *plane1, const void *plane2, int src_format, int64_t pitch0, int64_t pitch1,
                                          int64_t pitch2, int64_t n_stride0, int64_t n_stride1, int64_t n_stride2, int colour, void *out, int out_dtype,
                                          int N, int H, int W, int h, int w, const float *mean3, const float *std3, arseg_stream_t stream) {
    if (src_format != ARSEG_SRC_I420 && src_format != ARSEG_SRC_P010 && src_format != ARSEG_SRC_I010) return ARSEG_EINVAL;
    const bool planar = src_format != ARSEG_SRC_P010, wide = src_format != ARSEG_SRC_I420;
    ARSEG_CHECK_PTR(plane0); ARSEG_CHECK_PTR(plane1); ARSEG_CHECK_PTR(out); ARSEG_CHECK_PTR(mean3); ARSEG_CHECK_PTR(std3);
    if (planar) ARSEG_CHECK_PTR(plane2);
    ARSEG_CHECK_POS(N); ARSEG_CHECK_POS(H); ARSEG_CHECK_POS(W); ARSEG_CHECK_POS(h); ARSEG_CHECK_POS(w);
    if ((H & 1) || (W & 1)) return ARSEG_EINVAL;
    if (out_dtype != ARSEG_DT_F32 && out_dtype != ARSEG_DT_F16 && out_dtype != ARSEG_DT_BF16) return ARSEG_EINVAL;
    if (colour < 0 || colour > ARSEG_COLOUR_BT709_FULL) return ARSEG_EINVAL;
    if (std3[0] == 0.f || std3[1] == 0.f || std3[2] == 0.f || !ARSEG_ALIGNED16(out)) return ARSEG_EINVAL;
    const int64_t lrow = (wide ? 2 : 1) * (int64_t)W, crow = planar ? lrow / 2 : lrow;          // bytes of a luma / chroma row
    if (pitch0 < lrow || pitch1 < crow || n_stride0 < 0 || n_stride1 < 0) return ARSEG_EINVAL;
    if (planar && (pitch2 < crow || n_stride2 < 0)) return ARSEG_EINVAL;
    auto al = [](const void *q, int64_t a, int64_t b, unsigned m) { return ((reinterpret_cast<uintptr_t>(q) | (uintptr_t)a | (uintptr_t)b) & m) == 0; };
    if (wide && !(al(plane0, pitch0, n_stride0, 1u) && al(plane1, pitch1, n_stride1, 1u) && (!planar || al(plane2, pitch2, n_stride2, 1u)))) return ARSEG_EINVAL;
    YuvP p;
    p.p0 = (const uint8_t *)plane0; p.p1 = (const uint8_t *)plane1; p.p2 = planar ? (const uint8_t *)plane2 : nullptr; p.out = out;
    p.pitch0 = pitch0; p.pitch1 = pitch1; p.pitch2 = planar ? pitch2 : 0; p.ns0 = n_stride0; p.ns1 = n_stride1; p.ns2 = planar ? n_stride2 : 0;
    p.N = N; p.H = H; p.W = W; p.h = h; p.w = w; p.segs = arseg_cdiv(w, 256);
    for (int c = 0; c < 3; ++c) {
        p.na[c] = (float)(1.0 / (255.0 * (double)std3[c]));
        p.nb[c] = (float)(-(double)mean3[c] / (double)std3[c]);
    }
    p.k = COLOURS[colour];
    const bool full = colour == ARSEG_COLOUR_BT601_FULL || colour == ARSEG_COLOUR_BT709_FULL;
    p.cs = !wide ? 1.f : full ? (float)(255.0 / 1023.0) : 0.25f;
    p.cmid = wide ? 512.f : 128.f;
    const float sx = arseg_resize_scale(W, w, true);
    const bool staged = al(plane0, pitch0, n_stride0, 3u) && al(plane1, pitch1, n_stride1, 3u) && (!planar || al(plane2, pitch2, n_stride2, 3u)) && W >= 8 &&
                        255.f * sx + 8.f <= (float)IN_SPAN && (long long)N * h * p.segs < (1ll << 31);
    hipStream_t st = arseg_stream(stream);
    return src_format == ARSEG_SRC_I420 ? launch_yuv_dt<ARSEG_SRC_I420>(p, out_dtype, staged, st)
         : src_format == ARSEG_SRC_P010 ? launch_yuv_dt<ARSEG_SRC_P010>(p, out_dtype, staged, st) : launch_yuv_dt<ARSEG_SRC_I010>(p, out_dtype, staged, st);
}

extern "C" int arseg_frame_ingest_fwd(const void *plane0, const void *plane1, int src_format, int64_t pitch0, int64_t pitch1, int64_t n_stride0,
                                      int64_t n_stride1, int colour, void *out, int out_dtype, int N, int H, int W, int h, int w, const float *mean3,
                                      const float *std3, arseg_stream_t stream) {
    ARSEG_CHECK_PTR(plane0); ARSEG_CHECK_PTR(out); ARSEG_CHECK_PTR(mean3); ARSEG_CHECK_PTR(std3);
    ARSEG_CHECK_POS(N); ARSEG_CHECK_POS(H); ARSEG_CHECK_POS(W); ARSEG_CHECK_POS(h); ARSEG_CHECK_POS(w);
    if (src_format != ARSEG_SRC_RGB8 && src_format != ARSEG_SRC_NV12) return ARSEG_EINVAL;
    if (out_dtype != ARSEG_DT_F32 && out_dtype != ARSEG_DT_F16 && out_dtype != ARSEG_DT_BF16) return ARSEG_EINVAL;
    if (std3[0] == 0.f || std3[1] == 0.f || std3[2] == 0.f || !ARSEG_ALIGNED16(out)) return ARSEG_EINVAL;
    const bool nv12 = src_format == ARSEG_SRC_NV12;
    if (pitch0 < (nv12 ? (int64_t)W : 3 * (int64_t)W) || n_stride0 < 0) return ARSEG_EINVAL;
    if (nv12) {
        ARSEG_CHECK_PTR(plane1);
        if ((H & 1) || (W & 1) || pitch1 < (int64_t)W || n_stride1 < 0) return ARSEG_EINVAL;
        if (colour < 0 || colour > ARSEG_COLOUR_BT709_FULL) return ARSEG_EINVAL;
    }
    IngestP p;
    p.p0 = (const uint8_t *)plane0; p.p1 = nv12 ? (const uint8_t *)plane1 : nullptr; p.out = out;
    p.pitch0 = pitch0; p.pitch1 = nv12 ? pitch1 : 0; p.ns0 = n_stride0; p.ns1 = nv12 ? n_stride1 : 0;
    p.N = N; p.H = H; p.W = W; p.h = h; p.w = w; p.segs = arseg_cdiv(w, 256);
    for (int c = 0; c < 3; ++c) {
        p.na[c] = (float)(1.0 / (255.0 * (double)std3[c]));
        p.nb[c] = (float)(-(double)mean3[c] / (double)std3[c]);
    }
    p.k = COLOURS[nv12 ? colour : 0];
    auto al4 = [](const void *q, int64_t a, int64_t b) { return ((reinterpret_cast<uintptr_t>(q) | (uintptr_t)a | (uintptr_t)b) & 3u) == 0; };
    const float sx = arseg_resize_scale(W, w, true);
    const bool staged = al4(plane0, pitch0, n_stride0) && (!nv12 || al4(plane1, pitch1, n_stride1)) && W >= 8 && 255.f * sx + 8.f <= (float)IN_SPAN &&
                        (long long)N * h * p.segs < (1ll << 31);
    hipStream_t st = arseg_stream(stream);
    return nv12 ? launch_ingest_dt<true>(p, out_dtype, staged, st) : launch_ingest_dt<false>(p, out_dtype, staged, st);
}
