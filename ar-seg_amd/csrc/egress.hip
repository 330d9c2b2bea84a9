// Segmentation egress (include/arseg_hip.h, arseg_segment_egress_fwd): head logits in, what a deployed segmenter hands on out -- an 8-bit
// label plane (optionally through a train-id -> label-id table) and / or the frame with the classes painted over it in the decoder's own
// 8-bit plane format (RGB8, NV12, I420) -- in one launch for N frames.  The bilinear resize and the argmax are the evaluator tail's
// (arseg_label_pixel / arseg_label_run, arseg_device.h: one definition, so labels8 equals arseg_argmax_confusion_fwd's pred on all three
// routes); nothing of full-resolution size besides the outputs is written, and the int32 labels never exist.
//
// Thread ownership.  A thread reads every destination sample it writes from the source first and writes it exactly once, so a destination
// plane may be its source plane.  RGB8 / labels only: one pixel (per-pixel routes) or one run of S pixels (run route) of one row.  4:2:0:
// whole 2 x 2 luma blocks with their chroma sample -- one block (per-pixel routes), the S/2 blocks under a run on two rows (x4, x8: a run
// starts at S j + S/2, an even column), or for x2, whose runs start at odd columns, the aligned block [2c, 2c+2) with each pixel evaluated
// by its own run (c-1 for the left column, c for the right one: the formula is arseg_label_run's, unchanged).
// Stores are assembled per thread into 2- to 8-byte accesses where the address allows it (span_store, arseg_device.h); a byte per lane only on planes whose
// pointers or pitches are odd, or where a lane owns a single sample.
#include "arseg_device.h"

namespace {

constexpr int FMT_NONE = -1;          // labels only; otherwise enum arseg_src_format (RGB8, NV12, I420)

struct EgressP {
    const float *logits;
    uint8_t *lab;
    const uint8_t *s[3];
    uint8_t *d[3];
    long long lab_pitch, lab_ns, sp[3], sn[3], dp[3], dn[3];          // bytes per row / per image
    int N, n_cls, h, w, H, W, align;
    unsigned tab[32];                 // per class: P[k][0] | P[k][1] << 8 | P[k][2] << 16 | (lut ? lut[k] : k) << 24
    unsigned short wt[32];            // per class: a_k, 0 .. 256
};

__device__ __forceinline__ unsigned blend8(unsigned src, unsigned code, unsigned a) { return (src * (256u - a) + code * a + 128u) >> 8; }

// NC columns from ox on output row oy of frame n (4:2:0: rows oy and oy + 1, oy, ox and NC even), classes k0[c] (row oy) and k1[c] (row
// oy + 1): the label bytes and / or the painted samples.  Every sample is loaded, blended and stored by this thread alone.
template <int FMT, int NC>
__device__ __forceinline__ void paint(const EgressP &p, const uint2 *tab, int n, int oy, int ox, const int *k0, const int *k1) {
    constexpr bool YUV = FMT == ARSEG_SRC_NV12 || FMT == ARSEG_SRC_I420;
    static_assert(!YUV || NC % 2 == 0, "4:2:0 needs whole 2 x 2 blocks");
    uint2 e0[NC], e1[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) { e0[c] = tab[k0[c]]; e1[c] = YUV ? tab[k1[c]] : e0[c]; }
    if (p.lab) {
        unsigned v[NC];
        uint8_t *g = p.lab + (size_t)n * p.lab_ns + (size_t)oy * p.lab_pitch + ox;
#pragma unroll
        for (int c = 0; c < NC; ++c) v[c] = e0[c].x >> 24;
        span_store<NC>(g, v);
        if constexpr (YUV) {
#pragma unroll
            for (int c = 0; c < NC; ++c) v[c] = e1[c].x >> 24;
            span_store<NC>(g + p.lab_pitch, v);
        }
    }
    if constexpr (FMT == ARSEG_SRC_RGB8) {
        unsigned v[3 * NC];
        span_load<3 * NC>(p.s[0] + (size_t)n * p.sn[0] + (size_t)oy * p.sp[0] + 3 * (size_t)ox, v);
#pragma unroll
        for (int c = 0; c < NC; ++c)
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) v[3 * c + ch] = blend8(v[3 * c + ch], (e0[c].x >> (8 * ch)) & 0xffu, e0[c].y);
        span_store<3 * NC>(p.d[0] + (size_t)n * p.dn[0] + (size_t)oy * p.dp[0] + 3 * (size_t)ox, v);
    } else if constexpr (YUV) {
        unsigned y0[NC], y1[NC];
        const uint8_t *sl = p.s[0] + (size_t)n * p.sn[0] + (size_t)oy * p.sp[0] + ox;
        span_load<NC>(sl, y0);
        span_load<NC>(sl + p.sp[0], y1);
        // chroma sample cc of the span sits under columns 2 cc, 2 cc + 1 of both rows: A = sum of the four weights, per component
        // C' = (C (1024 - A) + sum a_i P[k_i][c] + 512) >> 10
        unsigned A[NC / 2], sb[NC / 2], sr[NC / 2];
#pragma unroll
        for (int cc = 0; cc < NC / 2; ++cc) {
            const uint2 q[4] = {e0[2 * cc], e0[2 * cc + 1], e1[2 * cc], e1[2 * cc + 1]};
            A[cc] = 0; sb[cc] = 512u; sr[cc] = 512u;
#pragma unroll
            for (int i = 0; i < 4; ++i) { A[cc] += q[i].y; sb[cc] += q[i].y * ((q[i].x >> 8) & 0xffu); sr[cc] += q[i].y * ((q[i].x >> 16) & 0xffu); }
        }
        const size_t cy = (size_t)(oy >> 1);
        if constexpr (FMT == ARSEG_SRC_NV12) {          // (Cb, Cr) pairs: byte offset 2 (ox / 2) = ox
            unsigned c[NC];
            span_load<NC>(p.s[1] + (size_t)n * p.sn[1] + cy * p.sp[1] + ox, c);
#pragma unroll
            for (int cc = 0; cc < NC / 2; ++cc) {
                c[2 * cc] = (c[2 * cc] * (1024u - A[cc]) + sb[cc]) >> 10;
                c[2 * cc + 1] = (c[2 * cc + 1] * (1024u - A[cc]) + sr[cc]) >> 10;
            }
            span_store<NC>(p.d[1] + (size_t)n * p.dn[1] + cy * p.dp[1] + ox, c);
        } else {
            unsigned cb[NC / 2], cr[NC / 2];
            span_load<NC / 2>(p.s[1] + (size_t)n * p.sn[1] + cy * p.sp[1] + (ox >> 1), cb);
            span_load<NC / 2>(p.s[2] + (size_t)n * p.sn[2] + cy * p.sp[2] + (ox >> 1), cr);
#pragma unroll
            for (int cc = 0; cc < NC / 2; ++cc) {
                cb[cc] = (cb[cc] * (1024u - A[cc]) + sb[cc]) >> 10;
                cr[cc] = (cr[cc] * (1024u - A[cc]) + sr[cc]) >> 10;
            }
            span_store<NC / 2>(p.d[1] + (size_t)n * p.dn[1] + cy * p.dp[1] + (ox >> 1), cb);
            span_store<NC / 2>(p.d[2] + (size_t)n * p.dn[2] + cy * p.dp[2] + (ox >> 1), cr);
        }
#pragma unroll
        for (int c = 0; c < NC; ++c) { y0[c] = blend8(y0[c], e0[c].x & 0xffu, e0[c].y); y1[c] = blend8(y1[c], e1[c].x & 0xffu, e1[c].y); }
        uint8_t *dl = p.d[0] + (size_t)n * p.dn[0] + (size_t)oy * p.dp[0] + ox;
        span_store<NC>(dl, y0);
        span_store<NC>(dl + p.dp[0], y1);
    }
}

// the per-class table of the launch: kernel arguments -> LDS (indexed by a per-lane class afterwards)
__device__ __forceinline__ void stage_table(const EgressP &p, uint2 *tab) {
    if (threadIdx.x < 32) tab[threadIdx.x] = uint2{p.tab[threadIdx.x], (unsigned)p.wt[threadIdx.x]};
    __syncthreads();
}

// ------------------------------------------------------------------ per-pixel routes: h == H && w == W, or any bilinear resize
template <int FMT>
__global__ __launch_bounds__(256) void egress_pixel_kernel(const EgressP p) {
    constexpr bool YUV = FMT == ARSEG_SRC_NV12 || FMT == ARSEG_SRC_I420;
    constexpr int B = YUV ? 2 : 1;                  // a thread owns a B x B block of pixels
    __shared__ uint2 tab[32];
    stage_table(p, tab);
    const int Hb = p.H / B, Wb = p.W / B;
    const long long total = (long long)p.N * Hb * Wb;
    const float sy = arseg_resize_scale(p.h, p.H, p.align != 0), sx = arseg_resize_scale(p.w, p.W, p.align != 0);
    const bool same = (p.h == p.H && p.w == p.W);
    for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long long)gridDim.x * blockDim.x) {
        const int bx = (int)(idx % Wb), by = (int)((idx / Wb) % Hb), n = (int)(idx / ((long long)Wb * Hb));
        int k0[B], k1[B];
#pragma unroll
        for (int c = 0; c < B; ++c) {
            k0[c] = arseg_label_pixel(p.logits, n, B * by, B * bx + c, p.n_cls, p.h, p.w, p.align, same, sy, sx);
            k1[c] = YUV ? arseg_label_pixel(p.logits, n, B * by + 1, B * bx + c, p.n_cls, p.h, p.w, p.align, same, sy, sx) : 0;
        }
        paint<FMT, B>(p, tab, n, B * by, B * bx, k0, k1);
    }
}

// ------------------------------------------------------------------ run route: exact x S upsample, align_corners == 0, S = 2 | 4 | 8
template <int S, int FMT>
__global__ __launch_bounds__(256) void egress_run_kernel(const EgressP p) {
    constexpr bool YUV = FMT == ARSEG_SRC_NV12 || FMT == ARSEG_SRC_I420;
    constexpr int B = YUV ? 2 : 1;                  // output rows per thread
    __shared__ uint2 tab[32];
    stage_table(p, tab);
    const int H = S * p.h, W = S * p.w, Hb = H / B;
    const float sc = arseg_resize_scale(p.h, H, false);          // = 1 / S exactly
    if constexpr (YUV && S == 2) {
        // runs start at odd columns: a thread owns the aligned block [2c, 2c+2) and takes each column from its own run
        const long long total = (long long)p.N * Hb * p.w;
        for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long long)gridDim.x * blockDim.x) {
            const int c = (int)(idx % p.w), by = (int)((idx / p.w) % Hb), n = (int)(idx / ((long long)p.w * Hb));
            int ka[2], kb[2], k0[2], k1[2];
            arseg_label_run<2>(p.logits, sc, n, 2 * by, c - 1, p.n_cls, p.h, p.w, ka);
            arseg_label_run<2>(p.logits, sc, n, 2 * by, c, p.n_cls, p.h, p.w, kb);
            k0[0] = ka[1]; k0[1] = kb[0];
            arseg_label_run<2>(p.logits, sc, n, 2 * by + 1, c - 1, p.n_cls, p.h, p.w, ka);
            arseg_label_run<2>(p.logits, sc, n, 2 * by + 1, c, p.n_cls, p.h, p.w, kb);
            k1[0] = ka[1]; k1[1] = kb[0];
            paint<FMT, 2>(p, tab, n, 2 * by, 2 * c, k0, k1);
        }
    } else {
        const int runs = p.w + 1;
        const long long total = (long long)p.N * Hb * runs;
        for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long long)gridDim.x * blockDim.x) {
            const int j = (int)(idx % runs) - 1, by = (int)((idx / runs) % Hb), n = (int)(idx / ((long long)runs * Hb));
            int k0[S], k1[S];
            arseg_label_run<S>(p.logits, sc, n, B * by, j, p.n_cls, p.h, p.w, k0);
            if constexpr (YUV) arseg_label_run<S>(p.logits, sc, n, B * by + 1, j, p.n_cls, p.h, p.w, k1);
            const int xs = S * j + S / 2;               // the run's first column; the first and the last run hold S/2 pixels of the frame
            if (xs >= 0 && xs + S <= W) paint<FMT, S>(p, tab, n, B * by, xs, k0, k1);
            else if (xs < 0) paint<FMT, S / 2>(p, tab, n, B * by, 0, k0 + S / 2, k1 + S / 2);
            else paint<FMT, S / 2>(p, tab, n, B * by, xs, k0, k1);
        }
    }
}

template <int FMT>
int launch_egress(const EgressP &p, hipStream_t st) {
    constexpr int B = (FMT == ARSEG_SRC_NV12 || FMT == ARSEG_SRC_I420) ? 2 : 1;
    const int S = p.H / p.h;
    if (!p.align && S * p.h == p.H && S * p.w == p.W && (S == 2 || S == 4 || S == 8)) {          // the route choice of arseg_argmax_confusion_fwd
        const long long total = (long long)p.N * (p.H / B) * (B == 2 && S == 2 ? p.w : p.w + 1);
        const dim3 g(arseg_grid_for(total, 4096));
        if (S == 8) hipLaunchKernelGGL((egress_run_kernel<8, FMT>), g, dim3(256), 0, st, p);
        else if (S == 4) hipLaunchKernelGGL((egress_run_kernel<4, FMT>), g, dim3(256), 0, st, p);
        else hipLaunchKernelGGL((egress_run_kernel<2, FMT>), g, dim3(256), 0, st, p);
        return arseg_launch_status();
    }
    hipLaunchKernelGGL((egress_pixel_kernel<FMT>), dim3(arseg_grid_for((long long)p.N * (p.H / B) * (p.W / B), 1024)), dim3(256), 0, st, p);
    return arseg_launch_status();
}

}  // namespace

extern "C" int arseg_segment_egress_fwd(const float *logits, int N, int n_cls, int h, int w, int H, int W, int align_corners, const uint8_t *lut,
                                        uint8_t *labels8, int64_t labels_pitch, int64_t labels_n_stride, int format, const void *src0,
                                        const void *src1, const void *src2, int64_t src_pitch0, int64_t src_pitch1, int64_t src_pitch2,
                                        int64_t src_n_stride0, int64_t src_n_stride1, int64_t src_n_stride2, void *dst0, void *dst1, void *dst2,
                                        int64_t dst_pitch0, int64_t dst_pitch1, int64_t dst_pitch2, int64_t dst_n_stride0, int64_t dst_n_stride1,
                                        int64_t dst_n_stride2, const uint8_t *palette, const uint16_t *weights, arseg_stream_t stream) {
    ARSEG_CHECK_PTR(logits);
    if (!labels8 && !dst0) return ARSEG_EINVAL;
    ARSEG_CHECK_POS(N); ARSEG_CHECK_POS(n_cls); ARSEG_CHECK_POS(h); ARSEG_CHECK_POS(w); ARSEG_CHECK_POS(H); ARSEG_CHECK_POS(W);
    if (n_cls > 32) return ARSEG_EINVAL;
    if (labels8 && (labels_pitch < (int64_t)W || labels_n_stride < 0)) return ARSEG_EINVAL;
    EgressP p = {};
    int fmt = FMT_NONE;
    if (dst0) {
        if (!src0 || !palette || !weights) return ARSEG_EINVAL;
        if (format != ARSEG_SRC_RGB8 && format != ARSEG_SRC_NV12 && format != ARSEG_SRC_I420) return ARSEG_EINVAL;          // 10-bit: not covered
        fmt = format;
        for (int k = 0; k < n_cls; ++k)
            if (weights[k] > 256) return ARSEG_EINVAL;
        const int planes = fmt == ARSEG_SRC_RGB8 ? 1 : fmt == ARSEG_SRC_NV12 ? 2 : 3;
        if (planes > 1 && ((H & 1) || (W & 1))) return ARSEG_EINVAL;
        const void *s[3] = {src0, src1, src2};
        void *d[3] = {dst0, dst1, dst2};
        const int64_t sp[3] = {src_pitch0, src_pitch1, src_pitch2}, sn[3] = {src_n_stride0, src_n_stride1, src_n_stride2};
        const int64_t dp[3] = {dst_pitch0, dst_pitch1, dst_pitch2}, dn[3] = {dst_n_stride0, dst_n_stride1, dst_n_stride2};
        for (int i = 0; i < planes; ++i) {
            const int64_t row = fmt == ARSEG_SRC_RGB8 ? 3 * (int64_t)W : (i == 0 || fmt == ARSEG_SRC_NV12) ? (int64_t)W : (int64_t)W / 2;
            if (!s[i] || !d[i] || sp[i] < row || dp[i] < row || sn[i] < 0 || dn[i] < 0) return ARSEG_EINVAL;
            p.s[i] = (const uint8_t *)s[i]; p.d[i] = (uint8_t *)d[i];
            p.sp[i] = sp[i]; p.sn[i] = sn[i]; p.dp[i] = dp[i]; p.dn[i] = dn[i];
        }
    }
    p.logits = logits; p.lab = labels8; p.lab_pitch = labels8 ? labels_pitch : 0; p.lab_ns = labels8 ? labels_n_stride : 0;
    p.N = N; p.n_cls = n_cls; p.h = h; p.w = w; p.H = H; p.W = W; p.align = align_corners ? 1 : 0;
    for (int k = 0; k < n_cls; ++k) {
        const unsigned l = lut ? lut[k] : (unsigned)k;
        p.tab[k] = (l << 24) | (dst0 ? (unsigned)palette[3 * k] | ((unsigned)palette[3 * k + 1] << 8) | ((unsigned)palette[3 * k + 2] << 16) : 0u);
        p.wt[k] = dst0 ? weights[k] : (unsigned short)0;
    }
    hipStream_t st = arseg_stream(stream);
    return fmt == FMT_NONE ? launch_egress<FMT_NONE>(p, st) : fmt == ARSEG_SRC_RGB8 ? launch_egress<ARSEG_SRC_RGB8>(p, st)
         : fmt == ARSEG_SRC_NV12 ? launch_egress<ARSEG_SRC_NV12>(p, st) : launch_egress<ARSEG_SRC_I420>(p, st);
}
