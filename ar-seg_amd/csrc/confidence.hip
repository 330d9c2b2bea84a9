// Segmentation confidence (include/arseg_hip.h, arseg_segment_confidence_fwd): head logits in, how much to trust the frame out -- an 8-bit
// plane of the softmax's top-1 probability (or its margin over the runner-up) per output pixel, the label plane next to it, and per frame
// three integer statistics (sum of the codes, pixels below a threshold, pixels per class) -- in one launch for N frames and one pass over
// the logits.  The bilinear resize and the argmax are the evaluator tail's (arseg_label_pixel / arseg_label_run, arseg_device.h: one
// definition, so labels8 equals arseg_argmax_confusion_fwd's pred on all three routes); the softmax rides on the class loop of that rule as
// an accumulator (ArsegSoftmaxAcc: running maximum, rescaled sum, runner-up), so the taps are loaded once and neither probabilities nor a
// per-class array exist anywhere.
//
// Thread mapping: the tail's -- one pixel (per-pixel routes) or one run of S pixels (run route) of one row of one frame.  A workgroup works
// on one frame at a time (blockIdx.y strides over the frames), so its counters belong to one row of `stats`: every thread keeps its sum of
// codes and its low count in registers, a wave adds them up, the class areas are counted in LDS, and a workgroup issues one 64-bit vector
// atomic add per non-zero counter and frame.  All counters are integers: the result does not depend on the order of the atomics.
#include "arseg_device.h"

namespace {

struct ConfP {
    const float *logits;
    uint8_t *conf, *lab;
    unsigned long long *stats;                          // [N][ARSEG_CONF_NSTATS]
    long long conf_pitch, conf_ns, lab_pitch, lab_ns;   // bytes per row / per image
    int N, n_cls, h, w, H, W, align, margin, low;
    uint8_t lut[32];                                    // lut ? lut[k] : k
};

struct ConfLds {
    unsigned long long cnt[ARSEG_CONF_NSTATS];          // this workgroup's share of one row of stats
    unsigned lut[32];
};

__device__ __forceinline__ void conf_stage(const ConfP &p, ConfLds &s) {
    if (threadIdx.x < 32) s.lut[threadIdx.x] = p.lut[threadIdx.x];
    if (threadIdx.x < ARSEG_CONF_NSTATS) s.cnt[threadIdx.x] = 0;
    __syncthreads();
}

// NC columns from ox on output row oy of frame n: classes k[c], codes q[c] -> the two planes and the thread's / workgroup's counters
template <int NC>
__device__ __forceinline__ void conf_emit(const ConfP &p, ConfLds &s, int n, int oy, int ox, const int *k, const unsigned *q, unsigned long long &sum,
                                          unsigned long long &low) {
    if (p.conf) {
        unsigned v[NC];
#pragma unroll
        for (int c = 0; c < NC; ++c) v[c] = q[c];
        span_store<NC>(p.conf + (size_t)n * p.conf_ns + (size_t)oy * p.conf_pitch + ox, v);
    }
    if (p.lab) {
        unsigned v[NC];
#pragma unroll
        for (int c = 0; c < NC; ++c) v[c] = s.lut[k[c]];
        span_store<NC>(p.lab + (size_t)n * p.lab_ns + (size_t)oy * p.lab_pitch + ox, v);
    }
    if (p.stats) {
        unsigned qs = 0, ls = 0, len = 0;
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            qs += q[c]; ls += (int)q[c] < p.low ? 1u : 0u; ++len;
            // neighbours of a run mostly share their class: one LDS add per stretch of equal labels
            if (c == NC - 1 || k[c + 1] != k[c]) { atomicAdd(&s.cnt[2 + k[c]], (unsigned long long)len); len = 0; }
        }
        sum += qs; low += ls;
    }
}

// The frame is done for this workgroup: registers -> wave -> LDS -> one atomic per non-zero counter; the counters are cleared for the next frame.
__device__ __forceinline__ void conf_flush(ConfLds &s, unsigned long long *row, int n_cls, unsigned long long sum, unsigned long long low) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { sum += __shfl_xor(sum, o, 64); low += __shfl_xor(low, o, 64); }
    if ((threadIdx.x & 63) == 0) {
        if (sum) atomicAdd(&s.cnt[0], sum);
        if (low) atomicAdd(&s.cnt[1], low);
    }
    __syncthreads();
    if (threadIdx.x < 2 + n_cls) {
        const unsigned long long c = s.cnt[threadIdx.x];
        if (c) atomicAdd(&row[threadIdx.x], c);
        s.cnt[threadIdx.x] = 0;
    }
    __syncthreads();
}

// ------------------------------------------------------------------ per-pixel routes: h == H && w == W, or any bilinear resize
__global__ __launch_bounds__(256) void confidence_pixel_kernel(const ConfP p) {
    __shared__ ConfLds s;
    conf_stage(p, s);
    const long long total = (long long)p.H * p.W;
    const float sy = arseg_resize_scale(p.h, p.H, p.align != 0), sx = arseg_resize_scale(p.w, p.W, p.align != 0);
    const bool same = (p.h == p.H && p.w == p.W);
    for (int n = blockIdx.y; n < p.N; n += gridDim.y) {
        unsigned long long sum = 0, low = 0;
        for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long long)gridDim.x * blockDim.x) {
            const int ox = (int)(idx % p.W), oy = (int)(idx / p.W);
            ArsegSoftmaxAcc<1> acc;
            const int k = arseg_label_pixel(p.logits, n, oy, ox, p.n_cls, p.h, p.w, p.align, same, sy, sx, &acc);
            const unsigned q = acc.code(0, p.margin != 0);
            conf_emit<1>(p, s, n, oy, ox, &k, &q, sum, low);
        }
        if (p.stats) conf_flush(s, p.stats + (size_t)n * ARSEG_CONF_NSTATS, p.n_cls, sum, low);
    }
}

// ------------------------------------------------------------------ run route: exact x S upsample, align_corners == 0, S = 2 | 4 | 8
template <int S>
__global__ __launch_bounds__(256) void confidence_run_kernel(const ConfP p) {
    __shared__ ConfLds s;
    conf_stage(p, s);
    const int H = S * p.h, W = S * p.w, runs = p.w + 1;
    const long long total = (long long)H * runs;
    const float sc = arseg_resize_scale(p.h, H, false);          // = 1 / S exactly
    for (int n = blockIdx.y; n < p.N; n += gridDim.y) {
        unsigned long long sum = 0, low = 0;
        for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long long)gridDim.x * blockDim.x) {
            const int j = (int)(idx % runs) - 1, oy = (int)(idx / runs);
            int k[S];
            unsigned q[S];
            ArsegSoftmaxAcc<S> acc;
            arseg_label_run<S>(p.logits, sc, n, oy, j, p.n_cls, p.h, p.w, k, &acc);
#pragma unroll
            for (int r = 0; r < S; ++r) q[r] = acc.code(r, p.margin != 0);
            const int xs = S * j + S / 2;               // the run's first column; the first and the last run hold S/2 pixels of the frame
            if (xs >= 0 && xs + S <= W) conf_emit<S>(p, s, n, oy, xs, k, q, sum, low);
            else if (xs < 0) conf_emit<S / 2>(p, s, n, oy, 0, k + S / 2, q + S / 2, sum, low);
            else conf_emit<S / 2>(p, s, n, oy, xs, k, q, sum, low);
        }
        if (p.stats) conf_flush(s, p.stats + (size_t)n * ARSEG_CONF_NSTATS, p.n_cls, sum, low);
    }
}

// workgroups per frame x frames: the tail's caps on the whole launch, shared among the frames
dim3 conf_grid(long long per_frame, int N, int cap) {
    const int gy = N < 65535 ? N : 65535;
    const long long share = cap / gy > 0 ? cap / gy : 1, need = (per_frame + 255) / 256;
    return dim3((unsigned)(need < share ? need : share), (unsigned)gy);
}

}  // namespace

extern "C" int arseg_segment_confidence_fwd(const float *logits, int N, int n_cls, int h, int w, int H, int W, int align_corners, int kind, int low,
                                            const uint8_t *lut, uint8_t *conf8, int64_t conf_pitch, int64_t conf_n_stride, uint8_t *labels8,
                                            int64_t labels_pitch, int64_t labels_n_stride, int64_t *stats, arseg_stream_t stream) {
    ARSEG_CHECK_PTR(logits);
    if (!conf8 && !labels8 && !stats) return ARSEG_EINVAL;
    ARSEG_CHECK_POS(N); ARSEG_CHECK_POS(n_cls); ARSEG_CHECK_POS(h); ARSEG_CHECK_POS(w); ARSEG_CHECK_POS(H); ARSEG_CHECK_POS(W);
    if (n_cls > 32) return ARSEG_EINVAL;
    if (kind != ARSEG_CONF_TOP1 && kind != ARSEG_CONF_MARGIN) return ARSEG_EINVAL;
    if (low < 0 || low > 256) return ARSEG_EINVAL;
    if (conf8 && (conf_pitch < (int64_t)W || conf_n_stride < 0)) return ARSEG_EINVAL;
    if (labels8 && (labels_pitch < (int64_t)W || labels_n_stride < 0)) return ARSEG_EINVAL;
    ConfP p = {};
    p.logits = logits; p.conf = conf8; p.lab = labels8; p.stats = reinterpret_cast<unsigned long long *>(stats);
    p.conf_pitch = conf8 ? conf_pitch : 0; p.conf_ns = conf8 ? conf_n_stride : 0;
    p.lab_pitch = labels8 ? labels_pitch : 0; p.lab_ns = labels8 ? labels_n_stride : 0;
    p.N = N; p.n_cls = n_cls; p.h = h; p.w = w; p.H = H; p.W = W; p.align = align_corners ? 1 : 0;
    p.margin = kind == ARSEG_CONF_MARGIN ? 1 : 0; p.low = low;
    for (int k = 0; k < n_cls; ++k) p.lut[k] = lut ? lut[k] : (uint8_t)k;
    hipStream_t st = arseg_stream(stream);
    const int S = H / h;
    if (!p.align && S * h == H && S * w == W && (S == 2 || S == 4 || S == 8)) {          // the route choice of arseg_argmax_confusion_fwd
        const dim3 g = conf_grid((long long)H * (w + 1), N, 4096);
        if (S == 8) hipLaunchKernelGGL((confidence_run_kernel<8>), g, dim3(256), 0, st, p);
        else if (S == 4) hipLaunchKernelGGL((confidence_run_kernel<4>), g, dim3(256), 0, st, p);
        else hipLaunchKernelGGL((confidence_run_kernel<2>), g, dim3(256), 0, st, p);
        return arseg_launch_status();
    }
    hipLaunchKernelGGL(confidence_pixel_kernel, conf_grid((long long)H * W, N, 1024), dim3(256), 0, st, p);
    return arseg_launch_status();
}
