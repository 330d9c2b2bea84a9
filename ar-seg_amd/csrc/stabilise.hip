// The keyframe prior along the motion chain (include/arseg_hip.h, arseg_segment_stabilise_fwd): where the motion link of a pixel is trustworthy
// and the frame's own decision is marginal, the pixel keeps the class the keyframe had at the motion-compensated position.  Head logits, the
// reference's train-id plane, the dense quarter-pel field mv_q, the per-frame hold threshold and (optionally) the chain's link bytes and the
// reference's confidence plane in; the label plane, an 8-bit hold plane (0 agree / 255 held / 192 own / 128 no prior) and per frame 7 + 2 x 32
// integer counters out -- in one launch for N frames and one pass over the logits.  The bilinear resize and the argmax are the evaluator
// tail's (arseg_label_pixel / arseg_label_run, arseg_device.h); the margin m - v_ref rides on the class loop of that rule as an accumulator
// (ArsegHoldAcc below: running maximum and the value of the reference's class), so the taps are loaded once and no per-class array exists.
//
// Thread mapping: consistency.hip's -- one pixel (per-pixel routes) or one run of S pixels (run route) of one row of one frame.  The link
// byte, the motion vector, the reference label and the reference's confidence code of a pixel are gathered BEFORE the class loop, so that
// the reference's class is known when the classes stream by; they are 1-byte gathers that L1 / L2 serve (consistency.hip says why they are
// not staged).  A workgroup works on one frame at a time (blockIdx.y strides over the frames), so its counters belong to one row of
// `stats` and its threshold is one scalar: the seven outcome counts live in registers and are added up across the wave once per frame,
// the 2 x 32 class counters of the held pixels are counted in LDS, and a workgroup issues one 64-bit vector atomic add per non-zero counter
// and frame.  All counters are integers: the result does not depend on the order of the atomics.
#include "arseg_device.h"

namespace {

struct StP {
    const float *logits;
    const uint8_t *ref, *conf, *link;                   // reference train ids; its confidence codes (or null); link planes (or null)
    const unsigned *mv;                                 // [N][H][W] of (mvx | mvy << 16), int16 quarter pels
    const float *bonus;                                 // [N]
    uint8_t *lab, *hold;
    unsigned long long *stats;                          // [N][ARSEG_ST_NSTATS]
    long long ref_pitch, ref_ns, conf_pitch, conf_ns, link_pitch, link_ns, lab_pitch, lab_ns, hold_pitch, hold_ns;          // bytes per row / per image
    int N, n_cls, h, w, H, W, align, ref_low;
    unsigned link_mask;
    uint8_t lut[32];                                    // lut ? lut[k] : k
};

struct StLds {
    unsigned long long cnt[ARSEG_ST_NSTATS];            // this workgroup's share of one row of stats
    unsigned lut[32];
};

// outcomes in the order they are decided and counted; a pixel without a prior carries -(outcome + 1) where one with a prior carries c_ref
constexpr int ST_UNLINKED = 0, ST_OUTSIDE = 1, ST_VOID = 2, ST_WEAK = 3, ST_AGREE = 4, ST_HELD = 5, ST_OWN = 6, ST_NOUT = 7;
constexpr int ST_INTO = 8, ST_FROM = 8 + 32;
constexpr unsigned ST_NOT_HELD = 0xffffu;

// Rides on the label rule: m[r] as ArsegSoftmaxAcc keeps it, and vref[r], the value of the step whose class index equals the reference's
// class of pixel r.  The rule does not pass k to step(), so left[r] counts the steps down to that class (a pixel without a prior starts
// below zero and never gets there): S + S + S registers.
template <int S>
struct ArsegHoldAcc {
    float m[S], vref[S];
    int left[S];
    __device__ __forceinline__ explicit ArsegHoldAcc(const int (&pre)[S]) {
#pragma unroll
        for (int r = 0; r < S; ++r) { m[r] = -INFINITY; vref[r] = -INFINITY; left[r] = pre[r]; }
    }
    __device__ __forceinline__ void step(int r, float v, float best, bool take) {
        vref[r] = left[r] == 0 ? v : vref[r];
        --left[r];
        m[r] = take ? v : m[r];
    }
    // HELD or OWN for pixel r, whose reference class differs from k*: strict, fp32, false when an operand is NaN (-inf - -inf included)
    __device__ __forceinline__ bool held(int r, float beta) const { return m[r] - vref[r] < beta; }
};

__device__ __forceinline__ void st_stage(const StP &p, StLds &s) {
    if (threadIdx.x < 32) s.lut[threadIdx.x] = p.lut[threadIdx.x];
    if (threadIdx.x < ARSEG_ST_NSTATS) s.cnt[threadIdx.x] = 0;
    __syncthreads();
}

// NC consecutive vectors of mv_q: 16-byte loads where the address allows, dword loads otherwise
template <int NC>
__device__ __forceinline__ void st_mv_load(const unsigned *g, unsigned (&m)[NC]) {
    if constexpr (NC % 4 == 0) {
        if (!((unsigned)reinterpret_cast<uintptr_t>(g) & 15u)) {
#pragma unroll
            for (int q = 0; q < NC; q += 4) {
                const u32x4 x = *reinterpret_cast<const u32x4 *>(g + q);
                m[q] = x.x; m[q + 1] = x.y; m[q + 2] = x.z; m[q + 3] = x.w;
            }
            return;
        }
    }
#pragma unroll
    for (int q = 0; q < NC; ++q) m[q] = g[q];
}

// NC columns from ox on row oy of frame n, all inside the frame: what the keyframe offers each of them -> pre[c] = c_ref, or -(outcome + 1)
// for UNLINKED / OUTSIDE / VOID / WEAK in that order.  An unlinked pixel reads neither mv_q nor the reference (a run with one takes its
// vectors word by word); a target off the frame is never read.
template <int NC>
__device__ __forceinline__ void st_prior(const StP &p, int n, int oy, int ox, int *pre) {
    bool linked[NC];
    bool any = false, all = true;
#pragma unroll
    for (int c = 0; c < NC; ++c) linked[c] = true;
    if (p.link) {
        unsigned l[NC];
        span_load<NC>(p.link + (size_t)n * p.link_ns + (size_t)oy * p.link_pitch + ox, l);
#pragma unroll
        for (int c = 0; c < NC; ++c) linked[c] = !(l[c] & p.link_mask);
    }
#pragma unroll
    for (int c = 0; c < NC; ++c) { any = any || linked[c]; all = all && linked[c]; pre[c] = -(ST_UNLINKED + 1); }
    if (!any) return;
    unsigned m[NC];
    const unsigned *g = p.mv + ((size_t)n * p.H + oy) * p.W + ox;
    if (all) st_mv_load<NC>(g, m);
    else {
#pragma unroll
        for (int c = 0; c < NC; ++c) m[c] = linked[c] ? g[c] : 0u;
    }
    const uint8_t *ref = p.ref + (size_t)n * p.ref_ns;
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        if (!linked[c]) continue;
        const int tx = ox + c + round_half_even_div4((int)(short)(m[c] & 0xffffu)), ty = oy + round_half_even_div4((int)(short)(m[c] >> 16));
        const bool inside = (unsigned)tx < (unsigned)p.W && (unsigned)ty < (unsigned)p.H;
        int v = -(ST_OUTSIDE + 1);
        if (inside) {                                                                    // no clamp
            const int r = ref[(size_t)ty * p.ref_pitch + tx];
            v = r < p.n_cls ? r : -(ST_VOID + 1);
            if (p.conf && r < p.n_cls && (int)p.conf[(size_t)n * p.conf_ns + (size_t)ty * p.conf_pitch + tx] < p.ref_low) v = -(ST_WEAK + 1);
        }
        pre[c] = v;
    }
}

// NC columns from ox on row oy of frame n: classes k[c], priors pre[c], HELD / OWN decisions hd[c] (read where pre[c] >= 0 and != k[c])
// -> the two planes and the thread's / workgroup's counters
template <int NC>
__device__ __forceinline__ void st_emit(const StP &p, StLds &s, int n, int oy, int ox, const int *k, const int *pre, const bool *hd,
                                        unsigned long long (&cnt)[ST_NOUT]) {
    int oc[NC];
    unsigned key[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        oc[c] = pre[c] < 0 ? -(pre[c] + 1) : (pre[c] == k[c] ? ST_AGREE : (hd[c] ? ST_HELD : ST_OWN));
        key[c] = oc[c] == ST_HELD ? ((unsigned)k[c] | ((unsigned)pre[c] << 8)) : ST_NOT_HELD;
    }
    if (p.hold) {
        unsigned v[NC];
#pragma unroll
        for (int c = 0; c < NC; ++c) v[c] = oc[c] == ST_AGREE ? 0u : (oc[c] == ST_HELD ? 255u : (oc[c] == ST_OWN ? 192u : 128u));
        span_store<NC>(p.hold + (size_t)n * p.hold_ns + (size_t)oy * p.hold_pitch + ox, v);
    }
    if (p.lab) {
        unsigned v[NC];
#pragma unroll
        for (int c = 0; c < NC; ++c) v[c] = s.lut[(oc[c] == ST_HELD ? pre[c] : k[c]) & 31];
        span_store<NC>(p.lab + (size_t)n * p.lab_ns + (size_t)oy * p.lab_pitch + ox, v);
    }
    if (p.stats) {
        unsigned len = 0;
#pragma unroll
        for (int c = 0; c < NC; ++c) {
#pragma unroll
            for (int o = 0; o < ST_NOUT; ++o) cnt[o] += oc[c] == o ? 1u : 0u;
            ++len;
            // neighbours of a run mostly share their class and their reference class: one pair of LDS adds per stretch of equal pairs
            if (c == NC - 1 || key[c + 1] != key[c]) {
                if (key[c] != ST_NOT_HELD) {
                    atomicAdd(&s.cnt[ST_INTO + (key[c] >> 8)], (unsigned long long)len);
                    atomicAdd(&s.cnt[ST_FROM + (key[c] & 0xffu)], (unsigned long long)len);
                }
                len = 0;
            }
        }
    }
}

// The frame is done for this workgroup: registers -> wave -> LDS -> one atomic per non-zero counter; the counters are cleared for the next frame.
__device__ __forceinline__ void st_flush(StLds &s, unsigned long long *row, unsigned long long (&cnt)[ST_NOUT]) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
        for (int i = 0; i < ST_NOUT; ++i) cnt[i] += __shfl_xor(cnt[i], o, 64);
    }
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int i = 0; i < ST_NOUT; ++i)
            if (cnt[i]) atomicAdd(&s.cnt[i], cnt[i]);
    }
    __syncthreads();
    if (threadIdx.x < ARSEG_ST_NSTATS) {
        const unsigned long long c = s.cnt[threadIdx.x];
        if (c) atomicAdd(&row[threadIdx.x], c);                     // (the reserved word is never counted into: it stays untouched)
        s.cnt[threadIdx.x] = 0;
    }
    __syncthreads();
}

// ------------------------------------------------------------------ per-pixel routes: h == H && w == W, or any bilinear resize
__global__ __launch_bounds__(256) void stabilise_pixel_kernel(const StP p) {
    __shared__ StLds s;
    st_stage(p, s);
    const long long total = (long long)p.H * p.W;
    const float sy = arseg_resize_scale(p.h, p.H, p.align != 0), sx = arseg_resize_scale(p.w, p.W, p.align != 0);
    const bool same = (p.h == p.H && p.w == p.W);
    for (int n = blockIdx.y; n < p.N; n += gridDim.y) {
        const float beta = p.bonus[n];
        unsigned long long cnt[ST_NOUT] = {};
        for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long long)gridDim.x * blockDim.x) {
            const int ox = (int)(idx % p.W), oy = (int)(idx / p.W);
            int pre[1];
            st_prior<1>(p, n, oy, ox, pre);
            ArsegHoldAcc<1> acc(pre);
            const int k = arseg_label_pixel(p.logits, n, oy, ox, p.n_cls, p.h, p.w, p.align, same, sy, sx, &acc);
            const bool hd = acc.held(0, beta);
            st_emit<1>(p, s, n, oy, ox, &k, pre, &hd, cnt);
        }
        if (p.stats) st_flush(s, p.stats + (size_t)n * ARSEG_ST_NSTATS, cnt);
    }
}

// ------------------------------------------------------------------ run route: exact x S upsample, align_corners == 0, S = 2 | 4 | 8
template <int S>
__global__ __launch_bounds__(256) void stabilise_run_kernel(const StP p) {
    __shared__ StLds s;
    st_stage(p, s);
    const int H = S * p.h, W = S * p.w, runs = p.w + 1;
    const long long total = (long long)H * runs;
    const float sc = arseg_resize_scale(p.h, H, false);          // = 1 / S exactly
    for (int n = blockIdx.y; n < p.N; n += gridDim.y) {
        const float beta = p.bonus[n];
        unsigned long long cnt[ST_NOUT] = {};
        for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long long)gridDim.x * blockDim.x) {
            const int j = (int)(idx % runs) - 1, oy = (int)(idx / runs);
            const int xs = S * j + S / 2;               // the run's first column; the first and the last run hold S/2 pixels of the frame
            const bool full = xs >= 0 && xs + S <= W;
            int pre[S], k[S];
            bool hd[S];
#pragma unroll
            for (int r = 0; r < S; ++r) pre[r] = -(ST_UNLINKED + 1);          // the half of a border run that lies off the frame: no pixel, no prior
            if (full) st_prior<S>(p, n, oy, xs, pre);
            else if (xs < 0) st_prior<S / 2>(p, n, oy, 0, pre + S / 2);
            else st_prior<S / 2>(p, n, oy, xs, pre);
            ArsegHoldAcc<S> acc(pre);
            arseg_label_run<S>(p.logits, sc, n, oy, j, p.n_cls, p.h, p.w, k, &acc);
#pragma unroll
            for (int r = 0; r < S; ++r) hd[r] = acc.held(r, beta);
            if (full) st_emit<S>(p, s, n, oy, xs, k, pre, hd, cnt);
            else if (xs < 0) st_emit<S / 2>(p, s, n, oy, 0, k + S / 2, pre + S / 2, hd + S / 2, cnt);
            else st_emit<S / 2>(p, s, n, oy, xs, k, pre, hd, cnt);
        }
        if (p.stats) st_flush(s, p.stats + (size_t)n * ARSEG_ST_NSTATS, cnt);
    }
}

// workgroups per frame x frames: the tail's caps on the whole launch, shared among the frames
dim3 st_grid(long long per_frame, int N, int cap) {
    const int gy = N < 65535 ? N : 65535;
    const long long share = cap / gy > 0 ? cap / gy : 1, need = (per_frame + 255) / 256;
    return dim3((unsigned)(need < share ? need : share), (unsigned)gy);
}

}  // namespace

extern "C" int arseg_segment_stabilise_fwd(const float *logits, int N, int n_cls, int h, int w, int H, int W, int align_corners,
                                           const uint8_t *ref_labels, int64_t ref_pitch, int64_t ref_image_stride, const int16_t *mv_q,
                                           const float *bonus, const uint8_t *link, int64_t link_pitch, int64_t link_image_stride,
                                           uint8_t link_mask, const uint8_t *ref_conf, int64_t conf_pitch, int64_t conf_image_stride, int ref_low,
                                           const uint8_t *lut, uint8_t *labels_out, int64_t labels_pitch, int64_t labels_image_stride,
                                           uint8_t *hold_out, int64_t hold_pitch, int64_t hold_image_stride, int64_t *stats,
                                           arseg_stream_t stream) {
    ARSEG_CHECK_PTR(logits); ARSEG_CHECK_PTR(ref_labels); ARSEG_CHECK_PTR(mv_q); ARSEG_CHECK_PTR(bonus);
    if (!labels_out && !hold_out && !stats) return ARSEG_EINVAL;
    ARSEG_CHECK_POS(N); ARSEG_CHECK_POS(n_cls); ARSEG_CHECK_POS(h); ARSEG_CHECK_POS(w); ARSEG_CHECK_POS(H); ARSEG_CHECK_POS(W);
    if (n_cls > 32 || ref_low < 0 || ref_low > 256) return ARSEG_EINVAL;
    if ((reinterpret_cast<uintptr_t>(mv_q) & 3u) || (reinterpret_cast<uintptr_t>(bonus) & 3u)) return ARSEG_EINVAL;
    if (ref_pitch < (int64_t)W || ref_image_stride < 0) return ARSEG_EINVAL;
    if (link && (link_pitch < (int64_t)W || link_image_stride < 0)) return ARSEG_EINVAL;
    if (ref_conf && (conf_pitch < (int64_t)W || conf_image_stride < 0)) return ARSEG_EINVAL;
    if (labels_out && (labels_pitch < (int64_t)W || labels_image_stride < 0)) return ARSEG_EINVAL;
    if (hold_out && (hold_pitch < (int64_t)W || hold_image_stride < 0)) return ARSEG_EINVAL;
    StP p = {};
    p.logits = logits; p.ref = ref_labels; p.ref_pitch = ref_pitch; p.ref_ns = ref_image_stride;
    p.mv = reinterpret_cast<const unsigned *>(mv_q); p.bonus = bonus;
    if (link && link_mask) { p.link = link; p.link_pitch = link_pitch; p.link_ns = link_image_stride; p.link_mask = link_mask; }
    if (ref_conf && ref_low > 0) { p.conf = ref_conf; p.conf_pitch = conf_pitch; p.conf_ns = conf_image_stride; p.ref_low = ref_low; }
    p.lab = labels_out; p.lab_pitch = labels_out ? labels_pitch : 0; p.lab_ns = labels_out ? labels_image_stride : 0;
    p.hold = hold_out; p.hold_pitch = hold_out ? hold_pitch : 0; p.hold_ns = hold_out ? hold_image_stride : 0;
    p.stats = reinterpret_cast<unsigned long long *>(stats);
    p.N = N; p.n_cls = n_cls; p.h = h; p.w = w; p.H = H; p.W = W; p.align = align_corners ? 1 : 0;
    for (int k = 0; k < n_cls; ++k) p.lut[k] = lut ? lut[k] : (uint8_t)k;
    hipStream_t st = arseg_stream(stream);
    const int S = H / h;
    if (!p.align && S * h == H && S * w == W && (S == 2 || S == 4 || S == 8)) {          // the route choice of arseg_argmax_confusion_fwd
        const dim3 g = st_grid((long long)H * (w + 1), N, 4096);
        if (S == 8) hipLaunchKernelGGL((stabilise_run_kernel<8>), g, dim3(256), 0, st, p);
        else if (S == 4) hipLaunchKernelGGL((stabilise_run_kernel<4>), g, dim3(256), 0, st, p);
        else hipLaunchKernelGGL((stabilise_run_kernel<2>), g, dim3(256), 0, st, p);
        return arseg_launch_status();
    }
    hipLaunchKernelGGL(stabilise_pixel_kernel, st_grid((long long)H * W, N, 1024), dim3(256), 0, st, p);
    return arseg_launch_status();
}
