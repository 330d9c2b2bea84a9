// Temporal consistency of the masks along the motion chain (include/arseg_hip.h, arseg_segment_consistency_fwd / arseg_labels_consistency_fwd):
// does the label of a pixel agree with the label of a reference frame (the GOP's keyframe) at the position its accumulated motion vector
// points to?  Head logits (or an 8-bit train-id plane), the reference's train-id plane and the dense quarter-pel field mv_q in; the label
// plane, an 8-bit change plane (0 agree / 255 differ / 128 not compared) and per frame 3 + 3 x 32 integer counters out -- in one launch for N
// frames and one pass over the logits.  The bilinear resize and the argmax are the evaluator tail's (arseg_label_pixel / arseg_label_run,
// arseg_device.h, with the default ArsegNoAcc: labels_out equals arseg_argmax_confusion_fwd's pred on all three routes).
//
// Thread mapping: confidence.hip's -- one pixel (per-pixel routes, plane form) or one run of S pixels (run route) of one row of one frame; the
// run's S motion vectors are one contiguous piece of mv_q.  The reference label is a 1-byte gather at the motion-compensated position:
// mv_q is smooth (block constant out of a decoder), so the targets of neighbouring pixels lie next to each other on one line of the
// reference plane, which L1 / L2 serve; it is not staged.  A workgroup works on one frame at a time (blockIdx.y strides over the frames), so
// its counters belong to one row of `stats`: compared / outside / void live in registers and are added up across the wave once per frame,
// the 3 x 32 class counters are counted in LDS, and a workgroup issues one 64-bit vector atomic add per non-zero counter and frame.  All
// counters are integers: the result does not depend on the order of the atomics.
// arseg_labels_consistency_linked_fwd: one more instantiation of the plane kernel, which reads the chain's link byte of a pixel first and leaves
// a flagged pixel out of the comparison (change 128, no counter of stats, its own count per frame).
#include "arseg_device.h"

namespace {

struct TcP {
    const float *logits;                                // logits form
    const uint8_t *src;                                 // plane form: the source train-id plane
    const uint8_t *ref;                                 // reference train-id planes
    const unsigned *mv;                                 // [N][H][W] of (mvx | mvy << 16), int16 quarter pels
    uint8_t *lab, *chg;
    unsigned long long *stats;                          // [N][ARSEG_TC_NSTATS]
    long long src_pitch, src_ns, ref_pitch, ref_ns, lab_pitch, lab_ns, chg_pitch, chg_ns;          // bytes per row / per image
    int N, n_cls, h, w, H, W, align;
    uint8_t lut[32];                                    // lut ? lut[k] : k
    // the linked plane form only (behind everything the other instantiations read):
    const uint8_t *link;                                // a link plane per frame (csrc/mv_records.hip)
    long long link_pitch, link_ns;
    unsigned long long *unlinked;                       // [N]
    unsigned link_mask;
};

struct TcLds {
    unsigned long long cnt[ARSEG_TC_NSTATS];            // this workgroup's share of one row of stats
    unsigned lut[32];
};

constexpr int TC_CUR = 3, TC_REF = 3 + 32, TC_INTER = 3 + 64;
constexpr unsigned TC_NOT_COMPARED = 0xffffu;

__device__ __forceinline__ void tc_stage(const TcP &p, TcLds &s) {
    if (threadIdx.x < 32) s.lut[threadIdx.x] = p.lut[threadIdx.x];
    if (threadIdx.x < ARSEG_TC_NSTATS) s.cnt[threadIdx.x] = 0;
    __syncthreads();
}

// NC consecutive vectors of mv_q: 16-byte loads where the address allows, dword loads otherwise
template <int NC>
__device__ __forceinline__ void tc_mv_load(const unsigned *g, unsigned (&m)[NC]) {
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

// NC columns from ox on row oy of frame n with the classes k[c] (>= n_cls: a void source label, plane form only): the motion-compensated
// comparison -> the two planes and the thread's / workgroup's counters
template <int NC>
__device__ __forceinline__ void tc_emit(const TcP &p, TcLds &s, int n, int oy, int ox, const int *k, unsigned long long &cmp,
                                        unsigned long long &out, unsigned long long &vd) {
    unsigned m[NC], key[NC], ch[NC];
    tc_mv_load<NC>(p.mv + ((size_t)n * p.H + oy) * p.W + ox, m);
    const uint8_t *ref = p.ref + (size_t)n * p.ref_ns;
    unsigned no = 0, nv = 0, nc = 0;
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        const int tx = ox + c + round_half_even_div4((int)(short)(m[c] & 0xffffu)), ty = oy + round_half_even_div4((int)(short)(m[c] >> 16));
        const bool inside = (unsigned)tx < (unsigned)p.W && (unsigned)ty < (unsigned)p.H;
        const unsigned r = inside ? ref[(size_t)ty * p.ref_pitch + tx] : 255u;          // no clamp: a target off the frame is never read
        const bool compared = inside && r < (unsigned)p.n_cls && k[c] < p.n_cls;
        no += inside ? 0u : 1u; nv += (inside && !compared) ? 1u : 0u; nc += compared ? 1u : 0u;
        key[c] = compared ? ((unsigned)k[c] | (r << 8)) : TC_NOT_COMPARED;
        ch[c] = compared ? ((unsigned)k[c] == r ? 0u : 255u) : 128u;
    }
    if (p.chg) span_store<NC>(p.chg + (size_t)n * p.chg_ns + (size_t)oy * p.chg_pitch + ox, ch);
    if (p.lab) {
        unsigned v[NC];
#pragma unroll
        for (int c = 0; c < NC; ++c) v[c] = s.lut[k[c] & 31];
        span_store<NC>(p.lab + (size_t)n * p.lab_ns + (size_t)oy * p.lab_pitch + ox, v);
    }
    if (p.stats) {
        unsigned len = 0;
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            ++len;
            // neighbours of a run mostly share their class and their reference class: one set of LDS adds per stretch of equal pairs
            if (c == NC - 1 || key[c + 1] != key[c]) {
                if (key[c] != TC_NOT_COMPARED) {
                    const unsigned kc = key[c] & 0xffu, rc = key[c] >> 8;
                    atomicAdd(&s.cnt[TC_CUR + kc], (unsigned long long)len);
                    atomicAdd(&s.cnt[TC_REF + rc], (unsigned long long)len);
                    if (kc == rc) atomicAdd(&s.cnt[TC_INTER + kc], (unsigned long long)len);
                }
                len = 0;
            }
        }
        cmp += nc; out += no; vd += nv;
    }
}

// The frame is done for this workgroup: registers -> wave -> LDS -> one atomic per non-zero counter; the counters are cleared for the next frame.
__device__ __forceinline__ void tc_flush(TcLds &s, unsigned long long *row, unsigned long long cmp, unsigned long long out, unsigned long long vd) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { cmp += __shfl_xor(cmp, o, 64); out += __shfl_xor(out, o, 64); vd += __shfl_xor(vd, o, 64); }
    if ((threadIdx.x & 63) == 0) {
        if (cmp) atomicAdd(&s.cnt[0], cmp);
        if (out) atomicAdd(&s.cnt[1], out);
        if (vd) atomicAdd(&s.cnt[2], vd);
    }
    __syncthreads();
    if (threadIdx.x < ARSEG_TC_NSTATS) {
        const unsigned long long c = s.cnt[threadIdx.x];
        if (c) atomicAdd(&row[threadIdx.x], c);
        s.cnt[threadIdx.x] = 0;
    }
    __syncthreads();
}

// ------------------------------------------------------------------ per-pixel routes: h == H && w == W, any bilinear resize, or (PLANE) a byte load
// LINKED (plane form): a pixel whose link byte has a bit of link_mask is unlinked -- decided first, nothing else of it is read
template <bool PLANE, bool LINKED = false>
__global__ __launch_bounds__(256) void consistency_pixel_kernel(const TcP p) {
    __shared__ TcLds s;
    tc_stage(p, s);
    const long long total = (long long)p.H * p.W;
    const float sy = arseg_resize_scale(p.h, p.H, p.align != 0), sx = arseg_resize_scale(p.w, p.W, p.align != 0);
    const bool same = (p.h == p.H && p.w == p.W);
    for (int n = blockIdx.y; n < p.N; n += gridDim.y) {
        unsigned long long cmp = 0, out = 0, vd = 0;
        [[maybe_unused]] unsigned long long unl = 0;
        for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long long)gridDim.x * blockDim.x) {
            const int ox = (int)(idx % p.W), oy = (int)(idx / p.W);
            if constexpr (LINKED) {
                if (p.link[(size_t)n * p.link_ns + (size_t)oy * p.link_pitch + ox] & p.link_mask) {
                    if (p.chg) p.chg[(size_t)n * p.chg_ns + (size_t)oy * p.chg_pitch + ox] = 128;
                    ++unl;
                    continue;
                }
            }
            int k;
            if constexpr (PLANE) k = p.src[(size_t)n * p.src_ns + (size_t)oy * p.src_pitch + ox];
            else k = arseg_label_pixel(p.logits, n, oy, ox, p.n_cls, p.h, p.w, p.align, same, sy, sx);
            tc_emit<1>(p, s, n, oy, ox, &k, cmp, out, vd);
        }
        if (p.stats) tc_flush(s, p.stats + (size_t)n * ARSEG_TC_NSTATS, cmp, out, vd);
        if constexpr (LINKED) {
            if (p.unlinked) {                                        // registers -> wave -> LDS -> one atomic per workgroup and frame
                __shared__ unsigned long long s_unl;
                if (threadIdx.x == 0) s_unl = 0;
                __syncthreads();
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) unl += __shfl_xor(unl, o, 64);
                if ((threadIdx.x & 63) == 0 && unl) atomicAdd(&s_unl, unl);
                __syncthreads();
                if (threadIdx.x == 0 && s_unl) atomicAdd(&p.unlinked[n], s_unl);
                __syncthreads();                                     // s_unl is cleared again for the next frame
            }
        }
    }
}

// ------------------------------------------------------------------ run route: exact x S upsample, align_corners == 0, S = 2 | 4 | 8
template <int S>
__global__ __launch_bounds__(256) void consistency_run_kernel(const TcP p) {
    __shared__ TcLds s;
    tc_stage(p, s);
    const int H = S * p.h, W = S * p.w, runs = p.w + 1;
    const long long total = (long long)H * runs;
    const float sc = arseg_resize_scale(p.h, H, false);          // = 1 / S exactly
    for (int n = blockIdx.y; n < p.N; n += gridDim.y) {
        unsigned long long cmp = 0, out = 0, vd = 0;
        for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long long)gridDim.x * blockDim.x) {
            const int j = (int)(idx % runs) - 1, oy = (int)(idx / runs);
            int k[S];
            arseg_label_run<S>(p.logits, sc, n, oy, j, p.n_cls, p.h, p.w, k);
            const int xs = S * j + S / 2;               // the run's first column; the first and the last run hold S/2 pixels of the frame
            if (xs >= 0 && xs + S <= W) tc_emit<S>(p, s, n, oy, xs, k, cmp, out, vd);
            else if (xs < 0) tc_emit<S / 2>(p, s, n, oy, 0, k + S / 2, cmp, out, vd);
            else tc_emit<S / 2>(p, s, n, oy, xs, k, cmp, out, vd);
        }
        if (p.stats) tc_flush(s, p.stats + (size_t)n * ARSEG_TC_NSTATS, cmp, out, vd);
    }
}

// workgroups per frame x frames: the tail's caps on the whole launch, shared among the frames
dim3 tc_grid(long long per_frame, int N, int cap) {
    const int gy = N < 65535 ? N : 65535;
    const long long share = cap / gy > 0 ? cap / gy : 1, need = (per_frame + 255) / 256;
    return dim3((unsigned)(need < share ? need : share), (unsigned)gy);
}

// what the two forms share: the reference planes, the field, the change plane and the statistics
int tc_common(TcP &p, int N, int n_cls, int H, int W, const uint8_t *ref_labels, int64_t ref_pitch, int64_t ref_image_stride, const int16_t *mv_q,
              uint8_t *change_out, int64_t change_pitch, int64_t change_image_stride, int64_t *stats) {
    ARSEG_CHECK_PTR(ref_labels); ARSEG_CHECK_PTR(mv_q);
    ARSEG_CHECK_POS(N); ARSEG_CHECK_POS(n_cls); ARSEG_CHECK_POS(H); ARSEG_CHECK_POS(W);
    if (n_cls > 32) return ARSEG_EINVAL;
    if (reinterpret_cast<uintptr_t>(mv_q) & 3u) return ARSEG_EINVAL;
    if (ref_pitch < (int64_t)W || ref_image_stride < 0) return ARSEG_EINVAL;
    if (change_out && (change_pitch < (int64_t)W || change_image_stride < 0)) return ARSEG_EINVAL;
    p.ref = ref_labels; p.ref_pitch = ref_pitch; p.ref_ns = ref_image_stride;
    p.mv = reinterpret_cast<const unsigned *>(mv_q);
    p.chg = change_out; p.chg_pitch = change_out ? change_pitch : 0; p.chg_ns = change_out ? change_image_stride : 0;
    p.stats = reinterpret_cast<unsigned long long *>(stats);
    p.N = N; p.n_cls = n_cls; p.H = H; p.W = W;
    return ARSEG_OK;
}

}  // namespace

extern "C" int arseg_segment_consistency_fwd(const float *logits, int N, int n_cls, int h, int w, int H, int W, int align_corners,
                                             const uint8_t *ref_labels, int64_t ref_pitch, int64_t ref_image_stride, const int16_t *mv_q,
                                             const uint8_t *lut, uint8_t *labels_out, int64_t labels_pitch, int64_t labels_image_stride,
                                             uint8_t *change_out, int64_t change_pitch, int64_t change_image_stride, int64_t *stats,
                                             arseg_stream_t stream) {
    ARSEG_CHECK_PTR(logits);
    if (!labels_out && !change_out && !stats) return ARSEG_EINVAL;
    ARSEG_CHECK_POS(h); ARSEG_CHECK_POS(w);
    if (labels_out && (labels_pitch < (int64_t)W || labels_image_stride < 0)) return ARSEG_EINVAL;
    TcP p = {};
    const int rc = tc_common(p, N, n_cls, H, W, ref_labels, ref_pitch, ref_image_stride, mv_q, change_out, change_pitch, change_image_stride, stats);
    if (rc != ARSEG_OK) return rc;
    p.logits = logits; p.lab = labels_out;
    p.lab_pitch = labels_out ? labels_pitch : 0; p.lab_ns = labels_out ? labels_image_stride : 0;
    p.h = h; p.w = w; p.align = align_corners ? 1 : 0;
    for (int k = 0; k < n_cls; ++k) p.lut[k] = lut ? lut[k] : (uint8_t)k;
    hipStream_t st = arseg_stream(stream);
    const int S = H / h;
    if (!p.align && S * h == H && S * w == W && (S == 2 || S == 4 || S == 8)) {          // the route choice of arseg_argmax_confusion_fwd
        const dim3 g = tc_grid((long long)H * (w + 1), N, 4096);
        if (S == 8) hipLaunchKernelGGL((consistency_run_kernel<8>), g, dim3(256), 0, st, p);
        else if (S == 4) hipLaunchKernelGGL((consistency_run_kernel<4>), g, dim3(256), 0, st, p);
        else hipLaunchKernelGGL((consistency_run_kernel<2>), g, dim3(256), 0, st, p);
        return arseg_launch_status();
    }
    hipLaunchKernelGGL((consistency_pixel_kernel<false>), tc_grid((long long)H * W, N, 1024), dim3(256), 0, st, p);
    return arseg_launch_status();
}

extern "C" int arseg_labels_consistency_fwd(const uint8_t *labels_in, int64_t in_pitch, int64_t in_image_stride, int N, int n_cls, int H, int W,
                                            const uint8_t *ref_labels, int64_t ref_pitch, int64_t ref_image_stride, const int16_t *mv_q,
                                            uint8_t *change_out, int64_t change_pitch, int64_t change_image_stride, int64_t *stats,
                                            arseg_stream_t stream) {
    ARSEG_CHECK_PTR(labels_in);
    if (!change_out && !stats) return ARSEG_EINVAL;
    if (in_pitch < (int64_t)W || in_image_stride < 0) return ARSEG_EINVAL;
    TcP p = {};
    const int rc = tc_common(p, N, n_cls, H, W, ref_labels, ref_pitch, ref_image_stride, mv_q, change_out, change_pitch, change_image_stride, stats);
    if (rc != ARSEG_OK) return rc;
    p.src = labels_in; p.src_pitch = in_pitch; p.src_ns = in_image_stride;
    p.h = H; p.w = W;
    hipLaunchKernelGGL((consistency_pixel_kernel<true>), tc_grid((long long)H * W, N, 1024), dim3(256), 0, arseg_stream(stream), p);
    return arseg_launch_status();
}

extern "C" int arseg_labels_consistency_linked_fwd(const uint8_t *labels_in, int64_t in_pitch, int64_t in_image_stride, int N, int n_cls, int H, int W,
                                                   const uint8_t *ref_labels, int64_t ref_pitch, int64_t ref_image_stride, const int16_t *mv_q,
                                                   uint8_t *change_out, int64_t change_pitch, int64_t change_image_stride, int64_t *stats,
                                                   const uint8_t *link, int64_t link_pitch, int64_t link_image_stride, uint8_t link_mask,
                                                   int64_t *unlinked, arseg_stream_t stream) {
    ARSEG_CHECK_PTR(labels_in); ARSEG_CHECK_PTR(link);
    if (!change_out && !stats) return ARSEG_EINVAL;
    if (in_pitch < (int64_t)W || in_image_stride < 0 || link_pitch < (int64_t)W || link_image_stride < 0) return ARSEG_EINVAL;
    if (reinterpret_cast<uintptr_t>(unlinked) & 7u) return ARSEG_EINVAL;
    TcP p = {};
    const int rc = tc_common(p, N, n_cls, H, W, ref_labels, ref_pitch, ref_image_stride, mv_q, change_out, change_pitch, change_image_stride, stats);
    if (rc != ARSEG_OK) return rc;
    p.src = labels_in; p.src_pitch = in_pitch; p.src_ns = in_image_stride;
    p.h = H; p.w = W;
    p.link = link; p.link_pitch = link_pitch; p.link_ns = link_image_stride; p.link_mask = link_mask;
    p.unlinked = reinterpret_cast<unsigned long long *>(unlinked);
    hipLaunchKernelGGL((consistency_pixel_kernel<true, true>), tc_grid((long long)H * W, N, 1024), dim3(256), 0, arseg_stream(stream), p);
    return arseg_launch_status();
}
