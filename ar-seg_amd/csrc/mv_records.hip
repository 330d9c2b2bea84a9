// Decoder motion-vector block records -> mv_q, chained to the keyframe frame by frame (contract: include/arseg_hip.h,
// arseg_mv_records_*).  A decoder exports motion as prediction-block records (position, size, vector, reference index); the fast
// paths read a dense int16 [H,W,2] field accumulated back to the keyframe.  One P-frame is two kernels:
//   scatter : a wave per record, its lanes over the record's clipped pixels, atomicMax of the record index into an int32 index map
//             (-1 = uncovered) -- the highest index wins wherever records overlap, in any arrival order
//   compose : four pixels per lane; index -> 16-byte record (neighbours share it through L1 / L2) -> intra rule, rounding, clamp ->
//             4 bytes gathered from merged[f2] -> 16-byte store into merged[f]; the index map is set back to -1 on the way, so the
//             next frame needs no fill pass
// The merged tensor is the chain state: within H, W <= 8192 every accumulated value fits int16, so the link of a pixel is
// out[f][y,x] = 4 (k2 - x, j2 - y) + (f2 > 0 ? out[f2][j2,k2] : 0) and mergeMotion's int4 link table (layers.hip) is not needed.
// B-frames (arseg_mv_records_bi_*): two index maps, one per prediction list (reserved & 1), the same two kernels per frame; a frame links to
// any frame already chained in this GOP (done_mask), before or after it in display order, and frames arrive in decode order.
// Link bytes (arseg_mv_*_link_*): the compose kernels' LINK = true instantiations also write one byte per pixel -- intra / uncovered / clamped
// at this hop or at any hop towards the keyframe, and the number of hops -- gathered from link[t] at the pixel merged[t] is gathered from, and
// count them per frame: flag counts in registers, hop bins in LDS, one 64-bit atomic per non-zero counter and workgroup (consistency.hip's scheme).
#include "arseg_device.h"

constexpr int MVR_MAX_DIM = 8192;      // 4 * 8191 = 32764: the largest accumulated displacement still fits int16
// The counted LINK launches: every workgroup ends with one 64-bit atomic per non-zero counter, all on the 160 bytes of one row of link_stats, and
// those serialise in L2 (measured: ~20 000 of them, 2048 workgroups of 256 threads at 1024x2048, cost more than the rest of the kernel).  So few and
// large workgroups: at most one of 1024 threads per CU of an MI355X.
constexpr int MVL_THREADS = 1024, MVL_GRID_CAP = 256;
constexpr int MVR_BAND = 256;          // frame rows per scatter band (blockIdx.y): bounds the pixels one wave covers of a frame-sized record

// record = int16 x, y, w, h, mvx, mvy, ref, reserved, read as one int4 (little endian)
__device__ __forceinline__ int rec_lo(int v) { return (int)(short)v; }
__device__ __forceinline__ int rec_hi(int v) { return v >> 16; }

// BI: idx is two maps of H * W words, the record's list bit (reserved & 1) picks one
template <bool BI>
__global__ __launch_bounds__(256) void mv_records_scatter_kernel(const int4 *__restrict__ rec, int n, int *__restrict__ idx, int H, int W) {
    const int lane = threadIdx.x & 63;
    const int wave = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), n_waves = gridDim.x * 4;
    const int band0 = blockIdx.y * MVR_BAND, band1 = min(band0 + MVR_BAND, H);
    for (int r = wave; r < n; r += n_waves) {
        const int4 q = rec[r];                                        // wave uniform
        const int x = rec_lo(q.x), y = rec_hi(q.x), w = rec_lo(q.y), h = rec_hi(q.y);
        if (w <= 0 || h <= 0) continue;                               // padding of a fixed-capacity buffer
        const int x0 = max(x, 0), x1 = min(x + w, W), y0 = max(y, band0), y1 = min(y + h, band1);
        if (x0 >= x1 || y0 >= y1) continue;
        const int cw = x1 - x0;
        const int sh = cw > 32 ? 6 : (cw <= 1 ? 0 : 32 - __clz(cw - 1));      // lanes along x: the power of two that covers min(cw, 64)
        const int lx = lane & ((1 << sh) - 1), ly = lane >> sh, lxn = 1 << sh, lyn = 64 >> sh;
        int *map = idx;
        if constexpr (BI) map += (size_t)(rec_hi(q.w) & 1) * H * W;
        for (int yy = y0 + ly; yy < y1; yy += lyn)
            for (int xx = x0 + lx; xx < x1; xx += lxn) atomicMax(map + yy * W + xx, r);      // 0 <= yy < H, 0 <= xx < W
    }
}

// link byte of a pixel from its own flags and the byte of its target (0 where the target is the keyframe): flags accumulate, hops count up to 15
__device__ __forceinline__ unsigned mvl_byte(unsigned own, unsigned gathered) {
    return ((own | gathered) & 7u) | (min(15u, 1u + (gathered >> 4)) << 4);
}

// this workgroup's share of one row of link_stats
struct MvlCount {
    unsigned *bins;                                                   // LDS [ARSEG_LINK_NSTATS], null: no statistics wanted
    unsigned intra = 0, uncovered = 0, clamped = 0, any = 0;          // this lane's
    unsigned hop = 0, len = 0;                                        // a stretch of equal hop counts not yet added
    __device__ __forceinline__ void add(unsigned lk) {
        intra += lk & 1u; uncovered += (lk >> 1) & 1u; clamped += (lk >> 2) & 1u; any += (lk & 7u) ? 1u : 0u;
        if (len && hop != (lk >> 4)) flush();
        hop = lk >> 4; ++len;
    }
    __device__ __forceinline__ void flush() {
        if (len) atomicAdd(&bins[4 + hop], len);
        len = 0;
    }
};

__device__ __forceinline__ void mvl_count_begin(unsigned *bins) {
    if (threadIdx.x < ARSEG_LINK_NSTATS) bins[threadIdx.x] = 0;
    __syncthreads();
}

// registers -> wave -> LDS -> one 64-bit atomic per non-zero counter.  Every thread of the workgroup comes here.
__device__ __forceinline__ void mvl_count_end(MvlCount &c, unsigned long long *row) {
    c.flush();
    unsigned v[4] = {c.intra, c.uncovered, c.clamped, c.any};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v[i] += __shfl_xor(v[i], o, 64);
        if ((threadIdx.x & 63) == 0 && v[i]) atomicAdd(&c.bins[i], v[i]);
    }
    __syncthreads();
    if (threadIdx.x < ARSEG_LINK_NSTATS) {
        const unsigned n = c.bins[threadIdx.x];
        if (n) atomicAdd(&row[threadIdx.x], (unsigned long long)n);
    }
}

// one pixel of frame f: packed (dx, dy) int16 pair.  id outside [0, n): no record (intra).  LINK: lk = the pixel's link byte.
template <bool LINK>
__device__ __forceinline__ unsigned mvr_compose(const int4 *__restrict__ rec, int n, int id, const unsigned *merged, int f, int x, int y, int H, int W,
                                                int max_ref, const uint8_t *link, unsigned &lk) {
    int mx = 0, my = 0, ref = 0;                                      // intra: zero motion, previous frame
    unsigned own = ARSEG_LINK_UNCOVERED;
    if (id >= 0 && id < n) {
        const int4 q = rec[id];
        const int r = rec_lo(q.w);
        own = ARSEG_LINK_INTRA;
        if (r >= 0 && r < max_ref) { mx = rec_lo(q.z); my = rec_hi(q.z); ref = r; own = 0; }
    }
    const int tx = x + round_half_even_div4(mx), ty = y + round_half_even_div4(my);
    const int k2 = min(max(tx, 0), W - 1), j2 = min(max(ty, 0), H - 1);
    const int f2 = max(0, f - ref - 1);
    int dx = 4 * (k2 - x), dy = 4 * (j2 - y);
    unsigned g = 0;
    if (f2 > 0) {                                                     // the target's own link, from the output of frame f2 < f
        const size_t at = ((size_t)f2 * H + j2) * W + k2;
        const unsigned p = merged[at];
        dx += rec_lo((int)p); dy += rec_hi((int)p);
        if constexpr (LINK) g = link[at];
    }
    if constexpr (LINK) lk = mvl_byte(own | ((k2 != tx || j2 != ty) ? (unsigned)ARSEG_LINK_CLAMPED : 0u), g);
    return ((unsigned)dx & 0xffffu) | ((unsigned)dy << 16);
}

// merged / out: the same tensor (frames < f are read, frame f is written): no __restrict__.  LINK: link / link_out likewise (link_out = frame f of
// link), stats = row f of link_stats or null; the 4-pixel form needs link_out 4-byte aligned.
template <bool VEC, bool LINK>
__global__ __launch_bounds__(LINK ? MVL_THREADS : 256) void mv_records_compose_kernel(const int4 *__restrict__ rec, int n, int *__restrict__ idx, const unsigned *merged, unsigned *out,
                                                                 int f, int H, int W, int max_ref, const uint8_t *link, uint8_t *link_out,
                                                                 unsigned long long *stats) {
    const int hw = H * W;
    MvlCount cnt = {};
    if constexpr (LINK) {
        __shared__ unsigned bins[ARSEG_LINK_NSTATS];
        if (stats) { cnt.bins = bins; mvl_count_begin(bins); }
    }
    if constexpr (VEC) {                                              // hw % 4 == 0, 16-byte aligned frames
        const int n4 = hw >> 2;
        for (int t = blockIdx.x * blockDim.x + threadIdx.x; t < n4; t += gridDim.x * blockDim.x) {
            const int4 id = reinterpret_cast<const int4 *>(idx)[t];
            int y = (t * 4) / W, x = t * 4 - y * W;
            const int ids[4] = {id.x, id.y, id.z, id.w};
            u32x4 o;
            unsigned lw = 0;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                unsigned lk = 0;
                o[k] = mvr_compose<LINK>(rec, n, ids[k], merged, f, x, y, H, W, max_ref, link, lk);
                if constexpr (LINK) {
                    lw |= lk << (8 * k);
                    if (cnt.bins) cnt.add(lk);
                }
                if (++x == W) { x = 0; ++y; }
            }
            reinterpret_cast<u32x4 *>(out)[t] = o;
            if constexpr (LINK) reinterpret_cast<unsigned *>(link_out)[t] = lw;
            reinterpret_cast<int4 *>(idx)[t] = make_int4(-1, -1, -1, -1);
        }
    } else {
        for (int pix = blockIdx.x * blockDim.x + threadIdx.x; pix < hw; pix += gridDim.x * blockDim.x) {
            const int y = pix / W, x = pix - y * W;
            unsigned lk = 0;
            out[pix] = mvr_compose<LINK>(rec, n, idx[pix], merged, f, x, y, H, W, max_ref, link, lk);
            if constexpr (LINK) {
                link_out[pix] = (uint8_t)lk;
                if (cnt.bins) cnt.add(lk);
            }
            idx[pix] = -1;
        }
    }
    if constexpr (LINK) {
        if (stats) mvl_count_end(cnt, stats);
    }
}

// ---- B-frames: two lists, decode order ----
// display-order target of reference code `ref` from frame f: ref >= 0 counts back from f - 1 (clamped to the keyframe), ref < 0 forward from f + 1
__device__ __forceinline__ int mvb_target(int f, int ref) { return ref >= 0 ? max(0, f - ref - 1) : f - ref; }

// bit (ref + 16) set where a winner with that ref is usable: ref in [-max_ref, max_ref) and its target already chained.  Wave uniform (kernel
// arguments only); max_ref <= 16 keeps the 32 codes in one word.
__device__ __forceinline__ unsigned mvb_usable_refs(int f, unsigned long long done, int max_ref) {
    unsigned m = 0;
    for (int ref = -max_ref; ref < max_ref; ++ref) {
        const int t = mvb_target(f, ref);
        if (t < 64 && ((done >> t) & 1ull)) m |= 1u << (ref + 16);
    }
    return m;
}

// link of one list: packed 4 (k2 - x, j2 - y) + (t > 0 ? merged[t][j2][k2] : 0).  LINK: lk = the list's link byte.
template <bool LINK>
__device__ __forceinline__ unsigned mvb_link(int4 q, int t, const unsigned *merged, int x, int y, int H, int W, const uint8_t *link, unsigned &lk) {
    const int tx = x + round_half_even_div4(rec_lo(q.z)), ty = y + round_half_even_div4(rec_hi(q.z));
    const int k2 = min(max(tx, 0), W - 1), j2 = min(max(ty, 0), H - 1);
    int dx = 4 * (k2 - x), dy = 4 * (j2 - y);
    unsigned g = 0;
    if (t > 0) {
        const size_t at = ((size_t)t * H + j2) * W + k2;
        const unsigned m = merged[at];
        dx += rec_lo((int)m); dy += rec_hi((int)m);
        if constexpr (LINK) g = link[at];
    }
    if constexpr (LINK) lk = mvl_byte((k2 != tx || j2 != ty) ? (unsigned)ARSEG_LINK_CLAMPED : 0u, g);
    return ((unsigned)dx & 0xffffu) | ((unsigned)dy << 16);
}

__device__ __forceinline__ int mvb_mean(int a, int b) {               // (a + b) / 2, half to even
    const int s = a + b, m = s >> 1;
    return m + (s & 1 & m);
}

// one pixel of frame f.  id0 / id1: the winners of list 0 / 1, outside [0, n) = none.  p: the nearest chained frame before f (intra target).
// LINK: lk = the pixel's link byte (both lists under MEAN: the flags of both, the larger hop count).
template <bool LINK>
__device__ __forceinline__ unsigned mvb_compose(const int4 *__restrict__ rec, int n, int id0, int id1, const unsigned *merged, int f, int p, unsigned usable,
                                                int policy, int pix, int x, int y, int H, int W, const uint8_t *link, unsigned &lk) {
    int4 q0 = make_int4(0, 0, 0, 0), q1 = q0;
    bool u0 = false, u1 = false;
    if ((unsigned)id0 < (unsigned)n) {
        q0 = rec[id0];
        const unsigned c = (unsigned)(rec_lo(q0.w) + 16);
        u0 = c < 32u && ((usable >> c) & 1u);
    }
    if ((unsigned)id1 < (unsigned)n) {
        q1 = rec[id1];
        const unsigned c = (unsigned)(rec_lo(q1.w) + 16);
        u1 = c < 32u && ((usable >> c) & 1u);
    }
    const int t0 = mvb_target(f, rec_lo(q0.w)), t1 = mvb_target(f, rec_lo(q1.w));
    if (u0 && u1 && policy != ARSEG_MVR_BI_MEAN) {                    // one list: one gather
        if (policy == ARSEG_MVR_BI_NEAR && abs(t1 - f) < abs(t0 - f)) u0 = false;
        else u1 = false;
    }
    if (!u0 && !u1) {                                                 // intra: zero motion to frame p
        if constexpr (LINK) {
            const bool won = (unsigned)id0 < (unsigned)n || (unsigned)id1 < (unsigned)n;
            lk = mvl_byte(won ? ARSEG_LINK_INTRA : ARSEG_LINK_UNCOVERED, p > 0 ? (unsigned)link[(size_t)p * H * W + pix] : 0u);
        }
        return p > 0 ? merged[(size_t)p * H * W + pix] : 0u;
    }
    unsigned k0 = 0, k1 = 0;
    const unsigned l0 = u0 ? mvb_link<LINK>(q0, t0, merged, x, y, H, W, link, k0) : 0u, l1 = u1 ? mvb_link<LINK>(q1, t1, merged, x, y, H, W, link, k1) : 0u;
    if constexpr (LINK) lk = ((k0 | k1) & 7u) | (max(k0 >> 4, k1 >> 4) << 4);          // an unused list left its byte at 0
    if (u0 && u1) return ((unsigned)mvb_mean(rec_lo((int)l0), rec_lo((int)l1)) & 0xffffu) | ((unsigned)mvb_mean(rec_hi((int)l0), rec_hi((int)l1)) << 16);
    return u0 ? l0 : l1;
}

// idx: two maps of hw words (list 0, list 1).  merged / out: the same tensor (frames in `done` are read, frame f, not in `done`, is written).
// LINK: as in mv_records_compose_kernel.
template <bool VEC, bool LINK>
__global__ __launch_bounds__(LINK ? MVL_THREADS : 256) void mv_records_bi_compose_kernel(const int4 *__restrict__ rec, int n, int *__restrict__ idx, const unsigned *merged, unsigned *out,
                                                                    int f, unsigned long long done, int policy, int H, int W, int max_ref,
                                                                    const uint8_t *link, uint8_t *link_out, unsigned long long *stats) {
    const int hw = H * W;
    const unsigned usable = mvb_usable_refs(f, done, max_ref);
    const int p = 63 - __clzll((long long)(done & ((1ull << f) - 1ull)));     // bit 0 of done is set, 1 <= f < 64
    int *idx1 = idx + hw;
    MvlCount cnt = {};
    if constexpr (LINK) {
        __shared__ unsigned bins[ARSEG_LINK_NSTATS];
        if (stats) { cnt.bins = bins; mvl_count_begin(bins); }
    }
    if constexpr (VEC) {                                              // hw % 4 == 0, 16-byte aligned frames
        const int n4 = hw >> 2;
        for (int t = blockIdx.x * blockDim.x + threadIdx.x; t < n4; t += gridDim.x * blockDim.x) {
            const int4 a = reinterpret_cast<const int4 *>(idx)[t], b = reinterpret_cast<const int4 *>(idx1)[t];
            int y = (t * 4) / W, x = t * 4 - y * W;
            const int ia[4] = {a.x, a.y, a.z, a.w}, ib[4] = {b.x, b.y, b.z, b.w};
            u32x4 o;
            unsigned lw = 0;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                unsigned lk = 0;
                o[k] = mvb_compose<LINK>(rec, n, ia[k], ib[k], merged, f, p, usable, policy, t * 4 + k, x, y, H, W, link, lk);
                if constexpr (LINK) {
                    lw |= lk << (8 * k);
                    if (cnt.bins) cnt.add(lk);
                }
                if (++x == W) { x = 0; ++y; }
            }
            reinterpret_cast<u32x4 *>(out)[t] = o;
            if constexpr (LINK) reinterpret_cast<unsigned *>(link_out)[t] = lw;
            reinterpret_cast<int4 *>(idx)[t] = make_int4(-1, -1, -1, -1);
            reinterpret_cast<int4 *>(idx1)[t] = make_int4(-1, -1, -1, -1);
        }
    } else {
        for (int pix = blockIdx.x * blockDim.x + threadIdx.x; pix < hw; pix += gridDim.x * blockDim.x) {
            const int y = pix / W, x = pix - y * W;
            unsigned lk = 0;
            out[pix] = mvb_compose<LINK>(rec, n, idx[pix], idx1[pix], merged, f, p, usable, policy, pix, x, y, H, W, link, lk);
            if constexpr (LINK) {
                link_out[pix] = (uint8_t)lk;
                if (cnt.bins) cnt.add(lk);
            }
            idx[pix] = -1;
            idx1[pix] = -1;
        }
    }
    if constexpr (LINK) {
        if (stats) mvl_count_end(cnt, stats);
    }
}

// the dense field of one frame as the reference's decoder dumps it: (mvx, mvy, ref) of the winning record, (0, 0, -1) where there is none
__global__ __launch_bounds__(256) void mv_records_dense_kernel(const int4 *__restrict__ rec, int n, int *__restrict__ idx, int16_t *__restrict__ dense, int hw) {
    for (int pix = blockIdx.x * blockDim.x + threadIdx.x; pix < hw; pix += gridDim.x * blockDim.x) {
        const int id = idx[pix];
        int mx = 0, my = 0, ref = -1;
        if (id >= 0 && id < n) {
            const int4 q = rec[id];
            mx = rec_lo(q.z); my = rec_hi(q.z); ref = rec_lo(q.w);
        }
        dense[(size_t)pix * 3] = (int16_t)mx; dense[(size_t)pix * 3 + 1] = (int16_t)my; dense[(size_t)pix * 3 + 2] = (int16_t)ref;
        idx[pix] = -1;
    }
}

// a[i] = b[i] = -1 (all bits set) for i < n; b may be null
__global__ __launch_bounds__(256) void mv_records_fill_kernel(unsigned *__restrict__ a, unsigned *__restrict__ b, int n) {
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        a[i] = 0xffffffffu;
        if (b != nullptr) b[i] = 0xffffffffu;
    }
}

// maps: index maps in the workspace (1: P-frames, 2: B-frames)
static int mvr_check_frame(const void *records, int n_records, const void *workspace, size_t workspace_bytes, int H, int W, int maps = 1) {
    if (n_records < 0 || (n_records > 0 && records == nullptr) || workspace == nullptr) return ARSEG_EINVAL;
    if (H <= 0 || W <= 0 || H > MVR_MAX_DIM || W > MVR_MAX_DIM) return ARSEG_EINVAL;
    if (workspace_bytes < maps * arseg_mv_records_workspace_bytes(H, W)) return ARSEG_EWORKSPACE;
    if (!ARSEG_ALIGNED16(workspace) || !ARSEG_ALIGNED16(records)) return ARSEG_EINVAL;
    return ARSEG_OK;
}

template <bool BI = false>
static void mvr_scatter(const int16_t *records, int n_records, int *idx, int H, int W, hipStream_t st) {
    if (n_records == 0) return;
    const int gx = (int)(((long long)n_records + 3) / 4 > 65536 ? 65536 : ((long long)n_records + 3) / 4);
    hipLaunchKernelGGL(mv_records_scatter_kernel<BI>, dim3(gx, arseg_cdiv(H, MVR_BAND)), dim3(256), 0, st, reinterpret_cast<const int4 *>(records), n_records, idx, H, W);
}

extern "C" size_t arseg_mv_records_workspace_bytes(int H, int W) {
    return H <= 0 || W <= 0 || H > MVR_MAX_DIM || W > MVR_MAX_DIM ? 0 : (size_t)H * W * sizeof(int32_t);
}

extern "C" int arseg_mv_records_reset(int16_t *merged, void *workspace, size_t workspace_bytes, int H, int W, arseg_stream_t stream) {
    ARSEG_CHECK_PTR(merged);
    const int bad = mvr_check_frame(nullptr, 0, workspace, workspace_bytes, H, W);
    if (bad) return bad;
    if (reinterpret_cast<uintptr_t>(merged) & 3u) return ARSEG_EINVAL;
    hipStream_t st = arseg_stream(stream);
    hipLaunchKernelGGL(mv_records_fill_kernel, dim3(arseg_grid_for((long long)H * W)), dim3(256), 0, st, reinterpret_cast<unsigned *>(workspace),
                       reinterpret_cast<unsigned *>(merged), H * W);
    return arseg_launch_status();
}

// launch geometry of a compose pass over `total` items: the plain one, or the counted one (see MVL_THREADS)
static void mvl_geometry(long long total, bool counted, dim3 &grid, dim3 &block) {
    block = dim3(counted ? MVL_THREADS : 256);
    grid = dim3(counted ? arseg_grid_for((total + 3) / 4, MVL_GRID_CAP) : arseg_grid_for(total));          // (total + 3) / 4 items of 256 = total of 1024
}

// link == null: the plain step; else the LINK instantiations, which also write frame f of link and add to row f of link_stats (may be null)
static int mvr_step(const int16_t *records, int n_records, int16_t *merged, int f, int gop, void *workspace, size_t workspace_bytes, int H, int W, int max_ref,
                    uint8_t *link, int64_t *link_stats, arseg_stream_t stream) {
    ARSEG_CHECK_PTR(merged);
    const int bad = mvr_check_frame(records, n_records, workspace, workspace_bytes, H, W);
    if (bad) return bad;
    if (max_ref < 1 || max_ref > 16 || f < 1 || f >= gop || (reinterpret_cast<uintptr_t>(merged) & 3u)) return ARSEG_EINVAL;
    if (reinterpret_cast<uintptr_t>(link_stats) & 7u) return ARSEG_EINVAL;
    hipStream_t st = arseg_stream(stream);
    int *idx = reinterpret_cast<int *>(workspace);
    const int hw = H * W;
    const unsigned *m = reinterpret_cast<const unsigned *>(merged);
    unsigned *out = reinterpret_cast<unsigned *>(merged) + (size_t)f * hw;
    uint8_t *lout = link ? link + (size_t)f * hw : nullptr;
    unsigned long long *row = link_stats ? reinterpret_cast<unsigned long long *>(link_stats) + (size_t)f * ARSEG_LINK_NSTATS : nullptr;
    mvr_scatter(records, n_records, idx, H, W, st);
    const int4 *rec = reinterpret_cast<const int4 *>(records);
    const bool vec = hw % 4 == 0 && ARSEG_ALIGNED16(merged) && !(reinterpret_cast<uintptr_t>(link) & 3u);
    dim3 grid, block;
    mvl_geometry(vec ? hw / 4 : hw, link_stats != nullptr, grid, block);
    if (vec && link)
        hipLaunchKernelGGL((mv_records_compose_kernel<true, true>), grid, block, 0, st, rec, n_records, idx, m, out, f, H, W, max_ref, link, lout, row);
    else if (link)
        hipLaunchKernelGGL((mv_records_compose_kernel<false, true>), grid, block, 0, st, rec, n_records, idx, m, out, f, H, W, max_ref, link, lout, row);
    else if (vec)
        hipLaunchKernelGGL((mv_records_compose_kernel<true, false>), grid, block, 0, st, rec, n_records, idx, m, out, f, H, W, max_ref, link, lout, row);
    else
        hipLaunchKernelGGL((mv_records_compose_kernel<false, false>), grid, block, 0, st, rec, n_records, idx, m, out, f, H, W, max_ref, link, lout, row);
    return arseg_launch_status();
}

extern "C" int arseg_mv_records_step_fwd(const int16_t *records, int n_records, int16_t *merged, int f, int gop, void *workspace, size_t workspace_bytes,
                                         int H, int W, int max_ref, arseg_stream_t stream) {
    return mvr_step(records, n_records, merged, f, gop, workspace, workspace_bytes, H, W, max_ref, nullptr, nullptr, stream);
}

extern "C" int arseg_mv_records_step_link_fwd(const int16_t *records, int n_records, int16_t *merged, int f, int gop, void *workspace, size_t workspace_bytes,
                                              int H, int W, int max_ref, uint8_t *link, int64_t *link_stats, arseg_stream_t stream) {
    ARSEG_CHECK_PTR(link);
    return mvr_step(records, n_records, merged, f, gop, workspace, workspace_bytes, H, W, max_ref, link, link_stats, stream);
}

// link[0] = 0 (the keyframe links to itself: no flag, no hop), every row of link_stats = 0
__global__ __launch_bounds__(256) void mv_link_reset_kernel(uint8_t *__restrict__ link, int hw, unsigned long long *__restrict__ stats, int n_stats) {
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < hw; i += gridDim.x * blockDim.x) link[i] = 0;
    if (stats != nullptr)
        for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n_stats; i += gridDim.x * blockDim.x) stats[i] = 0;
}

extern "C" int arseg_mv_link_reset(uint8_t *link, int64_t *link_stats, int gop, int H, int W, arseg_stream_t stream) {
    ARSEG_CHECK_PTR(link);
    if (gop < 1 || gop > (1 << 20) || H <= 0 || W <= 0 || H > MVR_MAX_DIM || W > MVR_MAX_DIM) return ARSEG_EINVAL;
    if (reinterpret_cast<uintptr_t>(link_stats) & 7u) return ARSEG_EINVAL;
    hipLaunchKernelGGL(mv_link_reset_kernel, dim3(arseg_grid_for((long long)H * W)), dim3(256), 0, arseg_stream(stream), link, H * W,
                       reinterpret_cast<unsigned long long *>(link_stats), gop * ARSEG_LINK_NSTATS);
    return arseg_launch_status();
}

extern "C" int arseg_mv_records_rasterize_fwd(const int16_t *records, int n_records, int16_t *dense_out, void *workspace, size_t workspace_bytes, int H, int W,
                                              arseg_stream_t stream) {
    ARSEG_CHECK_PTR(dense_out);
    const int bad = mvr_check_frame(records, n_records, workspace, workspace_bytes, H, W);
    if (bad) return bad;
    hipStream_t st = arseg_stream(stream);
    int *idx = reinterpret_cast<int *>(workspace);
    const int hw = H * W;
    hipLaunchKernelGGL(mv_records_fill_kernel, dim3(arseg_grid_for(hw)), dim3(256), 0, st, reinterpret_cast<unsigned *>(idx), (unsigned *)nullptr, hw);
    mvr_scatter(records, n_records, idx, H, W, st);
    hipLaunchKernelGGL(mv_records_dense_kernel, dim3(arseg_grid_for(hw)), dim3(256), 0, st, reinterpret_cast<const int4 *>(records), n_records, idx, dense_out, hw);
    return arseg_launch_status();
}

extern "C" size_t arseg_mv_records_bi_workspace_bytes(int H, int W) { return 2 * arseg_mv_records_workspace_bytes(H, W); }

extern "C" int arseg_mv_records_bi_reset(int16_t *merged, void *workspace, size_t workspace_bytes, int H, int W, arseg_stream_t stream) {
    ARSEG_CHECK_PTR(merged);
    const int bad = mvr_check_frame(nullptr, 0, workspace, workspace_bytes, H, W, 2);
    if (bad) return bad;
    if (reinterpret_cast<uintptr_t>(merged) & 3u) return ARSEG_EINVAL;
    hipStream_t st = arseg_stream(stream);
    const int hw = H * W;
    unsigned *ws = reinterpret_cast<unsigned *>(workspace);
    hipLaunchKernelGGL(mv_records_fill_kernel, dim3(arseg_grid_for(hw)), dim3(256), 0, st, ws, reinterpret_cast<unsigned *>(merged), hw);
    hipLaunchKernelGGL(mv_records_fill_kernel, dim3(arseg_grid_for(hw)), dim3(256), 0, st, ws + hw, (unsigned *)nullptr, hw);
    return arseg_launch_status();
}

static int mvb_step(const int16_t *records, int n_records, int16_t *merged, int f, int gop, uint64_t done_mask, int policy, void *workspace,
                    size_t workspace_bytes, int H, int W, int max_ref, uint8_t *link, int64_t *link_stats, arseg_stream_t stream) {
    ARSEG_CHECK_PTR(merged);
    const int bad = mvr_check_frame(records, n_records, workspace, workspace_bytes, H, W, 2);
    if (bad) return bad;
    if (max_ref < 1 || max_ref > 16 || f < 1 || f >= gop || gop > 64 || (reinterpret_cast<uintptr_t>(merged) & 3u)) return ARSEG_EINVAL;
    if (!(done_mask & 1u) || ((done_mask >> f) & 1u) || (gop < 64 && (done_mask >> gop) != 0)) return ARSEG_EINVAL;
    if (policy < ARSEG_MVR_BI_LIST0 || policy > ARSEG_MVR_BI_MEAN || (reinterpret_cast<uintptr_t>(link_stats) & 7u)) return ARSEG_EINVAL;
    hipStream_t st = arseg_stream(stream);
    int *idx = reinterpret_cast<int *>(workspace);
    const int hw = H * W;
    const unsigned *m = reinterpret_cast<const unsigned *>(merged);
    unsigned *out = reinterpret_cast<unsigned *>(merged) + (size_t)f * hw;
    uint8_t *lout = link ? link + (size_t)f * hw : nullptr;
    unsigned long long *row = link_stats ? reinterpret_cast<unsigned long long *>(link_stats) + (size_t)f * ARSEG_LINK_NSTATS : nullptr;
    const unsigned long long done = done_mask;
    mvr_scatter<true>(records, n_records, idx, H, W, st);
    const int4 *rec = reinterpret_cast<const int4 *>(records);
    const bool vec = hw % 4 == 0 && ARSEG_ALIGNED16(merged) && !(reinterpret_cast<uintptr_t>(link) & 3u);
    dim3 grid, block;
    mvl_geometry(vec ? hw / 4 : hw, link_stats != nullptr, grid, block);
    if (vec && link)
        hipLaunchKernelGGL((mv_records_bi_compose_kernel<true, true>), grid, block, 0, st, rec, n_records, idx, m, out, f, done, policy, H, W, max_ref, link,
                           lout, row);
    else if (link)
        hipLaunchKernelGGL((mv_records_bi_compose_kernel<false, true>), grid, block, 0, st, rec, n_records, idx, m, out, f, done, policy, H, W, max_ref, link,
                           lout, row);
    else if (vec)
        hipLaunchKernelGGL((mv_records_bi_compose_kernel<true, false>), grid, block, 0, st, rec, n_records, idx, m, out, f, done, policy, H, W, max_ref, link,
                           lout, row);
    else
        hipLaunchKernelGGL((mv_records_bi_compose_kernel<false, false>), grid, block, 0, st, rec, n_records, idx, m, out, f, done, policy, H, W, max_ref, link,
                           lout, row);
    return arseg_launch_status();
}

extern "C" int arseg_mv_records_bi_step_fwd(const int16_t *records, int n_records, int16_t *merged, int f, int gop, uint64_t done_mask, int policy,
                                            void *workspace, size_t workspace_bytes, int H, int W, int max_ref, arseg_stream_t stream) {
    return mvb_step(records, n_records, merged, f, gop, done_mask, policy, workspace, workspace_bytes, H, W, max_ref, nullptr, nullptr, stream);
}

extern "C" int arseg_mv_records_bi_step_link_fwd(const int16_t *records, int n_records, int16_t *merged, int f, int gop, uint64_t done_mask, int policy,
                                                 void *workspace, size_t workspace_bytes, int H, int W, int max_ref, uint8_t *link, int64_t *link_stats,
                                                 arseg_stream_t stream) {
    ARSEG_CHECK_PTR(link);
    return mvb_step(records, n_records, merged, f, gop, done_mask, policy, workspace, workspace_bytes, H, W, max_ref, link, link_stats, stream);
}
