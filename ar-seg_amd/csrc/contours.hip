// Region outlines of a row-run code as closed polygon loops (include/arseg_hip.h, arseg_rle_contours_fwd): a run code with its run_region
// (as arseg_labels_rle_fwd + arseg_rle_regions_fwd leave them) in; per frame the loops {region, first, count, hole} and the corners of
// every loop, in the contract's canonical order, out.  Nothing of the size of a frame is read or written: the run code already holds every
// vertical boundary segment of the mask -- the two ends of each run -- so the input is a few thousand words per frame and stays in L2.
//
// Edges.  Run i gives the edges 2 i (its left end, travelled upwards) and 2 i + 1 (its right end, travelled downwards): the region lies on
// the right hand.  The edge after an edge along its loop is found from the neighbouring row alone; between the two lies a horizontal
// stretch (a move, whose two end points are corners of the loop) or nothing (the next edge goes straight on: no corner).  The 2 r edges of
// a frame form a permutation whose cycles are the loops; the smallest edge of a cycle is the loop's leader.
//
// Scratch lives in the caller's workspace, per frame and edge slot (2 cap of them): the successor with the move's flag in bit 0, the
// corner where the move ends, and two 16-byte states {jump pointer, smallest edge of the window, weight up to the first occurrence of
// that edge, weight of the window} that the pointer jumping ping-pongs between.  The buffer that does not hold the final state takes the
// loops' {first, count} at their leaders afterwards.
// 4 + K launches, K = ceil(log2(2 cap)) fixed on the host; a phase boundary is a launch boundary: no workgroup waits for another, no flags
// are waited on, nothing spins on memory, no atomics are needed.
//   clear    the refusal decision: counts = {-1, -1} or {0, 0}.
//   succ     a wave owns a row (grid-stride over the rows, blockIdx.y strides over the frames), its lanes take the row's runs 64 at a time.
//            From the top of a left end (the bottom of a right end) the two pixels across the corner are looked up in the neighbouring row
//            by binary search; then the edge goes straight on, or turns and walks along the horizontal stretch, run by run, to the next
//            end of a run of its value.  Touching runs of one value are one region, so values and the connectivity decide everything.
//   jump     K times: a lane per edge combines its window with the window its pointer names; the first minimum is kept.  Once the window
//            covers the cycle every edge knows its leader and the weight from itself forward to the leader; further rounds change nothing.
//   scan     one workgroup per frame: the prefix (rc_block_scan) over the edges, of the leaders (a loop's index) and of their vertex totals (a loop's
//            first); counts and the loop records.
//   emit     the walk of succ over rows and runs: an edge with a move writes its two corners at first + position, the position turned by
//            one for a hole (which begins where its leader starts, not where it ends); words below vcap only.
// Integers throughout: every output is a pure function of the inputs.
//
// Bounds of the loops (nothing else loops):
//   grid-stride loops      over frames, rows, runs of a row and edges: counted.
//   rc_cover               a binary search over (first, last] of the neighbouring row: at most 31 rounds.
//   the walks              advance one run of one row per round and end at that row's first or last run at the latest.
//   the shuffles           6 rounds.
// Indices are clamped by runcode.h: a row's runs into [0, stored runs) of its frame, columns into [0, W].  Every successor
// is made from such a run index, so every pointer the jumps follow stays below twice the stored runs; a loop index or a vertex position
// is used only below lcap or vcap; a division is made only by a positive total.  A malformed run code gives meaningless loops and nothing
// outside the caller's buffers.
#include "runcode.h"

namespace {

typedef unsigned ct_u32x4 __attribute__((ext_vector_type(4), aligned(4)));
typedef int ct_i32x4 __attribute__((ext_vector_type(4), aligned(4)));

constexpr int CT_WAVES = 4;                             // waves (= rows in flight) per workgroup

struct CtP {
    const int *rs;                                      // [N][H + 1]
    const unsigned *runs;                               // [N][cap]
    const int *nreg;                                    // [N]
    const int *rr;                                      // run_region [N][cap]
    int *counts;                                        // [N][2]
    int *loops;                                         // [N][lcap][4] (may be null: lcap == 0)
    unsigned *verts;                                    // [N][vcap] (may be null: vcap == 0)
    unsigned *succ;                                     // [N][2 cap]: next edge << 1 | the move is not empty
    unsigned *endv;                                     // [N][2 cap]: the corner where the move ends
    ct_u32x4 *st[2];                                    // [N][2 cap] each: {pointer, smallest edge, weight to its first occurrence, weight}
    long long cap_stride, lcap, vcap;
    int cap;                                            // <= 1 << 29: an edge index is below 2^30
    int N, H, W, eight;
};

// The stored runs of a frame, or -1 for a frame that is refused: its run code overflowed or its regions are missing.
__device__ __forceinline__ int ct_total(const CtP &p, int n) {
    const int stored = rc_stored(p.rs[(size_t)n * (p.H + 1) + p.H], p.cap);
    return (stored < 0 || p.nreg[n] < 0) ? -1 : stored;          // (n_regions is not read for an overflowed frame)
}

// Eastwards along line Y, the top of run t (tl: the end of its row), the region below: the first run in [j, stop) of the row above with
// value v that starts before the end of t (at it too with 8-connectivity: the diagonal pixels are joined) -> its left end; else the
// right end of t.
__device__ __forceinline__ void ct_east(const unsigned *runs, int W, bool eight, int t, int tl, int Y, unsigned v, int j, int stop, unsigned &next,
                                        unsigned &corner) {
    const int t1 = rc_x1(runs, t, tl, W);
    for (; j < stop; ++j) {
        const int b0 = rc_x0(runs, j, W);
        if (eight ? b0 > t1 : b0 >= t1) break;
        if ((runs[j] & 0xffu) == v) { next = 2u * (unsigned)j; corner = ((unsigned)Y << 16) | (unsigned)b0; return; }
    }
    next = 2u * (unsigned)t + 1u; corner = ((unsigned)Y << 16) | (unsigned)t1;
}

// Westwards along line Y, the bottom of run t, the region above: the last run in [stop, k] of the row below (kl: its end) with value v
// that ends behind the start of t (at it too with 8-connectivity) -> its right end; else the left end of t.
__device__ __forceinline__ void ct_west(const unsigned *runs, int W, bool eight, int t, int Y, unsigned v, int k, int stop, int kl, unsigned &next,
                                        unsigned &corner) {
    const int t0 = rc_x0(runs, t, W);
    for (; k >= stop; --k) {
        const int k1 = rc_x1(runs, k, kl, W);
        if (eight ? k1 < t0 : k1 <= t0) break;
        if ((runs[k] & 0xffu) == v) { next = 2u * (unsigned)k + 1u; corner = ((unsigned)Y << 16) | (unsigned)k1; return; }
    }
    next = 2u * (unsigned)t; corner = ((unsigned)Y << 16) | (unsigned)t0;
}

__global__ __launch_bounds__(256) void contours_clear_kernel(const CtP p) {
    for (int n = blockIdx.x * blockDim.x + threadIdx.x; n < p.N; n += gridDim.x * blockDim.x) {
        const int v = ct_total(p, n) >= 0 ? 0 : -1;
        p.counts[2 * (size_t)n] = v; p.counts[2 * (size_t)n + 1] = v;
    }
}

__global__ __launch_bounds__(64 * CT_WAVES) void contours_succ_kernel(const CtP p) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const bool eight = p.eight != 0;
    for (int n = blockIdx.y; n < p.N; n += gridDim.y) {
        const int total = ct_total(p, n);
        if (total <= 0) continue;
        const int *rs = p.rs + (size_t)n * (p.H + 1);
        const unsigned *runs = p.runs + (size_t)n * p.cap_stride;
        const size_t edge0 = (size_t)n * 2 * p.cap_stride;
        for (int y = blockIdx.x * CT_WAVES + wave; y < p.H; y += gridDim.x * CT_WAVES) {
            // a malformed row_start may not lead outside [0, total): the three rows are clamped into it
            int first, last;
            rc_row(rs, y, total, first, last);
            const int pf = y > 0 ? rc_clamp(rs[y - 1], 0, first) : first, pl = first;              // the row above: [pf, pl), empty for y == 0
            const int nf = last, nl = y + 1 < p.H ? rc_clamp(rs[y + 2], last, total) : last;      // the row below: [nf, nl)
            for (int i = first + lane; i < last; i += 64) {                  // no lane needs another: nothing is shuffled here
                const unsigned v = runs[i] & 0xffu;
                const int a0 = rc_x0(runs, i, p.W), a1 = rc_x1(runs, i, last, p.W);
                for (int side = 0; side < 2; ++side) {
                    unsigned next, corner;
                    const unsigned own = side ? ((unsigned)(y + 1) << 16) | (unsigned)a1 : ((unsigned)y << 16) | (unsigned)a0;
                    if (side == 0) {                                        // arriving at (a0, y), heading up
                        if (pl <= pf) ct_east(runs, p.W, eight, i, last, y, v, 0, 0, next, corner);
                        else {
                            const int q = rc_cover(runs, pf, pl, a0);
                            const bool ur = (runs[q] & 0xffu) == v;
                            const bool ul = a0 > 0 && (rc_x0(runs, q, p.W) < a0 ? ur : (q > pf && (runs[q - 1] & 0xffu) == v));
                            if (ur && !ul) { next = 2u * (unsigned)q; corner = own; }
                            else if (ur || (eight && ul)) ct_west(runs, p.W, eight, ur ? q : q - 1, y, v, i - 1, first, last, next, corner);
                            else ct_east(runs, p.W, eight, i, last, y, v, q + 1, pl, next, corner);
                        }
                    } else {                                                // arriving at (a1, y + 1), heading down
                        if (nl <= nf) ct_west(runs, p.W, eight, i, y + 1, v, -1, 0, last, next, corner);
                        else {
                            const int q = rc_cover(runs, nf, nl, a1 - 1);
                            const bool bl = (runs[q] & 0xffu) == v;
                            const bool br = a1 < p.W && (rc_x1(runs, q, nl, p.W) > a1 ? bl : (q + 1 < nl && (runs[q + 1] & 0xffu) == v));
                            if (bl && !br) { next = 2u * (unsigned)q + 1u; corner = own; }
                            else if (bl || (eight && br)) ct_east(runs, p.W, eight, bl ? q : q + 1, nl, y + 1, v, i + 1, last, next, corner);
                            else ct_west(runs, p.W, eight, i, y + 1, v, q, nf, nl, next, corner);
                        }
                    }
                    const unsigned e = 2u * (unsigned)i + (unsigned)side, moved = corner != own ? 1u : 0u;
                    p.succ[edge0 + e] = (next << 1) | moved;
                    p.endv[edge0 + e] = corner;
                    p.st[0][edge0 + e] = ct_u32x4{next, e, 0u, 2u * moved};
                }
            }
        }
    }
}

// One round of pointer jumping, st[from] -> st[1 - from].  Windows: edge e holds the 2^k edges from e on; combined with the window its
// pointer names it holds 2^(k+1).  The first minimum is kept, so a window that wraps round its cycle stays correct.  The weights are
// unsigned: a window of many laps may wrap, but such a window holds its minimum in its first half and its weight is not used.
__global__ __launch_bounds__(256) void contours_jump_kernel(const CtP p, int from) {
    for (int n = blockIdx.y; n < p.N; n += gridDim.y) {
        const int total = ct_total(p, n);
        if (total <= 0) continue;
        const ct_u32x4 *src = p.st[from] + (size_t)n * 2 * p.cap_stride;
        ct_u32x4 *dst = p.st[1 - from] + (size_t)n * 2 * p.cap_stride;
        const unsigned edges = 2u * (unsigned)total;
        for (unsigned e = blockIdx.x * blockDim.x + threadIdx.x; e < edges; e += gridDim.x * blockDim.x) {
            const ct_u32x4 a = src[e];
            const ct_u32x4 b = src[min(a.x, edges - 1u)];
            dst[e] = ct_u32x4{b.x, min(a.y, b.y), a.y <= b.y ? a.z : a.w + b.z, a.w + b.w};
        }
    }
}

// Per frame: the leaders (the edges that are their window's smallest) counted and their totals summed over the edge array, 256 at a time
// with a carry (rc_block_scan) -> the loop records, {first, count, index} at the leader in st[1 - fin], and counts.
__global__ __launch_bounds__(256) void contours_scan_kernel(const CtP p, int fin) {
    __shared__ unsigned part[2 * 4];
    for (int n = blockIdx.x; n < p.N; n += gridDim.x) {
        const int total = ct_total(p, n);
        if (total < 0) continue;
        const size_t edge0 = (size_t)n * 2 * p.cap_stride;
        const ct_u32x4 *st = p.st[fin] + edge0;
        ct_u32x4 *info = p.st[1 - fin] + edge0;
        const unsigned *succ = p.succ + edge0;
        const int *rr = p.rr + (size_t)n * p.cap_stride;
        const unsigned edges = 2u * (unsigned)total;
        unsigned carry[2] = {0, 0};                                         // loops, vertices
        for (unsigned e0 = 0; e0 < edges; e0 += 256) {                      // e0 is uniform: every thread makes every pass
            const unsigned e = e0 + threadIdx.x;
            bool lead = false;
            unsigned count = 0;
            if (e < edges && st[e].y == e) {
                const unsigned s = succ[e];
                lead = true;
                count = 2u * (s & 1u) + st[min(s >> 1, edges - 1u)].z;       // its own move and the weight from its successor back to it
            }
            unsigned inc[2] = {lead ? 1u : 0u, count};
            rc_block_scan<2>(inc, carry, part);                             // both in one pass
            if (lead) {
                const unsigned index = inc[0] - 1u, firstv = inc[1] - count;
                info[e] = ct_u32x4{firstv, count, index, 0u};
                if ((long long)index < p.lcap)
                    *reinterpret_cast<ct_i32x4 *>(p.loops + ((size_t)n * p.lcap + index) * 4) =
                        ct_i32x4{rr[e >> 1], (int)firstv, (int)count, (int)(e & 1u)};
            }
        }
        if (threadIdx.x == 0) { p.counts[2 * (size_t)n] = (int)carry[0]; p.counts[2 * (size_t)n + 1] = (int)carry[1]; }
    }
}

__global__ __launch_bounds__(64 * CT_WAVES) void contours_emit_kernel(const CtP p, int fin) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int n = blockIdx.y; n < p.N; n += gridDim.y) {
        const int total = ct_total(p, n);
        if (total <= 0) continue;
        const int *rs = p.rs + (size_t)n * (p.H + 1);
        const unsigned *runs = p.runs + (size_t)n * p.cap_stride;
        const size_t edge0 = (size_t)n * 2 * p.cap_stride;
        const ct_u32x4 *st = p.st[fin] + edge0, *info = p.st[1 - fin] + edge0;
        unsigned *verts = p.verts + (size_t)n * p.vcap;
        const unsigned edges = 2u * (unsigned)total;
        for (int y = blockIdx.x * CT_WAVES + wave; y < p.H; y += gridDim.x * CT_WAVES) {
            int first, last;
            rc_row(rs, y, total, first, last);
            for (int i = first + lane; i < last; i += 64) {
                const int a0 = rc_x0(runs, i, p.W), a1 = rc_x1(runs, i, last, p.W);
                for (int side = 0; side < 2; ++side) {
                    const unsigned e = 2u * (unsigned)i + (unsigned)side;
                    if (!(p.succ[edge0 + e] & 1u)) continue;                // it goes straight on: no corner
                    const ct_u32x4 s = st[e];
                    const unsigned leader = min(s.y, edges - 1u);
                    const ct_u32x4 loop = info[leader];
                    const unsigned count = loop.y;
                    if (count == 0) continue;
                    // the leader's move holds positions 0 and 1; an edge whose weight forward to the leader is d holds count - d
                    unsigned q0 = (count - s.z % count) % count + (leader & 1u);
                    q0 = q0 >= count ? q0 - count : q0;
                    const unsigned q1 = q0 + 1u >= count ? 0u : q0 + 1u;
                    const long long i0 = (long long)loop.x + q0, i1 = (long long)loop.x + q1;
                    if (i0 < p.vcap) verts[i0] = side ? ((unsigned)(y + 1) << 16) | (unsigned)a1 : ((unsigned)y << 16) | (unsigned)a0;
                    if (i1 < p.vcap) verts[i1] = p.endv[edge0 + e];
                }
            }
        }
    }
}

// the rounds of pointer jumping that cover a cycle of 2 cap edges: the smallest K with 2^K >= 2 cap
int ct_rounds(int64_t cap) {
    int k = 1;
    while (((int64_t)1 << k) < 2 * cap) ++k;
    return k;
}

}  // namespace

// per frame and edge slot (2 cap of them): the successor, the corner of its move and two states of 16 bytes
extern "C" size_t arseg_rle_contours_workspace_bytes(int N, int64_t cap) {
    if (N <= 0 || cap <= 0) return 0;
    return (size_t)N * (size_t)cap * 80;
}

extern "C" int arseg_rle_contours_fwd(const int32_t *row_start, const uint32_t *runs, const int32_t *n_regions, const int32_t *run_region,
                                      int64_t cap, int N, int H, int W, int connectivity, int32_t *counts, int32_t *loops, int64_t lcap,
                                      uint32_t *verts, int64_t vcap, void *workspace, size_t workspace_bytes, arseg_stream_t stream) {
    ARSEG_CHECK_PTR(row_start); ARSEG_CHECK_PTR(runs); ARSEG_CHECK_PTR(n_regions); ARSEG_CHECK_PTR(run_region); ARSEG_CHECK_PTR(counts);
    ARSEG_CHECK_POS(N); ARSEG_CHECK_POS(H); ARSEG_CHECK_POS(W);
    if (cap <= 0 || cap > ((int64_t)1 << 29) || lcap < 0 || vcap < 0 || (loops == nullptr && lcap > 0) || (verts == nullptr && vcap > 0))
        return ARSEG_EINVAL;
    if ((connectivity != 4 && connectivity != 8) || H > 65535 || W > 65535) return ARSEG_EINVAL;
    if (rc_misaligned(4, row_start, runs, n_regions, run_region, counts, loops, verts, workspace)) return ARSEG_EINVAL;
    if (workspace_bytes < arseg_rle_contours_workspace_bytes(N, cap)) return ARSEG_EWORKSPACE;
    ARSEG_CHECK_PTR(workspace);
    CtP p = {};
    p.rs = row_start; p.runs = runs; p.nreg = n_regions; p.rr = run_region;
    p.counts = counts; p.loops = lcap ? loops : nullptr; p.verts = vcap ? verts : nullptr;
    const size_t slots = (size_t)N * 2 * (size_t)cap;
    p.st[0] = static_cast<ct_u32x4 *>(workspace);
    p.st[1] = p.st[0] + slots;
    p.succ = reinterpret_cast<unsigned *>(p.st[1] + slots);
    p.endv = p.succ + slots;
    p.cap_stride = cap; p.lcap = p.loops ? lcap : 0; p.vcap = p.verts ? vcap : 0;
    p.cap = (int)cap; p.N = N; p.H = H; p.W = W; p.eight = connectivity == 8;
    hipStream_t st = arseg_stream(stream);
    const dim3 per_row = rc_grid(N, H, CT_WAVES, 4096), per_edge = rc_grid(N, 2 * cap, 256, 4096);
    const int rounds = ct_rounds(cap), fin = rounds & 1;
    hipLaunchKernelGGL(contours_clear_kernel, dim3((unsigned)((N + 255) / 256 < 4096 ? (N + 255) / 256 : 4096)), dim3(256), 0, st, p);
    hipLaunchKernelGGL(contours_succ_kernel, per_row, dim3(64 * CT_WAVES), 0, st, p);
    for (int k = 0; k < rounds; ++k) hipLaunchKernelGGL(contours_jump_kernel, per_edge, dim3(256), 0, st, p, k & 1);
    hipLaunchKernelGGL(contours_scan_kernel, rc_frames(N), dim3(256), 0, st, p, fin);
    if (p.vcap > 0) hipLaunchKernelGGL(contours_emit_kernel, per_row, dim3(64 * CT_WAVES), 0, st, p, fin);          // not in a sizing pass
    return arseg_launch_status();
}
