// Region outlines simplified with shared borders (include/arseg_hip.h, arseg_contours_simplify_shared_fwd): counts, loops and verts as
// arseg_rle_contours_fwd leaves them and the run code they were traced from in; per loop its corners plus the junctions inside its
// straight edges (the expanded loop), cut into arcs at every junction passage, and of each arc the vertices that Douglas-Peucker keeps
// under a rule that does not depend on the direction of travel -- so the two loops that share an arc keep the same vertices of it --
// out, in the layout of arseg_contours_simplify_fwd.  Integers throughout: every output is a pure function of the inputs.
//
// Scratch lives in the caller's workspace, per frame: per loop slot the kept count (int32 [lcap]) and {first, count} of its expanded
// loop (int32 [lcap][2]); per vertex slot the offset of the vertex in its expanded loop (int32 [vcap]); per expanded slot, ecap = vcap +
// 2 cap of them, the vertex word (uint32) and a byte: the junction mark, which the walk turns into the keep flag.
// 7 launches, sized on the host from the capacities; a phase boundary is a launch boundary: no workgroup waits for another, nothing spins
// on memory, no atomics are needed.
//   mark     a lane owns a source vertex, whatever its loop (the loop is found by a binary search over the loop records, which are in
//            order of their first vertices): the junctions strictly inside the edge to the next vertex are counted -- on a horizontal
//            edge the runs of the outside row that begin inside it (two binary searches), on a vertical edge the rows at which the
//            outside column changes its value (a lane walks up to SS_SERIAL rows itself; a longer edge is taken by the whole wave, a
//            lane per row) -- and 1 + count stored.  A search is a chain of dependent loads; with a lane per vertex of the frame the
//            chains of all vertices run side by side instead of 64 at a time along the longest loop.
//   place    a wave owns a loop: 1 + count scanned over the loop in place: the vertex' offset in the expanded loop, the loop's
//            expanded count.
//   scan     one workgroup per frame: the refusal decision (counts_out = {-1, -1}); the prefix (rc_block_scan) over the loops' expanded
//            counts -> the first slot of every expanded loop.
//   expand   a lane owns a source vertex, as in mark: the vertex to its slot with its junction byte (the four pixels around it from the
//            run code: degree >= 3, or a frame corner), the junctions inside its edge behind it, found as in mark, with byte 1.
//   keep     a wave owns a loop: from its first junction passage (position 0 without one) cyclically, arc by arc -- an arc ends at the
//            next marked byte, and no byte inside it is set before its turn --: a closed arc first gets the position farthest from its
//            start; then simplify.hip's recursion without a stack on the flags, with the key {c, smallest vertex word}, the position
//            taken from the lane that holds the winning word (an arc visits no point twice); a closed arc that kept fewer than 3 is
//            flagged whole.  A flag the walk reads back is stored by every lane (the position is uniform), so program order alone makes
//            it visible.  An expanded loop of at most SS_STAGE slots is walked in the wave's own LDS, a longer one in place.
//   scan     the prefix over the kept counts -> counts_out and the loop records.
//   emit     a wave owns a loop: the flagged slots compacted in order with a ballot prefix to first'; words below vcap_out only.  Not
//            launched without verts_out.
//
// Bounds of the loops (nothing else loops):
//   grid-stride loops      over frames, loops, the vertices of a frame or a loop, the rows of an edge, the slots of an expanded loop:
//                          counted.
//   binary searches        rc_cover and the search for a vertex' loop: at most 31 rounds each.
//   the walk               every round keeps a vertex, advances to the next kept position or opens an arc: within 3 count + 1 rounds,
//                          and the loops are given 4 count + 8 explicitly.
//   the searches for flags 64 per round up to the arc's or the loop's end: counted.
// Clamps: a frame is processed only with 0 <= L <= lcap, 0 <= V <= vcap and row_start[H] <= cap; a loop's first is clamped into [0, V]
// and its count into [0, V - first]; a row's runs into the frame's stored runs (rc_row), so every run index stays below cap; a vertex'
// coordinates into [0, W] x [0, H] before a row or a column is taken from them, and a pixel outside the frame has no value; an expanded
// slot is written only below ecap and only below the offset of the next source vertex; an expanded loop's first is clamped into [0, ecap]
// and its count into [0, ecap - first], so every index into the LDS stage stays below count <= SS_STAGE; a position taken from a lane is
// clamped into the segment it was found in; an output index is used only below vcap_out, a loop index only below L <= lcap.  Offsets are
// summed as unsigned words.  Coordinates are taken as 16-bit fields and multiplied as unsigned words: a malformed vertex gives a
// meaningless product, never a trap.  No division is made.  Malformed input gives meaningless output and touches nothing outside the
// caller's buffers.
#include "runcode.h"

namespace {

typedef int ss_i32x4 __attribute__((ext_vector_type(4), aligned(4)));
typedef unsigned long long ss_u64;

constexpr int SS_WAVES = 4;                             // waves (= loops in flight) per workgroup
constexpr int SS_STAGE = 2048;                          // the longest expanded loop a wave stages in LDS: 10 KiB per wave, 40 per workgroup
constexpr int SS_SERIAL = 8;                            // the rows (or inserted vertices) of an edge a lane handles on its own

struct SsP {
    const int *row_start;                               // [N][H + 1]
    const unsigned *runs;                               // [N][cap]
    const int *counts;                                  // [N][2]
    const int *loops;                                   // [N][lcap][4]
    const unsigned *verts;                              // [N][vcap]
    int *counts_out;                                    // [N][2]
    int *loops_out;                                     // [N][lcap][4]
    unsigned *verts_out;                                // [N][vcap_out] (may be null: vcap_out == 0)
    int *kept;                                          // [N][lcap]
    unsigned *eloop;                                    // [N][lcap][2] = {first slot, slots} of the expanded loop
    unsigned *eoff;                                     // [N][vcap]: the vertex' offset in its expanded loop
    unsigned *ep;                                       // [N][ecap]: the expanded loops
    unsigned char *ef;                                  // [N][estride]: junction marks, then keep flags
    long long cap, lcap, vcap, vcap_out, ecap, estride;
    ss_u64 tol;                                         // 16 x the squared tolerance
    int N, H, W, ecap_k;                                // ecap_k: ecap as an index bound, below 2^31
};

struct SsFrame {
    const int *rs;
    const unsigned *runs;
    int L, V, total;                                    // loops, vertices, stored runs
};

// The loops, vertices and run code of a frame; false for a frame that is refused: its source was refused or overflowed.
__device__ __forceinline__ bool ss_frame(const SsP &p, int n, SsFrame &f) {
    f.L = p.counts[2 * (size_t)n]; f.V = p.counts[2 * (size_t)n + 1];
    f.rs = p.row_start + (size_t)n * (p.H + 1);
    f.runs = p.runs + (size_t)n * p.cap;
    f.total = rc_stored(f.rs[p.H], (int)p.cap);                                  // (cap <= 1 << 29)
    return f.L >= 0 && f.V >= 0 && f.L <= p.lcap && f.V <= p.vcap && f.total >= 0;
}

// A loop's record -> its first vertex and its count, clamped into the frame's V vertices.
__device__ __forceinline__ void ss_loop(const SsP &p, int n, int l, int V, int &first, int &cnt) {
    const int *rec = p.loops + ((size_t)n * p.lcap + l) * 4;
    first = rc_clamp(rec[1], 0, V);
    cnt = rc_clamp(rec[2], 0, V - first);
}

// A loop's expanded first slot and count, clamped into the frame's ecap slots.
__device__ __forceinline__ void ss_expanded(const SsP &p, int n, int l, int &first, int &cnt) {
    const unsigned *rec = p.eloop + ((size_t)n * p.lcap + l) * 2;
    first = (int)min(rec[0], (unsigned)p.ecap_k);
    cnt = (int)min(rec[1], (unsigned)(p.ecap_k - first));
}

// The value of pixel (x, y); -1 outside the frame (or in a row without runs).
__device__ __forceinline__ int ss_val(const SsP &p, const SsFrame &f, int y, int x) {
    if (y < 0 || y >= p.H || x < 0 || x >= p.W) return -1;
    int first, last;
    rc_row(f.rs, y, f.total, first, last);
    return first < last ? (int)(f.runs[rc_cover(f.runs, first, last, x)] & 0xffu) : -1;
}

// The values of pixels (x - 1, y) and (x, y) with one search.
__device__ __forceinline__ void ss_pair(const SsP &p, const SsFrame &f, int y, int x, int &vl, int &vr) {
    vl = vr = -1;
    if (y < 0 || y >= p.H || x < 0 || x > p.W) return;
    int first, last;
    rc_row(f.rs, y, f.total, first, last);
    if (first >= last) return;
    if (x == 0) { vr = (int)(f.runs[first] & 0xffu); return; }
    const int i = rc_cover(f.runs, first, last, x - 1);
    vl = (int)(f.runs[i] & 0xffu);
    if (x < p.W) vr = (int)(f.runs[i + 1 < last && (int)(f.runs[i + 1] >> 8) <= x ? i + 1 : i] & 0xffu);
}

// Is the grid corner w a junction: at least 3 of its four grid edges separate two values (or a pixel from the outside), or a frame corner.
__device__ __forceinline__ bool ss_junction(const SsP &p, const SsFrame &f, unsigned w) {
    const int x = (int)(w & 0xffffu), y = (int)(w >> 16);
    int a, b, c, d;
    ss_pair(p, f, y - 1, x, a, b);
    ss_pair(p, f, y, x, c, d);
    const int degree = (a != b) + (c != d) + (a != c) + (b != d);
    return degree >= 3 || ((x == 0 || x == p.W) && (y == 0 || y == p.H));
}

// The edge from a source vertex to the next one, as far as the junctions inside it go.
struct SsEdge {
    int kind;                                           // 0: nothing inside, 1: horizontal, 2: vertical
    int n;                                              // horizontal: the junctions inside; vertical: the rows to look at
    int at, step;                                       // horizontal: the first run in travel order; vertical: the first row; +1 or -1
    int fixed, col;                                     // horizontal: y; vertical: x, and the outside column
};

__device__ __forceinline__ SsEdge ss_edge(const SsP &p, const SsFrame &f, unsigned w, unsigned wn) {
    SsEdge e = {};
    const int x = min((int)(w & 0xffffu), p.W), y = min((int)(w >> 16), p.H), xn = min((int)(wn & 0xffffu), p.W), yn = min((int)(wn >> 16), p.H);
    if (y == yn && x != xn) {                                                // the region is below an edge heading east, above one heading west
        const bool east = xn > x;
        const int row = east ? y - 1 : y, lo = min(x, xn), hi = max(x, xn);
        if (row < 0 || row >= p.H || hi - lo < 2) return e;
        int first, last;
        rc_row(f.rs, row, f.total, first, last);
        if (first >= last) return e;
        const int i_lo = rc_cover(f.runs, first, last, lo), i_hi = rc_cover(f.runs, first, last, hi - 1);      // the runs that begin in (lo, hi)
        e.n = max(i_hi - i_lo, 0); e.kind = e.n > 0 ? 1 : 0;
        e.at = east ? i_lo + 1 : i_hi; e.step = east ? 1 : -1; e.fixed = y;
    } else if (x == xn && y != yn) {                                         // the region is left of an edge heading south, right of one heading north
        const bool south = yn > y;
        const int col = south ? x : x - 1, len = south ? yn - y : y - yn;
        if (col < 0 || col >= p.W || len < 2) return e;
        e.kind = 2; e.n = len - 1; e.at = south ? y + 1 : y - 1; e.step = south ? 1 : -1; e.fixed = x; e.col = col;
    }
    return e;
}

// A junction inside an edge -> its expanded slot.
__device__ __forceinline__ void ss_put(const SsP &p, int n, long long slot, unsigned word) {
    if (slot >= 0 && slot < p.ecap_k) {
        p.ep[(size_t)n * p.ecap + slot] = word;
        p.ef[(size_t)n * p.estride + slot] = 1;
    }
}

// The rows of a vertical edge by one lane: corner (x, r) is a junction iff the outside column changes between rows r - 1 and r.
template <bool WRITE>
__device__ __forceinline__ int ss_vertical_lane(const SsP &p, const SsFrame &f, int n, const SsEdge &e, long long slot, int allot) {
    int found = 0, prev = ss_val(p, f, e.step > 0 ? e.at - 1 : e.at, e.col);
    for (int k = 0; k < e.n; ++k) {
        const int r = e.at + e.step * k, cur = ss_val(p, f, e.step > 0 ? r : r - 1, e.col);
        if (cur != prev) {
            if (WRITE && found < allot) ss_put(p, n, slot + found, ((unsigned)r << 16) | (unsigned)e.fixed);
            ++found;
        }
        prev = cur;
    }
    return found;
}

// The same by the whole wave, a lane per row (e is uniform).
template <bool WRITE>
__device__ __forceinline__ int ss_vertical_wave(const SsP &p, const SsFrame &f, int n, const SsEdge &e, long long slot, int allot, int lane) {
    int found = 0;
    for (int base = 0; base < e.n; base += 64) {
        const int k = base + lane, r = e.at + e.step * k;
        const bool t = k < e.n && ss_val(p, f, r - 1, e.col) != ss_val(p, f, r, e.col);
        const ss_u64 m = __builtin_amdgcn_ballot_w64(t);
        const int to = found + __builtin_popcountll(m & ((1ull << lane) - 1ull));
        if (WRITE && t && to < allot) ss_put(p, n, slot + to, ((unsigned)r << 16) | (unsigned)e.fixed);
        found += __builtin_popcountll(m);
    }
    return found;
}

// An edge of lane src to every lane.
__device__ __forceinline__ SsEdge ss_edge_of(const SsEdge &e, int src) {
    SsEdge u;
    u.kind = __shfl(e.kind, src, 64); u.n = __shfl(e.n, src, 64); u.at = __shfl(e.at, src, 64); u.step = __shfl(e.step, src, 64);
    u.fixed = __shfl(e.fixed, src, 64); u.col = __shfl(e.col, src, 64);
    return u;
}

// The loop that holds vertex v of a frame with L >= 1 loops: the last one whose first vertex is at or before v (the records are in
// order of their first vertices); its first vertex and its count.  False for a vertex that no loop holds.
__device__ __forceinline__ bool ss_owner(const SsP &p, int n, const SsFrame &f, int v, int &l, int &first, int &cnt) {
    const int *rec = p.loops + (size_t)n * p.lcap * 4;
    int lo = 0, hi = f.L;
    while (hi - lo > 1) {                                                    // at most 31 rounds
        const int mid = (lo + hi) >> 1;
        if (rc_clamp(rec[4 * (size_t)mid + 1], 0, f.V) <= v) lo = mid; else hi = mid;
    }
    l = lo;
    ss_loop(p, n, l, f.V, first, cnt);
    return v >= first && v - first < cnt;
}

__global__ __launch_bounds__(256) void simplify_shared_mark_kernel(const SsP p) {
    const int lane = threadIdx.x & 63;
    for (int n = blockIdx.y; n < p.N; n += gridDim.y) {
        SsFrame f;
        if (!ss_frame(p, n, f) || f.L < 1) continue;
        const unsigned *P = p.verts + (size_t)n * p.vcap;
        unsigned *O = p.eoff + (size_t)n * p.vcap;
        for (int base = blockIdx.x * 256; base < f.V; base += gridDim.x * 256) {             // base is uniform: every lane makes every pass
            const int i = base + (int)threadIdx.x;
            int l, first, cnt;
            const bool mine = i < f.V && ss_owner(p, n, f, i, l, first, cnt);
            SsEdge e = {};
            if (mine) e = ss_edge(p, f, P[i], P[i + 1 < first + cnt ? i + 1 : first]);
            const bool wide = e.kind == 2 && e.n > SS_SERIAL;
            int inside = e.kind == 1 ? e.n : 0;
            if (e.kind == 2 && !wide) inside = ss_vertical_lane<false>(p, f, n, e, 0, 0);
            for (ss_u64 m = __builtin_amdgcn_ballot_w64(wide); m; m &= m - 1) {
                const int src = __builtin_ctzll(m);
                const int found = ss_vertical_wave<false>(p, f, n, ss_edge_of(e, src), 0, 0, lane);
                if (lane == src) inside = found;
            }
            if (i < f.V) O[i] = mine ? 1u + (unsigned)inside : 0u;
        }
    }
}

// Per loop, by a wave: 1 + count of its vertices scanned in place -> the vertex' offset in the expanded loop, the loop's expanded count.
__global__ __launch_bounds__(64 * SS_WAVES) void simplify_shared_place_kernel(const SsP p) {
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    for (int n = blockIdx.y; n < p.N; n += gridDim.y) {
        SsFrame f;
        if (!ss_frame(p, n, f)) continue;
        for (int l = blockIdx.x * SS_WAVES + wave; l < f.L; l += gridDim.x * SS_WAVES) {             // waves beyond L leave at once
            int first, cnt;
            ss_loop(p, n, l, f.V, first, cnt);
            first = __builtin_amdgcn_readfirstlane(first); cnt = __builtin_amdgcn_readfirstlane(cnt);
            unsigned *O = p.eoff + (size_t)n * p.vcap + first;
            unsigned carry = 0;
            for (int base = 0; base < cnt; base += 256) {                    // four loads in flight per lane
                unsigned own[4], inc[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) own[u] = base + 64 * u + lane < cnt ? O[base + 64 * u + lane] : 0u;
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    inc[u] = own[u];
#pragma unroll
                    for (int o = 1; o < 64; o <<= 1) {
                        const unsigned t = __shfl_up(inc[u], o, 64);
                        inc[u] += lane >= o ? t : 0u;
                    }
                }
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    if (base + 64 * u + lane < cnt) O[base + 64 * u + lane] = carry + inc[u] - own[u];
                    carry += __shfl(inc[u], 63, 64);
                }
            }
            if (lane == 0) p.eloop[((size_t)n * p.lcap + l) * 2 + 1] = carry;
        }
    }
}

// Per frame: refused or not; the loops' expanded counts summed, 256 at a time with a carry -> the first slot of every expanded loop.
__global__ __launch_bounds__(256) void simplify_shared_offsets_kernel(const SsP p) {
    __shared__ unsigned part[4];
    for (int n = blockIdx.x; n < p.N; n += gridDim.x) {
        SsFrame f;
        const bool ok = ss_frame(p, n, f);
        if (threadIdx.x == 0) { p.counts_out[2 * (size_t)n] = ok ? 0 : -1; p.counts_out[2 * (size_t)n + 1] = ok ? 0 : -1; }
        if (!ok) continue;
        unsigned carry = 0;
        for (int l0 = 0; l0 < f.L; l0 += 256) {                              // l0 is uniform: every thread makes every pass
            const int l = l0 + (int)threadIdx.x;
            const unsigned count = l < f.L ? p.eloop[((size_t)n * p.lcap + l) * 2 + 1] : 0u;
            unsigned inc = count;
            rc_block_scan<1>(&inc, &carry, part);
            if (l < f.L) p.eloop[((size_t)n * p.lcap + l) * 2] = inc - count;
        }
    }
}

__global__ __launch_bounds__(256) void simplify_shared_expand_kernel(const SsP p) {
    const int lane = threadIdx.x & 63;
    for (int n = blockIdx.y; n < p.N; n += gridDim.y) {
        SsFrame f;
        if (!ss_frame(p, n, f) || f.L < 1) continue;
        const unsigned *P = p.verts + (size_t)n * p.vcap;
        const unsigned *O = p.eoff + (size_t)n * p.vcap;
        for (int base = blockIdx.x * 256; base < f.V; base += gridDim.x * 256) {
            const int i = base + (int)threadIdx.x;
            int l, first, cnt;
            SsEdge e = {};
            long long slot = 0;
            int allot = 0;
            if (i < f.V && ss_owner(p, n, f, i, l, first, cnt)) {
                const unsigned *rec = p.eloop + ((size_t)n * p.lcap + l) * 2;
                const bool last = i + 1 >= first + cnt;
                const unsigned w = P[i], off = O[i], next = last ? rec[1] : O[i + 1];
                slot = (long long)rec[0] + off;
                allot = (int)min(next - off - 1u, 0x7fffffffu);              // the slots the mark launch counted behind this vertex
                if (slot < p.ecap_k) {
                    p.ep[(size_t)n * p.ecap + slot] = w;
                    p.ef[(size_t)n * p.estride + slot] = ss_junction(p, f, w) ? 1 : 0;
                }
                e = ss_edge(p, f, w, P[last ? first : i + 1]);
                if (e.kind == 1) e.n = min(e.n, allot);
                ++slot;
            }
            const bool wide = e.kind != 0 && e.n > SS_SERIAL;
            if (e.kind == 1 && !wide) {
                for (int k = 0; k < e.n; ++k) ss_put(p, n, slot + k, ((unsigned)e.fixed << 16) | (unsigned)rc_x0(f.runs, e.at + e.step * k, p.W));
            } else if (e.kind == 2 && !wide) {
                ss_vertical_lane<true>(p, f, n, e, slot, allot);
            }
            for (ss_u64 m = __builtin_amdgcn_ballot_w64(wide); m; m &= m - 1) {
                const int src = __builtin_ctzll(m);
                const SsEdge u = ss_edge_of(e, src);
                const long long to = __shfl(slot, src, 64);
                const int room = __shfl(allot, src, 64);
                if (u.kind == 1) {
                    for (int k = lane; k < u.n; k += 64) ss_put(p, n, to + k, ((unsigned)u.fixed << 16) | (unsigned)rc_x0(f.runs, u.at + u.step * k, p.W));
                } else {
                    ss_vertical_wave<true>(p, f, n, u, to, room, lane);
                }
            }
        }
    }
}

// {value, smallest vertex word} as one key: the larger value wins, then the smaller word.
__device__ __forceinline__ ss_u64 ss_key(unsigned value, unsigned word) { return ((ss_u64)value << 32) | (0xffffffffu - word); }

__device__ __forceinline__ unsigned ss_abs(unsigned v) { return (int)v < 0 ? 0u - v : v; }

// The first flagged position in [from, to), or `to`: 64 flags per round.  at: the rotation of the loop.
__device__ __forceinline__ int ss_next(const unsigned char *F, int from, int to, int rot, int E, int lane) {
    for (int base = from; base < to; base += 64) {
        int i = min(base + lane, to - 1) + rot;
        i = i >= E ? i - E : i;
        const ss_u64 m = __builtin_amdgcn_ballot_w64(base + lane < to && F[i] != 0);
        if (m) return base + __builtin_ctzll(m);
    }
    return to;
}

// The arcs of one expanded loop of E >= 1 slots, by one wave: P its vertices, F its junction marks, both in global memory or both in the
// wave's LDS stage -> the number of flags set when it is done.  Everything but the strided scans is uniform.
__device__ __forceinline__ int ss_walk(const unsigned *P, unsigned char *F, int E, ss_u64 tol, int lane) {
    // positions count from the first junction passage: position i is slot i + rot, cyclically, and position E closes the loop
    const int j0 = ss_next(F, 0, E, 0, E, lane), rot = j0 < E ? j0 : 0;
    auto at = [&](int i) { i += rot; return i >= E ? i - E : i; };
    const int limit = 4 * E + 8;
    int total = 0, round = 0;
    for (int a = 0; a < E && round < limit; ++round) {
        // ---- the arc from a: its end is the next mark (nothing inside it is flagged yet)
        const int end = ss_next(F, a + 1, E, rot, E, lane);
        const unsigned wa = P[at(a)];
        const bool closed = P[at(end)] == wa;
        F[at(a)] = 1;                                                        // (the start of a loop without a junction is no mark)
        int kept = 1, b = end;
        if (closed && end - a > 1) {                                         // the farthest position from the start, the smallest word of a tie
            const unsigned x0 = wa & 0xffffu, y0 = wa >> 16;
            ss_u64 key = 0;
            int pos = a + 1;
            for (int base = a + 1; base < end; base += 64) {
                const int i = base + lane;
                const unsigned w = P[at(min(i, end - 1))], dx = (w & 0xffffu) - x0, dy = (w >> 16) - y0;
                const ss_u64 k = ss_key(dx * dx + dy * dy, w);
                if (i < end && k > key) { key = k; pos = i; }
            }
            const ss_u64 best = wave_max_u64(key);
            const ss_u64 who = __builtin_amdgcn_ballot_w64(key == best);
            const int a1 = rc_clamp(__shfl(pos, who ? __builtin_ctzll(who) : 0, 64), a + 1, end - 1);
            F[at(a1)] = 1;                                                   // every lane stores: see the head of the file
            kept = 2; b = a1;
        }
        // ---- the walk: aa is final, b the next kept position after it
        for (int aa = a; aa < end && round < limit; ++round) {
            bool marked = false;
            if (b - aa > 1) {
                const unsigned w0 = P[at(aa)], wb = P[at(b)];
                const unsigned xa = w0 & 0xffffu, ya = w0 >> 16, ex = (wb & 0xffffu) - xa, ey = (wb >> 16) - ya;
                ss_u64 key = 0;
                int pos = aa + 1;
                for (int base = aa + 1; base < b; base += 256) {
                    unsigned w[4];
#pragma unroll
                    for (int u = 0; u < 4; ++u) w[u] = P[at(min(base + 64 * u + lane, b - 1))];
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        const int i = base + 64 * u + lane;
                        const unsigned c = ss_abs(ex * ((w[u] >> 16) - ya) - ey * ((w[u] & 0xffffu) - xa));      // 32-bit products
                        const ss_u64 k = ss_key(c, w[u]);
                        if (i < b && k > key) { key = k; pos = i; }
                    }
                }
                const ss_u64 best = wave_max_u64(key);
                const ss_u64 c = best >> 32, len2 = (ss_u64)(ex * ex + ey * ey);
                if (16ull * c * c > tol * len2) {                            // uniform: the one 64-bit comparison of the segment
                    const ss_u64 who = __builtin_amdgcn_ballot_w64(key == best);
                    const int i = rc_clamp(__shfl(pos, who ? __builtin_ctzll(who) : 0, 64), aa + 1, b - 1);
                    F[at(i)] = 1;
                    ++kept; b = i; marked = true;
                }
            }
            if (!marked) {                                                   // every interior vertex of (aa, b) is dropped
                aa = b;
                b = ss_next(F, aa + 1, end, rot, E, lane);
            }
        }
        if (closed && kept < 3) {                                            // no collapse of a closed arc: all of it stays
            for (int i = a + 1 + lane; i < end; i += 64) F[at(i)] = 1;
            kept = end - a;
        }
        total += kept;
        a = end;
    }
    return total;
}

__global__ __launch_bounds__(64 * SS_WAVES) void simplify_shared_keep_kernel(const SsP p) {
    __shared__ unsigned stage_p[SS_WAVES][SS_STAGE];
    __shared__ unsigned stage_f[SS_WAVES][SS_STAGE / 4];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    for (int n = blockIdx.y; n < p.N; n += gridDim.y) {
        SsFrame f;
        if (!ss_frame(p, n, f)) continue;
        for (int l = blockIdx.x * SS_WAVES + wave; l < f.L; l += gridDim.x * SS_WAVES) {
            int first, E;
            ss_expanded(p, n, l, first, E);
            first = __builtin_amdgcn_readfirstlane(first); E = __builtin_amdgcn_readfirstlane(E);
            const unsigned *P = p.ep + (size_t)n * p.ecap + first;
            unsigned char *F = p.ef + (size_t)n * p.estride + first;
            int kept = 0;
            if (E >= 1 && E <= SS_STAGE) {
                // the loop and its marks staged in the wave's own LDS: a round of the walk costs LDS latencies instead of L2's.  Only
                // this wave touches its stage; a wave's LDS accesses are served in order, and the fences keep the compiler from moving
                // an access across them.
                unsigned *sp = stage_p[wave];
                unsigned char *sf = reinterpret_cast<unsigned char *>(stage_f[wave]);
                for (int i = lane; i < E; i += 64) { sp[i] = P[i]; sf[i] = F[i]; }
                __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
                __builtin_amdgcn_wave_barrier();
                kept = ss_walk(sp, sf, E, p.tol, lane);
                __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
                __builtin_amdgcn_wave_barrier();
                for (int i = lane; i < E; i += 64) F[i] = sf[i];
            } else if (E >= 1) {
                kept = ss_walk(P, F, E, p.tol, lane);                        // a longer loop: in place, on the marks the expand launch wrote
            }
            if (lane == 0) p.kept[(size_t)n * p.lcap + l] = kept;
        }
    }
}

// Per frame: the kept counts summed over the loops, 256 at a time with a carry (rc_block_scan) -> the loop records and counts_out.
__global__ __launch_bounds__(256) void simplify_shared_scan_kernel(const SsP p) {
    __shared__ unsigned part[4];
    for (int n = blockIdx.x; n < p.N; n += gridDim.x) {
        SsFrame f;
        if (!ss_frame(p, n, f)) continue;
        unsigned carry = 0;
        for (int l0 = 0; l0 < f.L; l0 += 256) {                              // l0 is uniform: every thread makes every pass
            const int l = l0 + (int)threadIdx.x;
            const unsigned count = l < f.L ? (unsigned)p.kept[(size_t)n * p.lcap + l] : 0u;
            unsigned inc = count;
            rc_block_scan<1>(&inc, &carry, part);
            if (l < f.L) {
                const ss_i32x4 rec = *reinterpret_cast<const ss_i32x4 *>(p.loops + ((size_t)n * p.lcap + l) * 4);
                *reinterpret_cast<ss_i32x4 *>(p.loops_out + ((size_t)n * p.lcap + l) * 4) = ss_i32x4{rec.x, (int)(inc - count), (int)count, rec.w};
            }
        }
        if (threadIdx.x == 0) { p.counts_out[2 * (size_t)n] = f.L; p.counts_out[2 * (size_t)n + 1] = (int)carry; }
    }
}

__global__ __launch_bounds__(64 * SS_WAVES) void simplify_shared_emit_kernel(const SsP p) {
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    for (int n = blockIdx.y; n < p.N; n += gridDim.y) {
        SsFrame f;
        if (!ss_frame(p, n, f)) continue;
        unsigned *out = p.verts_out + (size_t)n * p.vcap_out;
        for (int l = blockIdx.x * SS_WAVES + wave; l < f.L; l += gridDim.x * SS_WAVES) {
            int first, E;
            ss_expanded(p, n, l, first, E);
            const unsigned *P = p.ep + (size_t)n * p.ecap + first;
            const unsigned char *F = p.ef + (size_t)n * p.estride + first;
            long long to0 = (long long)(unsigned)p.loops_out[((size_t)n * p.lcap + l) * 4 + 1];
            for (int base = 0; base < E; base += 64) {
                const int i = base + lane;
                const bool keep = i < E && F[min(i, E - 1)] != 0;
                const ss_u64 m = __builtin_amdgcn_ballot_w64(keep);
                const long long to = to0 + __builtin_popcountll(m & ((1ull << lane) - 1ull));
                if (keep && to < p.vcap_out) out[to] = P[i];
                to0 += __builtin_popcountll(m);
            }
        }
    }
}

// the slots of a frame's expanded loops: an expanded loop adds at most one vertex per end of an interior vertical unit border edge
bool ss_expanded_capacity(int64_t cap, int64_t vcap, size_t &ecap) {
    size_t twice;
    return !__builtin_mul_overflow((size_t)cap, (size_t)2, &twice) && !__builtin_add_overflow(twice, (size_t)vcap, &ecap);
}

}  // namespace

// per frame: 12 bytes per loop slot (the kept count, the expanded loop's first slot and count), 4 bytes per vertex slot (its offset in the
// expanded loop) and 5 bytes per expanded slot, vcap + 2 cap of them (the word, and the mark rounded up to 4 per frame), rounded up to
// 16 bytes in all; a size that does not fit size_t comes back as its largest value, which no workspace has
extern "C" size_t arseg_contours_simplify_shared_workspace_bytes(int N, int64_t cap, int64_t lcap, int64_t vcap) {
    if (N <= 0 || cap <= 0 || lcap < 0 || vcap < 0) return 0;
    const size_t none = ~(size_t)0;
    size_t ecap, loops, verts, words, marks, frame, bytes;
    if (!ss_expanded_capacity(cap, vcap, ecap) || ecap > none - 3) return none;
    marks = (ecap + 3) & ~(size_t)3;
    if (__builtin_mul_overflow((size_t)lcap, (size_t)12, &loops) || __builtin_mul_overflow((size_t)vcap, (size_t)4, &verts) ||
        __builtin_mul_overflow(ecap, (size_t)4, &words) || __builtin_add_overflow(loops, verts, &frame) ||
        __builtin_add_overflow(frame, words, &frame) || __builtin_add_overflow(frame, marks, &frame) ||
        __builtin_mul_overflow(frame, (size_t)N, &bytes) || bytes > none - 15)
        return none;
    return (bytes + 15) & ~(size_t)15;
}

extern "C" int arseg_contours_simplify_shared_fwd(const int32_t *row_start, const uint32_t *runs, int64_t cap, const int32_t *counts,
                                                  const int32_t *loops, int64_t lcap, const uint32_t *verts, int64_t vcap, int N, int H, int W,
                                                  int64_t tol2_q, int32_t *counts_out, int32_t *loops_out, uint32_t *verts_out,
                                                  int64_t vcap_out, void *workspace, size_t workspace_bytes, arseg_stream_t stream) {
    ARSEG_CHECK_PTR(row_start); ARSEG_CHECK_PTR(runs); ARSEG_CHECK_PTR(counts); ARSEG_CHECK_PTR(counts_out);
    ARSEG_CHECK_POS(N); ARSEG_CHECK_POS(H); ARSEG_CHECK_POS(W); ARSEG_CHECK_POS(cap);
    if (lcap < 0 || vcap < 0 || vcap_out < 0 || ((loops == nullptr || loops_out == nullptr) && lcap > 0) || (verts == nullptr && vcap > 0) ||
        (verts_out == nullptr && vcap_out > 0))
        return ARSEG_EINVAL;
    if (H > 16384 || W > 16384 || tol2_q < 0 || tol2_q > ((int64_t)1 << 30) || cap > ((int64_t)1 << 29)) return ARSEG_EINVAL;
    if (rc_misaligned(4, row_start, runs, counts, loops, verts, counts_out, loops_out, verts_out) || rc_misaligned(4, workspace)) return ARSEG_EINVAL;
    const void *ins[] = {row_start, runs, counts, loops, verts};
    const void *outs[] = {counts_out, loops_out, verts_out};
    for (const void *o : outs)
        for (const void *i : ins)
            if (o != nullptr && o == i) return ARSEG_EINVAL;                   // an output may not be an input
    const size_t need = arseg_contours_simplify_shared_workspace_bytes(N, cap, lcap, vcap);
    if (need == ~(size_t)0 || workspace_bytes < need) return ARSEG_EWORKSPACE;
    ARSEG_CHECK_PTR(workspace);
    size_t ecap = 0;
    ss_expanded_capacity(cap, vcap, ecap);
    SsP p = {};
    p.row_start = row_start; p.runs = runs; p.counts = counts; p.loops = loops; p.verts = verts;
    p.counts_out = counts_out; p.loops_out = loops_out; p.verts_out = vcap_out ? verts_out : nullptr;
    p.cap = cap; p.lcap = lcap; p.vcap = vcap; p.vcap_out = p.verts_out ? vcap_out : 0;
    p.ecap = (long long)ecap; p.estride = (long long)((ecap + 3) & ~(size_t)3); p.ecap_k = rc_cap((int64_t)ecap);
    p.kept = static_cast<int *>(workspace);
    p.eloop = reinterpret_cast<unsigned *>(p.kept + (size_t)N * (size_t)lcap);
    p.eoff = p.eloop + 2 * (size_t)N * (size_t)lcap;
    p.ep = p.eoff + (size_t)N * (size_t)vcap;
    p.ef = reinterpret_cast<unsigned char *>(p.ep + (size_t)N * ecap);
    p.tol = (ss_u64)tol2_q; p.N = N; p.H = H; p.W = W;
    hipStream_t st = arseg_stream(stream);
    const dim3 per_loop = rc_grid(N, lcap, SS_WAVES, 4096);
    const dim3 per_vertex = rc_grid(N, vcap, 256, 4096);
    hipLaunchKernelGGL(simplify_shared_mark_kernel, per_vertex, dim3(256), 0, st, p);
    hipLaunchKernelGGL(simplify_shared_place_kernel, per_loop, dim3(64 * SS_WAVES), 0, st, p);
    hipLaunchKernelGGL(simplify_shared_offsets_kernel, rc_frames(N), dim3(256), 0, st, p);
    hipLaunchKernelGGL(simplify_shared_expand_kernel, per_vertex, dim3(256), 0, st, p);
    hipLaunchKernelGGL(simplify_shared_keep_kernel, per_loop, dim3(64 * SS_WAVES), 0, st, p);
    hipLaunchKernelGGL(simplify_shared_scan_kernel, rc_frames(N), dim3(256), 0, st, p);
    if (p.vcap_out > 0) hipLaunchKernelGGL(simplify_shared_emit_kernel, per_loop, dim3(64 * SS_WAVES), 0, st, p);      // not in a sizing pass
    return arseg_launch_status();
}
