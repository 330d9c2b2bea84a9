// Region polygons rasterised back to a label plane, with the fidelity counters (include/arseg_hip.h, arseg_contours_fill_fwd): counts, loops
// and verts as arseg_rle_contours_fwd, arseg_contours_simplify_fwd or arseg_contours_simplify_shared_fwd leave them and the regions' values
// in; per frame the plane a consumer of the polygons draws (even-odd per region, the larger region number on top), the crossings it needed
// and gaps, excess, changed and the per-value areas against a reference plane out.  Integers throughout: every output is a pure function of
// the inputs, whatever order the atomics arrive in.  The load is a few tens of crossings per row: the launches are bound by latency.
//
// A crossing is one word (region << 16) | xs: the edge of a loop of `region` passes row y's centre line, and xs is the first column whose
// centre lies at or to the right of it (fl_xs: the header's formula).  Scratch lives in the caller's workspace: the crossings in per-row
// buckets (8 bytes each, [N][ecap]), per frame and row the difference array of the rows' crossing counts that becomes the scatter's cursor
// (int32 [N][H + 1]) and the buckets' offsets (int32 [N][H + 1]), and for W > FL_LINE one owner line per workgroup of the row launch.
// 5 launches, sized on the host from the capacities; a phase boundary is a launch boundary: no workgroup waits for another, nothing spins.
//   clear    the refusal decision: counts_out = -1 for a refused frame; the difference arrays zeroed.
//   count    a lane owns a vertex (grid-stride over the frame's vertices, blockIdx.y strides over the frames) and with it the edge to the
//            next vertex of its loop, which a binary search over the loops' first vertices finds: no lane waits for a long loop.  +1 at
//            the edge's first row, -1 behind its last -- two atomics per edge, not one per row.
//   scan     one workgroup per frame: the prefix of the differences is a row's crossing count, the prefix of those the bucket offsets
//            (rc_block_scan, twice, with carries) -> counts_out = E; the differences are left zero, as cursors; the frame's stats zeroed
//            if it will be painted.
//   scatter  count's walk again: every edge writes its word into each row it crosses, at the row's cursor (an atomic with return); an
//            edge of more than FL_SHORT rows is handed to the lane's wave, whose lanes stride over its rows.  The order inside a bucket
//            depends on the arrival, the set of words does not, and equal words cannot be told apart.
//   rows     a workgroup owns a row (grid-stride over the rows).  The bucket is staged in LDS when it has at most FL_STAGE words, else
//            read in place.  256 crossings at a time, a thread per crossing: one pass over the bucket counts the crossings of its region
//            before it in (xs, index) order and finds the nearest one behind it; an even count opens the span [xs, that one's xs).  The
//            256 spans go through LDS to the waves, which paint them into the owner line by integer max of region + 1 (lanes stride
//            over a span).  Then a thread per pixel: the byte out, the reference in and the pixel's code {covered, reference, value} back
//            into the line; with stats a second walk tallies the codes, the counters in registers and in an LDS histogram (per wave and distinct
//            code one LDS atomic per counter, fl_tally).  Per workgroup and frame one global atomic per non-zero counter.
//            Not launched in a sizing pass.
//
// Bounds of the loops (nothing else loops):
//   grid-stride loops      over frames, vertices, rows, a row's columns, the histogram: counted.
//   the search for a loop  a binary search over the frame's L loop records: at most 31 rounds.
//   an edge's rows         ymin .. ymax, both clamped into [0, H]: at most FL_SHORT rounds of a lane, H / 64 + 1 of a wave; a wave takes
//                          over at most 64 edges per stride.
//   the pairing            a thread reads its bucket once per chunk: m reads for each of m crossings, m <= E <= ecap -- m * m / 256 rounds
//                          per thread and row at the worst, in LDS for m <= FL_STAGE and in L2 beyond.
//   the painting           a wave paints at most 64 of a chunk's 256 spans, a span is at most W columns: counted.
//   fl_tally               every round retires at least the leading lane: at most 64 rounds.
//   the scans              6 shuffle steps per rc_block_scan, two scans per pass, H / 256 + 1 passes.
// Clamps: a frame is processed only with 0 <= L <= lcap, 0 <= V <= vcap and 0 <= R <= rcap; the search stays inside [0, L); a loop's
// first is clamped into [0, V] and its count into [0, V - first], and a vertex outside its loop is skipped, so every vertex index stays
// below V <= vcap; a vertex's x is clamped into [0, W] and its y into [0, H], so a row index is below H, a column at most W and every
// product of fl_xs below 2^31; a loop's region is clamped into [0, R - 1] (a frame
// without regions has no edges); a bucket's bounds are clamped into [0, E] with E <= ecap, a cursor's slot is used only below the
// bucket's end; a span's ends lie in [0, W] since every xs does.  Malformed input gives meaningless output and touches nothing outside
// the caller's buffers.
#include "runcode.h"

namespace {

constexpr int FL_SHORT = 2;                             // the tallest edge a lane of scatter keeps to itself, in rows
constexpr int FL_STAGE = 1024;                          // the largest bucket a row stages in LDS: 8 KiB
constexpr int FL_LINE = 8192;                           // the widest owner line held in LDS: 32 KiB
constexpr int FL_NSTATS = 3 + 3 * 256;                  // ARSEG_FILL_NSTATS

struct FlP {
    const int *counts;                                  // [N][2]
    const int *loops;                                   // [N][lcap][4]
    const unsigned *verts;                              // [N][vcap]
    const int *n_regions;                               // [N]
    const long long *records;                           // [N][rcap][8]
    const unsigned char *ref;                           // the reference plane (may be null)
    unsigned char *out;                                 // labels_out (null in a sizing pass)
    int *counts_out;                                    // [N]
    unsigned long long *stats;                          // [N][FL_NSTATS] (may be null)
    rc_u64 *events;                                     // [N][ecap]
    int *cursor;                                        // [N][H + 1]: the differences, then the cursors
    int *offset;                                        // [N][H + 1]
    unsigned *lines;                                    // [workgroups of rows][W] (W > FL_LINE only)
    long long lcap, vcap, rcap, ecap, estride, ref_pitch, ref_ns, out_pitch, out_ns;
    int N, H, W, background;
};

// The loops, vertices and regions of a frame; false for a frame that is refused.
__device__ __forceinline__ bool fl_frame(const FlP &p, int n, int &L, int &V, int &R) {
    L = p.counts[2 * (size_t)n]; V = p.counts[2 * (size_t)n + 1]; R = p.n_regions[n];
    return L >= 0 && V >= 0 && L <= p.lcap && V <= p.vcap && R >= 0 && R <= p.rcap;
}

// The first column whose centre lies at or right of the edge (xa, ya) -> (xb, yb), ya < yb, on row y's centre line: the header's formula.
__device__ __forceinline__ int fl_xs(int xa, int ya, int xb, int yb, int y, int W) {
    const int dy = yb - ya, t = 2 * y + 1 - 2 * ya;
    const int num = 2 * xa * dy + t * (xb - xa) - dy, den = 2 * dy;
    const int q = num / den;                                                  // towards zero: the ceiling of a negative quotient already
    return rc_clamp(q + (num % den > 0 ? 1 : 0), 0, W);
}

// Edge i of a loop of cnt vertices at P, clamped into the frame and ordered so that ya < yb; false for a horizontal edge.
__device__ __forceinline__ bool fl_edge(const FlP &p, const unsigned *P, int i, int cnt, int &xa, int &ya, int &xb, int &yb) {
    const unsigned a = P[i], b = P[i + 1 < cnt ? i + 1 : 0];
    xa = min((int)(a & 0xffffu), p.W); ya = min((int)(a >> 16), p.H);
    xb = min((int)(b & 0xffffu), p.W); yb = min((int)(b >> 16), p.H);
    if (ya > yb) { const int tx = xa, ty = ya; xa = xb; ya = yb; xb = tx; yb = ty; }
    return ya < yb;
}

__global__ __launch_bounds__(256) void fill_clear_kernel(const FlP p) {
    for (int n = blockIdx.y; n < p.N; n += gridDim.y) {
        int L, V, R;
        if (!fl_frame(p, n, L, V, R)) {
            if (blockIdx.x == 0 && threadIdx.x == 0) p.counts_out[n] = -1;
            continue;
        }
        int *diff = p.cursor + (size_t)n * (p.H + 1);
        for (int i = blockIdx.x * blockDim.x + threadIdx.x; i <= p.H; i += gridDim.x * blockDim.x) diff[i] = 0;
    }
}

// One crossing of scatter: the edge's word into row y's bucket, at the row's cursor.
__device__ __forceinline__ void fl_emit(rc_u64 *events, int *cursor, const int *offset, int E, rc_u64 region, int xa, int ya, int xb, int yb,
                                        int y, int W) {
    const int b0 = rc_clamp(offset[y], 0, E), b1 = rc_clamp(offset[y + 1], b0, E);
    const int slot = b0 + atomicAdd(cursor + y, 1);
    if (slot >= b0 && slot < b1) events[slot] = (region << 16) | (rc_u64)fl_xs(xa, ya, xb, yb, y, W);
}

// count (SCATTER false) and scatter (true): a lane per vertex of the frame, which is the edge to the next vertex of its loop.  The loop is
// the last one whose first vertex is at or before the lane's: the loops' firsts are a prefix sum, so a binary search finds it.  In scatter
// a lane writes the crossings of an edge of at most FL_SHORT rows itself; a longer edge is handed to the wave, whose lanes stride over its
// rows -- else the frame's tallest edge, one lane's chain of atomics with return, sets the launch's time.
template <bool SCATTER>
__global__ __launch_bounds__(256) void fill_edges_kernel(const FlP p) {
    const int lane = threadIdx.x & 63;
    for (int n = blockIdx.y; n < p.N; n += gridDim.y) {
        int L, V, R;
        if (!fl_frame(p, n, L, V, R) || R == 0 || L == 0) continue;
        int *cursor = p.cursor + (size_t)n * (p.H + 1);
        const int *offset = p.offset + (size_t)n * (p.H + 1);
        rc_u64 *events = p.events + (size_t)n * p.estride;
        const int *loops = p.loops + (size_t)n * p.lcap * 4;
        int E = 0;
        if (SCATTER) {
            const int total = offset[p.H];                                    // E, or INT_MAX beyond it
            if (total > p.ecap) continue;                                     // overflowed: counts_out only
            E = max(total, 0);
        }
        for (int v0 = blockIdx.x * blockDim.x; v0 < V; v0 += gridDim.x * blockDim.x) {      // uniform: the hand-over needs every lane
            const int v = v0 + (int)threadIdx.x;
            int lo = 0, hi = v < V ? L : 0;                                   // the loop lies in [lo, hi): at most 31 rounds
            while (hi - lo > 1) {
                const int mid = (lo + hi) >> 1;
                if (loops[4 * (size_t)mid + 1] <= v) lo = mid; else hi = mid;
            }
            const int *rec = loops + 4 * (size_t)lo;
            const int first = rc_clamp(rec[1], 0, V), cnt = rc_clamp(rec[2], 0, V - first);
            const rc_u64 region = (rc_u64)rc_clamp(rec[0], 0, R - 1);
            int xa = 0, ya = 0, xb = 0, yb = 0;
            // (malformed records: no loop may hold this vertex)
            const bool edge = v >= first && v < first + cnt && fl_edge(p, p.verts + (size_t)n * p.vcap + first, v - first, cnt, xa, ya, xb, yb);
            if (!SCATTER) {
                if (edge) { atomicAdd(cursor + ya, 1); atomicAdd(cursor + yb, -1); }
                continue;                                                     // (uniform: SCATTER is a constant)
            }
            const bool tall = edge && yb - ya > FL_SHORT;
            if (edge && !tall)
                for (int y = ya; y < yb; ++y) fl_emit(events, cursor, offset, E, region, xa, ya, xb, yb, y, p.W);
            for (rc_u64 todo = __ballot(tall); todo; todo &= todo - 1) {      // at most 64 rounds
                const int lead = __builtin_ctzll(todo);
                const int txa = __shfl(xa, lead, 64), tya = __shfl(ya, lead, 64), txb = __shfl(xb, lead, 64), tyb = __shfl(yb, lead, 64);
                const rc_u64 tregion = (rc_u64)(unsigned)__shfl((int)(unsigned)region, lead, 64);
                for (int y = tya + lane; y < tyb; y += 64) fl_emit(events, cursor, offset, E, tregion, txa, tya, txb, tyb, y, p.W);
            }
        }
    }
}

// Per frame: the rows' crossing counts (the prefix of the differences) and the buckets' offsets (the prefix of the counts) -> offset, E.
__global__ __launch_bounds__(256) void fill_scan_kernel(const FlP p) {
    __shared__ int part_c[4];
    __shared__ long long part_o[4];
    for (int n = blockIdx.x; n < p.N; n += gridDim.x) {
        int L, V, R;
        if (!fl_frame(p, n, L, V, R)) continue;
        int *cursor = p.cursor + (size_t)n * (p.H + 1);
        int *offset = p.offset + (size_t)n * (p.H + 1);
        int carry_c = 0;
        long long carry_o = 0;
        for (int y0 = 0; y0 < p.H; y0 += 256) {                               // y0 is uniform: every thread makes every pass
            const int y = y0 + (int)threadIdx.x;
            int c = y < p.H ? cursor[y] : 0;
            rc_block_scan<1>(&c, &carry_c, part_c);                           // the crossings of row y (0 beyond H: the differences sum to 0)
            c = y < p.H ? max(c, 0) : 0;
            long long o = c;
            rc_block_scan<1>(&o, &carry_o, part_o);
            if (y < p.H) { offset[y] = (int)min(o - c, (long long)INT_MAX); cursor[y] = 0; }
        }
        const long long E = carry_o;
        if (threadIdx.x == 0) { offset[p.H] = (int)min(E, (long long)INT_MAX); p.counts_out[n] = (int)min(E, (long long)INT_MAX); }
        if (p.stats != nullptr && p.out != nullptr && E <= p.ecap)
            for (int i = threadIdx.x; i < FL_NSTATS; i += 256) p.stats[(size_t)n * FL_NSTATS + i] = 0ull;
    }
}

// Crossing i of the bucket ev[0 .. m): the crossings of its region before it in (xs, index) order counted, the nearest behind it found ->
// true with the span [x0, x1) and the region when it opens one.
__device__ __forceinline__ bool fl_pair(const rc_u64 *ev, int m, int i, int &x0, int &x1, unsigned &region) {
    const rc_u64 key = ev[i];
    unsigned before = 0;
    rc_u64 next = ~0ull;
    for (int j = 0; j < m; ++j) {
        const rc_u64 k = ev[j];
        if ((k >> 16) != (key >> 16)) continue;
        if (k < key || (k == key && j < i)) ++before;
        else if (j != i && k < next) next = k;
    }
    x0 = (int)(key & 0xffffu);
    x1 = next == ~0ull ? x0 : (int)(next & 0xffffu);                          // (an even number per region and row: an opener has a partner)
    region = (unsigned)(key >> 16);
    return (before & 1u) == 0;
}

// The pixels of a wave tallied by their code {covered << 16 | reference << 8 | value}: per distinct code of the wave its leading lane adds
// the number of lanes that hold it to the LDS histogram (one LDS atomic per counter it touches) and to its own gaps and changed.  Every
// lane of the wave calls.
__device__ __forceinline__ void fl_tally(unsigned *hist, unsigned code, bool active, bool with_ref, int lane, unsigned &gaps, unsigned &changed) {
    rc_u64 todo = __ballot(active);
    while (todo) {
        const int lead = __builtin_ctzll(todo);
        const unsigned lc = (unsigned)__shfl((int)code, lead, 64);
        const rc_u64 same = __ballot(active && code == lc);
        if (lane == lead) {
            const unsigned count = (unsigned)__builtin_popcountll(same), v = lc & 0xffu, r = (lc >> 8) & 0xffu;
            const bool cover = (lc >> 16) != 0u;
            if (cover) atomicAdd(hist + 256 + v, count); else gaps += count;
            if (with_ref) {
                atomicAdd(hist + r, count);
                if (cover && v == r) atomicAdd(hist + 512 + v, count); else changed += count;
            }
        }
        todo &= ~same;
    }
}

// The owner line: LDS, or for wide rows the workgroup's own line in global memory, which it reads and writes past its L1.
template <bool WIDE> __device__ __forceinline__ void fl_line_store(unsigned *line, int x, unsigned v) {
    if (WIDE) __hip_atomic_store(line + x, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); else line[x] = v;
}
template <bool WIDE> __device__ __forceinline__ unsigned fl_line_load(unsigned *line, int x) {
    return WIDE ? __hip_atomic_load(line + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : line[x];
}

template <bool WIDE>
__global__ __launch_bounds__(256) void fill_rows_kernel(const FlP p) {
    extern __shared__ unsigned lds_line[];                                    // W words (none when WIDE)
    __shared__ rc_u64 stage[FL_STAGE];
    __shared__ int span_x0[256], span_x1[256];
    __shared__ unsigned span_own[256];
    __shared__ unsigned hist[3 * 256];                                        // ref_area, fill_area, both of the rows of this workgroup
    __shared__ unsigned long long total[3];                                   // gaps, the spans' lengths, changed
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int W = p.W;
    unsigned *line = WIDE ? p.lines + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * (size_t)W : lds_line;
    for (int n = blockIdx.y; n < p.N; n += gridDim.y) {
        int L, V, R;
        if (!fl_frame(p, n, L, V, R)) continue;
        const int *offset = p.offset + (size_t)n * (p.H + 1);
        const int E = offset[p.H];
        if (E > p.ecap) continue;                                             // overflowed: counts_out only
        const rc_u64 *events = p.events + (size_t)n * p.estride;
        const long long *records = p.records + (size_t)n * p.rcap * 8;
        for (int i = tid; i < 3 * 256; i += 256) hist[i] = 0u;
        if (tid < 3) total[tid] = 0ull;
        unsigned gaps = 0, changed = 0, rows = 0;
        unsigned long long covered = 0;
        __syncthreads();
        for (int y = blockIdx.x; y < p.H; y += gridDim.x) {
            const int b0 = rc_clamp(offset[y], 0, E), m = rc_clamp(offset[y + 1], b0, E) - b0;
            const bool staged = m <= FL_STAGE;
            for (int x = tid; x < W; x += 256) fl_line_store<WIDE>(line, x, 0u);
            if (staged)
                for (int i = tid; i < m; i += 256) stage[i] = events[b0 + i];
            __syncthreads();
            for (int c0 = 0; c0 < m; c0 += 256) {                             // uniform: every thread makes every pass
                const int i = c0 + tid;
                int x0 = 0, x1 = 0;
                unsigned region = 0;
                if (i < m && !(staged ? fl_pair(stage, m, i, x0, x1, region) : fl_pair(events + b0, m, i, x0, x1, region))) x1 = x0;
                x0 = min(x0, W); x1 = rc_clamp(x1, x0, W);                    // (every xs is at most W already)
                span_x0[tid] = x0; span_x1[tid] = x1; span_own[tid] = region + 1u;
                covered += (unsigned long long)(x1 - x0);
                __syncthreads();
                const int slots = min(256, m - c0);
                for (int s = wave; s < slots; s += 4) {
                    const int s0 = span_x0[s], s1 = span_x1[s];
                    const unsigned own = span_own[s];
                    for (int x = s0 + lane; x < s1; x += 64) atomicMax(line + x, own);
                }
                __syncthreads();
            }
            unsigned char *out = p.out + (size_t)n * p.out_ns + (size_t)y * p.out_pitch;
            const unsigned char *ref = p.ref ? p.ref + (size_t)n * p.ref_ns + (size_t)y * p.ref_pitch : nullptr;
            // the bytes out, four pixels of a thread at a time so that their loads are in flight together; a pixel's code goes back into
            // the line, where the same thread finds it again
            for (int xb = tid; xb < W; xb += 1024) {
                unsigned own[4], v[4], r[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) own[u] = xb + 256 * u < W ? fl_line_load<WIDE>(line, xb + 256 * u) : 0u;
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    v[u] = own[u] != 0u ? (unsigned)(records[(size_t)min(own[u] - 1u, (unsigned)(R - 1)) * 8] & 0xff) : (unsigned)p.background;
                    r[u] = ref != nullptr && xb + 256 * u < W ? ref[xb + 256 * u] : 0u;
                }
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int x = xb + 256 * u;
                    if (x < W) {
                        out[x] = (unsigned char)v[u];
                        fl_line_store<WIDE>(line, x, (own[u] != 0u ? 0x10000u : 0u) | (r[u] << 8) | v[u]);
                    }
                }
            }
            if (p.stats != nullptr)
                for (int xb = 0; xb < W; xb += 256) {                         // uniform: fl_tally needs every lane
                    const int x = xb + tid;
                    fl_tally(hist, x < W ? fl_line_load<WIDE>(line, x) : 0u, x < W, ref != nullptr, lane, gaps, changed);
                }
            ++rows;
            __syncthreads();                                                  // the line is cleared again
        }
        if (p.stats == nullptr) continue;                                     // (uniform)
        atomicAdd(&total[0], (unsigned long long)gaps);
        atomicAdd(&total[1], covered);
        atomicAdd(&total[2], (unsigned long long)changed);
        __syncthreads();
        unsigned long long *stats = p.stats + (size_t)n * FL_NSTATS;
        if (tid == 0 && total[0]) atomicAdd(stats, total[0]);
        if (tid == 1) {                                                       // excess = sum of k - covered pixels, over this workgroup's rows
            const unsigned long long excess = total[1] - ((unsigned long long)rows * (unsigned)W - total[0]);
            if (excess) atomicAdd(stats + 1, excess);
        }
        if (tid == 2 && total[2]) atomicAdd(stats + 2, total[2]);
        for (int i = tid; i < 3 * 256; i += 256)
            if (hist[i]) atomicAdd(stats + 3 + i, (unsigned long long)hist[i]);
        __syncthreads();                                                      // before the next frame clears them
    }
}

dim3 fl_rows_grid(int N, int H, int W) { return rc_grid(N, H, 1, W > FL_LINE ? 256 : 1024); }

}  // namespace

// per frame 8 bytes per crossing slot and twice 4 bytes per row and one more; for W > FL_LINE 4 W bytes per workgroup of the row launch;
// rounded up to 16 bytes in all; a size that does not fit size_t comes back as its largest value, which no workspace has
extern "C" size_t arseg_contours_fill_workspace_bytes(int N, int H, int W, int64_t lcap, int64_t vcap, int64_t ecap) {
    if (N <= 0 || H <= 0 || W <= 0 || H > 16384 || W > 16384 || lcap < 0 || vcap < 0 || ecap < 0) return 0;
    const size_t none = ~(size_t)0;
    if (ecap > INT64_MAX / 8) return none;
    size_t frame = 8 * (size_t)ecap, bytes;
    if (__builtin_add_overflow(frame, 8 * ((size_t)H + 1), &frame) || __builtin_mul_overflow(frame, (size_t)N, &bytes)) return none;
    if (W > FL_LINE) {
        const dim3 g = fl_rows_grid(N, H, W);
        if (__builtin_add_overflow(bytes, (size_t)g.x * g.y * 4 * (size_t)W, &bytes)) return none;
    }
    if (bytes > none - 15) return none;
    return (bytes + 15) & ~(size_t)15;
}

extern "C" int arseg_contours_fill_fwd(const int32_t *counts, const int32_t *loops, int64_t lcap, const uint32_t *verts, int64_t vcap,
                                       const int32_t *n_regions, const int64_t *records, int64_t rcap, int N, int H, int W, int background,
                                       const uint8_t *ref_labels, int64_t ref_pitch, int64_t ref_image_stride, uint8_t *labels_out,
                                       int64_t pitch, int64_t image_stride, int32_t *counts_out, int64_t *stats, int64_t ecap,
                                       void *workspace, size_t workspace_bytes, arseg_stream_t stream) {
    ARSEG_CHECK_PTR(counts); ARSEG_CHECK_PTR(n_regions); ARSEG_CHECK_PTR(counts_out);
    ARSEG_CHECK_POS(N); ARSEG_CHECK_POS(H); ARSEG_CHECK_POS(W);
    if (lcap < 0 || vcap < 0 || rcap < 0 || ecap < 0 || (loops == nullptr && lcap > 0) || (verts == nullptr && vcap > 0) ||
        (records == nullptr && rcap > 0) || (labels_out == nullptr && ecap > 0))
        return ARSEG_EINVAL;
    if (H > 16384 || W > 16384 || background < 0 || background > 255) return ARSEG_EINVAL;
    if (rc_misaligned(4, counts, loops, verts, n_regions, counts_out) || rc_misaligned(8, records, stats, workspace)) return ARSEG_EINVAL;
    if (labels_out != nullptr && (pitch < (int64_t)W || image_stride < 0)) return ARSEG_EINVAL;
    if (ref_labels != nullptr && (ref_pitch < (int64_t)W || ref_image_stride < 0)) return ARSEG_EINVAL;
    const void *ins[] = {counts, loops, verts, n_regions, records, ref_labels};
    const void *outs[] = {labels_out, counts_out, stats};
    for (const void *o : outs)
        for (const void *i : ins)
            if (o != nullptr && o == i) return ARSEG_EINVAL;
    if ((const void *)labels_out == (const void *)counts_out || (stats != nullptr && ((const void *)stats == (const void *)labels_out ||
                                                                                      (const void *)stats == (const void *)counts_out)))
        return ARSEG_EINVAL;
    const size_t need = arseg_contours_fill_workspace_bytes(N, H, W, lcap, vcap, ecap);
    if (need == ~(size_t)0 || workspace_bytes < need) return ARSEG_EWORKSPACE;
    ARSEG_CHECK_PTR(workspace);
    FlP p = {};
    p.counts = counts; p.loops = loops; p.verts = verts; p.n_regions = n_regions; p.records = reinterpret_cast<const long long *>(records);
    p.ref = ref_labels; p.out = labels_out; p.counts_out = counts_out; p.stats = reinterpret_cast<unsigned long long *>(stats);
    p.lcap = lcap; p.vcap = vcap; p.rcap = rcap; p.estride = ecap;
    p.ecap = ecap < (int64_t)INT32_MAX ? ecap : (int64_t)INT32_MAX - 1;          // a count saturates at INT32_MAX: always an overflow
    p.ref_pitch = ref_pitch; p.ref_ns = ref_image_stride; p.out_pitch = pitch; p.out_ns = image_stride;
    p.N = N; p.H = H; p.W = W; p.background = background;
    p.events = static_cast<rc_u64 *>(workspace);
    p.cursor = reinterpret_cast<int *>(p.events + (size_t)N * (size_t)ecap);
    p.offset = p.cursor + (size_t)N * ((size_t)H + 1);
    p.lines = reinterpret_cast<unsigned *>(p.offset + (size_t)N * ((size_t)H + 1));
    hipStream_t st = arseg_stream(stream);
    const dim3 per_vertex = rc_grid(N, vcap, 256, 4096);
    hipLaunchKernelGGL(fill_clear_kernel, rc_grid(N, (long long)H + 1, 256, 4096), dim3(256), 0, st, p);
    hipLaunchKernelGGL((fill_edges_kernel<false>), per_vertex, dim3(256), 0, st, p);
    hipLaunchKernelGGL(fill_scan_kernel, rc_frames(N), dim3(256), 0, st, p);
    if (labels_out == nullptr) return arseg_launch_status();                  // the sizing pass
    hipLaunchKernelGGL((fill_edges_kernel<true>), per_vertex, dim3(256), 0, st, p);
    const dim3 per_row = fl_rows_grid(N, H, W);
    if (W > FL_LINE) hipLaunchKernelGGL((fill_rows_kernel<true>), per_row, dim3(256), 0, st, p);
    else hipLaunchKernelGGL((fill_rows_kernel<false>), per_row, dim3(256), 4 * (size_t)W, st, p);
    return arseg_launch_status();
}
