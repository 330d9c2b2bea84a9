// Small regions of a row-run code absorbed into their neighbours (include/arseg_hip.h, arseg_rle_absorb_fwd): a run code with its run_region
// and region records (as arseg_labels_rle_fwd + arseg_rle_regions_fwd leave them), min_area and a table of protected values in; the run code
// of the plane in which every small region has taken the value of the stable neighbour it shares the longest 4-neighbour border with out,
// with the target of every region and the number of absorbed regions per frame.  Nothing of the size of a frame is read or written: the
// input is a few thousand words per frame and stays in L2.
//
// Scratch lives in the caller's workspace, per frame: a pair table of pcap slots {key = small region << 32 | stable region, border}, open
// addressed with linear probing as the tables of links.hip (a key is never removed: an insert that has seen all pcap slots taken by other
// keys has proven more than pcap distinct pairs, so -2 does not depend on timing); one 64-bit word per region (AB_STABLE for a stable
// region, else the packed best (border << 32 | ~stable region), 0 = none); and one flag word.
// Six launches; a phase boundary is a launch boundary: no workgroup waits for another, no flags are waited on, nothing spins on memory.
//   clear    the refusal decision (n_absorbed = -1 or 0), the flag 0, the table empty, the regions' words = AB_STABLE or 0 from the records.
//   vote     a wave owns a row (grid-stride over the rows, blockIdx.y strides over the frames), its lanes take the row's runs 64 at a time.
//            A lane pairs its run with its right neighbour (border 1): lanes next to each other that hold one key -- a speck between two
//            runs of one region -- are merged before anything leaves the wave (heads by __shfl_up, their ballot gives the lengths).  Then
//            it finds the first run of the row above that reaches its own by binary search and walks right while the overlap lasts; the
//            overlap lengths of consecutive runs above with one key are summed in the lane before the insert (the walks of the lanes have
//            different lengths, so they are not merged across lanes).  Only (small, stable) pairs are inserted: a 64-bit atomicCAS into
//            an empty slot, then a 64-bit atomicAdd.  A failed insert sets the frame's flag.  Vector atomics on global memory only.
//   resolve  one thread per slot: atomicMax of (border << 32 | ~stable region) into the small region's word: the largest border, then the
//            smaller index.
//   count    the first launch that writes an output, and the first that knows whether the vote fitted.  A wave per row: the new value of
//            every run (its target's value, else its own), a run survives if it is the first of its row or its new value differs from its
//            predecessor's; the survivors of the row into out_row_start[n][y + 1].
//   scan     one workgroup per frame: the prefix over out_row_start (rc_block_scan); target and n_absorbed (or -2) from the regions' words.
//   emit     the walk of count; a survivor's index is the row's base plus the survivors before it in the wave; words below out_cap only.
// Integers throughout: every output is a pure function of the inputs.
//
// Bounds of the loops (nothing else loops):
//   grid-stride loops      over frames, rows, runs of a row, slots and regions: counted.
//   rc_cover               a binary search over (first, last] of the row above: at most 31 rounds.
//   the walk               advances one run of the row above per round and ends at that row's last run at the latest.
//   rc_pair_insert         advances one slot per round and ends after pcap rounds at the latest.
//   the shuffles           6 rounds.
// Indices are clamped by runcode.h: a row's runs into [0, stored runs) of its frame, columns into [0, W]; a region number is
// used as an index only below the frame's region count, which is at most rcap in a frame that is not refused.  A malformed run code or
// run_region gives a meaningless code and nothing outside the caller's buffers.
#include "runcode.h"

namespace {

constexpr int AB_WAVES = 4;                             // waves (= rows in flight) per workgroup
constexpr rc_u64 AB_STABLE = ~0ull;                     // a stable region's word; a packed best holds a border < 2^32 - 1 (at most 2 H W - 2)

struct AbP {
    const int *rs;                                      // [N][H + 1]
    const unsigned *runs;                               // [N][cap]
    const int *nreg;                                    // [N]
    const int *rr;                                      // run_region [N][cap]
    const long long *reg;                               // regions [N][rcap][8]
    int *out_rs;                                        // [N][H + 1]
    unsigned *out_runs;                                 // [N][out_cap]
    int *target;                                        // [N][tcap] (may be null: tcap == 0)
    int *nabs;                                          // [N]
    rc_u64 *pairs;                                      // [N][pcap][2]: key, border
    rc_u64 *best;                                       // [N][rcap]
    unsigned *flag;                                     // [N][2]: the first word is used
    rc_u64 protect[4];                                  // bit v: value v is protected
    long long cap_stride, out_stride, rcap, tcap, pcap, min_area;
    int cap, out_cap;                                   // min(., INT32_MAX): an index is below 2^31
    int N, H, W;
};

// The stored runs of a frame, or -1 for a frame that is refused: its run code overflowed, or its regions are missing or more than the records.
__device__ __forceinline__ int ab_total(const AbP &p, int n) {
    const int stored = rc_stored(p.rs[(size_t)n * (p.H + 1) + p.H], p.cap), R = p.nreg[n];
    return (R < 0 || (long long)R > p.rcap) ? -1 : stored;
}

__device__ __forceinline__ bool ab_protected(const AbP &p, unsigned v) {
    const rc_u64 w = v < 64 ? p.protect[0] : v < 128 ? p.protect[1] : v < 192 ? p.protect[2] : p.protect[3];
    return (w >> (v & 63u)) & 1ull;
}

__device__ __forceinline__ void ab_add(const AbP &p, int n, rc_u64 *pairs, rc_u64 key, rc_u64 border) {
    const long long s = rc_pair_insert(pairs, p.pcap, key);
    if (s >= 0) atomicAdd(pairs + 2 * s + 1, border);
    else atomicOr(p.flag + 2 * (size_t)n, 1u);
}

// The key of two neighbouring regions a != b with the words wa and wb: (small, stable) in that order, RC_EMPTY for every other combination.
__device__ __forceinline__ rc_u64 ab_key(int a, rc_u64 wa, int b, rc_u64 wb) {
    if (a == b || (wa == AB_STABLE) == (wb == AB_STABLE)) return RC_EMPTY;
    return wa == AB_STABLE ? ((rc_u64)(unsigned)b << 32) | (unsigned)a : ((rc_u64)(unsigned)a << 32) | (unsigned)b;
}

// The value run i takes: its target's where its region has one, its own otherwise.  R: the frame's regions (<= rcap).
__device__ __forceinline__ unsigned ab_value(const unsigned *runs, const int *rr, const rc_u64 *best, const long long *reg, int R, int i) {
    const int r = rr[i];
    if ((unsigned)r < (unsigned)R) {
        const rc_u64 w = best[r];
        if (w != 0 && w != AB_STABLE) {
            const unsigned s = 0xffffffffu - (unsigned)(w & 0xffffffffull);
            if (s < (unsigned)R) return (unsigned)reg[(size_t)s * 8] & 0xffu;
        }
    }
    return runs[i] & 0xffu;
}

__global__ __launch_bounds__(256) void absorb_clear_kernel(const AbP p) {
    for (int n = blockIdx.y; n < p.N; n += gridDim.y) {
        const bool ok = ab_total(p, n) >= 0;
        if (blockIdx.x == 0 && threadIdx.x == 0) { p.nabs[n] = ok ? 0 : -1; p.flag[2 * (size_t)n] = 0; p.flag[2 * (size_t)n + 1] = 0; }
        if (!ok) continue;
        const long long R = p.nreg[n];
        rc_u64 *pairs = p.pairs + (size_t)n * p.pcap * 2, *best = p.best + (size_t)n * p.rcap;
        const long long *reg = p.reg + (size_t)n * p.rcap * 8;
        for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < max(p.pcap, R); i += (long long)gridDim.x * blockDim.x) {
            if (i < p.pcap) { pairs[2 * i] = RC_EMPTY; pairs[2 * i + 1] = 0; }
            if (i < R) best[i] = (reg[i * 8 + 1] >= p.min_area || ab_protected(p, (unsigned)reg[i * 8] & 0xffu)) ? AB_STABLE : 0ull;
        }
    }
}

__global__ __launch_bounds__(64 * AB_WAVES) void absorb_vote_kernel(const AbP p) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int n = blockIdx.y; n < p.N; n += gridDim.y) {
        const int total = ab_total(p, n);
        if (total <= 0) continue;
        const int R = p.nreg[n];
        const int *rs = p.rs + (size_t)n * (p.H + 1);
        const unsigned *runs = p.runs + (size_t)n * p.cap_stride;
        const int *rr = p.rr + (size_t)n * p.cap_stride;
        const rc_u64 *best = p.best + (size_t)n * p.rcap;
        rc_u64 *pairs = p.pairs + (size_t)n * p.pcap * 2;
        for (int y = blockIdx.x * AB_WAVES + wave; y < p.H; y += gridDim.x * AB_WAVES) {
            // a malformed row_start may not lead outside [0, total): both rows are clamped into it
            int first, last;
            rc_row(rs, y, total, first, last);
            const int pf = y > 0 ? rc_clamp(rs[y - 1], 0, first) : first, pl = first;          // the row above: [pf, pl), empty for y == 0
            for (int i0 = first; i0 < last; i0 += 64) {                     // i0 is wave uniform: every lane makes every pass
                const int i = i0 + lane;
                const bool live = i < last;
                int r = -1, a0 = 0, a1 = 0;
                rc_u64 wr = 0, key = RC_EMPTY;
                if (live) {
                    a0 = rc_x0(runs, i, p.W); a1 = rc_x1(runs, i, last, p.W);
                    r = rr[i];
                    if ((unsigned)r >= (unsigned)R) r = -1;
                    else wr = best[r];
                    if (r >= 0 && i + 1 < last) {                           // the right neighbour: one pair of pixels
                        const int q = rr[i + 1];
                        if ((unsigned)q < (unsigned)R) key = ab_key(r, wr, q, best[q]);
                    }
                }
                int len;
                const bool head = rc_segment(key, lane, len);
                if (head && key != RC_EMPTY) ab_add(p, n, pairs, key, (rc_u64)len);
                if (r < 0 || pl <= pf || a1 <= a0) continue;                // no shuffle follows in this pass
                rc_u64 open = RC_EMPTY, sum = 0;                            // the key of the last runs above and their overlap so far
                // from the first run j of the row above with b1 > a0 on: b1 is the start of run j + 1, or W behind the row's last run
                for (int j = rc_cover(runs, pf, pl, a0); j < pl; ++j) {
                    const int b0 = rc_x0(runs, j, p.W);
                    if (b0 >= a1) break;                                    // the row is sorted: no later run overlaps
                    const int b1 = rc_x1(runs, j, pl, p.W);
                    const int overlap = min(a1, b1) - max(a0, b0);
                    const int q = rr[j];
                    if (overlap <= 0 || (unsigned)q >= (unsigned)R) continue;
                    const rc_u64 k = ab_key(r, wr, q, best[q]);
                    if (k != open) {
                        if (open != RC_EMPTY) ab_add(p, n, pairs, open, sum);
                        open = k; sum = 0;
                    }
                    sum += (rc_u64)overlap;
                }
                if (open != RC_EMPTY) ab_add(p, n, pairs, open, sum);
            }
        }
    }
}

__global__ __launch_bounds__(256) void absorb_resolve_kernel(const AbP p) {
    for (int n = blockIdx.y; n < p.N; n += gridDim.y) {
        if (ab_total(p, n) < 0 || p.flag[2 * (size_t)n] != 0) continue;
        const long long R = p.nreg[n];
        const rc_u64 *pairs = p.pairs + (size_t)n * p.pcap * 2;
        rc_u64 *best = p.best + (size_t)n * p.rcap;
        for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < p.pcap; i += (long long)gridDim.x * blockDim.x) {
            const rc_u64 key = pairs[2 * i];
            if (key == RC_EMPTY) continue;
            const long long r = (long long)(key >> 32);
            if (r < R) atomicMax(best + r, (pairs[2 * i + 1] << 32) | (0xffffffffull - (key & 0xffffffffull)));          // the longest border, then the smaller index
        }
    }
}

// EMIT = false: the survivors of every row into out_row_start[n][y + 1].  EMIT = true: their words, from out_row_start[n][y] on.
template <bool EMIT>
__global__ __launch_bounds__(64 * AB_WAVES) void absorb_rows_kernel(const AbP p) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int n = blockIdx.y; n < p.N; n += gridDim.y) {
        const int total = ab_total(p, n);
        if (total < 0 || p.flag[2 * (size_t)n] != 0) continue;              // refused or overflowed: nothing of the frame is touched
        const int R = p.nreg[n];
        const int *rs = p.rs + (size_t)n * (p.H + 1);
        const unsigned *runs = p.runs + (size_t)n * p.cap_stride;
        const int *rr = p.rr + (size_t)n * p.cap_stride;
        const rc_u64 *best = p.best + (size_t)n * p.rcap;
        const long long *reg = p.reg + (size_t)n * p.rcap * 8;
        int *out_rs = p.out_rs + (size_t)n * (p.H + 1);
        unsigned *out_runs = p.out_runs + (size_t)n * p.out_stride;
        for (int y = blockIdx.x * AB_WAVES + wave; y < p.H; y += gridDim.x * AB_WAVES) {
            int first, last;
            rc_row(rs, y, total, first, last);
            int base = EMIT ? out_rs[y] : 0;
            for (int i0 = first; i0 < last; i0 += 64) {                     // i0 is wave uniform: every lane makes every pass
                const int i = i0 + lane;
                const bool live = i < last;
                const unsigned v = live ? ab_value(runs, rr, best, reg, R, i) : 0x100u;
                unsigned left = __shfl_up(v, 1, 64);
                if (lane == 0) left = i0 > first ? ab_value(runs, rr, best, reg, R, i0 - 1) : 0x100u;          // 0x100: no value, the row's first run survives
                const bool survives = live && v != left;
                const rc_u64 found = __ballot(survives);
                if constexpr (EMIT) {
                    const int idx = base + __popcll(found & ((1ull << lane) - 1ull));
                    if (survives && idx >= 0 && idx < p.out_cap) out_runs[idx] = (runs[i] & ~0xffu) | v;
                }
                base += __popcll(found);
            }
            if constexpr (!EMIT) {
                if (lane == 0) out_rs[y + 1] = base;
            }
        }
    }
}

// out_row_start[n][1 .. H]: counts -> their inclusive prefix, in place (rc_block_scan); target and n_absorbed from the regions' words
__global__ __launch_bounds__(256) void absorb_scan_kernel(const AbP p) {
    __shared__ int part[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;          // (for the count of the absorbed regions)
    for (int n = blockIdx.x; n < p.N; n += gridDim.x) {
        if (ab_total(p, n) < 0) continue;
        if (p.flag[2 * (size_t)n] != 0) {
            if (threadIdx.x == 0) p.nabs[n] = -2;
            continue;
        }
        int *rs = p.out_rs + (size_t)n * (p.H + 1);
        int carry = 0;
        for (int i0 = 1; i0 <= p.H; i0 += 256) {
            const int i = i0 + (int)threadIdx.x;
            int inc = i <= p.H ? rs[i] : 0;
            rc_block_scan<1>(&inc, &carry, part);
            if (i <= p.H) rs[i] = inc;
        }
        if (threadIdx.x == 0) rs[0] = 0;
        const int R = p.nreg[n];
        const rc_u64 *best = p.best + (size_t)n * p.rcap;
        int *target = p.target ? p.target + (size_t)n * p.tcap : nullptr;
        int absorbed = 0;
        for (int r0 = 0; r0 < R; r0 += 256) {                              // r0 is uniform: every thread makes every pass
            const int r = r0 + (int)threadIdx.x;
            int t = -1;
            if (r < R) {
                const rc_u64 w = best[r];
                if (w != AB_STABLE) t = w == 0 ? -2 : (int)(0xffffffffu - (unsigned)(w & 0xffffffffull));
                if (r < p.tcap) target[r] = t;
            }
            absorbed += __popcll(__ballot(t >= 0));
        }
        if (lane == 0) part[wave] = absorbed;
        __syncthreads();
        if (threadIdx.x == 0) p.nabs[n] = part[0] + part[1] + part[2] + part[3];
        __syncthreads();
    }
}

}  // namespace

// per frame: the pair table of pcap slots of two 64-bit words, one 64-bit word per region record, and the flag.  The rows' survivor counts
// live in out_row_start until the scan, so cap and H add nothing; they are taken so that the layout can follow them without a new signature.
extern "C" size_t arseg_rle_absorb_workspace_bytes(int N, int64_t cap, int64_t rcap, int H, int64_t pcap) {
    if (N <= 0 || cap <= 0 || rcap < 0 || H <= 0 || pcap <= 0) return 0;
    return (size_t)N * ((size_t)pcap * 16 + (size_t)rcap * 8 + 8);
}

extern "C" int arseg_rle_absorb_fwd(const int32_t *row_start, const uint32_t *runs, const int32_t *n_regions, const int32_t *run_region,
                                    int64_t cap, const int64_t *regions, int64_t rcap, int N, int H, int W, int64_t min_area,
                                    const uint8_t *protect, int32_t *out_row_start, uint32_t *out_runs, int64_t out_cap, int32_t *target,
                                    int64_t tcap, int32_t *n_absorbed, int64_t pcap, void *workspace, size_t workspace_bytes,
                                    arseg_stream_t stream) {
    ARSEG_CHECK_PTR(row_start); ARSEG_CHECK_PTR(runs); ARSEG_CHECK_PTR(n_regions); ARSEG_CHECK_PTR(run_region); ARSEG_CHECK_PTR(regions);
    ARSEG_CHECK_PTR(out_row_start); ARSEG_CHECK_PTR(out_runs); ARSEG_CHECK_PTR(n_absorbed);
    ARSEG_CHECK_POS(N); ARSEG_CHECK_POS(H); ARSEG_CHECK_POS(W);
    if (cap <= 0 || pcap <= 0 || out_cap <= 0 || min_area < 1 || rcap < 0 || tcap < 0 || (target == nullptr && tcap > 0)) return ARSEG_EINVAL;
    if (W > (1 << 24) || (int64_t)H * W > (int64_t)INT32_MAX) return ARSEG_EINVAL;
    if (rc_misaligned(4, row_start, runs, n_regions, run_region, out_row_start, out_runs, target, n_absorbed) ||
        rc_misaligned(8, regions, workspace))
        return ARSEG_EINVAL;
    if (workspace_bytes < arseg_rle_absorb_workspace_bytes(N, cap, rcap, H, pcap)) return ARSEG_EWORKSPACE;
    ARSEG_CHECK_PTR(workspace);
    AbP p = {};
    p.rs = row_start; p.runs = runs; p.nreg = n_regions; p.rr = run_region; p.reg = reinterpret_cast<const long long *>(regions);
    p.out_rs = out_row_start; p.out_runs = out_runs; p.target = target; p.nabs = n_absorbed;
    p.pairs = static_cast<rc_u64 *>(workspace);
    p.best = p.pairs + (size_t)N * (size_t)pcap * 2;
    p.flag = reinterpret_cast<unsigned *>(p.best + (size_t)N * (size_t)rcap);
    if (protect)
        for (int v = 0; v < 256; ++v)
            if (protect[v]) p.protect[v >> 6] |= 1ull << (v & 63);
    p.cap_stride = cap; p.out_stride = out_cap; p.rcap = rcap; p.tcap = target ? tcap : 0; p.pcap = pcap; p.min_area = min_area;
    p.cap = rc_cap(cap); p.out_cap = rc_cap(out_cap);
    p.N = N; p.H = H; p.W = W;
    hipStream_t st = arseg_stream(stream);
    // a frame that is not refused has at most min(rcap, H * W) regions
    const long long regions_most = rcap < (long long)H * W ? rcap : (long long)H * W;
    const dim3 per_item = rc_grid(N, pcap > regions_most ? pcap : regions_most, 256, 16384), per_slot = rc_grid(N, pcap, 256, 16384);
    const dim3 per_row = rc_grid(N, H, AB_WAVES, 16384);
    hipLaunchKernelGGL(absorb_clear_kernel, per_item, dim3(256), 0, st, p);
    hipLaunchKernelGGL(absorb_vote_kernel, per_row, dim3(64 * AB_WAVES), 0, st, p);
    hipLaunchKernelGGL(absorb_resolve_kernel, per_slot, dim3(256), 0, st, p);
    hipLaunchKernelGGL((absorb_rows_kernel<false>), per_row, dim3(64 * AB_WAVES), 0, st, p);
    hipLaunchKernelGGL(absorb_scan_kernel, rc_frames(N), dim3(256), 0, st, p);
    hipLaunchKernelGGL((absorb_rows_kernel<true>), per_row, dim3(64 * AB_WAVES), 0, st, p);
    return arseg_launch_status();
}
