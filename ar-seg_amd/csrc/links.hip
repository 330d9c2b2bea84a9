// Links from the regions of a frame to the regions of a reference frame along the motion chain (include/arseg_hip.h,
// arseg_region_links_fwd): two run codes with their run_region (as arseg_labels_rle_fwd + arseg_rle_regions_fwd leave them) and the dense
// quarter-pel field mv_q in; per frame the number of distinct (region, reference region) pairs, one record of 6 int64 per region and one of
// 4 int64 per reference region out.  The object-level form of consistency.hip: the same target rule, counted per pair of regions instead of
// per class.  mv_q is the only input of the size of a frame; the run codes are a few tens of KB and stay in L2.
//
// The pairs live in the caller's workspace, per frame: a pair table of pcap slots {key = r << 32 | k, count}, a table of pcap slots
// {key = k, packed best} for the reference regions (mutual must be exact without `back`), and one flag word.  Both tables are open
// addressed with linear probing; a key is never removed, so an insert that has seen all pcap slots taken by other keys has proven more than
// pcap distinct keys: -2 does not depend on timing.  The reference regions that occur are at most as many as the pairs, so the second table
// cannot fill up in a frame that was not flagged.
// Six launches; a phase boundary is a launch boundary: no workgroup waits for another, no flags are waited on, nothing spins on memory.
//   clear    both tables empty, the flag 0, n_pairs = 0 (or -1: the frame cannot be linked).
//   vote     a wave owns a row of the current frame (grid-stride over the rows, blockIdx.y strides over the frames) and walks it 64 pixels
//            at a time: a lane reads its mv_q dword (coalesced), finds its own run and the reference run under its target by binary search
//            and forms its key.  Neighbouring lanes with one key are merged before anything leaves the wave: heads by __shfl_up, their
//            ballot gives the lengths; a head inserts its key (64-bit atomicCAS into an empty slot) and adds its length.  A failed insert
//            sets the frame's flag.  Vector atomics on global memory only.
//   rows     the first launch that knows whether a frame overflowed, and the first that writes into links / back: the rows below the stored
//            region counts = {-1, 0, ...} for the frames that stand, n_pairs = -2 for the flagged ones, whose rows nobody touches.
//   outside  the row walk again for the pixels whose target leaves the frame (skipped without mv_q: none can): waves without one go on after
//            a ballot, the others merge per region as vote does and add into links[r][3].  -2 must leave a frame's rows untouched, and a
//            workspace sized by pcap alone has no room for a count per region, so this cannot be part of vote; the field's second read finds
//            it in the Infinity Cache.
//   resolve  one thread per slot of the pair table: atomicMax of (count << 32 | ~k) into links[r][1], atomicAdd into same / n_ref and into
//            covered / n_cur, the mirror image (count << 32 | ~r) into k's slot of the second table; the wave's occupied slots are counted
//            into n_pairs with one atomic.
//   finish   one thread per region unpacks its best and looks its reference region's best up (mutual); one per reference region alike.
// Integers throughout: every output is a pure function of the inputs.
//
// Bounds of the loops (nothing else loops):
//   grid-stride loops      over frames, rows, pixels of a row, slots and records: counted.
//   rc_cover               a binary search over [first, last) with first < last <= stored runs: at most 31 rounds.
//   rc_pair_insert / rc_pair_lookup  advance one slot per round and end after pcap rounds at the latest.
//   the shuffles           6 rounds.
// Indices are clamped by runcode.h: a row's runs into [0, stored runs) of its frame, a region number is used as an index only
// below the stored region count and the capacity, a target row only inside [0, H).  A malformed run code or run_region gives meaningless
// links and nothing outside the caller's buffers.
#include "runcode.h"

namespace {

constexpr int LK_WAVES = 4;                             // waves (= rows in flight) per workgroup

struct LkSide {
    const int *rs;                                      // [.][H + 1]
    const unsigned *runs;                               // [.][cap]
    const int *nreg;                                    // [.]
    const int *rr;                                      // run_region [.][cap]
    long long cap_stride;
    int cap;                                            // min(cap, INT32_MAX)
};

struct LkP {
    LkSide cur, ref;
    const unsigned *mv;                                 // [N][H][W] of (mvx | mvy << 16), or null: zero motion
    int *npairs;                                        // [N]
    long long *links;                                   // [N][rcap][6] (may be null: rcap == 0)
    long long *back;                                    // [N][kcap][4] (may be null: kcap == 0)
    rc_u64 *pairs;                                      // [N][pcap][2]: key, count
    rc_u64 *bests;                                      // [N][pcap][2]: k, count << 32 | ~r
    unsigned *flag;                                     // [N][2]: the first word is used
    long long rcap, kcap, pcap;
    int N, H, W, shared;
};

// The stored runs of a side's frame, or -1 where the frame has no regions: its run code overflowed or n_regions says so.
__device__ __forceinline__ int lk_total(const LkSide &s, int f, int H) {
    const int stored = rc_stored(s.rs[(size_t)f * (H + 1) + H], s.cap);
    return (stored < 0 || s.nreg[f] < 0) ? -1 : stored;          // (n_regions is not read for an overflowed frame)
}
__device__ __forceinline__ long long lk_rows(const LkSide &s, int f, long long capacity) { return min((long long)s.nreg[f], capacity); }

__global__ __launch_bounds__(256) void links_clear_kernel(const LkP p) {
    for (int n = blockIdx.y; n < p.N; n += gridDim.y) {
        const bool ok = lk_total(p.cur, n, p.H) >= 0 && lk_total(p.ref, p.shared ? 0 : n, p.H) >= 0;
        if (blockIdx.x == 0 && threadIdx.x == 0) { p.npairs[n] = ok ? 0 : -1; p.flag[2 * (size_t)n] = 0; p.flag[2 * (size_t)n + 1] = 0; }
        if (!ok) continue;
        rc_u64 *pairs = p.pairs + (size_t)n * p.pcap * 2, *bests = p.bests + (size_t)n * p.pcap * 2;
        for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < p.pcap; i += (long long)gridDim.x * blockDim.x) {
            pairs[2 * i] = RC_EMPTY; pairs[2 * i + 1] = 0;
            bests[2 * i] = RC_EMPTY; bests[2 * i + 1] = 0;
        }
    }
}

// OUTSIDE = false: the pairs into the table.  OUTSIDE = true: the pixels whose target leaves the frame into links[r][3].
template <bool OUTSIDE>
__global__ __launch_bounds__(64 * LK_WAVES) void links_vote_kernel(const LkP p) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int n = blockIdx.y; n < p.N; n += gridDim.y) {
        const int m = p.shared ? 0 : n;
        const int total = lk_total(p.cur, n, p.H), qtotal = lk_total(p.ref, m, p.H);
        if (total <= 0 || qtotal < 0) continue;
        long long rlim = 0;
        if constexpr (OUTSIDE) {
            rlim = lk_rows(p.cur, n, p.rcap);
            if (p.flag[2 * (size_t)n] != 0 || rlim <= 0) continue;          // flagged: its rows stay untouched; no rows: nothing to add into
        }
        const int *rs = p.cur.rs + (size_t)n * (p.H + 1), *qrs = p.ref.rs + (size_t)m * (p.H + 1);
        const unsigned *runs = p.cur.runs + (size_t)n * p.cur.cap_stride, *qruns = p.ref.runs + (size_t)m * p.ref.cap_stride;
        const int *rr = p.cur.rr + (size_t)n * p.cur.cap_stride, *qrr = p.ref.rr + (size_t)m * p.ref.cap_stride;
        rc_u64 *pairs = p.pairs + (size_t)n * p.pcap * 2;
        for (int y = blockIdx.x * LK_WAVES + wave; y < p.H; y += gridDim.x * LK_WAVES) {
            // a malformed row_start may not lead outside [0, total)
            int first, last;
            rc_row(rs, y, total, first, last);
            if (last <= first) continue;                                    // wave uniform
            const unsigned *mv = p.mv ? p.mv + ((size_t)n * p.H + y) * p.W : nullptr;
            for (int x0 = 0; x0 < p.W; x0 += 64) {                          // x0 is wave uniform: every lane makes every pass
                const int x = x0 + lane;
                const bool live = x < p.W;
                const unsigned mq = (live && mv) ? mv[x] : 0u;
                const int tx = x + round_half_even_div4((int)(short)(mq & 0xffffu)), ty = y + round_half_even_div4((int)(short)(mq >> 16));
                const bool inside = (unsigned)tx < (unsigned)p.W && (unsigned)ty < (unsigned)p.H;          // no clamp: a target off the frame is never read
                rc_u64 key = RC_EMPTY;
                if constexpr (OUTSIDE) {
                    if (__ballot(live && !inside) == 0ull) continue;
                    if (live && !inside) {
                        const int r = rr[rc_cover(runs, first, last, x)];
                        if (r >= 0 && r < rlim) key = (rc_u64)(unsigned)r;
                    }
                } else if (live && inside) {
                    const int i = rc_cover(runs, first, last, x);
                    const int r = rr[i];
                    int qf, ql;
                    rc_row(qrs, ty, qtotal, qf, ql);
                    if (r >= 0 && ql > qf) {
                        const int j = rc_cover(qruns, qf, ql, tx);
                        const int k = qrr[j];
                        if (k >= 0 && ((qruns[j] ^ runs[i]) & 0xffu) == 0) key = ((rc_u64)(unsigned)r << 32) | (unsigned)k;
                    }
                }
                int len;
                const bool head = rc_segment(key, lane, len);
                if (!head || key == RC_EMPTY) continue;                     // no shuffle follows in this pass
                if constexpr (OUTSIDE) {
                    atomicAdd(reinterpret_cast<rc_u64 *>(p.links + ((size_t)n * p.rcap + key) * 6 + 3), (rc_u64)len);
                } else {
                    const long long s = rc_pair_insert(pairs, p.pcap, key);
                    if (s >= 0) atomicAdd(pairs + 2 * s + 1, (rc_u64)len);
                    else atomicOr(p.flag + 2 * (size_t)n, 1u);
                }
            }
        }
    }
}

__global__ __launch_bounds__(256) void links_rows_kernel(const LkP p) {
    for (int n = blockIdx.y; n < p.N; n += gridDim.y) {
        const int m = p.shared ? 0 : n;
        if (lk_total(p.cur, n, p.H) < 0 || lk_total(p.ref, m, p.H) < 0) continue;
        if (p.flag[2 * (size_t)n] != 0) {
            if (blockIdx.x == 0 && threadIdx.x == 0) p.npairs[n] = -2;
            continue;
        }
        const long long rlim = lk_rows(p.cur, n, p.rcap), klim = lk_rows(p.ref, m, p.kcap);
        for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < max(rlim, klim); i += (long long)gridDim.x * blockDim.x) {
            if (i < rlim) {
                long long *row = p.links + ((size_t)n * p.rcap + i) * 6;
                row[0] = -1; row[1] = 0; row[2] = 0; row[3] = 0; row[4] = 0; row[5] = 0;
            }
            if (i < klim) {
                long long *row = p.back + ((size_t)n * p.kcap + i) * 4;
                row[0] = -1; row[1] = 0; row[2] = 0; row[3] = 0;
            }
        }
    }
}

__global__ __launch_bounds__(256) void links_resolve_kernel(const LkP p) {
    for (int n = blockIdx.y; n < p.N; n += gridDim.y) {
        const int m = p.shared ? 0 : n;
        if (lk_total(p.cur, n, p.H) < 0 || lk_total(p.ref, m, p.H) < 0 || p.flag[2 * (size_t)n] != 0) continue;
        const long long rlim = lk_rows(p.cur, n, p.rcap), klim = lk_rows(p.ref, m, p.kcap);
        const rc_u64 *pairs = p.pairs + (size_t)n * p.pcap * 2;
        rc_u64 *bests = p.bests + (size_t)n * p.pcap * 2;
        // the bound is rounded up to whole waves: every lane of a wave reaches the ballot
        const long long padded = (p.pcap + 63) / 64 * 64;
        for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < padded; i += (long long)gridDim.x * blockDim.x) {
            const rc_u64 key = i < p.pcap ? pairs[2 * i] : RC_EMPTY;
            const bool taken = key != RC_EMPTY;
            if (taken) {
                const rc_u64 count = pairs[2 * i + 1];
                const long long r = (long long)(key >> 32), k = (long long)(key & 0xffffffffu);
                if (r < rlim) {
                    rc_u64 *row = reinterpret_cast<rc_u64 *>(p.links + ((size_t)n * p.rcap + r) * 6);
                    atomicMax(row + 1, (count << 32) | (0xffffffffull - (rc_u64)k));           // the largest count, then the smaller k
                    atomicAdd(row + 2, count);
                    atomicAdd(row + 5, 1ull);
                }
                const long long s = rc_pair_insert(bests, p.pcap, (rc_u64)k);           // cannot fail: no more reference regions than pairs
                if (s >= 0) atomicMax(bests + 2 * s + 1, (count << 32) | (0xffffffffull - (rc_u64)r));
                if (k < klim) {
                    rc_u64 *row = reinterpret_cast<rc_u64 *>(p.back + ((size_t)n * p.kcap + k) * 4);
                    atomicAdd(row + 2, count);
                    atomicAdd(row + 3, 1ull);
                }
            }
            const rc_u64 found = __ballot(taken);
            if (found && (threadIdx.x & 63) == 0) atomicAdd(p.npairs + n, __popcll(found));
        }
    }
}

__global__ __launch_bounds__(256) void links_finish_kernel(const LkP p) {
    for (int n = blockIdx.y; n < p.N; n += gridDim.y) {
        const int m = p.shared ? 0 : n;
        if (lk_total(p.cur, n, p.H) < 0 || lk_total(p.ref, m, p.H) < 0 || p.flag[2 * (size_t)n] != 0) continue;
        const long long rlim = lk_rows(p.cur, n, p.rcap), klim = lk_rows(p.ref, m, p.kcap);
        const rc_u64 *bests = p.bests + (size_t)n * p.pcap * 2;
        for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < max(rlim, klim); i += (long long)gridDim.x * blockDim.x) {
            if (i < rlim) {
                long long *row = p.links + ((size_t)n * p.rcap + i) * 6;
                const rc_u64 best = (rc_u64)row[1];
                if (best) {
                    const rc_u64 k = 0xffffffffull - (best & 0xffffffffull);
                    const long long s = rc_pair_lookup(bests, p.pcap, k);
                    row[0] = (long long)k; row[1] = (long long)(best >> 32);
                    row[4] = (s >= 0 && 0xffffffffull - (bests[2 * s + 1] & 0xffffffffull) == (rc_u64)i) ? 1 : 0;
                }
            }
            if (i < klim) {
                const long long s = rc_pair_lookup(bests, p.pcap, (rc_u64)i);
                if (s >= 0) {
                    long long *row = p.back + ((size_t)n * p.kcap + i) * 4;
                    const rc_u64 best = bests[2 * s + 1];
                    row[0] = (long long)(0xffffffffull - (best & 0xffffffffull)); row[1] = (long long)(best >> 32);
                }
            }
        }
    }
}

int lk_side(LkSide &s, const int32_t *row_start, const uint32_t *runs, const int32_t *n_regions, const int32_t *run_region, int64_t cap) {
    ARSEG_CHECK_PTR(row_start); ARSEG_CHECK_PTR(runs); ARSEG_CHECK_PTR(n_regions); ARSEG_CHECK_PTR(run_region);
    if (cap <= 0) return ARSEG_EINVAL;
    if (rc_misaligned(4, row_start, runs, n_regions, run_region)) return ARSEG_EINVAL;
    s.rs = row_start; s.runs = runs; s.nreg = n_regions; s.rr = run_region;
    s.cap_stride = cap; s.cap = rc_cap(cap);
    return ARSEG_OK;
}

}  // namespace

// per frame: two tables of pcap slots of two 64-bit words, and the flag
extern "C" size_t arseg_region_links_workspace_bytes(int N, int64_t pcap) {
    if (N <= 0 || pcap <= 0) return 0;
    return (size_t)N * ((size_t)pcap * 32 + 8);
}

extern "C" int arseg_region_links_fwd(const int32_t *row_start, const uint32_t *runs, const int32_t *n_regions, const int32_t *run_region,
                                      int64_t cap, const int32_t *ref_row_start, const uint32_t *ref_runs, const int32_t *ref_n_regions,
                                      const int32_t *ref_run_region, int64_t ref_cap, int ref_shared, const int16_t *mv_q, int N, int H, int W,
                                      int32_t *n_pairs, int64_t *links, int64_t rcap, int64_t *back, int64_t kcap, int64_t pcap,
                                      void *workspace, size_t workspace_bytes, arseg_stream_t stream) {
    LkP p = {};
    int rc = lk_side(p.cur, row_start, runs, n_regions, run_region, cap);
    if (rc != ARSEG_OK) return rc;
    rc = lk_side(p.ref, ref_row_start, ref_runs, ref_n_regions, ref_run_region, ref_cap);
    if (rc != ARSEG_OK) return rc;
    ARSEG_CHECK_PTR(n_pairs);
    ARSEG_CHECK_POS(N); ARSEG_CHECK_POS(H); ARSEG_CHECK_POS(W);
    if (pcap <= 0 || rcap < 0 || kcap < 0 || (links == nullptr && rcap > 0) || (back == nullptr && kcap > 0)) return ARSEG_EINVAL;
    if (ref_shared != 0 && ref_shared != 1) return ARSEG_EINVAL;
    if (W > (1 << 24) || (int64_t)H * W > (int64_t)INT32_MAX) return ARSEG_EINVAL;
    if (rc_misaligned(4, n_pairs, mv_q) || rc_misaligned(8, links, back, workspace)) return ARSEG_EINVAL;
    if (workspace_bytes < arseg_region_links_workspace_bytes(N, pcap)) return ARSEG_EWORKSPACE;
    ARSEG_CHECK_PTR(workspace);
    p.mv = reinterpret_cast<const unsigned *>(mv_q);
    p.npairs = n_pairs;
    p.links = links ? reinterpret_cast<long long *>(links) : nullptr; p.rcap = links ? rcap : 0;
    p.back = back ? reinterpret_cast<long long *>(back) : nullptr; p.kcap = back ? kcap : 0;
    p.pcap = pcap;
    p.pairs = static_cast<rc_u64 *>(workspace);
    p.bests = p.pairs + (size_t)N * (size_t)pcap * 2;
    p.flag = reinterpret_cast<unsigned *>(p.bests + (size_t)N * (size_t)pcap * 2);
    p.N = N; p.H = H; p.W = W; p.shared = ref_shared;
    hipStream_t st = arseg_stream(stream);
    // a frame has at most min(cap, H * W) regions: the records beyond cannot be in use
    const long long most = p.rcap > p.kcap ? p.rcap : p.kcap, regions_most = p.cur.cap > p.ref.cap ? p.cur.cap : p.ref.cap;
    const dim3 per_slot = rc_grid(N, pcap, 256, 16384), per_row = rc_grid(N, H, LK_WAVES, 16384);
    const dim3 per_rec = rc_grid(N, most < regions_most ? most : regions_most, 256, 16384);
    hipLaunchKernelGGL(links_clear_kernel, per_slot, dim3(256), 0, st, p);
    hipLaunchKernelGGL((links_vote_kernel<false>), per_row, dim3(64 * LK_WAVES), 0, st, p);
    hipLaunchKernelGGL(links_rows_kernel, per_rec, dim3(256), 0, st, p);
    if (mv_q && p.links) hipLaunchKernelGGL((links_vote_kernel<true>), per_row, dim3(64 * LK_WAVES), 0, st, p);
    hipLaunchKernelGGL(links_resolve_kernel, per_slot, dim3(256), 0, st, p);
    hipLaunchKernelGGL(links_finish_kernel, per_rec, dim3(256), 0, st, p);
    return arseg_launch_status();
}
