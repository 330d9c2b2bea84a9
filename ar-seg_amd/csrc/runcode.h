// The row-run code of a label plane, defined once for the passes that work on it (rle.hip, regions.hip, links.hip, absorb.hip, contours.hip,
// simplify.hip, simplify_shared.hip): row_start int32 [N][H + 1] is the exclusive prefix of the rows' run counts, runs uint32 [N][cap] holds one word
// (x_first << 8) | value per run in (y, x) order, and a run ends where the next run of its row begins, or at W.  A frame whose
// row_start[n][H] exceeds cap overflowed: its runs are not all stored and every pass refuses it.
//
// Everything here clamps: a row's runs into [0, stored runs) of its frame, a column into [0, W], a run's end into [its start, W].  A
// malformed code therefore gives meaningless results and no access outside runs[n][0 .. stored runs).  With it live the two tools the
// passes share: the open-addressed table of 64-bit keys (links.hip, absorb.hip) and the 256-thread scan with a carry.
#pragma once
#include "arseg_device.h"

#include <limits.h>

typedef unsigned long long rc_u64;

// ------------------------------------------------------------------ frames, rows and runs
__device__ __forceinline__ int rc_clamp(int v, int lo, int hi) { return min(max(v, lo), hi); }

// The stored runs of a frame that needs `need` = row_start[n][H] of them: never below 0, -1 for a frame whose run code overflowed.
__device__ __forceinline__ int rc_stored(int need, int cap) { return need > cap ? -1 : max(need, 0); }

// Row y's runs [first, last), clamped into [0, total): a malformed row_start may not lead outside the stored runs.
__device__ __forceinline__ void rc_row(const int *rs, int y, int total, int &first, int &last) {
    first = rc_clamp(rs[y], 0, total);
    last = rc_clamp(rs[y + 1], first, total);
}

// The first column of run i and the column behind its last one; last: the end of run i's row.  0 <= x0 <= x1 <= W.
__device__ __forceinline__ int rc_x0(const unsigned *runs, int i, int W) { return min((int)(runs[i] >> 8), W); }
__device__ __forceinline__ int rc_x1(const unsigned *runs, int i, int last, int W) {
    return i + 1 < last ? rc_clamp((int)(runs[i + 1] >> 8), rc_x0(runs, i, W), W) : W;
}

// The run of the row [first, last), first < last, that covers column x: the last one that starts at or before x, the first one when none
// does.  A binary search: at most 31 rounds.
__device__ __forceinline__ int rc_cover(const unsigned *runs, int first, int last, int x) {
    int lo = first + 1, hi = last;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if ((int)(runs[mid] >> 8) > x) hi = mid; else lo = mid + 1;
    }
    return lo - 1;
}

// ------------------------------------------------------------------ a table of pcap slots {key, word}, open addressed with linear probing
constexpr rc_u64 RC_EMPTY = ~0ull;                      // no key

__device__ __forceinline__ long long rc_pair_slot(rc_u64 key, long long pcap) {
    const rc_u64 h = (key * 0x9E3779B97F4A7C15ull) >> 32;
    return pcap < (1ll << 32) ? (long long)((h * (rc_u64)pcap) >> 32) : (long long)h;
}
// The slot of key, taken when the key is new; -1 when all pcap slots hold other keys.  One slot per round: pcap rounds at the most.
__device__ __forceinline__ long long rc_pair_insert(rc_u64 *tab, long long pcap, rc_u64 key) {
    long long s = rc_pair_slot(key, pcap);
    for (long long t = 0; t < pcap; ++t) {
        rc_u64 old = __hip_atomic_load(tab + 2 * s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (old == RC_EMPTY) old = atomicCAS(tab + 2 * s, RC_EMPTY, key);
        if (old == RC_EMPTY || old == key) return s;
        s = s + 1 == pcap ? 0 : s + 1;
    }
    return -1;
}
// The slot of key in a finished table, -1 when it is not there.
__device__ __forceinline__ long long rc_pair_lookup(const rc_u64 *tab, long long pcap, rc_u64 key) {
    long long s = rc_pair_slot(key, pcap);
    for (long long t = 0; t < pcap; ++t) {
        const rc_u64 old = tab[2 * s];
        if (old == key) return s;
        if (old == RC_EMPTY) return -1;
        s = s + 1 == pcap ? 0 : s + 1;
    }
    return -1;
}

// Lanes next to each other that hold one key: true on the first lane of each stretch, with the stretch's length.  Every lane of the wave calls.
__device__ __forceinline__ bool rc_segment(rc_u64 key, int lane, int &len) {
    const rc_u64 left = __shfl_up(key, 1, 64);
    const bool head = lane == 0 || left != key;
    const rc_u64 heads = __ballot(head);
    const rc_u64 after = lane == 63 ? 0ull : heads >> (lane + 1);
    len = after ? __ffsll((long long)after) : 64 - lane;
    return head;
}

// ------------------------------------------------------------------ the scan
// One pass of a workgroup of 256 threads over 256 items with K values each: v[k] comes back as carry[k] plus the values of the threads up
// to and including this one, and carry[k] grows by the pass's total.  part: 4 K words of LDS.  Every thread calls, in uniform control flow;
// one pair of barriers per pass, whatever K is, the second one so that the next pass may write part again.
template <int K, class T>
__device__ __forceinline__ void rc_block_scan(T *v, T *carry, T *part) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const T t = __shfl_up(v[k], o, 64);
            v[k] += lane >= o ? t : 0;
        }
    }
#pragma unroll
    for (int k = 0; k < K; ++k)
        if (lane == 63) part[4 * k + wave] = v[k];
    __syncthreads();
#pragma unroll
    for (int k = 0; k < K; ++k) {
        T before = carry[k];
#pragma unroll
        for (int w = 0; w < 4; ++w) before += w < wave ? part[4 * k + w] : 0;
        carry[k] += part[4 * k] + part[4 * k + 1] + part[4 * k + 2] + part[4 * k + 3];
        v[k] += before;
    }
    __syncthreads();
}

// ------------------------------------------------------------------ host side
// workgroups per frame x frames for `items` items of work a workgroup takes `per` of, at most about `budget` in all: the kernels stride
static inline dim3 rc_grid(int N, long long items, int per, int budget) {
    const int gy = N < 65535 ? N : 65535;
    const long long share = budget / gy > 0 ? budget / gy : 1, need = (items + per - 1) / per;
    return dim3((unsigned)(need < share ? (need > 0 ? need : 1) : share), (unsigned)gy);
}
// one workgroup per frame, for the kernels that scan
static inline dim3 rc_frames(int N) { return dim3((unsigned)(N < 65535 ? N : 65535)); }

// a capacity as the kernels hold it: an index is below 2^31
static inline int rc_cap(int64_t cap) { return (int)(cap < (int64_t)INT32_MAX ? cap : (int64_t)INT32_MAX); }

// any of the pointers not a multiple of `align` (a power of two); null pointers pass
template <class... P>
static inline bool rc_misaligned(uintptr_t align, const P *...p) { return ((reinterpret_cast<uintptr_t>(p) | ...) & (align - 1)) != 0; }
