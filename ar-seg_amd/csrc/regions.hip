// Connected regions of a row-run code (include/arseg_hip.h, arseg_rle_regions_fwd): row_start int32 [N][H+1] and runs uint32 [N][cap] as
// arseg_labels_rle_fwd writes them in; per frame the number of regions, the region of every run and one record of 8 int64 per region out.  A
// union-find over a few thousand runs instead of two million pixels: the plane is never read.  The first kernels here that chase pointers and
// merge without locks.
//
// The forest lives in the caller's workspace: parent int32 [N][cap], an index into the frame's runs.
//   PARENTS ONLY EVER POINT TO SMALLER INDICES (or to the slot itself: a root), and a slot's parent only ever decreases.  Every loop that
//   follows a parent pointer therefore visits strictly decreasing indices >= 0 and ends after at most `index` steps, whatever the run code
//   holds and in whatever order the merges happen; and the root of a finished tree is its smallest index, so the result does not depend on
//   timing either.  Every value of parent is written by these kernels (init, atomicMin of a valid index, a store of an ancestor): a malformed
//   run code can make the regions meaningless, it cannot make a parent point outside [0, stored runs).
// Five launches; a phase boundary is a launch boundary: no workgroup waits for another, no flags, no look-back, no spinning on memory.
//   init     parent[i] = i for the stored runs.
//   link     a wave owns a row y >= 1 (grid-stride over the rows, blockIdx.y strides over the frames), its lanes take the row's runs at stride
//            64.  A lane finds the first run of row y - 1 that reaches its own by binary search on x_first, walks right while the overlap
//            holds and unites itself with every neighbour of its value: find both roots, atomicMin the smaller root into the larger root's
//            slot, go on from the value that was there when the slot was no longer a root.  Vector atomics on global memory only.  The finds
//            read with agent-scope loads (past the L1); a stale parent is an earlier, larger ancestor of the same tree and costs a step, not
//            the result: only what atomicMin returns decides.
//   flatten  parent[i] <- parent[parent[i]] until parent[i] is a root (pointer jumping, in place: a slot only moves to a higher ancestor, so
//            a reader meets an ancestor whichever value it sees).  Afterwards every slot holds its root, and i is a root iff parent[i] == i.
//   number   one workgroup per frame: the root flags of the stored runs scanned 256 at a time with a carry (rc_block_scan).  A root
//            gets its dense number into run_region and, below rcap, its record initialised (value; area = sums = 0; min = INT64_MAX;
//            max = -1); n_regions[n] = R, or -1 for a frame whose run code overflowed.
//   relabel  a wave takes 64 consecutive runs: run_region[i] = run_region[parent[i]]; the row of a run by binary search in row_start; the
//            run's span goes into its region's record with 64-bit integer atomics, reduced over the lanes of the wave that share a region
//            first (a background region holds hundreds of runs): the lanes of the first region still open are balloted, their values reduced,
//            and the first of them issues the 7 atomics.  Integers throughout: two runs of the program are bit-equal.
// A frame with row_start[n][H] > cap is skipped by every kernel (decided on the device, from row_start alone).
#include "runcode.h"

namespace {

constexpr int REG_WAVES = 4;                            // waves per workgroup

struct RegP {
    const int *rs;                                      // [N][H + 1]
    const unsigned *runs;                               // [N][cap]
    int *par;                                           // [N][cap]: the workspace
    int *rr;                                            // run_region [N][cap]
    long long *reg;                                     // regions [N][rcap][8] (may be null: rcap == 0)
    int *nreg;                                          // [N]
    long long cap_stride, rcap_stride;                  // words / records from frame to frame
    int cap, rcap;                                      // min(., INT32_MAX): an index is below 2^31
    int N, H, W;
    int d;                                              // 0: 4-connectivity, 1: 8-connectivity (a diagonal step closes a gap of one column)
};

// The stored runs of a frame: row_start[n][H], never below 0; -1 for a frame whose run code overflowed.  At most cap either way.
__device__ __forceinline__ int reg_total(const RegP &p, const int *rs) { return rc_stored(rs[p.H], p.cap); }

__device__ __forceinline__ int reg_load(const int *q) { return __hip_atomic_load(q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// The root above x.  Bounded: x strictly decreases (a negative or larger value would end the walk as well).
__device__ __forceinline__ int reg_find(const int *par, int x) {
    for (;;) {
        const int q = reg_load(par + x);
        if ((unsigned)q >= (unsigned)x) return x;
        x = q;
    }
}

// Unite the trees of a and b.  Bounded: from one round to the next max(a, b) strictly decreases.
__device__ __forceinline__ void reg_unite(int *par, int a, int b) {
    for (;;) {
        a = reg_find(par, a); b = reg_find(par, b);
        if (a == b) return;
        const int hi = max(a, b), lo = min(a, b);
        const int old = atomicMin(par + hi, lo);
        if (old == hi) return;                          // hi was a root and hangs under lo now
        a = old; b = lo;                                // hi hung under old < hi already: its slot holds min(old, lo), old and lo remain to unite
    }
}

__global__ __launch_bounds__(64 * REG_WAVES) void regions_init_kernel(const RegP p) {
    for (int n = blockIdx.y; n < p.N; n += gridDim.y) {
        const int total = reg_total(p, p.rs + (size_t)n * (p.H + 1));
        int *par = p.par + (size_t)n * p.cap_stride;
        for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) par[i] = i;
    }
}

__global__ __launch_bounds__(64 * REG_WAVES) void regions_link_kernel(const RegP p) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int n = blockIdx.y; n < p.N; n += gridDim.y) {
        const int *rs = p.rs + (size_t)n * (p.H + 1);
        const int total = reg_total(p, rs);
        if (total <= 0) continue;
        const unsigned *runs = p.runs + (size_t)n * p.cap_stride;
        int *par = p.par + (size_t)n * p.cap_stride;
        for (int y = 1 + blockIdx.x * REG_WAVES + wave; y < p.H; y += gridDim.x * REG_WAVES) {
            // a malformed row_start may not lead outside [0, total): both rows are clamped into it
            int pf, pl, first, last;
            rc_row(rs, y - 1, total, pf, pl);
            rc_row(rs, y, total, first, last);
            if (pl <= pf) continue;
            for (int i = first + lane; i < last; i += 64) {
                const unsigned word = runs[i];
                const int a0 = rc_x0(runs, i, p.W), a1 = rc_x1(runs, i, last, p.W);
                // from the first run j of row y - 1 with b1 + d > a0 on: b1 is the start of run j + 1, or W behind the row's last run
                for (int j = rc_cover(runs, pf, pl, a0 - p.d); j < pl; ++j) {
                    const unsigned other = runs[j];
                    if ((int)(other >> 8) >= a1 + p.d) break;              // b0 < a1 + d ends here: the row is sorted
                    if (((other ^ word) & 0xffu) == 0) reg_unite(par, i, j);
                }
            }
        }
    }
}

__global__ __launch_bounds__(64 * REG_WAVES) void regions_flatten_kernel(const RegP p) {
    for (int n = blockIdx.y; n < p.N; n += gridDim.y) {
        const int total = reg_total(p, p.rs + (size_t)n * (p.H + 1));
        int *par = p.par + (size_t)n * p.cap_stride;
        for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
            int q = reg_load(par + i);
            while ((unsigned)q < (unsigned)i) {                             // bounded: q strictly decreases
                const int g = reg_load(par + q);
                if ((unsigned)g >= (unsigned)q) break;                      // q is a root
                __hip_atomic_store(par + i, g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                q = g;
            }
        }
    }
}

__global__ __launch_bounds__(256) void regions_number_kernel(const RegP p) {
    __shared__ int part[4];
    for (int n = blockIdx.x; n < p.N; n += gridDim.x) {
        const int total = reg_total(p, p.rs + (size_t)n * (p.H + 1));
        if (total < 0) {
            if (threadIdx.x == 0) p.nreg[n] = -1;
            continue;
        }
        const unsigned *runs = p.runs + (size_t)n * p.cap_stride;
        const int *par = p.par + (size_t)n * p.cap_stride;
        int *rr = p.rr + (size_t)n * p.cap_stride;
        int carry = 0;
        for (int i0 = 0; i0 < total; i0 += 256) {
            const int i = i0 + (int)threadIdx.x;
            const bool root = i < total && par[i] == i;
            int inc = root ? 1 : 0;
            rc_block_scan<1>(&inc, &carry, part);
            if (root) {
                const int k = inc - 1;
                rr[i] = k;
                if (k < p.rcap) {
                    long long *row = p.reg + ((size_t)n * p.rcap_stride + k) * 8;
                    row[0] = runs[i] & 0xffu; row[1] = 0;
                    row[2] = LLONG_MAX; row[3] = LLONG_MAX;
                    row[4] = -1; row[5] = -1;
                    row[6] = 0; row[7] = 0;
                }
            }
        }
        if (threadIdx.x == 0) p.nreg[n] = carry;
    }
}

__global__ __launch_bounds__(64 * REG_WAVES) void regions_relabel_kernel(const RegP p) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int n = blockIdx.y; n < p.N; n += gridDim.y) {
        const int *rs = p.rs + (size_t)n * (p.H + 1);
        const int total = reg_total(p, rs);
        const unsigned *runs = p.runs + (size_t)n * p.cap_stride;
        const int *par = p.par + (size_t)n * p.cap_stride;
        int *rr = p.rr + (size_t)n * p.cap_stride;
        for (int i0 = (blockIdx.x * REG_WAVES + wave) * 64; i0 < total; i0 += gridDim.x * REG_WAVES * 64) {       // i0 is wave uniform
            const int i = i0 + lane;
            int k = -1;
            long long area = 0, sx = 0, sy = 0;
            int x_lo = INT_MAX, y_lo = INT_MAX, x_hi = -1, y_hi = -1;
            if (i < total) {
                const int root = par[i];                // a root after flatten: its number is in place since the last launch
                k = rr[root];
                if (root != i) rr[i] = k;
                if (k < p.rcap) {
                    int y = 0, top = p.H - 1;           // the last row with row_start <= i
                    while (y < top) {
                        const int mid = (y + top + 1) >> 1;
                        if (rs[mid] <= i) y = mid; else top = mid - 1;
                    }
                    const int a0 = rc_x0(runs, i, p.W), a1 = rc_x1(runs, i, min(rs[y + 1], total), p.W);
                    const long long len = a1 - a0;
                    area = len; sx = (long long)(a0 + a1 - 1) * len / 2; sy = (long long)y * len;
                    x_lo = a0; x_hi = a1 - 1; y_lo = y_hi = y;
                } else {
                    k = -1;                             // beyond the record capacity: labelled, not accumulated
                }
            }
            unsigned long long todo = __ballot(k >= 0);
            while (todo) {                              // one round per region among the wave's runs: at most 64
                const int leader = __ffsll((long long)todo) - 1;
                const int kl = __shfl(k, leader, 64);
                const bool mine = k == kl;
                const unsigned long long group = __ballot(mine);
                todo &= ~group;
                long long A = mine ? area : 0, SX = mine ? sx : 0, SY = mine ? sy : 0;
                int x0 = mine ? x_lo : INT_MAX, y0 = mine ? y_lo : INT_MAX, x1 = mine ? x_hi : -1, y1 = mine ? y_hi : -1;
                if (group & (group - 1)) {              // more than one lane
#pragma unroll
                    for (int o = 32; o > 0; o >>= 1) {
                        A += __shfl_xor(A, o, 64); SX += __shfl_xor(SX, o, 64); SY += __shfl_xor(SY, o, 64);
                        x0 = min(x0, __shfl_xor(x0, o, 64)); y0 = min(y0, __shfl_xor(y0, o, 64));
                        x1 = max(x1, __shfl_xor(x1, o, 64)); y1 = max(y1, __shfl_xor(y1, o, 64));
                    }
                }
                if (lane == leader) {
                    long long *row = p.reg + ((size_t)n * p.rcap_stride + kl) * 8;
                    atomicAdd(reinterpret_cast<unsigned long long *>(row + 1), (unsigned long long)A);
                    atomicMin(row + 2, (long long)x0); atomicMin(row + 3, (long long)y0);
                    atomicMax(row + 4, (long long)x1); atomicMax(row + 5, (long long)y1);
                    atomicAdd(reinterpret_cast<unsigned long long *>(row + 6), (unsigned long long)SX);
                    atomicAdd(reinterpret_cast<unsigned long long *>(row + 7), (unsigned long long)SY);
                }
            }
        }
    }
}

}  // namespace

extern "C" size_t arseg_rle_regions_workspace_bytes(int N, int64_t cap) {
    if (N <= 0 || cap <= 0) return 0;
    return (size_t)N * (size_t)cap * sizeof(int32_t);
}

extern "C" int arseg_rle_regions_fwd(const int32_t *row_start, const uint32_t *runs, int64_t cap, int N, int H, int W, int connectivity,
                                     int32_t *n_regions, int32_t *run_region, int64_t *regions, int64_t rcap, void *workspace,
                                     size_t workspace_bytes, arseg_stream_t stream) {
    ARSEG_CHECK_PTR(row_start); ARSEG_CHECK_PTR(runs); ARSEG_CHECK_PTR(n_regions); ARSEG_CHECK_PTR(run_region);
    ARSEG_CHECK_POS(N); ARSEG_CHECK_POS(H); ARSEG_CHECK_POS(W);
    if (cap <= 0 || rcap < 0 || (regions == nullptr && rcap > 0)) return ARSEG_EINVAL;
    if (connectivity != 4 && connectivity != 8) return ARSEG_EINVAL;
    if (W > (1 << 24) || (int64_t)H * W > (int64_t)INT32_MAX) return ARSEG_EINVAL;
    if (rc_misaligned(4, row_start, runs, n_regions, run_region, workspace) || rc_misaligned(8, regions)) return ARSEG_EINVAL;
    if (workspace_bytes < arseg_rle_regions_workspace_bytes(N, cap)) return ARSEG_EWORKSPACE;
    ARSEG_CHECK_PTR(workspace);
    RegP p = {};
    p.rs = row_start; p.runs = runs; p.par = static_cast<int *>(workspace); p.rr = run_region;
    p.reg = regions ? reinterpret_cast<long long *>(regions) : nullptr; p.nreg = n_regions;
    p.cap_stride = cap; p.rcap_stride = regions ? rcap : 0;
    p.cap = rc_cap(cap); p.rcap = regions ? rc_cap(rcap) : 0;
    p.N = N; p.H = H; p.W = W; p.d = connectivity == 8 ? 1 : 0;
    hipStream_t st = arseg_stream(stream);
    const dim3 per_run = rc_grid(N, p.cap, 64 * REG_WAVES, 16384), per_row = rc_grid(N, H, REG_WAVES, 16384), block(64 * REG_WAVES);
    hipLaunchKernelGGL(regions_init_kernel, per_run, block, 0, st, p);
    if (H > 1) hipLaunchKernelGGL(regions_link_kernel, per_row, block, 0, st, p);
    hipLaunchKernelGGL(regions_flatten_kernel, per_run, block, 0, st, p);
    hipLaunchKernelGGL(regions_number_kernel, rc_frames(N), dim3(256), 0, st, p);
    hipLaunchKernelGGL(regions_relabel_kernel, per_run, block, 0, st, p);
    return arseg_launch_status();
}
