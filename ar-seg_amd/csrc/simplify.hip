// Region outlines simplified to a pixel tolerance (include/arseg_hip.h, arseg_contours_simplify_fwd): counts, loops and verts as
// arseg_rle_contours_fwd leaves them in; per loop the vertices that Douglas-Peucker keeps -- on the two chains between the loop's first
// vertex and the vertex farthest from it -- out, in the same layout.  Integers throughout: every output is a pure function of the inputs.
// The pass reads and writes a few thousand words per frame, all of them in L2; it is bound by the latency of the longest loop's walk.
//
// Scratch lives in the caller's workspace: per frame and loop slot the loop's kept count (int32 [N][lcap]), per frame and vertex slot a
// keep flag (a byte, [N][vcap rounded up to 4]).
// 4 launches, sized on the host from the capacities; a phase boundary is a launch boundary: no workgroup waits for another, nothing spins
// on memory, no atomics are needed.
//   clear    the refusal decision: counts_out = {-1, -1} or {0, 0}; the keep flags below the frame's V are zeroed.
//   keep     a wave owns a loop (grid-stride over the loops, blockIdx.y strides over the frames).  The farthest vertex from P[0] by a
//            strided argmax and a wave reduction; then the recursion without a stack, the keep flags being the stack: with a final, b is
//            the next kept position after a; the interior of (a, b) is scanned 256 at a time for the key {c, smallest position} and the
//            key reduced over the wave; a vertex beyond the tolerance is kept and becomes b, otherwise a moves to b.  A flag is stored by
//            every lane of the wave (the position is uniform), so each lane reads back only bytes it has stored itself or that the clear
//            launch zeroed: program order alone makes the flags visible, no fence is needed.  A loop of at most SP_STAGE = 2048 vertices
//            is first copied into the wave's own LDS with its flags, walked there and its flags copied out: a round then waits for
//            LDS, not for L2.  Longer loops are walked in place.  The kept count after the fewer-than-3 rule.
//   scan     one workgroup per frame: the prefix with a carry (rc_block_scan) over the loops' kept counts -> counts_out and the loop records.
//   emit     a wave owns a loop: the kept vertices (all of them for a loop kept whole) compacted in order with a ballot prefix to first';
//            words below vcap_out only.  Not launched without verts_out.
//
// Bounds of the loops (nothing else loops):
//   grid-stride loops      over frames, loops, flag words and the vertices of a loop (the copies to and from LDS too): counted.
//   the walk               every round either keeps a vertex (at most count - 2 times) or advances a to the next kept position (at most
//                          count times): it ends within 2 count rounds, and the loop is given 2 count + 2 explicitly.
//   the search for b       64 flags per round from a + 1 to the loop's end: counted.
//   the reductions         4 DPP steps and 2 lane swaps (arseg_device.h, wave_max_u64).
// Clamps: a frame is processed only with 0 <= L <= lcap and 0 <= V <= vcap; a loop's first is clamped into [0, V] and its count into
// [0, V - first], so every vertex and flag index stays below V <= vcap, and an index into the LDS stage below count <= SP_STAGE; a position taken from a reduced key is clamped into the segment
// it was found in; an output index is used only below vcap_out, a loop index only below L <= lcap.  Coordinates are taken as 16-bit
// fields and multiplied as unsigned words: a malformed vertex gives a meaningless product, never a trap.  No division is made.  A
// malformed loop record gives meaningless output and touches nothing outside the caller's buffers.
#include "runcode.h"

namespace {

typedef int sp_i32x4 __attribute__((ext_vector_type(4), aligned(4)));

constexpr int SP_WAVES = 4;                             // waves (= loops in flight) per workgroup
constexpr int SP_STAGE = 2048;                          // the longest loop a wave stages in LDS: 10 KiB per wave, 40 per workgroup

struct SpP {
    const int *counts;                                  // [N][2]
    const int *loops;                                   // [N][lcap][4]
    const unsigned *verts;                              // [N][vcap]
    int *counts_out;                                    // [N][2]
    int *loops_out;                                     // [N][lcap][4]
    unsigned *verts_out;                                // [N][vcap_out] (may be null: vcap_out == 0)
    int *kept;                                          // [N][lcap]
    unsigned char *flags;                               // [N][fstride]
    long long lcap, vcap, vcap_out, fstride;
    unsigned long long tol;                             // 16 x the squared tolerance
    int N;
};

// The loops and vertices of a frame; false for a frame that is refused: its source was refused or overflowed.
__device__ __forceinline__ bool sp_frame(const SpP &p, int n, int &L, int &V) {
    L = p.counts[2 * (size_t)n]; V = p.counts[2 * (size_t)n + 1];
    return L >= 0 && V >= 0 && L <= p.lcap && V <= p.vcap;
}

// A loop's record -> its first vertex and its count, clamped into the frame's V vertices.
__device__ __forceinline__ void sp_loop(const SpP &p, int n, int l, int V, int &first, int &cnt) {
    const int *rec = p.loops + ((size_t)n * p.lcap + l) * 4;
    first = rc_clamp(rec[1], 0, V);
    cnt = rc_clamp(rec[2], 0, V - first);
}

// {value, smallest position} as one key: the larger value wins, then the smaller position.
__device__ __forceinline__ unsigned long long sp_key(unsigned value, int pos) { return ((unsigned long long)value << 32) | (0xffffffffu - (unsigned)pos); }
__device__ __forceinline__ int sp_key_pos(unsigned long long key) { return (int)(0xffffffffu - (unsigned)key); }

__device__ __forceinline__ unsigned sp_abs(unsigned v) { return (int)v < 0 ? 0u - v : v; }

__global__ __launch_bounds__(256) void simplify_clear_kernel(const SpP p) {
    for (int n = blockIdx.y; n < p.N; n += gridDim.y) {
        int L, V;
        const bool ok = sp_frame(p, n, L, V);
        if (blockIdx.x == 0 && threadIdx.x == 0) { p.counts_out[2 * (size_t)n] = ok ? 0 : -1; p.counts_out[2 * (size_t)n + 1] = ok ? 0 : -1; }
        if (!ok) continue;
        unsigned *words = reinterpret_cast<unsigned *>(p.flags + (size_t)n * p.fstride);           // V <= vcap: (V + 3) / 4 words lie within fstride
        const int nw = (V + 3) >> 2;
        for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < nw; i += gridDim.x * blockDim.x) words[i] = 0u;
    }
}

// The anchors and the walk of one loop of cnt >= 3 vertices, by one wave: P its vertices, F its keep flags (all zero), both in global
// memory or both in the wave's LDS stage -> the number of flags set.  Everything but the strided scans is uniform.
__device__ __forceinline__ int sp_walk(const unsigned *P, unsigned char *F, int cnt, unsigned long long tol, int lane) {
    // ---- the farthest vertex from P[0], the smallest position of a tie
    const unsigned w0 = P[0], x0 = w0 & 0xffffu, y0 = w0 >> 16;
    unsigned long long key = 0;
    for (int base = 0; base < cnt; base += 256) {
        unsigned w[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) w[u] = P[min(base + 64 * u + lane, cnt - 1)];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int i = base + 64 * u + lane;
            const unsigned dx = (w[u] & 0xffffu) - x0, dy = (w[u] >> 16) - y0;
            const unsigned long long k = sp_key(dx * dx + dy * dy, i);
            key = i < cnt && k > key ? k : key;
        }
    }
    key = wave_max_u64(key);                                                  // (lane 0 holds position 0: the key is never empty)
    const int a1 = rc_clamp(sp_key_pos(key), 0, cnt - 1);
    F[0] = 1; F[a1] = 1;                                                      // every lane stores: see the head of the file
    int kept = a1 > 0 ? 2 : 1;
    // ---- the walk: a is final, b the next kept position after it (cnt stands for the closing P[0])
    int a = 0, b = a1 > 0 ? a1 : cnt;
    for (int round = 0; round < 2 * cnt + 2 && a < cnt; ++round) {
        bool marked = false;
        if (b - a > 1) {
            const unsigned wa = P[a], wb = P[b < cnt ? b : 0];
            const unsigned xa = wa & 0xffffu, ya = wa >> 16, ex = (wb & 0xffffu) - xa, ey = (wb >> 16) - ya;
            key = 0;
            for (int base = a + 1; base < b; base += 256) {
                unsigned w[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) w[u] = P[min(base + 64 * u + lane, b - 1)];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int i = base + 64 * u + lane;
                    const unsigned c = sp_abs(ex * ((w[u] >> 16) - ya) - ey * ((w[u] & 0xffffu) - xa));      // 32-bit products
                    const unsigned long long k = sp_key(c, i);
                    key = i < b && k > key ? k : key;
                }
            }
            key = wave_max_u64(key);
            const unsigned long long c = key >> 32, len2 = (unsigned long long)(ex * ex + ey * ey);
            if (16ull * c * c > tol * len2) {                                // uniform: the one 64-bit comparison of the segment
                const int i = rc_clamp(sp_key_pos(key), a + 1, b - 1);
                F[i] = 1;
                ++kept; b = i; marked = true;
            }
        }
        if (!marked) {                                                       // every interior vertex of (a, b) is dropped
            a = b; b = cnt;
            for (int base = a + 1; base < cnt; base += 64) {
                const int i = base + lane;
                const unsigned long long m = __builtin_amdgcn_ballot_w64(i < cnt && F[min(i, cnt - 1)] != 0);
                if (m) { b = base + __builtin_ctzll(m); break; }
            }
        }
    }
    return kept;
}

__global__ __launch_bounds__(64 * SP_WAVES) void simplify_keep_kernel(const SpP p) {
    __shared__ unsigned stage_p[SP_WAVES][SP_STAGE];
    __shared__ unsigned stage_f[SP_WAVES][SP_STAGE / 4];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    for (int n = blockIdx.y; n < p.N; n += gridDim.y) {
        int L, V;
        if (!sp_frame(p, n, L, V)) continue;
        for (int l = blockIdx.x * SP_WAVES + wave; l < L; l += gridDim.x * SP_WAVES) {              // waves beyond L leave at once
            int first, cnt;
            sp_loop(p, n, l, V, first, cnt);
            first = __builtin_amdgcn_readfirstlane(first); cnt = __builtin_amdgcn_readfirstlane(cnt);
            const unsigned *P = p.verts + (size_t)n * p.vcap + first;
            unsigned char *F = p.flags + (size_t)n * p.fstride + first;
            int kept = cnt;
            if (cnt >= 3 && cnt <= SP_STAGE) {                               // (fewer than 3 cannot keep three: the loop goes out whole)
                // the loop and its flags staged in the wave's own LDS: a round of the walk costs LDS latencies instead of L2's.  Only
                // this wave touches its stage; a wave's LDS accesses are served in order, and the fences keep the compiler from moving
                // an access across them.
                unsigned *sp = stage_p[wave];
                unsigned char *sf = reinterpret_cast<unsigned char *>(stage_f[wave]);
                for (int i = lane; i < cnt; i += 64) sp[i] = P[i];
                for (int i = lane; i < (cnt + 3) >> 2; i += 64) stage_f[wave][i] = 0u;
                __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
                __builtin_amdgcn_wave_barrier();
                kept = sp_walk(sp, sf, cnt, p.tol, lane);
                __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
                __builtin_amdgcn_wave_barrier();
                for (int i = lane; i < cnt; i += 64) F[i] = sf[i];
            } else if (cnt >= 3) {
                kept = sp_walk(P, F, cnt, p.tol, lane);                      // a longer loop: in place, on the flags the clear launch zeroed
            }
            if (kept < 3) kept = cnt;                                        // no collapse: the loop goes out whole
            if (lane == 0) p.kept[(size_t)n * p.lcap + l] = kept;
        }
    }
}

// Per frame: the kept counts summed over the loops, 256 at a time with a carry (rc_block_scan) -> the loop records and counts_out.
__global__ __launch_bounds__(256) void simplify_scan_kernel(const SpP p) {
    __shared__ unsigned part[4];
    for (int n = blockIdx.x; n < p.N; n += gridDim.x) {
        int L, V;
        if (!sp_frame(p, n, L, V)) continue;
        unsigned carry = 0;
        for (int l0 = 0; l0 < L; l0 += 256) {                                // l0 is uniform: every thread makes every pass
            const int l = l0 + (int)threadIdx.x;
            const unsigned count = l < L ? (unsigned)p.kept[(size_t)n * p.lcap + l] : 0u;
            unsigned inc = count;
            rc_block_scan<1>(&inc, &carry, part);
            if (l < L) {
                const sp_i32x4 rec = *reinterpret_cast<const sp_i32x4 *>(p.loops + ((size_t)n * p.lcap + l) * 4);
                *reinterpret_cast<sp_i32x4 *>(p.loops_out + ((size_t)n * p.lcap + l) * 4) = sp_i32x4{rec.x, (int)(inc - count), (int)count, rec.w};
            }
        }
        if (threadIdx.x == 0) { p.counts_out[2 * (size_t)n] = L; p.counts_out[2 * (size_t)n + 1] = (int)carry; }
    }
}

__global__ __launch_bounds__(64 * SP_WAVES) void simplify_emit_kernel(const SpP p) {
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    for (int n = blockIdx.y; n < p.N; n += gridDim.y) {
        int L, V;
        if (!sp_frame(p, n, L, V)) continue;
        unsigned *out = p.verts_out + (size_t)n * p.vcap_out;
        for (int l = blockIdx.x * SP_WAVES + wave; l < L; l += gridDim.x * SP_WAVES) {
            int first, cnt;
            sp_loop(p, n, l, V, first, cnt);
            const unsigned *P = p.verts + (size_t)n * p.vcap + first;
            const unsigned char *F = p.flags + (size_t)n * p.fstride + first;
            const bool whole = p.kept[(size_t)n * p.lcap + l] == cnt;
            long long at = (long long)(unsigned)p.loops_out[((size_t)n * p.lcap + l) * 4 + 1];
            for (int base = 0; base < cnt; base += 64) {
                const int i = base + lane;
                const bool keep = i < cnt && (whole || F[min(i, cnt - 1)] != 0);
                const unsigned long long m = __builtin_amdgcn_ballot_w64(keep);
                const long long to = at + __builtin_popcountll(m & ((1ull << lane) - 1ull));
                if (keep && to < p.vcap_out) out[to] = P[i];
                at += __builtin_popcountll(m);
            }
        }
    }
}

long long sp_flag_stride(int64_t vcap) { return (long long)((vcap + 3) & ~(int64_t)3); }

}  // namespace

// per frame: a kept count per loop slot and a keep flag (a byte) per vertex slot, rounded up to 16 bytes in all; a size that does not fit
// size_t comes back as its largest value, which no workspace has
extern "C" size_t arseg_contours_simplify_workspace_bytes(int N, int64_t lcap, int64_t vcap) {
    if (N <= 0 || lcap < 0 || vcap < 0) return 0;
    const size_t none = ~(size_t)0;
    if (lcap > INT64_MAX / 8 || vcap > INT64_MAX / 2) return none;
    size_t frame = 4 * (size_t)lcap, bytes;
    if (__builtin_add_overflow(frame, (size_t)sp_flag_stride(vcap), &frame) || __builtin_mul_overflow(frame, (size_t)N, &bytes) || bytes > none - 15)
        return none;
    return (bytes + 15) & ~(size_t)15;
}

extern "C" int arseg_contours_simplify_fwd(const int32_t *counts, const int32_t *loops, int64_t lcap, const uint32_t *verts, int64_t vcap, int N,
                                           int H, int W, int64_t tol2_q, int32_t *counts_out, int32_t *loops_out, uint32_t *verts_out,
                                           int64_t vcap_out, void *workspace, size_t workspace_bytes, arseg_stream_t stream) {
    ARSEG_CHECK_PTR(counts); ARSEG_CHECK_PTR(counts_out);
    ARSEG_CHECK_POS(N); ARSEG_CHECK_POS(H); ARSEG_CHECK_POS(W);
    if (lcap < 0 || vcap < 0 || vcap_out < 0 || ((loops == nullptr || loops_out == nullptr) && lcap > 0) || (verts == nullptr && vcap > 0) ||
        (verts_out == nullptr && vcap_out > 0))
        return ARSEG_EINVAL;
    if (H > 16384 || W > 16384 || tol2_q < 0 || tol2_q > ((int64_t)1 << 30)) return ARSEG_EINVAL;
    if (rc_misaligned(4, counts, loops, verts, counts_out, loops_out, verts_out, workspace)) return ARSEG_EINVAL;
    if ((verts != nullptr && verts_out == verts) || (loops != nullptr && loops_out == loops) || counts_out == counts) return ARSEG_EINVAL;
    const size_t need = arseg_contours_simplify_workspace_bytes(N, lcap, vcap);
    if (need == ~(size_t)0 || workspace_bytes < need) return ARSEG_EWORKSPACE;
    ARSEG_CHECK_PTR(workspace);
    SpP p = {};
    p.counts = counts; p.loops = loops; p.verts = verts;
    p.counts_out = counts_out; p.loops_out = loops_out; p.verts_out = vcap_out ? verts_out : nullptr;
    p.lcap = lcap; p.vcap = vcap; p.vcap_out = p.verts_out ? vcap_out : 0; p.fstride = sp_flag_stride(vcap);
    p.kept = static_cast<int *>(workspace);
    p.flags = reinterpret_cast<unsigned char *>(p.kept + (size_t)N * (size_t)lcap);
    p.tol = (unsigned long long)tol2_q; p.N = N;
    hipStream_t st = arseg_stream(stream);
    const dim3 per_loop = rc_grid(N, lcap, SP_WAVES, 4096);
    hipLaunchKernelGGL(simplify_clear_kernel, rc_grid(N, p.fstride / 4, 256, 4096), dim3(256), 0, st, p);
    hipLaunchKernelGGL(simplify_keep_kernel, per_loop, dim3(64 * SP_WAVES), 0, st, p);
    hipLaunchKernelGGL(simplify_scan_kernel, rc_frames(N), dim3(256), 0, st, p);
    if (p.vcap_out > 0) hipLaunchKernelGGL(simplify_emit_kernel, per_loop, dim3(64 * SP_WAVES), 0, st, p);          // not in a sizing pass
    return arseg_launch_status();
}
