// The wave-per-block SAD search that the pyramid refinement (block_motion_pyr.hip) and the keyframe anchor (block_motion_anchor.hip) share,
// and the record and statistics pieces that the full search (block_motion.hip) writes too.  8-bit integer arithmetic, bit exact.
//   wave    : a wave per block, BMW_WAVES waves per workgroup that meet only for the statistics words, the grid capped at two workgroups per
//             compute unit and walked with its stride (bmw_grid: the 64-bit atomics of all workgroups land on one cache line)
//   windows : per centre the (B + 2 r)-row window of the reference plane in the wave's own LDS (bmw_stage), from the plane dword at or below
//             the window's left edge, so that window dwords are plane dwords; what lies outside the plane is 0 and is never part of a
//             candidate that counts.  A wave publishes its windows to itself with bmw_wave_sync, not s_barrier.  How many windows a wave has
//             and how far apart they lie is the kernel's own: it hands every helper the window it means
//   search  : lane i holds dword i of the block (bmw_load_block); a lane owns a candidate (centre, oy, ox): per block row and dword bmw_sad
//             realigns two window dwords (v_alignbyte_b32) against the block's dword, read with v_readlane_b32 into a scalar register, and one
//             v_sad_u8 adds the four differences
//   edge    : a block clipped by the right or bottom edge of its plane (w < B or h < B) takes the same path: its rows beyond h are skipped and
//             the bytes of columns beyond w are masked to 0 in both operands of the SAD
//   winner  : the kernel packs cost and vector into a 64-bit key of its own, BMW_NO_KEY where the border cuts the candidate off; bmw_wave_min
//             is the smallest key of the wave
#pragma once
#include "block_motion_luma.h"

constexpr int BMW_WAVES = 16, BMW_MAX_REFINE = 3;
constexpr unsigned long long BMW_NO_KEY = ~0ull;
// window dwords per row: 3 bytes of alignment, 2 r + B of candidates.  7 (B = 16) or 5 (B = 8) at every r <= 3: odd
template <int B> constexpr int BMW_WD = (B + 2 * BMW_MAX_REFINE + 3 + 3) / 4;

// What a wave wrote to its own part of LDS is visible to its other lanes: the writes have landed, and nothing moves across this point.
__device__ __forceinline__ void bmw_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// The window whose top left candidate is plane pixel (xl, ya) = (x0 + cx - r, y0 + cy - r) into win[(B + 2 r) * WD]: x is a multiple of 4 and
// x + 3 < pitch wherever x < W.
template <int B, int R>
__device__ __forceinline__ void bmw_stage(unsigned *win, const uint8_t *plane, long long pitch, int H, int W, int xl, int ya, int lane) {
    constexpr int WD = BMW_WD<B>, rows = B + 2 * R;
    const int xa = xl & ~3;
#pragma unroll
    for (int i0 = 0; i0 < rows * WD; i0 += 64) {
        const int i = i0 + lane, wy = i / WD, wx = i - wy * WD, y = ya + wy, x = xa + 4 * wx;
        if (i < rows * WD) win[wy * WD + wx] = y >= 0 && y < H && x >= 0 && x < W ? *reinterpret_cast<const unsigned *>(plane + (size_t)y * pitch + x) : 0u;
    }
}

// The block at (x0, y0), w columns of it inside the plane: lane i gets dword i, cmask[c] the bytes of dword column c that count (wave uniform)
template <int B>
__device__ __forceinline__ unsigned bmw_load_block(const uint8_t *cur, long long pitch, int H, int W, int x0, int y0, int lane, unsigned (&cmask)[B / 4]) {
    constexpr int CD = B / 4;
    const int w = min(B, W - x0);
    auto col_mask = [&](int c) { const int rem = w - 4 * c; return rem >= 4 ? 0xffffffffu : (rem <= 0 ? 0u : (1u << (8 * rem)) - 1u); };
#pragma unroll
    for (int c = 0; c < CD; ++c) cmask[c] = col_mask(c);
    unsigned mine = 0;
    if (lane < B * CD) {
        const int y = y0 + lane / CD, x = x0 + 4 * (lane % CD);
        if (y < H && x < W) mine = *reinterpret_cast<const unsigned *>(cur + (size_t)y * pitch + x) & col_mask(lane % CD);
    }
    return mine;
}

// The SAD of the h x w block against the candidate at offset (oxi, oyi) of win, a window staged from xl: sb = (xl & 3) + oxi, 0 .. 2 r + 3, so
// window byte (sb + c, oyi + rr) is the plane pixel under block pixel (c, rr).  The whole wave gets here: mine is read across lanes.
template <int B>
__device__ __forceinline__ unsigned bmw_sad(const unsigned *win, int oyi, int sb, int h, const unsigned (&cmask)[B / 4], unsigned mine) {
    constexpr int CD = B / 4, WD = BMW_WD<B>;
    const unsigned *p = win + oyi * WD + (sb >> 2);
    const unsigned sh = (unsigned)sb & 3u;
    unsigned sad = 0;
#pragma unroll
    for (int rr = 0; rr < B; ++rr) {
        if (rr < h) {                                                   // wave uniform
            unsigned d[CD + 1];
#pragma unroll
            for (int c = 0; c <= CD; ++c) d[c] = p[rr * WD + c];
#pragma unroll
            for (int c = 0; c < CD; ++c)
                sad = __builtin_amdgcn_sad_u8(__builtin_amdgcn_alignbyte(d[c + 1], d[c], sh) & cmask[c], (unsigned)__builtin_amdgcn_readlane((int)mine, rr * CD + c), sad);
        }
    }
    return sad;
}

// the smallest key of the wave, uniform
__device__ __forceinline__ unsigned long long bmw_wave_min(unsigned long long key) { return ~wave_max_u64(~key); }

// ---------------------------------------------------------------------------------------------- what every block search writes
// the 16-byte record arseg_mv_records_step_fwd takes: (x0, y0, w, h, 4 dx, 4 dy, ref, 0) as int16
__device__ __forceinline__ int4 bm_record(int x0, int y0, int w, int h, int dx, int dy, int ref) {
    return make_int4(x0 | (y0 << 16), w | (h << 16), ((4 * dx) & 0xffff) | ((4 * dy) << 16), ref);
}

// one block into the workgroup's partials of the ARSEG_BM_NSTATS counters: intra blocks, zero vectors, SAD and pixels of the matched ones
__device__ __forceinline__ void bm_stats_tally(unsigned *part, bool is_intra, int dx, int dy, unsigned sad, int pixels) {
    if (is_intra) atomicAdd(&part[0], 1u);
    else {
        if ((dx | dy) == 0) atomicAdd(&part[1], 1u);
        atomicAdd(&part[2], sad);
        atomicAdd(&part[3], (unsigned)pixels);
    }
}

// the workgroup's four partials into stats: one 64-bit atomic per non-zero counter.  Reached by the whole workgroup
template <class T>
__device__ __forceinline__ void bm_stats_flush(const T *part, unsigned long long *stats, int tid) {
    static_assert(ARSEG_BM_NSTATS == ARSEG_BMA_NSTATS, "one flush for both rows of counters");
    __syncthreads();
    if (tid < ARSEG_BM_NSTATS && part[tid]) atomicAdd(&stats[tid], (unsigned long long)part[tid]);
}

// ---------------------------------------------------------------------------------------------- host side
// what every block search checks of its arguments
static inline bool bm_args_ok(int H, int W, int B, int lambda, int intra, const void *records, const void *sad, const void *stats) {
    if (H < 1 || W < 1 || H > BM_MAX_DIM || W > BM_MAX_DIM || (B != 8 && B != 16) || lambda < 0 || lambda > 255 || intra < 0 || intra > 255) return false;
    return ARSEG_ALIGNED16(records) && !(reinterpret_cast<uintptr_t>(sad) & 3u) && !(reinterpret_cast<uintptr_t>(stats) & 7u);
}

// a byte plane that bmw_stage and bmw_load_block read in dwords (the keyframe anchor, the chain healing): the base 4-byte aligned, the pitch a
// multiple of 4 and at least (W + 3) & ~3
static inline bool bmw_plane_ok(const void *plane, int64_t pitch, int W) { return !(reinterpret_cast<uintptr_t>(plane) & 3u) && !(pitch & 3) && pitch >= ((W + 3) & ~3); }

// workgroups of BMW_WAVES blocks: two per compute unit fill the device, the rest of the blocks come with the grid's stride
static inline int bmw_grid(int n_blocks) { return min(arseg_cdiv(n_blocks, BMW_WAVES), 2 * arseg_cu_count()); }

// Runtime (B, r) as template arguments: launch(std::integral_constant<int, B>, std::integral_constant<int, r>).  The caller has checked both
template <class F>
static inline void bmw_dispatch(int B, int r, F &&launch) {
#define BMW_CASE(BB, RR) if (B == BB && r == RR) launch(std::integral_constant<int, BB>{}, std::integral_constant<int, RR>{});
    BMW_CASE(8, 1) BMW_CASE(8, 2) BMW_CASE(8, 3) BMW_CASE(16, 1) BMW_CASE(16, 2) BMW_CASE(16, 3)
#undef BMW_CASE
}
