// Block motion estimation for streams that come without motion vectors (contract: include/arseg_hip.h, arseg_block_motion_*): full search
// of every B x B block of the current frame's luma in the previous frame's, written as the 16-byte records arseg_mv_records_step_fwd takes.
// All of it is 8-bit integer arithmetic.  One launch:
//   tile    : a workgroup of 4 waves owns 64 x 32 pixels = 8 blocks of 16 or 32 blocks of 8.  It stages the tile of the current frame and the
//             window of the reference frame -- the tile and R pixels on every side (the left edge moved out to a multiple of 4, so that window
//             dwords are frame-column dwords) -- into LDS as luma8 bytes, converting the source format on the way in; bytes outside the
//             frame are 0 and are never part of a candidate that counts
//   search  : a wave owns a block, a lane a group of four horizontally adjacent candidates (dy, dx0 .. dx0 + 3), dx0 a multiple of 4 in
//             window columns; neighbouring lanes take neighbouring dy.  The block's own dwords are wave uniform and sit in registers; per
//             block row and block dword the lane reads the two window dwords under it as one pair and one v_qsad_pk_u16_u8 scores the
//             four candidates (the byte shifts 0 .. 3 of a 64-bit window against one dword, four 16-bit accumulators: a 16 x 16 SAD is
//             at most 65 280).  A v_sad_u8 form needs a v_alignbyte_b32 per dword and four times the instructions per candidate; it
//             measured 1.4 - 1.6 times slower
//   winner  : key = cost << 13 | rank per candidate (all ones where the frame border cuts the candidate off), minimum per lane, then across
//             the wave; lane 0 decodes the rank, applies the intra bound and stores the record with one 16-byte vector store
//   edge    : a block clipped by the right or bottom frame edge (w < B or h < B) takes a per-pixel walk, a lane per candidate
//   stats   : one LDS partial per counter and workgroup, one 64-bit atomic per non-zero counter
// The record, the statistics and the argument checks are block_motion_wave.h's, shared with the refinement and the anchor.
#include "block_motion_wave.h"

constexpr int BM_TW = 64, BM_TH = 32;                                  // tile in pixels
constexpr int BM_WIN_W = BM_TW + 2 * BM_MAX_R + 4, BM_WIN_H = BM_TH + 2 * BM_MAX_R;      // window at R = 32: 132 x 96 bytes

constexpr int BM_WPITCH = BM_WIN_W / 4;                                // window row pitch in dwords (33: odd), the same for every R: row offsets are immediates

struct BmSearch {
    int H, W, R, rpad, lam;
    int wused;                  // window dwords per row that are staged and read: (BM_TW + 2 rpad + 4) / 4 <= BM_WPITCH
};

__device__ __forceinline__ unsigned bm_key(const BmSearch &s, unsigned sad, int dx, int dy, bool valid) {
    const int side = 2 * s.R + 1;
    const unsigned cost = sad + (unsigned)(s.lam * (abs(dx) + abs(dy)));
    const unsigned rank = (dx | dy) == 0 ? 0u : (unsigned)(1 + (dy + s.R) * side + dx + s.R);
    return valid ? (cost << 13) | rank : 0xffffffffu;
}

typedef unsigned long long bm_u64_a4 __attribute__((aligned(4)));

// a whole B x B block at tile offset (bxp, byp), frame position (x0, y0): this lane's smallest key
template <int B>
__device__ __forceinline__ unsigned bm_search_full(const BmSearch &s, const unsigned *cur_t, const unsigned *win, int bxp, int byp, int x0, int y0, int lane) {
    constexpr int CD = B / 4;
    unsigned cur[B * CD];                                             // wave uniform
#pragma unroll
    for (int r = 0; r < B; ++r)
#pragma unroll
        for (int c = 0; c < CD; ++c) cur[r * CD + c] = cur_t[(byp + r) * (BM_TW / 4) + (bxp >> 2) + c];
    const int side = 2 * s.R + 1, groups = s.rpad / 2 + 1, total = side * groups;
    // the candidates the frame border leaves this block: dx in [dx_lo, dx_hi], dy in [dy_lo, dy_hi] (wave uniform)
    const int dx_lo = max(-s.R, -x0), dx_hi = min(s.R, s.W - B - x0), dy_lo = max(-s.R, -y0), dy_hi = min(s.R, s.H - B - y0);
    unsigned best = 0xffffffffu;
    for (int q = lane; q < total; q += 64) {
        // Neighbouring lanes go DOWN the window: lane addresses are BM_WPITCH = 33 dwords apart, bank (dyi + g) mod 32, so 32 lanes hit 32
        // banks (and where a group of lanes wraps from the last dy to the next g, side = 1 mod 32 at R = 16 and 32 keeps them apart).
        // Across the window -- g fastest -- the lanes of two rows fall on the same banks.
        const int g = q / side, dyi = q - g * side;
        // window byte (bxp + c + 4 g + shift, byp + r + dyi) = frame pixel (x0 + c + dx, y0 + r + dy), dx = 4 g - rpad + shift, dy = dyi - R
        const unsigned *p = win + (byp + dyi) * BM_WPITCH + (bxp >> 2) + g;
        unsigned long long acc = 0;
        // Dwords c, c + 1 as ONE 8-byte load (ds_read2_b32 into an aligned register pair): the pairs of neighbouring c overlap, and pairs put
        // together from single dwords cost a v_mov per dword.  16 loads are issued, then their 16 v_qsad: left to itself the scheduler
        // keeps one pair live and waits for every load in turn.
        constexpr int RB = 16 / CD;                                   // rows per batch
#pragma unroll
        for (int r0 = 0; r0 < B; r0 += RB) {
            unsigned long long wnd[16];
#pragma unroll
            for (int i = 0; i < 16; ++i) wnd[i] = *reinterpret_cast<const bm_u64_a4 *>(p + (r0 + i / CD) * BM_WPITCH + i % CD);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int i = 0; i < 16; ++i) acc = __builtin_amdgcn_qsad_pk_u16_u8(wnd[i], cur[(r0 + i / CD) * CD + i % CD], acc);
            __builtin_amdgcn_sched_barrier(0);
        }
        // key = (SAD << 13) + ((lambda (|dx| + |dy|)) << 13 | rank): rank < 2^13, so the second term is a sum too, and it is linear in k over
        // the group -- dx0 is a multiple of 4, so dx0 .. dx0 + 3 do not change sign and |dx0 + k| = |dx0| +- k.  Only (0, 0) breaks the line
        // (rank 0), at k = 0 of one group.
        const int dy = dyi - s.R, dx0 = 4 * g - s.rpad;
        const unsigned base0 = ((unsigned)(s.lam * (abs(dx0) + abs(dy))) << 13) + (unsigned)(1 + dyi * side + s.R + dx0);
        const unsigned step = (unsigned)((dx0 >= 0 ? s.lam : -s.lam) * 8192 + 1);
        // dx0 + k in [dx_lo, dx_hi] as one unsigned compare; a dy the border cuts off moves the whole group out of the range
        const unsigned t0 = dy >= dy_lo && dy <= dy_hi ? (unsigned)(dx0 - dx_lo) : 0x80000000u, span = (unsigned)(dx_hi - dx_lo);
        const unsigned lo = (unsigned)acc, hi = (unsigned)(acc >> 32);
        const unsigned k0 = ((lo & 0xffffu) << 13) + ((dx0 | dy) == 0 ? base0 & ~0x1fffu : base0);
        const unsigned k1 = ((lo >> 16) << 13) + base0 + step, k2 = ((hi & 0xffffu) << 13) + base0 + 2 * step, k3 = ((hi >> 16) << 13) + base0 + 3 * step;
        best = min(best, min(t0 <= span ? k0 : 0xffffffffu, t0 + 1 <= span ? k1 : 0xffffffffu));
        best = min(best, min(t0 + 2 <= span ? k2 : 0xffffffffu, t0 + 3 <= span ? k3 : 0xffffffffu));
    }
    return best;
}

// a block clipped to w x h by the frame edge: a lane per candidate, a byte per step
__device__ __forceinline__ unsigned bm_search_clipped(const BmSearch &s, const uint8_t *cur_t, const uint8_t *win, int bxp, int byp, int x0, int y0, int w, int h,
                                                      int lane) {
    const int side = 2 * s.R + 1, total = side * side, ww = BM_WPITCH * 4;
    unsigned best = 0xffffffffu;
    for (int q = lane; q < total; q += 64) {
        const int dyi = q / side, dx = q - dyi * side - s.R, dy = dyi - s.R;
        if (x0 + dx < 0 || x0 + w + dx > s.W || y0 + dy < 0 || y0 + h + dy > s.H) continue;
        unsigned sad = 0;
        for (int r = 0; r < h; ++r) {
            const uint8_t *a = cur_t + (byp + r) * BM_TW + bxp, *b = win + (byp + r + dyi) * ww + bxp + dx + s.rpad;
            for (int c = 0; c < w; ++c) sad += (unsigned)abs((int)a[c] - (int)b[c]);
        }
        best = min(best, bm_key(s, sad, dx, dy, true));
    }
    return best;
}

template <int F, int B>
__global__ __launch_bounds__(256) void block_motion_kernel(const uint8_t *__restrict__ cur, long long cur_pitch, const uint8_t *__restrict__ ref, long long ref_pitch,
                                                           BmSearch s, int intra, int ref_index, int bx_n, int4 *__restrict__ records, unsigned *__restrict__ sad_out,
                                                           unsigned long long *__restrict__ stats) {
    __shared__ unsigned cur_t[BM_TW * BM_TH / 4];
    __shared__ unsigned win[BM_WIN_W * BM_WIN_H / 4];
    __shared__ unsigned part[ARSEG_BM_NSTATS];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int tx0 = blockIdx.x * BM_TW, ty0 = blockIdx.y * BM_TH;
    for (int i = tid; i < BM_TW * BM_TH / 4; i += 256) {
        const int y = ty0 + i / (BM_TW / 4), x = tx0 + 4 * (i % (BM_TW / 4));
        cur_t[i] = y < s.H ? bm_luma4<F>(cur + (size_t)y * cur_pitch, x, s.W) : 0u;
    }
    const int win_h = BM_TH + 2 * s.R;                                // wused <= BM_WPITCH and win_h <= BM_WIN_H for R <= 32
    for (int i = tid; i < s.wused * win_h; i += 256) {
        const int wy = i / s.wused, wx = i - wy * s.wused, y = ty0 - s.R + wy, x = tx0 - s.rpad + 4 * wx;
        win[wy * BM_WPITCH + wx] = y >= 0 && y < s.H ? bm_luma4<F>(ref + (size_t)y * ref_pitch, x, s.W) : 0u;
    }
    if (tid < ARSEG_BM_NSTATS) part[tid] = 0;
    __syncthreads();
    constexpr int NBX = BM_TW / B, NB = NBX * (BM_TH / B);
    for (int b = wave; b < NB; b += 4) {                               // wave uniform
        const int bi = b / NBX, bj = b - bi * NBX, bxp = bj * B, byp = bi * B, x0 = tx0 + bxp, y0 = ty0 + byp;
        if (x0 >= s.W || y0 >= s.H) continue;
        const int w = min(B, s.W - x0), h = min(B, s.H - y0);
        unsigned key = w == B && h == B ? bm_search_full<B>(s, cur_t, win, bxp, byp, x0, y0, lane)
                                        : bm_search_clipped(s, reinterpret_cast<const uint8_t *>(cur_t), reinterpret_cast<const uint8_t *>(win), bxp, byp, x0, y0, w, h, lane);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) key = min(key, (unsigned)__shfl_xor((int)key, o, 64));
        if (lane == 0) {                                               // (0, 0) is always a candidate: key is a real one
            const int side = 2 * s.R + 1, rank = (int)(key & 0x1fffu);
            int dx = 0, dy = 0;
            if (rank) { dy = (rank - 1) / side - s.R; dx = (rank - 1) % side - s.R; }
            const unsigned sad = (key >> 13) - (unsigned)(s.lam * (abs(dx) + abs(dy)));
            const bool is_intra = sad > (unsigned)(intra * w * h);
            if (is_intra) { dx = 0; dy = 0; }
            const size_t at = (size_t)(y0 / B) * bx_n + x0 / B;
            records[at] = bm_record(x0, y0, w, h, dx, dy, is_intra ? ARSEG_BM_INTRA_REF : ref_index);
            if (sad_out) sad_out[at] = sad;
            if (stats) bm_stats_tally(part, is_intra, dx, dy, sad, w * h);
        }
    }
    if (stats) bm_stats_flush(part, stats, tid);
}

extern "C" size_t arseg_block_motion_workspace_bytes(int H, int W, int B, int R) {
    (void)H; (void)W; (void)B; (void)R;
    return 0;                                                          // the search keeps everything in LDS and registers
}

template <int F, int B>
static void bm_launch(const void *cur, long long cur_pitch, const void *ref, long long ref_pitch, const BmSearch &s, int intra, int ref_index, int16_t *records,
                      uint32_t *sad, int64_t *stats, hipStream_t st) {
    hipLaunchKernelGGL((block_motion_kernel<F, B>), dim3(arseg_cdiv(s.W, BM_TW), arseg_cdiv(s.H, BM_TH)), dim3(256), 0, st, reinterpret_cast<const uint8_t *>(cur),
                       cur_pitch, reinterpret_cast<const uint8_t *>(ref), ref_pitch, s, intra, ref_index, arseg_cdiv(s.W, B), reinterpret_cast<int4 *>(records), sad,
                       reinterpret_cast<unsigned long long *>(stats));
}

extern "C" int arseg_block_motion_fwd(const void *cur, int64_t cur_pitch, const void *ref, int64_t ref_pitch, int src_format, int H, int W, int B, int R, int lambda,
                                      int intra, int ref_index, int16_t *records, uint32_t *sad, int64_t *stats, void *workspace, size_t workspace_bytes,
                                      arseg_stream_t stream) {
    (void)workspace;
    ARSEG_CHECK_PTR(cur); ARSEG_CHECK_PTR(ref); ARSEG_CHECK_PTR(records);
    if (!bm_args_ok(H, W, B, lambda, intra, records, sad, stats) || R < 1 || R > BM_MAX_R || ref_index < 0 || ref_index > 15) return ARSEG_EINVAL;
    const int f = bm_format(src_format);
    if (f < 0) return ARSEG_EINVAL;
    if (!bm_plane_ok(f, cur, cur_pitch, W) || !bm_plane_ok(f, ref, ref_pitch, W)) return ARSEG_EINVAL;
    if (workspace_bytes < arseg_block_motion_workspace_bytes(H, W, B, R)) return ARSEG_EWORKSPACE;
    const int rpad = (R + 3) & ~3;
    const BmSearch s = {H, W, R, rpad, lambda, (BM_TW + 2 * rpad + 4) / 4};
    hipStream_t st = arseg_stream(stream);
#define BM_CASE(F)                                                                                                               \
    case F:                                                                                                                      \
        if (B == 8) bm_launch<F, 8>(cur, cur_pitch, ref, ref_pitch, s, intra, ref_index, records, sad, stats, st);                \
        else bm_launch<F, 16>(cur, cur_pitch, ref, ref_pitch, s, intra, ref_index, records, sad, stats, st);                      \
        break;
    switch (f) {
        BM_CASE(BM_U8) BM_CASE(BM_P010) BM_CASE(BM_I010) BM_CASE(BM_RGB8)
    }
#undef BM_CASE
    return arseg_launch_status();
}
