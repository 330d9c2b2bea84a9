// Hierarchical block motion search (contract: include/arseg_hip.h, arseg_luma_pyramid_* and arseg_block_motion_pyr_*): a luma8 pyramid per
// frame, the full search of block_motion.hip on its top level, and one refinement launch per level below it.  All of it is 8-bit integer
// arithmetic; the records of level 0 are the 16-byte records arseg_mv_records_step_fwd takes.
//   pyramid : a workgroup of 4 waves owns 64 x 32 pixels of the source (sides are multiples of 8 = 2^3, so a tile of every level starts on a
//             dword).  It converts the source to luma8 while staging (bm_luma4), writes level 0 as dwords, and reduces in LDS to levels
//             1 .. L (32 x 16, 16 x 8, 8 x 4 bytes), each written as dwords.  The 2 x 2 box reads its source with the row and column clamped to
//             the level's last: the replication for odd sizes happens in the tile that owns that row or column, and in no other
//   refine  : the wave-per-block search of block_motion_wave.h (windows, SAD, clipped blocks).  The wave reads the records of the parent and of
//             the two neighbour parents on its side (wave uniform): four centres with zero, a window each.  The same candidate from two
//             centres gives the same key twice: the minimum counts it once
//   winner  : key = cost << 20 | rank (64 bits), minimum over the wave on the VALU; the record is one 16-byte vector store.  Level 0 applies
//             the intra bound and writes sad and stats as block_motion.hip does
#include "block_motion_wave.h"

constexpr int PYR_MAX_LEVELS = 3, PYR_MAX_REFINE = BMW_MAX_REFINE;
constexpr int PYR_TW = 64, PYR_TH = 32;                                // tile of the source in pixels

struct PyrGeom {
    int H[PYR_MAX_LEVELS + 1], W[PYR_MAX_LEVELS + 1], pitch[PYR_MAX_LEVELS + 1];
    size_t off[PYR_MAX_LEVELS + 2];                                    // off[levels + 1] = the total
};

static PyrGeom pyr_geom(int H, int W, int levels) {
    PyrGeom g = {};
    for (int l = 0; l <= levels; ++l) {
        g.H[l] = l ? (g.H[l - 1] + 1) >> 1 : H;
        g.W[l] = l ? (g.W[l - 1] + 1) >> 1 : W;
        g.pitch[l] = (g.W[l] + 15) & ~15;
        g.off[l + 1] = g.off[l] + (size_t)g.pitch[l] * g.H[l];
    }
    return g;
}

static bool pyr_shape_ok(int H, int W, int levels) { return H >= 1 && W >= 1 && H <= BM_MAX_DIM && W <= BM_MAX_DIM && levels >= 1 && levels <= PYR_MAX_LEVELS; }

// One level from the one above it, both tiles in LDS: the TW x TH bytes of level l + 1 at (tx, ty) from the 2 TW x 2 TH bytes of level l, of
// which hs rows and ws columns exist (both >= 1 wherever an output exists; larger than the tile away from the edge).
template <int TW, int TH>
__device__ __forceinline__ void pyr_reduce(const uint8_t *src, int hs, int ws, unsigned *dst, uint8_t *out, int pitch, int Hd, int Wd, int tx, int ty, int tid) {
    constexpr int SP = 2 * TW;                                         // source row pitch in bytes
    for (int i = tid; i < TW * TH / 4; i += 256) {
        const int y = i / (TW / 4), x = 4 * (i % (TW / 4));
        unsigned v = 0;
        if (ty + y < Hd && tx + x < Wd) {
            const uint8_t *r0 = src + min(2 * y, hs - 1) * SP, *r1 = src + min(2 * y + 1, hs - 1) * SP;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int c0 = min(2 * (x + k), ws - 1), c1 = min(2 * (x + k) + 1, ws - 1);
                v |= (((unsigned)r0[c0] + r0[c1] + r1[c0] + r1[c1] + 2u) >> 2) << (8 * k);
            }
            *reinterpret_cast<unsigned *>(out + (size_t)(ty + y) * pitch + tx + x) = v;      // tx + x + 3 < pitch: a multiple of 16 above Wd
        }
        dst[i] = v;
    }
}

template <int F>
__global__ __launch_bounds__(256) void luma_pyramid_kernel(const uint8_t *__restrict__ plane, long long pitch, PyrGeom g, int levels, uint8_t *__restrict__ pyr) {
    __shared__ unsigned t0[PYR_TW * PYR_TH / 4], t1[PYR_TW * PYR_TH / 16], t2[PYR_TW * PYR_TH / 64], t3[PYR_TW * PYR_TH / 256];
    const int tid = threadIdx.x, tx0 = blockIdx.x * PYR_TW, ty0 = blockIdx.y * PYR_TH;
    for (int i = tid; i < PYR_TW * PYR_TH / 4; i += 256) {
        const int y = ty0 + i / (PYR_TW / 4), x = tx0 + 4 * (i % (PYR_TW / 4));
        unsigned v = 0;
        if (y < g.H[0] && x < g.W[0]) {
            v = bm_luma4<F>(plane + (size_t)y * pitch, x, g.W[0]);
            *reinterpret_cast<unsigned *>(pyr + (size_t)y * g.pitch[0] + x) = v;
        }
        t0[i] = v;
    }
    __syncthreads();
    pyr_reduce<PYR_TW / 2, PYR_TH / 2>(reinterpret_cast<const uint8_t *>(t0), g.H[0] - ty0, g.W[0] - tx0, t1, pyr + g.off[1], g.pitch[1], g.H[1], g.W[1], tx0 >> 1,
                                       ty0 >> 1, tid);
    if (levels < 2) return;                                            // uniform
    __syncthreads();
    pyr_reduce<PYR_TW / 4, PYR_TH / 4>(reinterpret_cast<const uint8_t *>(t1), g.H[1] - (ty0 >> 1), g.W[1] - (tx0 >> 1), t2, pyr + g.off[2], g.pitch[2], g.H[2],
                                       g.W[2], tx0 >> 2, ty0 >> 2, tid);
    if (levels < 3) return;
    __syncthreads();
    pyr_reduce<PYR_TW / 8, PYR_TH / 8>(reinterpret_cast<const uint8_t *>(t2), g.H[2] - (ty0 >> 2), g.W[2] - (tx0 >> 2), t3, pyr + g.off[3], g.pitch[3], g.H[3],
                                       g.W[3], tx0 >> 3, ty0 >> 3, tid);
}

extern "C" size_t arseg_luma_pyramid_bytes(int H, int W, int levels) { return pyr_shape_ok(H, W, levels) ? pyr_geom(H, W, levels).off[levels + 1] : 0; }

extern "C" int arseg_luma_pyramid_fwd(const void *plane, int64_t pitch, int src_format, int H, int W, int levels, uint8_t *pyramid, size_t pyramid_bytes,
                                      arseg_stream_t stream) {
    ARSEG_CHECK_PTR(plane); ARSEG_CHECK_PTR(pyramid);
    if (!pyr_shape_ok(H, W, levels)) return ARSEG_EINVAL;
    const int f = bm_format(src_format);
    if (f < 0 || !bm_plane_ok(f, plane, pitch, W) || !ARSEG_ALIGNED16(pyramid)) return ARSEG_EINVAL;
    const PyrGeom g = pyr_geom(H, W, levels);
    if (pyramid_bytes < g.off[levels + 1]) return ARSEG_EINVAL;
    hipStream_t st = arseg_stream(stream);
    const dim3 grid(arseg_cdiv(W, PYR_TW), arseg_cdiv(H, PYR_TH));
#define PYR_CASE(F)                                                                                                                      \
    case F: hipLaunchKernelGGL((luma_pyramid_kernel<F>), grid, dim3(256), 0, st, reinterpret_cast<const uint8_t *>(plane), pitch, g, levels, pyramid); break;
    switch (f) {
        PYR_CASE(BM_U8) PYR_CASE(BM_P010) PYR_CASE(BM_I010) PYR_CASE(BM_RGB8)
    }
#undef PYR_CASE
    return arseg_launch_status();
}

// ---------------------------------------------------------------------------------------------- refinement
struct PyrRefine {
    int H, W, pitch;            // the level searched
    int bx, n_blocks;           // its block grid
    int pbx, pby;               // the grid of the level above: the parents
    int lam;
    int final_level, intra, ref_index;
};

// B: the block; RF: r, a template argument so that every division of the lane index is by a constant and the loops have constant trip counts.
// The wave-per-block search is block_motion_wave.h's; this kernel's own are its four centres, the cost lam (|dx| + |dy|) and the key's rank
// (DESIGN.md section 6.21).  Every wave has four windows, each with rows for PYR_MAX_REFINE.
template <int B, int RF>
__global__ __launch_bounds__(64 * BMW_WAVES) void block_motion_refine_kernel(const uint8_t *__restrict__ cur, const uint8_t *__restrict__ ref, PyrRefine s,
                                                                             const int4 *__restrict__ parents, int4 *__restrict__ records,
                                                                             unsigned *__restrict__ sad_out, unsigned long long *__restrict__ stats) {
    constexpr int SLOT = (B + 2 * PYR_MAX_REFINE) * BMW_WD<B>;         // dwords of one window
    constexpr int r = RF, n = 2 * r + 1, n2 = n * n;
    __shared__ unsigned win_all[BMW_WAVES][4 * SLOT];
    __shared__ unsigned part[ARSEG_BM_NSTATS];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    unsigned *win = win_all[wave];
    if (tid < ARSEG_BM_NSTATS) part[tid] = 0;
    __syncthreads();
    for (int b = blockIdx.x * BMW_WAVES + wave; b < s.n_blocks; b += gridDim.x * BMW_WAVES) {          // wave uniform
        const int bi = b / s.bx, bj = b - bi * s.bx, x0 = bj * B, y0 = bi * B;
        const int w = min(B, s.W - x0), h = min(B, s.H - y0);
        // the four centres: zero, twice the parent's vector, twice the vectors of the parent's neighbours on this block's side
        const int pi = bi >> 1, pj = bj >> 1, nj = pj + ((bj & 1) ? 1 : -1), ni = pi + ((bi & 1) ? 1 : -1);
        const bool ok2 = nj >= 0 && nj < s.pbx, ok3 = ni >= 0 && ni < s.pby;
        const int v1 = parents[(size_t)pi * s.pbx + pj].z, v2 = parents[(size_t)pi * s.pbx + (ok2 ? nj : pj)].z, v3 = parents[(size_t)(ok3 ? ni : pi) * s.pbx + pj].z;
        const int cx1 = (short)(v1 & 0xffff) / 2, cy1 = (v1 >> 16) / 2;     // fields 4 and 5 are 4 v: twice the vector is half the field
        const int cx2 = (short)(v2 & 0xffff) / 2, cy2 = (v2 >> 16) / 2;
        const int cx3 = (short)(v3 & 0xffff) / 2, cy3 = (v3 >> 16) / 2;
        // The window of a neighbour that is not in the grid is not staged: no candidate reads it
        auto stage = [&](int k, int cx, int cy) { bmw_stage<B, r>(win + k * SLOT, ref, s.pitch, s.H, s.W, x0 + cx - r, y0 + cy - r, lane); };
        stage(0, 0, 0);
        stage(1, cx1, cy1);
        if (ok2) stage(2, cx2, cy2);
        if (ok3) stage(3, cx3, cy3);
        unsigned cmask[B / 4];
        const unsigned mine = bmw_load_block<B>(cur, s.pitch, s.H, s.W, x0, y0, lane, cmask);
        bmw_wave_sync();
        unsigned long long best = BMW_NO_KEY;
#pragma unroll 1
        for (int q0 = 0; q0 < 4 * n2; q0 += 64) {                       // wave uniform: the lane reads below are reached by the whole wave
            const int q = min(q0 + lane, 4 * n2 - 1), k = q / n2, t = q - k * n2, oyi = t / n, oxi = t - oyi * n;
            const int cx = k == 0 ? 0 : (k == 1 ? cx1 : (k == 2 ? cx2 : cx3)), cy = k == 0 ? 0 : (k == 1 ? cy1 : (k == 2 ? cy2 : cy3));
            const bool okc = k == 2 ? ok2 : (k == 3 ? ok3 : true);
            const int dx = cx + oxi - r, dy = cy + oyi - r;
            const bool valid = okc && q0 + lane < 4 * n2 && x0 + dx >= 0 && x0 + w + dx <= s.W && y0 + dy >= 0 && y0 + h + dy <= s.H;
            const unsigned sad = bmw_sad<B>(win + k * SLOT, oyi, ((x0 + cx - r) & 3) + oxi, h, cmask, mine);
            const unsigned cost = sad + (unsigned)(s.lam * (abs(dx) + abs(dy)));
            const unsigned rank = (dx | dy) == 0 ? 0u : (unsigned)(1 + (dy + 511) * 1023 + (dx + 511));
            const unsigned long long key = valid ? ((unsigned long long)cost << 20) | rank : BMW_NO_KEY;
            best = key < best ? key : best;
        }
        const unsigned long long key = bmw_wave_min(best);              // (0, 0) is always a candidate: a real key
        if (lane == 0) {
            const int rank = (int)(key & 0xfffffu);
            int dx = 0, dy = 0;
            if (rank) { dy = (rank - 1) / 1023 - 511; dx = (rank - 1) % 1023 - 511; }
            const unsigned sad = (unsigned)(key >> 20) - (unsigned)(s.lam * (abs(dx) + abs(dy)));
            const bool is_intra = s.final_level && sad > (unsigned)(s.intra * w * h);
            if (is_intra) { dx = 0; dy = 0; }
            records[b] = bm_record(x0, y0, w, h, dx, dy, is_intra ? ARSEG_BM_INTRA_REF : s.ref_index);
            if (sad_out) sad_out[b] = sad;
            if (stats) bm_stats_tally(part, is_intra, dx, dy, sad, w * h);
        }
        bmw_wave_sync();                                               // the next block's windows go where this one's were read
    }
    if (stats) bm_stats_flush(part, stats, tid);
}

static int pyr_blocks(const PyrGeom &g, int l, int B) { return arseg_cdiv(g.H[l], B) * arseg_cdiv(g.W[l], B); }

extern "C" size_t arseg_block_motion_pyr_workspace_bytes(int H, int W, int B, int levels) {
    if (!pyr_shape_ok(H, W, levels) || (B != 8 && B != 16)) return 0;
    const PyrGeom g = pyr_geom(H, W, levels);
    size_t n = 0;
    for (int l = 1; l <= levels; ++l) n += (size_t)pyr_blocks(g, l, B);
    return 16 * n;
}

extern "C" int arseg_block_motion_pyr_fwd(const uint8_t *cur_pyr, const uint8_t *ref_pyr, int H, int W, int levels, int B, int Rt, int r, int lambda, int intra,
                                          int ref_index, int16_t *records, uint32_t *sad, int64_t *stats, void *workspace, size_t workspace_bytes,
                                          arseg_stream_t stream) {
    ARSEG_CHECK_PTR(cur_pyr); ARSEG_CHECK_PTR(ref_pyr); ARSEG_CHECK_PTR(records); ARSEG_CHECK_PTR(workspace);
    if (!pyr_shape_ok(H, W, levels) || !bm_args_ok(H, W, B, lambda, intra, records, sad, stats)) return ARSEG_EINVAL;
    if (Rt < 1 || Rt > BM_MAX_R || r < 1 || r > PYR_MAX_REFINE || ref_index < 0 || ref_index > 15) return ARSEG_EINVAL;
    if (!ARSEG_ALIGNED16(cur_pyr) || !ARSEG_ALIGNED16(ref_pyr) || !ARSEG_ALIGNED16(workspace)) return ARSEG_EINVAL;
    if (workspace_bytes < arseg_block_motion_pyr_workspace_bytes(H, W, B, levels)) return ARSEG_EWORKSPACE;
    const PyrGeom g = pyr_geom(H, W, levels);
    int4 *lvl[PYR_MAX_LEVELS + 1] = {reinterpret_cast<int4 *>(records), reinterpret_cast<int4 *>(workspace)};      // the records of level l
    for (int l = 2; l <= levels; ++l) lvl[l] = lvl[l - 1] + pyr_blocks(g, l - 1, B);
    // top level: the full search on P_L, no intra test (255 never fires)
    int status = arseg_block_motion_fwd(cur_pyr + g.off[levels], g.pitch[levels], ref_pyr + g.off[levels], g.pitch[levels], ARSEG_SRC_NV12, g.H[levels],
                                        g.W[levels], B, Rt, lambda, 255, 0, reinterpret_cast<int16_t *>(lvl[levels]), nullptr, nullptr, nullptr, 0, stream);
    if (status != ARSEG_OK) return status;
    hipStream_t st = arseg_stream(stream);
    for (int l = levels - 1; l >= 0; --l) {
        const PyrRefine s = {g.H[l], g.W[l], g.pitch[l], arseg_cdiv(g.W[l], B), pyr_blocks(g, l, B), arseg_cdiv(g.W[l + 1], B), arseg_cdiv(g.H[l + 1], B),
                             lambda, l == 0, intra, l == 0 ? ref_index : 0};
        uint32_t *sad_l = l == 0 ? sad : nullptr;
        unsigned long long *stats_l = l == 0 ? reinterpret_cast<unsigned long long *>(stats) : nullptr;
        bmw_dispatch(B, r, [&](auto bb, auto rr) {
            hipLaunchKernelGGL((block_motion_refine_kernel<bb(), rr()>), dim3(bmw_grid(s.n_blocks)), dim3(64 * BMW_WAVES), 0, st, cur_pyr + g.off[l], ref_pyr + g.off[l], s,
                               lvl[l + 1], lvl[l], sad_l, stats_l);
        });
    }
    return arseg_launch_status();
}
