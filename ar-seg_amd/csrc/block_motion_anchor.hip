// Keyframe anchoring of estimated block motion (contract: include/arseg_hip.h, arseg_block_motion_anchor_fwd): every block of frame f is
// matched against the keyframe's luma around the displacement the chain would compose for it, and a block that matches gets a record with
// ref = f - 1, whose target is frame 0.  8-bit integer arithmetic; a sibling of block_motion_refine_kernel (block_motion_pyr.hip), whose
// shape it keeps:
//   wave    : a wave per block, 16 waves per workgroup that meet only for the four statistics words, the grid capped at two workgroups per
//             compute unit and walked with its stride (the 64-bit atomics of all workgroups land on one cache line)
//   centres : wave uniform -- the own record, up to four neighbour records and two to six 4-byte gathers from merged[f - 1]; up to seven,
//             of which only the distinct ones get a window and candidate slots (the union is a set: DESIGN.md section 6.22 has the timings)
//   windows : per centre the (B + 2 r)-row window of the keyframe in LDS, from the frame dword at or below the window's left edge, sized by
//             the template's own r; what lies outside the frame is 0 and is never part of a candidate that counts.  A wave publishes its
//             windows to itself with the fence + wave_barrier pair, not s_barrier
//   search  : lane i holds dword i of the block; a lane owns a candidate (centre, oy, ox): per block row and dword v_alignbyte_b32 of two
//             window dwords against the block's dword (v_readlane_b32), one v_sad_u8.  The same vector from two centres gives the same key
//   winner  : key = cost << 28 | (dy + 8192) << 14 | (dx + 8192), minimum over the wave; lane 0 stores the record with one 16-byte store
//   edge    : a clipped block (w < B or h < B) takes the same path: rows >= h are skipped, columns >= w masked in both operands
#include "block_motion_luma.h"

constexpr int BMA_WAVES = 16, BMA_CENTRES = 7, BMA_MAX_REFINE = 3, BMA_MAX_F = 16;
constexpr unsigned long long BMA_NO_KEY = ~0ull;

struct AnchorArgs {
    int H, W, bx, by, n_blocks;
    long long cur_pitch, key_pitch;
    int lam, intra, f;
};

__device__ __forceinline__ void bma_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

__device__ __forceinline__ int bma_round_half_even_div4(int v) {
    const int b = v >> 2, r = v & 3;
    return b + ((r > 2) || (r == 2 && (b & 1)) ? 1 : 0);
}

template <int B, int RF>
__global__ __launch_bounds__(64 * BMA_WAVES) void block_motion_anchor_kernel(const uint8_t *__restrict__ cur, const uint8_t *__restrict__ key, AnchorArgs s,
                                                                             const int4 *__restrict__ rec_in, const int *__restrict__ merged_prev,
                                                                             int4 *__restrict__ rec_out, unsigned *__restrict__ sad_out,
                                                                             unsigned long long *__restrict__ stats) {
    constexpr int CD = B / 4, r = RF, n = 2 * r + 1, n2 = n * n, ROWS = B + 2 * r;
    constexpr int WD = ((B + 2 * r + 3 + 3) / 4) | 1;                  // window dwords per row: 3 bytes of alignment, 2 r + B of candidates; odd: 7 or 5
    __shared__ unsigned win_all[BMA_WAVES][BMA_CENTRES * ROWS * WD];
    __shared__ int2 cent_all[BMA_WAVES][BMA_CENTRES + 1];             // per wave: its distinct centres
    __shared__ unsigned long long part[ARSEG_BMA_NSTATS];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    unsigned *win = win_all[wave];
    int2 *cent = cent_all[wave];
    if (tid < ARSEG_BMA_NSTATS) part[tid] = 0;
    __syncthreads();
    for (int b = blockIdx.x * BMA_WAVES + wave; b < s.n_blocks; b += gridDim.x * BMA_WAVES) {          // wave uniform
        const int bi = b / s.bx, bj = b - bi * s.bx, x0 = bj * B, y0 = bi * B;
        const int w = min(B, s.W - x0), h = min(B, s.H - y0);
        // the hop and the prediction of block (qi, qj), which is in the grid: wave uniform
        auto pred = [&](int qi, int qj, int &px, int &py) -> bool {
            const int4 q = rec_in[(size_t)qi * s.bx + qj];
            const bool usable = (short)(q.w & 0xffff) == 0;
            const int hx = usable ? bma_round_half_even_div4((short)(q.z & 0xffff)) : 0, hy = usable ? bma_round_half_even_div4(q.z >> 16) : 0;
            const int qx0 = qj * B, qy0 = qi * B, xc = qx0 + min(B, s.W - qx0) / 2, yc = qy0 + min(B, s.H - qy0) / 2;
            const int m = merged_prev[(size_t)min(max(yc + hy, 0), s.H - 1) * s.W + min(max(xc + hx, 0), s.W - 1)];
            px = hx + ((short)(m & 0xffff) >> 2);
            py = hy + ((m >> 16) >> 2);
            return usable;
        };
        int cxs[BMA_CENTRES], cys[BMA_CENTRES];
        bool oks[BMA_CENTRES];
        cxs[0] = 0; cys[0] = 0; oks[0] = true;
        const bool own_usable = pred(bi, bj, cxs[1], cys[1]);
        oks[1] = true;
        {
            const int m = merged_prev[(size_t)(y0 + h / 2) * s.W + x0 + w / 2];
            cxs[2] = (short)(m & 0xffff) >> 2; cys[2] = (m >> 16) >> 2; oks[2] = true;
        }
#pragma unroll
        for (int k = 3; k < BMA_CENTRES; ++k) {
            const int qi = bi + (k == 5 ? -1 : (k == 6 ? 1 : 0)), qj = bj + (k == 3 ? -1 : (k == 4 ? 1 : 0));
            cxs[k] = 0; cys[k] = 0;
            oks[k] = qi >= 0 && qi < s.by && qj >= 0 && qj < s.bx;
            if (oks[k]) oks[k] = pred(qi, qj, cxs[k], cys[k]);
        }
        const int c1x = cxs[1], c1y = cys[1];
        // The distinct centres, in order: a centre equal to an earlier one proposes nothing new (in a static or panned scene most coincide),
        // so it gets no window and no candidate slots.  nc is wave uniform, 1 .. 7; window j and cent[j] belong to the j-th distinct centre.
        // x is a multiple of 4 and x + 3 < pitch wherever x < W.
        int nc = 0;
#pragma unroll
        for (int k = 0; k < BMA_CENTRES; ++k) {
            bool take = oks[k];
#pragma unroll
            for (int j = 0; j < k; ++j) take = take && !(oks[j] && cxs[j] == cxs[k] && cys[j] == cys[k]);
            if (!take) continue;                                       // wave uniform
            if (lane == 0) cent[nc] = make_int2(cxs[k], cys[k]);
            const int ya = y0 + cys[k] - r, xa = (x0 + cxs[k] - r) & ~3;
#pragma unroll
            for (int i0 = 0; i0 < ROWS * WD; i0 += 64) {
                const int i = i0 + lane, wy = i / WD, wx = i - wy * WD, y = ya + wy, x = xa + 4 * wx;
                if (i < ROWS * WD)
                    win[(nc * ROWS + wy) * WD + wx] = y >= 0 && y < s.H && x >= 0 && x < s.W ? *reinterpret_cast<const unsigned *>(key + (size_t)y * s.key_pitch + x) : 0u;
            }
            ++nc;
        }
        const int nq = nc * n2;
        auto col_mask = [&](int c) { const int rem = w - 4 * c; return rem >= 4 ? 0xffffffffu : (rem <= 0 ? 0u : (1u << (8 * rem)) - 1u); };
        unsigned mine = 0;                                             // lane i: dword i of the block
        if (lane < B * CD) {
            const int y = y0 + lane / CD, x = x0 + 4 * (lane % CD);
            if (y < s.H && x < s.W) mine = *reinterpret_cast<const unsigned *>(cur + (size_t)y * s.cur_pitch + x) & col_mask(lane % CD);
        }
        unsigned cmask[CD];                                            // wave uniform
#pragma unroll
        for (int c = 0; c < CD; ++c) cmask[c] = col_mask(c);
        bma_wave_sync();
        unsigned long long best = BMA_NO_KEY;
#pragma unroll 1
        for (int q0 = 0; q0 < nq; q0 += 64) {                           // wave uniform: the lane reads below are reached by the whole wave
            const int q = min(q0 + lane, nq - 1), k = q / n2, t = q - k * n2, oyi = t / n, oxi = t - oyi * n;
            const int2 c = cent[k];
            const int cx = c.x, cy = c.y, dx = cx + oxi - r, dy = cy + oyi - r;
            const bool valid = q0 + lane < nq && x0 + dx >= 0 && x0 + w + dx <= s.W && y0 + dy >= 0 && y0 + h + dy <= s.H;
            // window byte (sb + c, oyi + rr) of centre k = keyframe pixel (x0 + dx + c, y0 + dy + rr)
            const int sb = ((x0 + cx - r) & 3) + oxi;                   // 0 .. 2 r + 3
            unsigned sad = 0;
            const unsigned *p = win + (k * ROWS + oyi) * WD + (sb >> 2);
            const unsigned sh = (unsigned)sb & 3u;
#pragma unroll
            for (int rr = 0; rr < B; ++rr) {
                if (rr < h) {                                           // wave uniform
                    unsigned d[CD + 1];
#pragma unroll
                    for (int c = 0; c <= CD; ++c) d[c] = p[rr * WD + c];
#pragma unroll
                    for (int c = 0; c < CD; ++c)
                        sad = __builtin_amdgcn_sad_u8(__builtin_amdgcn_alignbyte(d[c + 1], d[c], sh) & cmask[c], (unsigned)__builtin_amdgcn_readlane((int)mine, rr * CD + c), sad);
                }
            }
            const unsigned cost = sad + (unsigned)(s.lam * (abs(dx - c1x) + abs(dy - c1y)));
            const unsigned long long kq = valid ? ((unsigned long long)cost << 28) | (unsigned)(((dy + 8192) << 14) | (dx + 8192)) : BMA_NO_KEY;
            best = kq < best ? kq : best;
        }
        const unsigned long long kw = ~wave_max_u64(~best);             // (0, 0) is always a candidate: a real key, uniform
        if (lane == 0) {
            const int rank = (int)(kw & 0xfffffffu), dy = (rank >> 14) - 8192, dx = (rank & 16383) - 8192;
            const int drift = abs(dx - c1x) + abs(dy - c1y);
            const unsigned sad = (unsigned)(kw >> 28) - (unsigned)(s.lam * drift);
            const bool anchored = sad <= (unsigned)(s.intra * w * h);
            rec_out[b] = anchored ? make_int4(x0 | (y0 << 16), w | (h << 16), ((4 * dx) & 0xffff) | ((4 * dy) << 16), s.f - 1) : rec_in[b];
            if (anchored && sad_out) sad_out[b] = sad;
            if (stats) {
                if (anchored) {
                    atomicAdd(&part[0], 1ull);
                    if (!own_usable) atomicAdd(&part[1], 1ull);
                    if (drift) atomicAdd(&part[3], (unsigned long long)drift);
                } else atomicAdd(&part[2], 1ull);
            }
        }
        bma_wave_sync();                                               // the next block's windows go where this one's were read
    }
    if (stats) {
        __syncthreads();
        if (tid < ARSEG_BMA_NSTATS && part[tid]) atomicAdd(&stats[tid], part[tid]);
    }
}

// f == 1: the hop is the anchor
__global__ __launch_bounds__(256) void block_motion_anchor_copy_kernel(const int4 *__restrict__ rec_in, int4 *__restrict__ rec_out, int n) {
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) rec_out[i] = rec_in[i];
}

static bool bma_plane_ok(const void *plane, int64_t pitch, int W) { return !(reinterpret_cast<uintptr_t>(plane) & 3u) && !(pitch & 3) && pitch >= ((W + 3) & ~3); }

extern "C" int arseg_block_motion_anchor_fwd(const uint8_t *cur, int64_t cur_pitch, const uint8_t *key, int64_t key_pitch, int H, int W, int B, int r, int lambda,
                                             int intra, int f, const int16_t *records_in, const int16_t *merged_prev, int16_t *records_out, uint32_t *sad,
                                             int64_t *stats, arseg_stream_t stream) {
    ARSEG_CHECK_PTR(cur); ARSEG_CHECK_PTR(key); ARSEG_CHECK_PTR(records_in); ARSEG_CHECK_PTR(records_out);
    if (H < 1 || W < 1 || H > BM_MAX_DIM || W > BM_MAX_DIM || (B != 8 && B != 16) || r < 1 || r > BMA_MAX_REFINE) return ARSEG_EINVAL;
    if (lambda < 0 || lambda > 255 || intra < 0 || intra > 255 || f < 1 || f > BMA_MAX_F) return ARSEG_EINVAL;
    if (f >= 2 && merged_prev == nullptr) return ARSEG_EINVAL;
    if (!bma_plane_ok(cur, cur_pitch, W) || !bma_plane_ok(key, key_pitch, W)) return ARSEG_EINVAL;
    if (!ARSEG_ALIGNED16(records_in) || !ARSEG_ALIGNED16(records_out)) return ARSEG_EINVAL;
    if ((reinterpret_cast<uintptr_t>(merged_prev) & 3u) || (reinterpret_cast<uintptr_t>(sad) & 3u) || (reinterpret_cast<uintptr_t>(stats) & 7u)) return ARSEG_EINVAL;
    const AnchorArgs s = {H, W, arseg_cdiv(W, B), arseg_cdiv(H, B), arseg_cdiv(W, B) * arseg_cdiv(H, B), cur_pitch, key_pitch, lambda, intra, f};
    const uintptr_t in0 = reinterpret_cast<uintptr_t>(records_in), out0 = reinterpret_cast<uintptr_t>(records_out), bytes = (uintptr_t)16 * s.n_blocks;
    if (in0 < out0 + bytes && out0 < in0 + bytes) return ARSEG_EINVAL;
    hipStream_t st = arseg_stream(stream);
    const int4 *rin = reinterpret_cast<const int4 *>(records_in);
    int4 *rout = reinterpret_cast<int4 *>(records_out);
    if (f == 1) {
        hipLaunchKernelGGL(block_motion_anchor_copy_kernel, dim3(arseg_grid_for(s.n_blocks, 1024)), dim3(256), 0, st, rin, rout, s.n_blocks);
        return arseg_launch_status();
    }
    const dim3 grid(min(arseg_cdiv(s.n_blocks, BMA_WAVES), 2 * arseg_cu_count()));
#define BMA_CASE(BB, RR)                                                                                                                  \
    if (B == BB && r == RR)                                                                                                               \
        hipLaunchKernelGGL((block_motion_anchor_kernel<BB, RR>), grid, dim3(64 * BMA_WAVES), 0, st, cur, key, s, rin, reinterpret_cast<const int *>(merged_prev), rout, \
                           sad, reinterpret_cast<unsigned long long *>(stats));
    BMA_CASE(8, 1) BMA_CASE(8, 2) BMA_CASE(8, 3) BMA_CASE(16, 1) BMA_CASE(16, 2) BMA_CASE(16, 3)
#undef BMA_CASE
    return arseg_launch_status();
}
