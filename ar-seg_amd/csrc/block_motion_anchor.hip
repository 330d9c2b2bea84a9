// Keyframe anchoring of estimated block motion (contract: include/arseg_hip.h, arseg_block_motion_anchor_fwd): every block of frame f is
// matched against the keyframe's luma around the displacement the chain would compose for it, and a block that matches gets a record with
// ref = f - 1, whose target is frame 0.  8-bit integer arithmetic; the wave-per-block search (windows, SAD, clipped blocks) is
// block_motion_wave.h's, shared with block_motion_refine_kernel (block_motion_pyr.hip).  This kernel's own:
//   centres : wave uniform -- the own record, up to four neighbour records and two to six 4-byte gathers from merged[f - 1]; up to seven,
//             of which only the distinct ones get a window and candidate slots (the union is a set: DESIGN.md section 6.22 has the timings).
//             A window has rows for the template's own r
//   winner  : key = cost << 28 | (dy + 8192) << 14 | (dx + 8192), cost = SAD + lam |d - c1|: the same vector from two centres gives the same
//             key.  Minimum over the wave; lane 0 stores the record with one 16-byte store
#include "block_motion_wave.h"

constexpr int BMA_CENTRES = 7, BMA_MAX_F = 16;

struct AnchorArgs {
    int H, W, bx, by, n_blocks;
    long long cur_pitch, key_pitch;
    int lam, intra, f;
};

template <int B, int RF>
__global__ __launch_bounds__(64 * BMW_WAVES) void block_motion_anchor_kernel(const uint8_t *__restrict__ cur, const uint8_t *__restrict__ key, AnchorArgs s,
                                                                             const int4 *__restrict__ rec_in, const int *__restrict__ merged_prev,
                                                                             int4 *__restrict__ rec_out, unsigned *__restrict__ sad_out,
                                                                             unsigned long long *__restrict__ stats) {
    constexpr int r = RF, n = 2 * r + 1, n2 = n * n, SLOT = (B + 2 * r) * BMW_WD<B>;      // dwords of one window
    __shared__ unsigned win_all[BMW_WAVES][BMA_CENTRES * SLOT];
    __shared__ int2 cent_all[BMW_WAVES][BMA_CENTRES + 1];             // per wave: its distinct centres
    __shared__ unsigned long long part[ARSEG_BMA_NSTATS];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    unsigned *win = win_all[wave];
    int2 *cent = cent_all[wave];
    if (tid < ARSEG_BMA_NSTATS) part[tid] = 0;
    __syncthreads();
    for (int b = blockIdx.x * BMW_WAVES + wave; b < s.n_blocks; b += gridDim.x * BMW_WAVES) {          // wave uniform
        const int bi = b / s.bx, bj = b - bi * s.bx, x0 = bj * B, y0 = bi * B;
        const int w = min(B, s.W - x0), h = min(B, s.H - y0);
        // the hop and the prediction of block (qi, qj), which is in the grid: wave uniform
        auto pred = [&](int qi, int qj, int &px, int &py) -> bool {
            const int4 q = rec_in[(size_t)qi * s.bx + qj];
            const bool usable = (short)(q.w & 0xffff) == 0;
            const int hx = usable ? round_half_even_div4((short)(q.z & 0xffff)) : 0, hy = usable ? round_half_even_div4(q.z >> 16) : 0;
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
        int nc = 0;
#pragma unroll
        for (int k = 0; k < BMA_CENTRES; ++k) {
            bool take = oks[k];
#pragma unroll
            for (int j = 0; j < k; ++j) take = take && !(oks[j] && cxs[j] == cxs[k] && cys[j] == cys[k]);
            if (!take) continue;                                       // wave uniform
            if (lane == 0) cent[nc] = make_int2(cxs[k], cys[k]);
            bmw_stage<B, r>(win + nc * SLOT, key, s.key_pitch, s.H, s.W, x0 + cxs[k] - r, y0 + cys[k] - r, lane);
            ++nc;
        }
        const int nq = nc * n2;
        unsigned cmask[B / 4];
        const unsigned mine = bmw_load_block<B>(cur, s.cur_pitch, s.H, s.W, x0, y0, lane, cmask);
        bmw_wave_sync();
        unsigned long long best = BMW_NO_KEY;
#pragma unroll 1
        for (int q0 = 0; q0 < nq; q0 += 64) {                           // wave uniform: the lane reads below are reached by the whole wave
            const int q = min(q0 + lane, nq - 1), k = q / n2, t = q - k * n2, oyi = t / n, oxi = t - oyi * n;
            const int2 c = cent[k];
            const int cx = c.x, cy = c.y, dx = cx + oxi - r, dy = cy + oyi - r;
            const bool valid = q0 + lane < nq && x0 + dx >= 0 && x0 + w + dx <= s.W && y0 + dy >= 0 && y0 + h + dy <= s.H;
            const unsigned sad = bmw_sad<B>(win + k * SLOT, oyi, ((x0 + cx - r) & 3) + oxi, h, cmask, mine);
            const unsigned cost = sad + (unsigned)(s.lam * (abs(dx - c1x) + abs(dy - c1y)));
            const unsigned long long kq = valid ? ((unsigned long long)cost << 28) | (unsigned)(((dy + 8192) << 14) | (dx + 8192)) : BMW_NO_KEY;
            best = kq < best ? kq : best;
        }
        const unsigned long long kw = bmw_wave_min(best);               // (0, 0) is always a candidate: a real key
        if (lane == 0) {
            const int rank = (int)(kw & 0xfffffffu), dy = (rank >> 14) - 8192, dx = (rank & 16383) - 8192;
            const int drift = abs(dx - c1x) + abs(dy - c1y);
            const unsigned sad = (unsigned)(kw >> 28) - (unsigned)(s.lam * drift);
            const bool anchored = sad <= (unsigned)(s.intra * w * h);
            rec_out[b] = anchored ? bm_record(x0, y0, w, h, dx, dy, s.f - 1) : rec_in[b];
            if (anchored && sad_out) sad_out[b] = sad;
            if (stats) {
                if (anchored) {
                    atomicAdd(&part[0], 1ull);
                    if (!own_usable) atomicAdd(&part[1], 1ull);
                    if (drift) atomicAdd(&part[3], (unsigned long long)drift);
                } else atomicAdd(&part[2], 1ull);
            }
        }
        bmw_wave_sync();                                               // the next block's windows go where this one's were read
    }
    if (stats) bm_stats_flush(part, stats, tid);
}

// f == 1: the hop is the anchor
__global__ __launch_bounds__(256) void block_motion_anchor_copy_kernel(const int4 *__restrict__ rec_in, int4 *__restrict__ rec_out, int n) {
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) rec_out[i] = rec_in[i];
}

extern "C" int arseg_block_motion_anchor_fwd(const uint8_t *cur, int64_t cur_pitch, const uint8_t *key, int64_t key_pitch, int H, int W, int B, int r, int lambda,
                                             int intra, int f, const int16_t *records_in, const int16_t *merged_prev, int16_t *records_out, uint32_t *sad,
                                             int64_t *stats, arseg_stream_t stream) {
    ARSEG_CHECK_PTR(cur); ARSEG_CHECK_PTR(key); ARSEG_CHECK_PTR(records_in); ARSEG_CHECK_PTR(records_out);
    if (!bm_args_ok(H, W, B, lambda, intra, records_out, sad, stats) || r < 1 || r > BMW_MAX_REFINE || f < 1 || f > BMA_MAX_F) return ARSEG_EINVAL;
    if (f >= 2 && merged_prev == nullptr) return ARSEG_EINVAL;
    if (!bmw_plane_ok(cur, cur_pitch, W) || !bmw_plane_ok(key, key_pitch, W)) return ARSEG_EINVAL;
    if (!ARSEG_ALIGNED16(records_in) || (reinterpret_cast<uintptr_t>(merged_prev) & 3u)) return ARSEG_EINVAL;
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
    bmw_dispatch(B, r, [&](auto bb, auto rr) {
        hipLaunchKernelGGL((block_motion_anchor_kernel<bb(), rr()>), dim3(bmw_grid(s.n_blocks)), dim3(64 * BMW_WAVES), 0, st, cur, key, s, rin,
                           reinterpret_cast<const int *>(merged_prev), rout, sad, reinterpret_cast<unsigned long long *>(stats));
    });
    return arseg_launch_status();
}
