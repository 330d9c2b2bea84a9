// Healing of the flagged pixels of a motion chain on the keyframe (contract: include/arseg_hip.h, arseg_mv_chain_heal_fwd): the blocks of a
// fixed grid that hold intra / uncovered / clamped pixels of merged[f] are matched against the keyframe's luma around what the chain and the
// unflagged surroundings say, and where the flagged pixels match they get a one-hop vector to frame 0 and a clean link byte.  It works on the
// chain's output, so it does not matter who made the records.  8-bit integer arithmetic; the wave-per-block search (windows, SAD, clipped
// blocks) is block_motion_wave.h's, as in block_motion_anchor.hip.  Two launches:
//   decide  : a wave per block.  Lane i reads the four link bytes under dword i of the block and the wave counts the flagged ones with four
//             ballots; a block below min_flagged writes its record and leaves -- one byte per pixel read, nothing staged.  An examined block
//             gathers up to seven centres (wave uniform), searches the distinct ones like the anchor, and evaluates the winner once more
//             with each lane's flag bytes ANDed into both operands of its own v_sad_u8: SAD_flagged.  Writes decisions, sad and stats only,
//             so that no block reads what another one has healed
//   apply   : a thread per 4 pixels of a row reads its block's record; where the block is healed it rewrites the flagged pixels and tallies
//             the correction of the chain's link counters (signed LDS partials, one 64-bit two's-complement atomic per non-zero counter
//             and workgroup; the grid is capped at two workgroups per compute unit and walked with its stride, because those atomics
//             all land on one cache line: uncapped, 1024 x 2048 with 5 % of its blocks healed took 16 us longer)
#include "block_motion_wave.h"

constexpr int HL_CENTRES = 7;

struct HealArgs {
    int H, W, bx, by, n_blocks;
    long long cur_pitch, key_pitch;
    int lam, intra, flag_mask, min_flagged;
};

// link bytes x .. x + 3 of one row, packed little endian: rows are W bytes apart, so the address has any alignment; a byte at or beyond W
// reads 0 and is not touched
__device__ __forceinline__ unsigned hl_link4(const uint8_t *row, int x, int W) {
    unsigned out = 0;
    if (x + 4 <= W) {
        unsigned v[4];
        span_load<4>(row + x, v);
        out = v[0] | (v[1] << 8) | (v[2] << 16) | (v[3] << 24);
    } else {
#pragma unroll
        for (int i = 0; i < 3; ++i)
            if (x + i < W) out |= (unsigned)row[x + i] << (8 * i);
    }
    return out;
}

// 0xff in every byte of v that has a bit of the flag mask (m4: the mask, 1 .. 7, in all four bytes; 7 + 0x7f does not carry out of a byte)
__device__ __forceinline__ unsigned hl_flagged(unsigned v, unsigned m4) { return ((((v & m4) + 0x7f7f7f7fu) >> 7) & 0x01010101u) * 0xffu; }

// the sum of v over the wave, uniform
__device__ __forceinline__ unsigned hl_wave_sum(unsigned v) {
#pragma unroll
    for (int o = 32; o; o >>= 1) v += (unsigned)__shfl_xor((int)v, o);
    return (unsigned)__builtin_amdgcn_readfirstlane((int)v);
}

template <int B, int RF>
__global__ __launch_bounds__(64 * BMW_WAVES) void mv_chain_heal_decide_kernel(const uint8_t *__restrict__ cur, const uint8_t *__restrict__ key, HealArgs s,
                                                                              const int *__restrict__ merged, const uint8_t *__restrict__ link,
                                                                              int4 *__restrict__ dec, unsigned *__restrict__ sad_out,
                                                                              unsigned long long *__restrict__ stats) {
    constexpr int r = RF, n = 2 * r + 1, n2 = n * n, CD = B / 4, WD = BMW_WD<B>, SLOT = (B + 2 * r) * WD;      // dwords of one window
    __shared__ unsigned win_all[BMW_WAVES][HL_CENTRES * SLOT];
    __shared__ int2 cent_all[BMW_WAVES][HL_CENTRES + 1];              // per wave: its distinct centres
    __shared__ unsigned long long part[ARSEG_HEAL_NSTATS];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    unsigned *win = win_all[wave];
    int2 *cent = cent_all[wave];
    const unsigned m4 = (unsigned)s.flag_mask * 0x01010101u;
    if (tid < ARSEG_HEAL_NSTATS) part[tid] = 0;
    __syncthreads();
    for (int b = blockIdx.x * BMW_WAVES + wave; b < s.n_blocks; b += gridDim.x * BMW_WAVES) {          // wave uniform
        const int bi = b / s.bx, bj = b - bi * s.bx, x0 = bj * B, y0 = bi * B;
        const int w = min(B, s.W - x0), h = min(B, s.H - y0);
        // the link bytes under lane i's dword of the block: vm the bytes that are pixels of the block, fm the flagged ones among them
        unsigned lk = 0, vm = 0;
        if (lane < B * CD) {
            const int rr = lane / CD, rem = w - 4 * (lane % CD);
            if (rr < h && rem > 0) {
                lk = hl_link4(link + (size_t)(y0 + rr) * s.W, x0 + 4 * (lane % CD), s.W);
                vm = rem >= 4 ? 0xffffffffu : (1u << (8 * rem)) - 1u;
            }
        }
        const unsigned fm = hl_flagged(lk, m4) & vm;
        const int nf = __builtin_popcountll(__builtin_amdgcn_ballot_w64((fm & 0xffu) != 0)) + __builtin_popcountll(__builtin_amdgcn_ballot_w64((fm & 0xff00u) != 0)) +
                       __builtin_popcountll(__builtin_amdgcn_ballot_w64((fm & 0xff0000u) != 0)) + __builtin_popcountll(__builtin_amdgcn_ballot_w64((fm & 0xff000000u) != 0));
        if (nf < s.min_flagged) {                                      // skipped: most blocks of most frames end here
            if (lane == 0) {
                dec[b] = make_int4(x0 | (y0 << 16), w | (h << 16), 0, 2 | (nf << 16));
                if (stats && nf) atomicAdd(&part[4], (unsigned long long)nf);
            }
            continue;                                                  // no window of this wave was touched
        }
        // merged >> 2 at a pixel, wave uniform
        auto at = [&](int x, int y, int &cx, int &cy) {
            const int m = merged[(size_t)y * s.W + x];
            cx = (short)(m & 0xffff) >> 2;
            cy = (m >> 16) >> 2;
        };
        int cxs[HL_CENTRES], cys[HL_CENTRES];
        bool oks[HL_CENTRES];
        cxs[0] = 0; cys[0] = 0; oks[0] = true;
        at(x0 + w / 2, y0 + h / 2, cxs[1], cys[1]);
        oks[1] = true;
#pragma unroll
        for (int k = 2; k < 6; ++k) {                                  // the centre pixel of the left, right, upper and lower neighbour block
            const int qi = bi + (k == 4 ? -1 : (k == 5 ? 1 : 0)), qj = bj + (k == 2 ? -1 : (k == 3 ? 1 : 0));
            cxs[k] = 0; cys[k] = 0;
            oks[k] = qi >= 0 && qi < s.by && qj >= 0 && qj < s.bx;
            if (oks[k]) {
                const int qx0 = qj * B, qy0 = qi * B, xc = qx0 + min(B, s.W - qx0) / 2, yc = qy0 + min(B, s.H - qy0) / 2;
                oks[k] = (link[(size_t)yc * s.W + xc] & s.flag_mask) == 0;
                if (oks[k]) at(xc, yc, cxs[k], cys[k]);
            }
        }
        {                                                              // the first unflagged pixel of the block in raster order: lanes, then bytes
            const unsigned um = vm & ~fm;
            const unsigned long long ub = __builtin_amdgcn_ballot_w64(um != 0);
            cxs[6] = 0; cys[6] = 0;
            oks[6] = ub != 0;
            if (oks[6]) {
                const int L = __builtin_ctzll(ub), k = __builtin_ctz((unsigned)__builtin_amdgcn_readlane((int)um, L)) >> 3;
                at(x0 + 4 * (L % CD) + k, y0 + L / CD, cxs[6], cys[6]);
            }
        }
        const int c1x = cxs[1], c1y = cys[1];
        // The distinct centres, in order (block_motion_anchor.hip): window j and cent[j] belong to the j-th distinct centre; nc is 1 .. 7
        int nc = 0;
#pragma unroll
        for (int k = 0; k < HL_CENTRES; ++k) {
            bool take = oks[k];
#pragma unroll
            for (int j = 0; j < k; ++j) take = take && !(oks[j] && cxs[j] == cxs[k] && cys[j] == cys[k]);
            if (!take) continue;                                       // wave uniform
            if (lane == 0) cent[nc] = make_int2(cxs[k], cys[k]);
            bmw_stage<B, r>(win + nc * SLOT, key, s.key_pitch, s.H, s.W, x0 + cxs[k] - r, y0 + cys[k] - r, lane);
            ++nc;
        }
        const int nq = nc * n2;
        unsigned cmask[CD];
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
        const int rank = (int)(kw & 0xfffffffu), dy = (rank >> 14) - 8192, dx = (rank & 16383) - 8192;
        // SAD_flagged of the winner: it lies in the window of a centre within r of it; every lane takes its own dword of the block there
        int kk = 0;
        for (int j = nc - 1; j >= 0; --j) {                             // wave uniform; the first such window
            const int2 c = cent[j];
            if (abs(dx - c.x) <= r && abs(dy - c.y) <= r) kk = j;
        }
        unsigned sf = 0;
        if (lane < B * CD) {
            const int2 c = cent[kk];
            const int sb = ((x0 + c.x - r) & 3) + dx - c.x + r;
            const unsigned *p = win + kk * SLOT + (dy - c.y + r + lane / CD) * WD + (sb >> 2) + lane % CD;
            sf = __builtin_amdgcn_sad_u8(__builtin_amdgcn_alignbyte(p[1], p[0], (unsigned)sb & 3u) & fm, mine & fm, 0u);
        }
        sf = hl_wave_sum(sf);
        if (lane == 0) {
            const int drift = abs(dx - c1x) + abs(dy - c1y);
            const bool healed = sf <= (unsigned)(s.intra * nf);
            dec[b] = make_int4(x0 | (y0 << 16), w | (h << 16), ((4 * dx) & 0xffff) | ((4 * dy) << 16), (healed ? 0 : 1) | (nf << 16));
            if (sad_out) sad_out[b] = sf;
            if (stats) {
                atomicAdd(&part[0], 1ull);
                atomicAdd(&part[2], (unsigned long long)nf);
                if (healed) {
                    atomicAdd(&part[1], 1ull);
                    atomicAdd(&part[3], (unsigned long long)nf);
                    if (drift) atomicAdd(&part[5], (unsigned long long)drift);
                }
            }
        }
        bmw_wave_sync();                                               // the next block's windows go where this one's were read
    }
    if (stats) {                                                       // bm_stats_flush's pattern, for this entry's row of counters
        __syncthreads();
        if (tid < ARSEG_HEAL_NSTATS && part[tid]) atomicAdd(&stats[tid], part[tid]);
    }
}

// bshift: log2 B.  Four pixels of a row never straddle two blocks
__global__ __launch_bounds__(256) void mv_chain_heal_apply_kernel(const int2 *__restrict__ dec, int H, int W, int bx, int bshift, int flag_mask,
                                                                  int *__restrict__ merged, uint8_t *__restrict__ link, unsigned long long *__restrict__ row) {
    __shared__ int part[ARSEG_LINK_NSTATS];
    const int tid = threadIdx.x, wq = (W + 3) >> 2;
    const unsigned m4 = (unsigned)flag_mask * 0x01010101u;
    if (row) {
        if (tid < ARSEG_LINK_NSTATS) part[tid] = 0;
        __syncthreads();
    }
    for (long long i = (long long)blockIdx.x * 256 + tid; i < (long long)H * wq; i += (long long)gridDim.x * 256) {
        const int y = (int)(i / wq), x = 4 * (int)(i - (long long)y * wq);
        const int2 d = dec[2 * ((size_t)(y >> bshift) * bx + (x >> bshift)) + 1];       // (4 dx, 4 dy), (state, n)
        if ((short)(d.y & 0xffff) != 0) continue;
        uint8_t *lrow = link + (size_t)y * W;
        const unsigned lk = hl_link4(lrow, x, W), fm = hl_flagged(lk, m4);
        if (!fm) continue;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (!((fm >> (8 * k)) & 1u)) continue;
            merged[(size_t)y * W + x + k] = d.x;
            lrow[x + k] = 0x10;
            if (row) atomicSub(&part[4 + ((lk >> (8 * k + 4)) & 15u)], 1);
        }
        if (row) {                                                     // the old flags go, hop bin 1 comes
            const unsigned f = lk & fm;
            const int c0 = __builtin_popcount(f & 0x01010101u), c1 = __builtin_popcount(f & 0x02020202u), c2 = __builtin_popcount(f & 0x04040404u);
            const int c3 = __builtin_popcount(fm & 0x01010101u);
            if (c0) atomicSub(&part[0], c0);
            if (c1) atomicSub(&part[1], c1);
            if (c2) atomicSub(&part[2], c2);
            atomicSub(&part[3], c3);
            atomicAdd(&part[4 + 1], c3);
        }
    }
    if (row) {
        __syncthreads();
        if (tid < ARSEG_LINK_NSTATS && part[tid]) atomicAdd(&row[tid], (unsigned long long)(long long)part[tid]);
    }
}

extern "C" int arseg_mv_chain_heal_fwd(const uint8_t *cur, int64_t cur_pitch, const uint8_t *key, int64_t key_pitch, int H, int W, int B, int r, int lambda,
                                       int intra, int flag_mask, int min_flagged, int16_t *merged_f, uint8_t *link_f, int16_t *decisions, uint32_t *sad,
                                       int64_t *stats, int64_t *link_stats_row, arseg_stream_t stream) {
    ARSEG_CHECK_PTR(cur); ARSEG_CHECK_PTR(key); ARSEG_CHECK_PTR(merged_f); ARSEG_CHECK_PTR(link_f); ARSEG_CHECK_PTR(decisions);
    if (!bm_args_ok(H, W, B, lambda, intra, decisions, sad, stats) || r < 1 || r > BMW_MAX_REFINE) return ARSEG_EINVAL;
    if (flag_mask < 1 || flag_mask > 7 || min_flagged < 1 || min_flagged > 64) return ARSEG_EINVAL;
    if (!bmw_plane_ok(cur, cur_pitch, W) || !bmw_plane_ok(key, key_pitch, W)) return ARSEG_EINVAL;
    if ((reinterpret_cast<uintptr_t>(merged_f) & 3u) || (reinterpret_cast<uintptr_t>(link_stats_row) & 7u)) return ARSEG_EINVAL;
    const HealArgs s = {H, W, arseg_cdiv(W, B), arseg_cdiv(H, B), arseg_cdiv(W, B) * arseg_cdiv(H, B), cur_pitch, key_pitch, lambda, intra, flag_mask, min_flagged};
    hipStream_t st = arseg_stream(stream);
    bmw_dispatch(B, r, [&](auto bb, auto rr) {
        hipLaunchKernelGGL((mv_chain_heal_decide_kernel<bb(), rr()>), dim3(bmw_grid(s.n_blocks)), dim3(64 * BMW_WAVES), 0, st, cur, key, s,
                           reinterpret_cast<const int *>(merged_f), link_f, reinterpret_cast<int4 *>(decisions), sad, reinterpret_cast<unsigned long long *>(stats));
    });
    const int status = arseg_launch_status();
    if (status != ARSEG_OK) return status;
    // like bmw_grid: the correction of all workgroups lands on one cache line of link_stats_row, so there are at most two per compute unit
    hipLaunchKernelGGL(mv_chain_heal_apply_kernel, dim3(arseg_grid_for((long long)H * ((W + 3) >> 2), 2 * arseg_cu_count())), dim3(256), 0, st, reinterpret_cast<const int2 *>(decisions), H, W,
                       s.bx, B == 8 ? 3 : 4, flag_mask, reinterpret_cast<int *>(merged_f), link_f, reinterpret_cast<unsigned long long *>(link_stats_row));
    return arseg_launch_status();
}
