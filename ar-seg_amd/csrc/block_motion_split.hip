// Quad-tree split of estimated 16 x 16 block motion (contract: include/arseg_hip.h, arseg_block_motion_split_fwd): every parent block of the
// B = 16 grid is searched again as four 8 x 8 children around its own and its neighbours' vectors, and where four vectors explain the block
// better than one by more than split_gain -- or where an intra parent has a child that matches -- the children are written as records behind
// the parents', where the chain lets them win their pixels.  8-bit integer arithmetic; the wave-per-block search (windows, SAD, clipped
// blocks) is block_motion_wave.h's, shared with block_motion_refine_kernel (block_motion_pyr.hip), whose centres, cost and key these are.
// This kernel's own:
//   wave    : a wave per PARENT, BMS_WAVES per workgroup.  It reads the records of the parent and of its four neighbours once (wave
//             uniform), stages the windows of ALL four children -- sixteen of (8 + 2 r) x 5 dwords -- and loads their four blocks before it
//             waits once, so a parent costs two round trips to memory and not five; then it walks the children in turn: the child's 16
//             dwords in lanes 0 .. 15, one minimum over the wave.  The four winners stay in uniform registers.  Sixteen windows are 4.4 KB
//             per wave at r = 3: eight waves per workgroup keep that under the 64 KB a kernel may declare
//   S_q(P)  : the child's SAD at the parent's vector is the candidate (C1, 0, 0), which one lane of one pass owns: read from there
//   rows    : after the decision lanes 0 .. 3 store the four rows, 16 bytes each; every row of every parent is written
#include "block_motion_wave.h"

constexpr int BMS_WAVES = 8;
constexpr int BMS_MAX_V = 500;                                         // |Px|, |Py| of a usable parent: rank and cost stay inside the refinement's key

struct SplitArgs {
    int H, W, bx, by, n_parents;
    long long cur_pitch, ref_pitch;
    int lam, intra, split_gain, ref_index;
};

template <int RF>
__global__ __launch_bounds__(64 * BMS_WAVES) void block_motion_split_kernel(const uint8_t *__restrict__ cur, const uint8_t *__restrict__ ref, SplitArgs s,
                                                                            const int4 *__restrict__ rec_in, int4 *__restrict__ children,
                                                                            unsigned *__restrict__ sad_out, unsigned long long *__restrict__ stats) {
    constexpr int B = 8, PB = 16, r = RF, n = 2 * r + 1, n2 = n * n, SLOT = (B + 2 * r) * BMW_WD<B>;      // dwords of one window
    constexpr int Q1 = n2 + r * n + r;                                 // the candidate (C1, 0, 0) in the order of the passes below
    __shared__ unsigned win_all[BMS_WAVES][16 * SLOT];
    __shared__ unsigned long long part[ARSEG_BMS_NSTATS];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    unsigned *win = win_all[wave];
    if (tid < ARSEG_BMS_NSTATS) part[tid] = 0;
    __syncthreads();
    for (int b = blockIdx.x * BMS_WAVES + wave; b < s.n_parents; b += gridDim.x * BMS_WAVES) {          // wave uniform
        const int bi = b / s.bx, bj = b - bi * s.bx;
        // P of parent (qi, qj), which is in the grid, and whether it is usable: wave uniform
        auto parent = [&](int qi, int qj, int &px, int &py) -> bool {
            const int4 q = rec_in[(size_t)qi * s.bx + qj];
            px = round_half_even_div4((short)(q.z & 0xffff));
            py = round_half_even_div4(q.z >> 16);
            const int qx0 = qj * PB, qy0 = qi * PB, qw = min(PB, s.W - qx0), qh = min(PB, s.H - qy0);
            return (short)(q.w & 0xffff) == s.ref_index && abs(px) <= BMS_MAX_V && abs(py) <= BMS_MAX_V && qx0 + px >= 0 && qx0 + qw + px <= s.W &&
                   qy0 + py >= 0 && qy0 + qh + py <= s.H;
        };
        int Px = 0, Py = 0, nx[2] = {0, 0}, ny[2] = {0, 0}, ux[2] = {0, 0}, uy[2] = {0, 0};      // own; left / right; upper / lower
        const bool usable = parent(bi, bj, Px, Py);
        bool okn[2], oku[2];
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            const int qj = bj + (e ? 1 : -1), qi = bi + (e ? 1 : -1);
            okn[e] = qj >= 0 && qj < s.bx;
            if (okn[e]) okn[e] = parent(bi, qj, nx[e], ny[e]);
            oku[e] = qi >= 0 && qi < s.by;
            if (oku[e]) oku[e] = parent(qi, bj, ux[e], uy[e]);
        }
        int wdx[4], wdy[4];
        unsigned wsad[4], wcost[4], sp[4];                             // per child: the winner, and S_q(P)
        unsigned mine_q[4], cmask_q[4][B / 4];
        bool exists[4];
        // every window of every child and the four blocks, all loads in flight before the one wait
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int qx = q & 1, qy = q >> 1, x0 = PB * bj + B * qx, y0 = PB * bi + B * qy;
            exists[q] = s.W - x0 > 0 && s.H - y0 > 0;
            mine_q[q] = 0;
            cmask_q[q][0] = cmask_q[q][1] = 0;
            if (!exists[q]) continue;                                  // wave uniform
            // The window of a centre that is not there is not staged: no candidate reads it
            auto stage = [&](int k, int cx, int cy) { bmw_stage<B, r>(win + (4 * q + k) * SLOT, ref, s.ref_pitch, s.H, s.W, x0 + cx - r, y0 + cy - r, lane); };
            stage(0, 0, 0);
            if (usable) stage(1, Px, Py);
            if (okn[qx]) stage(2, nx[qx], ny[qx]);
            if (oku[qy]) stage(3, ux[qy], uy[qy]);
            mine_q[q] = bmw_load_block<B>(cur, s.cur_pitch, s.H, s.W, x0, y0, lane, cmask_q[q]);
        }
        bmw_wave_sync();
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int qx = q & 1, qy = q >> 1, x0 = PB * bj + B * qx, y0 = PB * bi + B * qy;
            const int w = min(B, s.W - x0), h = min(B, s.H - y0);
            wdx[q] = wdy[q] = 0;
            wsad[q] = wcost[q] = sp[q] = 0;
            if (!exists[q]) continue;                                  // wave uniform
            const int cx1 = Px, cy1 = Py, cx2 = nx[qx], cy2 = ny[qx], cx3 = ux[qy], cy3 = uy[qy];
            const bool ok1 = usable, ok2 = okn[qx], ok3 = oku[qy];
            const unsigned mine = mine_q[q];
            const unsigned(&cmask)[B / 4] = cmask_q[q];
            unsigned long long best = BMW_NO_KEY;
            unsigned at_p = 0;
#pragma unroll
            for (int q0 = 0; q0 < 4 * n2; q0 += 64) {                   // wave uniform: the lane reads below are reached by the whole wave
                const int c = min(q0 + lane, 4 * n2 - 1), k = c / n2, t = c - k * n2, oyi = t / n, oxi = t - oyi * n;
                const int cx = k == 0 ? 0 : (k == 1 ? cx1 : (k == 2 ? cx2 : cx3)), cy = k == 0 ? 0 : (k == 1 ? cy1 : (k == 2 ? cy2 : cy3));
                const bool okc = k == 0 ? true : (k == 1 ? ok1 : (k == 2 ? ok2 : ok3));
                const int dx = cx + oxi - r, dy = cy + oyi - r;
                const bool valid = okc && q0 + lane < 4 * n2 && x0 + dx >= 0 && x0 + w + dx <= s.W && y0 + dy >= 0 && y0 + h + dy <= s.H;
                const unsigned sad = bmw_sad<B>(win + (4 * q + k) * SLOT, oyi, ((x0 + cx - r) & 3) + oxi, h, cmask, mine);
                if (q0 == (Q1 / 64) * 64) at_p = (unsigned)__builtin_amdgcn_readlane((int)sad, Q1 % 64);
                const unsigned cost = sad + (unsigned)(s.lam * (abs(dx) + abs(dy)));
                const unsigned rank = (dx | dy) == 0 ? 0u : (unsigned)(1 + (dy + 511) * 1023 + (dx + 511));
                const unsigned long long key = valid ? ((unsigned long long)cost << 20) | rank : BMW_NO_KEY;
                best = key < best ? key : best;
            }
            const unsigned long long key = bmw_wave_min(best);          // (0, 0) is always a candidate: a real key
            const int rank = (int)(key & 0xfffffu);
            if (rank) { wdy[q] = (rank - 1) / 1023 - 511; wdx[q] = (rank - 1) % 1023 - 511; }
            wcost[q] = (unsigned)(key >> 20);
            wsad[q] = wcost[q] - (unsigned)(s.lam * (abs(wdx[q]) + abs(wdy[q])));
            sp[q] = usable ? at_p : 0u;                                // unusable: window 1 was not staged, the value is not a SAD
        }
        // the decision, wave uniform
        int lhs = s.lam * (abs(Px) + abs(Py)), n_matched = 0, n_intra = 0, pixels = 0;
        bool matched[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int x0 = PB * bj + B * (q & 1), y0 = PB * bi + B * (q >> 1), w = min(B, s.W - x0), h = min(B, s.H - y0);
            matched[q] = exists[q] && wsad[q] <= (unsigned)(s.intra * w * h);
            if (exists[q]) lhs += (int)sp[q] - (int)wcost[q];
            if (matched[q]) { ++n_matched; pixels += w * h; }
            else if (exists[q]) ++n_intra;
        }
        const bool split = usable ? lhs > s.split_gain : n_matched > 0;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            if (lane != q) continue;
            const int x0 = PB * bj + B * (q & 1), y0 = PB * bi + B * (q >> 1), w = min(B, s.W - x0), h = min(B, s.H - y0);
            int4 row = make_int4(0, 0, 0, 0);                          // covers nothing
            if (split && exists[q]) row = matched[q] ? bm_record(x0, y0, w, h, wdx[q], wdy[q], s.ref_index) : bm_record(x0, y0, w, h, 0, 0, ARSEG_BM_INTRA_REF);
            children[(size_t)4 * b + q] = row;
            if (sad_out) sad_out[(size_t)4 * b + q] = wsad[q];          // 0 for a child that does not exist
        }
        if (stats && split && lane == 0) {
            atomicAdd(&part[0], 1ull);
            if (!usable) atomicAdd(&part[1], 1ull);
            else atomicAdd(&part[4], (unsigned long long)lhs);         // lhs > split_gain >= 0
            if (n_matched) atomicAdd(&part[2], (unsigned long long)n_matched);
            if (n_intra) atomicAdd(&part[3], (unsigned long long)n_intra);
            if (pixels) atomicAdd(&part[5], (unsigned long long)pixels);
        }
        bmw_wave_sync();                                               // the next parent's windows go where this one's were read
    }
    if (stats) {                                                       // reached by the whole workgroup
        __syncthreads();
        if (tid < ARSEG_BMS_NSTATS && part[tid]) atomicAdd(&stats[tid], part[tid]);
    }
}

// workgroups of BMS_WAVES parents: four per compute unit fill the device as bmw_grid's two of sixteen waves do, the rest come with the stride
static inline int bms_grid(int n_parents) { return min(arseg_cdiv(n_parents, BMS_WAVES), 4 * arseg_cu_count()); }

extern "C" int arseg_block_motion_split_fwd(const uint8_t *cur, int64_t cur_pitch, const uint8_t *ref, int64_t ref_pitch, int H, int W, int r, int lambda,
                                            int intra, int split_gain, int ref_index, const int16_t *records_in, int16_t *children, uint32_t *child_sad,
                                            int64_t *stats, arseg_stream_t stream) {
    ARSEG_CHECK_PTR(cur); ARSEG_CHECK_PTR(ref); ARSEG_CHECK_PTR(records_in); ARSEG_CHECK_PTR(children);
    if (!bm_args_ok(H, W, 16, lambda, intra, children, child_sad, stats) || r < 1 || r > BMW_MAX_REFINE) return ARSEG_EINVAL;
    if (split_gain < 0 || split_gain > 65535 || ref_index < 0 || ref_index > 15 || !ARSEG_ALIGNED16(records_in)) return ARSEG_EINVAL;
    if (!bmw_plane_ok(cur, cur_pitch, W) || !bmw_plane_ok(ref, ref_pitch, W)) return ARSEG_EINVAL;
    const SplitArgs s = {H, W, arseg_cdiv(W, 16), arseg_cdiv(H, 16), arseg_cdiv(W, 16) * arseg_cdiv(H, 16), cur_pitch, ref_pitch, lambda, intra, split_gain, ref_index};
    const uintptr_t in0 = reinterpret_cast<uintptr_t>(records_in), out0 = reinterpret_cast<uintptr_t>(children), bytes = (uintptr_t)16 * s.n_parents;
    if (in0 < out0 + 4 * bytes && out0 < in0 + bytes) return ARSEG_EINVAL;
    hipStream_t st = arseg_stream(stream);
    bmw_dispatch(8, r, [&](auto, auto rr) {
        hipLaunchKernelGGL((block_motion_split_kernel<rr()>), dim3(bms_grid(s.n_parents)), dim3(64 * BMS_WAVES), 0, st, cur, ref, s,
                           reinterpret_cast<const int4 *>(records_in), reinterpret_cast<int4 *>(children), child_sad, reinterpret_cast<unsigned long long *>(stats));
    });
    return arseg_launch_status();
}
