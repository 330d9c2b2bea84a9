// Confusion counts in bands around the label boundaries (include/arseg_hip.h, arseg_label_bands_fwd): the int64 label planes the evaluators
// pass and the int32 predictions of the argmax tail in; per group of frames one confusion matrix per band of Chebyshev distance to the
// nearest pixel of another label, and / or the band of every pixel as a byte plane, out.  Integers throughout: every output is a pure
// function of the inputs, whatever order the atomics arrive in.  No floating point in this file.
//
// The distance D(p) of the header is separable.  With hd(x, y) the distance within row y to the nearest pixel of another byte (R + 1 if
// there is none within R, the largest radius) and v the byte at (x, y):
//   D(x, y) = min(hd(x, y), min over dy = 1 .. R, y' = y +- dy inside the image of (byte(x, y') != v ? dy : max(dy, hd(x, y'))))
// and the walk over dy stops once dy >= the best so far.  So the scratch is one 16-bit word per pixel, byte | hd << 8, in the caller's
// workspace ([N][H][W], dense), and there are 2 launches, sized on the host; a phase boundary is a launch boundary: no workgroup waits
// for another, nothing spins.
//   rows     a workgroup owns BD_SEG pixels of a row at a time (grid-stride over the frames' row segments).  The labels of the segment
//            and of 64 + 1 pixels either side become bytes in LDS; per 64-pixel chunk a wave's ballot of "differs from my left
//            neighbour" is a 64-bit mask (18 masks: the segment's 16 chunks and one either side); a pixel's hd is then a count of
//            leading zeros on the masks left of it and of trailing zeros right of it -- with R <= 32 one chunk either side suffices.
//            Chosen over the per-lane look of +-R bytes from the staged row by the generated code: the per-pixel part compiles to a
//            ds_read2_b64 and a ds_read_b64 of the three masks at wave-uniform addresses, four 64-bit shifts, two v_ffbh_u32, two
//            v_ffbl_b32, two v_min_u32 and a v_min3_u32 -- about 35 instructions and no loop --, where the look is a loop of up to R
//            rounds of two dependent byte reads and compares (up to 64 LDS reads and a divergent exit per pixel).  Either way the
//            launch moves 8 bytes in and 2 out per pixel.
//   columns  a workgroup owns a tile of BD_TW x BD_TH pixels at a time (blockIdx.y strides over the frames, blockIdx.x over the frame's
//            tiles, so a workgroup stays inside one frame between flushes).  The tile's words and its halo of R rows above and below go
//            to LDS (no halo left and right: hd has the row's part already); a thread walks dy for each of its 16 pixels, one 16-bit LDS
//            read per step; the band is the number of radii below D.  band_out gets the byte.  The tally goes into an LDS histogram of
//            (n_bands + 1) n_cls^2 32-bit counters, per wave and distinct (band, label, pred) code one LDS atomic (bd_tally), flushed per
//            workgroup and frame with one 64-bit global atomic per non-zero counter into hist[group[n]].
//
// Bounds of the loops (nothing else loops):
//   grid-stride loops   over frames, row segments, tiles, a tile's rows, the histogram: counted.
//   the staging         (BD_SEG + 129) / 256 + 1 rounds in rows, (BD_TH + 2 R) * BD_TW / 256 in columns, R <= 32 checked on the host.
//   the dy walk         dy = 1 .. R, left early once dy >= the best so far.
//   the bands           n_bands <= 8 compares, checked on the host.
//   bd_tally            every round retires at least the leading lane: at most 64 rounds.
// Clamps: a label outside [0, n_cls) or equal to ignore_label is the byte 255, so a label byte that counts is below n_cls <= 32; a
// prediction outside [0, n_cls) counts nowhere; a band is at most n_bands; so a counter's index is below (n_bands + 1) n_cls^2, the size
// of the LDS histogram the host asked for.  A group id outside [0, n_groups) counts nowhere.  Rows and columns outside the image are
// neither staged nor read.  Malformed labels only ever give void; nothing outside the caller's buffers is touched.
#include "arseg_common.h"

namespace {

constexpr int BD_SEG = 1024;                            // the pixels of a row a workgroup of rows takes at a time: 16 chunks of 64
constexpr int BD_NMASK = BD_SEG / 64 + 2;               // their masks and one chunk's either side
constexpr int BD_TW = 64;                               // the tile of columns: a wave is a row of it
constexpr int BD_TH = 64;                               // 16 pixels of a column per thread
constexpr int BD_RMAX = 32;                             // the largest radius
constexpr int BD_NBMAX = 8;                             // the most bands
constexpr unsigned BD_VOID = 255u;

struct BdP {
    const long long *label;                             // [N][H][W]
    const int *pred;                                    // [N][H][W] (may be null)
    const int *group;                                   // [N] (null: every frame is group 0)
    unsigned char *band_out;                            // (may be null)
    unsigned long long *hist;                           // [n_groups][n_bands + 1][n_cls][n_cls] (may be null)
    unsigned short *words;                              // the workspace: [N][H][W]
    long long band_pitch, band_ns;
    int radii[BD_NBMAX];
    int N, H, W, n_groups, n_cls, n_bands, R, ignore_label;
};

__device__ __forceinline__ unsigned bd_byte(long long lab, int n_cls, int ignore_label) {
    return lab >= 0 && lab < (long long)n_cls && lab != (long long)ignore_label ? (unsigned)lab : BD_VOID;
}

__global__ __launch_bounds__(256) void bands_rows_kernel(const BdP p) {
    __shared__ unsigned char bytes[BD_SEG + 129 + 3];   // bytes[i] is the pixel at column seg0 - 65 + i
    __shared__ unsigned long long masks[BD_NMASK];      // masks[k] bit j: column seg0 - 64 + 64 k + j differs from the one left of it
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int W = p.W, segs = (W + BD_SEG - 1) / BD_SEG;
    const long long items = (long long)p.N * p.H * segs;
    for (long long item = blockIdx.x; item < items; item += gridDim.x) {      // uniform: every thread makes every pass
        const int seg0 = (int)(item % segs) * BD_SEG;
        const long long row = item / segs;                                    // n * H + y
        const long long *lab = p.label + (size_t)row * (size_t)W;
        for (int i = tid; i < BD_SEG + 129; i += 256) {
            const int x = seg0 - 65 + i;
            bytes[i] = x >= 0 && x < W ? (unsigned char)bd_byte(lab[x], p.n_cls, p.ignore_label) : (unsigned char)0;
        }
        __syncthreads();
        for (int k = wave; k < BD_NMASK; k += 4) {                            // (the row's first pixel and those past its end: no change)
            const int x = seg0 - 64 + 64 * k + lane, i = 1 + 64 * k + lane;
            const unsigned long long m = __ballot(x > 0 && x < W && bytes[i] != bytes[i - 1]);
            if (lane == 0) masks[k] = m;
        }
        __syncthreads();
        unsigned short *out = p.words + (size_t)row * (size_t)W;
#pragma unroll
        for (int j = 0; j < BD_SEG / 256; ++j) {
            const int q = tid + 256 * j, x = seg0 + q;
            if (x >= W) continue;
            const int k = 1 + (q >> 6), i = q & 63;
            const unsigned long long prev = masks[k - 1], cur = masks[k], next = masks[k + 1];
            // left: bit 63 - d of wl is the mask bit of column x - d, whose left neighbour, at distance d + 1, differs
            const unsigned long long wl = (cur << (63 - i)) | (i < 63 ? prev >> (i + 1) : 0ull);
            // right: bit d of wr is the mask bit of column x + 1 + d, which differs from its left neighbour: from x, at distance d + 1
            const unsigned long long wr = (i < 63 ? cur >> (i + 1) : 0ull) | (next << (63 - i));
            const unsigned dl = wl ? (unsigned)__builtin_clzll(wl) + 1u : 65u, dr = wr ? (unsigned)__builtin_ctzll(wr) + 1u : 65u;
            const unsigned hd = min(min(dl, dr), (unsigned)p.R + 1u);
            out[x] = (unsigned short)((unsigned)bytes[65 + q] | (hd << 8));
        }
        __syncthreads();                                                      // before the next segment's bytes
    }
}

// The pixels of a wave tallied by their code (band * n_cls + label) * n_cls + pred: per distinct code of the wave its leading lane adds the
// number of lanes that hold it, one LDS atomic.  Every lane of the wave calls.
__device__ __forceinline__ void bd_tally(unsigned *lh, unsigned code, bool active, int lane) {
    unsigned long long todo = __ballot(active);
    while (todo) {
        const int lead = __builtin_ctzll(todo);
        const unsigned lc = (unsigned)__shfl((int)code, lead, 64);
        const unsigned long long same = __ballot(active && code == lc);
        if (lane == lead) atomicAdd(lh + lc, (unsigned)__builtin_popcountll(same));
        todo &= ~same;
    }
}

__global__ __launch_bounds__(256) void bands_cols_kernel(const BdP p) {
    extern __shared__ unsigned bd_lds[];                                      // the histogram (when a frame can count), then the tile
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int H = p.H, W = p.W, R = p.R, n_cls = p.n_cls;
    const int nh = p.hist != nullptr ? (p.n_bands + 1) * n_cls * n_cls : 0;
    unsigned *lh = bd_lds;
    unsigned short *tile = reinterpret_cast<unsigned short *>(bd_lds + nh);   // [BD_TH + 2 R][BD_TW]: row r is image row y0 - R + r
    const int tiles_x = (W + BD_TW - 1) / BD_TW, tiles = tiles_x * ((H + BD_TH - 1) / BD_TH);
    for (int n = blockIdx.y; n < p.N; n += gridDim.y) {
        const int g = p.hist == nullptr ? -1 : (p.group != nullptr ? p.group[n] : 0);
        const bool count = g >= 0 && g < p.n_groups;                          // uniform over the workgroup
        if (!count && p.band_out == nullptr) continue;
        if (count) {
            for (int i = tid; i < nh; i += 256) lh[i] = 0u;
            __syncthreads();
        }
        const unsigned short *words = p.words + (size_t)n * (size_t)H * (size_t)W;
        const int *pred = count ? p.pred + (size_t)n * (size_t)H * (size_t)W : nullptr;
        unsigned char *bout = p.band_out != nullptr ? p.band_out + (size_t)n * (size_t)p.band_ns : nullptr;
        for (int t = blockIdx.x; t < tiles; t += gridDim.x) {                 // uniform: every thread makes every pass
            const int x0 = (t % tiles_x) * BD_TW, y0 = (t / tiles_x) * BD_TH;
            const int x = x0 + lane;
            for (int r = wave; r < BD_TH + 2 * R; r += 4) {
                const int y = y0 - R + r;
                if (y >= 0 && y < H && x < W) tile[r * BD_TW + lane] = words[(size_t)y * (size_t)W + x];
            }
            __syncthreads();
            for (int ly = wave; ly < BD_TH; ly += 4) {                        // uniform: bd_tally needs every lane
                const int y = y0 + ly;
                const bool inside = y < H && x < W;
                int pr = -1;
                if (inside && count) pr = pred[(size_t)y * (size_t)W + x];
                unsigned v = BD_VOID, band = 0;
                if (inside) {
                    const unsigned short *col = tile + (R + ly) * BD_TW + lane;
                    const unsigned w0 = col[0];
                    v = w0 & 0xffu;
                    unsigned best = w0 >> 8;
                    for (unsigned dy = 1; dy <= (unsigned)R && dy < best; ++dy) {
                        if (y >= (int)dy) {
                            const unsigned u = col[-(int)dy * BD_TW];
                            best = min(best, (u & 0xffu) != v ? dy : max(dy, u >> 8));
                        }
                        if (y + (int)dy < H) {
                            const unsigned u = col[(int)dy * BD_TW];
                            best = min(best, (u & 0xffu) != v ? dy : max(dy, u >> 8));
                        }
                    }
                    for (int k = 0; k < p.n_bands; ++k) band += best > (unsigned)p.radii[k] ? 1u : 0u;
                    if (bout != nullptr) bout[(size_t)y * (size_t)p.band_pitch + x] = (unsigned char)band;
                }
                if (count) {
                    const bool active = inside && v != BD_VOID && pr >= 0 && pr < n_cls;
                    bd_tally(lh, active ? (band * (unsigned)n_cls + v) * (unsigned)n_cls + (unsigned)pr : 0u, active, lane);
                }
            }
            __syncthreads();                                                  // before the next tile's words
        }
        if (count) {
            __syncthreads();
            unsigned long long *hist = p.hist + (size_t)g * (size_t)nh;
            for (int i = tid; i < nh; i += 256)
                if (lh[i]) atomicAdd(hist + i, (unsigned long long)lh[i]);
            __syncthreads();                                                  // before the next frame clears them
        }
    }
}

}  // namespace

// 2 bytes per pixel, rounded up to 16 bytes in all; a size that does not fit size_t comes back as its largest value, which no workspace has
extern "C" size_t arseg_label_bands_workspace_bytes(int N, int H, int W) {
    if (N <= 0 || H <= 0 || W <= 0 || H > 16384 || W > 16384) return 0;
    const size_t none = ~(size_t)0;
    size_t bytes = 2 * (size_t)H * (size_t)W;
    if (__builtin_mul_overflow(bytes, (size_t)N, &bytes) || bytes > none - 15) return none;
    return (bytes + 15) & ~(size_t)15;
}

extern "C" int arseg_label_bands_fwd(const int64_t *label, const int32_t *pred, const int32_t *group, const int *radii, int n_bands,
                                     uint8_t *band_out, int64_t band_pitch, int64_t band_n_stride, int64_t *hist, int N, int n_groups,
                                     int n_cls, int H, int W, int ignore_label, void *workspace, size_t workspace_bytes,
                                     arseg_stream_t stream) {
    ARSEG_CHECK_PTR(label); ARSEG_CHECK_PTR(workspace); ARSEG_CHECK_PTR(radii);
    ARSEG_CHECK_POS(N); ARSEG_CHECK_POS(H); ARSEG_CHECK_POS(W);
    if (H > 16384 || W > 16384 || n_cls < 1 || n_cls > 32 || n_groups < 1 || n_bands < 1 || n_bands > BD_NBMAX) return ARSEG_EINVAL;
    for (int k = 0; k < n_bands; ++k)
        if (radii[k] < 1 || radii[k] > BD_RMAX || (k > 0 && radii[k] <= radii[k - 1])) return ARSEG_EINVAL;
    if (group == nullptr && n_groups > 1) return ARSEG_EINVAL;
    if (hist != nullptr && pred == nullptr) return ARSEG_EINVAL;
    if (band_out != nullptr && (band_pitch < (int64_t)W || band_n_stride < 0)) return ARSEG_EINVAL;
    if ((reinterpret_cast<uintptr_t>(label) & 7u) || (reinterpret_cast<uintptr_t>(hist) & 7u) || (reinterpret_cast<uintptr_t>(pred) & 3u) ||
        (reinterpret_cast<uintptr_t>(group) & 3u) || (reinterpret_cast<uintptr_t>(workspace) & 1u))
        return ARSEG_EINVAL;
    const size_t need = arseg_label_bands_workspace_bytes(N, H, W);
    if (need == ~(size_t)0 || workspace_bytes < need) return ARSEG_EWORKSPACE;
    BdP p = {};
    p.label = reinterpret_cast<const long long *>(label); p.pred = pred; p.group = group; p.band_out = band_out;
    p.hist = reinterpret_cast<unsigned long long *>(hist); p.words = static_cast<unsigned short *>(workspace);
    p.band_pitch = band_pitch; p.band_ns = band_n_stride;
    for (int k = 0; k < n_bands; ++k) p.radii[k] = radii[k];
    p.N = N; p.H = H; p.W = W; p.n_groups = n_groups; p.n_cls = n_cls; p.n_bands = n_bands; p.R = radii[n_bands - 1];
    p.ignore_label = ignore_label;
    hipStream_t st = arseg_stream(stream);
    const long long segments = (long long)N * H * ((W + BD_SEG - 1) / BD_SEG);
    hipLaunchKernelGGL(bands_rows_kernel, dim3((unsigned)(segments < 8192 ? segments : 8192)), dim3(256), 0, st, p);
    if (band_out == nullptr && hist == nullptr) return arseg_launch_status();  // the row pass alone: the workspace holds the words
    const int gy = N < 65535 ? N : 65535, share = 4096 / gy;
    const int tiles = ((W + BD_TW - 1) / BD_TW) * ((H + BD_TH - 1) / BD_TH);
    const int gx = tiles < share ? tiles : (share < 1 ? 1 : share);
    const size_t lds = (hist != nullptr ? 4 * (size_t)(n_bands + 1) * n_cls * n_cls : 0) + 2 * (size_t)(BD_TH + 2 * p.R) * BD_TW;
    hipLaunchKernelGGL(bands_cols_kernel, dim3(gx, gy), dim3(256), lds, st, p);
    return arseg_launch_status();
}
