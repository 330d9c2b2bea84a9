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
//
// Boundary IoU (arseg_boundary_iou_fwd) is the same two passes on two byte planes, the labels' and the predictions' (a prediction
// outside [0, n_cls) is the byte 255), with radii up to BI_RMAX = 64.  The byte mapping (bd_byte), the row pass (bd_rows) and the
// wave tally (bd_tally) are defined once and used by both entry points.
//   rows     boundary_rows_kernel: blockIdx.y is the plane; bd_rows on int64 labels with ignore_label, on int32 predictions without.
//            The words of the planes are the two halves of the workspace ([2][N][H][W]).  The three masks of a pixel reach 64 columns
//            either side (bits of columns x - 63 .. x to the left: distances 1 .. 64; of x + 1 .. x + 64 to the right), the staging
//            65, so hd is exact up to 64 and 65 = R + 1 beyond: enough for R = 64.
//   columns  boundary_cols_kernel: the tile of bands_cols_kernel, both planes' words with their halo of R rows in LDS (rows of 66 words;
//            at R = 64 two times 192 x 66 words, 49.5 KB), but no walk: a wave takes a column of the tile with its lanes as the rows, and
//            the band is read off ballots over the column's rows as bd_rows reads hd off ballots over a row's columns (bi_column, which
//            says why that equals the walk).  Then the border term min(x + 1, y + 1, W - x, H - y) when asked for, both bands, and three
//            codes per counting pixel into 3 (n_bands + 1) n_cls 32-bit LDS counters (at most 3456 bytes), flushed as above.  With a
//            plane to write, the tile's bands go through LDS (64 x 68 bytes, both bands in a byte) so that rows of 64 bytes leave
//            together: 57.1 KB of dynamic LDS at most, below the 64 KB a launch gets without an attribute.
// Its loops: the same grid-stride loops; the staging (BD_SEG + 129) / 256 + 1 rounds in rows and (BD_TH + 2 R) / 16 + 1 rounds of four
// rows per wave in columns, R <= 64 checked on the host; 16 columns per wave and tile, each 3 chunks of rows and n_bands <= 8 radii on
// two planes; three bd_tally of at most 64 rounds.
// Its clamps: both bytes of a counting pixel are below n_cls and both bands at most n_bands, so a counter's index is below
// 3 (n_bands + 1) n_cls; a staged row is read only where b is in [64 - R, 128 + R), the rows the host sized the tiles for, and only in
// columns inside the image, which were staged; the planes' rows are written inside [0, W) only.
#include "arseg_common.h"

namespace {

constexpr int BD_SEG = 1024;                            // the pixels of a row a workgroup of rows takes at a time: 16 chunks of 64
constexpr int BD_NMASK = BD_SEG / 64 + 2;               // their masks and one chunk's either side
constexpr int BD_TW = 64;                               // the tile of columns: a wave is a row of it
constexpr int BD_TH = 64;                               // 16 pixels of a column per thread
constexpr int BD_RMAX = 32;                             // the largest radius of label_bands
constexpr int BI_RMAX = 64;                             // the largest radius of boundary_iou: what the row pass' three masks reach
constexpr int BD_NBMAX = 8;                             // the most bands
constexpr int BI_PITCH = BD_TW + 2;                     // words per staged row of boundary_cols_kernel: 33 dwords, so that the 64 rows of a
                                                        // column, one per lane, spread over the LDS banks
constexpr int BI_OPITCH = BD_TW + 4;                    // bytes per row of its staged bands: 17 dwords, for the same reason
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

// The row pass on one plane of N * H rows of W values of T: words[x] = byte | hd << 8, hd capped at R + 1 <= 65.  ``bytes`` (BD_SEG + 129
// + 3) and ``masks`` (BD_NMASK) are the caller's LDS; every thread of the workgroup calls.
template <typename T>
__device__ __forceinline__ void bd_rows(const T *__restrict__ src, unsigned short *__restrict__ words, int N, int H, int W, int n_cls,
                                        int ignore_label, int R, unsigned char *bytes, unsigned long long *masks) {
    // bytes[i] is the pixel at column seg0 - 65 + i; masks[k] bit j: column seg0 - 64 + 64 k + j differs from the one left of it
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int segs = (W + BD_SEG - 1) / BD_SEG;
    const long long items = (long long)N * H * segs;
    for (long long item = blockIdx.x; item < items; item += gridDim.x) {      // uniform: every thread makes every pass
        const int seg0 = (int)(item % segs) * BD_SEG;
        const long long row = item / segs;                                    // n * H + y
        const T *lab = src + (size_t)row * (size_t)W;
        for (int i = tid; i < BD_SEG + 129; i += 256) {
            const int x = seg0 - 65 + i;
            bytes[i] = x >= 0 && x < W ? (unsigned char)bd_byte((long long)lab[x], n_cls, ignore_label) : (unsigned char)0;
        }
        __syncthreads();
        for (int k = wave; k < BD_NMASK; k += 4) {                            // (the row's first pixel and those past its end: no change)
            const int x = seg0 - 64 + 64 * k + lane, i = 1 + 64 * k + lane;
            const unsigned long long m = __ballot(x > 0 && x < W && bytes[i] != bytes[i - 1]);
            if (lane == 0) masks[k] = m;
        }
        __syncthreads();
        unsigned short *out = words + (size_t)row * (size_t)W;
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
            const unsigned hd = min(min(dl, dr), (unsigned)R + 1u);
            out[x] = (unsigned short)((unsigned)bytes[65 + q] | (hd << 8));
        }
        __syncthreads();                                                      // before the next segment's bytes
    }
}

__global__ __launch_bounds__(256) void bands_rows_kernel(const BdP p) {
    __shared__ unsigned char bytes[BD_SEG + 129 + 3];
    __shared__ unsigned long long masks[BD_NMASK];
    bd_rows(p.label, p.words, p.N, p.H, p.W, p.n_cls, p.ignore_label, p.R, bytes, masks);
}

// D of the pixel whose word is col[0], in a tile of BD_TW words per row with R rows of halo: the dy walk of the head of the file.  v: its byte.
__device__ __forceinline__ unsigned bd_walk(const unsigned short *col, int y, int H, int R, unsigned &v) {
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
    return best;
}

// the number of radii below D: the first k with D <= radii[k], n_bands for the interior
__device__ __forceinline__ unsigned bd_band(unsigned best, const int *radii, int n_bands) {
    unsigned band = 0;
    for (int k = 0; k < n_bands; ++k) band += best > (unsigned)radii[k] ? 1u : 0u;
    return band;
}

// The pixels of a wave tallied by their code (label_bands: (band * n_cls + label) * n_cls + pred): per distinct code of the wave its leading lane adds the
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
                    band = bd_band(bd_walk(tile + (R + ly) * BD_TW + lane, y, H, R, v), p.radii, p.n_bands);
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

struct BiP {
    const long long *label;                             // [N][H][W]
    const int *pred;                                    // [N][H][W]
    const int *group;                                   // [N] (null: every frame is group 0)
    unsigned char *lband, *pband;                       // the band planes of the labels and of the predictions (each may be null)
    unsigned long long *counts;                         // [n_groups][3][n_bands + 1][n_cls] (may be null)
    unsigned short *words;                              // the workspace: [2][N][H][W], the labels' words, then the predictions'
    long long lpitch, lns, ppitch, pns;
    int radii[BD_NBMAX];
    int N, H, W, n_groups, n_cls, n_bands, R, ignore_label, border;
};

__global__ __launch_bounds__(256) void boundary_rows_kernel(const BiP p) {
    __shared__ unsigned char bytes[BD_SEG + 129 + 3];
    __shared__ unsigned long long masks[BD_NMASK];
    if (blockIdx.y == 0)                                                      // uniform over the workgroup
        bd_rows(p.label, p.words, p.N, p.H, p.W, p.n_cls, p.ignore_label, p.R, bytes, masks);
    else                                                                      // no ignore_label: -1 is no byte's value
        bd_rows(p.pred, p.words + (size_t)p.N * (size_t)p.H * (size_t)p.W, p.N, p.H, p.W, p.n_cls, -1, p.R, bytes, masks);
}

// The band of the 64 pixels of column cx of a tile on one plane, lane = row, without the walk.  With bit b of a column's vectors the
// staged row y0 - 64 + b (b in [64 - R, 128 + R); rows outside the halo or the image give no bits), chg(b) "the byte of row b differs from
// that of row b - 1" and c_r(b) "hd of row b <= r": the walk's D is <= r exactly when hd of the pixel is <= r, or going up the nearest
// row b' with chg(b' + 1) or c_r(b') is within r, or going down the nearest b' with chg(b') or c_r(b') is.  (The walk's terms behind the
// first row of another byte are larger than that row's dy, so only the run of the pixel's byte matters; inside it max(dy, hd) <= r is
// dy <= r and hd <= r; the first row of another byte is the nearest chg.)  The three 64-bit ballots per vector play the part the three
// masks play in bd_rows: a pixel's 64 rows above and below are two shifts away.  band = the number of radii with D > r; the border term
// min(D, edge) <= r is D <= r or edge <= r.  v: the pixel's byte.  Every lane of the wave calls.
__device__ __forceinline__ unsigned bi_column(const unsigned short *tile, int cx, int y0, int H, int R, const int *radii, int n_bands, int lane,
                                              unsigned edge, unsigned &v) {
    unsigned w[3];
    bool here[3];
    unsigned long long chg[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const int b = 64 * c + lane, y = y0 - 64 + b;
        here[c] = b >= 64 - R && b < 128 + R && y >= 0 && y < H;
        const unsigned short *at = tile + (b - 64 + R) * BI_PITCH + cx;
        w[c] = here[c] ? (unsigned)at[0] : 0u;
        const bool above = here[c] && b > 64 - R && y > 0;
        const unsigned wa = above ? (unsigned)at[-BI_PITCH] : 0u;
        chg[c] = __ballot(above && (w[c] & 0xffu) != (wa & 0xffu));
    }
    v = w[1] & 0xffu;
    unsigned band = 0;
    for (int k = 0; k < n_bands; ++k) {
        const unsigned r = (unsigned)radii[k];                                // 1 .. 64
        const unsigned long long c0 = __ballot(here[0] && (w[0] >> 8) <= r), c1 = __ballot(here[1] && (w[1] >> 8) <= r),
                                 c2 = __ballot(here[2] && (w[2] >> 8) <= r);
        const unsigned long long u0 = c0 | (chg[0] >> 1) | (chg[1] << 63), u1 = c1 | (chg[1] >> 1) | (chg[2] << 63);      // going up
        const unsigned long long d1 = c1 | chg[1], d2 = c2 | chg[2];                                                    // going down
        // bit 64 - d of lo: the row d above the pixel; bit d - 1 of hi: the row d below it
        const unsigned long long lo = (u0 >> lane) | (lane > 0 ? u1 << (64 - lane) : 0ull);
        const unsigned long long hi = (lane < 63 ? d1 >> (lane + 1) : 0ull) | (d2 << (63 - lane));
        const bool within = (w[1] >> 8) <= r || (lo >> (64u - r)) != 0ull || (hi << (64u - r)) != 0ull || edge <= r;
        band += within ? 0u : 1u;
    }
    return band;
}

__global__ __launch_bounds__(256) void boundary_cols_kernel(const BiP p) {
    extern __shared__ unsigned bd_lds[];                                      // the counters (when a frame can count), the two tiles, the bands
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int H = p.H, W = p.W, R = p.R, n_cls = p.n_cls, nb1 = p.n_bands + 1;
    const int nh = p.counts != nullptr ? 3 * nb1 * n_cls : 0;
    const int rows = BD_TH + 2 * R;
    const bool planes = p.lband != nullptr || p.pband != nullptr;
    unsigned *lh = bd_lds;
    unsigned short *tile_l = reinterpret_cast<unsigned short *>(bd_lds + nh); // [rows][BI_PITCH]: row r is image row y0 - R + r
    unsigned short *tile_p = tile_l + rows * BI_PITCH;
    unsigned char *ob = reinterpret_cast<unsigned char *>(tile_p + rows * BI_PITCH);         // [BD_TH][BI_OPITCH] (with a plane): bg | bp << 4
    const size_t frame = (size_t)H * (size_t)W, plane = (size_t)p.N * frame;
    const int tiles_x = (W + BD_TW - 1) / BD_TW, tiles = tiles_x * ((H + BD_TH - 1) / BD_TH);
    for (int n = blockIdx.y; n < p.N; n += gridDim.y) {
        const int g = p.counts == nullptr ? -1 : (p.group != nullptr ? p.group[n] : 0);
        const bool count = g >= 0 && g < p.n_groups;                          // uniform over the workgroup
        if (!count && !planes) continue;
        if (count) {
            for (int i = tid; i < nh; i += 256) lh[i] = 0u;
            __syncthreads();
        }
        const unsigned short *wl = p.words + (size_t)n * frame, *wp = wl + plane;
        unsigned char *lout = p.lband != nullptr ? p.lband + (size_t)n * (size_t)p.lns : nullptr;
        unsigned char *pout = p.pband != nullptr ? p.pband + (size_t)n * (size_t)p.pns : nullptr;
        for (int t = blockIdx.x; t < tiles; t += gridDim.x) {                 // uniform: every thread makes every pass
            const int x0 = (t % tiles_x) * BD_TW, y0 = (t / tiles_x) * BD_TH;
            for (int r = wave; r < rows; r += 16) {                           // lane = column; four rows a round, their loads in flight together
                const int x = x0 + lane;
                unsigned short a[4], b[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int y = y0 - R + r + 4 * j;
                    const bool in = r + 4 * j < rows && y >= 0 && y < H && x < W;
                    const size_t at = in ? (size_t)y * (size_t)W + x : 0;
                    a[j] = in ? wl[at] : (unsigned short)0;
                    b[j] = in ? wp[at] : (unsigned short)0;
                }
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (r + 4 * j < rows) {                                   // (rows outside the image: zeros that nothing reads)
                        tile_l[(r + 4 * j) * BI_PITCH + lane] = a[j];
                        tile_p[(r + 4 * j) * BI_PITCH + lane] = b[j];
                    }
            }
            __syncthreads();
            for (int cx = wave; cx < BD_TW; cx += 4) {                        // lane = row; uniform: the ballots and bd_tally need every lane
                const int x = x0 + cx, y = y0 + lane;
                const bool inside = x < W && y < H;
                unsigned lv = BD_VOID, pv = BD_VOID, bg = 0, bp = 0;
                if (x < W) {                                                  // uniform over the wave
                    // the smallest r whose window leaves the image (of a pixel inside; the others' is not used)
                    const unsigned edge = p.border ? (unsigned)min(min(x + 1, y + 1), min(W - x, H - y)) : ~0u;
                    bg = bi_column(tile_l, cx, y0, H, R, p.radii, p.n_bands, lane, edge, lv);
                    bp = bi_column(tile_p, cx, y0, H, R, p.radii, p.n_bands, lane, edge, pv);
                    if (planes) ob[lane * BI_OPITCH + cx] = (unsigned char)(bg | bp << 4);    // both at most 8
                }
                if (count) {
                    const bool active = inside && lv != BD_VOID && pv != BD_VOID;
                    const bool hit = active && lv == pv;
                    bd_tally(lh, active ? bg * (unsigned)n_cls + lv : 0u, active, lane);
                    bd_tally(lh, active ? ((unsigned)nb1 + bp) * (unsigned)n_cls + pv : 0u, active, lane);
                    bd_tally(lh, hit ? (2u * (unsigned)nb1 + max(bg, bp)) * (unsigned)n_cls + lv : 0u, hit, lane);
                }
            }
            __syncthreads();
            if (planes) {
                for (int ly = wave; ly < BD_TH; ly += 4) {                    // lane = column again: rows of 64 bytes go out together
                    const int y = y0 + ly, x = x0 + lane;
                    if (y < H && x < W) {
                        const unsigned both = ob[ly * BI_OPITCH + lane];
                        if (lout != nullptr) lout[(size_t)y * (size_t)p.lpitch + x] = (unsigned char)(both & 15u);
                        if (pout != nullptr) pout[(size_t)y * (size_t)p.ppitch + x] = (unsigned char)(both >> 4);
                    }
                }
                __syncthreads();                                              // before the next tile's words and bands
            }
        }
        if (count) {
            __syncthreads();
            unsigned long long *counts = p.counts + (size_t)g * (size_t)nh;
            for (int i = tid; i < nh; i += 256)
                if (lh[i]) atomicAdd(counts + i, (unsigned long long)lh[i]);
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

// 2 words of 16 bits per pixel, rounded up to 16 bytes in all; saturating as arseg_label_bands_workspace_bytes does
extern "C" size_t arseg_boundary_iou_workspace_bytes(int N, int H, int W) {
    if (N <= 0 || H <= 0 || W <= 0 || H > 16384 || W > 16384) return 0;
    const size_t none = ~(size_t)0;
    size_t bytes = 4 * (size_t)H * (size_t)W;
    if (__builtin_mul_overflow(bytes, (size_t)N, &bytes) || bytes > none - 15) return none;
    return (bytes + 15) & ~(size_t)15;
}

extern "C" int arseg_boundary_iou_fwd(const int64_t *label, const int32_t *pred, const int32_t *group, const int *radii, int n_bands, int border,
                                      uint8_t *label_band_out, int64_t label_band_pitch, int64_t label_band_n_stride, uint8_t *pred_band_out,
                                      int64_t pred_band_pitch, int64_t pred_band_n_stride, int64_t *counts, int N, int n_groups, int n_cls,
                                      int H, int W, int ignore_label, void *workspace, size_t workspace_bytes, arseg_stream_t stream) {
    ARSEG_CHECK_PTR(label); ARSEG_CHECK_PTR(pred); ARSEG_CHECK_PTR(workspace); ARSEG_CHECK_PTR(radii);
    ARSEG_CHECK_POS(N); ARSEG_CHECK_POS(H); ARSEG_CHECK_POS(W);
    if (H > 16384 || W > 16384 || n_cls < 1 || n_cls > 32 || n_groups < 1 || n_bands < 1 || n_bands > BD_NBMAX) return ARSEG_EINVAL;
    for (int k = 0; k < n_bands; ++k)
        if (radii[k] < 1 || radii[k] > BI_RMAX || (k > 0 && radii[k] <= radii[k - 1])) return ARSEG_EINVAL;
    if (group == nullptr && n_groups > 1) return ARSEG_EINVAL;
    if (border != 0 && border != 1) return ARSEG_EINVAL;
    if (label_band_out == nullptr && pred_band_out == nullptr && counts == nullptr) return ARSEG_EINVAL;
    if (label_band_out != nullptr && (label_band_pitch < (int64_t)W || label_band_n_stride < 0)) return ARSEG_EINVAL;
    if (pred_band_out != nullptr && (pred_band_pitch < (int64_t)W || pred_band_n_stride < 0)) return ARSEG_EINVAL;
    if ((reinterpret_cast<uintptr_t>(label) & 7u) || (reinterpret_cast<uintptr_t>(counts) & 7u) || (reinterpret_cast<uintptr_t>(pred) & 3u) ||
        (reinterpret_cast<uintptr_t>(group) & 3u) || (reinterpret_cast<uintptr_t>(workspace) & 1u))
        return ARSEG_EINVAL;
    const size_t need = arseg_boundary_iou_workspace_bytes(N, H, W);
    if (need == ~(size_t)0 || workspace_bytes < need) return ARSEG_EWORKSPACE;
    BiP p = {};
    p.label = reinterpret_cast<const long long *>(label); p.pred = pred; p.group = group;
    p.lband = label_band_out; p.pband = pred_band_out; p.counts = reinterpret_cast<unsigned long long *>(counts);
    p.words = static_cast<unsigned short *>(workspace);
    p.lpitch = label_band_pitch; p.lns = label_band_n_stride; p.ppitch = pred_band_pitch; p.pns = pred_band_n_stride;
    for (int k = 0; k < n_bands; ++k) p.radii[k] = radii[k];
    p.N = N; p.H = H; p.W = W; p.n_groups = n_groups; p.n_cls = n_cls; p.n_bands = n_bands; p.R = radii[n_bands - 1];
    p.ignore_label = ignore_label; p.border = border;
    hipStream_t st = arseg_stream(stream);
    const long long segments = (long long)N * H * ((W + BD_SEG - 1) / BD_SEG);
    hipLaunchKernelGGL(boundary_rows_kernel, dim3((unsigned)(segments < 8192 ? segments : 8192), 2), dim3(256), 0, st, p);
    const int gy = N < 65535 ? N : 65535, share = 4096 / gy;
    const int tiles = ((W + BD_TW - 1) / BD_TW) * ((H + BD_TH - 1) / BD_TH);
    const int gx = tiles < share ? tiles : (share < 1 ? 1 : share);
    const size_t lds = (counts != nullptr ? 4 * (size_t)3 * (n_bands + 1) * n_cls : 0) + 2 * 2 * (size_t)(BD_TH + 2 * p.R) * BI_PITCH +
                       (label_band_out != nullptr || pred_band_out != nullptr ? (size_t)BD_TH * BI_OPITCH : 0);                      // <= 58496
    hipLaunchKernelGGL(boundary_cols_kernel, dim3(gx, gy), dim3(256), lds, st, p);
    return arseg_launch_status();
}
