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
//
// The contour F-measure counts (arseg_contour_f_fwd) take the same two byte planes (bd_byte) and the same tiles, groups, wave tally
// (bd_tally) and flush, but their distance is Euclidean and between the planes, so nothing of the row and column passes carries over.
// The scratch is one mark byte per pixel and plane in the caller's workspace ([2][N][H][W]): CF_NONE, or the class of a contour pixel
// with CF_COUNTS where both planes' bytes are classes.  2 launches, sized on the host.
//   marks    contour_marks_kernel: a tile of 64 x 64 pixels with a halo of one, both planes' bytes in LDS (255 outside the image, so
//            the border and void are one rule); the 3 x 3 test is byte compares (cf_mark); rows of 64 marks leave together.
//   match    contour_match_kernel: both planes' marks of the tile with a halo of R = radii[n_bands - 1] in LDS (CF_NONE outside the
//            image; at R = 32 two times 128 x 128 bytes), each plane's contour pixels of the tile compacted into a list with ballots and
//            a count of the lanes below (cf_compact), then a LANE per contour pixel: Chebyshev rings around it on the other plane's
//            marks, inside a ring outwards from the axes so that the first hit is the ring's least (cf_search, which says when it may
//            stop).  Two rounds: the first seeks within CF_R1 rings, where what it finds is final; the pixels it leaves -- the
//            unmatched among them, whose search is the whole disc -- are compacted again, so that long searches fill whole waves
//            instead of holding one up each.  The staging reads the marks four at a time (cf_load4: rows start at any alignment).
//            The band is the number of radii whose square is below m2.  A plane gets 255 in rows of 64 bytes wherever the tile has no
//            contour pixel, and a contour pixel's lane writes its band itself: a tenth of the bytes, and 8 KB of LDS less than staging
//            them, which at R = 19 is a workgroup more per CU.  Counters and flush as above.  50.3 KB of dynamic LDS at most.
// Its loops: the same grid-stride loops; the staging 17 rounds in marks and (64 + 2 R) / 8 rows per half wave in match, R <= 32 checked
// on the host; 16 rows per wave in cf_compact; two rounds of at most 4096 / 256 passes over list entries per plane and tile; rho = 0 .. R
// and t = 0 .. rho in cf_search; n_bands <= 8 compares; cf_dword's 4 bytes; bd_tally of at most 64 rounds.
// Its clamps: a contour pixel's class is a byte below n_cls and its band at most n_bands, so a counter's index is below
// 2 (n_bands + 1) n_cls; a list holds at most the tile's 4096 places; cf_search reads at most R marks from a pixel of the tile in either
// direction, inside the staged halo; cf_dword reads inside the 2 N H W marks only, whatever the row's alignment; marks and planes are
// written inside the image only.
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
constexpr int CF_RMAX = 32;                             // the largest radius of contour_f: a halo of 32 marks round a tile of 64 x 64
constexpr int CF_MPITCH = BD_TW + 4;                    // bytes per staged row of contour_marks_kernel: the tile and a pixel either side
constexpr unsigned CF_NONE = 0x80u;                     // the mark of a pixel that is no contour pixel
constexpr unsigned CF_COUNTS = 0x40u;                   // on a contour pixel's mark (its class, below 32): both planes' bytes are classes here
constexpr int CF_R1 = 2;                                // the rings of the first round of the search
constexpr unsigned CF_CLASS = 0xbfu;                    // a mark without CF_COUNTS: the class of a contour pixel, CF_NONE else

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

struct CfP {
    const long long *label;                             // [N][H][W]
    const int *pred;                                    // [N][H][W]
    const int *group;                                   // [N] (null: every frame is group 0)
    unsigned char *lmatch, *pmatch;                     // the match planes of the labels' and of the predictions' contours (each may be null)
    unsigned long long *counts;                         // [n_groups][2][n_bands + 1][n_cls] (may be null)
    unsigned char *marks;                               // the workspace: [2][N][H][W], the labels' marks, then the predictions'
    long long lpitch, lns, ppitch, pns;
    int radii[BD_NBMAX];
    int N, H, W, n_groups, n_cls, n_bands, R, ignore_label;
};

// The mark of the pixel whose byte is at[0] in a staged tile of CF_MPITCH bytes per row (bytes outside the image staged as 255): its class
// if one of its 8 neighbours holds another class -- a 255 neighbour, void or outside the image, makes no contour --, with CF_COUNTS when
// the other plane's byte at the pixel, ``other``, is a class too; CF_NONE else.
__device__ __forceinline__ unsigned cf_mark(const unsigned char *at, unsigned other) {
    const unsigned c = at[0];
    bool edge = false;
#pragma unroll
    for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
        for (int dx = -1; dx <= 1; ++dx) {
            const unsigned v = at[dy * CF_MPITCH + dx];
            edge |= v != c && v != BD_VOID;
        }
    return c != BD_VOID && edge ? c | (other != BD_VOID ? CF_COUNTS : 0u) : CF_NONE;
}

__global__ __launch_bounds__(256) void contour_marks_kernel(const CfP p) {
    __shared__ unsigned char sb[2][(BD_TH + 2) * CF_MPITCH];                  // row r, column c: the pixel (y0 - 1 + r, x0 - 1 + c)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int H = p.H, W = p.W;
    const size_t frame = (size_t)H * (size_t)W, plane = (size_t)p.N * frame;
    const int tiles_x = (W + BD_TW - 1) / BD_TW, tiles = tiles_x * ((H + BD_TH - 1) / BD_TH);
    for (int n = blockIdx.y; n < p.N; n += gridDim.y) {
        const long long *lab = p.label + (size_t)n * frame;
        const int *prd = p.pred + (size_t)n * frame;
        unsigned char *ml = p.marks + (size_t)n * frame, *mp = ml + plane;
        for (int t = blockIdx.x; t < tiles; t += gridDim.x) {                 // uniform: every thread makes every pass
            const int x0 = (t % tiles_x) * BD_TW, y0 = (t / tiles_x) * BD_TH;
            for (int i = tid; i < (BD_TH + 2) * (BD_TW + 2); i += 256) {
                const int r = i / (BD_TW + 2), c = i - r * (BD_TW + 2);
                const int y = y0 - 1 + r, x = x0 - 1 + c;
                const bool in = y >= 0 && y < H && x >= 0 && x < W;
                const size_t at = in ? (size_t)y * (size_t)W + x : 0;
                sb[0][r * CF_MPITCH + c] = (unsigned char)(in ? bd_byte(lab[at], p.n_cls, p.ignore_label) : BD_VOID);
                sb[1][r * CF_MPITCH + c] = (unsigned char)(in ? bd_byte((long long)prd[at], p.n_cls, -1) : BD_VOID);       // -1 is no byte's value
            }
            __syncthreads();
            for (int ly = wave; ly < BD_TH; ly += 4) {                        // lane = column: rows of 64 marks leave together
                const int y = y0 + ly, x = x0 + lane;
                if (y < H && x < W) {
                    const unsigned char *a = sb[0] + (ly + 1) * CF_MPITCH + lane + 1, *b = sb[1] + (ly + 1) * CF_MPITCH + lane + 1;
                    const size_t at = (size_t)y * (size_t)W + x;
                    ml[at] = (unsigned char)cf_mark(a, b[0]);
                    mp[at] = (unsigned char)cf_mark(b, a[0]);
                }
            }
            __syncthreads();                                                  // before the next tile's bytes
        }
    }
}

// The lanes of a wave that have a place (ly * 64 + lx) to add to a list in LDS: the wave's ballot and a count of the lanes below give a
// lane's slot behind the wave's base, which the leading lane takes off the list's counter.  Every lane of the wave calls.
__device__ __forceinline__ void cf_push(unsigned short *list, unsigned *n_list, bool is, unsigned place, int lane) {
    const unsigned long long m = __ballot(is);
    unsigned base = 0;
    if (lane == 0 && m) base = atomicAdd(n_list, (unsigned)__builtin_popcountll(m));
    base = (unsigned)__shfl((int)base, 0, 64);
    if (is) list[base + (unsigned)__builtin_popcountll(m & ((1ull << lane) - 1ull))] = (unsigned short)place;
}

// The contour pixels of one plane of the tile, compacted: list[0 .. *n_list) their places, in any order.  A wave takes a row of the tile at
// a time; ``mine`` is the tile's own part of the staged marks (pitch P).  Every thread of the workgroup calls.
__device__ __forceinline__ void cf_compact(const unsigned char *mine, int P, unsigned short *list, unsigned *n_list, int lane, int wave) {
    for (int ly = wave; ly < BD_TH; ly += 4) cf_push(list, n_list, mine[ly * P + lane] != CF_NONE, (unsigned)(ly * BD_TW + lane), lane);
}

// m2 of the contour pixel of class c at ``at`` against the other plane's staged marks (pitch P, a halo of at least R marks on every side,
// CF_NONE outside the image), as far as the band needs it: R * R + 1 for "none within R".  Chebyshev rings rho = 0, 1, ...: the marks of
// ring rho are at (+-rho, +-t) and (+-t, +-rho), t = 0 .. rho, squared distance rho^2 + t^2, so within a ring t ascends and the first hit
// is the ring's least.  A ring can improve on the best only while rho^2 < best -- not merely until the first ring with a hit: (5, 5) is in
// ring 5 at 50, (0, 6) in ring 6 at 36 --, and nothing below radii[0]^2 changes the band: a HIT within radii[0] ends the search ("none
// within R" is no hit, whatever radii[0] is: R may be the first round's few rings, below radii[0]).
__device__ __forceinline__ unsigned cf_search(const unsigned char *at, int P, unsigned c, int R, unsigned r0sq) {
    unsigned best = (unsigned)(R * R) + 1u;
    const unsigned enough = min(r0sq, (unsigned)(R * R));
    for (int rho = 0; rho <= R && (unsigned)(rho * rho) < best && best > enough; ++rho) {
        const unsigned char *up = at - rho * P, *dn = at + rho * P;
        for (int t = 0; t <= rho; ++t) {
            const unsigned d2 = (unsigned)(rho * rho + t * t);
            if (d2 >= best) break;
            const int tp = t * P;
            const unsigned a0 = up[t], a1 = up[-t], a2 = dn[t], a3 = dn[-t], a4 = at[tp - rho], a5 = at[-tp - rho], a6 = at[tp + rho], a7 = at[-tp + rho];
            const bool hit = (a0 & CF_CLASS) == c | (a1 & CF_CLASS) == c | (a2 & CF_CLASS) == c | (a3 & CF_CLASS) == c | (a4 & CF_CLASS) == c |
                             (a5 & CF_CLASS) == c | (a6 & CF_CLASS) == c | (a7 & CF_CLASS) == c;
            if (hit) {
                best = d2;
                break;
            }
        }
    }
    return best;
}

// The same m2 for the long searches of the second round, by rows: the pixel's own row of the other plane's marks, then the rows dy = 1, 2, ...
// above and below it while dy^2 < best, in each the columns within w of the pixel's, w the largest with dy^2 + w^2 < best -- inside the
// disc of R, and shrinking with every hit.  Four marks per aligned 32-bit LDS read: with the class in every byte XORed in, a mark of
// the class is a zero byte (the usual test), and a word with one is looked at byte by byte.  The bytes a word holds beyond w are marks
// too, at their true distance, and the minimum may take them.  ``row`` is the pixel's staged row of the other plane (its first byte,
// 4-byte aligned, pitch P a multiple of 4), ``cx`` its column there: cx - w >= 0 and cx + w < P for every w <= R.
__device__ __forceinline__ unsigned cf_scan(const unsigned char *row, int cx, int P, unsigned c, int R, unsigned r0sq) {
    unsigned best = (unsigned)(R * R) + 1u;
    const unsigned cw = c * 0x01010101u;
    int w = R;
    for (int dy = 0; dy <= R && (unsigned)(dy * dy) < best && best > r0sq; ++dy) {
        const int lim = (int)best - 1 - dy * dy;                              // >= 0: dx^2 may be at most this
        while (w * w > lim) --w;                                              // (w only ever shrinks: at most R steps in all)
        const int c0 = (cx - w) & ~3, c1 = cx + w;
        for (int side = dy == 0 ? 1 : 0; side < 2; ++side) {
            const unsigned char *r = side ? row + dy * P : row - dy * P;
            for (int col = c0; col <= c1; col += 4) {
                const unsigned v = (*reinterpret_cast<const unsigned *>(r + col) & (CF_CLASS * 0x01010101u)) ^ cw;
                if (((v - 0x01010101u) & ~v & 0x80808080u) == 0u) continue;   // no byte of v is zero
#pragma unroll
                for (int b = 0; b < 4; ++b)
                    if (((v >> (8 * b)) & 0xffu) == 0u) best = min(best, (unsigned)(dy * dy + (col + b - cx) * (col + b - cx)));
            }
        }
    }
    return best;
}

// Four bytes of the marks from the 4-byte aligned element ``a`` on (``total`` bytes in all): one 32-bit load where all four are inside, else
// byte by byte, zeros outside.
__device__ __forceinline__ unsigned cf_dword(const unsigned char *marks, long long a, long long total) {
    if (a >= 0 && a + 4 <= total) return *reinterpret_cast<const unsigned *>(marks + a);
    unsigned w = 0;
#pragma unroll
    for (int b = 0; b < 4; ++b)
        if (a + b >= 0 && a + b < total) w |= (unsigned)marks[a + b] << (8 * b);
    return w;
}

// The four marks from element e on, however e is aligned (rows start anywhere: W and R are any): the two aligned words around them, shifted.
__device__ __forceinline__ unsigned cf_load4(const unsigned char *marks, long long e, long long total) {
    const unsigned s = (unsigned)((reinterpret_cast<uintptr_t>(marks) + (uintptr_t)e) & 3u);
    const long long a = e - (long long)s;
    const unsigned lo = cf_dword(marks, a, total), hi = s ? cf_dword(marks, a + 4, total) : 0u;
    return (unsigned)(((unsigned long long)hi << 32 | lo) >> (8u * s));
}

// the number of radii whose square is below m2: the first k with m2 <= radii[k]^2, n_bands for unmatched
__device__ __forceinline__ unsigned cf_band(unsigned m2, const int *radii, int n_bands) {
    unsigned band = 0;
    for (int k = 0; k < n_bands; ++k) band += m2 > (unsigned)(radii[k] * radii[k]) ? 1u : 0u;
    return band;
}

__global__ __launch_bounds__(256) void contour_match_kernel(const CfP p) {
    extern __shared__ unsigned bd_lds[];                                      // the counters (when a frame can count), the two tiles, the lists
    __shared__ unsigned n_list[4];                                            // per plane: the contour pixels, those left to the second round
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int H = p.H, W = p.W, R = p.R, n_cls = p.n_cls, nb1 = p.n_bands + 1;
    const int nh = p.counts != nullptr ? 2 * nb1 * n_cls : 0;
    const int rows = BD_TH + 2 * R, P = (BD_TW + 2 * R + 3) & ~3;             // a staged plane: row r, column c is the pixel (y0 - R + r, x0 - R + c)
    const int R1 = R < CF_R1 ? R : CF_R1;
    const bool planes = p.lmatch != nullptr || p.pmatch != nullptr;
    unsigned *lh = bd_lds;
    unsigned char *tile = reinterpret_cast<unsigned char *>(bd_lds + nh);     // [2][rows][P]
    unsigned short *list = reinterpret_cast<unsigned short *>(tile + 2 * rows * P);          // [BD_TH * BD_TW]: the plane's contour pixels
    unsigned short *later = list + BD_TH * BD_TW;                             // [BD_TH * BD_TW]: those the first round leaves
    const unsigned r0sq = (unsigned)(p.radii[0] * p.radii[0]);
    const size_t frame = (size_t)H * (size_t)W, plane = (size_t)p.N * frame;
    const long long total = 2ll * (long long)plane;
    const int tiles_x = (W + BD_TW - 1) / BD_TW, tiles = tiles_x * ((H + BD_TH - 1) / BD_TH);
    for (int n = blockIdx.y; n < p.N; n += gridDim.y) {
        const int g = p.counts == nullptr ? -1 : (p.group != nullptr ? p.group[n] : 0);
        const bool count = g >= 0 && g < p.n_groups;                          // uniform over the workgroup
        if (!count && !planes) continue;
        if (count) {
            for (int i = tid; i < nh; i += 256) lh[i] = 0u;
            __syncthreads();
        }
        unsigned char *lout = p.lmatch != nullptr ? p.lmatch + (size_t)n * (size_t)p.lns : nullptr;
        unsigned char *pout = p.pmatch != nullptr ? p.pmatch + (size_t)n * (size_t)p.pns : nullptr;
        for (int t = blockIdx.x; t < tiles; t += gridDim.x) {                 // uniform: every thread makes every pass
            const int x0 = (t % tiles_x) * BD_TW, y0 = (t / tiles_x) * BD_TH;
            if (tid < 4) n_list[tid] = 0u;
            // half a wave per staged row, four marks per lane: lane j of the half takes the columns 4 j .. 4 j + 3
            for (int r = 2 * wave + (lane >> 5); r < rows; r += 8) {
                const int j = lane & 31, y = y0 - R + r, x = x0 - R + 4 * j;
                if (4 * j >= P) continue;
                unsigned keep = 0;                                            // 0xff per column inside the image
#pragma unroll
                for (int b = 0; b < 4; ++b) keep |= y >= 0 && y < H && x + b >= 0 && x + b < W ? 0xffu << (8 * b) : 0u;
                unsigned wl = 0, wp = 0;
                if (keep) {
                    const long long e = (long long)((size_t)n * frame) + (long long)y * W + x;
                    wl = cf_load4(p.marks, e, total);
                    wp = cf_load4(p.marks, (long long)plane + e, total);
                }
                const unsigned none = (CF_NONE * 0x01010101u) & ~keep;
                *reinterpret_cast<unsigned *>(tile + r * P + 4 * j) = (wl & keep) | none;
                *reinterpret_cast<unsigned *>(tile + (rows + r) * P + 4 * j) = (wp & keep) | none;
            }
            __syncthreads();
            if (planes)                                                       // 255 where there is no contour pixel; those get their band below
                for (int ly = wave; ly < BD_TH; ly += 4) {                    // lane = column: rows of 64 bytes go out together
                    const int y = y0 + ly, x = x0 + lane;
                    if (y < H && x < W) {
                        if (lout != nullptr && tile[(R + ly) * P + R + lane] == CF_NONE) lout[(size_t)y * (size_t)p.lpitch + x] = (unsigned char)BD_VOID;
                        if (pout != nullptr && tile[(rows + R + ly) * P + R + lane] == CF_NONE) pout[(size_t)y * (size_t)p.ppitch + x] = (unsigned char)BD_VOID;
                    }
                }
#pragma unroll
            for (int s = 0; s < 2; ++s) {                                     // a lane per contour pixel of plane s, sought on the other plane
                const unsigned char *mine = tile + (s * rows + R) * P + R, *theirs = tile + ((1 - s) * rows + R) * P + R;
                unsigned char *out = s == 0 ? lout : pout;
                const size_t opitch = (size_t)(s == 0 ? p.lpitch : p.ppitch);
                cf_compact(mine, P, list, n_list + 2 * s, lane, wave);
                __syncthreads();
                // Two rounds.  The first seeks within R1 rings only; what it finds there is final (every later ring is farther), and most
                // contour pixels of a fair prediction end here.  The others -- a few per wave, unmatched ones among them, whose search is
                // the whole disc -- are compacted again, so that the long searches fill whole waves instead of holding one up each, and
                // are sought by rows, four marks a read (cf_scan).
                for (int round = 0; round < 2; ++round) {
                    const unsigned short *from = round == 0 ? list : later;
                    const int n_from = (int)n_list[2 * s + round], reach = round == 0 ? R1 : R;
                    for (int base = 64 * wave; base < n_from; base += 256) {  // uniform over the wave: the ballots and bd_tally need every lane
                        const bool have = base + lane < n_from;
                        unsigned band = 0, c = 0, at = 0;
                        bool done = false, counts = false;
                        if (have) {
                            at = from[base + lane];
                            const int ly = (int)(at >> 6), lx = (int)(at & 63u);
                            const unsigned m = mine[ly * P + lx];
                            c = m & 31u;
                            counts = (m & CF_COUNTS) != 0u;
                            const unsigned m2 = round == 0 ? cf_search(theirs + ly * P + lx, P, c, reach, r0sq)
                                                           : cf_scan(theirs + ly * P - R, R + lx, P, c, R, r0sq);
                            done = reach == R || m2 <= (unsigned)(reach * reach);
                            band = cf_band(m2, p.radii, p.n_bands);
                            if (done && out != nullptr) out[(size_t)(y0 + ly) * opitch + (size_t)(x0 + lx)] = (unsigned char)band;
                        }
                        if (round == 0 && R1 < R) cf_push(later, n_list + 2 * s + 1, have && !done, at, lane);
                        if (count) {
                            const bool active = done && counts;
                            bd_tally(lh, active ? ((unsigned)(s * nb1) + band) * (unsigned)n_cls + c : 0u, active, lane);
                        }
                    }
                    __syncthreads();                                          // the second round's list is complete; then: before the next plane's lists
                }
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

// a mark per pixel and plane, 2 N H W bytes rounded up to 16 in all; saturating as arseg_label_bands_workspace_bytes does
extern "C" size_t arseg_contour_f_workspace_bytes(int N, int H, int W) {
    if (N <= 0 || H <= 0 || W <= 0 || H > 16384 || W > 16384) return 0;
    const size_t none = ~(size_t)0;
    size_t bytes = 2 * (size_t)H * (size_t)W;
    if (__builtin_mul_overflow(bytes, (size_t)N, &bytes) || bytes > none - 15) return none;
    return (bytes + 15) & ~(size_t)15;
}

extern "C" int arseg_contour_f_fwd(const int64_t *label, const int32_t *pred, const int32_t *group, const int *radii, int n_bands,
                                   uint8_t *label_match_out, int64_t label_match_pitch, int64_t label_match_n_stride, uint8_t *pred_match_out,
                                   int64_t pred_match_pitch, int64_t pred_match_n_stride, int64_t *counts, int N, int n_groups, int n_cls, int H,
                                   int W, int ignore_label, void *workspace, size_t workspace_bytes, arseg_stream_t stream) {
    ARSEG_CHECK_PTR(label); ARSEG_CHECK_PTR(pred); ARSEG_CHECK_PTR(workspace); ARSEG_CHECK_PTR(radii);
    ARSEG_CHECK_POS(N); ARSEG_CHECK_POS(H); ARSEG_CHECK_POS(W);
    if (H > 16384 || W > 16384 || n_cls < 1 || n_cls > 32 || n_groups < 1 || n_bands < 1 || n_bands > BD_NBMAX) return ARSEG_EINVAL;
    for (int k = 0; k < n_bands; ++k)
        if (radii[k] < 0 || radii[k] > CF_RMAX || (k > 0 && radii[k] <= radii[k - 1])) return ARSEG_EINVAL;
    if (group == nullptr && n_groups > 1) return ARSEG_EINVAL;
    if (label_match_out == nullptr && pred_match_out == nullptr && counts == nullptr) return ARSEG_EINVAL;
    if (label_match_out != nullptr && (label_match_pitch < (int64_t)W || label_match_n_stride < 0)) return ARSEG_EINVAL;
    if (pred_match_out != nullptr && (pred_match_pitch < (int64_t)W || pred_match_n_stride < 0)) return ARSEG_EINVAL;
    if ((reinterpret_cast<uintptr_t>(label) & 7u) || (reinterpret_cast<uintptr_t>(counts) & 7u) || (reinterpret_cast<uintptr_t>(pred) & 3u) ||
        (reinterpret_cast<uintptr_t>(group) & 3u) || (reinterpret_cast<uintptr_t>(workspace) & 1u))
        return ARSEG_EINVAL;
    const size_t need = arseg_contour_f_workspace_bytes(N, H, W);
    if (need == ~(size_t)0 || workspace_bytes < need) return ARSEG_EWORKSPACE;
    CfP p = {};
    p.label = reinterpret_cast<const long long *>(label); p.pred = pred; p.group = group;
    p.lmatch = label_match_out; p.pmatch = pred_match_out; p.counts = reinterpret_cast<unsigned long long *>(counts);
    p.marks = static_cast<unsigned char *>(workspace);
    p.lpitch = label_match_pitch; p.lns = label_match_n_stride; p.ppitch = pred_match_pitch; p.pns = pred_match_n_stride;
    for (int k = 0; k < n_bands; ++k) p.radii[k] = radii[k];
    p.N = N; p.H = H; p.W = W; p.n_groups = n_groups; p.n_cls = n_cls; p.n_bands = n_bands; p.R = radii[n_bands - 1];
    p.ignore_label = ignore_label;
    hipStream_t st = arseg_stream(stream);
    const int gy = N < 65535 ? N : 65535, share = 4096 / gy;
    const int tiles = ((W + BD_TW - 1) / BD_TW) * ((H + BD_TH - 1) / BD_TH);
    const int gx = tiles < share ? tiles : (share < 1 ? 1 : share);
    hipLaunchKernelGGL(contour_marks_kernel, dim3(gx, gy), dim3(256), 0, st, p);
    const size_t side = (size_t)(BD_TW + 2 * p.R), pitch = (side + 3) & ~(size_t)3;
    const size_t lds = (counts != nullptr ? 4 * (size_t)2 * (n_bands + 1) * n_cls : 0) + 2 * side * pitch + 2 * 2 * (size_t)BD_TH * BD_TW;         // <= 51456
    hipLaunchKernelGGL(contour_match_kernel, dim3(gx, gy), dim3(256), lds, st, p);
    return arseg_launch_status();
}
