// Row-run codes of 8-bit label planes (include/arseg_hip.h, arseg_labels_rle_fwd / arseg_rle_decode_fwd): uint8 [N][H][W] planes in, per frame
// the exclusive prefix of the rows' run counts (row_start, int32 [N][H+1]) and the runs in (y, x) order as words (x_first << 8) | value out;
// and the inverse.  The first kernels of the output half that count, scan and compact instead of mapping pixels.
//
// Encoder: three launches, no workgroup waits for another one (no look-back, no flags): the plane is read twice, and the second pass finds a
// 1 byte / pixel plane in L2 / Infinity Cache.
//   count  a wave owns a row (grid-stride over the rows, blockIdx.y strides over the frames).  A lane takes 16 pixels of the row: 16 bytes
//          packed in 4 dwords plus the byte to their left; the start mask of the piece is the non-zero bytes of (piece ^ piece shifted by
//          one byte), found on the packed dwords.  popcount per lane, one reduction per row, lane 0 stores the row's count to
//          row_start[n][y + 1].
//   scan   one workgroup per frame: row_start[n][1 .. H] -> its inclusive prefix in place, 256 entries at a time with a carry, and
//          row_start[n][0] = 0.
//   emit   the walk of count; a wave-exclusive scan of the lanes' counts (skipped for a pass without a start) on top of the wave's running
//          base, which begins at row_start[n][y]; a lane writes the words of its piece whose index is < cap.
// Decoder: a wave per row; a lane takes the runs row_start[n][y] + lane, + 64, ..., reads its word and the next one of the same row (or W) and
// fills [x_first, x_next): bytes up to a 4-byte boundary, dwords up to a 16-byte boundary, 16-byte stores, dwords, bytes.
#include "runcode.h"

namespace {

typedef unsigned u32x4_a4 __attribute__((ext_vector_type(4), aligned(4)));

constexpr int RLE_PIECE = 16;                           // pixels per lane and pass
constexpr int RLE_WAVES = 4;                            // waves (= rows in flight) per workgroup

struct RleP {
    const uint8_t *lab;                                 // encoder: the planes
    uint8_t *out;                                       // decoder: the planes
    int *rs;                                            // [N][H + 1]
    unsigned *runs;                                     // [N][cap] (encoder: may be null)
    long long pitch, ns;                                // bytes per row / per image
    long long cap_stride;                               // words from frame to frame of runs
    int cap;                                            // min(cap, INT32_MAX): an index is below 2^31
    int N, H, W;
};

// cnt (1 .. 16) pixels from g, packed: byte b of d[q] is pixel 4 q + b; the bytes from cnt on are zero.  Exactly the cnt bytes are read, with
// the widest loads the address allows (span_load's rule: 16 bytes on a 4-byte aligned address, 2 bytes on an even one, single bytes otherwise).
__device__ __forceinline__ void rle_piece(const uint8_t *g, int cnt, unsigned (&d)[4]) {
    const unsigned al = (unsigned)reinterpret_cast<uintptr_t>(g);
    if (cnt == RLE_PIECE && !(al & 3u)) {
        const u32x4_a4 x = *reinterpret_cast<const u32x4_a4 *>(g);
        d[0] = x.x; d[1] = x.y; d[2] = x.z; d[3] = x.w;
    } else if (cnt == RLE_PIECE && !(al & 1u)) {
#pragma unroll
        for (int q = 0; q < 4; ++q)
            d[q] = (unsigned)*reinterpret_cast<const uint16_t *>(g + 4 * q) | ((unsigned)*reinterpret_cast<const uint16_t *>(g + 4 * q + 2) << 16);
    } else {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            unsigned x = 0;
#pragma unroll
            for (int b = 0; b < 4; ++b)
                if (4 * q + b < cnt) x |= (unsigned)g[4 * q + b] << (8 * b);
            d[q] = x;
        }
    }
}

// bit b of the result = byte b of v is not zero
__device__ __forceinline__ unsigned rle_nonzero_bytes(unsigned v) {
    const unsigned t = (((v & 0x7f7f7f7fu) + 0x7f7f7f7fu) | v) & 0x80808080u;          // bit 7 of every non-zero byte
    return ((t >> 7) * 0x01020408u) >> 24;          // bits 0, 8, 16, 24 -> 24 .. 27: the 10 partial products fall on distinct bits (no carries)
}

// The 16-bit start mask of the piece of pixels [x, x + cnt) of a row: bit b = a run begins at x + b
__device__ __forceinline__ unsigned rle_starts(const uint8_t *row, int x, int cnt, unsigned (&d)[4]) {
    rle_piece(row + x, cnt, d);
    const unsigned left = x > 0 ? (unsigned)row[x - 1] : (~d[0] & 0xffu);               // x == 0 always begins a run
    unsigned m = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const unsigned sh = (d[q] << 8) | (q ? d[q - 1] >> 24 : left);
        m |= rle_nonzero_bytes(d[q] ^ sh) << (4 * q);
    }
    return m & (0xffffu >> (RLE_PIECE - cnt));
}

template <bool EMIT>
__global__ __launch_bounds__(64 * RLE_WAVES) void rle_encode_kernel(const RleP p) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int n = blockIdx.y; n < p.N; n += gridDim.y) {
        int *rs = p.rs + (size_t)n * (p.H + 1);
        unsigned *runs = EMIT ? p.runs + (size_t)n * p.cap_stride : nullptr;
        for (int y = blockIdx.x * RLE_WAVES + wave; y < p.H; y += gridDim.x * RLE_WAVES) {
            const uint8_t *row = p.lab + (size_t)n * p.ns + (size_t)y * p.pitch;
            int base = EMIT ? rs[y] : 0;
            int count = 0;
            for (int x0 = 0; x0 < p.W; x0 += 64 * RLE_PIECE) {          // x0 is wave uniform: every lane makes every pass
                const int x = x0 + lane * RLE_PIECE, cnt = min(p.W - x, RLE_PIECE);
                unsigned d[4] = {0, 0, 0, 0}, m = 0;
                if (cnt > 0) m = rle_starts(row, x, cnt, d);
                const int c = __popc(m);
                if constexpr (!EMIT) {
                    count += c;
                } else {
                    if (__ballot(c != 0) == 0ull) continue;          // a pass inside one run: nothing to write, the base stays
                    int inc = c;
#pragma unroll
                    for (int o = 1; o < 64; o <<= 1) {
                        const int t = __shfl_up(inc, o, 64);
                        inc += lane >= o ? t : 0;
                    }
                    int idx = base + inc - c;
                    base += __shfl(inc, 63, 64);
                    const unsigned long long lo = d[0] | ((unsigned long long)d[1] << 32), hi = d[2] | ((unsigned long long)d[3] << 32);
                    while (m) {
                        const int b = __ffs(m) - 1;
                        m &= m - 1;
                        const unsigned v = (unsigned)((b < 8 ? lo : hi) >> (8 * (b & 7))) & 0xffu;
                        if (idx >= 0 && idx < p.cap) runs[idx] = ((unsigned)(x + b) << 8) | v;
                        ++idx;
                    }
                }
            }
            if constexpr (!EMIT) {
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) count += __shfl_xor(count, o, 64);
                if (lane == 0) rs[y + 1] = count;
            }
        }
    }
}

// row_start[n][1 .. H]: counts -> their inclusive prefix, in place; row_start[n][0] = 0
__global__ __launch_bounds__(256) void rle_scan_kernel(const RleP p) {
    __shared__ int part[4];
    for (int n = blockIdx.x; n < p.N; n += gridDim.x) {
        int *rs = p.rs + (size_t)n * (p.H + 1);
        int carry = 0;
        for (int i0 = 1; i0 <= p.H; i0 += 256) {
            const int i = i0 + (int)threadIdx.x;
            int inc = i <= p.H ? rs[i] : 0;
            rc_block_scan<1>(&inc, &carry, part);
            if (i <= p.H) rs[i] = inc;
        }
        if (threadIdx.x == 0) rs[0] = 0;
    }
}

// len bytes of value v (v4 = v in every byte) from g on: exactly those bytes, with the widest stores the address allows
__device__ __forceinline__ void rle_fill(uint8_t *g, int len, unsigned v4) {
    uint8_t *const end = g + len;
    while (g < end && ((unsigned)reinterpret_cast<uintptr_t>(g) & 3u)) *g++ = (uint8_t)v4;
    while (end - g >= 4 && ((unsigned)reinterpret_cast<uintptr_t>(g) & 15u)) { *reinterpret_cast<unsigned *>(g) = v4; g += 4; }
    while (end - g >= 16) { *reinterpret_cast<u32x4 *>(g) = u32x4{v4, v4, v4, v4}; g += 16; }
    while (end - g >= 4) { *reinterpret_cast<unsigned *>(g) = v4; g += 4; }
    while (g < end) *g++ = (uint8_t)v4;
}

__global__ __launch_bounds__(64 * RLE_WAVES) void rle_decode_kernel(const RleP p) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int n = blockIdx.y; n < p.N; n += gridDim.y) {
        const int *rs = p.rs + (size_t)n * (p.H + 1);
        const unsigned *runs = p.runs + (size_t)n * p.cap_stride;
        for (int y = blockIdx.x * RLE_WAVES + wave; y < p.H; y += gridDim.x * RLE_WAVES) {
            uint8_t *row = p.out + (size_t)n * p.ns + (size_t)y * p.pitch;
            const int first = max(rs[y], 0), last = rs[y + 1];           // a malformed row_start may not lead outside runs[n][0 .. cap)
            const int stored = min(last, p.cap);
            for (int i = first + lane; i < stored; i += 64) {
                const unsigned word = runs[i];
                const int xa = rc_x0(runs, i, p.W);
                // the run ends where the next one of its row begins, or at W; a stored run whose successor in the row was cut off by cap
                // is known to hold its first pixel only
                const int xb = i + 1 >= last ? p.W : (i + 1 < p.cap ? (int)(runs[i + 1] >> 8) : xa + 1);
                const int len = min(xb, p.W) - xa;
                if (len > 0) rle_fill(row + xa, len, (word & 0xffu) * 0x01010101u);
            }
        }
    }
}

// what the two entry points share: the plane, row_start, runs and cap
int rle_common(RleP &p, const void *plane, int64_t pitch, int64_t image_stride, int N, int H, int W, const int32_t *row_start, const uint32_t *runs,
               int64_t cap) {
    ARSEG_CHECK_PTR(plane); ARSEG_CHECK_PTR(row_start);
    ARSEG_CHECK_POS(N); ARSEG_CHECK_POS(H); ARSEG_CHECK_POS(W);
    if (rc_misaligned(4, row_start, runs)) return ARSEG_EINVAL;
    if (runs && cap < 0) return ARSEG_EINVAL;
    if (pitch < (int64_t)W || image_stride < 0) return ARSEG_EINVAL;
    if (W > (1 << 24) || (int64_t)H * W > (int64_t)INT32_MAX) return ARSEG_EINVAL;
    p.rs = const_cast<int *>(row_start); p.runs = const_cast<unsigned *>(runs);
    p.pitch = pitch; p.ns = image_stride;
    p.cap_stride = runs ? cap : 0;
    p.cap = runs ? rc_cap(cap) : 0;
    p.N = N; p.H = H; p.W = W;
    return ARSEG_OK;
}

}  // namespace

extern "C" int arseg_labels_rle_fwd(const uint8_t *labels, int64_t pitch, int64_t image_stride, int N, int H, int W, int32_t *row_start,
                                    uint32_t *runs, int64_t cap, arseg_stream_t stream) {
    RleP p = {};
    const int rc = rle_common(p, labels, pitch, image_stride, N, H, W, row_start, runs, cap);
    if (rc != ARSEG_OK) return rc;
    p.lab = labels;
    hipStream_t st = arseg_stream(stream);
    const dim3 g = rc_grid(N, H, RLE_WAVES, 16384);
    hipLaunchKernelGGL((rle_encode_kernel<false>), g, dim3(64 * RLE_WAVES), 0, st, p);
    hipLaunchKernelGGL(rle_scan_kernel, rc_frames(N), dim3(256), 0, st, p);
    if (runs && p.cap > 0) hipLaunchKernelGGL((rle_encode_kernel<true>), g, dim3(64 * RLE_WAVES), 0, st, p);
    return arseg_launch_status();
}

extern "C" int arseg_rle_decode_fwd(const int32_t *row_start, const uint32_t *runs, int64_t cap, int N, int H, int W, uint8_t *labels_out,
                                    int64_t pitch, int64_t image_stride, arseg_stream_t stream) {
    ARSEG_CHECK_PTR(runs);
    RleP p = {};
    const int rc = rle_common(p, labels_out, pitch, image_stride, N, H, W, row_start, runs, cap);
    if (rc != ARSEG_OK) return rc;
    p.out = labels_out;
    if (p.cap == 0) return ARSEG_OK;          // no run is stored: every pixel stays
    hipLaunchKernelGGL(rle_decode_kernel, rc_grid(N, H, RLE_WAVES, 16384), dim3(64 * RLE_WAVES), 0, arseg_stream(stream), p);
    return arseg_launch_status();
}
