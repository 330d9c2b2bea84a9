// luma8 of the five source formats as the block search defines it (include/arseg_hip.h, arseg_block_motion_fwd): shared by the full search
// (block_motion.hip), which converts while it stages its windows, and by the luma pyramid (block_motion_pyr.hip), which converts once.
#pragma once
#include "arseg_device.h"

constexpr int BM_MAX_DIM = 8192, BM_MAX_R = 32;
enum { BM_U8 = 0, BM_P010 = 1, BM_I010 = 2, BM_RGB8 = 3 };             // how a sample becomes luma8

template <int F> constexpr int bm_sample_bytes = F == BM_U8 ? 1 : (F == BM_RGB8 ? 3 : 2);

// luma8 of the sample whose bytes are s[0 ..]
template <int F>
__device__ __forceinline__ unsigned bm_luma8(const unsigned *s) {
    if constexpr (F == BM_U8) return s[0];
    else if constexpr (F == BM_P010) return s[1];                                         // v >> 8
    else if constexpr (F == BM_I010) return ((s[0] | (s[1] << 8)) & 0x3ffu) >> 2;
    else return (77u * s[0] + 150u * s[1] + 29u * s[2] + 128u) >> 8;
}

// luma8 of pixels x .. x + 3 of one frame row, packed little endian; a pixel outside [0, W) reads 0.  row = the row's first byte.
template <int F>
__device__ __forceinline__ unsigned bm_luma4(const uint8_t *row, int x, int W) {
    constexpr int S = bm_sample_bytes<F>;
    unsigned out = 0;
    if (x >= 0 && x + 4 <= W) {
        unsigned v[4 * S];
        span_load<4 * S>(row + (size_t)x * S, v);
#pragma unroll
        for (int i = 0; i < 4; ++i) out |= bm_luma8<F>(v + i * S) << (8 * i);
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            if (x + i < 0 || x + i >= W) continue;
            unsigned v[S];
#pragma unroll
            for (int b = 0; b < S; ++b) v[b] = row[(size_t)(x + i) * S + b];
            out |= bm_luma8<F>(v) << (8 * i);
        }
    }
    return out;
}

static inline int bm_format(int src_format) {
    switch (src_format) {
    case ARSEG_SRC_NV12: case ARSEG_SRC_I420: return BM_U8;
    case ARSEG_SRC_P010: return BM_P010;
    case ARSEG_SRC_I010: return BM_I010;
    case ARSEG_SRC_RGB8: return BM_RGB8;
    default: return -1;
    }
}

// what a plane of format f (bm_format) must satisfy: bytes per sample and the alignment of its pitch and base
static inline bool bm_plane_ok(int f, const void *plane, int64_t pitch, int W) {
    const int64_t sample = f == BM_U8 ? 1 : (f == BM_RGB8 ? 3 : 2), align = f == BM_P010 || f == BM_I010 ? 2 : 1;
    return pitch >= sample * W && pitch % align == 0 && reinterpret_cast<uintptr_t>(plane) % align == 0;
}
