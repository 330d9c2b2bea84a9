// Calibration counts (include/arseg_hip.h, arseg_calibration_fwd): head logits and ground-truth labels in, the reliability table out -- per
// group of frames (keyframe distance), predicted class k* and 8-bit confidence code q how many counting pixels there were and how many of
// them were right -- in one launch for N frames and one pass over the logits.  Class and code are the confidence launch's: the bilinear
// resize and the argmax are the one label rule (arseg_label_pixel / arseg_label_run, arseg_device.h) and the softmax rides on its class loop
// as ArsegSoftmaxAcc, whose code() gives q; nothing of either is restated here, so (k*, q) is bit-equal to labels8 / conf8 of
// arseg_segment_confidence_fwd on all three routes.
//
// Thread mapping: confidence.hip's -- one pixel (per-pixel routes) or one run of S pixels (run route) of one row of one frame, blockIdx.y
// strides over the frames, the tail's caps on the launch.  A workgroup's LDS table therefore belongs to one group at a time.
//
// The table in LDS: one 32-bit word per (k*, q), n_cls x 256 words (19 KB at 19 classes, 32 KB at 32): the low half counts the pixels, the
// high half the right ones, so one LDS add serves both columns of cal.  A half holds 65535: a workgroup flushes at the end of a frame and
// after every CAL_FLUSH_PIXELS / (256 S) trips of its grid-stride loop, whichever comes first (the trip count is uniform over the
// workgroup, so the barriers of a flush inside the loop are too).
//
// The hot bin: on real logits most pixels of a wave are (k*, 255, right) with one k*, and 64 LDS adds on one address serialise.  A lane
// first adds up its own stretches of equal keys in registers (run route: conf_emit's "one add per stretch"), then the wave peels
// CAL_PEEL keys: the first active lane's key is broadcast, the lanes that hold it are balloted and summed (a popcount where every lane
// holds one pixel), their leader issues ONE LDS add, and they drop out.  Two rounds take a saturated wave -- with or without an outlier in
// its first lane -- and a two-class edge down to two adds; whatever is left (spread codes: mostly distinct addresses, which LDS serves
// side by side) adds for itself.  A round that finds its key in one lane only costs a broadcast, a compare and a ballot.
//
// The flush: every lane remembers in a register mask the classes it added to; at a flush the masks are OR-ed (wave, then LDS) and only
// the 256 codes of the classes seen are visited, thread t taking code t: one 64-bit vector atomic per non-zero half, and the word is
// cleared, so the table is all zero again without a pass over it.  A workgroup sees a few thousand neighbouring pixels per frame and so
// a handful of classes; scanning all n_cls x 256 words per frame would cost as much as the tally.  All counters are integers: the result
// does not depend on the order of the atomics.
#include "arseg_device.h"

namespace {

constexpr int CAL_PEEL = 2;                     // keys a wave aggregates before its lanes add for themselves
constexpr int CAL_FLUSH_PIXELS = 65535;         // what a 16-bit half of an LDS word holds
constexpr unsigned CAL_NONE = 0xffffffffu;      // key of a pixel that does not count

struct CalP {
    const float *logits;
    const int64_t *label;
    const int32_t *group;
    unsigned long long *cal;                    // [n_groups][n_cls][256][2]
    int N, n_groups, n_cls, h, w, H, W, ignore, align, margin;
};

extern __shared__ unsigned cal_lds[];           // [n_cls][256] packed counters, then one word: the classes seen since the last flush

__device__ __forceinline__ unsigned *cal_stage(const CalP &p) {
    for (int i = threadIdx.x; i <= p.n_cls * 256; i += blockDim.x) cal_lds[i] = 0;
    __syncthreads();
    return cal_lds;
}

// One key = k* x 256 + q and its packed count v (pixels | right << 16) per active lane -> the LDS table, called by the whole wave.  UNIT:
// every active lane holds exactly one pixel, so a ballot's popcount is the sum.
template <bool UNIT>
__device__ __forceinline__ void cal_tally(unsigned *tab, unsigned key, unsigned v, bool active, unsigned &seen) {
    unsigned long long todo = __ballot(active);
#pragma unroll
    for (int round = 0; round < CAL_PEEL; ++round) {
        if (!todo) break;                                                   // uniform
        const int lead = __builtin_ctzll(todo);
        const unsigned lk = (unsigned)__builtin_amdgcn_readlane((int)key, lead);
        const bool mine = active && key == lk;
        const unsigned long long m = __ballot(mine);
        unsigned sum = v;                                                   // a key held by its leader alone
        if (UNIT) {
            sum = (unsigned)__popcll(m) | ((unsigned)__popcll(__ballot(mine && (v >> 16))) << 16);
        } else if (__popcll(m) > 1) {                                       // uniform; at most 64 x 8 pixels: the halves do not carry
            sum = mine ? v : 0u;
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o, 64);
        }
        if ((int)(threadIdx.x & 63) == lead) { atomicAdd(&tab[lk], sum); seen |= 1u << (lk >> 8); }
        active = active && !mine;
        todo &= ~m;
    }
    if (active) { atomicAdd(&tab[key], v); seen |= 1u << (key >> 8); }
}

// LDS -> row = cal[g]: the classes seen, thread t their code t; the words visited are cleared.  Called by the whole workgroup (256 threads).
__device__ __forceinline__ void cal_flush(unsigned *tab, int n_cls, unsigned long long *row, unsigned &seen) {
    unsigned *seen_lds = tab + n_cls * 256;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) seen |= __shfl_xor(seen, o, 64);
    if ((threadIdx.x & 63) == 0 && seen) atomicOr(seen_lds, seen);
    seen = 0;
    __syncthreads();
    unsigned cls = __builtin_amdgcn_readfirstlane(*seen_lds);
    __syncthreads();                                                        // every wave has read it
    if (threadIdx.x == 0) *seen_lds = 0;
    while (cls) {
        const int i = __builtin_ctz(cls) * 256 + threadIdx.x;
        cls &= cls - 1;
        const unsigned x = tab[i];
        if (x) {
            atomicAdd(&row[2 * i], (unsigned long long)(x & 0xffffu));
            if (x >> 16) atomicAdd(&row[2 * i + 1], (unsigned long long)(x >> 16));
            tab[i] = 0;
        }
    }
    __syncthreads();                                                        // the next tally finds the table clear
}

// trips of a workgroup's grid-stride loop over `total` items: the same for all its threads
__device__ __forceinline__ long long cal_trips(long long total) {
    const long long first = (long long)blockIdx.x * blockDim.x, stride = (long long)gridDim.x * blockDim.x;
    return first < total ? (total - first + stride - 1) / stride : 0;
}

__device__ __forceinline__ bool cal_group(const CalP &p, int n, int &g) {
    g = p.group ? p.group[n] : 0;
    return g >= 0 && g < p.n_groups;                                        // uniform over the workgroup
}

// ------------------------------------------------------------------ per-pixel routes: h == H && w == W, or any bilinear resize
__global__ __launch_bounds__(256) void calibration_pixel_kernel(const CalP p) {
    unsigned *tab = cal_stage(p);
    const long long total = (long long)p.H * p.W, trips = cal_trips(total);
    const float sy = arseg_resize_scale(p.h, p.H, p.align != 0), sx = arseg_resize_scale(p.w, p.W, p.align != 0);
    const bool same = (p.h == p.H && p.w == p.W);
    constexpr int every = CAL_FLUSH_PIXELS / 256;
    for (int n = blockIdx.y; n < p.N; n += gridDim.y) {
        int g;
        if (!cal_group(p, n, g)) continue;
        unsigned long long *row = p.cal + (size_t)g * p.n_cls * 512;
        unsigned seen = 0;
        for (long long it = 0; it < trips; ++it) {
            long long idx = ((long long)blockIdx.x + it * gridDim.x) * blockDim.x + threadIdx.x;
            const bool live = idx < total;
            idx = live ? idx : total - 1;                                   // (a lane past the end recomputes the last pixel and counts nothing)
            const int ox = (int)(idx % p.W), oy = (int)(idx / p.W);
            ArsegSoftmaxAcc<1> acc;
            const int k = arseg_label_pixel(p.logits, n, oy, ox, p.n_cls, p.h, p.w, p.align, same, sy, sx, &acc);
            const unsigned q = acc.code(0, p.margin != 0);
            const long long lab = p.label[((long long)n * p.H + oy) * p.W + ox];
            const bool counts = live && lab != p.ignore && lab >= 0 && lab < p.n_cls;
            cal_tally<true>(tab, (unsigned)k * 256u + q, 1u | (lab == k ? 1u << 16 : 0u), counts, seen);
            if ((it + 1) % every == 0 && it + 1 < trips) cal_flush(tab, p.n_cls, row, seen);
        }
        cal_flush(tab, p.n_cls, row, seen);
    }
}

// ------------------------------------------------------------------ run route: exact x S upsample, align_corners == 0, S = 2 | 4 | 8
template <int S>
__global__ __launch_bounds__(256) void calibration_run_kernel(const CalP p) {
    unsigned *tab = cal_stage(p);
    const int H = S * p.h, W = S * p.w, runs = p.w + 1;
    const long long total = (long long)H * runs, trips = cal_trips(total);
    const float sc = arseg_resize_scale(p.h, H, false);          // = 1 / S exactly
    constexpr int every = CAL_FLUSH_PIXELS / (256 * S);
    for (int n = blockIdx.y; n < p.N; n += gridDim.y) {
        int g;
        if (!cal_group(p, n, g)) continue;
        unsigned long long *row = p.cal + (size_t)g * p.n_cls * 512;
        unsigned seen = 0;
        for (long long it = 0; it < trips; ++it) {
            long long idx = ((long long)blockIdx.x + it * gridDim.x) * blockDim.x + threadIdx.x;
            const bool live = idx < total;
            idx = live ? idx : total - 1;
            const int j = (int)(idx % runs) - 1, oy = (int)(idx / runs);
            int k[S];
            ArsegSoftmaxAcc<S> acc;
            arseg_label_run<S>(p.logits, sc, n, oy, j, p.n_cls, p.h, p.w, k, &acc);
            const int xs = S * j + S / 2;               // the run's first column; the first and the last run hold S/2 pixels of the frame
            const int64_t *lrow = p.label + ((long long)n * H + oy) * W;
            unsigned key[S], val[S];
#pragma unroll
            for (int r = 0; r < S; ++r) {
                const int ox = xs + r;
                const long long lab = lrow[min(max(ox, 0), W - 1)];
                const bool counts = live && ox >= 0 && ox < W && lab != p.ignore && lab >= 0 && lab < p.n_cls;
                key[r] = counts ? (unsigned)k[r] * 256u + acc.code(r, p.margin != 0) : CAL_NONE;
                val[r] = 1u | (lab == k[r] ? 1u << 16 : 0u);
            }
            unsigned v = 0;
#pragma unroll
            for (int r = 0; r < S; ++r) {               // neighbours of a run mostly share class and code: one key per stretch of equal ones
                v += key[r] != CAL_NONE ? val[r] : 0u;
                const bool emit = key[r] != CAL_NONE && (r == S - 1 || key[r + 1] != key[r]);
                if (__ballot(emit)) cal_tally<false>(tab, key[r], v, emit, seen);          // uniform
                v = emit ? 0u : v;
            }
            if ((it + 1) % every == 0 && it + 1 < trips) cal_flush(tab, p.n_cls, row, seen);
        }
        cal_flush(tab, p.n_cls, row, seen);
    }
}

// workgroups per frame x frames: the tail's caps on the whole launch, shared among the frames (confidence.hip's conf_grid)
dim3 cal_grid(long long per_frame, int N, int cap) {
    const int gy = N < 65535 ? N : 65535;
    const long long share = cap / gy > 0 ? cap / gy : 1, need = (per_frame + 255) / 256;
    return dim3((unsigned)(need < share ? need : share), (unsigned)gy);
}

}  // namespace

extern "C" int arseg_calibration_fwd(const float *logits, const int64_t *label, const int32_t *group, int64_t *cal, int N, int n_groups, int n_cls,
                                     int h, int w, int H, int W, int ignore_label, int align_corners, int kind, arseg_stream_t stream) {
    ARSEG_CHECK_PTR(logits); ARSEG_CHECK_PTR(label); ARSEG_CHECK_PTR(cal);
    if (n_groups < 1 || (!group && n_groups > 1)) return ARSEG_EINVAL;
    if (n_cls < 1 || n_cls > 32) return ARSEG_EINVAL;
    ARSEG_CHECK_POS(N); ARSEG_CHECK_POS(h); ARSEG_CHECK_POS(w); ARSEG_CHECK_POS(H); ARSEG_CHECK_POS(W);
    if (kind != ARSEG_CONF_TOP1 && kind != ARSEG_CONF_MARGIN) return ARSEG_EINVAL;
    if ((reinterpret_cast<uintptr_t>(label) & 7u) || (reinterpret_cast<uintptr_t>(cal) & 7u) || (reinterpret_cast<uintptr_t>(group) & 3u)) return ARSEG_EINVAL;
    CalP p = {};
    p.logits = logits; p.label = label; p.group = group; p.cal = reinterpret_cast<unsigned long long *>(cal);
    p.N = N; p.n_groups = n_groups; p.n_cls = n_cls; p.h = h; p.w = w; p.H = H; p.W = W; p.ignore = ignore_label;
    p.align = align_corners ? 1 : 0; p.margin = kind == ARSEG_CONF_MARGIN ? 1 : 0;
    hipStream_t st = arseg_stream(stream);
    const size_t lds = ((size_t)n_cls * 256 + 1) * sizeof(unsigned);
    const int S = H / h;
    if (!p.align && S * h == H && S * w == W && (S == 2 || S == 4 || S == 8)) {          // the route choice of arseg_segment_confidence_fwd
        const dim3 g = cal_grid((long long)H * (w + 1), N, 4096);
        if (S == 8) hipLaunchKernelGGL((calibration_run_kernel<8>), g, dim3(256), lds, st, p);
        else if (S == 4) hipLaunchKernelGGL((calibration_run_kernel<4>), g, dim3(256), lds, st, p);
        else hipLaunchKernelGGL((calibration_run_kernel<2>), g, dim3(256), lds, st, p);
        return arseg_launch_status();
    }
    hipLaunchKernelGGL(calibration_pixel_kernel, cal_grid((long long)H * W, N, 1024), dim3(256), lds, st, p);
    return arseg_launch_status();
}
