// The launch plans of the two conv engines, stated once (host only): what every arseg_conv_desc.tile_cfg of arseg_conv2d_fwd (fp32 storage,
// conv_igemm.hip / conv_up2_c64.hip) and of arseg_conv2d16_fwd (16-bit storage, conv16.hip) is, and the geometry the engines share.  The
// numbering is public (include/arseg_hip.h documents it); everything that needs the meaning of an id reads its row here.
#pragma once
#include "arseg_common.h"

// one id of an engine.  bm = output pixels of a tile, bn = its output channels, bk = K step, nbuf = LDS stages of the operand tiles;
// 0 = chosen per shape (the auto plans)
struct ConvPlanRow {
    int kind;              // enum arseg_conv_plan_kind
    int bm, bn, bk, nbuf;
    int patch_tw;          // patch-resident plans: forced width of the pixel tile; 0 = by the width of the map
    bool f16x3_only, fuses_up2, split_k;      // refused under other maths | applies desc.upsample2x itself | may take split-K
};
constexpr ConvPlanRow plan_tile(int bm, int bn, int bk, int nbuf) { return {ARSEG_PLAN_TILE, bm, bn, bk, nbuf, 0, false, false, true}; }
constexpr ConvPlanRow plan_patch(int bm, int bn, int bk, bool f16x3, int tw = 0) { return {ARSEG_PLAN_PATCH, bm, bn, bk, 2, tw, f16x3, true, false}; }

constexpr ConvPlanRow kConvPlans32[] = {
    {ARSEG_PLAN_AUTO, 0, 0, 32, 1, 0, false, false, true},
    // 1..4 double-buffered, 5..8 single-buffered (half the LDS, more workgroups per CU), 9..12 single-buffered with K step 64
    plan_tile(128, 128, 32, 2), plan_tile(128, 64, 32, 2), plan_tile(64, 64, 32, 2), plan_tile(64, 128, 32, 2),
    plan_tile(128, 128, 32, 1), plan_tile(128, 64, 32, 1), plan_tile(64, 64, 32, 1), plan_tile(64, 128, 32, 1),
    plan_tile(128, 128, 64, 1), plan_tile(128, 64, 64, 1), plan_tile(64, 64, 64, 1), plan_tile(64, 128, 64, 1),
    // 13..16 patch-resident 3x3 kernel: the input patch of a 128- / 256-pixel tile stays in LDS for all nine taps
    plan_patch(128, 64, 32, true), plan_patch(128, 128, 32, true), plan_patch(256, 64, 32, true), plan_patch(256, 128, 32, true),
    // 17..19 GEMM tiles on 8 / 16 waves (more reuse per byte from L2 / MALL)
    {ARSEG_PLAN_TILE_WIDE, 256, 128, 32, 1, 0, true, false, true}, {ARSEG_PLAN_TILE_WIDE, 128, 256, 32, 1, 0, true, false, true},
    {ARSEG_PLAN_TILE_WIDE, 256, 256, 32, 1, 0, true, false, true},
    // 20..22 the patch-resident kernel on squarer pixel tiles -- 256 pixels as 8 x 32 and as 16 x 16, 128 as 8 x 16 -- whose patch has less halo
    // than the 4 x 64 / 2 x 64 of a wide map (340 / 324 staged pixels against 396 per 256 outputs)
    plan_patch(256, 64, 32, true, 32), plan_patch(256, 64, 32, true, 16), plan_patch(128, 64, 32, true, 16),
    // 23 the persistent kernel of up_3 (conv_up2_c64.hip): 8 x 16 pixel tiles, 64 -> 64 channels
    {ARSEG_PLAN_UP2_C64, 128, 64, 32, 2, 0, true, true, false},
};

// the 16-bit engine: bn = channel tile, bk = K step in halves, bm = pixel tile
constexpr ConvPlanRow kConvPlans16[] = {
    {ARSEG_PLAN_AUTO, 128, 0, 0, 2, 0, false, false, true},
    plan_tile(128, 64, 32, 2), plan_tile(128, 128, 32, 2), plan_tile(128, 64, 64, 2), plan_tile(128, 128, 64, 2),
    // 5..8 patch-resident 3x3 kernel
    plan_patch(128, 64, 64, false), plan_patch(128, 128, 64, false), plan_patch(256, 64, 64, false), plan_patch(256, 128, 64, false),
    // 9 stem kernel (7x7 stride 2 pad 3, NHWC8 -> 64 channels): 8 x 32 output tiles, one MFMA K step = two taps, all weights resident in LDS
    {ARSEG_PLAN_STEM, 256, 64, 16, 1, 0, false, false, false},
    // 10..13 the patch-resident kernel on squarer pixel tiles: 8 x 32, 16 x 16, 8 x 32 with 128 channels, 8 x 16
    plan_patch(256, 64, 64, false, 32), plan_patch(256, 64, 64, false, 16), plan_patch(256, 128, 64, false, 32), plan_patch(128, 64, 64, false, 16),
};

template <int N>
static inline const ConvPlanRow *conv_plan_row(const ConvPlanRow (&table)[N], int tile_cfg) {      // null: not an id of that engine
    return tile_cfg >= 0 && tile_cfg < N && table[tile_cfg].kind != ARSEG_PLAN_NONE ? &table[tile_cfg] : nullptr;
}

// what a descriptor launches: the public part (the row's tile with the per-shape choices made) and the launch's own numbers
struct ConvPlan : arseg_conv_plan_info {
    int ktiles, ktiles_per_split, tiles_m, tiles_n, M, K, Kpad;
    void take(const ConvPlanRow &r) { kind = r.kind; bm = r.bm; bn = r.bn; bk = r.bk; nbuf = r.nbuf; fuses_upsample = r.fuses_up2; split_k_allowed = r.split_k; }
    void split(int n, int Cout) { nsplit = n; workspace_bytes = n > 1 ? (size_t)n * M * Cout * sizeof(float) : 0; }      // fp32 partials per K slice
};

// Output size of a descriptor (fills Ho, Wo, M, K), or why no plan of either engine can take it: nothing here looks at tile_cfg.
static inline int conv_geometry(const arseg_conv_desc *d, ConvPlan *pl) {
    if (!d || d->N <= 0 || d->H <= 0 || d->W <= 0 || d->Cin <= 0 || d->Cout <= 0 || d->R <= 0 || d->S <= 0 || d->stride <= 0 ||
        d->dil <= 0 || d->pad < 0)
        return ARSEG_EINVAL;
    if ((d->Cin & 3) || (d->in_ld & 3) || d->in_ld < d->Cin || d->out_ld < d->Cout) return ARSEG_EINVAL;
    if (d->R * d->S > 1 && (d->Cin & (d->Cin - 1))) return ARSEG_EUNSUPPORTED;
    if (d->math != ARSEG_MATH_F32 && d->math != ARSEG_MATH_F16X3 && d->math != ARSEG_MATH_F16) return ARSEG_EINVAL;
    pl->Ho = (d->H + 2 * d->pad - d->dil * (d->R - 1) - 1) / d->stride + 1;
    pl->Wo = (d->W + 2 * d->pad - d->dil * (d->S - 1) - 1) / d->stride + 1;
    if (pl->Ho <= 0 || pl->Wo <= 0) return ARSEG_EINVAL;
    const long long M = (long long)d->N * pl->Ho * pl->Wo;
    if (M > (1ll << 30) || (long long)d->N * d->H * d->W > (1ll << 30)) return ARSEG_EUNSUPPORTED;
    pl->M = (int)M; pl->K = d->R * d->S * d->Cin;
    return ARSEG_OK;
}

// operands are addressed through 32-bit buffer offsets: the extents of the fp32 engine (kpad32 = arseg_packed_k); the 16-bit engine, whose
// elements are half as large, is held to the same counts
static inline bool conv_fits_32bit(const arseg_conv_desc *d, int kpad32) {
    return ((long long)d->N * d->H * d->W * d->in_ld + d->Cin) * 4 < (1ll << 31) && (long long)d->Cout * kpad32 * 4 < (1ll << 31);
}

// Pixel tile th x tw (th * tw = bm) of a patch-resident plan on a map Wo wide: 64, 32 or 16 wide by the map, or the row's forced width, which
// is refused where the by-width tile is already that narrow (the same tile: not a new plan), as is a patch (tile + dilated halo) of more
// staged pixels than the kernel's LDS budget (288 for 128-pixel tiles, 448 for 256).
static inline int conv_patch_tile(int Wo, int dil, int bm, int forced_tw, int *tw, int *th) {
    *tw = Wo >= 48 ? 64 : (Wo >= 24 ? 32 : 16);
    if (forced_tw) { if (*tw <= forced_tw) return ARSEG_EUNSUPPORTED; *tw = forced_tw; }
    *th = bm / *tw;
    return (*th + 2 * dil) * (*tw + 2 * dil) > (bm == 128 ? 288 : 448) ? ARSEG_EUNSUPPORTED : ARSEG_OK;
}

// A patch-resident plan on this shape (3x3 stride 1 pad == dil, Cin a multiple of the engine's granule cin_mask + 1): its pixel tile and tile counts.
static inline int conv_patch_plan(const arseg_conv_desc *d, const ConvPlanRow &row, int cin_mask, ConvPlan *pl) {
    if (d->R != 3 || d->S != 3 || d->stride != 1 || d->pad != d->dil || (d->Cin & cin_mask) || d->batch > 1 || d->split_k > 1) return ARSEG_EUNSUPPORTED;
    if (d->upsample2x && (d->dil != 1 || (d->H & 1) || (d->W & 1))) return ARSEG_EUNSUPPORTED;
    if (int e = conv_patch_tile(pl->Wo, d->dil, row.bm, row.patch_tw, &pl->patch_tw, &pl->patch_th)) return e;
    pl->tiles_m = d->N * arseg_cdiv(pl->Ho, pl->patch_th) * arseg_cdiv(pl->Wo, pl->patch_tw);
    pl->tiles_n = arseg_cdiv(d->Cout, row.bn);
    return ARSEG_OK;
}

// The shape class of the persistent up_3 kernel: fp32 id 23 and arseg_conv_up2_c64_fwd (which is not told an id) both ask this.
static inline bool conv_up2_c64_shape(const arseg_conv_desc *d) {
    return d->upsample2x && d->math == ARSEG_MATH_F16X3 && d->Cin == 64 && d->Cout == 64 && d->R == 3 && d->S == 3 && d->stride == 1 && d->pad == 1 &&
           d->dil == 1 && !(d->H & 1) && !(d->W & 1) && d->batch <= 1 && d->split_k <= 1;
}
// ... and its extents in bytes (in = [N, H/2, W/2, in_ld], out = [N, H, W, out_ld]), which must stay inside 32-bit buffer offsets
static inline long long conv_up2_c64_in_bytes(const arseg_conv_desc *d) { return (((long long)d->N * (d->H >> 1) * (d->W >> 1) - 1) * d->in_ld + 64) * 4; }
static inline long long conv_up2_c64_out_bytes(const arseg_conv_desc *d) { return (((long long)d->N * d->H * d->W - 1) * d->out_ld + 64) * 4; }

// the 16-bit engine's plan of a descriptor (conv16.hip): the verdict of arseg_conv2d16_fwd before it looks at pointers.  Internal to the library.
__attribute__((visibility("hidden"))) int conv16_plan(const arseg_conv_desc *d, ConvPlan *pl);
constexpr int kConv16AutoUp2 = 7;      // the plan the 16-bit auto id stands for under upsample2x: 256 pixels x 64 channels, tile by the map's width
