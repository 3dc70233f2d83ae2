// THE launch rules of the GEMM family (see dispatch.hpp): pure functions of GemmParams and one device figure.  The contract they carry: a frame's bits
// do not depend on which other frames share its launch (frame sharding, the two launch streams and bench.py's bit check rest on it).  A choice that
// changes an fp32 summation order -- the K split, the column-statistics slicing of a kernel or a tile width -- looks at the PER-SAMPLE geometry and
// takes its grid depth at a nominal batch, never at the launch's; choices between bit-identical forms (the 256-row tile, its width, the persistent
// form, the tile order) may follow the batch.
#include "dispatch.hpp"
#include "../../include/vface_hip.h"

namespace {
constexpr int BM = VF_GEMM_BM, BK = VF_GEMM_BK, TP = VF_PATCH_TP, BM2 = VF_BIG_BM, BN2 = VF_BIG_BN;
// Nominal batch of the rules from rounds 1-3: 24 samples, the 8-frame clip.  pick_variant, split_for and the patch / im2col choice.
// (Tried and not taken: the plain GEMM's tile-width / split-K rules at 48 -- 83.19 vs 83.12 ms, HISTORY.md.)
constexpr long NOMINAL_BATCH_CLIP = 24;
// Nominal batch of the patch kernel's tile width (round 5) and of the 8x8 form's K split (round 6): 48 samples, one launch stream's half of the
// 32-frame headline and a rank's 16-frame share at N > 1.  Measured same-box: the width at 24 would hand the 32 x 32 640-channel launches the
// 128-wide tile -- 15 % faster THERE, 6 % slower at 48 and 96 samples; headline 79.34 -> 79.10 ms/step, conv family 33.4 -> 32.8 (profiles/r05_o).
// The split: K in two shares instead of four -- half the prologues, epilogues and fp32 partials; 32 frames 76.22 -> 75.83 ms/step (conv family 31.65
// -> 30.96), the 8-frame clip pays for it, 20.0 -> 20.6 (profiles/r06_i).
constexpr long NOMINAL_BATCH_STREAM = 48;
constexpr int SPLIT_K_MAX = 8;            // fp32 partial tiles per output tile, at most
constexpr int SPLIT_K_MAX_TILES = 192;    // no split above this many tiles at the nominal batch
constexpr int BIG_MIN_TILES = 192;        // the 256 x 320 tile from this many tiles on: about a round of the one-workgroup-per-CU grid (profiles/r05_c, r05_d)
constexpr int PATCH_MIN_TILES = 160;      // the patch-staged kernel from this many tiles at the nominal batch on (that grid is a multiple of 24: 145..168 act alike)

inline int forced_variant(int flags) { return (flags >> 8) & 0xF; }      // bits 8..11: forced schedule variant (A/B); 0 = automatic
inline bool misaligned(const void* p, unsigned mask) { return ((uintptr_t)p & mask) != 0; }
inline int residual_form(const GemmParams& p) { return p.res_f32 ? 2 : (p.residual ? 1 : 0); }

// Column-group width GN of the XCD-aware tile order.  An XCD (own L2) works through tiles / 8 consecutive tiles = a block of (tiles_xcd / GN) m-tiles
// x GN n-tiles, and fetches that block's activations and weight panels once: bytes per XCD = tiles_xcd / GN * A_mt + GN * W_nt, least at GN =
// sqrt(tiles_xcd * A_mt / W_nt).  (On the 16x16 level a fixed GN = 8 made every XCD fetch 80 % of the weights: 256 MB per launch measured.)  l2_cap:
// the GN weight panels, re-used over many rounds by the plain GEMMs, stay within half of the 4 MiB L2; the patch kernel has no cap.
int tile_group(int ntm, int ntn, double a_mt, double w_nt, bool l2_cap) {
    int gn = (int)(__builtin_sqrt((double)ntm * ntn / 8.0 * a_mt / w_nt) + 0.5);
    if (l2_cap && gn > (int)(2097152.0 / w_nt)) gn = (int)(2097152.0 / w_nt);
    return gn < 1 ? 1 : (gn > ntn ? ntn : gn);
}

// ---- inconv.hip: is this convolution the 16-stored-channel input form (the UNet's 9 (16 stored) -> 320 input convolution: K = 144 in one MFMA pass,
// bound by its stores)?  Per-sample geometry and epilogue form only.
bool conv_in16_ok(const GemmParams& p) {
    if (p.mode != 1 || p.Cin != 16 || p.ntaps != 9 || p.KH != 3 || p.KW != 3 || p.stride != 1 || p.upsample || p.pad != 1 || p.pad_x != 1) return false;
    if (p.A2 || p.residual || p.rowbias || p.gn_ab || p.out_phase || p.res_f32) return false;
    if (p.flags & (GEMM_GEGLU | GEMM_OUT_F32 | GEMM_NO_PATCH | GEMM_STAMPS | (0xF << 8))) return false;      // (GEMM_NO_PATCH: A/B, the generic kernel)
    if ((p.N % VF_IN16_CH) || p.K != VF_IN16_K || p.Kw < VF_IN16_K || (p.ldw & 7)) return false;
    if (p.OH != p.H || p.OW != p.W || ((p.H * p.W) & 63) || (p.W & 15) || p.M != (p.M / (p.H * p.W)) * p.H * p.W) return false;
    if (!p.C && !p.C32) return false;
    if (p.C && (misaligned(p.C, 15) || (p.ldc & 7))) return false;
    if (p.C32 && (misaligned(p.C32, 15) || (p.ldc32 & 3))) return false;
    if (p.colstats && (misaligned(p.colstats, 15) || (p.ld_colstats & 1))) return false;
    if (p.bias && misaligned(p.bias, 15)) return false;
    const unsigned long cb = p.C ? ((unsigned long)(p.M - 1) * p.ldc + p.N) * 2ul : 0ul, c32b = p.C32 ? ((unsigned long)(p.M - 1) * p.ldc32 + p.N) * 4ul : 0ul;
    return cb < 0xFFFF0000ul && c32b < 0xFFFF0000ul && p.a_bytes < 0xFFFF0000u;
}

// ---- conv.hip: 0 = this launch is not a patch-kernel shape; else the channel-tile width (160 | 128) the launch uses
int conv_patch_tile(const GemmParams& p) {
    if (p.mode != 1 || p.stride != 1 || p.upsample || (p.Cin & 63)) return 0;
    if (p.OH != p.H || p.OW != p.W || (p.H % TP) || (p.W % TP)) return 0;
    if (!((p.KH == 3 && p.KW == 3) || (p.KH == 2 && p.KW == 2)) || p.ntaps != p.KH * p.KW) return 0;
    if (p.pad < 0 || p.pad_x < 0 || p.pad > 1 || p.pad_x > 1) return 0;
    if ((p.flags & (GEMM_GEGLU | GEMM_OUT_F32 | GEMM_NARROW_EPILOGUE)) || (p.N & 7)) return 0;
    if ((p.flags & GEMM_STAMPS) && !(p.KH == 3 && p.N % 160 == 0 && p.colstats)) return 0;   // the stamped build: one instantiation
    if (p.A2 && (((p.K - p.K1) & 63) || p.KH != 3)) return 0;
    if (p.gn_ab && (p.KH != 3 || (p.ld_gn_ab < p.Cin) || misaligned(p.gn_ab, 15) || (p.flags & GEMM_STAMPS))) return 0;
    if (p.colstats && ((p.H * p.W) & 63)) return 0;
    if (p.residual && !p.res_f32 && (misaligned(p.residual, 15) || (p.ldr & 7))) return 0;
    if (misaligned(p.C, 15) || (p.C && (p.ldc & 7))) return 0;
    const bool ok160 = p.N % 160 == 0, ok128 = p.N % 128 == 0;
    if (p.gn_ab) return ok128 ? 128 : 0;   // the fused-normalisation build exists 128 wide only (the 160-wide one spilled 36 B)
    if (p.KH == 2 && (p.residual || p.res_f32)) return ok128 ? 128 : 0;      // ... and so does the 2 x 2 window with a residual operand
    if (ok160 && ok128 && !(p.flags & (GEMM_PATCH_BN160 | GEMM_STAMPS))) {
        // Both widths tile N (640, 1280, 1920 channels): one workgroup per CU, so a launch takes ceil(workgroups / CUs) rounds, and a 128-wide
        // workgroup takes ~0.8 of a 160-wide one (32 instead of 40 MFMAs per wave and K tile, same fixed costs).  Measured
        // (tools/quantisation_probe.py, 24 samples): 32x32 640->640: 160-wide 384 workgroups = 1.5 rounds 181.6 us, 128-wide 480 = 1.9 rounds 153.6
        // us; 16x16 1280->1280: 192 = 0.75 rounds 175.3 us vs 240 = 0.94 rounds 151.8 us.  Grid at NOMINAL_BATCH_STREAM on 256 CUs: the width changes
        // the summation order of the column statistics (batch invariance).
        const long tiles = NOMINAL_BATCH_STREAM * (p.H / TP) * (p.W / TP);
        const long r160 = (tiles * (p.N / 160) + 255) / 256, r128 = (tiles * (p.N / 128) + 255) / 256;
        return (r128 * 4 < r160 * 5) ? 128 : 160;      // r128 * 0.8 < r160
    }
    return ok160 ? 160 : ok128 ? 128 : 0;
}

// largest K split of the 8x8 form at N channels: four images per workgroup and N / 128 channel tiles give (nimg / 4) * (N / 128) workgroups -- 120 at
// NOMINAL_BATCH_STREAM on the UNet's 1280-channel level --, so K is split over channel chunks until the one-per-CU grid is about one round
int q8_grid_split(int N) {
    const int s = (int)(256 / (NOMINAL_BATCH_STREAM / 4 * (N / 128)));
    return s > SPLIT_K_MAX ? SPLIT_K_MAX : s;
}
// The 8 x 8 level through the patch-staged kernel (Q8 form): 0 = not such a launch, else the K split (number of fp32 partial tiles per output tile)
int conv_q8_split(const GemmParams& p) {
    if (p.mode != 1 || p.stride != 1 || p.upsample || p.out_phase || (p.Cin & 63) || p.gn_ab) return 0;
    if (p.H != 8 || p.W != 8 || p.OH != 8 || p.OW != 8 || p.KH != 3 || p.KW != 3 || p.ntaps != 9 || p.pad != 1 || p.pad_x != 1) return 0;
    if ((p.flags & (GEMM_GEGLU | GEMM_OUT_F32 | GEMM_NARROW_EPILOGUE | GEMM_NO_PATCH | GEMM_STAMPS | (0xF << 8))) || (p.N % 128)) return 0;
    if (p.A2 && ((p.K - p.K1) & 63)) return 0;
    if (p.rows_per_sample != 64 && p.rowbias) return 0;
    const int nchunks = p.Cin >> 6;
    int s = q8_grid_split(p.N);
    if (s > nchunks / 2) s = nchunks / 2;       // at least two chunks (18 K tiles) per share
    return s < 1 ? 0 : s;
}

// THE rule for which kernel a convolution launch runs -- 0: gemm.hip's implicit GEMM, 1: the patch-staged kernel (*arg = channel-tile width), 2: its
// 8x8 form (*arg = K split; the plan also needs the caller's split-K workspace, which every wrapper passes).  vf_plan_gemm dispatches on it and
// vface_conv_uses_patch_kernel (what bench.py prices launches by and the engine decides GroupNorm fusion by) reports it: one copy.  Geometry and
// flags only, grid depth at NOMINAL_BATCH_CLIP: the kernels give the same output bits but slice the column statistics differently.
int conv_kernel_choice(const GemmParams& p, int* arg) {
    *arg = 0;
    if (p.mode != 1 || forced_variant(p.flags) || (p.flags & GEMM_NO_PATCH)) return 0;
    const int bn = conv_patch_tile(p);
    if (bn && (NOMINAL_BATCH_CLIP * (p.H / TP) * (p.W / TP) * (p.N / bn) >= PATCH_MIN_TILES || (p.flags & GEMM_PATCH))) { *arg = bn; return 1; }
    *arg = (p.flags & GEMM_NO_Q8) ? 0 : conv_q8_split(p);
    return *arg ? 2 : 0;
}

// Plain GEMM through the patch-staged kernel's 256 x BN tile (8 waves, one workgroup per CU): the kernel's "fused 1x1 source" K loop IS a GEMM K loop
// -- 256 consecutive rows of A per workgroup as a halo-free 16 x 16 "image", no window tiles.  Versus gemm.hip's 128-row tile: 28 % fewer L2->LDS
// bytes per FLOP (measured where it pays: DESIGN 4).  0 = not a shape this form takes; else the channel-tile width.
int gemm_patch_tile(const GemmParams& p) {
    if (p.mode != 0 || p.A2 || p.out_phase || p.gn_ab || p.split_k > 1) return 0;
    if ((p.M % (TP * TP)) || (p.K & 63) || p.K < 128) return 0;
    if ((p.flags & (GEMM_GEGLU | GEMM_OUT_F32 | GEMM_NARROW_EPILOGUE | GEMM_STAMPS)) || (p.N & 7)) return 0;
    if (p.rowbias && (p.rows_per_sample <= 0 || (p.rows_per_sample % (TP * TP)))) return 0;
    if (p.residual && !p.res_f32 && (misaligned(p.residual, 15) || (p.ldr & 7))) return 0;
    if (misaligned(p.C, 15) || (p.C && (p.ldc & 7))) return 0;
    return p.N % 160 == 0 ? 160 : p.N % 128 == 0 ? 128 : 0;
}

// ---- gemm_big.hip: is this plain-GEMM launch one the 256 x 320 tile takes?  Shape, operands and epilogue form only.
bool gemm_big_ok(const GemmParams& p) {
    if (p.mode != 0 || p.out_phase || p.gn_ab || p.split_k > 1 || p.a2_row_mod) return false;
    if ((p.N % BN2) || (p.K & 63) || p.K < 128 || (p.Kw < p.K)) return false;
    if (p.A2 && ((p.K1 & 63) || p.K1 <= 0 || p.K1 >= p.K)) return false;
    if (p.flags & (GEMM_OUT_F32 | GEMM_NARROW_EPILOGUE | GEMM_F32_TRANSPOSE | GEMM_STAMPS | (0xF << 8))) return false;
    if (p.C32) {
        // the fp32 residual-stream form (EPI 3): carrier required; the per-sample row bias needs every 256-row tile inside one sample
        if (p.flags & GEMM_GEGLU) return false;
        if (misaligned(p.C32, 15) || (p.ldc32 & 3)) return false;
        if (p.rowbias && (p.rows_per_sample <= 0 || (p.rows_per_sample % BM2) || (p.ld_rowbias & 3) || misaligned(p.rowbias, 15))) return false;
        if (p.colstats && ((p.M & 63) || (p.ld_colstats & 1) || misaligned(p.colstats, 7))) return false;
    } else if (p.colstats || p.rowbias || !p.C) {
        return false;
    }
    if (p.C && (misaligned(p.C, 15) || (p.ldc & 7))) return false;
    if ((p.lda & 7) || (p.ldw & 7)) return false;
    if (p.residual && ((p.flags & GEMM_GEGLU) || misaligned(p.residual, 15) || (p.ldr & (p.res_f32 ? 3 : 7)))) return false;
    if (p.residual && !p.res_f32 && p.C32) return false;      // (16-bit residual rows: the 16-bit-output form only)
    if (p.bias && misaligned(p.bias, 15)) return false;
    return true;
}

// THE rule for which plain-GEMM kernel a launch runs.  Outputs and the fp32 carrier are bit-identical between the two kernels, so the choice may look
// at the batch (the per-64-row column statistics of the residual-stream form are not: another fold order -- one more reason that form is never chosen
// automatically); 16-bit-output launches take the 256 x 320 tile from BIG_MIN_TILES on.
bool gemm_big_choice(const GemmParams& p) {
    if ((p.flags & GEMM_NO_BIG) || !gemm_big_ok(p)) return false;
    if (p.flags & GEMM_BIG) return true;
    // the fp32 residual-stream form (EPI 3: proj_in / to_out / proj_out) is built, bit-identical and MEASURED SLOWER than the 128-row kernel on 14 of
    // 18 of the UNet's launches (profiles/r05_e: 0.78-1.29x): bound by their epilogue's HBM traffic (4 + 4 B per output element around a K = 640
    // loop), which two 128-row workgroups per CU overlap with each other's K loops and one 256-row workgroup cannot.  Selectable
    // (VFACE_TUNE_BIG_TILE), never chosen here.
    if (p.C32) return false;
    return (long)((p.M + BM2 - 1) / BM2) * (p.N / BN2) >= BIG_MIN_TILES;
}

// Tile width of a 256-row launch: 320 channels, or 256 where N allows both, K is short and the one-workgroup-per-CU grid then takes fewer tile-times
// (rounds of 256 workgroups).  MEASURED (tools/bench_gemm_widths.py, profiles/r06_h): a 256-wide tile is NOT 0.8 of a 320-wide one when K is deep --
// ff2 at K = 5120: 240 tiles in one round take as long as 192 (175 vs 180 us at 48 samples; 361 vs 349 at 96), the K loop waits for its activation
// pieces, which five n-tiles per m-tile request instead of four -- it pays where prologue and epilogue weigh: the 1280 x 1280 projections (55 -> 45
// us at 48 samples, 90 -> 80 at 96) and the dual-source projection under one round (80 -> 70).  Hence K <= 1280 only, and only where the rounds say
// so at 0.85 of a tile-time.  Same bits at both widths, so the choice may follow the batch; GEMM_BIG_W256 / _W320 force one.  The fp32
// residual-stream form is built 320 wide only.
int gemm_big_width(const GemmParams& p) {
    if (p.C32 || (p.N % 256) || (p.flags & GEMM_BIG_W320)) return 320;
    const long ntm = (p.M + BM2 - 1) / BM2;
    const long r320 = (ntm * (p.N / 320) + 255) / 256, r256 = (ntm * (p.N / 256) + 255) / 256;
    return ((p.flags & GEMM_BIG_W256) || (p.K <= 1280 && (double)r256 * 0.85 < (double)r320)) ? 256 : 320;
}

// ---- gemm.hip.  Schedule variants (flags bits 8..11 force one for A/B runs): 5 = 128x128x64 two stages, 6 = 128x160x64 two stages, 7 = 128x128x64
// one stage, 8 = 128x160x64 one stage; 11..15 run 8's kernel without column statistics (15 also turns the K split off in vf_splitk_workspace_bytes).
// 1-4, 9 and 10 were the experimental schedules of rounds 1-3: removed, refused.
bool variant_exists(int v) { return (v >= 5 && v <= 8) || v >= 11; }
int pick_variant(const GemmParams& p) {
    if (const int forced = forced_variant(p.flags)) return forced;
    const bool geglu = p.flags & GEMM_GEGLU;
    // BN = 160 moves 10 % fewer L2->LDS bytes per FLOP.  Where N is a multiple of 128 as well (640, 1280, 1920) it only pays once the grid is several
    // rounds deep (measured: +5..10 % at >= 1536 tiles, -3..5 % below: 160-wide tiles quantise a 1-2 round grid worse).  Grid depth at
    // NOMINAL_BATCH_CLIP when the per-sample geometry is known, like split_for: the column statistics are folded in a tile-shape-dependent order.
    const long mref = p.rows_per_sample > 1 ? NOMINAL_BATCH_CLIP * p.rows_per_sample : p.M;
    const long tiles160 = ((mref + BM - 1) / BM) * (p.N / 160);
    const bool n160 = !geglu && (p.N % 160 == 0) && ((p.N % 128 != 0) || tiles160 >= 1536);
    return n160 ? 6 : 5;
}

// Split-K factor for a launch whose tile grid would leave most of the 256 CUs (2 workgroups each) idle while every workgroup walks a long K loop (the
// 8x8-level convolutions: 120 tiles x 180..360 K tiles).  A function of the PER-SAMPLE geometry when the caller states it (rows_per_sample = OH*OW of
// a conv, h*w of a token matrix): tile count at NOMINAL_BATCH_CLIP, so a frame's bits do not depend on how many other frames share its launch (the
// fp32 summation order changes with the split) -- what frame sharding relies on.
int split_for(int M, int N, int K, int flags, int rows_per_sample) {
    if (flags & (GEMM_GEGLU | GEMM_OUT_F32)) return 1;
    if ((N & 7) || forced_variant(flags) == 0xF) return 1;
    const int bn = (N % 160 == 0) && (N % 128 != 0) ? 160 : 128;
    const long mref = rows_per_sample > 1 ? NOMINAL_BATCH_CLIP * rows_per_sample : M;
    const int tiles = (int)((mref + BM - 1) / BM) * ((N + bn - 1) / bn);
    const int nt = (K + BK - 1) / BK;
    if (tiles > SPLIT_K_MAX_TILES || nt < 16) return 1;
    int s = 512 / tiles;
    if (s > SPLIT_K_MAX) s = SPLIT_K_MAX;
    if (s > nt / 8) s = nt / 8;
    return s < 2 ? 1 : s;
}

// what both split-K forms need of the caller's workspace and of the operands the reduce kernel reads 8 channels at a time
bool split_operands_ok(const GemmParams& p, int s) {
    return p.workspace_bytes >= (long)s * p.M * p.N * 4 && !misaligned(p.workspace, 15) &&
           !(p.residual && (misaligned(p.residual, 15) || (p.ldr & 7))) && !(p.ldc & 7) && !misaligned(p.C, 15);
}

// THE rule for GEMM_STAMPS: is there a stamped instantiation for this launch?  conv.hip builds one (the patch-staged 3x3 kernel, 160 channels wide:
// conv_patch_tile) and gemm.hip one per tile width of its plain two-stage kernel with the wide 16-bit epilogue and no residual; no other form
// carries timing code.  The launch's colstats pointer is its stamp buffer, so no rule about statistics applies to it.
bool stamps_built(const GemmParams& p) {
    if ((p.flags & (GEMM_GEGLU | GEMM_OUT_F32 | GEMM_NARROW_EPILOGUE)) || (p.N & 7) || p.residual || p.C32 || p.gn_ab) return false;
    int arg;
    if (p.mode == 1) return conv_kernel_choice(p, &arg) == 1;
    return p.mode == 0 && (forced_variant(p.flags) == 0 || forced_variant(p.flags) == 5 || forced_variant(p.flags) == 6);
}

int validate(GemmParams& p) {
    p.split_k = 1; p.kt_per_split = 0;
    if (!p.A || !p.Wt || (!p.C && !p.C32) || !p.zeros) return VFACE_ERR_ARG;
    if (p.M <= 0 || p.N <= 0 || p.K <= 0) return VFACE_ERR_ARG;
    if (p.mode == 1 && p.ntaps == 0) { p.KH = p.KW = 3; p.ntaps = 9; p.pad_x = p.pad; }   // the plain 3x3 window
    if ((p.flags & GEMM_STAMPS) && !stamps_built(p)) return VFACE_ERR_SHAPE;
    if (p.res_f32 && !p.residual) p.res_f32 = 0;
    if (p.res_f32 || p.C32) {
        // the fp32 residual stream lives in the wide epilogue (and the split-K reduce) only
        if ((p.flags & (GEMM_GEGLU | GEMM_OUT_F32 | GEMM_NARROW_EPILOGUE)) || (p.N & 7)) return VFACE_ERR_SHAPE;
        if (p.C32 && (misaligned(p.C32, 15) || (p.ldc32 & 3))) return VFACE_ERR_ALIGN;
        if (p.res_f32 && (misaligned(p.residual, 15) || (p.ldr & 3))) return VFACE_ERR_ALIGN;
        if (p.out_phase && p.res_f32) return VFACE_ERR_SHAPE;
    }
    if ((p.K & 7) || (p.Kw & 7) || (p.lda & 7) || (p.ldw & 7) || (p.N & 3) || (p.ldc & 3)) return VFACE_ERR_ALIGN;
    if (((uintptr_t)p.A | (uintptr_t)p.Wt | (uintptr_t)p.zeros) & 15) return VFACE_ERR_ALIGN;
    if (misaligned(p.C, 7)) return VFACE_ERR_ALIGN;
    if (p.C32 && (misaligned(p.C, 15) || (p.ldc & 7))) return VFACE_ERR_ALIGN;
    if (p.residual && (misaligned(p.residual, 7) || (p.ldr & 3))) return VFACE_ERR_ALIGN;
    if (p.rowbias && (p.rows_per_sample <= 0 || (p.ld_rowbias & 3))) return VFACE_ERR_ARG;
    if ((p.flags & GEMM_GEGLU) && ((p.N & 31) || (p.flags & GEMM_OUT_F32) || p.residual || p.rowbias)) return VFACE_ERR_SHAPE;
    if (p.colstats && ((p.flags & (GEMM_GEGLU | GEMM_OUT_F32)) || (p.ld_colstats & 1) || misaligned(p.colstats, 15))) return VFACE_ERR_ARG;
    if (p.A2 && (p.K1 <= 0 || (p.K1 % BK) || (p.lda2 & 7) || misaligned(p.A2, 15))) return VFACE_ERR_ALIGN;
    if (p.A2 && p.mode == 1 && ((p.Cin % 64) || ((p.K - p.K1) % BK) || p.upsample || p.a2_row_mod)) return VFACE_ERR_SHAPE;
    if (p.mode == 1) {
        if (p.Cin <= 0 || (p.Cin & 7) || p.ntaps != p.KH * p.KW || p.ntaps > 9) return VFACE_ERR_SHAPE;
        if (p.A2 ? (p.K1 != p.ntaps * p.Cin || p.K <= p.K1) : (p.K != p.ntaps * p.Cin)) return VFACE_ERR_SHAPE;
        if (p.out_phase && (p.residual || (p.flags & GEMM_OUT_F32) || (p.N & 7))) return VFACE_ERR_SHAPE;
        if (p.out_phase && p.colstats && ((p.OH * p.OW) & 63)) return VFACE_ERR_SHAPE;
        if (p.stride != 1 && p.stride != 2) return VFACE_ERR_SHAPE;
    }
    // extents of the operand views for the buffer descriptors (bytes; must stay below 4 GiB - 16)
    const unsigned long es = 2, lim = 0xFFFFFFF0ul;
    const unsigned long rows = p.mode == 1 ? (unsigned long)(p.M / (p.OH * p.OW)) * p.H * p.W : (unsigned long)p.M;
    const unsigned long ab = ((rows - 1) * (unsigned long)p.lda + (p.mode == 1 ? p.Cin : (p.A2 ? p.K1 : p.K))) * es;
    const unsigned long wb = ((unsigned long)(p.N - 1) * p.ldw + p.Kw) * es;
    unsigned long a2b = 0;
    if (p.A2) a2b = ((unsigned long)((p.a2_row_mod > 0 ? p.a2_row_mod : p.M) - 1) * p.lda2 + (p.K - p.K1)) * es;
    if (ab >= lim || wb >= lim || a2b >= lim) return VFACE_ERR_SHAPE;
    p.a_bytes = (unsigned)ab; p.w_bytes = (unsigned)wb; p.a2_bytes = (unsigned)a2b;
    if (p.gn_ab) {
        if (p.mode != 1 || p.M <= 0) return VFACE_ERR_SHAPE;
        const unsigned long nimg = (unsigned long)(p.M / (p.OH * p.OW));
        const unsigned long gb = ((nimg - 1) * (unsigned long)p.ld_gn_ab + p.Cin) * 8ul;
        if (gb >= lim) return VFACE_ERR_SHAPE;
        p.gn_ab_bytes = (unsigned)gb;
    }
    return VFACE_OK;
}

// extents of the output, residual and carrier views for the epilogue's buffer descriptors (gemm_big.hip, inconv.hip); false: 4 GiB - 16 or more
bool output_extents(GemmParams& p) {
    const unsigned long nout = (p.flags & GEMM_GEGLU) ? (unsigned long)p.N / 2 : (unsigned long)p.N, lim = 0xFFFFFFF0ul;
    const unsigned long cb = p.C ? ((unsigned long)(p.M - 1) * p.ldc + nout) * 2ul : 0ul;
    const unsigned long rb = p.residual ? ((unsigned long)(p.M - 1) * p.ldr + p.N) * (p.res_f32 ? 4ul : 2ul) : 0ul;
    const unsigned long c32b = p.C32 ? ((unsigned long)(p.M - 1) * p.ldc32 + p.N) * 4ul : 0ul;
    p.c_bytes = (unsigned)cb; p.res_bytes = (unsigned)rb; p.c32_bytes = (unsigned)c32b;
    return cb < lim && rb < lim && c32b < lim;
}

// the patch-staged kernel on TP x TP-pixel tiles: window KH x KH, tile width bn (convolutions and the GEMM_PATCH form)
void plan_patch(VfGemmPlan& pl, int kernel, int bn) {
    const GemmParams& p = pl.p;
    const int KH = p.KH, KW = p.KW, npieces = ((TP + KW - 1) * (TP + KH - 1) + 7) / 8, nslot = (KH * KW % 3 == 0) ? 3 : 4;
    const int ntm = (p.M / (p.OH * p.OW)) * (p.H / TP) * (p.W / TP), ntn = p.N / bn;
    pl.kernel = kernel; pl.bn = bn; pl.mode = KH; pl.form = p.gn_ab ? 4 : (p.flags & GEMM_STAMPS) ? 3 : residual_form(p);
    pl.lds_bytes = 2 * npieces * 1024 + nslot * bn * 128 + (KH == 3 ? 2048 : 0); pl.grid_x = ntm * ntn;
    const double a_mt = (double)(TP + KW - 1) * (TP + KH - 1) * (p.Cin + (p.A2 ? (p.K - p.K1) : 0)) * 2.0;
    pl.p.tile_group = tile_group(ntm, ntn, a_mt, (double)bn * p.K * 2.0, false);
}

}  // namespace

int vf_plan_gemm(const GemmParams& p_in, int persistent_grid, VfGemmPlan* plan) {
    VfGemmPlan& pl = *plan;
    pl = VfGemmPlan{};
    pl.p = p_in; pl.grid_y = 1;
    GemmParams& p = pl.p;
    const int rc = validate(p);
    if (rc != VFACE_OK) return rc;
    // 1. the input convolution
    if (conv_in16_ok(p)) {
        output_extents(p);      // (conv_in16_ok has bounded them)
        const int nslices = p.M / 64;
        // a workgroup = the (up to) four 80-channel slices of a run of pixel slices; about two workgroups per CU in flight, each wave keeping its 26
        // KB of weight fragments over its whole run (at least 4 slices where the launch has them)
        int spw = (nslices + 511) / 512;
        if (spw < 4) spw = nslices < 4 ? nslices : 4;
        pl.kernel = VF_KERNEL_CONV_IN16; pl.bn = VF_IN16_CH; pl.slices_per_wg = spw;
        pl.grid_x = (nslices + spw - 1) / spw; pl.grid_y = (p.N / VF_IN16_CH + 3) / 4;
        return VFACE_OK;
    }
    // 2. convolutions: the patch-staged kernel, or its 8x8 form (four images per workgroup, K split over channel chunks, then the split-K reduce)
    int karg = 0;
    const int kchoice = conv_kernel_choice(p, &karg);
    if (kchoice == 1) { plan_patch(pl, VF_KERNEL_CONV_PATCH, karg); return VFACE_OK; }
    if (kchoice == 2 && p.workspace && split_operands_ok(p, karg) && (p.M % 64) == 0) {
        p.split_k = karg;
        pl.kernel = VF_KERNEL_CONV_Q8; pl.bn = 128; pl.mode = 3; pl.reduce = true;      // (fp32 partials even where the split is 1)
        pl.lds_bytes = 2 * 50 * 1024 + 3 * 128 * 128 + 2048; pl.grid_x = ((p.M / 64 + 3) / 4) * (p.N / 128) * p.split_k;
        return VFACE_OK;
    }
    // 3. a plain GEMM through the patch kernel (A/B): M / 256 images of 16 x 16 pixels, no window
    if (const int bn = (p.mode == 0 && (p.flags & GEMM_PATCH) && !forced_variant(p.flags)) ? gemm_patch_tile(p) : 0) {
        p.H = p.W = p.OH = p.OW = TP; p.Cin = 0; p.K1 = 0; p.KH = p.KW = 3; p.ntaps = 9; p.pad = p.pad_x = 0; p.stride = 1; p.upsample = 0;
        p.A2 = p.A; p.lda2 = p.lda; p.a2_bytes = p.a_bytes; p.a2_row_mod = 0;
        plan_patch(pl, VF_KERNEL_GEMM_PATCH, bn);
        return VFACE_OK;
    }
    // 4. long token matrices: the 256-row tile
    if (p.mode == 0 && gemm_big_choice(p)) {
        if (!output_extents(p)) return VFACE_ERR_SHAPE;
        const int bn = gemm_big_width(p), ntn = p.N / bn, ntm = (p.M + BM2 - 1) / BM2;
        pl.kernel = VF_KERNEL_GEMM_BIG; pl.bn = bn; pl.form = p.C32 ? 3 : (p.flags & GEMM_GEGLU) ? 1 : p.residual ? 2 : 0;
        pl.lds_bytes = 2 * (BM2 * 128 + bn * 128); pl.grid_x = ntn * ntm;
        p.tile_group = tile_group(ntm, ntn, (double)BM2 * p.K * 2.0, (double)bn * p.K * 2.0, true);
        return VFACE_OK;
    }
    // 5. gemm.hip
    if (p.gn_ab) return VFACE_ERR_SHAPE;   // the fused input normalisation exists in the patch-staged kernel only
    const int variant = pick_variant(p);
    const bool wide = variant == 5 || variant == 6;      // two-stage schedules: the ones the fp32 stream, odd windows and split-K run on
    if (!variant_exists(variant)) return VFACE_ERR_SHAPE;
    if ((p.res_f32 || p.C32) && !wide) return VFACE_ERR_SHAPE;
    if (p.mode == 1 && (p.ntaps != 9 || p.out_phase || p.A2) && !wide) return VFACE_ERR_SHAPE;
    if ((p.flags & GEMM_GEGLU) && (variant == 6 || variant == 8)) return VFACE_ERR_SHAPE;
    if (p.colstats && variant > 8) return VFACE_ERR_SHAPE;
    // 6. split-K
    if (p.workspace && !p.out_phase && wide && !forced_variant(p.flags) && !(p.flags & GEMM_STAMPS)) {
        const int s = split_for(p.M, p.N, p.K, p.flags, p.rows_per_sample);
        if (s > 1 && split_operands_ok(p, s)) {
            const int nt = (p.K + BK - 1) / BK;
            p.split_k = s;
            p.kt_per_split = (nt + s - 1) / s;
            if ((long)(s - 1) * p.kt_per_split >= nt) p.split_k = (nt + p.kt_per_split - 1) / p.kt_per_split;  // no empty split
        }
    }
    pl.kernel = VF_KERNEL_GEMM; pl.bn = (variant == 5 || variant == 7) ? 128 : 160; pl.stages = wide ? 2 : 1;
    pl.mode = p.mode == 0 ? 0 : (p.Cin % 64 == 0 ? 1 : 2); pl.form = (p.flags & GEMM_STAMPS) ? 3 : residual_form(p); pl.reduce = p.split_k > 1;
    pl.lds_bytes = pl.stages * (BM + pl.bn) * BK * 2;
    const int ntn = (p.N + pl.bn - 1) / pl.bn, ntm = (p.M + BM - 1) / BM, ntiles = ntm * ntn;
    // 7. persistent form: only where a workgroup would get more than one tile and the wide epilogue applies (measured on the UNet's shapes: +1..3 % for
    // the implicit convolutions, +-2 % noise for plain GEMMs, which keep one tile per workgroup unless GEMM_PERSIST asks otherwise), and only in the
    // instantiations that exist: not the generic window, not with a residual (they spilled 22-41 registers: gemm.hip launch_one)
    pl.persistent = wide && pl.mode != 2 && p.split_k == 1 && pl.form == 0 &&
                    !(p.flags & (GEMM_OUT_F32 | GEMM_NARROW_EPILOGUE | GEMM_NO_PERSIST | GEMM_STAMPS)) &&
                    !(p.N & 7) && ntiles > persistent_grid && (pl.mode != 0 || (p.flags & GEMM_PERSIST));
    pl.grid_x = pl.persistent ? persistent_grid : ntiles * p.split_k;
    // 8. tile order of the plain GEMM
    if (pl.mode == 0 && p.split_k == 1 && !p.tile_group)
        p.tile_group = (p.flags & GEMM_GN8) ? 8 : tile_group(ntm, ntn, (double)BM * p.K * 2.0, (double)pl.bn * p.K * 2.0, true);
    return VFACE_OK;
}

long vf_splitk_workspace_bytes(int M, int N, int K, int flags, int rows_per_sample) {
    int s = split_for(M, N, K, flags, rows_per_sample);
    if (s < 2) s = 0;
    if (rows_per_sample == 64 && (N % 128) == 0 && !(flags & (GEMM_GEGLU | GEMM_OUT_F32))) {
        // a 3x3 convolution on 8x8 images may take the Q8 form, which always ends in fp32 partials: room for the largest split conv_q8_split can
        // choose for this N
        const int s8 = q8_grid_split(N) < 1 ? 1 : q8_grid_split(N);
        if (s8 > s) s = s8;
    }
    return (long)s * M * N * 4;
}

int vf_conv_uses_patch_kernel(int H, int W, int Cin, int Cout, int window, int stride, int upsample, int flags) {
    if (H <= 0 || W <= 0 || Cin <= 0 || Cout <= 0 || (window != 2 && window != 3)) return 0;
    GemmParams p{};
    p.mode = 1; p.H = H; p.W = W; p.OH = H; p.OW = W; p.Cin = Cin; p.N = Cout; p.stride = stride; p.upsample = upsample ? 1 : 0;
    p.KH = p.KW = window; p.ntaps = window * window; p.pad = 1; p.pad_x = 1; p.flags = flags;
    p.K = p.K1 = p.ntaps * Cin; p.rows_per_sample = H * W;      // (no batch: the rule reads the per-sample geometry only)
    int arg;
    return conv_kernel_choice(p, &arg);
}
