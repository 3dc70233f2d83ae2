/* vface_hip.h -- C ABI of libvface_hip.so: the MI355X (gfx950) kernels behind VFace's per-frame DDIM
 * denoising hot path.
 *
 * The reference (Sanoojan/VFace, REFace/) has no FFI: its extension point is Python -- nn.Module
 * forwards and the closure `register_spa_attn_injection` installs on every `attn1`
 * (REFace/ldm/models/pnp_utils.py:57,289-339).  Each entry point below names the reference
 * call site(s) whose device work it replaces; the Python side that binds them (ctypes, raw device
 * pointers + the current HIP stream) is vface_amd/hip.py, and INTEGRATION.md shows the binding a
 * maintainer of the reference would add.
 *
 * Conventions
 *  - every pointer is a DEVICE pointer unless said otherwise; no allocation, no synchronisation, no
 *    global state inside: calls only enqueue kernels on `stream` (a hipStream_t passed as void*), so
 *    they can be captured into a hipGraph; re-entrant per stream.
 *  - `dtype`: 0 = fp16 (the reference's autocast type), 1 = bf16.  Accumulation, softmax and
 *    normalisation statistics are always fp32.
 *  - activations are token-major / NHWC: element (sample b, pixel p, channel c) at
 *    base[(b*HW + p)*ld + c]; `ld` lets a tensor be a channel slice of a wider (concatenated) buffer.
 *  - 16-bit rows must be 16-byte aligned and channel counts multiples of 8.
 *  - return value: 0 = ok; negative = VFACE_ERR_* (nothing was launched).  No exceptions cross the ABI.
 */
#ifndef VFACE_HIP_H
#define VFACE_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VFACE_ABI_VERSION 8   /* 8 (later additions, nothing changed): + vface_clip_patches, vface_clip_embed, vface_act, vface_cond_mix (the conditioning stage), vface_attention at dh = 64 and vface_yuv420_to_rgb (video in); 8: 7 minus the composite hooked-attn1 call and its workspace query (a hooked attn1 is a sequence of single-kernel calls issued by the caller), nothing else changed; 7 (later additions, nothing changed): + vface_temporal_gauss_halo, vface_adain_rows_workspace_bytes, vface_adain_rows, vface_adain_reduce_scale (the frame-sharded temporal / adaIn edits); 7: + the VFACE_TUNE_BIG_W256 / VFACE_TUNE_BIG_W320 flag bits of vface_gemm (the big tile's width: 256 x 256 beside 256 x 320, chosen by the library per launch; same results), nothing else of 6 changed; 6: + the VFACE_TUNE_BIG_TILE / VFACE_TUNE_NO_BIG_TILE flag bits of vface_gemm (csrc/gemm_big.hip: the 256 x 320 tile, chosen by the library from 192 tiles on; same results), nothing else of 5 changed; 5: + vface_st_front, vface_attn_out_ffn_fused, vface_attn_out_ffn_proj_fused, vface_gn_silu_conv3x3_small, vface_linear_small; vface_attention's v_sets carries the live-set count in bits 8..15, vface_pack_unet_input / vface_ddim_step take the two-branch batch; nothing else of 4 changed (4: + vface_ffn_fused, the flow-producer glue, the paste-back entry points) */

#define VFACE_OK 0
#define VFACE_ERR_ARG (-1)
#define VFACE_ERR_ALIGN (-2)
#define VFACE_ERR_SHAPE (-3)
#define VFACE_ERR_DTYPE (-4)
#define VFACE_ERR_LAUNCH (-5)
#define VFACE_ERR_WORKSPACE (-6)

#define VFACE_F16 0
#define VFACE_BF16 1

/* The flags word of vface_gemm / vface_conv3x3*: every bit the library reads is defined here (csrc/dispatch.hpp and vface_amd/hip.py name the same values) */
#define VFACE_EPI_GEGLU 1   /* out[m][c] = (acc_val + b) * gelu(acc_gate + b); Wt rows packed by vface layout */
#define VFACE_EPI_OUT_F32 2 /* store fp32 instead of the 16-bit type */
#define VFACE_TUNE_VARIANT(v) ((v) << 8) /* bits 8..11: force GEMM schedule variant v of csrc/gemm.hip: 5 | 6 = 128 | 160 channels per tile, two LDS stages; 7 | 8 = the same, one stage; 11..15 = 8 without column statistics (15: no K split either).  0 = automatic; 1..4, 9, 10 are refused (VFACE_ERR_SHAPE) */
#define VFACE_TUNE_NO_XCD_REMAP 0x1000     /* A/B: csrc/gemm.hip's plain GEMM walks its tiles in launch order, not in the XCD-aware order */
#define VFACE_TUNE_NO_SETPRIO 0x2000       /* A/B: csrc/gemm.hip: no raised wave priority around the MFMAs; csrc/conv.hip: the late waves issue their half of a K tile's loads apart */
#define VFACE_TUNE_STAMPS 0x4000           /* diagnostic (tools/stamp_gemm.py, tools/stamp_conv.py): run the stamped instantiation; colstats receives cycle counts per workgroup and wave, not statistics.  Built for the fp16 plain GEMM of variants 5 and 6 with the wide 16-bit epilogue and no residual, and for the patch-staged 3x3 convolution with Cout % 160 == 0; VFACE_ERR_SHAPE elsewhere */
#define VFACE_TUNE_NARROW_EPILOGUE 0x8000  /* A/B: csrc/gemm.hip stores straight from the accumulator layout (8 bytes per lane), without the LDS transpose */
#define VFACE_CONV_PAD_TRAILING 0x40000 /* vface_conv3x3: zero padding (left 0, right 1, top 0, bottom 1) instead of 1 all round */
#define VFACE_TUNE_NO_PERSISTENT 0x10000 /* one workgroup per output tile even where the persistent form would run */
#define VFACE_TUNE_PERSISTENT 0x20000    /* persistent form for a plain GEMM too (default: implicit convolutions only) */
#define VFACE_TUNE_NO_PATCH 0x80000      /* convolutions: never the patch-staged kernel (im2col-style staging, one load per tap) */
#define VFACE_TUNE_PATCH 0x100000        /* convolutions: the patch-staged kernel wherever the shape allows, however small the grid */
#define VFACE_TUNE_GN8 0x8000000          /* A/B: fixed column groups of 8 n-tiles in the plain GEMM's XCD-aware tile order (default: per-launch width) */
#define VFACE_TUNE_NO_Q8 0x4000000        /* A/B: 3x3 convolutions on 8x8 images stay on the im2col kernel (default: four images per workgroup through the patch-staged kernel + split-K reduce) */
#define VFACE_TUNE_PATCH_BN160 0x2000000  /* A/B: the patch-staged kernel's 160-channel tile wherever it divides Cout (default: the width whose one-per-CU grid has the cheaper last round) */
#define VFACE_TUNE_F32_TRANSPOSE 0x1000000 /* A/B: the epilogue's LDS transpose in fp32 even where nothing reads the fp32 sum (default there: 16 bits) */
#define VFACE_TUNE_BIG_TILE 0x10000000     /* vface_gemm: the 256 x 320 tile (csrc/gemm_big.hip) whenever the launch qualifies (N % 320 == 0, K % 64 == 0, 16-bit output, bias / GEGLU / fp32 residual only), however few tiles; default: from 192 tiles on.  Same bits as the 128-row kernel */
#define VFACE_TUNE_NO_BIG_TILE 0x20000000  /* A/B: never the 256 x 320 tile */
#define VFACE_TUNE_BIG_W256 0x200000       /* vface_gemm, big tile: 256 channels per tile wherever N % 256 == 0 (default: the width whose one-workgroup-per-CU grid takes fewer tile-times).  Same bits */
#define VFACE_TUNE_BIG_W320 0x400000       /* A/B: always 320 channels per tile */
/* (VFACE_TUNE_PATCH on vface_gemm: run a plain GEMM with M % 256 == 0, K % 64 == 0, N % 128|160 == 0, no GEGLU / fp32-only output
 *  through the patch-staged kernel's 256-row tile -- same bits as the default kernel, measured 3-18 % SLOWER on the UNet's shapes
 *  (tools/bench_kernels.py "patch256"): an A/B switch, never chosen automatically) */

/* fusion modes of the attn1 hook (pnp_utils.py:133-262): which single-kernel calls the caller issues between the projection and vface_attention */
#define VFACE_FUSION_NONE 0       /* switch_on == False, or unpatched CrossAttention.forward */
#define VFACE_FUSION_REPLACE 1    /* :133-143 and chunks == 2 (:259-262): q,k of every chunk <- chunk 0 */
#define VFACE_FUSION_LINEAR 2     /* "fft"/"flow_fix"/"fft_vfixed"/"mix": q,k <- own*W_a + chunk0*W_b (folded weights) */

int vface_abi_version(void);
const char* vface_error_string(int code);
/* Always 0 since round 4: the experimental GEMM schedules VFACE_TUNE_VARIANT(1..4, 9, 10) of rounds 1-3 (all measured slower,
 * HISTORY.md) were removed; those variant codes are refused with VFACE_ERR_SHAPE.  Kept so that version-4 callers still link. */
int vface_gemm_variants_built(void);

/* The fp32 residual stream (optional last argument of the GEMM-family calls; NULL = everything 16-bit).
 * The reference adds every residual in the autocast type (openaimodel.py:274 `skip_connection(x) + h`,
 * attention.py:240-242 `attn(...) + x`, :289 `x + x_in`); carrying those sums in fp32 between kernels removes the
 * largest single share of the 16-bit path's whole-network error.  A HOST struct, read during the call:
 *   residual32 / ldr32   the residual operand as fp32 [M][ldr32] -- used INSTEAD of the 16-bit `residual` argument
 *   out32 / ldo32        fp32 [M][ldo32] receives acc + bias + rowbias + residual before the rounding to 16 bits; the
 *                        16-bit output pointer of the call may then be NULL (no 16-bit copy wanted).  With `colstats`
 *                        the statistics are those of the fp32 values (what a GroupNorm reading out32 normalises).
 * 16-byte aligned, ld % 4 == 0; needs N % 8 == 0 and no GEGLU / OUT_F32 epilogue. */
typedef struct vface_stream32 {
    const float* residual32;
    int64_t ldr32;
    float* out32;
    int64_t ldo32;
    /* Convolutions only -- GroupNorm + SiLU fused into the operand path (openaimodel.py:201-205,225-232 `GroupNorm32 -> SiLU ->
     * conv`): in_scale_shift = fp32 [nimg][ld_scale_shift][2] pairs (a, b) per (image, input channel), from
     * vface_groupnorm_coeffs_from_cols; the matrix cores then see act(x * a + b) (act = SiLU if in_silu, else identity),
     * rounded once to the 16-bit type, zero padding applied AFTER the normalisation as in the reference.  Needs a launch
     * that runs the patch-staged kernel (vface_conv_uses_patch_kernel); otherwise VFACE_ERR_SHAPE.  NULL = off. */
    const float* in_scale_shift;
    int64_t ld_scale_shift;
    int in_silu;
} vface_stream32;

/* C[M][N] (+)= A[M][K] * Wt[N][K]^T with fused epilogue.
 * Replaces every nn.Linear / 1x1 conv on the path: to_q/to_k/to_v/to_out (attention.py:161-177),
 * GEGLU + FeedForward (attention.py:37-64), proj_in/proj_out (attention.py:261-276), ResBlock
 * emb_layers / skip_connection (openaimodel.py:218-241), time_embed (openaimodel.py:631-636).
 * A2 (optional): columns [K1, K) of the A operand come from A2[m % a2_row_mod][k - K1] (K1 % 64 == 0).
 * rowbias: fp32 [M/rows_per_sample][ld_rowbias] added per sample (time-embedding / cross-attention vector).
 * colstats (optional): fp32 [ceil(M/64)][ld_colstats][2] receives, per 64-row slice and output column, the (sum, sum of
 * squares) of the values as stored -- the statistics a following GroupNorm needs (vface_groupnorm_finalize_cols). */
int vface_gemm(const void* A, int64_t lda, const void* A2, int64_t lda2, int K1, int a2_row_mod, const void* Wt,
               int64_t ldw, int M, int N, int K, const float* bias, const float* rowbias, int rows_per_sample,
               int ld_rowbias, const void* residual, int64_t ldr, void* C, int64_t ldc, const void* zeros, int flags,
               int dtype, float* colstats, int64_t ld_colstats, void* workspace, int64_t workspace_bytes, void* stream,
               const vface_stream32* s32);

/* Bytes of device scratch a vface_gemm / vface_conv3x3 launch of this shape (M rows = nimg*OH*OW for a convolution,
 * K = 9*Cin) can use to split its K loop over more workgroups when M x N alone would leave most of the 256 CUs idle
 * (fp32 partial tiles summed in a fixed order: results stay reproducible).  0 = this shape is never split.
 * `workspace` may be NULL or smaller: the launch then runs unsplit.  rows_per_sample (OH*OW of a convolution, h*w of a
 * token matrix; <= 1 = unknown) makes the decision a function of the per-sample geometry only, so the bits of a sample
 * do not depend on the batch it is launched in; vface_gemm uses its own rows_per_sample argument the same way. */
int64_t vface_splitk_workspace_bytes(int M, int N, int K, int flags, int rows_per_sample);

/* Y = conv3x3(X) over NHWC, padding 1, stride 1|2, optional nearest x2 upsampling of X first, as an
 * implicit GEMM (nothing materialised).  Wt is packed [Cout][K = 9*Cin]: K order (64-channel chunk, tap, channel)
 * when Cin % 64 == 0, else (tap, channel) -- vface_amd/packing.py::pack_conv3x3.
 * Replaces nn.Conv2d in ResBlock.in_layers/out_layers (openaimodel.py:201-232), Downsample.op (:151-153),
 * Upsample.conv after F.interpolate (:108-118), input_blocks.0 (:668-674) and `out` (:821-825). */
int vface_conv3x3(const void* X, int64_t ldx, int nimg, int H, int W, int Cin, const void* Wt, int64_t ldw, int Cout,
                  int stride, int upsample, const float* bias, const float* rowbias, int ld_rowbias,
                  const void* residual, int64_t ldr, void* Y, int64_t ldy, const void* zeros, int flags, int dtype,
                  float* colstats, int64_t ld_colstats, void* workspace, int64_t workspace_bytes, void* stream,
                  const vface_stream32* s32);

/* Which kernel a vface_conv3x3 / vface_conv3x3_plus_1x1 (window = 3) / vface_upsample2x_conv3x3_phase (window = 2) launch of this
 * geometry runs: 1 = the patch-staged kernel (conv.hip: stride 1, H and W multiples of 16, Cin % 64 == 0, Cout % 160 == 0 or
 * % 128 == 0, 16-bit output, and a grid of at least 160 tiles at the nominal batch of 24 samples -- NOMINAL_BATCH_CLIP of
 * csrc/dispatch.cpp, where every rule of this family lives --, or VFACE_TUNE_PATCH), 2 = its 8x8 form (3x3 window on 8 x 8 images,
 * Cout % 128 == 0: four images per workgroup, K split over channel chunks by the grid at NOMINAL_BATCH_STREAM = 48 samples, then
 * the split-K reduce; taken when the caller passes the workspace vface_splitk_workspace_bytes asks for), 0 = the im2col-style
 * implicit GEMM (gemm.hip).  The answer depends on the per-sample geometry only, never on a batch.  For measurement harnesses
 * (bench.py prices the two kernels separately). */
int vface_conv_uses_patch_kernel(int H, int W, int Cin, int Cout, int window, int stride, int upsample, int flags);

/* Y = conv3x3(X) + X2 W2^T + bias: the second convolution of a ResBlock together with the block's 1x1 shortcut
 * (openaimodel.py:228-232, 274 `skip_connection(x) + h`; diffusionmodules/model.py:137-141 `nin_shortcut`), accumulated in
 * one K loop -- the shortcut's own launch, its 16-bit intermediate and the residual read disappear.  Wt: [Cout][9*Cin + C2],
 * the packed 3x3 weights followed by the 1x1 weights; X2: [nimg*H*W][ldx2 >= C2].  Cin % 64 == 0, C2 % 64 == 0, stride 1. */
int vface_conv3x3_plus_1x1(const void* X, int64_t ldx, int nimg, int H, int W, int Cin, const void* X2, int64_t ldx2, int C2,
                           const void* Wt, int64_t ldw, int Cout, const float* bias, const float* rowbias, int ld_rowbias,
                           void* Y, int64_t ldy, const void* zeros, int flags, int dtype, float* colstats,
                           int64_t ld_colstats, void* workspace, int64_t workspace_bytes, void* stream,
                           const vface_stream32* s32);

/* One output-parity phase of conv3x3(nearest_upsample2x(X)) (Upsample: openaimodel.py:108-118, diffusionmodules/model.py:
 * 55-58).  Every output pixel (2i+py, 2j+px) of the upsampled convolution sees only a 2x2 block of source pixels, so the
 * nine taps collapse -- exactly -- into four with pre-summed weights (vface_amd/packing.py::pack_upsample_phases): 4/9 of
 * the multiply-adds of running the 3x3 window over the upsampled image.  X: [nimg*H*W][ldx >= Cin]; Y: the FULL output
 * [nimg*2H*2W][ldy]; this call writes its rows (2i+py, 2j+px) only; call it for the four (py, px).  Wt: that phase's
 * [Cout][4*Cin] matrix.  No residual, 16-bit output, Cout % 8 == 0.  colstats (optional, H*W % 64 == 0): the
 * [nimg*4*H*W/64][ld_colstats][2] buffer of the FULL output; each phase fills its own quarter of every sample's slices
 * (sums over a sample are what vface_groupnorm_finalize_cols takes, so the slice order inside a sample is free). */
int vface_upsample2x_conv3x3_phase(const void* X, int64_t ldx, int nimg, int H, int W, int Cin, const void* Wt, int64_t ldw,
                                   int Cout, int py, int px, const float* bias, const float* rowbias, int ld_rowbias, void* Y,
                                   int64_t ldy, const void* zeros, int flags, int dtype, float* colstats,
                                   int64_t ld_colstats, void* stream, const vface_stream32* s32);

/* O = softmax(Q K^T * scale) V per (sample, head), streaming softmax, no [n x n] matrix.
 * Replaces attention.py:206-220 / pnp_utils.py:270-285, and at dh = 64 the self-attention of the CLIP image tower.  Output sample b uses q,k of sample qk_map[b] and
 * v of sample v_map[b] (NULL = identity): the zero-copy form of the hook's q/k/v row assignments. */
int vface_attention(const void* Q, const void* K, const void* V, int64_t ldq, int64_t ldk, int64_t ldv, int64_t bsq,
                    int64_t bsk, int64_t bsv, const int32_t* qk_map, const int32_t* v_map, void* O, int64_t ldo,
                    int64_t bso, int B, int heads, int n, int nk, int dh, float scale, int dtype, int v_sets,
                    int set_stride, void* stream);
/* v_sets > 1 ("shared scores", the "replace" injection pnp_utils.py:133-143 / :259-262 where every chunk takes q,k of
 * chunk 0): B counts the q/k samples; for g < v_sets output sample b + g*set_stride = softmax(q_b k_b^T * scale) v_s,
 * s = v_map[b + g*set_stride] (or b + g*set_stride), the probabilities computed once per (b, head).  Supported for
 * v_sets 2|3 and dh 8|16|32|40 (vface_attention_shared_scores_supported); other shapes: use qk_map.  * Bits 8..15 of v_sets: the number of LIVE sets (0 = all; supported: 2 of 3): sets g >= live are neither read nor written --
 * a batch that came without its last chunk (the sampler's dead-branch elimination) -- while every instruction that touches a live
 * set is that of the full call, so the live outputs are bit-identical to it. */
int vface_attention_shared_scores_supported(int dh, int v_sets);

/* y = LayerNorm(x) * gamma + beta, fp32 statistics (attention.py:231-233).  in_f32: x is the fp32 residual-stream
 * copy [M][ldx] (ldx in floats); y is always 16-bit (its consumer is a GEMM). */
int vface_layernorm(const void* x, int64_t ldx, const float* gamma, const float* beta, void* y, int64_t ldy, int M,
                    int C, float eps, int in_f32, int dtype, void* stream);

/* GroupNorm statistics (mean, rstd) per (image, group) -> stats[nimg][groups][2] fp32;
 * `partial` is scratch of vface_groupnorm_partial_floats() floats.  util.py:214-216, attention.py:76-77. */
int vface_groupnorm_partial_floats(int nimg, int hw, int C, int groups);
int vface_groupnorm_stats(const void* x, int64_t ldx, int nimg, int hw, int C, int groups, float eps, float* partial,
                          float* stats, int in_f32, int dtype, void* stream);
/* The same statistics from producer-side column sums (colstats of vface_gemm / vface_conv3x3); needs hw % 64 == 0. */
int vface_groupnorm_finalize_cols(const float* colstats, int64_t ld_colstats, int nimg, int hw, int C, int groups, float eps,
                                  float* stats, void* stream);
/* The same statistics folded with the affine parameters into per-(image, channel) pairs ab[img][c] = (a, b), a = rstd * gamma[c],
 * b = beta[c] - mean * a -- what vface_stream32.in_scale_shift takes (fp32 [nimg][C][2]). */
int vface_groupnorm_coeffs_from_cols(const float* colstats, int64_t ld_colstats, int nimg, int hw, int C, int groups, float eps,
                                     const float* gamma, const float* beta, float* ab, void* stream);
/* y = (x - mean) * rstd * gamma + beta, then SiLU if `silu` (openaimodel.py:201-205,225-232).  in_f32 (here and in
 * vface_groupnorm_stats): x is the fp32 residual-stream copy (ldx in floats); y is always 16-bit. */
int vface_groupnorm_apply(const void* x, int64_t ldx, const float* stats, const float* gamma, const float* beta,
                          void* y, int64_t ldy, int nimg, int hw, int C, int groups, int silu, int in_f32, int dtype,
                          void* stream);

/* Flow-guided temporal smoothing of a token-major map [F][h*w][C] (temporal_flow.py:40-53,222-237):
 *   dst[f] = alpha * src[f] + one_minus_alpha * bilinear(src[f-1], (x + dx, y + dy)); dst[0] = src[0]
 * (or warped from `prev` with `flow_prev` when given: the previous rank's boundary frame).
 * flow: fp32 [F-1][2][h][w] in pixels of the map; channel 0 = dx, 1 = dy.  Sampling coordinates follow
 * the reference's fp32 operation order exactly (bit-exact gather indices); flags bit 0 = use CUDA-ATen's
 * multiply-by-reciprocal for the scalar division.  dbg_x0/dbg_y0 (optional, int32 [F-1][h][w]) receive
 * the integer north-west corner of every bilinear footprint. */
int vface_flow_warp(const void* src, int64_t ld_src, int64_t fs_src, const void* prev, int64_t ld_prev,
                    const float* flow, const float* flow_prev, void* dst, int64_t ld_dst, int64_t fs_dst, int F,
                    int h, int w, int C, float alpha, float one_minus_alpha, int flags, int32_t* dbg_x0,
                    int32_t* dbg_y0, int dtype, void* stream);

/* Pixel-resolution optical flow -> the latent-resolution field vface_flow_warp takes.  The reference computes
 * RAFT flow between full-resolution frames (temporal_flow.py:163-188 `return_flow`; call site VFace_inference_batch.py:
 * 550-553) and hands it UNRESIZED to the warp of the 64 x 64 maps, where `grid + flow` fails (temporal_flow.py:43); the
 * resample is defined here: out[p][c][y][x] = mean(flow_px[p][c][y*f .. y*f+f-1][x*f .. x*f+f-1]) / f   (fp32 in and out;
 * H, W multiples of `factor`).  RAFT's own weights are third-party: the flow VALUES are outside this library. */
int vface_flow_to_latent(const float* flow_px, float* out, int pairs, int H, int W, int factor, void* stream);

/* ---- optical-flow producer (temporal_flow.py:27-38, 163-188: torchvision raft_large, 20 updates) -----------------
 * The convolutions and the all-pairs correlation of the RAFT-shaped network run through vface_gemm / vface_conv3x3; these are
 * the HBM-bound steps between them, all on token-major [M = nimg*H*W][ld] buffers of the 16-bit compute type.
 * PARITY UNPINNED: torchvision (pinned 0.14.1 by the reference's environment) is third-party, not under the reference tree and
 * not installed; the network is restated from the published architecture in oracle/raft.py and tested against that.
 *
 * vface_im2col: the KH x KW window (7x7, 1x5, 5x1: more than the implicit GEMM's 9 taps, or a non-square shape) as an explicit
 *   matrix out[m][tap*C + c], zero outside the image; C % 8 == 0, ldo >= KH*KW*C.  OH = (H + 2 pad_y - KH) / stride + 1. */
int vface_im2col(const void* X, int64_t ldx, int nimg, int H, int W, int C, int KH, int KW, int stride, int pad_y, int pad_x, void* out,
                 int64_t ldo, int dtype, void* stream);

/* nn.InstanceNorm2d statistics (per image and channel over hw pixels, biased variance): stats [nimg][C][2] = (mean, rstd);
 * `partial` = vface_channel_stats_partial_floats(nimg, hw, C) floats of scratch (fixed summation order: reproducible).
 * The moments are accumulated around each channel's value at the image's first pixel, so their error follows the spread of
 * the data and not mean^2 / var. */
int64_t vface_channel_stats_partial_floats(int nimg, int hw, int C);
int vface_channel_stats(const void* x, int64_t ldx, int nimg, int hw, int C, float eps, float* partial, float* stats, int dtype,
                        void* stream);

/* y = act((x - mean) * rstd + residual): stats NULL = no normalisation (the BatchNorm of the context encoder is folded into its
 * convolutions on the host), residual NULL = none; act 0 none | 1 ReLU | 2 tanh | 3 sigmoid; y (16-bit) and / or y32 (fp32). */
int vface_channel_norm_act(const void* x, int64_t ldx, const float* stats, const void* residual, int64_t ldr, void* y, int64_t ldy,
                           float* y32, int64_t ldy32, int64_t M, int hw, int C, int act, int dtype, void* stream);

/* ConvGRU gates: zr [M][2 hidden] = pre-activations of convz | convr; z = sigmoid -> z [M][ldz]; sigmoid(r) * h32 -> rh. */
int vface_gru_gate(const void* zr, int64_t ldzr, const float* h32, void* z, int64_t ldz, void* rh, int64_t ldrh, int64_t M, int hidden,
                   int dtype, void* stream);
/* h32 = (1 - z) h32 + z tanh(q) in place (fp32 master state), 16-bit copies into h16a / h16b (each may be NULL). */
int vface_gru_update(const void* q, int64_t ldq, const void* z, int64_t ldz, float* h32, void* h16a, int64_t lda, void* h16b, int64_t ldb,
                     int64_t M, int hidden, int dtype, void* stream);

/* F.avg_pool2d(x, 2, 2) over the last two dims of fp32 [R][h][w] (the correlation pyramid). */
int vface_avgpool2_f32(const float* x, float* y, int64_t R, int h, int w, void* stream);

/* CorrBlock.index_pyramid: out[m][l*81 + i*9 + j] = scale * bilinear(vols[l][m], (x + flow.x) / 2^l + i - 4, (y + flow.y) / 2^l + j - 4),
 * zero outside (grid_sample, align_corners = True); vols / hs / ws are HOST arrays of `levels` (<= 4) device pointers and sizes,
 * vols[l] = fp32 [M][hs[l]][ws[l]]; flow32 [M][2]; m = (pair*h + y)*w + x. */
int vface_corr_lookup(const float* const* vols, const int* hs, const int* ws, int levels, const float* flow32, int h, int w, float scale,
                      void* out, int64_t ldo, int64_t M, int dtype, void* stream);

/* flow32 [M][2] += delta32[m][0..1] (delta32 NULL: no change); 16-bit copies of the new flow into columns 0..1 of a / b / c. */
int vface_flow_update(float* flow32, const float* delta32, int64_t ldd, void* a, int64_t lda, void* b, int64_t ldb, void* c, int64_t ldc,
                      int64_t M, int dtype, void* stream);

/* upsample_flow: out [B][2][8h][8w] = sum_k softmax_k(mult * mask32[m][k*64 + fy*8 + fx]) * 8 * flow(neighbour k), zero padded. */
int vface_convex_upsample(const float* mask32, int64_t ldm, const float* flow32, float* out, int B, int h, int w, float mult,
                          void* stream);

/* ---- paste-back of a swapped crop into its original frame (VFace_inference_batch.py:597-636) ----------------
 * The reference runs these steps per frame on the host with numpy, Pillow and torchvision; each entry point replaces one of
 * them on device buffers, with Pillow's 8-bit arithmetic restated exactly (oracle/paste.py is pinned against Pillow itself).
 *
 * vface_frame_to_u8: `torch.clamp((x + 1) / 2, 0, 1)` (:597), `255. * x` and `.astype(np.uint8)` (:606-608).
 *   x planar [frames][3][H][W] in [-1, 1], in_kind 0 fp16 | 1 bf16 | 2 fp32: the arithmetic is fp32 (what `--precision full` computes;
 *   a 16-bit input is widened first); in_kind 3 = fp16 input AND fp16 arithmetic, every operation rounded to float16 as torch and
 *   numpy do on the float16 tensor `--precision autocast` (the reference's default) hands over -- pixels can differ by one between
 *   the two.  out interleaved [frames][H][W][3]. */
int vface_frame_to_u8(const void* x, uint8_t* out, int frames, int H, int W, int in_kind, void* stream);

/* One pass of `Image.resize(size, Image.BILINEAR)` on 8-bit RGB (:608, :623; Pillow Resample.c).  axis 0 resamples along x:
 * src [frames][lines][in_n][3] -> dst [frames][lines][out_n][3]; axis 1 along y: src [frames][in_n][lines][3] -> dst
 * [frames][out_n][lines][3] (lines = the row length).  bounds [out_n][2] = (first input sample, taps), kk [out_n][ksize] =
 * the 22-bit fixed-point taps of Pillow's precompute_coeffs + normalize_coeffs_8bpc -- host work, built once per size pair by
 * vface_amd/scripts/paste_back.py `resample_coeffs` and uploaded.  A resize is the x pass then the y pass. */
int vface_resample_u8(const uint8_t* src, uint8_t* dst, int frames, int in_n, int out_n, int lines, int axis, const int32_t* bounds,
                      const int32_t* kk, int ksize, void* stream);

/* `crop.convert('RGBA') + putalpha(255)`, `.transform(frame.size, Image.PERSPECTIVE, coeffs, Image.BILINEAR)` and
 * `frame.alpha_composite(projected)` (:627-633; Pillow Geometry.c / AlphaComposite.c) in one launch, IN PLACE on `frame`
 * [frames][H][W][3] (the background on entry, the pasted frame on return); crop [frames][crop_h][crop_w][3].
 * The eight coefficients (output pixel centre -> crop coordinates, the rows of `inv_transforms_all`, :625) come either from
 * device memory (coeffs_dev [frames][8] doubles) or, for frames == 1, from the host (coeffs_host[8], passed by value);
 * exactly one of the two must be non-NULL. */
int vface_perspective_paste(const uint8_t* crop, int crop_w, int crop_h, uint8_t* frame, int W, int H, int frames,
                            const double* coeffs_dev, const double* coeffs_host, void* stream);

/* `get_tensor()(orig_image)` (ToTensor + Normalize(0.5, 0.5), :48-56, :611) and `transforms.Resize([H, W])` on the tensor
 * (:612 = bilinear, align_corners false, no antialias): frame [frames][H][W][3] uint8 -> out planar [frames][3][OH][OW] fp32
 * in [-1, 1], the VAE encoder's input for the background round trip (:615-618).  fp32 arithmetic in ATen's order; ATen's CPU
 * kernel differs from it by <= 2 ulp (tests bound it at 2e-6). */
int vface_frame_normalise_resize(const uint8_t* frame, int W, int H, float* out, int OW, int OH, int frames, void* stream);

/* ---- video mux, colour half (REFace/scripts/VFace_inference_batch.py:646-654) ------------------------------------------------
 * The reference writes the pasted frames as PNG (:636) and asks ffmpeg for `-pix_fmt yuv420p -colorspace bt709 -color_range tv`
 * at 10 fps (:646-654); swscale converts on the host.  vface_rgb_to_yuv420 makes that conversion on the device, so the host
 * receives 1.5 bytes per pixel instead of 3 (vface_amd/scripts/mux.py writes them as YUV4MPEG2; H.264 and audio are not built; Motion-JPEG: below).
 *   rgb [frames][H][W][3], the layout the paste-back returns -> out: one I420 frame per frame, frame f at out + f * frame_stride:
 *   Y [H][W], Cb [ch][cw], Cr [ch][cw], cw = (W + 1) / 2, ch = (H + 1) / 2.  Bytes between frames are not written.
 *   Integer arithmetic, stated once in tests/mux_model.py and equal to it bit for bit: 16-bit BT.709 limited-range coefficients,
 *   half-up rounding, luma per pixel, chroma from the mean of the pixels of a 2 x 2 block that exist (centre-sited).  W and H
 *   may be odd; no alignment is required of either pointer or of frame_stride.
 *   NULL pointer, W, H or frames <= 0: VFACE_ERR_ARG; frame_stride < W * H + 2 * cw * ch: VFACE_ERR_SHAPE -- before the first HIP call. */
int vface_rgb_to_yuv420(const uint8_t* rgb, int W, int H, uint8_t* out, int64_t frame_stride, int frames, void* stream);

/* ---- video mux, compressed: baseline JPEG per frame (REFace/scripts/VFace_inference_batch.py:646-654) -----------------------
 * The reference ends in a compressed, playable file (:646-654, mp4; :656-658, gif).  H.264 is not built; these two entry points
 * make the entropy-coded scan of a baseline 4:2:0 JPEG of every frame on the device, vface_amd/scripts/mjpeg.py adds the headers and
 * writes the frames as Motion-JPEG into an AVI, and the host receives the compressed bytes only.  csrc/mjpeg.hip.
 *
 * vface_jpeg_coefficients: rgb [frames][H][W][3] -> quantised DCT coefficients, frame f at out + f * frame_stride (int16
 *   elements): [mcu_rows][mcu_cols][6][64], mcu_rows = (H + 15) / 16, mcu_cols = (W + 15) / 16, the six blocks of a 16 x 16 MCU in
 *   the order Y00 Y01 Y10 Y11 Cb Cr, 64 coefficients each in zigzag order.  A frame is extended to whole MCUs by replicating its last
 *   column and row.  One fused pass: RGB -> JFIF Y'CbCr, **full-range BT.601** (what every MJPEG decoder assumes; NOT the BT.709
 *   limited range of vface_rgb_to_yuv420) -> 2 x 2 chroma mean -> level shift -> 8 x 8 forward DCT -> quantise -> zigzag.  qluma,
 *   qchroma: device tables of 64 bytes, row-major, 1..255.  Integer arithmetic, stated once in tests/jpeg_model.py and equal to
 *   it bit for bit; |DC| <= 1024, |AC| <= 1023.  Elements between frames are not written.
 *   NULL pointer, W, H or frames <= 0: VFACE_ERR_ARG; W or H > 65535, frame_stride < mcu_rows * mcu_cols * 384: VFACE_ERR_SHAPE.
 *
 * vface_jpeg_entropy: coefficient frames as above (`mcus` = mcu_rows * mcu_cols per frame, frame f at coef + f * frame_stride) ->
 *   the scan of every frame, baseline Huffman coding with the four typical tables of T.81 Annex K, restart intervals of `restart`
 *   MCUs (the DRI value; a frame's last interval may be shorter): every interval starts with zero DC predictors and ends
 *   1-padded to a whole byte, FF bytes inside it are followed by a stuffed 00, and RSTm, m = index mod 8, stands between the
 *   intervals of a frame.  No EOI.  The scans are packed back to back into out (frame 0 first); lengths [frames] takes each
 *   frame's byte count.  Bytes past out_bytes are dropped, never written: out_bytes >= frames * (intervals * restart * 6 * 416 +
 *   2 * (intervals - 1)) always suffices (416 = twice the 64 * (16 + 10) bits of a block, for the stuffing), and a caller that
 *   gives less compares the sum of lengths with it.  workspace: vface_jpeg_entropy_workspace_bytes(mcus, frames, restart) bytes,
 *   16-byte aligned.  Three launches, no allocation, no host synchronisation.
 *   NULL pointer, mcus, frames, restart or out_bytes <= 0: VFACE_ERR_ARG; restart > 65535, frame_stride < mcus * 384, a workspace
 *   too small: VFACE_ERR_SHAPE; a workspace off 16 bytes: VFACE_ERR_ALIGN. */
int vface_jpeg_coefficients(const uint8_t* rgb, int W, int H, int frames, const uint8_t* qluma, const uint8_t* qchroma, int16_t* out,
                            int64_t frame_stride, void* stream);
size_t vface_jpeg_entropy_workspace_bytes(int mcus, int frames, int restart);
int vface_jpeg_entropy(const int16_t* coef, int64_t frame_stride, int mcus, int frames, int restart, uint8_t* out, int64_t out_bytes,
                       int32_t* lengths, void* workspace, size_t workspace_bytes, void* stream);

/* ---- PNG frames out (REFace/scripts/VFace_inference_batch.py:636) -------------------------------------------------------------
 * The reference's main output is one PNG per pasted frame (:636).  These entry points make the deflate body of every frame's zlib
 * stream on the device; vface_amd/scripts/png.py adds 78 01, the Adler-32, the chunk framing and the CRC, and the host receives the
 * compressed bytes and O(stripes) scalars only.  csrc/png.hip; the code-length construction is csrc/png_huffman.hpp, which a host
 * program runs under sanitizers.  The format is stated once in tests/png_model.py and equalled byte for byte.
 *
 * vface_png_filter (:636): rgb [frames][H][W][3] -> rows [frames][H][1 + 3 W]: every row's filter byte and filtered bytes.  A row
 *   takes the type (0 None, 1 Sub, 2 Up, 3 Average, 4 Paeth; bpp 3; the row above a frame's row 0 is zeros) whose filtered bytes,
 *   read as signed, have the smallest sum of absolute values; a tie goes to the lowest type.  Predictions read the source pixels.
 *   NULL pointer, W, H or frames <= 0: VFACE_ERR_ARG; W > 2^22 or (1 + 3 W) * H >= 2^31: VFACE_ERR_SHAPE.
 *
 * vface_png_deflate (:636): rows [frames][H][row_bytes] of ANY bytes, row_bytes >= 1 -> one deflate body per frame, packed back
 *   to back into out; offsets [frames] and lengths [frames] take each body's place and byte count.  A frame is cut into stripes
 *   of stripe_rows rows (the last may be shorter), coded independently by one workgroup each: a dynamic-Huffman block, BFINAL 0, of
 *   literals and distance-1 matches of 3..258 (greedy: a run's first byte is a literal, the rest is cut into matches of 258, a
 *   remainder of 3 or more is one match, of 1 or 2 literals), ended by symbol 256 and followed by an empty stored block (3 bits,
 *   padding, 00 00 FF FF) that byte-aligns it -- or, where that is not SMALLER, stored blocks of at most 65535 bytes.  03 00, an
 *   empty final fixed block, ends a body.  Lit/len codes of at most 15 bits, HLIT 29, one distance code of length 1, code-length
 *   codes of at most 7 bits, zero runs as symbols 18 and 17 (csrc/png_huffman.hpp).  adler [frames][stripes][2], stripes =
 *   ceil(H / stripe_rows): (s1, s2) of Adler-32 over every stripe's bytes alone.  Bytes past out_bytes are dropped, never written:
 *   out_bytes >= frames * vface_png_deflate_bound(row_bytes, H, stripe_rows) always suffices and is reached by incompressible rows.
 *   workspace: vface_png_deflate_workspace_bytes(row_bytes, H, frames, stripe_rows) bytes, 16-byte aligned.  Three launches, no
 *   allocation, no host synchronisation.
 *   NULL pointer, row_bytes, H, frames, stripe_rows or out_bytes <= 0: VFACE_ERR_ARG; row_bytes * H or the bound >= 2^31, a workspace
 *   too small: VFACE_ERR_SHAPE; a workspace off 16 bytes: VFACE_ERR_ALIGN. */
int vface_png_filter(const uint8_t* rgb, int W, int H, int frames, uint8_t* rows, void* stream);
int64_t vface_png_deflate_bound(int row_bytes, int rows, int stripe_rows);
size_t vface_png_deflate_workspace_bytes(int row_bytes, int H, int frames, int stripe_rows);
int vface_png_deflate(const uint8_t* rows, int row_bytes, int H, int frames, int stripe_rows, uint8_t* out, int64_t out_bytes,
                      int64_t* offsets, int32_t* lengths, uint32_t* adler, void* workspace, size_t workspace_bytes, void* stream);

/* ---- GIF out (REFace/scripts/VFace_inference_batch.py:658) ---------------------------------------------------------------------
 * The reference ends a run with clips.write_gif(...) of the pasted frames (:658).  These entry points make, per frame, a palette of
 * up to 256 colours and the complete image data of a GIF frame on the device; vface_amd/scripts/gif.py adds the fixed headers and the
 * 768 palette bytes.  csrc/gif.hip; the cut rule is csrc/gif_palette.hpp and the encoder csrc/gif_lzw.hpp, which a host program runs
 * under sanitizers.  The format is stated once in tests/gif_model.py and equalled bit for bit.  Every call that takes W and H:
 * W, H in 1..65535 and W * H <= 2^24 (a box's channel sum, at most 255 * 2^24, fits 32 bits), otherwise VFACE_ERR_SHAPE; a NULL
 * pointer or W, H, frames <= 0: VFACE_ERR_ARG.  No allocation, no host synchronisation.
 *
 * vface_gif_histogram (:658): rgb [frames][H][W][3] -> counts [frames][32768]: the pixels per cell,
 *   cell(r, g, b) = (r >> 3) << 10 | (g >> 3) << 5 | (b >> 3).  counts is zeroed by the call.
 *
 * vface_gif_boxes (:658): counts [frames][32768] -> labels [frames][32768], a box number per cell (0 for an empty cell), and
 *   ncolors [frames], the number of boxes = min(256, non-empty cells).  Median cut: box 0 holds every non-empty cell; up to 255 times
 *   the box with at least two non-empty cells and the largest population x longest side in cells (lowest number on a tie) is cut
 *   along its longest axis (ties R, G, B) at the population median, both sides non-empty; the upper side takes the next number.
 *
 * vface_gif_palette (:658): rgb and labels -> palette [frames][256][3]: entry i is the mean of the pixels whose cell lies in box i,
 *   each channel (2 sum + n) / (2 n) rounded down; an entry without pixels is zeros.  sums: frames * 4096 bytes of workspace,
 *   4-byte aligned (VFACE_ERR_ALIGN), zeroed by the call.
 *
 * vface_gif_map (:658): rgb, palette and ncolors -> indices [frames][W * H]: every pixel's entry of smallest squared RGB distance
 *   among the first ncolors[frame] (clamped to 1..256), the lowest index on a tie.  Exact search, 256 distances per pixel.
 *
 * vface_gif_lzw (:658): indices [frames][npix] -> every frame's image data packed back to back into out, frame f at offsets[f],
 *   offsets[frames] the end (offsets: int64 [frames + 1]).  Image data: 08, the bit stream padded to a byte in sub-blocks of at most
 *   255 bytes behind their length byte, 00.  Minimum code size 8 (Clear 256, end of information 257, first free code 258, 9 to 12
 *   bits, LSB first).  The stream is Clear, then per segment of seg_pixels indices (the last may be shorter) its greedy LZW codes
 *   from an empty table and its terminator: Clear if another segment follows, end of information after the last; a table that fills
 *   inside a segment is answered by a Clear at 12 bits.  One wave codes a segment; a code's bit offset follows from its number
 *   alone, so all codes are then placed in parallel.  Bytes at or past out_bytes are dropped, never written, and offsets stay
 *   the true ones: out_bytes >= frames * vface_gif_lzw_bound(npix, seg_pixels) always suffices.  workspace:
 *   vface_gif_lzw_workspace_bytes(npix, frames, seg_pixels) bytes, 16-byte aligned.  One memset and four launches.
 *   NULL pointer, npix, frames, seg_pixels or out_bytes <= 0: VFACE_ERR_ARG; npix > 2^24, seg_pixels > 65535, a workspace too
 *   small: VFACE_ERR_SHAPE; a workspace off 16 bytes: VFACE_ERR_ALIGN.  The two size queries return 0 for such arguments. */
int vface_gif_histogram(const uint8_t* rgb, int W, int H, int frames, uint32_t* counts, void* stream);
int vface_gif_boxes(const uint32_t* counts, int frames, uint8_t* labels, int32_t* ncolors, void* stream);
int vface_gif_palette(const uint8_t* rgb, int W, int H, int frames, const uint8_t* labels, uint8_t* palette, uint32_t* sums, void* stream);
int vface_gif_map(const uint8_t* rgb, int W, int H, int frames, const uint8_t* palette, const int32_t* ncolors, uint8_t* indices,
                  void* stream);
int64_t vface_gif_lzw_bound(int64_t npix, int seg_pixels);
size_t vface_gif_lzw_workspace_bytes(int64_t npix, int frames, int seg_pixels);
int vface_gif_lzw(const uint8_t* indices, int64_t npix, int frames, int seg_pixels, uint8_t* out, int64_t out_bytes, int64_t* offsets,
                  void* workspace, size_t workspace_bytes, void* stream);

/* ---- PNG frames in (REFace/scripts/VFace_inference_batch.py:285) --------------------------------------------------------------
 * The reference writes the target clip as {index}.png (:285) and reads the folder back.  vface_amd/scripts/png_in.py walks each
 * file's chunks on the host (CRCs, IHDR, the zlib header) and uploads the deflate bodies as they lie in the files; these entry
 * points make 8-bit RGB frames of them on the device.  csrc/png_in.hip; what file bytes steer is csrc/png_inflate.hpp, which a
 * host program runs under sanitizers.  The format is stated once in tests/png_inflate_model.py and equalled bit for bit.
 *
 * vface_png_inflate: raw deflate bodies (RFC 1951; no zlib header, no Adler-32), file f at streams + offsets[f], lengths[f] bytes
 *   -> the filtered rows, file f at rows + f * file_stride, exactly `expect` bytes where status[f] is 0.  Stored, fixed and dynamic
 *   blocks, code lengths up to 15 bits, repeats running across the literal/distance boundary, distances up to 32768.  One wave per
 *   file.  No byte outside [offsets[f], offsets[f] + lengths[f]) is read; a range that does not lie inside [0, stream_bytes) gets
 *   status 1.  No byte outside the file's `expect` bytes is written whatever the stream holds, and none past produced[f].
 *   status[f] is the first condition met in stream order (within a dynamic header in this order): 0 the final block ended with
 *   exactly `expect` bytes; 1 a bit was needed past the stream's end; 2 block type 3; 3 stored block, LEN != ~NLEN; 4 more than 286
 *   literal/length or 30 distance codes; 5 the code-length code is over-subscribed or incomplete; 6 repeat 16 with no previous length,
 *   or a repeat past HLIT + HDIST; 7 no code for symbol 256; 8 the literal/length set is over-subscribed, or incomplete and not a
 *   single 1-bit code; 9 the same for the distance set (no code at all is legal); 10 bits that are no literal/length code, or symbol
 *   286 / 287; 11 bits that are no distance code, or symbol 30 / 31; 12 a distance greater than the bytes produced so far; 13 more
 *   than `expect` bytes (the token that would pass it is not written); 14 the final block ended with fewer.  zlib 1.2.11 accepts a
 *   stream exactly where this does.  produced[f]: bytes written; consumed[f]: whole bytes of the body behind the last bit taken
 *   (lengths[f] for status 1 -- but 0, like produced[f], for a file whose range lies outside the stream buffer: nothing of it was
 *   read; bytes behind the final block are accepted and not counted); adler [files][2]: (s1, s2) of Adler-32
 *   over the produced bytes.  One launch, no allocation, no host synchronisation.
 *   NULL pointer, files, stream_bytes or expect <= 0: VFACE_ERR_ARG; expect or stream_bytes >= 2^31, file_stride < expect:
 *   VFACE_ERR_SHAPE.
 *
 * vface_png_unfilter: rows [files][H][1 + bpp W] at file_stride -> rgb [files][H][W][3]: the five filter types (0 None, 1 Sub,
 *   2 Up, 3 Average, 4 Paeth with ties a, b, c) undone with bytes mod 256, the row above row 0 zeros, bpp bytes to the left; bpp 4
 *   drops alpha, bpp 1 replicates grey.  status[f]: 0, or 1 + the first row whose filter byte is above 4.  A file whose
 *   inflate_status is not 0 is not read; its frame, and the frame of a file with a bad filter byte, is cleared to 0.  One wave per
 *   file walks bands of 64 rows in a skewed wavefront, every lane loading and storing its own row.
 *   NULL pointer, W, H or files <= 0: VFACE_ERR_ARG; bpp outside {1, 3, 4}, (1 + bpp W) * H >= 2^31, file_stride below that, or
 *   W > 8192 (the row carried between bands lives in LDS): VFACE_ERR_SHAPE. */
int vface_png_inflate(const uint8_t* streams, int64_t stream_bytes, const int64_t* offsets, const int32_t* lengths, int files,
                      uint8_t* rows, int64_t file_stride, int64_t expect, int32_t* status, int32_t* produced, int32_t* consumed,
                      uint32_t* adler, void* stream);
int vface_png_unfilter(const uint8_t* rows, int64_t file_stride, int W, int H, int bpp, int files, const int32_t* inflate_status,
                       uint8_t* rgb, int32_t* status, void* stream);

/* vface_png_inflate_parallel: vface_png_inflate on many waves per file, block by block (csrc/png_in_par.hip; the pieces and a host
 *   routine that sanitizers run are csrc/png_inflate_par.hpp, the protocol is stated in tests/png_inflate_par_model.py).  The
 *   arguments up to adler are vface_png_inflate's, and rows[0 .. produced), status, produced, consumed and adler are what it writes
 *   for EVERY input, valid or corrupt, bit for bit; nothing is written behind produced[f], nothing is read outside a file's range.
 *   A file's body is cut into chunks of chunk_bytes (64 .. 2^20, a multiple of 4).  Chunk 0's segment starts at bit 0; chunk c >= 1's
 *   at the smallest bit of its own range at which a dynamic block's header reads with status 0; a chunk without one starts none.
 *   One wave per segment counts its bytes (up to the first block that ends at or behind the next segment's start, or a final one);
 *   a file whose segments report no status, end exactly on one another with BFINAL in the last alone, and sum to `expect` is decoded
 *   segment by segment into 16-bit elements (a byte, or 0x8000 | k: the byte k positions into the 32 768 in front of the segment)
 *   and resolved in order into rows.  An accepted chain is the serial decode's own block sequence, by induction from bit 0.  Every
 *   other file is decoded by vface_png_inflate's kernel in the call's last launch.
 *   info: NULL or [files][4]: info[f][0] segments decoded in parallel and accepted, or 0 where the serial kernel decoded the file;
 *   info[f][1] why it did: 0 it did not, 1 the chain did not close, 2 a segment reported a status (1 .. 11), 3 the byte count is not
 *   `expect` (statuses 13, 14 among them), 4 a distance reaches in front of the file (status 12), 5 the file's range lies outside the
 *   buffer; where several hold, 5, 2, 1, 3, 4 in that order; info[f][2] candidates found; info[f][3] 0.
 *   workspace: vface_png_inflate_parallel_workspace_bytes(files, stream_bytes, expect, chunk_bytes) bytes (0 for arguments the call
 *   refuses), 16-byte aligned: the segment tables of files * ceil(stream_bytes / chunk_bytes) entries and 2 * files * expect bytes
 *   of elements.  Six launches, no allocation, no host synchronisation.
 *   Refusals are vface_png_inflate's, and: NULL workspace: VFACE_ERR_ARG; chunk_bytes outside 64 .. 2^20 or no multiple of 4, a
 *   workspace too small: VFACE_ERR_SHAPE; a workspace off 16 bytes: VFACE_ERR_ALIGN. */
size_t vface_png_inflate_parallel_workspace_bytes(int files, int64_t stream_bytes, int64_t expect, int chunk_bytes);
int vface_png_inflate_parallel(const uint8_t* streams, int64_t stream_bytes, const int64_t* offsets, const int32_t* lengths, int files,
                               uint8_t* rows, int64_t file_stride, int64_t expect, int32_t* status, int32_t* produced, int32_t* consumed,
                               uint32_t* adler, int chunk_bytes, void* workspace, size_t workspace_bytes, int32_t* info, void* stream);

/* ---- video in, colour half (REFace/scripts/VFace_inference_batch.py:240-285) --------------------------------------------------
 * The reference decodes the target video on the host (cv2.VideoCapture, BGR -> RGB, PNG per frame, :240-285).  The H.264 decoder
 * is not built here either; vface_amd/scripts/demux.py reads the YUV4MPEG2 file any decoder writes (`ffmpeg -i in.mp4 clip.y4m`),
 * the host uploads the I420 planes -- 1.5 bytes per pixel instead of 3 -- and vface_yuv420_to_rgb makes the 8-bit RGB frames on
 * the device: the inverse direction of vface_rgb_to_yuv420, same frame layout.
 *   i420: frame f at i420 + f * frame_stride: Y [H][W], Cb [ch][cw], Cr [ch][cw], cw = (W + 1) / 2, ch = (H + 1) / 2; bytes
 *   between frames are not read -> rgb [frames][H][W][3], dense.
 *   matrix: 0 = BT.709, 1 = BT.601 (Y4M cannot tag it); full_range: 0 = limited (`tv`: Y offset 16, scales 255/219 and 255/224),
 *   1 = full; chroma: 0 = nearest, 1 = centre-sited (C420jpeg; what vface_rgb_to_yuv420 writes), 2 = left (C420mpeg2: horizontally
 *   co-sited, vertically centred) -- the chroma of a pixel is the weighted sum of its four neighbouring samples in sixteenths,
 *   neighbour indices clamped into the plane.
 *   Integer arithmetic, stated once in tests/demux_model.py and equal to it bit for bit: 16-bit coefficients, one half-up rounding,
 *   then the clamp to 0..255.  W and H may be odd; no alignment is required of either pointer or of frame_stride.
 *   NULL pointer, W, H or frames <= 0, matrix / full_range / chroma outside their values: VFACE_ERR_ARG; frame_stride <
 *   W * H + 2 * cw * ch, or more than 2^31 - 1 strips of 2 rows x 16 pixels in all: VFACE_ERR_SHAPE -- before the first HIP call. */
int vface_yuv420_to_rgb(const uint8_t* i420, int64_t frame_stride, int W, int H, int frames, uint8_t* rgb, int matrix,
                        int full_range, int chroma, void* stream);

/* ---- video in, compressed: baseline JPEG per frame (REFace/scripts/VFace_inference_batch.py:240-285) --------------------------
 * The reference hands the target video to cv2.VideoCapture (:240-285).  Of the codecs that decodes, baseline JPEG is built here:
 * vface_amd/scripts/mjpeg_in.py walks an AVI with an MJPG stream and parses each frame's headers on the host (8-bit, three
 * components, Y 2 x 2, Cb and Cr 1 x 1, one scan), the SCANS cross to the device -- about a tenth of the I420 bytes at quality 90 --
 * and these entry points turn them into the I420 rows vface_yuv420_to_rgb reads (matrix 1, full_range 1, chroma 1: JFIF).
 * csrc/mjpeg_in.hip; the interval decoder is csrc/jpeg_interval.hpp, which a host program runs under sanitizers.
 *
 * Common to the three: `mcus` = mcu_rows * mcu_cols per frame, the same for every frame of a call; restart [frames] = the DRI
 *   value of each frame, 0 = none; a frame has ceil(mcus / restart) intervals (1 without restart, or where restart >= mcus);
 *   max_intervals >= the largest of those counts is the row length of `ranges`.  status [frames]: 0 = decoded, 1 = the scan does
 *   not hold the RST markers its header promises, 2 = they do not run RST0, RST1, .. mod 8, 3 = the bytes of an interval ran
 *   out before its blocks, 4 = bits that are no code of the table, 5 = DC category above 11, 6 = AC size above 10, 7 = a zero run
 *   past coefficient 63, 8 = a DC value outside int16.
 *
 * vface_jpeg_scan_index: scans = the frames' entropy-coded segments in one buffer of scan_bytes bytes, frame f at offsets[f],
 *   lengths[f] bytes (after SOS, up to EOI) -> ranges [frames][max_intervals][2] int32: (begin, end) of every restart interval in
 *   bytes of `scans`, the RST marker between two intervals in neither; entries past a frame's count are 0.  Writes status[f] =
 *   0, 1 or 2 for every frame; a refused frame's row of ranges is 0.  A frame whose bytes do not lie inside the buffer is refused (1).
 *   NULL pointer, mcus, frames, max_intervals or scan_bytes <= 0: VFACE_ERR_ARG; scan_bytes >= 2^31, max_intervals > mcus: VFACE_ERR_SHAPE.
 *
 * vface_jpeg_decode_entropy: ranges and status as vface_jpeg_scan_index left them -> out: quantised coefficients, frame f at
 *   out + f * frame_stride (int16 elements): [mcus][6][64], blocks Y00 Y01 Y10 Y11 Cb Cr, zigzag order -- the layout
 *   vface_jpeg_coefficients writes, so that vface_jpeg_entropy followed by these two calls is the identity.  tables: 2304 bytes per
 *   frame, 4-byte aligned: DC tables of Y, Cb, Cr, then their AC tables, each int32 maxcode[16], int32 valoff[16], uint8 vals[256]
 *   (csrc/jpeg_interval.hpp; mjpeg_in.huffman_block builds them).  Canonical Huffman decoding, stuffed 00 bytes skipped, DC
 *   prediction per component reset at every interval, ZRL, EOB, EXTEND of T.81 F.2.2.1.  Every frame's mcus * 384 elements are
 *   cleared first: what a refused frame or a failed interval did not reach is 0.  Elements between frames are not written.  A
 *   frame's status becomes the largest code of its intervals (3..8); frames with status 1 or 2 are not decoded.  No byte outside
 *   [begin, end) of an interval is read and no element outside its MCUs is written, whatever the bytes are.
 *   NULL pointer, mcus, frames, max_intervals or scan_bytes <= 0: VFACE_ERR_ARG; scan_bytes >= 2^31, max_intervals > mcus,
 *   frame_stride < mcus * 384: VFACE_ERR_SHAPE; tables off 4 bytes: VFACE_ERR_ALIGN.
 *
 * vface_jpeg_decode_entropy_parallel: vface_jpeg_decode_entropy's arguments, its output and its statuses -- the same for every input,
 *   valid or corrupt -- from many lanes per restart interval, for scans without restart markers (one interval per frame, which the
 *   call above gives ONE lane).  An interval is cut into subsequences of subseq_bytes raw scan bytes; one workgroup per (frame,
 *   interval) walks them in chunks of 64 or 256 (chosen on the host from scan_bytes / (frames * max_intervals) / subseq_bytes),
 *   decodes every subsequence of a chunk from a guessed state (its first bit, first block of an MCU, DC symbol next) and repeats, each
 *   lane taking its left neighbour's exit state, until a round changes nothing: at most one round per lane, whatever the bytes are.
 *   A prefix sum of the blocks begun places every lane's coefficients; DC values are a prefix sum of the differences per component.
 *   A frame in which the serial routine would report anything (3..8) is cleared and decoded again by that routine in the last launch
 *   of the call, on a device flag: status and partial output of a bad frame are vface_jpeg_decode_entropy's by construction.  The
 *   per-subsequence routine is csrc/jpeg_subseq.hpp, which a host program runs under sanitizers; the same promise holds for reads
 *   and writes.  workspace: vface_jpeg_decode_entropy_parallel_workspace_bytes(frames) bytes, 4-byte aligned.  rounds: NULL, or
 *   [frames][max_intervals] int32 = the rounds that changed a state, summed over an interval's chunks; 0 for a frame or interval
 *   that was not decoded.
 *   The refusals of vface_jpeg_decode_entropy, and: NULL workspace: VFACE_ERR_ARG; subseq_bytes outside 4..1024 or no multiple of 4,
 *   workspace_bytes too small: VFACE_ERR_SHAPE; workspace off 4 bytes: VFACE_ERR_ALIGN.
 *
 * vface_jpeg_planes: coefficient frames as above (frame f at coef + f * coef_stride) and quant [frames][3][64], the quantisation
 *   table of Y, Cb, Cr of every frame, row-major -> out: one I420 frame per frame, frame f at out + f * row_stride: Y [H][W], Cb
 *   [ch][cw], Cr [ch][cw], cw = (W + 1) / 2, ch = (H + 1) / 2, cropped out of the whole MCUs.  Dequantisation, an integer 8 x 8
 *   inverse DCT in two passes, + 128, clamp to 0..255; stated once in tests/jpeg_decode_model.py and equal to it bit for bit.  Within
 *   0.5 + 0.15 of a level of the fp64 definition for coefficients an encoder can produce; every sum fits int32 for every int16
 *   coefficient.  Bytes between frames are not written.
 *   NULL pointer, W, H or frames <= 0: VFACE_ERR_ARG; W or H > 65535, coef_stride < mcus * 384, row_stride < W * H + 2 * cw * ch:
 *   VFACE_ERR_SHAPE. */
int vface_jpeg_scan_index(const uint8_t* scans, int64_t scan_bytes, const int64_t* offsets, const int32_t* lengths,
                          const int32_t* restart, int mcus, int frames, int max_intervals, int32_t* ranges, int32_t* status,
                          void* stream);
int vface_jpeg_decode_entropy(const uint8_t* scans, int64_t scan_bytes, const int32_t* ranges, const int32_t* restart,
                              const uint8_t* tables, int mcus, int frames, int max_intervals, int16_t* out, int64_t frame_stride,
                              int32_t* status, void* stream);
size_t vface_jpeg_decode_entropy_parallel_workspace_bytes(int frames);
int vface_jpeg_decode_entropy_parallel(const uint8_t* scans, int64_t scan_bytes, const int32_t* ranges, const int32_t* restart,
                                       const uint8_t* tables, int mcus, int frames, int max_intervals, int16_t* out,
                                       int64_t frame_stride, int32_t* status, int subseq_bytes, void* workspace,
                                       size_t workspace_bytes, int32_t* rounds, void* stream);
int vface_jpeg_planes(const int16_t* coef, int64_t coef_stride, const uint8_t* quant, int W, int H, int frames, uint8_t* out,
                      int64_t row_stride, void* stream);

/* ---- frame intake: decoded frame -> aligned crop -> the sampler's tensors (the mirror image of the paste-back) ---------------
 * The reference runs these steps per frame on the host with Pillow and numpy.  The Lanczos shrink of a large face
 * (alignmengt.py:108-114) and the bicubic resize to 512 x 512 (video_swap_dataset.py:139) are vface_resample_u8 with the tap
 * tables of those filters (vface_amd/scripts/intake.py `resample_coeffs`).
 *
 * vface_quad_crop: the "Crop" and "Transform" steps of `crop_image` (REFace/src/utils/alignmengt.py:115-123, :142, reached from
 *   crop_faces_by_quads :255-263): `img.crop(window)` then `img.transform((out_size, out_size), Image.QUAD, quad + 0.5,
 *   Image.BILINEAR)` (Pillow Geometry.c quad_transform / bilinear_filter32RGB), without materialising the cropped image.
 *   frames [nframes][H][W][3]; out [nframes][out_size][out_size][3]; quads [nframes][8] doubles = the coefficients Pillow's
 *   Image.__transformer derives from the quad (a0 + a1 x + a2 y + a3 x y ; a4 ..), in WINDOW coordinates; windows [nframes][4]
 *   int32 = (x0, y0, x1, y1) of the crop window inside the frame, 0 <= x0 < x1 <= W and 0 <= y0 < y1 <= H.  Taps are clamped
 *   to the window, pixels that map outside it are 0 in all three bytes.  Bit-identical to Pillow. */
int vface_quad_crop(const uint8_t* frames, int W, int H, uint8_t* out, int out_size, int nframes, const double* quads,
                    const int32_t* windows, void* stream);

/* vface_dataset_tensors: `VideoDataset.__getitem_gray__` (REFace/ldm/data/video_swap_dataset.py:157-163, :214-221) and the mask
 *   resize of REFace/scripts/VFace_inference_batch.py:459.  crop [nframes][H][W][3] uint8, label [nframes][H][W] uint8 (any value
 *   0..255), member[256] uint8: non-zero where the label is on the `remove_mask_tar_FFHQ` list.
 *     image         [nframes][3][H][W]   fp32 = (u8 / 255 - 0.5) / 0.5            get_tensor() (:214)
 *     inpaint_mask  [nframes][1][H][W]   fp32 = 1 - isin(label, remove)             (:219)
 *     inpaint_image [nframes][3][H][W]   fp32 = image * inpaint_mask                (:221)
 *     mask_latent   [nframes][1][OH][OW] fp32 = transforms.Resize([OH, OW])(inpaint_mask): bilinear, align_corners false, no
 *                   antialias (:459), fp32 in vface_frame_normalise_resize's order; computed from the label map itself. */
int vface_dataset_tensors(const uint8_t* crop, const uint8_t* label, const uint8_t* member, int W, int H, float* image,
                          float* inpaint_image, float* inpaint_mask, float* mask_latent, int OW, int OH, int nframes, void* stream);

/* vface_source_tensors: what REFace/scripts/VFace_inference_batch.py makes of the SOURCE image once per clip (:324-355, :462, :468),
 *   one launch for nimg sources; no atomics, no allocation, capturable; an image's bits do not depend on nimg.
 *   crop  [nimg][S][S][3] uint8: the aligned crop (:254-258); img [nimg][H][W][3] uint8: the crop after `resize((W, H),
 *   Image.BILINEAR)` (:350, Pillow bilinear = vface_resample_u8); label [nimg][H][W] uint8 (any value 0..255); member[256] uint8:
 *   non-zero where the label is on the `preserve_mask_src_FFHQ` list (project_ffhq.yaml:217-224).
 *     mask        [nimg][1][H][W]    fp32 = isin(label, preserve) = ToTensor(255 m)                               (:324-341)
 *     masked      [nimg][3][H][W]    fp32 = (u8 / 255 - 0.5) / 0.5 * mask          ref_img_inv_ori                 (:350-352)
 *     inpaint     [nimg][3][H][W]    fp32 = masked * (1 - mask): x m (1 - m), zero for a {0, 1} mask; reproduced as it is (:354-355)
 *     mask_latent [nimg][1][OH][OW]  fp32 = Resize([OH, OW])(1 - mask): bilinear, align_corners false, no antialias, fp32 in
 *                 vface_frame_normalise_resize's order, from the label map itself (as vface_dataset_tensors)      (:462, :468)
 *     clip_image  [nimg][3][OC][OC]  fp32 = (q / 255 - mean_c) / std_c * Resize((OC, OC))(mask): get_tensor_clip() (:96-104) of
 *                 q = A.Resize(OC, OC)(crop), times the tensor-resized mask in the same fp32 order; each fp32 operation rounded
 *                 once (div, sub, div, mul)                                                                        (:342-347)
 *     clip_u8     [nimg][OC][OC][3]  uint8 = q itself; optional (NULL = not written)
 *   q is the 8-bit 2-tap resize of albumentations' default, cv2.INTER_LINEAR, in OpenCV's 11-bit fixed-point form: per output
 *   index d on an axis n_in -> n_out, f = (d + 0.5) n_in / n_out - 0.5 in double, s = floor(f), t = f - s (s < 0: s = 0, t = 0;
 *   s >= n_in - 1: s = n_in - 1, t = 0), second tap min(s + 1, n_in - 1), w1 = rint(2048 t), w0 = rint(2048 (1 - t)); rows
 *   R = p[s] w0 + p[s'] w1 in int32, q = (((v0 (R0 >> 4)) >> 16) + ((v1 (R1 >> 4)) >> 16) + 2) >> 2.  The host builds the tables
 *   (vface_amd/scripts/resample.py `linear_taps_u8`): xtap / ytap int32 [OC][2] = (s, s'), xw / yw int16 [OC][2] = (w0, w1).
 *   Parity with cv2.resize is NOT pinned: OpenCV is not available to this project's tests.
 *   Any required pointer NULL or any size <= 0: VFACE_ERR_ARG before the first HIP call. */
int vface_source_tensors(const uint8_t* crop, int S, const uint8_t* img, const uint8_t* label, const uint8_t* member, int W, int H,
                         const int32_t* xtap, const int16_t* xw, const int32_t* ytap, const int16_t* yw, float* mask, float* masked,
                         float* inpaint, float* mask_latent, int OW, int OH, float* clip_image, uint8_t* clip_u8, int OC, int nimg,
                         void* stream);

/* ---- face parsing: aligned crop -> label map (BiSeNet over ResNet-18) ---------------------------------------------------------
 * The reference runs `faceParsing_demo` -> `FaceParser.forward` -> `BiSeNet` (REFace/pretrained/face_parsing/{face_parsing_demo,
 * model,resnet}.py; scripts/VFace_inference_batch.py:251, 292-294) one frame at a time in fp32.  Its convolutions are vface_conv3x3 /
 * vface_im2col + vface_gemm with eval-mode BatchNorm folded in on the host, its ReLUs vface_channel_norm_act and its global average
 * pools the means of vface_channel_stats (vface_amd/parsing.py); these entry points are the rest.  All: raw device pointers, no
 * allocation, no synchronisation, capturable; a refusal launches nothing; no atomics (bits do not depend on the batch).
 *
 * vface_parse_prefilter: `FaceParser.preprocess_img` with `BicubicDownSample(factor=2)` (face_parsing_demo.py:124-193, 260-264).
 *   crops [nframes][H2][W2][3] uint8 -> out [nframes * H2/2 * W2/2][ldo] 16-bit, 8 channels written per pixel (3 values, 5 zeros):
 *   u8 / 255; the 8-tap separable filter k[i] = bicubic((i - 4 + 0.5) / 2), a = -0.5, normalised to sum 1 -- vertical pass, then
 *   horizontal, `reflect` padding 3 + 3, stride 2; clamp(0, 1); (x - seg_mean) / seg_std (model.py:15-16).  fp32 throughout, one
 *   rounding.  factor must be 2 and H2, W2 even and >= 8 (VFACE_ERR_SHAPE otherwise). */
int vface_parse_prefilter(const uint8_t* crops, int W2, int H2, int factor, void* out, int64_t ldo, int nframes, int dtype,
                          void* stream);

/* vface_maxpool3x3s2: nn.MaxPool2d(3, stride 2, padding 1) (resnet.py:64) on NHWC 16-bit rows; padding is -inf.
 *   x [nimg * H * W][ldx] -> y [nimg * OH * OW][ldy], OH = (H - 1) / 2 + 1, OW likewise; C % 8 == 0. */
int vface_maxpool3x3s2(const void* x, int64_t ldx, int nimg, int H, int W, int C, void* y, int64_t ldy, int dtype, void* stream);

/* vface_channel_gate: y[m][c] = x[m][c] * g[m / hw][c] + r (one fp32 fma, one rounding to 16 bits); g fp32 [nimg][ldg].  r is at
 *   most one of: rvec fp32 [nimg][ldrv] (model.py:122: `feat32_arm + avg_up`, the nearest upsample of a 1 x 1 map), rten 16-bit
 *   [M][ldr] (:127), add_x != 0 for x itself (:214-215); none: the plain gate (:88).  y may be x.  M % hw == 0, C % 8 == 0. */
int vface_channel_gate(const void* x, int64_t ldx, const float* g, int64_t ldg, const float* rvec, int64_t ldrv, const void* rten,
                       int64_t ldr, int add_x, void* y, int64_t ldy, int64_t M, int hw, int C, int dtype, void* stream);

/* vface_pooled_linear: the 1 x 1 convolutions on globally pooled vectors (model.py:85-87, :118, :210-213), fp32:
 *   out[n][o] = act(sum_k W[o][k] * a[n * lda + k * sa] + bias[o]), W fp32 [N][K] (BatchNorm folded in), bias may be NULL,
 *   act 0 none | 1 ReLU | 3 sigmoid (vface_channel_norm_act's codes).  sa = 2 reads the means where vface_channel_stats left them. */
int vface_pooled_linear(const float* a, int64_t lda, int sa, const float* W, const float* bias, float* out, int64_t ldo, int nimg,
                        int N, int K, int act, void* stream);

/* vface_upsample_argmax_u8: `F.interpolate(.., (H, W), 'bilinear', align_corners=True)` (model.py:258) + `torch.argmax(dim=1)`
 *   (face_parsing_demo.py:278) + a byte table (the 12-class map of :74-122, or the identity) in one pass: the full-resolution logit
 *   planes never exist.  logits fp32 [nframes * h * w][ld], columns 0 .. ncls - 1 compared (ncls <= 32 <= table entries; columns
 *   ncls .. ld - 1 may hold anything); out [nframes][H][W] uint8 = table[first maximal class].  ld % 4 == 0. */
int vface_upsample_argmax_u8(const float* logits, int64_t ld, int nframes, int h, int w, int ncls, const uint8_t* table,
                             uint8_t* out, int H, int W, void* stream);

/* ---- conditioning: the CLIP ViT image embedder, its mapper and the feature mix -----------------------------------------------
 * The reference runs `FrozenCLIPEmbedder` (REFace/ldm/modules/encoders/modules.py:211-264: HF CLIPVisionModel ViT-L/14, pooled output,
 * visual_projection, `mapper2` of encoders/xf.py, `final_ln2`) on every batch of target frames (scripts/VFace_inference_batch.py:442,
 * :500 -> ddpm.py:872-1045 `conditioning_with_feat`) in stock PyTorch.  Its projections are vface_gemm (q | k | v as one [3 C][C]
 * weight, the residual adds through vface_stream32), its attention vface_attention at dh = 64 on the three strided thirds of that
 * buffer, its LayerNorms vface_layernorm (in_f32); these entry points are the rest.  All: raw device pointers, no allocation, no
 * synchronisation, capturable; a refusal launches nothing; no atomics (a sample's bits do not depend on the batch).
 *
 * vface_clip_patches: the image as the patch matrix of CLIPVisionEmbeddings.patch_embedding (Conv2d 14 x 14, stride 14, no bias):
 *   out [B * grid * grid][ldo >= 640] 16-bit, row (b, py, px), column c * 196 + ky * 14 + kx -- the flattening of the weight
 *   [hidden][3][14][14] -- columns 588 .. 639 zero (K padded to a multiple of 64), so the embedding is one vface_gemm with K = 640.
 *   img fp32 planar [B][3][H][W].  prep == 0: img is already CLIP-normalised at 14 grid x 14 grid and is copied (one rounding).
 *   prep == 1: img is in [-1, 1] at any size -- ddpm.py:907-912 `un_norm`, `TF.normalize(CLIP mean, std)`, `TF.resize((224, 224))`
 *   (bilinear, align_corners false, NO antialias: what torchvision 0.14.1 does to a tensor; fp32 in vface_frame_normalise_resize's
 *   order); mask (optional, fp32 [B][H][W] = inpaint_mask): every pixel is first multiplied by (1 - mask)
 *   (scripts/VFace_inference_batch.py:493-496, where the normalisation follows the resize: equal up to fp32 rounding, the bilinear
 *   weights sum to 1).  dbg_x0 / dbg_y0 (optional, prep only, int32 [14 grid] each): the first source column / row of every output
 *   column / row.  grid <= 64. */
int vface_clip_patches(const float* img, int H, int W, const float* mask, int prep, void* out, int64_t ldo, int B, int grid,
                       int32_t* dbg_x0, int32_t* dbg_y0, int dtype, void* stream);

/* vface_clip_embed: CLIPVisionEmbeddings.forward behind the convolution (`cat([class_embedding, patch_embeds]) + position_embedding`)
 *   and, with gamma / beta, CLIPVisionTransformer's `pre_layrnorm` (the reference's spelling) on the sum:
 *   x32 [B * (patches + 1)][ldo] fp32: row b (patches + 1) from cls + pos[0], row b (patches + 1) + 1 + p from tok[b patches + p] +
 *   pos[1 + p]; gamma == beta == NULL: the sums themselves; otherwise their LayerNorm (fp32 two-pass statistics, eps), so the fp32
 *   residual stream starts unrounded.  tok [B * patches][ldt]: the patch GEMM's output, 16-bit, or fp32 when tok_f32 (the out32
 *   carrier of vface_stream32); cls, gamma, beta fp32 [C], pos fp32 [patches + 1][C].  C % 8 == 0. */
int vface_clip_embed(const void* tok, int64_t ldt, int tok_f32, const float* cls, const float* pos, const float* gamma, const float* beta,
                     float eps, float* x32, int64_t ldo, int B, int patches, int C, int dtype, void* stream);

/* vface_act: an activation on a 16-bit matrix view x [rows][ldx] -> y [rows][ldy] (y may be x), fp32 inside, one rounding.
 *   kind 0: quick_gelu v * sigmoid(1.702 v) (HF activations.py QuickGELUActivation, the ViT's MLP); kind 1: the erf GELU
 *   (encoders/xf.py MLP `nn.GELU()` of the mapper).  cols % 8 == 0. */
int vface_act(const void* x, int64_t ldx, void* y, int64_t ldy, int64_t rows, int cols, int kind, int dtype, void* stream);

/* vface_cond_mix: ddpm.py:1038-1039 `(c * clip_weight + c2 * ID_weight + landmarks * Landmarks_weight) / (sum of the weights)`:
 *   out[b][n] = (a w_a + b w_b + c w_c) / w_sum in fp32, summed left to right; operands fp32, contiguous [rows_x][N] with rows_x = B,
 *   or 1 for one row shared by every sample (the source's features); a NULL operand is left out (:1018-1019 without landmarks).
 *   w_sum is passed in (the reference forms it in double and rounds once).  out32 fp32 [B][ldo32] and / or out16 16-bit [B][ldo16].
 *   N % 4 == 0. */
int vface_cond_mix(const float* a, int rows_a, float w_a, const float* b, int rows_b, float w_b, const float* c, int rows_c, float w_c,
                   float w_sum, float* out32, int64_t ldo32, void* out16, int64_t ldo16, int B, int N, int dtype, void* stream);

/* ---- identity features (ArcFace IR-SE50) --------------------------------------------------------------------------------------------
 * The reference computes `id_feat` with `IDLoss.extract_feats` (REFace/ldm/models/diffusion/ddpm.py:91-124, :1010): a pooling and
 * crop chain in front of `Backbone(112, 50, 'ir_se')` (REFace/src/Face_models/encoders/{model_irse,helpers}.py), once for the source
 * and once per target frame (scripts/VFace_inference_batch.py:437, :442, :500).  Its convolutions are vface_conv3x3 / vface_im2col +
 * vface_gemm with the foldable BatchNorms folded on the host, its squeeze-excite pools vface_channel_stats + vface_pooled_linear, its
 * output layer one vface_gemm (vface_amd/arcface.py); these entry points are the rest.  All: raw device pointers, no allocation,
 * no synchronisation, capturable; a refusal launches nothing; no atomics (a sample's bits do not depend on the batch); fp32
 * arithmetic and one rounding per stored value.
 *
 * vface_id_prep: `extract_feats` up to the network (ddpm.py:114-119) in one pass.  img fp32 planar [B][3][H][W] ->
 *   out [B * 112 * 112][ldo >= 8] 16-bit, 8 channels written per pixel (3 values, 5 zeros).  clip_img != 0: `un_norm_clip`
 *   (x * std + mean per channel) then (x - 0.5) / 0.5; 0: the input as it is.  Then AdaptiveAvgPool2d(256) unless H == 256 (the
 *   reference's own condition; W >= 220 then), the crop [35:223, 32:220], AdaptiveAvgPool2d(112); bins floor(i In / Out) ..
 *   ceil((i + 1) In / Out), the two means nested as the reference nests them.  prep == 1 (clip_img must be set): img is a [-1, 1]
 *   frame at any size with an optional fp32 mask [B][H][W]; it is first brought to the CLIP-normalised 224 x 224 image by
 *   vface_clip_patches' prep == 1 expressions, in its order. */
int vface_id_prep(const float* img, int H, int W, const float* mask, int prep, int clip_img, void* out, int64_t ldo, int B, int dtype,
                  void* stream);

/* vface_prelu: y[m][c] = x > 0 ? x : slope[c] * x on 16-bit views x [M][ldx] -> y [M][ldy] (y may be x); slope fp32 [C].
 *   z (optional, 16-bit [M][ldz], distinct from x and y): z[m][c] = za[c] * y32 + zb[c] from the unrounded y (the first unit's
 *   leading BatchNorm2d, helpers.py:108).  C % 8 == 0. */
int vface_prelu(const void* x, int64_t ldx, const float* slope, void* y, int64_t ldy, const float* za, const float* zb, void* z,
                int64_t ldz, int64_t M, int C, int dtype, void* stream);

/* vface_se_gate_add: the end of a `bottleneck_IR_SE` unit (helpers.py:65-72, 116-119):
 *   y[m][c] = res[m][c] * g[m / (OH * OW)][c] + sc, g fp32 [nimg][ldg], one fp32 fma.  sc_stride == 0: sc is row m of a tensor of
 *   the output's size, H x W that size (the 1 x 1 convolution shortcut).  sc_stride 1 | 2: sc is pixel (n, oy * s, ox * s) of the
 *   unit's input [nimg * H * W][lds] -- MaxPool2d(1, s) -- and the output is OH x OW, OH = (H - 1) / s + 1, OW likewise.
 *   z (optional): z[m][c] = za[c] * y32 + zb[c], the NEXT unit's leading BatchNorm2d: it precedes a zero-padded convolution, so the
 *   padding must follow it and it cannot be folded.  y and z are each rounded once from the fp32 sum.  y may be res.  C % 8 == 0. */
int vface_se_gate_add(const void* res, int64_t ldr, const float* g, int64_t ldg, const void* sc, int64_t lds, int sc_stride, int nimg,
                      int H, int W, int C, void* y, int64_t ldy, const float* za, const float* zb, void* z, int64_t ldz, int dtype,
                      void* stream);

/* vface_l2norm_rows: `l2_norm` (helpers.py:15-18): out[b][:] = x[b][:] / ||x[b]||_2 on fp32 rows [B][ldx] -> [B][ldo]; the squares
 *   are summed relative to the row's largest magnitude, in a fixed order that does not depend on B.  N % 4 == 0. */
int vface_l2norm_rows(const float* x, int64_t ldx, float* out, int64_t ldo, int B, int N, void* stream);

/* The FeedForward third of BasicTransformerBlock._forward in ONE launch (REFace/ldm/modules/attention.py:243 `x = ff(norm3(x)) + x`,
 * FeedForward / GEGLU :37-64, LayerNorm :233):  out = W2 (a * gelu(g)) + b2 + x,  [a ; g] = W1 LN(x) + b1.
 * x32: the block's running sum, fp32 [M][ldx] (LayerNorm input and residual).  W1: ff.net[0].proj.weight [8C][C] 16-bit with rows
 * interleaved in 16-row value / gate blocks (the vface_gemm GEGLU packing), b1 in the same order; W2p: ff.net[2].weight [C][4C] with
 * the columns of every aligned 32-block stored in the order 8g + j <- 16 (j >> 2) + 4g + (j & 3) (the k order in which two 16 x 16
 * accumulator tiles of the hidden activations form one k32 MFMA operand: vface_amd/packing.py::pack_ffn_w2).  out16 (16-bit) and /
 * or out32 (fp32) receive the result.  The [M x 4C] hidden matrix never exists; LayerNorm statistics and the GEGLU are fp32, the
 * normalised activations and the hidden activations are rounded to 16 bits once, as in the three-kernel path.
 * Supported: C in {64, 128, 320} (one wave keeps C / 16 x 2 output tiles in registers), M % 128 == 0: vface_ffn_fused_supported();
 * other shapes: VFACE_ERR_SHAPE (the caller runs vface_layernorm + vface_gemm(GEGLU) + vface_gemm). */
int vface_ffn_fused_supported(int64_t M, int C);
int vface_ffn_fused(const float* x32, int64_t ldx, const float* gamma, const float* beta, float eps, const void* W1, const float* b1,
                    const void* W2p, const float* b2, void* out16, int64_t ldo, float* out32, int64_t ldo32, int M, int C,
                    int dtype, void* stream);

/* vface_ffn_fused with the attn1 OUT-PROJECTION in front, one launch (attention.py:239-243; the single-token attn2 is the per-sample
 * row bias):
 *   t1  = att_16 @ Wo^T + bo + rowbias[row / rows_per_sample] + resid          (fp32, never stored)
 *   out = ff.net[2]( GEGLU( ff.net[0]( LayerNorm(t1; gamma, beta, eps) ) ) ) + t1
 * att: [M][C] 16-bit attention output; resid: [M][C] fp32 (the running sum before attn1); rowbias optional fp32
 * [M / rows_per_sample][ld_rowbias] (rows_per_sample % 128 == 0).  WoW1 = [C + 8C][C] 16-bit: to_out's C rows, then ff.net[0]'s
 * 8C rows in the GEGLU-interleaved order of vface_ffn_fused with their k columns permuted like vface_st_front's projection rows
 * (packing.pack_attn_out_ffn).  b1, W2p, b2, out16 / out32, shapes: as vface_ffn_fused. */
int vface_attn_out_ffn_fused(const void* att, int64_t ldatt, const float* resid, int64_t ldr, const float* rowbias, int64_t ld_rowbias,
                             int rows_per_sample, const void* WoW1, const float* bo, const float* gamma, const float* beta, float eps,
                             const float* b1, const void* W2p, const float* b2, void* out16, int64_t ldo, float* out32,
                             int64_t ldo32, int M, int C, int dtype, void* stream);

/* ... and the SpatialTransformer's proj_out + residual behind it (attention.py:286-289 `x = proj_out(x); return x + x_in`), same launch:
 *   y = (out of vface_attn_out_ffn_fused)_16 @ Wpo^T + b_po + x_in
 * WoW1Wp = vface_attn_out_ffn_fused's stream + the C rows of proj_out with their k columns permuted the same way
 * (packing.pack_attn_out_ffn(.., w_proj_out)); x_in: the transformer's fp32 input [M][ld_xin]; y goes to out16 (optional) / out32
 * (optional, at least one); colstats (optional): [M / 64][ld_colstats][2] fp32 (sum, sum of squares) of y's columns per 64-row
 * slice -- what vface_gemm's epilogue hands the next GroupNorm (vface_groupnorm_finalize_cols / _coeffs_from_cols). */
int vface_attn_out_ffn_proj_fused(const void* att, int64_t ldatt, const float* resid, int64_t ldr, const float* rowbias, int64_t ld_rowbias,
                                  int rows_per_sample, const void* WoW1Wp, const float* bo, const float* gamma, const float* beta, float eps,
                                  const float* b1, const void* W2p, const float* b2, const float* b_po, const float* x_in, int64_t ld_xin,
                                  void* out16, int64_t ldo, float* out32, int64_t ldo32, float* colstats, int64_t ld_colstats, int M, int C,
                                  int dtype, void* stream);

/* The UNet's `out` layer in one launch (openaimodel.py:712-716, :905): out = conv3x3( SiLU( x * a[img] + b[img] )_16 ) + bias with Cout
 * in {3, 4}, Cin % 64 == 0; x: [nimg*H*W][ldx] fp32 residual-stream carrier (in_f32) or 16-bit; (a, b): vface_groupnorm_coeffs_from_cols;
 * Wt: [Cout][9*Cin] 16-bit in vface_conv3x3's k order; out: fp32 [nimg*H*W][ldo].  Replaces finalize + apply + an implicit-GEMM whose
 * 128-wide tile is 97 % padding at four output channels. */
int vface_gn_silu_conv3x3_small(const void* x, int64_t ldx, int in_f32, const float* gn_ab, int64_t ld_ab, const void* Wt, const float* bias,
                                float* out, int64_t ldo, int nimg, int H, int W, int Cin, int Cout, int dtype, void* stream);

/* Linear layers on a handful of rows -- the time-embedding chain (openaimodel.py:874-875 `emb = self.time_embed(timestep_embedding(t))`,
 * :264-271 `emb_layers(emb)` = Linear(SiLU(emb)) of every ResBlock as one matrix; util.py:151-171):
 *   out[m][n] = act( sum_k a[m][k] W[n][k] + bias[n] ),  M <= 96, N % 32 == 0, K in {320, 640, 1280}
 * a: [M][lda] 16-bit; act = SiLU when `silu`; out 16-bit, or fp32 when `out_f32`.  Replaces three vface_gemm + two vface_silu
 * launches of a forward (a 128-row GEMM tile is 81 % padding at M = 24) by three; the SiLU now acts on the fp32 sum (one rounding
 * instead of two). */
int vface_linear_small_supported(int M, int N, int K);
int vface_linear_small(const void* a, int64_t lda, const void* W, int64_t ldw, const float* bias, void* out,
                       int64_t ldo, int out_f32, int silu, int M, int N, int K, int dtype, void* stream);

/* Fused FRONT of a SpatialTransformer (attention.py:278-284 norm -> proj_in -> tokens; :239 norm1; :179-183 to_q / to_k / to_v of
 * attn1), one launch for GroupNorm-apply + proj_in + LayerNorm + the attn1 projection on token matrices with C in {64, 128, 320}:
 *   t0  = (x32 * a[img] + b[img])_16 @ W_in^T + b_in            fp32 [M][C]   (the carrier the attn1 out-projection adds to)
 *   qkv = LayerNorm(t0; gamma, beta, eps)_16 @ W_p^T            16-bit [M][ldq], projection column j at qkv[:, j]
 * (a, b) = vface_groupnorm_coeffs_from_cols of x's producer (fp32 pairs [nimg][ld_ab][2]); hw = rows per image, M % 128 == 0,
 * hw % 128 == 0.  Wcat = [C + NQ][C] 16-bit: the C rows of proj_in, then the NQ projection rows with their k columns permuted
 * inside every aligned block of 16: position 8 h + j holds original column 8 (j >> 2) + 4 h + (j & 3) (packing.ffn_w2_perm).
 * Rows [0, rows_full) get projection columns [0, NQ), the others only [nq_lo, NQ) (the hook's "replace": chunks >= 1 project V
 * only, pnp_utils.py:133-142); rows_full % 128 == 0, NQ % 32 == 0, nq_lo % 32 == 0.  ln (optional): LayerNorm(t0) as a 16-bit
 * matrix too (what the dual-source projections of the hook's linear fusions read).  No workspace; capturable. */
int vface_st_front_supported(int64_t M, int C, int hw);
int vface_st_front(const float* x32, int64_t ldx, const float* gn_ab, int64_t ld_ab, int hw, const void* Wcat, const float* b_in,
                   const float* gamma, const float* beta, float eps, float* t0, int64_t ldt0, void* qkv, int64_t ldq, void* ln,
                   int64_t ldln, int M, int C, int NQ, int rows_full, int nq_lo, int dtype, void* stream);

/* fusion="temporal" (pnp_utils.py:59-90,145-154): 5-tap Gaussian (sigma 1, renormalised at the clip ends) over the
 * FRAME axis of src [F][n][C] (chunk 0's q|k), written to dst1 and dst2 (chunk 1 and chunk 2). */
int vface_temporal_gauss(const void* src, int64_t ld_src, int64_t fs_src, void* dst1, void* dst2, int64_t ld_dst,
                         int64_t fs_dst, int F, int n, int C, int dtype, void* stream);
/* fusion="adaIn" (face_swap_utils.py:372-389, normalized=True): per-row AdaIN of a (structure) to b (own) over
 * the channel axis, then division by the GLOBAL unbiased std of the fused tensor: dst [rows][C]. */
size_t vface_adain_workspace_bytes(int64_t rows, int C);
int vface_adain_fusion(const void* a, int64_t lda, const void* b, int64_t ldb, void* dst, int64_t ldd, int64_t rows, int C,
                       void* workspace, size_t workspace_bytes, int dtype, void* stream);

/* The two frame-coupled modes on a FRAME SHARD (parallel.FrameShard: this rank holds global frames [first, first + F) of a clip
 * of F_total frames; the forward exchanges what the edit needs from the other ranks between these launches).
 * vface_temporal_gauss on the shard: window frames outside it are read from prev (global frames first-2, first-1 at slab 0, 1)
 * and next (global first+F, first+F+1 at slab 0, 1), slab s / token t / channel c at base[s*fs_halo + t*ld_halo + c]; the
 * window still ends only at the clip's real ends (0, F_total).  prev may be NULL iff first == 0, next iff first + F == F_total;
 * slabs whose frame lies outside the clip are not read.  The shard's rows equal vface_temporal_gauss's rows of the whole clip
 * bit for bit (same taps, order and weights).  No workspace; capturable. */
int vface_temporal_gauss_halo(const void* src, int64_t ld_src, int64_t fs_src, const void* prev, const void* next, int64_t ld_halo,
                              int64_t fs_halo, void* dst1, void* dst2, int64_t ld_dst, int64_t fs_dst, int F, int first, int F_total,
                              int n, int C, int dtype, void* stream);
/* vface_adain_fusion in two launches around a cross-rank gather.  vface_adain_rows: the per-row AdaIN of this shard's rows into
 * the workspace (fp32) and each row's partial (sum, centred sum of squares) into partial [rows][2] (fp64).
 * vface_adain_reduce_scale: the global unbiased std from partial [partial_rows][2] -- every rank's partials in global row order,
 * the array vface_adain_fusion reduces over -- then dst [rows][C] = fused / (std + 1e-5) from the workspace vface_adain_rows
 * filled (same rows, C).  Rows + reduce_scale over the whole array equal vface_adain_fusion bit for bit.  Capturable. */
size_t vface_adain_rows_workspace_bytes(int64_t rows, int C);
int vface_adain_rows(const void* a, int64_t lda, const void* b, int64_t ldb, int64_t rows, int C, double* partial, void* workspace,
                     size_t workspace_bytes, int dtype, void* stream);
int vface_adain_reduce_scale(const double* partial, int64_t partial_rows, int C, void* workspace, size_t workspace_bytes, void* dst,
                             int64_t ldd, int64_t rows, int dtype, void* stream);

/* Small ops */
/* util.py:151-171 timestep_embedding: out[N][dim] = [cos(t f_i) | sin(t f_i)] */
int vface_timestep_embedding(const int64_t* t, void* out, int N, int dim, int dtype, void* stream);
/* nn.SiLU on a flat buffer (time_embed / emb_layers, openaimodel.py:218-224,631-636); in_f32: x is fp32 */
int vface_silu(const void* x, void* y, int64_t count, int in_f32, int dtype, void* stream);

/* ---- first-stage KL-VAE (ldm/models/autoencoder.py:285-335, diffusionmodules/model.py:368-570) ----
 * The encoder / decoder are sequences of vface_conv3x3 (VFACE_CONV_PAD_TRAILING for Downsample :72-77, `upsample` for
 * Upsample :55-58), vface_groupnorm_* (eps 1e-6, swish) and vface_gemm; two more entry points cover what is new. */
/* P[m][:] = softmax(scores[m][:] * scale), fp32 in, 16-bit out, N <= 16384 (AttnBlock :183-186: one head of 512 channels;
 * its scores come from vface_gemm with VFACE_EPI_OUT_F32). */
int vface_softmax_rows(const float* scores, int64_t ld_s, void* P, int64_t ld_p, int M, int N, float scale, int dtype,
                       void* stream);
/* z[F][zc][hw] (fp32 NCHW) = (mean + exp(0.5*clamp(logvar,-30,20)) * noise) * scale from moments [F*hw][ld >= 2*zc] (fp32
 * NHWC: mean | logvar); noise NULL = mode.  DiagonalGaussianDistribution.sample (distributions.py:24-37) followed by
 * get_first_stage_encoding's scale_factor. */
int vface_vae_sample(const float* moments, int64_t ld_moments, const float* noise, float* z, int F, int hw, int zc,
                     float scale, void* stream);
int vface_cast_f32(const float* src, void* dst, int64_t count, int dtype, void* stream);
/* ddim_w_inv.py:633,654-655: x_in = cat[cat[x,inp,mask], cat[x,inp,mask], cat[inv_t,inp,mask]] -> NHWC [3F][hw][cpad].
 * inv == NULL: only [uncond ; cond] = [2F][hw][cpad] (the recon third of the batch is a pure sink of the sampler -- its x_prev is
 * dropped, ddim_w_inv.py:703-707,738, and no hook mode reads chunk 2 -- so a caller may leave it out: exact). */
int vface_pack_unet_input(const float* x, const float* inv, const float* inpaint, const float* mask, void* out, int F,
                          int h, int w, int cpad, int dtype, void* stream);
int vface_nchw_to_nhwc(const float* x, void* out, int N, int C, int hw, int cpad, int dtype, void* stream);
int vface_nhwc_to_nchw_f32(const float* x, int64_t ldx, float* out, int N, int C, int hw, void* stream);
/* ddim_w_inv.py:666-667,686-700: guidance + x0 prediction + x_{t-1}; eps = NHWC fp32 UNet output of
 * [uncond ; cond ; recon]; x, inv, outputs NCHW fp32 [F][C][hw].  pred_x0 / x_prev_recon / noise optional.
 * single_branch == 1: eps holds ONE branch [F] and is used unguided -- with a_t = a(t - T/S), a_prev = a(t),
 * sigma 0 this is the inversion update of ddim_invert (ddim_w_inv.py:436-449).  single_branch == 2: eps holds [uncond ; cond]
 * only ([2F]: see vface_pack_unet_input with inv == NULL); x_prev_recon is then not written. */
int vface_ddim_step(const float* eps, int64_t lde, const float* x, const float* inv, float* x_prev, float* pred_x0,
                    float* x_prev_recon, int F, int C, int hw, float scale, float a_t, float a_prev, float sigma_t,
                    float sqrt_one_minus_at, const float* noise, int single_branch, void* stream);
/* strided 2-D copy of 16-bit rows (th.cat([h, hs.pop()], 1), openaimodel.py:898, when not written in place) */
int vface_copy2d(const void* src, int64_t ld_src, void* dst, int64_t ld_dst, int64_t rows, int cols, int dtype,
                 void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VFACE_HIP_H */
