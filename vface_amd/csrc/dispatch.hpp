// The GEMM-family launch plan: dispatch.cpp validates a vface_gemm / vface_conv3x3 / vface_conv3x3_plus_1x1 / vface_upsample2x_conv3x3_phase call, fills
// the extents and composes every rule into one VfGemmPlan; the launchers in gemm.hip, gemm_big.hip, conv.hip and inconv.hip map it onto a template
// instantiation and evaluate nothing.  Host-only: no HIP header, so a plain C++ compiler builds it and tests/test_dispatch_cpu.py pins it without a GPU.
#pragma once
#include <stdint.h>

enum { GEMM_GEGLU = 1, GEMM_OUT_F32 = 2, GEMM_NO_XCD_REMAP = 0x1000, GEMM_NO_SETPRIO = 0x2000, GEMM_STAMPS = 0x4000 /* the stamped instantiation: cycle counts per part go to the colstats pointer (tools/stamp_gemm.py, stamp_conv.py) */, GEMM_NARROW_EPILOGUE = 0x8000, GEMM_NO_PERSIST = 0x10000, GEMM_PERSIST = 0x20000,
       GEMM_NO_PATCH = 0x80000, GEMM_PATCH = 0x100000, GEMM_GN8 = 0x8000000 /* A/B: fixed column groups of 8 n-tiles in the plain GEMM's tile order */, GEMM_NO_Q8 = 0x4000000 /* A/B: the 8x8 level stays on the im2col kernel */, GEMM_PATCH_BN160 = 0x2000000 /* A/B: the patch kernel's 160-wide tile wherever it divides N */, GEMM_F32_TRANSPOSE = 0x1000000 /* A/B: epilogue transposes in fp32 even where 16 bits would do */,
       GEMM_BIG = 0x10000000 /* take gemm_big.hip's 256 x 320 tile whenever the launch qualifies */, GEMM_NO_BIG = 0x20000000 /* A/B: never */,
       GEMM_BIG_W256 = 0x200000 /* gemm_big.hip: the 256-channel tile width wherever N allows it */, GEMM_BIG_W320 = 0x400000 /* ... never */ };  // (0x40000 = VFACE_CONV_PAD_TRAILING)  // bits 8..11 of flags: forced schedule variant (0 = automatic)

struct GemmParams {
    int mode;  // 0: plain A[M][K]; 1: implicit 3x3 conv over NHWC
    const void* A;
    long lda;  // plain: row stride; conv: pixel stride (>= Cin) in elements
    const void* A2;  // optional second source for k >= K1 (plain mode), row = m % a2_row_mod
    long lda2;
    int K1, a2_row_mod;
    const void* Wt;  // [N][ldw]
    long ldw;
    int Kw;  // valid k columns of Wt (multiple of 8)
    int M, N, K;
    // conv geometry (stored input H x W, output OH x OW)
    int H, W, Cin, OH, OW, stride, upsample;
    int pad;  // leading (top) zero padding: 1, or 0 for the VAE encoder's (0,1,0,1) stride-2 convolution
    int pad_x;           // leading (left) zero padding; KH x KW window (ntaps = KH*KW <= 9; 0 = the plan fills 3x3)
    int KH, KW, ntaps;
    int out_phase;       // 0, or 4 | (py << 1) | px: output rows are the (py, px) parity phase of a 2OH x 2OW image
    const float* bias;     // [N] or null
    const float* rowbias;  // [M / rows_per_sample][ld_rowbias] or null
    int rows_per_sample;
    int ld_rowbias;
    const void* residual;  // [M][ldr] or null
    long ldr;
    void* C;  // [M][ldc] 16-bit (or fp32 with GEMM_OUT_F32); may be null when C32 is given
    long ldc;
    // fp32 residual stream: `residual` is fp32 [M][ldr] when res_f32; C32 (optional) receives the fp32 sum
    // bias + rowbias + residual + acc BEFORE the rounding to 16 bits -- the carrier the next residual add / norm reads
    int res_f32;
    float* C32;
    long ldc32;
    // fused input normalisation (patch-staged convolution only): the operand the matrix cores see is
    // act(x * a[img][ci] + b[img][ci]) with (a, b) fp32 pairs at gn_ab[(img * ld_gn_ab + ci) * 2]; act = SiLU if gn_silu
    const float* gn_ab;
    long ld_gn_ab;
    int gn_silu;
    unsigned gn_ab_bytes;   // filled by the plan
    const void* zeros;  // >= 16 zero bytes, 16-B aligned
    int flags;
    unsigned a_bytes, a2_bytes, w_bytes;  // filled by the plan: extents of the operand views
    float* colstats;     // optional [ceil(M/64)][ld_colstats][2] per-64-row-slice column (sum, sumsq) of the stored values
    long ld_colstats;
    // split-K (plan-chosen when a workspace is supplied and the tile grid underfills the chip): fp32 partial tiles
    // [split_k][M][N] in `workspace`, summed in split order by a second kernel that also runs the epilogue
    float* workspace;
    long workspace_bytes;
    int split_k, kt_per_split;  // filled by the plan
    int tile_group;             // n-tiles per column group of the XCD-aware tile order (plan; 0 = 8)
    unsigned res_bytes, c_bytes, c32_bytes;  // gemm_big.hip, inconv.hip (filled by the plan): extents of the residual view, of the 16-bit output view and of the fp32 carrier view
};

// tile shapes the rules reason about, which the kernel files take from here: gemm.hip's rows and K depth per tile, conv.hip's TP x TP-pixel output tile,
// gemm_big.hip's tile, inconv.hip's output channels per wave and its K (9 taps x 16 stored channels)
constexpr int VF_GEMM_BM = 128, VF_GEMM_BK = 64, VF_PATCH_TP = 16, VF_BIG_BM = 256, VF_BIG_BN = 320, VF_IN16_CH = 80, VF_IN16_K = 144;

// gemm.hip's 128-row implicit GEMM (plain or im2col-style) | conv.hip's patch-staged stride-1 convolution | its 8x8 form (four images per workgroup,
// K split over channel chunks) | a plain GEMM through it (GEMM_PATCH) | gemm_big.hip's 256 x 320 | 256 tile | inconv.hip's 16-stored-channel input convolution
enum VfGemmKernel { VF_KERNEL_GEMM, VF_KERNEL_CONV_PATCH, VF_KERNEL_CONV_Q8, VF_KERNEL_GEMM_PATCH, VF_KERNEL_GEMM_BIG, VF_KERNEL_CONV_IN16 };

// Everything a launcher needs.  `p`: the validated GemmParams with every extent, split_k, kt_per_split, tile_group filled (GEMM_PATCH: geometry rewritten)
struct VfGemmPlan {
    GemmParams p;
    int kernel, bn;    // VfGemmKernel; tile width in channels
    int stages, mode;  // gemm.hip: LDS stages 1 | 2; 0 plain | 1 convolution, Cin % 64 == 0 | 2 convolution, generic window.  conv.hip: mode = the window, 3 | 2
    int form;          // residual form 0 none | 1 16-bit | 2 fp32 | 3 cycle stamps (GEMM_STAMPS) (conv.hip also 4 fused GroupNorm); gemm_big.hip: epilogue 0 bias | 1 GEGLU | 2 residual | 3 fp32 stream
    bool persistent;   // gemm.hip: grid_x resident workgroups walk the tiles
    bool reduce;       // the split-K reduce follows: it sums the fp32 partial tiles in split order and runs the epilogue (always behind the 8x8 form)
    int grid_x, grid_y, lds_bytes;      // (dynamic LDS)
    int slices_per_wg; // inconv.hip: 64-pixel slices one workgroup walks
};

// persistent_grid: workgroups a persistent launch keeps resident, the one device figure the rules need.  Returns VFACE_OK or the error the call answers.
int vf_plan_gemm(const GemmParams& p, int persistent_grid, VfGemmPlan* plan);
long vf_splitk_workspace_bytes(int M, int N, int K, int flags, int rows_per_sample);
int vf_conv_uses_patch_kernel(int H, int W, int Cin, int Cout, int window, int stride, int upsample, int flags);   // 0 im2col | 1 patch | 2 8x8 form
