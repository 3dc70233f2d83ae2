// What capi.cpp, or one kernel file of another, needs from the kernel files: the parameter structs and launchers of the entry
// points that capi.cpp sequences, and the launchers gemm.hip's dispatch calls across files.  An entry point that only validates
// and launches is defined beside its kernel as the extern "C" function itself and is not declared here (include/vface_hip.h is).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <atomic>

// hipFuncSetAttribute(MaxDynamicSharedMemorySize) is a per-DEVICE setting of a kernel: one bit per device ordinal, set with an
// atomic OR (two host threads launching the same kernel for the first time both set the attribute -- idempotent -- and neither
// skips it; a process that drives a second GPU sets it there too)
struct VfOncePerDevice {
    std::atomic<unsigned long long> done{0};
    bool set_lds(const void* kern, int bytes) {
        int dev = 0;
        if (hipGetDevice(&dev) != hipSuccess) return false;
        const unsigned long long bit = 1ull << (dev & 63);
        if (done.load(std::memory_order_acquire) & bit) return true;
        if (hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, bytes) != hipSuccess) return false;
        done.fetch_or(bit, std::memory_order_release);
        return true;
    }
};

#include "dispatch.hpp"      // GemmParams, the GEMM_* flag bits and the launch plan
bool vf_gemm_variants_built();
int vf_launch_gemm(const GemmParams& p, int dtype, hipStream_t stream);
int vf_launch_conv_patch(const VfGemmPlan& plan, int dtype, hipStream_t stream);   // conv.hip: the patch-staged kernel, its 8x8 form (main pass) and its plain-GEMM form
int vf_launch_gemm_big(const VfGemmPlan& plan, int dtype, hipStream_t stream);     // gemm_big.hip: the 256 x 320 | 256 tile
int vf_launch_conv_in16(const VfGemmPlan& plan, int dtype, hipStream_t stream);    // inconv.hip: the 16-stored-channel input convolution (K = 144 in one MFMA pass)
bool vf_attention_shared_scores_supported(int dh, int v_sets);

// ffn.hip: fused LayerNorm -> ff.net[0] (GEGLU) -> ff.net[2] -> + x over token matrices with C in {64, 128, 320}, M % 128 == 0
struct FfnParams {
    const float* x32; long ldx;      // [M][C] fp32: the block's running sum (LayerNorm input AND residual)
    const float* gamma; const float* beta; float eps;
    const void* W1;                  // [8C][C] 16-bit, GEGLU rows interleaved in 16-row value / gate blocks (packing.pack_geglu)
    const float* b1;                 // [8C] in the same row order
    const void* W2p;                 // [C][4C] 16-bit, columns permuted per 32 (packing.pack_ffn_w2)
    const float* b2;                 // [C]
    void* out16; long ldo;           // [M][C] 16-bit result (or null)
    float* out32; long ldo32;        // optional fp32 result
    int M, C;
    // att != null: the attn1 out-projection runs in front (ffn.hip "PRE"): x32 is unused, the running sum is formed in-kernel as
    // t1 = att @ Wo^T + bo + rowbias[row / rows_per_sample] + resid; W1 is then [C + 8C][C]: to_out's rows, then ff.net[0]'s
    // (GEGLU-interleaved rows, k columns in ffn_w2_perm order)
    const void* att; long ldatt;     // [M][C] 16-bit attention output
    const float* resid; long ldr;    // [M][C] fp32: the running sum before attn1 (t0)
    const float* bo;                 // [C] to_out bias
    const float* rowbias; long ld_rowbias; int rows_per_sample;   // optional fp32 [M / rows_per_sample][ld]: attn2's contribution
    // Wpo_in_stream (with att): the SpatialTransformer's proj_out runs behind (ffn.hip "POST"): W1 is [C + 8C + C][C] -- proj_out's rows
    // last, k columns in ffn_w2_perm order --, the outputs are y = proj_out(t3) + b_po + x_in and its per-64-row column statistics
    int Wpo_in_stream;
    const float* b_po;               // [C]
    const float* x_in; long ld_xin;  // [M][C] fp32: the SpatialTransformer's input
    float* colstats; long ld_colstats;   // optional [M / 64][ld][2] (sum, sum of squares) of y
};
bool vf_ffn_fused_supported(long M, int C);
int vf_launch_ffn_fused(const FfnParams& p, int dtype, hipStream_t stream);

// linear_small.hip: out[M][N] = act(a[M][K] W[N][K]^T + bias) on M <= 96 rows (the time-embedding chain)
struct LinearSmallParams {
    const void* a; long lda;         // [M][K] 16-bit
    const void* W; long ldw;         // [N][K] 16-bit
    const float* bias;               // [N] or null
    void* out; long ldo; int out_f32;
    int silu;
    int M, N, K;
};
bool vf_linear_small_supported(int M, int N, int K);
int vf_launch_linear_small(const LinearSmallParams& p, int dtype, hipStream_t stream);

// stfront.hip: GroupNorm-apply -> proj_in -> (t0 out) -> LayerNorm -> attn1 projection, one launch; C in {64, 128, 320}
struct StFrontParams {
    const float* x32; long ldx;      // [M][C] fp32: the SpatialTransformer's input (residual-stream carrier)
    const float* ab; long ld_ab;     // GroupNorm (scale, shift) pairs [nimg][ld_ab][2] (vface_groupnorm_coeffs_from_cols)
    int hw;                          // rows per image (a multiple of 128)
    const void* Wcat;                // [C + NQ][C] 16-bit: proj_in rows, then the projection rows with k columns in ffn_w2_perm order
    const float* b_in;               // [C] proj_in bias
    const float* gamma; const float* beta; float eps;   // norm1
    float* t0; long ldt0;            // [M][C] fp32 out: proj_in(GroupNorm(x)) + bias
    void* qkv; long ldq;             // [M][ldq] 16-bit out: projection column j at qkv[:, j]
    void* ln; long ldln;             // optional [M][C] 16-bit out: LayerNorm(t0)
    int M, C, NQ;
    int rows_full, nq_lo;            // rows [0, rows_full): projection columns [0, NQ); the other rows: columns [nq_lo, NQ)
    int gridA;                       // filled by the launcher
};
bool vf_st_front_supported(long M, int C, int hw);
int vf_launch_st_front(const StFrontParams& p, int dtype, hipStream_t stream);

// outconv.hip: GroupNorm-apply + SiLU + 3x3 convolution to 3 / 4 output channels in one launch (the UNet's `out` layer)
struct OutConvParams {
    const void* x; long ldx; int in_f32;   // [nimg*H*W][ldx] fp32 carrier (in_f32) or 16-bit
    const float* ab; long ld_ab;           // GroupNorm (scale, shift) pairs [nimg][ld_ab][2]
    const void* Wt;                        // [Cout][9*Cin] 16-bit, k order (64-channel chunk, tap, channel) (packing.pack_conv3x3)
    const float* bias;                     // [Cout] or null
    float* out; long ldo;                  // [nimg*H*W][ldo] fp32
    int nimg, H, W, Cin, Cout;
};
bool vf_out_conv_supported(int Cin, int Cout);
int vf_launch_out_conv(const OutConvParams& p, int dtype, hipStream_t stream);

struct AttnParams {
    const void* Q; const void* K; const void* V;  // [B][n][ld*], head h at column h*dh
    long ldq, ldk, ldv;           // row (token) strides in elements
    long bsq, bsk, bsv;           // batch (sample) strides in elements
    const int* qk_map;            // [B] source sample of q,k for output sample b, or null (identity)
    const int* v_map;             // [B] source sample of v, or null
    void* O; long ldo, bso;       // [B][n][ldo]
    int B, heads, n, nk, dh;      // nk = number of keys (== n for self-attention)
    float scale;
    int variant;  // 0 = automatic; queries-per-wave variants for A/B benchmarking
    unsigned k_bytes, v_bytes;    // filled by the launcher: extents of the K / V views (buffer descriptors, < 4 GiB)
    int v_sets, set_stride;  // > 1: B q/k samples; output (and value) sample of set g is b + g*set_stride, scores shared
    int v_sets_live;         // 0 = all; 2 of v_sets == 3: only sets 0, 1 are read / written, with the arithmetic of the full call
};
int vf_launch_attention(const AttnParams& p, int dtype, hipStream_t stream);

// png_in.hip: vface_png_inflate's one-wave-per-file kernel on the files whose flag is set (flags == nullptr: on all), for
// png_in_par.hip's fallback; the arguments are vface_png_inflate's, already checked
int vf_launch_png_inflate(const uint8_t* streams, int64_t stream_bytes, const int64_t* offsets, const int32_t* lengths, int files, uint8_t* rows,
                          int64_t file_stride, int64_t expect, int32_t* status, int32_t* produced, int32_t* consumed, uint32_t* adler,
                          const int* flags, hipStream_t stream);

// pointwise.hip / raft.hip: what capi.cpp's size queries and workspace checks call
int vf_gn_partial_floats(int nimg, int hw, int C, int groups);
int vf_chan_stats_slices(int hw);
int vf_launch_timestep_embedding(const long long* t, void* out, int N, int dim, int dtype, hipStream_t stream);
size_t vf_adain_workspace_bytes(long rows, int C);
int vf_launch_adain(const void* a, long lda, const void* b, long ldb, void* dst, long ldd, long rows, int C, void* ws,
                    int dtype, hipStream_t stream);
size_t vf_adain_rows_workspace_bytes(long rows, int C);
int vf_launch_adain_rows(const void* a, long lda, const void* b, long ldb, long rows, int C, double* partial, void* ws,
                         int dtype, hipStream_t stream);
int vf_launch_adain_reduce_scale(const double* partial, long partial_rows, int C, void* ws, void* dst, long ldd, long rows,
                                 int dtype, hipStream_t stream);
