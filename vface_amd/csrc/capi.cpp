// The entry points of libvface_hip.so (include/vface_hip.h) that decide something before a launch: they fill a parameter struct,
// check a workspace or answer a query.  Every other entry point is defined in its kernel's .hip file.
#include "../../include/vface_hip.h"

#include <hip/hip_runtime.h>

#include "launch.hpp"
#include "vface_kernels.hpp"

namespace {
GemmParams plain_gemm(const void* A, long lda, const void* Wt, long ldw, int M, int N, int K, const float* bias,
                      void* C, long ldc, const void* zeros) {
    GemmParams p{};
    p.mode = 0; p.A = A; p.lda = lda; p.Wt = Wt; p.ldw = ldw; p.Kw = K; p.M = M; p.N = N; p.K = K;
    p.bias = bias; p.C = C; p.ldc = ldc; p.zeros = zeros;
    return p;
}
// the optional fp32 residual stream of a GEMM-family call
inline void apply_s32(GemmParams& p, const vface_stream32* s) {
    if (!s) return;
    if (s->residual32) { p.residual = s->residual32; p.ldr = s->ldr32; p.res_f32 = 1; }
    if (s->out32) { p.C32 = s->out32; p.ldc32 = s->ldo32; }
    if (s->in_scale_shift) { p.gn_ab = s->in_scale_shift; p.ld_gn_ab = s->ld_scale_shift; p.gn_silu = s->in_silu ? 1 : 0; }
}
}  // namespace

extern "C" {

int vface_abi_version(void) { return VFACE_ABI_VERSION; }
int vface_gemm_variants_built(void) { return vf_gemm_variants_built() ? 1 : 0; }

const char* vface_error_string(int code) {
    switch (code) {
        case VFACE_OK: return "ok";
        case VFACE_ERR_ARG: return "invalid argument (null pointer or non-positive size)";
        case VFACE_ERR_ALIGN: return "pointer or leading dimension not aligned (16-bit rows need 16 B, channels % 8)";
        case VFACE_ERR_SHAPE: return "unsupported shape";
        case VFACE_ERR_DTYPE: return "unsupported dtype (0 = fp16, 1 = bf16)";
        case VFACE_ERR_LAUNCH: return "kernel launch failed";
        case VFACE_ERR_WORKSPACE: return "workspace too small";
        default: return "unknown error";
    }
}

int vface_gemm(const void* A, int64_t lda, const void* A2, int64_t lda2, int K1, int a2_row_mod, const void* Wt,
               int64_t ldw, int M, int N, int K, const float* bias, const float* rowbias, int rows_per_sample,
               int ld_rowbias, const void* residual, int64_t ldr, void* C, int64_t ldc, const void* zeros, int flags,
               int dtype, float* colstats, int64_t ld_colstats, void* workspace, int64_t workspace_bytes, void* stream,
               const vface_stream32* s32) {
    GemmParams p = plain_gemm(A, lda, Wt, ldw, M, N, K, bias, C, ldc, zeros);
    p.colstats = colstats; p.ld_colstats = ld_colstats;
    p.workspace = static_cast<float*>(workspace); p.workspace_bytes = workspace ? workspace_bytes : 0;
    p.A2 = A2; p.lda2 = lda2; p.K1 = K1; p.a2_row_mod = a2_row_mod;
    p.rowbias = rowbias; p.rows_per_sample = rows_per_sample; p.ld_rowbias = ld_rowbias;
    p.residual = residual; p.ldr = ldr; p.flags = flags;
    apply_s32(p, s32);
    return vf_launch_gemm(p, dtype, vf_stream(stream));
}

int vface_conv3x3(const void* X, int64_t ldx, int nimg, int H, int W, int Cin, const void* Wt, int64_t ldw, int Cout,
                  int stride, int upsample, const float* bias, const float* rowbias, int ld_rowbias,
                  const void* residual, int64_t ldr, void* Y, int64_t ldy, const void* zeros, int flags, int dtype,
                  float* colstats, int64_t ld_colstats, void* workspace, int64_t workspace_bytes, void* stream,
                  const vface_stream32* s32) {
    if (nimg <= 0 || H <= 0 || W <= 0 || Cin <= 0 || Cout <= 0) return VFACE_ERR_ARG;
    if (stride != 1 && stride != 2) return VFACE_ERR_SHAPE;
    if (flags & VFACE_EPI_GEGLU) return VFACE_ERR_SHAPE;
    GemmParams p{};
    p.mode = 1; p.A = X; p.lda = ldx; p.Wt = Wt; p.ldw = ldw; p.Kw = 9 * Cin;
    p.H = H; p.W = W; p.Cin = Cin; p.stride = stride; p.upsample = upsample ? 1 : 0;
    const int VH = upsample ? 2 * H : H, VW = upsample ? 2 * W : W;
    // VFACE_CONV_PAD_TRAILING: zero padding (0,1,0,1) -- F.pad then a padding-0 convolution (diffusionmodules/model.py:72-77)
    p.pad = (flags & VFACE_CONV_PAD_TRAILING) ? 0 : 1;
    p.OH = (VH + p.pad + 1 - 3) / stride + 1; p.OW = (VW + p.pad + 1 - 3) / stride + 1;
    p.M = nimg * p.OH * p.OW; p.N = Cout; p.K = 9 * Cin;
    p.bias = bias; p.rowbias = rowbias; p.rows_per_sample = p.OH * p.OW; p.ld_rowbias = ld_rowbias;
    p.residual = residual; p.ldr = ldr; p.C = Y; p.ldc = ldy; p.zeros = zeros; p.flags = flags;
    p.colstats = colstats; p.ld_colstats = ld_colstats;
    p.workspace = static_cast<float*>(workspace); p.workspace_bytes = workspace ? workspace_bytes : 0;
    apply_s32(p, s32);
    return vf_launch_gemm(p, dtype, vf_stream(stream));
}

int vface_conv_uses_patch_kernel(int H, int W, int Cin, int Cout, int window, int stride, int upsample, int flags) {
    return vf_conv_uses_patch_kernel(H, W, Cin, Cout, window, stride, upsample, flags);     // the plan's own rule (dispatch.cpp), not a restatement of it
}

int vface_conv3x3_plus_1x1(const void* X, int64_t ldx, int nimg, int H, int W, int Cin, const void* X2, int64_t ldx2, int C2,
                           const void* Wt, int64_t ldw, int Cout, const float* bias, const float* rowbias, int ld_rowbias,
                           void* Y, int64_t ldy, const void* zeros, int flags, int dtype, float* colstats,
                           int64_t ld_colstats, void* workspace, int64_t workspace_bytes, void* stream,
                           const vface_stream32* s32) {
    if (nimg <= 0 || H <= 0 || W <= 0 || Cin <= 0 || Cout <= 0 || C2 <= 0 || !X2) return VFACE_ERR_ARG;
    if (flags & (VFACE_EPI_GEGLU | VFACE_CONV_PAD_TRAILING)) return VFACE_ERR_SHAPE;
    GemmParams p{};
    p.mode = 1; p.A = X; p.lda = ldx; p.Wt = Wt; p.ldw = ldw; p.Kw = 9 * Cin + C2;
    p.A2 = X2; p.lda2 = ldx2; p.K1 = 9 * Cin;
    p.H = H; p.W = W; p.Cin = Cin; p.stride = 1; p.upsample = 0; p.pad = 1;
    p.OH = H; p.OW = W;
    p.M = nimg * H * W; p.N = Cout; p.K = 9 * Cin + C2;
    p.bias = bias; p.rowbias = rowbias; p.rows_per_sample = H * W; p.ld_rowbias = ld_rowbias;
    p.C = Y; p.ldc = ldy; p.zeros = zeros; p.flags = flags;
    p.colstats = colstats; p.ld_colstats = ld_colstats;
    p.workspace = static_cast<float*>(workspace); p.workspace_bytes = workspace ? workspace_bytes : 0;
    apply_s32(p, s32);
    return vf_launch_gemm(p, dtype, vf_stream(stream));
}

int vface_upsample2x_conv3x3_phase(const void* X, int64_t ldx, int nimg, int H, int W, int Cin, const void* Wt, int64_t ldw,
                                   int Cout, int py, int px, const float* bias, const float* rowbias, int ld_rowbias, void* Y,
                                   int64_t ldy, const void* zeros, int flags, int dtype, float* colstats,
                                   int64_t ld_colstats, void* stream, const vface_stream32* s32) {
    if (nimg <= 0 || H <= 0 || W <= 0 || Cin <= 0 || Cout <= 0 || (py & ~1) || (px & ~1)) return VFACE_ERR_ARG;
    if (s32 && s32->residual32) return VFACE_ERR_SHAPE;
    if (flags & (VFACE_EPI_GEGLU | VFACE_EPI_OUT_F32 | VFACE_CONV_PAD_TRAILING)) return VFACE_ERR_SHAPE;
    GemmParams p{};
    p.mode = 1; p.A = X; p.lda = ldx; p.Wt = Wt; p.ldw = ldw; p.Kw = 4 * Cin;
    p.H = H; p.W = W; p.Cin = Cin; p.stride = 1; p.upsample = 0;
    // output parity py sees source rows {i-1, i} (py = 0) or {i, i+1} (py = 1): a 2-tap window with leading pad 1 - py
    p.KH = p.KW = 2; p.ntaps = 4; p.pad = 1 - py; p.pad_x = 1 - px;
    p.OH = H; p.OW = W; p.out_phase = 4 | (py << 1) | px;
    p.M = nimg * H * W; p.N = Cout; p.K = 4 * Cin;
    p.bias = bias; p.rowbias = rowbias; p.rows_per_sample = H * W; p.ld_rowbias = ld_rowbias;
    p.C = Y; p.ldc = ldy; p.zeros = zeros; p.flags = flags;
    p.colstats = colstats; p.ld_colstats = ld_colstats;
    apply_s32(p, s32);
    return vf_launch_gemm(p, dtype, vf_stream(stream));
}

int64_t vface_splitk_workspace_bytes(int M, int N, int K, int flags, int rows_per_sample) {
    if (M <= 0 || N <= 0 || K <= 0) return 0;
    return vf_splitk_workspace_bytes(M, N, K, flags, rows_per_sample);
}

int vface_attention(const void* Q, const void* K, const void* V, int64_t ldq, int64_t ldk, int64_t ldv, int64_t bsq,
                    int64_t bsk, int64_t bsv, const int32_t* qk_map, const int32_t* v_map, void* O, int64_t ldo,
                    int64_t bso, int B, int heads, int n, int nk, int dh, float scale, int dtype, int v_sets,
                    int set_stride, void* stream) {
    AttnParams p{};
    p.v_sets = v_sets & 0xFF; p.v_sets_live = (v_sets >> 8) & 0xFF; p.set_stride = set_stride;      // (bits 8..15: live sets)
    p.Q = Q; p.K = K; p.V = V; p.ldq = ldq; p.ldk = ldk; p.ldv = ldv; p.bsq = bsq; p.bsk = bsk; p.bsv = bsv;
    p.qk_map = qk_map; p.v_map = v_map; p.O = O; p.ldo = ldo; p.bso = bso;
    p.B = B; p.heads = heads; p.n = n; p.nk = nk; p.dh = dh; p.scale = scale;
    p.variant = dtype >> 8;  // bits 8+ of dtype: schedule variant (benchmarking); 0 = automatic
    return vf_launch_attention(p, dtype & 0xFF, vf_stream(stream));
}

int vface_attention_shared_scores_supported(int dh, int v_sets) {
    return vf_attention_shared_scores_supported(dh, v_sets) ? 1 : 0;
}

int vface_groupnorm_partial_floats(int nimg, int hw, int C, int groups) {
    if (nimg <= 0 || hw <= 0 || groups <= 0) return VFACE_ERR_ARG;
    return vf_gn_partial_floats(nimg, hw, C, groups);
}

int64_t vface_channel_stats_partial_floats(int nimg, int hw, int C) {
    if (nimg <= 0 || hw <= 0 || C <= 0) return 0;
    return (int64_t)nimg * vf_chan_stats_slices(hw) * C * 2;
}

int vface_ffn_fused_supported(int64_t M, int C) { return vf_ffn_fused_supported((long)M, C) ? 1 : 0; }

int vface_ffn_fused(const float* x32, int64_t ldx, const float* gamma, const float* beta, float eps, const void* W1, const float* b1,
                    const void* W2p, const float* b2, void* out16, int64_t ldo, float* out32, int64_t ldo32, int M, int C,
                    int dtype, void* stream) {
    FfnParams p{};
    p.x32 = x32; p.ldx = ldx; p.gamma = gamma; p.beta = beta; p.eps = eps; p.W1 = W1; p.b1 = b1; p.W2p = W2p; p.b2 = b2;
    p.out16 = out16; p.ldo = ldo; p.out32 = out32; p.ldo32 = ldo32; p.M = M; p.C = C;
    return vf_launch_ffn_fused(p, dtype, vf_stream(stream));
}

int vface_attn_out_ffn_fused(const void* att, int64_t ldatt, const float* resid, int64_t ldr, const float* rowbias, int64_t ld_rowbias,
                             int rows_per_sample, const void* WoW1, const float* bo, const float* gamma, const float* beta, float eps,
                             const float* b1, const void* W2p, const float* b2, void* out16, int64_t ldo, float* out32,
                             int64_t ldo32, int M, int C, int dtype, void* stream) {
    if (!att) return VFACE_ERR_ARG;
    FfnParams p{};
    p.att = att; p.ldatt = ldatt; p.resid = resid; p.ldr = ldr; p.rowbias = rowbias; p.ld_rowbias = ld_rowbias;
    p.rows_per_sample = rows_per_sample; p.bo = bo; p.gamma = gamma; p.beta = beta; p.eps = eps; p.W1 = WoW1; p.b1 = b1; p.W2p = W2p;
    p.b2 = b2; p.out16 = out16; p.ldo = ldo; p.out32 = out32; p.ldo32 = ldo32; p.M = M; p.C = C;
    return vf_launch_ffn_fused(p, dtype, vf_stream(stream));
}

int vface_attn_out_ffn_proj_fused(const void* att, int64_t ldatt, const float* resid, int64_t ldr, const float* rowbias, int64_t ld_rowbias,
                                  int rows_per_sample, const void* WoW1Wp, const float* bo, const float* gamma, const float* beta, float eps,
                                  const float* b1, const void* W2p, const float* b2, const float* b_po, const float* x_in, int64_t ld_xin,
                                  void* out16, int64_t ldo, float* out32, int64_t ldo32, float* colstats, int64_t ld_colstats, int M, int C,
                                  int dtype, void* stream) {
    if (!att || !x_in || !b_po) return VFACE_ERR_ARG;
    FfnParams p{};
    p.att = att; p.ldatt = ldatt; p.resid = resid; p.ldr = ldr; p.rowbias = rowbias; p.ld_rowbias = ld_rowbias;
    p.rows_per_sample = rows_per_sample; p.bo = bo; p.gamma = gamma; p.beta = beta; p.eps = eps; p.W1 = WoW1Wp; p.b1 = b1; p.W2p = W2p;
    p.b2 = b2; p.out16 = out16; p.ldo = ldo; p.out32 = out32; p.ldo32 = ldo32; p.M = M; p.C = C;
    p.Wpo_in_stream = 1; p.b_po = b_po; p.x_in = x_in; p.ld_xin = ld_xin; p.colstats = colstats; p.ld_colstats = ld_colstats;
    return vf_launch_ffn_fused(p, dtype, vf_stream(stream));
}

int vface_gn_silu_conv3x3_small(const void* x, int64_t ldx, int in_f32, const float* gn_ab, int64_t ld_ab, const void* Wt, const float* bias,
                                float* out, int64_t ldo, int nimg, int H, int W, int Cin, int Cout, int dtype, void* stream) {
    OutConvParams p{};
    p.x = x; p.ldx = ldx; p.in_f32 = in_f32; p.ab = gn_ab; p.ld_ab = ld_ab; p.Wt = Wt; p.bias = bias; p.out = out; p.ldo = ldo;
    p.nimg = nimg; p.H = H; p.W = W; p.Cin = Cin; p.Cout = Cout;
    return vf_launch_out_conv(p, dtype, vf_stream(stream));
}

int vface_linear_small_supported(int M, int N, int K) { return vf_linear_small_supported(M, N, K) ? 1 : 0; }

int vface_linear_small(const void* a, int64_t lda, const void* W, int64_t ldw, const float* bias, void* out,
                       int64_t ldo, int out_f32, int silu, int M, int N, int K, int dtype, void* stream) {
    LinearSmallParams p{};
    p.a = a; p.lda = lda; p.W = W; p.ldw = ldw; p.bias = bias; p.out = out;
    p.ldo = ldo; p.out_f32 = out_f32; p.silu = silu; p.M = M; p.N = N; p.K = K;
    return vf_launch_linear_small(p, dtype, vf_stream(stream));
}

int vface_st_front_supported(int64_t M, int C, int hw) { return vf_st_front_supported((long)M, C, hw) ? 1 : 0; }

int vface_st_front(const float* x32, int64_t ldx, const float* gn_ab, int64_t ld_ab, int hw, const void* Wcat, const float* b_in,
                   const float* gamma, const float* beta, float eps, float* t0, int64_t ldt0, void* qkv, int64_t ldq, void* ln,
                   int64_t ldln, int M, int C, int NQ, int rows_full, int nq_lo, int dtype, void* stream) {
    StFrontParams p{};
    p.x32 = x32; p.ldx = ldx; p.ab = gn_ab; p.ld_ab = ld_ab; p.hw = hw; p.Wcat = Wcat; p.b_in = b_in; p.gamma = gamma; p.beta = beta;
    p.eps = eps; p.t0 = t0; p.ldt0 = ldt0; p.qkv = qkv; p.ldq = ldq; p.ln = ln; p.ldln = ldln; p.M = M; p.C = C; p.NQ = NQ;
    p.rows_full = rows_full; p.nq_lo = nq_lo;
    return vf_launch_st_front(p, dtype, vf_stream(stream));
}

size_t vface_adain_workspace_bytes(int64_t rows, int C) { return rows > 0 && C > 0 ? vf_adain_workspace_bytes(rows, C) : 0; }
int vface_adain_fusion(const void* a, int64_t lda, const void* b, int64_t ldb, void* dst, int64_t ldd, int64_t rows, int C,
                       void* workspace, size_t workspace_bytes, int dtype, void* stream) {
    if (rows > 0 && C > 0 && workspace_bytes < vf_adain_workspace_bytes(rows, C)) return VFACE_ERR_WORKSPACE;
    return vf_launch_adain(a, lda, b, ldb, dst, ldd, rows, C, workspace, dtype, vf_stream(stream));
}
size_t vface_adain_rows_workspace_bytes(int64_t rows, int C) {
    return rows > 0 && C > 0 ? vf_adain_rows_workspace_bytes(rows, C) : 0;
}
int vface_adain_rows(const void* a, int64_t lda, const void* b, int64_t ldb, int64_t rows, int C, double* partial, void* workspace,
                     size_t workspace_bytes, int dtype, void* stream) {
    if (rows > 0 && C > 0 && workspace_bytes < vf_adain_rows_workspace_bytes(rows, C)) return VFACE_ERR_WORKSPACE;
    return vf_launch_adain_rows(a, lda, b, ldb, rows, C, partial, workspace, dtype, vf_stream(stream));
}
int vface_adain_reduce_scale(const double* partial, int64_t partial_rows, int C, void* workspace, size_t workspace_bytes, void* dst,
                             int64_t ldd, int64_t rows, int dtype, void* stream) {
    if (rows > 0 && C > 0 && workspace_bytes < vf_adain_rows_workspace_bytes(rows, C)) return VFACE_ERR_WORKSPACE;
    return vf_launch_adain_reduce_scale(partial, partial_rows, C, workspace, dst, ldd, rows, dtype, vf_stream(stream));
}

int vface_timestep_embedding(const int64_t* t, void* out, int N, int dim, int dtype, void* stream) {
    return vf_launch_timestep_embedding(reinterpret_cast<const long long*>(t), out, N, dim, dtype, vf_stream(stream));
}

}  // extern "C"
