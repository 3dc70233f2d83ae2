// Glue kernels of the conditioning path: the CLIP ViT image embedder with its mapper (REFace/ldm/modules/encoders/modules.py:211-264,
// encoders/xf.py) and the feature mix of `conditioning_with_feat` (REFace/ldm/models/diffusion/ddpm.py:872-1045).  The projections
// run on vface_gemm, the attention on vface_attention (dh = 64), the LayerNorms on vface_layernorm and the residual adds on the
// fp32 residual stream of the GEMM; what is here is the rest:
//
//   clip_patches_kernel   the image as the patch matrix of the 14 x 14 stride-14 convolution (HF CLIPVisionEmbeddings.patch_embedding):
//                         row (b, py, px), column c * 196 + ky * 14 + kx -- the flattening of the weight [hidden][3][14][14] -- zero
//                         from column 588 to 639, so the patch embedding is one vface_gemm with K = 640.  Either a pass-through of an
//                         already normalised image, or the whole of ddpm.py:907-912: `tar * 1.0`, un_norm, TF.normalize with CLIP's
//                         mean / std, TF.resize to the patch grid's size (bilinear, align_corners false, no antialias), with the
//                         `(1 - inpaint_mask)` factor of scripts/VFace_inference_batch.py:493 in front when a mask is given.  fp32
//                         throughout, one rounding to the storage type.
//   clip_embed_kernel     CLIPVisionEmbeddings.forward: the class-token row in front of each sample's patch rows, plus the position
//                         table, and `pre_layrnorm` on the sum -> the fp32 residual stream (which so starts unrounded)
//   act_kernel            quick_gelu (the ViT's MLP) / erf-GELU (xf.py MLP of the mapper) on a 16-bit matrix view, fp32 inside
//   cond_mix_kernel       ddpm.py:1038-1039: (c w_c + c2 w_id + lm w_lm) / (w_c + w_id + w_lm) on [B, N] fp32 rows, each operand
//                         either per sample or one row for all
//
// HBM-bound byte movers, one thread per 8 (16-bit) or 4 (fp32) columns (the embedding: one wave per row).  No atomics, every sum
// in a fixed order: a sample's bits do not depend on the batch it is in.  Contraction is OFF where the reference rounds every product (ATen's interpolation and the mix).
#include "common.hpp"
#include "launch.hpp"
#include "vface_kernels.hpp"

namespace {

constexpr int PATCH = 14, PATCH_K = 3 * PATCH * PATCH, PATCH_KP = 640;      // 588 columns, padded to a multiple of 64

// img [B][3][H][W] fp32, mask [B][H][W] fp32 or NULL -> out [B * G * G][ldo], columns 0 .. 639.  PREP = false: H == W == 14 G.
template <class TT, bool PREP>
__global__ __launch_bounds__(256) void clip_patches_kernel(const float* __restrict__ img, int H, int W, const float* __restrict__ mask,
                                                           typename TT::elem* __restrict__ out, long ldo, int G, long total,
                                                           int* __restrict__ dbg_x0, int* __restrict__ dbg_y0) {
#pragma clang fp contract(off)
    using E = typename TT::elem;
    using V8 = typename TT::v8;
    const float mean[3] = {0.48145466f, 0.4578275f, 0.40821073f}, sd[3] = {0.26862954f, 0.26130258f, 0.27577711f};
    const int S = PATCH * G;
    // ATen's area_pixel_compute_scale without align_corners: in / out in fp32
    const float sy = (float)H / (float)S, sx = (float)W / (float)S;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const long m = i / (PATCH_KP / 8);
        const int k0 = (int)(i - m * (PATCH_KP / 8)) * 8;
        const int px = (int)(m % G), py = (int)((m / G) % G);
        const long b = m / ((long)G * G);
        V8 o;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int k = k0 + e;
            float v = 0.0f;
            if (k < PATCH_K) {
                const int c = k / (PATCH * PATCH), r = k - c * (PATCH * PATCH);
                const int ky = r / PATCH, kx = r - ky * PATCH;
                const int oy = py * PATCH + ky, ox = px * PATCH + kx;
                const float* plane = img + (b * 3 + c) * (long)H * W;
                if constexpr (!PREP) {
                    v = plane[(long)oy * W + ox];
                } else {
                    const float fy = fmaxf(sy * ((float)oy + 0.5f) - 0.5f, 0.0f), fx = fmaxf(sx * ((float)ox + 0.5f) - 0.5f, 0.0f);
                    const int y0 = min((int)fy, H - 1), x0 = min((int)fx, W - 1);
                    const int y1 = min(y0 + 1, H - 1), x1 = min(x0 + 1, W - 1);
                    const float ly1 = fy - (float)y0, lx1 = fx - (float)x0;
                    const float ly0 = 1.0f - ly1, lx0 = 1.0f - lx1;
                    const float* mk = mask ? mask + b * (long)H * W : nullptr;
                    auto tap = [&](int yy, int xx) {
                        float x = plane[(long)yy * W + xx];
                        if (mk) x = x * (1.0f - mk[(long)yy * W + xx]);
                        return ((x + 1.0f) / 2.0f - mean[c]) / sd[c];
                    };
                    const float top = lx0 * tap(y0, x0) + lx1 * tap(y0, x1);
                    const float bot = lx0 * tap(y1, x0) + lx1 * tap(y1, x1);
                    v = ly0 * top + ly1 * bot;
                    if (b == 0 && c == 0) {
                        if (dbg_x0 && oy == 0) dbg_x0[ox] = x0;
                        if (dbg_y0 && ox == 0) dbg_y0[oy] = y0;
                    }
                }
            }
            o[e] = from_f32<E>(v);
        }
        *reinterpret_cast<V8*>(out + m * ldo + k0) = o;
    }
}

// tok [B * P][ldt] (fp32 or 16-bit), cls [C], pos [P + 1][C] fp32 -> x32 [B * (P + 1)][ldo]: row b (P + 1) = cls + pos[0],
// row b (P + 1) + 1 + p = tok[b P + p] + pos[1 + p]; with gamma / beta the row's LayerNorm (`pre_layrnorm`) instead of the row.
// One wave per row, lane l on columns 4 l + 256 j; the statistics in two passes over the re-formed row (mean, then the centred
// squares), each a per-lane sum in column order and wave_sum's butterfly: the same order whatever the batch.
template <class T>
__global__ __launch_bounds__(256) void clip_embed_kernel(const T* __restrict__ tok, long ldt, const float* __restrict__ cls,
                                                         const float* __restrict__ pos, const float* __restrict__ gamma,
                                                         const float* __restrict__ beta, float eps, float* __restrict__ x32, long ldo,
                                                         int P, int C, long rows) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x & 63;
    const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;                                     // (whole waves leave: no barrier below)
    const long b = row / (P + 1);
    const int t = (int)(row - b * (P + 1));
    const T* src = t ? tok + (b * P + (t - 1)) * ldt : nullptr;
    auto load = [&](int c0) {
        float4 v;
        if (src) v = float4{to_f32(src[c0]), to_f32(src[c0 + 1]), to_f32(src[c0 + 2]), to_f32(src[c0 + 3])};
        else v = *reinterpret_cast<const float4*>(cls + c0);
        const float4 p = *reinterpret_cast<const float4*>(pos + (long)t * C + c0);
        return float4{v.x + p.x, v.y + p.y, v.z + p.z, v.w + p.w};
    };
    float* dst = x32 + row * ldo;
    if (!gamma) {
        for (int c0 = lane * 4; c0 < C; c0 += 256) *reinterpret_cast<float4*>(dst + c0) = load(c0);
        return;
    }
    float s = 0.0f;
    for (int c0 = lane * 4; c0 < C; c0 += 256) {
        const float4 v = load(c0);
        s = s + v.x; s = s + v.y; s = s + v.z; s = s + v.w;
    }
    const float mean = wave_sum(s) / (float)C;
    float q = 0.0f;
    for (int c0 = lane * 4; c0 < C; c0 += 256) {
        const float4 v = load(c0);
        const float d0 = v.x - mean, d1 = v.y - mean, d2 = v.z - mean, d3 = v.w - mean;
        q = q + d0 * d0; q = q + d1 * d1; q = q + d2 * d2; q = q + d3 * d3;
    }
    const float rstd = 1.0f / sqrtf(wave_sum(q) / (float)C + eps);
    for (int c0 = lane * 4; c0 < C; c0 += 256) {
        const float4 v = load(c0);
        const float4 g = *reinterpret_cast<const float4*>(gamma + c0), bt = *reinterpret_cast<const float4*>(beta + c0);
        *reinterpret_cast<float4*>(dst + c0) = float4{(v.x - mean) * rstd * g.x + bt.x, (v.y - mean) * rstd * g.y + bt.y,
                                                      (v.z - mean) * rstd * g.z + bt.z, (v.w - mean) * rstd * g.w + bt.w};
    }
}

// y[r][c] = act(x[r][c]); kind 0: quick_gelu v sigmoid(1.702 v) = v / (1 + exp(-1.702 v)); 1: erf-GELU (gelu_erf_f).  y may be x.
template <class TT, int KIND>
__global__ __launch_bounds__(256) void act_kernel(const typename TT::elem* x, long ldx, typename TT::elem* y, long ldy, long rows,
                                                  int cols) {
    using E = typename TT::elem;
    using V8 = typename TT::v8;
    const int c8 = cols / 8;
    const long total = rows * c8;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const long r = i / c8;
        const int c0 = (int)(i - r * c8) * 8;
        const V8 v = *reinterpret_cast<const V8*>(x + r * ldx + c0);
        V8 o;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float f = to_f32(v[j]);
            o[j] = from_f32<E>(KIND == 0 ? f / (1.0f + __expf(-1.702f * f)) : gelu_erf_f(f));
        }
        *reinterpret_cast<V8*>(y + r * ldy + c0) = o;
    }
}

struct MixOperand { const float* p; long ld; float w; };     // ld = 0: one row for every sample; p = NULL: absent

// out[b][n] = (a w_a + b w_b + c w_c) / wsum, the sum in the reference's order (left to right), absent operands left out
template <class TT>
__global__ __launch_bounds__(256) void cond_mix_kernel(MixOperand a, MixOperand b, MixOperand c, float wsum, float* __restrict__ out32,
                                                       long ldo32, typename TT::elem* __restrict__ out16, long ldo16, int N, long total) {
#pragma clang fp contract(off)
    using E = typename TT::elem;
    using V4 = typename TT::v4;
    const int n4 = N / 4;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const long r = i / n4;
        const int c0 = (int)(i - r * n4) * 4;
        float s[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        bool first = true;
        const MixOperand ops[3] = {a, b, c};
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            if (!ops[k].p) continue;
            const float4 v = *reinterpret_cast<const float4*>(ops[k].p + r * ops[k].ld + c0);
            const float t[4] = {v.x * ops[k].w, v.y * ops[k].w, v.z * ops[k].w, v.w * ops[k].w};
#pragma unroll
            for (int j = 0; j < 4; ++j) s[j] = first ? t[j] : s[j] + t[j];
            first = false;
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) s[j] = s[j] / wsum;
        if (out32) *reinterpret_cast<float4*>(out32 + r * ldo32 + c0) = float4{s[0], s[1], s[2], s[3]};
        if (out16) {
            V4 o;
#pragma unroll
            for (int j = 0; j < 4; ++j) o[j] = from_f32<E>(s[j]);
            *reinterpret_cast<V4*>(out16 + r * ldo16 + c0) = o;
        }
    }
}

}  // namespace

extern "C" int vface_clip_patches(const float* img, int H, int W, const float* mask, int prep, void* out, int64_t ldo, int B, int G,
                                  int32_t* dbg_x0, int32_t* dbg_y0, int dtype, void* stream_) {
    hipStream_t stream = vf_stream(stream_);
    if (!img || !out || B <= 0 || G <= 0 || H <= 0 || W <= 0) return VF_ERR_ARG;
    if (!prep && (mask || dbg_x0 || dbg_y0)) return VF_ERR_ARG;
    if (G > 64 || ldo < PATCH_KP || (!prep && (H != PATCH * G || W != PATCH * G))) return VF_ERR_SHAPE;
    if ((long)H * W > 0x7fffffffL / 4) return VF_ERR_SHAPE;
    if ((ldo & 7) || ((uintptr_t)out & 15) || ((uintptr_t)img & 3) || ((uintptr_t)mask & 3)) return VF_ERR_ALIGN;
    const long total = (long)B * G * G * (PATCH_KP / 8);
    DISPATCH_DTYPE(dtype, {
        using E = typename TT::elem;
        if (prep)
            hipLaunchKernelGGL((clip_patches_kernel<TT, true>), dim3(vf_grid(total, 256, 16384)), dim3(256), 0, stream, img, H, W, mask, (E*)out, ldo, G,
                               total, dbg_x0, dbg_y0);
        else
            hipLaunchKernelGGL((clip_patches_kernel<TT, false>), dim3(vf_grid(total, 256, 16384)), dim3(256), 0, stream, img, H, W, mask, (E*)out, ldo, G,
                               total, dbg_x0, dbg_y0);
    });
    return vf_launched();
}

extern "C" int vface_clip_embed(const void* tok, int64_t ldt, int tok_f32, const float* cls, const float* pos, const float* gamma,
                                const float* beta, float eps, float* x32, int64_t ldo, int B, int P, int C, int dtype, void* stream_) {
    hipStream_t stream = vf_stream(stream_);
    if (!tok || !cls || !pos || !x32 || B <= 0 || P <= 0 || C <= 0 || ((gamma != nullptr) != (beta != nullptr))) return VF_ERR_ARG;
    if (ldt < C || ldo < C) return VF_ERR_SHAPE;
    if ((C & 7) || (ldt & 7) || (ldo & 3)) return VF_ERR_ALIGN;
    if (((uintptr_t)tok | (uintptr_t)cls | (uintptr_t)pos | (uintptr_t)x32 | (uintptr_t)gamma | (uintptr_t)beta) & 15) return VF_ERR_ALIGN;
    const long rows = (long)B * (P + 1);
    const dim3 grid((unsigned)((rows + 3) / 4));
    if (tok_f32) {
        hipLaunchKernelGGL((clip_embed_kernel<float>), grid, dim3(256), 0, stream, (const float*)tok, ldt, cls, pos, gamma, beta, eps, x32, ldo,
                           P, C, rows);
        return vf_launched();
    }
    DISPATCH_DTYPE(dtype, {
        using E = typename TT::elem;
        hipLaunchKernelGGL((clip_embed_kernel<E>), grid, dim3(256), 0, stream, (const E*)tok, ldt, cls, pos, gamma, beta, eps, x32, ldo, P, C,
                           rows);
    });
    return vf_launched();
}

extern "C" int vface_act(const void* x, int64_t ldx, void* y, int64_t ldy, int64_t rows, int cols, int kind, int dtype, void* stream_) {
    hipStream_t stream = vf_stream(stream_);
    if (!x || !y || rows <= 0 || cols <= 0) return VF_ERR_ARG;
    if (kind != 0 && kind != 1) return VF_ERR_ARG;
    if (ldx < cols || ldy < cols) return VF_ERR_SHAPE;
    if ((cols & 7) || (ldx & 7) || (ldy & 7) || (((uintptr_t)x | (uintptr_t)y) & 15)) return VF_ERR_ALIGN;
    const long total = rows * (cols / 8);
    DISPATCH_DTYPE(dtype, {
        using E = typename TT::elem;
        if (kind == 0) hipLaunchKernelGGL((act_kernel<TT, 0>), dim3(vf_grid(total, 256, 16384)), dim3(256), 0, stream, (const E*)x, ldx, (E*)y, ldy, rows, cols);
        else hipLaunchKernelGGL((act_kernel<TT, 1>), dim3(vf_grid(total, 256, 16384)), dim3(256), 0, stream, (const E*)x, ldx, (E*)y, ldy, rows, cols);
    });
    return vf_launched();
}

extern "C" int vface_cond_mix(const float* a, int rows_a, float wa, const float* b, int rows_b, float wb, const float* c, int rows_c,
                              float wc, float wsum, float* out32, int64_t ldo32, void* out16, int64_t ldo16, int B, int N, int dtype,
                              void* stream_) {
    hipStream_t stream = vf_stream(stream_);
    if (B <= 0 || N <= 0 || (!out32 && !out16) || (!a && !b && !c)) return VF_ERR_ARG;
    if (!(wsum != 0.0f)) return VF_ERR_ARG;
    if ((a && rows_a != 1 && rows_a != B) || (b && rows_b != 1 && rows_b != B) || (c && rows_c != 1 && rows_c != B)) return VF_ERR_SHAPE;
    if ((out32 && ldo32 < N) || (out16 && ldo16 < N)) return VF_ERR_SHAPE;
    if ((N & 3) || (ldo32 & 3) || (ldo16 & 3)) return VF_ERR_ALIGN;
    if (((uintptr_t)a | (uintptr_t)b | (uintptr_t)c | (uintptr_t)out32) & 15) return VF_ERR_ALIGN;
    if ((uintptr_t)out16 & 7) return VF_ERR_ALIGN;
    // operands are contiguous [rows][N]: a broadcast operand has row stride 0
    const MixOperand oa{a, rows_a == 1 ? 0 : (long)N, wa}, ob{b, rows_b == 1 ? 0 : (long)N, wb}, oc{c, rows_c == 1 ? 0 : (long)N, wc};
    const long total = (long)B * (N / 4);
    DISPATCH_DTYPE(dtype, {
        using E = typename TT::elem;
        hipLaunchKernelGGL((cond_mix_kernel<TT>), dim3(vf_grid(total, 256, 16384)), dim3(256), 0, stream, oa, ob, oc, wsum, out32, ldo32, (E*)out16, ldo16, N,
                           total);
    });
    return vf_launched();
}
