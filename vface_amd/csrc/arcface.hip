// Glue kernels of the identity network: ArcFace IR-SE50 behind `IDLoss.extract_feats` (REFace/ldm/models/diffusion/ddpm.py:91-124,
// REFace/src/Face_models/encoders/{model_irse,helpers}.py).  Its convolutions run on vface_conv3x3 / vface_im2col + vface_gemm with
// the foldable BatchNorms folded on the host, its global average pools are vface_channel_stats and the squeeze-excite 1x1s
// vface_pooled_linear (vface_amd/arcface.py); what is here is the work only this network has, on token-major (NHWC) buffers:
//
//   id_prep_kernel       extract_feats up to the network (ddpm.py:114-119): un_norm_clip, (x - 0.5) / 0.5, AdaptiveAvgPool2d(256)
//                        unless the height is 256 already, the crop [35:223, 32:220], AdaptiveAvgPool2d(112) -> 8 channels per
//                        pixel (3 used, 5 zero), the rows the stem reads.  The two means are nested as the reference nests them:
//                        every element of the 256 map is a mean of its own bin, and the 112 map averages those.  With `prep` the
//                        224 x 224 CLIP image is formed from a [-1, 1] frame first, by clip_patches_kernel's expressions.
//   prelu_kernel         y = x > 0 ? x : slope[c] x, and optionally z = a[c] y32 + b[c] from the unrounded y
//   se_gate_add_kernel   y = res * g[img][c] + shortcut (helpers.py:65-72, 116-119); the shortcut is a same-sized tensor or the
//                        unit's input subsampled (MaxPool2d(1, stride)); optionally z = a[c] y32 + b[c]: the next unit's leading
//                        BatchNorm2d, which sits in front of a zero-padded convolution and so cannot be folded into it
//   l2norm_rows_kernel   x / ||x||_2 per fp32 row (helpers.py:15-18)
//
// HBM-bound byte movers: 16-byte accesses along the channel axis, one thread per 8 channels (the prep: per output pixel; the norm:
// one wave per row).  No atomics, every sum in a fixed order: a sample's bits do not depend on the batch it is in.
#include "common.hpp"
#include "launch.hpp"
#include "vface_kernels.hpp"

namespace {

constexpr int ID_POOL = 256, ID_Y0 = 35, ID_X0 = 32, ID_CROP = 188, ID_OUT = 112, CLIP_SIZE = 224;

// PyTorch's adaptive pooling bins: floor(i In / Out) .. ceil((i + 1) In / Out)
__device__ __forceinline__ int bin_lo(int i, int in, int out) { return (int)(((long)i * in) / out); }
__device__ __forceinline__ int bin_hi(int i, int in, int out) { return (int)(((long)(i + 1) * in + out - 1) / out); }

// img [B][3][H][W] fp32 (mask [B][H][W] fp32 or NULL, PREP only) -> out [B * 112 * 112][ldo], columns 0 .. 7.
// SH x SW is the size of the image the chain of extract_feats sees: H x W itself, or 224 x 224 with PREP.
template <class TT, bool PREP>
__global__ __launch_bounds__(256) void id_prep_kernel(const float* __restrict__ img, int H, int W, const float* __restrict__ mask,
                                                      int clip_img, typename TT::elem* __restrict__ out, long ldo, long total) {
#pragma clang fp contract(off)
    using E = typename TT::elem;
    using V8 = typename TT::v8;
    const float mean[3] = {0.48145466f, 0.4578275f, 0.40821073f}, sd[3] = {0.26862954f, 0.26130258f, 0.27577711f};
    const int SH = PREP ? CLIP_SIZE : H, SW = PREP ? CLIP_SIZE : W;
    const bool pool1 = SH != ID_POOL;                            // the reference's own condition: `x.shape[2] != 256`
    // ATen's area_pixel_compute_scale without align_corners: in / out in fp32 (PREP only)
    const float sy = (float)H / (float)CLIP_SIZE, sx = (float)W / (float)CLIP_SIZE;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const int ox = (int)(i % ID_OUT), oy = (int)((i / ID_OUT) % ID_OUT);
        const long b = i / ((long)ID_OUT * ID_OUT);
        const float* mk = (PREP && mask) ? mask + b * (long)H * W : nullptr;
        V8 o;
#pragma unroll
        for (int c = 0; c < 8; ++c) o[c] = from_f32<E>(0.0f);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float* plane = img + (b * 3 + c) * (long)H * W;
            // the image extract_feats pools, at (yy, xx) of SH x SW
            auto src = [&](int yy, int xx) {
                float v;
                if constexpr (!PREP) {
                    v = plane[(long)yy * W + xx];
                } else {                                         // clip_patches_kernel<PREP>, expression for expression
                    const float fy = fmaxf(sy * ((float)yy + 0.5f) - 0.5f, 0.0f), fx = fmaxf(sx * ((float)xx + 0.5f) - 0.5f, 0.0f);
                    const int y0 = min((int)fy, H - 1), x0 = min((int)fx, W - 1);
                    const int y1 = min(y0 + 1, H - 1), x1 = min(x0 + 1, W - 1);
                    const float ly1 = fy - (float)y0, lx1 = fx - (float)x0;
                    const float ly0 = 1.0f - ly1, lx0 = 1.0f - lx1;
                    auto tap = [&](int ty, int tx) {
                        float x = plane[(long)ty * W + tx];
                        if (mk) x = x * (1.0f - mk[(long)ty * W + tx]);
                        return ((x + 1.0f) / 2.0f - mean[c]) / sd[c];
                    };
                    const float top = lx0 * tap(y0, x0) + lx1 * tap(y0, x1);
                    const float bot = lx0 * tap(y1, x0) + lx1 * tap(y1, x1);
                    v = ly0 * top + ly1 * bot;
                }
                if (clip_img) v = ((v * sd[c] + mean[c]) - 0.5f) / 0.5f;      // un_norm_clip, then TF.normalize(0.5, 0.5)
                return v;
            };
            // element (py, px) of the 256 x 256 map: its own bin's mean, or the image itself
            auto pooled = [&](int py, int px) {
                if (!pool1) return src(py, px);
                const int ya = bin_lo(py, SH, ID_POOL), yb = bin_hi(py, SH, ID_POOL);
                const int xa = bin_lo(px, SW, ID_POOL), xb = bin_hi(px, SW, ID_POOL);
                float s = 0.0f;
                for (int yy = ya; yy < yb; ++yy)
                    for (int xx = xa; xx < xb; ++xx) s = s + src(yy, xx);
                return s / (float)((yb - ya) * (xb - xa));
            };
            const int ya = bin_lo(oy, ID_CROP, ID_OUT), yb = bin_hi(oy, ID_CROP, ID_OUT);
            const int xa = bin_lo(ox, ID_CROP, ID_OUT), xb = bin_hi(ox, ID_CROP, ID_OUT);
            float s = 0.0f;
            for (int yy = ya; yy < yb; ++yy)
                for (int xx = xa; xx < xb; ++xx) s = s + pooled(ID_Y0 + yy, ID_X0 + xx);
            o[c] = from_f32<E>(s / (float)((yb - ya) * (xb - xa)));
        }
        *reinterpret_cast<V8*>(out + i * ldo) = o;
    }
}

__device__ __forceinline__ void load8(const float* p, float (&v)[8]) {
    const float4 a = *reinterpret_cast<const float4*>(p), b = *reinterpret_cast<const float4*>(p + 4);
    v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
}

// y[m][c] = x > 0 ? x : slope[c] x; z[m][c] = za[c] y32 + zb[c] (z NULL: not written).  y may be x: a thread reads its 8 values
// before it writes them, so no __restrict__ on either.
template <class TT>
__global__ __launch_bounds__(256) void prelu_kernel(const typename TT::elem* x, long ldx, const float* __restrict__ slope,
                                                    typename TT::elem* y, long ldy, const float* __restrict__ za,
                                                    const float* __restrict__ zb, typename TT::elem* __restrict__ z, long ldz, long M,
                                                    int C) {
    using E = typename TT::elem;
    using V8 = typename TT::v8;
    const int c8 = C / 8;
    const long total = M * c8;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const long m = i / c8;
        const int c0 = (int)(i - m * c8) * 8;
        const V8 v = *reinterpret_cast<const V8*>(x + m * ldx + c0);
        float sl[8], f[8];
        load8(slope + c0, sl);
        V8 o;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float t = to_f32(v[j]);
            f[j] = t > 0.0f ? t : sl[j] * t;
            o[j] = from_f32<E>(f[j]);
        }
        *reinterpret_cast<V8*>(y + m * ldy + c0) = o;
        if (z) {
            float a[8], bb[8];
            load8(za + c0, a);
            load8(zb + c0, bb);
            V8 q;
#pragma unroll
            for (int j = 0; j < 8; ++j) q[j] = from_f32<E>(fmaf(a[j], f[j], bb[j]));
            *reinterpret_cast<V8*>(z + m * ldz + c0) = q;
        }
    }
}

// y[m][c] = res[m][c] g[m / (OH OW)][c] + sc, m = (n, oy, ox) of the OH x OW output.  s == 0: sc = row m of a same-sized tensor;
// s >= 1: sc = pixel (n, oy s, ox s) of the H x W input of the unit.  z as in prelu_kernel.  y may be res.
template <class TT>
__global__ __launch_bounds__(256) void se_gate_add_kernel(const typename TT::elem* res, long ldr, const float* __restrict__ g, long ldg,
                                                          const typename TT::elem* __restrict__ sc, long lds, int s, int H, int W,
                                                          int OH, int OW, typename TT::elem* y, long ldy,
                                                          const float* __restrict__ za, const float* __restrict__ zb,
                                                          typename TT::elem* __restrict__ z, long ldz, long M, int C) {
    using E = typename TT::elem;
    using V8 = typename TT::v8;
    const int c8 = C / 8;
    const long total = M * c8;
    const long ohw = (long)OH * OW;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const long m = i / c8;
        const int c0 = (int)(i - m * c8) * 8;
        const long n = m / ohw;
        long row = m;
        if (s) {
            const long p = m - n * ohw;
            const int oy = (int)(p / OW), ox = (int)(p - (long)oy * OW);
            row = (n * H + (long)oy * s) * W + (long)ox * s;      // oy s <= H - 1 by OH = (H - 1) / s + 1
        }
        const V8 r = *reinterpret_cast<const V8*>(res + m * ldr + c0);
        const V8 t = *reinterpret_cast<const V8*>(sc + row * lds + c0);
        float gg[8], f[8];
        load8(g + n * ldg + c0, gg);
        V8 o;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            f[j] = fmaf(to_f32(r[j]), gg[j], to_f32(t[j]));
            o[j] = from_f32<E>(f[j]);
        }
        *reinterpret_cast<V8*>(y + m * ldy + c0) = o;
        if (z) {
            float a[8], bb[8];
            load8(za + c0, a);
            load8(zb + c0, bb);
            V8 q;
#pragma unroll
            for (int j = 0; j < 8; ++j) q[j] = from_f32<E>(fmaf(a[j], f[j], bb[j]));
            *reinterpret_cast<V8*>(z + m * ldz + c0) = q;
        }
    }
}

// out[r][:] = x[r][:] / ||x[r]||_2.  One wave per row, lane l on columns 4 l + 256 j: the row's largest magnitude first (so the
// squares neither overflow nor vanish), then the sum of (x / max)^2 per lane in column order and wave_sum's butterfly -- the same
// order whatever the batch.  A zero row gives 0 / 0, as the reference does.
__global__ __launch_bounds__(256) void l2norm_rows_kernel(const float* __restrict__ x, long ldx, float* __restrict__ out, long ldo,
                                                          int B, int N) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x & 63;
    const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= B) return;                                        // (whole waves leave: no barrier below)
    const float* src = x + row * ldx;
    float mx = 0.0f;
    for (int c0 = lane * 4; c0 < N; c0 += 256) {
        const float4 v = *reinterpret_cast<const float4*>(src + c0);
        mx = fmaxf(mx, fmaxf(fmaxf(fabsf(v.x), fabsf(v.y)), fmaxf(fabsf(v.z), fabsf(v.w))));
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
    float q = 0.0f;
    for (int c0 = lane * 4; c0 < N; c0 += 256) {
        const float4 v = *reinterpret_cast<const float4*>(src + c0);
        const float a = v.x / mx, b = v.y / mx, c = v.z / mx, d = v.w / mx;
        q = q + a * a; q = q + b * b; q = q + c * c; q = q + d * d;
    }
    const float norm = mx * sqrtf(wave_sum(q));
    for (int c0 = lane * 4; c0 < N; c0 += 256) {
        const float4 v = *reinterpret_cast<const float4*>(src + c0);
        *reinterpret_cast<float4*>(out + row * ldo + c0) = float4{v.x / norm, v.y / norm, v.z / norm, v.w / norm};
    }
}

}  // namespace

extern "C" int vface_id_prep(const float* img, int H, int W, const float* mask, int prep, int clip_img, void* out, int64_t ldo, int B,
                             int dtype, void* stream_) {
    hipStream_t stream = vf_stream(stream_);
    if (!img || !out || B <= 0 || H <= 0 || W <= 0) return VF_ERR_ARG;
    if (!prep && mask) return VF_ERR_ARG;
    if (prep && !clip_img) return VF_ERR_ARG;                    // the frame becomes a CLIP-normalised image: the chain un-normalises it
    if (ldo < 8) return VF_ERR_SHAPE;
    if (!prep && H == ID_POOL && W < ID_X0 + ID_CROP) return VF_ERR_SHAPE;      // a 256-high image is cropped as it is
    if ((long)H * W > 0x7fffffffL / 4 || (long)B * ID_OUT * ID_OUT > 0x7fffffffL) return VF_ERR_SHAPE;
    if ((ldo & 7) || ((uintptr_t)out & 15) || ((uintptr_t)img & 3) || ((uintptr_t)mask & 3)) return VF_ERR_ALIGN;
    const long total = (long)B * ID_OUT * ID_OUT;
    DISPATCH_DTYPE(dtype, {
        using E = typename TT::elem;
        if (prep)
            hipLaunchKernelGGL((id_prep_kernel<TT, true>), dim3(vf_grid(total, 256, 16384)), dim3(256), 0, stream, img, H, W, mask, clip_img, (E*)out, ldo,
                               total);
        else
            hipLaunchKernelGGL((id_prep_kernel<TT, false>), dim3(vf_grid(total, 256, 16384)), dim3(256), 0, stream, img, H, W, mask, clip_img, (E*)out, ldo,
                               total);
    });
    return vf_launched();
}

extern "C" int vface_prelu(const void* x, int64_t ldx, const float* slope, void* y, int64_t ldy, const float* za, const float* zb, void* z,
                           int64_t ldz, int64_t M, int C, int dtype, void* stream_) {
    hipStream_t stream = vf_stream(stream_);
    if (!x || !slope || !y || M <= 0 || C <= 0) return VF_ERR_ARG;
    if (z && (!za || !zb || z == x || z == y)) return VF_ERR_ARG;
    if (ldx < C || ldy < C || (z && ldz < C)) return VF_ERR_SHAPE;
    if ((C & 7) || (ldx & 7) || (ldy & 7) || (z && (ldz & 7))) return VF_ERR_ALIGN;
    if (((uintptr_t)x | (uintptr_t)y | (uintptr_t)z | (uintptr_t)slope | (uintptr_t)(z ? za : nullptr) | (uintptr_t)(z ? zb : nullptr)) & 15)
        return VF_ERR_ALIGN;
    DISPATCH_DTYPE(dtype, {
        using E = typename TT::elem;
        hipLaunchKernelGGL((prelu_kernel<TT>), dim3(vf_grid(M * (C / 8), 256, 16384)), dim3(256), 0, stream, (const E*)x, ldx, slope, (E*)y, ldy, za, zb,
                           (E*)z, ldz, M, C);
    });
    return vf_launched();
}

extern "C" int vface_se_gate_add(const void* res, int64_t ldr, const float* g, int64_t ldg, const void* sc, int64_t lds, int sc_stride,
                                 int nimg, int H, int W, int C, void* y, int64_t ldy, const float* za, const float* zb, void* z,
                                 int64_t ldz, int dtype, void* stream_) {
    hipStream_t stream = vf_stream(stream_);
    if (!res || !g || !sc || !y || nimg <= 0 || H <= 0 || W <= 0 || C <= 0) return VF_ERR_ARG;
    if (z && (!za || !zb || z == res || z == y || z == sc)) return VF_ERR_ARG;
    if (sc_stride < 0 || sc_stride > 2) return VF_ERR_SHAPE;
    if (sc_stride && y == sc) return VF_ERR_ARG;                 // the strided read crosses threads: not in place in the input
    if (ldr < C || ldg < C || lds < C || ldy < C || (z && ldz < C)) return VF_ERR_SHAPE;
    if ((C & 7) || (ldr & 7) || (lds & 7) || (ldy & 7) || (ldg & 3) || (z && (ldz & 7))) return VF_ERR_ALIGN;
    if (((uintptr_t)res | (uintptr_t)sc | (uintptr_t)y | (uintptr_t)z | (uintptr_t)g | (uintptr_t)(z ? za : nullptr) |
         (uintptr_t)(z ? zb : nullptr)) & 15)
        return VF_ERR_ALIGN;
    const int s = sc_stride ? sc_stride : 1;
    const int OH = (H - 1) / s + 1, OW = (W - 1) / s + 1;
    const long M = (long)nimg * OH * OW;
    DISPATCH_DTYPE(dtype, {
        using E = typename TT::elem;
        hipLaunchKernelGGL((se_gate_add_kernel<TT>), dim3(vf_grid(M * (C / 8), 256, 16384)), dim3(256), 0, stream, (const E*)res, ldr, g, ldg,
                           (const E*)sc, lds, sc_stride, H, W, OH, OW, (E*)y, ldy, za, zb, (E*)z, ldz, M, C);
    });
    return vf_launched();
}

extern "C" int vface_l2norm_rows(const float* x, int64_t ldx, float* out, int64_t ldo, int B, int N, void* stream_) {
    hipStream_t stream = vf_stream(stream_);
    if (!x || !out || B <= 0 || N <= 0) return VF_ERR_ARG;
    if (ldx < N || ldo < N) return VF_ERR_SHAPE;
    if ((N & 3) || (ldx & 3) || (ldo & 3) || (((uintptr_t)x | (uintptr_t)out) & 15)) return VF_ERR_ALIGN;
    hipLaunchKernelGGL(l2norm_rows_kernel, dim3((unsigned)(((long)B + 3) / 4)), dim3(256), 0, stream, x, ldx, out, ldo, B, N);
    return vf_launched();
}
