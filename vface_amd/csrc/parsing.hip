// Glue kernels of the face-parsing network (BiSeNet over ResNet-18; REFace/pretrained/face_parsing/{face_parsing_demo,model,
// resnet}.py, called from scripts/VFace_inference_batch.py:251, 292-294).  Its convolutions run on the GEMM / implicit-GEMM kernels
// (gemm.hip, conv.hip) and its ReLUs on chan_norm_act_kernel (raft.hip); what is here is the work only this network has, on
// token-major (NHWC) buffers:
//
//   parse_prefilter_kernel     FaceParser.preprocess_img (face_parsing_demo.py:260-264) with BicubicDownSample(factor=2) (:124-193):
//                              u8 / 255, the 8-tap separable filter (vertical pass, then horizontal, reflect padding 3 + 3, stride 2),
//                              clamp(0, 1), (x - seg_mean) / seg_std (model.py:15-16) -> 8 channels per pixel (3 used, 5 zero), the
//                              layout the 7x7 window matrix reads.  fp32 throughout, one rounding to the storage type.
//   maxpool3x3s2_kernel        nn.MaxPool2d(3, 2, 1) (resnet.py:64): padding is -inf, not zero
//   channel_gate_kernel        y = x * g[img][c] + r: the attention gates (model.py:88, :214-215) with the add that follows them
//                              (:122 a per-image vector -- the nearest upsample of a 1x1 map is a broadcast; :127 a tensor; :215 x)
//   pooled_linear_kernel       the 1x1 convolutions on globally pooled vectors (:85-87, :118, :210-213): fp32 [nimg][K] -> [nimg][N],
//                              one wave per output, lanes over K in a fixed order; the pooled mean is read where vface_channel_stats
//                              left it (stride 2 floats)
//   upsample_argmax_u8_kernel  F.interpolate(bilinear, align_corners=True) of the logits (:258) + argmax over classes
//                              (face_parsing_demo.py:278) + a 32-entry byte table (the 12-class map of :74-122, or the identity):
//                              one byte per pixel leaves the chip, the full-resolution logit planes never exist.
//
// HBM-bound byte movers: 16-byte accesses along the channel axis, one thread per 8 channels (or per output pixel).  No atomics:
// every sum has a fixed order, so a frame's bits do not depend on the batch it is in.  Contraction is OFF where the reference
// rounds every product (ATen's interpolation; tests/parse_model.py restates the order).
#include "common.hpp"
#include "launch.hpp"
#include "vface_kernels.hpp"

namespace {

struct Taps8 { float k[8]; };

__device__ __forceinline__ int reflect(int i, int n) { return i < 0 ? -i : (i >= n ? 2 * n - 2 - i : i); }

// crops [F][H2][W2][3] u8 -> out [F * (H2/2) * (W2/2)][ldo] (8 channels written per pixel: 3 values, 5 zeros)
template <class TT>
__global__ __launch_bounds__(256) void parse_prefilter_kernel(const unsigned char* __restrict__ crops, int W2, int H2, Taps8 taps,
                                                              typename TT::elem* __restrict__ out, long ldo, long total) {
#pragma clang fp contract(off)
    using E = typename TT::elem;
    using V8 = typename TT::v8;
    const int h = H2 / 2, w = W2 / 2;
    const float mean[3] = {0.485f, 0.456f, 0.406f}, sd[3] = {0.229f, 0.224f, 0.225f};
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const int ox = (int)(i % w), oy = (int)((i / w) % h);
        const unsigned char* img = crops + (i / ((long)w * h)) * H2 * W2 * 3;
        float acc[3] = {0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int j = 0; j < 8; ++j) {                       // horizontal pass over the vertical pass's column 2 ox - 3 + j
            const int x = reflect(2 * ox - 3 + j, W2);
            float col[3] = {0.0f, 0.0f, 0.0f};
#pragma unroll
            for (int t = 0; t < 8; ++t) {
                const unsigned char* p = img + ((long)reflect(2 * oy - 3 + t, H2) * W2 + x) * 3;
#pragma unroll
                for (int c = 0; c < 3; ++c) col[c] = col[c] + taps.k[t] * ((float)p[c] / 255.0f);
            }
#pragma unroll
            for (int c = 0; c < 3; ++c) acc[c] = acc[c] + taps.k[j] * col[c];
        }
        V8 o;
#pragma unroll
        for (int c = 0; c < 8; ++c) o[c] = from_f32<E>(0.0f);
#pragma unroll
        for (int c = 0; c < 3; ++c) o[c] = from_f32<E>((fminf(fmaxf(acc[c], 0.0f), 1.0f) - mean[c]) / sd[c]);
        *reinterpret_cast<V8*>(out + i * ldo) = o;
    }
}

// x [nimg * H * W][ldx] -> y [nimg * OH * OW][ldy], window 3, stride 2, padding 1 with -inf; 8 channels per thread
template <class TT>
__global__ __launch_bounds__(256) void maxpool3x3s2_kernel(const typename TT::elem* __restrict__ x, long ldx, int H, int W, int C, int OH,
                                                           int OW, typename TT::elem* __restrict__ y, long ldy, long M) {
    using E = typename TT::elem;
    using V8 = typename TT::v8;
    const int c8 = C / 8;
    const long total = M * c8;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const long m = i / c8;
        const int c0 = (int)(i - m * c8) * 8;
        const int ox = (int)(m % OW), oy = (int)((m / OW) % OH);
        const long img = m / ((long)OW * OH);
        float best[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) best[j] = -INFINITY;
#pragma unroll
        for (int ky = 0; ky < 3; ++ky) {
            const int iy = 2 * oy - 1 + ky;
            if (iy < 0 || iy >= H) continue;
#pragma unroll
            for (int kx = 0; kx < 3; ++kx) {
                const int ix = 2 * ox - 1 + kx;
                if (ix < 0 || ix >= W) continue;
                const V8 v = *reinterpret_cast<const V8*>(x + ((img * H + iy) * W + ix) * ldx + c0);
#pragma unroll
                for (int j = 0; j < 8; ++j) best[j] = fmaxf(best[j], to_f32(v[j]));
            }
        }
        V8 o;
#pragma unroll
        for (int j = 0; j < 8; ++j) o[j] = from_f32<E>(best[j]);      // exact: the maximum is one of the inputs
        *reinterpret_cast<V8*>(y + m * ldy + c0) = o;
    }
}

// y[m][c] = x[m][c] * g[m / hw][c] + r, r = 0 | rvec[m / hw][c] (fp32) | rten[m][c] | x[m][c]; fma in fp32, one rounding to 16 bits
template <class TT>
__global__ __launch_bounds__(256) void channel_gate_kernel(const typename TT::elem* __restrict__ x, long ldx, const float* __restrict__ g,
                                                           long ldg, const float* __restrict__ rvec, long ldrv,
                                                           const typename TT::elem* __restrict__ rten, long ldr, int add_x,
                                                           typename TT::elem* __restrict__ y, long ldy, long M, int hw, int C) {
    using E = typename TT::elem;
    using V8 = typename TT::v8;
    const int c8 = C / 8;
    const long total = M * c8;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const long m = i / c8;
        const int c0 = (int)(i - m * c8) * 8;
        const long img = m / hw;
        const V8 v = *reinterpret_cast<const V8*>(x + m * ldx + c0);
        const float4 g0 = *reinterpret_cast<const float4*>(g + img * ldg + c0), g1 = *reinterpret_cast<const float4*>(g + img * ldg + c0 + 4);
        const float gg[8] = {g0.x, g0.y, g0.z, g0.w, g1.x, g1.y, g1.z, g1.w};
        float r[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) r[j] = 0.0f;
        if (rvec) {
            const float4 r0 = *reinterpret_cast<const float4*>(rvec + img * ldrv + c0), r1 = *reinterpret_cast<const float4*>(rvec + img * ldrv + c0 + 4);
            r[0] = r0.x; r[1] = r0.y; r[2] = r0.z; r[3] = r0.w; r[4] = r1.x; r[5] = r1.y; r[6] = r1.z; r[7] = r1.w;
        } else if (rten) {
            const V8 t = *reinterpret_cast<const V8*>(rten + m * ldr + c0);
#pragma unroll
            for (int j = 0; j < 8; ++j) r[j] = to_f32(t[j]);
        } else if (add_x) {
#pragma unroll
            for (int j = 0; j < 8; ++j) r[j] = to_f32(v[j]);
        }
        V8 o;
#pragma unroll
        for (int j = 0; j < 8; ++j) o[j] = from_f32<E>(fmaf(to_f32(v[j]), gg[j], r[j]));
        *reinterpret_cast<V8*>(y + m * ldy + c0) = o;
    }
}

// out[n][o] = act(sum_k W[o][k] * a[n * lda + k * sa] + bias[o]); one wave per (n, o): lane l adds k = l, l + 64, .. in order, then
// the butterfly of wave_sum -- the same order whatever the batch
__global__ __launch_bounds__(256) void pooled_linear_kernel(const float* __restrict__ a, long lda, int sa, const float* __restrict__ W,
                                                            const float* __restrict__ bias, float* __restrict__ out, long ldo, int nimg,
                                                            int N, int K, int act) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x & 63;
    const long wave = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (wave >= (long)nimg * N) return;                          // (whole waves leave: no barrier below)
    const long n = wave / N;
    const int o = (int)(wave - n * N);
    float s = 0.0f;
    for (int k = lane; k < K; k += 64) s = s + W[(long)o * K + k] * a[n * lda + (long)k * sa];
    s = wave_sum(s);
    if (lane == 0) {
        s = s + (bias ? bias[o] : 0.0f);
        if (act == 1) s = fmaxf(s, 0.0f);
        else if (act == 3) s = 1.0f / (1.0f + expf(-s));
        out[n * ldo + o] = s;
    }
}

// logits [F * h * w][ld] fp32 (columns 0 .. ncls - 1 compared) -> out [F][H][W] u8 = table[argmax_c bilinear(logits)(y, x)]
__global__ __launch_bounds__(256) void upsample_argmax_u8_kernel(const float* __restrict__ logits, long ld, int h, int w, int ncls,
                                                                 const unsigned char* __restrict__ table, unsigned char* __restrict__ out,
                                                                 int H, int W, long total) {
#pragma clang fp contract(off)
    // ATen's area_pixel_compute_scale for align_corners: (in - 1) / (out - 1) in fp32, 0 for a single output row
    const float sy = H > 1 ? (float)(h - 1) / (float)(H - 1) : 0.0f, sx = W > 1 ? (float)(w - 1) / (float)(W - 1) : 0.0f;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const int ox = (int)(i % W), oy = (int)((i / W) % H);
        const long f = i / ((long)W * H);
        const float fy = sy * (float)oy, fx = sx * (float)ox;
        const int y0 = min((int)fy, h - 1), x0 = min((int)fx, w - 1);
        const int y1 = y0 + (y0 < h - 1 ? 1 : 0), x1 = x0 + (x0 < w - 1 ? 1 : 0);
        const float ly1 = fminf(fmaxf(fy - (float)y0, 0.0f), 1.0f), lx1 = fminf(fmaxf(fx - (float)x0, 0.0f), 1.0f);
        const float ly0 = 1.0f - ly1, lx0 = 1.0f - lx1;
        const float* p00 = logits + ((f * h + y0) * w + x0) * ld;
        const float* p01 = logits + ((f * h + y0) * w + x1) * ld;
        const float* p10 = logits + ((f * h + y1) * w + x0) * ld;
        const float* p11 = logits + ((f * h + y1) * w + x1) * ld;
        float best = 0.0f;
        int arg = 0;
        for (int c4 = 0; c4 < ncls; c4 += 4) {                   // ld % 4 == 0 and ld >= ncls: the chunk stays inside the row
            const float4 a = *reinterpret_cast<const float4*>(p00 + c4), b = *reinterpret_cast<const float4*>(p01 + c4);
            const float4 c = *reinterpret_cast<const float4*>(p10 + c4), d = *reinterpret_cast<const float4*>(p11 + c4);
            const float v0 = ly0 * (lx0 * a.x + lx1 * b.x) + ly1 * (lx0 * c.x + lx1 * d.x);
            const float v1 = ly0 * (lx0 * a.y + lx1 * b.y) + ly1 * (lx0 * c.y + lx1 * d.y);
            const float v2 = ly0 * (lx0 * a.z + lx1 * b.z) + ly1 * (lx0 * c.z + lx1 * d.z);
            const float v3 = ly0 * (lx0 * a.w + lx1 * b.w) + ly1 * (lx0 * c.w + lx1 * d.w);
            // strictly greater: the first maximal index wins (torch.argmax); columns >= ncls are loaded but never compared
            if (c4 == 0) best = v0;
            else if (v0 > best) { best = v0; arg = c4; }
            if (c4 + 1 < ncls && v1 > best) { best = v1; arg = c4 + 1; }
            if (c4 + 2 < ncls && v2 > best) { best = v2; arg = c4 + 2; }
            if (c4 + 3 < ncls && v3 > best) { best = v3; arg = c4 + 3; }
        }
        out[i] = table[arg];
    }
}

}  // namespace

extern "C" int vface_parse_prefilter(const uint8_t* crops, int W2, int H2, int factor, void* out, int64_t ldo, int nframes, int dtype,
                                     void* stream_) {
    hipStream_t stream = vf_stream(stream_);
    if (!crops || !out || nframes <= 0 || W2 <= 0 || H2 <= 0) return VF_ERR_ARG;
    if (factor != 2 || (W2 & 1) || (H2 & 1) || W2 < 8 || H2 < 8 || ldo < 8) return VF_ERR_SHAPE;     // reflection needs 3 < size
    if ((long)W2 * H2 > 0x7fffffffL / 3) return VF_ERR_SHAPE;
    if ((ldo & 7) || ((uintptr_t)out & 15)) return VF_ERR_ALIGN;
    // BicubicDownSample.__init__: k[i] = bicubic((i - 4 + 0.5) / 2), a = -0.5, normalised by its fp32 sum (torch.sum's order on
    // eight values is sequential)
    Taps8 taps;
    float sum = 0.0f;
    for (int i = 0; i < 8; ++i) {
        const float x = fabsf(((float)i - 4.0f + 0.5f) / 2.0f), a = -0.5f;
        taps.k[i] = x <= 1.0f ? (a + 2.0f) * (x * x * x) - (a + 3.0f) * (x * x) + 1.0f
                              : (x < 2.0f ? a * (x * x * x) - 5.0f * a * (x * x) + 8.0f * a * x - 4.0f * a : 0.0f);
        sum += taps.k[i];
    }
    for (int i = 0; i < 8; ++i) taps.k[i] /= sum;
    const long total = (long)nframes * (H2 / 2) * (W2 / 2);
    DISPATCH_DTYPE(dtype, {
        using E = typename TT::elem;
        hipLaunchKernelGGL((parse_prefilter_kernel<TT>), dim3(vf_grid(total, 256, 16384)), dim3(256), 0, stream, crops, W2, H2, taps, (E*)out, ldo, total);
    });
    return vf_launched();
}

extern "C" int vface_maxpool3x3s2(const void* x, int64_t ldx, int nimg, int H, int W, int C, void* y, int64_t ldy, int dtype,
                                  void* stream_) {
    hipStream_t stream = vf_stream(stream_);
    if (!x || !y || nimg <= 0 || H <= 0 || W <= 0 || C <= 0) return VF_ERR_ARG;
    if (ldx < C || ldy < C) return VF_ERR_SHAPE;
    if ((C & 7) || (ldx & 7) || (ldy & 7) || (((uintptr_t)x | (uintptr_t)y) & 15)) return VF_ERR_ALIGN;
    const int OH = (H - 1) / 2 + 1, OW = (W - 1) / 2 + 1;
    const long M = (long)nimg * OH * OW;
    DISPATCH_DTYPE(dtype, {
        using E = typename TT::elem;
        hipLaunchKernelGGL((maxpool3x3s2_kernel<TT>), dim3(vf_grid(M * (C / 8), 256, 16384)), dim3(256), 0, stream, (const E*)x, ldx, H, W, C, OH, OW, (E*)y,
                           ldy, M);
    });
    return vf_launched();
}

extern "C" int vface_channel_gate(const void* x, int64_t ldx, const float* g, int64_t ldg, const float* rvec, int64_t ldrv,
                                  const void* rten, int64_t ldr, int add_x, void* y, int64_t ldy, int64_t M, int hw, int C, int dtype,
                                  void* stream_) {
    hipStream_t stream = vf_stream(stream_);
    if (!x || !g || !y || M <= 0 || hw <= 0 || C <= 0) return VF_ERR_ARG;
    if ((rvec != nullptr) + (rten != nullptr) + (add_x != 0) > 1) return VF_ERR_ARG;
    if (M % hw || ldx < C || ldy < C || ldg < C || (rvec && ldrv < C) || (rten && ldr < C)) return VF_ERR_SHAPE;
    if ((C & 7) || (ldx & 7) || (ldy & 7) || (ldr & 7) || (ldg & 3) || (ldrv & 3)) return VF_ERR_ALIGN;
    if (((uintptr_t)x | (uintptr_t)y | (uintptr_t)rten | (uintptr_t)g | (uintptr_t)rvec) & 15) return VF_ERR_ALIGN;
    DISPATCH_DTYPE(dtype, {
        using E = typename TT::elem;
        hipLaunchKernelGGL((channel_gate_kernel<TT>), dim3(vf_grid(M * (C / 8), 256, 16384)), dim3(256), 0, stream, (const E*)x, ldx, g, ldg, rvec, ldrv,
                           (const E*)rten, ldr, add_x, (E*)y, ldy, M, hw, C);
    });
    return vf_launched();
}

extern "C" int vface_pooled_linear(const float* a, int64_t lda, int sa, const float* W, const float* bias, float* out, int64_t ldo,
                                   int nimg, int N, int K, int act, void* stream_) {
    hipStream_t stream = vf_stream(stream_);
    if (!a || !W || !out || nimg <= 0 || N <= 0 || K <= 0 || sa <= 0) return VF_ERR_ARG;
    if (act != 0 && act != 1 && act != 3) return VF_ERR_ARG;
    if (ldo < N || lda < (long)(K - 1) * sa + 1) return VF_ERR_SHAPE;
    hipLaunchKernelGGL(pooled_linear_kernel, dim3((unsigned)(((long)nimg * N + 3) / 4)), dim3(256), 0, stream, a, lda, sa, W, bias, out, ldo,
                       nimg, N, K, act);
    return vf_launched();
}

extern "C" int vface_upsample_argmax_u8(const float* logits, int64_t ld, int nframes, int h, int w, int ncls, const uint8_t* table,
                                        uint8_t* out, int H, int W, void* stream_) {
    hipStream_t stream = vf_stream(stream_);
    if (!logits || !table || !out || nframes <= 0 || h <= 0 || w <= 0 || H <= 0 || W <= 0) return VF_ERR_ARG;
    if (ncls <= 0 || ncls > 32 || ld < ncls) return VF_ERR_SHAPE;
    if ((ld & 3) || ((uintptr_t)logits & 15)) return VF_ERR_ALIGN;
    const long total = (long)nframes * H * W;
    hipLaunchKernelGGL(upsample_argmax_u8_kernel, dim3(vf_grid(total, 256, 16384)), dim3(256), 0, stream, logits, ld, h, w, ncls, table, out, H, W, total);
    return vf_launched();
}
