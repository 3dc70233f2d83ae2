// Frame intake: from a decoded video frame to the tensors the sampler consumes (the mirror image of paste.hip).
//
// The reference does this frame by frame on the HOST with Pillow and numpy: `crop_image` (REFace/src/utils/alignmengt.py:99-145,
// reached from crop_faces_by_quads :255-263) makes the aligned crop, `VideoDataset.__getitem_gray__`
// (ldm/data/video_swap_dataset.py:135-240) makes image / inpaint_mask / inpaint_image, and VFace_inference_batch.py:459 resizes the
// mask to the latent grid.  Here the frames stay in HBM:
//
//   quad_crop_kernel         `img.crop(window)` + `img.transform((S, S), QUAD, quad + 0.5, BILINEAR)` (:115-123, :142; Pillow
//                            Geometry.c quad_transform / bilinear_filter32RGB): pixel CENTRES mapped through the bilinear QUAD map in
//                            double precision (no division), inside test on the WINDOW [0, w) x [0, h), taps clamped to the
//                            window (Pillow transforms the cropped image, so its edge repeats), double blend truncated to 8 bits,
//                            0 in all three bytes outside (an RGB image has no alpha).
//   dataset_tensors_kernel   get_tensor()(img) (:214), 1 - ToTensor(255 * isin(label, remove)) (:157-163, :219), image * mask (:221):
//                            uint8 crop + uint8 label map -> three planar fp32 tensors, one thread per pixel.
//   mask_latent_kernel       transforms.Resize on the mask tensor (VFace_inference_batch.py:459 = F.interpolate bilinear,
//                            align_corners = False, no antialias).  It reads the LABEL map, not inpaint_mask, so it does not depend
//                            on dataset_tensors_kernel's writes and may share its stream position with it.
//   source_tensors_kernel    the SOURCE image's side of VFace_inference_batch.py (:324-355, :462, :468): preserve mask, masked image,
//                            its (zero) inpaint image, the latent mask and the CLIP-normalised 224 x 224 image times the resized mask,
//                            one launch.  The 8-bit resize inside it stands for albumentations' A.Resize (cv2.INTER_LINEAR): OpenCV's
//                            11-bit fixed-point form as DESIGN §9 states it; parity with cv2.resize itself is NOT pinned (OpenCV is
//                            not available to the tests).
//
// The Lanczos shrink (:108-114) and the bicubic 512 x 512 resize (video_swap_dataset.py:139) are resample_u8_kernel of paste.hip
// with other tap tables (vface_amd/scripts/intake.py).  HBM-bound byte work, no LDS, one thread per output pixel, coalesced along x.
// Contraction is OFF: Pillow (C, no FMA on generic x86-64) and ATen round every product.
#include "common.hpp"
#include "launch.hpp"
#include "vface_kernels.hpp"

namespace {

// frames [F][Hs][Ws][3]; quads [F][8] = Pillow's QUAD coefficients in WINDOW coordinates; windows [F][4] = (x0, y0, x1, y1) in the
// frame (0 <= x0 < x1 <= Ws, 0 <= y0 < y1 <= Hs: checked by the caller, re-clamped here so that no tap can leave the frame);
// out [F][S][S][3]
__global__ __launch_bounds__(256) void quad_crop_kernel(const unsigned char* __restrict__ frames, int Ws, int Hs,
                                                        unsigned char* __restrict__ out, int S, const double* __restrict__ quads,
                                                        const int* __restrict__ windows) {
#pragma clang fp contract(off)
    const unsigned char* frame = frames + (long)blockIdx.y * Hs * Ws * 3;
    out += (long)blockIdx.y * S * S * 3;
    double a[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) a[j] = quads[(long)blockIdx.y * 8 + j];
    const int wx0 = min(max(windows[blockIdx.y * 4 + 0], 0), Ws - 1), wy0 = min(max(windows[blockIdx.y * 4 + 1], 0), Hs - 1);
    const int w = min(max(windows[blockIdx.y * 4 + 2], wx0 + 1), Ws) - wx0, h = min(max(windows[blockIdx.y * 4 + 3], wy0 + 1), Hs) - wy0;
    const unsigned char* win = frame + ((long)wy0 * Ws + wx0) * 3;
    const long total = (long)S * S;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const int py = (int)(i / S), px = (int)(i - (long)py * S);
        const double xc = px + 0.5, yc = py + 0.5;
        double xin = a[0] + a[1] * xc + a[2] * yc + a[3] * xc * yc;
        double yin = a[4] + a[5] * xc + a[6] * yc + a[7] * xc * yc;
        if (!(xin >= 0.0 && xin < (double)w && yin >= 0.0 && yin < (double)h)) {
            out[i * 3 + 0] = 0;
            out[i * 3 + 1] = 0;
            out[i * 3 + 2] = 0;
            continue;
        }
        xin -= 0.5;
        yin -= 0.5;
        const int x = xin < 0.0 ? (int)floor(xin) : (int)xin;
        const int y = yin < 0.0 ? (int)floor(yin) : (int)yin;
        const double dx = xin - x, dy = yin - y;
        const int x0 = min(max(x, 0), w - 1), x1 = min(max(x + 1, 0), w - 1);
        const int y0 = min(max(y, 0), h - 1);
        const bool has2 = (y + 1 >= 0) && (y + 1 < h);
        const unsigned char* r0 = win + (long)y0 * Ws * 3;
        const unsigned char* r1 = win + (long)(has2 ? y + 1 : y0) * Ws * 3;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const double p00 = r0[x0 * 3 + c], p01 = r0[x1 * 3 + c];
            double v1 = p00 + (p01 - p00) * dx;
            double v2 = v1;
            if (has2) {
                const double p10 = r1[x0 * 3 + c], p11 = r1[x1 * 3 + c];
                v2 = p10 + (p11 - p10) * dx;
            }
            v1 = v1 + (v2 - v1) * dy;
            out[i * 3 + c] = (unsigned char)(int)v1;
        }
    }
}

// crop [F][H][W][3], label [F][H][W], member[256] (1 = the label is on the remove list) -> image, inpaint [F][3][H][W], mask [F][1][H][W]
__global__ __launch_bounds__(256) void dataset_tensors_kernel(const unsigned char* __restrict__ crop,
                                                              const unsigned char* __restrict__ label,
                                                              const unsigned char* __restrict__ member, float* __restrict__ image,
                                                              float* __restrict__ inpaint, float* __restrict__ mask, long hw) {
#pragma clang fp contract(off)
    crop += (long)blockIdx.y * hw * 3;
    label += (long)blockIdx.y * hw;
    image += (long)blockIdx.y * hw * 3;
    inpaint += (long)blockIdx.y * hw * 3;
    mask += (long)blockIdx.y * hw;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < hw; i += (long)gridDim.x * 256) {
        const float m = 1.0f - (member[label[i]] ? 1.0f : 0.0f);      // 1 - ToTensor(255 or 0) = 1 - {1, 0}
        mask[i] = m;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float v = ((float)crop[i * 3 + c] / 255.0f - 0.5f) / 0.5f;
            image[(long)c * hw + i] = v;
            inpaint[(long)c * hw + i] = v * m;
        }
    }
}

// one bilinear sample of a {0, 1} map read through the membership table, frame_normalise_resize_kernel's fp32 order on one channel;
// `invert`: 1 - member (an inpaint mask) or member itself (the source's preserve mask)
__device__ __forceinline__ float member_bilinear(const unsigned char* __restrict__ label, const unsigned char* __restrict__ member,
                                                 int W, int H, int ox, int oy, float sx, float sy, bool invert) {
#pragma clang fp contract(off)
    const float fy = fmaxf(sy * ((float)oy + 0.5f) - 0.5f, 0.0f), fx = fmaxf(sx * ((float)ox + 0.5f) - 0.5f, 0.0f);
    const int y0 = min((int)fy, H - 1), x0 = min((int)fx, W - 1);
    const int y1 = min(y0 + 1, H - 1), x1 = min(x0 + 1, W - 1);
    const float ly1 = fy - (float)y0, lx1 = fx - (float)x0;
    const float ly0 = 1.0f - ly1, lx0 = 1.0f - lx1;
    auto px = [&](int yy, int xx) {
        const float m = member[label[(long)yy * W + xx]] ? 1.0f : 0.0f;
        return invert ? 1.0f - m : m;
    };
    const float top = lx0 * px(y0, x0) + lx1 * px(y0, x1);
    const float bot = lx0 * px(y1, x0) + lx1 * px(y1, x1);
    return ly0 * top + ly1 * bot;
}

// label [F][H][W] -> out [F][1][OH][OW] = resize_bilinear(1 - member[label])
__global__ __launch_bounds__(256) void mask_latent_kernel(const unsigned char* __restrict__ label,
                                                          const unsigned char* __restrict__ member, int W, int H,
                                                          float* __restrict__ out, int OW, int OH) {
    label += (long)blockIdx.y * H * W;
    out += (long)blockIdx.y * OH * OW;
    const float sy = (float)H / (float)OH, sx = (float)W / (float)OW;
    const long total = (long)OW * OH;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const int oy = (int)(i / OW), ox = (int)(i - (long)oy * OW);
        out[i] = member_bilinear(label, member, W, H, ox, oy, sx, sy, true);
    }
}

// The source image's tensors (VFace_inference_batch.py:324-355, :462, :468) in one launch.  Work items of one image, in this order:
//   [0, H W)                   mask = isin(label, preserve) (:324-341), masked = get_tensor()(img) * mask (:350-352),
//                              inpaint = masked * (1 - mask) (:354-355: x m (1 - m), zero for a {0, 1} mask; kept as the reference has it)
//   [H W, H W + OH OW)         mask_latent = Resize([OH, OW])(1 - mask) (:462, :468)
//   [.., + OC OC)              clip_image = get_tensor_clip()(A.Resize(OC, OC)(crop)) * Resize((OC, OC))(mask) (:342-347); the 8-bit
//                              resize is the 11-bit fixed-point 2-tap form (include/vface_hip.h), taps and weights from the host's tables
// crop [nimg][S][S][3], img [nimg][H][W][3], label [nimg][H][W]; xtap / ytap [OC][2] source indices, xw / yw [OC][2] weights
__global__ __launch_bounds__(256) void source_tensors_kernel(
    const unsigned char* __restrict__ crop, int S, const unsigned char* __restrict__ img, const unsigned char* __restrict__ label,
    const unsigned char* __restrict__ member, int W, int H, const int* __restrict__ xtap, const short* __restrict__ xw,
    const int* __restrict__ ytap, const short* __restrict__ yw, float* __restrict__ mask, float* __restrict__ masked,
    float* __restrict__ inpaint, float* __restrict__ mask_latent, int OW, int OH, float* __restrict__ clip_image,
    unsigned char* __restrict__ clip_u8, int OC) {
#pragma clang fp contract(off)
    const long hw = (long)H * W, nlat = (long)OH * OW, nclip = (long)OC * OC;
    crop += (long)blockIdx.y * S * S * 3;
    img += (long)blockIdx.y * hw * 3;
    label += (long)blockIdx.y * hw;
    mask += (long)blockIdx.y * hw;
    masked += (long)blockIdx.y * hw * 3;
    inpaint += (long)blockIdx.y * hw * 3;
    mask_latent += (long)blockIdx.y * nlat;
    clip_image += (long)blockIdx.y * nclip * 3;
    if (clip_u8) clip_u8 += (long)blockIdx.y * nclip * 3;
    const float mean[3] = {0.48145466f, 0.4578275f, 0.40821073f}, stdv[3] = {0.26862954f, 0.26130258f, 0.27577711f};
    const long total = hw + nlat + nclip;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        if (i < hw) {
            const float m = member[label[i]] ? 1.0f : 0.0f;               // ToTensor(255 or 0) = {1, 0}
            const float keep = 1.0f - m;
            mask[i] = m;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float v = ((float)img[i * 3 + c] / 255.0f - 0.5f) / 0.5f * m;
                masked[(long)c * hw + i] = v;
                inpaint[(long)c * hw + i] = v * keep;
            }
        } else if (i < hw + nlat) {
            const long j = i - hw;
            const int oy = (int)(j / OW), ox = (int)(j - (long)oy * OW);
            mask_latent[j] = member_bilinear(label, member, W, H, ox, oy, (float)W / (float)OW, (float)H / (float)OH, true);
        } else {
            const long j = i - hw - nlat;
            const int oy = (int)(j / OC), ox = (int)(j - (long)oy * OC);
            // (the tables come from the host: re-clamped so that no tap can leave the crop)
            const int xa = min(max(xtap[ox * 2], 0), S - 1), xb = min(max(xtap[ox * 2 + 1], 0), S - 1);
            const int ya = min(max(ytap[oy * 2], 0), S - 1), yb = min(max(ytap[oy * 2 + 1], 0), S - 1);
            const int w0 = xw[ox * 2], w1 = xw[ox * 2 + 1], v0 = yw[oy * 2], v1 = yw[oy * 2 + 1];
            const unsigned char* r0 = crop + (long)ya * S * 3;
            const unsigned char* r1 = crop + (long)yb * S * 3;
            const float mr = member_bilinear(label, member, W, H, ox, oy, (float)W / (float)OC, (float)H / (float)OC, false);
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const int R0 = r0[xa * 3 + c] * w0 + r0[xb * 3 + c] * w1;
                const int R1 = r1[xa * 3 + c] * w0 + r1[xb * 3 + c] * w1;
                const int q = (((v0 * (R0 >> 4)) >> 16) + ((v1 * (R1 >> 4)) >> 16) + 2) >> 2;
                const unsigned char q8 = (unsigned char)min(max(q, 0), 255);
                if (clip_u8) clip_u8[j * 3 + c] = q8;
                clip_image[(long)c * nclip + j] = ((float)q8 / 255.0f - mean[c]) / stdv[c] * mr;
            }
        }
    }
}

}  // namespace

extern "C" int vface_quad_crop(const uint8_t* frames, int Ws, int Hs, uint8_t* out, int S, int nframes, const double* quads,
                               const int32_t* windows, void* stream_) {
    hipStream_t stream = vf_stream(stream_);
    if (!frames || !out || !quads || !windows || nframes <= 0 || Ws <= 0 || Hs <= 0 || S <= 0) return VF_ERR_ARG;
    if ((long)Ws * Hs > 0x7fffffffL / 3 || (long)S * S > 0x7fffffffL / 3) return VF_ERR_SHAPE;
    hipLaunchKernelGGL(quad_crop_kernel, dim3(vf_grid((long)S * S, 256, 8192), nframes), dim3(256), 0, stream, frames, Ws, Hs, out, S, quads, windows);
    return vf_launched();
}

extern "C" int vface_dataset_tensors(const uint8_t* crop, const uint8_t* label, const uint8_t* member, int W, int H, float* image,
                                     float* inpaint_image, float* inpaint_mask, float* mask_latent, int OW, int OH, int nframes,
                                     void* stream_) {
    hipStream_t stream = vf_stream(stream_);
    if (!crop || !label || !member || !image || !inpaint_image || !inpaint_mask || !mask_latent) return VF_ERR_ARG;
    if (nframes <= 0 || W <= 0 || H <= 0 || OW <= 0 || OH <= 0) return VF_ERR_ARG;
    if ((long)W * H > 0x7fffffffL / 3) return VF_ERR_SHAPE;
    hipLaunchKernelGGL(dataset_tensors_kernel, dim3(vf_grid((long)W * H, 256, 8192), nframes), dim3(256), 0, stream, crop, label, member, image,
                       inpaint_image, inpaint_mask, (long)W * H);
    hipLaunchKernelGGL(mask_latent_kernel, dim3(vf_grid((long)OW * OH, 256, 8192), nframes), dim3(256), 0, stream, label, member, W, H, mask_latent,
                       OW, OH);
    return vf_launched();
}

extern "C" int vface_source_tensors(const uint8_t* crop, int S, const uint8_t* img, const uint8_t* label, const uint8_t* member, int W,
                                    int H, const int32_t* xtap, const int16_t* xw, const int32_t* ytap, const int16_t* yw, float* mask,
                                    float* masked, float* inpaint, float* mask_latent, int OW, int OH, float* clip_image,
                                    uint8_t* clip_u8, int OC, int nimg, void* stream_) {
    hipStream_t stream = vf_stream(stream_);
    if (!crop || !img || !label || !member || !xtap || !xw || !ytap || !yw) return VF_ERR_ARG;
    if (!mask || !masked || !inpaint || !mask_latent || !clip_image) return VF_ERR_ARG;      // (clip_u8 is optional)
    if (nimg <= 0 || S <= 0 || W <= 0 || H <= 0 || OW <= 0 || OH <= 0 || OC <= 0) return VF_ERR_ARG;
    if (nimg > 65535 || (long)S * S > 0x7fffffffL / 3 || (long)W * H > 0x7fffffffL / 3 || (long)OC * OC > 0x7fffffffL / 3 ||
        (long)OW * OH > 0x7fffffffL)
        return VF_ERR_SHAPE;
    const long total = (long)W * H + (long)OW * OH + (long)OC * OC;
    hipLaunchKernelGGL(source_tensors_kernel, dim3(vf_grid(total, 256, 8192), nimg), dim3(256), 0, stream, crop, S, img, label, member, W, H,
                       xtap, xw, ytap, yw, mask, masked, inpaint, mask_latent, OW, OH, clip_image, clip_u8, OC);
    return vf_launched();
}
