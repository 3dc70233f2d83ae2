// Colour-conversion half of the video mux (REFace/scripts/VFace_inference_batch.py:646-654): the pasted 8-bit RGB
// frames -> I420 (`-pix_fmt yuv420p`), BT.709 matrix, limited (`tv`) range, on the frames where they already are (HBM).  The
// reference hands PNG files to ffmpeg, whose swscale makes this conversion on the host; here it is one launch, and the host
// receives 1.5 bytes per pixel instead of 3.  H.264 and audio are not built: scripts/mux.py writes the planes as YUV4MPEG2.
//
// The arithmetic is integer and is stated once, in tests/mux_model.py (`rgb_to_i420`); this kernel equals it bit for bit:
//   Y' = (kLuma . (R, G, B) + (16 << 16) + (1 << 15)) >> 16                              per pixel
//   C  = (kCb|kCr . (sum R, sum G, sum B) + (128 << (16 + s)) + (1 << (15 + s))) >> (16 + s)
//        over the 2^s pixels of the 2 x 2 block that exist (4; 2 on an odd last column or row; 1 in the odd corner)
// 16-bit coefficients rounded from the fp64 BT.709 constants; each chroma row sums to zero.  No clamp: Y' stays in [16, 235], Cb
// and Cr in [16, 240], and every sum inside int32 (mux_model.value_ranges; tests/test_mux_cpu.py reads the tables below).
//
// Streaming, ~4.5 bytes per pixel (3 in, 1.5 out), no reuse: no LDS.  One thread owns a strip of two rows x 16 pixels = one 48-byte
// read per row and a 16-byte Y store per row, 8 bytes of Cb and of Cr -- so that the widest access (16 B per lane) serves both the
// reads and the Y stores, and neighbouring lanes touch neighbouring bytes.  W * 3 is no multiple of 4 in general, so a row may start
// at any byte: a strip takes the widest form its ADDRESS allows (16-byte, 4-byte, single bytes), the same for the stores; tails
// (fewer than 16 pixels) go byte by byte.  All indexing of the strip's registers is static after unrolling: nothing in scratch.
#include "common.hpp"
#include "launch.hpp"
#include "vface_kernels.hpp"

namespace {

constexpr int kLuma[3] = {11966, 40254, 4064};
constexpr int kCb[3] = {-6596, -22189, 28785};
constexpr int kCr[3] = {28784, -26145, -2639};
constexpr int kStrip = 16;           // pixels per row of a thread's strip
constexpr int kMuxGridCap = 2048;    // workgroups of 256 threads: eight per CU, then the grid loops (tests/test_mux_gpu.py GRID_CAP)

// 48 bytes of a row (16 pixels) into 12 words; pixels past `npix` read as zero (so they add nothing to a chroma sum)
__device__ inline void load_strip(const unsigned char* __restrict__ p, int npix, unsigned (&w)[12]) {
    const unsigned long a = (unsigned long)p;
    if (npix == kStrip && (a & 15) == 0) {
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            const uint4 v = ((const uint4*)p)[i];
            w[4 * i] = v.x; w[4 * i + 1] = v.y; w[4 * i + 2] = v.z; w[4 * i + 3] = v.w;
        }
    } else if (npix == kStrip && (a & 3) == 0) {
#pragma unroll
        for (int i = 0; i < 12; ++i) w[i] = ((const unsigned*)p)[i];
    } else {
        const int nb = npix * 3;
#pragma unroll
        for (int i = 0; i < 12; ++i) {
            unsigned v = 0;
#pragma unroll
            for (int b = 0; b < 4; ++b)
                if (4 * i + b < nb) v |= (unsigned)p[4 * i + b] << (8 * b);
            w[i] = v;
        }
    }
}

// N = 4 (Y: 16 bytes) or 2 (a chroma plane: 8 bytes); only the first nb bytes exist
template <int N>
__device__ inline void store_bytes(unsigned char* __restrict__ p, const unsigned (&w)[N], int nb) {
    const unsigned long a = (unsigned long)p;
    if (nb == 4 * N && (a & (4 * N - 1)) == 0) {
        if constexpr (N == 4) *(uint4*)p = make_uint4(w[0], w[1], w[2], w[3]);
        else *(uint2*)p = make_uint2(w[0], w[1]);
    } else if (nb == 4 * N && (a & 3) == 0) {
#pragma unroll
        for (int i = 0; i < N; ++i) ((unsigned*)p)[i] = w[i];
    } else {
#pragma unroll
        for (int i = 0; i < 4 * N; ++i)
            if (i < nb) p[i] = (unsigned char)(w[i >> 2] >> (8 * (i & 3)));
    }
}

__device__ inline int byte_of(const unsigned (&w)[12], int i) { return (int)((w[i >> 2] >> (8 * (i & 3))) & 255u); }

// rgb [frames][H][W][3]; out: frame f at f * frame_stride: Y [H][W], Cb [ch][cw], Cr [ch][cw].  One item = one strip.
__global__ __launch_bounds__(256) void rgb_to_yuv420_kernel(const unsigned char* __restrict__ rgb, int W, int H,
                                                            unsigned char* __restrict__ out, long frame_stride, long items,
                                                            int strips, int cw, int ch) {
    const long per_frame = (long)strips * ch;
    for (long it = (long)blockIdx.x * 256 + threadIdx.x; it < items; it += (long)gridDim.x * 256) {
        const long f = it / per_frame;
        const long r = it - f * per_frame;
        const int cy = (int)(r / strips), sx = (int)(r - (long)cy * strips);
        const int x0 = sx * kStrip, y0 = 2 * cy;
        const int npix = min(kStrip, W - x0);
        const bool two = y0 + 1 < H;
        const unsigned char* src = rgb + ((f * H + y0) * (long)W + x0) * 3;
        unsigned char* yp = out + f * frame_stride + (long)y0 * W + x0;
        unsigned char* cbp = out + f * frame_stride + (long)W * H + (long)cy * cw + (x0 >> 1);
        unsigned char* crp = cbp + (long)cw * ch;

        unsigned r0[12], r1[12];
        load_strip(src, npix, r0);
        if (two) load_strip(src + (long)W * 3, npix, r1);
        else {
#pragma unroll
            for (int i = 0; i < 12; ++i) r1[i] = 0;
        }

        unsigned ya[4] = {0, 0, 0, 0}, yb[4] = {0, 0, 0, 0}, cb[2] = {0, 0}, cr[2] = {0, 0};
        const int sy = two ? 1 : 0;
#pragma unroll
        for (int k = 0; k < kStrip / 2; ++k) {
            int sr = 0, sg = 0, sb = 0;
#pragma unroll
            for (int j = 2 * k; j < 2 * k + 2; ++j) {
                const int ra = byte_of(r0, 3 * j), ga = byte_of(r0, 3 * j + 1), ba = byte_of(r0, 3 * j + 2);
                const int rb = byte_of(r1, 3 * j), gb = byte_of(r1, 3 * j + 1), bb = byte_of(r1, 3 * j + 2);
                const int y_a = (kLuma[0] * ra + kLuma[1] * ga + kLuma[2] * ba + (16 << 16) + (1 << 15)) >> 16;
                const int y_b = (kLuma[0] * rb + kLuma[1] * gb + kLuma[2] * bb + (16 << 16) + (1 << 15)) >> 16;
                ya[j >> 2] |= (unsigned)y_a << (8 * (j & 3));
                yb[j >> 2] |= (unsigned)y_b << (8 * (j & 3));
                sr += ra + rb; sg += ga + gb; sb += ba + bb;
            }
            // pixels of this block that exist: (1 or 2 columns) x (1 or 2 rows) = 2^s
            const int s = 16 + sy + ((x0 + 2 * k + 1 < W) ? 1 : 0);
            const int u = (kCb[0] * sr + kCb[1] * sg + kCb[2] * sb + (128 << s) + (1 << (s - 1))) >> s;
            const int v = (kCr[0] * sr + kCr[1] * sg + kCr[2] * sb + (128 << s) + (1 << (s - 1))) >> s;
            cb[k >> 2] |= (unsigned)u << (8 * (k & 3));
            cr[k >> 2] |= (unsigned)v << (8 * (k & 3));
        }
        store_bytes<4>(yp, ya, npix);
        if (two) store_bytes<4>(yp + W, yb, npix);
        const int nc = (npix + 1) >> 1;
        store_bytes<2>(cbp, cb, nc);
        store_bytes<2>(crp, cr, nc);
    }
}

}  // namespace

extern "C" int vface_rgb_to_yuv420(const uint8_t* rgb, int W, int H, uint8_t* out, int64_t frame_stride, int frames, void* stream_) {
    hipStream_t stream = vf_stream(stream_);
    if (!rgb || !out || W <= 0 || H <= 0 || frames <= 0) return VF_ERR_ARG;
    const long cw = ((long)W + 1) / 2, ch = ((long)H + 1) / 2;
    if (frame_stride < (long)W * H + 2 * cw * ch) return VF_ERR_SHAPE;      // the frames would overlap
    const long strips = ((long)W + kStrip - 1) / kStrip;
    const long items = strips * ch * frames;
    hipLaunchKernelGGL(rgb_to_yuv420_kernel, dim3(vf_grid(items, 256, kMuxGridCap)), dim3(256), 0, stream, rgb, W, H, out,
                       (long)frame_stride, items, (int)strips, (int)cw, (int)ch);
    return vf_launched();
}
