// Colour-conversion half of the video intake, the mirror of mux.hip: I420 (`yuv420p`) frames as a YUV4MPEG2 file carries them ->
// the 8-bit RGB frames the intake, the parser, the flow producer and the paste-back consume.  The reference decodes the target
// video on the host (REFace/scripts/VFace_inference_batch.py:240-285: cv2.VideoCapture, BGR -> RGB, PNG); here the host uploads
// the planes, 1.5 bytes per pixel instead of 3, and this one launch makes the frames where they are used (HBM).  The H.264
// decoder is not built: scripts/demux.py reads YUV4MPEG2.
//
// The arithmetic is integer and is stated once, in tests/demux_model.py (`i420_to_rgb`); this kernel equals it bit for bit:
//   u16, v16 = the chroma of the pixel in sixteenths: the four neighbouring samples with integer weights that sum to 16, every
//              neighbour index clamped into the plane --
//                nearest  16 c[y >> 1][x >> 1]
//                centre   (3, 1) / 4 between sample i = x >> 1 and i - 1 (even x) or i + 1 (odd x), the same for rows
//                left     (4, 0) on even x, (2, 2) between i and i + 1 on odd x; rows as in centre
//   R = clamp((16 cY (Y - off) + cRV (v16 - 2048)                      + 2^19) >> 20, 0, 255)
//   G = clamp((16 cY (Y - off) + cGV (v16 - 2048) + cGU (u16 - 2048) + 2^19) >> 20, 0, 255)
//   B = clamp((16 cY (Y - off) + cBU (u16 - 2048)                      + 2^19) >> 20, 0, 255)
// 16-bit coefficients rounded from the fp64 constants of the matrix and the range; one rounding, then the clamp; every sum inside
// int32 (demux_model.value_ranges; tests/test_demux_cpu.py reads the tables below).
//
// Streaming, ~4.5 bytes per pixel (1.5 in, 3 out), no reuse beyond the chroma neighbours (the rows above and below hit in L2): no
// LDS.  One thread owns a strip of two rows x 16 pixels, the two rows of one chroma row: a 16-byte Y read and a 48-byte store per
// row, 8 bytes of Cb and of Cr plus one neighbour on each side from each of the (up to) three chroma rows the two luma rows touch.
// W * 3 is no multiple of 4 in general, so a row may start at any byte: a strip takes the widest form its ADDRESS allows (16-byte,
// 4-byte, single bytes), reads and stores alike; tails (fewer than 16 pixels) go byte by byte.  All indexing of the strip's
// registers is static after unrolling: nothing in scratch.
#include "common.hpp"
#include "launch.hpp"
#include "vface_kernels.hpp"

namespace {

// (cY, cRV, cGV, cGU, cBU) x 2^16, rounded; [limited, full] per matrix
constexpr int kBt709[2][5] = {{76309, 117489, -34925, -13975, 138438}, {65536, 103206, -30679, -12276, 121609}};
constexpr int kBt601[2][5] = {{76309, 104597, -53279, -25675, 132201}, {65536, 91881, -46802, -22553, 116130}};
constexpr int kStrip = 16;             // pixels per row of a thread's strip
constexpr int kDemuxGridCap = 2048;    // workgroups of 256 threads: eight per CU, then the grid loops (tests/test_demux_gpu.py GRID_CAP)
enum { kNearest = 0, kCentre = 1, kLeft = 2 };

struct DemuxCoeffs {
    int cy16, crv, cgv, cgu, cbu;           // cy16 = 16 cY
    int kr, kg, kb;                         // the constant of each channel's sum: 2^19 - 16 cY off - 2048 (its chroma coefficients)
};

// 16 bytes of a Y row into 4 words; only the first npix bytes exist
__device__ inline void load_luma(const unsigned char* __restrict__ p, int npix, unsigned (&w)[4]) {
    const unsigned long a = (unsigned long)p;
    if (npix == kStrip && (a & 15) == 0) {
        const uint4 v = *(const uint4*)p;
        w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
    } else if (npix == kStrip && (a & 3) == 0) {
#pragma unroll
        for (int i = 0; i < 4; ++i) w[i] = ((const unsigned*)p)[i];
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            unsigned v = 0;
#pragma unroll
            for (int b = 0; b < 4; ++b)
                if (4 * i + b < npix) v |= (unsigned)p[4 * i + b] << (8 * b);
            w[i] = v;
        }
    }
}

// the strip's samples of one chroma row: e[1..8] = row[i0 .. i0 + 7], e[0] and e[9] the neighbours, every index clamped into
// [0, cw - 1] (so a sample past the row's end reads as the row's last one, which is the clamp of the model)
template <int MODE>
__device__ inline void load_chroma(const unsigned char* __restrict__ row, int i0, int cw, int (&e)[10]) {
    if (i0 + 8 <= cw) {
        const unsigned char* p = row + i0;
        const unsigned long a = (unsigned long)p;
        unsigned w0, w1;
        if ((a & 7) == 0) {
            const uint2 v = *(const uint2*)p;
            w0 = v.x; w1 = v.y;
        } else if ((a & 3) == 0) {
            w0 = ((const unsigned*)p)[0]; w1 = ((const unsigned*)p)[1];
        } else {
            w0 = w1 = 0;
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                w0 |= (unsigned)p[b] << (8 * b);
                w1 |= (unsigned)p[4 + b] << (8 * b);
            }
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            e[1 + k] = (int)((w0 >> (8 * k)) & 255u);
            e[5 + k] = (int)((w1 >> (8 * k)) & 255u);
        }
        e[0] = e[9] = 0;
        if (MODE == kCentre) e[0] = row[max(i0 - 1, 0)];
        if (MODE != kNearest) e[9] = row[min(i0 + 8, cw - 1)];
    } else {
#pragma unroll
        for (int m = 0; m < 10; ++m) e[m] = row[min(max(i0 - 1 + m, 0), cw - 1)];
    }
}

// The weights are a product of a vertical and a horizontal pair, so the rows are blended first, at the 10 samples of the strip
// (quarters, <= 1020), and the columns second, at its 16 pixels (sixteenths): the same integers as the four-tap sum, fewer of them.
template <int MODE>
__device__ inline void blend_rows(const int (&own)[10], const int (&other)[10], int (&q)[10]) {
#pragma unroll
    for (int m = 0; m < 10; ++m) q[m] = MODE == kNearest ? 4 * own[m] : __mul24(3, own[m]) + other[m];
}

// pixel p of the strip (x0 is even, so p has the parity of x) from the blended samples q[1 + k], its neighbours q[k] and q[2 + k]
template <int MODE>
__device__ inline int chroma_sixteenths(const int (&q)[10], int p) {
    const int k = p >> 1;
    if (MODE == kCentre) return __mul24(3, q[1 + k]) + ((p & 1) ? q[2 + k] : q[k]);
    if (MODE == kLeft) return (p & 1) ? 2 * (q[1 + k] + q[2 + k]) : 4 * q[1 + k];
    return 4 * q[1 + k];
}

// 48 bytes of an output row from 12 words; only the first npix pixels exist
__device__ inline void store_rgb(unsigned char* __restrict__ p, const unsigned (&w)[12], int npix) {
    const unsigned long a = (unsigned long)p;
    if (npix == kStrip && (a & 15) == 0) {
#pragma unroll
        for (int i = 0; i < 3; ++i) ((uint4*)p)[i] = make_uint4(w[4 * i], w[4 * i + 1], w[4 * i + 2], w[4 * i + 3]);
    } else if (npix == kStrip && (a & 3) == 0) {
#pragma unroll
        for (int i = 0; i < 12; ++i) ((unsigned*)p)[i] = w[i];
    } else {
        const int nb = npix * 3;
#pragma unroll
        for (int i = 0; i < 48; ++i)
            if (i < nb) p[i] = (unsigned char)(w[i >> 2] >> (8 * (i & 3)));
    }
}

__device__ inline int clamp_byte(int v) { return min(max(v, 0), 255); }

// one output row of the strip: luma words `yw`, the row's own chroma row and the other one it blends with (centre, left).
// The constants of the three sums -- the rounding term, -16 cY off and -2048 x the chroma coefficients -- are folded into kr, kg,
// kb on the host: R = (16 cY Y + cRV v16 + kr) >> 20 is the model's sum term for term.  Every factor fits 24 bits (|coefficient| <
// 2^18, 16 cY < 2^21, Y < 2^8, u16, v16 < 2^12) and every partial sum int32 (demux_model.value_ranges), so the full-rate 24-bit
// multiply gives the bits of the quarter-rate 32-bit one.
template <int MODE>
__device__ inline void convert_row(const unsigned (&yw)[4], const int (&u_own)[10], const int (&u_other)[10], const int (&v_own)[10],
                                   const int (&v_other)[10], const DemuxCoeffs& c, unsigned (&out)[12]) {
    int uq[10], vq[10];
    blend_rows<MODE>(u_own, u_other, uq);
    blend_rows<MODE>(v_own, v_other, vq);
#pragma unroll
    for (int i = 0; i < 12; ++i) out[i] = 0;
#pragma unroll
    for (int p = 0; p < kStrip; ++p) {
        const int y = (int)((yw[p >> 2] >> (8 * (p & 3))) & 255u);
        const int u16 = chroma_sixteenths<MODE>(uq, p), v16 = chroma_sixteenths<MODE>(vq, p);
        const int luma = __mul24(c.cy16, y);
        const int r = clamp_byte((luma + c.kr + __mul24(c.crv, v16)) >> 20);
        const int g = clamp_byte((luma + c.kg + __mul24(c.cgv, v16) + __mul24(c.cgu, u16)) >> 20);
        const int b = clamp_byte((luma + c.kb + __mul24(c.cbu, u16)) >> 20);
        out[(3 * p) >> 2] |= (unsigned)r << (8 * ((3 * p) & 3));
        out[(3 * p + 1) >> 2] |= (unsigned)g << (8 * ((3 * p + 1) & 3));
        out[(3 * p + 2) >> 2] |= (unsigned)b << (8 * ((3 * p + 2) & 3));
    }
}

// in: frame f at f * frame_stride: Y [H][W], Cb [ch][cw], Cr [ch][cw]; rgb [frames][H][W][3].  One item = one strip.
template <int MODE>
__global__ __launch_bounds__(256) void yuv420_to_rgb_kernel(const unsigned char* __restrict__ in, long frame_stride, int W, int H,
                                                            unsigned char* __restrict__ rgb, unsigned items, unsigned strips, int cw,
                                                            int ch, DemuxCoeffs c) {
    // (items < 2^31, so the counter cannot wrap past the last stride of the capped grid; 32-bit divisions)
    const unsigned per_frame = strips * (unsigned)ch;
    for (unsigned it = blockIdx.x * 256 + threadIdx.x; it < items; it += gridDim.x * 256) {
        const long f = it / per_frame;
        const unsigned r = it - (unsigned)f * per_frame;
        const int cy = (int)(r / strips), sx = (int)(r - (unsigned)cy * strips);
        const int x0 = sx * kStrip, y0 = 2 * cy, i0 = x0 >> 1;
        const int npix = min(kStrip, W - x0);
        const bool two = y0 + 1 < H;
        const unsigned char* yp = in + f * frame_stride + (long)y0 * W + x0;
        const unsigned char* cbp = in + f * frame_stride + (long)W * H;
        const unsigned char* crp = cbp + (long)cw * ch;
        unsigned char* dst = rgb + ((f * H + y0) * (long)W + x0) * 3;

        unsigned ya[4], yb[4] = {0, 0, 0, 0};
        load_luma(yp, npix, ya);
        if (two) load_luma(yp + W, npix, yb);

        // chroma rows: the strip's own, the one above (even luma row) and the one below (odd luma row), clamped into the plane
        int u_own[10], v_own[10], u_up[10], v_up[10], u_dn[10], v_dn[10];
        load_chroma<MODE>(cbp + (long)cy * cw, i0, cw, u_own);
        load_chroma<MODE>(crp + (long)cy * cw, i0, cw, v_own);
        if (MODE != kNearest) {
            const long up = max(cy - 1, 0), dn = min(cy + 1, ch - 1);
            load_chroma<MODE>(cbp + up * cw, i0, cw, u_up);
            load_chroma<MODE>(crp + up * cw, i0, cw, v_up);
            load_chroma<MODE>(cbp + dn * cw, i0, cw, u_dn);
            load_chroma<MODE>(crp + dn * cw, i0, cw, v_dn);
        }

        unsigned out[12];
        convert_row<MODE>(ya, u_own, MODE == kNearest ? u_own : u_up, v_own, MODE == kNearest ? v_own : v_up, c, out);
        store_rgb(dst, out, npix);
        if (two) {
            convert_row<MODE>(yb, u_own, MODE == kNearest ? u_own : u_dn, v_own, MODE == kNearest ? v_own : v_dn, c, out);
            store_rgb(dst + (long)W * 3, out, npix);
        }
    }
}

}  // namespace

extern "C" int vface_yuv420_to_rgb(const uint8_t* i420, int64_t frame_stride, int W, int H, int frames, uint8_t* rgb, int matrix,
                                   int full_range, int chroma, void* stream_) {
    hipStream_t stream = vf_stream(stream_);
    if (!i420 || !rgb || W <= 0 || H <= 0 || frames <= 0) return VF_ERR_ARG;
    if (matrix < 0 || matrix > 1 || full_range < 0 || full_range > 1 || chroma < 0 || chroma > 2) return VF_ERR_ARG;
    const long cw = ((long)W + 1) / 2, ch = ((long)H + 1) / 2;
    if (frame_stride < (long)W * H + 2 * cw * ch) return VF_ERR_SHAPE;      // a frame would read into the next one
    const int* t = (matrix == 0 ? kBt709 : kBt601)[full_range];
    const int k0 = (1 << 19) - 16 * t[0] * (full_range ? 0 : 16);
    const DemuxCoeffs c = {16 * t[0], t[1], t[2], t[3], t[4], k0 - 2048 * t[1], k0 - 2048 * (t[2] + t[3]), k0 - 2048 * t[4]};
    const long strips = ((long)W + kStrip - 1) / kStrip;
    const long items = strips * ch * frames;
    if (items > 0x7fffffffL) return VF_ERR_SHAPE;                           // the kernel counts strips in 32 bits (2^36 pixels)
    const dim3 grid(vf_grid(items, 256, kDemuxGridCap)), block(256);
    if (chroma == kNearest)
        hipLaunchKernelGGL(yuv420_to_rgb_kernel<kNearest>, grid, block, 0, stream, i420, (long)frame_stride, W, H, rgb, (unsigned)items,
                           (unsigned)strips, (int)cw, (int)ch, c);
    else if (chroma == kCentre)
        hipLaunchKernelGGL(yuv420_to_rgb_kernel<kCentre>, grid, block, 0, stream, i420, (long)frame_stride, W, H, rgb, (unsigned)items,
                           (unsigned)strips, (int)cw, (int)ch, c);
    else
        hipLaunchKernelGGL(yuv420_to_rgb_kernel<kLeft>, grid, block, 0, stream, i420, (long)frame_stride, W, H, rgb, (unsigned)items,
                           (unsigned)strips, (int)cw, (int)ch, c);
    return vf_launched();
}
