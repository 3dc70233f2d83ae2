// Motion-JPEG half of the video mux (REFace/scripts/VFace_inference_batch.py:646-654 ends in a compressed, playable
// file): the pasted 8-bit RGB frames -> the entropy-coded scan of a baseline 4:2:0 JPEG per frame, on the frames where they
// already are.  scripts/mjpeg.py adds the headers and writes the frames into an AVI; the host receives the compressed bytes only.
//
// Two entry points, each beside its kernels:
//   vface_jpeg_coefficients   RGB -> JFIF Y'CbCr (full-range BT.601, NOT the BT.709 tv range of mux.hip) -> 2 x 2 chroma mean ->
//                             level shift -> 8 x 8 forward DCT -> quantise -> zigzag, one fused pass
//   vface_jpeg_entropy        Huffman coding (the four Annex-K tables) with restart intervals, then compaction of a frame's scan
//
// The arithmetic is integer and is stated once, in tests/jpeg_model.py; these kernels equal it bit for bit:
//   Y  = (19595 R + 38470 G + 7471 B + 32768) >> 16
//   Cb = min(255, (-11059 SR - 21709 SG + 32768 SB + (128 << 18) + (1 << 17)) >> 18)      S over the 2 x 2 block
//   Cr = min(255, ( 32768 SR - 27439 SG -  5329 SB + (128 << 18) + (1 << 17)) >> 18)
//   rows: t = (C . (x - 128) + (1 << 10)) >> 11      columns: c = C . t      C[k][n] = rint(8192 a_k cos((2n + 1) k pi / 16))
//   q = sign(c) ((|c| + (d >> 1)) / d), d = Q << 15  ==  sign(c) ((n * ceil(2^20 / Q)) >> 20), n = (|c| + (Q << 14)) >> 15
// Integer sums are exact in any order: the 8-point transform is split into its even and odd halves (C[k][7 - n] = +-C[k][n]).
// The reciprocal multiply is exact for every n the transform can produce (n <= 1151) and every Q in 1..255; every sum fits
// int32 (jpeg_model.value_ranges, tests/test_mjpeg_cpu.py).
#include "common.hpp"
#include "launch.hpp"
#include "vface_kernels.hpp"

namespace {

constexpr int kDct[8][8] = {{2896, 2896, 2896, 2896, 2896, 2896, 2896, 2896},
                            {4017, 3406, 2276, 799, -799, -2276, -3406, -4017},
                            {3784, 1567, -1567, -3784, -3784, -1567, 1567, 3784},
                            {3406, -799, -4017, -2276, 2276, 4017, 799, -3406},
                            {2896, -2896, -2896, 2896, 2896, -2896, -2896, 2896},
                            {2276, -4017, 799, 3406, -3406, -799, 4017, -2276},
                            {1567, -3784, 3784, -1567, -1567, 3784, -3784, 1567},
                            {799, -2276, 3406, -4017, 4017, -3406, 2276, -799}};
// kZigzag[k] = row-major index (8 v + u) of the k-th coefficient of the scan
__device__ const unsigned char kZigzag[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                              41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                              30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
constexpr int kMcuPerGroup = 4;       // one MCU (16 x 16 pixels, 6 blocks) per wave, four waves per workgroup
constexpr int kJpegGridCap = 2048;    // workgroups before the grid loops (tests/test_mjpeg_gpu.py GRID_CAP)
constexpr int kMcuCoefs = 6 * 64;
constexpr int kRecipShift = 20;

// one 8-point transform: even outputs from the sums x[n] + x[7 - n], odd ones from the differences
__device__ inline void dct8(const int (&x)[8], int (&y)[8]) {
    int s[4], d[4];
#pragma unroll
    for (int n = 0; n < 4; ++n) { s[n] = x[n] + x[7 - n]; d[n] = x[n] - x[7 - n]; }
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        int acc = 0;
#pragma unroll
        for (int n = 0; n < 4; ++n) acc += kDct[k][n] * ((k & 1) ? d[n] : s[n]);
        y[k] = acc;
    }
}

// rgb [frames][H][W][3]; out: frame f at f * frame_stride (elements): [mcu_rows][mcu_cols][6][64] int16, zigzag order, blocks
// Y00 Y01 Y10 Y11 Cb Cr.  qy, qc: the quantisation tables, row-major.  A workgroup takes four MCUs at a time, one per wave; the
// loop's trip count is the same for every wave of the workgroup (the barriers), a wave past the last MCU idles through it.
__global__ __launch_bounds__(256) void jpeg_coefficients_kernel(const unsigned char* __restrict__ rgb, int W, int H,
                                                                const unsigned char* __restrict__ qy,
                                                                const unsigned char* __restrict__ qc, short* __restrict__ out,
                                                                long frame_stride, long mcus, long groups, int mcu_cols,
                                                                int per_frame) {
    __shared__ int px[kMcuPerGroup][6][64];     // the six blocks, level-shifted pixels; after the column pass the coefficients c
    __shared__ int tt[kMcuPerGroup][6][64];     // after the row pass
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int zz = kZigzag[lane];
    const int qyv = max(1, (int)qy[zz]), qcv = max(1, (int)qc[zz]);
    const unsigned ry = ((1u << kRecipShift) + qyv - 1) / qyv, rc = ((1u << kRecipShift) + qcv - 1) / qcv;

    for (long g = blockIdx.x; g < groups; g += gridDim.x) {
        const long m = g * kMcuPerGroup + wave;
        const bool live = m < mcus;
        const long f = live ? m / per_frame : 0;
        const int rem = live ? (int)(m - f * per_frame) : 0;
        if (live) {
            // lane: row r of the MCU, pixels x4 .. x4 + 3; coordinates clamped into the frame (replication of the last column and row)
            const int my = rem / mcu_cols, mx = rem - my * mcu_cols;
            const int r = lane >> 2, x4 = (lane & 3) * 4;
            const int gy = min(my * 16 + r, H - 1), gx0 = mx * 16 + x4;
            const unsigned char* row = rgb + (f * H + gy) * (long)W * 3;
            int R[4], G[4], B[4];
            const unsigned char* p = row + (long)gx0 * 3;
            if (gx0 + 4 <= W && ((unsigned long)p & 3) == 0) {
                const unsigned w0 = ((const unsigned*)p)[0], w1 = ((const unsigned*)p)[1], w2 = ((const unsigned*)p)[2];
                R[0] = w0 & 255; G[0] = (w0 >> 8) & 255; B[0] = (w0 >> 16) & 255;
                R[1] = w0 >> 24; G[1] = w1 & 255; B[1] = (w1 >> 8) & 255;
                R[2] = (w1 >> 16) & 255; G[2] = w1 >> 24; B[2] = w2 & 255;
                R[3] = (w2 >> 8) & 255; G[3] = (w2 >> 16) & 255; B[3] = w2 >> 24;
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const unsigned char* q = row + (long)min(gx0 + j, W - 1) * 3;
                    R[j] = q[0]; G[j] = q[1]; B[j] = q[2];
                }
            }
            const int yb = (r >> 3) * 2 + (x4 >> 3), yo = (r & 7) * 8 + (x4 & 7);
#pragma unroll
            for (int j = 0; j < 4; ++j) px[wave][yb][yo + j] = ((19595 * R[j] + 38470 * G[j] + 7471 * B[j] + 32768) >> 16) - 128;
            // the row below (r ^ 1) is lane ^ 4: both lanes get the sums of the two 2 x 2 blocks; the even row makes Cb, the odd one Cr
            int sr[2], sg[2], sb[2];
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                sr[h] = R[2 * h] + R[2 * h + 1]; sg[h] = G[2 * h] + G[2 * h + 1]; sb[h] = B[2 * h] + B[2 * h + 1];
                sr[h] += __shfl_xor(sr[h], 4); sg[h] += __shfl_xor(sg[h], 4); sb[h] += __shfl_xor(sb[h], 4);
            }
            const int co = (r >> 1) * 8 + (x4 >> 1);
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int acc = (r & 1) ? 32768 * sr[h] - 27439 * sg[h] - 5329 * sb[h] : -11059 * sr[h] - 21709 * sg[h] + 32768 * sb[h];
                px[wave][4 + (r & 1)][co + h] = min(255, (acc + (128 << 18) + (1 << 17)) >> 18) - 128;
            }
        }
        __syncthreads();
        if (live && lane < 48) {        // rows: lane = (block, row)
            const int b = lane >> 3, r = lane & 7;
            int x[8], y[8];
#pragma unroll
            for (int n = 0; n < 8; ++n) x[n] = px[wave][b][r * 8 + n];
            dct8(x, y);
#pragma unroll
            for (int k = 0; k < 8; ++k) tt[wave][b][r * 8 + k] = (y[k] + (1 << 10)) >> 11;
        }
        __syncthreads();
        if (live && lane < 48) {        // columns: lane = (block, column)
            const int b = lane >> 3, u = lane & 7;
            int x[8], y[8];
#pragma unroll
            for (int n = 0; n < 8; ++n) x[n] = tt[wave][b][n * 8 + u];
            dct8(x, y);
#pragma unroll
            for (int k = 0; k < 8; ++k) px[wave][b][k * 8 + u] = y[k];
        }
        __syncthreads();
        if (live) {                     // quantise and store: lane = position in the scan
            short* o = out + f * frame_stride + (long)rem * kMcuCoefs + lane;
#pragma unroll
            for (int b = 0; b < 6; ++b) {
                const int c = px[wave][b][zz];
                const unsigned n = ((unsigned)abs(c) + ((unsigned)(b < 4 ? qyv : qcv) << 14)) >> 15;
                const int q = (int)((n * (b < 4 ? ry : rc)) >> kRecipShift);
                o[b * 64] = (short)(c < 0 ? -q : q);
            }
        }
        __syncthreads();
    }
}

}  // namespace

extern "C" int vface_jpeg_coefficients(const uint8_t* rgb, int W, int H, int frames, const uint8_t* qluma, const uint8_t* qchroma,
                                       int16_t* out, int64_t frame_stride, void* stream_) {
    hipStream_t stream = vf_stream(stream_);
    if (!rgb || !qluma || !qchroma || !out || W <= 0 || H <= 0 || frames <= 0) return VF_ERR_ARG;
    if (W > 65535 || H > 65535) return VF_ERR_SHAPE;                          // SOF0 carries 16 bits
    const long mcu_cols = (W + 15) / 16, per_frame = mcu_cols * ((H + 15) / 16);
    if (frame_stride < per_frame * kMcuCoefs) return VF_ERR_SHAPE;            // the frames would overlap
    const long mcus = per_frame * frames, groups = (mcus + kMcuPerGroup - 1) / kMcuPerGroup;
    hipLaunchKernelGGL(jpeg_coefficients_kernel, dim3(vf_grid(groups, 1, kJpegGridCap)), dim3(256), 0, stream, rgb, W, H, qluma,
                       qchroma, out, (long)frame_stride, mcus, groups, (int)mcu_cols, (int)per_frame);
    return vf_launched();
}

// ---- entropy coding ----------------------------------------------------------------------------------------------------------
// Baseline Huffman coding with the typical tables of T.81 Annex K (BITS, HUFFVAL), as the DHT segments of scripts/mjpeg.py carry them.
namespace {

__device__ const unsigned char kDcBits[2][16] = {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0}, {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0}};
__device__ const unsigned char kAcBits[2][16] = {{0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7D},
                                                 {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77}};
__device__ const unsigned char kAcVals[2][162] = {
    {0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81,
     0x91, 0xA1, 0x08, 0x23, 0x42, 0xB1, 0xC1, 0x15, 0x52, 0xD1, 0xF0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0A, 0x16, 0x17, 0x18,
     0x19, 0x1A, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2A, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3A, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48,
     0x49, 0x4A, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5A, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6A, 0x73, 0x74, 0x75,
     0x76, 0x77, 0x78, 0x79, 0x7A, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8A, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99,
     0x9A, 0xA2, 0xA3, 0xA4, 0xA5, 0xA6, 0xA7, 0xA8, 0xA9, 0xAA, 0xB2, 0xB3, 0xB4, 0xB5, 0xB6, 0xB7, 0xB8, 0xB9, 0xBA, 0xC2, 0xC3,
     0xC4, 0xC5, 0xC6, 0xC7, 0xC8, 0xC9, 0xCA, 0xD2, 0xD3, 0xD4, 0xD5, 0xD6, 0xD7, 0xD8, 0xD9, 0xDA, 0xE1, 0xE2, 0xE3, 0xE4, 0xE5,
     0xE6, 0xE7, 0xE8, 0xE9, 0xEA, 0xF1, 0xF2, 0xF3, 0xF4, 0xF5, 0xF6, 0xF7, 0xF8, 0xF9, 0xFA},
    {0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08,
     0x14, 0x42, 0x91, 0xA1, 0xB1, 0xC1, 0x09, 0x23, 0x33, 0x52, 0xF0, 0x15, 0x62, 0x72, 0xD1, 0x0A, 0x16, 0x24, 0x34, 0xE1, 0x25,
     0xF1, 0x17, 0x18, 0x19, 0x1A, 0x26, 0x27, 0x28, 0x29, 0x2A, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3A, 0x43, 0x44, 0x45, 0x46, 0x47,
     0x48, 0x49, 0x4A, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5A, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6A, 0x73, 0x74,
     0x75, 0x76, 0x77, 0x78, 0x79, 0x7A, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8A, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97,
     0x98, 0x99, 0x9A, 0xA2, 0xA3, 0xA4, 0xA5, 0xA6, 0xA7, 0xA8, 0xA9, 0xAA, 0xB2, 0xB3, 0xB4, 0xB5, 0xB6, 0xB7, 0xB8, 0xB9, 0xBA,
     0xC2, 0xC3, 0xC4, 0xC5, 0xC6, 0xC7, 0xC8, 0xC9, 0xCA, 0xD2, 0xD3, 0xD4, 0xD5, 0xD6, 0xD7, 0xD8, 0xD9, 0xDA, 0xE2, 0xE3, 0xE4,
     0xE5, 0xE6, 0xE7, 0xE8, 0xE9, 0xEA, 0xF2, 0xF3, 0xF4, 0xF5, 0xF6, 0xF7, 0xF8, 0xF9, 0xFA}};

// Worst case of one block, in bits: each of its 64 coefficients costs at most a 16-bit code and 10 value bits (the DC at most
// 11 + 11; a ZRL, 11 bits, stands for 16 zero coefficients, the EOB, 4 bits, for at least one): 64 x 26 = 1664 bits = 208
// bytes, doubled because every byte may be an FF that takes a stuffed 00 behind it.  The 1-padding of an interval completes its
// last byte and stays inside the 208.  An interval's slot of the workspace is that times its blocks.
constexpr int kBlockBytesBound = 2 * (64 * (16 + 10) / 8);
constexpr int kEntropyGridCap = 16384;    // workgroups of one wave before the grid loops over the intervals
constexpr int kWinWords = 64;             // the wave's bit window: carry (< 8 bits) + a block (<= 1664) + padding (< 8) < 2048 bits

// (code << 5 | length) of the i-th symbol of a table, canonical assignment (T.81 Annex C)
__device__ inline unsigned canonical_code(const unsigned char* bits, int i) {
    int code = 0, first = 0;
    for (int l = 1; l <= 16; ++l) {
        const int nb = bits[l - 1];
        if (i < first + nb) return ((unsigned)(code + i - first) << 5) | (unsigned)l;
        code = (code + nb) << 1;
        first += nb;
    }
    return 0;
}

template <typename T>
__device__ inline T wave_inclusive_scan(T x, int lane) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const T y = __shfl_up(x, d);
        if (lane >= d) x += y;
    }
    return x;
}

// One wave per restart interval: `restart` MCUs (fewer in a frame's last interval), DC predictors reset at its start, 1-padded to
// a whole byte at its end, FF bytes stuffed -- so the intervals are independent.  Lane k holds coefficient k of the current
// block: the zero runs come from the ballot of the non-zero lanes, each lane builds its own bits (ZRLs, code, value; lane 0 the DC
// difference, lane 63 the EOB if its coefficient is zero), a prefix sum of the lengths places them, LDS atomic OR merges them into
// the wave's window.  After every block the whole bytes of the window go out (stuffed, placed by a second prefix sum) to the
// interval's slot in the workspace and the open byte is carried to the front of the window.
__global__ __launch_bounds__(64) void jpeg_entropy_kernel(const short* __restrict__ coef, long frame_stride, int mcus, int restart,
                                                          int nint, long total, unsigned char* __restrict__ slots, long slot_bytes,
                                                          int* __restrict__ lens) {
    __shared__ unsigned actab[2][256];
    __shared__ unsigned dctab[2][32];
    __shared__ unsigned win[kWinWords];
    const int lane = threadIdx.x;
    for (int t = 0; t < 2; ++t) {
        for (int i = lane; i < 256; i += 64) actab[t][i] = 0;
        if (lane < 32) dctab[t][lane] = 0;
    }
    __syncthreads();
    for (int t = 0; t < 2; ++t) {
        for (int i = lane; i < 162; i += 64) actab[t][kAcVals[t][i]] = canonical_code(kAcBits[t], i);
        if (lane < 12) dctab[t][lane] = canonical_code(kDcBits[t], lane);
    }
    __syncthreads();

    for (long iv = blockIdx.x; iv < total; iv += gridDim.x) {
        const long f = iv / nint;
        const int i = (int)(iv - f * nint);
        const int m0 = i * restart, m1 = min(m0 + restart, mcus);
        const short* cf = coef + f * frame_stride + (long)m0 * kMcuCoefs;
        unsigned char* dst = slots + iv * slot_bytes;
        win[lane] = 0;
        __syncthreads();
        int pred0 = 0, pred1 = 0, pred2 = 0;
        unsigned carry = 0;     // bits of the open byte at the front of the window
        long written = 0;
        const int nblk = (m1 - m0) * 6;
        for (int blk = 0; blk < nblk; ++blk) {
            const int b = blk % 6, comp = b < 4 ? 0 : b - 3, t = comp ? 1 : 0;
            int v = cf[(long)blk * 64 + lane];
            const int dc = __shfl(v, 0);
            const int pred = comp == 0 ? pred0 : (comp == 1 ? pred1 : pred2);
            if (comp == 0) pred0 = dc; else if (comp == 1) pred1 = dc; else pred2 = dc;
            if (lane == 0) v -= pred;
            const unsigned long long mask = __ballot(v != 0) & ~1ull;          // the non-zero AC positions
            const unsigned a = (unsigned)abs(v);
            const int s = a ? 32 - __clz(a) : 0;
            const unsigned vb = (unsigned)(v < 0 ? v - 1 : v) & ((1u << s) - 1u);
            unsigned long long bits = 0;
            int L = 0;
            if (lane == 0) {
                const unsigned e = dctab[t][min(s, 31)];
                bits = ((unsigned long long)(e >> 5) << s) | vb;
                L = (int)(e & 31) + s;
            } else if (v != 0) {
                const unsigned long long below = mask & ((1ull << lane) - 1ull);
                const int p = below ? 63 - __clzll(below) : 0;
                const int run = lane - 1 - p, nz = run >> 4;
                const unsigned z = actab[t][0xF0];
#pragma unroll
                for (int k = 0; k < 3; ++k)
                    if (k < nz) { bits = (bits << (z & 31)) | (z >> 5); L += (int)(z & 31); }
                const unsigned e = actab[t][((run & 15) << 4) | (s & 15)];
                bits = (bits << ((e & 31) + s)) | ((unsigned long long)(e >> 5) << s) | vb;
                L += (int)(e & 31) + s;
            } else if (lane == 63) {
                const unsigned e = actab[t][0];
                bits = e >> 5;
                L = (int)(e & 31);
            }
            const int incl = wave_inclusive_scan(L, lane);
            const int tot = __shfl(incl, 63);
            if (L > 0 && L <= 64) {
                const unsigned P = carry + (unsigned)(incl - L);
                const unsigned long long hi = bits << (64 - L);
                const unsigned o = P & 31, w = P >> 5;
                const unsigned w0 = (unsigned)(hi >> (32 + o)), w1 = (unsigned)(hi >> o), w2 = o ? (unsigned)(hi << (32 - o)) : 0u;
                if (w0 && w < kWinWords) atomicOr(&win[w], w0);
                if (w1 && w + 1 < kWinWords) atomicOr(&win[w + 1], w1);
                if (w2 && w + 2 < kWinWords) atomicOr(&win[w + 2], w2);
            }
            unsigned wbits = carry + (unsigned)tot;
            if (blk == nblk - 1) {                                              // 1-padding to the byte
                const unsigned pad = (8 - (wbits & 7)) & 7;
                if (pad && lane == 0 && (wbits >> 5) < kWinWords) atomicOr(&win[wbits >> 5], ((1u << pad) - 1u) << (32 - (wbits & 31) - pad));
                wbits += pad;
            }
            __syncthreads();
            // the whole bytes leave: lane = word of the window, four bytes, most significant first
            const int nbytes = (int)(wbits >> 3);
            const unsigned word = win[lane];
            const unsigned cw = win[min(nbytes >> 2, kWinWords - 1)];
            const int valid = max(0, min(4, nbytes - 4 * lane));
            int cnt = valid;
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (j < valid && ((word >> (24 - 8 * j)) & 255u) == 255u) ++cnt;
            const int oincl = wave_inclusive_scan(cnt, lane);
            long at = written + (oincl - cnt);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (j < valid) {
                    const unsigned byte = (word >> (24 - 8 * j)) & 255u;
                    if (at < slot_bytes) dst[at] = (unsigned char)byte;
                    ++at;
                    if (byte == 255u) {
                        if (at < slot_bytes) dst[at] = 0;
                        ++at;
                    }
                }
            }
            written += __shfl(oincl, 63);
            __syncthreads();
            carry = wbits & 7;
            win[lane] = (lane == 0 && carry) ? ((cw >> (24 - 8 * (nbytes & 3))) & 255u) << 24 : 0u;
            __syncthreads();
        }
        if (lane == 0) lens[iv] = (int)min(written, slot_bytes);
    }
}

// offs[i] = where interval i starts in the packed output: the exclusive prefix sum of (length + 2 for the RST marker behind every
// interval but a frame's last) over all intervals of all frames; offs[total] = the end.  One workgroup.
__global__ __launch_bounds__(256) void jpeg_offsets_kernel(const int* __restrict__ lens, long* __restrict__ offs, long total, int nint) {
    __shared__ long long wsum[4];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    long long base = 0;
    for (long s = 0; s < total; s += 256) {
        const long i = s + tid;
        const long long v = i < total ? lens[i] + ((int)(i % nint) != nint - 1 ? 2 : 0) : 0;
        const long long incl = wave_inclusive_scan(v, lane);
        if (lane == 63) wsum[wave] = incl;
        __syncthreads();
        long long before = 0, all = 0;
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            if (w < wave) before += wsum[w];
            all += wsum[w];
        }
        if (i < total) offs[i] = base + before + (incl - v);
        base += all;
        __syncthreads();
    }
    if (tid == 0) offs[total] = base;
}

// copies every interval from its slot to its place, RSTm (m = index in the frame mod 8) behind it unless it ends the frame, and
// writes each frame's byte count.  Bytes that would land past `out_bytes` are dropped (the caller sees it from the lengths).
__global__ __launch_bounds__(256) void jpeg_pack_kernel(const unsigned char* __restrict__ slots, long slot_bytes, const int* __restrict__ lens,
                                                        const long* __restrict__ offs, long total, int nint, unsigned char* __restrict__ out,
                                                        long out_bytes, int* __restrict__ lengths) {
    for (long iv = blockIdx.x; iv < total; iv += gridDim.x) {
        const unsigned char* src = slots + iv * slot_bytes;
        const long o = offs[iv];
        const int n = lens[iv], i = (int)(iv % nint);
        for (int j = threadIdx.x; j < n; j += 256)
            if (o + j < out_bytes) out[o + j] = src[j];
        if (threadIdx.x == 0) {
            if (i != nint - 1) {
                if (o + n < out_bytes) out[o + n] = 0xFF;
                if (o + n + 1 < out_bytes) out[o + n + 1] = (unsigned char)(0xD0 + (i & 7));
            } else {
                lengths[iv / nint] = (int)(o + n - offs[iv - i]);
            }
        }
    }
}

inline size_t align16(size_t n) { return (n + 15) & ~(size_t)15; }

}  // namespace

extern "C" size_t vface_jpeg_entropy_workspace_bytes(int mcus, int frames, int restart) {
    if (mcus <= 0 || frames <= 0 || restart <= 0) return 0;
    const size_t nint = ((size_t)mcus + restart - 1) / restart, total = nint * frames;
    const size_t slot = (size_t)std::min(restart, mcus) * 6 * kBlockBytesBound;
    return align16(total * sizeof(int)) + align16((total + 1) * sizeof(long)) + total * slot;
}

extern "C" int vface_jpeg_entropy(const int16_t* coef, int64_t frame_stride, int mcus, int frames, int restart, uint8_t* out,
                                  int64_t out_bytes, int32_t* lengths, void* workspace, size_t workspace_bytes, void* stream_) {
    hipStream_t stream = vf_stream(stream_);
    if (!coef || !out || !lengths || !workspace || mcus <= 0 || frames <= 0 || restart <= 0 || out_bytes <= 0) return VF_ERR_ARG;
    if (restart > 65535 || frame_stride < (long)mcus * kMcuCoefs) return VF_ERR_SHAPE;      // DRI carries 16 bits
    if (workspace_bytes < vface_jpeg_entropy_workspace_bytes(mcus, frames, restart)) return VF_ERR_SHAPE;
    if (((size_t)workspace & 15) != 0) return VF_ERR_ALIGN;
    const long nint = ((long)mcus + restart - 1) / restart, total = nint * frames;
    const long slot = (long)std::min(restart, mcus) * 6 * kBlockBytesBound;
    int* lens = (int*)workspace;
    long* offs = (long*)((char*)workspace + align16(total * sizeof(int)));
    unsigned char* slots = (unsigned char*)offs + align16((total + 1) * sizeof(long));
    hipLaunchKernelGGL(jpeg_entropy_kernel, dim3(vf_grid(total, 1, kEntropyGridCap)), dim3(64), 0, stream, (const short*)coef,
                       (long)frame_stride, mcus, restart, (int)nint, total, slots, slot, lens);
    hipLaunchKernelGGL(jpeg_offsets_kernel, dim3(1), dim3(256), 0, stream, (const int*)lens, offs, total, (int)nint);
    hipLaunchKernelGGL(jpeg_pack_kernel, dim3(vf_grid(total, 1, kEntropyGridCap)), dim3(256), 0, stream, (const unsigned char*)slots,
                       slot, (const int*)lens, (const long*)offs, total, (int)nint, out, (long)out_bytes, lengths);
    return vf_launched();
}
