// GIF out (REFace/scripts/VFace_inference_batch.py:658: clips.write_gif of the pasted frames): the pasted 8-bit RGB frames -> per frame
// a palette of up to 256 colours and the complete image data of a GIF frame (08, the LZW bit stream in sub-blocks, 00), on the frames
// where they already are.  scripts/gif.py adds the fixed headers and the 768 palette bytes; the host receives the palettes, the
// offsets and the bytes that exist.
//
// Five entry points, each beside its kernels, one stage of tests/gif_model.py each:
//   vface_gif_histogram   counts of the frame's pixels in 32768 cells of 8 x 8 x 8
//   vface_gif_boxes       median cut on the counts: a box number per cell, the number of boxes (csrc/gif_palette.hpp has the rule)
//   vface_gif_palette     a box's colour: the mean of the pixels in its cells
//   vface_gif_map         every pixel's nearest palette entry by exact search
//   vface_gif_lzw         segments of the index stream coded independently (csrc/gif_lzw.hpp has the encoder), every code placed at
//                         its bit offset, the sub-block framing
// The format is stated once, in tests/gif_model.py; these kernels equal it bit for bit.
#include "common.hpp"
#include "gif_lzw.hpp"
#include "gif_palette.hpp"
#include "launch.hpp"
#include "vface_kernels.hpp"

namespace {

constexpr int kGifHistShare = 65536;      // pixels of a frame that one workgroup counts in LDS before it adds them to the frame's counts
constexpr int kGifHistGridCap = 1024;     // workgroups, one (frame, share) each, before the grid loops (tests/test_gif_gpu.py)
constexpr int kGifBoxesGridCap = 64;      // workgroups, one frame each
constexpr int kGifPaletteShare = 16384;
constexpr int kGifPaletteGridCap = 2048;
constexpr int kGifMapShare = 8192;
constexpr int kGifMapGridCap = 4096;
constexpr int kGifLzwGridCap = 4096;      // workgroups of one wave, one (frame, segment) each
constexpr int kGifFlatGridCap = 2048;     // the pack and the framing: grid-stride over codes and bytes, 256 per workgroup
constexpr int kGifStage = 1024;           // indices a wave stages in LDS for its encoding lane
constexpr long kGifMaxPixels = 1L << 24;  // 255 * 2^24 < 2^32: a box's channel sum fits 32 bits
constexpr int kGifMaxSide = 65535;

inline bool gif_size_ok(int W, int H) { return W <= kGifMaxSide && H <= kGifMaxSide && (long)W * H <= kGifMaxPixels; }

// ---- histogram ---------------------------------------------------------------------------------------------------------------------
// One workgroup per (frame, share): 32768 counters in LDS (128 KiB: one workgroup per CU, so it is 16 waves wide).  Neighbouring
// pixels of real frames fall into one cell: a wave whose pixels all do adds their number once.
__global__ __launch_bounds__(1024) void gif_histogram_kernel(const unsigned char* __restrict__ rgb, long npix, long shares, long total,
                                                             unsigned* __restrict__ counts) {
    __shared__ unsigned h[kGifCells];
    const int tid = threadIdx.x, lane = tid & 63;
    for (long item = blockIdx.x; item < total; item += gridDim.x) {
        const long f = item / shares, p0 = (item - f * shares) * kGifHistShare, p1 = min(npix, p0 + kGifHistShare);
        const unsigned char* src = rgb + f * npix * 3;
        for (int i = tid; i < kGifCells; i += 1024) h[i] = 0;
        __syncthreads();
        for (long base = p0 + (tid - lane); base < p1; base += 1024) {
            const long p = base + lane;
            const bool valid = p < p1;
            const int cell = valid ? vf_gif_cell(src[3 * p], src[3 * p + 1], src[3 * p + 2]) : -1;
            const int first = __shfl(cell, 0);                       // lane 0 is valid: base < p1
            const unsigned long long all = __ballot(valid);
            if (__ballot(valid && cell != first) == 0) {
                if (lane == 0) atomicAdd(&h[first], (unsigned)__popcll(all));
            } else if (valid) {
                atomicAdd(&h[cell], 1u);
            }
        }
        __syncthreads();
        for (int i = tid; i < kGifCells; i += 1024)
            if (h[i]) atomicAdd(&counts[f * kGifCells + i], h[i]);
        __syncthreads();
    }
}

}  // namespace

extern "C" int vface_gif_histogram(const uint8_t* rgb, int W, int H, int frames, uint32_t* counts, void* stream_) {
    hipStream_t stream = vf_stream(stream_);
    if (!rgb || !counts || W <= 0 || H <= 0 || frames <= 0) return VF_ERR_ARG;
    if (!gif_size_ok(W, H)) return VF_ERR_SHAPE;
    const long npix = (long)W * H, shares = (npix + kGifHistShare - 1) / kGifHistShare, total = shares * frames;
    if (hipMemsetAsync(counts, 0, (size_t)frames * kGifCells * sizeof(uint32_t), stream) != hipSuccess) return VF_ERR_LAUNCH;
    hipLaunchKernelGGL(gif_histogram_kernel, dim3(vf_grid(total, 1, kGifHistGridCap)), dim3(1024), 0, stream, rgb, npix, shares, total, counts);
    return vf_launched();
}

// ---- boxes -------------------------------------------------------------------------------------------------------------------------
namespace {

enum { RED_POP = 0, RED_CELLS = 1, RED_LO = 2, RED_HI = 5, RED_WORDS = 8 };

__device__ inline void red_reset(int* red) {
    red[RED_POP] = 0; red[RED_CELLS] = 0;
    for (int a = 0; a < 3; ++a) { red[RED_LO + a] = 31; red[RED_HI + a] = 0; }
}

__device__ inline void red_merge(int* red, const VfGifBox& b) {
    if (b.ncells == 0) return;
    atomicAdd((unsigned*)&red[RED_POP], b.pop);
    atomicAdd(&red[RED_CELLS], b.ncells);
    for (int a = 0; a < 3; ++a) { atomicMin(&red[RED_LO + a], b.lo[a]); atomicMax(&red[RED_HI + a], b.hi[a]); }
}

__device__ inline void red_store(const int* red, VfGifBox& b) {
    b.pop = (unsigned)red[RED_POP]; b.ncells = red[RED_CELLS];
    for (int a = 0; a < 3; ++a) { b.lo[a] = red[RED_LO + a]; b.hi[a] = red[RED_HI + a]; }
}

constexpr int kGifBoxesThreads = 512;
constexpr int kGifBoxesOwn = kGifCells / kGifBoxesThreads;      // cells a thread owns, their counts in its registers

// One workgroup of 8 waves per frame; thread t owns cells t, t + 512, ... and keeps their 64 counts in registers, so the 2 x 255
// passes over the cells read LDS labels only.  A split is: the keys' maximum (a wave reduction), the chosen box's populations along its
// axis (LDS adds), the cut (gif_palette.hpp), and one pass that relabels the upper side and collects both sides' extents and populations.
__global__ __launch_bounds__(kGifBoxesThreads) void gif_boxes_kernel(const unsigned* __restrict__ counts, int frames, unsigned char* __restrict__ labels,
                                                                     int* __restrict__ ncolors) {
    __shared__ unsigned char lab[kGifCells];
    __shared__ VfGifBox boxes[kGifColors];
    __shared__ unsigned marg[32];
    __shared__ int red[2][RED_WORDS];
    __shared__ unsigned long long wkey[kGifBoxesThreads / 64];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    for (int f = blockIdx.x; f < frames; f += gridDim.x) {
        const unsigned* cnt = counts + (long)f * kGifCells;
        unsigned own[kGifBoxesOwn];
#pragma unroll
        for (int j = 0; j < kGifBoxesOwn; ++j) own[j] = cnt[tid + j * kGifBoxesThreads];
        if (tid == 0) red_reset(red[0]);
        __syncthreads();
        {
            VfGifBox mine;
            vf_gif_box_reset(mine);
#pragma unroll
            for (int j = 0; j < kGifBoxesOwn; ++j) {
                const int c = tid + j * kGifBoxesThreads;
                lab[c] = 0;
                if (own[j]) vf_gif_box_add(mine, c, own[j]);
            }
            red_merge(red[0], mine);
        }
        __syncthreads();
        if (tid == 0) red_store(red[0], boxes[0]);
        __syncthreads();
        int nb = 1;
        while (nb < kGifColors) {
            unsigned long long key = tid < nb ? vf_gif_box_key(boxes[tid], tid) : 0ull;
#pragma unroll
            for (int d = 32; d >= 1; d >>= 1) {
                const unsigned long long other = __shfl_xor(key, d);
                if (other > key) key = other;
            }
            if (lane == 0) wkey[wave] = key;
            if (tid < 32) marg[tid] = 0;
            if (tid == 0) { red_reset(red[0]); red_reset(red[1]); }
            __syncthreads();
            unsigned long long best = wkey[0];
#pragma unroll
            for (int k = 1; k < kGifColors / 64; ++k) best = wkey[k] > best ? wkey[k] : best;     // boxes live on the first four waves
            if (best == 0) break;                                    // the same for every thread
            const int i = 255 - (int)(best & 255);
            const int axis = vf_gif_box_axis(boxes[i]), lo = boxes[i].lo[axis], hi = boxes[i].hi[axis];
            const unsigned pop = boxes[i].pop;
#pragma unroll
            for (int j = 0; j < kGifBoxesOwn; ++j) {
                const int c = tid + j * kGifBoxesThreads;
                if (own[j] && lab[c] == i) atomicAdd(&marg[vf_gif_cell_coord(c, axis)], own[j]);
            }
            __syncthreads();
            const int cut = vf_gif_box_cut(marg, lo, hi, pop);
            VfGifBox lower, upper;
            vf_gif_box_reset(lower);
            vf_gif_box_reset(upper);
#pragma unroll
            for (int j = 0; j < kGifBoxesOwn; ++j) {
                const int c = tid + j * kGifBoxesThreads;
                if (own[j] && lab[c] == i) {
                    if (vf_gif_cell_coord(c, axis) > cut) {
                        lab[c] = (unsigned char)nb;
                        vf_gif_box_add(upper, c, own[j]);
                    } else {
                        vf_gif_box_add(lower, c, own[j]);
                    }
                }
            }
            red_merge(red[0], lower);
            red_merge(red[1], upper);
            __syncthreads();
            if (tid == 0) { red_store(red[0], boxes[i]); red_store(red[1], boxes[nb]); }
            ++nb;
            __syncthreads();
        }
        for (int c = tid; c < kGifCells; c += kGifBoxesThreads) labels[(long)f * kGifCells + c] = lab[c];
        if (tid == 0) ncolors[f] = nb;
        __syncthreads();
    }
}

}  // namespace

extern "C" int vface_gif_boxes(const uint32_t* counts, int frames, uint8_t* labels, int32_t* ncolors, void* stream_) {
    hipStream_t stream = vf_stream(stream_);
    if (!counts || !labels || !ncolors || frames <= 0) return VF_ERR_ARG;
    hipLaunchKernelGGL(gif_boxes_kernel, dim3(vf_grid(frames, 1, kGifBoxesGridCap)), dim3(kGifBoxesThreads), 0, stream, counts, frames, labels, ncolors);
    return vf_launched();
}

// ---- palette -----------------------------------------------------------------------------------------------------------------------
namespace {

// One workgroup per (frame, share): sums of R, G, B and the pixel count per box in LDS, added to the frame's sums at the end.  A wave
// whose pixels all lie in one box reduces them first.
__global__ __launch_bounds__(256) void gif_palette_sum_kernel(const unsigned char* __restrict__ rgb, long npix, long shares, long total,
                                                              const unsigned char* __restrict__ labels, unsigned* __restrict__ sums) {
    __shared__ unsigned acc[kGifColors * 4];
    const int tid = threadIdx.x, lane = tid & 63;
    for (long item = blockIdx.x; item < total; item += gridDim.x) {
        const long f = item / shares, p0 = (item - f * shares) * kGifPaletteShare, p1 = min(npix, p0 + kGifPaletteShare);
        const unsigned char* src = rgb + f * npix * 3;
        const unsigned char* lab = labels + f * kGifCells;
        for (int i = tid; i < kGifColors * 4; i += 256) acc[i] = 0;
        __syncthreads();
        for (long base = p0 + (tid - lane); base < p1; base += 256) {
            const long p = base + lane;
            const bool valid = p < p1;
            unsigned r = 0, g = 0, b = 0, n = 0;
            int box = -1;
            if (valid) {
                r = src[3 * p]; g = src[3 * p + 1]; b = src[3 * p + 2]; n = 1;
                box = lab[vf_gif_cell((int)r, (int)g, (int)b)];
            }
            const int first = __shfl(box, 0);
            if (__ballot(valid && box != first) == 0) {
#pragma unroll
                for (int d = 32; d >= 1; d >>= 1) {
                    r += __shfl_xor(r, d); g += __shfl_xor(g, d); b += __shfl_xor(b, d); n += __shfl_xor(n, d);
                }
                if (lane == 0) {
                    atomicAdd(&acc[first * 4], r); atomicAdd(&acc[first * 4 + 1], g); atomicAdd(&acc[first * 4 + 2], b);
                    atomicAdd(&acc[first * 4 + 3], n);
                }
            } else if (valid) {
                atomicAdd(&acc[box * 4], r); atomicAdd(&acc[box * 4 + 1], g); atomicAdd(&acc[box * 4 + 2], b); atomicAdd(&acc[box * 4 + 3], 1u);
            }
        }
        __syncthreads();
        if (acc[tid * 4 + 3]) {
#pragma unroll
            for (int k = 0; k < 4; ++k) atomicAdd(&sums[(f * kGifColors + tid) * 4 + k], acc[tid * 4 + k]);
        }
        __syncthreads();
    }
}

// an entry with no pixel is a box that does not exist: zeros
__global__ __launch_bounds__(256) void gif_palette_mean_kernel(const unsigned* __restrict__ sums, long entries, unsigned char* __restrict__ palette) {
    for (long e = blockIdx.x * 256L + threadIdx.x; e < entries; e += gridDim.x * 256L) {
        const unsigned n = sums[e * 4 + 3];
#pragma unroll
        for (int k = 0; k < 3; ++k) palette[e * 3 + k] = n ? (unsigned char)vf_gif_mean(sums[e * 4 + k], n) : 0;
    }
}

}  // namespace

extern "C" int vface_gif_palette(const uint8_t* rgb, int W, int H, int frames, const uint8_t* labels, uint8_t* palette, uint32_t* sums,
                                 void* stream_) {
    hipStream_t stream = vf_stream(stream_);
    if (!rgb || !labels || !palette || !sums || W <= 0 || H <= 0 || frames <= 0) return VF_ERR_ARG;
    if (!gif_size_ok(W, H)) return VF_ERR_SHAPE;
    if (((size_t)sums & 3) != 0) return VF_ERR_ALIGN;
    const long npix = (long)W * H, shares = (npix + kGifPaletteShare - 1) / kGifPaletteShare, total = shares * frames;
    if (hipMemsetAsync(sums, 0, (size_t)frames * kGifColors * 4 * sizeof(uint32_t), stream) != hipSuccess) return VF_ERR_LAUNCH;
    hipLaunchKernelGGL(gif_palette_sum_kernel, dim3(vf_grid(total, 1, kGifPaletteGridCap)), dim3(256), 0, stream, rgb, npix, shares, total, labels,
                       sums);
    hipLaunchKernelGGL(gif_palette_mean_kernel, dim3(vf_grid(frames, 1, kGifPaletteGridCap)), dim3(256), 0, stream, (const unsigned*)sums,
                       (long)frames * kGifColors, palette);
    return vf_launched();
}

// ---- index map ---------------------------------------------------------------------------------------------------------------------
namespace {

// One workgroup per (frame, share); the frame's palette in LDS, every lane reads the same entry (a broadcast).  A strictly smaller
// distance replaces the best: the lowest index wins a tie.
__global__ __launch_bounds__(256) void gif_map_kernel(const unsigned char* __restrict__ rgb, long npix, long shares, long total,
                                                      const unsigned char* __restrict__ palette, const int* __restrict__ ncolors,
                                                      unsigned char* __restrict__ indices) {
    __shared__ int pr[kGifColors], pg[kGifColors], pb[kGifColors];
    const int tid = threadIdx.x;
    for (long item = blockIdx.x; item < total; item += gridDim.x) {
        const long f = item / shares, p0 = (item - f * shares) * kGifMapShare, p1 = min(npix, p0 + kGifMapShare);
        const unsigned char* src = rgb + f * npix * 3;
        const int nc = min(max(ncolors[f], 1), kGifColors);
        pr[tid] = palette[(f * kGifColors + tid) * 3];
        pg[tid] = palette[(f * kGifColors + tid) * 3 + 1];
        pb[tid] = palette[(f * kGifColors + tid) * 3 + 2];
        __syncthreads();
        for (long p = p0 + tid; p < p1; p += 256) {
            const int r = src[3 * p], g = src[3 * p + 1], b = src[3 * p + 2];
            int best = 0x7FFFFFFF, at = 0;
            for (int j = 0; j < nc; ++j) {
                const int dr = r - pr[j], dg = g - pg[j], db = b - pb[j];
                const int d = dr * dr + dg * dg + db * db;
                if (d < best) { best = d; at = j; }
            }
            indices[f * npix + p] = (unsigned char)at;
        }
        __syncthreads();
    }
}

}  // namespace

extern "C" int vface_gif_map(const uint8_t* rgb, int W, int H, int frames, const uint8_t* palette, const int32_t* ncolors, uint8_t* indices,
                             void* stream_) {
    hipStream_t stream = vf_stream(stream_);
    if (!rgb || !palette || !ncolors || !indices || W <= 0 || H <= 0 || frames <= 0) return VF_ERR_ARG;
    if (!gif_size_ok(W, H)) return VF_ERR_SHAPE;
    const long npix = (long)W * H, shares = (npix + kGifMapShare - 1) / kGifMapShare, total = shares * frames;
    hipLaunchKernelGGL(gif_map_kernel, dim3(vf_grid(total, 1, kGifMapGridCap)), dim3(256), 0, stream, rgb, npix, shares, total, palette, ncolors,
                       indices);
    return vf_launched();
}

// ---- LZW ---------------------------------------------------------------------------------------------------------------------------
namespace {

// One wave per (frame, segment).  The wave zeroes the table and stages kGifStage indices in LDS; lane 0 walks them (gif_lzw.hpp) and
// writes the codes as 16-bit values into the segment's slot of the workspace; cnt takes their number.
__global__ __launch_bounds__(64) void gif_lzw_encode_kernel(const unsigned char* __restrict__ indices, long npix, int seg_pixels, long nseg,
                                                            long total, unsigned short* __restrict__ codes, long cap, int* __restrict__ cnt) {
    __shared__ unsigned table[kGifLzwSlots];
    __shared__ unsigned char stage[kGifStage];
    const int lane = threadIdx.x;
    for (long iv = blockIdx.x; iv < total; iv += gridDim.x) {
        const long f = iv / nseg, s = iv - f * nseg, p0 = s * seg_pixels;
        const int n = (int)min((long)seg_pixels, npix - p0);
        const unsigned char* src = indices + f * npix + p0;
        unsigned short* out = codes + iv * cap;
        VfGifLzwState st;
        vf_gif_lzw_begin(st);
        bool clear = true;
        int pos = 0;
        while (pos < n) {
            if (clear)
                for (int i = lane; i < kGifLzwSlots; i += 64) table[i] = 0;
            const int m = min(kGifStage, n - pos);
            for (int i = lane; i < m; i += 64) stage[i] = src[pos + i];
            __syncthreads();
            int took = m;
            if (lane == 0) took = vf_gif_lzw_run(stage, m, st, table, out, cap);
            took = __shfl(took, 0);
            clear = took < m;
            pos += took;
            __syncthreads();
        }
        if (lane == 0) {
            vf_gif_lzw_finish(st, s == nseg - 1, out, cap);
            cnt[iv] = (int)st.count;
        }
    }
}

template <typename T>
__device__ inline T gif_wave_inclusive_scan(T x, int lane) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const T y = __shfl_up(x, d);
        if (lane >= d) x += y;
    }
    return x;
}

// segbit[iv] = where segment iv's first code starts in its frame's bit stream (bit 9: behind the leading Clear), nbytes[f] = the
// stream's padded length, offsets[f] = where frame f's image data starts in the packed output, offsets[frames] = the end.  One workgroup.
__global__ __launch_bounds__(256) void gif_lzw_offsets_kernel(const int* __restrict__ cnt, long nseg, int frames, long long* __restrict__ segbit,
                                                              long long* __restrict__ nbytes, long long* __restrict__ offsets) {
    __shared__ long long wsum[4];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    long long at = 0;
    for (int f = 0; f < frames; ++f) {
        long long base = 9;
        for (long s0 = 0; s0 < nseg; s0 += 256) {
            const long s = s0 + tid;
            const long long v = s < nseg ? vf_gif_lzw_bits(cnt[f * nseg + s]) : 0;
            const long long incl = gif_wave_inclusive_scan(v, lane);
            if (lane == 63) wsum[wave] = incl;
            __syncthreads();
            long long before = 0, all = 0;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (k < wave) before += wsum[k];
                all += wsum[k];
            }
            if (s < nseg) segbit[f * nseg + s] = base + before + (incl - v);
            base += all;
            __syncthreads();
        }
        const long long nb = (base + 7) >> 3;
        if (tid == 0) { nbytes[f] = nb; offsets[f] = at; }
        at += 1 + nb + (nb + 254) / 255 + 1;
    }
    if (tid == 0) offsets[frames] = at;
}

// every code to its bit offset in the frame's zeroed bit stream -- LSB first: bit P of the stream is bit P & 31 of word P >> 5
__global__ __launch_bounds__(256) void gif_lzw_pack_kernel(const unsigned short* __restrict__ codes, long cap, const int* __restrict__ cnt,
                                                           const long long* __restrict__ segbit, long nseg, long total, unsigned* __restrict__ bits,
                                                           long words) {
    const long n = total * cap;
    for (long t = blockIdx.x * 256L + threadIdx.x; t < n; t += gridDim.x * 256L) {
        const long iv = t / cap, j = t - iv * cap;
        if (j >= cnt[iv]) continue;
        const long f = iv / nseg;
        unsigned* w = bits + f * words;
        if (j == 0 && iv == f * nseg) atomicOr(&w[0], (unsigned)kGifClear);          // the stream's leading Clear, 9 bits
        const long long P = segbit[iv] + vf_gif_lzw_bits(j);
        const long at = (long)(P >> 5);
        const int o = (int)(P & 31);
        const unsigned long long v = (unsigned long long)codes[t] << o;
        if (at < words) atomicOr(&w[at], (unsigned)v);
        if ((v >> 32) && at + 1 < words) atomicOr(&w[at + 1], (unsigned)(v >> 32));
    }
}

// byte k of a frame's stream goes to 2 + k + k / 255 of the frame's range: behind the 08 and one length byte per 255; the length bytes,
// the 08 and the closing 00 are written here too.  Bytes that would land at or past out_bytes are dropped.
__global__ __launch_bounds__(256) void gif_lzw_frame_kernel(const unsigned* __restrict__ bits, long words, long kmax, int frames,
                                                            const long long* __restrict__ nbytes, const long long* __restrict__ offsets,
                                                            unsigned char* __restrict__ out, long long out_bytes) {
    const long n = (long)frames * kmax;
    for (long t = blockIdx.x * 256L + threadIdx.x; t < n; t += gridDim.x * 256L) {
        const long f = t / kmax, k = t - f * kmax;
        const long long nb = nbytes[f], o = offsets[f];
        if (k >= nb) continue;
        auto put = [&](long long at, unsigned v) { if (at < out_bytes) out[at] = (unsigned char)v; };
        put(o + 2 + k + k / 255, (bits[f * words + (k >> 2)] >> (8 * (k & 3))) & 255u);
        if (k % 255 == 0) put(o + 1 + k + k / 255, (unsigned)min(255LL, nb - k));
        if (k == 0) { put(o, 8u); put(offsets[f + 1] - 1, 0u); }
    }
}

inline size_t align16(size_t n) { return (n + 15) & ~(size_t)15; }

struct GifLzwPlan {
    long nseg, total, cap, words, kmax;
    size_t cnt_at, segbit_at, nbytes_at, codes_at, bits_at, bytes;
};

// kmax: a frame's stream in bytes at most (every segment at its most codes); words: that in 32-bit words and one to spare
inline GifLzwPlan gif_lzw_plan(long npix, int frames, int seg_pixels) {
    GifLzwPlan p;
    const long full = npix / seg_pixels, last = npix % seg_pixels;
    p.nseg = full + (last ? 1 : 0);
    p.total = p.nseg * frames;
    p.cap = (vf_gif_lzw_max_codes(std::min((long)seg_pixels, npix)) + 1) & ~1L;
    const long maxbits = 9 + full * vf_gif_lzw_bits(vf_gif_lzw_max_codes(seg_pixels)) + (last ? vf_gif_lzw_bits(vf_gif_lzw_max_codes(last)) : 0);
    p.kmax = (maxbits + 7) / 8;
    p.words = (p.kmax + 3) / 4 + 1;
    p.cnt_at = 0;
    p.segbit_at = p.cnt_at + align16(p.total * sizeof(int));
    p.nbytes_at = p.segbit_at + align16(p.total * sizeof(long long));
    p.codes_at = p.nbytes_at + align16((size_t)frames * sizeof(long long));
    p.bits_at = p.codes_at + align16((size_t)p.total * p.cap * sizeof(unsigned short));
    p.bytes = p.bits_at + align16((size_t)frames * p.words * sizeof(unsigned));
    return p;
}

inline bool gif_lzw_shape_ok(int64_t npix, int frames, int seg_pixels) {
    return npix >= 1 && npix <= kGifMaxPixels && frames >= 1 && seg_pixels >= 1 && seg_pixels <= 65535;
}

}  // namespace

extern "C" int64_t vface_gif_lzw_bound(int64_t npix, int seg_pixels) {
    if (!gif_lzw_shape_ok(npix, 1, seg_pixels)) return 0;
    const long nb = gif_lzw_plan(npix, 1, seg_pixels).kmax;
    return 1 + nb + (nb + 254) / 255 + 1;
}

extern "C" size_t vface_gif_lzw_workspace_bytes(int64_t npix, int frames, int seg_pixels) {
    if (!gif_lzw_shape_ok(npix, frames, seg_pixels)) return 0;
    return gif_lzw_plan(npix, frames, seg_pixels).bytes;
}

extern "C" int vface_gif_lzw(const uint8_t* indices, int64_t npix, int frames, int seg_pixels, uint8_t* out, int64_t out_bytes, int64_t* offsets,
                             void* workspace, size_t workspace_bytes, void* stream_) {
    hipStream_t stream = vf_stream(stream_);
    if (!indices || !out || !offsets || !workspace || npix <= 0 || frames <= 0 || seg_pixels <= 0 || out_bytes <= 0) return VF_ERR_ARG;
    if (!gif_lzw_shape_ok(npix, frames, seg_pixels)) return VF_ERR_SHAPE;
    const GifLzwPlan p = gif_lzw_plan(npix, frames, seg_pixels);
    if (workspace_bytes < p.bytes) return VF_ERR_SHAPE;
    if (((size_t)workspace & 15) != 0) return VF_ERR_ALIGN;
    char* ws = (char*)workspace;
    int* cnt = (int*)(ws + p.cnt_at);
    long long* segbit = (long long*)(ws + p.segbit_at);
    long long* nbytes = (long long*)(ws + p.nbytes_at);
    unsigned short* codes = (unsigned short*)(ws + p.codes_at);
    unsigned* bits = (unsigned*)(ws + p.bits_at);
    if (hipMemsetAsync(bits, 0, (size_t)frames * p.words * sizeof(unsigned), stream) != hipSuccess) return VF_ERR_LAUNCH;
    hipLaunchKernelGGL(gif_lzw_encode_kernel, dim3(vf_grid(p.total, 1, kGifLzwGridCap)), dim3(64), 0, stream, indices, (long)npix, seg_pixels, p.nseg,
                       p.total, codes, p.cap, cnt);
    hipLaunchKernelGGL(gif_lzw_offsets_kernel, dim3(1), dim3(256), 0, stream, (const int*)cnt, p.nseg, frames, segbit, nbytes, (long long*)offsets);
    hipLaunchKernelGGL(gif_lzw_pack_kernel, dim3(vf_grid(p.total * p.cap, 256, kGifFlatGridCap)), dim3(256), 0, stream, (const unsigned short*)codes,
                       p.cap, (const int*)cnt, (const long long*)segbit, p.nseg, p.total, bits, p.words);
    hipLaunchKernelGGL(gif_lzw_frame_kernel, dim3(vf_grid((long)frames * p.kmax, 256, kGifFlatGridCap)), dim3(256), 0, stream, (const unsigned*)bits,
                       p.words, p.kmax, frames, (const long long*)nbytes, (const long long*)offsets, out, (long long)out_bytes);
    return vf_launched();
}
