// PNG frames in (REFace/scripts/VFace_inference_batch.py:285 writes the target clip as {index}.png, and a run reads them back): the
// zlib bodies of a batch's files -> 8-bit RGB frames, on the device where every later stage reads them.  The counterpart of
// csrc/png.hip.  scripts/png_in.py walks the chunks, checks their CRCs and the zlib header on the host, uploads the deflate bodies
// as they lie in the files and folds the Adler-32 from the two halves each file returns.
//
// Two entry points, each beside its kernel:
//   vface_png_inflate    RFC 1951, all three block types, one wave per file: the symbol chain of a stream is serial, so the bit
//                        position and the symbol decode are wave-uniform, and the 64 lanes share what has width -- the loads of the
//                        stream into LDS, the flush of pending literals, match and stored-block copies, the rows' way to global
//                        memory and the Adler sums.  The last 32 KiB of output are a ring in LDS: a match reads the ring, never
//                        global memory that a lane of the same wave has just written.
//   vface_png_unfilter   the five PNG filter types undone in a skewed wavefront: lane r is on row y0 + r one pixel behind lane
//                        r - 1, so that left, up and up-left arrive by cross-lane moves; bands of 64 rows one after another
// Everything that file bytes steer and that indexes memory is csrc/png_inflate.hpp, which a host program runs under sanitizers; the
// format is stated once in tests/png_inflate_model.py and equalled bit for bit.
#include "common.hpp"
#include "launch.hpp"
#include "png_inflate.hpp"
#include "vface_kernels.hpp"

namespace {

constexpr int kInflateGridCap = 1024;     // workgroups, one file each, before the grid loops
constexpr int kUnfilterGridCap = 1024;
constexpr int kRingMask = kInfWindow - 1;
constexpr int kFlushBytes = 4096;         // the ring's new bytes leave for global memory once there are this many
constexpr int kInChunk = 256, kInWindow = 512;   // the stream crosses LDS in chunks of 4 bytes per lane; two chunks are kept
constexpr unsigned kAdlerMod = 65521u;
constexpr int kUnfilterMaxW = 8192;       // the row carried from band to band lives in LDS, one word per pixel

// The stream of one file behind VfInfBits: bytes [loaded - 512, loaded) stand in `win` at their position mod 512.  `ensure` runs
// in every lane alike (the reader's state is wave-uniform) and loads the next chunk once the reader is within 8 bytes of the end
// of what is loaded; a refill asks for at most 8 bytes from `pos` on.  No byte at or behind `end` is loaded.
struct LdsStream {
    const unsigned char* bytes;     // the file's first byte
    unsigned char* win;
    long loaded, end;
    int lane;
    __device__ void ensure(long pos) {
        while (pos + 8 > loaded && loaded < end) {
#pragma unroll
            for (int k = 0; k < kInChunk / 64; ++k) {
                const long q = loaded + lane + 64 * k;
                if (q < end) win[q & (kInWindow - 1)] = bytes[q];
            }
            loaded += kInChunk;
            __syncthreads();
        }
    }
    __device__ unsigned at(long pos) const { return win[pos & (kInWindow - 1)]; }
};

template <typename T>
__device__ inline T wave_sum(T x) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) x += __shfl_xor(x, d);
    return x;
}

// One workgroup of ONE wave per file: __launch_bounds__(64) is part of the contract of csrc/png_inflate.hpp's table builds, whose
// serial parts every lane does alike on the same LDS addresses, which only a single wave in lockstep may do.
// Every lane runs the decode with the same values; what a lane does alone is marked by `lane`.
// A file's bytes go to the ring as they are produced and from the ring to rows + f * file_stride in pieces of about kFlushBytes,
// which is also where the Adler halves are summed; what was produced before a fault is written too, nothing behind it.
// With `flags` (the last launch of vface_png_inflate_parallel, csrc/png_in_par.hip; nullptr otherwise): only files whose flag is set
// are decoded, and nothing of the others is touched.
__global__ __launch_bounds__(64) void png_inflate_kernel(const unsigned char* __restrict__ streams, long stream_bytes,
                                                         const long* __restrict__ offsets, const int* __restrict__ lengths, int files,
                                                         unsigned char* __restrict__ rows, long file_stride, long expect,
                                                         int* __restrict__ status_out, int* __restrict__ produced,
                                                         int* __restrict__ consumed, unsigned* __restrict__ adler,
                                                         const int* __restrict__ flags) {
    __shared__ unsigned char ring[kInfWindow];
    __shared__ VfInfTables tb;
    __shared__ unsigned char win[kInWindow];
    const int lane = threadIdx.x;

    for (long f = blockIdx.x; f < files; f += gridDim.x) {
        if (flags && !flags[f]) continue;
        const long off = offsets[f], n = lengths[f];
        unsigned s1 = 1, s2 = 0;
        long op = 0, flushed = 0, used = 0;
        int status = VF_INF_OK;
        if (off < 0 || n < 0 || off > stream_bytes || n > stream_bytes - off) {
            status = VF_INF_SHORT;                  // the file's range does not lie inside the buffer: nothing of it is read
        } else {
            unsigned char* out = rows + f * file_stride;
            VfInfBits<LdsStream> b = {{streams + off, win, 0, n, lane}, 0, n, 0ull, 0};
            int npend = 0;                          // literals not yet in the ring: lane k holds the k-th
            unsigned mylit = 0;
            // ring -> global memory and the checksum, [flushed, upto)
            auto flush = [&](long upto) {
                const long L = upto - flushed;
                unsigned long long a1 = 0, a2 = 0;
                for (long i = lane; i < L; i += 64) {
                    const unsigned v = ring[(flushed + i) & kRingMask];
                    out[flushed + i] = (unsigned char)v;
                    a1 += v;
                    a2 += (unsigned long long)(L - i) * v;
                }
                a1 = wave_sum(a1);
                a2 = wave_sum(a2);
                s2 = (unsigned)((s2 + (unsigned long long)(L % kAdlerMod) * s1 + a2 % kAdlerMod) % kAdlerMod);
                s1 = (unsigned)((s1 + a1 % kAdlerMod) % kAdlerMod);
                flushed = upto;
            };
            auto flush_pending = [&]() {
                if (lane < npend) ring[(op + lane) & kRingMask] = (unsigned char)mylit;
                op += npend;
                npend = 0;
                __syncthreads();
                if (op - flushed >= kFlushBytes) flush(op);
            };

            int final_block = 0;
            while (status == VF_INF_OK && !final_block) {
                int type, stored;
                status = VF_INF_UNIFORM(vf_inf_block(b, final_block, type, stored));
                if (status != VF_INF_OK) break;
                final_block = VF_INF_UNIFORM(final_block);
                type = VF_INF_UNIFORM(type);
                if (type == 0) {
                    stored = VF_INF_UNIFORM(stored);
                    if (op + stored > expect) { status = VF_INF_TOO_LONG; break; }
                    for (int done = 0; done < stored;) {
                        const int piece = min(stored - done, kFlushBytes);
                        for (int i = lane; i < piece; i += 64) ring[(op + i) & kRingMask] = b.src.bytes[b.pos + done + i];
                        __syncthreads();
                        op += piece;
                        done += piece;
                        if (op - flushed >= kFlushBytes) flush(op);
                    }
                    b.pos += stored;
                    b.src.loaded = b.pos & ~(long)(kInChunk - 1);       // the window starts over at the chunk that holds pos
                    continue;
                }
                if (type == 1) vf_inf_fixed_tables(tb, lane, 64);
                else status = VF_INF_UNIFORM(vf_inf_dynamic_tables(b, tb, lane, 64));
                while (status == VF_INF_OK) {
                    VfInfToken t;
                    status = VF_INF_UNIFORM(vf_inf_token(b, tb, t));
                    if (status != VF_INF_OK) break;
                    const int length = VF_INF_UNIFORM(t.length), value = VF_INF_UNIFORM(t.value);
                    if (length < 0) break;
                    if (length == 0) {
                        if (op + npend + 1 > expect) { status = VF_INF_TOO_LONG; break; }
                        if (lane == npend) mylit = (unsigned)value;
                        if (++npend == 64) flush_pending();
                        continue;
                    }
                    flush_pending();
                    if (value > op) { status = VF_INF_TOO_FAR; break; }
                    if (op + length > expect) { status = VF_INF_TOO_LONG; break; }
                    // out[p + i] = out[p - d + i mod d]: every source byte lies in front of the match, so the lanes do not wait for one another
                    if (value >= length) {
                        for (int i = lane; i < length; i += 64) {
                            const unsigned char v = ring[(op - value + i) & kRingMask];
                            ring[(op + i) & kRingMask] = v;
                        }
                    } else {
                        for (int i = lane; i < length; i += 64) {
                            const unsigned char v = ring[(op - value + i % value) & kRingMask];
                            ring[(op + i) & kRingMask] = v;
                        }
                    }
                    __syncthreads();
                    op += length;
                    if (op - flushed >= kFlushBytes) flush(op);
                }
                flush_pending();                    // a block's last literals, also behind a fault: they were produced
            }
            if (status == VF_INF_OK && op != expect) status = VF_INF_TOO_FEW;
            flush(op);
            used = status == VF_INF_SHORT ? n : vf_inf_consumed(b);
        }
        if (lane == 0) {
            status_out[f] = status;
            produced[f] = (int)op;
            consumed[f] = (int)used;
            adler[2 * f] = s1;
            adler[2 * f + 1] = s2;
        }
        __syncthreads();
    }
}

}  // namespace

// the launch itself, for vface_png_inflate_parallel's flagged files too (the caller has checked the arguments)
int vf_launch_png_inflate(const uint8_t* streams, int64_t stream_bytes, const int64_t* offsets, const int32_t* lengths, int files, uint8_t* rows,
                          int64_t file_stride, int64_t expect, int32_t* status, int32_t* produced, int32_t* consumed, uint32_t* adler,
                          const int* flags, hipStream_t stream) {
    hipLaunchKernelGGL(png_inflate_kernel, dim3(vf_grid(files, 1, kInflateGridCap)), dim3(64), 0, stream, streams, (long)stream_bytes,
                       (const long*)offsets, lengths, files, rows, (long)file_stride, (long)expect, status, produced, consumed, adler, flags);
    return vf_launched();
}

extern "C" int vface_png_inflate(const uint8_t* streams, int64_t stream_bytes, const int64_t* offsets, const int32_t* lengths, int files,
                                 uint8_t* rows, int64_t file_stride, int64_t expect, int32_t* status, int32_t* produced, int32_t* consumed,
                                 uint32_t* adler, void* stream_) {
    hipStream_t stream = vf_stream(stream_);
    if (!streams || !offsets || !lengths || !rows || !status || !produced || !consumed || !adler || files <= 0 || stream_bytes <= 0 ||
        expect <= 0)
        return VF_ERR_ARG;
    if (expect >= (1L << 31) || stream_bytes >= (1L << 31) || file_stride < expect) return VF_ERR_SHAPE;
    return vf_launch_png_inflate(streams, stream_bytes, offsets, lengths, files, rows, file_stride, expect, status, produced, consumed, adler,
                                 nullptr, stream);
}

// ---- unfilter ---------------------------------------------------------------------------------------------------------------------
namespace {

__device__ inline int paeth(int a, int b, int c) {
    const int p = a + b - c, pa = abs(p - a), pb = abs(p - b), pc = abs(p - c);
    return (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);       // ties go a, b, c
}

// One workgroup of one wave per file (the walk below is written for ONE wave: __launch_bounds__(64)).  A band is 64 rows, lane r
// on row y0 + r; at step t the lane is on pixel t - r.  Its left pixel is its own last one; up is the last pixel of lane r - 1 (one
// cross-lane move per step) and up-left the one it was handed the step before.  Lane 0 takes up from the row lane 63 left in LDS
// when it walked the band above.  Every lane loads its own row's bytes and stores its own pixels straight to global memory: the walk
// is bound by latency, not by bandwidth, and staging the rows through LDS tiles measured twice as slow.  A pixel is 3 bytes
// in one word: alpha is never looked at (the filters work channel by channel), grey is one channel replicated on the way out.
template <int BPP>
__global__ __launch_bounds__(64) void png_unfilter_kernel(const unsigned char* __restrict__ rows, long file_stride, int W, int H, int files,
                                                          const int* __restrict__ inflate_status, unsigned char* __restrict__ rgb,
                                                          int* __restrict__ status) {
    constexpr int CH = BPP == 1 ? 1 : 3;                        // channels that are undone
    __shared__ unsigned carry[kUnfilterMaxW];
    const int lane = threadIdx.x;
    const long row_bytes = 1 + (long)BPP * W, frame_bytes = (long)H * W * 3;

    for (long f = blockIdx.x; f < files; f += gridDim.x) {
        const unsigned char* src = rows + f * file_stride;
        unsigned char* dst = rgb + f * frame_bytes;
        const bool skip = inflate_status[f] != 0;
        int bad = H;                                            // the first row whose filter byte is above 4
        if (!skip)
            for (int y = lane; y < H; y += 64)
                if (src[y * row_bytes] > 4) { bad = y; break; }
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) bad = min(bad, __shfl_xor(bad, d));
        if (lane == 0) status[f] = bad < H ? 1 + bad : 0;
        if (skip || bad < H) {                                  // a file that is not decoded is cleared
            for (long i = lane; i < frame_bytes; i += 64) dst[i] = 0;
            continue;
        }
        for (int y0 = 0; y0 < H; y0 += 64) {
            const int row = y0 + lane;
            const unsigned char* in = src + (row < H ? row : 0) * row_bytes;     // (a lane past the last row reads nothing)
            unsigned char* out = dst + (long)(row < H ? row : 0) * W * 3;
            const int ft = row < H ? in[0] : 0;
            unsigned left = 0, upleft = 0, mine = 0;            // packed pixels: this row's last, the row above's last but one, this row's last
            __syncthreads();                                    // the row the band above left in `carry`
            for (int t = 0; t < W + 63; ++t) {
                const int x = t - lane;
                unsigned up = __shfl_up(mine, 1);
                const bool on = row < H && x >= 0 && x < W;
                if (lane == 0) up = (on && y0 > 0) ? carry[x] : 0u;
                if (on) {
                    if (x == 0) { left = 0; upleft = 0; }
                    unsigned pix = 0;
#pragma unroll
                    for (int c = 0; c < CH; ++c) {
                        const int raw = in[1 + (long)x * BPP + c];
                        const int a = (left >> (8 * c)) & 255, b = (up >> (8 * c)) & 255, cc = (upleft >> (8 * c)) & 255;
                        const int pred = ft == 0 ? 0 : ft == 1 ? a : ft == 2 ? b : ft == 3 ? (a + b) >> 1 : paeth(a, b, cc);
                        const unsigned v = (unsigned)(raw + pred) & 255u;
                        pix |= v << (8 * c);
                        out[(long)x * 3 + c] = (unsigned char)v;
                    }
                    if (CH == 1) {
                        out[(long)x * 3 + 1] = (unsigned char)pix;
                        out[(long)x * 3 + 2] = (unsigned char)pix;
                    }
                    if (lane == 63) carry[x] = pix;
                    left = pix;
                    upleft = up;
                    mine = pix;
                }
            }
        }
        __syncthreads();
    }
}

}  // namespace

extern "C" int vface_png_unfilter(const uint8_t* rows, int64_t file_stride, int W, int H, int bpp, int files, const int32_t* inflate_status,
                                  uint8_t* rgb, int32_t* status, void* stream_) {
    hipStream_t stream = vf_stream(stream_);
    if (!rows || !inflate_status || !rgb || !status || W <= 0 || H <= 0 || files <= 0) return VF_ERR_ARG;
    if (bpp != 1 && bpp != 3 && bpp != 4) return VF_ERR_SHAPE;
    const long frame = (1 + (long)bpp * W) * H;
    if (frame >= (1L << 31) || file_stride < frame || W > kUnfilterMaxW) return VF_ERR_SHAPE;
    const dim3 grid(vf_grid(files, 1, kUnfilterGridCap)), block(64);
    if (bpp == 1) hipLaunchKernelGGL(png_unfilter_kernel<1>, grid, block, 0, stream, rows, (long)file_stride, W, H, files, inflate_status, rgb, status);
    else if (bpp == 3) hipLaunchKernelGGL(png_unfilter_kernel<3>, grid, block, 0, stream, rows, (long)file_stride, W, H, files, inflate_status, rgb, status);
    else hipLaunchKernelGGL(png_unfilter_kernel<4>, grid, block, 0, stream, rows, (long)file_stride, W, H, files, inflate_status, rgb, status);
    return vf_launched();
}
