// PNG frames out (REFace/scripts/VFace_inference_batch.py:636: one PNG per pasted frame): the pasted 8-bit RGB frames -> the body of
// a zlib stream per frame, on the frames where they already are.  scripts/png.py adds 78 01, the Adler-32 (combined from the
// per-stripe partials), the chunk framing and the CRC; the host receives the compressed bytes and O(stripes) scalars only.
//
// Two entry points, each beside its kernels:
//   vface_png_filter    every row's filter type by the minimum sum of absolute values, its filter byte and filtered bytes
//   vface_png_deflate   a zlib-body compressor for row buffers of ANY bytes: stripes of rows, each one dynamic-Huffman block of
//                       literals and distance-1 matches (zlib's Z_RLE token set) closed by an empty stored block, or stored blocks
//                       where that is not smaller; then compaction of a frame's stripes
// The format is stated once, in tests/png_model.py; these kernels equal it byte for byte.  The code-length construction and the
// layout of the header's code-length sequence are csrc/png_huffman.hpp, which a host program runs under sanitizers.
#include "common.hpp"
#include "launch.hpp"
#include "png_huffman.hpp"
#include "vface_kernels.hpp"

namespace {

constexpr int kPngFilterGridCap = 2048;   // workgroups of 4 rows (one per wave) before the grid loops (tests/test_png_gpu.py)
constexpr int kPngDeflateGridCap = 4096;  // workgroups, one (frame, stripe) each, before the grid loops
constexpr int kStoredMax = 65535;
constexpr unsigned kAdler = 65521u;
constexpr int kChunk = 256;               // positions of a stripe a workgroup walks per step: one per thread
constexpr int kRing = 16;                 // 64-bit words of run-start flags kept: four chunks, the current one and 2 ahead (a match looks 258 ahead)
// the bit window: the open byte (< 8 bits), then the header (kPngMaxHeaderBits) or a chunk's tokens (256 x (15 + 5 + 1)), then the
// end of block (15), the sync (3 + 7 + 32)
constexpr int kWinWords = 192;
static_assert(kWinWords * 32 >= 8 + kChunk * 21 + 15 + 42 && kWinWords * 32 >= 8 + kPngMaxHeaderBits, "window");

__device__ inline int abs_signed_byte(int v) { return v < 128 ? v : 256 - v; }

// the five filtered bytes of one byte: x, a = left, b = up, c = up left
__device__ inline void png_filtered(int x, int a, int b, int c, int (&f)[5]) {
    const int p = a + b - c, pa = abs(p - a), pb = abs(p - b), pc = abs(p - c);
    const int paeth = (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
    f[0] = x; f[1] = (x - a) & 255; f[2] = (x - b) & 255; f[3] = (x - ((a + b) >> 1)) & 255; f[4] = (x - paeth) & 255;
}

// rgb [frames * H][W][3] -> rows [frames * H][1 + 3 W].  One wave per row: the five candidate sums in one pass over the row and the
// row above (zeros above a frame's first row), a wave reduction, then the chosen filter in a second pass (the reads hit in cache).
__global__ __launch_bounds__(256) void png_filter_kernel(const unsigned char* __restrict__ rgb, int W, int H, long nrows, long groups,
                                                         unsigned char* __restrict__ rows) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int rb = 3 * W;
    for (long g = blockIdx.x; g < groups; g += gridDim.x) {
        const long r = g * 4 + wave;
        if (r >= nrows) continue;
        const bool top = (r % H) == 0;
        const unsigned char* cur = rgb + r * (long)rb;
        const unsigned char* up = top ? cur : cur - rb;   // read only where !top
        unsigned sum[5] = {0, 0, 0, 0, 0};
        for (int i = lane; i < rb; i += 64) {
            const int x = cur[i], a = i >= 3 ? cur[i - 3] : 0, b = top ? 0 : up[i], c = (top || i < 3) ? 0 : up[i - 3];
            int f[5];
            png_filtered(x, a, b, c, f);
#pragma unroll
            for (int t = 0; t < 5; ++t) sum[t] += (unsigned)abs_signed_byte(f[t]);
        }
#pragma unroll
        for (int t = 0; t < 5; ++t)
#pragma unroll
            for (int d = 32; d >= 1; d >>= 1) sum[t] += __shfl_xor(sum[t], d);
        int best = 0;
        unsigned least = sum[0];
#pragma unroll
        for (int t = 1; t < 5; ++t)
            if (sum[t] < least) { least = sum[t]; best = t; }     // a tie keeps the lower type
        unsigned char* out = rows + r * (long)(rb + 1);
        if (lane == 0) out[0] = (unsigned char)best;
        for (int i = lane; i < rb; i += 64) {
            const int x = cur[i], a = i >= 3 ? cur[i - 3] : 0, b = top ? 0 : up[i], c = (top || i < 3) ? 0 : up[i - 3];
            int f[5];
            png_filtered(x, a, b, c, f);
            out[1 + i] = (unsigned char)(best == 0 ? f[0] : best == 1 ? f[1] : best == 2 ? f[2] : best == 3 ? f[3] : f[4]);
        }
    }
}

}  // namespace

extern "C" int vface_png_filter(const uint8_t* rgb, int W, int H, int frames, uint8_t* rows, void* stream_) {
    hipStream_t stream = vf_stream(stream_);
    if (!rgb || !rows || W <= 0 || H <= 0 || frames <= 0) return VF_ERR_ARG;
    if (W > (1 << 22) || (long)(3 * (long)W + 1) * H >= (1L << 31)) return VF_ERR_SHAPE;      // a row's sums fit 32 bits; a frame's rows fit vface_png_deflate
    const long nrows = (long)frames * H, groups = (nrows + 3) / 4;
    hipLaunchKernelGGL(png_filter_kernel, dim3(vf_grid(groups, 1, kPngFilterGridCap)), dim3(256), 0, stream, rgb, W, H, nrows, groups, rows);
    return vf_launched();
}

// ---- deflate -----------------------------------------------------------------------------------------------------------------------
namespace {

// the order in which a dynamic header carries the lengths of the code-length code (RFC 1951 3.2.7)
__device__ const unsigned char kHclenOrder[kPngCodeLen] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};

template <typename T>
__device__ inline T wave_inclusive_scan(T x, int lane) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const T y = __shfl_up(x, d);
        if (lane >= d) x += y;
    }
    return x;
}

__host__ __device__ inline long stored_bytes(long n) { return n + 5 * ((n + kStoredMax - 1) / kStoredMax); }

// The four routines below decide the tokens.  They are plain integer code, __host__ as well as __device__, so that a host program can
// walk a buffer exactly as the kernel does.
// flag(q): a run of equal bytes starts at q -- also at 0 and at every q >= n, so that the stripe's end closes the last run
__host__ __device__ inline bool run_starts(const unsigned char* src, long q, long n) { return q == 0 || q >= n || src[q] != src[q - 1]; }

// distance from p to the next run start behind it, capped at 258; flags[g & 15] holds the flags of positions 64 g .. 64 g + 63
__host__ __device__ inline int next_start(const unsigned long long* flags, long p) {
    const long q = p + 1, g = q >> 6;
    const int bit = (int)(q & 63);
    unsigned long long w = flags[g & (kRing - 1)] >> bit;
    if (w) return 1 + (int)__builtin_ctzll(w) < 258 ? 1 + (int)__builtin_ctzll(w) : 258;
    int d = 65 - bit;
    for (int i = 1; i <= 5 && d <= 258; ++i, d += 64) {
        w = flags[(g + i) & (kRing - 1)];
        if (w) return d + (int)__builtin_ctzll(w) < 258 ? d + (int)__builtin_ctzll(w) : 258;
    }
    return 258;
}

// the last run start at or before p, looking no further back than the chunk's first word g0; `before` = the one before the chunk
__host__ __device__ inline long last_start(const unsigned long long* flags, long p, long g0, long before) {
    long g = p >> 6;
    unsigned long long w = flags[g & (kRing - 1)] & (~0ull >> (63 - (int)(p & 63)));
    while (!w && g > g0) { --g; w = flags[g & (kRing - 1)]; }
    return w ? g * 64 + 63 - __builtin_clzll(w) : before;
}

// The token that STARTS at position p of the stripe, if one does: a run's first byte is a literal; the rest of the run is cut into
// matches of 258 from its second byte on; what is left behind the last whole one is a match if it is 3 or more, literals if 1 or 2.
// -> symbol (0 .. 285) or -1; for a match, `extra` = its extra bits' value and `ebits` their count.
__host__ __device__ inline int token_at(int byte, long p, long start, int ahead, int& extra, int& ebits) {
    extra = 0; ebits = 0;
    const long o = p - start;
    if (o == 0) return byte;
    const int r = (int)((o - 1) % 258);
    const int mlen = r + ahead < 258 ? r + ahead : 258;   // of the match that starts r bytes back
    if (mlen < 3) return byte;
    if (r != 0) return -1;
    const int idx = vf_png_len_index(mlen);
    extra = mlen - vf_png_len_base(idx);
    ebits = vf_png_len_extra(idx);
    return 257 + idx;
}

struct Walk {               // a thread's place in the walk over a stripe, one chunk per step
    long start;             // the last run start before the current chunk
    int b0, b1, b2;         // its byte in the current chunk and the two ahead
};

// the flags of chunk c (positions 256 c ..), one 64-bit word per wave, and the thread's byte there
__device__ inline int stage_chunk(const unsigned char* src, long n, long c, unsigned long long* flags, int wave, int lane) {
    const long q = c * kChunk + threadIdx.x;
    const unsigned long long w = __ballot(run_starts(src, q, n));
    if (lane == 0) flags[(c * 4 + wave) & (kRing - 1)] = w;
    return q < n ? src[q] : 0;
}

// One workgroup per (frame, stripe).  Pass 1 walks the stripe, counts the tokens' symbols in LDS and sums Adler-32's two halves.
// The 286 counts are ranked by one lane each, one lane builds the code lengths, the canonical codes and the header
// (png_huffman.hpp).  If the dynamic block with its sync is smaller than the stored form, pass 2 walks the stripe again (the
// bytes come from L2), places every token's bits by a prefix sum of the bit lengths and merges them into the LDS window with
// atomic OR -- LSB first: bit P of the stream is bit P & 31 of word P >> 5 -- and the window's whole bytes go to the stripe's slot
// after every chunk.  Otherwise the stripe is copied into stored blocks.
__global__ __launch_bounds__(256) void png_deflate_kernel(const unsigned char* __restrict__ rows, int row_bytes, int H, int stripe_rows,
                                                          int nstripes, long total, unsigned char* __restrict__ slots, long slot_bytes,
                                                          int* __restrict__ lens, unsigned* __restrict__ adler) {
    __shared__ unsigned hist[kPngMaxSyms];
    __shared__ VfPngHuffScratch scratch;
    __shared__ unsigned char len[kPngMaxSyms];          // lit/len lengths, then the distance code's at [286]
    __shared__ unsigned short code[kPngMaxSyms];
    __shared__ unsigned short cl_syms[kPngMaxSyms];
    __shared__ unsigned cl_count[kPngCodeLen];
    __shared__ unsigned char cl_len[kPngCodeLen];
    __shared__ unsigned short cl_code[kPngCodeLen];
    __shared__ unsigned long long flags[kRing];
    __shared__ unsigned win[kWinWords];
    __shared__ unsigned wsum[4];
    __shared__ unsigned sums[2];
    __shared__ unsigned long long token_bits;
    __shared__ int used, header_bits, window_bits;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;

    for (long iv = blockIdx.x; iv < total; iv += gridDim.x) {
        const long f = iv / nstripes;
        const int si = (int)(iv - f * nstripes);
        const int r0 = si * stripe_rows;
        const long n = (long)min(stripe_rows, H - r0) * row_bytes;
        const unsigned char* src = rows + (f * H + r0) * (long)row_bytes;
        unsigned char* dst = slots + iv * slot_bytes;
        const long chunks = (n + kChunk - 1) / kChunk;

        for (int i = tid; i < kPngMaxSyms; i += 256) hist[i] = i == 256 ? 1u : 0u;
        for (int i = tid; i < kWinWords; i += 256) win[i] = 0;
        if (tid == 0) { sums[0] = 0; sums[1] = 0; token_bits = 0; used = 0; }
        __syncthreads();

        // ---- pass 1: the histogram and the checksum
        Walk w;
        w.start = 0;
        w.b0 = stage_chunk(src, n, 0, flags, wave, lane);
        w.b1 = stage_chunk(src, n, 1, flags, wave, lane);
        unsigned long long a1 = 0, a2 = 0;
        for (long c = 0; c < chunks; ++c) {
            w.b2 = stage_chunk(src, n, c + 2, flags, wave, lane);
            __syncthreads();
            const long p = c * kChunk + tid;
            if (p < n) {
                int extra, ebits;
                const int sym = token_at(w.b0, p, last_start(flags, p, c * 4, w.start), next_start(flags, p), extra, ebits);
                if (sym >= 0) atomicAdd(&hist[sym], 1u);
                a1 += (unsigned)w.b0;
                a2 += (unsigned long long)(n - p) * (unsigned)w.b0;
            }
            w.start = last_start(flags, c * kChunk + kChunk - 1, c * 4, w.start);
            w.b0 = w.b1; w.b1 = w.b2;
        }
        atomicAdd(&sums[0], (unsigned)(a1 % kAdler));
        atomicAdd(&sums[1], (unsigned)(a2 % kAdler));
        __syncthreads();
        if (tid == 0) {
            adler[iv * 2] = (1u + sums[0]) % kAdler;
            adler[iv * 2 + 1] = (unsigned)((n + sums[1]) % kAdler);
        }

        // ---- the codes
        for (int i = tid; i < kPngLitLen; i += 256)
            if (hist[i]) {
                const int r = vf_png_rank(hist, kPngLitLen, i);
                scratch.sym[r] = (unsigned short)i;
                scratch.leaf[r] = hist[i];
                atomicAdd(&used, 1);
            }
        __syncthreads();
        if (tid == 0) {
            vf_png_lengths_from_sorted(used, kPngLitLen, kPngLitLenBits, len, scratch);
            vf_png_canonical(len, kPngLitLen, code, scratch);
            len[kPngLitLen] = 1;                            // one distance code: it takes one bit
            const int m = vf_png_code_length_symbols(len, kPngSeq, cl_syms);
            for (int i = 0; i < kPngCodeLen; ++i) cl_count[i] = 0;
            for (int i = 0; i < m; ++i) ++cl_count[cl_syms[i] & 255];
            vf_png_huffman(cl_count, kPngCodeLen, kPngCodeLenBits, cl_len, cl_code, scratch);
            // the header into the window: BFINAL 0, BTYPE 2, HLIT, HDIST, HCLEN, the code-length code in the permuted order, the lengths
            int pos = 0;
            auto put = [&](unsigned v, int nb) {
                if (nb == 0) return;
                const int o = pos & 31, at = pos >> 5;
                win[at] |= v << o;
                if (o + nb > 32) win[at + 1] |= v >> (32 - o);
                pos += nb;
            };
            int hclen = kPngCodeLen;
            while (hclen > 4 && cl_len[kHclenOrder[hclen - 1]] == 0) --hclen;
            put(0, 1); put(2, 2); put(kPngLitLen - 257, 5); put(0, 5); put((unsigned)(hclen - 4), 4);
            for (int i = 0; i < hclen; ++i) put(cl_len[kHclenOrder[i]], 3);
            for (int i = 0; i < m; ++i) {
                const int s = cl_syms[i] & 255;
                put(cl_code[s], cl_len[s]);
                if (s == 17) put((unsigned)(cl_syms[i] >> 8), 3);
                if (s == 18) put((unsigned)(cl_syms[i] >> 8), 7);
            }
            header_bits = pos;
        }
        __syncthreads();
        for (int i = tid; i < kPngLitLen; i += 256)
            if (hist[i]) {
                const int xb = i > 256 ? vf_png_len_extra(i - 257) + 1 : 0;     // a match's extra bits and its one distance bit
                atomicAdd(&token_bits, (unsigned long long)hist[i] * (unsigned)(len[i] + xb));
            }
        __syncthreads();
        // the dynamic form: the block, then 3 bits of an empty stored block, padding to the byte, 00 00 FF FF
        const long dynamic = (long)((header_bits + token_bits + 3 + 7) >> 3) + 4;
        const long stored = stored_bytes(n);

        if (dynamic >= stored) {
            // ---- stored blocks: BFINAL 0, BTYPE 00 in a byte of their own, LEN, NLEN, the bytes
            const long blocks = (n + kStoredMax - 1) / kStoredMax;
            for (long b = tid; b < blocks; b += 256) {
                const unsigned l = (unsigned)min((long)kStoredMax, n - b * kStoredMax);
                unsigned char* h = dst + b * (kStoredMax + 5);
                h[0] = 0; h[1] = (unsigned char)(l & 255); h[2] = (unsigned char)(l >> 8);
                h[3] = (unsigned char)(~l & 255); h[4] = (unsigned char)((~l >> 8) & 255);
            }
            for (long i = tid; i < n; i += 256) dst[i + 5 * (i / kStoredMax + 1)] = src[i];
            if (tid == 0) lens[iv] = (int)stored;
            __syncthreads();
            continue;
        }

        // ---- pass 2: the bits
        long written = 0;
        unsigned carry = 0;                 // bits of the open byte at the front of the window
        // the window's whole bytes leave for the slot; the open byte moves to the front
        auto flush = [&](unsigned wbits) {
            const int nbytes = (int)(wbits >> 3);
            const unsigned tail = (win[nbytes >> 2] >> (8 * (nbytes & 3))) & 255u;
            for (int j = tid; j < nbytes; j += 256)
                if (written + j < slot_bytes) dst[written + j] = (unsigned char)((win[j >> 2] >> (8 * (j & 3))) & 255u);
            __syncthreads();
            for (int j = tid; j < kWinWords; j += 256) win[j] = j == 0 ? tail : 0u;
            __syncthreads();
            written += nbytes;
            carry = wbits & 7;
        };
        flush((unsigned)header_bits);
        w.start = 0;
        w.b0 = stage_chunk(src, n, 0, flags, wave, lane);
        w.b1 = stage_chunk(src, n, 1, flags, wave, lane);
        for (long c = 0; c < chunks; ++c) {
            w.b2 = stage_chunk(src, n, c + 2, flags, wave, lane);
            __syncthreads();
            const long p = c * kChunk + tid;
            unsigned bits = 0;
            int nb = 0;
            if (p < n) {
                int extra, ebits;
                const int sym = token_at(w.b0, p, last_start(flags, p, c * 4, w.start), next_start(flags, p), extra, ebits);
                if (sym >= 0) {
                    const int l = len[sym];
                    bits = (unsigned)code[sym] | ((unsigned)extra << l);            // the distance code, one 0 bit, sits above the extra bits
                    nb = l + ebits + (sym > 256 ? 1 : 0);
                }
            }
            w.start = last_start(flags, c * kChunk + kChunk - 1, c * 4, w.start);
            w.b0 = w.b1; w.b1 = w.b2;
            const int incl = wave_inclusive_scan(nb, lane);
            if (lane == 63) wsum[wave] = (unsigned)incl;
            __syncthreads();
            unsigned before = 0, all = 0;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (k < wave) before += wsum[k];
                all += wsum[k];
            }
            if (nb > 0) {
                const unsigned P = carry + before + (unsigned)(incl - nb);
                const unsigned o = P & 31, at = P >> 5;
                const unsigned long long v = (unsigned long long)bits << o;
                if (at < kWinWords) atomicOr(&win[at], (unsigned)v);
                if ((v >> 32) && at + 1 < kWinWords) atomicOr(&win[at + 1], (unsigned)(v >> 32));
            }
            __syncthreads();
            flush(carry + all);
        }
        // the end of block, the empty stored block that byte-aligns the stripe
        if (tid == 0) {
            unsigned pos = carry;
            const unsigned long long v = (unsigned long long)code[256] << pos;      // carry < 8, the code has at most 15 bits
            win[0] |= (unsigned)v;
            pos += len[256] + 3;
            pos = (pos + 7) & ~7u;
            win[pos >> 5] |= 0xFFFF0000u << (pos & 31);
            if (pos & 31) win[(pos >> 5) + 1] |= 0xFFFF0000u >> (32 - (pos & 31));
            window_bits = (int)(pos + 32);
        }
        __syncthreads();
        flush((unsigned)window_bits);
        if (tid == 0) lens[iv] = (int)min(written, slot_bytes);
        __syncthreads();
    }
}

// offs[i] = where stripe i starts in the packed output: the exclusive prefix sum of (length + 2 for the final 03 00 behind a
// frame's last stripe) over all stripes of all frames; offs[total] = the end.  One workgroup.
__global__ __launch_bounds__(256) void png_offsets_kernel(const int* __restrict__ lens, long* __restrict__ offs, long total, int nstripes) {
    __shared__ long long wsum[4];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    long long base = 0;
    for (long s = 0; s < total; s += 256) {
        const long i = s + tid;
        const long long v = i < total ? lens[i] + ((int)(i % nstripes) == nstripes - 1 ? 2 : 0) : 0;
        const long long incl = wave_inclusive_scan(v, lane);
        if (lane == 63) wsum[wave] = incl;
        __syncthreads();
        long long before = 0, all = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (k < wave) before += wsum[k];
            all += wsum[k];
        }
        if (i < total) offs[i] = base + before + (incl - v);
        base += all;
        __syncthreads();
    }
    if (tid == 0) offs[total] = base;
}

// copies every stripe from its slot to its place (every stripe is whole bytes: a byte copy), 03 00 -- an empty final fixed block --
// behind a frame's last, and writes each frame's offset and byte count.  Bytes that would land past `out_bytes` are dropped.
__global__ __launch_bounds__(256) void png_pack_kernel(const unsigned char* __restrict__ slots, long slot_bytes, const int* __restrict__ lens,
                                                       const long* __restrict__ offs, long total, int nstripes, unsigned char* __restrict__ out,
                                                       long out_bytes, long* __restrict__ offsets, int* __restrict__ lengths) {
    for (long iv = blockIdx.x; iv < total; iv += gridDim.x) {
        const unsigned char* src = slots + iv * slot_bytes;
        const long o = offs[iv];
        const int n = lens[iv], i = (int)(iv % nstripes);
        for (int j = threadIdx.x; j < n; j += 256)
            if (o + j < out_bytes) out[o + j] = src[j];
        if (threadIdx.x == 0 && i == nstripes - 1) {
            if (o + n < out_bytes) out[o + n] = 0x03;
            if (o + n + 1 < out_bytes) out[o + n + 1] = 0x00;
            offsets[iv / nstripes] = offs[iv - i];
            lengths[iv / nstripes] = (int)(o + n + 2 - offs[iv - i]);
        }
    }
}

inline size_t align16(size_t n) { return (n + 15) & ~(size_t)15; }

}  // namespace

extern "C" int64_t vface_png_deflate_bound(int row_bytes, int rows, int stripe_rows) {
    if (row_bytes <= 0 || rows <= 0 || stripe_rows <= 0) return 0;
    const long full = rows / stripe_rows, last = rows % stripe_rows;
    return full * stored_bytes((long)stripe_rows * row_bytes) + (last ? stored_bytes(last * row_bytes) : 0) + 2;
}

extern "C" size_t vface_png_deflate_workspace_bytes(int row_bytes, int H, int frames, int stripe_rows) {
    if (row_bytes <= 0 || H <= 0 || frames <= 0 || stripe_rows <= 0) return 0;
    const size_t nstripes = ((size_t)H + stripe_rows - 1) / stripe_rows, total = nstripes * frames;
    const size_t slot = (size_t)stored_bytes((long)std::min(stripe_rows, H) * row_bytes);
    return align16(total * sizeof(int)) + align16((total + 1) * sizeof(long)) + total * slot;
}

extern "C" int vface_png_deflate(const uint8_t* rows, int row_bytes, int H, int frames, int stripe_rows, uint8_t* out, int64_t out_bytes,
                                 int64_t* offsets, int32_t* lengths, uint32_t* adler, void* workspace, size_t workspace_bytes,
                                 void* stream_) {
    hipStream_t stream = vf_stream(stream_);
    if (!rows || !out || !offsets || !lengths || !adler || !workspace || row_bytes <= 0 || H <= 0 || frames <= 0 || stripe_rows <= 0 ||
        out_bytes <= 0)
        return VF_ERR_ARG;
    if ((long)row_bytes * H >= (1L << 31) || vface_png_deflate_bound(row_bytes, H, stripe_rows) >= (1L << 31)) return VF_ERR_SHAPE;
    if (workspace_bytes < vface_png_deflate_workspace_bytes(row_bytes, H, frames, stripe_rows)) return VF_ERR_SHAPE;
    if (((size_t)workspace & 15) != 0) return VF_ERR_ALIGN;
    const long nstripes = ((long)H + stripe_rows - 1) / stripe_rows, total = nstripes * frames;
    const long slot = stored_bytes((long)std::min(stripe_rows, H) * row_bytes);
    int* lens = (int*)workspace;
    long* offs = (long*)((char*)workspace + align16(total * sizeof(int)));
    unsigned char* slots = (unsigned char*)offs + align16((total + 1) * sizeof(long));
    hipLaunchKernelGGL(png_deflate_kernel, dim3(vf_grid(total, 1, kPngDeflateGridCap)), dim3(256), 0, stream, rows, row_bytes, H, stripe_rows,
                       (int)nstripes, total, slots, slot, lens, adler);
    hipLaunchKernelGGL(png_offsets_kernel, dim3(1), dim3(256), 0, stream, (const int*)lens, offs, total, (int)nstripes);
    hipLaunchKernelGGL(png_pack_kernel, dim3(vf_grid(total, 1, kPngDeflateGridCap)), dim3(256), 0, stream, (const unsigned char*)slots, slot,
                       (const int*)lens, (const long*)offs, total, (int)nstripes, out, (long)out_bytes, (long*)offsets, lengths);
    return vf_launched();
}
