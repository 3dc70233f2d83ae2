// PNG frames in, inflate of ONE stream on many waves (the follow-up csrc/png_in.hip names): zlib starts a new deflate block every
// lit_bufsize tokens, a block can be decoded without its predecessors but for where it starts and the 32 KiB of output in front of
// it, and both can be supplied afterwards (the algorithm of pugz and rapidgzip).  The protocol -- find, count, validate, place,
// write, resolve, fall back -- is stated in csrc/png_inflate_par.hpp and tests/png_inflate_par_model.py; the kernels below equal the
// model in the candidate list, in which files fall back and why, and in everything vface_png_inflate returns.
//
// Six launches, always: find (one wave per chunk: every lane puts the 8 bit positions of its byte to the cheap test in registers, the
// survivors get the wave-wide header parse, smallest position first), count (one wave per segment, no window at all), validate +
// place (one wave per file: reductions and a prefix sum over its segments), write (one wave per segment into the 16-bit plane; its own
// earlier output is read from a 16-bit ring of 32 768 elements in LDS that starts out as the markers themselves, so a match copies
// elements without asking where its source lies), resolve (one workgroup per file, segments in order) and png_inflate_kernel on the
// flagged files (csrc/png_in.hip: status and partial output of such a file are vface_png_inflate's by construction).
// Everything that file bytes steer and that indexes memory is csrc/png_inflate_par.hpp and csrc/png_inflate.hpp, which host programs
// run under sanitizers.
#include "common.hpp"
#include "launch.hpp"
#include "png_inflate_par.hpp"
#include "vface_kernels.hpp"

namespace {

constexpr int kFindGridCap = 2048, kCountGridCap = 2048, kWriteGridCap = 1024, kValidateGridCap = 1024, kResolveGridCap = 256;
constexpr int kResolveThreads = 1024;
constexpr int kRingMask = kInfWindow - 1;
constexpr int kFlushElements = 4096;      // the ring's new elements leave for the plane once there are this many
constexpr int kInChunk = 256, kInWindow = 512;
constexpr long kAdlerPiece = 1L << 20;    // elements summed before the halves are folded: (2^20)^2 * 255 stays far inside 64 bits

// The stream of one file behind VfInfBits, as csrc/png_in.hip's: bytes [loaded - 512, loaded) stand in `win` at their position mod
// 512, loaded chunk by chunk by the whole wave.  seek() starts the window over at the chunk that holds pos; raw() is the byte in
// global memory (asked only for pos < end: csrc/png_inflate_par.hpp).
struct ParStream {
    const unsigned char* bytes;
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
    __device__ void seek(long pos) { loaded = pos & ~(long)(kInChunk - 1); }
    __device__ unsigned at(long pos) const { return win[pos & (kInWindow - 1)]; }
    __device__ unsigned raw(long pos) const { return bytes[pos]; }
};

// a 64-bit value every lane holds alike, said so to the compiler
__device__ inline long uniform64(long x) {
    const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)x), hi = __builtin_amdgcn_readfirstlane((unsigned)((unsigned long)x >> 32));
    return (long)(((unsigned long)hi << 32) | lo);
}
__device__ inline bool range_inside(long off, long n, long stream_bytes) { return !(off < 0 || n < 0 || off > stream_bytes || n > stream_bytes - off); }

// ---- find: slot (f, c) <- the bit at which chunk c of file f starts a segment, or -1.  One wave per slot (the table builds of
// csrc/png_inflate.hpp are written for exactly one wave in lockstep).
__global__ __launch_bounds__(64) void png_par_find_kernel(const unsigned char* __restrict__ streams, long stream_bytes, const long* __restrict__ offsets,
                                                          const int* __restrict__ lengths, int files, int chunk_bytes, long maxc,
                                                          long* __restrict__ cand) {
    __shared__ VfInfTables tb;
    __shared__ unsigned char win[kInWindow];
    const int lane = threadIdx.x;
    for (long slot = blockIdx.x; slot < files * maxc; slot += gridDim.x) {
        const long f = slot / maxc, c = slot % maxc;
        const long off = offsets[f], n = lengths[f];
        long found = -1;
        if (range_inside(off, n, stream_bytes) && c < vf_inf_par_chunks(n, chunk_bytes)) {
            if (c == 0) {
                found = 0;
            } else {
                const ParStream src = {streams + off, win, 0, n, lane};
                const long hi = (c + 1) * chunk_bytes < n ? (c + 1) * chunk_bytes : n;
                for (long base = c * chunk_bytes; base < hi && found < 0; base += 64) {
                    const unsigned mask = base + lane < hi ? vf_inf_par_quick8(src, n, base + lane) : 0u;
                    unsigned long long any = __ballot(mask != 0u);
                    while (any && found < 0) {                              // lanes in order, a lane's bits in order: the smallest position first
                        const int l = __ffsll((long long)any) - 1;
                        any &= any - 1;
                        unsigned m = (unsigned)__builtin_amdgcn_readfirstlane((int)__shfl(mask, l));
                        while (m && found < 0) {
                            const long p = 8 * (base + l) + (__ffs((int)m) - 1);
                            m &= m - 1;
                            if (vf_inf_par_passes(src, n, p, tb, lane, 64)) found = p;
                        }
                    }
                }
            }
        }
        if (lane == 0) cand[slot] = found;
        __syncthreads();
    }
}

// the start of the next segment of file f behind chunk c, or -1
__device__ inline long next_start(const long* cand, long f, long c, long chunks, long maxc, int lane) {
    long next = -1;
    for (long base = c + 1; base < chunks && next < 0; base += 64) {
        const long v = base + lane < chunks ? cand[f * maxc + base + lane] : -1;
        const unsigned long long any = __ballot(v >= 0);
        if (any) next = __shfl(v, __ffsll((long long)any) - 1);
    }
    return uniform64(next);
}

// ---- count: one wave per segment decodes from its start until a block ends at or behind the next segment's start, writing nothing
__global__ __launch_bounds__(64) void png_par_count_kernel(const unsigned char* __restrict__ streams, const long* __restrict__ offsets,
                                                           const int* __restrict__ lengths, int files, int chunk_bytes, long maxc,
                                                           const long* __restrict__ cand, VfInfSegment* __restrict__ segs) {
    __shared__ VfInfTables tb;
    __shared__ unsigned char win[kInWindow];
    const int lane = threadIdx.x;
    for (long slot = blockIdx.x; slot < files * maxc; slot += gridDim.x) {
        const long start = uniform64(cand[slot]);
        if (start < 0) continue;                        // (such a slot's file lies inside the buffer: find looked)
        const long f = slot / maxc, c = slot % maxc, n = lengths[f];
        const long next = next_start(cand, f, c, vf_inf_par_chunks(n, chunk_bytes), maxc, lane);
        VfInfBits<ParStream> b = vf_inf_open(ParStream{streams + offsets[f], win, 0, n, lane}, n, start);
        VfInfCountSink sink;
        VfInfSegment r;
        vf_inf_par_segment(b, next, tb, lane, 64, sink, r);
        if (lane == 0) {
            r.start = start;
            r.offset = 0;
            r.closes = r.status == VF_INF_OK && (next >= 0 ? (!r.final_seen && r.end == next) : r.final_seen);
            r.pad = 0;
            segs[slot] = r;
        }
        __syncthreads();
    }
}

template <typename T>
__device__ inline T wave_sum(T x) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) x += __shfl_xor(x, d);
    return x;
}

// ---- validate and place: one wave per file.  flags[f] = the file falls back; meta[f] = {segments, reason, candidates, 0};
// last_end[f] = the bit behind the last segment; every segment's offset = the exclusive prefix sum of the counts.
__global__ __launch_bounds__(64) void png_par_validate_kernel(long stream_bytes, const long* __restrict__ offsets, const int* __restrict__ lengths,
                                                              int files, int chunk_bytes, long maxc, long expect, const long* __restrict__ cand,
                                                              VfInfSegment* __restrict__ segs, int* __restrict__ flags, int* __restrict__ meta,
                                                              long* __restrict__ last_end) {
    const int lane = threadIdx.x;
    for (long f = blockIdx.x; f < files; f += gridDim.x) {
        const long n = lengths[f];
        int reason = VF_INF_PAR_NONE, nseg = 0;
        long end = 0;
        if (!range_inside(offsets[f], n, stream_bytes)) {
            reason = VF_INF_PAR_RANGE;
        } else {
            const long chunks = vf_inf_par_chunks(n, chunk_bytes);
            long total = 0;
            int any_status = 0, open_chain = 0;
            for (long base = 0; base < chunks; base += 64) {
                const long c = base + lane;
                const bool valid = c < chunks && cand[f * maxc + c] >= 0;
                VfInfSegment* s = segs + f * maxc + c;
                const long count = valid ? s->produced : 0;
                long incl = count;
#pragma unroll
                for (int d = 1; d < 64; d <<= 1) {
                    const long t = __shfl_up(incl, d);
                    if (lane >= d) incl += t;
                }
                if (valid) {
                    s->offset = total + incl - count;
                    any_status |= s->status != VF_INF_OK;
                    open_chain |= !s->closes;
                    end = s->end > end ? s->end : end;
                }
                total += __shfl(incl, 63);
                nseg += __popcll(__ballot(valid));
            }
#pragma unroll
            for (int d = 32; d >= 1; d >>= 1) {
                const long t = __shfl_xor(end, d);
                end = t > end ? t : end;
            }
            if (__any(any_status)) reason = VF_INF_PAR_STATUS;
            else if (__any(open_chain)) reason = VF_INF_PAR_CHAIN;
            else if (total != expect) reason = VF_INF_PAR_COUNT;
        }
        if (lane == 0) {
            flags[f] = reason != VF_INF_PAR_NONE;
            meta[4 * f] = nseg;
            meta[4 * f + 1] = reason;
            meta[4 * f + 2] = nseg > 0 ? nseg - 1 : 0;
            meta[4 * f + 3] = 0;
            last_end[f] = end;
        }
    }
}

// ---- write.  The sink of csrc/png_inflate_par.hpp's loop on one wave: literals wait in the lanes (lane k holds the k-th) and go to
// the ring 64 at a time; a match and a stored block are copied by the lanes side by side; the ring leaves for the plane in pieces.
// ring[j] starts out as 0x8000 | j: position s < 0 of the segment lies at ring[s & 32767] = ring[32768 + s], which IS its marker.
struct RingSink {
    unsigned short* ring;
    unsigned short* plane;      // the segment's first element
    long limit, offset;         // the segment's counted length; the bytes of the file in front of it
    int lane;
    long op = 0, flushed = 0;
    int npend = 0;
    unsigned mylit = 0;
    __device__ void to_plane(long upto) {
        for (long i = flushed + lane; i < upto; i += 64) plane[i] = ring[i & kRingMask];       // i < upto <= limit
        flushed = upto;
    }
    __device__ void flush() {
        if (lane < npend) ring[(op + lane) & kRingMask] = (unsigned short)mylit;
        op += npend;
        npend = 0;
        __syncthreads();
        if (op - flushed >= kFlushElements) to_plane(op);
    }
    __device__ int literal(int v) {
        if (op + npend + 1 > limit) return VF_INF_TOO_LONG;
        if (lane == npend) mylit = (unsigned)v;
        if (++npend == 64) flush();
        return VF_INF_OK;
    }
    __device__ int match(int length, int distance) {
        flush();
        if (distance > offset + op) return VF_INF_TOO_FAR;
        if (op + length > limit) return VF_INF_TOO_LONG;
        // every source element lies in front of the match (i mod distance): the lanes do not wait for one another
        for (int i = lane; i < length; i += 64) {
            const unsigned short v = ring[(op - distance + (distance >= length ? i : i % distance)) & kRingMask];
            ring[(op + i) & kRingMask] = v;
        }
        __syncthreads();
        op += length;
        if (op - flushed >= kFlushElements) to_plane(op);
        return VF_INF_OK;
    }
    __device__ int stored(const ParStream& src, long pos, int len) {
        flush();
        if (op + len > limit) return VF_INF_TOO_LONG;
        for (int done = 0; done < len;) {
            const int piece = min(len - done, kFlushElements);
            for (int i = lane; i < piece; i += 64) ring[(op + i) & kRingMask] = (unsigned short)src.raw(pos + done + i);
            __syncthreads();
            op += piece;
            done += piece;
            if (op - flushed >= kFlushElements) to_plane(op);
        }
        return VF_INF_OK;
    }
    __device__ long produced() const { return op; }
};

// One wave per segment of every file that validate accepted.  A segment whose decode does not repeat its count -- a distance in
// front of the file's first byte is the one way there is -- flags the file; `rows` is not touched here.
__global__ __launch_bounds__(64) void png_par_write_kernel(const unsigned char* __restrict__ streams, const long* __restrict__ offsets,
                                                           const int* __restrict__ lengths, int files, int chunk_bytes, long maxc, long expect,
                                                           const long* __restrict__ cand, const VfInfSegment* __restrict__ segs,
                                                           unsigned short* __restrict__ plane, int* flags, int* meta) {
    extern __shared__ __attribute__((aligned(16))) unsigned short ring[];       // kInfWindow elements
    __shared__ VfInfTables tb;
    __shared__ unsigned char win[kInWindow];
    const int lane = threadIdx.x;
    for (long slot = blockIdx.x; slot < files * maxc; slot += gridDim.x) {
        const long start = uniform64(cand[slot]);
        const long f = slot / maxc, c = slot % maxc;
        if (start < 0 || __builtin_amdgcn_readfirstlane(flags[f])) continue;
        const long n = lengths[f];
        const long next = next_start(cand, f, c, vf_inf_par_chunks(n, chunk_bytes), maxc, lane);
        const long count = uniform64(segs[slot].produced), offset = uniform64(segs[slot].offset);
        for (int j = lane; j < kInfWindow / 4; j += 64) {                       // four markers a store
            const unsigned long long m = 0x8003800280018000ull + 0x0004000400040004ull * (unsigned long long)j;
            ((unsigned long long*)ring)[j] = m;
        }
        __syncthreads();
        VfInfBits<ParStream> b = vf_inf_open(ParStream{streams + offsets[f], win, 0, n, lane}, n, start);
        // (offset + count <= expect: validate summed the counts to exactly expect)
        RingSink sink = {ring, plane + f * expect + offset, offset + count <= expect ? count : 0, offset, lane};
        VfInfSegment r;
        vf_inf_par_segment(b, next, tb, lane, 64, sink, r);
        sink.to_plane(sink.op);
        if ((r.status != VF_INF_OK || r.produced != count) && lane == 0) {
            flags[f] = 1;
            meta[4 * f] = 0;
            meta[4 * f + 1] = r.status == VF_INF_TOO_FAR ? VF_INF_PAR_FAR : VF_INF_PAR_STATUS;
        }
        __syncthreads();
    }
}

// ---- resolve: one workgroup per accepted file, its segments in order.  Every element becomes a byte of `rows`; a marker reads
// `rows` where an earlier segment of this workgroup has finished it: the barrier between two segments carries a workgroup-scope
// fence, and the waves of a workgroup share their CU's vector cache, so the bytes are there.  The Adler halves are folded piece by
// piece in stream order.  Also writes status, produced, consumed, adler and info of the accepted files and info of the others.
__global__ __launch_bounds__(kResolveThreads) void png_par_resolve_kernel(const int* __restrict__ lengths, int files, int chunk_bytes, long maxc,
                                                                         long expect, const long* __restrict__ cand,
                                                                         const VfInfSegment* __restrict__ segs,
                                                                         const unsigned short* __restrict__ plane, const int* __restrict__ flags,
                                                                         const int* __restrict__ meta, const long* __restrict__ last_end,
                                                                         unsigned char* rows, long file_stride, int* __restrict__ status_out,
                                                                         int* __restrict__ produced, int* __restrict__ consumed,
                                                                         unsigned* __restrict__ adler, int* __restrict__ info) {
    __shared__ unsigned long long red[2][kResolveThreads / 64];
    const int tid = threadIdx.x;
    for (long f = blockIdx.x; f < files; f += gridDim.x) {
        if (flags[f]) {
            if (tid == 0 && info) {
                info[4 * f] = 0;
                info[4 * f + 1] = meta[4 * f + 1];
                info[4 * f + 2] = meta[4 * f + 2];
                info[4 * f + 3] = 0;
            }
            continue;
        }
        unsigned char* out = rows + f * file_stride;
        const unsigned short* elements = plane + f * expect;
        const long chunks = vf_inf_par_chunks(lengths[f], chunk_bytes);
        unsigned s1 = 1, s2 = 0;
        for (long c = 0; c < chunks; ++c) {
            if (cand[f * maxc + c] < 0) continue;
            const long offset = segs[f * maxc + c].offset, count = segs[f * maxc + c].produced;
            for (long done = 0; done < count; done += kAdlerPiece) {
                const long L = count - done < kAdlerPiece ? count - done : kAdlerPiece;
                unsigned long long a1 = 0, a2 = 0;
#pragma unroll 4
                for (long i = tid; i < L; i += kResolveThreads) {
                    const unsigned v = vf_inf_par_resolve(elements[offset + done + i], offset, out);
                    out[offset + done + i] = (unsigned char)v;
                    a1 += v;
                    a2 += (unsigned long long)(L - i) * v;
                }
                a1 = wave_sum(a1);
                a2 = wave_sum(a2);
                if ((tid & 63) == 0) {
                    red[0][tid >> 6] = a1;
                    red[1][tid >> 6] = a2;
                }
                __syncthreads();
                a1 = 0;
                a2 = 0;
#pragma unroll
                for (int w = 0; w < kResolveThreads / 64; ++w) {
                    a1 += red[0][w];
                    a2 += red[1][w];
                }
                vf_inf_par_adler(s1, s2, a1, a2, L);
                __threadfence_block();
                __syncthreads();                        // this segment's bytes are there for the next one's markers; `red` is free again
            }
        }
        if (tid == 0) {
            status_out[f] = VF_INF_OK;
            produced[f] = (int)expect;
            consumed[f] = (int)((last_end[f] + 7) >> 3);
            adler[2 * f] = s1;
            adler[2 * f + 1] = s2;
            if (info) {
                info[4 * f] = meta[4 * f];
                info[4 * f + 1] = 0;
                info[4 * f + 2] = meta[4 * f + 2];
                info[4 * f + 3] = 0;
            }
        }
    }
}

inline size_t a16(size_t x) { return (x + 15) & ~(size_t)15; }
inline long max_chunks(int64_t stream_bytes, int chunk_bytes) { return (long)((stream_bytes + chunk_bytes - 1) / chunk_bytes); }
inline bool chunk_ok(int chunk_bytes) { return chunk_bytes >= kInfParMinChunk && chunk_bytes <= kInfParMaxChunk && chunk_bytes % 4 == 0; }

}  // namespace

extern "C" size_t vface_png_inflate_parallel_workspace_bytes(int files, int64_t stream_bytes, int64_t expect, int chunk_bytes) {
    if (files <= 0 || stream_bytes <= 0 || expect <= 0 || stream_bytes >= (1L << 31) || expect >= (1L << 31) || !chunk_ok(chunk_bytes)) return 0;
    const size_t slots = (size_t)files * (size_t)max_chunks(stream_bytes, chunk_bytes);
    return a16((size_t)files * sizeof(int)) + a16((size_t)files * 4 * sizeof(int)) + a16((size_t)files * sizeof(long)) + a16(slots * sizeof(long)) +
           a16(slots * sizeof(VfInfSegment)) + a16((size_t)files * (size_t)expect * sizeof(unsigned short));
}

extern "C" int vface_png_inflate_parallel(const uint8_t* streams, int64_t stream_bytes, const int64_t* offsets, const int32_t* lengths, int files,
                                          uint8_t* rows, int64_t file_stride, int64_t expect, int32_t* status, int32_t* produced,
                                          int32_t* consumed, uint32_t* adler, int chunk_bytes, void* workspace, size_t workspace_bytes,
                                          int32_t* info, void* stream_) {
    static VfOncePerDevice attr_set;
    hipStream_t stream = vf_stream(stream_);
    if (!streams || !offsets || !lengths || !rows || !status || !produced || !consumed || !adler || !workspace || files <= 0 ||
        stream_bytes <= 0 || expect <= 0)
        return VF_ERR_ARG;
    if (expect >= (1L << 31) || stream_bytes >= (1L << 31) || file_stride < expect || !chunk_ok(chunk_bytes)) return VF_ERR_SHAPE;
    if (workspace_bytes < vface_png_inflate_parallel_workspace_bytes(files, stream_bytes, expect, chunk_bytes)) return VF_ERR_SHAPE;
    if ((uintptr_t)workspace & 15) return VF_ERR_ALIGN;
    const long maxc = max_chunks(stream_bytes, chunk_bytes), slots = files * maxc;
    char* at = (char*)workspace;
    int* flags = (int*)at;
    at += a16((size_t)files * sizeof(int));
    int* meta = (int*)at;
    at += a16((size_t)files * 4 * sizeof(int));
    long* last_end = (long*)at;
    at += a16((size_t)files * sizeof(long));
    long* cand = (long*)at;
    at += a16((size_t)slots * sizeof(long));
    VfInfSegment* segs = (VfInfSegment*)at;
    at += a16((size_t)slots * sizeof(VfInfSegment));
    unsigned short* plane = (unsigned short*)at;
    constexpr int ring_bytes = kInfWindow * (int)sizeof(unsigned short);
    if (!attr_set.set_lds(reinterpret_cast<const void*>(png_par_write_kernel), ring_bytes)) return VF_ERR_LAUNCH;
    const long* offs = (const long*)offsets;
    hipLaunchKernelGGL(png_par_find_kernel, dim3(vf_grid(slots, 1, kFindGridCap)), dim3(64), 0, stream, streams, (long)stream_bytes, offs, lengths,
                       files, chunk_bytes, maxc, cand);
    hipLaunchKernelGGL(png_par_count_kernel, dim3(vf_grid(slots, 1, kCountGridCap)), dim3(64), 0, stream, streams, offs, lengths, files,
                       chunk_bytes, maxc, (const long*)cand, segs);
    hipLaunchKernelGGL(png_par_validate_kernel, dim3(vf_grid(files, 1, kValidateGridCap)), dim3(64), 0, stream, (long)stream_bytes, offs, lengths,
                       files, chunk_bytes, maxc, (long)expect, (const long*)cand, segs, flags, meta, last_end);
    hipLaunchKernelGGL(png_par_write_kernel, dim3(vf_grid(slots, 1, kWriteGridCap)), dim3(64), ring_bytes, stream, streams, offs, lengths, files,
                       chunk_bytes, maxc, (long)expect, (const long*)cand, (const VfInfSegment*)segs, plane, flags, meta);
    hipLaunchKernelGGL(png_par_resolve_kernel, dim3(vf_grid(files, 1, kResolveGridCap)), dim3(kResolveThreads), 0, stream, lengths, files,
                       chunk_bytes, maxc, (long)expect, (const long*)cand, (const VfInfSegment*)segs, (const unsigned short*)plane,
                       (const int*)flags, (const int*)meta, (const long*)last_end, rows, (long)file_stride, status, produced, consumed, adler, info);
    return vf_launch_png_inflate(streams, stream_bytes, offsets, lengths, files, rows, file_stride, expect, status, produced, consumed, adler,
                                 flags, stream);
}
