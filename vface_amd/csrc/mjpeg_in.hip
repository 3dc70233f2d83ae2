// Motion-JPEG half of the video intake (REFace/scripts/VFace_inference_batch.py:240-285 decodes the target video on the
// host): the scans of baseline 4:2:0 JPEG frames, as vface_amd/scripts/mjpeg_in.py cuts them out of an AVI, -> the I420 rows that
// vface_yuv420_to_rgb (csrc/demux.hip) turns into RGB frames.  The host parses headers only; the compressed bytes cross to the device.
//
// Four entry points, each beside its kernels -- the mirror image of csrc/mjpeg.hip:
//   vface_jpeg_scan_index      finds the RSTm markers of every frame's scan: the byte range of every restart interval
//   vface_jpeg_decode_entropy  Huffman decoding with the frame's own tables, one lane per interval -> the coefficient layout that
//                              vface_jpeg_coefficients writes (vface_jpeg_entropy followed by this is the identity)
//   vface_jpeg_decode_entropy_parallel  the same output from many lanes per interval: fixed-size subsequences decoded from guessed
//                              states and stitched by self-synchronisation (csrc/jpeg_subseq.hpp), for scans without restart markers
//   vface_jpeg_planes          dequantisation, 8 x 8 inverse DCT, level shift, clamp, crop -> I420 rows
//
// The interval decoder is csrc/jpeg_interval.hpp, shared with a host program that runs it under sanitizers: the bytes of a file
// steer it, and no input may take a load or a store outside the buffers (the rules stand in that file).  The other two kernels
// have data-independent addressing.
//
// The inverse DCT is integer and is stated once, in tests/jpeg_decode_model.py; vface_jpeg_planes equals it bit for bit:
//   d = clamp(q Q, -2048, 2047)                                     q the coefficient, Q its quantiser
//   C[k][n] = rint(32768 a_k cos((2n + 1) k pi / 16)),  a_0 = sqrt(1/8), a_k = 1/2
//   columns: t[m][u] = clamp((sum_v C[v][m] d[v][u] + (1 << 10)) >> 11, -16384, 16383)      (4 fraction bits)
//   rows:    p[m][n] = clamp(((sum_u C[u][n] t[m][u] + (1 << 18)) >> 19) + 128, 0, 255)
// Both clamps are out of reach of coefficients an encoder can produce (|d| <= 1153, |t| <= 16 x 703) and make every sum fit int32
// for every int16 coefficient and every Q (jpeg_decode_model.value_ranges).
#include "common.hpp"
#include "jpeg_interval.hpp"
#include "jpeg_subseq.hpp"
#include "launch.hpp"
#include "vface_kernels.hpp"

namespace {

constexpr int kMcuCoefs = 6 * 64;
constexpr int kScanGridCap = 1024;        // workgroups (one frame each) before the grid loops (tests/test_mjpeg_in_gpu.py)
constexpr int kScanBytesPerThread = 8;
constexpr int kDecodeGridCap = 4096;      // workgroups of one wave (64 intervals of one frame) before the grid loops
constexpr int kPlanesGridCap = 2048;      // workgroups of 4 MCUs, as in csrc/mjpeg.hip
constexpr int kMcuPerGroup = 4;

template <typename T>
__device__ inline T wave_inclusive_scan(T x, int lane) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const T y = __shfl_up(x, d);
        if (lane >= d) x += y;
    }
    return x;
}

// intervals of a frame of `mcus` MCUs whose DRI says `restart` (0 = none)
__host__ __device__ inline int interval_count(int mcus, int restart) {
    return restart <= 0 || restart >= mcus ? 1 : (mcus + restart - 1) / restart;
}

// One workgroup per frame.  Inside a scan FF is followed by 00, RSTm or EOI only, so "FF then D0..D7" IS a marker: every thread
// compares kScanBytesPerThread bytes, a prefix sum over the workgroup numbers the markers, and marker j ends interval j and opens
// interval j + 1.  ranges [frames][max_intervals][2] (begin, end; bytes of `scans`).  A marker past the count the header promises
// is counted and not stored.  A frame with a wrong count or a wrong order, or whose bytes do not lie inside the buffer, gets its
// status and a row of zeros.
__global__ __launch_bounds__(256) void jpeg_scan_index_kernel(const unsigned char* __restrict__ scans, const long* __restrict__ offsets,
                                                              const int* __restrict__ lengths, const int* __restrict__ restart,
                                                              long scan_bytes, int mcus, int frames, int max_intervals,
                                                              int* __restrict__ ranges, int* __restrict__ status) {
    __shared__ int wsum[4];
    __shared__ int disorder;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    for (int f = blockIdx.x; f < frames; f += gridDim.x) {
        const long off = offsets[f];
        const bool inside = off >= 0 && lengths[f] >= 0 && off <= scan_bytes - lengths[f];      // (device data: checked, not trusted; no sum that could wrap)
        const long len = inside ? lengths[f] : 0;
        const int want = min(interval_count(mcus, restart[f]), max_intervals);
        const unsigned char* p = scans + off;
        int* row = ranges + (long)f * max_intervals * 2;
        if (tid == 0) disorder = 0;
        __syncthreads();
        int base = 0;
        for (long s = 0; s < len; s += 256 * kScanBytesPerThread) {
            const long i0 = s + tid * kScanBytesPerThread;
            unsigned flags = 0;
            int cnt = 0;
#pragma unroll
            for (int j = 0; j < kScanBytesPerThread; ++j) {
                const long i = i0 + j;
                if (i + 1 < len && p[i] == 0xFF && (p[i + 1] & 0xF8) == 0xD0) {
                    flags |= 1u << j;
                    ++cnt;
                }
            }
            const int incl = wave_inclusive_scan(cnt, lane);
            if (lane == 63) wsum[wave] = incl;
            __syncthreads();
            int before = 0, all = 0;
#pragma unroll
            for (int w = 0; w < 4; ++w) {
                if (w < wave) before += wsum[w];
                all += wsum[w];
            }
            int m = base + before + incl - cnt;         // the number of this thread's first marker
#pragma unroll
            for (int j = 0; j < kScanBytesPerThread; ++j) {
                if (flags & (1u << j)) {
                    const long i = i0 + j;
                    if ((p[i + 1] & 7) != (m & 7)) disorder = 1;
                    if (m + 1 < want) {
                        row[2 * m + 1] = (int)(off + i);
                        row[2 * (m + 1)] = (int)(off + i + 2);
                    }
                    ++m;
                }
            }
            base += all;
            __syncthreads();
        }
        const int code = !inside || base != want - 1 ? VF_JPEG_MARKER_COUNT : (disorder ? VF_JPEG_MARKER_ORDER : VF_JPEG_OK);
        __syncthreads();
        if (code != VF_JPEG_OK) {
            for (int i = tid; i < 2 * max_intervals; i += 256) row[i] = 0;
        } else {
            if (tid == 0) {
                row[0] = (int)off;
                row[2 * (want - 1) + 1] = (int)(off + len);
            }
            for (int i = 2 * want + tid; i < 2 * max_intervals; i += 256) row[i] = 0;
        }
        if (tid == 0) status[f] = code;
        __syncthreads();
    }
}

}  // namespace

extern "C" int vface_jpeg_scan_index(const uint8_t* scans, int64_t scan_bytes, const int64_t* offsets, const int32_t* lengths,
                                     const int32_t* restart, int mcus, int frames, int max_intervals, int32_t* ranges,
                                     int32_t* status, void* stream_) {
    hipStream_t stream = vf_stream(stream_);
    if (!scans || !offsets || !lengths || !restart || !ranges || !status || mcus <= 0 || frames <= 0 || max_intervals <= 0 ||
        scan_bytes <= 0)
        return VF_ERR_ARG;
    if (scan_bytes > 0x7FFFFFFFL || max_intervals > mcus) return VF_ERR_SHAPE;       // the ranges are int32; an interval holds an MCU
    static_assert(sizeof(long) == sizeof(int64_t), "offsets are passed as long");
    hipLaunchKernelGGL(jpeg_scan_index_kernel, dim3(vf_grid(frames, 1, kScanGridCap)), dim3(256), 0, stream, scans,
                       (const long*)offsets, lengths, restart, (long)scan_bytes, mcus, frames, max_intervals, ranges, status);
    return vf_launched();
}

// ---- entropy decoding ---------------------------------------------------------------------------------------------------------
namespace {

// out: frame f at f * frame_stride, mcus * 384 elements of it; elements between frames are not written
__global__ __launch_bounds__(256) void jpeg_clear_kernel(short* __restrict__ out, long frame_stride, long per_frame, long total) {
    for (long i = blockIdx.x * 256L + threadIdx.x; i < total; i += gridDim.x * 256L) {
        const long f = i / per_frame;
        out[f * frame_stride + (i - f * per_frame)] = 0;
    }
}

// A workgroup of one wave serves 64 consecutive intervals of ONE frame: it stages that frame's tables in LDS, then lane l decodes
// interval 64 c + l with the shared routine.  Frames that vface_jpeg_scan_index refused are left cleared.  A range that does not
// lie inside the scan buffer (the ranges are device data) is refused as VF_JPEG_SHORT before a byte is read.  The frame's status
// is the largest of its intervals' codes.
// With `flags` (the last launch of vface_jpeg_decode_entropy_parallel; nullptr otherwise): only frames whose flag is set are decoded,
// and the workgroup clears the MCUs of its 64 intervals first.
__global__ __launch_bounds__(64) void jpeg_decode_entropy_kernel(const unsigned char* __restrict__ scans, long scan_bytes,
                                                                 const int* __restrict__ ranges, const int* __restrict__ restart,
                                                                 const unsigned char* __restrict__ tables, int mcus, int frames,
                                                                 int max_intervals, int chunks, short* __restrict__ out,
                                                                 long frame_stride, int* status, const int* __restrict__ flags) {
    __shared__ VfJpegTables tab;
    static_assert(sizeof(VfJpegTables) == 2304 && sizeof(VfJpegTables) % 4 == 0, "the table block of scripts/mjpeg_in.py");
    const int lane = threadIdx.x;
    const long items = (long)frames * chunks;
    for (long it = blockIdx.x; it < items; it += gridDim.x) {
        const int f = (int)(it / chunks), c = (int)(it - (long)f * chunks);
        if (flags && !flags[f]) continue;
        __syncthreads();
        const unsigned* src = (const unsigned*)(tables + (long)f * sizeof(VfJpegTables));
        for (int i = lane; i < (int)(sizeof(VfJpegTables) / 4); i += 64) ((unsigned*)&tab)[i] = src[i];
        __syncthreads();
        const int r = restart[f];
        const int step = r <= 0 || r >= mcus ? mcus : r;
        const int n = min(interval_count(mcus, r), max_intervals);
        if (flags) {
            const long lo = min((long)c * 64 * step, (long)mcus) * kMcuCoefs, hi = min(((long)c * 64 + 64) * step, (long)mcus) * kMcuCoefs;
            if (c * 64 < n)
                for (long e = lo + lane; e < hi; e += 64) out[f * frame_stride + e] = 0;
            __syncthreads();
        }
        const int i = c * 64 + lane;
        if (i >= n || status[f] == VF_JPEG_MARKER_COUNT || status[f] == VF_JPEG_MARKER_ORDER) continue;
        const int m0 = i * step, m1 = min(m0 + step, mcus);
        const long begin = ranges[((long)f * max_intervals + i) * 2], end = ranges[((long)f * max_intervals + i) * 2 + 1];
        int code = VF_JPEG_SHORT;
        if (m0 < m1 && begin >= 0 && begin <= end && end <= scan_bytes)
            code = vf_jpeg_decode_interval(scans, begin, end, &tab, (m1 - m0) * 6, out + f * frame_stride + (long)m0 * kMcuCoefs);
        if (code != VF_JPEG_OK) atomicMax(&status[f], code);
    }
}

}  // namespace

extern "C" int vface_jpeg_decode_entropy(const uint8_t* scans, int64_t scan_bytes, const int32_t* ranges, const int32_t* restart,
                                         const uint8_t* tables, int mcus, int frames, int max_intervals, int16_t* out,
                                         int64_t frame_stride, int32_t* status, void* stream_) {
    hipStream_t stream = vf_stream(stream_);
    if (!scans || !ranges || !restart || !tables || !out || !status || mcus <= 0 || frames <= 0 || max_intervals <= 0 ||
        scan_bytes <= 0)
        return VF_ERR_ARG;
    if (scan_bytes > 0x7FFFFFFFL || max_intervals > mcus || frame_stride < (long)mcus * kMcuCoefs) return VF_ERR_SHAPE;
    if (((size_t)tables & 3) != 0) return VF_ERR_ALIGN;
    const long per_frame = (long)mcus * kMcuCoefs, total = per_frame * frames;
    hipLaunchKernelGGL(jpeg_clear_kernel, dim3(vf_grid(total, 256 * 8, 4096)), dim3(256), 0, stream, (short*)out, (long)frame_stride,
                       per_frame, total);
    const int chunks = (max_intervals + 63) / 64;
    hipLaunchKernelGGL(jpeg_decode_entropy_kernel, dim3(vf_grid((long)frames * chunks, 1, kDecodeGridCap)), dim3(64), 0, stream,
                       scans, (long)scan_bytes, ranges, restart, tables, mcus, frames, max_intervals, chunks, (short*)out,
                       (long)frame_stride, status, (const int*)nullptr);
    return vf_launched();
}

// ---- entropy decoding, many lanes per interval -----------------------------------------------------------------------------------
namespace {

constexpr int kParallelGridCap = 4096;    // workgroups (one (frame, interval) each) before the grid loops

__global__ __launch_bounds__(256) void jpeg_flags_clear_kernel(int* __restrict__ flags, int frames) {
    for (int i = blockIdx.x * 256 + threadIdx.x; i < frames; i += gridDim.x * 256) flags[i] = 0;
}

// exclusive prefix sum of x over the L lanes of the workgroup, and the sum of all; wsum: L / 64 words of LDS
template <int L>
__device__ inline int group_exclusive_scan(int x, int* wsum, int& all) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int incl = wave_inclusive_scan(x, lane);
    if (lane == 63) wsum[wave] = incl;
    __syncthreads();
    int before = 0;
    all = 0;
#pragma unroll
    for (int w = 0; w < L / 64; ++w) {
        if (w < wave) before += wsum[w];
        all += wsum[w];
    }
    __syncthreads();
    return before + incl - x;
}

// One workgroup of L lanes per (frame, interval); csrc/jpeg_subseq.hpp states the subsequences, the state and the routine.
//   The interval is walked in chunks of L subsequences.  Lane 0 of a chunk starts from the verified exit state of the chunk before
//   (the interval's first bit, slot 0, k 0 for chunk 0), every other lane from its guess.  Then rounds: lane i >= 1 compares lane
//   i - 1's exit state with the start state it used last and decodes again only where they differ; the chunk is done when a round
//   changes nothing -- after at most L - 1 rounds that change something, since lane j is exact after j rounds whatever the bytes
//   are.  rounds [frames][max_intervals] counts the rounds that changed something, summed over the chunks.
//   Write pass: a prefix sum of the blocks the lanes began gives every lane its first block; it decodes once more from its
//   verified start state and writes AC coefficients and DC differences.  DC pass: per component an inclusive scan of the
//   differences over the interval's MCUs (int32 arithmetic, wrap-around not undefined: the first sum that leaves int16 is seen).
//   Anything the serial routine would report -- met by a lane that holds a block below `blocks`, too few blocks begun, a DC sum
//   outside int16, a range outside the buffer -- sets flags[f]; the launch behind this one decodes such a frame serially.
template <int L>
__global__ __launch_bounds__(L) void jpeg_decode_parallel_kernel(const unsigned char* __restrict__ scans, long scan_bytes,
                                                                 const int* __restrict__ ranges, const int* __restrict__ restart,
                                                                 const unsigned char* __restrict__ tables, int mcus, int frames,
                                                                 int max_intervals, int subseq_bytes, short* __restrict__ out,
                                                                 long frame_stride, const int* __restrict__ status,
                                                                 int* __restrict__ flags, int* __restrict__ rounds) {
    __shared__ VfJpegTables tab;
    __shared__ VfJpegSubState exits[L];
    __shared__ int wsum[L / 64];
    const int tid = threadIdx.x;
    const long items = (long)frames * max_intervals;
    for (long it = blockIdx.x; it < items; it += gridDim.x) {
        const int f = (int)(it / max_intervals), i = (int)(it - (long)f * max_intervals);
        const int r = restart[f];
        const int step = r <= 0 || r >= mcus ? mcus : r;
        const int n = min(interval_count(mcus, r), max_intervals);
        const int refused = status[f];
        const int m0 = min((long)i * step, (long)mcus), m1 = min(m0 + step, mcus);
        const long begin = ranges[it * 2], end = ranges[it * 2 + 1];
        const bool inside = m0 < m1 && begin >= 0 && begin <= end && end <= scan_bytes;
        if (i >= n || refused == VF_JPEG_MARKER_COUNT || refused == VF_JPEG_MARKER_ORDER || !inside) {       // (the same for every lane)
            if (tid == 0) {
                if (rounds) rounds[it] = 0;
                if (i < n && refused != VF_JPEG_MARKER_COUNT && refused != VF_JPEG_MARKER_ORDER) flags[f] = 1;
            }
            continue;
        }
        __syncthreads();
        const unsigned* src = (const unsigned*)(tables + (long)f * sizeof(VfJpegTables));
        for (int w = tid; w < (int)(sizeof(VfJpegTables) / 4); w += L) ((unsigned*)&tab)[w] = src[w];
        __syncthreads();
        const int blocks = (m1 - m0) * 6, max_steps = 8 * subseq_bytes;
        short* o = out + f * frame_stride + (long)m0 * kMcuCoefs;
        const long nsub = vf_jpeg_subseq_count(end - begin, subseq_bytes);
        VfJpegSubState carry = {(int32_t)begin, 0};
        long blocks_before = 0;
        int ran = 0;
        bool fault = false;
        for (long c0 = 0; c0 < nsub; c0 += L) {
            const bool live = c0 + tid < nsub;
            const long sub_begin = begin + (c0 + tid) * subseq_bytes, sub_end = sub_begin + subseq_bytes;
            VfJpegSubState start = carry, reached = carry;
            int begun = 0;
            if (live) {
                if (tid > 0) start = vf_jpeg_subseq_guess(scans, begin, end, sub_begin);
                reached = start;
                vf_jpeg_decode_subseq(scans, begin, end, sub_end, max_steps, &tab, reached, begun, 0, 0, nullptr);
            }
            exits[tid] = reached;
            for (int round = 0; round < L; ++round) {
                __syncthreads();
                VfJpegSubState want = start;
                if (live && tid > 0) want = exits[tid - 1];
                const bool changed = !vf_jpeg_sub_same(want, start);
                if (!__syncthreads_or(changed ? 1 : 0)) break;          // (a barrier: every exit state has been read)
                ++ran;
                if (changed) {
                    start = reached = want;
                    vf_jpeg_decode_subseq(scans, begin, end, sub_end, max_steps, &tab, reached, begun, 0, 0, nullptr);
                    exits[tid] = reached;
                }
            }
            __syncthreads();
            carry = exits[L - 1];
            int all;
            const int first = group_exclusive_scan<L>(live ? begun : 0, wsum, all);
            if (live) {
                int again;
                VfJpegSubState from = start;
                if (vf_jpeg_decode_subseq(scans, begin, end, sub_end, max_steps, &tab, from, again, blocks_before + first, blocks, o) != VF_JPEG_OK)
                    fault = true;
            }
            blocks_before += all;
        }
        if (blocks_before < blocks) fault = true;
        __syncthreads();                                                // the differences are in memory for every lane
        unsigned before[3] = {0u, 0u, 0u};
        for (int mb = 0; mb < m1 - m0; mb += L) {
            const int m = mb + tid;
            short* p = o + (long)m * kMcuCoefs;
            unsigned y[4] = {0u, 0u, 0u, 0u}, cb = 0u, cr = 0u;
            if (m < m1 - m0) {
#pragma unroll
                for (int q = 0; q < 4; ++q) y[q] = (unsigned)(int)p[q * 64] + (q ? y[q - 1] : 0u);
                cb = (unsigned)(int)p[4 * 64];
                cr = (unsigned)(int)p[5 * 64];
            }
            int all_y, all_cb, all_cr;
            const unsigned by = before[0] + (unsigned)group_exclusive_scan<L>((int)y[3], wsum, all_y);
            const unsigned bcb = before[1] + (unsigned)group_exclusive_scan<L>((int)cb, wsum, all_cb);
            const unsigned bcr = before[2] + (unsigned)group_exclusive_scan<L>((int)cr, wsum, all_cr);
            if (m < m1 - m0) {
                const int v[6] = {(int)(by + y[0]), (int)(by + y[1]), (int)(by + y[2]), (int)(by + y[3]), (int)(bcb + cb), (int)(bcr + cr)};
#pragma unroll
                for (int q = 0; q < 6; ++q) {
                    if (v[q] < -32768 || v[q] > 32767) fault = true;
                    p[q * 64] = (short)v[q];
                }
            }
            before[0] += (unsigned)all_y;
            before[1] += (unsigned)all_cb;
            before[2] += (unsigned)all_cr;
        }
        if (fault) flags[f] = 1;
        if (rounds && tid == 0) rounds[it] = ran;
    }
}

}  // namespace

extern "C" size_t vface_jpeg_decode_entropy_parallel_workspace_bytes(int frames) {
    return frames > 0 ? (size_t)frames * sizeof(int) : 0;
}

extern "C" int vface_jpeg_decode_entropy_parallel(const uint8_t* scans, int64_t scan_bytes, const int32_t* ranges,
                                                  const int32_t* restart, const uint8_t* tables, int mcus, int frames,
                                                  int max_intervals, int16_t* out, int64_t frame_stride, int32_t* status,
                                                  int subseq_bytes, void* workspace, size_t workspace_bytes, int32_t* rounds,
                                                  void* stream_) {
    hipStream_t stream = vf_stream(stream_);
    if (!scans || !ranges || !restart || !tables || !out || !status || !workspace || mcus <= 0 || frames <= 0 || max_intervals <= 0 ||
        scan_bytes <= 0)
        return VF_ERR_ARG;
    if (scan_bytes > 0x7FFFFFFFL || max_intervals > mcus || frame_stride < (long)mcus * kMcuCoefs) return VF_ERR_SHAPE;
    if (subseq_bytes < kVfJpegSubseqMin || subseq_bytes > kVfJpegSubseqMax || subseq_bytes % 4 != 0) return VF_ERR_SHAPE;
    if (workspace_bytes < vface_jpeg_decode_entropy_parallel_workspace_bytes(frames)) return VF_ERR_SHAPE;
    if (((size_t)tables & 3) != 0 || ((size_t)workspace & 3) != 0) return VF_ERR_ALIGN;
    int* flags = (int*)workspace;
    const long per_frame = (long)mcus * kMcuCoefs, total = per_frame * frames;
    hipLaunchKernelGGL(jpeg_clear_kernel, dim3(vf_grid(total, 256 * 8, 4096)), dim3(256), 0, stream, (short*)out, (long)frame_stride,
                       per_frame, total);
    hipLaunchKernelGGL(jpeg_flags_clear_kernel, dim3(vf_grid(frames, 256, 64)), dim3(256), 0, stream, flags, frames);
    const dim3 grid(vf_grid((long)frames * max_intervals, 1, kParallelGridCap));
    if (vf_jpeg_subseq_lanes((long)scan_bytes, frames, max_intervals, subseq_bytes) == kVfJpegLanesLong)
        hipLaunchKernelGGL(jpeg_decode_parallel_kernel<kVfJpegLanesLong>, grid, dim3(kVfJpegLanesLong), 0, stream, scans, (long)scan_bytes,
                           ranges, restart, tables, mcus, frames, max_intervals, subseq_bytes, (short*)out, (long)frame_stride,
                           (const int*)status, flags, rounds);
    else
        hipLaunchKernelGGL(jpeg_decode_parallel_kernel<kVfJpegLanesShort>, grid, dim3(kVfJpegLanesShort), 0, stream, scans, (long)scan_bytes,
                           ranges, restart, tables, mcus, frames, max_intervals, subseq_bytes, (short*)out, (long)frame_stride,
                           (const int*)status, flags, rounds);
    const int chunks = (max_intervals + 63) / 64;
    hipLaunchKernelGGL(jpeg_decode_entropy_kernel, dim3(vf_grid((long)frames * chunks, 1, kDecodeGridCap)), dim3(64), 0, stream, scans,
                       (long)scan_bytes, ranges, restart, tables, mcus, frames, max_intervals, chunks, (short*)out, (long)frame_stride,
                       status, (const int*)flags);
    return vf_launched();
}

// ---- coefficients -> I420 rows -------------------------------------------------------------------------------------------------
namespace {

constexpr int kIdct[8][8] = {{11585, 11585, 11585, 11585, 11585, 11585, 11585, 11585},
                             {16069, 13623, 9102, 3196, -3196, -9102, -13623, -16069},
                             {15137, 6270, -6270, -15137, -15137, -6270, 6270, 15137},
                             {13623, -3196, -16069, -9102, 9102, 16069, 3196, -13623},
                             {11585, -11585, -11585, 11585, 11585, -11585, -11585, 11585},
                             {9102, -16069, 3196, 13623, -13623, -3196, 16069, -9102},
                             {6270, -15137, 15137, -6270, -6270, 15137, -15137, 6270},
                             {3196, -9102, 13623, -16069, 16069, -13623, 9102, -3196}};
// kUnzigzag[k] = row-major index (8 v + u) of the k-th coefficient of the scan (kZigzag of csrc/mjpeg.hip)
__device__ const unsigned char kUnzigzag[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                                41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                                30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
constexpr int kDequantMax = 2047;                 // d in [-2048, 2047]
constexpr int kPass1Shift = 11, kPass1Max = 16383;      // t in [-16384, 16383]: 4 fraction bits
constexpr int kPass2Shift = 19;

// one 8-point inverse transform: x[n] = sum_k C[k][n] X[k]; C[k][7 - n] = (-1)^k C[k][n], so the even and the odd frequencies give
// the sum and the difference of x[n] and x[7 - n].  Integer sums are exact in any order.
__device__ inline void idct8(const int (&X)[8], int (&x)[8]) {
#pragma unroll
    for (int n = 0; n < 4; ++n) {
        int e = 0, o = 0;
#pragma unroll
        for (int k = 0; k < 8; k += 2) {
            e += kIdct[k][n] * X[k];
            o += kIdct[k + 1][n] * X[k + 1];
        }
        x[n] = e + o;
        x[7 - n] = e - o;
    }
}

// coef: frame f at f * coef_stride, [mcus][6][64] zigzag; quant [frames][3][64] row-major, by component; out: frame f at
// f * row_stride: Y [H][W], Cb [ch][cw], Cr [ch][cw].  One wave per MCU, four per workgroup, the loop's trip count the same for
// every wave of the workgroup (the barriers), as in jpeg_coefficients_kernel.
__global__ __launch_bounds__(256) void jpeg_planes_kernel(const short* __restrict__ coef, long coef_stride,
                                                          const unsigned char* __restrict__ quant, int W, int H,
                                                          unsigned char* __restrict__ out, long row_stride, long mcus, long groups,
                                                          int mcu_cols, int per_frame) {
    __shared__ int px[kMcuPerGroup][6][64];
    __shared__ int tt[kMcuPerGroup][6][64];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int zz = kUnzigzag[lane];
    const int cw = (W + 1) / 2, ch = (H + 1) / 2;
    for (long g = blockIdx.x; g < groups; g += gridDim.x) {
        const long m = g * kMcuPerGroup + wave;
        const bool live = m < mcus;
        const long f = live ? m / per_frame : 0;
        const int rem = live ? (int)(m - f * per_frame) : 0;
        if (live) {                     // dequantise: lane = position in the scan
            const short* c = coef + f * coef_stride + (long)rem * kMcuCoefs + lane;
            const unsigned char* q = quant + f * 192;
#pragma unroll
            for (int b = 0; b < 6; ++b) {
                const int d = (int)c[b * 64] * (int)q[(b < 4 ? 0 : b - 3) * 64 + zz];
                px[wave][b][zz] = min(kDequantMax, max(-kDequantMax - 1, d));
            }
        }
        __syncthreads();
        if (live && lane < 48) {        // columns: lane = (block, u)
            const int b = lane >> 3, u = lane & 7;
            int X[8], x[8];
#pragma unroll
            for (int v = 0; v < 8; ++v) X[v] = px[wave][b][v * 8 + u];
            idct8(X, x);
#pragma unroll
            for (int r = 0; r < 8; ++r)
                tt[wave][b][r * 8 + u] = min(kPass1Max, max(-kPass1Max - 1, (x[r] + (1 << (kPass1Shift - 1))) >> kPass1Shift));
        }
        __syncthreads();
        if (live && lane < 48) {        // rows: lane = (block, row)
            const int b = lane >> 3, r = lane & 7;
            int X[8], x[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) X[u] = tt[wave][b][r * 8 + u];
            idct8(X, x);
#pragma unroll
            for (int n = 0; n < 8; ++n)
                px[wave][b][r * 8 + n] = min(255, max(0, ((x[n] + (1 << (kPass2Shift - 1))) >> kPass2Shift) + 128));
        }
        __syncthreads();
        if (live) {                     // store, cropped: lane = (row, 4 pixels) of the luma, one sample of each chroma block
            const int my = rem / mcu_cols, mx = rem - my * mcu_cols;
            unsigned char* o = out + f * row_stride;
            const int r = lane >> 2, x4 = (lane & 3) * 4;
            const int gy = my * 16 + r;
            if (gy < H) {
                const int yb = (r >> 3) * 2 + (x4 >> 3), yo = (r & 7) * 8 + (x4 & 7);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int gx = mx * 16 + x4 + j;
                    if (gx < W) o[(long)gy * W + gx] = (unsigned char)px[wave][yb][yo + j];
                }
            }
            const int cy = my * 8 + (lane >> 3), cx = mx * 8 + (lane & 7);
            if (cy < ch && cx < cw) {
                o[(long)W * H + (long)cy * cw + cx] = (unsigned char)px[wave][4][lane];
                o[(long)W * H + (long)cw * ch + (long)cy * cw + cx] = (unsigned char)px[wave][5][lane];
            }
        }
        __syncthreads();
    }
}

}  // namespace

extern "C" int vface_jpeg_planes(const int16_t* coef, int64_t coef_stride, const uint8_t* quant, int W, int H, int frames,
                                 uint8_t* out, int64_t row_stride, void* stream_) {
    hipStream_t stream = vf_stream(stream_);
    if (!coef || !quant || !out || W <= 0 || H <= 0 || frames <= 0) return VF_ERR_ARG;
    if (W > 65535 || H > 65535) return VF_ERR_SHAPE;
    const long mcu_cols = (W + 15) / 16, per_frame = mcu_cols * ((H + 15) / 16);
    const long frame_bytes = (long)W * H + 2L * ((W + 1) / 2) * ((H + 1) / 2);
    if (coef_stride < per_frame * kMcuCoefs || row_stride < frame_bytes) return VF_ERR_SHAPE;
    const long mcus = per_frame * frames, groups = (mcus + kMcuPerGroup - 1) / kMcuPerGroup;
    hipLaunchKernelGGL(jpeg_planes_kernel, dim3(vf_grid(groups, 1, kPlanesGridCap)), dim3(256), 0, stream, (const short*)coef,
                       (long)coef_stride, quant, W, H, out, (long)row_stride, mcus, groups, (int)mcu_cols, (int)per_frame);
    return vf_launched();
}
