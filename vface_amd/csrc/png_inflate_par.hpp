// Inflate of ONE stream on many waves, block by block, on top of csrc/png_inflate.hpp: the pieces csrc/png_in_par.hip's kernels are
// made of (vface_png_inflate_parallel), written once for the device and the host.  tests/png_inflate_par_probe.cpp runs
// vf_inf_stream_parallel from a plain C++ program under the address and undefined-behaviour sanitizers; tests/png_inflate_par_model.py
// states the protocol in Python, and both equal it in the candidate list, the fallback reason and everything the serial routine returns.
//
// A deflate block can be decoded without its predecessors but for where it starts and the 32 KiB of output in front of it (the
// algorithm of pugz and rapidgzip).  The seven steps:
//   find      the body is cut into chunks of chunk_bytes; chunk 0's segment starts at bit 0, chunk c >= 1's at the smallest bit of
//             the chunk's own range at which a DYNAMIC block start passes (vf_inf_par_quick in registers for every position, then
//             vf_inf_par_passes: the whole header through vf_inf_dynamic_tables); a chunk without one starts no segment
//   count     a segment is decoded block after block, writing nothing, until a block ends at a bit >= the next segment's start, or
//             was final (vf_inf_par_segment with VfInfCountSink)
//   validate  no segment reports a status (else reason 2); every segment ends exactly on the next one's start without BFINAL and the
//             last one saw BFINAL (else 1); the counts sum to `expect` (else 3).  By induction from bit 0 an accepted chain IS the
//             serial decode's block sequence: a false candidate costs a fallback and never a wrong byte
//   place     the exclusive prefix sum of the counts: every segment's offset
//   write     the segment again, into 16-bit elements: < 256 a byte, 0x8000 | k "the byte k positions into the 32 768 bytes in front
//             of this segment's first byte"; a match that copies from such an element copies the element.  A distance greater than
//             offset + the bytes produced so far flags the file (reason 4: status 12 is the serial routine's to report)
//   resolve   segments in order: an element becomes a byte; a marker reads the output where an earlier segment has finished it
//   fall back a flagged file is the serial routine's, whole
//
// Everything that file bytes steer and that indexes memory is here or in png_inflate.hpp, and holds for EVERY input:
//   - a reader is opened only at a bit inside the stream, and loads a byte only where pos < end (png_inflate.hpp's reader);
//   - the window of the cheap test is read byte by byte, each only where pos < len; what lies behind the end reads as 0 and the
//     test itself refuses a header that would need it;
//   - a plane element is written only below the segment's counted length, which validate has summed to exactly `expect`;
//   - a marker is made only for a source inside the 32 768 elements in front of the segment, and only where the distance has been
//     checked against offset + produced, so resolve reads [0, offset) alone -- and checks it again.
// This file has no include of the HIP runtime: a C++17 host compiler reads it as it is.
#pragma once
#include "png_inflate.hpp"

constexpr int kInfParMinChunk = 64, kInfParMaxChunk = 1 << 20;
constexpr unsigned kInfMark = 0x8000u;

enum VfInfParReason {
    VF_INF_PAR_NONE = 0,
    VF_INF_PAR_CHAIN = 1,       // the chain did not close
    VF_INF_PAR_STATUS = 2,      // a segment reported a status
    VF_INF_PAR_COUNT = 3,       // the byte count is not `expect`
    VF_INF_PAR_FAR = 4,         // a reference reaches in front of the file
    VF_INF_PAR_RANGE = 5,       // the file's range lies outside the buffer
};

// ---- a reader opened at an arbitrary bit.  A Src of this file adds to png_inflate.hpp's: seek(pos) before bytes from another place
// are asked for (the device starts its LDS window over), raw(pos) = the byte itself, for a stored block's payload.
struct VfInfParHostSrc {
    const uint8_t* bytes;
    VF_INF_HD void ensure(long) {}
    VF_INF_HD void seek(long) {}
    VF_INF_HD unsigned at(long pos) const { return bytes[pos]; }
    VF_INF_HD unsigned raw(long pos) const { return bytes[pos]; }
};
// the exact bit position of a reader: the bits taken so far
template <class Src>
VF_INF_HD long vf_inf_bitpos(const VfInfBits<Src>& b) { return 8 * b.pos - b.n; }
// a reader that stands on bit `bit` of a stream of `len` bytes; 0 <= bit < 8 len (a reader opened elsewhere holds nothing and
// every take of it fails)
template <class Src>
VF_INF_HD VfInfBits<Src> vf_inf_open(Src src, long len, long bit) {
    const bool inside = bit >= 0 && (bit >> 3) < len;
    VfInfBits<Src> b = {src, inside ? bit >> 3 : len, len, 0ull, 0};
    if (inside) {
        b.src.seek(b.pos);
        unsigned v;
        vf_inf_take(b, (int)(bit & 7), v);
    }
    return b;
}

// ---- find
// Bytes [at, at + 16) of the stream as two words, least significant byte first; a byte at or behind `len` reads as 0 and is not loaded.
template <class Src>
VF_INF_HD void vf_inf_par_window(const Src& src, long len, long at, unsigned long long& lo, unsigned long long& hi) {
    lo = 0;
    hi = 0;
    for (int i = 0; i < 8; ++i) {
        if (at + i < len) lo |= (unsigned long long)src.raw(at + i) << (8 * i);
        if (at + 8 + i < len) hi |= (unsigned long long)src.raw(at + 8 + i) << (8 * i);
    }
}
// The cheap test of a block start, on the 96 bits from the position on (lo: the first 64, hi: the next 32) of which `avail` lie inside
// the stream: BTYPE 2, HLIT <= 29, HDIST <= 29, the 17 + 3 (HCLEN + 4) bits are there, and the code-length code is exactly complete
// (its Kraft sum in 128ths is 128) -- each of them necessary for vf_inf_dynamic_tables to return 0.
VF_INF_HD bool vf_inf_par_quick(unsigned long long lo, unsigned hi, long avail) {
    if (((lo >> 1) & 3u) != 2u || avail < 17) return false;
    if (((lo >> 3) & 31u) > 29u || ((lo >> 8) & 31u) > 29u) return false;
    const int ncode = (int)((lo >> 13) & 15u) + 4;
    if (avail < 17 + 3 * ncode) return false;
    unsigned long long x = (lo >> 17) | ((unsigned long long)hi << 47);        // the 3-bit lengths, 57 bits at most
    int kraft = 0;
    for (int i = 0; i < ncode; ++i) {
        const int l = (int)(x & 7u);
        x >>= 3;
        kraft += l ? 128 >> l : 0;
    }
    return kraft == 128;
}
// the 8 positions of byte `at`: bit j of the result = position 8 at + j passes the cheap test
template <class Src>
VF_INF_HD unsigned vf_inf_par_quick8(const Src& src, long len, long at) {
    unsigned long long lo, hi;
    vf_inf_par_window(src, len, at, lo, hi);
    unsigned mask = 0;
    for (int j = 0; j < 8; ++j) {
        const unsigned long long l = j ? (lo >> j) | (hi << (64 - j)) : lo;
        if (vf_inf_par_quick(l, (unsigned)(hi >> j), 8 * (len - at) - j)) mask |= 1u << j;
    }
    return mask;
}
// A block start passes at `bit`: BTYPE 2 (either BFINAL) and the dynamic header behind it yields status 0 within the stream.
// One wave in lockstep on the device (tb is built); the tables are those of the block where it passes.
template <class Src>
VF_INF_HD bool vf_inf_par_passes(Src src, long len, long bit, VfInfTables& tb, int lane, int nlanes) {
    VfInfBits<Src> b = vf_inf_open(src, len, bit);
    unsigned v;
    if (!vf_inf_take(b, 3, v) || (v >> 1) != 2u) return false;
    return VF_INF_UNIFORM(vf_inf_dynamic_tables(b, tb, lane, nlanes)) == VF_INF_OK;
}
// chunks of a stream of `len` bytes: chunk 0 always is (an empty stream's segment reports status 1)
VF_INF_HD long vf_inf_par_chunks(long len, int chunk_bytes) { return len <= 0 ? 1 : (len + chunk_bytes - 1) / chunk_bytes; }
// the candidate of chunk c >= 1, or -1: the serial statement of what the device's lanes look for side by side
template <class Src>
VF_INF_HD long vf_inf_par_candidate(Src src, long len, long c, int chunk_bytes, VfInfTables& tb) {
    const long hi = (c + 1) * chunk_bytes < len ? (c + 1) * chunk_bytes : len;
    for (long at = c * chunk_bytes; at < hi; ++at) {
        unsigned mask = vf_inf_par_quick8(src, len, at);
        for (int j = 0; j < 8; ++j)
            if ((mask >> j & 1u) && vf_inf_par_passes(src, len, 8 * at + j, tb, 0, 1)) return 8 * at + j;
    }
    return -1;
}

// ---- count and write: one loop, two sinks
struct VfInfSegment {
    long start, end;            // bits: where it was opened; behind the last block decoded (status 0)
    long produced;
    long offset;                // place: the bytes of the segments in front
    int status;
    int final_seen;             // status 0 and the last block decoded was a final one
    int closes;                 // count: it ends on the next segment's start without BFINAL, or is the last and saw BFINAL
    int pad;
};
// A Sink takes what the blocks hold: literal(v), match(length, distance), stored(src, pos, n), each 0 or a status; flush() behind a
// block; produced().
struct VfInfCountSink {
    long n = 0;
    VF_INF_HD int literal(int) { n += 1; return VF_INF_OK; }
    VF_INF_HD int match(int length, int) { n += length; return VF_INF_OK; }
    template <class Src>
    VF_INF_HD int stored(const Src&, long, int len) { n += len; return VF_INF_OK; }
    VF_INF_HD void flush() {}
    VF_INF_HD long produced() const { return n; }
};
// the host's plane sink: plane = the segment's first element, `limit` its counted length, `offset` the bytes in front of it
struct VfInfPlaneSink {
    uint16_t* plane;
    long limit, offset;
    long n = 0;
    VF_INF_HD int literal(int v) {
        if (n + 1 > limit) return VF_INF_TOO_LONG;
        plane[n++] = (uint16_t)v;
        return VF_INF_OK;
    }
    VF_INF_HD int match(int length, int distance) {
        if (distance > offset + n) return VF_INF_TOO_FAR;
        if (n + length > limit) return VF_INF_TOO_LONG;
        for (int i = 0; i < length; ++i) {
            const long at = n - distance + i % distance;             // >= -32768: a distance is at most 32768
            plane[n + i] = at >= 0 ? plane[at] : (uint16_t)(kInfMark | (unsigned)(kInfWindow + at));
        }
        n += length;
        return VF_INF_OK;
    }
    template <class Src>
    VF_INF_HD int stored(const Src& src, long pos, int len) {
        if (n + len > limit) return VF_INF_TOO_LONG;
        for (int i = 0; i < len; ++i) plane[n + i] = (uint16_t)src.raw(pos + i);
        n += len;
        return VF_INF_OK;
    }
    VF_INF_HD void flush() {}
    VF_INF_HD long produced() const { return n; }
};

// Blocks from where `b` stands until one ends at a bit >= stop_at (stop_at < 0: there is no next segment) or was final.  One wave
// in lockstep on the device: every lane runs it with the same values.  -> r.status, r.end, r.final_seen, r.produced.
template <class Src, class Sink>
VF_INF_HD void vf_inf_par_segment(VfInfBits<Src>& b, long stop_at, VfInfTables& tb, int lane, int nlanes, Sink& sink, VfInfSegment& r) {
    int status = VF_INF_OK, final_block = 0;
    long end = vf_inf_bitpos(b);
    while (status == VF_INF_OK) {
        int type, stored;
        status = VF_INF_UNIFORM(vf_inf_block(b, final_block, type, stored));
        if (status != VF_INF_OK) break;
        final_block = VF_INF_UNIFORM(final_block);
        type = VF_INF_UNIFORM(type);
        if (type == 0) {
            stored = VF_INF_UNIFORM(stored);
            status = sink.stored(b.src, b.pos, stored);             // (vf_inf_block has found the bytes inside the stream)
            if (status != VF_INF_OK) break;
            b.pos += stored;
            b.src.seek(b.pos);
        } else {
            if (type == 1) vf_inf_fixed_tables(tb, lane, nlanes);
            else status = VF_INF_UNIFORM(vf_inf_dynamic_tables(b, tb, lane, nlanes));
            while (status == VF_INF_OK) {
                VfInfToken t;
                status = VF_INF_UNIFORM(vf_inf_token(b, tb, t));
                if (status != VF_INF_OK) break;
                const int length = VF_INF_UNIFORM(t.length), value = VF_INF_UNIFORM(t.value);
                if (length < 0) break;
                status = length == 0 ? sink.literal(value) : sink.match(length, value);
            }
            sink.flush();
            if (status != VF_INF_OK) break;
        }
        end = vf_inf_bitpos(b);
        if (final_block || (stop_at >= 0 && end >= stop_at)) break;
    }
    r.status = status;
    r.end = end;
    r.final_seen = status == VF_INF_OK && final_block;
    r.produced = sink.produced();
}

// ---- resolve: element i of the segment at `offset` -> its byte; rows = the file's first output byte.  A marker reads [0, offset)
// alone (one that would not -- write has refused every such distance -- reads nothing and gives 0).
VF_INF_HD unsigned vf_inf_par_resolve(unsigned element, long offset, const uint8_t* rows) {
    if (element < 256u) return element;
    const long at = offset - kInfWindow + (long)(element & 0x7FFFu);
    return at >= 0 && at < offset ? rows[at] : 0u;
}
// Adler-32's halves continued over a piece of L bytes with a1 = the sum of its bytes and a2 = the sum of (L - i) byte[i]
VF_INF_HD void vf_inf_par_adler(unsigned& s1, unsigned& s2, unsigned long long a1, unsigned long long a2, long L) {
    s2 = (unsigned)((s2 + (unsigned long long)(L % 65521) * s1 + a2 % 65521u) % 65521u);
    s1 = (unsigned)((s1 + a1 % 65521u) % 65521u);
}

// ---- the whole stream through the seven steps, serially: the statement of what vface_png_inflate_parallel does to one file.
// plane: `expect` elements; segs: vf_inf_par_chunks(len, chunk_bytes) records, of which the first info[0] (or, where the file falls
// back, those that were counted) are filled; candidates: as many longs less one.  Returns what vf_inf_stream returns, with
// adler[2] = (s1, s2) over out[0 .. produced) and info[4] = {segments accepted or 0, VfInfParReason, candidates found, 0}.
inline int vf_inf_stream_parallel(const uint8_t* stream, long len, uint8_t* out, long expect, int chunk_bytes, VfInfTables& tb, uint16_t* plane,
                                  VfInfSegment* segs, long* candidates, long& produced, long& consumed, unsigned* adler, int* info) {
    const VfInfParHostSrc src = {stream};
    const long chunks = vf_inf_par_chunks(len, chunk_bytes);
    long nseg = 0;
    segs[nseg++].start = 0;
    for (long c = 1; c < chunks; ++c) {                                         // find
        const long p = vf_inf_par_candidate(src, len, c, chunk_bytes, tb);
        if (p >= 0) {
            candidates[nseg - 1] = p;
            segs[nseg++].start = p;
        }
    }
    int reason = VF_INF_PAR_NONE;
    bool any_status = false, open_chain = false;
    long total = 0;
    for (long i = 0; i < nseg; ++i) {                                           // count, validate, place
        VfInfSegment& s = segs[i];
        const long next = i + 1 < nseg ? segs[i + 1].start : -1;
        VfInfBits<VfInfParHostSrc> b = vf_inf_open(src, len, s.start);
        VfInfCountSink sink;
        vf_inf_par_segment(b, next, tb, 0, 1, sink, s);
        s.closes = s.status == VF_INF_OK && (next >= 0 ? (!s.final_seen && s.end == next) : s.final_seen);
        s.offset = total;
        total += s.produced;
        any_status |= s.status != VF_INF_OK;
        open_chain |= !s.closes;
    }
    if (any_status) reason = VF_INF_PAR_STATUS;
    else if (open_chain) reason = VF_INF_PAR_CHAIN;
    else if (total != expect) reason = VF_INF_PAR_COUNT;
    for (long i = 0; i < nseg && reason == VF_INF_PAR_NONE; ++i) {              // write
        VfInfSegment& s = segs[i];
        VfInfBits<VfInfParHostSrc> b = vf_inf_open(src, len, s.start);
        VfInfPlaneSink sink = {plane + s.offset, s.produced, s.offset};
        VfInfSegment again = s;
        vf_inf_par_segment(b, i + 1 < nseg ? segs[i + 1].start : -1, tb, 0, 1, sink, again);
        if (again.status == VF_INF_TOO_FAR) reason = VF_INF_PAR_FAR;
        else if (again.status != VF_INF_OK || again.produced != s.produced) reason = VF_INF_PAR_STATUS;     // (never: the count said otherwise)
    }
    info[0] = reason == VF_INF_PAR_NONE ? (int)nseg : 0;
    info[1] = reason;
    info[2] = (int)(nseg - 1);
    info[3] = 0;
    unsigned s1 = 1, s2 = 0;
    int status;
    if (reason != VF_INF_PAR_NONE) {                                            // fall back
        status = vf_inf_stream(stream, len, out, expect, tb, produced, consumed);
        for (long done = 0; done < produced;) {
            const long L = produced - done < 4096 ? produced - done : 4096;
            unsigned long long a1 = 0, a2 = 0;
            for (long i = 0; i < L; ++i) {
                a1 += out[done + i];
                a2 += (unsigned long long)(L - i) * out[done + i];
            }
            vf_inf_par_adler(s1, s2, a1, a2, L);
            done += L;
        }
    } else {                                                                    // resolve
        for (long i = 0; i < nseg; ++i) {
            const VfInfSegment& s = segs[i];
            for (long done = 0; done < s.produced;) {
                const long L = s.produced - done < 4096 ? s.produced - done : 4096;
                unsigned long long a1 = 0, a2 = 0;
                for (long k = 0; k < L; ++k) {
                    const unsigned v = vf_inf_par_resolve(plane[s.offset + done + k], s.offset, out);
                    out[s.offset + done + k] = (uint8_t)v;
                    a1 += v;
                    a2 += (unsigned long long)(L - k) * v;
                }
                vf_inf_par_adler(s1, s2, a1, a2, L);
                done += L;
            }
        }
        status = VF_INF_OK;
        produced = expect;
        consumed = (segs[nseg - 1].end + 7) >> 3;
    }
    adler[0] = s1;
    adler[1] = s2;
    return status;
}
