// Inflate (RFC 1951) for the PNG frames in (REFace/scripts/VFace_inference_batch.py:285 writes the {index}.png frames a run reads),
// written once for the device and the host: csrc/png_in.hip walks a stream with these pieces on one wave per file,
// tests/png_inflate_probe.cpp runs vf_inf_stream from a plain C++ program under the address and undefined-behaviour sanitizers,
// and tests/png_inflate_model.py restates the format in Python.
//
// Everything that file bytes steer and that indexes memory is HERE, and is written to hold for EVERY input, not only for deflate:
//   - the bit reader loads a byte only where pos < end; what is asked for past the end is status 1, never a read;
//   - a code table is built only from a length set that passed its validity rule (never over-subscribed), so the canonical walk
//     indexes sym[] below the number of lengths; the walk takes at most 15 bits;
//   - a code-length repeat is checked against HLIT + HDIST before it is stored;
//   - a distance is checked against the bytes produced, and a token against `expect`, before a byte of it is written.
// The status of a stream is the FIRST condition met in stream order (VfInfStatus; within a dynamic header in the order listed);
// zlib 1.2.11 accepts a stream exactly where the status is 0 or would be but for the byte count (inflate.c / inftrees.c).
//
// Tables live in a VfInfTables that the caller owns (LDS on the device): no routine here keeps an array of its own.  The routines
// that only BUILD are written for `nlanes` callers that all hold the same values (the device's 64 lanes; the host calls with 0 of 1):
// what is order-dependent every caller does alike on the same addresses, the fast tables are filled entry by entry, lane-strided.
// On the device that holds for ONE wave in lockstep only (count[l]++, offs[l]++ and lens[have++] are read-modify-writes that all
// lanes make with the same value): never call vf_inf_count, vf_inf_fixed_tables or vf_inf_dynamic_tables from a workgroup of more than
// one wave with nlanes > 1 -- a wider workgroup lets one wave build (nlanes = 64) while the others wait at a barrier of their own.
// This file has no include of the HIP runtime: a C++17 host compiler reads it as it is.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define VF_INF_HD __host__ __device__ inline
#else
#define VF_INF_HD inline
#endif
// between a table's serial part and its lane-strided fill, and behind the fill: one wave per workgroup on the device
#if defined(__HIP_DEVICE_COMPILE__)
#define VF_INF_SYNC() __syncthreads()
#define VF_INF_UNIFORM(x) __builtin_amdgcn_readfirstlane(x)     // a value every lane holds alike, said so to the compiler
#else
#define VF_INF_SYNC() ((void)0)
template <typename T>
VF_INF_HD T vf_inf_same(T x) { return x; }
#define VF_INF_UNIFORM(x) vf_inf_same(x)
#endif

enum VfInfStatus {
    VF_INF_OK = 0,              // the final block ended with exactly `expect` bytes
    VF_INF_SHORT = 1,           // a bit was needed past the stream's end
    VF_INF_BLOCK_TYPE = 2,      // block type 3
    VF_INF_STORED_LEN = 3,      // stored block: LEN != ~NLEN
    VF_INF_TOO_MANY = 4,        // more than 286 literal/length codes or more than 30 distance codes
    VF_INF_CODE_LENGTHS = 5,    // the code-length code is over-subscribed or incomplete
    VF_INF_REPEAT = 6,          // repeat 16 with no previous length, or a repeat past HLIT + HDIST
    VF_INF_NO_END = 7,          // no code for symbol 256
    VF_INF_LITLEN_SET = 8,      // the literal/length set is over-subscribed, or incomplete and not a single 1-bit code
    VF_INF_DIST_SET = 9,        // the same for the distance set (no code at all is legal)
    VF_INF_LITLEN_CODE = 10,    // bits that are no literal/length code, or symbol 286 / 287
    VF_INF_DIST_CODE = 11,      // bits that are no distance code, or symbol 30 / 31
    VF_INF_TOO_FAR = 12,        // a distance greater than the bytes produced so far
    VF_INF_TOO_LONG = 13,       // more than `expect` bytes
    VF_INF_TOO_FEW = 14,        // the final block ended with fewer than `expect` bytes
};

constexpr int kInfLitLen = 288;         // the fixed code names 288 symbols; a dynamic header at most 286
constexpr int kInfDist = 32;            // the fixed code names 32; a dynamic header at most 30
constexpr int kInfCodeLen = 19;
constexpr int kInfLitFastBits = 10, kInfDistFastBits = 9, kInfCodeLenFastBits = 7;
constexpr int kInfWindow = 32768;

// One canonical code: count[l] codes of length l, sym[] the symbols by (length, symbol), fast[v] = (symbol << 4 | length) of the
// code that the low bits of v start with where it has at most FB bits, else 0.
template <int N, int FB>
struct VfInfCode {
    uint16_t count[16];
    uint16_t offs[16];
    uint16_t sym[N];
    uint16_t fast[1 << FB];
};

struct VfInfTables {
    VfInfCode<kInfLitLen, kInfLitFastBits> lit;
    VfInfCode<kInfDist, kInfDistFastBits> dist;
    VfInfCode<kInfCodeLen, kInfCodeLenFastBits> cl;
    uint8_t lens[kInfLitLen + kInfDist];        // the lengths a header carries: literal/length, then distance
};

// ---- the bounded bit reader.  Src: at(pos) = byte pos of the stream, asked only for pos < end; ensure(pos) is called before bytes
// from pos on are asked for (the device stages the stream through LDS there).
struct VfInfHostSrc {
    const uint8_t* bytes;
    VF_INF_HD void ensure(long) {}
    VF_INF_HD unsigned at(long pos) const { return bytes[pos]; }
};

template <class Src>
struct VfInfBits {
    Src src;
    long pos, end;              // the next byte to load; the stream's length
    unsigned long long acc;     // the low n bits are the next bits of the stream, least significant first
    int n;
};

template <class Src>
VF_INF_HD void vf_inf_refill(VfInfBits<Src>& b) {
    b.src.ensure(b.pos);
    for (int i = 0; i < 8 && b.n <= 56 && b.pos < b.end; ++i) {
        b.acc |= (unsigned long long)b.src.at(b.pos) << b.n;
        b.pos += 1;
        b.n += 8;
    }
}
// k <= 32 bits, or false where the stream does not hold them (status 1)
template <class Src>
VF_INF_HD bool vf_inf_take(VfInfBits<Src>& b, int k, unsigned& v) {
    if (b.n < k) vf_inf_refill(b);
    if (b.n < k) return false;
    v = (unsigned)(b.acc & ((1ull << k) - 1ull));
    b.acc >>= k;
    b.n -= k;
    return true;
}
// whole bytes of the stream behind the bits taken so far
template <class Src>
VF_INF_HD long vf_inf_consumed(const VfInfBits<Src>& b) { return b.pos - (b.n >> 3); }

// ---- tables
// The canonical walk (one bit at a time, as zlib's puff.c): the code that `v` starts with, LSB first, among at most `avail` bits.
// -> symbol and `len`; -1: 15 bits that are no code; -2: the bits ran out first.
template <int N, int FB>
VF_INF_HD int vf_inf_walk(const VfInfCode<N, FB>& t, unsigned v, int avail, int& len) {
    int code = 0, first = 0, index = 0;
    for (int l = 1; l <= 15; ++l) {
        if (l > avail) return -2;
        code |= (int)(v & 1u);
        v >>= 1;
        const int cnt = t.count[l];
        if (code - cnt < first) {
            len = l;
            const int at = index + (code - first);
            return at < N ? t.sym[at] : -1;
        }
        index += cnt;
        first = (first + cnt) << 1;
        code <<= 1;
    }
    return -1;
}

// lens[0 .. n) -> count, offs, sym.  Returns what is left of the code space in units of 2^-15: 0 = complete, > 0 = incomplete,
// < 0 = over-subscribed (the table is then NOT built).  `single` = the set is exactly one code of one bit; `none` = no code at all.
template <int N, int FB>
VF_INF_HD int vf_inf_count(VfInfCode<N, FB>& t, const uint8_t* lens, int n, bool& single, bool& none) {
    for (int l = 0; l < 16; ++l) t.count[l] = 0;
    for (int i = 0; i < n; ++i) t.count[lens[i] & 15] = (uint16_t)(t.count[lens[i] & 15] + 1);
    none = t.count[0] == n;
    int left = 1 << 15, used = 0;
    for (int l = 1; l <= 15; ++l) {
        left -= (int)t.count[l] << (15 - l);
        used += t.count[l];
    }
    single = used == 1 && t.count[1] == 1;
    if (left < 0) return left;
    t.offs[1] = 0;
    for (int l = 1; l < 15; ++l) t.offs[l + 1] = (uint16_t)(t.offs[l] + t.count[l]);
    for (int i = 0; i < n; ++i) {
        const int l = lens[i] & 15;
        if (l) {
            t.sym[t.offs[l]] = (uint16_t)i;
            t.offs[l] = (uint16_t)(t.offs[l] + 1);
        }
    }
    t.count[0] = 0;
    return left;
}
// the fast table of a built code, entries lane, lane + nlanes, ...
template <int N, int FB>
VF_INF_HD void vf_inf_fill(VfInfCode<N, FB>& t, int lane, int nlanes) {
    VF_INF_SYNC();
    for (int v = lane; v < (1 << FB); v += nlanes) {
        int len = 0;
        const int s = vf_inf_walk(t, (unsigned)v, FB, len);
        t.fast[v] = s >= 0 ? (uint16_t)((s << 4) | len) : (uint16_t)0;
    }
    VF_INF_SYNC();
}

// The next symbol of `t`: >= 0 and its bits are taken; -1: no code (nothing taken); -2: the stream ended inside the code.
template <class Src, int N, int FB>
VF_INF_HD int vf_inf_symbol(VfInfBits<Src>& b, const VfInfCode<N, FB>& t) {
    if (b.n < 15) vf_inf_refill(b);
    int len = 0, s;
    const unsigned e = b.n >= FB ? VF_INF_UNIFORM((unsigned)t.fast[(unsigned)b.acc & ((1u << FB) - 1u)]) : 0u;
    if (e) {
        s = (int)(e >> 4);
        len = (int)(e & 15u);
    } else {
        s = VF_INF_UNIFORM(vf_inf_walk(t, (unsigned)b.acc & 0x7FFFu, b.n, len));
        if (s < 0) return s;
        len = VF_INF_UNIFORM(len);
    }
    b.acc >>= len;
    b.n -= len;
    return s;
}

// deflate's length and distance codes: symbol 257 + i stands for lengths from vf_inf_len_base(i) with vf_inf_len_extra(i) extra
// bits, i = 0 .. 28; distance symbol i likewise, i = 0 .. 29
VF_INF_HD int vf_inf_len_base(int i) { return i < 8 ? 3 + i : (i == 28 ? 258 : 3 + ((4 + (i & 3)) << ((i >> 2) - 1))); }
VF_INF_HD int vf_inf_len_extra(int i) { return (i < 8 || i == 28) ? 0 : (i >> 2) - 1; }
VF_INF_HD int vf_inf_dist_base(int i) { return i < 4 ? 1 + i : 1 + ((2 + (i & 1)) << ((i >> 1) - 1)); }
VF_INF_HD int vf_inf_dist_extra(int i) { return i < 4 ? 0 : (i >> 1) - 1; }

// the fixed code of block type 1 (RFC 1951 3.2.6): 288 literal/length symbols of 8, 9, 7, 8 bits and 32 distance symbols of 5
VF_INF_HD void vf_inf_fixed_tables(VfInfTables& tb, int lane, int nlanes) {
    VF_INF_SYNC();
    for (int i = 0; i < kInfLitLen; ++i) tb.lens[i] = (uint8_t)(i < 144 ? 8 : i < 256 ? 9 : i < 280 ? 7 : 8);
    for (int i = 0; i < kInfDist; ++i) tb.lens[kInfLitLen + i] = 5;
    bool single, none;
    vf_inf_count(tb.lit, tb.lens, kInfLitLen, single, none);
    vf_inf_count(tb.dist, tb.lens + kInfLitLen, kInfDist, single, none);
    vf_inf_fill(tb.lit, lane, nlanes);
    vf_inf_fill(tb.dist, lane, nlanes);
}

// the header of a dynamic block (RFC 1951 3.2.7) -> the block's two tables, or the first status met
template <class Src>
VF_INF_HD int vf_inf_dynamic_tables(VfInfBits<Src>& b, VfInfTables& tb, int lane, int nlanes) {
    // the order in which the header carries the lengths of the code-length code
    const unsigned long long order_lo = 0x0B050A0609070800ull, order_hi = 0x0F010E020D030C04ull;     // 0, 8, 7, 9, 6, 10, 5, 11 | 4, 12, 3, 13, 2, 14, 1, 15
    unsigned hlit, hdist, hclen, v;
    if (!vf_inf_take(b, 5, hlit) || !vf_inf_take(b, 5, hdist) || !vf_inf_take(b, 4, hclen)) return VF_INF_SHORT;
    const int nlen = (int)hlit + 257, ndist = (int)hdist + 1, ncode = (int)hclen + 4;
    if (nlen > 286 || ndist > 30) return VF_INF_TOO_MANY;
    VF_INF_SYNC();
    for (int i = 0; i < kInfCodeLen; ++i) tb.lens[i] = 0;
    for (int i = 0; i < ncode; ++i) {
        if (!vf_inf_take(b, 3, v)) return VF_INF_SHORT;
        const int s = i < 3 ? 16 + i : (int)(((i < 11 ? order_lo : order_hi) >> (8 * ((i - 3) & 7))) & 255u);
        tb.lens[s] = (uint8_t)v;
    }
    bool single, none;
    if (vf_inf_count(tb.cl, tb.lens, kInfCodeLen, single, none) != 0) return VF_INF_CODE_LENGTHS;
    vf_inf_fill(tb.cl, lane, nlanes);
    int have = 0, prev = -1;
    while (have < nlen + ndist) {
        const int s = vf_inf_symbol(b, tb.cl);
        if (s < 0) return VF_INF_SHORT;         // (the code is complete: only the end of the stream stops it)
        if (s < 16) {
            tb.lens[have++] = (uint8_t)s;
            prev = s;
            continue;
        }
        int fill = 0, times;
        if (s == 16) {
            if (prev < 0) return VF_INF_REPEAT;
            if (!vf_inf_take(b, 2, v)) return VF_INF_SHORT;
            fill = prev;
            times = 3 + (int)v;
        } else {
            if (!vf_inf_take(b, s == 17 ? 3 : 7, v)) return VF_INF_SHORT;
            times = (s == 17 ? 3 : 11) + (int)v;
            prev = 0;
        }
        if (have + times > nlen + ndist) return VF_INF_REPEAT;
        for (int i = 0; i < times; ++i) tb.lens[have++] = (uint8_t)fill;
    }
    if (tb.lens[256] == 0) return VF_INF_NO_END;
    // the distance lengths move behind 288 literal/length lengths, last first (the two ranges may overlap)
    for (int i = ndist - 1; i >= 0; --i) tb.lens[kInfLitLen + i] = tb.lens[nlen + i];
    int left = vf_inf_count(tb.lit, tb.lens, nlen, single, none);
    if (left < 0 || (left > 0 && !single)) return VF_INF_LITLEN_SET;
    left = vf_inf_count(tb.dist, tb.lens + kInfLitLen, ndist, single, none);
    if (left < 0 || (left > 0 && !single && !none)) return VF_INF_DIST_SET;
    vf_inf_fill(tb.lit, lane, nlanes);
    vf_inf_fill(tb.dist, lane, nlanes);
    return VF_INF_OK;
}

// One token of a Huffman-coded block: a literal (length 0, `value` = the byte), the end of the block (length -1), or a match of
// `length` bytes from `value` bytes back.  Returns 0 or the status; a failed token has taken the bits in front of what failed.
struct VfInfToken {
    int length, value;
};
template <class Src>
VF_INF_HD int vf_inf_token(VfInfBits<Src>& b, const VfInfTables& tb, VfInfToken& t) {
    const int s = vf_inf_symbol(b, tb.lit);
    if (s < 0) return s == -2 ? VF_INF_SHORT : VF_INF_LITLEN_CODE;
    if (s < 256) { t.length = 0; t.value = s; return VF_INF_OK; }
    if (s == 256) { t.length = -1; t.value = 0; return VF_INF_OK; }
    if (s > 285) return VF_INF_LITLEN_CODE;
    unsigned v = 0;
    if (!vf_inf_take(b, vf_inf_len_extra(s - 257), v)) return VF_INF_SHORT;
    t.length = vf_inf_len_base(s - 257) + (int)v;
    const int d = vf_inf_symbol(b, tb.dist);
    if (d < 0) return d == -2 ? VF_INF_SHORT : VF_INF_DIST_CODE;
    if (d > 29) return VF_INF_DIST_CODE;
    v = 0;
    if (!vf_inf_take(b, vf_inf_dist_extra(d), v)) return VF_INF_SHORT;
    t.value = vf_inf_dist_base(d) + (int)v;
    return VF_INF_OK;
}

// the three bits in front of a block, and of a stored block LEN: 0 or the status.  Behind a stored block's header the reader stands
// on a byte boundary with nothing held: the block's bytes are stream[b.pos .. b.pos + len), and the caller moves b.pos past them.
template <class Src>
VF_INF_HD int vf_inf_block(VfInfBits<Src>& b, int& final_block, int& type, int& stored_len) {
    unsigned v;
    if (!vf_inf_take(b, 3, v)) return VF_INF_SHORT;
    final_block = (int)(v & 1u);
    type = (int)(v >> 1);
    stored_len = 0;
    if (type == 3) return VF_INF_BLOCK_TYPE;
    if (type != 0) return VF_INF_OK;
    b.acc >>= b.n & 7;
    b.n -= b.n & 7;
    if (!vf_inf_take(b, 32, v)) return VF_INF_SHORT;
    b.pos -= b.n >> 3;
    b.acc = 0;
    b.n = 0;
    if ((v & 0xFFFFu) != ((~v >> 16) & 0xFFFFu)) return VF_INF_STORED_LEN;
    stored_len = (int)(v & 0xFFFFu);
    if (b.end - b.pos < stored_len) return VF_INF_SHORT;
    return VF_INF_OK;
}

// ---- the whole stream, serially: the statement of what vface_png_inflate does to one file.  stream[0 .. len) -> out[0 .. produced),
// produced <= expect; consumed = whole bytes of the stream behind the last bit taken (len where the status is 1).  A token that
// fails (too far, too long) writes nothing.
VF_INF_HD int vf_inf_stream(const uint8_t* stream, long len, uint8_t* out, long expect, VfInfTables& tb, long& produced, long& consumed) {
    VfInfBits<VfInfHostSrc> b = {{stream}, 0, len, 0ull, 0};
    long p = 0;
    int status = VF_INF_OK, final_block = 0;
    while (status == VF_INF_OK && !final_block) {
        int type, stored;
        status = vf_inf_block(b, final_block, type, stored);
        if (status != VF_INF_OK) break;
        if (type == 0) {
            if (p + stored > expect) { status = VF_INF_TOO_LONG; break; }
            for (int i = 0; i < stored; ++i) out[p + i] = stream[b.pos + i];
            p += stored;
            b.pos += stored;
            continue;
        }
        if (type == 1) vf_inf_fixed_tables(tb, 0, 1);
        else status = vf_inf_dynamic_tables(b, tb, 0, 1);
        while (status == VF_INF_OK) {
            VfInfToken t;
            status = vf_inf_token(b, tb, t);
            if (status != VF_INF_OK || t.length < 0) break;
            if (t.length == 0) {
                if (p + 1 > expect) { status = VF_INF_TOO_LONG; break; }
                out[p++] = (uint8_t)t.value;
                continue;
            }
            if (t.value > p) { status = VF_INF_TOO_FAR; break; }
            if (p + t.length > expect) { status = VF_INF_TOO_LONG; break; }
            for (int i = 0; i < t.length; ++i) out[p + i] = out[p - t.value + i % t.value];
            p += t.length;
        }
    }
    if (status == VF_INF_OK && p != expect) status = VF_INF_TOO_FEW;
    produced = p;
    consumed = status == VF_INF_SHORT ? len : vf_inf_consumed(b);
    return status;
}
