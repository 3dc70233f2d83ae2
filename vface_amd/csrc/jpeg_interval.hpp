// The entropy decoder of one restart interval of a baseline 4:2:0 JPEG scan, written once for the device and the host.
//
// csrc/mjpeg_in.hip calls vf_jpeg_decode_interval from one lane per interval; tests/jpeg_interval_probe.cpp calls the same function
// from a plain C++ program under the address and undefined-behaviour sanitizers.  This is the one routine of the library whose
// control flow is steered by file bytes, so it is written to hold for EVERY input, not only for JPEG:
//   - every byte read is gated by `pos < end`; nothing before `begin` or at and after `end` is read;
//   - every table index is checked against the table before the load, every coefficient index is checked <= 63 before the store;
//   - every loop has a bound that does not depend on the bytes: the refill adds at most 8 bytes, a code has at most 16 bits, a
//     block has at most 63 AC symbols -- `blocks` x 64 symbols in all;
//   - nothing outside out[0 .. blocks * 64) is written.  The caller clears `out` first: blocks that are not reached stay zero.
// This file has no include of the HIP runtime: a C++17 host compiler reads it as it is.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define VF_JPEG_HD __host__ __device__ inline
#else
#define VF_JPEG_HD inline
#endif

// One Huffman table in the form the decoder reads (T.81 F.2.2.3, built by vface_amd/scripts/mjpeg_in.huffman_block):
//   maxcode[l - 1]  the largest code of length l, -1 where no code has that length
//   valoff[l - 1]   index into vals of the first symbol of length l, minus the smallest code of length l
//   vals            HUFFVAL, zero-padded
struct VfJpegHuff {
    int32_t maxcode[16];
    int32_t valoff[16];
    uint8_t vals[256];
};
// the tables of a frame by COMPONENT (Y, Cb, Cr), as its SOS names them: 6 x 384 = 2304 bytes
struct VfJpegTables {
    VfJpegHuff dc[3];
    VfJpegHuff ac[3];
};

// status of a frame: 0 = decoded; 1, 2 come from vface_jpeg_scan_index, the others from the interval decoder
enum VfJpegStatus {
    VF_JPEG_OK = 0,
    VF_JPEG_MARKER_COUNT = 1,   // the scan does not hold ceil(mcus / restart) - 1 RST markers
    VF_JPEG_MARKER_ORDER = 2,   // the markers do not run RST0, RST1, ... mod 8
    VF_JPEG_SHORT = 3,          // the bytes ran out before the blocks did
    VF_JPEG_BAD_CODE = 4,       // 16 bits that are no code of the table
    VF_JPEG_DC_CATEGORY = 5,    // a DC difference category above 11
    VF_JPEG_AC_SIZE = 6,        // an AC size above 10
    VF_JPEG_RUN = 7,            // a zero run that passes coefficient 63
    VF_JPEG_RANGE = 8,          // a DC value outside int16 after prediction
};

struct VfJpegBits {
    const uint8_t* bytes;
    long pos, end;
    unsigned long long acc;     // the low `n` bits are the next bits of the stream, most significant first
    int n;
};

// tops the window up to more than 56 bits where the interval has them.  FF 00 is the data byte FF; FF before anything else, or
// as the last byte, ends the data (a marker: the bytes behind it are not the interval's).
VF_JPEG_HD void vf_jpeg_refill(VfJpegBits& b) {
    for (int i = 0; i < 8 && b.n <= 56 && b.pos < b.end; ++i) {
        const unsigned v = b.bytes[b.pos];
        if (v == 0xFFu) {
            if (b.pos + 1 < b.end && b.bytes[b.pos + 1] == 0) {
                b.pos += 2;
            } else {
                b.pos = b.end;
                break;
            }
        } else {
            b.pos += 1;
        }
        b.acc = (b.acc << 8) | v;
        b.n += 8;
    }
}

// the next symbol of table `t`, or a negative status
VF_JPEG_HD int vf_jpeg_symbol(VfJpegBits& b, const VfJpegHuff* t) {
    vf_jpeg_refill(b);
    const unsigned peek = b.n >= 16 ? (unsigned)(b.acc >> (b.n - 16)) & 0xFFFFu : (unsigned)(b.acc << (16 - b.n)) & 0xFFFFu;
    for (int l = 1; l <= 16; ++l) {
        const int code = (int)(peek >> (16 - l));
        if (code <= t->maxcode[l - 1]) {
            if (l > b.n) return -VF_JPEG_SHORT;
            const long idx = (long)code + t->valoff[l - 1];       // (64 bits: the table's words are data too)
            if (idx < 0 || idx > 255) return -VF_JPEG_BAD_CODE;
            b.n -= l;
            return t->vals[idx];
        }
    }
    return b.n < 16 ? -VF_JPEG_SHORT : -VF_JPEG_BAD_CODE;
}

// `s` (1..15) further bits as the signed value of T.81 F.2.2.1 (EXTEND); `ok` goes false where the bits ran out
VF_JPEG_HD int vf_jpeg_receive_extend(VfJpegBits& b, int s, bool& ok) {
    vf_jpeg_refill(b);
    if (s > b.n) {
        ok = false;
        return 0;
    }
    const int v = (int)((b.acc >> (b.n - s)) & ((1ull << s) - 1ull));
    b.n -= s;
    return v < (1 << (s - 1)) ? v - (1 << s) + 1 : v;
}

// bytes[begin, end): one restart interval, without the RST marker behind it.  blocks = 6 x its MCUs, in the order Y00 Y01 Y10 Y11
// Cb Cr; out: blocks x 64 coefficients in zigzag order, cleared by the caller.  Returns a VfJpegStatus.  Bits left over at the end
// (the 1-padding, or more) are not looked at.
VF_JPEG_HD int vf_jpeg_decode_interval(const uint8_t* bytes, long begin, long end, const VfJpegTables* tables, int blocks,
                                       int16_t* out) {
    VfJpegBits b = {bytes, begin, end < begin ? begin : end, 0ull, 0};
    int pred[3] = {0, 0, 0};
    for (int blk = 0; blk < blocks; ++blk) {
        const int slot = blk % 6, comp = slot < 4 ? 0 : slot - 3;
        int16_t* o = out + (long)blk * 64;
        const int s = vf_jpeg_symbol(b, &tables->dc[comp]);
        if (s < 0) return -s;
        if (s > 11) return VF_JPEG_DC_CATEGORY;
        bool ok = true;
        if (s) pred[comp] += vf_jpeg_receive_extend(b, s, ok);
        if (!ok) return VF_JPEG_SHORT;
        if (pred[comp] < -32768 || pred[comp] > 32767) return VF_JPEG_RANGE;
        o[0] = (int16_t)pred[comp];
        int k = 1;
        for (int sym = 0; sym < 63 && k < 64; ++sym) {
            const int rs = vf_jpeg_symbol(b, &tables->ac[comp]);
            if (rs < 0) return -rs;
            const int r = rs >> 4, sz = rs & 15;
            if (sz == 0) {
                if (r != 15) break;         // EOB (libjpeg reads every r0 but ZRL as the end of the block)
                k += 16;
                continue;
            }
            if (sz > 10) return VF_JPEG_AC_SIZE;
            k += r;
            if (k > 63) return VF_JPEG_RUN;
            const int v = vf_jpeg_receive_extend(b, sz, ok);
            if (!ok) return VF_JPEG_SHORT;
            o[k] = (int16_t)v;
            k += 1;
        }
    }
    return VF_JPEG_OK;
}
