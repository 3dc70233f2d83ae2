// The LZW half of the GIF writer (REFace/scripts/VFace_inference_batch.py:658), written once for the device and the host:
// csrc/gif.hip runs the encoder on one lane per segment, tests/gif_probe.cpp runs it in a plain C++ program under the address and
// undefined-behaviour sanitizers, and tests/gif_model.py restates the format in Python.
//
// Minimum code size 8: Clear 256, end of information 257, first free code 258, 9 to 12 bits.  A segment is coded from an empty
// table: greedy longest match, every data code emitted assigns the next free code to (that code, the byte that followed).  When
// no code is free -- 4095 is assigned, 3839 data codes behind the last Clear -- the encoder emits Clear and goes on with an empty
// table.  The segment's terminator (Clear, or end of information behind a frame's last segment) follows its last data code.
// So a segment's codes come in periods of kGifLzwPeriod, and the k-th code of a period has a width that depends on k alone:
// 9 for k = 0, else min(12, max(9, bit length of 257 + k)) -- the decoder's table lags by one entry and the decoder widens when
// ITS next free code reaches 2^width.  vf_gif_lzw_bits(j) is therefore the bit offset of a segment's code j in closed form, and
// the packer places every code without a scan over widths.
// Greedy LZW output is unique: the table below is a detail.  It is a hash of (prefix << 8 | byte) into kGifLzwSlots words, linear
// probing, a word = key << 12 | code, 0 = empty (a code is at least 258).
// This file has no include of the HIP runtime: a C++17 host compiler reads it as it is.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define VF_LZW_HD __host__ __device__ inline
#else
#define VF_LZW_HD inline
#endif

constexpr int kGifClear = 256, kGifEoi = 257, kGifFirst = 258, kGifTable = 4096;
constexpr int kGifLzwPeriod = kGifTable - kGifFirst + 2;     // 3839 data codes and the forced Clear
constexpr int kGifLzwSlots = 8192;                           // at most 3838 entries live: under half full

struct VfGifLzwState {
    int32_t prefix;      // the code of the string matched so far; -1: none (a segment's start, or behind a forced Clear)
    int32_t next;        // the next free code
    int64_t count;       // codes written so far
};

VF_LZW_HD void vf_gif_lzw_begin(VfGifLzwState& st) { st.prefix = -1; st.next = kGifFirst; st.count = 0; }

VF_LZW_HD int64_t vf_gif_lzw_cum(int64_t k) {      // bits of the first k codes of a period
    return 9 * k + (k > 255 ? k - 255 : 0) + (k > 767 ? k - 767 : 0) + (k > 1791 ? k - 1791 : 0);
}
// bits of the first j codes of a segment
VF_LZW_HD int64_t vf_gif_lzw_bits(int64_t j) { return (j / kGifLzwPeriod) * vf_gif_lzw_cum(kGifLzwPeriod) + vf_gif_lzw_cum(j % kGifLzwPeriod); }
VF_LZW_HD int vf_gif_lzw_width(int64_t j) {
    const int64_t k = j % kGifLzwPeriod;
    return k >= 1791 ? 12 : k >= 767 ? 11 : k >= 255 ? 10 : 9;
}
// the most codes a segment of m indices can make: m data codes, a forced Clear behind every 3839 of them, the terminator
VF_LZW_HD int64_t vf_gif_lzw_max_codes(int64_t m) { return m + m / (kGifLzwPeriod - 1) + 1; }

VF_LZW_HD void vf_gif_lzw_emit(VfGifLzwState& st, int code, uint16_t* codes, int64_t cap) {
    if (st.count < cap) codes[st.count] = (uint16_t)code;
    ++st.count;
}

// the code of (prefix, byte), or -1: then, where a code is free, `next` now stands for it
VF_LZW_HD int vf_gif_lzw_find_or_add(uint32_t* table, int prefix, int byte, int next) {
    const uint32_t key = (uint32_t)prefix << 8 | (uint32_t)byte;
    uint32_t slot = (key * 2654435761u) >> 19;
    for (int probes = 0; probes < kGifLzwSlots; ++probes) {
        const uint32_t e = table[slot];
        if (e == 0) {
            if (next < kGifTable) table[slot] = key << 12 | (uint32_t)next;
            return -1;
        }
        if ((e >> 12) == key) return (int)(e & 4095u);
        slot = (slot + 1) & (kGifLzwSlots - 1);
    }
    return -1;      // not reached: the table is never full
}

// Codes up to m indices from px.  Returns how many were taken: m, or fewer when the table filled -- the forced Clear is
// written, st.prefix is -1, and the CALLER zeroes the table before the next call, which starts at the index not taken.
VF_LZW_HD int vf_gif_lzw_run(const uint8_t* px, int m, VfGifLzwState& st, uint32_t* table, uint16_t* codes, int64_t cap) {
    int i = 0;
    if (st.prefix < 0 && m > 0) st.prefix = px[i++];
    for (; i < m; ++i) {
        const int ch = px[i];
        const int hit = vf_gif_lzw_find_or_add(table, st.prefix, ch, st.next);
        if (hit >= 0) { st.prefix = hit; continue; }
        vf_gif_lzw_emit(st, st.prefix, codes, cap);
        if (st.next < kGifTable) {
            ++st.next;
            st.prefix = ch;
        } else {
            vf_gif_lzw_emit(st, kGifClear, codes, cap);
            st.next = kGifFirst;
            st.prefix = -1;
            return i;
        }
    }
    return m;
}

// the last data code and the terminator
VF_LZW_HD void vf_gif_lzw_finish(VfGifLzwState& st, bool last, uint16_t* codes, int64_t cap) {
    vf_gif_lzw_emit(st, st.prefix, codes, cap);
    vf_gif_lzw_emit(st, last ? kGifEoi : kGifClear, codes, cap);
}
