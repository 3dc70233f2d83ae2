// Decoding INSIDE a restart interval in parallel: the per-subsequence routine, written once for the device and the host.
//
// csrc/mjpeg_in_parallel.hip calls vf_jpeg_decode_subseq from one lane per subsequence; tests/jpeg_subseq_probe.cpp calls the same
// function from a plain C++ program under the address and undefined-behaviour sanitizers, with the lanes of a chunk as a loop.
//
// An interval bytes[begin, end) is cut into subsequences of `subseq_bytes` RAW scan bytes: subsequence i is
// [begin + i S, begin + (i + 1) S), and there are (end - begin) / S + 1 of them, so that the position `end` itself has an owner.
// A lane owns the SYMBOLS (a Huffman code with its extra bits) whose first bit lies in its subsequence.  The decoder's state
// between two symbols is VfJpegSubState: the position of the next bit, the slot 0..5 within the MCU and k 0..63 within the block
// (k = 0: the next symbol is a DC code).  The DC predictor and the absolute block number are not part of it: the caller recovers
// both by prefix sums (the blocks a lane began; the DC DIFFERENCES this routine writes).
//
// Positions are canonical, so that two lanes that reached the same bit compare equal: `pos` is the raw index of the data byte that
// holds the next bit -- never the 00 of an FF 00 pair -- and `bit` counts the bits of that byte already used, 0..7.
//
// A lane that decodes from a GUESSED state (vf_jpeg_subseq_guess: first bit of the subsequence, slot 0, k 0) reads bits that may
// be no symbol boundary at all, so the routine holds for every state and every byte, by the rules of jpeg_interval.hpp: every
// byte read is gated by `pos < end`, every table and coefficient index is checked before the access, the loop runs at most
// 8 S + 1 times whatever the bytes are, and only out[0 .. blocks * 64) is written.  What the serial routine reports as a fault is
// handled by ONE rule in every pass, so that the chain of verified states is the same in all of them:
//   - no code of the table, or a code whose symbol index lies outside the table: one bit is skipped, the state stays;
//   - a DC category above 11, an AC size above 10, a run past coefficient 63: the code's bits are used up, the state stays;
//   - the bits run out (inside a symbol or before one): the lane stops and its exit position is `end`.
// Every step therefore uses at least one bit or ends the lane.  In the write pass the first such condition met while the lane
// holds a block below `blocks` is returned; the caller then decodes the frame again with vf_jpeg_decode_interval, so status and
// partial output of a bad stream are the serial routine's by construction.
// This file has no include of the HIP runtime: a C++17 host compiler reads it as it is.
#pragma once
#include "jpeg_interval.hpp"

constexpr int kVfJpegSubseqMin = 4, kVfJpegSubseqMax = 1024;      // subseq_bytes: a multiple of 4 in this range
constexpr int kVfJpegLanesShort = 64, kVfJpegLanesLong = 256;     // lanes (subsequences) per chunk: the two instantiations

struct VfJpegSubState {
    int32_t pos;                // raw byte index (into the scan buffer) of the data byte that holds the next bit
    int32_t sk;                 // bit | slot << 3 | k << 6
};
VF_JPEG_HD bool vf_jpeg_sub_same(const VfJpegSubState& a, const VfJpegSubState& b) { return a.pos == b.pos && a.sk == b.sk; }

// the subsequences of an interval of n >= 0 bytes
VF_JPEG_HD long vf_jpeg_subseq_count(long n, int subseq_bytes) { return n / subseq_bytes + 1; }

// lanes per chunk the entry point picks for a call: the long form once the AVERAGE interval holds more subsequences than the
// short form has lanes.  Host arithmetic on the call's arguments only (vface_amd/hip.py jpeg_parallel_lanes is the same rule).
inline int vf_jpeg_subseq_lanes(long scan_bytes, long frames, long max_intervals, int subseq_bytes) {
    const long intervals = frames * max_intervals > 0 ? frames * max_intervals : 1;
    return scan_bytes / intervals / subseq_bytes >= kVfJpegLanesShort ? kVfJpegLanesLong : kVfJpegLanesShort;
}

// the state a lane guesses for the subsequence that begins at raw byte `at` (begin < at <= end): its first bit, slot 0, k 0.  A
// subsequence that begins on the 00 of an FF 00 pair skips it (inside live data a 00 behind FF is always stuffing).
VF_JPEG_HD VfJpegSubState vf_jpeg_subseq_guess(const uint8_t* bytes, long begin, long end, long at) {
    if (at > begin && at < end && bytes[at - 1] == 0xFFu && bytes[at] == 0) at += 1;
    return VfJpegSubState{(int32_t)at, 0};
}

// vf_jpeg_refill with one difference: a marker (FF before anything but 00, or FF as the last byte) ends the data by pulling `end`
// down to it, so that `pos` stays the index of the next byte that would be loaded.  After it either n > 56 or pos == end, and then
// the vf_jpeg_refill inside vf_jpeg_symbol / vf_jpeg_receive_extend loads nothing.
VF_JPEG_HD void vf_jpeg_sub_refill(VfJpegBits& b) {
    for (int i = 0; i < 8 && b.n <= 56 && b.pos < b.end; ++i) {
        const unsigned v = b.bytes[b.pos];
        if (v == 0xFFu) {
            if (b.pos + 1 < b.end && b.bytes[b.pos + 1] == 0) {
                b.pos += 2;
            } else {
                b.end = b.pos;
                break;
            }
        } else {
            b.pos += 1;
        }
        b.acc = (b.acc << 8) | v;
        b.n += 8;
    }
}

// the canonical position of the next bit: the window holds ceil(n / 8) data bytes, each FF among them took two raw bytes
VF_JPEG_HD void vf_jpeg_sub_position(const VfJpegBits& b, long& pos, int& bit) {
    const int held = (b.n + 7) >> 3;
    int raw = held;
    for (int j = 0; j < 8; ++j)
        if (j < held && ((b.acc >> (8 * j)) & 0xFFull) == 0xFFull) ++raw;
    pos = b.pos - raw;
    bit = (8 - (b.n & 7)) & 7;
}

// One subsequence.  bytes[begin, end): the interval; sub_end: the raw index behind the lane's subsequence (a symbol that would
// begin at or behind it is the next lane's); max_steps = 8 x subseq_bytes.  st: the start state on entry, the exit state on return
// -- except in the write pass, which leaves it alone.  begun: the blocks whose DC symbol this lane decoded.
// out == nullptr: a synchronisation pass; nothing is written, nothing is reported, the lane runs to the end of its subsequence.
// out != nullptr: the write pass from a VERIFIED start state.  first_block = the blocks begun before this lane (a lane that
//   starts inside a block, k > 0, continues block first_block - 1); out is the interval's blocks x 64 coefficients, cleared by the
//   caller; AC coefficients are written in zigzag order and the DC coefficient as its DIFFERENCE.  The lane stops at block
//   `blocks`; a lane whose first block lies at or behind it writes nothing and reports nothing.
// Returns 0, or in the write pass the VfJpegStatus (3..7) of the first condition the serial routine would report.
VF_JPEG_HD int vf_jpeg_decode_subseq(const uint8_t* bytes, long begin, long end, long sub_end, int max_steps, const VfJpegTables* tables,
                                     VfJpegSubState& st, int& begun, long first_block, int blocks, int16_t* out) {
    begun = 0;
    if (end < begin) end = begin;
    long at = st.pos < begin ? begin : (st.pos > end ? end : (long)st.pos);
    VfJpegBits b = {bytes, at, end, 0ull, 0};
    vf_jpeg_sub_refill(b);
    const int used = st.sk & 7;
    b.n = b.n >= used ? b.n - used : 0;
    int slot = (st.sk >> 3) & 7, k = (st.sk >> 6) & 63;
    if (slot > 5) slot = 0;
    long blk = first_block - (k > 0 ? 1 : 0);           // the block in hand (k > 0) or the next one to begin (k == 0)
    if (out && (blk < 0 || (k > 0 && blk >= blocks))) return VF_JPEG_OK;
    for (int step = 0; step <= max_steps; ++step) {
        vf_jpeg_sub_refill(b);
        long pos;
        int bit;
        vf_jpeg_sub_position(b, pos, bit);
        if (pos >= sub_end || step == max_steps) {
            if (!out) st = VfJpegSubState{(int32_t)pos, bit | slot << 3 | k << 6};
            return VF_JPEG_OK;
        }
        if (out && k == 0 && blk >= blocks) return VF_JPEG_OK;
        const int comp = slot < 4 ? 0 : slot - 3;
        int fault = 0;
        bool ok = true;
        if (b.n == 0) {
            fault = VF_JPEG_SHORT;
        } else if (k == 0) {
            const int s = vf_jpeg_symbol(b, &tables->dc[comp]);
            if (s < 0) {
                fault = -s;
            } else if (s > 11) {
                fault = VF_JPEG_DC_CATEGORY;
            } else {
                vf_jpeg_sub_refill(b);
                const int diff = s ? vf_jpeg_receive_extend(b, s, ok) : 0;
                if (!ok) {
                    fault = VF_JPEG_SHORT;
                } else {
                    if (out) out[blk * 64] = (int16_t)diff;
                    begun += 1;
                    k = 1;
                }
            }
        } else {
            const int rs = vf_jpeg_symbol(b, &tables->ac[comp]);
            const int r = rs >> 4, sz = rs & 15;
            bool done = false;
            if (rs < 0) {
                fault = -rs;
            } else if (sz == 0) {
                if (r != 15) done = true;               // EOB
                else if ((k += 16) >= 64) done = true;  // ZRL; past 63 the serial routine's block loop ends without a word
            } else if (sz > 10) {
                fault = VF_JPEG_AC_SIZE;
            } else if (k + r > 63) {
                fault = VF_JPEG_RUN;
            } else {
                vf_jpeg_sub_refill(b);
                const int v = vf_jpeg_receive_extend(b, sz, ok);
                if (!ok) {
                    fault = VF_JPEG_SHORT;
                } else {
                    k += r;
                    if (out) out[blk * 64 + k] = (int16_t)v;
                    if (++k == 64) done = true;
                }
            }
            if (done) {
                slot = slot == 5 ? 0 : slot + 1;
                k = 0;
                blk += 1;
            }
        }
        if (fault) {
            if (out) return fault;                      // (the lane holds a live block: checked above)
            if (fault == VF_JPEG_SHORT) {
                st = VfJpegSubState{(int32_t)end, slot << 3 | k << 6};
                return VF_JPEG_OK;
            }
            if (fault == VF_JPEG_BAD_CODE && b.n > 0) b.n -= 1;
        }
    }
    return VF_JPEG_OK;
}
