// The Huffman half of the PNG encoder's deflate blocks (REFace/scripts/VFace_inference_batch.py:636), written once for the
// device and the host: csrc/png.hip calls these routines from one lane per stripe, tests/png_huffman_probe.cpp calls them from a
// plain C++ program under the address and undefined-behaviour sanitizers, and tests/png_model.py restates them in Python.
//
// The two choices the format leaves open are made HERE:
//   1. Length-limited construction.  The used symbols are sorted by (count, symbol) ascending.  A Huffman tree is built over them by
//      the two-queue merge (leaves in one queue, merged nodes in creation order in the other; on equal weight the LEAF is taken
//      first, which gives the shallowest of the optimal trees).  Only the NUMBER of leaves per depth is kept.  Depths above the
//      limit are folded into the limit and the counts are repaired until the Kraft sum is exactly 1: while it is too large, one
//      code of the limit length is removed from the sum by turning one code of the longest shorter length l into two of l + 1
//      (the heuristic of zlib's gen_bitlen and miniz).  The lengths then go to the symbols by rank: the most frequent symbol takes
//      the shortest length; among equal counts the HIGHER symbol number is the more frequent rank.
//      One used symbol takes length 1 (an incomplete code, as deflate allows for a single distance code); none: all zero.
//   2. Code-length sequence of a dynamic header.  Runs of ZERO lengths use the repeat symbols: while a run has 11 or more left,
//      symbol 18 with min(run, 138); then 3..10 left: symbol 17; 1 or 2 left: literal zeros.  Symbol 16 is never used: non-zero
//      lengths are always written one by one.
// Canonical codes follow RFC 1951 3.2.2 and are returned bit-reversed, ready for deflate's LSB-first stream.
// This file has no include of the HIP runtime: a C++17 host compiler reads it as it is.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define VF_PNG_HD __host__ __device__ inline
#else
#define VF_PNG_HD inline
#endif

constexpr int kPngLitLen = 286;          // literals 0..255, end of block 256, length codes 257..285
constexpr int kPngCodeLen = 19;          // the code-length alphabet
constexpr int kPngMaxSyms = 288;
constexpr int kPngLitLenBits = 15;
constexpr int kPngCodeLenBits = 7;
constexpr int kPngSeq = kPngLitLen + 1;  // lengths a header carries: 286 lit/len (HLIT = 29) and one distance code (HDIST = 0)
// 3 block bits, HLIT 5, HDIST 5, HCLEN 4, 19 x 3, and kPngSeq lengths at 7 bits each when no run is found
constexpr int kPngMaxHeaderBits = 3 + 14 + kPngCodeLen * 3 + kPngSeq * kPngCodeLenBits;

struct VfPngHuffScratch {
    uint32_t leaf[kPngMaxSyms];          // counts of the used symbols, ascending
    uint32_t node[kPngMaxSyms];          // weights of the merged nodes, in creation order
    uint16_t sym[kPngMaxSyms];           // sym[rank] = symbol
    uint16_t leaf_parent[kPngMaxSyms];
    uint16_t node_parent[kPngMaxSyms];
    uint16_t node_depth[kPngMaxSyms];
    uint32_t per_len[32 + kPngMaxSyms];  // leaves per depth (a depth can reach the number of symbols - 1 before limiting)
    uint32_t next[17], cnt[17];          // the canonical assignment's counters (here, not on the stack: the device has no stack to spare)
};

// true where symbol a sorts before symbol b: (count, symbol) ascending
VF_PNG_HD bool vf_png_before(const uint32_t* count, int a, int b) { return count[a] < count[b] || (count[a] == count[b] && a < b); }

// rank of used symbol i among the used symbols of count[0 .. n): how many sort before it.  The device calls it from one lane per symbol.
VF_PNG_HD int vf_png_rank(const uint32_t* count, int n, int i) {
    int r = 0;
    for (int j = 0; j < n; ++j)
        if (count[j] != 0 && vf_png_before(count, j, i)) ++r;
    return r;
}

// s.sym[0 .. used) and s.leaf[0 .. used) hold the used symbols and their counts in ascending order -> len[0 .. n): code lengths,
// none above maxbits (2^maxbits >= used).
VF_PNG_HD void vf_png_lengths_from_sorted(int used, int n, int maxbits, uint8_t* len, VfPngHuffScratch& s) {
    for (int i = 0; i < n; ++i) len[i] = 0;
    if (used <= 0) return;
    if (used == 1) { len[s.sym[0]] = 1; return; }
    // two-queue merge
    int li = 0, ni = 0;
    for (int k = 0; k < used - 1; ++k) {
        uint32_t w = 0;
        for (int pick = 0; pick < 2; ++pick) {
            if (li < used && (ni >= k || s.leaf[li] <= s.node[ni])) { w += s.leaf[li]; s.leaf_parent[li++] = (uint16_t)k; }
            else { w += s.node[ni]; s.node_parent[ni++] = (uint16_t)k; }
        }
        s.node[k] = w;
    }
    const int top = used + 31;
    for (int d = 0; d <= top; ++d) s.per_len[d] = 0;
    s.node_depth[used - 2] = 0;
    for (int k = used - 3; k >= 0; --k) s.node_depth[k] = (uint16_t)(s.node_depth[s.node_parent[k]] + 1);
    for (int i = 0; i < used; ++i) ++s.per_len[s.node_depth[s.leaf_parent[i]] + 1];
    // the limit: fold, then repair the Kraft sum (in units of 2^-maxbits)
    for (int d = maxbits + 1; d <= top; ++d) { s.per_len[maxbits] += s.per_len[d]; s.per_len[d] = 0; }
    uint32_t kraft = 0;
    for (int d = 1; d <= maxbits; ++d) kraft += s.per_len[d] << (maxbits - d);
    while (kraft > (1u << maxbits)) {
        --s.per_len[maxbits];
        for (int d = maxbits - 1; d >= 1; --d)
            if (s.per_len[d]) { --s.per_len[d]; s.per_len[d + 1] += 2; break; }
        --kraft;
    }
    // by rank: the most frequent symbols take the shortest lengths
    int r = used;
    for (int d = 1; d <= maxbits; ++d)
        for (uint32_t c = s.per_len[d]; c > 0; --c) len[s.sym[--r]] = (uint8_t)d;
}

// len[0 .. n) -> code[0 .. n): the canonical codes (RFC 1951 3.2.2), bit-reversed; 0 where len is 0
VF_PNG_HD void vf_png_canonical(const uint8_t* len, int n, uint16_t* code, VfPngHuffScratch& s) {
    uint32_t* next = s.next;
    uint32_t* cnt = s.cnt;
    for (int d = 0; d <= 16; ++d) cnt[d] = 0;
    for (int i = 0; i < n; ++i) ++cnt[len[i] & 15];
    cnt[0] = 0;
    uint32_t c = 0;
    next[0] = 0;
    for (int d = 1; d <= 16; ++d) { c = (c + cnt[d - 1]) << 1; next[d] = c; }
    for (int i = 0; i < n; ++i) {
        const int d = len[i] & 15;
        uint32_t v = d ? next[d]++ : 0, rev = 0;
        for (int b = 0; b < d; ++b) { rev = (rev << 1) | (v & 1); v >>= 1; }
        code[i] = (uint16_t)rev;
    }
}

// The whole routine: count[0 .. n) (n <= 288) -> lengths limited to maxbits and bit-reversed canonical codes.
VF_PNG_HD void vf_png_huffman(const uint32_t* count, int n, int maxbits, uint8_t* len, uint16_t* code, VfPngHuffScratch& s) {
    int used = 0;
    for (int i = 0; i < n; ++i) {
        if (count[i] == 0) continue;
        int at = used++;                 // insertion sort, ascending
        while (at > 0 && vf_png_before(count, i, s.sym[at - 1])) { s.sym[at] = s.sym[at - 1]; --at; }
        s.sym[at] = (uint16_t)i;
    }
    for (int r = 0; r < used; ++r) s.leaf[r] = count[s.sym[r]];
    vf_png_lengths_from_sorted(used, n, maxbits, len, s);
    vf_png_canonical(len, n, code, s);
}

// seq[0 .. n): the code lengths a header carries -> out[0 .. returned): symbols of the code-length alphabet, each (symbol |
// extra << 8), extra = the repeat count less 3 (symbol 17) or less 11 (symbol 18).  out holds n entries.
VF_PNG_HD int vf_png_code_length_symbols(const uint8_t* seq, int n, uint16_t* out) {
    int m = 0;
    for (int i = 0; i < n;) {
        if (seq[i] != 0) { out[m++] = seq[i++]; continue; }
        int run = 1;
        while (i + run < n && seq[i + run] == 0) ++run;
        i += run;
        while (run >= 11) { const int take = run < 138 ? run : 138; out[m++] = (uint16_t)(18 | ((take - 11) << 8)); run -= take; }
        if (run >= 3) { out[m++] = (uint16_t)(17 | ((run - 3) << 8)); run = 0; }
        while (run-- > 0) out[m++] = 0;
    }
    return m;
}

// deflate's length codes: symbol 257 + i stands for lengths kPngLenBase[i] .. with kPngLenExtra[i] extra bits
VF_PNG_HD int vf_png_len_base(int i) {
    return i < 8 ? 3 + i : (i == 28 ? 258 : 3 + ((4 + (i & 3)) << ((i >> 2) - 1)));
}
VF_PNG_HD int vf_png_len_extra(int i) { return (i < 8 || i == 28) ? 0 : (i >> 2) - 1; }
// length 3 .. 258 -> index of its length code, 0 .. 28
VF_PNG_HD int vf_png_len_index(int length) {
    if (length == 258) return 28;
    const int v = length - 3;
    if (v < 8) return v;
    int e = 0;
    while ((v >> (e + 3)) != 0) ++e;     // v >> e is in 4 .. 7
    return 4 * e + (v >> e);
}
