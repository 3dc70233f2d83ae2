// csrc/png_huffman.hpp -- the routines one lane of vface_png_deflate runs per stripe -- as a host program, built with
// -fsanitize=address,undefined by tests/test_png_cpu.py.
//
//   png_huffman_probe cases.bin
// cases.bin: records of int32 n, int32 maxbits, uint32 count[n].  For every record the program builds the lengths and the codes
// twice -- by vf_png_huffman (its own insertion sort) and the way the kernel does (vf_png_rank per symbol, then
// vf_png_lengths_from_sorted and vf_png_canonical) -- and checks: both agree; no length above maxbits; a length exactly where a
// count is; Kraft sum = 1 (1/2 for a single symbol); no two symbols share a (code, length); the header's code-length symbols expand
// back to the lengths.  It prints one line per record, "lengths l0 l1 ...", which the test compares with tests/png_model.py's.
// Every buffer is a heap allocation of exactly the promised size.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "png_huffman.hpp"

static int fail(long rec, const char* what) {
    std::printf("record %ld: %s\n", rec, what);
    return 1;
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    std::FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    // the length codes: every length 3 .. 258 lies in its code's range
    for (int length = 3; length <= 258; ++length) {
        const int i = vf_png_len_index(length);
        if (i < 0 || i > 28) return fail(-1, "length index out of range");
        const int extra = length - vf_png_len_base(i);
        if (extra < 0 || extra >= (1 << vf_png_len_extra(i))) return fail(-1, "length outside its code");
        if (i < 28 && vf_png_len_base(i + 1) <= length) return fail(-1, "a later code holds the length");
    }
    long rec = 0;
    int32_t head[2];
    while (std::fread(head, sizeof(int32_t), 2, f) == 2) {
        const int n = head[0], maxbits = head[1];
        if (n < 1 || n > kPngMaxSyms || maxbits < 1 || maxbits > 15) return fail(rec, "bad record");
        std::unique_ptr<uint32_t[]> count(new uint32_t[n]);
        if (std::fread(count.get(), sizeof(uint32_t), n, f) != (size_t)n) return fail(rec, "short record");
        std::unique_ptr<uint8_t[]> len(new uint8_t[n]), len2(new uint8_t[n]);
        std::unique_ptr<uint16_t[]> code(new uint16_t[n]), code2(new uint16_t[n]);
        std::unique_ptr<VfPngHuffScratch> s(new VfPngHuffScratch), s2(new VfPngHuffScratch);
        vf_png_huffman(count.get(), n, maxbits, len.get(), code.get(), *s);
        // the kernel's way: one lane per symbol ranks it
        int used = 0;
        for (int i = 0; i < n; ++i)
            if (count[i]) {
                const int r = vf_png_rank(count.get(), n, i);
                if (r < 0 || r >= n) return fail(rec, "rank out of range");
                s2->sym[r] = (uint16_t)i;
                s2->leaf[r] = count[i];
                ++used;
            }
        vf_png_lengths_from_sorted(used, n, maxbits, len2.get(), *s2);
        vf_png_canonical(len2.get(), n, code2.get(), *s2);
        if (std::memcmp(len.get(), len2.get(), n) || std::memcmp(code.get(), code2.get(), n * sizeof(uint16_t))) return fail(rec, "the two ways differ");
        unsigned long kraft = 0;
        for (int i = 0; i < n; ++i) {
            if ((count[i] != 0) != (len[i] != 0)) return fail(rec, "a length without a count, or a count without a length");
            if (len[i] > maxbits) return fail(rec, "a length above the limit");
            if (len[i]) kraft += 1ul << (maxbits - len[i]);
            if (len[i] && (code[i] >> len[i])) return fail(rec, "a code wider than its length");
        }
        if (used >= 2 && kraft != (1ul << maxbits)) return fail(rec, "Kraft sum is not 1");
        if (used == 1 && kraft != (1ul << (maxbits - 1))) return fail(rec, "a single symbol does not take one bit");
        for (int i = 0; i < n; ++i)
            for (int j = i + 1; j < n; ++j)
                if (len[i] && len[i] == len[j] && code[i] == code[j]) return fail(rec, "two symbols share a code");
        // the header's sequence expands back to the lengths
        std::unique_ptr<uint16_t[]> cl(new uint16_t[n]);
        const int m = vf_png_code_length_symbols(len.get(), n, cl.get());
        if (m < 0 || m > n) return fail(rec, "code-length symbols out of range");
        int at = 0;
        for (int i = 0; i < m; ++i) {
            const int sym = cl[i] & 255, extra = cl[i] >> 8;
            if (sym == 16 || sym > 18) return fail(rec, "a symbol the layout never uses");
            const int reps = sym == 17 ? 3 + extra : sym == 18 ? 11 + extra : 1;
            if ((sym == 17 && extra > 7) || (sym == 18 && extra > 127)) return fail(rec, "a repeat count out of range");
            for (int k = 0; k < reps; ++k, ++at)
                if (at >= n || len[at] != (sym < 16 ? sym : 0)) return fail(rec, "the sequence does not expand to the lengths");
        }
        if (at != n) return fail(rec, "the sequence is short");
        std::printf("lengths");
        for (int i = 0; i < n; ++i) std::printf(" %d", len[i]);
        std::printf("\n");
        ++rec;
    }
    std::fclose(f);
    std::printf("records %ld\n", rec);
    return 0;
}
