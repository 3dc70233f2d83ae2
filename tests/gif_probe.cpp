// csrc/gif_palette.hpp and csrc/gif_lzw.hpp as a plain host program (tests/test_gif_cpu.py compiles it with
// -fsanitize=address,undefined): the median cut and the LZW encoder exactly as the kernels of csrc/gif.hip call them.
// Input: records, little endian.
//   'H', int32 n, n x (uint32 cell, uint32 count)        -> "boxes <ncolors> <label of every listed cell>"
//   'S', int32 n, int32 last, n bytes                    -> "codes <bits> <code> <code> ..."
// The program itself checks: an empty cell keeps label 0; every box's extent, population and cell count equal a recount; the
// encoder staged in pieces of 1024, 7 and n indices writes the same codes; their number stays within vf_gif_lzw_max_codes, in
// buffers of exactly that size; vf_gif_lzw_bits equals the sum of vf_gif_lzw_width.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "gif_lzw.hpp"
#include "gif_palette.hpp"

static void die(const char* what, long record) {
    std::fprintf(stderr, "record %ld: %s\n", record, what);
    std::exit(2);
}

static std::vector<uint16_t> encode(const std::vector<uint8_t>& px, bool last, int piece, long record) {
    const int n = (int)px.size();
    const int64_t cap = vf_gif_lzw_max_codes(n);
    std::vector<uint16_t> codes((size_t)cap);
    std::vector<uint32_t> table(kGifLzwSlots);
    std::vector<uint8_t> stage((size_t)piece);
    VfGifLzwState st;
    vf_gif_lzw_begin(st);
    bool clear = true;
    int pos = 0;
    while (pos < n) {
        if (clear) std::fill(table.begin(), table.end(), 0u);
        const int m = n - pos < piece ? n - pos : piece;
        std::memcpy(stage.data(), px.data() + pos, (size_t)m);
        const int took = vf_gif_lzw_run(stage.data(), m, st, table.data(), codes.data(), cap);
        if (took < 0 || took > m) die("the encoder took more than it was given", record);
        clear = took < m;
        pos += took;
    }
    vf_gif_lzw_finish(st, last, codes.data(), cap);
    if (st.count > cap) die("more codes than vf_gif_lzw_max_codes", record);
    codes.resize((size_t)st.count);
    return codes;
}

int main(int argc, char** argv) {
    if (argc != 2) return 1;
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 1;
    std::vector<uint32_t> counts(kGifCells);
    std::vector<uint8_t> labels(kGifCells);
    std::vector<VfGifBox> boxes(kGifColors);
    long records = 0;
    for (int kind; (kind = std::fgetc(f)) != EOF; ++records) {
        int32_t n = 0;
        if (std::fread(&n, 4, 1, f) != 1 || n < 1) die("bad record", records);
        if (kind == 'H') {
            std::vector<uint32_t> pairs((size_t)n * 2);
            if (std::fread(pairs.data(), 8, (size_t)n, f) != (size_t)n) die("short record", records);
            std::fill(counts.begin(), counts.end(), 0u);
            for (int i = 0; i < n; ++i) counts[pairs[2 * i] % kGifCells] = pairs[2 * i + 1];
            const int nc = vf_gif_boxes_serial(counts.data(), labels.data(), boxes.data());
            if (nc < 1 || nc > kGifColors) die("ncolors out of range", records);
            for (int i = 0; i < nc; ++i) {
                VfGifBox again;
                vf_gif_box_reset(again);
                for (int c = 0; c < kGifCells; ++c)
                    if (counts[c] && labels[c] == i) vf_gif_box_add(again, c, counts[c]);
                if (again.ncells < 1 || std::memcmp(&again, &boxes[i], sizeof again) != 0) die("a box differs from its recount", records);
            }
            for (int c = 0; c < kGifCells; ++c)
                if ((!counts[c] && labels[c]) || labels[c] >= nc) die("a label out of place", records);
            std::printf("boxes %d", nc);
            for (int i = 0; i < n; ++i) std::printf(" %d", (int)labels[pairs[2 * i] % kGifCells]);
            std::printf("\n");
        } else if (kind == 'S') {
            int32_t last = 0;
            if (std::fread(&last, 4, 1, f) != 1) die("short record", records);
            std::vector<uint8_t> px((size_t)n);
            if (std::fread(px.data(), 1, (size_t)n, f) != (size_t)n) die("short record", records);
            const std::vector<uint16_t> codes = encode(px, last != 0, 1024, records);
            if (codes != encode(px, last != 0, 7, records) || codes != encode(px, last != 0, n, records)) die("the staging changes the codes", records);
            int64_t bits = 0;
            for (size_t j = 0; j < codes.size(); ++j) {
                if (vf_gif_lzw_bits((int64_t)j) != bits) die("vf_gif_lzw_bits is not the sum of the widths", records);
                if (codes[j] >> vf_gif_lzw_width((int64_t)j)) die("a code wider than its width", records);
                bits += vf_gif_lzw_width((int64_t)j);
            }
            std::printf("codes %lld", (long long)bits);
            for (uint16_t c : codes) std::printf(" %d", (int)c);
            std::printf("\n");
        } else {
            die("unknown record", records);
        }
    }
    std::fclose(f);
    std::printf("records %ld\n", records);
    return 0;
}
