// csrc/png_inflate.hpp's serial routine as a host program (tests/test_png_in_cpu.py builds it with -fsanitize=address,undefined and
// compares what it writes with tests/png_inflate_model.py).  Every stream and every output stands in a heap block of exactly its
// size, so that a byte read or written outside it is the sanitizer's to report.
//   in:  records of  int32 length, int32 expect, length bytes
//   out: records of  int32 status, int32 produced, int32 consumed, produced bytes
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>

#include "png_inflate.hpp"

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* in = fopen(argv[1], "rb");
    FILE* out = fopen(argv[2], "wb");
    if (!in || !out) return 2;
    std::unique_ptr<VfInfTables> tables(new VfInfTables);
    long records = 0;
    int32_t head[2];
    while (fread(head, sizeof(int32_t), 2, in) == 2) {
        const long n = head[0], expect = head[1];
        if (n < 0 || expect < 0) return 3;
        uint8_t* stream = (uint8_t*)malloc(n ? n : 1);
        uint8_t* bytes = (uint8_t*)malloc(expect ? expect : 1);
        if (!stream || !bytes || (n && fread(stream, 1, n, in) != (size_t)n)) return 3;
        memset(tables.get(), 0xA5, sizeof(VfInfTables));       // a table entry that is read was built for THIS block
        long produced = -1, consumed = -1;
        const int status = vf_inf_stream(stream, n, bytes, expect, *tables, produced, consumed);
        if (produced < 0 || produced > expect || consumed < 0 || consumed > n) return 4;
        const int32_t result[3] = {status, (int32_t)produced, (int32_t)consumed};
        fwrite(result, sizeof(int32_t), 3, out);
        fwrite(bytes, 1, produced, out);
        free(stream);
        free(bytes);
        ++records;
    }
    fclose(in);
    if (fclose(out) != 0) return 5;
    printf("records %ld\n", records);
    return 0;
}
