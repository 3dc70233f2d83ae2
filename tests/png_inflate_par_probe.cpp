// csrc/png_inflate_par.hpp's host routine as a host program (tests/test_png_in_parallel_cpu.py builds it with
// -fsanitize=address,undefined and compares what it writes with tests/png_inflate_par_model.py).  Every stream, plane, segment table
// and output stands in a heap block of exactly its size, so that a byte read or written outside it is the sanitizer's to report.
//   in:  records of  int32 length, int32 expect, int32 chunk_bytes, length bytes
//   out: records of  int32 status, produced, consumed, s1, s2, info[4], candidates; int64 per candidate; produced bytes
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>

#include "png_inflate_par.hpp"

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* in = fopen(argv[1], "rb");
    FILE* out = fopen(argv[2], "wb");
    if (!in || !out) return 2;
    std::unique_ptr<VfInfTables> tables(new VfInfTables);
    long records = 0;
    int32_t head[3];
    while (fread(head, sizeof(int32_t), 3, in) == 3) {
        const long n = head[0], expect = head[1];
        const int chunk_bytes = head[2];
        if (n < 0 || expect <= 0 || chunk_bytes < kInfParMinChunk || chunk_bytes > kInfParMaxChunk || chunk_bytes % 4) return 3;
        const long chunks = vf_inf_par_chunks(n, chunk_bytes);
        uint8_t* stream = (uint8_t*)malloc(n ? n : 1);
        uint8_t* bytes = (uint8_t*)malloc(expect);
        uint16_t* plane = (uint16_t*)malloc(expect * sizeof(uint16_t));
        VfInfSegment* segs = (VfInfSegment*)malloc(chunks * sizeof(VfInfSegment));
        long* candidates = (long*)malloc((chunks > 1 ? chunks - 1 : 1) * sizeof(long));
        if (!stream || !bytes || !plane || !segs || !candidates || (n && fread(stream, 1, n, in) != (size_t)n)) return 3;
        memset(tables.get(), 0xA5, sizeof(VfInfTables));       // a table entry that is read was built for THIS block
        memset(plane, 0xEE, expect * sizeof(uint16_t));        // an element that is resolved was written for THIS stream
        long produced = -1, consumed = -1;
        unsigned adler[2] = {0, 0};
        int info[4] = {-1, -1, -1, -1};
        const int status = vf_inf_stream_parallel(stream, n, bytes, expect, chunk_bytes, *tables, plane, segs, candidates, produced, consumed,
                                                  adler, info);
        if (produced < 0 || produced > expect || consumed < 0 || consumed > n || info[2] < 0 || info[2] >= chunks) return 4;
        const int32_t result[10] = {status, (int32_t)produced, (int32_t)consumed, (int32_t)adler[0], (int32_t)adler[1],
                                    info[0], info[1], info[2], info[3], info[2]};
        fwrite(result, sizeof(int32_t), 10, out);
        for (int i = 0; i < info[2]; ++i) {
            const int64_t p = candidates[i];
            fwrite(&p, sizeof(int64_t), 1, out);
        }
        fwrite(bytes, 1, produced, out);
        free(stream);
        free(bytes);
        free(plane);
        free(segs);
        free(candidates);
        ++records;
    }
    fclose(in);
    if (fclose(out) != 0) return 5;
    printf("records %ld\n", records);
    return 0;
}
