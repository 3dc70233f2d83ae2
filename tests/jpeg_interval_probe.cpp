// A stand-alone host program around vf_jpeg_decode_interval (vface_amd/csrc/jpeg_interval.hpp), the routine the entropy decoder's
// kernel runs per lane, built by tests/test_mjpeg_in_cpu.py with -fsanitize=address,undefined.  The routine is steered by file bytes;
// here every buffer it is given is a heap allocation of exactly the promised size, so a load or store outside one ends the run.
//
//   jpeg_interval_probe CASES MUTATIONS SEED
//
// CASES, little-endian, one record after another:
//   u32 scan_bytes, the scan;  u32 begin, u32 end (the interval);  2304 table bytes (VfJpegTables);  u32 blocks;
//   u32 status the model expects;  blocks x 64 int16 the model expects (what it decoded before a fault, zeros behind).
// Every record is decoded twice: inside the whole scan at [begin, end), and as a copy of exactly the interval's bytes at [0, n);
// status and coefficients must equal the record's.  Then MUTATIONS seeded mutations of the records that decoded (bytes flipped,
// the interval cut short, FF xx inserted; one in eight with a byte of the tables overwritten as well) are decoded from exact-size
// copies: any status 0..8 passes, any sanitizer report fails.
// Prints "cases N mutations M" and a histogram of the mutations' statuses; exits 0 when everything held.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "jpeg_interval.hpp"

namespace {

struct Case {
    std::vector<uint8_t> scan;
    uint32_t begin, end, blocks, status;
    VfJpegTables tables;
    std::vector<int16_t> want;
};

bool read_exact(FILE* f, void* p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }

// decodes bytes[begin, end) of a heap copy of exactly `n` bytes into a heap buffer of exactly blocks x 64 coefficients
int decode(const uint8_t* src, size_t n, long begin, long end, const VfJpegTables& tables, uint32_t blocks, std::vector<int16_t>& got) {
    uint8_t* bytes = (uint8_t*)malloc(n ? n : 1);
    if (n) memcpy(bytes, src, n);
    VfJpegTables* t = (VfJpegTables*)malloc(sizeof(VfJpegTables));
    memcpy(t, &tables, sizeof(VfJpegTables));
    int16_t* out = (int16_t*)calloc((size_t)blocks * 64 ? (size_t)blocks * 64 : 1, sizeof(int16_t));
    const int status = vf_jpeg_decode_interval(n ? bytes : nullptr, begin, end, t, (int)blocks, out);
    got.assign(out, out + (size_t)blocks * 64);
    free(out);
    free(t);
    free(bytes);
    return status;
}

uint64_t rng_state;
uint32_t rnd() {
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 7;
    rng_state ^= rng_state << 17;
    return (uint32_t)(rng_state >> 16);
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 4) {
        fprintf(stderr, "usage: %s CASES MUTATIONS SEED\n", argv[0]);
        return 2;
    }
    static_assert(sizeof(VfJpegTables) == 2304, "the table block of vface_amd/scripts/mjpeg_in.py");
    FILE* f = fopen(argv[1], "rb");
    if (!f) {
        fprintf(stderr, "cannot open %s\n", argv[1]);
        return 2;
    }
    const long mutations = atol(argv[2]);
    rng_state = 0x9E3779B97F4A7C15ull ^ (uint64_t)atoll(argv[3]);
    std::vector<Case> cases;
    for (;;) {
        Case c;
        uint32_t n;
        if (fread(&n, 4, 1, f) != 1) break;
        c.scan.resize(n);
        bool ok = read_exact(f, c.scan.data(), n) && read_exact(f, &c.begin, 4) && read_exact(f, &c.end, 4) &&
                  read_exact(f, &c.tables, sizeof(VfJpegTables)) && read_exact(f, &c.blocks, 4) && read_exact(f, &c.status, 4);
        if (ok) {
            c.want.resize((size_t)c.blocks * 64);
            ok = read_exact(f, c.want.data(), c.want.size() * 2);
        }
        if (!ok || c.begin > c.end || c.end > n) {
            fprintf(stderr, "record %zu of %s is malformed\n", cases.size(), argv[1]);
            return 2;
        }
        cases.push_back(std::move(c));
    }
    fclose(f);
    int failures = 0;
    std::vector<int16_t> got;
    for (size_t i = 0; i < cases.size(); ++i) {
        const Case& c = cases[i];
        for (int form = 0; form < 2; ++form) {
            const int status = form == 0 ? decode(c.scan.data(), c.scan.size(), c.begin, c.end, c.tables, c.blocks, got)
                                         : decode(c.scan.data() + c.begin, c.end - c.begin, 0, c.end - c.begin, c.tables, c.blocks, got);
            if (status != (int)c.status || got != c.want) {
                size_t at = 0;
                while (at < got.size() && got[at] == c.want[at]) ++at;
                fprintf(stderr, "case %zu form %d: status %d, the model says %u; first difference at coefficient %zu of %zu\n", i, form,
                        status, c.status, at, got.size());
                ++failures;
            }
        }
    }
    std::vector<size_t> valid;
    for (size_t i = 0; i < cases.size(); ++i)
        if (cases[i].status == 0 && cases[i].end - cases[i].begin >= 4 && cases[i].end - cases[i].begin <= 4096) valid.push_back(i);
    long histogram[16] = {0};
    long done = 0;
    for (; done < mutations && !valid.empty(); ++done) {
        const Case& c = cases[valid[rnd() % valid.size()]];
        std::vector<uint8_t> b(c.scan.begin() + c.begin, c.scan.begin() + c.end);
        const int edits = 1 + rnd() % 3;
        for (int e = 0; e < edits && !b.empty(); ++e) {
            const uint32_t kind = rnd() % 4, at = rnd() % b.size();
            if (kind == 0) b[at] ^= (uint8_t)(1u << (rnd() % 8));                   // one bit
            else if (kind == 1) b[at] = (uint8_t)rnd();                             // one byte
            else if (kind == 2) b.resize(at);                                       // cut short
            else {                                                                  // FF xx inserted
                const uint8_t ins[2] = {0xFF, (uint8_t)rnd()};
                b.insert(b.begin() + at, ins, ins + 2);
            }
        }
        VfJpegTables tables = c.tables;
        if (rnd() % 8 == 0) ((uint8_t*)&tables)[rnd() % sizeof(VfJpegTables)] = (uint8_t)rnd();      // and a table the parser did not make
        const int status = decode(b.data(), b.size(), 0, (long)b.size(), tables, c.blocks, got);
        if (status < 0 || status > 8) {
            fprintf(stderr, "mutation %ld: status %d\n", done, status);
            ++failures;
        } else {
            ++histogram[status];
        }
    }
    printf("cases %zu mutations %ld\n", cases.size(), done);
    for (int s = 0; s <= 8; ++s) printf("status %d: %ld\n", s, histogram[s]);
    return failures ? 1 : 0;
}
