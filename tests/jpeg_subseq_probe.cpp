// A stand-alone host program around vf_jpeg_decode_subseq (vface_amd/csrc/jpeg_subseq.hpp), the routine the parallel entropy
// decoder's kernel runs per lane, built by tests/test_mjpeg_in_parallel_cpu.py with -fsanitize=address,undefined.  It is the kernel
// jpeg_decode_parallel_kernel of csrc/mjpeg_in.hip with the lanes of a chunk as a loop: guessed states, rounds until nothing
// changes, the chunk's carry, the prefix sum of the blocks begun, the write pass, the DC pass, and the serial routine for whatever
// the serial routine would refuse.  Every buffer is a heap allocation of exactly the promised size.
//
//   jpeg_subseq_probe CASES MUTATIONS SEED SUBSEQ_BYTES LANES
//
// CASES: the records of tests/jpeg_interval_probe.cpp.  Every record is decoded inside the whole scan and as an exact copy of the
// interval; status and coefficients must equal the record's AND vf_jpeg_decode_interval's.  Then MUTATIONS seeded mutations (the
// kinds of jpeg_interval_probe.cpp) must give vf_jpeg_decode_interval's status and coefficients.
// Prints "cases N mutations M", one line "record I subsequences S chunks C rounds R" per record, and a histogram of the mutations'
// statuses; exits 0 when everything held.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "jpeg_subseq.hpp"

namespace {

struct Case {
    std::vector<uint8_t> scan;
    uint32_t begin, end, blocks, status;
    VfJpegTables tables;
    std::vector<int16_t> want;
};

bool read_exact(FILE* f, void* p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }

int subseq_bytes = 128, lanes = 64;

struct Counts {
    long subsequences, chunks, rounds;
};

// one interval, as one workgroup of the kernel decodes it; out: blocks x 64, cleared
int decode_parallel(const uint8_t* bytes, long begin, long end, const VfJpegTables* tables, int blocks, int16_t* out, Counts& counts) {
    const int L = lanes, S = subseq_bytes, max_steps = 8 * S;
    const long nsub = vf_jpeg_subseq_count(end - begin, S);
    counts = {nsub, 0, 0};
    std::vector<VfJpegSubState> start(L), reached(L), want(L);
    std::vector<int> begun(L);
    VfJpegSubState carry = {(int32_t)begin, 0};
    long blocks_before = 0;
    bool fault = false;
    for (long c0 = 0; c0 < nsub; c0 += L) {
        const int live = (int)(nsub - c0 < L ? nsub - c0 : L);
        counts.chunks += 1;
        for (int t = 0; t < live; ++t) {
            const long sub_begin = begin + (c0 + t) * S;
            start[t] = t ? vf_jpeg_subseq_guess(bytes, begin, end, sub_begin) : carry;
            reached[t] = start[t];
            vf_jpeg_decode_subseq(bytes, begin, end, sub_begin + S, max_steps, tables, reached[t], begun[t], 0, 0, nullptr);
        }
        for (int round = 0; round < L; ++round) {
            bool any = false;
            for (int t = 1; t < live; ++t) {
                want[t] = reached[t - 1];
                any = any || !vf_jpeg_sub_same(want[t], start[t]);
            }
            if (!any) break;
            counts.rounds += 1;
            for (int t = 1; t < live; ++t) {
                if (vf_jpeg_sub_same(want[t], start[t])) continue;
                start[t] = reached[t] = want[t];
                vf_jpeg_decode_subseq(bytes, begin, end, begin + (c0 + t) * S + S, max_steps, tables, reached[t], begun[t], 0, 0, nullptr);
            }
        }
        if (live == L) carry = reached[L - 1];
        for (int t = 0; t < live; ++t) {
            int again;
            VfJpegSubState from = start[t];
            if (vf_jpeg_decode_subseq(bytes, begin, end, begin + (c0 + t) * S + S, max_steps, tables, from, again, blocks_before, blocks, out) !=
                VF_JPEG_OK)
                fault = true;
            blocks_before += begun[t];
        }
    }
    if (blocks_before < blocks) fault = true;
    long long pred[3] = {0, 0, 0};
    for (int blk = 0; blk < blocks; ++blk) {
        const int slot = blk % 6, comp = slot < 4 ? 0 : slot - 3;
        pred[comp] += out[(long)blk * 64];
        if (pred[comp] < -32768 || pred[comp] > 32767) {
            fault = true;
            break;
        }
        out[(long)blk * 64] = (int16_t)pred[comp];
    }
    if (!fault) return VF_JPEG_OK;
    if (blocks) memset(out, 0, (size_t)blocks * 64 * sizeof(int16_t));
    return vf_jpeg_decode_interval(bytes, begin, end, tables, blocks, out);
}

// decodes bytes[begin, end) of a heap copy of exactly `n` bytes into a heap buffer of exactly blocks x 64 coefficients
int decode(bool parallel, const uint8_t* src, size_t n, long begin, long end, const VfJpegTables& tables, uint32_t blocks,
           std::vector<int16_t>& got, Counts& counts) {
    uint8_t* bytes = (uint8_t*)malloc(n ? n : 1);
    if (n) memcpy(bytes, src, n);
    VfJpegTables* t = (VfJpegTables*)malloc(sizeof(VfJpegTables));
    memcpy(t, &tables, sizeof(VfJpegTables));
    int16_t* out = (int16_t*)calloc((size_t)blocks * 64 ? (size_t)blocks * 64 : 1, sizeof(int16_t));
    const int status = parallel ? decode_parallel(n ? bytes : nullptr, begin, end, t, (int)blocks, out, counts)
                                : vf_jpeg_decode_interval(n ? bytes : nullptr, begin, end, t, (int)blocks, out);
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
    if (argc != 6) {
        fprintf(stderr, "usage: %s CASES MUTATIONS SEED SUBSEQ_BYTES LANES\n", argv[0]);
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
    subseq_bytes = atoi(argv[4]);
    lanes = atoi(argv[5]);
    if (subseq_bytes < kVfJpegSubseqMin || subseq_bytes > kVfJpegSubseqMax || subseq_bytes % 4 != 0 || lanes < 2 || lanes > 1024) {
        fprintf(stderr, "SUBSEQ_BYTES is a multiple of 4 in 4..1024, LANES 2..1024\n");
        return 2;
    }
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
    printf("cases %zu mutations %ld\n", cases.size(), mutations);
    int failures = 0;
    std::vector<int16_t> got, serial;
    Counts counts = {0, 0, 0}, unused = {0, 0, 0};
    for (size_t i = 0; i < cases.size(); ++i) {
        const Case& c = cases[i];
        for (int form = 0; form < 2; ++form) {
            const uint8_t* src = form == 0 ? c.scan.data() : c.scan.data() + c.begin;
            const size_t n = form == 0 ? c.scan.size() : c.end - c.begin;
            const long begin = form == 0 ? c.begin : 0, end = form == 0 ? c.end : c.end - c.begin;
            const int status = decode(true, src, n, begin, end, c.tables, c.blocks, got, counts);
            const int status_serial = decode(false, src, n, begin, end, c.tables, c.blocks, serial, unused);
            if (status != (int)c.status || got != c.want || status != status_serial || got != serial) {
                size_t at = 0;
                while (at < got.size() && got[at] == serial[at]) ++at;
                fprintf(stderr, "case %zu form %d: status %d, the serial routine says %d, the model %u; first difference at coefficient %zu of %zu\n",
                        i, form, status, status_serial, c.status, at, got.size());
                ++failures;
            }
        }
        printf("record %zu subsequences %ld chunks %ld rounds %ld\n", i, counts.subsequences, counts.chunks, counts.rounds);
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
        const int status = decode(true, b.data(), b.size(), 0, (long)b.size(), tables, c.blocks, got, unused);
        const int status_serial = decode(false, b.data(), b.size(), 0, (long)b.size(), tables, c.blocks, serial, unused);
        if (status != status_serial || got != serial || status < 0 || status > 8) {
            fprintf(stderr, "mutation %ld: status %d, the serial routine says %d, coefficients %s\n", done, status, status_serial,
                    got == serial ? "equal" : "differ");
            ++failures;
        } else {
            ++histogram[status];
        }
    }
    for (int s = 0; s <= 8; ++s) printf("status %d: %ld\n", s, histogram[s]);
    return failures ? 1 : 0;
}
