// Driver of tests/test_dispatch_cpu.py: plain C++, linked with vface_amd/csrc/dispatch.cpp only.
// stdin: one launch per line, `field=value` tokens naming GemmParams members (pointers as integers, 0 = null) and `persistent_grid`.
// stdout: the launch plan of that line, and the split-K workspace the Python wrappers would have asked for.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "dispatch.hpp"

#define INT_FIELDS(X) X(mode) X(lda) X(lda2) X(K1) X(a2_row_mod) X(ldw) X(Kw) X(M) X(N) X(K) X(H) X(W) X(Cin) X(OH) X(OW) X(stride) \
    X(upsample) X(pad) X(pad_x) X(KH) X(KW) X(ntaps) X(out_phase) X(rows_per_sample) X(ld_rowbias) X(ldr) X(ldc) X(res_f32) X(ldc32) \
    X(ld_gn_ab) X(gn_silu) X(flags) X(ld_colstats) X(workspace_bytes)
#define PTR_FIELDS(X) X(A) X(A2) X(Wt) X(bias) X(rowbias) X(residual) X(C) X(C32) X(gn_ab) X(zeros) X(colstats) X(workspace)

static const char* KERNEL[6] = {"gemm", "conv_patch", "conv_q8", "gemm_patch", "gemm_big", "conv_in16"};

int main() {
    static char line[8192];
    while (fgets(line, sizeof line, stdin)) {
        GemmParams p{};
        int persistent_grid = 512;
        for (char* tok = strtok(line, " \n"); tok; tok = strtok(nullptr, " \n")) {
            char* eq = strchr(tok, '=');
            if (!eq) { fprintf(stderr, "bad token %s\n", tok); return 2; }
            *eq = 0;
            const long long v = strtoll(eq + 1, nullptr, 0);
            bool known = !strcmp(tok, "persistent_grid");
            if (known) persistent_grid = (int)v;
#define X(f) if (!strcmp(tok, #f)) { p.f = (decltype(p.f))v; known = true; }
            INT_FIELDS(X)
#undef X
#define X(f) if (!strcmp(tok, #f)) { p.f = reinterpret_cast<decltype(p.f)>((uintptr_t)v); known = true; }
            PTR_FIELDS(X)
#undef X
            if (!known) { fprintf(stderr, "unknown field %s\n", tok); return 2; }
        }
        VfGemmPlan pl;
        const int rc = vf_plan_gemm(p, persistent_grid, &pl);
        const long ws = (p.M > 0 && p.N > 0 && p.K > 0) ? vf_splitk_workspace_bytes(p.M, p.N, p.K, p.flags, p.rows_per_sample) : 0;
        if (rc) { printf("rc=%d workspace_needed=%ld\n", rc, ws); continue; }
        printf("rc=0 kernel=%s bn=%d stages=%d mode=%d form=%d persistent=%d split_k=%d kt_per_split=%d tile_group=%d grid=%d,%d lds=%d "
               "slices_per_wg=%d reduce=%d workspace_needed=%ld\n",
               KERNEL[pl.kernel], pl.bn, pl.stages, pl.mode, pl.form, (int)pl.persistent, pl.p.split_k, pl.p.kt_per_split, pl.p.tile_group,
               pl.grid_x, pl.grid_y, pl.lds_bytes, pl.slices_per_wg, (int)pl.reduce, ws);
    }
    return 0;
}
