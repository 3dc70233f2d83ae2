"""The GEMM-family launch rules (vface_amd/csrc/dispatch.cpp) without a GPU: the file and a small driver (tests/dispatch_probe.cpp)
build as plain C++17 -- no ``-x hip``, no HIP include path -- and the plans they give are pinned.

tests/golden/dispatch_unet_plans.txt holds the distinct GEMM-family launches of one 512 x 512 DDIM step of the full hooked UNet at 24,
48 and 96 samples (recorded at the four C entry points on an MI355X: ``bench.py --eager --streams 1 --frames 8 | 16 | 32``), each
as the GemmParams capi.cpp builds for it, with the plan the rules gave BEFORE they moved into dispatch.cpp (a stand-alone harness
around verbatim copies of the old rule functions wrote the rows; dispatch.cpp never did).  A row changes only when a rule changes:
the nominal batches (24 and 48 samples), the 192-tile thresholds and the persistent grid all show in it.
tests/golden/dispatch_boundary_plans.txt, written the same way, holds fifteen synthetic launches on BOTH sides of the thresholds the UNet
does not sit on: the split cap of 8 in both split rules; 192, 193 and 200 tiles in the split rule; 188, 191 and 192 tiles in the 256-row tile's;
the 24-sample grid in the schedule (1536 tiles of 160), split and patch / im2col rules; the 48-sample grid in the tile-width rule and the 8x8
form's split (12 image quads at 11 channel tiles).  Moving 24, 48, either 192 or the cap 8 by one in either direction changes a row.  The
patch / im2col threshold of 160 tiles is pinned as far as it can act: the grid it is compared with is a multiple of 24, and the rows at 144
and 168 tiles fail for any value outside 145..168."""
import os
import subprocess

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "vface_amd", "csrc")
TABLE = os.path.join(ROOT, "tests", "golden", "dispatch_unet_plans.txt")
BOUNDARY = os.path.join(ROOT, "tests", "golden", "dispatch_boundary_plans.txt")
CXX = "/opt/rocm/lib/llvm/bin/clang++"
BATCHES = range(1, 97)


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    if not os.path.exists(CXX):
        pytest.skip("no ROCm clang++ here")
    exe = str(tmp_path_factory.mktemp("dispatch") / "dispatch_probe")
    subprocess.run([CXX, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC, os.path.join(ROOT, "tests", "dispatch_probe.cpp"),
                    os.path.join(CSRC, "dispatch.cpp"), "-o", exe], check=True)

    def run(launches):
        text = "".join(" ".join(f"{k}={v}" for k, v in launch.items()) + "\n" for launch in launches)
        out = subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout.splitlines()
        assert len(out) == len(launches)
        return [dict(kv.split("=") for kv in line.split()) for line in out]
    return run


def _table(path=TABLE):
    rows = []
    for line in open(path):
        fields, plan = line.strip().split(" => ")
        rows.append(({k: int(v) for k, v in (kv.split("=") for kv in fields.split())}, dict(kv.split("=") for kv in plan.split())))
    return rows


def test_plans_of_the_unet_are_the_pinned_ones(probe):
    rows = _table()
    assert len(rows) >= 250 and {24, 48, 96} <= {f["M"] // f["rows_per_sample"] for f, _ in rows if f.get("rows_per_sample", 0) > 1}
    assert {"gemm", "gemm_big", "conv_patch", "conv_q8", "conv_in16"} <= {p.get("kernel") for _, p in rows}
    assert any(int(p.get("split_k", 1)) > 1 for _, p in rows) and any(p.get("persistent") == "1" for _, p in rows)
    rows += _table(BOUNDARY)
    assert {p["split_k"] for _, p in rows} >= {"1", "2", "8"}
    got = probe([f for f, _ in rows])
    for (fields, want), plan in zip(rows, got):
        assert plan == want, fields


def _per_sample(rows):
    """The table's distinct per-sample geometries: convolutions, and GEMMs whose caller states rows_per_sample > 1."""
    seen, out = set(), []
    for f, _ in rows:
        if f.get("rows_per_sample", 0) <= 1 or f["M"] % f["rows_per_sample"]:
            continue
        g = dict(f, M=0, workspace=4096, workspace_bytes=1 << 40)      # (the workspace never the reason a split is not taken)
        key = tuple(sorted(g.items()))
        if key not in seen:
            seen.add(key)
            out.append(g)
    return out


def test_bit_affecting_choices_do_not_follow_the_batch(probe):
    """A sample's bits must not depend on which other samples share its launch: at every table geometry, for every batch from 1 to
    96, the K split is the same, and where column statistics are requested so are the kernel (the 256-row tile counts as the
    128-row kernel: bit-identical) and the tile width, which fix the order the statistics are folded in."""
    geoms = _per_sample(_table())
    assert len(geoms) >= 60
    plans = probe([dict(g, M=b * g["rows_per_sample"]) for g in geoms for b in BATCHES])
    n = len(BATCHES)
    for i, g in enumerate(geoms):
        def bits(p):
            kernel = "gemm" if p["kernel"] == "gemm_big" else p["kernel"]
            return (p["split_k"], p["kt_per_split"], p["reduce"]) + ((kernel, p["bn"]) if g.get("colstats") else ())
        kinds = {bits(p) for p in plans[i * n:(i + 1) * n]}
        assert len(kinds) == 1, (g, kinds)      # (no exception is needed under the rules as they stand)


def test_every_planned_split_fits_the_workspace_the_wrappers_ask_for(probe):
    rows = _table()
    launches = [f for f, _ in rows] + [dict(g, M=b * g["rows_per_sample"]) for g in _per_sample(rows) for b in (1, 2, 3, 7, 24, 48, 96)]
    splits = 0
    for f, p in zip(launches, probe(launches)):
        if p.get("reduce") == "1":
            splits += 1
            assert int(p["split_k"]) * f["M"] * f["N"] * 4 <= int(p["workspace_needed"]), (f, p)
    assert splits >= 20


GEMM_OUT_F32, GEMM_STAMPS, GEMM_NARROW_EPILOGUE, GEMM_NO_PATCH, GEMM_PATCH = 2, 0x4000, 0x8000, 0x80000, 0x100000      # (dispatch.hpp; pinned against the header in test_host_cpu.py)
VFACE_ERR_SHAPE = -3


def test_stamped_launches_plan_onto_the_built_stamped_forms_or_are_refused(probe):
    """GEMM_STAMPS has three instantiations behind it: gemm.hip's plain two-stage kernel at both tile widths (form 3), and the patch-staged 3x3
    convolution 160 channels wide (form 3 there too).  Every other stamped launch is refused with VFACE_ERR_SHAPE, never run without stamps."""
    ptrs = dict(A=0x10000, Wt=0x20000, C=0x30000, zeros=0x40000, bias=0x50000, colstats=0x60000)
    plain = dict(ptrs, lda=192, ldw=192, Kw=192, M=200, N=320, K=192, rows_per_sample=1, ldc=320, ld_colstats=320)
    conv = dict(ptrs, mode=1, lda=64, ldw=576, Kw=576, M=256, N=160, K=576, H=16, W=16, OH=16, OW=16, Cin=64, stride=1, pad=1,
                rows_per_sample=256, ldc=160, ld_colstats=160)
    launches = [dict(plain, flags=GEMM_STAMPS | (5 << 8)), dict(plain, flags=GEMM_STAMPS | (6 << 8)),
                dict(plain, flags=GEMM_STAMPS | (5 << 8) | GEMM_OUT_F32), dict(plain, flags=GEMM_STAMPS | (5 << 8) | GEMM_NARROW_EPILOGUE),
                dict(plain, flags=GEMM_STAMPS | (7 << 8)), dict(conv, flags=GEMM_STAMPS | GEMM_NO_PATCH),
                dict(conv, flags=GEMM_STAMPS | GEMM_PATCH)]
    w128, w160, f32, narrow, one_stage, im2col, patch = probe(launches)
    for plan, bn in ((w128, 128), (w160, 160)):
        assert (plan["rc"], plan["kernel"], plan["stages"], plan["mode"], plan["form"]) == ("0", "gemm", "2", "0", "3"), plan
        assert (int(plan["bn"]), plan["persistent"], plan["split_k"], plan["reduce"]) == (bn, "0", "1", "0"), plan
        assert plan["grid"] == f"{2 * ((320 + bn - 1) // bn)},1", plan
    for refused in (f32, narrow, one_stage, im2col):
        assert int(refused["rc"]) == VFACE_ERR_SHAPE and "kernel" not in refused, refused
    assert (patch["rc"], patch["kernel"], patch["bn"], patch["mode"], patch["form"], patch["grid"]) == ("0", "conv_patch", "160", "3", "3", "1,1"), patch
    # the same launches without the flag plan as before: form 0, and the refused forms run
    for launch, plan in zip(launches, probe([dict(l, flags=l["flags"] & ~GEMM_STAMPS, colstats=0) for l in launches])):
        assert plan["rc"] == "0" and plan["form"] == "0", (launch, plan)
