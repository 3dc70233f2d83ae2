"""``vface_gemm`` and the convolutions per element against fp64 on the MI355X: every output element within
``kernel_bounds.gemm_ref_and_bound`` / ``conv_ref_and_bound`` -- bounds built from fp64 quantities of the reference alone, shown by
test_gemm_bound_cpu.py to admit a model of the kernels' rounding points and to refuse one-line defects of it -- on the tails of the
128 x (128 | 160) x 64 tile, through every epilogue (wide, narrow, split-K reduce, GEGLU, the fp32 residual stream), on the 256-row
forms, and for the convolutions on the im2col kernel, the patch-staged kernel, its 8 x 8 form, the fused 1x1 shortcut and the
parity phases of the upsampling convolution; with the column statistics against the fp64 sums of what was stored.

Buffers: every output (16-bit, fp32, fp32 carrier, column statistics) is a view inside a ``sentinel`` buffer -- one row above, two
below, 8 columns left and 16 right of it, so ``ldc = N + 24`` -- and after the call everything outside the view has its sentinel
bits.  The A operand sits 8 columns into a buffer 16 columns wider, a 16-bit / fp32 residual 8 / 4 columns into one twice that
wider (``ldr != N``).  Shapes are the smallest that reach the edge in question; the production shapes stay with the rel-L2 tests
of test_kernels_gpu.py, which the bit-identity tests there tie to the two kernels pinned here.

Forms that have a query are asserted through it: ``vface_splitk_workspace_bytes`` (the shape really splits),
``vface_conv_uses_patch_kernel`` (which convolution kernel runs), the error code of a refused combination.  The 256 x 320 tile
and the 256-row patch form of a plain GEMM have no query: their cases meet the conditions the header states for the flag."""
import math

import pytest
import torch

from kernel_bounds import (Framed, assert_within, colstats_ref_and_bound, conv_ref_and_bound, gemm_ref_and_bound, note, rnd, same_bits, strided)

pytestmark = pytest.mark.gpu

DEV = "cuda"
DTS = [torch.float16, torch.bfloat16]
ERR_ARG, ERR_ALIGN, ERR_SHAPE = -1, -2, -3          # include/vface_hip.h


def hip():
    from vface_amd import hip as h
    h.load()
    return h


def plain_slices(M):
    return [torch.arange(s, min(s + 64, M)) for s in range(0, M, 64)]


def check_stats(cs, stored, slices, what, family):
    ref, bound = colstats_ref_and_bound(stored, slices)
    got = cs.result(what + " colstats", rows=torch.arange(len(slices)))[:len(slices)]
    note(family, assert_within(got, ref, bound, what + " colstats"), bound)


# ================================================================================================ 2.1 GEMM
def run_gemm(h, dt, M, N, K, *, what, family, variant=0, flags=0, bias=False, rps=0, res=None, out="16", k1=0, row_mod=0, geglu=False,
             stats=False, split_k=False, splits=1, seed=0):
    """One launch and its checks.  ``res``: None | "16" | "32"; ``out``: "16" | "f32" (VFACE_EPI_OUT_F32) | "32" (carrier only, NULL
    16-bit output) | "both"; ``k1`` / ``row_mod``: dual source; ``rps``: rows per sample of a row bias (0: none)."""
    a, w = rnd((M, K), 11 + seed, dt), rnd((N, K), 12 + seed, dt, 1 / math.sqrt(K))
    args = dict(out_f32=out != "16", splits=splits, geglu=geglu)
    kw = dict(flags=flags | (variant << 8) | (h.EPI_GEGLU if geglu else 0) | (h.EPI_OUT_F32 if out == "f32" else 0), split_k=split_k)
    nout = N // 2 if geglu else N
    wd = w
    if bias:
        args["bias"] = rnd((N,), 13 + seed, torch.float32)
        if geglu:
            args["bias"][N // 2:] = torch.linspace(-8.0, 8.0, N // 2)      # gates over [-8, 8]: both branches and the deep negative tail
        kw["bias"] = args["bias"].to(DEV)
    if geglu:
        from vface_amd.packing import pack_geglu
        wd, bp = pack_geglu(w, args["bias"])
        kw["bias"] = bp.to(DEV)
    if rps:
        args["rows_per_sample"] = rps
        args["rowbias"] = rnd((-(-M // rps), N), 14 + seed, torch.float32)
        kw.update(rowbias=strided(args["rowbias"], 4), rows_per_sample=rps)
    if res == "16":
        args["residual"] = rnd((M, N), 15 + seed, dt)
        off = 8 if N % 8 == 0 else 4
        kw.update(residual=strided(args["residual"], off), ldr=N + 2 * off)
    elif res == "32":
        args["residual"] = rnd((M, N), 15 + seed, torch.float32)
        kw["residual32"] = strided(args["residual"], 4)
    if k1:
        a2 = rnd((row_mod, K - k1), 16 + seed, dt)
        full = torch.cat([a[:, :k1], a2[torch.arange(M) % row_mod]], 1)
        kw.update(a2=strided(a2, 8), lda2=K - k1 + 16, k1=k1, a2_row_mod=row_mod)
        ad = strided(a[:, :k1].contiguous(), 8)
        lda = k1 + 16
    else:
        full, ad, lda = a, strided(a, 8), K + 16
    o16 = Framed(M, nout, dt) if out in ("16", "both") else None
    o32 = Framed(M, nout, torch.float32) if out != "16" else None
    cs = Framed(-(-M // 64) + 1, N, torch.float32, pair=True) if stats else None
    if stats:
        kw["colstats"] = cs.stats_arg
    if out == "f32":
        target, ldc = o32.view, o32.ld
    else:
        target, ldc = (o16.view, o16.ld) if o16 is not None else (None, 0)
        if o32 is not None:
            kw["out32"] = o32.view
    h.gemm(ad, wd.to(DEV), target, M=M, N=N, K=K, lda=lda, ldc=ldc, **kw)
    ref, bound = gemm_ref_and_bound(full, w, dt, **args)
    g32 = o32.result(what + " fp32") if o32 is not None else None
    g16 = o16.result(what) if o16 is not None else None
    main = g32 if g32 is not None else g16
    note(family, assert_within(main, ref, bound, what), bound)
    if g32 is not None and g16 is not None:
        assert same_bits(g16, g32.to(dt)), f"{what}: the 16-bit output is not out32 rounded once"
    if stats:
        check_stats(cs, main, plain_slices(M), what, family + " colstats")


TAIL_M, TAIL_N, TAIL_K = (1, 127, 129, 200), (8, 72, 136, 168, 320), (8, 56, 64, 72, 136)
TAIL_FORMS = [(torch.float16, v) for v in (0, 5, 6, 7, 8)] + [(torch.bfloat16, 0), (torch.bfloat16, 6)]


@pytest.mark.parametrize("M", TAIL_M)
@pytest.mark.parametrize("dt,variant", TAIL_FORMS)
def test_gemm_tile_tails(dt, variant, M):
    """The whole M x N x K grid of tile tails; bias, row bias (two samples) and a strided 16-bit residual each on about half of it."""
    h = hip()
    for i, N in enumerate(TAIL_N):
        for j, K in enumerate(TAIL_K):
            bits = i + 5 * j + 3 * TAIL_M.index(M)
            run_gemm(h, dt, M, N, K, what=f"tails {dt} v{variant} {M}x{N}x{K}", family="gemm tails", variant=variant, bias=bool(bits & 1),
                     rps=(M + 1) // 2 if bits & 2 else 0, res="16" if bits & 4 else None, seed=bits)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("N,variant,out", [(4, 0, "16"), (12, 0, "16"), (132, 0, "16"), (132, 6, "16"), (12, 7, "16"), (72, 0, "f32"), (12, 5, "f32"),
                                           (168, 8, "f32"), (136, 7, "16"), (168, 8, "16")])
def test_gemm_narrow_epilogue(dt, N, variant, out):
    """Every way into the 4-channels-per-lane epilogue: N % 8 != 0, the fp32 output, the single-stage schedules."""
    h = hip()
    run_gemm(h, dt, 200, N, 72, what=f"narrow {dt} N={N} v{variant} {out}", family="gemm narrow", variant=variant, out=out, bias=True, rps=100,
             res="16")


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("variant", [0, 7])
@pytest.mark.parametrize("rps", [24, 100, 128, 192])
def test_gemm_rowbias_across_a_tile(dt, variant, rps):
    """128-row tiles inside one sample (preloaded row bias), straddling two and several (read per row)."""
    h = hip()
    run_gemm(h, dt, 4 * rps, 136, 72, what=f"rowbias {dt} v{variant} rps={rps}", family="gemm rowbias", variant=variant, bias=True, rps=rps)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("variant", [0, 7])
@pytest.mark.parametrize("k1,k2", [(64, 8), (64, 72), (128, 8), (128, 72)])
def test_gemm_dual_source(dt, variant, k1, k2):
    h = hip()
    run_gemm(h, dt, 200, 72, k1 + k2, what=f"dual {dt} v{variant} k1={k1} k2={k2}", family="gemm dual source", variant=variant, bias=True,
             k1=k1, row_mod=56)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("M,N,K", [(130, 72, 64), (200, 320, 136)])
@pytest.mark.parametrize("res,out", [("32", "16"), (None, "32"), ("32", "both"), ("16", "both"), ("32", "32")])
def test_gemm_fp32_residual_stream(dt, M, N, K, res, out):
    h = hip()
    run_gemm(h, dt, M, N, K, what=f"stream32 {dt} {M}x{N}x{K} res={res} out={out}", family="gemm fp32 stream", bias=True, rps=(M + 1) // 2,
             res=res, out=out)


def test_gemm_refuses_the_fp32_stream_where_it_has_no_epilogue():
    """N % 8 != 0, the fp32-only output and the single-stage schedules have no fp32 carrier: VFACE_ERR_SHAPE, nothing written."""
    h = hip()
    dt = torch.float16
    for N, variant, flags in ((12, 0, 0), (72, 7, 0), (72, 0, h.EPI_OUT_F32)):
        a, w = rnd((64, 64), 1, dt).to(DEV), rnd((N, 64), 2, dt).to(DEV)
        o32 = Framed(64, N, torch.float32)
        with pytest.raises(h.VFaceHipError, match=rf"\(code {ERR_SHAPE}\)"):
            h.gemm(a, w, None if not flags else o32.view, M=64, N=N, K=64, lda=64, ldc=o32.ld if flags else 0, out32=o32.view,
                   flags=flags | (variant << 8))
        o32.result("refused", rows=torch.arange(0))


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("variant", [0, 5, 7])
@pytest.mark.parametrize("nout", [32, 64, 512])
def test_gemm_geglu(dt, variant, nout):
    h = hip()
    run_gemm(h, dt, 130, 2 * nout, 72, what=f"geglu {dt} v{variant} nout={nout}", family="gemm geglu", variant=variant, bias=True, geglu=True)


SPLITS = {1024: 2, 1096: 2, 1544: 3}      # two shares; two with a K tail in the last; three uneven ones (9, 9, 7 K tiles)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("K", list(SPLITS))
@pytest.mark.parametrize("M", [64, 200])
@pytest.mark.parametrize("extras", [False, True])
def test_gemm_split_k(dt, K, M, extras):
    h = hip()
    N, rps = 320, (M // 4 if extras else 1)
    assert h.load().vface_splitk_workspace_bytes(M, N, K, 0, rps) == SPLITS[K] * M * N * 4, "the shape no longer splits as this case assumes"
    run_gemm(h, dt, M, N, K, what=f"splitk {dt} {M}x{N}x{K} extras={extras}", family="gemm split-K", bias=True, rps=rps if extras else 0,
             res="16" if extras else None, split_k=True, splits=SPLITS[K])


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("M", [64, 200, 257])
@pytest.mark.parametrize("N", [128, 320])
@pytest.mark.parametrize("form", ["wide", "narrow", "wide32", "splitk", "splitk32"])
def test_gemm_colstats(dt, M, N, form):
    """(sum, sum of squares) per 64-row slice and column against the fp64 sums of the stored values: rows at and beyond M do not
    contribute (the last slice of M = 200 has 8 rows, of M = 257 one), the slice after the last and the columns beyond N keep
    their sentinel."""
    h = hip()
    split = form.startswith("splitk")
    K = 1024 if split else 72
    if split:
        assert h.load().vface_splitk_workspace_bytes(M, N, K, 0, 1) == 2 * M * N * 4
    run_gemm(h, dt, M, N, K, what=f"colstats {dt} {M}x{N} {form}", family="gemm" + (" split-K" if split else ""), variant=7 if form == "narrow" else 0,
             bias=True, res="32" if form.endswith("32") else "16", out="both" if form.endswith("32") else "16", stats=True, split_k=split,
             splits=2 if split else 1)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("name", ["big", "big_res16", "big_geglu", "big_stream32", "big_w256", "patch256_160", "patch256_128"])
def test_gemm_big_tile_and_256_row_forms(dt, name):
    """One direct case each of the forms the bit-identity tests of test_kernels_gpu.py compare with the 128-row kernel.  K = 128 is
    the least both forms take; VFACE_TUNE_BIG_W256 needs N % 256 == 0 beside N % 320 == 0, so its case is N = 1280."""
    h = hip()
    big, fam = h.TUNE_BIG_TILE, "gemm 256-row forms"
    if name == "big":
        run_gemm(h, dt, 300, 320, 128, what=f"{name} {dt}", family=fam, flags=big, bias=True)
    elif name == "big_res16":
        run_gemm(h, dt, 300, 320, 128, what=f"{name} {dt}", family=fam, flags=big, bias=True, res="16")
    elif name == "big_geglu":
        run_gemm(h, dt, 300, 640, 128, what=f"{name} {dt}", family=fam, flags=big, bias=True, geglu=True)
    elif name == "big_stream32":
        run_gemm(h, dt, 512, 320, 128, what=f"{name} {dt}", family=fam, flags=big, bias=True, rps=256, res="32", out="both", stats=True)
    elif name == "big_w256":
        run_gemm(h, dt, 300, 1280, 128, what=f"{name} {dt}", family=fam, flags=big | h.TUNE_BIG_W256, bias=True)
    else:
        run_gemm(h, dt, 512, 320 if name.endswith("160") else 256, 128, what=f"{name} {dt}", family=fam, flags=h.TUNE_PATCH, bias=True, rps=256,
                 res="16")


# ================================================================================================ 2.2 convolutions
def conv_inputs(dt, nimg, cin, cout, H, W, window=3, seed=0):
    x = (rnd((nimg, cin, H, W), 21 + seed, dt).float() + 1.0).to(dt)     # + 1: a tap that should read the zero page counts
    w = rnd((cout, cin, window, window), 22 + seed, dt, 1 / math.sqrt(window * window * cin))
    return x, w


def nhwc(x):
    """``[nimg, C, H, W]`` -> the device view ``[nimg * H * W, C]`` with ``ldx = C + 16``"""
    nimg, c, H, W = x.shape
    return strided(x.permute(0, 2, 3, 1).reshape(nimg * H * W, c).contiguous(), 8)


def patch_slices(nimg, H, W, phase=None):
    """Row sets of the patch-staged kernel's statistics slices (csrc/conv.hip): a wave's 4 image rows x 16 columns of a 16 x 16
    tile, slice = image * (H W / 64) + tile * 4 + wave row; a phase launch files its slices at [(image * 4 + phase) * (H W / 64) ..)
    and its pixels (y, x) are pixels (2 y + py, 2 x + px) of the 2H x 2W output."""
    out = []
    for img in range(nimg):
        for ph in ([None] if phase is None else range(4)):
            for ty in range(H // 16):
                for tx in range(W // 16):
                    for wm in range(4):
                        y = (ty * 16 + wm * 4 + torch.arange(4))[:, None]
                        x = (tx * 16 + torch.arange(16))[None, :]
                        if ph is None:
                            out.append(((img * H + y) * W + x).reshape(-1))
                        else:
                            out.append(((img * 2 * H + 2 * y + ph // 2) * 2 * W + 2 * x + ph % 2).reshape(-1))
    return out


def im2col_phase_slices(nimg, H, W):
    """gemm.hip: 64 consecutive pixels of the phase grid per slice, filed by (image, phase)."""
    out = []
    for img in range(nimg):
        for ph in range(4):
            for j in range(H * W // 64):
                q = 64 * j + torch.arange(64)
                out.append((img * 2 * H + 2 * (q // W) + ph // 2) * 2 * W + 2 * (q % W) + ph % 2)
    return out


def run_conv(h, dt, *, what, family, nimg, cin, cout, H, W, flags, kernel, stride=1, upsample=False, trailing=False, bias=True, rowbias=True,
             res=None, out="16", gn=None, c2=0, stats=False, split_k=False, splits=1, seed=0):
    """One ``vface_conv3x3`` / ``vface_conv3x3_plus_1x1`` launch and its checks; ``kernel``: what vface_conv_uses_patch_kernel must say."""
    from vface_amd.packing import pack_conv3x3
    assert h.conv_uses_patch_kernel(H, W, cin, cout, 3, stride, upsample, flags) == kernel, what
    x, w = conv_inputs(dt, nimg, cin, cout, H, W, seed=seed)
    pad = (0, 1, 0, 1) if trailing else (1, 1, 1, 1)
    VH, VW = (2 * H, 2 * W) if upsample else (H, W)
    OH, OW = (VH + pad[0] + pad[1] - 3) // stride + 1, (VW + pad[2] + pad[3] - 3) // stride + 1
    M = nimg * OH * OW
    args = dict(stride=stride, upsample=upsample, pad=pad, out_f32=out != "16", splits=splits)
    kw = dict(flags=flags | (h.CONV_PAD_TRAILING if trailing else 0), split_k=split_k)
    if bias:
        args["bias"] = rnd((cout,), 23 + seed, torch.float32)
        kw["bias"] = args["bias"].to(DEV)
    if rowbias:
        args["rowbias"] = rnd((nimg, cout), 24 + seed, torch.float32)
        kw["rowbias"] = strided(args["rowbias"], 4)
    if res == "16":
        args["residual"] = rnd((M, cout), 25 + seed, dt)
        kw.update(residual=strided(args["residual"], 8), ldr=cout + 16)
    elif res == "32":
        args["residual"] = rnd((M, cout), 25 + seed, torch.float32)
        kw["residual32"] = strided(args["residual"], 4)
    if gn is not None:
        args["scale_shift"] = torch.stack([1 + 0.3 * rnd((nimg, cin), 26, torch.float32), 0.5 + 0.3 * rnd((nimg, cin), 27, torch.float32)], -1).contiguous()
        args["silu"] = gn
        kw.update(gn_ab=args["scale_shift"].to(DEV), gn_silu=gn)
    o16 = Framed(M, cout, dt) if out in ("16", "both") else None
    o32 = Framed(M, cout, torch.float32) if out != "16" else None
    if o32 is not None:
        kw["out32"] = o32.view
    cs = Framed(M // 64 + 1, cout, torch.float32, pair=True) if stats else None
    if stats:
        kw["colstats"] = cs.stats_arg
    xd = nhwc(x)
    target, ldy = (o16.view, o16.ld) if o16 is not None else (None, 0)
    if c2:
        args["x2"], args["w2"] = rnd((M, c2), 28, dt), rnd((cout, c2), 29, dt, 1 / math.sqrt(c2))
        wt = torch.cat([pack_conv3x3(w), args["w2"]], 1).contiguous().to(DEV)
        h.conv3x3_plus_1x1(xd, strided(args["x2"], 8), wt, target, nimg=nimg, H=H, W=W, cin=cin, c2=c2, cout=cout, ldx=cin + 16, ldx2=c2 + 16,
                           ldy=ldy, **kw)
    else:
        h.conv3x3(xd, pack_conv3x3(w).to(DEV), target, nimg=nimg, H=H, W=W, cin=cin, cout=cout, ldx=cin + 16, ldy=ldy, stride=stride,
                  upsample=upsample, **kw)
    ref, bound = conv_ref_and_bound(x, w, dt, **args)
    assert ref.shape == (M, cout)
    g32 = o32.result(what + " fp32") if o32 is not None else None
    g16 = o16.result(what) if o16 is not None else None
    main = g32 if g32 is not None else g16
    note(family, assert_within(main, ref, bound, what), bound)
    if g32 is not None and g16 is not None:
        assert same_bits(g16, g32.to(dt)), f"{what}: the 16-bit output is not out32 rounded once"
    if stats:
        check_stats(cs, main, patch_slices(nimg, H, W) if kernel == 1 else plain_slices(M), what, family + " colstats")


IM2COL_MODES = {"s1": dict(), "s2": dict(stride=2), "up": dict(upsample=True), "s2_trailing": dict(stride=2, trailing=True)}


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("mode", list(IM2COL_MODES))
@pytest.mark.parametrize("cin", [8, 24, 64, 128])
def test_conv_im2col_kernel(dt, mode, cin):
    """gemm.hip's implicit GEMM (VFACE_TUNE_NO_PATCH): the generic window path (Cin 8, 24) and the wave-uniform tap path (64, 128),
    three images, every border tap weighted by the constant in x; stride 2 and the trailing padding on odd and even sizes."""
    h = hip()
    for i, cout in enumerate((8, 72, 160)):
        for j, (H, W) in enumerate(((1, 1), (3, 5), (7, 6), (16, 16))):
            bits = i + 3 * j
            if mode == "s2_trailing" and H == 1:
                continue                  # a 1 x 1 image padded (0, 1, 0, 1) holds no 3 x 3 window: there is no such convolution
            run_conv(h, dt, what=f"im2col {dt} {mode} cin={cin} cout={cout} {H}x{W}", family="conv im2col", nimg=3, cin=cin, cout=cout, H=H, W=W,
                     flags=h.TUNE_NO_PATCH, kernel=0, bias=bool(bits & 1), rowbias=bool(bits & 2), res="16" if bits & 4 else None, seed=bits,
                     **IM2COL_MODES[mode])


@pytest.mark.parametrize("dt", DTS)
def test_conv_im2col_kernel_split_k(dt):
    """K = 1152 on a shallow grid: two shares of nine K tiles, the epilogue and the statistics in the split-K reduce."""
    h = hip()
    assert h.load().vface_splitk_workspace_bytes(3 * 256, 160, 1152, h.TUNE_NO_PATCH, 256) == 2 * 3 * 256 * 160 * 4
    run_conv(h, dt, what=f"im2col split-K {dt}", family="conv im2col split-K", nimg=3, cin=128, cout=160, H=16, W=16, flags=h.TUNE_NO_PATCH, kernel=0,
             res="16", stats=True, split_k=True, splits=2)


PATCH_SHAPES = [(16, 16, 64, 128, 1), (16, 32, 128, 160, 3), (32, 16, 64, 320, 1), (16, 16, 128, 320, 3), (32, 16, 128, 128, 3), (16, 32, 64, 160, 1)]


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("form", ["rowbias", "res16", "res32", "out32", "stats"])
@pytest.mark.parametrize("H,W,cin,cout,nimg", PATCH_SHAPES)
def test_conv_patch_staged_kernel(dt, form, H, W, cin, cout, nimg):
    h = hip()
    kw = {"rowbias": dict(), "res16": dict(res="16"), "res32": dict(res="32", out="both"), "out32": dict(out="32"),
          "stats": dict(res="16", stats=True)}[form]
    run_conv(h, dt, what=f"patch {dt} {form} {H}x{W} cin={cin} cout={cout} nimg={nimg}", family="conv patch-staged", nimg=nimg, cin=cin, cout=cout,
             H=H, W=W, flags=h.TUNE_PATCH, kernel=1, **kw)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("silu", [True, False])
@pytest.mark.parametrize("H,W,cin,cout,nimg", PATCH_SHAPES)
def test_conv_patch_staged_fused_groupnorm_input(dt, silu, H, W, cin, cout, nimg):
    """act(x a + b) with b != 0 in the operand path: a padding tap that were normalised too would read act(b), not 0.  The fused form
    is built 128 channels wide only: other widths are refused with VFACE_ERR_SHAPE, never run without their normalisation."""
    h = hip()
    what = f"patch gn {dt} silu={silu} {H}x{W} cin={cin} cout={cout} nimg={nimg}"
    if cout % 128:
        with pytest.raises(h.VFaceHipError, match=rf"\(code {ERR_SHAPE}\)"):
            run_conv(h, dt, what=what, family="conv fused GroupNorm", nimg=nimg, cin=cin, cout=cout, H=H, W=W, flags=h.TUNE_PATCH, kernel=1, gn=silu)
        return
    run_conv(h, dt, what=what, family="conv fused GroupNorm", nimg=nimg, cin=cin, cout=cout, H=H, W=W, flags=h.TUNE_PATCH, kernel=1, gn=silu)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("nimg", [1, 5, 6])
@pytest.mark.parametrize("cin", [128, 256])
def test_conv_8x8_form(dt, nimg, cin):
    """Four images per workgroup (a tail at 1, 5, 6 images), K split over channel chunks (cin / 128 shares), epilogue and the
    per-image statistics in the split-K reduce; with the workspace the header asks for (what hip.conv3x3 passes)."""
    h = hip()
    assert h.load().vface_splitk_workspace_bytes(nimg * 64, 128, 9 * cin, 0, 64) >= (cin // 128) * nimg * 64 * 128 * 4
    run_conv(h, dt, what=f"8x8 {dt} nimg={nimg} cin={cin}", family="conv 8x8 form", nimg=nimg, cin=cin, cout=128, H=8, W=8, flags=0, kernel=2,
             res="32", out="both", stats=True, split_k=True, splits=cin // 128)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("c2", [64, 128])
@pytest.mark.parametrize("kernel", [0, 1])
def test_conv_plus_1x1_shortcut(dt, c2, kernel):
    h = hip()
    H, W, cout, flags = ((16, 16, 160, h.TUNE_PATCH) if kernel else (7, 6, 72, h.TUNE_NO_PATCH))
    run_conv(h, dt, what=f"plus1x1 {dt} c2={c2} kernel={kernel}", family="conv plus 1x1", nimg=3, cin=64, cout=cout, H=H, W=W, flags=flags,
             kernel=kernel, c2=c2, out="both" if kernel else "16")


def unpack_window(wp, cin, win):
    """``packing.pack_conv_window``'s [Cout, taps * Cin] back to [Cout, Cin, win, win]."""
    cout, taps = wp.shape[0], win * win
    t = wp.reshape(cout, cin // 64, taps, 64).permute(0, 2, 1, 3) if cin % 64 == 0 else wp.reshape(cout, taps, cin)
    return t.reshape(cout, win, win, cin).permute(0, 3, 1, 2).contiguous()


def launch_phase(h, xd, wd, out, bd, rbd, cs, *, nimg, H, W, cin, cout, py, px, flags, dt):
    """ONE ``vface_upsample2x_conv3x3_phase`` call (``hip.upsample2x_conv3x3`` only runs all four)."""
    rc = h.load().vface_upsample2x_conv3x3_phase(h._p(xd), xd.stride(0), nimg, H, W, cin, h._p(wd), 4 * cin, cout, py, px, h._p(bd), h._p(rbd),
                                                 rbd.stride(0), h._p(out.view), out.ld, h._p(h.zeros_page(xd.device)), flags, h.dtype_code(dt),
                                                 h._p(cs.stats_arg) if cs is not None else None, cs.ld if cs is not None else 0, h._stream(), None)
    h._check(rc, "vface_upsample2x_conv3x3_phase")


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("kernel,cin,cout,H,W,stats", [(0, 24, 72, 3, 5, False), (0, 64, 72, 8, 8, True), (0, 128, 160, 16, 8, True), (1, 64, 160, 16, 16, True),
                                                     (1, 128, 128, 16, 32, True)])
def test_conv_upsample_parity_phases(dt, kernel, cin, cout, H, W, stats):
    """The four phases of conv3x3(nearest x2 upsample) into ONE sentinel output: after each single call only that phase's rows
    (2 i + py, 2 j + px) have changed; each phase against its own 2 x 2 kernel (the pre-summed taps as rounded to the 16-bit type);
    the statistics in each kernel's own slice layout."""
    h = hip()
    from vface_amd.packing import pack_upsample_phases
    nimg, flags = 3, (h.TUNE_PATCH if kernel else h.TUNE_NO_PATCH)
    assert h.conv_uses_patch_kernel(H, W, cin, cout, 2, 1, False, flags) == kernel
    x, w = conv_inputs(dt, nimg, cin, cout, H, W)
    wph = pack_upsample_phases(w.float()).to(dt)
    bias, rb = rnd((cout,), 3, torch.float32), rnd((nimg, cout), 4, torch.float32)
    out = Framed(nimg * 4 * H * W, cout, dt)
    cs = Framed(nimg * 4 * H * W // 64 + 1, cout, torch.float32, pair=True) if stats else None
    xd, wd, bd, rbd = nhwc(x), wph.to(DEV), bias.to(DEV), strided(rb, 4)
    rows_all = torch.arange(nimg * 4 * H * W).reshape(nimg, 2 * H, 2 * W)
    full_ref, full_bound = torch.zeros(nimg * 4 * H * W, cout, dtype=torch.float64), torch.zeros(nimg * 4 * H * W, cout, dtype=torch.float64)
    for py in (0, 1):
        for px in (0, 1):
            launch_phase(h, xd, wd[2 * py + px], out, bd, rbd, cs, nimg=nimg, H=H, W=W, cin=cin, cout=cout, py=py, px=px, flags=flags, dt=dt)
            rows = rows_all[:, py::2, px::2].reshape(-1)
            got = out.result(f"phase ({py}, {px})", rows=rows)
            ref, bound = conv_ref_and_bound(x, unpack_window(wph[2 * py + px], cin, 2), dt, pad=(1 - py, py, 1 - px, px), bias=bias, rowbias=rb)
            note("conv parity phases", assert_within(got[rows], ref, bound, f"phase {dt} kernel={kernel} ({py}, {px}) cin={cin} {H}x{W}"), bound)
            full_ref[rows], full_bound[rows] = ref, bound
    final = out.result("all phases", rows=torch.arange(0))
    assert_within(final, full_ref, full_bound, f"phases {dt} kernel={kernel}: the assembled output")
    if stats:
        slices = patch_slices(nimg, H, W, phase=True) if kernel else im2col_phase_slices(nimg, H, W)
        check_stats(cs, final, slices, f"phases {dt} kernel={kernel}", "conv parity phases colstats")


def test_conv_refusals_launch_nothing():
    """The fused GroupNorm input on the im2col kernel, a GEGLU flag and trailing padding on the shortcut form: refused with the
    documented code, the framed output untouched."""
    h = hip()
    from vface_amd.packing import pack_conv3x3
    dt, nimg, cin, cout, H = torch.float16, 1, 64, 128, 16
    x, w = conv_inputs(dt, nimg, cin, cout, H, H)
    out = Framed(nimg * H * H, cout, dt)
    ab = torch.ones(nimg, cin, 2, dtype=torch.float32, device=DEV)
    base = dict(nimg=nimg, H=H, W=H, cin=cin, cout=cout, ldx=cin + 16, ldy=out.ld)
    xd, wd = nhwc(x), pack_conv3x3(w).to(DEV)
    for kw in (dict(gn_ab=ab, flags=h.TUNE_NO_PATCH), dict(flags=h.EPI_GEGLU), dict(stride=3)):
        with pytest.raises(h.VFaceHipError, match=rf"\(code {ERR_SHAPE}\)"):
            h.conv3x3(xd, wd, out.view, **base, **kw)
    out.result("refused", rows=torch.arange(0))


# ================================================================================================ 2.3 the stamped instantiations
class StampBuffer:
    """The ``colstats`` argument of a VFACE_TUNE_STAMPS launch: ``count`` floats behind a 16-byte-aligned offset into a flat sentinel
    buffer, shaped ``[rows, n, 2]`` as the wrappers expect it (they pass its address and ``n`` on)."""

    def __init__(self, count, n):
        from kernel_bounds import sentinel
        self.count, self.lead = count, 20
        rows = -(-count // (2 * n))
        self.keep = sentinel(1, self.lead + rows * 2 * n + 64, torch.float32).reshape(-1)
        self.dev = self.keep.to(DEV)
        self.arg = self.dev[self.lead:self.lead + rows * 2 * n].view(rows, n, 2)

    def result(self, what, written=True):
        """The ``count`` floats of the layout, after the check that every float before and behind them is still the sentinel."""
        torch.cuda.synchronize()
        allv = self.dev.cpu()
        expect = self.keep.clone()
        if written:
            expect[self.lead:self.lead + self.count] = allv[self.lead:self.lead + self.count]
        assert same_bits(allv, expect), f"{what}: a stamp outside the layout"
        return allv[self.lead:self.lead + self.count].clone()


def assert_counts(c, what):
    assert torch.isfinite(c).all() and (c > 0).all() and (c < 2.0 ** 32).all(), (what, c)


@pytest.mark.parametrize("variant", [5, 6])
def test_gemm_stamped_instantiation(variant):
    """M 200 x N 320 x K 192 (a row tail in the second m-tile, a column tail at width 128, three K tiles: prologue, steady state and last
    tile): the stamped launch stores the bits of the plain one, and every wave of every workgroup files its counts inside
    ``2 x [workgroup][wave][4]`` floats."""
    h = hip()
    dt, M, N, K = torch.float16, 200, 320, 192
    a, w, b = strided(rnd((M, K), 31, dt), 8), rnd((N, K), 32, dt, 1 / math.sqrt(K)).to(DEV), rnd((N,), 33, torch.float32).to(DEV)
    nwg = -(-M // 128) * -(-N // (128 if variant == 5 else 160))
    plain, stamped, st = Framed(M, N, dt), Framed(M, N, dt), StampBuffer(2 * nwg * 16, N)
    h.gemm(a, w, plain.view, M=M, N=N, K=K, lda=K + 16, ldc=plain.ld, bias=b, flags=variant << 8, split_k=False)
    h.gemm(a, w, stamped.view, M=M, N=N, K=K, lda=K + 16, ldc=stamped.ld, bias=b, flags=(variant << 8) | h.TUNE_STAMPS, colstats=st.arg,
           split_k=False)
    want, got = plain.result(f"plain v{variant}"), stamped.result(f"stamped v{variant}")
    assert want.abs().max() > 0.5 and torch.equal(got, want)
    d = st.result(f"stamps v{variant}").view(2, nwg, 4, 4)
    assert_counts(d[0, :, :, :3], f"v{variant}: prologue, K loop, epilogue")
    assert torch.isfinite(d).all() and (d >= 0).all()


def test_conv_patch_stamped_instantiation():
    """64 -> 160 channels on one 16 x 16 image: one workgroup of eight waves, ``[workgroup][wave][8]`` floats."""
    h = hip()
    from vface_amd.packing import pack_conv3x3
    dt, nimg, cin, cout, H = torch.float16, 1, 64, 160, 16
    x, w = conv_inputs(dt, nimg, cin, cout, H, H)
    xd, wd, b = nhwc(x), pack_conv3x3(w).to(DEV), rnd((cout,), 34, torch.float32).to(DEV)
    plain, stamped, st = Framed(H * H, cout, dt), Framed(H * H, cout, dt), StampBuffer(8 * 8, cout)
    base = dict(nimg=nimg, H=H, W=H, cin=cin, cout=cout, ldx=cin + 16, bias=b)
    assert h.conv_uses_patch_kernel(H, H, cin, cout, 3, 1, False, h.TUNE_PATCH) == 1      # (the stamped plan is pinned in test_dispatch_cpu.py)
    h.conv3x3(xd, wd, plain.view, ldy=plain.ld, flags=h.TUNE_PATCH, **base)
    h.conv3x3(xd, wd, stamped.view, ldy=stamped.ld, flags=h.TUNE_PATCH | h.TUNE_STAMPS, colstats=st.arg, **base)
    want, got = plain.result("plain patch"), stamped.result("stamped patch")
    assert want.abs().max() > 0.5 and torch.equal(got, want)
    d = st.result("patch stamps").view(8, 8)
    assert_counts(d[:, :3], "patch: prologue, K loop, epilogue")
    assert torch.isfinite(d).all() and (d >= 0).all()


def test_stamped_launch_of_a_form_without_stamps_is_refused():
    """The fp32 output has no stamped instantiation: VFACE_ERR_SHAPE, neither the output nor the stamp buffer written."""
    h = hip()
    dt, M, N, K = torch.float16, 200, 320, 192
    a, w = rnd((M, K), 31, dt).to(DEV), rnd((N, K), 32, dt, 1 / math.sqrt(K)).to(DEV)
    out, st = Framed(M, N, torch.float32), StampBuffer(2 * 6 * 16, N)
    with pytest.raises(h.VFaceHipError, match=rf"\(code {ERR_SHAPE}\)"):
        h.gemm(a, w, out.view, M=M, N=N, K=K, lda=K, ldc=out.ld, flags=(5 << 8) | h.TUNE_STAMPS | h.EPI_OUT_F32, colstats=st.arg, split_k=False)
    out.result("refused", rows=torch.arange(0))
    st.result("refused", written=False)
