"""The identity network's kernels per element against fp64 on the MI355X, fp16 and bf16: ``vface_prelu`` / ``vface_se_gate_add`` /
``vface_l2norm_rows`` / ``vface_id_prep`` (csrc/arcface.hip) within the bounds of arcface_bounds.py -- built from fp64 quantities of
the reference alone; test_arcface_bound_cpu.py shows that they admit torch's fp32 evaluation and refuse one-line defects -- and the
existing kernels at the shapes this network is the first to hand them: the stem's 3x3 with Cin = 8, ``vface_channel_stats`` at
hw = 49 and 12, the M = B head GEMM with K = 25088.  Outputs are views inside sentinel buffers whose frame is checked bit for bit
(``kernel_bounds.Framed``), every leading dimension differs from the width, and data movement (the strided shortcut read, the five
zero channels) is checked bit for bit."""
import math

import pytest
import torch

import arcface_bounds as ab
import clip_bounds as cb
from kernel_bounds import U32, Framed, assert_within, conv_ref_and_bound, gemm_ref_and_bound, note, rnd, same_bits, strided

pytestmark = pytest.mark.gpu

DEV = "cuda"
DTS = [torch.float16, torch.bfloat16]
ERR_ARG, ERR_SHAPE = -1, -3
CAP_ITEMS = 16384 * 256            # the launchers' vf_grid cap times the block: beyond it a thread takes more than one item


def hip():
    from vface_amd import hip as h
    h.load()
    return h


def _vecs(C_, seed):
    """(slope of both signs with 0 and 1 among them, za, zb) fp32 [C]."""
    slope = torch.cat([torch.linspace(-0.5, 0.5, C_ - 2), torch.tensor([0.0, 1.0])])
    return slope, rnd((C_,), seed, torch.float32) + 1.5, rnd((C_,), seed + 1, torch.float32)


# ------------------------------------------------------------------------------------------------ vface_prelu
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("C_", [8, 72])
@pytest.mark.parametrize("in_place", [False, True])
@pytest.mark.parametrize("with_z", [False, True])
def test_prelu(dt, C_, in_place, with_z):
    h = hip()
    M = 2 * 6 * 4
    x = rnd((M, C_), 100 + C_, dt, 2.0)
    slope, za, zb = _vecs(C_, 5)
    y, by, z, bz = ab.prelu_ref_and_bound(x, slope, dt, za if with_z else None, zb if with_z else None)
    out = Framed(M, C_, dt)
    if in_place:
        out.view.copy_(x.to(DEV))
        out.keep[1:1 + M, 8:8 + C_] = x
        xd = out.view
    else:
        xd = strided(x, 8)
    zf = Framed(M, C_, dt) if with_z else None
    h.prelu(xd, slope.to(DEV), out.view, M=M, C_=C_, z=zf.view if with_z else None, za=za.to(DEV) if with_z else None,
            zb=zb.to(DEV) if with_z else None)
    what = f"prelu {dt} C={C_} in_place={in_place} z={with_z}"
    note("prelu", assert_within(out.result(what), y, by, what), by)
    if with_z:
        note("prelu z", assert_within(zf.result(what + " z"), z, bz, what + " z"), bz)
    if not in_place:
        assert same_bits(xd.cpu(), x), "the input changed"


def test_prelu_past_the_launch_cap():
    """M (C / 8) > 16384 x 256: threads take a second item.  y is x or ONE fp32 product rounded once: the CPU's fp32 gives the same
    bits, so the comparison is exact (and cheap at 34 M elements); z = fma, rounded once, likewise."""
    h = hip()
    dt, C_ = torch.float16, 8
    M = CAP_ITEMS + 4099
    assert M * (C_ // 8) > CAP_ITEMS
    x = rnd((M, C_), 9, dt, 2.0)
    slope, za, zb = _vecs(C_, 7)
    out, zf = Framed(M, C_, dt), Framed(M, C_, dt)
    h.prelu(strided(x, 8), slope.to(DEV), out.view, M=M, C_=C_, z=zf.view, za=za.to(DEV), zb=zb.to(DEV))
    f = x.float()
    y32 = torch.where(f > 0, f, slope * f)
    assert same_bits(out.result("prelu past the cap"), y32.to(dt))
    z64 = za.double() * y32.double() + zb.double()              # exact in fp64: one rounding to fp32, then one to fp16 -- not
    got = zf.result("prelu past the cap, z").double()           # always the fma's single rounding, so: within half an ulp + U32
    assert_within(got, z64, ab.as_16bit(z64, U32 * z64.abs(), dt), "prelu past the cap, z")


def test_prelu_refusals_launch_nothing():
    h = hip()
    dt = torch.float16
    x = strided(rnd((8, 16), 1, dt), 8)
    slope = torch.ones(16, device=DEV)
    out = Framed(8, 16, dt)
    with pytest.raises(h.VFaceHipError, match=rf"\(code {ERR_ARG}\)"):      # z aliases y
        h.prelu(x, slope, out.view, M=8, C_=16, z=out.view, za=slope, zb=slope)
    with pytest.raises(h.VFaceHipError):                                    # C % 8
        h.prelu(x, slope[:12].contiguous(), out.view, M=8, C_=12)
    with pytest.raises(h.VFaceHipError):                                    # fp16 slopes
        h.prelu(x, slope.half(), out.view, M=8, C_=16)
    out.result("refused", rows=torch.arange(0))


# ------------------------------------------------------------------------------------------------ vface_se_gate_add
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("H,W", [(6, 4), (7, 5)])
@pytest.mark.parametrize("mode", ["s1", "s2", "same"])
@pytest.mark.parametrize("with_z", [False, True])
def test_se_gate_add(dt, H, W, mode, with_z):
    """``s1`` / ``s2``: the shortcut is the unit's H x W input read at stride 1 / 2; ``same``: a tensor of the output's size."""
    h = hip()
    nimg, C_ = 3, 24
    s = 2 if mode == "s2" else 1
    OH, OW = (H - 1) // s + 1, (W - 1) // s + 1
    M = nimg * OH * OW
    res = rnd((M, C_), 11, dt)
    xin = rnd((nimg * H * W if mode != "same" else M, C_), 12, dt)
    g = torch.sigmoid(rnd((nimg, C_), 13, torch.float32))
    _, za, zb = _vecs(C_, 14)
    sc = ab.strided_rows(xin, nimg, H, W, s) if mode != "same" else xin
    y, by, z, bz = ab.se_gate_add_ref_and_bound(res, g, sc, dt, nimg=nimg, za=za if with_z else None, zb=zb if with_z else None)
    out = Framed(M, C_, dt)
    zf = Framed(M, C_, dt) if with_z else None
    gd = strided(g, 4)
    size = dict(H=OH, W=OW, sc_stride=0) if mode == "same" else dict(H=H, W=W, sc_stride=s)
    h.se_gate_add(strided(res, 8), gd, strided(xin, 16), out.view, nimg=nimg, C_=C_, z=zf.view if with_z else None,
                  za=za.to(DEV) if with_z else None, zb=zb.to(DEV) if with_z else None, **size)
    what = f"se_gate_add {dt} {H}x{W} {mode} z={with_z}"
    note("se_gate_add", assert_within(out.result(what), y, by, what), by)
    if with_z:
        note("se_gate_add z", assert_within(zf.result(what + " z"), z, bz, what + " z"), bz)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("H,W,s", [(6, 4, 2), (7, 5, 2), (7, 5, 1)])
def test_se_gate_add_reads_the_strided_pixel(dt, H, W, s):
    """Every pixel of the input holds its own row index (at most 3 x 35 - 1 = 104: exact in both types) and the residual is zero:
    the output IS the index of the pixel each output row read -- (n, oy s, ox s), OH = (H - 1) / s + 1."""
    h = hip()
    nimg, C_ = 3, 8
    OH, OW = (H - 1) // s + 1, (W - 1) // s + 1
    M = nimg * OH * OW
    xin = torch.arange(nimg * H * W, dtype=torch.float32)[:, None].expand(-1, C_).to(dt).contiguous()
    out = Framed(M, C_, dt)
    h.se_gate_add(torch.zeros(M, C_, dtype=dt, device=DEV), torch.ones(nimg, C_, device=DEV), strided(xin, 8), out.view, nimg=nimg, H=H, W=W,
                  C_=C_, sc_stride=s)
    want = torch.tensor([(n * H + oy * s) * W + ox * s for n in range(nimg) for oy in range(OH) for ox in range(OW)], dtype=torch.float32)
    assert OH == math.ceil(H / s) and torch.equal(out.result("index")[:, 0].float(), want)
    assert torch.equal(out.result("index").float(), want[:, None].expand(-1, C_))


def test_se_gate_add_refusals_launch_nothing():
    h = hip()
    dt = torch.float16
    res, xin = strided(rnd((12, 16), 1, dt), 8), strided(rnd((24, 16), 2, dt), 8)
    g = torch.ones(1, 16, device=DEV)
    out = Framed(12, 16, dt)
    with pytest.raises(h.VFaceHipError, match=rf"\(code {ERR_SHAPE}\)"):
        h.se_gate_add(res, g, xin, out.view, nimg=1, H=6, W=4, C_=16, sc_stride=3)
    with pytest.raises(h.VFaceHipError, match=rf"\(code {ERR_ARG}\)"):      # z without its pair is refused by the wrapper or the library
        h.se_gate_add(res, g, xin, out.view, nimg=1, H=6, W=4, C_=16, sc_stride=2, z=res, za=g[0].contiguous(), zb=g[0].contiguous())
    with pytest.raises(h.VFaceHipError):
        h.se_gate_add(res, g.half(), xin, out.view, nimg=1, H=6, W=4, C_=16, sc_stride=2)
    out.result("refused", rows=torch.arange(0))


# ------------------------------------------------------------------------------------------------ vface_l2norm_rows
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("N", [512, 8])
def test_l2norm_rows(B, N):
    """Row 0 ordinary; with B = 3 row 1 tiny (1e-25: its squares vanish in fp32) and row 2 large (1e25: they overflow)."""
    h = hip()
    x = rnd((B, N), 20 + N, torch.float32)
    if B == 3:
        x[1] *= 1e-25
        x[2] *= 1e25
    ref, bound = ab.l2norm_ref_and_bound(x)
    out = Framed(B, N, torch.float32)
    h.l2norm_rows(strided(x, 4), out.view, B=B, N=N)
    got = out.result(f"l2norm B={B} N={N}")
    note("l2norm", assert_within(got, ref, bound, f"l2norm B={B} N={N}"), bound)
    assert float((got.double().norm(dim=1) - 1).abs().max()) < 1e-5
    if B == 3:      # a row's bits do not depend on the batch
        alone = Framed(1, N, torch.float32)
        h.l2norm_rows(strided(x[:1].contiguous(), 4), alone.view, B=1, N=N)
        assert same_bits(alone.result("alone"), got[:1])


# ------------------------------------------------------------------------------------------------ vface_id_prep
def _check_prep(h, dt, img, ref, bound, what, **kw):
    B = img.shape[0]
    out = Framed(B * 112 * 112, 8, dt)
    h.id_prep(img.to(DEV), out.view, **kw)
    got = out.result(what)
    assert same_bits(got[:, 3:], torch.zeros(B * 112 * 112, 5, dtype=dt)), f"{what}: channels 3..7 are zero"
    want, b = ab.rows8(ref)[:, :3], ab.rows8(bound)[:, :3]
    print(f"{what}: bound median {float(b.median()):.2e}, |ref| median {float(want.abs().median()):.2e}")
    note("id_prep", assert_within(got[:, :3], want, b, what), b)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("S", [224, 256])
@pytest.mark.parametrize("clip_img", [True, False])
def test_id_prep_on_noise(dt, S, clip_img):
    """Noise: neighbouring pixels are unrelated, so a bin edge off by one anywhere moves an output by a large fraction of a pixel's
    value (test_arcface_bound_cpu.py moves every edge and sees each beyond this bound).  224: both pools; 256: the second only."""
    h = hip()
    img = torch.randn(2, 3, S, S, generator=torch.Generator().manual_seed(S + clip_img))
    ref, bound = ab.id_prep_ref_and_bound(img, dt, clip_img=clip_img)
    _check_prep(h, dt, img, ref, bound, f"id_prep {dt} {S} clip_img={clip_img}", clip_img=clip_img)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("H,W", [(64, 48), (512, 512)])
def test_id_prep_from_frames(dt, H, W):
    """prep == 1: a [-1, 1] frame and a mask -> the CLIP image in ``vface_clip_patches``' order (its fp64 value and fp32 error
    terms: clip_bounds) -> the chain."""
    h = hip()
    frames = cb.smooth_frames(2, H, W, seed=H)
    mask = (torch.rand(2, H, W, generator=torch.Generator().manual_seed(5)) > 0.6).float()
    for mk in (mask, None):
        clip64, e32 = ab.clip_image_ref_and_e32(frames, mk)
        ref, bound = ab.id_prep_ref_and_bound(clip64, dt, clip_img=True, e_in=e32)
        _check_prep(h, dt, frames, ref, bound, f"id_prep from frames {dt} {H}x{W} mask={mk is not None}", prep=True,
                    mask=None if mk is None else mk.to(DEV))


def test_id_prep_refusals_launch_nothing():
    h = hip()
    out = Framed(112 * 112, 8, torch.float16)
    with pytest.raises(h.VFaceHipError, match=rf"\(code {ERR_SHAPE}\)"):      # a 256-high image is cropped as it is: [32:220] needs W >= 220
        h.id_prep(torch.zeros(1, 3, 256, 200, device=DEV), out.view)
    with pytest.raises(h.VFaceHipError, match=rf"\(code {ERR_ARG}\)"):        # a mask belongs to prep
        h.id_prep(torch.zeros(1, 3, 224, 224, device=DEV), out.view, mask=torch.zeros(1, 224, 224, device=DEV))
    with pytest.raises(h.VFaceHipError, match=rf"\(code {ERR_ARG}\)"):        # a frame becomes a CLIP image: clip_img cannot be off
        h.id_prep(torch.zeros(1, 3, 64, 64, device=DEV), out.view, prep=True, clip_img=False)
    out.result("refused", rows=torch.arange(0))


# ------------------------------------------------------------------------------------------------ existing kernels, new shapes
@pytest.mark.parametrize("dt", DTS)
def test_stem_conv3x3_cin8(dt):
    """The stem: 3x3, Cin = 8 (K = 72) -> 64 with a bias, on 6 x 4, two images; within ``conv_ref_and_bound``."""
    h = hip()
    from vface_amd.packing import pack_conv3x3
    nimg, cin, cout, H, W = 2, 8, 64, 6, 4
    x = (rnd((nimg, cin, H, W), 31, dt).float() + 1.0).to(dt)
    x[:, 3:] = 0                                                 # the stem's rows: three values, five zeros
    w = rnd((cout, cin, 3, 3), 32, dt, 1 / math.sqrt(27))
    bias = rnd((cout,), 33, torch.float32)
    out = Framed(nimg * H * W, cout, dt)
    xd = strided(x.permute(0, 2, 3, 1).reshape(nimg * H * W, cin).contiguous(), 8)
    h.conv3x3(xd, pack_conv3x3(w, 8).to(DEV), out.view, nimg=nimg, H=H, W=W, cin=cin, cout=cout, ldx=cin + 16, ldy=out.ld, bias=bias.to(DEV),
              split_k=False)
    ref, bound = conv_ref_and_bound(x, w, dt, bias=bias)
    note("stem conv", assert_within(out.result(f"stem conv {dt}"), ref, bound, f"stem conv {dt}"), bound)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("hw,C_", [(49, 512), (12, 64)])
def test_channel_stats_means_on_small_maps(dt, hw, C_):
    """The squeeze-excite pool: the mean ``vface_channel_stats`` leaves at [..., 0], hw = 49 (the last stage's 7 x 7) and 12, three
    images.  Bound: test_glue_kernels_gpu.test_channel_stats_and_norm's, one slice: L = ceil(hw / 32) + 34 fp32 roundings of sums
    about the channel's first pixel, d_mean = L U32 mean |x - p| + U32 |mean|."""
    h = hip()
    nimg = 3
    x = (rnd((nimg, hw, C_), 40 + hw, dt).float() + torch.linspace(-3, 3, C_)).to(dt)
    x64 = x.double()
    mean = x64.mean(1)
    L = -(-hw // 32) + 34
    bound = L * U32 * (x64 - x64[:, :1]).abs().mean(1) + U32 * mean.abs()
    stats = h.channel_stats(strided(x.reshape(nimg * hw, C_), 8), nimg=nimg, hw=hw, C_=C_, ldx=C_ + 16)
    torch.cuda.synchronize()
    note("se pool", assert_within(stats.cpu()[..., 0], mean, bound, f"channel means hw={hw}"), bound)
    one = h.channel_stats(strided(x[:1].reshape(hw, C_).contiguous(), 8), nimg=1, hw=hw, C_=C_, ldx=C_ + 16)
    assert same_bits(one.cpu(), stats.cpu()[:1]), "an image's statistics do not depend on the batch"


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("M", [1, 3])
def test_head_gemm_k25088(dt, M):
    """The output layer: M = B rows of K = 25088 against [512][25088], bias, fp32 out, no split-K; within ``gemm_ref_and_bound``.
    Row 0 of the M = 3 launch has the bits of the M = 1 launch."""
    h = hip()
    N, K = 512, 25088
    a, w = rnd((3, K), 50, dt), rnd((N, K), 51, dt, 1 / math.sqrt(K))
    bias = rnd((N,), 52, torch.float32)
    out = Framed(M, N, torch.float32)
    wd = w.to(DEV)
    h.gemm(strided(a[:M].contiguous(), 8), wd, out.view, M=M, N=N, K=K, lda=K + 16, ldc=out.ld, bias=bias.to(DEV), flags=h.EPI_OUT_F32,
           split_k=False)
    ref, bound = gemm_ref_and_bound(a[:M], w, dt, bias=bias, out_f32=True)
    got = out.result(f"head gemm {dt} M={M}")
    note("head gemm", assert_within(got, ref, bound, f"head gemm {dt} M={M}"), bound)
    if M == 3:
        one = Framed(1, N, torch.float32)
        h.gemm(strided(a[:1].contiguous(), 8), wd, one.view, M=1, N=N, K=K, lda=K + 16, ldc=one.ld, bias=bias.to(DEV), flags=h.EPI_OUT_F32,
               split_k=False)
        assert same_bits(one.result("head gemm alone"), got[:1]), "a sample's features do not depend on the batch"
