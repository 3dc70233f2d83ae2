"""Face parsing on the MI355X: the kernels of csrc/parsing.hip one by one against fp64 on their exact 16-bit / 8-bit inputs, in
sentinel-filled buffers; the whole network against the reference's own runs (tests/golden/parse.npz); FaceParser, faceParsing_demo
and the CLI's --parse.

u = 2^-24 per fp32 operation (kernel_bounds.U32), d = half an ulp of the output type at the value the bound admits.  Every bound
is derived in its test's docstring from the operations the kernel performs; the network's bounds come from the reference's own
half-precision error E_ref, recorded in the fixture."""
import functools
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import GOLDEN, ROOT
from kernel_bounds import (U32, assert_within, channel_gate_ref_and_bound, pooled_linear_ref_and_bound, rnd, same_bits, sentinel,
                           ulp)

sys.path.insert(0, GOLDEN)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import cases_parse as cp  # noqa: E402
import parse_model as pm  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda"
DTYPES = [torch.float16, torch.bfloat16]


def hip():
    from vface_amd import hip as h
    h.load()
    return h


# ========================================================================================================== the kernels, alone
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("H2,W2,F_", [(16, 24, 2), (70, 66, 2), (1024, 1024, 1)])
def test_prefilter(dt, H2, W2, F_):
    """16 x 24 -> 8 x 12 (every pixel within reach of a reflected edge), 70 x 66 -> 35 x 33 (odd output sizes, grid tail) and the
    production 1024^2 -> 512^2.  Reference: tests/parse_model.prefilter in fp64 on the same bytes, with the kernel's fp32 taps and
    constants (they are its definition).  Bound, with A = sum |k| = 1.1875 and inputs in [0, 1]: x = u8 / 255 carries u; a
    vertical sum is 8 products and 8 additions on top, |error| <= 10 u A; the horizontal sum repeats that on values <= A with
    that error: <= A 10 u A + 9 u A^2 < 20 u A^2; the clamp does not expand it; the subtraction adds u |v - mean| <= u; the
    division by std_c scales all of it and adds u |result|; one rounding to the storage type:
        bound = (20 A^2 + 1) u / std_c + u |ref| + d.
    Channels 3..7 are +0, columns past the eighth keep their sentinel."""
    h = hip()
    g = np.random.Generator(np.random.PCG64([H2, W2]))
    u8 = np.stack([cp.crop(H2 // 2, W2 // 2, 40 + f) for f in range(F_)]) if H2 >= 64 else g.integers(0, 256, (F_, H2, W2, 3), dtype=np.uint8)
    u8[0, :4, :4] = 255
    u8[0, -4:, -4:] = 0
    M = F_ * (H2 // 2) * (W2 // 2)
    sent = sentinel(M + 1, 16, dt)
    od = sent.to(DEV)
    h.parse_prefilter(torch.from_numpy(u8).to(DEV), od[:M, :8])
    got = od.cpu()
    ref = torch.from_numpy(pm.prefilter(u8, np.float64).reshape(M, 3))
    A = float(np.abs(pm.taps().astype(np.float64)).sum())
    assert abs(A - 1.1875) < 1e-6
    b0 = (20 * A * A + 1) * U32 / torch.tensor(pm.SEG_STD.astype(np.float64)) + U32 * ref.abs()
    err = assert_within(got[:M, :3], ref, b0 + 0.5 * ulp(ref.abs() + b0, dt), f"prefilter {H2}x{W2} {dt}")
    print(f"prefilter {H2}x{W2} {dt}: max err {float(err.max()):.3e}")
    assert same_bits(got[:M, 3:8], torch.zeros(M, 5, dtype=dt)), "channels 3..7 must be +0"
    assert same_bits(got[:M, 8:], sent[:M, 8:]) and same_bits(got[M:], sent[M:]), "stores outside the eight channels"


def test_prefilter_refusals():
    h = hip()
    crops = torch.zeros(1, 16, 24, 3, dtype=torch.uint8, device=DEV)
    out = torch.full((96, 8), 7.0, dtype=torch.float16, device=DEV)
    for factor in (1, 4):
        with pytest.raises(h.VFaceHipError, match="shape"):
            h.parse_prefilter(crops, out, factor)
    with pytest.raises(h.VFaceHipError):
        h.parse_prefilter(crops, out.float(), 2)                                  # not a 16-bit type
    with pytest.raises(h.VFaceHipError):
        h.parse_prefilter(crops.cpu(), out, 2)
    assert bool((out == 7.0).all()), "a refusal must leave the output untouched"
    lib = h.load()
    assert lib.vface_parse_prefilter(crops.data_ptr(), 24, 15, 2, out.data_ptr(), 8, 1, 0, None) == -3     # odd height
    assert lib.vface_parse_prefilter(crops.data_ptr(), 24, 16, 2, out.data_ptr(), 8, 1, 5, None) == -4     # dtype code
    assert lib.vface_parse_prefilter(None, 24, 16, 2, out.data_ptr(), 8, 1, 0, None) == -1
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("C", [8, 64])
@pytest.mark.parametrize("H,W", [(6, 10), (7, 9)])
def test_maxpool(dt, H, W, C):
    """Three images, input and output column views of wider buffers (ld = C + 16).  Every input is negative, so a zero in place of
    the -inf padding would win at the border.  A maximum is one of its inputs: bit for bit against F.max_pool2d."""
    h = hip()
    nimg = 3
    OH, OW = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    xh = sentinel(nimg * H * W, C + 16, dt)
    xh[:, 8:8 + C] = -(rnd((nimg * H * W, C), 3 * C + H, dt).abs() + 0.125)
    yh = sentinel(nimg * OH * OW + 1, C + 16, dt)
    xd, yd = xh.to(DEV), yh.to(DEV)
    h.maxpool3x3s2(xd[:, 8:], yd[:, 8:], nimg=nimg, H=H, W=W, C_=C, ldx=C + 16, ldy=C + 16)
    got = yd.cpu()
    x = xh[:, 8:8 + C].float().reshape(nimg, H, W, C).permute(0, 3, 1, 2)
    ref = F.max_pool2d(x, 3, 2, 1).permute(0, 2, 3, 1).reshape(nimg * OH * OW, C).to(dt)
    assert bool((ref < 0).all())
    assert same_bits(got[:-1, 8:8 + C], ref)
    assert same_bits(got[:, :8], yh[:, :8]) and same_bits(got[:, 8 + C:], yh[:, 8 + C:]) and same_bits(got[-1:], yh[-1:])
    with pytest.raises(h.VFaceHipError):
        h.maxpool3x3s2(xd[:, 8:], yd[:, 8:], nimg=nimg, H=H, W=W, C_=C + 4, ldx=C + 16, ldy=C + 16)        # C % 8
    assert same_bits(yd.cpu(), got)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("C", [128, 256])
@pytest.mark.parametrize("form", ["none", "vec", "tensor", "x"])
@pytest.mark.parametrize("inplace", [False, True])
def test_channel_gate(dt, C, form, inplace):
    """y = x g + r for nimg = 3, hw = 4, all four forms of r, in place and not.  The kernel does one fp32 fma (the 16-bit operands
    and the fp32 gate are exact in it), then one rounding to the storage type: bound = u |ref| + d
    (kernel_bounds.channel_gate_ref_and_bound, which parse_bounds.check_stage applies to the engine's own operands)."""
    h = hip()
    nimg, hw = 3, 4
    M = nimg * hw
    xh = sentinel(M + 1, C + 8, dt)
    xh[:M, :C] = rnd((M, C), C + 1, dt)
    g = torch.rand(nimg, C, generator=torch.Generator().manual_seed(C)) * 1.2 - 0.1
    rvec = torch.randn(nimg, C, generator=torch.Generator().manual_seed(C + 2)) if form == "vec" else None
    rten = rnd((M, C), C + 3, dt) if form == "tensor" else None
    xd = xh.to(DEV)
    yd = xd if inplace else sentinel(M + 1, C + 8, dt).to(DEV)
    h.channel_gate(xd[:M], g.to(DEV), yd[:M], M=M, hw=hw, C_=C, rvec=None if rvec is None else rvec.to(DEV),
                   rten=None if rten is None else rten.to(DEV), add_x=form == "x")
    got = yd.cpu()
    ref, bound = channel_gate_ref_and_bound(xh[:M, :C], g, hw, dt, rvec=rvec, rten=rten, add_x=form == "x")
    assert_within(got[:M, :C], ref, bound, f"channel_gate {form} {dt}")
    assert same_bits(got[:M, C:], xh[:M, C:]) and same_bits(got[M:], xh[M:]), "stores outside the C channels"
    if not inplace:
        assert same_bits(xd.cpu(), xh)


def test_channel_gate_refusals():
    h = hip()
    x = torch.ones(12, 128, dtype=torch.float16, device=DEV)
    y = torch.full((12, 128), 7.0, dtype=torch.float16, device=DEV)
    g = torch.ones(3, 128, device=DEV)
    with pytest.raises(h.VFaceHipError):
        h.channel_gate(x, g, y, M=12, hw=4, C_=128, rvec=g, add_x=True)            # two forms of r at once
    with pytest.raises(h.VFaceHipError):
        h.channel_gate(x, g, y, M=12, hw=5, C_=128)                               # M % hw
    with pytest.raises(h.VFaceHipError):
        h.channel_gate(x, g, y, M=12, hw=4, C_=100)                               # C % 8
    with pytest.raises(h.VFaceHipError):
        h.channel_gate(x, g.half(), y, M=12, hw=4, C_=128)                        # the gate is fp32
    torch.cuda.synchronize()
    assert bool((y == 7.0).all())


@pytest.mark.parametrize("K,N,act,sa", [(512, 128, 1, 2), (128, 128, 3, 2), (256, 64, 1, 2), (64, 256, 3, 1)])
def test_pooled_linear(K, N, act, sa):
    """The four pooled 1x1 convolutions of the network (conv_avg, conv_atten, ffm.conv1, ffm.conv2), nimg = 3, the operand read
    with the stride vface_channel_stats leaves (2) or densely.  A lane adds ceil(K / 64) products in order, six butterfly levels
    follow, then the bias: every partial sum is bounded by S = sum |w a| + |b|, so |error| <= (ceil(K / 64) + 8) u S before the
    activation.  ReLU does not expand it; the sigmoid's slope is <= 1/4 and its own evaluation (expf, a division) is allowed
    4 x the relative error of torch's fp32 sigmoid on these inputs (kernel_bounds.cpu_fp32_rel_error): all of it is
    kernel_bounds.pooled_linear_ref_and_bound."""
    h = hip()
    nimg = 3
    g = torch.Generator().manual_seed(K + N)
    a = torch.randn(nimg, K, sa, generator=g)
    w = torch.randn(N, K, generator=g) / K ** 0.5
    b = torch.randn(N, generator=g) * 0.1
    out = torch.full((nimg + 1, N + 4), 7.0, device=DEV)
    h.pooled_linear(a.to(DEV), w.to(DEV), b.to(DEV), out[:nimg], nimg=nimg, N=N, K=K, lda=K * sa, sa=sa, act=act)
    got = out.cpu()
    ref, bound = pooled_linear_ref_and_bound(a[:, :, 0], w, b, "relu" if act == 1 else "sigmoid")
    assert_within(got[:nimg, :N], ref, bound, f"pooled_linear K={K} N={N} act={act}")
    assert bool((got[:nimg, N:] == 7.0).all()) and bool((got[nimg:] == 7.0).all())
    with pytest.raises(h.VFaceHipError):
        h.pooled_linear(a.to(DEV), w.to(DEV), b.to(DEV), out[:nimg], nimg=nimg, N=N, K=K, lda=K * sa, sa=sa, act=2)   # tanh: not built


def _logit_case(F_, h_, w_, seed, ld=32):
    g = torch.Generator().manual_seed(seed)
    lo = torch.full((F_ * h_ * w_, ld), float("nan"))
    lo[:, :19] = torch.randn(F_ * h_ * w_, 19, generator=g)
    return lo


@pytest.mark.parametrize("seg12", [False, True])
@pytest.mark.parametrize("F_,h_,w_,H,W", [(2, 2, 3, 16, 24), (2, 8, 8, 64, 64), (1, 64, 64, 512, 512)])
def test_upsample_argmax(F_, h_, w_, H, W, seg12):
    """N(0, 1) logits in 19 of 32 columns, NaN in the other 13 (a NaN that reached a comparison would change a label).  Reference:
    tests/parse_model.upsample in fp64 with the kernel's fp32 weights.  The kernel's value is ly0 (lx0 a + lx1 b) + ly1 (lx0 c +
    lx1 d): four roundings deep over terms whose absolute sum is at most m = max |logit| (lx0 + lx1 and ly0 + ly1 are 1 within u),
    so each interpolated logit is within B = 4 u m (1 + 2u) of the fp64 one, and the argmax can differ only where the fp64 margin
    is at most 2 B.  Labels must equal table[fp64 argmax] wherever the margin exceeds 2 B; at most 0.1 % of the pixels may be left
    out.  The frame past the output keeps its fill."""
    h = hip()
    from vface_amd import parsing
    lo = _logit_case(F_, h_, w_, 100 * h_ + H)
    table = parsing.seg12_table() if seg12 else parsing.identity_table()
    out = torch.full((F_ + 1, H, W), 0xAB, dtype=torch.uint8, device=DEV)
    h.upsample_argmax_u8(lo.to(DEV), table.to(DEV), F=F_, h=h_, w=w_, ncls=19, H=H, W=W, out=out[:F_])
    got = out.cpu().numpy()
    full = pm.upsample(lo[:, :19].double().numpy().reshape(F_, h_, w_, 19), H, W, np.float64)
    lab, margin = pm.argmax_and_margin(full)
    if F_ * h_ * w_ >= 128:      # (twelve low-resolution cells cannot show nineteen classes)
        assert len(np.unique(lab)) == 19
    B = 4 * U32 * float(lo[:, :19].abs().max()) * (1 + 2 * U32)
    sure = margin > 2 * B
    print(f"upsample_argmax {h_}x{w_}->{H}x{W}: B {B:.3e}, left out {1 - sure.mean():.2e}, differing anywhere {(got[:F_] != table.numpy()[lab]).sum()}")
    assert 1.0 - sure.mean() <= 1e-3
    assert np.array_equal(got[:F_][sure], table.numpy()[lab][sure])
    assert (got[F_] == 0xAB).all()


def test_upsample_argmax_ties_and_refusals():
    """Two classes with bit-identical planes that dominate every pixel: the lower index everywhere (torch.argmax's rule on ties)."""
    h = hip()
    from vface_amd import parsing
    lo = _logit_case(1, 8, 8, 9)
    lo[:, 3] += 10.0
    lo[:, 7] = lo[:, 3]
    ident = parsing.identity_table().to(DEV)
    got = h.upsample_argmax_u8(lo.to(DEV), ident, F=1, h=8, w=8, ncls=19, H=64, W=64)
    assert bool((got == 3).all())
    lo[:, 0] = lo[:, 3]
    assert bool((h.upsample_argmax_u8(lo.to(DEV), ident, F=1, h=8, w=8, ncls=19, H=64, W=64) == 0).all())
    # ncls not a multiple of four and the row no longer than it has to be: column 19 is loaded, never compared
    lo20 = lo[:, :20].contiguous()
    lo20[:, 19] = float("inf")
    assert bool((h.upsample_argmax_u8(lo20.to(DEV), ident, F=1, h=8, w=8, ncls=19, H=64, W=64) == 0).all())
    out = torch.full((1, 64, 64), 0xAB, dtype=torch.uint8, device=DEV)
    lod = lo.to(DEV)
    for kw in (dict(ncls=33), dict(ncls=0)):
        with pytest.raises(h.VFaceHipError):
            h.upsample_argmax_u8(lod, ident, F=1, h=8, w=8, H=64, W=64, out=out, **kw)
    with pytest.raises(h.VFaceHipError):
        h.upsample_argmax_u8(lod.half(), ident, F=1, h=8, w=8, ncls=19, H=64, W=64, out=out)
    lib = h.load()
    assert lib.vface_upsample_argmax_u8(lod.data_ptr(), 18, 1, 8, 8, 18, ident.data_ptr(), out.data_ptr(), 64, 64, None) == -2   # ld % 4
    torch.cuda.synchronize()
    assert bool((out == 0xAB).all()), "a refusal must leave the output untouched"


# ========================================================================================================== the whole network
@functools.lru_cache(None)
def fixture():
    z = np.load(os.path.join(GOLDEN, "parse.npz"), allow_pickle=False)
    return {k: z[k] for k in z.files}


@functools.lru_cache(None)
def state_dict():
    from vface_amd.pretrained.face_parsing import BiSeNet
    from vface_amd.utils import synth
    net = BiSeNet(n_classes=cp.N_CLASSES)
    synth.fill_parser_(net, seed=cp.WEIGHT_SEED)
    return net.state_dict()


@functools.lru_cache(None)
def engine(dt):
    from vface_amd.parsing import ParseEngine
    return ParseEngine(state_dict(), dt, DEV)


@functools.lru_cache(None)
def reference_margin(H, W):
    """Full-resolution fp64 margin (top - runner-up) of the reference's double-precision logits: computed once per size."""
    low = fixture()[f"{H}x{W}.logits64"].astype(np.float64)
    return pm.argmax_and_margin(pm.upsample(np.ascontiguousarray(low.transpose(1, 2, 0))[None], H, W, np.float64))[1][0]


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("H,W", cp.NET_SIZES)
def test_network(dt, H, W):
    """Three frames (the recorded one first) in one batch, then each alone.

    * every frame's logits and label maps are bit-identical to the same frame run alone;
    * logits: max |difference| from the reference's double-precision run <= 2 E_ref, E_ref = the reference's own half-precision
      (CPU) error against that run; the factor 2 covers the accumulation order of its half kernels against the fp32-accumulating
      MFMA path.  bf16: 8 x that (the ratio of the two types' ulps);
    * labels (19 and 12 classes) equal the reference's wherever its double-precision margin is >= 4 E_ref (32 E_ref for bf16) --
      each of two logits may move by the logit bound -- with at most 5 % of the pixels left out.

    Measured on an MI355X (max |logit difference| / bound, share of pixels left out, labels differing inside the rule): see
    DESIGN 9, "Face parsing"."""
    z, tag, eng = fixture(), f"{H}x{W}", engine(dt)
    e_ref = float(z[f"{tag}.e_ref"]) * (8.0 if dt == torch.bfloat16 else 1.0)
    seeds = [cp.SEEDS[(H, W)], 21, 22]
    crops = torch.from_numpy(np.stack([cp.crop(H, W, s) for s in seeds])).to(DEV)
    low = eng.logits(eng.prefilter(crops), 3, H, W)
    lab19, lab12 = eng.labels(crops, False), eng.labels(crops, True)
    assert low.shape == (3 * (H // 8) * (W // 8), 32) and low.dtype == torch.float32 and not bool(low[:, 19:].any())
    assert lab19.shape == (3, H, W) and lab19.dtype == torch.uint8
    hw8 = (H // 8) * (W // 8)
    for f in range(3):
        one = crops[f:f + 1].contiguous()
        assert torch.equal(eng.logits(eng.prefilter(one), 1, H, W).view(torch.int32), low[f * hw8:(f + 1) * hw8].view(torch.int32)), f
        assert torch.equal(eng.labels(one, False)[0], lab19[f]) and torch.equal(eng.labels(one, True)[0], lab12[f]), f
    got = low[:hw8, :19].cpu().double().reshape(H // 8, W // 8, 19).permute(2, 0, 1).numpy()
    err = float(np.abs(got - z[f"{tag}.logits64"].astype(np.float64)).max())
    sure = reference_margin(H, W) >= 4 * e_ref
    l19, l12 = lab19[0].cpu().numpy(), lab12[0].cpu().numpy()
    print(f"network {tag} {dt}: max |dlogit| {err:.3e} (bound {2 * e_ref:.3e}), left out {1 - sure.mean():.4f}, "
          f"labels differing inside the rule {(l19 != z[f'{tag}.labels19'])[sure].sum()}, anywhere {(l19 != z[f'{tag}.labels19']).sum()}")
    assert err <= 2 * e_ref
    assert 1.0 - sure.mean() <= 0.05
    assert np.array_equal(l19[sure], z[f"{tag}.labels19"][sure])
    assert np.array_equal(l12[sure], z[f"{tag}.labels12"][sure])


def test_network_refusals():
    h = hip()
    eng = engine(torch.float16)
    with pytest.raises(h.VFaceHipError, match="multiple of 32"):
        eng.labels(torch.zeros(1, 96, 128, 3, dtype=torch.uint8, device=DEV))
    with pytest.raises(h.VFaceHipError, match="GPU"):
        eng.labels(torch.zeros(1, 128, 128, 3, dtype=torch.uint8))
    with pytest.raises(h.VFaceHipError):
        eng.logits(torch.zeros(64 * 64, 8, dtype=torch.bfloat16, device=DEV), 1, 64, 64)          # the engine's type is fp16


# ================================================================================================================= the pipeline
@functools.lru_cache(None)
def face_parser():
    from vface_amd.pretrained.face_parsing import FaceParser
    return FaceParser(seg_ckpt=None, size=1024, device=DEV)


def test_face_parser_labels_equal_the_pieces_chained_by_hand():
    """1024^2 crops go straight in; 640^2 crops go through Pillow's bilinear resize (resample_u8 with the bilinear tables) first."""
    h = hip()
    from vface_amd.scripts.resample import resample_coeffs
    fp = face_parser()
    eng = fp.seg.engine
    crops = torch.from_numpy(np.stack([cp.crop(512, 512, 31), cp.crop(512, 512, 32)])).to(DEV)
    for seg12 in (True, False):
        got = fp.labels(crops, convert_to_seg12=seg12)
        low = eng.logits(eng.prefilter(crops), 2, 512, 512)
        ref = h.upsample_argmax_u8(low, eng.tables[seg12], F=2, h=64, w=64, ncls=19, H=512, W=512)
        assert got.shape == (2, 512, 512) and got.dtype == torch.uint8 and got.is_cuda and torch.equal(got, ref)
    assert int(fp.labels(crops).max()) < 12
    small = torch.from_numpy(cp.crop(320, 320, 33)[None]).to(DEV)
    b, k = (torch.from_numpy(t).to(DEV) for t in resample_coeffs(640, 1024, "bilinear"))
    big = h.resample_u8(h.resample_u8(small, 1024, 0, b, k), 1024, 1, b, k)
    assert torch.equal(fp.labels(small), eng.labels(big, True))


def test_face_parsing_demo_equals_the_batch_form():
    from PIL import Image
    from vface_amd.pretrained.face_parsing import faceParsing_demo
    fp = face_parser()
    u8 = cp.crop(512, 512, 34)
    crops = torch.from_numpy(u8[None]).to(DEV)
    for seg12 in (True, False):
        out = faceParsing_demo(fp, Image.fromarray(u8), convert_to_seg12=seg12)
        assert isinstance(out, np.ndarray) and out.dtype == np.uint8 and out.shape == (512, 512)
        assert np.array_equal(out, fp.labels(crops, convert_to_seg12=seg12)[0].cpu().numpy())
    seg = fp(Image.fromarray(u8))
    assert seg.dtype == torch.int64 and torch.equal(seg, fp.labels(crops, convert_to_seg12=False)[0].long())


def test_cli_parse(tmp_path):
    """`--synthetic --with_vae --intake --parse --paste_back`, two frames, one step, 512 x 512, the small UNet of the intake's CLI
    test: it runs, times a `parse` stage, and the label maps are the parser's, not the synthetic rings."""
    import yaml
    from test_intake_gpu import small_cfg
    from vface_amd.scripts import VFace_inference_batch as cli
    ypath = tmp_path / "small.yaml"
    ypath.write_text(yaml.safe_dump({"model": {"params": {"unet_config": {"params": dict(small_cfg(), image_size=64)}}}}))
    args = ["--synthetic", "--with_vae", "--intake", "--parse", "--paste_back", "--frame_size", "640", "--config", str(ypath),
            "--n_frames", "2", "--n_samples", "2", "--H", "512", "--W", "512", "--max_steps", "1", "--ddim_steps", "50", "--skip_save",
            "--Base_dir", str(tmp_path / "a")]
    opt = cli.build_parser().parse_args(args)
    opt.return_samples = True
    torch.manual_seed(opt.seed)
    b = cli.run_synthetic(opt)["batches"][0]
    assert b["finite"] and b["pixels"] == [2, 3, 512, 512] and b["pasted"] == [2, 640, 640, 3]
    assert b["stage_seconds"]["parse"] > 0 and b["stage_seconds"]["intake"] > 0
    labels = b["labels"]
    assert labels.shape == (2, 512, 512) and labels.dtype == torch.uint8 and labels.is_cuda and int(labels.max()) < 12
    rings = cli.synthetic_intake_inputs(2, 640, 512, 512, opt.seed + 1000)[2]
    assert not torch.equal(labels.cpu(), rings)
