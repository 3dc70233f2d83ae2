"""The two convolution launches the conv-net engines share (vface_amd/convnet.py: `conv3`, `window`) on a bare ConvNetEngine, element by
element against fp64, in both compute types and with `split_k` on and off.

Two images of 12 x 20 (hw = 240 is no multiple of the 64- and 128-row tiles, so their tails are stored), the smallest channel counts
the launchers take (K, lda, ldw multiples of 8; N, ldc multiples of 4; a 16-byte aligned operand, an 8-byte aligned output).

The reference is the fp64 convolution of the ROUNDED 16-bit operands plus the fp32 bias, `ref`.  With S the same convolution of the
absolute values plus |b| and K = kh kw C_pad products per output, fp32 accumulation in any order -- the split-K partial sums and the
bias add included -- errs by at most acc = (K + 8) U32 S.  An fp32 output may be off by acc + U32 |ref|; a 16-bit output by
acc + 0.5 ulp(|ref| + acc), one rounding taken at the largest value the bound admits.  A zero-padded output column has S = 0."""
import functools

import pytest
import torch
import torch.nn.functional as F

from kernel_bounds import U32, assert_within, rnd, same_bits, sentinel, ulp

pytestmark = pytest.mark.gpu

DEV = "cuda"
DTYPES = [torch.float16, torch.bfloat16]
NIMG, H, W = 2, 12, 20

# name: (kh, kw, cin, cout, stride) + what the layer and the launch carry
CASES = {
    "stem7x7s2": dict(win=(7, 7, 3, 4, 2), cin_pad=8, tokens8=True),                 # from the 8-column token rows; N = 4
    "w1x5": dict(win=(1, 5, 8, 8, 1), bias=True),
    "w5x1": dict(win=(5, 1, 8, 6, 1), bias=True, cout_pad=8),                        # columns 6, 7 are padding
    "w1x1s2": dict(win=(1, 1, 8, 8, 2)),                                             # through im2col
    "w1x1slice": dict(win=(1, 1, 8, 8, 1), bias=True, slice=True),                   # no im2col; column slices in and out
    "w1x5out32": dict(win=(1, 5, 8, 8, 1), bias=True, out32=True),
    "w7x7split": dict(win=(7, 7, 24, 8, 1), bias=True),                              # K = 1176: the one shape here that splits K
    "c3": dict(win=(3, 3, 8, 8, 1)),
    "c3s2": dict(win=(3, 3, 8, 8, 2), bias=True, bn=True),                           # folded BatchNorm and bias
    "c3up": dict(win=(3, 3, 8, 4, 1), bias=True, upsample=True),
    "c3out32": dict(win=(3, 3, 16, 8, 1), bias=True, out32=True),
    "c3pad": dict(win=(3, 3, 8, 5, 1), bn=True, cout_pad=8),
}


def hip():
    from vface_amd import hip as h
    h.load()
    return h


@functools.lru_cache(None)
def state_dict():
    """fp32, variance-preserving weights so that the outputs are O(1)."""
    sd = {}
    for i, (name, c) in enumerate(CASES.items()):
        kh, kw, cin, cout, _ = c["win"]
        g = torch.Generator().manual_seed(100 + i)
        sd[name + ".weight"] = torch.randn(cout, cin, kh, kw, generator=g) / (kh * kw * cin) ** 0.5
        if c.get("bias"):
            sd[name + ".bias"] = torch.randn(cout, generator=g)
        if c.get("bn"):
            sd[name + ".bn.weight"], sd[name + ".bn.bias"] = torch.rand(cout, generator=g) + 0.5, torch.randn(cout, generator=g)
            sd[name + ".bn.running_mean"], sd[name + ".bn.running_var"] = torch.randn(cout, generator=g), torch.rand(cout, generator=g) + 0.1
    return sd


@functools.lru_cache(None)
def engine(dt, split_k):
    from vface_amd.convnet import ConvNetEngine
    eng = ConvNetEngine(dt, DEV)
    eng.split_k = split_k
    for name, c in CASES.items():
        eng.add_conv(state_dict(), name, name + ".bn" if c.get("bn") else None, cin_pad=c.get("cin_pad"), cout_pad=c.get("cout_pad"))
    return eng


@functools.lru_cache(None)
def reference(name, dt):
    """(input NCHW: fp32 for the token-row case, else 16-bit; ref, bound): fp64 [M, cout_pad], from the rounded operands alone."""
    from vface_amd.convnet import fold_bn
    c, sd = CASES[name], state_dict()
    kh, kw, cin, cout, stride = c["win"]
    x = rnd((NIMG, cin, H, W), 7 + len(name), torch.float32 if c.get("tokens8") else dt)
    w, b = sd[name + ".weight"], sd.get(name + ".bias")
    if c.get("bn"):
        w, b = fold_bn(w, *(sd[f"{name}.bn.{k}"] for k in ("weight", "bias", "running_mean", "running_var")), b=b)
    npad = c.get("cout_pad", cout) - cout
    w64 = F.pad(w.to(dt).double(), (0, 0, 0, 0, 0, 0, 0, npad))
    b64 = F.pad(b.double(), (0, npad)) if b is not None else torch.zeros(cout + npad, dtype=torch.float64)
    x64 = x.to(dt).double()
    if c.get("upsample"):
        x64 = F.interpolate(x64, scale_factor=2, mode="nearest")
    conv = lambda xx, ww, bb: F.conv2d(xx, ww, bb, stride=stride, padding=((kh - 1) // 2, (kw - 1) // 2)).permute(0, 2, 3, 1).reshape(-1, cout + npad)
    ref, S = conv(x64, w64, b64), conv(x64.abs(), w64.abs(), b64.abs())
    K = kh * kw * (c.get("cin_pad") or cin)
    acc = (K + 8) * U32 * S
    bound = acc + U32 * ref.abs() if c.get("out32") else acc + 0.5 * ulp(ref.abs() + acc, dt)
    return x, ref, bound


def tokens(x):
    return x.permute(0, 2, 3, 1).reshape(-1, x.shape[1]).contiguous()


@pytest.mark.parametrize("split_k", [True, False])
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("name", list(CASES))
def test_conv(name, dt, split_k):
    h, eng, c = hip(), engine(dt, split_k), CASES[name]
    kh, kw, cin, cout, stride = c["win"]
    x, ref, bound = reference(name, dt)
    p = eng.P[name]
    N = c.get("cout_pad", cout)
    assert p["cout"] == N and (p["b"] is None) == (not c.get("bias") and not c.get("bn"))
    up = 2 if c.get("upsample") else 1
    M = NIMG * ((up * H - 1) // stride + 1) * ((up * W - 1) // stride + 1)
    assert ref.shape == (M, N)
    odt = torch.float32 if c.get("out32") else dt
    # the output is the first M rows (for the slice case: columns 8 .. 15 of 24) of a sentinel-filled buffer
    cols, c0 = (24, 8) if c.get("slice") else (N, 0)
    host = sentinel(M + 1, cols, odt)
    buf = host.to(DEV)
    out = buf[:M, c0:c0 + N]
    if c.get("tokens8"):
        xd, C_, ldx = eng.tokens8(x.to(DEV)), 8, 8
        assert same_bits(xd.cpu()[:, :3], tokens(x).to(dt)) and not bool(xd[:, 3:].any())
    elif c.get("slice"):                        # columns 8 .. 15 of 24: ldx > C_
        wide = sentinel(NIMG * H * W, 24, dt)
        wide[:, 8:16] = tokens(x)
        xd, C_, ldx = wide.to(DEV)[:, 8:], cin, 24
    else:
        xd, C_, ldx = tokens(x).to(DEV), cin, cin
    if (kh, kw) == (3, 3):
        assert p["kind"] == "conv3"
        eng.conv3(name, xd, out, nimg=NIMG, H=H, W=W, ldx=ldx, stride=stride, upsample=bool(c.get("upsample")), out32=bool(c.get("out32")))
    else:
        assert p["kind"] == "gemm"
        if name == "w7x7split":                 # the launch this case is here for: split_k=True really splits
            assert h.load().vface_splitk_workspace_bytes(M, N, kh * kw * C_, 0, 1) > 0
        eng.window(name, xd, out, nimg=NIMG, H=H, W=W, C_=C_, ldx=ldx, stride=stride, out32=bool(c.get("out32")))
    torch.cuda.synchronize()
    got = buf.cpu()
    assert_within(got[:M, c0:c0 + N], ref, bound, f"{name} {dt} split_k={split_k}")
    if N > cout:
        assert not bool(got[:M, c0 + cout:c0 + N].any()), "the zero-padded output columns"
    assert same_bits(got[M:], host[M:]), "a store past the last row"
    if c.get("slice"):
        assert same_bits(got[:, :c0], host[:, :c0]) and same_bits(got[:, c0 + N:], host[:, c0 + N:]), "a store outside the column slice"


def test_fp32_compute_type_is_refused_at_construction():
    from vface_amd.convnet import ConvNetEngine
    with pytest.raises(hip().VFaceHipError, match="fp16 or bf16"):
        ConvNetEngine(torch.float32, DEV)
