"""The glue kernels of the flow producer (csrc/raft.hip) and of the VAE / UNet plumbing (csrc/pointwise.hip), one by one, at the
shapes the product runs (512 x 512 frames) and at the edges where such kernels go wrong.

Every case rounds its inputs to the 16-bit type first and computes the reference in fp64 on the CPU from those exact values.
Data movement is compared bit for bit.  Arithmetic is compared element by element against a bound derived in the test's
docstring: u = 2^-24 per fp32 operation, 0.5 ulp of the output type on top; no rel-L2 (an L2 norm hides one wrong pixel).
Outputs are written into sentinel-filled buffers, so a store outside the slot fails the test.  "Wrap" cases pass the launch cap
(16384 blocks of 256 in raft.hip, 8192 in pointwise.hip), so a thread's second trip through its grid-stride loop is compared too.

Transcendental steps (tanhf, __expf, exp2, expf): the operation count does not bound them.  Their allowance is taken from the
reference's own arithmetic -- 4 x the worst relative error of torch's fp32 function against fp64 on the inputs of the case, at
least 4 x 2^-23 (kernel_bounds.cpu_fp32_rel_error; the factor 4 because the fast GPU exponentials are specified a few ulp
looser than libm's) -- plus 2^-126 absolute where an fp32 intermediate may be flushed."""
import math

import pytest
import torch
import torch.nn.functional as F

from kernel_bounds import (TINY32, U32, act_ref_and_bound, assert_within, avgpool2_ref, channel_norm_ref_and_bound,
                           channel_stats_ref_and_bound, convex_upsample_ref_and_bound, corr_lookup_ref_and_bound, cpu_fp32_rel_error,
                           flow_update_ref, gru_gate_ref_and_bound, gru_update_ref_and_bound, norm_act_pre_ref_and_bound, rnd, same_bits,
                           sentinel, softmax_rows_ref_and_bound, ulp)

pytestmark = pytest.mark.gpu

DEV = "cuda"
DTYPES = [torch.float16, torch.bfloat16]
CAP_RAFT = 16384 * 256                # work items past which raft.hip's kernels wrap
CAP_POINT = 8192 * 256                # the same for pointwise.hip


def hip():
    from vface_amd import hip as h
    h.load()
    return h


def randn(shape, seed, scale=1.0):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale


def fmax(dt):
    return torch.finfo(dt).max


# ====================================================================================== pure data movement: bit for bit
def _im2col_ref(x, nimg, H, W, C, kh, kw, stride):
    """[nimg H W, C] 16-bit -> [M, kh kw C] in (tap, channel) order from F.unfold, on the bit patterns (exact in fp32)."""
    bits = x.contiguous().view(torch.int16).float().reshape(nimg, H, W, C).permute(0, 3, 1, 2)
    cols = F.unfold(bits, (kh, kw), padding=((kh - 1) // 2, (kw - 1) // 2), stride=stride)      # [nimg, C kh kw, L], channel-major
    L = cols.shape[-1]
    return cols.reshape(nimg, C, kh * kw, L).permute(0, 3, 2, 1).reshape(nimg * L, kh * kw * C).to(torch.int16).view(x.dtype)


WINDOWS = [(7, 7, 2), (1, 5, 1), (5, 1, 1), (1, 1, 2), (3, 3, 1), (3, 3, 2)]


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("C", [8, 96, 328, 384])
@pytest.mark.parametrize("kh,kw,stride", WINDOWS)
def test_im2col(dt, kh, kw, stride, C):
    """The window matrix of the engines' `window` (pad = (k - 1) // 2) at an odd 13 x 11 map (the stride-2 output size rounds),
    three images, the input a column view of a wider buffer (ldx = C + 16) and the output rows 8 sentinel columns longer than
    kh kw C.  Zero padding is +0, as F.unfold's."""
    h = hip()
    nimg, H, W = 3, 13, 11
    OH, OW = (H - 1) // stride + 1, (W - 1) // stride + 1
    M, K = nimg * OH * OW, kh * kw * C
    xh = sentinel(nimg * H * W, C + 16, dt)
    xh[:, 8:8 + C] = rnd((nimg * H * W, C), 7 * C + kh, dt)
    oh = sentinel(M, K + 8, dt)
    xd, od = xh.to(DEV), oh.to(DEV)
    h.im2col(xd[:, 8:], od, nimg=nimg, H=H, W=W, C_=C, kh=kh, kw=kw, stride=stride, pad_y=(kh - 1) // 2, pad_x=(kw - 1) // 2, ldx=C + 16)
    got = od.cpu()
    ref = _im2col_ref(xh[:, 8:8 + C], nimg, H, W, C, kh, kw, stride)
    assert ref.shape == (M, K)
    assert same_bits(got[:, :K], ref), f"first differing row {int((got[:, :K] != ref).any(1).int().argmax())}"
    assert same_bits(got[:, K:], oh[:, K:]), "columns past kh kw C must not change"
    assert same_bits(xd.cpu(), xh)


@pytest.mark.parametrize("dt", DTYPES)
def test_im2col_wrap_stem_512(dt):
    """Wrap: the 7 x 7 stride-2 stem of two 512 x 512 images, 131072 x 49 x 1 = 6.4 M items (cap 4.19 M)."""
    h = hip()
    nimg, H, W, C = 2, 512, 512, 8
    M, K = nimg * 256 * 256, 49 * C
    assert M * 49 * (C // 8) > CAP_RAFT
    xh = rnd((nimg * H * W, C), 5, dt)
    od = sentinel(M + 1, K, dt).to(DEV)
    h.im2col(xh.to(DEV), od, nimg=nimg, H=H, W=W, C_=C, kh=7, kw=7, stride=2, pad_y=3, pad_x=3)
    got = od.cpu()
    ref = _im2col_ref(xh, nimg, H, W, C, 7, 7, 2)
    assert same_bits(got[:M], ref), f"first differing row {int((got[:M] != ref).any(1).int().argmax())}"
    assert same_bits(got[M:], sentinel(M + 1, K, dt)[M:]), "the row past the matrix must not change"


def test_im2col_refusals():
    h = hip()
    z = lambda cols: torch.zeros(3 * 13 * 11, cols, dtype=torch.float16, device=DEV)
    x, out = z(32), z(9 * 32)
    kw = dict(nimg=3, H=13, W=11, kh=3, kw=3, stride=1, pad_y=1, pad_x=1)
    h.im2col(x, out, C_=16, ldx=32, **kw)                                       # (the accepted form of the calls below)
    with pytest.raises(h.VFaceHipError):
        h.im2col(x, out, C_=12, ldx=32, **kw)                                   # C % 8
    with pytest.raises(h.VFaceHipError):
        h.im2col(x, out, C_=16, ldx=20, **kw)                                   # ldx % 8
    with pytest.raises(h.VFaceHipError):
        h.im2col(x, z(9 * 32 + 4), C_=16, ldx=32, **kw)                          # ldo % 8
    with pytest.raises(h.VFaceHipError):
        h.im2col(x, z(9 * 8), C_=16, ldx=32, **kw)                               # ldo < kh kw C
    with pytest.raises(h.VFaceHipError):
        h.im2col(x, out, C_=16, ldx=32, nimg=3, H=13, W=5, kh=7, kw=7, stride=2, pad_y=0, pad_x=0)      # (5 - 7) / 2 + 1 = 0 columns


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("rows,cols,wrap", [(37, 128, False), (1, 8, False), (9 * 16384 + 3, 128, True)])
def test_copy2d_columns_of_a_wider_buffer(dt, rows, cols, wrap):
    """The engine's copy hx[:, 256:] -> rhx[:, 256:] (ld 384 both): the slot equals the source bit for bit, every other column
    of the target keeps its sentinel.  Wrap: 147459 rows x 16 vectors = 2.36 M items (cap 2.10 M)."""
    h = hip()
    assert (rows * (cols // 8) > CAP_POINT) == wrap
    src = sentinel(rows, 384, dt)
    src[:, 256:256 + cols] = rnd((rows, cols), rows + cols, dt)
    dsth = sentinel(rows + 1, 384, dt).flip(0).contiguous()
    sd, dd = src.to(DEV), dsth.to(DEV)
    h.copy2d(sd[:, 256:], dd[:, 256:], rows=rows, cols=cols, ld_src=384, ld_dst=384)
    got = dd.cpu()
    assert same_bits(got[:rows, 256:256 + cols], src[:, 256:256 + cols])
    keep = dsth.clone()
    keep[:rows, 256:256 + cols] = src[:, 256:256 + cols]
    assert same_bits(got, keep), "a store outside the slot"
    assert same_bits(sd.cpu(), src)
    if not wrap:
        with pytest.raises(h.VFaceHipError):
            h.copy2d(sd[:, 256:], dd[:, 256:], rows=rows, cols=cols + 4, ld_src=384, ld_dst=384)      # cols % 8


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("N,C,hw,cpad", [(3, 3, 13 * 11, 8), (2, 4, 77, 4), (1, 9, 5, 16), (2, 3, 512 * 512, 8)])
def test_nchw_to_nhwc(dt, N, C, hw, cpad):
    """fp32 NCHW -> 16-bit tokens [N hw, cpad]: the value's own rounding (x.to(dt)), channels C .. cpad - 1 are +0, nothing past
    the last row.  The last case is the engines' `tokens8` of two 512 x 512 images: 4.19 M items, a wrap (cap 2.10 M)."""
    h = hip()
    x = randn((N, C, hw), N * hw + C, 3.0)
    oh = sentinel(N * hw + 1, cpad, dt)
    od = oh.to(DEV)
    h.nchw_to_nhwc(x.to(DEV), od, N=N, C_=C, hw=hw, cpad=cpad)
    ref = torch.zeros(N, hw, cpad, dtype=dt)
    ref[:, :, :C] = x.permute(0, 2, 1).to(dt)
    got = od.cpu()
    assert same_bits(got[:N * hw], ref.reshape(N * hw, cpad))
    assert same_bits(got[N * hw:], oh[N * hw:])


@pytest.mark.parametrize("N,C,hw,ldx", [(3, 4, 13 * 11, 8), (1, 3, 1, 3), (2, 5, 1000, 16), (9, 4, 65536, 8)])
def test_nhwc_to_nchw_f32(N, C, hw, ldx):
    """fp32 tokens with row stride ldx > C -> NCHW, bit for bit.  The last case is 2.36 M items, a wrap (cap 2.10 M)."""
    h = hip()
    x = randn((N * hw, ldx), N + hw, 2.0)
    oh = sentinel(1, N * C * hw + 7, torch.float32)[0]
    od = oh.to(DEV)
    h.nhwc_to_nchw_f32(x.to(DEV), od, N=N, C_=C, hw=hw, ldx=ldx)
    got = od.cpu()
    ref = x.reshape(N, hw, ldx)[:, :, :C].permute(0, 2, 1).reshape(-1)
    assert same_bits(got[:N * C * hw], ref.contiguous())
    assert same_bits(got[N * C * hw:], oh[N * C * hw:])


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("with_inv", [False, True])
def test_pack_unet_input_two_and_three_chunks(dt, with_inv):
    """x_in = cat[x9, x9, cat[inv, inpaint, mask]] as 16-bit tokens padded to cpad; `inv=None` packs the first two chunks only
    and must leave the rows of a third alone."""
    h = hip()
    Fn, hh, ww, cpad = 3, 5, 7, 16
    hw = hh * ww
    x, inv, inp, mask = randn((Fn, 4, hw), 1), randn((Fn, 4, hw), 2), randn((Fn, 4, hw), 3), randn((Fn, 1, hw), 4)
    oh = sentinel(3 * Fn * hw + 1, cpad, dt)
    od = oh.to(DEV)
    d = lambda t: t.to(DEV)
    h.pack_unet_input(d(x), d(inv) if with_inv else None, d(inp), d(mask), od, F=Fn, h=hh, w=ww, cpad=cpad)
    chunks = [x, x, inv][:3 if with_inv else 2]
    ref = torch.zeros(len(chunks), Fn, hw, cpad, dtype=dt)
    for k, first in enumerate(chunks):
        ref[k, :, :, :9] = torch.cat([first, inp, mask], 1).permute(0, 2, 1).to(dt)
    n = len(chunks) * Fn * hw
    got = od.cpu()
    assert same_bits(got[:n], ref.reshape(n, cpad))
    assert same_bits(got[n:], oh[n:]), "rows past the packed chunks must not change"


def _cast_table(dt):
    """Ties to even, the largest finite value, the first value that rounds to inf, subnormals of the target, signed zeros, inf, NaN."""
    fi = torch.finfo(dt)
    p = {torch.float16: 10, torch.bfloat16: 7}[dt]
    half = 2.0 ** -(p + 1)
    sub = fi.smallest_normal * 2.0 ** -p                     # smallest subnormal of dt
    vals = [1.0 + half, 1.0 + 3 * half, 1.0 + half * (1 + 2.0 ** -10), 1.0 + half * (1 - 2.0 ** -10), 2.0 + 2 * half, 2.0 + 6 * half,
            fi.max, fi.max * (1 + half * 0.999), fi.max * (1 + half), fi.max * (1 + 2 * half), fi.smallest_normal, fi.smallest_normal * (1 - half),
            sub, 0.5 * sub, 0.5 * sub * (1 + 2.0 ** -10), 1.5 * sub, 2.5 * sub, 0.25 * sub, 0.0, float("inf"), float("nan"), 65504.0, 65519.99, 65520.0]
    t = torch.tensor(vals, dtype=torch.float64).to(torch.float32)
    return torch.cat([t, -t])


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("count", [48, 1000, CAP_POINT + 77])
def test_cast_f32_rounds_as_torch(dt, count):
    """fp32 -> 16-bit equals x.to(dt) bit for bit (round to nearest, ties to even, overflow to inf, gradual underflow, -0), NaN
    where and only where the input is NaN.  Counts off the block size, and one past the launch cap (wrap)."""
    h = hip()
    table = _cast_table(dt)
    x = torch.cat([table, randn((count - table.numel(),), count, 100.0)]) if count > table.numel() else table[:count]
    oh = sentinel(1, count + 5, dt)[0]
    od = oh.to(DEV)
    h.cast_f32(x.to(DEV), od[:count])
    got, ref = od.cpu(), x.to(dt)
    nan = torch.isnan(x)
    assert torch.equal(torch.isnan(got[:count]), nan), "NaN exactly where the input is NaN"
    assert same_bits(torch.where(nan, torch.zeros_like(ref), got[:count]), torch.where(nan, torch.zeros_like(ref), ref)), \
        f"first difference at {int(((got[:count] != ref) & ~nan).int().argmax())}"
    assert same_bits(got[count:], oh[count:])


@pytest.mark.parametrize("R,hh,ww", [(5, 64, 64), (5, 32, 32), (5, 16, 16), (7, 5, 7), (3, 9, 2), (8192, 64, 64)])
def test_avgpool2_f32(R, hh, ww):
    """The correlation pyramid's 2 x 2 mean equals ((a + b) + c + d) * 0.25 in fp32 on the CPU in the kernel's order: three
    correctly rounded adds and an exact scale, so equality is derived.  Odd sizes drop the last row / column.  Wrap: R = 8192
    maps of 64 x 64 = 8.4 M outputs (cap 4.19 M)."""
    h = hip()
    x = randn((R, hh, ww), R + hh, 4.0)
    oh_, ow_ = hh // 2, ww // 2
    oh = sentinel(1, R * oh_ * ow_ + 3, torch.float32)[0]
    od = oh.to(DEV)
    h.avgpool2_f32(x.to(DEV), od, R=R, h=hh, w=ww)
    ref = avgpool2_ref(x)
    got = od.cpu()
    assert same_bits(got[:ref.numel()].reshape(ref.shape), ref.contiguous())
    assert same_bits(got[ref.numel():], oh[ref.numel():])


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("M,ncopies,with_delta", [(1000, 1, True), (1000, 2, True), (1000, 3, True), (1000, 1, False), (333, 3, False),
                                                  (CAP_RAFT + 5, 1, True)])
def test_flow_update(dt, M, ncopies, with_delta):
    """flow32 += delta32[:, :2] (ldd = 8) equals the fp32 sum on the CPU; the 16-bit copies equal its rounding, written into
    columns 382..383 of a 384-wide buffer (the GRU input), 0..1 of an 8-wide one (the flow convolution's input) and 256..257;
    every other column keeps its sentinel.  `delta32 = None` only copies.  The last case wraps (one token per item)."""
    h = hip()
    flow = randn((M, 2), M, 5.0)
    delta = randn((M, 8), M + 1, 0.7)
    fd = flow.to(DEV)
    wrap = M > CAP_RAFT
    slots = [(sentinel(M, 8, dt), 0)] if wrap else [(sentinel(M, 384, dt), 382), (sentinel(M, 8, dt), 0), (sentinel(M, 384, dt), 256)][:ncopies]
    bufs = [s.to(DEV) for s, _ in slots]
    h.flow_update(fd, delta.to(DEV) if with_delta else None, [(b[:, c:], b.stride(0)) for b, (_, c) in zip(bufs, slots)], dtype=dt)
    ref = flow_update_ref(flow, delta if with_delta else None)
    assert same_bits(fd.cpu(), ref)
    for b, (host, c) in zip(bufs, slots):
        keep = host.clone()
        keep[:, c:c + 2] = ref.to(dt)
        assert same_bits(b.cpu(), keep), f"copy at column {c}"


# ====================================================================================== InstanceNorm statistics and apply
STAT_R = (0.0, 3.0, 16.0, 64.0)
STAT_CASES = [(hw, C, nimg) for hw in (1, 31, 192, 2047, 2048, 2049, 3072, 16383, 16384, 16385, 65536) for C in (8, 64, 96, 200)
              for nimg in (1, 3) if hw * C * nimg <= 65536 * 200]        # (the largest: the 512 x 512 stem's hw at 200 channels)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("hw,C,nimg", STAT_CASES)
def test_channel_stats_and_norm(dt, hw, C, nimg):
    """nn.InstanceNorm2d's (mean, 1 / sqrt(var + 1e-5)) per image and channel, then the normalised output from those statistics.
    Channel 0 is constant, channel 1 all zeros, channel c >= 2 is N(m, 1) with r = |m| / std = (0, 3, 16, 64)[c % 4], rounded
    to the 16-bit type; the input is a column view (ldx = C + 16).  hw crosses the 1 / 4 / 16 slice thresholds, slices whose
    last part is shorter (2049, 16385), and reaches the 512 x 512 stem (65536).

    Bounds: kernel_bounds.channel_stats_ref_and_bound (moments about the pivot) and channel_norm_ref_and_bound.  A constant channel
    has d = 0 exactly: mean exact, var = 0, rstd = fp32(1 / sqrt(eps)), normalised output exactly 0."""
    h = hip()
    eps = float(torch.tensor(1e-5, dtype=torch.float32))          # the fp32 number the kernel is handed
    g = torch.Generator().manual_seed(hw * 1000 + C * 3 + nimg)
    x = torch.randn(nimg, hw, C, generator=g)
    rs = torch.tensor([STAT_R[c % 4] * (-1.0 if c % 8 >= 4 else 1.0) for c in range(C)])
    x = x + rs
    x[:, :, 0] = 3.25
    x[:, :, 1] = 0.0
    xh = sentinel(nimg * hw, C + 16, dt)
    xh[:, 8:8 + C] = x.reshape(nimg * hw, C).to(dt)
    x64 = xh[:, 8:8 + C].double().reshape(nimg, hw, C)
    st_ref, st_bound = channel_stats_ref_and_bound(x64, eps)
    mean, rstd, d_mean, d_rstd = st_ref[..., 0], st_ref[..., 1], st_bound[..., 0], st_bound[..., 1]

    xd = xh.to(DEV)
    stats = h.channel_stats(xd[:, 8:], nimg=nimg, hw=hw, C_=C, ldx=C + 16, eps=eps)
    again = h.channel_stats(xd[:, 8:], nimg=nimg, hw=hw, C_=C, ldx=C + 16, eps=eps)
    assert torch.equal(stats, again), "the statistics must not depend on the launch"
    st = stats.cpu().double()
    groups = [(r, [c for c in range(2, C) if c % 4 == k]) for k, r in enumerate(STAT_R)]
    rel = (st[..., 1] - rstd).abs() / rstd                   # (printed before anything is asserted, so a failing run shows it too)
    print(f"\nchannel_stats {dt} hw={hw} C={C} nimg={nimg}: rstd rel err (bound) " +
          "; ".join(f"r={r:g}: {float(rel[:, ch].max()):.2e} ({float((d_rstd / rstd)[:, ch].max()):.2e})" for r, ch in groups))
    assert_within(st[..., 0], mean, d_mean, f"mean hw={hw} C={C}")
    assert_within(st[..., 1], rstd, d_rstd, f"rstd hw={hw} C={C}")
    assert torch.equal(st[:, :2, 0], x64[:, 0, :2]), "the mean of a constant channel is exact"
    assert torch.equal(st[:, :2, 1].float(), torch.full((nimg, 2), 1.0 / math.sqrt(eps), dtype=torch.float64).float()), "var = 0"

    yh = sentinel(nimg * hw, C + 16, dt)
    yd = yh.to(DEV)
    h.channel_norm_act(xd[:, 8:], yd[:, 8:], M=nimg * hw, hw=hw, C_=C, act=h.ACT_NONE, stats=stats, ldx=C + 16, ldy=C + 16)
    got = yd.cpu()
    ref, bound = channel_norm_ref_and_bound(x64, st_ref, st_bound, dt)
    e_out = assert_within(got[:, 8:8 + C].reshape(nimg, hw, C), ref, bound, f"normalised output hw={hw} C={C}")
    assert bool((got[:, 8:10] == 0).all()), "a constant channel normalises to exactly 0"
    assert same_bits(got[:, :8], yh[:, :8]) and same_bits(got[:, 8 + C:], yh[:, 8 + C:]), "columns outside the slot must not change"
    print("  normalised output, worst err / bound: " + "; ".join(f"r={r:g}: {float((e_out / bound)[:, :, ch].max()):.2f}" for r, ch in groups))


ACTS = ["none", "relu", "tanh", "sigmoid"]
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("act", ACTS)
def test_channel_norm_act_forms(dt, act):
    """y = act((x - mean) rstd + residual) in every form the engine uses and the header allows: statistics or not x residual or
    not x outputs {16-bit, fp32, both} x {out of place, in place, y == residual} x {contiguous, x a column view with ldx = 256
    and y columns 128..255 of a 384-wide buffer}.  Statistics are given fp32 numbers (the reference reads those exact values).
    Inputs hold +-30 and +-the largest finite value of the type (/ 8 for the unbounded activations with statistics or a
    residual, where the result would leave the type's range): results are finite and inside the activation's range.
    Bound: kernel_bounds.norm_act_pre_ref_and_bound, act_ref_and_bound."""
    h = hip()
    nimg, hw, C = 3, 37, 128
    M = nimg * hw
    code = {"none": h.ACT_NONE, "relu": h.ACT_RELU, "tanh": h.ACT_TANH, "sigmoid": h.ACT_SIGMOID}[act]
    stats32 = torch.stack([randn((nimg, C), 1, 2.0), randn((nimg, C), 2).abs() + 0.25], -1).contiguous()
    ran = 0
    for layout in ("contiguous", "views"):
        for place in ("out", "inplace", "y_is_res"):
            for outs in ("16", "32", "both"):
                for with_stats in (False, True):
                    for with_res in (False, True):
                        if (place != "out" and outs == "32") or (place == "y_is_res" and not with_res):
                            continue
                        big = fmax(dt) / (8.0 if act in ("none", "relu") and (with_stats or with_res) else 1.0)
                        X = rnd((M, C), 3 + ran, dt, 2.0)
                        X[0, :8] = torch.tensor([30.0, -30.0, big, -big, 0.0, -0.0, 88.0, -88.0]).to(dt)
                        X[M - 1, C - 4:] = torch.tensor([30.0, -30.0, big, -big]).to(dt)
                        R = rnd((M, C), 1000 + ran, dt)
                        ldx, ldy, col = (C, C, 0) if layout == "contiguous" else (256, 384, 128)
                        yh = sentinel(M + 1, ldy, dt)
                        xh = sentinel(M, ldx, dt)
                        xh[:, col:col + C] = X
                        if place == "inplace":
                            yh[:M, col:col + C] = X
                        if place == "y_is_res":
                            yh[:M, col:col + C] = R
                        yd, xd, rd = yh.to(DEV), xh.to(DEV), R.to(DEV)
                        y32h = sentinel(M, C + 8, torch.float32)
                        y32d = y32h.to(DEV)
                        yv = yd[:M, col:]
                        xv = yv if place == "inplace" else xd[:, col:]
                        res = None if not with_res else (yv if place == "y_is_res" else rd)
                        h.channel_norm_act(xv, yv if outs != "32" else None, M=M, hw=hw, C_=C, act=code,
                                           stats=stats32.to(DEV) if with_stats else None, residual=res,
                                           y32=y32d if outs != "16" else None, ldx=ldy if place == "inplace" else ldx, ldy=ldy,
                                           ldr=(ldy if place == "y_is_res" else C) if with_res else None)
                        what = f"{act} {layout} {place} outs={outs} stats={with_stats} res={with_res}"
                        v, dv = norm_act_pre_ref_and_bound(X.double(), stats32.double() if with_stats else None, R.double() if with_res else None, hw)
                        lo, hi = {"none": (-math.inf, math.inf), "relu": (0.0, math.inf), "tanh": (-1.0, 1.0), "sigmoid": (0.0, 1.0)}[act]
                        if outs != "32":
                            got = yd.cpu()
                            ref, b = act_ref_and_bound(v, dv, act, dt)
                            assert_within(got[:M, col:col + C], ref, b, what + " y")
                            assert float(got[:M, col:col + C].float().min()) >= lo and float(got[:M, col:col + C].float().max()) <= hi, what
                            keep = yh.clone()
                            keep[:M, col:col + C] = got[:M, col:col + C]
                            assert same_bits(got, keep), what + ": a store outside y's slot"
                        else:
                            assert same_bits(yd.cpu(), yh), what + ": y = None must leave the buffer alone"
                        if outs != "16":
                            got32 = y32d.cpu()
                            ref, b = act_ref_and_bound(v, dv, act, torch.float32)
                            assert_within(got32[:, :C], ref, b, what + " y32")
                            assert float(got32[:, :C].min()) >= lo and float(got32[:, :C].max()) <= hi, what
                            assert same_bits(got32[:, C:], y32h[:, C:]), what + ": a store outside y32's slot"
                        else:
                            assert same_bits(y32d.cpu(), y32h)
                        assert same_bits(xd.cpu(), xh) and same_bits(rd.cpu(), R), what + ": inputs must not change"
                        ran += 1
    assert ran == 2 * (3 * 2 * 2 + 2 * 2 * 2 + 2 * 2 * 1)


@pytest.mark.parametrize("dt", DTYPES)
def test_channel_norm_act_wrap(dt):
    """Wrap: the stem's InstanceNorm + ReLU of 9 images of 256 x 256 tokens, C = 64: 4.72 M items (cap 4.19 M), in place,
    with the kernel's own statistics, which the reference reads as given fp32 numbers (they are bounded against fp64 in
    test_channel_stats_and_norm at this hw).  Bound: kernel_bounds.norm_act_pre_ref_and_bound, act_ref_and_bound."""
    h = hip()
    nimg, hw, C = 9, 65536, 64
    assert nimg * hw * (C // 8) > CAP_RAFT
    xh = (torch.randn(nimg * hw, C, generator=torch.Generator().manual_seed(3)) + torch.linspace(-3, 3, C)).to(dt)
    x64 = xh.double().reshape(nimg, hw, C)
    xd = xh.to(DEV)
    stats = h.channel_stats(xd, nimg=nimg, hw=hw, C_=C)
    h.channel_norm_act(xd, xd, M=nimg * hw, hw=hw, C_=C, act=h.ACT_RELU, stats=stats)
    st = stats.cpu().double()
    m, s = st[:, None, :, 0], st[:, None, :, 1]
    v = (x64 - m) * s
    ref, b = act_ref_and_bound(v, 2 * U32 * v.abs(), "relu", dt)
    assert_within(xd.cpu().reshape(nimg, hw, C), ref, b, "wrap")


# ====================================================================================== ConvGRU
SAT = [30.0, -30.0, 88.0, -88.0, 100.0, -100.0, 0.0, -0.0]


def _gru_gate_case(h, dt, zr, h32, M, Hd):
    """Run gru_gate as the engine does (z contiguous-ish with 8 sentinel columns, rh = columns 0..Hd-1 of a 384-wide buffer) and
    return (z, rh) on the host after the sentinel checks."""
    zh, rhh = sentinel(M + 1, Hd + 8, dt), sentinel(M + 1, 384, dt)
    zd, rhd = zh.to(DEV), rhh.to(DEV)
    h.gru_gate(zr, h32, zd, rhd, M=M, hidden=Hd, ldrh=384)
    z, rh = zd.cpu(), rhd.cpu()
    assert same_bits(z[:, Hd:], zh[:, Hd:]) and same_bits(z[M:], zh[M:]), "z: a store outside the slot"
    assert same_bits(rh[:, Hd:], rhh[:, Hd:]) and same_bits(rh[M:], rhh[M:]), "r h: a store outside columns 0..hidden-1"
    return z[:M, :Hd].contiguous(), rh[:M, :Hd].contiguous()


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("M,Hd", [(300, 128), (37, 96), (9 * 4096 + 3, 128)])
def test_gru_gate(dt, M, Hd):
    """z = sigmoid(zr[:, :Hd]) and sigmoid(zr[:, Hd:]) * h32 (the header's formulas) in fp64, with saturated pre-activations
    (+-30, +-88, +-100, +-the largest finite value).  Bound: z: the sigmoid allowance E z + 2^-126 + 0.5 ulp; r h: (E + u) |r h|
    + 2^-126 (1 + |h|) + 0.5 ulp (one product; a flushed sigmoid is multiplied by h).  The last case wraps: 4.72 M items (cap 4.19 M)."""
    h = hip()
    zr = rnd((M, 2 * Hd), M + Hd, dt, 3.0)
    zr[0, :8] = torch.tensor(SAT).to(dt)
    zr[0, Hd:Hd + 8] = torch.tensor(SAT).to(dt)
    zr[M - 1, Hd - 2:Hd + 2] = torch.tensor([fmax(dt), -fmax(dt), fmax(dt), -fmax(dt)]).to(dt)
    h32 = randn((M, Hd), M, 1.0)
    z, rh = _gru_gate_case(h, dt, zr.to(DEV), h32.to(DEV), M, Hd)
    zref, zb, rref, rb = gru_gate_ref_and_bound(zr, h32, dt)
    assert_within(z, zref, zb, "z")
    assert_within(rh, rref, rb, "r h")
    assert float(z.float().min()) >= 0.0 and float(z.float().max()) <= 1.0


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("M,Hd,with_b", [(300, 128, True), (300, 128, False), (37, 96, True), (9 * 4096 + 3, 128, False)])
def test_gru_update(dt, M, Hd, with_b):
    """The fp32 master state against fp64 within gru_update_ref_and_bound; the 16-bit copies are the roundings of the stored state, bit
    for bit, h16a into columns 0..Hd-1 of a 384-wide buffer (the next step's hx), h16b given or None.  The last case wraps."""
    h = hip()
    q = rnd((M, Hd), M + 1, dt, 3.0)
    q[0, :8] = torch.tensor(SAT).to(dt)
    q[M - 1, -2:] = torch.tensor([fmax(dt), -fmax(dt)]).to(dt)
    z = torch.rand(M, Hd, generator=torch.Generator().manual_seed(M)).to(dt)
    z[0, :4] = torch.tensor([0.0, 1.0, 1.0, 0.0]).to(dt)
    h32 = randn((M, Hd), M + 2)
    hd = h32.to(DEV)
    ah, bh = sentinel(M + 1, 384, dt), sentinel(M + 1, Hd + 8, dt)
    ad, bd = ah.to(DEV), bh.to(DEV)
    h.gru_update(q.to(DEV), z.to(DEV), hd, ad, 384, bd if with_b else None, Hd + 8, M=M, hidden=Hd)
    ref, bound = gru_update_ref_and_bound(q, z, h32.double(), dt)
    got = hd.cpu()
    assert_within(got, ref, bound, "h32")
    for name, buf, host, used in (("h16a", ad, ah, True), ("h16b", bd, bh, with_b)):
        keep = host.clone()
        if used:
            keep[:M, :Hd] = got.to(dt)
        assert same_bits(buf.cpu(), keep), name


@pytest.mark.parametrize("dt", DTYPES)
def test_gru_twenty_steps_carry_the_state(dt):
    """20 alternating gate / update steps with fresh random zr and q, the fp32 state carried on the GPU, against the fp64
    recurrence carried on the CPU.  The reference reads the 16-bit z the kernel stored (as the update kernel does in the engine),
    so the state's bound obeys e' <= (1 - z) e + the step's own bound (gru_update_ref_and_bound); r h is bounded with the state's e:
    (E + u) |r h| + r e + 2^-126 (1 + |h|) + 0.5 ulp."""
    h = hip()
    M, Hd = 200, 128
    h32 = randn((M, Hd), 77)
    href, e = h32.double(), torch.zeros(M, Hd, dtype=torch.float64)
    hd = h32.to(DEV)
    hx = sentinel(M, 384, dt).to(DEV)
    for step in range(20):
        zr, q = rnd((M, 2 * Hd), 100 + step, dt, 2.0), rnd((M, Hd), 200 + step, dt, 2.0)
        z, rh = _gru_gate_case(h, dt, zr.to(DEV), hd, M, Hd)
        zref, zb, rref, rb = gru_gate_ref_and_bound(zr, href, dt, h_err=e)
        assert_within(z, zref, zb, f"step {step} z")
        assert_within(rh, rref, rb, f"step {step} r h")
        h.gru_update(q.to(DEV), z.to(DEV), hd, hx, 384, None, 0, M=M, hidden=Hd)
        href_new, b = gru_update_ref_and_bound(q, z, href, dt)
        e = (1 - z.double()) * e + b
        href = href_new
        assert_within(hd.cpu(), href, e, f"step {step} h32")
    assert same_bits(hx.cpu()[:, :Hd], hd.cpu().to(dt)) and same_bits(hx.cpu()[:, Hd:], sentinel(M, 384, dt)[:, Hd:])
    print(f"\ngru 20 steps {dt}: max |h - ref| {float((hd.cpu().double() - href).abs().max()):.2e}, bound there {float(e.max()):.2e}")


# ====================================================================================== correlation lookup
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("levels,B,hh,ww", [(2, 2, 16, 24), (4, 2, 16, 24), (2, 1, 64, 64), (4, 4, 64, 64)])
def test_corr_lookup(dt, levels, B, hh, ww):
    """Flows are multiples of 1/64, so x + flow, its division by 2^l and the window offsets are exact in fp32 and the reference's
    sample points are the kernel's.  The first tokens are steered so that (x + fx) and (y + fy) land on -8, -5, -4, -1, -1/2, 0,
    3 1/4, w - 5, w - 4, w - 1, w - 1/2, w, w + 3, w + 4, w + 8: with the nine offsets every level meets integers, exactly -1,
    w_l - 1 and w_l, and points inside the half-open border cells (-1, 0) and (w_l - 1, w_l).  A few tokens sit at +-1e6 and
    must read exactly 0; the rest are N(0, 3).  The output is `levels` x 81 columns of a 328-wide sentinel buffer.
    Bound: each of the four terms passes two products and two sums, and the scale one more: 5 u S with S = scale sum_k w_k |v_k|,
    plus 0.5 ulp of the type.  The last case is the wrap: 16384 tokens x 324 = 5.3 M items (cap 4.19 M)."""
    h = hip()
    M = B * hh * ww
    assert (M * levels * 81 > CAP_RAFT) == (B == 4)
    vols = [randn((M, hh >> l, ww >> l), 10 * levels + l + hh, 4.0) for l in range(levels)]
    flow = torch.round(randn((M, 2), M, 3.0) * 64) / 64
    m = torch.arange(M)
    px, py = (m % ww).float(), ((m // ww) % hh).float()
    tx = torch.tensor([-8, -5, -4, -1, -0.5, 0, 3.25, ww - 5, ww - 4, ww - 1, ww - 0.5, ww, ww + 3, ww + 4, ww + 8])
    ty = torch.tensor([-8, -5, -4, -1, -0.5, 0, 3.25, hh - 5, hh - 4, hh - 1, hh - 0.5, hh, hh + 3, hh + 4, hh + 8])
    n = 15 * 16
    k = torch.arange(n)
    flow[:n, 0] = tx[k % 15] - px[:n]
    flow[:n, 1] = ty[(k // 15 + k) % 15] - py[:n]
    flow[n:n + 4] = torch.tensor([[1e6, 0.0], [0.0, -1e6], [-1e6, 1e6], [1e6, 1e6]])
    scale = 1.0 / 16.0
    oh = sentinel(M + 1, 328, dt)
    od = oh.to(DEV)
    h.corr_lookup([v.to(DEV) for v in vols], flow.to(DEV), od[:M], h=hh, w=ww, scale=scale)
    got = od.cpu()
    ref, bound = corr_lookup_ref_and_bound(vols, flow, B, hh, ww, scale, dt)
    K = levels * 81
    assert_within(got[:M, :K], ref, bound, f"lookup levels={levels} {hh}x{ww}")
    assert bool((got[n:n + 4, :K] == 0).all()), "windows a million cells away read exactly 0"
    assert int((ref[:n] != 0).sum()) > n * K // 20 and int((ref[:n] == 0).sum()) > n * K // 20, "the steered tokens straddle the border"
    assert same_bits(got[:, K:], oh[:, K:]) and same_bits(got[M:], oh[M:]), "columns past levels x 81 must not change"


# ====================================================================================== convex upsampling
@pytest.mark.parametrize("B,hh,ww", [(2, 8, 10), (1, 1, 1), (17, 64, 64)])
def test_convex_upsample(B, hh, ww):
    """out[b, :, 8 y + fy, 8 x + fx] = sum_k softmax_k(mult mask[m, k, fy, fx]) 8 flow[neighbour k of m] in fp64 (F.unfold's zero
    padding: a neighbour outside the map adds 0 to the sum and its weight stays in the softmax).  Logits reach +-320 before
    mult = 0.25 (+-80 after: exp must not overflow); ldm = 584 > 576.
    Bound.  Weight k carries a relative error eps_k = E + 3 u |d_k|, d_k = its logit minus the row's largest (E: the softmax
    allowance of the module docstring, measured on these logits; the subtraction and the scaling by log2 e inside __expf round
    in proportion to |d_k|).  Numerator and denominator are 9 sums each, every term one product, then one division:
    sum_k w_k (eps_k + 10 u) |8 f_k| + |out| (sum_k w_k eps_k + 10 u), and 2^-126 (sum_k |8 f_k| + 1): an exponential below the
    normal range may be flushed, and it is multiplied by 8 f_k.  The last case wraps: 4.46 M items (cap 4.19 M)."""
    h = hip()
    M = B * hh * ww
    assert (M * 64 > CAP_RAFT) == (B == 17)
    g = torch.Generator().manual_seed(M)
    spread = torch.tensor([1.0, 8.0, 40.0, 100.0])[torch.randint(0, 4, (M, 1), generator=g)]
    mask = (torch.randn(M, 584, generator=g) * spread).clamp(-320, 320)
    mask[0, :576:64] = torch.tensor([320.0, -320.0, 320.0, 0.0, -320.0, 319.0, 1.0, -1.0, 300.0])[:9]
    mask[M - 1, 5:576:64] = -320.0
    flow = randn((M, 2), M + 1, 3.0)
    out = h.convex_upsample(mask.to(DEV), flow.to(DEV), B=B, h=hh, w=ww, mult=0.25).cpu()
    ref, bound = convex_upsample_ref_and_bound(mask, flow, B, hh, ww, 0.25)
    assert_within(out, ref, bound, f"convex upsample {B}x{hh}x{ww}")


# ====================================================================================== softmax over rows
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("M", [1, 7])
@pytest.mark.parametrize("N", [4, 1020, 1024, 1028, 4096, 16380, 16384])
def test_softmax_rows(dt, M, N):
    """P = softmax(S scale) over N columns, fp32 in, 16-bit out, ld_s = N + 4 and ld_p = N + 4 (4 sentinel columns).  Row 0 has one
    logit 100 above the rest after scaling (p = 1 there, the others below half the smallest subnormal: exactly 0), row 1 is
    constant (p = 1 / N), the rest are N(0, 3) / scale.  N crosses the 1024-column register steps and reaches the limit 16384.
    Bound, relative to p: the exponent of 2 is fma(s, c, -max c) with c = fl(scale log2 e): c is off by 2 u relative and each
    of the two terms rounds once, so the argument is off by 4 u A, A = max|s| scale log2 e, for numerator and denominator alike:
    8 ln2 u A; the row sum is 16 + 8 + 3 fp32 sums, the reciprocal and the product 2 more; the exp2 allowance E of the module
    docstring (torch's fp32 softmax on these rows).  Then 0.5 ulp of the type, and 2^-126 for a flushed intermediate.  The
    row sums differ from the reference's by at most the sum of the bounds, i.e. N x 0.5 ulp plus the fp32 terms."""
    h = hip()
    scale = 0.125
    S = randn((M, N + 4), 31 * N + M, 3.0 / scale)
    S[0, :N] = randn((N,), N, 1.0 / scale)
    S[0, N // 3] = S[0, :N].max() + 100.0 / scale
    if M > 1:
        S[1, :N] = 2.5
    oh = sentinel(M + 1, N + 4, dt)
    od = oh.to(DEV)
    h.softmax_rows(S.to(DEV), od, M=M, N=N, scale=scale, ld_s=N + 4, ld_p=N + 4)
    got = od.cpu()
    ref, bound = softmax_rows_ref_and_bound(S[:, :N], scale, dt)      # (S scale is exact: a power of two)
    assert_within(got[:M, :N], ref, bound, f"softmax N={N}")
    assert float(got[0, N // 3]) == 1.0 and int((got[0, :N] != 0).sum()) == 1, "one dominant logit takes all the mass"
    sums = got[:M, :N].double().sum(1)
    assert bool(((sums - ref.sum(1)).abs() <= bound.sum(1)).all()), sums
    assert same_bits(got[:, N:], oh[:, N:]) and same_bits(got[M:], oh[M:]), "columns past N must not change"


def test_softmax_rows_refusals():
    h = hip()
    S = torch.zeros(2, 16400, dtype=torch.float32, device=DEV)
    P = torch.zeros(2, 16400, dtype=torch.float16, device=DEV)
    h.softmax_rows(S, P, M=2, N=16384, scale=1.0)
    with pytest.raises(h.VFaceHipError):
        h.softmax_rows(S, P, M=2, N=6, scale=1.0)               # N % 4
    with pytest.raises(h.VFaceHipError):
        h.softmax_rows(S, P, M=2, N=16388, scale=1.0)           # past the 16 float4 per thread the row is held in


# ====================================================================================== VAE latent sample, SiLU
@pytest.mark.parametrize("Fn,zc,hw,ldm", [(3, 4, 11 * 13, 16), (1, 4, 1, 8), (9, 4, 65536, 8)])
@pytest.mark.parametrize("mode", [True, False])
def test_vae_sample(Fn, zc, hw, ldm, mode):
    """z = (mean + exp(0.5 clamp(logvar, -30, 20)) noise) scale from fp32 moments [F hw, ldm >= 2 zc] into NCHW fp32; `noise =
    None` gives the mode, mean x scale.  Log-variances include -40, -30, 20, 25 (both sides of each clamp edge).
    Bound: mode: one product, u |z|.  Sample: 0.5 lv is exact; exp carries the allowance E (torch's fp32 exp on the clamped
    halves); its product with the noise, the sum and the scaling round once each: (E + 3 u) |std noise scale| + 2 u |z|.
    The last case wraps: 9 x 4 x 65536 = 2.36 M items (cap 2.10 M)."""
    h = hip()
    scale = 0.18215
    s32 = float(torch.tensor(scale, dtype=torch.float32))
    assert (Fn * zc * hw > CAP_POINT) == (Fn == 9)
    mom = randn((Fn * hw, ldm), Fn + hw, 3.0)
    edge = torch.tensor([-40.0, -30.0, 20.0, 25.0, -30.000002, -29.999998, 19.999998, 20.000002])
    mom[0, zc:2 * zc] = edge[:zc]
    mom[-1, zc:2 * zc] = edge[4:4 + zc]
    if hw > 1:
        mom[1, zc:2 * zc] = edge[:zc].flip(0)
    noise = randn((Fn, zc, hw), 5)
    zh = sentinel(1, Fn * zc * hw + 5, torch.float32)[0]
    zd = zh.to(DEV)
    h.vae_sample(mom.to(DEV), None if mode else noise.to(DEV), zd, F=Fn, hw=hw, zc=zc, scale=scale)
    got = zd.cpu()
    mm = mom.reshape(Fn, hw, ldm).permute(0, 2, 1).double()
    mean, lv = mm[:, :zc], mm[:, zc:2 * zc].clamp(-30.0, 20.0)
    if mode:
        ref = mean * s32
        bound = U32 * ref.abs()
    else:
        E = cpu_fp32_rel_error(torch.exp, (0.5 * lv).float())
        dev = torch.exp(0.5 * lv) * noise.double() * s32
        ref = mean * s32 + dev
        bound = (E + 3 * U32) * dev.abs() + 2 * U32 * ref.abs() + TINY32
    n = Fn * zc * hw
    assert_within(got[:n].reshape(Fn, zc, hw), ref, bound, f"vae_sample mode={mode}")
    assert same_bits(got[n:], zh[n:])


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("in_f32", [True, False])
@pytest.mark.parametrize("count", [1000, CAP_POINT + 13])
def test_silu(dt, in_f32, count):
    """x sigmoid(x) from fp32 or 16-bit input to the 16-bit type, in place for the 16-bit input (as the engine's time embedding
    does), at +-20, +-88 and +-the largest finite value of the type.  x / (1 + __expf(-x)): the exponential's argument scaling
    rounds in proportion to |x| (2 u |x| relative, weighted by e / (1 + e) <= 1), the sum and the division once each, and the
    sigmoid allowance E of the module docstring: (E + (2 |x| + 2) u) |ref| + 2^-126 + 0.5 ulp.  The second count wraps."""
    h = hip()
    x = randn((count,), count, 4.0)
    x[:8] = torch.tensor([20.0, -20.0, 88.0, -88.0, fmax(dt), -fmax(dt), 0.0, -0.0])
    x = x if in_f32 else x.to(dt)
    oh = sentinel(1, count + 3, dt)[0]
    if in_f32:
        od = oh.to(DEV)
        h.silu(x.to(DEV), od[:count])
    else:
        oh[:count] = x
        od = oh.to(DEV)
        h.silu(od[:count], od[:count])
    got = od.cpu()
    x64 = x.double()
    ref = x64 * torch.sigmoid(x64)
    E = cpu_fp32_rel_error(torch.sigmoid, x.float())
    bound = (E + (2 * x64.abs() + 2) * U32) * ref.abs() + TINY32 + 0.5 * ulp(ref, dt)
    keep = torch.isfinite(ref) & (ref.abs() <= fmax(dt))
    assert bool(keep.all())
    assert_within(got[:count], ref, bound, f"silu in_f32={in_f32}")
    assert same_bits(got[count:], oh[count:])
