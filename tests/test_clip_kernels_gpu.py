"""The conditioning kernels per element against fp64 on the MI355X, fp16 and bf16: ``vface_attention`` at head dimension 64 (the
CLIP image tower: 257 = 4 * 64 + 1 tokens, the last key block one key and the last query tile one query) within
``kernel_bounds.attention_ref_and_bound``, and ``vface_clip_patches`` / ``vface_clip_embed`` / ``vface_act`` / ``vface_cond_mix``
(csrc/clip.hip) within the bounds of clip_bounds.py -- built from fp64 quantities of the reference alone; test_clip_bound_cpu.py shows
that they admit torch's fp32 evaluation and refuse one-line defects.  Outputs are views inside sentinel buffers whose frame is
checked bit for bit (``kernel_bounds.Framed``); data movement (patch order, the zero pad, the gather's source rows and columns) is
checked bit for bit."""
import pytest
import torch

import clip_bounds as cb
from attention_model import KVB, base2_gap_to_median, late_key_excess, make_inputs
from kernel_bounds import Framed, assert_within, attention_ref_and_bound, note, rnd, same_bits, sentinel, strided

pytestmark = pytest.mark.gpu

DEV = "cuda"
DTS = [torch.float16, torch.bfloat16]
ERR_SHAPE = -3


def hip():
    from vface_amd import hip as h
    h.load()
    return h


# ------------------------------------------------------------------------------------------------ attention at dh = 64
def _packed_attention(h, qkv, *, B, n, heads, dh, scale, variant=0):
    """``qkv [B, n, 3 d]`` on the CPU -> the kernel's ``[B, n, d]``: q | k | v are the three strided thirds of ONE packed
    ``[B n][3 d + 24]`` buffer (what the engine passes) whose 24 tail columns are NaN; the output lies 4 elements into a sentinel
    buffer with row stride d + 12 and two gap rows per sample, and every element outside it keeps its bits."""
    dt, d = qkv.dtype, heads * dh
    ld = 3 * d + 24
    buf = torch.full((B * n, ld), float("nan"), dtype=dt)
    buf[:, :3 * d] = qkv.reshape(B * n, 3 * d)
    dev = buf.to(DEV)
    ldo, bso, oo = d + 12, (n + 2) * (d + 12), 4
    keep = sentinel(1, oo + B * bso + ldo, dt).flatten()
    od = keep.to(DEV)
    flat = dev.view(-1)
    h.attention(flat, flat[d:], flat[2 * d:], od[oo:], B=B, heads=heads, n=n, nk=n, dh=dh, ldq=ld, ldk=ld, ldv=ld, bsq=n * ld, bsk=n * ld,
                bsv=n * ld, ldo=ldo, bso=bso, scale=scale, variant=variant)
    torch.cuda.synchronize()
    got_all = od.cpu()
    view = lambda t: t[oo:oo + B * bso].as_strided((B, n, d), (bso, ldo, 1))
    got = view(got_all).clone()
    expect = keep.clone()
    view(expect).copy_(got)
    assert same_bits(got_all, expect), "a store outside the output view"
    assert same_bits(dev.cpu(), buf), "the packed input changed"
    return got


def _check_attention(got, qkv, *, heads, dh, scale, pairs, what):
    d = heads * dh
    assert bool(torch.isfinite(got.float()).all()), f"{what}: non-finite output"
    worst = 0.0
    for b, hd in pairs:
        c = slice(hd * dh, (hd + 1) * dh)
        o, bound = attention_ref_and_bound(qkv[b, :, :d][:, c], qkv[b, :, d:2 * d][:, c], qkv[b, :, 2 * d:][:, c], scale, got.dtype)
        err = assert_within(got[b, :, c], o, bound, f"{what} sample {b} head {hd}")
        worst = max(worst, float((err / bound).max()))
    print(f"{what}: worst err / bound {worst:.3f}")


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("heads", [2, 16])
@pytest.mark.parametrize("n", [5, 10, 65, 257])
def test_attention_dh64_on_the_thirds_of_a_packed_buffer(dt, heads, n):
    """n = nk: 5 and 10 (the `tiny` configuration), 65 = one key block and one key, 257 = the ViT-L/14 sequence; every (sample,
    head) at 2 heads, every head of both samples at 16."""
    h = hip()
    B, dh = 2, 64
    qkv = rnd((B, n, 3 * heads * dh), 640 + n + heads, dt)
    got = _packed_attention(h, qkv, B=B, n=n, heads=heads, dh=dh, scale=dh ** -0.5)
    _check_attention(got, qkv, heads=heads, dh=dh, scale=dh ** -0.5, pairs=[(b, hd) for b in range(B) for hd in range(heads)],
                     what=f"dh64 {dt} heads={heads} n={n}")


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("variant", [0, 2])
@pytest.mark.parametrize("family", ["peaked", "late_spike", "dominant", "over_soft", "over_hard"])
def test_attention_dh64_softmax_stress_at_257(dt, family, variant):
    """The softmax-stress families of test_attention_gpu.py at n = nk = 257, dh = 64 (variant 0 default, 2 exact scale): rows whose
    maximum keeps rising, a dominating key near the end, fp16 probabilities in the subnormal range, and a late key that makes the
    speculative pass's fp16 P reach 2^15 (finite) or overflow (the tile runs again with the checked loop).  With 257 keys the late
    key (index 255) sits in the last FULL block and the one key behind it is alone in its block."""
    h = hip()
    B, heads, dh, n = 2, 2, 64, 257
    scale = dh ** -0.5
    parts = [[make_inputs(family, dt, n, n, dh, scale, seed=7 * b + hd) for hd in range(heads)] for b in range(B)]
    q, k, v = (torch.stack([torch.cat([parts[b][hd][i] for hd in range(heads)], dim=1) for b in range(B)]) for i in range(3))
    for b in range(B):
        for hd in range(heads):
            qq, kk, _ = parts[b][hd]
            if family == "peaked":
                assert float(((qq.double() @ kk.double().T) * scale).std()) > 10
            if family == "dominant":
                assert 15.0 <= base2_gap_to_median(qq, kk, scale) <= 22.0
            if family == "over_soft":
                ex = late_key_excess(qq, kk, scale, n - 2)
                assert n - 2 >= KVB and 14.0 < float(ex.min()) and float(ex.max()) < 15.9
            if family == "over_hard":
                assert n - 2 >= KVB and float(late_key_excess(qq, kk, scale, n - 2).min()) >= 20.0
    qkv = torch.cat([q, k, v], dim=2)
    got = _packed_attention(h, qkv, B=B, n=n, heads=heads, dh=dh, scale=scale, variant=variant)
    _check_attention(got, qkv, heads=heads, dh=dh, scale=scale, pairs=[(b, hd) for b in range(B) for hd in range(heads)],
                     what=f"dh64 stress {family} {dt} variant={variant}")


def test_attention_dh64_has_no_shared_score_form():
    """The one new instantiation is the plain call; the shared-score forms stay at dh 8 | 16 | 32 | 40 and refuse 64 on the host."""
    h = hip()
    assert not h.load().vface_attention_shared_scores_supported(64, 2)
    dt, heads, dh, n, B = torch.float16, 2, 64, 16, 1
    d = heads * dh
    z = torch.zeros(2 * B * n * d, dtype=dt, device=DEV)
    keep = sentinel(2 * B * n, d, dt).flatten()
    out = keep.to(DEV)
    with pytest.raises(h.VFaceHipError, match=rf"\(code {ERR_SHAPE}\)"):
        h.attention(z, z, z, out, B=B, heads=heads, n=n, nk=n, dh=dh, ldq=d, ldk=d, ldv=d, bsq=n * d, bsk=n * d, bsv=n * d, ldo=d,
                    bso=n * d, scale=0.125, v_sets=2, set_stride=1)
    torch.cuda.synchronize()
    assert same_bits(out.cpu(), keep)


# ------------------------------------------------------------------------------------------------ vface_clip_patches
def _patches(h, img, grid, dt, *, prep, mask=None, dbg=False):
    """The kernel's patch matrix ``[B grid grid, 640]`` on the CPU (frame checked), and the two index vectors when asked."""
    B, _, H, W = img.shape
    out = Framed(B * grid * grid, cb.PATCH_KP, dt)
    S = cb.PATCH * grid
    dx = torch.full((S,), -7, dtype=torch.int32, device=DEV) if dbg else None
    dy = torch.full((S,), -7, dtype=torch.int32, device=DEV) if dbg else None
    src, mk = img.to(DEV), None if mask is None else mask.to(DEV)
    h.clip_patches(src, out.view, B=B, grid=grid, H=H, W=W, ldo=out.ld, prep=prep, mask=mk, dbg_x0=dx, dbg_y0=dy)
    got = out.result("clip_patches")
    assert same_bits(src.cpu(), img), "the image changed"
    return (got, dx.cpu(), dy.cpu()) if dbg else got


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("grid", [3, 16])
def test_clip_patches_pass_through_is_the_unfolded_image_bit_for_bit(dt, grid):
    """Data movement: row (b, py, px), column c 196 + ky 14 + kx holds the image's pixel rounded once; columns 588 .. 639 are +0."""
    h = hip()
    B, S = 2, cb.PATCH * grid
    img = torch.randn(B, 3, S, S, generator=torch.Generator().manual_seed(grid)) * 1.5
    got = _patches(h, img, grid, dt, prep=False)
    assert same_bits(got[:, :cb.PATCH_K], cb.patch_matrix(img).to(dt)), "patch order"
    assert same_bits(got[:, cb.PATCH_K:], torch.zeros(B * grid * grid, cb.PATCH_KP - cb.PATCH_K, dtype=dt)), "zero pad"
    with pytest.raises(h.VFaceHipError, match=rf"\(code {ERR_SHAPE}\)"):        # a pass-through needs the grid's own size
        h.clip_patches(img.to(DEV), torch.empty(B * grid * grid, 640, dtype=dt, device=DEV), B=B, grid=grid + 1, H=S, W=S, ldo=640, prep=False)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("H,W", [(64, 48), (40, 40)])
def test_clip_patches_prep_against_fp64_in_both_orders(dt, H, W, masked):
    """The whole of ``prep`` to a 42 x 42 image (a downscale with two scales, and an upscale), with and without the inpainting mask:
    the reference's two orders (normalise then resize, ddpm.py:907-912; resize then normalise, VFace_inference_batch.py:493-496)
    are ONE fp64 value, the kernel is within the bound of it, and its gather starts at the integer restatement's rows and columns."""
    h = hip()
    B, grid = 2, 3
    S = cb.PATCH * grid
    img = cb.smooth_frames(B, H, W, seed=H + W)
    mask = None
    if masked:
        mask = (torch.rand(B, H, W, generator=torch.Generator().manual_seed(5)) > 0.6).float()
        mask[:, H // 4:H // 2, W // 4:W // 2] = 1.0                      # a solid region and scattered pixels
    got, x0, y0 = _patches(h, img, grid, dt, prep=True, mask=mask, dbg=True)
    assert torch.equal(x0.long(), cb.source_index(W, S)) and torch.equal(y0.long(), cb.source_index(H, S)), "gather footprint"
    ref, bound = cb.prep_ref_and_bound(img, mask, S, dt)
    other = cb.prep_ref(img, mask, S, order="resize_first")
    assert float((ref - other).abs().max()) <= 1e-13 * float(ref.abs().max()), "the two orders are one value"
    for r in (ref, other):
        err = assert_within(got[:, :cb.PATCH_K], cb.patch_matrix(r), cb.patch_matrix(bound), f"prep {dt} {H}x{W} masked={masked}")
    note("clip_patches", err, cb.patch_matrix(bound))
    assert same_bits(got[:, cb.PATCH_K:], torch.zeros(B * grid * grid, cb.PATCH_KP - cb.PATCH_K, dtype=dt)), "zero pad"


# ------------------------------------------------------------------------------------------------ vface_clip_embed
@pytest.mark.parametrize("tok_dt", [torch.float16, torch.bfloat16, torch.float32])
@pytest.mark.parametrize("P", [9, 256])
@pytest.mark.parametrize("ln", [False, True])
def test_clip_embed_class_row_position_add_row_order(tok_dt, P, ln):
    """B = 3, 9 patches of width 128 (half a wave's columns idle) and 256 of width 1024; without the LayerNorm the rows are torch's
    fp32 sums bit for bit (class row first, the position table per token), with it they are within LayerNorm's fp32 bound.  The
    class rows and the position table are scaled apart so a row taken from the wrong token is far outside it."""
    h = hip()
    B, C = 3, 128 if P == 9 else 1024
    tok = rnd((B * P, C), 31 + P, tok_dt)
    cls, pos = rnd((C,), 32, torch.float32, 3.0), rnd((P + 1, C), 33, torch.float32, 0.5)
    gamma, beta = (1.0 + 0.1 * rnd((C,), 34, torch.float32), 0.1 * rnd((C,), 35, torch.float32)) if ln else (None, None)
    out = Framed(B * (P + 1), C, torch.float32)
    src = strided(tok, 8)
    h.clip_embed(src, cls.to(DEV), pos.to(DEV), out.view, B=B, patches=P, C_=C, ldt=src.stride(0), ldo=out.ld,
                 gamma=None if gamma is None else gamma.to(DEV), beta=None if beta is None else beta.to(DEV))
    got = out.result("clip_embed")
    ref, bound = cb.embed_ref_and_bound(tok, cls, pos, B, gamma, beta)
    note("clip_embed", assert_within(got, ref, bound, f"embed {tok_dt} P={P} ln={ln}"), bound)
    if not ln:      # an fp32 sum of two fp32-representable operands: the kernel's bits are torch's
        rows = torch.cat([cls.view(1, 1, C).expand(B, 1, C), tok.float().view(B, P, C)], 1) + pos[None]
        assert same_bits(got, rows.reshape(B * (P + 1), C))


# ------------------------------------------------------------------------------------------------ vface_act
def _act_inputs(dt, rows, cols):
    v = rnd((rows, cols), 77, dt, 3.0)
    edge = torch.tensor([0.0, -0.0, 12.0, -12.0, 11.5, -11.5, 1e-4, -1e-4, 0.5, -0.5, 6.0, -6.0, 2.0 ** -14, -2.0 ** -14, 8.0, -8.0])
    v[0, :16] = edge.to(dt)
    v[rows - 1, cols - 16:] = edge.flip(0).to(dt)
    ramp = torch.linspace(-12.0, 12.0, cols)
    v[1] = ramp.to(dt)
    return v


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("kind", [0, 1])
@pytest.mark.parametrize("in_place", [False, True])
def test_act_quick_gelu_and_erf_gelu(dt, kind, in_place):
    """|v| up to 12, the signed zeros, a ramp over the whole range; a strided input view with NaN around it; in place."""
    h = hip()
    rows, cols = 37, 136
    v = _act_inputs(dt, rows, cols)
    ref, bound = cb.act_ref_and_bound(v, kind, dt)
    if in_place:
        out = Framed(rows, cols, dt)
        out.view.copy_(v.to(DEV))
        out.keep = out.dev.cpu()
        h.act(out.view, out.view, rows=rows, cols=cols, ldx=out.ld, ldy=out.ld, kind=kind)
    else:
        out = Framed(rows, cols, dt)
        src = strided(v, 8)
        h.act(src, out.view, rows=rows, cols=cols, ldx=src.stride(0), ldy=out.ld, kind=kind)
    got = out.result("act")
    note(f"act{kind}", assert_within(got, ref, bound, f"act kind={kind} {dt} in_place={in_place}"), bound)
    assert float(got[0, 0]) == 0.0 and float(got[0, 1]) == 0.0, "act(+-0) is 0"


# ------------------------------------------------------------------------------------------------ vface_cond_mix
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("rows", [(5, 5, 5), (1, 5, 5), (5, 1, 1), (5, 5, 0), (0, 5, 5)])
def test_cond_mix_broadcast_absent_operand_shipped_weights(dt, rows):
    """(c w_c + c2 w_id + lm w_lm) / (w_c + w_id + w_lm) with the shipped weights 1, 10, 0.05: every operand per sample, the first
    / the last two as one row for all, and one operand absent (its weight leaves the sum); fp32 and 16-bit outputs of one launch."""
    h = hip()
    B, N = 5, 768
    ops = [(rnd((r, N), 50 + i, torch.float32) if r else None, w) for i, (r, w) in enumerate(zip(rows, cb.WEIGHTS))]
    o32, o16 = Framed(B, N, torch.float32), Framed(B, N, dt)
    h.cond_mix([(None if t is None else t.to(DEV), w) for t, w in ops], B=B, N=N, out32=o32.view, ldo32=o32.ld, out16=o16.view, ldo16=o16.ld)
    ref, e32 = cb.mix_ref_and_bound(ops, B)
    g32, g16 = o32.result("cond_mix fp32"), o16.result("cond_mix 16-bit")
    note("cond_mix", assert_within(g32, ref, e32, f"mix fp32 rows={rows}"), e32)
    from kernel_bounds import as_16bit
    assert_within(g16, ref, as_16bit(ref, e32, dt), f"mix {dt} rows={rows}")
    assert same_bits(g16, g32.to(dt)), "the 16-bit output is the fp32 output rounded once"
