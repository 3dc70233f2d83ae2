"""``vface_attention`` per element against fp64 on the MI355X: every output of every checked (sample, head) within
``kernel_bounds.attention_ref_and_bound`` -- a bound built from fp64 quantities of the reference alone, shown by
test_attention_bound_cpu.py to admit a model of the kernel's rounding points and to refuse one-line defects of it -- at nk != n,
on key and query tails, through strided views whose surroundings are poisoned, at the production lengths, and on softmax inputs
that stress the lazily raised / speculative reference.  Everything goes through ``hip.attention``; default dispatch unless said.

Buffers (``_launch``): q, k, v in three allocations, row strides d + 24 / d + 40 / d + 56, the view 8 elements
into its allocation, one / two / three gap rows between samples; every element the call must not read is NaN or +-6e4.  The output
goes 4 elements into a ``sentinel`` buffer with row stride d + 12 and two gap rows per sample; after the call every element outside
the output view has its sentinel bits."""
import pytest
import torch

from attention_model import AGGREGATE_MARGIN, KVB, attention_model, base2_gap_to_median, late_key_excess, make_inputs
from kernel_bounds import assert_within, attention_ref_and_bound, rnd, same_bits, sentinel

pytestmark = pytest.mark.gpu

DEV = "cuda"
DTS = [torch.float16, torch.bfloat16]
ERR_ARG, ERR_ALIGN, ERR_SHAPE = -1, -2, -3          # include/vface_hip.h


def hip():
    from vface_amd import hip as h
    h.load()
    return h


def _poisoned(total, dt, nan):
    if nan:
        return torch.full((total,), float("nan"), dtype=dt)
    return (6.0e4 * (1.0 - 2.0 * (torch.arange(total) % 2))).to(dt)


def _strided(x, ld, gap_rows, off, nan):
    """``x [B, rows, d]`` laid into a poisoned flat buffer: returns (buffer, element offset of the view, ld, sample stride)."""
    B, rows, d = x.shape
    bs = (rows + gap_rows) * ld
    buf = _poisoned(off + B * bs, x.dtype, nan)
    buf[off:off + B * bs].as_strided((B, rows, d), (bs, ld, 1)).copy_(x)
    return buf, off, ld, bs


def _launch(h, q, k, v, *, heads, dh, scale, nan=True, dead=(), **kw):
    """``q [B, n, d]``, ``k [B, nk, d]``, ``v [Bo, nk, d]`` on the CPU -> the kernel's ``[Bo, n, d]`` on the CPU, after the checks on what
    the call must not touch.  Bo = B, or for the shared-score form (``v_sets``, ``set_stride`` [, ``v_sets_live``] in ``kw``)
    (v_sets - 1) set_stride + B: output sample b + g set_stride takes the probabilities of q, k sample b and v of that sample.
    ``dead``: samples of v and of the output that the call must neither read nor write -- a gap sample between two sets and, with 2
    live sets of 3, the third set.  They lie INSIDE both allocations: their v is poison (NaN or +-6e4), their output keeps its
    sentinel bits; a kernel that touches them shows as a wrong value or a changed sentinel, never as an access out of bounds."""
    B, n, d = q.shape
    nk, Bo = k.shape[1], v.shape[0]
    dt = q.dtype
    assert d == heads * dh and Bo == (kw.get("v_sets", 1) - 1) * kw.get("set_stride", 0) + B
    dead = sorted(dead)
    if dead:
        v = v.clone()
        v[dead] = _poisoned(nk * d, dt, nan).reshape(nk, d)
    (qb, qo, ldq, bsq), (kb, ko, ldk, bsk), (vb, vo, ldv, bsv) = (_strided(t, d + p, g, 8, nan) for t, p, g in ((q, 24, 1), (k, 40, 2), (v, 56, 3)))
    ldo, bso, oo = d + 12, (n + 2) * (d + 12), 4
    keep = sentinel(1, oo + Bo * bso + ldo, dt).flatten()
    qd, kd, vd, od = qb.to(DEV), kb.to(DEV), vb.to(DEV), keep.to(DEV)
    h.attention(qd[qo:], kd[ko:], vd[vo:], od[oo:], B=B, heads=heads, n=n, nk=nk, dh=dh, ldq=ldq, ldk=ldk, ldv=ldv, bsq=bsq, bsk=bsk,
                bsv=bsv, ldo=ldo, bso=bso, scale=scale, **kw)
    torch.cuda.synchronize()
    got_all = od.cpu()
    view = lambda t: t[oo:oo + Bo * bso].as_strided((Bo, n, d), (bso, ldo, 1))
    got = view(got_all).clone()
    expect = keep.clone()
    written = [s for s in range(Bo) if s not in dead]
    view(expect)[written] = got[written]
    assert same_bits(got_all, expect), "a store outside the output view (or into a dead sample of it)"
    assert same_bits(qd.cpu(), qb) and same_bits(kd.cpu(), kb) and same_bits(vd.cpu(), vb), "an input changed"
    return got


def _check(got, q, k, v, *, heads, dh, scale, pairs, what, qk_map=None, v_map=None):
    """Every element of the chosen (sample, head) pairs within the bound; returns the worst err / bound."""
    assert bool(torch.isfinite(got.float()).all()), f"{what}: non-finite output"
    worst = 0.0
    for b, hd in pairs:
        bq = int(qk_map[b]) if qk_map is not None else b
        bv = int(v_map[b]) if v_map is not None else b
        c = slice(hd * dh, (hd + 1) * dh)
        o, bound = attention_ref_and_bound(q[bq, :, c], k[bq, :, c], v[bv, :, c], scale, got.dtype)
        err = assert_within(got[b, :, c], o, bound, f"{what} sample {b} head {hd}")
        worst = max(worst, float((err / bound).max()))
    print(f"{what}: worst err / bound {worst:.3f}")
    return worst


def _all_pairs(B, heads):
    return [(b, hd) for b in range(B) for hd in range(heads)]


# ------------------------------------------------------------------------------------------------ 1, 2: cross-attention grid
NKS = [1, 2, 63, 64, 65, 77, 128, 200]
# queries per workgroup (16 * waves * query tiles per wave) of the instantiation the dispatcher picks: n on it and one past it
EDGES = {8: [128, 129], 16: [128, 129], 32: [128, 129], 40: [512, 513], 80: [128, 129], 160: [64, 65, 128, 129, 256, 257]}


def _grid():
    """The product dh x n x nk thinned: per dh every nk and every n at least once, and every query-tile edge with a short, a full, a
    just-over and a long key walk (checked here, at collection)."""
    cases = []
    for dh, edges in EDGES.items():
        ns = edges + [1, 15, 17]
        mine = [(ns[i % len(ns)], NKS[i % len(NKS)]) for i in range(max(len(ns), len(NKS)))]
        for j, n in enumerate(edges):
            mine += [(n, (63, 64, 65, 200)[j % 4]), (n, (65, 128, 2, 64)[j % 4])]
        mine = sorted(set(mine))
        assert {nk for _, nk in mine} == set(NKS) and {n for n, _ in mine} == set(ns)
        assert all(len({nk for n_, nk in mine if n_ == n}) >= 2 for n in edges)
        for group in ((1, 2, 63), (64,), (65,), (128, 200)):
            assert any(nk in group for _, nk in mine)
        cases += [(dh, n, nk) for n, nk in mine]
    return cases


GRID = _grid()


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("dh,n,nk", GRID)
def test_cross_attention_grid_strided_poisoned_views(dt, dh, n, nk):
    h = hip()
    B, heads = 2, 3
    d = heads * dh
    scale = dh ** -0.5 * (0.6 if (dh + n + nk) % 3 == 0 else 1.0)
    q, k, v = rnd((B, n, d), 100 + n, dt), rnd((B, nk, d), 200 + nk, dt), rnd((B, nk, d), 300 + nk + dh, dt)
    got = _launch(h, q, k, v, heads=heads, dh=dh, scale=scale, nan=(n + nk) % 2 == 0)
    _check(got, q, k, v, heads=heads, dh=dh, scale=scale, pairs=_all_pairs(B, heads), what=f"grid {dt} dh={dh} n={n} nk={nk}")


# ------------------------------------------------------------------------------------------------ 3: sample maps with nk != n
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("dh,n,nk,which", [(40, 200, 77, "perm"), (80, 130, 65, "perm"), (40, 96, 200, "v_fixed"), (160, 70, 128, "v_fixed"),
                                           (8, 129, 63, "perm")])
def test_sample_maps_on_separate_k_v_buffers(dt, dh, n, nk, which):
    """qk_map / v_map with the three buffers on three different sample strides: a sample index applied with another buffer's stride
    lands in other data or in poison."""
    from vface_amd.engine import sample_map
    h = hip()
    heads = 2
    d = heads * dh
    if which == "perm":
        B = 4
        qk_map, v_map = torch.tensor([2, 0, 3, 1], dtype=torch.int32), torch.tensor([1, 3, 0, 2], dtype=torch.int32)
    else:
        B = 6
        qk_map, v_map = None, sample_map("v_fixed", B, 2)
        assert v_map.tolist() == [0, 1, 2, 2, 4, 4]
    scale = dh ** -0.5
    q, k, v = rnd((B, n, d), 11, dt), rnd((B, nk, d), 12, dt), rnd((B, nk, d), 13, dt)
    got = _launch(h, q, k, v, heads=heads, dh=dh, scale=scale, nan=which == "perm",
                  qk_map=None if qk_map is None else qk_map.to(DEV), v_map=v_map.to(DEV))
    _check(got, q, k, v, heads=heads, dh=dh, scale=scale, pairs=_all_pairs(B, heads), qk_map=qk_map, v_map=v_map,
           what=f"maps {dt} dh={dh} n={n} nk={nk} {which}")


# ------------------------------------------------------------------------------------------------ 4: production lengths
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("dh,n", [(40, 4096), (80, 1024), (160, 256), (160, 64)])
def test_self_attention_at_production_lengths(dt, dh, n):
    """The UNet's four self-attention shapes, 8 heads, q | k | v packed in one [B, n, 3d] buffer as the engine passes them; all
    queries of four (sample, head) pairs of a seeded draw, per element.

    (40, 4096) adds the one AGGREGATE assertion: on flat rows the per-element bound is weakest against 16-bit accumulation of O
    across key blocks (0.3 .. 0.4 of it), so rel_l2(kernel, fp64) <= AGGREGATE_MARGIN * rel_l2(CPU model, fp64) on the same rows.
    Measured on the MI355X, four (sample, head) pairs: fp16 kernel 3.617e-4, model 3.617e-4; bf16 kernel 2.909e-3, model 2.909e-3;
    kernel / model 1.000 in both (the model is the kernel's arithmetic up to the order of fp32 additions), so the margin is 1.25."""
    h = hip()
    B, heads = 2, 8
    d = heads * dh
    scale = dh ** -0.5
    qkv = rnd((B, n, 3 * d), 41 + dh, dt)
    qd = qkv.to(DEV)
    ldo, bso = d + 12, (n + 2) * (d + 12)
    keep = sentinel(1, 4 + B * bso + ldo, dt).flatten()
    od = keep.to(DEV)
    h.attention(qd, qd[:, :, d:], qd[:, :, 2 * d:], od[4:], B=B, heads=heads, n=n, nk=n, dh=dh, ldq=3 * d, ldk=3 * d, ldv=3 * d,
                bsq=n * 3 * d, bsk=n * 3 * d, bsv=n * 3 * d, ldo=ldo, bso=bso, scale=scale)
    torch.cuda.synchronize()
    got_all = od.cpu()
    view = lambda t: t[4:4 + B * bso].as_strided((B, n, d), (bso, ldo, 1))
    got = view(got_all).clone()
    expect = keep.clone()
    view(expect).copy_(got)
    assert same_bits(got_all, expect), "a store outside the output view"
    q, k, v = qkv[..., :d], qkv[..., d:2 * d], qkv[..., 2 * d:]
    draw = torch.randperm(B * heads, generator=torch.Generator().manual_seed(dh + n))[:4].tolist()
    pairs = [(i // heads, i % heads) for i in draw]
    _check(got, q, k, v, heads=heads, dh=dh, scale=scale, pairs=pairs, what=f"production {dt} dh={dh} n={n}")
    if n >= 4096:
        num = den = ref2 = 0.0
        for b, hd in pairs:
            c = slice(hd * dh, (hd + 1) * dh)
            o, _ = attention_ref_and_bound(q[b, :, c], k[b, :, c], v[b, :, c], scale, dt)
            m = attention_model(q[b, :, c], k[b, :, c], v[b, :, c], scale, dt, form="spec")
            num += float((got[b, :, c].double() - o).square().sum())
            den += float((m.double() - o).square().sum())
            ref2 += float(o.square().sum())
        kern, model = (num / ref2) ** 0.5, (den / ref2) ** 0.5
        print(f"aggregate {dt} dh={dh} n={n}: rel-L2 kernel {kern:.3e} model {model:.3e} kernel / model {kern / model:.3f}")
        assert AGGREGATE_MARGIN <= 2.0 and kern <= AGGREGATE_MARGIN * model, (kern, model)


# ------------------------------------------------------------------------------------------------ 5: softmax stress
STRESS = [(fam, dh, n, nk, variant) for fam in ("peaked", "late_spike", "dominant", "over_soft", "over_hard")
          for dh, n, nk in ((40, 320, 640), (80, 192, 256), (160, 130, 256))
          for variant in ((0, 2, 16, 8) if dh == 40 else (0, 2))]


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("family,dh,n,nk,variant", STRESS)
def test_softmax_stress_per_element(dt, family, dh, n, nk, variant):
    """Ordinary inputs with a defined answer that stress the softmax reference: rows whose maximum keeps rising (peaked), a key
    near the end that dominates (late_spike), one dominant key in the first block with the rest ~18 base-2 units below it -- fp16
    probabilities in the subnormal range, where a flush to zero would lose up to nk * 2^-14 (dominant) --, and a late key 14-15 /
    20 or more base-2 units above the first block's maximum: the speculative pass's fp16 P reaches 2^15 and stays finite / overflows
    and the tile runs again with the checked loop (over_soft / over_hard; in bf16 two more cases).  Variants: 0 default, 2 exact
    scale, 16 checked loop only, 8 four waves per workgroup (dh = 40)."""
    h = hip()
    B, heads = 2, 2
    scale = dh ** -0.5
    parts = [[make_inputs(family, dt, n, nk, dh, scale, seed=7 * b + hd) for hd in range(heads)] for b in range(B)]
    q, k, v = (torch.stack([torch.cat([parts[b][hd][i] for hd in range(heads)], dim=1) for b in range(B)]) for i in range(3))
    for b in range(B):
        for hd in range(heads):
            qq, kk, _ = parts[b][hd]
            if family == "peaked":
                assert float(((qq.double() @ kk.double().T) * scale).std()) > 10
            if family == "dominant":
                assert 15.0 <= base2_gap_to_median(qq, kk, scale) <= 22.0
            if family == "over_soft":
                ex = late_key_excess(qq, kk, scale, nk - 2)
                assert nk - 2 >= KVB and 14.0 < float(ex.min()) and float(ex.max()) < 15.9
            if family == "over_hard":
                assert nk - 2 >= KVB and float(late_key_excess(qq, kk, scale, nk - 2).min()) >= 20.0
    got = _launch(h, q, k, v, heads=heads, dh=dh, scale=scale, nan=variant != 0, variant=variant)
    _check(got, q, k, v, heads=heads, dh=dh, scale=scale, pairs=_all_pairs(B, heads),
           what=f"stress {family} {dt} dh={dh} n={n} nk={nk} variant={variant}")


# ------------------------------------------------------------------------------------------------ 6: refusals on the host
def test_refusals_return_before_any_launch():
    """What ``vf_launch_attention`` rejects on the host, with the code it documents; the output buffer keeps its bits."""
    h = hip()
    dt, heads, dh, n, nk, B = torch.float16, 2, 40, 16, 16, 2
    d = heads * dh
    q = torch.zeros(B * n * d, dtype=dt, device=DEV)
    k = torch.zeros(B * nk * d, dtype=dt, device=DEV)
    v = torch.zeros(B * nk * d, dtype=dt, device=DEV)
    keep = sentinel(B * n, d, dt).flatten()
    out = keep.to(DEV)
    base = dict(B=B, heads=heads, n=n, nk=nk, dh=dh, ldq=d, ldk=d, ldv=d, bsq=n * d, bsk=nk * d, bsv=nk * d, ldo=d, bso=n * d, scale=dh ** -0.5)
    h.attention(q, k, v, out, **base)                                  # the base call itself is accepted
    torch.cuda.synchronize()
    out.copy_(keep)
    for change, code in ((dict(nk=0), ERR_ARG), (dict(ldk=d + 4), ERR_ALIGN), (dict(ldo=d + 2), ERR_ALIGN),
                         (dict(bsk=2 ** 31), ERR_SHAPE),               # the K view would span 4 GiB: past a buffer descriptor's reach
                         (dict(bsv=2 ** 31), ERR_SHAPE),
                         (dict(B=1, v_sets=2, v_sets_live=1, set_stride=1), ERR_SHAPE)):
        with pytest.raises(h.VFaceHipError, match=rf"\(code {code}\)"):
            h.attention(q, k, v, out, **{**base, **change})
    torch.cuda.synchronize()
    assert same_bits(out.cpu(), keep)
