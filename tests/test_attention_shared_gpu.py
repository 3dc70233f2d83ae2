"""The shared-score instantiations of ``vface_attention`` (``v_sets`` 2 or 3: one softmax of q, k sample b applied to the values of
samples b, b + set_stride [, b + 2 set_stride]; ``v_sets_live`` 2 of 3: the dead-branch batch) per element against fp64 on the
MI355X, with the helpers, the buffers and the bound of test_attention_gpu.py (``kernel_bounds.attention_ref_and_bound``, unchanged:
test_attention_bound_cpu.py shows it admits the model with either denominator form and refuses the seeded defects for 2 and 3
sets too).  For output sample b + g set_stride the reference is the fp64 softmax of q, k of sample b applied to v of sample
``v_map[b + g set_stride]``.  Every value sample is drawn with its own seed, scale and offset, so a set or a frame taken for
another lands far outside the bound; the samples the call must neither read nor write -- gap samples, and the third set of
``v_sets_live = 2`` -- lie inside the allocations as poison / sentinel (``_launch(dead=...)``).

Which case reaches which instantiation of ``dispatch_l`` (template arguments DH, QT, G, LAZY, W32, NWV, GL; each in both dtypes):

  <dh, 2, 2, true>            dh 8, 16, 32, 40     grid[(2, 2)], set_stride[(2, 2)] (dh 40, 8), v_map[(2, 2)] (dh 40, 16), stress (dh 40, 8)
  <dh, 2, 2, false>           exact scale          stress variant 2 at dh 40 and 8 with (2, 2)
  <dh, 2, 3, true>            dh 8, 16, 32         grid[(3, 3)], set_stride (dh 8), v_map (dh 16), stress dh 16 / 32
  <40, 2, 3, true, false, 8>  eight waves          grid[(3, 3)] dh 40, set_stride, v_map, stress variant 0, production
  <40, 2, 3, true>            four waves           stress variant 8 with (3, 3)
  <40, 2, 3, true, true>      32 x 32 x 16         stress variant 4 with (3, 3)
  <40, 2, 3, false, ...>      exact scale          stress variant 2 with (3, 3)
  <dh, 2, 3, true, false, 4, 2>   2 live of 3      grid[(3, 2)] dh 8, 16, 32, set_stride (dh 8), v_map (dh 16), stress dh 32
  <40, 2, 3, true, false, 8, 2>   eight waves      grid[(3, 2)] dh 40, set_stride, v_map, stress variant 0, production
  <40, 2, 3, true, false, 4, 2>   four waves       stress variant 8 with (3, 2)
  <.., false, .., 2>              exact scale      stress variant 2 with (3, 2)"""
import functools

import pytest
import torch

from attention_model import AGGREGATE_MARGIN, KVB, attention_model, base2_gap_to_median, late_key_excess, make_inputs, ones_column
from kernel_bounds import attention_ref_and_bound, rnd, same_bits, sentinel
from test_attention_gpu import DEV, DTS, ERR_SHAPE, _check, _launch, hip

pytestmark = pytest.mark.gpu

SETS = [(2, 2), (3, 3), (3, 2)]                     # (v_sets, v_sets_live)


def _samples(B, G, live, ss):
    """(all samples of the allocation, the live output samples, the dead ones) of B frames in G sets ``ss`` samples apart."""
    Bo = (G - 1) * ss + B
    alive = [b + g * ss for g in range(live) for b in range(B)]
    return Bo, alive, [s for s in range(Bo) if s not in alive]


def _values(Bo, nk, d, dt, seed):
    """``[Bo, nk, d]``: every sample with its own seed, scale and offset."""
    return torch.stack([(rnd((nk, d), seed + 31 * s, torch.float32) * (0.5 + 0.3 * s) + 0.4 * (s - 2)).to(dt) for s in range(Bo)])


def _run(h, dt, *, B, heads, dh, n, nk, G, live, ss, seed, scale=None, v_map=None, nan=True, variant=0, what=""):
    d = heads * dh
    scale = dh ** -0.5 if scale is None else scale
    Bo, alive, dead = _samples(B, G, live, ss)
    q, k, v = rnd((B, n, d), seed, dt), rnd((B, nk, d), seed + 1, dt), _values(Bo, nk, d, dt, seed + 2)
    kw = dict(v_map=v_map.to(DEV)) if v_map is not None else {}
    got = _launch(h, q, k, v, heads=heads, dh=dh, scale=scale, nan=nan, dead=dead, v_sets=G, v_sets_live=live, set_stride=ss,
                  variant=variant, **kw)
    return _check(got, q, k, v, heads=heads, dh=dh, scale=scale, pairs=[(o, hd) for o in alive for hd in range(heads)],
                  qk_map=[o % ss for o in range(Bo)], v_map=v_map, what=what)


# ------------------------------------------------------------------------------------------------ 1: grid
NKS = [1, 63, 64, 65, 77, 128, 200]


def _edges(G, dh):
    """n on and one past the queries per workgroup (16 x waves x 2 query tiles): eight waves at dh = 40 with three sets."""
    return [128, 129, 256, 257] if (G == 3 and dh == 40) else [128, 129]


def _grid():
    """(G, live) x dh x n x nk thinned as test_attention_gpu._grid does: per instantiation every nk and every n at least once, every
    query-tile edge with two key walks, nk != n throughout (checked here, at collection)."""
    cases = []
    for G, live in SETS:
        for dh in (8, 16, 32, 40):
            edges = _edges(G, dh)
            ns = edges + [1, 17]
            m = max(len(ns), len(NKS))
            off = next(o for o in range(len(ns)) if all(ns[(i + o) % len(ns)] != NKS[i % len(NKS)] for i in range(m)))
            mine = [(ns[(i + off) % len(ns)], NKS[i % len(NKS)]) for i in range(m)]
            for j, n in enumerate(edges):
                mine += [(n, (63, 64, 65, 200)[j % 4]), (n, (65, 77, 1, 64)[j % 4])]
            mine = sorted(set(mine))
            assert {nk for _, nk in mine} == set(NKS) and {n for n, _ in mine} == set(ns) and all(n != nk for n, nk in mine)
            assert all(len({nk for n_, nk in mine if n_ == n}) >= 2 for n in edges)
            cases += [(G, live, dh, n, nk) for n, nk in mine]
    return cases


GRID = _grid()


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("G,live,dh,n,nk", GRID)
def test_shared_scores_grid_strided_poisoned_views(dt, G, live, dh, n, nk):
    scale = dh ** -0.5 * (0.6 if (dh + n + nk) % 3 == 0 else 1.0)
    _run(hip(), dt, B=2, heads=3, dh=dh, n=n, nk=nk, G=G, live=live, ss=2, seed=100 + n + nk, scale=scale, nan=(n + nk) % 2 == 0,
         what=f"sets grid {dt} G={G}/{live} dh={dh} n={n} nk={nk}")


# ------------------------------------------------------------------------------------------------ 2: a gap sample between sets
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("G,live", SETS)
@pytest.mark.parametrize("dh,n,nk", [(40, 257, 77), (8, 129, 200)])
def test_set_stride_past_the_batch(dt, G, live, dh, n, nk):
    """``set_stride = B + 1``: one sample between two sets belongs to nobody.  Its v is poison and is never read, its output keeps
    its bits; an output or value sample taken ``B`` apart instead lands in it."""
    _run(hip(), dt, B=2, heads=3, dh=dh, n=n, nk=nk, G=G, live=live, ss=3, seed=7 + dh, nan=dh == 40,
         what=f"set stride {dt} G={G}/{live} dh={dh} n={n} nk={nk}")


# ------------------------------------------------------------------------------------------------ 3: v_map per set
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("G,live", SETS)
@pytest.mark.parametrize("dh,n,nk,which", [(40, 200, 77, "perm"), (16, 130, 65, "perm"), (40, 96, 200, "v_fixed"), (16, 70, 128, "v_fixed")])
def test_value_maps_per_set(dt, G, live, dh, n, nk, which):
    """``v_map`` is indexed with the OUTPUT sample b + g set_stride: a permutation over the value samples of the live sets, and the
    engine's ``v_fixed`` map (set 0 itself, every later set its first frame).  Entries of a dead set point at its poison."""
    from vface_amd.engine import sample_map
    B = 2
    Bo, alive, dead = _samples(B, G, live, B)
    if which == "perm":
        order = torch.randperm(len(alive), generator=torch.Generator().manual_seed(G + live + dh)).tolist()
        v_map = torch.arange(Bo, dtype=torch.int32)
        for o, src in zip(alive, order):
            v_map[o] = alive[src]
        assert sorted(v_map[alive].tolist()) == alive and v_map[alive].tolist() != alive
    else:
        v_map = sample_map("v_fixed", Bo, B)
        assert v_map.tolist() == [0, 1, 2, 2, 4, 4][:Bo]
    _run(hip(), dt, B=B, heads=3, dh=dh, n=n, nk=nk, G=G, live=live, ss=B, seed=11 + dh, v_map=v_map, nan=which == "perm",
         what=f"sets maps {dt} G={G}/{live} dh={dh} n={n} nk={nk} {which}")


# ------------------------------------------------------------------------------------------------ 4: softmax stress
FAMS = ("peaked", "late_spike", "dominant", "over_soft", "over_hard")
VARIANTS = {(2, 2): (0, 2), (3, 3): (0, 2, 8, 4), (3, 2): (0, 2, 8)}      # 8: four waves (dh 40, three sets); 4: 32 x 32 x 16 (all live)
STRESS = [(fam, 40, G, live, var) for fam in FAMS for G, live in SETS for var in VARIANTS[(G, live)]]
STRESS += [(fam, 8, 2, 2, var) for fam in FAMS for var in (0, 2)]          # dh 8 with two sets: no ones column, where one set has one
STRESS += [("peaked", 16, 3, 3, 0), ("late_spike", 32, 3, 2, 0)]


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("family,dh,G,live,variant", STRESS)
def test_shared_scores_softmax_stress(dt, family, dh, G, live, variant):
    """The five families of ``attention_model.make_inputs`` at n = 320, nk = 640 (ten key blocks, a query tail) on the forms that have
    no speculative pass: the lazily raised reference of the default form and the exact scale (variant 2), on four waves (8) and on
    the 32 x 32 x 16 form (4) where they exist.  q, k of every (frame, head) and v of every (sample, head) are drawn apart; all live
    sets of every frame are checked, on the head (frame + set) % 3."""
    h = hip()
    B, heads, n, nk, ss = 2, 3, 320, 640, 2
    scale = dh ** -0.5
    Bo, alive, dead = _samples(B, G, live, ss)
    parts = [[make_inputs(family, dt, n, nk, dh, scale, seed=7 * b + hd) for hd in range(heads)] for b in range(B)]
    q, k = (torch.stack([torch.cat([parts[b][hd][i] for hd in range(heads)], dim=1) for b in range(B)]) for i in range(2))
    v = _values(Bo, nk, heads * dh, dt, 900 + dh)
    if dh == 40:
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
    got = _launch(h, q, k, v, heads=heads, dh=dh, scale=scale, nan=variant != 0, dead=dead, v_sets=G, v_sets_live=live, set_stride=ss,
                  variant=variant)
    _check(got, q, k, v, heads=heads, dh=dh, scale=scale, pairs=[(o, (o % ss + o // ss) % heads) for o in alive],
           qk_map=[o % ss for o in range(Bo)], what=f"sets stress {family} {dt} dh={dh} G={G}/{live} variant={variant}")


# ------------------------------------------------------------------------------------------------ 5: production shape
PROD = dict(F=2, heads=8, dh=40, n=4096)
TRIPLES = {3: [(0, 5, 0), (1, 2, 1), (0, 7, 2), (1, 0, 2)], 2: [(0, 5, 0), (1, 2, 1), (1, 6, 0), (0, 3, 1)]}      # (frame, head, set) by live sets


@functools.lru_cache(maxsize=None)
def _prod_inputs(dt):
    """``[3F, n, 3d]``: q | k | v packed as ``UNetEngine._attn1`` passes them; the v third of every sample on its own scale and offset."""
    F_, heads, dh, n = (PROD[key] for key in ("F", "heads", "dh", "n"))
    d = heads * dh
    qkv = rnd((3 * F_, n, 3 * d), 77, dt)
    qkv[:, :, 2 * d:] = _values(3 * F_, n, d, dt, 78)
    return qkv


@functools.lru_cache(maxsize=None)
def _prod_ref(dt, f, hd, g):
    """(fp64 reference, bound, CPU model) of one (frame, head, set): computed once, shared by the two cases, left unchanged."""
    F_, heads, dh, n = (PROD[key] for key in ("F", "heads", "dh", "n"))
    d = heads * dh
    qkv = _prod_inputs(dt)
    c = slice(hd * dh, (hd + 1) * dh)
    q, k, v = qkv[f, :, :d][:, c], qkv[f, :, d:2 * d][:, c], qkv[f + g * F_, :, 2 * d:][:, c]
    o, bound = attention_ref_and_bound(q, k, v, dh ** -0.5, dt)
    return o, bound, attention_model(q, k, v, dh ** -0.5, dt, form="lazy", denom_rounded=ones_column(3 * dh))


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("live", [3, 2])
def test_shared_scores_at_the_production_shape(dt, live):
    """Level 0 of the ``replace`` schedule: dh = 40, n = nk = 4096, 8 heads, F = 2 frames, three sets ``F`` samples apart in one
    ``[3F, n, 3d]`` buffer; all three live, and 2 live of 3.  Whatever the call must not read is poison: the q | k thirds of every
    sample past the first F and, with 2 live sets, the whole third set.  Four (frame, head, set) triples per element, plus the
    AGGREGATE assertion of test_self_attention_at_production_lengths against the model of this form (lazy reference, denominator
    from the rounded P: 3 x 40 is no multiple of 16): rel_l2(kernel, fp64) <= AGGREGATE_MARGIN * rel_l2(model, fp64).
    Measured on the MI355X, four triples each: three live sets fp16 kernel 2.079e-4, model 2.078e-4; bf16 1.664e-3 both; two live of
    three fp16 1.775e-4 both; bf16 1.421e-3 both; kernel / model 1.000 in all four, as for the plain form: the margin stays 1.25."""
    from kernel_bounds import assert_within
    h = hip()
    F_, heads, dh, n = (PROD[key] for key in ("F", "heads", "dh", "n"))
    d = heads * dh
    scale = dh ** -0.5
    qkv = _prod_inputs(dt).clone()
    qkv[F_:, :, :2 * d] = float("nan")
    if live == 2:
        qkv[2 * F_:] = float("nan")
    before = qkv.clone()
    qd = qkv.to(DEV)
    Bo = 3 * F_
    ldo, bso = d + 12, (n + 2) * (d + 12)
    keep = sentinel(1, 4 + Bo * bso + ldo, dt).flatten()
    od = keep.to(DEV)
    h.attention(qd, qd[:, :, d:], qd[:, :, 2 * d:], od[4:], B=F_, heads=heads, n=n, nk=n, dh=dh, ldq=3 * d, ldk=3 * d, ldv=3 * d,
                bsq=n * 3 * d, bsk=n * 3 * d, bsv=n * 3 * d, ldo=ldo, bso=bso, scale=scale, v_sets=3, v_sets_live=live, set_stride=F_)
    torch.cuda.synchronize()
    got_all = od.cpu()
    view = lambda t: t[4:4 + Bo * bso].as_strided((Bo, n, d), (bso, ldo, 1))
    got = view(got_all).clone()
    expect = keep.clone()
    view(expect)[:live * F_] = got[:live * F_]
    assert same_bits(got_all, expect), "a store outside the output view (or into the dead set)"
    assert same_bits(qd.cpu(), before), "an input changed"
    num = den = ref2 = 0.0
    for f, hd, g in TRIPLES[live]:
        o, bound, m = _prod_ref(dt, f, hd, g)
        mine = got[f + g * F_][:, hd * dh:(hd + 1) * dh]
        err = assert_within(mine, o, bound, f"production sets {dt} live={live} frame {f} head {hd} set {g}")
        print(f"production sets {dt} live={live} frame {f} head {hd} set {g}: worst err / bound {float((err / bound).max()):.3f}")
        num += float((mine.double() - o).square().sum())
        den += float((m.double() - o).square().sum())
        ref2 += float(o.square().sum())
    kern, model = (num / ref2) ** 0.5, (den / ref2) ** 0.5
    print(f"aggregate sets {dt} live={live}: rel-L2 kernel {kern:.3e} model {model:.3e} kernel / model {kern / model:.3f}")
    assert AGGREGATE_MARGIN <= 2.0 and kern <= AGGREGATE_MARGIN * model, (kern, model)


# ------------------------------------------------------------------------------------------------ 6: refusals on the host
def test_refusals_with_value_sets_return_before_any_launch():
    """What ``vf_launch_attention`` rejects of a shared-score call, with the code it documents; the output keeps its bits."""
    h = hip()
    dt, heads, dh, n, nk, B = torch.float16, 2, 40, 16, 24, 2
    d = heads * dh
    q = torch.zeros(B * n * d, dtype=dt, device=DEV)
    k = torch.zeros(B * nk * d, dtype=dt, device=DEV)
    v = torch.zeros(3 * B * nk * d, dtype=dt, device=DEV)
    keep = sentinel(3 * B * n, d, dt).flatten()
    out = keep.to(DEV)
    base = dict(B=B, heads=heads, n=n, nk=nk, dh=dh, ldq=d, ldk=d, ldv=d, bsq=n * d, bsk=nk * d, bsv=nk * d, ldo=d, bso=n * d, scale=dh ** -0.5,
                v_sets=3, set_stride=B)
    h.attention(q, k, v, out, **base)                                  # the base call itself is accepted
    torch.cuda.synchronize()
    assert not same_bits(out.cpu(), keep)
    out.copy_(keep)
    q80 = torch.zeros(B * n * 160, dtype=dt, device=DEV)
    for tensors, change in (((q80, q80, q80), dict(dh=80, ldq=160, ldk=160, ldv=160, bsq=n * 160, bsk=nk * 160, bsv=nk * 160, ldo=160, bso=n * 160)),
                            ((q, k, v), dict(set_stride=0)), ((q, k, v), dict(v_sets=4)), ((q, k, v), dict(v_sets=2, v_sets_live=1)),
                            # 2 sets of a stride of 2 + 2 frames = 6 samples: the fifth sample stride is what passes 4 GiB
                            ((q, k, v), dict(bsk=2 ** 29)), ((q, k, v), dict(bsv=2 ** 29)),
                            ((q, k, v), dict(v_sets=2, set_stride=5, bsv=2 ** 29))):
        with pytest.raises(h.VFaceHipError, match=rf"\(code {ERR_SHAPE}\)"):
            h.attention(*tensors, out, **{**base, **change})
    torch.cuda.synchronize()
    assert same_bits(out.cpu(), keep)
    # the same sample stride with ONE set would stay below 4 GiB: it is the set stride that the extent is computed with
    assert (B - 1) * 2 ** 29 * 2 < 0xFFFFFFF0 <= ((3 - 1) * B + B - 1) * 2 ** 29 * 2
