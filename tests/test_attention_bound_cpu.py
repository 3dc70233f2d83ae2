"""The attention bound's own test, no GPU: ``kernel_bounds.attention_ref_and_bound`` must admit the CPU model of the kernel's rounding
points (``attention_model``: lazy, exact and speculative reference, denominator from rounded or unrounded P) on EVERY element, and
must refuse each seeded one-line defect on the input family meant to expose it.  That is what shows that test_attention_gpu.py can
fail.  The only threshold is 1 (error / bound); which defect shows on which family is reasoned below, not fitted:

* tail_unmasked -- keys past nk take part with K = 0 (score 0): visible when nk % 64 != 0 and a score of 0 carries weight, i.e. on
  flat rows and where the few live keys of the last block are not far above 0 (N(0,1), late spike at nk = 77).
* no_rescale -- O keeps its old scale when the reference rises: needs a reference that rises after block 0 (peaked, late spike,
  the two overflow families).
* flush_p -- fp16 only: probabilities below 2^-14 lost; needs most of the row there (dominant key, rest ~18 base-2 units below).
* o16 -- O rounded to 16 bits after every key block: error grows with the block count; per element it shows on the dominant family
  from 16 blocks on in fp16 (bound ~1.5 ulp; bf16 from 64 blocks on at dh >= 80), on flat rows only in aggregate -- the rel-L2
  ratio to the correct model at 4096 keys.
* last_key_dropped -- one key of nk: visible while one key weighs more than the bound (flat rows up to ~1024 keys in fp16, ~200 in
  bf16)."""
import pytest
import torch

from attention_model import AGGREGATE_MARGIN, DEFECTS, attention_model, base2_gap_to_median, late_key_excess, make_inputs
from conftest import rel_l2
from kernel_bounds import attention_ref_and_bound

N = 48
DTS = [torch.float16, torch.bfloat16]
FORMS = [(f, r) for f in ("lazy", "exact", "spec") for r in (True, False)]


def expected_outside(family, dt, nk, dh):
    f16 = dt == torch.float16
    out = set()
    if family == "normal":
        if (-nk) % 64 >= 8:                          # a single padding key among 63 flat ones stays inside the bf16 bound
            out.add("tail_unmasked")
        if nk <= (1024 if f16 else 200):
            out.add("last_key_dropped")
    elif family == "peaked":
        out.add("no_rescale")
        if f16 and nk == 200:
            out.add("flush_p")
    elif family == "late_spike":
        out.add("no_rescale")
        if nk == 77:
            out.add("tail_unmasked")
    elif family == "dominant":
        if f16:
            out.add("flush_p")
        if nk >= 1024 and (f16 or (nk >= 4096 and dh >= 80)):
            out.add("o16")
    elif family in ("over_soft", "over_hard"):
        out.add("no_rescale")
    return out


def worst_ratio(got, o, b):
    got = got.double()
    if not bool(torch.isfinite(got).all()):
        return float("inf")
    return float(((got - o).abs() / b).max())


CASES = [(fam, dh, nk) for fam in ("normal", "peaked", "late_spike", "dominant") for dh in (40, 80) for nk in (77, 200, 1024)]
CASES += [(fam, 40, 200) for fam in ("over_soft", "over_hard")] + [("normal", 160, 200), ("dominant", 160, 1024), ("dominant", 80, 4096), ("normal", 8, 65), ("normal", 16, 63), ("normal", 32, 50)]


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("family,dh,nk", CASES)
def test_bound_admits_the_model_and_refuses_each_defect(dt, family, dh, nk):
    scale = dh ** -0.5 if (dh + nk) % 3 else 1.3 * dh ** -0.5
    q, k, v = make_inputs(family, dt, N, nk, dh, scale, seed=nk + dh)
    o, b = attention_ref_and_bound(q, k, v, scale, dt)
    assert bool((b > 0).all()) and bool(torch.isfinite(b).all())
    if family == "dominant":
        assert 15.0 <= base2_gap_to_median(q, k, scale) <= 22.0
    if family == "over_soft":
        ex = late_key_excess(q, k, scale, nk - 2)
        assert 14.0 < float(ex.min()) and float(ex.max()) < 15.9, (float(ex.min()), float(ex.max()))
    if family == "over_hard":
        assert float(late_key_excess(q, k, scale, nk - 2).min()) >= 20.0
    for form, rounded in FORMS:
        r = worst_ratio(attention_model(q, k, v, scale, dt, form=form, denom_rounded=rounded), o, b)
        print(f"{family} {dt} dh={dh} nk={nk} {form} denom_rounded={rounded}: worst err / bound {r:.3f}")
        assert r <= 1.0, (form, rounded, r)
    want = expected_outside(family, dt, nk, dh)
    for d in DEFECTS:
        r = worst_ratio(attention_model(q, k, v, scale, dt, defect=d), o, b)
        print(f"{family} {dt} dh={dh} nk={nk} defect {d}: worst err / bound {r:.3g}")
        if d in want:
            assert r > 1.0, (d, r)


def test_every_defect_is_refused_somewhere():
    seen = set()
    for dt in DTS:
        for family, dh, nk in CASES:
            seen |= expected_outside(family, dt, nk, dh)
    assert seen == set(DEFECTS)


@pytest.mark.parametrize("dt", DTS)
def test_aggregate_margin_separates_16_bit_accumulation_at_4096_keys(dt):
    """Flat rows at 4096 keys: the per-element bound leaves 16-bit accumulation of O inside (~0.3 of it); the aggregate assertion of
    test_attention_gpu.py -- rel-L2 to fp64 at most AGGREGATE_MARGIN x the correct model's -- does not."""
    dh, nk = 40, 4096
    scale = dh ** -0.5
    q, k, v = make_inputs("normal", dt, 4 * N, nk, dh, scale, seed=5)
    o, b = attention_ref_and_bound(q, k, v, scale, dt)
    good = attention_model(q, k, v, scale, dt)
    assert worst_ratio(good, o, b) <= 1.0
    for form in ("exact", "spec"):
        assert rel_l2(attention_model(q, k, v, scale, dt, form=form), o) <= AGGREGATE_MARGIN * rel_l2(good, o)
    ratio = rel_l2(attention_model(q, k, v, scale, dt, defect="o16"), o) / rel_l2(good, o)
    print(f"{dt}: 16-bit O / correct model rel-L2 = {ratio:.2f}, model rel-L2 {rel_l2(good, o):.2e}")
    assert AGGREGATE_MARGIN <= 2.0 and ratio > AGGREGATE_MARGIN


# ------------------------------------------------------------------------------------------------- the shared-score instantiations
SET_SHAPES = [(130, 200), (17, 63), (129, 65)]


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("sets", [2, 3])
@pytest.mark.parametrize("dh", [8, 16, 32, 40])
@pytest.mark.parametrize("n,nk", SET_SHAPES)
def test_bound_admits_the_shared_score_forms_and_refuses_the_same_defects(dt, sets, dh, n, nk):
    """The shared-score instantiations (2 or 3 value sets behind one softmax) have neither a speculative pass nor, set for set, other
    arithmetic than the plain kernel -- but the spare column that forms the denominator exists for OTHER head dims (sets x dh no
    multiple of 16: dh 40 and 8 with 3 sets, neither with 2).  ``attention_model(sets=...)`` selects that form: inside the bound
    on all six families, lazy and exact scale; and every defect the bound refuses for one set it refuses here."""
    scale = dh ** -0.5
    seen = set()
    for family in ("normal", "peaked", "late_spike", "dominant", "over_soft", "over_hard"):
        q, k, v = make_inputs(family, dt, n, nk, dh, scale, seed=nk + dh)
        o, b = attention_ref_and_bound(q, k, v, scale, dt)
        for form in ("lazy", "exact"):
            r = worst_ratio(attention_model(q, k, v, scale, dt, form=form, sets=sets), o, b)
            print(f"{family} {dt} dh={dh} sets={sets} n={n} nk={nk} {form}: worst err / bound {r:.3f}")
            assert r <= 1.0, (family, form, r)
        for d in DEFECTS:
            one = worst_ratio(attention_model(q, k, v, scale, dt, defect=d), o, b)
            many = worst_ratio(attention_model(q, k, v, scale, dt, defect=d, sets=sets), o, b)
            if d == "flush_p":
                # the one defect whose size depends on the denominator form itself (a denominator summed from the unrounded P does
                # not lose what the numerator loses): held to its own reasoning, not to the one-set form -- fp16, most of the row in
                # the subnormal range (dominant) and enough keys there for nk 2^-18 to outweigh the bound (nk = 200)
                if family == "dominant" and dt == torch.float16 and nk == 200:
                    assert many > 1.0, (family, d, many)
                    seen.add(d)
            elif one > 1.0:
                assert many > 1.0, (family, d, one, many)
                seen.add(d)
    # a dropped key shows at every one of these shapes, a missing rescale wherever there is a second key block, an unmasked tail
    # wherever the last block has 8 padding keys or more; 16-bit O needs 16 key blocks and more (test_aggregate_margin_...)
    want = {"last_key_dropped"} | ({"no_rescale"} if nk > 64 else set()) | ({"tail_unmasked"} if (-nk) % 64 >= 8 else set())
    want |= {"flush_p"} if dt == torch.float16 and nk == 200 else set()
    assert seen >= want, (seen, want)


def test_the_model_takes_the_denominator_form_of_the_value_tile():
    from attention_model import ones_column
    assert [ones_column(g * dh) for g in (1, 2, 3) for dh in (8, 16, 32, 40)] == [True, False, False, True, False, False, False, False,
                                                                                   True, False, False, True]
