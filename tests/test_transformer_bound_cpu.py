"""The norm and fused-transformer bounds' own test, no GPU: the fp64 references of kernel_bounds.py (``layernorm_ref_and_bound``, ``gn_stats_``,
``gn_cols_``, ``gn_apply_``, ``linear_small_``, ``st_front_*`` and ``ffn_ref_and_bound``) must admit the CPU model of the kernels'
rounding points (transformer_model.py) on EVERY element of every family, in both types, and must refuse each seeded one-line
defect on the families named for it.  That is what shows that test_transformer_kernels_gpu.py can fail.  The only threshold is 1
(error / bound).  Which defect shows where is reasoned, not fitted:

* ln_half_lanes -- LayerNorm statistics over one lane half (C / 2 channels): the mean of half a row is off by spread / sqrt(C / 2)
  (0.09 spreads at C = 256), the output by that times rstd |gamma| -- 100x a bf16 half-ulp.  Every LayerNorm and chain family.
* ln_var_cm1 -- variance over C - 1: rstd, and so t = d rstd gamma, low by 1 / (2 C) = 7.8e-3 at C = 64, 1.6e-3 at C = 320, against a
  half-ulp of 2.4e-4 .. 4.9e-4 |y| (fp16) and 2e-3 .. 3.9e-3 |y| (bf16); beta makes |t| > |y| on many elements.  Asserted at C = 64
  in both types, at C = 320 in fp16 only: in bf16 1.6e-3 |t| needs |t| > 1.2 |y| .. 2.4 |y|, which happens but is not argued for.
* ln_no_eps -- eps dropped: rstd high by eps / (2 var); nothing at spread 1 (5e-6), 41 % at the family whose row spread is
  sqrt(eps) = 3.2e-3 ("ln_sqrt_eps"), where it is asserted, in both types.
* ln_one_pass -- var = E[x^2] - mean^2 in fp32: at mean / spread = 64 the sums carry 4097 var, their fp32 rounding (>= U32 4097 var,
  sqrt(C) times that typically) moves rstd by 1e-4 .. 3e-3 against e32 / |t| ~ C U32 / 2 = 1e-5 and a half-ulp of 2.4e-4 |y| in
  fp16.  Asserted on "ln_offset64" in fp16; NOT in bf16, whose half-ulp (2e-3 |y| and more) is as large as the effect.
* gn_chunk_group -- the group index taken per 8-channel chunk: wrong wherever a chunk spans two groups (cpg = 3, 10, 65), right
  where cpg % 8 == 0.  Statistics, coefficients and apply; images of different mean, groups of different mean.
* gn_tail_pixels -- the last hw % 128 pixels missing from the sums: the mean low by (hw % 128) / hw of itself (1.5 % at hw = 130)
  against D U32 ~ 1e-5.  The statistics families with hw > 128, hw % 128 != 0.
* k_unpermuted -- projection / W2 / proj_out k columns left in the module's order (``packing`` called for the weights, the
  activations not taken in ``ffn_w2_perm`` order): another function of the inputs.  st_front (qkv), PLAIN (W2), PRE (W1), POST.
* image0_ab -- a token tile past the first takes image 0's (a, b): images differ in mean and scale, t0 of tiles 1, 2 is wrong.
* rowbias_sample0 -- a workgroup takes sample 0's row bias: samples' row biases are independent N(0, 0.5): PRE and POST.
* geglu_mispaired -- a value row meets the gate row of its neighbour: another function.  All three forms.
* t1_rounded16 -- t1 rounded to 16 bits before the LayerNorm: t1 moves by up to u |t1|, LayerNorm's own fp32 error is 1e-5, so
  about half of the ln operands round to the other neighbour where ``round_operand`` grants a tie to a few per cent of them; each
  flip is one spacing q of the type, and reaches the output as ~ q |w1| |w2| sqrt(terms): 3e-4 in fp16, 2.4e-3 in bf16.  The
  chain's bound holds the ties it must grant (a_err = d_h |W2|^T over 4C hidden units, ~ 5e-4 at C = 64 IN BOTH TYPES: fewer ties
  in bf16, each 8x larger) -- so the PRE chain refuses it in bf16 at C = 64 and NOT in fp16, nor at C = 128 where a_err has doubled.
  POST refuses it in both types at both widths, but only as a difference to the PRE form (below).
* residual_after_rounding -- the residual (PLAIN, PRE) or x_in (POST) added after the rounding to 16 bits: off by half a 16-bit
  ulp of the rounded part, 2.4e-4 .. 4.9e-4 of an O(1) value in fp16.  POST: against the stage bound (1e-5), both types.  PLAIN,
  PRE: against the chain's bound, which at N(0, 1 / 4C) weights is as large (above); asserted on the "_small_w2" families, whose
  FeedForward part is 1 / 64 of the sum (its ties with it) and whose b2 is O(1) -- PLAIN at both widths, PRE at C = 64.
* stats_slices_swapped -- the two 64-row statistics slices of a workgroup exchanged: rows carry an offset per 64-row slice, so the
  sums differ by 64 x the offset's difference.  POST with statistics.

The PRE chain: none of its intermediates is exposed and its t1 carries a GEMM's fp32 error into the LayerNorm, so more ln
operands sit within reach of a tie than in PLAIN; ln_var_cm1 (3.9e-3 of t at C = 128) is asserted there at C = 64 only.
POST is checked against the stage bound behind the PRE form's own fp32 output (``t3_from``): 10x to 100x tighter than the chain's,
and it refuses every defect of the list -- those of code the two forms share show as a difference only if one form has them, so for
shared code the PRE chain's bound is the guard, with the limits stated above.

Not asserted in bf16: ln_var_cm1 at C = 320 (LayerNorm family) and ln_one_pass.  Not asserted in fp16: t1_rounded16 on PRE.
Everything else is asserted in both types."""
import math

import pytest
import torch

import transformer_model as tm
from kernel_bounds import (as_16bit, colstats_ref_and_bound, ffn_ref_and_bound, gn_apply_ref_and_bound, gn_cols_ref_and_bound,
                           gn_stats_ref_and_bound, layernorm_ref_and_bound, linear_small_ref_and_bound, rnd, st_front_qkv_ref_and_bound,
                           st_front_t0_ref_and_bound)
from vface_amd import packing

DTS = [torch.float16, torch.bfloat16]
F16, BF16 = DTS


def ratio(got, ref, b):
    got = got.double()
    if not bool(torch.isfinite(got).all()):
        return float("inf")
    assert bool((b > 0).all()) and bool(torch.isfinite(b).all())
    return float(((got - ref).abs() / b).max())


def check(name, dt, run, want):
    """``run(defect) -> worst err / bound``; the model inside, every defect of ``want`` outside."""
    r = run(None)
    print(f"{name} {dt}: model worst err / bound {r:.3f}")
    assert r <= 1.0, (name, r)
    for d in tm.DEFECTS:
        r = run(d)
        if r is None:
            continue
        print(f"{name} {dt} defect {d}: worst err / bound {r:.3g}")
        if d in want:
            assert r > 1.0, (name, d, r)


# ------------------------------------------------------------------------------------------------ LayerNorm
LN_FAMILIES = {"ln_c64": dict(C=64, offset=0.0, spread=1.0), "ln_c320": dict(C=320, offset=8.0, spread=1.0),
               "ln_c520_16bit": dict(C=520, offset=0.0, spread=1.0, in16=True), "ln_offset64": dict(C=320, offset=64.0, spread=1.0),
               "ln_sqrt_eps": dict(C=320, offset=0.0, spread=math.sqrt(1e-5)), "ln_constant_row": dict(C=320, offset=3.0, spread=0.0)}


def ln_expect(name, dt):
    want = {"ln_half_lanes"}
    if name == "ln_constant_row":
        return set()                               # nothing to take statistics of: every form gives beta
    if name == "ln_c64" or dt == F16:
        want.add("ln_var_cm1")
    if name == "ln_sqrt_eps":
        want.add("ln_no_eps")
    if name == "ln_offset64" and dt == F16:
        want.add("ln_one_pass")
    return want


def ln_inputs(f, dt, seed=1):
    C = f["C"]
    x = rnd((77, C), seed, torch.float32, f["spread"]) + f["offset"]
    if f.get("in16"):
        x = x.to(dt)
    return x, 1.0 + rnd((C,), seed + 1, torch.float32, 0.2), rnd((C,), seed + 2, torch.float32, 0.2)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("family", list(LN_FAMILIES))
def test_layernorm_bound_admits_the_model_and_refuses_each_defect(dt, family):
    x, g, b = ln_inputs(LN_FAMILIES[family], dt)
    ref, bound = layernorm_ref_and_bound(x, g, b, 1e-5, dt)
    check(family, dt, lambda d: ratio(tm.layernorm_model(x, g, b, 1e-5, dt, d), ref, bound) if d is None or d in tm.LN_DEFECTS else None,
          ln_expect(family, dt))


# ------------------------------------------------------------------------------------------------ GroupNorm
GN_FAMILIES = {"cpg1": dict(C=32, groups=32, hw=130), "cpg3": dict(C=96, groups=32, hw=257), "cpg10": dict(C=320, groups=32, hw=130),
               "cpg65": dict(C=2080, groups=32, hw=100), "cpg8": dict(C=256, groups=32, hw=257), "cpg1_64": dict(C=64, groups=64, hw=7)}


def gn_input(f, dt, in32, ms=4.0, nimg=3):
    """Images differ in mean and scale, groups in mean; mean / spread up to ``ms``."""
    C, hw = f["C"], f["hw"]
    scale = torch.tensor([1.0, 0.5, 2.0])[:nimg, None, None]
    grp = (torch.arange(C) // max(C // f["groups"], 1) % 5 - 2.0)[None, None, :] * (ms / 2.0)
    x = (rnd((nimg, hw, C), 5, torch.float32) + grp) * scale
    return x if in32 else x.to(dt)


def gn_expect(f):
    cpg = f["C"] // f["groups"]
    want = set()
    if cpg % 8:
        want.add("gn_chunk_group")                 # (cpg = 1: a chunk of 8 channels is 8 groups)
    if f["hw"] > 128 and f["hw"] % 128:
        want.add("gn_tail_pixels")
    return want


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("in32", [True, False])
@pytest.mark.parametrize("family", list(GN_FAMILIES))
def test_groupnorm_stats_and_apply_bounds(dt, in32, family):
    f = GN_FAMILIES[family]
    x = gn_input(f, dt, in32)
    g, b = 1.0 + rnd((f["C"],), 6, torch.float32, 0.3), rnd((f["C"],), 7, torch.float32, 0.2)
    for eps in (1e-5, 1e-6):
        ref, bound = gn_stats_ref_and_bound(x, f["groups"], eps)
        check(f"gn stats {family} eps={eps}", dt,
              lambda d: ratio(tm.gn_stats_model(x, f["groups"], eps, d), ref, bound) if d is None or d in tm.GN_DEFECTS else None, gn_expect(f))
    st = tm.gn_stats_model(x, f["groups"], 1e-5)
    for silu in (False, True):
        ref, bound = gn_apply_ref_and_bound(x, st, g, b, f["groups"], silu, dt)
        check(f"gn apply {family} silu={silu}", dt,
              lambda d: ratio(tm.gn_apply_model(x, st, g, b, f["groups"], silu, dt, d), ref, bound) if d in (None, "gn_chunk_group") else None,
              gn_expect(f) - {"gn_tail_pixels"})


def cols_of(x32):
    """Per-64-row (sum, sum of squares) in fp32 of ``x32 [nimg, hw, C]`` -> ``[nimg hw / 64, C, 2]``."""
    nimg, hw, C = x32.shape
    sl = x32.reshape(nimg * hw // 64, 64, C)
    return torch.stack([sl.sum(1), (sl * sl).sum(1)], -1)


@pytest.mark.parametrize("cpg", [1, 3, 10, 65, 8])
@pytest.mark.parametrize("hw", [64, 128])
def test_groupnorm_cols_bounds(cpg, hw):
    groups, nimg = 32, 3
    C = cpg * groups
    f = dict(C=C, groups=groups, hw=hw)
    cs = cols_of(gn_input(f, F16, True))
    cs[0:hw // 64, :cpg, 0] = 64 * 1.5
    cs[0:hw // 64, :cpg, 1] = 64 * 2.25                              # group 0 of image 0: zero variance
    cs[0:hw // 64, cpg:2 * cpg, 0] = 64 * 1.1
    cs[0:hw // 64, cpg:2 * cpg, 1] = 64 * 1.2099999                  # group 1: fp32 sums that give a slightly negative variance
    g, b = 1.0 + rnd((C,), 6, torch.float32, 0.3), rnd((C,), 7, torch.float32, 0.2)
    for eps in (1e-5, 1e-6):
        st, stb, ab, abb = gn_cols_ref_and_bound(cs, nimg, hw, groups, eps, g, b)
        assert float(st[0, 1, 1]) == 1.0 / math.sqrt(eps), "the negative variance is clamped"

        def run(d):
            if d not in (None, "gn_chunk_group"):
                return None
            mst, mab = tm.gn_cols_model(cs, nimg, hw, groups, eps, g, b, d)
            return max(ratio(mst, st, stb), ratio(mab, ab, abb))
        check(f"gn cols cpg={cpg} hw={hw} eps={eps}", F16, run, {"gn_chunk_group"} if cpg % 8 else set())


# ------------------------------------------------------------------------------------------------ linear_small
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("silu,f32out", [(False, False), (True, False), (False, True), (True, True)])
def test_linear_small_bound_admits_the_model(dt, silu, f32out):
    a, w, bias = rnd((33, 640), 1, dt), rnd((96, 640), 2, dt, 1 / math.sqrt(640)), rnd((96,), 3, torch.float32)
    ref, bound = linear_small_ref_and_bound(a, w, dt, bias, silu, f32out)
    assert ratio(tm.linear_small_model(a, w, dt, bias, silu, f32out), ref, bound) <= 1.0
    shifted = tm.linear_small_model(a, w, dt, bias.roll(4), silu, f32out)          # (gemm_model's bias_lane_shift, whole vector)
    assert ratio(shifted, ref, bound) > 1.0


# ------------------------------------------------------------------------------------------------ the fused chains
def image_rows(M, hw, C, seed):
    """Token rows whose images differ in mean and scale and whose 64-row slices carry an offset of their own."""
    img = torch.arange(M) // hw
    x = rnd((M, C), seed, torch.float32) * (1.0 + 0.5 * (img % 3))[:, None] + (0.7 * (img % 3) - 0.5)[:, None]
    return x + (0.25 * ((torch.arange(M) // 64) % 4))[:, None]


def chain_weights(C, dt, small_w2=False):
    k = dict(gamma=1.0 + rnd((C,), 33, torch.float32, 0.2), beta=rnd((C,), 34, torch.float32, 0.2), eps=1e-5,
             w1=rnd((8 * C, C), 35, dt, C ** -0.5), b1=rnd((8 * C,), 36, torch.float32, 0.3),
             w2=rnd((C, 4 * C), 37, dt, (4 * C) ** -0.5), b2=rnd((C,), 38, torch.float32, 0.3))
    k["b1"][4 * C:] = torch.linspace(-8.0, 8.0, 4 * C)              # gates over [-8, 8]
    if small_w2:                                                     # the FeedForward's own part 1 / 64 of the sum, its bias O(1)
        k["w2"], k["b2"] = (k["w2"].float() / 64).to(dt), rnd((C,), 38, torch.float32, 1.0)
    return k


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("C", [64, 128])
def test_st_front_bounds(dt, C):
    M, hw = 384, 128
    x = image_rows(M, hw, C, 21)
    g, b = 1.0 + rnd((C,), 26, torch.float32, 0.3), rnd((C,), 27, torch.float32, 0.2)
    _, ab = tm.gn_cols_model(cols_of(x.reshape(M // hw, hw, C)), M // hw, hw, 32, 1e-6, g, b)
    w_in, b_in, w_p = rnd((C, C), 23, dt, C ** -0.5), rnd((C,), 24, torch.float32, 0.1), rnd((3 * C, C), 25, dt, C ** -0.5)
    lg, lb = 1.0 + rnd((C,), 28, torch.float32, 0.3), rnd((C,), 29, torch.float32, 0.2)
    wcat = packing.pack_st_front(w_in, w_p)
    t0r, t0b = st_front_t0_ref_and_bound(x, ab, hw, w_in, b_in, dt)

    def run(d):
        if d in tm.GN_DEFECTS or d in ("rowbias_sample0", "geglu_mispaired", "t1_rounded16", "residual_after_rounding", "stats_slices_swapped",
                                       "ln_no_eps", "ln_one_pass"):
            return None
        t0, ln, qkv = tm.st_front_model(x, ab, hw, wcat, b_in, lg, lb, 1e-5, dt, d)
        r0 = ratio(t0, t0r, t0b)
        if r0 > 1.0:
            return r0                                                 # (later stages are checked against the device's t0)
        lr, lbd, qr, qb = st_front_qkv_ref_and_bound(t0, lg, lb, 1e-5, w_p, dt, ln=ln)
        _, _, qr2, qb2 = st_front_qkv_ref_and_bound(t0, lg, lb, 1e-5, w_p, dt)
        return max(r0, ratio(ln, lr, lbd), ratio(qkv, qr, qb), ratio(qkv, qr2, qb2))
    check(f"st_front C={C}", dt, run, {"k_unpermuted", "image0_ab", "ln_half_lanes", "ln_var_cm1"} - ({"ln_var_cm1"} if (C, dt) == (128, BF16) else set()))


def ffn_case(form, C, dt):
    M, rps = 384, 128
    kw = chain_weights(C, dt, form.endswith("_small_w2"))
    form = form.replace("_small_w2", "")
    ref_kw, mod_kw = dict(kw), dict(gamma=kw["gamma"], beta=kw["beta"], eps=kw["eps"], b2=kw["b2"])
    w1p, mod_kw["b1p"] = packing.pack_geglu(kw["w1"], kw["b1"])
    mod_kw["w2p"] = packing.pack_ffn_w2(kw["w2"])
    if form == "plain":
        x = image_rows(M, rps, C, 31)
        ref_kw["x32"] = mod_kw["x32"] = x
        mod_kw["w1p"] = w1p
        return ref_kw, mod_kw
    att, resid = rnd((M, C), 41, dt, 0.8), image_rows(M, rps, C, 42)
    wo, bo, rb = rnd((C, C), 44, dt, C ** -0.5), rnd((C,), 45, torch.float32, 0.2), rnd((M // rps, C), 46, torch.float32, 0.5)
    ref_kw.update(att=att, wo=wo, bo=bo, rowbias=rb, rows_per_sample=rps, resid=resid)
    mod_kw.update(att=att, bo=bo, rowbias=rb, rows_per_sample=rps, resid=resid, w1p=None)
    if form == "pre":
        mod_kw["w_stream"] = packing.pack_attn_out_ffn(wo, w1p)
        return ref_kw, mod_kw
    wpo, b_po, x_in = rnd((C, C), 47, dt, C ** -0.5), rnd((C,), 48, torch.float32, 0.2), image_rows(M, rps, C, 49)
    ref_kw.update(wpo=wpo, b_po=b_po, x_in=x_in)
    mod_kw.update(w_stream=packing.pack_attn_out_ffn(wo, w1p, wpo), b_po=b_po, x_in=x_in, want_stats=True)
    return ref_kw, mod_kw


_UP = {"k_unpermuted", "geglu_mispaired", "ln_half_lanes", "ln_var_cm1"}
FFN_EXPECT = {"plain": _UP, "pre": _UP | {"rowbias_sample0", "t1_rounded16"},
              "plain_small_w2": {"residual_after_rounding"}, "pre_small_w2": {"residual_after_rounding", "rowbias_sample0"},
              "post": _UP | {"residual_after_rounding", "rowbias_sample0", "t1_rounded16", "stats_slices_swapped"}}


def ffn_expect(form, C, dt):
    """What the module docstring argues for: the PRE chain's subtle defects at C = 64 only, t1_rounded16 there in bf16 only."""
    want = set(FFN_EXPECT[form])
    if form.startswith("pre") and C > 64:
        want -= {"ln_var_cm1", "t1_rounded16", "residual_after_rounding"}
    if form == "pre" and dt == F16:
        want -= {"t1_rounded16"}
    return want


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("C", [64, 128])
@pytest.mark.parametrize("form", list(FFN_EXPECT))
def test_ffn_bounds(dt, C, form):
    """PLAIN and PRE against the whole chain's bound.  POST against the stage bound behind the PRE form's fp32 output of the same
    inputs (``t3_from``: the correct PRE model stands for the sibling launch), and the correct model inside the chain's bound too."""
    ref_kw, mod_kw = ffn_case(form, C, dt)
    M = (ref_kw["x32"] if "x32" in ref_kw else ref_kw["att"]).shape[0]
    slices = [torch.arange(s, s + 64) for s in range(0, M, 64)]
    if form == "post":
        pre_kw = {k: v for k, v in mod_kw.items() if k not in ("b_po", "x_in", "want_stats")}
        pre_kw["w_stream"] = mod_kw["w_stream"][:9 * C]
        pre32 = tm.ffn_model(dt, **pre_kw)[0]
        ref, e = ffn_ref_and_bound(dt, t3_from=pre32, **ref_kw)
        cref, ce = ffn_ref_and_bound(dt, **ref_kw)
        good = tm.ffn_model(dt, **mod_kw)
        r = ratio(good[0], cref, ce)
        print(f"ffn post C={C} {dt}: model against the whole chain's bound {r:.3f}; the chain's bound / the stage's, median {float((ce / e).median()):.0f}")
        assert r <= 1.0
    else:
        ref, e = ffn_ref_and_bound(dt, **ref_kw)
    b32, b16 = e, as_16bit(ref, e, dt)

    def run(d):
        if d in tm.GN_DEFECTS or d in ("image0_ab", "ln_no_eps", "ln_one_pass") or (form.startswith("plain") and d in ("rowbias_sample0", "t1_rounded16")) \
                or (d == "stats_slices_swapped" and form != "post"):
            return None
        out = tm.ffn_model(dt, defect=d, **mod_kw)
        r = max(ratio(out[0], ref, b32), ratio(out[1], ref, b16))
        if form == "post":
            cr, cb = colstats_ref_and_bound(out[0], slices)
            r = max(r, ratio(out[2], cr, cb))
        return r
    check(f"ffn {form} C={C}", dt, run, ffn_expect(form, C, dt))


def test_every_defect_is_refused_somewhere():
    seen = {"gn_chunk_group", "gn_tail_pixels", "image0_ab"}
    for name in LN_FAMILIES:
        seen |= ln_expect(name, F16)
    for form in FFN_EXPECT:
        seen |= ffn_expect(form, 64, BF16)
    assert seen == set(tm.DEFECTS)
