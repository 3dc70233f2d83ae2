"""The GEMM and convolution bounds' own test, no GPU: ``kernel_bounds.gemm_ref_and_bound`` / ``conv_ref_and_bound`` must admit the CPU
model of the kernels' rounding points (``gemm_model`` / ``conv_model``) on EVERY element of every family, in both types, and must
refuse each seeded one-line defect on the families meant to expose it.  That is what shows that test_gemm_conv_gpu.py can fail.
The only threshold is 1 (error / bound).  Inputs are N(0, 1) operands against N(0, 1 / K) weights, so an output is O(1) and its
bound about half a unit in the last place (5e-4 in fp16, 4e-3 in bf16); which defect shows where is reasoned, not fitted:

* k_tail_dropped -- the last K % 64 columns ignored: 8 of K columns carry sqrt(8 / K) of an output's spread -- 0.24 at K = 136,
  0.085 at K = 1096 (the case a rel-L2 of 1e-3 lets through), 20x a bf16 half-ulp.  Every family with K % 64 != 0.
* row_tail -- the last row of an M tail keeps its neighbour's value: off by the difference of two independent O(1) rows.  Every
  family with M % 128 != 0.
* bias_lane_shift -- one lane group reads its four biases 4 columns on: off by the difference of two N(0, 1) biases on a quarter
  of the columns.  Every family with a bias.
* rowbias_tile_sample -- a 128-row tile takes the row bias of its first row's sample: off by the difference of two N(0, 1) row
  biases on the rows of every later sample of the tile.  The families whose tiles straddle samples (100 and 16 rows per sample).
* residual_after_rounding -- round(round(t) + r) against round(t + r): the first rounding is off by up to half an ulp of t, the
  second by up to half an ulp of the sum; where the two have one sign and t is not smaller than the sum they add up to a whole
  ulp against a bound of half an ulp + e32, and e32 ~ K U32 is 100x (fp16) to 1000x (bf16) below an ulp.  Over 14400 elements
  that alignment occurs in both types, so both are asserted ("tails": 16-bit residual, O(1) like the sum).
* acc16 -- the accumulator rounded to 16 bits after every K tile: T tiles add up to T u |acc|, and the last of these roundings
  comes BEFORE the epilogue's addends (a residual_after_rounding of the bias), against half an ulp of the output + e32.  Asserted
  where a bias, row bias or residual follows (3 tiles) and at K = 1096 (18 tiles: ~2.4 u |acc| rms, 4 sigma over 20000 elements).
  Not asserted at K = 1544 in fp16: e32 = (K + 8) U32 A is a worst case linear in K and there reaches 4x the fp16 half-ulp, so
  the margin thins with K (the price of a bound no summation order can exceed).
* geglu_swapped -- value and gate exchanged: another function of the inputs altogether; the GEGLU family.
* pad_wraps -- a left / right padding tap reads the last / first pixel of the neighbouring row: with the constant 1.0 added to x
  the wrongly read pixel contributes ~ w (1 + N(0, 1)) per channel where a zero belongs.  Every convolution family wider than a pixel.
* pad_trailing_as_symmetric -- (0, 1, 0, 1) padding run as (1, 1, 1, 1): every output reads a window one pixel up and left;
  the trailing-padding families.
* stride2_odd -- the last output row / column of a stride-2 convolution at odd size starts one pixel early; the odd stride-2 family.

Nothing stays unrefused in bf16: every defect above is asserted in both types."""
import math

import pytest
import torch

from gemm_model import DEFECTS, conv_model, gemm_model
from kernel_bounds import conv_ref_and_bound, gemm_ref_and_bound, rnd

DTS = [torch.float16, torch.bfloat16]


def _gemm_family(name, dt):
    """-> (kwargs of gemm_ref_and_bound / gemm_model, a, w)"""
    M, N, K, kw = {"tails": (200, 72, 136, dict(bias=True, residual=True)),
                   "rowbias": (400, 136, 72, dict(bias=True, rowbias=100)),
                   "long_k": (64, 320, 1096, dict(bias=True)),
                   "split3": (64, 320, 1544, dict(rowbias=16, residual=True, splits=3)),
                   "split2_tail": (200, 320, 1096, dict(bias=True, splits=2)),
                   "out_f32": (129, 12, 72, dict(bias=True, out_f32=True)),
                   "res32_out32": (130, 72, 64, dict(bias=True, residual32=True, out_f32=True)),
                   "geglu": (130, 128, 64, dict(bias=True, geglu=True))}[name]
    a, w = rnd((M, K), 1, dt), rnd((N, K), 2, dt, 1 / math.sqrt(K))
    args = dict(out_f32=kw.get("out_f32", False), splits=kw.get("splits", 1), geglu=kw.get("geglu", False))
    if kw.get("bias"):
        args["bias"] = rnd((N,), 3, torch.float32)
        if args["geglu"]:                              # gates from -8 to 8: both branches of gelu_erf_f and its deep negative tail
            args["bias"][N // 2:] = torch.linspace(-8.0, 8.0, N // 2)
    if kw.get("rowbias"):
        args["rows_per_sample"] = kw["rowbias"]
        args["rowbias"] = rnd((M // kw["rowbias"], N), 4, torch.float32)
    if kw.get("residual"):
        args["residual"] = rnd((M, N), 5, dt)
    if kw.get("residual32"):
        args["residual"] = rnd((M, N), 5, torch.float32)
    return args, a, w


GEMM_EXPECT = {"tails": {"k_tail_dropped", "row_tail", "bias_lane_shift", "residual_after_rounding", "acc16"},
               "rowbias": {"k_tail_dropped", "row_tail", "bias_lane_shift", "rowbias_tile_sample", "acc16"},
               "long_k": {"k_tail_dropped", "bias_lane_shift", "acc16"},
               "split3": {"k_tail_dropped", "rowbias_tile_sample"},
               "split2_tail": {"k_tail_dropped", "row_tail", "bias_lane_shift", "acc16"},
               "out_f32": {"k_tail_dropped", "row_tail", "bias_lane_shift"},
               "res32_out32": {"row_tail", "bias_lane_shift"},
               "geglu": {"geglu_swapped", "row_tail"}}

CONV_FAMILIES = {"s1": dict(cin=8, cout=8, H=7, W=6), "s1_fast": dict(cin=64, cout=72, H=3, W=5),
                 "s2_odd": dict(cin=8, cout=8, H=7, W=5, stride=2), "s2_even": dict(cin=24, cout=8, H=6, W=6, stride=2),
                 "up": dict(cin=8, cout=8, H=3, W=5, upsample=True),
                 "trailing_even": dict(cin=8, cout=8, H=6, W=6, stride=2, pad=(0, 1, 0, 1)),
                 "trailing_odd": dict(cin=8, cout=8, H=7, W=5, stride=2, pad=(0, 1, 0, 1)),
                 "one_pixel": dict(cin=8, cout=8, H=1, W=1),
                 "gn_silu": dict(cin=64, cout=8, H=4, W=4, gn=True, silu=True), "gn": dict(cin=64, cout=8, H=4, W=4, gn=True),
                 "plus_1x1": dict(cin=64, cout=8, H=4, W=4, c2=64),
                 "phase": dict(cin=8, cout=8, H=4, W=5, window=2, pad=(1, 0, 0, 1))}
CONV_EXPECT = {"s1": {"pad_wraps"}, "s1_fast": {"pad_wraps"}, "s2_odd": {"pad_wraps", "stride2_odd"}, "s2_even": {"pad_wraps"},
               "up": {"pad_wraps"}, "trailing_even": {"pad_trailing_as_symmetric"}, "trailing_odd": {"pad_trailing_as_symmetric"},
               "one_pixel": set(), "gn_silu": {"pad_wraps"}, "gn": {"pad_wraps"}, "plus_1x1": {"pad_wraps"}, "phase": {"pad_wraps"}}


def _conv_family(name, dt):
    f = dict(CONV_FAMILIES[name])
    cin, cout, H, W, nimg, win = f.pop("cin"), f.pop("cout"), f.pop("H"), f.pop("W"), 3, f.pop("window", 3)
    x = (rnd((nimg, cin, H, W), 1, dt).float() + 1.0).to(dt)       # the constant makes every border tap count
    w = rnd((cout, cin, win, win), 2, dt, 1 / math.sqrt(win * win * cin))
    args = dict(stride=f.get("stride", 1), upsample=f.get("upsample", False), pad=f.get("pad", (1, 1, 1, 1)),
                bias=rnd((cout,), 3, torch.float32), rowbias=rnd((nimg, cout), 4, torch.float32))
    if f.get("gn"):
        args["scale_shift"] = torch.stack([1 + 0.3 * rnd((nimg, cin), 6, torch.float32), 0.5 + 0.3 * rnd((nimg, cin), 7, torch.float32)], -1)
        args["silu"] = f.get("silu", False)
    if f.get("c2"):
        args["x2"], args["w2"] = rnd((nimg * H * W, f["c2"]), 8, dt), rnd((cout, f["c2"]), 9, dt, 1 / math.sqrt(f["c2"]))
    return args, x, w


def worst_ratio(got, ref, b):
    got = got.double()
    if not bool(torch.isfinite(got).all()):
        return float("inf")
    return float(((got - ref).abs() / b).max())


def _run(kind, family, dt, ref_fn, model_fn, args, x, w, want):
    ref, b = ref_fn(x, w, dt, **args)
    assert bool((b > 0).all()) and bool(torch.isfinite(b).all())
    r = worst_ratio(model_fn(x, w, dt, **args), ref, b)
    print(f"{kind} {family} {dt}: model worst err / bound {r:.3f}")
    assert r <= 1.0, r
    for d in DEFECTS:
        r = worst_ratio(model_fn(x, w, dt, defect=d, **args), ref, b)
        print(f"{kind} {family} {dt} defect {d}: worst err / bound {r:.3g}")
        if d in want:
            assert r > 1.0, (d, r)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("family", list(GEMM_EXPECT))
def test_gemm_bound_admits_the_model_and_refuses_each_defect(dt, family):
    args, a, w = _gemm_family(family, dt)
    _run("gemm", family, dt, gemm_ref_and_bound, gemm_model, args, a, w, GEMM_EXPECT[family])


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("family", list(CONV_FAMILIES))
def test_conv_bound_admits_the_model_and_refuses_each_defect(dt, family):
    args, x, w = _conv_family(family, dt)
    _run("conv", family, dt, conv_ref_and_bound, conv_model, args, x, w, CONV_EXPECT[family])


def test_every_defect_is_refused_somewhere():
    seen = set()
    for s in list(GEMM_EXPECT.values()) + list(CONV_EXPECT.values()):
        seen |= s
    assert seen == set(DEFECTS)


@pytest.mark.parametrize("dt", DTS)
def test_fp32_form_of_the_bound_refuses_what_the_16_bit_form_cannot_see(dt):
    """Where out32 is written the fp32 form applies (e32 + U32 |pre|, ~1e-5 here): a K tail, a shifted bias and a 16-bit
    accumulator are 100x to 10000x outside it; the 16-bit copy is then pinned bit for bit as out32.to(dt) by the GPU test."""
    args, a, w = _gemm_family("res32_out32", dt)
    ref, b = gemm_ref_and_bound(a, w, dt, **args)
    assert float(b.max()) < 1e-4
    assert worst_ratio(gemm_model(a, w, dt, defect="acc16", **args), ref, b) > 10.0
