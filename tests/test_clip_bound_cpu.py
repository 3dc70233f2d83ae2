"""What the conditioning stage's GPU tests rest on, without a GPU.

1. The per-element bounds of clip_bounds.py admit torch's own fp32 evaluation of each kernel and refuse one-line defects of it.
2. tests/clip_model.py -- the emulation whose error, times 1.25, is test_clip_gpu.py's tolerance -- against the reference's recorded
   outputs (tests/golden/clip.npz) at ``tiny``, ``wide`` and ``full``:
   * in fp32 it IS the reference's network: it reproduces the double run to fp32 rounding, at every recorded intermediate;
   * A CONDITION, NOT A MEASUREMENT: in fp16 and in bf16 its error may not exceed the error of the reference's own
     ``torch.autocast`` run (``e_ref16`` / ``e_ref_bf16``, read from the fixture): an engine that keeps the residual stream in fp32
     has to beat a run that rounds it at every layer;
   * each seeded one-line defect lands past the tolerance (1.25 x the clean emulation's error)."""
import functools

import pytest
import torch
import torch.nn.functional as F

import clip_bounds as cb
import clip_model as cm
from clip_model import cc          # tests/golden/cases_clip.py
from conftest import load_golden
from kernel_bounds import as_16bit, assert_within, rnd

DTS = [torch.float16, torch.bfloat16]


def _outside(got, ref, bound):
    return int(((got.double() - ref).abs() > bound).sum())


# ------------------------------------------------------------------------------------------------ 1: the per-element bounds
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("H,W", [(64, 48), (40, 40)])
def test_prep_bound_admits_aten_in_both_orders_and_refuses_defects(dt, H, W):
    S = 42
    img = cb.smooth_frames(2, H, W, seed=H + W)
    mask = (torch.rand(2, H, W, generator=torch.Generator().manual_seed(5)) > 0.6).float()
    m, s = cb.CLIP_MEAN.float().view(1, 3, 1, 1), cb.CLIP_STD.float().view(1, 3, 1, 1)
    resize = lambda t, **k: F.interpolate(t, (S, S), mode="bilinear", align_corners=False, **k)
    for mk in (None, mask):
        ref, bound = cb.prep_ref_and_bound(img, mk, S, dt)
        x = img if mk is None else img * (1.0 - mk)[:, None]
        u = (x + 1.0) / 2.0
        assert_within(resize((u - m) / s).to(dt), ref, bound, "normalise, then resize (ddpm.py:907-912)")
        assert_within(((resize(u) - m) / s).to(dt), ref, bound, "resize, then normalise (VFace_inference_batch.py:493-496)")
        n = ref.numel()
        assert _outside(resize((((x - m) / s) + 1.0) / 2.0).to(dt), ref, bound) > 0.9 * n, "mean / std before un_norm"
        assert _outside(F.interpolate((u - m) / s, (S, S), mode="bilinear", align_corners=True).to(dt), ref, bound) > 0.5 * n, "align_corners"
        if H > S:
            assert _outside(resize((u - m) / s, antialias=True).to(dt), ref, bound) > 0.5 * n, "an antialiased resize"
        if mk is not None:
            assert _outside(resize(((img * mk[:, None] + 1.0) / 2.0 - m) / s).to(dt), ref, bound) > 0.3 * n, "mask instead of 1 - mask"
    for size, out in ((64, 42), (48, 42), (40, 42), (512, 224)):        # the integer restatement is ATen's fp32 index
        o = torch.arange(out, dtype=torch.float32)
        src = torch.clamp(torch.tensor(size / out, dtype=torch.float32) * (o + 0.5) - 0.5, min=0.0)
        assert torch.equal(src.long(), cb.source_index(size, out))


@pytest.mark.parametrize("dt", DTS)
def test_act_bound_admits_fp32_and_refuses_the_other_function(dt):
    v = torch.cat([rnd((64, 64), 1, dt, 3.0).flatten(), torch.linspace(-12, 12, 4096).to(dt), torch.tensor([0.0, -0.0]).to(dt)])
    f = v.float()
    quick, erf = (f * torch.sigmoid(1.702 * f)).to(dt), F.gelu(f).to(dt)
    for kind, good, other in ((0, quick, erf), (1, erf, quick)):
        ref, bound = cb.act_ref_and_bound(v, kind, dt)
        assert_within(good, ref, bound, f"act {kind}")
        assert _outside(other, ref, bound) > 0.25 * v.numel()
        assert _outside(F.gelu(f, approximate="tanh").to(dt), ref, bound) > (0.02 if kind else 0.25) * v.numel()


def test_embed_and_mix_bounds_admit_fp32_and_refuse_defects():
    B, P, C = 3, 9, 128
    tok, cls, pos = rnd((B * P, C), 1, torch.float16), rnd((C,), 2, torch.float32, 3.0), rnd((P + 1, C), 3, torch.float32, 0.5)
    gamma, beta = 1.0 + 0.1 * rnd((C,), 4, torch.float32), 0.1 * rnd((C,), 5, torch.float32)
    rows = torch.cat([cls.view(1, 1, C).expand(B, 1, C), tok.float().view(B, P, C)], 1) + pos[None]
    ref, bound = cb.embed_ref_and_bound(tok, cls, pos, B)
    assert_within(rows.reshape(-1, C), ref, bound, "embed")
    no_pos_on_class = rows.clone()
    no_pos_on_class[:, 0] = cls
    assert _outside(no_pos_on_class.reshape(-1, C), ref, bound) > 0.9 * B * C
    shifted = torch.cat([cls.view(1, 1, C).expand(B, 1, C), tok.float().view(B, P, C)], 1) + pos.roll(1, 0)[None]
    assert _outside(shifted.reshape(-1, C), ref, bound) > 0.9 * ref.numel()
    ref, bound = cb.embed_ref_and_bound(tok, cls, pos, B, gamma, beta)
    ln = F.layer_norm(rows, (C,), gamma, beta, 1e-5).reshape(-1, C)
    assert_within(ln, ref, bound, "embed + pre_layrnorm")
    assert _outside(ln.half().float(), ref, bound) > 0.5 * ref.numel(), "a stream that starts rounded to 16 bits"
    N = 768
    ops = [(rnd((5, N), 10, torch.float32), 1.0), (rnd((1, N), 11, torch.float32), 10.0), (rnd((5, N), 12, torch.float32), 0.05)]
    ref, e32 = cb.mix_ref_and_bound(ops, 5)
    got = (ops[0][0] * 1.0 + ops[1][0] * 10.0 + ops[2][0] * 0.05) / (1.0 + 10.0 + 0.05)
    assert_within(got, ref, e32, "mix")
    assert _outside(ops[0][0] * 1.0 + ops[1][0] * 10.0 + ops[2][0] * 0.05, ref, e32) > 0.9 * ref.numel(), "weight_division dropped"
    assert _outside((ops[0][0] * 1.0 + ops[1][0] * 10.0 + ops[2][0] * 0.05) / 11.0, ref, e32) > 0.9 * ref.numel(), "a weight left out of the sum"


# ------------------------------------------------------------------------------------------------ 2: the emulation
@functools.lru_cache(maxsize=None)
def _case(name):
    return cm.engine_cfg(name), cm.synth_weights(name), torch.from_numpy(cc.frames(name)), load_golden("clip")


@functools.lru_cache(maxsize=None)
def _clean(name, dt):
    cfg, sd, frames, z = _case(name)
    return cm.rel_l2(cm.encode_from_frames(sd, cfg, dt, frames), z[f"{name}.e64"])


@pytest.mark.parametrize("name", list(cc.CONFIGS))
def test_emulation_in_fp32_is_the_references_network(name):
    cfg, sd, frames, z = _case(name)
    taps = {}
    e = cm.encode_from_frames(sd, cfg, torch.float32, frames, taps=taps)
    assert cm.rel_l2(e, z[f"{name}.e64"]) < 5e-6 and cm.rel_l2(z[f"{name}.e32"], z[f"{name}.e64"]) < 5e-6
    if name == "tiny":
        for k in cc.INTERMEDIATES:
            assert cm.rel_l2(taps[k].reshape(z[f"tiny.{k}"].shape), z[f"tiny.{k}"]) < 5e-6, k


@pytest.mark.parametrize("dt,tag", [(torch.float16, "e_ref16"), (torch.bfloat16, "e_ref_bf16")])
@pytest.mark.parametrize("name", list(cc.CONFIGS))
def test_emulated_error_does_not_exceed_the_references_own_autocast_error(name, dt, tag):
    e_ref = float(_case(name)[3][f"{name}.{tag}"])
    err = _clean(name, dt)
    print(f"{name} {dt}: emulated {err:.3e}, reference autocast {e_ref:.3e}")
    assert 0.0 < err <= e_ref, (name, dt, err, e_ref)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("defect", cm.DEFECTS)
@pytest.mark.parametrize("name", ["tiny", "wide"])
def test_seeded_defects_land_past_the_tolerance(name, defect, dt):
    cfg, sd, frames, z = _case(name)
    bound = cm.MARGIN * _clean(name, dt)
    err = cm.rel_l2(cm.encode_from_frames(sd, cfg, dt, frames, defect=defect), z[f"{name}.e64"])
    print(f"{name} {dt} {defect}: {err:.3e} against a tolerance of {bound:.3e}")
    assert err > bound, (name, defect, dt, err, bound)


@pytest.mark.parametrize("dt", DTS)
def test_mix_restated_against_torch_linear(dt):
    """``clip_model.conditioning64`` is the ten lines of ddpm.py it restates: against ``nn.Linear`` modules and the reference's
    expression evaluated in fp32 torch, and the emulated operands stay within the 16-bit roundings of the fixture's E."""
    cfg, sd, frames, z = _case("tiny")
    mix = cm.mix_weights()
    id_feat, lm = (torch.from_numpy(a) for a in cc.side_inputs())
    e = z["tiny.e32"]
    lin = {n: torch.nn.Linear(*reversed(s)) for n, s in cm.MIX_LINEARS.items()}
    for n, l in lin.items():
        l.load_state_dict({"weight": mix[n + ".weight"], "bias": mix[n + ".bias"]})
    with torch.no_grad():
        c = lin["proj_out_source"](e[:1]) + lin["proj_out_target"](e)
        c2, l3 = lin["ID_proj_out"](id_feat).unsqueeze(1), lin["landmark_proj_out"](lm).unsqueeze(1)
        want = (c * 1.0 + c2 * 10.0 + l3 * 0.05) / (1.0 + 10.0 + 0.05)
    assert cm.rel_l2(want, cm.conditioning64(e[:1], e, id_feat, lm, mix)) < 2e-6
    r = lambda t: t.to(dt).float()
    emu = cm.encode_from_frames(sd, cfg, dt, frames)
    got = cm.conditioning64(emu[:1], emu, r(id_feat), r(lm), {k: (r(v) if k.endswith("weight") else v) for k, v in mix.items()})
    assert cm.rel_l2(got, cm.conditioning64(z["tiny.e64"][:1], z["tiny.e64"], id_feat, lm, mix)) < (2e-3 if dt == torch.float16 else 1.6e-2)
