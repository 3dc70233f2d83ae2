"""``vface_amd.clip.ClipEngine`` and the conditioning stage of the ``LatentDiffusion`` mirror on the MI355X against the reference's own
outputs (tests/golden/clip.npz: ``FrozenCLIPEmbedder`` run on the CPU in double precision, make_clip_golden.py).

Tolerance: rel-L2(engine, double run) <= 1.25 x rel-L2(tests/clip_model.py, double run) -- the CPU emulation of this engine's
rounding points on the same inputs, computed here BEFORE the GPU result is looked at; 1.25 is the margin smoke.py and the bf16 UNet
test use over their emulations.  test_clip_bound_cpu.py holds the emulation itself against the reference: it may not exceed the error
of the reference's own autocast run, and one-line defects of it land past this tolerance.  ``tiny`` is checked at every recorded
intermediate so a failure names its layer, ``wide`` (257 tokens, the production GEMM shapes) at the output.  Measured values: DESIGN 9."""
import functools

import pytest
import torch

import clip_model as cm
from clip_model import cc          # tests/golden/cases_clip.py
from conftest import load_golden
from kernel_bounds import same_bits

pytestmark = pytest.mark.gpu

DEV = "cuda"
DTS = [torch.float16, torch.bfloat16]


@functools.lru_cache(maxsize=None)
def _case(name):
    """(cfg, fp32 state dict, frames, fixture) of a configuration: built once, shared, never modified."""
    return cm.engine_cfg(name), cm.synth_weights(name), torch.from_numpy(cc.frames(name)), load_golden("clip")


@functools.lru_cache(maxsize=None)
def _emulated(name, dt):
    cfg, sd, frames, _ = _case(name)
    taps = {}
    return cm.encode_from_frames(sd, cfg, dt, frames, taps=taps), taps


@functools.lru_cache(maxsize=None)
def _engine(name, dt):
    from vface_amd.clip import ClipEngine
    cfg, sd, _, _ = _case(name)
    return ClipEngine(sd, cfg, dt, DEV)


def _assert_close(got, emulated, ref64, what):
    bound = cm.MARGIN * cm.rel_l2(emulated, ref64)
    err = cm.rel_l2(got.float().cpu(), ref64)
    print(f"{what}: rel-L2 engine {err:.3e} emulation {bound / cm.MARGIN:.3e} bound {bound:.3e}")
    assert bool(torch.isfinite(got.float()).all()) and err <= bound, (what, err, bound)


@pytest.mark.parametrize("dt", DTS)
def test_tiny_engine_at_every_recorded_intermediate(dt):
    cfg, sd, frames, z = _case("tiny")
    emu, emu_taps = _emulated("tiny", dt)                             # the tolerance exists before the engine runs
    taps = {}
    got = _engine("tiny", dt).encode_from_frames(frames.to(DEV), taps=taps)
    torch.cuda.synchronize()
    for k in cc.INTERMEDIATES:
        ref = z[f"tiny.{k}"]
        _assert_close(taps[k].reshape(ref.shape), emu_taps[k].reshape(ref.shape), ref, f"tiny {dt} {k}")
    _assert_close(got, emu, z["tiny.e64"], f"tiny {dt} E")


@pytest.mark.parametrize("dt", DTS)
def test_wide_engine_at_the_output(dt):
    cfg, sd, frames, z = _case("wide")
    emu, _ = _emulated("wide", dt)
    got = _engine("wide", dt).encode_from_frames(frames.to(DEV))
    assert got.shape == (cc.BATCH, 1, cc.PROJ) and got.dtype == dt
    _assert_close(got, emu, z["wide.e64"], f"wide {dt} E")


@pytest.mark.parametrize("name", ["tiny", "wide"])
def test_batch_independence_one_frame_against_three(name):
    """A frame's E does not depend on the batch it is launched in: B = 1 against B = 3, bit for bit, for every frame."""
    cfg, sd, frames, _ = _case(name)
    eng = _engine(name, torch.float16)
    three = torch.cat([frames, frames[:1].flip(-1)]).to(DEV)
    whole = eng.encode_from_frames(three)
    for i in range(3):
        assert same_bits(eng.encode_from_frames(three[i:i + 1]).cpu(), whole[i:i + 1].cpu()), f"{name}: frame {i}"


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("masked", [False, True])
def test_encode_from_frames_is_encode_on_the_prep_kernels_own_output(dt, masked):
    """The fused path (resize inside the patch gather) and the two-step path (the prepared image handed to ``encode``) are the same
    launches behind the patch matrix: E is bit-identical when ``encode`` is given the prep kernel's own image."""
    cfg, sd, frames, _ = _case("tiny")
    eng = _engine("tiny", dt)
    B, S, G = frames.shape[0], cfg["image"], cfg["image"] // 14
    mask = None
    if masked:
        mask = (torch.rand(B, 1, *frames.shape[2:], generator=torch.Generator().manual_seed(2)) > 0.5).float().to(DEV)
    a0 = eng.patches(frames.to(DEV), prep=True, mask=mask)
    img = torch.nn.functional.fold(a0[:, :588].float().view(B, G * G, 588).transpose(1, 2), (S, S), 14, stride=14)   # un-patchify: exact
    assert same_bits(eng.encode(img).cpu(), eng.encode_from_frames(frames.to(DEV), mask).cpu())


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("shared_source", [True, False])
def test_conditioning_with_feat_through_latent_diffusion(dt, shared_source):
    """``LatentDiffusion(cond_stage_config=...)`` loads a checkpoint-style state dict (``cond_stage_model.*`` with the reference's
    unused keys, the four projections) and ``conditioning_with_feat`` returns the shipped mix.  Reference: the ten lines of
    ddpm.py:901-915, 1009-1039 restated in fp64 (``clip_model.conditioning64``; the reference's module cannot be imported without
    pytorch_lightning, dlib and torchvision) on the fixture's double-run E; tolerance: 1.25 x the same mix of the emulated E with
    16-bit operands."""
    from vface_amd.ldm.models.diffusion.ddpm import LatentDiffusion
    cfg, sd, frames, z = _case("tiny")
    tiny_unet = dict(image_size=8, in_channels=9, out_channels=4, model_channels=32, attention_resolutions=[4, 2, 1], num_res_blocks=1,
                     channel_mult=[1, 2, 4, 4], num_heads=8, use_spatial_transformer=True, transformer_depth=1, context_dim=768,
                     use_checkpoint=True, legacy=False)
    ldm = LatentDiffusion(tiny_unet, cond_stage_config=dict(params=dict(vision_config=cfg, compute_dtype=dt)))
    mix = cm.mix_weights()
    ckpt = {**ldm.state_dict(), **{"cond_stage_model." + k: v for k, v in sd.items()}, **mix,
            "cond_stage_model.model.logit_scale": torch.zeros(()), "cond_stage_model.final_ln.weight": torch.zeros(1024)}
    ldm.load_state_dict(ckpt)
    ldm = ldm.to(DEV)
    id_feat, landmarks = (torch.from_numpy(a) for a in cc.side_inputs())
    B = frames.shape[0]
    e64 = z["tiny.e64"]
    emu, _ = _emulated("tiny", dt)
    src = slice(0, 1) if shared_source else slice(0, B)
    r = lambda t: t.to(dt).float()
    ref = cm.conditioning64(e64[src], e64, id_feat, landmarks, mix)
    emulated = cm.conditioning64(emu[src], emu, r(id_feat), r(landmarks), {k: (r(v) if k.endswith("weight") else v) for k, v in mix.items()}).float()
    x = torch.from_numpy(cm.prep32(frames, cfg["image"]).numpy())[src].to(DEV)           # the source image: already resized and normalised
    got = ldm.conditioning_with_feat(x, landmarks=landmarks.to(DEV), tar=frames.to(DEV), id_feat=id_feat.to(DEV))
    assert got.shape == (B, 1, 768) and got.dtype == torch.float32
    _assert_close(got, emulated, ref, f"conditioning_with_feat {dt} shared_source={shared_source}")
    enc = ldm.cond_stage_model
    again = ldm.conditioning_with_feat(None, landmarks=landmarks.to(DEV), id_feat=id_feat.to(DEV), e_src=enc.encode(x),
                                       e_tar=enc.encode_from_frames(frames.to(DEV)))
    assert same_bits(again.cpu(), got.cpu()), "E handed in: the same launches"
