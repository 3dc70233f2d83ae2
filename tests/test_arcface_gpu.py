"""``vface_amd.arcface.ArcFaceEngine``, the ``Backbone`` / ``IDLoss`` mirrors and ``LatentDiffusion.conditioning_with_feat`` on the
MI355X against the reference's own outputs (tests/golden/arcface.npz: ``Backbone`` and ``bottleneck_IR_SE`` run on the CPU in double
precision, make_arcface_golden.py).

Tolerance: rel-L2(engine, double run) <= 1.25 x rel-L2(tests/arcface_model.py, double run) -- the CPU emulation of this engine's
rounding points on the same inputs, computed here BEFORE the GPU result is looked at; 1.25 is the margin the conditioning encoder's
test uses over its emulation, for the same reason (the order of fp32 additions inside the MFMA tiles, which the emulation does not
restate).  test_arcface_bound_cpu.py holds the emulation itself against the reference: it may not exceed the error of the
reference's own 16-bit run, and one-line defects of it land past this tolerance.  Measured values: DESIGN 9."""
import pytest
import torch

import arcface_model as am
from arcface_model import ca
from conftest import load_golden
from kernel_bounds import same_bits

pytestmark = pytest.mark.gpu

DEV = "cuda"
DTS = [torch.float16, torch.bfloat16]
TINY_UNET = dict(image_size=8, in_channels=9, out_channels=4, model_channels=32, attention_resolutions=[4, 2, 1], num_res_blocks=1,
                 channel_mult=[1, 2, 4, 4], num_heads=8, use_spatial_transformer=True, transformer_depth=1, context_dim=768,
                 use_checkpoint=True, legacy=False)


def nhwc(x):
    N, C_, H, W = x.shape
    return x.permute(0, 2, 3, 1).reshape(N * H * W, C_).contiguous()


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("name", list(ca.UNIT_CASES))
def test_unit_against_the_reference(dt, name):
    """One ``bottleneck_IR_SE`` on a small odd map: the reference's own unit class in double, the engine's ``unit`` on the rounded
    input with its leading BatchNorm applied by ``vface_prelu``'s ``z`` output."""
    from vface_amd.arcface import ArcFaceEngine
    g = load_golden("arcface")
    sd, x, (cin, depth, stride, H, W, n) = am.unit_case(name)
    ref = g[f"{name}.out64"]
    tol = am.MARGIN * am.rel_l2(am.run_unit(sd, "u", x, cin, depth, stride, dt), ref)
    eng = ArcFaceEngine(None, dt, DEV)
    eng.add_unit({k: v.double() for k, v in sd.items() if torch.is_floating_point(v)}, "u", cin, depth, stride)
    xd = nhwc(x).to(dt).to(DEV)
    z = eng.lead_in("u", xd, M=n * H * W, C_=cin)
    y, zn, OH, OW = eng.unit("u", xd, z, nimg=n, H=H, W=W, cin=cin, depth=depth, stride=stride)
    torch.cuda.synchronize()
    assert zn is None and (OH, OW) == tuple(ref.shape[2:])
    got = y.cpu().double().reshape(n, OH, OW, depth).permute(0, 3, 1, 2)
    err = am.rel_l2(got, ref)
    print(f"unit {name} {dt}: rel-L2 {err:.3e}, tolerance {tol:.3e} (1.25 x the emulation); max abs {float((got - ref).abs().max()):.3e}, "
          f"the reference's own 16-bit run {float(g[name + ('.e_ref16' if dt == torch.float16 else '.e_ref_bf16')]):.3e}")
    assert bool(torch.isfinite(got).all()) and err <= tol


@pytest.fixture(scope="module")
def network():
    return {dt: _engine(dt) for dt in DTS}


def _engine(dt):
    from vface_amd.arcface import ArcFaceEngine
    return ArcFaceEngine(am.network().state_dict(), dt, DEV)


def _rows(x, dt):
    """The fixture's network input [B, 3, 112, 112] as the stem's token rows."""
    import arcface_bounds as ab
    return ab.rows8(x.float()).to(dt).to(DEV)


@pytest.mark.parametrize("dt", DTS)
def test_network_against_the_reference(network, dt):
    g = load_golden("arcface")
    tol = am.MARGIN * am.rel_l2(am.emulated(dt), g["feat64"])
    eng = network[dt]
    taps = {}
    got = eng.features(_rows(g["prep"], dt), 2, taps=taps).cpu()
    err = am.rel_l2(got, g["feat64"])
    e_ref = float(g["e_ref16" if dt == torch.float16 else "e_ref_bf16"])
    stds = [float(taps[f"body.{i}"].float().std()) for i in (0, 6, 20, 23)]
    print(f"network {dt}: rel-L2 {err:.3e}, tolerance {tol:.3e} (1.25 x the emulation), the reference's own 16-bit run {e_ref:.3e}; "
          f"unit output std at 0 / 6 / 20 / 23: {stds}; max |x| {max(float(t.float().abs().max()) for t in taps.values()):.2f}")
    assert got.dtype == torch.float32 and tuple(got.shape) == (2, 512) and bool(torch.isfinite(got).all())
    assert float((got.double().norm(dim=1) - 1).abs().max()) < 1e-5
    assert err <= tol
    # from the frames: vface_id_prep(prep=1) in front, the same tolerance (the chain's fp32 error is far below a 16-bit rounding)
    again = eng.extract_feats_from_frames(am.frames().to(DEV)).cpu()
    err2 = am.rel_l2(again, g["feat64"])
    print(f"network {dt} from the frames: rel-L2 {err2:.3e}")
    assert err2 <= tol


@pytest.mark.parametrize("dt", DTS)
def test_a_frame_does_not_depend_on_its_batch(network, dt):
    g = load_golden("arcface")
    eng = network[dt]
    x = torch.cat([g["prep"], g["prep"][:1].flip(3)])
    three = eng.features(_rows(x, dt), 3).cpu()
    one = eng.features(_rows(x[:1], dt), 1).cpu()
    assert same_bits(three[:1], one)
    assert not same_bits(three[2:3], one)


def test_mirrors_and_conditioning_with_feat():
    """``Backbone.forward``, ``IDLoss.extract_feats`` and ``LatentDiffusion.conditioning_with_feat(id_feat=None)`` are the engine;
    a given ``id_feat`` is used as it is; loading or casting drops the engine; a CPU tensor raises."""
    import clip_model as cm
    from vface_amd import hip
    from vface_amd.ldm.models.diffusion.ddpm import IDLoss, LatentDiffusion
    from vface_amd.utils import synth
    g = load_golden("arcface")
    dt = torch.float16
    x112 = g["prep"].float().to(DEV)
    net = am.network()
    sd = net.state_dict()
    idl = IDLoss(compute_dtype=dt)
    idl.facenet.load_state_dict(sd)
    idl = idl.to(DEV)
    first = idl.facenet(x112)
    tol = am.MARGIN * am.rel_l2(am.emulated(dt), g["feat64"])
    assert isinstance(first, list) and len(first) == 1 and am.rel_l2(first[0].cpu(), g["feat64"]) <= tol
    eng = idl.facenet.engine
    assert idl.facenet.engine is eng
    idl.facenet.load_state_dict(sd)
    assert idl.facenet._engine is None
    assert idl.facenet.engine is not eng and idl.half().facenet._engine is None
    idl = idl.float()
    with pytest.raises(hip.VFaceHipError):
        idl.facenet(x112.cpu())
    with pytest.raises(hip.VFaceHipError):
        idl.extract_feats(torch.zeros(1, 3, 224, 224))
    with pytest.raises(NotImplementedError):
        idl(x112, x112)
    # the conditioning stage with the identity network: checkpoint-style keys load, id_feat=None computes it from x
    cfg = cm.engine_cfg("tiny")
    ldm = LatentDiffusion(TINY_UNET, cond_stage_config=dict(params=dict(vision_config=cfg, compute_dtype=dt), other_params=dict(arcface=True)))
    synth.fill_module_(ldm.cond_stage_model, seed=5)
    for name in ("proj_out_source", "proj_out_target", "ID_proj_out", "landmark_proj_out"):
        synth.fill_module_(getattr(ldm, name), seed=5, prefix=name + ".")
    ckpt = {**ldm.state_dict(), **{"face_ID_model.facenet." + k: v for k, v in sd.items()}}
    ldm.load_state_dict(ckpt)
    ldm = ldm.to(DEV)
    assert same_bits(ldm.face_ID_model.facenet.state_dict()["body.3.res_layer.2.weight"].cpu(), sd["body.3.res_layer.2.weight"])
    S = cfg["image"]
    gen = torch.Generator().manual_seed(3)
    x = torch.randn(2, 3, 224, 224, generator=gen).to(DEV)
    e_src = ldm.get_learned_conditioning(torch.randn(2, 3, S, S, generator=gen).to(DEV))
    e_tar = ldm.get_learned_conditioning(torch.randn(2, 3, S, S, generator=gen).to(DEV))
    lmk = torch.rand(2, 136, generator=gen).to(DEV)
    feats = ldm.face_ID_model.extract_feats(x)[0]
    assert tuple(feats.shape) == (2, 512) and float((feats.double().norm(dim=1) - 1).abs().max()) < 1e-5
    auto = ldm.conditioning_with_feat(x, landmarks=lmk, e_src=e_src, e_tar=e_tar)
    given = ldm.conditioning_with_feat(x, landmarks=lmk, id_feat=feats, e_src=e_src, e_tar=e_tar)
    other = ldm.conditioning_with_feat(x, landmarks=lmk, id_feat=feats.flip(0), e_src=e_src, e_tar=e_tar)
    assert same_bits(auto, given) and not same_bits(other, given)
    with pytest.raises(NotImplementedError, match="id_feat"):      # no image to compute it from
        ldm.conditioning_with_feat(None, landmarks=lmk, e_src=e_src, e_tar=e_tar)
    # without the option nothing is built and the checkpoint's keys stay outside
    plain = LatentDiffusion(TINY_UNET, cond_stage_config=dict(params=dict(vision_config=cfg, compute_dtype=dt)))
    assert not hasattr(plain, "face_ID_model") and not any(k.startswith("face_ID_model") for k in plain.state_dict())
    with pytest.raises(NotImplementedError, match="id_feat"):
        plain.to(DEV).conditioning_with_feat(x, landmarks=lmk, e_src=e_src, e_tar=e_tar)
    # the frames' entry point is prep + extract_feats in one pass: the same image as the encoder's
    frames = am.frames()[:1, :, ::4, ::4].contiguous().to(DEV)
    mask = (torch.rand(1, 1, 128, 128, generator=gen) > 0.5).float().to(DEV)
    a = ldm.face_ID_model.extract_feats_from_frames(frames, mask)[0]
    b = ldm.face_ID_model.extract_feats_from_frames(frames)[0]
    assert tuple(a.shape) == (1, 512) and not same_bits(a, b)
