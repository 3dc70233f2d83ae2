"""The conditioning stage's host side without a GPU: the engine's key list against the reference's recorded state dict, the weight
packing, the state-dict rules of the ``FrozenCLIPEmbedder`` mirror (the reference's unused keys dropped, unknown ones refused), the
unchanged default ``LatentDiffusion``, and the ctypes signatures of the new entry points against the header."""
import os
import re

import pytest
import torch

import clip_model as cm
from clip_model import cc          # tests/golden/cases_clip.py
from conftest import ROOT, load_golden


def _recorded(z, name):
    keys = [str(k) for k in z[f"{name}.keys"]]
    shapes = [tuple(int(x) for x in str(s).split(",")) if str(s) else () for s in z[f"{name}.shapes"]]
    return dict(zip(keys, shapes))


@pytest.mark.parametrize("name", list(cc.CONFIGS))
def test_engine_keys_and_shapes_are_the_references(name):
    """Every key the engine reads is in the reference module's state dict with that shape; every other recorded key falls under
    the prefixes the mirror drops (the text tower, text_projection, logit_scale, mapper, final_ln, projection_back)."""
    from vface_amd import clip
    rec = _recorded(load_golden("clip"), name)
    want = clip.state_shapes(cm.engine_cfg(name))
    assert all(k in rec and rec[k] == s for k, s in want.items()), [k for k, s in want.items() if rec.get(k) != s][:5]
    rest = [k for k in rec if k not in want]
    assert rest and all(k.startswith(clip.UNUSED_PREFIXES) for k in rest), [k for k in rest if not k.startswith(clip.UNUSED_PREFIXES)][:5]
    assert {k.split(".")[0] if not k.startswith("model.") else ".".join(k.split(".")[:2]) for k in rest} == {
        "model.text_model", "model.text_projection", "model.logit_scale", "mapper", "final_ln", "projection_back"}
    used, dropped = clip.split_state_dict({k: torch.empty(s) for k, s in rec.items()}, cm.engine_cfg(name))
    assert set(used) == set(want) and sorted(dropped) == sorted(rest)


def test_full_configuration_is_vit_l14():
    from vface_amd import clip
    assert cm.engine_cfg("full") == clip.VIT_L14
    n = sum(int(torch.tensor(s).prod()) if s else 1 for s in clip.state_shapes(clip.VIT_L14).values())
    assert 300e6 < n < 345e6, n                                        # the 304 M-parameter tower + projection + mapper2


def test_patch_weight_packing_round_trips():
    from vface_amd import clip, hip
    w = torch.randn(128, 3, 14, 14, generator=torch.Generator().manual_seed(0))
    wp = clip.pack_patch_weight(w)
    assert wp.shape == (128, hip.CLIP_PATCH_KP) and torch.equal(clip.unpack_patch_weight(wp), w)
    assert not wp[:, hip.CLIP_PATCH_K:].any()
    # column order = nn.Unfold's = vface_clip_patches': the packed GEMM is the convolution
    x = torch.randn(2, 3, 42, 42, generator=torch.Generator().manual_seed(1))
    cols = torch.nn.functional.unfold(x, 14, stride=14).transpose(1, 2)
    conv = torch.nn.functional.conv2d(x, w, stride=14).flatten(2).transpose(1, 2)
    assert torch.allclose(cols @ wp[:, :hip.CLIP_PATCH_K].T, conv, atol=1e-4)


def test_mirror_loads_the_references_state_dict_and_refuses_strangers():
    from vface_amd import hip
    from vface_amd.ldm.modules.encoders import modules as enc
    rec = _recorded(load_golden("clip"), "tiny")
    m = enc.FrozenCLIPEmbedder(vision_config=cm.engine_cfg("tiny"))
    sd = {k: torch.full(s, 0.5) for k, s in rec.items()}
    m.load_state_dict(sd)
    mine = m.state_dict()
    assert set(mine) < set(rec) and all(bool((v == 0.5).all()) for v in mine.values())
    assert not any(k.startswith(("mapper.", "final_ln.", "projection_back.", "model.text_model.")) for k in mine)
    with pytest.raises(hip.VFaceHipError, match="unexpected key"):
        m.load_state_dict({**sd, "model.vision_model.encoder.layers.0.self_attn.rel_pos": torch.zeros(1)})
    with pytest.raises(hip.VFaceHipError, match="missing"):
        m.load_state_dict({k: v for k, v in sd.items() if k != "final_ln2.weight"})
    with pytest.raises(hip.VFaceHipError, match="shape"):
        m.load_state_dict({**sd, "final_ln2.weight": torch.zeros(1024)})
    with pytest.raises(NotImplementedError, match="text tower"):
        m.forward_probabilities(["a face"], None)
    for other in ("FrozenCLIPImageEmbedder", "FrozenCLIPTextEmbedder", "BERTEmbedder", "SpatialRescaler"):
        with pytest.raises(NotImplementedError, match=other):
            getattr(enc, other)()
    with pytest.raises(NotImplementedError, match="nothing is fetched"):
        enc.FrozenCLIPEmbedder(version="openai/clip-vit-base-patch32")


TINY_UNET = dict(image_size=8, in_channels=9, out_channels=4, model_channels=32, attention_resolutions=[4, 2, 1], num_res_blocks=1,
                 channel_mult=[1, 2, 4, 4], num_heads=8, use_spatial_transformer=True, transformer_depth=1, context_dim=768,
                 use_checkpoint=True, legacy=False)


def test_default_latent_diffusion_is_unchanged_and_the_stage_is_opt_in():
    from vface_amd.ldm.models.diffusion.ddpm import LatentDiffusion
    plain = LatentDiffusion(TINY_UNET)
    assert all(k.startswith("model.diffusion_model.") for k in plain.state_dict())
    assert not hasattr(plain, "cond_stage_model") and not hasattr(plain, "proj_out_source")
    cond = LatentDiffusion(TINY_UNET, cond_stage_config=dict(params=dict(vision_config=cm.engine_cfg("tiny"))))
    extra = {k.split(".")[0] for k in cond.state_dict() if not k.startswith("model.")}
    assert extra == {"cond_stage_model", "learnable_vector", "proj_out_source", "proj_out_target", "ID_proj_out", "landmark_proj_out"}
    assert (cond.clip_weight, cond.ID_weight, cond.Landmarks_weight) == (1.0, 10.0, 0.05)
    assert cond.ID_proj_out.weight.shape == (768, 512) and cond.landmark_proj_out.weight.shape == (768, 136)
    # a checkpoint's cond_stage_model.* keys are loaded; the reference's unused ones are dropped on the way
    ckpt = {**cond.state_dict(), "cond_stage_model.mapper.resblocks.0.ln_1.weight": torch.zeros(1024),
            "cond_stage_model.model.text_model.final_layer_norm.bias": torch.zeros(32)}
    ckpt["cond_stage_model.final_ln2.bias"] = torch.full((768,), 0.25)
    cond.load_state_dict(ckpt)
    assert bool((cond.cond_stage_model.state_dict()["final_ln2.bias"] == 0.25).all())
    with pytest.raises(NotImplementedError, match="shipped configuration"):
        LatentDiffusion(TINY_UNET, cond_stage_config=dict(other_params=dict(concat_feat=True)))
    with pytest.raises(NotImplementedError, match="id_feat"):
        cond.conditioning_with_feat(torch.zeros(1, 3, 42, 42), landmarks=torch.zeros(1, 136), tar=torch.zeros(1, 3, 8, 8))


def test_new_entry_points_match_the_header_argument_for_argument():
    """hip.SIGNATURES against include/vface_hip.h for the four new calls: argument count and the pointer / integer / float kind."""
    from vface_amd import hip
    import ctypes as C
    text = open(os.path.join(ROOT, "include", "vface_hip.h")).read()
    kind = {C.c_void_p: "p", C.c_int64: "l", C.c_int: "i", C.c_float: "f"}
    for name in ("vface_clip_patches", "vface_clip_embed", "vface_act", "vface_cond_mix"):
        m = re.search(r"\bint " + name + r"\(([^;]*)\);", text)
        assert m, name
        want = ""
        for arg in (a.strip() for a in m.group(1).replace("\n", " ").split(",")):
            want += "p" if "*" in arg else "l" if arg.startswith("int64_t") else "f" if arg.startswith("float") else "i"
        assert "".join(kind[a] for a in hip.SIGNATURES[name][1]) == want, name
    assert "VFACE_ABI_VERSION 8" in text


def test_cli_accepts_clip_cond():
    from vface_amd.scripts.VFace_inference_batch import build_parser
    opt = build_parser().parse_args(["--synthetic", "--clip_cond"])
    assert opt.clip_cond and not build_parser().parse_args(["--synthetic"]).clip_cond
