"""The identity network's host side without a GPU: the entry points exist in the header and the ctypes table, the mirror ``Backbone``
has the reference's state dict, the fp64 folds of ``vface_amd.arcface`` (BatchNorm into the convolutions, the output layer as one
matrix, the leading BatchNorms as pairs) reproduce the reference's recorded double runs (tests/golden/arcface.npz), the bin tables
of ``vface_id_prep``'s host twin are torch's, and what is not shipped raises."""
import os
import re

import pytest
import torch
import torch.nn.functional as F

import arcface_model as am
from arcface_model import ca
from conftest import ROOT, load_golden

ENTRY_POINTS = ("vface_id_prep", "vface_prelu", "vface_se_gate_add", "vface_l2norm_rows")


def test_entry_points_in_header_table_and_library():
    from vface_amd import hip
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "vface_hip.h")).read(), flags=re.S)
    lib = hip.load()
    for name in ENTRY_POINTS:
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
        assert name in hip.SIGNATURES and hasattr(lib, name), name
    assert lib.vface_abi_version() == 8
    assert "arcface.hip" in open(os.path.join(ROOT, "vface_amd", "csrc", "Makefile")).read()


def test_mirror_state_dict_is_the_references():
    g = load_golden("arcface")
    sd = am.network().state_dict()
    assert len(sd) == 397
    assert list(sd.keys()) == [str(k) for k in g["keys"]]
    assert [",".join(str(s) for s in v.shape) for v in sd.values()] == [str(s) for s in g["shapes"]]
    from vface_amd.src.Face_models.encoders.model_irse import Backbone
    plain = Backbone(112, 50, "ir_se", affine=False).state_dict()
    assert "output_layer.4.weight" not in plain and "output_layer.4.running_var" in plain and len(plain) == 395


@pytest.mark.parametrize("name", list(ca.UNIT_CASES))
def test_fp64_fold_reproduces_the_unit(name):
    g = load_golden("arcface")
    sd, x, (cin, depth, stride, H, W, n) = am.unit_case(name)
    got = am.run_unit(sd, "u", x, cin, depth, stride)
    ref = g[f"{name}.out64"]
    assert got.shape == ref.shape == (n, depth, (H - 1) // stride + 1, (W - 1) // stride + 1)
    assert float((got - ref).abs().max()) < 1e-12 * float(ref.abs().max())


def test_fp64_fold_reproduces_the_network():
    """From the frames, through the CLIP image and the chain's twin, with the double run's own constants: ``feat64`` to fp64
    rounding.  From the stored ``prep`` (rounded to fp32 in the fixture, 6e-8) to that rounding."""
    import clip_bounds as cb
    g = load_golden("arcface")
    sd = am.network().state_dict()
    img = cb.prep_ref(am.frames(), None, 224)
    x = am.prep_twin(img, decimal_constants=True)
    assert float((x - g["prep"].double()).abs().max()) < 2.0 ** -23 * float(x.abs().max())
    assert am.rel_l2(am.features(sd, x), g["feat64"]) < 1e-12
    assert am.rel_l2(am.features(sd, g["prep"]), g["feat64"]) < 2e-7
    assert am.rel_l2(g["feat32"], g["feat64"]) < 1e-5
    assert float((g["feat64"].norm(dim=1) - 1).abs().max()) < 1e-12


def test_fold_head_without_affine_and_bn_pair():
    g = torch.Generator().manual_seed(3)
    C_, hw, N = 8, 4, 6
    sd = {"o.0.weight": torch.rand(C_, generator=g) + 0.5, "o.0.bias": torch.randn(C_, generator=g), "o.0.running_mean": torch.randn(C_, generator=g),
          "o.0.running_var": torch.rand(C_, generator=g) + 0.5, "o.3.weight": torch.randn(N, C_ * hw, generator=g), "o.3.bias": torch.randn(N, generator=g),
          "o.4.running_mean": torch.randn(N, generator=g), "o.4.running_var": torch.rand(N, generator=g) + 0.5}
    sd = {k: v.double() for k, v in sd.items()}
    from vface_amd.arcface import bn_pair, fold_head
    x = torch.randn(3, C_, 2, 2, generator=g).double()
    for affine in (False, True):
        if affine:
            sd["o.4.weight"], sd["o.4.bias"] = torch.rand(N, generator=g).double() + 0.5, torch.randn(N, generator=g).double()
        t = F.batch_norm(x, sd["o.0.running_mean"], sd["o.0.running_var"], sd["o.0.weight"], sd["o.0.bias"], False, 0.0, 1e-5)
        t = t.reshape(3, -1) @ sd["o.3.weight"].T + sd["o.3.bias"]
        ref = F.batch_norm(t, sd["o.4.running_mean"], sd["o.4.running_var"], sd.get("o.4.weight"), sd.get("o.4.bias"), False, 0.0, 1e-5)
        w, b = fold_head(sd, "o", hw)
        got = x.permute(0, 2, 3, 1).reshape(3, -1) @ w.T + b
        assert float((got - ref).abs().max()) < 1e-12
    a, b = bn_pair(sd, "o.0")
    assert torch.allclose(a[None, :, None, None] * x + b[None, :, None, None],
                          F.batch_norm(x, sd["o.0.running_mean"], sd["o.0.running_var"], sd["o.0.weight"], sd["o.0.bias"], False, 0.0, 1e-5), atol=1e-13)


@pytest.mark.parametrize("H,W", [(224, 224), (256, 256), (256, 220), (300, 200)])
def test_bin_tables_are_torchs(H, W):
    """The twin's integer bins against ``adaptive_avg_pool2d`` itself, through both pools and the crop, on noise (a bin edge off by
    one anywhere moves an output by a large fraction of a pixel's value); a 256-high image skips the first pool."""
    x = torch.randn(2, 3, H, W, generator=torch.Generator().manual_seed(H + W), dtype=torch.float64)
    ref = x if H == 256 else F.adaptive_avg_pool2d(x, (256, 256))
    ref = F.adaptive_avg_pool2d(ref[:, :, 35:223, 32:220], (112, 112))
    got = am.prep_twin(x, clip_img=False)
    assert float((got - ref).abs().max()) < 1e-13
    for n_in, n_out in ((224, 256), (188, 112), (H, 256)):
        b = am.bins(n_in, n_out)
        assert b[0][0] == 0 and b[-1][1] == n_in and all(lo < hi for lo, hi in b)
        m = am.pool_matrix(n_in, n_out)
        v = torch.randn(1, 1, n_in, 1, dtype=torch.float64, generator=torch.Generator().manual_seed(1))
        assert torch.allclose((m @ v[0, 0]), F.adaptive_avg_pool2d(v, (n_out, 1))[0, 0], atol=1e-14)


def test_unsupported_configurations_raise():
    from vface_amd.arcface import check_config
    from vface_amd.src.Face_models.encoders.model_irse import Backbone
    for kw in (dict(input_size=224), dict(num_layers=100), dict(num_layers=152), dict(mode="ir")):
        with pytest.raises(NotImplementedError, match="num_layers=50"):
            Backbone(**{**dict(input_size=112, num_layers=50, mode="ir_se"), **kw})
    with pytest.raises(NotImplementedError, match="single scale"):
        check_config(multi_scale=True)
    with pytest.raises(NotImplementedError):
        am.network().forward(torch.zeros(1, 3, 112, 112), multi_scale=True)
    with pytest.raises(NotImplementedError):
        am.network().forward(torch.zeros(1, 3, 224, 224))


def test_cpu_tensors_raise_without_a_fallback():
    from vface_amd import hip
    x = torch.zeros(1, 3, 112, 112)
    with pytest.raises(hip.VFaceHipError):
        am.network().forward(x)
    out = torch.zeros(112 * 112, 8, dtype=torch.float16)
    with pytest.raises(hip.VFaceHipError):
        hip.id_prep(torch.zeros(1, 3, 224, 224), out)
    with pytest.raises(hip.VFaceHipError):
        hip.l2norm_rows(torch.zeros(1, 8), torch.zeros(1, 8), B=1, N=8)


def test_fill_moves_prelu_slopes_and_running_means():
    sd = am.network().state_dict()
    slopes = torch.cat([v for k, v in sd.items() if re.search(r"(input_layer\.2|res_layer\.2)\.weight$", k)])
    assert 0.14 < float(slopes.min()) and float(slopes.max()) < 0.36
    means = torch.cat([v for k, v in sd.items() if k.endswith("running_mean")])
    assert float(means.abs().max()) < 0.11
    gains = torch.cat([v for k, v in sd.items() if re.search(r"res_layer\.[04]\.weight$", k)])
    assert 0.89 < float(gains.min()) and float(gains.max()) < 1.11


def test_cli_flag_needs_clip_cond_and_is_off_by_default():
    from vface_amd.scripts.VFace_inference_batch import build_parser, run_synthetic
    assert build_parser().parse_args(["--synthetic", "--clip_cond"]).arcface is False
    assert build_parser().parse_args(["--synthetic", "--clip_cond", "--arcface"]).arcface is True
    with pytest.raises(SystemExit, match="--clip_cond"):
        run_synthetic(build_parser().parse_args(["--synthetic", "--arcface"]))


def test_latent_diffusion_builds_the_identity_network_only_when_asked():
    import clip_model as cm
    from vface_amd.ldm.models.diffusion.ddpm import IDLoss, LatentDiffusion
    unet = dict(image_size=8, in_channels=9, out_channels=4, model_channels=32, attention_resolutions=[4, 2, 1], num_res_blocks=1,
                channel_mult=[1, 2, 4, 4], num_heads=8, use_spatial_transformer=True, transformer_depth=1, context_dim=768,
                use_checkpoint=True, legacy=False)
    stage = dict(params=dict(vision_config=cm.engine_cfg("tiny")))
    plain = LatentDiffusion(unet, cond_stage_config=stage)
    assert not hasattr(plain, "face_ID_model")
    with_id = LatentDiffusion(unet, cond_stage_config=dict(stage, other_params=dict(arcface=True)))
    keys = [k for k in with_id.state_dict() if k.startswith("face_ID_model.")]
    assert len(keys) == 397 and all(k.startswith("face_ID_model.facenet.") for k in keys)
    sd = am.network().state_dict()
    with_id.load_state_dict({**with_id.state_dict(), **{"face_ID_model.facenet." + k: v for k, v in sd.items()}})
    assert torch.equal(with_id.face_ID_model.facenet.state_dict()["input_layer.2.weight"], sd["input_layer.2.weight"])
    with pytest.raises(NotImplementedError, match="training loss"):
        with_id.face_ID_model(None, None)
    with pytest.raises(NotImplementedError, match="single scale"):
        IDLoss(multiscale=True)
