"""Face parsing without a GPU: the CPU model of the kernels (tests/parse_model.py) against the reference's own outputs
(tests/golden/parse.npz, written by tests/golden/make_parse_golden.py from REFace/pretrained/face_parsing), the host-side pieces
(BatchNorm fold, state-dict keys, label table, synthetic fill) and every refusal that needs no device."""
import ctypes
import functools
import os
import re
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import GOLDEN, ROOT

sys.path.insert(0, GOLDEN)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import cases_parse as cp  # noqa: E402
import parse_model as pm  # noqa: E402
from vface_amd import hip, parsing  # noqa: E402
from vface_amd.pretrained.face_parsing import BiSeNet, FaceParser, Resnet18, faceParsing_demo, init_faceParsing_pretrained_model  # noqa: E402
from vface_amd.utils import synth  # noqa: E402

NEW_ENTRIES = ("vface_parse_prefilter", "vface_maxpool3x3s2", "vface_channel_gate", "vface_pooled_linear", "vface_upsample_argmax_u8")


@functools.lru_cache(None)
def fixture():
    path = os.path.join(GOLDEN, "parse.npz")
    assert os.path.exists(path), "tests/golden/parse.npz is missing (tests/golden/make_parse_golden.py writes it)"
    z = np.load(path, allow_pickle=False)
    return {k: z[k] for k in z.files}


@functools.lru_cache(None)
def state_dict():
    net = BiSeNet(n_classes=cp.N_CLASSES)
    synth.fill_parser_(net, seed=cp.WEIGHT_SEED)
    return net.state_dict()


@functools.lru_cache(None)
def model_run(H, W):
    """The CPU model on the recorded frame of one size, computed once: pre-filter and logits in both precisions, the fp32 labels
    in the kernel's order and the fp64 margin at full resolution."""
    u8 = cp.crop(H, W, cp.SEEDS[(H, W)])
    out = {}
    for name, npdt, tdt in (("32", np.float32, torch.float32), ("64", np.float64, torch.float64)):
        p = pm.prefilter(u8, npdt)
        low = pm.net_logits(state_dict(), torch.from_numpy(np.ascontiguousarray(p.transpose(2, 0, 1)[None])), tdt)[0].numpy()
        out["pre" + name], out["low" + name] = p, low
        full = pm.upsample(np.ascontiguousarray(low.transpose(1, 2, 0))[None], H, W, npdt)
        out["lab" + name], out["margin" + name] = (a[0] for a in pm.argmax_and_margin(full))
    return out


def rel(a, b):
    return float(np.abs(a.astype(np.float64) - b.astype(np.float64)).max() / np.abs(b).max())


@pytest.mark.parametrize("H,W", cp.NET_SIZES)
def test_model_matches_the_reference(H, W):
    """Pre-filter and 1/8-resolution logits within 1e-5 (relative to the largest value) of the reference's fp32 run; labels equal
    to the reference's wherever the fp64 margin (top - runner-up at full resolution) is at least 1e-4, with at most 0.1 % of the
    pixels left out."""
    z, m, tag = fixture(), model_run(H, W), f"{H}x{W}"
    if f"{tag}.prefilter" in z:
        assert rel(m["pre32"].transpose(2, 0, 1), z[f"{tag}.prefilter"]) <= 1e-5
    assert rel(m["low32"], z[f"{tag}.logits32"]) <= 1e-5
    assert rel(m["low64"], z[f"{tag}.logits64"]) <= 1e-5
    sure = m["margin64"] >= 1e-4
    assert 1.0 - sure.mean() <= 1e-3
    assert np.array_equal(m["lab32"][sure], z[f"{tag}.labels19"][sure])
    assert np.array_equal(pm.seg12_table()[m["lab32"]][sure], z[f"{tag}.labels12"][sure])


@pytest.mark.parametrize("H,W", cp.NET_SIZES)
def test_committed_inputs_stay_under_the_label_rules_cap(H, W):
    """The GPU label rule leaves out pixels whose fp64 margin is under 4 E_ref (fp16) or 32 E_ref (bf16: ulp ratio 8); the inputs
    of cases_parse.py were chosen so that this is under 5 % of the pixels at every size.  Reference numbers only."""
    e_ref = float(fixture()[f"{H}x{W}.e_ref"])
    margin = model_run(H, W)["margin64"]
    assert 1e-3 < e_ref < 1e-2
    assert (margin < 4 * e_ref).mean() <= 0.05
    assert (margin < 32 * e_ref).mean() <= 0.05


def test_seg12_table_on_every_byte():
    """The 32-entry table against the reference's relabelling of arange(256): equal on the entries the kernel can index (a class
    index is below 32); every value past them the reference maps to 0, as it does 15, 16 and 18."""
    ref = fixture()["seg12_of_arange"]
    assert ref.shape == (256,) and ref.dtype == np.uint8
    t = pm.seg12_table()
    assert t.shape == (32,) and np.array_equal(t, ref[:32]) and not ref[32:].any()
    assert sorted(set(t.tolist())) == list(range(12))
    assert np.array_equal(parsing.identity_table().numpy(), np.arange(32))


def test_batchnorm_fold_is_exact_in_fp64():
    g = torch.Generator().manual_seed(5)
    for cin, cout, k, stride in ((3, 8, 7, 2), (8, 16, 3, 1), (16, 8, 1, 2)):
        w = torch.randn(cout, cin, k, k, generator=g, dtype=torch.float64)
        gamma, beta = torch.rand(cout, generator=g, dtype=torch.float64) + 0.5, torch.randn(cout, generator=g, dtype=torch.float64)
        mean, var = torch.randn(cout, generator=g, dtype=torch.float64), torch.rand(cout, generator=g, dtype=torch.float64) + 0.1
        x = torch.randn(2, cin, 9, 10, generator=g, dtype=torch.float64)
        ref = F.batch_norm(F.conv2d(x, w, stride=stride, padding=k // 2), mean, var, gamma, beta, False, 0.0, 1e-5)
        wf, bf = parsing.fold_bn(w, gamma, beta, mean, var)
        assert wf.dtype == torch.float64
        assert (F.conv2d(x, wf, bf, stride=stride, padding=k // 2) - ref).abs().max() < 1e-12


def test_state_dict_keys_are_the_references():
    z, sd = fixture(), state_dict()
    assert len(sd) == 191 and list(sd.keys()) == z["keys"].tolist()
    assert [",".join(str(s) for s in v.shape) for v in sd.values()] == z["shapes"].tolist()
    assert not hasattr(Resnet18, "init_weight")          # the reference's downloads from a URL
    assert sorted(k for k in sd if k.startswith("conv_out16.conv_out") or k.startswith("conv_out32.conv_out")) == [
        "conv_out16.conv_out.weight", "conv_out32.conv_out.weight"]


def test_fill_parser_keeps_the_network_alive():
    """Under the plain fill every running mean is 1 +- 0.1 against zero-mean convolution outputs: the ReLUs cut everything and
    every logit is exactly zero.  With the means centred the logits have spread and several labels occur."""
    H, W = cp.NET_SIZES[0]
    m = model_run(H, W)
    assert m["low32"].std() > 0.1 and len(np.unique(m["lab32"])) >= 4
    dead = BiSeNet(n_classes=cp.N_CLASSES)
    synth.fill_module_(dead, seed=cp.WEIGHT_SEED)
    x = torch.from_numpy(np.ascontiguousarray(m["pre32"].transpose(2, 0, 1)[None]))
    assert not pm.net_logits(dead.state_dict(), x, torch.float32).any()
    a, b = dead.state_dict(), state_dict()
    for k in a:
        if k.endswith("running_mean"):
            assert torch.equal(a[k] - 1.0, b[k]), k
        else:
            assert torch.equal(a[k], b[k]), k


def test_new_entries_in_header_ctypes_and_library():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "vface_hip.h")).read(), flags=re.S)
    lib = hip.load()
    assert lib.vface_abi_version() == 8
    for name in NEW_ENTRIES:
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", src, flags=re.S)
        assert m, f"{name} is not declared in include/vface_hip.h"
        assert len(m.group(1).split(",")) == len(hip.SIGNATURES[name][1]), name
        assert hasattr(ctypes.CDLL(hip.LIB_PATH), name)
        args = [None if a is ctypes.c_void_p else 0 for a in hip.SIGNATURES[name][1]]
        assert getattr(lib, name)(*args) == -1, name         # VFACE_ERR_ARG before anything is launched


def test_refusals_without_a_gpu(tmp_path):
    fp = FaceParser(seg_ckpt=None, size=128, device="cpu")
    with pytest.raises(hip.VFaceHipError, match="GPU"):
        fp.labels(torch.zeros(1, 128, 128, 3, dtype=torch.uint8))
    with pytest.raises(hip.VFaceHipError, match="GPU"):
        fp.seg(torch.zeros(1, 3, 64, 64))
    from PIL import Image
    with pytest.raises(hip.VFaceHipError, match="GPU"):
        faceParsing_demo(fp, Image.fromarray(np.zeros((128, 128, 3), np.uint8)))
    with pytest.raises(NotImplementedError, match="segnext"):
        init_faceParsing_pretrained_model("segnext", None, "")
    with pytest.raises(NotImplementedError, match="segnext"):
        faceParsing_demo(fp, None, model_name="segnext")
    for size in (100, 96, 64, 1000):
        with pytest.raises(hip.VFaceHipError, match="multiple"):
            FaceParser(seg_ckpt=None, size=size, device="cpu")
    for H, W in ((48, 64), (64, 32), (100, 128), (64, 72)):
        with pytest.raises(hip.VFaceHipError, match="multiple of 32"):
            parsing.ParseEngine.check_size(H, W)
    parsing.ParseEngine.check_size(64, 96)
    with pytest.raises(hip.VFaceHipError, match="fp16 or bf16"):
        parsing.ParseEngine(state_dict(), torch.float32, "cpu")


def test_cli_refuses_parse_without_intake_or_at_another_size(tmp_path):
    from vface_amd.scripts import VFace_inference_batch as cli
    base = ["--synthetic", "--with_vae", "--n_frames", "2", "--n_samples", "2", "--max_steps", "1", "--Base_dir", str(tmp_path)]
    with pytest.raises(SystemExit, match="--parse.*--intake"):
        cli.main(base + ["--parse"])
    with pytest.raises(SystemExit, match="--parse needs --H 512 --W 512"):
        cli.main(base + ["--parse", "--intake", "--H", "256", "--W", "256"])
    with pytest.raises(NotImplementedError, match="segnext"):
        cli.main(base + ["--parse", "--intake", "--faceParser_name", "segnext"])
    opt = cli.build_parser().parse_args(base)
    assert opt.parse is False and opt.seg12 is True and opt.faceParser_name == "default" and opt.faceParsing_ckpt is None
