"""What test_vae_stages_gpu.py rests on, without a GPU: tests/vae_model.py -- the emulation whose error, times 1.25 (rel-L2) and 2
(worst element), is that file's tolerance -- against the reference's recorded outputs (tests/golden/vae_stages.npz) and against
one-line defects of itself.

1. In fp32, with no 16-bit rounding, the model IS the reference's network: every recorded ``ragged`` intermediate and the final
   outputs of both cases to 1e-5 rel-L2, the tolerance test_oracle_golden.py holds the oracle to on the same elements.
2. A CONDITION, NOT A MEASUREMENT: in fp16 and bf16 the model's rel-L2 against the fixture's fp64 outputs may not exceed the error
   of the reference's own ``torch.autocast`` run on the same outputs (z_mode, z_sample, dec; read from the fixture) -- the rule of
   test_clip_bound_cpu.py.
3. The chunk rule and the attention-length rule of ``vae_engine`` (pure functions).
4. Each seeded defect lands past the stage tolerance on every stage case that owns it, in both types: its rel-L2 against the fp64
   stage reference exceeds 1.25 x the clean model's.  The table (vae_model.OWNERS; stage cases: vae_model.STAGES):

     defect                          stage cases that must fail
     attn_scale_n                    attn.16x128.peaked, attn.768x512.peaked   (n^-1/2 = c^-1/2 within 3 % at (120, 128): not owned there;
                                                                                flat scores hide any scale: the peaked input family)
     softmax_over_queries            attn.*.peaked                             (near-flat probabilities are near-symmetric: peaked family)
     p_times_k                       attn.16x128, attn.120x128, attn.768x512
     value_bias_dropped              attn.16x128, attn.120x128, attn.768x512
     downsample_leading_pad          down.128.6x10, down.128.16x24
     gn_eps_1e5                      res.128.128.6x10.lowvar                   (input std 1e-2: var 1e-4 against eps 1e-5 / 1e-6)
     fold_bias_term_dropped          enc_tail.6x10, enc_tail.16x24             (conv_out bias x 10, so wq @ bc is not a rounding)
     post_quant_bias_into_conv_in    dec_head.6x10, dec_head.16x24             (post_quant bias x 10; only border pixels differ)
     residual_after_norm1            res.128.128.6x10, res.128.256.16x24, res.256.512.6x10
     upsample_phases_swapped         up.512.16x24                              (the only form with phases)
     no_swish_before_conv_out        enc_tail.6x10, dec_tail.16x24

   Not claimed: "the residual added after the 16-bit rounding".  It adds one rounding of the size of the clean error's own terms (a
   factor of about 1.15 in rel-L2 at these stages), inside the 1.25 allowance; the per-element GEMM and convolution bounds of
   test_gemm_conv_gpu.py are what refuses it."""
import pytest
import torch

import vae_model as vm
from vae_model import cv
from conftest import load_golden, rel_l2
from oracle import vae as ovae
from vface_amd import hip, vae_engine as ve

DTS = list(vm.DTS)
OUTS = ("z_mode", "z_sample", "dec")


def _run(case, dt):
    return vm.run_case(case, dt, load_golden("vae_stages"))


@pytest.mark.parametrize("case", list(cv.CASES))
def test_model_in_fp32_is_the_references_network(case):
    g = load_golden("vae_stages")
    out, taps = _run(case, torch.float32)
    for k in ("moments",) + OUTS:
        assert rel_l2(out[k], g[f"{case}.{k}"]) < 1e-5, k
    if case == "ragged":
        assert sorted(taps) == sorted(cv.enc_stages() + cv.dec_stages())
        for k, v in taps.items():
            assert rel_l2(cv.take(case, k, v), g[f"ragged.{k}"]) < 1e-5, k


TYPES = {"f16": torch.float16, "bf16": torch.bfloat16}


@pytest.mark.parametrize("case,tag", [(c, t) for c in cv.CASES for t in cv.AUTOCAST[c]])
def test_model_error_does_not_exceed_the_references_own_autocast_error(case, tag):
    dt = TYPES[tag]
    g = load_golden("vae_stages")
    out, _ = _run(case, dt)
    for k in OUTS:
        err, e_ref = rel_l2(out[k], g[f"{case}.{k}"]), rel_l2(vm.autocast_output(g, case, k, tag), g[f"{case}.{k}"])
        print(f"{case} {tag} {k}: model {err:.3e}, reference autocast {e_ref:.3e}")
        assert 0.0 < err <= e_ref, (case, tag, k, err, e_ref)


def test_frames_per_chunk_and_attention_length_rules():
    ffhq = [256, 256, 512, 1024]                   # widest row per level of the shipped decoder (the mid q | k buffer is 2 x 512)
    f16 = torch.float16
    assert ve.frames_per_chunk(512, 512, ffhq, f16) == 8 and ve.frames_per_chunk(768, 768, ffhq, f16) == 8
    assert ve.frames_per_chunk(512, 512, ffhq, f16, max_frames=3) == 3, "never above max_frames"
    # 1024^2: 8 frames of 256 channels are exactly 4 GiB, dispatch.cpp allows below 4 GiB - 16
    assert ve.frames_per_chunk(1024, 1024, ffhq, f16) == 7
    assert 7 * 1024 * 1024 * 256 * 2 < hip.OPERAND_BYTES_LIMIT <= 8 * 1024 * 1024 * 256 * 2
    # the smallest size that needs a chunk of 1: two frames reach the limit from H W = 2^22 on; one row of 8 pixels less fits two
    assert ve.frames_per_chunk(2048, 2048, ffhq, f16) == 1 and ve.frames_per_chunk(2048, 2040, ffhq, f16) == 2
    assert ve.frames_per_chunk(2048, 2048, 256, f16) == 1 and ve.frames_per_chunk(2048, 2048, 128, f16) == 3
    assert ve.frames_per_chunk(1024, 1024, 256, torch.float32) == 3          # the element size counts
    with pytest.raises(hip.VFaceHipError):
        ve.frames_per_chunk(4096, 4096, ffhq, f16)                        # one frame alone is past the limit
    assert ve.frames_per_chunk(8, 8, [32, 64, 128, 4096], f16) == 8       # a deep level decides where it is the widest in bytes
    assert ve.frames_per_chunk(2048, 2048, [8, 8, 8, 16384], f16) == 1      # 256 x 256 rows of 16384: two frames are 4 GiB
    for h, w in ((64, 64), (96, 96), (128, 128), (10, 12), (1, 8)):
        ve.check_attention_tokens(h, w, "ok")
    for h, w in ((11, 11), (1, 257), (128, 136), (1, 4)):                # 121 and 257 and 4: not multiples of 8; 17408 > 16384
        with pytest.raises(hip.VFaceHipError, match="multiple of 8 and at most 16384"):
            ve.check_attention_tokens(h, w, "refused")


def test_unpack_undoes_the_kernels_k_order():
    from vface_amd import packing
    for cin in (4, 24, 64, 128):
        w = torch.randn(8, cin, 3, 3, generator=torch.Generator().manual_seed(cin))
        cinp = (cin + 7) // 8 * 8
        assert torch.equal(vm.unpack_conv(packing.pack_conv3x3(w), cinp)[:, :cin], w)
        ph = packing.pack_upsample_phases(w)
        k = vm.unpack_conv(ph[2 * 1 + 0], cinp, 2, 2)[:, :cin]            # py = 1, px = 0: rows {i, i + 1}, columns {j - 1, j}
        assert torch.allclose(k[:, :, 0, 1], w[:, :, :2, 1:].sum((2, 3)), atol=1e-6)


CASES_OWNED = [(d, name) for d in vm.DEFECTS for name in vm.OWNERS[d]]


def test_every_defect_has_an_owner_and_every_owner_exists():
    assert set(vm.OWNERS) == set(vm.DEFECTS) and len(vm.DEFECTS) >= 10
    assert all(name in vm.STAGES for names in vm.OWNERS.values() for name in names)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("defect,name", CASES_OWNED)
def test_seeded_defects_land_past_the_stage_tolerance(defect, name, dt):
    sd, x, ref, (l2, worst) = vm.stage_clean(name, dt)
    with torch.no_grad():
        got = vm.stage_model(name, vm.stage_pack(name, sd, dt, "cpu", defect), x, dt, defect)
    e_l2, e_worst = vm.figures(got, ref)
    print(f"{name} {dt} {defect}: rel-L2 {e_l2:.3e} against {vm.MARGIN_L2 * l2:.3e}; worst {e_worst:.3e} against {vm.MARGIN_WORST * worst:.3e}")
    assert e_l2 > vm.MARGIN_L2 * l2, (name, defect, dt, e_l2, l2)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("name", [n for n in vm.STAGES if n not in vm.LARGE])
def test_stage_inputs_are_what_they_claim(name, dt):
    """The clean model is finite and close at every stage case; the peaked family reaches |q.k| c^-1/2 of 15 .. 45, the plain one
    stays below 8; the two frames differ in scale."""
    sd, x, ref, (l2, worst) = vm.stage_clean(name, dt)
    assert 0.0 < l2 < (4e-3 if dt == torch.float16 else 3e-2), (name, l2)
    assert float(x[1].std()) > 2.5 * float(x[0].std())
    kind, g, family = vm.STAGES[name]
    if kind == "attn":
        sd64 = {k: v.double() for k, v in sd.items()}
        h = torch.nn.functional.group_norm(x.double(), 32, sd64["s.norm.weight"], sd64["s.norm.bias"], eps=1e-6)
        q, k = (ovae._conv(sd64, f"s.{n}", h, padding=0).flatten(2) for n in ("q", "k"))
        top = float((q.transpose(1, 2) @ k).abs().max()) * g["c"] ** -0.5
        assert (15.0 < top < 45.0) if family == "peaked" else top < 8.0, (name, top)
