"""The face parser (vface_amd/parsing.py, ``ParseEngine.logits``) stage by stage against fp64: every launch fed its own stage's input.

Every launch ``logits`` makes, with its flags and operand form, against the stage of ``parse_bounds.check_stage`` that pins it
(``stage[...]`` = test_stage at that stage; "per element" = the kernel alone on synthetic operands in test_parse_gpu.py /
test_glue_kernels_gpu.py / test_gemm_conv_gpu.py; r = ``cp.resnet``, b = ``cp.resnet.layerL.B``):

  launch (parsing.py)                           flags / operand form                                        pinned by
  window  r.conv1, once per frame chunk         im2col 7x7 stride 2, C_ = ldx = 8, K = 392, row slices of   stage[stem] (the whole batch from the x8 tap;
                                                x8 and of the output; no split (split_k = False)            wide: chunks of 2 + 1 frames, counted)
  relu  (channel_norm_act in place) x 14        stem, b.conv1 x 8, ARM x 2, head32, convblk, conv_out       the stage of each (bit-exact)
  vface_maxpool3x3s2                            -inf padding, 64 channels                                   stage[stem] (bit-exact)
  conv3   b.conv1                               3x3, stride 1 / 2, ldx = the input's row stride (256 for    stage[layerL.B]
                                                layer3.0: it reads cat[:, :128])
  conv3   b.conv2                               3x3, stride 1                                               stage[layerL.B]
  window  b.downsample.0                        im2col 1x1 stride 2, no split                               stage[layer2.0, layer3.0, layer4.0]
  vface_channel_norm_act  residual sums x 8     relu(shortcut + conv2); y = conv2's buffer, or the column   stage[layerL.B] (+ b.out == b.sum);
                                                view cat[:, :128] (ldy 256) for layer2.1                    stage[ffm] (ffm.cat's left half)
  vface_channel_stats  x 4                      means of layer4.1.out (hw 6 / 4), both ARMs, convblk        stage[avg, arm32, arm16, ffm] (mean half)
  vface_pooled_linear  conv_avg                 K = 512 read at stride 2 (lda 1024), ReLU, fp32             stage[avg]
  conv3   cp.armNN.conv.conv                    3x3 on layer4.1.out (cin 512) / layer3.1.out (cin 256)      stage[arm32, arm16]
  vface_pooled_linear  armNN.conv_atten         K = 128 at stride 2 (lda 256), folded bn_atten, sigmoid     stage[arm32, arm16]
  vface_channel_gate  arm32                     in place, r = rvec (the fp32 avg, per image)                stage[arm32]
  conv3   cp.conv_head32.conv                   upsample = 1: 3 x 2 -> 6 x 4 (wide), 2 x 2 -> 4 x 4 (small) stage[head32]
  vface_channel_gate  arm16                     in place, r = rten (16-bit up32)                            stage[arm16]
  conv3   cp.conv_head16.conv                   upsample = 1, out = the column view cat[:, 128:] (ldy 256)  stage[head16]; stage[ffm] (ffm.cat's right half)
  vface_channel_norm_act  relu, column view     cat[:, 128:] in place, ldx = ldy = 256                      stage[head16] (bit-exact)
  window  ffm.convblk.conv                      1x1 stride 1: the plain GEMM on cat, K = lda = 256          stage[ffm] (input: the two producers' taps)
  vface_pooled_linear  ffm.conv1 / ffm.conv2    K = 256 at stride 2, ReLU / K = 64 dense, sigmoid; no bias  stage[ffm]
  vface_channel_gate  ffm                       in place, add_x (feat * atten + feat)                       stage[ffm]
  conv3   conv_out.conv.conv                    3x3, 256 -> 256                                             stage[out]
  window  conv_out.conv_out                     1x1, EPI_OUT_F32, N = 32 (19 + 13 zero rows), no bias       stage[out] (+ columns 19..31 zero)

Cases (parse_bounds.CASES; weights ``synth.fill_parser_``, crops ``cases_parse.crop`` with three seeds): ``wide``, 3 frames of
96 x 64 (maps 48 x 32 .. 3 x 2: non-square, hw = 6 at layer 4; ``window_budget_bytes`` = 2.5 stem window matrices, so the stem runs
as 2 + 1 frames); ``small``, 3 frames of 64 x 64, the smallest legal input (layer 4 is 2 x 2, M = 12; layer 2 is 8 x 8, where
``vface_conv_uses_patch_kernel`` decides the form: test_small_case_forms prints what each 8 x 8 launch took).

Tolerances.  The stages: per element against fp64 with kernel_bounds.py's derived bounds, inputs assembled from the taps of the
producing launches (parse_bounds.py); test_parse_bound_cpu.py shows on the CPU that they admit ``parse_model.engine_taps``'s
restatement of the engine at every stage and refuse twenty-three one-line defects at the stage that owns each.  The network level:
rel-L2 and the worst element's |err| / rms(ref) of the logits against ``parse_model.net_logits`` IN fp64 on the engine's own
pre-filter output, each against the SAME figure of ``engine_taps`` on the same rows, computed on the CPU: rel-L2 x 1.25, the worst
element x 2 (the project's allowances, test_vae_stages_gpu.py's docstring gives the reasons).  No bound comes from the GPU's output."""
import pytest
import torch

import parse_bounds as pb
import parse_model as pm

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DTS = list(pm.DTS)


@pytest.fixture(scope="module")
def sd():
    return pb.base_sd()


_ENG, _TAPS = {}, {}


def engine(case, sd, dt):
    if (case, dt) not in _ENG:
        from vface_amd.parsing import ParseEngine
        budget = pb.CASES[case]["budget"]
        _ENG[(case, dt)] = ParseEngine(sd, dt, DEV, **({} if budget is None else dict(window_budget_bytes=budget)))
    return _ENG[(case, dt)]


def engine_taps(case, sd, dt):
    """The engine once per (case, dtype) with a cloning tap."""
    if (case, dt) not in _TAPS:
        c = pb.CASES[case]
        eng, taps = engine(case, sd, dt), pb.Taps()
        taps["_geom"] = dict(F=c["F"], H=c["H"], W=c["W"])
        eng.logits(eng.prefilter(torch.from_numpy(pb.crops(case)).to(DEV)), c["F"], c["H"], c["W"], tap=taps)
        torch.cuda.synchronize()
        _TAPS[(case, dt)] = taps
    return _TAPS[(case, dt)]


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("stage", pb.stages())
@pytest.mark.parametrize("case", list(pb.CASES))
def test_stage(case, stage, dt, sd):
    pb.check_stage(engine_taps(case, sd, dt), sd, dt, stage)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("case", list(pb.CASES))
def test_tapped_run_equals_untapped_run(case, dt, sd, monkeypatch):
    """Bit for bit; and the stem of ``wide`` runs as chunks of 2 + 1 frames (counted at the launch)."""
    c = pb.CASES[case]
    eng = engine(case, sd, dt)
    stem, real = [], eng.window
    monkeypatch.setattr(eng, "window", lambda name, *a, **k: (stem.append(k["nimg"]) if name.endswith("resnet.conv1") else None, real(name, *a, **k))[1])
    x8 = eng.prefilter(torch.from_numpy(pb.crops(case)).to(DEV))
    plain = eng.logits(x8, c["F"], c["H"], c["W"])
    assert stem == ([2, 1] if case == "wide" else [3]), stem
    tapped = eng.logits(x8, c["F"], c["H"], c["W"], tap=pb.Taps())
    assert plain.dtype == torch.float32 and torch.equal(plain.view(torch.int32), tapped.view(torch.int32))
    assert torch.equal(plain.cpu().view(torch.int32), engine_taps(case, sd, dt)["logits"].view(torch.int32))


def test_small_case_forms():
    """Which kernel each 3 x 3 launch with an 8 x 8 input or output takes at 64 x 64 (0: implicit GEMM, 1: patch-staged, 2: the 8 x 8
    form, four images per workgroup -- with three images present): printed, and the launch rules' answer is one of the three."""
    from vface_amd import hip
    r = pm.R
    launches = [(f"{r}.layer2.0.conv1", 16, 16, 64, 128, 2, False), (f"{r}.layer2.0.conv2", 8, 8, 128, 128, 1, False),
                (f"{r}.layer2.1.conv1", 8, 8, 128, 128, 1, False), (f"{r}.layer2.1.conv2", 8, 8, 128, 128, 1, False),
                (f"{r}.layer3.0.conv1", 8, 8, 128, 256, 2, False), ("cp.conv_head16.conv", 4, 4, 128, 128, 1, True),
                ("conv_out.conv.conv", 8, 8, 256, 256, 1, False)]
    assert pb.geometry(64, 64)[2] == (8, 8) and pb.geometry(64, 64)[4] == (2, 2)
    for name, H, W, cin, cout, stride, up in launches:
        form = hip.conv_uses_patch_kernel(H, W, cin, cout, 3, stride, up)
        oh = (2 * H if up else H) // stride
        splits = pb.splits_of(3 * oh * oh, cout, 9 * cin, 0, oh * oh)
        print(f"[parse forms] {name}: input {H}x{W}{' upsampled' if up else ''} stride {stride} cin {cin} cout {cout}: form {form}, K shares allowed for {splits}")
        assert form in (0, 1, 2), (name, form)


_REF = {}


def net_refs(case, sd, dt, x8):
    """fp64 network and the model's own figures on the engine's pre-filter rows (CPU, once per (case, dtype))."""
    if (case, dt) not in _REF:
        c = pb.CASES[case]
        geom = (c["F"], c["H"], c["W"])
        ref = pm.tok(pm.net_logits(sd, pm.img(x8.float()[:, :3], *geom).double(), torch.float64))
        model = pm.engine_taps(sd, None, dt, x8=x8, geom=geom, step=pb.stem_step(case))["logits"][:, :19]
        _REF[(case, dt)] = (ref, pm.figures(model, ref))
    return _REF[(case, dt)]


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("case", list(pb.CASES))
def test_network_level_against_fp64(case, dt, sd):
    """The logits against ``parse_model.net_logits`` in fp64 on the engine's own pre-filter output, within 1.25 x (rel-L2) and 2 x
    (worst element over rms) of ``parse_model.engine_taps``'s own figures on the same rows."""
    taps = engine_taps(case, sd, dt)
    ref, (m_l2, m_worst) = net_refs(case, sd, dt, taps["x8"])
    l2, worst = pm.figures(taps["logits"][:, :19], ref)
    print(f"[parse network] {case} {str(dt)[6:]}: rel-L2 model {m_l2:.3e} bound {pm.MARGIN_L2 * m_l2:.3e} measured {l2:.3e} (x {l2 / m_l2:.2f}) | "
          f"worst model {m_worst:.3e} bound {pm.MARGIN_WORST * m_worst:.3e} measured {worst:.3e} (x {worst / m_worst:.2f})")
    assert bool(torch.isfinite(taps["logits"]).all())
    assert l2 <= pm.MARGIN_L2 * m_l2, (case, dt, "rel-L2", l2, m_l2)
    assert worst <= pm.MARGIN_WORST * m_worst, (case, dt, "worst element", worst, m_worst)
