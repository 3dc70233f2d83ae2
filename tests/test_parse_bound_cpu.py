"""What test_parse_stages_gpu.py rests on, without a GPU: parse_bounds.check_stage -- the per-stage checker of the face parser --
against ``parse_model.engine_taps``, the engine's rounding points restated on the CPU.

1. In fp32 (no rounding) the model IS the network: its logits equal ``parse_model.net_logits`` in fp64 on the same input to 1e-5.
2. THE BOUNDS ADMIT A CORRECT IMPLEMENTATION: the clean model passes ``check_stage`` at every stage of both cases (``wide``: 3 frames
   of 96 x 64, the stem in chunks of 2 + 1 frames; ``small``: 3 frames of 64 x 64), in fp16 and bf16.
3. LIVENESS, a condition on the inputs checked on the clean model alone: in every ReLU tap between 5 % and 95 % of the elements are
   positive; every sigmoid gate has at least half its entries in (0.02, 0.98); the gates of frames 1 and 2 differ from frame 0's by
   more than the gate's bound in at least half the channels.  (A dead ReLU or a saturated gate would hide a defect behind it; gates
   that do not vary by frame would hide a gate taken from the wrong frame.)
4. Each of the twenty-three one-line defects of ``parse_model.DEFECTS`` is refused on the ``wide`` case, and the FIRST stage that
   fails is the one that owns it:

     defect                                first failing stage   what refuses it
     stem_chunk2_over_chunk1               stem                  the stem convolution of frames 0 and 2 against the whole batch's x8
     stem_chunk2_reads_frame0              stem                  the stem convolution of frame 2
     maxpool_window_2x2                    stem                  the max-pool of the tapped ReLU, bit for bit
     residual_from_conv1                   layer1.0              the residual sum from the conv2 tap
     identity_shortcut_dropped             layer1.0              the residual sum from the block's input tap
     downsample_without_bn_shift           layer2.0              downsample.0 against weights folded with the shift
     bn_fold_var_for_std                   layer1.0              conv1 against weights folded with sqrt(var + eps)
     feat8_in_right_half                   ffm                   ffm.cat == cat[layer2.1.out | relu(conv_head16)]
     cat_halves_swapped                    ffm                   the same
     cat_right_half_without_relu           ffm                   the same
     arm_gate_relu                         arm32                 the gate against sigmoid of the pooled sum
     arm32_without_avg                     arm32                 the gated sum with the cp.conv_avg tap added
     avg_of_frame0                         arm32                 the gated sum of frames 1, 2
     gate_of_frame0                        arm32                 the gated sum of frames 1, 2
     arm16_adds_before_gating              arm16                 the gated sum
     mean_is_sum                           avg                   the mean against fp64
     mean_by_other_levels_hw               arm16                 the mean against fp64
     head_upsample_rows_cols_exchanged     head32                the upsampled convolution (the map is 3 x 2)
     ffm_without_plus_feat                 ffm                   the gated sum with add_x
     ffm_conv1_without_relu                ffm                   ffm.conv1 against relu of the pooled sum
     conv_out_without_relu                 out                   ReLU in place
     logits_rounded_to_16bit               out                   the class head against the fp32-output bound
     mean_rounded_to_16bit                 avg                   the mean against the fp32 bound

   The issue's "zero padding instead of -inf in the max-pool" is not among them: on post-ReLU data it is an identity."""
import pytest
import torch

import parse_bounds as pb
import parse_model as pm
from conftest import rel_l2
from kernel_bounds import pooled_linear_ref_and_bound

DTS = list(pm.DTS)
GATES = {"cp.arm32.conv_atten": "cp.arm32.mean", "cp.arm16.conv_atten": "cp.arm16.mean", "ffm.conv2": "ffm.conv1"}


@pytest.fixture(scope="module")
def sd():
    return pb.base_sd()


_CLEAN = {}


def clean_taps(case, sd, dt):
    if (case, dt) not in _CLEAN:
        _CLEAN[(case, dt)] = pb.model_taps(case, sd, dt)
    return _CLEAN[(case, dt)]


@pytest.mark.parametrize("case", list(pb.CASES))
def test_model_in_fp32_is_the_network(case, sd):
    c = pb.CASES[case]
    taps = pb.model_taps(case, sd, torch.float32)
    x = pm.img(taps["x8"][:, :3], c["F"], c["H"], c["W"])
    ref = pm.tok(pm.net_logits(sd, x.double(), torch.float64))
    assert rel_l2(taps["logits"][:, :19], ref) < 1e-5
    assert pb.stem_step("wide") == 2 and pb.stem_step("small") == 3


def test_stages_and_defects_are_consistent():
    s = pb.stages()
    assert len(set(s)) == len(s)
    assert len(pm.DEFECTS) >= 16 and set(pm.DEFECTS.values()) <= set(s)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("case", list(pb.CASES))
def test_clean_model_passes_every_stage(case, dt, sd):
    taps = clean_taps(case, sd, dt)
    for s in pb.stages():
        pb.check_stage(taps, sd, dt, s)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("case", list(pb.CASES))
def test_liveness_of_the_cases(case, dt, sd):
    taps = clean_taps(case, sd, dt)
    P = pm.weights(sd, dt)
    relus = [k for k in taps if k.endswith((".act", ".sum")) or k in ("cp.conv_avg", "ffm.conv1")]
    assert len(relus) == 25, relus      # stem, 8 x (conv1, sum), 2 ARMs, 2 heads, convblk, conv_out, conv_avg, ffm.conv1
    for k in relus:
        share = float((taps[k] > 0).float().mean())
        assert 0.05 <= share <= 0.95, (k, share)
    for k, src in GATES.items():
        g = taps[k]
        assert float(((g > 0.02) & (g < 0.98)).float().mean()) >= 0.5, k
        a = taps[src][..., 0] if src.endswith(".mean") else taps[src]
        _, bound = pooled_linear_ref_and_bound(a.float(), *P[k], "sigmoid")
        for f in (1, 2):
            differ = (g[f] - g[0]).abs() > (bound[f] + bound[0])
            assert float(differ.float().mean()) >= 0.5, (k, f)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("defect", list(pm.DEFECTS))
def test_seeded_defect_is_refused_at_the_stage_that_owns_it(defect, dt, sd):
    taps = pb.model_taps("wide", sd, dt, defect)
    stage, msg = pb.first_failing_stage(taps, sd, dt)
    print(f"{defect} {dt}: {stage}: {msg}")
    assert stage == pm.DEFECTS[defect], (defect, dt, stage, msg)
