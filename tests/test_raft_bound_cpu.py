"""What test_raft_stages_gpu.py rests on, without a GPU: raft_bounds.check_stage -- the per-stage checker of the flow producer --
against tests/raft_model.py, the engine's rounding points restated on the CPU.

1. In fp32 (no rounding) the model IS oracle/raft.py's network: its taps equal the oracle's named intermediates to 1e-5 rel-L2, and
   the oracle runs in fp64 (it follows the dtype of its inputs) within 1e-4 cells of its fp32 run.
2. THE BOUNDS ADMIT A CORRECT IMPLEMENTATION: the clean model passes ``check_stage`` at every stage of both cases (encoders alone:
   3 images of 40 x 56; the chain: 2 pairs of 128 x 136, two updates, steered flows), in fp16 and bf16.
3. Each of the eighteen one-line defects of ``raft_model.DEFECTS`` is refused, and the FIRST stage that fails is the one that owns it:

     defect                            first failing stage            what refuses it
     zr_halves_swapped                 u0.convgru1                    z against sigmoid of the first half of zr
     update_z_swapped                  u0.convgru1                    h32 against (1 - z) h + z tanh(q)
     gru2_reads_old_hidden             u0.convgru2                    the zr launch's rows == cat[round(h32 after convgru1), x]
     convq_flow_slot_stale             u1.convgru1                    rhx[:, 128:] == hx[:, 128:] at the convq launch (the flow of
                                                                      update 0 is zero, so update 1 is the first that can show it)
     flow_slot_xy_swapped              u1.motion                      hx[:, 382:384] == round(flow32)
     context_through_tanh              init                           hx[:, 128:256] == relu(context half)
     initial_h32_from_16bit            init                           h32 against tanh in fp32
     hidden_rounded_between_updates    u1.convgru1                    r * h and h32 from the h32 TAP of the update before
     delta_added_to_16bit_flow         u1.head                        flow32' == flow32 + delta[:, :2] in fp32
     lookup_window_transposed          u0.lookup                      the lookup per element
     lookup_level_not_divided          u0.lookup
     corr_scale_twice                  u0.lookup
     instance_norm_unbiased            feature_encoder.stem           the statistics (hw = 4352: 1 / (2 hw) = 1.1e-4 against 3e-6)
     residual_before_norm              feature_encoder.layer2.0       the strided block's norm + residual per element
     bn_fold_without_eps               context_encoder.stem           the stem against weights folded WITH eps (``stage_sd``: a BatchNorm
                                                                      whose running variance is 1e-4, or eps would be a rounding)
     mask_quarter_left_out             upsample                       the convex upsampling per element
     flow_times_8_left_out             upsample
     motion_flow_columns_swapped       u0.motion                      hx[:, 382:384] == round(flow32)"""
import pytest
import torch

import raft_bounds as rb
import raft_model as rm
from conftest import rel_l2
from oracle import raft as oraft

DTS = list(rm.DTS)


@pytest.fixture(scope="module")
def sd():
    return rb.base_sd()


_CLEAN = {}


def clean_taps(case, sd, dt):
    if (case, dt) not in _CLEAN:
        _CLEAN[(case, dt)] = rb.model_taps(case, sd, dt)
    return _CLEAN[(case, dt)]


def test_oracle_runs_in_fp64_and_fp32_is_unchanged_by_it(sd):
    x = rb.images("chain")
    up32, low32 = oraft.raft_forward(sd, x[1:], x[:-1], 3, all_low_res=True)
    sd64 = {k: v.double() for k, v in sd.items()}
    up64, low64 = oraft.raft_forward(sd64, x[1:].double(), x[:-1].double(), 3, all_low_res=True)
    assert up64.dtype == torch.float64 and up32.dtype == torch.float32
    assert float((low32[-1].double() - low64[-1]).abs().max()) < 1e-4
    taps = {}
    assert torch.equal(oraft.encoder(sd, "feature_encoder", x, taps), oraft.encoder(sd, "feature_encoder", x)), "taps change no arithmetic"
    assert "feature_encoder.layer2.0.downsample.1" in taps and "feature_encoder.conv" in taps


def test_model_in_fp32_is_the_oracles_network(sd):
    """Every tap of the unrounded model against the oracle's intermediate of the same graph node."""
    f32 = torch.float32
    x = rb.images("chain")
    B, h, w = 2, 16, 17
    taps = rb.model_taps("chain", sd, f32)
    ot = {}
    fm = oraft.encoder(sd, "feature_encoder", torch.cat([x[1:], x[:-1]], 0), ot)
    ctx = oraft.encoder(sd, "context_encoder", x[1:], ot)
    n = lambda t: rm.tok(t)
    for enc in rb.ENCODERS:
        k = "1" if enc == "context_encoder" else "0"          # the engine's context convolutions carry the folded BatchNorm
        assert rel_l2(taps[f"{enc}.convnormrelu.0"], n(ot[f"{enc}.convnormrelu.{k}"])) < 1e-5
        assert rel_l2(taps[f"{enc}.layer2.0.out"], n(ot[f"{enc}.layer2.0.out"])) < 1e-5
        assert rel_l2(taps[f"{enc}.layer2.0.downsample.0"], n(ot[f"{enc}.layer2.0.downsample.{k}"])) < 1e-5
        assert rel_l2(taps[f"{enc}.conv"], n(ot[f"{enc}.conv"])) < 1e-5
    pyr = oraft.corr_pyramid(fm[:B], fm[B:])
    for l in range(4):
        assert rel_l2(taps[f"corr.vol{l}"] / 16.0, pyr[l][:, 0]) < 1e-5
    hidden, context = torch.tanh(ctx[:, :128]), torch.relu(ctx[:, 128:])
    assert rel_l2(taps["init.h32"], n(hidden)) < 1e-5 and rel_l2(taps["init.hx"][:, 128:], n(context)) < 1e-5
    coords0 = oraft.coords_grid(B, h, w)
    corr = oraft.corr_lookup(pyr, coords0)
    assert rel_l2(taps["u0.corr"][:, :324], n(corr)) < 1e-5
    ut = {}
    hidden1, delta = oraft.update_block(sd, hidden, context, corr, coords0 - coords0, ut)
    me = "update_block.motion_encoder"
    pairs = [("u0.convcorr1.0", f"{me}.convcorr1.0", None), ("u0.convflow2.0", f"{me}.convflow2.0", None), ("u0.motion.act", "motion", 126),
             ("u0.convgru1.z", "convgru1.z", None), ("u0.convgru1.rh", "convgru1.rh", None), ("u0.convgru1.q", "update_block.recurrent_block.convgru1.convq", None),
             ("u0.convgru1.h32", "convgru1.hidden", None), ("u0.convgru2.h32", "convgru2.hidden", None), ("u0.delta", "delta", 2)]
    for mine, theirs, cols in pairs:
        got = taps[mine] if cols is None else taps[mine][:, :cols]
        assert rel_l2(got, n(ut[theirs])) < 1e-5, (mine, theirs)
    assert torch.equal(hidden1, ut["convgru2.hidden"])
    # the second update starts from steered flows: the lookup at fractional, partly out-of-range coordinates, and the upsampling
    flow1 = rm.img(taps["u1.flow32.in"], B, h, w)
    ref = n(oraft.corr_lookup(pyr, coords0 + flow1))
    assert float((taps["u1.corr"][:, :324] - ref).abs().max()) < 2e-5 * float(ref.abs().max())
    up = oraft.upsample_flow(sd, rm.img(taps["u1.convgru2.h32"], B, h, w), rm.img(taps["u1.flow32"], B, h, w))
    assert rel_l2(taps["up"], up) < 1e-5


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("case", list(rb.CASES))
def test_clean_model_passes_every_stage(case, dt, sd):
    taps = clean_taps(case, sd, dt)
    for s in rb.stages_of(case):
        rb.check_stage(taps, sd, dt, s)


def test_every_stage_of_a_case_is_listed_once():
    for case in rb.CASES:
        s = rb.stages_of(case)
        assert len(set(s)) == len(s)
    assert len(rm.DEFECTS) >= 12 and set(rm.DEFECTS.values()) <= set(rb.stages_of("chain"))


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("defect", list(rm.DEFECTS))
def test_seeded_defect_is_refused_at_the_stage_that_owns_it(defect, dt, sd):
    taps = rb.model_taps("chain", sd, dt, defect)
    stage, msg = rb.first_failing_stage(taps, sd, dt, rb.stages_of("chain"))
    print(f"{defect} {dt}: {stage}: {msg}")
    assert stage == rm.DEFECTS[defect], (defect, dt, stage, msg)
