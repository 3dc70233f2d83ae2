"""The RAFT-shaped flow producer (vface_amd/raft.py) stage by stage against fp64: every launch fed its own stage's input.

Every launch ``RaftEngine`` makes, with its flags and operand form, against the stage of ``raft_bounds.check_stage`` that pins it
(``stage[...]`` = test_stage_of_the_encoders_alone / test_stage_of_the_chain at that stage; "per element" = the kernel alone on
synthetic operands in test_glue_kernels_gpu.py / test_gemm_conv_gpu.py):

  launch (raft.py)                              flags / operand form                                        pinned by
  vface_nchw_to_nhwc  (tokens8)                 fp32 NCHW -> 16-bit rows of 8, channels 3..7 zero           stage[<enc>.stem] (x8 == round(images), zeros)
  vface_channel_stats  (_norm_act)              InstanceNorm only; 1 slice (hw 560, 140, 35) / 4 slices     stage[feature_encoder.*] (.stats taps)
                                                (hw 4352, 1088, 272 of the chain)
  vface_channel_norm_act  (_norm_act)           in place; stats or none; residual = t2; y = t2 (the sum)    stage[<enc>.*] (.act taps; plain ReLU: bit-exact)
  window  <enc>.convnormrelu.0                  im2col 7x7 stride 2, C_ = ldx = 8, K = 392; BatchNorm       stage[<enc>.stem]
                                                folded (context)
  conv3   <b>.convnormrelu1.0                   3x3, stride 1 / 2, ldx = cin                                stage[<enc>.layerL.B]
  conv3   <b>.convnormrelu2.0                   3x3, stride 1                                               stage[<enc>.layerL.B]
  window  <b>.downsample.0                      im2col 1x1 stride 2                                         stage[<enc>.layer2.0, layer3.0]
  window  <enc>.conv                            1x1 stride 1: the plain GEMM on the rows, no im2col         stage[<enc>.head]
  vface_gemm  correlation, one per pair         A, Wt = two row blocks of the feature rows, fp32 out,       stage[corr]
                                                ldc = hw, N = hw = 272 (no multiple of a tile), no split
  vface_avgpool2_f32  x 3                       16x17 -> 8x8 -> 4x4 -> 2x2 (the odd width floors)           stage[corr] (bit-exact)
  vface_channel_norm_act  tanh, y32 = h32       x = ctx[:, :128] (ldx 256), y = hx[:, :128] (ldy 384)       stage[init]
  vface_channel_norm_act  relu, column views    ctx[:, 128:] -> hx[:, 128:256], ldx 256, ldy 384            stage[init] (bit-exact)
  vface_copy2d  context half, once              hx[:, 128:256] -> rhx[:, 128:256]                           stage[init], stage[uK.convgruG] (rhx == hx)
  vface_corr_lookup                             4 levels, scale 1/16 before the rounding, 324 of 328 cols   stage[uK.lookup] (u1: steered, outside the map)
  window  convcorr1.0                           1x1, C_ = ldx = 328 (4 zero columns), plain GEMM            stage[uK.motion]
  relu  (channel_norm_act in place) x 5         c1, f1, cf (both halves), hx[:, 256:] (ld 384), fh          stage[uK.motion], stage[uK.head] (bit-exact)
  conv3   convcorr2.0                           out = cf[:, :192] (ldy 256)                                 stage[uK.motion]
  window  convflow1.0                           im2col 7x7, C_ = ldx = 8 (flow8: 2 + 6 zero columns)        stage[uK.motion] (input: round(flow32 tap))
  conv3   convflow2.0                           out = the column view cf[:, 192:]                           stage[uK.motion] (cf.act == relu(cat))
  conv3   conv.0                                cout padded 126 -> 128, out = hx[:, 256:384] (ldy 384)      stage[uK.motion] (+ columns 126..127 zero)
  vface_flow_update  (copy only)                flow32 -> hx[:, 382:384]                                    stage[uK.motion] (bit-exact)
  vface_copy2d  motion half, every update       hx[:, 256:] -> rhx[:, 256:]                                 stage[uK.convgruG] (rhx[:, 128:] == hx[:, 128:])
  window  <g>.zr                                z | r concatenated, im2col 1x5 / 5x1, C_ = ldx = 384        stage[uK.convgruG] (input from the taps, not hx)
  vface_gru_gate                                z (16-bit), r * h32 -> rhx[:, :128] (ldrh 384)              stage[uK.convgruG]
  window  <g>.convq                             im2col 1x5 / 5x1 on rhx                                     stage[uK.convgruG] (input: cat[r*h, context,
                                                                                                            motion, round(flow32)] taps, not rhx)
  vface_gru_update                              h32 in place (fp32), 16-bit copy -> hx[:, :128]             stage[uK.convgruG] (h32 bound; copy bit-exact)
  conv3   flow_head.conv1                       cin 128 of ldx 384 (hx[:, :128])                            stage[uK.head]
  conv3   flow_head.conv2                       EPI_OUT_F32, cout padded 2 -> 8                             stage[uK.head] (+ columns 2..7 zero)
  vface_flow_update  (+ delta)                  flow32 += delta[:, :2] (ldd 8); 16-bit copy -> flow8        stage[uK.head] (bit-exact)
  conv3   mask_predictor.convrelu.0             cin 128 of ldx 384                                          stage[upsample]
  window  mask_predictor.conv                   1x1, EPI_OUT_F32, N = 576                                   stage[upsample]
  vface_convex_upsample                         mult 0.25                                                   stage[upsample]
  flow(): chunking by corr_budget_bytes         3 pairs as 3 chunks                                         test_flow_is_the_stages_chained_and_chunks_agree

Tolerances.  The stages: per element against fp64 with kernel_bounds.py's derived bounds, inputs assembled from the taps of the
producing launches (raft_bounds.py); test_raft_bound_cpu.py shows on the CPU that they admit tests/raft_model.py's restatement of
the engine at every stage and refuse eighteen one-line defects at the stage that owns each.  The network level (c): rel-L2 and the
worst element's |err| / rms(ref) of the low-resolution flow after each update and of the final field against oracle/raft.py IN fp64,
each against the SAME figure of tests/raft_model.py on the same inputs, computed on the CPU: rel-L2 x 1.25, the worst element x 2
(the project's allowances, test_vae_stages_gpu.py's docstring gives the reasons).  No bound comes from the GPU's output.
Parity with torchvision's weights stays unpinned (oracle/raft.py)."""
import pytest
import torch

import raft_bounds as rb
import raft_model as rm
from oracle import raft as oraft

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DTS = list(rm.DTS)


@pytest.fixture(scope="module")
def sd():
    return rb.base_sd()


def engine(sd, dt, **kw):
    from vface_amd.raft import RaftEngine
    return RaftEngine(sd, dt, DEV, **kw)


_TAPS = {}


def engine_taps(case, sd, dt):
    """The engine once per (case, dtype), its stages driven by hand with a cloning tap."""
    if (case, dt) in _TAPS:
        return _TAPS[(case, dt)]
    c, x = rb.CASES[case], rb.images(case)
    eng, taps = engine(sd, dt), rb.Taps()
    xd = x.to(DEV)
    with torch.no_grad():
        if case == "enc":
            taps["_geom"] = dict(B=c["N"], H=c["H"], W=c["W"], nimg={e: c["N"] for e in rb.ENCODERS})
            for e in rb.ENCODERS:
                taps[f"_images.{e}"] = x
                eng._encoder(e, eng.tokens8(xd), c["N"], c["H"], c["W"], taps)
        else:
            taps["_geom"] = dict(B=c["B"], H=c["H"], W=c["W"], updates=c["updates"])
            taps["_images.feature_encoder"], taps["_images.context_encoder"] = torch.cat([x[1:], x[:-1]], 0), x[1:]
            st = eng.correlation_stage(xd[1:], xd[:-1], taps)
            eng.context_stage(st, xd[1:], taps)
            for k in range(c["updates"]):
                if k == 1:
                    rb.steer_(st.flow32, st.flow8, st.w, dt)
                taps.prefix = f"u{k}."
                eng.update_stage(st, taps)
            taps.prefix = ""
            eng.upsample_stage(st, taps)
    torch.cuda.synchronize()
    _TAPS[(case, dt)] = taps
    return taps


# ================================================================================================ (a) the encoders alone
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("stage", rb.stages_of("enc"))
def test_stage_of_the_encoders_alone(stage, dt, sd):
    """3 images of 40 x 56: maps of 20 x 28, 10 x 14 and 5 x 7 (hw 560, 140, 35 -- the last two no multiple of any tile, all on the
    one-slice statistics path), every layer of both encoders."""
    rb.check_stage(engine_taps("enc", sd, dt), sd, dt, stage)


# ================================================================================================ (b) the chain
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("stage", rb.stages_of("chain"))
def test_stage_of_the_chain(stage, dt, sd):
    """2 pairs of 128 x 136 (16 x 17 maps, 272 rows per pair; encoders at 64 x 68 after the stem: the four-slice statistics):
    correlation and pyramid, the initial state, TWO updates -- in the second the flow is non-zero, the carried h32 differs from its
    16-bit rounding and a few tokens' windows fall partly and wholly outside the map (``raft_bounds.steer_``) -- and the upsampling."""
    taps = engine_taps("chain", sd, dt)
    if stage == "u1.lookup":
        ref = rb.corr_lookup_ref_and_bound([taps[f"corr.vol{l}"].float() for l in range(4)], taps["u1.flow32.in"], 2, 16, 17, 1 / 16.0, dt)[0]
        assert bool((ref[0, :243] == 0).all()) and int((ref[5] == 0).sum()) > 20 and int((ref[5] != 0).sum()) > 20, "steered windows straddle the border"
        assert not torch.equal(taps["u0.convgru2.h32"], taps["u0.convgru2.h32"].to(dt).float()), "the carried h32 is not its 16-bit rounding"
    rb.check_stage(taps, sd, dt, stage)


# ================================================================================================ (c) the network level
@pytest.fixture(scope="module")
def net_refs(sd):
    """fp64 oracle and the model's own figures on the chain's inputs, 3 updates (CPU, once)."""
    x = rb.images("chain")
    sd64 = {k: v.double() for k, v in sd.items()}
    up64, low64 = oraft.raft_forward(sd64, x[1:].double(), x[:-1].double(), 3, all_low_res=True)
    figs = {}
    for dt in DTS:
        lows = []
        up, _ = rm.flow(sd, x[1:], x[:-1], 3, dt, lows=lows)
        figs[dt] = [rm.figures(l, r) for l, r in zip(lows, low64)] + [rm.figures(up, up64)]
    return up64, low64, figs


@pytest.mark.parametrize("dt", DTS)
def test_network_level_against_the_fp64_oracle(dt, sd, net_refs):
    """The low-resolution flow after each of 3 updates and the final field against oracle/raft.py in fp64, within 1.25 x (rel-L2) and
    2 x (worst element) of tests/raft_model.py's own figures on the same inputs."""
    up64, low64, figs = net_refs
    x = rb.images("chain").to(DEV)
    eng = engine(sd, dt)
    with torch.no_grad():
        st = eng.correlation_stage(x[1:], x[:-1])
        eng.context_stage(st, x[1:])
        lows = []
        for _ in range(3):
            eng.update_stage(st)
            lows.append(rm.img(st.flow32.cpu(), st.B, st.h, st.w))
        up, _ = eng.upsample_stage(st)
    got = [rm.figures(l, r) for l, r in zip(lows, low64)] + [rm.figures(up.cpu(), up64)]
    names = ["update 1", "update 2", "update 3", "upsampled"]
    for n, (l2, worst), (m_l2, m_worst) in zip(names, got, figs[dt]):
        print(f"[raft network] {n} {str(dt)[6:]}: rel-L2 model {m_l2:.3e} bound {rm.MARGIN_L2 * m_l2:.3e} measured {l2:.3e} (x {l2 / m_l2:.2f}) | "
              f"worst model {m_worst:.3e} bound {rm.MARGIN_WORST * m_worst:.3e} measured {worst:.3e} (x {worst / m_worst:.2f})")
    assert bool(torch.isfinite(up).all())
    for n, (l2, worst), (m_l2, m_worst) in zip(names, got, figs[dt]):
        assert l2 <= rm.MARGIN_L2 * m_l2, (n, dt, "rel-L2", l2, m_l2)
        assert worst <= rm.MARGIN_WORST * m_worst, (n, dt, "worst element", worst, m_worst)


# ================================================================================================ (d) composition
def test_flow_is_the_stages_chained_and_chunks_agree(sd, monkeypatch):
    """``flow()`` is bit for bit the four stages chained by hand; with ``corr_budget_bytes`` below two pairs' volumes 3 pairs run as 3
    chunks (counted), each pair within 2 x the model's worst-element error of the one-chunk run (split-K is chosen from M, so the
    bits may differ) and both within that of fp64; a single pair runs."""
    dt, iters = torch.float16, 2
    from vface_amd.utils import synth
    x = synth.synth_normal("raft.stages.compose", (4, 3, 128, 136)).clamp(-1, 1)
    xd = x.to(DEV)
    eng = engine(sd, dt)
    up, low = eng.flow(xd[1:], xd[:-1], iters, return_low_res=True)
    with torch.no_grad():
        st = eng.correlation_stage(xd[1:], xd[:-1])
        eng.context_stage(st, xd[1:])
        for _ in range(iters):
            eng.update_stage(st)
        up_h, low_h = eng.upsample_stage(st)
    assert torch.equal(up, up_h) and torch.equal(low, low_h), "flow() is the stages chained"

    per_pair = (16 * 17) ** 2 * 4 * 4 // 3 + 1
    small = engine(sd, dt, corr_budget_bytes=2 * per_pair - 1)
    calls = []
    real = small.correlation_stage
    monkeypatch.setattr(small, "correlation_stage", lambda a, b, tap=None: (calls.append(a.shape[0]), real(a, b, tap))[1])
    up_c = small.flow(xd[1:], xd[:-1], iters)
    assert calls == [1, 1, 1], calls
    sd64 = {k: v.double() for k, v in sd.items()}
    up64 = oraft.raft_forward(sd64, x[1:].double(), x[:-1].double(), iters)
    up_m, _ = rm.flow(sd, x[1:], x[:-1], iters, dt)
    for b in range(3):
        fig = float((up_m[b].double() - up64[b]).abs().max())
        d_cw = float((up_c[b] - up[b]).abs().max())
        e_c, e_w = float((up_c[b].cpu().double() - up64[b]).abs().max()), float((up[b].cpu().double() - up64[b]).abs().max())
        print(f"[raft chunks] pair {b}: model's worst element {fig:.3e} px; chunked - whole {d_cw:.3e}; chunked - fp64 {e_c:.3e}; whole - fp64 {e_w:.3e}")
        assert d_cw <= 2 * fig and e_c <= 2 * fig and e_w <= 2 * fig, (b, fig, d_cw, e_c, e_w)
    one = eng.flow(xd[1:2], xd[:1], iters)
    assert one.shape == (1, 2, 128, 136) and bool(torch.isfinite(one).all())
