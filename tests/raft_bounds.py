"""``check_stage``: one stage of the flow producer (vface_amd/raft.py) against fp64, per element, from the taps of a run -- the
engine's on the GPU (test_raft_stages_gpu.py) or tests/raft_model.py's on the CPU (test_raft_bound_cpu.py: the clean model passes
every stage, eighteen one-line defects are each refused at the stage that owns them).

For each launch of the stage the checker
1. assembles the launch's input FROM THE TAPS OF THE PRODUCING LAUNCHES as oracle/raft.py's graph names them -- never from the buffer
   the consuming launch reads: the ConvGRU rows are ``cat[hidden, context, motion, flow]`` built from the h32 tap (rounded), the
   context tap of the initial state, this update's motion tap and the rounded ``flow32`` tap, not ``hx`` / ``rhx``, so a stale or
   misplaced column slot shows;
2. computes the launch in fp64 from those values and the weights as the engine packs them (folded in fp32, rounded, padded:
   ``raft_model.weights``) and bounds it per element with kernel_bounds.py's derived bounds (``conv_ref_and_bound`` /
   ``gemm_ref_and_bound`` with the split count of ``vface_splitk_workspace_bytes``; the glue kernels' ``*_ref_and_bound``);
3. asserts bit-exact identities where the arithmetic is exact (ReLU in place, the 16-bit copies of ``h32`` and ``flow32``, the
   copied column slots, the pyramid, ``flow32 + delta``, the zero padding columns).
``note()`` prints the headroom per family; no threshold is made from it.

Taps: a dict name -> CPU tensor (token rows ``[M, C]``; 16-bit buffers in their own type or as fp32 holding its values), update k's
names prefixed ``u{k}.``; ``taps["_geom"]`` = dict(B, H, W[, updates]), ``taps["_images.<enc>"]`` = the NCHW images each encoder was given.  Plain functions, nothing collected by pytest."""
import torch

import raft_model as rm
from kernel_bounds import (act_ref_and_bound, assert_within, avgpool2_ref, channel_stats_ref_and_bound, conv_ref_and_bound,
                           convex_upsample_ref_and_bound, corr_lookup_ref_and_bound, flow_update_ref, gemm_ref_and_bound,
                           gru_gate_ref_and_bound, gru_update_ref_and_bound, norm_act_pre_ref_and_bound, note)
from raft_model import ENC_STRIDES, HIDDEN, img

ENCODERS = ("feature_encoder", "context_encoder")
EPS32 = float(torch.tensor(1e-5, dtype=torch.float32))


def splits_of(M, N, K, flags=0, rps=1):
    """How many K shares the launch rules give a GEMM-family launch (host-only: no GPU needed)."""
    from vface_amd import hip
    return max(1, hip.load().vface_splitk_workspace_bytes(M, N, K, flags, rps) // (M * N * 4))


def _f32_flag():
    from vface_amd import hip
    return hip.EPI_OUT_F32


def enc_stages(enc):
    return [f"{enc}.stem"] + [f"{enc}.layer{li}.{bi}" for li in (1, 2, 3) for bi in (0, 1)] + [f"{enc}.head"]


def update_stages(k):
    return [f"u{k}.{s}" for s in ("lookup", "motion", "convgru1", "convgru2", "head")]


def chain_stages(updates):
    return ["corr", "init"] + [s for k in range(updates) for s in update_stages(k)] + ["upsample"]


def rd(t, dt):
    """round_dt: the 16-bit rounding of an fp32 tensor, as fp32."""
    return t.float().to(dt).float()


def _eq(a, b, what):
    """Equal values (a 16-bit buffer against fp32 holding 16-bit values; -0 == +0)."""
    a, b = a.float(), b.float()
    assert a.shape == b.shape, (what, a.shape, b.shape)
    if not torch.equal(a, b):
        bad = (a != b)
        i = tuple(int(v) for v in bad.nonzero()[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {a.numel()} differ; first at {i}: {float(a[i])!r} against {float(b[i])!r}")


def _conv(fam, what, P, name, x, N, H, W, got, dt, stride=1, out_f32=False):
    """One convolution launch (``conv3`` for 3 x 3, else ``window``: im2col + GEMM, or the plain GEMM of a 1 x 1 stride-1 window)
    from its input rows ``x`` against the tap ``got``."""
    w, b = P[name]
    cout, cin, kh, kw = w.shape
    OH, OW = (H - 1) // stride + 1, (W - 1) // stride + 1
    M = N * OH * OW
    flags = _f32_flag() if out_f32 else 0
    s = splits_of(M, cout, 9 * cin, flags, M // N) if (kh, kw) == (3, 3) else splits_of(M, cout, kh * kw * cin, flags, 1)
    ref, bound = conv_ref_and_bound(img(x.float()[:, :cin], N, H, W), w, dt, stride=stride,
                                    pad=((kh - 1) // 2, (kh - 1) // 2, (kw - 1) // 2, (kw - 1) // 2), bias=b, out_f32=out_f32, splits=s)
    note(fam, assert_within(got, ref, bound, what), bound)


def _relu_in_place(taps, pre, post, what):
    _eq(taps[post], torch.relu(taps[pre].float()), f"{what}: ReLU in place is exact")


def _norm_act(fam, taps, name, pre, N, hw, inst, residual, dt):
    """``RaftEngine._norm_act``: the statistics against fp64 of the stored convolution output, then the apply FROM THE DEVICE'S
    statistics (so its bound carries no statistics error); a plain ReLU is exact."""
    x64 = pre.double()
    st = None
    if inst:
        ref, bound = channel_stats_ref_and_bound(x64.reshape(N, hw, -1), EPS32)
        st = taps[f"{name}.stats"].double()
        note(f"{fam} stats", assert_within(st, ref, bound, f"{name}.stats"), bound)
    if st is None and residual is None:
        _eq(taps[f"{name}.act"], torch.relu(pre.float()), f"{name}.act: ReLU in place is exact")
        return
    v, dv = norm_act_pre_ref_and_bound(x64, st, None if residual is None else residual.double(), hw)
    ref, bound = act_ref_and_bound(v, dv, "relu", dt)
    note(f"{fam} norm+act", assert_within(taps[f"{name}.act"], ref, bound, f"{name}.act"), bound)


def _check_encoder(taps, P, dt, enc, part, N, H, W):
    inst = enc == "feature_encoder"
    fam = "raft enc"
    H1, W1 = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    if part == "stem":
        x8 = taps[f"{enc}.x8"]
        assert x8.shape == (N * H * W, 8)
        _eq(x8[:, 3:], torch.zeros(N * H * W, 5), f"{enc}.x8: channels 3..7 are zero")
        _eq(x8[:, :3], rd(rm.tok(taps[f"_images.{enc}"]), dt), f"{enc}.x8 == round_dt(the images as token rows)")
        _conv(f"{fam} stem 7x7", f"{enc}.convnormrelu.0", P, f"{enc}.convnormrelu.0", x8, N, H, W, taps[f"{enc}.convnormrelu.0"], dt, stride=2)
        _norm_act(fam, taps, f"{enc}.convnormrelu", taps[f"{enc}.convnormrelu.0"], N, H1 * W1, inst, None, dt)
        return
    h, w, prev = H1, W1, f"{enc}.convnormrelu.act"
    for li, stride in enumerate(ENC_STRIDES[1:], start=1):
        for bi in (0, 1):
            b = f"{enc}.layer{li}.{bi}"
            st = stride if bi == 0 else 1
            oh, ow = (h - 1) // st + 1, (w - 1) // st + 1
            if part == f"layer{li}.{bi}":
                x = taps[prev]
                _conv(f"{fam} conv3x3", f"{b}.convnormrelu1.0", P, f"{b}.convnormrelu1.0", x, N, h, w, taps[f"{b}.convnormrelu1.0"], dt, stride=st)
                _norm_act(fam, taps, f"{b}.convnormrelu1", taps[f"{b}.convnormrelu1.0"], N, oh * ow, inst, None, dt)
                _conv(f"{fam} conv3x3", f"{b}.convnormrelu2.0", P, f"{b}.convnormrelu2.0", taps[f"{b}.convnormrelu1.act"], N, oh, ow,
                      taps[f"{b}.convnormrelu2.0"], dt)
                _norm_act(fam, taps, f"{b}.convnormrelu2", taps[f"{b}.convnormrelu2.0"], N, oh * ow, inst, None, dt)
                y = taps[f"{b}.convnormrelu2.act"]
                if st != 1:
                    _conv(f"{fam} 1x1 stride 2", f"{b}.downsample.0", P, f"{b}.downsample.0", x, N, h, w, taps[f"{b}.downsample.0"], dt, stride=st)
                    _norm_act(fam, taps, f"{b}.downsample", taps[f"{b}.downsample.0"], N, oh * ow, inst, y, dt)
                    _eq(taps[f"{b}.out"], taps[f"{b}.downsample.act"], f"{b}.out")
                else:
                    _norm_act(fam, taps, f"{b}.sum", x, N, oh * ow, False, y, dt)
                    _eq(taps[f"{b}.out"], taps[f"{b}.sum.act"], f"{b}.out")
                return
            h, w, prev = oh, ow, f"{b}.out"
    assert part == "head", part
    _conv(f"{fam} head 1x1", f"{enc}.conv", P, f"{enc}.conv", taps[prev], N, h, w, taps[f"{enc}.conv"], dt)


def _gru_x(taps, u, dt):
    """The x of both ConvGRUs of update ``u`` as the oracle's graph names it: cat[context, motion, flow] from the producers' taps."""
    return torch.cat([taps["init.hx"].float()[:, HIDDEN:256], taps[f"u{u}.motion.act"].float()[:, :126], rd(taps[f"u{u}.flow32.in"], dt)], 1)


def _h32_before(taps, u, g):
    if g == "convgru2":
        return taps[f"u{u}.convgru1.h32"]
    return taps["init.h32"] if u == 0 else taps[f"u{u - 1}.convgru2.h32"]


def check_stage(taps, sd, dt, stage):
    """Raises AssertionError (naming the launch and the worst element) if ``stage`` of the run that left ``taps`` is out of bound."""
    P = _weights(sd, dt)
    g = taps["_geom"]
    B, H, W = g["B"], g["H"], g["W"]
    for enc in ENCODERS:
        if stage.startswith(enc + "."):
            n = g.get("nimg", {}).get(enc, 2 * B if enc == "feature_encoder" else B)
            return _check_encoder(taps, P, dt, enc, stage[len(enc) + 1:], n, H, W)
    h, w = H // 8, W // 8
    hw, M = h * w, B * h * w
    me, rb = "update_block.motion_encoder", "update_block.recurrent_block"
    if stage == "corr":
        fm = taps["feature_encoder.conv"]
        v0 = taps["corr.vol0"].reshape(M, hw)
        assert splits_of(hw, hw, 256, _f32_flag()) == 1, "an fp32-output launch never splits K"
        for b in range(B):
            ref, bound = gemm_ref_and_bound(fm[b * hw:(b + 1) * hw], fm[(B + b) * hw:(B + b + 1) * hw], dt, out_f32=True)
            note("raft corr volume", assert_within(v0[b * hw:(b + 1) * hw], ref, bound, f"corr.vol0 pair {b}"), bound)
        for l in range(1, 4):
            want = avgpool2_ref(taps[f"corr.vol{l - 1}"].float())
            assert tuple(taps[f"corr.vol{l}"].shape) == tuple(want.shape) == (M, h >> l, w >> l)
            _eq(taps[f"corr.vol{l}"], want, f"corr.vol{l}: three fp32 adds and an exact scale")
    elif stage == "init":
        ctx = taps["context_encoder.conv"].float()
        ref, bound = act_ref_and_bound(ctx[:, :HIDDEN].double(), torch.zeros(M, HIDDEN, dtype=torch.float64), "tanh", torch.float32)
        note("raft init tanh", assert_within(taps["init.h32"], ref, bound, "init.h32"), bound)
        _eq(taps["init.hx"][:, :HIDDEN], rd(taps["init.h32"], dt), "init.hx[:, :128] == round_dt(h32)")
        _eq(taps["init.hx"][:, HIDDEN:], torch.relu(ctx[:, HIDDEN:]), "init.hx[:, 128:256] == relu(context half)")
        _eq(taps["init.rhx"], taps["init.hx"][:, HIDDEN:], "rhx[:, 128:256] == hx[:, 128:256]")
    elif stage == "upsample":
        u = g["updates"] - 1
        hid = rd(taps[f"u{u}.convgru2.h32"], dt)
        _conv("raft conv3x3", "mask.0", P, "mask_predictor.convrelu.0", hid, B, h, w, taps["mask.0"], dt)
        _relu_in_place(taps, "mask.0", "mask.act", "mask.act")
        _conv("raft mask 1x1 f32", "mask", P, "mask_predictor.conv", taps["mask.act"], B, h, w, taps["mask"], dt, out_f32=True)
        ref, bound = convex_upsample_ref_and_bound(taps["mask"].float(), taps[f"u{u}.flow32"].float(), B, h, w, 0.25)
        note("raft convex upsample", assert_within(taps["up"], ref, bound, "up"), bound)
    else:
        k, part = stage.split(".", 1)
        u = int(k[1:])
        t = lambda name: taps[f"u{u}.{name}"]
        if part == "lookup":
            flow_in = t("flow32.in").float()
            if u > 0:
                _eq(t("flow8.in")[:, :2], rd(flow_in, dt), "flow8[:, :2] == round_dt(flow32) at the update's start")
            ref, bound = corr_lookup_ref_and_bound([taps[f"corr.vol{l}"].float() for l in range(4)], flow_in, B, h, w, 1.0 / 16.0, dt)
            note("raft lookup", assert_within(t("corr")[:, :324], ref, bound, f"{stage}: corr"), bound)
            _eq(t("corr")[:, 324:], torch.zeros(M, 4), "corr[:, 324:328] stay zero")
        elif part == "motion":
            _conv("raft convcorr1 1x1", f"{stage}: convcorr1.0", P, f"{me}.convcorr1.0", t("corr"), B, h, w, t("convcorr1.0"), dt)
            _relu_in_place(taps, f"u{u}.convcorr1.0", f"u{u}.convcorr1.act", "convcorr1.act")
            _conv("raft conv3x3", f"{stage}: convcorr2.0", P, f"{me}.convcorr2.0", t("convcorr1.act"), B, h, w, t("convcorr2.0"), dt)
            flow8 = torch.cat([rd(t("flow32.in"), dt), torch.zeros(M, 6)], 1)
            _conv("raft convflow1 7x7", f"{stage}: convflow1.0", P, f"{me}.convflow1.0", flow8, B, h, w, t("convflow1.0"), dt)
            _relu_in_place(taps, f"u{u}.convflow1.0", f"u{u}.convflow1.act", "convflow1.act")
            _conv("raft conv3x3", f"{stage}: convflow2.0", P, f"{me}.convflow2.0", t("convflow1.act"), B, h, w, t("convflow2.0"), dt)
            cf = torch.cat([t("convcorr2.0").float(), t("convflow2.0").float()], 1)
            _eq(t("cf.act"), torch.relu(cf), "cf.act == relu(cat[convcorr2, convflow2]): the two column views of cf")
            _conv("raft conv3x3", f"{stage}: motion.0", P, f"{me}.conv.0", torch.relu(cf), B, h, w, t("motion.0"), dt)
            _eq(t("motion.0")[:, 126:], torch.zeros(M, 2), "motion columns 126..127 (zero weights) are zero")
            _relu_in_place(taps, f"u{u}.motion.0", f"u{u}.motion.act", "motion.act")
            _eq(t("hx.flow"), rd(t("flow32.in"), dt), "hx[:, 382:384] == round_dt(flow32)")
        elif part in ("convgru1", "convgru2"):
            x = _gru_x(taps, u, dt)
            h32 = _h32_before(taps, u, part).float()
            hx = torch.cat([rd(h32, dt), x], 1)
            _eq(t(f"{part}.hx"), hx, f"{part}: the zr launch's rows == cat[round_dt(h32), context, motion, round_dt(flow32)]")
            _conv("raft gru zr 1x5 / 5x1", f"{stage}: zr", P, f"{rb}.{part}.zr", hx, B, h, w, t(f"{part}.zr"), dt)
            zr = t(f"{part}.zr")
            zref, zb, rref, rbound = gru_gate_ref_and_bound(zr, h32, dt)
            note("raft gru gate z", assert_within(t(f"{part}.z"), zref, zb, f"{stage}: z"), zb)
            note("raft gru gate r h", assert_within(t(f"{part}.rh"), rref, rbound, f"{stage}: r * h"), rbound)
            _eq(t(f"{part}.rhx")[:, HIDDEN:], t(f"{part}.hx")[:, HIDDEN:], f"{part}: rhx[:, 128:] == hx[:, 128:] at the convq launch")
            _eq(t(f"{part}.rhx")[:, :HIDDEN], t(f"{part}.rh"), f"{part}: rhx[:, :128] is r * h")
            _conv("raft gru convq 1x5 / 5x1", f"{stage}: q", P, f"{rb}.{part}.convq", torch.cat([t(f"{part}.rh").float(), x], 1), B, h, w,
                  t(f"{part}.q"), dt)
            ref, bound = gru_update_ref_and_bound(t(f"{part}.q"), t(f"{part}.z"), h32.double(), dt)
            note("raft gru update h32", assert_within(t(f"{part}.h32"), ref, bound, f"{stage}: h32"), bound)
            _eq(t(f"{part}.hx_h"), rd(t(f"{part}.h32"), dt), f"{part}: hx[:, :128] == round_dt(h32)")
        elif part == "head":
            hid = rd(t("convgru2.h32"), dt)
            _conv("raft conv3x3", f"{stage}: fh.0", P, "update_block.flow_head.conv1", hid, B, h, w, t("fh.0"), dt)
            _relu_in_place(taps, f"u{u}.fh.0", f"u{u}.fh.act", "fh.act")
            _conv("raft flow head 3x3 f32", f"{stage}: delta", P, "update_block.flow_head.conv2", t("fh.act"), B, h, w, t("delta"), dt, out_f32=True)
            _eq(t("delta")[:, 2:], torch.zeros(M, 6), "delta columns 2..7 (zero weights) are zero")
            want = flow_update_ref(t("flow32.in").float(), t("delta").float())
            _eq(t("flow32"), want, "flow32' == flow32 + delta[:, :2] in fp32")
            _eq(t("flow8"), torch.cat([rd(want, dt), torch.zeros(M, 6)], 1), "flow8 == [round_dt(flow32'), 0 x 6]")
        else:
            raise KeyError(stage)


_W = {}


def _weights(sd, dt):
    key = (id(sd), dt)
    if key not in _W:
        _W.clear()
        _W[key] = (sd, rm.weights(sd, dt))
    return _W[key][1]


def first_failing_stage(taps, sd, dt, stages):
    """The first stage of ``stages`` that ``check_stage`` refuses, with its message; (None, None) if all pass."""
    for s in stages:
        try:
            check_stage(taps, sd, dt, s)
        except AssertionError as e:
            return s, str(e)
    return None, None


# ------------------------------------------------------------------------------------------------ the cases of both test files
CASES = {"enc": dict(N=3, H=40, W=56),                      # (a) maps 20x28, 10x14, 5x7: hw = 560, 140, 35 -- the one-slice statistics
         "chain": dict(B=2, H=128, W=136, updates=2)}       # (b) 16x17 maps, pyramid 16x17, 8x8, 4x4, 2x2; encoders at 64x68 = 4352 pixels


def base_sd():
    """test_raft_gpu.py's synthetic weights (a flow head that moves) with ``raft_model.stage_sd``'s BatchNorm."""
    from oracle import raft as oraft
    from vface_amd.utils import synth
    s = synth.synth_state_dict(oraft.param_shapes(), seed=0)
    s["update_block.flow_head.conv2.weight"] = s["update_block.flow_head.conv2.weight"] * 4.0
    return rm.stage_sd(s)


def images(case):
    from vface_amd.utils import synth
    c = CASES[case]
    n = c["N"] if case == "enc" else c["B"] + 1
    return synth.synth_normal(f"raft.stages.{case}", (n, 3, c["H"], c["W"])).clamp(-1, 1)


def stages_of(case):
    if case == "enc":
        return [s for e in ENCODERS for s in enc_stages(e)]
    up = CASES[case]["updates"]
    return enc_stages("feature_encoder") + ["corr"] + enc_stages("context_encoder") + chain_stages(up)[1:]


def steer_(flow32, flow8, w, dt):
    """Before the second update: a few tokens' flow moved so their 9 x 9 windows fall partly and wholly outside the map (token 0:
    wholly, as test_correlation_pyramid_lookup_matches_oracle; the others straddle a border at some level), ``flow8`` following as
    the rounding of ``flow32`` (what ``vface_flow_update`` keeps true).  In place, on either device."""
    vals = {0: (-20.0, 30.0), 5: (-6.3, 2.2), w + 3: (1.7, -5.6), 100: (float(w) + 2.25, 0.4), 271: (3.7, 5.1), 300: (-11.5, -3.25)}
    for m, (fx, fy) in vals.items():
        flow32[m, 0], flow32[m, 1] = fx, fy
    flow8[:, :2] = flow32.to(dt).to(flow8.dtype)


class Taps(dict):
    """tap(name, tensor) -> a CPU clone under ``prefix + name``."""
    prefix = ""

    def __call__(self, name, t):
        self[self.prefix + name] = t.detach().cpu().clone()


def model_taps(case, sd, dt, defect=None):
    """tests/raft_model.py on a case -> its taps (with ``_geom``)."""
    c, x = CASES[case], images(case)
    P = rm.weights(sd, dt, defect)
    taps = Taps()
    r = rm.rounder(dt)
    with torch.no_grad():
        if case == "enc":
            taps["_geom"] = dict(B=c["N"], H=c["H"], W=c["W"], nimg={e: c["N"] for e in ENCODERS})
            x8 = torch.nn.functional.pad(r(rm.tok(x)), (0, 5))
            for e in ENCODERS:
                taps[f"_images.{e}"] = x
                rm.encoder(P, e, x8, c["N"], c["H"], c["W"], dt, taps, defect)
            return taps
        taps["_geom"] = dict(B=c["B"], H=c["H"], W=c["W"], updates=c["updates"])
        taps["_images.feature_encoder"], taps["_images.context_encoder"] = torch.cat([x[1:], x[:-1]], 0), x[1:]
        st = rm.correlation_stage(P, x[1:], x[:-1], dt, taps, defect)
        rm.context_stage(P, st, x[1:], dt, taps, defect)
        for k in range(c["updates"]):
            if k == 1:
                steer_(st.flow32, st.flow8, st.w, dt)
            taps.prefix = f"u{k}."
            rm.update_stage(P, st, dt, taps, defect)
        taps.prefix = ""
        rm.upsample_stage(P, st, dt, taps, defect)
    return taps
