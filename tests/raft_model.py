"""The flow producer's engine (vface_amd/raft.py) restated in torch on the CPU with ITS rounding points, for ``dt`` in fp16 / bf16
(fp32: no rounding at all -- then it is oracle/raft.py's network, which test_raft_bound_cpu.py holds it to).

* Weights are folded in fp32 (``convnet.fold_bn``), rounded to ``dt`` and padded as ``ConvNetEngine.add_conv`` pads them
  (``weights``): cin 3 -> 8 (stems), 2 -> 8 (convflow1), 324 -> 328 (convcorr1); cout 126 -> 128 (motion), 2 -> 8 (flow head);
  z | r concatenated.  Biases stay fp32.
* Every buffer the engine keeps in 16 bits is rounded where the engine rounds it: each convolution's output, each norm /
  activation output, the lookup's features, z, r * h, the 16-bit copy of the hidden state, the flow slot and ``flow8``.
* Every fp32 buffer stays fp32: the correlation volume and pyramid, the InstanceNorm statistics, ``h32``, ``flow32``, ``delta``,
  the mask.  The 1/16 correlation scale is applied in the lookup, before its rounding.
* Accumulation is the CPU's fp32 (another order than the MFMA's: what the 1.25 / 2 margins of the network-level test are for).
* ``tap(name, tensor)`` is called under the names ``RaftEngine``'s stages use, with token rows ``[M, C]`` of the engine's widths.
* ``defect=``: one of ``DEFECTS``, each a one-line departure from the engine (test_raft_bound_cpu.py shows raft_bounds.check_stage
  refuses each at the stage that owns it).

Plain functions, nothing collected by pytest."""
import torch
import torch.nn.functional as F

from vface_amd.convnet import fold_bn

ENC_LAYERS = (64, 64, 96, 128, 256)
ENC_STRIDES = (2, 1, 2, 2)
HIDDEN = 128
MARGIN_L2 = 1.25      # rel-L2: the project's allowance over an emulation (test_clip_gpu.py, test_vae_stages_gpu.py)
MARGIN_WORST = 2.0    # the worst element: an extreme-value statistic of the same distribution
DTS = (torch.float16, torch.bfloat16)

# defect -> the stage of raft_bounds that owns it (u0 / u1: the first / second update of the chain case)
DEFECTS = {
    "zr_halves_swapped": "u0.convgru1",
    "update_z_swapped": "u0.convgru1",
    "gru2_reads_old_hidden": "u0.convgru2",
    "convq_flow_slot_stale": "u1.convgru1",
    "flow_slot_xy_swapped": "u1.motion",
    "context_through_tanh": "init",
    "initial_h32_from_16bit": "init",
    "hidden_rounded_between_updates": "u1.convgru1",
    "delta_added_to_16bit_flow": "u1.head",
    "lookup_window_transposed": "u0.lookup",
    "lookup_level_not_divided": "u0.lookup",
    "corr_scale_twice": "u0.lookup",
    "instance_norm_unbiased": "feature_encoder.stem",
    "residual_before_norm": "feature_encoder.layer2.0",
    "bn_fold_without_eps": "context_encoder.stem",
    "mask_quarter_left_out": "upsample",
    "flow_times_8_left_out": "upsample",
    "motion_flow_columns_swapped": "u0.motion",
}


def rounder(dt):
    return (lambda t: t) if dt == torch.float32 else (lambda t: t.to(dt).float())


def figures(got, ref64):
    """(rel-L2, worst |err| / rms(ref)) against an fp64 reference."""
    e = got.double() - ref64.double()
    rms = float(ref64.double().pow(2).mean().sqrt().clamp_min(1e-30))
    return float(e.norm() / ref64.double().norm().clamp_min(1e-30)), float(e.abs().max()) / rms


def tok(x):
    """[N, C, H, W] -> token rows [N H W, C]."""
    return x.permute(0, 2, 3, 1).reshape(-1, x.shape[1]).contiguous()


def img(t, N, H, W):
    return t.reshape(N, H, W, -1).permute(0, 3, 1, 2).contiguous()


def stage_sd(sd):
    """The state dict of the stage tests from test_raft_gpu.py's (a flow head that moves, x 4): the context stem's BatchNorm gets a
    running variance of 1e-4 (gain x 1e-2, so the activations keep their size) -- beside eps = 1e-5 that is a 5 % term, so a fold
    that drops eps is not a rounding."""
    sd = {k: v.clone() for k, v in sd.items()}
    sd["context_encoder.convnormrelu.1.running_var"] = sd["context_encoder.convnormrelu.1.running_var"] * 1e-4
    sd["context_encoder.convnormrelu.1.weight"] = sd["context_encoder.convnormrelu.1.weight"] * 1e-2
    return sd


def weights(sd, dt, defect=None):
    """name -> (w [cout_pad, cin_pad, kh, kw] fp32 holding values of ``dt``, b [cout_pad] fp32), keyed as ``RaftEngine.P``."""
    sd = {k: v.detach().float().cpu() for k, v in sd.items()}
    r = rounder(dt)
    P = {}

    def add(name, bn=None, cin_pad=None, cout_pad=None, store=None, src=None):
        s = src or sd
        w, b = s[name + ".weight"], s[name + ".bias"]
        if bn is not None:
            w, b = fold_bn(w, sd[bn + ".weight"], sd[bn + ".bias"], sd[bn + ".running_mean"], sd[bn + ".running_var"],
                           eps=0.0 if defect == "bn_fold_without_eps" else 1e-5, b=b)
        cout, cin, kh, kw = w.shape
        cp = cin_pad if cin_pad is not None else (cin + 7) // 8 * 8
        op = cout_pad if cout_pad is not None else cout
        wp, bp = torch.zeros(op, cp, kh, kw), torch.zeros(op)
        wp[:cout, :cin], bp[:cout] = w, b
        P[store or name] = (r(wp), bp)

    for enc, bn in (("feature_encoder", False), ("context_encoder", True)):
        add(f"{enc}.convnormrelu.0", f"{enc}.convnormrelu.1" if bn else None, cin_pad=8)
        for li in (1, 2, 3):
            for bi in (0, 1):
                b = f"{enc}.layer{li}.{bi}"
                add(f"{b}.convnormrelu1.0", f"{b}.convnormrelu1.1" if bn else None)
                add(f"{b}.convnormrelu2.0", f"{b}.convnormrelu2.1" if bn else None)
                if f"{b}.downsample.0.weight" in sd:
                    add(f"{b}.downsample.0", f"{b}.downsample.1" if bn else None)
        add(f"{enc}.conv")
    m = "update_block.motion_encoder"
    add(f"{m}.convcorr1.0", cin_pad=328)
    add(f"{m}.convcorr2.0")
    add(f"{m}.convflow1.0", cin_pad=8)
    add(f"{m}.convflow2.0")
    add(f"{m}.conv.0", cout_pad=128)
    for g in ("convgru1", "convgru2"):
        p = f"update_block.recurrent_block.{g}"
        zr = {f"zr.{k}": torch.cat([sd[f"{p}.convz.{k}"], sd[f"{p}.convr.{k}"]], 0) for k in ("weight", "bias")}
        add("zr", store=f"{p}.zr", src=zr)
        add(f"{p}.convq")
    add("update_block.flow_head.conv1")
    add("update_block.flow_head.conv2", cout_pad=8)
    add("mask_predictor.convrelu.0")
    add("mask_predictor.conv")
    return P


def conv(P, name, x, N, H, W, stride=1):
    """'same'-padded convolution of token rows ``x [N H W, cin_pad]`` in fp32 -> fp32 rows (the caller rounds)."""
    w, b = P[name]
    kh, kw = w.shape[2:]
    return tok(F.conv2d(img(x[:, :w.shape[1]], N, H, W), w, b, stride=stride, padding=((kh - 1) // 2, (kw - 1) // 2)))


def _no(name, t):
    pass


def instance_stats(x, N, defect=None):
    """(mean, 1 / sqrt(var + 1e-5)) per image and channel of rows ``x [N hw, C]``: fp64 sums rounded to fp32, as the kernel's fold."""
    x64 = x.double().reshape(N, -1, x.shape[1])
    var = x64.var(1, unbiased=defect == "instance_norm_unbiased")
    return torch.stack([x64.mean(1), 1.0 / torch.sqrt(var + float(torch.tensor(1e-5, dtype=torch.float32)))], -1).float()


def encoder(P, enc, x8, N, H, W, dt, tap=None, defect=None):
    """``RaftEngine._encoder``: rows ``x8 [N H W, 8]`` of ``dt`` values -> ``[N H/8 W/8, 256]``."""
    tap = tap or _no
    r = rounder(dt)
    inst = enc == "feature_encoder"

    def norm_act(x, name, n_img, use_inst, residual=None):
        v = x
        if use_inst:
            st = instance_stats(x, n_img, defect)
            tap(f"{name}.stats", st)
            hw = x.shape[0] // n_img
            if defect == "residual_before_norm" and residual is not None:
                st = instance_stats(x + residual, n_img)
                v, residual = ((x + residual) - st[:, :, 0].repeat_interleave(hw, 0)) * st[:, :, 1].repeat_interleave(hw, 0), None
            else:
                v = (x - st[:, :, 0].repeat_interleave(hw, 0)) * st[:, :, 1].repeat_interleave(hw, 0)
        if residual is not None:
            v = v + residual
        y = r(torch.relu(v))
        tap(f"{name}.act", y)
        return y

    tap(f"{enc}.x8", x8)
    x = r(conv(P, f"{enc}.convnormrelu.0", x8, N, H, W, ENC_STRIDES[0]))
    tap(f"{enc}.convnormrelu.0", x)
    H, W = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    x = norm_act(x, f"{enc}.convnormrelu", N, inst)
    for li, stride in enumerate(ENC_STRIDES[1:], start=1):
        for bi in (0, 1):
            b = f"{enc}.layer{li}.{bi}"
            st = stride if bi == 0 else 1
            OH, OW = (H - 1) // st + 1, (W - 1) // st + 1
            t = r(conv(P, f"{b}.convnormrelu1.0", x, N, H, W, st))
            tap(f"{b}.convnormrelu1.0", t)
            t = norm_act(t, f"{b}.convnormrelu1", N, inst)
            t2 = r(conv(P, f"{b}.convnormrelu2.0", t, N, OH, OW))
            tap(f"{b}.convnormrelu2.0", t2)
            t2 = norm_act(t2, f"{b}.convnormrelu2", N, inst)
            if st != 1:
                s = r(conv(P, f"{b}.downsample.0", x, N, H, W, st))
                tap(f"{b}.downsample.0", s)
                x = norm_act(s, f"{b}.downsample", N, inst, residual=t2)
            else:
                x = norm_act(x, f"{b}.sum", N, False, residual=t2)
            tap(f"{b}.out", x)
            H, W = OH, OW
    out = r(conv(P, f"{enc}.conv", x, N, H, W))
    tap(f"{enc}.conv", out)
    return out


def lookup(vols, flow32, B, h, w, defect=None):
    """The 4 x 81 bilinear window features in fp32-faithful arithmetic (fp64 of the fp32 sample point), x 1/16, unrounded."""
    M = B * h * w
    m = torch.arange(M)
    px, py = (m % w).float(), ((m // w) % h).float()
    off = (torch.arange(9) - 4).float()
    scale = 1.0 / 16.0
    if defect == "corr_scale_twice":
        scale = scale * scale
    out = []
    for l, vol in enumerate(vols):
        hl, wl = vol.shape[-2:]
        inv = 1.0 if defect == "lookup_level_not_divided" else 1.0 / (1 << l)
        sx = (((px + flow32[:, 0]) * inv)[:, None, None] + off[None, :, None]).double().expand(M, 9, 9)
        sy = (((py + flow32[:, 1]) * inv)[:, None, None] + off[None, None, :]).double().expand(M, 9, 9)
        if defect == "lookup_window_transposed":
            sx, sy = sx.transpose(1, 2), sy.transpose(1, 2)
        x0, y0 = torch.floor(sx), torch.floor(sy)
        ax, ay = sx - x0, sy - y0
        flat = vol.reshape(M, hl * wl).double()
        val = torch.zeros(M, 9, 9, dtype=torch.float64)
        for dy in (0, 1):
            for dx in (0, 1):
                xx, yy = x0 + dx, y0 + dy
                ok = (xx >= 0) & (xx < wl) & (yy >= 0) & (yy < hl)
                idx = (yy.clamp(0, hl - 1) * wl + xx.clamp(0, wl - 1)).long().reshape(M, 81)
                wgt = (ay if dy else 1 - ay) * (ax if dx else 1 - ax)
                val = val + wgt * torch.gather(flat, 1, idx).reshape(M, 9, 9) * ok
        out.append((val.reshape(M, 81) * scale).float())
    return torch.cat(out, 1)


class State:
    """What ``vface_amd.raft.FlowState`` holds, on the CPU (16-bit buffers as fp32 tensors of ``dt`` values)."""


def correlation_stage(P, image1, image2, dt, tap=None, defect=None):
    tap = tap or _no
    r = rounder(dt)
    B, _, H, W = image1.shape
    st = State()
    st.B, st.H, st.W, st.h, st.w = B, H, W, H // 8, W // 8
    st.hw, st.M = st.h * st.w, B * st.h * st.w
    x8 = F.pad(r(tok(torch.cat([image1, image2], 0).float())), (0, 5))
    fm = encoder(P, "feature_encoder", x8, 2 * B, H, W, dt, tap, defect)
    hw = st.hw
    vols = [torch.cat([fm[b * hw:(b + 1) * hw] @ fm[(B + b) * hw:(B + b + 1) * hw].T for b in range(B)], 0).reshape(st.M, st.h, st.w)]
    tap("corr.vol0", vols[0])
    for l in range(1, 4):
        x = vols[-1]
        oh, ow = x.shape[1] // 2, x.shape[2] // 2
        c = x[:, :2 * oh, :2 * ow]
        vols.append((((c[:, 0::2, 0::2] + c[:, 0::2, 1::2]) + c[:, 1::2, 0::2]) + c[:, 1::2, 1::2]) * 0.25)
        tap(f"corr.vol{l}", vols[-1])
    st.vols = vols
    return st


def context_stage(P, st, image1, dt, tap=None, defect=None):
    tap = tap or _no
    r = rounder(dt)
    M = st.M
    ctx = encoder(P, "context_encoder", F.pad(r(tok(image1.float())), (0, 5)), st.B, st.H, st.W, dt, tap, defect)
    st.hx, st.rhx = torch.zeros(M, 384), torch.zeros(M, 384)
    st.h32 = torch.tanh(ctx[:, :HIDDEN])
    if defect == "initial_h32_from_16bit":
        st.h32 = r(st.h32)
    tap("init.h32", st.h32)
    st.hx[:, :HIDDEN] = r(st.h32)
    st.hx[:, HIDDEN:256] = r(torch.tanh(ctx[:, HIDDEN:])) if defect == "context_through_tanh" else torch.relu(ctx[:, HIDDEN:])
    tap("init.hx", st.hx[:, :256])
    st.rhx[:, HIDDEN:256] = st.hx[:, HIDDEN:256]
    tap("init.rhx", st.rhx[:, HIDDEN:256])
    st.flow32, st.flow8 = torch.zeros(M, 2), torch.zeros(M, 8)
    st.cf = torch.zeros(M, 256)


def update_stage(P, st, dt, tap=None, defect=None):
    tap = tap or _no
    r = rounder(dt)
    B, h, w, M = st.B, st.h, st.w, st.M
    me, rb = "update_block.motion_encoder", "update_block.recurrent_block"
    hx, rhx = st.hx, st.rhx
    tap("flow32.in", st.flow32)
    tap("flow8.in", st.flow8)
    corr = F.pad(r(lookup(st.vols, st.flow32, B, h, w, defect)), (0, 4))
    tap("corr", corr)
    c1 = r(conv(P, f"{me}.convcorr1.0", corr, B, h, w))
    tap("convcorr1.0", c1)
    c1 = torch.relu(c1)
    tap("convcorr1.act", c1)
    cf = st.cf
    cf[:, :192] = r(conv(P, f"{me}.convcorr2.0", c1, B, h, w))
    tap("convcorr2.0", cf[:, :192])
    f1 = r(conv(P, f"{me}.convflow1.0", st.flow8, B, h, w))
    tap("convflow1.0", f1)
    f1 = torch.relu(f1)
    tap("convflow1.act", f1)
    cf[:, 192:] = r(conv(P, f"{me}.convflow2.0", f1, B, h, w))
    tap("convflow2.0", cf[:, 192:])
    cf.copy_(torch.relu(cf))
    tap("cf.act", cf)
    mo = r(conv(P, f"{me}.conv.0", cf, B, h, w))
    tap("motion.0", mo)
    mo = torch.relu(mo)
    tap("motion.act", mo)
    f16 = r(st.flow32)
    if defect == "flow_slot_xy_swapped":
        f16 = f16.flip(1)
    if defect == "motion_flow_columns_swapped":
        hx[:, 256:258], hx[:, 258:] = f16, mo[:, :126]
    else:
        hx[:, 256:], hx[:, 382:] = mo, f16
    tap("hx.flow", hx[:, 382:])
    ncopy = 126 if defect == "convq_flow_slot_stale" else 128
    rhx[:, 256:256 + ncopy] = hx[:, 256:256 + ncopy]
    tap("rhx.x", rhx[:, 256:])
    h_before = (st.h32.clone(), hx[:, :HIDDEN].clone())
    for g in ("convgru1", "convgru2"):
        h32_in = st.h32
        if defect == "gru2_reads_old_hidden" and g == "convgru2":
            h32_in, hx = h_before[0], torch.cat([h_before[1], hx[:, HIDDEN:]], 1)
        tap(f"{g}.hx", hx)
        zr = r(conv(P, f"{rb}.{g}.zr", hx, B, h, w))
        tap(f"{g}.zr", zr)
        zh, rh_ = (zr[:, HIDDEN:], zr[:, :HIDDEN]) if defect == "zr_halves_swapped" else (zr[:, :HIDDEN], zr[:, HIDDEN:])
        z = r(torch.sigmoid(zh))
        rhx[:, :HIDDEN] = r(torch.sigmoid(rh_) * h32_in)
        tap(f"{g}.z", z)
        tap(f"{g}.rh", rhx[:, :HIDDEN])
        tap(f"{g}.rhx", rhx)
        q = r(conv(P, f"{rb}.{g}.convq", rhx, B, h, w))
        tap(f"{g}.q", q)
        if defect == "update_z_swapped":
            st.h32 = z * h32_in + (1 - z) * torch.tanh(q)
        else:
            st.h32 = (1 - z) * h32_in + z * torch.tanh(q)
        hx = st.hx
        hx[:, :HIDDEN] = r(st.h32)
        tap(f"{g}.h32", st.h32)
        tap(f"{g}.hx_h", hx[:, :HIDDEN])
    fh = r(conv(P, "update_block.flow_head.conv1", hx, B, h, w))
    tap("fh.0", fh)
    fh = torch.relu(fh)
    tap("fh.act", fh)
    delta = conv(P, "update_block.flow_head.conv2", fh, B, h, w)
    tap("delta", delta)
    st.flow32 = (r(st.flow32) if defect == "delta_added_to_16bit_flow" else st.flow32) + delta[:, :2]
    st.flow8 = F.pad(r(st.flow32), (0, 6))
    tap("flow32", st.flow32)
    tap("flow8", st.flow8)
    if defect == "hidden_rounded_between_updates":
        st.h32 = r(st.h32)


def upsample_stage(P, st, dt, tap=None, defect=None):
    tap = tap or _no
    r = rounder(dt)
    B, h, w, M = st.B, st.h, st.w, st.M
    fh = r(conv(P, "mask_predictor.convrelu.0", st.hx, B, h, w))
    tap("mask.0", fh)
    fh = torch.relu(fh)
    tap("mask.act", fh)
    mask = conv(P, "mask_predictor.conv", fh, B, h, w)
    tap("mask", mask)
    lg = (1.0 if defect == "mask_quarter_left_out" else 0.25) * mask.reshape(M, 9, 64)
    wgt = torch.softmax(lg, 1)
    f8 = (1.0 if defect == "flow_times_8_left_out" else 8.0) * img(st.flow32, B, h, w)
    nb = F.unfold(f8, 3, padding=1).reshape(B, 2, 9, h * w).permute(0, 3, 1, 2).reshape(M, 2, 9, 1)
    up = (wgt[:, None] * nb).sum(2).reshape(B, h, w, 2, 8, 8).permute(0, 3, 1, 4, 2, 5).reshape(B, 2, 8 * h, 8 * w)
    tap("up", up)
    return up, img(st.flow32, B, h, w)


def flow(sd, image1, image2, iters, dt, defect=None, lows=None):
    """``RaftEngine.flow`` as one chunk -> (up, low); ``lows``: a list that receives the low-resolution flow after every update."""
    P = weights(sd, dt, defect)
    st = correlation_stage(P, image1, image2, dt, None, defect)
    context_stage(P, st, image1, dt, None, defect)
    for _ in range(iters):
        update_stage(P, st, dt, None, defect)
        if lows is not None:
            lows.append(img(st.flow32, st.B, st.h, st.w))
    return upsample_stage(P, st, dt, None, defect)
