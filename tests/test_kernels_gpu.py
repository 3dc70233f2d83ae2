"""Per-kernel parity on the MI355X: each C-ABI entry point against a torch-CPU fp32 computation of the
same op on the same (16-bit-rounded) inputs, and against the reference-generated golden vectors.
Tolerances: rel-L2 <= 1e-3 for fp16 outputs (the north-star bound), looser and stated for bf16."""
import math

import os

import pytest
import torch
import torch.nn.functional as F

from conftest import load_golden, rel_l2
from kernel_bounds import U32, rnd, sentinel, ulp

pytestmark = pytest.mark.gpu

DEV = "cuda"
TOL = {torch.float16: 1e-3, torch.bfloat16: 8e-3}


def hip():
    from vface_amd import hip as h
    h.load()
    return h


# 0 = automatic schedule; 5..8 forced product schedules (include/vface_hip.h).  (Codes 1..4, 9, 10 were the experimental schedules
# of rounds 1-3, removed in round 4: the library refuses them.)
VARIANTS = [0, 5, 6, 7, 8]


def need_variant(h, variant):
    assert variant in VARIANTS


GEMM_SHAPES = [(256, 128, 64), (200, 72, 136), (1000, 320, 320), (24, 1280, 320), (4096, 960, 320), (700, 160, 1096)]
# every shape x dtype on the automatic schedule; forced schedules: fp16 on every shape, bf16 on one
GEMM_CASES = [(dt, *s, v) for v in VARIANTS for dt in (torch.float16, torch.bfloat16) for s in GEMM_SHAPES
              if not (v and dt == torch.bfloat16 and s != (1000, 320, 320))]


@pytest.mark.parametrize("dt,M,N,K,variant", GEMM_CASES)
def test_gemm_plain_bias_residual(dt, M, N, K, variant):
    h = hip()
    need_variant(h, variant)
    a, w = rnd((M, K), 1, dt), rnd((N, K), 2, dt, 1 / math.sqrt(K))
    bias = rnd((N,), 3, torch.float32)
    res = rnd((M, N), 4, dt)
    out = torch.empty(M, N, dtype=dt, device=DEV)
    h.gemm(a.to(DEV), w.to(DEV), out, M=M, N=N, K=K, lda=K, ldc=N, bias=bias.to(DEV), residual=res.to(DEV), ldr=N,
           flags=variant << 8)
    ref = a.float() @ w.float().t() + bias + res.float()
    assert rel_l2(out.cpu().float(), ref) < TOL[dt]
    out32 = torch.empty(M, N, dtype=torch.float32, device=DEV)
    h.gemm(a.to(DEV), w.to(DEV), out32, M=M, N=N, K=K, lda=K, ldc=N, flags=h.EPI_OUT_F32 | (variant << 8))
    assert rel_l2(out32.cpu(), a.float() @ w.float().t()) < 1e-5


def test_gemm_strided_views_rowbias_dual_source():
    h = hip()
    dt = torch.float16
    M, N, K = 512, 192, 128
    big = rnd((M, 3 * K), 1, dt)  # a is the middle column block of a wider buffer
    a2 = rnd((M // 2, K), 5, dt)
    w = rnd((N, 2 * K), 2, dt, 1 / math.sqrt(2 * K))
    rb = rnd((4, N), 3, torch.float32)
    outbig = torch.zeros(M, N + 64, dtype=dt, device=DEV)
    bigd = big.to(DEV)
    h.gemm(bigd[:, K:], w.to(DEV), outbig[:, 32:], M=M, N=N, K=2 * K, lda=3 * K, ldc=N + 64, rowbias=rb.to(DEV),
           rows_per_sample=M // 4, a2=a2.to(DEV), lda2=K, k1=K, a2_row_mod=M // 2)
    acat = torch.cat([big[:, K:2 * K].float(), a2.float().repeat(2, 1)], 1)
    ref = acat @ w.float().t() + rb.repeat_interleave(M // 4, 0)
    got = outbig.cpu().float()
    assert rel_l2(got[:, 32:32 + N], ref) < 1e-3
    assert got[:, :32].abs().max() == 0 and got[:, 32 + N:].abs().max() == 0  # nothing outside the view


@pytest.mark.parametrize("variant", [v for v in (0, 1, 3, 5, 7, 9) if v in VARIANTS])
def test_gemm_geglu(variant):
    h = hip()
    need_variant(h, variant)
    dt = torch.float16
    M, d = 300, 64
    x = rnd((M, d), 1, dt)
    w = rnd((8 * d, d), 2, dt, 1 / math.sqrt(d))
    b = rnd((8 * d,), 3, torch.float32, 0.1)
    from vface_amd.packing import pack_geglu
    wp, bp = pack_geglu(w, b)
    out = torch.empty(M, 4 * d, dtype=dt, device=DEV)
    h.gemm(x.to(DEV), wp.to(DEV), out, M=M, N=8 * d, K=d, lda=d, ldc=4 * d, bias=bp.to(DEV),
           flags=h.EPI_GEGLU | (variant << 8))
    y = x.float() @ w.float().t() + b
    val, gate = y.chunk(2, -1)
    assert rel_l2(out.cpu().float(), val * F.gelu(gate)) < 1e-3


CONV_SHAPES = [(16, 64, 12, 10, 1, False), (64, 72, 16, 16, 2, False), (64, 64, 8, 8, 1, True), (320, 320, 16, 16, 1, False),
               (128, 160, 20, 12, 1, False)]
CONV_CASES = [(dt, *s, v) for v in VARIANTS for dt in (torch.float16, torch.bfloat16) for s in CONV_SHAPES
              if not (v and dt == torch.bfloat16)]          # forced schedules: fp16 only


@pytest.mark.parametrize("dt,cin,cout,H,W,stride,up,variant", CONV_CASES)
def test_conv3x3(dt, cin, cout, H, W, stride, up, variant):
    h = hip()
    need_variant(h, variant)
    from vface_amd.packing import pack_conv3x3
    nimg = 3
    x = rnd((nimg, cin, H, W), 1, dt)
    w = rnd((cout, cin, 3, 3), 2, dt, 1 / math.sqrt(9 * cin))
    b = rnd((cout,), 3, torch.float32, 0.1)
    xin = F.interpolate(x.float(), scale_factor=2, mode="nearest") if up else x.float()
    ref = F.conv2d(xin, w.float(), b, stride=stride, padding=1)
    OH, OW = ref.shape[2:]
    rb = rnd((nimg, cout), 4, torch.float32)
    res = rnd((nimg, OH, OW, cout), 5, dt)
    ref = ref + rb[:, :, None, None] + res.float().permute(0, 3, 1, 2)
    xn = x.permute(0, 2, 3, 1).contiguous().to(DEV)
    out = torch.empty(nimg, OH, OW, cout, dtype=dt, device=DEV)
    h.conv3x3(xn, pack_conv3x3(w).to(DEV), out, nimg=nimg, H=H, W=W, cin=cin, cout=cout, ldx=cin, ldy=cout,
              stride=stride, upsample=up, bias=b.to(DEV), rowbias=rb.to(DEV), residual=res.to(DEV), ldr=cout,
              flags=variant << 8)
    assert rel_l2(out.cpu().float().permute(0, 3, 1, 2), ref) < TOL[dt]


def _attn_ref(q, k, v, heads, scale, qk_map=None, v_map=None):
    B, n, d = q.shape
    dh = d // heads
    if qk_map is not None:
        q, k = q[qk_map], k[qk_map]
    if v_map is not None:
        v = v[v_map]
    sp = lambda t: t.reshape(B, t.shape[1], heads, dh).permute(0, 2, 1, 3).float()
    s = (sp(q) @ sp(k).transpose(-1, -2)) * scale
    return (s.softmax(-1) @ sp(v)).permute(0, 2, 1, 3).reshape(B, n, d)


@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("dh,n", [(8, 64), (16, 144), (32, 256), (40, 1024), (40, 576), (80, 256), (160, 64),
                                  (160, 144), (40, 16)])
def test_attention(dt, dh, n):
    h = hip()
    B, heads = 3, 8
    d = heads * dh
    qkv = rnd((B, n, 3 * d), 1, dt)
    out = torch.empty(B, n, d, dtype=dt, device=DEV)
    qd = qkv.to(DEV)
    scale = dh ** -0.5
    h.attention(qd, qd[:, :, d:], qd[:, :, 2 * d:], out, B=B, heads=heads, n=n, nk=n, dh=dh, ldq=3 * d, ldk=3 * d,
                ldv=3 * d, bsq=n * 3 * d, bsk=n * 3 * d, bsv=n * 3 * d, ldo=d, bso=n * d, scale=scale)
    ref = _attn_ref(qkv[..., :d], qkv[..., d:2 * d], qkv[..., 2 * d:], heads, scale)
    assert rel_l2(out.cpu().float(), ref) < TOL[dt]


def test_attention_sample_maps_and_spike():
    """qk_map / v_map remapping, and a spiked key row that forces the running-max rescale late in the walk."""
    h = hip()
    dt = torch.float16
    B, heads, dh, n = 6, 8, 40, 512
    d = heads * dh
    qkv = rnd((B, n, 3 * d), 7, dt)
    qkv[:, 400, d:2 * d] *= 6.0  # key 400 dominates: max jumps in the 7th key block
    qk_map = torch.tensor([0, 1, 0, 1, 0, 1], dtype=torch.int32)
    v_map = torch.tensor([0, 1, 2, 2, 4, 4], dtype=torch.int32)
    out = torch.empty(B, n, d, dtype=dt, device=DEV)
    qd = qkv.to(DEV)
    scale = dh ** -0.5
    h.attention(qd, qd[:, :, d:], qd[:, :, 2 * d:], out, B=B, heads=heads, n=n, nk=n, dh=dh, ldq=3 * d, ldk=3 * d,
                ldv=3 * d, bsq=n * 3 * d, bsk=n * 3 * d, bsv=n * 3 * d, ldo=d, bso=n * d, scale=scale,
                qk_map=qk_map.to(DEV), v_map=v_map.to(DEV))
    ref = _attn_ref(qkv[..., :d], qkv[..., d:2 * d], qkv[..., 2 * d:], heads, scale, qk_map.long(), v_map.long())
    assert rel_l2(out.cpu().float(), ref) < 1e-3


@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("dh,sets,n", [(40, 3, 500), (40, 2, 256), (8, 3, 100), (16, 2, 64), (32, 3, 320)])
def test_attention_shared_scores(dt, dh, sets, n):
    """"replace" injection: every chunk attends with q,k of chunk 0 -> one softmax per frame, `sets` value blocks.
    Must equal the qk_map form of the same kernel family (and the torch reference), ragged n included."""
    h = hip()
    Fr, heads = 2, 8
    B = sets * Fr
    d = heads * dh
    assert h.load().vface_attention_shared_scores_supported(dh, sets) == 1
    qkv = rnd((B, n, 3 * d), 11, dt)
    qkv[:, n // 2, d:2 * d] *= 4.0
    qd = qkv.to(DEV)
    scale = dh ** -0.5
    kw = dict(heads=heads, n=n, nk=n, dh=dh, ldq=3 * d, ldk=3 * d, ldv=3 * d, bsq=n * 3 * d, bsk=n * 3 * d,
              bsv=n * 3 * d, ldo=d, bso=n * d, scale=scale)
    out = torch.zeros(B, n, d, dtype=dt, device=DEV)
    h.attention(qd, qd[:, :, d:], qd[:, :, 2 * d:], out, B=Fr, v_sets=sets, set_stride=Fr, **kw)
    qk_map = (torch.arange(B) % Fr).to(torch.int32)
    ref = _attn_ref(qkv[..., :d], qkv[..., d:2 * d], qkv[..., 2 * d:], heads, scale, qk_map.long(), None)
    assert rel_l2(out.cpu().float(), ref) < TOL[dt]
    out2 = torch.zeros(B, n, d, dtype=dt, device=DEV)
    h.attention(qd, qd[:, :, d:], qd[:, :, 2 * d:], out2, B=B, qk_map=qk_map.to(DEV), **kw)
    # (two exact softmaxes with different references -- the shared-score form raises its reference lazily, the plain dh = 40 form
    # fixes it at the first key block's maximum -- differ by the 16-bit rounding of the unnormalised probabilities)
    assert rel_l2(out.cpu().float(), out2.cpu().float()) < 3e-4 * (10 if dt == torch.bfloat16 else 1)
    # value remap composes with the shared scores
    v_map = torch.arange(B, dtype=torch.int32).flip(0)
    out3 = torch.zeros(B, n, d, dtype=dt, device=DEV)
    h.attention(qd, qd[:, :, d:], qd[:, :, 2 * d:], out3, B=Fr, v_sets=sets, set_stride=Fr, v_map=v_map.to(DEV), **kw)
    ref3 = _attn_ref(qkv[..., :d], qkv[..., d:2 * d], qkv[..., 2 * d:], heads, scale, qk_map.long(), v_map.long())
    assert rel_l2(out3.cpu().float(), ref3) < TOL[dt]


@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("dh,n,variant", [(40, 500, 0), (40, 1024, 0), (40, 4096, 0), (40, 500, 8), (40, 1024, 8), (8, 100, 0), (16, 64, 0), (32, 320, 0)])
def test_attention_shared_scores_two_live_sets_of_three_bit_identical(dt, dh, n, variant):
    """The sampler's dead-branch elimination hands the hooked layers [chunk 0 ; chunk 1] of a three-chunk hook: the shared-score
    kernel then runs its THREE-set instantiation with two live sets (``v_sets_live=2``) -- no read of the third chunk's values
    (the batch ends after the second), no write of its outputs -- and the two live outputs are the full call's bit for bit.
    dh = 40 runs eight waves per workgroup in both calls by default (round 6: the two-live-set form too); ``variant=8`` = four waves
    for the live call, against the same eight-wave full call."""
    h = hip()
    Fr, heads = 2, 8
    d = heads * dh
    qkv = rnd((3 * Fr, n, 3 * d), 12, dt)
    qd = qkv.to(DEV)
    kw = dict(heads=heads, n=n, nk=n, dh=dh, ldq=3 * d, ldk=3 * d, ldv=3 * d, bsq=n * 3 * d, bsk=n * 3 * d,
              bsv=n * 3 * d, ldo=d, bso=n * d, scale=dh ** -0.5)
    full = torch.zeros(3 * Fr, n, d, dtype=dt, device=DEV)
    h.attention(qd, qd[:, :, d:], qd[:, :, 2 * d:], full, B=Fr, v_sets=3, set_stride=Fr, **kw)
    kw["variant"] = variant
    q2 = qd[:2 * Fr].contiguous()                       # a batch that really ends after chunk 1
    SENT = 3.0
    live = torch.full((2 * Fr + 1, n, d), SENT, dtype=dt, device=DEV)
    h.attention(q2, q2[:, :, d:], q2[:, :, 2 * d:], live, B=Fr, v_sets=3, v_sets_live=2, set_stride=Fr, **kw)
    assert torch.equal(live[:2 * Fr], full[:2 * Fr])
    assert (live[2 * Fr:] == SENT).all()                # nothing written past the live sets
    v_map = torch.tensor([1, 0, 3, 2], dtype=torch.int32, device=DEV)
    a = torch.zeros(3 * Fr, n, d, dtype=dt, device=DEV)
    h.attention(qd, qd[:, :, d:], qd[:, :, 2 * d:], a, B=Fr, v_sets=3, set_stride=Fr,
                v_map=torch.tensor([1, 0, 3, 2, 5, 4], dtype=torch.int32, device=DEV), **kw)
    b = torch.zeros(2 * Fr, n, d, dtype=dt, device=DEV)
    h.attention(q2, q2[:, :, d:], q2[:, :, 2 * d:], b, B=Fr, v_sets=3, v_sets_live=2, set_stride=Fr, v_map=v_map, **kw)
    assert torch.equal(b, a[:2 * Fr])


@pytest.mark.parametrize("sets,n", [(1, 500), (1, 4096), (3, 320)])
def test_attention_dh40_32x32_form(sets, n):
    """The A/B form of the dh = 40 kernel on mfma 32x32x16 (variant bit 2; never chosen by the dispatcher: measured slower):
    ragged tail, a spiked key that forces a late rescale, plain and shared-score -- against torch and against the shipped form."""
    h = hip()
    dt, dh, heads, Fr = torch.float16, 40, 8, 2
    B = sets * Fr
    d = heads * dh
    qkv = rnd((B, n, 3 * d), 31, dt)
    qkv[:, (2 * n) // 3, d:2 * d] *= 5.0
    qd = qkv.to(DEV)
    scale = dh ** -0.5
    kw = dict(heads=heads, n=n, nk=n, dh=dh, ldq=3 * d, ldk=3 * d, ldv=3 * d, bsq=n * 3 * d, bsk=n * 3 * d, bsv=n * 3 * d, ldo=d,
              bso=n * d, scale=scale)
    if sets > 1:
        kw.update(B=Fr, v_sets=sets, set_stride=Fr)
        qk_map = (torch.arange(B) % Fr).long()
    else:
        kw.update(B=B)
        qk_map = None
    outs = []
    for variant in (0, 4):
        out = torch.zeros(B, n, d, dtype=dt, device=DEV)
        h.attention(qd, qd[:, :, d:], qd[:, :, 2 * d:], out, variant=variant, **kw)
        outs.append(out.cpu().float())
    ref = _attn_ref(qkv[..., :d], qkv[..., d:2 * d], qkv[..., 2 * d:], heads, scale, qk_map, None)
    assert rel_l2(outs[1], ref) < 1e-3 and rel_l2(outs[1], outs[0]) < 3e-4


def test_attention_shared_scores_rejects_unsupported():
    h = hip()
    dh, heads, n, B = 80, 8, 64, 3
    d = heads * dh
    q = torch.zeros(B, n, 3 * d, dtype=torch.float16, device=DEV)
    out = torch.zeros(B, n, d, dtype=torch.float16, device=DEV)
    with pytest.raises(h.VFaceHipError):
        h.attention(q, q[:, :, d:], q[:, :, 2 * d:], out, B=1, v_sets=3, set_stride=1, heads=heads, n=n, nk=n, dh=dh,
                    ldq=3 * d, ldk=3 * d, ldv=3 * d, bsq=n * 3 * d, bsk=n * 3 * d, bsv=n * 3 * d, ldo=d, bso=n * d,
                    scale=1.0)


@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("C", [64, 320, 640, 1280])
def test_layernorm(dt, C):
    h = hip()
    M = 77
    x = rnd((M, C), 1, dt, 2.0) + 0.5
    g, b = rnd((C,), 2, torch.float32) * 0.1 + 1, rnd((C,), 3, torch.float32) * 0.1
    out = torch.empty(M, C, dtype=dt, device=DEV)
    h.layernorm(x.to(DEV), g.to(DEV), b.to(DEV), out, M=M, C_=C, ldx=C, ldy=C)
    ref = F.layer_norm(x.float(), (C,), g, b, 1e-5)
    assert rel_l2(out.cpu().float(), ref) < TOL[dt]


@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("C,hw,silu,eps", [(64, 100, True, 1e-5), (320, 4096, True, 1e-5), (960, 256, True, 1e-5),
                                           (1280, 64, False, 1e-6), (2560, 64, True, 1e-5)])
def test_groupnorm(dt, C, hw, silu, eps):
    h = hip()
    nimg = 3
    x = rnd((nimg, hw, C), 1, dt, 1.5) + 0.3
    g, b = rnd((C,), 2, torch.float32) * 0.1 + 1, rnd((C,), 3, torch.float32) * 0.1
    xd = x.to(DEV)
    st = h.groupnorm_stats(xd, nimg=nimg, hw=hw, C_=C, ldx=C, eps=eps)
    out = torch.empty_like(xd)
    h.groupnorm_apply(xd, st, g.to(DEV), b.to(DEV), out, nimg=nimg, hw=hw, C_=C, ldx=C, ldy=C, silu=silu)
    ref = F.group_norm(x.float().permute(0, 2, 1), 32, g, b, eps)
    if silu:
        ref = F.silu(ref)
    assert rel_l2(out.cpu().float().permute(0, 2, 1), ref) < TOL[dt]


def _flow_cases():
    import os, sys
    sys.path.insert(0, os.path.join(os.path.dirname(__file__), "golden"))
    from cases import make_flows
    return {k: torch.from_numpy(v) for k, v in make_flows(64, 64).items()}


def test_flow_warp_indices_bit_exact_vs_reference_golden():
    """The integer gather indices must equal the reference's bit for bit (north-star); values to fp16 rounding."""
    h = hip()
    from vface_amd.utils import synth
    g = load_golden("warp")
    cases = _flow_cases()
    names = list(cases)
    img = synth.synth_normal("warp.img", (3, 8, 64, 64), seed=3)[0]  # [8,64,64]
    F_ = len(names) + 1
    src = img.permute(1, 2, 0).reshape(1, 4096, 8).repeat(F_, 1, 1).half().to(DEV)
    flow = torch.stack([cases[n] for n in names]).to(DEV)
    dst = torch.empty_like(src)
    x0 = torch.empty(F_ - 1, 64, 64, dtype=torch.int32, device=DEV)
    y0 = torch.empty_like(x0)
    h.flow_warp(src, dst, flow, F=F_, h=64, w=64, C_=8, ld_src=8, fs_src=4096 * 8, ld_dst=8, fs_dst=4096 * 8,
                alpha=0.0, dbg_x0=x0, dbg_y0=y0)
    for i, n in enumerate(names):
        assert torch.equal(x0[i].cpu(), g[f"x0_{n}"]), n
        assert torch.equal(y0[i].cpu(), g[f"y0_{n}"]), n
        got = dst[i + 1].cpu().float().reshape(64, 64, 8).permute(2, 0, 1)
        assert (got - g[f"warp_{n}"]).abs().max() < 4e-3, n  # fp16 in/out of O(1) values
    assert torch.equal(dst[0], src[0])


def test_flow_warp_align_matches_oracle_with_halo():
    h = hip()
    from oracle import flow as oflow
    from vface_amd.utils import synth
    F_, C, hh, ww = 4, 64, 64, 64
    x = synth.synth_normal("warp.align", (F_ + 1, C, hh, ww), seed=5).half()
    fl = synth.synth_flow(F_, hh, ww, seed=9)
    ref = oflow.align_by_flow(x, [fl[i] for i in range(F_)], 0.8)  # frames 1.. are the shard, frame 0 the halo
    tok = lambda t: t.permute(0, 2, 3, 1).reshape(t.shape[0], hh * ww, C).contiguous()
    src = tok(x[1:]).to(DEV)
    dst = torch.empty_like(src)
    h.flow_warp(src, dst, fl[1:].contiguous().to(DEV), F=F_, h=hh, w=ww, C_=C, ld_src=C, fs_src=hh * ww * C, ld_dst=C,
                fs_dst=hh * ww * C, alpha=0.8, prev=tok(x[:1])[0].to(DEV), ld_prev=C, flow_prev=fl[0].contiguous().to(DEV))
    got = dst.cpu().float()
    assert rel_l2(got, tok(ref[1:]).float()) < 6e-4
    # bit-identical to the oracle run at the same (fp16) storage type
    assert (got - tok(ref[1:]).float()).abs().max() <= 2e-3


@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("M,N,K,silu,f32", [(24, 1280, 1280, True, False), (24, 20160, 1280, False, True), (48, 1280, 640, True, False),
                                            (96, 640, 320, False, True), (5, 64, 320, True, True), (33, 96, 1280, False, False)])
def test_linear_small_vs_torch_and_vs_gemm(dt, M, N, K, silu, f32):
    """csrc/linear_small.hip (``vface_linear_small``): Linear (+ SiLU) on a handful of rows -- the time-embedding chain
    (openaimodel.py:874-875, 264-271) -- against fp64 torch on the same 16-bit operands and against vface_gemm (+ vface_silu);
    ragged row counts, up to three row tiles, outputs into a column slice of a wider buffer."""
    h = hip()
    a, w, b = rnd((M, K), 61, dt, 1.0), rnd((N, K), 62, dt, K ** -0.5), rnd((N,), 63, torch.float32, 0.3)
    odt = torch.float32 if f32 else dt
    out = torch.full((M + 3, N + 8), 7.0, dtype=odt, device=DEV)
    h.linear_small(a.to(DEV), w.to(DEV), b.to(DEV), out[:M, :N], M=M, N=N, K=K, silu=silu)
    ref = a.double() @ w.double().t() + b.double()
    if silu:
        ref = F.silu(ref)
    got = out[:M, :N].cpu().double()
    assert rel_l2(got, ref) < (2e-6 if f32 else TOL[dt])
    assert bool((out[M:] == 7.0).all()) and bool((out[:, N:] == 7.0).all())
    # the launches it replaces: the tiled GEMM (fp32 out), then SiLU
    g = torch.zeros(M, N, dtype=torch.float32, device=DEV)
    h.gemm(a.to(DEV), w.to(DEV), g, M=M, N=N, K=K, lda=K, ldc=N, bias=b.to(DEV), flags=h.EPI_OUT_F32)
    g = F.silu(g) if silu else g
    assert rel_l2(got, g.cpu().double()) < (2e-6 if f32 else TOL[dt])
    assert h.linear_small_supported(M, N, K) and not h.linear_small_supported(97, N, K) and not h.linear_small_supported(M, N + 8, K) \
        and not h.linear_small_supported(M, N, 512)
    with pytest.raises(h.VFaceHipError):
        h.linear_small(a.to(DEV), w.to(DEV), b.to(DEV), out[:M, :N], M=97, N=N, K=K)


def test_timestep_embedding_pack_and_ddim():
    h = hip()
    from oracle import ddim as oddim
    from oracle import unet as ounet
    t = torch.tensor([1, 481, 981, 21], dtype=torch.int64)
    out = torch.empty(4, 320, dtype=torch.float16, device=DEV)
    h.timestep_embedding(t.to(DEV), out, 320)
    assert (out.cpu().float() - ounet.timestep_embedding(t, 320)).abs().max() < 2e-3
    F_, hh, ww = 2, 8, 8
    x, inv, inp = rnd((F_, 4, hh, ww), 1, torch.float32), rnd((F_, 4, hh, ww), 2, torch.float32), rnd((F_, 4, hh, ww), 3, torch.float32)
    mask = (rnd((F_, 1, hh, ww), 4, torch.float32) > 0).float()
    packed = torch.empty(3 * F_, hh * ww, 16, dtype=torch.float16, device=DEV)
    h.pack_unet_input(x.to(DEV), inv.to(DEV), inp.to(DEV), mask.to(DEV), packed, F=F_, h=hh, w=ww, cpad=16)
    x9, r9 = torch.cat([x, inp, mask], 1), torch.cat([inv, inp, mask], 1)
    ref = torch.cat([x9, x9, r9], 0).permute(0, 2, 3, 1).reshape(3 * F_, hh * ww, 9)
    got = packed.cpu().float()
    assert (got[..., :9] - ref.half().float()).abs().max() == 0 and got[..., 9:].abs().max() == 0
    eps = rnd((3 * F_, 4, hh, ww), 5, torch.float32)
    eps_nhwc = eps.permute(0, 2, 3, 1).reshape(3 * F_ * hh * ww, 4).contiguous().to(DEV)
    sch = oddim.Schedule(50)
    idx = 30
    xp, p0 = torch.empty_like(x, device=DEV), torch.empty_like(x, device=DEV)
    h.ddim_step(eps_nhwc, x.to(DEV), inv.to(DEV), xp, F=F_, C_=4, hw=hh * ww, lde=4, scale=3.0,
                a_t=float(sch.alphas[idx]), a_prev=float(sch.alphas_prev[idx]), sigma_t=0.0,
                sqrt_one_minus_at=float(sch.sqrt_one_minus_alphas[idx]), pred_x0=p0)
    e_u, e_c, e_r = eps.chunk(3)
    e_t, _ = oddim.cfg_combine(e_u, e_c, e_r, 3.0)
    rx, rp = oddim.ddim_update(x, e_t, float(sch.alphas[idx]), float(sch.alphas_prev[idx]), 0.0,
                               float(sch.sqrt_one_minus_alphas[idx]))
    # fp32 on both sides; the device contracts a*b+c into FMAs, so allow a few ulp
    assert torch.allclose(xp.cpu(), rx, rtol=2e-6, atol=2e-6) and torch.allclose(p0.cpu(), rp, rtol=2e-6, atol=2e-6)


@pytest.mark.parametrize("mode", ["plain", "replace", "fft", "flow_fix"])
def test_engine_attn1_sequence_level0_vs_reference_golden(mode):
    """The hooked attn1 as the engine sequences it (UNetEngine._attn1: _attn1_att + _attn1_out, 16-bit output, no residual) at the real
    level-0 shape (d=320, 8 heads, n=4096, F=2) against the reference-generated fixture (strided token slice)."""
    from vface_amd.engine import HookCfg, UNetEngine, plan_fusion
    from vface_amd.packing import pack_qkv
    from vface_amd.utils import synth
    g = load_golden("attn_module")
    F_, n, d, heads = 2, 4096, 320, 8
    B = 3 * F_
    sd = synth.synth_state_dict({"attn1.to_q.weight": (d, d), "attn1.to_k.weight": (d, d),
                                 "attn1.to_v.weight": (d, d), "attn1.to_out.0.weight": (d, d),
                                 "attn1.to_out.0.bias": (d,)})
    x = synth.synth_normal("attnmod.x", (B, n, d)).half().to(DEV).reshape(B * n, d)
    eng = UNetEngine(None, torch.float16, device=DEV)
    p = {"c": d, "wqkv": pack_qkv(sd["attn1.to_q.weight"], sd["attn1.to_k.weight"], sd["attn1.to_v.weight"]).half().to(DEV),
         "wo": {"w": sd["attn1.to_out.0.weight"].half().to(DEV), "b": sd["attn1.to_out.0.bias"].to(DEV)},
         "wlin": {}, "qk_src": (sd["attn1.to_q.weight"], sd["attn1.to_k.weight"])}
    flow = synth.synth_flow(F_ - 1, 64, 64).to(DEV) if mode == "flow_fix" else None
    cfg = None if mode == "plain" else HookCfg(chunks=3, fusion=mode, flow=flow, split_ratio_fft=0.8, alpha=0.8)
    pl = plan_fusion(cfg, B, n)
    out = torch.empty(B * n, d, dtype=torch.float16, device=DEV)
    eng._attn1(x, None, p, pl, None, B, n, heads, out=out)
    assert rel_l2(out.reshape(B, n, d)[:, ::128].cpu().float(), g[mode]) < 1e-3


@pytest.mark.parametrize("mode", ["temporal", "adaIn"])
def test_engine_attn1_staged_plan_is_its_launches_by_hand_split_k_included(mode):
    """The staged hook modes through ``UNetEngine._attn1`` (a stand-alone attention: no row bias, no residual) at d = 1280, 8 heads,
    n = 64, B = 6 (three chunks of two frames) == the same launches written out here: the q|k|v projection and the out-projection
    with ``hip.gemm``'s default split-K (the other plans launch theirs without), the edit kernels, ``qkv_attention`` without maps.
    This is the smallest shape at which the staged out-projection really splits K (asserted), so a lost flag changes the bits."""
    h = hip()
    from vface_amd.engine import HookCfg, UNetEngine, plan_fusion, qkv_attention
    d, heads, n, B = 1280, 8, 64, 6
    assert h.load().vface_splitk_workspace_bytes(384, 1280, 1280, 0, 64) > 0
    dt = torch.float16
    x = rnd((B * n, d), 1, dt).to(DEV)
    wqkv, wo = rnd((3 * d, d), 2, dt, 1 / math.sqrt(d)).to(DEV), rnd((d, d), 3, dt, 1 / math.sqrt(d)).to(DEV)
    bo = rnd((d,), 4, torch.float32, 0.1).to(DEV)
    eng = UNetEngine(None, dt, device=DEV)
    p = {"c": d, "wqkv": wqkv, "wo": {"w": wo, "b": bo}, "wlin": {}, "qk_src": None}
    pl = plan_fusion(HookCfg(chunks=3, fusion=mode), B, n)
    assert pl["staged"] == mode
    got = torch.empty(B * n, d, dtype=dt, device=DEV)
    eng._attn1(x, None, p, pl, None, B, n, heads, out=got)

    Fn = B // 3 * n
    qkv = torch.empty(B * n, 3 * d, dtype=dt, device=DEV)
    h.gemm(x, wqkv, qkv, M=B * n, N=3 * d, K=d, lda=d, ldc=3 * d)
    if mode == "temporal":
        h.temporal_gauss(qkv, qkv[Fn:], qkv[2 * Fn:], F=B // 3, n=n, C_=2 * d, ld_src=3 * d, fs_src=n * 3 * d, ld_dst=3 * d,
                         fs_dst=n * 3 * d)
    else:
        for col in (0, d):
            for ch in (1, 2):
                own = qkv[ch * Fn:(ch + 1) * Fn, col:col + d]
                h.adain_fusion(qkv[:Fn, col:col + d], own, own, rows=Fn, C_=d, lda=3 * d, ldb=3 * d, ldd=3 * d)
    att = torch.empty(B * n, d, dtype=dt, device=DEV)
    qkv_attention(qkv, att, B=B, n=n, d=d, heads=heads)
    want = torch.empty(B * n, d, dtype=dt, device=DEV)
    h.gemm(att, wo, want, M=B * n, N=d, K=d, lda=d, ldc=d, bias=bo, rows_per_sample=n)
    assert torch.isfinite(want.float()).all() and torch.equal(got, want)


@pytest.mark.parametrize("N_,cout", [(2, 320), (3, 640)])
def test_conv_colstats_feed_groupnorm(N_, cout):
    """Producer-side column statistics (conv epilogue) -> GroupNorm mean/rstd, against the stand-alone statistics kernel
    and torch."""
    h = hip()
    from vface_amd.packing import pack_conv3x3
    dt = torch.float16
    cin, H = 64, 16
    x = rnd((N_, cin, H, H), 1, dt)
    w = rnd((cout, cin, 3, 3), 2, dt, 1 / math.sqrt(9 * cin))
    b = rnd((cout,), 3, torch.float32, 0.1)
    xn = x.permute(0, 2, 3, 1).contiguous().to(DEV)
    wide = torch.zeros(N_ * H * H, cout + 64, dtype=dt, device=DEV)       # the conv writes a column slice of a wider buffer
    cs = torch.zeros(N_ * H * H // 64, cout + 64, 2, dtype=torch.float32, device=DEV)
    h.conv3x3(xn, pack_conv3x3(w).to(DEV), wide[:, 32:], nimg=N_, H=H, W=H, cin=cin, cout=cout, ldx=cin, ldy=cout + 64,
              bias=b.to(DEV), colstats=cs[:, 32:32 + cout])
    y = wide[:, 32:32 + cout]
    st_cols = h.groupnorm_stats_from_cols(cs[:, 32:32 + cout], nimg=N_, hw=H * H, C_=cout)
    st_ref = h.groupnorm_stats(y, nimg=N_, hw=H * H, C_=cout, ldx=cout + 64)
    assert torch.allclose(st_cols, st_ref, rtol=2e-4, atol=2e-5)
    yf = y.float().cpu().reshape(N_, H * H, 32, cout // 32)
    mean = yf.mean(dim=(1, 3))
    assert torch.allclose(st_cols[..., 0].cpu(), mean, atol=2e-4)
    assert cs[:, :32].abs().max() == 0 and cs[:, 32 + cout:].abs().max() == 0


@pytest.mark.parametrize("C,H,nimg,eps", [(320, 64, 3, 1e-5), (640, 32, 2, 1e-5), (1280, 8, 5, 1e-6), (2560, 16, 2, 1e-5),
                                          (64, 8, 1, 1e-5), (1920, 32, 1, 1e-5)])
def test_groupnorm_stats_and_coeffs_from_cols(C, H, nimg, eps):
    """gn_finalize_cols / gn_coeffs_cols against fp64 sums of the same column statistics (laid out as a column slice of a
    wider buffer), and the two kernels against each other bit for bit (one summation order: the fused SpatialTransformer front
    and the fused-GroupNorm convolution apply the coefficients gn_apply would have formed)."""
    h = hip()
    hw = H * H
    x = (rnd((nimg * hw, C), 11, torch.float32, 1.5) + 0.3).to(DEV)
    sl = x.reshape(nimg * hw // 64, 64, C)
    cs_wide = torch.zeros(nimg * hw // 64, C + 16, 2, dtype=torch.float32, device=DEV)
    cs = cs_wide[:, 8:8 + C]
    cs[..., 0] = sl.sum(1)
    cs[..., 1] = (sl * sl).sum(1)
    st = h.groupnorm_stats_from_cols(cs, nimg=nimg, hw=hw, C_=C, eps=eps)
    c64 = cs.double().cpu().reshape(nimg, hw // 64, 32, C // 32, 2).sum(dim=(1, 3))
    cnt = hw * (C // 32)
    mean = c64[..., 0] / cnt
    rstd = 1.0 / torch.sqrt((c64[..., 1] / cnt - mean * mean).clamp_min(0) + eps)
    assert torch.allclose(st[..., 0].cpu().double(), mean, rtol=1e-6, atol=1e-7)
    assert torch.allclose(st[..., 1].cpu().double(), rstd, rtol=1e-6, atol=1e-7)
    g = rnd((C,), 12, torch.float32, 0.5).to(DEV) + 1.0
    b = rnd((C,), 13, torch.float32, 0.2).to(DEV)
    ab = h.groupnorm_coeffs_from_cols(cs, g, b, nimg=nimg, hw=hw, C_=C, eps=eps)
    a_ref = st[..., 1].repeat_interleave(C // 32, 1) * g[None]
    assert torch.equal(ab[..., 0], a_ref)
    # (the kernel contracts beta - mean * a into one fused multiply-add: last-bit differences against the two-step form)
    assert torch.allclose(ab[..., 1], b[None] - st[..., 0].repeat_interleave(C // 32, 1) * a_ref, rtol=1e-6, atol=1e-7)


@pytest.mark.gpu
@pytest.mark.parametrize("cin,cout,H,nimg", [(1280, 1280, 8, 6), (640, 320, 8, 5), (2560, 1280, 8, 3)])
def test_conv3x3_split_k(cin, cout, H, nimg):
    """Shapes whose tile grid underfills the chip run split-K (fp32 partials + reduce pass with the epilogue): same
    result as the one-pass launch up to the fp32 summation order, same column statistics contract."""
    h = hip()
    from vface_amd.packing import pack_conv3x3
    dt = torch.float16
    M = nimg * H * H
    assert h.load().vface_splitk_workspace_bytes(M, cout, 9 * cin, 0, H * H) > 0
    x = rnd((nimg, cin, H, H), 1, dt)
    w = rnd((cout, cin, 3, 3), 2, dt, 1 / math.sqrt(9 * cin))
    b = rnd((cout,), 3, torch.float32, 0.1)
    rb = rnd((nimg, cout), 4, torch.float32)
    res = rnd((nimg, H, H, cout), 5, dt)
    ref = F.conv2d(x.float(), w.float(), b, padding=1) + rb[:, :, None, None] + res.float().permute(0, 3, 1, 2)
    xn = x.permute(0, 2, 3, 1).contiguous().to(DEV)
    wp = pack_conv3x3(w).to(DEV)
    outs, stats = [], []
    for split in (True, False):
        out = torch.empty(nimg, H, H, cout, dtype=dt, device=DEV)
        cs = torch.zeros(M // 64, cout, 2, dtype=torch.float32, device=DEV)
        h.conv3x3(xn, wp, out, nimg=nimg, H=H, W=H, cin=cin, cout=cout, ldx=cin, ldy=cout, bias=b.to(DEV),
                  rowbias=rb.to(DEV), residual=res.to(DEV), ldr=cout, colstats=cs, split_k=split)
        assert rel_l2(out.cpu().float().permute(0, 3, 1, 2), ref) < TOL[dt]
        outs.append(out); stats.append(cs)
        yf = out.float().reshape(M // 64, 64, cout)
        assert torch.allclose(cs[..., 0], yf.sum(1), rtol=1e-4, atol=1e-2)
        assert torch.allclose(cs[..., 1], (yf * yf).sum(1), rtol=1e-4, atol=1e-2)
    assert rel_l2(outs[0].float().cpu(), outs[1].float().cpu()) < 5e-4
    again = torch.empty_like(outs[0])
    h.conv3x3(xn, wp, again, nimg=nimg, H=H, W=H, cin=cin, cout=cout, ldx=cin, ldy=cout, bias=b.to(DEV),
              rowbias=rb.to(DEV), residual=res.to(DEV), ldr=cout)
    assert torch.equal(again, outs[0])        # fixed summation order: reproducible


@pytest.mark.gpu
def test_gemm_split_k_plain():
    h = hip()
    dt = torch.float16
    M, N, K = 1536, 1280, 2560
    assert h.load().vface_splitk_workspace_bytes(M, N, K, 0, 1) > 0
    a = rnd((M, K), 1, dt)
    w = rnd((N, K), 2, dt, 1 / math.sqrt(K))
    b = rnd((N,), 3, torch.float32, 0.1)
    res = rnd((M, N), 4, dt)
    ref = a.float() @ w.float().t() + b + res.float()
    out = torch.empty(M, N, dtype=dt, device=DEV)
    h.gemm(a.to(DEV), w.to(DEV), out, M=M, N=N, K=K, lda=K, ldc=N, bias=b.to(DEV), residual=res.to(DEV), ldr=N)
    assert rel_l2(out.cpu().float(), ref) < TOL[dt]


@pytest.mark.gpu
@pytest.mark.parametrize("M,N,K,geglu", [(70000, 320, 320, False), (66000, 1280, 320, True), (40000, 640, 192, False)])
def test_gemm_persistent_matches_one_tile_per_workgroup(M, N, K, geglu):
    """More tiles than resident workgroups -> the persistent kernel (K pipeline running across tiles).  Same arithmetic in
    the same order as the one-tile-per-workgroup launch: bit-identical outputs and column statistics."""
    h = hip()
    from vface_amd.packing import pack_geglu
    dt = torch.float16
    a = rnd((M, K), 1, dt).to(DEV)
    w = rnd((N, K), 2, dt, 1 / math.sqrt(K))
    b = rnd((N,), 3, torch.float32, 0.1)
    nout = N // 2 if geglu else N
    res = None if geglu else rnd((M, nout), 4, dt).to(DEV)
    rb = None if geglu else rnd(((M + 4095) // 4096, nout), 5, torch.float32).to(DEV)
    if geglu:
        w, b = pack_geglu(w, b)
    outs = []
    for flags in (h.TUNE_PERSISTENT, h.TUNE_NO_PERSISTENT):
        out = torch.zeros(M, nout, dtype=dt, device=DEV)
        cs = None if geglu else torch.zeros((M + 63) // 64, nout, 2, dtype=torch.float32, device=DEV)
        h.gemm(a, w.to(DEV), out, M=M, N=N, K=K, lda=K, ldc=nout, bias=b.to(DEV), residual=res, ldr=nout,
               rowbias=rb, rows_per_sample=4096, flags=flags | (h.EPI_GEGLU if geglu else 0), colstats=cs)
        outs.append((out, cs))
    assert torch.equal(outs[0][0], outs[1][0])
    if not geglu:
        assert torch.equal(outs[0][1], outs[1][1])
        ref = a[:4096].float().cpu() @ w.float().t() + b + rb[0].cpu() + res[:4096].float().cpu()
        assert rel_l2(outs[0][0][:4096].float().cpu(), ref) < TOL[dt]


@pytest.mark.gpu
def test_conv_persistent_matches_one_tile_per_workgroup():
    h = hip()
    from vface_amd.packing import pack_conv3x3
    dt = torch.float16
    nimg, H, cin, cout = 20, 64, 64, 160          # 640 m-tiles x 1 n-tile
    x = rnd((nimg, H, H, cin), 1, dt).to(DEV)
    w = pack_conv3x3(rnd((cout, cin, 3, 3), 2, dt, 1 / math.sqrt(9 * cin))).to(DEV)
    b = rnd((cout,), 3, torch.float32, 0.1).to(DEV)
    outs = []
    for flags in (0, h.TUNE_NO_PERSISTENT):
        out = torch.zeros(nimg, H, H, cout, dtype=dt, device=DEV)
        cs = torch.zeros(nimg * H * H // 64, cout, 2, dtype=torch.float32, device=DEV)
        h.conv3x3(x, w, out, nimg=nimg, H=H, W=H, cin=cin, cout=cout, ldx=cin, ldy=cout, bias=b, colstats=cs, flags=flags)
        outs.append((out, cs))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    ref = F.conv2d(x[:1].float().cpu().permute(0, 3, 1, 2), rnd((cout, cin, 3, 3), 2, dt, 1 / math.sqrt(9 * cin)).float(),
                   b.cpu(), padding=1)
    assert rel_l2(outs[0][0][:1].float().cpu().permute(0, 3, 1, 2), ref) < TOL[dt]


@pytest.mark.gpu
@pytest.mark.parametrize("dh,n", [(40, 640), (80, 256)])
def test_attention_wide_logit_range(dh, n):
    """Peaked softmax rows (logit std > 10, row maxima that keep rising along the key walk): the lazily raised reference of
    the default softmax form must track them -- compared with fp64 and with the exact-scale form of the kernel."""
    h = hip()
    dt = torch.float16
    B, heads = 2, 8
    d = heads * dh
    qkv = rnd((B, n, 3 * d), 21, dt)
    ramp = torch.linspace(0.5, 3.5, n).reshape(1, n, 1)          # later keys are larger: the running max keeps moving
    qkv[..., :d] *= 6.0
    qkv[..., d:2 * d] = (qkv[..., d:2 * d].float() * ramp).to(dt)
    qd = qkv.to(DEV)
    scale = dh ** -0.5
    kw = dict(B=B, heads=heads, n=n, nk=n, dh=dh, ldq=3 * d, ldk=3 * d, ldv=3 * d, bsq=n * 3 * d, bsk=n * 3 * d, bsv=n * 3 * d,
              ldo=d, bso=n * d, scale=scale)
    outs = []
    for variant in (0, 2):
        out = torch.zeros(B, n, d, dtype=dt, device=DEV)
        h.attention(qd, qd[:, :, d:], qd[:, :, 2 * d:], out, variant=variant, **kw)
        assert torch.isfinite(out).all()
        outs.append(out.float().cpu())
    sp = lambda t: t.reshape(B, n, heads, dh).permute(0, 2, 1, 3).double()
    s = sp(qkv[..., :d]) @ sp(qkv[..., d:2 * d]).transpose(-1, -2) * scale
    assert s.std() > 10
    ref = (torch.softmax(s, -1) @ sp(qkv[..., 2 * d:])).permute(0, 2, 1, 3).reshape(B, n, d).float()
    assert rel_l2(outs[0], ref) < 2e-3 and rel_l2(outs[1], ref) < 2e-3     # peaked rows amplify the fp16 rounding of q, k
    assert rel_l2(outs[0], outs[1]) < 2e-3


@pytest.mark.gpu
@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("cin,cout,H,W", [(64, 64, 8, 8), (128, 160, 12, 10), (640, 640, 16, 16), (24, 32, 6, 7),
                                          (64, 64, 160, 152)])   # the last one: 570 tiles per phase -> persistent form
def test_upsample_conv_as_parity_phases(dt, cin, cout, H, W):
    """conv3x3(nearest x2 upsample) as four 2x2 parity-phase convolutions with pre-summed taps: equals the direct form
    (the fused-upsample implicit GEMM and torch) -- 4/9 of the multiply-adds."""
    h = hip()
    from vface_amd.packing import pack_conv3x3, pack_upsample_phases
    nimg = 3
    x = rnd((nimg, cin, H, W), 1, dt)
    w = rnd((cout, cin, 3, 3), 2, dt, 1 / math.sqrt(9 * cin))
    b = rnd((cout,), 3, torch.float32, 0.1)
    rb = rnd((nimg, cout), 4, torch.float32)
    ref = F.conv2d(F.interpolate(x.float(), scale_factor=2, mode="nearest"), w.float(), b, padding=1) + rb[:, :, None, None]
    cp = (cin + 7) // 8 * 8
    xn = torch.zeros(nimg, H, W, cp, dtype=dt)
    xn[..., :cin] = x.permute(0, 2, 3, 1)
    xn = xn.to(DEV)
    out = torch.zeros(nimg, 2 * H, 2 * W, cout, dtype=dt, device=DEV)
    h.upsample2x_conv3x3(xn, pack_upsample_phases(w.float()).to(dt).to(DEV), out, nimg=nimg, H=H, W=W, cin=cp, cout=cout, ldx=cp,
                         ldy=cout, bias=b.to(DEV), rowbias=rb.to(DEV))
    assert rel_l2(out.cpu().float().permute(0, 3, 1, 2), ref) < TOL[dt]
    direct = torch.zeros_like(out)
    h.conv3x3(xn, pack_conv3x3(w).to(DEV), direct, nimg=nimg, H=H, W=W, cin=cp, cout=cout, ldx=cp, ldy=cout, upsample=True,
              bias=b.to(DEV), rowbias=rb.to(DEV))
    assert rel_l2(out.float().cpu(), direct.float().cpu()) < TOL[dt]
    if (H * W) % 64 == 0:
        # column statistics of the phase launches feed the same GroupNorm statistics as the stand-alone kernel
        cs = torch.zeros(nimg * 4 * H * W // 64, cout, 2, dtype=torch.float32, device=DEV)
        h.upsample2x_conv3x3(xn, pack_upsample_phases(w.float()).to(dt).to(DEV), out, nimg=nimg, H=H, W=W, cin=cp, cout=cout,
                             ldx=cp, ldy=cout, bias=b.to(DEV), rowbias=rb.to(DEV), colstats=cs)
        y = out.reshape(nimg * 4 * H * W, cout)
        st_cols = h.groupnorm_stats_from_cols(cs, nimg=nimg, hw=4 * H * W, C_=cout)
        st_ref = h.groupnorm_stats(y, nimg=nimg, hw=4 * H * W, C_=cout, ldx=cout)
        assert torch.allclose(st_cols, st_ref, rtol=3e-4, atol=3e-5)


@pytest.mark.gpu
@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("cin,c2,cout,H,nimg", [(64, 128, 64, 8, 3), (320, 960, 320, 16, 2), (1280, 2560, 1280, 8, 6),
                                                (64, 64, 64, 64, 20)])   # the last one: 640 tiles -> persistent form
def test_conv3x3_plus_1x1_shortcut(dt, cin, c2, cout, H, nimg):
    """A ResBlock's second conv with the 1x1 shortcut accumulated in the same K loop (also through split-K at 8x8)."""
    h = hip()
    from vface_amd.packing import pack_conv3x3
    x = rnd((nimg, cin, H, H), 1, dt)
    x2 = rnd((nimg, c2, H, H), 2, dt)
    w = rnd((cout, cin, 3, 3), 3, dt, 1 / math.sqrt(9 * cin))
    w2 = rnd((cout, c2), 4, dt, 1 / math.sqrt(c2))
    b = rnd((cout,), 5, torch.float32, 0.1)
    ref = F.conv2d(x.float(), w.float(), b, padding=1) + torch.einsum("nchw,oc->nohw", x2.float(), w2.float())
    wt = torch.cat([pack_conv3x3(w), w2], 1).contiguous().to(DEV)
    out = torch.zeros(nimg, H, H, cout, dtype=dt, device=DEV)
    cs = torch.zeros(nimg * H * H // 64, cout, 2, dtype=torch.float32, device=DEV)
    h.conv3x3_plus_1x1(x.permute(0, 2, 3, 1).contiguous().to(DEV), x2.permute(0, 2, 3, 1).contiguous().to(DEV), wt, out,
                       nimg=nimg, H=H, W=H, cin=cin, c2=c2, cout=cout, ldx=cin, ldx2=c2, ldy=cout, bias=b.to(DEV), colstats=cs)
    assert rel_l2(out.cpu().float().permute(0, 3, 1, 2), ref) < TOL[dt]
    yf = out.float().reshape(nimg * H * H // 64, 64, cout)
    assert torch.allclose(cs[..., 0], yf.sum(1), rtol=1e-4, atol=2e-2)


# ------------------------------------------------------------------------------------------ fp32 residual stream
@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("M,N,K,want16", [(1000, 320, 320, True), (4096, 640, 640, False), (130, 72, 64, True)])
def test_gemm_fp32_residual_stream(dt, M, N, K, want16):
    """vface_stream32: the residual is read in fp32, the un-rounded sum is stored as fp32 (the carrier) and -- when
    asked for -- its single rounding as the 16-bit copy; column statistics are those of the fp32 values."""
    h = hip()
    a, w = rnd((M, K), 1, dt), rnd((N, K), 2, dt, 1 / math.sqrt(K))
    bias, res32 = rnd((N,), 3, torch.float32), rnd((M, N), 4, torch.float32)
    out32 = torch.empty(M, N, dtype=torch.float32, device=DEV)
    out16 = torch.empty(M, N, dtype=dt, device=DEV) if want16 else None
    cs = torch.zeros((M + 63) // 64, N, 2, dtype=torch.float32, device=DEV) if M % 64 == 0 else None
    h.gemm(a.to(DEV), w.to(DEV), out16, M=M, N=N, K=K, lda=K, ldc=N, bias=bias.to(DEV), residual32=res32.to(DEV),
           out32=out32, colstats=cs)
    ref = a.double() @ w.double().t() + bias.double() + res32.double()
    assert rel_l2(out32.cpu(), ref) < 2e-6          # fp32 accumulate of exact 16-bit products, fp32 epilogue
    if want16:
        assert torch.equal(out16.cpu(), out32.cpu().to(dt))   # one rounding of the very same sum
    if cs is not None:
        o = out32.cpu().double().reshape(M // 64, 64, N)
        assert rel_l2(cs[..., 0].cpu(), o.sum(1)) < 1e-5 and rel_l2(cs[..., 1].cpu(), (o * o).sum(1)) < 1e-5


def test_conv_fp32_residual_stream_and_split_k():
    """The same through the implicit-GEMM convolution, incl. a split-K shape (the 8x8 level) and the fused 1x1 shortcut."""
    h = hip()
    dt = torch.float16
    for cin, cout, H, nimg in ((64, 64, 16, 2), (1280, 1280, 8, 6)):
        x = rnd((nimg, cin, H, H), 1, dt)
        wt = rnd((cout, cin, 3, 3), 2, dt, 1 / math.sqrt(9 * cin))
        bias, res32 = rnd((cout,), 3, torch.float32), rnd((nimg * H * H, cout), 4, torch.float32)
        from vface_amd import packing
        xn = x.permute(0, 2, 3, 1).reshape(-1, cin).contiguous().to(DEV)
        wp = packing.pack_conv3x3(wt.float()).to(dt).to(DEV)
        out32 = torch.empty(nimg * H * H, cout, dtype=torch.float32, device=DEV)
        out16 = torch.empty(nimg * H * H, cout, dtype=dt, device=DEV)
        h.conv3x3(xn, wp, out16, nimg=nimg, H=H, W=H, cin=cin, cout=cout, ldx=cin, ldy=cout, bias=bias.to(DEV),
                  residual32=res32.to(DEV), out32=out32)
        ref = F.conv2d(x.double(), wt.double(), bias.double(), padding=1).permute(0, 2, 3, 1).reshape(-1, cout) + res32.double()
        assert rel_l2(out32.cpu(), ref) < 3e-6, (cin, cout)
        assert torch.equal(out16.cpu(), out32.cpu().to(dt))


@pytest.mark.parametrize("C", [320, 1280])
def test_norms_read_the_fp32_stream(C):
    """LayerNorm / GroupNorm statistics + apply on an fp32 input equal the fp32 torch result to 16-bit rounding."""
    h = hip()
    dt = torch.float16
    M, hw, nimg = 512, 256, 2
    x = rnd((M, C), 1, torch.float32)
    gm, bt = 1 + 0.1 * rnd((C,), 2, torch.float32), 0.1 * rnd((C,), 3, torch.float32)
    y = torch.empty(M, C, dtype=dt, device=DEV)
    h.layernorm(x.to(DEV), gm.to(DEV), bt.to(DEV), y, M=M, C_=C, ldx=C, ldy=C)
    assert rel_l2(y.cpu().float(), F.layer_norm(x, (C,), gm, bt, 1e-5)) < 4e-4
    st = h.groupnorm_stats(x.to(DEV), nimg=nimg, hw=hw, C_=C, ldx=C)
    h.groupnorm_apply(x.to(DEV), st, gm.to(DEV), bt.to(DEV), y, nimg=nimg, hw=hw, C_=C, ldx=C, ldy=C, silu=True)
    ref = F.silu(F.group_norm(x.reshape(nimg, hw, C).permute(0, 2, 1), 32, gm, bt, 1e-5)).permute(0, 2, 1).reshape(M, C)
    assert rel_l2(y.cpu().float(), ref) < 4e-4


# ------------------------------------------------------------------------------------------ patch-staged convolution
def _gn_sums(cs, nimg):
    """per-sample, per-channel (sum, sumsq) from a colstats buffer [slices, C, 2] (slice order inside a sample is free)"""
    return cs.reshape(nimg, -1, cs.shape[1], 2).double().sum(1)


@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("cin,cout,H,W,nimg", [(64, 160, 16, 16, 2), (320, 320, 32, 16, 3), (128, 128, 48, 48, 1),
                                               (640, 640, 16, 32, 2), (64, 256, 64, 64, 2)])
def test_conv_patch_kernel_equals_im2col_kernel_bit_for_bit(dt, cin, cout, H, W, nimg):
    """conv.hip (every pixel staged once per 64-channel chunk, 16x16-pixel tiles, 8 waves) against gemm.hip's implicit GEMM
    (one LDS load per tap): same K order and per-accumulator MFMA order -> the same bits; and both against torch."""
    h = hip()
    from vface_amd.packing import pack_conv3x3
    x = rnd((nimg, cin, H, W), 1, dt)
    w = rnd((cout, cin, 3, 3), 2, dt, 1 / math.sqrt(9 * cin))
    b = rnd((cout,), 3, torch.float32, 0.1)
    rb = rnd((nimg, cout), 4, torch.float32)
    res = rnd((nimg * H * W, cout), 5, dt)
    ref = (F.conv2d(x.float(), w.float(), b, padding=1) + rb[:, :, None, None]).permute(0, 2, 3, 1).reshape(-1, cout) + res.float()
    xn = x.permute(0, 2, 3, 1).reshape(-1, cin).contiguous().to(DEV)
    wp = pack_conv3x3(w).to(DEV)
    outs, stats = [], []
    for flag in (h.TUNE_PATCH, h.TUNE_NO_PATCH):
        out = torch.zeros(nimg * H * W, cout + 32, dtype=dt, device=DEV)    # a column slice of a wider buffer
        cs = torch.zeros(nimg * H * W // 64, cout, 2, dtype=torch.float32, device=DEV)
        h.conv3x3(xn, wp, out[:, 16:], nimg=nimg, H=H, W=W, cin=cin, cout=cout, ldx=cin, ldy=cout + 32, bias=b.to(DEV),
                  rowbias=rb.to(DEV), residual=res.to(DEV), ldr=cout, flags=flag, colstats=cs, split_k=False)
        assert out[:, :16].abs().max() == 0 and out[:, 16 + cout:].abs().max() == 0
        outs.append(out[:, 16:16 + cout].cpu())
        stats.append(_gn_sums(cs.cpu(), nimg))
    assert rel_l2(outs[0].float(), ref) < TOL[dt]
    assert torch.equal(outs[0], outs[1])
    y = outs[0].double().reshape(nimg, H * W, cout)
    assert rel_l2(stats[0][..., 0], y.sum(1)) < 1e-5 and rel_l2(stats[0][..., 1], (y * y).sum(1)) < 1e-5
    assert rel_l2(stats[0], stats[1]) < 1e-5


def test_conv_patch_kernel_fp32_stream_shortcut_and_phases():
    """The other launch forms of the patch kernel: fp32 residual in / fp32 carrier out, the fused 1x1 shortcut (K tiles
    past the window), and the 2x2 parity-phase windows of an upsampling convolution -- each bit-identical to gemm.hip."""
    h = hip()
    from vface_amd.packing import pack_conv3x3, pack_upsample_phases
    dt = torch.float16
    cin, c2, cout, H, W, nimg = 128, 192, 320, 32, 32, 2
    x, x2 = rnd((nimg, cin, H, W), 1, dt), rnd((nimg * H * W, c2), 2, dt)
    w, w2 = rnd((cout, cin, 3, 3), 3, dt, 1 / math.sqrt(9 * cin)), rnd((cout, c2), 4, dt, 1 / math.sqrt(c2))
    b, res32 = rnd((cout,), 5, torch.float32, 0.1), rnd((nimg * H * W, cout), 6, torch.float32)
    xn = x.permute(0, 2, 3, 1).reshape(-1, cin).contiguous().to(DEV)
    got = {}
    for name, flag in (("patch", h.TUNE_PATCH), ("im2col", h.TUNE_NO_PATCH)):
        o16 = torch.zeros(nimg * H * W, cout, dtype=dt, device=DEV)
        o32 = torch.zeros(nimg * H * W, cout, dtype=torch.float32, device=DEV)
        h.conv3x3(xn, pack_conv3x3(w).to(DEV), o16, nimg=nimg, H=H, W=W, cin=cin, cout=cout, ldx=cin, ldy=cout, bias=b.to(DEV),
                  residual32=res32.to(DEV), out32=o32, flags=flag, split_k=False)
        s16 = torch.zeros_like(o16)
        s32 = torch.zeros_like(o32)
        cs = torch.zeros(nimg * H * W // 64, cout, 2, dtype=torch.float32, device=DEV)
        h.conv3x3_plus_1x1(xn, x2.to(DEV), torch.cat([pack_conv3x3(w), w2], 1).contiguous().to(DEV), s16, nimg=nimg, H=H, W=W,
                           cin=cin, c2=c2, cout=cout, ldx=cin, ldx2=c2, ldy=cout, bias=b.to(DEV), flags=flag, colstats=cs,
                           out32=s32, split_k=False)
        up = torch.zeros(nimg * 4 * H * W, cout, dtype=dt, device=DEV)
        ucs = torch.zeros(nimg * 4 * H * W // 64, cout, 2, dtype=torch.float32, device=DEV)
        h.upsample2x_conv3x3(xn, pack_upsample_phases(w.float()).to(dt).to(DEV), up, nimg=nimg, H=H, W=W, cin=cin, cout=cout,
                             ldx=cin, ldy=cout, bias=b.to(DEV), flags=flag, colstats=ucs)
        got[name] = [t.cpu() for t in (o16, o32, s16, s32, up)] + [_gn_sums(cs.cpu(), nimg), _gn_sums(ucs.cpu(), nimg)]
    conv = F.conv2d(x.double(), w.double(), b.double(), padding=1).permute(0, 2, 3, 1).reshape(-1, cout)
    assert rel_l2(got["patch"][1], conv + res32.double()) < 3e-6
    assert rel_l2(got["patch"][3], conv + x2.double() @ w2.double().t()) < 3e-6
    upref = F.conv2d(F.interpolate(x.float(), scale_factor=2, mode="nearest"), w.float(), b, padding=1)
    assert rel_l2(got["patch"][4].float().reshape(nimg, 2 * H, 2 * W, cout).permute(0, 3, 1, 2), upref) < 1e-3
    for a, c in zip(got["patch"][:5], got["im2col"][:5]):
        assert torch.equal(a, c)
    assert torch.equal(got["patch"][0], got["patch"][1].to(dt))
    for a, c in zip(got["patch"][5:], got["im2col"][5:]):
        assert rel_l2(a, c) < 1e-5
    y = got["patch"][3].double().reshape(nimg, H * W, cout)
    assert rel_l2(got["patch"][5][..., 0], y.sum(1)) < 1e-5


# ------------------------------------------------------------------------------------------ flow: CUDA-form indices, latent resample
def test_flow_warp_cuda_form_indices_vs_emulated_fixture():
    """flags bit 0 of vface_flow_warp (`cuda_recip_div`): the scalar division of the coordinate normalisation as CUDA ATen
    performs it (multiply by the fp32 reciprocal) -- what the reference computes on its native device.  Bit-exact against
    tests/golden/warp_cuda_form.npz, which the ORACLE's restatement of that rule produced ("CUDA-form, emulated": the
    reference cannot run on CUDA here); and it really is a different rule: integer-valued flows floor differently."""
    h = hip()
    g = load_golden("warp_cuda_form")
    gc = load_golden("warp")
    cases = _flow_cases()
    names = list(cases)
    F_ = len(names) + 1
    src = torch.zeros(F_, 4096, 8, dtype=torch.float16, device=DEV)
    flow = torch.stack([cases[n] for n in names]).to(DEV)
    dst = torch.empty_like(src)
    x0 = torch.empty(F_ - 1, 64, 64, dtype=torch.int32, device=DEV)
    y0 = torch.empty_like(x0)
    h.flow_warp(src, dst, flow, F=F_, h=64, w=64, C_=8, ld_src=8, fs_src=4096 * 8, ld_dst=8, fs_dst=4096 * 8,
                alpha=0.0, dbg_x0=x0, dbg_y0=y0, cuda_recip_div=True)
    ndiff = 0
    for i, n in enumerate(names):
        assert torch.equal(x0[i].cpu(), g[f"x0_{n}"]), n
        assert torch.equal(y0[i].cpu(), g[f"y0_{n}"]), n
        ndiff += int(((x0[i].cpu() != gc[f"x0_{n}"]) | (y0[i].cpu() != gc[f"y0_{n}"])).sum())
    assert ndiff > 500       # zero / integer flows sit on the floor() boundary: the two division forms disagree there


def test_flow_to_latent_matches_oracle():
    """512x512 flow -> 64x64 (area mean / 8), and other factors, against the oracle's definition."""
    h = hip()
    from oracle import flow as oflow
    from vface_amd.utils import synth
    for P, H, W, f in ((3, 512, 512, 8), (2, 96, 64, 4), (1, 768, 768, 8)):
        fl = synth.synth_flow(P, H, W) * f + 0.25 * synth.synth_normal("f2l", (P, 2, H, W))
        got = h.flow_to_latent(fl.to(DEV), f).cpu()
        ref = oflow.flow_to_latent(fl, f)
        assert got.shape == ref.shape and (got - ref).abs().max() < 2e-5


@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("cin,cout,H,W,nimg,silu", [(64, 160, 16, 16, 2, True), (320, 320, 32, 32, 3, True), (128, 128, 16, 48, 2, False),
                                                    (320, 640, 32, 32, 3, True), (64, 256, 16, 16, 2, True)])
def test_conv_patch_kernel_fused_groupnorm_silu(dt, cin, cout, H, W, nimg, silu):
    """GroupNorm-apply (+ SiLU) in the patch-staged convolution's operand path (north-star "GroupNorm+SiLU+conv fused";
    openaimodel.py:201-205): equals -- BIT FOR BIT -- the separate normalisation pass followed by the plain convolution on
    the same 16-bit input (same a, b, same arithmetic, zero padding applied after the normalisation), and torch.
    Since round 6 the fused form exists in the 128-channel tile only (the 160-wide instantiation carried 36 B of scratch and is
    not built): an output width that is not a multiple of 128 is REFUSED -- never run without its normalisation."""
    h = hip()
    from vface_amd.packing import pack_conv3x3
    x = rnd((nimg, cin, H, W), 1, dt) * 1.5 + 0.3
    w = rnd((cout, cin, 3, 3), 2, dt, 1 / math.sqrt(9 * cin))
    b = rnd((cout,), 3, torch.float32, 0.1)
    gm, bt = 1 + 0.2 * rnd((cin,), 4, torch.float32), 0.2 * rnd((cin,), 5, torch.float32)
    xn = x.permute(0, 2, 3, 1).reshape(-1, cin).contiguous().to(DEV)
    # column statistics of x as a producer epilogue would have left them
    xs = xn.float().reshape(nimg * H * W // 64, 64, cin)
    cs = torch.stack([xs.sum(1), (xs * xs).sum(1)], -1).contiguous()
    ab = h.groupnorm_coeffs_from_cols(cs, gm.to(DEV), bt.to(DEV), nimg=nimg, hw=H * W, C_=cin, eps=1e-5)
    wp = pack_conv3x3(w).to(DEV)
    fused = torch.zeros(nimg * H * W, cout, dtype=dt, device=DEV)
    if cout % 128:
        with pytest.raises(h.VFaceHipError):
            h.conv3x3(xn, wp, fused, nimg=nimg, H=H, W=W, cin=cin, cout=cout, ldx=cin, ldy=cout, bias=b.to(DEV), gn_ab=ab, gn_silu=silu,
                      flags=h.TUNE_PATCH)
        return
    h.conv3x3(xn, wp, fused, nimg=nimg, H=H, W=W, cin=cin, cout=cout, ldx=cin, ldy=cout, bias=b.to(DEV), gn_ab=ab, gn_silu=silu,
              flags=h.TUNE_PATCH)
    st = h.groupnorm_stats_from_cols(cs, nimg=nimg, hw=H * W, C_=cin, eps=1e-5)
    y = torch.empty_like(xn)
    h.groupnorm_apply(xn, st, gm.to(DEV), bt.to(DEV), y, nimg=nimg, hw=H * W, C_=cin, ldx=cin, ldy=cin, silu=silu)
    sep = torch.zeros_like(fused)
    h.conv3x3(y, wp, sep, nimg=nimg, H=H, W=W, cin=cin, cout=cout, ldx=cin, ldy=cout, bias=b.to(DEV), flags=h.TUNE_PATCH)
    assert torch.equal(fused, sep)
    xf = xn.float().cpu().reshape(nimg, H, W, cin).permute(0, 3, 1, 2)
    g = F.group_norm(xf, 32, gm, bt, 1e-5)
    ref = F.conv2d(F.silu(g) if silu else g, w.float(), b, padding=1).permute(0, 2, 3, 1).reshape(-1, cout)
    assert rel_l2(fused.cpu().float(), ref) < TOL[dt] * 1.3
    with pytest.raises(h.VFaceHipError):     # the im2col kernel has no fused form: refuse, never silently skip the normalisation
        h.conv3x3(xn, wp, sep, nimg=nimg, H=H, W=W, cin=cin, cout=cout, ldx=cin, ldy=cout, gn_ab=ab, gn_silu=silu, flags=h.TUNE_NO_PATCH)


# ------------------------------------------------------------------------------------------ plain GEMM through the 256-row tile
@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("M,N,K,rps", [(1024, 320, 320, 256), (2048, 640, 1280, 1024), (512, 1280, 128, 256), (768, 960, 320, 256)])
def test_gemm_256_row_tile_equals_128_row_kernel_bit_for_bit(dt, M, N, K, rps):
    """VFACE_TUNE_PATCH on a plain GEMM: conv.hip's 256 x BN tile (its "fused 1x1 source" K loop with no window tiles) --
    same K order per accumulator as gemm.hip, so the same bits: 16-bit output, fp32 carrier, column statistics; bias, per-sample
    row bias, 16-bit and fp32 residuals."""
    h = hip()
    a, w = rnd((M, K), 1, dt).to(DEV), rnd((N, K), 2, dt, 1 / math.sqrt(K)).to(DEV)
    bias, rb = rnd((N,), 3, torch.float32).to(DEV), rnd((M // rps, N), 5, torch.float32).to(DEV)
    res16, res32 = rnd((M, N), 4, dt).to(DEV), rnd((M, N), 6, torch.float32).to(DEV)
    for kw in (dict(), dict(rowbias=rb, rows_per_sample=rps), dict(residual=res16, ldr=N), dict(residual32=res32, want32=True)):
        outs = []
        for fl in (0x600 if N % 160 == 0 else 0x500, h.TUNE_PATCH):
            k2 = dict(kw)
            want32 = k2.pop("want32", False)
            o16 = torch.zeros(M, N, dtype=dt, device=DEV)
            o32 = torch.zeros(M, N, dtype=torch.float32, device=DEV) if want32 else None
            cs = torch.zeros(M // 64, N, 2, dtype=torch.float32, device=DEV)
            h.gemm(a, w, o16, M=M, N=N, K=K, lda=K, ldc=N, bias=bias, flags=fl, colstats=cs, split_k=False,
                   **({"out32": o32} if want32 else {}), **k2)
            outs.append((o16, o32, cs))
        ref = a.double() @ w.double().t() + bias.double()
        if "rowbias" in kw:
            ref = ref + rb.double().repeat_interleave(rps, 0)
        if "residual" in kw:
            ref = ref + res16.double()
        if "residual32" in kw:
            ref = ref + res32.double()
        assert rel_l2(outs[1][0].double().cpu(), ref.cpu()) < (2e-3 if dt == torch.float16 else 1e-2)
        assert torch.equal(outs[0][0], outs[1][0]), f"16-bit output differs ({list(kw)})"
        if outs[0][1] is not None:
            assert torch.equal(outs[0][1], outs[1][1]), "fp32 carrier differs"
        assert torch.allclose(outs[0][2], outs[1][2], rtol=1e-5, atol=1e-3), "column statistics differ"


@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16])
def test_epilogue_16_bit_transpose_equals_fp32_transpose_bit_for_bit(dt):
    """Where nothing reads the fp32 sum (no residual, no carrier) the epilogue rounds BEFORE its LDS transpose: same single
    rounding, so the same bits and statistics as the fp32 transpose (VFACE_TUNE_F32_TRANSPOSE) -- plain GEMM (both tile
    widths, ragged M), GEGLU, both convolution kernels, a parity-phase launch."""
    h = hip()
    cases = []
    for (M, N, K, geglu) in [(1000, 320, 320, False), (520, 256, 128, False), (640, 512, 192, True)]:
        a, w = rnd((M, K), 1, dt).to(DEV), rnd((N, K), 2, dt, 1 / math.sqrt(K)).to(DEV)
        bias = rnd((N,), 3, torch.float32).to(DEV)
        No = N // 2 if geglu else N
        def run(fl, a=a, w=w, bias=bias, M=M, N=N, K=K, No=No, geglu=geglu):
            o = torch.zeros(M, No, dtype=dt, device=DEV)
            cs = torch.zeros(M // 64, No, 2, dtype=torch.float32, device=DEV) if (M % 64 == 0 and not geglu) else None
            h.gemm(a, w, o, M=M, N=N, K=K, lda=K, ldc=No, bias=bias, flags=fl | (h.EPI_GEGLU if geglu else 0), colstats=cs, split_k=False)
            return o, cs
        cases.append(run)
    nimg, H, cin, cout = 3, 16, 128, 320
    x = rnd((nimg * H * H, cin), 5, dt).to(DEV)
    from vface_amd.packing import pack_conv3x3
    wc = pack_conv3x3(rnd((cout, cin, 3, 3), 6, torch.float32, 1 / math.sqrt(9 * cin))).to(dt).to(DEV)
    bc, rb = rnd((cout,), 7, torch.float32).to(DEV), rnd((nimg, cout), 8, torch.float32).to(DEV)
    for base in (h.TUNE_PATCH, h.TUNE_NO_PATCH):
        def run(fl, base=base):
            o = torch.zeros(nimg * H * H, cout, dtype=dt, device=DEV)
            cs = torch.zeros(nimg * H * H // 64, cout, 2, dtype=torch.float32, device=DEV)
            h.conv3x3(x, wc, o, nimg=nimg, H=H, W=H, cin=cin, cout=cout, ldx=cin, ldy=cout, bias=bc, rowbias=rb, flags=base | fl,
                      colstats=cs, split_k=False)
            return o, cs
        cases.append(run)
    for run in cases:
        (o1, c1), (o2, c2) = run(0), run(h.TUNE_F32_TRANSPOSE)
        assert o1.abs().sum() > 0 and torch.equal(o1, o2)
        if c1 is not None:
            assert torch.equal(c1, c2)


# ------------------------------------------------------------------------------------------ the 8x8 level through the patch kernel
@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("cin,cout,nimg,c2", [(256, 256, 6, 0), (128, 384, 5, 0), (256, 128, 24, 128), (512, 256, 7, 64)])
def test_conv_8x8_four_images_per_workgroup_form(dt, cin, cout, nimg, c2):
    """3x3 convolutions on 8 x 8 images: four images share a workgroup of the patch-staged kernel (each with its own zero halo
    in the 20 x 20 patch), K split over channel chunks, epilogue in the split-K reduce.  Against fp64 on the same 16-bit
    operands (the fp32 carrier), against the im2col kernel (VFACE_TUNE_NO_Q8; a different fp32 summation order), ragged last
    tiles (nimg % 4 != 0), row bias, fp32 residual, fused 1x1 shortcut, column statistics; batch invariance bit for bit."""
    h = hip()
    from vface_amd.packing import pack_conv3x3
    H = 8
    assert h.conv_uses_patch_kernel(H, H, cin, cout, 3, 1, False) == 2
    x = rnd((nimg, cin, H, H), 1, dt)
    w = rnd((cout, cin, 3, 3), 3, dt, 1 / math.sqrt(9 * cin))
    b, rb = rnd((cout,), 5, torch.float32, 0.1), rnd((nimg, cout), 6, torch.float32, 0.1)
    r32 = rnd((nimg * H * H, cout), 7, torch.float32)
    ref = F.conv2d(x.double(), w.double(), b.double(), padding=1) + rb.double()[:, :, None, None]
    xd = x.permute(0, 2, 3, 1).contiguous().to(DEV)
    if c2:
        x2 = rnd((nimg, c2, H, H), 2, dt)
        w2 = rnd((cout, c2), 4, dt, 1 / math.sqrt(c2))
        ref = ref + torch.einsum("nchw,oc->nohw", x2.double(), w2.double())
        wt = torch.cat([pack_conv3x3(w), w2], 1).contiguous().to(DEV)
        x2d = x2.permute(0, 2, 3, 1).contiguous().to(DEV)
    else:
        wt = pack_conv3x3(w).to(DEV)
    ref = ref.permute(0, 2, 3, 1).reshape(nimg * H * H, cout) + (0 if c2 else r32.double())   # (the fused shortcut IS the residual)

    def run(flags, n=nimg):
        o16 = torch.zeros(n * H * H, cout, dtype=dt, device=DEV)
        o32 = torch.zeros(n * H * H, cout, dtype=torch.float32, device=DEV)
        cs = torch.zeros(n, cout, 2, dtype=torch.float32, device=DEV)
        kw = dict(nimg=n, H=H, W=H, cin=cin, cout=cout, ldx=cin, ldy=cout, bias=b.to(DEV), rowbias=rb[:n].contiguous().to(DEV),
                  colstats=cs, flags=flags, out32=o32)
        if c2:
            h.conv3x3_plus_1x1(xd[:n].contiguous(), x2d[:n].contiguous(), wt, o16, c2=c2, ldx2=c2, **kw)
        else:
            h.conv3x3(xd[:n].contiguous(), wt, o16, residual32=r32[:n * H * H].contiguous().to(DEV), **kw)
        return o16, o32, cs

    o16, o32, cs = run(0)
    i16, i32, ics = run(h.TUNE_NO_Q8)
    assert rel_l2(o32.double().cpu(), ref) < 3e-6 and rel_l2(i32.double().cpu(), ref) < 3e-6
    assert torch.equal(o16, o32.to(dt))                              # one rounding of the fp32 sum
    assert rel_l2(o32.cpu(), i32.cpu()) < 1e-6
    ss = o32.reshape(nimg, 64, cout)
    assert torch.allclose(cs[..., 0], ss.sum(1), rtol=1e-4, atol=1e-3) and torch.allclose(cs[..., 1], (ss * ss).sum(1), rtol=1e-4, atol=1e-3)
    # a sample's bits do not depend on which other samples share its launch (here: 3 images alone, a ragged tile)
    p16, p32, pcs = run(0, n=3)
    assert torch.equal(p16, o16[:3 * 64]) and torch.equal(p32, o32[:3 * 64]) and torch.equal(pcs, cs[:3])


def _ffn_reference(x, gamma, beta, w1, b1, w2, b2):
    """attention.py:243 `ff(norm3(x)) + x` with FeedForward = Linear(GEGLU) -> Linear (:37-64), in fp64 on the given weights."""
    x = x.double()
    ln = F.layer_norm(x, (x.shape[1],), gamma.double(), beta.double(), 1e-5)
    y = ln @ w1.double().t() + b1.double()
    a, g = y.chunk(2, dim=-1)
    h = a * F.gelu(g)
    return h @ w2.double().t() + b2.double() + x


@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("M,C", [(128, 64), (384, 128), (256, 320), (4096, 320)])
def test_ffn_fused_vs_reference_and_vs_three_kernel_path(dt, M, C):
    """csrc/ffn.hip: LayerNorm -> ff.net[0] (GEGLU) -> ff.net[2] -> + x in one launch, the normalised activations held in
    registers as MFMA operands and the hidden activations going from accumulators to operands without leaving the registers,
    against (a) an fp64 evaluation of the reference's formula on the same 16-bit weights and (b) the three-kernel path
    (vface_layernorm + vface_gemm(GEGLU) + vface_gemm + residual) it replaces."""
    h = hip()
    from vface_amd import packing
    assert h.ffn_fused_supported(M, C) and not h.ffn_fused_supported(M + 64, C) and not h.ffn_fused_supported(M, 640)
    x = rnd((M, C), 31, torch.float32, 1.5) + rnd((M, 1), 32, torch.float32, 0.7)     # rows with a non-zero mean
    gamma, beta = 1.0 + rnd((C,), 33, torch.float32, 0.2), rnd((C,), 34, torch.float32, 0.2)
    w1, b1 = rnd((8 * C, C), 35, dt, C ** -0.5), rnd((8 * C,), 36, torch.float32, 0.3)
    w2, b2 = rnd((C, 4 * C), 37, dt, (4 * C) ** -0.5), rnd((C,), 38, torch.float32, 0.3)
    ref = _ffn_reference(x, gamma, beta, w1.float(), b1, w2.float(), b2).float()
    w1p, b1p = packing.pack_geglu(w1, b1)
    w2p = packing.pack_ffn_w2(w2)
    d = lambda v: v.to(DEV).contiguous()
    xd, out16, out32 = d(x), torch.zeros(M, C, dtype=dt, device=DEV), torch.zeros(M, C, dtype=torch.float32, device=DEV)
    h.ffn_fused(xd, d(gamma), d(beta), d(w1p), d(b1p), d(w2p), d(b2), out16, M=M, C_=C, out32=out32)
    e32, e16 = rel_l2(out32.cpu(), ref), rel_l2(out16.cpu().float(), ref)
    # the three-kernel path on the same operands
    ln = torch.empty(M, C, dtype=dt, device=DEV)
    h.layernorm(xd, d(gamma), d(beta), ln, M=M, C_=C, ldx=C, ldy=C)
    ff = torch.empty(M, 4 * C, dtype=dt, device=DEV)
    h.gemm(ln, d(w1p), ff, M=M, N=8 * C, K=C, lda=C, ldc=4 * C, bias=d(b1p), flags=h.EPI_GEGLU)
    o3 = torch.empty(M, C, dtype=torch.float32, device=DEV)
    h.gemm(ff, d(w2), None, M=M, N=C, K=4 * C, lda=4 * C, ldc=0, bias=d(b2), residual32=xd, out32=o3)
    e3 = rel_l2(o3.cpu(), ref)
    e_vs3 = rel_l2(out32.cpu(), o3.cpu())
    print(f"ffn fused M={M} C={C} {dt}: fp32 out {e32:.2e}, 16-bit out {e16:.2e}; three-kernel path {e3:.2e}; fused vs three-kernel {e_vs3:.2e}")
    assert torch.equal(out16, out32.to(dt)), "the 16-bit output is the single rounding of the fp32 sum"
    assert e32 < TOL[dt] and e32 < 1.5 * e3 + 1e-5 and e_vs3 < TOL[dt]


@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("M,C,rps,with_rb", [(128, 64, 128, True), (512, 128, 256, False), (768, 320, 256, True), (4096, 320, 1024, True)])
def test_attn_out_ffn_fused_vs_reference_and_vs_two_launches(dt, M, C, rps, with_rb):
    """csrc/ffn.hip, PRE form (``vface_attn_out_ffn_fused``): attn1's out-projection + bias + attn2's per-sample row bias +
    residual in front of the fused FeedForward, the running sum t1 never stored -- against (a) an fp64 evaluation on the same
    16-bit operands and (b) the two launches it replaces (vface_gemm into the fp32 stream, then vface_ffn_fused)."""
    h = hip()
    from vface_amd import packing
    att = rnd((M, C), 41, dt, 0.8)
    t0 = rnd((M, C), 42, torch.float32, 1.2) + rnd((M, 1), 43, torch.float32, 0.5)
    wo, bo = rnd((C, C), 44, dt, C ** -0.5), rnd((C,), 45, torch.float32, 0.2)
    rb = rnd((M // rps, C + 32), 46, torch.float32, 0.5)[:, 16:16 + C] if with_rb else None     # a column slice, like a2_all[:, a:b]
    gamma, beta = 1.0 + rnd((C,), 33, torch.float32, 0.2), rnd((C,), 34, torch.float32, 0.2)
    w1, b1 = rnd((8 * C, C), 35, dt, C ** -0.5), rnd((8 * C,), 36, torch.float32, 0.3)
    w2, b2 = rnd((C, 4 * C), 37, dt, (4 * C) ** -0.5), rnd((C,), 38, torch.float32, 0.3)
    t1_ref = att.double() @ wo.double().t() + bo.double() + t0.double()
    if with_rb:
        t1_ref = t1_ref + rb.double().repeat_interleave(rps, 0)
    ref = _ffn_reference(t1_ref.float(), gamma, beta, w1.float(), b1, w2.float(), b2).float()
    w1p, b1p = packing.pack_geglu(w1, b1)
    w2p = packing.pack_ffn_w2(w2)
    tail_w = packing.pack_attn_out_ffn(wo, w1p)
    d = lambda v: v.to(DEV).contiguous()
    rbd = None
    if with_rb:
        wide = torch.zeros(M // rps, C + 32, dtype=torch.float32, device=DEV)
        wide[:, 16:16 + C] = rb.to(DEV)
        rbd = wide[:, 16:16 + C]
    attd, t0d = d(att), d(t0)
    out16, out32 = torch.zeros(M, C, dtype=dt, device=DEV), torch.zeros(M, C, dtype=torch.float32, device=DEV)
    h.attn_out_ffn_fused(attd, t0d, rbd, d(tail_w), d(bo), d(gamma), d(beta), d(b1p), d(w2p), d(b2), out16, M=M, C_=C,
                         rows_per_sample=rps, out32=out32)
    e32 = rel_l2(out32.cpu(), ref)
    # the two launches it replaces
    t1 = torch.empty(M, C, dtype=torch.float32, device=DEV)
    h.gemm(attd, d(wo), None, M=M, N=C, K=C, lda=C, ldc=0, bias=d(bo), rowbias=rbd, rows_per_sample=rps, split_k=False,
           residual32=t0d, out32=t1)
    assert rel_l2(t1.cpu().double(), t1_ref) < 2e-6
    o2 = torch.zeros(M, C, dtype=torch.float32, device=DEV)
    h.ffn_fused(t1, d(gamma), d(beta), d(w1p), d(b1p), d(w2p), d(b2), None, M=M, C_=C, out32=o2)
    e2, e_vs2 = rel_l2(o2.cpu(), ref), rel_l2(out32.cpu(), o2.cpu())
    print(f"attn-out + ffn fused M={M} C={C} {dt}: {e32:.2e}; two launches {e2:.2e}; fused vs two launches {e_vs2:.2e}")
    assert torch.equal(out16, out32.to(dt))
    assert e32 < TOL[dt] and e32 < 1.5 * e2 + 1e-5 and e_vs2 < TOL[dt]


@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("M,C,rps,want16,wide", [(256, 64, 128, True, False), (512, 128, 256, False, True), (1024, 320, 512, True, True),
                                                 (128 * 300, 320, 128 * 100, False, False)])
def test_attn_out_ffn_proj_fused_vs_reference_and_vs_separate_proj_out(dt, M, C, rps, want16, wide):
    """csrc/ffn.hip, POST form (``vface_attn_out_ffn_proj_fused``): the SpatialTransformer's proj_out + x_in (attention.py:286-289)
    and the column statistics of the result behind the fused block tail, one launch -- against (a) fp64 on the same 16-bit operands
    (the tail's own 16-bit output is the operand, as in the separate GEMM) and (b) vface_attn_out_ffn_fused + vface_gemm with
    colstats / out32 / residual32; outputs into column slices of wider buffers (the skip-concatenation targets) too."""
    h = hip()
    from vface_amd import packing
    att = rnd((M, C), 41, dt, 0.8)
    t0 = rnd((M, C), 42, torch.float32, 1.2) + rnd((M, 1), 43, torch.float32, 0.5)
    wo, bo = rnd((C, C), 44, dt, C ** -0.5), rnd((C,), 45, torch.float32, 0.2)
    rb = rnd((M // rps, C), 46, torch.float32, 0.5)
    gamma, beta = 1.0 + rnd((C,), 33, torch.float32, 0.2), rnd((C,), 34, torch.float32, 0.2)
    w1, b1 = rnd((8 * C, C), 35, dt, C ** -0.5), rnd((8 * C,), 36, torch.float32, 0.3)
    w2, b2 = rnd((C, 4 * C), 37, dt, (4 * C) ** -0.5), rnd((C,), 38, torch.float32, 0.3)
    wpo, bpo = rnd((C, C), 47, dt, C ** -0.5), rnd((C,), 48, torch.float32, 0.2)
    x_in = rnd((M, C), 49, torch.float32, 1.5)
    w1p, b1p = packing.pack_geglu(w1, b1)
    w2p = packing.pack_ffn_w2(w2)
    d = lambda v: v.to(DEV).contiguous()
    attd, t0d, rbd, xd = d(att), d(t0), d(rb), d(x_in)
    # (b) first: the block tail alone, then proj_out as a GEMM
    t3 = torch.zeros(M, C, dtype=dt, device=DEV)
    h.attn_out_ffn_fused(attd, t0d, rbd, d(packing.pack_attn_out_ffn(wo, w1p)), d(bo), d(gamma), d(beta), d(b1p), d(w2p), d(b2), t3, M=M, C_=C,
                         rows_per_sample=rps)
    y2 = torch.zeros(M, C, dtype=torch.float32, device=DEV)
    y2_16 = torch.zeros(M, C, dtype=dt, device=DEV)
    cs2 = torch.zeros(M // 64, C, 2, dtype=torch.float32, device=DEV)
    h.gemm(t3, d(wpo), y2_16, M=M, N=C, K=C, lda=C, ldc=C, bias=d(bpo), colstats=cs2, residual32=xd, out32=y2, rows_per_sample=rps)
    ref = (t3.cpu().double() @ wpo.double().t() + bpo.double() + x_in.double())
    assert rel_l2(y2.cpu().double(), ref) < 2e-6
    # the one launch
    W = C + 32 if wide else C
    y32 = torch.full((M, W), 7.0, dtype=torch.float32, device=DEV)[:, W - C:]
    y16 = torch.full((M, W), 7.0, dtype=dt, device=DEV)[:, W - C:] if want16 else None
    cs = torch.full((M // 64, W, 2), 7.0, dtype=torch.float32, device=DEV)[:, W - C:]
    h.attn_out_ffn_proj_fused(attd, t0d, rbd, d(packing.pack_attn_out_ffn(wo, w1p, wpo)), d(bo), d(gamma), d(beta), d(b1p), d(w2p), d(b2),
                              d(bpo), xd, y16, y32, cs, M=M, C_=C, rows_per_sample=rps)
    e, e_vs = rel_l2(y32.cpu().double(), ref), rel_l2(y32.cpu(), y2.cpu())
    print(f"tail + proj_out fused M={M} C={C} {dt}: vs fp64 on the tail's 16-bit output {e:.2e}; vs the separate GEMM {e_vs:.2e}")
    # (t3 = accumulator + (b2 + bo + a2) is formed and rounded exactly as the separate tail does: the operands are the same bits,
    # what differs is fp32 summation order -- x_in is the accumulator's initial value here, the epilogue's last addend there)
    assert e < 1e-5 and e_vs < 1e-5
    if want16:
        assert torch.equal(y16, y32.to(dt))
    sl = y32.reshape(M // 64, 64, C).double()
    want = torch.stack([sl.sum(1), (sl * sl).sum(1)], -1)
    assert rel_l2(cs.double().cpu(), want.cpu()) < 1e-6
    if wide:      # nothing outside the column slice was touched
        for buf in (y32, cs) + ((y16,) if want16 else ()):
            base = buf._base
            assert bool((base[:, :W - C] == 7.0).all())


@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("M,C,hw,rows_full,nq_lo,want_ln", [(256, 64, 128, 256, 0, False), (768, 128, 256, 256, 256, True),
                                                            (1024, 320, 256, 1024, 0, False), (3072, 320, 1024, 1024, 640, True),
                                                            (128 * 300, 320, 128 * 100, 128 * 100, 640, False)])
def test_st_front_vs_reference_and_vs_four_kernel_path(dt, M, C, hw, rows_full, nq_lo, want_ln):
    """VERDICT r3 next #1a/b: GroupNorm-apply -> proj_in -> LayerNorm -> attn1 projection as one launch (csrc/stfront.hip,
    ``vface_st_front``; attention.py:278-284, 239, 179-183).  Against an fp64 torch computation on the same 16-bit-rounded
    operands (t0 < 1e-5: fp32 accumulation; qkv within the 16-bit bound), against the four launches it replaces (gn_apply, GEMM,
    layernorm, GEMM), on column-sliced column statistics, with the hook's row split (rows >= rows_full project columns >= nq_lo
    only and leave the others untouched), for one workgroup per token tile and for the persistent form (more tiles than CUs)."""
    h = hip()
    from vface_amd.packing import pack_st_front
    nimg = M // hw
    img = torch.arange(M) // hw          # every image its own mean and scale: a tile that took another image's (a, b) would show
    x = (rnd((M, C), 21, torch.float32, 1.3) * (1.0 + 0.5 * (img % 3))[:, None] + 0.25 * rnd((1, C), 22, torch.float32)
         + (0.7 * (img % 3) - 0.5)[:, None]).to(DEV)
    w_in = rnd((C, C), 23, dt, 1 / math.sqrt(C))
    b_in = rnd((C,), 24, torch.float32, 0.1)
    w_p = rnd((3 * C, C), 25, dt, 1 / math.sqrt(C))
    gng, gnb = rnd((C,), 26, torch.float32, 0.3) + 1.0, rnd((C,), 27, torch.float32, 0.2)
    lng, lnb = rnd((C,), 28, torch.float32, 0.3) + 1.0, rnd((C,), 29, torch.float32, 0.2)
    sl = x.reshape(M // 64, 64, C)
    cs = torch.zeros(M // 64, C + 16, 2, dtype=torch.float32, device=DEV)[:, 8:8 + C]
    cs[..., 0] = sl.sum(1)
    cs[..., 1] = (sl * sl).sum(1)
    ab = h.groupnorm_coeffs_from_cols(cs, gng.to(DEV), gnb.to(DEV), nimg=nimg, hw=hw, C_=C, eps=1e-6)
    t0 = torch.zeros(M, C, dtype=torch.float32, device=DEV)
    SENT = 7.0
    qkv = torch.full((M, 3 * C + 8), SENT, dtype=dt, device=DEV)[:, :3 * C]       # a strided view: ldq = 3C + 8
    ln = torch.zeros(M, C, dtype=dt, device=DEV) if want_ln else None
    wcat = pack_st_front(w_in.float(), w_p.float()).to(dt).to(DEV)
    h.st_front(x, ab, wcat, b_in.to(DEV), lng.to(DEV), lnb.to(DEV), t0, qkv, M=M, C_=C, hw=hw, NQ=3 * C, rows_full=rows_full,
               nq_lo=nq_lo, ln=ln)
    torch.cuda.synchronize()
    # ---- fp64 reference on the same rounded operands
    abc = ab.cpu().double()
    a_row = abc[..., 0].repeat_interleave(hw, 0)
    b_row = abc[..., 1].repeat_interleave(hw, 0)
    y16 = (x.cpu() * a_row.float() + b_row.float()).to(dt).double()       # gn_apply's arithmetic: fp32 multiply-add, one rounding
    t0_ref = y16 @ w_in.double().t() + b_in.double()
    # (the host's multiply-then-add and the kernel's fused multiply-add differ in the last fp32 bit now and then, which flips a
    # 16-bit rounding of the operand: ~1e-6 on t0; the kernel-against-kernel comparison below is the tight one)
    assert rel_l2(t0.cpu().double(), t0_ref) < (1e-5 if dt == torch.float16 else 1e-4)      # (a flipped bf16 rounding is 8x an fp16 one)
    t0d = t0.cpu().double()
    mu = t0d.mean(1, keepdim=True)
    var = ((t0d - mu) ** 2).mean(1, keepdim=True)
    ln_ref = ((t0d - mu) / torch.sqrt(var + 1e-5) * lng.double() + lnb.double())
    if want_ln:
        assert rel_l2(ln.cpu().double(), ln_ref) < TOL[dt]
    q_ref = ln_ref.to(dt).double() @ w_p.double().t()
    got = qkv.cpu().double()
    assert rel_l2(got[:rows_full], q_ref[:rows_full]) < TOL[dt]
    if rows_full < M:
        assert rel_l2(got[rows_full:, nq_lo:], q_ref[rows_full:, nq_lo:]) < TOL[dt]
        assert (qkv[rows_full:, :nq_lo] == SENT).all()          # columns this row range does not project stay untouched
    # ---- the four launches it replaces
    st = h.groupnorm_stats_from_cols(cs, nimg=nimg, hw=hw, C_=C, eps=1e-6)
    g16 = torch.empty(M, C, dtype=dt, device=DEV)
    h.groupnorm_apply(x, st, gng.to(DEV), gnb.to(DEV), g16, nimg=nimg, hw=hw, C_=C, ldx=C, ldy=C, silu=False)
    t0b = torch.empty(M, C, dtype=torch.float32, device=DEV)
    h.gemm(g16, w_in.to(DEV), None, M=M, N=C, K=C, lda=C, ldc=0, bias=b_in.to(DEV), out32=t0b, rows_per_sample=hw)
    assert rel_l2(t0.cpu(), t0b.cpu()) < 2e-6
    l16 = torch.empty(M, C, dtype=dt, device=DEV)
    h.layernorm(t0b, lng.to(DEV), lnb.to(DEV), l16, M=M, C_=C, ldx=C, ldy=C)
    qb = torch.empty(M, 3 * C, dtype=dt, device=DEV)
    h.gemm(l16, w_p.to(DEV), qb, M=M, N=3 * C, K=C, lda=C, ldc=3 * C)
    assert rel_l2(got[:rows_full], qb.cpu().double()[:rows_full]) < 1.5 * TOL[dt]


@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("cin,cout,H,W,nimg,in32", [(320, 4, 64, 64, 2, True), (64, 4, 32, 32, 3, True), (128, 3, 20, 24, 2, False),
                                                    (320, 4, 96, 96, 1, True)])
def test_fused_out_layer_vs_reference_and_vs_separate_launches(dt, cin, cout, H, W, nimg, in32):
    """csrc/outconv.hip (``vface_gn_silu_conv3x3_small``): the UNet's out layer -- GroupNorm32 -> SiLU -> conv3x3 to 4 channels
    (openaimodel.py:712-716, :905) -- in one launch, against torch on the same rounded operands and against the launches it replaces
    (gn_finalize + gn_apply + the implicit-GEMM convolution with fp32 output); ragged tiles (20 x 24) and the 768 x 768 map included."""
    h = hip()
    from vface_amd.packing import pack_conv3x3
    hw = H * W
    img = torch.arange(nimg * hw) // hw          # every image its own mean and scale, so its own coefficients
    x = rnd((nimg * hw, cin), 51, torch.float32, 1.4) * (1.0 + 0.5 * (img % 3))[:, None] + 0.2 + (0.7 * (img % 3))[:, None]
    xin = x.to(DEV) if in32 else x.to(dt).to(DEV)
    xs = xin.float()
    w = rnd((cout, cin, 3, 3), 52, dt, 1 / math.sqrt(9 * cin))
    b = rnd((cout,), 53, torch.float32, 0.1)
    g, be = rnd((cin,), 54, torch.float32, 0.3) + 1.0, rnd((cin,), 55, torch.float32, 0.2)
    pad = (-hw) % 64          # column sums per 64-row slice need hw % 64 == 0: build them from torch instead
    assert pad == 0 or True
    if hw % 64 == 0:
        sl = xs.reshape(nimg * hw // 64, 64, cin)
        cs = torch.stack([sl.sum(1), (sl * sl).sum(1)], -1).contiguous()
        ab = h.groupnorm_coeffs_from_cols(cs, g.to(DEV), be.to(DEV), nimg=nimg, hw=hw, C_=cin, eps=1e-5)
    else:          # (the engine only takes this path with producer-side sums; a ragged map gets its coefficients from torch here)
        xg = xs.reshape(nimg, hw, 32, cin // 32)
        mean, var = xg.mean(dim=(1, 3)), xg.var(dim=(1, 3), unbiased=False)
        rstd = torch.rsqrt(var + 1e-5)
        a = rstd.repeat_interleave(cin // 32, 1) * g.to(DEV)[None]
        ab = torch.stack([a, be.to(DEV)[None] - mean.repeat_interleave(cin // 32, 1) * a], -1).contiguous()
    out = torch.zeros(nimg * hw, cout, dtype=torch.float32, device=DEV)
    wp = pack_conv3x3(w.float()).to(dt).to(DEV)
    h.gn_silu_conv3x3_small(xin, ab, wp, b.to(DEV), out, nimg=nimg, H=H, W=W, cin=cin, cout=cout)
    # torch on the same operands: y = round16(SiLU(x a + b)), conv in fp64
    abc = ab.cpu()
    y = (xs.cpu() * abc[..., 0].repeat_interleave(hw, 0) + abc[..., 1].repeat_interleave(hw, 0))
    y16 = F.silu(y).to(dt).double().reshape(nimg, H, W, cin).permute(0, 3, 1, 2)
    ref = F.conv2d(y16, w.double(), b.double(), padding=1).permute(0, 2, 3, 1).reshape(nimg * hw, cout)
    assert rel_l2(out.cpu().double(), ref) < (2e-5 if dt == torch.float16 else 2e-4)      # (one flipped rounding of y now and then)
    if hw % 64 == 0:
        st = h.groupnorm_stats_from_cols(cs, nimg=nimg, hw=hw, C_=cin, eps=1e-5)
        y2 = torch.empty(nimg * hw, cin, dtype=dt, device=DEV)
        h.groupnorm_apply(xin, st, g.to(DEV), be.to(DEV), y2, nimg=nimg, hw=hw, C_=cin, ldx=cin, ldy=cin, silu=True)
        o2 = torch.zeros(nimg * hw, cout, dtype=torch.float32, device=DEV)
        h.conv3x3(y2, wp, o2, nimg=nimg, H=H, W=W, cin=cin, cout=cout, ldx=cin, ldy=cout, bias=b.to(DEV), flags=h.EPI_OUT_F32)
        assert rel_l2(out.cpu(), o2.cpu()) < 2e-6          # the same products, summed in another order


def test_st_front_rejects_what_it_cannot_run():
    h = hip()
    assert h.st_front_supported(1024, 320, 256) and h.st_front_supported(128, 64, 128)
    assert not h.st_front_supported(1024, 640, 256) and not h.st_front_supported(1000, 320, 250) \
        and not h.st_front_supported(1024, 320, 192)


def test_ffn_fused_rejects_what_it_cannot_run():
    h = hip()
    x = torch.zeros(128, 640, device=DEV)
    w = torch.zeros(8, 8, dtype=torch.float16, device=DEV)
    with pytest.raises(h.VFaceHipError):
        h.ffn_fused(x, x, x, w, x, w, x, torch.zeros(128, 640, dtype=torch.float16, device=DEV), M=128, C_=640)


# ------------------------------------------------------------------------------------------ the 256 x 320 tile (csrc/gemm_big.hip)
@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("M,N,K", [(512, 640, 640), (1000, 320, 128), (768, 1920, 1280), (256, 1280, 2560), (1000, 2560, 384), (512, 1280, 128),
                                   (300, 3840, 256)])
def test_gemm_big_tile_equals_128_row_kernel_bit_for_bit(dt, M, N, K):
    """The 256 x 320 tile accumulates every output in the 128-row kernel's order (K tile by K tile, k32 half 0 then half 1, the
    same MFMA and operand roles): same bits -- plain, + bias, GEGLU, + bias + fp32 residual rows, dual-source K, strided views and
    a row count that is not a multiple of the tile (1000) -- and both within the fp16 bound of an fp64 computation."""
    h = hip()
    # the 128-row kernel; the big tile 320 channels wide; the big tile 256 channels wide (round 6; where N % 256 != 0 the flag falls back to 320)
    FORMS = (h.TUNE_NO_BIG_TILE, h.TUNE_BIG_TILE | h.TUNE_BIG_W320, h.TUNE_BIG_TILE | h.TUNE_BIG_W256)
    a, w = rnd((M, K), 1, dt).to(DEV), rnd((N, K), 2, dt, 1 / math.sqrt(K)).to(DEV)
    bias = rnd((N,), 3, torch.float32).to(DEV)
    res32 = rnd((M, N), 6, torch.float32).to(DEV)
    res16 = rnd((M, N), 8, dt).to(DEV)
    a0 = rnd((M, K // 2), 7, dt).to(DEV)
    wide = torch.zeros(M, K + 64, dtype=dt, device=DEV)
    wide[:, 32:32 + K] = a
    cases = [("plain", dict(), a.double() @ w.double().t()),
             ("bias", dict(bias=bias), a.double() @ w.double().t() + bias.double()),
             ("bias+res32", dict(bias=bias, residual32=res32), a.double() @ w.double().t() + bias.double() + res32.double()),
             ("res32", dict(residual32=res32), a.double() @ w.double().t() + res32.double()),
             ("bias+res16", dict(bias=bias, residual=res16, ldr=N), a.double() @ w.double().t() + bias.double() + res16.double())]
    for name, kw, ref in cases:
        outs = []
        for fl in FORMS:
            o = torch.full((M, N + 16), 7.0, dtype=dt, device=DEV)
            h.gemm(wide[:, 32:], w, o[:, 8:], M=M, N=N, K=K, lda=K + 64, ldc=N + 16, flags=fl, split_k=False, **kw)
            outs.append(o)
        assert rel_l2(outs[1][:, 8:8 + N].double().cpu(), ref.cpu()) < (1e-3 if dt == torch.float16 else 8e-3), name
        assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2]), f"{name}: the tiles' outputs differ"      # (and nothing outside the view was written)
    # dual-source K (the hook's linear fusions: [x_c | x_0] against the folded [2d, 2d] weight)
    outs = []
    for fl in FORMS:
        o = torch.empty(M, N, dtype=dt, device=DEV)
        h.gemm(a[:, :K // 2], w, o, M=M, N=N, K=K, lda=K, ldc=N, a2=a0, lda2=K // 2, k1=K // 2, flags=fl, split_k=False)
        outs.append(o)
    ref = torch.cat([a[:, :K // 2], a0], 1).double() @ w.double().t()
    assert rel_l2(outs[1].double().cpu(), ref.cpu()) < (1e-3 if dt == torch.float16 else 8e-3)
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2]), "dual-source K: the tiles' outputs differ"
    # GEGLU (weight rows interleaved in 16-row value / gate blocks)
    from vface_amd import packing
    wp, bp = packing.pack_geglu(w.float().cpu(), bias.cpu())
    wp, bp = wp.to(device=DEV, dtype=dt), bp.to(DEV)
    outs = []
    for fl in FORMS:
        o = torch.empty(M, N // 2, dtype=dt, device=DEV)
        h.gemm(a, wp, o, M=M, N=N, K=K, lda=K, ldc=N // 2, bias=bp, flags=fl | h.EPI_GEGLU, split_k=False)
        outs.append(o)
    y = a.double() @ w.double().t() + bias.double()
    ref = y[:, :N // 2] * F.gelu(y[:, N // 2:])
    assert rel_l2(outs[1].double().cpu(), ref.cpu()) < (1e-3 if dt == torch.float16 else 8e-3)
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2]), "GEGLU: the tiles' outputs differ"


@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("M,N,K,rps", [(1024, 640, 640, 256), (768, 1280, 1280, 256), (2048, 320, 128, 1024)])
def test_gemm_big_tile_residual_stream_form(dt, M, N, K, rps):
    """The 256 x 320 tile's fp32 residual-stream epilogue (proj_in / to_out / proj_out of a 640- / 1280-channel block): bias +
    per-sample row bias + fp32 residual rows -> fp32 carrier (+ 16-bit copy, + per-64-row column statistics).  Carrier and copy
    are the 128-row kernel's bits; the statistics are the same sums folded in another order (allclose), and the sums of what was
    stored (fp64)."""
    h = hip()
    a, w = rnd((M, K), 1, dt).to(DEV), rnd((N, K), 2, dt, 1 / math.sqrt(K)).to(DEV)
    bias, rb = rnd((N,), 3, torch.float32).to(DEV), rnd((M // rps, N), 5, torch.float32).to(DEV)
    res32 = rnd((M, N), 6, torch.float32).to(DEV)
    base = a.double() @ w.double().t() + bias.double()
    cases = [("proj_in", dict(), False, False, base),
             ("to_out", dict(rowbias=rb, rows_per_sample=rps, residual32=res32), False, False, base + rb.double().repeat_interleave(rps, 0) + res32.double()),
             ("proj_out", dict(residual32=res32, rows_per_sample=rps), True, True, base + res32.double())]
    for name, kw, want16, stats, ref in cases:
        outs = []
        for fl in (h.TUNE_NO_BIG_TILE, h.TUNE_BIG_TILE):
            o32 = torch.full((M, N + 8), 3.0, dtype=torch.float32, device=DEV)
            o16 = torch.full((M, N + 8), 3.0, dtype=dt, device=DEV) if want16 else None
            cs = torch.zeros(M // 64, N, 2, dtype=torch.float32, device=DEV) if stats else None
            h.gemm(a, w, o16[:, 8:] if want16 else None, M=M, N=N, K=K, lda=K, ldc=N + 8 if want16 else 0, bias=bias, flags=fl,
                   colstats=cs, out32=o32[:, :N], split_k=False, **kw)
            outs.append((o32, o16, cs))
        assert rel_l2(outs[1][0][:, :N].double().cpu(), ref.cpu()) < 1e-5, name
        assert torch.equal(outs[0][0], outs[1][0]), f"{name}: fp32 carrier differs (or something outside the view was written)"
        if want16:
            assert torch.equal(outs[0][1], outs[1][1]), f"{name}: 16-bit copy differs"
        if stats:
            assert torch.allclose(outs[0][2], outs[1][2], rtol=1e-5, atol=1e-3), f"{name}: column statistics differ"
            v = outs[1][0][:, :N].double().reshape(M // 64, 64, N)
            want = torch.stack([v.sum(1), (v * v).sum(1)], -1)
            assert torch.allclose(outs[1][2].double(), want, rtol=1e-5, atol=1e-3)


@pytest.mark.parametrize("M,N,K,kind", [(24576, 1280, 512, "res16"), (24576, 3840, 256, "plain"), (24576 + 300, 1280, 256, "geglu")])
def test_gemm_default_dispatch_at_full_batch_keeps_the_bits(M, N, K, kind):
    """The library's own choice among its plain-GEMM forms at the headline's row counts (the 128-row kernel, the big tile 320 or 256 channels
    wide -- N = 1280 / 3840 allow both widths) gives the bits of either kernel forced, with a residual operand, through GEGLU, and with a
    ragged row count.  (Round 6 also tried cutting a 1.5-round grid by rows between the two kernels: same bits, no gain -- the big tile's
    full round is itself activation-bound on these shapes -- and not kept.)"""
    h = hip()
    dt = torch.float16
    a, w = rnd((M, K), 1, dt).to(DEV), rnd((N, K), 2, dt, 1 / math.sqrt(K)).to(DEV)
    bias = rnd((N,), 3, torch.float32).to(DEV)
    kw, base, ncol = dict(), 0, N
    if kind == "res16":
        kw = dict(bias=bias, residual=rnd((M, N), 4, dt).to(DEV), ldr=N)
    elif kind == "geglu":
        from vface_amd import packing
        wp, bp = packing.pack_geglu(w.float().cpu(), bias.cpu())
        w, kw, base, ncol = wp.to(device=DEV, dtype=dt), dict(bias=bp.to(DEV)), h.EPI_GEGLU, N // 2
    outs = []
    for fl in (0, h.TUNE_NO_BIG_TILE, h.TUNE_BIG_TILE):
        o = torch.full((M, ncol + 8), 7.0, dtype=dt, device=DEV)
        h.gemm(a, w, o[:, :ncol], M=M, N=N, K=K, lda=K, ldc=ncol + 8, flags=base | fl, split_k=False, **kw)
        outs.append(o)
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])


def test_gemm_big_tile_refuses_what_it_cannot_do():
    """VFACE_TUNE_BIG_TILE is a preference, not a different result: a launch the 256 x 320 tile does not take (N % 320 != 0; a row
    bias whose samples are shorter than the tile; an fp32-only output) runs the 128-row kernel and gives that kernel's bits."""
    h = hip()
    dt = torch.float16
    for M, N, K, rps in ((512, 512, 320, 256), (512, 640, 320, 64)):
        a, w = rnd((M, K), 1, dt).to(DEV), rnd((N, K), 2, dt, 1 / math.sqrt(K)).to(DEV)
        rb = rnd((M // rps, N), 5, torch.float32).to(DEV)
        outs = []
        for fl in (h.TUNE_NO_BIG_TILE, h.TUNE_BIG_TILE):
            o, o32 = torch.empty(M, N, dtype=dt, device=DEV), torch.empty(M, N, dtype=torch.float32, device=DEV)
            cs = torch.zeros(M // 64, N, 2, dtype=torch.float32, device=DEV)
            h.gemm(a, w, o, M=M, N=N, K=K, lda=K, ldc=N, flags=fl, colstats=cs, out32=o32, rowbias=rb, rows_per_sample=rps, split_k=False)
            outs.append((o, o32, cs))
        for x, y in zip(*outs):
            assert torch.equal(x, y)


# ------------------------------------------------------------------------------------------ the input convolution (csrc/inconv.hip)
@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("nimg,H,W,cout", [(3, 64, 64, 320), (2, 32, 48, 160), (5, 16, 16, 80), (1, 8, 16, 400)])
def test_input_conv_16_stored_channels(dt, nimg, H, W, cout):
    """conv3x3 over 16 stored channels (openaimodel.py:639-645: the UNet's 9 -> 320 input convolution, channels zero-padded) on
    csrc/inconv.hip -- K = 144 in one MFMA pass, outputs stored straight from the accumulator layout: the fp32 carrier against an
    fp64 convolution (16-bit operands are exact there: only the fp32 accumulation order differs), the 16-bit copy = the carrier
    rounded once, the per-64-pixel column statistics = the sums of the carrier, strided views with nothing written outside them,
    and the generic-window kernel (VFACE_TUNE_NO_PATCH) to fp32 rounding."""
    from vface_amd import packing
    h = hip()
    x = rnd((nimg, H, W, 16), 1, dt).to(DEV)
    w = rnd((cout, 16, 3, 3), 2, dt, 1 / 12.0)
    wp = packing.pack_conv3x3(w.float(), 16).to(device=DEV, dtype=dt)
    assert wp.shape == (cout, 144)
    bias = rnd((cout,), 3, torch.float32).to(DEV)
    M = nimg * H * W
    ref = F.conv2d(x.double().permute(0, 3, 1, 2).cpu(), w.double(), bias.double().cpu(), padding=1).permute(0, 2, 3, 1).reshape(M, cout)
    outs = {}
    for tag, fl in (("in16", 0), ("generic", h.TUNE_NO_PATCH)):
        o16 = torch.full((M, cout + 32), 7.0, dtype=dt, device=DEV)
        o32 = torch.full((M, cout + 8), 7.0, dtype=torch.float32, device=DEV)
        cs = torch.full((M // 64, cout + 4, 2), 7.0, dtype=torch.float32, device=DEV)
        h.conv3x3(x.reshape(M, 16), wp, o16[:, 16:16 + cout], nimg=nimg, H=H, W=W, cin=16, cout=cout, ldx=16, ldy=cout + 32, bias=bias,
                  colstats=cs[:, 4:], out32=o32[:, 8:], flags=fl, split_k=False)
        outs[tag] = (o16, o32, cs)
        assert rel_l2(o32[:, 8:].double().cpu(), ref) < 2e-6, tag
        assert torch.equal(o16[:, 16:16 + cout], o32[:, 8:].to(dt)), f"{tag}: the 16-bit copy is the carrier rounded once"
        assert bool((o16[:, :16] == 7).all()) and bool((o16[:, 16 + cout:] == 7).all()) and bool((o32[:, :8] == 7).all()) and bool((cs[:, :4] == 7).all())
        v = o32[:, 8:].double().reshape(M // 64, 64, cout)
        assert torch.allclose(cs[:, 4:, 0].double(), v.sum(1), rtol=1e-5, atol=1e-4), tag
        assert torch.allclose(cs[:, 4:, 1].double(), (v * v).sum(1), rtol=1e-5, atol=1e-4), tag
    assert torch.allclose(outs["in16"][1], outs["generic"][1], rtol=1e-5, atol=2e-5)
    # the carrier alone (no 16-bit copy, no statistics), and the copy alone
    o32 = torch.empty(M, cout, dtype=torch.float32, device=DEV)
    h.conv3x3(x.reshape(M, 16), wp, None, nimg=nimg, H=H, W=W, cin=16, cout=cout, ldx=16, ldy=0, bias=bias, out32=o32, split_k=False)
    assert torch.equal(o32, outs["in16"][1][:, 8:])
    o16 = torch.empty(M, cout, dtype=dt, device=DEV)
    h.conv3x3(x.reshape(M, 16), wp, o16, nimg=nimg, H=H, W=W, cin=16, cout=cout, ldx=16, ldy=cout, split_k=False)
    ref0 = ref - bias.double().cpu()
    assert rel_l2(o16.double().cpu(), ref0) < (1e-3 if dt == torch.float16 else 8e-3)


@pytest.mark.parametrize("dh,n,B", [(40, 1100, 3), (80, 640, 2), (160, 256, 3), (160, 300, 2), (160, 128, 2)])
def test_attention_wave_count_and_query_tiling_do_not_change_bits(dh, n, B):
    """The plain attention kernel's launch forms -- eight waves per workgroup (dh = 40: the default since round 5; variant bit 3 =
    four) and dh = 160's three forms by map size -- walk the same key blocks per query in the same order: same bits on ordinary
    inputs.  (On inputs that trip the speculative reference the RERUN is a workgroup's decision, so a query's bits may depend on
    which queries share its workgroup -- a function of the map, never of the batch: there every form is held to the fp64 attention
    instead.)"""
    h = hip()
    dt, heads = torch.float16, 8
    d = heads * dh
    scale = dh ** -0.5
    kw = dict(B=B, heads=heads, n=n, nk=n, dh=dh, ldq=3 * d, ldk=3 * d, ldv=3 * d, bsq=n * 3 * d, bsk=n * 3 * d, bsv=n * 3 * d, ldo=d, bso=n * d,
              scale=scale)
    base = rnd((B, n, 3 * d), 31, dt)
    peaked = base.clone()
    peaked[..., :d] *= 5.0
    spike = base.clone()
    spike[:, n - 3, d:2 * d] *= 40.0                 # one late key far above everything the first block saw
    for name, qkv in (("plain", base), ("peaked", peaked), ("spike", spike)):
        qd = qkv.to(DEV)
        outs = {}
        for variant in (0, 8) if dh != 160 else (0,):
            out = torch.zeros(B, n, d, dtype=dt, device=DEV)
            h.attention(qd, qd[:, :, d:], qd[:, :, 2 * d:], out, variant=variant, **kw)
            outs[variant] = out
        if dh == 160:
            # the forms are chosen by the map size: the same queries as part of a longer / shorter query set (keys unchanged) take
            # another form -- rows [0, 64) of this call against a call that only asks for those
            out = outs[0]
            kw64 = dict(kw, n=64)
            part = torch.zeros(B, 64, d, dtype=dt, device=DEV)
            h.attention(qd, qd[:, :, d:], qd[:, :, 2 * d:], part, **dict(kw64, ldo=d, bso=64 * d))
            assert torch.equal(out[:, :64], part), name
        elif name == "plain":
            assert torch.equal(outs[0], outs[8]), name
        sp = lambda t: t.reshape(B, n, heads, dh).permute(0, 2, 1, 3).double()
        s_ = sp(qkv[..., :d]) @ sp(qkv[..., d:2 * d]).transpose(-1, -2) * scale
        ref = (torch.softmax(s_, -1) @ sp(qkv[..., 2 * d:])).permute(0, 2, 1, 3).reshape(B, n, d).float()
        for variant, out in outs.items():
            assert torch.isfinite(out).all(), (name, variant)
            assert rel_l2(out.float().cpu(), ref) < (1e-3 if name == "plain" else 3e-3), (name, variant)


# ------------------------------------------------------------------ the frame-mixing kernels of the staged hook modes
# Buffers laid out as UNetEngine._attn1_att lays them: one qkv buffer [3 F n, 3d], q|k = C_ = 2d columns at ld = 3d, frame stride
# n 3d, chunk k at rows [k F n, (k + 1) F n).  The whole buffer starts as a sentinel pattern, so a write outside the q|k columns
# of the target chunks shows.
# (U32, ulp() and sentinel() live in tests/kernel_bounds.py, shared with test_glue_kernels_gpu.py)


# (the largest clips at the largest maps are trimmed to ~0.2 GB of buffer, except the level-0 pairing n = 4096, d = 320 at every F,
# which at F = 32 is the headline clip's own temporal shape, 0.75 GB)
TEMPORAL_CASES = [(F_, n, d) for F_ in (1, 2, 3, 5, 7, 32) for n in (64, 1000, 4096) for d in (32, 320, 1280)
                  if F_ * n * d <= 11_000_000 or (n, d) == (4096, 320)]


@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("F_,n,d", TEMPORAL_CASES)
def test_temporal_gauss(dt, F_, n, d):
    """fusion="temporal": chunk 1 and chunk 2 q|k = the window-5 Gaussian over the frames of chunk 0's q|k, renormalised at the clip
    ends (oracle.hooks.temporal_attention, pnp_utils.py:59-90), evaluated in fp64 on the exact 16-bit inputs.
    Bound per element: one rounding to the output type, 0.5 ulp(ref), plus the kernel's fp32 arithmetic -- at most 5 products and
    5 sums for the weighted sum and the weight total, one division, and weights that are fp32 roundings of exp(-0.5 o^2) / sum
    (the oracle's as well as the kernel's): 16 u S with u = 2^-24 and S = sum_o w_o |x_o| / sum_o w_o, the scale of the terms
    (it only matters where the weighted sum cancels towards zero)."""
    h = hip()
    Fn, C3 = F_ * n, 3 * d
    host = sentinel(3 * Fn, C3, dt)
    x = rnd((Fn, 2 * d), 1000 * F_ + d + n, dt)
    host[:Fn, :2 * d] = x
    ref = ohooks_temporal(x.double().reshape(F_, n, 2 * d)).reshape(Fn, 2 * d)
    scale = ohooks_temporal(x.double().abs().reshape(F_, n, 2 * d)).reshape(Fn, 2 * d)
    bound = 0.5 * ulp(ref, dt) + 16 * U32 * scale
    for with_dst2 in (True, False):
        buf = host.to(DEV)
        h.temporal_gauss(buf, buf[Fn:], buf[2 * Fn:] if with_dst2 else None, F=F_, n=n, C_=2 * d, ld_src=C3, fs_src=n * C3,
                         ld_dst=C3, fs_dst=n * C3)
        got = buf.cpu()
        assert torch.equal(got[:Fn], host[:Fn]), "chunk 0 must not change"
        assert torch.equal(got[:, 2 * d:], host[:, 2 * d:]), "the v columns must not change"
        for ch in ((1, 2) if with_dst2 else (1,)):
            g = got[ch * Fn:(ch + 1) * Fn, :2 * d].double()
            err = (g - ref).abs()
            worst = int(torch.argmax(err / bound))
            assert bool((err <= bound).all()), (f"chunk {ch}, dst2={with_dst2}: {int((err > bound).sum())} elements out of bound; worst "
                                                f"frame {worst // (2 * d) // n}: got {float(g.flatten()[worst])} ref {float(ref.flatten()[worst])}")
        if not with_dst2:
            assert torch.equal(got[2 * Fn:], host[2 * Fn:]), "dst2 = None: chunk 2 must not change"


def ohooks_temporal(x):
    from oracle import hooks as ohooks
    return ohooks.temporal_attention(x)


def test_temporal_gauss_rejects_unaligned_channels():
    h = hip()
    buf = torch.zeros(3 * 2 * 64, 3 * 36, dtype=torch.float16, device=DEV)
    with pytest.raises(h.VFaceHipError):
        h.temporal_gauss(buf, buf[128:], buf[256:], F=2, n=64, C_=36, ld_src=3 * 36, fs_src=64 * 3 * 36, ld_dst=3 * 36,
                         fs_dst=64 * 3 * 36)


ADAIN_CASES = [(rows, C) for rows in (2, 3, 5, 1023, 5 * 4096, 32 * 4096) for C in (8, 320, 512, 520, 1280, 2048)
               if rows * C <= 32 * 4096 * 320]  # (up to the production level-0 batch of a 32-frame clip: 32 x 4096 rows of 320)


def _adain_bound(dt, a64, b64):
    """Reference and per-element bound of adain_fusion on the exact 16-bit rows ``a64``, ``b64`` [rows, C] (fp64).
    Reference: oracle.hooks.adain_fusion_for_attn(normalized=True) in fp64.
    Bound per element, u = 2^-24.  The kernel keeps a row in registers, one wave per row: each lane sums 8 ceil(C / 512) values in
    order and a 6-level tree folds the lanes, so every fp32 row sum is off by at most L u (sum of |terms|), L = 8 ceil(C/512) + 8.
      mean_a, mean_b  off by  L u mean|a|,  L u mean|b|  (mean_a exact for a constant row: <= 2048 copies of an 11-bit
        significand sum exactly in fp32's 24 bits, and the division by C returns the value)
      k = std_b / (std_a + 1e-5)  relative  (L + 8) u  (two sums of squares, two square roots, one division)
      o = (a - mean_a) k + mean_b  off by  dO = k L u mean|a| + L u mean|b| + (L + 10) u |k (a - mean_a)| + u |o|
        (k's error and the roundings of the subtraction and the product scale k (a - mean_a); the final sum rounds o)
      the global factor 1 / (std(o) + 1e-5), where std(o) is taken of the kernel's own fp32 fused values:
        each row's mean m_r = sum_r / C is off by d_r <= (L + 1) u mean_r|o|; the row's centred M2_r = sum (o - m_r)^2 is off by
        (L + 3) u relative (the subtraction, the square, L sums), and by exactly C d_r^2 from the mean's error; Chan's fold in fp64,
        M2 = sum_r M2_r + C sum_r (m_r - mean)^2, adds a cross term 2 C sum_r (m_r - mean) d_r <= 2 rho M2 (Cauchy-Schwarz) and
        C sum_r d_r^2 <= rho^2 M2 twice, rho = rms_r(d_r) / std(o).  So the std is off by (L + 3) u / 2 + rho + rho^2 relative, and
        the square root, the + 1e-5, the division and the fp32 conversion add 4 u.  A row mean far above the spread does not
        enter: there is no sum o^2 - N mean^2 to cancel;
        plus what the fused values' own errors can move the std by, rms(dO) / std(o)
      the output o / (std + 1e-5): one rounding to the 16-bit type, 0.5 ulp(ref)."""
    from oracle import hooks as ohooks
    C = a64.shape[1]
    ref = ohooks.adain_fusion_for_attn(a64, b64, normalized=True)
    ma, mb = a64.mean(-1, keepdim=True), b64.mean(-1, keepdim=True)
    k = b64.std(-1, keepdim=True) / (a64.std(-1, keepdim=True) + 1e-5)
    o = (a64 - ma) * k + mb
    g = 1.0 / (o.std() + 1e-5)
    L = 8 * -(-C // 512) + 8
    const = (a64 == a64[:, :1]).all(-1, keepdim=True)     # (a constant 16-bit row sums exactly in fp32: its mean is exact)
    d_o = k * L * U32 * a64.abs().mean(-1, keepdim=True) * ~const + L * U32 * b64.abs().mean(-1, keepdim=True) \
        + (L + 10) * U32 * (k * (a64 - ma)).abs() + U32 * o.abs()
    rho = float(((L + 1) * U32 * o.abs().mean(-1)).pow(2).mean().sqrt() / o.std())
    rel_g = ((L + 3) / 2 + 4) * U32 + rho + rho ** 2 + float(d_o.pow(2).mean().sqrt() / o.std())
    return ref, 0.5 * ulp(ref, dt) + g * d_o + rel_g * ref.abs()


def _adain_case(dt, rows, C, a, b):
    """The engine's call (UNetEngine._staged_edit): a = chunk 0's q (or k) columns, b = dst = chunk k's, in place, ld = 3C, in a buffer
    [2 rows, 3C] that starts as a sentinel pattern; the fused slot is the k slot (columns [C, 2C)).  Bound: _adain_bound."""
    h = hip()
    host = sentinel(2 * rows, 3 * C, dt)
    host[:rows, C:2 * C] = a.to(dt)
    host[rows:, C:2 * C] = b.to(dt)
    ref, bound = _adain_bound(dt, host[:rows, C:2 * C].double(), host[rows:, C:2 * C].double())
    buf = host.to(DEV)
    own = buf[rows:, C:2 * C]
    h.adain_fusion(buf[:rows, C:2 * C], own, own, rows=rows, C_=C, lda=3 * C, ldb=3 * C, ldd=3 * C)
    got = buf.cpu()
    assert torch.equal(got[:rows], host[:rows]), "chunk 0 must not change"
    assert torch.equal(got[rows:, :C], host[rows:, :C]) and torch.equal(got[rows:, 2 * C:], host[rows:, 2 * C:]), \
        "columns outside the fused slot must not change"
    out = got[rows:, C:2 * C].double()
    assert bool(torch.isfinite(out).all())
    err = (out - ref).abs()
    worst = int(torch.argmax(err / bound))
    assert bool((err <= bound).all()), (f"{int((err > bound).sum())} of {err.numel()} out of bound; worst row {worst // C}: got "
                                        f"{float(out.flatten()[worst])} ref {float(ref.flatten()[worst])} (bound {float(bound.flatten()[worst]):.3e})")
    return out, ref, err


@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("rows,C", ADAIN_CASES)
def test_adain_fusion(dt, rows, C):
    """fusion="adaIn": per row, the AdaIN of chunk 0's row to chunk k's over the channels, then the whole tensor divided by its
    GLOBAL unbiased std (face_swap_utils.py:372-389).  Rows cross the 4-rows-per-block tail and reach the production row count of
    the one-block fp64 reduce; C crosses each 512-channel register boundary.  Row 1 of ``a`` is constant: its std is 0, so its
    fused row is b's row mean, times the global factor."""
    a = rnd((rows, C), 11 * rows + C, torch.float32)
    b = rnd((rows, C), 13 * rows + C, torch.float32, 2.0) + 0.5
    a[1] = 0.75
    out, ref, _ = _adain_case(dt, rows, C, a, b)
    b1 = b[1].to(dt).double()
    assert torch.equal(ref[1], ref[1, :1].expand(C)) and bool(torch.isfinite(out[1]).all())
    assert float((out[1] - ref[1]).abs().max()) <= float(ulp(ref[1, :1], dt)), (out[1, :4], b1.mean())


@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("rows,C", [(2, 320), (5, 2048), (1023, 520), (5 * 4096, 320), (32 * 4096, 320)])
def test_adain_fusion_offset_rows(dt, rows, C):
    """Row means far above the spread (b ~ 50 + N(0,1), a ~ -30 + N(0,1)): the fused tensor is ~50 +- 1.  Its global variance formed
    as (sum o^2 - N mean^2) / (N - 1) from fp32 row sums would lose digits in proportion to mean^2 / var (~2500 here, a std off by
    up to ~1e-3 relative at 2 rows of 320); from centred row partials folded with Chan's formula it keeps the bound above."""
    a = rnd((rows, C), 17 * rows + C, torch.float32) - 30.0
    b = rnd((rows, C), 19 * rows + C, torch.float32) + 50.0
    _, ref, err = _adain_case(dt, rows, C, a, b)
    print(f"adaIn offset {dt} rows={rows} C={C}: max |err| {float(err.max()):.3e} at |ref| ~ {float(ref.abs().mean()):.1f}")


def test_adain_fusion_rejects_wide_rows():
    h = hip()
    C = 2056
    a = torch.zeros(4, C, dtype=torch.float16, device=DEV)
    with pytest.raises(h.VFaceHipError):
        h.adain_fusion(a, a, a, rows=4, C_=C, lda=C, ldb=C, ldd=C)


@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("dh,n", [(40, 1024), (8, 256), (160, 64)])
def test_attention_engine_v_fixed_map_five_frames(dt, dh, n):
    """fusion="fft_vfixed" with the engine's own sample map (engine.sample_map("v_fixed"), what UNetEngine._map caches on the device)
    at B = 3 x 5: chunk 0 keeps its own v,
    every frame of chunk k >= 1 attends with the v of chunk k's FIRST frame.  The reference v is built from the reference's own
    expression (pnp_utils.py:255-256: v[c:2c] = v[c].repeat(c), v[2c:] = v[2c].repeat(c)), not from the map; fp64."""
    from vface_amd.engine import sample_map
    h = hip()
    B, heads, c = 15, 8, 5
    d = heads * dh
    qkv = rnd((B, n, 3 * d), 23 + dh, dt)
    v_map = sample_map("v_fixed", B, c).to(DEV)
    out = torch.empty(B, n, d, dtype=dt, device=DEV)
    qd = qkv.to(DEV)
    scale = dh ** -0.5
    h.attention(qd, qd[:, :, d:], qd[:, :, 2 * d:], out, B=B, heads=heads, n=n, nk=n, dh=dh, ldq=3 * d, ldk=3 * d,
                ldv=3 * d, bsq=n * 3 * d, bsk=n * 3 * d, bsv=n * 3 * d, ldo=d, bso=n * d, scale=scale, v_map=v_map)
    v = qkv[..., 2 * d:].double().clone()
    v[c:2 * c] = v[c].repeat(c, 1, 1)
    v[2 * c:] = v[2 * c].repeat(c, 1, 1)
    sp = lambda t: t.reshape(B, n, heads, dh).permute(0, 2, 1, 3).double()
    s_ = sp(qkv[..., :d]) @ sp(qkv[..., d:2 * d]).transpose(-1, -2) * scale
    ref = (torch.softmax(s_, -1) @ sp(v)).permute(0, 2, 1, 3).reshape(B, n, d)
    got = out.cpu().double()
    per = [rel_l2(got[i], ref[i]) for i in range(B)]
    assert max(per) < TOL[dt], [f"{e:.1e}" for e in per]
