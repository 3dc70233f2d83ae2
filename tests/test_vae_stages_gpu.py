"""The first-stage KL-VAE engine (vface_amd/vae_engine.py) stage by stage: the mid attention past 64 tokens, odd sizes, H != W.

Every launch ``VAEEngine`` makes, with its flags and operand forms, against the test that pins it (stage cases: tests/vae_model.py
``STAGES``; fixtures: tests/golden/vae_stages.npz, cases_vae.py):

  launch                                      flags / operand form                                     pinned by
  vface_nchw_to_nhwc                          fp32 NCHW -> 16-bit NHWC, 8 stored channels              engine_on_fixtures, input_forms (per element:
                                                                                                       test_glue_kernels_gpu.py)
  vface_conv3x3, stride 1                     bias; column statistics when hw % 64 == 0                stage[res.*], stage[dec_head.*]
  vface_conv3x3, stride 1, residual           16-bit residual rows, ldr = C                            stage[res.*]
  vface_conv3x3, stride 2                     VFACE_CONV_PAD_TRAILING                                  stage[down.*], test_vae_gpu.py::test_trailing_pad_stride2_conv
  vface_conv3x3, upsample                     nine taps on the upsampled grid                          stage[up.128.6x10]
  vface_upsample2x_conv3x3_phase x 4          pre-summed 2 x 2 taps, column statistics                 stage[up.512.16x24] (asserts which form ran)
  vface_conv3x3, VFACE_EPI_OUT_F32            N = 8 (quant_conv folded in) / N = 4 (3 + one zero)      stage[enc_tail.*], stage[dec_tail.*]
  vface_groupnorm_stats                       from pixels, eps 1e-6 (hw % 64 != 0)                     stage[*.6x10], attn_unit[16x128, 120x128]
  vface_groupnorm_stats_from_cols             from the producer's column sums (hw % 64 == 0)           stage[*.16x24, *.8x16], attn_unit[768x512, 4096x512]
  vface_groupnorm_apply                       with and without swish, ldy = C                          stage[res.*], attn_unit
  vface_gemm  nin_shortcut                    bias, rows_per_sample = hw                               stage[res.128.256.*, res.256.512.*]
  vface_gemm  q | k                           N = 2 c, bias                                            attn_unit
  vface_gemm  scores                          A, Wt = halves of one [n, 2c] buffer (lda = ldw = 2c),   attn_score_gemm
                                              VFACE_EPI_OUT_F32, N = n; never splits K
  vface_softmax_rows                          fp32 [n, n] -> 16-bit, scale c^-1/2, ld = n              attn_softmax_rows, test_vae_gpu.py::test_softmax_rows_kernel
  vface_gemm  V^T = Wv h^T                    the WEIGHT is A (M = c), Wt = activation rows, N = n     attn_vt_gemm
  vface_gemm  P V^T                           K = lda = ldw = n, column bias = value bias; splits K    attn_pv_gemm (split and unsplit at K = 4096, 9216),
                                              by 4 at (n, c) = (4096, 512), not at 768 or 9216         attn_unit[4096x512] (the engine's own call)
  vface_gemm  proj_out                        bias, 16-bit residual, column statistics, rps = n        attn_unit (+ the returned statistics)
  vface_gemm  post_quant                      M x 8 x 8, bias                                          stage[dec_head.*]
  vface_nhwc_to_nchw_f32                      ldx = 4                                                  engine_on_fixtures, chunking

Tolerances.  (a) is per element against fp64 with kernel_bounds.py's bounds.  (b), (c) and the intermediates of (d): rel-L2 and the
worst element's |err| / rms(ref) against fp64 (``oracle.vae`` on the host, fed the engine's own 16-bit stage input and the unrounded
weights), each against the SAME figure of tests/vae_model.py on the same inputs, computed on the CPU: rel-L2 x 1.25 (the project's
allowance in test_clip_gpu.py: fp32 accumulation order, BLAS against MFMA), the worst element x 2 (an extreme-value statistic of the
same distribution; which element the order hits moves it).  No bound comes from the GPU's output.  test_vae_bound_cpu.py shows that
these tolerances refuse eleven one-line defects on the stage cases that own them.  Final outputs of (d) also keep
test_vae_gpu.py's rule: below 1.1 x the reference's own autocast error."""
import math

import pytest
import torch

import vae_model as vm
from vae_model import cv
from conftest import load_golden, rel_l2
from kernel_bounds import Framed, assert_within, colstats_ref_and_bound, gemm_ref_and_bound, note, rnd, same_bits, softmax_rows_ref_and_bound

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DTS = list(vm.DTS)
ATTN_SHAPES = [(16, 128), (120, 128), (768, 512)]


def hip():
    from vface_amd import hip as h
    h.load()
    return h


def splits_of(h, M, N, K, flags=0, rps=1):
    return max(1, h.load().vface_splitk_workspace_bytes(M, N, K, flags, rps) // (M * N * 4))


# ================================================================================================ (a) the launches of _attn, per element
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("n,c", ATTN_SHAPES)
def test_attn_score_gemm(dt, n, c):
    """scores = q k^T: both operands are column views of one [n, 2c] buffer, fp32 out, N = n (a tail in N at n = 16 and 120)."""
    h = hip()
    qk = rnd((n, 2 * c), 7 * n + c, dt)
    assert h.load().vface_splitk_workspace_bytes(n, n, c, h.EPI_OUT_F32, 1) == 0, "an fp32-output launch never splits K"
    qkd = qk.to(DEV)
    out = Framed(n, n, torch.float32)
    h.gemm(qkd, qkd[:, c:], out.view, M=n, N=n, K=c, lda=2 * c, ldw=2 * c, ldc=out.ld, flags=h.EPI_OUT_F32)
    ref, bound = gemm_ref_and_bound(qk[:, :c], qk[:, c:], dt, out_f32=True)
    note("vae attn scores", assert_within(out.result(f"scores {n}x{c}"), ref, bound, f"scores {dt} n={n} c={c}"), bound)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("n,c", ATTN_SHAPES)
def test_attn_softmax_rows(dt, n, c):
    """The engine's form: contiguous [n, n], scale c^-1/2 (2^-3.5, 2^-4.5: not a power of two), scaled scores of the peaked family's
    size, std 6.25: one dominant row, one flat row."""
    h = hip()
    scale = float(int(c) ** -0.5)
    S = torch.randn((n, n), generator=torch.Generator().manual_seed(n + c)) * (6.25 / scale)
    S[0, n // 3] = S[0].max() + 100.0 / scale
    S[1] = 2.5
    od = torch.full((n + 1, n), -3.0, dtype=dt, device=DEV)
    h.softmax_rows(S.to(DEV), od, M=n, N=n, scale=scale)
    got = od.cpu()
    ref, bound = softmax_rows_ref_and_bound(S, scale, dt)
    note("vae attn softmax", assert_within(got[:n], ref, bound, f"softmax {dt} n={n}"), bound)
    assert float(got[0, n // 3]) == 1.0 and int((got[0] != 0).sum()) == 1 and bool((got[n] == -3.0).all())


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("n,c", ATTN_SHAPES)
def test_attn_vt_gemm(dt, n, c):
    """V^T = Wv h^T: the weight is the A operand (M = c), the activation rows are Wt, N = n."""
    h = hip()
    wv, g = rnd((c, c), 3 * n + c, dt, 1 / math.sqrt(c)), rnd((n, c), 5 * n + c, dt)
    assert splits_of(h, c, n, c) == 1
    out = Framed(c, n, dt)
    h.gemm(wv.to(DEV), g.to(DEV), out.view, M=c, N=n, K=c, lda=c, ldw=c, ldc=out.ld)
    ref, bound = gemm_ref_and_bound(wv, g, dt)
    note("vae attn V^T", assert_within(out.result(f"V^T {n}x{c}"), ref, bound, f"V^T {dt} n={n} c={c}"), bound)


def softmax_operand(M, K, dt, seed):
    """Real softmax rows as the A operand: non-negative, summing to 1; row 0 peaked (all its mass on one key), row 1 flat."""
    S = torch.randn((M, K), generator=torch.Generator().manual_seed(seed)) * 3.0
    S[0, K // 3] = 200.0
    S[1] = 0.0
    return torch.softmax(S.double(), 1).to(dt)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("K,M,N,split", [(16, 16, 128, True), (120, 120, 128, True), (768, 768, 512, True), (4096, 200, 72, True),
                                         (4096, 200, 72, False), (9216, 200, 72, True), (9216, 200, 72, False)])
def test_attn_pv_gemm(dt, K, M, N, split):
    """att = P V^T + bv: K = lda = ldw = n with the value bias as the column bias.  The short K are the engine's own (M, N) = (n, c);
    at the two production lengths only the K loop is under test (M = 200, N = 72).  ``split``: the binding's default workspace (8
    shares at M x N = 200 x 72) or none -- the engine's own call splits by 4 at (4096, 512) and not at (9216, 512) or below."""
    h = hip()
    assert splits_of(h, 4096, 512, 4096) == 4 and splits_of(h, 9216, 512, 9216) == 1 and splits_of(h, 768, 512, 768) == 1
    s = splits_of(h, M, N, K) if split else 1
    assert s == (8 if K >= 4096 and split else 1), "the shape no longer splits as this case assumes"
    P, vt, bv = softmax_operand(M, K, dt, K + M), rnd((N, K), K + N, dt), rnd((N,), K, torch.float32)
    out = Framed(M, N, dt)
    h.gemm(P.to(DEV), vt.to(DEV), out.view, M=M, N=N, K=K, lda=K, ldw=K, ldc=out.ld, bias=bv.to(DEV), split_k=split)
    ref, bound = gemm_ref_and_bound(P, vt, dt, bias=bv, splits=s)
    got = out.result(f"P V^T K={K}")
    note("vae attn P V^T", assert_within(got, ref, bound, f"P V^T {dt} K={K} split={s}"), bound)
    assert_within(got[0], (vt[:, K // 3].double() + bv.double()), bound[0], "the peaked row is one key's value plus the bias")


# ================================================================================================ (b), (c) the stages as units
class _Dev(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.p = torch.nn.Parameter(torch.zeros(1, device=DEV))


def engine(dt):
    from vface_amd.vae_engine import VAEEngine
    return VAEEngine(_Dev(), dt)


def to_act(x, dt):
    """NCHW fp32 holding values of ``dt`` -> the engine's ``Act``, with the column sums its producer would have left (hw % 64 == 0:
    the fp64 sums of the stored values per 64-row slice, rounded to fp32) or without (the next GroupNorm reads the pixels)."""
    from vface_amd.engine import Act
    B, C, H, W = x.shape
    t = vm.tokens(x)
    cs = None
    if (H * W) % 64 == 0 and C % 8 == 0:
        s = t.double().reshape(-1, 64, C)
        cs = torch.stack([s.sum(1), (s * s).sum(1)], -1).float().to(DEV)
    return Act(t.to(dt).to(DEV), B, H, W, cs)


def from_act(a, cols=None):
    torch.cuda.synchronize()
    t = a.t.float().cpu()
    return vm.image(t if cols is None else t[:, :cols], a.N, a.H, a.W)


def hold(name, dt, got, ref, model_figs):
    """Print, then assert, the two figures of a stage against the model's (DESIGN.md's VAE table is these lines)."""
    l2, worst = vm.figures(got, ref)
    m_l2, m_worst = model_figs
    print(f"[vae stage] {name} {str(dt)[6:]}: rel-L2 model {m_l2:.3e} bound {vm.MARGIN_L2 * m_l2:.3e} measured {l2:.3e} | worst model "
          f"{m_worst:.3e} bound {vm.MARGIN_WORST * m_worst:.3e} measured {worst:.3e}")
    assert bool(torch.isfinite(got).all()), name
    assert l2 <= vm.MARGIN_L2 * m_l2, (name, dt, "rel-L2", l2, m_l2)
    assert worst <= vm.MARGIN_WORST * m_worst, (name, dt, "worst element", worst, m_worst)


def check_returned_stats(a, name):
    """The column statistics a stage hands to the next GroupNorm, against the fp64 sums of what it stored."""
    if a.hw % 64:
        assert a.cs is None, name
        return
    assert a.cs is not None, name
    torch.cuda.synchronize()
    stored = a.t.cpu()
    # Which 64 rows of an image a slice holds differs between the kernels (plain rows, 8 x 8 patches, one parity phase); what the
    # next GroupNorm folds is the image's slices together, so that is what is held: the fp64 total of an image's hw / 64 slices
    # against the fp64 sums of the image's stored rows, with the bound of 64-row fp32 sums (``colstats_ref_and_bound``).
    assert tuple(a.cs.shape) == (a.M // 64, a.C, 2)
    ref, bound = colstats_ref_and_bound(stored, [torch.arange(i * a.hw, (i + 1) * a.hw) for i in range(a.N)])
    got = a.cs.cpu().double().reshape(a.N, a.hw // 64, a.C, 2).sum(1)
    bound = bound * (68.0 / (a.hw + 4))                 # 64 + 4 roundings per term, not hw + 4: the slices meet in fp64 here
    note("vae stage colstats", assert_within(got, ref, bound, f"{name} column statistics per image"), bound)


ATTN_UNITS = [(n, dt) for n in vm.STAGES if vm.STAGES[n][0] == "attn" and n not in vm.LARGE for dt in DTS] + \
             [(n, torch.float16) for n in vm.LARGE]


@pytest.mark.parametrize("name,dt", ATTN_UNITS)
def test_attn_unit(name, dt):
    """``VAEEngine._attn`` against ``oracle.vae.attn_block`` in fp64: n = 16, 120 (10 x 12), 768 (24 x 32) with two frames that differ
    in scale, in both score families, and once the production shape n = 4096, c = 512 (one frame, fp16)."""
    sd, x, ref, figs = vm.stage_clean(name, dt)
    eng = engine(dt)
    out = eng._attn(to_act(x, dt), vm.stage_pack(name, sd, dt, DEV))
    hold(name, dt, from_act(out), ref, figs)
    check_returned_stats(out, name)


OTHER_UNITS = [n for n in vm.STAGES if vm.STAGES[n][0] != "attn"]


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("name", OTHER_UNITS)
def test_stage_unit(name, dt, monkeypatch):
    """Every other stage as the engine sequences it, against the matching ``oracle.vae`` function in fp64."""
    h = hip()
    kind, g, _ = vm.STAGES[name]
    sd, x, ref, figs = vm.stage_clean(name, dt)
    eng, P = engine(dt), vm.stage_pack(name, sd, dt, DEV)
    phase_launches = []
    real = h.upsample2x_conv3x3
    monkeypatch.setattr(h, "upsample2x_conv3x3", lambda *a, **k: (phase_launches.append(1), real(*a, **k))[1])
    if kind == "res":
        out = eng._res(to_act(x, dt), P)
    elif kind == "down":
        out = eng._conv(to_act(x, dt), P, stride=2, trailing_pad=True)
    elif kind == "up":
        from vface_amd.engine import _phase_form_pays
        assert ((g["H"] * g["W"]) % 64 == 0 and _phase_form_pays(g["H"] * g["W"], g["c"])) == vm.PHASE_FORM[name]
        out = eng._conv(to_act(x, dt), P, upsample=True)
        assert bool(phase_launches) == vm.PHASE_FORM[name], "the other upsampling form ran"
    elif kind == "dec_head":
        out = eng._post_quant_conv_in(eng._input(x.to(DEV)), P)
    elif kind == "enc_tail":
        out = eng._norm_out_conv(to_act(x, dt), P["enc.norm_out"], P["enc.conv_out"])
    else:
        out = eng._norm_out_conv(to_act(x, dt), P["dec.norm_out"], P["dec.conv_out"])
    hold(name, dt, from_act(out, ref.shape[1]), ref, figs)
    if kind in ("enc_tail", "dec_tail"):
        assert out.t.dtype == torch.float32 and out.cs is None
        if kind == "dec_tail":
            assert bool((out.t[:, 3] == 0).all()), "the zero output channel that pads N to 4"
    else:
        check_returned_stats(out, name)


# ================================================================================================ (d) the engine on the new fixtures
def build_vae(case, dt):
    from vface_amd.ldm.models.autoencoder import AutoencoderKL
    from vface_amd.utils import synth
    m = AutoencoderKL(ddconfig=cv.DD[cv.CASES[case]["cfg"]], embed_dim=4, compute_dtype=dt)
    synth.fill_module_(m, seed=0, prefix="vae.")
    return m.to(DEV)


@pytest.mark.parametrize("dt,tag", [(torch.float16, "f16"), (torch.bfloat16, "bf16")])
@pytest.mark.parametrize("case", list(cv.CASES))
def test_engine_on_fixtures(case, dt, tag):
    """``ragged`` (two frames of 80 x 96: n = 120, pixel statistics at the two deepest levels) at every recorded intermediate, and the
    final outputs of ``ragged`` and ``wide`` (192 x 256: n = 768, c = 512), on the fixture's elements."""
    g = load_golden("vae_stages")
    model_out, model_taps = vm.run_case(case, dt, g)
    m = build_vae(case, dt)
    assert sum(p.numel() for p in m.parameters()) == int(g[f"{case}.n_params"])
    x, noise = cv.inputs(case)
    taps = {}
    post = m.engine.encode(x.to(DEV), taps=taps)
    dec = m.engine.decode((g[f"{case}.z_sample"].float() / cv.SCALE).to(DEV), taps=taps).cpu()
    got = {"z_mode": post.mode(cv.SCALE).cpu(), "z_sample": post.sample(noise.to(DEV), cv.SCALE).cpu(), "dec": cv.take(case, "dec", dec, cv.K_DEC)}
    if case == "ragged":
        assert sorted(taps) == sorted(cv.enc_stages() + cv.dec_stages())
        for k in cv.enc_stages() + cv.dec_stages():
            ref = g[f"ragged.{k}"]
            hold(f"ragged.{k}", dt, cv.take(case, k, from_act(taps[k])), ref, vm.figures(cv.take(case, k, model_taps[k]), ref))
    for k in ("z_mode", "z_sample", "dec"):
        ref = g[f"{case}.{k}"]
        hold(f"{case}.{k}", dt, got[k], ref, vm.figures(model_out[k], ref))
        if tag in cv.AUTOCAST[case]:
            e, e_ref = rel_l2(got[k], ref), rel_l2(vm.autocast_output(g, case, k, tag), ref)
            print(f"[vae fixture] {case}.{k} {tag}: {e:.3e}; the reference under autocast {e_ref:.3e}")
            assert e < 1.1 * e_ref, (case, k, tag, e, e_ref)


# ================================================================================================ (e) engine properties at small size
def test_chunking_does_not_change_a_bit():
    """F = 5 with ``max_frames`` = 2 (chunks of 2, 2, 1) equals ``max_frames`` = 8 (one chunk) bit for bit, encode and decode."""
    from vface_amd.utils import synth
    from vface_amd.vae_engine import VAEEngine
    m = build_vae("ragged", torch.float16)
    x = synth.synth_normal("vae.chunks.x", (5, 3, 32, 48)).clamp(-1, 1).to(DEV)
    x[3] *= 0.25
    whole, split = VAEEngine(m, torch.float16, max_frames=8), VAEEngine(m, torch.float16, max_frames=2)
    mo = whole.encode(x).parameters
    assert same_bits(mo, split.encode(x).parameters)
    z = whole.encode(x).mode()
    d = whole.decode(z)
    assert d.shape == (5, 3, 32, 48) and bool(torch.isfinite(d).all()) and same_bits(d, split.decode(z))


def test_a_frame_alone_equals_the_frame_in_the_batch():
    g = load_golden("vae_stages")
    m = build_vae("ragged", torch.float16)
    x, _ = cv.inputs("ragged")
    x = x.to(DEV)
    z = (g["ragged.z_sample"].float() / cv.SCALE).to(DEV)
    both, alone = m.encode(x).parameters, m.encode(x[1:2]).parameters
    n = alone.shape[0]
    assert n == 120 and same_bits(both[n:2 * n], alone)
    assert same_bits(m.decode(z)[1:2], m.decode(z[1:2]))


def test_input_forms():
    """A non-contiguous input and a 16-bit input are the same frames: bit-equal to the contiguous fp32 tensor of the same values."""
    m = build_vae("ragged", torch.float16)
    x, _ = cv.inputs("ragged")
    x16 = x.half()
    want = m.encode(x16.float().to(DEV)).parameters
    assert same_bits(m.encode(x16.to(DEV)).parameters, want), "a 16-bit input"
    nc = x16.float().to(DEV).permute(0, 1, 3, 2).contiguous().permute(0, 1, 3, 2)
    assert not nc.is_contiguous() and same_bits(m.encode(nc).parameters, want), "a non-contiguous input"
    z = m.encode(x16.float().to(DEV)).mode()
    dwant = m.decode(z)
    zn = z.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
    assert not zn.is_contiguous() and same_bits(m.decode(zn), dwant)
    assert same_bits(m.decode(z.half()), m.decode(z.half().float()))


# ================================================================================================ section 4: refused up front
@pytest.mark.parametrize("side,shape", [("encode", (1, 3, 88, 88)), ("encode", (2, 3, 8, 2056)), ("decode", (1, 4, 11, 11)),
                                        ("decode", (2, 4, 1, 257))])
def test_sizes_the_launches_cannot_run_are_refused_before_anything_runs(side, shape, monkeypatch):
    """88 x 88 (n = 121) and 8 x 2056 (n = 257): the error names the rule, no kernel wrapper returns (every one of them ends in
    ``hip._check``), nothing is allocated and the packed weights are not even built."""
    h = hip()
    m = build_vae("ragged", torch.float16)
    eng = m.engine
    x = torch.zeros(shape, device=DEV)
    torch.cuda.synchronize()
    calls, before = [], torch.cuda.memory_allocated()
    real = h._check
    monkeypatch.setattr(h, "_check", lambda rc, what: (calls.append(what), real(rc, what))[1])
    with pytest.raises(h.VFaceHipError, match="multiple of 8 and at most 16384"):
        getattr(eng, side)(x)
    assert not calls and eng._packed is None and torch.cuda.memory_allocated() == before
    monkeypatch.undo()
    ok = eng.encode(torch.zeros(1, 3, 32, 32, device=DEV)) if side == "encode" else eng.decode(torch.zeros(1, 4, 4, 4, device=DEV))
    assert eng._packed is not None and ok is not None
