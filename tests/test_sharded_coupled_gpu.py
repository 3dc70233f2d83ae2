"""Frame sharding of the frame-coupled hook modes, ``temporal`` (+-2 frames) and ``adaIn`` (a std over every frame), on the MI355X box.

* The kernel entry points the sharded edit runs: ``vface_temporal_gauss_halo`` on every shard equals the unsharded
  ``vface_temporal_gauss``'s rows bit for bit (the headline's level-0 shape at F = 32 included); ``vface_adain_rows`` per shard, the
  partials concatenated in row order, then ``vface_adain_reduce_scale`` equals ``vface_adain_fusion`` bit for bit.
* The whole UNet: shards run as gloo processes on the one GPU (host staging, as tests/test_sharded_gpu.py's two-process run) and
  their concatenated eps must ``torch.equal`` the unsharded run -- both exchange forms, eager and hipGraph-segmented replay, and two
  DDIMSampler steps (shared uncond / cond prefix, with and without the dead branches).
(The in-process harnesses of tests/test_sharded_gpu.py -- the loop-back shards and the RCCL self-loop -- run the shards of a clip
one after another; they cannot carry these exchanges: a shard's temporal halo needs the NEXT shard's frames and the adaIn gather
every shard's rows before the earlier shard's forward can go on.)"""
import os

import pytest
import torch
import torch.multiprocessing as mp

from vface_amd.parallel import frame_range

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _cfg():
    return dict(image_size=32, in_channels=9, out_channels=4, model_channels=64, attention_resolutions=[4, 2, 1],
                num_res_blocks=2, channel_mult=[1, 2, 4, 4], num_heads=8, use_spatial_transformer=True,
                transformer_depth=1, context_dim=768, legacy=False)


def _rnd(shape, seed, dt):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=g).to(dt)


# ------------------------------------------------------------------------------------------------ kernel entry points
@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("F_,n,d,worlds", [(5, 64, 32, (1, 2, 3, 5)), (7, 1000, 320, (2, 4)), (4, 256, 1280, (3,)),
                                           (32, 4096, 320, (1, 3, 32))])
def test_temporal_gauss_halo_equals_unsharded_rows(dt, F_, n, d, worlds):
    """Every shard of ``frame_range`` splits (one-frame shards included) through the halo form, its window frames outside the shard
    read from two-slab buffers (slabs past the clip's ends hold NaN: they must not be read), equals the unsharded kernel's rows."""
    from vface_amd import hip
    Fn, C3 = F_ * n, 3 * d
    src = _rnd((Fn, C3), 7 * F_ + d, dt).to(DEV)
    full = torch.zeros(2 * Fn, C3, dtype=dt, device=DEV)
    hip.temporal_gauss(src, full, full[Fn:], F=F_, n=n, C_=2 * d, ld_src=C3, fs_src=n * C3, ld_dst=C3, fs_dst=n * C3)
    qk = src[:, :2 * d].reshape(F_, n, 2 * d)
    nan = torch.full((n, 2 * d), float("nan"), dtype=dt, device=DEV)
    for world in worlds:
        for r in range(world):
            f0, fc = frame_range(r, world, F_)
            prev = torch.stack([qk[g] if 0 <= g < F_ else nan for g in (f0 - 2, f0 - 1)]).contiguous() if f0 > 0 else None
            nxt = torch.stack([qk[g] if 0 <= g < F_ else nan for g in (f0 + fc, f0 + fc + 1)]).contiguous() if f0 + fc < F_ else None
            out = torch.zeros(2 * fc * n, C3, dtype=dt, device=DEV)
            hip.temporal_gauss_halo(src[f0 * n:], prev, nxt, out, out[fc * n:], F=fc, first=f0, F_total=F_, n=n, C_=2 * d, ld_src=C3,
                                    fs_src=n * C3, ld_dst=C3, fs_dst=n * C3, ld_halo=2 * d, fs_halo=n * 2 * d)
            for ch in range(2):
                got = out[ch * fc * n:(ch + 1) * fc * n]
                ref = full[ch * Fn + f0 * n:ch * Fn + (f0 + fc) * n]
                assert torch.equal(got, ref), f"world {world} rank {r} (frames {f0}..{f0 + fc - 1}), chunk {ch + 1}"


def test_temporal_gauss_halo_rejects_missing_slabs():
    from vface_amd import hip
    buf = torch.zeros(3 * 2 * 64, 3 * 32, dtype=torch.float16, device=DEV)
    slab = torch.zeros(2 * 64, 2 * 32, dtype=torch.float16, device=DEV)
    kw = dict(n=64, C_=64, ld_src=96, fs_src=64 * 96, ld_dst=96, fs_dst=64 * 96, ld_halo=64, fs_halo=64 * 64)
    for prev, nxt, first, total in ((None, slab, 1, 4), (slab, None, 1, 4), (slab, slab, 3, 4)):
        with pytest.raises(hip.VFaceHipError):
            hip.temporal_gauss_halo(buf, prev, nxt, buf[128:], None, F=2, first=first, F_total=total, **kw)


@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("C,splits", [(320, (3 * 4096, 2 * 4096)), (520, (500, 300, 223)), (64, (1024, 1024, 1024, 1024, 1024)),
                                      (2048, (3, 2)), (1280, (64, 1, 191))])
def test_adain_rows_gather_reduce_equals_fusion(dt, C, splits):
    """``vface_adain_rows`` on each shard's rows (uneven splits), the fp64 partials laid side by side in row order -- what the
    exchange's gather hands back --, then ``vface_adain_reduce_scale`` on each shard: ``vface_adain_fusion``'s result bit for bit,
    in the engine's layout (q | k column slot of a 3C-wide buffer, in place)."""
    from vface_amd import hip
    rows = sum(splits)
    host = _rnd((2 * rows, 3 * C), 5 * rows + C, torch.float32)
    host[rows:] = host[rows:] * 2.0 + 0.5
    host = host.to(dt)
    ref = host.to(DEV)
    own = ref[rows:, C:2 * C]
    hip.adain_fusion(ref[:rows, C:2 * C], own, own, rows=rows, C_=C, lda=3 * C, ldb=3 * C, ldd=3 * C)
    buf = host.to(DEV)
    parts, wss, r0 = [], [], 0
    for m in splits:
        p = torch.empty(m, 2, dtype=torch.float64, device=DEV)
        ws = torch.empty(hip.adain_rows_workspace_bytes(m, C), dtype=torch.uint8, device=DEV)
        hip.adain_rows(buf[r0:r0 + m, C:2 * C], buf[rows + r0:rows + r0 + m, C:2 * C], p, ws, rows=m, C_=C, lda=3 * C, ldb=3 * C)
        parts.append(p)
        wss.append(ws)
        r0 += m
    glob = torch.cat(parts).contiguous()
    r0 = 0
    for m, ws in zip(splits, wss):
        hip.adain_reduce_scale(glob, ws, buf[rows + r0:rows + r0 + m, C:2 * C], partial_rows=rows, rows=m, C_=C, ldd=3 * C)
        r0 += m
    assert torch.equal(buf, ref)


def test_adain_split_entry_points_reject_bad_arguments():
    from vface_amd import hip
    C, m = 64, 8
    a = torch.zeros(m, C, dtype=torch.float16, device=DEV)
    p = torch.zeros(m, 2, dtype=torch.float64, device=DEV)
    ws = torch.empty(hip.adain_rows_workspace_bytes(m, C), dtype=torch.uint8, device=DEV)
    with pytest.raises(hip.VFaceHipError):       # workspace too small
        hip.adain_rows(a, a, p, ws[:16], rows=m, C_=C, lda=C, ldb=C)
    with pytest.raises(hip.VFaceHipError):       # more local rows than the gathered array holds
        hip.adain_reduce_scale(p[:4], ws, a, partial_rows=4, rows=m, C_=C, ldd=C)


# ------------------------------------------------------------------------------------------------ the whole UNet, shards as processes
def _inputs(total, h, w, f0, fc, dev):
    from vface_amd.utils import synth
    xs = [synth.synth_normal(f"coupled.x.{c}", (total, 9, h, w)) for c in range(3)]
    cs = [synth.synth_normal(f"coupled.c.{c}", (total, 1, 768)) for c in range(3)]
    return torch.cat([t[f0:f0 + fc] for t in xs]).to(dev), torch.cat([t[f0:f0 + fc] for t in cs]).to(dev)


def _sampler_inputs(total, h, w, f0, fc, dev):
    from oracle import ddim as oddim
    from vface_amd.utils import synth
    sl = lambda t: t[f0:f0 + fc].to(dev)
    x_T = sl(synth.synth_normal("coupled.xT", (total, 4, h, w)))
    c, uc, tc = (sl(synth.synth_normal(f"coupled.{k}", (total, 1, 768))) for k in ("c", "uc", "tc"))
    inp = sl(synth.synth_normal("coupled.inpaint", (total, 4, h, w)) * 0.18215)
    mask = sl(synth.synth_mask(total, h, w))
    inv = {int(s): sl(synth.synth_normal(f"coupled.inv.{int(s)}", (total, 4, h, w))) for s in oddim.ddim_timesteps(50)}
    return x_T, c, uc, tc, inp, mask, inv


def _forwards(rank, world, total, dist):
    """Every case of one shard: {(form, fusion): [eps eager, eps capturing call, eps replay], ...}, exchanges per forward and
    graph segments; {("sampler", fusion, drop): img after two DDIM steps}.  ``world == 1``: the unsharded reference."""
    from vface_amd import hip
    from vface_amd.engine import Act
    from vface_amd.ldm.models.diffusion.ddim_w_inv import DDIMSampler, HookPlan
    from vface_amd.ldm.models.diffusion.ddpm import LatentDiffusion
    from vface_amd.ldm.models.pnp_utils import register_spa_attn_injection as reg
    from vface_amd.parallel import FrameShard
    from vface_amd.utils import synth
    h = w = 32
    ldm = LatentDiffusion(_cfg())
    synth.fill_module_(ldm.unet, seed=0)
    ldm = ldm.to(DEV)
    sampler = DDIMSampler(ldm)
    eng = ldm.unet.engine
    f0, fc = frame_range(rank, world, total)
    x, ctx = _inputs(total, h, w, f0, fc, DEV)
    tt = torch.full((3 * fc,), 481, dtype=torch.long, device=DEV)
    N, C, H, W = x.shape
    cpad = (C + 7) // 8 * 8
    xin = torch.empty(N * H * W, cpad, dtype=eng.dtype, device=DEV)
    hip.nchw_to_nhwc(x.float().contiguous(), xin, N=N, C_=C, hw=H * W, cpad=cpad)
    res = {"f0": f0, "fc": fc}
    forms = ("p2p", "allgather") if world > 1 else ("p2p",)
    for form in forms:
        FrameShard(rank, world, total, dist if world > 1 else None, mode=form).install(eng)
        for fusion in ("temporal", "adaIn"):
            reg(sampler, 1, switch_on=False, input_blocks=True, middle_block=True, output_blocks=True)
            reg(sampler, 1, switch_on=True, input_blocks=True, middle_block=False, output_blocks=False, chunks=3,
                block_indices=list(range(9)), fusion=fusion, split_ratio_fft=0.8, alpha=0.8)
            eng._graphs, eng._graph_failed = {}, set()
            outs = []
            for graph in ((False, True, True) if world > 1 else (False,)):
                eng.use_graph = graph
                outs.append(eng.step_forward_nhwc(Act(xin, N, H, W), tt, ctx).clone().reshape(N, H * W, -1).cpu())
                if not graph:
                    res[("exchanges", form, fusion)] = eng._halo_k
            res[(form, fusion)] = outs
            res[("segments", form, fusion)] = [len(g["segments"]) for g in eng._graphs.values()]
            res[("graph_failed", form, fusion)] = len(eng._graph_failed)
    # two DDIM steps through the sampler: graph-replayed forwards, the uncond / cond prefix shared, with / without the dead branches
    FrameShard(rank, world, total, dist if world > 1 else None).install(eng)
    eng.use_graph, eng._graphs, eng._graph_failed = True, {}, set()
    x_T, c, uc, tc, inp, mask, inv = _sampler_inputs(total, h, w, f0, fc, DEV)
    sampler.flow_gate = "flow_hw"
    assert sampler.share_prefix
    for fusion in ("temporal", "adaIn"):
        sampler.hook_plan = HookPlan(fusion=fusion)
        for drop in (False, True):
            sampler.drop_dead_branches = drop
            img, _ = sampler.sample(S=50, batch_size=fc, shape=[4, h, w], conditioning=c, target_conditioning=tc,
                                    inverse_results_dir=inv, verbose=False, unconditional_guidance_scale=3.0,
                                    unconditional_conditioning=uc, eta=0.0, x_T=x_T, flow=None,
                                    test_model_kwargs={"inpaint_image": inp, "inpaint_mask": mask}, max_steps=2)
            res[("sampler", fusion, drop)] = img.clone().cpu()
    res[("sampler_graph_failed",)] = len(eng._graph_failed)
    eng.halo_exchange = None
    return res


def _shard_proc(rank, world, total, outdir):
    import torch.distributed as dist
    dist.init_process_group("gloo", init_method=f"file://{outdir}/rendezvous_{total}_{world}", rank=rank, world_size=world)
    try:
        res = _forwards(rank, world, total, dist)
        torch.save(res, os.path.join(outdir, f"t{total}_w{world}_r{rank}.pt"))
        dist.barrier()
    finally:
        dist.destroy_process_group()


_REF = {}


@pytest.mark.parametrize("total,world", [(5, 2), (5, 3), (4, 3)])
def test_coupled_shards_equal_unsharded(total, world, tmp_path):
    """5 frames over 2 ranks ([3, 2]: point-to-point), 5 over 3 ([2, 2, 1]) and 4 over 3 ([2, 1, 1]: rank 2's frame 3 needs frame 1,
    two ranks away) -- the one-frame layouts take the all-gather form also when point-to-point is asked for.  Each case: temporal
    and adaIn, both exchange forms, kernel by kernel, the capturing call and a pure replay of the graph segments (one exchange per
    hooked input-block layer: six, so 13 segments), and two DDIMSampler steps.  Concatenated shards == the unsharded run, bit for bit."""
    if total not in _REF:
        _REF[total] = _forwards(0, 1, total, None)
    ref = _REF[total]
    ctx = mp.get_context("spawn")
    procs = [ctx.Process(target=_shard_proc, args=(r, world, total, str(tmp_path))) for r in range(world)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(600)
    assert [p.exitcode for p in procs] == [0] * world
    res = [torch.load(os.path.join(str(tmp_path), f"t{total}_w{world}_r{r}.pt")) for r in range(world)]
    failures = []
    for d in res:
        f0, fc = d["f0"], d["fc"]
        for form in ("p2p", "allgather"):
            for fusion in ("temporal", "adaIn"):
                full = ref[("p2p", fusion)][0].reshape(3, total, -1)
                want = full[:, f0:f0 + fc].reshape(3 * fc, *ref[("p2p", fusion)][0].shape[1:])
                for what, got in zip(("eager", "capturing call", "replay"), d[(form, fusion)]):
                    if not torch.equal(got, want):
                        failures.append(f"{form} {fusion} {what} frames {f0}..{f0 + fc - 1}: max diff {(got - want).abs().max():.3e}")
                assert d[("exchanges", form, fusion)] == 6, d[("exchanges", form, fusion)]
                assert d[("segments", form, fusion)] == [13] and d[("graph_failed", form, fusion)] == 0, \
                    (form, fusion, d[("segments", form, fusion)])
        for fusion in ("temporal", "adaIn"):
            for drop in (False, True):
                got, want = d[("sampler", fusion, drop)], ref[("sampler", fusion, drop)][f0:f0 + fc]
                if not torch.equal(got, want):
                    failures.append(f"sampler {fusion} drop={drop} frames {f0}..{f0 + fc - 1}: max diff {(got - want).abs().max():.3e}")
        assert d[("sampler_graph_failed",)] == 0
    assert not failures, "; ".join(failures)
