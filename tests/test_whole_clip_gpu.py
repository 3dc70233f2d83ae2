"""Whole clips on the MI355X box: a clip sampled in batches, ``flow_fix`` coupled across the batch boundaries by
``parallel.ClipCarry``, equals the clip sampled as ONE batch bit for bit.

* Sampler level: ``DDIMSampler.sample`` on 5 frames as one batch, and as batches (2, 2, 1) and (3, 2) with the carry and the boundary
  flow field -- kernel by kernel and from segmented hipGraph replay (three steps: the third is a pure replay), the uncond / cond
  prefix shared or not, three live chunks or two (dead-branch elimination), fp16 and one bf16 case.  ``torch.equal``.  The one
  reference per dtype is the plainest form: one batch, kernel by kernel, nothing shared, nothing dropped.
* A capture that falls back (injected failures, a byte budget nothing fits) leaves the carry exact: its capture pass stores nothing.
* Negative control: the same batches without the carry leave batch 0 equal and frame 0 of batch 1 different.
* ``run_synthetic --whole_clip`` on the tiny UNet: the seeded provider's per-clip stand-ins, coupled (``flow_fix``) and not (``fft``).
* Command line: ``run_clip --whole_clip`` on 5 frames of 320 x 240 gives the same pasted frames at ``--n_samples 2`` (three
  batches, the last of one frame) and ``--n_samples 5`` (one batch); without the flag ``--n_samples 2`` drops the fifth frame."""
import os

import numpy as np
import pytest
import torch
from PIL import Image

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
TOTAL, H, W, STEPS = 5, 32, 32, 3


def _cfg():
    """The tiny UNet of tests/test_sharded_gpu.py."""
    return dict(image_size=32, in_channels=9, out_channels=4, model_channels=64, attention_resolutions=[4, 2, 1],
                num_res_blocks=2, channel_mult=[1, 2, 4, 4], num_heads=8, use_spatial_transformer=True,
                transformer_depth=1, context_dim=768, legacy=False)


_MODELS, _REF = {}, {}


def _sampler(dt):
    """One model and sampler per compute dtype for the whole module."""
    if dt not in _MODELS:
        from vface_amd.ldm.models.diffusion.ddim_w_inv import DDIMSampler
        from vface_amd.ldm.models.diffusion.ddpm import LatentDiffusion
        from vface_amd.utils import synth
        ldm = LatentDiffusion(dict(_cfg(), compute_dtype=dt))
        synth.fill_module_(ldm.unet, seed=0)
        sampler = DDIMSampler(ldm.to(DEV))
        sampler.flow_gate = "flow_hw"
        _MODELS[dt] = sampler
    return _MODELS[dt]


def _clip():
    """The clip's sampler inputs, per global frame (host), and its F - 1 synthetic flow fields."""
    from oracle import ddim as oddim
    from vface_amd.utils import synth
    d = {"x_T": synth.synth_normal("whole.xT", (TOTAL, 4, H, W)),
         "inp": synth.synth_normal("whole.inpaint", (TOTAL, 4, H, W)) * 0.18215, "mask": synth.synth_mask(TOTAL, H, W),
         "inv": {int(s): synth.synth_normal(f"whole.inv.{int(s)}", (TOTAL, 4, H, W)) for s in oddim.ddim_timesteps(50)},
         "flow": synth.synth_flow(TOTAL - 1, H, W)}
    for k in ("c", "uc", "tc"):
        d[k] = synth.synth_normal(f"whole.{k}", (TOTAL, 1, 768))
    return d


def _sample(sampler, clip, first, count, carry=None):
    """``DDIMSampler.sample`` on frames [first, first + count) of the clip: its own fields, and with ``carry`` the boundary field."""
    sl = lambda t: t[first:first + count].to(DEV)
    flow = [f[None] for f in clip["flow"][first:first + count - 1]]
    kw = {}
    if carry is not None:
        kw = {"carry": carry, "boundary_flow": clip["flow"][first - 1] if first else None}
    img, _ = sampler.sample(S=50, batch_size=count, shape=[4, H, W], conditioning=sl(clip["c"]), target_conditioning=sl(clip["tc"]),
                            inverse_results_dir={s: sl(v) for s, v in clip["inv"].items()}, verbose=False,
                            unconditional_guidance_scale=3.0, unconditional_conditioning=sl(clip["uc"]), eta=0.0, x_T=sl(clip["x_T"]),
                            flow=flow, test_model_kwargs={"inpaint_image": sl(clip["inp"]), "inpaint_mask": sl(clip["mask"])},
                            max_steps=STEPS, **kw)
    return img.clone()


def _configure(sampler, graph, share, drop):
    eng = sampler.model.model.diffusion_model.engine
    eng.use_graph, eng._graphs, eng._graph_failed = graph, {}, set()
    sampler.share_prefix, sampler.drop_dead_branches = share, drop
    return eng


def _reference(dt):
    """The clip as ONE batch of 5 frames: kernel by kernel, every chunk on its own, all three chunks."""
    if dt not in _REF:
        sampler = _sampler(dt)
        _configure(sampler, False, False, False)
        _REF[dt] = (_clip(), _sample(sampler, _clip(), 0, TOTAL))
    return _REF[dt]


@pytest.fixture(autouse=True)
def _restore():
    saved = {dt: (s.model.model.diffusion_model.engine.use_graph, s.share_prefix, s.drop_dead_branches) for dt, s in _MODELS.items()}
    yield
    for dt, s in _MODELS.items():
        eng = s.model.model.diffusion_model.engine
        eng._graphs, eng._graph_failed = {}, set()
        assert eng.halo_exchange is None and eng.halo_flow is None and eng.halo_hw is None     # the sampler took the carry off again
        if dt in saved:
            eng.use_graph, s.share_prefix, s.drop_dead_branches = saved[dt]


CASES = [(torch.float16, graph, share, drop) for graph in (False, True) for share in (True, False) for drop in (False, True)]
CASES.append((torch.bfloat16, True, True, False))


@pytest.mark.parametrize("dt,graph,share,drop", CASES)
def test_batches_with_the_carry_equal_one_batch_bit_for_bit(dt, graph, share, drop):
    from vface_amd.parallel import ClipCarry, clip_batches
    clip, whole = _reference(dt)
    sampler = _sampler(dt)
    eng = _configure(sampler, graph, share, drop)
    for n_samples, counts in ((2, [2, 2, 1]), (3, [3, 2])):
        plan = clip_batches(TOTAL, n_samples)
        assert [c for _, c in plan] == counts
        eng._graphs = {}
        carry = ClipCarry(plan)
        for k, (first, count) in enumerate(plan):
            carry.begin_batch(k)
            got = _sample(sampler, clip, first, count, carry)
            want = whole[first:first + count]
            assert torch.equal(got, want), (f"n_samples {n_samples} batch {k} (frames {first}..{first + count - 1}): per-frame max diff "
                                            f"{(got - want).abs().flatten(1).amax(1).tolist()}")
            assert eng.halo_exchange is None
            # what this batch hands on: one [n, 2d] 16-bit slab per step and hooked level-0 layer; the last batch keeps nothing
            assert carry.carry_bytes() == (0 if k + 1 == len(plan) else STEPS * 2 * H * W * 2 * 64 * 2)
            assert len(carry.generations) <= 2
        assert not eng._graph_failed, "capture fell back to kernel-by-kernel launches"
        if graph:
            # one capture per (reads a slab or not, frames): five segments each, cut at the two exchanges' start and finish
            assert sorted(len(g["segments"]) for g in eng._graphs.values()) == [5] * len(set((k > 0, c) for k, (_, c) in enumerate(plan)))
        else:
            assert not eng._graphs


def test_batches_of_one_shape_replay_one_capture():
    """``--n_samples 1``: five one-frame batches, none with a field of its own.  Batch 0 (reads no slab) captures once, batches 1..4
    replay ONE capture between them, and the clip still equals the one-batch run."""
    from vface_amd.parallel import ClipCarry, clip_batches
    clip, whole = _reference(torch.float16)
    sampler = _sampler(torch.float16)
    eng = _configure(sampler, True, True, False)
    plan = clip_batches(TOTAL, 1)
    carry = ClipCarry(plan)
    for k, (first, count) in enumerate(plan):
        carry.begin_batch(k)
        assert torch.equal(_sample(sampler, clip, first, count, carry), whole[first:first + count]), k
    assert not eng._graph_failed and len(eng._graphs) == 2


@pytest.mark.parametrize("how", ["mid_batch0", "mid_batch1", "warmup_done_batch0", "over_budget"])
def test_a_capture_that_falls_back_leaves_the_carry_exact(how, monkeypatch):
    """A capture that is dropped returns the warm-up forward's eps and runs no further forward, so nothing overwrites what the
    capture pass did to the carry -- a pass whose kernels are recorded, not run, and whose slabs therefore hold no data.  Capture
    failures injected while one batch samples (``VFACE_TEST_FAIL_CAPTURE``: after the warm-up, or with one exchange started and not
    finished) and a byte budget no capture fits: that batch and the batches behind it still equal the one-batch run bit for bit."""
    import warnings
    from vface_amd.parallel import ClipCarry, clip_batches
    clip, whole = _reference(torch.float16)
    sampler = _sampler(torch.float16)
    eng = _configure(sampler, True, True, False)
    budget = eng.graph_budget_bytes
    plan = clip_batches(TOTAL, 2)
    carry = ClipCarry(plan)
    try:
        if how == "over_budget":
            eng.graph_budget_bytes = 1
        for k, (first, count) in enumerate(plan):
            carry.begin_batch(k)
            if how.endswith(f"batch{k}"):
                monkeypatch.setenv("VFACE_TEST_FAIL_CAPTURE", how.rsplit("_", 1)[0])
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                got = _sample(sampler, clip, first, count, carry)
            monkeypatch.delenv("VFACE_TEST_FAIL_CAPTURE", raising=False)
            want = whole[first:first + count]
            assert torch.equal(got, want), f"{how} batch {k}: per-frame max diff {(got - want).abs().flatten(1).amax(1).tolist()}"
        # the fallback really happened: every form under the budget case, the one batch's form otherwise
        assert (len(eng._graph_failed), len(eng._graphs)) == ((3, 0) if how == "over_budget" else (1, 2))
    finally:
        eng.graph_budget_bytes = budget


def test_without_the_carry_the_seam_shows():
    """The negative control: the same batches, nothing carried.  Batch 0 reads no frame before it and equals the one-batch run;
    frame 0 of batch 1 misses its predecessor and does not."""
    clip, whole = _reference(torch.float16)
    sampler = _sampler(torch.float16)
    _configure(sampler, False, True, False)
    assert torch.equal(_sample(sampler, clip, 0, 2), whole[0:2])
    got = _sample(sampler, clip, 2, 2)
    assert not torch.equal(got[0], whole[2])


def test_a_batch_after_the_first_needs_its_boundary_field():
    from vface_amd.parallel import ClipCarry, clip_batches
    clip, _ = _reference(torch.float16)
    sampler = _sampler(torch.float16)
    _configure(sampler, False, True, False)
    carry = ClipCarry(clip_batches(TOTAL, 2))
    carry.begin_batch(1)
    with pytest.raises(ValueError, match="needs boundary_flow"):
        _sample(sampler, clip, 0, 2, carry)     # (`_sample` hands over no boundary field for first == 0; the carry is at batch 1)


# ------------------------------------------------------------------------------------------------ the command line
N, FW, FH = 5, 320, 240


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """The clip of tests/test_clip_run_gpu.py with a fifth frame -- the one without landmarks, so the one-frame tail takes its crop
    and label map across a batch boundary -- and three runs of it, two DDIM steps each."""
    import yaml
    from test_clip_io_cpu import square, template_landmarks
    from test_clip_run_gpu import small_cfg
    from vface_amd.scripts import VFace_inference_batch as cli
    root = tmp_path_factory.mktemp("whole_clip")
    rng = np.random.default_rng(11)
    frames = rng.integers(0, 256, (N, FH, FW, 3), dtype=np.uint8)
    (root / "frames").mkdir()
    for i in range(N):
        Image.fromarray(frames[i]).save(root / "frames" / f"{i}.png")
    Image.fromarray(rng.integers(0, 256, (180, 200, 3), dtype=np.uint8)).save(root / "src.png")
    lm = np.stack([template_landmarks(square(160 + 4 * i, 120 - 3 * i, 60 + 2 * i, 0.06 * i)) for i in range(N)])
    lm[4] = np.nan
    np.savez(root / "lm.npz", frames=lm, source=template_landmarks(square(100, 90, 50, -0.1)),
             crops=rng.integers(100, 412, (N, 68, 2)).astype(np.float64), source_crop=rng.integers(100, 412, (68, 2)).astype(np.float64))
    (root / "small.yaml").write_text(yaml.safe_dump({"model": {"params": {"unet_config": {"params": small_cfg()}}}}))

    def run(tag, n_samples, more=()):
        args = ["--target_frames", str(root / "frames"), "--src_image", str(root / "src.png"), "--landmarks", str(root / "lm.npz"),
                "--video_out", str(root / f"{tag}.y4m"), "--synthetic_weights", "--config", str(root / "small.yaml"),
                "--H", "512", "--W", "512", "--max_steps", "2", "--ddim_steps", "50", "--n_frames", str(N), "--n_samples", str(n_samples),
                "--Base_dir", str(root / tag), *more]
        opt = cli.build_parser().parse_args(args)
        opt.return_samples = True
        torch.manual_seed(opt.seed)
        return cli.run_clip(opt)["batches"]

    return {"root": root, "whole2": run("w2", 2, ["--whole_clip"]), "whole5": run("w5", 5, ["--whole_clip"]), "plain2": run("p2", 2)}


def cat(batches, key):
    return torch.cat([b[key] for b in batches])


def test_whole_clip_writes_every_frame_and_the_same_frames_for_every_n_samples(runs):
    a, b = runs["whole2"], runs["whole5"]
    assert [x["frames"] for x in a] == [2, 2, 1] and [x["frame_ids"] for x in a] == [[0, 1], [2, 3], [4]]
    assert [x["frames"] for x in b] == [5] and b[0]["frame_ids"] == [0, 1, 2, 3, 4]
    assert [x["coupled"] for x in a] == [False, True, True] and [x["coupled"] for x in b] == [False]
    assert a[0]["carry_bytes"] == a[1]["carry_bytes"] > 0 and a[2]["carry_bytes"] == 0 and b[0]["carry_bytes"] == 0
    assert ["boundary_flow" in x["stage_seconds"] for x in a] == [False, True, True] and "boundary_flow" not in b[0]["stage_seconds"]
    assert a[2]["pasted"] == [1, FH, FW, 3] and a[2]["pixels"] == [1, 3, 512, 512] and all(x["finite"] for x in a + b)
    # in the order of the stages, so that a difference names the first stage that makes it
    for key in ("crops", "labels", "conditioning", "samples", "pasted_frames"):
        got, want = cat(a, key), cat(b, key)
        differ = [f for f in range(N) if not torch.equal(got[f], want[f])]
        assert not differ, f"{key}: frames {differ} differ between --n_samples 2 and --n_samples 5"
    assert tuple(cat(a, "pasted_frames").shape) == (N, FH, FW, 3)


@pytest.mark.parametrize("tag", ["w2", "w5"])
def test_whole_clip_outputs_on_disk_are_the_pasted_frames(runs, tag):
    import mux_model as mm
    from vface_amd import hip
    pasted = cat(runs["whole2" if tag == "w2" else "whole5"], "pasted_frames")
    results = runs["root"] / tag / "results"
    assert sorted(os.listdir(results), key=lambda s: int(s.split(".")[0])) == [f"{i}.png" for i in range(N)]
    for i in range(N):
        assert np.array_equal(np.array(Image.open(results / f"{i}.png")), pasted[i].cpu().numpy()), i
    tags, payload = mm.read_y4m(str(runs["root"] / f"{tag}.y4m"))
    assert (tags["W"], tags["H"]) == (str(FW), str(FH)) and payload.shape == (N, mm.frame_bytes(FW, FH))
    assert np.array_equal(payload, hip.rgb_to_yuv420(pasted).cpu().numpy())


def test_without_the_flag_the_tail_frame_is_dropped_as_before(runs):
    p = runs["plain2"]
    assert [x["frame_ids"] for x in p] == [[0, 1], [2, 3]] and [x["frames"] for x in p] == [2, 2]
    assert all("coupled" not in x and "carry_bytes" not in x and "boundary_flow" not in x["stage_seconds"] for x in p)
    assert tuple(cat(p, "pasted_frames").shape) == (4, FH, FW, 3)
    assert sorted(os.listdir(runs["root"] / "p2" / "results"), key=lambda s: int(s.split(".")[0])) == [f"{i}.png" for i in range(4)]


@pytest.mark.parametrize("fusion", ["flow_fix", "fft"])
def test_seeded_whole_clip_run_is_the_same_for_every_n_samples(fusion, tmp_path):
    """``run_synthetic --whole_clip`` on the tiny UNet (256 x 256: 32 x 32 latents), 5 frames, two steps: the seeded provider's
    per-clip stand-ins and its boundary field.  ``flow_fix`` is coupled; ``fft`` couples no frames, takes the flag for the plan and
    the draws only, and its run does not enter the flow stage at all."""
    import yaml
    from vface_amd.scripts import VFace_inference_batch as cli
    (tmp_path / "tiny.yaml").write_text(yaml.safe_dump({"model": {"params": {"unet_config": {"params": _cfg()}}}}))

    def run(n_samples):
        opt = cli.build_parser().parse_args(["--synthetic", "--whole_clip", "--config", str(tmp_path / "tiny.yaml"), "--H", "256", "--W", "256",
                                             "--fusion", fusion, "--flow_gate", "flow_hw", "--no_inversion", "--max_steps", "2", "--n_frames", "5",
                                             "--n_samples", str(n_samples), "--skip_save", "--Base_dir", str(tmp_path / "out")])
        opt.return_samples = True
        torch.manual_seed(opt.seed)
        return cli.run_synthetic(opt)["batches"]

    a, b = run(2), run(5)
    assert [x["frames"] for x in a] == [2, 2, 1] and [x["frames"] for x in b] == [5]
    assert [x["coupled"] for x in a] == ([False, True, True] if fusion == "flow_fix" else [False] * 3)
    assert ["boundary_flow" in x["stage_seconds"] for x in a] == ([False, True, True] if fusion == "flow_fix" else [False] * 3)
    got, want = torch.cat([x["samples"] for x in a]), b[0]["samples"]
    differ = [f for f in range(5) if not torch.equal(got[f], want[f])]
    assert not differ, f"frames {differ} differ between --n_samples 2 and --n_samples 5"
