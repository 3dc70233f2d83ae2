"""``--whole_clip`` without a GPU: the batch plan, the carry's store (``parallel.ClipCarry``, on host tensors), the option checks and
the per-frame random draws."""
import numpy as np
import pytest
import torch
from PIL import Image

from test_clip_io_cpu import landmark_file, write_frames
from vface_amd.parallel import ClipCarry, clip_batches
from vface_amd.scripts import VFace_inference_batch as cli
from vface_amd.scripts import clip_io
from vface_amd.scripts.inputs import ClipRunInputs, SeededInputs, batch_plan
from vface_amd.scripts.pipeline import DRAWS, frame_noise


def options(*args):
    return cli.normalise_options(cli.build_parser().parse_args(list(args)))


# ------------------------------------------------------------------------------------------------ the batch plan
def test_batch_plan_exact_multiples_tails_and_short_clips():
    assert clip_batches(24, 6) == [(0, 6), (6, 6), (12, 6), (18, 6)]
    assert clip_batches(6, 6) == [(0, 6)]
    for n_samples in (2, 3, 6, 7):
        for tail in range(1, n_samples):                    # every tail length 1 .. n_samples - 1, the one-frame tail included
            plan = clip_batches(2 * n_samples + tail, n_samples)
            assert plan == [(0, n_samples), (n_samples, n_samples), (2 * n_samples, tail)]
    assert clip_batches(25, 6)[-1] == (24, 1)
    assert clip_batches(4, 6) == [(0, 4)] and clip_batches(1, 6) == [(0, 1)]        # n_frames < n_samples: one batch of n_frames
    assert clip_batches(5, 1) == [(f, 1) for f in range(5)]
    assert clip_batches(0, 6) == []
    for n_frames in range(0, 30):                           # every frame in exactly one batch, in order, none longer than n_samples
        for n_samples in range(1, 9):
            plan = clip_batches(n_frames, n_samples)
            assert [f for first, count in plan for f in range(first, first + count)] == list(range(n_frames))
            assert all(1 <= count <= n_samples for _, count in plan)
    for bad in ((5, 0), (-1, 2)):
        with pytest.raises(ValueError):
            clip_batches(*bad)


def test_the_run_plan_drops_the_tail_without_the_flag_and_keeps_it_with():
    assert batch_plan(options("--synthetic", "--n_frames", "25", "--n_samples", "6")) == [(0, 6), (6, 6), (12, 6), (18, 6)]
    assert batch_plan(options("--synthetic", "--n_frames", "25", "--n_samples", "6", "--whole_clip")) == clip_batches(25, 6)
    assert batch_plan(options("--synthetic", "--n_frames", "4", "--n_samples", "6")) == []


# ------------------------------------------------------------------------------------------------ the carry's store
def slab(v):
    return torch.full((4, 6), float(v), dtype=torch.float16)


def forward(carry, step, values):
    """One UNet forward as the engine and the sampler drive the exchange: the step stated once, then per hooked layer the ordinal,
    the start and the finish.  Returns what each finish handed back."""
    carry.set_step(step)
    got = []
    for k, v in enumerate(values):
        carry.set_index(k)
        got.append(carry.finish_exchange(carry.start_exchange(slab(v))))
    return got


def test_carry_is_keyed_by_step_and_ordinal_and_a_repeated_start_overwrites():
    carry = ClipCarry(clip_batches(5, 2))
    assert (carry.world, carry.total, carry.rank, carry.first, carry.count) == (3, 5, 0, 0, 2)
    assert forward(carry, 0, [10, 11]) == [None, None]                  # batch 0 reads nothing
    assert forward(carry, 0, [20, 21]) == [None, None]                  # the capturing call's second and third forward of step 0 ..
    assert forward(carry, 0, [30, 31]) == [None, None]
    assert forward(carry, 1, [40, 41]) == [None, None]
    assert sorted(carry.generations[0]) == [(0, 0), (0, 1), (1, 0), (1, 1)]          # .. overwrote, never appended
    assert carry.carry_bytes() == 4 * 4 * 6 * 2
    carry.begin_batch(1)
    assert (carry.rank, carry.first, carry.count) == (1, 2, 2)
    # read in another order than written: the key decides, not the call count
    got = forward(carry, 1, [50, 51])
    assert [float(g[0, 0]) for g in got] == [40.0, 41.0]
    got = forward(carry, 0, [60, 61])
    assert [float(g[0, 0]) for g in got] == [30.0, 31.0]
    assert float(carry.generations[0][(0, 0)][0, 0]) == 30.0            # what batch 1 wrote went to ITS generation, not the one it reads
    assert float(carry.generations[1][(0, 0)][0, 0]) == 60.0


def test_carry_reading_what_the_previous_batch_never_wrote_names_step_and_ordinal():
    carry = ClipCarry(clip_batches(4, 2))
    forward(carry, 0, [1, 2])
    forward(carry, 1, [3, 4])                                           # batch 0 ran two steps
    carry.begin_batch(1)
    forward(carry, 0, [5, 6])
    forward(carry, 1, [7, 8])
    with pytest.raises(KeyError) as e:
        forward(carry, 2, [9, 10])                                      # batch 1 runs a third
    assert "DDIM step 2" in str(e.value) and "ordinal 0" in str(e.value) and "batch 0 never wrote" in str(e.value)
    carry.set_step(1)
    carry.set_index(2)                                                  # a third hooked layer the previous batch did not have
    with pytest.raises(KeyError) as e:
        carry.finish_exchange(carry.start_exchange(slab(0)))
    assert "DDIM step 1" in str(e.value) and "ordinal 2" in str(e.value)
    fresh = ClipCarry(clip_batches(4, 2))
    fresh.set_index(0)
    with pytest.raises(RuntimeError, match="state the DDIM step"):
        fresh.start_exchange(slab(0))


def test_carry_keeps_two_generations_and_the_last_batch_keeps_nothing():
    carry = ClipCarry(clip_batches(7, 2))                               # (2, 2, 2, 1)
    for k in range(4):
        carry.begin_batch(k)
        got = forward(carry, 0, [100 * k, 100 * k + 1])
        assert sorted(carry.generations) == ([0] if k == 0 else [k - 1, k])
        assert got == [None, None] if k == 0 else [float(g[0, 0]) for g in got] == [100.0 * (k - 1), 100.0 * (k - 1) + 1]
        assert carry.carry_bytes() == (0 if k == 3 else 2 * 4 * 6 * 2)
    assert carry.generations[3] == {}
    ids = {id(s) for s in carry.generations[2].values()}
    carry.begin_batch(0)                                                # the clip again: only the generation being written is left
    assert sorted(carry.generations) == [0] and carry.generations[0] == {}
    forward(carry, 0, [1, 2])
    assert {id(s) for s in carry.generations[0].values()} == ids        # (a dropped generation's slabs are the new one's buffers)
    with pytest.raises(IndexError):
        carry.begin_batch(4)


def test_carry_is_immune_to_a_capture_pass_and_lets_go_after_the_last_batch():
    """What a hipGraph capture does to an exchange (replay._capture): a warm-up forward with real slabs, then the capture pass, whose
    kernels are recorded and not run -- the slabs it hands over hold no data.  If the capture is then dropped (it failed, or its pool is
    over budget) there is no first replay to overwrite them, and ``drain`` re-starts the warm-up's remaining tails without stating an
    ordinal.  The store must hold the warm-up's slabs after all of that."""
    carry = ClipCarry(clip_batches(4, 2))
    forward(carry, 0, [1, 2])                                           # the warm-up forward
    carry.capture_pass(True)
    assert forward(carry, 0, [float("nan"), float("nan")]) == [None, None]      # the capture pass: calls made, nothing kept
    carry.drain(None, [slab(float("nan"))])                             # an aborted pass: ordinal 1's tail, index left at whatever it was
    carry.capture_pass(False)
    assert [float(carry.generations[0][(0, k)][0, 0]) for k in range(2)] == [1.0, 2.0]
    forward(carry, 0, [3, 4])                                           # a first replay, where there is one, stores again
    assert [float(carry.generations[0][(0, k)][0, 0]) for k in range(2)] == [3.0, 4.0]
    carry.end_batch()
    assert sorted(carry.generations) == [0]                             # not the last batch: kept for the next one
    carry.begin_batch(1)
    assert [float(g[0, 0]) for g in forward(carry, 0, [5, 6])] == [3.0, 4.0]
    carry.end_batch()
    assert 0 not in carry.generations and carry.carry_bytes() == 0      # the last batch's loop is over: what it read is let go


def test_frame_shard_states_its_own_graph_signature():
    from vface_amd.parallel import FrameShard, LoopbackShard
    sh = FrameShard(0, 1, 5)
    assert sh.graph_signature() == (id(sh), 0, 1, 0, 5) and sh.capture_pass(True) is None
    a, b = LoopbackShard(0, 2, 5, {}), LoopbackShard(1, 2, 5, {})
    assert a.graph_signature()[1:] == (0, 2, 0, 3) and b.graph_signature()[1:] == (1, 2, 3, 2)


def test_carry_of_one_batch_exchanges_nothing_and_the_coupled_modes_raise():
    one = ClipCarry(clip_batches(4, 6))
    one.set_step(0)
    assert one.world == 1 and one.start_exchange(slab(1)) is None and one.finish_exchange(None) is None
    carry = ClipCarry(clip_batches(4, 2))
    with pytest.raises(NotImplementedError, match="NEXT batch"):
        carry.start_temporal(slab(0))
    with pytest.raises(NotImplementedError, match="every frame of the clip"):
        carry.start_gather(slab(0))
    assert carry.agree(True, False) == (True, False)
    # what a captured forward depends on: reading a slab or not, and the frames -- not which batch
    carry.begin_batch(1)
    sig = carry.graph_signature()
    carry.begin_batch(0)
    assert carry.graph_signature() != sig
    three = ClipCarry(clip_batches(6, 2))
    three.begin_batch(1)
    sig = three.graph_signature()
    three.begin_batch(2)
    assert three.graph_signature() == sig

    class Engine:
        halo_exchange = halo_flow = halo_hw = None
    eng = Engine()
    with pytest.raises(ValueError, match="needs the flow field"):
        three.install(eng, None, (8, 8))
    three.install(eng, torch.zeros(1, 2, 8, 8), (8, 8))
    assert eng.halo_exchange is three and tuple(eng.halo_flow.shape) == (2, 8, 8) and eng.halo_hw == (8, 8)
    three.uninstall(eng)
    assert eng.halo_exchange is None and eng.halo_flow is None and eng.halo_hw is None
    one.install(eng, None, (8, 8))
    assert eng.halo_exchange is None


# ------------------------------------------------------------------------------------------------ the options
@pytest.mark.parametrize("args, message", [
    (("--fusion", "temporal"), "--fusion temporal needs the NEXT batch's first two frames"),
    (("--fusion", "adaIn"), "--fusion adaIn needs a standard deviation over every frame of the clip"),
    (("--pipeline_inversion",), "--whole_clip and --pipeline_inversion together are not built"),
    (("--ddim_eta", "0.5"), "--whole_clip needs --ddim_eta 0"),
])
def test_check_options_refuses_what_would_depend_on_n_samples(args, message):
    with pytest.raises(SystemExit) as e:
        cli.check_options(options("--synthetic", "--whole_clip", *args))
    assert message in str(e.value)
    cli.check_options(options("--synthetic", *args))                    # without the flag the same options pass, as they did


def test_whole_clip_is_off_by_default_and_passes_with_the_uncoupled_modes():
    assert options("--synthetic").whole_clip is False
    assert cli.normalise_options(__import__("argparse").Namespace()).whole_clip is False
    for fusion in ("flow_fix", "none", "fft", "replace", "mix"):
        cli.check_options(options("--synthetic", "--whole_clip", "--fusion", fusion, "--drop_dead_branches"))
    opt = options("--target_frames", "d", "--src_image", "s.png", "--landmarks", "l.npz", "--synthetic_weights", "--whole_clip")
    cli.check_options(opt)
    assert all(getattr(opt, name) for name in cli.CLIP_STAGES)


# ------------------------------------------------------------------------------------------------ draws and inputs per frame
def test_a_frames_draw_is_the_same_in_every_batch_and_position():
    shape = (4, 8, 8)
    clip = frame_noise(42, range(7), "inpaint", shape)
    assert tuple(clip.shape) == (7, 4, 8, 8) and clip.dtype == torch.float32
    for n_samples in (1, 2, 3, 7):
        for first, count in clip_batches(7, n_samples):
            assert torch.equal(frame_noise(42, range(first, first + count), "inpaint", shape), clip[first:first + count])
    assert torch.equal(frame_noise(42, [5, 2], "inpaint", shape), clip[[5, 2]])
    # frame, draw and seed each change it; the global generator is neither read nor moved
    draws = [frame_noise(42, [3], d, shape) for d in DRAWS] + [frame_noise(43, [3], "inpaint", shape), frame_noise(42, [4], "inpaint", shape)]
    for i in range(len(draws)):
        for j in range(i):
            assert not torch.equal(draws[i], draws[j]), (i, j)
    torch.manual_seed(0)
    a = torch.randn(3)
    torch.manual_seed(0)
    frame_noise(42, range(3), "z2_tar", shape)
    assert torch.equal(torch.randn(3), a)
    assert abs(float(clip.mean())) < 0.1 and abs(float(clip.std()) - 1.0) < 0.1


def test_seeded_provider_feeds_a_frame_the_same_whatever_batch_holds_it():
    """7 frames of 64 x 64 (8 x 8 latents): every per-frame stand-in, cut as (2, 2, 2, 1) and (3, 3, 1), equals the one-batch cut."""
    base = ("--synthetic", "--whole_clip", "--n_frames", "7", "--H", "64", "--W", "64", "--frame_size", "96", "--ddim_steps", "4")
    whole = SeededInputs(options(*base, "--n_samples", "7"), "cpu")
    asks = {"tokens": lambda p, k: torch.cat(p.tokens(k), 1), "images": lambda p, k: p.images(k), "latents": lambda p, k: p.latents(k),
            "latent_mask": lambda p, k: p.latent_mask(k), "keep_mask": lambda p, k: p.keep_mask(k),
            "id_feats": lambda p, k: torch.cat(p.id_feats(k), 1), "landmarks": lambda p, k: p.landmarks(k),
            "frames": lambda p, k: p.intake_frames(k)[0], "labels": lambda p, k: p.intake_frames(k)[3],
            "quads": lambda p, k: torch.from_numpy(p.intake_frames(k)[2]), "paste_frames": lambda p, k: p.paste_target(k, 1024)[0],
            "paste_coeffs": lambda p, k: torch.from_numpy(np.stack(p.paste_target(k, 1024)[1])),
            "inversion_cache": lambda p, k: torch.cat(list(p.inversion_cache(k, torch.tensor([1, 251])).values()), 1),
            "z2_tar": lambda p, k: p.inversion_latents(k)[:p.count(k)], "z2_src": lambda p, k: p.inversion_latents(k)[p.count(k):]}
    want = {name: ask(whole, 0) for name, ask in asks.items()}
    clip_flow = whole.flow(0)
    assert len(clip_flow) == 6 and whole.boundary_flow(0) is None and whole.inherits(0) == [False] * 7
    for n_samples in (2, 3):
        p = SeededInputs(options(*base, "--n_samples", str(n_samples)), "cpu")
        for k, (first, count) in enumerate(clip_batches(7, n_samples)):
            for name, ask in asks.items():
                got = ask(p, k)
                assert got.shape[0] == count and torch.equal(got, want[name][first:first + count]), (name, n_samples, k)
            own = p.flow(k)
            assert len(own) == count - 1 and all(torch.equal(a, b) for a, b in zip(own, clip_flow[first:first + count - 1]))
            assert (p.boundary_flow(k) is None) if k == 0 else torch.equal(p.boundary_flow(k), clip_flow[first - 1])
            assert p.inherits(k) == [False] * count
        assert p._fields(0) is p._fields(1) and p.boundary_flow(1) is p._fields(1)[n_samples - 1]     # the clip's fields: made once per provider
    px = SeededInputs(options(*base, "--n_samples", "3", "--flow_pixels"), "cpu")
    assert tuple(px.boundary_flow(1).shape) == (1, 2, 64, 64) and tuple(px.flow(1)[0].shape) == (1, 2, 64, 64)


def test_clip_provider_walks_every_frame_with_a_shorter_last_batch(tmp_path):
    """5 frames in batches of 2: (2, 2, 1).  Frame 4 -- the one-frame tail -- has no landmarks: it takes the crop of frame 3, read
    again from the batch before, and that batch's last label map."""
    frames = write_frames(tmp_path / "f", 5, size=(320, 240))
    Image.fromarray(frames[0, :100, :90]).save(tmp_path / "src.png")
    _, arrays = landmark_file(str(tmp_path / "lm.npz"), n=5, nan=(4,))
    clip = clip_io.ClipInputs(str(tmp_path / "f"), str(tmp_path / "src.png"), str(tmp_path / "lm.npz"), 5, 512, 512)
    opt = options("--target_frames", str(tmp_path / "f"), "--n_samples", "2", "--n_frames", "5", "--whole_clip")
    p = ClipRunInputs(clip, opt, "cpu")
    assert [p.frame_ids(k) for k in range(3)] == [[0, 1], [2, 3], [4]]
    assert p.inherits(2) == [True]
    maps = lambda k, n: torch.stack([torch.full((8, 8), 10 * k + f, dtype=torch.uint8) for f in range(n)])
    p.carry_labels(0, maps(0, 2))
    p.carry_labels(1, maps(1, 2))
    assert torch.equal(p.carry_labels(2, maps(2, 1))[0], maps(1, 2)[1])
    paste_into, crop_from, quads, labels = p.intake_frames(2)
    assert np.array_equal(paste_into.numpy(), frames[4:5]) and np.array_equal(crop_from.numpy(), frames[3:4]) and labels is None
    assert np.array_equal(quads, clip.quads[4:5]) and tuple(p.landmarks(2).shape) == (1, 136) and not p.landmarks(2).any()
    # the reader itself: the plan's rows with the flag, the reference's without
    assert clip.batch(2, 2, whole_clip=True)["frame_ids"] == [4] and clip.batch(1, 2)["frame_ids"] == [2, 3]
    assert clip.batch(0, 5, whole_clip=True)["frame_ids"] == [0, 1, 2, 3, 4]
    plain = ClipRunInputs(clip, options("--target_frames", str(tmp_path / "f"), "--n_samples", "2", "--n_frames", "5"), "cpu")
    assert plain.plan == [(0, 2), (2, 2)] and plain.frame_ids(1) == [2, 3]
