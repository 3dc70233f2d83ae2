"""The exchanges of the frame-coupled hook modes on CPU with gloo (world sizes 2 and 4, uneven and one-frame shards): the temporal
halo (``FrameShard.start_temporal``: the two frames before and the two after every shard, a frame two ranks away included) and the
adaIn row-partial gather (``FrameShard.start_gather``: every rank's rows in global row order), in both exchange forms, and the
bounded wait of both when a peer never shows up."""
import os
import tempfile

import pytest
import torch
import torch.multiprocessing as mp

from vface_amd.parallel import FrameShard, frame_range

# (total frames per world size) -- shards as frame_range splits them
LAYOUTS = {2: (5, 4, 3, 2), 4: (9, 6, 5, 4)}      # world 2: [3,2] [2,2] [2,1] [1,1]; world 4: [3,2,2,2] [2,2,1,1] [2,1,1,1] [1,1,1,1]
N, C, P = 3, 8, 4                                 # tokens per frame, channels, partial arrays per gather


def _frames(total):
    """Global chunk-0 q|k stand-in: frame g holds g + (token, channel) / 1000, so every slot names its frame."""
    t = torch.arange(N * C, dtype=torch.float32).reshape(N, C) / 1000
    return torch.stack([g + t for g in range(total)]).to(torch.float16)


def _partials(total):
    """Global [P, total * N, 2] fp64 row partials: row r of array p = (r + 0.25 p, -r)."""
    r = torch.arange(total * N, dtype=torch.float64)
    return torch.stack([torch.stack([r + 0.25 * p, -r], -1) for p in range(P)])


def _worker(rank, world, store, q):
    import torch.distributed as dist
    dist.init_process_group("gloo", init_method=f"file://{store}", rank=rank, world_size=world)
    try:
        out = []
        for total in LAYOUTS[world]:
            X, part_g = _frames(total), _partials(total)
            for mode in ("p2p", "allgather"):
                sh = FrameShard(rank, world, total, dist, mode=mode)
                mine = X[sh.first:sh.first + sh.count]
                lo = min(sh.count, 2)
                edges = torch.full((4, N, C), float("nan"), dtype=X.dtype)
                edges[:lo] = mine[:lo]
                edges[4 - lo:] = mine[sh.count - lo:]
                halo = sh.finish_exchange(sh.start_temporal(edges))
                want = sh.halo_frames()
                got = [None if g is None else (float(halo[s, 0, 0]), bool(torch.equal(halo[s], X[g]))) for s, g in enumerate(want)]
                part = part_g[:, sh.first * N:(sh.first + sh.count) * N].contiguous()
                glob = sh.finish_exchange(sh.start_gather(part))
                out.append((total, mode, sh.temporal_form(), want, got, tuple(glob.shape), bool(torch.equal(glob, part_g))))
        q.put((rank, out))
    finally:
        dist.destroy_process_group()


def _spawn(target, world, *args, timeout=180):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    store = os.path.join(tempfile.mkdtemp(prefix="vface_rdzv_"), "store")
    procs = [ctx.Process(target=target, args=(r, world, store, q) + args) for r in range(world)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(timeout)
    return procs, q


@pytest.mark.parametrize("world", [2, 4])
def test_temporal_halo_and_adain_gather(world):
    """Every rank receives exactly the global frames its +-2 window needs, in order (first-2, first-1, last+1, last+2; none past
    the clip's ends), through point-to-point where every shard holds two frames and through the all-gather otherwise (a
    one-frame shard's neighbour two ranks away); the gathered row partials are every rank's rows in global row order."""
    procs, q = _spawn(_worker, world)
    assert [p.exitcode for p in procs] == [0] * world
    res = dict(q.get(timeout=5) for _ in range(world))
    for rank in range(world):
        for total, mode, form, want, got, gshape, gather_ok in res[rank]:
            first, count = frame_range(rank, world, total)
            last = first + count - 1
            assert want == [g if 0 <= g < total else None for g in (first - 2, first - 1, last + 1, last + 2)]
            assert form == ("p2p" if mode == "p2p" and total // world >= 2 else "allgather"), (total, mode, form)
            for s, g in enumerate(want):
                if g is not None:
                    assert got[s][1], f"world {world}, {total} frames, {mode}, rank {rank}: slot {s} holds frame {got[s][0]}, not {g}"
            assert gshape == (P, total * N, 2) and gather_ok, (world, total, mode, rank)
    if world == 4:      # 5 frames as [2, 1, 1, 1]: rank 2 (frame 3) needs frame 1, which lives on rank 0
        (t5,) = [r for r in res[2] if r[0] == 5 and r[1] == "p2p"]
        assert t5[3][0] == 1 and t5[4][0][1] and t5[2] == "allgather"


def _silent_peer_worker(rank, world, store, q, kind):
    """Rank 0 never takes part; rank 1's temporal halo / adaIn gather must give up within the bound and exit non-zero."""
    import time
    import torch.distributed as dist
    from vface_amd.parallel import ExchangeTimeout
    os.environ["VFACE_EXCHANGE_TIMEOUT_S"] = "2"
    dist.init_process_group("gloo", init_method=f"file://{store}", rank=rank, world_size=world)
    sh = FrameShard(rank, world, 4, dist)
    if rank == 0:
        time.sleep(6)            # alive, but never sends
        q.put((0, "slept", 0.0))
        q.close(); q.join_thread()
        os._exit(0)
    t0 = time.monotonic()
    try:
        if kind == "temporal":
            sh.finish_exchange(sh.start_temporal(torch.zeros(4, N, C)))
        else:
            sh.finish_exchange(sh.start_gather(torch.zeros(P, 2 * N, 2, dtype=torch.float64)))
    except ExchangeTimeout as e:
        q.put((1, str(e), time.monotonic() - t0))
        q.close(); q.join_thread()
        os._exit(3)
    q.put((1, "no timeout", 0.0))
    q.close(); q.join_thread()
    os._exit(0)


@pytest.mark.parametrize("kind", ["temporal", "gather"])
def test_silent_peer_times_out(kind):
    """``finish_exchange`` of both new exchanges is bounded (``VFACE_EXCHANGE_TIMEOUT_S``): a rank whose peer never takes part raises
    ``ExchangeTimeout`` naming who it waited for, and its process exits non-zero within the bound."""
    procs, q = _spawn(_silent_peer_worker, 2, kind, timeout=60)
    msgs = dict((m[0], m[1:]) for m in (q.get(timeout=5) for _ in range(2)))
    assert procs[1].exitcode == 3 and procs[0].exitcode == 0
    text, waited = msgs[1]
    assert "did not complete within 2 s" in text and waited < 10, text
    assert ("rank 0" in text) if kind == "temporal" else ("all 2 ranks" in text), text
