"""The boundary-exchange protocol (``parallel.Exchange``) without a GPU: who implements it, the one-neighbour rule of the in-process
hand-overs driven the way the engine drives them, the warm-up wrapper of a capture, and the helper that sets the engine's three
boundary attributes."""
import pytest
import torch

from vface_amd.parallel import (ClipCarry, Exchange, FrameShard, InProcessExchange, LoopbackShard, StreamShard, clip_batches,
                                set_boundary)
from vface_amd.replay import _CountingExchange, _GraphSegments


def slab(v):
    return torch.full((4, 8), float(v), dtype=torch.float16)


def forward(ex, values):
    """One UNet forward's exchanges as the engine issues them: the ordinal stated before every start."""
    got = []
    for k, v in enumerate(values):
        ex.set_index(k)
        got.append(ex.finish_exchange(ex.start_exchange(slab(v))))
    return got


def loopback_world(world):
    store = {}
    shards = [LoopbackShard(r, world, 5, store) for r in range(world)]

    def at(r):
        shards[r].begin_forward()
        return shards[r]
    return at


def carry_world(world):
    carry = ClipCarry(clip_batches(2 * world, 2))

    def at(k):
        carry.begin_batch(k)
        carry.set_step(3)
        return carry
    return at


def test_every_exchange_class_implements_the_protocol():
    for cls in (FrameShard, LoopbackShard, ClipCarry, StreamShard, _GraphSegments, _CountingExchange):
        assert issubclass(cls, Exchange), cls
    for cls in (LoopbackShard, ClipCarry, StreamShard):
        assert issubclass(cls, InProcessExchange) and not issubclass(cls, FrameShard), cls
    assert not Exchange.times_itself and not FrameShard.times_itself and _GraphSegments.times_itself
    sh = FrameShard(0, 1, 5)
    assert (sh.rank, sh.world, sh.first, sh.count, sh.total) == (0, 1, 0, 5, 5)
    assert sh.agree(False, True) == (False, True) and sh.start_exchange(slab(0)) is None and sh.finish_exchange(None) is None


@pytest.mark.parametrize("make", [loopback_world, carry_world])
def test_a_scripted_forward_hands_each_slab_to_the_successor_under_its_ordinal(make):
    at = make(2)
    assert forward(at(0), [10, 11]) == [None, None]                 # rank / batch 0 receives nothing
    got = forward(at(1), [20, 21])
    assert [g.shape for g in got] == [(4, 8)] * 2 and [float(g[0, 0]) for g in got] == [10.0, 11.0]
    assert all(torch.equal(g, slab(v)) for g, v in zip(got, (10, 11)))
    ex = at(1)
    assert ex.agree(False, True) == (False, True) and ex.agree(True) == (True, False)
    for start in (ex.start_temporal, ex.start_gather):
        with pytest.raises(NotImplementedError, match="one after another"):
            start(slab(0))
    one = make(1)(0)
    one.set_index(0)
    assert one.start_exchange(slab(1)) is None and one.finish_exchange(None) is None


def test_stream_halves_refuse_the_two_sided_exchanges_too():
    half = StreamShard(1, 2, 4, {})
    assert (half.first, half.count, half.total) == (2, 2, 4)
    for start in (half.start_temporal, half.start_gather):
        with pytest.raises(NotImplementedError, match="NEXT half"):
            start(slab(0))


def test_the_counting_wrapper_records_the_tails_and_forwards_recv_and_the_ordinal():
    class Seen(LoopbackShard):
        seen = []

        def start_exchange(self, tail, recv=None):
            self.seen.append((self.index, recv))
            return super().start_exchange(tail, recv)

    inner = Seen(1, 2, 5, {0: [slab(7), slab(8)]})
    counting = _CountingExchange(inner)
    assert (counting.rank, counting.world, counting.first, counting.count, counting.total) == (1, 2, 3, 2, 5)
    tails, buf = [slab(1), slab(2)], slab(0)
    got = []
    for k, (t, recv) in enumerate(zip(tails, (buf, None))):
        counting.set_index(k)
        got.append(counting.finish_exchange(counting.start_exchange(t, recv=recv)))
    assert [float(g[0, 0]) for g in got] == [7.0, 8.0]
    assert len(counting.tails) == 2 and all(a is b for a, b in zip(counting.tails, tails))      # in call order
    assert [k for k, _ in inner.seen] == [0, 1] and inner.seen[0][1] is buf and inner.seen[1][1] is None
    with pytest.raises(NotImplementedError):
        counting.start_temporal(slab(0))
    assert counting.tails[2][0] == "temporal"


def test_set_boundary_sets_all_three_returns_what_was_there_and_restores_it():
    class Engine:
        halo_exchange = halo_flow = halo_hw = None
    eng, ex = Engine(), LoopbackShard(1, 2, 5, {})
    flow = torch.arange(2 * 6 * 8, dtype=torch.float64).reshape(2, 8, 6).transpose(1, 2)     # neither fp32 nor contiguous
    assert set_boundary(eng, ex, flow, flow.shape[-2:]) == (None, None, None)
    assert eng.halo_exchange is ex and eng.halo_hw == (6, 8) and type(eng.halo_hw) is tuple
    assert eng.halo_flow.dtype == torch.float32 and eng.halo_flow.is_contiguous() and torch.equal(eng.halo_flow.double(), flow)
    first = (eng.halo_exchange, eng.halo_flow, eng.halo_hw)
    other = LoopbackShard(0, 2, 5, {})
    previous = set_boundary(eng, other)                                 # an exchange alone: no flow, no hw
    assert all(a is b for a, b in zip(previous, first))
    assert eng.halo_exchange is other and eng.halo_flow is None and eng.halo_hw is None
    set_boundary(eng, *previous)
    assert all(a is b for a, b in zip((eng.halo_exchange, eng.halo_flow), first[:2])) and eng.halo_hw == (6, 8)
    assert set_boundary(eng)[0] is ex                                   # nothing given: all three cleared
    assert eng.halo_exchange is None and eng.halo_flow is None and eng.halo_hw is None
