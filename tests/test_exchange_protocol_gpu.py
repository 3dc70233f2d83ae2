"""``parallel.StreamShard`` on two real HIP streams, driven through the protocol alone (no kernel of the library runs): half 0's slab
of every (step, ordinal) reaches half 1 on the other stream, through slots and events that are each used again by the next step."""
import pytest
import torch

from vface_amd.parallel import StreamShard

pytestmark = pytest.mark.gpu


def test_stream_halves_hand_over_every_slab_of_two_steps_and_two_ordinals():
    dev = torch.device("cuda", 0)
    shared = {}
    halves = [StreamShard(h, 2, 4, shared) for h in range(2)]
    streams = [torch.cuda.Stream(dev), torch.cuda.Stream(dev)]
    seen = []
    for step in range(2):
        handles, got, want = [[], []], [], []
        # half 0's host calls of a step are all enqueued before half 1's, as the engine walks the halves
        with torch.cuda.stream(streams[0]):
            for k in range(2):
                tail = torch.full((4, 8), 10.0 * step + k + 1, dtype=torch.float16, device=dev)
                want.append(tail)
                halves[0].set_index(k)
                handles[0].append(halves[0].start_exchange(tail))
                assert halves[0].finish_exchange(handles[0][k]) is None
        with torch.cuda.stream(streams[1]):
            for k in range(2):
                halves[1].set_index(k)
                handles[1].append(halves[1].start_exchange(torch.zeros(4, 8, dtype=torch.float16, device=dev)))
                got.append(halves[1].finish_exchange(handles[1][k]).clone())        # (the slot is written again by the next step)
        streams[1].synchronize()
        for k in range(2):
            assert got[k].dtype == torch.float16 and torch.equal(got[k], want[k]), (step, k, got[k][0, 0].item())
        seen.append({key: (id(shared["slots"][key]), id(shared["events"][key])) for key in shared["slots"]})
    assert sorted(seen[0]) == [(0, 0), (0, 1)] and seen[0] == seen[1]       # one slot and one event per ordinal, re-used by step 2
    torch.cuda.synchronize()
