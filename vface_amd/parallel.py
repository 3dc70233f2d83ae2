"""The boundary exchange of the hooked ``attn1``: ONE protocol (``Exchange``) for the frames a forward does not hold itself.

``Exchange`` is everything ``UNetEngine`` and ``replay`` call on ``engine.halo_exchange`` (set with ``set_boundary``).  It is implemented
by ``FrameShard`` (the ranks of a clip over ``torch.distributed``: one process per GPU, RCCL over xGMI), by the in-process one-neighbour
hand-overs of ``InProcessExchange`` -- ``LoopbackShard`` (ranks one after another), ``ClipCarry`` (the batches of a whole clip,
``--whole_clip``, planned by ``clip_batches``), ``StreamShard`` (the two frame halves of a batch on two HIP streams) -- and by
``replay``'s two wrappers around any of these while a hipGraph is captured.

The hot path shards by frame: every rank runs the full 3-way batch for a contiguous range of frames.  FSAI and
structure injection have no cross-frame dependency.  Three hook modes read other frames, and each has its
exchange step here, issued between the hooked ``attn1``'s projection and its edit:

* ``flow_fix`` reads exactly one neighbour (F9): rank r needs rank r-1's LAST frame's fused q|k of chunk 1 at the level-0
  hooked layers.  Per hooked level-0 layer and DDIM step, a ``[n, 2d]`` 16-bit slab (5.2 MB at 512x512: 2.6 MB each of q and
  k) moves one hop down the chain -- point-to-point ``isend/irecv`` (xGMI is point-to-point, so a one-hop shift costs one link
  transfer), or an all-gather of the slabs when ``mode="allgather"`` (``start_exchange``).  The transfer is started right after
  chunk 1's fused projection and waited for just before the warp, so it overlaps chunk 2's projection
  (see ``UNetEngine._attn1_att``).
* ``temporal`` smooths chunk 0's q|k over +-2 frames: rank r needs the two frames before and the two after its range, in both
  directions, at EVERY hooked layer (``start_temporal``): each rank sends its first two frames down and its last two up
  (point-to-point), or -- with ``mode="allgather"``, or when a shard holds fewer than two frames, so that a needed frame may
  live two ranks away -- all ranks all-gather their first two and last two frames and each picks the ones it needs.
* ``adaIn`` divides by a std over ALL frames: every rank's fp64 row partials (sum, centred M2; ``vface_adain_rows``) are
  all-gathered, padded to the largest shard, and laid out in global row order (``start_gather``) -- the exact array the
  unsharded reduce reads.

``finish_exchange`` completes any of the three (bounded: ``exchange_timeout_s``, ``ExchangeTimeout``).  Under gloo with device
tensors every form runs through host staging (the rehearsal on a box without one GPU per rank).
"""
from __future__ import annotations

import datetime
import os
from typing import Optional

import torch


class ExchangeTimeout(RuntimeError):
    """A boundary exchange did not complete within the bound: the message names this rank and the peer(s) it waited for.
    Callers (bench.py, the entry script) exit non-zero on it instead of waiting for the driver's limit."""


def exchange_timeout_s() -> float:
    """Bound on one boundary exchange, seconds (``VFACE_EXCHANGE_TIMEOUT_S``, default 120).  Under gloo / host staging it is
    the ``Work.wait`` timeout; under RCCL the waits are stream-ordered (the host does not block), so the same figure is handed
    to ``init_process_group(timeout=..)`` (``process_group_timeout``) and RCCL's watchdog aborts the process when a peer never
    shows up; ``VFACE_EXCHANGE_BLOCKING=1`` polls ``Work.is_completed`` on the host instead and raises ``ExchangeTimeout``."""
    return float(os.environ.get("VFACE_EXCHANGE_TIMEOUT_S", "120"))


def process_group_timeout() -> datetime.timedelta:
    return datetime.timedelta(seconds=exchange_timeout_s())


def frame_range(rank: int, world: int, total: int):
    """Contiguous split of ``total`` frames; the first ``total % world`` ranks get one extra."""
    base, extra = divmod(total, world)
    first = rank * base + min(rank, extra)
    return first, base + (1 if rank < extra else 0)


def clip_batches(n_frames: int, n_samples: int):
    """The batch plan of a whole clip: ``[(first, count), ...]`` -- frames ``[0, n_samples)``, ``[n_samples, 2 n_samples)`` .. and,
    where ``n_frames`` is no multiple of ``n_samples``, a last, shorter batch (a one-frame tail is a batch; a clip shorter than
    ``n_samples`` is one batch of ``n_frames``).  Every frame is in exactly one batch.  The loop over batches, the input providers
    and ``ClipCarry`` all read the plan from here."""
    n_frames, n_samples = int(n_frames), int(n_samples)
    if n_frames < 0 or n_samples < 1:
        raise ValueError(f"clip_batches: n_frames >= 0 and n_samples >= 1; got {n_frames}, {n_samples}")
    return [(first, min(n_samples, n_frames - first)) for first in range(0, n_frames, n_samples)]


def set_boundary(engine, exchange=None, flow: Optional[torch.Tensor] = None, hw=None, device=None):
    """Set the engine's three boundary attributes together: ``halo_exchange``, ``halo_flow`` (the field from the frame before
    the forward's first one into it, made contiguous fp32 on ``device``) and ``halo_hw`` (the (h, w) of the clip's flow fields).
    With nothing given all three are cleared.  Returns the triple that was there: ``set_boundary(engine, *previous)`` restores it."""
    previous = (engine.halo_exchange, engine.halo_flow, engine.halo_hw)
    engine.halo_exchange = exchange
    engine.halo_flow = None if flow is None else flow.to(device=device, dtype=torch.float32).contiguous()
    engine.halo_hw = None if hw is None else (int(hw[0]), int(hw[1]))
    return previous


class Exchange:
    """What ``UNetEngine`` and ``replay`` may call on ``engine.halo_exchange``: the contract of every boundary exchange.

    * Identity: ``rank`` of ``world`` holds frames ``[first, first + count)`` of ``total``.
    * Position: ``set_index(k)`` before every start; ``capture_pass(on)`` around the capture pass of a hipGraph capture.
    * The three exchanges, each started with the data to send (and, optionally, a persistent buffer ``recv`` to receive into where
      the form allows it) and completed by ``finish_exchange(handle)``; handles are opaque to the caller, ``None`` is one:
      ``start_exchange(tail)`` -> the predecessor's last-frame slab, or None on rank 0 / in a world of one;
      ``start_temporal(edges)`` -> the two frames before and the two after the range; ``start_gather(part)`` -> every rank's rows, of
      shape ``gather_shape(part)``.
    * Capture bookkeeping: ``graph_signature()``, ``agree(ok, over_budget)``, ``drain(pending, remaining)``.
    * ``times_itself``: the object puts ``engine.exchange_events`` around its own host-issued exchanges; the engine then does not."""

    index = 0
    times_itself = False

    def __init__(self, rank: int = 0, world: int = 1, total_frames: int = 0):
        self.rank, self.world, self.total = rank, world, total_frames
        self.first, self.count = frame_range(rank, world, total_frames)

    def adopt_identity(self, inner: "Exchange") -> None:
        """A wrapper shows the identity of what it wraps."""
        self.rank, self.world, self.first, self.count, self.total = inner.rank, inner.world, inner.first, inner.count, inner.total

    def set_index(self, k: int) -> None:
        """Ordinal of the NEXT exchange inside its UNet forward (0 = the first hooked flow layer, 1 = the second ..): the engine
        states it before every ``start_exchange`` -- eagerly and from the host calls between hipGraph segments alike -- so that an
        exchange object that keeps per-layer state (``StreamShard``) never has to infer it from call counts."""
        self.index = int(k)

    def graph_signature(self):
        """What of this exchange a captured forward depends on: part of ``replay``'s graph key."""
        return (id(self), self.rank, self.world, self.first, self.count)

    def capture_pass(self, on: bool) -> None:
        """``replay`` says when the capture pass of a hipGraph capture begins and ends.  In that pass the forward's kernels are
        recorded, not run, so the slab a ``start_exchange`` is handed there holds no data yet; the call is still made, because
        the ranks of a clip must pair their calls.  Nothing to do for an exchange whose slabs are consumed by the same forward;
        one that KEEPS them (``ClipCarry``) must not keep these."""

    # ---- flow bookkeeping: global flow[i] maps frame i -> frame i+1 (temporal_flow.py:163-188, F-1 fields)
    def local_flow(self, global_flow: torch.Tensor) -> torch.Tensor:
        """Fields between consecutive frames INSIDE this shard: ``[count-1, 2, h, w]``."""
        return global_flow[self.first:self.first + self.count - 1]

    def halo_flow(self, global_flow: torch.Tensor) -> Optional[torch.Tensor]:
        """The field from the previous rank's last frame into this shard's first frame, or None on rank 0."""
        if self.first == 0:
            return None
        return global_flow[self.first - 1]

    def install(self, engine, global_flow: Optional[torch.Tensor] = None, device=None) -> None:
        """Hook the exchange into a ``UNetEngine``: flow_fix layers use it with the clip's flow fields (``global_flow``
        ``[total-1, 2, h, w]``), temporal / adaIn layers without any."""
        flow, hw = (None, None) if global_flow is None else (self.halo_flow(global_flow), global_flow.shape[-2:])
        set_boundary(engine, self if self.world > 1 else None, flow, hw, device)

    # ---- the three exchanges: every implementation has all of them (one that cannot do a form says so: NotImplementedError)
    def start_exchange(self, tail: torch.Tensor, recv: Optional[torch.Tensor] = None):
        raise NotImplementedError

    def start_temporal(self, edges: torch.Tensor, recv: Optional[torch.Tensor] = None):
        raise NotImplementedError

    def start_gather(self, part: torch.Tensor, recv: Optional[torch.Tensor] = None):
        raise NotImplementedError

    def gather_shape(self, part: torch.Tensor):
        """Shape of what ``finish_exchange`` returns for ``start_gather(part)``."""
        return (int(part.shape[0]), int(part.shape[1]) // self.count * self.total) + tuple(part.shape[2:])

    def finish_exchange(self, handle) -> Optional[torch.Tensor]:
        raise NotImplementedError

    # ---- one decision for all ranks of a clip (hipGraph capture outcome)
    def agree(self, ok: bool, over_budget: bool = False):
        """``(every rank ok, any rank over budget)``.  A rank whose capture failed and a rank whose capture succeeded must take ONE
        decision, or their exchange counts stop pairing.  Here: one process, whose own verdict is everybody's."""
        return bool(ok), bool(over_budget)

    def drain(self, pending, remaining) -> None:
        """Finish the paired exchanges of an aborted forward so that the neighbours' calls still match: ``pending`` = a handle
        that was started and not finished (or None), ``remaining`` = the slabs (tensors shaped like the tails the forward would
        have sent; contents irrelevant) of the exchanges not yet started -- a ``(kind, tensor)`` pair for a temporal halo or an
        adaIn gather (kind ``"temporal"`` / ``"gather"``)."""
        if pending is not None:
            self.finish_exchange(pending)
        for tail in remaining:
            kind, t = tail if isinstance(tail, tuple) else ("exchange", tail)
            self.finish_exchange(getattr(self, "start_" + kind)(t))


class FrameShard(Exchange):
    """The ranks of a clip over ``torch.distributed``: rank r holds ``frame_range(r, world, total)``."""

    def __init__(self, rank: int, world: int, total_frames: int, dist=None, mode: str = "p2p"):
        super().__init__(rank, world, total_frames)
        self.dist = dist
        self.mode = mode
        if world > 1 and dist is None:
            raise ValueError("world_size > 1 needs torch.distributed")

    def _staged(self, t: torch.Tensor):
        """``(what the backend is handed, the device the result goes back to)``.  gloo cannot move device memory peer to peer: a
        rehearsal on a box without one GPU per rank runs the same protocol through host staging (a CPU copy, and the device to return
        to).  Production runs use backend "nccl" (RCCL over xGMI): the tensor itself, and None."""
        if t.is_cuda and self.dist.get_backend() == "gloo":
            return t.detach().to("cpu").contiguous(), t.device
        return t.contiguous(), None

    def handle(self, works, result, peers: Optional[str] = None):
        """The handle of a started exchange: the works to wait for, ``result()`` -> what ``finish_exchange`` returns once they are
        done, and whom to name when they are not done in time (default: the flow halo's peers)."""
        return (works, result, peers)

    def start_exchange(self, tail: torch.Tensor, recv: Optional[torch.Tensor] = None):
        """Send this shard's last-frame slab to rank+1 and start receiving rank-1's.  Returns a handle.
        ``recv``: a persistent receive buffer shaped like ``tail`` (the hipGraph-segmented forward bakes its address into
        the captured warp launch); default: a fresh one per call."""
        if self.world == 1:
            return None
        d = self.dist
        src, dev = self._staged(tail)
        if self.mode == "allgather" and dev is None:
            bufs = torch.empty((self.world * src.shape[0],) + tuple(src.shape[1:]), dtype=src.dtype, device=src.device)
            work = d.all_gather_into_tensor(bufs, src, async_op=True)  # rank r's slab = rows [r*n, (r+1)*n)
            return self.handle([work], lambda: bufs.view((self.world,) + tuple(src.shape))[self.rank - 1] if self.rank > 0 else None)
        ops, halo = [], None
        if self.rank + 1 < self.world:
            ops.append(d.P2POp(d.isend, src, self.rank + 1))
        if self.rank > 0:
            halo = recv if (recv is not None and dev is None) else torch.empty_like(src)
            ops.append(d.P2POp(d.irecv, halo, self.rank - 1))
        return self.handle(d.batch_isend_irecv(ops), lambda: halo.to(dev) if (halo is not None and dev is not None) else halo)

    # ---- the two-directional halo of fusion="temporal" (+-2 frames) and the row-partial gather of fusion="adaIn"
    def temporal_form(self) -> str:
        """``"p2p"`` where every shard holds at least two frames (a +-2 window then reaches the neighbouring ranks only), else
        ``"allgather"``.  Decided from (mode, world, total) alone -- ``frame_range`` gives the last rank the fewest frames -- so
        every rank of the clip makes the same choice."""
        return "p2p" if self.mode == "p2p" and self.total // self.world >= 2 else "allgather"

    def halo_frames(self):
        """Global frames of the four slots ``start_temporal``'s result holds: first-2, first-1, last+1, last+2 (None: outside the clip)."""
        last = self.first + self.count - 1
        return [g if 0 <= g < self.total else None for g in (self.first - 2, self.first - 1, last + 1, last + 2)]

    def _edge_slot(self, g: int):
        """(rank, slot of its ``edges``) that carries global frame ``g`` -- one of the owner's first two or last two frames
        whenever another rank's window reaches it."""
        for q in range(self.world):
            f, c = frame_range(q, self.world, self.total)
            if f <= g < f + c:
                j = g - f
                return q, (j if j < 2 else 4 - (c - j))
        raise IndexError(g)

    def start_temporal(self, edges: torch.Tensor, recv: Optional[torch.Tensor] = None):
        """Start the temporal halo exchange.  ``edges`` ``[4, ...]``: this shard's frames first, first+1, last-1, last (a
        one-frame shard: its frame in slots 0 and 3).  ``finish_exchange`` then returns ``[4, ...]``: global frames first-2,
        first-1, last+1, last+2 (``halo_frames``; a slot outside the clip is left unwritten).  ``recv``: a persistent buffer
        shaped like ``edges`` to receive into where the form allows it (RCCL point-to-point)."""
        if self.world == 1:
            return None
        d = self.dist
        src, dev = self._staged(edges)
        if self.temporal_form() == "p2p":
            halo = recv if (recv is not None and dev is None) else torch.empty_like(src)
            ops = []
            if self.rank > 0:
                ops += [d.P2POp(d.isend, src[0:2], self.rank - 1), d.P2POp(d.irecv, halo[0:2], self.rank - 1)]
            if self.rank + 1 < self.world:
                ops += [d.P2POp(d.isend, src[2:4], self.rank + 1), d.P2POp(d.irecv, halo[2:4], self.rank + 1)]
            peers = " and ".join(f"rank {q}" for q in (self.rank - 1, self.rank + 1) if 0 <= q < self.world) + " (their edge frames)"
            return self.handle(d.batch_isend_irecv(ops), lambda: halo.to(dev) if dev is not None else halo, peers)
        bufs = torch.empty((self.world * 4,) + tuple(src.shape[1:]), dtype=src.dtype, device=src.device)
        work = d.all_gather_into_tensor(bufs, src, async_op=True)       # rank q's edge slots = rows [4q, 4q + 4)

        def pick():
            halo = torch.empty((4,) + tuple(bufs.shape[1:]), dtype=bufs.dtype, device=bufs.device)
            for s, g in enumerate(self.halo_frames()):
                if g is not None:
                    q, slot = self._edge_slot(g)
                    halo[s].copy_(bufs[4 * q + slot])
            return halo.to(dev) if dev is not None else halo
        return self.handle([work], pick, f"all {self.world} ranks (all-gather of edge frames)")

    def start_gather(self, part: torch.Tensor, recv: Optional[torch.Tensor] = None):
        """Start the gather of adaIn row partials: ``part`` ``[P, count * n, 2]`` fp64 (P arrays of this shard's rows).
        ``finish_exchange`` returns ``[P, total * n, 2]``: every rank's rows in global row order.  Shards of unequal length are
        padded to the longest for the all-gather.  (``recv`` is accepted for symmetry; the result is always assembled.)"""
        if self.world == 1:
            return None
        d = self.dist
        P, rows = int(part.shape[0]), int(part.shape[1])
        n = rows // self.count
        most = frame_range(0, self.world, self.total)[1] * n
        src, dev = self._staged(part)
        if rows < most:
            src = torch.cat([src, torch.zeros((P, most - rows) + tuple(src.shape[2:]), dtype=src.dtype, device=src.device)], 1)
        flat = torch.empty((self.world * P,) + tuple(src.shape[1:]), dtype=src.dtype, device=src.device)
        work = d.all_gather_into_tensor(flat, src, async_op=True)       # rank q's arrays = rows [qP, (q + 1)P)
        bufs = flat.view((self.world, P) + tuple(src.shape[1:]))

        def assemble():
            out = torch.empty((P, self.total * n) + tuple(bufs.shape[3:]), dtype=bufs.dtype, device=bufs.device)
            for q in range(self.world):
                f, c = frame_range(q, self.world, self.total)
                out[:, f * n:(f + c) * n].copy_(bufs[q, :, :c * n])
            return out.to(dev) if dev is not None else out
        return self.handle([work], assemble, f"all {self.world} ranks (all-gather of adaIn row partials)")

    def _peers(self) -> str:
        peers = ([f"rank {self.rank - 1} (its last-frame slab)"] if self.rank > 0 else []) + \
                ([f"rank {self.rank + 1} (to take ours)"] if self.rank + 1 < self.world else [])
        return " and ".join(peers) if self.mode != "allgather" else f"all {self.world} ranks (all-gather)"

    def _wait(self, works, peers: Optional[str] = None) -> None:
        """Bounded wait on the works of one exchange.  gloo (and any backend whose ``wait`` blocks the host) takes the timeout
        directly; RCCL's ``wait`` only orders the stream, so the bound there is the process group's own timeout (watchdog),
        unless ``VFACE_EXCHANGE_BLOCKING=1`` asks for host polling.  ``peers``: whom the exchange waits for, named in the
        ``ExchangeTimeout`` message (default: the flow halo's peers)."""
        limit = exchange_timeout_s()
        backend = self.dist.get_backend()
        poll = backend != "gloo" and os.environ.get("VFACE_EXCHANGE_BLOCKING") == "1"
        import time
        t0 = time.monotonic()
        for w in works:
            try:
                if poll:
                    while not w.is_completed():
                        if time.monotonic() - t0 > limit:
                            raise TimeoutError
                        time.sleep(1e-4)
                    w.wait()
                elif backend == "gloo":
                    left = max(limit - (time.monotonic() - t0), 1e-3)
                    if w.wait(datetime.timedelta(seconds=left)) is False:
                        raise TimeoutError
                else:
                    w.wait()
            except (TimeoutError, RuntimeError) as e:
                if isinstance(e, TimeoutError) or "time" in str(e).lower():
                    raise ExchangeTimeout(f"rank {self.rank} of {self.world}: the boundary exchange did not complete within "
                                          f"{limit:g} s -- waited for {peers or self._peers()}") from e
                raise

    def finish_exchange(self, handle) -> Optional[torch.Tensor]:
        """Wait (bounded: ``exchange_timeout_s``) for the transfer; returns the previous rank's slab (None on rank 0 / single
        rank) -- or, for a ``start_temporal`` / ``start_gather`` handle, what those describe.  Raises ``ExchangeTimeout`` naming
        the peer when it does not arrive."""
        if handle is None:
            return None
        works, result, peers = handle
        self._wait(works, peers)
        return result()

    def agree(self, ok: bool, over_budget: bool = False):
        """All-reduce the two flags over the ranks of the clip."""
        if self.world == 1:
            return bool(ok), bool(over_budget)
        d = self.dist
        dev = "cuda" if d.get_backend() == "nccl" else "cpu"
        t = torch.tensor([0 if ok else 1, 1 if over_budget else 0], dtype=torch.int32, device=dev)
        d.all_reduce(t, op=d.ReduceOp.MAX)
        bad, over = (int(v) for v in t.cpu())
        return bad == 0, over != 0

    def slab_bytes_per_step(self, n: int, d: int, layers: int = 2, elem: int = 2) -> int:
        """Bytes this rank SENDS per DDIM step: one ``[n, 2d]`` slab per hooked level-0 layer (none from the last rank)."""
        return 0 if self.rank + 1 >= self.world else layers * n * 2 * d * elem


class InProcessExchange(Exchange):
    """A one-neighbour hand-over inside ONE process: whoever is at ``rank`` leaves its last-frame slab under a key, its successor
    fetches the slab its predecessor left under the same key.  The chain has no cycle (rank 0 needs nothing).  A subclass says what
    the key is (``_key``), where a slab is put (``_put``) and where the predecessor's is fetched (``_fetch``), and why nothing
    but the one neighbour behind can be served (``one_neighbour_only``: the temporal halo and the adaIn gather are refused)."""

    last_stores = False         # whether the last rank's slabs, which nobody reads, are put too

    def start_exchange(self, tail: torch.Tensor, recv=None):
        if self.world == 1:
            return None
        key = self._key()
        if self.rank + 1 < self.world or self.last_stores:
            self._put(key, tail)
        return (key,)

    def finish_exchange(self, handle):
        if handle is None or self.rank == 0:
            return None
        return self._fetch(handle[0])

    def start_temporal(self, edges, recv=None):
        raise NotImplementedError(self.one_neighbour_only)

    start_gather = start_temporal


class LoopbackShard(InProcessExchange):
    """All shards of a clip run ONE AFTER ANOTHER in one process on one GPU: rank r's boundary slabs are kept in memory
    (in call order -- one per hooked level-0 layer and UNet call) and handed to rank r+1 when it runs, so running the ranks in
    order needs no concurrency.  Same engine code path as the RCCL exchange (``UNetEngine._attn1_att``), which makes it the strict
    bit-for-bit test of that path (tests/test_sharded_gpu.py) and a way to walk a clip that does not fit one batch through one GPU."""

    one_neighbour_only = ("a loop-back shard runs the ranks one after another: the temporal halo needs the NEXT rank's frames too, "
                          "the adaIn gather every rank's rows (run the shards as processes: FrameShard)")
    last_stores = True          # (every rank's list then counts the exchanges of its forward)

    def __init__(self, rank: int, world: int, total_frames: int, store: dict):
        super().__init__(rank, world, total_frames)
        self.store = store          # {rank: [slab, ...]} shared by the shards of one clip
        self.store.setdefault(rank, [])
        self._next = 0

    def begin_forward(self):
        """Call before each UNet forward of this shard: its slabs are re-recorded, the predecessor's re-read."""
        self.store[self.rank] = []
        self._next = 0

    def _key(self):
        return self._next           # call order

    def _put(self, key, tail):
        self.store[self.rank].append(tail.detach().clone())
        self._next += 1

    def _fetch(self, key):
        return self.store[self.rank - 1][key]


class ClipCarry(InProcessExchange):
    """The batches of ONE clip walked one after another through one GPU, each through its whole DDIM loop, with ``flow_fix``
    coupled across the batch boundaries: batch k keeps its last frame's fused q|k slab of EVERY step and hooked level-0 layer,
    batch k + 1 reads them where the unbatched clip reads the frame before.  One object per clip; ``begin_batch(k)`` moves it to
    batch k of the plan (``clip_batches``), which is what ``rank`` / ``first`` / ``count`` then say -- not ``frame_range``.

    * The store is keyed by ``(step, ordinal)``: the sampler states the DDIM step before each UNet call (``set_step``), the engine
      the ordinal of the exchange inside the forward (``set_index``), eagerly and from the host calls between hipGraph segments
      alike.  A capturing call runs the forward up to three times -- warm-up, capture pass, first replay -- so a repeated
      ``start_exchange`` for one key overwrites its slab; the capture pass's slabs hold no data (its kernels are recorded, not
      run) and are not stored (``capture_pass``), so a capture that falls back to the warm-up forward's result -- it failed, or
      its pool is over the byte budget -- leaves the warm-up's slabs in place; nothing is owed to another rank (``drain``).
    * Two generations at most are alive: the one being read (batch k - 1's) and the one being written (batch k's); the slabs of
      an older one are recycled as the buffers of the one being written.  One generation is steps x hooked layers x ``[n, 2d]``
      16-bit (50 x 2 x 4096 x 640 x 2 B = 524 MB at 512 x 512).  The last batch keeps nothing, and ``end_batch`` after its loop
      lets go of what it read.
    * Reading a key the previous batch never wrote (it ran fewer steps, or another hook plan) raises, naming step and ordinal.
    * ``temporal`` needs the NEXT batch's frames and ``adaIn`` every frame of the clip: both raise, as on a loop-back shard."""

    one_neighbour_only = ("a clip carry runs the batches one after another: the temporal halo needs the NEXT batch's frames too, "
                          "the adaIn gather every frame of the clip")

    def __init__(self, batches):
        self.batches = [(int(f), int(c)) for f, c in batches]
        if not self.batches:
            raise ValueError("ClipCarry: a clip has at least one batch")
        super().__init__(0, len(self.batches), sum(c for _, c in self.batches))      # (first / count: begin_batch)
        self._capturing = False
        self.generations: dict = {}     # batch -> {(step, ordinal): slab}
        self._spare: list = []          # slabs of dropped generations, re-used as buffers
        self.step: Optional[int] = None
        self.begin_batch(0)

    def begin_batch(self, k: int) -> None:
        """Move to batch ``k`` of the plan: it reads generation k - 1 and writes generation k (anew); every other one is dropped."""
        if not 0 <= k < self.world:
            raise IndexError(f"ClipCarry: batch {k} of a plan of {self.world}")
        self.rank = int(k)
        self.first, self.count = self.batches[k]
        for g in [g for g in self.generations if g != k - 1]:
            self._spare += list(self.generations.pop(g).values())
        self.generations[k] = {}
        if k + 1 == self.world:
            self._spare = []        # (the last batch writes nothing: the buffers are let go)
        self.step = None

    def end_batch(self) -> None:
        """After the batch's DDIM loop: the last batch of the clip lets go of the generation it read (nobody reads it again)."""
        if self.rank + 1 == self.world:
            self.generations.pop(self.rank - 1, None)

    def capture_pass(self, on: bool) -> None:
        self._capturing = bool(on)

    def drain(self, pending, remaining) -> None:
        """An aborted capture owes nobody an exchange here, and the warm-up forward's slabs are already stored."""

    def set_step(self, step: int) -> None:
        """The DDIM step of the NEXT UNet forward (the sampler's loop counter), stated before it."""
        self.step = int(step)

    def _key(self):
        if self.step is None:
            raise RuntimeError("ClipCarry: the sampler has to state the DDIM step (set_step) before a UNet forward that exchanges")
        return (self.step, int(self.index))

    def _put(self, key, tail):
        if self._capturing:
            return
        gen = self.generations[self.rank]
        slot = gen.get(key)
        if slot is None or slot.shape != tail.shape or slot.dtype != tail.dtype or slot.device != tail.device:
            at = next((i for i, s in enumerate(self._spare)
                       if s.shape == tail.shape and s.dtype == tail.dtype and s.device == tail.device), None)
            slot = gen[key] = self._spare.pop(at) if at is not None else torch.empty_like(tail, memory_format=torch.contiguous_format)
        slot.copy_(tail)        # (stream-ordered, on the stream of the forward; a second start for this key lands here again)

    def _fetch(self, key):
        slab = self.generations.get(self.rank - 1, {}).get(key)
        if slab is None:
            raise KeyError(f"ClipCarry: batch {self.rank} reads the slab of DDIM step {key[0]}, exchange ordinal {key[1]}, which batch "
                           f"{self.rank - 1} never wrote (it ran fewer steps, or with another hook plan)")
        return slab

    def carry_bytes(self) -> int:
        """Bytes of the generation being written: what this batch hands to the next one."""
        return sum(s.numel() * s.element_size() for s in self.generations.get(self.rank, {}).values())

    def graph_signature(self):
        """What of this object a captured forward depends on (``replay``'s graph key): whether it reads a slab, and how many frames
        it holds -- not which batch of the plan it is at, so that batches of one shape replay one capture."""
        return (id(self), self.rank > 0, self.world, self.count)

    def install(self, engine, boundary_flow: Optional[torch.Tensor] = None, hw=None, device=None) -> None:
        """Hook the carry into a ``UNetEngine`` for the batch it is at.  ``boundary_flow`` ``[2, h, w]``: the field from the previous
        batch's last frame into this batch's frame 0 (batch 0: None); ``hw``: the (h, w) of the clip's flow fields.  A clip of one
        batch has no boundary: nothing is installed."""
        if self.world == 1:
            set_boundary(engine)
            return
        if self.rank > 0 and boundary_flow is None:
            raise ValueError(f"ClipCarry: batch {self.rank} needs the flow field from the previous batch's last frame into its frame 0")
        flow = boundary_flow.reshape(2, boundary_flow.shape[-2], boundary_flow.shape[-1]) if self.rank > 0 else None
        set_boundary(engine, self, flow, hw, device)

    @staticmethod
    def uninstall(engine) -> None:
        set_boundary(engine)


class StreamShard(InProcessExchange):
    """The two frame halves of ONE batch on one GPU as two shards that run AT THE SAME TIME on two HIP streams (the engine's two
    launch streams under ``flow_fix``, whose warp reads the previous frame: UNetEngine._step_forward_split).  Half 0 hands the
    fused q|k of its last frame to half 1 at every hooked flow layer, through device memory and an event:

      half 0, on its stream:  slab -> slot[k] (device copy), then record event[k]            (start_exchange)
      half 1, on its stream:  wait for event[k]; the warp (or the graph's receive buffer) then reads slot[k]   (finish_exchange)

    What makes this hand-over safe, each a hazard the form withdrawn in round 4 may have had (its code was never committed):
    * one slot and one event PER exchange ordinal k (``set_index``), never one re-used slot: half 0 does not wait for half 1, so it
      reaches the second hooked layer and stores its slab there while half 1 may not yet have consumed the first;
    * the ordinal is STATED by the engine, not counted here: a capturing call runs the forward three times (warm-up, capture
      pass, first replay), a replay once -- a counter drifts between the two;
    * half 0's host calls of a step are all enqueued BEFORE half 1's (the engine walks the halves in order), so when half 1
      enqueues its wait the event's latest record IS this step's: a wait enqueued before that record would refer to the previous
      step's and return at once -- reading the previous step's slab (the ~1e-3-sized, frame-3-then-5 difference of
      gpurun_out/r4E_t.log is what a stale slab produces after three DDIM steps);
    * slot[k] is re-written only by the next step's half 0, which starts after this step's join (both streams waited for);
    * slots and events are allocated once and never freed (no caching-allocator re-use across streams);
    * every stream-ordered call here goes to ``torch.cuda.current_stream()``: the warm-up forward of a capture runs on a side
      stream, the capture pass's real exchanges on the capturing stream, replays on the half's launch stream."""

    one_neighbour_only = ("the halves of a batch on two streams hand one frame forward: the temporal halo needs the NEXT half's frames "
                          "too, the adaIn gather every frame's rows (such a batch runs whole)")

    def __init__(self, rank: int, world: int, total_frames: int, shared: dict):
        super().__init__(rank, world, total_frames)
        self.shared = shared            # {"slots": {(rank, k): tensor}, "events": {(rank, k): Event}} of the batch's shards
        self.shared.setdefault("slots", {})
        self.shared.setdefault("events", {})

    def _key(self):
        return self.index               # the ordinal, as stated

    def _put(self, k, tail):
        key = (self.rank, k)
        slot = self.shared["slots"].get(key)
        if slot is None or slot.shape != tail.shape or slot.dtype != tail.dtype:
            slot = self.shared["slots"][key] = torch.empty(tail.shape, dtype=tail.dtype, device=tail.device)
        slot.copy_(tail)
        ev = self.shared["events"].get(key)
        if ev is None:
            ev = self.shared["events"][key] = torch.cuda.Event()
        ev.record()                                   # on the current stream, behind the copy

    def _fetch(self, k):
        key = (self.rank - 1, k)
        ev = self.shared["events"].get(key)
        if ev is None:
            raise RuntimeError(f"StreamShard: half {self.rank} reached exchange {k} before half {self.rank - 1} issued it "
                               "(the halves must be enqueued in order)")
        torch.cuda.current_stream().wait_event(ev)
        return self.shared["slots"][key]
