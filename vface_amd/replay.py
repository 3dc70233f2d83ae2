"""How the UNet forward of a DDIM step reaches the device: kernel by kernel, as a captured hipGraph (in segments cut where a
frame-sharded forward exchanges with its neighbours), or as two frame halves on two HIP streams at once -- with the overlap probe,
the bit self-check and the both-ways timing that decide whether an engine keeps that form.  ``UNetEngine`` (engine.py), which
inherits from ``_StepReplay``, says what one forward computes; no kernel is called from this file.

The boundary exchange is spoken to through ``parallel.Exchange`` alone.  Two implementations of it live here, both wrappers around
the engine's own exchange while a hipGraph is captured: ``_CountingExchange`` (the warm-up forward) and ``_GraphSegments`` (the
capture pass, and the host calls of every replay)."""
from __future__ import annotations

import gc
import os
import warnings
from typing import Dict, Optional

import torch

from . import hip
from .parallel import Exchange, StreamShard, set_boundary


def _timed(cur, fn):
    """``(ms, fn())``: HIP events on stream ``cur`` around what ``fn`` enqueues, waited for."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(cur)
    out = fn()
    e1.record(cur)
    e1.synchronize()
    return e0.elapsed_time(e1), out


def _between_events(events, fn):
    """``fn()`` -- one ``finish_exchange`` -- with a (start, end) pair of HIP events around what it enqueues on the current stream,
    appended to ``events`` (the engine's ``exchange_events``: a list, or None: not timed)."""
    if events is None:
        return fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    events.append((e0, e1))
    return out


class _GraphSegments(Exchange):
    """Capture of one UNet forward as a chain of hipGraphs sharing ONE memory pool, cut wherever the forward calls the
    frame-shard exchange (``start_exchange`` / ``finish_exchange``): those two calls are host-issued RCCL operations and run
    BETWEEN segment replays, on the same stream, in the captured order.  Installed as the engine's ``halo_exchange`` while
    capturing.  Buffers the captured launches exchange with the host calls have fixed addresses: the slab to send is a view
    of a pool tensor; the slab received lands in a persistent ``recv`` buffer owned by this object (the inner exchange
    receives straight into it where it can -- RCCL p2p -- otherwise its result is copied there).
    An unsharded forward is the degenerate case: one segment, no host call."""

    times_itself = True           # (its host calls run at every replay, where the engine's own timing is not on the path)

    def __init__(self, engine, inner):
        self.engine, self.inner = engine, inner
        self.stream = torch.cuda.Stream()
        self.pool = torch.cuda.graph_pool_handle()
        self.segments: list = []      # [(CUDAGraph, host_op | None)]
        self.keep: list = []          # tensors the host ops refer to
        self.cur = None
        self.n_started = 0            # exchanges the capture pass has started for real ..
        self.pending = None           # .. and the state dict of one that was started and not yet finished
        if inner is not None:
            self.adopt_identity(inner)

    def begin(self):
        self.cur = torch.cuda.CUDAGraph()
        # (thread_local: a collective backend's watchdog thread may poll events while this thread captures)
        self.cur.capture_begin(pool=self.pool, capture_error_mode="thread_local")

    def end(self, host_op):
        # A segment in which the forward launched nothing (two exchange calls back to back: half 0 of a coupled split has
        # nothing to wait for) is not kept -- torch says so with a warning at capture_end; replaying it would be a no-op launch
        # per step.  Its host call, if any, still runs at its place in the chain.
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            self.cur.capture_end()
        empty = any("Graph is empty" in str(w.message) for w in caught)
        for w in caught:
            if "Graph is empty" not in str(w.message):
                warnings.warn_explicit(w.message, w.category, w.filename, w.lineno)
        if not empty or host_op is not None:
            self.segments.append((None if empty else self.cur, host_op))
        self.cur = None

    def abort(self):
        """End a capture that will not be used.  ``capture_end`` must run on the CAPTURING stream: the exception that brings us
        here has already unwound the ``with torch.cuda.stream(..)`` block, and ending the capture from another stream is a
        fatal HIP error (process abort), not a Python exception."""
        if self.cur is not None:
            try:
                with torch.cuda.stream(self.stream):
                    self.cur.capture_end()
            except Exception:
                pass
            self.cur = None

    # ---- the exchange interface (parallel.Exchange), as seen by UNetEngine._attn1_att while capturing: the ordinal the engine
    # states (set_index) is baked into the host call; ``recv`` is this object's to choose
    def start_exchange(self, tail: torch.Tensor, recv=None):
        recv = torch.empty_like(tail) if self.inner.rank > 0 else None      # (allocated in the shared pool: lives with the graphs)
        return self._start("start_exchange", tail, recv)

    def start_temporal(self, edges: torch.Tensor, recv=None):
        """The temporal halo (``FrameShard.start_temporal``): every rank receives (frames on both sides)."""
        return self._start("start_temporal", edges, torch.empty_like(edges))

    def start_gather(self, part: torch.Tensor, recv=None):
        """The adaIn row-partial gather (``FrameShard.start_gather``): the gathered array lands in a persistent buffer."""
        return self._start("start_gather", part, torch.empty(self.inner.gather_shape(part), dtype=part.dtype, device=part.device))

    def _start(self, method: str, tail: torch.Tensor, recv: Optional[torch.Tensor]):
        inner, state, k = self.inner, {}, self.index
        self.keep += [tail, recv, state]

        def op():
            inner.set_index(k)                     # (the replayed host call states the same ordinal as the captured forward did)
            state["h"] = getattr(inner, method)(tail, recv=recv)
        self.end(op)
        op()                       # the capture pass exchanges for real too (garbage slabs): the ranks' calls stay paired
        self.n_started += 1
        self.pending = state
        self.begin()
        return (state, recv)

    def finish_exchange(self, handle):
        state, recv = handle
        inner, eng = self.inner, self.engine
        if os.environ.get("VFACE_TEST_FAIL_CAPTURE") == "mid":      # (test hook: die with one exchange started, not finished)
            raise RuntimeError("injected capture failure (VFACE_TEST_FAIL_CAPTURE)")

        def finish():
            halo = inner.finish_exchange(state.pop("h"))
            if halo is not None and recv is not None and halo.data_ptr() != recv.data_ptr():
                recv.copy_(halo)
        op = lambda: _between_events(eng.exchange_events, finish)
        self.end(op)
        op()
        self.pending = None
        self.begin()
        return recv


class _CountingExchange(Exchange):
    """The frame-shard exchange seen by the warm-up forward of a capture: passes every call through and records the slabs a
    forward sends (shapes only), so that a capture pass that dies half-way can finish its paired exchanges (``Exchange.drain``)."""

    def __init__(self, inner):
        self.inner, self.tails = inner, []
        self.adopt_identity(inner)

    def set_index(self, k: int) -> None:
        self.inner.set_index(k)

    def start_exchange(self, tail, recv=None):
        self.tails.append(tail)
        return self.inner.start_exchange(tail, recv=recv)

    def start_temporal(self, edges, recv=None):
        self.tails.append(("temporal", edges))
        return self.inner.start_temporal(edges, recv=recv)

    def start_gather(self, part, recv=None):
        self.tails.append(("gather", part))
        return self.inner.start_gather(part, recv=recv)

    def finish_exchange(self, handle):
        return self.inner.finish_exchange(handle)


class _StepReplay:
    """Base class of ``UNetEngine``, which supplies ``forward_nhwc``, the packed weights and the ``halo_*`` exchange attributes."""

    def _init_replay(self):
        # hipGraph replay of the UNet forward of a DDIM step (step_forward_nhwc): capture once per (batch, resolution, hook
        # configuration, context shape) and replay -- the default since round 3 (bit-equal to kernel-by-kernel launches, one
        # host call per step instead of ~1200; what bench.py times); VFACE_GRAPH=0 launches kernel by kernel.  The C ABI is
        # allocation-free and stream-ordered, so the captured graph is exactly the eager launch sequence.  Every cached graph
        # pins a private pool with the activations of one forward (~0.45 GB per frame at 512 x 512): the cache is bounded by
        # BYTES (VFACE_GRAPH_GB, default 64 of the 288 GB) and by count, least recently used first; a forward whose pool alone
        # exceeds the budget is not cached and runs kernel by kernel.
        self.use_graph = os.environ.get("VFACE_GRAPH", "1") != "0"
        self._graphs: "Dict[tuple, dict]" = {}
        self._graph_failed: set = set()       # keys whose capture failed: they run kernel by kernel, other keys still capture
        self.graph_capacity = 12        # (a split configuration holds three graphs: two halves and, for its self-check and timing, the whole batch)
        self.graph_budget_bytes = int(float(os.environ.get("VFACE_GRAPH_GB", "64")) * (1 << 30))
        self.split_streams = int(os.environ.get("VFACE_STREAMS", "2"))      # two launch streams (_step_forward_split); 1 = one stream
        self._split_state: "Dict[tuple, dict]" = {}
        self._split_pair = None
        self._split_verified = False
        self.split_overlap = None      # step time / (half A + half B) of the measured split step: ~0.5 = the halves ran at once
        self.split_selfcheck = os.environ.get("VFACE_SPLIT_SELFCHECK", "1") != "0"      # (_split_bit_check, _split_time_both; 0 skips both)
        self.split_checked: Dict[str, bool] = {}       # kind -> the halves' eps equalled the single sequence's
        self.split_timing: Dict[tuple, tuple] = {}     # (kind, samples, H, W) -> (ms of a two-sequence step, ms of a one-sequence step)
        self._split_off: set = set()                   # ... the configurations that stay on one launch sequence because it measured faster

    def _hooked_cfgs(self):
        """The ``HookCfg`` (or None) of every SpatialTransformer's first attn1, in ``layer_table()`` order."""
        for kind, _, mod in self.unet.layer_table():
            if kind == "st":
                yield getattr(mod.transformer_blocks[0].attn1, "_vface_cfg", None)

    # ------------------------------------------------------------------ hipGraph replay of a step's forward
    # Every engine switch that changes the captured launch sequence: part of the graph key, so that toggling one on a live engine
    # does not replay a stale graph (tests/test_host_cpu.py holds every VFACE_* switch of the initialisers against this list)
    _GRAPH_SWITCHES = ("stream32", "fuse_gn", "fuse_ffn", "fuse_front", "fuse_tail", "fuse_post", "fuse_temb", "fuse_out", "concat32",
                       "interior16", "live_chunks", "share_prefix")

    def _hook_signature(self):
        """(signature, flows): everything the hooked attn1 layers contribute to the launch sequence -- the HookCfg fields and
        the flow tensors' shapes -- and the distinct flow tensors themselves, in order of first use."""
        sig, flows = [], []
        for cfg in self._hooked_cfgs():
            if cfg is None:
                sig.append(None)
                continue
            fl = cfg.flow
            if fl is not None and not any(f is fl for f in flows):
                flows.append(fl)
            sig.append((cfg.switch_on, cfg.chunks, cfg.fusion, cfg.split_ratio_fft, cfg.alpha, cfg.flow_gate,
                        (next(i for i, f in enumerate(flows) if f is fl), tuple(fl.shape)) if fl is not None else None))
        return tuple(sig), flows

    _SPLIT_SAFE = ("replace", "fft", "fft_vfixed", "mix")      # hook modes that never read another FRAME (pnp_utils.py:133-262)
    # ... and the one that reads exactly ONE neighbour (temporal_flow.py:222-237): its halves run as two in-process frame shards,
    # half 0 handing its last frame's fused q|k to half 1 at every hooked flow layer (parallel.StreamShard)
    _SPLIT_COUPLED = ("flow_fix",)

    def _split_plan(self, N: int):
        """Index tensors of the two frame halves of an N-sample batch (frames [0, F/2) and [F/2, F) of every chunk), or None when
        this forward has to stay whole: one stream asked for, frames sharded over ranks, a hook mode that couples frames
        (flow_fix's warp, temporal, adaIn), an odd frame count, or a batch too small to be worth two launch sequences."""
        plan, self._split_coupled = self._split_decide(N)
        return plan

    def _split_decide(self, N: int):
        """``_split_plan``, and what it publishes as ``_split_coupled``: the flow_fix HookCfgs whose halves hand one frame over, or None."""
        if self.split_streams < 2 or self.halo_exchange is not None or N < 12:      # (8 samples: 11.75 vs 11.46 ms whole, profiles/r04_n)
            return None, None
        chunks, coupled = 1, []
        for cfg in self._hooked_cfgs():
            if cfg is None or not cfg.switch_on or cfg.chunks not in (2, 3):
                continue
            if cfg.chunks == 3 and cfg.fusion in self._SPLIT_COUPLED and os.environ.get("VFACE_SPLIT_COUPLED", "1") != "0":
                if cfg.flow is not None:
                    if coupled and coupled[0].flow is not cfg.flow:
                        return None, None          # (two different flow tensors in one forward: one halo field cannot serve both)
                    if not any(c is cfg for c in coupled):
                        coupled.append(cfg)
            elif cfg.chunks == 3 and cfg.fusion not in self._SPLIT_SAFE:
                return None, None
            there = cfg.chunks if self.live_chunks is None else self.live_chunks
            if chunks not in (1, there):
                return None, None
            chunks = there
        if self.share_prefix:
            # the batch is the sampler's [x ; x ; inv_t]: each half must again be three chunks of the same frames
            # (_shared_block), also when no hook says so
            want = 3 if self.live_chunks is None else self.live_chunks
            if chunks == 1:
                chunks = want
            elif chunks != want:
                return None, None
        if N % chunks or (N // chunks) % 2:
            return None, None
        if coupled and coupled[0].flow.shape[0] != N // chunks - 1:
            return None, None                      # (plan_fusion will raise on it: leave the whole batch to say so)
        key = (N, chunks)
        plan = self._split_state.get(("plan",) + key)
        if plan is None:
            F_ = N // chunks
            plan = [torch.tensor([c * F_ + f for c in range(chunks) for f in range(lo, hi)], dtype=torch.int64, device=self.device)
                    for lo, hi in ((0, F_ // 2), (F_ // 2, F_))]
            self._split_state[("plan",) + key] = plan
        return plan, coupled or None

    def _concurrent_stream_pair(self):
        """Two side streams whose launches really overlap: a spin kernel on each, timed together and alone -- a pair that shares a
        hardware queue takes twice as long together and is replaced (three tries; then the pair is kept, and the halves simply run
        one after the other on it)."""
        pair = None
        for _ in range(3):
            pair = [torch.cuda.Stream(), torch.cuda.Stream()]
            cur = torch.cuda.current_stream()
            spin = 300_000          # 0.15 ms at core clock (3 ms if the counter is the 100 MHz timer): long against a launch, short once per engine

            def spin_on(streams):
                for s in streams:
                    s.wait_stream(cur)
                    with torch.cuda.stream(s):
                        torch.cuda._sleep(spin)
                for s in streams:
                    cur.wait_stream(s)
            timed = lambda streams: _timed(cur, lambda: spin_on(streams))[0]
            try:
                timed(pair)
                one, both = timed(pair[:1]), timed(pair)
            except Exception:      # (no spin kernel in this torch build: keep the pair untested)
                break
            if both < 1.5 * one:
                break
        return pair

    def _step_forward_split(self, x: Act, timesteps: torch.Tensor, context: torch.Tensor, plan, coupled=None, timing=False) -> torch.Tensor:
        """Two launch streams (VFACE_STREAMS=2, the default): a graph-replayed forward whose frames are not coupled across the split
        (no hook, or replace / fft / mix: every edit stays inside a frame's own chunks; ``coupled``: flow_fix, _split_coupled_halves) runs
        as two half-batches -- frames [0, F/2) and [F/2, F) of every chunk, ``plan`` -- on two HIP streams at once, each with its own
        hipGraph and split-K scratch, joined on the calling stream.  The kernels that own a whole CU per workgroup run their HBM
        phases in lock-step across the chip; two independent launch sequences put one half's HBM-bound launches beside
        the other's matrix-bound ones.  Every kernel is batch-invariant, so the halves' results are the full batch's bit for bit
        (tests); measured 1-4.5 % per step depending on the box (profiles/r04_n).  The SECOND split step of every kind ("coupled" /
        "free") at a shape also checks and times the form; ``timing``: one of that timing's own replays, which does neither."""
        cur = torch.cuda.current_stream()
        st = self._split_buffers(x, timesteps, context, plan, cur)
        kind = "coupled" if coupled else "free"
        calls = st["calls_by_kind"][kind] = st["calls_by_kind"].get(kind, 0) + 1
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(6)] if calls == 2 and not self._split_verified else None
        if ev is not None:
            ev[0].record(cur)
        halves = self._split_coupled_halves(st, coupled) if coupled else None
        outs = self._split_run_halves(st, x, plan, coupled, halves, cur, ev)
        if ev is not None:
            self._split_probe_verdict(ev, cur)
        if st["eps"] is None or st["eps"].shape[1] != outs[0].shape[1]:
            st["eps"] = torch.empty(x.M, outs[0].shape[1], dtype=outs[0].dtype, device=self.device)
        eps, rows = st["eps"], st["eps"].view(x.N, -1)
        for idx, o in zip(plan, outs):      # gather the halves' rows
            o.record_stream(cur)
            rows.index_copy_(0, idx, o.reshape(len(idx), -1))
        if timing or not self.split_selfcheck or calls != 2:
            return eps
        if kind not in self.split_checked:
            whole = self._split_bit_check(kind, x, timesteps, context, eps)
            if whole is not None:
                return whole
        # (the timing is skipped where the extra graph would crowd the graph cache: the whole batch's pool ~ the two halves' together)
        tkey = (kind, x.N, x.H, x.W)
        if tkey not in self.split_timing and 4 * sum(v["bytes"] for v in self._graphs.values()) <= self.graph_budget_bytes:
            return self._split_time_both(tkey, x, timesteps, context, plan, coupled, cur)
        return eps

    def _split_buffers(self, x: Act, timesteps: torch.Tensor, context: torch.Tensor, plan, cur) -> dict:
        """The shape's state: the stream pair, the halves' context slices and their x / t buffers, filled with this step's rows."""
        N, hw, C = x.N, x.H * x.W, x.t.shape[1]
        skey = (N, x.H, x.W, C, x.t.dtype, tuple(context.shape[1:]), cur.cuda_stream, len(plan[0]))
        st = self._split_state.get(skey)
        if st is None:
            # ONE pair of side streams per engine, created back to back: HIP maps streams onto a few hardware queues round-robin
            # in creation order, and two streams that land on the same queue run their launches one after the other (measured: a
            # pair created later, for another configuration, shared a queue -- 24.2 instead of 16.3 ms per inversion step)
            if self._split_pair is None:
                self._split_pair = self._concurrent_stream_pair()
            st = self._split_state[skey] = {
                "streams": self._split_pair, "ctx_id": None, "ctx": None, "ctx_keep": None, "calls_by_kind": {},
                "x": [torch.empty(len(i) * hw, C, dtype=x.t.dtype, device=self.device) for i in plan],
                "t": [torch.empty(len(i), dtype=torch.int64, device=self.device) for i in plan], "eps": None}
        cid = (id(context), context._version)
        if st["ctx_id"] != cid:
            # (stable tensor objects per half: the graphs' and the eager path's context caches key on identity)
            st["ctx"] = [context.index_select(0, i).contiguous() for i in plan]
            st["ctx_id"], st["ctx_keep"] = cid, context
        ts = timesteps.to(device=self.device, dtype=torch.int64)
        xv = x.t.reshape(x.N, -1)
        for h, idx in enumerate(plan):
            torch.index_select(xv, 0, idx, out=st["x"][h].view(len(idx), -1))
            torch.index_select(ts, 0, idx, out=st["t"][h])
        return st

    def _split_coupled_halves(self, st: dict, coupled) -> list:
        """flow_fix: the halves as two in-process frame shards (parallel.StreamShard).  Per half: its own exchange object, the flow
        fields between ITS frames, and -- half 1 -- the field from half 0's last frame into its first.  The slices are kept
        (one object per flow tensor and half): the graphs' private flow copies are refreshed by tensor identity."""
        fl = coupled[0].flow
        F_all = fl.shape[0] + 1
        fkey = (id(fl), fl._version)
        if st.get("flow_key") != fkey:
            st["flow_key"], st["flow_keep"] = fkey, fl
            st["flow_slices"] = [fl[:F_all // 2 - 1], fl[F_all // 2:]]
            st["flow_halo"] = fl[F_all // 2 - 1]
        if "shard_objs" not in st:
            shared = {}
            st["shard_objs"] = [StreamShard(h, 2, F_all, shared) for h in range(2)]
        return [(st["shard_objs"][h], st["flow_slices"][h] if st["flow_slices"][h].shape[0] else None,
                 st["flow_halo"] if h else None) for h in range(2)]

    def _split_run_halves(self, st: dict, x: Act, plan, coupled, halves, cur, ev) -> list:
        """Fork: each half's forward on its side stream and in its own split-K workspace domain (coupled: as the frame shard ``halves[h]``,
        the engine's exchange attributes and the cfgs' flow restored afterwards); join on ``cur``.  ``ev``: the overlap probe's events, or None."""
        from .engine import Act
        outs = []
        flows = [(c, c.flow) for c in (coupled or [])]
        saved = set_boundary(self)      # (no exchange is installed on an engine that splits: _split_decide)
        try:
            for h, idx in enumerate(plan):
                s = st["streams"][h]
                s.wait_stream(cur)
                if halves is not None:
                    shard, lflow, hflow = halves[h]
                    set_boundary(self, shard, hflow, flows[0][1].shape[-2:])
                    for c, _ in flows:
                        c.flow = lflow
                with torch.cuda.stream(s), hip.workspace_domain(h + 1):
                    if ev is not None:
                        ev[1 + 2 * h].record(s)
                    outs.append(self._step_forward_one(Act(st["x"][h], len(idx), x.H, x.W), st["t"][h], st["ctx"][h]))
                    if ev is not None:
                        ev[2 + 2 * h].record(s)
        finally:
            set_boundary(self, *saved)
            for c, f in flows:
                c.flow = f
        for s in st["streams"]:
            cur.wait_stream(s)
        return outs

    def _split_probe_verdict(self, ev, cur) -> None:
        """Once per engine, on the second split step (graphs captured by the first), the overlap is MEASURED on the real work: events
        around each half and around the fork / join.  Halves that run at once each take about as long as the whole step
        (total / (t_A + t_B) ~ 0.5); halves that were put on one hardware queue run back to back (~ 1.0, and a half-batch sequence
        alone is 30 % less efficient than the full batch): then the engine goes back to one launch sequence for good."""
        ev[5].record(cur)
        ev[5].synchronize()
        total, ta, tb = ev[0].elapsed_time(ev[5]), ev[1].elapsed_time(ev[2]), ev[3].elapsed_time(ev[4])
        self._split_verified = True
        self.split_overlap = total / max(ta + tb, 1e-6)
        if self.split_overlap > 0.8:
            warnings.warn(f"vface_amd: the two launch streams do not overlap on this device (step {total:.2f} ms, halves {ta:.2f} + "
                          f"{tb:.2f} ms): back to one launch sequence")
            self.split_streams = 1

    def _split_bit_check(self, kind: str, x: Act, timesteps: torch.Tensor, context: torch.Tensor, eps: torch.Tensor):
        """Self-check of the two-sequence form: the SECOND split step of every split configuration kind ("free": halves
        that never read each other; "coupled": flow_fix's halves handing one frame over, parallel.StreamShard) is also run as ONE
        launch sequence over the whole batch and the two eps compared bit for bit (one extra forward per kind and engine).  A
        mismatch -- round 4 / 5: a kernel of one half mis-executing beside the other half's attention waves -- makes the engine
        return the single sequence's result (None: the bits agree) and stay on one launch sequence for good."""
        whole = self._step_forward_one(x, timesteps, context)
        same = self.split_checked[kind] = bool(torch.equal(whole, eps))
        if not same:
            warnings.warn(f"vface_amd: the two launch sequences ({kind} halves) did NOT reproduce the single sequence's bits on this "
                          "device: back to one launch sequence")
            self.split_streams = 1
        return None if same else whole

    def _split_time_both(self, tkey, x: Act, timesteps: torch.Tensor, context: torch.Tensor, plan, coupled, cur) -> torch.Tensor:
        """Whether two launch sequences beat one depends on the batch, the hook mode and the box: coupled (flow_fix) halves wait for each
        other at every hooked flow layer (round 6: 16 frames 38.0 vs 38.5 ms, 32 frames 78.0 vs 74.2), and since the launch rules follow
        the 48-sample half batch and the shared block issues its tail twice, free halves no longer win everywhere either (32 frames fft,
        same box: 75.3 vs 74.4-75.0 as one sequence; round 4-5: two sequences won by 1-4 %).  So on the second split step of every (kind,
        batch, resolution) BOTH forms are timed -- two replays each, the whole batch's graph captured for it -- and the configuration
        keeps the faster one (the single sequence only if it wins by more than 0.5 %).  Returns the split form's eps."""
        split = lambda: self._step_forward_split(x, timesteps, context, plan, coupled, timing=True)
        self._step_forward_one(x, timesteps, context)                    # (captures the whole batch's graph if the bit check did not)
        t_whole = min(_timed(cur, lambda: self._step_forward_one(x, timesteps, context))[0] for _ in range(2))
        t_split, eps = _timed(cur, split)
        t_split = min(t_split, _timed(cur, split)[0])
        self.split_timing[tkey] = (t_split, t_whole)
        if t_whole < 0.995 * t_split:
            self._split_off.add(tkey)
        return eps

    def step_forward_nhwc(self, x: Act, timesteps: torch.Tensor, context: torch.Tensor) -> torch.Tensor:
        """``forward_nhwc`` for the DDIM loop; with two launch streams (``split_streams``) and a batch whose frames are not
        coupled, the two frame halves through ``_step_forward_one`` at once."""
        if self.use_graph and x.t32 is None and x.t.is_contiguous():
            plan, coupled = self._split_decide(x.N)
            if plan is not None and ("coupled" if coupled else "free", x.N, x.H, x.W) not in self._split_off:
                return self._step_forward_split(x, timesteps, context, plan, coupled)
        return self._step_forward_one(x, timesteps, context)

    def _step_forward_one(self, x: Act, timesteps: torch.Tensor, context: torch.Tensor) -> torch.Tensor:
        """``forward_nhwc`` for the DDIM loop: with ``use_graph`` the launch sequence of one forward is captured into a
        hipGraph the first time a (batch, resolution, hook configuration) combination is seen and replayed afterwards -- the
        same kernels on the same buffers, one host call per step instead of ~1200 (ddim_w_inv.py:299-305 calls the UNet once
        per step with nothing but x and t changing).  What changes between steps or clips is copied into the graph's own
        input buffers: x, t every step; the context projections and the flow fields when a new clip brings new tensors.
        The returned eps is the graph's output buffer: consume it before the next call.
        A frame-sharded engine (``halo_exchange`` installed: RCCL point-to-point exchange inside the forward) is captured as
        graph SEGMENTS cut at the exchange calls -- [.. fused q|k of chunk 1] send/recv [projections it overlaps] wait
        [warp, attention, .. next hooked layer ..] -- with the two ``isend/irecv`` + ``wait`` pairs issued from the host between
        segment replays (5 segments and 4 host calls per step instead of ~1200 launches).  A capture failure (or a pool
        over the byte budget) runs the eager path for that configuration -- decided ONCE for all ranks of a sharded clip
        (``Exchange.agree``), the failing rank first completing the exchanges its aborted pass owed its neighbours
        (``Exchange.drain``), and the capturing call returns the warm-up forward's eps instead of running a further forward."""
        if not self.use_graph or x.t32 is not None:
            return self.forward_nhwc(x, timesteps, context)
        self._ensure_packed()
        sig, flows = self._hook_signature()
        ex = self.halo_exchange
        # (an exchange object that is moved along the batches of a clip, parallel.ClipCarry, says itself what of its position a
        #  captured forward depends on: batches of one shape then replay one capture)
        shard_sig = None if ex is None else (ex.graph_signature() +
                                             (self.halo_hw, None if self.halo_flow is None else tuple(self.halo_flow.shape)))
        key = (x.N, x.H, x.W, tuple(x.t.shape), x.t.dtype, self._version, *(getattr(self, a) for a in self._GRAPH_SWITCHES),
               hip._ws_domain, self.exchange_events is not None, sig,
               tuple(context.shape), torch.cuda.current_stream().cuda_stream, shard_sig)
        g = self._graphs.get(key)
        if g is None:
            if key in self._graph_failed:
                return self.forward_nhwc(x, timesteps, context)
            g = self._capture(key, x, timesteps, context, flows)
            if "eps_only" in g:
                # no graph for this configuration (capture failed or over budget, on this rank or -- sharded -- on any rank of
                # the clip: one decision for all).  The warm-up forward already computed this call's eps from the same inputs;
                # a second forward here would issue exchanges the other ranks do not make.
                return g["eps_only"]
        else:
            self._graphs[key] = self._graphs.pop(key)      # most recently used last
        cid = (id(context), context._version)
        if cid != g["ctx_id"]:
            g["a2"].copy_(self.context_projections(context, x.N))
            g["ctx_id"], g["ctx_keep"] = cid, context
        for dst, src in zip(g["flows"], flows):
            if (id(src), src._version) != g["flow_ids"].get(id(dst)):
                dst.copy_(src)
                g["flow_ids"][id(dst)] = (id(src), src._version)
                g["flow_keep"][id(dst)] = src
        if g["halo_flow"] is not None and (id(self.halo_flow), self.halo_flow._version) != g["halo_flow_id"]:
            g["halo_flow"].copy_(self.halo_flow)      # (the graph reads its own copy: FrameShard.install may hand a new tensor)
            g["halo_flow_id"], g["halo_flow_keep"] = (id(self.halo_flow), self.halo_flow._version), self.halo_flow
        g["x"].copy_(x.t)
        g["t"].copy_(timesteps)
        for graph, host_op in g["segments"]:
            if graph is not None:
                graph.replay()
            if host_op is not None:
                host_op()
        return g["eps"]

    def _capture(self, key, x: Act, timesteps: torch.Tensor, context: torch.Tensor, flows):
        from .engine import Act
        xs = torch.empty_like(x.t)
        ts = timesteps.to(device=self.device, dtype=torch.int64).clone()
        xs.copy_(x.t)
        # The graph reads two kinds of buffers that are not produced inside it: the context projections and the flow fields.
        # It gets PRIVATE copies of both (refreshed in place when a later clip brings other tensors), so neither the caller's
        # flow tensors nor the eager path's context cache are ever written to.
        cfgs = []
        for cfg in self._hooked_cfgs():
            if cfg is not None and cfg.flow is not None and not any(c is cfg for c in cfgs):
                cfgs.append(cfg)
        own_flows = [f.clone() for f in flows]
        saved_flows = [c.flow for c in cfgs]
        saved_cache = self._a2_cache
        real_exchange, real_halo_flow = self.halo_exchange, self.halo_flow
        own_halo_flow = real_halo_flow.clone() if (real_exchange is not None and real_halo_flow is not None) else None
        seg, eps_warm, counting, ok, pool_bytes = None, None, None, True, 0
        saved = set_boundary(self, real_exchange, real_halo_flow if own_halo_flow is None else own_halo_flow, self.halo_hw)
        try:
            a2 = self.context_projections(context, x.N).clone()
            self._a2_cache = (context, context._version, self._packed, a2)
            for c in cfgs:
                c.flow = own_flows[next(i for i, f in enumerate(flows) if f is c.flow)]
            # warm-up on a side stream (the documented capture recipe): fills the folded-weight caches, sets every kernel's
            # shared-memory attribute, and brings the allocator to its steady state.  (Sharded: a real forward with real
            # exchanges -- every rank of the clip captures at the same step, so the calls pair up.)
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            if real_exchange is not None:
                counting = self.halo_exchange = _CountingExchange(real_exchange)
            with torch.cuda.stream(side):
                eps_warm = self.forward_nhwc(Act(xs, x.N, x.H, x.W), ts, context)
            torch.cuda.current_stream().wait_stream(side)
            if os.environ.get("VFACE_TEST_FAIL_CAPTURE") == "warmup_done":      # (test hook: a capture that dies before its pass)
                raise RuntimeError("injected capture failure (VFACE_TEST_FAIL_CAPTURE)")
            # the captured launches write to the split-K workspace / read the zero page that exist NOW: the warm-up above must
            # have grown them to their final size (hip.py grows by REPLACING the tensor)
            fixed = lambda: [{k: v.data_ptr() for k, v in d.items()} for d in (hip._splitk_ws, hip._zeros)]
            before = fixed()
            gc.collect()                             # (before mem0: what it frees is not part of this capture's pool)
            torch.cuda.synchronize()
            mem0 = torch.cuda.memory_allocated(self.device)
            seg = _GraphSegments(self, real_exchange)
            if real_exchange is not None:
                self.halo_exchange = seg             # start_exchange / finish_exchange cut the capture (see _GraphSegments)
                real_exchange.capture_pass(True)     # (the slabs this pass hands over hold no data: Exchange.capture_pass)
            # No garbage collection inside the capture pass: a cycle collected there can release device objects of an earlier
            # configuration (its graphs, their pool, events), and releasing them while this thread captures is a fatal runtime
            # error, not a Python exception.  Collected above, as ``torch.cuda.graph`` does; the collector stays off until the end.
            gc_was_on = gc.isenabled()
            gc.disable()
            try:
                with torch.cuda.stream(seg.stream):
                    seg.begin()
                    eps = self.forward_nhwc(Act(xs, x.N, x.H, x.W), ts, context)
                    seg.end(None)
            finally:
                if gc_was_on:
                    gc.enable()
            torch.cuda.current_stream().wait_stream(seg.stream)
            pool_bytes = max(0, torch.cuda.memory_allocated(self.device) - mem0)
            if fixed() != before:
                raise RuntimeError("the split-K workspace / zero page was re-allocated during capture (warm-up did not reach the steady state)")
        except Exception as e:  # capture is an optimisation of the same launch sequence: the eager path is the same code
            if seg is not None:
                seg.abort()
            if eps_warm is None:
                raise            # the warm-up forward itself failed: the eager path is the same code and would fail the same way
            warnings.warn(f"vface_amd: hipGraph capture of the UNet forward failed ({type(e).__name__}: {e}); "
                          "this configuration runs kernel by kernel")
            ok = False
            if real_exchange is not None:
                # the other ranks of the clip are in (or past) their capture pass, which exchanges for real: finish the
                # exchanges this rank's aborted pass still owes them, so every rank has made the same number of calls
                st = seg.pending if seg is not None else None
                done = seg.n_started if seg is not None else 0
                real_exchange.drain(st.pop("h", None) if st else None, counting.tails[done:])
        finally:
            set_boundary(self, *saved)
            if real_exchange is not None:
                real_exchange.capture_pass(False)
            for c, f in zip(cfgs, saved_flows):
                c.flow = f
            self._a2_cache = saved_cache
        over = ok and pool_bytes > self.graph_budget_bytes      # one forward larger than the whole budget: do not pin it
        if real_exchange is not None:
            # ONE decision for the ranks of a clip (pool_bytes follows each rank's own frame count): a rank that replays
            # segments and a rank that launches eagerly would still pair, but a rank that RE-RUNS the forward would not
            all_ok, any_over = real_exchange.agree(ok, over)
            ok, over = all_ok, any_over
        if not ok or over:
            self._graph_failed.add(key)
            seg = None
            return {"eps_only": eps_warm}
        while self._graphs and (len(self._graphs) >= self.graph_capacity or
                                sum(v["bytes"] for v in self._graphs.values()) + pool_bytes > self.graph_budget_bytes):
            self._graphs.pop(next(iter(self._graphs)))      # least recently used first
        g = {"segments": seg.segments, "keep": seg.keep, "bytes": pool_bytes, "x": xs, "t": ts, "eps": eps, "a2": a2,
             "ctx_id": (id(context), context._version),
             "halo_flow": own_halo_flow, "halo_flow_keep": real_halo_flow,
             "halo_flow_id": None if own_halo_flow is None else (id(real_halo_flow), real_halo_flow._version),
             "ctx_keep": context, "flows": own_flows, "flow_ids": {id(d): (id(s_), s_._version) for d, s_ in zip(own_flows, flows)},
             "flow_keep": {id(d): s_ for d, s_ in zip(own_flows, flows)}, "packed": self._packed,
             # the split-K workspace the captured launches write to (hip.py grows it by REPLACING the tensor: keep this one alive)
             "splitk_ws": dict(hip._splitk_ws), "zeros": dict(hip._zeros)}
        self._graphs[key] = g
        return g
