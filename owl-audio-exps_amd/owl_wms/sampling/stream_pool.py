"""Many streaming sessions in one batch (the reference's inference/causvid_pipeline.py:112-163 serves one
session per pipeline and set of weights): ``StreamPool`` is ``FrameStream`` for ``n_slots`` independent
sessions of the video core (GameRFTCore on the DiT) that arrive and leave at different times and share every
forward.

The pool owns a ``SlotRingKVCache``: K/V rings ``[n_slots, cap, H D]`` (``2 n_slots`` batch rows
``[cond | uncond]`` with CFG) allocated once, and one device state ``[n_slots, 4]``, row s = {start, cached
tokens, rope offset, live}.  The slot forms of the ring kernels (``owlk_qk_rope_fwd_kv_ring_slots``,
``owlk_attn_decode_ring_slots_fwd``, ``owlk_ring_advance_slots``) read row ``b mod n_slots`` for batch row b, so
each session has its own window, wraps and RoPE positions; an idle slot rides along with zero inputs, reads no
cache row and gets finite rows it never sees.  A tick is FrameStream's frame on the fixed ``n_slots`` batch:
Euler steps, the finished frames copied out, the re-noise, the forward that writes the frames' rows, the
advance of every live row on the device.  ``graphed`` False / True / "frame" as FrameStream: one captured
Euler step, or the whole tick as one graph; the live flags and positions are read on the device, so opening,
closing, wrapping and rebasing never recapture, and the three modes give the same bits.

Noise: a session owns a device ``torch.Generator`` seeded at ``open``; its draws are a B = 1 FrameStream's in
shape and order (the context zlerp, then per frame the start noise and the re-noise), made outside the graph.
A session's sample therefore depends neither on its neighbours nor on its slot number.  Rebase is per slot
and host-driven (``SlotRingKVCache.rebase``: ``owlk_rope_rebase`` on the slot's batch rows, then the slot's
state row rewritten between replays).
"""
import torch

from ..nn.attn import check_rope_rows
from ..nn.kv_cache import SlotRingKVCache
from .schedulers import euler_dt, renoise
from .step_graph import FrameGraph
from .stream import FrameStream


class StreamPool(FrameStream):
    """``open(x, mouse, btn, seed) -> slot``, ``step({slot: (mouse_1, btn_1)}) -> {slot: frame}``,
    ``close_slot(slot)``, ``close()``; FrameStream's arguments and checks plus ``n_slots``."""

    def __init__(self, core, n_slots: int, n_steps: int = 16, cfg_scale: float = 1.3, noise_prev: float = 0.2,
                 max_cached_frames: int = 120, custom_schedule=None, graphed=False, ring_frames=None) -> None:
        super().__init__(core, n_steps, cfg_scale, noise_prev, max_cached_frames, custom_schedule, graphed,
                         ring_frames)
        if not isinstance(n_slots, int) or isinstance(n_slots, bool) or n_slots < 1:
            raise ValueError(f"StreamPool: n_slots must be a positive integer; got {n_slots!r}")
        self.n_slots = n_slots
        cfg = core.config
        device = next(core.parameters()).device
        self.kv_cache = SlotRingKVCache(cfg, self.ring_frames * cfg.tokens_per_frame, n_slots,
                                        2 * n_slots if self._cfg() else n_slots, rope=core.transformer.rope,
                                        device=device)
        self.frames_generated = [0] * n_slots
        self.rebases = [0] * n_slots
        self.ticks = 0
        self._gens = [None] * n_slots
        # a tick's named inputs over all n_slots rows (x0 start noise, z0 re-noise draws, t ones, the controls),
        # created once the first session fixed the shapes and written in place per tick: only the live slots'
        # rows of x0 / z0 / mouse / btn change, an idle slot's rows are zero
        self._in = None

    @property
    def live(self):
        """the live slots, ascending"""
        return self.kv_cache.live_slots()

    def start(self, *a, **k):
        raise RuntimeError("StreamPool: sessions are opened one at a time with open(x, mouse, btn, seed)")

    # ------------------------------------------------------------------ sessions
    @torch.no_grad()
    def open(self, x, mouse, btn, seed):
        """A new session from its context x [1, n, c, h, w] (1 <= n <= max_cached_frames) with controls mouse
        [1, >= n, 2], btn [1, >= n, n_buttons]: the lowest free slot, FrameStream.start's context pass (zlerp
        at noise_prev from the session's generator, one cache-updating forward; with CFG both halves from the
        conditioned pass) for that slot alone into that slot's rows of the rings, then its state row
        {0, n tpf, n tpf, 1}.  -> the slot."""
        cache, tpf = self.kv_cache, self.core.config.tokens_per_frame
        if x.dim() != 5 or x.size(0) != 1:
            raise ValueError(f"StreamPool.open: one session's context [1, n, c, h, w]; got {tuple(x.shape)}")
        n = x.size(1)
        if not 1 <= n <= self.max_cached_frames:
            raise ValueError(f"StreamPool.open: {n} context frames do not fit max_cached_frames = "
                             f"{self.max_cached_frames}")
        if self._in is not None and (x.shape[2:] != self._in["x0"].shape[2:] or x.dtype != self._in["x0"].dtype):
            raise ValueError(f"StreamPool.open: frames of shape {tuple(x.shape[2:])} / {x.dtype} in a pool of "
                             f"{tuple(self._in['x0'].shape[2:])} / {self._in['x0'].dtype}")
        slot = cache.free_slot()
        if slot is None:
            raise RuntimeError(f"StreamPool.open: all {self.n_slots} slots are live")
        if self._in is None:
            x0 = x.new_zeros(self.n_slots, 1, *x.shape[2:])
            self._like = (x0,)
            self._in = {"x0": x0, "z0": torch.zeros_like(x0), "t": x.new_ones(self.n_slots, 1),
                        **self._controls(mouse.new_zeros(self.n_slots, 1, mouse.size(2)),
                                         btn.new_zeros(self.n_slots, 1, btn.size(2)))}
            self._dt = euler_dt(self.n_steps, self.custom_schedule, x)
        gen = torch.Generator(device=x.device)
        gen.manual_seed(int(seed))
        self._gens[slot] = gen
        z = torch.randn(x.shape, generator=gen, device=x.device, dtype=x.dtype)
        noisy = renoise(x, z, self.noise_prev)  # zlerp with the session's draw
        ts = x.new_full((1, n), self.noise_prev)
        view = cache.slot_view(slot)
        view.enable_cache_updates()
        self._forward(view, (noisy,), ts, mouse[:, :n], btn[:, :n])
        assert all(view.start[i] == 0 and view.len[i] == n * tpf for i in range(len(view.len)))
        cache.open_slot(slot, n * tpf)
        self.frames_generated[slot] = 0
        self.rebases[slot] = 0
        return slot

    def close_slot(self, slot):
        """The session leaves: the slot goes idle on host and device and a later open() may take it.  Its
        rows stay in the rings and are never read again (a new session's window starts with its own rows)."""
        if not (isinstance(slot, int) and 0 <= slot < self.n_slots and self.kv_cache.live[slot]):
            raise ValueError(f"StreamPool.close_slot: slot {slot!r} is not live")
        self.kv_cache.close_slot(slot)
        self._gens[slot] = None
        for k in ("x0", "z0", "mouse", "btn"):  # the idle slot rides along with zero inputs
            self._in[k][slot].zero_()

    def close(self, check=True):
        """Release the captured step or tick, then compare every slot's device state row with its host
        mirror (in every mode: the position moves on the device alone)."""
        if self._step_graph is not None:
            self._step_graph.release()
        self._step_graph = None
        cache = self.kv_cache
        if check and cache is not None and cache.dev.is_cuda:
            dev, host = cache.device_state(), cache.host_state()
            if dev != host:
                raise RuntimeError(f"StreamPool: the slots' state rows on the device (start, cached, offset, live) = "
                                   f"{dev} differ from the host mirror {host} after {self.ticks} ticks; a count of "
                                   "-1 marks a state the ring kernels refused to follow")

    # ------------------------------------------------------------------ one tick
    def _rebase_if_needed(self, slot):
        """FrameStream's rule for one slot: before a tick on which its rows would pass the RoPE table its
        cached K is re-rotated so that its oldest live key sits at position 0; other slots are untouched."""
        core, cache = self.core, self.kv_cache
        rope, tpf = core.transformer.rope, core.config.tokens_per_frame
        off = cache.offsets[slot]
        if off + tpf <= rope.cos.shape[0]:
            return
        impl = str(getattr(core.config, "rope_impl", "ortho")).lower()
        if impl not in self.rebase_ropes:
            raise RuntimeError(f"StreamPool: frame {self.frames_generated[slot]} of slot {slot} would pass the "
                               f"{rope.cos.shape[0]}-row RoPE table and rope_impl {impl!r} cannot be rebased by "
                               f"this stream; it rebases {self.rebase_ropes}")
        cache.rebase(slot, off - cache.len[slot], rope)
        self.rebases[slot] += 1

    @torch.no_grad()
    def step(self, controls):
        """One new frame for every live slot: controls {slot: (mouse_1 [1, 1, 2], btn_1 [1, 1, n_buttons])} for
        exactly the live slots -> {slot: frame [1, 1, c, h, w]}.  One batched forward per Euler step over all
        n_slots rows; idle slots ride along with zero inputs."""
        core, cache = self.core, self.kv_cache
        live = cache.live_slots()
        if set(controls) != set(live):
            raise ValueError(f"StreamPool.step: controls for slots {sorted(controls)}, live slots {live}: every live "
                             "slot needs controls and no idle slot takes any")
        if not live:
            return {}
        tpf = core.config.tokens_per_frame
        for s in live:
            self._rebase_if_needed(s)
        # the positions the replayed graph reads on the device, checked per live slot as an eager forward does
        for s in live:
            check_rope_rows(core.transformer.rope, cache.offsets[s], tpf)
        tick = self._in
        for s in live:  # a B = 1 FrameStream's draws, in its order, from the session's generator
            for k in ("x0", "z0"):
                row = tick[k][s:s + 1]
                torch.randn(row.shape, generator=self._gens[s], out=row)
            tick["mouse"][s:s + 1].copy_(controls[s][0])
            tick["btn"][s:s + 1].copy_(controls[s][1])
        ctrl = {k: v for k, v in tick.items() if k not in ("x0", "z0", "t")}
        core.transformer.enable_decoding()
        try:
            if self.graphed == "frame" and self.ticks > 0:
                # tick 0 ran eagerly (bf16 weight copies, workspaces outside the graph pool); tick 1 captures,
                # and the graph's static buffers become the pool's inputs: no copy-in from then on
                fg = self._step_graph
                if fg is None:
                    if self._pool is None:
                        self._pool = torch.cuda.graph_pool_handle()
                    fg = self._step_graph = FrameGraph(self._frame, tick, self._pool)
                    self._in = fg.bufs
                fg.replay()
                cache.advance(tpf, self.max_cached_frames * tpf, device=False)
                self.graph_replays += 1
                frame = fg.outputs()[0]
            elif self.graphed is True:
                xs, t = self._denoise((tick["x0"],), tick["t"], ctrl)
                frame = self._commit_frame(xs, t, (tick["z0"],), ctrl)[0]
            else:
                frame = self._frame(tick)[0]
        finally:
            core.transformer.disable_decoding()
        self.ticks += 1
        for s in live:
            self.frames_generated[s] += 1
        return {s: frame[s:s + 1] for s in live}  # views of this tick's own copy of the frames
