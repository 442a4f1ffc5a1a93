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

``AVStreamPool`` / ``AVDiTStreamPool`` are the same for the audio + video core (GameRFTAudioCore) on the MMDiT
and on the plain DiT: ``AVFrameStream`` / ``AVDiTFrameStream`` for ``n_slots`` sessions, 65-row joint frames on
the slot forms of the joint-frame kernels (``owlk_mm_qk_rope_fwd_kv_ring_slots``,
``owlk_attn_decode_joint_ring_slots_fwd``) and of the wide decode attention
(``owlk_attn_decode_wide_ring_slots_fwd``).  A session's draws are a B = 1 audio + video stream's: context
video, context audio, then per tick video noise, audio noise, video re-noise, audio re-noise.  The three pools
share ``_SlotPool``, which is written over a tuple of latents as ``_RingStream`` is.
"""
import torch

from ..nn.attn import check_rope_rows
from ..nn.kv_cache import SlotRingKVCache
from .schedulers import euler_dt, renoise
from .step_graph import FrameGraph
from .stream import AVDiTFrameStream, AVFrameStream, FrameStream


class _SlotPool:
    """What the pools share, over a tuple of latents ((x,) for video, (video, audio) for audio + video): mixed
    in front of the B = 1 stream class whose frame the pool batches (its constructor checks, _forward, _guided,
    _controls, ``decoding`` and ``rebase_ropes``).  A subclass supplies its constructor (the stream's arguments
    plus ``n_slots``, then _init_pool), open() / start() with its own signature, and how a slot's frame is
    handed out (_slot_frame)."""

    def _init_pool(self, n_slots):
        name, core = type(self).__name__, self.core
        if not isinstance(n_slots, int) or isinstance(n_slots, bool) or n_slots < 1:
            raise ValueError(f"{name}: n_slots must be a positive integer; got {n_slots!r}")
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
        # a tick's named inputs over all n_slots rows (x{i} start noise, z{i} re-noise draws per latent i, t
        # ones, the controls), created once the first session fixed the shapes and written in place per tick:
        # only the live slots' rows of x{i} / z{i} / mouse / btn change, an idle slot's rows are zero
        self._in = None

    @property
    def live(self):
        """the live slots, ascending"""
        return self.kv_cache.live_slots()

    def _slot_frame(self, frames, slot):
        """what step() hands out for `slot` from the tick's frames (one [n_slots, 1, ...] tensor per latent)"""
        raise NotImplementedError

    # ------------------------------------------------------------------ sessions
    @torch.no_grad()
    def _open(self, latents, mouse, btn, seed):
        """A new session from its context latents (each [1, n, ...], 1 <= n <= max_cached_frames) with controls
        mouse [1, >= n, 2], btn [1, >= n, n_buttons]: the lowest free slot, the B = 1 stream's context pass
        (each latent zlerp-ed at noise_prev with a draw from the session's generator, in tuple order; one
        cache-updating forward) for that slot alone into that slot's rows of the rings, then its state row
        {0, n tpf, n tpf, 1}.  -> the slot."""
        name, cache, tpf = type(self).__name__, self.kv_cache, self.core.config.tokens_per_frame
        x = latents[0]
        n = x.size(1)
        if not 1 <= n <= self.max_cached_frames:
            raise ValueError(f"{name}.open: {n} context frames do not fit max_cached_frames = "
                             f"{self.max_cached_frames}")
        if self._in is not None:
            for i, l in enumerate(latents):
                like = self._in[f"x{i}"]
                if l.shape[2:] != like.shape[2:] or l.dtype != like.dtype:
                    raise ValueError(f"{name}.open: frames of shape {tuple(l.shape[2:])} / {l.dtype} in a pool of "
                                     f"{tuple(like.shape[2:])} / {like.dtype}")
        slot = cache.free_slot()
        if slot is None:
            raise RuntimeError(f"{name}.open: all {self.n_slots} slots are live")
        if self._in is None:
            self._like = tuple(l.new_zeros(self.n_slots, 1, *l.shape[2:]) for l in latents)
            self._in = {**{f"x{i}": l for i, l in enumerate(self._like)},
                        **{f"z{i}": torch.zeros_like(l) for i, l in enumerate(self._like)},
                        "t": x.new_ones(self.n_slots, 1),
                        **self._controls(mouse.new_zeros(self.n_slots, 1, mouse.size(2)),
                                         btn.new_zeros(self.n_slots, 1, btn.size(2)))}
            self._dt = euler_dt(self.n_steps, self.custom_schedule, x)
        gen = torch.Generator(device=x.device)
        gen.manual_seed(int(seed))
        self._gens[slot] = gen
        # zlerp with the session's draws
        noisy = tuple(renoise(l, torch.randn(l.shape, generator=gen, device=l.device, dtype=l.dtype), self.noise_prev)
                      for l in latents)
        ts = x.new_full((1, n), self.noise_prev)
        view = cache.slot_view(slot)
        view.enable_cache_updates()
        self._forward(view, noisy, ts, mouse[:, :n], btn[:, :n])
        assert all(view.start[i] == 0 and view.len[i] == n * tpf for i in range(len(view.len)))
        cache.open_slot(slot, n * tpf)
        self.frames_generated[slot] = 0
        self.rebases[slot] = 0
        return slot

    def _draw_keys(self):
        """the per-slot noise inputs of a tick, in a B = 1 stream's draw order"""
        return [f"{c}{i}" for c in "xz" for i in range(len(self._like))]

    def close_slot(self, slot):
        """The session leaves: the slot goes idle on host and device and a later open() may take it.  Its
        rows stay in the rings and are never read again (a new session's window starts with its own rows)."""
        if not (isinstance(slot, int) and 0 <= slot < self.n_slots and self.kv_cache.live[slot]):
            raise ValueError(f"{type(self).__name__}.close_slot: slot {slot!r} is not live")
        self.kv_cache.close_slot(slot)
        self._gens[slot] = None
        for k in (*self._draw_keys(), "mouse", "btn"):  # the idle slot rides along with zero inputs
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
                raise RuntimeError(f"{type(self).__name__}: the slots' state rows on the device (start, cached, "
                                   f"offset, live) = {dev} differ from the host mirror {host} after {self.ticks} "
                                   "ticks; a count of -1 marks a state the ring kernels refused to follow")

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
            raise RuntimeError(f"{type(self).__name__}: frame {self.frames_generated[slot]} of slot {slot} would pass "
                               f"the {rope.cos.shape[0]}-row RoPE table and rope_impl {impl!r} cannot be rebased by "
                               f"this stream; it rebases {self.rebase_ropes}")
        cache.rebase(slot, off - cache.len[slot], rope)
        self.rebases[slot] += 1

    @torch.no_grad()
    def step(self, controls):
        """One new frame for every live slot: controls {slot: (mouse_1 [1, 1, 2], btn_1 [1, 1, n_buttons])} for
        exactly the live slots -> {slot: frame} (_slot_frame: [1, 1, c, h, w], or (video, audio) for an audio +
        video pool).  One batched forward per Euler step over all n_slots rows; idle slots ride along with zero
        inputs."""
        core, cache = self.core, self.kv_cache
        live = cache.live_slots()
        if set(controls) != set(live):
            raise ValueError(f"{type(self).__name__}.step: controls for slots {sorted(controls)}, live slots {live}: "
                             "every live slot needs controls and no idle slot takes any")
        if not live:
            return {}
        tpf = core.config.tokens_per_frame
        for s in live:
            self._rebase_if_needed(s)
        # the positions the replayed graph reads on the device, checked per live slot as an eager forward does
        for s in live:
            check_rope_rows(core.transformer.rope, cache.offsets[s], tpf)
        tick = self._in
        draws = self._draw_keys()
        for s in live:  # a B = 1 stream's draws, in its order, from the session's generator
            for k in draws:
                row = tick[k][s:s + 1]
                torch.randn(row.shape, generator=self._gens[s], out=row)
            tick["mouse"][s:s + 1].copy_(controls[s][0])
            tick["btn"][s:s + 1].copy_(controls[s][1])
        ctrl = {k: v for k, v in tick.items() if k not in draws and k != "t"}
        n = len(self._like)
        if self.decoding:
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
                frames = fg.outputs()
            elif self.graphed is True:
                xs, t = self._denoise(tuple(tick[f"x{i}"] for i in range(n)), tick["t"], ctrl)
                frames = self._commit_frame(xs, t, tuple(tick[f"z{i}"] for i in range(n)), ctrl)
            else:
                frames = self._frame(tick)
        finally:
            core.transformer.disable_decoding()
        self.ticks += 1
        for s in live:
            self.frames_generated[s] += 1
        return {s: self._slot_frame(frames, s) for s in live}  # views of this tick's own copy of the frames


class StreamPool(_SlotPool, FrameStream):
    """``open(x, mouse, btn, seed) -> slot``, ``step({slot: (mouse_1, btn_1)}) -> {slot: frame}``,
    ``close_slot(slot)``, ``close()``; FrameStream's arguments and checks plus ``n_slots``."""

    def __init__(self, core, n_slots: int, n_steps: int = 16, cfg_scale: float = 1.3, noise_prev: float = 0.2,
                 max_cached_frames: int = 120, custom_schedule=None, graphed=False, ring_frames=None) -> None:
        super().__init__(core, n_steps, cfg_scale, noise_prev, max_cached_frames, custom_schedule, graphed,
                         ring_frames)
        self._init_pool(n_slots)

    def start(self, *a, **k):
        raise RuntimeError("StreamPool: sessions are opened one at a time with open(x, mouse, btn, seed)")

    def open(self, x, mouse, btn, seed):
        """A new session from its context x [1, n, c, h, w] (1 <= n <= max_cached_frames) with controls mouse
        [1, >= n, 2], btn [1, >= n, n_buttons]: the lowest free slot, FrameStream.start's context pass (zlerp
        at noise_prev from the session's generator, one cache-updating forward; with CFG both halves from the
        conditioned pass) for that slot alone into that slot's rows of the rings, then its state row
        {0, n tpf, n tpf, 1}.  -> the slot."""
        if x.dim() != 5 or x.size(0) != 1:
            raise ValueError(f"StreamPool.open: one session's context [1, n, c, h, w]; got {tuple(x.shape)}")
        return self._open((x,), mouse, btn, seed)

    def _slot_frame(self, frames, slot):
        return frames[0][slot:slot + 1]


class _AVSlotPool(_SlotPool):
    """The audio + video pools: ``open(video, audio, mouse, btn, seed) -> slot``, ``step({slot: (mouse_1,
    btn_1)}) -> {slot: (video frame [1, 1, c, h, w], audio frame [1, 1, ca])}``, ``close_slot(slot)``,
    ``close()``; the B = 1 stream's arguments and _check_core refusals plus ``n_slots``.  CFG as the stream
    forms it: one batch [cond | uncond] of 2 n_slots rows, has_controls = [True] * n_slots + [False] * n_slots
    (a session's context pass: [True, False] on its two batch rows)."""

    def __init__(self, core, n_slots: int, n_steps: int = 16, cfg_scale: float = 1.3, noise_prev: float = 0.2,
                 max_cached_frames: int = 120, graphed=False, ring_frames=None) -> None:
        super().__init__(core, n_steps, cfg_scale, noise_prev, max_cached_frames, graphed, ring_frames)
        self._init_pool(n_slots)
        device = self.kv_cache.dev.device
        # has_controls of a tick (every slot) and of one session's context pass
        self._hc, self._hc_one = (torch.tensor([True] * n + [False] * n if self._cfg() else [True] * n, device=device)
                                  for n in (n_slots, 1))

    def _forward(self, cache, xs, t, mouse, btn):
        hc = self._hc if cache is self.kv_cache else self._hc_one
        return self.core(*self._rep(*xs, t, mouse, btn), has_controls=hc, kv_cache=cache)

    def start(self, *a, **k):
        raise RuntimeError(f"{type(self).__name__}: sessions are opened one at a time with open(video, audio, mouse, "
                           "btn, seed)")

    def open(self, video, audio, mouse, btn, seed):
        """A new session from its context video [1, n, c, h, w] / audio [1, n, ca] (1 <= n <= max_cached_frames)
        with controls mouse [1, >= n, 2], btn [1, >= n, n_buttons]: the lowest free slot, the stream's start()
        for that slot alone (draws: context video, context audio) into that slot's rows of the rings.  -> the
        slot."""
        if video.dim() != 5 or video.size(0) != 1 or audio.dim() != 3 or audio.shape[:2] != video.shape[:2]:
            raise ValueError(f"{type(self).__name__}.open: one session's context video [1, n, c, h, w] and audio "
                             f"[1, n, ca]; got {tuple(video.shape)} and {tuple(audio.shape)}")
        return self._open((video, audio), mouse, btn, seed)

    def _slot_frame(self, frames, slot):
        return frames[0][slot:slot + 1], frames[1][slot:slot + 1]


class AVStreamPool(_AVSlotPool, AVFrameStream):
    """AVFrameStream for n_slots sessions of the MMDiT core (backbone ``mmdit``, head_dim 64) on the slot forms
    of the joint-frame ring kernels (MMDiTBlock._forward_ring_decode)."""


class AVDiTStreamPool(_AVSlotPool, AVDiTFrameStream):
    """AVDiTFrameStream for n_slots sessions of the dit-backbone core (head_dim 64, at most 80 tokens per frame)
    on ``owlk_qk_rope_fwd_kv_ring_slots`` + the wide slot decode attention (Attn._attend); like its stream it
    rebases on OrthoRoPE as well."""


def av_pool_cls(backbone):
    """The audio + video pool class of a GameRFTAudioCore's backbone (as stream.av_stream_cls)."""
    return AVDiTStreamPool if backbone == "dit" else AVStreamPool
