"""Endless frame streaming (reference: inference/causvid_pipeline.py:112-163, ``pipe(new_mouse, new_btn) ->
frame``) on libowlk's device-state decode path.

``FrameStream`` feeds a causal ``GameRFTCore`` live controls one frame at a time for as long as the
caller likes.  The reference pipeline re-runs its whole sliding window of frames for every Euler step of
every call; here the window lives in the KV cache and only the new frame is computed.  It is
``AVCachingSamplerV2`` (av_caching_v2.py:24-144) turned inside out -- the same
context caching, Euler steps, CFG batch and torch draws in the same order -- with the two limits of
that sampler removed:

* the KV cache is a ring (``RingKVCache``): ``(max_cached_frames + 1) * tokens_per_frame`` rows per
  layer, allocated once; writes and evictions wrap, the addresses never move, so one captured Euler
  step (``graphed=True``) replays for every step of every frame across wraps;
* before a frame whose rows would pass the RoPE table the cached, already rotated K is re-rotated in
  place so that the oldest live key sits at position 0 (``owlk_rope_rebase``).  MotionRoPE and
  Audio1DRoPE angles are linear in the frame index, so q.k depends only on frame differences and the
  attention is unchanged up to the table's fp32 precision and one bf16 rounding of K per rebase.

``StreamSampler`` (sampler id ``av_stream``) drives a ``FrameStream`` behind the samplers' call
signature, for eval rollouts longer than ``config.n_frames``.

``AVFrameStream`` / ``AVStreamSampler`` (sampler id ``av_audio_stream``) are the same for the audio + video
core (GameRFTAudioCore on the MMDiT): 65-row joint frames [64 video | 1 audio] on the ring forms of the
joint-frame decode kernels, both modalities updated from one forward.  ``AVDiTFrameStream`` is the same
for the core on the plain DiT (``backbone: dit``, the reference's configs/causvid.yml): the 65-row frame on
the wide ring decode attention (owlk_attn_decode_wide_ring_fwd); the sampler id serves both backbones.
``AudioStream`` / ``AudioStreamSampler`` (sampler id ``audio_stream``) are the same for the audio core
(AudioRFTCore): one token per frame, unconditional, no controls.

``graphed`` on every class: False (eager), True (one captured Euler step replayed for every step of every
frame; the forward that commits the finished frame stays eager) or "frame" -- the whole frame as one graph,
the commit and the eviction included: the ring position {start, cached, offset} is advanced on the device by
``owlk_ring_advance`` (RingKVCache.advance), the host keeps an exact mirror of it, and ``close()`` compares
the two.  The three modes give the same bits.
"""
import torch

from .. import kernels as K
from ..nn.attn import check_rope_rows
from ..nn.kv_cache import RingKVCache
from ..utils import batch_permute_to_length
from .av_caching_v2 import guided_velocity
from .schedulers import euler_dt, renoise, zlerp
from .step_graph import FrameGraph, StepGraph

REBASE_ROPES = ("motion", "audio1d")  # angle tables linear in the frame index (prefix-stable)


def graph_mode(compile_on_decode, frame_graph):
    """A sampler's ``compile_on_decode`` / ``frame_graph`` pair -> a stream's ``graphed``."""
    return "frame" if compile_on_decode and frame_graph else compile_on_decode


class _RingStream:
    """FrameStream and the audio + video streams over a tuple of latents -- (x,) for video, (video, audio) for
    audio + video, (x,) for audio: the context pass into a RingKVCache, one frame per step (rebase, draws, Euler
    steps eager or replayed from one captured step, zlerp, the cache-updating forward, eviction -- or all of it
    after the draws as one captured frame, _frame) and the captured step's or frame's life cycle.  A subclass
    supplies the core it accepts (its __init__), how one guided prediction is formed (_guided) and how the core
    is called with the cache (_forward)."""

    custom_schedule = None  # FrameStream's option
    decoding = False  # transformer.enable_decoding() around a step (FrameStream, AVDiTFrameStream)
    rebase_ropes = REBASE_ROPES  # the rope_impl values the class may rebase (AVDiTFrameStream: ortho as well)

    def __init__(self, core, n_steps, cfg_scale, noise_prev, max_cached_frames, graphed, ring_frames=None):
        name, cfg = type(self).__name__, core.config
        if graphed not in (False, True, "frame"):
            raise ValueError(f"{name}: graphed must be False, True (one captured Euler step) or 'frame' (the whole "
                             f"frame captured); got {graphed!r}")
        if max_cached_frames < 1:
            raise ValueError(f"{name}: max_cached_frames must be at least 1")
        if max_cached_frames + 1 >= cfg.n_frames:
            raise ValueError(f"{name}: max_cached_frames + 1 = {max_cached_frames + 1} must be below "
                             f"config.n_frames = {cfg.n_frames}: the cached frames and the new one must fit the "
                             "RoPE table with room to rebase into")
        self.core = core
        self.n_steps = n_steps
        self.cfg_scale = cfg_scale
        self.noise_prev = noise_prev
        self.max_cached_frames = max_cached_frames
        if ring_frames is not None and ring_frames < max_cached_frames + 1:
            raise ValueError(f"{name}: ring_frames = {ring_frames} cannot hold max_cached_frames + 1 "
                             f"= {max_cached_frames + 1} frames")
        # the ring's size in frames; a larger ring wraps later and changes no bit of the output
        self.ring_frames = max_cached_frames + 1 if ring_frames is None else ring_frames
        self.graphed = graphed
        self.frames_generated = 0
        self.rebases = 0
        self.graph_replays = 0
        self.kv_cache = None
        self._step_graph = None
        self._pool = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close(check=exc[0] is None)  # an error on its way out is not replaced by the state check's
        return False

    def close(self, check=True):
        """Release the captured step or frame (after its queued replays have run).  In frame mode the ring
        position moved on the device alone: it is read back here and compared with the host mirror, which
        is where a state the kernels refused to follow (cached = -1, NaN frames since) surfaces."""
        if self._step_graph is not None:
            self._step_graph.release()
        self._step_graph = None
        cache = self.kv_cache
        if check and self.graphed == "frame" and cache is not None and cache.dev is not None:
            dev, host = cache.device_state(), (cache.start[0], len(cache), cache.get_offset(0))
            if dev != host:
                raise RuntimeError(f"{type(self).__name__}: the ring position on the device (start, cached, offset) "
                                   f"= {dev} differs from the host mirror {host} after {self.frames_generated} "
                                   "frames; a count of -1 marks a state the ring kernels refused to follow")

    def _cfg(self):
        return self.cfg_scale != 1.0

    def _rep(self, *ts):
        return [torch.cat([a, a]) for a in ts] if self._cfg() else list(ts)

    # ------------------------------------------------------------------ what a subclass supplies
    def _forward(self, cache, xs, t, mouse, btn):
        """The core on the latents xs at times t against `cache`, with CFG as one 2B batch [cond | uncond]
        (the context pass, the cache-updating forward of a finished frame)."""
        raise NotImplementedError

    def _guided(self, xs, t, ctrl):
        """One guided prediction per latent from the frame's controls `ctrl` (_controls)."""
        raise NotImplementedError

    def _controls(self, mouse_1, btn_1):
        """The named per-frame inputs of _guided (the captured step's static input buffers)."""
        return {"mouse": mouse_1, "btn": btn_1}

    # ------------------------------------------------------------------ context
    @torch.no_grad()
    def _start(self, latents, mouse, btn):
        """Cache the context frames: each latent zlerp-ed to noise_prev (in tuple order), one cache-updating
        forward, then the position moves to the device."""
        self.close()
        core, cfg = self.core, self.core.config
        B, init_len = latents[0].size(0), latents[0].size(1)
        if not 1 <= init_len <= self.max_cached_frames:
            raise ValueError(f"{type(self).__name__}.start: {init_len} context frames do not fit max_cached_frames = "
                             f"{self.max_cached_frames}")
        self._dt = euler_dt(self.n_steps, self.custom_schedule, latents[0])
        cache = RingKVCache(cfg, self.ring_frames * cfg.tokens_per_frame, rope=core.transformer.rope)
        cache.reset(2 * B if self._cfg() else B)
        noisy = tuple(zlerp(x, self.noise_prev) for x in latents)
        ts = latents[0].new_full((B, init_len), self.noise_prev)
        cache.enable_cache_updates()
        # a core without controls (AudioStream) passes None for both
        self._forward(cache, noisy, ts, *(c if c is None else c[:, :init_len] for c in (mouse, btn)))
        cache.disable_cache_updates()
        cache.enable_device_state()
        self._like, self._t1 = tuple(x[:, :1] for x in latents), ts[:, :1]
        self.kv_cache = cache
        self.frames_generated = 0
        self.rebases = 0
        self.graph_replays = 0
        return self

    # ------------------------------------------------------------------ one frame
    def _rebase_if_needed(self):
        """Before a frame whose rows would pass the RoPE table: re-rotate the cached K so that the
        oldest live key sits at position 0."""
        core, cache = self.core, self.kv_cache
        rope = core.transformer.rope
        tpf = core.config.tokens_per_frame
        off = cache.get_offset(0)
        if off + tpf <= rope.cos.shape[0]:
            return
        impl = str(getattr(core.config, "rope_impl", "ortho")).lower()
        if impl not in self.rebase_ropes:
            raise RuntimeError(f"{type(self).__name__}: frame {self.frames_generated} would pass the "
                               f"{rope.cos.shape[0]}-row RoPE table and rope_impl {impl!r} cannot be rebased by this "
                               f"stream; it rebases {self.rebase_ropes}")
        cache.rebase(off - len(cache), rope)
        self.rebases += 1

    def _euler_step(self, xs, t, ctrl, dt):
        """One Euler step of every latent from one guided prediction: x - dt * pred, t - dt."""
        preds = self._guided(xs, t, ctrl)
        return tuple(x - dt * p for x, p in zip(xs, preds)), t - dt

    def _denoise(self, xs, t, ctrl):
        """The frame's n_steps Euler steps.  graphed: ONE step captured on the first frame (a StepGraph) and
        replayed for every step of every frame.  The ring's addresses are fixed and the kernels read the
        position from the device, so wraps and rebases leave the graph valid."""
        dt = self._dt
        if not self.graphed:
            for t_idx in range(self.n_steps):
                xs, t = self._euler_step(xs, t, ctrl, dt[t_idx])
            return xs, t
        sg, first = self._step_graph, 0
        names = [f"x{i}" for i in range(len(xs))]
        if sg is None:
            # first frame: step 0 eagerly (bf16 weight copies, workspaces outside the graph pool)
            xs, t = self._euler_step(xs, t, ctrl, dt[0])
            if self.n_steps == 1:
                return xs, t

            def step(s, c, sdt):
                nxs, nt = self._euler_step(tuple(s[k] for k in names), s["t"], c, sdt)
                return (*nxs, nt)

            if self._pool is None:
                self._pool = torch.cuda.graph_pool_handle()
            sg = self._step_graph = StepGraph(step, {**dict(zip(names, xs)), "t": t}, ctrl, dt[1], self._pool)
            first = 1
        else:
            # the replayed step reads its positions from the device: check them here as the eager
            # step's forward does (the kernels would only poison the rows with NaN)
            check_rope_rows(self.core.transformer.rope, self.kv_cache.get_offset(0),
                            self.core.config.tokens_per_frame)
            # the frame's state and whatever _controls returns
            sg.load(**dict(zip(names, xs)), t=t, **ctrl)
        for t_idx in range(first, self.n_steps):
            sg.replay(dt[t_idx])
        self.graph_replays += self.n_steps - first
        *xs, t = sg.state()
        return tuple(xs), t

    def _frame(self, s):
        """graphed="frame": the whole frame as one function of the named tensors s -- the start noise x{i},
        the re-noise draws z{i}, the time t (ones) and the controls -- with nothing decided on the host:
        the n_steps Euler steps (dt from the persistent self._dt), the finished frame copied out, the
        re-noise, the forward on the re-noised frame and the ring position's advance on the device
        (owlk_ring_advance).  On the ring path a forward writes its rows behind the window whether or not
        cache updates are enabled -- should_update only moves the host bookkeeping -- so the last forward
        is an ordinary decode forward and `advance` stands for commit_device + sync_device_state +
        truncate.  Eager it also advances the host mirror; captured it executes nothing and the mirror
        stays (RingKVCache.advance)."""
        n = len(self._like)
        xs, t = tuple(s[f"x{i}"] for i in range(n)), s["t"]
        own = {"t"} | {f"{c}{i}" for c in "xz" for i in range(n)}
        ctrl = {k: v for k, v in s.items() if k not in own}  # what _controls returned
        for t_idx in range(self.n_steps):
            xs, t = self._euler_step(xs, t, ctrl, self._dt[t_idx])
        return self._commit_frame(xs, t, tuple(s[f"z{i}"] for i in range(n)), ctrl)

    def _commit_frame(self, xs, t, zs, ctrl):
        """_frame after its Euler steps: the finished frame copied out, the re-noise with the draws zs, the
        forward on the re-noised frame, the ring position's advance on the device."""
        tpf = self.core.config.tokens_per_frame
        frame = tuple(x.clone() for x in xs)
        noisy = tuple(renoise(x, z, self.noise_prev) for x, z in zip(xs, zs))
        t_noisy = torch.ones_like(t) * self.noise_prev
        self._forward(self.kv_cache, noisy, t_noisy, ctrl.get("mouse"), ctrl.get("btn"))
        self.kv_cache.advance(tpf, self.max_cached_frames * tpf)
        return frame

    def _graphed_frame(self, xs, t, ctrl):
        """One frame in frame mode.  The noise is drawn here, outside the graph, in the other modes' order
        (the start noise xs came first, now one re-noise draw per latent; they draw nothing in between).
        Frame 0 runs _frame eagerly (bf16 weight copies, workspaces outside the graph pool); frame 1
        captures it (a FrameGraph); from then on a frame is copy-in, one replay, clone-out, and the host
        mirror of the ring position follows by the same rule (exact: the rule is deterministic)."""
        cache, tpf = self.kv_cache, self.core.config.tokens_per_frame
        zs = tuple(torch.randn_like(x) for x in self._like)
        s = {**{f"x{i}": x for i, x in enumerate(xs)}, **{f"z{i}": z for i, z in enumerate(zs)}, "t": t, **ctrl}
        if self.frames_generated == 0:
            return self._frame(s)
        # the replayed frame reads its positions from the device: check them here as an eager forward does
        check_rope_rows(self.core.transformer.rope, cache.get_offset(0), tpf)
        fg = self._step_graph
        if fg is None:
            if self._pool is None:
                self._pool = torch.cuda.graph_pool_handle()
            fg = self._step_graph = FrameGraph(self._frame, s, self._pool)
        else:
            fg.load(**s)
        fg.replay()
        cache.advance(tpf, self.max_cached_frames * tpf, device=False)
        self.graph_replays += 1
        return fg.outputs()

    @torch.no_grad()
    def _step(self, mouse_1, btn_1):
        """One new frame from the controls mouse_1 [b, 1, 2], btn_1 [b, 1, n_buttons] -> a tuple of latents
        [b, 1, ...].  Draws one noise per latent (tuple order), denoises over n_steps Euler steps, re-noises
        each latent (zlerp, tuple order) and commits the frame to the cache, then evicts the oldest frame
        once more than max_cached_frames are cached."""
        if self.kv_cache is None:
            raise RuntimeError(f"{type(self).__name__}.step before start(): cache the context frames first")
        core, cache = self.core, self.kv_cache
        self._rebase_if_needed()
        xs = tuple(torch.randn_like(x) for x in self._like)
        t = torch.ones_like(self._t1)
        ctrl = self._controls(mouse_1, btn_1)
        if self.decoding:
            core.transformer.enable_decoding()
        if self.graphed == "frame":
            try:
                frame = self._graphed_frame(xs, t, ctrl)
            finally:
                core.transformer.disable_decoding()
            self.frames_generated += 1
            return frame
        try:
            xs, t = self._denoise(xs, t, ctrl)
            frame = tuple(x.clone() for x in xs)
            noisy = tuple(zlerp(x, self.noise_prev) for x in xs)
            t_noisy = torch.ones_like(t) * self.noise_prev
            cache.enable_cache_updates()
            self._forward(cache, noisy, t_noisy, mouse_1, btn_1)
        finally:
            cache.disable_cache_updates()
            core.transformer.disable_decoding()
        if cache.n_frames() > self.max_cached_frames:
            cache.truncate(1, front=False)
        self.frames_generated += 1
        return frame


class FrameStream(_RingStream):
    """The video core (GameRFTCore on the DiT): ``pipe(controls) -> frame``.  CFG as AVCachingSamplerV2
    forms it (guided_velocity: [cond | null controls]); both halves of the cache are filled from the
    conditioned pass."""

    decoding = True

    def __init__(self, core, n_steps: int = 16, cfg_scale: float = 1.3, noise_prev: float = 0.2,
                 max_cached_frames: int = 120, custom_schedule=None, graphed=False, ring_frames=None) -> None:
        super().__init__(core, n_steps, cfg_scale, noise_prev, max_cached_frames, graphed, ring_frames)
        cfg = core.config
        D = cfg.d_model // cfg.n_heads
        if cfg.backbone != "dit" or not K.decode_dev_supported(D, cfg.tokens_per_frame):
            raise ValueError("FrameStream: needs the DiT device-state decode path (head_dim 64 or 128, at most 64 "
                             f"tokens per frame); got backbone {cfg.backbone!r}, head_dim {D}, "
                             f"{cfg.tokens_per_frame} tokens per frame")
        self.custom_schedule = custom_schedule

    def _forward(self, cache, xs, t, mouse, btn):
        return self.core(*self._rep(*xs, t, mouse, btn), kv_cache=cache)

    def _controls(self, mouse_1, btn_1):
        return {"mouse": mouse_1, "btn": btn_1, "nm": torch.zeros_like(mouse_1), "nb": torch.zeros_like(btn_1)}

    def _guided(self, xs, t, ctrl):
        return (guided_velocity(self.core, self.kv_cache, self.cfg_scale, xs[0], t, ctrl["mouse"], ctrl["btn"],
                                ctrl["nm"], ctrl["nb"]),)

    def start(self, x, mouse, btn):
        """Cache the context frames x [b, n, c, h, w] with their controls, as AVCachingSamplerV2 does
        (zlerp at noise_prev; with CFG one 2B batch [cond | uncond])."""
        return self._start((x,), mouse, btn)

    def step(self, mouse_1, btn_1):
        """One new frame from the controls mouse_1 [b, 1, 2], btn_1 [b, 1, n_buttons] -> [b, 1, c, h, w]
        (_RingStream._step)."""
        return self._step(mouse_1, btn_1)[0]


class StreamSampler:
    """Sampler id ``av_stream``: AVCachingSamplerV2's call signature on a FrameStream, so a rollout may
    run past config.n_frames.  ``max_window`` counts as the sampler's does (list entries, the context
    as one): the stream caches ``max_window + init_len - 1`` frames.  None: the longest window the
    RoPE table leaves room to rebase in, ``config.n_frames - 2`` frames."""

    def __init__(self, n_steps: int = 16, cfg_scale: float = 1.3, num_frames: int = 60, noise_prev: float = 0.2,
                 max_window=None, custom_schedule=None, frame_graph: bool = False) -> None:
        self.n_steps = n_steps
        self.cfg_scale = cfg_scale
        self.num_frames = num_frames
        self.noise_prev = noise_prev
        self.max_window = max_window
        self.custom_schedule = custom_schedule
        self.frame_graph = frame_graph  # compile_on_decode captures the whole frame, not one Euler step

    @torch.no_grad()
    def __call__(self, model, x, mouse, btn, compile_on_decode=False):
        """model: a GameRFTCore; returns [b, init + new, c, h, w]."""
        init_len = x.size(1)
        cached = model.config.n_frames - 2 if self.max_window is None else self.max_window + init_len - 1
        num_frames = min(self.num_frames, mouse.size(1) - init_len)
        latents = [x.clone()]
        with FrameStream(model, self.n_steps, self.cfg_scale, self.noise_prev, cached, self.custom_schedule,
                         graphed=graph_mode(compile_on_decode, self.frame_graph)) as stream:
            stream.start(x, mouse, btn)
            for idx in range(num_frames):
                i = init_len + idx
                latents.append(stream.step(mouse[:, i:i + 1], btn[:, i:i + 1]))
        return torch.cat(latents, dim=1)


class _AVRingStream(_RingStream):
    """AVFrameStream and AVDiTFrameStream: FrameStream for the audio + video core (GameRFTAudioCore):
    ``pipe(controls) -> (video frame, audio frame)`` for as long as the caller likes, 65-row joint frames
    [64 video | 1 audio] on a RingKVCache.  A subclass names the core it accepts (_check_core) and, where
    they differ from _RingStream's, ``decoding`` and ``rebase_ropes``.

    A persistent-cache sampler: every frame is noised (zlerp at noise_prev) and cached ONCE, as
    AVCachingSamplerV2 does for video.  It is not ``av_causal``'s algorithm, which re-noises the whole
    window and refills the cache for every generated frame, so its samples are not comparable with
    ``av_causal``'s draw for draw.  The new rows are roped at the cache's absolute offset; the reference's
    MMAttn (mmattn.py:60-62) ropes them at the cached length, which collides with live keys once the
    oldest frame has been evicted -- the reason its causal samplers refill the cache per frame.

    Draws, in order -- start: video context, audio context; per step(): video noise, audio noise, then
    (after the Euler steps) the clean video frame's zlerp, the clean audio frame's.  CFG as
    AVWindowSampler._guided forms it: one 2B batch [cond | uncond], has_controls = [True] * B + [False] * B,
    pred = uncond + cfg_scale (cond - uncond) per modality; cfg_scale 1.0 runs the conditional pass alone.
    ``ring_frames`` (default max_cached_frames + 1) sizes the ring; a larger ring wraps later and changes
    no bit of the output."""

    def __init__(self, core, n_steps: int = 16, cfg_scale: float = 1.3, noise_prev: float = 0.2,
                 max_cached_frames: int = 120, graphed: bool = False, ring_frames=None) -> None:
        cfg = core.config
        self._check_core(cfg, cfg.d_model // cfg.n_heads)
        super().__init__(core, n_steps, cfg_scale, noise_prev, max_cached_frames, graphed, ring_frames)

    def _check_core(self, cfg, D):
        """ValueError, naming what it got, unless this class streams the core of config cfg (head_dim D)."""
        raise NotImplementedError

    def _forward(self, cache, xs, t, mouse, btn):
        return self.core(*self._rep(*xs, t, mouse, btn), has_controls=self._hc, kv_cache=cache)

    def _guided(self, xs, t, ctrl):
        pv, pa = self._forward(self.kv_cache, xs, t, ctrl["mouse"], ctrl["btn"])
        if self._cfg():
            B = xs[0].shape[0]
            pv = pv[B:] + self.cfg_scale * (pv[:B] - pv[B:])
            pa = pa[B:] + self.cfg_scale * (pa[:B] - pa[B:])
        return pv, pa

    def start(self, video, audio, mouse, btn):
        """Cache the context frames video [b, n, c, h, w] / audio [b, n, ca] with their controls: each
        zlerp-ed to noise_prev, one cache-updating forward (with CFG one 2B batch [cond | uncond])."""
        B = video.size(0)
        self._hc = torch.ones(2 * B if self._cfg() else B, dtype=torch.bool, device=video.device)
        if self._cfg():
            self._hc[B:] = False
        return self._start((video, audio), mouse, btn)

    def step(self, mouse_1, btn_1):
        """One new frame from the controls mouse_1 [b, 1, 2], btn_1 [b, 1, n_buttons] -> (video
        [b, 1, c, h, w], audio [b, 1, ca]) (_RingStream._step)."""
        return self._step(mouse_1, btn_1)


class AVFrameStream(_AVRingStream):
    """The MMDiT core (backbone ``mmdit``, head_dim 64), on the ring forms of the MMDiT's joint-frame decode
    kernels (MMDiTBlock._forward_ring_decode)."""

    def _check_core(self, cfg, D):
        if cfg.backbone != "mmdit" or D != 64:
            raise ValueError("AVFrameStream: needs the MMDiT joint-frame decode path (backbone 'mmdit', head_dim 64); "
                             f"got backbone {cfg.backbone!r}, head_dim {D}")


class AVDiTFrameStream(_AVRingStream):
    """The dit-backbone core (the reference's configs/causvid.yml: ``game_rft_audio`` with ``backbone: dit``,
    the audio token appended to each frame's video tokens through the plain DiT; head_dim 64, at most 80
    tokens per frame), on ``owlk_qk_rope_fwd_kv_ring`` + the wide ring decode attention
    (``owlk_attn_decode_wide_ring_fwd``, Attn._attend), ``DiT.enable_decoding()`` around a step.

    It may rebase on OrthoRoPE (the reference's default) as well: the angle of token r of frame f is
    a_r + f * delta -- only the time axis moves, linearly -- and owlk_rope_rebase forms its rotation from
    two table rows, so it needs linearity only, not the prefix stability that OrthoRoPE's linspace time
    axis lacks (tests/test_av_dit_stream_cpu.py has the bound)."""

    decoding = True
    rebase_ropes = ("motion", "audio1d", "ortho")

    def _check_core(self, cfg, D):
        if cfg.backbone != "dit" or D != 64 or not 0 < cfg.tokens_per_frame <= K.WIDE_DECODE_ROWS:
            raise ValueError("AVDiTFrameStream: needs the DiT ring decode path (backbone 'dit', head_dim 64, at most "
                             f"{K.WIDE_DECODE_ROWS} tokens per frame); got backbone {cfg.backbone!r}, head_dim {D}, "
                             f"{cfg.tokens_per_frame} tokens per frame")


def av_stream_cls(backbone):
    """The audio + video stream class of a GameRFTAudioCore's backbone."""
    return AVDiTFrameStream if backbone == "dit" else AVFrameStream


class AVStreamSampler:
    """Sampler id ``av_audio_stream``: the causal audio + video samplers' call signature and return value
    on the stream class of the model's backbone (av_stream_cls: AVFrameStream for ``mmdit``, AVDiTFrameStream
    for ``dit``), so a rollout may run past config.n_frames (MotionRoPE; with OrthoRoPE the dit stream
    rebases too, the MMDiT stream runs to the end of its table and then raises).  A persistent-cache
    sampler -- each frame noised and cached once -- not ``av_causal``'s re-noise-the-window-per-frame algorithm: the two are not comparable draw for
    draw.  ``max_cached_frames`` None: the longest window the RoPE table leaves room to rebase in,
    ``config.n_frames - 2`` frames."""

    def __init__(self, n_steps: int = 16, cfg_scale: float = 1.3, num_frames: int = 60, noise_prev: float = 0.2,
                 max_cached_frames=None, frame_graph: bool = False) -> None:
        self.n_steps = n_steps
        self.cfg_scale = cfg_scale
        self.num_frames = num_frames
        self.noise_prev = noise_prev
        self.max_cached_frames = max_cached_frames
        self.frame_graph = frame_graph  # compile_on_decode captures the whole frame, not one Euler step

    @torch.no_grad()
    def __call__(self, model, video, audio, mouse, btn, decode_fn=None, audio_decode_fn=None, image_scale=1,
                 audio_scale=1, compile_on_decode=False):
        """model: a GameRFTAudioCore; returns (x [b, n + num_frames, c, h, w], audio [b, n + num_frames, ca],
        mouse, btn) with the controls extended as the causal samplers extend them."""
        n = video.size(1)
        cached = model.config.n_frames - 2 if self.max_cached_frames is None else self.max_cached_frames
        ext_mouse, ext_btn = batch_permute_to_length(mouse, btn, n + self.num_frames)
        vs, as_ = [video.clone()], [audio.clone()]
        with av_stream_cls(model.config.backbone)(model, self.n_steps, self.cfg_scale, self.noise_prev, cached,
                                                  graphed=graph_mode(compile_on_decode, self.frame_graph)) as stream:
            stream.start(video, audio, ext_mouse, ext_btn)
            for idx in range(self.num_frames):
                i = n + idx
                v, a = stream.step(ext_mouse[:, i:i + 1], ext_btn[:, i:i + 1])
                vs.append(v)
                as_.append(a)
        x, audio = torch.cat(vs, dim=1), torch.cat(as_, dim=1)
        if decode_fn is not None:
            x = decode_fn(x * image_scale)
        if audio_decode_fn is not None:
            audio = audio_decode_fn(audio * audio_scale)
        return x, audio, ext_mouse, ext_btn


class AudioStream(_RingStream):
    """The audio core (AudioRFTCore, the reference's configs/audio.yml): ``pipe() -> token`` for as long as
    the caller likes.  Unconditional, one token per frame, no CFG and no controls: AudioCachingSampler
    (audio_caching.py) turned inside out on a RingKVCache -- the same context caching, Euler steps and torch
    draws in the same order -- on ``owlk_qk_rope_fwd_kv_ring`` + ``owlk_attn_decode_ring_fwd`` at one query
    row, local layers on the last ``local_window`` tokens.  It rebases on Audio1DRoPE (and MotionRoPE), so
    it runs past the RoPE table, and its one-token forwards -- launch-bound, n_steps + 1 per token -- are
    what a captured step or frame removes most of."""

    decoding = True

    def __init__(self, core, n_steps: int = 16, noise_prev: float = 0.2, max_cached_frames: int = 120,
                 custom_schedule=None, graphed=False, ring_frames=None) -> None:
        super().__init__(core, n_steps, 1.0, noise_prev, max_cached_frames, graphed, ring_frames)
        cfg = core.config
        D = cfg.d_model // cfg.n_heads
        if cfg.backbone != "dit" or cfg.tokens_per_frame != 1 or not K.decode_dev_supported(D, 1):
            raise ValueError("AudioStream: needs the DiT device-state decode path (head_dim 64 or 128) at one token "
                             f"per frame; got backbone {cfg.backbone!r}, head_dim {D}, {cfg.tokens_per_frame} tokens "
                             "per frame")
        self.custom_schedule = custom_schedule

    def _forward(self, cache, xs, t, mouse, btn):
        return self.core(xs[0], t, doc_id=None, kv_cache=cache)

    def _controls(self, mouse_1, btn_1):
        return {}

    def _guided(self, xs, t, ctrl):
        return (self._forward(self.kv_cache, xs, t, None, None),)

    def start(self, x):
        """Cache the context tokens x [b, n, c], as AudioCachingSampler does (zlerp at noise_prev)."""
        return self._start((x,), None, None)

    def step(self):
        """One new token -> [b, 1, c] (_RingStream._step)."""
        return self._step(None, None)[0]


class AudioStreamSampler:
    """Sampler id ``audio_stream``: AudioCachingSampler's call signature and return value on an AudioStream,
    so a rollout may run past config.n_frames.  ``max_window`` counts as that sampler's does (list entries,
    the context as one): the stream caches ``max_window + init_len - 1`` tokens.  None: the longest window
    the RoPE table leaves room to rebase in, ``config.n_frames - 2`` tokens.  ``compile_on_decode`` replays
    one captured Euler step, with ``frame_graph`` one captured token."""

    def __init__(self, n_steps: int = 16, num_tokens: int = 120, noise_prev: float = 0.2, custom_schedule=None,
                 max_window=None, frame_graph: bool = False) -> None:
        self.n_steps = n_steps
        self.num_tokens = num_tokens
        self.noise_prev = noise_prev
        self.custom_schedule = custom_schedule
        self.max_window = max_window
        self.frame_graph = frame_graph

    @torch.no_grad()
    def __call__(self, model, x, decode_fn=None, vae_scale=1.0, compile_on_decode=False):
        """model: an AudioRFTCore; x [b, init_len, c] -> [b, init_len + num_tokens, c] (+ waveforms)."""
        init_len = x.size(1)
        cached = model.config.n_frames - 2 if self.max_window is None else self.max_window + init_len - 1
        latents = [x.clone()]
        with AudioStream(model, self.n_steps, self.noise_prev, cached, self.custom_schedule,
                         graphed=graph_mode(compile_on_decode, self.frame_graph)) as stream:
            stream.start(x)
            for _ in range(self.num_tokens):
                latents.append(stream.step())
        full = torch.cat(latents, dim=1)
        if decode_fn is not None:
            return full, decode_fn(full * vae_scale)
        return full
