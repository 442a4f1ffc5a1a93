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
joint-frame decode kernels, both modalities updated from one forward.
"""
import torch

from .. import kernels as K
from ..nn.attn import check_rope_rows
from ..nn.kv_cache import RingKVCache
from ..utils import batch_permute_to_length
from .av_caching_v2 import _release_graph
from .schedulers import get_deltas, get_sd3_euler

REBASE_ROPES = ("motion", "audio1d")  # angle tables linear in the frame index (prefix-stable)


class _RingStream:
    """What FrameStream and AVFrameStream share: the captured step's life cycle, zlerp and the RoPE rebase
    of the ring cache.  Expects self.core, self.kv_cache, self.frames_generated, self.rebases and
    self._step_graph = (graph, static buffers) or None."""

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def close(self):
        """Release the captured step (after its queued replays have run)."""
        if self._step_graph is not None:
            _release_graph(self._step_graph[0])
        self._step_graph = None

    @staticmethod
    def zlerp(x, alpha):
        z = torch.randn_like(x)
        return x * (1.0 - alpha) + z * alpha

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
        if impl not in REBASE_ROPES:
            raise RuntimeError(f"{type(self).__name__}: frame {self.frames_generated} would pass the "
                               f"{rope.cos.shape[0]}-row RoPE table and rope_impl {impl!r} cannot be rebased (its "
                               f"table is not linear in the frame index, nor prefix-stable); use one of {REBASE_ROPES}")
        cache.rebase(off - len(cache), rope)
        self.rebases += 1


class FrameStream(_RingStream):
    def __init__(self, core, n_steps: int = 16, cfg_scale: float = 1.3, noise_prev: float = 0.2,
                 max_cached_frames: int = 120, custom_schedule=None, graphed: bool = False) -> None:
        cfg = core.config
        if max_cached_frames < 1:
            raise ValueError("FrameStream: max_cached_frames must be at least 1")
        if max_cached_frames + 1 >= cfg.n_frames:
            raise ValueError(f"FrameStream: max_cached_frames + 1 = {max_cached_frames + 1} must be below "
                             f"config.n_frames = {cfg.n_frames}: the cached frames and the new one must fit the "
                             "RoPE table with room to rebase into")
        D = cfg.d_model // cfg.n_heads
        if cfg.backbone != "dit" or not K.decode_dev_supported(D, cfg.tokens_per_frame):
            raise ValueError("FrameStream: needs the DiT device-state decode path (head_dim 64 or 128, at most 64 "
                             f"tokens per frame); got backbone {cfg.backbone!r}, head_dim {D}, "
                             f"{cfg.tokens_per_frame} tokens per frame")
        self.core = core
        self.n_steps = n_steps
        self.cfg_scale = cfg_scale
        self.noise_prev = noise_prev
        self.max_cached_frames = max_cached_frames
        self.custom_schedule = custom_schedule
        self.graphed = graphed
        self.frames_generated = 0
        self.rebases = 0
        self.kv_cache = None
        self._step_graph = None
        self._pool = None

    def _rep(self, *ts):
        return [torch.cat([a, a]) for a in ts] if self.cfg_scale != 1.0 else list(ts)

    @torch.no_grad()
    def start(self, x, mouse, btn):
        """Cache the context frames x [b, n, c, h, w] with their controls, as AVCachingSamplerV2 does
        (zlerp at noise_prev; with CFG one 2B batch [cond | uncond])."""
        self.close()
        core, cfg = self.core, self.core.config
        B, init_len = x.size(0), x.size(1)
        if not 1 <= init_len <= self.max_cached_frames:
            raise ValueError(f"FrameStream.start: {init_len} context frames do not fit max_cached_frames = "
                             f"{self.max_cached_frames}")
        if self.custom_schedule is None:
            self._dt = get_sd3_euler(self.n_steps).to(device=x.device, dtype=x.dtype)
        else:
            self._dt = torch.tensor(get_deltas(list(self.custom_schedule)), device=x.device, dtype=torch.float32)
        tpf = cfg.tokens_per_frame
        cache = RingKVCache(cfg, (self.max_cached_frames + 1) * tpf, rope=core.transformer.rope)
        cache.reset(2 * B if self.cfg_scale != 1.0 else B)
        mouse, btn = mouse[:, :init_len], btn[:, :init_len]
        x_noisy = self.zlerp(x, self.noise_prev)
        self._t_prev = x.new_full((B, init_len), self.noise_prev)
        cache.enable_cache_updates()
        core(*self._rep(x_noisy, self._t_prev, mouse, btn), kv_cache=cache)
        cache.disable_cache_updates()
        cache.enable_device_state()
        self._x1 = x[:, :1]
        self.kv_cache = cache
        self.frames_generated = 0
        self.rebases = 0
        return self

    # ------------------------------------------------------------------ one frame
    def _euler_step(self, x, t, mouse, btn, null_mouse, null_btn, dt):
        """av_caching_v2.py:96-110: one Euler step with optional CFG (cond | uncond as one 2B batch)."""
        core, cache = self.core, self.kv_cache
        if self.cfg_scale != 1.0:
            B = x.shape[0]
            pred = core(torch.cat([x, x]), torch.cat([t, t]), torch.cat([mouse, null_mouse]),
                        torch.cat([btn, null_btn]), kv_cache=cache)
            pred_v, pred_u = pred[:B], pred[B:]
            pred_v = pred_u + self.cfg_scale * (pred_v - pred_u)
        else:
            pred_v = core(x, t, mouse, btn, kv_cache=cache)
        return x - dt * pred_v, t - dt

    def _euler_replay(self, x, t, mouse, btn, null_mouse, null_btn):
        """AVCachingSamplerV2._euler_replay: ONE Euler step captured on the first frame and replayed for
        every step of every frame.  The ring's addresses are fixed and the kernels read the position
        from the device, so wraps and rebases leave the graph valid."""
        dt, st, first = self._dt, self._step_graph, 0
        if st is None:
            # first frame: step 0 eagerly (bf16 weight copies, workspaces outside the graph pool)
            x, t = self._euler_step(x, t, mouse, btn, null_mouse, null_btn, dt[0])
            if self.n_steps == 1:
                return x, t
            bufs = {"x": x.clone(), "t": t.clone(), "dt": dt[1].clone(), "mouse": mouse.clone(), "btn": btn.clone(),
                    "nm": null_mouse.clone(), "nb": null_btn.clone()}
            if self._pool is None:
                self._pool = torch.cuda.graph_pool_handle()
            g = torch.cuda.CUDAGraph()
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                with torch.cuda.graph(g, pool=self._pool, stream=side):
                    nx, nt = self._euler_step(bufs["x"], bufs["t"], bufs["mouse"], bufs["btn"], bufs["nm"],
                                              bufs["nb"], bufs["dt"])
                    bufs["x"].copy_(nx)
                    bufs["t"].copy_(nt)
            torch.cuda.current_stream().wait_stream(side)
            self._step_graph = st = (g, bufs)
            first = 1
        else:
            g, bufs = st
            # the replayed step reads its positions from the device: check them here as the eager
            # step's Attn._attend does (the kernels would only poison the rows with NaN)
            check_rope_rows(self.core.transformer.rope, self.kv_cache.get_offset(0),
                            self.core.config.tokens_per_frame)
            for k, v in (("x", x), ("t", t), ("mouse", mouse), ("btn", btn)):
                bufs[k].copy_(v)
        g, bufs = st
        for t_idx in range(first, self.n_steps):
            bufs["dt"].copy_(dt[t_idx])
            g.replay()
        return bufs["x"].clone(), bufs["t"].clone()

    @torch.no_grad()
    def step(self, mouse_1, btn_1):
        """One new frame from the controls mouse_1 [b, 1, 2], btn_1 [b, 1, n_buttons] -> [b, 1, c, h, w].
        Denoises it over n_steps Euler steps, re-noises it (zlerp) and commits it to the cache, then
        evicts the oldest frame once more than max_cached_frames are cached."""
        if self.kv_cache is None:
            raise RuntimeError("FrameStream.step before start(): cache the context frames first")
        core, cache = self.core, self.kv_cache
        self._rebase_if_needed()
        B = self._x1.size(0)
        curr_x, curr_t = torch.randn_like(self._x1), self._t_prev.new_ones(B, 1)
        null_mouse, null_btn = torch.zeros_like(mouse_1), torch.zeros_like(btn_1)
        core.transformer.enable_decoding()
        try:
            if self.graphed:
                curr_x, curr_t = self._euler_replay(curr_x, curr_t, mouse_1, btn_1, null_mouse, null_btn)
            else:
                for t_idx in range(self.n_steps):
                    curr_x, curr_t = self._euler_step(curr_x, curr_t, mouse_1, btn_1, null_mouse, null_btn,
                                                      self._dt[t_idx])
            frame = curr_x.clone()
            x_noisy = self.zlerp(curr_x, self.noise_prev)
            t_noisy = torch.ones_like(curr_t) * self.noise_prev
            cache.enable_cache_updates()
            core(*self._rep(x_noisy, t_noisy, mouse_1, btn_1), kv_cache=cache)
            cache.disable_cache_updates()
        finally:
            core.transformer.disable_decoding()
        if cache.n_frames() > self.max_cached_frames:
            cache.truncate(1, front=False)
        self.frames_generated += 1
        return frame


class StreamSampler:
    """Sampler id ``av_stream``: AVCachingSamplerV2's call signature on a FrameStream, so a rollout may
    run past config.n_frames.  ``max_window`` counts as the sampler's does (list entries, the context
    as one): the stream caches ``max_window + init_len - 1`` frames.  None: the longest window the
    RoPE table leaves room to rebase in, ``config.n_frames - 2`` frames."""

    def __init__(self, n_steps: int = 16, cfg_scale: float = 1.3, num_frames: int = 60, noise_prev: float = 0.2,
                 max_window=None, custom_schedule=None) -> None:
        self.n_steps = n_steps
        self.cfg_scale = cfg_scale
        self.num_frames = num_frames
        self.noise_prev = noise_prev
        self.max_window = max_window
        self.custom_schedule = custom_schedule

    @torch.no_grad()
    def __call__(self, model, x, mouse, btn, compile_on_decode=False):
        """model: a GameRFTCore; returns [b, init + new, c, h, w]."""
        init_len = x.size(1)
        cached = model.config.n_frames - 2 if self.max_window is None else self.max_window + init_len - 1
        num_frames = min(self.num_frames, mouse.size(1) - init_len)
        latents = [x.clone()]
        with FrameStream(model, self.n_steps, self.cfg_scale, self.noise_prev, cached, self.custom_schedule,
                         graphed=compile_on_decode) as stream:
            stream.start(x, mouse, btn)
            for idx in range(num_frames):
                i = init_len + idx
                latents.append(stream.step(mouse[:, i:i + 1], btn[:, i:i + 1]))
        return torch.cat(latents, dim=1)


class AVFrameStream(_RingStream):
    """FrameStream for the audio + video core (GameRFTAudioCore, backbone ``mmdit``): ``pipe(controls) ->
    (video frame, audio frame)`` for as long as the caller likes, on the ring forms of the MMDiT's
    joint-frame decode kernels (MMDiTBlock._forward_ring_decode).

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
        D = cfg.d_model // cfg.n_heads
        if cfg.backbone != "mmdit" or D != 64:
            raise ValueError("AVFrameStream: needs the MMDiT joint-frame decode path (backbone 'mmdit', head_dim 64); "
                             f"got backbone {cfg.backbone!r}, head_dim {D}")
        if max_cached_frames < 1:
            raise ValueError("AVFrameStream: max_cached_frames must be at least 1")
        if max_cached_frames + 1 >= cfg.n_frames:
            raise ValueError(f"AVFrameStream: max_cached_frames + 1 = {max_cached_frames + 1} must be below "
                             f"config.n_frames = {cfg.n_frames}: the cached frames and the new one must fit the "
                             "RoPE table with room to rebase into")
        if ring_frames is not None and ring_frames < max_cached_frames + 1:
            raise ValueError(f"AVFrameStream: ring_frames = {ring_frames} cannot hold max_cached_frames + 1 = "
                             f"{max_cached_frames + 1} frames")
        self.core = core
        self.n_steps = n_steps
        self.cfg_scale = cfg_scale
        self.noise_prev = noise_prev
        self.max_cached_frames = max_cached_frames
        self.ring_frames = ring_frames if ring_frames is not None else max_cached_frames + 1
        self.graphed = graphed
        self.frames_generated = 0
        self.rebases = 0
        self.kv_cache = None
        self._step_graph = None
        self._pool = None

    def _cfg(self):
        return self.cfg_scale != 1.0

    def _rep(self, *ts):
        return [torch.cat([a, a]) for a in ts] if self._cfg() else list(ts)

    @torch.no_grad()
    def start(self, video, audio, mouse, btn):
        """Cache the context frames video [b, n, c, h, w] / audio [b, n, ca] with their controls: each
        zlerp-ed to noise_prev, one cache-updating forward (with CFG one 2B batch [cond | uncond])."""
        self.close()
        core, cfg = self.core, self.core.config
        B, init_len = video.size(0), video.size(1)
        if not 1 <= init_len <= self.max_cached_frames:
            raise ValueError(f"AVFrameStream.start: {init_len} context frames do not fit max_cached_frames = "
                             f"{self.max_cached_frames}")
        self._dt = get_sd3_euler(self.n_steps).to(device=video.device, dtype=video.dtype)
        cache = RingKVCache(cfg, self.ring_frames * cfg.tokens_per_frame, rope=core.transformer.rope)
        cache.reset(2 * B if self._cfg() else B)
        mouse, btn = mouse[:, :init_len], btn[:, :init_len]
        v_noisy = self.zlerp(video, self.noise_prev)
        a_noisy = self.zlerp(audio, self.noise_prev)
        ts = video.new_full((B, init_len), self.noise_prev)
        self._hc = torch.ones(2 * B if self._cfg() else B, dtype=torch.bool, device=video.device)
        if self._cfg():
            self._hc[B:] = False
        cache.enable_cache_updates()
        core(*self._rep(v_noisy, a_noisy, ts, mouse, btn), has_controls=self._hc, kv_cache=cache)
        cache.disable_cache_updates()
        cache.enable_device_state()
        self._v1, self._a1, self._t1 = video[:, :1], audio[:, :1], ts[:, :1]
        self.kv_cache = cache
        self.frames_generated = 0
        self.rebases = 0
        return self

    # ------------------------------------------------------------------ one frame
    def _euler_step(self, xv, xa, t, mouse, btn, dt):
        """One Euler step of both modalities from one forward (FrameStream._euler_step's arithmetic)."""
        pv, pa = self.core(*self._rep(xv, xa, t, mouse, btn), has_controls=self._hc, kv_cache=self.kv_cache)
        if self._cfg():
            B = xv.shape[0]
            pv = pv[B:] + self.cfg_scale * (pv[:B] - pv[B:])
            pa = pa[B:] + self.cfg_scale * (pa[:B] - pa[B:])
        return xv - dt * pv, xa - dt * pa, t - dt

    def _euler_replay(self, xv, xa, t, mouse, btn):
        """FrameStream._euler_replay for two modalities: step 0 of the first frame eagerly, then ONE
        captured Euler step replayed for every step of every frame (the ring's addresses are fixed and
        the kernels read the position from the device)."""
        dt, st, first = self._dt, self._step_graph, 0
        if st is None:
            xv, xa, t = self._euler_step(xv, xa, t, mouse, btn, dt[0])
            if self.n_steps == 1:
                return xv, xa, t
            bufs = {"xv": xv.clone(), "xa": xa.clone(), "t": t.clone(), "dt": dt[1].clone(), "mouse": mouse.clone(),
                    "btn": btn.clone()}
            if self._pool is None:
                self._pool = torch.cuda.graph_pool_handle()
            g = torch.cuda.CUDAGraph()
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                with torch.cuda.graph(g, pool=self._pool, stream=side):
                    nv, na, nt = self._euler_step(bufs["xv"], bufs["xa"], bufs["t"], bufs["mouse"], bufs["btn"],
                                                  bufs["dt"])
                    bufs["xv"].copy_(nv)
                    bufs["xa"].copy_(na)
                    bufs["t"].copy_(nt)
            torch.cuda.current_stream().wait_stream(side)
            self._step_graph = st = (g, bufs)
            first = 1
        else:
            g, bufs = st
            # the replayed step reads its positions from the device: check them here as the eager
            # step's MMDIT.forward does (the kernels would only poison the rows with NaN)
            check_rope_rows(self.core.transformer.rope, self.kv_cache.get_offset(0),
                            self.core.config.tokens_per_frame)
            for k, v in (("xv", xv), ("xa", xa), ("t", t), ("mouse", mouse), ("btn", btn)):
                bufs[k].copy_(v)
        g, bufs = st
        for t_idx in range(first, self.n_steps):
            bufs["dt"].copy_(dt[t_idx])
            g.replay()
        return bufs["xv"].clone(), bufs["xa"].clone(), bufs["t"].clone()

    @torch.no_grad()
    def step(self, mouse_1, btn_1):
        """One new frame from the controls mouse_1 [b, 1, 2], btn_1 [b, 1, n_buttons] -> (video
        [b, 1, c, h, w], audio [b, 1, ca]).  Denoises it over n_steps Euler steps, re-noises both
        modalities (zlerp) and commits the frame to the cache, then evicts the oldest frame once more
        than max_cached_frames are cached."""
        if self.kv_cache is None:
            raise RuntimeError("AVFrameStream.step before start(): cache the context frames first")
        core, cache = self.core, self.kv_cache
        self._rebase_if_needed()
        xv, xa = torch.randn_like(self._v1), torch.randn_like(self._a1)
        t = torch.ones_like(self._t1)
        if self.graphed:
            xv, xa, t = self._euler_replay(xv, xa, t, mouse_1, btn_1)
        else:
            for t_idx in range(self.n_steps):
                xv, xa, t = self._euler_step(xv, xa, t, mouse_1, btn_1, self._dt[t_idx])
        video, audio = xv.clone(), xa.clone()
        v_noisy = self.zlerp(xv, self.noise_prev)
        a_noisy = self.zlerp(xa, self.noise_prev)
        t_noisy = torch.ones_like(t) * self.noise_prev
        cache.enable_cache_updates()
        try:
            core(*self._rep(v_noisy, a_noisy, t_noisy, mouse_1, btn_1), has_controls=self._hc, kv_cache=cache)
        finally:
            cache.disable_cache_updates()
        if cache.n_frames() > self.max_cached_frames:
            cache.truncate(1, front=False)
        self.frames_generated += 1
        return video, audio


class AVStreamSampler:
    """Sampler id ``av_audio_stream``: the causal audio + video samplers' call signature and return value
    on an AVFrameStream, so a rollout may run past config.n_frames (MotionRoPE; OrthoRoPE streams to the
    end of its table and then raises).  A persistent-cache sampler -- each frame noised and cached once --
    not ``av_causal``'s re-noise-the-window-per-frame algorithm: the two are not comparable draw for
    draw.  ``max_cached_frames`` None: the longest window the RoPE table leaves room to rebase in,
    ``config.n_frames - 2`` frames."""

    def __init__(self, n_steps: int = 16, cfg_scale: float = 1.3, num_frames: int = 60, noise_prev: float = 0.2,
                 max_cached_frames=None) -> None:
        self.n_steps = n_steps
        self.cfg_scale = cfg_scale
        self.num_frames = num_frames
        self.noise_prev = noise_prev
        self.max_cached_frames = max_cached_frames

    @torch.no_grad()
    def __call__(self, model, video, audio, mouse, btn, decode_fn=None, audio_decode_fn=None, image_scale=1,
                 audio_scale=1, compile_on_decode=False):
        """model: a GameRFTAudioCore; returns (x [b, n + num_frames, c, h, w], audio [b, n + num_frames, ca],
        mouse, btn) with the controls extended as the causal samplers extend them."""
        n = video.size(1)
        cached = model.config.n_frames - 2 if self.max_cached_frames is None else self.max_cached_frames
        ext_mouse, ext_btn = batch_permute_to_length(mouse, btn, n + self.num_frames)
        vs, as_ = [video.clone()], [audio.clone()]
        with AVFrameStream(model, self.n_steps, self.cfg_scale, self.noise_prev, cached,
                           graphed=compile_on_decode) as stream:
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
