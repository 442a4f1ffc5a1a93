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
"""
import torch

from .. import kernels as K
from ..nn.attn import check_rope_rows
from ..nn.kv_cache import RingKVCache
from .av_caching_v2 import _release_graph
from .schedulers import get_deltas, get_sd3_euler

REBASE_ROPES = ("motion", "audio1d")  # angle tables linear in the frame index (prefix-stable)


class FrameStream:
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

    # ------------------------------------------------------------------ life cycle
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
            raise RuntimeError(f"FrameStream: frame {self.frames_generated} would pass the {rope.cos.shape[0]}-row "
                               f"RoPE table and rope_impl {impl!r} cannot be rebased (its table is not linear in "
                               f"the frame index, nor prefix-stable); use one of {REBASE_ROPES}")
        cache.rebase(off - len(cache), rope)
        self.rebases += 1

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
