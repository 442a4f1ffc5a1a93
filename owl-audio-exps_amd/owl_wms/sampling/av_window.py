"""AVWindowSampler / CausalAVWindowSampler / CausalAVWindowSamplerNoCFG (reference:
owl_wms/sampling/av_window.py:15-372) for the audio + video core (GameRFTAudioCore).

Every generated frame is inpainted at the end of a window of ``window_length`` frames: the last
``window_length - 1`` clean frames re-noised to ``noise_prev`` plus one pure-noise frame (ts =
noise_prev, 1 on the last), denoised by ``n_steps`` Euler steps of the sd3 schedule that update the
last frame only.  Noise is drawn with torch.randn_like in the reference's order and shapes -- per
generated frame: video history [b, W-1, c, h, w], new video frame [b, c, h, w], audio history
[b, W-1, ca], new audio frame [b, ca].

``av_window`` runs the whole window through the model at every step (no cache).  The causal samplers
run it once per frame (step 0, a cache-updating forward), drop the frame being denoised from the
cache (``truncate(1, front=True)``) and decode it alone against the cache for the remaining steps,
with ``model.transformer.enable_decoding()`` around those steps (the MMDiT's fused joint-frame decode
path, nn/mmattn.py).

CFG: the reference runs the unconditional and the conditional forward one after the other, each with
its own cache.  Here both run as ONE forward of batch 2B -- rows [cond | uncond], has_controls =
[True] * B + [False] * B -- over one cache of batch 2B whose halves are exactly the reference's two
caches (as AVCachingSamplerV2 does).  ``cfg_scale <= 0`` in the causal sampler makes the unconditional
prediction only, as the reference does.

``compile_on_decode`` (causal samplers): the cache is emptied and refilled for every generated frame,
so every frame launches the same kernels on the same shapes.  The first frame runs eagerly (bf16
weight copies, workspaces and the cache buffers are made outside the graph pool); the second frame's
whole denoise -- prefill, the host's truncate bookkeeping, the decode steps, the Euler updates -- is
captured into one HIP graph on static input buffers and replayed for it and every later frame.  The
draws stay outside the graph.  Same kernels and arithmetic as the eager loop: bit-identical output.
"""
import torch

from ..nn.kv_cache import KVCache
from ..utils import batch_permute_to_length
from .schedulers import euler_dt, zlerp
from .step_graph import _release_graph, capture


class AVWindowSampler:
    """av_window.py:15-124.  Returns (video_out, audio_out, x, audio, mouse, btn)."""

    def __init__(self, n_steps=20, cfg_scale=1.3, window_length=60, num_frames=60, noise_prev=0.2,
                 only_return_generated=False):
        self.n_steps = n_steps
        self.cfg_scale = cfg_scale
        self.window_length = window_length
        self.num_frames = num_frames
        self.noise_prev = noise_prev
        self.only_return_generated = only_return_generated

    # ---- shared by the three samplers
    def _history(self, clean_v, clean_a):
        """step_history (av_window.py:54-66): the window's noised history + the new frame, four draws."""
        W = self.window_length
        hv = clean_v[:, -W:].clone()
        hv[:, :-1] = zlerp(hv[:, 1:], self.noise_prev)
        hv[:, -1] = torch.randn_like(hv[:, 0])
        ha = clean_a[:, -W:].clone()
        ha[:, :-1] = zlerp(ha[:, 1:], self.noise_prev)
        ha[:, -1] = torch.randn_like(ha[:, 0])
        ts = torch.ones(hv.shape[0], hv.shape[1], device=hv.device, dtype=hv.dtype)
        ts[:, :-1] = self.noise_prev
        return hv, ha, ts

    def _guided(self, model, xs, has_controls, cfg, kv_cache=None):
        """One prediction for xs = (video, audio, ts, mouse, btn): with cfg both passes as one 2B batch
        [cond | uncond] and pred = uncond + cfg_scale (cond - uncond)."""
        if cfg:
            xs = [torch.cat([t, t]) for t in xs]
        kw = {} if kv_cache is None else {"kv_cache": kv_cache}
        pv, pa = model(*xs, has_controls=has_controls, **kw)
        if cfg:
            B = pv.shape[0] // 2
            pv = pv[B:] + self.cfg_scale * (pv[:B] - pv[B:])
            pa = pa[B:] + self.cfg_scale * (pa[:B] - pa[B:])
        return pv, pa

    @staticmethod
    def _controls(B, cfg, conditioned, device):
        if cfg:
            hc = torch.zeros(2 * B, dtype=torch.bool, device=device)
            hc[:B] = True
            return hc
        return torch.full((B,), bool(conditioned), dtype=torch.bool, device=device)

    def _cut(self, x, audio, mouse, btn):
        if self.only_return_generated:
            n = self.num_frames
            return x[:, -n:], audio[:, -n:], mouse[:, -n:], btn[:, -n:]
        return x, audio, mouse, btn

    @torch.no_grad()
    def __call__(self, model, video, audio, mouse, btn, decode_fn=None, audio_decode_fn=None, image_scale=1,
                 audio_scale=1):
        """model: a GameRFTAudioCore; video [b, n, c, h, w], audio [b, n, ca], mouse [b, n, 2], btn
        [b, n, n_buttons] -> latents [b, n + num_frames, ...] (the generated ones with only_return_generated)."""
        W = self.window_length
        dt = euler_dt(self.n_steps, None, video)
        clean_v, clean_a = video.clone(), audio.clone()
        ext_mouse, ext_btn = batch_permute_to_length(mouse, btn, self.num_frames + W)
        hc = self._controls(video.shape[0], True, True, video.device)
        for frame_idx in range(self.num_frames):
            hv, ha, ts = self._history(clean_v, clean_a)
            mw, bw = ext_mouse[:, frame_idx:frame_idx + W], ext_btn[:, frame_idx:frame_idx + W]
            for step_idx in range(self.n_steps):
                pv, pa = self._guided(model, (hv, ha, ts, mw, bw), hc, True)
                hv[:, -1] = hv[:, -1] - pv[:, -1] * dt[step_idx]
                ha[:, -1] = ha[:, -1] - pa[:, -1] * dt[step_idx]
                ts[:, -1] = ts[:, -1] - dt[step_idx]
            clean_v = torch.cat([clean_v, hv[:, -1:]], dim=1)
            clean_a = torch.cat([clean_a, ha[:, -1:]], dim=1)
        x, audio, ext_mouse, ext_btn = self._cut(clean_v, clean_a, ext_mouse, ext_btn)
        video_out = decode_fn(x * image_scale) if decode_fn is not None else None
        audio_out = audio_decode_fn(audio * audio_scale) if audio_decode_fn is not None else None
        return video_out, audio_out, x, audio, ext_mouse, ext_btn


class CausalAVWindowSampler(AVWindowSampler):
    """av_window.py:126-265.  Returns (x, audio, mouse, btn)."""

    conditioned = False  # without CFG (cfg_scale <= 0): the unconditional prediction only
    use_decoding = True  # model.transformer.enable_decoding() around the decode steps

    def _cfg(self):
        return self.cfg_scale > 0

    def _denoise(self, model, cache, hv, ha, ts, mw, bw, dt, hc):
        """One generated frame: step 0 fills the cache from the whole window, the frame being denoised
        is dropped from it, steps 1.. decode that frame alone -> its (video [b, 1, c, h, w], audio
        [b, 1, ca]) after the last step."""
        cfg = self._cfg()
        cache.rewind()
        cache.enable_cache_updates()
        try:
            pv, pa = self._guided(model, (hv, ha, ts, mw, bw), hc, cfg, cache)
            cache.truncate(1, front=True)  # the final frame doesn't go in cache
        finally:
            cache.disable_cache_updates()
        # the reference writes every step's result back into the window's last frame: its dtype
        xv = (hv[:, -1:] - pv[:, -1:] * dt[0]).to(hv.dtype)
        xa = (ha[:, -1:] - pa[:, -1:] * dt[0]).to(ha.dtype)
        t = ts[:, -1:] - dt[0]
        if self.n_steps == 1:
            return xv, xa
        m1, b1 = mw[:, -1:], bw[:, -1:]
        tr = model.transformer
        was = bool(getattr(tr, "decoding", False))
        if self.use_decoding:
            tr.enable_decoding()
        try:
            for step_idx in range(1, self.n_steps):
                pv, pa = self._guided(model, (xv, xa, t, m1, b1), hc, cfg, cache)
                xv = (xv - pv * dt[step_idx]).to(hv.dtype)
                xa = (xa - pa * dt[step_idx]).to(ha.dtype)
                t = t - dt[step_idx]
        finally:
            if self.use_decoding and not was:
                tr.disable_decoding()
        return xv, xa

    @torch.no_grad()
    def __call__(self, model, video, audio, mouse, btn, decode_fn=None, audio_decode_fn=None, image_scale=1,
                 audio_scale=1, compile_on_decode=False):
        W = self.window_length
        B = video.shape[0]
        cfg = self._cfg()
        dt = euler_dt(self.n_steps, None, video)
        clean_v, clean_a = video.clone(), audio.clone()
        ext_mouse, ext_btn = batch_permute_to_length(mouse, btn, self.num_frames + W)
        hc = self._controls(B, cfg, self.conditioned, video.device)
        cache = KVCache(model.config)
        cache.reset(2 * B if cfg else B)
        graph = static = outs = None
        try:
            for frame_idx in range(self.num_frames):
                ins = self._history(clean_v, clean_a) + (ext_mouse[:, frame_idx:frame_idx + W],
                                                         ext_btn[:, frame_idx:frame_idx + W])
                # the graph's shapes: a full window (a shorter context grows frame by frame, eagerly)
                fixed = compile_on_decode and frame_idx > 0 and ins[0].shape[1] == W
                if fixed and graph is None:
                    static = [t.clone() for t in ins]
                    graph, outs = capture(lambda: self._denoise(model, cache, *static, dt, hc))
                if fixed and [t.shape for t in ins] == [t.shape for t in static]:
                    for dst, src in zip(static, ins):
                        dst.copy_(src)
                    graph.replay()
                    xv, xa = outs[0].clone(), outs[1].clone()
                else:
                    xv, xa = self._denoise(model, cache, *ins, dt, hc)
                clean_v = torch.cat([clean_v, xv], dim=1)
                clean_a = torch.cat([clean_a, xa], dim=1)
        finally:
            if graph is not None:
                _release_graph(graph)  # drains the queued replays first
        x, audio, ext_mouse, ext_btn = self._cut(clean_v, clean_a, ext_mouse, ext_btn)
        if decode_fn is not None:
            x = decode_fn(x * image_scale)
        if audio_decode_fn is not None:
            audio = audio_decode_fn(audio * audio_scale)
        return x, audio, ext_mouse, ext_btn


class CausalAVWindowSamplerNoCFG(CausalAVWindowSampler):
    """av_window.py:268-372: the conditional prediction alone, one cache."""

    conditioned = True

    def _cfg(self):
        return False
