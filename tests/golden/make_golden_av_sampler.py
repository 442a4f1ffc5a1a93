"""Golden fixtures for the audio + video window samplers (av_window / av_causal / av_causal_no_cfg)
from the REFERENCE on CPU.

Runs only where /root/reference exists.  On top of make_golden_mmdit's reconstruction of the MMDiT
model (``build``, ``mmdit_cfg``) and make_golden_sampler's shims (the CPU KV cache, our
``get_sd3_euler`` restatement, the ``owl_wms.configs`` stub):
  * ``owl_wms.utils`` is the reference's own module (batch_permute_to_length; B = 1, so its randperm
    is the identity) and ``tqdm`` a pass-through when the package is absent;
  * torch.randn_like draws are injected from seeded tensors in the reference's order -- per generated
    frame: video history [b, W-1, c, h, w], new video frame [b, c, h, w], audio history [b, W-1, ca],
    new audio frame [b, ca].
Two runs of each sampler:
  * ``model.*``: the tiny MMCFG model (det_init_ base seed 5000) under bf16 autocast, as the
    reference trainer's eval step runs it;
  * ``stub.*``: a stub core in fp32 that ignores the cache -- per frame video_pred = a x + b ts +
    c has_controls sum(mouse), audio likewise -- which pins the samplers' own arithmetic (history
    step, Euler updates, CFG mix, control windows) for the CPU test.
B = 1, 4 context frames, window_length 4, num_frames 2, n_steps 3, noise_prev 0.2, CFG 1.3.

    python tests/golden/make_golden_av_sampler.py          # av_sampler_tiny.pt
"""
import os
import sys
import types
from types import SimpleNamespace

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as G  # noqa: E402
import make_golden_mmdit as MM  # noqa: E402  (the reconstructed reference MMDiT)
import make_golden_sampler as S  # noqa: E402  (configs stub, CPU cache shim, our sd3 schedule)

from oracle.params import det_init_, det_tensor  # noqa: E402

try:
    import tqdm  # noqa: F401
except ImportError:
    _tq = types.ModuleType("tqdm")
    _tq.tqdm = lambda it, *a, **k: it
    sys.modules["tqdm"] = _tq

G._load("owl_wms.utils", "owl_wms/utils/__init__.py")
r_win = G._load("owl_wms.sampling.av_window", "owl_wms/sampling/av_window.py")

B, CTX, W, NEW, STEPS, NOISE_PREV, CFG_SCALE = 1, 4, 4, 2, 3, 0.2, 1.3
SAMPLERS = {"av_window": "AVWindowSampler", "av_causal": "CausalAVWindowSampler",
            "av_causal_no_cfg": "CausalAVWindowSamplerNoCFG"}
STUB = dict(av=0.35, bv=-0.2, cv=0.05, aa=-0.25, ba=0.3, ca=-0.04)


class StubCore(torch.nn.Module):
    """Per frame: video_pred = av x + bv ts + cv has_controls sum(mouse); audio likewise (fp32)."""

    def __init__(self, cfg):
        super().__init__()
        self.config = cfg

    def forward(self, x, audio, ts, mouse, btn, has_controls=None, kv_cache=None):
        hc = torch.ones(x.shape[0]) if has_controls is None else has_controls.float()
        m = mouse.float().sum(-1) * hc[:, None]
        pv = STUB["av"] * x + STUB["bv"] * ts[:, :, None, None, None] + STUB["cv"] * m[:, :, None, None, None]
        pa = STUB["aa"] * audio + STUB["ba"] * ts[:, :, None] + STUB["ca"] * m[:, :, None]
        return pv, pa


def _inputs(cfg, seed):
    bf = G.bf16_exact
    C, s, Ca = cfg.channels, cfg.sample_size, cfg.audio_channels
    x = bf(det_tensor((B, CTX, C, s, s), seed))
    audio = bf(det_tensor((B, CTX, Ca), seed + 1))
    mouse = bf(det_tensor((B, CTX, 2), seed + 2))
    g = torch.Generator().manual_seed(seed + 3)
    btn = (torch.rand((B, CTX, cfg.n_buttons), generator=g) < 0.5).float()
    like = []
    for f in range(NEW):
        k = seed + 10 + 4 * f
        like += [bf(det_tensor((B, W - 1, C, s, s), k)), bf(det_tensor((B, C, s, s), k + 1)),
                 bf(det_tensor((B, W - 1, Ca), k + 2)), bf(det_tensor((B, Ca), k + 3))]
    return x, audio, mouse, btn, like


def _run(core, sid, ins, autocast, **kw):
    x, audio, mouse, btn, like = ins
    sampler = getattr(r_win, SAMPLERS[sid])(n_steps=STEPS, cfg_scale=CFG_SCALE, window_length=W, num_frames=NEW,
                                            noise_prev=NOISE_PREV, **kw)
    with G.inject_rng(randn_like=like), torch.autocast("cpu", dtype=torch.bfloat16, enabled=autocast):
        out = sampler(core, x, audio, mouse, btn)
    return [None if t is None else t.float() for t in out]


def gen():
    cfg = MM.mmdit_cfg()
    out = {"dt": S.get_sd3_euler(STEPS), "stub.coeffs": dict(STUB),
           "settings": dict(B=B, ctx=CTX, window_length=W, num_frames=NEW, n_steps=STEPS, noise_prev=NOISE_PREV,
                            cfg_scale=CFG_SCALE)}
    model = det_init_(MM.build(cfg), base_seed=5000).eval()
    stub = StubCore(SimpleNamespace(**vars(cfg)))
    for tag, core, autocast, seed in (("model", model.core, True, 9100), ("stub", stub, False, 9200)):
        ins = _inputs(cfg, seed)
        for k, v in zip(("x", "audio", "mouse", "btn", "noise"), ins):
            out[f"{tag}.in.{k}"] = v
        for sid in SAMPLERS:
            res = _run(core, sid, ins, autocast)
            out[f"{tag}.{sid}.out"] = res
            print(tag, sid, [None if t is None else tuple(t.shape) for t in res])
        if tag == "stub":
            for sid in SAMPLERS:
                out[f"stub.{sid}.out_generated"] = _run(core, sid, ins, autocast, only_return_generated=True)
    return out


def main():
    torch.manual_seed(0)
    out = gen()
    path = os.path.join(HERE, "av_sampler_tiny.pt")
    torch.save(out, path)
    print(path, os.path.getsize(path) // 1024, "KiB", "dt", out["dt"].tolist())


if __name__ == "__main__":
    main()
