"""Model-level parity of the HIP path against the reference's own golden vectors.

Tolerances (bf16 autocast semantics on both sides):
  |d loss| / loss <= 5e-3, prediction rel-L2 <= 2e-2, parameter-gradient rel-L2 <= 2e-2 (bf16 inputs;
  measured <= 5e-3) and grad norms within 5e-2 (both modes),
  config-1 10-step loss trajectory within 2e-2 relative per step (GPU bf16 vs reference fp32).
"""
import math
import os
from types import SimpleNamespace

import pytest
import torch

from conftest import REPO, golden
from oracle.params import det_init_, det_tensor

pytestmark = pytest.mark.gpu
GR = golden("gamerft_tiny.pt")


def rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


TINY = dict(model_id="game_rft", sample_size=8, channels=32, n_layers=2, n_heads=2, d_model=128,
            tokens_per_frame=64, n_buttons=11, cfg_prob=0.1, n_frames=8, causal=True, uncond=False,
            backbone="dit", has_audio=False, rope_impl="motion", rope_ats_delta=2.0, local_window=2,
            global_window=None)


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _model(d_model=128):
    """TINY (d128 / 2 heads: head_dim 64); d_model=256 gives head_dim 128 (the dit_v4_5B attention
    shape) with the gamerft_d128 fixture's weights."""
    from owl_wms.configs import model_config
    from owl_wms.models.gamerft import GameRFT
    return det_init_(GameRFT(model_config(**dict(TINY, d_model=d_model))),
                     base_seed=1000 if d_model == 128 else 1100).cuda().train()


def _run(mode="bf16"):
    from owl_wms.models.flow import InjectedNoise
    p = f"gamerft.{mode}."
    m = _model()
    m.noise_source = InjectedNoise({"rand_b": GR[p + "in.rand_b"], "ts_raw": GR[p + "in.ts_raw"],
                                    "z": GR[p + "in.z"]})
    d = m(GR[p + "in.x"].cuda(), GR[p + "in.mouse"].cuda(), GR[p + "in.btn"].cuda(), GR[p + "in.doc_id"].cuda(),
          return_dict=True)
    d["diffusion_loss"].backward()
    return m, d


@pytest.mark.parametrize("mode", ["bf16", "fp32"])
def test_gamerft_loss_pred_grads_vs_reference(mode):
    m, d = _run(mode)
    p = f"gamerft.{mode}."
    assert torch.equal(d["cfg_mask"].cpu(), GR[p + "cfg_mask"])
    lref = GR[p + "loss"].item()
    assert abs(d["diffusion_loss"].item() - lref) / lref < 5e-3
    assert rel(d["pred_video"], GR[p + "pred"]) < 2e-2
    n_full = 0
    for i, (k, prm) in enumerate(sorted(m.named_parameters())):
        st = GR[p + "gradstat." + k]
        assert abs(prm.grad.double().norm().item() - st[3].item()) <= 5e-2 * st[3].item() + 1e-7, k
        # elementwise grads only vs the bf16-input reference: this path takes latents and ts in
        # bf16 on entry (the reference trainer's bf16 loader under autocast, rft_trainer.py:146,
        # 183-187); with fp32 inputs the reference keeps ts in fp32 and sin(1000 t) differs in
        # phase, which moves cancellation-heavy grads by 15-30 % (loss, pred and norms still agree)
        if mode == "bf16" and p + "grad." + k in GR:
            assert rel(prm.grad, GR[p + "grad." + k]) < 2e-2, k
            n_full += 1
    assert n_full >= 6 or mode == "fp32"


def test_gamerft_d128_loss_pred_grads_vs_reference():
    """Head dim 128 (the dit_v4_5B path: D = 128 attention, qk_rope and MotionRoPE tables, gradient
    checkpointing with the kept attention output) on a tiny d256 / 2-head GameRFT vs the reference's
    own fixture (tests/golden/make_golden.py d128); bf16 autocast semantics, SURVEY §8(c)."""
    from owl_wms.configs import model_config
    from owl_wms.models.flow import InjectedNoise
    from owl_wms.models.gamerft import GameRFT
    G = golden("gamerft_d128.pt")
    p = "d128.bf16."
    m = det_init_(GameRFT(model_config(**dict(TINY, d_model=256, gradient_checkpointing=True))),
                  base_seed=1100).cuda().train()
    assert [[k, list(v.shape)] for k, v in m.state_dict().items()] == G["d128.schema"]
    m.noise_source = InjectedNoise({"rand_b": G[p + "in.rand_b"], "ts_raw": G[p + "in.ts_raw"], "z": G[p + "in.z"]})
    d = m(G[p + "in.x"].cuda(), G[p + "in.mouse"].cuda(), G[p + "in.btn"].cuda(), G[p + "in.doc_id"].cuda(),
          return_dict=True)
    d["diffusion_loss"].backward()
    assert torch.equal(d["cfg_mask"].cpu(), G[p + "cfg_mask"])
    lref = G[p + "loss"].item()
    assert abs(d["diffusion_loss"].item() - lref) / lref < 5e-3
    assert rel(d["pred_video"], G[p + "pred"]) < 2e-2
    n = 0
    for i, (k, prm) in enumerate(sorted(m.named_parameters())):
        st = G[p + "gradstat." + k]
        assert abs(prm.grad.double().norm().item() - st[3].item()) <= 5e-2 * st[3].item() + 1e-7, k
        if p + "grad." + k in G:
            assert rel(prm.grad, G[p + "grad." + k]) < 2e-2, (k, rel(prm.grad, G[p + "grad." + k]))
            n += 1
    assert n >= 6


def test_muon_step_on_reference_grads_gpu():
    """muon.py:66-84 on libowlk NS, fed the reference's own grads.

    The library NS rounds as the eager reference does, so the update is pinned to both the oracle
    Muon step and the reference's own update (muon.after.full); NS's five chaotic bf16 iterations
    amplify the remaining fp32 accumulation-order differences to a few % rel-L2 on this [384, 128]
    gradient (0.1 in round 1, with the scalar applied after the product)."""
    from oracle.ref_model import muon_step_1rank
    from owl_wms.muon import Muon
    k = "core.transformer.blocks.0.attn.qkv.weight"
    m = _model()
    prm = dict(m.named_parameters())[k]
    p0 = prm.detach().clone()
    prm.grad = GR["gamerft.fp32.grad." + k].cuda().clone()
    Muon([prm], lr=1e-3, momentum=0.95, rank=0, world_size=1).step()
    q = torch.nn.Parameter(p0.cpu().clone())
    q.grad = GR["gamerft.fp32.grad." + k].clone()
    muon_step_1rank([q], {}, lr=1e-3, momentum=0.95)
    r_oracle = rel(prm.detach() - p0, q.detach() - p0.cpu())
    ref = GR["muon.after.full." + k]
    r_ref = rel(prm.detach() - p0, ref - p0.cpu())
    assert r_oracle < 5e-2 and r_ref < 5e-2, (r_oracle, r_ref)


def test_combined_optimizer_partition_and_step():
    from owl_wms.muon import init_muon
    m, _ = _run("fp32")
    opt = init_muon(m, rank=0, world_size=1, lr=1e-3, momentum=0.95, adamw_lr=1e-4, adamw_wd=1e-4,
                    adamw_eps=1e-15, adamw_betas=[0.9, 0.95],
                    adamw_keys=["core.proj_in", "core.proj_out.proj", "core.t_embed", "core.control_embed", "gate",
                                "adaln"])
    names = {id(p): n for n, p in m.named_parameters()}
    muon_names = sorted(names[id(p)] for g in opt.muon.param_groups for p in g["params"])
    assert muon_names == sorted(GR["muon.muon_params"])
    before = {n: p.detach().clone() for n, p in m.named_parameters()}
    grads = {n: p.grad.detach().clone() for n, p in m.named_parameters()}
    opt.step()
    # Muon param: NS amplifies small-singular-value directions ~3.4^5x, so grads that differ by a
    # few % (bf16 vs fp32 reference) give O(1) elementwise differences; the update's scale is fixed
    k = "core.transformer.blocks.0.attn.qkv.weight"
    upd = dict(m.named_parameters())[k].detach() - before[k] * (1 - 1e-3 * 0.01)
    ref = GR["muon.after.full." + k] - before[k].cpu() * (1 - 1e-3 * 0.01)
    assert abs(upd.norm().item() / ref.norm().item() - 1) < 0.1
    # AdamW param, first step: update = -lr * g / (|g| + eps) - lr * wd * p  (sign of the grad)
    ka = "core.transformer.blocks.0.adaln1.fc.weight"
    ua = dict(m.named_parameters())[ka].detach() - before[ka] * (1 - 1e-4 * 1e-4)
    agree = (torch.sign(ua) == -torch.sign(grads[ka])).float().mean().item()
    assert agree > 0.999 and abs(ua.abs().mean().item() / 1e-4 - 1) < 1e-2
    sd = opt.state_dict()
    assert set(sd) == {"adamw", "muon"}


def test_audio_config1_trajectory():
    """BASELINE configs[0]: 2-layer/128-d audio DiT, batch 1, 10 AdamW steps vs reference losses."""
    from owl_wms.configs import model_config
    from owl_wms.models.audiorft import AudioRFT
    from owl_wms.models.flow import InjectedNoise
    ref = golden("audio_traj.pt")["audio.losses"]
    cfg = model_config(model_id="audio_rft", sample_size=120, channels=64, n_layers=2, n_heads=2, d_model=128,
                       tokens_per_frame=1, n_frames=10000, cfg_prob=0.0, causal=True, uncond=True, backbone="dit",
                       has_audio=True, rope_impl="audio1d", local_window=16, global_window=None)
    m = det_init_(AudioRFT(cfg), base_seed=3000).cuda().train()
    from owl_wms.muon import FusedAdamW  # the trainer's AdamW (owlk_adamw)
    opt = FusedAdamW(m.parameters(), lr=1e-4, betas=(0.9, 0.999), weight_decay=0.01, eps=1e-8)
    for step in range(10):
        m.noise_source = InjectedNoise({"ts_raw": det_tensor((1, 120), 3200 + step),
                                        "z": det_tensor((1, 120, 64), 3300 + step)})
        loss = m(det_tensor((1, 120, 64), 3100 + step).cuda())
        loss.backward()
        torch.nn.utils.clip_grad_norm_(m.parameters(), max_norm=10.0)
        opt.step()
        opt.zero_grad(set_to_none=True)
        assert abs(loss.item() - ref[step].item()) / ref[step].item() < 2e-2, (step, loss.item(), ref[step].item())


@pytest.mark.parametrize("d_model", [128, 256])
def test_kv_cache_decode_matches_full_forward(d_model):
    """SURVEY §4 invariant: cached decode of the last frame == the full masked forward (head_dim 64
    and, at d_model 256, 128: the dit_v4_5B eval path, attn.py:86-107)."""
    from owl_wms.nn.kv_cache import KVCache
    m = _model(d_model).eval()
    core = m.core
    B, n = 1, 8
    x = det_tensor((B, n, 32, 8, 8), 900).cuda()
    t = torch.sigmoid(det_tensor((B, n), 901)).cuda().bfloat16()
    mouse = det_tensor((B, n, 2), 902).cuda().bfloat16()
    btn = (det_tensor((B, n, 11), 903) > 0).cuda().bfloat16()
    with torch.no_grad():
        full = core(x, t, mouse, btn)
        cache = KVCache(core.config)
        cache.reset(B)
        cache.enable_cache_updates()
        core(x[:, :-1], t[:, :-1], mouse[:, :-1], btn[:, :-1], kv_cache=cache)
        cache.disable_cache_updates()
        core.transformer.enable_decoding()
        last = core(x[:, -1:], t[:, -1:], mouse[:, -1:], btn[:, -1:], kv_cache=cache)
        core.transformer.disable_decoding()
    # the tiny config's local window is 2 frames: decode keeps the last 2 frames of keys, exactly
    # what the mask allows the last frame to see in the full pass
    assert rel(last[:, 0], full[:, -1]) < 2e-2


MMCFG = dict(model_id="game_rft_audio", sample_size=8, channels=32, audio_channels=16, n_layers=2, n_heads=2,
             d_model=128, tokens_per_frame=65, n_buttons=11, n_mouse_axes=2, cfg_prob=0.1, n_frames=6, causal=True,
             uncond=False, backbone="mmdit", local_window=2, global_window=4, has_audio=True)


def test_mmdit_loss_pred_grads_vs_reference():
    """BASELINE configs[3] path (two-stream MMDiT, tpf 65 joint attention, shared modulation) vs the
    reconstructed reference (tests/golden/make_golden_mmdit.py), bf16 autocast semantics."""
    from owl_wms.configs import model_config
    from owl_wms.models.flow import InjectedNoise
    from owl_wms.models.gamerft_audio import GameRFTAudio
    MM = golden("mmdit_tiny.pt")
    p = "mmdit.bf16."
    m = det_init_(GameRFTAudio(model_config(**MMCFG)), base_seed=5000).cuda().train()
    m.noise_source = InjectedNoise({"rand_b": MM[p + "in.rand_b"], "ts_raw": MM[p + "in.ts_raw"],
                                    "z": [MM[p + "in.z_video"], MM[p + "in.z_audio"]]})
    d = m(MM[p + "in.x"].cuda(), MM[p + "in.audio"].cuda(), MM[p + "in.mouse"].cuda(), MM[p + "in.btn"].cuda(),
          return_dict=True)
    d["diffusion_loss"].backward()
    assert torch.equal(d["cfg_mask"].cpu(), MM[p + "cfg_mask"])
    for k in ("diffusion_loss", "video_loss", "audio_loss"):
        assert abs(d[k].item() - MM[p + k].item()) <= 5e-3 * MM[p + k].item(), (k, d[k].item(), MM[p + k].item())
    assert rel(d["pred_video"], MM[p + "pred_video"]) < 2e-2
    assert rel(d["pred_audio"], MM[p + "pred_audio"]) < 2e-2
    n = 0
    for i, (k, prm) in enumerate(sorted(m.named_parameters())):
        st = MM[p + "gradstat." + k]
        assert abs(prm.grad.double().norm().item() - st[3].item()) <= 5e-2 * st[3].item() + 1e-7, k
        if p + "grad." + k in MM:
            assert rel(prm.grad, MM[p + "grad." + k]) < 2e-2, (k, rel(prm.grad, MM[p + "grad." + k]))
            n += 1
    assert n >= 10


@pytest.mark.parametrize("n_ctx", [5, 3])
def test_mmdit_kv_cache_decode_matches_full_forward(n_ctx):
    """MMDiT cache path (mmattn.py:46-72): the context frames cached, then the next joint frame(s)
    decoded against the cache (RoPE at the cached offset, frame mask with q_offset = cached tokens,
    local window 2 / global window 4 frames) == the same frames of the full masked forward."""
    from owl_wms.configs import model_config
    from owl_wms.models.gamerft_audio import GameRFTAudio
    from owl_wms.nn.kv_cache import KVCache
    m = det_init_(GameRFTAudio(model_config(**MMCFG)), base_seed=5000).cuda().eval()
    core = m.core
    B, n = 2, 6
    x = det_tensor((B, n, 32, 8, 8), 910).cuda().bfloat16()
    au = det_tensor((B, n, 16), 911).cuda().bfloat16()
    t = torch.sigmoid(det_tensor((B, n), 912)).cuda().bfloat16()
    mouse = det_tensor((B, n, 2), 913).cuda().bfloat16()
    btn = (det_tensor((B, n, 11), 914) > 0).cuda().bfloat16()
    with torch.no_grad():
        fv, fa = core(x, au, t, mouse, btn)
        cache = KVCache(core.config)
        cache.reset(B)
        cache.enable_cache_updates()
        cv, ca = core(x[:, :n_ctx], au[:, :n_ctx], t[:, :n_ctx], mouse[:, :n_ctx], btn[:, :n_ctx], kv_cache=cache)
        cache.disable_cache_updates()
        assert cache.length_at(0) == n_ctx * 65
        lv, la = core(x[:, n_ctx:], au[:, n_ctx:], t[:, n_ctx:], mouse[:, n_ctx:], btn[:, n_ctx:], kv_cache=cache)
    assert rel(cv, fv[:, :n_ctx]) < 1e-5 and rel(ca, fa[:, :n_ctx]) < 1e-5  # the context pass is the masked forward
    assert rel(lv, fv[:, n_ctx:]) < 2e-2 and rel(la, fa[:, n_ctx:]) < 2e-2


@pytest.mark.parametrize("heads", [4, 2])
def test_mmdit_joint_rows_in_place_equals_frame_mux(heads, monkeypatch):
    """MMDiTBlockFn with the joint 65-token frame layout read and written in place (video GEMMs on
    frame-strided rows, owlk_gemm_frames / owlk_colsum_frames; audio rows as plain strided views)
    == the same block through the frame_mux interleave / split copies (mmattn.py:54-60, 77-80):
    outputs and every gradient within bf16 GEMM tolerance (d 256, head_dim 64 and 128)."""
    from owl_wms.configs import model_config
    from owl_wms.models.gamerft_audio import GameRFTAudio
    from owl_wms.nn import mmattn
    cfg = dict(MMCFG, d_model=256, n_heads=heads, n_frames=8)
    from owl_wms.utils.grad_reducer import GradReducer
    res = []
    # in place with the gradients written straight into GradReducer bucket views (the sinks the
    # audio side stream's backward writes before lane.join, then reports), in place into .grad,
    # and the frame_mux path
    for inplace, reducer in ((True, True), (True, False), (False, False)):
        if not inplace:
            monkeypatch.setattr(mmattn, "_in_place_ok", lambda *a: False)
        m = det_init_(GameRFTAudio(model_config(**cfg)), base_seed=5100).cuda().train()
        red = GradReducer(m.parameters(), world_size=1) if reducer else None
        B, n = 2, 8
        x = det_tensor((B, n, 32, 8, 8), 920).cuda().bfloat16()
        au = det_tensor((B, n, 16), 921).cuda().bfloat16()
        t = torch.sigmoid(det_tensor((B, n), 922)).cuda().bfloat16()
        mouse = det_tensor((B, n, 2), 923).cuda().bfloat16()
        btn = (det_tensor((B, n, 11), 924) > 0).cuda().bfloat16()
        if red is not None:
            red.begin(False)
        pv, pa = m.core(x, au, t, mouse, btn)
        (pv.float().square().mean() + pa.float().square().mean()).backward()
        if red is not None:
            red.finish()
        res.append((pv.float(), pa.float(),
                    {k: p.grad.float().clone() for k, p in m.named_parameters() if p.grad is not None}))
    (v0, a0, g0), (v1, a1, g1), (v2, a2, g2) = res
    assert torch.equal(v0, v1) and torch.equal(a0, a1)
    assert set(g1) <= set(g0)  # the reducer's bucket views exist for every parameter
    for k in g1:  # same kernels, same order: the bucket-view writes give the same bits
        assert torch.equal(g0[k], g1[k]), k
    for k in set(g0) - set(g1):  # parameters the loss does not reach: zero in their bucket view
        assert not g0[k].any(), k
    assert rel(v1, v2) < 1e-2 and rel(a1, a2) < 1e-2
    assert g1.keys() == g2.keys() and len(g1) > 20
    for k in g2:
        assert rel(g1[k], g2[k]) < 2e-2, (k, rel(g1[k], g2[k]))


@pytest.mark.parametrize("n", [1, 2, 4, 5])
def test_mmdit_few_frames_in_place_equals_frame_mux(n, monkeypatch):
    """MMDiT forward + backward over 1-5 frames (mmdit_v2's d % 256 == 0 in-place layout; no KV
    cache): at <= 4 frames the block takes the frame_mux path (its video GEMMs would be decode-
    sized), at 5 the in-place one; either equals the frame_mux path."""
    from owl_wms.configs import model_config
    from owl_wms.models.gamerft_audio import GameRFTAudio
    from owl_wms.nn import mmattn
    cfg = dict(MMCFG, d_model=256, n_heads=4, n_frames=n)
    res = []
    for force_mux in (False, True):
        if force_mux:
            monkeypatch.setattr(mmattn, "_in_place_ok", lambda *a: False)
        m = det_init_(GameRFTAudio(model_config(**cfg)), base_seed=5100).cuda().train()
        x = det_tensor((1, n, 32, 8, 8), 930).cuda().bfloat16()
        au = det_tensor((1, n, 16), 931).cuda().bfloat16()
        t = torch.sigmoid(det_tensor((1, n), 932)).cuda().bfloat16()
        mouse = det_tensor((1, n, 2), 933).cuda().bfloat16()
        btn = (det_tensor((1, n, 11), 934) > 0).cuda().bfloat16()
        pv, pa = m.core(x, au, t, mouse, btn)
        (pv.float().square().mean() + pa.float().square().mean()).backward()
        res.append((pv.float(), pa.float(), {k: p.grad.float() for k, p in m.named_parameters()
                                             if p.grad is not None}))
    (v1, a1, g1), (v2, a2, g2) = res
    assert torch.isfinite(v1).all() and torch.isfinite(a1).all()
    assert rel(v1, v2) < 1e-2 and rel(a1, a2) < 1e-2
    for k in g2:
        assert rel(g1[k], g2[k]) < 2e-2, (k, rel(g1[k], g2[k]))


class _Draws:
    """Replay torch.randn / randn_like draws (reference order) on the draw's device/dtype."""

    def __init__(self, randn=(), like=()):
        self.q = {"randn": list(randn), "like": list(like)}

    def __enter__(self):
        self.saved = (torch.randn, torch.randn_like)

        def randn(*shape, device=None, dtype=None, **kw):
            return self.q["randn"].pop(0).to(device=device, dtype=dtype or torch.float32)

        def like(x, **kw):
            return self.q["like"].pop(0).to(device=x.device, dtype=x.dtype)

        torch.randn, torch.randn_like = randn, like
        return self

    def __exit__(self, *exc):
        torch.randn, torch.randn_like = self.saved
        assert not any(self.q.values()), "unconsumed draws"


def test_av_caching_sampler_vs_reference():
    """AVCachingSamplerV2 (av_caching_v2.py:24-144): 4 context frames + 3 generated, 2 Euler steps,
    CFG 1.3, through the libowlk KV-cache decode path; sampled latents within 2e-2."""
    from owl_wms.sampling import get_sampler_cls
    S = golden("sampler_tiny.pt")
    m = _model().eval()
    sampler = get_sampler_cls("av_caching")(n_steps=2, cfg_scale=1.3, num_frames=3, noise_prev=0.2)
    with _Draws(like=S["av.noise"]):
        out = sampler(m.core, S["av.in.x"].cuda(), S["av.in.mouse"].cuda(), S["av.in.btn"].cuda())
    assert out.shape == S["av.out"].shape
    assert rel(out[:, :4], S["av.out"][:, :4]) == 0.0
    assert rel(out[:, 4:], S["av.out"][:, 4:]) < 2e-2


def test_av_caching_sampler_head_dim_128_vs_reference():
    """AVCachingSamplerV2 (av_caching_v2.py:47-144) at head_dim 128 -- the attention width of
    configs/dit_v4_5B.yml -- against the reference sampler's own latents (tests/golden/
    make_golden_sampler.py d128: the gamerft_d128 weights, 4 context + 3 generated frames, 2 Euler
    steps, CFG 1.3, bf16 autocast); through the D = 128 decode attention.  Within 2e-2."""
    from owl_wms.sampling import get_sampler_cls
    S = golden("sampler_d128.pt")
    m = _model(d_model=256).eval()
    sampler = get_sampler_cls("av_caching")(n_steps=2, cfg_scale=1.3, num_frames=3, noise_prev=0.2)
    with _Draws(like=S["av128.noise"]):
        out = sampler(m.core, S["av128.in.x"].cuda(), S["av128.in.mouse"].cuda(), S["av128.in.btn"].cuda())
    assert out.shape == S["av128.out"].shape
    assert rel(out[:, :4], S["av128.out"][:, :4]) == 0.0
    assert rel(out[:, 4:], S["av128.out"][:, 4:]) < 2e-2


def test_audio_caching_sampler_vs_reference():
    from owl_wms.configs import model_config
    from owl_wms.models.audiorft import AudioRFT
    from owl_wms.sampling import get_sampler_cls
    S = golden("sampler_tiny.pt")
    cfg = model_config(model_id="audio_rft", sample_size=120, channels=64, n_layers=2, n_heads=2, d_model=128,
                       tokens_per_frame=1, n_frames=10000, cfg_prob=0.0, causal=True, uncond=True, backbone="dit",
                       has_audio=True, rope_impl="audio1d", local_window=16, global_window=None)
    m = det_init_(AudioRFT(cfg), base_seed=3000).cuda().eval()
    sampler = get_sampler_cls("audio_caching")(n_steps=2, num_tokens=3, noise_prev=0.2)
    with _Draws(randn=S["audio.noise_randn"], like=S["audio.noise_like"]):
        out = sampler(m.core, S["audio.in.x"].cuda())
    assert out.shape == S["audio.out"].shape
    assert rel(out[:, 8:], S["audio.out"][:, 8:]) < 2e-2


def test_checkpointed_blocks_reuse_attention():
    """gradient_checkpointing (dit_v4_5B): the re-run of each block inside backward takes the
    attention output kept from the first pass, so one attention forward runs per layer per step;
    loss and every gradient equal the non-checkpointed step (the re-run is bit-exact; fp32-atomic
    bias-gradient sums aside, hence a 1e-6 bound).  lean_activations (h1, h2, roped q / k and
    silu(a_pre) recomputed in the backward of non-checkpointed blocks) gives the same step too."""
    from owl_wms import _lib
    from owl_wms.configs import model_config
    from owl_wms.models.flow import InjectedNoise
    from owl_wms.models.gamerft import GameRFT
    p = "gamerft.bf16."
    grads, losses, nfwd = [], [], []
    runs = ((False, None, False), (True, None, False), (True, 1, False), (False, None, True), (True, 1, True))
    for ckpt, n_ck, lean in runs:  # n_ck: checkpoint_layers (first n only)
        kw = dict(TINY, gradient_checkpointing=ckpt, lean_activations=lean)
        if n_ck is not None:
            kw["checkpoint_layers"] = n_ck
        m = det_init_(GameRFT(model_config(**kw)), base_seed=1000).cuda().train()
        m.noise_source = InjectedNoise({"rand_b": GR[p + "in.rand_b"], "ts_raw": GR[p + "in.ts_raw"],
                                        "z": GR[p + "in.z"]})
        _lib.profile_begin()
        loss = m(GR[p + "in.x"].cuda(), GR[p + "in.mouse"].cuda(), GR[p + "in.btn"].cuda(),
                 GR[p + "in.doc_id"].cuda())
        loss.backward()
        prof = _lib.profile_end()
        nfwd.append(sum(n for k, (n, _, _) in prof.items() if k.startswith("attn_fwd")))
        losses.append(loss.item())
        grads.append({k: q.grad.detach().clone() for k, q in m.named_parameters() if q.grad is not None})
    assert nfwd == [TINY["n_layers"]] * len(runs)
    for j in range(1, len(runs)):
        assert losses[0] == losses[j]
        assert grads[0].keys() == grads[j].keys()
        for k in grads[0]:
            assert rel(grads[j][k], grads[0][k]) < 1e-6, k


def _packed_table(path, lens, seed=0):
    """A small NpyTable of dit-shaped documents (tiny config: 32 ch, 8x8, 11 buttons)."""
    import numpy as np
    from owl_wms.data.npy_table import NpyTable
    rs = np.random.RandomState(seed)
    cols = ["depth_latent", "mouse", "buttons", "tarball", "pt_idx", "missing", "truncated", "seq_len"]
    t = NpyTable(str(path), columns=cols, array_columns=["depth_latent", "mouse", "buttons"])
    for i, n in enumerate(lens):
        t.append(depth_latent=rs.randn(n, 32, 8, 8).astype(np.float32), mouse=rs.randn(n, 2).astype(np.float32),
                 buttons=(rs.rand(n, 11) < 0.5).astype(np.float32), tarball="t", pt_idx=i, missing=False,
                 truncated=False, seq_len=n)


def test_packed_batch_loss_grads_vs_oracle(tmp_path):
    """A sequence-packed window (3 documents inside 8 frames) through the HIP
    path against the CPU oracle on the same batch and injected noise; SURVEY §8(c) tolerances."""
    from oracle import ref_model as M
    from owl_wms.data import get_loader
    from owl_wms.models.flow import InjectedNoise
    _packed_table(tmp_path, [3, 2, 6, 4, 5])
    loader = get_loader("sequence_packing", 1, dataset_path=str(tmp_path), window_length=8,
                        batch_columns=["depth_latent", "mouse", "buttons"], num_workers=0)
    batches = list(loader)
    assert len(batches) == 20 // 8
    x, mouse, btn, doc = batches[0]
    assert x.dtype == torch.bfloat16 and doc.shape == (1, 8) and len(doc.unique()) >= 2
    B = 1
    noise = {"rand_b": torch.tensor([0.05]), "ts_raw": det_tensor((B, 8), 4).bfloat16().float(),
             "z": det_tensor((B, 8, 32, 8, 8), 5).bfloat16().float()}
    m = _model()
    m.noise_source = InjectedNoise(noise)
    loss = m(x.cuda(), mouse.cuda(), btn.cuda(), doc.cuda())
    loss.backward()
    from owl_wms.configs import model_config  # noqa: F401
    ref = det_init_(M.GameRFT(SimpleNamespace(**TINY)), base_seed=1000).train()
    with torch.autocast("cpu", dtype=torch.bfloat16):
        rl, _, _ = ref(x, mouse, btn, doc, noise)
    rl.backward()
    assert abs(loss.item() - rl.item()) / rl.item() <= 5e-3
    for name in ("core.transformer.blocks.0.attn.qkv.weight", "core.transformer.blocks.1.mlp.fc1.weight"):
        g = dict(m.named_parameters())[name].grad
        rg = dict(ref.named_parameters())[name].grad
        assert rel(g, rg) <= 2e-2, name


def test_trainer_reads_packed_table(tmp_path):
    """train.py's trainer on a sequence_packing config whose dataset_path is an NpyTable: two
    optimizer steps (accum 2) on packed multi-document windows, finite losses, EMA updated."""
    import yaml
    from owl_wms.configs import Config
    from owl_wms.trainers import get_trainer_cls
    _packed_table(tmp_path / "table", [3, 2, 6, 4, 5, 7, 9])
    cfg = {"model": dict(TINY), "train": {
        "trainer_id": "rft", "data_id": "sequence_packing",
        "data_kwargs": {"window_length": 8, "dataset_path": str(tmp_path / "table"),
                        "batch_columns": ["depth_latent", "mouse", "buttons"], "num_workers": 0},
        "target_batch_size": 2, "batch_size": 1, "epochs": 10, "opt": "Muon",
        "opt_kwargs": yaml.safe_load(open(os.path.join(REPO, "configs", "dit_v4.yml")))["train"]["opt_kwargs"],
        "checkpoint_dir": str(tmp_path / "ckpt"), "save_interval": 1000,
        "sample_interval": 100000, "vae_scale": 1.0}, "wandb": {"project": "p", "run_name": "r"}}
    (tmp_path / "c.yml").write_text(yaml.safe_dump(cfg))
    c = Config.from_yaml(str(tmp_path / "c.yml"))
    tr = get_trainer_cls("rft")(c.train, c.wandb, c.model, 0, 0, 1)
    tr.max_steps = 2
    tr.train()
    assert len(tr.history) == 2
    assert all(torch.isfinite(torch.tensor(h["diffusion_loss"])) for h in tr.history)


@pytest.mark.parametrize("n_steps,cfg,custom,d_model,device_state", [
    pytest.param(4, 1.3, None, 128, True, id="4-1.3-None-128"),
    pytest.param(3, 1.0, None, 128, True, id="3-1.0-None-128"),
    pytest.param(3, 1.3, [1.0, 0.7, 0.3], 128, True, id="3-1.3-custom2-128"),
    pytest.param(3, 1.3, None, 256, True, id="3-1.3-None-256"),
    pytest.param(3, 1.3, None, 128, False, id="3-1.3-None-128-host")])
def test_graphed_decode_equals_eager(n_steps, cfg, custom, d_model, device_state):
    """compile_on_decode: the per-frame Euler steps replayed from a HIP graph give the same sampled
    latents as the eager loop, bit for bit (same kernels, same buffers' contents, same order);
    also with a custom schedule (its deltas live in device memory the graph reads) and at head_dim
    128 (d_model 256: dit_v4_5B's decode shape).  The "host" case sets the sampler's device_state
    False: the host-position path, one capture per frame (AVCachingSamplerV2._euler_graphed), a warm
    first frame and all-replay later frames."""
    from owl_wms.sampling import get_sampler_cls
    m = _model(d_model).eval()
    g = torch.Generator().manual_seed(5)
    x = torch.randn(2, 4, 32, 8, 8, generator=g).bfloat16().cuda()
    mouse = torch.randn(2, 8, 2, generator=g).bfloat16().cuda()
    btn = (torch.rand(2, 8, 11, generator=g) < 0.5).bfloat16().cuda()
    outs = []
    for graphed in (False, True):
        torch.manual_seed(123)
        s = get_sampler_cls("av_caching")(n_steps=n_steps, cfg_scale=cfg, num_frames=4, noise_prev=0.2,
                                          custom_schedule=custom)
        s.device_state = device_state
        outs.append(s(m.core, x, mouse, btn, compile_on_decode=graphed))
    assert outs[0].shape == (2, 8, 32, 8, 8)
    assert torch.equal(outs[0], outs[1])


@pytest.mark.parametrize("d_model", [128, 256])
def test_device_state_decode_matches_host_state(d_model):
    """AVCachingSamplerV2 with the cache position on the device (owlk_qk_rope_fwd_kv_dev +
    owlk_attn_decode_fwd: one captured step for every frame) == the host-position decode path
    (lengths baked into each launch), eager, within attention summation order; the graphed
    device-state run equals its eager run bit for bit (test_graphed_decode_equals_eager).
    d_model 256 = head_dim 128 (dit_v4_5B)."""
    from owl_wms.sampling import get_sampler_cls
    m = _model(d_model).eval()
    g = torch.Generator().manual_seed(7)
    # 3 context + 5 new frames = the model's n_frames (8): every RoPE position lies in the table
    # (round 4 ran 4 + 5 here, past the table: the rope kernels read 64 rows beyond it, which is
    # what faulted in profiles/r4ac_gemm_nowait_tests_fault.log; such calls now raise)
    x = torch.randn(2, 3, 32, 8, 8, generator=g).bfloat16().cuda()
    mouse = torch.randn(2, 8, 2, generator=g).bfloat16().cuda()
    btn = (torch.rand(2, 8, 11, generator=g) < 0.5).bfloat16().cuda()
    outs = []
    for dev in (False, True):
        torch.manual_seed(321)
        s = get_sampler_cls("av_caching")(n_steps=4, cfg_scale=1.3, num_frames=5, noise_prev=0.2)
        s.device_state = dev
        outs.append(s(m.core, x, mouse, btn).float())
    assert rel(outs[1], outs[0]) < 2e-2
    assert torch.isfinite(outs[1]).all()


def test_fused_handoff_timeout_reaches_the_loss(monkeypatch):
    """A timed-out dQ hand-off of the single-pass backward (forced: kernels.FUSED_FAIL_TEST, variant
    bit 6) is not a silent wrong gradient: the qkv weight gradients come out non-finite, and after one
    Muon / AdamW step (rft_trainer.py:186-199's consumer of the gradients) the next loss is NaN."""
    from owl_wms import kernels
    from owl_wms.muon import init_muon
    monkeypatch.setattr(kernels, "FUSED_FAIL_TEST", True)
    m, d = _run("bf16")
    assert torch.isfinite(d["diffusion_loss"]).item()  # the forward is untouched
    bad = [k for k, p in m.named_parameters() if p.grad is not None and not torch.isfinite(p.grad).all()]
    assert any("qkv" in k for k in bad), bad
    opt = init_muon(m, lr=1e-3, momentum=0.95, adamw_lr=1e-4, adamw_wd=1e-4, adamw_eps=1e-15,
                    adamw_betas=[0.9, 0.95], adamw_keys=["core.proj_in", "core.proj_out.proj", "core.t_embed",
                                                         "core.control_embed", "gate", "adaln"])
    opt.step()
    monkeypatch.setattr(kernels, "FUSED_FAIL_TEST", False)
    m.zero_grad(set_to_none=True)
    d2 = m(GR["gamerft.bf16.in.x"].cuda(), GR["gamerft.bf16.in.mouse"].cuda(), GR["gamerft.bf16.in.btn"].cuda(),
           GR["gamerft.bf16.in.doc_id"].cuda(), return_dict=True)
    assert torch.isnan(d2["diffusion_loss"]).item()


@pytest.mark.parametrize("device_state,graphed", [(False, False), (True, False), (True, True)])
def test_decode_past_rope_table_raises(device_state, graphed):
    """Decoding past config.n_frames frames: the reference's rope slices cos[offset:offset + n] short
    and its rotation fails (rope.py:46-49); this path raises before any kernel reads past the table
    (4 context + 5 new frames with n_frames 8), on the eager, device-state and replayed paths, and the
    GPU is left healthy (the sync below)."""
    from owl_wms.sampling import get_sampler_cls
    m = _model(128).eval()
    g = torch.Generator().manual_seed(7)
    x = torch.randn(1, 4, 32, 8, 8, generator=g).bfloat16().cuda()
    mouse = torch.randn(1, 9, 2, generator=g).bfloat16().cuda()
    btn = (torch.rand(1, 9, 11, generator=g) < 0.5).bfloat16().cuda()
    s = get_sampler_cls("av_caching")(n_steps=2, cfg_scale=1.3, num_frames=5, noise_prev=0.2)
    s.device_state = device_state
    with pytest.raises(RuntimeError, match="RoPE positions"):
        s(m.core, x, mouse, btn, compile_on_decode=graphed)
    torch.cuda.synchronize()


def _dp_worker(rank, ws, port, q):
    import os as _os
    _os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=ws)  # gloo on GPU tensors: one card, 2 ranks
    try:
        from owl_wms.muon import init_muon
        from owl_wms.utils.grad_reducer import GradReducer
        torch.cuda.set_device(0)
        m = _model()
        kw = dict(lr=1e-3, momentum=0.95, adamw_lr=1e-4, adamw_wd=1e-4, adamw_eps=1e-15, adamw_betas=[0.9, 0.95],
                  adamw_keys=["core.proj_in", "core.proj_out.proj", "core.t_embed", "core.control_embed", "gate",
                              "adaln"])
        opt = init_muon(m, rank=rank, world_size=ws, **kw)
        red = GradReducer(m.parameters(), world_size=ws)
        g = torch.Generator().manual_seed(100 + rank)
        for micro in range(2):
            red.begin(sync=micro == 1)
            x = torch.randn(1, 8, 32, 8, 8, generator=g).bfloat16().cuda()
            mouse = torch.randn(1, 8, 2, generator=g).bfloat16().cuda()
            btn = (torch.rand(1, 8, 11, generator=g) < 0.5).bfloat16().cuda()
            (m(x, mouse, btn, torch.zeros(1, 8, dtype=torch.long).cuda()) / 2).backward()
            red.finish()
        opt.step()
        torch.cuda.synchronize()
        q.put((rank, {k: p.detach().cpu().numpy() for k, p in m.named_parameters()}))  # plain bytes
    finally:
        dist.destroy_process_group()


def test_data_parallel_step_two_ranks_on_gpu():
    """The N > 1 training step on GPU tensors (2 ranks sharing the card over gloo; RCCL needs one
    GPU per rank): bucketed grad all-reduce, distributed Muon (round-robin NS + all_gather) and
    AdamW on the HIP passes -- replicas must be bit-identical afterwards."""
    import os as _os
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 29700 + _os.getpid() % 1000
    procs = [ctx.Process(target=_dp_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = dict(q.get(timeout=100) for _ in range(2))
    for p in procs:
        p.join(30)
        assert p.exitcode == 0
    assert res[0].keys() == res[1].keys()
    for k in res[0]:
        assert (res[0][k] == res[1][k]).all(), k


def _tiny_trainer_cfg(tmp_path, model_over=None, **train_over):
    import yaml
    from owl_wms.configs import Config
    train = {"trainer_id": "rft", "data_id": "synthetic", "data_kwargs": {"window_length": 8},
             "target_batch_size": 2, "batch_size": 1, "epochs": 1, "opt": "Muon",
             "opt_kwargs": yaml.safe_load(open(os.path.join(REPO, "configs", "dit_v4.yml")))["train"]["opt_kwargs"],
             "checkpoint_dir": str(tmp_path / "ckpt"), "save_interval": 2, "sample_interval": 10 ** 9,
             "vae_scale": 1.0, "seed": 77}
    train.update(train_over)
    (tmp_path / "c.yml").write_text(yaml.safe_dump({"model": dict(TINY, **(model_over or {})), "train": train,
                                                    "wandb": {"project": "p", "run_name": "r"}}))
    return Config.from_yaml(str(tmp_path / "c.yml"))


def _step_keyed_trainer():
    """RFTTrainer whose synthetic batches are keyed by the global optimizer step (a resumed run
    restarts its loader, as the reference's does; keying by step gives both runs the same data)."""
    from owl_wms.data import synthetic_video_batch
    from owl_wms.trainers.rft_trainer import RFTTrainer

    class T(RFTTrainer):
        def loader(self):
            tr = self

            class L:
                def __iter__(self):
                    i = 0
                    while True:
                        yield synthetic_video_batch(tr.model_cfg, 1, seed=500 + 10 * tr.total_step_counter + i % 2,
                                                    n_docs=1 + i % 2)
                        i += 1
            return L()
    return T


def test_trainer_resume_equals_uninterrupted(tmp_path):
    """rft_trainer.py:64-121 + base.py:61-72: 2 Muon steps -> save -> a fresh trainer with
    resume_ckpt (model / EMA keys through the prefix strip, strict load) -> 1 more step gives the
    same parameters, EMA weights and optimizer state as 3 uninterrupted steps, bit for bit."""
    T = _step_keyed_trainer()
    c = _tiny_trainer_cfg(tmp_path)
    a = T(c.train, c.wandb, c.model, 0, 0, 1)
    a.max_steps = 3
    a.train()
    ck = tmp_path / "ckpt" / "step_2.pt"
    assert ck.exists()
    state = torch.load(ck, weights_only=True)
    assert set(state) == {"model", "ema", "opt", "steps"} and state["steps"] == 2
    # a reference-style checkpoint: compiled + DDP prefixes on model and EMA keys
    state["model"] = {"_orig_mod.module." + k: v for k, v in state["model"].items()}
    state["ema"] = {(k.replace("ema_model.", "ema_model._orig_mod.module.") if k.startswith("ema_model.") else k): v
                    for k, v in state["ema"].items()}
    torch.save(state, tmp_path / "ref_style.pt")
    (tmp_path / "b").mkdir(exist_ok=True)
    c2 = _tiny_trainer_cfg(tmp_path / "b", resume_ckpt=str(tmp_path / "ref_style.pt"))
    b = T(c2.train, c2.wandb, c2.model, 0, 0, 1)
    b.max_steps = 1
    b.train()
    assert b.total_step_counter == a.total_step_counter == 3
    assert b.history[0]["diffusion_loss"] == a.history[2]["diffusion_loss"]
    for (k, p), (k2, q) in zip(a.model.named_parameters(), b.model.named_parameters()):
        assert k == k2 and torch.equal(p, q), k
    for s, t in zip(a.ema.shadow, b.ema.shadow):
        assert torch.equal(s, t)
    assert a.ema.step == b.ema.step == 3
    sa, sb = a.opt.state_dict(), b.opt.state_dict()
    for part in ("adamw", "muon"):
        assert sa[part]["param_groups"] == sb[part]["param_groups"]
        for i, st in sa[part]["state"].items():
            for kk, v in st.items():
                assert torch.equal(v, sb[part]["state"][i][kk]), (part, i, kk)


def _trainer_worker(rank, ws, port, q, cfg_path):
    import os as _os
    _os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=ws)  # one card, 2 ranks: gloo on GPU tensors
    try:
        from owl_wms.configs import Config
        from owl_wms.trainers import get_trainer_cls
        torch.cuda.set_device(0)
        c = Config.from_yaml(cfg_path)
        tr = get_trainer_cls("rft")(c.train, c.wandb, c.model, rank, 0, ws)
        tr.max_steps = 2
        tr.train()
        torch.cuda.synchronize()
        q.put((rank, {k: p.detach().cpu().numpy() for k, p in tr.model.named_parameters()},
               [s.detach().cpu().numpy() for s in tr.ema.shadow], tr.history))
    finally:
        dist.destroy_process_group()


def test_trainer_two_ranks_on_gpu(tmp_path):
    """The trainer's N > 1 path (rft_trainer.py:95-228) with 2 ranks sharing the card over gloo:
    accum = target_batch / batch / world micro-steps per rank, the bucketed all-reduce, distributed
    Muon, EMA, the eval sampler with n_samples split over ranks (rft_trainer.py:155-170), the logged
    diffusion_loss summed over ranks (utils/logging.py:33-64), rank 0's checkpoint.  Replicas must be
    bit-identical and log the same loss."""
    import os as _os
    import torch.multiprocessing as mp
    c = _tiny_trainer_cfg(tmp_path, target_batch_size=4, sample_interval=2, sampler_id="av_caching", n_samples=2,
                          sampler_kwargs={"n_steps": 2, "cfg_scale": 1.0, "num_frames": 2, "noise_prev": 0.2,
                                          "only_return_generated": False},
                          sample_data_id="cod", sample_data_kwargs={"window_length": 4})
    assert c.train.target_batch_size == 4
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 29800 + _os.getpid() % 1000
    procs = [ctx.Process(target=_trainer_worker, args=(r, 2, port, q, str(tmp_path / "c.yml"))) for r in range(2)]
    for p in procs:
        p.start()
    res = {r: (prm, ema, hist) for r, prm, ema, hist in (q.get(timeout=150) for _ in range(2))}
    for p in procs:
        p.join(30)
        assert p.exitcode == 0
    (p0, e0, h0), (p1, e1, h1) = res[0], res[1]
    assert p0.keys() == p1.keys()
    for k in p0:
        assert (p0[k] == p1[k]).all(), k
    for a, b in zip(e0, e1):
        assert (a == b).all()
    assert len(h0) == len(h1) == 2
    for r0, r1 in zip(h0, h1):
        assert r0["diffusion_loss"] == r1["diffusion_loss"] and r0["step"] == r1["step"]
        assert math.isfinite(r0["diffusion_loss"])
    assert "eval/frames" in h0[0] and h0[0]["eval/samples"] == 2  # step 0 evaluates, 1 sample per rank
    assert (tmp_path / "ckpt" / "step_2.pt").exists()


def test_bench_two_ranks_json_line():
    """bench.py's N > 1 path as the driver launches it (torch.distributed.run, 2 ranks, barrier +
    max-over-ranks timing, one JSON line from rank 0), rehearsed with both ranks on this card
    (OWL_BENCH_SHARE_GPU: collectives over gloo, since RCCL needs one GPU per rank) at 64 frames."""
    import json
    import subprocess
    import sys
    env = dict(os.environ, OWL_BENCH_SHARE_GPU="1", MASTER_ADDR="127.0.0.1")
    port = 29900 + os.getpid() % 97
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr",
           "127.0.0.1", "--master-port", str(port), os.path.join(REPO, "bench.py"), "--gpus", "2", "--steps", "1",
           "--warmup", "1", "--frames", "64", "--no-cpu-baseline", "--no-profile"]
    r = subprocess.run(cmd, cwd=REPO, env=env, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]  # rank 0 only
    d = json.loads(lines[0])
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
                "vs_baseline", "dtype", "data", "config"):
        assert key in d, key
    assert d["n_gpus"] == 2 and d["steps"] == 1 and d["warmup"] == 1 and d["value"] > 0
    assert d["scaling"] == "strong" and d["config"]["parallelism"] == "dp2" and d["config"]["global_batch"] == 16
    # value: whole-job tokens / s (the driver's contract: total over all ranks / max-over-ranks time,
    # it computes scaling efficiency from the per-N values itself); the metric's per-GPU reading is
    # tokens_per_s_per_gpu = value / n_gpus
    assert abs(d["value"] - 16 * 64 * 64 / (d["ms_per_step"] / 1e3)) <= 1e-3 * d["value"]
    assert abs(d["tokens_per_s_per_gpu"] - d["value"] / d["n_gpus"]) <= 0.1


def test_bench_plain_run_dumps_outputs(tmp_path):
    """A plain bench.py run (no --full) on the TINY config: the result line keeps the contract's keys
    with no profile / CPU-baseline fields filled, --steps sets the timed steps, and --dump-outputs
    writes the last step's loss / params / ema as float32 .npy files of the documented sizes."""
    import json
    import subprocess
    import sys

    import numpy as np
    from bench import DUMP_PER_TENSOR
    from owl_wms.configs import model_config
    from owl_wms.models.gamerft import GameRFT
    _tiny_trainer_cfg(tmp_path)
    out = tmp_path / "dump"
    cmd = [sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
           "--global-batch", "2", "--config", str(tmp_path / "c.yml"), "--dump-outputs", str(out)]
    r = subprocess.run(cmd, cwd=str(tmp_path), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup"):
        assert key in d, key
    assert d["steps"] == 2 and d["warmup"] == 1 and d["value"] > 0 and d["ms_per_step"] > 0
    assert d["unit"] == "latent-tokens/s" and d["higher_is_better"] is True and d["dtype"] == "bf16"
    tol = 1e-3 + 0.05 / d["ms_per_step"]  # ms_per_step is rounded to 0.1 ms
    assert abs(d["value"] - 2 * 8 * 64 / (d["ms_per_step"] / 1e3)) <= tol * d["value"]
    assert d["roofline"] is None and d["cpu_baseline"] is None and "kernel_rates" not in d
    assert r.stderr.count("[bench] step ") == 2 and "PMC pass" not in r.stderr
    assert sorted(p.name for p in out.iterdir()) == ["ema.npy", "loss.npy", "params.npy"]
    n = sum(min(p.numel(), DUMP_PER_TENSOR) for p in GameRFT(model_config(**TINY)).parameters())
    arrays = {k: np.load(out / f"{k}.npy") for k in ("loss", "params", "ema")}
    assert arrays["loss"].shape == (2,) and arrays["params"].shape == arrays["ema"].shape == (n,)
    for a in arrays.values():
        assert a.dtype == np.float32 and np.isfinite(a).all()
    assert (arrays["loss"] > 0).all() and arrays["params"].std() > 0
    # the EMA copies the weights on its first updates (decay 0 at step 0 and 1), then lags them
    assert not np.array_equal(arrays["params"], arrays["ema"])
    assert np.abs(arrays["params"] - arrays["ema"]).max() < 0.1


def test_trainer_eval_sampler_at_sample_interval(tmp_path):
    """rft_trainer.py:213, 243-280: the EMA model's sampler runs at step 0 and every
    sample_interval; latents land in eval_sample_dir as vid.<step>.pt (4 context + 2 generated)."""
    from owl_wms.trainers import get_trainer_cls
    c = _tiny_trainer_cfg(tmp_path, sample_interval=2, sampler_id="av_caching", n_samples=1,
                          sampler_kwargs={"n_steps": 2, "cfg_scale": 1.0, "num_frames": 2, "noise_prev": 0.2,
                                          "only_return_generated": False},
                          sample_data_id="cod", sample_data_kwargs={"window_length": 4},
                          eval_sample_dir=str(tmp_path / "eval"))
    tr = get_trainer_cls("rft")(c.train, c.wandb, c.model, 0, 0, 1)
    tr.max_steps = 3
    tr.train()
    assert [("eval/frames" in h) for h in tr.history] == [True, False, True]
    for step in (0, 2):
        v = torch.load(tmp_path / "eval" / f"vid.{step}.pt", weights_only=True)
        assert v.shape == (1, 6, 32, 8, 8) and torch.isfinite(v.float()).all()


def test_trainer_eval_sampler_head_dim_128(tmp_path):
    """dit_v4_5B's eval path at head_dim 128 (d 256 / 2 heads): the trainer evaluates with the
    av_caching sampler (device-state decode, graphed Euler steps) at step 0 and every step
    (sample_interval 1) of a 2-step Muon run (configs/dit_v4_5B.yml sampler_id av_caching;
    rft_trainer.py:213, 243-280)."""
    from owl_wms.trainers import get_trainer_cls
    c = _tiny_trainer_cfg(tmp_path, model_over={"d_model": 256, "gradient_checkpointing": True}, sample_interval=1,
                          sampler_id="av_caching", n_samples=1,
                          sampler_kwargs={"n_steps": 3, "cfg_scale": 1.3, "num_frames": 3, "noise_prev": 0.2,
                                          "only_return_generated": False},
                          sample_data_id="cod", sample_data_kwargs={"window_length": 4},
                          eval_sample_dir=str(tmp_path / "eval"))
    tr = get_trainer_cls("rft")(c.train, c.wandb, c.model, 0, 0, 1)
    assert tr.model.core.transformer.blocks[0].attn.qkv.weight.shape[1] // c.model.n_heads == 128
    tr.max_steps = 2
    tr.train()
    assert [("eval/frames" in h) for h in tr.history] == [True, True]
    for step in (0, 1):
        v = torch.load(tmp_path / "eval" / f"vid.{step}.pt", weights_only=True)
        assert v.shape == (1, 7, 32, 8, 8) and torch.isfinite(v.float()).all()


def test_optimizer_step_refreshes_bf16_weights():
    """The fused optimizer passes write parameters through raw pointers; the version-keyed bf16
    weight caches must see it: after a Muon + AdamW step the model's forward equals that of a fresh
    model holding the same weights (bit for bit)."""
    from owl_wms.muon import init_muon
    from owl_wms.models.flow import InjectedNoise
    m, _ = _run("bf16")
    opt = init_muon(m, rank=0, world_size=1, lr=1e-2, momentum=0.95, adamw_lr=1e-2, adamw_wd=1e-4, adamw_eps=1e-15,
                    adamw_betas=[0.9, 0.95], adamw_keys=["core.proj_in", "core.proj_out.proj", "core.t_embed",
                                                         "core.control_embed", "gate", "adaln"])
    opt.step()
    fresh = _model()
    fresh.load_state_dict(m.state_dict())
    p = "gamerft.bf16."
    outs = []
    for mm in (m, fresh):
        mm.noise_source = InjectedNoise({"rand_b": GR[p + "in.rand_b"], "ts_raw": GR[p + "in.ts_raw"],
                                         "z": GR[p + "in.z"]})
        with torch.no_grad():
            outs.append(mm(GR[p + "in.x"].cuda(), GR[p + "in.mouse"].cuda(), GR[p + "in.btn"].cuda(),
                           GR[p + "in.doc_id"].cuda(), return_dict=True)["pred_video"])
    assert torch.equal(outs[0], outs[1])


def test_stacked_modulation_matches_four_linears():
    """fused.ModFn (DiTBlock.modulation: the four per-frame Linears of adaln1, gate1, adaln2, gate2 as
    one stacked GEMM with one dX GEMM in backward) == the four Linears on libowlk (nn/fused.linear):
    outputs, the cond gradient and every weight / bias gradient within bf16 GEMM tolerance."""
    import torch.nn.functional as F
    from owl_wms.nn.fused import ModFn, linear, stacked_modulation_weights
    torch.manual_seed(3)
    d, b, n = 256, 2, 24
    shapes = (2 * d, d, 2 * d, d)
    base = []
    for o in shapes:
        base += [torch.randn(o, d) * d ** -0.5, torch.randn(o) * 0.1]
    rs = [torch.randn(b, n, o, device="cuda") for o in shapes]
    cond0 = torch.randn(b, n, d)

    def run(stacked):
        ps = [torch.nn.Parameter(t.clone().cuda()) for t in base]
        cond = cond0.clone().cuda().requires_grad_(True)
        s = F.silu(cond)
        if stacked:
            owner = torch.nn.Module()
            W, bv = stacked_modulation_weights(owner, ps)
            outs = ModFn.apply(s, W, bv, *ps)
        else:
            outs = [linear(s, ps[2 * i], ps[2 * i + 1]) for i in range(4)]
        loss = sum((o.float() * r).sum() for o, r in zip(outs, rs))
        loss.backward()
        return [o.detach().float() for o in outs], cond.grad.float(), [p.grad.float() for p in ps]

    o1, c1, g1 = run(True)
    o2, c2, g2 = run(False)
    for a, r in zip(o1, o2):
        assert rel(a, r) < 1e-2
    assert rel(c1, c2) < 1e-2
    for a, r in zip(g1, g2):
        assert rel(a, r) < 1e-2
