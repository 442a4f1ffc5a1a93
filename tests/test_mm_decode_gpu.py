"""The MMDiT's fused joint-frame decode path on the GPU: the two kernels (kernels.mm_qk_rope_fwd_kv,
kernels.attn_decode_joint_fwd), MMDiTBlock._forward_decode, the audio + video window samplers against the
reference's own runs (tests/golden/make_golden_av_sampler.py, ``model.*``), the per-frame HIP graph, and
the AV trainer's eval step.

Bounds: 1e-2 rel-L2 is the project's bf16 per-op bound; 4e-3 (lse) / 5e-3 (O) between
two attention kernels on the same keys are test_attention_decode_split_keys' bounds; 2e-2 on sampled
latents and on cached-decode vs full forward is SURVEY §8(c) (test_av_caching_sampler_vs_reference,
test_mmdit_kv_cache_decode_matches_full_forward)."""
import os

import pytest
import torch

from conftest import REPO, golden
from oracle.params import det_init_, det_tensor

pytestmark = pytest.mark.gpu

DEV = "cuda"
MMCFG = dict(model_id="game_rft_audio", sample_size=8, channels=32, audio_channels=16, n_layers=2, n_heads=2,
             d_model=128, tokens_per_frame=65, n_buttons=11, n_mouse_axes=2, cfg_prob=0.1, n_frames=6, causal=True,
             uncond=False, backbone="mmdit", local_window=2, global_window=4, has_audio=True)
CANARY = 7.0


def K():
    from owl_wms import kernels
    return kernels


def rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


def rnd(*shape, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g).to(torch.bfloat16).to(DEV)


@pytest.fixture(scope="module", autouse=True)
def _needs_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from owl_wms._lib import lib
    lib()


def _guarded(rows, cols, pad=8):
    """a [rows, cols] bf16 view in the middle of a canary-filled buffer -> (buffer, view)"""
    buf = torch.full((pad + rows + pad, cols), CANARY, device=DEV, dtype=torch.bfloat16)
    return buf, buf[pad:pad + rows]


def _guards_intact(buf, rows, pad=8):
    return bool((buf[:pad] == CANARY).all()) and bool((buf[pad + rows:] == CANARY).all())


# ---------------------------------------------------------------- (a) rope for joint frames
@pytest.mark.parametrize("nf,offset", [(1, 0), (1, 130), (3, 65)])
def test_mm_rope_equals_interleave_rope_extend(nf, offset):
    """q, k, v bit for bit what frame_interleave -> qk_rope_fwd -> the cache copy produce, with the cache
    slots in the middle of a larger buffer; nothing outside the slots or past q is written."""
    k = K()
    B, H, D, n0, n1 = 2, 2, 64, 64, 1
    d, T = H * D, nf * (n0 + n1)
    n_tab = offset + T + 3
    g = torch.Generator().manual_seed(5)
    ang = torch.rand(n_tab, D // 2, generator=g) * 6.2831853
    cos, sin = torch.cos(ang).to(DEV), torch.sin(ang).to(DEV)
    qkv0, qkv1 = rnd(B * nf * n0, 3 * d, seed=11), rnd(B * nf * n1, 3 * d, seed=12)
    cap, s = offset + T + 40, offset + 7  # slots [s, s + T) of cap rows

    qkvj = k.frame_interleave(qkv0, qkv1, n0, n1)
    qkr, _ = k.qk_rope_fwd(qkvj, H, D, cos, sin, offset, T)
    q_ref = qkr.view(B, T, 2 * d)[:, :, :d]
    kb_ref = torch.full((B, cap, d), CANARY, device=DEV, dtype=torch.bfloat16)
    vb_ref = kb_ref.clone()
    kb_ref[:, s:s + T].copy_(qkr.view(B, T, 2 * d)[:, :, d:])
    vb_ref[:, s:s + T].copy_(qkvj.view(B, T, 3 * d)[:, :, 2 * d:])

    kb = torch.full((B, cap, d), CANARY, device=DEV, dtype=torch.bfloat16)
    vb = kb.clone()
    qbuf, qv = _guarded(B * T, d)
    q = qv.view(B, T, d)
    k.mm_qk_rope_fwd_kv(qkv0, qkv1, B, nf, n0, n1, H, D, cos, sin, offset, q, kb[:, s:s + T], vb[:, s:s + T])
    torch.cuda.synchronize()
    assert torch.equal(q, q_ref)
    assert torch.equal(kb, kb_ref) and torch.equal(vb, vb_ref)  # the slots, and every row around them
    assert _guards_intact(qbuf, B * T)
    with pytest.raises(RuntimeError, match="rope table"):
        k.mm_qk_rope_fwd_kv(qkv0, qkv1, B, nf, n0, n1, H, D, cos, sin, offset + 4, q, kb[:, s:s + T], vb[:, s:s + T])


# ---------------------------------------------------------------- (b) joint decode attention
_ATTN = {}


def _attn_inputs():
    """unit-RMS q and the 1,040-row unit-RMS key buffer + values, made once (read-only)"""
    if not _ATTN:
        B, H, D, Lq, cap = 2, 3, 64, 65, 1040
        unit = lambda t: (t.float().view(*t.shape[:-1], H, D) * torch.rsqrt(
            t.float().view(*t.shape[:-1], H, D).pow(2).mean(-1, keepdim=True))).bfloat16().view(t.shape)
        _ATTN.update(q=unit(rnd(B, Lq, H * D, seed=70)), k=unit(rnd(B, cap, H * D, seed=71)),
                     v=rnd(B, cap, H * D, seed=72))
    return _ATTN["q"], _ATTN["k"], _ATTN["v"]


@pytest.mark.parametrize("Lkv,window", [(65, 0), (260, 0), (585, 0), (1040, 0), (585, 130)])
def test_joint_decode_attention(Lkv, window):
    """One 65-row joint frame against Lkv keys (65: two key tiles, two waves idle; a 130-row window
    view of a 585-row cache): == fp32 torch attention (1e-2, the audio row alone too), == attn_fwd +
    frame_split on the same keys (lse 4e-3, O 5e-3), video / audio rows written apart and nowhere else,
    deterministic."""
    k = K()
    B, H, D, n0, n1 = 2, 3, 64, 64, 1
    Lq, d = n0 + n1, H * D
    q, kfull, vfull = _attn_inputs()
    kk, v = kfull[:, :Lkv], vfull[:, :Lkv]
    if window:
        kk, v = kk[:, -window:], v[:, -window:]
    L = kk.shape[1]
    b0, o0 = _guarded(B * n0, d)
    b1, o1 = _guarded(B * n1, d)
    bound = k.qk_norm_bound(D)
    _, _, lse = k.attn_decode_joint_fwd(q, kk, v, H, D, n0, n1, score_bound=bound, want_lse=True, o0=o0, o1=o1)
    torch.cuda.synchronize()
    assert _guards_intact(b0, B * n0) and _guards_intact(b1, B * n1)
    o = torch.cat([o0.view(B, n0, d), o1.view(B, n1, d)], dim=1)

    qf, kf, vf = (t.float().view(B, -1, H, D).transpose(1, 2) for t in (q, kk, v))
    ref = (torch.softmax(qf @ kf.transpose(-1, -2) * D ** -0.5, dim=-1) @ vf).transpose(1, 2).reshape(B, Lq, d)
    r_all, r_audio = rel(o, ref), rel(o[:, n0:], ref[:, n0:])
    print(f"joint decode Lkv={L}: rel all {r_all:.2e} audio row {r_audio:.2e}")
    assert r_all < 1e-2
    assert r_audio < 1e-2

    og, lse_g = k.attn_fwd(q, kk, v, H, D, k.FrameMask(1, None, False, 0, None), score_bound=bound)
    g0, g1 = k.frame_split(og.view(B * Lq, d), n0, n1)
    assert (lse - lse_g).abs().max().item() < 4e-3
    assert rel(o0, g0) < 5e-3 and rel(o1, g1) < 5e-3

    p0, p1, lse2 = k.attn_decode_joint_fwd(q, kk, v, H, D, n0, n1, score_bound=bound, want_lse=True)
    assert torch.equal(p0, o0) and torch.equal(p1, o1) and torch.equal(lse2, lse)
    # lse is optional
    n0_, n1_, none = k.attn_decode_joint_fwd(q, kk, v, H, D, n0, n1, score_bound=bound)
    assert none is None and torch.equal(n0_, o0) and torch.equal(n1_, o1)


# ---------------------------------------------------------------- block path
@pytest.fixture(scope="module")
def mm_model():
    from owl_wms.configs import model_config
    from owl_wms.models.gamerft_audio import GameRFTAudio
    return det_init_(GameRFTAudio(model_config(**MMCFG)), base_seed=5000).cuda().eval()


def _block_inputs():
    B, n = 2, 6
    return (det_tensor((B, n, 32, 8, 8), 910).cuda().bfloat16(), det_tensor((B, n, 16), 911).cuda().bfloat16(),
            torch.sigmoid(det_tensor((B, n), 912)).cuda().bfloat16(), det_tensor((B, n, 2), 913).cuda().bfloat16(),
            (det_tensor((B, n, 11), 914) > 0).cuda().bfloat16())


def _cached_decode(core, ins, n_ctx, decoding):
    from owl_wms.nn.kv_cache import KVCache
    tr = core.transformer
    with torch.no_grad():
        cache = KVCache(core.config)
        cache.reset(ins[0].shape[0])
        cache.enable_cache_updates()
        if decoding:
            tr.enable_decoding()
        try:
            ctx = core(*(t[:, :n_ctx] for t in ins), kv_cache=cache)
            cache.disable_cache_updates()
            assert cache.length_at(0) == n_ctx * 65
            last = core(*(t[:, n_ctx:] for t in ins), kv_cache=cache)
        finally:
            tr.disable_decoding()
    return ctx, last


def test_mmdit_decoding_flag_defaults_off(mm_model):
    tr = mm_model.core.transformer
    assert tr.decoding is False and not any(b.decoding for b in tr.blocks)
    tr.enable_decoding()
    assert tr.decoding and all(b.decoding for b in tr.blocks)
    tr.disable_decoding()
    assert tr.decoding is False and not any(b.decoding for b in tr.blocks)


def test_block_decode_last_frame_matches_full_forward(mm_model):
    """n_ctx = 5: the sixth frame decoded alone on the fused path (local window 2 / global window 4
    frames of the 6 cached + new) == that frame of the full masked forward, video and audio."""
    core, ins = mm_model.core, _block_inputs()
    with torch.no_grad():
        fv, fa = core(*ins)
    (cv, ca), (lv, la) = _cached_decode(core, ins, 5, True)
    (_, _), (ov, oa) = _cached_decode(core, ins, 5, False)
    print(f"decoding on vs off: video {rel(lv, ov):.2e} audio {rel(la, oa):.2e}; "
          f"vs full forward: video {rel(lv, fv[:, 5:]):.2e} audio {rel(la, fa[:, 5:]):.2e}")
    assert rel(lv, fv[:, 5:]) < 2e-2
    assert rel(la, fa[:, 5:]) < 2e-2


def test_block_multi_frame_decoding_on_equals_off(mm_model):
    """n_ctx = 3: the cache-filling pass (offset 0) and a 3-frame cached call, decoding on: the rope
    kernel writes the same q, k, v and the masked attention is the same launch -> identical bits."""
    core, ins = mm_model.core, _block_inputs()
    on_ctx, on_last = _cached_decode(core, ins, 3, True)
    off_ctx, off_last = _cached_decode(core, ins, 3, False)
    for a, b in zip(on_ctx + on_last, off_ctx + off_last):
        assert torch.equal(a, b)


# ---------------------------------------------------------------- samplers vs the reference
def _sample(model, sid, S, use_decoding=True, **call_kw):
    from owl_wms.sampling import get_sampler_cls
    from test_av_samplers_cpu import _Draws
    st = S["settings"]
    sampler = get_sampler_cls(sid)(n_steps=st["n_steps"], cfg_scale=st["cfg_scale"], window_length=st["window_length"],
                                   num_frames=st["num_frames"], noise_prev=st["noise_prev"])
    sampler.use_decoding = use_decoding
    with _Draws(S["model.in.noise"]):
        out = sampler(model.core, *(S[f"model.in.{k}"].cuda() for k in ("x", "audio", "mouse", "btn")), **call_kw)
    return out


@pytest.mark.parametrize("sid,use_decoding", [("av_window", True), ("av_causal", True), ("av_causal_no_cfg", True),
                                              ("av_causal", False)])
def test_av_samplers_vs_reference(mm_model, sid, use_decoding):
    """4 context + 2 generated frames, window 4, 3 Euler steps, CFG 1.3, the reference's draws: context
    exact, generated video and audio within 2e-2 each; av_causal also with the fused path forced off."""
    S = golden("av_sampler_tiny.pt")
    out = _sample(mm_model, sid, S, use_decoding)
    ref = S[f"model.{sid}.out"]
    assert len(out) == len(ref)
    assert not mm_model.core.transformer.decoding
    x, audio = out[-4], out[-3]
    rx, ra = ref[-4], ref[-3]
    assert x.shape == rx.shape and audio.shape == ra.shape
    n = S["model.in.x"].shape[1]
    assert torch.equal(x[:, :n].cpu().float(), rx[:, :n]) and torch.equal(audio[:, :n].cpu().float(), ra[:, :n])
    rv, raud = rel(x[:, n:], rx[:, n:]), rel(audio[:, n:], ra[:, n:])
    print(f"{sid} decoding={use_decoding}: generated video rel {rv:.2e} audio rel {raud:.2e}")
    assert rv < 2e-2
    assert raud < 2e-2
    assert torch.equal(out[-2].cpu().float(), ref[-2]) and torch.equal(out[-1].cpu().float(), ref[-1])


# ---------------------------------------------------------------- one graph per generated frame
@pytest.mark.parametrize("sid", ["av_causal", "av_causal_no_cfg"])
def test_graphed_frames_equal_eager(mm_model, sid):
    """compile_on_decode: frame 0 eager, frame 1 captured + replayed, frame 2 a replay -> the eager
    loop's bits."""
    from owl_wms.sampling import get_sampler_cls
    S = golden("av_sampler_tiny.pt")
    ins = [S[f"model.in.{k}"].cuda() for k in ("x", "audio", "mouse", "btn")]
    sampler = get_sampler_cls(sid)(n_steps=3, cfg_scale=1.3, window_length=4, num_frames=3, noise_prev=0.2)
    outs = []
    for graphed in (False, True):
        torch.manual_seed(123)
        outs.append(sampler(mm_model.core, *ins, compile_on_decode=graphed))
    torch.cuda.synchronize()
    for a, b in zip(*outs):
        assert a.shape == b.shape and torch.equal(a, b)
    assert outs[0][0].shape[1] == 7 and torch.isfinite(outs[0][0].float()).all()
    assert not mm_model.core.transformer.decoding


# ---------------------------------------------------------------- trainer eval
def test_av_trainer_eval_step(tmp_path):
    """AVRFTTrainer with sampler_id av_causal samples at every step (sample_interval 1): 4 context + 2
    generated frames of video and audio from the EMA core."""
    import math

    import yaml
    from owl_wms.configs import Config
    from owl_wms.trainers import get_trainer_cls
    opt = yaml.safe_load(open(os.path.join(REPO, "configs", "mmdit_v2.yml")))["train"]["opt_kwargs"]
    train = {"trainer_id": "av", "data_id": "synthetic", "data_kwargs": {"window_length": 6}, "target_batch_size": 1,
             "batch_size": 1, "epochs": 1, "opt": "Muon", "opt_kwargs": opt, "checkpoint_dir": str(tmp_path / "ckpt"),
             "save_interval": 10 ** 9, "sample_interval": 1, "vae_scale": 1.0, "seed": 77, "sampler_id": "av_causal",
             "n_samples": 1, "sample_data_id": "cod", "sample_data_kwargs": {"window_length": 4},
             "sampler_kwargs": {"n_steps": 2, "cfg_scale": 1.3, "window_length": 4, "num_frames": 2,
                                "noise_prev": 0.2, "only_return_generated": False}}
    (tmp_path / "c.yml").write_text(yaml.safe_dump({"model": MMCFG, "train": train,
                                                    "wandb": {"project": "p", "run_name": "r"}}))
    c = Config.from_yaml(str(tmp_path / "c.yml"))
    tr = get_trainer_cls("av")(c.train, c.wandb, c.model, 0, 0, 1)
    tr.max_steps = 1
    tr.train()
    rec = tr.history[0]
    for key in ("eval/samples", "eval/frames", "eval/latent_std", "eval/audio_std"):
        assert key in rec and math.isfinite(rec[key]), key
    assert rec["eval/frames"] == 4 + 2 and rec["eval/samples"] == 1
    assert not tr.get_module(ema=True).core.transformer.decoding
