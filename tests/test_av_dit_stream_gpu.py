"""Model-level tests of audio + video streaming on the DiT backbone (owl_wms/sampling/stream.py:
AVDiTFrameStream on a RingKVCache through Attn._attend's wide ring pair, sampler id av_audio_stream) on the
tiny model of tests/test_av_stream_gpu.py with backbone "dit": d_model 128, 2 heads, 2 layers, 65 tokens per
frame, local_window 2, global_window 4.  The cases, inputs and seeds mirror that file's.

Bounds.  A wrapping ring against one that never wraps, graphed against eager, the sampler id against the
hand-driven stream: torch.equal -- the same kernels' arithmetic in the same order and the same torch draws.
The ring path against the existing decode path (SingleKVCache + DiT.enable_decoding: qk_rope_fwd_kv +
attn_fwd, other kernels), cached decode against the full masked forward, and a rebased stream against a
table long enough to need none: rel-L2 2e-2, the project's bound between equivalent decode paths
(test_mmdit_kv_cache_decode_matches_full_forward).  The full forward against the CPU oracle
(fp32 weights, bf16 autocast, as the goldens are made): rel-L2 2e-2, the bound of
test_mmdit_loss_pred_grads_vs_reference."""
import functools

import pytest
import torch

from oracle import ref_model as M
from oracle.params import det_init_

pytestmark = pytest.mark.gpu

DITCFG = dict(model_id="game_rft_audio", sample_size=8, channels=32, audio_channels=16, n_layers=2, n_heads=2,
              d_model=128, tokens_per_frame=65, n_buttons=11, n_mouse_axes=2, cfg_prob=0.1, n_frames=8, causal=True,
              uncond=False, backbone="dit", local_window=2, global_window=4, has_audio=True, rope_impl="motion",
              rope_ats_delta=2.0)
TPF = 65


def rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


def finite(*ts):
    return all(bool(torch.isfinite(t.float()).all()) for t in ts)


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


@functools.lru_cache(maxsize=None)
def _model(n_frames=8, rope_impl="motion", copy=0):
    """the weights do not depend on n_frames or rope_impl: the RoPE tables are non-persistent buffers.  copy:
    a second instance of the same model (one whose tables a test replaces)"""
    from owl_wms.configs import model_config
    from owl_wms.models.gamerft_audio import GameRFTAudio
    kw = dict(DITCFG, n_frames=n_frames, rope_impl=rope_impl)
    return det_init_(GameRFTAudio(model_config(**kw)), base_seed=5000).cuda().eval()


def _inputs(b, init, total, seed=7):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(b, init, 32, 8, 8, generator=g).bfloat16().cuda()
    audio = torch.randn(b, init, 16, generator=g).bfloat16().cuda()
    mouse = torch.randn(b, total, 2, generator=g).bfloat16().cuda()
    btn = (torch.rand(b, total, 11, generator=g) < 0.5).bfloat16().cuda()
    return x, audio, mouse, btn


def _stream(core, ins, frames, seed=321, **kw):
    """hand-driven AVDiTFrameStream: (video [b, n, c, h, w], audio [b, n, ca], the stream after close, buffer
    addresses after start(), addresses and row counts after the last frame)"""
    from owl_wms.sampling.stream import AVDiTFrameStream
    x, audio, mouse, btn = ins
    init = x.size(1)
    torch.manual_seed(seed)
    with AVDiTFrameStream(core, **kw) as s:
        s.start(x, audio, mouse, btn)
        ptrs0 = [(kb.data_ptr(), vb.data_ptr()) for kb, vb in s.kv_cache.bufs]
        out = [s.step(mouse[:, init + i:init + i + 1], btn[:, init + i:init + i + 1]) for i in range(frames)]
        ptrs1 = [(kb.data_ptr(), vb.data_ptr()) for kb, vb in s.kv_cache.bufs]
        rows = [(kb.shape[1], vb.shape[1]) for kb, vb in s.kv_cache.bufs]
    torch.cuda.synchronize()
    return torch.cat([o[0] for o in out], 1), torch.cat([o[1] for o in out], 1), s, ptrs0, ptrs1, rows


class _RefDiTAudioCore(M.GameRFTAudioCore):
    """The oracle's GameRFTAudioCore with its transformer replaced by its DiT (gamerft_audio.py:68-76, backbone
    "dit"): the audio token appended to each frame's 64 video tokens, one stream, then split."""

    def __init__(self, cfg):
        super().__init__(cfg)
        self.transformer = M.DiT(cfg)

    def forward(self, x, audio, t, mouse, btn, has_controls=None):
        cond = self.t_embed(t)
        ctrl = self.control_embed(mouse, btn)
        if has_controls is not None:
            ctrl = torch.where(has_controls[:, None, None], ctrl, torch.zeros_like(ctrl))
        cond = cond + ctrl
        b, n, c, h, w = x.shape
        d = self.cfg.d_model
        xv = self.proj_in(x.permute(0, 1, 3, 4, 2).reshape(b, n, h * w, c))
        xa = self.audio_proj_in(audio).view(b, n, 1, d)
        joint = self.transformer(torch.cat([xv, xa], 2).reshape(b, n * (h * w + 1), d), cond)
        joint = joint.view(b, n, h * w + 1, d)
        video, aud = joint[:, :, :-1].reshape(b, n * h * w, d), joint[:, :, -1]
        video = self.proj_out(M.R.layer_norm(video), M.R.layer_norm(cond))
        return video.reshape(b, n, h, w, c).permute(0, 1, 4, 2, 3), self.audio_proj_out(aud, cond)


@pytest.mark.parametrize("rope_impl", ["motion", "ortho"])
def test_dit_backbone_full_forward_matches_the_oracle(rope_impl):
    """The dit-backbone core's masked forward over 6 frames (local window 2, global window 4), one sample with
    its controls dropped, against the oracle on the CPU carrying the model's state_dict in fp32, evaluated
    as the goldens of test_mmdit_loss_pred_grads_vs_reference are (tests/golden/make_golden_mmdit.py: fp32
    weights under bf16 autocast, the reference's training and sampling semantics), which is what that test's
    2e-2 bounds.  The same oracle evaluated in fp32 is printed beside it: on this tiny model bf16 semantics
    alone move the video output by 1.0e-1 and the audio output by 1.6e-2 (oracle autocast against oracle
    fp32 on the CPU, the MMDiT oracle the same), so that figure says nothing about the kernels."""
    from types import SimpleNamespace
    m = _model(8, rope_impl)
    ref = _RefDiTAudioCore(SimpleNamespace(**dict(DITCFG, rope_impl=rope_impl))).float().eval()
    ref.load_state_dict({k: v.detach().float().cpu() for k, v in m.core.state_dict().items()}, strict=True)
    rope = m.core.transformer.rope
    tab_c, tab_s = rel(rope.cos, ref.transformer.cos), rel(rope.sin, ref.transformer.sin)
    x, audio, mouse, btn = _inputs(2, 6, 6)
    g = torch.Generator().manual_seed(11)
    t = torch.sigmoid(torch.randn(2, 6, generator=g)).bfloat16().cuda()
    hc = torch.tensor([True, False]).cuda()
    with torch.no_grad():
        pv, pa = m.core(x, audio, t, mouse, btn, has_controls=hc)
        args = (x.cpu(), audio.cpu(), t.cpu(), mouse.cpu(), btn.cpu(), hc.cpu())
        with torch.autocast("cpu", dtype=torch.bfloat16):
            rv, ra = ref(*args)
        fv, fa = ref(*(a.float() for a in args[:5]), args[5])
    ev, ea = rel(pv, rv), rel(pa, ra)
    print(f"dit-backbone AV core against the oracle, {rope_impl}: video rel-L2 {ev:.3e}, audio {ea:.3e} (against "
          f"the oracle evaluated in fp32: video {rel(pv, fv):.3e}, audio {rel(pa, fa):.3e}; tables: cos "
          f"{tab_c:.1e}, sin {tab_s:.1e})")
    assert finite(pv, pa, rv, ra)
    assert pv.shape == rv.shape == (2, 6, 32, 8, 8) and pa.shape == ra.shape == (2, 6, 16)
    assert ev < 2e-2
    assert ea < 2e-2


def test_first_streamed_frame_matches_the_full_masked_forward():
    """3 context frames, one Euler step (dt = 1), no CFG: with the stream's four draws replayed, the
    streamed frame == noise - 1.0 * core(the full 4-frame window)[:, -1], video and audio, within 2e-2."""
    m = _model(8)
    ins = _inputs(2, 3, 4)
    x, audio, mouse, btn = ins
    v, a, s, *_ = _stream(m.core, ins, 1, n_steps=1, cfg_scale=1.0, noise_prev=0.2, max_cached_frames=4)
    assert v.shape == (2, 1, 32, 8, 8) and a.shape == (2, 1, 16)
    torch.manual_seed(321)
    zv, za = torch.randn_like(x), torch.randn_like(audio)
    nv, na = torch.randn_like(x[:, :1]), torch.randn_like(audio[:, :1])
    wv = torch.cat([x * (1.0 - 0.2) + zv * 0.2, nv], 1)
    wa = torch.cat([audio * (1.0 - 0.2) + za * 0.2, na], 1)
    ts = x.new_full((2, 4), 0.2)
    ts[:, -1] = 1.0
    with torch.no_grad():
        pv, pa = m.core(wv, wa, ts, mouse, btn)
    want_v, want_a = nv - 1.0 * pv[:, -1:], na - 1.0 * pa[:, -1:]
    rv, ra = rel(v, want_v), rel(a, want_a)
    print(f"first streamed frame against the full masked forward: video rel-L2 {rv:.3e}, audio {ra:.3e}")
    assert finite(v, a, want_v, want_a)
    assert rv <= 2e-2
    assert ra <= 2e-2
    assert not m.core.transformer.decoding


def _linear_loop(core, ins, frames, n_steps, cfg_scale, noise_prev, seed=321):
    """AVDiTFrameStream's algorithm on the existing kernels only: SingleKVCache + DiT.enable_decoding
    (qk_rope_fwd_kv into the cache's slots, attn_fwd unmasked over [cache | new]), the same draws in the same
    order, the same Euler arithmetic; no eviction."""
    from owl_wms.nn.kv_cache import KVCache
    from owl_wms.sampling.schedulers import get_sd3_euler
    x, audio, mouse, btn = ins
    B, init = x.shape[:2]
    cfg = cfg_scale != 1.0
    rep = (lambda *ts: [torch.cat([t, t]) for t in ts]) if cfg else (lambda *ts: list(ts))
    hc = torch.ones(2 * B if cfg else B, dtype=torch.bool, device=x.device)
    if cfg:
        hc[B:] = False
    zl = lambda t: t * (1.0 - noise_prev) + torch.randn_like(t) * noise_prev
    dt = get_sd3_euler(n_steps).to(device=x.device, dtype=x.dtype)
    tr = core.transformer
    vs, as_ = [], []
    torch.manual_seed(seed)
    with torch.no_grad():
        cache = KVCache(core.config)
        cache.reset(2 * B if cfg else B)
        vn, an = zl(x), zl(audio)
        ts = x.new_full((B, init), noise_prev)
        cache.enable_cache_updates()
        core(*rep(vn, an, ts, mouse[:, :init], btn[:, :init]), has_controls=hc, kv_cache=cache)
        cache.disable_cache_updates()
        tr.enable_decoding()
        try:
            for i in range(frames):
                m1, b1 = mouse[:, init + i:init + i + 1], btn[:, init + i:init + i + 1]
                xv, xa = torch.randn_like(x[:, :1]), torch.randn_like(audio[:, :1])
                t = torch.ones_like(ts[:, :1])
                for k in range(n_steps):
                    pv, pa = core(*rep(xv, xa, t, m1, b1), has_controls=hc, kv_cache=cache)
                    if cfg:
                        pv = pv[B:] + cfg_scale * (pv[:B] - pv[B:])
                        pa = pa[B:] + cfg_scale * (pa[:B] - pa[B:])
                    xv, xa, t = xv - dt[k] * pv, xa - dt[k] * pa, t - dt[k]
                vs.append(xv.clone())
                as_.append(xa.clone())
                vn, an = zl(xv), zl(xa)
                cache.enable_cache_updates()
                core(*rep(vn, an, torch.ones_like(t) * noise_prev, m1, b1), has_controls=hc, kv_cache=cache)
                cache.disable_cache_updates()
                assert cache.length_at(0) == cache.get_offset(0) == (init + i + 1) * TPF
        finally:
            tr.disable_decoding()
    return torch.cat(vs, 1), torch.cat(as_, 1)


@pytest.mark.parametrize("cfg_scale", [1.3, 1.0])
def test_ring_path_matches_the_existing_decode_path_before_the_first_eviction(cfg_scale):
    """3 context + 3 generated frames, max_cached_frames 6 (no eviction: offsets and cached lengths
    coincide), 3 steps: the ring pair end to end against today's decode kernels, rel-L2 2e-2 (the attention
    kernels differ, so not torch.equal)."""
    m = _model(8)
    ins = _inputs(2, 3, 6)
    v, a, s, *_ = _stream(m.core, ins, 3, n_steps=3, cfg_scale=cfg_scale, noise_prev=0.2, max_cached_frames=6)
    assert s.kv_cache.start[0] == 0 and s.kv_cache.n_frames() == 6 and s.rebases == 0
    rv, ra = _linear_loop(m.core, ins, 3, 3, cfg_scale, 0.2)
    ev, ea = rel(v, rv), rel(a, ra)
    print(f"ring path against the existing decode path, cfg {cfg_scale}: video rel-L2 {ev:.3e}, audio {ea:.3e}")
    assert finite(v, a, rv, ra)
    assert ev <= 2e-2
    assert ea <= 2e-2
    assert not m.core.transformer.decoding


def test_wrapping_ring_equals_a_ring_that_never_wraps():
    """3 context frames, max_cached_frames 4, 12 generated frames on the 32-frame table: the default ring of
    5 frames wraps (11 evictions), ring_frames 16 never does; eager and graphed; all bit-identical.  The
    buffers keep their 5 * 65 rows and their addresses."""
    m = _model(32)
    ins = _inputs(2, 3, 15)
    kw = dict(n_steps=3, cfg_scale=1.3, noise_prev=0.2, max_cached_frames=4)
    v, a, s, ptrs0, ptrs1, rows = _stream(m.core, ins, 12, **kw)
    assert finite(v, a)
    assert s.frames_generated == 12 and s.rebases == 0
    cap = 5 * TPF
    assert len(rows) == DITCFG["n_layers"] and all(r == (cap, cap) for r in rows)
    assert ptrs0 == ptrs1 and len({p for pair in ptrs0 for p in pair}) == 2 * DITCFG["n_layers"]
    assert s.kv_cache.n_frames() == 4 and s.kv_cache.get_offset(0) == 15 * TPF
    assert s.kv_cache.start[0] == (11 * TPF) % cap
    v16, a16, s16, *_ = _stream(m.core, ins, 12, ring_frames=16, **kw)
    assert s16.kv_cache.start[0] == 11 * TPF and s16.kv_cache.capacity == 16 * TPF  # never wrapped
    assert finite(v16, a16)
    assert torch.equal(v, v16) and torch.equal(a, a16)
    for rf in (None, 16):
        vg, ag, sg, g0, g1, _ = _stream(m.core, ins, 12, graphed=True, ring_frames=rf, **kw)
        assert g0 == g1 and sg.frames_generated == 12
        assert finite(vg, ag)
        assert torch.equal(vg, v) and torch.equal(ag, a), rf
    assert not m.core.transformer.decoding


def _past_the_table(short, long_, what):
    """12 frames from 3 context frames with max_cached_frames 4 on `short` (an 8-frame table: positions would
    reach 15) against `long_` (32 frames, no rebase): >= 2 rebases, video and audio within rel-L2 2e-2,
    graphed == eager bit for bit."""
    ins = _inputs(2, 3, 15)
    kw = dict(n_steps=3, cfg_scale=1.3, noise_prev=0.2, max_cached_frames=4)
    rv, ra, s_ref, *_ = _stream(long_.core, ins, 12, **kw)
    assert s_ref.rebases == 0
    v, a, s, ptrs0, ptrs1, rows = _stream(short.core, ins, 12, **kw)
    assert s.rebases >= 2 and s.frames_generated == 12
    assert ptrs0 == ptrs1 and all(r == (5 * TPF, 5 * TPF) for r in rows)
    ev, ea = rel(v, rv), rel(a, ra)
    print(f"AV DiT stream past the {what} table ({s.rebases} rebases) against the 32-frame table: video rel-L2 "
          f"{ev:.3e}, audio rel-L2 {ea:.3e}")
    vg, ag, sg, *_ = _stream(short.core, ins, 12, graphed=True, **kw)
    assert sg.rebases == s.rebases
    assert finite(v, a, rv, ra, vg, ag)
    assert torch.equal(vg, v) and torch.equal(ag, a)
    assert ev <= 2e-2
    assert ea <= 2e-2


def _same_weights(a, b):
    for (ka, a_), (kb_, b_) in zip(sorted(a.state_dict().items()), sorted(b.state_dict().items())):
        assert ka == kb_ and torch.equal(a_, b_), ka


def test_av_dit_stream_past_the_motion_table():
    """n_frames 8 against 32 with the same weights; the short MotionRoPE table is a bit-identical prefix."""
    short, long_ = _model(8), _model(32)
    _same_weights(short, long_)
    rs, rl = short.core.transformer.rope, long_.core.transformer.rope
    n = rs.cos.shape[0]
    assert n == 8 * TPF and rl.cos.shape[0] == 32 * TPF
    assert torch.equal(rs.cos, rl.cos[:n]) and torch.equal(rs.sin, rl.sin[:n])
    _past_the_table(short, long_, "motion")


def test_av_dit_stream_past_the_ortho_table():
    """The same run on the 8-frame OrthoRoPE table: it rebases (at least twice) instead of raising.  The
    reference is a second 32-frame model with the same weights whose tables carry the 8-frame law extended to
    32 frames: angles a_r + f * delta in fp64 from the 8-frame get_freqs (a_r frame 0's, delta the mean frame
    step), cos and sin taken to fp32.  (The 32-frame OrthoRoPE table itself is another law: its time axis is a
    linspace over its own n_frames.)  The bound is the motion twin's: the table contributes under 1e-4 rad of
    rotation error against the bf16 rounding of K (2^-8) that both tables share."""
    short, long_ = _model(8, "ortho"), _model(32, "ortho", copy=1)
    _same_weights(short, long_)
    rs, rl = short.core.transformer.rope, long_.core.transformer.rope
    ang = rs.get_freqs(short.core.config).double().view(8, TPF, -1)
    delta = (ang[7] - ang[0]) / 7.0
    ext = ang[0][None] + torch.arange(32, dtype=torch.float64)[:, None, None] * delta[None]
    fit = (ext[:8] - ang).abs().max().item()
    print(f"8-frame ortho law extended to 32 frames: max |extended - table| over the 8 frames {fit:.2e} rad")
    assert delta.abs().max().item() > 0.0 and rl.cos.shape == (32 * TPF, 32)
    rl.cos.copy_(ext.cos().float().view(32 * TPF, -1))
    rl.sin.copy_(ext.sin().float().view(32 * TPF, -1))
    # the same law: three fp32 roundings of an angle (2^-22 * 402 rad each) at most apart on the 8 frames
    assert fit < 3 * 2.0 ** -22 * ang.abs().max().item()
    _past_the_table(short, long_, "ortho")


def test_ring_attention_path_refuses_what_the_ring_cannot_serve():
    """Two frames at once against a ring cache at offset > 0: Attn._attend's RuntimeError."""
    from owl_wms.sampling.stream import AVDiTFrameStream
    m = _model(8)
    x, audio, mouse, btn = _inputs(1, 3, 6)
    with AVDiTFrameStream(m.core, n_steps=1, cfg_scale=1.0, max_cached_frames=5) as s:
        s.start(x, audio, mouse, btn)
        two = (x[:, :2], audio[:, :2], x.new_ones(1, 2), mouse[:, 3:5], btn[:, 3:5])
        m.core.transformer.enable_decoding()
        try:
            with pytest.raises(RuntimeError, match="one frame at a time.*at most 80 rows.*130 rows"):
                m.core(*two, kv_cache=s.kv_cache)
        finally:
            m.core.transformer.disable_decoding()
        with pytest.raises(RuntimeError, match="one frame at a time"):  # masked: refused as well
            m.core(*two, kv_cache=s.kv_cache)
    torch.cuda.synchronize()


def test_av_audio_stream_registry_id_on_the_dit_core():
    """sampler_id av_audio_stream on the dit core == a hand-driven AVDiTFrameStream with the same seed; it
    returns (x, audio, mouse, btn) with av_causal's shapes."""
    from owl_wms.sampling import get_sampler_cls
    m = _model(8)
    ins = _inputs(2, 3, 10)
    x, audio, mouse, btn = ins
    smp = get_sampler_cls("av_audio_stream")(n_steps=2, cfg_scale=1.3, num_frames=7, noise_prev=0.2,
                                             max_cached_frames=4)
    torch.manual_seed(321)
    out = smp(m.core, x, audio, mouse, btn)  # 10 control columns = 3 + 7: used as given, no permuted copies
    assert len(out) == 4
    assert torch.equal(out[0][:, :3], x) and torch.equal(out[1][:, :3], audio)
    assert torch.equal(out[2], mouse) and torch.equal(out[3], btn)
    hv, ha, s, *_ = _stream(m.core, ins, 7, n_steps=2, cfg_scale=1.3, noise_prev=0.2, max_cached_frames=4)
    assert s.rebases >= 1  # 3 + 7 frames on an 8-frame table
    assert finite(hv, ha, out[0], out[1])
    assert torch.equal(out[0][:, 3:], hv) and torch.equal(out[1][:, 3:], ha)
    # av_causal with a window of the 3 context frames extends the controls to the same length
    ref = get_sampler_cls("av_causal")(n_steps=2, cfg_scale=1.3, window_length=3, num_frames=7, noise_prev=0.2)(
        _model(32).core, x, audio, mouse[:, :3], btn[:, :3])
    assert [t.shape for t in out] == [t.shape for t in ref]
    short = smp(m.core, x, audio, mouse[:, :3], btn[:, :3])  # controls extended by batch_permute_to_length
    assert [t.shape for t in short] == [t.shape for t in ref]
    assert torch.equal(short[2][:, :3], mouse[:, :3]) and finite(short[0])
