"""Model-level tests of endless audio + video streaming (owl_wms/sampling/stream.py: AVFrameStream on a
RingKVCache through MMDiTBlock._forward_ring_decode, sampler id av_audio_stream) on the tiny MMDiT of
tests/test_mm_decode_gpu.py with MotionRoPE.

Bounds.  Ring path against the existing decode path (SingleKVCache + MMDIT.enable_decoding) before the
first eviction, a wrapping ring against one that never wraps, graphed against eager: torch.equal -- the
same kernels' arithmetic in the same order and the same torch draws.  Cached decode against the full
masked forward, and a rebased stream against a table long enough to need none: rel-L2 2e-2, the project's
bound between equivalent decode paths (test_mmdit_kv_cache_decode_matches_full_forward)."""
import functools

import pytest
import torch

from oracle.params import det_init_

pytestmark = pytest.mark.gpu

MMCFG = dict(model_id="game_rft_audio", sample_size=8, channels=32, audio_channels=16, n_layers=2, n_heads=2,
             d_model=128, tokens_per_frame=65, n_buttons=11, n_mouse_axes=2, cfg_prob=0.1, n_frames=8, causal=True,
             uncond=False, backbone="mmdit", local_window=2, global_window=4, has_audio=True, rope_impl="motion",
             rope_ats_delta=2.0)
TPF = 65


def rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


@functools.lru_cache(maxsize=None)
def _model(n_frames=8, rope_impl="motion"):
    """the weights do not depend on n_frames or rope_impl: the RoPE tables are non-persistent buffers"""
    from owl_wms.configs import model_config
    from owl_wms.models.gamerft_audio import GameRFTAudio
    kw = dict(MMCFG, n_frames=n_frames, rope_impl=rope_impl)
    return det_init_(GameRFTAudio(model_config(**kw)), base_seed=5000).cuda().eval()


def _inputs(b, init, total, seed=7):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(b, init, 32, 8, 8, generator=g).bfloat16().cuda()
    audio = torch.randn(b, init, 16, generator=g).bfloat16().cuda()
    mouse = torch.randn(b, total, 2, generator=g).bfloat16().cuda()
    btn = (torch.rand(b, total, 11, generator=g) < 0.5).bfloat16().cuda()
    return x, audio, mouse, btn


def _stream(core, ins, frames, seed=321, **kw):
    """hand-driven AVFrameStream: (video [b, n, c, h, w], audio [b, n, ca], the stream after close, buffer
    addresses after start(), addresses and row counts after the last frame)"""
    from owl_wms.sampling.stream import AVFrameStream
    x, audio, mouse, btn = ins
    init = x.size(1)
    torch.manual_seed(seed)
    with AVFrameStream(core, **kw) as s:
        s.start(x, audio, mouse, btn)
        ptrs0 = [(kb.data_ptr(), vb.data_ptr()) for kb, vb in s.kv_cache.bufs]
        out = [s.step(mouse[:, init + i:init + i + 1], btn[:, init + i:init + i + 1]) for i in range(frames)]
        ptrs1 = [(kb.data_ptr(), vb.data_ptr()) for kb, vb in s.kv_cache.bufs]
        rows = [(kb.shape[1], vb.shape[1]) for kb, vb in s.kv_cache.bufs]
    torch.cuda.synchronize()
    return torch.cat([o[0] for o in out], 1), torch.cat([o[1] for o in out], 1), s, ptrs0, ptrs1, rows


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
    assert torch.isfinite(v.float()).all() and torch.isfinite(a.float()).all()
    assert rv <= 2e-2
    assert ra <= 2e-2


def _linear_loop(core, ins, frames, n_steps, cfg_scale, noise_prev, seed=321):
    """AVFrameStream's algorithm on the existing kernels only: SingleKVCache + MMDIT.enable_decoding
    (_forward_decode), the same draws in the same order, the same Euler arithmetic; no eviction."""
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
def test_ring_path_equals_the_existing_decode_path_before_the_first_eviction(cfg_scale):
    """3 context + 3 generated frames, max_cached_frames 6 (no eviction: offsets and cached lengths
    coincide), 3 steps: the ring kernels end to end == the linear joint-frame kernels, bit for bit."""
    m = _model(8)
    ins = _inputs(2, 3, 6)
    v, a, s, *_ = _stream(m.core, ins, 3, n_steps=3, cfg_scale=cfg_scale, noise_prev=0.2, max_cached_frames=6)
    assert s.kv_cache.start[0] == 0 and s.kv_cache.n_frames() == 6 and s.rebases == 0
    rv, ra = _linear_loop(m.core, ins, 3, 3, cfg_scale, 0.2)
    assert torch.isfinite(v.float()).all() and torch.isfinite(a.float()).all()
    assert torch.equal(v, rv) and torch.equal(a, ra)
    assert not m.core.transformer.decoding


def test_wrapping_ring_equals_a_ring_that_never_wraps():
    """3 context frames, max_cached_frames 4, 12 generated frames on the 32-frame table: the default ring of
    5 frames wraps (11 evictions), ring_frames 16 never does; eager and graphed; all bit-identical.  The
    buffers keep their 5 * 65 rows and their addresses."""
    m = _model(32)
    ins = _inputs(2, 3, 15)
    kw = dict(n_steps=3, cfg_scale=1.3, noise_prev=0.2, max_cached_frames=4)
    v, a, s, ptrs0, ptrs1, rows = _stream(m.core, ins, 12, **kw)
    assert torch.isfinite(v.float()).all() and torch.isfinite(a.float()).all()
    assert s.frames_generated == 12 and s.rebases == 0
    cap = 5 * TPF
    assert len(rows) == MMCFG["n_layers"] and all(r == (cap, cap) for r in rows)
    assert ptrs0 == ptrs1 and len({p for pair in ptrs0 for p in pair}) == 2 * MMCFG["n_layers"]
    assert s.kv_cache.n_frames() == 4 and s.kv_cache.get_offset(0) == 15 * TPF
    assert s.kv_cache.start[0] == (11 * TPF) % cap
    v16, a16, s16, *_ = _stream(m.core, ins, 12, ring_frames=16, **kw)
    assert s16.kv_cache.start[0] == 11 * TPF and s16.kv_cache.capacity == 16 * TPF  # never wrapped
    assert torch.equal(v, v16) and torch.equal(a, a16)
    for rf in (None, 16):
        vg, ag, sg, g0, g1, _ = _stream(m.core, ins, 12, graphed=True, ring_frames=rf, **kw)
        assert g0 == g1 and sg.frames_generated == 12
        assert torch.equal(vg, v) and torch.equal(ag, a), rf


def test_av_stream_past_the_rope_table():
    """n_frames 8 against 32 with the same weights, 3 context frames, max_cached_frames 4, 12 frames:
    positions would reach 15, so the short table's stream rebases at least twice.  Video and audio within
    rel-L2 2e-2 of the 32-frame table's stream; graphed == eager bit for bit."""
    short, long_ = _model(8), _model(32)
    for (ka, a_), (kb_, b_) in zip(sorted(short.state_dict().items()), sorted(long_.state_dict().items())):
        assert ka == kb_ and torch.equal(a_, b_), ka
    rs, rl = short.core.transformer.rope, long_.core.transformer.rope
    n = rs.cos.shape[0]
    assert n == 8 * TPF and rl.cos.shape[0] == 32 * TPF
    assert torch.equal(rs.cos, rl.cos[:n]) and torch.equal(rs.sin, rl.sin[:n])  # a bit-identical prefix
    ins = _inputs(2, 3, 15)
    kw = dict(n_steps=3, cfg_scale=1.3, noise_prev=0.2, max_cached_frames=4)
    rv, ra, s_ref, *_ = _stream(long_.core, ins, 12, **kw)
    assert s_ref.rebases == 0
    v, a, s, ptrs0, ptrs1, rows = _stream(short.core, ins, 12, **kw)
    assert s.rebases >= 2 and s.frames_generated == 12
    assert ptrs0 == ptrs1 and all(r == (5 * TPF, 5 * TPF) for r in rows)
    assert torch.isfinite(v.float()).all() and torch.isfinite(a.float()).all()
    ev, ea = rel(v, rv), rel(a, ra)
    print(f"AV stream past the table ({s.rebases} rebases) against the 32-frame table: video rel-L2 {ev:.3e}, "
          f"audio rel-L2 {ea:.3e}")
    vg, ag, sg, *_ = _stream(short.core, ins, 12, graphed=True, **kw)
    assert sg.rebases == s.rebases
    assert torch.equal(vg, v) and torch.equal(ag, a)
    assert ev <= 2e-2
    assert ea <= 2e-2


def test_ortho_rope_streams_to_the_end_of_its_table_then_raises():
    from owl_wms.sampling.stream import AVFrameStream
    ortho = _model(8, "ortho")
    x, audio, mouse, btn = _inputs(1, 3, 9)
    with AVFrameStream(ortho.core, n_steps=2, cfg_scale=1.0, max_cached_frames=4) as so:
        so.start(x, audio, mouse, btn)
        for i in range(5):  # positions 3..7: inside the table
            v, a = so.step(mouse[:, 3 + i:4 + i], btn[:, 3 + i:4 + i])
            assert torch.isfinite(v.float()).all() and torch.isfinite(a.float()).all()
        with pytest.raises(RuntimeError, match="cannot be rebased"):
            so.step(mouse[:, 8:9], btn[:, 8:9])
        assert so.frames_generated == 5 and so.rebases == 0
    torch.cuda.synchronize()


def test_ring_block_path_refuses_what_the_ring_cannot_serve():
    """More than one frame against a ring cache at offset > 0: a clear RuntimeError (as Attn._attend)."""
    from owl_wms.sampling.stream import AVFrameStream
    m = _model(8)
    x, audio, mouse, btn = _inputs(1, 3, 6)
    with AVFrameStream(m.core, n_steps=1, cfg_scale=1.0, max_cached_frames=5) as s:
        s.start(x, audio, mouse, btn)
        two = (x[:, :2], audio[:, :2], x.new_ones(1, 2), mouse[:, 3:5], btn[:, 3:5])
        with pytest.raises(RuntimeError, match="one joint frame at a time"):
            m.core(*two, kv_cache=s.kv_cache)
    torch.cuda.synchronize()


def test_av_audio_stream_registry_id():
    """sampler_id av_audio_stream == a hand-driven AVFrameStream with the same seed; it returns (x, audio,
    mouse, btn) with av_causal's shapes."""
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
    assert torch.equal(out[0][:, 3:], hv) and torch.equal(out[1][:, 3:], ha)
    # av_causal with a window of the 3 context frames extends the controls to the same length
    ref = get_sampler_cls("av_causal")(n_steps=2, cfg_scale=1.3, window_length=3, num_frames=7, noise_prev=0.2)(
        _model(32).core, x, audio, mouse[:, :3], btn[:, :3])
    assert [t.shape for t in out] == [t.shape for t in ref]
    short = smp(m.core, x, audio, mouse[:, :3], btn[:, :3])  # controls extended by batch_permute_to_length
    assert [t.shape for t in short] == [t.shape for t in ref]
    assert torch.equal(short[2][:, :3], mouse[:, :3]) and torch.isfinite(short[0].float()).all()
