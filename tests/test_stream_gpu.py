"""Model-level tests of endless frame streaming (owl_wms/sampling/stream.py: FrameStream on a
RingKVCache, sampler id av_stream) on the tiny GameRFT of tests/test_model_gpu.py.

Ring against linear: the stream is AVCachingSamplerV2 on ring buffers, same kernels' arithmetic in the
same order and the same torch draws, so torch.equal.  Past the RoPE table: each rebase rounds the cached
K to bf16 once more and the table carries fp32 angles, so the frames agree with a model whose table is
long enough within the project's bound for sampled latents between equivalent decode paths, rel-L2 2e-2
(the device-state against host-state sampler pair at the same shape is printed beside it)."""
import functools

import pytest
import torch

from oracle.params import det_init_

pytestmark = pytest.mark.gpu

TINY = dict(model_id="game_rft", sample_size=8, channels=32, n_layers=2, n_heads=2, d_model=128,
            tokens_per_frame=64, n_buttons=11, cfg_prob=0.1, n_frames=8, causal=True, uncond=False,
            backbone="dit", has_audio=False, rope_impl="motion", rope_ats_delta=2.0, local_window=2,
            global_window=None)


def rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


@functools.lru_cache(maxsize=None)
def _model(d_model=128, n_frames=8, rope_impl="motion"):
    """tests/test_model_gpu.py's _model with the RoPE table length / kind as arguments (the weights do
    not depend on either: the tables are non-persistent buffers)"""
    from owl_wms.configs import model_config
    from owl_wms.models.gamerft import GameRFT
    kw = dict(TINY, d_model=d_model, n_frames=n_frames, rope_impl=rope_impl)
    return det_init_(GameRFT(model_config(**kw)), base_seed=1000 if d_model == 128 else 1100).cuda().eval()


def _inputs(b, init, total, seed=7):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(b, init, 32, 8, 8, generator=g).bfloat16().cuda()
    mouse = torch.randn(b, total, 2, generator=g).bfloat16().cuda()
    btn = (torch.rand(b, total, 11, generator=g) < 0.5).bfloat16().cuda()
    return x, mouse, btn


def _stream(core, x, mouse, btn, frames, seed=321, **kw):
    """hand-driven FrameStream: (frames [b, n, c, h, w], the stream after close, buffer addresses after
    start(), buffer addresses and row counts after the last frame)"""
    from owl_wms.sampling.stream import FrameStream
    init = x.size(1)
    torch.manual_seed(seed)
    with FrameStream(core, **kw) as s:
        s.start(x, mouse, btn)
        ptrs0 = [(kb.data_ptr(), vb.data_ptr()) for kb, vb in s.kv_cache.bufs]
        out = [s.step(mouse[:, init + i:init + i + 1], btn[:, init + i:init + i + 1]) for i in range(frames)]
        ptrs1 = [(kb.data_ptr(), vb.data_ptr()) for kb, vb in s.kv_cache.bufs]
        rows = [(kb.shape[1], vb.shape[1]) for kb, vb in s.kv_cache.bufs]
    torch.cuda.synchronize()
    return torch.cat(out, 1), s, ptrs0, ptrs1, rows


@pytest.mark.parametrize("graphed", [False, True])
@pytest.mark.parametrize("cfg_scale", [1.3, 1.0])
@pytest.mark.parametrize("d_model", [128, 256])
def test_ring_stream_equals_linear_sampler(d_model, cfg_scale, graphed):
    """3 context frames, max_cached_frames 6, 14 generated frames: the 7-frame ring wraps twice.
    == av_caching with max_window 4 (the same eviction rule) bit for bit; the buffers keep their
    7 * 64 rows and their addresses."""
    from owl_wms.sampling import get_sampler_cls
    m = _model(d_model, 32)
    x, mouse, btn = _inputs(2, 3, 17)
    torch.manual_seed(321)
    ref = get_sampler_cls("av_caching")(n_steps=4, cfg_scale=cfg_scale, num_frames=14, noise_prev=0.2, max_window=4)(
        m.core, x, mouse, btn, compile_on_decode=graphed)
    out, s, ptrs0, ptrs1, rows = _stream(m.core, x, mouse, btn, 14, n_steps=4, cfg_scale=cfg_scale, noise_prev=0.2,
                                         max_cached_frames=6, graphed=graphed)
    assert ref.shape == (2, 17, 32, 8, 8) and out.shape == (2, 14, 32, 8, 8)
    assert torch.isfinite(out.float()).all()
    assert torch.equal(out, ref[:, 3:])
    assert s.frames_generated == 14 and s.rebases == 0
    assert s.kv_cache.n_frames() == 6 and s.kv_cache.get_offset(0) == 17 * 64
    assert s.kv_cache.start[0] == (11 * 64) % (7 * 64)  # 11 evictions on a 7-frame ring: wrapped


def test_ring_memory_is_bounded():
    """After 14 frames every layer's buffers still have 7 * 64 rows at the addresses from after start()."""
    m = _model(128, 32)
    x, mouse, btn = _inputs(2, 3, 17)
    _, s, ptrs0, ptrs1, rows = _stream(m.core, x, mouse, btn, 14, n_steps=2, cfg_scale=1.3, noise_prev=0.2,
                                       max_cached_frames=6)
    assert len(rows) == TINY["n_layers"] and all(r == (7 * 64, 7 * 64) for r in rows)
    assert ptrs0 == ptrs1 and len({p for pair in ptrs0 for p in pair}) == 2 * TINY["n_layers"]


def test_stream_past_the_rope_table():
    """n_frames 8, 3 context frames, max_cached_frames 4, 12 generated frames: positions would reach
    15, so the stream rebases (at frames 5 and 9).  Against the same weights with a 32-frame table and no
    rebase, same seed: generated frames within rel-L2 2e-2; graphed == eager bit for bit."""
    from owl_wms.sampling import get_sampler_cls
    short, long_ = _model(128, 8), _model(128, 32)
    for (ka, a), (kb_, b) in zip(sorted(short.state_dict().items()), sorted(long_.state_dict().items())):
        assert ka == kb_ and torch.equal(a, b), ka
    rs, rl = short.core.transformer.rope, long_.core.transformer.rope
    n = rs.cos.shape[0]
    assert n == 8 * 64 and rl.cos.shape[0] == 32 * 64
    assert torch.equal(rs.cos, rl.cos[:n]) and torch.equal(rs.sin, rl.sin[:n])  # a bit-identical prefix
    x, mouse, btn = _inputs(2, 3, 15)
    kw = dict(n_steps=4, cfg_scale=1.3, noise_prev=0.2, max_cached_frames=4)
    ref, s_ref, *_ = _stream(long_.core, x, mouse, btn, 12, **kw)
    assert s_ref.rebases == 0
    out, s, ptrs0, ptrs1, rows = _stream(short.core, x, mouse, btn, 12, **kw)
    assert s.rebases >= 2 and s.frames_generated == 12
    assert ptrs0 == ptrs1 and all(r == (5 * 64, 5 * 64) for r in rows)
    assert torch.isfinite(out.float()).all()
    # the yardstick: two existing, equivalent decode paths (device-state against host-state sampler)
    yard = []
    for dev in (False, True):
        torch.manual_seed(321)
        smp = get_sampler_cls("av_caching")(n_steps=4, cfg_scale=1.3, num_frames=12, noise_prev=0.2, max_window=2)
        smp.device_state = dev
        yard.append(smp(long_.core, x, mouse, btn)[:, 3:].float())
    r = rel(out, ref)
    print(f"stream past the table ({s.rebases} rebases) against the 32-frame table: rel-L2 {r:.3e}; "
          f"yardstick device-state against host-state sampler: rel-L2 {rel(yard[1], yard[0]):.3e}")
    assert torch.equal(ref, yard[1].to(ref.dtype))  # the no-rebase stream is the device-state sampler
    out_g, s_g, *_ = _stream(short.core, x, mouse, btn, 12, graphed=True, **kw)
    assert s_g.rebases == s.rebases
    assert torch.equal(out_g, out)
    assert r <= 2e-2


def test_av_stream_registry_id():
    """sampler_id av_stream -> [b, init + num_frames, c, h, w], equal to a hand-driven FrameStream."""
    from owl_wms.sampling import get_sampler_cls
    m = _model(128, 8)
    x, mouse, btn = _inputs(2, 3, 13)
    torch.manual_seed(321)
    smp = get_sampler_cls("av_stream")(n_steps=2, cfg_scale=1.3, num_frames=10, noise_prev=0.2, max_window=2)
    out = smp(m.core, x, mouse, btn)
    assert out.shape == (2, 13, 32, 8, 8) and torch.equal(out[:, :3], x)
    hand, s, *_ = _stream(m.core, x, mouse, btn, 10, n_steps=2, cfg_scale=1.3, noise_prev=0.2, max_cached_frames=4)
    assert s.rebases >= 1  # 3 + 10 frames on an 8-frame table
    assert torch.equal(out[:, 3:], hand)


def test_stream_refusals():
    from owl_wms.sampling.stream import FrameStream
    m = _model(128, 8)
    with pytest.raises(ValueError, match="n_frames"):
        FrameStream(m.core, n_steps=2, max_cached_frames=7)
    s = FrameStream(m.core, n_steps=2, max_cached_frames=4)
    x, mouse, btn = _inputs(1, 3, 9)
    with pytest.raises(RuntimeError, match="before start"):
        s.step(mouse[:, 3:4], btn[:, 3:4])
    ortho = _model(128, 8, "ortho")
    with FrameStream(ortho.core, n_steps=2, cfg_scale=1.0, max_cached_frames=4) as so:
        so.start(x, mouse, btn)
        for i in range(5):  # positions 3..7: inside the table
            so.step(mouse[:, 3 + i:4 + i], btn[:, 3 + i:4 + i])
        with pytest.raises(RuntimeError, match="cannot be rebased"):
            so.step(mouse[:, 8:9], btn[:, 8:9])
        assert so.frames_generated == 5 and so.rebases == 0
    torch.cuda.synchronize()
