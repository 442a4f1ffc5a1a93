"""GPU tests of endless audio streaming (owl_wms/sampling/stream.py: AudioStream on a RingKVCache, sampler id
audio_stream) on the tiny audio_rft of tests/test_model_gpu.py with local_window 2, so the windowed ring
decode runs.

The stream decodes one token per forward: owlk_qk_rope_fwd_kv_ring + owlk_attn_decode_ring_fwd at ONE query
row against rings shorter than a 64-key tile -- shapes no earlier test runs, so the first test here is at
kernel level.

Bounds.  Ring against linear kernels, ring sizes and graph modes against each other: torch.equal (the same
arithmetic in the same order).  The decode attention against an fp64 softmax of the same bf16 inputs: rel-L2
5e-3, the bound tests/test_kernels_gpu.py::test_attention_decode_device_state holds the device-state decode
attention to.  Stream against audio_caching (different attention kernels) and a rebased stream against a
table long enough to need no rebase: rel-L2 2e-2, the project's bound between equivalent decode paths."""
import functools

import pytest
import torch

from oracle.params import det_init_

pytestmark = pytest.mark.gpu

DEV = "cuda"
AUDIO = dict(model_id="audio_rft", sample_size=120, channels=64, n_layers=2, n_heads=2, d_model=128,
             tokens_per_frame=1, n_frames=32, cfg_prob=0.0, causal=True, uncond=True, backbone="dit", has_audio=True,
             rope_impl="audio1d", local_window=2, global_window=None)


def rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


def rnd(*shape, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g).to(torch.bfloat16).to(DEV)


def unit(t, D):
    """rows RMS-normalised per head (what the rope kernels hand the attention: |q.k| <= D)"""
    f = t.float().view(*t.shape[:-1], -1, D)
    return (f * torch.rsqrt(f.pow(2).mean(-1, keepdim=True))).bfloat16().view(t.shape)


def dev_state(*v):
    return torch.tensor(list(v) + [0] * (4 - len(v)), dtype=torch.int64, device=DEV)


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


CAP, B, H, D = 300, 2, 2, 64
CACHED = (0, 15, 16, 62, 63, 64, 254, 255, 256)


def test_one_token_ring_decode_kernels():
    """owlk_attn_decode_ring_fwd at Lq = Lnew = 1 on a 300-row ring, for cached counts around the 16-row DMA
    group and the 64-key tile (0: the new row alone), with and without a 16-key window, unwrapped and wrapped
    (start = cap - 7): o and lse == owlk_attn_decode_fwd on the unrolled copy bit for bit, and o within 5e-3
    rel-L2 of the fp64 softmax over the same keys.  owlk_qk_rope_fwd_kv_ring at L = 1: q and the one K / V row
    it writes == owlk_qk_rope_fwd_kv_dev's on the unrolled copy."""
    from owl_wms import kernels as k
    from owl_wms.nn.rope import lang_freqs
    q = unit(rnd(B, 1, H * D, seed=1), D)
    kb = unit(rnd(B, CAP, H * D, seed=2), D)
    vb = rnd(B, CAP, H * D, seed=3)
    bound = k.qk_norm_bound(D)
    ang = torch.arange(CAP + 8, dtype=torch.float32)[:, None] * lang_freqs(D)[None]
    cos, sin = ang.cos().to(DEV).contiguous(), ang.sin().to(DEV).contiguous()
    qkv = rnd(B, 3 * H * D, seed=4)
    worst = 0.0
    for start in (0, CAP - 7):
        kl, vl = torch.roll(kb, -start, 1).contiguous(), torch.roll(vb, -start, 1).contiguous()
        for cached in CACHED:
            total = cached + 1
            for window in (0, 16):
                o, lse = k.attn_decode_ring_fwd(q, kb, vb, H, D, dev_state(start, cached), 1, window, score_bound=bound)
                o0, lse0 = k.attn_decode_fwd(q, kl, vl, H, D, dev_state(0, cached), 1, window, score_bound=bound)
                case = (start, cached, window)
                assert torch.isfinite(o.float()).all() and torch.isfinite(lse).all(), case
                assert torch.equal(o, o0) and torch.equal(lse, lse0), case
                first = total - window if 0 < window < total else 0
                ks = kl[:, first:total].double().view(B, -1, H, D)
                vs = vl[:, first:total].double().view(B, -1, H, D)
                p = torch.einsum("bhd,bkhd->bhk", q.double().view(B, H, D), ks) * D ** -0.5
                ref = torch.einsum("bhk,bkhd->bhd", p.softmax(-1), vs).reshape(B, 1, H * D)
                r = rel(o, ref)
                worst = max(worst, r)
                assert r < 5e-3, (case, r)
            # the rope kernel's single row: the new token's K / V behind `cached` rows, wrapped or not
            kr, vr = kb.clone(), vb.clone()
            krl, vrl = kl.clone(), vl.clone()
            qo = torch.zeros(B, 1, H * D, device=DEV, dtype=torch.bfloat16)
            ql = torch.zeros_like(qo)
            k.qk_rope_fwd_kv_ring(qkv, B, 1, H, D, cos, sin, dev_state(start, cached, cached + 5), qo, kr, vr)
            k.qk_rope_fwd_kv_dev(qkv, B, 1, H, D, cos, sin, dev_state(0, cached, cached + 5), ql, krl, vrl)
            assert torch.equal(qo, ql), (start, cached)
            assert torch.equal(torch.roll(kr, -start, 1), krl) and torch.equal(torch.roll(vr, -start, 1), vrl)
            row = (start + cached) % CAP
            changed = (kr != kb).any(-1).any(0).nonzero().flatten().tolist()
            assert changed == [row] and torch.equal(vr[:, row], qkv[:, 2 * H * D:]), (start, cached)
    print(f"one-token ring decode attention against fp64: worst rel-L2 {worst:.3e} (bound 5e-3)")


@functools.lru_cache(maxsize=None)
def _model(n_frames=32):
    """tests/test_model_gpu.py's tiny audio_rft (seed 3000) with local_window 2 and the table length as an
    argument (the weights do not depend on it: the tables are non-persistent buffers)"""
    from owl_wms.configs import model_config
    from owl_wms.models.audiorft import AudioRFT
    return det_init_(AudioRFT(model_config(**dict(AUDIO, n_frames=n_frames))), base_seed=3000).cuda().eval()


def _inputs(b, init, seed=7):
    return torch.randn(b, init, 64, generator=torch.Generator().manual_seed(seed)).bfloat16().cuda()


def _stream(core, x, tokens, seed=321, **kw):
    """hand-driven AudioStream: (tokens [b, n, c], the stream after close, buffer addresses after start() and
    after the last token)"""
    from owl_wms.sampling.stream import AudioStream
    torch.manual_seed(seed)
    with AudioStream(core, **kw) as s:
        s.start(x)
        ptrs0 = [(kb.data_ptr(), vb.data_ptr()) for kb, vb in s.kv_cache.bufs]
        out = [s.step() for _ in range(tokens)]
        ptrs1 = [(kb.data_ptr(), vb.data_ptr()) for kb, vb in s.kv_cache.bufs]
    torch.cuda.synchronize()
    return torch.cat(out, 1), s, ptrs0, ptrs1


def test_audio_stream_against_audio_caching():
    """8 context tokens + 4 generated, 2 steps, no eviction, same seed: the same draws in the same order, the
    ring decode kernels against audio_caching's attention over [cache | new] views."""
    from owl_wms.sampling import get_sampler_cls
    m = _model(32)
    x = _inputs(2, 8)
    torch.manual_seed(321)
    ref = get_sampler_cls("audio_caching")(n_steps=2, num_tokens=4, noise_prev=0.2)(m.core, x)
    out, s, *_ = _stream(m.core, x, 4, n_steps=2, noise_prev=0.2, max_cached_frames=12)
    assert ref.shape == (2, 12, 64) and out.shape == (2, 4, 64)
    assert s.frames_generated == 4 and s.kv_cache.start[0] == 0 and len(s.kv_cache) == 12
    r = rel(out, ref[:, 8:])
    print(f"audio stream against audio_caching, 4 tokens: rel-L2 {r:.3e}")
    assert torch.isfinite(out.float()).all()
    assert not m.core.transformer.decoding
    assert r <= 2e-2


def test_wrapping_ring_equals_a_ring_that_never_wraps_and_the_graphs():
    """3 context tokens, max_cached_frames 4, 12 tokens on the 32-row table: the default 5-row ring wraps
    (11 evictions), ring_frames 16 never does; step graph and frame graph; all bit-identical."""
    m = _model(32)
    x = _inputs(2, 3)
    kw = dict(n_steps=3, noise_prev=0.2, max_cached_frames=4)
    out, s, ptrs0, ptrs1 = _stream(m.core, x, 12, **kw)
    assert torch.isfinite(out.float()).all() and s.frames_generated == 12 and s.rebases == 0
    assert ptrs0 == ptrs1 and all(kb.shape[1] == 5 for kb, _ in s.kv_cache.bufs)
    assert (s.kv_cache.start[0], len(s.kv_cache), s.kv_cache.get_offset(0)) == (11 % 5, 4, 15)
    o16, s16, *_ = _stream(m.core, x, 12, ring_frames=16, **kw)
    assert s16.kv_cache.start[0] == 11 and s16.kv_cache.capacity == 16  # never wrapped
    assert torch.equal(o16, out)
    og, sg, g0, g1 = _stream(m.core, x, 12, graphed=True, **kw)
    assert g0 == g1 and sg.graph_replays == 12 * 3 - 1 and torch.equal(og, out)
    of, sf, f0, f1 = _stream(m.core, x, 12, graphed="frame", **kw)
    assert f0 == f1 and sf.graph_replays == 11 and torch.equal(of, out)
    assert sf.kv_cache.device_state() == (1, 4, 15)


def test_audio_stream_past_the_rope_table():
    """n_frames 8 against 32 with the same weights, 3 context tokens, max_cached_frames 4, 12 tokens: positions
    would reach 15, so the short table's stream rebases at least twice.  Within rel-L2 2e-2 of the 32-row
    table's stream (measured on an MI355X: 4.8e-4 with 2 rebases); eager, step graph and frame graph
    bit-identical."""
    short, long_ = _model(8), _model(32)
    for (ka, a), (kb_, b) in zip(sorted(short.state_dict().items()), sorted(long_.state_dict().items())):
        assert ka == kb_ and torch.equal(a, b), ka
    rs, rl = short.core.transformer.rope, long_.core.transformer.rope
    assert rs.cos.shape == (8, 32) and rl.cos.shape == (32, 32)
    assert torch.equal(rs.cos, rl.cos[:8]) and torch.equal(rs.sin, rl.sin[:8])  # a bit-identical prefix
    x = _inputs(2, 3)
    kw = dict(n_steps=3, noise_prev=0.2, max_cached_frames=4)
    ref, s_ref, *_ = _stream(long_.core, x, 12, **kw)
    assert s_ref.rebases == 0
    out, s, ptrs0, ptrs1 = _stream(short.core, x, 12, **kw)
    assert s.rebases >= 2 and s.frames_generated == 12 and ptrs0 == ptrs1
    assert torch.isfinite(out.float()).all()
    r = rel(out, ref)
    print(f"audio stream past the table ({s.rebases} rebases) against the 32-row table: rel-L2 {r:.3e}")
    for mode in (True, "frame"):
        og, sg, *_ = _stream(short.core, x, 12, graphed=mode, **kw)
        assert sg.rebases == s.rebases and torch.equal(og, out), mode
    assert r <= 2e-2


def test_audio_stream_registry_id():
    """sampler id audio_stream -> [b, init + num_tokens, c], equal to a hand-driven AudioStream; max_window
    counts as audio_caching's (the context as one entry): max_window 2 with 3 context tokens caches 4."""
    from owl_wms.sampling import get_sampler_cls
    m = _model(8)
    x = _inputs(2, 3)
    hand, s, *_ = _stream(m.core, x, 10, n_steps=2, noise_prev=0.2, max_cached_frames=4)
    assert s.rebases >= 1  # 3 + 10 tokens on an 8-row table
    for kw, graph in ((dict(), False), (dict(), True), (dict(frame_graph=True), True)):
        torch.manual_seed(321)
        smp = get_sampler_cls("audio_stream")(n_steps=2, num_tokens=10, noise_prev=0.2, max_window=2, **kw)
        out = smp(m.core, x, compile_on_decode=graph)
        assert out.shape == (2, 13, 64) and torch.equal(out[:, :3], x)
        assert torch.equal(out[:, 3:], hand), (kw, graph)
    full, wav = smp(m.core, x, decode_fn=lambda z: z * 2.0, vae_scale=0.5)
    assert full.shape == (2, 13, 64) and wav.shape == full.shape
