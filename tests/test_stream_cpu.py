"""Host-side tests of endless frame streaming (no GPU): RingKVCache bookkeeping on CPU tensors, the
eviction rule shared with AVCachingSamplerV2's max_window, the linearity of the RoPE angle tables that
the rebase rests on, and the header / binding agreement of the new C entries."""
import ctypes
import os
import re
from types import SimpleNamespace

import pytest
import torch

from conftest import REPO

NEW_ENTRIES = ("owlk_qk_rope_fwd_kv_ring", "owlk_attn_decode_ring_fwd", "owlk_rope_rebase")
TPF, D_MODEL = 4, 8


def _cfg(n_layers=2):
    return SimpleNamespace(n_layers=n_layers, tokens_per_frame=TPF, n_heads=1, d_model=D_MODEL, backbone="dit")


def _frame(idx, b=1):
    """K / V rows of frame idx: every element of token t is the token's global index (V: negated)"""
    ids = torch.arange(idx * TPF, (idx + 1) * TPF, dtype=torch.float32)
    k = ids[None, :, None].expand(b, TPF, D_MODEL).contiguous()
    return k, -k


def test_ring_cache_bookkeeping(monkeypatch):
    from owl_wms import kernels
    from owl_wms.nn.kv_cache import RingKVCache, SingleKVCache
    cfg = _cfg()
    cap = 3 * TPF
    c = RingKVCache(cfg, cap, rope=SimpleNamespace(cos="cos", sin="sin"))
    assert isinstance(c, SingleKVCache) and c.ring
    c.reset(1)
    ctx = [torch.cat(t, 1) for t in zip(_frame(0), _frame(1))]  # 2 context frames, from row 0
    for i in range(cfg.n_layers):
        c.update(ctx[0], ctx[1], i)
    assert c.start == [0, 0] and c.len == [2 * TPF] * 2 and c.offsets == [2 * TPF] * 2
    ptrs = [(kb.data_ptr(), vb.data_ptr()) for kb, vb in c.bufs]
    assert all(kb.shape == (1, cap, D_MODEL) and vb.shape == (1, cap, D_MODEL) for kb, vb in c.bufs)
    c.enable_device_state()
    assert c.dev.tolist() == [0, 2 * TPF, 2 * TPF, 0]
    evicted = 0
    for f in range(2, 12):  # 10 frames through a 3-frame ring, 2 kept: it wraps three times
        k, v = _frame(f)
        for i in range(cfg.n_layers):
            both_k, both_v = c.extend(i, k, v)  # what the ring rope kernel writes, then [cache | new]
            want = torch.arange((f - 2) * TPF, (f + 1) * TPF, dtype=torch.float32)
            assert torch.equal(both_k[0, :, 0], want) and torch.equal(both_v[0, :, 0], -want)
            assert c.len[i] == 2 * TPF  # extend does not commit
            c.commit_device(i, TPF)
        assert c.n_frames() == 3 and c.get_offset(0) == (f + 1) * TPF
        with pytest.raises(AssertionError, match="capacity"):
            c.commit_device(0, TPF)
        c.truncate(1, front=False)
        evicted += 1
        assert c.start == [(evicted * TPF) % cap] * 2 and c.len == [2 * TPF] * 2
        assert c.offsets == [(f + 1) * TPF] * 2  # truncate keeps the offsets
        assert c.dev.tolist() == [c.start[0], 2 * TPF, (f + 1) * TPF, 0]
        kk, vv = c.get(1)
        assert torch.equal(kk[0, :, 0], torch.arange((f - 1) * TPF, (f + 1) * TPF, dtype=torch.float32))
        assert torch.equal(vv, -kk)
    assert [(kb.data_ptr(), vb.data_ptr()) for kb, vb in c.bufs] == ptrs
    assert all(kb.shape[1] == cap for kb, _ in c.bufs)
    # front=True drops the newest frame: the start stays
    s0 = c.start[0]
    c.truncate(1, front=True)
    assert c.start == [s0] * 2 and c.len == [TPF] * 2
    for i in range(cfg.n_layers):
        c.commit_device(i, TPF)  # back to 2 frames (positions keep counting)
    # rebase: one owlk_rope_rebase per layer over the live rows, then the offsets drop
    calls = []
    monkeypatch.setattr(kernels, "rope_rebase", lambda kb, H, D, start, rows, cos, sin, old, new: calls.append(
        (kb.data_ptr(), H, D, start, rows, cos, sin, old, new)))
    off = c.get_offset(0)
    oldest = off - len(c)
    with pytest.raises(AssertionError, match="whole frames"):
        c.rebase(TPF + 1)
    with pytest.raises(RuntimeError, match="below 0"):
        c.rebase(oldest + TPF)
    assert calls == [] and c.offsets == [off] * 2
    c.rebase(oldest)
    assert calls == [(ptrs[i][0], 1, D_MODEL, s0, 2 * TPF, "cos", "sin", oldest, 0) for i in range(cfg.n_layers)]
    assert c.offsets == [2 * TPF] * 2 and c.start == [s0] * 2 and c.len == [2 * TPF] * 2
    assert c.dev.tolist() == [s0, 2 * TPF, 2 * TPF, 0]
    c.rebase(0)
    assert len(calls) == cfg.n_layers
    # the existing factory and class are untouched
    from owl_wms.nn.kv_cache import KVCache
    assert type(KVCache(_cfg())) is SingleKVCache and not getattr(KVCache(_cfg()), "ring", False)


@pytest.mark.parametrize("init_len", [1, 3, 8])
@pytest.mark.parametrize("extra", [0, 1, 5])
def test_eviction_rule_matches_sampler_max_window(init_len, extra):
    """FrameStream(max_cached_frames=M) evicts exactly when AVCachingSamplerV2(max_window=M - init_len + 1)
    does (that sampler counts list entries, the context as one), and the ring never holds more than
    M + 1 frames -- its capacity.  Pure counting on the two caches' bookkeeping."""
    from owl_wms.nn.kv_cache import RingKVCache, SingleKVCache
    M = init_len + extra
    max_window = M - init_len + 1
    cfg = _cfg(1)
    n_new = 3 * (M + 2)
    ring = RingKVCache(cfg, (M + 1) * TPF)
    lin = SingleKVCache(cfg)
    z = torch.zeros(1, init_len * TPF, D_MODEL)
    for c in (ring, lin):
        c.reset(1)
        c.update(z, z, 0)
    lin.enable_device_state((init_len + n_new + 1) * TPF)
    latents = 1  # the sampler's list: the context is one entry
    for idx in range(n_new):
        ring.commit_device(0, TPF)
        lin.commit_device(0, TPF)
        latents += 1
        stream_evicts = ring.n_frames() > M
        sampler_evicts = latents > max_window
        assert stream_evicts == sampler_evicts, idx
        assert ring.n_frames() <= M + 1
        if stream_evicts:
            ring.truncate(1, front=False)
            lin.truncate(1, front=False)
        assert len(ring) == len(lin) and ring.get_offset(0) == lin.get_offset(0)
        assert ring.start[0] == lin.start[0] % ring.capacity
    assert ring.n_frames() == M
    assert lin.bufs[0][0].shape[1] > ring.bufs[0][0].shape[1] == (M + 1) * TPF


@pytest.mark.parametrize("impl", ["motion", "audio1d"])
def test_rope_angles_are_linear_in_the_frame_index(impl):
    """The rebase's premise.  The exact angle of (frame f, token) is position x frequency with the
    position linear in f, and the fp32 table rounds each product once (relative error <= 2^-24).  So in
    fp64 the difference for an s-frame shift is constant over (frame, token) up to 2^-22 max|angle|
    (two roundings per difference, two differences compared), and a shorter table is a bit-identical
    prefix of a longer one."""
    from owl_wms.configs import model_config
    from owl_wms.nn.rope import get_rope_cls
    kw = dict(model_id="game_rft", sample_size=8, channels=32, n_layers=2, n_heads=2, d_model=128,
              tokens_per_frame=64, n_buttons=11, n_frames=8, causal=True, backbone="dit", has_audio=False,
              rope_impl=impl, rope_ats_delta=2.0, local_window=2, global_window=None)
    tabs = {}
    for nf in (8, 32):
        # the 1-D table has one position per frame, the audio slot (RoPE.__init__ drops it otherwise)
        cfg = model_config(**dict(kw, n_frames=nf, has_audio=impl == "audio1d"))
        rope = get_rope_cls(impl)(cfg)
        ang = rope.get_freqs(cfg)
        ang = ang.view(nf, -1, ang.size(-1))
        if impl == "motion":
            ang = ang[:, :-1]
        assert rope.cos.shape == (nf * ang.shape[1], 32)
        tabs[nf] = (ang.double(), rope.cos, rope.sin)
    n8 = tabs[8][1].shape[0]
    assert torch.equal(tabs[8][1], tabs[32][1][:n8]) and torch.equal(tabs[8][2], tabs[32][2][:n8])
    for nf in (8, 32):
        a = tabs[nf][0]  # [frames, tokens, D/2]
        bound = 2.0 ** -22 * a.abs().max().item()
        for s in (1, 3, 5):
            d = a[s:] - a[:-s]
            spread = (d.amax(0) - d.amin(0)).max().item()  # over frames, per (token, pair)
            tok_spread = (d.amax((0, 1)) - d.amin((0, 1))).max().item()  # over frames and tokens
            assert spread <= bound and tok_spread <= bound, (nf, s, spread, tok_spread, bound)


def _header_protos():
    hdr = re.sub(r"/\*.*?\*/", " ", open(os.path.join(REPO, "include", "owlk.h")).read(), flags=re.S)
    protos = {}
    for m in re.finditer(r"\b(?:int|long)\s+(owlk_\w+)\s*\(([^)]*)\)\s*;", hdr):
        kinds = []
        for a in [x.strip() for x in m.group(2).split(",")]:
            if a in ("", "void"):
                continue
            if "*" in a:
                kinds.append("P")
            else:
                kinds.append({"long": "L", "int": "I", "float": "F"}[re.match(r"(?:const\s+)?(long|int|float)\b", a).group(1)])
        protos[m.group(1)] = kinds
    return protos


def test_new_entries_header_binding_and_library_agree():
    from owl_wms._lib import LIB_PATH, _SIGS, exported_symbols
    kind = {ctypes.c_void_p: "P", ctypes.c_long: "L", ctypes.c_int: "I", ctypes.c_float: "F"}
    protos = _header_protos()
    for name in NEW_ENTRIES:
        assert name in protos and name in _SIGS and name in exported_symbols(), name
        assert [kind[a] for a in _SIGS[name]] == protos[name], name
    # the ring forms take exactly the linear forms' arguments
    assert protos["owlk_qk_rope_fwd_kv_ring"] == protos["owlk_qk_rope_fwd_kv_dev"]
    assert protos["owlk_attn_decode_ring_fwd"] == protos["owlk_attn_decode_fwd"]
    hdr = open(os.path.join(REPO, "include", "owlk.h")).read()
    for name in NEW_ENTRIES:  # a header comment citing the reference lines it serves, like its neighbours
        comment = hdr[:hdr.index("int " + name)].rsplit("/*", 1)[1]
        assert re.search(r"\w+\.py(:\d+)?", comment), name
    assert os.path.exists(LIB_PATH), "libowlk.so not built (run __graft_entry__.build())"
    h = ctypes.CDLL(LIB_PATH)
    for name in NEW_ENTRIES:
        assert hasattr(h, name), name


def test_sampler_registry_has_av_stream():
    from owl_wms.sampling import get_sampler_cls
    from owl_wms.sampling.stream import FrameStream, StreamSampler
    assert get_sampler_cls("av_stream") is StreamSampler
    s = StreamSampler(n_steps=2, cfg_scale=1.0, num_frames=3, noise_prev=0.2, max_window=2, custom_schedule=None)
    assert (s.n_steps, s.num_frames, s.max_window) == (2, 3, 2)
    core = SimpleNamespace(config=SimpleNamespace(n_frames=8, d_model=128, n_heads=2, tokens_per_frame=64,
                                                  backbone="dit"))
    with pytest.raises(ValueError, match="n_frames"):
        FrameStream(core, max_cached_frames=7)
    with pytest.raises(RuntimeError, match="before start"):
        FrameStream(core, max_cached_frames=4).step(None, None)
