"""Host-side tests of multi-session audio + video streaming (no GPU): the header / binding / library agreement of
the three audio + video slot entries, the constructor checks of AVStreamPool / AVDiTStreamPool, av_pool_cls, and
SlotRingKVCache's mirror against the per-slot rule written out at 65 rows per frame."""
import ctypes
import os
import random
import re
from types import SimpleNamespace

import pytest
import torch

from conftest import REPO
from test_stream_cpu import _header_protos
from test_stream_pool_cpu import Model

# slot entry -> (single-state entry, index of n_slots in the slot entry's argument list)
ENTRIES = {
    "owlk_mm_qk_rope_fwd_kv_ring_slots": ("owlk_mm_qk_rope_fwd_kv_ring", 15),
    "owlk_attn_decode_joint_ring_slots_fwd": ("owlk_attn_decode_joint_ring_fwd", 22),
    "owlk_attn_decode_wide_ring_slots_fwd": ("owlk_attn_decode_wide_ring_fwd", 20),
}


def test_av_slot_entries_header_binding_and_library_agree():
    from owl_wms._lib import LIB_PATH, _SIGS, exported_symbols
    kind = {ctypes.c_void_p: "P", ctypes.c_long: "L", ctypes.c_int: "I", ctypes.c_float: "F"}
    protos = _header_protos()
    hdr = open(os.path.join(REPO, "include", "owlk.h")).read()
    assert os.path.exists(LIB_PATH), "libowlk.so not built (run __graft_entry__.build())"
    h = ctypes.CDLL(LIB_PATH)
    for name, (single, i) in ENTRIES.items():
        assert name in protos and name in _SIGS and name in exported_symbols(), name
        assert [kind[a] for a in _SIGS[name]] == protos[name], name
        # the single-state entry's arguments with n_slots (a long) right after state (its only long* argument)
        assert protos[single][i - 1] == "P" and protos[name] == protos[single][:i] + ["L"] + protos[single][i:], name
        args = re.search(r"int\s+" + name + r"\s*\(([^)]*)\)", hdr).group(1)
        assert re.search(r"const long\*\s*state,\s*long n_slots\b", args), name
        assert args.count("long*") == 1, name
        comment = hdr[:hdr.index("int " + name)].rsplit("/*", 1)[1]
        assert re.search(r"causvid_pipeline\.py:112-163", comment), name  # the reference lines it stands for
        assert re.search(r"mmattn\.py:46-86|attn\.py:86-107", comment), name
        assert hasattr(h, name), name
    text = open(os.path.join(REPO, "INTEGRATION.md")).read()
    assert all(name in text for name in ENTRIES)


def test_av_slot_entries_refuse_on_the_host():
    """B not a multiple of n_slots, n_slots < 1 and a null lse return 1 and launch nothing (no GPU needed)."""
    from owl_wms._lib import lib
    h = lib()
    a = 4096  # a non-null, 16-byte aligned address; a refused call launches nothing
    kv = (a, 128, 128 * 325, a, 128, 128 * 325)
    for B, n_slots, lse in ((6, 4, a), (6, 0, a), (6, -2, a), (6, 3, None), (0, 3, a), (65538, 2, a)):
        assert h.owlk_attn_decode_joint_ring_slots_fwd(a, 128, 128 * 65, *kv, a, 128, a, 128, lse, B, 2, 64, 1, 64,
                                                       0.125, 8.0, a, n_slots, 0, 325, None) == 1, (B, n_slots, lse)
        assert b"attn_decode_joint_ring_slots_fwd" in h.owlk_last_error()
        assert h.owlk_attn_decode_wide_ring_slots_fwd(a, 128, 128 * 65, *kv, a, 128, 128 * 65, lse, B, 2, 65, 64,
                                                      0.125, 8.0, a, n_slots, 65, 0, 325, None) == 1, (B, n_slots, lse)
        assert b"attn_decode_wide_ring_slots_fwd" in h.owlk_last_error()
    for B, n_slots in ((6, 4), (6, 0), (6, -2), (0, 3)):
        assert h.owlk_mm_qk_rope_fwd_kv_ring_slots(a, 384, a, 384, B, 1, 64, 1, 2, 64, a, a, 32, 2080, a, n_slots, a,
                                                   128, 128 * 65, *kv, 325, None) == 1, (B, n_slots)
        assert b"mm_qk_rope_fwd_kv_ring_slots" in h.owlk_last_error()


def _core(**kw):
    cfg = dict(n_frames=8, d_model=128, n_heads=2, n_layers=2, tokens_per_frame=65, sample_size=8, backbone="mmdit",
               rope_impl="motion")
    cfg.update(kw)
    return SimpleNamespace(config=SimpleNamespace(**cfg), parameters=lambda: iter([torch.zeros(1)]),
                           transformer=SimpleNamespace(rope=None))


def test_av_pool_cls_picks_by_backbone():
    from owl_wms.sampling.stream import AVDiTFrameStream, AVFrameStream
    from owl_wms.sampling.stream_pool import AVDiTStreamPool, AVStreamPool, StreamPool, av_pool_cls
    assert av_pool_cls("mmdit") is AVStreamPool and av_pool_cls("dit") is AVDiTStreamPool
    assert issubclass(AVStreamPool, AVFrameStream) and issubclass(AVDiTStreamPool, AVDiTFrameStream)
    assert AVDiTStreamPool.rebase_ropes == AVDiTFrameStream.rebase_ropes and "ortho" in AVDiTStreamPool.rebase_ropes
    assert "ortho" not in AVStreamPool.rebase_ropes
    # one pool logic for the three classes
    assert AVStreamPool.step is AVDiTStreamPool.step is StreamPool.step
    assert AVStreamPool.close is StreamPool.close and AVStreamPool.close_slot is StreamPool.close_slot


@pytest.mark.parametrize("backbone", ["mmdit", "dit"])
def test_constructor_checks(backbone):
    from owl_wms.sampling.stream_pool import av_pool_cls
    Pool = av_pool_cls(backbone)
    other = "dit" if backbone == "mmdit" else "mmdit"
    p = Pool(_core(backbone=backbone), 3, max_cached_frames=4, graphed="frame")
    assert (p.n_slots, p.ring_frames, p.graphed, p.live, p.graph_replays, p.ticks) == (3, 5, "frame", [], 0, 0)
    assert p.frames_generated == [0, 0, 0] and p.rebases == [0, 0, 0]
    assert p.kv_cache.bufs[0][0].shape == (6, 5 * 65, 128) and p.kv_cache.dev.shape == (3, 4)
    assert p._hc.tolist() == [True] * 3 + [False] * 3 and p._hc_one.tolist() == [True, False]
    q = Pool(_core(backbone=backbone), 2, cfg_scale=1.0, max_cached_frames=4)
    assert q.kv_cache.bufs[0][0].shape[0] == 2 and q._hc.tolist() == [True, True] and q._hc_one.tolist() == [True]
    assert Pool(_core(backbone=backbone), 1, max_cached_frames=4, ring_frames=9).ring_frames == 9
    for bad in (0, -1, 1.5, None, True):
        with pytest.raises(ValueError, match="n_slots"):
            Pool(_core(backbone=backbone), bad, max_cached_frames=4)
    for bad in ("bogus", 2, None):
        with pytest.raises(ValueError, match="graphed"):
            Pool(_core(backbone=backbone), 2, max_cached_frames=4, graphed=bad)
    with pytest.raises(ValueError, match="at least 1"):
        Pool(_core(backbone=backbone), 2, max_cached_frames=0)
    with pytest.raises(ValueError, match="n_frames"):
        Pool(_core(backbone=backbone), 2, max_cached_frames=7)
    with pytest.raises(ValueError, match="ring_frames"):
        Pool(_core(backbone=backbone), 2, max_cached_frames=4, ring_frames=4)
    with pytest.raises(ValueError, match=f"backbone '{other}'"):  # the stream's _check_core refusal
        Pool(_core(backbone=other), 2, max_cached_frames=4)
    with pytest.raises(ValueError, match="head_dim 32"):
        Pool(_core(backbone=backbone, d_model=64), 2, max_cached_frames=4)
    with pytest.raises(ValueError, match="head_dim 128"):
        Pool(_core(backbone=backbone, d_model=256), 2, max_cached_frames=4)
    if backbone == "dit":
        with pytest.raises(ValueError, match="81 tokens per frame"):
            Pool(_core(backbone=backbone, tokens_per_frame=81), 2, max_cached_frames=4)
        assert Pool(_core(backbone=backbone, tokens_per_frame=80), 2, max_cached_frames=4).kv_cache.capacity == 400
    with pytest.raises(RuntimeError, match=r"open\(video, audio, mouse, btn, seed\)"):
        p.start(None, None, None, None)
    with pytest.raises(ValueError, match="not live"):
        p.close_slot(0)
    assert p.step({}) == {}
    with pytest.raises(ValueError, match="live slots"):
        p.step({0: (None, None)})  # controls for a slot that is not live
    p.close()


@pytest.mark.parametrize("seed", [0, 1])
def test_mirror_follows_the_per_slot_rule_at_65_rows(seed):
    """the pool's cache (CFG batch, 65-row frames, 5-frame rings) against the rule written out per slot"""
    from owl_wms.sampling.stream_pool import AVStreamPool
    rng = random.Random(seed)
    L, ring_frames, max_frames, n = 65, 5, 4, 3
    c = AVStreamPool(_core(), n, max_cached_frames=max_frames).kv_cache
    assert c.capacity == ring_frames * L and c.dev.shape == (n, 4)
    model = [None] * n
    wraps = 0
    for step in range(300):
        r = rng.random()
        free = [s for s in range(n) if model[s] is None]
        if r < 0.15 and free:
            s = c.free_slot()
            assert s == min(free)
            rows = rng.randint(1, max_frames) * L
            c.open_slot(s, rows)
            model[s] = Model(rows, ring_frames * L)
        elif r < 0.25 and len(free) < n:
            s = rng.choice([s for s in range(n) if model[s] is not None])
            c.close_slot(s)
            model[s] = None
        else:
            before = [m.start if m else None for m in model]
            c.advance(L, max_frames * L, device=False)
            for m in model:
                if m:
                    m.advance(L, max_frames * L)
            wraps += sum(1 for m, b in zip(model, before) if m and m.start < b)
        want = [m.row() if m else (0, 0, 0, 0) for m in model]
        assert c.host_state() == want, step
        assert all(m is None or m.start % L == 0 and m.len % L == 0 for m in model)
    assert wraps >= 2  # rings went round
