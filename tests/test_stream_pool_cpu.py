"""Host-side tests of multi-session streaming (no GPU): SlotRingKVCache's mirror against a straightforward
per-slot model over random open / close / advance sequences, slot allocation, StreamPool's argument checks, and
the header / binding / library agreement of the three slot entries."""
import ctypes
import os
import random
import re
from types import SimpleNamespace

import pytest
import torch

from conftest import REPO
from test_stream_cpu import _header_protos

ENTRIES = {
    "owlk_qk_rope_fwd_kv_ring_slots": "owlk_qk_rope_fwd_kv_ring",
    "owlk_attn_decode_ring_slots_fwd": "owlk_attn_decode_ring_fwd",
    "owlk_ring_advance_slots": "owlk_ring_advance",
}


def _cache(n_slots, L=4, ring_frames=5, cfg=True):
    from owl_wms.nn.kv_cache import SlotRingKVCache
    config = SimpleNamespace(n_layers=2, tokens_per_frame=L, n_heads=1, d_model=8, backbone="dit")
    return SlotRingKVCache(config, ring_frames * L, n_slots, 2 * n_slots if cfg else n_slots, device="cpu")


class Model:
    """one session's ring position, the rule written out"""

    def __init__(self, rows, cap):
        self.start, self.len, self.off, self.cap = 0, rows, rows, cap

    def advance(self, L, max_rows):
        self.len += L
        self.off += L
        if self.len > max_rows:
            self.start = (self.start + L) % self.cap
            self.len -= L

    def row(self):
        return (self.start, self.len, self.off, 1)


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_mirror_follows_the_per_slot_rule(seed):
    rng = random.Random(seed)
    L, ring_frames, max_frames, n = 4, 5, 4, 4
    c = _cache(n, L, ring_frames)
    assert c.dev.shape == (n, 4) and all(kb.shape == (2 * n, ring_frames * L, 8) for kb, _ in c.bufs)
    model = [None] * n
    wraps = 0
    for step in range(400):
        r = rng.random()
        free = [s for s in range(n) if model[s] is None]
        if r < 0.15 and free:
            s = c.free_slot()
            assert s == min(free)  # the lowest free slot
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
        assert c.live_slots() == [s for s in range(n) if model[s]]
        assert c.get_offset(0) == max((m.off for m in model if m), default=0)
        assert (c.free_slot() is None) == all(model)
    assert wraps >= 2  # rings went round
    with pytest.raises(AssertionError, match="advance"):
        c.advance(L, ring_frames * L, device=False)


def test_open_and_close_write_the_device_row():
    c = _cache(3, cfg=False)
    assert all(kb.shape[0] == 3 for kb, _ in c.bufs)
    c.open_slot(0, 8)
    c.open_slot(1, 4)
    assert c.device_state() == [(0, 8, 8, 1), (0, 4, 4, 1), (0, 0, 0, 0)] == c.host_state()
    c.close_slot(0)
    assert c.device_state() == [(0, 0, 0, 0), (0, 4, 4, 1), (0, 0, 0, 0)] and c.free_slot() == 0
    with pytest.raises(AssertionError, match="idle"):
        c.close_slot(0)
    with pytest.raises(AssertionError, match="live"):
        c.open_slot(1, 4)
    v = c.slot_view(1)  # the slot's batch rows, nothing allocated
    assert v.bufs[0][0].data_ptr() == c.bufs[0][0][1].data_ptr() and v.bufs[0][0].shape == (1, 20, 8)
    with pytest.raises(RuntimeError, match="advance"):
        c.commit_device(0, 4)


def _core(**kw):
    cfg = dict(n_frames=8, d_model=128, n_heads=2, n_layers=2, tokens_per_frame=64, backbone="dit",
               rope_impl="motion")
    cfg.update(kw)
    return SimpleNamespace(config=SimpleNamespace(**cfg), parameters=lambda: iter([torch.zeros(1)]),
                           transformer=SimpleNamespace(rope=None))


def test_constructor_checks():
    from owl_wms.sampling.stream_pool import StreamPool
    p = StreamPool(_core(), 3, max_cached_frames=4, graphed="frame")
    assert (p.n_slots, p.ring_frames, p.graphed, p.live, p.graph_replays, p.ticks) == (3, 5, "frame", [], 0, 0)
    assert p.frames_generated == [0, 0, 0] and p.rebases == [0, 0, 0]
    assert p.kv_cache.bufs[0][0].shape == (6, 5 * 64, 128) and p.kv_cache.dev.shape == (3, 4)
    assert StreamPool(_core(), 2, cfg_scale=1.0, max_cached_frames=4).kv_cache.bufs[0][0].shape[0] == 2
    assert StreamPool(_core(), 1, max_cached_frames=4, ring_frames=9).ring_frames == 9
    for bad in (0, -1, 1.5, None, True):
        with pytest.raises(ValueError, match="n_slots"):
            StreamPool(_core(), bad, max_cached_frames=4)
    for bad in ("bogus", 2, None):
        with pytest.raises(ValueError, match="graphed"):
            StreamPool(_core(), 2, max_cached_frames=4, graphed=bad)
    with pytest.raises(ValueError, match="at least 1"):
        StreamPool(_core(), 2, max_cached_frames=0)
    with pytest.raises(ValueError, match="n_frames"):
        StreamPool(_core(), 2, max_cached_frames=7)
    with pytest.raises(ValueError, match="ring_frames"):
        StreamPool(_core(), 2, max_cached_frames=4, ring_frames=4)
    with pytest.raises(ValueError, match="backbone 'mmdit'"):
        StreamPool(_core(backbone="mmdit"), 2, max_cached_frames=4)
    with pytest.raises(ValueError, match="head_dim 32"):
        StreamPool(_core(d_model=64), 2, max_cached_frames=4)
    with pytest.raises(ValueError, match="65 tokens per frame"):
        StreamPool(_core(tokens_per_frame=65), 2, max_cached_frames=4)
    with pytest.raises(RuntimeError, match="open"):
        p.start(None, None, None)
    with pytest.raises(ValueError, match="not live"):
        p.close_slot(0)
    assert p.step({}) == {}
    with pytest.raises(ValueError, match="live slots"):
        p.step({0: (None, None)})
    p.close()


def test_slot_entries_header_binding_and_library_agree():
    from owl_wms._lib import LIB_PATH, _SIGS, exported_symbols
    kind = {ctypes.c_void_p: "P", ctypes.c_long: "L", ctypes.c_int: "I", ctypes.c_float: "F"}
    protos = _header_protos()
    hdr = open(os.path.join(REPO, "include", "owlk.h")).read()
    assert os.path.exists(LIB_PATH), "libowlk.so not built (run __graft_entry__.build())"
    h = ctypes.CDLL(LIB_PATH)
    for name, single in ENTRIES.items():
        assert name in protos and name in _SIGS and name in exported_symbols(), name
        assert [kind[a] for a in _SIGS[name]] == protos[name], name
        # the single-state entry's arguments with n_slots (a long) right after state (the first long* argument)
        i = {"owlk_ring_advance": 1, "owlk_qk_rope_fwd_kv_ring": 11, "owlk_attn_decode_ring_fwd": 20}[single]
        assert protos[single][i - 1] == "P" and protos[name] == protos[single][:i] + ["L"] + protos[single][i:], name
        args = re.search(r"int\s+" + name + r"\s*\(([^)]*)\)", hdr).group(1)
        assert re.search(r"\*\s*state,\s*long n_slots\b", args), name
        comment = hdr[:hdr.index("int " + name)].rsplit("/*", 1)[1]
        assert re.search(r"causvid_pipeline\.py:112-163", comment), name  # the reference lines it stands for
        assert hasattr(h, name), name
    assert "attn.py:83-107" in hdr
    text = open(os.path.join(REPO, "INTEGRATION.md")).read()
    assert all(name in text for name in ENTRIES)


def test_ring_advance_slots_refuses_on_the_host():
    """Every host-side refusal returns 1 and launches nothing (no GPU needed)."""
    from owl_wms._lib import lib
    h = lib()
    a = 4096  # a non-null address; a refused call launches nothing
    for state, n, L, max_rows, cap in ((None, 2, 64, 256, 320), (a, 0, 64, 256, 320), (a, -3, 64, 256, 320),
                                       (a, 2, 0, 256, 320), (a, 2, 64, 0, 320), (a, 2, 64, 257, 320),
                                       (a, 2, 400, 1, 320), (a, 2, 64, 256, 0)):
        assert h.owlk_ring_advance_slots(state, n, L, max_rows, cap, None) == 1, (state, n, L, max_rows, cap)
