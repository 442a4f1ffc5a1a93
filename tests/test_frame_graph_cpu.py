"""Host-side tests of the whole-frame graph mode and of audio streaming (no GPU): RingKVCache.advance
against the host sequence it replaces, renoise against zlerp, the ``graphed`` modes the four stream classes
accept, AudioStream's refusals, the sampler registry, and the header / binding / library agreement and
host refusals of owlk_ring_advance."""
import ctypes
import os
import re
from types import SimpleNamespace

import pytest
import torch

from conftest import REPO
from test_stream_cpu import _header_protos

ENTRY = "owlk_ring_advance"


def _cache(L, ring_frames, n_layers=2):
    from owl_wms.nn.kv_cache import RingKVCache
    cfg = SimpleNamespace(n_layers=n_layers, tokens_per_frame=L, n_heads=1, d_model=8, backbone="dit")
    c = RingKVCache(cfg, ring_frames * L)
    c.reset(1)
    z = torch.zeros(1, L, 8)  # one context frame, from row 0
    for i in range(n_layers):
        c.update(z, z, i)
    return c


@pytest.mark.parametrize("L,ring_frames,max_frames", [(1, 5, 4), (64, 7, 6), (65, 5, 4), (65, 16, 4)])
def test_advance_is_commit_then_truncate(L, ring_frames, max_frames):
    """60 frames: advance(device=False) against commit_device on every layer, then truncate(1) when over --
    start, len and offsets equal after every frame, wraps included."""
    new, old = _cache(L, ring_frames), _cache(L, ring_frames)
    wraps = 0
    for f in range(60):
        new.advance(L, max_frames * L, device=False)
        for i in range(old.config.n_layers):
            old.commit_device(i, L)
        if old.n_frames() > max_frames:
            s0 = old.start[0]
            old.truncate(1, front=False)
            wraps += old.start[0] < s0
        assert (new.start, new.len, new.offsets) == (old.start, old.len, old.offsets), f
        assert new.n_frames() <= max_frames and 0 <= new.start[0] < ring_frames * L
    assert new.n_frames() == max_frames and new.get_offset(0) == 61 * L
    assert wraps >= 2  # the ring went round
    with pytest.raises(AssertionError, match="advance"):
        new.advance(L, ring_frames * L, device=False)  # max_rows + L must fit the ring
    with pytest.raises(AssertionError, match="advance"):
        new.advance(0, max_frames * L, device=False)


def test_renoise_is_zlerp_with_the_noise_in_hand():
    from owl_wms.sampling.schedulers import renoise, zlerp
    x = torch.randn(2, 3, 5, generator=torch.Generator().manual_seed(1)).bfloat16()
    torch.manual_seed(5)
    want = zlerp(x, 0.2)
    torch.manual_seed(5)
    z = torch.randn_like(x)
    assert torch.equal(renoise(x, z, 0.2), want)
    assert torch.equal(renoise(x, z, 0.2), x * (1.0 - 0.2) + z * 0.2)


def _core(**kw):
    cfg = dict(n_frames=8, d_model=128, n_heads=2, tokens_per_frame=64, backbone="dit", rope_impl="motion")
    cfg.update(kw)
    return SimpleNamespace(config=SimpleNamespace(**cfg))


def _stream_classes():
    from owl_wms.sampling.stream import AVDiTFrameStream, AVFrameStream, AudioStream, FrameStream
    return ((FrameStream, _core()), (AVFrameStream, _core(backbone="mmdit", tokens_per_frame=65)),
            (AVDiTFrameStream, _core(tokens_per_frame=65)), (AudioStream, _core(tokens_per_frame=1)))


def test_graphed_modes():
    for cls, core in _stream_classes():
        for bad in ("bogus", "step", 2, None):
            with pytest.raises(ValueError, match="graphed"):
                cls(core, max_cached_frames=4, graphed=bad)
        for mode in (False, True, "frame"):
            s = cls(core, max_cached_frames=4, graphed=mode)
            assert s.graphed == mode and s.graph_replays == 0 and s.ring_frames == 5
        assert cls(core, max_cached_frames=4, ring_frames=9).ring_frames == 9  # every class takes ring_frames
        with pytest.raises(ValueError, match="ring_frames"):
            cls(core, max_cached_frames=4, ring_frames=4)


def test_samplers_select_the_frame_graph():
    from owl_wms.sampling import get_sampler_cls
    from owl_wms.sampling.stream import AVStreamSampler, AudioStreamSampler, StreamSampler, graph_mode
    assert get_sampler_cls("audio_stream") is AudioStreamSampler
    for cls in (StreamSampler, AVStreamSampler, AudioStreamSampler):
        assert cls().frame_graph is False and cls(frame_graph=True).frame_graph is True
    assert graph_mode(False, False) is False and graph_mode(True, False) is True
    assert graph_mode(True, True) == "frame" and graph_mode(False, True) is False
    s = AudioStreamSampler(n_steps=2, num_tokens=3, noise_prev=0.2, custom_schedule=None, max_window=2)
    assert (s.n_steps, s.num_tokens, s.max_window) == (2, 3, 2)


def test_audio_stream_refusals():
    from owl_wms.sampling.stream import AudioStream
    ok = _core(tokens_per_frame=1, rope_impl="audio1d")
    assert AudioStream(ok, max_cached_frames=4).cfg_scale == 1.0 and AudioStream.decoding
    assert AudioStream(ok, max_cached_frames=4)._controls(None, None) == {}
    assert AudioStream(_core(tokens_per_frame=1, d_model=256), max_cached_frames=4)  # head_dim 128
    with pytest.raises(ValueError, match="backbone 'mmdit'"):
        AudioStream(_core(tokens_per_frame=1, backbone="mmdit"), max_cached_frames=4)
    with pytest.raises(ValueError, match="64 tokens per frame"):
        AudioStream(_core(), max_cached_frames=4)
    with pytest.raises(ValueError, match="head_dim 32"):
        AudioStream(_core(tokens_per_frame=1, d_model=64), max_cached_frames=4)
    with pytest.raises(ValueError, match="at least 1"):
        AudioStream(ok, max_cached_frames=0)
    with pytest.raises(ValueError, match="n_frames"):
        AudioStream(ok, max_cached_frames=7)
    with pytest.raises(RuntimeError, match="before start"):
        AudioStream(ok, max_cached_frames=4).step()


def test_ring_advance_header_binding_and_library_agree():
    from owl_wms._lib import LIB_PATH, _SIGS, exported_symbols
    kind = {ctypes.c_void_p: "P", ctypes.c_long: "L", ctypes.c_int: "I", ctypes.c_float: "F"}
    protos = _header_protos()
    assert ENTRY in protos and ENTRY in _SIGS and ENTRY in exported_symbols()
    assert [kind[a] for a in _SIGS[ENTRY]] == protos[ENTRY] == ["P", "L", "L", "L", "P"]
    hdr = open(os.path.join(REPO, "include", "owlk.h")).read()
    comment = hdr[:hdr.index("int " + ENTRY)].rsplit("/*", 1)[1]
    assert re.search(r"causvid_pipeline\.py:\d+", comment)  # the reference lines it serves, like its neighbours
    assert os.path.exists(LIB_PATH), "libowlk.so not built (run __graft_entry__.build())"
    assert hasattr(ctypes.CDLL(LIB_PATH), ENTRY)


def test_ring_advance_refuses_on_the_host():
    """Every host-side refusal returns 1 and launches nothing (no GPU needed)."""
    from owl_wms._lib import lib
    h = lib()
    a = 4096  # a non-null address; a refused call launches nothing
    for state, L, max_rows, cap in ((None, 64, 256, 320), (a, 0, 256, 320), (a, -64, 256, 320), (a, 64, 0, 320),
                                    (a, 64, -1, 320), (a, 64, 257, 320), (a, 64, 320, 320), (a, 400, 1, 320),
                                    (a, 64, 256, 0)):
        assert h.owlk_ring_advance(state, L, max_rows, cap, None) == 1, (state, L, max_rows, cap)
