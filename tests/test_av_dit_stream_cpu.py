"""Host-side tests of audio + video streaming on the DiT backbone (no GPU): the header / binding / library
agreement and the host refusals of the wide ring decode entry, the shapes the attention module sends it,
every refusal of AVDiTFrameStream against a SimpleNamespace config, the sampler registry, and the linearity
of OrthoRoPE in the frame index that its rebase rests on."""
import ctypes
import os
import re
from types import SimpleNamespace

import pytest
import torch

from conftest import REPO
from test_stream_cpu import _header_protos

ENTRY = "owlk_attn_decode_wide_ring_fwd"


def test_wide_ring_entry_header_binding_and_library_agree():
    from owl_wms._lib import LIB_PATH, _SIGS, exported_symbols
    kind = {ctypes.c_void_p: "P", ctypes.c_long: "L", ctypes.c_int: "I", ctypes.c_float: "F"}
    protos = _header_protos()
    assert ENTRY in protos and ENTRY in _SIGS and ENTRY in exported_symbols()
    assert [kind[a] for a in _SIGS[ENTRY]] == protos[ENTRY]
    assert protos[ENTRY] == protos["owlk_attn_decode_ring_fwd"]  # the 64-row ring entry's argument list
    hdr = open(os.path.join(REPO, "include", "owlk.h")).read()
    comment = hdr[:hdr.index("int " + ENTRY)].rsplit("/*", 1)[1]
    assert re.search(r"attn\.py:86-107", comment) and "causvid_pipeline.py" in comment  # the lines it serves
    assert os.path.exists(LIB_PATH), "libowlk.so not built (run __graft_entry__.build())"
    assert hasattr(ctypes.CDLL(LIB_PATH), ENTRY)


def test_wide_ring_entry_refuses_on_the_host():
    """Every host-side refusal returns 1 and launches nothing (no GPU needed)."""
    from owl_wms._lib import lib
    h = lib()
    a = 4096  # an aligned non-null address; a refused call launches nothing
    args = dict(q=a, ldq=128, sqb=65 * 128, kbuf=a, ldk=128, skb=390 * 128, vbuf=a, ldv=128, svb=390 * 128, o=a,
                ldo=128, sob=65 * 128, lse=None, B=1, H=2, Lq=65, D=64, scale=0.125, bound=64.5, state=a, Lnew=65,
                window=0, cap=390, stream=None)
    assert len(args) == 24
    call = lambda **kw: h.owlk_attn_decode_wide_ring_fwd(*{**args, **kw}.values())
    bad_args = (dict(D=128), dict(D=96), dict(Lq=81), dict(Lq=0), dict(Lq=-1), dict(Lnew=0), dict(Lnew=-65),
                dict(cap=64), dict(state=None), dict(bound=0.0), dict(bound=-1.0), dict(bound=320.0),
                dict(q=a + 8), dict(kbuf=a + 8), dict(vbuf=a + 8), dict(o=a + 8), dict(ldq=132), dict(ldk=132),
                dict(ldv=132), dict(ldo=132), dict(ldq=64), dict(ldk=64), dict(ldv=64), dict(ldo=64),
                dict(window=-1))
    for bad in bad_args:
        assert call(**bad) == 1, bad
    assert 320.0 * 0.125 >= 40.0  # score_bound * scale at the refused bound


def test_decode_wide_supported():
    from owl_wms import kernels as K
    assert K.WIDE_DECODE_ROWS == 80
    assert K.decode_wide_supported(64, 65) and K.decode_wide_supported(64, 80)
    for D, L in ((64, 64), (64, 81), (128, 65)):
        assert not K.decode_wide_supported(D, L), (D, L)
    # the 64-row contract of the existing pair is as it was
    assert K.decode_dev_supported(64, 64) and K.decode_dev_supported(128, 64)
    assert not K.decode_dev_supported(64, 65) and not K.decode_dev_supported(64, 0)


def _core(**kw):
    cfg = dict(n_frames=8, d_model=128, n_heads=2, tokens_per_frame=65, backbone="dit", rope_impl="ortho")
    cfg.update(kw)
    return SimpleNamespace(config=SimpleNamespace(**cfg))


def test_av_dit_frame_stream_refusals():
    from owl_wms.sampling.stream import AVDiTFrameStream, AVFrameStream, _RingStream
    with pytest.raises(ValueError, match="backbone 'mmdit'"):
        AVDiTFrameStream(_core(backbone="mmdit"), max_cached_frames=4)
    with pytest.raises(ValueError, match="head_dim 128"):
        AVDiTFrameStream(_core(d_model=256), max_cached_frames=4)
    with pytest.raises(ValueError, match="81 tokens per frame"):
        AVDiTFrameStream(_core(tokens_per_frame=81), max_cached_frames=4)
    with pytest.raises(ValueError, match="at least 1"):
        AVDiTFrameStream(_core(), max_cached_frames=0)
    with pytest.raises(ValueError, match="n_frames"):
        AVDiTFrameStream(_core(), max_cached_frames=7)
    assert AVDiTFrameStream(_core(), max_cached_frames=6).ring_frames == 7  # 7 of the table's 8 frames: the limit
    with pytest.raises(ValueError, match="AVDiTFrameStream: ring_frames"):
        AVDiTFrameStream(_core(), max_cached_frames=4, ring_frames=4)
    ok = AVDiTFrameStream(_core(), max_cached_frames=4, ring_frames=5)
    assert ok.ring_frames == 5 and AVDiTFrameStream(_core(), max_cached_frames=4).ring_frames == 5
    assert AVDiTFrameStream(_core(tokens_per_frame=80), max_cached_frames=4).decoding
    with pytest.raises(RuntimeError, match="before start"):
        ok.step(None, None)
    with pytest.raises(ValueError, match="context frames"):
        ok.start(torch.zeros(1, 5, 4, 8, 8), torch.zeros(1, 5, 3), torch.zeros(1, 5, 2), torch.zeros(1, 5, 11))
    with pytest.raises(ValueError, match="context frames"):
        ok.start(torch.zeros(1, 0, 4, 8, 8), torch.zeros(1, 0, 3), torch.zeros(1, 0, 2), torch.zeros(1, 0, 11))
    # one base over _RingStream; the two classes differ in the core they accept (and what follows from it)
    base = AVDiTFrameStream.__mro__[1]
    assert base is AVFrameStream.__mro__[1] and issubclass(base, _RingStream) and base is not _RingStream
    for name in ("__init__", "_forward", "_guided", "start", "step"):
        assert name not in vars(AVDiTFrameStream) and name not in vars(AVFrameStream), name


def test_sampler_registry_still_serves_av_audio_stream():
    from owl_wms.sampling import AV_CORE_SAMPLERS, get_sampler_cls
    from owl_wms.sampling.stream import AVDiTFrameStream, AVFrameStream, AVStreamSampler, av_stream_cls
    assert get_sampler_cls("av_audio_stream") is AVStreamSampler and "av_audio_stream" in AV_CORE_SAMPLERS
    assert av_stream_cls("dit") is AVDiTFrameStream and av_stream_cls("mmdit") is AVFrameStream


class _Reached(Exception):
    pass


class _CacheAtTheTableEnd:
    """a cache whose next frame would pass an 8-frame table: 4 live frames, the newest at frame 7"""

    def __init__(self):
        self.rebased = []

    def get_offset(self, i=0):
        return 8 * 65

    def __len__(self):
        return 4 * 65

    def rebase(self, shift, rope):
        self.rebased.append((shift, rope))
        raise _Reached


def test_ortho_rebase_is_the_dit_streams_alone():
    """At the end of an ortho table AVDiTFrameStream.step reaches cache.rebase (oldest live key to position
    0); AVFrameStream raises there as before, and the module-level tuple is as it was."""
    from owl_wms.sampling.stream import REBASE_ROPES, AVDiTFrameStream, AVFrameStream
    assert REBASE_ROPES == ("motion", "audio1d")
    assert AVFrameStream.rebase_ropes == REBASE_ROPES
    assert set(AVDiTFrameStream.rebase_ropes) == set(REBASE_ROPES) | {"ortho"}
    rope = SimpleNamespace(cos=torch.zeros(8 * 65, 32))
    for impl in AVDiTFrameStream.rebase_ropes:
        core = _core(rope_impl=impl)
        core.transformer = SimpleNamespace(rope=rope)
        s = AVDiTFrameStream(core, max_cached_frames=4)
        s.kv_cache = _CacheAtTheTableEnd()
        with pytest.raises(_Reached):
            s.step(None, None)
        assert s.kv_cache.rebased == [(4 * 65, rope)], impl
    core = _core(backbone="mmdit")
    core.transformer = SimpleNamespace(rope=rope)
    s = AVFrameStream(core, max_cached_frames=4)
    s.kv_cache = _CacheAtTheTableEnd()
    with pytest.raises(RuntimeError, match="cannot be rebased") as e:
        s.step(None, None)
    assert s.kv_cache.rebased == [] and "ortho" in str(e.value)


@pytest.mark.parametrize("head_dim", [64, 128])
def test_ortho_rope_audio_slot_is_linear_in_the_frame_index(head_dim):
    """OrthoRoPE with the audio slot (65 tokens per frame): only the time axis moves with the frame, angle
    a_r + f * delta.  In fp64 an s-frame angle shift is constant over frames and all 65 tokens within
    2^-22 max|angle| (test_motion_rope_audio_slot_is_linear_in_the_frame_index's assertion and bound: each
    fp32 product rounds once, 2^-24 relative; two roundings per difference, two differences compared).  No
    prefix assertion: the time axis is a linspace over n_frames, so a short table is no prefix of a long one,
    and owlk_rope_rebase, which forms its rotation from two rows of the table in hand, does not need one."""
    from owl_wms.configs import model_config
    from owl_wms.nn.rope import get_rope_cls
    kw = dict(model_id="game_rft_audio", sample_size=8, channels=32, audio_channels=16, n_layers=2, n_heads=2,
              d_model=2 * head_dim, tokens_per_frame=65, n_buttons=11, causal=True, backbone="dit", has_audio=True,
              rope_impl="ortho", local_window=2, global_window=4)
    for nf in (8, 16, 32):
        cfg = model_config(**dict(kw, n_frames=nf))
        rope = get_rope_cls("ortho")(cfg)
        ang = rope.get_freqs(cfg)
        assert rope.cos.shape == (nf * 65, head_dim // 2) and ang.shape == rope.cos.shape
        a = ang.view(nf, 65, -1).double()  # [frames, 65, D/2]
        bound = 2.0 ** -22 * a.abs().max().item()
        for s in (1, 3, 5):
            d = a[s:] - a[:-s]
            spread = (d.amax(0) - d.amin(0)).max().item()  # over frames, per (token, pair)
            tok_spread = (d.amax((0, 1)) - d.amin((0, 1))).max().item()  # over frames and all 65 tokens
            print(f"ortho head_dim {head_dim} n_frames {nf} shift {s}: spread {spread:.2e} over tokens "
                  f"{tok_spread:.2e} bound {bound:.2e}")
            assert spread <= bound and tok_spread <= bound, (nf, s, spread, tok_spread, bound)
            assert d.abs().max().item() > 0.0  # the time axis does move
