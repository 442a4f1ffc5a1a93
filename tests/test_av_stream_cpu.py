"""Host-side tests of endless audio + video streaming (no GPU): the header / binding / library agreement
of the two ring joint-frame entries, the sampler registry, every refusal of AVFrameStream against a
SimpleNamespace config, and the MotionRoPE audio slot's linearity that the rebase rests on."""
import ctypes
import os
import re
from types import SimpleNamespace

import pytest
import torch

from conftest import REPO
from test_stream_cpu import _header_protos

NEW_ENTRIES = ("owlk_mm_qk_rope_fwd_kv_ring", "owlk_attn_decode_joint_ring_fwd")


def test_new_entries_header_binding_and_library_agree():
    from owl_wms._lib import LIB_PATH, _SIGS, exported_symbols
    kind = {ctypes.c_void_p: "P", ctypes.c_long: "L", ctypes.c_int: "I", ctypes.c_float: "F"}
    protos = _header_protos()
    hdr = open(os.path.join(REPO, "include", "owlk.h")).read()
    assert os.path.exists(LIB_PATH), "libowlk.so not built (run __graft_entry__.build())"
    h = ctypes.CDLL(LIB_PATH)
    for name in NEW_ENTRIES:
        assert name in protos and name in _SIGS and name in exported_symbols(), name
        assert [kind[a] for a in _SIGS[name]] == protos[name], name
        comment = hdr[:hdr.index("int " + name)].rsplit("/*", 1)[1]
        assert re.search(r"\w+\.py(:\d+)?", comment), name  # cites the reference lines it serves
        assert hasattr(h, name), name
    # the linear rope entry's arguments with tab_off -> state and the ring capacity added
    lin = protos["owlk_mm_qk_rope_fwd_kv"]
    assert protos["owlk_mm_qk_rope_fwd_kv_ring"] == lin[:14] + ["P"] + lin[15:24] + ["L", "P"]


def test_ring_entries_refuse_on_the_host():
    """The linear entries' host-side refusals (return 1, nothing launched; no GPU needed)."""
    from owl_wms._lib import lib
    h = lib()
    a = 4096  # an aligned non-null address; a refused call launches nothing
    rope_args = dict(qkv0=a, ld0=384, qkv1=a, ld1=384, B=1, nf=1, n0=64, n1=1, H=2, D=64, cos=a, sin=a, ld_tab=32,
                     n_tab=390, state=a, qo=a, ldqo=128, sqo=65 * 128, kbuf=a, ldk=128, skb=455 * 128, vbuf=a, ldv=128,
                     svb=455 * 128, cap=455, stream=None)
    attn_args = dict(q=a, ldq=128, sqb=65 * 128, kbuf=a, ldk=128, skb=455 * 128, vbuf=a, ldv=128, svb=455 * 128, o0=a,
                     ldo0=128, o1=a, ldo1=128, lse=None, B=1, H=2, n0=64, n1=1, D=64, scale=0.125, bound=64.5,
                     state=a, window=0, cap=455, stream=None)
    rope = lambda **kw: h.owlk_mm_qk_rope_fwd_kv_ring(*{**rope_args, **kw}.values())
    attn = lambda **kw: h.owlk_attn_decode_joint_ring_fwd(*{**attn_args, **kw}.values())
    for bad in (dict(D=96), dict(n0=0), dict(state=None), dict(cap=64), dict(n_tab=64), dict(ldk=64), dict(ld0=380),
                dict(kbuf=a + 8), dict(ldqo=132)):
        assert rope(**bad) == 1, bad
    for bad in (dict(D=128), dict(n0=80), dict(state=None), dict(cap=64), dict(bound=0.0), dict(q=a + 8),
                dict(ldk=132), dict(ldo1=64), dict(window=-1)):
        assert attn(**bad) == 1, bad


def _core(**kw):
    cfg = dict(n_frames=8, d_model=128, n_heads=2, tokens_per_frame=65, backbone="mmdit", rope_impl="motion")
    cfg.update(kw)
    return SimpleNamespace(config=SimpleNamespace(**cfg))


def test_sampler_registry_has_av_audio_stream():
    from owl_wms.sampling import AV_CORE_SAMPLERS, get_sampler_cls
    from owl_wms.sampling.stream import AVStreamSampler
    assert get_sampler_cls("av_audio_stream") is AVStreamSampler
    assert "av_audio_stream" in AV_CORE_SAMPLERS and "av_causal" in AV_CORE_SAMPLERS
    s = AVStreamSampler(n_steps=2, cfg_scale=1.0, num_frames=3, noise_prev=0.2, max_cached_frames=4)
    assert (s.n_steps, s.cfg_scale, s.num_frames, s.noise_prev, s.max_cached_frames) == (2, 1.0, 3, 0.2, 4)
    assert AVStreamSampler().max_cached_frames is None


def test_av_frame_stream_refusals():
    from owl_wms.sampling.stream import REBASE_ROPES, AVFrameStream
    with pytest.raises(ValueError, match="mmdit"):
        AVFrameStream(_core(backbone="dit"), max_cached_frames=4)
    with pytest.raises(ValueError, match="head_dim 128"):
        AVFrameStream(_core(d_model=256), max_cached_frames=4)
    with pytest.raises(ValueError, match="at least 1"):
        AVFrameStream(_core(), max_cached_frames=0)
    with pytest.raises(ValueError, match="n_frames"):
        AVFrameStream(_core(), max_cached_frames=7)
    assert AVFrameStream(_core(), max_cached_frames=6).ring_frames == 7  # 7 of the table's 8 frames: the limit
    with pytest.raises(ValueError, match="ring_frames"):
        AVFrameStream(_core(), max_cached_frames=4, ring_frames=4)
    ok = AVFrameStream(_core(), max_cached_frames=4, ring_frames=5)
    assert ok.ring_frames == 5 and AVFrameStream(_core(), max_cached_frames=4).ring_frames == 5
    with pytest.raises(RuntimeError, match="before start"):
        ok.step(None, None)
    with pytest.raises(ValueError, match="context frames"):
        ok.start(torch.zeros(1, 5, 4, 8, 8), torch.zeros(1, 5, 3), torch.zeros(1, 5, 2), torch.zeros(1, 5, 11))
    with pytest.raises(ValueError, match="context frames"):
        ok.start(torch.zeros(1, 0, 4, 8, 8), torch.zeros(1, 0, 3), torch.zeros(1, 0, 2), torch.zeros(1, 0, 11))
    # a rebase falling due on a table that is not linear in the frame index: refused, naming the ones that are
    core = _core(rope_impl="ortho")
    core.transformer = SimpleNamespace(rope=SimpleNamespace(cos=torch.zeros(8 * 65, 32)))
    s = AVFrameStream(core, max_cached_frames=4)
    s.kv_cache = SimpleNamespace(get_offset=lambda i=0: 8 * 65)
    with pytest.raises(RuntimeError) as e:
        s.step(None, None)
    assert all(r in str(e.value) for r in REBASE_ROPES) and "ortho" in str(e.value)


def test_motion_rope_audio_slot_is_linear_in_the_frame_index():
    """MotionRoPE with the audio slot (has_audio, 65 tokens per frame): the 8-frame table is a
    bit-identical prefix of the 32-frame one, and in fp64 an s-frame angle shift is constant over frames
    and all 65 tokens within 2^-22 max|angle| (test_rope_angles_are_linear_in_the_frame_index's idiom:
    each fp32 product rounds once, 2^-24 relative; two roundings per difference, two differences
    compared).  What the MMDiT stream's rebase rests on for the audio row."""
    from owl_wms.configs import model_config
    from owl_wms.nn.rope import get_rope_cls
    kw = dict(model_id="game_rft_audio", sample_size=8, channels=32, audio_channels=16, n_layers=2, n_heads=2,
              d_model=128, tokens_per_frame=65, n_buttons=11, n_frames=8, causal=True, backbone="mmdit",
              has_audio=True, rope_impl="motion", rope_ats_delta=2.0, local_window=2, global_window=4)
    tabs = {}
    for nf in (8, 32):
        cfg = model_config(**dict(kw, n_frames=nf))
        rope = get_rope_cls("motion")(cfg)
        ang = rope.get_freqs(cfg)
        ang = ang.view(nf, -1, ang.size(-1))
        assert ang.shape[1] == 65 and rope.cos.shape == (nf * 65, 32)
        tabs[nf] = (ang.double(), rope.cos, rope.sin)
    n8 = tabs[8][1].shape[0]
    assert torch.equal(tabs[8][1], tabs[32][1][:n8]) and torch.equal(tabs[8][2], tabs[32][2][:n8])
    for nf in (8, 32):
        a = tabs[nf][0]  # [frames, 65, D/2]
        bound = 2.0 ** -22 * a.abs().max().item()
        for s in (1, 3, 5):
            d = a[s:] - a[:-s]
            spread = (d.amax(0) - d.amin(0)).max().item()  # over frames, per (token, pair)
            tok_spread = (d.amax((0, 1)) - d.amin((0, 1))).max().item()  # over frames and all 65 tokens
            assert spread <= bound and tok_spread <= bound, (nf, s, spread, tok_spread, bound)
