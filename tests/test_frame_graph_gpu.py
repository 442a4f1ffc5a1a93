"""GPU tests of the whole-frame graph mode of the ring streams (owl_wms/sampling/stream.py
``graphed="frame"``): owlk_ring_advance against the host rule it replaces, and the three existing stream
classes in frame mode against their eager and step-graph modes on the tiny models and runs of
tests/test_stream_gpu.py, tests/test_av_stream_gpu.py and tests/test_av_dit_stream_gpu.py.

Bounds.  Everything here is torch.equal or integer equality: the frame graph launches the eager frame's
kernels on the same values in the same order (the noise is drawn outside the graph in the eager order), and
the advance rule is integer arithmetic."""
import pytest
import torch

import test_av_dit_stream_gpu as DIT
import test_av_stream_gpu as MM
import test_stream_gpu as VID

pytestmark = pytest.mark.gpu

DEV = "cuda"


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def K():
    from owl_wms import kernels
    return kernels


def dev_state(*v):
    return torch.tensor(list(v) + [0] * (4 - len(v)), dtype=torch.int64, device=DEV)


def host_rule(s, n, o, L, max_rows, cap):
    n, o = n + L, o + L
    if n > max_rows:
        s, n = (s + L) % cap, n - L
    return s, n, o


@pytest.mark.parametrize("L", [1, 64, 65])
def test_ring_advance_follows_the_host_rule(L):
    """40 launches from 3 cached frames on a 7-frame ring that keeps 6 (it wraps five times), the state
    read back after each; the fourth word stays 0."""
    k = K()
    cap, max_rows = 7 * L, 6 * L
    want = (0, 3 * L, 3 * L)
    st = dev_state(*want)
    for i in range(40):
        k.ring_advance(st, L, max_rows, cap)
        want = host_rule(*want, L, max_rows, cap)
        assert st.tolist() == [*want, 0], i
    assert want == ((37 * L) % cap, max_rows, 43 * L)
    # a ring that starts at its last row, and the largest window the host check lets through
    st = dev_state(cap - 1, max_rows, 100)
    k.ring_advance(st, L, max_rows, cap)
    assert st.tolist() == [(cap - 1 + L) % cap, max_rows, 100 + L, 0]
    with pytest.raises(RuntimeError, match="ring_advance"):
        k.ring_advance(st, L, max_rows + 1, cap)


@pytest.mark.parametrize("L", [1, 65])
def test_ring_advance_does_not_follow_a_state_outside_the_contract(L):
    """cached + L > cap, start >= cap, cached < 0 (and start < 0, offset < 0): cached becomes -1, start and
    offset stay; the guard path writes one word and reads three."""
    k = K()
    cap, max_rows = 5 * L, 4 * L
    for bad in ((0, cap - L + 1, 7), (cap, L, 7), (2, -1, 7), (-1, L, 7), (0, L, -1), (cap + 3, cap, 9)):
        st = dev_state(*bad)
        k.ring_advance(st, L, max_rows, cap)
        assert st.tolist() == [bad[0], -1, bad[2], 0], bad
        k.ring_advance(st, L, max_rows, cap)  # and it stays poisoned
        assert st.tolist() == [bad[0], -1, bad[2], 0], bad
    st = dev_state(cap - 1, cap - L, 7)  # the last state inside the contract is followed
    k.ring_advance(st, L, max_rows, cap)
    assert st.tolist() == [(cap - 1 + L) % cap, cap - L, 7 + L, 0]


def _mirror(s):
    c = s.kv_cache
    assert len({(c.start[i], c.len[i], c.offsets[i]) for i in range(c.config.n_layers)}) == 1
    return c.start[0], len(c), c.get_offset(0)


@pytest.mark.parametrize("cfg_scale", [1.3, 1.0])
@pytest.mark.parametrize("d_model", [128, 256])
def test_frame_stream_frame_graph_equals_step_graph_equals_eager(d_model, cfg_scale):
    """tests/test_stream_gpu.py's run (3 context frames, max_cached_frames 6, 14 frames, 4 steps; head_dim 64
    and 128): the three modes bit for bit; the device state equals the mirror after 11 evictions on the 7-frame
    ring; the buffers keep their addresses; 13 replays (frame 0 runs eagerly, frame 1 captures)."""
    m = VID._model(d_model, 32)
    x, mouse, btn = VID._inputs(2, 3, 17)
    kw = dict(n_steps=4, cfg_scale=cfg_scale, noise_prev=0.2, max_cached_frames=6)
    eager, s_e, *_ = VID._stream(m.core, x, mouse, btn, 14, graphed=False, **kw)
    step, s_s, *_ = VID._stream(m.core, x, mouse, btn, 14, graphed=True, **kw)
    out, s, ptrs0, ptrs1, rows = VID._stream(m.core, x, mouse, btn, 14, graphed="frame", **kw)
    assert out.shape == (2, 14, 32, 8, 8) and torch.isfinite(out.float()).all()
    assert torch.equal(out, eager) and torch.equal(step, eager)
    assert s.frames_generated == 14 and s.rebases == 0
    assert s.graph_replays == 13 and s_s.graph_replays == 14 * 4 - 1 and s_e.graph_replays == 0
    want = ((11 * 64) % (7 * 64), 6 * 64, 17 * 64)
    assert s.kv_cache.device_state() == _mirror(s) == _mirror(s_e) == want
    assert ptrs0 == ptrs1 and all(r == (7 * 64, 7 * 64) for r in rows)
    assert not m.core.transformer.decoding


def test_frame_graph_past_the_rope_table():
    """n_frames 8, max_cached_frames 4, 12 frames: the rebases run between replays on host positions and
    resynchronise the device vector; frame mode == eager bit for bit with the same rebases."""
    m = VID._model(128, 8)
    x, mouse, btn = VID._inputs(2, 3, 15)
    kw = dict(n_steps=4, cfg_scale=1.3, noise_prev=0.2, max_cached_frames=4)
    eager, s_e, *_ = VID._stream(m.core, x, mouse, btn, 12, **kw)
    out, s, ptrs0, ptrs1, _ = VID._stream(m.core, x, mouse, btn, 12, graphed="frame", **kw)
    assert s_e.rebases >= 2 and s.rebases == s_e.rebases and s.graph_replays == 11
    assert torch.isfinite(out.float()).all() and torch.equal(out, eager)
    assert s.kv_cache.device_state() == _mirror(s) == _mirror(s_e)
    assert ptrs0 == ptrs1


def _av_runs(T, model, runs):
    """frame mode == eager, video and audio, and the device state == the mirror, for each (model args, stream
    keywords) of `runs` on test module T's helpers"""
    for margs, kw, rebases in runs:
        m = model(*margs)
        ins = T._inputs(2, 3, 15)
        v, a, s_e, *_ = T._stream(m.core, ins, 12, **kw)
        vf, af, s, ptrs0, ptrs1, _ = T._stream(m.core, ins, 12, graphed="frame", **kw)
        assert torch.isfinite(vf.float()).all() and torch.isfinite(af.float()).all()
        assert torch.equal(vf, v) and torch.equal(af, a), (margs, kw)
        assert s.frames_generated == 12 and s.graph_replays == 11
        assert (s.rebases >= 2) == rebases and s.rebases == s_e.rebases
        assert s.kv_cache.device_state() == _mirror(s) == _mirror(s_e), (margs, kw)
        assert ptrs0 == ptrs1
        assert not m.core.transformer.decoding


KW_AV = dict(n_steps=3, cfg_scale=1.3, noise_prev=0.2, max_cached_frames=4)


def test_av_frame_stream_frame_graph_equals_eager():
    """tests/test_av_stream_gpu.py's wrapping-ring run (default ring and ring_frames 16) and its past-the-table
    run, 65-row joint frames on the MMDiT."""
    _av_runs(MM, MM._model, (((32,), KW_AV, False), ((32,), dict(KW_AV, ring_frames=16), False),
                             ((8,), KW_AV, True)))


@pytest.mark.parametrize("rope_impl", ["motion", "ortho"])
def test_av_dit_frame_stream_frame_graph_equals_eager(rope_impl):
    """tests/test_av_dit_stream_gpu.py's wrapping-ring run and its past-the-table run, 65-row frames on the
    wide ring decode, MotionRoPE and OrthoRoPE (which this stream rebases too)."""
    _av_runs(DIT, DIT._model, (((32, rope_impl), KW_AV, False), ((8, rope_impl), KW_AV, True)))


def test_samplers_with_frame_graph_equal_the_eager_call():
    from owl_wms.sampling import get_sampler_cls
    m = VID._model(128, 8)
    x, mouse, btn = VID._inputs(2, 3, 13)
    outs = []
    for fg, graph in ((False, False), (True, True), (True, False)):
        torch.manual_seed(321)
        smp = get_sampler_cls("av_stream")(n_steps=2, cfg_scale=1.3, num_frames=10, noise_prev=0.2, max_window=2,
                                           frame_graph=fg)
        outs.append(smp(m.core, x, mouse, btn, compile_on_decode=graph))
    assert outs[0].shape == (2, 13, 32, 8, 8) and torch.isfinite(outs[0].float()).all()
    assert torch.equal(outs[1], outs[0]) and torch.equal(outs[2], outs[0])
    for T in (MM, DIT):
        core = T._model(8).core
        xv, audio, mouse, btn = T._inputs(2, 3, 10)
        outs = []
        for fg, graph in ((False, False), (True, True)):
            torch.manual_seed(321)
            smp = get_sampler_cls("av_audio_stream")(n_steps=2, cfg_scale=1.3, num_frames=7, noise_prev=0.2,
                                                     max_cached_frames=4, frame_graph=fg)
            outs.append(smp(core, xv, audio, mouse, btn, compile_on_decode=graph))
        assert torch.equal(outs[1][0], outs[0][0]) and torch.equal(outs[1][1], outs[0][1])
        assert torch.isfinite(outs[0][0].float()).all() and torch.isfinite(outs[0][1].float()).all()


def test_close_reports_a_device_state_that_left_the_mirror():
    """close() in frame mode reads the device vector back: a position that differs from the mirror (here set by
    hand after the last frame, to a count the kernels would not follow) raises, naming both."""
    from owl_wms.sampling.stream import FrameStream
    m = VID._model(128, 32)
    x, mouse, btn = VID._inputs(1, 3, 6)
    torch.manual_seed(321)
    s = FrameStream(m.core, n_steps=1, cfg_scale=1.0, max_cached_frames=6, graphed="frame")
    s.start(x, mouse, btn)
    for i in range(3):
        s.step(mouse[:, 3 + i:4 + i], btn[:, 3 + i:4 + i])
    assert s.kv_cache.device_state() == (0, 6 * 64, 6 * 64)
    s.kv_cache.dev[1] = -1
    with pytest.raises(RuntimeError, match=r"\(0, -1, 384\).*\(0, 384, 384\)"):
        s.close()
    s.kv_cache.sync_device_state()
    s.close()
