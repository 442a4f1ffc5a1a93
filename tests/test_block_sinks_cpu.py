"""The DiT / MMDiT blocks' gradient sinks, on CPU with every launch stubbed out (no GPU, no library).

The backward writes dW / db straight into the parameters' GradReducer bucket views and tells the
reducer when a view is complete (fused.wgrad_into / bgrad_into, their `done`).  The reducer may start
a bucket's all-reduce on that word, so it must come once per parameter and, in the MMDiT block, only
after the audio side stream has been joined: a launch order no numerical test sees.
"""
import contextlib
from types import SimpleNamespace

import pytest
import torch

import conftest  # noqa: F401  (sys.path)


class _Lib:
    """libowlk's workspace-size queries: a positive multiple of 256 for every shape"""

    def __getattr__(self, name):
        assert name.endswith("_bytes"), f"only size queries are stubbed, not {name}"
        return lambda *args: 256


@pytest.fixture
def log(monkeypatch):
    """Everything the blocks do in order: entry names of the launches (nothing runs), 'fork' / 'join'
    of the MMDiT audio lane, ('ready', parameter) for each report to the reducer."""
    from owl_wms import kernels as K
    from owl_wms.nn import mmattn
    events = []

    class Lane:
        def __init__(self, device, enable):
            pass

        def fork(self):
            events.append("fork")

        def join(self):
            events.append("join")

        def on(self, s):
            return contextlib.nullcontext()

        def mark(self, ts):
            pass

    monkeypatch.setattr(K, "call", lambda name, *args, **kw: events.append(name))
    monkeypatch.setattr(K, "stream", lambda: None)
    monkeypatch.setattr(K, "lib", lambda: _Lib())
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: False)
    monkeypatch.setattr(mmattn, "_AudioLane", Lane)
    return events


def _reducer(module, events):
    """GradReducer over the module's parameters whose grad_ready is recorded"""
    from owl_wms.utils.grad_reducer import GradReducer
    params = list(module.parameters())
    assert len(params) == 16
    r = GradReducer(params, world_size=1)
    ready = r.grad_ready

    def record(p):
        events.append(("ready", p))
        ready(p)
    r.grad_ready = record  # fused.grad_done looks it up on the instance
    r.begin(True)
    return r


def _view_versions(module):
    return [p.grad._version for p in module.parameters()]


def _check_sinks(module, events, versions):
    """every parameter reported once; none of them handed a gradient by autograd, which would have
    added it onto the bucket view in place (the stubbed launches write nothing): versions are the
    views' version counters from before the backward"""
    params = list(module.parameters())
    reported = [e[1] for e in events if isinstance(e, tuple)]
    assert len(reported) == 16
    assert {id(p) for p in reported} == {id(p) for p in params}
    assert _view_versions(module) == versions
    for p in params:
        assert p.grad is not None and p.grad.data_ptr() == p._owl_grad_view.data_ptr()


@pytest.mark.parametrize("d,frames", [(128, 2), (256, 5)])  # the frame_mux layout, the in-place layout
def test_mmdit_reports_each_parameter_once_and_outside_the_lane(log, d, frames):
    from owl_wms import kernels as K
    from owl_wms.nn import mmattn
    assert mmattn._in_place_ok(d, 64, 1, frames) == (d == 256)
    cfg = SimpleNamespace(d_model=d, n_heads=2, sample_size=8, tokens_per_frame=65, n_frames=frames, has_audio=True)
    block = mmattn.MMDiTBlock(cfg, 0)
    _reducer(block, log)
    x0 = torch.zeros(1, frames * 64, d, requires_grad=True)
    x1 = torch.zeros(1, frames, d, requires_grad=True)
    c0, c1 = (torch.zeros(1, frames, 6 * d, dtype=torch.bfloat16, requires_grad=True) for _ in range(2))
    y0, y1 = block(x0, x1, c0, c1, K.FrameMask(65, 2, True, 0, None))
    del log[:]
    versions = _view_versions(block)
    torch.autograd.backward([y0, y1], [torch.zeros_like(y0), torch.zeros_like(y1)])

    assert log.count("fork") == 2 and log.count("join") == 2
    forked = False
    for e in log:
        if e in ("fork", "join"):
            assert forked == (e == "join"), "fork / join out of step"
            forked = e == "fork"
        elif isinstance(e, tuple):
            assert not forked, "a parameter was reported to the reducer before the audio lane was joined"
    _check_sinks(block, log, versions)


def _dit_backward(log, split_stack):
    from owl_wms import kernels as K
    from owl_wms.nn.attn import DiTBlock
    d = 128
    cfg = SimpleNamespace(d_model=d, n_heads=2, sample_size=8, tokens_per_frame=64, n_frames=2, has_audio=False,
                          local_window=2)
    block = DiTBlock(cfg, 0)
    _reducer(block, log)
    if split_stack:  # one modulation weight's view no longer adjacent to its neighbours': still a sink
        w = block.gate1.fc_c.weight
        w._owl_grad_view = torch.zeros_like(w)
        w.grad = w._owl_grad_view
    x = torch.zeros(1, 2 * 64, d, requires_grad=True)
    cond = torch.zeros(1, 2, d, requires_grad=True)
    y = block(x, cond, K.FrameMask(64, 2, True, 0, None))
    del log[:]
    versions = _view_versions(block)
    y.backward(torch.zeros_like(y))
    _check_sinks(block, log, versions)
    return log.count("owlk_gemm")


def test_dit_reports_each_parameter_once_and_stacks_the_modulation_wgrad(log):
    stacked = _dit_backward(log, split_stack=False)
    del log[:]
    split = _dit_backward(log, split_stack=True)
    # the four modulation weights' gradients: one GEMM onto the [6d, d] stack of their views, or four
    assert split - stacked == 3
