"""The audio + video window samplers (sampling/av_window.py) on the CPU: registry, the samplers' own
arithmetic against the reference's runs with a stub core (tests/golden/make_golden_av_sampler.py,
``stub.*``), the decoding flag's restore, and the refusals of the two MMDiT decode C entries."""
import os
from types import SimpleNamespace

import pytest
import torch

from conftest import golden

IDS = {"av_window": "AVWindowSampler", "av_causal": "CausalAVWindowSampler",
       "av_causal_no_cfg": "CausalAVWindowSamplerNoCFG"}


def rel(a, b):
    a, b = a.double(), b.double()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


class _Draws:
    """torch.randn_like draws replayed in order; every one must be consumed."""

    def __init__(self, like):
        self.q = list(like)

    def __enter__(self):
        self.saved = torch.randn_like

        def like(x, **kw):
            t = self.q.pop(0)
            assert t.shape == x.shape, (tuple(t.shape), tuple(x.shape))
            return t.to(device=x.device, dtype=x.dtype)

        torch.randn_like = like
        return self

    def __exit__(self, *exc):
        torch.randn_like = self.saved
        if exc[0] is None:
            assert not self.q, f"{len(self.q)} unconsumed draws"


class _Transformer:
    def __init__(self):
        self.decoding = False
        self.log = []

    def enable_decoding(self):
        self.decoding = True
        self.log.append("on")

    def disable_decoding(self):
        self.decoding = False
        self.log.append("off")


class StubCore:
    """The fixture's stub: per frame video_pred = av x + bv ts + cv has_controls sum(mouse), audio
    likewise; ignores the cache."""

    def __init__(self, coeffs, fail_at=None):
        self.c = coeffs
        self.config = SimpleNamespace(backbone="mmdit", n_layers=2, tokens_per_frame=65)
        self.transformer = _Transformer()
        self.calls = []
        self.fail_at = fail_at

    def __call__(self, x, audio, ts, mouse, btn, has_controls=None, kv_cache=None):
        self.calls.append((x.shape[0], x.shape[1], self.transformer.decoding, kv_cache is not None))
        if self.fail_at is not None and len(self.calls) > self.fail_at:
            raise RuntimeError("stub failure")
        c = self.c
        hc = torch.ones(x.shape[0]) if has_controls is None else has_controls.float()
        m = mouse.float().sum(-1) * hc[:, None]
        pv = c["av"] * x + c["bv"] * ts[:, :, None, None, None] + c["cv"] * m[:, :, None, None, None]
        pa = c["aa"] * audio + c["ba"] * ts[:, :, None] + c["ca"] * m[:, :, None]
        return pv, pa


def _sampler(sid, S, **kw):
    from owl_wms.sampling import get_sampler_cls
    st = S["settings"]
    return get_sampler_cls(sid)(n_steps=st["n_steps"], cfg_scale=st["cfg_scale"], window_length=st["window_length"],
                                num_frames=st["num_frames"], noise_prev=st["noise_prev"], **kw)


def _ins(S, tag="stub"):
    return [S[f"{tag}.in.{k}"] for k in ("x", "audio", "mouse", "btn")]


def test_registry():
    from owl_wms.sampling import av_window, get_sampler_cls
    for sid, name in IDS.items():
        assert get_sampler_cls(sid) is getattr(av_window, name)
    import inspect
    for name in IDS.values():
        sig = inspect.signature(getattr(av_window, name).__init__)
        assert [(k, p.default) for k, p in list(sig.parameters.items())[1:]] == [
            ("n_steps", 20), ("cfg_scale", 1.3), ("window_length", 60), ("num_frames", 60), ("noise_prev", 0.2),
            ("only_return_generated", False)]
    with pytest.raises(ValueError):
        get_sampler_cls("av_no_such_sampler")


@pytest.mark.parametrize("sid", list(IDS))
def test_stub_core_matches_reference(sid):
    """fp32, elementwise, the same formulas: rel-L2 <= 1e-6 against the reference's stub run; exact
    context; the reference's arity and shapes; every draw consumed."""
    S = golden("av_sampler_tiny.pt")
    core = StubCore(S["stub.coeffs"])
    ref = S[f"stub.{sid}.out"]
    with _Draws(S["stub.in.noise"]):
        out = _sampler(sid, S)(core, *_ins(S))
    assert len(out) == len(ref) == (6 if sid == "av_window" else 4)
    n_ctx = S["stub.in.x"].shape[1]
    for o, r in zip(out, ref):
        assert (o is None) == (r is None)
        if r is not None:
            assert o.shape == r.shape
            assert rel(o, r) <= 1e-6, rel(o, r)
    x, audio = out[-4], out[-3]
    assert torch.equal(x[:, :n_ctx], S["stub.in.x"]) and torch.equal(audio[:, :n_ctx], S["stub.in.audio"])
    assert not core.transformer.decoding
    W, steps, new = S["settings"]["window_length"], S["settings"]["n_steps"], S["settings"]["num_frames"]
    if sid == "av_window":  # the whole window at every step, cond | uncond as one batch, no cache
        assert core.calls == [(2, W, False, False)] * (steps * new)
    else:  # one cached window pass, then the last frame alone with decoding on
        nb = 2 if sid == "av_causal" else 1
        assert core.calls == ([(nb, W, False, True)] + [(nb, 1, True, True)] * (steps - 1)) * new


@pytest.mark.parametrize("sid", list(IDS))
def test_only_return_generated_slices_as_reference(sid):
    S = golden("av_sampler_tiny.pt")
    ref = S[f"stub.{sid}.out_generated"]
    with _Draws(S["stub.in.noise"]):
        out = _sampler(sid, S, only_return_generated=True)(StubCore(S["stub.coeffs"]), *_ins(S))
    new = S["settings"]["num_frames"]
    for o, r in zip(out, ref):
        if r is not None:
            assert o.shape == r.shape and o.shape[1] == new
            assert rel(o, r) <= 1e-6


def test_decode_fn_applied():
    S = golden("av_sampler_tiny.pt")
    ref = S["stub.av_window.out"]
    with _Draws(S["stub.in.noise"]):
        out = _sampler("av_window", S)(StubCore(S["stub.coeffs"]), *_ins(S), decode_fn=lambda t: t + 1.0,
                                       audio_decode_fn=lambda t: -t, image_scale=2.0, audio_scale=3.0)
    assert rel(out[0], ref[2] * 2.0 + 1.0) <= 1e-6 and rel(out[1], -3.0 * ref[3]) <= 1e-6
    assert rel(out[2], ref[2]) <= 1e-6 and rel(out[3], ref[3]) <= 1e-6
    ref = S["stub.av_causal.out"]
    with _Draws(S["stub.in.noise"]):
        out = _sampler("av_causal", S)(StubCore(S["stub.coeffs"]), *_ins(S), decode_fn=lambda t: t + 1.0,
                                       audio_decode_fn=lambda t: -t, image_scale=2.0, audio_scale=3.0)
    assert rel(out[0], ref[0] * 2.0 + 1.0) <= 1e-6 and rel(out[1], -3.0 * ref[1]) <= 1e-6


def test_causal_cfg_scale_zero_is_unconditional_only():
    """av_window.py:214-223: cfg_scale <= 0 -> the unconditional prediction alone (batch B)."""
    from owl_wms.sampling import get_sampler_cls
    S = golden("av_sampler_tiny.pt")
    st = S["settings"]
    core = StubCore(S["stub.coeffs"])
    coeffs0 = dict(S["stub.coeffs"], cv=0.0, ca=0.0)  # has_controls False == no control term
    kw = dict(n_steps=st["n_steps"], cfg_scale=0.0, window_length=st["window_length"], num_frames=st["num_frames"],
              noise_prev=st["noise_prev"])
    with _Draws(S["stub.in.noise"]):
        a = get_sampler_cls("av_causal")(**kw)(core, *_ins(S))
    with _Draws(S["stub.in.noise"]):
        b = get_sampler_cls("av_causal_no_cfg")(**kw)(StubCore(coeffs0), *_ins(S))
    assert {c[0] for c in core.calls} == {1}
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


@pytest.mark.parametrize("sid", ["av_causal", "av_causal_no_cfg"])
def test_decoding_flag_restored_when_the_model_raises(sid):
    S = golden("av_sampler_tiny.pt")
    core = StubCore(S["stub.coeffs"], fail_at=2)  # the second decode step of the first frame
    with pytest.raises(RuntimeError, match="stub failure"):
        with _Draws(S["stub.in.noise"]):
            _sampler(sid, S)(core, *_ins(S))
    assert core.calls[-1][2] is True  # it failed with decoding on
    assert core.transformer.decoding is False and core.transformer.log == ["on", "off"]


def test_av_trainer_other_sampler_ids_sample_nothing():
    from owl_wms.trainers.rft_trainer import AVRFTTrainer

    class T(AVRFTTrainer):
        def __init__(self, sid):
            self.train_cfg = {"sampler_id": sid} if sid else {}

    assert T(None).eval_setup() == (None, None)
    assert T("av_caching").eval_setup() == (None, None)


# ---- C entries: refused on the host before any HIP call (no GPU needed)
def _joint_args(n0=64, n1=1, D=64, q=4096, ldq=128):
    return (q, ldq, 0, 8192, 128, 0, 12288, 128, 0, 16384, 128, 20480, 128, None, 1, 2, n0, n1, 130, D, D ** -0.5,
            1.02 * D, None)


def _rope_args(tab_off=0, n_tab=390, q=16384, nf=1):
    return (4096, 384, 8192, 384, 1, nf, 64, 1, 2, 64, 32768, 36864, 32, n_tab, tab_off, q, 128, 0, 20480, 128, 0,
            24576, 128, 0, None)


@pytest.mark.parametrize("name,args,msg", [
    ("owlk_attn_decode_joint_fwd", _joint_args(n0=80, n1=1), "at most 80 rows (got 81)"),
    ("owlk_attn_decode_joint_fwd", _joint_args(D=128), "head_dim 128 not built"),
    ("owlk_attn_decode_joint_fwd", _joint_args(q=4104), "16-byte aligned"),
    ("owlk_attn_decode_joint_fwd", _joint_args(ldq=132), "16-byte aligned"),
    ("owlk_mm_qk_rope_fwd_kv", _rope_args(tab_off=390 - 64), "past the 390-row rope table"),
    ("owlk_mm_qk_rope_fwd_kv", _rope_args(nf=7), "past the 390-row rope table"),
    ("owlk_mm_qk_rope_fwd_kv", _rope_args(q=16392), "16-byte aligned"),
])
def test_mm_decode_entries_refuse_bad_arguments(name, args, msg):
    from owl_wms import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libowlk.so not built (run __graft_entry__.build())")
    assert getattr(_lib.lib(), name)(*args) == 1
    assert msg in _lib.lib().owlk_last_error().decode()
    with pytest.raises(RuntimeError):
        _lib.call(name, *args)
