"""Gradients through the KV-cache decode step: the parts that need no GPU.

* the C ABI of owlk_attn_decode_bwd refuses what its kernels cannot take, on the host;
* RolloutManager's control flow (sf_vid_only.py:112-225) with a stub model and a recording cache;
* get_critic_loss / get_dmd_loss (sf_vid_only.py:229-349) against an fp64 restatement.
"""
import os
import random
import re

import pytest
import torch
from torch import nn

import conftest  # noqa: F401  (sys.path)


# ---------------------------------------------------------------------------------------- 1. ABI
def _args(D=64, Lq=64, Lkv=384, Lnew=64, q=4096, ws=8192, ws_bytes=None, B=1, H=2):
    """Stand-in 16-byte-aligned addresses; nothing is dereferenced (the checks fail first)."""
    from owl_wms._lib import lib
    ld = H * D
    if ws_bytes is None:
        ws_bytes = lib().owlk_attn_decode_bwd_ws_bytes(B, H, Lq, Lkv, D if D in (64, 128) else 64)
    p = (4096, ld, 0)
    return ((q, ld, 0) + p + p + p + (4096, 4096) + p + p + p
            + (B, H, Lq, Lkv, Lnew, D, D ** -0.5, ws, ws_bytes, None))


def _need_lib():
    from owl_wms import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libowlk.so not built (run __graft_entry__.build())")
    return _lib


@pytest.mark.parametrize("kw,msg", [
    (dict(D=96), "head_dim 96 not built"),
    (dict(Lkv=32, Lnew=64), "Lnew=64 must lie in 0 .. Lkv=32"),
    (dict(q=4098), "16-byte aligned"),
    (dict(ws_bytes=1024), "workspace of 1024 bytes"),
    (dict(ws=8200), "workspace must be 256-byte aligned"),
    (dict(Lq=0), "bad sizes"),
])
def test_decode_bwd_abi_refusals(kw, msg):
    _lib = _need_lib()
    args = _args(**kw)
    assert _lib.lib().owlk_attn_decode_bwd(*args) != 0
    assert msg in _lib.lib().owlk_last_error().decode()
    with pytest.raises(RuntimeError, match=re.escape(msg)):
        _lib.call("owlk_attn_decode_bwd", *args)


def test_decode_bwd_ws_bytes():
    q = _need_lib().lib().owlk_attn_decode_bwd_ws_bytes
    for D in (64, 128):
        prev = 0
        for Lkv in (1, 63, 64, 128, 129, 256, 257, 1000, 3840, 4160):
            n = q(2, 3, 64, Lkv, D)
            assert n > 0 and n % 256 == 0 and n >= prev
            assert n >= 2 * 3 * 64 * D * 4  # at least one split's fp32 partial dQ
            prev = n
    assert q(1, 24, 64, 3840, 64) == 24 * 15 * 64 * 64 * 4  # 256-key splits at head_dim 64
    assert q(1, 20, 64, 3840, 128) == 20 * 30 * 64 * 128 * 4  # 128-key splits at head_dim 128
    assert q(1, 2, 64, 384, 96) == 0


# ---------------------------------------------------------------------------------------- 2. rollout
class _Cfg:
    n_layers, tokens_per_frame, backbone = 2, 4, "dit"


class _RecordingCache:
    log = None

    def __init__(self, config):
        self.should_update = False

    def reset(self, b):
        self.log.append(("reset", b))

    def enable_cache_updates(self):
        self.should_update = True
        self.log.append("enable")

    def disable_cache_updates(self):
        self.should_update = False
        self.log.append("disable")

    def truncate(self, amt, front=False):
        self.log.append(("truncate", amt, front))


class _StubCore(nn.Module):
    """velocity = a * x + ts: ignores the cache; records each call"""

    def __init__(self, log):
        super().__init__()
        self.a = nn.Parameter(torch.tensor(0.5))
        self.calls = log
        outer = self

        class T:
            def enable_decoding(self):
                outer.calls.append("decoding on")

            def disable_decoding(self):
                outer.calls.append("decoding off")
        self.transformer = T()

    def forward(self, x, ts, mouse, btn, kv_cache=None):
        self.calls.append(("model", x.shape[1], torch.is_grad_enabled(), kv_cache.should_update, float(ts.mean())))
        return self.a * x + ts[:, :, None, None, None]


def test_rollout_manager_control_flow(monkeypatch):
    from owl_wms.trainers import self_forcing as SF
    log = []
    _RecordingCache.log = log
    monkeypatch.setattr(SF, "KVCache", _RecordingCache)
    B, ctx, roll, C, h = 2, 3, 2, 3, 2
    torch.manual_seed(0)
    video, mouse, btn = torch.randn(B, ctx, C, h, h), torch.randn(B, ctx, 2), torch.rand(B, ctx, 5).round()
    model = _StubCore(log)
    random.seed(5)
    steps = [random.randint(1, 3) for _ in range(roll)]  # the draws get_rollouts will make
    random.seed(5)
    out, m2, b2, gmask = SF.RolloutManager(_Cfg(), min_rollout_frames=roll, rollout_steps=3).get_rollouts(
        model, video, mouse, btn)

    assert out.shape == video.shape and m2.shape == mouse.shape and b2.shape == btn.shape
    assert gmask.shape == (B, ctx) and gmask.dtype == torch.bool
    assert torch.equal(gmask, torch.tensor([[False, True, True]] * B))  # last `ctx` of [3 context | 2 generated]
    assert torch.equal(out[:, 0], video[:, -1])  # the window's first frame is the last context frame

    expect = [("reset", B), "enable", ("model", ctx, False, True, 0.0), "disable", "decoding on"]
    for n in steps:
        for s in range(n - 1):  # Euler steps of 1/3 without gradient
            expect.append(("model", 1, False, False, pytest.approx(1.0 - s / 3)))
        expect.append(("model", 1, True, False, pytest.approx(1.0 - (n - 1) / 3)))  # the one step with grad
        expect += ["enable", ("model", 1, False, True, 0.0), "disable", ("truncate", 1, False)]
    expect.append("decoding off")
    assert log == expect
    assert sum(1 for e in log if isinstance(e, tuple) and e[0] == "model" and e[2]) == roll

    out[gmask].square().sum().backward()
    assert model.a.grad is not None and model.a.grad.abs().item() > 0


# ---------------------------------------------------------------------------------------- 3. losses
class _Lin(nn.Module):
    def __init__(self, a, b, c):
        super().__init__()
        self.a, self.b, self.c = nn.Parameter(torch.tensor(a)), b, c

    def forward(self, x, ts, mouse, btn, kv_cache=None):
        return self.a * x + self.b * ts[:, :, None, None, None] + self.c * mouse.sum(-1)[:, :, None, None, None] \
            + 0.1 * btn.sum(-1)[:, :, None, None, None]


class _FixedRollout:
    """a rollout manager whose rollout is given (the losses are what is under test)"""

    def __init__(self, video, mouse, btn, mask, noise):
        self.out, self.noise_source = (video, mouse, btn, mask), noise

    def get_rollouts(self, model, video, mouse, btn):
        v, m, b, g = self.out
        return v * model.a / model.a.detach(), m, b, g  # value unchanged, gradient path to the student


def _loss_setup():
    from owl_wms.trainers import self_forcing as SF
    torch.manual_seed(3)
    B, N, C, h = 2, 4, 3, 2
    f64 = torch.float64  # the formulas are under test, not fp32 rounding: everything in double
    video, mouse, btn = torch.randn(B, N, C, h, h, dtype=f64), torch.randn(B, N, 2, dtype=f64), \
        torch.rand(B, N, 5, dtype=f64).round()
    mask = torch.tensor([[False, False, True, True], [False, True, True, True]])
    ts_raw, z = torch.randn(B, N, dtype=f64), torch.randn(B, N, C, h, h, dtype=f64)
    rm = _FixedRollout(video, mouse, btn, mask, SF.InjectedRolloutNoise([ts_raw, z]))
    return SF, rm, video, mouse, btn, mask, ts_raw, z


def _v64(net, x, ts, mouse, btn):
    a, b, c = float(net.a.detach()), net.b, net.c
    e = lambda t: t[:, :, None, None, None]  # noqa: E731
    return a * x + b * e(ts) + c * e(mouse.double().sum(-1)) + 0.1 * e(btn.double().sum(-1))


def test_critic_loss_formula():
    SF, rm, video, mouse, btn, mask, ts_raw, z = _loss_setup()
    student, critic = _Lin(1.0, 0.0, 0.0), _Lin(0.7, 0.3, 0.2)
    loss = SF.get_critic_loss(student, critic, video, mouse, btn, rm)
    V, Z, ts = video.double(), z.double(), ts_raw.sigmoid().double()
    e = ts[:, :, None, None, None]
    noisy = V * (1 - e) + Z * e
    m = mask[:, :, None, None, None].double()
    ref = (((_v64(critic, noisy, ts, mouse, btn) - (Z - V)) * m) ** 2).mean()  # masked frames count as zeros
    assert abs(loss.item() - ref.item()) <= 1e-6 * abs(ref.item())
    loss.backward()
    assert critic.a.grad is not None and student.a.grad is None  # no gradient to the student


@pytest.mark.parametrize("cfg", [1.5, 1.0])
def test_dmd_loss_formula(cfg):
    SF, rm, video, mouse, btn, mask, ts_raw, z = _loss_setup()
    student, critic, teacher = _Lin(1.0, 0.0, 0.0), _Lin(0.7, 0.3, 0.2), _Lin(0.9, -0.2, 0.4)
    loss = SF.get_dmd_loss(student, critic, teacher, video, mouse, btn, rm, cfg_scale=cfg)
    V, Z, ts = video.double(), z.double(), ts_raw.sigmoid().double()
    e = ts[:, :, None, None, None]
    noisy = V * (1 - e) + Z * e
    vc = _v64(teacher, noisy, ts, mouse, btn)
    vu = _v64(teacher, noisy, ts, torch.zeros_like(mouse), torch.zeros_like(btn))
    vt = vu + cfg * (vc - vu) if cfg != 1.0 else vc
    mu_t, mu_c = noisy - e * vt, noisy - e * _v64(critic, noisy, ts, mouse, btn)
    norm = (V - mu_t).abs().mean(dim=[1, 2, 3, 4], keepdim=True)
    grad = (mu_c - mu_t) / norm
    ref = 0.5 * (grad[mask] ** 2).mean()  # 0.5 mse(video, video - grad) over the generated frames
    assert abs(loss.item() - ref.item()) <= 1e-6 * abs(ref.item())
    loss.backward()
    # d loss / d video = grad / n on the masked frames: through v * a / a.detach(), d/da = sum(video * grad) / n
    n = grad[mask].numel()
    assert abs(student.a.grad.item() - (V[mask] * grad[mask]).sum().item() / n) <= 1e-4 * abs(student.a.grad.item())
    assert critic.a.grad is None and teacher.a.grad is None


def test_dmd_loss_nan_to_num():
    """a sample whose teacher estimate equals the video exactly has normaliser 0 and, with critic ==
    teacher, gradient 0 / 0: nan_to_num makes that a zero gradient, and the loss stays finite"""
    SF, rm, video, mouse, btn, mask, ts_raw, z = _loss_setup()
    video, z, mouse, btn = video.clone(), z.clone(), mouse.clone(), btn.clone()
    video[0], z[0], mouse[0], btn[0] = 0, 0, 0, 0  # noisy[0] = 0 and the stubs' velocity there is 0
    rm = _FixedRollout(video, mouse, btn, mask, SF.InjectedRolloutNoise([ts_raw, z]))
    student, net = _Lin(1.0, 0.0, 0.0), _Lin(0.7, 0.0, 0.2)
    loss = SF.get_dmd_loss(student, net, net, video, mouse, btn, rm, cfg_scale=1.0)
    assert torch.isfinite(loss) and loss.item() == 0.0  # critic == teacher: zero gradient everywhere


def test_trainer_registry_points_at_the_rollout():
    from owl_wms.trainers import get_trainer_cls
    with pytest.raises(NotImplementedError, match="self_forcing.py"):
        get_trainer_cls("sf_vid_only")
