"""CausVid distillation (trainers/causvid.py, trainers/causvid_trainer.py): the parts that need no GPU.

* the registry, the two configs, the new TrainingConfig keys;
* the torch tails in float64 on stub linear models against a restatement of causvid_vid_only.py:101-309 written
  out here (loss values and d / d student), for the video model and for the audio + video form;
* the draw order, the bit-exact context frames, who gets a gradient, the all-false mask;
* the C ABI of the three kernels refuses what they cannot take, on the host.
"""
import os
import re

import pytest
import torch
from torch import nn

from conftest import REPO

F64 = torch.float64


# ------------------------------------------------------------------------------ registry, configs
def test_registry_returns_the_causvid_trainer():
    from owl_wms.trainers import get_trainer_cls
    from owl_wms.trainers.causvid_trainer import CausVidTrainer
    from owl_wms.trainers.distill_base import DistillTrainer
    from owl_wms.trainers.sf_trainer import SelfForceTrainer
    assert get_trainer_cls("causvid") is CausVidTrainer
    assert issubclass(CausVidTrainer, DistillTrainer) and issubclass(SelfForceTrainer, DistillTrainer)


def test_training_config_defaults():
    from owl_wms.configs import TrainingConfig
    c = TrainingConfig()
    assert (c.regression_weight, c.gen_mask_p, c.noise_prev, c.cfg_scale) == (0.0, 0.25, 0.2, 1.5)


@pytest.mark.parametrize("name,student_of,window,sampler", [
    ("dit_v4_causvid.yml", "dit_v4_sf.yml", 60, "av_caching"),
    ("mmdit_v2_causvid.yml", "mmdit_v2.yml", 16, "av_causal_no_cfg")])
def test_configs_load(name, student_of, window, sampler):
    from owl_wms.configs import Config
    from owl_wms.sampling import get_sampler_cls
    c = Config.from_yaml(os.path.join(REPO, "configs", name))
    t = c.train
    assert t.trainer_id == "causvid" and c.model.cfg_prob == 0 and c.model.causal
    assert t.data_kwargs.window_length == window and t.sample_data_kwargs.window_length == window
    assert (t.update_ratio, t.gen_mask_p, t.noise_prev, t.cfg_scale, t.regression_weight) == (5, 0.25, 0.2, 1.5, 0.0)
    assert t.opt == "AdamW" and t.opt_kwargs.lr == 2.0e-6 and t.d_opt_kwargs.lr == 2.0e-6
    assert t.teacher_ckpt is None and t.student_ckpt is None and t.resume_ckpt is None
    assert t.sampler_id == sampler and get_sampler_cls(sampler) is not None
    assert os.path.exists(os.path.join(REPO, t.teacher_cfg))
    same_arch = lambda m: {k: v for k, v in m.items() if k != "cfg_prob"}  # noqa: E731
    assert same_arch(c.model) == same_arch(Config.from_yaml(os.path.join(REPO, "configs", student_of)).model)
    assert same_arch(c.model) == same_arch(Config.from_yaml(os.path.join(REPO, t.teacher_cfg)).model)


# ------------------------------------------------------------------------------ stub models
def _e(t, like):
    return t.reshape(t.shape + (1,) * (like.dim() - 2))


class _Lin(nn.Module):
    """video model: velocity = a x + b ts + c sum(mouse) + 0.1 sum(btn)"""

    def __init__(self, a, b, c):
        super().__init__()
        self.a, self.b, self.c = nn.Parameter(torch.tensor(a, dtype=F64)), b, c

    def forward(self, x, ts, mouse, btn):
        return self.a * x + _e(self.b * ts + self.c * mouse.sum(-1) + 0.1 * btn.sum(-1), x)


class _LinAV(nn.Module):
    """audio + video model: the same per modality (audio with its own slope a2 and half the control term);
    has_controls False drops the control term, as the model's unconditional branch does"""

    def __init__(self, a, b, c):
        super().__init__()
        self.a, self.a2 = nn.Parameter(torch.tensor(a, dtype=F64)), nn.Parameter(torch.tensor(0.5 * a, dtype=F64))
        self.b, self.c = b, c

    def forward(self, x, audio, ts, mouse, btn, has_controls=None):
        ctrl = self.c * mouse.sum(-1) + 0.1 * btn.sum(-1)
        if has_controls is not None:
            ctrl = ctrl * has_controls.to(ctrl.dtype)[:, None]
        return self.a * x + _e(self.b * ts + ctrl, x), self.a2 * audio + _e(self.b * ts + 0.5 * ctrl, audio)


STUDENT, CRITIC, TEACHER = (1.1, 0.1, -0.3), (0.7, 0.3, 0.2), (0.9, -0.2, 0.4)
P, NOISE_PREV = 0.5, 0.2


def _setup(av, seed=3, p=P):
    """inputs, the injected draws in call order and fresh models"""
    from owl_wms.trainers import causvid as CV
    from owl_wms.trainers.self_forcing import InjectedRolloutNoise
    g = torch.Generator().manual_seed(seed)
    B, N, C, h, Ca = 2, 4, 3, 2, 8
    r = lambda *s: torch.randn(*s, generator=g, dtype=F64)  # noqa: E731
    x = dict(video=r(B, N, C, h, h), audio=r(B, N, Ca) if av else None, mouse=r(B, N, 2),
             btn=torch.rand(B, N, 5, generator=g, dtype=F64).round())
    shapes = [(B, N, C, h, h)] + ([(B, N, Ca)] if av else [])
    d = dict(u=torch.rand(B, N, generator=g), idx=torch.randint(0, 2, (B, N), generator=g),
             z=[r(*s) for s in shapes], ts_raw=r(B, N), z2=[r(*s) for s in shapes])
    draws = [d["u"], d["idx"]] + d["z"] + [d["ts_raw"]] + d["z2"]
    cls = _LinAV if av else _Lin
    models = [cls(*q) for q in (STUDENT, CRITIC, TEACHER)]
    rollouts = CV.CausVidRollouts(None, noise_prev=NOISE_PREV, gen_mask_p=p, noise_source=InjectedRolloutNoise(draws))
    return CV, x, d, models, rollouts


# ------------------------------------------------------------------------------ the restatement
def _run(model, xs, ts, mouse, btn, uncond=False):
    if len(xs) == 1:
        if uncond:
            mouse, btn = torch.zeros_like(mouse), torch.zeros_like(btn)
        return [model(xs[0], ts, mouse, btn)]
    hc = torch.zeros(xs[0].shape[0], dtype=torch.bool) if uncond else None
    return list(model(xs[0], xs[1], ts, mouse, btn, has_controls=hc))


def ref_rollout(student, xs, mouse, btn, d, p):
    """causvid_vid_only.py:132-164 -> (out, mask, ts_full, noisy)"""
    mask = d["u"] < p
    ts = torch.tensor([1.0, 0.5], dtype=F64)[d["idx"]]
    ts_full = torch.where(mask, ts, torch.full_like(ts, NOISE_PREV))
    noisy = [x * (1 - _e(ts_full, x)) + z * _e(ts_full, x) for x, z in zip(xs, d["z"])]
    v = _run(student, noisy, ts_full, mouse, btn)
    out = [torch.where(_e(mask, y), y - vi * _e(ts_full, y), x) for y, vi, x in zip(noisy, v, xs)]
    return out, mask, ts_full, noisy


def ref_critic(student, critic, xs, mouse, btn, d, p):
    """:171-208, summed over the modalities -> (loss, [part per modality])"""
    with torch.no_grad():
        out, mask, _, _ = ref_rollout(student, xs, mouse, btn, d, p)
        ts = d["ts_raw"].sigmoid()
        noisy = [o * (1 - _e(ts, o)) + z * _e(ts, o) for o, z in zip(out, d["z2"])]
    pred = _run(critic, noisy, ts, mouse, btn)
    parts = [(((pv - (z - o)) * _e(mask, o)) ** 2).mean() for pv, z, o in zip(pred, d["z2"], out)]
    return sum(parts), parts


def ref_gen(student, critic, teacher, xs, mouse, btn, d, p, cfg, w):
    """:210-309, summed over the modalities -> (loss, [dmd per modality], [regression per modality], pieces)"""
    out, mask, ts_full, noisy1 = ref_rollout(student, xs, mouse, btn, d, p)
    with torch.no_grad():
        ts = d["ts_raw"].sigmoid()
        noisy = [o * (1 - _e(ts, o)) + z * _e(ts, o) for o, z in zip(out, d["z2"])]
        vc = _run(teacher, noisy, ts, mouse, btn)
        vt = vc
        if cfg != 1.0:
            vu = _run(teacher, noisy, ts, mouse, btn, uncond=True)
            vt = [u + cfg * (c - u) for c, u in zip(vc, vu)]
        vk = _run(critic, noisy, ts, mouse, btn)
    dmds, regs, gs = [], [], []
    for o, x, y, t, k in zip(out, xs, noisy, vt, vk):
        with torch.no_grad():
            mu_t, mu_k = y - _e(ts, y) * t, y - _e(ts, y) * k
            norm = (o - mu_t).abs().mean(dim=list(range(1, o.dim())), keepdim=True)
            g = torch.nan_to_num((mu_k - mu_t) / norm, nan=0.0)
            target = (o - g).detach()
        m = _e(mask, o)
        dmds.append(0.5 * ((o * m - target * m) ** 2).mean())
        regs.append(((o * m - x * m) ** 2).mean())
        gs.append(g)
    loss = sum(dmds) + w * sum(regs)
    return loss, dmds, regs, dict(out=out, mask=mask, ts_full=ts_full, noisy1=noisy1, g=gs)


def _close(a, b, tol=1e-9):
    a, b = (float(t.detach()) if isinstance(t, torch.Tensor) else float(t) for t in (a, b))
    return abs(a - b) <= tol * max(abs(b), 1e-300)


def _xs(x):
    return [x["video"]] + ([x["audio"]] if x["audio"] is not None else [])


def _grads(model):
    return [q.grad for q in model.parameters()]


# ------------------------------------------------------------------------------ the torch tails
@pytest.mark.parametrize("av", [False, True], ids=["game_rft", "game_rft_audio"])
def test_critic_loss_formula(av):
    CV, x, d, (student, critic, _), rollouts = _setup(av)
    loss, parts = CV.get_critic_loss(student, critic, x["video"], x["mouse"], x["btn"], rollouts, audio=x["audio"],
                                     fused=False)
    loss.backward()
    rs, rc, _ = _setup(av)[3]
    ref, rparts = ref_critic(rs, rc, _xs(x), x["mouse"], x["btn"], d, P)
    ref.backward()
    print(f"critic loss av={av}: {loss.item():.12e} ref {ref.item():.12e}")
    assert _close(loss, ref) and loss.item() > 0
    assert list(parts) == ["critic_loss", "critic_loss_audio"][:len(rparts)]
    assert all(_close(parts[k], r) for k, r in zip(parts, rparts))
    assert all(_close(a, b) for a, b in zip(_grads(critic), _grads(rc)))
    assert all(g is None for g in _grads(student))  # no gradient to the student


@pytest.mark.parametrize("w", [0.0, 0.5])
@pytest.mark.parametrize("cfg", [1.5, 1.0])
@pytest.mark.parametrize("av", [False, True], ids=["game_rft", "game_rft_audio"])
def test_gen_loss_formula(av, cfg, w):
    CV, x, d, (student, critic, teacher), rollouts = _setup(av)
    loss, parts = CV.get_gen_loss(student, critic, teacher, x["video"], x["mouse"], x["btn"], rollouts, cfg_scale=cfg,
                                  regression_weight=w, audio=x["audio"], fused=False)
    loss.backward()
    rs, rc, rt = _setup(av)[3]
    xs = _xs(x)
    ref, dmds, regs, pc = ref_gen(rs, rc, rt, xs, x["mouse"], x["btn"], d, P, cfg, w)
    ref.backward()
    print(f"gen loss av={av} cfg={cfg} w={w}: {loss.item():.12e} ref {ref.item():.12e}; "
          f"d/da {student.a.grad.item():.12e} ref {rs.a.grad.item():.12e}")
    assert _close(loss, ref) and loss.item() > 0
    for s, dm, rg in zip(("", "_audio"), dmds, regs):
        assert _close(parts["dmd_loss" + s], dm) and _close(parts["regression_loss" + s], rg)
    assert ("dmd_loss_audio" in parts) == av and int(parts["gen_frames"]) == int(pc["mask"].sum()) > 0
    assert all(_close(a, b) for a, b in zip(_grads(student), _grads(rs)))
    # the only path is out -> v: d gen / d v = -ts_full m (g + 2 w (out - orig)) / n, and d v / d slope = noisy
    for q, o, orig, g, y in zip(student.parameters(), pc["out"], xs, pc["g"], pc["noisy1"]):
        dv = -_e(pc["ts_full"], o) * _e(pc["mask"], o) * (g + 2 * w * (o.detach() - orig)) / o.numel()
        assert _close(q.grad, (dv * y).sum(), 1e-8)
    # only the student learns from this loss
    assert all(g is None for g in _grads(critic) + _grads(teacher))


def test_gen_loss_all_false_mask_is_zero():
    CV, x, d, (student, critic, teacher), rollouts = _setup(True, p=0.0)
    loss, parts = CV.get_gen_loss(student, critic, teacher, x["video"], x["mouse"], x["btn"], rollouts,
                                  regression_weight=0.5, audio=x["audio"], fused=False)
    loss.backward()
    assert loss.item() == 0.0 and int(parts["gen_frames"]) == 0
    assert all(float(v) == 0.0 for v in parts.values())
    assert all(g is not None and g.item() == 0.0 for g in _grads(student))
    CV, x, d, (student, critic, _), rollouts = _setup(True, p=0.0)
    closs, _ = CV.get_critic_loss(student, critic, x["video"], x["mouse"], x["btn"], rollouts, audio=x["audio"],
                                  fused=False)
    closs.backward()
    assert closs.item() == 0.0 and all(g.item() == 0.0 for g in _grads(critic))


# ------------------------------------------------------------------------------ the rollout
@pytest.mark.parametrize("av", [False, True], ids=["game_rft", "game_rft_audio"])
def test_rollout_matches_and_keeps_context_frames_bit_for_bit(av):
    CV, x, d, (student, _, _), rollouts = _setup(av)
    out, mouse, btn, mask, orig = rollouts.get_rollouts(student, x["video"], x["mouse"], x["btn"], audio=x["audio"])
    rs = _setup(av)[3][0]
    xs = _xs(x)
    rout, rmask, _, _ = ref_rollout(rs, xs, x["mouse"], x["btn"], d, P)
    outs, origs = (list(out), list(orig)) if av else ([out], [orig])
    assert torch.equal(mask, rmask) and mask.any() and not mask.all()
    assert mouse is x["mouse"] and btn is x["btn"]
    for o, r, clean, given in zip(outs, rout, origs, xs):
        assert clean is given
        assert torch.allclose(o, r, rtol=1e-12, atol=0) and o.requires_grad
        assert torch.equal(o[~mask], given[~mask])  # context frames: the input, bit for bit
        assert not torch.equal(o[mask], given[mask])
    with torch.no_grad():  # the caller's grad mode applies
        _, _, _, (s2, _, _), r2 = _setup(av)
        o2 = r2.get_rollouts(s2, x["video"], x["mouse"], x["btn"], audio=x["audio"])[0]
        assert not (o2[0] if av else o2).requires_grad


def test_draw_order():
    """gen_mask, ts, z_video, z_audio in the rollout; then ts, z_video, z_audio in the loss -- all through the
    noise source"""
    from owl_wms.trainers.self_forcing import InjectedRolloutNoise, RolloutNoise
    CV, x, d, (student, critic, teacher), rollouts = _setup(True)
    log = []

    class Recording(InjectedRolloutNoise):
        def _next(self, shape, device, dtype):
            log.append((tuple(shape), dtype))
            return super()._next(shape, device, dtype)

    rollouts.noise_source = Recording(rollouts.noise_source.draws)
    CV.get_gen_loss(student, critic, teacher, x["video"], x["mouse"], x["btn"], rollouts, audio=x["audio"], fused=False)
    v, a = tuple(x["video"].shape), tuple(x["audio"].shape)
    assert log == [((2, 4), torch.float32), ((2, 4), torch.long), (v, F64), (a, F64), ((2, 4), F64), (v, F64), (a, F64)]
    assert rollouts.noise_source.i == 7
    # the default source makes the same kinds of draws
    torch.manual_seed(0)
    n = RolloutNoise()
    u, i = n.rand((2, 4), "cpu"), n.randint(0, 2, (2, 4), "cpu")
    assert u.dtype == torch.float32 and 0 <= u.min() and u.max() < 1 and tuple(u.shape) == (2, 4)
    assert i.dtype == torch.long and set(i.flatten().tolist()) <= {0, 1} and tuple(i.shape) == (2, 4)


# ------------------------------------------------------------------------------ C ABI
def _need_lib():
    from owl_wms import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libowlk.so not built (run __graft_entry__.build())")
    return _lib


def _mix(x=4096, ts=4096, noisy=8192, F=16):
    return (x, 4096, 0, ts, None, 0.2, 1, 2, F, noisy, None, None)


def _x0(noisy=4096, v=4096, mask=4096, F=16):
    return (noisy, 4096, 0, v, 0, 4096, mask, 1, 2, F, 8192, None)


def _gen(out=4096, dv=8192, v_critic=4096, F=16, ws=12288, ws_bytes=None, B=1):
    from owl_wms._lib import lib
    if ws_bytes is None:
        ws_bytes = lib().owlk_causvid_gen_loss_ws_bytes(B, 2, F if F % 8 == 0 else 16)
    return (out, 4096, 4096, 0, 4096, None, v_critic, 0, 4096, 4096, 4096, B, 2, F, 1.5, 0.0, 4096, dv, ws, ws_bytes,
            None)


@pytest.mark.parametrize("name,args,msg", [
    ("owlk_causvid_mix", lambda: _mix(F=12), "causvid_mix: F=12 elements per frame must be a multiple of 8"),
    ("owlk_causvid_mix", lambda: _mix(ts=None), "causvid_mix: x, z, ts and noisy are required"),
    ("owlk_causvid_mix", lambda: _mix(x=4104), "causvid_mix: tensors must be 16-byte aligned"),
    ("owlk_causvid_mix", lambda: _mix(F=0), "causvid_mix: bad sizes"),
    ("owlk_causvid_x0", lambda: _x0(F=20), "causvid_x0: F=20 elements per frame must be a multiple of 8"),
    ("owlk_causvid_x0", lambda: _x0(mask=None), "causvid_x0: noisy, clean, v, ts_full, mask and out are required"),
    ("owlk_causvid_x0", lambda: _x0(v=4098), "causvid_x0: tensors must be 16-byte aligned"),
    ("owlk_causvid_gen_loss", lambda: _gen(F=12), "causvid_gen_loss: F=12 elements per frame must be a multiple of 8"),
    ("owlk_causvid_gen_loss", lambda: _gen(v_critic=None), "ts_full, mask, losses and dv are required"),
    ("owlk_causvid_gen_loss", lambda: _gen(dv=8200), "causvid_gen_loss: tensors must be 16-byte aligned"),
    ("owlk_causvid_gen_loss", lambda: _gen(ws_bytes=8), "causvid_gen_loss: workspace of 8 bytes"),
    ("owlk_causvid_gen_loss", lambda: _gen(ws=None), "causvid_gen_loss: workspace of"),
    ("owlk_causvid_gen_loss", lambda: _gen(B=70000), "causvid_gen_loss: bad sizes B=70000"),
])
def test_c_abi_refusals(name, args, msg):
    """refused on the host before any HIP call (nothing is dereferenced: the addresses are stand-ins)"""
    _lib = _need_lib()
    args = args()
    assert getattr(_lib.lib(), name)(*args) != 0
    assert msg in _lib.lib().owlk_last_error().decode()
    with pytest.raises(RuntimeError, match=re.escape(msg)):
        _lib.call(name, *args)


def test_gen_loss_ws_bytes():
    q = _need_lib().lib().owlk_causvid_gen_loss_ws_bytes
    assert q(1, 1, 8) == 3 * 4 and q(2, 4, 16) == 3 * 2 * 4  # one workgroup per sample
    assert q(3, 5, 8192) == 3 * 3 * 10 * 4  # 5 * 1024 chunks per sample: 10 workgroups each
    assert q(1, 60, 8192) == 3 * 120 * 4 and q(1, 16, 64) == 3 * 4
    assert q(1, 1, 12) == 0 and q(0, 1, 8) == 0 and q(70000, 1, 8) == 0
