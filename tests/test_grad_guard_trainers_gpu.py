"""``train.grad_guard`` in the trainers, on the GPU with the tiny models of test_model_gpu.py and
test_sf_trainer_gpu.py: a non-finite gradient costs one optimizer step and nothing else, a finite one is
only watched (Muon) or clipped as before (AdamW), a resumed guarded run equals an uninterrupted one, and
``max_consecutive_skips`` ends a run that skips on and on.

Bad values are written into a bucket just before the guard looks (a wrapper around GradReducer.grad_guard);
no kernel is made to misbehave."""
import math
import os

import pytest
import torch
import yaml

from conftest import REPO

pytestmark = pytest.mark.gpu

TINY = dict(model_id="game_rft", sample_size=8, channels=32, n_layers=2, n_heads=2, d_model=128,
            tokens_per_frame=64, n_buttons=11, cfg_prob=0.1, n_frames=8, causal=True, uncond=False,
            backbone="dit", has_audio=False, rope_impl="motion", rope_ats_delta=2.0, local_window=2,
            global_window=None)


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


# ------------------------------------------------------------------ helpers
def rft_trainer(ckpt_dir, opt="AdamW", **train):
    from owl_wms.configs import TrainingConfig, WANDBConfig, make_section, model_config
    from owl_wms.trainers.rft_trainer import RFTTrainer
    if opt == "Muon":
        opt_kwargs = yaml.safe_load(open(os.path.join(REPO, "configs", "dit_v4.yml")))["train"]["opt_kwargs"]
    else:
        opt_kwargs = {"lr": 1.0e-3, "betas": [0.9, 0.999]}
    kw = dict(trainer_id="rft", data_id="synthetic", data_kwargs={"window_length": 4}, target_batch_size=2,
              batch_size=1, epochs=1, opt=opt, opt_kwargs=opt_kwargs, checkpoint_dir=str(ckpt_dir),
              save_interval=10 ** 9, sample_interval=10 ** 9, vae_scale=1.0, seed=77)
    kw.update(train)
    torch.manual_seed(0)  # the model's own initialisation
    return RFTTrainer(make_section(TrainingConfig, kw), make_section(WANDBConfig, {}), model_config(**TINY), 0, 0, 1)


def sf_trainer(ckpt_dir, **train):
    from owl_wms.configs import TrainingConfig, WANDBConfig, make_section, model_config
    from owl_wms.trainers import get_trainer_cls
    kw = dict(trainer_id="sforce_vid", data_id="cod", data_kwargs={"window_length": 4}, batch_size=1,
              target_batch_size=2, opt="AdamW", opt_kwargs={"lr": 1.0e-3, "betas": [0.9, 0.999]},
              d_opt_kwargs={"lr": 2.0e-3, "betas": [0.9, 0.999]}, update_ratio=2, rollout_steps=2,
              min_rollout_frames=2, seed=11, checkpoint_dir=str(ckpt_dir), save_interval=1000, sample_interval=1000)
    kw.update(train)
    torch.manual_seed(0)
    return get_trainer_cls("sforce_vid")(make_section(TrainingConfig, kw), make_section(WANDBConfig, {}),
                                         model_config(**TINY))


def snap(module):
    return {k: v.detach().clone() for k, v in module.state_dict().items()}


def same(a, b):
    return a.keys() == b.keys() and all(torch.equal(a[k], b[k]) for k in a)


def opt_snap(opt):
    """every state tensor of an optimizer (FusedAdamW, or the AdamW + Muon pair), cloned"""
    sd = opt.state_dict()
    parts = {"opt": sd} if "state" in sd else sd
    return {f"{part}.{i}.{k}": torch.as_tensor(v).detach().clone().cpu()
            for part, d in parts.items() for i, st in d["state"].items() for k, v in st.items()}


def finite(d):
    return all(bool(torch.isfinite(v).all()) for v in d.values())


def poison(monkeypatch, when):
    """GradReducer.grad_guard with a NaN written into flat[0][0] first, on the calls ``when(reducer, i)`` picks"""
    from owl_wms.utils.grad_reducer import GradReducer
    orig, calls = GradReducer.grad_guard, []

    def grad_guard(self, max_norm=None):
        i = len(calls)
        calls.append((self, max_norm))
        if when(self, i):
            self.flat[0][0] = float("nan")
        return orig(self, max_norm)

    monkeypatch.setattr(GradReducer, "grad_guard", grad_guard)
    return calls


def run_rft(tr, steps):
    """train ``steps`` optimizer steps; -> the state after each (seen from the EMA update, the step's last act)"""
    from owl_wms.utils.grad_reducer import EMA
    update, after = EMA.update, []

    def ema_update(self):
        update(self)
        after.append(dict(model=snap(tr.model), opt=opt_snap(tr.opt), ema=snap(tr.ema.ema_model), ema_step=tr.ema.step,
                          bucket_max=max(float(b.abs().max()) for b in tr.reducer.flat)))

    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(EMA, "update", ema_update)
        tr.max_steps = steps
        tr.train()
        torch.cuda.synchronize()
    return after


# ------------------------------------------------------------------ RFTTrainer
@pytest.mark.parametrize("opt", ["AdamW", "Muon"])
def test_rft_skips_the_poisoned_step_only(opt, tmp_path, monkeypatch):
    tr = rft_trainer(tmp_path, opt=opt, grad_guard=True)
    calls = poison(monkeypatch, lambda red, i: i == 1)
    s = run_rft(tr, 3)
    for rec in tr.history:
        print(rec)
    # norm only for Muon, the configured threshold otherwise
    assert [mn for _, mn in calls] == [None if opt == "Muon" else 10.0] * 3
    # step 1: nothing moved but the EMA's counter, and the buckets were zeroed
    assert same(s[1]["model"], s[0]["model"]) and same(s[1]["opt"], s[0]["opt"])
    assert tr.history[1]["skipped"] == 1 and not math.isfinite(tr.history[1]["grad_norm"])
    assert s[1]["ema_step"] == s[0]["ema_step"] + 1 == 2
    assert [x["bucket_max"] for x in s] == [0.0, 0.0, 0.0]
    assert math.isfinite(tr.history[1]["diffusion_loss"])
    # steps 0 and 2 train
    assert tr.history[0]["skipped"] == 0 and math.isfinite(tr.history[0]["grad_norm"]) and tr.history[0]["grad_norm"] > 0
    assert not same(s[2]["model"], s[1]["model"]) and finite(s[2]["model"]) and finite(s[2]["opt"])
    assert tr.history[2]["skipped"] == 1 and math.isfinite(tr.history[2]["grad_norm"])
    if opt == "AdamW":
        steps = {float(v) for k, v in s[2]["opt"].items() if k.endswith(".step")}
        assert steps == {2.0} and {float(v) for k, v in s[1]["opt"].items() if k.endswith(".step")} == {1.0}
    else:
        bufs = [k for k in s[0]["opt"] if k.endswith("momentum_buffer")]
        assert bufs and all(torch.equal(s[1]["opt"][k], s[0]["opt"][k]) for k in bufs)
        assert any(not torch.equal(s[2]["opt"][k], s[1]["opt"][k]) for k in bufs)


@pytest.mark.parametrize("opt,over", [("Muon", {}), ("AdamW", {"grad_clip_norm": 1.0e9})])
def test_rft_guard_only_watches(opt, over, tmp_path):
    """no bad value, and for AdamW a threshold out of reach: guard on and guard off give the same bits"""
    on = rft_trainer(tmp_path / "on", opt=opt, grad_guard=True, **over)
    s_on = run_rft(on, 2)
    off = rft_trainer(tmp_path / "off", opt=opt, **over)
    s_off = run_rft(off, 2)
    assert off.train_cfg.grad_guard is False and len(off.history) == 2
    for rec in on.history:
        print(rec)
        assert math.isfinite(rec["grad_norm"]) and rec["grad_norm"] > 0 and rec["skipped"] == 0
    assert all("grad_norm" not in rec and "skipped" not in rec for rec in off.history)
    assert [r["diffusion_loss"] for r in on.history] == [r["diffusion_loss"] for r in off.history]
    for a, b in zip(s_on, s_off):
        assert same(a["model"], b["model"]) and same(a["ema"], b["ema"]) and same(a["opt"], b["opt"])
        assert a["ema_step"] == b["ema_step"]


def test_rft_consecutive_skip_limit(tmp_path, monkeypatch):
    tr = rft_trainer(tmp_path, grad_guard=True, max_consecutive_skips=2)
    poison(monkeypatch, lambda red, i: True)
    tr.max_steps = 5
    with pytest.raises(RuntimeError, match=r"step 2: 3 model optimizer steps skipped in a row"):
        tr.train()
    print(tr.history)
    assert [r["step"] for r in tr.history] == [0, 1] and [r["skipped"] for r in tr.history] == [1, 2]


# ------------------------------------------------------------------ SelfForceTrainer
@pytest.fixture(scope="module")
def sf_guarded(tmp_path_factory):
    """3 uninterrupted guarded outer steps, nothing injected"""
    tr = sf_trainer(tmp_path_factory.mktemp("sf_guarded"), grad_guard=True)
    tr.max_steps = 3
    tr.train()
    torch.cuda.synchronize()
    return tr


def test_sf_poisoned_critic_update_is_skipped_alone(tmp_path, monkeypatch):
    tr = sf_trainer(tmp_path, grad_guard=True)
    poison(monkeypatch, lambda red, i: red is tr.critic_reducer and i == 0)  # the first of two critic updates
    log, step = [], tr._step

    def _step(model, opt, reducer):
        before, o_before = snap(model), opt_snap(opt)
        r = step(model, opt, reducer)
        log.append(("critic" if model is tr.critic else "student", before, snap(model), o_before, opt_snap(opt)))
        return r

    tr._step = _step
    tr.max_steps = 1
    tr.train()
    torch.cuda.synchronize()
    rec = tr.history[0]
    print(rec)
    assert [e[0] for e in log] == ["critic", "critic", "student"]
    assert same(log[0][1], log[0][2]) and same(log[0][3], log[0][4])  # skipped: critic and its optimizer as before
    assert not same(log[1][1], log[1][2]) and finite(log[1][2])  # the other critic update trains
    assert not same(log[2][1], log[2][2]) and finite(log[2][2])  # and so does the student
    assert rec["skipped"] == 1
    for k in ("critic_loss", "dmd_loss", "g_norm", "time"):
        assert math.isfinite(rec[k]), (k, rec)
    assert max(float(b.abs().max()) for b in tr.critic_reducer.flat) == 0.0


def test_sf_g_norm_equals_the_unguarded_run(sf_guarded, tmp_path):
    """the default threshold on both sides: the first logged g_norm (of the gradient before its clip) agrees"""
    off = sf_trainer(tmp_path)
    off.max_steps = 1
    off.train()
    a, b = sf_guarded.history[0]["g_norm"], off.history[0]["g_norm"]
    print(f"g_norm guarded {a!r} unguarded {b!r} rel {abs(a - b) / b:.3e}")
    assert "skipped" not in off.history[0] and sf_guarded.history[0]["skipped"] == 0
    assert math.isfinite(a) and abs(a - b) <= 1e-5 * b


def test_sf_guarded_resume_is_bit_identical(sf_guarded, tmp_path):
    a = sf_guarded
    b = sf_trainer(tmp_path, grad_guard=True, save_interval=2)
    b.max_steps = 2
    b.train()
    ckpt = os.path.join(str(tmp_path), "step_2.pt")
    assert sorted(torch.load(ckpt, map_location="cpu", weights_only=True)) == sorted(
        ["model", "ema", "opt", "critic", "critic_opt", "steps"])
    c = sf_trainer(tmp_path, grad_guard=True, resume_ckpt=ckpt)
    c.max_steps = 1
    c.train()
    torch.cuda.synchronize()
    assert c.total_step_counter == a.total_step_counter == 3 and c.history[0]["step"] == 2
    for k in ("dmd_loss", "critic_loss", "g_norm"):
        assert c.history[0][k] == a.history[2][k], k
    assert same(snap(c.student), snap(a.student)) and same(snap(c.critic), snap(a.critic))
    assert same(snap(c.ema.ema_model), snap(a.ema.ema_model)) and c.ema.step == a.ema.step == 3
    assert same(opt_snap(c.opt), opt_snap(a.opt)) and same(opt_snap(c.critic_opt), opt_snap(a.critic_opt))
