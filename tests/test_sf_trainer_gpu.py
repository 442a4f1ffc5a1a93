"""SelfForceTrainer (trainers/sf_trainer.py) on the GPU, with the tiny model of test_decode_grad_gpu.py
on synthetic data: the phases of the outer step train what they should and nothing else, a resumed run
equals an uninterrupted one bit for bit, and the eval sampler runs on the EMA core."""
import os

import pytest
import torch

import conftest  # noqa: F401  (sys.path)

pytestmark = pytest.mark.gpu

TINY = dict(model_id="game_rft", sample_size=8, channels=32, n_layers=2, n_heads=2, d_model=128,
            tokens_per_frame=64, n_buttons=11, cfg_prob=0.1, n_frames=8, causal=True, uncond=False,
            backbone="dit", has_audio=False, rope_impl="motion", rope_ats_delta=2.0, local_window=2,
            global_window=None)


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def make_trainer(ckpt_dir, **train):
    from owl_wms.configs import TrainingConfig, WANDBConfig, make_section, model_config
    from owl_wms.trainers import get_trainer_cls
    kw = dict(trainer_id="sforce_vid", data_id="cod", data_kwargs={"window_length": 4}, batch_size=1,
              target_batch_size=2, opt="AdamW", opt_kwargs={"lr": 1.0e-3, "betas": [0.9, 0.999]},
              d_opt_kwargs={"lr": 2.0e-3, "betas": [0.9, 0.999]}, update_ratio=2, rollout_steps=2,
              min_rollout_frames=2, seed=11, checkpoint_dir=str(ckpt_dir), save_interval=1000, sample_interval=1000)
    kw.update(train)
    torch.manual_seed(0)  # the three cores' own initialisation
    return get_trainer_cls("sforce_vid")(make_section(TrainingConfig, kw), make_section(WANDBConfig, {}),
                                         model_config(**TINY))


def snap(module):
    return {k: v.detach().clone() for k, v in module.state_dict().items()}


def same(a, b):
    return a.keys() == b.keys() and all(torch.equal(a[k], b[k]) for k in a)


def opt_state_equal(a, b):
    sa, sb = a.state_dict()["state"], b.state_dict()["state"]
    if sa.keys() != sb.keys():
        return False
    return all(torch.equal(torch.as_tensor(sa[i][k]).cpu(), torch.as_tensor(sb[i][k]).cpu())
               for i in sa for k in sa[i])


@pytest.fixture(scope="module")
def three_steps(tmp_path_factory):
    """3 uninterrupted outer steps, with the models snapshotted around each phase"""
    tr = make_trainer(tmp_path_factory.mktemp("run_a"))
    log = []
    critic_phase, student_phase, outer_step = tr.critic_phase, tr.student_phase, tr.outer_step

    def around(name, phase):
        def run():
            before = {m: snap(getattr(tr, m)) for m in ("teacher", "student", "critic")}
            phase()
            log.append((name, before, {m: snap(getattr(tr, m)) for m in ("teacher", "student", "critic")}))
        return run

    def outer():
        outer_step()
        log.append(("ema", tr.ema.step, snap(tr.ema.ema_model)))

    tr.critic_phase, tr.student_phase, tr.outer_step = around("critic", critic_phase), around("student", student_phase), outer
    tr.max_steps = 3
    tr.train()
    torch.cuda.synchronize()
    return tr, log


def test_two_outer_steps_train_the_right_models(three_steps):
    tr, log = three_steps
    for rec in tr.history[:2]:
        print(rec)
        for k in ("critic_loss", "dmd_loss", "g_norm", "time"):
            assert k in rec and torch.isfinite(torch.tensor(rec[k])), (k, rec)
    assert [r["step"] for r in tr.history] == [0, 1, 2]
    initial = log[0][1]
    phases = [e for e in log if e[0] in ("critic", "student")][:4]
    assert [e[0] for e in phases] == ["critic", "student", "critic", "student"]
    for name, before, after in phases:
        assert same(after["teacher"], initial["teacher"])  # the teacher never moves
        if name == "critic":
            assert not same(after["critic"], before["critic"]) and same(after["student"], before["student"])
        else:
            assert not same(after["student"], before["student"]) and same(after["critic"], before["critic"])
    emas = [e for e in log if e[0] == "ema"]
    assert emas[1][1] == 2 and not same(emas[1][2], initial["student"])
    assert not tr.student.transformer.decoding and not tr.critic.transformer.decoding


def test_resume_is_bit_identical(three_steps, tmp_path):
    a, _ = three_steps
    b = make_trainer(tmp_path, save_interval=2)
    b.max_steps = 2
    b.train()
    ckpt = os.path.join(str(tmp_path), "step_2.pt")
    assert sorted(torch.load(ckpt, map_location="cpu", weights_only=True)) == sorted(
        ["model", "ema", "opt", "critic", "critic_opt", "steps"])
    c = make_trainer(tmp_path, resume_ckpt=ckpt)
    c.max_steps = 1
    c.train()
    torch.cuda.synchronize()
    assert c.total_step_counter == a.total_step_counter == 3 and c.history[0]["step"] == 2
    assert c.history[0]["dmd_loss"] == a.history[2]["dmd_loss"]
    assert c.history[0]["critic_loss"] == a.history[2]["critic_loss"]
    assert same(snap(c.student), snap(a.student)) and same(snap(c.critic), snap(a.critic))
    assert same(snap(c.ema.ema_model), snap(a.ema.ema_model)) and c.ema.step == a.ema.step == 3
    assert opt_state_equal(c.opt, a.opt) and opt_state_equal(c.critic_opt, a.critic_opt)


def test_eval_runs_at_step_zero(tmp_path):
    tr = make_trainer(tmp_path, sampler_id="av_caching", n_samples=1, sample_data_id="cod",
                      sample_data_kwargs={"window_length": 4},
                      sampler_kwargs={"n_steps": 2, "num_frames": 2, "cfg_scale": 1.0, "noise_prev": 0.0})
    tr.max_steps = 1
    tr.train()
    rec = tr.history[0]
    print(rec)
    assert rec["eval/samples"] == 1 and rec["eval/frames"] == 6  # 4 context frames + 2 generated
    assert torch.isfinite(torch.tensor(rec["eval/latent_std"])) and rec["eval/latent_std"] > 0
