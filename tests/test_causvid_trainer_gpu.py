"""CausVidTrainer (trainers/causvid_trainer.py) on the GPU, on synthetic data.

* the tiny game_rft of test_sf_trainer_gpu.py, window 8, gen_mask_p 0.5: each phase of the outer step trains its
  own model and nothing else, the records are finite and every step generates frames, a resumed run equals an
  uninterrupted one bit for bit, and the eval sampler runs on the EMA core;
* the tiny game_rft_audio of test_av_stream_gpu.py (mmdit, audio_channels 16): both modalities' losses are logged
  and finite, the student's video and audio heads both learn, the teacher never moves, the eval of
  AVRFTTrainer runs and nothing is left in decoding mode."""
import math
import os

import pytest
import torch

import conftest  # noqa: F401  (sys.path)

pytestmark = pytest.mark.gpu

TINY = dict(model_id="game_rft", sample_size=8, channels=32, n_layers=2, n_heads=2, d_model=128,
            tokens_per_frame=64, n_buttons=11, cfg_prob=0.1, n_frames=8, causal=True, uncond=False,
            backbone="dit", has_audio=False, rope_impl="motion", rope_ats_delta=2.0, local_window=2,
            global_window=None)
MMCFG = dict(model_id="game_rft_audio", sample_size=8, channels=32, audio_channels=16, n_layers=2, n_heads=2,
             d_model=128, tokens_per_frame=65, n_buttons=11, n_mouse_axes=2, cfg_prob=0.1, n_frames=8, causal=True,
             uncond=False, backbone="mmdit", local_window=2, global_window=4, has_audio=True, rope_impl="motion",
             rope_ats_delta=2.0)
MODELS = ("teacher", "student", "critic")


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def make_trainer(ckpt_dir, model=TINY, **train):
    from owl_wms.configs import TrainingConfig, WANDBConfig, make_section, model_config
    from owl_wms.trainers import get_trainer_cls
    # seed 11: with gen_mask_p 0.5 every one of the steps below generates frames (asserted)
    kw = dict(trainer_id="causvid", data_id="cod", data_kwargs={"window_length": 8}, batch_size=1,
              target_batch_size=2, opt="AdamW", opt_kwargs={"lr": 1.0e-3, "betas": [0.9, 0.999]},
              d_opt_kwargs={"lr": 2.0e-3, "betas": [0.9, 0.999]}, update_ratio=2, gen_mask_p=0.5,
              regression_weight=0.25, seed=11, checkpoint_dir=str(ckpt_dir), save_interval=1000, sample_interval=1000)
    kw.update(train)
    torch.manual_seed(0)  # the three cores' own initialisation
    return get_trainer_cls("causvid")(make_section(TrainingConfig, kw), make_section(WANDBConfig, {}),
                                      model_config(**model))


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


def run_logged(tr, steps):
    """``steps`` outer steps with the three models snapshotted around each phase"""
    log = []
    critic_phase, student_phase, outer_step = tr.critic_phase, tr.student_phase, tr.outer_step

    def around(name, phase):
        def run():
            before = {m: snap(getattr(tr, m)) for m in MODELS}
            phase()
            log.append((name, before, {m: snap(getattr(tr, m)) for m in MODELS}))
        return run

    def outer():
        outer_step()
        log.append(("ema", tr.ema.step, snap(tr.ema.ema_model)))

    tr.critic_phase, tr.student_phase, tr.outer_step = around("critic", critic_phase), around("student", student_phase), outer
    tr.max_steps = steps
    tr.train()
    torch.cuda.synchronize()
    return log


def check_phases(log, n_steps):
    initial = log[0][1]
    phases = [e for e in log if e[0] in ("critic", "student")]
    assert [e[0] for e in phases] == ["critic", "student"] * n_steps
    for name, before, after in phases:
        assert same(after["teacher"], initial["teacher"])  # the teacher never moves
        if name == "critic":
            assert not same(after["critic"], before["critic"]) and same(after["student"], before["student"])
        else:
            assert not same(after["student"], before["student"]) and same(after["critic"], before["critic"])
    return initial, phases


# ------------------------------------------------------------------------------------ game_rft
@pytest.fixture(scope="module")
def three_steps(tmp_path_factory):
    tr = make_trainer(tmp_path_factory.mktemp("run_a"))
    return tr, run_logged(tr, 3)


def test_outer_steps_train_the_right_models(three_steps):
    tr, log = three_steps
    for rec in tr.history:
        print(rec)
        for k in ("critic_loss", "dmd_loss", "regression_loss", "g_norm", "gen_frames", "time"):
            assert k in rec and math.isfinite(rec[k]), (k, rec)
        assert rec["gen_frames"] > 0 and rec["gen_frames"] == int(rec["gen_frames"]) <= 2 * 8
        assert rec["critic_loss"] > 0 and rec["dmd_loss"] > 0 and rec["regression_loss"] > 0
        assert "dmd_loss_audio" not in rec
    assert [r["step"] for r in tr.history] == [0, 1, 2]
    initial, _ = check_phases(log, 3)
    emas = [e for e in log if e[0] == "ema"]
    assert emas[1][1] == 2 and not same(emas[1][2], initial["student"])


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
    for k in ("dmd_loss", "regression_loss", "critic_loss", "gen_frames", "g_norm"):
        assert c.history[0][k] == a.history[2][k], k
    assert same(snap(c.student), snap(a.student)) and same(snap(c.critic), snap(a.critic))
    assert same(snap(c.ema.ema_model), snap(a.ema.ema_model)) and c.ema.step == a.ema.step == 3
    assert opt_state_equal(c.opt, a.opt) and opt_state_equal(c.critic_opt, a.critic_opt)


def test_eval_runs_at_step_zero(tmp_path):
    tr = make_trainer(tmp_path, update_ratio=1, sampler_id="av_caching", n_samples=1, sample_data_id="cod",
                      sample_data_kwargs={"window_length": 4},
                      sampler_kwargs={"n_steps": 2, "num_frames": 2, "cfg_scale": 1.0, "noise_prev": 0.0})
    tr.max_steps = 1
    tr.train()
    rec = tr.history[0]
    print(rec)
    assert rec["eval/samples"] == 1 and rec["eval/frames"] == 6  # 4 context frames + 2 generated
    assert math.isfinite(rec["eval/latent_std"]) and rec["eval/latent_std"] > 0
    assert not tr.ema.ema_model.transformer.decoding and not tr.student.transformer.decoding


# ------------------------------------------------------------------------------------ game_rft_audio
def test_audio_video_model_trains_both_heads(tmp_path):
    tr = make_trainer(tmp_path, model=MMCFG, update_ratio=1, sampler_id="av_causal_no_cfg", n_samples=1,
                      sample_data_id="cod", sample_data_kwargs={"window_length": 4}, sample_interval=1,
                      sampler_kwargs={"n_steps": 2, "window_length": 4, "num_frames": 2, "noise_prev": 0.2,
                                      "only_return_generated": False})
    assert tr.av
    log = run_logged(tr, 2)
    for rec in tr.history:
        print(rec)
        for k in ("critic_loss", "critic_loss_audio", "dmd_loss", "dmd_loss_audio", "regression_loss",
                  "regression_loss_audio", "g_norm", "gen_frames"):
            assert k in rec and math.isfinite(rec[k]), (k, rec)
        assert rec["gen_frames"] > 0
        for key in ("eval/samples", "eval/frames", "eval/latent_std", "eval/audio_std"):
            assert key in rec and math.isfinite(rec[key]), key
        assert rec["eval/frames"] == 4 + 2 and rec["eval/samples"] == 1
    _, phases = check_phases(log, 2)
    for name, before, after in phases:
        if name == "student":  # both modalities' heads learn from the student's loss
            for w in ("proj_out.proj.weight", "audio_proj_out.proj.weight"):
                assert not torch.equal(after["student"][w], before["student"][w]), w
    for m in (tr.teacher, tr.student, tr.critic, tr.ema.ema_model):
        assert not m.transformer.decoding
