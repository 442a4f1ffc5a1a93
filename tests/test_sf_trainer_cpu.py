"""SelfForceTrainer (trainers/sf_trainer.py): the parts that need no GPU -- the registry, the config,
the new TrainingConfig keys, the checkpoint's key handling and the construction of the three cores."""
import os

import pytest
import torch

from conftest import REPO

TINY = dict(model_id="game_rft", sample_size=8, channels=32, n_layers=2, n_heads=2, d_model=128,
            tokens_per_frame=64, n_buttons=11, cfg_prob=0.1, n_frames=8, causal=False, uncond=False,
            backbone="dit", has_audio=False, rope_impl="motion", rope_ats_delta=2.0, local_window=2,
            global_window=None)


def test_registry_returns_the_self_forcing_trainer():
    from owl_wms.trainers import get_trainer_cls
    from owl_wms.trainers.sf_trainer import SelfForceTrainer
    assert get_trainer_cls("sforce_vid") is SelfForceTrainer
    for unbuilt in ("causvid_vid", "ode_distill_vid"):
        with pytest.raises(NotImplementedError, match=unbuilt):
            get_trainer_cls(unbuilt)


def test_training_config_defaults():
    from owl_wms.configs import TrainingConfig
    c = TrainingConfig()
    assert c.student_ckpt is None and c.d_opt_kwargs is None
    assert (c.update_ratio, c.rollout_steps, c.min_rollout_frames) == (5, 1, 8)


def test_self_forcing_config_loads():
    from owl_wms.configs import Config
    c = Config.from_yaml(os.path.join(REPO, "configs", "dit_v4_sf.yml"))
    t = c.train
    assert t.trainer_id == "sforce_vid" and c.model.cfg_prob == 0 and c.model.causal
    assert (t.update_ratio, t.rollout_steps, t.min_rollout_frames) == (5, 2, 50)
    assert t.data_kwargs.window_length == 60 and t.opt == "AdamW"
    assert t.opt_kwargs.lr == 2.0e-6 and t.d_opt_kwargs.lr == 2.0e-6
    assert t.teacher_ckpt is None and t.student_ckpt is None and t.resume_ckpt is None
    assert t.sampler_id == "av_caching" and t.sampler_kwargs.n_steps == 2
    assert os.path.exists(os.path.join(REPO, t.teacher_cfg))
    # the student's architecture is the teacher's
    teacher = Config.from_yaml(os.path.join(REPO, t.teacher_cfg)).model
    assert {k: v for k, v in c.model.items() if k != "cfg_prob"} == {k: v for k, v in teacher.items()
                                                                    if k != "cfg_prob"}


def test_checkpoint_entries_ignore_the_reference_scalers():
    from owl_wms.trainers.sf_trainer import CKPT_KEYS, checkpoint_entries
    w = {"module.proj_in.weight": torch.ones(1)}
    state = {"model": dict(w), "ema": {"ema_model.module.proj_in.weight": torch.ones(1), "step": torch.tensor(3)},
             "opt": {"state": {}}, "critic": dict(w), "critic_opt": {"state": {}}, "steps": 7,
             "scaler": {"scale": 65536.0}, "critic_scaler": {"scale": 65536.0}}
    out = checkpoint_entries(state)
    assert tuple(out) == CKPT_KEYS and out["steps"] == 7
    assert list(out["model"]) == ["proj_in.weight"] and list(out["critic"]) == ["proj_in.weight"]
    assert "ema_model.proj_in.weight" in out["ema"] and "step" in out["ema"]
    plain = {k: v for k, v in state.items() if "scaler" not in k}
    assert tuple(checkpoint_entries(plain)) == CKPT_KEYS  # this trainer's own checkpoints have none
    with pytest.raises(KeyError, match="critic_opt"):
        checkpoint_entries({k: v for k, v in plain.items() if k != "critic_opt"})
    with pytest.raises(KeyError, match="discriminator"):
        checkpoint_entries(dict(plain, discriminator={}))


def test_construction_builds_three_cores():
    from owl_wms.configs import TrainingConfig, WANDBConfig, make_section, model_config
    from owl_wms.models.gamerft import GameRFTCore
    from owl_wms.trainers.sf_trainer import SelfForceTrainer
    torch.manual_seed(0)
    tr = SelfForceTrainer(make_section(TrainingConfig, dict(trainer_id="sforce_vid")), make_section(WANDBConfig, {}),
                          model_config(**TINY))
    assert tr.model_cfg.cfg_prob == 0.0 and tr.model_cfg.causal is True
    for m in (tr.teacher, tr.student, tr.critic):
        assert isinstance(m, GameRFTCore)
    assert not tr.teacher.training and not any(p.requires_grad for p in tr.teacher.parameters())
    for (n, a), b in zip(tr.student.named_parameters(), tr.critic.parameters()):
        assert a is not b and a.data_ptr() != b.data_ptr() and torch.equal(a, b), n
        assert a.requires_grad and b.requires_grad
