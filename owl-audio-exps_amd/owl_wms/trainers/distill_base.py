"""What the distillation trainers share (sf_trainer.SelfForceTrainer, causvid_trainer.CausVidTrainer;
reference: sf_vid_only.py:351-589, causvid_vid_only.py:311-560): a frozen teacher, a student and a critic
through ``load_core``, an optimizer and a GradReducer for each trained model, the restarting batch iterator,
per-micro-step seeding, batch skipping on resume, the checkpoint keys and the outer loop -- ``update_ratio``
critic updates, one student update, the EMA update, eval, checkpoint.  A subclass gives ``make_rollouts``,
``critic_phase`` and ``student_phase``.
"""
import gc
import random
from copy import deepcopy

import torch
import torch.distributed as dist

from ..configs import Config
from ..data import get_loader
from ..models import get_model_cls
from ..muon import FusedAdamW
from ..utils import Timer, freeze, strip_prefixes, versatile_load
from ..utils.grad_reducer import EMA, GradReducer
from ..utils.logging import LogHelper
from .base import BaseTrainer
from .rft_trainer import LatentEval

CKPT_KEYS = ("model", "ema", "opt", "critic", "critic_opt", "steps")
CKPT_IGNORED = ("scaler", "critic_scaler")  # the reference's GradScaler states: nothing to restore here


def checkpoint_entries(state):
    """The entries ``load`` restores from a checkpoint dict (a distillation trainer's here or the reference's,
    sf_vid_only.py:411-422): the six of CKPT_KEYS, module./_orig_mod. prefixes stripped from the weights;
    GradScaler entries are dropped, anything else unknown or missing is an error."""
    missing = [k for k in CKPT_KEYS if k not in state]
    unknown = [k for k in state if k not in CKPT_KEYS + CKPT_IGNORED]
    if missing or unknown:
        raise KeyError(f"distillation checkpoint: missing {missing}, unknown {unknown}")
    out = {k: state[k] for k in CKPT_KEYS}
    for k in ("model", "ema", "critic"):
        out[k] = strip_prefixes(out[k])
    return out


def load_core(model_cfg, ckpt_path):
    """sf_vid_only.py:359-387: the model from its config, weights through versatile_load into the full
    model first and into ``.core`` if that fails; -> the core"""
    model = get_model_cls(model_cfg.model_id)(model_cfg)
    if ckpt_path:
        sd = versatile_load(ckpt_path)
        try:
            model.load_state_dict(sd)
        except RuntimeError:
            model.core.load_state_dict(sd)
    return model.core


class _Batches:
    """sf_vid_only.py:90-110 (SoftResetIterator): restarts the loader when it runs out"""

    def __init__(self, loader):
        self.loader, self.it = loader, iter(loader)

    def __next__(self):
        try:
            return next(self.it)
        except StopIteration:
            self.it = iter(self.loader)
            return next(self.it)


class DistillTrainer(LatentEval, BaseTrainer):
    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self.model_cfg.cfg_prob = 0.0  # causal student, no control dropout (:355-357)
        self.model_cfg.causal = True
        teacher_cfg = self.train_cfg.get("teacher_cfg")
        teacher_cfg = Config.from_yaml(teacher_cfg).model if teacher_cfg else deepcopy(self.model_cfg)
        self.teacher = load_core(teacher_cfg, self.train_cfg.get("teacher_ckpt"))
        self.student = load_core(self.model_cfg, self.train_cfg.get("student_ckpt"))
        self.critic = deepcopy(self.student)
        freeze(self.teacher)
        self.teacher.eval()
        if self.rank == 0:
            print(f"Model has {sum(p.numel() for p in self.student.parameters()):,} parameters")
        self.ema = self.opt = self.critic_opt = None
        self.total_step_counter = 0
        self.max_steps = None  # optional cap on outer steps (plumbing runs)
        self.history = []

    def eval_core(self):
        return self.ema.ema_model  # the EMA of the student, a core already

    # ------------------------------------------------------------------ checkpoint
    def save(self):
        if self.rank != 0:
            return
        super().save({"model": self.student.state_dict(), "ema": self.ema.state_dict(), "opt": self.opt.state_dict(),
                      "critic": self.critic.state_dict(), "critic_opt": self.critic_opt.state_dict(),
                      "steps": self.total_step_counter})

    def load(self):
        ckpt = self.train_cfg.get("resume_ckpt")
        if not ckpt:
            return
        state = checkpoint_entries(super().load(ckpt))
        self.student.load_state_dict(state["model"])
        self.ema.load_state_dict(state["ema"])
        self.opt.load_state_dict(state["opt"])
        self.critic.load_state_dict(state["critic"])
        self.critic_opt.load_state_dict(state["critic_opt"])
        self.total_step_counter = int(state["steps"])

    # ------------------------------------------------------------------ training state
    def _optimizer(self, params, kwargs):
        kwargs = dict(kwargs or {})
        if "betas" in kwargs:
            kwargs["betas"] = tuple(kwargs["betas"])
        cls = FusedAdamW if self.train_cfg.opt == "AdamW" else getattr(torch.optim, self.train_cfg.opt)
        return cls(params, **kwargs)

    def make_rollouts(self):
        """the rollout manager the two phases hand to their losses"""
        raise NotImplementedError

    def prepare(self):
        """sf_vid_only.py:442-500: modules to the device, EMA, optimizers, reducers, checkpoint, data"""
        torch.cuda.set_device(self.local_rank)
        cfg = self.train_cfg
        self.teacher = self.teacher.cuda()
        self.student = self.student.cuda().train()
        self.critic = self.critic.cuda().train()
        if self.world_size > 1:  # identical weights on every rank (DDP's init broadcast)
            with torch.no_grad():
                for m in (self.teacher, self.student, self.critic):
                    for p in m.parameters():
                        dist.broadcast(p, 0)
        self.ema = EMA(self.student, beta=0.99, update_after_step=0, update_every=1)
        self.opt = self._optimizer(self.student.parameters(), cfg.opt_kwargs)
        self.critic_opt = self._optimizer(self.critic.parameters(), cfg.get("d_opt_kwargs") or cfg.opt_kwargs)
        self.reducer = GradReducer(self.student.parameters(), world_size=self.world_size)
        self.critic_reducer = GradReducer(self.critic.parameters(), world_size=self.world_size)
        self.load()
        self.accum = max(1, cfg.target_batch_size // cfg.batch_size // self.world_size)
        self.update_ratio = int(cfg.get("update_ratio") or 1)
        self.rollouts = self.make_rollouts()
        self.metrics = LogHelper()
        kw = dict(cfg.get("data_kwargs") or {})
        kw.setdefault("batch_columns", ["depth_latent", "mouse", "buttons"])
        self.batches = _Batches(get_loader(cfg.get("data_id") or "synthetic", cfg.batch_size,
                                           model_cfg=self.model_cfg, **kw))
        self.micro_per_step = (self.update_ratio + 1) * self.accum
        if cfg.get("seed") is not None:  # a resumed run reads on where the saved one stopped
            for _ in range(self.total_step_counter * self.micro_per_step):
                next(self.batches)
        self._micro = 0

    def micro_index(self):
        """the micro-step about to run, counted from the start of training"""
        return self.total_step_counter * self.micro_per_step + self._micro

    def get_batch(self):
        """the next (vid, mouse, btn) on the device, latents scaled; seeds the micro-step when asked to"""
        seed = self.train_cfg.get("seed")
        if seed is not None:
            s = int(seed) + 7919 * self.micro_index() + 104729 * self.rank
            torch.manual_seed(s)
            random.seed(s)
        self._micro += 1
        vid, mouse, btn = [t.cuda(non_blocking=True) for t in next(self.batches)[:3]]  # doc_id, if any, is unused
        return vid / self.train_cfg.vae_scale, mouse, btn

    def _step(self, model, opt, reducer):
        if self.train_cfg.get("grad_guard"):
            g_norm = self.guarded_step(opt, reducer, self.train_cfg.grad_clip_norm,
                                       name="critic" if model is self.critic else "student").norm
        else:
            g_norm = torch.nn.utils.clip_grad_norm_(model.parameters(), max_norm=self.train_cfg.grad_clip_norm)
            opt.step()
        reducer.zero_grad()
        return g_norm

    # ------------------------------------------------------------------ the two phases
    def critic_phase(self):
        raise NotImplementedError

    def student_phase(self):
        raise NotImplementedError

    def outer_step(self):
        self._micro = 0
        self.critic_phase()
        self.student_phase()
        self.ema.update()

    # ------------------------------------------------------------------ training loop
    def train(self):
        self.prepare()
        timer = Timer()
        timer.reset()
        sample_loader, sampler = self.eval_setup()
        while self.max_steps is None or len(self.history) < self.max_steps:
            self.outer_step()
            rec = self.metrics.pop()
            if self.train_cfg.get("grad_guard"):
                rec["skipped"] = self.skipped
            rec["time"] = timer.hit()
            timer.reset()
            if sampler is not None and self.total_step_counter % self.train_cfg.sample_interval == 0:
                ev = self.eval_step(sample_loader, sampler)
                gc.collect()
                torch.cuda.empty_cache()
                if ev:
                    rec.update(ev)
            rec["step"] = self.total_step_counter
            self.history.append(rec)
            if self.rank == 0:
                print(rec, flush=True)
            self.total_step_counter += 1
            if self.total_step_counter % self.train_cfg.save_interval == 0:
                self.save()
            self.barrier()
