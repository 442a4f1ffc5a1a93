"""SelfForceTrainer (reference: owl_wms/trainers/sf_vid_only.py:351-589, trainer id ``sforce_vid``) for
MI355X: self-forcing distillation of a causal student from a frozen teacher, with a critic that learns
the flow of the student's own rollouts (trainers/self_forcing.py has the rollout and the two losses).

One outer step, as in the reference: ``update_ratio`` critic updates (student frozen), each ``accum``
micro-steps of ``get_critic_loss / accum``, clip-norm ``train.grad_clip_norm`` (10) and an optimizer step;
then one student update (critic frozen) of ``accum`` micro-steps of ``get_dmd_loss(cfg_scale=1.5) / accum``,
the same clip and a step; then the EMA update, logging, the eval sampler every ``sample_interval``
(RFTTrainer's eval path, on the EMA core) and a checkpoint every ``save_interval``.  ``max_steps`` counts
outer steps.

Differences from the reference, on purpose:
* RolloutManager gets ``min_rollout_frames`` and ``rollout_steps`` by keyword; the reference passes them
  positionally in swapped order (sf_vid_only.py:496 against :113);
* the student's optimizer steps once per accumulation window, like the critic's; in the reference the
  step sits inside the micro-step loop (:563), so only the last micro-step's gradient is whole;
* no GradScaler (gradients are fp32 buckets, utils/grad_reducer.py) and no autocast (the cores run
  their own bf16 kernels); ``load`` ignores a reference checkpoint's ``scaler`` / ``critic_scaler``.  What
  went with the scaler, the skipped optimizer step on an inf / NaN gradient (sf_vid_only.py:503-508), is back
  behind ``train.grad_guard``: norm, clip and finite check in one pass over the buckets, a non-finite
  critic or student gradient skips that optimizer step only (BaseTrainer.guarded_step); off by default;
* no DDP wrapper (GradReducer, one per trained model), no VAE decoder, no wandb: metrics go to
  ``self.history`` and stdout, eval returns summary statistics of the sampled latents;
* a ``None`` checkpoint path leaves the module's own initialisation (plumbing runs and tests); a
  ``None`` ``teacher_cfg`` gives the teacher the student's architecture;
* the batch's ``doc_id`` is ignored: a KV-cache rollout has no document mask (the cache holds one
  sequence per sample), as in the reference, whose loader yields no doc_id at all;
* optional ``train.seed`` seeds torch's generator and Python's ``random`` (the rollout's step counts) per
  micro-step and, on resume, skips the batches already consumed, so a resumed run is bit-identical to
  an uninterrupted one.

What this trainer shares with the CausVid one -- the three cores, the optimizers and reducers, the batch
iterator, seeding, resume, the checkpoint keys and the outer loop -- is trainers/distill_base.py.
"""
from ..utils import freeze, unfreeze
from .distill_base import CKPT_KEYS, DistillTrainer, checkpoint_entries  # noqa: F401  (the checkpoint's interface)
from .self_forcing import RolloutManager, get_critic_loss, get_dmd_loss


class SelfForceTrainer(DistillTrainer):
    def make_rollouts(self):
        return RolloutManager(self.model_cfg, min_rollout_frames=self.train_cfg.min_rollout_frames,
                              rollout_steps=self.train_cfg.rollout_steps)

    # ------------------------------------------------------------------ the two phases (:517-564)
    def critic_phase(self):
        freeze(self.student)
        unfreeze(self.critic)
        for _ in range(self.update_ratio):
            for micro in range(self.accum):
                vid, mouse, btn = self.get_batch()
                self.critic_reducer.begin(sync=micro == self.accum - 1)
                loss = get_critic_loss(self.student, self.critic, vid, mouse, btn, self.rollouts) / self.accum
                loss.backward()
                self.critic_reducer.finish()
                self.metrics.log("critic_loss", loss)
            self._step(self.critic, self.critic_opt, self.critic_reducer)

    def student_phase(self):
        freeze(self.critic)
        unfreeze(self.student)
        for micro in range(self.accum):
            vid, mouse, btn = self.get_batch()
            self.reducer.begin(sync=micro == self.accum - 1)
            loss = get_dmd_loss(self.student, self.critic, self.teacher, vid, mouse, btn, self.rollouts,
                                cfg_scale=1.5) / self.accum
            loss.backward()
            self.reducer.finish()
            self.metrics.log("dmd_loss", loss)
        self.metrics.log("g_norm", self._step(self.student, self.opt, self.reducer))
