"""CausVidTrainer (trainer id ``causvid``, the one the reference's configs/causvid.yml names; reference:
owl_wms/trainers/causvid_vid_only.py:311-560) for MI355X: CausVid distillation of a causal student from a
frozen teacher for the video model (``game_rft``) and the audio + video model (``game_rft_audio``), with a
critic that learns the flow of the student's teacher-forced one-step outputs (trainers/causvid.py has the
rollout and the two losses).

One outer step is the self-forcing trainer's (trainers/distill_base.py): ``update_ratio`` critic updates
(student frozen) of ``accum`` micro-steps of ``get_critic_loss / accum``, then one student update (critic
frozen) of ``accum`` micro-steps of ``get_gen_loss / accum`` = (dmd + ``regression_weight`` regression) /
accum, each with the ``train.grad_clip_norm`` clip (or ``guarded_step`` under ``train.grad_guard``), then the
EMA update (beta 0.99), the eval sampler every ``sample_interval`` and a checkpoint every ``save_interval``.
``train.gen_mask_p``, ``train.noise_prev`` and ``train.cfg_scale`` set the rollout's mask probability, the
context frames' noise level and the teacher's guidance.

Differences from the reference, on purpose (beyond those listed in sf_trainer.py, which hold here too):
* the student's optimizer steps once per accumulation window; the reference's (:529) sits inside the
  micro-step loop;
* the audio + video model trains on synthetic audio latents, drawn as AVRFTTrainer.batch_loss draws them
  and seeded by the micro-step, and is evaluated as AVRFTTrainer is (the samplers of AV_CORE_SAMPLERS);
* metrics: critic_loss, dmd_loss, regression_loss (each with an _audio twin on the audio + video model),
  g_norm, and gen_frames, the number of frames the student's micro-steps generated.
"""
import torch

from ..sampling import AV_CORE_SAMPLERS
from ..utils import freeze, unfreeze
from .causvid import CausVidRollouts, get_critic_loss, get_gen_loss
from .distill_base import DistillTrainer
from .rft_trainer import AVRFTTrainer, LatentEval


class CausVidTrainer(DistillTrainer):
    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self.av = self.model_cfg.model_id == "game_rft_audio"

    def make_rollouts(self):
        return CausVidRollouts(self.model_cfg, noise_prev=self.train_cfg.noise_prev,
                               gen_mask_p=self.train_cfg.gen_mask_p)

    def get_batch(self):
        """(vid, mouse, btn, audio): audio None for the video model, synthetic latents for the audio + video one"""
        index = self.micro_index()
        vid, mouse, btn = super().get_batch()
        audio = None
        if self.av:
            g = torch.Generator().manual_seed(index)
            audio = torch.randn(vid.shape[0], vid.shape[1], self.model_cfg.audio_channels, generator=g)
            audio = audio.cuda().to(vid.dtype)
        return vid, mouse, btn, audio

    def _log(self, parts):
        for k, v in parts.items():
            self.metrics.log(k, v if k == "gen_frames" else v / self.accum)

    # ------------------------------------------------------------------ the two phases (:500-530)
    def critic_phase(self):
        freeze(self.student)
        unfreeze(self.critic)
        for _ in range(self.update_ratio):
            for micro in range(self.accum):
                vid, mouse, btn, audio = self.get_batch()
                self.critic_reducer.begin(sync=micro == self.accum - 1)
                loss, parts = get_critic_loss(self.student, self.critic, vid, mouse, btn, self.rollouts, audio=audio)
                (loss / self.accum).backward()
                self.critic_reducer.finish()
                self._log(parts)
            self._step(self.critic, self.critic_opt, self.critic_reducer)

    def student_phase(self):
        freeze(self.critic)
        unfreeze(self.student)
        cfg = self.train_cfg
        for micro in range(self.accum):
            vid, mouse, btn, audio = self.get_batch()
            self.reducer.begin(sync=micro == self.accum - 1)
            loss, parts = get_gen_loss(self.student, self.critic, self.teacher, vid, mouse, btn, self.rollouts,
                                       cfg_scale=cfg.cfg_scale, regression_weight=cfg.regression_weight, audio=audio)
            (loss / self.accum).backward()
            self.reducer.finish()
            self._log(parts)
        self.metrics.log("g_norm", self._step(self.student, self.opt, self.reducer))

    # ------------------------------------------------------------------ eval
    def eval_setup(self):
        if self.av and self.train_cfg.get("sampler_id") not in AV_CORE_SAMPLERS:
            return None, None
        return LatentEval.eval_setup(self)

    def eval_step(self, sample_loader, sampler):
        if self.av:
            return AVRFTTrainer.eval_step(self, sample_loader, sampler)
        return LatentEval.eval_step(self, sample_loader, sampler)
