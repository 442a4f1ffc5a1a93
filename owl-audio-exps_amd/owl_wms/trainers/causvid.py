"""CausVid rollouts and its two distillation losses (reference: owl_wms/trainers/causvid_vid_only.py:
RolloutManager 101-164, get_critic_loss 171-208, get_dmd_loss 210-309), for the video model (``game_rft``)
and the audio + video model (``game_rft_audio``).

The "rollout" is one teacher-forced training forward over the window: a random ``gen_mask_p`` of the
frames are noised to ts = 1 or 0.5 and denoised in one step (x0 = noisy - ts v), the others are noised to
``noise_prev`` as context and returned clean.  It needs no KV cache and no gradient through decode steps.
The critic learns the flow of these outputs; the student is pulled along critic - teacher (DMD), plus an
optional regression to the clean frames.  Both means run over every element of the window (frames off the
mask count as zeros), unlike trainers/self_forcing.py, which averages over the generated frames alone.
The trainer built on these is trainers/causvid_trainer.py (``causvid``).  On the GPU the element-wise
tails are the libowlk kernels of csrc/distill.hip (``fused``: self_forcing._use_kernels); the torch tails
stay for other devices and dtypes.

The audio + video form (its reference file is absent) is the same algorithm per modality, as GameRFTAudio's
loss is MSE(video) + MSE(audio): gen_mask, ts and the losses' ts are one per frame, shared; the rollout
draws z_video then z_audio, the losses ts, z_video, z_audio; every modality has its own normalizer, DMD,
regression and critic MSE, and the losses are the sums.  The teacher's unconditional branch is zero
controls for ``game_rft`` (causvid_vid_only.py:241-246) and ``has_controls`` all False for
``game_rft_audio`` (what its samplers use, sampling/av_window.py).

Differences from the reference, on purpose:
* every draw goes through a noise source (self_forcing.RolloutNoise), in the order gen_mask, ts, z;
* no wandb image logging;
* a rollout returns ``(out, mouse, btn, gen_mask, video)``; the reference's ``orig_video`` clone is the input.
"""
from collections import namedtuple

import torch
import torch.nn.functional as F

from .self_forcing import _CriticLossFn, _critic_tail, _per_frame, _use_kernels, RolloutNoise

Rollout = namedtuple("Rollout", "out v noisy ts_full gen_mask")
SUFFIXES = ("", "_audio")  # metric names per modality


def _forward(model, xs, ts, mouse, btn, uncond=False):
    """the model on one or two modalities -> the list of its velocities; ``uncond``: the unconditional branch"""
    if len(xs) == 1:
        if uncond:
            mouse, btn = torch.zeros_like(mouse), torch.zeros_like(btn)
        return [model(xs[0], ts, mouse, btn)]
    has_controls = torch.zeros(xs[0].shape[0], dtype=torch.bool, device=xs[0].device) if uncond else None
    return list(model(xs[0], xs[1], ts, mouse, btn, has_controls=has_controls))


def _mix(x, z, ts, gen_mask, noise_prev, fused):
    """x (1 - t) + z t, t = ts on the mask's frames (every frame without a mask), noise_prev elsewhere -> (noisy, t)"""
    if fused:
        from .. import kernels as K
        # noise_prev as the tensors' dtype holds it, so that both paths noise the context alike
        return K.causvid_mix(x, z, ts, gen_mask, torch.tensor(noise_prev, dtype=x.dtype).item())
    t = ts if gen_mask is None else torch.where(gen_mask, ts, torch.full_like(ts, noise_prev))
    e = _per_frame(t, x)
    return x * (1. - e) + z * e, t


def _x0(noisy, clean, v, ts_full, gen_mask, fused):
    if fused:
        from .. import kernels as K
        return K.causvid_x0(noisy, clean, v.detach(), ts_full, gen_mask)
    e = _per_frame(ts_full.to(noisy.dtype), noisy)
    return torch.where(_per_frame(gen_mask, noisy), noisy - v * e, clean)


class CausVidRollouts:
    """causvid_vid_only.py:101-164."""

    def __init__(self, model_cfg, noise_prev=0.2, gen_mask_p=0.25, noise_source=None):
        self.model_cfg = model_cfg
        self.noise_prev, self.gen_mask_p = float(noise_prev), float(gen_mask_p)
        self.noise_source = noise_source if noise_source is not None else RolloutNoise()

    def rollout(self, model, xs, mouse, btn, fused=False, tail_grad=True):
        """xs: [video] or [video, audio] -> Rollout of per-modality lists.  The model runs in the caller's
        grad mode; ``tail_grad`` False forms ``out`` without autograd (the fused generator loss differentiates
        with respect to ``v`` itself)."""
        video, noise = xs[0], self.noise_source
        b, n = video.shape[:2]
        with torch.no_grad():
            gen_mask = noise.rand((b, n), video.device) < self.gen_mask_p
            valid = torch.tensor([1.0, 0.5], device=video.device, dtype=video.dtype)
            ts = valid[noise.randint(0, 2, (b, n), video.device)]
            zs = [noise.randn_like(x) for x in xs]
            mixed = [_mix(x, z, ts, gen_mask, self.noise_prev, fused) for x, z in zip(xs, zs)]
            noisy, ts_full = [m[0] for m in mixed], mixed[0][1]
        v = _forward(model, noisy, ts_full.to(video.dtype), mouse, btn)
        grad = tail_grad and torch.is_grad_enabled() and any(t.requires_grad for t in v)
        with torch.set_grad_enabled(grad):
            out = [_x0(y, x, vi, ts_full, gen_mask, fused and not grad) for y, x, vi in zip(noisy, xs, v)]
        return Rollout(out, v, noisy, ts_full, gen_mask)

    def get_rollouts(self, model, video, mouse, btn, audio=None, fused=False):
        """-> (out, mouse, btn, gen_mask, video); with ``audio``, out and the clean input are (video, audio) pairs"""
        xs = [video] if audio is None else [video, audio]
        r = self.rollout(model, xs, mouse, btn, fused=fused)
        if audio is None:
            return r.out[0], mouse, btn, r.gen_mask, video
        return tuple(r.out), mouse, btn, r.gen_mask, (video, audio)


def _loss_draws(outs, noise, fused):
    """self_forcing._loss_draws per modality: ts = sigmoid(randn(b, n)), then one z and one noised tensor each"""
    x = outs[0]
    ts = noise.randn((x.shape[0], x.shape[1]), x.device, x.dtype).sigmoid()
    zs = [noise.randn_like(o) for o in outs]
    return ts, zs, [_mix(o, z, ts, None, 0.0, fused)[0] for o, z in zip(outs, zs)]


def _gen_tail(out, orig, noisy, ts, v_cond, v_uncond, v_critic, gen_mask, cfg_scale):
    """the reference's tail (causvid_vid_only.py:255-306) in torch -> (dmd, regression); v_uncond None is its
    cfg_scale == 1 branch"""
    with torch.no_grad():
        e = _per_frame(ts, out)
        v_teacher = v_cond if v_uncond is None else v_uncond + cfg_scale * (v_cond - v_uncond)
        mu_teacher = noisy - e * v_teacher
        mu_critic = noisy - e * v_critic
        normalizer = torch.abs(out - mu_teacher).mean(dim=list(range(1, out.dim())), keepdim=True)
        grad = torch.nan_to_num((mu_critic - mu_teacher) / normalizer, nan=0.0)
        target = (out.double() - grad.double()).detach()
    m = _per_frame(gen_mask, out)
    dmd = 0.5 * F.mse_loss(out.double() * m, target * m, reduction="mean")
    return dmd, F.mse_loss(out * m, orig * m, reduction="mean")


class _GenLossFn(torch.autograd.Function):
    """owlk_causvid_gen_loss on the student's velocity ``v`` (out = noisy - ts_full v): -> (dmd + w regression,
    dmd, regression).  The first carries the gradient -- backward scales the kept d / d v by the incoming
    one -- the two parts are for the log."""

    @staticmethod
    def forward(ctx, v, out, orig, noisy2, v_cond, v_uncond, v_critic, ts2, ts_full, gen_mask, cfg_scale, w):
        from .. import kernels as K
        if v.shape != v_cond.shape or v.dtype != v_cond.dtype:
            raise RuntimeError(f"causvid_gen_loss: the student's velocity ({tuple(v.shape)}, {v.dtype}) and the "
                               f"teacher's ({tuple(v_cond.shape)}, {v_cond.dtype}) must agree")
        losses, dv = K.causvid_gen_loss(out, orig, noisy2, v_cond, v_uncond, v_critic, ts2, ts_full, gen_mask,
                                        cfg_scale, w)
        ctx.save_for_backward(dv)
        dmd, reg = losses[0].clone(), losses[1].clone()
        ctx.mark_non_differentiable(dmd, reg)
        return dmd + w * reg, dmd, reg

    @staticmethod
    def backward(ctx, grad_gen, _grad_dmd, _grad_reg):
        dv, = ctx.saved_tensors
        return ((dv * grad_gen).to(dv.dtype),) + (None,) * 11


def _modalities(video, audio):
    return [video] if audio is None else [video, audio]


def get_critic_loss(student, critic, video, mouse, btn, rollouts, audio=None, noise_source=None, fused=None):
    """causvid_vid_only.py:171-208: the critic learns the flow of the student's rollout (no gradient to the
    student): mse of its velocity against z - out on the mask's frames, the others counting as zeros in the
    mean -- exactly self_forcing's critic tail (owlk_critic_loss on the GPU).  -> (loss, {name: part})."""
    noise = noise_source if noise_source is not None else rollouts.noise_source
    xs = _modalities(video, audio)
    use = _use_kernels(fused, video)
    with torch.no_grad():
        r = rollouts.rollout(student, xs, mouse, btn, fused=use)
        ts, zs, noisy = _loss_draws(r.out, noise, use)
    preds = _forward(critic, noisy, ts, mouse, btn)
    tail = _CriticLossFn.apply if use else _critic_tail
    parts = {"critic_loss" + s: tail(p, z, o, r.gen_mask) for s, p, z, o in zip(SUFFIXES, preds, zs, r.out)}
    return sum(parts.values()), parts


def get_gen_loss(student, critic, teacher, video, mouse, btn, rollouts, cfg_scale=1.5, regression_weight=0.0,
                 audio=None, noise_source=None, fused=None):
    """causvid_vid_only.py:210-309: the DMD loss of the student's rollout plus ``regression_weight`` times its
    regression to the clean frames.  The DMD direction is the critic's denoised estimate minus the teacher's
    (the teacher with classifier-free guidance; no unconditional pass at cfg_scale 1), scaled per sample by mean
    |out - teacher estimate|; both means run over every element.  The only gradient path is out -> the
    student's velocity, which owlk_causvid_gen_loss differentiates directly on the GPU.
    -> (loss, {name: part}) with the parts dmd_loss, regression_loss (and their _audio twins), gen_frames."""
    noise = noise_source if noise_source is not None else rollouts.noise_source
    xs = _modalities(video, audio)
    use = _use_kernels(fused, video)
    r = rollouts.rollout(student, xs, mouse, btn, fused=use, tail_grad=not use)
    with torch.no_grad():
        ts, zs, noisy = _loss_draws([o.detach() for o in r.out], noise, use)
        v_cond = _forward(teacher, noisy, ts, mouse, btn)
        v_uncond = _forward(teacher, noisy, ts, mouse, btn, uncond=True) if cfg_scale != 1.0 else [None] * len(xs)
        v_critic = _forward(critic, noisy, ts, mouse, btn)
    total, parts = 0.0, {}
    for i, s in enumerate(SUFFIXES[:len(xs)]):
        if use:
            gen, dmd, reg = _GenLossFn.apply(r.v[i], r.out[i], xs[i], noisy[i], v_cond[i], v_uncond[i], v_critic[i],
                                             ts, r.ts_full, r.gen_mask, float(cfg_scale), float(regression_weight))
        else:
            dmd, reg = _gen_tail(r.out[i], xs[i], noisy[i], ts, v_cond[i], v_uncond[i], v_critic[i], r.gen_mask,
                                 cfg_scale)
            gen = dmd + regression_weight * reg
        total = total + gen
        parts["dmd_loss" + s], parts["regression_loss" + s] = dmd.detach(), reg.detach()
    parts["gen_frames"] = r.gen_mask.sum()
    return total, parts
