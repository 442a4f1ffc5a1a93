"""Self-forcing rollouts and the two distillation losses (reference: owl_wms/trainers/sf_vid_only.py:
RolloutManager 112-225, get_critic_loss 229-260, get_dmd_loss 262-349).

A rollout caches a context window without gradient, then generates frames one at a time against the
KV cache; the LAST Euler step of each frame carries a gradient through the decode step (the
differentiable KV-cache decode block, nn/fused.DiTBlockFn with a decode geometry), everything else runs
without one.  The trainer built on these is trainers/sf_trainer.py (``sforce_vid``).  On the GPU the two
losses' element-wise tails are the libowlk kernels of csrc/distill.hip (``fused``), one deterministic
fp32 pass each; the torch tails stay for other devices and dtypes.

Differences from the reference, on purpose:
* no "warmup call" before the context pass (sf_vid_only.py:154): it works around autocast's
  weight-cast cache, which this path does not have (parameters are cast through a version-keyed cache);
* the per-frame timestep multiplies the velocity as ``ts[:, :, None, None, None]`` -- the reference
  multiplies the [b, 1] tensor directly, which broadcasts against the trailing (h, w) axes and only
  works when b is 1 or equals h; the value (ts = 1 on the last step) is the same;
* no wandb image logging in the DMD loss;
* every ``randn`` draw goes through a noise source (``RolloutNoise`` by default: ``torch.randn_like`` /
  ``torch.randn`` in the reference's order), so parity tests can inject the draws.
"""
import random

import torch
import torch.distributed as dist
import torch.nn.functional as F

from ..nn.kv_cache import KVCache
from ..utils import batch_permute_to_length


class RolloutNoise:
    """Default noise source: fresh draws on the input's device, in the reference's order."""

    def randn_like(self, x):
        return torch.randn_like(x)

    def randn(self, shape, device, dtype):
        return torch.randn(*shape, device=device, dtype=dtype)

    def rand(self, shape, device, dtype=torch.float32):
        return torch.rand(*shape, device=device, dtype=dtype)

    def randint(self, low, high, shape, device):
        return torch.randint(low, high, tuple(shape), device=device, dtype=torch.long)


class InjectedRolloutNoise:
    """Parity runs: replay pre-drawn tensors, one per draw, in call order (as models/flow.py's
    InjectedNoise does for the training loss)."""

    def __init__(self, draws):
        self.draws, self.i = list(draws), 0

    def _next(self, shape, device, dtype):
        t = self.draws[self.i]
        self.i += 1
        assert tuple(t.shape) == tuple(shape), f"injected draw {self.i - 1}: {tuple(t.shape)} != {tuple(shape)}"
        return t.to(device=device, dtype=dtype)

    def randn_like(self, x):
        return self._next(x.shape, x.device, x.dtype)

    def randn(self, shape, device, dtype):
        return self._next(shape, device, dtype)

    def rand(self, shape, device, dtype=torch.float32):
        return self._next(shape, device, dtype)

    def randint(self, low, high, shape, device):
        return self._next(shape, device, torch.long)


def _per_frame(t, like=None):
    """t [b, n] against a [b, n, c, h, w] video, or against ``like`` [b, n, ...] (the audio latents are [b, n, c])"""
    return t[:, :, None, None, None] if like is None else t.reshape(t.shape + (1,) * (like.dim() - 2))


def lerp_batched(x, z, t):
    """x (1 - t) + z t with t [b, n] per frame (sf_vid_only.py:86-88)."""
    t = _per_frame(t)
    return x * (1. - t) + z * t


class RolloutManager:
    """sf_vid_only.py:112-225.  ``get_rollouts`` returns the last ``window`` frames of [context |
    generated], the controls for them and a mask that is True on the generated frames (the only
    ones that carry a gradient)."""

    def __init__(self, model_cfg, min_rollout_frames=8, rollout_steps=1, noise_source=None):
        self.model_cfg = model_cfg
        self.min_rollout_frames = min_rollout_frames
        self.rollout_steps = rollout_steps
        self.noise_source = noise_source if noise_source is not None else RolloutNoise()

    def get_rollouts(self, model, video, mouse, btn):
        core = model.module if hasattr(model, "module") else model
        noise = self.noise_source
        kv_cache = KVCache(self.model_cfg)
        kv_cache.reset(video.shape[0])

        window = video.shape[1]
        n_roll = self.min_rollout_frames
        if dist.is_available() and dist.is_initialized():  # every rank generates the same number of frames
            n = torch.tensor(n_roll, device=video.device)
            dist.broadcast(n, src=0)
            n_roll = int(n.item())

        # controls for the frames past the window: batch-permuted copies of the given ones
        ext_mouse, ext_btn = batch_permute_to_length(mouse, btn, window + n_roll)

        # ---- the context window into the cache, clean (ts = 0), no gradient
        ts = torch.zeros_like(video[:, :, 0, 0, 0])
        with torch.no_grad():
            kv_cache.enable_cache_updates()
            model(video, ts, mouse, btn, kv_cache=kv_cache)
            kv_cache.disable_cache_updates()

        gen_mask = torch.zeros(video.shape[0], window + n_roll, dtype=torch.bool, device=video.device)
        gen_mask[:, window:] = True

        core.transformer.enable_decoding()
        try:
            for f in range(n_roll):
                ts_1 = torch.ones_like(video[:, 0:1, 0, 0, 0])
                frame = noise.randn_like(video[:, 0:1])
                mouse_1, btn_1 = ext_mouse[:, window + f:window + f + 1], ext_btn[:, window + f:window + f + 1]

                # a random number of Euler steps of size 1 / rollout_steps; the last one jumps to ts = 0
                # (frame - ts v) and is the only one with a gradient
                n_steps = random.randint(1, self.rollout_steps)
                dt = 1. / self.rollout_steps
                for step in range(n_steps - 1):
                    with torch.no_grad():
                        v = model(frame, ts_1, mouse_1, btn_1, kv_cache=kv_cache)
                        frame = frame - dt * v
                        ts_1 = ts_1 - dt
                v = model(frame, ts_1, mouse_1, btn_1, kv_cache=kv_cache)
                frame = frame - _per_frame(ts_1) * v
                ts_1 = torch.zeros_like(ts_1)

                # the clean frame joins the cache, the oldest frame leaves it
                with torch.no_grad():
                    kv_cache.enable_cache_updates()
                    model(frame, ts_1, mouse_1, btn_1, kv_cache=kv_cache)
                    kv_cache.disable_cache_updates()
                    kv_cache.truncate(1, front=False)

                video = torch.cat([video, frame.to(video.dtype)], dim=1)
        finally:
            core.transformer.disable_decoding()

        return video[:, -window:], ext_mouse[:, -window:], ext_btn[:, -window:], gen_mask[:, -window:]


def _loss_draws(video, noise):
    """ts = sigmoid(randn(b, n)) and the noised video (the two draws both losses make, in this order)"""
    ts = noise.randn((video.shape[0], video.shape[1]), video.device, video.dtype).sigmoid()
    z = noise.randn_like(video)
    return ts, z, lerp_batched(video, z, ts)


def _critic_tail(pred, z, video, grad_mask):
    """the reference's tail (sf_vid_only.py:250-260) in torch, in the tensors' own dtype"""
    m = _per_frame(grad_mask, pred)
    return F.mse_loss(pred * m, (z - video) * m)


def _dmd_tail(video, noisy, ts, v_cond, v_uncond, v_critic, grad_mask, cfg_scale):
    """the reference's tail (sf_vid_only.py:300-349) in torch: v_uncond None is its cfg_scale == 1 branch"""
    with torch.no_grad():
        v_teacher = v_cond if v_uncond is None else v_uncond + cfg_scale * (v_cond - v_uncond)
        mu_teacher = noisy - _per_frame(ts) * v_teacher
        mu_critic = noisy - _per_frame(ts) * v_critic
        normalizer = torch.abs(video - mu_teacher).mean(dim=[1, 2, 3, 4], keepdim=True)
        grad = torch.nan_to_num((mu_critic - mu_teacher) / normalizer, nan=0.0)
        target = (video.double() - grad.double()).detach()[grad_mask]
    return 0.5 * F.mse_loss(video[grad_mask].double(), target, reduction="mean")


class _CriticLossFn(torch.autograd.Function):
    """owlk_critic_loss: the loss and d loss / d pred from one pass; backward scales the kept gradient by
    the incoming one on the device"""

    @staticmethod
    def forward(ctx, pred, z, video, grad_mask):
        from .. import kernels as K
        loss, dpred = K.critic_loss(pred, z, video, grad_mask)
        ctx.save_for_backward(dpred)
        return loss

    @staticmethod
    def backward(ctx, grad_output):
        dpred, = ctx.saved_tensors
        return dpred * grad_output, None, None, None


class _DMDLossFn(torch.autograd.Function):
    """owlk_dmd_loss: the loss and d loss / d video (zero off the generated frames) in two passes"""

    @staticmethod
    def forward(ctx, video, noisy, ts, v_cond, v_uncond, v_critic, grad_mask, cfg_scale):
        from .. import kernels as K
        loss, dvideo = K.dmd_loss(video, noisy, v_cond, v_uncond, v_critic, ts, grad_mask, cfg_scale)
        ctx.save_for_backward(dvideo)
        return loss

    @staticmethod
    def backward(ctx, grad_output):
        dvideo, = ctx.saved_tensors
        return (dvideo * grad_output).to(dvideo.dtype), None, None, None, None, None, None, None


def _use_kernels(fused, video):
    """fused=None: the libowlk tails for a CUDA rollout in bf16 or fp32, the torch tails otherwise (the
    CPU formula tests run in float64); False forces torch; True insists on the kernels"""
    ok = video.is_cuda and video.dtype in (torch.bfloat16, torch.float32)
    if fused and not ok:
        raise RuntimeError(f"fused distillation losses need a CUDA rollout in bf16 or fp32 (got {video.device}, "
                           f"{video.dtype})")
    return ok if fused is None else bool(fused)


def get_critic_loss(student, critic, video, mouse, btn, rollout_manager, noise_source=None, fused=None):
    """sf_vid_only.py:229-260: the critic learns the flow of the student's rollouts (no gradient to
    the student): mse of its velocity against z - video on the generated frames; the masked-out
    frames count as zeros in the mean.  The tail is owlk_critic_loss on the GPU (``fused``: _use_kernels)."""
    noise = noise_source if noise_source is not None else rollout_manager.noise_source
    with torch.no_grad():
        video, mouse, btn, grad_mask = rollout_manager.get_rollouts(model=student, video=video, mouse=mouse, btn=btn)
        ts, z, noisy = _loss_draws(video, noise)
    pred = critic(noisy, ts, mouse, btn)
    if _use_kernels(fused, video):
        return _CriticLossFn.apply(pred, z, video, grad_mask)
    return _critic_tail(pred, z, video, grad_mask)


def get_dmd_loss(student, critic, teacher, video, mouse, btn, rollout_manager, cfg_scale=1.5, noise_source=None,
                 fused=None):
    """sf_vid_only.py:262-349: distribution-matching loss of the student's rollout.  The gradient
    direction (critic's denoised estimate - teacher's, the teacher with classifier-free guidance), scaled
    per sample by mean |video - teacher estimate|, becomes a fixed double-precision target video - grad;
    0.5 mse against it over the generated frames then has exactly that gradient.  On the GPU
    (``fused``: _use_kernels) owlk_dmd_loss forms that loss and gradient directly, in fp32 from the
    loaded values."""
    noise = noise_source if noise_source is not None else rollout_manager.noise_source
    video, mouse, btn, grad_mask = rollout_manager.get_rollouts(model=student, video=video, mouse=mouse, btn=btn)
    with torch.no_grad():
        ts, z, noisy = _loss_draws(video, noise)
        v_cond = teacher(noisy, ts, mouse, btn)
        v_uncond = None
        if cfg_scale != 1.0:
            v_uncond = teacher(noisy, ts, torch.zeros_like(mouse), torch.zeros_like(btn))
        v_critic = critic(noisy, ts, mouse, btn)
    if _use_kernels(fused, video):
        return _DMDLossFn.apply(video, noisy, ts, v_cond, v_uncond, v_critic, grad_mask, float(cfg_scale))
    return _dmd_tail(video, noisy, ts, v_cond, v_uncond, v_critic, grad_mask, cfg_scale)
