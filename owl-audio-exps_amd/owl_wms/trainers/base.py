"""BaseTrainer (reference: owl_wms/trainers/base.py:10-75) without the wandb dependency."""
import os

import torch
import torch.distributed as dist


class BaseTrainer:
    def __init__(self, train_cfg, logging_cfg, model_cfg, global_rank=0, local_rank=0, world_size=1):
        self.rank, self.local_rank, self.world_size = global_rank, local_rank, world_size
        self.train_cfg, self.logging_cfg, self.model_cfg = train_cfg, logging_cfg, model_cfg
        self.device = f"cuda:{local_rank}"
        self.skipped, self._skip_runs = 0, {}  # train.grad_guard: skipped optimizer steps, and in a row per name

    def barrier(self):
        if self.world_size > 1:
            dist.barrier()

    def guarded_step(self, opt, reducer, max_norm=None, name="model"):
        """The optimizer step under ``train.grad_guard``: one pass over the reducer's buckets gives the
        gradient norm (clipped to ``max_norm`` when given) and whether it is finite; a non-finite gradient
        skips ``opt.step()`` and leaves the optimizer's state untouched, as GradScaler.step does in the
        reference (sf_vid_only.py:503-508).  The caller zeroes the gradients and runs the scheduler and the
        EMA either way.  ``self.skipped`` counts the skips; more than ``train.max_consecutive_skips`` of
        ``name``'s steps in a row raise.  -> the GuardResult."""
        res = reducer.grad_guard(max_norm)
        runs = self._skip_runs
        if res.finite:
            opt.step()
            runs[name] = 0
            return res
        self.skipped += 1
        runs[name] = runs.get(name, 0) + 1
        if self.rank == 0:
            print(f"grad_guard: step {self.total_step_counter}: non-finite {name} gradient (norm {res.norm}), "
                  f"optimizer step skipped ({self.skipped} so far)", flush=True)
        limit = self.train_cfg.get("max_consecutive_skips")
        if limit is not None and runs[name] > int(limit):
            raise RuntimeError(f"grad_guard: step {self.total_step_counter}: {runs[name]} {name} optimizer steps "
                               f"skipped in a row (max_consecutive_skips = {limit})")
        return res

    def save(self, save_dict):
        """base.py:61-72: checkpoint_dir/step_N.pt (+ EMA-only weights to output_path)."""
        os.makedirs(self.train_cfg.checkpoint_dir, exist_ok=True)
        torch.save(save_dict, os.path.join(self.train_cfg.checkpoint_dir, f"step_{self.total_step_counter}.pt"))
        out = getattr(self.train_cfg, "output_path", None)
        if "ema" in save_dict and out:
            prefix = "ema_model."
            d = {k[len(prefix):]: v for k, v in save_dict["ema"].items() if k.startswith(prefix)}
            os.makedirs(out, exist_ok=True)
            torch.save(d, os.path.join(out, f"step_{self.total_step_counter}.pt"))

    def load(self, path):
        return torch.load(path, map_location="cpu", weights_only=True)
