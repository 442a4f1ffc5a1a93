"""Self-forcing distillation: what the loss tails cost, and their share of one outer step.

(1) The DMD and critic loss tails (forward + backward to the rollout / the critic's output) on libowlk
    (csrc/distill.hip) against the torch tails of trainers/self_forcing.py (``fused=False``), at the
    reference's shape B8 N60 C128 8x8 in bf16.  Device events, warmed, the two versions alternated in
    one process; beside the fused time, the bytes the kernels move over the achievable HBM rate.
(2) One outer step of configs/dit_v4_sf.yml on synthetic data at batch 1 without accumulation (5 critic
    updates + 1 student update), and the share of it the tails take (the tails timed alone at that
    step's shape, B1 N60).

    python tools/sf_bench.py [--skip-step] [--steps 2]
"""
import argparse
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "owl-audio-exps_amd")]
import torch  # noqa: E402

from owl_wms.configs import Config  # noqa: E402
from owl_wms.trainers import get_trainer_cls  # noqa: E402
from owl_wms.trainers import self_forcing as SF  # noqa: E402

HBM_TBS = 6.3  # achievable HBM rate on MI355X (8.0 spec), TB/s
BF16 = torch.bfloat16


def tail_inputs(B, N=60, C=128, h=8, n_gen=50, seed=0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    r = lambda *s: torch.randn(*s, device="cuda", generator=g).to(BF16)  # noqa: E731
    x = dict(video=r(B, N, C, h, h), z=r(B, N, C, h, h), v_cond=r(B, N, C, h, h), v_uncond=r(B, N, C, h, h),
             v_critic=r(B, N, C, h, h), pred=r(B, N, C, h, h), ts=torch.rand(B, N, device="cuda", generator=g).to(BF16))
    x["noisy"] = SF.lerp_batched(x["video"], x["z"], x["ts"])
    x["mask"] = torch.zeros(B, N, dtype=torch.bool, device="cuda")
    x["mask"][:, N - n_gen:] = True  # the generated frames of a 50-frame rollout
    return x


def tails(x):
    """{name: callable}: each runs one tail forward and its backward"""
    def dmd(fused):
        v = x["video"].detach().requires_grad_()
        if fused:
            loss = SF._DMDLossFn.apply(v, x["noisy"], x["ts"], x["v_cond"], x["v_uncond"], x["v_critic"], x["mask"], 1.5)
        else:
            loss = SF._dmd_tail(v, x["noisy"], x["ts"], x["v_cond"], x["v_uncond"], x["v_critic"], x["mask"], 1.5)
        loss.backward()
        return loss

    def critic(fused):
        p = x["pred"].detach().requires_grad_()
        loss = SF._CriticLossFn.apply(p, x["z"], x["video"], x["mask"]) if fused else \
            SF._critic_tail(p, x["z"], x["video"], x["mask"])
        loss.backward()
        return loss

    return {"dmd fused": lambda: dmd(True), "dmd torch": lambda: dmd(False),
            "critic fused": lambda: critic(True), "critic torch": lambda: critic(False)}


def time_alternating(fns, warmup=5, rounds=20, inner=10):
    """median over rounds of the mean time of ``inner`` calls, in us; the versions take turns per round"""
    for f in fns.values():
        for _ in range(warmup):
            f()
    torch.cuda.synchronize()
    times = {k: [] for k in fns}
    for _ in range(rounds):
        for k, f in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(inner):
                f()
            e1.record()
            e1.synchronize()
            times[k].append(e0.elapsed_time(e1) * 1e3 / inner)
    return {k: sorted(v)[len(v) // 2] for k, v in times.items()}, {k: (min(v), max(v)) for k, v in times.items()}


def tail_bytes(x):
    """bytes the fused tails move, from the shapes (bf16 everywhere): the DMD pair reads video, noisy,
    v_cond, v_uncond (pass 1, every frame), v_cond, v_uncond, v_critic on the mask's frames and writes
    dvideo (pass 2); the critic pass reads pred, z, video on the mask's frames and writes dpred"""
    n = x["video"].numel()
    frac = x["mask"].float().mean().item()
    return {"dmd fused": 2 * n * (4 + 3 * frac + 1), "critic fused": 2 * n * (3 * frac + 1)}


def report_tails(tag, x):
    med, spread = time_alternating(tails(x))
    by = tail_bytes(x)
    print(f"loss tails, forward + backward, {tag} ({x['video'].numel() / 1e6:.2f} M elements, bf16):")
    for k, us in med.items():
        lo, hi = spread[k]
        extra = ""
        if k in by:
            extra = f"   {by[k] / 1e6:6.1f} MB moved, {by[k] / HBM_TBS / 1e6:5.1f} us at {HBM_TBS} TB/s"
        print(f"  {k:13s} {us:9.1f} us  (rounds {lo:.1f} .. {hi:.1f}){extra}", flush=True)
    for name in ("dmd", "critic"):
        print(f"  {name}: torch / fused = {med[name + ' torch'] / med[name + ' fused']:.2f}x")
    return med


def outer_step(steps):
    cfg = Config.from_yaml(os.path.join(REPO, "configs", "dit_v4_sf.yml"))
    cfg.train.teacher_cfg = os.path.join(REPO, cfg.train.teacher_cfg)
    cfg.train.batch_size = cfg.train.target_batch_size = 1  # batch 1, no accumulation
    cfg.train.sampler_id = None
    cfg.train.seed = 0
    torch.manual_seed(0)
    tr = get_trainer_cls(cfg.train.trainer_id)(cfg.train, cfg.wandb, cfg.model)
    tr.prepare()
    tr.outer_step()  # warm-up: first launches, allocator
    tr.metrics.pop()
    torch.cuda.synchronize()
    ts = []
    for _ in range(steps):
        tr.total_step_counter += 1
        t0 = time.time()
        tr.outer_step()
        rec = tr.metrics.pop()  # reads the losses back: ends in a device synchronise
        torch.cuda.synchronize()
        ts.append(time.time() - t0)
        print(f"  outer step: {ts[-1]:.3f} s  {rec}", flush=True)
    return sum(ts) / len(ts), tr.update_ratio


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--skip-step", action="store_true", help="only the loss tails (1)")
    ap.add_argument("--steps", type=int, default=2, help="timed outer steps after one warm-up step (2)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "sf_bench needs a GPU"
    print(f"device: {torch.cuda.get_device_name(0)}")
    report_tails("B8 N60 C128 8x8", tail_inputs(8))
    if not args.skip_step:
        med = report_tails("B1 N60 C128 8x8 (the step's shape)", tail_inputs(1))
        print("one outer step of configs/dit_v4_sf.yml, synthetic data, batch 1, no accumulation:")
        step_s, ratio = outer_step(args.steps)
        for kind in ("fused", "torch"):
            tail_s = (ratio * med[f"critic {kind}"] + med[f"dmd {kind}"]) * 1e-6
            print(f"  {ratio} critic + 1 dmd {kind} tails (timed alone): {tail_s * 1e3:.3f} ms = "
                  f"{100 * tail_s / step_s:.4f} % of the {step_s:.3f} s step (measured with the fused tails)")
