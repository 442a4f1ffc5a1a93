"""CausVid distillation: what its three fused tails cost, and their share of one outer step.

(1) owlk_causvid_mix, owlk_causvid_x0 and owlk_causvid_gen_loss (forward + backward to the student's velocity)
    against their torch forms in trainers/causvid.py (``fused=False``), at each config's shape in bf16:
    configs/dit_v4_causvid.yml B8 N60 C128 8x8 and configs/mmdit_v2_causvid.yml B16 N16 (video C128 8x8 and
    audio C64).  Device events, warmed, the two versions alternated in one process; median and range over the
    rounds, and beside the fused time the bytes the kernels move over the achievable HBM rate.
(2) One outer step of each config on synthetic data at batch 1 without accumulation (5 critic updates + 1
    student update), and the share of it the tails take (timed alone at that step's shape).

    python tools/causvid_bench.py [--skip-step] [--steps 2]
"""
import argparse
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "owl-audio-exps_amd")]
import torch  # noqa: E402

from owl_wms.configs import Config  # noqa: E402
from owl_wms.trainers import causvid as CV  # noqa: E402
from owl_wms.trainers import get_trainer_cls  # noqa: E402

HBM_TBS = 6.3  # achievable HBM rate on MI355X (8.0 spec), TB/s
BF16 = torch.bfloat16
P, NOISE_PREV, CFG, W = 0.25, 0.2, 1.5, 0.0  # the configs' values


def tail_inputs(B, N, frame, seed=0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    r = lambda: torch.randn(B, N, *frame, device="cuda", generator=g).to(BF16)  # noqa: E731
    x = {k: r() for k in ("clean", "z", "v", "orig", "noisy2", "v_cond", "v_uncond", "v_critic")}
    x["mask"] = torch.rand(B, N, device="cuda", generator=g) < P
    x["ts"] = torch.tensor([1.0, 0.5], device="cuda")[torch.randint(0, 2, (B, N), device="cuda", generator=g)]
    x["ts2"] = torch.rand(B, N, device="cuda", generator=g)
    x["noisy"], x["ts_full"] = CV._mix(x["clean"], x["z"], x["ts"], x["mask"], NOISE_PREV, True)
    x["out"] = CV._x0(x["noisy"], x["clean"], x["v"], x["ts_full"], x["mask"], True)
    return x


def tails(x):
    """{name: callable}: mix and x0 run forward; gen runs forward and the backward to v"""
    def gen(fused):
        v = x["v"].detach().requires_grad_()
        if fused:
            loss = CV._GenLossFn.apply(v, x["out"], x["orig"], x["noisy2"], x["v_cond"], x["v_uncond"], x["v_critic"],
                                       x["ts2"], x["ts_full"], x["mask"], CFG, W)[0]
        else:  # the torch form differentiates through out = noisy - ts_full v
            out = CV._x0(x["noisy"], x["clean"], v, x["ts_full"], x["mask"], False)
            dmd, reg = CV._gen_tail(out, x["orig"], x["noisy2"], x["ts2"].to(BF16), x["v_cond"], x["v_uncond"],
                                    x["v_critic"], x["mask"], CFG)
            loss = dmd + W * reg
        loss.backward()
        return loss

    fns = {}
    for kind, fused in (("fused", True), ("torch", False)):
        ts, tf = (x["ts"], x["ts_full"]) if fused else (x["ts"].to(BF16), x["ts_full"].to(BF16))
        fns[f"mix {kind}"] = lambda f=fused, ts=ts: CV._mix(x["clean"], x["z"], ts, x["mask"], NOISE_PREV, f)
        fns[f"x0 {kind}"] = lambda f=fused, tf=tf: CV._x0(x["noisy"], x["clean"], x["v"], tf, x["mask"], f)
        fns[f"gen {kind}"] = lambda f=fused: gen(f)
    return fns


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
    """bytes the fused tails move, from the shapes (bf16): mix reads x, z and writes noisy; x0 reads one of
    (noisy, v) / clean per frame -- two tensors on the mask's frames, one elsewhere -- and writes out; the gen
    pair reads out, noisy2, v_cond, v_uncond (pass 1, every frame), out, orig, v_cond, v_uncond, v_critic on the
    mask's frames and writes dv (pass 2)"""
    n = x["clean"].numel()
    frac = x["mask"].float().mean().item()
    return {"mix fused": 2 * n * 3, "x0 fused": 2 * n * (1 + frac + 1), "gen fused": 2 * n * (4 + 5 * frac + 1)}


def report_tails(tag, x):
    med, spread = time_alternating(tails(x))
    by = tail_bytes(x)
    print(f"tails, {tag} ({x['clean'].numel() / 1e6:.3f} M elements, bf16, {int(x['mask'].sum())} of "
          f"{x['mask'].numel()} frames on the mask):")
    for k, us in med.items():
        lo, hi = spread[k]
        extra = f"   {by[k] / 1e6:6.1f} MB moved, {by[k] / HBM_TBS / 1e6:5.1f} us at {HBM_TBS} TB/s" if k in by else ""
        print(f"  {k:10s} {us:9.1f} us  (rounds {lo:.1f} .. {hi:.1f}){extra}", flush=True)
    for name in ("mix", "x0", "gen"):
        print(f"  {name}: torch / fused = {med[name + ' torch'] / med[name + ' fused']:.2f}x")
    return med


def outer_step(config, steps):
    cfg = Config.from_yaml(os.path.join(REPO, "configs", config))
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
    ratio = tr.update_ratio
    del tr
    torch.cuda.empty_cache()
    return sum(ts) / len(ts), ratio


def report_step(config, steps, meds):
    """a critic micro-step runs mix, x0, mix (and the critic tail, self-forcing's); a student micro-step mix, mix,
    gen (+ x0 fused, which the torch gen form contains) -- per modality"""
    print(f"one outer step of configs/{config}, synthetic data, batch 1, no accumulation:")
    step_s, ratio = outer_step(config, steps)
    for kind in ("fused", "torch"):
        us = 0.0
        for med in meds:
            critic = 2 * med[f"mix {kind}"] + med[f"x0 {kind}"]
            student = 2 * med[f"mix {kind}"] + med[f"gen {kind}"] + (med["x0 fused"] if kind == "fused" else 0.0)
            us += ratio * critic + student
        print(f"  the CausVid {kind} tails of {ratio} critic + 1 student micro-steps (timed alone): {us * 1e-3:.3f} ms "
              f"= {100 * us * 1e-6 / step_s:.4f} % of the {step_s:.3f} s step (measured with the fused tails)")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--skip-step", action="store_true", help="only the tails (1)")
    ap.add_argument("--steps", type=int, default=2, help="timed outer steps after one warm-up step (2)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "causvid_bench needs a GPU"
    print(f"device: {torch.cuda.get_device_name(0)}")
    report_tails("dit_v4_causvid B8 N60 C128 8x8", tail_inputs(8, 60, (128, 8, 8)))
    report_tails("mmdit_v2_causvid B16 N16 video C128 8x8", tail_inputs(16, 16, (128, 8, 8)))
    report_tails("mmdit_v2_causvid B16 N16 audio C64", tail_inputs(16, 16, (64,)))
    if not args.skip_step:
        v60 = report_tails("B1 N60 C128 8x8 (dit_v4_causvid's step)", tail_inputs(1, 60, (128, 8, 8)))
        report_step("dit_v4_causvid.yml", args.steps, [v60])
        v16 = report_tails("B1 N16 C128 8x8 (mmdit_v2_causvid's step, video)", tail_inputs(1, 16, (128, 8, 8)))
        a16 = report_tails("B1 N16 C64 (mmdit_v2_causvid's step, audio)", tail_inputs(1, 16, (64,)))
        report_step("mmdit_v2_causvid.yml", args.steps, [v16, a16])
