"""Time the gradient guard (owlk_grad_guard) on dit_v4's real bucket layout against torch's clip.

The model is built on the device and its GradReducer's flat buckets are filled with seeded values.  Three
passes over the same gradients alternate in one process after a warm-up, each call between its own pair
of device events:

    guard, norm only      kernels.grad_guard(flat)                  (what a Muon run pays)
    guard, active clip    kernels.grad_guard(flat, max_norm)        max_norm = 0.9 of the current norm
    torch, active clip    torch.nn.utils.clip_grad_norm_(model.parameters(), max_norm)   (the unguarded path)

and a device-to-device copy_ of the largest bucket gives the copy bandwidth (bytes read + written over
time) that the norm-only floor, bytes read / copy bandwidth, is taken from.  Every active clip takes a
tenth off the gradients, so the next one clips again and the norm stays far above the formula's 1e-6; the
norm is checked once, before any clip, against torch.linalg.vector_norm in float64.

    python tools/grad_guard_bench.py [--config configs/dit_v4.yml] [--rounds 20] [--warmup 3]
"""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "owl-audio-exps_amd")]
import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="configs/dit_v4.yml")
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("grad_guard_bench: no GPU; a time measured anywhere else says nothing")
    from owl_wms import kernels as K
    from owl_wms.configs import Config
    from owl_wms.models import get_model_cls
    from owl_wms.utils.grad_reducer import GradReducer

    cfg = Config.from_yaml(os.path.join(REPO, args.config))
    torch.manual_seed(0)
    model = get_model_cls(cfg.model.model_id)(cfg.model).cuda().train()
    red = GradReducer(model.parameters(), world_size=1)
    g = torch.Generator(device="cuda").manual_seed(1)
    for buf in red.flat:
        buf.normal_(0.0, 1e-3, generator=g)
    params = list(model.parameters())
    n_views = sum(1 for p in params if p.grad is not None)
    lengths = [b.numel() for b in red.flat]
    nbytes = 4 * sum(lengths)
    print(f"{args.config}: {len(red.flat)} buckets, {n_views} parameter views, {sum(lengths):,} fp32 gradients "
          f"({nbytes / 1e9:.3f} GB); bucket lengths {lengths}", flush=True)

    ref = float(torch.sqrt(sum(torch.linalg.vector_norm(b, dtype=torch.float64) ** 2 for b in red.flat)))
    st = K.grad_guard(red.flat).tolist()
    st2 = K.grad_guard(red.flat).tolist()
    rel = abs(st[0] - ref) / ref
    print(f"norm: guard {st[0]!r}  float64 {ref!r}  rel err {rel:.3e}  finite {st[2]}  coef {st[1]}  "
          f"second call equal: {st == st2}", flush=True)

    big = max(red.flat, key=lambda b: b.numel())
    dst = torch.empty_like(big)
    cur = [st[0]]  # the current norm, followed on the host: every active clip scales it by 0.9

    def guard_norm():
        K.grad_guard(red.flat)

    def guard_clip():
        cur[0] *= 0.9
        K.grad_guard(red.flat, cur[0])

    def torch_clip():
        cur[0] *= 0.9
        torch.nn.utils.clip_grad_norm_(params, max_norm=cur[0])

    def copy():
        dst.copy_(big)

    passes = {"guard_norm": guard_norm, "guard_clip": guard_clip, "torch_clip": torch_clip, "copy": copy}
    ms = {k: [] for k in passes}
    for r in range(args.warmup + args.rounds):
        for k, fn in passes.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            if r >= args.warmup:
                ms[k].append(e0.elapsed_time(e1))
    end = K.grad_guard(red.flat).tolist()
    print(f"after {2 * (args.warmup + args.rounds)} active clips: norm {end[0]!r}, followed on the host "
          f"{cur[0]!r}, finite {end[2]}", flush=True)

    med = {k: statistics.median(v) for k, v in ms.items()}
    for k, v in ms.items():
        print(f"{k:11s} median {med[k]:8.3f} ms  min {min(v):8.3f}  max {max(v):8.3f}  (n = {len(v)})")
    copy_bw = 2 * 4 * big.numel() / (med["copy"] * 1e-3)  # bytes read + written per second
    floor_ms = nbytes / copy_bw * 1e3
    res = {"config": args.config, "buckets": len(red.flat), "views": n_views, "grad_bytes": nbytes,
           "norm_rel_err": rel, "copy_GBps": copy_bw / 1e9, "norm_floor_ms": floor_ms,
           "guard_norm_ms": med["guard_norm"], "guard_norm_over_floor": med["guard_norm"] / floor_ms,
           "guard_norm_GBps": nbytes / (med["guard_norm"] * 1e-3) / 1e9,
           "guard_clip_ms": med["guard_clip"], "torch_clip_ms": med["torch_clip"],
           "torch_over_guard_clip": med["torch_clip"] / med["guard_clip"]}
    print(f"copy bandwidth {copy_bw / 1e9:.0f} GB/s (read + written, one {4 * big.numel() / 1e6:.0f} MB bucket); "
          f"norm-only floor {floor_ms:.3f} ms; guard norm-only {med['guard_norm']:.3f} ms = "
          f"{res['guard_norm_over_floor']:.2f} x floor ({res['guard_norm_GBps']:.0f} GB/s read)")
    print(f"active clip: guard {med['guard_clip']:.3f} ms, torch {med['torch_clip']:.3f} ms "
          f"(torch / guard = {res['torch_over_guard_clip']:.2f})")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
