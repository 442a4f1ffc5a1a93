"""Multi-session streaming (sampling/stream_pool.py StreamPool: n_slots sessions in one batch on per-slot ring
state) against one FrameStream session (B = 1) at the same settings: wall ms per tick and generated frames per
second per card, every slot live, the whole tick / frame captured (graphed="frame"), alternated in one process
on a config's model with weights as initialised.

    python tools/stream_pool_bench.py [--config configs/dit_v4.yml] [--ctx 8] [--cached 30] [--ticks 24]
                                      [--steps 16] [--cfgs 1.0 1.3] [--slots 1 2 4 8] [--rounds 3]

Every run opens its sessions with --ctx context frames (different data and seeds per slot), runs until the ring
holds --cached frames and then --ticks more.  Every step() is timed on the host with a synchronize after it;
reported per round is the median over the steady-state ticks (tick 0, which runs eagerly, tick 1, which
captures, and the ticks before the ring is full left out), then the median and range over the rounds.  The
positions stay inside the RoPE table, so no run rebases.

The one condition: StreamPool(n_slots = 1) must not tax a single session -- its median per tick has to lie
within the min - max spread of the FrameStream rounds of the same run and CFG scale.  The verdict is printed
with both numbers, whichever way it falls.
"""
import argparse
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "owl-audio-exps_amd")]
import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="configs/dit_v4.yml")
    ap.add_argument("--ctx", type=int, default=8)
    ap.add_argument("--cached", type=int, default=30, help="max_cached_frames of every stream")
    ap.add_argument("--ticks", type=int, default=24, help="steady-state ticks per run")
    ap.add_argument("--steps", type=int, default=16)
    ap.add_argument("--cfgs", type=float, nargs="+", default=[1.0, 1.3])
    ap.add_argument("--slots", type=int, nargs="+", default=[1, 2, 4, 8])
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "stream_pool_bench needs a GPU"
    from owl_wms.configs import Config
    from owl_wms.models import get_model_cls
    from owl_wms.sampling.stream import FrameStream
    from owl_wms.sampling.stream_pool import StreamPool
    mc = Config.from_yaml(os.path.join(REPO, args.config)).model
    torch.manual_seed(0)
    model = get_model_cls(mc.model_id)(mc).cuda().eval()
    core = model.core
    fill = max(2, args.cached - args.ctx + 1)  # tick 0 eager, tick 1 captures; then until the ring is full
    n = fill + args.ticks
    assert args.ctx <= args.cached and args.ctx + n <= mc.n_frames, "the run must stay inside the RoPE table"
    ns_max = max(args.slots)
    x = torch.randn(ns_max, args.ctx, mc.channels, mc.sample_size, mc.sample_size, device="cuda").bfloat16()
    mouse = torch.randn(ns_max, args.ctx + n, 2, device="cuda").bfloat16()
    btn = (torch.rand(ns_max, args.ctx + n, mc.n_buttons, device="cuda") < 0.5).bfloat16()
    print(f"{args.config}: ctx {args.ctx}, max_cached_frames {args.cached}, {args.steps} steps, graphed='frame', "
          f"{fill} ticks to fill the ring + {args.ticks} steady ticks per run, all slots live; {args.rounds} rounds, "
          "variants alternated", flush=True)

    def timed(step):
        per = []
        torch.cuda.synchronize()
        for i in range(n):
            t0 = time.perf_counter()
            step(args.ctx + i)
            torch.cuda.synchronize()
            per.append((time.perf_counter() - t0) * 1e3)
        return statistics.median(per[fill:])

    def run_single(cfg, _):
        torch.manual_seed(1)
        with FrameStream(core, args.steps, cfg, 0.2, args.cached, graphed="frame") as s:
            s.start(x[:1], mouse[:1], btn[:1])
            steady = timed(lambda i: s.step(mouse[:1, i:i + 1], btn[:1, i:i + 1]))
            return steady, f"{s.graph_replays} graph replays, {s.rebases} rebases"

    def run_pool(cfg, ns):
        with StreamPool(core, ns, args.steps, cfg, 0.2, args.cached, graphed="frame") as p:
            for s in range(ns):
                p.open(x[s:s + 1], mouse[s:s + 1], btn[s:s + 1], seed=1 + s)
            steady = timed(lambda i: p.step({s: (mouse[s:s + 1, i:i + 1], btn[s:s + 1, i:i + 1]) for s in range(ns)}))
            return steady, f"{p.graph_replays} graph replays, {sum(p.rebases)} rebases, {len(p.live)} live slots"

    for cfg in args.cfgs:
        variants = [("FrameStream B=1", run_single, 1)] + [(f"StreamPool n_slots={ns}", run_pool, ns)
                                                          for ns in args.slots]
        for name, fn, ns in variants:  # warm-up of each
            fn(cfg, ns)
        res = {v[0]: [] for v in variants}
        for rnd in range(args.rounds):
            for name, fn, ns in variants:
                steady, note = fn(cfg, ns)
                res[name].append(steady)
                print(f"cfg {cfg} round {rnd} {name:22s}: steady {steady:7.2f} ms per tick ({note})", flush=True)
        med = {k: statistics.median(v) for k, v in res.items()}
        for name, _, ns in variants:
            v = res[name]
            print(f"cfg {cfg} {name:22s} {med[name]:7.2f} ms per tick (min {min(v):.2f}, max {max(v):.2f} over "
                  f"{args.rounds} rounds) = {ns * 1e3 / med[name]:6.1f} generated frames/s per card, "
                  f"{med[name] / med['FrameStream B=1']:.3f} x one session's time", flush=True)
        if 1 in args.slots:
            one, fs = med["StreamPool n_slots=1"], res["FrameStream B=1"]
            where = "BELOW" if one < min(fs) else "ABOVE" if one > max(fs) else "within"
            print(f"cfg {cfg} n_slots=1 against FrameStream: pool {one:.2f} ms per frame, FrameStream "
                  f"{med['FrameStream B=1']:.2f} (min {min(fs):.2f}, max {max(fs):.2f}): {where} the FrameStream "
                  "rounds' spread", flush=True)


if __name__ == "__main__":
    main()
