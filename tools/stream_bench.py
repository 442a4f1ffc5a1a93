"""Endless streaming (sampling/stream.py FrameStream: ring KV cache + RoPE rebase) against
AVCachingSamplerV2(max_window=...) at the same settings: wall ms per generated frame, eager and HIP-graph
replay (for the stream also graphed="frame", the whole frame as one graph), alternated in one process on a
config's model with random-init weights (N = 1).

    python tools/stream_bench.py [--config configs/dit_v4.yml] [--ctx 8] [--cached 120] [--frames 360]
                                 [--steps 16] [--cfg 1.0] [--table-frames 256] [--reps 2]

The stream's run must hold at least 2 wraps of the ring and 1 rebase.  A rebase falls due when the
positions reach the end of the RoPE table (1536 frames at dit_v4), so the stream runs on the first
--table-frames frames of the table (a bit-identical prefix: the tables are prefix-stable); the sampler,
which cannot pass the table, keeps the whole of it.  Per-frame cost does not depend on the table length.

Reported per run: total wall / frames (context pass and graph capture included, as the sampler's call
has them inside), and for the stream the median over the steady-state frames (after the ring is full).
AVCachingSamplerV2 and the linear kernels it runs are the ones of the commit before the stream was
added, so its rows are also that commit's timing on the same box.
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
    ap.add_argument("--cached", type=int, default=120, help="FrameStream max_cached_frames")
    ap.add_argument("--frames", type=int, default=360)
    ap.add_argument("--steps", type=int, default=16)
    ap.add_argument("--cfg", type=float, default=1.0)
    ap.add_argument("--table-frames", type=int, default=256)
    ap.add_argument("--reps", type=int, default=2)
    args = ap.parse_args()
    from owl_wms.configs import Config
    from owl_wms.models import get_model_cls
    from owl_wms.sampling import get_sampler_cls
    from owl_wms.sampling.stream import FrameStream
    cfg = Config.from_yaml(os.path.join(REPO, args.config))
    mc = cfg.model
    torch.manual_seed(0)
    model = get_model_cls(mc.model_id)(mc).cuda().eval()
    core, rope, tpf = model.core, model.core.transformer.rope, mc.tokens_per_frame
    full = (rope.cos, rope.sin)
    short = tuple(t[:args.table_frames * tpf] for t in full)
    assert args.cached + 1 < args.table_frames <= mc.n_frames and args.ctx + args.frames <= mc.n_frames
    n = args.ctx + args.frames
    x = torch.randn(1, args.ctx, mc.channels, mc.sample_size, mc.sample_size, device="cuda").bfloat16()
    mouse = torch.randn(1, n, 2, device="cuda").bfloat16()
    btn = (torch.rand(1, n, mc.n_buttons, device="cuda") < 0.5).bfloat16()
    max_window = args.cached - args.ctx + 1
    print(f"{args.config}: ctx {args.ctx}, {args.frames} frames, {args.steps} steps, cfg {args.cfg}, "
          f"max_cached_frames {args.cached} (sampler max_window {max_window}), stream table "
          f"{args.table_frames} frames", flush=True)

    def run_stream(graphed):
        rope.cos, rope.sin = short
        try:
            # per-frame times from events on the stream: no host sync inside the run (the sampler has
            # none either, and its eager cache-update launches overlap the work still queued)
            evs = [torch.cuda.Event(enable_timing=True) for _ in range(args.frames + 1)]
            torch.manual_seed(1)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            with FrameStream(core, args.steps, args.cfg, 0.2, args.cached, graphed=graphed) as s:
                s.start(x, mouse, btn)
                evs[0].record()
                for i in range(args.frames):
                    s.step(mouse[:, args.ctx + i:args.ctx + i + 1], btn[:, args.ctx + i:args.ctx + i + 1])
                    evs[i + 1].record()
                torch.cuda.synchronize()
                total = (time.perf_counter() - t0) * 1e3 / args.frames
                per = [evs[i].elapsed_time(evs[i + 1]) for i in range(args.frames)]
                evictions = max(0, args.ctx + args.frames - args.cached)
                wraps = evictions // (args.cached + 1)
                rows = {kb.shape[1] for kb, _ in s.kv_cache.bufs}
                steady = per[args.cached - args.ctx + 1:]
                return total, statistics.median(steady), (f"{wraps} wraps, {s.rebases} rebases, "
                                                          f"{rows.pop()} rows per layer")
        finally:
            rope.cos, rope.sin = full

    def run_sampler(graphed):
        torch.manual_seed(1)
        s = get_sampler_cls("av_caching")(n_steps=args.steps, cfg_scale=args.cfg, num_frames=args.frames,
                                          noise_prev=0.2, max_window=max_window)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        s(core, x, mouse, btn, compile_on_decode=graphed)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / args.frames, None, f"{(n + 1) * tpf} rows per layer"

    res, steadies = {}, {}
    modes = {False: "eager", True: "graph", "frame": "frame"}
    for rep in range(args.reps):
        for graphed, mode in modes.items():
            # "frame" (the whole frame as one graph) is a mode of the stream alone
            for name, fn in (("stream", run_stream), ("sampler", run_sampler))[:1 if graphed == "frame" else 2]:
                total, steady, note = fn(graphed)
                res.setdefault((name, graphed), []).append(total)
                st = ""
                if steady is not None:
                    steadies.setdefault(mode, []).append(steady)
                    st = f", steady-state median {steady:.2f} ms"
                print(f"rep {rep} {name:7s} {mode}: {total:.2f} ms per generated frame{st} ({note})", flush=True)
    for mode, v in steadies.items():
        print(f"stream {mode}: steady-state {statistics.median(v):.2f} ms per generated frame (min {min(v):.2f}, max "
              f"{max(v):.2f} over {args.reps} reps)", flush=True)
    ratio = statistics.median(steadies["frame"]) / statistics.median(steadies["graph"])
    print(f"stream frame / stream graph = {ratio:.3f} (steady-state medians; the graph column is the code of the "
          "commit before the frame mode)", flush=True)
    for graphed in (False, True):
        mode = "graph" if graphed else "eager"
        a, b = res[("stream", graphed)], res[("sampler", graphed)]
        spread = max(max(v) - min(v) for v in (a, b))
        print(f"{mode}: stream {statistics.mean(a):.2f} ms, sampler {statistics.mean(b):.2f} ms per generated frame "
              f"(stream / sampler {statistics.mean(a) / statistics.mean(b):.3f}; run-to-run spread "
              f"{spread:.2f} ms)", flush=True)


if __name__ == "__main__":
    main()
