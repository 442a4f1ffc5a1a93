"""Endless audio streaming (sampling/stream.py AudioStream: ring KV cache, one-token ring decode, RoPE rebase)
eager, with one captured Euler step and with the whole token captured (graphed="frame"), against
audio_caching at the same settings: wall ms per generated token, alternated in one process on
configs/audio.yml's sizes with weights as initialised (B = 1).

    python tools/audio_stream_bench.py [--ctx 120] [--cached 120] [--tokens 64] [--steps 16]
                                       [--table-rows 160] [--tokens-a 8] [--tokens-b 40] [--rounds 3]

The context fills the window (--ctx = --cached), so every generated token sees the steady state: 120 cached
tokens, one eviction per token.  The stream runs on the first --table-rows rows of the Audio1DRoPE table (a
bit-identical prefix), so the run holds wraps of the ring and at least one rebase; audio_caching, which cannot
pass the table, keeps the whole of it (max_window 1 with --ctx context tokens caches --ctx tokens, its
counting).  Per-token cost does not depend on the table length.

Stream rows: every step() is timed on the host with a synchronize after it; reported per round is the median
over the steady-state tokens (token 0, which runs eagerly, token 1, which captures in frame mode, and the
rebase tokens left out), then the median and range over the rounds.  audio_caching rows:
(T_b - T_a) / (tokens_b - tokens_a) per round.  audio_caching's code and the stream's graphed=True column are
those of the commit before the frame mode, so they are also that commit's timing on the same box.
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
    ap.add_argument("--config", default="configs/audio.yml")
    ap.add_argument("--ctx", type=int, default=120)
    ap.add_argument("--cached", type=int, default=120, help="the stream's max_cached_frames")
    ap.add_argument("--tokens", type=int, default=64)
    ap.add_argument("--steps", type=int, default=16)
    ap.add_argument("--table-rows", type=int, default=160)
    ap.add_argument("--tokens-a", type=int, default=8)
    ap.add_argument("--tokens-b", type=int, default=40)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "audio_stream_bench needs a GPU"
    from owl_wms.configs import Config
    from owl_wms.models import get_model_cls
    from owl_wms.sampling import get_sampler_cls
    from owl_wms.sampling.stream import AudioStream
    mc = Config.from_yaml(os.path.join(REPO, args.config)).model
    torch.manual_seed(0)
    model = get_model_cls(mc.model_id)(mc).cuda().eval()
    core, rope = model.core, model.core.transformer.rope
    full = (rope.cos, rope.sin)
    assert args.ctx <= args.cached and args.cached + 1 < args.table_rows <= mc.n_frames
    short = tuple(t[:args.table_rows] for t in full)
    x = torch.randn(1, args.ctx, mc.channels, device="cuda").bfloat16()
    print(f"{args.config} (AudioStream): B 1, ctx {args.ctx}, {args.steps} steps; stream: max_cached_frames "
          f"{args.cached}, {args.tokens} tokens, table {args.table_rows} rows; audio_caching: max_window "
          f"{args.cached - args.ctx + 1}, {args.tokens_a} / {args.tokens_b} tokens; {args.rounds} rounds, variants "
          "alternated", flush=True)

    def run_stream(graphed):
        rope.cos, rope.sin = short
        try:
            per, rebased = [], []
            torch.manual_seed(1)
            with AudioStream(core, args.steps, 0.2, args.cached, graphed=graphed) as s:
                s.start(x)
                torch.cuda.synchronize()
                for _ in range(args.tokens):
                    r0 = s.rebases
                    t0 = time.perf_counter()
                    s.step()
                    torch.cuda.synchronize()
                    per.append((time.perf_counter() - t0) * 1e3)
                    rebased.append(s.rebases != r0)
                full_from = max(2, args.cached - args.ctx + 1)  # token 0 eager, token 1 captures the frame
                steady = [t for t, rb in list(zip(per, rebased))[full_from:] if not rb]
                reb = [t for t, rb in zip(per, rebased) if rb]
                note = (f"{s.rebases} rebases (rebase tokens {', '.join(f'{t:.2f}' for t in reb)} ms), "
                        f"{s.graph_replays} graph replays, {s.kv_cache.capacity} cache rows per layer")
                return statistics.median(per), statistics.median(steady), note
        finally:
            rope.cos, rope.sin = full

    def run_caching(_):
        ts = []
        for tokens in (args.tokens_a, args.tokens_b):
            s = get_sampler_cls("audio_caching")(n_steps=args.steps, num_tokens=tokens, noise_prev=0.2,
                                                 max_window=args.cached - args.ctx + 1)
            torch.manual_seed(1)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            s(core, x)
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        steady = (ts[1] - ts[0]) / (args.tokens_b - args.tokens_a)
        return ts[1] / args.tokens_b, steady, f"{args.cached} cached tokens, host positions"

    variants = (("stream eager", run_stream, False), ("stream graph", run_stream, True),
                ("stream frame", run_stream, "frame"), ("audio_caching", run_caching, False))
    for name, fn, graphed in variants:  # warm-up of each
        fn(graphed)
    res = {v[0]: [] for v in variants}
    for rnd in range(args.rounds):
        for name, fn, graphed in variants:
            allt, steady, note = fn(graphed)
            res[name].append(steady)
            print(f"round {rnd} {name:14s}: {allt:7.2f} ms per generated token (all tokens), steady {steady:7.2f} ms "
                  f"({note})", flush=True)
    med = {k: statistics.median(v) for k, v in res.items()}
    for name, *_ in variants:
        v = res[name]
        print(f"{name:14s} steady {med[name]:7.2f} ms per generated token (min {min(v):.2f}, max {max(v):.2f} over "
              f"{args.rounds} rounds)", flush=True)
    print(f"stream frame / stream graph = {med['stream frame'] / med['stream graph']:.3f}, stream frame / "
          f"audio_caching = {med['stream frame'] / med['audio_caching']:.3f}, stream eager / audio_caching = "
          f"{med['stream eager'] / med['audio_caching']:.3f} (steady medians)", flush=True)


if __name__ == "__main__":
    main()
