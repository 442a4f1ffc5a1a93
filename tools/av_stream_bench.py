"""Endless audio + video streaming (sampling/stream.py AVFrameStream / AVDiTFrameStream: ring KV cache, ring
decode kernels, RoPE rebase) against av_causal(window_length = ctx + 1) at the same settings: wall ms per
generated frame, eager and HIP graph (one captured Euler step; for the stream also graphed="frame", the whole
frame as one graph), alternated in one process on configs/mmdit_v2.yml's sizes with weights
as initialised (B = 1).  --backbone and --rope override the config's fields and select the stream class.

    python tools/av_stream_bench.py [--backbone mmdit|dit] [--rope motion|ortho] [--ctx 15] [--cached 15]
                                    [--frames 48] [--steps 4] [--cfg 1.3] [--table-frames 40] [--rounds 3]

The stream's run must hold at least 2 wraps of the ring and 1 rebase, so it runs on a RoPE table of
--table-frames frames: for motion the first --table-frames frames of the model's table (a bit-identical
prefix: MotionRoPE tables are prefix-stable), for ortho (not prefix-stable) the table of the same config
with n_frames = --table-frames.  av_causal, which refills its cache per frame, keeps the whole table.
Per-frame cost does not depend on the table length.

Stream rows: every step() is timed on the host with a synchronize after it (a caller who shows the frame
waits for it too); reported per round are the median over all frames and over the steady-state frames
(ring full, the eager first frame / graph capture and the rebase frames left out), then the median and range
of those over the rounds.  av_causal rows: (T_b - T_a) / (frames_b - frames_a) per round, as
tools/av_decode_bench.py forms its steady state.  None of av_causal's code differs from the commit before
the stream was added, so its rows are also that commit's timing on the same box.

Then the ring joint decode attention against the linear one on the same keys (1,040 and 16,640), alternated,
timed with events, and the wide ring decode attention (the dit backbone's) against the joint ring kernel
(the same bits) and against attn_fwd unmasked over the same [cache | new] rows, which is what a dit-backbone
decode step runs without a ring.
"""
import argparse
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "owl-audio-exps_amd")]
import torch  # noqa: E402


def alternated(fns, rounds, iters):
    """name -> 'median us (min, max)' per call over `rounds` rounds of `iters` calls, the variants alternated
    within a round, timed with events, after one warm-up round"""
    res = {k: [] for k in fns}
    for _ in range(rounds + 1):
        for name, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(iters):
                fn()
            e1.record()
            torch.cuda.synchronize()
            res[name].append(e0.elapsed_time(e1) * 1e3 / iters)
    return {k: f"{statistics.median(v[1:]):.1f} us (min {min(v[1:]):.1f}, max {max(v[1:]):.1f})"
            for k, v in res.items()}


def attention_ab(H, D, rounds, iters=50):
    """ring against linear joint decode attention, one 65-row frame, B = 1 and 2 (the CFG batch)"""
    from owl_wms import kernels as K
    n0, n1 = 64, 1
    L = n0 + n1
    unit = lambda t: (t.float().view(*t.shape[:-1], H, D) * torch.rsqrt(
        t.float().view(*t.shape[:-1], H, D).pow(2).mean(-1, keepdim=True))).bfloat16().view(t.shape)
    bound = K.qk_norm_bound(D)
    for keys in (1040, 16640):
        for B in (1, 2):
            q = unit(torch.randn(B, L, H * D, device="cuda"))
            kb = unit(torch.randn(B, keys, H * D, device="cuda"))
            vb = torch.randn(B, keys, H * D, device="cuda").bfloat16()
            start = keys - 40  # the wrap inside a key tile
            st = torch.tensor([start, keys - L, 0, 0], dtype=torch.int64, device="cuda")
            kl, vl = torch.roll(kb, -start, 1).contiguous(), torch.roll(vb, -start, 1).contiguous()
            o0 = torch.empty(B * n0, H * D, device="cuda", dtype=torch.bfloat16)
            o1 = torch.empty(B * n1, H * D, device="cuda", dtype=torch.bfloat16)
            fns = {"ring": lambda: K.attn_decode_joint_ring_fwd(q, kb, vb, H, D, n0, n1, st, 0, score_bound=bound,
                                                               o0=o0, o1=o1),
                   "linear": lambda: K.attn_decode_joint_fwd(q, kl, vl, H, D, n0, n1, score_bound=bound, o0=o0, o1=o1)}
            a = [t.clone() for t in fns["ring"]()[:2]]
            b = fns["linear"]()[:2]
            same = all(torch.equal(x, y) for x, y in zip(a, b))
            res = alternated(fns, rounds, iters)
            print(f"joint decode attention, {keys} keys, B {B}, H {H}: ring {res['ring']}, linear {res['linear']}; "
                  f"same bits: {same}", flush=True)
            # the wide ring kernel (one output, the dit backbone's) against the joint ring kernel, and against
            # attn_fwd unmasked over the unrolled [cache | new] rows
            ow = torch.empty(B, L, H * D, device="cuda", dtype=torch.bfloat16)
            mask = K.FrameMask(1, None, False, 0, None)
            fns = {"wide": lambda: K.attn_decode_wide_ring_fwd(q, kb, vb, H, D, st, L, 0, score_bound=bound, o=ow),
                   "joint": fns["ring"],
                   "attn_fwd": lambda: K.attn_fwd(q, kl, vl, H, D, mask, score_bound=bound)}
            w = fns["wide"]()[0].clone()
            same = torch.equal(w[:, :n0].reshape(B * n0, -1), a[0]) and \
                torch.equal(w[:, n0:].reshape(B * n1, -1), a[1])
            ref = fns["attn_fwd"]()[0].float()
            err = ((w.float() - ref).norm() / ref.norm()).item()
            res = alternated(fns, rounds, iters)
            print(f"wide decode attention, {keys} keys, B {B}, H {H}: wide ring {res['wide']}, joint ring "
                  f"{res['joint']}; same bits: {same}", flush=True)
            print(f"wide decode attention, {keys} keys, B {B}, H {H}: wide ring {res['wide']}, attn_fwd unmasked "
                  f"{res['attn_fwd']}; rel-L2 {err:.1e}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="configs/mmdit_v2.yml")
    ap.add_argument("--backbone", choices=("mmdit", "dit"), default="mmdit")
    ap.add_argument("--rope", choices=("motion", "ortho"), default="motion")
    ap.add_argument("--ctx", type=int, default=15)
    ap.add_argument("--cached", type=int, default=15, help="the stream's max_cached_frames")
    ap.add_argument("--frames", type=int, default=48)
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--cfg", type=float, default=1.3)
    ap.add_argument("--table-frames", type=int, default=40)
    ap.add_argument("--frames-a", type=int, default=3)
    ap.add_argument("--frames-b", type=int, default=9)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--skip-attention", action="store_true", help="the streams only, not the attention kernels' A/B")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "av_stream_bench needs a GPU"
    from owl_wms.configs import Config
    from owl_wms.models import get_model_cls
    from owl_wms.sampling import get_sampler_cls
    from owl_wms.nn.rope import get_rope_cls
    from owl_wms.sampling.stream import av_stream_cls
    cfg = Config.from_yaml(os.path.join(REPO, args.config))
    mc = cfg.model
    mc.backbone, mc.rope_impl = args.backbone, args.rope
    stream_cls = av_stream_cls(mc.backbone)
    torch.manual_seed(0)
    model = get_model_cls(mc.model_id)(mc).cuda().eval()
    core, rope, tpf = model.core, model.core.transformer.rope, mc.tokens_per_frame
    full = (rope.cos, rope.sin)
    assert args.cached + 1 < args.table_frames <= mc.n_frames
    if args.rope == "motion":
        short = tuple(t[:args.table_frames * tpf] for t in full)
    else:  # the table a model with n_frames = --table-frames carries
        n_frames, mc.n_frames = mc.n_frames, args.table_frames
        short_rope = get_rope_cls(args.rope)(mc).cuda()
        mc.n_frames = n_frames
        short = (short_rope.cos, short_rope.sin)
        assert short[0].shape == (args.table_frames * tpf, full[0].shape[1])
    W, n = args.ctx + 1, args.ctx + args.frames
    # av_causal inpaints at the end of a window of W frames, W - 1 = ctx of them history: it takes W context
    # frames and re-noises the last ctx; the stream caches the same ctx frames once
    xw = torch.randn(1, W, mc.channels, mc.sample_size, mc.sample_size, device="cuda").bfloat16()
    audiow = torch.randn(1, W, mc.audio_channels, device="cuda").bfloat16()
    x, audio = xw[:, 1:], audiow[:, 1:]
    mouse = torch.randn(1, n, 2, device="cuda").bfloat16()
    btn = (torch.rand(1, n, mc.n_buttons, device="cuda") < 0.5).bfloat16()
    print(f"{args.config} (backbone {mc.backbone}, rope_impl {mc.rope_impl}, {stream_cls.__name__}): B 1, ctx "
          f"{args.ctx}, {args.steps} steps, cfg {args.cfg}; stream: max_cached_frames {args.cached}, {args.frames} frames, table {args.table_frames} frames; av_causal: "
          f"window {W}, {args.frames_a} / {args.frames_b} frames; {args.rounds} rounds, variants alternated",
          flush=True)

    def run_stream(graphed):
        rope.cos, rope.sin = short
        try:
            per, rebased = [], []
            torch.manual_seed(1)
            with stream_cls(core, args.steps, args.cfg, 0.2, args.cached, graphed=graphed) as s:
                s.start(x, audio, mouse, btn)
                torch.cuda.synchronize()
                for i in range(args.frames):
                    r0 = s.rebases
                    t0 = time.perf_counter()
                    s.step(mouse[:, args.ctx + i:args.ctx + i + 1], btn[:, args.ctx + i:args.ctx + i + 1])
                    torch.cuda.synchronize()
                    per.append((time.perf_counter() - t0) * 1e3)
                    rebased.append(s.rebases != r0)
                evictions = max(0, args.ctx + args.frames - args.cached)
                wraps = evictions // (args.cached + 1)
                rows = {kb.shape[1] for kb, _ in s.kv_cache.bufs}
                # the ring is full; frame 0 is eager / captures the step, frame 1 captures the frame
                full_from = max(2 if graphed == "frame" else 1, args.cached - args.ctx + 1)
                steady = [t for t, rb in list(zip(per, rebased))[full_from:] if not rb]
                reb = [t for t, rb in zip(per, rebased) if rb]
                note = (f"{wraps} wraps, {s.rebases} rebases (rebase frames {', '.join(f'{t:.2f}' for t in reb)} ms), "
                        f"{rows.pop()} cache rows per layer")
                return statistics.median(per), statistics.median(steady), (min(per), max(per)), note
        finally:
            rope.cos, rope.sin = full

    def run_causal(graphed):
        ts = []
        for frames in (args.frames_a, args.frames_b):
            s = get_sampler_cls("av_causal")(n_steps=args.steps, cfg_scale=args.cfg, window_length=W, num_frames=frames)
            torch.manual_seed(1)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            s(core, xw, audiow, mouse[:, :W], btn[:, :W], compile_on_decode=graphed)
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        steady = (ts[1] - ts[0]) / (args.frames_b - args.frames_a)
        return ts[1] / args.frames_b, steady, None, f"{W * tpf} cache rows per layer, refilled per frame"

    variants = (("stream eager", run_stream, False), ("stream graph", run_stream, True),
                ("stream frame", run_stream, "frame"),
                ("av_causal eager", run_causal, False), ("av_causal graph", run_causal, True))
    for name, fn, graphed in variants:  # warm-up of each
        fn(graphed)
    res = {v[0]: [] for v in variants}
    for rnd in range(args.rounds):
        for name, fn, graphed in variants:
            allf, steady, rng, note = fn(graphed)
            res[name].append(steady)
            extra = f", per-frame range {rng[0]:.2f} .. {rng[1]:.2f}" if rng else ""
            print(f"round {rnd} {name:16s}: {allf:7.2f} ms per generated frame (all frames), steady {steady:7.2f} ms"
                  f"{extra} ({note})", flush=True)
    for name, *_ in variants:
        v = res[name]
        print(f"{name:16s} steady {statistics.median(v):7.2f} ms per generated frame (min {min(v):.2f}, "
              f"max {max(v):.2f} over {args.rounds} rounds)", flush=True)
    for mode in ("eager", "graph"):
        a, b = statistics.median(res[f"stream {mode}"]), statistics.median(res[f"av_causal {mode}"])
        print(f"{mode}: stream / av_causal = {a / b:.3f} (steady medians)", flush=True)
    a, b = statistics.median(res["stream frame"]), statistics.median(res["stream graph"])
    print(f"stream frame / stream graph = {a / b:.3f} (steady medians; the graph column is the code of the commit "
          "before the frame mode)", flush=True)
    if not args.skip_attention:
        attention_ab(mc.n_heads, mc.d_model // mc.n_heads, args.rounds)


if __name__ == "__main__":
    main()
