"""ms per generated frame of the av_causal sampler (sampling/av_window.py) on a config's MMDiT with
weights as initialised, B = 1: the MMDiT cache path with decoding off (MMDiTBlock._forward_cached),
decoding on eager (_forward_decode: joint-frame rope + joint decode attention; and with the rope kernel
alone, the masked attention kept) and decoding on with one HIP graph per generated frame
(compile_on_decode).

The variants alternate in one process after a warm-up run of each.  Every round times a run of
--frames-a and a run of --frames-b generated frames per variant; the steady-state figure is
(T_b - T_a) / (frames_b - frames_a), which cancels the per-call set-up, the eager first frame and the
graph capture.  Reported: median, min and max over the rounds, and the whole-call ms per frame of the
longer run.  Also the libowlk entry calls one block makes per decode step, counted, off and on.

    python tools/av_decode_bench.py [--config configs/mmdit_v2.yml] [--window 16] [--steps 4] [--cfg 1.3]
"""
import argparse
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "owl-audio-exps_amd")]
import torch  # noqa: E402

# (name, decoding, graphed, joint decode attention)
VARIANTS = (("decoding off", False, False, True), ("decoding on, rope only", True, False, False),
            ("decoding on, eager", True, False, True), ("decoding on, graph", True, True, True))


def block_calls(model, sampler, ins):
    """libowlk entry calls of blocks[0] in each forward of one generated frame -> list of counts"""
    from owl_wms import kernels
    n = [0]
    real = kernels.call

    def counting(*a, **k):
        n[0] += 1
        return real(*a, **k)

    counts, mark = [], [0]
    blk = model.core.transformer.blocks[0]
    h0 = blk.register_forward_pre_hook(lambda m, i: mark.__setitem__(0, n[0]))
    h1 = blk.register_forward_hook(lambda m, i, o: counts.append(n[0] - mark[0]))
    kernels.call = counting
    try:
        keep, sampler.num_frames = sampler.num_frames, 1
        sampler(model.core, *ins)
        sampler.num_frames = keep
    finally:
        kernels.call = real
        h0.remove()
        h1.remove()
    return counts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="configs/mmdit_v2.yml")
    ap.add_argument("--window", type=int, default=16)
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--cfg", type=float, default=1.3)
    ap.add_argument("--frames-a", type=int, default=3)
    ap.add_argument("--frames-b", type=int, default=9)
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "av_decode_bench needs a GPU"
    from owl_wms.configs import Config
    from owl_wms.models import get_model_cls
    from owl_wms.nn.mmattn import MMDiTBlock
    from owl_wms.sampling import get_sampler_cls
    cfg = Config.from_yaml(os.path.join(REPO, args.config))
    mc = cfg.model
    torch.manual_seed(0)
    model = get_model_cls(mc.model_id)(mc).cuda().eval()
    W = args.window
    ins = (torch.randn(1, W, mc.channels, mc.sample_size, mc.sample_size, device="cuda").bfloat16(),
           torch.randn(1, W, mc.audio_channels, device="cuda").bfloat16(),
           torch.randn(1, W, 2, device="cuda").bfloat16(),
           (torch.rand(1, W, mc.n_buttons, device="cuda") < 0.5).bfloat16())

    def run(decoding, graphed, frames, joint=True):
        MMDiTBlock.joint_attention = joint
        s = get_sampler_cls("av_causal")(n_steps=args.steps, cfg_scale=args.cfg, window_length=W, num_frames=frames)
        s.use_decoding = decoding
        torch.manual_seed(1)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = s(model.core, *ins, compile_on_decode=graphed)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    print(f"{args.config}: av_causal, B 1, window {W}, {args.steps} steps, cfg {args.cfg}; "
          f"{args.rounds} rounds of {args.frames_a} / {args.frames_b} frames, variants alternated", flush=True)
    for name, dec, _, joint in VARIANTS[:3]:
        MMDiTBlock.joint_attention = joint
        s = get_sampler_cls("av_causal")(n_steps=args.steps, cfg_scale=args.cfg, window_length=W, num_frames=1)
        s.use_decoding = dec
        c = block_calls(model, s, ins)
        print(f"libowlk calls per block: {name}: prefill {c[0]}, decode step {c[1:]}", flush=True)
    outs = {}
    for name, dec, gr, joint in VARIANTS:  # warm-up: every shape of every variant
        outs[name] = run(dec, gr, args.frames_a, joint)[1]
    steady = {v[0]: [] for v in VARIANTS}
    whole = {v[0]: [] for v in VARIANTS}
    for _ in range(args.rounds):
        for name, dec, gr, joint in VARIANTS:
            ta, _ = run(dec, gr, args.frames_a, joint)
            tb, _ = run(dec, gr, args.frames_b, joint)
            steady[name].append((tb - ta) / (args.frames_b - args.frames_a))
            whole[name].append(tb / args.frames_b)
    for name, *_ in VARIANTS:
        v, w = steady[name], whole[name]
        print(f"{name:22s} steady {statistics.median(v):8.2f} ms/frame (min {min(v):.2f}, max {max(v):.2f}); "
              f"whole call {statistics.median(w):8.2f} ms/frame (min {min(w):.2f}, max {max(w):.2f})", flush=True)
    base = statistics.median(steady[VARIANTS[0][0]])
    for name, *_ in VARIANTS[1:]:
        print(f"{name}: {base / statistics.median(steady[name]):.3f}x of decoding off (steady medians)")
    a, _, b, c = (outs[v[0]] for v in VARIANTS)
    rel = lambda x, y: ((x.float() - y.float()).norm() / y.float().norm()).item()
    print(f"graph == eager bits: {all(torch.equal(x, y) for x, y in zip(b, c))}; on vs off rel video "
          f"{rel(b[0], a[0]):.2e} audio {rel(b[1], a[1]):.2e}")


if __name__ == "__main__":
    main()
