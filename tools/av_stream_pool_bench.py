"""Multi-session audio + video streaming (sampling/stream_pool.py AVStreamPool / AVDiTStreamPool: n_slots
sessions in one batch on per-slot ring state) against one session on the backbone's B = 1 stream class
(AVFrameStream / AVDiTFrameStream) at the same settings: wall ms per tick and generated frames per second per
card, every slot live, the whole tick / frame captured (graphed="frame"), alternated in one process on
configs/mmdit_v2.yml's sizes with weights as initialised.

    python tools/av_stream_pool_bench.py [--config configs/mmdit_v2.yml] [--backbones mmdit dit] [--ctx 15]
                                         [--cached 15] [--ticks 40] [--steps 4] [--cfgs 1.3 1.0]
                                         [--slots 1 2 4 8] [--rounds 3] [--skip-attention]

Every run opens its sessions with --ctx context frames (different data and seeds per slot), runs until the ring
holds --cached frames and then --ticks more.  Every step() is timed on the host with a synchronize after it;
reported per round is the median over the steady-state ticks (tick 0, which runs eagerly, tick 1, which
captures, and the ticks before the ring is full left out), then the median and range over the rounds.  The
positions stay inside the RoPE table, so no run rebases.

Reported, not gated: whether the one-slot pool's median per tick lies within the min - max spread of the B = 1
stream's rounds of the same backbone and CFG scale.

Then the slot instantiations of the wide and joint ring decode attention against their single-state
instantiations on the same buffers (one live slot, B 1, 1,040 and 16,640 keys), in isolation, alternated, timed
with events; the expectation is equality within the rounds' spread.
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
    """name -> [us per call] over `rounds` rounds of `iters` calls, the variants alternated within a round,
    timed with events, after one warm-up round"""
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
    return {k: v[1:] for k, v in res.items()}


def attention_ab(H, D, rounds):
    """slot against single-state instantiations of the joint and the wide ring decode attention: one 65-row
    frame, B 1, one live slot whose row is the single state"""
    from owl_wms import kernels as K
    n0, n1 = 64, 1
    L = n0 + n1
    unit = lambda t: (t.float().view(*t.shape[:-1], H, D) * torch.rsqrt(  # noqa: E731
        t.float().view(*t.shape[:-1], H, D).pow(2).mean(-1, keepdim=True))).bfloat16().view(t.shape)
    bound = K.qk_norm_bound(D)
    fmt = lambda v: f"{statistics.median(v):.1f} us (min {min(v):.1f}, max {max(v):.1f})"  # noqa: E731
    for keys, iters in ((1040, 2000), (16640, 400)):
        q = unit(torch.randn(1, L, H * D, device="cuda"))
        kb = unit(torch.randn(1, keys, H * D, device="cuda"))
        vb = torch.randn(1, keys, H * D, device="cuda").bfloat16()
        start = keys - 40  # the wrap inside a key tile
        st = torch.tensor([start, keys - L, 0, 0], dtype=torch.int64, device="cuda")
        sts = torch.tensor([[start, keys - L, 0, 1]], dtype=torch.int64, device="cuda")
        o0 = torch.empty(n0, H * D, device="cuda", dtype=torch.bfloat16)
        o1 = torch.empty(n1, H * D, device="cuda", dtype=torch.bfloat16)
        ow = torch.empty(1, L, H * D, device="cuda", dtype=torch.bfloat16)
        pairs = {
            "joint": (lambda: K.attn_decode_joint_ring_fwd(q, kb, vb, H, D, n0, n1, st, 0, score_bound=bound, o0=o0,
                                                           o1=o1, want_lse=True),
                      lambda: K.attn_decode_joint_ring_slots_fwd(q, kb, vb, H, D, n0, n1, sts, 0, score_bound=bound,
                                                                 o0=o0, o1=o1)),
            "wide": (lambda: K.attn_decode_wide_ring_fwd(q, kb, vb, H, D, st, L, 0, score_bound=bound, o=ow),
                     lambda: K.attn_decode_wide_ring_slots_fwd(q, kb, vb, H, D, sts, L, 0, score_bound=bound, o=ow)),
        }
        for name, (single, slots) in pairs.items():
            a = [t.clone() for t in single()]
            b = slots()
            same = all(torch.equal(x, y) for x, y in zip(a, b))
            res = alternated({"single": single, "slots": slots}, rounds, iters)
            s, p = res["single"], res["slots"]
            med = statistics.median(p)
            where = "BELOW" if med < min(s) else "ABOVE" if med > max(s) else "within"
            print(f"{name} ring decode attention, {keys} keys, B 1, H {H}, {iters} calls per round: single-state "
                  f"{fmt(s)}, slot form {fmt(p)}: slot median {where} the single-state rounds' spread; same bits: "
                  f"{same}", flush=True)


def bench_backbone(args, backbone):
    from owl_wms.configs import Config
    from owl_wms.models import get_model_cls
    from owl_wms.sampling.stream import av_stream_cls
    from owl_wms.sampling.stream_pool import av_pool_cls
    mc = Config.from_yaml(os.path.join(REPO, args.config)).model
    mc.backbone = backbone
    stream_cls, pool_cls = av_stream_cls(backbone), av_pool_cls(backbone)
    torch.manual_seed(0)
    model = get_model_cls(mc.model_id)(mc).cuda().eval()
    core = model.core
    fill = max(2, args.cached - args.ctx + 1)  # tick 0 eager, tick 1 captures; then until the ring is full
    n = fill + args.ticks
    assert args.ctx <= args.cached and args.ctx + n <= mc.n_frames, "the run must stay inside the RoPE table"
    ns_max = max(args.slots)
    x = torch.randn(ns_max, args.ctx, mc.channels, mc.sample_size, mc.sample_size, device="cuda").bfloat16()
    audio = torch.randn(ns_max, args.ctx, mc.audio_channels, device="cuda").bfloat16()
    mouse = torch.randn(ns_max, args.ctx + n, 2, device="cuda").bfloat16()
    btn = (torch.rand(ns_max, args.ctx + n, mc.n_buttons, device="cuda") < 0.5).bfloat16()
    print(f"{args.config} (backbone {backbone}, {stream_cls.__name__} / {pool_cls.__name__}): ctx {args.ctx}, "
          f"max_cached_frames {args.cached}, {args.steps} steps, graphed='frame', {fill} ticks to fill the ring + "
          f"{args.ticks} steady ticks per run, all slots live; {args.rounds} rounds, variants alternated", flush=True)

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
        with stream_cls(core, args.steps, cfg, 0.2, args.cached, graphed="frame") as s:
            s.start(x[:1], audio[:1], mouse[:1], btn[:1])
            steady = timed(lambda i: s.step(mouse[:1, i:i + 1], btn[:1, i:i + 1]))
            return steady, f"{s.graph_replays} graph replays, {s.rebases} rebases"

    def run_pool(cfg, ns):
        with pool_cls(core, ns, args.steps, cfg, 0.2, args.cached, graphed="frame") as p:
            for s in range(ns):
                p.open(x[s:s + 1], audio[s:s + 1], mouse[s:s + 1], btn[s:s + 1], seed=1 + s)
            steady = timed(lambda i: p.step({s: (mouse[s:s + 1, i:i + 1], btn[s:s + 1, i:i + 1]) for s in range(ns)}))
            return steady, f"{p.graph_replays} graph replays, {sum(p.rebases)} rebases, {len(p.live)} live slots"

    one = f"{stream_cls.__name__} B=1"
    for cfg in args.cfgs:
        variants = [(one, run_single, 1)] + [(f"{pool_cls.__name__} n_slots={ns}", run_pool, ns) for ns in args.slots]
        for name, fn, ns in variants:  # warm-up of each
            fn(cfg, ns)
        res = {v[0]: [] for v in variants}
        for rnd in range(args.rounds):
            for name, fn, ns in variants:
                steady, note = fn(cfg, ns)
                res[name].append(steady)
                print(f"{backbone} cfg {cfg} round {rnd} {name:28s}: steady {steady:7.2f} ms per tick ({note})",
                      flush=True)
        med = {k: statistics.median(v) for k, v in res.items()}
        for name, _, ns in variants:
            v = res[name]
            print(f"{backbone} cfg {cfg} {name:28s} {med[name]:7.2f} ms per tick (min {min(v):.2f}, max {max(v):.2f} "
                  f"over {args.rounds} rounds) = {ns * 1e3 / med[name]:6.1f} generated frames/s per card, "
                  f"{med[name] / med[one]:.3f} x one session's time", flush=True)
        if 1 in args.slots:
            p1, fs = med[f"{pool_cls.__name__} n_slots=1"], res[one]
            where = "BELOW" if p1 < min(fs) else "ABOVE" if p1 > max(fs) else "within"
            print(f"{backbone} cfg {cfg} n_slots=1 against {stream_cls.__name__}: pool {p1:.2f} ms per frame, stream "
                  f"{med[one]:.2f} (min {min(fs):.2f}, max {max(fs):.2f}): {where} the stream rounds' spread",
                  flush=True)
    return mc.n_heads, mc.d_model // mc.n_heads


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="configs/mmdit_v2.yml")
    ap.add_argument("--backbones", nargs="+", choices=("mmdit", "dit"), default=["mmdit", "dit"])
    ap.add_argument("--ctx", type=int, default=15)
    ap.add_argument("--cached", type=int, default=15, help="max_cached_frames of every stream")
    ap.add_argument("--ticks", type=int, default=40, help="steady-state ticks per run")
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--cfgs", type=float, nargs="+", default=[1.3, 1.0])
    ap.add_argument("--slots", type=int, nargs="+", default=[1, 2, 4, 8])
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--attention-rounds", type=int, default=7)
    ap.add_argument("--skip-attention", action="store_true", help="the pools only, not the attention kernels' A/B")
    ap.add_argument("--skip-pools", action="store_true", help="the attention kernels' A/B only")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "av_stream_pool_bench needs a GPU"
    H, D = 24, 64  # mmdit_v2's heads
    if not args.skip_pools:
        for backbone in args.backbones:
            H, D = bench_backbone(args, backbone)
            torch.cuda.empty_cache()
    if not args.skip_attention:
        attention_ab(H, D, args.attention_rounds)


if __name__ == "__main__":
    main()
