"""Backward of the decode attention (owlk_attn_decode_bwd: dQ over [cache | frame], dK / dV of the new
frame's rows) at the self-forcing rollout shapes of dit_v4 (24 heads, D 64) and dit_v4_5B (20 heads,
D 128): one 64-token frame of queries against a 60-frame window (global layer, 3,840 keys) or a
16-frame window (local layer, 1,024 keys), B = 1 and 4.

Compared with the only alternative a user has today: the same three gradients by bf16 torch.matmul
and torch's softmax backward on the same GPU, from head-major contiguous copies and the SAVED bf16
probabilities (so the torch side recomputes nothing and pays no layout change).

Both are captured into a HIP graph of `iters` calls and replayed (a Python loop of launches is
CPU-bound at these sizes); the two are timed alternately, `rounds` times, after a warm-up of every
shape, and the minimum and median over the rounds are printed.  ours = owlk_attn_delta +
owlk_attn_decode_bwd (2 launches) + the reduce.  HBM floor = the bytes of K and V read once / 8.0
TB/s (MI355X_MICROARCH: 8.0 TB/s spec, ~6.3 achievable).

    python tools/attn_decode_bwd_bench.py [--out profiles/attn_decode_bwd_bench.log]
"""
import argparse
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "owl-audio-exps_amd"), os.path.join(REPO, "tools")]
import torch  # noqa: E402

from owl_wms import kernels as K  # noqa: E402
from decode_gemm_bench import timeit  # noqa: E402

HBM_PEAK = 8.0e12  # bytes / s (spec)


def shape_case(B, H, D, Lq, Lkv, Lnew, rounds, iters, log):
    hd = H * D
    g = torch.Generator(device="cuda").manual_seed(0)

    def unit(L):
        t = torch.randn(B, L, H, D, device="cuda", generator=g)
        return (t * torch.rsqrt(t.pow(2).mean(-1, keepdim=True))).bfloat16().view(B, L, hd)

    q, k = unit(Lq), unit(Lkv)
    v = torch.randn(B, Lkv, hd, device="cuda", generator=g).bfloat16()
    do = torch.randn(B, Lq, hd, device="cuda", generator=g).bfloat16()
    o, lse = K.attn_fwd(q, k, v, H, D, K.FrameMask(1, None, False, 0, None), score_bound=K.qk_norm_bound(D))
    dq, dk, dv = torch.empty_like(q), torch.empty(B, Lnew, hd, device="cuda", dtype=torch.bfloat16), \
        torch.empty(B, Lnew, hd, device="cuda", dtype=torch.bfloat16)

    def ours():
        K.attn_decode_bwd(q, k, v, o, do, lse, H, D, Lnew, dq, dk, dv)

    # the torch composition: head-major contiguous operands and the saved probabilities
    hm = lambda t, L: t.view(B, L, H, D).permute(0, 2, 1, 3).contiguous()  # noqa: E731
    q4, k4, v4, do4 = hm(q, Lq), hm(k, Lkv), hm(v, Lkv), hm(do, Lq)
    scale = D ** -0.5
    p4 = torch.softmax((q4 @ k4.transpose(-1, -2)).float() * scale, -1).bfloat16()
    res = {}

    def torch_bwd():
        dp = do4 @ v4.transpose(-1, -2)
        ds = torch._softmax_backward_data(dp, p4, -1, torch.bfloat16)
        res["dq"] = (ds @ k4) * scale
        res["dk"] = (ds[..., Lkv - Lnew:].transpose(-1, -2) @ q4) * scale
        res["dv"] = p4[..., Lkv - Lnew:].transpose(-1, -2) @ do4

    # same results first (faster and different is not faster)
    ours()
    torch_bwd()
    torch.cuda.synchronize()
    rel = lambda a, b: ((a.float() - b.float()).norm() / b.float().norm()).item()  # noqa: E731
    back = lambda t, L: t.permute(0, 2, 1, 3).reshape(B, L, hd)  # noqa: E731
    agree = (rel(dq, back(res["dq"], Lq)), rel(dk, back(res["dk"], Lnew)), rel(dv, back(res["dv"], Lnew)))

    t_ours, t_torch = [], []
    for _ in range(rounds):  # alternating
        t_ours.append(timeit(ours, iters=iters, reps=10))
        t_torch.append(timeit(torch_bwd, iters=iters, reps=10))
    floor_us = 2.0 * B * Lkv * hd * 2 / HBM_PEAK * 1e6
    flops = 8.0 * D * H * B * Lq * Lkv
    mo, mt = min(t_ours), min(t_torch)
    line = (f"B {B} H {H:2d} D {D:3d} Lq {Lq} Lkv {Lkv:5d} Lnew {Lnew}: ours min {mo:7.2f} us (median "
            f"{statistics.median(t_ours):7.2f}), torch bf16 min {mt:7.2f} us (median {statistics.median(t_torch):7.2f}), "
            f"torch / ours {mt / mo:5.2f}x; HBM floor {floor_us:5.2f} us = {100 * floor_us / mo:4.1f} % of ours; "
            f"{flops / mo * 1e-6:6.2f} TFLOP/s algorithmic; ours vs torch rel-L2 dq {agree[0]:.1e} dk {agree[1]:.1e} "
            f"dv {agree[2]:.1e}")
    print(line, flush=True)
    log.append(line)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also write the lines to this file")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=50)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU: there is no CPU timing"
    log = [f"device {torch.cuda.get_device_name(0)}; torch {torch.__version__}; HIP graph of {a.iters} calls x 10 "
           f"replays per sample, {a.rounds} alternating rounds; clocks as found (not pinned)"]
    print(log[0], flush=True)
    for H, D in ((24, 64), (20, 128)):
        for B in (1, 4):
            for Lkv in (3840, 1024):
                shape_case(B, H, D, 64, Lkv, 64, a.rounds, a.iters, log)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(log) + "\n")


if __name__ == "__main__":
    main()
