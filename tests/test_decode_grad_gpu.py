"""Gradients through the KV-cache decode step, on the GPU.

* owlk_attn_decode_bwd against fp32 autograd of softmax(scale q k^T) v on the CPU (rel-L2 < 1e-2 per
  output: the per-op bound of the attention tests), with canaries around every output
  view and a bitwise repeat;
* GameRFTCore's decode step with a gradient against the CPU oracle under bf16 autocast (bounds of
  test_model_gpu.py: output / input-gradient / weight-gradient rel-L2 < 2e-2, gradient norms within
  5e-2), with the cache mutated before backward(), and against the no-grad decode forward;
* RolloutManager against a restatement of the reference rollout (sf_vid_only.py:112-225) over the oracle.

Each figure is printed before it is asserted (pytest -s shows them).
"""
import random
from types import SimpleNamespace

import pytest
import torch

import conftest  # noqa: F401  (sys.path)
from oracle.params import det_init_, det_tensor

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16

TINY = dict(model_id="game_rft", sample_size=8, channels=32, n_layers=2, n_heads=2, d_model=128,
            tokens_per_frame=64, n_buttons=11, cfg_prob=0.1, n_frames=8, causal=True, uncond=False,
            backbone="dit", has_audio=False, rope_impl="motion", rope_ats_delta=2.0, local_window=2,
            global_window=None)


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


# ------------------------------------------------------------------------------------ 4. the kernel
#        B  H  D    Lq   Lkv   Lnew
CASES = [(2, 2, 64, 64, 384, 64),     # base case
         (1, 2, 128, 64, 384, 64),    # head_dim 128
         (1, 3, 64, 64, 64, 64),      # no cache
         (1, 2, 64, 65, 325, 65),     # nothing a multiple of 16
         (1, 2, 64, 64, 1000, 64),    # ragged last split
         (1, 2, 64, 128, 448, 128),   # two frames at once
         (1, 2, 64, 64, 4160, 64),    # many splits
         (1, 1, 128, 64, 4160, 64),   # many splits, head_dim 128
         (1, 2, 64, 64, 320, 0)]      # no new rows, null dk / dv
CANARY = 7.0


def _canary_view(B, L, cols):
    """a [B, L, cols] view strictly inside a canary-filled tensor, and that tensor"""
    buf = torch.full((B, L + 2, cols + 16), CANARY, device="cuda", dtype=BF16)
    return buf[:, 1:L + 1, 8:8 + cols], buf


def _outside_untouched(buf, L, cols):
    m = torch.ones_like(buf, dtype=torch.bool)
    m[:, 1:L + 1, 8:8 + cols] = False
    return bool((buf[m] == CANARY).all())


@pytest.mark.parametrize("case", CASES, ids=lambda c: "B%d-H%d-D%d-Lq%d-Lkv%d-new%d" % c)
def test_attn_decode_bwd_vs_fp32_autograd(case):
    from owl_wms import kernels as K
    B, H, D, Lq, Lkv, Lnew = case
    hd = H * D
    g = torch.Generator().manual_seed(17)

    def unit(*shape):  # RMS-normalised per head, as QK-RMSNorm leaves q and k: the forward's score bound holds
        t = torch.randn(*shape, H, D, generator=g)
        return (t / t.pow(2).mean(-1, keepdim=True).sqrt()).reshape(*shape, hd)

    # strided token-major views, as the block passes them: q inside [B, Lq, 2 H D], k | v inside [B, Lkv, 3 H D]
    qbuf = torch.zeros(B, Lq, 2 * hd, dtype=BF16)
    qbuf[:, :, :hd] = unit(B, Lq).to(BF16)
    kvbuf = torch.zeros(B, Lkv, 3 * hd, dtype=BF16)
    kvbuf[:, :, hd:2 * hd] = unit(B, Lkv).to(BF16)
    kvbuf[:, :, 2 * hd:] = torch.randn(B, Lkv, hd, generator=g).to(BF16)
    do_c = torch.randn(B, Lq, hd, generator=g).to(BF16)
    qg, kvg, do = qbuf.cuda(), kvbuf.cuda(), do_c.cuda()
    q, k, v = qg[:, :, :hd], kvg[:, :, hd:2 * hd], kvg[:, :, 2 * hd:]
    o, lse = K.attn_fwd(q, k, v, H, D, K.FrameMask(1, None, False, 0, None), score_bound=K.qk_norm_bound(D))

    def run():
        dq, dq_buf = _canary_view(B, Lq, hd)
        dk, dk_buf = _canary_view(B, Lnew, hd) if Lnew else (None, None)
        dv, dv_buf = _canary_view(B, Lnew, hd) if Lnew else (None, None)
        K.attn_decode_bwd(q, k, v, o, do, lse, H, D, Lnew, dq, dk, dv)
        torch.cuda.synchronize()
        return (dq, dk, dv), (dq_buf, dk_buf, dv_buf)

    (dq, dk, dv), bufs = run()
    for buf, L in zip(bufs, (Lq, Lnew, Lnew)):
        assert buf is None or _outside_untouched(buf, L, hd), "wrote outside its output view"

    # fp32 autograd on the CPU from the same bf16 inputs
    heads = lambda t, L: t.float().view(B, L, H, D).permute(0, 2, 1, 3)  # noqa: E731
    q32 = heads(qbuf[:, :, :hd], Lq).requires_grad_()
    k32 = heads(kvbuf[:, :, hd:2 * hd], Lkv).requires_grad_()
    v32 = heads(kvbuf[:, :, 2 * hd:], Lkv).requires_grad_()
    o32 = torch.softmax(q32 @ k32.transpose(-1, -2) * D ** -0.5, -1) @ v32
    o32.backward(heads(do_c, Lq))
    flat = lambda t, L: t.permute(0, 2, 1, 3).reshape(B, L, hd)  # noqa: E731
    assert rel(o, flat(o32.detach(), Lq)) < 1e-2
    figs = {"dq": rel(dq, flat(q32.grad, Lq))}
    if Lnew:
        figs["dk_new"] = rel(dk, flat(k32.grad, Lkv)[:, Lkv - Lnew:])
        figs["dv_new"] = rel(dv, flat(v32.grad, Lkv)[:, Lkv - Lnew:])
    print("attn_decode_bwd", case, {n: f"{x:.2e}" for n, x in figs.items()})
    for n, x in figs.items():
        assert x < 1e-2, (n, x)

    # determinism: a second call gives the same bits (outputs and canaries)
    _, bufs2 = run()
    for a, b in zip(bufs, bufs2):
        assert a is None or torch.equal(a, b)


# ------------------------------------------------------------------------------------ model level
class OracleCache:
    """The reference KV cache's interface as oracle.ref_model reads it (K / V as [B, H, T, D], detached)."""

    def __init__(self, n_layers, tpf):
        self.kv, self.off, self.should_update, self.tpf = [None] * n_layers, [0] * n_layers, False, tpf

    def offset(self, i):
        return self.off[i]

    def length(self):
        return 0 if self.kv[0] is None else self.kv[0][0].shape[2]

    def get(self, i):
        return self.kv[i]

    def update(self, i, k, v):
        self.off[i] += k.shape[2] - (0 if self.kv[i] is None else self.kv[i][0].shape[2])
        self.kv[i] = (k.detach(), v.detach())

    def truncate_oldest(self, frames):
        self.kv = [(k[:, :, frames * self.tpf:], v[:, :, frames * self.tpf:]) for k, v in self.kv]


def _inputs(B, n, seed):
    return (det_tensor((B, n, 32, 8, 8), seed).to(BF16), det_tensor((B, n), seed + 1).sigmoid().to(BF16),
            det_tensor((B, n, 2), seed + 2).to(BF16), (det_tensor((B, n, 11), seed + 3) > 0).to(BF16))


def _cuda(ts):
    return tuple(t.cuda() for t in ts)


B, NCTX = 2, 5
W_LOSS = det_tensor((B, 1, 32, 8, 8), 77)


def _our_core(d_model):
    from owl_wms.configs import model_config
    from owl_wms.models.gamerft import GameRFTCore
    cfg = model_config(**dict(TINY, d_model=d_model))
    return det_init_(GameRFTCore(cfg), base_seed=1000).cuda().train(), cfg


def _our_decode(d_model, mutate=False, grad=True):
    """5 context frames cached without grad, the 6th decoded (with grad: loss = sum(out * w), backward;
    mutate: between forward and backward the cache takes another frame and ejects its oldest, as the
    rollout does).  -> (out, x.grad, {name: grad})"""
    from owl_wms.nn.kv_cache import KVCache
    core, cfg = _our_core(d_model)
    cache = KVCache(cfg)
    cache.reset(B)
    with torch.no_grad():
        cache.enable_cache_updates()
        core(*_cuda(_inputs(B, NCTX, 1)), kv_cache=cache)
        cache.disable_cache_updates()
    core.transformer.enable_decoding()
    x, ts, mouse, btn = _cuda(_inputs(B, 1, 11))
    if not grad:
        with torch.no_grad():
            return core(x, ts, mouse, btn, kv_cache=cache), None, None
    x.requires_grad_()
    out = core(x, ts, mouse, btn, kv_cache=cache)
    assert out.grad_fn is not None, "the decode step carries no gradient"
    loss = (out.float() * W_LOSS.cuda()).sum()
    if mutate:
        with torch.no_grad():
            cache.enable_cache_updates()
            core(*_cuda(_inputs(B, 1, 21)), kv_cache=cache)
            cache.disable_cache_updates()
            cache.truncate(1, front=False)
    loss.backward()
    torch.cuda.synchronize()
    return out.detach(), x.grad, {n: p.grad for n, p in core.named_parameters()}


def _oracle_decode(d_model):
    from oracle import ref_model as M
    ref = det_init_(M.GameRFTCore(SimpleNamespace(**dict(TINY, d_model=d_model))), base_seed=1000).train()
    cache = OracleCache(TINY["n_layers"], TINY["tokens_per_frame"])
    # the context pass and the decode pass in SEPARATE autocast contexts: in one, the weight casts cached
    # under no_grad would leave every parameter gradient None
    with torch.no_grad(), torch.autocast("cpu", dtype=BF16):
        cache.should_update = True
        ref(*_inputs(B, NCTX, 1), cache=cache)
        cache.should_update = False
    ref.transformer.decoding = True
    x, ts, mouse, btn = _inputs(B, 1, 11)
    x.requires_grad_()
    with torch.autocast("cpu", dtype=BF16):
        out = ref(x, ts, mouse, btn, cache=cache)
    (out.float() * W_LOSS).sum().backward()
    return out.detach(), x.grad, {n: p.grad for n, p in ref.named_parameters()}


_RUNS = {}


def _cached(kind, d_model, **kw):
    key = (kind, d_model, tuple(sorted(kw.items())))
    if key not in _RUNS:
        _RUNS[key] = (_our_decode if kind == "ours" else _oracle_decode)(d_model, **kw)
    return _RUNS[key]


@pytest.mark.parametrize("d_model", [128, 256])
def test_decode_step_grads_vs_oracle(d_model):
    """Layer 0 is global (384 keys), layer 1 local (128 keys); d_model 256 is head_dim 128."""
    out, dx, grads = _cached("ours", d_model)
    rout, rdx, rgrads = _cached("oracle", d_model)
    assert set(grads) == set(rgrads)
    print(f"decode d{d_model}: out {rel(out, rout):.2e}  dx {rel(dx, rdx):.2e}")
    worst = 0.0
    for n in sorted(grads):
        assert grads[n] is not None and rgrads[n] is not None, n
        a, b = grads[n].double().norm().item(), rgrads[n].double().norm().item()
        assert b > 0, n
        e = rel(grads[n], rgrads[n])
        worst = max(worst, e)
        print(f"  {n:48s} norm {a:.4e} / {b:.4e} ({abs(a - b) / b:.1e})  rel-L2 {e:.2e}")
    print(f"  worst elementwise rel-L2 over all parameters: {worst:.2e}")
    assert rel(out, rout) < 2e-2
    assert rel(dx, rdx) < 2e-2
    for n in sorted(grads):
        a, b = grads[n].double().norm().item(), rgrads[n].double().norm().item()
        assert abs(a - b) <= 5e-2 * b + 1e-7, n
    for blk in (0, 1):
        for w in ("attn.qkv", "attn.out", "mlp.fc1", "mlp.fc2"):
            n = f"transformer.blocks.{blk}.{w}.weight"
            assert rel(grads[n], rgrads[n]) < 2e-2, (n, rel(grads[n], rgrads[n]))


def test_cache_mutated_before_backward():
    """The rollout overwrites the new frame's cache slots, appends and ejects frames before backward():
    the block's own K/V snapshot keeps the gradients bit for bit."""
    out, dx, grads = _cached("ours", 128)
    out2, dx2, grads2 = _cached("ours", 128, mutate=True)
    assert torch.equal(out, out2) and torch.equal(dx, dx2)
    for n in grads:
        assert torch.equal(grads[n], grads2[n]), n


def test_grad_path_forward_matches_no_grad_decode():
    out, _, _ = _cached("ours", 128)
    ref, _, _ = _cached("ours", 128, grad=False)
    print(f"grad-path forward vs no-grad decode: rel-L2 {rel(out, ref):.2e}, bitwise equal: {torch.equal(out, ref)}")
    assert rel(out, ref) < 5e-3


# ------------------------------------------------------------------------------------ 8. the rollout
def _oracle_rollout(ref, video, mouse, btn, ext_mouse, ext_btn, draws, n_roll):
    """sf_vid_only.py:112-225 over the oracle core (rollout_steps = 1: every frame is one step with grad)"""
    cache = OracleCache(TINY["n_layers"], TINY["tokens_per_frame"])
    window = video.shape[1]
    with torch.no_grad(), torch.autocast("cpu", dtype=BF16):
        cache.should_update = True
        ref(video, torch.zeros_like(video[:, :, 0, 0, 0]), mouse, btn, cache=cache)
        cache.should_update = False
    ref.transformer.decoding = True
    for f in range(n_roll):
        ts_1 = torch.ones_like(video[:, 0:1, 0, 0, 0])
        frame = draws[f]
        m1, b1 = ext_mouse[:, window + f:window + f + 1], ext_btn[:, window + f:window + f + 1]
        with torch.autocast("cpu", dtype=BF16):
            v = ref(frame, ts_1, m1, b1, cache=cache)
        frame = frame - ts_1[:, :, None, None, None] * v
        with torch.no_grad(), torch.autocast("cpu", dtype=BF16):
            cache.should_update = True
            ref(frame, ts_1 * 0, m1, b1, cache=cache)
            cache.should_update = False
            cache.truncate_oldest(1)
        video = torch.cat([video, frame], dim=1)
    ref.transformer.decoding = False
    return video[:, -window:]


def test_rollout_vs_oracle_rollout(monkeypatch):
    from oracle import ref_model as M
    from owl_wms.trainers import self_forcing as SF
    n_ctx, n_roll = 4, 2  # offsets reach 6 of the 8-frame RoPE table
    video, _, mouse, btn = _inputs(B, n_ctx, 31)
    draws = [det_tensor((B, 1, 32, 8, 8), 41 + i).to(BF16) for i in range(n_roll)]
    target = det_tensor((B * n_roll, 32, 8, 8), 51)
    torch.manual_seed(0)
    ext_mouse, ext_btn = SF.batch_permute_to_length(mouse, btn, n_ctx + n_roll)
    # both sides get the same extended controls
    monkeypatch.setattr(SF, "batch_permute_to_length",
                        lambda m, b, n: (ext_mouse.to(m.device), ext_btn.to(m.device)))

    core, cfg = _our_core(128)
    rm = SF.RolloutManager(cfg, min_rollout_frames=n_roll, rollout_steps=1,
                           noise_source=SF.InjectedRolloutNoise(draws))
    random.seed(0)
    out, m2, b2, gmask = rm.get_rollouts(core, video.cuda(), mouse.cuda(), btn.cuda())
    assert out.shape == video.shape and torch.equal(gmask.cpu(), torch.tensor([[False, False, True, True]] * B))
    assert torch.equal(m2.cpu(), ext_mouse[:, -n_ctx:]) and torch.equal(b2.cpu(), ext_btn[:, -n_ctx:])
    assert not core.transformer.decoding
    (0.5 * torch.nn.functional.mse_loss(out[gmask].float(), target.cuda())).backward()
    torch.cuda.synchronize()

    ref = det_init_(M.GameRFTCore(SimpleNamespace(**TINY)), base_seed=1000).train()
    rout = _oracle_rollout(ref, video, mouse, btn, ext_mouse, ext_btn, draws, n_roll)
    (0.5 * torch.nn.functional.mse_loss(rout[gmask.cpu()].float(), target)).backward()

    assert torch.equal(out[:, :2].cpu(), video[:, -2:])  # the context frames pass through
    e = rel(out[:, 2:], rout[:, 2:])
    print(f"rollout: generated frames rel-L2 {e:.2e}")
    rgrads = dict(ref.named_parameters())
    figs = []
    for n, p in core.named_parameters():
        if ".blocks." in n and n.endswith(".weight"):
            a, b = p.grad.double().norm().item(), rgrads[n].grad.double().norm().item()
            print(f"  {n:48s} norm {a:.4e} / {b:.4e} ({abs(a - b) / b:.1e})")
            figs.append((n, a, b))
    assert e < 2e-2
    assert len(figs) == 2 * 8
    for n, a, b in figs:
        assert abs(a - b) <= 5e-2 * b, n
