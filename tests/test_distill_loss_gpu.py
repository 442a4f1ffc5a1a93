"""The self-forcing loss tails on libowlk (csrc/distill.hip), on the GPU.

* owlk_dmd_loss / owlk_critic_loss against an fp64 restatement of the reference's tails on the CPU
  (sf_vid_only.py:229-349 written out: mu's, normalizer, nan_to_num, target, 0.5 mse over video[mask],
  autograd for the gradient), from the same bf16- or fp32-valued inputs.
  Bounds: loss within 1e-5 relative; an fp32 gradient within 1e-5 rel-L2; a bf16 gradient within one bf16
  rounding, |a - b| <= 2^-8 |b| + 1e-5 max|b|.  Why they hold: the element math is fp32 with about 20
  roundings of 6e-8 each, the sums are of non-negative terms (fp32 per workgroup, double across them),
  and the normalizer's relative error enters the loss twice -- all well under 1e-5.
  Frames off the mask get exactly zero; a second call gives the same bits.
* get_dmd_loss / get_critic_loss with ``fused=None`` (the kernels) against ``fused=False`` (the torch
  tails) on stub models.

Each figure is printed before it is asserted (pytest -s shows them).
"""
import re

import pytest
import torch
import torch.nn.functional as F
from torch import nn

import conftest  # noqa: F401  (sys.path)

pytestmark = pytest.mark.gpu
BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
DEV = "cuda"

M1 = [[False, False, True, True], [False, True, True, True]]
M2 = [[True] * 5, [False] * 5, [False, True, False, True, True]]  # one sample all true, one all false
#        name      B  N  C    h  mask
SHAPES = {"B2N4C32": (2, 4, 32, 8, M1),
          "B3N5C128": (3, 5, 128, 8, M2),  # 5 * 8192 / 8 chunks per sample: several workgroups each
          "B1N1F8": (1, 1, 8, 1, [[True]])}


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if DEV == "cuda" and not torch.cuda.is_available():
        pytest.skip("no GPU")


def rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-300)).item()


def within_one_bf16_rounding(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return bool(((a - b).abs() <= 2.0 ** -8 * b.abs() + 1e-5 * b.abs().max()).all())


_INPUTS = {}


def inputs(shape, dtype):
    """seeded inputs of one shape, the video side in ``dtype`` (CPU tensors; made once, never modified)"""
    key = (shape, dtype)
    if key not in _INPUTS:
        B, N, C, h, mask = SHAPES[shape]
        g = torch.Generator().manual_seed(sum(map(ord, shape)))
        r = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
        video, z = r(B, N, C, h, h).to(dtype), r(B, N, C, h, h).to(dtype)
        ts = r(B, N).sigmoid()
        e = ts[:, :, None, None, None]
        noisy = (video.float() * (1 - e) + z.float() * e).to(dtype)
        v_cond, v_uncond, v_critic = (r(B, N, C, h, h).to(BF16) for _ in range(3))
        _INPUTS[key] = dict(video=video, z=z, noisy=noisy, ts=ts, mask=torch.tensor(mask), v_cond=v_cond,
                            v_uncond=v_uncond, v_critic=v_critic, pred=r(B, N, C, h, h).to(BF16))
    return _INPUTS[key]


# ------------------------------------------------------------------------------------ fp64 checkers
def ref_dmd(video, noisy, ts, v_cond, v_uncond, v_critic, mask, cfg):
    """sf_vid_only.py:300-349 in float64 -> (loss, d loss / d video)"""
    V = video.double().requires_grad_()
    e = ts.double()[:, :, None, None, None]
    v_teacher = v_cond.double()
    if v_uncond is not None:
        v_teacher = v_uncond.double() + cfg * (v_teacher - v_uncond.double())
    with torch.no_grad():
        mu_teacher = noisy.double() - e * v_teacher
        mu_critic = noisy.double() - e * v_critic.double()
        normalizer = torch.abs(V - mu_teacher).mean(dim=[1, 2, 3, 4], keepdim=True)
        grad = torch.nan_to_num((mu_critic - mu_teacher) / normalizer, nan=0.0)
        target = (V - grad)[mask]
    loss = 0.5 * F.mse_loss(V[mask], target, reduction="mean")
    loss.backward()
    return loss.detach(), V.grad


def ref_critic(pred, z, video, mask):
    """sf_vid_only.py:250-260 in float64 -> (loss, d loss / d pred)"""
    P = pred.double().requires_grad_()
    m = mask[:, :, None, None, None].double()
    loss = F.mse_loss(P * m, (z.double() - video.double()) * m)
    loss.backward()
    return loss.detach(), P.grad


_REFS = {}


def cached_ref(kind, shape, dtype, cfg=None):
    key = (kind, shape, dtype, cfg)
    if key not in _REFS:
        x = inputs(shape, dtype)
        if kind == "dmd":
            _REFS[key] = ref_dmd(x["video"], x["noisy"], x["ts"], x["v_cond"], None if cfg == 1.0 else x["v_uncond"],
                                 x["v_critic"], x["mask"], cfg)
        else:
            _REFS[key] = ref_critic(x["pred"], x["z"], x["video"], x["mask"])
    return _REFS[key]


def run_dmd(x, cfg):
    from owl_wms import kernels as K
    d = {k: v.to(DEV) for k, v in x.items()}
    out = K.dmd_loss(d["video"], d["noisy"], d["v_cond"], None if cfg == 1.0 else d["v_uncond"], d["v_critic"],
                     d["ts"], d["mask"], cfg)
    if DEV == "cuda":
        torch.cuda.synchronize()
    return out


def check_grad(tag, got, want, dtype, mask):
    assert got.dtype == dtype and got.shape == want.shape
    off = ~mask
    assert bool((got.cpu()[off] == 0).all()), f"{tag}: frames off the mask must get exactly zero"
    if dtype == F32:
        e = rel(got, want)
        print(f"{tag}: gradient rel-L2 {e:.2e}")
        assert e <= 1e-5
    else:
        a, b = got.double().cpu(), want.double()
        worst = ((a - b).abs() / (2.0 ** -8 * b.abs() + 1e-5 * b.abs().max())).max().item()
        print(f"{tag}: bf16 gradient, worst error / bound {worst:.3f}")
        assert within_one_bf16_rounding(got, want)


# ------------------------------------------------------------------------------------ the kernels
@pytest.mark.parametrize("dtype", [BF16, F32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("cfg", [1.5, 1.0], ids=["cfg1.5", "cfg1-null-uncond"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_dmd_loss_vs_fp64(shape, cfg, dtype):
    x = inputs(shape, dtype)
    rloss, rgrad = cached_ref("dmd", shape, dtype, cfg)
    loss, dvideo = run_dmd(x, cfg)
    assert loss.dtype == F32 and loss.dim() == 0
    e = abs(loss.item() - rloss.item()) / abs(rloss.item())
    print(f"dmd {shape} cfg {cfg} {dtype}: loss {loss.item():.8e} ref {rloss.item():.8e} rel {e:.2e}")
    assert e <= 1e-5
    check_grad(f"dmd {shape}", dvideo, rgrad, dtype, x["mask"])
    loss2, dvideo2 = run_dmd(x, cfg)  # fixed-order sums: the same bits again
    assert torch.equal(loss, loss2) and torch.equal(dvideo, dvideo2)


@pytest.mark.parametrize("dtype", [BF16, F32], ids=["bf16", "fp32"])
def test_dmd_zero_normalizer_with_critic_equal_teacher(dtype):
    """sample 0: video == noisy and a zero teacher velocity make its normalizer exactly 0; with the critic
    equal to the teacher there, its gradient is 0 / 0 -> nan_to_num -> 0 and the loss stays finite"""
    x = {k: v.clone() for k, v in inputs("B2N4C32", dtype).items()}
    x["noisy"][0] = x["video"][0]
    x["v_cond"][0] = 0
    x["v_critic"][0] = 0
    rloss, rgrad = ref_dmd(x["video"], x["noisy"], x["ts"], x["v_cond"], None, x["v_critic"], x["mask"], 1.0)
    loss, dvideo = run_dmd(x, 1.0)
    assert torch.isfinite(loss) and bool((dvideo[0] == 0).all()) and bool((rgrad[0] == 0).all())
    e = abs(loss.item() - rloss.item()) / abs(rloss.item())
    print(f"dmd zero normalizer {dtype}: loss rel {e:.2e}")
    assert e <= 1e-5
    check_grad("dmd zero normalizer", dvideo, rgrad, dtype, x["mask"])


def test_dmd_all_false_mask():
    """M = 0: the mean over nothing is NaN (as F.mse_loss gives), the gradient all zeros"""
    x = dict(inputs("B2N4C32", BF16))
    x["mask"] = torch.zeros_like(x["mask"])
    loss, dvideo = run_dmd(x, 1.5)
    assert torch.isnan(loss) and bool((dvideo == 0).all())


@pytest.mark.parametrize("dtype", [BF16, F32], ids=["bf16", "fp32"])
def test_dmd_backward_scales_the_gradient(dtype):
    """through the autograd function: (loss * 0.25).backward() leaves 0.25 x dvideo, within one rounding"""
    from owl_wms.trainers import self_forcing as SF
    x = {k: v.to(DEV) for k, v in inputs("B2N4C32", dtype).items()}
    _, dvideo = run_dmd(inputs("B2N4C32", dtype), 1.5)
    video = x["video"].clone().requires_grad_()
    loss = SF._DMDLossFn.apply(video, x["noisy"], x["ts"], x["v_cond"], x["v_uncond"], x["v_critic"], x["mask"], 1.5)
    (loss * 0.25).backward()
    assert video.grad.dtype == dtype
    want = 0.25 * dvideo.double()
    ulp = 2.0 ** -8 if dtype == BF16 else 2.0 ** -24
    assert bool(((video.grad.double() - want).abs() <= ulp * want.abs()).all())
    assert bool((video.grad.cpu()[~inputs("B2N4C32", dtype)["mask"]] == 0).all())


@pytest.mark.parametrize("dtype", [BF16, F32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_critic_loss_vs_fp64(shape, dtype):
    from owl_wms import kernels as K
    x = inputs(shape, dtype)
    rloss, rgrad = cached_ref("critic", shape, dtype)

    def run():
        out = K.critic_loss(x["pred"].to(DEV), x["z"].to(DEV), x["video"].to(DEV), x["mask"].to(DEV))
        if DEV == "cuda":
            torch.cuda.synchronize()
        return out

    loss, dpred = run()
    assert loss.dtype == F32 and loss.dim() == 0
    e = abs(loss.item() - rloss.item()) / abs(rloss.item())
    print(f"critic {shape} {dtype}: loss {loss.item():.8e} ref {rloss.item():.8e} rel {e:.2e}")
    assert e <= 1e-5
    check_grad(f"critic {shape}", dpred, rgrad, BF16, x["mask"])
    loss2, dpred2 = run()
    assert torch.equal(loss, loss2) and torch.equal(dpred, dpred2)


def test_critic_backward_scales_the_gradient():
    from owl_wms import kernels as K
    from owl_wms.trainers import self_forcing as SF
    x = {k: v.to(DEV) for k, v in inputs("B2N4C32", BF16).items()}
    _, dpred = K.critic_loss(x["pred"], x["z"], x["video"], x["mask"])
    pred = x["pred"].clone().requires_grad_()
    (SF._CriticLossFn.apply(pred, x["z"], x["video"], x["mask"]) * 0.25).backward()
    want = 0.25 * dpred.double()
    assert pred.grad.dtype == BF16 and bool(((pred.grad.double() - want).abs() <= 2.0 ** -8 * want.abs()).all())


def test_refusals():
    """F % 8 != 0 is refused by the library with its message; tensors that do not fit each other by the binding"""
    from owl_wms import kernels as K
    t = lambda *s, dt=BF16: torch.zeros(*s, dtype=dt, device=DEV)  # noqa: E731
    m = torch.ones(1, 1, dtype=torch.bool, device=DEV)
    with pytest.raises(RuntimeError, match=re.escape("dmd_loss: F=12 elements per frame must be a multiple of 8")):
        K.dmd_loss(t(1, 1, 12), t(1, 1, 12), t(1, 1, 12), None, t(1, 1, 12), t(1, 1, dt=F32), m, 1.0)
    with pytest.raises(RuntimeError, match=re.escape("critic_loss: F=12 elements per frame must be a multiple of 8")):
        K.critic_loss(t(1, 1, 12), t(1, 1, 12), t(1, 1, 12), m)
    with pytest.raises(RuntimeError, match="dmd_loss: v_critic has shape"):
        K.dmd_loss(t(1, 1, 16), t(1, 1, 16), t(1, 1, 16), None, t(1, 1, 8), t(1, 1, dt=F32), m, 1.0)
    with pytest.raises(RuntimeError, match="dmd_loss: mask has shape"):
        K.dmd_loss(t(1, 1, 16), t(1, 1, 16), t(1, 1, 16), None, t(1, 1, 16), t(1, 1, dt=F32), m.expand(1, 2), 1.0)
    with pytest.raises(RuntimeError, match="critic_loss: z has shape"):
        K.critic_loss(t(1, 1, 16), t(1, 2, 16), t(1, 1, 16), m)
    with pytest.raises(RuntimeError, match="dmd_loss: v_critic must be torch.bfloat16"):
        K.dmd_loss(t(1, 1, 16), t(1, 1, 16), t(1, 1, 16), None, t(1, 1, 16, dt=F32), t(1, 1, dt=F32), m, 1.0)


# ------------------------------------------------------------------------------------ the loss functions
class _Lin(nn.Module):
    """velocity = a x + b ts + c sum(mouse) + 0.1 sum(btn), as the CPU formula tests' stub (fp32 out)"""

    def __init__(self, a, b, c):
        super().__init__()
        self.a, self.b, self.c = nn.Parameter(torch.tensor(a)), b, c

    def forward(self, x, ts, mouse, btn, kv_cache=None):
        e = lambda t: t[:, :, None, None, None]  # noqa: E731
        return self.a * x + self.b * e(ts) + self.c * e(mouse.sum(-1)) + 0.1 * e(btn.sum(-1))


class _FixedRollout:
    """a rollout manager whose rollout is given; the value is unchanged, the gradient reaches the student"""

    def __init__(self, video, mouse, btn, mask, noise):
        self.out, self.noise_source = (video, mouse, btn, mask), noise

    def get_rollouts(self, model, video, mouse, btn):
        v, m, b, g = self.out
        return v * model.a / model.a.detach(), m, b, g


def _stub_setup():
    from owl_wms.trainers import self_forcing as SF
    x = inputs("B2N4C32", F32)
    g = torch.Generator().manual_seed(9)
    mouse, btn = torch.randn(2, 4, 2, generator=g).to(DEV), torch.rand(2, 4, 5, generator=g).round().to(DEV)
    ts_raw = torch.randn(2, 4, generator=g).to(DEV)
    video, z, mask = x["video"].to(DEV), x["z"].to(DEV), x["mask"].to(DEV)
    rm = lambda: _FixedRollout(video, mouse, btn, mask, SF.InjectedRolloutNoise([ts_raw, z]))  # noqa: E731
    return SF, rm, video, mouse, btn


def _agree(tag, a, b):
    e = abs(a - b) / abs(b)
    print(f"{tag}: fused {a:.8e} torch {b:.8e} rel {e:.2e}")
    assert e <= 1e-4


@pytest.mark.parametrize("cfg", [1.5, 1.0])
def test_get_dmd_loss_fused_matches_torch_tail(cfg):
    SF, rm, video, mouse, btn = _stub_setup()
    res = {}
    for fused in (None, False):
        student, critic, teacher = (_Lin(*p).to(DEV) for p in ((1.0, 0.0, 0.0), (0.7, 0.3, 0.2), (0.9, -0.2, 0.4)))
        loss = SF.get_dmd_loss(student, critic, teacher, video, mouse, btn, rm(), cfg_scale=cfg, fused=fused)
        loss.backward()
        assert critic.a.grad is None and teacher.a.grad is None  # only the student learns from this loss
        res[fused] = (loss.item(), student.a.grad.item())
    _agree(f"get_dmd_loss cfg {cfg}: loss", res[None][0], res[False][0])
    _agree(f"get_dmd_loss cfg {cfg}: d/d student.a", res[None][1], res[False][1])


def test_get_critic_loss_fused_matches_torch_tail():
    SF, rm, video, mouse, btn = _stub_setup()
    res = {}
    for fused in (None, False):
        student, critic = _Lin(1.0, 0.0, 0.0).to(DEV), _Lin(0.7, 0.3, 0.2).to(DEV)
        loss = SF.get_critic_loss(student, critic, video, mouse, btn, rm(), fused=fused)
        loss.backward()
        assert student.a.grad is None  # no gradient to the student
        res[fused] = (loss.item(), critic.a.grad.item())
    _agree("get_critic_loss: loss", res[None][0], res[False][0])
    _agree("get_critic_loss: d/d critic.a", res[None][1], res[False][1])
