"""The CausVid tails on libowlk (csrc/distill.hip: owlk_causvid_mix, owlk_causvid_x0, owlk_causvid_gen_loss),
on the GPU.

* each kernel against an fp64 restatement of the reference's lines on the CPU (causvid_vid_only.py:142-162 for the
  noising and the one-step denoise, :268-306 for the generator loss with autograd for the gradient to the
  student's velocity), from the same bf16- or fp32-valued inputs.
  Bounds, those of test_distill_loss_gpu.py, whose argument carries over with two more fp32 roundings per
  element (r = out - orig and the g + 2 w r sum): losses within 1e-5 relative; an fp32 dv (and an fp32 noisy /
  out, three fp32 roundings of 6e-8) within 1e-5 rel-L2; a bf16 dv, noisy or out within one bf16 rounding,
  |a - b| <= 2^-8 |b| + 1e-5 max|b|.  dv is exactly zero off the mask, out there is clean bit for bit, ts_full is
  exact, a second call gives the same bits.
* get_gen_loss / get_critic_loss with ``fused=None`` (the kernels) against ``fused=False`` (the torch tails) on
  stub models, for the video and the audio + video form, to 1e-4.

Each figure is printed before it is asserted (pytest -s shows them).
"""
import pytest
import torch
from torch import nn

import conftest  # noqa: F401  (sys.path)

pytestmark = pytest.mark.gpu
BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
DEV = "cuda"
NOISE_PREV = 0.2

M1 = [[False, False, True, True], [False, True, True, True]]
M2 = [[True] * 5, [False] * 5, [False, True, False, True, True]]  # one sample all true, one all false
#          name         frame shape   mask
SHAPES = {"B2N4F2048": ((32, 8, 8), M1),
          "B3N5F8192": ((128, 8, 8), M2),  # 5 * 8192 / 8 chunks per sample: several workgroups each
          "B1N1F8": ((8,), [[True]]),
          "B2N4F16": ((16,), M1)}  # the tiny audio latents
DTYPES = [(BF16, BF16), (F32, F32), (BF16, F32)]  # (latents, velocities)
DT_IDS = ["bf16", "fp32", "bf16-v32"]


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _e(t, like):
    return t.reshape(t.shape + (1,) * (like.dim() - 2))


_INPUTS = {}


def inputs(shape, dt, vdt):
    """seeded inputs of one shape (CPU tensors; made once, never modified)"""
    key = (shape, dt, vdt)
    if key not in _INPUTS:
        frame, mask = SHAPES[shape]
        mask = torch.tensor(mask)
        B, N = mask.shape
        g = torch.Generator().manual_seed(sum(map(ord, shape)))
        r = lambda dtype: torch.randn(B, N, *frame, generator=g).to(dtype)  # noqa: E731
        x = dict(mask=mask, clean=r(dt), z=r(dt), noisy=r(dt), out=r(dt), noisy2=r(dt), v=r(vdt), v_cond=r(vdt),
                 v_uncond=r(vdt), v_critic=r(vdt))
        x["orig"] = (x["out"].float() + 0.5 * torch.randn(B, N, *frame, generator=g)).to(dt)
        x["ts"] = torch.tensor([1.0, 0.5])[torch.randint(0, 2, (B, N), generator=g)]
        x["ts2"] = torch.randn(B, N, generator=g).sigmoid()
        x["ts_full"] = torch.where(mask, x["ts"], torch.tensor(NOISE_PREV))
        _INPUTS[key] = x
    return _INPUTS[key]


# ------------------------------------------------------------------------------------ fp64 checkers
def ref_mix(x, z, ts, mask, noise_prev):
    """causvid_vid_only.py:142-147 (mask None: lerp_batched, :196) in float64 -> (noisy, ts_full)"""
    t = ts.float() if mask is None else torch.where(mask, ts.float(), torch.tensor(noise_prev, dtype=F32))
    e = _e(t.double(), x)
    return x.double() * (1 - e) + z.double() * e, t


def ref_x0(noisy, clean, v, ts_full, mask):
    """:158-162 in float64"""
    return torch.where(_e(mask, noisy), noisy.double() - v.double() * _e(ts_full.double(), noisy), clean.double())


def ref_gen(x, cfg, w):
    """:255-306 in float64 -> (dmd, regression, d (dmd + w regression) / d v).  ``out`` keeps its given value and
    carries the gradient path of out = noisy - ts_full v on the mask's frames."""
    V = x["v"].double().requires_grad_()
    m = _e(x["mask"], V).double()
    out = x["out"].double() - _e(x["ts_full"].double(), V) * m * (V - V.detach())
    e = _e(x["ts2"].double(), V)
    v_teacher = x["v_cond"].double()
    if cfg != 1.0:
        v_teacher = x["v_uncond"].double() + cfg * (v_teacher - x["v_uncond"].double())
    with torch.no_grad():
        mu_teacher = x["noisy2"].double() - e * v_teacher
        mu_critic = x["noisy2"].double() - e * x["v_critic"].double()
        normalizer = torch.abs(out - mu_teacher).mean(dim=list(range(1, out.dim())), keepdim=True)
        grad = torch.nan_to_num((mu_critic - mu_teacher) / normalizer, nan=0.0)
        target = (out - grad).detach()
    dmd = 0.5 * ((out * m - target * m) ** 2).mean()
    reg = ((out * m - x["orig"].double() * m) ** 2).mean()
    (dmd + w * reg).backward()
    return dmd.detach(), reg.detach(), V.grad


_REFS = {}


def cached_ref_gen(shape, dt, vdt, cfg, w):
    key = (shape, dt, vdt, cfg, w)
    if key not in _REFS:
        _REFS[key] = ref_gen(inputs(shape, dt, vdt), cfg, w)
    return _REFS[key]


def rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-300)).item()


def check_tensor(tag, got, want, dtype):
    """fp32: 1e-5 rel-L2; bf16: within one rounding"""
    assert got.dtype == dtype and got.shape == want.shape, (tag, got.dtype, got.shape)
    if dtype == F32:
        e = rel(got, want)
        print(f"{tag}: fp32, rel-L2 {e:.2e}")
        assert e <= 1e-5
    else:
        a, b = got.double().cpu(), want.double()
        bound = 2.0 ** -8 * b.abs() + 1e-5 * b.abs().max()
        worst = ((a - b).abs() / bound.clamp_min(1e-300)).max().item() if b.abs().max() > 0 else float(a.abs().max())
        print(f"{tag}: bf16, worst error / bound {worst:.3f}")
        assert bool(((a - b).abs() <= bound).all())


def check_loss(tag, got, want):
    e = abs(got - want) / abs(want) if want != 0 else abs(got)
    print(f"{tag}: {got:.8e} ref {want:.8e} rel {e:.2e}")
    assert e <= 1e-5


def run_gen(x, cfg, w):
    from owl_wms import kernels as K
    d = {k: v.to(DEV) for k, v in x.items()}
    out = K.causvid_gen_loss(d["out"], d["orig"], d["noisy2"], d["v_cond"], None if cfg == 1.0 else d["v_uncond"],
                             d["v_critic"], d["ts2"], d["ts_full"], d["mask"], cfg, w)
    torch.cuda.synchronize()
    return out


# ------------------------------------------------------------------------------------ the kernels
@pytest.mark.parametrize("masked", [True, False], ids=["rollout", "null-mask"])
@pytest.mark.parametrize("dt", [BF16, F32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_mix_vs_fp64(shape, dt, masked):
    from owl_wms import kernels as K
    x = inputs(shape, dt, BF16)
    ts, mask = (x["ts"], x["mask"]) if masked else (x["ts2"], None)
    want, want_t = ref_mix(x["clean"], x["z"], ts, mask, NOISE_PREV)

    def run():
        out = K.causvid_mix(x["clean"].to(DEV), x["z"].to(DEV), ts.to(DEV), None if mask is None else mask.to(DEV),
                            NOISE_PREV)
        torch.cuda.synchronize()
        return out

    noisy, ts_full = run()
    assert ts_full.dtype == F32 and torch.equal(ts_full.cpu(), want_t)  # exact
    check_tensor(f"mix {shape} masked={masked}", noisy, want, dt)
    noisy2, ts_full2 = run()
    assert torch.equal(noisy, noisy2) and torch.equal(ts_full, ts_full2)


@pytest.mark.parametrize("dt,vdt", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("shape", list(SHAPES))
def test_x0_vs_fp64(shape, dt, vdt):
    from owl_wms import kernels as K
    x = inputs(shape, dt, vdt)
    want = ref_x0(x["noisy"], x["clean"], x["v"], x["ts_full"], x["mask"])

    def run():
        out = K.causvid_x0(*(x[k].to(DEV) for k in ("noisy", "clean", "v", "ts_full", "mask")))
        torch.cuda.synchronize()
        return out

    out = run()
    check_tensor(f"x0 {shape}", out, want, dt)
    off = ~x["mask"]
    bits = torch.int16 if dt == BF16 else torch.int32
    assert torch.equal(out.cpu()[off].view(bits), x["clean"][off].view(bits)), "frames off the mask: clean, bit for bit"
    assert torch.equal(out, run())


@pytest.mark.parametrize("dt,vdt", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("cfg,w", [(1.5, 0.0), (1.5, 0.5), (1.0, 0.5)], ids=["cfg1.5-w0", "cfg1.5-w0.5",
                                                                             "cfg1-null-uncond-w0.5"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_gen_loss_vs_fp64(shape, cfg, w, dt, vdt):
    x = inputs(shape, dt, vdt)
    rdmd, rreg, rdv = cached_ref_gen(shape, dt, vdt, cfg, w)
    losses, dv = run_gen(x, cfg, w)
    assert losses.dtype == F32 and tuple(losses.shape) == (2,)
    tag = f"gen {shape} cfg {cfg} w {w} {dt}/{vdt}"
    check_loss(f"{tag}: dmd", losses[0].item(), rdmd.item())
    check_loss(f"{tag}: regression", losses[1].item(), rreg.item())
    assert bool((dv.cpu()[~x["mask"]] == 0).all()), "frames off the mask must get exactly zero"
    check_tensor(f"{tag}: dv", dv, rdv, vdt)
    losses2, dv2 = run_gen(x, cfg, w)  # fixed-order sums: the same bits again
    assert torch.equal(losses, losses2) and torch.equal(dv, dv2)


@pytest.mark.parametrize("dt,vdt", DTYPES[:2], ids=DT_IDS[:2])
def test_gen_zero_normalizer_with_critic_equal_teacher(dt, vdt):
    """sample 0: out == noisy2 and a zero teacher velocity make its normalizer exactly 0; with the critic equal to
    the teacher there, g is 0 / 0 -> nan_to_num -> 0: the losses stay finite and dv there is the regression's"""
    x = {k: v.clone() for k, v in inputs("B2N4F2048", dt, vdt).items()}
    x["noisy2"][0] = x["out"][0]
    x["v_cond"][0] = 0
    x["v_critic"][0] = 0
    rdmd, rreg, rdv = ref_gen(x, 1.0, 0.5)
    losses, dv = run_gen(x, 1.0, 0.5)
    assert bool(torch.isfinite(losses).all()) and bool(torch.isfinite(dv).all())
    check_loss("gen zero normalizer: dmd", losses[0].item(), rdmd.item())
    check_loss("gen zero normalizer: regression", losses[1].item(), rreg.item())
    check_tensor("gen zero normalizer: dv", dv, rdv, vdt)
    x0 = dict(x, orig=x["out"])  # and without a regression term: nothing at all on sample 0
    _, dv0 = run_gen(x0, 1.0, 0.5)
    assert bool((dv0[0] == 0).all())


def test_gen_all_false_mask():
    """no generated frame: both losses are 0 (means over every element, not over the mask's), dv all zeros"""
    x = dict(inputs("B2N4F2048", BF16, BF16))
    x["mask"] = torch.zeros_like(x["mask"])
    losses, dv = run_gen(x, 1.5, 0.5)
    print("all-false mask:", losses.tolist())
    assert losses.tolist() == [0.0, 0.0] and bool((dv == 0).all())


@pytest.mark.parametrize("dt,vdt", DTYPES[:2], ids=DT_IDS[:2])
def test_gen_backward_scales_the_gradient(dt, vdt):
    """through the autograd function: (gen * 0.25).backward() leaves 0.25 x dv on v, within one rounding; the two
    logged parts carry no gradient"""
    from owl_wms.trainers import causvid as CV
    x = inputs("B2N4F2048", dt, vdt)
    losses, dv = run_gen(x, 1.5, 0.5)
    d = {k: t.to(DEV) for k, t in x.items()}
    v = d["v"].clone().requires_grad_()
    gen, dmd, reg = CV._GenLossFn.apply(v, d["out"], d["orig"], d["noisy2"], d["v_cond"], d["v_uncond"], d["v_critic"],
                                        d["ts2"], d["ts_full"], d["mask"], 1.5, 0.5)
    assert torch.equal(dmd, losses[0]) and torch.equal(reg, losses[1]) and torch.equal(gen, losses[0] + 0.5 * losses[1])
    assert gen.requires_grad and not dmd.requires_grad and not reg.requires_grad
    (gen * 0.25).backward()
    assert v.grad.dtype == vdt
    want = 0.25 * dv.double()
    ulp = 2.0 ** -8 if vdt == BF16 else 2.0 ** -24
    worst = ((v.grad.double() - want).abs() / want.abs().clamp_min(1e-300)).max().item()
    print(f"backward scaling {vdt}: worst relative error {worst:.3e} (one rounding: {ulp:.3e})")
    assert bool(((v.grad.double() - want).abs() <= ulp * want.abs()).all())
    assert bool((v.grad.cpu()[~x["mask"]] == 0).all())


def test_binding_refusals():
    from owl_wms import kernels as K
    t = lambda *s, dt=BF16: torch.zeros(*s, dtype=dt, device=DEV)  # noqa: E731
    m, ts = torch.ones(1, 1, dtype=torch.bool, device=DEV), t(1, 1, dt=F32)
    with pytest.raises(RuntimeError, match="causvid_mix: F=12 elements per frame must be a multiple of 8"):
        K.causvid_mix(t(1, 1, 12), t(1, 1, 12), ts, m, 0.2)
    with pytest.raises(RuntimeError, match="causvid_mix: z has shape"):
        K.causvid_mix(t(1, 1, 16), t(1, 2, 16), ts, m, 0.2)
    with pytest.raises(RuntimeError, match="causvid_x0: ts_full has shape"):
        K.causvid_x0(t(1, 1, 16), t(1, 1, 16), t(1, 1, 16), t(1, 2, dt=F32), m)
    with pytest.raises(RuntimeError, match="causvid_x0: clean must be torch.bfloat16"):
        K.causvid_x0(t(1, 1, 16), t(1, 1, 16, dt=F32), t(1, 1, 16), ts, m)
    g = lambda **kw: K.causvid_gen_loss(*[kw.get(k, t(1, 1, 16)) for k in ("out", "orig", "noisy2", "v_cond")], None,  # noqa: E731
                                        kw.get("v_critic", t(1, 1, 16)), ts, ts, kw.get("mask", m), 1.0, 0.0)
    with pytest.raises(RuntimeError, match="causvid_gen_loss: v_critic has shape"):
        g(v_critic=t(1, 1, 8))
    with pytest.raises(RuntimeError, match="causvid_gen_loss: v_critic must be torch.bfloat16"):
        g(v_critic=t(1, 1, 16, dt=F32))
    with pytest.raises(RuntimeError, match="causvid_gen_loss: mask has shape"):
        g(mask=m.expand(1, 2))


# ------------------------------------------------------------------------------------ the loss functions
class _Lin(nn.Module):
    """velocity = a x + b ts + c sum(mouse) + 0.1 sum(btn) (fp32 out)"""

    def __init__(self, a, b, c):
        super().__init__()
        self.a, self.b, self.c = nn.Parameter(torch.tensor(a)), b, c

    def forward(self, x, ts, mouse, btn):
        return self.a * x + _e(self.b * ts + self.c * mouse.sum(-1) + 0.1 * btn.sum(-1), x)


class _LinAV(nn.Module):
    """the same per modality; has_controls False drops the control term"""

    def __init__(self, a, b, c):
        super().__init__()
        self.a, self.a2, self.b, self.c = nn.Parameter(torch.tensor(a)), nn.Parameter(torch.tensor(0.5 * a)), b, c

    def forward(self, x, audio, ts, mouse, btn, has_controls=None):
        ctrl = self.c * mouse.sum(-1) + 0.1 * btn.sum(-1)
        if has_controls is not None:
            ctrl = ctrl * has_controls.to(ctrl.dtype)[:, None]
        return self.a * x + _e(self.b * ts + ctrl, x), self.a2 * audio + _e(self.b * ts + 0.5 * ctrl, audio)


def _stub_run(av, which, cfg, fused):
    from owl_wms.trainers import causvid as CV
    from owl_wms.trainers.self_forcing import InjectedRolloutNoise
    g = torch.Generator().manual_seed(9)
    B, N = 2, 4
    r = lambda *s: torch.randn(*s, generator=g).to(DEV)  # noqa: E731
    video, audio = r(B, N, 32, 8, 8), r(B, N, 16) if av else None
    mouse, btn = r(B, N, 2), torch.rand(B, N, 5, generator=g).round().to(DEV)
    shapes = [video.shape] + ([audio.shape] if av else [])
    draws = [torch.tensor(M1).logical_not().float() * 0.9, torch.randint(0, 2, (B, N), generator=g)] \
        + [r(*s) for s in shapes] + [r(B, N)] + [r(*s) for s in shapes]  # rand < 0.5 exactly on M1's frames
    rollouts = CV.CausVidRollouts(None, noise_prev=NOISE_PREV, gen_mask_p=0.5, noise_source=InjectedRolloutNoise(draws))
    cls = _LinAV if av else _Lin
    student, critic, teacher = (cls(*p).to(DEV) for p in ((1.1, 0.1, -0.3), (0.7, 0.3, 0.2), (0.9, -0.2, 0.4)))
    if which == "gen":
        loss, parts = CV.get_gen_loss(student, critic, teacher, video, mouse, btn, rollouts, cfg_scale=cfg,
                                      regression_weight=0.5, audio=audio, fused=fused)
        learner, others = student, (critic, teacher)
    else:
        loss, parts = CV.get_critic_loss(student, critic, video, mouse, btn, rollouts, audio=audio, fused=fused)
        learner, others = critic, (student,)
    loss.backward()
    assert all(p.grad is None for m in others for p in m.parameters())  # only the learner gets a gradient
    res = {"loss": loss.item()}
    res.update({k: v.item() for k, v in parts.items()})
    res.update({f"d/d {n}": p.grad.item() for n, p in learner.named_parameters()})
    return res


def _agree(tag, fused, torch_):
    assert fused.keys() == torch_.keys()
    for k in fused:
        a, b = fused[k], torch_[k]
        e = abs(a - b) / abs(b)
        print(f"{tag}: {k}: fused {a:.8e} torch {b:.8e} rel {e:.2e}")
        assert e <= 1e-4


@pytest.mark.parametrize("cfg", [1.5, 1.0])
@pytest.mark.parametrize("av", [False, True], ids=["game_rft", "game_rft_audio"])
def test_get_gen_loss_fused_matches_torch_tail(av, cfg):
    res = {fused: _stub_run(av, "gen", cfg, fused) for fused in (None, False)}
    assert res[None]["gen_frames"] == 5 and ("dmd_loss_audio" in res[None]) == av
    _agree(f"get_gen_loss av={av} cfg={cfg}", res[None], res[False])


@pytest.mark.parametrize("av", [False, True], ids=["game_rft", "game_rft_audio"])
def test_get_critic_loss_fused_matches_torch_tail(av):
    res = {fused: _stub_run(av, "critic", 1.5, fused) for fused in (None, False)}
    assert ("critic_loss_audio" in res[None]) == av
    _agree(f"get_critic_loss av={av}", res[None], res[False])
