"""Kernel-level tests of the endless-streaming entries (include/owlk.h): the ring forms of the
device-state decode kernels (owlk_qk_rope_fwd_kv_ring, owlk_attn_decode_ring_fwd) against the linear
forms on unrolled (torch.roll-ed) copies of the buffers, bit for bit, and owlk_rope_rebase against an
fp64 rotation of the same bf16 input.

Tolerances.  Ring against linear: torch.equal (same arithmetic in the same order, only the DMA rows'
source addresses differ).  Rebase: fp32 math with one final bf16 rounding, so each element lies within
one bf16 rounding of the fp64 result, the project's idiom |a - b| <= 2^-8 |b| + 1e-5 max|b|.
Attention under a rebase: rel-L2 <= 1e-2, the project's decode-attention parity bound."""
from types import SimpleNamespace

import pytest
import torch

from oracle import ref_ops as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
CAP = 384
B, H = 2, 2


def K():
    from owl_wms import kernels
    return kernels


def rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


def rnd(*shape, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g).to(torch.bfloat16).to(DEV)


def unit(t, D):
    """rows RMS-normalised per head (what the rope kernels hand the attention: |q.k| <= D)"""
    f = t.float().view(*t.shape[:-1], -1, D)
    return (f * torch.rsqrt(f.pow(2).mean(-1, keepdim=True))).bfloat16().view(t.shape)


def dev_state(*v):
    return torch.tensor(list(v) + [0] * (4 - len(v)), dtype=torch.int64, device=DEV)


@pytest.fixture(scope="module", autouse=True)
def _needs_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from owl_wms._lib import lib
    lib()


def ring_states(L):
    """(name, start, cached) for Lnew = L new rows on a CAP-row ring"""
    return [("no wrap", 0, 128),
            ("wrap inside a key tile and a 16-row DMA group", CAP - 40, 128),
            ("wrap on a tile boundary", CAP - 64, 128),
            ("the new rows wrap", 200, CAP - 200 - 10),
            ("full ring", 100, CAP - L)]


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("L", [64, 24])
def test_ring_attention_equals_linear_on_unrolled_buffers(D, L):
    """owlk_attn_decode_ring_fwd on ring buffers == owlk_attn_decode_fwd on torch.roll-ed copies with
    start 0: o and lse bit for bit, for every wrap position and with / without a key window (with
    start = CAP - 40, cached 128, L 64 and a 128-key window the window's first key lies past the wrap)."""
    k = K()
    q = unit(rnd(B, L, H * D, seed=1), D)
    kb = unit(rnd(B, CAP, H * D, seed=2), D)
    vb = rnd(B, CAP, H * D, seed=3)
    bound = k.qk_norm_bound(D)
    for name, start, cached in ring_states(L):
        assert 0 <= start < CAP and cached + L <= CAP
        if name == "the new rows wrap":
            assert start + cached < CAP < start + cached + L
        kl, vl = torch.roll(kb, -start, 1).contiguous(), torch.roll(vb, -start, 1).contiguous()
        for window in (0, 128):
            o, lse = k.attn_decode_ring_fwd(q, kb, vb, H, D, dev_state(start, cached), L, window, score_bound=bound)
            o0, lse0 = k.attn_decode_fwd(q, kl, vl, H, D, dev_state(0, cached), L, window, score_bound=bound)
            assert torch.isfinite(o0.float()).all() and torch.isfinite(lse0).all(), (name, window)
            assert torch.equal(o, o0) and torch.equal(lse, lse0), (name, window)
    # the window really hides the keys before it: changing them changes nothing
    start, cached = CAP - 40, 128
    o, lse = k.attn_decode_ring_fwd(q, kb, vb, H, D, dev_state(start, cached), L, 128, score_bound=bound)
    kb2, vb2 = kb.clone(), vb.clone()
    hidden = (torch.arange(0, cached + L - 128, device=DEV) + start) % CAP
    kb2[:, hidden] = unit(rnd(B, hidden.numel(), H * D, seed=4), D)
    vb2[:, hidden] = rnd(B, hidden.numel(), H * D, seed=5)
    o2, lse2 = k.attn_decode_ring_fwd(q, kb2, vb2, H, D, dev_state(start, cached), L, 128, score_bound=bound)
    assert torch.equal(o, o2) and torch.equal(lse, lse2)


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("L", [64, 24])
def test_ring_rope_write_equals_linear(D, L):
    """owlk_qk_rope_fwd_kv_ring: q and the K/V rows it writes equal owlk_qk_rope_fwd_kv_dev's on the
    unrolled buffer bit for bit; every other row keeps its sentinel."""
    k = K()
    ang = R.motion_rope_angles(6, 8, D)
    cos, sin = ang.cos().to(DEV), ang.sin().to(DEV)
    qkv = rnd(B * L, 3 * H * D, seed=10)
    off = 3 * 64
    for name, start, cached in ring_states(L):
        kb = torch.full((B, CAP, H * D), 7.0, device=DEV, dtype=torch.bfloat16)
        vb = torch.full((B, CAP, H * D), -7.0, device=DEV, dtype=torch.bfloat16)
        kl, vl = kb.clone(), vb.clone()
        q = torch.zeros(B, L, H * D, device=DEV, dtype=torch.bfloat16)
        ql = torch.zeros_like(q)
        k.qk_rope_fwd_kv_ring(qkv, B, L, H, D, cos, sin, dev_state(start, cached, off), q, kb, vb)
        k.qk_rope_fwd_kv_dev(qkv, B, L, H, D, cos, sin, dev_state(0, cached, off), ql, kl, vl)
        assert torch.equal(q, ql), name
        assert torch.equal(torch.roll(kb, -start, 1), kl) and torch.equal(torch.roll(vb, -start, 1), vl), name
        rows = (torch.arange(cached, cached + L, device=DEV) + start) % CAP  # token t's row
        written = torch.zeros(CAP, dtype=torch.bool, device=DEV)
        written[rows] = True
        assert (kb[:, ~written] == 7.0).all() and (vb[:, ~written] == -7.0).all(), name
        assert not (kb[:, rows] == 7.0).all(-1).any(), name
        assert torch.equal(vb[:, rows].reshape(B * L, H * D), qkv[:, 2 * H * D:]), name


@pytest.mark.parametrize("D", [64, 128])
def test_ring_states_outside_the_contract_are_not_followed(D):
    """cached + Lnew > cap, start >= cap or start < 0 (the guard the linear entries have,
    test_decode_positions_are_bounded): NaN q / o / lse, the cache untouched, nothing read."""
    k = K()
    L = 64
    ang = R.motion_rope_angles(3, 8, D)
    rows = ang.shape[0]
    cos, sin = ang.cos().to(DEV), ang.sin().to(DEV)
    qkv = rnd(B * L, 3 * H * D, seed=20)
    kb, vb = unit(rnd(B, CAP, H * D, seed=21), D), rnd(B, CAP, H * D, seed=22)
    k0, v0 = kb.clone(), vb.clone()
    qn = unit(rnd(B, L, H * D, seed=23), D)
    for st in ([0, CAP - L + 1, 0], [CAP - 8, CAP - L + 1, 0], [CAP, 0, 0], [-64, 0, 0], [0, -1, 0]):
        q = torch.zeros(B, L, H * D, device=DEV, dtype=torch.bfloat16)
        k.qk_rope_fwd_kv_ring(qkv, B, L, H, D, cos, sin, dev_state(*st), q, kb, vb)
        o, lse = k.attn_decode_ring_fwd(qn, kb, vb, H, D, dev_state(*st), L, 0, score_bound=k.qk_norm_bound(D))
        torch.cuda.synchronize()
        assert torch.equal(kb, k0) and torch.equal(vb, v0), st
        assert torch.isnan(q.float()).all(), st
        assert torch.isnan(o.float()).all() and torch.isnan(lse).all(), st
    for st in ([0, 0, rows - L + 1], [0, 0, -1]):  # table rows outside n_tab
        q = torch.zeros(B, L, H * D, device=DEV, dtype=torch.bfloat16)
        k.qk_rope_fwd_kv_ring(qkv, B, L, H, D, cos, sin, dev_state(*st), q, kb, vb)
        torch.cuda.synchronize()
        assert torch.equal(kb, k0) and torch.equal(vb, v0) and torch.isnan(q.float()).all(), st
    # the last state inside the contract is followed: a full ring starting at its last row
    o, lse = k.attn_decode_ring_fwd(qn, kb, vb, H, D, dev_state(CAP - 1, CAP - L), L, 0,
                                    score_bound=k.qk_norm_bound(D))
    assert torch.isfinite(o.float()).all() and torch.isfinite(lse).all()


def _ring_cache(D, kb, vb, start, rows, offset, cos, sin):
    from owl_wms.nn.kv_cache import RingKVCache
    cfg = SimpleNamespace(n_layers=1, tokens_per_frame=64, n_heads=H, d_model=H * D)
    c = RingKVCache(cfg, kb.shape[1], rope=SimpleNamespace(cos=cos, sin=sin))
    c.reset(kb.shape[0])
    c.bufs[0], c.start[0], c.len[0], c.offsets[0] = (kb, vb), start, rows, offset
    return c


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("shift", [1, 5])
@pytest.mark.parametrize("start", [32, CAP - 100])
def test_rope_rebase_against_fp64(D, shift, start):
    """RingKVCache.rebase -> owlk_rope_rebase on 192 live rows (wrapping for start = CAP - 100) rotated
    at frames 6..8 of a 12-frame motion table, moved down by `shift` frames: each element within one
    bf16 rounding of the fp64 rotation by the angle difference; rows off the window and V unchanged
    bit for bit; the same call on the same input gives the same bits."""
    rows, old = 192, 6 * 64
    new = old - shift * 64
    ang = R.motion_rope_angles(12, 8, D)
    cos, sin = ang.cos().to(DEV), ang.sin().to(DEV)
    kin, vin = rnd(B, CAP, H * D, seed=30), rnd(B, CAP, H * D, seed=31)
    outs = []
    for _ in range(2):
        kb, vb = kin.clone(), vin.clone()
        c = _ring_cache(D, kb, vb, start, rows, old + rows, cos, sin)
        c.rebase(shift * 64)
        assert c.offsets[0] == new + rows and c.start[0] == start and c.len[0] == rows
        assert torch.equal(vb, vin)
        outs.append(kb)
    assert torch.equal(outs[0], outs[1])
    live = (torch.arange(rows, device=DEV) + start) % CAP
    dead = torch.ones(CAP, dtype=torch.bool, device=DEV)
    dead[live] = False
    assert torch.equal(outs[0][:, dead], kin[:, dead])
    delta = (ang[new:new + rows].double() - ang[old:old + rows].double()).to(DEV)  # [rows, D/2]
    x = kin[:, live].double().view(B, rows, H, 2, D // 2)
    cd, sd = delta.cos()[None, :, None], delta.sin()[None, :, None]
    ref = torch.stack([x[..., 0, :] * cd - x[..., 1, :] * sd, x[..., 1, :] * cd + x[..., 0, :] * sd], -2)
    got = outs[0][:, live].double().view(B, rows, H, 2, D // 2)
    err = (got - ref).abs()
    bound = 2.0 ** -8 * ref.abs() + 1e-5 * ref.abs().max()
    print(f"rope_rebase D={D} shift={shift} start={start}: max |err| {err.max().item():.3e}, "
          f"max err/bound {(err / bound).max().item():.3f}")
    assert (err <= bound).all()
    assert not torch.equal(outs[0][:, live], kin[:, live])


def test_rope_rebase_refuses_rows_outside_the_table():
    k = K()
    D = 64
    ang = R.motion_rope_angles(4, 8, D)
    cos, sin = ang.cos().to(DEV), ang.sin().to(DEV)
    kb = rnd(B, CAP, H * D, seed=40)
    k0 = kb.clone()
    with pytest.raises(RuntimeError, match="rope table"):
        k.rope_rebase(kb, H, D, 0, 128, cos, sin, 3 * 64, 0)  # old rows 192..319 of 256
    with pytest.raises(RuntimeError, match="rope table"):
        k.rope_rebase(kb, H, D, 0, 128, cos, sin, 64, -64)
    with pytest.raises(RuntimeError, match="ring window"):
        k.rope_rebase(kb, H, D, CAP, 128, cos, sin, 64, 0)
    torch.cuda.synchronize()
    assert torch.equal(kb, k0)


@pytest.mark.parametrize("D", [64, 128])
def test_attention_is_invariant_under_a_rebase(D):
    """K of 3 frames roped at frames 6..8 with q at frame 9, against the same K rebased down by 5 frames
    with q roped at frame 4: the decode attention outputs agree within the decode-attention parity
    bound (the angles are linear in the frame index, so q.k depends only on frame differences)."""
    k = K()
    p, n, s, L, start = 6, 3, 5, 64, CAP - 100
    ang = R.motion_rope_angles(12, 8, D)
    cos, sin = ang.cos().to(DEV), ang.sin().to(DEV)
    ctx = rnd(B * n * L, 3 * H * D, seed=50)
    new = rnd(B * L, 3 * H * D, seed=51)
    kl = torch.zeros(B, CAP, H * D, device=DEV, dtype=torch.bfloat16)
    vl = torch.zeros_like(kl)
    qd = torch.empty(B, n * L, H * D, device=DEV, dtype=torch.bfloat16)
    k.qk_rope_fwd_kv(ctx, B, n * L, H, D, cos, sin, p * L, qd, kl[:, :n * L], vl[:, :n * L])
    outs = []
    for shift in (0, s):
        kb, vb = torch.roll(kl, start, 1).contiguous(), torch.roll(vl, start, 1).contiguous()
        if shift:
            k.rope_rebase(kb, H, D, start, n * L, cos, sin, p * L, (p - shift) * L)
        st = dev_state(start, n * L, (p + n - shift) * L)
        q = torch.empty(B, L, H * D, device=DEV, dtype=torch.bfloat16)
        k.qk_rope_fwd_kv_ring(new, B, L, H, D, cos, sin, st, q, kb, vb)
        o, _ = k.attn_decode_ring_fwd(q, kb, vb, H, D, st, L, 0, score_bound=k.qk_norm_bound(D))
        outs.append(o)
    r = rel(outs[1], outs[0])
    print(f"attention under a {s}-frame rebase, D={D}: rel-L2 {r:.3e}")
    assert torch.isfinite(outs[0].float()).all() and r <= 1e-2
