"""Kernel-level tests of the MMDiT joint-frame ring entries (include/owlk.h: owlk_mm_qk_rope_fwd_kv_ring,
owlk_attn_decode_joint_ring_fwd) against their linear siblings on unrolled (torch.roll-ed) copies of the
buffers.

Tolerance: torch.equal throughout -- the ring forms run the linear kernels' arithmetic in the same order,
only the destination rows (rope) and each LDS-DMA row's source address (attention) wrap.

Shapes: B 2, H 2, D 64, a (64, 1) joint frame on a 455-row ring (7 frames), and one sweep of a (16, 1)
frame on a 119-row ring: 17 rows leave three of the five 16-query tiles empty and every key tile ragged."""
import pytest
import torch

from oracle import ref_ops as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
B, H, D = 2, 2, 64


def K():
    from owl_wms import kernels
    return kernels


def rnd(*shape, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g).to(torch.bfloat16).to(DEV)


def unit(t):
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


# (n0, n1) -> (cap, [(name, start, cached)]); "full ring" is re-based on the call's L (cached = cap - L)
SHAPES = {
    (64, 1): (455, [("no wrap", 0, 130),
                    ("wrap inside a key tile and a 16-row DMA group (logical row 40)", 415, 130),
                    ("wrap on a tile boundary (logical row 64)", 391, 130),
                    ("the new rows straddle the end", 195, 240),
                    ("full ring", 100, 390),
                    ("empty cache: Lkv 65, two waves idle, and it wraps", 415, 0)]),
    (16, 1): (119, [("no wrap", 0, 34),
                    ("wrap inside a tile", 109, 34),
                    ("the new rows straddle the end", 51, 60),
                    ("full ring", 20, 102),
                    ("empty cache, wraps", 110, 0)]),
}
_IN = {}


def _attn_inputs(n0, n1):
    """unit-RMS q and ring buffers for a shape, made once and read-only"""
    if (n0, n1) not in _IN:
        cap = SHAPES[(n0, n1)][0]
        _IN[(n0, n1)] = (unit(rnd(B, n0 + n1, H * D, seed=1)), unit(rnd(B, cap, H * D, seed=2)),
                         rnd(B, cap, H * D, seed=3))
    return _IN[(n0, n1)]


@pytest.mark.parametrize("n0,n1", [(64, 1), (16, 1)])
def test_ring_joint_attention_equals_linear_on_unrolled_buffers(n0, n1):
    """owlk_attn_decode_joint_ring_fwd on ring buffers == owlk_attn_decode_joint_fwd on rows [first, total)
    of torch.roll(-start) copies: o0, o1 and lse bit for bit and finite, for every state, unwindowed and
    with a two-frame window (with (415, 130) and window 130 the window's first key lies past the wrap)."""
    k = K()
    L = n0 + n1
    cap, states = SHAPES[(n0, n1)]
    q, kb, vb = _attn_inputs(n0, n1)
    bound = k.qk_norm_bound(D)
    for name, start, cached in states:
        total = cached + L
        assert 0 <= start < cap and total <= cap, name
        kl, vl = torch.roll(kb, -start, 1), torch.roll(vb, -start, 1)
        for window in (0, 2 * L):
            first = total - window if window > 0 and total > window else 0
            if (n0, start, cached, window) == (64, 415, 130, 130):
                assert start + first > cap  # the first visible key lies past the wrap
            o0, o1, lse = k.attn_decode_joint_ring_fwd(q, kb, vb, H, D, n0, n1, dev_state(start, cached), window,
                                                       score_bound=bound, want_lse=True)
            r0, r1, rl = k.attn_decode_joint_fwd(q, kl[:, first:total], vl[:, first:total], H, D, n0, n1,
                                                 score_bound=bound, want_lse=True)
            for t in (r0, r1, rl):
                assert torch.isfinite(t.float()).all(), (name, window)
            assert torch.equal(o0, r0) and torch.equal(o1, r1) and torch.equal(lse, rl), (name, window)


def test_ring_joint_attention_window_hides_the_keys_before_it():
    """(415, 130), window 130: overwriting the 65 hidden keys (and every dead row of the ring) changes
    nothing."""
    k = K()
    n0, n1, cap = 64, 1, 455
    q, kb, vb = _attn_inputs(n0, n1)
    start, cached, window = 415, 130, 130
    st, bound = dev_state(start, cached), k.qk_norm_bound(D)
    o0, o1, lse = k.attn_decode_joint_ring_fwd(q, kb, vb, H, D, n0, n1, st, window, score_bound=bound, want_lse=True)
    first, total = cached + 65 - window, cached + 65
    visible = torch.zeros(cap, dtype=torch.bool, device=DEV)
    visible[(torch.arange(first, total, device=DEV) + start) % cap] = True
    kb2, vb2 = kb.clone(), vb.clone()
    n_hid = int((~visible).sum())
    kb2[:, ~visible] = unit(rnd(B, n_hid, H * D, seed=4))
    vb2[:, ~visible] = rnd(B, n_hid, H * D, seed=5)
    p0, p1, lse2 = k.attn_decode_joint_ring_fwd(q, kb2, vb2, H, D, n0, n1, st, window, score_bound=bound,
                                                want_lse=True)
    assert torch.equal(o0, p0) and torch.equal(o1, p1) and torch.equal(lse, lse2)


@pytest.mark.parametrize("n0,n1,nf", [(64, 1, 1), (64, 1, 2), (16, 1, 1)])
def test_ring_mm_rope_write_equals_linear(n0, n1, nf):
    """owlk_mm_qk_rope_fwd_kv_ring (MotionRoPE angles with the audio slot, rope offset 3 frames): q and the
    rolled K / V buffers equal owlk_mm_qk_rope_fwd_kv writing slots [cached, cached + L) at tab_off = off
    bit for bit; every other row keeps its sentinel; the V rows are the sources' V columns."""
    k = K()
    tpf, d = n0 + n1, H * D
    L = nf * tpf
    cap, states = SHAPES[(n0, n1)]
    ang = R.motion_rope_angles(8, int(n0 ** 0.5), D, has_audio=True)
    assert ang.shape[0] == 8 * tpf
    cos, sin = ang.cos().to(DEV), ang.sin().to(DEV)
    qkv0, qkv1 = rnd(B * nf * n0, 3 * d, seed=10), rnd(B * nf * n1, 3 * d, seed=11)
    off = 3 * tpf
    v_src = k.frame_interleave(qkv0, qkv1, n0, n1)[:, 2 * d:]  # the joint rows' V columns [B L, d]
    for name, start, cached in states:
        if name == "full ring":
            cached = cap - L
        assert 0 <= start < cap and cached + L <= cap and off + L <= ang.shape[0], name
        if "straddle" in name:
            assert start + cached < cap < start + cached + L
        kb = torch.full((B, cap, d), 7.0, device=DEV, dtype=torch.bfloat16)
        vb = torch.full((B, cap, d), -7.0, device=DEV, dtype=torch.bfloat16)
        kl, vl = kb.clone(), vb.clone()
        q = torch.zeros(B, L, d, device=DEV, dtype=torch.bfloat16)
        ql = torch.zeros_like(q)
        k.mm_qk_rope_fwd_kv_ring(qkv0, qkv1, B, nf, n0, n1, H, D, cos, sin, dev_state(start, cached, off), q, kb, vb)
        k.mm_qk_rope_fwd_kv(qkv0, qkv1, B, nf, n0, n1, H, D, cos, sin, off, ql, kl[:, cached:cached + L],
                            vl[:, cached:cached + L])
        assert torch.equal(q, ql), name
        assert torch.equal(torch.roll(kb, -start, 1), kl) and torch.equal(torch.roll(vb, -start, 1), vl), name
        rows = (torch.arange(cached, cached + L, device=DEV) + start) % cap  # token t's row
        written = torch.zeros(cap, dtype=torch.bool, device=DEV)
        written[rows] = True
        assert (kb[:, ~written] == 7.0).all() and (vb[:, ~written] == -7.0).all(), name
        assert not (kb[:, rows] == 7.0).all(-1).any(), name
        assert torch.equal(vb[:, rows].reshape(B * L, d), v_src), name


def test_ring_states_outside_the_contract_are_not_followed():
    """cached + L > cap, start >= cap, start < 0, cached < 0, table rows outside n_tab (the guard
    qk_rope_kv_k / attn_fwd16_split_k have): NaN q / o0 / o1 / lse, the buffers untouched.  The last
    state inside the contract, (cap - 1, cap - 65), gives finite output."""
    k = K()
    n0, n1, cap = 64, 1, 455
    L, d = 65, H * D
    ang = R.motion_rope_angles(3, 8, D, has_audio=True)
    n_tab = ang.shape[0]
    cos, sin = ang.cos().to(DEV), ang.sin().to(DEV)
    qkv0, qkv1 = rnd(B * n0, 3 * d, seed=20), rnd(B * n1, 3 * d, seed=21)
    qn, kb0, vb0 = _attn_inputs(n0, n1)
    kb, vb = kb0.clone(), vb0.clone()
    bound = k.qk_norm_bound(D)
    for st in ([0, cap - L + 1, 0], [cap - 8, cap - L + 1, 0], [cap, 0, 0], [-65, 0, 0], [0, -1, 0]):
        q = torch.zeros(B, L, d, device=DEV, dtype=torch.bfloat16)
        k.mm_qk_rope_fwd_kv_ring(qkv0, qkv1, B, 1, n0, n1, H, D, cos, sin, dev_state(*st), q, kb, vb)
        o0, o1, lse = k.attn_decode_joint_ring_fwd(qn, kb, vb, H, D, n0, n1, dev_state(*st), 0, score_bound=bound,
                                                   want_lse=True)
        torch.cuda.synchronize()
        assert torch.equal(kb, kb0) and torch.equal(vb, vb0), st
        assert torch.isnan(q.float()).all(), st
        assert torch.isnan(o0.float()).all() and torch.isnan(o1.float()).all() and torch.isnan(lse).all(), st
    for st in ([0, 0, n_tab - L + 1], [0, 0, -1]):  # table rows outside n_tab
        q = torch.zeros(B, L, d, device=DEV, dtype=torch.bfloat16)
        k.mm_qk_rope_fwd_kv_ring(qkv0, qkv1, B, 1, n0, n1, H, D, cos, sin, dev_state(*st), q, kb, vb)
        torch.cuda.synchronize()
        assert torch.equal(kb, kb0) and torch.equal(vb, vb0) and torch.isnan(q.float()).all(), st
    st = dev_state(cap - 1, cap - L, n_tab - L)  # a full ring starting at its last row, the table's last rows
    o0, o1, lse = k.attn_decode_joint_ring_fwd(qn, kb, vb, H, D, n0, n1, st, 0, score_bound=bound, want_lse=True)
    assert torch.isfinite(o0.float()).all() and torch.isfinite(o1.float()).all() and torch.isfinite(lse).all()
    q = torch.zeros(B, L, d, device=DEV, dtype=torch.bfloat16)
    k.mm_qk_rope_fwd_kv_ring(qkv0, qkv1, B, 1, n0, n1, H, D, cos, sin, st, q, kb, vb)
    assert torch.isfinite(q.float()).all() and not torch.equal(kb, kb0)
