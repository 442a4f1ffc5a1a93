"""Kernel-level tests of the slot forms of the ring entries (include/owlk.h: owlk_qk_rope_fwd_kv_ring_slots,
owlk_attn_decode_ring_slots_fwd, owlk_ring_advance_slots): one state row {start, cached, offset, live} per
slot, batch row b on row b mod n_slots.

Tolerances: none.  A live slot runs the single-state ring kernels' statements on its own rows and state row,
so its q rows, ring rows, o and lse are torch.equal to owlk_qk_rope_fwd_kv_ring / owlk_attn_decode_ring_fwd on
the [slot::n_slots] views with that state.  An idle slot's ring rows keep every bit, its q and o are zero, its
lse -inf.  A live slot outside the contract gets NaN q / o rows, its ring rows keep every bit, and the other
slots stay bit-equal to the reference.  owlk_ring_advance_slots equals the host rule row by row."""
import pytest
import torch

from oracle import ref_ops as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
NS, H, TPF = 3, 2, 64
B = 2 * NS  # the CFG batch [cond | uncond]
CAP = 5 * TPF
# slot 0 plain; slot 1's window wraps (256 + 192 > 320) and its new rows land behind it at 128..; slot 2 idle
STATES = [(0, 128, 128, 1), (256, 192, 1000, 1), (0, 0, 0, 0)]


def K():
    from owl_wms import kernels
    return kernels


def rnd(*shape, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g).to(torch.bfloat16).to(DEV)


def unit(t, D):
    """rows RMS-normalised per head (what the rope kernel hands the attention: |q.k| <= D)"""
    f = t.float().view(*t.shape[:-1], -1, D)
    return (f * torch.rsqrt(f.pow(2).mean(-1, keepdim=True))).bfloat16().view(t.shape)


def slot_state(rows):
    return torch.tensor(rows, dtype=torch.int64, device=DEV)


def one_state(row):
    return torch.tensor(list(row[:3]) + [0], dtype=torch.int64, device=DEV)


@pytest.fixture(scope="module", autouse=True)
def _needs_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from owl_wms._lib import lib
    lib()


@pytest.fixture(scope="module")
def tables():
    """MotionRoPE tables of 17 frames (1088 rows: slot 1 ropes at 1000..1063) per head_dim"""
    out = {}
    for D in (64, 128):
        ang = R.motion_rope_angles(17, 8, D)
        out[D] = (ang.cos().to(DEV), ang.sin().to(DEV))
    return out


def pattern(D, seed):
    """ring buffers pre-filled with a fixed pattern: K rows normalised like roped keys, V random"""
    return unit(rnd(B, CAP, H * D, seed=seed), D), rnd(B, CAP, H * D, seed=seed + 1)


def run_rope(k, qkv, L, D, cos, sin, state, kb, vb):
    q = torch.full((kb.shape[0], L, H * D), 3.0, device=DEV, dtype=torch.bfloat16)
    fn = k.qk_rope_fwd_kv_ring_slots if state.dim() == 2 else k.qk_rope_fwd_kv_ring
    fn(qkv, kb.shape[0], L, H, D, cos, sin, state, q, kb, vb)
    return q


def slot_rows(t, s):
    """the batch rows of slot s: [cond, uncond]"""
    return t[s::NS]


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("L", [64, 16])
def test_slot_rope_equals_single_state_per_slot(D, L, tables):
    k = K()
    cos, sin = tables[D]
    qkv = rnd(B * L, 3 * H * D, seed=10)
    kb0, vb0 = pattern(D, 20)
    kb, vb = kb0.clone(), vb0.clone()
    q = run_rope(k, qkv, L, D, cos, sin, slot_state(STATES), kb, vb)
    for s in (0, 1):
        # the single-state ring entry on the slot's views: its batch rows' qkv, its own state
        kr, vr = kb0.clone(), vb0.clone()
        qkv_s = qkv.view(B, L, -1)[s::NS].reshape(2 * L, -1).contiguous()
        qr = run_rope(k, qkv_s, L, D, cos, sin, one_state(STATES[s]), slot_rows(kr, s), slot_rows(vr, s))
        assert torch.isfinite(qr.float()).all()
        assert torch.equal(slot_rows(q, s), qr), s
        assert torch.equal(slot_rows(kb, s), slot_rows(kr, s)) and torch.equal(slot_rows(vb, s), slot_rows(vr, s)), s
        assert not torch.equal(slot_rows(kb, s), slot_rows(kb0, s))  # the new rows were written
    # the idle slot: ring rows bit for bit as they were, q zero
    assert torch.equal(slot_rows(kb, 2), slot_rows(kb0, 2)) and torch.equal(slot_rows(vb, 2), slot_rows(vb0, 2))
    assert (slot_rows(q, 2) == 0).all()


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("L", [64, 16])
def test_slot_attention_equals_single_state_per_slot(D, L):
    k = K()
    q = unit(rnd(B, L, H * D, seed=1), D)
    kb, vb = pattern(D, 30)
    bound = k.qk_norm_bound(D)
    for window in (0, 128):
        kb1, vb1 = kb.clone(), vb.clone()
        o, lse = k.attn_decode_ring_slots_fwd(q, kb1, vb1, H, D, slot_state(STATES), L, window, score_bound=bound)
        assert torch.equal(kb1, kb) and torch.equal(vb1, vb)  # attention writes no ring row
        for s in (0, 1):
            qs = slot_rows(q, s).contiguous()
            o0, lse0 = k.attn_decode_ring_fwd(qs, slot_rows(kb, s), slot_rows(vb, s), H, D, one_state(STATES[s]), L,
                                              window, score_bound=bound)
            assert torch.isfinite(o0.float()).all() and torch.isfinite(lse0).all()
            assert torch.equal(slot_rows(o, s), o0) and torch.equal(slot_rows(lse, s), lse0), (s, window)
        assert (slot_rows(o, 2) == 0).all() and (slot_rows(lse, 2) == float("-inf")).all()
    # the two live slots see different keys: their outputs differ although the queries repeat
    q2 = q.clone()
    q2[1::NS] = q2[0::NS]
    o2, _ = k.attn_decode_ring_slots_fwd(q2, kb, vb, H, D, slot_state(STATES), L, 0, score_bound=bound)
    assert not torch.equal(slot_rows(o2, 0), slot_rows(o2, 1))


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("L", [64, 16])
def test_poisoned_slot_is_alone(D, L, tables):
    """slot 1 with cached + L > cap: its q and o all NaN, its ring rows untouched, slot 0 still bit-equal to
    the single-state entries, the idle slot still zero."""
    k = K()
    cos, sin = tables[D]
    bad = list(STATES)
    bad[1] = (256, CAP - L + 1, 1000, 1)
    assert bad[1][1] + L > CAP
    qkv = rnd(B * L, 3 * H * D, seed=11)
    kb0, vb0 = pattern(D, 40)
    kb, vb = kb0.clone(), vb0.clone()
    q = run_rope(k, qkv, L, D, cos, sin, slot_state(bad), kb, vb)
    assert torch.isnan(slot_rows(q, 1).float()).all()
    assert torch.equal(slot_rows(kb, 1), slot_rows(kb0, 1)) and torch.equal(slot_rows(vb, 1), slot_rows(vb0, 1))
    kr, vr = kb0.clone(), vb0.clone()
    qkv_0 = qkv.view(B, L, -1)[0::NS].reshape(2 * L, -1).contiguous()
    qr = run_rope(k, qkv_0, L, D, cos, sin, one_state(bad[0]), slot_rows(kr, 0), slot_rows(vr, 0))
    assert torch.equal(slot_rows(q, 0), qr) and torch.equal(slot_rows(kb, 0), slot_rows(kr, 0))
    assert torch.equal(slot_rows(vb, 0), slot_rows(vr, 0))
    assert (slot_rows(q, 2) == 0).all() and torch.equal(slot_rows(kb, 2), slot_rows(kb0, 2))
    # attention on the buffers as the rope left them
    qa = unit(rnd(B, L, H * D, seed=2), D)
    bound = k.qk_norm_bound(D)
    o, lse = k.attn_decode_ring_slots_fwd(qa, kb, vb, H, D, slot_state(bad), L, 0, score_bound=bound)
    assert torch.isnan(slot_rows(o, 1).float()).all() and torch.isnan(slot_rows(lse, 1)).all()
    o0, lse0 = k.attn_decode_ring_fwd(slot_rows(qa, 0).contiguous(), slot_rows(kb, 0), slot_rows(vb, 0), H, D,
                                      one_state(bad[0]), L, 0, score_bound=bound)
    assert torch.equal(slot_rows(o, 0), o0) and torch.equal(slot_rows(lse, 0), lse0)
    assert torch.isfinite(o0.float()).all()
    assert (slot_rows(o, 2) == 0).all()
    # a rope offset past the table poisons the q rows of that slot alone as well
    bad[1] = (256, 192, 17 * TPF - L + 1, 1)
    kb, vb = kb0.clone(), vb0.clone()
    q = run_rope(k, qkv, L, D, cos, sin, slot_state(bad), kb, vb)
    assert torch.isnan(slot_rows(q, 1).float()).all() and torch.equal(slot_rows(kb, 1), slot_rows(kb0, 1))
    assert torch.equal(slot_rows(q, 0), qr)


def host_rule(row, L, max_rows, cap):
    start, cached, off, live = row
    if not live:
        return row
    if not (0 <= start < cap and 0 <= cached and cached + L <= cap and 0 <= off):
        return (start, -1, off, live)
    cached, off = cached + L, off + L
    if cached > max_rows:
        start, cached = (start + L) % cap, cached - L
    return (start, cached, off, live)


def test_ring_advance_slots_follows_the_host_rule_per_row():
    k = K()
    L, max_rows, cap = 64, 256, 320
    rows = [(0, 128, 128, 1),        # does not evict
            (256, 256, 4000, 1),     # evicts, start wraps to 0
            (192, 77, 9, 0),         # idle: left alone whatever it holds
            (64, 300, 500, 1)]       # cached + L > cap: out of contract
    st = slot_state(rows)
    want = rows
    for step in range(3):
        k.ring_advance_slots(st, L, max_rows, cap)
        want = [host_rule(r, L, max_rows, cap) for r in want]
        assert [tuple(r) for r in st.tolist()] == want, step
    assert want[0] == (64, 256, 320, 1) and want[1][0] == (256 + 3 * 64) % 320 and want[1][1:] == (256, 4192, 1)
    assert want[2] == rows[2]
    assert want[3] == (64, -1, 500, 1)  # only cached changed, and it stays -1


def test_slot_entries_refuse_on_the_host():
    """every host-checked argument error returns 1 and launches nothing"""
    from owl_wms._lib import lib
    h = lib()
    st = slot_state(STATES)
    p = st.data_ptr()
    for args in ((None, 3, 64, 256, 320), (p, 0, 64, 256, 320), (p, -1, 64, 256, 320), (p, 3, 0, 256, 320),
                 (p, 3, 64, 0, 320), (p, 3, 64, 257, 320), (p, 3, 400, 1, 320), (p, 3, 64, 256, 0)):
        assert h.owlk_ring_advance_slots(*args, None) == 1, args
    k = K()
    D, L = 64, 64
    q = unit(rnd(B, L, H * D, seed=1), D)
    kb, vb = pattern(D, 50)
    bound = k.qk_norm_bound(D)
    with pytest.raises(RuntimeError, match="multiple of n_slots"):  # 6 batch rows on 4 state rows
        k.call("owlk_attn_decode_ring_slots_fwd", k.ptr(q), q.stride(1), q.stride(0), k.ptr(kb), kb.stride(1),
               kb.stride(0), k.ptr(vb), vb.stride(1), vb.stride(0), k.ptr(q), q.stride(1), q.stride(0), k.ptr(q), B, H,
               L, D, D ** -0.5, bound, k.ptr(st), 4, L, 0, CAP, k.stream())
    with pytest.raises(RuntimeError, match="state pointer"):
        k.call("owlk_qk_rope_fwd_kv_ring_slots", k.ptr(q), q.stride(1), B * L, L, H, D, k.ptr(q), k.ptr(q), 32, 1088,
               None, 3, k.ptr(q), q.stride(1), q.stride(0), k.ptr(kb), kb.stride(1), kb.stride(0), k.ptr(vb),
               vb.stride(1), vb.stride(0), CAP, k.stream())
    with pytest.raises(RuntimeError, match="multiple of n_slots"):
        k.call("owlk_qk_rope_fwd_kv_ring_slots", k.ptr(q), q.stride(1), B * L, L, H, D, k.ptr(q), k.ptr(q), 32, 1088,
               k.ptr(st), 4, k.ptr(q), q.stride(1), q.stride(0), k.ptr(kb), kb.stride(1), kb.stride(0), k.ptr(vb),
               vb.stride(1), vb.stride(0), CAP, k.stream())
