"""Kernel-level tests of the slot forms of the audio + video ring entries (include/owlk.h:
owlk_mm_qk_rope_fwd_kv_ring_slots, owlk_attn_decode_joint_ring_slots_fwd, owlk_attn_decode_wide_ring_slots_fwd):
one state row {start, cached, offset, live} per slot, batch row b on row b mod n_slots.

Tolerances: none.  A live slot runs the single-state kernels' statements on its own rows and state row, so its q
rows, ring rows, o0 / o1 / o and lse are torch.equal to owlk_mm_qk_rope_fwd_kv_ring / owlk_attn_decode_joint_ring_fwd
/ owlk_attn_decode_wide_ring_fwd on the [slot::n_slots] views with that state.  An idle slot's ring rows keep every
bit, its q and o rows are zero, its lse -inf.  A live slot outside the contract gets NaN q / o rows and lse, its
ring rows keep every bit, and the other slots stay bit-equal to the clean run.

Shapes: 3 slots, CFG batch 6, H 2, D 64; joint frames of 65 rows (64 + 1) and 80 rows (64 + 16: all five query
tiles full), for the wide entry also 17 query rows; rings of 5 frames.  Slot 0 is plain {0, 2L, 2L, 1}, slot 1
wraps {4L, 3L, off, 1} (its window passes the ring's end and its new rows land at row 2L), slot 2 is idle: the
three slots of one launch have 3L, 4L and no keys (2L each under a two-frame window), so a launch-wide key count
would show in slot 0 or slot 1."""
import pytest
import torch

from oracle import ref_ops as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
NS, H, D = 3, 2, 64
B = 2 * NS  # the CFG batch [cond | uncond]
OFF1 = 1000  # slot 1's rope offset
FRAMES = [(64, 1), (64, 16)]


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


def states(L):
    return [(0, 2 * L, 2 * L, 1), (4 * L, 3 * L, OFF1, 1), (0, 0, 0, 0)]


def slot_state(rows):
    return torch.tensor(rows, dtype=torch.int64, device=DEV)


def one_state(row):
    return torch.tensor(list(row[:3]) + [0], dtype=torch.int64, device=DEV)


def slot_rows(t, s):
    """the batch rows of slot s: [cond, uncond]"""
    return t[s::NS]


@pytest.fixture(scope="module", autouse=True)
def _needs_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from owl_wms._lib import lib
    lib()


@pytest.fixture(scope="module")
def table():
    """MotionRoPE angles with the audio slot, 17 frames (1105 rows: slot 1 ropes at 1000..1079)"""
    ang = R.motion_rope_angles(17, 8, D, has_audio=True)
    assert ang.shape[0] >= OFF1 + 80
    return ang.cos().to(DEV), ang.sin().to(DEV)


_PAT = {}


def pattern(L, seed):
    """ring buffers [B, 5 L, H D] pre-filled with a fixed pattern (K rows normalised like roped keys, V random),
    made once per shape and read-only: callers clone"""
    if (L, seed) not in _PAT:
        _PAT[(L, seed)] = (unit(rnd(B, 5 * L, H * D, seed=seed)), rnd(B, 5 * L, H * D, seed=seed + 1))
    return _PAT[(L, seed)]


def run_mm_rope(k, qkv0, qkv1, n0, n1, cos, sin, state, kb, vb):
    nb = kb.shape[0]
    q = torch.full((nb, n0 + n1, H * D), 3.0, device=DEV, dtype=torch.bfloat16)
    fn = k.mm_qk_rope_fwd_kv_ring_slots if state.dim() == 2 else k.mm_qk_rope_fwd_kv_ring
    fn(qkv0, qkv1, nb, 1, n0, n1, H, D, cos, sin, state, q, kb, vb)
    return q


def slot_qkv(qkv, n, s):
    """the rows of slot s's two batch rows of a modality's qkv GEMM output [B n, 3 H D]"""
    return qkv.view(B, n, -1)[s::NS].reshape(2 * n, -1).contiguous()


def new_rows(st, L):
    """the physical ring rows a frame of L rows is written to under the state row st"""
    start, cached = st[0], st[1]
    return (torch.arange(cached, cached + L, device=DEV) + start) % (5 * L)


@pytest.mark.parametrize("n0,n1", FRAMES)
def test_slot_mm_rope_equals_single_state_per_slot(n0, n1, table):
    k = K()
    cos, sin = table
    L, d = n0 + n1, H * D
    st = states(L)
    assert (st[1][0] + st[1][1]) % (5 * L) == 2 * L and st[1][0] + st[1][1] > 5 * L  # wraps, new rows at 2L
    qkv0, qkv1 = rnd(B * n0, 3 * d, seed=10), rnd(B * n1, 3 * d, seed=11)
    kb0, vb0 = pattern(L, 20)
    kb, vb = kb0.clone(), vb0.clone()
    q = run_mm_rope(k, qkv0, qkv1, n0, n1, cos, sin, slot_state(st), kb, vb)
    for s in (0, 1):
        kr, vr = kb0.clone(), vb0.clone()
        qr = run_mm_rope(k, slot_qkv(qkv0, n0, s), slot_qkv(qkv1, n1, s), n0, n1, cos, sin, one_state(st[s]),
                         slot_rows(kr, s), slot_rows(vr, s))
        assert torch.isfinite(qr.float()).all()
        assert torch.equal(slot_rows(q, s), qr), s
        assert torch.equal(slot_rows(kb, s), slot_rows(kr, s)) and torch.equal(slot_rows(vb, s), slot_rows(vr, s)), s
        rows = new_rows(st[s], L)
        assert int(rows[0]) == 2 * L  # both live slots write rows 2L .. 3L - 1, from different tables rows
        # every new row differs from the pattern, every other row keeps it
        assert not (slot_rows(kb, s)[:, rows] == slot_rows(kb0, s)[:, rows]).all(-1).any(), s
        assert not (slot_rows(vb, s)[:, rows] == slot_rows(vb0, s)[:, rows]).all(-1).any(), s
        keep = torch.ones(5 * L, dtype=torch.bool, device=DEV)
        keep[rows] = False
        assert torch.equal(slot_rows(kb, s)[:, keep], slot_rows(kb0, s)[:, keep]), s
    assert not torch.equal(slot_rows(kb, 0)[:, 2 * L:3 * L], slot_rows(kb, 1)[:, 2 * L:3 * L])
    # the idle slot: ring rows bit for bit as they were, q zero
    assert torch.equal(slot_rows(kb, 2), slot_rows(kb0, 2)) and torch.equal(slot_rows(vb, 2), slot_rows(vb0, 2))
    assert (slot_rows(q, 2) == 0).all()


def joint_slots(k, q, kb, vb, n0, n1, st, window):
    return k.attn_decode_joint_ring_slots_fwd(q, kb, vb, H, D, n0, n1, st, window, score_bound=k.qk_norm_bound(D))


def joint_one(k, q, kb, vb, n0, n1, st, window):
    return k.attn_decode_joint_ring_fwd(q, kb, vb, H, D, n0, n1, st, window, score_bound=k.qk_norm_bound(D),
                                        want_lse=True)


def split(o, n, s):
    """slot s's rows of a per-modality output [B n, H D]"""
    return o.view(B, n, -1)[s::NS].reshape(2 * n, -1)


@pytest.mark.parametrize("n0,n1", FRAMES)
def test_slot_joint_attention_equals_single_state_per_slot(n0, n1):
    k = K()
    L = n0 + n1
    st = states(L)
    q = unit(rnd(B, L, H * D, seed=1))
    kb, vb = pattern(L, 30)
    for window in (0, 2 * L):
        kb1, vb1 = kb.clone(), vb.clone()
        o0, o1, lse = joint_slots(k, q, kb1, vb1, n0, n1, slot_state(st), window)
        assert torch.equal(kb1, kb) and torch.equal(vb1, vb)  # attention writes no ring row
        for s in (0, 1):
            r0, r1, rl = joint_one(k, slot_rows(q, s).contiguous(), slot_rows(kb, s), slot_rows(vb, s), n0, n1,
                                   one_state(st[s]), window)
            for t in (r0, r1, rl):
                assert torch.isfinite(t.float()).all()
            assert torch.equal(split(o0, n0, s), r0) and torch.equal(split(o1, n1, s), r1), (s, window)
            assert torch.equal(slot_rows(lse, s), rl), (s, window)
        assert (split(o0, n0, 2) == 0).all() and (split(o1, n1, 2) == 0).all()
        assert (slot_rows(lse, 2) == float("-inf")).all()
    # the two live slots see different keys: their outputs differ although the queries repeat
    q2 = q.clone()
    q2[1::NS] = q2[0::NS]
    p0, _, pl = joint_slots(k, q2, kb, vb, n0, n1, slot_state(st), 0)
    assert not torch.equal(split(p0, n0, 0), split(p0, n0, 1)) and not torch.equal(slot_rows(pl, 0), slot_rows(pl, 1))


def wide_slots(k, q, kb, vb, st, Lnew, window):
    return k.attn_decode_wide_ring_slots_fwd(q, kb, vb, H, D, st, Lnew, window, score_bound=k.qk_norm_bound(D))


def wide_one(k, q, kb, vb, st, Lnew, window):
    return k.attn_decode_wide_ring_fwd(q, kb, vb, H, D, st, Lnew, window, score_bound=k.qk_norm_bound(D))


@pytest.mark.parametrize("L", [65, 80, 17])
def test_slot_wide_attention_equals_single_state_and_the_joint_slot_form(L):
    k = K()
    st = states(L)
    q = unit(rnd(B, L, H * D, seed=2))
    kb, vb = pattern(L, 30)
    for window in (0, 2 * L):
        kb1, vb1 = kb.clone(), vb.clone()
        o, lse = wide_slots(k, q, kb1, vb1, slot_state(st), L, window)
        assert torch.equal(kb1, kb) and torch.equal(vb1, vb)
        for s in (0, 1):
            ro, rl = wide_one(k, slot_rows(q, s).contiguous(), slot_rows(kb, s), slot_rows(vb, s), one_state(st[s]), L,
                              window)
            assert torch.isfinite(ro.float()).all() and torch.isfinite(rl).all()
            assert torch.equal(slot_rows(o, s), ro) and torch.equal(slot_rows(lse, s), rl), (s, window)
        assert (slot_rows(o, 2) == 0).all() and (slot_rows(lse, 2) == float("-inf")).all()
        # the wide slot form's o equals the joint slot form's o0 | o1, and lse, on the same buffers
        n0, n1 = (64, L - 64) if L > 64 else (16, L - 16)
        o0, o1, jl = joint_slots(k, q, kb, vb, n0, n1, slot_state(st), window)
        assert torch.equal(o[:, :n0].reshape(B * n0, -1), o0) and torch.equal(o[:, n0:].reshape(B * n1, -1), o1)
        assert torch.equal(lse, jl), window
    # a strided destination: the rows beyond the frame keep their sentinel
    big = torch.full((B, L + 3, H * D), 5.0, device=DEV, dtype=torch.bfloat16)
    k.attn_decode_wide_ring_slots_fwd(q, kb, vb, H, D, slot_state(st), L, 0, score_bound=k.qk_norm_bound(D),
                                      o=big[:, :L])
    o, _ = wide_slots(k, q, kb, vb, slot_state(st), L, 0)
    assert torch.equal(big[:, :L], o) and (big[:, L:] == 5.0).all()


@pytest.mark.parametrize("n0,n1", FRAMES)
def test_poisoned_slot_is_alone(n0, n1, table):
    """slot 1 {0, cap - L + 1, 0, 1} (total > cap): its q / o / lse all NaN, its ring rows untouched, slots 0 and
    2 bit-equal to the clean run.  An out-of-contract input the kernels are specified to refuse."""
    k = K()
    cos, sin = table
    L, d = n0 + n1, H * D
    cap = 5 * L
    st = states(L)
    bad = list(st)
    bad[1] = (0, cap - L + 1, 0, 1)
    assert bad[1][1] + L > cap
    qkv0, qkv1 = rnd(B * n0, 3 * d, seed=12), rnd(B * n1, 3 * d, seed=13)
    kb0, vb0 = pattern(L, 40)
    kc, vc = kb0.clone(), vb0.clone()
    qc = run_mm_rope(k, qkv0, qkv1, n0, n1, cos, sin, slot_state(st), kc, vc)  # the clean run
    kb, vb = kb0.clone(), vb0.clone()
    q = run_mm_rope(k, qkv0, qkv1, n0, n1, cos, sin, slot_state(bad), kb, vb)
    assert torch.isnan(slot_rows(q, 1).float()).all()
    assert torch.equal(slot_rows(kb, 1), slot_rows(kb0, 1)) and torch.equal(slot_rows(vb, 1), slot_rows(vb0, 1))
    for s in (0, 2):
        assert torch.equal(slot_rows(q, s), slot_rows(qc, s)), s
        assert torch.equal(slot_rows(kb, s), slot_rows(kc, s)) and torch.equal(slot_rows(vb, s), slot_rows(vc, s)), s
    assert torch.isfinite(slot_rows(q, 0).float()).all() and (slot_rows(q, 2) == 0).all()
    # attention on the buffers as the clean rope left them
    qa = unit(rnd(B, L, H * D, seed=3))
    c0, c1, cl = joint_slots(k, qa, kc, vc, n0, n1, slot_state(st), 0)
    kb1, vb1 = kc.clone(), vc.clone()
    o0, o1, lse = joint_slots(k, qa, kb1, vb1, n0, n1, slot_state(bad), 0)
    assert torch.equal(kb1, kc) and torch.equal(vb1, vc)
    assert torch.isnan(split(o0, n0, 1).float()).all() and torch.isnan(split(o1, n1, 1).float()).all()
    assert torch.isnan(slot_rows(lse, 1)).all()
    for s in (0, 2):
        assert torch.equal(split(o0, n0, s), split(c0, n0, s)) and torch.equal(split(o1, n1, s), split(c1, n1, s)), s
        assert torch.equal(slot_rows(lse, s), slot_rows(cl, s)), s
    assert torch.isfinite(split(o0, n0, 0).float()).all() and (split(o0, n0, 2) == 0).all()
    co, cwl = wide_slots(k, qa, kc, vc, slot_state(st), L, 0)
    o, wl = wide_slots(k, qa, kc, vc, slot_state(bad), L, 0)
    assert torch.isnan(slot_rows(o, 1).float()).all() and torch.isnan(slot_rows(wl, 1)).all()
    for s in (0, 2):
        assert torch.equal(slot_rows(o, s), slot_rows(co, s)) and torch.equal(slot_rows(wl, s), slot_rows(cwl, s)), s
    # a rope offset past the table poisons the q rows of that slot alone as well
    bad[1] = (4 * L, 3 * L, cos.shape[0] - L + 1, 1)
    kb, vb = kb0.clone(), vb0.clone()
    q = run_mm_rope(k, qkv0, qkv1, n0, n1, cos, sin, slot_state(bad), kb, vb)
    assert torch.isnan(slot_rows(q, 1).float()).all() and torch.equal(slot_rows(kb, 1), slot_rows(kb0, 1))
    assert torch.equal(slot_rows(q, 0), slot_rows(qc, 0)) and torch.equal(slot_rows(kb, 0), slot_rows(kc, 0))


def test_slot_entries_refuse_on_the_host(table):
    """B not a multiple of n_slots, or a null lse, returns 1 from the entries and launches nothing: every output
    keeps its sentinel.  (The state has four rows, so the refused n_slots = 4 names rows that exist.)"""
    from owl_wms._lib import lib
    h = lib()
    k = K()
    cos, sin = table
    n0, n1 = 64, 1
    L, d = n0 + n1, H * D
    cap = 5 * L
    st = slot_state(states(L) + [(0, 0, 0, 0)])
    q = unit(rnd(B, L, d, seed=1))
    kb, vb = (t.clone() for t in pattern(L, 50))
    kb0, vb0 = kb.clone(), vb.clone()
    bound, scale = k.qk_norm_bound(D), D ** -0.5
    o = torch.full((B, L, d), 5.0, device=DEV, dtype=torch.bfloat16)
    lse = torch.full((B, H, L), 5.0, device=DEV)
    p = lambda t: t.data_ptr()  # noqa: E731
    kv = (p(kb), kb.stride(1), kb.stride(0), p(vb), vb.stride(1), vb.stride(0))

    def joint(lse_ptr, n_slots):
        o1 = p(o) + 2 * B * n0 * d  # the audio rows behind the video rows of the one sentinel buffer
        return h.owlk_attn_decode_joint_ring_slots_fwd(p(q), q.stride(1), q.stride(0), *kv, p(o), d, o1, d, lse_ptr, B,
                                                       H, n0, n1, D, scale, bound, p(st), n_slots, 0, cap, None)

    def wide(lse_ptr, n_slots):
        return h.owlk_attn_decode_wide_ring_slots_fwd(p(q), q.stride(1), q.stride(0), *kv, p(o), o.stride(1),
                                                      o.stride(0), lse_ptr, B, H, L, D, scale, bound, p(st), n_slots,
                                                      L, 0, cap, None)

    for fn in (joint, wide):
        assert fn(p(lse), 4) == 1  # 6 batch rows on 4 state rows
        assert b"multiple of n_slots" in h.owlk_last_error()
        assert fn(None, 3) == 1  # null lse
        assert fn(p(lse), 0) == 1
    qkv0, qkv1 = rnd(B * n0, 3 * d, seed=10), rnd(B * n1, 3 * d, seed=11)
    for n_slots in (4, 0, -3):
        assert h.owlk_mm_qk_rope_fwd_kv_ring_slots(p(qkv0), 3 * d, p(qkv1), 3 * d, B, 1, n0, n1, H, D, p(cos), p(sin),
                                                   cos.stride(0), cos.shape[0], p(st), n_slots, p(o), o.stride(1),
                                                   o.stride(0), *kv, cap, None) == 1, n_slots
        assert b"multiple of n_slots" in h.owlk_last_error()
    torch.cuda.synchronize()
    assert (o == 5.0).all() and (lse == 5.0).all() and torch.equal(kb, kb0) and torch.equal(vb, vb0)
    # the wrappers refuse the same before the call
    with pytest.raises(AssertionError, match="multiple"):
        k.attn_decode_wide_ring_slots_fwd(q, kb, vb, H, D, st, L, 0, score_bound=bound)
    with pytest.raises(AssertionError, match="slot state"):
        k.attn_decode_joint_ring_slots_fwd(q, kb, vb, H, D, n0, n1, st[0], 0, score_bound=bound)
