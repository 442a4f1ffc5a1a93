"""Kernel-level tests of the wide ring decode attention (include/owlk.h: owlk_attn_decode_wide_ring_fwd), the
dit backbone's 65-row audio + video frame on a ring cache: attn_decode_joint_k's ring body with one output.

Tolerances.  Against the joint ring kernel on the same buffers and state: torch.equal (the same body, only
the output addressing differs).  Against fp32 torch attention over the gathered logical keys: rel-L2 1e-2,
on the last row alone too; against attn_fwd unmasked on the same keys: |lse| 4e-3, O rel-L2 5e-3 -- the
bounds of test_joint_decode_attention.

Shapes: B 2, H 2, D 64, a ring of 390 rows (6 frames of 65: no multiple of the 64-key tile), Lq 65 (four
full query tiles and one row of the fifth) and 80 (all five full); every state unwindowed and with a
130-key window."""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
B, H, D = 2, 2, 64
CAP = 390
WINDOW = 130
CANARY = 768.0  # exact in bf16, far outside any attention output of unit-variance V


def K():
    from owl_wms import kernels
    return kernels


def rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


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


def ring_states(L):
    """(name, start, cached) for Lnew = L new rows on the CAP-row ring (tests/test_stream_ring_gpu.py's)"""
    return [("no wrap", 0, 130),
            ("wrap inside a key tile and a 16-row DMA group", CAP - 40, 130),
            ("wrap on a tile boundary", CAP - 64, 130),
            ("the new rows wrap", 200, CAP - 200 - 10),
            ("full ring", 100, CAP - L)]


_IN = {}


def _inputs(L):
    """unit-RMS q and ring buffers, made once per Lq and read-only"""
    if L not in _IN:
        _IN[L] = (unit(rnd(B, L, H * D, seed=1)), unit(rnd(B, CAP, H * D, seed=2)), rnd(B, CAP, H * D, seed=3))
    return _IN[L]


def _logical(buf, start, cached, L, window):
    """the visible logical keys [first, total) of the ring, gathered"""
    total = cached + L
    first = total - window if window > 0 and total > window else 0
    rows = (torch.arange(first, total, device=DEV) + start) % CAP
    return buf.index_select(1, rows)


_REF = {}


def _fp32_reference(L, start, cached, window):
    """fp32 torch attention over the gathered logical keys, computed once per case"""
    key = (L, start, cached, window)
    if key not in _REF:
        q, kb, vb = _inputs(L)
        kk, v = _logical(kb, start, cached, L, window), _logical(vb, start, cached, L, window)
        qf, kf, vf = (t.float().view(B, -1, H, D).transpose(1, 2) for t in (q, kk, v))
        _REF[key] = (torch.softmax(qf @ kf.transpose(-1, -2) * D ** -0.5, dim=-1) @ vf).transpose(1, 2).reshape(
            B, L, H * D)
    return _REF[key]


def _guarded_out(L, pad=8, col_pad=64, row_pad=3):
    """o as a strided view of a canary-filled buffer: ldo = H D + col_pad > H D, batch stride (L + row_pad +
    16) ldo > L ldo, 16 spare rows behind each batch's block and `pad` rows around it all -> (buffer, view,
    mask of the view's elements)"""
    d = H * D
    rows = L + row_pad + 16
    buf = torch.full((pad + B * rows + pad, d + col_pad), CANARY, device=DEV, dtype=torch.bfloat16)
    o = buf[pad:pad + B * rows].view(B, rows, d + col_pad)[:, :L, :d]
    assert o.stride(1) > d and o.stride(0) > L * o.stride(1)
    inside = torch.zeros_like(buf, dtype=torch.bool)
    inside[pad:pad + B * rows].view(B, rows, d + col_pad)[:, :L, :d] = True
    return buf, o, inside


@pytest.mark.parametrize("L", [65, 80])
def test_wide_ring_attention(L):
    """Every ring state, unwindowed and with a 130-key window: == the joint ring kernel (n0 = L - 1, n1 = 1) bit
    for bit, == fp32 torch attention and == attn_fwd on the gathered logical keys within the joint kernel's
    bounds, written through a strided o with nothing outside its B x L x H D block touched (at L = 65 no row
    65..79), and the same bits on a second call."""
    k = K()
    q, kb, vb = _inputs(L)
    n0, n1, d = L - 1, 1, H * D
    bound = k.qk_norm_bound(D)
    for name, start, cached in ring_states(L):
        assert 0 <= start < CAP and cached + L <= CAP, name
        if name == "the new rows wrap":
            assert start + cached < CAP < start + cached + L
        for window in (0, WINDOW):
            case = (name, window)
            st = dev_state(start, cached)
            buf, o, inside = _guarded_out(L)
            _, lse = k.attn_decode_wide_ring_fwd(q, kb, vb, H, D, st, L, window, score_bound=bound, o=o)
            torch.cuda.synchronize()
            assert torch.isfinite(o.float()).all() and torch.isfinite(lse).all(), case
            assert (buf[~inside] == CANARY).all(), case  # rows L..L+18 of each batch, the pad columns, the ends
            assert not (o == CANARY).all(-1).any(), case

            j0, j1, jl = k.attn_decode_joint_ring_fwd(q, kb, vb, H, D, n0, n1, st, window, score_bound=bound,
                                                      want_lse=True)
            assert torch.isfinite(j0.float()).all() and torch.isfinite(j1.float()).all() and \
                torch.isfinite(jl).all(), case
            assert torch.equal(o[:, :n0], j0.view(B, n0, d)), case
            assert torch.equal(o[:, n0:], j1.view(B, n1, d)), case
            assert torch.equal(lse, jl), case

            ref = _fp32_reference(L, start, cached, window)
            assert torch.isfinite(ref).all(), case
            r_all, r_last = rel(o, ref), rel(o[:, -1:], ref[:, -1:])
            print(f"wide ring decode L={L} {name}, window {window}: rel all {r_all:.2e} last row {r_last:.2e}")
            assert r_all < 1e-2, case
            assert r_last < 1e-2, case

            kk, v = _logical(kb, start, cached, L, window), _logical(vb, start, cached, L, window)
            og, lse_g = k.attn_fwd(q, kk, v, H, D, k.FrameMask(1, None, False, 0, None), score_bound=bound)
            assert torch.isfinite(og.float()).all() and torch.isfinite(lse_g).all(), case
            assert (lse - lse_g).abs().max().item() < 4e-3, case
            assert rel(o, og) < 5e-3, case

            o2, lse2 = k.attn_decode_wide_ring_fwd(q, kb, vb, H, D, st, L, window, score_bound=bound)
            assert o2.is_contiguous() and torch.equal(o2, o) and torch.equal(lse2, lse), case


@pytest.mark.parametrize("L", [65, 80])
def test_wide_ring_window_hides_the_keys_before_it(L):
    """start = CAP - 40, cached 130, window 130: overwriting the hidden keys (and every dead row of the ring)
    changes no bit."""
    k = K()
    q, kb, vb = _inputs(L)
    start, cached = CAP - 40, 130
    st, bound = dev_state(start, cached), k.qk_norm_bound(D)
    o, lse = k.attn_decode_wide_ring_fwd(q, kb, vb, H, D, st, L, WINDOW, score_bound=bound)
    first, total = cached + L - WINDOW, cached + L
    visible = torch.zeros(CAP, dtype=torch.bool, device=DEV)
    visible[(torch.arange(first, total, device=DEV) + start) % CAP] = True
    n_hid = int((~visible).sum())
    assert n_hid == CAP - WINDOW
    kb2, vb2 = kb.clone(), vb.clone()
    kb2[:, ~visible] = unit(rnd(B, n_hid, H * D, seed=4))
    vb2[:, ~visible] = rnd(B, n_hid, H * D, seed=5)
    o2, lse2 = k.attn_decode_wide_ring_fwd(q, kb2, vb2, H, D, st, L, WINDOW, score_bound=bound)
    assert torch.isfinite(o.float()).all() and torch.isfinite(lse).all()
    assert torch.equal(o, o2) and torch.equal(lse, lse2)
    # and the visible ones are read: changing one of them changes the output
    kb3 = kb.clone()
    kb3[:, (start + first) % CAP] = -kb[:, (start + first) % CAP]
    o3, _ = k.attn_decode_wide_ring_fwd(q, kb3, vb, H, D, st, L, WINDOW, score_bound=bound)
    assert not torch.equal(o, o3)


@pytest.mark.parametrize("L", [65, 80])
def test_wide_ring_states_outside_the_contract_are_not_followed(L):
    """start = cap, cached + Lnew > cap, a negative cached (and a negative start): o and lse all NaN, the K / V
    buffers unchanged.  The last state inside the contract, a full ring starting at its last row, is
    followed."""
    k = K()
    q, kb0, vb0 = _inputs(L)
    kb, vb = kb0.clone(), vb0.clone()
    bound = k.qk_norm_bound(D)
    for st in ([CAP, 0], [0, CAP - L + 1], [CAP - 8, CAP - L + 1], [0, -1], [-65, 0]):
        buf, o, inside = _guarded_out(L)
        _, lse = k.attn_decode_wide_ring_fwd(q, kb, vb, H, D, dev_state(*st), L, 0, score_bound=bound, o=o)
        torch.cuda.synchronize()
        assert torch.equal(kb, kb0) and torch.equal(vb, vb0), st
        assert torch.isnan(o.float()).all() and torch.isnan(lse).all(), st
        assert (buf[~inside] == CANARY).all(), st
    o, lse = k.attn_decode_wide_ring_fwd(q, kb, vb, H, D, dev_state(CAP - 1, CAP - L), L, 0, score_bound=bound)
    assert torch.isfinite(o.float()).all() and torch.isfinite(lse).all()
