"""Attention kernels against probes that resolve single rows and single (query, key) pairs, and a
row-resolved comparison on the existing tests' random inputs.

Every other attention test is a whole-tensor relative L2 error (or a bitwise comparison of two of
our kernels), which a wrong pair at a tile seam, a window edge or a document edge passes.  Here
the references are the dense float64 forms of oracle/attn_probe.py over the mask of
ref_ops.frame_mask; the kernels' own mask helpers only feed the kernels.

  forward    count probe: every (row, residue) count of visible keys and every row's key count
  backward   pair probes: every allowed pair lands in one element of dV, dQ or dK, within 2^-6 of
             that element's absolute budget; the identically zero gradient must be exactly 0;
             outputs start as NaN
  decode     the same probes on attn_decode_fwd (the whole cache buffers coded, dead rows included),
             the split-key form of attn_fwd, attn_decode_joint_fwd and attn_decode_bwd
  random     per (batch, head, row): ||got - ref|| / max(||ref row||, median row norm).  O: 2^-7
             (twice the worst-case bf16 output rounding; the P and q' roundings average over >= 64
             keys), for the unbounded forward and, these inputs keeping |q.k| within qk_norm_bound,
             for the bounded forms production runs (attn_fwd4 / attn_fwd16_k; measured worst 0.0073
             against 0.0033 unbounded).  dQ, dK, dV: 3 x the largest per-row error of the
             bf16-emulating model (attn_probe.bf16_model) over all these cases, measured on the
             CPU: MODEL_ROW_ERR = 0.00862 (dQ; dK 0.00516, dV 0.00451, O 0.00356), so ROW_BOUND_GRAD = 0.02586; fp32
             summation order is what the factor 3 allows for (tests/test_attn_probe_cpu.py asserts
             that the model stays below a third of the bound).
"""
import pytest
import torch

from oracle import attn_probe as P

pytestmark = pytest.mark.gpu

DEV = "cuda"
NAN = float("nan")


def K():
    from owl_wms import kernels
    return kernels


@pytest.fixture(scope="module", autouse=True)
def _needs_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from owl_wms._lib import lib
    lib()


def _ids(cases):
    return [c.id for c in cases]


def _mask(case):
    """the kernels' mask arguments for a case (their own helper: the host code under test)"""
    k = K()
    arrays = None
    if case.docs:
        arrays = k.frame_arrays(case.doc_ids().to(DEV), case.n_frames, case.window, case.causal)
        assert arrays["runs"] == (case.docs == "runs")
    return k.FrameMask(case.tpf, case.window, case.causal, case.q_offset, arrays)


def _delta(o, do, H, D):
    from owl_wms import _lib
    B, L = o.shape[:2]
    delta = torch.empty(B, H, L, device=DEV, dtype=torch.float32)
    _lib.call("owlk_attn_delta", _lib.ptr(o), _lib.ptr(do), o.stride(1), B, L, H, D, _lib.ptr(delta), _lib.stream())
    return delta


# ----------------------------------------------------------------------------- forward count probe
@pytest.mark.parametrize("case", P.FWD_CASES + P.FWD_CASES_128, ids=_ids(P.FWD_CASES + P.FWD_CASES_128))
def test_forward_count_probe(case, monkeypatch):
    """score_bound 0: attn_fwd2_k (D 64) / attn_fwd_k (D 128).  Bounded: OWLK_FWD4 = 1 -> attn_fwd4 for
    document-free training shapes that are unwindowed or have windows of >= 4096 tokens (its pipelined
    run, and the one-tile statement where a row sees one key tile); otherwise and with OWLK_FWD4 = 0
    attn_fwd16_k, with 128-key tiles (D 64) / 48 queries per wave (D 128) on those long sweeps and
    in base form on the short windows."""
    k = K()
    mask = _mask(case)
    for code in ("mod", "div"):
        expect = P.count_expect(case, code, DEV)
        q, kk, v = (P.pack(t, case.B, case.H).to(DEV) for t in P.count_inputs(case, code))
        for bound in (0.0, k.qk_norm_bound(case.D)):
            for fwd4 in (("0", "1") if bound > 0 and case.D == 64 else ("1",)):
                monkeypatch.setenv("OWLK_FWD4", fwd4)
                o = torch.full((case.B, case.Lq, case.H * case.D), NAN, device=DEV, dtype=torch.bfloat16)
                o, lse = k.attn_fwd(q, kk, v, case.H, case.D, mask, o=o, score_bound=bound)
                P.check_count(case, o, lse, expect, f"code {code} bound {bound} OWLK_FWD4={fwd4}")


# ----------------------------------------------------------------------------- backward pair probes
def _fused_variants(case):
    if case.D != 64 or case.docs == "split":
        return ()
    return (0, 5, 129) if case.docs else (0, 1, 5, 128, 129)


def _run_bwd(case, zero, path, monkeypatch, expect, which=("dv", "dq", "dk")):
    """path: "dispatch", "split" (OWLK_BWD_FUSED=0) or a variant of attn_bwd_fused"""
    k = K()
    mask = _mask(case)
    q, kk, v, do = (P.pack(t, case.B, case.H).to(DEV) for t in P.pair_inputs(case, zero))
    o, lse = k.attn_fwd(q, kk, v, case.H, case.D, mask, score_bound=k.qk_norm_bound(case.D))
    got = {n: torch.full_like(q, NAN) for n in ("dq", "dk", "dv")}
    if isinstance(path, int):
        ws = k.attn_bwd_fused(q, kk, v, do, lse, _delta(o, do, case.H, case.D), case.H, case.D, mask, got["dq"], got["dk"],
                              got["dv"], case.scale, path)
        torch.cuda.synchronize()
        assert ws[:256].view(torch.int32)[8].item() == 0, "hand-off wait timed out"
    else:
        if path == "split":
            monkeypatch.setenv("OWLK_BWD_FUSED", "0")
        else:
            monkeypatch.delenv("OWLK_BWD_FUSED", raising=False)
        k.attn_bwd(q, kk, v, o, do, lse, case.H, case.D, mask, got["dq"], got["dk"], got["dv"])
    P.check_pair(case, zero, got, expect, which, f"path {path}")


_BWD = P.BWD_CASES + P.BWD_CASES_128


@pytest.mark.parametrize("zero", ["q", "k"])
@pytest.mark.parametrize("case", _BWD, ids=_ids(_BWD))
def test_backward_pair_probes(case, zero, monkeypatch):
    """kernels.attn_bwd as dispatched (D 64 document-free and run-form documents: the fused pass,
    one wave per SIMD without a window; otherwise the two kernels), with OWLK_BWD_FUSED=0 (the two
    kernels; the general document path for recurring documents), and attn_bwd_fused's variants."""
    expect = P.pair_expect(case, zero, DEV)
    for path in ("dispatch", "split") + _fused_variants(case):
        _run_bwd(case, zero, path, monkeypatch, expect)


@pytest.mark.parametrize("case", P.BWD_TOKEN_CASES, ids=_ids(P.BWD_TOKEN_CASES))
def test_backward_pair_probe_token_causal(case, monkeypatch):
    """tpf 1 with a window of 40 tokens: the dV probe only (every element one term); without a
    window the pair share drops to 0.004 and rows of one key make s_j - m_i vanish."""
    expect = P.pair_expect(case, "q", DEV)
    for path in ("dispatch", "split") + _fused_variants(case):
        _run_bwd(case, "q", path, monkeypatch, expect, which=("dv", "dk"))


@pytest.mark.parametrize("zero", ["q", "k"])
@pytest.mark.parametrize("case", P.BWD_LONG_SPLIT, ids=_ids(P.BWD_LONG_SPLIT))
def test_backward_pair_probes_long_split(case, zero, monkeypatch):
    """71 x 64 tokens, window 64 frames, through the two kernels: the 128-row tiles of long_sweep"""
    _run_bwd(case, zero, "split", monkeypatch, P.pair_expect(case, zero, DEV))


@pytest.mark.parametrize("zero", ["q", "k"])
@pytest.mark.parametrize("case", P.BWD_LONG_W4, ids=_ids(P.BWD_LONG_W4))
def test_backward_pair_probes_long_w4(case, zero, monkeypatch):
    """130 x 64 tokens without a window: the one-wave-per-SIMD kernel's steady run and its drain
    (variant 129, and the default dispatch, which picks it for unwindowed layers)"""
    k = K()
    assert k.fused_bwd_variant(case.D, _mask(case)) & 128
    expect = P.pair_expect(case, zero, DEV)
    for path in (129, "dispatch"):
        _run_bwd(case, zero, path, monkeypatch, expect)


# ----------------------------------------------------------------------------- decode, forward
def _uniform_expect(vcode, lo, hi, B, Lq):
    """count_expect of rows that all see the keys [lo, hi)"""
    counts = vcode[lo:hi].sum(0).to(DEV)[None, None, :].expand(1, Lq, -1)
    assert counts.max().item() <= P.COUNT_CAP
    return counts, torch.full((1, Lq), float(hi - lo), dtype=P.F64, device=DEV)


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("Lq", [64, 50, 1])
@pytest.mark.parametrize("start,cached,window", [(0, 576, 0), (128, 960, 256), (64, 200, 0), (0, 64, 128), (3, 957, 1)])
def test_decode_device_state_count_probe(D, Lq, start, cached, window):
    """attn_fwd16_split_k with the cache position on the device: the whole cache buffers carry the
    count code, rows outside [start, start + cached + Lq) included, so a dead or out-of-window row
    that is read shows as a wrong count."""
    k = K()
    B, H, cap = 2, 2, 2048
    total = cached + Lq
    first = total - window if 0 < window < total else 0
    case = P.unmasked(B, H, Lq, total - first, D=D)
    state = torch.tensor([start, cached, 0, 0], dtype=torch.int64, device=DEV)
    q = torch.zeros(B, Lq, H * D, device=DEV, dtype=torch.bfloat16)
    kb = P.pack(P.onehot(torch.arange(cap), D), B, H).to(DEV)
    for code in ("mod", "div"):
        vcode = P.count_code(cap, D, code)
        vb = P.pack(vcode, B, H).to(DEV)
        o, lse = k.attn_decode_fwd(q, kb, vb, H, D, state, Lq, window, score_bound=k.qk_norm_bound(D))
        P.check_count(case, o, lse, _uniform_expect(vcode, start + first, start + total, B, Lq),
                      f"code {code}: live buffer rows [{start + first}, {start + total})")


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("Lq", [64, 37, 1])
@pytest.mark.parametrize("Lkv", [256, 320, 1000, 4096])
def test_decode_split_keys_count_probe(Lq, Lkv, D):
    """attn_fwd's split-key form (attn_fwd16_split_k: <= 64 queries, unmasked, bounded, >= 4 key tiles)"""
    k = K()
    case = P.unmasked(2, 3, Lq, Lkv, D=D)
    for code in ("mod", "div"):
        q, kk, v = (P.pack(t, case.B, case.H).to(DEV) for t in P.count_inputs(case, code))
        o, lse = k.attn_fwd(q, kk, v, case.H, D, _mask(case), score_bound=k.qk_norm_bound(D))
        P.check_count(case, o, lse, P.count_expect(case, code, DEV), f"code {code}")


@pytest.mark.parametrize("n0,n1", [(64, 1), (64, 16)])
@pytest.mark.parametrize("Lkv", [65, 130, 1000, 1105])
def test_decode_joint_count_probe(n0, n1, Lkv):
    """attn_decode_joint_k: one joint frame of 65 or 80 rows over the key rows, with its lse"""
    k = K()
    D = 64
    case = P.unmasked(2, 2, n0 + n1, Lkv, D=D)
    for code in ("mod", "div"):
        q, kk, v = (P.pack(t, case.B, case.H).to(DEV) for t in P.count_inputs(case, code))
        o0, o1, lse = k.attn_decode_joint_fwd(q, kk, v, case.H, D, n0, n1, score_bound=k.qk_norm_bound(D), want_lse=True)
        o = torch.cat([o0.view(case.B, n0, -1), o1.view(case.B, n1, -1)], 1)
        P.check_count(case, o, lse, P.count_expect(case, code, DEV), f"code {code}")


# ----------------------------------------------------------------------------- decode, backward
def _nan_view(B, L, cols):
    buf = torch.full((B, L + 2, cols + 16), NAN, device=DEV, dtype=torch.bfloat16)
    return buf[:, 1:L + 1, 8:8 + cols], buf


def _surroundings_untouched(buf, L, cols):
    m = torch.ones_like(buf, dtype=torch.bool)
    m[:, 1:L + 1, 8:8 + cols] = False
    return bool(torch.isnan(buf[m].float()).all())


_DEC = [(c, n, z) for c, news in P.DECODE_BWD_CASES for n in news for z in ("q", "k")]


@pytest.mark.parametrize("case,Lnew,zero", _DEC, ids=[f"{c.id}-new{n}-{z}" for c, n, z in _DEC])
def test_decode_backward_pair_probes(case, Lnew, zero):
    """attn_decode_bwd: the dQ probe on every row and the dV / dK probes on the Lnew new key rows;
    rows before Lkv - Lnew belong to the cache, so dk_new / dv_new are views into larger NaN-filled
    buffers whose surroundings must stay untouched."""
    k = K()
    B, H, D, hd = case.B, case.H, case.D, case.H * case.D
    q, kk, v, do = (P.pack(t, B, H).to(DEV) for t in P.pair_inputs(case, zero))
    o, lse = k.attn_fwd(q, kk, v, H, D, _mask(case), score_bound=k.qk_norm_bound(D))
    dq, dq_buf = _nan_view(B, case.Lq, hd)
    dk, dk_buf = _nan_view(B, Lnew, hd) if Lnew else (None, None)
    dv, dv_buf = _nan_view(B, Lnew, hd) if Lnew else (None, None)
    k.attn_decode_bwd(q, kk, v, o, do, lse, H, D, Lnew, dq, dk, dv)
    torch.cuda.synchronize()
    for buf, L in ((dq_buf, case.Lq), (dk_buf, Lnew), (dv_buf, Lnew)):
        assert buf is None or _surroundings_untouched(buf, L, hd), "wrote outside its output view"
    which = ("dv", "dq", "dk") if Lnew else ("dq",)
    P.check_pair(case, zero, {"dq": dq, "dk": dk, "dv": dv}, P.pair_expect(case, zero, DEV), which,
                 f"Lnew {Lnew}", rows=torch.arange(case.Lkv - Lnew, case.Lkv, device=DEV))


# ----------------------------------------------------------------------------- row-resolved random inputs
_RANDOM = P.random_cases()


@pytest.mark.parametrize("case,kind", _RANDOM, ids=[f"{kind}-{c.id}" for c, kind in _RANDOM])
def test_random_inputs_row_resolved(case, kind):
    """The inputs of test_attention_fwd_bwd (ATTN_CASES) and of
    test_attention_bwd_fused_vs_oracle_and_split (FUSED_CASES) through attn_fwd and attn_bwd as
    dispatched, every row of O, dQ, dK and dV on its own."""
    k = K()
    tensors = P.random_inputs(case, kind)
    q, kk, v, do = (t.to(DEV) for t in tensors)
    mask = _mask(case)
    o, lse = k.attn_fwd(q, kk, v, case.H, case.D, mask)
    got = {n: torch.full_like(q, NAN) for n in ("dq", "dk", "dv")}
    k.attn_bwd(q, kk, v, o, do, lse, case.H, case.D, mask, got["dq"], got["dk"], got["dv"])
    got["o"] = o
    # the bounded forward (attn_fwd4 / attn_fwd16_k, what production runs): its promise holds here
    qh, kh = (P.heads(t, case.H, case.D).float() for t in (q, kk))
    assert (qh @ kh.transpose(-1, -2)).abs().max().item() <= k.qk_norm_bound(case.D)
    got["o_bounded"], _ = k.attn_fwd(q, kk, v, case.H, case.D, mask, score_bound=k.qk_norm_bound(case.D))
    ref = P.random_outputs(P.dense_ref, case, tensors, DEV)
    ref["o_bounded"] = ref["o"]
    msg = []
    for name in ("o", "o_bounded", "dq", "dk", "dv"):
        bound = P.ROW_BOUND_O if name.startswith("o") else P.ROW_BOUND_GRAD
        err = P.row_errors(P.heads(got[name], case.H, case.D), ref[name])
        worst = err.max().item()
        print(f"{case.id} {name}: worst row error {worst:.5f} (bound {bound:.5f})")
        if not worst <= bound:  # NaN fails
            bad = ~(err <= bound)
            e = torch.where(torch.isfinite(err), err, torch.full_like(err, float("inf")))  # a NaN row is the worst
            b, h, i = (int(x) for x in (e == e.max()).nonzero()[0])
            msg.append(f"{name}: {int(bad.sum())} rows above {bound:.5f}; worst: batch {b} head {h} row {i} "
                       f"(tile {i // P.TILE}, frame {i // case.tpf} + {i % case.tpf}): {err[b, h, i].item():.5f}")
    assert not msg, f"{case.id}:\n" + "\n".join(msg)
