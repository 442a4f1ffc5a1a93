"""The attention probes of oracle/attn_probe.py proved on the CPU before any kernel sees them, for
every case tests/test_attn_exact_gpu.py runs:

  (a) the bf16-emulating model of a correct kernel passes every probe;
  (b) the sensitivity condition holds: every allowed pair's own term is >= 2^-5 of the absolute
      budget A of the element it lands in;
  (c) single-pair flips of the mask fail a probe assertion.  A backward kernel that drops or adds
      the pair (i, j) (P[i, j] = 2^(0 - lse_i) = 1 / n_i from the forward's lse) moves exactly one
      element of dV, dQ and dK by the pair's own term; the flip is caught where that term, less the
      model's own rounding error in that element, exceeds the tolerance 2^-6 A.  Removed pairs:
      every allowed pair the probe codes (all of them below 640 tokens; on the long cases all pairs
      of the selected tiles, > 10^5, which hold the tile, frame and window edges).  Added pairs:
      every disallowed pair in the same or the adjacent frame.  In the forward a flipped pair moves
      2^lse by one key against a tolerance of a quarter.  Besides that derivation, sampled real
      flips (up to 50 removed and 50 added pairs per probe, in distinct rows and elements) go
      through the model and the probe assertions themselves: check_count / check_pair must raise and
      flag every flipped pair's own row or element;
  (d) a frame-seam bug (the first token of every frame also sees the first token of the next
      frame) passes rel-L2 < 1e-2 at 32 x 64 tokens and fails the count probe;
  and the dense reference equals fp32 autograd and the probes' closed forms.
"""
import functools
from dataclasses import replace

import pytest
import torch

from oracle import attn_probe as P
from oracle import ref_ops as R

FWD = P.FWD_CASES + P.FWD_CASES_128
# decode forward: rows that all see the same keys; the shapes of the GPU file's three decode tests
DECODE_FWD = ([P.unmasked(1, 1, Lq, n, D=D) for D in (64, 128) for Lq in (64, 1) for n in (640, 626, 577, 256, 264, 250, 201, 128, 114, 65, 1)]
              + [P.unmasked(1, 1, Lq, Lkv, D=D) for D in (64, 128) for Lq in (64, 37, 1) for Lkv in (256, 320, 1000, 4096)]
              + [P.unmasked(1, 1, Lq, Lkv) for Lq in (65, 80) for Lkv in (65, 130, 1000, 1105)])
BWD = P.BWD_CASES + P.BWD_CASES_128 + P.BWD_LONG_SPLIT + P.BWD_LONG_W4 + [c for c, _ in P.DECODE_BWD_CASES]
BWD_RUNS = [(c, z) for c in BWD for z in ("q", "k")] + [(c, "q") for c in P.BWD_TOKEN_CASES]
N_FLIPS = 50


def _ids(cases):
    return [c.id for c in cases]


def _probes(case, zero):
    if case.tpf == 1 and case.causal:
        return ("dv",)
    return ("dv", "dq") if zero == "q" else ("dv", "dk")


@functools.lru_cache(maxsize=None)
def _analysis(case, zero):
    """(ref, A, model) of a pair probe, dicts of [Bm, L, D]"""
    ref, A = P.pair_expect(case, zero)
    model = P.per_batch(P.bf16_model, P.pair_inputs(case, zero), case.mask(), case.scale)
    return ref, A, model


def _as_kernel_output(case, t):
    """[Bm, L, D] -> what a kernel would hand back for a one-head case"""
    return replace(case, H=1), t.to(torch.bfloat16)


# ----------------------------------------------------------------------------- the dense reference itself
def test_dense_ref_equals_autograd_and_closed_forms():
    case = P.frames(2, 1, 5, 13, 2, True, "runs")
    g = torch.Generator().manual_seed(1)
    q, k, v, do = (torch.randn(case.Lkv, 16, generator=g, dtype=P.F64) for _ in range(4))
    m = case.mask()[1]
    qa, ka, va = (t.clone().requires_grad_() for t in (q, k, v))
    s = (qa @ ka.T * 0.3).masked_fill(~m, float("-inf"))
    o = torch.softmax(s, -1) @ va
    o.backward(do)
    r = P.dense_ref(q, k, v, do, m, 0.3, chunk=7)
    for got, want in ((r["o"], o.detach()), (r["dq"], qa.grad), (r["dk"], ka.grad), (r["dv"], va.grad),
                      (r["lse2"], torch.logsumexp(s.detach(), -1) / P.LN2)):
        assert (got - want).abs().max().item() < 1e-12
    # the closed forms of the module docstring, on a 65-token-frame window case
    case = P.FWD_CASES[2]
    m = case.mask()[0].to(P.F64)
    n, sg, D = m.sum(-1), P.signs(case.Lkv), case.D
    mean = (m @ sg) / n
    ri = P.onehot(torch.arange(case.Lq), D)
    ref, A, _ = _analysis(case, "q")
    assert (ref["dv"][0] - (m / n[:, None]).T @ ri).abs().max().item() < 1e-12
    ds = m * (sg[None, :] - mean[:, None]) / n[:, None]
    assert (ref["dq"][0] - case.scale * ds @ ri).abs().max().item() < 1e-12
    assert not ref["dk"].any()
    ref, A, _ = _analysis(case, "k")
    assert (ref["dk"][0] - case.scale * ds.T @ ri).abs().max().item() < 1e-12
    assert not ref["dq"].any()
    assert (ref["lse2"][0] - torch.log2(n)).abs().max().item() < 1e-12


# ----------------------------------------------------------------------------- (a) forward
@pytest.mark.parametrize("case", FWD + DECODE_FWD, ids=_ids(FWD + DECODE_FWD))
def test_a_model_passes_count_probe_and_a_flipped_key_fails(case):
    for code in ("mod", "div"):
        expect = P.count_expect(case, code)
        q, k, v = P.count_inputs(case, code)
        mod = P.per_batch(P.bf16_model, (q, k, v, torch.zeros_like(q)), case.mask(), case.scale)
        c1, o = _as_kernel_output(case, mod["o"])
        P.check_count(c1, o, mod["lse2"][:, None], expect, f"model, code {code}")
        # (c) forward: one key more or fewer moves 2^lse by 1; the model's own error leaves > 0.25 of it
        err = (torch.exp2(mod["lse2"]) - expect[1]).abs().max().item()
        assert 1.0 - err > 0.25
    if case in FWD:
        _real_forward_flips(case)


def _real_forward_flips(case):
    """sampled single-pair flips through the model and check_count itself"""
    g = torch.Generator().manual_seed(5)
    mask = case.mask()
    flipped = mask.clone()
    fk = torch.arange(case.Lkv) // case.tpf
    picks = []
    for b in range(mask.shape[0]):
        for n_, i in enumerate(torch.randperm(case.Lq, generator=g)[:2 * N_FLIPS].tolist()):
            row = mask[b, i]
            near = (fk - (i + case.q_offset) // case.tpf).abs() <= 1
            cand = (~row & near) if n_ % 2 else (row if int(row.sum()) > 1 else row & False)
            cand = cand.nonzero()[:, 0]
            if cand.numel():
                j = int(cand[int(torch.randint(cand.numel(), (1,), generator=g))])
                flipped[b, i, j] = ~mask[b, i, j]
                picks.append((b, i))
    assert len(picks) >= N_FLIPS // 2
    q, k, v = P.count_inputs(case, "mod")
    mod = P.per_batch(P.bf16_model, (q, k, v, torch.zeros_like(q)), flipped, case.scale)
    c1, o = _as_kernel_output(case, mod["o"])
    expect = P.count_expect(case, "mod")
    with pytest.raises(AssertionError, match="count probe"):
        P.check_count(c1, o, mod["lse2"][:, None], expect)
    _, bad, badl = P.count_bad(c1, o, mod["lse2"][:, None], expect)
    assert int(badl.sum()) == len(picks)  # exactly the flipped rows
    for b, i in picks:
        assert badl[b, 0, i] and bad[b, 0, i].any(), case.locate(i)


# ----------------------------------------------------------------------------- (a), (b), (c) backward
@pytest.mark.parametrize("case,zero", BWD_RUNS, ids=[f"{c.id}-{z}" for c, z in BWD_RUNS])
def test_abc_backward_pair_probes(case, zero):
    ref, A, model = _analysis(case, zero)
    probes = _probes(case, zero)
    # (a) the model of a correct kernel passes, the zero gradient exactly
    c1 = replace(case, H=1)
    which = probes + (("dk",) if zero == "q" else ("dq",))
    P.check_pair(c1, zero, {n: model[n].to(torch.bfloat16) for n in which}, (ref, A), which, "model")
    for b in range(ref["dv"].shape[0]):
        for probe in probes:
            # (b) sensitivity
            share = P.min_share(case, probe, A[probe][b], b)
            assert share >= P.MIN_SHARE, f"{case.id} {probe} batch {b}: smallest pair share {share:.4f}"
            # (c) flips
            rows, cols, T, land, allowed = P.pair_terms(case, probe, b)
            coded = T > 0
            caught = T - land((model[probe][b] - ref[probe][b]).abs()) > P.BWD_TOL * land(A[probe][b])
            removed = allowed & coded
            assert removed.any()
            miss = removed & ~caught
            assert not miss.any(), f"{case.id} {probe}: {int(miss.sum())} of {int(removed.sum())} removed pairs pass; " \
                                   f"first {case.locate(int(rows[miss.nonzero()[0][0]]), int(cols[miss.nonzero()[0][1]]))}"
            fq, fk = (rows + case.q_offset) // case.tpf, cols // case.tpf
            added = ~allowed & coded & ((fq[:, None] - fk[None, :]).abs() <= 1)
            miss = added & ~caught
            assert not miss.any(), f"{case.id} {probe}: {int(miss.sum())} of {int(added.sum())} added pairs pass; " \
                                   f"first {case.locate(int(rows[miss.nonzero()[0][0]]), int(cols[miss.nonzero()[0][1]]))}"


    _real_backward_flips(case, zero, probes, (ref, A))


def _real_backward_flips(case, zero, probes, expect):
    """sampled single-pair flips of the backward's mask (the forward, so lse and delta, keeps the
    right one) through the model and check_pair itself: every flipped pair's own element is flagged"""
    g = torch.Generator().manual_seed(6)
    mask = case.mask()
    flipped = mask.clone()
    picks = []
    for b in range(mask.shape[0]):
        used_rows, used_kv = set(), set()
        for probe in probes:
            rows, cols, T, land, allowed = P.pair_terms(case, probe, b)
            fq, fk = (rows + case.q_offset) // case.tpf, cols // case.tpf
            near = (fq[:, None] - fk[None, :]).abs() <= 1
            n_each = min(N_FLIPS, rows.numel() // (2 * len(probes)))
            for cand in (allowed & (T > 0), ~allowed & (T > 0) & near):
                idx = cand.nonzero()
                got = 0
                for r, c in idx[torch.randperm(idx.shape[0], generator=g)[:40 * n_each]].tolist():
                    i, j = int(rows[r]), int(cols[c])
                    if i in used_rows or (j, i % case.D) in used_kv:
                        continue
                    used_rows.add(i), used_kv.add((j, i % case.D))
                    flipped[b, i, j] = ~mask[b, i, j]
                    picks.append((b, probe, i, j))
                    got += 1
                    if got == n_each:
                        break
                assert got or not idx.shape[0]
    assert picks
    t = P.pair_inputs(case, zero)
    outs = [P.bf16_model(*t, mask[b], case.scale, bwd_mask=flipped[b]) for b in range(mask.shape[0])]
    got = {n: torch.stack([o[n] for o in outs]).to(torch.bfloat16) for n in ("dq", "dk", "dv")}
    c1 = replace(case, H=1)
    with pytest.raises(AssertionError, match="pair probe"):
        P.check_pair(c1, zero, got, expect, probes)
    bad = {probe: P.pair_bad(c1, zero, got, expect, probe)[3] for probe in probes}
    for b, probe, i, j in picks:
        hit = bad[probe][b, 0, i, j % case.D] if probe == "dq" else bad[probe][b, 0, j, i % case.D]
        assert hit, f"{probe}: flipped pair passes: {case.locate(i, j)}"
    # and the gradient that is identically zero stays exactly zero under the flips
    zero_name = "dk" if zero == "q" else "dq"
    assert not P.pair_bad(c1, zero, got, expect, zero_name)[3].any()


def test_b_token_causal_without_window_is_not_admissible():
    """why tpf 1 runs only as the count probe and the windowed dV probe"""
    case = P.frames(1, 1, 300, 1)
    _, A = P.pair_expect(case, "q")
    assert P.min_share(case, "dv", A["dv"][0]) < P.MIN_SHARE


# ----------------------------------------------------------------------------- (d)
def test_d_frame_seam_bug_passes_rel_l2_and_fails_count_probe():
    case = P.frames(1, 1, 32, 64)
    L, D = case.Lkv, case.D
    good = case.mask()
    bad = P.seam_bug(good, case.tpf)
    assert int((bad & ~good).sum()) == 31
    q, k, v = (P.randn_bf16((1, 1, L, D), 40 + i).float() for i in range(3))
    o_good, o_bad = R.attention(q, k, v, good), R.attention(q, k, v, bad)
    rel = ((o_bad - o_good).norm() / o_good.norm()).item()
    assert rel < 1e-2, rel  # what every whole-tensor check lets through (3.9e-3)
    cq, ck, cv = P.count_inputs(case, "mod")
    mod = P.per_batch(P.bf16_model, (cq, ck, cv, torch.zeros_like(cq)), bad, case.scale)
    with pytest.raises(AssertionError, match=r"31 wrong counts, 31 wrong lse rows\n  O: batch 0 head 0 query row 0 "):
        P.check_count(case, mod["o"].to(torch.bfloat16), mod["lse2"][:, None], P.count_expect(case, "mod"))


# ----------------------------------------------------------------------------- row-resolved bound
def test_model_row_errors_stay_below_a_third_of_the_gradient_bound():
    worst = {}
    for case, kind in P.random_cases():
        t = P.random_inputs(case, kind)
        first = case.Lkv >= 4000  # the long cases on their first head: their rows repeat the short ones' statistics
        ref = P.random_outputs(P.dense_ref, case, t, first_head_only=first)
        mod = P.random_outputs(P.bf16_model, case, t, first_head_only=first)
        for name in ("o", "dq", "dk", "dv"):
            worst[name] = max(worst.get(name, 0.0), P.row_errors(mod[name], ref[name]).max().item())
    print("bf16 model, worst per-row errors:", {n: round(e, 5) for n, e in worst.items()})
    assert worst["o"] <= P.ROW_BOUND_O
    assert max(worst[n] for n in ("dq", "dk", "dv")) <= P.ROW_BOUND_GRAD / 3
    assert max(worst[n] for n in ("dq", "dk", "dv")) >= 0.9 * P.MODEL_ROW_ERR  # the recorded figure is the measured one
