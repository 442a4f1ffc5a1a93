"""Attention probes that resolve single rows and single (query, key) pairs.

TEST INFRASTRUCTURE ONLY -- see oracle/__init__.py.  Plain dense float64 references of masked
attention and its backward, and probe inputs whose exact answers are small integers or single
terms, so that one wrong (query, key) pair anywhere shows in one named element.  The masks come
from ref_ops.frame_mask (attn.py:24-62 evaluated densely); nothing here knows how a kernel tiles.

Uniform-softmax probes.  With q = 0 or k = 0 every score is exactly 0, so P[i, j] = 1 / n_i on the
n_i visible keys of row i and lse2 = log2 n_i; every input (0, +-1, unit vectors) is exact in bf16.

  count (forward)  V[j] = e_{j mod D} ("mod" code) or e_{(j div D) mod D} ("div" code):
                   O[i, d] n_i = number of visible keys of row i with code d.
  pair (backward)  dO[i] = e_{i mod D}, V[j] = s_j 1_D, s_j = +-1 a fixed hash of j:
                   dV[j, d] = sum_{i sees j, i = d (mod D)} 1 / n_i          (either run)
      run "q" (q = 0, K[j] = e_{j mod D}):
                   dQ[i, d] = scale / n_i sum_{j visible, j = d} (s_j - m_i),  dK == 0
      run "k" (k = 0, Q[i] = e_{i mod D}):
                   dK[j, d] = scale sum_{i sees j, i = d} (s_j - m_i) / n_i,   dQ == 0
                   (m_i: the mean of s over row i's keys)
  selectors        the coded operand (dO and Q rows: sel_q; K rows: sel_k) is non-zero only on the
                   listed 64-row tiles, so that long shapes keep few terms per element.

Tolerances (derived, not measured):
  forward   round(O n_ref) == the integer counts (bf16 output error <= count 2^-9 < 0.25 while
            every count <= 128: asserted on the expected counts); |2^lse2 - n_ref| < 0.25.
  backward  |got - ref| <= 2^-6 A per element, A = the same sum over the absolute values of its
            terms (dense_ref(absolute=True)): four bf16 roundings (P, dS, delta through O, the
            output) of <= 2^-9 on every term give 2^-7 A; the factor 2 is margin.  The gradient
            that is identically zero must be == 0.
  sensitivity  a case is admissible for a probe only if every allowed pair's own term is >= 2^-5 A
            of the element it lands in (twice the tolerance): pair_terms() / min_share().
"""
import math
from dataclasses import dataclass, replace

import torch

from . import ref_ops as R

F64 = torch.float64
BF16 = torch.bfloat16
TILE = 64  # rows of a selector tile (and of the tile coordinates printed on failure)
BWD_TOL = 2.0 ** -6
MIN_SHARE = 2.0 ** -5
COUNT_CAP = 128
LN2 = math.log(2.0)


# ----------------------------------------------------------------------------- cases
@dataclass(frozen=True)
class Case:
    B: int
    H: int
    Lq: int
    Lkv: int
    tpf: int
    window: object = None  # frames
    causal: bool = True
    docs: object = None  # None | "runs" | "split"
    D: int = 64
    sel_q: object = None  # tuple of 64-row query tiles carrying dO / Q rows (None: all)
    sel_k: object = None  # tuple of 64-row key tiles carrying K rows (None: all)

    @property
    def q_offset(self):
        return self.Lkv - self.Lq if self.tpf > 1 or self.causal else 0

    @property
    def n_frames(self):
        return (self.Lkv + self.tpf - 1) // self.tpf

    @property
    def scale(self):
        return self.D ** -0.5

    @property
    def id(self):
        s = f"B{self.B}H{self.H}-{self.Lq}x{self.Lkv}-tpf{self.tpf}-w{self.window}-{'c' if self.causal else 'nc'}"
        if self.docs:
            s += f"-{self.docs}"
        if self.sel_q or self.sel_k:
            s += "-sel" + "_".join(str(t) for t in self.sel_q or ())
        return s + f"-D{self.D}"

    def doc_ids(self):
        """[B, n_frames] int64 or None.  "runs": contiguous documents (the last sample three of
        them); "split": two documents that recur every other pair of frames."""
        if not self.docs:
            return None
        nf = self.n_frames
        doc = torch.zeros(self.B, nf, dtype=torch.long)
        if self.docs == "split":
            doc[:] = (torch.arange(nf) // 2) % 2
        else:
            doc[:, nf // 3:] = 1
            doc[-1, 2 * nf // 3:] = 2
        return doc

    def mask(self):
        """[B or 1, Lq, Lkv] bool from ref_ops.frame_mask"""
        if self.tpf == 1 and not self.causal and self.window is None and not self.docs:
            # the decode kernels have no mask; frame_mask's "no window" is a window of Lkv frames,
            # which would cut query rows >= Lkv off key 0 where a joint frame outnumbers its keys
            return torch.ones(1, self.Lq, self.Lkv, dtype=torch.bool)
        return R.frame_mask(self.Lq, self.Lkv, self.tpf, self.window, self.doc_ids(), self.q_offset, self.causal)

    def locate(self, row, key=None):
        s = f"query row {row} (tile {row // TILE}, frame {(row + self.q_offset) // self.tpf} + {(row + self.q_offset) % self.tpf})"
        if key is not None:
            s += f", key {key} (tile {key // TILE}, frame {key // self.tpf} + {key % self.tpf})"
        return s


def frames(B, H, nf, tpf, window=None, causal=True, docs=None, new=0, **kw):
    """nf frames of tpf tokens; new > 0: cached prefill, the queries are the last `new` frames"""
    return Case(B, H, (new or nf) * tpf, nf * tpf, tpf, window, causal, docs, **kw)


def unmasked(B, H, Lq, Lkv, **kw):
    """the decode kernels' mask: every query sees every key"""
    return Case(B, H, Lq, Lkv, 1, None, False, None, **kw)


# forward count probe: (B, H, n_frames, tpf, window, causal) and documents
FWD_CASES = [
    frames(1, 2, 8, 64), frames(2, 3, 7, 65), frames(1, 2, 7, 65, 3),
    frames(1, 2, 8, 64, 2), frames(1, 2, 10, 64, None, False), frames(1, 2, 8, 64, 3, False),
    frames(1, 1, 300, 1), frames(1, 1, 300, 1, 40),
    frames(2, 2, 8, 64, None, True, "runs"), frames(2, 2, 8, 64, None, True, "split"),
    frames(1, 2, 7, 65, 3, True, "runs"), frames(1, 2, 7, 65, 3, True, "split"),
    frames(1, 1, 71, 64, 64), frames(1, 1, 72, 65, 64),  # the far window edge is reached
    # cached prefill: 2 new frames over 6 cached
    frames(1, 2, 8, 64, None, new=2), frames(1, 2, 8, 65, None, new=2),
    frames(1, 2, 8, 64, 3, new=2), frames(1, 2, 8, 65, 3, new=2),
]
# D 128: launch_fwd<128> and launch_bwd<128> take every mask (no one-wave-per-SIMD forms there)
FWD_CASES_128 = [replace(c, D=128) for c in FWD_CASES]

# backward pair probes: the <= 640-token training shapes.  kernels.attn_bwd serves Lq == Lkv with
# q_offset 0 only, so the cached-prefill cases have no backward to probe.
BWD_CASES = [c for c in FWD_CASES if c.Lq == c.Lkv <= 640 and c.tpf > 1]
BWD_CASES_128 = [replace(c, D=128) for c in BWD_CASES]
# tpf 1: the dV probe only, with a window of at most D tokens (every element a single term)
BWD_TOKEN_CASES = [replace(c, D=D) for c in FWD_CASES if c.tpf == 1 and c.window == 40 for D in (64, 128)]
# long shapes with selectors (first / last tile, the tiles at the window edge and at frame seams).
# Each runs twice, with the near and the far query tiles: rows of 64..128 keys (terms 1 / n_i of
# 2^-6) and rows of >= 4096 keys in one dV / dK element would leave the far pairs a share of 0.005
# to 0.010, below the sensitivity condition; apart they keep >= 0.16.
_K71, _K130 = (0, 1, 6, 7, 63, 64, 70), (0, 1, 63, 64, 128, 129)
BWD_LONG_SPLIT = [frames(1, 1, 71, 64, 64, sel_q=(0, 1), sel_k=_K71),
                  frames(1, 1, 71, 64, 64, sel_q=(63, 64, 65, 70), sel_k=_K71)]
BWD_LONG_W4 = [frames(1, 1, 130, 64, None, sel_q=(0, 1), sel_k=_K130),
               frames(1, 1, 130, 64, None, sel_q=(64, 65, 128, 129), sel_k=_K130)]

# decode backward (unmasked, Lkv <= 512): (Case, the Lnew values: 0, 64 and Lq)
DECODE_BWD_CASES = [(unmasked(2, 2, 64, 384), (0, 64)), (unmasked(1, 2, 65, 325), (0, 64, 65)),
                    (unmasked(1, 2, 128, 448), (0, 64, 128)), (unmasked(1, 2, 64, 384, D=128), (0, 64))]


# ----------------------------------------------------------------------------- probe inputs
def signs(L):
    """s_j = +-1: bit 16 of j * 2654435761 mod 2^32 (Knuth's multiplicative hash)"""
    j = torch.arange(L, dtype=torch.int64)
    return (((j * 2654435761) % (1 << 32)) >> 16 & 1).to(F64) * 2 - 1


def onehot(idx, D):
    out = torch.zeros(idx.numel(), D, dtype=F64)
    out[torch.arange(idx.numel()), idx % D] = 1.0
    return out


def _select(x, tiles):
    if tiles is None:
        return x
    keep = torch.zeros(x.shape[0], dtype=torch.bool)
    for t in tiles:
        keep[t * TILE:(t + 1) * TILE] = True
    return x * keep[:, None].to(x.dtype)


def tile_rows(L, tiles):
    if tiles is None:
        return torch.arange(L)
    return torch.cat([torch.arange(t * TILE, min(L, (t + 1) * TILE)) for t in tiles])


def count_code(L, D, code):
    j = torch.arange(L)
    return onehot(j if code == "mod" else j // D, D)


def count_inputs(case, code):
    """(q, k, v) [L, D] float64 of the forward count probe"""
    return (torch.zeros(case.Lq, case.D, dtype=F64), onehot(torch.arange(case.Lkv), case.D),
            count_code(case.Lkv, case.D, code))


def pair_inputs(case, zero):
    """(q, k, v, do) [L, D] float64 of the backward pair probes; zero = "q" or "k" """
    D = case.D
    i, j = torch.arange(case.Lq), torch.arange(case.Lkv)
    do = _select(onehot(i, D), case.sel_q)
    v = signs(case.Lkv)[:, None].expand(case.Lkv, D).clone()
    if zero == "q":
        q, k = torch.zeros(case.Lq, D, dtype=F64), _select(onehot(j, D), case.sel_k)
    else:
        q, k = _select(onehot(i, D), case.sel_q), torch.zeros(case.Lkv, D, dtype=F64)
    return q, k, v, do


def pack(x, B, H):
    """[L, D] -> the kernels' token-major [B, L, H D] bf16 (every batch and head the same rows)"""
    assert torch.equal(x.to(BF16).to(x.dtype), x), "probe input not exact in bf16"
    return x.to(BF16)[None, :, None, :].expand(B, x.shape[0], H, x.shape[1]).reshape(B, x.shape[0], -1).contiguous()


def heads(t, H, D):
    """the kernels' [B, L, >= H D] -> [B, H, L, D] float64"""
    B, L = t.shape[:2]
    return t[..., :H * D].reshape(B, L, H, D).permute(0, 2, 1, 3).to(F64)


# ----------------------------------------------------------------------------- dense references
def _rows(q, k, mask, scale):
    s = (q @ k.T) * scale
    s = s.masked_fill(~mask, float("-inf"))
    mx = s.amax(-1, keepdim=True)
    mx = torch.where(torch.isfinite(mx), mx, torch.zeros_like(mx))
    e = torch.exp(s - mx)
    l = e.sum(-1, keepdim=True)
    return e, l, mx


def dense_ref(q, k, v, do, mask, scale, absolute=False, chunk=1024):
    """Masked attention and its backward in float64 from a boolean [Lq, Lkv] mask: q, do [Lq, D];
    k, v [Lkv, D] -> dict o, lse2 (base 2; -inf on rows without a key), dq, dk, dv, written out as
    the P, dP, delta and dS products (row chunks only bound the memory).  absolute=True: the same
    sums over the absolute values of their terms (P |V|, P^T |dO|, scale |dS| |K|, scale |dS|^T |Q|),
    the per-element budgets A of the probes' tolerance."""
    q, k, v, do = (t.to(F64) for t in (q, k, v, do))
    Lq, Lkv = q.shape[0], k.shape[0]
    out = {"o": torch.zeros_like(q), "lse2": torch.zeros(Lq, dtype=F64, device=q.device), "dq": torch.zeros_like(q),
           "dk": torch.zeros_like(k), "dv": torch.zeros_like(v)}
    for r0 in range(0, Lq, chunk):
        sl = slice(r0, min(Lq, r0 + chunk))
        e, l, mx = _rows(q[sl], k, mask[sl], scale)
        p = e / l.clamp_min(1e-300)
        o = p @ v
        out["lse2"][sl] = ((mx + torch.log(l)) / LN2).squeeze(-1)
        dp = do[sl] @ v.T
        delta = (do[sl] * o).sum(-1, keepdim=True)
        ds = p * (dp - delta)
        if absolute:
            out["o"][sl] = p @ v.abs()
            out["dv"] += p.T @ do[sl].abs()
            out["dq"][sl] = scale * (ds.abs() @ k.abs())
            out["dk"] += scale * (ds.abs().T @ q[sl].abs())
        else:
            out["o"][sl] = o
            out["dv"] += p.T @ do[sl]
            out["dq"][sl] = scale * (ds @ k)
            out["dk"] += scale * (ds.T @ q[sl])
    return out


def bf(x):
    return x.to(torch.float32).to(BF16).to(F64)


def bf16_model(q, k, v, do, mask, scale, chunk=1024, bwd_mask=None):
    """The rounding chain of a correct kernel on top of exact sums: the unnormalised P and dS enter
    their products as bf16 operands, delta is formed from the forward's bf16 O, and O, dQ, dK, dV
    leave as bf16.  fp32 summation order is not modelled.  bwd_mask: the mask of the backward where
    it differs from the forward's (a backward kernel with a wrong predicate, fed the right lse)."""
    q, k, v, do = (t.to(F64) for t in (q, k, v, do))
    Lq = q.shape[0]
    out = {"o": torch.zeros_like(q), "lse2": torch.zeros(Lq, dtype=F64, device=q.device), "dq": torch.zeros_like(q),
           "dk": torch.zeros_like(k), "dv": torch.zeros_like(v)}
    for r0 in range(0, Lq, chunk):
        sl = slice(r0, min(Lq, r0 + chunk))
        e, l, mx = _rows(q[sl], k, mask[sl], scale)
        lc = l.clamp_min(1e-300)
        o = bf(bf(e) @ v / lc)
        out["o"][sl] = o
        out["lse2"][sl] = ((mx + torch.log(l)) / LN2).squeeze(-1)
        p = e / lc
        if bwd_mask is not None:  # P = exp(s - lse) on the backward's own pairs
            p = torch.exp(((q[sl] @ k.T) * scale - mx).masked_fill(~bwd_mask[sl], float("-inf"))) / lc
        delta = (do[sl] * o).sum(-1, keepdim=True)
        ds = bf(p * (do[sl] @ v.T - delta))
        out["dv"] += bf(p).T @ do[sl]
        out["dq"][sl] = bf(scale * (ds @ k))
        out["dk"] += scale * (ds.T @ q[sl])
    out["dk"], out["dv"] = bf(out["dk"]), bf(out["dv"])
    return out


def per_batch(fn, tensors, mask, scale, **kw):
    """fn (dense_ref / bf16_model) on [L, D] inputs for every mask batch -> dict of [Bm, L, D]"""
    outs = [fn(*tensors, mask[b], scale, **kw) for b in range(mask.shape[0])]
    return {key: torch.stack([o[key] for o in outs]) for key in outs[0]}


# ----------------------------------------------------------------------------- expectations and checks
def count_expect(case, code, device="cpu"):
    """(counts [Bm, Lq, D], n [Bm, Lq]) float64 integers; asserts the cap the tolerance rests on"""
    m = case.mask().to(device)
    vc = count_code(case.Lkv, case.D, code).to(device)
    counts = (m.to(torch.float32) @ vc.to(torch.float32)).to(F64)  # integers < 2^24: exact
    n = m.sum(-1).to(F64)
    assert counts.max().item() <= COUNT_CAP, f"{case.id}: a count of {counts.max().item()} voids the rounding bound"
    assert n.min().item() >= 1 and n.max().item() <= 8192
    return counts, n


def count_bad(case, o, lse2, expect):
    """(rounded counts, wrong (b, h, row, residue) counts, wrong (b, h, row) key counts)"""
    counts, n = expect
    got = torch.round(heads(o, case.H, case.D) * n[:, None, :, None])
    bad = (got != counts[:, None]) | ~torch.isfinite(got)
    return got, bad, ~((torch.exp2(lse2.to(F64)) - n[:, None]).abs() < 0.25)


def check_count(case, o, lse2, expect, what=""):
    """o [B, Lq, >= H D], lse2 [B, H, Lq] against count_expect: every (row, residue) count and
    every row's key count."""
    counts, n = expect
    got, bad, badl = count_bad(case, o, lse2, expect)
    if bad.any() or badl.any():
        msg = [f"count probe {case.id} {what}: {int(bad.sum())} wrong counts, {int(badl.sum())} wrong lse rows"]
        if bad.any():
            b, h, i, d = (int(x) for x in bad.nonzero()[0])
            msg.append(f"  O: batch {b} head {h} {case.locate(i)} residue {d}: counted {got[b, h, i, d].item():.0f}, "
                       f"expected {counts[min(b, counts.shape[0] - 1), i, d].item():.0f} of {n[min(b, n.shape[0] - 1), i].item():.0f} keys")
        if badl.any():
            b, h, i = (int(x) for x in badl.nonzero()[0])
            msg.append(f"  lse: batch {b} head {h} {case.locate(i)}: 2^lse = {2.0 ** lse2[b, h, i].item():.3f}, "
                       f"expected {n[min(b, n.shape[0] - 1), i].item():.0f} keys")
        raise AssertionError("\n".join(msg))


def pair_expect(case, zero, device="cpu"):
    """(ref, A): dense_ref and its absolute form on the pair probe, dicts of [Bm, L, D]"""
    m = case.mask().to(device)
    t = [x.to(device) for x in pair_inputs(case, zero)]
    return per_batch(dense_ref, t, m, case.scale), per_batch(dense_ref, t, m, case.scale, absolute=True)


def pair_bad(case, zero, got, expect, name, rows=None):
    """(got, ref, A, wrong elements) of one gradient, [B, H, L, D] (ref and A with one head)"""
    ref, A = expect
    g = heads(got[name], case.H, case.D)
    r, a = ref[name][:, None], A[name][:, None]
    if rows is not None and name != "dq":
        r, a = r[:, :, rows], a[:, :, rows]
    if name == ("dk" if zero == "q" else "dq"):
        assert not r.any()
        return g, r, a, ~(g == 0)
    return g, r, a, ~((g - r).abs() <= BWD_TOL * a)


def check_pair(case, zero, got, expect, which=("dv", "dq", "dk"), what="", rows=None):
    """got: dict dq / dk / dv [B, L, >= H D] (rows: dk / dv hold only these key rows).  The gradient
    that is identically zero in this run must be exactly zero; the others within 2^-6 A."""
    msg = []
    for name in which:
        g, r, a, bad = pair_bad(case, zero, got, expect, name, rows)
        zero_grad = name == ("dk" if zero == "q" else "dq")
        if bad.any():
            b, h, i, d = (int(x) for x in bad.nonzero()[0])
            row = i if rows is None or name == "dq" else int(rows[i])
            where = case.locate(row) if name == "dq" else f"key row {row} (tile {row // TILE}, frame {row // case.tpf} + {row % case.tpf})"
            bb = min(b, r.shape[0] - 1)
            msg.append(f"  {name}{' (must be 0)' if zero_grad else ''}: {int(bad.sum())} elements; first: batch {b} head {h} "
                       f"{where} residue {d}: got {g[b, h, i, d].item():.6g}, expected {r[bb, 0, i, d].item():.6g}, "
                       f"budget A {a[bb, 0, i, d].item():.6g}")
    if msg:
        raise AssertionError(f"pair probe {case.id} run {zero} {what}:\n" + "\n".join(msg))


# ----------------------------------------------------------------------------- sensitivity and flips
def pair_terms(case, probe, b=0):
    """The own term of every (query, key) pair in a pair probe and the element it lands in.
    probe: "dv", "dk" (rows = the sel_q query rows, every key) or "dq" (every query, the sel_k keys).
    -> (rows, cols, T [r, c] term magnitudes, land(X [L, D]) -> X gathered at each pair's element,
    allowed [r, c])."""
    m = case.mask()[b]
    s = signs(case.Lkv)
    n = m.sum(-1).to(F64).clamp_min(1)
    mean = (m.to(F64) @ s) / n
    if probe == "dq":
        rows, cols = torch.arange(case.Lq), tile_rows(case.Lkv, case.sel_k)
        coded = torch.zeros(case.Lq, dtype=torch.bool)
        coded[tile_rows(case.Lq, case.sel_q)] = True  # dO rows: rows outside carry no gradient at all
    else:
        rows, cols = tile_rows(case.Lq, case.sel_q), torch.arange(case.Lkv)
        coded = torch.ones(case.Lq, dtype=torch.bool)
    sub = m[rows][:, cols]
    if probe == "dv":
        T = (1.0 / n[rows])[:, None].expand(sub.shape).clone()
    else:
        T = case.scale * (s[cols][None, :] - mean[rows][:, None]).abs() / n[rows][:, None]
    T = T * coded[rows][:, None]

    def land(X):
        if probe == "dq":
            return X[rows][:, cols % case.D]  # dQ[i, j mod D]
        return X[cols][:, rows % case.D].T  # dV / dK [j, i mod D]
    return rows, cols, T, land, sub


def min_share(case, probe, A, b=0):
    """smallest own-term / A over the allowed pairs the probe codes (the sensitivity condition)"""
    rows, cols, T, land, sub = pair_terms(case, probe, b)
    coded = sub & (T > 0) if probe == "dq" and case.sel_q is not None else sub
    share = T / land(A).clamp_min(1e-300)
    return share[coded].min().item() if coded.any() else float("inf")


def seam_bug(mask, tpf):
    """a frame-seam bug: the first token of every frame also sees the first token of the next frame
    (1.5 % of all rows wrong; at 32 x 64 tokens it moves O by 3.9e-3 in rel-L2)"""
    m = mask.clone()
    i = torch.arange(0, m.shape[-2] - tpf, tpf)
    m[..., i, i + tpf] = True
    return m


# ----------------------------------------------------------------------------- row-resolved random inputs
ROW_BOUND_O = 2.0 ** -7  # twice the worst-case bf16 output rounding
# the largest per-row error of bf16_model against dense_ref over random_cases(), all of O's and the
# gradients' rows (dQ of the first frames, where a row's 64 keys average the dS roundings least);
# measured on the CPU over every (batch, head) of the cases below 4,000 tokens and the first head of
# the longer ones (their rows repeat the short cases' statistics), asserted by
# tests/test_attn_probe_cpu.py
MODEL_ROW_ERR = 0.00862
ROW_BOUND_GRAD = 3 * MODEL_ROW_ERR  # fp32 summation order is not modelled


def row_errors(got, ref):
    """[B, H, L, D] -> per (b, h, row) ||got - ref|| / max(||ref row||, median row norm of ref)"""
    rn = ref.norm(dim=-1)
    return (got - ref).norm(dim=-1) / torch.maximum(rn, rn.median())


def randn_bf16(shape, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g).to(BF16)


# the inputs of tests/test_kernels_gpu.py ATTN_CASES (seeds 40..43, drawn as [B L, H D]) and of
# tests/test_attn_fused_gpu.py FUSED_CASES (seeds 100..103, drawn as [B, L, H D]), restated
ATTN_CASES = [
    (1, 2, 8, 64, None, False), (1, 2, 8, 64, 2, False), (2, 2, 6, 64, None, True), (1, 1, 40, 1, 16, False),
    (1, 2, 5, 65, 2, False), (2, 1, 9, 4, 3, True), (1, 2, 24, 64, 16, True), (1, 2, 7, 65, None, False),
    (2, 2, 8, 64, None, "split"), (1, 2, 12, 64, 4, "split"), (1, 2, 24, 64, None, False), (1, 1, 300, 1, None, False),
    (1, 2, 80, 64, 64, False), (2, 2, 70, 64, 64, "split"), (1, 2, 72, 65, 64, False),
]
ATTN_CASES_128 = (0, 2, 4, 6, 12, 13)
FUSED_CASES = [
    (1, 2, 8, 64, True, None), (2, 3, 20, 64, True, None), (1, 2, 7, 65, True, None), (1, 1, 300, 1, True, None),
    (1, 2, 40, 64, False, None), (2, 8, 48, 64, True, None), (1, 2, 48, 64, True, 16), (1, 2, 30, 65, True, 4),
    (1, 2, 40, 64, False, 3), (1, 1, 600, 1, True, 100), (2, 3, 30, 65, True, 4),
]


def random_cases():
    """[(Case, "attn" | "fused")] of the existing tests' random-input cases"""
    out = []
    for i, (B, H, nf, tpf, window, docs) in enumerate(ATTN_CASES):
        d = "split" if docs == "split" else ("runs" if docs else None)
        out.append((frames(B, H, nf, tpf, window, True, d), "attn"))
    for i in ATTN_CASES_128:
        out.append((replace(out[i][0], D=128), "attn"))
    for B, H, nf, tpf, causal, window in FUSED_CASES:
        out.append((frames(B, H, nf, tpf, window, causal), "fused"))
    return out


def random_inputs(case, kind):
    """(q, k, v, do) [B, L, H D] bf16 on the CPU, bit for bit what the existing tests draw"""
    B, L, hd = case.B, case.Lkv, case.H * case.D
    if kind == "attn":
        return tuple(randn_bf16((B * L, hd), 40 + i).view(B, L, hd) for i in range(4))
    return tuple(randn_bf16((B, L, hd), 100 + i) for i in range(4))


def random_outputs(fn, case, tensors, device="cpu", first_head_only=False):
    """fn (dense_ref / bf16_model) over every (batch, head) -> dict of [B, H, L, D] float64
    (first_head_only: [1, 1, L, D] of batch 0, head 0)"""
    m = case.mask().to(device)
    q, k, v, do = (heads(t.to(device), case.H, case.D) for t in tensors)
    B, H = (1, 1) if first_head_only else (case.B, case.H)
    res = {}
    for b in range(B):
        for h in range(H):
            r = fn(q[b, h], k[b, h], v[b, h], do[b, h], m[min(b, m.shape[0] - 1)], case.scale)
            for key, val in r.items():
                res.setdefault(key, []).append(val)
    return {key: torch.stack(val).view(B, H, *val[0].shape) for key, val in res.items()}
