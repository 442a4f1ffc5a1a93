"""The core the attention asm generators (gen_fused4_asm.py, gen_fwd4_asm.py) share: the instruction
record, register-list helpers, the wait / hazard pass and the gap filler.

finalize() counts every LDS operation (in-order completion; lgkmcnt is 4 bits, so counts above 15
over-wait) and pads the MFMA hazards with s_nop:
  VALU write -> MFMA read: 2 wait states; 16x16x32 MFMA write -> VALU / LDS read: 8 (hipcc's own
  padding on gfx950), 32x32x16: 12; MFMA read or write -> VALU / LDS-load write of that register:
  12 (margin).
"""
import re


class Ins:
    __slots__ = ("text", "kind", "reads", "writes", "lds", "cost", "mfma_c", "passes", "meta")

    def __init__(self, text, kind, reads=(), writes=(), lds=False, cost=4, mfma_c=(), passes=4, meta=None):
        self.text = text
        self.kind = kind  # mfma | valu | exp | ldsr | ldsw | cmp | nop | wait | salu | raw
        self.reads = list(reads)  # physical registers ('v', n) / ('a', n)
        self.writes = list(writes)
        self.lds = lds
        self.cost = cost
        self.mfma_c = list(mfma_c)  # registers read as the accumulator input (chain)
        self.passes = passes
        self.meta = meta  # the instruction's meaning for a schedule check: (op, ...)


def vr(lo, n):
    return [("v", lo + i) for i in range(n)]


def ar(lo, n):
    return [("a", lo + i) for i in range(n)]


def rng(f, lo, n):
    return f"{f}[{lo}:{lo + n - 1}]" if n > 1 else f"{f}{lo}"


def interleave(mfmas, fillers, lo=0, hi=None, first=None):
    """place the filler instructions (in order) evenly into the gaps before mfmas[lo:hi]; returns the
    program.  first: a list of filler groups that must go before specific MFMA indices {idx: [ins]}"""
    n = len(mfmas)
    hi = n if hi is None else hi
    slots = [[] for _ in range(n + 1)]
    if first:
        for i, ins in first.items():
            slots[i] += ins
    m = len(fillers)
    for k, x in enumerate(fillers):
        g = lo + (k * (hi - lo)) // max(m, 1)
        slots[g].append(x)
    prog = []
    for i in range(n):
        prog += slots[i]
        prog.append(mfmas[i])
    prog += slots[n]
    return prog


def finalize(prog, allow_pending=False):
    """Insert lgkmcnt waits and hazard nops; returns the instruction texts and statistics.  allow_pending:
    LDS loads may still fly at the end (the caller drains them with lgkmcnt(0) before their use)."""
    out = []
    # LDS bookkeeping
    issued = 0          # LDS ops issued so far
    done_upto = 0       # all LDS ops with index < done_upto are known complete
    pending = {}        # register -> LDS op index that writes it (loads not yet waited for)
    # hazard bookkeeping: per register (position in wait states) of last write / MFMA access
    pos = 0
    last_w = {}   # reg -> (pos, kind)
    last_mfma = {}  # reg -> pos of the last MFMA reading it as the accumulator or writing it
    last_ab = {}    # reg -> pos of the last MFMA reading it as the A / B operand
    nops = waits = 0

    def ws_since(p):
        return pos - p - 1  # instructions strictly between

    for ins in prog:
        if ins.kind == "wait":
            out.append(ins.text)
            pos += 1
            if "lgkmcnt(0)" in ins.text:
                done_upto = issued
                pending.clear()
            continue
        # 1. LDS results this instruction consumes
        # (an LDS load's WAR on its destination against an older LDS read of the same registers is ordered
        # (in-order), so only reads are looked up)
        need = -1
        for r in ins.reads:
            if r in pending:
                need = max(need, pending[r])
        if need >= done_upto:
            cnt = issued - need - 1
            cnt = min(cnt, 15)
            out.append(f"s_waitcnt lgkmcnt({cnt})")
            waits += 1
            pos += 1
            done_upto = issued - cnt
            for r in list(pending):
                if pending[r] < done_upto:
                    del pending[r]
        # 2. hazards
        pad = 0
        if ins.kind == "mfma":
            for r in ins.reads:
                if r in ins.mfma_c and last_w.get(r, (-99, "", 0))[1] == "mfma":
                    continue  # accumulate chain
                w = last_w.get(r)
                if w and w[1] in ("valu", "exp"):
                    pad = max(pad, 2 - ws_since(w[0]))
                if w and w[1] == "mfma":
                    pad = max(pad, w[2] + 4 - ws_since(w[0]))
            for r in ins.writes:
                w = last_w.get(r)
                if w and w[1] in ("valu", "exp"):
                    pad = max(pad, 2 - ws_since(w[0]))
        else:
            for r in ins.reads:
                w = last_w.get(r)
                if w and w[1] == "mfma":
                    pad = max(pad, w[2] - ws_since(w[0]))
            for r in ins.writes:
                m = last_mfma.get(r)
                if m is not None:
                    pad = max(pad, 12 - ws_since(m))
                m = last_ab.get(r)
                if m is not None:
                    pad = max(pad, 2 - ws_since(m))
        while pad > 0:
            n = min(pad, 8)
            out.append(f"s_nop {n - 1}")
            pos += n
            pad -= n
            nops += 1
        # 3. issue (a raw block -- branches, stores -- counts as one wait state: its shortest path)
        out += ins.text.split("\n")
        if ins.lds:
            idx = issued
            issued += 1
            if ins.kind == "ldsr":
                for r in ins.writes:
                    pending[r] = idx
        for r in ins.writes:
            last_w[r] = (pos, "mfma" if ins.kind == "mfma" else ("ld" if ins.kind == "ldsr" else "valu"),
                         12 if ins.passes == 8 else 8)
        if ins.kind == "mfma":
            for r in ins.mfma_c + ins.writes:
                last_mfma[r] = pos
            for r in ins.reads:
                if r not in ins.mfma_c:
                    last_ab[r] = pos
        m = re.match(r"s_nop (\d+)", ins.text)
        pos += int(m.group(1)) + 1 if m else 1
    # end: the last MFMAs' results / operands are the compiler's again after the statement
    out.append("s_nop 7")
    out.append("s_nop 3")
    assert allow_pending or not pending, "LDS loads never waited for"
    return out, dict(nops=nops, waits=waits, instrs=len(out))
