#!/usr/bin/env python3
"""Generate the hand-placed K-loop of the 256 x 256 ping-pong bf16 GEMM (gemm.hip `gemm_pp_kernel<.., ASM>`).

    python tools/gen_gemm_pp_asm.py            # checks, then writes owl-audio-exps_amd/csrc/gemm_pp_step.inc
    python tools/gen_gemm_pp_asm.py --out F    # ... to F
    python tools/gen_gemm_pp_asm.py --stats    # checks and prints the per-layout statistics only

The loop keeps gemm_pp_kernel's tile, waves, LDS images and phases: 8 waves in two groups (wr = 0 / 1:
rows 0-127 / 128-255 of the tile) one barrier apart, four phases per K-tile of 64, one 16-MFMA quadrant
per phase, every accumulator fed in the same K order.  What changes is where everything else sits:

* the ring is ten 16-KiB half-tile slots (160 KiB) filled first-in first-out in the order B cols 0-127,
  B cols 128-255, A rows 0-127, A rows 128-255 of each K-tile (B is read last in phase 1, A in phase 2,
  so B's slots free first).  Half-tile h (= 4 tile + that order) sits in slot 2 ((h / 2) % 5) + h % 2;
  the ring period is five K-tiles, so the loop is five tile bodies long;
* every phase stages exactly one half-tile (two LDS-DMA pieces per wave): global phase P stages
  half-tile P + LEAD (LEAD = 7), i.e. a half-tile is in flight for 4-7 phases before its first read
  (gemm_pp_kernel: 4-5) and no phase carries more than two pieces;
* one counted wait per K-tile, `s_waitcnt vmcnt(6)` in phase 3: everything but the three youngest
  half-tiles has landed, which is all of the next K-tile; the reads of a phase are counted too
  (`lgkmcnt(n)` lets the k-substep 0 MFMAs start while the k-substep 1 fragments are still coming);
* addresses are an SGPR base (advanced once per K-tile) plus a 32-bit lane offset; the LDS read
  addresses are lane VGPRs moved from slot to slot by one `v_add_u32` per K-tile in an MFMA shadow.

Registers are fixed: accumulators v[0:127] (acc[i][j] = v[16 i + 4 j ..], compiler-visible as eight
16-float operands), fragments v[128:191], DMA lane offsets v[192:199], read addresses v[200:211];
s[64:65] / s[66:67] the A / B tile bases, s68 the K-tiles left, s[72:75] = A step, B step, the wave's
LDS-DMA base (M0), wr.

Before anything is written the generator executes prologue -> loop -> drain symbolically (`check_all`)
for every layout, 1 .. 13 K-tiles (every residue of the ring period entered and left, plus 1-3 tiles)
and both wave groups, and asserts
  1. the two groups pass the same number of barriers;
  2. every LDS read of a slot follows, in barrier order, the counted vmcnt of BOTH groups that retired
     the slot's DMA (wait before barrier n, read after barrier n: the one-phase rule);
  3. every restage of a slot follows the barrier after the lgkmcnt that retired the slot's last read;
  4. every MFMA operand register holds the fragment it should (retired by an lgkmcnt before the MFMA),
     each accumulator receives K-tile 0 substep 0, 1, K-tile 1 substep 0, ... in order, and no LDS
     read overwrites a fragment register less than 12 wait states after an MFMA that reads it.
"""
import argparse
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(REPO, "owl-audio-exps_amd", "csrc", "gemm_pp_step.inc")

HALF = 16384
NPAIR = 5  # ring: five 32-KiB slot pairs
LEAD = int(os.environ.get("PPA_LEAD", 7))  # global phase P stages half-tile P + LEAD
MF = "v_mfma_f32_16x16x32_bf16"
WAR_WS = 12  # MFMA operand read -> LDS-load write of that register, wait states (margin)

# fixed registers
V_DMA, V_RA, V_RB = 192, 200, 208
S_AB, S_BB, S_REM, S_ASTEP, S_BSTEP, S_M0B, S_WR = 64, 66, 68, 72, 73, 74, 75
KINDS = ("B0", "B1", "A0", "A1")  # FIFO order of a K-tile's half-tiles; also the order of the DMA lane offsets


def ACC(i, j):
    return 16 * i + 4 * j


def AF(i, kk):
    return 128 + 8 * i + 4 * kk


def BF(s, j, kk):  # s = 0: columns half n0 of the wave (phases 0, 3), 1: n1 (phases 1, 2)
    return 160 + 16 * s + 8 * j + 4 * kk


def slot_of(h):
    return 2 * ((h // 2) % NPAIR) + h % 2


def rng(lo, n):
    return f"v[{lo}:{lo + n - 1}]"


class Ins:
    """One instruction (or label).  `text` is formatted from the same fields the checker executes."""

    def __init__(self, op, **kw):
        self.op = op
        self.seg = None
        self.__dict__.update(kw)

    def lines(self):
        o = self.op
        if o == "label":
            return [f".Lpp_{self.name}%=:"]
        if o == "bar":
            return ["s_barrier"]
        if o == "vmcnt":
            return [f"s_waitcnt vmcnt({self.n})"]
        if o == "lgkmcnt":
            return [f"s_waitcnt lgkmcnt({self.n})"]
        if o == "dma":  # piece i of half-tile kind k into ring slot `slot`
            base = S_AB if KINDS[self.k][0] == "A" else S_BB
            return [f"s_add_u32 m0, s{S_M0B}, {self.slot * HALF + self.i * 1024}", "s_nop 0",
                    f"global_load_lds_dwordx4 v{V_DMA + 2 * self.k + self.i}, s[{base}:{base + 1}]"]
        if o == "sadd":  # the A / B tile base one K-tile on
            b, st = (S_AB, S_ASTEP) if self.opnd == "A" else (S_BB, S_BSTEP)
            return [f"s_add_u32 s{b}, s{b}, s{st}", f"s_addc_u32 s{b + 1}, s{b + 1}, 0"]
        if o == "read":
            ins = "ds_read_b128" if self.n == 4 else "ds_read_b64_tr_b16"
            return [f"{ins} {rng(self.dst, self.n)}, v{self.vreg} offset:{self.imm}"]
        if o == "vadd":
            return [f"v_add_u32 v{self.vreg}, 0x{self.delta & 0xffffffff:x}, v{self.vreg}"]
        if o == "mfma":
            return [f"{MF} {rng(self.c, 4)}, {rng(self.a, 4)}, {rng(self.b, 4)}, {rng(self.c, 4)}"]
        if o == "prio":
            return [f"s_setprio {self.n}"]
        if o == "nop":
            return [f"s_nop {self.n - 1}"]
        if o == "cmp_lt":  # scc = s[reg] < imm
            return [f"s_cmp_lt_u32 s{self.reg}, {self.imm}"]
        if o == "cmp_eq":
            return [f"s_cmp_eq_u32 s{self.reg}, {self.imm}"]
        if o == "br":  # cond: None (always), 0 / 1 (scc)
            ins = "s_branch" if self.cond is None else f"s_cbranch_scc{self.cond}"
            return [f"{ins} .Lpp_{self.target}%="]
        if o == "dec":
            return [f"s_sub_u32 s{S_REM}, s{S_REM}, 1"]
        raise ValueError(o)


# ---------------------------------------------------------------- the schedule
def seg(key, instrs):
    """Tag a run of instructions that recurs with the same text: the emitter writes it once, as a macro."""
    for ins in instrs:
        ins.seg = key
    return instrs


def dma_half(h):
    return seg(f"D{KINDS[h % 4]}_S{slot_of(h)}", [Ins("dma", k=h % 4, i=i, slot=slot_of(h)) for i in range(2)])


def reads(opnd, trans, half, s=0):
    """The wave's fragment reads of one operand half (A: rows 64 half .. + 63 of its 128; B: columns
    32 half .. + 31 of its 64), as [kk] -> list of Ins.  Row offsets are immediates for k-contiguous
    operands; transposed operands have one lane address per 16-row block (the XOR swizzle)."""
    out = [[], []]
    n = 4 if opnd == "A" else 2
    vbase = V_RA if opnd == "A" else V_RB
    for kk in range(2):
        for x in range(n):
            dst = AF(x, kk) if opnd == "A" else BF(s, x, kk)
            blk = n * half + x
            if not trans:
                out[kk].append(Ins("read", opnd=opnd, trans=False, n=4, dst=dst, vreg=vbase + kk, imm=16 * blk * 128))
            else:
                for part in range(2):
                    out[kk].append(Ins("read", opnd=opnd, trans=True, n=2, dst=dst + 2 * part, vreg=vbase + blk,
                                       imm=kk * 8192 + part * 1024))
    return out


def quad(mh, nh, kk):
    s = 0 if nh == 0 else 1
    return [Ins("mfma", c=ACC(4 * mh + i, 2 * nh + j), a=AF(i, kk), b=BF(s, j, kk)) for i in range(4) for j in range(2)]


def tile_body(r, kind, AT, BT):
    """K-tile t = r (mod 5).  kind: 'steady' (t <= nk - 3), 'penult' (t = nk - 2), 'last'."""
    o = []
    QUADS = ((0, 0), (0, 1), (1, 1), (1, 0))
    for p in range(4):
        rd = [[], []]
        if p == 0:
            b, a = reads("B", BT, 0, 0), reads("A", AT, 0)
            rd = [b[0] + a[0], b[1] + a[1]]
        elif p == 1:
            rd = reads("B", BT, 1, 1)
        elif p == 2:
            rd = reads("A", AT, 1)
        o += seg(f"R{p}", rd[0] + rd[1])
        # one half-tile per phase: P + LEAD, where it exists
        h = 4 * r + p + LEAD  # (mod 20: only the slot and the kind matter)
        stage = kind == "steady" or (kind == "penult" and p + LEAD < 8)
        if stage:
            if h % 4 == 2:  # A rows 0-127 of a new K-tile
                o.append(Ins("sadd", opnd="A"))
            o += dma_half(h)
            if h % 4 == 1:  # B cols 128-255: the tile's B is complete
                o.append(Ins("sadd", opnd="B"))
        if p == 3 and kind != "last":
            o.append(Ins("vmcnt", n=6 if kind == "steady" else 0))
        mh, nh = QUADS[p]
        q0, q1 = quad(mh, nh, 0), quad(mh, nh, 1)
        o += seg(f"M{p}A", [Ins("bar")] + ([Ins("lgkmcnt", n=min(len(rd[1]), 15))] if rd[0] or rd[1] else []) +
                 [Ins("prio", n=1)] + q0[:2])
        if kind != "last" and p in (2, 3):
            # the B (phase 2) / A (phase 3) read addresses move to the next K-tile's slot pair
            pair = (2 * r + (1 if p == 3 else 0)) % NPAIR
            delta = ((pair + 2) % NPAIR - pair) * 2 * HALF
            nv = (8 if AT else 2) if p == 3 else (4 if BT else 2)
            o += seg(f"V{'A' if p == 3 else 'B'}_{'P' if delta > 0 else 'M'}{abs(delta) // HALF}",
                     [Ins("vadd", vreg=(V_RA if p == 3 else V_RB) + x, delta=delta) for x in range(nv)])
        o += seg(f"M{p}B", q0[2:] + ([Ins("lgkmcnt", n=0)] if rd[1] else []) + q1 + [Ins("prio", n=0), Ins("bar")])
    return o


def program(AT, BT):
    o = []
    # prologue: half-tiles 0 .. LEAD - 1 (K-tile 0 only when there is no second one)
    assert LEAD == 7
    o += dma_half(0) + dma_half(1) + [Ins("sadd", opnd="B")] + dma_half(2) + dma_half(3) + [Ins("sadd", opnd="A")]
    o += [Ins("cmp_lt", reg=S_REM, imm=2), Ins("br", cond=1, target="p1")]
    o += dma_half(4) + dma_half(5) + [Ins("sadd", opnd="B")] + dma_half(6)
    o += [Ins("vmcnt", n=6), Ins("br", cond=None, target="p2"), Ins("label", name="p1"), Ins("vmcnt", n=0),
          Ins("label", name="p2"), Ins("bar")]
    # group 1 runs one barrier behind group 0
    o += [Ins("cmp_eq", reg=S_WR, imm=1), Ins("br", cond=0, target="g0"), Ins("bar"), Ins("label", name="g0")]
    for r in range(NPAIR):
        o += [Ins("label", name=f"r{r}"), Ins("cmp_lt", reg=S_REM, imm=3), Ins("br", cond=1, target=f"t{r}")]
        o += tile_body(r, "steady", AT, BT) + [Ins("dec")]
    o.append(Ins("br", cond=None, target="r0"))
    for r in range(NPAIR):
        o += [Ins("label", name=f"t{r}"), Ins("cmp_lt", reg=S_REM, imm=2), Ins("br", cond=1, target=f"l{r}")]
        o += tile_body(r, "penult", AT, BT) + [Ins("br", cond=None, target=f"l{(r + 1) % NPAIR}")]
    for r in range(NPAIR):
        o += [Ins("label", name=f"l{r}")] + tile_body(r, "last", AT, BT) + [Ins("br", cond=None, target="end")]
    # group 0's last barrier pairs with group 1's: every MFMA and LDS read of the block is done
    o += [Ins("label", name="end"), Ins("cmp_eq", reg=S_WR, imm=0), Ins("br", cond=0, target="g1"), Ins("bar"),
          Ins("label", name="g1"), Ins("nop", n=8), Ins("nop", n=8)]  # MFMA results -> the compiler's reads
    return pad_war(o)


def pad_war(prog):
    """s_nop before an LDS read that would overwrite a fragment register within WAR_WS wait states of an
    MFMA reading it.  Straight-line distance; every branch target starts with reads only after a barrier
    of the previous body, which `check` re-verifies on the executed path."""
    out = []
    last_use = {}  # reg -> wait-state clock of the last MFMA reading it
    clock = 0
    for ins in prog:
        if ins.op == "read":
            need = max((last_use.get(ins.dst + e, -10 ** 9) + WAR_WS - clock for e in range(ins.n)), default=0)
            while need > 0:
                n = min(need, 8)
                out.append(Ins("nop", n=n))
                out[-1].seg = ins.seg
                clock += n
                need -= n
        if ins.op == "mfma":
            for e in range(4):
                last_use[ins.a + e] = clock
                last_use[ins.b + e] = clock
        clock += ins.n if ins.op == "nop" else (0 if ins.op == "label" else len(ins.lines()))
        out.append(ins)
    return out


# ---------------------------------------------------------------- symbolic execution
class CheckError(AssertionError):
    pass


def req(c, msg):
    if not c:
        raise CheckError(msg)


def execute(prog, nk, wr, AT, BT):
    """Run one wave of group wr over nk K-tiles.  Returns (barriers passed, dma events, read events,
    mfma events); the B column half of the wave does not change the program (it is a lane offset)."""
    labels = {ins.name: n for n, ins in enumerate(prog) if ins.op == "label"}
    pc, scc, rem, count, clock = 0, 0, nk, 0, 0
    base = {"A": 0, "B": 0}  # K-tile the SGPR bases point at
    vaddr = {V_RA + x: 2 * HALF for x in range(8)}  # K-tile 0: B in pair 0, A in pair 1
    vaddr.update({V_RB + x: 0 for x in range(4)})
    vm, lg = [], []  # outstanding LDS-DMA pieces / LDS reads (in order)
    dmas, rds, mfmas = [], [], []
    regs = {}  # fragment register -> (read event, word)
    last_use = {}
    steps = 0
    while pc < len(prog):
        ins = prog[pc]
        pc += 1
        steps += 1
        req(steps < 10 ** 6, "runaway program")
        o = ins.op
        if o == "label":
            continue
        if o == "bar":
            count += 1
        elif o == "vmcnt":
            while len(vm) > ins.n:
                vm.pop(0)["retired"] = count
        elif o == "lgkmcnt":
            while len(lg) > ins.n:
                lg.pop(0)["retired"] = count
        elif o == "dma":
            kind = KINDS[ins.k]
            ev = dict(count=count, slot=ins.slot, i=ins.i, opnd=kind[0], half=int(kind[1]), tile=base[kind[0]],
                      retired=None, seq=len(dmas))
            req(ev["tile"] < nk, f"nk={nk} wr={wr}: DMA of K-tile {ev['tile']} (out of range)")
            req(0 <= ins.slot < 2 * NPAIR, "DMA slot out of the ring")
            dmas.append(ev)
            vm.append(ev)
        elif o == "sadd":
            base[ins.opnd] += 1
        elif o == "read":
            for e in range(ins.n):
                gap = clock - last_use.get(ins.dst + e, -10 ** 9)
                req(gap >= WAR_WS, f"nk={nk} wr={wr}: LDS read overwrites v{ins.dst + e} {gap} wait states after its MFMA")
            ev = dict(count=count, ins=ins, addr=vaddr[ins.vreg] + ins.imm, retired=None, after_dma=len(dmas), seq=len(rds))
            rds.append(ev)
            lg.append(ev)
            for e in range(ins.n):
                regs[ins.dst + e] = (ev, e)
        elif o == "vadd":
            vaddr[ins.vreg] = (vaddr[ins.vreg] + ins.delta) & 0xffffffff
            if vaddr[ins.vreg] >= 1 << 31:
                vaddr[ins.vreg] -= 1 << 32
        elif o == "mfma":
            for e in range(4):
                last_use[ins.a + e] = clock
                last_use[ins.b + e] = clock
            mfmas.append(dict(ins=ins, a=[regs.get(ins.a + e) for e in range(4)], b=[regs.get(ins.b + e) for e in range(4)],
                              lg_out=[id(x) for x in lg]))
        elif o == "cmp_lt":
            scc = int((rem if ins.reg == S_REM else wr) < ins.imm)
        elif o == "cmp_eq":
            scc = int((rem if ins.reg == S_REM else wr) == ins.imm)
        elif o == "br":
            if ins.cond is None or ins.cond == scc:
                pc = labels[ins.target]
        elif o == "dec":
            rem -= 1
        elif o in ("prio", "nop"):
            pass
        else:
            raise ValueError(o)
        clock += ins.n if o == "nop" else len(ins.lines())
    req(not vm, f"nk={nk} wr={wr}: {len(vm)} LDS-DMA pieces never waited for")
    req(not lg, f"nk={nk} wr={wr}: LDS reads never waited for")
    return count, dmas, rds, mfmas


def decode_read(ev, wr, bh, AT, BT):
    """(slot, 16-row block, kk, first word) a read fetches for a wave of group wr, B column half bh."""
    ins = ev["ins"]
    addr = ev["addr"] + (wr if ins.opnd == "A" else bh) * HALF
    req(0 <= addr < 2 * NPAIR * HALF, f"LDS read at {addr}: outside the ring")
    slot, inner = divmod(addr, HALF)
    trans = AT if ins.opnd == "A" else BT
    req(trans == ins.trans, "read form does not match the layout")
    if not trans:
        req(inner % (16 * 128) == 0, "row offset is not a 16-row block")
        return slot, inner // (16 * 128), ins.vreg - (V_RA if ins.opnd == "A" else V_RB), 0
    req(inner % 1024 == 0 and inner % 8192 in (0, 1024), "transposed read offset")
    return slot, ins.vreg - (V_RA if ins.opnd == "A" else V_RB), inner // 8192, 2 * ((inner % 8192) // 1024)


def check(prog, nk, AT, BT):
    runs = {wr: execute(prog, nk, wr, AT, BT) for wr in (0, 1)}
    # 1. barrier counts
    req(runs[0][0] == runs[1][0], f"nk={nk}: barrier counts differ: {runs[0][0]} vs {runs[1][0]}")
    # both groups issue the same DMA sequence (every wave stages 1/8 of every half-tile)
    sig = [[(d["slot"], d["i"], d["opnd"], d["half"], d["tile"]) for d in runs[wr][1]] for wr in (0, 1)]
    req(sig[0] == sig[1], f"nk={nk}: the groups stage different pieces")
    for d0, d1 in zip(sig[0][0::2], sig[0][1::2]):
        req(d0[0] == d1[0] and d0[2:] == d1[2:] and (d0[1], d1[1]) == (0, 1), "half-tile pieces are not paired")
    for wr in (0, 1):
        _, dmas, rds, mfmas = runs[wr]
        other = runs[1 - wr][1]
        for bh in (0, 1):
            what = {}
            for ev in rds:
                slot, blk, kk, w0 = decode_read(ev, wr, bh, AT, BT)
                opnd = ev["ins"].opnd
                # the half-tile the slot holds in program order of this wave
                mine = [d for d in dmas[:ev["after_dma"]] if d["slot"] == slot]
                req(mine, f"nk={nk} wr={wr}: read of slot {slot} before any DMA")
                x = mine[-1]
                req(x["opnd"] == opnd and x["half"] == (wr if opnd == "A" else bh),
                    f"nk={nk} wr={wr} bh={bh}: {opnd} read hits the slot of {x['opnd']}{x['half']}")
                # 2. RAW: both groups' waits for both pieces, one barrier before the read
                for grp in (dmas, other):
                    for i in (0, 1):
                        d = grp[x["seq"] - x["i"] + i]
                        req(d["retired"] is not None and ev["count"] >= d["retired"] + 1,
                            f"nk={nk} wr={wr}: read of slot {slot} (K-tile {x['tile']}) at barrier {ev['count']}, "
                            f"DMA waited for at {d['retired']}")
                # 3. WAR: the next DMA into the slot, by either group
                for grp in (dmas, other):
                    nxt = [d for d in grp[x["seq"] - x["i"] + 2:] if d["slot"] == slot]
                    if nxt:
                        req(ev["retired"] is not None and nxt[0]["count"] >= ev["retired"] + 1,
                            f"nk={nk} wr={wr}: slot {slot} restaged at barrier {nxt[0]['count']}, its read retired at {ev['retired']}")
                what[ev["seq"]] = (opnd, x["tile"], blk, kk, w0)
            # 4. MFMA operands and the K order of every accumulator
            seen = {}
            for m in mfmas:
                ins = m["ins"]
                I, J = ins.c // 16, (ins.c % 16) // 4
                req(ins.c % 4 == 0 and ins.c < 128, "accumulator register")
                frag = []
                for name, srcs, blk in (("A", m["a"], I), ("B", m["b"], J)):
                    req(all(s is not None for s in srcs), f"nk={nk}: MFMA reads an unwritten {name} fragment")
                    got = []
                    for e, (ev, w) in enumerate(srcs):
                        req(id(ev) not in m["lg_out"], f"nk={nk} wr={wr}: MFMA reads v{(ins.a if name == 'A' else ins.b) + e} before its lgkmcnt")
                        opnd, tile, rblk, kk, w0 = what[ev["seq"]]
                        req(opnd == name and rblk == blk and w0 + w == e,
                            f"nk={nk} wr={wr}: MFMA acc[{I}][{J}] {name} operand holds {opnd} block {rblk} word {w0 + w}")
                        got.append((tile, kk))
                    req(len(set(got)) == 1, "fragment words of different reads")
                    frag.append(got[0])
                req(frag[0] == frag[1], f"nk={nk}: A and B fragments of different K positions {frag}")
                n = seen.get(ins.c, 0)
                req(frag[0] == (n // 2, n % 2), f"nk={nk} wr={wr}: acc[{I}][{J}] product {n} is K-tile/substep {frag[0]}")
                seen[ins.c] = n + 1
            req(len(seen) == 32 and all(v == 2 * nk for v in seen.values()), f"nk={nk}: accumulators miss products")
    return runs[0][0]


def check_all(AT, BT, prog=None, nks=range(1, 14)):
    prog = prog or program(AT, BT)
    return {nk: check(prog, nk, AT, BT) for nk in nks}


# ---------------------------------------------------------------- emission
def stats(prog):
    n = {}
    for ins in prog:
        n[ins.op] = n.get(ins.op, 0) + 1
    return {"lines": sum(len(i.lines()) for i in prog), "mfma": n.get("mfma", 0), "read": n.get("read", 0),
            "dma": n.get("dma", 0), "nop": n.get("nop", 0), "barrier": n.get("bar", 0)}


def pack(tokens, indent, width=118, cont=""):
    """Tokens joined by spaces into lines of at most `width` characters."""
    lines, cur = [], ""
    for t in tokens:
        if cur and len(indent) + len(cur) + 1 + len(t) + len(cont) > width:
            lines.append(indent + cur + cont)
            cur = ""
        cur = f"{cur} {t}" if cur else t
    if cur:
        lines.append(indent + cur)
    return lines


def emit(AT, BT, prog, macros):
    """The statement of one layout.  A tagged run (seg) becomes a use of a string-literal macro, defined once per
    distinct text in `macros` (name -> lines; a run whose text differs from an earlier one of its tag gets a
    numbered name); the expansion is the flat instruction list the checks ran on."""
    tokens, n = [], 0
    while n < len(prog):
        ins = prog[n]
        if ins.seg is None:
            if ins.op in ("label", "br") and tokens and tokens[-1] != "\n":
                tokens.append("\n")
            tokens += [f'"{l}\\n"' for l in ins.lines()]
            if ins.op == "br":
                tokens.append("\n")
            n += 1
            continue
        m = n
        while m < len(prog) and prog[m].seg == ins.seg:
            m += 1
        text = tuple(l for i in prog[n:m] for l in i.lines())
        name, k = f"PPA_{ins.seg}", 1
        while macros.get(name, text) != text:
            k += 1
            name = f"PPA_{ins.seg}_{k}"
        macros[name] = text
        tokens.append(name)
        n = m
    rows, cur = [], []
    for t in tokens + ["\n"]:
        if t == "\n":
            rows += pack(cur, "      ")
            cur = []
        else:
            cur.append(t)
    body = "\n".join(rows)
    clob = ['"memory"', '"m0"', '"scc"'] + [f'"v{i}"' for i in range(128, 192)]
    acc = ", ".join(f'"+{{v[{16 * i}:{16 * i + 15}]}}"(c[{i}])' for i in range(8))
    return f"""template <>
__attribute__((always_inline)) DEV void gemm_pp_loop<{str(AT).lower()}, {str(BT).lower()}>(f32x16 (&c)[8], PPLane& f, const void* ab, const void* bb,
                                                                  unsigned nk, u32x4 sc) {{
  asm volatile(
{body}
      : {acc},
        "+{{v[{V_RA}:{V_RA + 7}]}}"(f.ra), "+{{v[{V_RB}:{V_RB + 3}]}}"(f.rb), "+{{s[{S_AB}:{S_AB + 1}]}}"(ab), "+{{s[{S_BB}:{S_BB + 1}]}}"(bb), "+{{s{S_REM}}}"(nk)
      : "{{v[{V_DMA}:{V_DMA + 7}]}}"(f.dma), "{{s[{S_ASTEP}:{S_ASTEP + 3}]}}"(sc)
      : {", ".join(clob)});
}}
"""


HDR = """// GENERATED by tools/gen_gemm_pp_asm.py -- do not edit.  The hand-placed K-loop of
// gemm_pp_kernel<.., ASM = true> (gemm.hip): see the generator's docstring for the schedule and for
// what its symbolic check proves about every path through this code.
#pragma once

typedef unsigned int u32x8 __attribute__((ext_vector_type(8)));
constexpr int PPA_LDS_BYTES = %d;  // the ring: ten 16-KiB half-tile slots
constexpr int PPA_A_PAIR0 = %d;     // K-tile 0: B halves in slots 0 / 1, A halves at this byte offset

// per-lane operands: the LDS-DMA source offsets of the wave's two pieces of the half-tiles B cols 0-127,
// B cols 128-255, A rows 0-127, A rows 128-255 (bytes from the tile base of the K-tile); the LDS byte
// addresses of the fragment reads at K-tile 0 (k-contiguous operands: [k-substep]; transposed: [16-row block])
struct PPLane {
  u32x8 dma, ra;
  u32x4 rb;
};

// c: acc[i][j] = c[i][4 j ..]; ab / bb: the tile's first K-tile of A / B; nk >= 1 K-tiles of 64;
// sc = {bytes per K-tile of A, of B, LDS-DMA base of the wave (ring + 2048 wave), wave group}
template <bool AT, bool BT>
__attribute__((always_inline)) DEV void gemm_pp_loop(f32x16 (&c)[8], PPLane& f, const void* ab, const void* bb,
                                                     unsigned nk, u32x4 sc);
""" % (2 * NPAIR * HALF, 2 * HALF)


def generate():
    parts, st, macros = [], {}, {}
    for AT in (False, True):
        for BT in (False, True):
            prog = program(AT, BT)
            bars = check_all(AT, BT, prog)
            st[(AT, BT)] = dict(stats(prog), barriers_at=bars)
            parts.append(f"// layout (AT, BT) = ({int(AT)}, {int(BT)}): {st[(AT, BT)]['lines']} instructions\n" +
                         emit(AT, BT, prog, macros))
    defs = ["// recurring runs of the statements below: D<half-tile>_S<slot> two LDS-DMA pieces (with the tile base's step),",
            "// R<phase> the fragment reads of a phase, M<phase>A / M<phase>B barrier, waits and the quadrant's MFMAs around the",
            "// V<operand>_<step> read-address moves (P / M: plus / minus that many half-tile slots)"]
    for name, text in macros.items():
        defs += [f"#define {name} \\"] + pack([f'"{l}\\n"' for l in text], "  ", cont=" \\")
    return "\n".join([HDR, "\n".join(defs) + "\n"] + parts), st


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--stats", action="store_true")
    ap.add_argument("--out", default=OUT)
    args = ap.parse_args()
    text, st = generate()
    for k, v in st.items():
        print(f"layout {int(k[0])}{int(k[1])}: {v}", file=sys.stderr)
    if args.stats:
        return
    with open(args.out, "w") as f:
        f.write(text)
    print("wrote", args.out, file=sys.stderr)


if __name__ == "__main__":
    main()
