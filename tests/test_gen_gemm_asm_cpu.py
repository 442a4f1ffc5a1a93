"""tools/gen_gemm_pp_asm.py: the symbolic check of the generated GEMM K-loop (barrier counts, read-after-DMA
and restage-after-read order, MFMA operands and K order) holds for every layout and K-tile count, it does
catch broken schedules, and the committed generated files are what their generators write."""
import importlib.util
import os
import subprocess
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "owl-audio-exps_amd", "csrc")


@pytest.fixture(scope="module")
def gen():
    spec = importlib.util.spec_from_file_location("gen_gemm_pp_asm", os.path.join(REPO, "tools", "gen_gemm_pp_asm.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


@pytest.mark.parametrize("at,bt", [(False, False), (False, True), (True, False), (True, True)])
def test_symbolic_check_every_layout_and_residue(gen, at, bt):
    """1 .. 13 K-tiles: 1, 2, 3 tiles, then every residue of the five-tile ring period entered and left
    twice; both wave groups and both B halves inside check().  Eight barriers per K-tile plus the
    prologue's and the stagger's."""
    bars = gen.check_all(at, bt)
    assert sorted(bars) == list(range(1, 14))
    assert all(bars[nk] == 8 * nk + 2 for nk in bars)


def _mutations():
    def vmcnt_late(p):  # the K-tile wait lets one more half-tile stay in flight
        for i in p:
            if i.op == "vmcnt" and i.n == 6:
                i.n = 8

    def barrier_lost(p):
        del p[[n for n, i in enumerate(p) if i.op == "bar"][40]]

    def wrong_slot(p):
        next(i for i in p if i.op == "dma").slot += 2

    def address_step(p):
        next(i for i in p if i.op == "vadd").delta += 16384

    def lgkm_lost(p):
        del p[[n for n, i in enumerate(p) if i.op == "lgkmcnt" and i.n == 0][3]]

    def operand_swapped(p):
        ms = [i for i in p if i.op == "mfma"]
        ms[4].b, ms[5].b = ms[5].b, ms[4].b

    def restage_early(p):  # a steady-state DMA pair moved one phase (two barriers) up
        d = [n for n, i in enumerate(p) if i.op == "dma"][20]
        pair = [p.pop(d), p.pop(d)]
        b = [n for n, i in enumerate(p) if i.op == "bar" and n < d][-2]
        p[b:b] = pair

    def pad_lost(p):
        del p[next(n for n, i in enumerate(p) if i.op == "nop" and n > 100)]

    return [vmcnt_late, barrier_lost, wrong_slot, address_step, lgkm_lost, operand_swapped, restage_early, pad_lost]


@pytest.mark.parametrize("mutate", _mutations(), ids=lambda f: f.__name__)
def test_check_catches_broken_schedules(gen, mutate):
    prog = gen.program(False, True)
    mutate(prog)
    with pytest.raises(gen.CheckError):
        gen.check_all(False, True, prog)


@pytest.mark.parametrize("tool,inc", [("gen_gemm_pp_asm.py", "gemm_pp_step.inc"),
                                      ("gen_fused4_asm.py", "attn_bwd_fused4_step.inc"),
                                      ("gen_fwd4_asm.py", "attn_fwd4_step.inc")])
def test_committed_inc_regenerates_byte_identically(tmp_path, tool, inc):
    out = tmp_path / inc
    env = {k: v for k, v in os.environ.items() if not k.startswith(("F4_", "W4F_", "PPA_"))}  # no schedule knobs
    subprocess.run([sys.executable, os.path.join(REPO, "tools", tool), "--out", str(out)], check=True, env=env,
                   capture_output=True)
    assert out.read_bytes() == open(os.path.join(CSRC, inc), "rb").read()
