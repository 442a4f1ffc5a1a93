"""tools/asmgen.py, the core of the attention asm generators: finalize's lgkmcnt waits and MFMA hazard
padding on tiny programs, the forward generator's symbolic schedule check (it passes, and it catches
broken schedules), and both generators ignoring the environment."""
import importlib.util
import os
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOLS = os.path.join(REPO, "tools")
CSRC = os.path.join(REPO, "owl-audio-exps_amd", "csrc")
END = ["s_nop 7", "s_nop 3"]  # finalize closes every statement with these


def _load(name):
    path = list(sys.path)
    sys.path.insert(0, TOOLS)
    try:
        spec = importlib.util.spec_from_file_location(name, os.path.join(TOOLS, name + ".py"))
        m = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(m)
    finally:
        sys.path[:] = path  # (the generators put their directory in front themselves)
    return m


@pytest.fixture(scope="module")
def ag():
    return _load("asmgen")


@pytest.fixture(scope="module")
def fwd():
    return _load("gen_fwd4_asm")


def _ld(ag, lo, n=4):
    return ag.Ins(f"ds_read_b128 {ag.rng('v', lo, n)}, v1", "ldsr", writes=ag.vr(lo, n), lds=True)


def _valu_r(ag, r):
    return ag.Ins(f"v_mov_b32 v2, v{r}", "valu", reads=ag.vr(r, 1), writes=ag.vr(2, 1))


def _valu_w(ag, r):
    return ag.Ins(f"v_mov_b32 v{r}, 0", "valu", writes=ag.vr(r, 1))


def _mfma(ag, d, a, b=8, chain=False, passes=4):
    c = ag.vr(d, 4) if chain else []
    return ag.Ins(f"mfma v{d} v{a} v{b}", "mfma", reads=ag.vr(a, 4) + ag.vr(b, 4) + c, writes=ag.vr(d, 4), mfma_c=c,
                  passes=passes)


def test_waits_count_lds_ops_in_flight(ag):
    p = [_ld(ag, 100), _ld(ag, 104), _valu_r(ag, 100), _valu_r(ag, 104)]
    out, st = ag.finalize(p)
    assert out == [p[0].text, p[1].text, "s_waitcnt lgkmcnt(1)", p[2].text, "s_waitcnt lgkmcnt(0)", p[3].text] + END
    assert st["waits"] == 2


def test_wait_count_clamped_to_four_bits(ag):
    p = [_ld(ag, 100 + 4 * i) for i in range(17)] + [_valu_r(ag, 100)]
    out, _ = ag.finalize(p, allow_pending=True)
    assert out == [x.text for x in p[:17]] + ["s_waitcnt lgkmcnt(15)", p[17].text] + END


def test_valu_write_then_mfma_read(ag):
    p = [_valu_w(ag, 100), _mfma(ag, 120, 100)]
    assert ag.finalize(p)[0] == [p[0].text, "s_nop 1", p[1].text] + END


@pytest.mark.parametrize("passes,pad", [(4, ["s_nop 7"]), (8, ["s_nop 7", "s_nop 3"])], ids=["16x16x32", "32x32x16"])
def test_mfma_write_then_valu_read(ag, passes, pad):
    p = [_mfma(ag, 120, 100, passes=passes), _valu_r(ag, 120)]
    assert ag.finalize(p)[0] == [p[0].text] + pad + [p[1].text] + END


def test_mfma_operand_read_then_valu_write(ag):
    p = [_mfma(ag, 120, 100), _valu_w(ag, 100)]
    assert ag.finalize(p)[0] == [p[0].text, "s_nop 1", p[1].text] + END


def test_mfma_write_then_lds_load_into_it(ag):
    p = [_mfma(ag, 120, 100), _ld(ag, 120)]
    assert ag.finalize(p, allow_pending=True)[0] == [p[0].text, "s_nop 7", "s_nop 3", p[1].text] + END


def test_accumulate_chain_needs_no_padding(ag):
    p = [_mfma(ag, 120, 100), _mfma(ag, 120, 104, chain=True)]
    out, st = ag.finalize(p)
    assert out == [p[0].text, p[1].text] + END and st["nops"] == 0


def test_unwaited_lds_load_is_an_error(ag):
    with pytest.raises(AssertionError):
        ag.finalize([_ld(ag, 100)])
    ag.finalize([_ld(ag, 100)], allow_pending=True)


# ---------------------------------------------------------------- the forward generator's schedule check
def test_fwd4_self_check_passes(fwd):
    fwd.self_check()


def _meta(x):
    return getattr(x, "meta", None) or (None,)


def _kfrag_early(fwd):  # part 1's K fragment (kk 0, kd 0) re-read before part 0's S MFMAs consumed it
    p = fwd.build_tile(0, False)
    x = p.pop(next(n for n, i in enumerate(p) if _meta(i) == ("LK", 0, 0, (0, 1))))
    p.insert(next(n for n, i in enumerate(p) if _meta(i)[0] == "S"), x)
    return [p]


def _exp_lost(fwd):
    p = fwd.build_tile(1, True)
    del p[next(n for n, i in enumerate(p) if _meta(i)[0] == "E")]
    return [p]


def _vfrag_early(fwd):  # the next tile's V^T fragment loaded while V(t, 0) still reads those registers
    pro, bodies, drains = fwd.run_parts(0)
    b = list(bodies[0])
    x = b.pop(next(n for n, i in enumerate(b) if _meta(i)[0] == "LV" and _meta(i)[4] == (1, 0)))
    b.insert(0, x)
    return [pro, b, drains[1]]


def _kd_swapped(fwd):  # an S^T chain started by its second k-step
    p = fwd.build_tile(2, False)
    n0, n1 = (next(n for n, i in enumerate(p) if _meta(i)[:5] == ("S", "X", 0, kd, 3)) for kd in (0, 1))
    p[n0], p[n1] = p[n1], p[n0]
    return [p]


@pytest.mark.parametrize("mutated", [_kfrag_early, _exp_lost, _vfrag_early, _kd_swapped], ids=lambda f: f.__name__[1:])
def test_fwd4_check_catches_broken_schedules(fwd, mutated):
    st = None
    with pytest.raises(AssertionError):
        for prog in mutated(fwd):
            st = fwd.check_program(prog, st)


# ---------------------------------------------------------------- no environment
@pytest.mark.parametrize("tool,inc", [("gen_fused4_asm", "attn_bwd_fused4_step.inc"), ("gen_fwd4_asm", "attn_fwd4_step.inc")])
def test_generators_ignore_the_environment(tmp_path, monkeypatch, tool, inc):
    for k in ("F4_CHECK=64", "F4_XEXP=1", "W4F_XEXP=1"):
        monkeypatch.setenv(*k.split("="))
    out = tmp_path / inc
    monkeypatch.setattr(sys, "argv", [tool + ".py", "--out", str(out)])
    _load(tool).main()  # (the module is executed with the variables set, as a fresh process would)
    assert out.read_bytes() == open(os.path.join(CSRC, inc), "rb").read()
