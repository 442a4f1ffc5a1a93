"""owlk_grad_guard on the GPU (kernels.grad_guard): the global norm of a list of fp32 buffers against float64,
the fused clip against its formula and torch's clip_grad_norm_, the finite flag on NaN / Inf / fp32 overflow,
bit-for-bit determinism, untouched neighbours, and the binding's refusals.

Every buffer list is carved out of one allocation at 16-byte-aligned offsets with canaries between the
buffers, so a write outside a buffer shows.  A workgroup owns 65536 consecutive elements of one buffer and a
launch takes 16 buffers: the layouts cover lengths around the 4-element vector, a buffer of several whole
chunks (the unchecked fast path) and one more buffer than a pointer table holds."""
import math

import pytest
import torch

import conftest  # noqa: F401  (sys.path)

pytestmark = pytest.mark.gpu

MAX_NORM = 10.0
CANARY = 12345.0
PAD = 4  # canary elements around every buffer (16 bytes: keeps the offsets aligned)
CHUNK = 1 << 16
ISSUE = [1, 3, 4, 5, 1023, 1024, 1025, 8 * 1024 + 7]
LAYOUTS = {
    "issue": ISSUE,
    **{f"single{n}": [n] for n in ISSUE},
    "table": [1025] + [5, 1024, 7, 64, 1023] * 3 + [4 * 1024 + 2, 8 * 1024 + 7],  # 18 buffers: two launches
    "empty": [1025, 0, 4, 0, 8 * 1024 + 7, 0],
    "chunks": [2 * CHUNK + 5, CHUNK, CHUNK - 1],  # whole chunks, a short last one, several workgroups
}


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def carve(lengths, seed=0, target=None):
    """-> (arena, views): seeded normal values in the views, scaled so that their float64 norm is ``target``"""
    offs, o = [], PAD
    for n in lengths:
        offs.append(o)
        o += (n + 3) // 4 * 4 + PAD
    arena = torch.full((o,), CANARY, device="cuda", dtype=torch.float32)
    g = torch.Generator(device="cuda").manual_seed(seed)
    views = [arena[a:a + n] for a, n in zip(offs, lengths)]
    for v in views:
        v.copy_(torch.randn(v.numel(), device="cuda", generator=g))
    if target is not None:
        s = target / norm64(views)
        for v in views:
            v.mul_(s)
    return arena, views


def norm64(views):
    return float(torch.sqrt(sum(v.double().pow(2).sum() for v in views)))


def inside(arena, views):
    m = torch.zeros_like(arena, dtype=torch.bool)
    for v in views:
        m[v.storage_offset():v.storage_offset() + v.numel()] = True
    return m


def bits(t):
    return t.view(torch.int32)


def cat64(views):
    return torch.cat([v.double().flatten() for v in views])


def rel_l2(a, b):
    return float((a - b).norm() / b.norm())


def guard(views, max_norm=None):
    from owl_wms import kernels as K
    st = K.grad_guard(views, max_norm)
    assert st.dtype == torch.float32 and st.shape == (4,) and st.is_cuda
    return st.tolist()


@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_norm_and_unclipped_buffers(layout):
    """norm about half of max_norm: state = {norm, 1, 1, 0} and nothing is written, with a threshold, with
    None and with 0 (norm only)"""
    arena, views = carve(LAYOUTS[layout], seed=1, target=0.5 * MAX_NORM)
    before, ref = arena.clone(), norm64(views)
    for mn in (MAX_NORM, None, 0):
        norm, coef, finite, zero = guard(views, mn)
        err = abs(norm - ref) / ref
        print(f"{layout} max_norm={mn}: norm {norm!r} float64 {ref!r} rel err {err:.3e} coef {coef} finite {finite}")
        assert err <= 1e-5
        assert coef == 1.0 and finite == 1.0 and zero == 0.0
        assert torch.equal(bits(arena), bits(before))


@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_clipped_buffers(layout):
    """norm about 3 max_norm: g * max_norm / (norm64 + 1e-6), and what torch's clip leaves"""
    arena, views = carve(LAYOUTS[layout], seed=2, target=3.0 * MAX_NORM)
    before, ref = arena.clone(), norm64(views)
    want = cat64(views) * (MAX_NORM / (ref + 1e-6))
    ps = [torch.nn.Parameter(torch.empty_like(v)) for v in views]
    for p, v in zip(ps, views):
        p.grad = v.clone()
    tnorm = torch.nn.utils.clip_grad_norm_([p for p in ps if p.numel()], max_norm=MAX_NORM)
    norm, coef, finite, _ = guard(views, MAX_NORM)
    e_norm = abs(norm - ref) / ref
    e_formula = rel_l2(cat64(views), want)
    e_torch = rel_l2(cat64(views), cat64([p.grad for p in ps]))
    print(f"{layout}: norm {norm!r} float64 {ref!r} rel err {e_norm:.3e} (torch {float(tnorm)!r}); coef {coef!r}; "
          f"rel-L2 to the formula {e_formula:.3e}, to clip_grad_norm_ {e_torch:.3e}")
    assert e_norm <= 1e-5 and finite == 1.0
    assert abs(coef - MAX_NORM / (ref + 1e-6)) <= 1e-5 * coef and coef < 0.5
    assert e_formula <= 1e-5
    assert e_torch <= 1e-5
    m = inside(arena, views)
    assert torch.equal(arena[~m], before[~m])  # canaries, alignment gaps included
    assert abs(norm64(views) - MAX_NORM) <= 1e-4 * MAX_NORM


BAD = {"nan": float("nan"), "+inf": float("inf"), "-inf": float("-inf")}
# (buffer, element): the first of the first buffer, the last of the last buffer (its scalar tail), and an
# element of the first buffer of the second launch
WHERE = {"first": (0, 0), "tail": (-1, -1), "past_table": (16, 3)}


@pytest.mark.parametrize("where", list(WHERE))
@pytest.mark.parametrize("bad", list(BAD))
def test_non_finite_element_clears_the_flag_and_writes_nothing(bad, where):
    from owl_wms import kernels as K
    arena, views = carve(LAYOUTS["table"], seed=3, target=3.0 * MAX_NORM)  # would be clipped if finite
    assert K.GRAD_GUARD_TABLE == WHERE["past_table"][0] < len(views) - 1 and views[-1].numel() % 4
    b, k = WHERE[where]
    views[b][k] = BAD[bad]
    before = arena.clone()
    for mn in (MAX_NORM, None):
        norm, coef, finite, _ = guard(views, mn)
        print(f"{bad} at {where}, max_norm={mn}: norm {norm} coef {coef} finite {finite}")
        assert finite == 0.0 and coef == 1.0 and not math.isfinite(norm)
        assert torch.equal(bits(arena), bits(before))


@pytest.mark.parametrize("layout", ["issue", "chunks"])
def test_fp32_overflow_of_a_square_skips(layout):
    """1e20 is finite, its square is not in fp32: the partial overflows, and that step is skipped by design"""
    arena, views = carve(LAYOUTS[layout], seed=4, target=3.0 * MAX_NORM)
    views[-1][7] = 1e20
    before = arena.clone()
    norm, coef, finite, _ = guard(views, MAX_NORM)
    print(f"{layout}: one element 1e20 -> norm {norm} coef {coef} finite {finite}")
    assert finite == 0.0 and coef == 1.0
    assert torch.equal(bits(arena), bits(before))


@pytest.mark.parametrize("layout", ["issue", "table", "chunks"])
def test_two_calls_give_the_same_bits(layout):
    """a second call on a fresh copy, and a third under a CU reserve: the split never looks at the machine"""
    from owl_wms import _lib, kernels as K
    runs = []

    def run():
        arena, views = carve(LAYOUTS[layout], seed=5, target=3.0 * MAX_NORM)
        st = K.grad_guard(views, MAX_NORM)
        runs.append((st.clone(), arena.clone()))

    run()
    run()
    try:
        _lib.call("owlk_set_cu_reserve", 32)
        run()
    finally:
        _lib.call("owlk_set_cu_reserve", 0)
    print(layout, [r[0].tolist() for r in runs])
    for st, arena in runs[1:]:
        assert torch.equal(bits(st), bits(runs[0][0])) and torch.equal(bits(arena), bits(runs[0][1]))


def test_refusals_and_the_empty_list():
    from owl_wms import kernels as K
    arena, views = carve([64, 64], seed=6)
    with pytest.raises(RuntimeError, match="buffer 1 must be 16-byte aligned"):
        K.grad_guard([views[0], arena[PAD + 1:PAD + 9]])
    with pytest.raises(RuntimeError, match=r"buffer 1 must be float32 \(got torch.bfloat16\)"):
        K.grad_guard([views[0], views[1].bfloat16()])
    with pytest.raises(RuntimeError, match="buffer 0 must be contiguous"):
        K.grad_guard([views[0][::2]])
    with pytest.raises(RuntimeError, match="buffer 1 must be a device tensor"):
        K.grad_guard([views[0], views[1].cpu()])
    for mn in (None, MAX_NORM):
        st = guard([], mn)
        print("count 0:", st)
        assert st == [0.0, 1.0, 1.0, 0.0]
    st = guard([arena[:0], arena[:0]], MAX_NORM)  # nothing but empty buffers
    assert st == [0.0, 1.0, 1.0, 0.0]
