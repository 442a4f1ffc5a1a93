"""The generated K-loop of the 256^2 ping-pong GEMM (gemm_pp_step.inc, tools/gen_gemm_pp_asm.py) against
gemm_pp_kernel's HIP-source loop, bit for bit (torch.equal), through owlk_set_gemm_pp.

M = N = 512: four tiles, both wave groups, both B halves.  K = 64 n for n = 1 .. 7 enters and leaves the
five-tile ring period at every slot (6, 7 = one period + 1, + 2; 11, 12 a second time round).  Operands
are random per K-tile (scaled as in test_gemm_epi_exact_gpu.py), so a stale or early-read slot changes
bits.  Every epilogue runs at the layout it has in the training step.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
M = N = 512
KS = [64 * n for n in (1, 2, 3, 4, 5, 6, 7, 11, 12)]
EPI_KS = [192, 448]


def K():
    from owl_wms import kernels
    return kernels


@pytest.fixture(scope="module", autouse=True)
def _needs_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from owl_wms._lib import lib
    lib()


def both(fn):
    """fn() under the HIP-source loop (body 1) and the generated loop (body 2), every 256^2-tileable shape
    forced onto the ping-pong kernel; returns the two results."""
    from owl_wms import _lib
    outs = []
    try:
        for body in (1, 2):
            _lib.call("owlk_set_gemm_pp", body, 1)
            outs.append(fn())
        torch.cuda.synchronize()
    finally:
        _lib.call("owlk_set_gemm_pp", -1, -1)
    return outs


def same(a, b):
    a = a if isinstance(a, (tuple, list)) else (a,)
    b = b if isinstance(b, (tuple, list)) else (b,)
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert torch.equal(x, y), (x.float() - y.float()).abs().max().item()


def operands(Kd, at, bt, seed, m=M, n=N):
    g = torch.Generator().manual_seed(seed)
    A = (torch.randn((Kd, m) if at else (m, Kd), generator=g) * 0.5).bfloat16().to(DEV)
    B = (torch.randn((Kd, n) if bt else (n, Kd), generator=g) * 0.05).bfloat16().to(DEV)
    return A, B


def extras(seed, m=M, n=N):
    g = torch.Generator().manual_seed(1000 + seed)
    bias = (torch.randn(n, generator=g) * 0.3).float().to(DEV)
    x = torch.randn(m, n, generator=g).bfloat16().to(DEV)
    return bias, x


def test_first_contact_smallest_case():
    """One K-tile, layout 00, bf16 STORE: prologue -> last tile -> drain only."""
    k = K()
    A, B = operands(64, False, False, 0)
    o1, o2 = both(lambda: k.gemm(A, B))
    same(o1, o2)
    ref = A.float() @ B.float().t()
    assert ((o2.float() - ref).norm() / ref.norm()).item() < 1e-2


@pytest.mark.parametrize("out_f32", [False, True])
@pytest.mark.parametrize("at,bt", [(False, False), (False, True), (True, True), (True, False)])
def test_store_every_k(at, bt, out_f32):
    k = K()
    for Kd in KS:
        A, B = operands(Kd, at, bt, Kd)
        o1, o2 = both(lambda: k.gemm(A, B, a_trans=at, b_trans=bt, out_f32=out_f32))
        same(o1, o2)
    ref = (A.float().t() if at else A.float()) @ (B.float() if bt else B.float().t())
    assert ((o2.float() - ref).norm() / ref.norm()).item() < 1e-2


def test_ragged_m():
    """M = 512 + 40: the last tile row is partial (rows clamped in the LDS-DMA source offsets)."""
    k = K()
    for bt in (False, True):
        A, B = operands(448, False, bt, 5, m=M + 40)
        same(*both(lambda: k.gemm(A, B, b_trans=bt)))


@pytest.mark.parametrize("Kd", EPI_KS)
def test_store_bias_beta(Kd):
    k = K()
    A, B = operands(Kd, False, False, Kd + 1)
    bias, x = extras(1)

    def run():
        c = x.clone()
        k.gemm(A, B, out=c, epi=k.EPI_STORE, alpha=1.0, beta=0.5, bias=bias)
        return c
    same(*both(run))


@pytest.mark.parametrize("Kd", EPI_KS)
def test_silu(Kd):
    """fc1 forward: layout 00, bias, aux = the pre-activation."""
    k = K()
    A, B = operands(Kd, False, False, Kd + 2)
    bias, _ = extras(2)

    def run():
        c = torch.empty(M, N, device=DEV, dtype=torch.bfloat16)
        aux = torch.empty_like(c)
        k.gemm(A, B, out=c, epi=k.EPI_SILU, bias=bias, aux=aux)
        return c, aux
    same(*both(run))


@pytest.mark.parametrize("Kd", EPI_KS)
def test_dsilu_colsum(Kd):
    """fc2 dX: layout 01, aux = the pre-activation, resid <- silu(aux), fused column sums."""
    k = K()
    A, B = operands(Kd, False, True, Kd + 3)
    _, x = extras(3)

    def run():
        c = torch.empty(M, N, device=DEV, dtype=torch.bfloat16)
        act = torch.empty_like(c)
        cs = torch.zeros(N, device=DEV, dtype=torch.float32)
        k.gemm(A, B, b_trans=True, out=c, epi=k.EPI_DSILU, aux=x, resid=act, colsum=cs)
        return c, act, cs
    same(*both(run))


@pytest.mark.parametrize("Kd", EPI_KS)
def test_gate_resid(Kd):
    """out-projection / fc2 forward: layout 00, per-frame gate (64 rows per frame), residual, aux."""
    k = K()
    A, B = operands(Kd, False, False, Kd + 4)
    bias, x = extras(4)
    g = torch.Generator().manual_seed(40)
    gate = torch.randn(M // 64, N, generator=g).bfloat16().to(DEV)

    def run():
        c = torch.empty(M, N, device=DEV, dtype=torch.bfloat16)
        aux = torch.empty_like(c)
        k.gemm(A, B, out=c, epi=k.EPI_GATE_RESID, bias=bias, aux=aux, gate=gate, tpf=64, resid=x)
        return c, aux
    same(*both(run))


@pytest.mark.parametrize("Kd", EPI_KS)
def test_delta(Kd):
    """out-projection dX with the attention backward's delta: layout 01."""
    k = K()
    H, D = N // 64, 64
    dy, w = operands(Kd, False, True, Kd + 5)
    _, o = extras(5)
    same(*both(lambda: k.gemm_attn_delta(dy, w, o, H, D, 256)))


@pytest.mark.parametrize("Kd", EPI_KS)
def test_qkrope(Kd):
    """qkv projection with QK-RMSNorm + RoPE: layout 00, N = 3 H D = 768 (three tile columns)."""
    from oracle import ref_ops as R
    k = K()
    H, D = 4, 64
    h, w = operands(Kd, False, False, Kd + 6, n=3 * H * D)
    bias, _ = extras(6, n=3 * H * D)
    ang = R.motion_rope_angles(M // 64 + 8, 8, D)
    cos, sin = ang.cos().to(DEV).contiguous(), ang.sin().to(DEV).contiguous()
    same(*both(lambda: k.gemm_qk_rope(h, w, bias, H, D, cos, sin, 0, 256)))


@pytest.mark.parametrize("beta", [0.0, 1.0])
@pytest.mark.parametrize("m,n,Kd,splits", [(2304, 2560, 8192 + 64, 2), (M, N, 8192 + 64, 8)])
def test_splitk_ragged_last_chunk(m, n, Kd, splits, beta):
    """fp32 weight gradients (layout 11) on the split-K plan with a workspace.  90 tiles: two chunks of 65
    and 64 K-tiles; four tiles: eight chunks, the last one 10 K-tiles against 17."""
    from owl_wms import _lib
    k = K()
    assert _lib.lib().owlk_gemm_splitk_bytes(m, n, Kd, 1, 1, 1, 1, k.EPI_STORE, beta) == splits * m * n * 4
    A, B = operands(Kd, True, True, 7, m=m, n=n)
    g = torch.Generator().manual_seed(70)
    c0 = torch.randn(m, n, generator=g).float().to(DEV)

    def run():
        out = c0.clone()
        k.gemm(A, B, a_trans=True, b_trans=True, out=out, out_f32=True, beta=beta)
        return out
    o1, o2 = both(run)
    same(o1, o2)
    ref = A.float().t() @ B.float() + (c0 if beta else 0.0)
    assert ((o2 - ref).norm() / ref.norm()).item() < 1e-5
