"""The row-wise HBM-bound kernels (elementwise.hip: AdaLN forward / backward, gate backward, the fused
AdaLN + gate backward, gate_resid; frames.hip: LayerNorm forward / backward), element by element.

References are float64 torch on the CPU from the same bf16 inputs; every assertion is per element and a
failure names row, column and frame.  No whole-tensor norms.

Shapes: d reaches every chunks-per-lane instantiation of OWLK_CPL_DISPATCH (8: one lane; 136: cpl 1;
520: cpl 2 with one lane in the second chunk; 1000: cpl 2 ragged; 1024; 2048: cpl 4; 3080: cpl 7 ->
<8> with the top chunk empty; 4096: cpl 8, 128 KiB of LDS in the backward), tpf reaches the row loop's
cases (1, 3: fewer rows than waves; 4: no prefetch; 5: one prefetch; 65: ragged against 4).

Inputs: frame f's modulation rows are scaled by (1 + f), token row t of x by (0.5 + t mod 7), so a wrong
frame index or a swapped rstd moves elements by far more than any bound; LayerNorm rows carry a mean of
about +-4 standard deviations.

Bounds (u = 2^-24, the fp32 unit roundoff; DEPTH = 8 MAXC + 6 <= 70 is the longest chain of fp32
additions in a row reduction: up to 64 elements per lane in sequence, then the 6 butterfly steps):
  rstd         the sum of squares has <= DEPTH roundings of positive terms (relative error <= 70 u), the
               square root halves that, the division, the eps add and a 1-ulp rsq add 3 u: 38 u < 2^-18
  y (AdaLN)    with the kernel's own rstd every step is one fp32 operation followed by RNE: bit-equal
  yact         hardware exp / rcp: one bf16 ulp of bf16(silu(y))
  dx           one bf16 ulp of the reference (the final RNE of a value within the fp32 bound of it) +
               DEPTH u (|r dy t1| + |r xh| mean_j |g_j xh_j| + |dres|): the summation-depth bound of the
               d-term dot product, and that many u on the other terms for the elementwise roundings
  column sums  tpf u sum_t |term|: each wave adds ceil(tpf / 4) terms in sequence (one rounding each, the
               product contracted or exact), the four wave partials add 3 more: <= tpf roundings for
               every tpf used here; + one bf16 ulp where the sum is stored as bf16
  LayerNorm    mean: DEPTH u mean|x| + u |mean|; rstd as above (the centred squares are positive; the
               error of mu enters squared); y with the kernel's mean / rstd: two fp32 roundings and the
               RNE, one bf16 ulp; dx: as AdaLN's with 6 more u for the elementwise roundings of
               xh = (x - mu) r, dy xh, the two divisions by d, the subtraction and the product with r
The FinalLayer backward (ypre) first puts dy through the bf16 silu backward.  Its hardware sigmoid is
accurate to a few fp32 ulps, so the inputs of that case are drawn until no element's float64 value lies
within 2^-17 (1 + |ypre|) |dy| of a bf16 rounding boundary: the rounded dy is then the same for every
accurate evaluation and the bounds above apply unchanged.
"""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16 = torch.bfloat16

U = 2.0 ** -24
DEPTH = 70
LN_EXTRA = 6
RSTD_REL = 2.0 ** -18
RMS_EPS = 1.1920928955078125e-07  # finfo(float32).eps, F.rms_norm's default
LN_EPS = 1e-5
SENT = -776.0  # exact in bf16 and fp32; no kernel output of these inputs is a whole tensor of it


def K():
    from owl_wms import kernels
    return kernels


@pytest.fixture(scope="module", autouse=True)
def _needs_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from owl_wms._lib import lib
    lib()


# (d, tpf, F, wide): wide = x / dy / y rows are 16-byte-aligned column slices of a wider buffer.  Every d
# with at least two tpf, every tpf with at least two d; T = F tpf is no multiple of 4 in most cases
CASES = [(8, 1, 3, False), (8, 65, 2, True), (136, 3, 3, True), (136, 5, 2, False), (520, 4, 3, False),
         (520, 1, 2, True), (1000, 5, 3, True), (1000, 65, 2, False), (1024, 1, 3, False), (1024, 4, 2, True),
         (2048, 3, 3, False), (2048, 65, 2, True), (3080, 4, 2, False), (3080, 5, 3, True), (4096, 3, 2, True),
         (4096, 5, 3, False), (4096, 65, 2, False)]
case_ids = [f"d{d}-tpf{t}-F{f}{'-wide' if w else ''}" for d, t, f, w in CASES]
cases = pytest.mark.parametrize("case", CASES, ids=case_ids)


def bf(t):
    return t.to(BF16)


def ulps(a, b):
    """bf16 ulp distance on the monotonic integer line (-0 == +0)"""
    def key(t):
        i = t.contiguous().view(torch.int16).int()
        return torch.where(i >= 0, i, -32768 - i)
    return (key(a) - key(b)).abs()


def ulp_bf16(v):
    """one bf16 ulp at the magnitude of each float64 value"""
    _, e = torch.frexp(v.abs().clamp_min(2.0 ** -120))
    return torch.pow(2.0, (e - 8).double())


def _where(i, ncol, tpf):
    r, c = divmod(int(i), ncol)
    return f"frame {r} col {c}" if tpf is None else f"row {r} col {c} frame {r // tpf}"


def assert_bits(got, ref, what, tpf=None):
    got, ref = got.cpu(), ref.cpu()
    assert got.shape == ref.shape and got.dtype == ref.dtype, what
    if got.dtype == BF16:
        bad = ulps(got, ref) != 0
    else:
        bad = ~((got == ref) | (got.isnan() & ref.isnan()))
    if bad.any():
        i = bad.flatten().nonzero()[0].item()
        pytest.fail(f"{what}: {_where(i, got.shape[-1], tpf)}: got {got.flatten()[i].item()!r}, expected "
                    f"{ref.flatten()[i].item()!r} ({int(bad.sum())} of {bad.numel()} elements differ)")


def assert_within(got, ref, bound, what, tpf=None):
    """|got - ref| <= bound per element (float64 on the CPU; a NaN fails)"""
    got = got.cpu().double()
    if got.dim() == 1:
        got, ref, bound = got[:, None], ref[:, None], bound[:, None]
    assert got.shape == ref.shape == bound.shape, what
    err = (got - ref).abs()
    bad = ~(err <= bound)
    if bad.any():
        i = bad.flatten().nonzero()[0].item()
        pytest.fail(f"{what}: {_where(i, got.shape[-1], tpf)}: got {got.flatten()[i].item()!r}, reference "
                    f"{ref.flatten()[i].item()!r}, |error| {err.flatten()[i].item():.3e} > bound "
                    f"{bound.flatten()[i].item():.3e} ({int(bad.sum())} of {bad.numel()} elements out of bound)")


def assert_sentinel(t, what):
    t = t.cpu().float()
    bad = t != SENT
    if bad.any():
        i = bad.flatten().nonzero()[0].item()
        pytest.fail(f"{what}: stray write at flat index {i} of shape {tuple(t.shape)} "
                    f"({int(bad.sum())} elements overwritten)")


# ------------------------------------------------------------------ inputs (CPU, once per case)
def dsilu64(dy, yp):
    yp = yp.double()
    sg = 1.0 / (1.0 + torch.exp(-yp))
    return dy.double() * sg * (1.0 + yp * (1.0 - sg))


def settle_dsilu(dy, yp, g):
    """redraw the elements whose silu backward lies near a bf16 rounding boundary (module docstring);
    -> dy, ypre and the bf16 silu backward of dy every accurate evaluation gives"""
    for _ in range(200):
        v = dsilu64(dy, yp)
        m = dy.double().abs() * (1.0 + yp.double().abs()) * 2.0 ** -17
        lo, hi = bf(v - m), bf(v + m)
        amb = ulps(lo, hi) != 0
        if not amb.any():
            return dy, yp, lo
        n = int(amb.sum())
        dy, yp = dy.clone(), yp.clone()
        dy[amb] = bf(torch.randn(n, generator=g) * 2.0)
        yp[amb] = bf((torch.randn(n, generator=g) * 2.0).clamp(-8.0, 8.0))
    raise AssertionError("no unambiguous silu-backward inputs found")


@functools.lru_cache(maxsize=None)
def data(d, tpf, F):
    g = torch.Generator().manual_seed(100003 * d + 101 * tpf + F)
    T = F * tpf
    t = torch.arange(T)
    x = bf(torch.randn(T, d, generator=g) * (0.5 + t % 7)[:, None])
    # [scale1 | shift1 | gate1 | scale2 | shift2 | gate2] like the block's stacked modulation matrix
    mods = bf(torch.randn(F, 6 * d, generator=g) * 0.3 * (1.0 + torch.arange(F))[:, None])
    dy = bf(torch.randn(T, d, generator=g) * (0.25 + t % 5)[:, None])
    dres = bf(torch.randn(T, d, generator=g) * 0.5)
    yb = bf(torch.randn(T, d, generator=g) * (0.5 + t % 3)[:, None])
    yp = bf((torch.randn(T, d, generator=g) * 2.0).clamp(-8.0, 8.0))
    dyf, yp, dv = settle_dsilu(dy.clone(), yp, g)
    sign = torch.where(t % 2 == 0, 1.0, -1.0)
    xln = bf((torch.randn(T, d, generator=g) + (sign * (3.5 + 0.5 * (t % 3)))[:, None]) * (0.5 + t % 7)[:, None])
    return dict(x=x, mods=mods, dy=dy, dres=dres, yb=yb, yp=yp, dyf=dyf, dv=dv, xln=xln,
                fi=t // tpf, T=T)


def rows(t, wide):
    """the tensor on the device, contiguous or as a 16-byte-aligned column slice of a wider buffer"""
    if not wide:
        return t.to(DEV)
    buf = torch.full((t.shape[0], t.shape[1] + 24), 3.0, dtype=t.dtype, device=DEV)
    v = buf[:, 8:8 + t.shape[1]]
    v.copy_(t)
    assert v.data_ptr() % 16 == 0 and (v.stride(0) * v.element_size()) % 16 == 0
    return v


@functools.lru_cache(maxsize=None)
def fwd_out(case):
    """the AdaLN forward of both of the block's AdaLN layers, shared by the backward tests"""
    d, tpf, F, wide = case
    D = data(d, tpf, F)
    k = K()
    x, mods = rows(D["x"], wide), D["mods"].to(DEV)
    y, rstd, ya = k.adaln_fwd(x, mods[:, :d], mods[:, d:2 * d], tpf, act=True)
    y2, rstd2 = k.adaln_fwd(x, mods[:, 3 * d:4 * d], mods[:, 4 * d:5 * d], tpf)
    torch.cuda.synchronize()
    return y.cpu(), rstd.cpu(), ya.cpu(), y2.cpu(), rstd2.cpu()


# ------------------------------------------------------------------ AdaLN forward
def adaln_replay(x, a, b, fi, r32):
    """y with the kernel's rstd: bf16(bf16(bf16(x r) bf16(1 + a)) + b), one fp32 operation per rounding"""
    xn = bf(x.float() * r32[:, None]).float()
    t1 = bf(1.0 + a.float()).float()[fi]
    return bf(bf(xn * t1).float() + b.float()[fi]), xn


@cases
def test_adaln_fwd(case):
    d, tpf, F, wide = case
    D = data(d, tpf, F)
    y, rstd, ya, y2, rstd2 = fwd_out(case)
    r64 = 1.0 / torch.sqrt((D["x"].double() ** 2).mean(1) + RMS_EPS)
    assert_within(rstd, r64, RSTD_REL * r64, "adaln_fwd rstd", tpf)
    assert_bits(rstd2, rstd, "adaln_fwd rstd (second layer)", tpf)
    m = D["mods"]
    assert_bits(y, adaln_replay(D["x"], m[:, :d], m[:, d:2 * d], D["fi"], rstd)[0], "adaln_fwd y", tpf)
    assert_bits(y2, adaln_replay(D["x"], m[:, 3 * d:4 * d], m[:, 4 * d:5 * d], D["fi"], rstd)[0],
                "adaln_fwd y (second layer)", tpf)
    y64 = y.double()
    ref = bf(y64 / (1.0 + torch.exp(-y64)))
    bad = ulps(ya, ref) > 1
    if bad.any():
        i = bad.flatten().nonzero()[0].item()
        pytest.fail(f"adaln_fwd yact: {_where(i, d, tpf)}: got {ya.flatten()[i].item()!r}, bf16(silu(y)) "
                    f"{ref.flatten()[i].item()!r} ({int(bad.sum())} elements beyond one ulp)")


# ------------------------------------------------------------------ AdaLN backward
def adaln_bwd_ref(dv, x, r32, a, fi, F, tpf, dres):
    """float64 dx / dscale / dshift and their bounds; dv is dy as the kernel uses it (after the silu
    backward in the FinalLayer form), r32 the kernel's rstd"""
    d = x.shape[1]
    r = r32.double()[:, None]
    t1 = bf(1.0 + a.float()).double()[fi]
    xh = x.double() * r
    g = dv.double() * t1
    gx = g * xh
    res = dres.double() if dres is not None else torch.zeros_like(xh)
    dx = r * (g - xh * gx.mean(1, keepdim=True)) + res
    bdx = ulp_bf16(dx) + DEPTH * U * ((r * g).abs() + (r * xh).abs() * gx.abs().mean(1, keepdim=True) + res.abs())
    xn = bf(x.float() * r32[:, None]).double()  # the kernel rounds the fp32 product to bf16
    tsc = (dv.double() * xn).view(F, tpf, d)
    tsh = dv.double().view(F, tpf, d)
    return dict(dx=dx, bdx=bdx, dsc=tsc.sum(1), bsc=tpf * U * tsc.abs().sum(1), dsh=tsh.sum(1),
                bsh=tpf * U * tsh.abs().sum(1))


def check_dmod(dm, ref, d, what, is_bf16):
    ex = (lambda s: ulp_bf16(s)) if is_bf16 else (lambda s: 0.0)
    assert_within(dm[:, :d], ref["dsc"], ref["bsc"] + ex(ref["dsc"]), what + " dscale")
    assert_within(dm[:, d:], ref["dsh"], ref["bsh"] + ex(ref["dsh"]), what + " dshift")


@pytest.mark.parametrize("mode", ["plain", "dres", "ypre"])
@cases
def test_adaln_bwd(case, mode):
    d, tpf, F, wide = case
    D = data(d, tpf, F)
    k = K()
    rstd = fwd_out(case)[1]
    a = D["mods"][:, :d]
    dy_c = D["dyf"] if mode == "ypre" else D["dy"]
    dv = D["dv"] if mode == "ypre" else D["dy"]
    dres_c = D["dres"] if mode == "dres" else None
    ref = adaln_bwd_ref(dv, D["x"], rstd, a, D["fi"], F, tpf, dres_c)
    x, dy, mods, r = rows(D["x"], wide), rows(dy_c, wide), D["mods"].to(DEV), rstd.to(DEV)
    dres = rows(dres_c, wide) if dres_c is not None else None
    ypre = rows(D["yp"], wide) if mode == "ypre" else None
    dx, dmod = k.adaln_bwd(dy, x, r, mods[:, :d], tpf, dres=dres, ypre=ypre)
    assert_within(dx, ref["dx"], ref["bdx"], f"adaln_bwd[{mode}] dx", tpf)
    check_dmod(dmod, ref, d, f"adaln_bwd[{mode}]", False)
    # the bf16 form, into columns [d, 3d) of a wider sentinel-filled modulation-gradient matrix
    dm = torch.full((F, 6 * d), SENT, device=DEV, dtype=BF16)
    dxb = k.adaln_bwd_into(dy, x, r, mods[:, :d], tpf, dm[:, d:3 * d], dres=dres, ypre=ypre)
    assert_bits(dxb, dx, f"adaln_bwd_into[{mode}] dx against the fp32-dmod form", tpf)
    check_dmod(dm[:, d:3 * d], ref, d, f"adaln_bwd_into[{mode}]", True)
    assert_sentinel(dm[:, :d], "adaln_bwd_into: columns left of dmod")
    assert_sentinel(dm[:, 3 * d:], "adaln_bwd_into: columns right of dmod")


# ------------------------------------------------------------------ gate backward, fused AdaLN + gate backward
def gate_bwd_ref(dout, y, g, fi, F, tpf):
    """dy = bf16(dout g) (one product, exact in fp32 before the RNE); dg = sum_t dout y; dbf = sum_t dy
    over the ROUNDED dy"""
    d = y.shape[1]
    dy = bf(dout.float() * g.float()[fi])
    tg = (dout.double() * y.double()).view(F, tpf, d)
    tb = dy.double().view(F, tpf, d)
    return dict(dy=dy, dg=tg.sum(1), bg=tpf * U * tg.abs().sum(1), dbf=tb.sum(1), bb=tpf * U * tb.abs().sum(1))


@cases
def test_gate_bwd(case):
    d, tpf, F, wide = case
    D = data(d, tpf, F)
    k = K()
    g_c = D["mods"][:, 2 * d:3 * d]
    ref = gate_bwd_ref(D["dy"], D["yb"], g_c, D["fi"], F, tpf)
    dout, y, mods = rows(D["dy"], wide), rows(D["yb"], wide), D["mods"].to(DEV)
    dy, dg, dbf = k.gate_bwd(dout, y, mods[:, 2 * d:3 * d], tpf)
    assert_bits(dy, ref["dy"], "gate_bwd dy", tpf)
    assert_within(dg, ref["dg"], ref["bg"], "gate_bwd dg")
    assert_within(dbf, ref["dbf"], ref["bb"], "gate_bwd dbias_frames (sum of the rounded dy)")
    dm = torch.full((F, 6 * d), SENT, device=DEV, dtype=BF16)
    dy2, dg2, dbf2 = k.gate_bwd(dout, y, mods[:, 2 * d:3 * d], tpf, dg_out=dm[:, 2 * d:3 * d])
    assert_bits(dy2, ref["dy"], "gate_bwd[dg bf16] dy", tpf)
    assert_bits(dbf2, dbf, "gate_bwd[dg bf16] dbias_frames against the fp32-dg form")
    assert_within(dm[:, 2 * d:3 * d], ref["dg"], ref["bg"] + ulp_bf16(ref["dg"]), "gate_bwd[dg bf16] dg")
    assert_sentinel(dm[:, :2 * d], "gate_bwd: columns left of dg_out")
    assert_sentinel(dm[:, 3 * d:], "gate_bwd: columns right of dg_out")
    assert k.gate_bwd(dout, y, mods[:, 2 * d:3 * d], tpf, want_bias=False)[2] is None


@cases
def test_adaln_gate_bwd_into(case):
    """the MLP-branch AdaLN backward (scale2) feeding the attention branch's gate (gate1), as the block's
    backward calls it: dx and dmod to adaln_bwd's bounds, the gate's outputs against the kernel's own dx"""
    d, tpf, F, wide = case
    D = data(d, tpf, F)
    k = K()
    rstd = fwd_out(case)[1]
    ref = adaln_bwd_ref(D["dy"], D["x"], rstd, D["mods"][:, 3 * d:4 * d], D["fi"], F, tpf, D["dres"])
    x, dh, dres, y = (rows(D[n], wide) for n in ("x", "dy", "dres", "yb"))
    mods, r = D["mods"].to(DEV), rstd.to(DEV)
    dm = torch.full((F, 6 * d), SENT, device=DEV, dtype=BF16)
    dx, dyg, dbf = k.adaln_gate_bwd_into(dh, x, r, mods[:, 3 * d:4 * d], tpf, dm[:, 3 * d:5 * d], dres, y,
                                         mods[:, 2 * d:3 * d], dm[:, 2 * d:3 * d])
    assert_within(dx, ref["dx"], ref["bdx"], "adaln_gate_bwd dx", tpf)
    check_dmod(dm[:, 3 * d:5 * d], ref, d, "adaln_gate_bwd", True)
    gref = gate_bwd_ref(dx.cpu(), D["yb"], D["mods"][:, 2 * d:3 * d], D["fi"], F, tpf)
    assert_bits(dyg, gref["dy"], "adaln_gate_bwd dyg = bf16(dx g) of its own dx", tpf)
    assert_within(dm[:, 2 * d:3 * d], gref["dg"], gref["bg"] + ulp_bf16(gref["dg"]), "adaln_gate_bwd dg")
    assert_within(dbf, gref["dbf"], gref["bb"], "adaln_gate_bwd dbias_frames (sum of the rounded dyg)")
    assert_sentinel(dm[:, :2 * d], "adaln_gate_bwd: columns left of dg_out | dmod")
    assert_sentinel(dm[:, 5 * d:], "adaln_gate_bwd: columns right of dmod")
    dm2 = torch.full((F, 6 * d), SENT, device=DEV, dtype=BF16)
    dx2, dyg2, none = k.adaln_gate_bwd_into(dh, x, r, mods[:, 3 * d:4 * d], tpf, dm2[:, 3 * d:5 * d], dres, y,
                                            mods[:, 2 * d:3 * d], dm2[:, 2 * d:3 * d], want_bias=False)
    assert none is None
    assert_bits(dx2, dx, "adaln_gate_bwd[no bias] dx", tpf)
    assert_bits(dyg2, dyg, "adaln_gate_bwd[no bias] dyg", tpf)
    assert_bits(dm2, dm, "adaln_gate_bwd[no bias] dmod | dg")


# ------------------------------------------------------------------ gate + residual
@cases
def test_gate_resid(case):
    d, tpf, F, wide = case
    D = data(d, tpf, F)
    k = K()
    x, y, mods = rows(D["x"], wide), rows(D["yb"], wide), D["mods"].to(DEV)
    out = k.gate_resid(x, y, mods[:, 2 * d:3 * d], tpf)
    t = bf(D["mods"][:, 2 * d:3 * d].float()[D["fi"]] * D["yb"].float())
    assert_bits(out, bf(D["x"].float() + t.float()), "gate_resid", tpf)


@pytest.mark.parametrize("Mx,N,Kd,tpf", [(195, 136, 72, 65), (40, 1024, 64, 1)])
def test_gate_resid_equals_gemm_epilogue(Mx, N, Kd, tpf):
    """gate_resid rebuilds the GATE_RESID GEMM epilogue's output from its kept inputs, bit for bit"""
    k = K()
    g = torch.Generator().manual_seed(77)
    F = Mx // tpf
    A = bf(torch.randn(Mx, Kd, generator=g) * 0.5).to(DEV)
    B = bf(torch.randn(N, Kd, generator=g) * 0.2).to(DEV)
    bias = (torch.randn(N, generator=g) * 0.3).to(DEV)
    x = bf(torch.randn(Mx, N, generator=g) * (0.5 + torch.arange(Mx) % 7)[:, None]).to(DEV)
    gate = bf(torch.randn(F, 6 * N, generator=g) * (1.0 + torch.arange(F))[:, None]).to(DEV)[:, 2 * N:3 * N]
    y1 = torch.empty(Mx, N, device=DEV, dtype=BF16)
    c = k.gemm(A, B, bias=bias, epi=k.EPI_GATE_RESID, aux=y1, gate=gate, tpf=tpf, resid=x)
    assert_bits(k.gate_resid(x, y1, gate, tpf), c, "gate_resid against gemm(epi=EPI_GATE_RESID)", tpf)


# ------------------------------------------------------------------ LayerNorm
@functools.lru_cache(maxsize=None)
def ln_out(case):
    d, tpf, F, wide = case
    D = data(d, tpf, F)
    y, mean, rstd = K().layernorm_fwd(rows(D["xln"], wide))
    torch.cuda.synchronize()
    return y.cpu(), mean.cpu(), rstd.cpu()


@cases
def test_layernorm_fwd(case):
    d, tpf, F, wide = case
    x = data(d, tpf, F)["xln"].double()
    y, mean, rstd = ln_out(case)
    mu64 = x.mean(1)
    assert_within(mean, mu64, DEPTH * U * x.abs().mean(1) + U * mu64.abs(), "layernorm_fwd mean", 1)
    r64 = 1.0 / torch.sqrt(((x - mu64[:, None]) ** 2).mean(1) + LN_EPS)
    assert_within(rstd, r64, RSTD_REL * r64, "layernorm_fwd rstd", 1)
    ref = (x - mean.double()[:, None]) * rstd.double()[:, None]
    assert_within(y, ref, ulp_bf16(ref), "layernorm_fwd y with the kernel's mean / rstd", 1)


@cases
def test_layernorm_bwd(case):
    d, tpf, F, wide = case
    D = data(d, tpf, F)
    _, mean, rstd = ln_out(case)
    dx = K().layernorm_bwd(rows(D["dy"], wide), rows(D["xln"], wide), mean.to(DEV), rstd.to(DEV))
    r = rstd.double()[:, None]
    xh = (D["xln"].double() - mean.double()[:, None]) * r
    g = D["dy"].double()
    ref = r * (g - g.mean(1, keepdim=True) - xh * (g * xh).mean(1, keepdim=True))
    bound = ulp_bf16(ref) + (DEPTH + LN_EXTRA) * U * (
        (r * g).abs() + r * g.abs().mean(1, keepdim=True) + (r * xh).abs() * (g * xh).abs().mean(1, keepdim=True))
    assert_within(dx, ref, bound, "layernorm_bwd dx", 1)


# ------------------------------------------------------------------ padded outputs: nothing outside [T, d] is written
@pytest.mark.parametrize("case", [(136, 5, 3, True), (3080, 3, 3, False), (4096, 65, 2, False)],
                         ids=["d136-tpf5", "d3080-tpf3", "d4096-tpf65"])
def test_padded_outputs_keep_their_sentinels(case):
    """every kernel through the C ABI with output row strides > d and spare rows behind T (T % 4 != 0, so
    the forward's last workgroup has idle waves): the [T, d] block equals the wrapper's output bit for bit,
    every other element of the buffers still holds the sentinel"""
    from owl_wms import _lib
    d, tpf, F, wide = case
    D = data(d, tpf, F)
    k = K()
    T, PR, PC = D["T"], 5, 16
    assert T % 4 != 0
    p, st = _lib.ptr, _lib.stream

    def padded(dtype=BF16):
        return torch.full((T + PR, d + PC), SENT, device=DEV, dtype=dtype)

    def vec():
        return torch.full((T + PR,), SENT, device=DEV, dtype=torch.float32)

    def check(buf, want, what):
        assert_bits(buf[:T, :d], want, what, tpf)
        assert_sentinel(buf[:T, d:], what + ": columns behind d")
        assert_sentinel(buf[T:], what + ": rows behind T")

    def check_vec(v, want, what):
        assert_bits(v[:T], want, what)
        assert_sentinel(v[T:], what + ": rows behind T")

    x, dy, dres, yb, xln = (rows(D[n], wide) for n in ("x", "dy", "dres", "yb", "xln"))
    mods = D["mods"].to(DEV)
    sc, sh, g = mods[:, :d], mods[:, d:2 * d], mods[:, 2 * d:3 * d]
    ldm = mods.stride(0)

    y0, r0, ya0 = k.adaln_fwd(x, sc, sh, tpf, act=True)
    y, ya, r = padded(), padded(), vec()
    _lib.call("owlk_adaln_fwd", p(x), x.stride(0), p(sc), p(sh), ldm, tpf, T, d, p(y), d + PC, p(r), p(ya), st())
    check(y, y0, "adaln_fwd y")
    check(ya, ya0, "adaln_fwd yact")
    check_vec(r, r0, "adaln_fwd rstd")

    dm0 = torch.full((F, 6 * d), SENT, device=DEV, dtype=BF16)
    dx0 = k.adaln_bwd_into(dy, x, r0, sc, tpf, dm0[:, :2 * d], dres=dres)
    dx, dm = padded(), torch.full((F + 2, 6 * d), SENT, device=DEV, dtype=BF16)
    _lib.call("owlk_adaln_bwd", p(dy), dy.stride(0), p(x), x.stride(0), p(r0), p(sc), ldm, tpf, T, d, p(dres),
              dres.stride(0), p(dx), d + PC, p(dm), p(dm[:, d:]), dm.stride(0), None, 1, st())
    check(dx, dx0, "adaln_bwd dx")
    assert_bits(dm[:F], dm0, "adaln_bwd dmod")
    assert_sentinel(dm[F:], "adaln_bwd dmod: rows behind F")

    dyg0, _, dbf0 = k.gate_bwd(dy, yb, g, tpf, dg_out=dm0[:, 2 * d:3 * d])
    dyg, dbf = padded(), torch.full((F + 2, d + PC), SENT, device=DEV, dtype=torch.float32)
    _lib.call("owlk_gate_bwd", p(dy), dy.stride(0), p(yb), yb.stride(0), p(g), ldm, tpf, T, d, p(dyg), d + PC,
              p(dm[:, 2 * d:]), dm.stride(0), 1, p(dbf), d + PC, st())
    check(dyg, dyg0, "gate_bwd dy")
    assert_bits(dm[:F], dm0, "gate_bwd dg")
    assert_bits(dbf[:F, :d], dbf0, "gate_bwd dbias_frames")
    assert_sentinel(dbf[:F, d:], "gate_bwd dbias_frames: columns behind d")
    assert_sentinel(dbf[F:], "gate_bwd dbias_frames: rows behind F")
    assert_sentinel(dm[F:], "gate_bwd dg: rows behind F")

    dm1 = torch.full((F, 6 * d), SENT, device=DEV, dtype=BF16)
    dx1, dyg1, dbf1 = k.adaln_gate_bwd_into(dy, x, r0, mods[:, 3 * d:4 * d], tpf, dm1[:, 3 * d:5 * d], dres, yb, g,
                                            dm1[:, 2 * d:3 * d])
    dx, dyg = padded(), padded()
    dbf = torch.full((F + 2, d + PC), SENT, device=DEV, dtype=torch.float32)
    dm = torch.full((F + 2, 6 * d), SENT, device=DEV, dtype=BF16)
    _lib.call("owlk_adaln_gate_bwd", p(dy), dy.stride(0), p(x), x.stride(0), p(r0), p(mods[:, 3 * d:]), ldm, tpf, T,
              d, p(dres), dres.stride(0), p(dx), d + PC, p(dm[:, 3 * d:]), p(dm[:, 4 * d:]), dm.stride(0), 1, p(yb),
              yb.stride(0), p(g), ldm, p(dyg), d + PC, p(dm[:, 2 * d:]), dm.stride(0), 1, p(dbf), d + PC, st())
    check(dx, dx1, "adaln_gate_bwd dx")
    check(dyg, dyg1, "adaln_gate_bwd dyg")
    assert_bits(dm[:F], dm1, "adaln_gate_bwd dmod | dg")
    assert_sentinel(dm[F:], "adaln_gate_bwd dmod | dg: rows behind F")
    assert_bits(dbf[:F, :d], dbf1, "adaln_gate_bwd dbias_frames")
    assert_sentinel(dbf[:F, d:], "adaln_gate_bwd dbias_frames: columns behind d")
    assert_sentinel(dbf[F:], "adaln_gate_bwd dbias_frames: rows behind F")

    out = padded()
    _lib.call("owlk_gate_resid", p(x), x.stride(0), p(yb), yb.stride(0), p(g), ldm, tpf, T, d, p(out), d + PC, st())
    check(out, k.gate_resid(x, yb, g, tpf), "gate_resid")

    yl0, mu0, rl0 = k.layernorm_fwd(xln)
    yl, mu, rl = padded(), vec(), vec()
    _lib.call("owlk_layernorm_fwd", p(xln), xln.stride(0), T, d, p(yl), d + PC, p(mu), p(rl), st())
    check(yl, yl0, "layernorm_fwd y")
    check_vec(mu, mu0, "layernorm_fwd mean")
    check_vec(rl, rl0, "layernorm_fwd rstd")
    dxl = padded()
    _lib.call("owlk_layernorm_bwd", p(dy), dy.stride(0), p(xln), xln.stride(0), p(mu0), p(rl0), T, d, p(dxl), d + PC,
              st())
    check(dxl, k.layernorm_bwd(dy, xln, mu0, rl0), "layernorm_bwd dx")


# ------------------------------------------------------------------ contracts
def test_rows_wider_than_the_maximum_are_rejected():
    """d > 64 * 8 * MAXCPL = 4096 has no instantiation: every entry refuses it with a message, before any
    launch"""
    k = K()
    d, T = 4104, 4
    x = torch.zeros(T, d, device=DEV, dtype=BF16)
    m = torch.zeros(1, 2 * d, device=DEV, dtype=BF16)
    r = torch.ones(T, device=DEV)
    with pytest.raises(RuntimeError, match="adaln_fwd: bad d=4104"):
        k.adaln_fwd(x, m[:, :d], m[:, d:], 4)
    with pytest.raises(RuntimeError, match="adaln_bwd: bad d=4104"):
        k.adaln_bwd(x, x, r, m[:, :d], 4)
    with pytest.raises(RuntimeError, match="gate_bwd: bad d=4104"):
        k.gate_bwd(x, x, m[:, :d], 4)
    with pytest.raises(RuntimeError, match="adaln_gate_bwd: bad d=4104"):
        k.adaln_gate_bwd_into(x, x, r, m[:, :d], 4, torch.zeros_like(m), x, x, m[:, :d], torch.zeros_like(m[:, :d]))
    with pytest.raises(RuntimeError, match="layernorm_fwd: bad d=4104"):
        k.layernorm_fwd(x)
    with pytest.raises(RuntimeError, match="layernorm_bwd: bad d=4104"):
        k.layernorm_bwd(x, x, r, r)


def test_adaln_bwd_ypre_shares_dys_rows():
    """owlk_adaln_bwd reads ypre with dy's row stride (include/owlk.h): the wrappers refuse a ypre laid
    out differently, and a ypre that is a column slice like dy gives the contiguous call's bits"""
    k = K()
    d, tpf, F = 136, 5, 2
    D = data(d, tpf, F)
    mods = D["mods"].to(DEV)
    x, dy, yp = D["x"].to(DEV), D["dyf"].to(DEV), D["yp"].to(DEV)
    _, rstd = k.adaln_fwd(x, mods[:, :d], mods[:, d:2 * d], tpf)
    dx0, dmod0 = k.adaln_bwd(dy, x, rstd, mods[:, :d], tpf, ypre=yp)
    dx1, dmod1 = k.adaln_bwd(rows(D["dyf"], True), x, rstd, mods[:, :d], tpf, ypre=rows(D["yp"], True))
    assert_bits(dx1, dx0, "adaln_bwd[ypre] dx, strided against contiguous", tpf)
    assert_bits(dmod1, dmod0, "adaln_bwd[ypre] dmod, strided against contiguous")
    dm = torch.zeros(F, 2 * d, device=DEV, dtype=BF16)
    with pytest.raises(AssertionError, match="ypre"):
        k.adaln_bwd(dy, x, rstd, mods[:, :d], tpf, ypre=rows(D["yp"], True))
    with pytest.raises(AssertionError, match="ypre"):
        k.adaln_bwd_into(rows(D["dyf"], True), x, rstd, mods[:, :d], tpf, dm, ypre=yp)
