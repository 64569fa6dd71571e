"""The dense-layer entry points of csrc/dense.hip called directly (-m gpu): nerf_dense_fwd / _dgrad / _wgrad and nerf_build_inputs
through the C ABI with raw pointers, against the same expression in float64 torch on the CPU.

Every operand is a column range of a wider matrix (leading dimension > width, column offset > 0) that is filled with a sentinel
before the call; everything outside the written range must hold the sentinel afterwards.  Two data regimes for the GEMMs:
  integers  operands are integers in [-8, 8]: every product and partial sum is an integer below 2^24, so the fp32 result is exact in
            any summation order, with or without FMA -- compared BIT FOR BIT with the float64 result cast to fp32.  (x, w and dy are
            drawn without zeros: a sum with a nonzero term that comes out 0 is +0 in any order, so no result's sign of zero
            depends on the order either.  The constructed rows do hold zeros, next to a cancelling nonzero pair.)
  floats    seeded randn; per element |got - ref| <= gamma_n * S with S the same expression on absolute values, gamma_n = n u / (1 - n u),
            u = 2^-24, n = inner length + 2: the forward error bound of an fp32 dot product in any order plus the two epilogue
            additions.  No measured tolerance; a reduced-precision GEMM mode fails it.
Also here: the empty batch (C level, DenseNeRF, render_rays) and the slicing of DenseNeRF.query."""
import pytest
import torch

import nerf_oracle as orc
from test_gpu_dense import ARCHS, _net
from test_gpu_parity import dev, npa  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

SENT = -77777.0         # what the wider matrices hold outside the operand's column range
U = 2.0 ** -24
SHAPES = [(1, 1, 1), (63, 3, 5), (257, 27, 65), (300, 90, 128), (64, 256, 3)]           # (P, K, N)
COLSUM_ROWS = 2048      # rows per block of the bias gradient's first pass (csrc/dense.hip)


def gamma(n):
    return n * U / (1.0 - n * U)


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


class Wide:
    """a [rows, lo + cols + pad] sentinel-filled device matrix whose columns lo : lo + cols are the operand"""

    def __init__(self, dev, rows, cols, lo, pad, inner=None):
        self.lo, self.cols, self.ld = lo, cols, lo + cols + pad
        host = torch.full((rows, self.ld), SENT, dtype=torch.float32)
        host[:, lo:lo + cols] = float("nan") if inner is None else inner         # NaN: an output that must not be read
        self.t = host.to(dev)

    @property
    def ptr(self):
        return self.t.data_ptr() + 4 * self.lo

    def inner(self):
        return self.t[:, self.lo:self.lo + self.cols].cpu()

    def outside_untouched(self):
        c = self.t.cpu().clone()
        c[:, self.lo:self.lo + self.cols] = SENT
        return bool((c == SENT).all())


def ints(g, *shape, lo=-8, hi=8, nonzero=False):
    if nonzero:
        return (torch.randint(1, hi + 1, shape, generator=g) * (2 * torch.randint(0, 2, shape, generator=g) - 1)).float()
    return torch.randint(lo, hi + 1, shape, generator=g).float()


def operands(regime, g, *shape, nonzero=False):
    return ints(g, *shape, nonzero=nonzero) if regime == "integers" else torch.randn(*shape, generator=g)


def compare(regime, got, ref, S, n, what):
    """integers: bit for bit with the float64 result cast to fp32 (+ 0.0: a zero is +0); floats: |got - ref| <= gamma_n S"""
    assert got.shape == ref.shape, what
    if regime == "integers":
        want = (ref + 0.0).to(torch.float32)
        assert bool((want.double() == ref).all()), what        # the float64 result is an integer below 2^24
        bad = bits(got) != bits(want)
        assert not bool(bad.any()), (what, int(bad.sum()), got[bad][:4], want[bad][:4])
    else:
        err = (got.double() - ref).abs()
        over = err > gamma(n) * S
        assert not bool(over.any()), (what, int(over.sum()), float((err / S.clamp_min(1e-300)).max()), gamma(n))


# ---------------------------------------------------------------- nerf_dense_fwd
def fwd_reference(x, w, bias, y_old, accumulate, relu):
    pre = x.double() @ w.double().T
    S = x.double().abs() @ w.double().abs().T
    if accumulate:
        pre, S = pre + y_old.double(), S + y_old.double().abs()
    if bias is not None:
        pre, S = pre + bias.double(), S + bias.double().abs()
    return (torch.relu(pre) if relu else pre), pre, S


@pytest.mark.parametrize("regime", ["integers", "floats"])
@pytest.mark.parametrize("P,K,N", SHAPES)
def test_dense_fwd(npa, dev, P, K, N, regime):
    """relu(y_old * accumulate + x w^T + bias) for accumulate x bias x relu, operands inside wider matrices."""
    hb = npa.hip_backend
    L = hb.lib()
    g = torch.Generator().manual_seed(1000 + P + K + N)
    for accumulate in (0, 1):
        for with_bias in (False, True):
            for relu in (0, 1):
                what = ("fwd", regime, P, K, N, accumulate, with_bias, relu)
                x = operands(regime, g, P, K, nonzero=True)
                w = operands(regime, g, N, K, nonzero=True)
                bias = operands(regime, g, N) if with_bias else None
                y_old = operands(regime, g, P, N)
                constructed = regime == "integers" and K >= 3 and P >= 2
                if constructed:         # rows 0 and 1, column 0: pre-activations exactly 0 and exactly -1
                    if with_bias:
                        bias[0] = float(torch.randint(-3, 4, (1,), generator=g))
                    y_old[0:2, 0] = ints(g, 2, lo=-3, hi=3)
                    w[0, 2] = 1.0
                    for r, target in ((0, 0.0), (1, -1.0)):
                        x[r] = 0.0
                        x[r, 0], x[r, 1] = w[0, 1], -w[0, 0]           # a cancelling nonzero pair
                        x[r, 2] = target - (float(bias[0]) if with_bias else 0.0) - (float(y_old[r, 0]) if accumulate else 0.0)
                    assert float(x.abs().max()) <= 8.0
                X, Wm = Wide(dev, P, K, 2, 3, x), Wide(dev, N, K, 1, 2, w)
                Y = Wide(dev, P, N, 3, 1, y_old if accumulate else None)
                b_dev = None if bias is None else bias.to(dev)
                hb._check(L.nerf_dense_fwd(X.ptr, X.ld, K, Wm.ptr, Wm.ld, None if bias is None else b_dev.data_ptr(), Y.ptr, Y.ld, N, P,
                                           accumulate, relu, hb._stream()), "nerf_dense_fwd")
                got = Y.inner()
                ref, pre, S = fwd_reference(x, w, bias, y_old, accumulate, relu)
                if constructed:
                    assert float(pre[0, 0]) == 0.0 and float(pre[1, 0]) == -1.0, what
                    if relu:
                        assert bits(got)[0, 0] == 0 and bits(got)[1, 0] == 0, (what, got[0:2, 0])      # +0, not -0
                compare(regime, got, ref, S, K + 2, what)
                assert Y.outside_untouched() and X.outside_untouched() and Wm.outside_untouched(), what
                assert torch.equal(X.inner(), x) and torch.equal(Wm.inner(), w), what
                if bias is not None:
                    assert torch.equal(b_dev.cpu(), bias), what


# ---------------------------------------------------------------- nerf_dense_dgrad
TINY = 2.0 ** -126          # the smallest positive normal fp32
ACT_VALUES = torch.tensor([0.0, -0.0, TINY, 1.0, -1.0])


def relu_outputs(g, P, K):
    """[P, K] of +0, -0, the smallest positive normal, 1 and -1 (each present when P * K >= 5), in a seeded order"""
    n = P * K
    return ACT_VALUES[torch.arange(n) % 5][torch.randperm(n, generator=g)].reshape(P, K).clone()


@pytest.mark.parametrize("regime", ["integers", "floats"])
@pytest.mark.parametrize("P,K,N", SHAPES)
def test_dense_dgrad(npa, dev, P, K, N, regime):
    """(dx_old * accumulate + dy w) where act > 0, +0 elsewhere, for accumulate x act in {None, given with ldact > K}."""
    hb = npa.hip_backend
    L = hb.lib()
    g = torch.Generator().manual_seed(2000 + P + K + N)
    for accumulate in (0, 1):
        for with_act in (False, True):
            what = ("dgrad", regime, P, K, N, accumulate, with_act)
            dy = operands(regime, g, P, N, nonzero=True)
            w = operands(regime, g, N, K, nonzero=True)
            dx_old = operands(regime, g, P, K)
            act = relu_outputs(g, P, K) if with_act else None
            DY, Wm = Wide(dev, P, N, 1, 2, dy), Wide(dev, N, K, 2, 1, w)
            DX = Wide(dev, P, K, 3, 2, dx_old if accumulate else None)
            A = Wide(dev, P, K, 2, 4, act) if with_act else None
            hb._check(L.nerf_dense_dgrad(DY.ptr, DY.ld, N, Wm.ptr, Wm.ld, DX.ptr, DX.ld, K, P, accumulate, A.ptr if with_act else None,
                                         A.ld if with_act else 0, hb._stream()), "nerf_dense_dgrad")
            got = DX.inner()
            val = dy.double() @ w.double()
            S = dy.double().abs() @ w.double().abs()
            if accumulate:
                val, S = val + dx_old.double(), S + dx_old.double().abs()
            if with_act:
                keep = act > 0
                assert bool((keep == ((bits(act) > 0) & (bits(act) < 0x7f800000))).all())      # strictly positive: not +0, not -0, not -1
                if P * K >= 5:
                    assert bool(keep.any()) and not bool(keep.all()) and bool((act == TINY).any())
                assert bool((bits(got)[~keep] == 0).all()), (what, "masked entries are +0")
                val =torch.where(keep, val, torch.zeros_like(val))         # the kernel stores 0.0f over the masked entries
            compare(regime, got, val, S, N + 2, what)
            assert DX.outside_untouched() and DY.outside_untouched() and Wm.outside_untouched(), what
            assert torch.equal(DY.inner(), dy) and torch.equal(Wm.inner(), w), what
            if with_act:
                assert A.outside_untouched() and bool((bits(A.inner()) == bits(act)).all()), what


# ---------------------------------------------------------------- nerf_dense_wgrad
WGRAD_K = {1: 3, 2047: 40, 2048: 3, 2049: 40, 5000: 3}         # K per P
WGRAD_N = (1, 3, 64, 65, 130)          # either side of the 64-column block of the column sum
SCRATCH_TAIL = 96


def run_wgrad(npa, dev, dy, x, dw_old, db_old, accumulate, with_bias, what):
    """one call on fresh buffers: (dw, dbias or None), after the checks of everything the call must leave alone"""
    hb = npa.hip_backend
    L = hb.lib()
    P, N = dy.shape
    K = x.shape[1]
    DY, X = Wide(dev, P, N, 2, 1, dy), Wide(dev, P, K, 1, 3, x)
    DW = Wide(dev, N, K, 3, 2, dw_old if accumulate else None)
    DB = Wide(dev, 1, N, 2, 2, db_old.reshape(1, N) if accumulate else None) if with_bias else None
    n_scr = L.nerf_dense_wgrad_scratch_floats(P, N)
    scratch = torch.full((n_scr + SCRATCH_TAIL,), SENT, dtype=torch.float32, device=dev) if with_bias else None
    hb._check(L.nerf_dense_wgrad(DY.ptr, DY.ld, N, X.ptr, X.ld, K, P, DW.ptr, DW.ld, DB.ptr if with_bias else None,
                                 scratch.data_ptr() if with_bias else None, accumulate, hb._stream()), "nerf_dense_wgrad")
    assert DW.outside_untouched() and DY.outside_untouched() and X.outside_untouched(), what
    assert torch.equal(DY.inner(), dy) and torch.equal(X.inner(), x), what
    if with_bias:
        assert DB.outside_untouched(), what
        assert bool((scratch[n_scr:].cpu() == SENT).all()), (what, "floats behind the scratch")
    return DW.inner(), (DB.inner().reshape(N) if with_bias else None)


@pytest.mark.parametrize("regime", ["integers", "floats"])
@pytest.mark.parametrize("P", sorted(WGRAD_K))
def test_dense_wgrad(npa, dev, P, regime):
    """dw (+)= dy^T x and dbias (+)= column sums of dy around the 2048-row block and the 64-column block; accumulate applies to both;
    dbias = NULL takes no scratch; two calls on the same inputs give the same bits (deterministic two-pass sum, no split-K atomics)."""
    K = WGRAD_K[P]
    g = torch.Generator().manual_seed(3000 + P)
    for N in WGRAD_N:
        dy = operands(regime, g, P, N, nonzero=True)
        x = operands(regime, g, P, K, nonzero=True)
        dw_old, db_old = operands(regime, g, N, K), operands(regime, g, N)
        ref_w, S_w = dy.double().T @ x.double(), dy.double().abs().T @ x.double().abs()
        ref_b, S_b = dy.double().sum(0), dy.double().abs().sum(0)
        for accumulate in (0, 1):
            rw, Sw, rb, Sb = ref_w, S_w, ref_b, S_b
            if accumulate:
                rw, Sw, rb, Sb = rw + dw_old.double(), Sw + dw_old.double().abs(), rb + db_old.double(), Sb + db_old.double().abs()
            for with_bias in (False, True):
                what = ("wgrad", regime, P, N, K, accumulate, with_bias)
                dw, db = run_wgrad(npa, dev, dy, x, dw_old, db_old, accumulate, with_bias, what)
                compare(regime, dw, rw, Sw, P + 2, what + ("dw",))
                if with_bias:
                    compare(regime, db, rb, Sb, P + 2, what + ("dbias",))
                    dw2, db2 = run_wgrad(npa, dev, dy, x, dw_old, db_old, accumulate, with_bias, what)
                    assert bool((bits(dw2) == bits(dw)).all()) and bool((bits(db2) == bits(db)).all()), (what, "run to run")


def test_dense_wgrad_two_column_ranges_of_one_dw(npa, dev):
    """The skip layer's weight gradient: two calls write disjoint column ranges of one dw (input part with the bias gradient, hidden
    part without) = one GEMM against the concatenated input."""
    hb = npa.hip_backend
    L = hb.lib()
    g = torch.Generator().manual_seed(77)
    P, N, K1, K2 = 2049, 65, 5, 40
    dy, x1, x2 = ints(g, P, N, nonzero=True), ints(g, P, K1, nonzero=True), ints(g, P, K2, nonzero=True)
    DY, X1, X2 = Wide(dev, P, N, 1, 1, dy), Wide(dev, P, K1, 2, 1, x1), Wide(dev, P, K2, 1, 2, x2)
    DW = Wide(dev, N, K1 + K2, 2, 3)
    db = torch.full((N,), float("nan"), device=dev)
    scratch = torch.empty(L.nerf_dense_wgrad_scratch_floats(P, N), dtype=torch.float32, device=dev)
    hb._check(L.nerf_dense_wgrad(DY.ptr, DY.ld, N, X1.ptr, X1.ld, K1, P, DW.ptr, DW.ld, db.data_ptr(), scratch.data_ptr(), 0, hb._stream()),
              "nerf_dense_wgrad")
    first = DW.inner()
    assert bool(torch.isnan(first[:, K1:]).all()) and not bool(torch.isnan(first[:, :K1]).any())         # the other range is not touched
    hb._check(L.nerf_dense_wgrad(DY.ptr, DY.ld, N, X2.ptr, X2.ld, K2, P, DW.ptr + 4 * K1, DW.ld, None, None, 0, hb._stream()),
              "nerf_dense_wgrad")
    ref = dy.double().T @ torch.cat([x1, x2], 1).double()
    compare("integers", DW.inner(), ref, None, P + 2, "skip-layer dw")
    compare("integers", db.cpu(), dy.double().sum(0), None, P + 2, "skip-layer dbias")
    assert DW.outside_untouched()


def test_dense_wgrad_scratch_floats(npa):
    L = npa.hip_backend.lib()
    for P in list(WGRAD_K) + [4096, 4097]:
        for N in WGRAD_N:
            assert L.nerf_dense_wgrad_scratch_floats(P, N) == -(-P // COLSUM_ROWS) * N, (P, N)
    for P, N in ((0, 5), (-1, 5), (5, 0), (5, -3), (0, 0)):
        assert L.nerf_dense_wgrad_scratch_floats(P, N) == 0, (P, N)


# ---------------------------------------------------------------- nerf_build_inputs
def bands_of(v, L):
    """float64 [n, 6 L]: (sin, cos) of the exact fp32 arguments v * 2^f, in get_embedder's column order"""
    out = []
    for f in range(L):
        a = v.double() * 2.0 ** f           # exact: the kernel's fp32 product with a power of two is too
        out += [torch.sin(a), torch.cos(a)]
    return torch.cat(out, 1) if out else v.new_zeros((v.shape[0], 0), dtype=torch.float64)


def check_encoding(got, v, L, what):
    """columns of one encoded 3-vector: identity bit for bit, then 2 L bands within the fused encoder's 2e-6"""
    assert bool((bits(got[:, :3]) == bits(v)).all()), (what, "identity columns")
    if L > 0:
        err = (got[:, 3:].double() - bands_of(v, L)).abs()
        assert float(err.max()) <= 2e-6, (what, float(err.max()), int(err.max(0).values.argmax()))


@pytest.mark.parametrize("views", ["none_stride8", "stride11", "stride13"])
@pytest.mark.parametrize("n_rays,S", [(1, 1), (3, 5), (129, 2), (52, 5)])
def test_build_inputs(npa, dev, n_rays, S, views):
    """x[p] = [enc(fl(o + fl(d z_p))) | enc(viewdir)] with ray p // S: the identity embedding, zero bands and frequency counts up
    to 16 (the guard accepts 24; no other test goes past 10); the view direction comes from the LAST three columns of a record (stride
    13: columns 8 and 9 hold junk); ldx = width + 3."""
    hb = npa.hip_backend
    L = hb.lib()
    use_viewdirs, stride = {"none_stride8": (0, 8), "stride11": (1, 11), "stride13": (1, 13)}[views]
    g = torch.Generator().manual_seed(n_rays * 31 + S)
    P = n_rays * S
    rays = torch.randn(n_rays, stride, generator=g)
    rays[:, 0:3] = (torch.rand(n_rays, 3, generator=g) * 2 - 1) * 1.5
    rays[:, 3:6] = torch.nn.functional.normalize(torch.randn(n_rays, 3, generator=g), dim=-1)
    vd = torch.nn.functional.normalize(torch.randn(n_rays, 3, generator=g), dim=-1)
    if use_viewdirs:
        rays[:, 8:] = 1e30          # stride 13: columns 8 and 9 (and 10, overwritten below) are junk
        rays[:, stride - 3:] = vd
    z = torch.rand(n_rays, S, generator=g) * 2.5          # |o + d z| up to about 4, as the scenes have
    pts = (rays[:, None, 0:3] + rays[:, None, 3:6] * z[:, :, None]).reshape(P, 3)       # fp32: one product, one sum, each rounded
    assert float(pts.abs().max()) < 5.2 and (P < 8 or float(pts.abs().max()) > 1.0)
    vd_rows = vd[:, None, :].expand(n_rays, S, 3).reshape(P, 3)
    rays_d, z_d = rays.to(dev), z.to(dev)
    for multires in (-1, 0, 1, 6, 10, 16):
        for multires_views in ((-1, 0, 2, 4) if use_viewdirs else (4,)):         # (read only with view directions)
            what = ("build_inputs", n_rays, S, views, multires, multires_views)
            cx = 3 if multires < 0 else 3 + 6 * multires
            cd = 0 if not use_viewdirs else (3 if multires_views < 0 else 3 + 6 * multires_views)
            X = Wide(dev, P, cx + cd, 1, 2)
            hb._check(L.nerf_build_inputs(rays_d.data_ptr(), stride, z_d.data_ptr(), n_rays, S, multires, multires_views, use_viewdirs,
                                          X.ptr, X.ld, hb._stream()), "nerf_build_inputs")
            got = X.inner()
            assert X.ld == cx + cd + 3 and X.outside_untouched(), what
            assert not bool(torch.isnan(got).any()), (what, "a column of the row was not written")
            check_encoding(got[:, :cx], pts, max(multires, 0), what + ("xyz",))
            if use_viewdirs:
                check_encoding(got[:, cx:], vd_rows, max(multires_views, 0), what + ("dir",))
    assert torch.equal(rays_d.cpu(), rays) and torch.equal(z_d.cpu(), z)


# ---------------------------------------------------------------- the empty batch
def test_empty_batch_at_the_c_level(npa, dev):
    """P == 0 / n_rays == 0 is a valid call (include/nerf_hip.h): the row operands may be NULL as an empty tensor's pointer is, and the
    weight gradient of no rows is zeros (accumulate = 0) or what was there (accumulate = 1)."""
    hb = npa.hip_backend
    L = hb.lib()
    assert torch.empty((0, 5), device=dev).data_ptr() == 0
    N, K = 5, 7
    Wm = Wide(dev, N, K, 1, 2, ints(torch.Generator().manual_seed(1), N, K))
    st = hb._stream()
    assert L.nerf_dense_fwd(None, K + 1, K, Wm.ptr, Wm.ld, None, None, N + 2, N, 0, 0, 1, st) == 0
    assert L.nerf_dense_dgrad(None, N + 1, N, Wm.ptr, Wm.ld, None, K + 3, K, 0, 0, None, 0, st) == 0
    assert L.nerf_build_inputs(None, 11, None, 0, 5, 10, 4, 1, None, 90, st) == 0
    old_w, old_b = ints(torch.Generator().manual_seed(2), N, K), ints(torch.Generator().manual_seed(3), 1, N)
    for accumulate in (0, 1):
        for with_bias in (False, True):
            DW, DB = Wide(dev, N, K, 2, 3, old_w), Wide(dev, 1, N, 1, 1, old_b)
            assert L.nerf_dense_wgrad(None, N, N, None, K, K, 0, DW.ptr, DW.ld, DB.ptr if with_bias else None, None, accumulate, st) == 0
            assert DW.outside_untouched() and DB.outside_untouched(), (accumulate, with_bias)
            want_w = old_w if accumulate else torch.zeros(N, K)
            want_b = old_b if accumulate or not with_bias else torch.zeros(1, N)
            assert bool((bits(DW.inner()) == bits(want_w)).all()) and bool((bits(DB.inner()) == bits(want_b)).all()), (accumulate, with_bias)


@pytest.mark.parametrize("name", ["narrow_shallow", "no_viewdirs_small"])
def test_empty_batch_through_the_module(npa, dev, name):
    """net(x [0, C]) returns [0, 4 | output_ch]; its backward leaves exact zeros in every parameter that gets a gradient at P > 0, as
    the reference's nn.Linear stack does, and None in views_linears without view directions."""
    arch = ARCHS[name]
    net, _ = _net(npa, dev, arch, 31)
    C = arch["input_ch"] + arch["input_ch_views"]
    out = net(torch.zeros(0, C, device=dev))
    assert out.shape == (0, 4 if arch["use_viewdirs"] else arch["output_ch"]) and out.device.type == "cuda"
    out.sum().backward()
    some = net(torch.ones(3, C, device=dev))
    want = {k for k, p_ in zip(dict(net.named_parameters()), torch.autograd.grad(some.sum(), list(net.parameters()), allow_unused=True))
            if p_ is not None}
    assert len(want) >= 2 * arch["D"] + 2
    for k, p in net.named_parameters():
        if k in want:
            assert p.grad is not None and p.grad.shape == p.shape and bool((bits(p.grad) == 0).all()), k
        else:
            assert k.startswith("views_linears") and not arch["use_viewdirs"] and p.grad is None, k


@pytest.mark.parametrize("name", ["narrow_shallow", "no_viewdirs_small"])
def test_empty_batch_through_render_rays(npa, dev, name):
    """render_rays on 0 rays: the keys, their order and the trailing shapes of the 96-ray call, 0 rows, on the device; a backward
    leaves zero gradients in both networks."""
    arch = ARCHS[name]
    net_c, _ = _net(npa, dev, arch, 31)
    net_f, _ = _net(npa, dev, arch, 32)
    cols = 11 if arch["use_viewdirs"] else 8
    kw = dict(N_samples=8, N_importance=8, network_fine=net_f, retraw=True)
    full = npa.render_rays(orc.synthetic_rays(96, seed=3)[:, :cols].contiguous().to(dev), net_c, None, **kw)
    (full["rgb_map"].sum() + full["rgb0"].sum()).backward()
    want = [{k for k, p in net.named_parameters() if p.grad is not None} for net in (net_c, net_f)]
    for net in (net_c, net_f):
        net.zero_grad(set_to_none=True)
    out = npa.render_rays(torch.zeros(0, cols, device=dev), net_c, None, **kw)
    assert list(out) == list(full) == ["rgb0", "disp0", "acc0", "z_std", "rgb_map", "disp_map", "acc_map", "raw"]
    for k, v in out.items():
        assert v.shape == (0,) + full[k].shape[1:] and v.device.type == "cuda" and v.dtype == torch.float32, (k, v.shape)
    (out["rgb_map"].sum() + out["rgb0"].sum()).backward()
    for net, names in zip((net_c, net_f), want):
        assert len(names) >= 2 * arch["D"] + 2
        for k, p in net.named_parameters():
            if k in names:
                assert p.grad is not None and bool((bits(p.grad) == 0).all()), k
            else:
                assert p.grad is None, k
    assert list(npa.render_rays(torch.zeros(0, cols, device=dev), net_c, None, N_samples=8, N_importance=0)) == ["rgb_map", "disp_map", "acc_map"]


# ---------------------------------------------------------------- DenseNeRF.query in slices
def test_query_does_not_depend_on_its_slicing(npa, dev, monkeypatch):
    """Without gradients query() evaluates QUERY_SLICE_POINTS points at a time.  Small-integer weights, rays and depths make every
    layer exact, so the sliced query, the unsliced one (gradients enabled) and the float64 layer stack agree bit for bit: the
    row-to-ray mapping holds across slice boundaries."""
    import nerf_pytorch_amd.dense as dense
    assert dense.QUERY_SLICE_POINTS == 1 << 20
    monkeypatch.setattr(dense, "QUERY_SLICE_POINTS", 1000)
    S = 5
    per_slice = 1000 // S
    n = 3 * per_slice + 7
    g = torch.Generator().manual_seed(9)
    net = npa.NeRF(D=2, W=8, input_ch=3, input_ch_views=3, output_ch=4, skips=[], use_viewdirs=True).to(dev)
    assert type(net).__name__ == "DenseNeRF" and (net.multires, net.multires_views) == (-1, -1)
    P = {k: ints(g, *v.shape, lo=-1, hi=1) for k, v in net.state_dict().items()}
    net.load_state_dict(P)
    rays = torch.cat([ints(g, n, 3, lo=-2, hi=2), ints(g, n, 3, lo=-1, hi=1), torch.zeros(n, 2), ints(g, n, 3, lo=-1, hi=1)], 1)
    z = ints(g, n, S, lo=0, hi=4)
    rows = []
    apply = dense._DenseMLP.apply
    monkeypatch.setattr(dense._DenseMLP, "apply", lambda *a: (rows.append(a[1].shape[0]), apply(*a))[1])
    with torch.no_grad():
        sliced = net.query(rays.to(dev), z.to(dev))
    assert rows == [per_slice * S] * 3 + [7 * S], rows
    del rows[:]
    whole = net.query(rays.to(dev), z.to(dev))
    assert rows == [n * S] and whole.requires_grad and not sliced.requires_grad
    assert sliced.shape == whole.shape == (n, S, 4)
    assert bool((bits(sliced) == bits(whole)).all())
    # the float64 layer stack (run_nerf_helpers.py:96-119) on the points o + d z and the broadcast directions
    W = {k: v.double() for k, v in P.items()}
    lin = lambda h, nm: h @ W[nm + ".weight"].T + W[nm + ".bias"]
    pts = (rays[:, None, 0:3] + rays[:, None, 3:6] * z[:, :, None]).double()
    dirs = rays[:, None, 8:11].expand(n, S, 3).double()
    h = torch.relu(lin(torch.relu(lin(pts, "pts_linears.0")), "pts_linears.1"))
    hv = torch.relu(lin(torch.cat([lin(h, "feature_linear"), dirs], -1), "views_linears.0"))
    ref = torch.cat([lin(hv, "rgb_linear"), lin(h, "alpha_linear")], -1)
    assert float(ref.abs().max()) < 2 ** 24 and float(ref.abs().max()) > 8
    assert torch.equal(sliced.cpu().double(), ref)
