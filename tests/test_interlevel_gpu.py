"""GPU tests (-m gpu) of the interlevel-loss kernels against their definition, and of interlevel_loss as a public piece.

THE DEFINITION is render.interlevel_loss_reference, run in float64 on the fp32 inputs the kernel sees (the comparisons of fp32 depths are
exact in any precision, so kernel and definition see the same overlap pattern).  THE YARDSTICK of the tolerance is the same function
run in float32 on the same inputs against its own float64 run: the kernel's largest absolute error over the case set may be at most
4 x the yardstick's (the kernel adds the same terms; only the order of the reductions differs), and never needs to be below
2^-22 * max(1, the largest |value| of the float64 run) -- one ulp of it --, taken separately for the loss and for the gradient (an
entry of which is a sum over many target intervals of terms up to 2 each)."""
import pytest
import torch

import nerf_oracle as orc
from test_gpu_occupancy import bits_equal
from test_gpu_parity import datapath, dev, maxdiff, nets, npa  # noqa: F401  (fixtures)
from test_interlevel_cpu import KINDS, case, definition

pytestmark = pytest.mark.gpu

F64 = torch.float64
SIZES = [(1, 1), (2, 3), (63, 65), (65, 64), (64, 192), (257, 130)]        # (P, S): the lane strides' boundaries at 64 and 256
COUNTS = [1, 5, 130]


@pytest.fixture(scope="module")
def measured(npa, dev):
    """every (P, S, n) case once: kernel and yardstick errors of loss and gradient against the float64 definition"""
    hb = npa.hip_backend
    rows = []
    for P, S in SIZES:
        for n in COUNTS:
            wp, zp, w, z = case(P, S, n, seed=1000 * P + S + n)
            g = 2.0 * torch.rand(n, generator=torch.Generator().manual_seed(P + S + n)) - 1.0      # |upstream| <= 1
            g[1::3] = 0.0
            L64, G64 = definition(wp, zp, w, z, F64, g)
            L32, G32 = definition(wp, zp, w, z, torch.float32, g)
            wpd, zpd, wd, zd, gd = (t.to(dev) for t in (wp, zp, w, z, g))
            loss = hb.interlevel(wpd, zpd, wd, zd)
            dwp = hb.interlevel_bwd(wpd, zpd, wd, zd, gd)
            rows.append(dict(P=P, S=S, n=n, wp=wpd, zp=zpd, w=wd, z=zd, g=gd, loss=loss, dwp=dwp, L64=L64, G64=G64,
                             eL=maxdiff(loss, L64), eG=maxdiff(dwp, G64), yL=maxdiff(L32, L64), yG=maxdiff(G32, G64)))
    return rows


def test_kernels_against_the_definition(measured):
    eL, eG = max(r["eL"] for r in measured), max(r["eG"] for r in measured)
    yL, yG = max(r["yL"] for r in measured), max(r["yG"] for r in measured)
    top_L, top_G = max(float(r["L64"].abs().max()) for r in measured), max(float(r["G64"].abs().max()) for r in measured)
    print(f"\ninterlevel kernels vs the float64 definition over {len(measured)} cases: loss {eL:.3e} (float32 definition {yL:.3e}, largest "
          f"value {top_L:.3e}), gradient {eG:.3e} (float32 definition {yG:.3e}, largest value {top_G:.3e})")
    for r in measured:
        print(f"  P={r['P']} S={r['S']} n={r['n']}: loss {r['eL']:.3e} ({r['yL']:.3e}), gradient {r['eG']:.3e} ({r['yG']:.3e})")
        assert r["loss"].shape == (r["n"],) and r["dwp"].shape == (r["n"], r["P"])
        assert bool(torch.isfinite(r["loss"]).all()) and bool(torch.isfinite(r["dwp"]).all()), (r["P"], r["S"], r["n"])
        assert float(r["loss"].min()) >= 0.0 and float((r["dwp"] * r["g"][:, None]).max()) <= 0.0
    assert eL <= max(4.0 * yL, 2.0 ** -22 * max(1.0, top_L)), (eL, yL, top_L)
    assert eG <= max(4.0 * yG, 2.0 ** -22 * max(1.0, top_G)), (eG, yG, top_G)
    assert top_L > 0.1 and top_G > 1.0          # the hinge is open somewhere


def test_the_special_rows_are_exact(measured):
    """the envelope proposal and an all-zero target give exactly 0 in loss and gradient; a zero upstream gives a zero row; an all-zero
    proposal leaves every target weight uncovered"""
    seen = set()
    for r in measured:
        for i in range(r["n"]):
            kind = KINDS[i % len(KINDS)]
            if kind in ("envelope", "all-zero target"):
                assert float(r["loss"][i]) == 0.0 and not bool(r["dwp"][i].any()), (r["P"], r["S"], r["n"], i, kind)
                seen.add(kind)
            if float(r["g"][i]) == 0.0:
                assert not bool(r["dwp"][i].any()), (r["P"], r["S"], r["n"], i, kind)
            if kind == "all-zero proposal":
                w = r["w"][i].double()
                assert float(r["loss"][i]) == pytest.approx(float((w * w / (w + 1e-7)).sum()), rel=1e-5, abs=0)
    assert seen == {"envelope", "all-zero target"}


def test_accumulate_out_and_two_runs(npa, dev, measured):
    hb = npa.hip_backend
    for r in measured:
        if r["n"] != 130:
            continue
        n, P = r["n"], r["P"]
        args = (r["wp"], r["zp"], r["w"], r["z"])
        pre = torch.randn(n, P, generator=torch.Generator().manual_seed(P)).to(dev)
        out = pre.clone()
        ret = hb.interlevel_bwd(*args, r["g"], out=out, accumulate=True)
        assert ret is out and bits_equal(out, pre + r["dwp"])         # one fp32 addition per entry
        fresh = torch.full((n, P), float("nan"), device=dev)
        hb.interlevel_bwd(*args, r["g"], out=fresh)
        assert bits_equal(fresh, r["dwp"])                              # the same inputs, the same bits
        assert bits_equal(hb.interlevel(*args), r["loss"])
        with pytest.raises(hb.NerfHipError, match="accumulate"):
            hb.interlevel_bwd(*args, r["g"], accumulate=True)
        with pytest.raises(hb.NerfHipError, match="is not"):
            hb.interlevel_bwd(*args, r["g"], out=fresh[:, :-1].contiguous() if P > 1 else fresh[:-1])


def test_the_largest_rows(npa, dev):
    """P = S = 4096, the limit (64 KiB of LDS in the adjoint), nested and independent depths: against the definition at the module's
    tolerance (the [3, 4096, 4096] mask on the device)"""
    hb = npa.hip_backend
    wp, zp, w, z = (t[:3].to(dev) for t in case(4096, 4096, 3, seed=9))
    g = torch.tensor([1.0, -0.5, 0.75], device=dev)
    L64, G64 = definition(wp, zp, w, z, F64, g)
    L32, G32 = definition(wp, zp, w, z, torch.float32, g)
    loss, dwp = hb.interlevel(wp, zp, w, z), hb.interlevel_bwd(wp, zp, w, z, g)
    print(f"\nP = S = 4096: loss {maxdiff(loss, L64):.3e} (float32 definition {maxdiff(L32, L64):.3e}), gradient {maxdiff(dwp, G64):.3e} "
          f"(float32 definition {maxdiff(G32, G64):.3e})")
    assert maxdiff(loss, L64) <= max(4.0 * maxdiff(L32, L64), 2.0 ** -22 * max(1.0, float(L64.abs().max())))
    assert maxdiff(dwp, G64) <= max(4.0 * maxdiff(G32, G64), 2.0 ** -22 * max(1.0, float(G64.abs().max())))


def test_interlevel_loss_composes_with_raw2outputs(npa, dev, nets, monkeypatch):
    """torch.autograd.grad through two raw2outputs nodes -> interlevel_loss on raw from the fixture networks (48 rays, 64 coarse and 192
    refined depths) against the same chain with interlevel_loss_reference in float64: the loss and d loss / d proposal weights at the
    kernel tolerance measured here on these inputs; the target side gets no gradient; leading shapes; no launch without an upstream"""
    hb = npa.hip_backend
    nc, nf, _, _ = nets
    n, P, n_f = 48, 64, 128
    rays = orc.synthetic_rays(n, seed=12).to(dev)
    rnd = orc.synthetic_randoms(n, P, n_f, seed=5)
    z_c = hb.sample_coarse(rays, torch.linspace(0.0, 1.0, P, device=dev), False, rnd["t_rand"].to(dev))
    query = lambda z, net: npa.run_network(rays[:, None, 0:3] + rays[:, None, 3:6] * z[:, :, None], rays[:, 8:11], net, None, None)
    with torch.no_grad():
        raw_c0 = query(z_c, nc)
        raw_c0[..., 3] -= 2.0       # a thinner coarse histogram: the hinge opens
        w_c0 = npa.raw2outputs(raw_c0, z_c, rays[:, 3:6], 0.0, True)[3]
        z_f = hb.sample_fine(z_c, w_c0.contiguous(), n_f, rnd["u"].to(dev), None)[0]
        raw_f0 = query(z_f, nf)
    up = (2.0 * torch.rand(n, generator=torch.Generator().manual_seed(2)) - 1.0).to(dev)

    def run(fn, dtype):
        raw_c, raw_f = raw_c0.clone().requires_grad_(True), raw_f0.clone().requires_grad_(True)
        w_c = npa.raw2outputs(raw_c, z_c, rays[:, 3:6], 0.0, True)[3]
        w_f = npa.raw2outputs(raw_f, z_f, rays[:, 3:6], 0.0, True)[3]
        loss = fn(w_c.to(dtype), z_c, w_f.to(dtype), z_f)
        d_w, d_raw_c, d_raw_f = torch.autograd.grad((loss * up.to(dtype)).sum(), (w_c, raw_c, raw_f), allow_unused=True)
        return loss.detach(), d_w, d_raw_c, d_raw_f, w_c.detach(), w_f.detach()
    L, d_w, d_raw_c, d_raw_f, w_c, w_f = run(npa.interlevel_loss, torch.float32)
    L64, d_w64, d_raw_c64, d_raw_f64, _, _ = run(npa.interlevel_loss_reference, F64)
    L32, d_w32, _, _, _, _ = run(npa.interlevel_loss_reference, torch.float32)
    assert float((L64 > 0).double().mean()) >= 0.5 and d_raw_f is None and d_raw_f64 is None
    tol_L = max(4.0 * maxdiff(L32, L64), 2.0 ** -22 * max(1.0, float(L64.abs().max())))
    tol_G = max(4.0 * maxdiff(d_w32, d_w64), 2.0 ** -22 * max(1.0, float(d_w64.abs().max())))
    amp = 2.0 * float(((z_c[:, 1:] - z_c[:, :-1]) * rays[:, 3:6].norm(dim=-1, keepdim=True)).max())
    print(f"\ninterlevel_loss after raw2outputs: loss {maxdiff(L, L64):.3e} (bound {tol_L:.3e}), d_proposal_weights {maxdiff(d_w, d_w64):.3e} "
          f"(bound {tol_G:.3e}), d_raw {maxdiff(d_raw_c, d_raw_c64):.3e} (bound {tol_G * max(1.0, amp):.3e})")
    assert L.shape == (n,) and L.dtype == torch.float32
    assert maxdiff(L, L64) <= tol_L and maxdiff(d_w, d_w64) <= tol_G
    assert maxdiff(d_raw_c, d_raw_c64) <= tol_G * max(1.0, amp) and float(d_raw_c64.abs().max()) > 0
    # leading shape [4, 12] -> [4, 12]
    v = lambda t: t.view(4, 12, t.shape[-1])
    assert bits_equal(npa.interlevel_loss(v(w_c), v(z_c), v(w_f), v(z_f)).reshape(-1), L)
    # an upstream of None launches nothing
    monkeypatch.setattr(hb, "interlevel_bwd", lambda *a, **k: pytest.fail("interlevel_bwd launched without an upstream"))
    raw = raw_c0.clone().requires_grad_(True)
    rgb, _, _, w_, _ = npa.raw2outputs(raw, z_c, rays[:, 3:6], 0.0, True)
    unused = npa.interlevel_loss(w_, z_c, w_f, z_f)
    (g,) = torch.autograd.grad(rgb.sum() + w_.sum(), raw)
    assert unused.requires_grad and bool(torch.isfinite(g).all())
