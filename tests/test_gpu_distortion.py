"""GPU tests (-m gpu) of the distortion-loss kernels against their definition, and of distortion_loss as a public piece.

THE DEFINITION is render.distortion_loss_reference, run in float64 on the fp32 inputs the kernel sees.  THE YARDSTICK of the tolerance
is the same function run in float32 on the same inputs against its own float64 run: the kernel's largest absolute error over the case
set may be at most 4 x the yardstick's (the wave scan sums in another order, not more terms), and never needs to be below 2^-22 -- one
ulp of the largest value the loss (sum w <= 1, m in [0, 1]: L <= 4/3) or a gradient entry (<= 8/3) can take."""
import pytest
import torch

import nerf_oracle as orc
import nerf_pytorch_amd
from test_distortion_cpu import FAR, NEAR, families
from test_gpu_occupancy import bits_equal
from test_gpu_parity import datapath, dev, maxdiff, nets, npa  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

F64 = torch.float64
FLOOR = 2.0 ** -22
SIZES = [1, 2, 63, 64, 65, 192, 257]        # the lane-segment boundaries C = 1 -> 2 (64 | 65) and 4 -> 5 (257)
COUNTS = [1, 5, 130]
KINDS = ("surface", "all zero", "one weight", "duplicated depths", "far == near", "fog", "spikes", "padded tail")


def case(S, n, seed):
    """fp32 (w [n, S], z [n, S] non-decreasing, near_far [n, 2]) on the CPU: row i is of kind KINDS[i % 8]"""
    k = -(-n // len(KINDS))
    if S >= 2:
        z3, w3 = families(k, S, seed)
    else:
        g = torch.Generator().manual_seed(seed)
        z3 = NEAR + (FAR - NEAR) * torch.rand(3 * k, 1, generator=g, dtype=F64)
        w3 = torch.rand(3 * k, 1, generator=g, dtype=F64)
    fam = {"surface": (z3[:k], w3[:k]), "fog": (z3[k:2 * k], w3[k:2 * k]), "spikes": (z3[2 * k:], w3[2 * k:])}
    z, w = torch.empty(n, S, dtype=F64), torch.empty(n, S, dtype=F64)
    nf = torch.tensor([[NEAR, FAR]], dtype=F64).repeat(n, 1)
    for i in range(n):
        kind, j = KINDS[i % len(KINDS)], i // len(KINDS)
        zi, wi = (t[j].clone() for t in fam.get(kind, fam["fog"]))
        if kind == "all zero":
            wi.zero_()
        elif kind == "one weight":
            keep = (7 * j + 3) % S
            wi = torch.where(torch.arange(S) == keep, torch.full_like(wi, 0.8), torch.zeros_like(wi))
        elif kind == "duplicated depths":           # every second depth repeats its predecessor
            zi[1::2] = zi[0::2][:zi[1::2].numel()].clone()
        elif kind == "far == near":
            nf[i, 1] = nf[i, 0]
        elif kind == "padded tail":                 # the march's padding: the tail repeats one depth with w = 0
            cut = max(S // 3, 1)
            zi[cut:] = zi[cut - 1]
            wi[cut:] = 0.0
        z[i], w[i] = zi, wi
    assert bool((z[:, 1:] >= z[:, :-1]).all())
    return w.float(), z.float(), nf.float()


def reference(w, z, nf, g, dtype, device="cpu"):
    """(loss [n], d (loss . g) / d w [n, S]) of the definition in `dtype`, as float64 tensors (plain torch on `device`)"""
    w, z, nf, g = (t.to(device) for t in (w, z, nf, g))
    w_ = w.to(dtype).requires_grad_(True)
    loss = nerf_pytorch_amd.distortion_loss_reference(w_, z.to(dtype), nf[:, 0].to(dtype), nf[:, 1].to(dtype))
    (grad,) = torch.autograd.grad((loss * g.to(dtype)).sum(), w_)
    return loss.detach().double(), grad.double()


@pytest.fixture(scope="module")
def measured(npa, dev):
    """every (S, n) case once: kernel and yardstick errors of loss and gradient against the float64 definition"""
    hb = npa.hip_backend
    rows = []
    for S in SIZES:
        for n in COUNTS:
            w, z, nf = case(S, n, seed=1000 * S + n)
            g = 2.0 * torch.rand(n, generator=torch.Generator().manual_seed(S + n)) - 1.0      # |upstream| <= 1: the floor's premise
            g[1::3] = 0.0
            L64, G64 = reference(w, z, nf, g, F64)
            L32, G32 = reference(w, z, nf, g, torch.float32)
            wd, zd, nfd, gd = (t.to(dev) for t in (w, z, nf, g))
            loss = hb.distortion(wd, zd, nfd)
            dw = hb.distortion_bwd(wd, zd, nfd, gd)
            rows.append(dict(S=S, n=n, w=wd, z=zd, nf=nfd, g=gd, loss=loss, dw=dw, L64=L64, G64=G64,
                             eL=maxdiff(loss, L64), eG=maxdiff(dw, G64), yL=maxdiff(L32, L64), yG=maxdiff(G32, G64)))
    return rows


def test_kernels_against_the_definition(measured):
    eL, eG = max(r["eL"] for r in measured), max(r["eG"] for r in measured)
    yL, yG = max(r["yL"] for r in measured), max(r["yG"] for r in measured)
    print(f"\ndistortion kernels vs the float64 definition over {len(measured)} cases: loss {eL:.3e} (float32 definition {yL:.3e}), "
          f"gradient {eG:.3e} (float32 definition {yG:.3e})")
    for r in measured:
        assert r["loss"].shape == (r["n"],) and r["dw"].shape == (r["n"], r["S"])
        assert bool(torch.isfinite(r["loss"]).all()) and bool(torch.isfinite(r["dw"]).all()), (r["S"], r["n"])
    assert eL <= max(4.0 * yL, FLOOR), (eL, yL)
    assert eG <= max(4.0 * yG, FLOOR), (eG, yG)


def test_the_special_rows_are_exact(measured):
    """S = 1, all-zero weights and far == near give exactly 0 in loss and gradient; a zero upstream gives a zero row"""
    for r in measured:
        kinds = [KINDS[i % len(KINDS)] for i in range(r["n"])]
        for i, kind in enumerate(kinds):
            if r["S"] == 1 or kind in ("all zero", "far == near"):
                assert float(r["loss"][i]) == 0.0, (r["S"], r["n"], i, kind)
            if kind == "far == near" or float(r["g"][i]) == 0.0:
                assert not bool(r["dw"][i].any()), (r["S"], r["n"], i, kind)


def test_accumulate_out_and_the_ray_record_addressing(npa, dev, measured):
    hb = npa.hip_backend
    for r in measured:
        if r["n"] != 130 or r["S"] not in (1, 65, 257):
            continue
        n, S = r["n"], r["S"]
        pre = torch.randn(n, S, generator=torch.Generator().manual_seed(S)).to(dev)
        out = pre.clone()
        ret = hb.distortion_bwd(r["w"], r["z"], r["nf"], r["g"], out=out, accumulate=True)
        assert ret is out and bits_equal(out, pre + r["dw"])         # one fp32 addition per entry
        fresh = torch.full((n, S), float("nan"), device=dev)
        hb.distortion_bwd(r["w"], r["z"], r["nf"], r["g"], out=fresh)
        assert bits_equal(fresh, r["dw"])
        # near / far inside 11-column ray records, and one pair for all rays (stride 0)
        rays = torch.randn(n, 11, generator=torch.Generator().manual_seed(3)).to(dev)
        rays[:, 6:8] = r["nf"]
        assert bits_equal(hb.distortion(r["w"], r["z"], rays, nf_stride=11, nf_offset=6), r["loss"])
        assert bits_equal(hb.distortion_bwd(r["w"], r["z"], rays, r["g"], nf_stride=11, nf_offset=6), r["dw"])
        same = torch.tensor([NEAR, FAR], device=dev)
        plain = [i for i in range(n) if KINDS[i % len(KINDS)] != "far == near"]
        assert bits_equal(hb.distortion(r["w"], r["z"], same, nf_stride=0)[plain], r["loss"][plain])
        with pytest.raises(hb.NerfHipError, match="too few"):
            hb.distortion(r["w"], r["z"], rays[:-1], nf_stride=11, nf_offset=6)
        with pytest.raises(hb.NerfHipError, match="accumulate"):
            hb.distortion_bwd(r["w"], r["z"], r["nf"], r["g"], accumulate=True)


def test_the_largest_row(npa, dev):
    """S = 4096, the slot limit (64 samples per lane, 64 KiB of LDS in the adjoint): against the definition at the module's tolerance"""
    hb = npa.hip_backend
    z, w = families(1, 4096, seed=9)
    w, z = w.float(), z.float()
    nf = torch.tensor([[NEAR, FAR]]).repeat(3, 1)
    g = torch.tensor([1.0, -0.5, 0.75])
    L64, G64 = reference(w, z, nf, g, F64, dev)          # (a [3, 4096, 4096] tensor per step: on the device)
    L32, G32 = reference(w, z, nf, g, torch.float32, dev)
    loss = hb.distortion(w.to(dev), z.to(dev), nf.to(dev))
    dw = hb.distortion_bwd(w.to(dev), z.to(dev), nf.to(dev), g.to(dev))
    print(f"\nS = 4096: loss {maxdiff(loss, L64):.3e} (float32 definition {maxdiff(L32, L64):.3e}), gradient {maxdiff(dw, G64):.3e} "
          f"(float32 definition {maxdiff(G32, G64):.3e})")
    assert maxdiff(loss, L64) <= max(4.0 * maxdiff(L32, L64), FLOOR)
    assert maxdiff(dw, G64) <= max(4.0 * maxdiff(G32, G64), FLOOR)


def test_distortion_loss_composes_with_raw2outputs(npa, dev, nets, monkeypatch):
    """torch.autograd.grad through raw2outputs -> distortion_loss on raw from a real network (48 rays x 64 samples) against the same
    chain with distortion_loss_reference in float64: the loss and d loss / d weights at the kernel tolerance (the yardstick measured
    here, on these inputs); d loss / d raw through the compositing's adjoint, which both chains share, at that tolerance times
    sum_k |d w_k / d raw_i| <= 2 dist_i |d| (the finite distances), the amplification of an error in d_weights."""
    hb = npa.hip_backend
    nc = nets[0]
    n, S = 48, 64
    rays = orc.synthetic_rays(n, seed=12).to(dev)
    rnd = orc.synthetic_randoms(n, S, 128, seed=5)
    z = hb.sample_coarse(rays, torch.linspace(0.0, 1.0, S, device=dev), False, rnd["t_rand"].to(dev))
    with torch.no_grad():
        raw0 = npa.run_network(rays[:, None, 0:3] + rays[:, None, 3:6] * z[:, :, None], rays[:, 8:11], nc, None, None)
    near, far = rays[:, 6], rays[:, 7]
    up = (2.0 * torch.rand(n, generator=torch.Generator().manual_seed(2)) - 1.0).to(dev)

    def run(fn, dtype):
        raw = raw0.clone().requires_grad_(True)
        w = npa.raw2outputs(raw, z, rays[:, 3:6], 0.0, True)[3]
        loss = fn(w.to(dtype), z.to(dtype), near.to(dtype), far.to(dtype))
        d_w, d_raw = torch.autograd.grad((loss * up.to(dtype)).sum(), (w, raw))
        return loss.detach(), d_w, d_raw, w.detach()
    L, d_w, d_raw, w = run(npa.distortion_loss, torch.float32)
    L64, d_w64, d_raw64, _ = run(npa.distortion_loss_reference, F64)
    L32, d_w32, _, _ = run(npa.distortion_loss_reference, torch.float32)
    assert float(w.sum(-1).max()) > 0.5 and float(L64.max()) > 1e-3          # a scene with something in it
    tol_L = max(4.0 * maxdiff(L32, L64), FLOOR)
    tol_G = max(4.0 * maxdiff(d_w32, d_w64), FLOOR)
    amp = 2.0 * float(((z[:, 1:] - z[:, :-1]) * rays[:, 3:6].norm(dim=-1, keepdim=True)).max())
    print(f"\ndistortion_loss after raw2outputs: loss {maxdiff(L, L64):.3e} (bound {tol_L:.3e}), d_weights {maxdiff(d_w, d_w64):.3e} "
          f"(bound {tol_G:.3e}), d_raw {maxdiff(d_raw, d_raw64):.3e} (bound {tol_G * max(1.0, amp):.3e})")
    assert L.shape == (n,) and L.dtype == torch.float32
    assert maxdiff(L, L64) <= tol_L and maxdiff(d_w, d_w64) <= tol_G
    assert maxdiff(d_raw, d_raw64) <= tol_G * max(1.0, amp) and float(d_raw64.abs().max()) > 0
    # Python numbers for near / far: one pair for all rays
    zz = z.clone()
    assert maxdiff(npa.distortion_loss(w, zz, 2.0, 6.0), npa.distortion_loss_reference(w.double(), zz.double(), 2.0, 6.0)) <= tol_L
    # leading shape [4, 12] -> [4, 12]
    assert bits_equal(npa.distortion_loss(w.view(4, 12, S), z.view(4, 12, S), near.view(4, 12), far.view(4, 12)).reshape(-1), L)
    # an upstream of None launches nothing
    calls = []
    monkeypatch.setattr(hb, "distortion_bwd", lambda *a, **k: calls.append(1) or pytest.fail("distortion_bwd launched without an upstream"))
    raw = raw0.clone().requires_grad_(True)
    rgb, _, _, w_, _ = npa.raw2outputs(raw, z, rays[:, 3:6], 0.0, True)
    unused = npa.distortion_loss(w_, z, near, far)
    (g,) = torch.autograd.grad(rgb.sum() + w_.sum(), raw)
    assert calls == [] and unused.requires_grad and bool(torch.isfinite(g).all())
