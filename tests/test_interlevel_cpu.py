"""CPU: the interlevel loss without a GPU -- the exports and argument checks of nerf_interlevel_fwd / _bwd, the wrappers' and
render_rays' signatures, the refusals, and the definition (interlevel_loss_reference) in float64 against a plain Python double loop over
the intervals and against its closed forms.  `case` builds the rows the GPU tests run the kernels on."""
import ctypes
import inspect
import os

import pytest
import torch

import nerf_pytorch_amd as npa
from test_distortion_cpu import FAR, NEAR, composited

F64 = torch.float64
KINDS = ("nested", "independent", "duplicated depths", "target wider than the proposal", "padded tail", "all-zero target",
         "all-zero proposal", "envelope")


def overlap_mask(zp, z):
    """[n, S, P] bool: target interval j and proposal interval i intersect in positive length (+inf behind each last depth)"""
    inf = torch.full_like(z[:, :1], float("inf"))
    z1, p1 = torch.cat([z[:, 1:], inf], -1), torch.cat([zp[:, 1:], inf], -1)
    return torch.maximum(z[:, :, None], zp[:, None, :]) < torch.minimum(z1[:, :, None], p1[:, None, :])


def envelope(zp, w, z):
    """the smallest proposal that covers the target: wp_i = the largest w_j among the target intervals overlapping proposal interval i"""
    return (overlap_mask(zp, z).to(w.dtype) * w[:, :, None]).amax(1)


def case(P, S, n, seed):
    """fp32 (wp [n, P], zp [n, P], w [n, S], z [n, S]) on the CPU, depths non-decreasing: row i is of kind KINDS[i % 8].
    nested: the finer side's depths are the sorted union of the coarser side's and further draws (S >= P: the render's case, every
    target interval inside one proposal interval; S < P the other way round).  duplicated depths: every second depth repeats its
    predecessor, on the target in even rows of the kind and on the proposal in odd ones.  target wider: it starts 0.5 in front of the
    first proposal depth and ends 0.5 behind the last.  padded tail: the last two thirds of the target repeat one depth with weight 0
    (odd rows of the kind: of the proposal).  envelope: nested depths, the proposal is `envelope` of the target, and a target
    interval of zero length (a tie of two fp32 draws) carries no weight."""
    g = torch.Generator().manual_seed(seed)
    draw = lambda k: (NEAR + (FAR - NEAR) * torch.rand(n, k, generator=g)).sort(-1).values
    zp, z = draw(P), draw(S)
    if S >= P:
        z_nested, zp_nested = torch.cat([zp, draw(S - P)], -1).sort(-1).values, zp.clone()
        zp_nested[:, 0] = z_nested[:, 0]        # both start at the ray's first depth, as the coarse and the refining pass do
    else:
        z_nested, zp_nested = z, torch.cat([z, draw(P - S)], -1).sort(-1).values
    for i in range(n):
        kind, odd = KINDS[i % len(KINDS)], (i // len(KINDS)) % 2 == 1
        if kind in ("nested", "envelope"):
            z[i], zp[i] = z_nested[i], zp_nested[i]
        elif kind == "duplicated depths":
            t = zp[i] if odd else z[i]
            t[1::2] = t[0::2][:t[1::2].numel()].clone()
        elif kind == "target wider than the proposal":
            z[i] = (NEAR - 0.5 + (FAR - NEAR + 1.0) * torch.rand(S, generator=g)).sort().values
        elif kind == "padded tail":
            t = zp[i] if odd else z[i]
            cut = max(t.numel() // 3, 1)
            t[cut:] = t[cut - 1]
    sigma = lambda zz: 60.0 * ((zz > 3.5) & (zz < 3.7)).double() + 3.0 * torch.rand(zz.shape, generator=g, dtype=F64)
    w = composited(z.double(), sigma(z)).float()
    wp = composited(zp.double(), 0.5 * sigma(zp)).float()
    for i in range(n):
        kind, odd = KINDS[i % len(KINDS)], (i // len(KINDS)) % 2 == 1
        if kind == "padded tail":
            (wp if odd else w)[i, max((P if odd else S) // 3, 1):] = 0.0
        elif kind == "all-zero target":
            w[i] = 0.0
        elif kind == "all-zero proposal":
            wp[i] = 0.0
        elif kind == "envelope":
            w[i, :-1] *= (z[i, 1:] > z[i, :-1]).float()
            wp[i] = envelope(zp[i:i + 1], w[i:i + 1], z[i:i + 1])[0]
    assert bool((z[:, 1:] >= z[:, :-1]).all()) and bool((zp[:, 1:] >= zp[:, :-1]).all())
    return wp, zp, w, z


def double_loop(wp, zp, w, z):
    """the definition as a Python loop over pairs of intervals, in Python floats: (loss [n], d loss / d wp [n, P])"""
    n, P, S = wp.shape[0], wp.shape[1], w.shape[1]
    loss, grad = torch.zeros(n, dtype=F64), torch.zeros(n, P, dtype=F64)
    inf = float("inf")
    for r in range(n):
        zp_, z_ = zp[r].tolist() + [inf], z[r].tolist() + [inf]
        for j in range(S):
            over = [i for i in range(P) if max(z_[j], zp_[i]) < min(z_[j + 1], zp_[i + 1])]
            bound = 0.0
            for i in over:
                bound += float(wp[r, i])
            wj = float(w[r, j])
            excess = max(0.0, wj - bound)
            loss[r] += excess * excess / (wj + 1e-7)
            for i in over:
                grad[r, i] += -2.0 * excess / (wj + 1e-7)
    return loss, grad


def definition(wp, zp, w, z, dtype, g=None):
    """(loss [n], d (loss . g) / d wp [n, P]) of interlevel_loss_reference run in `dtype`, as float64 tensors"""
    wp_ = wp.detach().to(dtype).clone().requires_grad_(True)
    loss = npa.interlevel_loss_reference(wp_, zp, w.to(dtype), z)
    up = torch.ones_like(loss) if g is None else g.to(dtype=dtype, device=loss.device)
    (grad,) = torch.autograd.grad((loss * up).sum(), wp_)
    return loss.detach().double(), grad.double()


def test_the_library_exports_and_binds_both_entry_points():
    hb = npa.hip_backend
    raw = ctypes.CDLL(npa.build.LIB_PATH)
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "nerf_hip.h")) as f:
        header = f.read()
    for name in ("nerf_interlevel_fwd", "nerf_interlevel_bwd"):
        proto = f"int {name}(const float* proposal_weights, const float* proposal_z, int n_proposal, const float* weights,"
        assert hasattr(raw, name) and name in hb.EXPORTS and proto in header, name
    assert "#define NERF_ABI_VERSION 10" in header and hb.ABI_VERSION == 10 and raw.nerf_abi_version() == 10
    assert list(inspect.signature(hb.interlevel).parameters) == ["proposal_weights", "proposal_z", "weights", "z_vals"]
    sig = inspect.signature(hb.interlevel_bwd).parameters
    assert list(sig) == ["proposal_weights", "proposal_z", "weights", "z_vals", "d_loss", "out", "accumulate"]
    assert sig["out"].default is None and sig["accumulate"].default is False
    for name in ("interlevel_loss", "interlevel_loss_reference"):
        assert name in npa.__all__ and callable(getattr(npa, name)), name
        assert list(inspect.signature(getattr(npa, name)).parameters) == ["proposal_weights", "proposal_z", "weights", "z_vals"]


def test_both_kernels_are_in_the_resource_table_without_scratch():
    """hipcc's resource table of the build that produced the library: the forward and the adjoint form, no scratch, no spills"""
    rows = {k: v for k, v in npa.build.resource_usage().items() if "interlevel_kernel" in k}
    assert len(rows) == 2 and any("<true>" in k for k in rows) and any("<false>" in k for k in rows), sorted(rows)
    for k, v in rows.items():
        assert v["scratch_bytes_per_lane"] == 0 and v.get("vgpr_spills", 0) == 0 and v.get("sgpr_spills", 0) == 0, (k, v)


def test_argument_errors_are_codes_and_an_empty_batch_launches_nothing():
    L = npa.hip_backend.lib()
    buf = (ctypes.c_float * 64)()
    ptr = ctypes.addressof(buf)
    fwd = lambda wp, zp, P, w, z, S, n, loss: L.nerf_interlevel_fwd(wp, zp, P, w, z, S, n, loss, None)
    bwd = lambda wp, zp, P, w, z, S, n, g, dwp: L.nerf_interlevel_bwd(wp, zp, P, w, z, S, n, g, dwp, 0, None)
    ok_f, ok_b = [ptr, ptr, 4, ptr, ptr, 4, 1, ptr], [ptr, ptr, 4, ptr, ptr, 4, 1, ptr, ptr]
    for args, call, pointers in ((ok_f, fwd, (0, 1, 3, 4, 7)), (ok_b, bwd, (0, 1, 3, 4, 7, 8))):
        for k in pointers:
            bad = list(args)
            bad[k] = None
            assert call(*bad) == -1 and "null pointer" in L.nerf_last_error().decode(), (call, k)
        # the limits, refused before anything is launched or read (host memory stands in for the device buffers)
        for P, S, n in ((4, 0, 1), (4, 4097, 1), (0, 4, 1), (4097, 4, 1), (4, 4, -1)):
            bad = list(args)
            bad[2], bad[5], bad[6] = P, S, n
            assert call(*bad) == -1 and "bad size" in L.nerf_last_error().decode(), (call, P, S, n)
        none = list(args)
        none[2], none[5], none[6] = 4096, 4096, 0
        assert call(*none) == 0       # no rays: nothing to do


def test_cpu_tensors_and_mismatched_shapes_are_rejected():
    hb = npa.hip_backend
    wp, zp, w, z = case(4, 8, 3, seed=1)
    with pytest.raises(hb.NerfHipError, match="GPU"):
        hb.interlevel(wp, zp, w, z)
    with pytest.raises(hb.NerfHipError, match="GPU"):
        hb.interlevel_bwd(wp, zp, w, z, torch.ones(3))
    with pytest.raises(hb.NerfHipError, match="GPU"):
        npa.interlevel_loss(wp, zp, w, z)
    with pytest.raises(hb.NerfHipError, match="belong"):
        hb.interlevel(wp, zp, w[:2], z[:2])
    with pytest.raises(hb.NerfHipError, match="accumulate"):
        hb.interlevel_bwd(wp, zp, w, z, torch.ones(3), accumulate=True)
    for args in ((wp, zp[:, :3], w, z), (wp, zp, w, z[:, :4]), (wp, zp, w[:2], z[:2])):
        with pytest.raises(ValueError, match="belong"):
            npa.interlevel_loss(*args)


def test_render_rays_takes_interlevel_as_a_keyword_only_bool_and_refuses_what_it_cannot_serve(monkeypatch):
    params = inspect.signature(npa.render_rays).parameters
    p = params["interlevel"]
    assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default is False
    assert list(params)[list(params).index("distortion") + 1] == "interlevel"
    net = npa.NeRF(D=8, W=256, input_ch=63, output_ch=5, skips=[4], input_ch_views=27, use_viewdirs=True)
    monkeypatch.setattr(npa.hip_backend, "lib", lambda: pytest.fail("a guard let a call reach the library"))
    rays = torch.zeros(4, 11)
    grid = None     # (the refusals come before the grid is looked at)
    for bad in (1, 0.5, "yes", None):
        with pytest.raises(ValueError, match="interlevel"):
            npa.render_rays(rays, net, None, N_samples=8, N_importance=4, interlevel=bad)
    with pytest.raises(ValueError, match="interlevel.*N_importance"):
        npa.render_rays(rays, net, None, N_samples=8, N_importance=0, interlevel=True)
    with pytest.raises(ValueError, match="interlevel.*grid"):
        npa.render_rays(rays, net, None, N_samples=8, N_importance=4, interlevel=True, occupancy=grid, proposal="grid")
    with pytest.raises(ValueError, match="interlevel.*march"):
        npa.render_rays(rays, net, None, N_samples=8, N_importance=4, interlevel=True, occupancy=grid, proposal="march", march_steps=16)
    # the empty batch: an empty [0] tensor under the key, which comes last, behind "distortion"
    for kw in (dict(), dict(retraw=True)):
        ret = npa.render_rays(torch.zeros(0, 11), net, None, N_samples=8, N_importance=4, interlevel=True, **kw)
        assert list(ret)[-1] == "interlevel" and ret["interlevel"].shape == (0,) and ret["interlevel"].dtype == torch.float32
        both = npa.render_rays(torch.zeros(0, 11), net, None, N_samples=8, N_importance=4, interlevel=True, distortion=True, **kw)
        assert list(both)[-2:] == ["distortion", "interlevel"] and both["distortion"].shape == (0,)
        off = npa.render_rays(torch.zeros(0, 11), net, None, N_samples=8, N_importance=4, **kw)
        assert "interlevel" not in off and list(off) == list(ret)[:-1]


@pytest.mark.parametrize("P,S", [(1, 1), (2, 3), (5, 4), (7, 12)])
def test_the_definition_agrees_with_a_double_loop_over_the_intervals(P, S):
    wp, zp, w, z = case(P, S, 16, seed=10 * P + S)
    L, G = definition(wp, zp, w, z, F64)
    L_loop, G_loop = double_loop(wp, zp, w, z)
    assert float((L - L_loop).abs().max()) <= 1e-12 and float((G - G_loop).abs().max()) <= 1e-12
    assert L.shape == (16,) and float(L.max()) > 0 and float(G.abs().max()) > 0


def test_the_definition_meets_its_closed_forms():
    ref = npa.interlevel_loss_reference
    for P, S in ((4, 12), (12, 4), (64, 192)):
        wp, zp, w, z = case(P, S, 16, seed=P + S)
        kinds = [KINDS[i % len(KINDS)] for i in range(16)]
        for dtype in (F64, torch.float32):
            L, G = definition(wp, zp, w, z, dtype)
            for i, kind in enumerate(kinds):
                if kind == "envelope":      # the per-interval maximum of the target weights: exactly nothing to penalise, in any precision
                    assert float(w[i].max()) > 0 and float(L[i]) == 0.0 and not bool(G[i].any()), (P, S, dtype, i)
                elif kind == "all-zero target":
                    assert float(L[i]) == 0.0 and not bool(G[i].any()), (P, S, dtype, i)
                elif kind == "all-zero proposal":       # bound = 0: sum w^2 / (w + 1e-7)
                    wi = w[i].to(dtype)
                    assert float(L[i]) == pytest.approx(float((wi * wi / (wi + 1e-7)).sum()), rel=1e-6 if dtype != F64 else 1e-14, abs=0)
    # leading shapes: [2, 8, .] -> [2, 8]; the dtype follows the proposal weights
    wp, zp, w, z = case(4, 12, 16, seed=3)
    a = ref(wp.double(), zp, w.double(), z)
    b = ref(wp.double().view(2, 8, 4), zp.view(2, 8, 4), w.double().view(2, 8, 12), z.view(2, 8, 12))
    assert a.dtype == F64 and b.shape == (2, 8) and torch.equal(a, b.reshape(-1)) and ref(wp, zp, w, z).dtype == torch.float32


def test_the_definition_gives_the_target_side_and_the_depths_no_gradient():
    wp, zp, w, z = (t.double() for t in case(6, 9, 8, seed=4))
    wp.requires_grad_(True)
    w.requires_grad_(True)
    L = npa.interlevel_loss_reference(wp, zp, w, z)
    g_wp, g_w = torch.autograd.grad(L.sum(), (wp, w), allow_unused=True)
    assert g_w is None and float(g_wp.abs().max()) > 0 and float(g_wp.max()) <= 0.0        # more proposal weight never raises the loss
    zg, zpg = z.clone().requires_grad_(True), zp.clone().requires_grad_(True)
    assert not npa.interlevel_loss_reference(wp.detach(), zpg, w.detach(), zg).requires_grad
