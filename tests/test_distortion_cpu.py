"""CPU: the distortion loss without a GPU -- the exports and argument checks of nerf_distortion_fwd / _bwd, render_rays' keyword, and the
definition (distortion_loss_reference) in float64 against closed forms and its autograd gradient against the closed-form dL/dw."""
import ctypes
import inspect
import os

import pytest
import torch

import nerf_pytorch_amd as npa

F64 = torch.float64
NEAR, FAR = 2.0, 6.0


def composited(z, sigma):
    """compositing weights as in raw2outputs with |d| = 1: alpha_i T_i, the last distance 1e10"""
    dists = torch.cat([z[:, 1:] - z[:, :-1], torch.full_like(z[:, :1], 1e10)], -1)
    alpha = 1.0 - torch.exp(-torch.relu(sigma) * dists)
    T = torch.cumprod(torch.cat([torch.ones_like(alpha[:, :1]), 1.0 - alpha + 1e-10], -1), -1)[:, :-1]
    return alpha * T


def families(n, S, seed, dtype=F64):
    """the three weight recipes: (z [3n, S] sorted uniform draws in [NEAR, FAR], w [3n, S]) -- a thin opaque surface, a fog, sparse spikes"""
    g = torch.Generator().manual_seed(seed)
    z = (NEAR + (FAR - NEAR) * torch.rand(3 * n, S, generator=g, dtype=F64)).sort(-1).values
    u = torch.rand(3 * n, S, generator=g, dtype=F64)
    surface = 60.0 * ((z[:n] > 3.5) & (z[:n] < 3.7)).to(F64) + 0.05 * u[:n]
    fog = 2.0 * u[n:2 * n]
    spikes = 100.0 * u[2 * n:] * (torch.rand(n, S, generator=g) < 0.1).to(F64)
    w = composited(z, torch.cat([surface, fog, spikes], 0))
    return z.to(dtype), w.to(dtype)


def closed_form_grad(w, z, near, far):
    """dL/dw_k = 2 sum_j w_j |m_k - m_j| + 2/3 w_k dl_k, written out"""
    s = (z - near) / (far - near)
    m = torch.cat([0.5 * (s[:, :-1] + s[:, 1:]), s[:, -1:]], -1)
    dl = torch.cat([s[:, 1:] - s[:, :-1], torch.zeros_like(s[:, :1])], -1)
    return 2.0 * (w[:, None, :] * (m[:, :, None] - m[:, None, :]).abs()).sum(-1) + (2.0 / 3.0) * w * dl


def test_the_library_exports_and_binds_both_entry_points():
    hb = npa.hip_backend
    raw = ctypes.CDLL(npa.build.LIB_PATH)
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "nerf_hip.h")) as f:
        header = f.read()
    for name in ("nerf_distortion_fwd", "nerf_distortion_bwd"):
        assert hasattr(raw, name) and name in hb.EXPORTS and f"int {name}(const float* weights, const float* z_vals, const float* near_far, int nf_stride," in header, name
    assert "#define NERF_ABI_VERSION 10" in header and hb.ABI_VERSION == 10
    assert callable(hb.distortion) and callable(hb.distortion_bwd)
    assert list(inspect.signature(hb.distortion).parameters) == ["weights", "z_vals", "near_far", "nf_stride", "nf_offset"]
    assert list(inspect.signature(hb.distortion_bwd).parameters)[:6] == ["weights", "z_vals", "near_far", "d_loss", "out", "accumulate"]
    for name in ("distortion_loss", "distortion_loss_reference"):
        assert name in npa.__all__ and callable(getattr(npa, name)), name
        assert list(inspect.signature(getattr(npa, name)).parameters) == ["weights", "z_vals", "near", "far"]


def test_both_kernels_are_in_the_resource_table_without_scratch():
    """hipcc's resource table of the build that produced the library: the forward and the adjoint form, no scratch, no spills"""
    rows = {k: v for k, v in npa.build.resource_usage().items() if "distortion_kernel" in k}
    assert len(rows) == 2 and any("<true>" in k for k in rows) and any("<false>" in k for k in rows), sorted(rows)
    for k, v in rows.items():
        assert v["scratch_bytes_per_lane"] == 0 and v.get("vgpr_spills", 0) == 0 and v.get("sgpr_spills", 0) == 0, (k, v)


def test_argument_errors_are_codes_and_an_empty_batch_launches_nothing():
    L = npa.hip_backend.lib()
    buf = (ctypes.c_float * 64)()
    ptr = ctypes.addressof(buf)
    fwd = lambda w, z, nf, n, S, loss: L.nerf_distortion_fwd(w, z, nf, 11, n, S, loss, None)
    bwd = lambda w, z, nf, n, S, g, dw: L.nerf_distortion_bwd(w, z, nf, 11, n, S, g, dw, 0, None)
    for args in ((None, ptr, ptr, 1, 4, ptr), (ptr, None, ptr, 1, 4, ptr), (ptr, ptr, None, 1, 4, ptr), (ptr, ptr, ptr, 1, 4, None)):
        assert fwd(*args) == -1 and "null pointer" in L.nerf_last_error().decode(), args
    for args in ((None, ptr, ptr, 1, 4, ptr, ptr), (ptr, None, ptr, 1, 4, ptr, ptr), (ptr, ptr, None, 1, 4, ptr, ptr),
                 (ptr, ptr, ptr, 1, 4, None, ptr), (ptr, ptr, ptr, 1, 4, ptr, None)):
        assert bwd(*args) == -1 and "null pointer" in L.nerf_last_error().decode(), args
    # the limits, refused before anything is launched or read (host memory stands in for the device buffers)
    for n, S in ((1, 0), (1, 4097), (-1, 8)):
        assert fwd(ptr, ptr, ptr, n, S, ptr) == -1 and "bad size" in L.nerf_last_error().decode(), (n, S)
        assert bwd(ptr, ptr, ptr, n, S, ptr, ptr) == -1 and "bad size" in L.nerf_last_error().decode(), (n, S)
    assert fwd(ptr, ptr, ptr, 0, 4096, ptr) == 0 and bwd(ptr, ptr, ptr, 0, 4096, ptr, ptr) == 0        # no rays: nothing to do


def test_cpu_tensors_are_rejected_by_the_binding_and_the_public_function():
    hb = npa.hip_backend
    w, z = torch.rand(3, 8), torch.rand(3, 8).sort(-1).values
    nf = torch.tensor([[0.0, 1.0]] * 3)
    with pytest.raises(hb.NerfHipError, match="GPU"):
        hb.distortion(w, z, nf)
    with pytest.raises(hb.NerfHipError, match="GPU"):
        hb.distortion_bwd(w, z, nf, torch.ones(3))
    with pytest.raises(hb.NerfHipError, match="GPU"):
        npa.distortion_loss(w, z, 0.0, 1.0)
    with pytest.raises(ValueError, match="shape"):
        npa.distortion_loss(w, z[:, :4], 0.0, 1.0)


def test_render_rays_takes_distortion_as_a_keyword_only_bool(monkeypatch):
    p = inspect.signature(npa.render_rays).parameters["distortion"]
    assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default is False
    net = npa.NeRF(D=8, W=256, input_ch=63, output_ch=5, skips=[4], input_ch_views=27, use_viewdirs=True)
    monkeypatch.setattr(npa.hip_backend, "lib", lambda: pytest.fail("a guard let a call reach the library"))
    for bad in (1, 0.5, "yes", None):
        with pytest.raises(ValueError, match="distortion"):
            npa.render_rays(torch.zeros(4, 11), net, None, N_samples=8, distortion=bad)
    # the empty batch: an empty [0] tensor under the key, which comes last
    for kw in (dict(), dict(N_importance=4), dict(retraw=True)):
        ret = npa.render_rays(torch.zeros(0, 11), net, None, N_samples=8, distortion=True, **kw)
        assert list(ret)[-1] == "distortion" and ret["distortion"].shape == (0,) and ret["distortion"].dtype == torch.float32
        assert "distortion" not in npa.render_rays(torch.zeros(0, 11), net, None, N_samples=8, **kw)


def test_the_definition_meets_its_closed_forms_in_float64():
    ref = npa.distortion_loss_reference
    t = lambda *v: torch.tensor([list(v)], dtype=F64)
    s = lambda z: (z - NEAR) / (FAR - NEAR)
    # S = 1: nothing to spread over
    assert float(ref(t(0.7), t(3.0), NEAR, FAR)) == 0.0
    # S = 2: m0 = (s0 + s1) / 2, m1 = s1, dl0 = s1 - s0, dl1 = 0
    w0, w1, z0, z1 = 0.3, 0.45, 2.5, 4.25
    want = 2 * w0 * w1 * abs(0.5 * (s(z0) + s(z1)) - s(z1)) + w0 * w0 * (s(z1) - s(z0)) / 3
    assert float(ref(t(w0, w1), t(z0, z1), NEAR, FAR)) == pytest.approx(want, rel=1e-14, abs=0)
    # one non-zero weight: 1/3 w^2 dl of its own interval (0 for the last sample, whose interval has no length)
    z = t(2.0, 2.5, 3.5, 5.0, 6.0)
    for k in range(5):
        w = torch.zeros(1, 5, dtype=F64)
        w[0, k] = 0.8
        dl = float(s(z[0, k + 1]) - s(z[0, k])) if k < 4 else 0.0
        assert float(ref(w, z, NEAR, FAR)) == pytest.approx(0.64 * dl / 3, rel=1e-14, abs=0)
    # all-zero weights; far == near (and far < near): 0, no NaN, also in the gradient
    assert float(ref(torch.zeros(1, 5, dtype=F64), z, NEAR, FAR)) == 0.0
    for near, far in ((3.0, 3.0), (3.0, 2.0)):
        w = torch.full((1, 5), 0.2, dtype=F64, requires_grad=True)
        L = ref(w, z, near, far)
        (g,) = torch.autograd.grad(L.sum(), w)
        assert float(L.detach()) == 0.0 and torch.equal(g, torch.zeros_like(g))
    # near / far as per-ray tensors and as numbers agree; the dtype follows the weights
    zz, ww = families(4, 16, seed=3)
    a = ref(ww, zz, NEAR, FAR)
    b = ref(ww, zz, torch.full((12,), NEAR, dtype=F64), torch.full((12,), FAR, dtype=F64))
    assert torch.equal(a, b) and a.dtype == F64 and a.shape == (12,)
    assert ref(ww.float(), zz.float(), NEAR, FAR).dtype == torch.float32
    # translation and scale of the depths together with near / far change nothing (s is what enters)
    c = ref(ww, 3.0 * zz + 1.0, 3.0 * NEAR + 1.0, 3.0 * FAR + 1.0)
    assert torch.allclose(a, c, rtol=1e-12, atol=0)


@pytest.mark.parametrize("S", [2, 7, 64, 65])
def test_the_definitions_autograd_gradient_is_the_closed_form(S):
    z, w = families(3, S, seed=S)
    w = w.clone().requires_grad_(True)
    L = npa.distortion_loss_reference(w, z, NEAR, FAR)
    (g,) = torch.autograd.grad(L.sum(), w)
    want = closed_form_grad(w.detach(), z, NEAR, FAR)
    assert float((g - want).abs().max()) <= 1e-14 * max(1.0, float(want.abs().max()))
    assert float(L.detach().max()) <= 4.0 / 3.0 and float(g.abs().max()) <= 8.0 / 3.0       # the bounds the GPU tolerance floor rests on
    # no gradient to the depths, near or far
    zg = z.clone().requires_grad_(True)
    assert not npa.distortion_loss_reference(w.detach(), zg, NEAR, FAR).requires_grad
