"""Host-side checks of the ray / point / pose gradient entry points (no GPU): argument errors come back as codes, and the exports
are declared (the header <-> exports test of test_host_cpu.py covers their names)."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "oracle")):
    if _p not in sys.path:
        sys.path.insert(0, _p)


def _lib():
    import nerf_pytorch_amd
    return nerf_pytorch_amd.hip_backend.lib()


def test_field_input_grad_argument_errors():
    L = _lib()
    A, B, C, D = 0x1000, 0x2000, 0x3000, 0x4000
    assert L.nerf_field_input_grad(None, A, B, 11, C, 4, 4, D, 0, None) == -1 and b"null pointer" in L.nerf_last_error()
    assert L.nerf_field_input_grad(A, None, B, 11, C, 4, 4, D, 0, None) == -1
    assert L.nerf_field_input_grad(A, B, C, 11, D, 4, 4, None, 0, None) == -1
    assert L.nerf_field_input_grad(A, B, C, 11, D, 4, 0, 0x5000, 0, None) == -1 and b"bad size" in L.nerf_last_error()
    assert L.nerf_field_input_grad(A, B, C, 11, D, 4, -3, 0x5000, 0, None) == -1
    assert L.nerf_field_input_grad(A, B, C, 8, D, 4, 4, 0x5000, 0, None) == -1 and b"ray_stride" in L.nerf_last_error()
    # a delta buffer this library never wrote: no layout record, refused (nothing is dereferenced)
    assert L.nerf_field_input_grad(A, 0x7f000, C, 11, D, 4, 4, 0x5000, 0, None) == -1 and b"layout record" in L.nerf_last_error()


def test_raw2outputs_bwd_geom_argument_errors():
    L = _lib()
    a = [0x1000, 0x2000, 0x3000, 3, 4, 8, None, 0.0, 0, 0x4000, None, None, None, None, 0x5000]
    assert L.nerf_raw2outputs_bwd_geom(*a, None, None, None) == -1 and b"both NULL" in L.nerf_last_error()
    b = list(a)
    b[0] = None
    assert L.nerf_raw2outputs_bwd_geom(*b, 0x6000, None, None) == -1 and b"null pointer" in L.nerf_last_error()
    c = list(a)
    c[5] = 0
    assert L.nerf_raw2outputs_bwd_geom(*c, 0x6000, None, None) == -1 and b"bad size" in L.nerf_last_error()
    d = list(a)
    d[7] = 1.0          # noise std > 0 without draws
    assert L.nerf_raw2outputs_bwd_geom(*d, None, 0x6000, None) == -1 and b"noise" in L.nerf_last_error()


def test_embed_bwd_argument_errors():
    L = _lib()
    assert L.nerf_embed_bwd(None, 4, 10, 0x1000, 0x2000, 0, None) == -1 and b"null pointer" in L.nerf_last_error()
    assert L.nerf_embed_bwd(0x1000, -1, 10, 0x2000, 0x3000, 0, None) == -1 and b"bad size" in L.nerf_last_error()
    assert L.nerf_embed_bwd(0x1000, 4, 31, 0x2000, 0x3000, 0, None) == -1
    assert L.nerf_embed_bwd(0x1000, 0, 10, 0x2000, 0x3000, 0, None) == 0        # empty: nothing to do


def _fixture():
    import numpy as np
    return np.load(os.path.join(ROOT, "tests", "golden", "raygrad.npz"))


def _check(name, got64, got32, gold):
    """the fp64 oracle sits at exactly the reference's own recorded fp32-vs-fp64 distance, the fp32 oracle within it, and that noise is
    small against the gradient (the fixture is a meaningful yardstick)"""
    import torch
    ref = torch.tensor(gold[name]).double()
    noise, mx = float(gold[name + "/noise"]), float(gold[name + "/max"])
    d64 = float((got64.double() - ref).abs().max())
    d32 = float((got32.double() - ref).abs().max())
    print(f"{name}: |oracle64 - reference| {d64:.3e}, |oracle32 - reference| {d32:.3e}, recorded noise {noise:.3e} of max {mx:.3e}")
    assert d64 <= 1.001 * noise + 1e-12 * mx, (d64, noise)
    assert d32 <= noise + 1e-12 * mx, (d32, noise)
    assert noise <= 5e-3 * mx, (noise, mx)


def _generator():
    import importlib.util
    spec = importlib.util.spec_from_file_location("_make_golden_raygrad", os.path.join(ROOT, "tests", "golden", "make_golden_raygrad.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_oracle_ray_gradients_match_the_reference_fixture():
    """d loss / d ray records of render_rays (256 rays, 64 + 128 samples, jitter + density noise) and d/dx of Embedder.embed, recorded
    from the real reference: the oracle reproduces them within the reference's own rounding noise"""
    import torch
    import nerf_oracle as orc
    g, gold = _generator(), _fixture()
    Pc, Pf = orc.scene_params()
    rays, target, kw = g.ray_case()
    assert abs(float(rays.double().abs().sum()) - float(gold["rays_checksum"])) == 0.0
    rnd = g.draw_randoms()
    _check("rays", g.oracle_ray_grad(rays, rnd, target, Pc, Pf, kw), g.oracle_ray_grad(rays, rnd, target, Pc, Pf, kw, torch.float32), gold)
    _check("embed", g.oracle_embed_grad(), g.oracle_embed_grad(torch.float32), gold)


def test_oracle_pose_gradients_match_the_reference_fixture():
    """d loss / d c2w of a 20 x 24 render(c2w=pose), lego-like and fern-like (NDC), recorded from the real reference"""
    import torch
    import nerf_oracle as orc
    g, gold = _generator(), _fixture()
    Pc, Pf = orc.scene_params()
    for ndc, tag in ((False, "pose_lego"), (True, "pose_fern")):
        _check(tag, g.oracle_pose_grad(ndc, Pc, Pf), g.oracle_pose_grad(ndc, Pc, Pf, torch.float32), gold)
