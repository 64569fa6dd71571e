"""CPU: the gradient of the baked training render with respect to its rays, without a GPU -- the reference's new keywords leave the
defaults bit for bit; float64 autograd of render_rays_reference(ray_grad=True) against the closed form of DESIGN.md 3.26 written here as a
plain loop over samples and corners; gradcheck with the geometry frozen; a camera pose recovered through PoseRefinement, RayBatcher and
ray_records (the scene of the GPU recovery test); the export of nerf_baked_train_bwd_rays (csrc/baked_rays.hip) and its argument errors."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

import nerf_pytorch_amd as npa
from nerf_pytorch_amd.baked import BakedField, _render_reference, ray_records
from nerf_pytorch_amd.occupancy import OccupancyGrid
from nerf_pytorch_amd.pose import se3_exp
from test_baked_gpu import DS, GRIDS, box_of, field_of, rays_of
from test_baked_train_cpu import bits
from test_baked_train_gpu import KINK, fields_of, kept_blend, upstream

CPU = torch.device("cpu")
F64 = torch.float64
NAN, INF = float("nan"), float("inf")
OUT = ("rgb_map", "acc_map", "depth_map")
C1 = 0.4886025119029199
C2, C3, C4 = 1.0925484305920792, 0.31539156525252005, 0.5462742152960396


# ------------------------------------------------------------------------------------------------ the defaults
@pytest.mark.parametrize("degree", [0, 1, 2])
def test_the_defaults_are_unchanged(degree):
    rays, u, _ = rays_of("5x6x7", 130, 3 + degree, True)
    field = field_of("5x6x7", degree, CPU, stop_eps=0.25)
    trainer = field.trainable()
    live = rays.clone().requires_grad_(True)
    for white in (False, True):
        for dtype in (F64, torch.float32):
            for ref, keys in ((field.render_rays_reference, OUT + ("disp_map",)), (trainer.render_rays_reference, OUT)):
                want = ref(rays, u, white, 1 << 14, dtype)
                for got in (ref(rays, u, white, 1 << 14, dtype, ray_grad=False), ref(rays, u, white, 1 << 14, dtype, ray_grad=False, geometry=None),
                            ref(live, u, white, 1 << 14, dtype)):
                    assert torch.equal(got["n_samples"], want["n_samples"]) and not any(got[k].requires_grad for k in keys)
                    assert all(bits(got[k], want[k]) for k in keys)
                with_grad = ref(live, u, white, 1 << 14, dtype, ray_grad=True)
                assert torch.equal(with_grad["n_samples"], want["n_samples"]) and int(want["n_samples"].sum()) > 500
                assert all(with_grad[k].requires_grad for k in OUT)
            args = ("test", field.grid, field.index, field.table, degree, field.step_size, 0.0, rays, u, white, 1 << 14, dtype, None)
            a, b = _render_reference(*args), _render_reference(*args, ray_grad=False, geometry=None)
            assert all(bits(a[k], b[k]) for k in OUT)
    with pytest.raises(ValueError, match="geometry"):
        trainer.render_rays_reference(rays, u, geometry=rays)
    with pytest.raises(ValueError, match="geometry"):
        trainer.render_rays_reference(rays, u, ray_grad=True, geometry=rays[:5])


# ------------------------------------------------------------------------------------------------ the closed form, as a loop
def geometry_of(field, rays, u, max_steps=1 << 14):
    """(ray int64 [S], z fp32 [S], cell int64 [S, 3]) of the kept samples, ray-major and in order of k: the reference's fp32 expressions"""
    grid = field.grid
    r, ok, uu, dn, M, _ = OccupancyGrid._march_rays("test", rays, u, max_steps, 1)
    dz = torch.tensor(field.step_size, dtype=torch.float32) / dn
    z, valid = OccupancyGrid._world_steps(r, ok & torch.isfinite(dz[:, 0]) & (dz[:, 0] > 0), uu, dz, M)
    pts = r[:, None, 0:3] + r[:, None, 3:6] * z[:, :, None]
    f32 = lambda a: torch.tensor(np.asarray(a, dtype=np.float32))
    t = (pts - f32(grid.lo)) * f32(grid.scale)
    inside, _, bit = grid._classify(pts)
    rows, cols = (valid & inside & bit).nonzero(as_tuple=True)
    return rows, z[rows, cols], torch.floor(t[rows, cols]).to(torch.int64)


def sh_of(view, degree):
    x, y, z = view
    Y = [0.28209479177387814]
    if degree >= 1:
        Y += [-C1 * y, C1 * z, -C1 * x]
    if degree >= 2:
        Y += [C2 * x * y, -C2 * y * z, C3 * (2.0 * z * z - x * x - y * y), -C2 * x * z, C4 * (x * x - y * y)]
    return np.array(Y)


def sh_jacobian(view, degree):
    """[B, 3]: dY_b / d(x, y, z)"""
    x, y, z = view
    J = [[0.0, 0.0, 0.0]]
    if degree >= 1:
        J += [[0.0, -C1, 0.0], [0.0, 0.0, C1], [-C1, 0.0, 0.0]]
    if degree >= 2:
        J += [[C2 * y, C2 * x, 0.0], [0.0, -C2 * z, -C2 * y], [-2.0 * C3 * x, -2.0 * C3 * y, 4.0 * C3 * z], [-C2 * z, 0.0, -C2 * x],
              [2.0 * C4 * x, -2.0 * C4 * y, 0.0]]
    return np.array(J)


def closed_form(field, rays, u, white, G):
    """float64 [N, rays.shape[1]]: the gradient of sum G[0] . rgb_map + G[1] acc_map + G[2] depth_map with respect to the rays, by the closed
    form: per ray a forward loop over its kept samples, then back to front the sample gradients of DESIGN.md 3.23 and per sample the
    contraction with the eight corner rows"""
    grid, degree = field.grid, field.sh_degree
    B = (degree + 1) ** 2
    V = 1 + 3 * B
    ny, nz = grid.resolution[1] + 1, grid.resolution[2] + 1
    table, index = field.table.double().numpy(), field.index.numpy()
    lo, scale = np.asarray(grid.lo, dtype=np.float32).astype(np.float64), np.asarray(grid.scale, dtype=np.float32).astype(np.float64)
    ds = float(np.float32(field.step_size))
    R = rays.double().numpy()
    rows, zs, cells = (a.numpy() for a in geometry_of(field, rays, u))
    Gr, Ga, Gd = (g.double().numpy() for g in G)
    out = np.zeros(R.shape)
    for ray in np.unique(rows):
        o, d, view = R[ray, 0:3], R[ray, 3:6], R[ray, 8:11]
        Y = sh_of(view, degree)
        samples, T = [], 1.0
        for s in np.nonzero(rows == ray)[0]:
            z, cell = float(zs[s]), cells[s]
            f = (o + d * z - lo) * scale - cell
            corner, v = [], np.zeros(V)
            for q in range(8):
                qx, qy, qz = (q >> 2) & 1, (q >> 1) & 1, q & 1
                row = table[index[((cell[0] + qx) * ny + cell[1] + qy) * nz + cell[2] + qz], :V]
                v = v + (f[0] if qx else 1.0 - f[0]) * (f[1] if qy else 1.0 - f[1]) * (f[2] if qz else 1.0 - f[2]) * row
                corner.append(row)
            logits = np.array([sum(v[1 + c * B + b] * Y[b] for b in range(B)) for c in range(3)])
            col = 1.0 / (1.0 + np.exp(-logits))
            e = math.exp(-max(v[0], 0.0) * ds)
            alpha = 1.0 - e
            t = 1.0 - alpha + 1e-10
            samples.append((z, f, corner, v, col, e, alpha, t, T))
            T = T * t
        ga = Ga[ray] - Gr[ray].sum() if white else Ga[ray]
        S = 0.0
        d_o, d_d, dY = np.zeros(3), np.zeros(3), np.zeros(B)
        for z, f, corner, v, col, e, alpha, t, T in reversed(samples):
            w = alpha * T
            q = float(Gr[ray] @ col) + ga + Gd[ray] * z
            dalpha = q * T - S / t
            S = S + q * w
            a = np.zeros(V)
            a[0] = dalpha * ds * e if v[0] >= 0.0 else 0.0
            dl = w * Gr[ray] * col * (1.0 - col)
            for c in range(3):
                for b in range(B):
                    a[1 + c * B + b] = dl[c] * Y[b]
                    dY[b] += dl[c] * v[1 + c * B + b]
            df = np.zeros(3)
            for q_, row in enumerate(corner):
                qx, qy, qz = (q_ >> 2) & 1, (q_ >> 1) & 1, q_ & 1
                wx, wy, wz = (f[0] if qx else 1.0 - f[0]), (f[1] if qy else 1.0 - f[1]), (f[2] if qz else 1.0 - f[2])
                r = float(a @ row)
                df += np.array([(1.0 if qx else -1.0) * wy * wz, (1.0 if qy else -1.0) * wx * wz, (1.0 if qz else -1.0) * wx * wy]) * r
            dx = scale * df
            d_o += dx
            d_d += z * dx
        out[ray, 0:3], out[ray, 3:6], out[ray, 8:11] = d_o, d_d, sh_jacobian(view, degree).T @ dY
    return torch.from_numpy(out)


def autograd_of(trainer, rays, u, white, G, dtype=F64, geometry=None):
    """autograd's gradient of the ray_grad=True reference with respect to the rays, in dtype"""
    live = rays.detach().to(dtype).clone().requires_grad_(True)          # (a copy: rays itself stays as it is)
    out = trainer.render_rays_reference(live, u, white, dtype=dtype, ray_grad=True, geometry=geometry)
    loss = (out["rgb_map"] * G[0].to(dtype)).sum() + (out["acc_map"] * G[1].to(dtype)).sum() + (out["depth_map"] * G[2].to(dtype)).sum()
    grad, = torch.autograd.grad(loss, live, allow_unused=True)
    return torch.zeros_like(live) if grad is None else grad


@pytest.mark.parametrize("name", list(GRIDS))
@pytest.mark.parametrize("degree", [0, 1, 2])
def test_autograd_against_the_closed_form(name, degree):
    """30 rays, every kind three times (the three invalid rays included).  Both sides are float64 evaluations of one formula in different
    orders: they agree to 1e-9 x the largest |gradient|."""
    field = field_of(name, degree, CPU)
    trainer = field.trainable()
    for with_u in (False, True):
        rays, u, _ = rays_of(name, 30, 77 + degree, with_u)
        wide = torch.cat([rays, torch.full((30, 2), NAN)], -1)        # two further columns: never read
        for white in (False, True):
            G = upstream(30, 5 + degree + 2 * white)
            want = closed_form(field, rays, u, white, G)
            got = autograd_of(trainer, wide, u, white, G)
            top = float(want.abs().max())
            err = float((got[:, :11] - want).abs().max())
            print(f"\n{name}, degree {degree}, u {'given' if with_u else 'None'}, white {white}: |autograd - loop| {err:.3e}, largest |gradient| {top:.3e}")
            assert top > 1.0 and bool(torch.isfinite(got).all())
            assert err <= 1e-9 * top
            assert not bool(got[:, 6:8].any()) and not bool(got[:, 11:].any())
            empty = trainer.render_rays_reference(rays, u)["n_samples"] == 0
            assert int(empty.sum()) >= 6 and not bool(got[empty].any())
            if degree == 0:
                assert not bool(got[:, 8:11].any())
            else:
                assert int(got[~empty][:, 8:11].abs().sum(-1).gt(0).sum()) >= 10      # (a ray through sigma <= 0 alone has no weight)


@pytest.mark.parametrize("degree", [0, 1, 2])
def test_gradcheck_with_frozen_geometry(degree):
    """p -> reference(p, ray_grad=True, geometry=rays0) over the columns 0:6 and 8:11 of six rays of the 5 x 6 x 7 set (130 and 65 candidates,
    one that starts inside, one along each axis on cell planes: f = 0, where a step leaves [0, 1] and the blend extrapolates).  Without
    geometry= a finite difference in d would move every z with |d|.  With it the function is smooth but for the ReLU: the node seed is
    fields_of's, no kept sample lies within 1e-4 of the kink, and a step of eps = 1e-7 moves a blend by at most |d v0 / d x| (1 + z) eps <
    4e-5 (scale 4, corner differences below 100, z < 4).  atol: the rounding of a central difference, 1e-16 x |outputs| / eps ~ 1e-8,
    with a margin."""
    field, _, seed = fields_of("5x6x7", degree, CPU)
    trainer = field.trainable()
    rays, u, _ = rays_of("5x6x7", 10, 21 + degree, True)
    pick = torch.tensor([0, 1, 4, 5, 6, 7])
    rays0, u0 = rays[pick].double(), u[pick]
    v0, _ = kept_blend(field, rays[pick], u0)
    assert v0.numel() > 100 and float(v0.abs().min()) >= KINK, (seed, float(v0.abs().min()))

    def fn(p):
        full = torch.cat([p[:, :6], rays0[:, 6:8], p[:, 6:]], -1)
        out = trainer.render_rays_reference(full, u0, True, dtype=F64, ray_grad=True, geometry=rays0)
        return torch.cat([out["rgb_map"].reshape(-1), out["acc_map"], out["depth_map"]])
    p = torch.cat([rays0[:, :6], rays0[:, 8:11]], -1).clone().requires_grad_(True)
    assert torch.autograd.gradcheck(fn, (p,), eps=1e-7, atol=1e-6, rtol=1e-5)


# ------------------------------------------------------------------------------------------------ pose recovery
POSE = dict(H=12, W=12, focal=16.0, near=1.5, far=4.5, degree=1, twist=(0.02, -0.03, 0.025, 0.05, -0.04, 0.03), lr=5e-3, steps=40)


def pose_scene(device):
    """(field, true pose [1, 3, 4] float64, K): a Gaussian density blob in the middle of the 8^3 box, every cell occupied, colour logits
    linear in the position (the DC coefficients) with a constant degree-1 part; a 12 x 12 camera 3 in front of the centre, tilted a
    little so that no ray runs along an axis"""
    res, lo, hi = box_of("8x8x8")
    axes = [torch.linspace(l, h, r + 1, dtype=F64) for l, h, r in zip(lo, hi, res)]
    p = torch.stack(torch.meshgrid(*axes, indexing="ij"), -1)
    centre = 0.5 * (torch.tensor(lo, dtype=F64) + torch.tensor(hi, dtype=F64))
    q = p - centre
    nodes = torch.zeros(9, 9, 9, 13, dtype=F64)
    nodes[..., 0] = 15.0 * torch.exp(-(q * q).sum(-1) / (2.0 * 0.45 ** 2))
    slopes = torch.tensor([[2.0, -1.0, 0.5], [-1.5, 1.0, 2.0], [0.5, 2.0, -1.0]], dtype=F64)
    for c in range(3):
        nodes[..., 1 + 4 * c] = (q @ slopes[c]) / 0.28209479177387814
        nodes[..., 2 + 4 * c:5 + 4 * c] = torch.tensor([0.5, -0.3, 0.2], dtype=F64) * (1.0 - 0.5 * c)
    grid = OccupancyGrid.from_mask(torch.ones(res, dtype=torch.bool), lo, hi, device=device)
    field = BakedField.from_nodes(grid, nodes.float(), 1, step_size=DS)
    base = torch.eye(4, dtype=F64)
    base[:3, 3] = centre + torch.tensor([0.0, 0.0, 3.0], dtype=F64)
    tilt = se3_exp(torch.tensor([[0.05, 0.08, -0.03, 0.0, 0.0, 0.0]], dtype=F64))[0]
    centred = torch.eye(4, dtype=F64)
    centred[:3, 3] = centre
    back = torch.eye(4, dtype=F64)
    back[:3, 3] = -centre
    true = (centred @ tilt @ back @ base)[None, :3, :4]           # the tilt turns the camera about the box's centre
    K = np.array([[POSE["focal"], 0, 0.5 * POSE["W"]], [0, POSE["focal"], 0.5 * POSE["H"]], [0, 0, 1]])
    return field, true, K


def pixel_rays(pose, K, H, W):
    """[2, H W, 3]: the rays of every pixel in image order, RayBatcher's expression"""
    jj, ii = torch.meshgrid(torch.arange(H, dtype=pose.dtype, device=pose.device), torch.arange(W, dtype=pose.dtype, device=pose.device),
                            indexing="ij")
    dirs = torch.stack([(ii - K[0][2]) / K[0][0], -(jj - K[1][2]) / K[1][1], -torch.ones_like(ii)], -1).reshape(-1, 3)
    return torch.stack([pose[:3, 3].expand(H * W, 3), torch.sum(dirs[:, None, :] * pose[:3, :3], -1)], 0)


def recover(render, target, true, K, device, dtype):
    """the loop of both recovery tests: PoseRefinement(1) started at POSE["twist"], a RayBatcher whose batch is the whole image, Adam on
    xi; returns the losses, the one before the first step first"""
    H, W = POSE["H"], POSE["W"]
    refine = npa.PoseRefinement(1).to(device=device, dtype=dtype)
    with torch.no_grad():
        refine.xi.copy_(torch.tensor([POSE["twist"]], dtype=dtype))
    batcher = npa.RayBatcher(target.view(1, H, W, 3), K, H * W, [0], generator=torch.Generator().manual_seed(4))
    opt = torch.optim.Adam(refine.parameters(), lr=POSE["lr"])
    poses = true.to(device=device, dtype=dtype)
    losses = []
    for _ in range(POSE["steps"] + 1):
        opt.zero_grad()
        rays, rgb = batcher.next(refine(poses))
        loss = ((render(ray_records(rays, POSE["near"], POSE["far"])) - rgb) ** 2).mean()
        losses.append(float(loss.detach()))
        loss.backward()
        opt.step()
    return losses


def test_ray_records():
    g = torch.Generator().manual_seed(1)
    batch = torch.randn(2, 7, 3, generator=g, dtype=F64).requires_grad_(True)
    rec = ray_records(batch, 2.0, 6.0)
    assert rec.shape == (7, 11) and rec.dtype == F64 and torch.equal(rec[:, 0:3], batch[0]) and torch.equal(rec[:, 3:6], batch[1])
    assert bool((rec[:, 6] == 2.0).all()) and bool((rec[:, 7] == 6.0).all())
    assert torch.allclose(rec[:, 8:11].norm(dim=-1), torch.ones(7, dtype=F64), atol=1e-15)
    assert torch.allclose(rec[:, 8:11] * batch[1].norm(dim=-1, keepdim=True), batch[1], atol=1e-15)
    assert torch.autograd.gradcheck(lambda b: ray_records(b, 2.0, 6.0), (batch,))
    assert "ray_records" in npa.__all__ and npa.ray_records is ray_records and npa.baked.ray_records is ray_records
    with pytest.raises(ValueError, match="2, N, 3"):
        ray_records(torch.zeros(7, 6), 2.0, 6.0)


def test_pose_recovery_on_the_reference():
    """float64, the CPU reference: from the twist POSE["twist"], POSE["steps"] Adam steps at POSE["lr"] end below a quarter of the initial
    loss -- the scene, the twist, the learning rate and the step count of the GPU recovery test (tests/test_baked_rays_gpu.py)"""
    field, true, K = pose_scene(CPU)
    trainer = field.trainable()
    H, W = POSE["H"], POSE["W"]
    with torch.no_grad():
        first = ray_records(pixel_rays(true[0], K, H, W), POSE["near"], POSE["far"])
        out = trainer.render_rays_reference(first, white_bkgd=True)
        target = out["rgb_map"]
    assert int((out["n_samples"] > 0).sum()) == H * W and 0.3 < float(out["acc_map"].mean()) < 0.98
    render = lambda rays: trainer.render_rays_reference(rays, white_bkgd=True, dtype=F64, ray_grad=True)["rgb_map"]
    losses = recover(render, target, true, K, CPU, F64)
    print(f"\npose recovery, float64 reference: loss {losses[0]:.4e} -> {losses[-1]:.4e} in {POSE['steps']} Adam steps "
          f"(ratio {losses[-1] / losses[0]:.4f}; smallest on the way {min(losses):.4e})")
    assert losses[0] > 1e-5
    assert losses[-1] < 0.25 * losses[0]


# ------------------------------------------------------------------------------------------------ exports
def test_the_library_exports_and_binds_the_entry_point():
    hb = npa.hip_backend
    raw = ctypes.CDLL(npa.build.LIB_PATH)
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "nerf_hip.h")) as f:
        header = f.read()
    name = "nerf_baked_train_bwd_rays"
    assert hasattr(raw, name) and name in hb.EXPORTS and f"int {name}(" in header and callable(hb.baked_train_bwd_rays)
    assert "#define NERF_ABI_VERSION 10" in header and hb.ABI_VERSION == 10 and hb.lib().nerf_abi_version() == 10
    assert "baked_rays.hip" in npa.build.SOURCES
    rows = {k: v for k, v in npa.build.resource_usage().items() if v["source"] == "baked_rays.hip"}
    assert len(rows) == 3 and all("baked_train_bwd_rays_kernel" in k for k in rows), sorted(rows)          # one per degree
    for k, v in rows.items():
        assert v["scratch_bytes_per_lane"] == 0 and v.get("vgpr_spills", 0) == 0 and v.get("sgpr_spills", 0) == 0 and v["lds_bytes"] == 0, (k, v)


def test_every_limit_is_refused_before_a_launch():
    """host memory stands in for the device buffers: nothing is launched or read"""
    hb = npa.hip_backend
    L = hb.lib()
    buf = (ctypes.c_float * 64)()
    ptr = (ctypes.addressof(buf) + 15) & ~15
    desc = hb.NerfOccGrid((ctypes.c_float * 3)(0, 0, 0), (ctypes.c_float * 3)(1, 1, 1), (ctypes.c_int * 3)(2, 2, 2), 0, ptr)
    nobits = hb.NerfOccGrid((ctypes.c_float * 3)(0, 0, 0), (ctypes.c_float * 3)(1, 1, 1), (ctypes.c_int * 3)(2, 2, 2), 0, None)
    err = lambda: L.nerf_last_error().decode()

    def rays_(grid=desc, rows=1, degree=0, stride=11, n=1, total=1, **null):
        a = dict(index=ptr, table=ptr, rays=ptr, records=ptr, grads=ptr, offsets=ptr, out=ptr)
        a.update(null)
        return L.nerf_baked_train_bwd_rays(None if grid is None else ctypes.byref(grid), a["index"], a["table"], rows, degree, a["rays"], stride, n,
                                           a["records"], a["grads"], a["offsets"], total, a["out"], None)

    for name in ("index", "table", "rays", "records", "grads", "offsets", "out"):
        assert rays_(**{name: None}) == -1 and "null" in err(), name
    assert rays_(grid=None) == -1 and "null" in err()
    assert rays_(grid=nobits) == -1 and "null" in err()
    for degree in (-1, 3):
        assert rays_(degree=degree) == -1 and "sh_degree" in err(), degree
    for stride in (10, 0, -11):
        assert rays_(stride=stride) == -1 and "11 columns" in err(), stride
    assert rays_(n=-1) == -1 and "bad size" in err()
    for r in (0, -1):
        assert rays_(rows=r) == -1 and "n_rows" in err(), r
    for total in (-1, (1 << 30) + 1):
        assert rays_(total=total) == -1 and "2^30" in err(), total
    assert rays_(table=ptr + 8) == -1 and "aligned" in err()
    assert rays_(records=ptr + 8) == -1 and "aligned" in err()
    assert rays_(grads=ptr + 4) == -1 and "aligned" in err()
    # no rays: nothing to do (no samples: zeros written to device memory, tests/test_baked_rays_gpu.py)
    for degree in (0, 1, 2):
        assert rays_(n=0, degree=degree, total=0) == 0 and rays_(n=0, degree=degree, total=5) == 0
    # the binding refuses host tensors before the library is reached
    with pytest.raises(hb.NerfHipError, match="on the GPU"):
        hb.baked_train_bwd_rays(desc, torch.zeros(27, dtype=torch.int32), torch.zeros(1, 4, dtype=torch.float16), 0, torch.zeros(2, 11),
                                torch.zeros(1, 12), torch.zeros(1, 4), torch.zeros(3, dtype=torch.int32), 0)
