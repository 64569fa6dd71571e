"""GPU tests (-m gpu) of the baked training render's gradient to its rays (csrc/baked_rays.hip, BakedTrainer.render_rays(ray_grad=True))
against its definition.

THE DEFINITION is float64 autograd of BakedTrainer.render_rays_reference(ray_grad=True) on the CPU, at the fp16 table's values, of the loss
sum G . rgb_map + g_acc acc_map + g_depth depth_map with seeded random G, g_acc, g_depth, with respect to the rays.  THE YARDSTICK is the
same autograd in float32 against float64 (the project's rule for this family, tests/test_baked_train_gpu.py): over each case set -- one
grid, one ray count, one degree; u None and given, white_bkgd off and on -- the kernel's largest absolute error over d_rays may be at most
max(4 x the yardstick's, 2^-22 x the largest |gradient| of the definition).
Condition on the inputs, asserted: no kept sample's float64 blend has |v0| < 1e-4 (the node seeds of tests/test_baked_train_gpu.py's
fields_of); no sample is left out.

Shapes: tests/test_baked_gpu.py's -- grids 5 x 6 x 7 and 8^3 at DS = 0.02, 1 / 5 / 130 rays of the ten kinds: the smallest at which rounds
of 64 records, partly filled rounds, axis rays on cell planes (f = 0), misses and invalid rays can go wrong."""
import pytest
import torch

from test_baked_gpu import COUNTS, GRIDS, KINDS, rays_of
from test_baked_rays_cpu import POSE, autograd_of, pixel_rays, pose_scene, recover
from test_baked_train_gpu import KINK, OUT, cases_of, fields_of, kept_blend, upstream, within
from test_gpu_occupancy import bits_equal
from test_gpu_parity import dev, maxdiff, npa  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

F64 = torch.float64


def kernels(trainer, rays, u, white, G, ray_grad=True, max_steps=1 << 14):
    """(the outputs, the gradient of `values`, the gradient of the rays -- None without ray_grad) of the trainer on the GPU"""
    d = trainer.device
    live = rays.detach().to(d).requires_grad_(True)
    out = trainer.render_rays(live, None if u is None else u.to(d), white, max_steps, ray_grad=ray_grad)
    wrt = [trainer.values, live] if ray_grad else [trainer.values]
    grads = torch.autograd.grad([out[k] for k in OUT], wrt, [g.to(d) for g in G])
    return out, grads[0], grads[1] if ray_grad else None


@pytest.fixture(scope="module")
def measured(npa, dev):
    """every case once: {(grid, n, degree): [rows]} and the fields {(grid, degree): (cpu, gpu, seed)}"""
    out, fields = {}, {}
    for name in GRIDS:
        for degree in (0, 1, 2):
            cpu, gpu, seed = fields_of(name, degree, dev)
            fields[(name, degree)] = (cpu, gpu, seed)
            ct, gt = cpu.trainable(), gpu.trainable()
            for i, (n, rays, u, white) in enumerate(cases_of(name, degree)):
                G = upstream(n, 11 * i + degree)
                g64, g32 = autograd_of(ct, rays, u, white, G, F64), autograd_of(ct, rays, u, white, G, torch.float32)
                plain, plain_grad, _ = kernels(gt, rays, u, white, G, ray_grad=False)
                got, grad, d_rays = kernels(gt, rays, u, white, G)
                out.setdefault((name, n, degree), []).append(dict(
                    n=n, rays=rays, u=u, white=white, G=G, g64=g64, plain=plain, plain_grad=plain_grad, out=got, grad=grad, d_rays=d_rays,
                    stats=dict(gt.last_stats), err=maxdiff(d_rays, g64), yard=maxdiff(g32, g64), top=float(g64.abs().max())))
    return out, fields


def test_the_condition_on_the_inputs(measured):
    rows, fields = measured
    for (name, n, degree), rs in rows.items():
        cpu = fields[(name, degree)][0]
        for r in rs:
            v0, _ = kept_blend(cpu, r["rays"], r["u"])
            assert v0.numel() == r["stats"]["samples"] and r["stats"]["rays"] == n
            assert v0.numel() == 0 or float(v0.abs().min()) >= KINK, (name, n, degree, fields[(name, degree)][2])


def test_the_option_changes_nothing_else(measured):
    """the forward outputs and the gradient of `values` have the bits they have without ray_grad"""
    for key, rs in measured[0].items():
        for r in rs:
            assert all(bits_equal(r["out"][k], r["plain"][k]) and r["out"][k].requires_grad for k in OUT), key
            assert bits_equal(r["grad"], r["plain_grad"]), key
        if key[1] == 130:
            assert any(bool(r["grad"].any()) for r in rs)


@pytest.mark.parametrize("name", list(GRIDS))
@pytest.mark.parametrize("degree", [0, 1, 2])
@pytest.mark.parametrize("n", COUNTS)
def test_d_rays_against_the_definition(measured, name, degree, n):
    rows = measured[0][(name, n, degree)]
    assert len(rows) == 4 and [r["white"] for r in rows] == [False, True, False, True] and rows[0]["u"] is None and rows[2]["u"] is not None
    for r in rows:
        assert r["d_rays"].shape == (n, 11) and r["d_rays"].dtype == torch.float32 and bool(torch.isfinite(r["d_rays"]).all())
    if n > 1:
        assert max(r["top"] for r in rows) > 0.0
    within(rows, f"d_rays: {name}, {n} rays, degree {degree}")


def test_exact_zeros(npa, dev, measured):
    rows, fields = measured
    for (name, n, degree), rs in rows.items():
        for r in rs:
            d = r["d_rays"].cpu()
            assert not bool(d[:, 6:8].any()), (name, n, degree)
            empty = torch.arange(n) % len(KINDS) >= 8             # the misses and the invalid rays
            assert not bool(d[empty].any()) and not bool(r["g64"][empty].any()), (name, n, degree)
            if degree == 0:
                assert not bool(d[:, 8:11].any())
            if n == 130:
                assert int(d[~empty][:, 0:6].abs().sum(-1).gt(0).sum()) > 80
    # a 13-column ray tensor: the gradient has its shape, the two further columns get zeros and the record's columns the same bits
    for degree in (0, 2):
        r = rows[("5x6x7", 130, degree)][-1]
        trainer = fields[("5x6x7", degree)][1].trainable()
        wide = torch.cat([r["rays"], torch.full((130, 2), float("nan"))], -1)
        _, grad, d = kernels(trainer, wide, r["u"], r["white"], r["G"])
        assert d.shape == (130, 13) and not bool(d[:, 11:].any()) and bits_equal(d[:, :11].contiguous(), r["d_rays"]) and bits_equal(grad, r["grad"])


def test_empty_batches(npa, dev, measured):
    """no rays at all, and rays that keep nothing (misses and invalid rays only): zeros, through .backward() as well"""
    cpu, gpu, _ = measured[1][("8x8x8", 1)]
    rays, u, _ = rays_of("8x8x8", 130, 4, True)
    empty = torch.arange(130) % len(KINDS) >= 8
    trainer = gpu.trainable()
    for rr, uu in ((rays[empty], u[empty]), (rays[:0], u[:0]), (rays[:0], None)):
        out, grad, d = kernels(trainer, rr, uu, True, upstream(rr.shape[0], 1))
        assert trainer.last_stats == {"rays": rr.shape[0], "samples": 0}
        assert d.shape == rr.shape and d.dtype == torch.float32 and not bool(d.any()) and not bool(grad.any())
        live = rr.to(dev).requires_grad_(True)
        got = trainer.render_rays(live, uu.to(dev) if uu is not None else None, True, ray_grad=True)
        (got["rgb_map"].sum() + got["depth_map"].sum()).backward()
        assert live.grad is not None and live.grad.shape == rr.shape and not bool(live.grad.any())
        trainer.values.grad = None


@pytest.mark.parametrize("degree", [0, 1, 2])
def test_two_backward_calls_give_the_same_bits(npa, dev, measured, degree):
    rows, fields = measured
    for name in GRIDS:
        trainer = fields[(name, degree)][1].trainable()
        r = rows[(name, 130, degree)][-1]
        a = kernels(trainer, r["rays"], r["u"], r["white"], r["G"])[2]
        b = kernels(trainer, r["rays"], r["u"], r["white"], r["G"])[2]
        assert bits_equal(a, b) and bits_equal(a, r["d_rays"]) and bool(a.any())


@pytest.mark.parametrize("degree", [0, 2])
def test_localisation_mode_runs_no_sort_and_no_row_pass(npa, dev, measured, degree, monkeypatch):
    """values.requires_grad_(False): d_rays has the same bits, and neither the inverted index nor nerf_baked_train_bwd_rows is called"""
    rows, fields = measured
    hb, baked = npa.hip_backend, npa.baked
    calls = {"rows": 0, "sort": 0, "rays": 0, "samples": 0}

    def counting(key, fn):
        def wrapper(*a, **kw):
            calls[key] += 1
            return fn(*a, **kw)
        return wrapper
    monkeypatch.setattr(hb, "baked_train_bwd_rows", counting("rows", hb.baked_train_bwd_rows))
    monkeypatch.setattr(hb, "baked_train_bwd_rays", counting("rays", hb.baked_train_bwd_rays))
    monkeypatch.setattr(hb, "baked_train_bwd_samples", counting("samples", hb.baked_train_bwd_samples))
    monkeypatch.setattr(baked, "inverted_index", counting("sort", baked.inverted_index))
    r = rows[("8x8x8", 130, degree)][-1]
    trainer = fields[("8x8x8", degree)][1].trainable()
    G = [g.to(dev) for g in r["G"]]
    u = r["u"].to(dev)
    # both: every pass once
    live = r["rays"].to(dev).requires_grad_(True)
    out = trainer.render_rays(live, u, r["white"], ray_grad=True)
    torch.autograd.backward([out[k] for k in OUT], G)
    assert calls == {"rows": 1, "sort": 1, "rays": 1, "samples": 1} and bits_equal(live.grad, r["d_rays"]) and bits_equal(trainer.values.grad, r["grad"])
    # the table alone, with rays that require grad but without the option: no ray pass
    trainer.values.grad = None
    out = trainer.render_rays(live, u, r["white"])
    torch.autograd.backward([out[k] for k in OUT], G)
    assert calls == {"rows": 2, "sort": 2, "rays": 1, "samples": 2} and bits_equal(trainer.values.grad, r["grad"])
    # the rays alone
    trainer.values.grad = None
    trainer.values.requires_grad_(False)
    live = r["rays"].to(dev).requires_grad_(True)
    out = trainer.render_rays(live, u, r["white"], ray_grad=True)
    assert all(bits_equal(out[k], r["out"][k]) for k in OUT)
    torch.autograd.backward([out[k] for k in OUT], G)
    assert calls == {"rows": 2, "sort": 2, "rays": 2, "samples": 3}
    assert bits_equal(live.grad, r["d_rays"]) and trainer.values.grad is None


def test_pose_recovery(npa, dev):
    """the scene, the twist, the learning rate and the step count of tests/test_baked_rays_cpu.py's float64 loop, which ends below a quarter
    of its initial loss; here through PoseRefinement, RayBatcher, ray_records and render_rays(ray_grad=True) in fp32 on the fp16 table,
    with the table frozen: below half"""
    field, true, K = pose_scene(dev)
    trainer = field.trainable()
    trainer.values.requires_grad_(False)
    H, W = POSE["H"], POSE["W"]
    with torch.no_grad():
        first = npa.ray_records(pixel_rays(true[0].to(dev).float(), K, H, W), POSE["near"], POSE["far"])
        target = trainer.render_rays(first, white_bkgd=True)["rgb_map"]
    assert trainer.last_stats["samples"] > 20 * H * W
    render = lambda rays: trainer.render_rays(rays, white_bkgd=True, ray_grad=True)["rgb_map"]
    losses = recover(render, target, true, K, dev, torch.float32)
    print(f"\npose recovery on the GPU: loss {losses[0]:.4e} -> {losses[-1]:.4e} in {POSE['steps']} Adam steps (ratio {losses[-1] / losses[0]:.4f})")
    assert losses[0] > 1e-5
    assert losses[-1] < 0.5 * losses[0]


def test_render_rays_with_a_baked_field_still_has_no_backward(npa, dev, measured):
    field = measured[1][("8x8x8", 1)][1]
    rays = rays_of("8x8x8", 130, 4, False)[0].to(dev)
    got = npa.render_rays(rays, None, None, N_samples=64, baked=field)
    assert not any(v.requires_grad for v in got.values())
    with pytest.raises(ValueError, match="no backward"):
        npa.render_rays(rays.clone().requires_grad_(True), None, None, N_samples=64, baked=field)
