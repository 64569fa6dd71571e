"""GPU tests (-m gpu) of occupancy grids from training cameras and silhouettes: nerf_occ_view_carve against the two definitions
(OccupancyGrid.view_counts_reference / carved_reference) evaluated on the CPU, bit for bit, on a non-cubic grid with a ragged last word
and cameras of every kind; then the wiring -- from_views, DensityGrid.restrict_to_views followed by update(), and a training step
through a restricted DensityGrid during its warm-up."""
import pytest
import torch

import nerf_oracle as orc
import nerf_pytorch_amd as npa_
from test_gpu_occupancy import BOX_HI, BOX_LO, BOX_R, bits_equal
from test_gpu_occupancy_train import fresh_nets, grads_of, loss_of, positive_median_density, scene_target, zero_grads
from test_gpu_parity import dev, nets, npa  # noqa: F401  (fixtures)
from test_view_carve_cpu import look_at, ring, sphere_silhouette

pytestmark = pytest.mark.gpu

CPU = torch.device("cpu")
RES = (37, 21, 63)              # 48,951 cells: the last word holds 23 of them, the last wave 55
LO, HI = (-1.5, -1.0, -2.0), (1.5, 1.0, 2.0)
H, W = 40, 56
NEAR, FAR = 0.5, 6.0
K = torch.tensor([[60.0, 0.0, 28.0], [0.0, 60.0, 20.0], [0.0, 0.0, 1.0]])


def six_cameras():
    """two ordinary cameras, one inside the box, one looking away from it, one with a NaN entry, one with its own K"""
    c2w = torch.stack([look_at((3.5, 0.5, 1.0)), look_at((-1.0, 3.0, -2.0)), look_at((0.4, -0.3, 0.2), target=(3.0, 1.0, -1.0)),
                       look_at((0.0, -4.0, 0.5), target=(0.0, -9.0, 0.5)), look_at((2.0, 2.0, 2.0)), look_at((0.5, -3.5, 2.5))])
    c2w[4, 1, 0] = float("nan")
    Ks = K[None].repeat(6, 1, 1)
    Ks[5] = torch.tensor([[95.0, 0.0, 25.5], [0.0, 80.0, 22.25], [0.0, 0.0, 1.0]])
    return c2w, Ks


def six_masks():
    """random blobs (8 x 8 pixel blocks), camera 1 all foreground, camera 5 all background"""
    g = torch.Generator().manual_seed(17)
    masks = (torch.rand(6, 5, 7, generator=g) < 0.4).repeat_interleave(8, 1).repeat_interleave(8, 2)
    masks[1], masks[5] = True, False
    return masks


@pytest.fixture(scope="module")
def reference():
    """the definitions on the CPU, computed once: (grid, c2w, Ks, masks, count int32 [cells], carved words int32)"""
    grid = npa_.OccupancyGrid(LO, HI, RES, device=CPU)
    c2w, Ks = six_cameras()
    masks = six_masks()
    count = grid.view_counts_reference(c2w, H, W, Ks, NEAR, FAR).reshape(-1)
    carved = npa_.occupancy._pack_bits(grid.carved_reference(c2w, H, W, Ks, NEAR, FAR, masks).reshape(-1))
    return grid, c2w, Ks, masks, count, carved


def test_the_kernel_equals_the_definitions_bit_for_bit(npa, dev, reference):
    """seen == view_counts_reference (torch.equal) and the carved words == carved_reference's, with the table and without it, in one
    call and as two accumulate chunks of 4 + 2 views"""
    hb, occ = npa.hip_backend, npa.occupancy
    ref_grid, c2w, Ks, masks, count, carved = reference
    # the scene exercises what it claims to
    per_view = torch.stack([ref_grid.view_counts_reference(c2w[v:v + 1], H, W, Ks[v:v + 1], NEAR, FAR).reshape(-1) for v in range(6)])
    print(f"\ncells seen per camera {per_view.sum(-1).tolist()}, carved {int(occ._unpack_bits(carved, ref_grid.n_cells).sum())} of {ref_grid.n_cells}")
    assert int(per_view[3].sum()) == 0 and int(per_view[4].sum()) == 0 and all(int(per_view[v].sum()) > 1000 for v in (0, 1, 2, 5))
    assert 1000 < int(occ._unpack_bits(carved, ref_grid.n_cells).sum()) < ref_grid.n_cells - 1000
    assert ref_grid.n_cells % 32 == 23 and ref_grid.n_cells % 64 == 55

    grid = npa.OccupancyGrid(LO, HI, RES, device=dev)
    desc = grid._desc()
    cams, _, _, near_m, far_m, m, _ = occ._view_inputs("test", c2w, H, W, Ks, NEAR, FAR, 0.5, masks)
    cams, sat = cams.to(dev), occ._mask_sat(masks.to(dev))
    n_words = grid.bits.numel()

    def run(chunks, with_sat):
        seen = torch.full((grid.n_cells,), -7, dtype=torch.int32, device=dev)
        words = torch.full((n_words,), -1, dtype=torch.int32, device=dev) if with_sat else None
        for n, (a, b) in enumerate(chunks):
            hb.occ_view_carve(desc, grid.width, cams[a:b].contiguous(), H, W, near_m, far_m, m, sat[a:b].contiguous() if with_sat else None,
                              seen, words, accumulate=n > 0)
        return seen.cpu(), None if words is None else words.cpu()
    for chunks in ([(0, 6)], [(0, 4), (4, 6)]):
        seen, words = run(chunks, True)
        assert torch.equal(seen, count), (chunks, int((seen != count).sum()))
        assert torch.equal(words, carved), (chunks, int((words != carved).sum()))
        assert int(words[-1]) >> 23 == 0                    # the unused bits of the last word
        seen, words = run(chunks, False)
        assert torch.equal(seen, count) and words is None, chunks
    # the public forms, the views in chunks of one table each
    keep_bytes, occ._SAT_BYTES = occ._SAT_BYTES, 4 * (H + 1) * (W + 1)
    try:
        assert torch.equal(grid.view_counts(c2w, H, W, Ks, NEAR, FAR).cpu().reshape(-1), count)
        assert torch.equal(occ._pack_bits(grid.carved(c2w, H, W, Ks, NEAR, FAR, masks).reshape(-1)).cpu(), carved)
    finally:
        occ._SAT_BYTES = keep_bytes
    assert torch.equal(occ._pack_bits(grid.carved(c2w, H, W, Ks, NEAR, FAR, masks).reshape(-1)).cpu(), carved)
    with pytest.raises(hb.NerfHipError, match="come together"):
        hb.occ_view_carve(desc, grid.width, cams, H, W, near_m, far_m, m, sat, torch.empty(grid.n_cells, dtype=torch.int32, device=dev), None)


def test_from_views_equals_the_reference(npa, dev, reference):
    ref_grid, c2w, Ks, masks, count, _ = reference
    for kw in (dict(masks=masks), dict(), dict(masks=masks, min_views=2), dict(min_views=3, margin_px=2.0)):
        got = npa.OccupancyGrid.from_views(c2w, H, W, Ks, NEAR, FAR, LO, HI, RES, device=dev, **kw)
        want = ref_grid.views_keep_reference(c2w, H, W, Ks, NEAR, FAR, **kw)
        assert got.bits.is_cuda and torch.equal(got.to_mask().cpu(), want), kw
        assert 0 < int(want.sum()) < want.numel(), kw
    want = ref_grid.views_keep_reference(c2w, H, W, Ks, NEAR, FAR, masks=masks)
    grown = torch.nn.functional.max_pool3d(want[None, None].float(), 3, 1, 1)[0, 0] > 0
    got = npa.OccupancyGrid.from_views(c2w, H, W, Ks, NEAR, FAR, LO, HI, RES, masks=masks, dilate=1, outside="skip", device=dev)
    assert torch.equal(got.to_mask().cpu(), grown) and got.outside == "skip"
    # restrict on a plain grid on the GPU: one AND
    plain = npa.OccupancyGrid(LO, HI, RES, device=dev).restrict(got)
    assert torch.equal(plain.bits, got.bits)


def hull_cameras():
    """the cameras of the ball scene: the batch's own at (0, 0, 4) looking down -z and a ring of 8 at radius 4, 30 degrees up, 64 x 64
    pixels; silhouettes of a ball of radius 1"""
    c2w = torch.cat([look_at((0.0, 0.0, 4.0), world_up=(0.0, 1.0, 0.0))[None], ring(8)])
    Kh = torch.tensor([[70.0, 0.0, 32.0], [0.0, 70.0, 32.0], [0.0, 0.0, 1.0]])
    masks = torch.stack([sphere_silhouette(c, Kh, 64, 64, radius=1.0) for c in c2w])
    return c2w, Kh, masks


def test_restrict_to_views_survives_an_update(npa, dev, nets):
    nf = nets[1]
    c2w, Kh, masks = hull_cameras()
    thr = positive_median_density(npa, nf, dev, BOX_R)
    g = npa.DensityGrid(BOX_LO, BOX_HI, BOX_R, device=dev, sigma_threshold=thr, dilate=1)
    assert g.restrict_to_views(c2w, 64, 64, Kh, 2.0, 6.0, masks=masks) is g
    hull = npa.OccupancyGrid(BOX_LO, BOX_HI, BOX_R, device=CPU).views_keep_reference(c2w, 64, 64, Kh, 2.0, 6.0, masks=masks)
    assert torch.equal(g.to_mask().cpu(), hull) and torch.equal(g.keep, g.bits) and 0.02 < g.fraction_occupied() < 0.3
    free = npa.DensityGrid(BOX_LO, BOX_HI, BOX_R, device=dev, sigma_threshold=thr, dilate=1).update(nf)
    g.update(nf)
    assert torch.equal(g.bits, g._bits_reference()) and torch.equal(g.bits, free.bits & g.keep)
    assert 0 < int(g.to_mask().sum()) < int(free.to_mask().sum()) and not bool((g.to_mask().cpu() & ~hull).any())
    state = g.state_dict()
    h = npa.DensityGrid(BOX_LO, BOX_HI, BOX_R, device=dev).load_state_dict(state)
    assert h.keep.is_cuda and torch.equal(h.keep, g.keep) and torch.equal(h.update(nf).bits, g.bits)
    assert torch.equal(g.restrict(None).bits, free.bits) and g.keep is None


def test_a_training_step_through_the_hull_during_the_warm_up(npa, dev, nets):
    """render_rays(occupancy=a DensityGrid restricted to the hull, never updated), forward and parameter gradients, against the same call
    with a DensityGrid whose bits were set from the hull by hand: bit for bit (256 rays, 64 + 128 samples, fp16x3), and the grid skips"""
    c2w, Kh, masks = hull_cameras()
    prev = npa.get_precision()
    npa.set_precision("fp16x3")
    try:
        nc, nf = fresh_nets(npa, dev, nets)
        rays = orc.synthetic_rays(256, seed=21).to(dev)
        rnd = {k: v.to(dev) for k, v in orc.synthetic_randoms(256, 64, 128, seed=22).items()}
        target = scene_target(dev, 256)
        restricted = npa.DensityGrid(BOX_LO, BOX_HI, BOX_R, device=dev).restrict_to_views(c2w, 64, 64, Kh, 2.0, 6.0, masks=masks)
        assert not restricted.maybe_update(nf, 0) and restricted.n_updates == 0        # the warm-up
        by_hand = npa.DensityGrid(BOX_LO, BOX_HI, BOX_R, device=dev)
        by_hand.bits = npa.OccupancyGrid.from_views(c2w, 64, 64, Kh, 2.0, 6.0, BOX_LO, BOX_HI, BOX_R, masks=masks, device=dev).bits.clone()
        kw = dict(N_samples=64, N_importance=128, network_fine=nf, white_bkgd=True, perturb=1.0, raw_noise_std=1.0, randoms=rnd, retraw=True)
        runs = []
        for grid in (restricted, by_hand):
            zero_grads(nc, nf)
            out = npa.render_rays(rays, nc, None, occupancy=grid, **kw)
            loss_of(npa, out, target).backward()
            runs.append((out, grads_of(nc), grads_of(nf), dict(grid.last_stats)))
        zero_grads(nc, nf)
    finally:
        npa.set_precision(prev)
    (a, ac, af, sa), (b, bc, bf, sb) = runs
    assert list(a) == list(b) and all(bits_equal(a[k].detach(), b[k].detach()) for k in a)
    assert all(bits_equal(x, y) for x, y in zip(ac + af, bc + bf)) and float(torch.cat([g.reshape(-1) for g in ac]).abs().max()) > 0
    print(f"\nevaluated {sa['evaluated']} of {sa['total']} samples through the hull")
    assert sa == sb and 0 < sa["evaluated"] < sa["total"] and sa["total"] == 256 * 256
