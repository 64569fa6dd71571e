"""Triangle meshes of the fixture fine network (nerf_iso_count / nerf_iso_emit, mesh.py) on one MI355X, at 128^3 and 256^3 nodes over
[-2, 2]^3, the level at the median of the positive node densities:
  * density_volume (the network at every node);
  * the two entry points alone -- the four count launches, the two emit launches -- HIP events around back-to-back calls;
  * extract_mesh end to end (the counts' read-back and the allocation of the outputs included), V, F and the scratch bytes;
  * at 128^3 the torch definition (extract_mesh_reference) on the same GPU beside it: the only baseline there is;
  * DensityGrid.extract_mesh on the share-0.25 ball grid of the other grid scripts carrying one update's densities, at sigma_threshold.

    python tools/exp_mesh.py --out profiles/r22_exp_mesh.json
"""
import grid_exp as gx

ap = gx.parser(__doc__)
args = ap.parse_args()
torch, wl, npa, hb, dev = gx.load(args, "exp_mesh")
S = gx.Scene(wl, npa, dev, perturb=0.)
mesh = npa.mesh

result = {"tree": args.label, "box": [S.LO[0], S.HI[0]], "precision": "fp16x3", "level": "median of the positive node densities"}
for n in (128, 256):
    row = {}
    row["density_volume_ms"] = gx.row_stats(gx.time_alternating([("v", lambda: npa.density_volume(S.nf, S.LO, S.HI, n))], 1, args.reps, warmup=1)["v"])
    volume = npa.density_volume(S.nf, S.LO, S.HI, n)
    level = float(volume[volume > 0].median())
    _, level32, lo32, step32 = mesh._lattice("exp_mesh", volume, level, S.LO, S.HI)
    counts, scratch = hb.iso_count(volume, level32)
    V, F = counts.tolist()
    row.update(level=level, vertices=V, faces=F, scratch_bytes=4 * hb.lib().nerf_iso_scratch_words(n, n, n))
    row["iso_count_us (edges + scan + cubes + scan)"] = gx.time_launches(lambda: hb.iso_count(volume, level32), args.reps, launches=20)
    row["iso_emit_us (vertices + faces)"] = gx.time_launches(lambda: hb.iso_emit(volume, level32, lo32, step32, None, scratch, V, F), args.reps,
                                                             launches=20)
    row["extract_mesh_ms"] = gx.row_stats(gx.time_alternating([("m", lambda: npa.extract_mesh(volume, level, S.LO, S.HI))], 1, args.reps,
                                                              warmup=1)["m"])
    if n == 128:
        v, f = npa.extract_mesh(volume, level, S.LO, S.HI)
        v_ref, f_ref = npa.extract_mesh_reference(volume, level, S.LO, S.HI)
        row["equals_the_torch_reference"] = bool(torch.equal(f, f_ref) and torch.equal(v.view(torch.int32), v_ref.view(torch.int32)))
        row["extract_mesh_reference_on_the_gpu_ms"] = gx.row_stats(gx.time_alternating(
            [("r", lambda: npa.extract_mesh_reference(volume, level, S.LO, S.HI))], 1, args.reps, warmup=1)["r"])
    result[f"{n}^3 nodes"] = row
    del volume, scratch

# ---- the grid's own preview
def share_of(grid):
    torch.manual_seed(0)
    with torch.no_grad():
        S.render(occupancy=grid)
    return gx.evaluated_share(grid)


g, radius = S.ball_with_share(npa.DensityGrid, share_of, 0.25)
with torch.no_grad():
    g.density = npa.DensityGrid(S.LO, S.HI, S.R, device=dev).update(S.nf).density
v, f = g.extract_mesh()
result["DensityGrid.extract_mesh, share 0.25"] = dict(
    gx.row_stats(gx.time_alternating([("g", g.extract_mesh)], 1, args.reps, warmup=1)["g"]), ball_radius=radius, grid_resolution=S.R,
    sigma_threshold=g.sigma_threshold, vertices=v.shape[0], faces=f.shape[0], fraction_occupied=g.fraction_occupied())
gx.emit(result, args.out)
