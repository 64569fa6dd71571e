"""CPU: the four march references (OccupancyGrid.march_reference / march_step_reference, DensityGrid.march_stop_reference /
march_step_stop_reference) against what they returned before they were put on one shared walk -- tests/golden/march_references.npz,
written by tests/golden/make_golden_march.py at the commit in front of that change.  Bit for bit: fp32 as int32, flags and levels exactly."""
import os

import numpy as np
import pytest
import torch

from test_march_stop_cpu import ball_density_grid

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "march_references.npz")
SHAPES = ((1, 1), (7, 2), (65, 64), (130, 9))


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as f:
        return {k: f[k] for k in f.files}


def same_bits(got, want):
    got = got.detach().contiguous()
    return got.dtype == torch.float32 and want.dtype == np.float32 and got.shape == want.shape and np.array_equal(
        got.view(torch.int32).numpy(), want.view(np.int32))


@pytest.mark.parametrize("M,S", SHAPES)
@pytest.mark.parametrize("outside", ["skip", "evaluate"])
def test_the_march_references_return_what_they_returned(golden, outside, M, S):
    grid = ball_density_grid(outside)
    assert float(grid.density.double().sum()) == float(golden[f"density_checksum/{outside}"])
    key = f"{outside}/{M}x{S}"
    rays, u, eps = torch.from_numpy(golden[f"rays/{key}"]), torch.from_numpy(golden[f"u/{key}"]), float(golden["eps"])
    assert rays.shape == (96, 8) and u.shape == (96,) and eps == 1e-2
    names = [str(c) for c in golden["cases"]]
    assert len(names) == 20 and len(set(names)) == 20
    seen = set()
    for i, name in enumerate(names):
        form, tag, *rest = name.split()
        uu = {"u": u, "none": None}[tag]
        want_z, want_stop, want_flags = golden[f"z_vals/{key}"][i], golden[f"z_stop/{key}"][i], golden[f"flags/{key}"][i]
        if form == "march":
            z, z_stop, tr = grid.march_reference(rays, uu, M, S)
            st = lv = None
        elif form == "march_stop":
            z, z_stop, tr, st = grid.march_stop_reference(rays, uu, M, S, eps)
            lv = None
        elif form == "step":
            z, z_stop, tr, lv = grid.march_step_reference(rays, uu, float(rest[0]), M, S, int(rest[1]))
            st = None
        else:
            assert form == "step_stop"
            z, z_stop, tr, lv, st = grid.march_step_stop_reference(rays, uu, float(rest[0]), M, S, eps, int(rest[1]))
        seen.add((form, tag) + tuple(rest))
        assert same_bits(z, want_z), (key, name)
        assert same_bits(z_stop, want_stop), (key, name)
        assert tr.dtype == torch.bool and np.array_equal(tr.numpy(), want_flags[:, 0] != 0), (key, name)
        if st is None:
            assert not want_flags[:, 1].any()
        else:
            assert st.dtype == torch.bool and np.array_equal(st.numpy(), want_flags[:, 1] != 0), (key, name)
        if lv is None:
            assert not want_flags[:, 2].any()
        else:
            assert lv.dtype == torch.int32 and np.array_equal(lv.numpy(), want_flags[:, 2].astype(np.int32)), (key, name)
    steps = {(f, t, ds, fit) for f in ("step", "step_stop") for t in ("u", "none") for ds in ("0.015625", "0.37") for fit in ("0", "3")}
    assert seen == {(f, t) for f in ("march", "march_stop") for t in ("u", "none")} | steps
