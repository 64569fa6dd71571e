"""CPU tests of the two pure helpers under render._backward, the one backward of render_rays' dense and grid autograd nodes:
_sub_chunks (how a ray chunk is cut into sub-chunks, for both forwards and the dense node's recompute plan) and _upstream (which output's
upstream gradient belongs to which pass).  The expected values are the expressions both nodes carried before they shared these helpers,
written out here literally."""
import itertools
import sys
from types import SimpleNamespace

import pytest

import nerf_pytorch_amd  # noqa: F401

render = sys.modules["nerf_pytorch_amd.render"]

SUB_CHUNK_CASES = [(1, 1024), (160, 1024), (1024, 1024), (1025, 1024), (65, 64), (2500, 1024), (160, 64), (32768, 22528), (32768, 10240),
                   (4096, 1024), (200, 100)]


def formula(n, sub):
    """both forwards' text before _sub_chunks: the sub-chunk size and the tiles of a chunk of n > sub rays"""
    ceil_div = lambda a, b: -(-a // b)
    sub = min(sub, 64 * ceil_div(ceil_div(n, ceil_div(n, sub)), 64))        # equal sub-chunks, multiples of 64 rays
    return sub, [(lo, min(lo + sub, n)) for lo in range(0, n, sub)]


@pytest.mark.parametrize("n,sub", SUB_CHUNK_CASES)
def test_sub_chunks_cover_the_rays_in_equal_multiples_of_64(n, sub):
    got_sub, tiles = render._sub_chunks(n, sub)
    assert tiles[0][0] == 0 and tiles[-1][1] == n
    assert all(a[1] == b[0] for a, b in zip(tiles, tiles[1:])) and all(lo < hi for lo, hi in tiles)       # no gap, no overlap, none empty
    assert all(hi - lo <= sub for lo, hi in tiles)
    if n <= sub:        # one tile, and the size the caller gave stays what the plan reports
        assert (got_sub, tiles) == (sub, [(0, n)])
        return
    assert (got_sub, tiles) == formula(n, sub)
    sizes = [hi - lo for lo, hi in tiles]
    assert len(tiles) > 1 and set(sizes[:-1]) == {got_sub} and sizes[-1] <= got_sub
    assert got_sub % 64 == 0 or got_sub == sub      # (a sub that is no multiple of 64 itself caps the rounded size)
    assert render._sub_chunks(n, got_sub) == (got_sub, tiles)       # the recompute plan cuts the same tiles from the size the forward reported


def test_sub_chunks_of_the_documented_sizes():
    assert render._sub_chunks(2500, 1024) == (896, [(0, 896), (896, 1792), (1792, 2500)])
    assert render._sub_chunks(160, 64) == (64, [(0, 64), (64, 128), (128, 160)])
    assert render._sub_chunks(1025, 1024) == (576, [(0, 576), (576, 1025)])
    sub, tiles = render._sub_chunks(32768, 22528)
    assert sub == 16384 and tiles == [(0, 16384), (16384, 32768)]


# every output layout of the two nodes: (name, N_importance, coarse_image, the outputs in front of the trailing losses)
LAYOUTS = [("coarse_only", 0, True, ("rgb", "disp", "acc", "raw")),
           ("two_passes", 24, True, ("rgb", "disp", "acc", "raw", "rgb0", "disp0", "acc0", "z_std")),
           ("grid_proposal", 24, False, ("rgb", "disp", "acc", "raw", "z_std"))]
UPSTREAM_CASES = [(name, dist, inter) for (name, *_), dist, inter in itertools.product(LAYOUTS, (False, True), (False, True))
                  if not inter or name == "two_passes"]       # render_rays refuses interlevel without a coarse pass and a refining one


@pytest.mark.parametrize("name,dist,inter", UPSTREAM_CASES)
def test_upstream_sorts_every_output_gradient_to_its_pass(name, dist, inter):
    _, n_f, coarse_image, outputs = next(l for l in LAYOUTS if l[0] == name)
    outputs = outputs + (("distortion",) if dist else ()) + (("interlevel",) if inter else ())
    g = {k: object() for k in outputs}      # distinct sentinels: nothing is read from them
    gouts = tuple(g[k] for k in outputs)
    cfg = SimpleNamespace(N_importance=n_f, distortion=dist, interlevel=inter)
    up_c, up_f = render._upstream(cfg, gouts, coarse_image)
    # (rgb, disp, acc, raw, distortion, interlevel) per pass: the distortion loss with the last pass, the interlevel loss with the coarse one
    last = (g["rgb"], g["disp"], g["acc"], g["raw"], g.get("distortion"), None)
    if name == "coarse_only":
        want_c, want_f = last, None
    elif name == "two_passes":
        want_c, want_f = (g["rgb0"], g["disp0"], g["acc0"], None, None, g.get("interlevel")), last
    else:
        want_c, want_f = None, last
    for got, want in ((up_c, want_c), (up_f, want_f)):
        assert (got is None) == (want is None)
        if want is not None:
            assert len(got) == 6 and all(a is b for a, b in zip(got, want))


@pytest.mark.parametrize("name,dist,inter", UPSTREAM_CASES)
def test_upstream_equals_the_nodes_former_expressions(name, dist, inter):
    _, n_f, coarse_image, outputs = next(l for l in LAYOUTS if l[0] == name)
    gouts = tuple(object() for _ in outputs + (("distortion",) if dist else ()) + (("interlevel",) if inter else ()))
    cfg = SimpleNamespace(N_importance=n_f, distortion=dist, interlevel=inter)
    fine = n_f > 0
    up_f = (gouts[0], gouts[1], gouts[2], gouts[3], gouts[-2 if inter else -1] if dist else None, None)
    if not coarse_image:
        up_c = None
    else:
        up_c = (gouts[4], gouts[5], gouts[6], None, None, gouts[-1] if inter else None) if fine else None
    if not fine:
        up_c, up_f = up_f, None
    assert render._upstream(cfg, gouts, coarse_image) == (up_c, up_f)
