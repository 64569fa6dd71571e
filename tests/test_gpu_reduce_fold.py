"""Chunk reduction and folded feature layer in one grid (-m gpu): wgrad_reduce_fold_kernel against wgrad_reduce_kernel +
wgrad_fold_kernel of the same library (NERF_BWD_FOLD_LAUNCHES=0 in the environment, read per call).

The fold workgroups sum their own slices of the chunk partials in the reduction's order and run the fold's FMA chains term for
term, so the gradients of one field_bwd are compared as words: every tensor, with `accumulate` off (onto NaN) and on (onto noise),
through the sparse and the dense backward.  5 x 64 = 320 points: two chunks of partial sums; 37 x 5 = 185: one, ragged.
"""
import pytest
import torch

import nerf_oracle as orc
from test_gpu_parity import dev, nets, npa  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu


def one_bwd(hb, net, act, d_raw, precision, accumulate, sparse):
    n, S, _ = d_raw.shape
    if accumulate:
        grad = torch.randn(hb.N_PARAMS, generator=torch.Generator().manual_seed(11)).to(d_raw.device)
    else:
        grad = torch.full((hb.N_PARAMS,), float("nan"), device=d_raw.device)
    prev = hb.BWD_SKIP_DEAD
    hb.BWD_SKIP_DEAD = sparse
    try:
        hb.field_bwd(net.packed_params(precision), act, d_raw, grad, accumulate, precision=precision, params=net.flat_params())
    finally:
        hb.BWD_SKIP_DEAD = prev
    return grad


@pytest.mark.parametrize("precision", ["fp16x3", "bf16x3", "fp16x3w"])
@pytest.mark.parametrize("shape", [(5, 64), (37, 5)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_one_grid_equals_reduce_then_fold(npa, dev, nets, precision, shape, monkeypatch):
    hb = npa.hip_backend
    net = nets[1]
    n, S = shape
    g = torch.Generator().manual_seed(13 * n + S)
    rays = orc.synthetic_rays(n, seed=3).to(dev)
    z = torch.sort(torch.rand(n, S, generator=g) * 4 + 2, -1)[0].to(dev)
    d_raw = (torch.randn(n, S, 4, generator=g) * 1e-3).to(dev)
    d_raw.view(-1, 4)[64:128] = 0.0         # (two dead tiles: the sparse backward has something to skip)
    _, act = hb.field_fwd(net.packed_params(precision), rays, z, save_act=True, precision=precision)
    try:
        for sparse in (True, False):
            for accumulate in (False, True):
                grads = {}
                for fused in ("0", "1"):
                    monkeypatch.setenv("NERF_BWD_FOLD_LAUNCHES", fused)
                    grads[fused] = one_bwd(hb, net, act, d_raw, precision, accumulate, sparse)
                assert bool(torch.isfinite(grads["1"]).all())
                for nm, off, shp in hb.param_table():
                    k = 1
                    for s in shp:
                        k *= int(s)
                    a, b = grads["0"][off:off + k].view(torch.int32), grads["1"][off:off + k].view(torch.int32)
                    assert torch.equal(a, b), f"{nm} [{precision}, accumulate={accumulate}, sparse={sparse}]: {int((a != b).sum())} of {k} words differ"
    finally:
        hb.WORKSPACE.give(act)
