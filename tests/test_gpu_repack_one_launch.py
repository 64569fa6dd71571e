"""The one-launch repack of two networks (-m gpu): pack3_fused_kernel against derive_folded_kernel + pack3_all_kernel of the same
library (NERF_BWD_FOLD_LAUNCHES=0 in the environment, read per call).

The fused kernel's workgroups compute the folded matrix W' = Wv[:, :256] Wf and b' themselves, in fp64 in derive_folded_kernel's
order, and round once: the whole packed buffer of either network -- both fragment streams, the small parameters, the `derived`
region -- is compared word for word, on buffers poisoned beforehand (a word neither form writes keeps the poison in both).  The
parameters are such that fp32 accumulation of W' would round differently from fp64 in many entries (checked here), so a kernel
that accumulated in fp32 could not pass.  The kernel relies on the lo word of a W' element sitting 512 elements behind its hi word
with the same source: checked against the library's own tables.
"""
import ctypes

import numpy as np
import pytest
import torch

from test_gpu_parity import dev, npa  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

POISON = 0x5A5A5A5A


def test_lo_words_of_the_folded_units_sit_512_elements_behind_their_hi_words(npa):
    hb = npa.hip_backend
    L = hb.lib()
    n_params = hb.N_PARAMS
    for fn in (L.nerf_debug_pack16_table, L.nerf_debug_pack3_table):
        tab = (ctypes.c_int * (2 * L.nerf_packed3_floats()))()
        assert fn(tab) == 0
        t = np.frombuffer(tab, dtype=np.int32)
        folded = np.nonzero(t >= 2 * n_params)[0]
        assert folded.size == 2 * 128 * 256 and folded.size == folded[-1] - folded[0] + 1 and folded[0] % 1024 == 0
        g = t[folded].reshape(-1, 2, 512)
        assert (g[:, 0] % 2 == 0).all() and (g[:, 1] == g[:, 0] + 1).all()
        assert np.unique(g[:, 0]).size == 128 * 256                # every W' element exactly once


@pytest.mark.parametrize("precision", ["fp16x3", "bf16x3"])
def test_one_launch_equals_derive_then_pack(npa, dev, precision, monkeypatch):
    hb = npa.hip_backend
    L = hb.lib()
    dp = hb.DATAPATHS[precision]
    g = torch.Generator().manual_seed(33)
    flats = []
    for scale in (1.0, 37.0):
        flat = torch.randn(hb.N_PARAMS, generator=g) * scale
        flat[::7] *= 1e3                                            # cancellation between large and small terms of a dot product
        flats.append(flat.to(dev))
    # the parameters tell fp32 from fp64 accumulation of W'
    for flat in flats:
        tab = {nm: (off, shape) for nm, off, shape in hb.param_table()}
        (ov, sv), (of, sf) = tab["views_linears.0.weight"], tab["feature_linear.weight"]
        wv = flat[ov:ov + sv[0] * sv[1]].view(*sv)[:, :256]
        wf = flat[of:of + sf[0] * sf[1]].view(*sf)
        w64 = (wv.double() @ wf.double()).float()
        w32 = (wv.cpu() @ wf.cpu()).to(dev)
        assert int((w64 != w32).sum()) > 1000
    out = {}
    for fused in ("0", "1"):
        monkeypatch.setenv("NERF_BWD_FOLD_LAUNCHES", fused)
        bufs = [torch.full((L.nerf_packed3_floats(),), 0, dtype=torch.int32, device=dev).fill_(POISON) for _ in flats]
        hb._check(L.nerf_pack_params_split_pair(flats[0].data_ptr(), bufs[0].data_ptr(), flats[1].data_ptr(), bufs[1].data_ptr(),
                                                dp.pack_streams, dp.pack_split, hb._stream()), "nerf_pack_params_split_pair")
        out[fused] = bufs
    for net in range(2):
        a, b = out["0"][net], out["1"][net]
        assert int((b == POISON).sum()) == int((a == POISON).sum())
        assert torch.equal(a, b), f"network {net}: {int((a != b).sum())} of {a.numel()} packed words differ"
    # one network through the single-network entry point takes the same launch
    for fused in ("0", "1"):
        monkeypatch.setenv("NERF_BWD_FOLD_LAUNCHES", fused)
        buf = torch.zeros(L.nerf_packed3_floats(), dtype=torch.int32, device=dev).fill_(POISON)
        hb._check(L.nerf_pack_params_split(flats[1].data_ptr(), buf.data_ptr(), dp.pack_streams, dp.pack_split, hb._stream()), "nerf_pack_params_split")
        assert torch.equal(buf, out["0"][1])
