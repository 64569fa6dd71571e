"""The sparse delta chain's prologue (-m gpu): bwd_prologue_kernel -- the pass over d_raw (maximum, liveness bitmap) and the
replication of the per-ray direction encoding in one launch -- against the launches it replaces, delta_amax_kernel<true> and
replicate_dir_bf16_kernel, which the same library still runs with NERF_BWD_FOLD_LAUNCHES=0 in the
environment (read per call).  live_scan_kernel follows in both forms.

Everything is compared as words: the live buffer (header, list up to the count, bitmap, prefix words), the four scale words of the
delta buffer, the replicated directions in the save buffer (hi and, for fp16x3w, lo mirror) and, since they come for free, the
gradients.  List words behind the count and every word the kernels do not own must keep the poison the test put there, in both forms.
"""
import pytest
import torch

import nerf_oracle as orc
from test_gpu_parity import dev, nets, npa  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

POISON = 0x5A5A5A5A
SHAPES = [(3, 64), (37, 5), (33, 192)]      # 6 tiles; 185 points: ragged last tile and bitmap word; 198 tiles: seven bitmap words


def patterns(n, S, dev_):
    """d_raw [n, S, 4] per name; tiles are 32 consecutive points of the flattened launch"""
    g = torch.Generator().manual_seed(100 * n + S)
    base = (torch.randn(n * S, 4, generator=g) * 1e-3).to(dev_)
    tile = torch.arange(n * S, device=dev_) // 32
    out = {"all dead": torch.zeros_like(base), "all live": base.clone()}
    alt = base.clone()
    alt[tile % 2 == 0] = 0.0
    out["alternating tiles"] = alt
    # tiles 0, 2, 4 are dead in `alt`: a -0 word keeps tile 0 dead, a subnormal revives tile 2, a NaN tile 4
    odd = alt.clone()
    odd[5, 1] = -0.0
    odd.view(torch.int32)[2 * 32 + 7, 2] = 1
    odd[4 * 32 + 31 if n * S > 4 * 32 + 31 else n * S - 1, 3] = float("nan")
    out["-0, subnormal, NaN"] = odd
    return {k: v.view(n, S, 4).contiguous() for k, v in out.items()}


class Pass:
    """one saved forward and the buffers every backward of the test reuses"""

    def __init__(self, npa, dev_, net, n, S, precision):
        self.hb, self.net, self.n, self.S, self.precision = npa.hip_backend, net, n, S, precision
        hb = self.hb
        g = torch.Generator().manual_seed(7 * n + S)
        rays = orc.synthetic_rays(n, seed=3).to(dev_)
        z = torch.sort(torch.rand(n, S, generator=g) * 4 + 2, -1)[0].to(dev_)
        _, self.act = hb.field_fwd(net.packed_params(precision), rays, z, save_act=True, precision=precision)
        L = hb.lib()
        self.delta = torch.zeros(max(L.nerf_delta_floats(n, S), hb.delta_floats(n, S, precision)), device=dev_)
        self.partial = torch.zeros(L.nerf_wgrad_partial_floats(n, S), device=dev_)
        self.two = precision == "fp16x3w"
        self.act_reg = hb.buffer_regions(n, S, 2 if self.two else 1)
        self.scale = hb.buffer_regions(n, S, 2 if self.two else 1, is_delta=True)["scale"]
        self.words = L.nerf_live_tiles_words(n, S)

    def dir_words(self):
        """the [ray][feature][8 copies] records (hi, lo), or the whole per-point region when the samples do not fill whole tiles"""
        a = self.act.view(torch.int32)
        size = max(self.n * 32 * 4, ((self.n * self.S + 31) // 32 * 32) * 16)
        offs = [self.act_reg["dir_pt"]] + ([self.act_reg["lo"] + self.act_reg["dir_pt"]] if self.two else [])
        return [a[o:o + size] for o in offs]

    def run(self, d_raw, fused, monkeypatch, accumulate=False):
        hb = self.hb
        monkeypatch.setenv("NERF_BWD_FOLD_LAUNCHES", "1" if fused else "0")
        live_buf = hb.live_list(self.n, self.S, d_raw.device)
        live_buf[:self.words].fill_(POISON)
        for w in self.dir_words():
            w.fill_(POISON)
        self.delta.view(torch.int32)[self.scale:self.scale + 4].fill_(POISON)
        if accumulate:
            grad = torch.randn(hb.N_PARAMS, generator=torch.Generator().manual_seed(5)).to(d_raw.device)
        else:
            grad = torch.full((hb.N_PARAMS,), float("nan"), device=d_raw.device)
        hb._field_bwd(hb.lib(), self.net.packed_params(self.precision), self.act, d_raw, grad, accumulate, self.precision, self.delta,
                      self.partial, self.n, self.S, self.net.flat_params())
        assert hb.LAST_LIVE is live_buf
        return {"live": live_buf[:self.words].clone(), "scale": self.delta.view(torch.int32)[self.scale:self.scale + 4].clone(),
                "dirs": [w.clone() for w in self.dir_words()], "grad": grad.view(torch.int32).clone()}


def assert_same(ps, old, new, d_raw, what):
    T = (ps.n * ps.S + 31) // 32
    n_words = (T + 31) // 32
    count = int(old["live"][0])
    bits = d_raw.reshape(-1, 4).view(torch.int32) & 0x7FFFFFFF
    pad = torch.zeros(T * 32, 4, dtype=torch.int32, device=d_raw.device)
    pad[:bits.shape[0]] = bits
    want = torch.nonzero((pad.view(T, 128) != 0).any(1)).flatten().to(torch.int32)
    for name, r in (("separate", old), ("fused", new)):
        lv = r["live"]
        assert lv[:4].tolist() == [want.numel(), T, 0, 0], f"{what} [{name}]: header {lv[:4].tolist()}"
        assert torch.equal(lv[4:4 + count], want), f"{what} [{name}]: list"
        assert bool((lv[4 + count:4 + T] == POISON).all()), f"{what} [{name}]: list words behind the count were written"
        assert int(lv[4 + T + n_words + n_words]) == count, f"{what} [{name}]: last prefix word"
    assert torch.equal(old["live"], new["live"]), f"{what}: live buffers differ"
    assert torch.equal(old["scale"], new["scale"]), f"{what}: scale words {old['scale'].tolist()} vs {new['scale'].tolist()}"
    if ps.precision != "bf16x3":
        flat = d_raw.reshape(-1)
        amax = flat[~torch.isnan(flat)].abs().max().view(torch.int32)
        assert new["scale"].tolist() == [int(amax), 0, 0, 0], f"{what}: scale words {new['scale'].tolist()}"
    else:       # (bf16 parts carry no scale: nobody touches the four words)
        assert new["scale"].tolist() == [POISON] * 4, f"{what}: scale words of the bf16 split"
    # (the prologue replicates only when a ray's samples fill whole tiles; otherwise the per-point expansion is the weight-gradient call's, unchanged)
    written = ps.n * 32 * 4 if ps.S % 32 == 0 else 0
    for a, b in zip(old["dirs"], new["dirs"]):
        assert not bool((b[:written] == POISON).any()), f"{what}: direction records not written"
        assert torch.equal(a, b), f"{what}: replicated directions differ"
    assert torch.equal(old["grad"], new["grad"]), f"{what}: gradients differ"


@pytest.mark.parametrize("precision", ["fp16x3", "fp16x3w", "bf16x3"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_prologue_equals_the_separate_launches(npa, dev, nets, precision, shape, monkeypatch):
    n, S = shape
    ps = Pass(npa, dev, nets[1], n, S, precision)
    try:
        for what, d_raw in patterns(n, S, dev).items():
            old = ps.run(d_raw, False, monkeypatch)
            new = ps.run(d_raw, True, monkeypatch)
            assert_same(ps, old, new, d_raw, f"{n}x{S} {precision} {what}")
    finally:
        ps.hb.WORKSPACE.give(ps.act)


def test_same_buffers_three_times_in_a_row(npa, dev, nets, monkeypatch):
    """the maximum word is re-armed by every call: three fused passes on the same delta / live buffers, each with another pattern
    and no poison in between, leave what the separate launches leave"""
    n, S, precision = 33, 192, "fp16x3"
    ps = Pass(npa, dev, nets[1], n, S, precision)
    try:
        pats = patterns(n, S, dev)
        order = ["all live", "alternating tiles", "all dead"]
        olds = {k: ps.run(pats[k], False, monkeypatch, accumulate=True) for k in order}
        hb = ps.hb
        monkeypatch.setenv("NERF_BWD_FOLD_LAUNCHES", "1")
        for k in order:
            grad = torch.randn(hb.N_PARAMS, generator=torch.Generator().manual_seed(5)).to(dev)
            hb._field_bwd(hb.lib(), ps.net.packed_params(precision), ps.act, pats[k], grad, True, precision, ps.delta, ps.partial, n, S,
                          ps.net.flat_params())
            live = hb.LAST_LIVE[:ps.words]
            T = (n * S + 31) // 32
            count = int(olds[k]["live"][0])
            assert torch.equal(live[:4 + count], olds[k]["live"][:4 + count]), k
            assert torch.equal(live[4 + T:], olds[k]["live"][4 + T:]), k
            assert torch.equal(ps.delta.view(torch.int32)[ps.scale:ps.scale + 4], olds[k]["scale"]), k
            assert torch.equal(grad.view(torch.int32), olds[k]["grad"]), k
    finally:
        ps.hb.WORKSPACE.give(ps.act)
