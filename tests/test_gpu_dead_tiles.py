"""Dead-tile skipping in the backward of the split datapaths (-m gpu): the sparse forms (nerf_field_dgrad_split_live /
nerf_field_wgrad_phase_live, taken by hip_backend.field_bwd) against the dense forms OF THE SAME BUILD.

A 32-point tile whose d_raw is all +-0 is dead: the delta chain neither computes nor stores it, the weight-gradient GEMM does not
stream it.  Skipping is exact (the deltas of such a tile are exact zeros and add +-0 to sums that start at +0), so everything here
is compared bit for bit: gradients as int32 words, deltas of live tiles region by region, the live list against one computed in
torch.  Dead tiles of the delta buffer must still hold the sentinel the test put there (the contract "a dead tile's deltas are not
written").  With an Inf / NaN saved activation the dense forms give 0 * Inf = NaN where the sparse forms give 0; that only happens
after the fp16 range guard has failed and is not emulated.

Dead-tile shares of the real losses (CPU oracle, 4096-ray batches: lego 0.40-0.41 coarse / 0.30-0.32 fine, 512 fern rays 0.37 /
0.28): the 1024-ray subsets here assert 0.15 <= share <= 0.6 per pass and print the value.
"""
import pytest
import torch

import nerf_oracle as orc
import workloads as wl
from test_gpu_parity import dev, nets, npa  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

SPLITS = ["fp16x3", "fp16x3w", "bf16x3"]
SENTINEL16 = 0x3c5a         # a finite 16-bit pattern in either element type (fp16 1.088, bf16 0.0133)


def torch_live(d_raw):
    """ascending live tile numbers of d_raw [n, S, 4]: a tile is live iff any of its words has (bits & 0x7fffffff) != 0"""
    bits = d_raw.reshape(-1, 4).view(torch.int32) & 0x7fffffff
    P = bits.shape[0]
    T = (P + 31) // 32
    pad = torch.zeros(T * 32, 4, dtype=torch.int32, device=d_raw.device)
    pad[:P] = bits
    return torch.nonzero((pad.view(T, 128) != 0).any(1)).flatten().to(torch.int32)


def chunk_tiles(P):
    """tiles per point chunk of the 12-job weight-gradient plan (csrc/field_bwd.hip, wgrad_chunks)"""
    n = max(1, min(21, (P + 255) // 256))
    pts = ((P + n - 1) // n + 31) // 32 * 32
    return pts // 32


def run_bwd(hb, net, act, d_raw, precision, sparse, accumulate, seed=5):
    """one field backward through the binding's own sequence on buffers we can look at; the delta buffer starts as sentinels"""
    n, S, _ = d_raw.shape
    L = hb.lib()
    dev_ = d_raw.device
    delta = torch.zeros(max(L.nerf_delta_floats(n, S), hb.delta_floats(n, S, precision)), device=dev_)
    delta.view(torch.int16).fill_(SENTINEL16)
    partial = torch.zeros(L.nerf_wgrad_partial_floats(n, S), device=dev_)
    if accumulate:
        grad = torch.randn(hb.N_PARAMS, generator=torch.Generator().manual_seed(seed)).to(dev_)
    else:
        grad = torch.full((hb.N_PARAMS,), float("nan"), device=dev_)
    prev = hb.BWD_SKIP_DEAD
    hb.BWD_SKIP_DEAD = sparse
    try:
        hb._field_bwd(L, net.packed_params(precision), act, d_raw, grad, accumulate, precision, delta, partial, n, S, net.flat_params())
        live = hb.LAST_LIVE
        assert (live is not None) == sparse
        live = live.clone() if sparse else None
    finally:
        hb.BWD_SKIP_DEAD = prev
    return grad, delta, live


def check_pass(hb, net, act, d_raw, precision, what, expect_count=None):
    """dense vs sparse on one (act, d_raw): gradients (plain and accumulated), live list, deltas.  Returns the dead share."""
    n, S, _ = d_raw.shape
    P = n * S
    T = (P + 31) // 32
    want = torch_live(d_raw)
    for accumulate in (False, True):
        gd, dd, _ = run_bwd(hb, net, act, d_raw, precision, False, accumulate)
        gs, ds, live = run_bwd(hb, net, act, d_raw, precision, True, accumulate)
        assert torch.equal(gd.view(torch.int32), gs.view(torch.int32)), f"{what} [{precision}, accumulate={accumulate}]: gradients differ"
    count = int(live[0])
    assert int(live[1]) == T
    assert count == want.numel(), f"{what}: {count} live tiles on the device, {want.numel()} in torch"
    assert torch.equal(live[4:4 + count], want), f"{what}: the live list is not the ascending list of live tiles"
    if expect_count is not None:
        assert count == expect_count, f"{what}: {count} live tiles, the pattern has {expect_count}"
    # deltas: live tiles as the dense run wrote them, dead tiles untouched
    alive_pt = torch.zeros(T * 32, dtype=torch.bool, device=d_raw.device)
    alive_pt.view(T, 32)[want.long()] = True
    alive_pt = alive_pt[:P]
    sentinel = torch.tensor([SENTINEL16], dtype=torch.int16).view(torch.float16 if precision != "bf16x3" else torch.bfloat16).float().item()
    parts = ["hi", "lo"] if precision == "fp16x3w" else ["hi"]
    for region in [f"h{i}" for i in range(8)] + ["hv", "graw"]:
        for part in parts:
            rd = hb.delta_rows(dd, n, S, region, precision, part=part).float()
            rs = hb.delta_rows(ds, n, S, region, precision, part=part).float()
            # (bit patterns: a NaN delta must equal the dense run's NaN)
            assert torch.equal(rd[alive_pt].view(torch.int32), rs[alive_pt].view(torch.int32)), f"{what}: deltas of live tiles differ in {region}.{part}"
            assert bool((rs[~alive_pt] == sentinel).all()), f"{what}: a dead tile of {region}.{part} was written"
    if precision != "bf16x3":
        assert torch.equal(hb.delta_scale_word(dd, n, S), hb.delta_scale_word(ds, n, S))
    return 1.0 - count / T


def saved_pass(npa, dev, net, n_rays, S, precision, seed=3):
    hb = npa.hip_backend
    g = torch.Generator().manual_seed(1000 * n_rays + S)
    rays = orc.synthetic_rays(n_rays, seed=seed).to(dev)
    z = torch.sort(torch.rand(n_rays, S, generator=g) * 4 + 2, -1)[0].to(dev)
    d_raw = (torch.randn(n_rays, S, 4, generator=g) * 1e-3).to(dev)
    _, act = hb.field_fwd(net.packed_params(precision), rays, z, save_act=True, precision=precision)
    return rays, z, d_raw, act


@pytest.mark.parametrize("precision", SPLITS)
def test_constructed_patterns(npa, dev, nets, precision):
    """random d_raw with chosen tiles zeroed, 129 rays x 64 samples (258 tiles, 20 chunks of 13 tiles)"""
    hb = npa.hip_backend
    nf = nets[1]
    n, S = 129, 64
    rays, z, d_raw, act = saved_pass(npa, dev, nf, n, S, precision)
    P, T, ct = n * S, n * S // 32, chunk_tiles(n * S)
    assert T == 258 and ct == 13
    tiles = torch.arange(T, device=dev)

    def masked(keep, fill=0.0):
        d = d_raw.clone().view(T, 32, 4)
        d[~keep] = fill
        return d.view(n, S, 4)

    cases = {
        "every tile dead": (masked(tiles < 0), 0),
        "only the first tile live": (masked(tiles == 0), 1),
        "only the last tile live": (masked(tiles == T - 1), 1),
        "one live tile in the middle of a chunk": (masked(tiles == 3 * ct + 6), 1),
        "alternating tiles": (masked(tiles % 2 == 1), T // 2),
        "a whole chunk dead": (masked((tiles < ct) | (tiles >= 2 * ct)), T - ct),
        "dead tiles made of -0.0": (masked(tiles % 3 == 0, fill=-0.0), (T + 2) // 3),
        "no tile dead": (d_raw, T),
    }
    # ... and dead tiles that mix +0 and -0 words
    mixed = masked(tiles % 2 == 0).view(T, 32, 4)
    mixed[1::2, ::2] = -0.0
    cases["dead tiles of mixed zeros"] = (mixed.view(n, S, 4), (T + 1) // 2)
    try:
        for what, (d, count) in cases.items():
            share = check_pass(hb, nf, act, d.contiguous(), precision, what, expect_count=count)
            print(f"{precision} {what}: dead share {share:.3f}")
    finally:
        hb.WORKSPACE.give(act)


@pytest.mark.parametrize("precision", SPLITS)
def test_nan_word_makes_a_tile_live(npa, dev, nets, precision):
    hb = npa.hip_backend
    nf = nets[1]
    n, S = 129, 64
    rays, z, d_raw, act = saved_pass(npa, dev, nf, n, S, precision)
    T = n * S // 32
    d = torch.zeros_like(d_raw).view(T, 32, 4)
    d[7, 13, 2] = float("nan")
    d[100, 0, 0] = float("inf")
    d[200, 31, 3] = 1e-42            # a subnormal
    d = d.view(n, S, 4)
    try:
        want = torch_live(d)
        assert want.tolist() == [7, 100, 200]
        check_pass(hb, nf, act, d, precision, "NaN / Inf / subnormal words", expect_count=3)
    finally:
        hb.WORKSPACE.give(act)


@pytest.mark.parametrize("precision", SPLITS)
@pytest.mark.parametrize("n_rays,S", [(37, 64), (5, 192), (333, 77), (37, 5), (1, 1)])
def test_ragged_point_counts(npa, dev, nets, precision, n_rays, S):
    """P not a multiple of 128 (37 x 64, 5 x 192: the last workgroup of the delta chain is not full) and not of 32 (333 x 77, 37 x 5,
    1 x 1: the last tile is ragged), with the last tile live and dead"""
    hb = npa.hip_backend
    nf = nets[1]
    rays, z, d_raw, act = saved_pass(npa, dev, nf, n_rays, S, precision)
    P = n_rays * S
    T = (P + 31) // 32
    flat = d_raw.reshape(P, 4)
    tile_of = torch.arange(P, device=dev) // 32
    try:
        for last_live in (True, False):
            d = flat.clone()
            dead = (tile_of % 3 == 1) if T > 1 else torch.zeros(P, dtype=torch.bool, device=dev)
            dead = dead | (tile_of == T - 1) if not last_live else dead & (tile_of != T - 1)
            d[dead] = 0.0
            count = int(torch.unique(tile_of[~dead]).numel())
            check_pass(hb, nf, act, d.view(n_rays, S, 4).contiguous(), precision, f"{n_rays} x {S}, last tile {'live' if last_live else 'dead'}",
                       expect_count=count)
    finally:
        hb.WORKSPACE.give(act)


def _bench_kwargs(cfg, nc, nf):
    return dict(network_query_fn=None, perturb=1.0, N_importance=128, network_fine=nf, N_samples=64, network_fn=nc, use_viewdirs=True,
                white_bkgd=cfg["white_bkgd"], raw_noise_std=cfg["raw_noise_std"], ndc=cfg["ndc"], lindisp=False, near=cfg["near"], far=cfg["far"])


def _fresh_nets(npa, dev, nets):
    kw = dict(D=8, W=256, input_ch=63, output_ch=5, skips=[4], input_ch_views=27, use_viewdirs=True)
    nc, nf = npa.NeRF(**kw).to(dev), npa.NeRF(**kw).to(dev)
    nc.load_state_dict(nets[2])
    nf.load_state_dict(nets[3])
    return nc, nf


@pytest.mark.parametrize("precision", SPLITS)
@pytest.mark.parametrize("config", ["lego", "fern"])
def test_real_training_loss(npa, dev, nets, monkeypatch, precision, config):
    """the d_raw of the bench-shaped loss (render of 1024 rays, both networks, img2mse x 2, perturb = 1): every field backward of
    the step is ALSO run dense and sparse on buffers of the test's own, before the step's own call goes on"""
    hb = npa.hip_backend
    cfg = wl.LEGO if config == "lego" else wl.FERN
    nc, nf = _fresh_nets(npa, dev, nets)
    batch = (wl.lego_batch(1024, seed=0) if config == "lego" else wl.fern_batch(1024, seed=0)).to(dev)
    target = torch.rand(1024, 3, generator=torch.Generator().manual_seed(77)).to(dev)
    shares = {}
    inner = hb._field_bwd

    def spy(L, packed, act, d_raw, grad, accumulate, prec, delta, partial, n, S, params, input_grad=None):
        net = nc if S == 64 else nf
        assert prec == precision
        monkeypatch.setattr(hb, "_field_bwd", inner)
        try:
            shares[S] = check_pass(hb, net, act, d_raw.contiguous(), precision, f"{config} pass of {S} samples")
        finally:
            monkeypatch.setattr(hb, "_field_bwd", spy)
        return inner(L, packed, act, d_raw, grad, accumulate, prec, delta, partial, n, S, params, input_grad)

    prev = npa.get_precision()
    npa.set_precision(precision)
    every = hb.RANGE_MONITOR.every
    hb.RANGE_MONITOR.every = 0          # (a delta scan due would send the step's own call down the dense path: tested below)
    try:
        torch.manual_seed(0)
        rgb, disp, acc, extras = npa.render(cfg["H"], cfg["W"], wl.intrinsics(cfg), chunk=32768, rays=batch, verbose=False, retraw=True,
                                            **_bench_kwargs(cfg, nc, nf))
        loss = npa.img2mse(rgb, target) + npa.img2mse(extras["rgb0"], target)
        monkeypatch.setattr(hb, "_field_bwd", spy)
        loss.backward()
    finally:
        monkeypatch.setattr(hb, "_field_bwd", inner)
        hb.RANGE_MONITOR.every = every
        npa.set_precision(prev)
    assert sorted(shares) == [64, 192], f"field backwards seen: {sorted(shares)}"
    for S, share in sorted(shares.items()):
        print(f"{config} {precision}: dead-tile share of the {'coarse' if S == 64 else 'fine'} pass = {share:.4f}")
        assert 0.15 <= share <= 0.6, f"{config}, pass of {S} samples: dead-tile share {share:.4f}"


@pytest.mark.parametrize("precision", ["fp16x3", "fp16x3w"])
def test_three_adam_steps_switch_on_and_off(npa, dev, nets, precision):
    """three FlatAdam steps of the bench-shaped step leave bit-identical parameters with the switch on and off"""
    hb = npa.hip_backend
    cfg = wl.LEGO
    results = []
    prev = npa.get_precision()
    npa.set_precision(precision)
    prev_skip = hb.BWD_SKIP_DEAD
    try:
        for skip in (True, False):
            hb.BWD_SKIP_DEAD = skip
            nc, nf = _fresh_nets(npa, dev, nets)
            opt = npa.FlatAdam(list(nc.parameters()) + list(nf.parameters()), lr=5e-4, betas=(0.9, 0.999))
            torch.manual_seed(0)
            used = []
            for step in range(3):
                batch = wl.lego_batch(1024, seed=step).to(dev)
                target = torch.rand(1024, 3, generator=torch.Generator().manual_seed(77 + step)).to(dev)
                rgb, disp, acc, extras = npa.render(cfg["H"], cfg["W"], wl.intrinsics(cfg), chunk=32768, rays=batch, verbose=False, retraw=True,
                                                    **_bench_kwargs(cfg, nc, nf))
                opt.zero_grad()
                loss = npa.img2mse(rgb, target) + npa.img2mse(extras["rgb0"], target)
                loss.backward()
                used.append(hb.LAST_LIVE is not None)
                opt.step()
            # the sparse forms ran whenever no delta scan of the range monitor was due (its first step scans)
            assert (any(used) if skip else not any(used)), used
            results.append((nc.flat_params().clone(), nf.flat_params().clone(), loss.detach().clone()))
    finally:
        hb.BWD_SKIP_DEAD = prev_skip
        npa.set_precision(prev)
    for a, b in zip(*results):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize("precision", ["fp16x3", "fp16x3w"])
def test_other_readers_of_the_deltas_get_the_dense_forms(npa, dev, nets, precision):
    """the input gradient and a due range scan read deltas of every tile: field_bwd takes the dense forms for that pass"""
    hb = npa.hip_backend
    nf = nets[1]
    n, S = 129, 64
    rays, z, d_raw, act = saved_pass(npa, dev, nf, n, S, precision)
    T = n * S // 32
    d = d_raw.clone().view(T, 32, 4)
    d[torch.arange(T, device=dev) % 2 == 0] = 0.0
    d = d.view(n, S, 4).contiguous()
    L = hb.lib()
    try:
        ref, _, _ = run_bwd(hb, nf, act, d, precision, False, False)
        # (a) a range scan of the deltas is due
        delta = torch.zeros(max(L.nerf_delta_floats(n, S), hb.delta_floats(n, S, precision)), device=dev)
        delta.view(torch.int16).fill_(SENTINEL16)
        partial = torch.zeros(L.nerf_wgrad_partial_floats(n, S), device=dev)
        grad = torch.full((hb.N_PARAMS,), float("nan"), device=dev)
        assert hb.BWD_SKIP_DEAD
        hb.RANGE_MONITOR.delta_scans_due = 1
        try:
            hb._field_bwd(L, nf.packed_params(precision), act, d, grad, False, precision, delta, partial, n, S, nf.flat_params())
        finally:
            hb.RANGE_MONITOR.delta_scans_due = 0
        assert hb.LAST_LIVE is None
        assert torch.equal(grad.view(torch.int32), ref.view(torch.int32))
        rows = hb.delta_rows(delta, n, S, "h3", precision).float()
        assert bool((rows[:32] == 0).all())                 # tile 0 is dead and WAS written (zeros), as the scan needs
        hb.RANGE_MONITOR.poll(wait=True)
        # (b) the input gradient is requested
        outs = []
        for skip in (True, False):
            prev = hb.BWD_SKIP_DEAD
            hb.BWD_SKIP_DEAD = skip
            try:
                g2 = torch.full((hb.N_PARAMS,), float("nan"), device=dev)
                d_rays = torch.zeros(n, rays.shape[1], device=dev)
                hb.field_bwd(nf.packed_params(precision), act, d, g2, False, precision, params=nf.flat_params(), input_grad=(rays, z, d_rays, False))
                assert hb.LAST_LIVE is None
                outs.append((g2, d_rays))
            finally:
                hb.BWD_SKIP_DEAD = prev
        assert torch.equal(outs[0][0].view(torch.int32), outs[1][0].view(torch.int32)) and torch.equal(outs[0][0].view(torch.int32), ref.view(torch.int32))
        assert torch.equal(outs[0][1].view(torch.int32), outs[1][1].view(torch.int32))
    finally:
        hb.WORKSPACE.give(act)
