"""Pin oracle/nerf_oracle.py against the real reference (build container only).

Imports /root/reference/run_nerf.py with ``imageio`` and ``cv2`` stubbed (they
are used only by loaders / image writers), runs the reference functions and the
oracle restatement on identical inputs on CPU, and asserts bit-identical fp32
results function by function.

``--record tests/golden/oracle_pin.npz`` stores every reference value it compares
against (48 rays); ``tests/test_oracle_golden.py`` replays that fixture
(``main(n_rays=48, golden=...)``): the same comparisons, bit for bit, with the
reference's side read from the file instead of computed.
"""
import hashlib
import os
import sys
import types

import numpy as np
import torch

REF = os.environ.get("NERF_REFERENCE", "/root/reference")
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import nerf_oracle as orc  # noqa: E402


def load_reference():
    for name in ("imageio", "cv2"):
        if name not in sys.modules:
            sys.modules[name] = types.ModuleType(name)
    if REF not in sys.path:
        sys.path.insert(0, REF)
    import run_nerf  # noqa
    import run_nerf_helpers  # noqa
    return run_nerf, run_nerf_helpers


def reference_networks(helpers, P):
    net = helpers.NeRF(D=8, W=256, input_ch=63, output_ch=5, skips=[4], input_ch_views=27, use_viewdirs=True)
    net.load_state_dict({k: v.clone() for k, v in P.items()})
    return net


_GOLD = None        # replay: {what: the reference's value} recorded by --record; the reference is not imported
_RECORD = None      # live run under --record: collects the reference's values by `what`


DIGEST_ABOVE = 16384      # --record keeps a larger value as the SHA-256 of its shape, dtype and bytes (the fixture stays small)


def _digest(t):
    a = np.ascontiguousarray(t.detach().numpy())
    return np.frombuffer(hashlib.sha256(f"{a.shape} {a.dtype}".encode() + a.tobytes()).digest(), np.uint8)


def recorded(what):
    return what in _GOLD or "sha256:" + what in _GOLD


def reference(thunk):
    """the reference's value, computed (live) -- None when replaying recorded values"""
    return None if _GOLD is not None else thunk()


def ref_keys(ref, prefix):
    """the keys of a dict the reference returned (live) / recorded under `prefix <key>` (replay)"""
    if _GOLD is None:
        return list(ref)
    names = [w[len("sha256:"):] if w.startswith("sha256:") else w for w in _GOLD]
    return [w[len(prefix) + 1:] for w in names if w.startswith(prefix + " ") and " " not in w[len(prefix) + 1:]]


def same(a, b, what):
    if _GOLD is not None:
        assert recorded(what), f"{what}: not in the recorded reference values"
        if "sha256:" + what in _GOLD:
            eq = np.array_equal(_digest(a), _GOLD["sha256:" + what])
            print(f"  {what:28s} bit-identical={eq}  (digest)")
            assert eq, f"{what}: oracle differs from reference (SHA-256 of the recorded value)"
            return
        b = torch.from_numpy(np.array(_GOLD[what]))
    elif _RECORD is not None:
        assert not any(k in _RECORD for k in (what, "sha256:" + what)), what
        v = b.detach().numpy().copy()
        if v.nbytes > DIGEST_ABOVE:
            _RECORD["sha256:" + what] = _digest(b)
        else:
            _RECORD[what] = v
    a = a.detach()
    b = b.detach()
    eq = torch.equal(a, b) or bool(((a == b) | (torch.isnan(a) & torch.isnan(b))).all())
    md = float((a - b).abs().nan_to_num(0).max()) if a.numel() else 0.0
    print(f"  {what:28s} bit-identical={eq}  max|d|={md:.3e}")
    assert eq, f"{what}: oracle differs from reference (max|d|={md})"


def main(n_rays=96, golden=None, record=None):
    """golden: replay the reference's values from this mapping ({what: array}, --record's file); record: fill this dict"""
    global _GOLD, _RECORD
    _GOLD, _RECORD = golden, record
    try:
        _pin(n_rays)
    finally:
        _GOLD = _RECORD = None


def _pin(n_rays):
    live = _GOLD is None
    torch.manual_seed(0)
    run_nerf, helpers = load_reference() if live else (None, None)
    Pc = orc.make_params(11, gain=1.0, sigma_bias=0.5)
    Pf = orc.make_params(12, gain=1.0, sigma_bias=0.5)
    net_c, net_f = (reference_networks(helpers, Pc), reference_networks(helpers, Pf)) if live else (None, None)
    if live:
        embed_fn, ch = helpers.get_embedder(10, 0)
        embeddirs_fn, chv = helpers.get_embedder(4, 0)
        assert (ch, chv) == (63, 27)
        qfn = lambda inputs, viewdirs, network_fn: run_nerf.run_network(
            inputs, viewdirs, network_fn, embed_fn=embed_fn, embeddirs_fn=embeddirs_fn, netchunk=1024 * 64)
    rays = orc.synthetic_rays(n_rays, seed=3)
    print("posenc / field_mlp")
    torch.manual_seed(1)        # (the reference's network constructors above draw from the global generator)
    x = torch.randn(257, 3) * 3.0
    same(orc.posenc(x, 10), reference(lambda: embed_fn(x)), "posenc L=10")
    same(orc.posenc(x, 4), reference(lambda: embeddirs_fn(x)), "posenc L=4")
    feats = torch.cat([orc.posenc(x, 10), orc.posenc(x / x.norm(dim=-1, keepdim=True), 4)], -1)    # (== the reference's: above)
    same(orc.field_mlp(Pc, feats), reference(lambda: net_c(feats)), "field_mlp")

    print("composite / inverse_cdf")
    raw = torch.randn(n_rays, 64, 4) * 3.0
    z = torch.sort(torch.rand(n_rays, 64) * 4.0 + 2.0, -1)[0]
    for wb in (False, True):
        got = orc.composite(raw, z, rays[:, 3:6], None, wb)
        ref = reference(lambda: run_nerf.raw2outputs(raw, z, rays[:, 3:6], 0.0, wb)) or (None,) * 5
        for g, r, nm in zip(got, ref, ("rgb", "disp", "acc", "weights", "depth")):
            same(g, r, f"composite wb={wb} {nm}")
    w = got[3]
    zmid = 0.5 * (z[..., 1:] + z[..., :-1])
    same(orc.inverse_cdf(zmid, w[..., 1:-1], 128, None), reference(lambda: helpers.sample_pdf(zmid, w[..., 1:-1], 128, det=True)),
         "inverse_cdf det")
    # random u: reference draws torch.rand inside; replay the same stream
    torch.manual_seed(5)
    ref_s = reference(lambda: helpers.sample_pdf(zmid, w[..., 1:-1], 128, det=False))
    torch.manual_seed(5)
    u = torch.rand(n_rays, 128)
    same(orc.inverse_cdf(zmid, w[..., 1:-1], 128, u), ref_s, "inverse_cdf random u")

    print("trace_rays (render_rays), deterministic test-time configuration")
    kw = dict(network_fn=net_c, network_query_fn=qfn if live else None, N_samples=64, retraw=True, lindisp=False, perturb=0.0,
              N_importance=128, network_fine=net_f, white_bkgd=True, raw_noise_std=0.0)
    ref = reference(lambda: run_nerf.render_rays(rays, **kw))
    got = orc.trace_rays(rays, Pc, Pf, 64, 128, perturb=0.0, white_bkgd=True, retraw=True)
    for k in ref_keys(ref, "trace det"):
        same(got[k], ref and ref[k], f"trace det {k}")

    print("trace_rays, training configuration (perturb=1, raw_noise_std=1, lindisp) with replayed RNG")
    kw.update(perturb=1.0, raw_noise_std=1.0, lindisp=True, white_bkgd=False)
    torch.manual_seed(9)
    ref = reference(lambda: run_nerf.render_rays(rays, **kw))
    torch.manual_seed(9)      # replay the order of draws of run_nerf.py:371,:285, helpers:208, :285
    t_rand = torch.rand(n_rays, 64)
    noise_c = torch.randn(n_rays, 64)
    u = torch.rand(n_rays, 128)
    noise_f = torch.randn(n_rays, 192)
    got = orc.trace_rays(rays, Pc, Pf, 64, 128, perturb=1.0, lindisp=True, white_bkgd=False, raw_noise_std=1.0,
                         retraw=True, t_rand=t_rand, u=u, noise_c=noise_c, noise_f=noise_f)
    for k in ref_keys(ref, "trace train"):
        same(got[k], ref and ref[k], f"trace train {k}")

    print("gradients (loss of run_nerf.py:765-772)")
    target = torch.rand(n_rays, 3)
    kw.update(perturb=0.0, raw_noise_std=0.0, lindisp=False, white_bkgd=True)
    loss = None
    if live:
        ref = run_nerf.render_rays(rays, **kw)
        loss = helpers.img2mse(ref["rgb_map"], target) + helpers.img2mse(ref["rgb0"], target)
        loss.backward()
    Pc_g = {k: v.clone().requires_grad_(True) for k, v in Pc.items()}
    Pf_g = {k: v.clone().requires_grad_(True) for k, v in Pf.items()}
    got = orc.trace_rays(rays, Pc_g, Pf_g, 64, 128, perturb=0.0, white_bkgd=True)
    l2 = orc.mse(got["rgb_map"], target) + orc.mse(got["rgb0"], target)
    l2.backward()
    same(l2, loss, "loss")
    for tag, P_g, net in (("coarse", Pc_g, net_c), ("fine", Pf_g, net_f)):
        ref_grads = {k: p.grad for k, p in net.state_dict(keep_vars=True).items()} if live else {}
        for k in (ref_grads if live else P_g):
            same(P_g[k].grad, ref_grads.get(k), f"grad {tag} {k}")

    print("assemble_rays / pinhole_rays / ndc_warp via reference render() boundary")
    H, W, focal = 20, 24, 30.0
    K = np.array([[focal, 0, 0.5 * W], [0, focal, 0.5 * H], [0, 0, 1]])
    c2w = torch.tensor([[1.0, 0, 0, 0.1], [0, 0.8, -0.6, 0.2], [0, 0.6, 0.8, 4.0]])
    ro, rd = reference(lambda: helpers.get_rays(H, W, K, c2w)) or (None, None)
    go, gd = orc.pinhole_rays(H, W, K, c2w)
    same(go, ro, "pinhole rays_o")
    same(gd, rd, "pinhole rays_d")
    c2w_ff = torch.tensor([[1.0, 0, 0, 0.1], [0, 1.0, 0, 0.2], [0, 0, 1.0, 0.3]])
    ro2, rd2 = orc.pinhole_rays(H, W, K, c2w_ff)            # (== the reference's get_rays: above)
    a, b = reference(lambda: helpers.ndc_rays(H, W, focal, 1.0, ro2, rd2)) or (None, None)
    c, d = orc.ndc_warp(H, W, focal, 1.0, ro2, rd2)
    same(c, a, "ndc rays_o")
    same(d, b, "ndc rays_d")
    kw_r = dict(kw)
    ref_list = reference(lambda: run_nerf.render(H, W, K, chunk=128, rays=torch.stack([go.reshape(-1, 3)[:64], gd.reshape(-1, 3)[:64]], 0),
                                                 ndc=False, near=2.0, far=6.0, use_viewdirs=True, **kw_r)) or (None, None, None, {"raw": None})
    flat = orc.assemble_rays(go.reshape(-1, 3)[:64], gd.reshape(-1, 3)[:64], 2.0, 6.0)
    got = orc.trace_in_chunks(flat, 128, P_coarse=Pc, P_fine=Pf, n_coarse=64, n_fine=128, perturb=0.0,
                              white_bkgd=True, retraw=True)
    same(got["rgb_map"], ref_list[0], "render() rgb_map")
    same(got["disp_map"], ref_list[1], "render() disp_map")
    same(got["acc_map"], ref_list[2], "render() acc_map")
    same(got["raw"], ref_list[3]["raw"], "render() raw")
    print("render(ndc=True) on forward-facing rays (configs/fern.txt: near=0, far=1, raw_noise_std=1, no white_bkgd)")
    cfg = orc.FERN
    Kf = orc.intrinsics(cfg)
    batch = orc.fern_batch(48, seed=2)
    kw_f = dict(kw)
    kw_f.update(perturb=1.0, raw_noise_std=1.0, white_bkgd=False)
    torch.manual_seed(21)
    ref_list = reference(lambda: run_nerf.render(cfg["H"], cfg["W"], Kf, chunk=1024, rays=batch, ndc=True, near=0.0, far=1.0,
                                                 use_viewdirs=True, **kw_f)) or (None, None, None, {"raw": None, "z_std": None})
    torch.manual_seed(21)
    rnd = dict(t_rand=torch.rand(48, 64), noise_c=torch.randn(48, 64), u=torch.rand(48, 128), noise_f=torch.randn(48, 192))
    flat = orc.assemble_render_rays(cfg["H"], cfg["W"], Kf, batch[0], batch[1], True, 0.0, 1.0)
    got = orc.trace_rays(flat, Pc, Pf, 64, 128, perturb=1.0, white_bkgd=False, raw_noise_std=1.0, retraw=True, **rnd)
    same(got["rgb_map"], ref_list[0], "render(ndc) rgb_map")
    same(got["disp_map"], ref_list[1], "render(ndc) disp_map")
    same(got["acc_map"], ref_list[2], "render(ndc) acc_map")
    same(got["raw"], ref_list[3]["raw"], "render(ndc) raw")
    same(got["z_std"], ref_list[3]["z_std"], "render(ndc) z_std")
    print("other architectures (netdepth / netwidth / multires / i_embed = -1 / use_viewdirs = False -> output_linear)")
    ARCHS = {"no_viewdirs": orc.arch_of(use_viewdirs=False), "narrow_shallow": orc.arch_of(D=6, W=128, multires=6, multires_views=2),
             "identity_embedding": orc.arch_of(D=4, W=64, multires=-1, multires_views=-1, output_ch=4),
             "no_viewdirs_small": orc.arch_of(D=7, W=96, multires=3, use_viewdirs=False, output_ch=4)}
    for name, arch in ARCHS.items():
        A = {k: arch[k] for k in ("D", "W", "input_ch", "input_ch_views", "output_ch", "skips", "use_viewdirs")}
        nets, Ps = [], []
        for seed in (31, 32):
            P = orc.make_arch_params(arch, seed)
            if live:
                net = helpers.NeRF(**A)
                assert [(k, tuple(v.shape)) for k, v in net.state_dict().items()] == orc.arch_param_shapes(arch), name
                net.load_state_dict({k: v.clone() for k, v in P.items()})
                nets.append(net)
            Ps.append(P)
        rr = rays if arch["use_viewdirs"] else rays[:, :8]          # render() appends view directions only with use_viewdirs
        ref = None
        if live:
            i_embed = -1 if arch["multires"] < 0 else 0
            e_fn, ch = helpers.get_embedder(arch["multires"], i_embed)
            ed_fn, chv = helpers.get_embedder(arch["multires_views"], i_embed) if arch["use_viewdirs"] else (None, 0)
            assert (ch, chv) == (arch["input_ch"], arch["input_ch_views"]), name
            qfn = lambda inputs, viewdirs, network_fn, e_fn=e_fn, ed_fn=ed_fn: run_nerf.run_network(
                inputs, viewdirs, network_fn, embed_fn=e_fn, embeddirs_fn=ed_fn, netchunk=1024 * 64)
            torch.manual_seed(13)
            ref = run_nerf.render_rays(rr, network_fn=nets[0], network_query_fn=qfn, N_samples=24, retraw=True, lindisp=False, perturb=1.0,
                                       N_importance=40, network_fine=nets[1], white_bkgd=True, raw_noise_std=0.5)
        torch.manual_seed(13)
        rnd = dict(t_rand=torch.rand(n_rays, 24), noise_c=torch.randn(n_rays, 24), u=torch.rand(n_rays, 40), noise_f=torch.randn(n_rays, 64))
        Pg = [{k: v.clone().requires_grad_(True) for k, v in P.items()} for P in Ps]
        got = orc.trace_rays(rr, Pg[0], Pg[1], 24, 40, perturb=1.0, white_bkgd=True, raw_noise_std=0.5, retraw=True, arch=arch, **rnd)
        for k in ref_keys(ref, name):
            same(got[k], ref and ref[k], f"{name} {k}")
        if live:
            loss = helpers.img2mse(ref["rgb_map"], target) + helpers.img2mse(ref["rgb0"], target)
            loss.backward()
        (orc.mse(got["rgb_map"], target) + orc.mse(got["rgb0"], target)).backward()
        for i, P in enumerate(Pg):
            ref_grads = {k: p.grad for k, p in nets[i].state_dict(keep_vars=True).items()} if live else {}
            for k in P:
                what = f"{name} grad{i} {k}"
                if (ref_grads.get(k) is not None or P[k].grad is not None) if live else recorded(what):
                    same(P[k].grad, ref_grads.get(k), what)        # (views_linears is unused without view directions)
    print("ORACLE PINNED: every function bit-identical to the reference on CPU")


if __name__ == "__main__":
    if "--record" in sys.argv:
        out = sys.argv[sys.argv.index("--record") + 1]
        rec = {}
        main(n_rays=48, record=rec)
        np.savez_compressed(out, **rec)
        print(f"recorded {len(rec)} reference values -> {out}")
    else:
        main()
