"""CPU: what render_rays refuses, as one literal table -- the exception type and the whole message of every refusal that needs no GPU
(the option checks, the network and ray-record checks, the injected draws, the grid guards, the baked guards), the winner of a call
that is wrong in two ways, the three readings of a bool march_fit, and the last_stats keys batchify_rays derives from unchecked
keywords.  A refused call launches nothing: hip_backend.lib is patched to fail the test."""
import numpy as np
import pytest
import torch

import nerf_pytorch_amd as npa
from test_baked_cpu import constant_field
from test_march_cpu import HI, LO, NET_KW, RES, _rays

CPU = torch.device("cpu")
NAN = float("nan")
V, N, T = ValueError, NotImplementedError, TypeError

# placeholders of the table, resolved per test (world())
DGRID, PLAIN, FIELD, HOOK = "<DensityGrid>", "<OccupancyGrid>", "<BakedField>", "<hook>"
MARCH = dict(occupancy=DGRID, proposal="march", march_steps=64)
PMARCH = dict(occupancy=PLAIN, proposal="march", march_steps=64)

BELONGS = "render_rays: {} belongs to proposal=\"march\""
MARCH_STEPS = "render_rays: proposal=\"march\" needs march_steps, an int with 1 <= march_steps <= 16384, got {}"
FIT_MUST = "render_rays: march_fit must be an int with 0 <= march_fit <= 8, got {}"
STEP_MUST = "render_rays: march_step_size must be a finite real number > 0 (as an fp32 value), got {}"
EPS_MUST = "render_rays: march_stop_eps must be a float with 0 < eps < 1, got {}"
EARLY_MUST = "render_rays: early_stop_eps must be None or a float with 0 < eps < 1, got {}"
BAKED = "render_rays: baked= renders from the baked field alone and cannot be combined with {}"
INTER_PROPOSAL = ("render_rays: interlevel=True fits the coarse network's weights to the refining pass's; proposal={} has no coarse "
                  "network pass")
INTER_FINE = "render_rays: interlevel=True needs a refining pass to fit the coarse weights to: N_importance must be > 0"
CLIP = "render_rays: clip_to_occupancy=True needs an occupancy grid (occupancy=)"
EARLY_MARCH = "render_rays: early_stop_eps together with proposal=\"march\": there are no coarse weights to stop on"
EARLY_GRID = "render_rays: early_stop_eps needs an occupancy grid (occupancy=): the stop is applied by the grid's compaction"
LINDISP = "render_rays: proposal=\"march\" with lindisp=True is not implemented (the steps are equal in depth)"
FIT_NEEDS_STEP = "render_rays: march_fit doubles the world-space step of a ray: it needs march_step_size"
NO_DENSITIES = "render_rays: {} reads the densities of an occupancy.DensityGrid (occupancy=); {}"

# (id, keywords over N_samples=8, N_importance=8 and two fused networks; "_net" / "_rays" / "_query" / "_grad" choose the rest, type, message)
REFUSED = [
    # ---- distortion / interlevel, in front of everything but baked
    ("distortion-int", dict(distortion=1), V, "render_rays: distortion must be a bool, got 1"),
    ("distortion-none", dict(distortion=None), V, "render_rays: distortion must be a bool, got None"),
    ("interlevel-str", dict(interlevel="yes"), V, "render_rays: interlevel must be a bool, got 'yes'"),
    ("distortion-then-interlevel", dict(distortion=1, interlevel=2), V, "render_rays: distortion must be a bool, got 1"),
    ("interlevel-grid", dict(interlevel=True, occupancy=DGRID, proposal="grid"), V, INTER_PROPOSAL.format("'grid'")),
    ("interlevel-march", dict(interlevel=True, **MARCH), V, INTER_PROPOSAL.format("'march'")),
    ("interlevel-then-unknown-proposal", dict(interlevel=True, proposal="bogus"), V, INTER_PROPOSAL.format("'bogus'")),
    ("interlevel-np-bool-no-fine", dict(interlevel=np.bool_(True), N_importance=0), V, INTER_FINE),
    ("interlevel-proposal-then-no-fine", dict(interlevel=True, proposal="grid", N_importance=0), V, INTER_PROPOSAL.format("'grid'")),
    ("interlevel-no-fine-then-clip", dict(interlevel=True, N_importance=0, clip_to_occupancy=True), V, INTER_FINE),
    ("distortion-np-bool-then-clip", dict(distortion=np.bool_(True), clip_to_occupancy=True), V, CLIP),
    # ---- the grid options
    ("clip-without-grid", dict(clip_to_occupancy=True), V, CLIP),
    ("clip-then-march-steps", dict(clip_to_occupancy=True, march_steps=4), V, CLIP),
    ("march-steps-without-march", dict(march_steps=4), V, BELONGS.format("march_steps")),
    ("march-steps-with-grid-proposal", dict(march_steps=4, occupancy=DGRID, proposal="grid"), V, BELONGS.format("march_steps")),
    ("march-steps-then-stop-eps", dict(march_steps=4, march_stop_eps=0.1), V, BELONGS.format("march_steps")),
    ("stop-eps-without-march", dict(march_stop_eps=0.1), V, BELONGS.format("march_stop_eps")),
    ("stop-eps-then-step-size", dict(march_stop_eps=0.1, march_step_size=0.1), V, BELONGS.format("march_stop_eps")),
    ("step-size-without-march", dict(march_step_size=0.1), V, BELONGS.format("march_step_size")),
    ("step-size-then-fit", dict(march_step_size=0.1, march_fit=1), V, BELONGS.format("march_step_size")),
    ("fit-without-march", dict(march_fit=1), V, BELONGS.format("march_fit")),
    ("fit-np-int-without-march", dict(march_fit=np.int64(2)), V, BELONGS.format("march_fit")),
    ("fit-float-without-march", dict(march_fit=1.5), V, BELONGS.format("march_fit")),
    # (the check reads a bool as SET, whatever its value)
    ("fit-true-without-march", dict(march_fit=True), V, BELONGS.format("march_fit")),
    ("fit-false-without-march", dict(march_fit=False), V, BELONGS.format("march_fit")),
    ("fit-np-false-without-march", dict(march_fit=np.bool_(False)), V, BELONGS.format("march_fit")),
    # (None and an integer zero of either spelling are off: the call gets as far as its next mistake)
    ("fit-none-is-off", dict(march_fit=None, early_stop_eps=2.0), V, EARLY_MUST.format("2.0")),
    ("fit-np-zero-is-off", dict(march_fit=np.int64(0), early_stop_eps=2.0), V, EARLY_MUST.format("2.0")),
    ("fit-then-unknown-proposal", dict(march_fit=1, proposal="bogus"), V, BELONGS.format("march_fit")),
    ("march-without-grid", dict(proposal="march", march_steps=64), V,
     "render_rays: proposal=\"march\" walks an occupancy grid (occupancy=): none was given"),
    ("march-without-grid-or-steps", dict(proposal="march"), V,
     "render_rays: proposal=\"march\" walks an occupancy grid (occupancy=): none was given"),
    ("march-steps-none", dict(occupancy=DGRID, proposal="march"), V, MARCH_STEPS.format("None")),
    ("march-steps-bool", dict(MARCH, march_steps=True), V, MARCH_STEPS.format("True")),
    ("march-steps-zero", dict(MARCH, march_steps=0), V, MARCH_STEPS.format("0")),
    ("march-steps-large", dict(MARCH, march_steps=16385), V, MARCH_STEPS.format("16385")),
    ("march-steps-float", dict(MARCH, march_steps=64.0), V, MARCH_STEPS.format("64.0")),
    ("march-steps-np-int-accepted", dict(MARCH, march_steps=np.int64(64), lindisp=True), N, LINDISP),
    ("march-steps-then-early-stop", dict(MARCH, march_steps=0, early_stop_eps=0.1), V, MARCH_STEPS.format("0")),
    ("early-stop-with-march", dict(MARCH, early_stop_eps=0.1), V, EARLY_MARCH),
    ("early-stop-out-of-range-with-march", dict(MARCH, early_stop_eps=2.0), V, EARLY_MARCH),
    ("early-stop-with-march-then-slots", dict(MARCH, early_stop_eps=0.1, N_samples=4096), V, EARLY_MARCH),
    ("march-too-many-slots", dict(MARCH, N_samples=4090, N_importance=7), V,
     "render_rays: proposal=\"march\" fills at most 4096 slots per ray (N_samples + N_importance)"),
    ("march-no-slot", dict(MARCH, N_samples=0, N_importance=-3), V,
     "render_rays: proposal=\"march\" needs at least one slot per ray (N_samples + N_importance)"),
    ("march-lindisp", dict(MARCH, lindisp=True), N, LINDISP),
    ("march-lindisp-then-fit", dict(MARCH, lindisp=True, march_fit=9), N, LINDISP),
    ("fit-without-step", dict(MARCH, march_fit=1), V, FIT_NEEDS_STEP),
    ("fit-np-int-without-step", dict(MARCH, march_fit=np.int64(3)), V, FIT_NEEDS_STEP),
    ("fit-out-of-range-without-step", dict(MARCH, march_fit=9), V, FIT_MUST.format("9")),
    ("fit-true-without-step", dict(MARCH, march_fit=True), V, FIT_MUST.format("True")),
    ("fit-false-without-step", dict(MARCH, march_fit=False), V, FIT_MUST.format("False")),
    ("fit-np-true-with-step", dict(MARCH, march_step_size=0.1, march_fit=np.bool_(True)), V,
     FIT_MUST.format(repr(np.bool_(True)))),       # ("True" or "np.True_": numpy's own repr, which changed with numpy 2)
    ("fit-negative", dict(MARCH, march_step_size=0.1, march_fit=-1), V, FIT_MUST.format("-1")),
    ("fit-str", dict(MARCH, march_step_size=0.1, march_fit="2"), V, FIT_MUST.format("'2'")),
    ("step-size-zero", dict(MARCH, march_step_size=0.0), V, STEP_MUST.format("0.0")),
    ("step-size-bool", dict(PMARCH, march_step_size=True), V, STEP_MUST.format("True")),
    ("step-size-nan", dict(MARCH, march_step_size=NAN), V, STEP_MUST.format("nan")),
    ("step-size-then-fit-value", dict(MARCH, march_step_size=-1.0, march_fit=9), V, STEP_MUST.format("-1.0")),
    ("step-size-then-stop-eps", dict(MARCH, march_step_size=0.0, march_stop_eps=1.0), V, STEP_MUST.format("0.0")),
    ("stop-eps-one", dict(MARCH, march_stop_eps=1.0), V, EPS_MUST.format("1.0")),
    ("stop-eps-bool", dict(MARCH, march_stop_eps=True), V, EPS_MUST.format("True")),
    ("stop-eps-value-then-plain-grid", dict(PMARCH, march_stop_eps=0.0), V, EPS_MUST.format("0.0")),
    ("stop-eps-plain-grid", dict(PMARCH, march_stop_eps=0.01), V, NO_DENSITIES.format("march_stop_eps", "a plain OccupancyGrid has none")),
    ("early-stop-zero", dict(occupancy=DGRID, early_stop_eps=0.0), V, EARLY_MUST.format("0.0")),
    ("early-stop-one", dict(occupancy=DGRID, early_stop_eps=1), V, EARLY_MUST.format("1.0")),
    ("early-stop-nan", dict(occupancy=DGRID, early_stop_eps=NAN), V, EARLY_MUST.format("nan")),
    ("early-stop-range-then-no-grid", dict(early_stop_eps=2.0), V, EARLY_MUST.format("2.0")),
    ("early-stop-without-grid", dict(early_stop_eps=0.1), V, EARLY_GRID),
    ("early-stop-without-grid-or-fine", dict(early_stop_eps=0.1, N_importance=0), V, EARLY_GRID),
    ("early-stop-without-fine", dict(occupancy=PLAIN, early_stop_eps=0.1, N_importance=0), V,
     "render_rays: early_stop_eps stops the refining pass from the coarse pass's weights: N_importance must be > 0"),
    ("early-stop-then-unknown-proposal", dict(early_stop_eps=0.1, proposal="bogus"), V, EARLY_GRID),
    ("proposal-unknown", dict(proposal="bogus"), V, "render_rays: proposal must be None, \"grid\" or \"march\", got 'bogus'"),
    ("proposal-int", dict(occupancy=DGRID, proposal=1), V, "render_rays: proposal must be None, \"grid\" or \"march\", got 1"),
    ("proposal-grid-without-grid", dict(proposal="grid"), V, NO_DENSITIES.format("proposal=\"grid\"", "none was given")),
    ("proposal-grid-plain", dict(occupancy=PLAIN, proposal="grid"), V, NO_DENSITIES.format("proposal=\"grid\"", "a plain OccupancyGrid has none")),
    ("proposal-grid-plain-then-no-fine", dict(occupancy=PLAIN, proposal="grid", N_importance=0), V,
     NO_DENSITIES.format("proposal=\"grid\"", "a plain OccupancyGrid has none")),
    ("proposal-grid-without-fine", dict(occupancy=DGRID, proposal="grid", N_importance=0), V,
     "render_rays: proposal=\"grid\" draws importance samples: N_importance must be > 0"),
    # ---- networks and ray records, behind every option check
    ("networks-mixed", dict(_net="mixed"), N,
     "render_rays: network_fn / network_fine must both be fused-kernel NeRF modules (D=8, W=256, 10 / 4 frequencies, view directions) "
     "or both general ones (nerf_pytorch_amd.NeRF builds either)"),
    ("option-then-networks", dict(_net="mixed", proposal="bogus"), V, "render_rays: proposal must be None, \"grid\" or \"march\", got 'bogus'"),
    ("rays-eight-columns", dict(_rays="8col"), V,
     "render_rays: these networks use view directions; the ray records need 11 columns (render(use_viewdirs=True))"),
    ("networks-then-rays", dict(_net="mixed", _rays="8col"), N,
     "render_rays: network_fn / network_fine must both be fused-kernel NeRF modules (D=8, W=256, 10 / 4 frequencies, view directions) "
     "or both general ones (nerf_pytorch_amd.NeRF builds either)"),
    ("dense-rays-grad", dict(_net="dense", _rays="grad", _grad=True), N,
     "render_rays: gradients to rays / sample points / camera poses are implemented for the fused NeRF architecture only, not for "
     "general (DenseNeRF) networks"),
    ("dense-rays-eight-columns", dict(_net="dense", _rays="8col"), V,
     "render_rays: a network with view directions needs ray records with 11 columns"),
    ("randoms-rows", dict(perturb=1.0, randoms={"t_rand": torch.zeros(3, 8), "u": torch.zeros(8, 8)}), V,
     "render_rays: randoms['t_rand'] has 3 rows for 8 rays"),
    ("randoms-rows-of-the-march", dict(MARCH, perturb=1.0, randoms={"u_march": torch.zeros(5)}), V,
     "render_rays: randoms['u_march'] has 5 rows for 8 rays"),
    ("randoms-rows-then-hook-with-grid", dict(occupancy=DGRID, _query=HOOK, raw_noise_std=1.0,
                                              randoms={"noise_c": torch.zeros(8, 8), "noise_f": torch.zeros(2, 16)}), V,
     "render_rays: randoms['noise_f'] has 2 rows for 8 rays"),
    ("grid-with-hook", dict(occupancy=DGRID, _query=HOOK), N,
     "render_rays: occupancy= together with a user network_query_fn is not implemented (mask inside the hook with "
     "occupancy.occupied(pts) instead)"),
    ("grid-with-dense", dict(occupancy=DGRID, _net="dense"), N,
     "render_rays: occupancy= together with general (DenseNeRF) networks is not implemented; the grid path runs the fused NeRF "
     "architecture only"),
    ("grid-with-hook-then-dense", dict(occupancy=DGRID, _query=HOOK, _net="dense"), N,
     "render_rays: occupancy= together with a user network_query_fn is not implemented (mask inside the hook with "
     "occupancy.occupied(pts) instead)"),
    ("plain-grid-with-gradient", dict(occupancy=PLAIN, _grad=True), N,
     "render_rays: a plain OccupancyGrid together with a needed gradient (grad mode on and parameters or rays that require grad) is "
     "not implemented: a static grid would hide what the network has not learnt yet.  Render under torch.no_grad(), or train through "
     "an occupancy.DensityGrid (the grid that follows the network: maybe_update every step)"),
    ("plain-march-with-gradient", dict(PMARCH, march_step_size=0.1, march_fit=2, _grad=True), N,
     "render_rays: a plain OccupancyGrid together with a needed gradient (grad mode on and parameters or rays that require grad) is "
     "not implemented: a static grid would hide what the network has not learnt yet.  Render under torch.no_grad(), or train through "
     "an occupancy.DensityGrid (the grid that follows the network: maybe_update every step)"),
    # ---- baked: in front of every other check, whatever else is wrong with the call
    ("baked-not-a-field", dict(baked=DGRID), V, "render_rays: baked must be None or a baked.BakedField, got DensityGrid"),
    ("baked-not-a-field-then-options", dict(baked=7, retraw=True), V, "render_rays: baked must be None or a baked.BakedField, got int"),
    ("baked-retraw", dict(baked=FIELD, retraw=True), V, BAKED.format("retraw")),
    ("baked-several", dict(baked=FIELD, interlevel=True, occupancy=DGRID, retraw=1, march_fit=2, raw_noise_std=0.5), V,
     BAKED.format("retraw, raw_noise_std, occupancy, march_fit, interlevel")),
    ("baked-all", dict(baked=FIELD, retraw=True, raw_noise_std=1.0, randoms={}, occupancy=PLAIN, clip_to_occupancy=True, proposal="march",
                       early_stop_eps=0.1, march_steps=4, march_stop_eps=0.1, march_step_size=0.1, march_fit=1, distortion=True,
                       interlevel=True), V,
     BAKED.format("retraw, raw_noise_std, randoms, occupancy, clip_to_occupancy, proposal, early_stop_eps, march_steps, march_stop_eps, "
                  "march_step_size, march_fit, distortion, interlevel")),
    ("baked-then-invalid-distortion", dict(baked=FIELD, distortion=1), V, BAKED.format("distortion")),
    ("baked-then-invalid-options", dict(baked=FIELD, clip_to_occupancy=True, march_steps=0, interlevel=None), V,
     BAKED.format("clip_to_occupancy, march_steps, interlevel")),
    # (the baked guard reads False as off and True as set; a numpy bool is neither an int nor None: set, whatever its value)
    ("baked-fit-true", dict(baked=FIELD, march_fit=True), V, BAKED.format("march_fit")),
    ("baked-fit-false-is-off", dict(baked=FIELD, march_fit=False, retraw=True), V, BAKED.format("retraw")),
    ("baked-fit-np-false", dict(baked=FIELD, march_fit=np.bool_(False), retraw=True), V, BAKED.format("retraw, march_fit")),
    ("baked-fit-np-zero-is-off", dict(baked=FIELD, march_fit=np.int64(0), distortion=np.bool_(False)), V, BAKED.format("distortion")),
    ("baked-fit-none-is-off", dict(baked=FIELD, march_fit=None, proposal="grid"), V, BAKED.format("proposal")),
    ("baked-fit-float", dict(baked=FIELD, march_fit=0.0), V, BAKED.format("march_fit")),
    ("baked-with-hook", dict(baked=FIELD, _query=HOOK), V,
     "render_rays: baked= together with a user network_query_fn: there is no network to query"),
    ("baked-options-then-hook", dict(baked=FIELD, _query=HOOK, distortion=True), V, BAKED.format("distortion")),
    ("baked-rays-eight-columns", dict(baked=FIELD, _rays="8col"), V,
     "render_rays: baked= needs ray records of 11 columns (o, d, near, far, viewdir: render(use_viewdirs=True))"),
    ("baked-hook-then-rays", dict(baked=FIELD, _query=HOOK, _rays="8col"), V,
     "render_rays: baked= together with a user network_query_fn: there is no network to query"),
    ("baked-rays-grad", dict(baked=FIELD, _rays="grad", _grad=True), V,
     "render_rays: baked= has no backward: rays that require grad are refused (render under torch.no_grad() or detach them)"),
]


@pytest.fixture(scope="module")
def world():
    """the objects the table's placeholders stand for, built once (no call that is refused changes them)"""
    dense_kw = dict(D=4, W=64, input_ch=3, output_ch=4, skips=[2], input_ch_views=3, use_viewdirs=True)
    w = {DGRID: npa.DensityGrid(LO, HI, RES, device=CPU), PLAIN: npa.OccupancyGrid(LO, HI, RES, device=CPU),
         FIELD: constant_field(1.0, (0.0, 0.0, 0.0)), HOOK: lambda pts, viewdirs, net: None,
         "fused": (npa.NeRF(**NET_KW), npa.NeRF(**NET_KW)), "dense": (npa.NeRF(**dense_kw), npa.NeRF(**dense_kw))}
    w["mixed"] = (w["fused"][0], w["dense"][1])
    assert isinstance(w["dense"][0], npa.dense.DenseNeRF) and not isinstance(w["fused"][0], npa.dense.DenseNeRF)
    return w


def call_of(world, kw):
    """(positional arguments, keywords, grad mode) of the table's call"""
    kw = {k: world[v] if isinstance(v, str) and v in (DGRID, PLAIN, FIELD, HOOK) else v for k, v in kw.items()}
    net, fine = world[kw.pop("_net", "fused")]
    rays = {"11col": _rays(8), "8col": _rays(8)[:, :8], "grad": _rays(8).requires_grad_(True)}[kw.pop("_rays", "11col")]
    query, grad = kw.pop("_query", None), kw.pop("_grad", False)
    return (rays, net, query), {"N_samples": 8, "N_importance": 8, "network_fine": fine, **kw}, grad


@pytest.mark.parametrize("kw,exc,message", [pytest.param(*c[1:], id=c[0]) for c in REFUSED])
def test_a_refused_call_raises_exactly_this(world, monkeypatch, kw, exc, message):
    monkeypatch.setattr(npa.hip_backend, "lib", lambda: pytest.fail("a refused call reached the library"))
    args, kwargs, grad = call_of(world, kw)
    for mode in ((True,) if grad else (False, True)):       # (what does not ask for grad mode is refused alike in both)
        with torch.set_grad_enabled(mode), pytest.raises((V, N, T)) as caught:
            npa.render_rays(*args, **kwargs)
        assert type(caught.value) is exc and str(caught.value) == message


def test_the_table_names_every_case_once():
    ids = [c[0] for c in REFUSED]
    assert len(set(ids)) == len(ids)


def test_the_layers_that_forward_keywords_refuse_alike(world, monkeypatch):
    monkeypatch.setattr(npa.hip_backend, "lib", lambda: pytest.fail("a refused call reached the library"))
    net, fine = world["fused"]
    rays = _rays(8)
    kw = dict(network_fn=net, network_query_fn=None, N_samples=8, N_importance=8, network_fine=fine)
    with pytest.raises(V) as caught:
        npa.batchify_rays(rays, 4, march_fit=True, **kw)
    assert str(caught.value) == BELONGS.format("march_fit")
    with pytest.raises(V) as caught:        # batchify_rays' own check of the injected draws, in front of the first chunk
        npa.batchify_rays(rays, 4, randoms={"u": torch.zeros(3, 8)}, proposal="bogus", **kw)
    assert str(caught.value) == "randoms['u'] has 3 rows for 8 rays"
    K = np.array([[10.0, 0, 2.0], [0, 10.0, 2.0], [0, 0, 1]])
    with pytest.raises(V) as caught:
        npa.render(4, 2, K, chunk=8, rays=(rays[:, 0:3], rays[:, 3:6]), ndc=False, near=2.0, far=6.0, use_viewdirs=True,
                   baked=world[FIELD], march_fit=np.bool_(False), **kw)
    assert str(caught.value) == BAKED.format("march_fit")


# what batchify_rays starts a grid's summed last_stats from: it sees the keywords as they were given and checks none of them (a call
# of zero rays reaches no check at all), and reads a bool march_fit -- of either spelling and value -- as OFF
STATS = [
    (dict(), ()),
    (dict(clip_to_occupancy=True), ("rays_hit", "rays")),
    (dict(early_stop_eps=0.1), ("rays_stopped",)),
    (dict(clip_to_occupancy=1, early_stop_eps=7), ("rays_hit", "rays", "rays_stopped")),
    (dict(proposal="grid", march_stop_eps=0.1, march_fit=2), ()),
    (dict(proposal="march"), ("rays_truncated",)),
    (dict(proposal="march", march_stop_eps=0.1), ("rays_truncated", "rays_stopped")),
    (dict(proposal="march", march_fit=3), ("rays_truncated", "rays_refit")),
    (dict(proposal="march", march_fit=np.int64(2), march_stop_eps=0.5, clip_to_occupancy=True),
     ("rays_hit", "rays", "rays_truncated", "rays_stopped", "rays_refit")),
    (dict(proposal="march", march_fit=0), ("rays_truncated",)),
    (dict(proposal="march", march_fit=None), ("rays_truncated",)),
    (dict(proposal="march", march_fit=True), ("rays_truncated",)),
    (dict(proposal="march", march_fit=np.bool_(True)), ("rays_truncated",)),
    (dict(proposal="march", march_fit=False), ("rays_truncated",)),
    (dict(proposal="march", march_fit=-1), ("rays_truncated",)),
    (dict(proposal="march", march_fit=1.5), ("rays_truncated",)),
    (dict(proposal="march", march_fit="2"), ("rays_truncated",)),
    (dict(proposal=b"march", march_fit=2), ()),
]


@pytest.mark.parametrize("kw,keys", STATS, ids=[str(i) for i in range(len(STATS))])
def test_batchify_rays_derives_the_stats_keys_from_unchecked_keywords(world, monkeypatch, kw, keys):
    monkeypatch.setattr(npa.hip_backend, "lib", lambda: pytest.fail("an empty call reached the library"))
    grid = npa.OccupancyGrid(LO, HI, RES, device=CPU)
    out = npa.batchify_rays(_rays(0), 4, network_fn=world["fused"][0], network_query_fn=None, N_samples=8, occupancy=grid, **kw)
    assert out == {} and list(grid.last_stats) == ["evaluated", "total", *keys] and set(grid.last_stats.values()) == {0}


EMPTY = [   # (keywords, keys of the dict in order, columns of raw, last_stats keys behind "evaluated" and "total" -- None: no grid)
    (dict(), ["rgb_map", "disp_map", "acc_map", "raw", "rgb0", "disp0", "acc0", "z_std"], 16, None),
    (dict(N_importance=0, distortion=True), ["rgb_map", "disp_map", "acc_map", "raw", "distortion"], 8, None),
    (dict(distortion=True, interlevel=True),
     ["rgb_map", "disp_map", "acc_map", "raw", "rgb0", "disp0", "acc0", "z_std", "distortion", "interlevel"], 16, None),
    (dict(occupancy=DGRID, clip_to_occupancy=True, early_stop_eps=0.1, interlevel=True),
     ["rgb_map", "disp_map", "acc_map", "raw", "rgb0", "disp0", "acc0", "z_std", "interlevel"], 16, ("rays_hit", "rays", "rays_stopped")),
    (dict(occupancy=DGRID, proposal="grid", distortion=True), ["rgb_map", "disp_map", "acc_map", "raw", "z_std", "distortion"], 16, ()),
    (dict(MARCH, distortion=True), ["rgb_map", "disp_map", "acc_map", "raw", "distortion"], 16, ("rays_truncated",)),
    (dict(MARCH, N_importance=0, march_stop_eps=0.1, march_step_size=0.1, march_fit=np.int64(1)),
     ["rgb_map", "disp_map", "acc_map", "raw"], 8, ("rays_truncated", "rays_stopped", "rays_refit")),
]


@pytest.mark.parametrize("retraw", [False, True])
@pytest.mark.parametrize("kw,names,columns,stats", EMPTY, ids=[str(i) for i in range(len(EMPTY))])
def test_the_empty_batch_of_fused_networks(world, monkeypatch, kw, names, columns, stats, retraw):
    """no rays: the keys, their order, the trailing shapes and the grid's zeroed stats, without a launch (the GPU suite holds the same
    table against the calls with rays: tests/test_render_options_gpu.py)"""
    monkeypatch.setattr(npa.hip_backend, "lib", lambda: pytest.fail("an empty call reached the library"))
    args, kwargs, _ = call_of(world, kw)
    grid = kwargs.get("occupancy")
    if grid is not None:
        monkeypatch.setattr(grid, "_desc", lambda: None)        # (the empty batch validates the grid's device; this one lives on the CPU)
        grid.last_stats = None
    out = npa.render_rays(args[0][:0], *args[1:], retraw=retraw, **kwargs)
    assert list(out) == [k for k in names if retraw or k != "raw"]
    tails = {"rgb_map": (3,), "rgb0": (3,), "raw": (columns, 4)}
    for k, v in out.items():
        assert v.shape == (0,) + tails.get(k, ()) and v.dtype == torch.float32, k
    if grid is not None:
        assert list(grid.last_stats) == ["evaluated", "total", *stats] and set(grid.last_stats.values()) == {0}
