"""GPU test (-m gpu) of the SEQUENCE OF LAUNCHES of render_rays' two occupancy-grid paths: every call into the library that the grid
paths make -- which function, on tensors of which shapes, with which flags -- against tests/golden/grid_call_trace.json.  The value tests
(test_gpu_occupancy*.py, test_gpu_ray_clip.py, test_gpu_grid_proposal.py, test_gpu_early_stop.py, test_gpu_march.py) pin what these paths
compute; this one pins what they launch, which is what "as fast as before" means on paths bench.py does not time.

The fixture was written by this file on the commit BEFORE the two paths were folded into one pass chain (render._grid_chain /
_grid_pass), so the chain is not its own yardstick.  It holds the count M of occupied points of every pass, which for a refining pass
depends on the coarse network's fp16x3 weights through sample_fine: after a toolchain change that moves a sample across a cell boundary
the fixture has to be recorded again, on a commit whose sequence is known to be right:

    NERF_RECORD_CALL_TRACE=tests/golden/grid_call_trace.json python -m pytest -m gpu tests/test_gpu_grid_call_trace.py

Only the public API and spies on hip_backend attributes are used.  160 rays in ray sub-chunks of 64 (tiles of 64, 64 and 32 rays: the
last one uneven), N_samples = 16 + N_importance = 24 (a row of 40: no multiple of the 64-lane wavefront), fp16x3, injected randoms, two
networks.  hb.max_saved_rays never returns fewer than 1024 rays whatever SAVE_BUDGET_BYTES says (so 160 rays cannot be split through the
budget, as test_gpu_grid_proposal notes); the 64-ray sub-chunks are therefore forced one level up, by replacing hb.max_saved_rays.

Per call: the function, the shapes of its tensor arguments (positional by index, keywords by name, tuples such as field_bwd's
input_grad= element by element), and the flags save_act, accumulate and whether z_stop is None.  An argument that is a LEASE of
hb.WORKSPACE (occ_compact's slot / records, the act buffers, and occ_expand's raw_c where it is a flat buffer and not a [max(M, 1), 1, 4]
tensor) is recorded as "lease": take() hands out any idle buffer of up to twice the request, so its extent says what the pool held,
not what the path asked for; where the fixture says "lease" for raw_c, any raw_c is accepted.  What the path asked for is the second
list: the sizes of all hb.WORKSPACE.take calls (the library's own included).  Against the fixture no configuration may take more often,
the rows with a backward must take exactly the same, and a no_grad row may differ only by the two temporaries of a compacted pass (the
compacted raw, 4 max(M, 1) floats, and the M zero depths), which the pass may allocate with torch instead of leasing."""
import json
import os

import pytest
import torch

import nerf_oracle as orc
from test_gpu_occupancy import BOX_LO, BOX_HI, ball_grid
from test_gpu_occupancy_train import ball_dgrid, loss_of
from test_gpu_parity import dev, nets, npa  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "grid_call_trace.json")
N, N_C, N_F, SUB = 160, 16, 24, 64
TRACED = ("sample_coarse", "sample_fine", "occ_ray_span", "occ_proposal_weights", "occ_stop_depth", "occ_march", "occ_compact", "field_fwd",
          "occ_expand", "raw2outputs", "raw2outputs_bwd", "occ_gather", "field_bwd", "occ_fold_rays")
LEASES = {"occ_compact": ("3", "4", "slot", "records"), "field_fwd": ("act",), "field_bwd": ("1", "act")}
CONFIGS = {"plain": {}, "clip": dict(clip_to_occupancy=True), "proposal_grid": dict(proposal="grid"), "early_stop": dict(early_stop_eps=0.5),
           "march": dict(proposal="march", march_steps=64), "all_empty": {}}
ROWS = [f"{name}/{mode}" for name in CONFIGS for mode in ("no_grad", "backward")]


def shapes_of(v):
    if isinstance(v, torch.Tensor):
        return list(v.shape)
    if isinstance(v, (tuple, list)):
        return [shapes_of(x) for x in v if isinstance(x, (torch.Tensor, tuple, list))]
    return None


def entry_of(name, args, kwargs):
    named = [(str(i), a) for i, a in enumerate(args)] + list(kwargs.items())
    lease = lambda k, v: k in LEASES.get(name, ()) or (name == "occ_expand" and k in ("1", "raw_c") and v.dim() == 1)
    shapes = {k: ("lease" if lease(k, v) else shapes_of(v)) for k, v in named if shapes_of(v) is not None}
    e = {"fn": name, "shapes": shapes}
    if name == "field_fwd":
        e["save_act"] = bool(kwargs.get("save_act", args[3] if len(args) > 3 else False))
    if name == "field_bwd":
        e["accumulate"] = bool(kwargs["accumulate"] if "accumulate" in kwargs else args[4])
    if name == "occ_fold_rays":
        e["accumulate"] = bool(kwargs.get("accumulate", args[4] if len(args) > 4 else False))
    if name == "occ_compact":
        e["z_stop_is_none"] = (kwargs.get("z_stop") if "z_stop" in kwargs else (args[5] if len(args) > 5 else None)) is None
    return e


def temporaries(calls):
    """per compacted pass of a no_grad row, in the order the pass takes them: [4 max(M, 1)] and, with M > 0, [M]"""
    out, m = [], 0
    for e in calls:
        if e["fn"] == "occ_compact":
            m = 0
        elif e["fn"] == "field_fwd":
            m = e["shapes"]["1"][0]
        elif e["fn"] == "occ_expand":
            out.append([4 * max(m, 1)] + ([m] if m > 0 else []))
    return out


def without_temporaries(takes, calls):
    """the fixture's take list of a no_grad row with every pass's two temporaries taken out where the pass made them: each pass takes
    slot, records, (occ_compact's own scratch,) then the temporaries"""
    takes = list(takes)
    at = 0
    for temps in temporaries(calls):
        while takes[at:at + len(temps)] != temps:
            at += 1
            assert at < len(takes), "the fixture's take list does not hold the temporaries its own call list implies"
        del takes[at:at + len(temps)]
    return takes


@pytest.fixture(scope="module")
def traces(npa, dev, nets):
    hb = npa.hip_backend
    nc, nf, _, _ = nets
    rays = orc.synthetic_rays(N, seed=12).to(dev)
    rnd = {k: v.to(dev) for k, v in orc.synthetic_randoms(N, N_C, N_F, seed=5).items()}
    rnd_march = {"u_march": torch.rand(N, generator=torch.Generator().manual_seed(24)).to(dev), "noise_f": rnd["noise_f"]}
    target = torch.rand(N, 3, generator=torch.Generator().manual_seed(77)).to(dev)
    no_cells = torch.zeros(2, 2, 2, dtype=torch.bool)
    plain = {"ball": ball_grid(npa, dev), "empty": npa.OccupancyGrid.from_mask(no_cells, BOX_LO, BOX_HI, outside="skip", device=dev)}
    dense = {"ball": ball_dgrid(npa, dev), "empty": npa.DensityGrid.from_mask(no_cells, BOX_LO, BOX_HI, outside="skip", device=dev)}
    calls, takes = [], []
    mp = pytest.MonkeyPatch()
    prev = npa.get_precision()
    out = {}
    try:
        npa.set_precision("fp16x3")
        mp.setattr(hb, "max_saved_rays", lambda *a, **k: SUB)
        for name in TRACED:
            mp.setattr(hb, name, lambda *a, _f=getattr(hb, name), _n=name, **k: (calls.append(entry_of(_n, a, k)), _f(*a, **k))[1])
        mp.setattr(hb.WORKSPACE, "take", lambda n_floats, device, _f=hb.WORKSPACE.take: (takes.append(int(n_floats)), _f(n_floats, device))[1])
        for row in ROWS:
            name, mode = row.split("/")
            extra = CONFIGS[name]
            which = "empty" if name == "all_empty" else "ball"
            grid = dense[which] if (mode == "backward" or extra.get("proposal") == "grid") else plain[which]
            kw = dict(N_samples=N_C, N_importance=N_F, network_fine=nf, white_bkgd=True, perturb=1.0, raw_noise_std=1.0,
                      randoms=rnd_march if name == "march" else rnd, occupancy=grid, **extra)
            hb.WORKSPACE.clear()
            del calls[:], takes[:]
            if mode == "no_grad":
                with torch.no_grad():
                    npa.render_rays(rays, nc, None, **kw)
            else:
                r = rays.clone().requires_grad_(True)
                loss_of(npa, npa.render_rays(r, nc, None, **kw), target).backward()
                for m in (nc, nf):
                    for p in m.parameters():
                        p.grad = None
            torch.cuda.synchronize()
            out[row] = {"calls": list(calls), "takes": list(takes)}
    finally:
        mp.undo()
        npa.set_precision(prev)
        hb.WORKSPACE.clear()
    record = os.environ.get("NERF_RECORD_CALL_TRACE")
    if record:
        with open(record, "w") as f:
            f.write("{\n" + ",\n".join(f'{json.dumps(k)}: {json.dumps(v, separators=(",", ":"))}' for k, v in out.items()) + "\n}\n")      # one row per line
    return json.loads(json.dumps(out))      # (tuples -> lists, as the fixture holds them)


@pytest.fixture(scope="module")
def golden():
    with open(FIXTURE) as f:
        return json.load(f)


def test_the_rows_cover_every_traced_function_and_the_uneven_tile(traces):
    """the net is as wide as it claims: every traced function is called somewhere, the rows with a backward run three sub-chunks whose last
    one has 32 rays, and the all-empty grid launches no field kernel"""
    seen = {e["fn"] for t in traces.values() for e in t["calls"]}
    assert seen == set(TRACED)
    per_tile = [e["shapes"]["0"][0] for e in traces["plain/backward"]["calls"] if e["fn"] == "sample_coarse"]
    assert per_tile == [64, 64, 32]
    assert [e["shapes"]["0"][0] for e in traces["plain/no_grad"]["calls"] if e["fn"] == "sample_coarse"] == [N]
    for mode in ("no_grad", "backward"):
        assert not any(e["fn"] in ("field_fwd", "field_bwd") for e in traces[f"all_empty/{mode}"]["calls"])


@pytest.mark.parametrize("row", ROWS)
def test_calls_equal_the_fixture(traces, golden, row):
    got, want = traces[row]["calls"], golden[row]["calls"]
    for i, (g, w) in enumerate(zip(got, want)):
        if w["fn"] == "occ_expand" and w["shapes"]["1"] == "lease":
            g = dict(g, shapes=dict(g["shapes"], **{"1": "lease"}))
        assert g == w, f"{row}: call {i} differs"
    assert len(got) == len(want), f"{row}: {len(got)} calls, the fixture has {len(want)}: {[e['fn'] for e in got]}"


@pytest.mark.parametrize("row", ROWS)
def test_workspace_takes_against_the_fixture(traces, golden, row):
    got, want = traces[row]["takes"], golden[row]["takes"]
    assert len(got) <= len(want), f"{row}: {len(got)} WORKSPACE.take calls, the fixture has {len(want)}"
    if row.endswith("/backward"):
        assert got == want
    else:
        assert got == want or got == without_temporaries(want, golden[row]["calls"]), (row, got, want)
