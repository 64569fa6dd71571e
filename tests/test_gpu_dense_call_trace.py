"""GPU test (-m gpu) of the SEQUENCE OF EVENTS of render_rays' dense autograd node (render._RenderRays), forward and backward, in its three
backward plans: every call into the library -- which function, on tensors of which shapes, with which flags --, every lease taken from and
handed back to hb.WORKSPACE, every GRAD_READY_HOOKS call and LAST_BACKWARD_PLAN, as ONE ordered list per row, against
tests/golden/dense_call_trace.json.  The value tests (test_gpu_parity.py, test_gpu_ray_grad.py, test_gpu_distortion_render.py,
test_interlevel_render_gpu.py) pin what the node computes; this one pins what it launches and when it lets go of its buffers, as
test_gpu_grid_call_trace.py does for the grid paths (whose shapes_of / entry_of it uses).

The fixture was written by this file on the commit BEFORE the two nodes' backwards were given one driver (render._backward), with that
commit's render.py, so the driver is not its own yardstick.  It holds no value that depends on the weights; it has to be recorded again
only when the sequence is meant to change, on a commit whose sequence is known to be right:

    NERF_RECORD_CALL_TRACE=tests/golden/dense_call_trace.json python -m pytest -m gpu tests/test_gpu_dense_call_trace.py

160 rays, N_samples = 16 + N_importance = 24, fp16x3, injected randoms.  Rows = plan x networks x loss:
  plan      "one launch" (hb.max_saved_rays as it is), "resident sub-chunks" (hb.max_saved_rays replaced by 64 rays: tiles of 64, 64 and
            32 rays, the last one uneven), "recompute" (the same with hb.SAVE_TOTAL_BYTES = 0);
  networks  two, one shared by both passes, coarse-only (N_importance = 0);
  loss      the two images; the images, the distortion loss, the interlevel loss and a loss on `raw` (coarse-only: without the interlevel
            loss, which render_rays refuses there); the images with rays that require grad; the images with the coarse network frozen
            (two networks only: with one network nothing would require a gradient and no backward exists).
Per event: a library call as test_gpu_grid_call_trace.entry_of records it (act buffers as "lease"), {"take": floats}, {"give": k} = the
buffer the row's k-th take handed out went back to the pool (-1: a buffer no take of this row handed out), {"grad_ready": "c" | "f"}."""
import json
import os
import sys

import pytest
import torch

import nerf_oracle as orc
from test_gpu_grid_call_trace import entry_of
from test_gpu_parity import dev, nets, npa  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dense_call_trace.json")
N, N_C, N_F, SUB = 160, 16, 24, 64
TRACED = ("sample_coarse", "field_fwd", "raw2outputs", "sample_fine", "distortion", "interlevel", "distortion_bwd", "interlevel_bwd",
          "raw2outputs_bwd", "field_bwd")
PLANS = {"one_launch": "one launch", "resident": "resident sub-chunks", "recompute": "recompute"}
LOSSES = {"two": ("image", "losses", "rays_grad", "frozen_coarse"), "shared": ("image", "losses", "rays_grad"),
          "coarse_only": ("image", "losses", "rays_grad")}
ROWS = [f"{plan}/{net}/{loss}" for plan in PLANS for net in LOSSES for loss in LOSSES[net]]


@pytest.fixture(scope="module")
def traces(npa, dev, nets):
    hb = npa.hip_backend
    render = sys.modules["nerf_pytorch_amd.render"]
    nc, nf, _, _ = nets
    rays = orc.synthetic_rays(N, seed=12).to(dev)
    rnd = {k: v.to(dev) for k, v in orc.synthetic_randoms(N, N_C, N_F, seed=5).items()}
    rnd_coarse = {k: rnd[k] for k in ("t_rand", "noise_c")}
    target = torch.rand(N, 3, generator=torch.Generator().manual_seed(77)).to(dev)
    events, handed = [], {}
    n_takes = [0]

    def take(n_floats, device, _f=hb.WORKSPACE.take):
        t = _f(n_floats, device)
        events.append({"take": int(n_floats)})
        handed[t.data_ptr()] = n_takes[0]
        n_takes[0] += 1
        return t

    def give(t, _f=hb.WORKSPACE.give):
        if t is not None:
            events.append({"give": handed.get(t.data_ptr(), -1)})
        return _f(t)

    hook = lambda model, flat: events.append({"grad_ready": "c" if model is nc else "f"})
    mp = pytest.MonkeyPatch()
    prev = npa.get_precision()
    out = {}
    render.GRAD_READY_HOOKS.append(hook)
    try:
        npa.set_precision("fp16x3")
        for name in TRACED:
            mp.setattr(hb, name, lambda *a, _f=getattr(hb, name), _n=name, **k: (events.append(entry_of(_n, a, k)), _f(*a, **k))[1])
        mp.setattr(hb.WORKSPACE, "take", take)
        mp.setattr(hb.WORKSPACE, "give", give)
        for row in ROWS:
            plan, net, loss = row.split("/")
            with pytest.MonkeyPatch.context() as mrow:
                if plan != "one_launch":
                    mrow.setattr(hb, "max_saved_rays", lambda *a, **k: SUB)
                if plan == "recompute":
                    mrow.setattr(hb, "SAVE_TOTAL_BYTES", 0)
                fine = net != "coarse_only"
                kw = dict(N_samples=N_C, N_importance=N_F if fine else 0, network_fine=nf if net == "two" else None, white_bkgd=True,
                          perturb=1.0, raw_noise_std=1.0, randoms=rnd if fine else rnd_coarse)
                if loss == "losses":
                    kw.update(retraw=True, distortion=True, interlevel=fine)
                r = rays.clone().requires_grad_(True) if loss == "rays_grad" else rays
                for p in nc.parameters():
                    p.requires_grad_(loss != "frozen_coarse")
                hb.WORKSPACE.clear()
                del events[:]
                handed.clear()
                n_takes[0] = 0
                try:
                    res = npa.render_rays(r, nc, None, **kw)
                    events.append({"plan": list(render.LAST_BACKWARD_PLAN)})
                    total = npa.img2mse(res["rgb_map"], target) + (npa.img2mse(res["rgb0"], target) if fine else 0.0)
                    if loss == "losses":
                        total = total + res["distortion"].mean() + (res["raw"] ** 2).mean() + (res["interlevel"].mean() if fine else 0.0)
                    total.backward()
                    torch.cuda.synchronize()
                finally:
                    for m in (nc, nf):
                        for p in m.parameters():
                            p.grad = None
                            p.requires_grad_(True)
                out[row] = list(events)
    finally:
        render.GRAD_READY_HOOKS.remove(hook)
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


def test_the_rows_cover_every_traced_function_every_plan_and_the_uneven_tile(traces):
    """the net is as wide as it claims: every traced function is called somewhere, every row took the plan its name says, the sub-chunked
    rows run three tiles whose last one has 32 rays, the recompute plan runs its forward twice (without saving, then with), every saved
    activation buffer goes back to the pool, and a frozen coarse network is never announced"""
    assert {e["fn"] for t in traces.values() for e in t if "fn" in e} == set(TRACED)
    for row, t in traces.items():
        plan = row.split("/")[0]
        (got_plan,) = [e["plan"] for e in t if "plan" in e]
        assert got_plan[:2] == [PLANS[plan], N] and (got_plan[2] >= N if plan == "one_launch" else got_plan[2] == SUB), row
        tiles = [e["shapes"]["0"][0] for e in t if e.get("fn") == "sample_coarse"]
        assert tiles == {"one_launch": [N], "resident": [64, 64, 32], "recompute": [N, 64, 64, 32]}[plan], row
        saves = {e["save_act"] for e in t[:[i for i, e in enumerate(t) if "plan" in e][0]] if e.get("fn") == "field_fwd"}
        assert saves == ({False} if plan == "recompute" else {True}), row
        assert sum("give" in e for e in t) >= sum(e.get("fn") == "field_fwd" and e["save_act"] for e in t), row
        ready = [e["grad_ready"] for e in t if "grad_ready" in e]
        assert ready == (["f"] if row.endswith("frozen_coarse") else ["c", "f"] if "/two/" in row else ["c"]), row


@pytest.mark.parametrize("row", ROWS)
def test_events_equal_the_fixture(traces, golden, row):
    got, want = traces[row], golden[row]
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, f"{row}: event {i} differs"
    assert len(got) == len(want), f"{row}: {len(got)} events, the fixture has {len(want)}"
