"""render_rays' options, parsed once: RayOptions (the call's arguments, checked and normalised, and everything derived from them),
RenderCfg (what the passes read), the random draws and the returned dict.  Host code without a launch: nothing here calls into
hip_backend, so a refused call has not even loaded the library.

The two predicates every reader of the options shares -- "is this the march" (_is_march) and "which doubling count does march_fit
spell" (_fit_level) -- are defined here once; batchify_rays, which sees the keywords unchecked, uses them through
unchecked_stats_keys instead of copies."""
import dataclasses
from typing import Any, Optional

import numpy as np
import torch

from .occupancy import DensityGrid, _check_march_eps, _check_march_step


def _is_march(proposal):
    return isinstance(proposal, str) and proposal == "march"


def _fit_level(march_fit, bool_is_int=False):
    """march_fit as it was given, before any check: the doubling count it spells (None: 0), or None for what is no int.  Its three
    readers differ on bools, DELIBERATELY -- each reading is observable and pinned (tests/test_render_options_cpu.py):
      the check (ray_options): a bool of either spelling is no int, hence SET -- refused without the march, "must be an int" with it;
      the stats keys (_stats_keys, also on unchecked keywords): a bool is no int, hence NO "rays_refit" -- the key follows only a count > 0;
      the baked guard (options_set, bool_is_int=True): a Python bool is the int it is -- False is off, True is set --, and a numpy bool
        is neither an int nor None: set, whatever its value."""
    if march_fit is None:
        return 0
    if isinstance(march_fit, (int, np.integer)) and (bool_is_int or not isinstance(march_fit, bool)):
        return int(march_fit)
    return None


def _stats_keys(clip_to_occupancy, early_stop_eps, proposal, march_stop_eps, march_fit):
    """the last_stats keys the grid options add to "evaluated" and "total", from the options checked or not"""
    march = _is_march(proposal)
    return ((("rays_hit", "rays") if clip_to_occupancy else ()) + (("rays_stopped",) if early_stop_eps is not None else ())
            + (("rays_truncated",) if march else ()) + (("rays_stopped",) if march and march_stop_eps is not None else ())
            + (("rays_refit",) if march and (_fit_level(march_fit) or 0) > 0 else ()))


def unchecked_stats_keys(kwargs):
    """RayOptions.stats_keys for batchify_rays, from render_rays' keywords AS GIVEN: batchify_rays validates nothing itself (a call of
    zero rays reaches no check at all) and sums exactly the keys the chunks' calls will write"""
    return _stats_keys(kwargs.get("clip_to_occupancy"), kwargs.get("early_stop_eps"), kwargs.get("proposal"), kwargs.get("march_stop_eps"),
                       kwargs.get("march_fit", 0))


def options_set(*, retraw, raw_noise_std, randoms, occupancy, clip_to_occupancy, proposal, early_stop_eps, march_steps, march_stop_eps,
                march_step_size, march_fit, distortion, interlevel, **_):
    """the names of the options a call set, in the order of render_rays' signature, from the arguments as given (nothing is checked:
    the baked guard, which refuses them all, comes in front of every check)"""
    on = dict(retraw=bool(retraw), raw_noise_std=raw_noise_std > 0., randoms=randoms is not None, occupancy=occupancy is not None,
              clip_to_occupancy=bool(clip_to_occupancy), proposal=proposal is not None, early_stop_eps=early_stop_eps is not None,
              march_steps=march_steps is not None, march_stop_eps=march_stop_eps is not None, march_step_size=march_step_size is not None,
              march_fit=_fit_level(march_fit, bool_is_int=True) != 0, distortion=distortion is not False, interlevel=interlevel is not False)
    return [k for k, v in on.items() if v]


@dataclasses.dataclass(frozen=True, eq=False)
class RayOptions:
    """render_rays' arguments after every check, normalised (ray_options builds it); what follows from them is a property, written once"""
    N_samples: int
    N_importance: int
    retraw: bool
    lindisp: bool
    perturb: Any                        # as given: compared with 0
    white_bkgd: bool
    raw_noise_std: Any                  # as given: compared with 0, the scale the kernels apply is draw_randoms'
    pytest: Any
    randoms: Optional[dict]
    occupancy: Any
    clip_to_occupancy: Any
    proposal: Optional[str]             # None, "grid" or "march"
    early_stop_eps: Optional[float]
    march_steps: Optional[int]
    march_stop_eps: Optional[float]
    march_step_size: Optional[float]
    march_fit: int
    distortion: bool
    interlevel: bool

    @property
    def march(self):
        return _is_march(self.proposal)

    @property
    def one_pass(self):
        """a proposal or the march: ONE network is evaluated, on depths a grid chose, and there is no coarse image"""
        return self.proposal is not None

    @property
    def slots(self):
        """sample points per ray of the last pass: the columns of raw"""
        return self.N_samples + max(self.N_importance, 0)

    @property
    def stats_keys(self):
        return _stats_keys(self.clip_to_occupancy, self.early_stop_eps, self.proposal, self.march_stop_eps, self.march_fit)

    @property
    def random_keys(self):
        """the keys of ``randoms`` the call reads, in the order they are drawn without it"""
        jitter, noise, fine = bool(self.perturb > 0.), bool(self.raw_noise_std > 0.), self.N_importance > 0
        if self.march:
            return ("u_march",) * jitter + ("noise_f",) * noise
        return ("t_rand",) * jitter + ("noise_c",) * (noise and not self.one_pass) + ("u",) * (jitter and fine) + ("noise_f",) * (noise and fine)

    @property
    def output_names(self):
        """the names of the call's output tuple, as every path but the hooked one produces it: the image of the last pass and its raw,
        the coarse image (two network passes only), z_std (a refining pass drew from a pdf), the losses"""
        names = ("rgb_map", "disp_map", "acc_map", "raw")
        if self.N_importance > 0 and not self.march:
            names += (() if self.one_pass else ("rgb0", "disp0", "acc0")) + ("z_std",)
        return names + (("distortion",) if self.distortion else ()) + (("interlevel",) if self.interlevel else ())

    def empty_outputs(self, device):
        """the output tuple of a call without rays: empty tensors of the right trailing shapes, as the reference returns them"""
        tails = {"rgb_map": (3,), "rgb0": (3,), "raw": (self.slots, 4)}
        return tuple(torch.zeros((0,) + tails.get(k, ()), dtype=torch.float32, device=device) for k in self.output_names)


def ray_options(*, N_samples, retraw, lindisp, perturb, N_importance, white_bkgd, raw_noise_std, pytest, randoms, occupancy,
                clip_to_occupancy, proposal, early_stop_eps, march_steps, march_stop_eps, march_step_size, march_fit, distortion,
                interlevel):
    """render_rays' arguments as given -> RayOptions: every check of the options, in the order that decides which mistake of a call is
    reported, in front of everything else (a refused call launches nothing, not even hb.lib())."""
    for name, value in (("distortion", distortion), ("interlevel", interlevel)):
        if not isinstance(value, (bool, np.bool_)):
            raise ValueError(f"render_rays: {name} must be a bool, got {value!r}")
    if interlevel:
        if proposal is not None:
            raise ValueError(f"render_rays: interlevel=True fits the coarse network's weights to the refining pass's; proposal={proposal!r} "
                             "has no coarse network pass")
        if int(N_importance) <= 0:
            raise ValueError("render_rays: interlevel=True needs a refining pass to fit the coarse weights to: N_importance must be > 0")
    if clip_to_occupancy and occupancy is None:
        raise ValueError("render_rays: clip_to_occupancy=True needs an occupancy grid (occupancy=)")
    march = _is_march(proposal)
    fit_off = _fit_level(march_fit) == 0
    for name, is_set in (("march_steps", march_steps is not None), ("march_stop_eps", march_stop_eps is not None),
                         ("march_step_size", march_step_size is not None), ("march_fit", not fit_off)):
        if is_set and not march:
            raise ValueError(f"render_rays: {name} belongs to proposal=\"march\"")
    if march:
        if occupancy is None:
            raise ValueError("render_rays: proposal=\"march\" walks an occupancy grid (occupancy=): none was given")
        if isinstance(march_steps, bool) or not isinstance(march_steps, (int, np.integer)) or not (1 <= int(march_steps) <= 16384):
            raise ValueError(f"render_rays: proposal=\"march\" needs march_steps, an int with 1 <= march_steps <= 16384, got {march_steps!r}")
        if early_stop_eps is not None:
            raise ValueError("render_rays: early_stop_eps together with proposal=\"march\": there are no coarse weights to stop on")
        if int(N_samples) + max(int(N_importance), 0) > 4096:
            raise ValueError("render_rays: proposal=\"march\" fills at most 4096 slots per ray (N_samples + N_importance)")
        if int(N_samples) + max(int(N_importance), 0) < 1:
            raise ValueError("render_rays: proposal=\"march\" needs at least one slot per ray (N_samples + N_importance)")
        if lindisp:
            raise NotImplementedError("render_rays: proposal=\"march\" with lindisp=True is not implemented (the steps are equal in depth)")
        march_steps = int(march_steps)
        if march_step_size is not None or not fit_off:
            if march_step_size is None:
                _check_march_step(1.0, march_fit, "render_rays")
                raise ValueError("render_rays: march_fit doubles the world-space step of a ray: it needs march_step_size")
            march_step_size, march_fit = _check_march_step(march_step_size, march_fit, "render_rays")
        if march_stop_eps is not None:
            march_stop_eps = _check_march_eps(march_stop_eps, "render_rays")
            if not isinstance(occupancy, DensityGrid):
                raise ValueError("render_rays: march_stop_eps reads the densities of an occupancy.DensityGrid (occupancy=); "
                                 "a plain OccupancyGrid has none")
    if early_stop_eps is not None:
        early_stop_eps = float(early_stop_eps)
        if not (0.0 < early_stop_eps < 1.0):        # (also refuses NaN)
            raise ValueError(f"render_rays: early_stop_eps must be None or a float with 0 < eps < 1, got {early_stop_eps!r}")
        if occupancy is None:
            raise ValueError("render_rays: early_stop_eps needs an occupancy grid (occupancy=): the stop is applied by the grid's compaction")
        if int(N_importance) <= 0:
            raise ValueError("render_rays: early_stop_eps stops the refining pass from the coarse pass's weights: N_importance must be > 0")
    if not march and proposal not in (None, "grid"):
        raise ValueError(f"render_rays: proposal must be None, \"grid\" or \"march\", got {proposal!r}")
    if proposal is not None and not march:
        if not isinstance(occupancy, DensityGrid):
            raise ValueError("render_rays: proposal=\"grid\" reads the densities of an occupancy.DensityGrid (occupancy=); "
                             + ("none was given" if occupancy is None else "a plain OccupancyGrid has none"))
        if int(N_importance) <= 0:
            raise ValueError("render_rays: proposal=\"grid\" draws importance samples: N_importance must be > 0")
    return RayOptions(N_samples=int(N_samples), N_importance=int(N_importance), retraw=bool(retraw), lindisp=bool(lindisp), perturb=perturb,
                      white_bkgd=bool(white_bkgd), raw_noise_std=raw_noise_std, pytest=pytest, randoms=randoms, occupancy=occupancy,
                      clip_to_occupancy=clip_to_occupancy, proposal=proposal, early_stop_eps=early_stop_eps, march_steps=march_steps,
                      march_stop_eps=march_stop_eps, march_step_size=march_step_size, march_fit=0 if fit_off else int(march_fit),
                      distortion=bool(distortion), interlevel=bool(interlevel))


@dataclasses.dataclass(frozen=True)
class RenderCfg:
    """what the passes of one render_rays call read: every field exists on every path; a variant is a dataclasses.replace"""
    N_samples: int
    N_importance: int
    lindisp: bool
    white_bkgd: bool
    raw_noise_std: float                # the scale the kernels apply to the drawn noise (draw_randoms)
    precision: str
    need_grad: bool                     # a backward can follow: activations are saved
    distortion: bool
    interlevel: bool
    proposal: Optional[str]             # "grid" or None (the march is march_steps)
    early_stop_eps: Optional[float]
    march_steps: Optional[int]
    march_stop_eps: Optional[float]
    march_step_size: Optional[float]
    march_fit: int

    @staticmethod
    def datapath(precision, need_grad, grid):
        """the reduced inference class runs the fp16x3 products when a gradient is needed (it is an inference form) or a grid is given
        (its last-sample fix-up is per ray, the grid's compacted points are not)"""
        return "fp16x3" if precision == "fp16_fp8c" and (need_grad or grid) else precision

    @classmethod
    def of(cls, opt, *, raw_noise_std, precision, need_grad, grid):
        return cls(N_samples=opt.N_samples, N_importance=opt.N_importance, lindisp=opt.lindisp, white_bkgd=opt.white_bkgd,
                   raw_noise_std=raw_noise_std, precision=cls.datapath(precision, need_grad, grid), need_grad=bool(need_grad),
                   distortion=opt.distortion, interlevel=opt.interlevel, proposal=None if opt.march else opt.proposal,
                   early_stop_eps=opt.early_stop_eps, march_steps=opt.march_steps, march_stop_eps=opt.march_stop_eps,
                   march_step_size=opt.march_step_size, march_fit=opt.march_fit)


def draw_randoms(opt, n, dev):
    """render_rays' random tensors for n rays, the keys opt.random_keys names: injected (opt.randoms, checked for their row count) or
    drawn in the reference's order and shapes.  Returns (rnd, the noise scale the kernels apply)."""
    pytest = opt.pytest
    if opt.randoms is not None:
        rnd = {k: opt.randoms[k].to(device=dev, dtype=torch.float32).contiguous() for k in opt.random_keys}
        for k, v in rnd.items():
            if v.shape[0] != n:
                raise ValueError(f"render_rays: randoms[{k!r}] has {v.shape[0]} rows for {n} rays")
        return rnd, float(opt.raw_noise_std)
    shapes = {"t_rand": (n, opt.N_samples), "noise_c": (n, opt.N_samples), "u": (n, opt.N_importance), "noise_f": (n, opt.slots), "u_march": (n,)}

    def draw(key):      # (the reference's pytest hook draws again with numpy, seeded per tensor, its noise pre-scaled in float64: run_nerf.py:290)
        noise, shape = key.startswith("noise"), shapes[key]
        t = (torch.randn if noise else torch.rand)(shape, device=dev)
        if pytest:
            np.random.seed(0)
            t = torch.Tensor(np.random.rand(*shape) * (opt.raw_noise_std if noise else 1.)).to(dev)
        return t.contiguous()
    # random_keys is in the reference's draw order: t_rand (:371) -> noise coarse (:285) -> u (helpers:208) -> noise fine (:285); the
    # march's: u_march (one offset per ray) -> the noise of its one pass
    rnd = {k: draw(k) for k in opt.random_keys}
    if pytest and opt.N_importance > 0 and not opt.march and "u" not in rnd:
        # det + pytest: the reference builds u with np.linspace in float64 and casts it (helpers:213-215), which is NOT
        # torch.linspace's fp32 sequence (one ulp apart in 30 of 64 / 8 of 128 entries: tests/test_host_cpu.py) -- hand the
        # kernel the reference's numbers as explicit draws
        rnd["u"] = torch.Tensor(np.broadcast_to(np.linspace(0., 1., opt.N_importance), shapes["u"]).copy()).to(dev)
    return rnd, 1.0 if pytest and opt.raw_noise_std > 0. else float(opt.raw_noise_std)


def result_dict(opt, outs, coarse_first):
    """THE returned dict of an output tuple named by opt.output_names ("raw" only with retraw).  coarse_first: the key order of the staged
    paths -- the hooked one's, which the grid paths and the general networks share: the coarse image and z_std in front; else the
    fused node's, which the empty batch has always had: the tuple's own order.  The losses' keys come last either way."""
    named = {k: v for k, v in zip(opt.output_names, outs) if k != "raw" or opt.retraw}
    front = {k: named.pop(k) for k in ("rgb0", "disp0", "acc0", "z_std") if coarse_first and k in named}
    return {**front, **named}
