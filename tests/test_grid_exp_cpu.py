"""tools/grid_exp.py, the harness the six grid experiment scripts share: the pieces that can be checked without a GPU.  The expressions
the scripts carried before the harness (ball mask, bisection, the order of calls of the alternating timer) are written out here."""
import importlib.util
import json
import os
import statistics

import pytest
import torch

_PATH = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "grid_exp.py")
_spec = importlib.util.spec_from_file_location("grid_exp", _PATH)
gx = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gx)


@pytest.mark.parametrize("radius", [0.0, 0.5, 1.0, 4.0])
def test_ball_mask(radius):
    R, lo, hi = 16, -2.0, 2.0
    c = lo + (torch.arange(R, dtype=torch.float64) + 0.5) * (hi - lo) / R
    x, y, z = torch.meshgrid(c, c, c, indexing="ij")
    want = (x * x + y * y + z * z) <= radius * radius
    got = gx.ball_mask(R, lo, hi, radius)
    assert got.dtype == torch.bool and got.shape == (R, R, R)
    assert torch.equal(got, want)
    if radius == 0.0:
        assert not got.any()
    if radius == 4.0:
        assert got.all()


@pytest.mark.parametrize("want", [0.5, 0.25, 0.1])
def test_bisect_radius(want):
    def share_of(r):
        return min(1.0, r / 4)
    seen = []

    def recorded(r):
        seen.append(r)
        return share_of(r)
    got = gx.bisect_radius(recorded, want)
    lo, hi, mids = 0.0, 4.0, []
    for _ in range(14):
        mid = 0.5 * (lo + hi)
        mids.append(mid)
        if share_of(mid) < want:
            lo = mid
        else:
            hi = mid
    assert len(seen) == 14 and seen == mids
    assert got == hi
    assert share_of(got) >= want > share_of(got - 4 / 2 ** 14)


class _FakeEvent:
    clock = 0.0

    def __init__(self, enable_timing=False):
        assert enable_timing
        self.t = None

    def record(self):
        _FakeEvent.clock += 1.5
        self.t = _FakeEvent.clock

    def elapsed_time(self, other):
        return other.t - self.t


@pytest.fixture
def fake_cuda(monkeypatch):
    syncs = []
    monkeypatch.setattr(torch.cuda, "Event", _FakeEvent)
    monkeypatch.setattr(torch.cuda, "synchronize", lambda: syncs.append(1))
    return syncs


@pytest.mark.parametrize("warmup", [2, 3])
def test_time_alternating_call_order(fake_cuda, warmup):
    calls = []
    configs = [(n, (lambda n=n: calls.append(n))) for n in "abc"]
    times = gx.time_alternating(configs, k=3, reps=2, warmup=warmup)
    assert "".join(calls) == "".join(n * warmup for n in "abc") + "aaabbbccc" * 2
    assert list(times) == ["a", "b", "c"]
    assert all(len(t) == 2 for t in times.values())
    assert all(ms == 1.5 / 3 for t in times.values() for ms in t)       # one event tick around k = 3 calls
    assert len(fake_cuda) == 1 + 2 * 3      # after the warm-up, then after every timed group


def test_time_launches(fake_cuda):
    calls = []
    got = gx.time_launches(lambda: calls.append(1), reps=4, launches=100, warmup=3)
    assert len(calls) == 3 + 4 * 100
    assert list(got) == ["us_median", "us_min", "us_max"]
    assert got["us_median"] == 1.5 / 100 * 1e3
    assert len(fake_cuda) == 4              # none between the warm-up and the first event


def test_row_stats():
    ms = [3.0, 1.0, 2.0, 5.0]
    assert gx.row_stats(ms) == {"ms_median": statistics.median(ms), "ms_min": 1.0, "ms_max": 5.0}
    row = gx.row_stats(ms, n_rays=4096)
    assert list(row) == ["ms_median", "ms_min", "ms_max", "rays_per_s"]
    assert row["ms_median"] == 2.5 and row["rays_per_s"] == 4096 / 2.5 * 1e3


def test_kernel_ms():
    summary = {"occ_count": {"ms": 1.0}, "occ_stop_depth": {"ms": 0.25}, "field_fwd<fp16x3>": {"ms": 8.0}, "field_bwd": {"ms": 16.0},
               "wgrad1_kernel<fp16>": {"ms": 32.0}, "composite": {"ms": 64.0}}
    assert gx.kernel_ms(summary, "occ_") == 1.25
    assert gx.kernel_ms(summary, "occ_stop_depth") == 0.25
    assert gx.kernel_ms(summary, "field_fwd") == 8.0
    assert gx.kernel_ms(summary, ("field_", "wgrad")) == 56.0
    assert gx.kernel_ms({}, "occ_") == 0


def test_kernel_summary_restores_timer():
    class KernelTimer:
        def summary(self):
            return {"k": {"ms": 1.0}}

    class hb:
        TIMER = "the caller's timer"
    hb.KernelTimer = KernelTimer
    inside = []
    assert gx.kernel_summary(hb, lambda: inside.append(hb.TIMER)) == {"k": {"ms": 1.0}}
    assert isinstance(inside[0], KernelTimer) and hb.TIMER == "the caller's timer"

    def raising():
        assert isinstance(hb.TIMER, KernelTimer)
        raise RuntimeError("the thunk failed")
    with pytest.raises(RuntimeError, match="the thunk failed"):
        gx.kernel_summary(hb, raising)
    assert hb.TIMER == "the caller's timer"


def test_psnr_db():
    a = torch.zeros(4, 3)
    assert gx.psnr_db(a, a) is None
    assert gx.psnr_db(a, a + 0.1) == pytest.approx(20.0, abs=1e-5)


def test_emit(tmp_path, capsys):
    result = {"rows": {"a": {"ms_median": 1.5}}, "note": None}
    out = tmp_path / "not" / "there" / "r.json"
    gx.emit(result, str(out))
    printed = capsys.readouterr().out
    assert out.read_text() == printed == json.dumps(result, indent=1) + "\n"
    gx.emit(result, None)
    assert capsys.readouterr().out == printed


def test_parser_and_import_without_the_library():
    assert "npa" not in gx.__dict__ and "wl" not in gx.__dict__          # load() imports them, from --root
    args = gx.parser("d").parse_args([])
    assert (args.label, args.out, args.reps) == ("this commit", None, 5) and not hasattr(args, "steps") and not hasattr(args, "trace")
    assert os.path.samefile(args.root, os.path.dirname(os.path.dirname(_PATH)))
    args = gx.parser("d", steps="s", trace="t").parse_args(["--steps", "4", "--trace", "--reps", "3"])
    assert (args.steps, args.trace, args.reps) == (4, True, 3)
