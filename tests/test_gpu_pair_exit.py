"""Exit-driven pair-mode loops on the GPU: every probe of tests/pair_exit_probes.py, rendered with the exit-driven
loops (MMHIP_PAIR_EXIT=1, with the back edge as one asm statement and as plain C++), with the per-iteration selects
(MMHIP_PAIR_EXIT=0) and one pixel at a time (MMHIP_PAIR=0), must give the oracle's bytes."""
import numpy as np
import pytest

import mathmap_amd as mm
from oracle.ccgen import CpuFilter
from tests import filters as F
from tests import launch_sizes as LS
from tests.pair_exit_probes import PROBES, SIZES, by_name

pytestmark = pytest.mark.gpu

# (label, environment)
MODES = [
    ("exit", {"MMHIP_PAIR": "1", "MMHIP_PAIR_EXIT": "1"}),
    ("exit_cpp_tail", {"MMHIP_PAIR": "1", "MMHIP_PAIR_EXIT": "1", "MMHIP_PAIR_EXIT_TAIL": "0"}),
    ("per_iteration", {"MMHIP_PAIR": "1", "MMHIP_PAIR_EXIT": "0"}),
    ("unpaired", {"MMHIP_PAIR": "0"}),
]
SWITCHES = ("MMHIP_PAIR", "MMHIP_PAIR_EXIT", "MMHIP_PAIR_EXIT_TAIL")


def render_modes(make, sizes, monkeypatch, **render_args):
    """{(mode, size): frame} of the filter `make()` builds under each mode's environment"""
    outs = {}
    for label, env in MODES:
        for k in SWITCHES:
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        flt = make()
        paired = "mm_p += 2)" in flt.kernel_source
        assert paired == (label != "unpaired"), label
        assert ("#define MM_PAIR_EXIT 1\n" in flt.kernel_source) == label.startswith("exit"), label
        for w, h in sizes:
            outs[label, (w, h)] = flt.invoke(w, h).render(**render_args)
    return outs


@pytest.mark.parametrize("name", [p[0] for p in PROBES])
def test_probe_matches_oracle_in_every_mode(name, monkeypatch):
    src = by_name(name)
    outs = render_modes(lambda: mm.Filter(src), SIZES, monkeypatch)
    oracle = CpuFilter(mm.Filter(src).ir_json_raw)
    for (label, (w, h)), got in outs.items():
        want = oracle.render(w, h)
        assert np.array_equal(got, want), (name, label, w, h, int((got != want).sum()))


def test_launch_geometry_edges(monkeypatch):
    """The probe with every kind of exit copy on frames at the edges of the launch geometry (tests/launch_sizes.py): both
    sides of the first rows-per-work-item cut and the XCD-order round, partial last tile column and row group."""
    src = by_name("iv_and_lane_phi")
    monkeypatch.setenv("MMHIP_PAIR", "1")
    geo = mm.Filter(src).launch_geometry
    monkeypatch.delenv("MMHIP_PAIR")
    g = geo(64, 64)
    sizes = [(w, h) for _, w, h, _ in LS.cut_sizes(g["tile_w"], g["tile_h"])[:2]]
    sizes += [(w, h) for _, w, h, _ in LS.xcd_sizes(g["tile_w"], g["tile_h"], g["unroll"])]
    outs = render_modes(lambda: mm.Filter(src), sizes, monkeypatch)
    oracle = CpuFilter(mm.Filter(src).ir_json_raw)
    wants = {s: oracle.render(*s) for s in sizes}
    for (label, s), got in outs.items():
        assert np.array_equal(got, wants[s]), (label, s, int((got != wants[s]).sum()))


@pytest.mark.parametrize("spec", [False, True], ids=["generic", "specialised"])
def test_mandelbrot_in_every_mode(spec, monkeypatch):
    """The flagship filter, generic and with its user values baked in, on ragged frames."""
    def make():
        flt = F.load("mandelbrot")
        return flt.specialized({}) if spec else flt
    sizes = [(83, 61), (640, 333)]
    outs = render_modes(make, sizes, monkeypatch, t=0.25)
    oracle = CpuFilter(F.load("mandelbrot").ir_json_raw)
    wants = {s: oracle.render(*s, t=0.25) for s in sizes}
    for (label, s), got in outs.items():
        assert np.array_equal(got, wants[s]), (label, s, int((got != wants[s]).sum()))
