"""The peeled first loop trip on the GPU: every probe of tests/pair_peel_probes.py, compiled specialised, rendered with the
peel switched on (MMHIP_PAIR_PEEL=1), with the default (unpeeled), with each other new switch off, with the per-iteration selects (MMHIP_PAIR_EXIT=0) and
one pixel at a time (MMHIP_PAIR=0), on ragged frames and one frame at the launch geometry's first cut, must give the oracle's
bytes; the probe with a -0 in its first trip also its float map, bit for bit."""
import ctypes as C

import numpy as np
import pytest

import mathmap_amd as mm
from mathmap_amd._lib import lib
from oracle.ccgen import CpuFilter
from tests import launch_sizes as LS
from tests.pair_peel_probes import PEEL_PROBES, SIZES, by_name

pytestmark = pytest.mark.gpu

# (label, environment)
MODES = [
    ("peeled", {"MMHIP_PAIR": "1", "MMHIP_PAIR_PEEL": "1"}),
    ("default", {"MMHIP_PAIR": "1"}),
    ("compare_tail", {"MMHIP_PAIR": "1", "MMHIP_PAIR_PEEL": "1", "MMHIP_PAIR_EXIT_TAIL": "1"}),
    ("pixel_store", {"MMHIP_PAIR": "1", "MMHIP_PAIR_PEEL": "1", "MMHIP_PAIR_PACK": "0"}),
    ("per_iteration", {"MMHIP_PAIR": "1", "MMHIP_PAIR_PEEL": "1", "MMHIP_PAIR_EXIT": "0"}),
    ("unpaired", {"MMHIP_PAIR": "0", "MMHIP_PAIR_PEEL": "1"}),
]
SWITCHES = ("MMHIP_PAIR", "MMHIP_PAIR_EXIT", "MMHIP_PAIR_EXIT_TAIL", "MMHIP_PAIR_PACK", "MMHIP_PAIR_PEEL")


def filters_by_mode(src, monkeypatch):
    out = []
    for label, env in MODES:
        for k in SWITCHES:
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        flt = mm.Filter(src).specialized({})
        assert ("mm_p += 2)" in flt.kernel_source) == (label != "unpaired"), label
        out.append((label, flt))
    return out


@pytest.mark.parametrize("name", [p[0] for p in PEEL_PROBES])
def test_probe_matches_oracle_in_every_mode(name, monkeypatch):
    src = by_name(name)
    flts = filters_by_mode(src, monkeypatch)
    if dict((p[0], p[2]) for p in PEEL_PROBES)[name] > 0:
        assert flts[0][1].kernel_source != flts[1][1].kernel_source          # MMHIP_PAIR_PEEL=1 is the peeled text
    g = flts[0][1].launch_geometry(64, 64)
    sizes = SIZES + [(w, h) for _, w, h, _ in LS.cut_sizes(g["tile_w"], g["tile_h"])[:1]]
    oracle = CpuFilter(mm.Filter(src).ir_json_raw)
    for w, h in sizes:
        want = oracle.render(w, h, t=0.3)
        for label, flt in flts:
            got = flt.invoke(w, h).render(t=0.3)
            assert np.array_equal(got, want), (label, w, h, int((got != want).sum()))


def test_minus_zero_float_map_bit_for_bit(monkeypatch):
    src = by_name("minus_zero")
    w, h = 83, 61
    want = CpuFilter(mm.Filter(src).ir_json_raw).render(w, h, floatmap=True)
    assert np.signbit(want[..., 2]).any() and not np.signbit(want[..., 0]).any()
    for label, flt in filters_by_mode(src, monkeypatch):
        dev = lib().mmhip_device_alloc(w * h * 16)
        assert dev
        try:
            inv = flt.invoke(w, h)
            inv.render_rows(dev, 0, h, floatmap=True)
            inv.sync()
            got = np.empty((h, w, 4), np.float32)
            assert lib().mmhip_copy_to_host(got.ctypes.data_as(C.c_void_p), C.c_void_p(dev), w * h * 16) == 0
        finally:
            lib().mmhip_device_free(dev)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), label
