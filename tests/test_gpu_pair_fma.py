"""The fused doubling of exit-driven pair-mode loops on the GPU: every probe of tests/pair_fma_probes.py, compiled specialised,
rendered with the defaults (fused, under its guard), with MMHIP_PAIR_FMA2=0, with the per-iteration selects
(MMHIP_PAIR_EXIT=0) and one pixel at a time (MMHIP_PAIR=0), on a ragged frame and one frame at the launch geometry's first
cut, must give the oracle's bytes; the overflow probes and the probe of signed zeros and denormals also their float maps, bit
for bit; and the specialised Mandelbrot kernel the generic kernel's and the oracle's frame."""
import ctypes as C

import numpy as np
import pytest

import mathmap_amd as mm
from mathmap_amd._lib import lib
from oracle.ccgen import CpuFilter
from tests import filters as F
from tests import launch_sizes as LS
from tests.pair_fma_probes import FMA_PROBES, RAGGED, by_name

pytestmark = pytest.mark.gpu

# (label, environment)
MODES = [
    ("default", {"MMHIP_PAIR": "1"}),
    ("unfused", {"MMHIP_PAIR": "1", "MMHIP_PAIR_FMA2": "0"}),
    ("per_iteration", {"MMHIP_PAIR": "1", "MMHIP_PAIR_EXIT": "0"}),
    ("unpaired", {"MMHIP_PAIR": "0"}),
]
SWITCHES = ("MMHIP_PAIR", "MMHIP_PAIR_EXIT", "MMHIP_PAIR_EXIT_TAIL", "MMHIP_PAIR_PACK", "MMHIP_PAIR_PEEL", "MMHIP_PAIR_FMA2")
FUSED = dict((p[0], p[2]) for p in FMA_PROBES)


def filters_by_mode(name, monkeypatch):
    """[(mode, filter)] of the probe compiled under each mode's environment"""
    out = []
    for label, env in MODES:
        for k in SWITCHES:
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        flt = mm.Filter(by_name(name)).specialized({})
        ks = flt.kernel_source
        assert ("mm_p += 2)" in ks) == (label != "unpaired"), label
        assert ks.count("__builtin_fmaf(") == (2 * FUSED[name] if label == "default" else 0), label
        out.append((label, flt))
    return out


def render_float_map(flt, w, h):
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
    return got


@pytest.mark.parametrize("name", [p[0] for p in FMA_PROBES])
def test_probe_matches_oracle_in_every_mode(name, monkeypatch):
    """A ragged 67 x 41 frame, and one frame at the launch geometry's first cut."""
    flts = filters_by_mode(name, monkeypatch)
    g = flts[0][1].launch_geometry(64, 64)
    sizes = [RAGGED] + [(w, h) for _, w, h, _ in LS.cut_sizes(g["tile_w"], g["tile_h"])[:1]]
    oracle = CpuFilter(mm.Filter(by_name(name)).ir_json_raw)
    for w, h in sizes:
        want = oracle.render(w, h)
        for label, flt in flts:
            got = flt.invoke(w, h).render()
            assert np.array_equal(got, want), (label, w, h, int((got != want).sum()))


@pytest.mark.parametrize("name", ["overflow", "overflow_half", "zeros_denormals"])
def test_float_map_bit_for_bit(name, monkeypatch):
    """+inf where t + t overflows (a bare fma would leave a finite value), the signs of zeros, denormals."""
    w, h = RAGGED
    want = CpuFilter(mm.Filter(by_name(name)).ir_json_raw).render(w, h, floatmap=True)
    if name == "zeros_denormals":
        assert np.signbit(want[..., 0]).any() and ((np.abs(want[..., 1]) > 0) & (np.abs(want[..., 1]) < 1e-38)).any()
    else:
        assert np.isposinf(want[..., 0]).sum() > 200
    for label, flt in filters_by_mode(name, monkeypatch):
        got = render_float_map(flt, w, h)
        diff = got.view(np.uint32) != want.view(np.uint32)
        assert not diff.any(), (label, int(diff.sum()))


def test_specialised_mandelbrot_equals_generic_and_oracle(monkeypatch):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    w, h = 256, 192
    spec = F.load("mandelbrot", specialize=True)
    text = F.load("mandelbrot").specialized({}).kernel_source      # what the specialising filter compiles at invoke()
    assert text.count("__builtin_fmaf(") == 2 and "mm_fma2_ok(" in text
    generic = F.load("mandelbrot")
    assert "__builtin_fmaf(" not in generic.kernel_source
    a = generic.invoke(w, h).render()
    b = spec.invoke(w, h).render()
    want = CpuFilter(generic.ir_json_raw).render(w, h)
    assert int((a != b).sum()) == 0 and int((b != want).sum()) == 0
    assert len(np.unique(b[..., 0])) > 16          # the escape bands are there
