"""The counted back edge and the pair kernels' result pack on the GPU: every probe of tests/pair_count_probes.py, rendered
with the new defaults, with each new switch off (MMHIP_PAIR_EXIT_TAIL=1: the compare-and-mask tail, MMHIP_PAIR_PACK=0: a
pixel at a time through mm_store_pixel), with the per-iteration selects (MMHIP_PAIR_EXIT=0) and one pixel at a time
(MMHIP_PAIR=0), must give the oracle's bytes."""
import ctypes as C

import numpy as np
import pytest

import mathmap_amd as mm
from mathmap_amd._lib import lib
from oracle.ccgen import CpuFilter
from tests import filters as F
from tests import launch_sizes as LS
from tests.pair_count_probes import COUNT_PROBES, PACK_PROBES, SIZES, by_name

pytestmark = pytest.mark.gpu

# (label, environment)
MODES = [
    ("default", {"MMHIP_PAIR": "1"}),
    ("compare_tail", {"MMHIP_PAIR": "1", "MMHIP_PAIR_EXIT_TAIL": "1"}),
    ("pixel_store", {"MMHIP_PAIR": "1", "MMHIP_PAIR_PACK": "0"}),
    ("per_iteration", {"MMHIP_PAIR": "1", "MMHIP_PAIR_EXIT": "0"}),
    ("unpaired", {"MMHIP_PAIR": "0"}),
]
SWITCHES = ("MMHIP_PAIR", "MMHIP_PAIR_EXIT", "MMHIP_PAIR_EXIT_TAIL", "MMHIP_PAIR_PACK")


def filters_by_mode(src, monkeypatch):
    """[(mode, filter)] of the probe compiled under each mode's environment"""
    out = []
    for label, env in MODES:
        for k in SWITCHES:
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        flt = mm.Filter(src)
        ks = flt.kernel_source
        assert ("mm_p += 2)" in ks) == (label != "unpaired"), label
        assert ("mm_store_pair(" in ks) == (label in ("default", "compare_tail")), label
        out.append((label, flt))
    return out


def check_sizes(src, sizes, monkeypatch, uservals=None):
    oracle = CpuFilter(mm.Filter(src).ir_json_raw)
    wants = {s: oracle.render(*s, uservals=uservals) for s in sizes}
    for label, flt in filters_by_mode(src, monkeypatch):
        for w, h in sizes:
            inv = flt.invoke(w, h)
            for k, v in (uservals or {}).items():
                inv.set(k, v)
            got = inv.render()
            assert np.array_equal(got, wants[w, h]), (label, w, h, int((got != wants[w, h]).sum()))


def first_cut(src, monkeypatch):
    """the frame just below the first rows-per-work-item cut of the probe's launch geometry (tests/launch_sizes.py)"""
    monkeypatch.setenv("MMHIP_PAIR", "1")
    g = mm.Filter(src).launch_geometry(64, 64)
    monkeypatch.delenv("MMHIP_PAIR")
    return [(w, h) for _, w, h, _ in LS.cut_sizes(g["tile_w"], g["tile_h"])[:1]]


@pytest.mark.parametrize("name", [p[0] for p in COUNT_PROBES + PACK_PROBES])
def test_probe_matches_oracle_in_every_mode(name, monkeypatch):
    """Ragged frames, and one frame at the launch geometry's first cut."""
    src = by_name(name)
    check_sizes(src, SIZES + first_cut(src, monkeypatch), monkeypatch)


@pytest.mark.parametrize("name,uservals", [("register_bound", {"lim": 11}), ("register_bound", {"lim": 0}),
                                           ("register_init", {"start": 8}), ("register_init", {"start": 12})])
def test_register_probes_with_other_arguments(name, uservals, monkeypatch):
    """The run-time distance: a longer loop, a bound and a start at which no trip passes the test."""
    check_sizes(by_name(name), SIZES[:2], monkeypatch, uservals)


@pytest.mark.parametrize("name", ["step_two", "literal_alpha"])
def test_launch_geometry_edges(name, monkeypatch):
    """Frames at the edges of the launch geometry (tests/launch_sizes.py): both sides of the first rows-per-work-item cut
    and the XCD-order round, partial last tile column and row group."""
    src = by_name(name)
    monkeypatch.setenv("MMHIP_PAIR", "1")
    geo = mm.Filter(src).launch_geometry
    monkeypatch.delenv("MMHIP_PAIR")
    g = geo(64, 64)
    sizes = [(w, h) for _, w, h, _ in LS.cut_sizes(g["tile_w"], g["tile_h"])[1:2]]
    sizes += [(w, h) for _, w, h, _ in LS.xcd_sizes(g["tile_w"], g["tile_h"], g["unroll"])]
    check_sizes(src, sizes, monkeypatch)


def render_format(flt, w, h, bpp, floatmap):
    px = 16 if floatmap else bpp
    dev = lib().mmhip_device_alloc(w * h * px)
    assert dev
    try:
        inv = flt.invoke(w, h)
        inv.render_rows(dev, 0, h, bpp=bpp, floatmap=floatmap)
        inv.sync()
        out = np.empty((h, w, 4), np.float32) if floatmap else np.empty((h, w, bpp), np.uint8)
        assert lib().mmhip_copy_to_host(out.ctypes.data_as(C.c_void_p), C.c_void_p(dev), w * h * px) == 0
    finally:
        lib().mmhip_device_free(dev)
    return out


@pytest.mark.parametrize("name", ["two_equal", "literal_colour", "out_of_range"])
def test_other_output_formats_take_the_old_path(name, monkeypatch):
    """bpp 1 to 3 and float maps go through mm_store_pixel inside mm_store_pair: the oracle's bytes, and its floats bit for bit."""
    src = by_name(name)
    w, h = 83, 61
    oracle = CpuFilter(mm.Filter(src).ir_json_raw)
    flts = filters_by_mode(src, monkeypatch)[:3]
    for bpp, floatmap in ((1, False), (2, False), (3, False), (4, True)):
        want = oracle.render(w, h, bpp=bpp, floatmap=floatmap)
        for label, flt in flts:
            got = render_format(flt, w, h, bpp, floatmap)
            same = np.array_equal(got.view(np.uint32), want.view(np.uint32)) if floatmap else np.array_equal(got, want)
            assert same, (label, bpp, floatmap)


def test_specialised_mandelbrot_8192_equals_generic():
    w = h = 8192
    text = F.load("mandelbrot").specialized({}).kernel_source      # what the specialising filter compiles at invoke()
    assert "s_add_u32 %2, %2, 1" in text and "mm_store_pair(" in text
    a = F.load("mandelbrot").invoke(w, h).render()
    b = F.load("mandelbrot", specialize=True).invoke(w, h).render()
    assert np.array_equal(a, b)
