"""Whole frames at every launch geometry of the pixel kernel, HIP (through the C ABI) against the threaded CPU oracle.

The kernel's shape changes with the frame: rows per work-item (ppt 1 / 2 / 4 / 8 / 16 from the workgroup count),
partial last tile columns and row groups, XCD order 2's whole swizzle rounds, the multiply-high tile division and its
plain fallback.  tests/launch_sizes.py derives the sizes that reach each of them from the kernel's own geometry
(mmhip_filter_launch_geometry) and tests/test_launch_geometry_table.py checks, without a GPU, that they do.  Here every
pixel of those frames is compared, for one filter per kernel class; then forced geometries (the MMHIP_* hooks) on small
frames, which must equal the oracle and the default geometry byte for byte; then row bands and regions written into a
buffer with sentinel rows and a padded row stride, which must equal the full frame and leave every other byte alone."""
import ctypes as C
import os

import numpy as np
import pytest

import mathmap_amd as mm
from mathmap_amd._lib import lib
from oracle.ccgen import CpuFilter
from tests import filters as F
from tests import launch_sizes as L
from tests.expectations import Expectations
from tests.test_gpu_closures import BLUR_OF_CLOSURE

pytestmark = pytest.mark.gpu
EXP = Expectations("gpu_vs_oracle")
THREADS = max(1, min(16, len(os.sched_getaffinity(0))))
# the single-pixel class (Droste) is rendered whole at 8192^2 by tests/test_gpu_baseline_sizes.py
FRAME_CLASSES = ("pair", "unroll1", "short_fetch", "medium_fetch", "row_slice")
# classes whose result is their coordinates alone (or an exact function of them): held bit-exact, float map included
EXACT = ("pair", "unroll1", "short_fetch", "row_slice")
FLOATMAP_MAX_PIXELS = 4 << 20
CLOSURE_FRAME = (1024, 8200)          # the closure's own launch: 64 x 129 workgroups at ppt 4


def input_image():
    return F.synthetic_image(1024, 768, seed=5)


def chunked_stats(a, b, rows=1 << 16):
    """gpu_util.stats without its int64 copies of whole frames."""
    mx = nd = n1 = 0
    for r in range(0, a.shape[0], rows):
        d = np.abs(a[r:r + rows].astype(np.int16) - b[r:r + rows].astype(np.int16))
        if d.size:
            mx, nd, n1 = max(mx, int(d.max())), nd + int((d > 0).sum()), n1 + int((d > 1).sum())
    return mx, nd, n1


def render_whole(inv, w, h, t, floatmap=False):
    px = 16 if floatmap else 4
    dev = lib().mmhip_device_alloc(w * h * px)
    assert dev
    try:
        inv.render_rows(dev, 0, h, t=t, floatmap=floatmap)
        inv.sync()
        out = np.empty((h, w, 4), np.float32 if floatmap else np.uint8)
        assert lib().mmhip_copy_to_host(out.ctypes.data_as(C.c_void_p), C.c_void_p(dev), w * h * px) == 0
    finally:
        lib().mmhip_device_free(C.c_void_p(dev))
    return out


def first_difference(got, want):
    bad = np.argwhere(np.any(got != want, axis=-1))
    return None if not len(bad) else (tuple(int(v) for v in bad[0]), len(bad))


@pytest.mark.parametrize("name", FRAME_CLASSES)
def test_whole_frames_across_launch_buckets(name):
    flt = L.class_filter(name)
    assert L.class_errors(name, flt, flt.launch_geometry(64, 64)) == []
    cf = CpuFilter(flt.ir_json_raw)
    images = {"in": input_image()} if F.image_names(flt) else {}
    t = 0.3
    for lab, w, h in L.frame_cases(flt.launch_geometry):
        geo = flt.launch_geometry(w, h)
        inv = flt.invoke(w, h)
        for k, v in images.items():
            inv.set_image(k, v)
        got = render_whole(inv, w, h, t)
        want = cf.render(w, h, images=images, t=t, threads=THREADS)
        case = "geometry/%s/%s/%dx%d/ppt%d" % (name, lab, w, h, geo["ppt"])
        if name in EXACT:
            assert np.array_equal(got, want), (case, geo, first_difference(got, want))
        else:
            mx, nd, n1 = chunked_stats(got, want)
            EXP.check(case, mx, nd, n1, got.size)
        del got, want
        if name in EXACT and w * h <= FLOATMAP_MAX_PIXELS:
            gm = render_whole(inv, w, h, t, floatmap=True)
            wm = cf.render(w, h, images=images, t=t, threads=THREADS, floatmap=True)
            assert np.array_equal(gm.view(np.uint32), wm.view(np.uint32)), (case, "float map")


# (class, hooks, frame): about 30 forced geometries on small frames
FORCED = [
    ("pair", {"MMHIP_PPT": "1"}, (333, 251)), ("pair", {"MMHIP_PPT": "3"}, (333, 251)),
    ("pair", {"MMHIP_PPT": "16"}, (1, 517)), ("pair", {"MMHIP_PPT": "5"}, (333, 251)),
    ("unroll1", {"MMHIP_PPT": "2"}, (333, 251)), ("unroll1", {"MMHIP_PPT": "5"}, (1, 517)),
    ("unroll1", {"MMHIP_PPT": "16"}, (333, 251)),
    ("short_fetch", {"MMHIP_PPT": "1"}, (333, 251)), ("short_fetch", {"MMHIP_PPT": "16"}, (333, 251)),
    ("short_fetch", {"MMHIP_PPT": "5"}, (1, 517)),
    ("row_slice", {"MMHIP_PPT": "3"}, (333, 251)), ("medium_fetch", {"MMHIP_PPT": "16"}, (333, 251)),
    ("pair", {"MMHIP_TILE_W": "8"}, (333, 251)), ("short_fetch", {"MMHIP_TILE_W": "32"}, (333, 251)),
    ("unroll1", {"MMHIP_TILE_W": "256"}, (333, 251)), ("row_slice", {"MMHIP_TILE_W": "256"}, (1, 517)),
    ("medium_fetch", {"MMHIP_TILE_W": "8"}, (333, 251)),
    ("pair", {"MMHIP_XCD_ORDER": "0"}, (333, 251)), ("unroll1", {"MMHIP_XCD_ORDER": "1"}, (333, 251)),
    ("short_fetch", {"MMHIP_XCD_ORDER": "1"}, (333, 251)), ("medium_fetch", {"MMHIP_XCD_ORDER": "0"}, (333, 251)),
    ("pair", {"MMHIP_UNROLL": "1"}, (333, 251)), ("pair", {"MMHIP_UNROLL": "3"}, (333, 251)),
    ("short_fetch", {"MMHIP_UNROLL": "8"}, (333, 251)), ("row_slice", {"MMHIP_UNROLL": "3"}, (1, 517)),
    ("medium_fetch", {"MMHIP_UNROLL": "8"}, (333, 251)),
    ("pair", {"MMHIP_UNROLL": "3", "MMHIP_PPT": "5"}, (333, 251)),
    ("short_fetch", {"MMHIP_TILE_W": "8", "MMHIP_PPT": "16"}, (333, 251)),
    ("unroll1", {"MMHIP_TILE_W": "256", "MMHIP_UNROLL": "8", "MMHIP_PPT": "3"}, (333, 251)),
    ("row_slice", {"MMHIP_TILE_W": "32", "MMHIP_XCD_ORDER": "1", "MMHIP_PPT": "2"}, (1, 517)),
    ("medium_fetch", {"MMHIP_TILE_W": "256", "MMHIP_UNROLL": "3", "MMHIP_PPT": "5"}, (1, 517)),
]


def _forced_id(c):
    return "%s-%s-%dx%d" % (c[0], "-".join("%s%s" % (k[6:].lower(), v) for k, v in sorted(c[1].items())), *c[2])


@pytest.mark.parametrize("name,hooks,frame", FORCED, ids=[_forced_id(c) for c in FORCED])
def test_forced_geometry_equals_default_and_oracle(name, hooks, frame, monkeypatch):
    w, h = frame
    images = {"in": input_image()} if name != "pair" and name != "unroll1" else {}
    t = 0.6

    def render(flt):
        inv = flt.invoke(w, h)
        for k, v in images.items():
            inv.set_image(k, v)
        return render_whole(inv, w, h, t)

    base = L.class_filter(name)
    default = render(base)
    for k, v in hooks.items():
        monkeypatch.setenv(k, v)
    flt = L.class_filter(name)
    g = flt.launch_geometry(w, h)
    # the hooks took effect (a forced geometry that is not reached must fail, not pass)
    if "MMHIP_TILE_W" in hooks:
        assert g["tile_w"] == int(hooks["MMHIP_TILE_W"]) and g["tile_h"] == 256 // g["tile_w"], g
    if "MMHIP_UNROLL" in hooks:
        assert g["unroll"] == int(hooks["MMHIP_UNROLL"]) and not g["pair_mode"], g
        assert "#define MM_UNROLL %s\n" % hooks["MMHIP_UNROLL"] in flt.kernel_source
    if "MMHIP_XCD_ORDER" in hooks:
        assert g["xcd_order"] == int(hooks["MMHIP_XCD_ORDER"])
        assert "#define MM_XCD_ORDER %s\n" % hooks["MMHIP_XCD_ORDER"] in flt.kernel_source
    if "MMHIP_PPT" in hooks:
        assert g["ppt"] == L.round_up(int(hooks["MMHIP_PPT"]), g["unroll"]), g
    got = render(flt)
    assert np.array_equal(got, default), (_forced_id((name, hooks, frame)), g, first_difference(got, default))
    want = CpuFilter(flt.ir_json_raw).render(w, h, images=images, t=t)
    if name in EXACT:
        assert np.array_equal(got, want), first_difference(got, want)
    else:
        mx, nd, n1 = chunked_stats(got, want)
        EXP.check("geometry/forced/%s" % _forced_id((name, hooks, frame)), mx, nd, n1, got.size)


# ---- row bands and regions stay inside their rows ----

SENTINEL_ROWS = 3


def band_into_sentinels(inv, first, last, bpp, floatmap, region, rw, render_w, t):
    """Renders rows [first, last) into a buffer of SENTINEL_ROWS filler rows above and below the band and a padded row
    stride (a float map's rows are the frame's render width apart, so its padding is the rest of each row), filled
    with a byte pattern first.  Returns (band [rows, rw, px], whether every byte outside the band's pixels is intact)."""
    px = 16 if floatmap else bpp
    stride = render_w * 16 if floatmap else rw * bpp + 13
    n = last - first
    nbytes = stride * (n + 2 * SENTINEL_ROWS)
    pattern = np.random.default_rng(first * 7 + bpp).integers(0, 256, nbytes, dtype=np.uint8)
    dev = lib().mmhip_device_alloc(nbytes)
    assert dev
    try:
        assert lib().mmhip_copy_to_device(C.c_void_p(dev), pattern.ctypes.data_as(C.c_void_p), nbytes) == 0
        inv.render_rows(dev + SENTINEL_ROWS * stride, first, last, t=t, row_stride=stride, bpp=bpp, floatmap=floatmap,
                        region=region)
        inv.sync()
        host = np.empty(nbytes, np.uint8)
        assert lib().mmhip_copy_to_host(host.ctypes.data_as(C.c_void_p), C.c_void_p(dev), nbytes) == 0
    finally:
        lib().mmhip_device_free(C.c_void_p(dev))
    mask = np.zeros((n + 2 * SENTINEL_ROWS, stride), bool)
    mask[SENTINEL_ROWS:SENTINEL_ROWS + n, :rw * px] = True
    rows = host.reshape(-1, stride)
    intact = np.array_equal(rows[~mask], pattern.reshape(-1, stride)[~mask])
    band = rows[SENTINEL_ROWS:SENTINEL_ROWS + n, :rw * px].copy()
    return band, intact


def band_set(h, geo):
    """1 row, 7 rows and right after them 7 rows ending at the last row (as many rows as the launch before: what a
    launch may keep of the one before must not be its rows), tile_h * ppt - 1 and + 1 rows, a long band ending at the
    last row."""
    g = geo["tile_h"] * geo["ppt"]
    return [(5, 6), (11, 18), (h - 7, h), (40, 40 + g - 1), (h // 2, h // 2 + g + 1), (7, h)]


@pytest.mark.parametrize("name", ["pair", "row_slice"])
def test_bands_and_regions_stay_inside_their_rows(name):
    flt = L.class_filter(name)
    g0 = flt.launch_geometry(64, 64)
    w = 2047
    tiles_x = -(-w // g0["tile_w"])
    h = -(-40000 // tiles_x) * g0["tile_h"] + 5
    geo = flt.launch_geometry(w, h)
    assert geo["ppt"] >= 4 and geo["wg1"] >= 32768, geo
    images = {"in": input_image()} if F.image_names(flt) else {}
    inv = flt.invoke(w, h)
    for k, v in images.items():
        inv.set_image(k, v)
    cf = CpuFilter(flt.ir_json_raw)
    t = 0.45
    bands = band_set(h, geo)
    rx, ry, rw, rh = 37, 101, w - 37 - 29, h - 101 - 3
    # the long band runs at ppt >= 4 too, in the frame and in the region
    assert flt.launch_geometry(w, h - 7)["ppt"] >= 4 and flt.launch_geometry(rw, rh - 7)["ppt"] >= 4
    bad = []
    for bpp, floatmap in ((4, False), (1, False), (2, False), (3, False), (4, True)):
        want = cf.render(w, h, images=images, t=t, bpp=bpp, floatmap=floatmap, threads=THREADS)
        px = 16 if floatmap else bpp
        full = want.view(np.uint8).reshape(h, w * px)
        for region in (None, (rx, ry, rw, rh)):
            off_x, off_y, cw = (0, 0, w) if region is None else (rx, ry, rw)
            for lo, hi in bands:
                if region is not None:
                    lo, hi = min(ry + lo, ry + rh - 1), min(ry + hi, ry + rh)
                band, intact = band_into_sentinels(inv, lo, hi, bpp, floatmap, region, cw, w, t)
                tag = (bpp, floatmap, region, lo, hi)
                if not intact:
                    bad.append(("bytes outside the band changed",) + tag)
                ref = full[lo:hi, off_x * px:(off_x + cw) * px]
                if not np.array_equal(band, ref):
                    bad.append(("band differs",) + tag + (first_difference(band, ref),))
    assert not bad, (name, geo, bad)


def test_closure_band_stays_inside_its_rows():
    """BLUR_OF_CLOSURE at a frame where the closure image's own launch runs at ppt >= 4: the whole frame equals the
    oracle, row bands written between sentinel rows equal its rows and touch nothing else."""
    w, h = CLOSURE_FRAME
    flt = mm.Filter(BLUR_OF_CLOSURE)
    assert flt.launch_geometry(w, h, closure=0)["ppt"] >= 4
    img = F.synthetic_image(w, h, seed=3)
    inv = flt.invoke(w, h)
    inv.set("k", 1.3)
    inv.set_image("in", img)
    t = 0.6
    full = render_whole(inv, w, h, t)
    # (one oracle thread: its native filters share the frame's memo of results between the rows it renders)
    want = CpuFilter(flt.ir_json_raw).render(w, h, uservals={"k": 1.3}, images={"in": img}, t=t)
    assert np.array_equal(full, want), first_difference(full, want)
    for lo, hi in ((0, 1), (77, 84), (h // 2, h // 2 + 63), (h - 1500, h)):
        band, intact = band_into_sentinels(inv, lo, hi, 4, False, None, w, w, t)
        assert intact, (lo, hi)
        assert np.array_equal(band.reshape(hi - lo, w, 4), full[lo:hi]), (lo, hi)
