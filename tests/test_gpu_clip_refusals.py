"""What the three clip entry points refuse (mmhip_render_clip, mmhip_render_clip_supersampled, mmhip_render_clip_shutter):
the whole text of mmhip_last_error() for every argument check, the order of the checks, the empty row band that returns 0
without writing, and the smallest frame stride that is accepted.  The expected texts are written out here, not taken from
the library.  Nothing but the accepted strides at the end of a test launches a kernel, and up to there the clip counters
stay 0."""
import ctypes as C

import numpy as np
import pytest

import mathmap_amd as mm
from mathmap_amd._lib import lib

pytestmark = pytest.mark.gpu
SRC = "filter f () rgba:[t, 0, 0, 1] end"
W = H = 8
BYTES = 4096
SENTINEL = 0xA5
ENTRIES = ("render_clip", "render_clip_supersampled", "render_clip_shutter")
HAS_ROWS_AND_FLOATMAP = ("render_clip", "render_clip_shutter")


@pytest.fixture(scope="module")
def flt():
    return mm.Filter(SRC, supersampling=True)


@pytest.fixture
def dev():
    p = lib().mmhip_device_alloc(BYTES)
    assert p
    fill = np.full(BYTES, SENTINEL, np.uint8)
    assert lib().mmhip_copy_to_device(C.c_void_p(p), fill.ctypes.data_as(C.c_void_p), BYTES) == 0
    yield p
    lib().mmhip_device_free(C.c_void_p(p))


def call(entry, inv, dev, n=2, frames=True, ts=True, samples=2, span=0.1, region_w=W, region_h=H, first_row=0, last_row=H,
         row_stride=W * 4, frame_stride=W * H * 4, bpp=4, floatmap=0):
    """One call of mmhip_<entry> through the C ABI (entry points without rows or floatmap do not get them); (rc, message)."""
    fr = (C.c_int * 2)(0, 1) if frames else None
    tt = (C.c_float * 2)(0.0, 0.5) if ts else None
    region = [0, 0, region_w, region_h]
    rows = [first_row, last_row]
    out = [C.c_void_p(dev), row_stride, C.c_int64(frame_stride), bpp]
    if entry == "render_clip":
        args = [n, fr, tt] + region + rows + out + [floatmap]
    elif entry == "render_clip_supersampled":
        args = [n, fr, tt] + region + out
    else:
        args = [n, fr, tt, samples, C.c_float(span)] + region + rows + out + [floatmap]
    rc = getattr(lib(), "mmhip_" + entry)(inv._h, *(args + [None]))
    return rc, lib().mmhip_last_error().decode()


def counters(inv):
    return (lib().mmhip_clip_batched_launches(inv._h), lib().mmhip_clip_supersampled_batches(inv._h),
            lib().mmhip_clip_shutter_batches(inv._h))


def refused(entry, inv, dev, message, **kw):
    rc, got = call(entry, inv, dev, **kw)
    assert rc == -1, (entry, kw, rc)
    assert got == message, (entry, kw, got)
    assert counters(inv) == (0, 0, 0), (entry, kw)


def device_bytes(dev):
    out = np.empty(BYTES, np.uint8)
    assert lib().mmhip_copy_to_host(out.ctypes.data_as(C.c_void_p), C.c_void_p(dev), BYTES) == 0
    return out


@pytest.mark.parametrize("entry", ENTRIES)
def test_argument_checks_their_texts_and_their_order(flt, dev, entry):
    inv = flt.invoke(W, H)
    arrays = entry + ": frames and ts must be arrays of num_frames entries"
    refused(entry, inv, dev, entry + ": num_frames must be at least 1", n=0)
    refused(entry, inv, dev, arrays, frames=False)
    refused(entry, inv, dev, arrays, ts=False)
    refused(entry, inv, dev, "output_bpp must be 1..4", bpp=0)
    refused(entry, inv, dev, "output_bpp must be 1..4", bpp=5)
    refused(entry, inv, dev, "empty region", region_w=0)
    refused(entry, inv, dev, "empty region", region_h=0)
    refused(entry, inv, dev, entry + ": frame_stride 255 is smaller than one frame's band (256 bytes)", frame_stride=255)
    if entry in HAS_ROWS_AND_FLOATMAP:
        refused(entry, inv, dev, entry + ": frame_stride 1023 is smaller than one frame's band (1024 bytes)", frame_stride=1023, floatmap=1)
    # the order of the checks
    refused(entry, inv, dev, entry + ": num_frames must be at least 1", n=0, bpp=0)
    refused(entry, inv, dev, "output_bpp must be 1..4", bpp=0, region_w=0)
    if entry in HAS_ROWS_AND_FLOATMAP:
        # an empty band after the clamp of the rows: nothing to do, nothing written (the stride is not looked at: 0 is too small)
        for first, last, stride in ((5, 5, 256), (7, 3, 0)):
            assert call(entry, inv, dev, first_row=first, last_row=last, frame_stride=stride)[0] == 0
            assert counters(inv) == (0, 0, 0)
        assert (device_bytes(dev) == SENTINEL).all()
    # the smallest strides that hold a frame's band are accepted (these render: the counters move from here on)
    assert call(entry, inv, dev, frame_stride=256)[0] == 0
    if entry in HAS_ROWS_AND_FLOATMAP:
        assert call(entry, inv, dev, frame_stride=1024, floatmap=1)[0] == 0
        # rows outside the region are clamped to it (new_template.c.in:238-239): the whole region is the band
        assert call(entry, inv, dev, first_row=-3, last_row=100)[0] == 0
    assert lib().mmhip_sync(inv._h) == 0


def test_shutter_checks_that_come_first(flt, dev):
    inv = flt.invoke(W, H)
    e = "render_clip_shutter"
    refused(e, inv, dev, "render_clip_shutter: samples must be 1 to 256, not 0", samples=0)
    refused(e, inv, dev, "render_clip_shutter: samples must be 1 to 256, not 257", samples=257)
    refused(e, inv, dev, "render_clip_shutter: samples must be 1 to 256, not 0", samples=0, n=0)
    refused(e, inv, dev, "render_clip_shutter: samples must be 1 to 256, not 257", samples=257, n=0)
    # one sample per frame is the plain clip: its checks, under its name
    refused(e, inv, dev, "render_clip: num_frames must be at least 1", samples=1, n=0)
    refused(e, inv, dev, "render_clip_shutter: span must be finite", samples=2, span=float("nan"), n=0)


def test_shutter_refuses_a_region_wider_than_the_render_width(flt, dev):
    inv = flt.invoke(W, H)
    inv.set_render_size(4, 8)
    refused("render_clip_shutter", inv, dev, "render_clip_shutter: the region is wider than the render width", region_w=8)
