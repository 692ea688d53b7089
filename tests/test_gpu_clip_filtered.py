"""Filtered clips on the GPU (mmhip_render_clip_filtered: sub-sample maps of a haloed rectangle under k_filter_combine_clip).

The yardstick is tests/clip_filter_reference.py: the sub-samples are whole-frame render_rows(floatmap=True) calls of a
*second* invocation at the grid's offsets and the restated times, put through the restatement's two sums.  Everything is
compared bit for bit, in whole sentinel-filled buffers: float maps by NaN position and bit pattern, bytes as they are."""
import ctypes as C
import hashlib
import itertools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import mathmap_amd as mm
from mathmap_amd._lib import lib, selftest_lib
from tests import clip_filter_reference as X
from tests import filters as F
from tests import sample_grid_reference as G
from tests import shutter_fused_probes as P
from tests import shutter_reference as R
from tests.fetch_reference import pack
from tests.test_gpu_clip_sampled import PROBES, Layout, compiled, invoke, sub_sample_maps
from tests.test_gpu_clip_shutter import SENTINEL, device_filled, device_read, read_png, same_buffer

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "mathmap_amd", "mathmap_hip_cli")
f32 = np.float32
W, H, SPAN = P.W, P.H, 0.07
FRAMES, TS = [1, 0], [0.3, 0.8]


def render(inv, lay, aa, aa_filter, aa_radius=None, samples=1, span=None, frames=FRAMES, ts=TS, region=None, rows=None):
    dev = device_filled(lay.total)
    try:
        assert inv.render_clip(frames=frames, ts=ts, out_ptr=dev + lay.lead, rows=rows, region=region, row_stride=lay.stride,
                               frame_stride=lay.fstride, bpp=lay.bpp, floatmap=lay.floatmap, shutter_samples=samples,
                               shutter_span=span, aa=aa, aa_filter=aa_filter, aa_radius=aa_radius) is None
        inv.sync()
        return device_read(dev, lay.total)
    finally:
        lib().mmhip_device_free(C.c_void_p(dev))


def restated(flt, image, w, h, aa, aa_filter, radius, samples=1, span=0.0, frames=FRAMES, ts=TS):
    """The float frames [N, h, w, 4] the statement gives, from a second invocation's whole-frame sub-samples."""
    other = invoke(flt, image, w, h)
    subs = sub_sample_maps(other, frames, ts, samples, span, aa)
    return [X.frame(subs[i], X.KERNELS[aa_filter], radius) for i in range(len(frames))]


# ---- 1. the main sweep, against the restatement ----

SIZES = [(1, 1), (2, 1), (3, 4), (16, 16), (17, 17), (97, 61)]
FILTERS = [("box", 0.5), ("tent", 1.0), ("tent", 1.5), ("gaussian", 1.5), ("mitchell", 2.0)]
GRIDS = [1, 2, 3, (2, 1), (1, 3)]
NAMES = ["rotate", "pair", "rand", "wave", "blur"]
# the cross product has 750 members: every 11th of it (11 shares no factor with the 5s and the 6, so sizes, filters, grids
# and probes all rotate against each other), and tent at radius 4 (D = 4) at 17 x 17 with every grid
SWEEP = [case for k, case in enumerate(itertools.product(SIZES, FILTERS, GRIDS, NAMES)) if k % 11 == 0]
SWEEP += [((17, 17), ("tent", 4.0), grid, NAMES[k]) for k, grid in enumerate(GRIDS)]


def sweep_id(case):
    (w, h), (name, radius), grid, probe = case
    return "%dx%d-%s%g-aa%s-%s" % (w, h, name, radius, "x".join(str(v) for v in G.grid(grid)), probe)


def test_the_sweep_covers_what_it_should():
    assert 70 <= len(SWEEP) <= 80                       # two formats each: near 150 renders
    for k, values in enumerate((SIZES, FILTERS, GRIDS, NAMES)):
        assert {case[k] for case in SWEEP[:-5]} == set(values), k
    assert [case[:2] for case in SWEEP[-5:]] == [((17, 17), ("tent", 4.0))] * 5 and [case[2] for case in SWEEP[-5:]] == GRIDS


@pytest.mark.parametrize("case", SWEEP, ids=sweep_id)
def test_frames_equal_the_restatement(case):
    (w, h), (aa_filter, radius), aa, name = case
    flt, image = compiled(name)
    want_px = restated(flt, image, w, h, aa, aa_filter, radius)
    inv = invoke(flt, image, w, h)
    for floatmap in (True, False):
        lay = Layout(len(FRAMES), w, h, w, floatmap=floatmap, gap=80)
        got = render(inv, lay, aa, aa_filter, radius)
        want = lay.expected([m if floatmap else pack(m, 4) for m in want_px])
        assert same_buffer(got, want, floatmap), (sweep_id(case), "floatmap" if floatmap else "bytes")
    assert inv.clip_filtered_batches() == 2
    assert inv.clip_sampled_batches() == 0 and inv.clip_shutter_batches() == 0 and inv.clip_adaptive_batches() == 0


def test_default_radii_are_the_stated_ones():
    flt, image = compiled("rotate")
    inv = invoke(flt, image, 17, 17)
    for aa_filter, radius in X.DEFAULT_RADII.items():
        lay = Layout(len(FRAMES), 17, 17, 17, floatmap=True)
        assert np.array_equal(render(inv, lay, 2, aa_filter), render(inv, lay, 2, aa_filter, radius)), aa_filter


# ---- 2. bands and regions equal the same pixels of the whole-frame call ----

@pytest.fixture(scope="module")
def whole_frame():
    """Mitchell at radius 2 (D = 2) over a 2 x 2 grid of the 97 x 61 rotate probe: the whole-frame call, as floats and bytes."""
    flt, image = compiled("rotate")
    inv = invoke(flt, image)
    out = {}
    for floatmap in (True, False):
        lay = Layout(len(FRAMES), W, H, W, floatmap=floatmap)
        buf = render(inv, lay, 2, "mitchell")[lay.lead:lay.lead + len(FRAMES) * lay.fstride]
        out[floatmap] = buf.view(f32).reshape(len(FRAMES), H, W, 4) if floatmap else buf.reshape(len(FRAMES), H, W, 4)
    return out


@pytest.mark.parametrize("case", ["band 0-7", "band 7-8", "band 8-61", "region"])
def test_bands_and_regions_equal_the_whole_frame_call(whole_frame, case):
    region, rows = {"band 0-7": (None, (0, 7)), "band 7-8": (None, (7, 8)), "band 8-61": (None, (8, 61)), "region": ((5, 3, 40, 30), None)}[case]
    rx, ry, rw, rh = region if region is not None else (0, 0, W, H)
    first, last = rows if rows is not None else (ry, ry + rh)
    flt, image = compiled("rotate")
    inv = invoke(flt, image)
    for floatmap in (True, False):
        lay = Layout(len(FRAMES), rw, last - first, W, floatmap=floatmap, gap=48)
        got = render(inv, lay, 2, "mitchell", region=region, rows=rows)
        want = lay.expected([whole_frame[floatmap][i, first:last, rx:rx + rw] for i in range(len(FRAMES))])
        assert same_buffer(got, want, floatmap), (case, floatmap)


@pytest.mark.parametrize("bpp", [1, 2, 3])
def test_padded_rows_and_frame_gaps_at_every_format(bpp):
    flt, image = compiled("rotate")
    want_px = restated(flt, image, W, H, (2, 1), "gaussian", 1.5)
    inv = invoke(flt, image)
    region = (5, 3, 40, 30)
    lay = Layout(len(FRAMES), 40, 30, W, bpp=bpp, row_pad=13, gap=101, lead=61 + bpp)
    got = render(inv, lay, (2, 1), "gaussian", region=region)
    want = lay.expected([pack(m[3:33, 5:45], bpp) for m in want_px])
    assert np.array_equal(got, want), bpp


# ---- 3. box at radius 0.5 is the existing grid mean where the association cannot matter ----

@pytest.mark.parametrize("aa", [(2, 1), (1, 2), (4, 1)], ids=str)
@pytest.mark.parametrize("name", ["rotate", "pair"])
def test_box_at_half_a_pixel_equals_the_grid_mean(name, aa):
    """With weights 1/2 or 1/4 along one axis and 1 along the other every product is exact, so the two associations give
    the same bits -- as long as no sub-sample is a denormal (a scaled one would lose bits) or -0 (its sum with +0 depends on
    the order).  That is checked here on the CPU, from the oracle's float maps at the same offsets, before the GPU is asked."""
    from oracle.ccgen import CpuFilter
    w, h = 33, 21
    flt, image = compiled(name)
    assert image is None
    images = {"in": F.synthetic_image(w, h, seed=5)} if F.image_names(flt) else {}
    cpu = CpuFilter(flt.ir_json_raw)
    for a in range(aa[0]):
        for b in range(aa[1]):
            for t, frame in zip(TS, FRAMES):
                bits = cpu.render(w, h, images=images, t=t, frame=frame, floatmap=True,
                                  sampling_offset=(float(G.offsets(aa[0])[a]), float(G.offsets(aa[1])[b]))).view(np.uint32)
                assert not (((bits & 0x7f800000) == 0) & ((bits & 0x007fffff) != 0)).any() and not (bits == 0x80000000).any(), (name, aa, a, b, t)
    inv = invoke(flt, image, w, h)
    for floatmap in (True, False):
        lay = Layout(len(FRAMES), w, h, w, floatmap=floatmap)
        got = render(inv, lay, aa, "box", 0.5)
        dev = device_filled(lay.total)
        try:
            inv.render_clip(frames=FRAMES, ts=TS, out_ptr=dev + lay.lead, row_stride=lay.stride, frame_stride=lay.fstride, floatmap=floatmap, aa=aa)
            inv.sync()
            plain = device_read(dev, lay.total)
        finally:
            lib().mmhip_device_free(C.c_void_p(dev))
        assert same_buffer(got, plain, floatmap), (name, aa, floatmap)
    assert inv.clip_filtered_batches() == 2 and inv.clip_sampled_batches() == 2


# ---- 4. with a shutter ----

def test_a_shutter_of_three_under_a_tent():
    flt, image = compiled("rotate")
    want_px = restated(flt, image, W, H, 2, "tent", 1.0, samples=3, span=SPAN)
    plain_px = restated(flt, image, W, H, 2, "tent", 1.0)
    assert not R.same_floats(want_px[0], plain_px[0])
    inv = invoke(flt, image)
    inv.enable_timing(True)
    for floatmap in (True, False):
        lay = Layout(len(FRAMES), W, H, W, floatmap=floatmap, gap=16)
        got = render(inv, lay, 2, "tent", samples=3, span=SPAN)
        assert same_buffer(got, lay.expected([m if floatmap else pack(m, 4) for m in want_px]), floatmap), floatmap
    assert [name for name, ms in inv.drain_native_kernel_ms()] == ["filter_combine_clip"] * 2      # one pass per call


CHILD = r"""
import hashlib, json, sys
sys.path.insert(0, %r)
from tests.test_gpu_clip_filtered import compiled, invoke, W, H, SPAN
flt, image = compiled("rotate")
inv = invoke(flt, image)
inv.enable_timing(True)
n = int(sys.argv[1])
frames, ts = list(range(n)), [0.1 + 0.2 * i for i in range(n)]
out = inv.render_clip(frames=frames, ts=ts, shutter_samples=3, shutter_span=SPAN, aa=2, aa_filter="tent")
print(json.dumps({"plan": flt.clip_filtered_plan(W, H, W, H, 3, 2, "tent", n), "batches": inv.clip_filtered_batches(),
                  "native": [name for name, ms in inv.drain_native_kernel_ms()], "sha": hashlib.sha256(out.tobytes()).hexdigest()}))
"""


@pytest.mark.parametrize("case", ["two batches", "carry"])
def test_batches_and_passes_leave_the_bytes_alone(case):
    bps = H * 16 * W                                       # the whole frame: the halo is clipped away
    if case == "two batches":            # a frame is 3 * 4 maps, two fit: 3 frames are 2 + 1
        n, budget, want = 3, 24 * bps + 100, dict(frames_per_batch=2, batches=2, steps_per_pass=3, passes=1, carry=0)
    else:                                # 5 maps: (5 - 1) / 4 = 1 time step per pass beside the carry
        n, budget, want = 1, 5 * bps, dict(frames_per_batch=1, batches=1, steps_per_pass=1, passes=3, carry=1)
    env = dict(os.environ, MMHIP_CLIP_SHUTTER_BYTES=str(budget))
    r = subprocess.run([sys.executable, "-c", CHILD % ROOT, str(n)], cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    res = json.loads(r.stdout.strip().splitlines()[-1])
    assert res["plan"] == dict(want, bytes_per_sample=bps, halo_columns=W, halo_rows=H), res["plan"]
    assert res["batches"] == want["batches"]
    assert res["native"] == ["filter_combine_clip"] * (want["batches"] * want["passes"])
    flt, image = compiled("rotate")
    inv = invoke(flt, image)
    here = flt.clip_filtered_plan(W, H, W, H, 3, 2, "tent", n)
    assert here["batches"] == 1 and here["passes"] == 1      # this process has the default budget
    single = inv.render_clip(frames=list(range(n)), ts=[0.1 + 0.2 * i for i in range(n)], shutter_samples=3, shutter_span=SPAN, aa=2, aa_filter="tent")
    assert res["sha"] == hashlib.sha256(single.tobytes()).hexdigest()


# ---- 5. the kernel alone ----

def synthetic(frames, steps, sy, sx, h, w, seed):
    """Whole-frame maps [frames, steps, sy, sx, h, w, 4] of ordinary values with NaN, the infinities, -0 and denormals among them."""
    rng = np.random.default_rng(seed)
    maps = rng.uniform(-0.25, 1.25, (frames, steps, sy, sx, h, w, 4)).astype(f32)
    tiny = np.nextafter(f32(0), f32(1))
    flat = maps.reshape(-1, 4)
    for k, v in enumerate((np.nan, np.inf, -np.inf, -0.0, 0.0, tiny, -tiny, f32(1e-39), f32(5.877472e-39), f32(1.1754942e-38), f32(3e38), f32(-3e38))):
        where = rng.integers(0, flat.shape[0], 6)
        flat[where[:3]] = v                                # whole texels
        flat[where[3:], rng.integers(0, 4, 3)] = v         # single channels
    return maps


def run_kernel(maps, aa_filter, radius, rect=None, bpp=4, floatmap=False, steps_per_pass=0, row_pad=0, gap=0):
    """maps: whole-frame [frames, steps, sy, sx, h, w, 4].  The launcher gets the haloed rectangle of `rect` = (x, y, w, h)
    cut out of them -- the columns of a map's rows behind the rectangle's hold NaN: nothing may read them -- and the whole
    sentinel-filled output buffer comes back with its layout."""
    frames, steps, sy, sx, h, w, _ = maps.shape
    rx, ry, rw, rh = rect if rect is not None else (0, 0, w, h)
    big_d = X.reach(radius)
    x0, y0, x1, y1 = max(0, rx - big_d), max(0, ry - big_d), min(w, rx + rw + big_d), min(h, ry + rh + big_d)
    halo = np.full((frames, steps, sy, sx, y1 - y0, w, 4), np.nan, f32)
    halo[..., :x1 - x0, :] = maps[..., y0:y1, x0:x1, :]
    halo = np.ascontiguousarray(halo.reshape(frames, steps, sy * sx, y1 - y0, w, 4))
    lead = 0 if floatmap else 8 if bpp == 4 and row_pad == 0 else 5      # (bpp 4 once from an aligned start: the 32-bit stores)
    lay = Layout(frames, rw, rh, w, bpp=bpp, floatmap=floatmap, row_pad=row_pad, gap=gap, lead=lead, tail=9)
    out = np.empty(lay.total, np.uint8)
    rc = selftest_lib().mmhip_selftest_filter_combine(halo.ctypes.data_as(C.c_void_p), frames, steps, sx, sy, X.KERNELS[aa_filter], radius, w, h, rx, ry,
                                                      rw, rh, bpp, 1 if floatmap else 0, lay.stride or 0, lay.fstride, steps_per_pass, lay.lead,
                                                      out.ctypes.data_as(C.c_void_p), lay.total, SENTINEL, 0, None)
    assert rc == 0, selftest_lib().mmhip_selftest_error().decode()
    return out, lay


KERNEL_CASES = {
    # name: (frames, steps, sy, sx, h, w), filter, radius, rect, steps per pass
    "tent whole frame": ((2, 1, 2, 2, 13, 37), "tent", 1.0, None, 0),
    "mitchell rectangle": ((2, 2, 1, 3, 21, 45), "mitchell", 2.0, (3, 2, 35, 9), 0),
    "mitchell rectangle with a carry": ((1, 3, 2, 1, 21, 45), "mitchell", 2.0, (3, 2, 35, 9), 1),
    "corner rectangle": ((1, 1, 2, 2, 21, 45), "gaussian", 1.5, (0, 10, 25, 11), 0),
    "the most LDS": ((1, 1, 8, 1, 19, 35), "tent", 4.0, (1, 1, 33, 17), 0),      # D = 4 and sy = 8: 64 KiB
    "one sample per pixel": ((1, 2, 1, 1, 9, 33), "gaussian", 1.5, None, 1),
}


@pytest.mark.parametrize("case", list(KERNEL_CASES))
def test_the_kernel_alone_on_maps_with_special_values(case):
    shape, aa_filter, radius, rect, per_pass = KERNEL_CASES[case]
    maps = synthetic(*shape, seed=len(case))
    assert np.isnan(maps).any() and np.isinf(maps).any()
    rx, ry, rw, rh = rect if rect is not None else (0, 0, shape[5], shape[4])
    want_px = [X.frame(maps[i], X.KERNELS[aa_filter], radius)[ry:ry + rh, rx:rx + rw] for i in range(shape[0])]
    assert any(np.isnan(m).any() for m in want_px) and any((~np.isnan(m)).any() for m in want_px)
    for floatmap, bpp, row_pad, gap in ((True, 4, 0, 32), (False, 4, 0, 0), (False, 4, 3, 7), (False, 3, 5, 11), (False, 2, 0, 1), (False, 1, 7, 0)):
        got, lay = run_kernel(maps, aa_filter, radius, rect, bpp, floatmap, per_pass, row_pad, gap)
        want = lay.expected([m if floatmap else pack(m, bpp) for m in want_px])
        assert same_buffer(got, want, floatmap), (case, floatmap, bpp, row_pad, gap)


def test_one_tap_of_weight_one_stores_what_the_shutter_combine_stores():
    """The two kernels share one pixel store: the box at half a pixel over a 1 x 1 grid and one step is one tap of weight
    1.0f and inv_k 1, the shutter combine of one sample is the sample times 1, so the buffers are equal byte for byte --
    sentinels and the bits of a float map's NaNs included -- at every layout."""
    maps = synthetic(2, 1, 1, 1, 13, 37, seed=7)
    assert np.isnan(maps).any() and np.isinf(maps).any() and X.reach(0.5) == 0
    frames, h, w = 2, 13, 37
    samples = np.ascontiguousarray(maps.reshape(frames, 1, h, w, 4))
    for floatmap, bpp, row_pad, gap in ((True, 4, 0, 32), (False, 4, 0, 0), (False, 4, 3, 7), (False, 3, 5, 11), (False, 2, 0, 1), (False, 1, 7, 0)):
        filtered, lay = run_kernel(maps, "box", 0.5, None, bpp, floatmap, 0, row_pad, gap)
        assert lay.lead % 2 == (1 if not floatmap and (bpp != 4 or row_pad) else 0)      # bpp 4 once aligned, once from an odd offset
        combined = np.empty(lay.total, np.uint8)
        rc = selftest_lib().mmhip_selftest_shutter_combine(samples.ctypes.data_as(C.c_void_p), frames, 1, h, w, w, bpp, 1 if floatmap else 0,
                                                           lay.stride or 0, lay.fstride, 0, lay.lead, combined.ctypes.data_as(C.c_void_p),
                                                           lay.total, SENTINEL, 0, None)
        assert rc == 0, selftest_lib().mmhip_selftest_error().decode()
        assert (filtered != SENTINEL).any() and (filtered[:lay.lead] == SENTINEL).all() and (filtered[-9:] == SENTINEL).all()
        assert np.array_equal(filtered, combined), (floatmap, bpp, row_pad, gap)


# ---- 6. call hygiene ----

def test_the_callers_sampling_offset_is_put_back():
    flt, image = compiled("rotate")
    inv, fresh = invoke(flt, image), invoke(flt, image)
    fresh.set_sampling_offset(-0.5, 0.25)
    want = fresh.render(t=0.3, frame=1)
    assert not np.array_equal(want, invoke(flt, image).render(t=0.3, frame=1))
    inv.set_sampling_offset(-0.5, 0.25)
    got = inv.render_clip(frames=FRAMES, ts=TS, aa=(2, 3), aa_filter="tent")
    assert np.array_equal(inv.render(t=0.3, frame=1), want)
    # the call renders at the grid's offsets, whatever the caller's
    assert np.array_equal(got, invoke(flt, image).render_clip(frames=FRAMES, ts=TS, aa=(2, 3), aa_filter="tent"))


def test_refused_calls_leave_the_offset_and_say_why():
    flt, image = compiled("rotate")
    inv, fresh = invoke(flt, image), invoke(flt, image)
    for v in (inv, fresh):
        v.set_sampling_offset(0.25, -0.5)
    dev = device_filled(4096)
    try:
        for region, rows, word in (((-1, 0, 10, 10), None, "columns"), ((90, 0, 10, 10), None, "columns"), ((0, 55, 10, 10), None, "rows"),
                                   ((0, 55, 10, 10), (58, 62), "rows")):
            with pytest.raises(mm.MathMapError, match="render_clip_filtered: the (region's )?%s" % word):
                inv.render_clip(frames=FRAMES, ts=TS, out_ptr=dev, region=region, rows=rows, aa=2, aa_filter="tent", frame_stride=2048)
        assert (device_read(dev, 4096) == SENTINEL).all()
    finally:
        lib().mmhip_device_free(C.c_void_p(dev))
    assert inv.clip_filtered_batches() == 0
    assert np.array_equal(inv.render(t=0.3, frame=1), fresh.render(t=0.3, frame=1))
    # a nested clip that fails behind the first change of the offset (tests/test_gpu_clip_sampled.py has the same for aa alone)
    flt = mm.Filter(P.BLUR)
    seq = P.SEQ[:, :H, :W]
    inv, fresh = flt.invoke(W, H), flt.invoke(W, H)
    for v in (inv, fresh):
        v.set_image("in", seq)
        v.set_native_input_frame("current")
        v.set_sampling_offset(0.25, -0.5)
    with pytest.raises(mm.MathMapError, match="frame"):
        inv.render_clip(frames=[1, 7], ts=[0.2, 0.4], aa=2, aa_filter="tent")
    assert np.array_equal(inv.render(t=0.3, frame=1), fresh.render(t=0.3, frame=1))
    fresh.set_sampling_offset(0.0, 0.0)
    assert not np.array_equal(inv.render(t=0.3, frame=1), fresh.render(t=0.3, frame=1))


def test_counters_and_timing_labels():
    flt, image = compiled("rotate")
    inv = invoke(flt, image)
    inv.enable_timing(True)
    lay = Layout(len(FRAMES), W, H, W)
    render(inv, lay, (2, 3), "mitchell", samples=2, span=SPAN)
    assert inv.clip_filtered_batches() == 1
    assert inv.clip_sampled_batches() == 0 and inv.clip_sampled_fused_batches() == 0 and inv.clip_adaptive_batches() == 0
    assert inv.clip_shutter_batches() == 0 and inv.clip_shutter_fused_batches() == 0
    assert inv.clip_batched_launches() == 6                   # one nested clip per grid point, N * K entries each
    assert [name for name, ms in inv.drain_native_kernel_ms()] == ["filter_combine_clip"]
    assert len(inv.drain_kernel_ms()) == 6


def test_plain_aa_and_adaptive_clips_around_a_filtered_clip():
    flt, image = compiled("rotate")
    inv = invoke(flt, image)

    def others():
        return (inv.render_clip(frames=FRAMES, ts=TS), inv.render_clip(frames=FRAMES, ts=TS, aa=2),
                inv.render_clip(frames=FRAMES, ts=TS, aa=2, aa_threshold=0.05))
    before = others()
    filtered = inv.render_clip(frames=FRAMES, ts=TS, aa=2, aa_filter="mitchell")
    for b in before:
        assert not np.array_equal(filtered, b)
    for a, b in zip(others(), before):
        assert np.array_equal(a, b)
    assert np.array_equal(inv.render_clip(frames=FRAMES, ts=TS, aa=2, aa_filter="mitchell"), filtered)
    assert np.array_equal(inv.render_clip(frames=FRAMES, ts=TS, aa=2, aa_filter=None), before[1])


def test_cli_writes_the_python_result(tmp_path):
    src = "filter swirl (float k: 0-8 (3)) rgba:[0.5 + 0.5 * sin(k * r + t * 6), 0.5 + 0.5 * cos(a * 5 + t * 3), frame / 6, 1] end"
    want = mm.Filter(src).invoke(W, H).render_clip(num_frames=3, aa=2, aa_filter="mitchell")
    assert not np.array_equal(want, mm.Filter(src).invoke(W, H).render_clip(num_frames=3, aa=2))
    p = subprocess.run([CLI, "-F", "3", "--aa=2", "--aa-filter=mitchell", "--batch-frames=2", "-s", "%dx%d" % (W, H), src, str(tmp_path / "m%d.png")],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert p.returncode == 0, p.stderr
    for i in range(3):
        assert np.array_equal(read_png(str(tmp_path / ("m%d.png" % i))), want[i, :, :, :3]), i
    # a radius behind the colon, a 1 x 1 grid and a shutter
    want = mm.Filter(src).invoke(W, H).render_clip(num_frames=3, aa=1, aa_filter="gaussian", aa_radius=2.5, shutter_samples=2, shutter=0.5)
    p = subprocess.run([CLI, "-F", "3", "--aa=1", "--aa-filter=gaussian:2.5", "--shutter-samples=2", "--shutter=0.5", "-s", "%dx%d" % (W, H), src,
                        str(tmp_path / "g%d.png")], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert p.returncode == 0, p.stderr
    for i in range(3):
        assert np.array_equal(read_png(str(tmp_path / ("g%d.png" % i))), want[i, :, :, :3]), i
