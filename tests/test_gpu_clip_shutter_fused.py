"""Fused motion blur on the GPU (mmhip_render_clip_shutter_fused, mm_pixels_shutter).

Two yardsticks.  tests/shutter_reference.py: the sub-samples are single render_rows(floatmap=True) calls of a *second*
invocation at the restated times, summed and packed in NumPy.  And render_clip(shutter_mode="maps"), the path through
sub-sample maps, whose bytes the fused call promises.  Outputs go into sentinel-filled buffers that are compared whole:
float maps by NaN position and bit pattern, bytes as they are."""
import ctypes as C
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import mathmap_amd as mm
from mathmap_amd._lib import lib
from tests import shutter_fused_probes as P
from tests import shutter_reference as R
from tests.test_gpu_clip_shutter import SENTINEL, device_filled, device_read, read_png, same_buffer, sub_sample_maps

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "mathmap_amd", "mathmap_hip_cli")
f32 = np.float32
W, H, N, K, SPAN = P.W, P.H, 3, 4, 0.07
FRAMES = [2, 0, 1]
TS = [0.9, 0.1, 0.5]
LEAD, TAIL = 64, 64

_filters = {}


def probe(name):
    """(filter, image) of a probe, compiled once per session: its modules are built once."""
    if name not in _filters:
        _filters[name] = P.compiled(name)
    return _filters[name]


def layout(inv, n, region=None, rows=None, bpp=4, floatmap=False, row_pad=0, frame_gap=0):
    """row_stride (None for float maps), the distance between rows, the bytes of a row, frame_stride and the buffer's size."""
    rx, ry, rw, rh = region if region is not None else (0, 0, inv.render_width, inv.render_height)
    first, last = rows if rows is not None else (ry, ry + rh)
    nrows = last - first
    if floatmap:
        stride, row_step, row_bytes = None, 16 * inv.render_width, 16 * rw
        band = nrows * row_step
    else:
        stride = row_step = rw * bpp + row_pad
        row_bytes = rw * bpp
        band = (nrows - 1) * stride + row_bytes
    fstride = nrows * row_step + frame_gap
    return stride, row_step, row_bytes, nrows, fstride, LEAD + (n - 1) * fstride + band + TAIL


def render_buffer(inv, mode, k, span, frames=FRAMES, ts=TS, region=None, rows=None, bpp=4, floatmap=False, row_pad=0, frame_gap=0):
    """The whole sentinel-filled buffer around the frames of one render_clip call."""
    stride, _, _, _, fstride, total = layout(inv, len(frames), region, rows, bpp, floatmap, row_pad, frame_gap)
    dev = device_filled(total)
    try:
        assert inv.render_clip(frames=frames, ts=ts, out_ptr=dev + LEAD, rows=rows, region=region, row_stride=stride, frame_stride=fstride,
                               bpp=bpp, floatmap=floatmap, shutter_samples=k, shutter_span=span, shutter_mode=mode) is None
        inv.sync()
        return device_read(dev, total)
    finally:
        lib().mmhip_device_free(C.c_void_p(dev))


def restated_buffer(other, k, span, frames=FRAMES, ts=TS, bpp=4, floatmap=False):
    _, row_step, row_bytes, nrows, fstride, total = layout(other, len(frames), None, None, bpp, floatmap)
    subs = sub_sample_maps(other, frames, ts, k, span)
    want = np.full(total, SENTINEL, np.uint8)
    for i in range(len(frames)):
        px = R.combine(subs[i], bpp=bpp, floatmap=floatmap)
        for r in range(nrows):
            at = LEAD + i * fstride + r * row_step
            want[at:at + row_bytes] = np.ascontiguousarray(px[r]).view(np.uint8).reshape(-1)
    return want, subs


# ---- 1. against the NumPy restatement ----

@pytest.mark.parametrize("name", list(P.PROBES))
def test_fused_frames_equal_the_restatement(name):
    flt, image = probe(name)
    inv, other = P.invoke(flt, image), P.invoke(flt, image)
    for floatmap in (True, False):
        want, subs = restated_buffer(other, K, SPAN, floatmap=floatmap)
        got = render_buffer(inv, "fused", K, SPAN, floatmap=floatmap)
        assert same_buffer(got, want, floatmap), (name, floatmap)
    if name not in ("droste", "mandelbrot"):           # (the reference's two examples do not read t)
        assert not R.same_floats(subs[:, 0], subs[:, K - 1]), (name, "the sub-samples do not differ: nothing is blurred")
    assert inv.clip_shutter_fused_batches() == 2 and inv.clip_shutter_batches() == 0 and other.clip_shutter_fused_batches() == 0
    if name == "extreme":
        m = np.stack([R.combine(subs[i], floatmap=True) for i in range(N)])
        assert np.isnan(m).any() and np.isposinf(m).any() and np.isneginf(m).any() and (m[np.isfinite(m)] < 0).any() and (m[np.isfinite(m)] > 1).any()


# ---- 2. against the path through sub-sample maps ----

CONFIGS = [
    dict(size=(1, 1), k=2), dict(size=(16, 16), k=2), dict(size=(17, 17), k=2), dict(size=(17, 17), k=256),
    dict(k=2), dict(k=3), dict(k=8), dict(k=3, span=0.0), dict(k=3, span=-0.05),
    dict(k=2, bpp=1), dict(k=3, bpp=2), dict(k=2, bpp=3), dict(k=3, floatmap=True),
    dict(k=3, rows=(5, 23)), dict(k=3, rows=(5, 23), floatmap=True),
    dict(k=2, region=(11, 7, 70, 41)), dict(k=2, region=(11, 7, 70, 41), rows=(13, 40), floatmap=True),
    dict(k=2, bpp=3, row_pad=13, frame_gap=101), dict(k=2, bpp=4, row_pad=8, frame_gap=4), dict(k=2, floatmap=True, frame_gap=80),
    dict(k=2, region=(11, 7, 70, 41), bpp=2, row_pad=5, frame_gap=3),
]


@pytest.mark.parametrize("name", list(P.PROBES))
def test_fused_bytes_equal_the_maps_path(name):
    flt, image = probe(name)
    pairs = {}
    for cfg in CONFIGS:
        cfg = dict(cfg)
        size = cfg.pop("size", (W, H))
        if size not in pairs:
            pairs[size] = (P.invoke(flt, image, *size), P.invoke(flt, image, *size))
        fused_inv, maps_inv = pairs[size]
        k, span = cfg.pop("k"), cfg.pop("span", SPAN)
        before = fused_inv.clip_shutter_fused_batches()
        got = render_buffer(fused_inv, "fused", k, span, **cfg)
        want = render_buffer(maps_inv, "maps", k, span, **cfg)
        assert same_buffer(got, want, cfg.get("floatmap", False)), (name, size, k, span, cfg)
        assert (got[:LEAD] == SENTINEL).all() and (got[-TAIL:] == SENTINEL).all()
        assert fused_inv.clip_shutter_fused_batches() == before + 1
        if cfg.get("frame_gap"):
            _, row_step, _, nrows, fstride, _ = layout(fused_inv, N, cfg.get("region"), cfg.get("rows"), cfg.get("bpp", 4), cfg.get("floatmap", False),
                                                       cfg.get("row_pad", 0), cfg["frame_gap"])
            for i in range(N - 1):
                gap = got[LEAD + i * fstride + nrows * row_step:LEAD + (i + 1) * fstride]
                assert gap.size == cfg["frame_gap"] and (gap == SENTINEL).all(), (name, cfg, i)
    for fused_inv, maps_inv in pairs.values():
        assert fused_inv.clip_shutter_batches() == 0 and maps_inv.clip_shutter_fused_batches() == 0 and maps_inv.clip_shutter_batches() > 0


# ---- 3. counters and timing ----

@pytest.mark.parametrize("name", list(P.PROBES))
def test_counters(name):
    flt, image = probe(name)
    inv = P.invoke(flt, image)
    plan = mm.Filter.clip_shutter_fused_plan(flt.specialized() if P.PROBES[name][1].get("specialize") else flt, W, H, K, N)
    assert plan["fused"] == 1 and plan["batches"] == 1
    assert (plan["slots_per_batch"] == 1) == (name in ("shared", "mandelbrot"))
    inv.enable_timing(True)
    assert inv.drain_kernel_ms() == []
    before = (inv.clip_shutter_batches(), inv.clip_batched_launches(), inv.clip_native_batches(), inv.clip_prologue_frames())
    render_buffer(inv, "fused", K, SPAN)
    assert inv.clip_shutter_fused_batches() == 1
    assert (inv.clip_shutter_batches(), inv.clip_batched_launches(), inv.clip_native_batches()) == before[:3]
    assert inv.clip_prologue_frames() - before[3] == (1 if plan["slots_per_batch"] == 1 else N * K)
    ms = inv.drain_kernel_ms()
    assert len(ms) == 1 and ms[0] > 0
    assert inv.drain_native_kernel_ms() == []              # no combine kernel
    # one sub-sample per frame is the plain clip: the call delegates
    render_buffer(inv, "fused", 1, SPAN)
    assert inv.clip_shutter_fused_batches() == 1 and inv.clip_batched_launches() == before[1] + 1


# ---- 4. several batches (the cap is read once: a child process) ----

CHILD = r"""
import hashlib, json, sys
sys.path.insert(0, %r)
from tests import shutter_fused_probes as P
from tests.test_gpu_clip_shutter_fused import render_buffer
name = sys.argv[1]
flt, image = P.compiled(name)
inv = P.invoke(flt, image)
inv.enable_timing(True)
frames, ts = [0, 2, 1, 0, 2], [0.1, 0.3, 0.5, 0.7, 0.9]
out = {}
for what, extra in (("bytes", dict(bpp=3, row_pad=5, frame_gap=7)), ("floats", dict(floatmap=True, frame_gap=16))):
    out[what] = hashlib.sha256(render_buffer(inv, "fused", 3, 0.07, frames=frames, ts=ts, **extra).tobytes()).hexdigest()
print(json.dumps(dict(out, plan=flt.clip_shutter_fused_plan(P.W, P.H, 3, 5), batches=inv.clip_shutter_fused_batches(),
                      prologue=inv.clip_prologue_frames(), ms=len(inv.drain_kernel_ms()), maps=inv.clip_shutter_batches())))
"""


@pytest.mark.parametrize("name", ["wave", "shared"])
def test_several_batches_leave_the_bytes_alone(name):
    env = dict(os.environ, MMHIP_CLIP_MAX_FRAMES="8")
    r = subprocess.run([sys.executable, "-c", CHILD % ROOT, name], cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    res = json.loads(r.stdout.strip().splitlines()[-1])
    shared = name == "shared"
    assert res["plan"] == dict(fused=1, frames_per_batch=2, batches=3, slots_per_batch=1 if shared else 6, grid_x=res["plan"]["grid_x"])
    assert res["batches"] == 6 and res["ms"] == 6 and res["maps"] == 0            # two calls of three batches
    assert res["prologue"] == (2 if shared else 2 * 15)
    # this process has no cap: one batch
    flt, image = probe(name)
    assert flt.clip_shutter_fused_plan(W, H, 3, 5)["batches"] == 1
    inv = P.invoke(flt, image)
    frames, ts = [0, 2, 1, 0, 2], [0.1, 0.3, 0.5, 0.7, 0.9]
    for what, extra in (("bytes", dict(bpp=3, row_pad=5, frame_gap=7)), ("floats", dict(floatmap=True, frame_gap=16))):
        here = render_buffer(inv, "fused", 3, 0.07, frames=frames, ts=ts, **extra)
        assert hashlib.sha256(here.tobytes()).hexdigest() == res[what], (name, what)
    assert inv.clip_shutter_fused_batches() == 2


# ---- 5. filters that are not fused ----

@pytest.mark.parametrize("name", list(P.FALLBACKS))
def test_native_calls_and_closures_take_the_maps_path(name):
    flt, image = P.compiled(name)
    inv, other = P.invoke(flt, image), P.invoke(flt, image)
    for floatmap in (False, True):
        got = render_buffer(inv, "fused", K, SPAN, floatmap=floatmap)
        want = render_buffer(other, "maps", K, SPAN, floatmap=floatmap)
        assert same_buffer(got, want, floatmap), (name, floatmap)
    assert inv.clip_shutter_fused_batches() == 0 and inv.clip_shutter_batches() == 2 == other.clip_shutter_batches()


# ---- 6. state ----

@pytest.mark.parametrize("name", ["wave", "pair", "sequence"])
def test_an_invocation_goes_from_one_path_to_the_other(name):
    flt, image = probe(name)
    inv = P.invoke(flt, image)
    fresh = [P.invoke(flt, image) for _ in range(3)]
    fused = render_buffer(inv, "fused", K, SPAN)
    plain = inv.render(t=0.3, frame=1)
    maps = render_buffer(inv, "maps", K, SPAN)
    again = render_buffer(inv, "fused", K, SPAN, frames=[1, 2, 0], ts=[0.2, 0.6, 0.4])
    assert np.array_equal(fused, maps)
    assert np.array_equal(fused, render_buffer(fresh[0], "fused", K, SPAN))
    assert np.array_equal(plain, fresh[1].render(t=0.3, frame=1))
    assert np.array_equal(again, render_buffer(fresh[2], "fused", K, SPAN, frames=[1, 2, 0], ts=[0.2, 0.6, 0.4]))
    assert not np.array_equal(again, fused)
    assert np.array_equal(inv.render(t=0.3, frame=1), plain)


# ---- 7. a frame whose float map is beyond 4 GiB ----

def test_a_frame_beyond_4_gib_of_float_map():
    w, h, k = 16384, 16385, 2
    flt = mm.Filter(P.CHEAP)
    inv = flt.invoke(w, h)
    assert h * 16 * w > 1 << 32
    assert flt.clip_shutter_fused_plan(w, h, k, 1)["fused"] == 1
    frame_bytes = w * 4 * h
    dev = lib().mmhip_device_alloc(frame_bytes)
    assert dev
    band_dev = lib().mmhip_device_alloc(4 * w * 4)
    assert band_dev
    try:
        with pytest.raises(mm.MathMapError, match="4 GiB"):
            inv.render_clip(frames=[0], ts=[0.25], out_ptr=dev, shutter_samples=k, shutter_span=0.1, shutter_mode="maps")
        assert inv.clip_shutter_batches() == 0
        inv.render_clip(frames=[0], ts=[0.25], out_ptr=dev, shutter_samples=k, shutter_span=0.1, shutter_mode="fused")
        inv.sync()
        assert inv.clip_shutter_fused_batches() == 1
        seen = []
        for first in (0, h // 2, h - 4):                 # the host never holds the frame
            got = np.empty(4 * w * 4, np.uint8)
            assert lib().mmhip_copy_to_host(got.ctypes.data_as(C.c_void_p), C.c_void_p(dev + first * w * 4), got.size) == 0
            inv.render_clip(frames=[0], ts=[0.25], out_ptr=band_dev, rows=(first, first + 4), shutter_samples=k, shutter_span=0.1, shutter_mode="maps")
            inv.sync()
            want = device_read(band_dev, got.size)
            assert np.array_equal(got, want), first
            seen.append(got)
        assert not np.array_equal(seen[0], seen[2])
    finally:
        lib().mmhip_device_free(C.c_void_p(band_dev))
        lib().mmhip_device_free(C.c_void_p(dev))


# ---- 8. the command line ----

def test_cli_fused_files_are_the_maps_files(tmp_path):
    base = [CLI, "-F", "3", "--shutter-samples=4", "--shutter=0.5", "-s", "%dx%d" % (W, H)]
    for tag, extra in (("maps", []), ("fused", ["--shutter-mode=fused"]), ("named", ["--shutter-mode=maps"]),
                       ("batched", ["--shutter-mode=fused", "--batch-frames=2"])):
        p = subprocess.run(base + extra + [P.PAIR, str(tmp_path / (tag + "%d.png"))], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                           timeout=300)
        assert p.returncode == 0, p.stderr
    want = mm.Filter(P.PAIR).invoke(W, H).render_clip(num_frames=3, shutter_samples=4, shutter=0.5, shutter_mode="fused")
    for i in range(3):
        maps = open(str(tmp_path / ("maps%d.png" % i)), "rb").read()
        for tag in ("fused", "named", "batched"):
            assert open(str(tmp_path / ("%s%d.png" % (tag, i))), "rb").read() == maps, (tag, i)
        assert np.array_equal(read_png(str(tmp_path / ("fused%d.png" % i))), want[i, :, :, :3]), i
    assert not np.array_equal(want[0], want[1])
