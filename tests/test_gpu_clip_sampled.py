"""Grid-supersampled clips on the GPU (mmhip_render_clip_sampled through sub-sample maps, mmhip_render_clip_sampled_fused in
the registers of mm_pixels_sampled).

The yardstick is tests/sample_grid_reference.py: the sub-samples are single render_rows(floatmap=True) calls of a *second*
invocation at set_sampling_offset(ox_a, oy_b) and the restated times, summed in NumPy in the order s = j * G + b * sx + a.
Everything is compared bit for bit, in whole sentinel-filled buffers: float maps by NaN position and bit pattern, bytes
as they are."""
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
from tests import clip_probes
from tests import filters as F
from tests import sample_grid_reference as G
from tests import shutter_fused_probes as P
from tests import shutter_reference as R
from tests.test_gpu_clip_shutter import ROTATE, SENTINEL, device_filled, device_read, read_png, same_buffer

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "mathmap_amd", "mathmap_hip_cli")
f32 = np.float32
W, H, N, SPAN = P.W, P.H, 3, 0.07
FRAMES = [2, 0, 1]
TS = [0.9, 0.1, 0.5]
MODES = ("maps", "fused")

# RAND's call counter starts again in every sub-sample; the pixel reads x and y, so that every grid point differs
RANDOM = """filter noisy_xy ()
  p = rand(0, 1);
  q = rand(0, 1) * t;
  rgba:[p + y * 0.25, q, rand(-1, 1) * x + t, 1]
end
"""

# Native results and closure images are float maps, which are sampled at the nearest texel: at the pixels' own centres every
# offset inside the footprint reads the same one.  These two sample them at 0.8 of the coordinates, where grid points differ.
BLUR = """stretched filter blur_t (stretched image in)
  b = gaussian_blur(in, 0.04 + t * 0.05, 0.05);
  b(xy * 0.8)
end
"""
CLOSURE = """
filter inner2 (image in, float k: 0-2 (1.0))
  in(xy * k) * 0.8 + rgba:[t * 0.5, frame * 0.01, 0.1, 0]
end

filter outer (image in, float s: 0-1 (0.03), float k: 0-2 (0.5))
  b = gaussian_blur(inner2(in, k * (1 + t)), s, s);
  b(xy * 0.8)
end
"""

# name -> (text or fixture name, Filter options, frames of `in`, has a fused variant)
PROBES = {
    "rotate": (ROTATE, {}, None, True),                      # the rotating bilinear fetch
    "pair": (P.PAIR, {}, None, True),                        # the pair-mode escape loop
    "pond": ("pond", {}, None, True),
    "wave": (clip_probes.WAVE, {}, None, False),             # a per-row slice: the maps path under either mode
    "sequence": (P.SEQUENCE, {}, P.SEQ, True),               # in(xy, frame) on a 3-frame sequence
    "rand": (RANDOM, {}, None, True),
    "extreme": (P.EXTREME, {}, None, False),                 # (its exp(.. y ..) is a per-row slice too)
    "blur": (BLUR, {}, None, False),                         # gaussian_blur with sigma following t
    "closure": (CLOSURE, {}, None, False),
}
MAPS_ONLY = ("blur", "closure")


def compiled(name):
    src, opts, image, _ = PROBES[name]
    return (F.load(src, **opts) if src in F.NAMES else mm.Filter(src, **opts)), image


def invoke(flt, image, w=W, h=H):
    return P.invoke(flt, image, w, h)


def sub_sample_maps(inv, frames, ts, samples, span, aa, region=None, rows=None):
    """float32 [N, K, sy, sx, rows, region_w, 4]: every sub-sample one render_rows(floatmap=True) at its offset and time."""
    sx, sy = G.grid(aa)
    ox, oy = G.offsets(sx), G.offsets(sy)
    rx, ry, rw, rh = region if region is not None else (0, 0, inv.render_width, inv.render_height)
    first, last = rows if rows is not None else (ry, ry + rh)
    times = R.sample_ts(ts, samples, span)
    size = (last - first) * 16 * inv.render_width
    out = np.empty((len(frames), samples, sy, sx, last - first, rw, 4), f32)
    dev = lib().mmhip_device_alloc(size)
    assert dev
    try:
        for b in range(sy):
            for a in range(sx):
                inv.set_sampling_offset(float(ox[a]), float(oy[b]))
                for i, frame in enumerate(frames):
                    for j in range(samples):
                        inv.render_rows(dev, first, last, t=float(times[i, j]), frame=int(frame), floatmap=True, region=(rx, ry, rw, rh))
                        inv.sync()
                        out[i, j, b, a] = device_read(dev, size).view(f32).reshape(last - first, inv.render_width, 4)[:, :rw]
    finally:
        lib().mmhip_device_free(C.c_void_p(dev))
        inv.set_sampling_offset(0.0, 0.0)
    return out


class Layout:
    """Where the frames of a call land in a sentinel-filled buffer: rows padded by `row_pad` bytes, `gap` bytes between frames."""

    def __init__(self, n, rw, nrows, render_w, bpp=4, floatmap=False, row_pad=0, gap=0, lead=64, tail=64):
        self.n, self.rw, self.nrows, self.bpp, self.floatmap, self.lead = n, rw, nrows, bpp, floatmap, lead
        if floatmap:
            self.stride, self.row_step, self.row_bytes = None, 16 * render_w, rw * 16
        else:
            self.stride = self.row_step = rw * bpp + row_pad
            self.row_bytes = rw * bpp
        self.fstride = nrows * self.row_step + gap
        self.total = lead + n * self.fstride + tail

    def expected(self, frames_px):
        want = np.full(self.total, SENTINEL, np.uint8)
        for i, px in enumerate(frames_px):
            for r in range(self.nrows):
                at = self.lead + i * self.fstride + r * self.row_step
                want[at:at + self.row_bytes] = np.ascontiguousarray(px[r]).view(np.uint8).reshape(-1)
        return want


def render(inv, lay, mode, aa, samples=1, span=None, frames=FRAMES, ts=TS, region=None, rows=None):
    dev = device_filled(lay.total)
    try:
        assert inv.render_clip(frames=frames, ts=ts, out_ptr=dev + lay.lead, rows=rows, region=region, row_stride=lay.stride,
                               frame_stride=lay.fstride, bpp=lay.bpp, floatmap=lay.floatmap, shutter_samples=samples,
                               shutter_span=span, shutter_mode=mode, aa=aa) is None
        inv.sync()
        return device_read(dev, lay.total)
    finally:
        lib().mmhip_device_free(C.c_void_p(dev))


# ---- 1. against the restatement ----

CONFIGS = {"aa2": (2, 1), "aa3x1": ((3, 1), 1), "aa1x3": ((1, 3), 1), "aa2_k3": (2, 3)}


@pytest.mark.parametrize("config", list(CONFIGS))
@pytest.mark.parametrize("name", list(PROBES))
def test_frames_equal_the_restatement(name, config):
    aa, k = CONFIGS[config]
    sx, sy = G.grid(aa)
    flt, image = compiled(name)
    other = invoke(flt, image)
    subs = sub_sample_maps(other, FRAMES, TS, k, SPAN, aa)
    for i in range(N):                 # something is anti-aliased
        if sx > 1:
            assert not R.same_floats(subs[i, 0, 0, 0], subs[i, 0, 0, sx - 1]), (name, i, "sub-samples of different a are equal")
        if sy > 1:
            assert not R.same_floats(subs[i, 0, 0, 0], subs[i, 0, sy - 1, 0]), (name, i, "sub-samples of different b are equal")
    for mode in MODES[:1] if name in MAPS_ONLY else MODES:
        inv = invoke(flt, image)
        for floatmap in (True, False):
            lay = Layout(N, W, H, W, floatmap=floatmap, gap=80)
            got = render(inv, lay, mode, aa, k, SPAN)
            want = lay.expected([G.combine(subs[i], bpp=4, floatmap=floatmap) for i in range(N)])
            assert same_buffer(got, want, floatmap), (name, config, mode, "floatmap" if floatmap else "bytes")
        fused = mode == "fused" and PROBES[name][3]
        assert inv.clip_sampled_fused_batches() == (2 if fused else 0), (name, mode)
        assert inv.clip_sampled_batches() == (0 if fused else 2), (name, mode)
        assert inv.clip_shutter_batches() == 0 and inv.clip_shutter_fused_batches() == 0


# ---- 2. coverage pinned without the GPU's help ----

V_EDGE = "stretched filter v_edge () if x < 0.1 then rgba:[1, 1, 1, 1] else rgba:[0, 0, 0, 1] end end"
H_EDGE = "stretched filter h_edge () if y < 0.1 then rgba:[1, 1, 1, 1] else rgba:[0, 0, 0, 1] end end"


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("which", ["vertical", "horizontal"])
def test_a_hard_edge_has_the_coverage_worked_out_in_numpy(which, mode):
    n = 16
    pos = np.arange(n, dtype=np.float64)
    o = G.offsets(4).astype(np.float64)
    if which == "vertical":
        src, aa = V_EDGE, (4, 1)
        coord = ((pos[None, :] - 7.5 + o[:, None]) / 7.5).astype(f32)          # x_a of column col: [4, 16]
    else:
        src, aa = H_EDGE, (1, 4)
        coord = ((-pos[None, :] + 7.5 - o[:, None]) / 7.5).astype(f32)         # y_b of row
    inside = (coord < f32(0.1)).astype(f32)                                       # [4, 16]
    line = R.mean(inside[:, :, None].repeat(4, axis=2))[:, 0]                     # the mean of the indicator, in the sum's order
    if which == "vertical":
        assert line[8] == f32(0.75) and line[7] == 1 and line[9] == 0
        grey = np.broadcast_to(line[None, :], (n, n))
    else:
        grey = np.broadcast_to(line[:, None], (n, n))
    want_px = np.stack([grey, grey, grey, np.ones((n, n), f32)], axis=2).astype(f32)
    inv = mm.Filter(src).invoke(n, n)
    lay = Layout(1, n, n, n, floatmap=True)
    got = render(inv, lay, mode, aa, frames=[0], ts=[0.0])
    assert same_buffer(got, lay.expected([want_px]), True), (which, mode)
    assert (inv.clip_sampled_fused_batches(), inv.clip_sampled_batches()) == ((1, 0) if mode == "fused" else (0, 1))


# ---- 3. fused against maps, on the shapes where the kernel can go wrong ----

def both_modes(flt, image, w, h, lay_args, aa, samples=1, span=None, frames=(1, 0), ts=(0.3, 0.8), region=None, rows=None):
    rx, ry, rw, rh = region if region is not None else (0, 0, w, h)
    first, last = rows if rows is not None else (ry, ry + rh)
    out = {}
    for mode in MODES:
        inv = invoke(flt, image, w, h)
        lay = Layout(len(frames), rw, last - first, w, **lay_args)
        out[mode] = render(inv, lay, mode, aa, samples, span, list(frames), list(ts), region, rows)
        assert (inv.clip_sampled_fused_batches() > 0) == (mode == "fused"), mode
        assert (inv.clip_sampled_batches() > 0) == (mode == "maps"), mode
    assert np.count_nonzero(out["maps"] != SENTINEL) > 0
    return out


@pytest.mark.parametrize("aa", [2, 3, (2, 1), (1, 8), (8, 8)], ids=str)
@pytest.mark.parametrize("size", [(1, 1), (16, 16), (17, 17), (97, 61)], ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("name", ["rotate", "pair"])
def test_fused_equals_maps_at_every_size_and_grid(name, size, aa):
    flt, image = compiled(name)
    w, h = size
    for floatmap in (True, False):
        out = both_modes(flt, image, w, h, dict(floatmap=floatmap, gap=48), aa)
        assert same_buffer(out["fused"], out["maps"], floatmap), (name, size, aa, floatmap)


@pytest.mark.parametrize("span", [0.0, -0.05])
@pytest.mark.parametrize("case", ["aa4x4_k16", "aa2_k3"])
def test_fused_equals_maps_with_a_shutter(case, span):
    """(4, 4) with K = 16 is K * G = 256, the most a call takes."""
    aa, k, (w, h) = {"aa4x4_k16": ((4, 4), 16, (17, 17)), "aa2_k3": (2, 3, (97, 61))}[case]
    flt, image = compiled("rotate")
    for floatmap in (True, False):
        out = both_modes(flt, image, w, h, dict(floatmap=floatmap), aa, k, span)
        assert same_buffer(out["fused"], out["maps"], floatmap), (case, span, floatmap)


@pytest.mark.parametrize("bpp", [1, 2, 3, 4])
def test_fused_equals_maps_at_every_format_with_padded_rows_and_frame_gaps(bpp):
    flt, image = compiled("rotate")
    out = both_modes(flt, image, W, H, dict(bpp=bpp, row_pad=13, gap=101, lead=61 + bpp), (2, 3), 2, SPAN)
    assert np.array_equal(out["fused"], out["maps"]), bpp
    # gaps and sentinels untouched, in both: the bytes between the rows of frame 0
    lay = Layout(2, W, H, W, bpp=bpp, row_pad=13, gap=101, lead=61 + bpp)
    for buf in out.values():
        assert (buf[:lay.lead] == SENTINEL).all() and (buf[lay.lead + W * bpp:lay.lead + lay.stride] == SENTINEL).all()
        assert (buf[lay.lead + H * lay.stride:lay.lead + lay.fstride] == SENTINEL).all()


@pytest.mark.parametrize("case", ["band", "region", "region and band"])
def test_fused_equals_maps_on_bands_and_regions(case):
    region, rows = {"band": (None, (5, 23)), "region": ((11, 7, 70, 41), None), "region and band": ((11, 7, 70, 41), (13, 40))}[case]
    flt, image = compiled("rotate")
    other = invoke(flt, image)
    subs = sub_sample_maps(other, [1, 0], [0.3, 0.8], 2, SPAN, (3, 2), region=region, rows=rows)
    for floatmap, lay_args in ((True, dict(floatmap=True, gap=32)), (False, dict(bpp=3, row_pad=5, gap=7))):
        out = both_modes(flt, image, W, H, lay_args, (3, 2), 2, SPAN, region=region, rows=rows)
        assert same_buffer(out["fused"], out["maps"], floatmap), (case, floatmap)
        lay = Layout(2, subs.shape[5], subs.shape[4], W, **lay_args)
        want = lay.expected([G.combine(subs[i], bpp=lay.bpp, floatmap=floatmap) for i in range(2)])
        assert same_buffer(out["maps"], want, floatmap), (case, floatmap)


# ---- 4. counters, labels, batches ----

def test_counters_and_timing_labels():
    flt, image = compiled("rotate")
    inv = invoke(flt, image)
    inv.enable_timing(True)
    lay = Layout(N, W, H, W)
    render(inv, lay, "maps", (2, 3), 2, SPAN)
    assert inv.clip_sampled_batches() == 1 and inv.clip_sampled_fused_batches() == 0
    assert inv.clip_shutter_batches() == 0 and inv.clip_shutter_fused_batches() == 0
    assert inv.clip_batched_launches() == 6                   # one nested clip per grid point, N * K entries each
    assert [name for name, ms in inv.drain_native_kernel_ms()] == ["shutter_combine_clip"]
    assert len(inv.drain_kernel_ms()) == 6
    prologues = inv.clip_prologue_frames()
    render(inv, lay, "fused", (2, 3), 2, SPAN)
    assert inv.clip_sampled_batches() == 1 and inv.clip_sampled_fused_batches() == 1
    assert inv.clip_shutter_batches() == 0 and inv.clip_shutter_fused_batches() == 0 and inv.clip_batched_launches() == 6
    assert inv.clip_prologue_frames() == prologues + N * 2    # a slot per frame and time step, not per grid point
    assert inv.drain_native_kernel_ms() == [] and len(inv.drain_kernel_ms()) == 1


CHILD = r"""
import hashlib, json, sys
sys.path.insert(0, %r)
from tests.test_gpu_clip_sampled import compiled, invoke, W, H, SPAN
n, k, sx, sy = (int(v) for v in sys.argv[1:5])
flt, image = compiled("rotate")
inv = invoke(flt, image)
inv.enable_timing(True)
frames, ts = list(range(n)), [0.1 + 0.2 * i for i in range(n)]
out = inv.render_clip(frames=frames, ts=ts, shutter_samples=k, shutter_span=SPAN, aa=(sx, sy))
print(json.dumps({"plan": flt.clip_sampled_plan(W, H, W, k, (sx, sy), n), "batches": inv.clip_sampled_batches(),
                  "native": [name for name, ms in inv.drain_native_kernel_ms()], "sha": hashlib.sha256(out.tobytes()).hexdigest()}))
"""


@pytest.mark.parametrize("case", ["three batches", "carry"])
def test_batches_and_passes_leave_the_bytes_alone(case):
    bps = H * 16 * W
    if case == "three batches":          # a frame is 2 * 4 maps, two fit: 5 frames are 2 + 2 + 1
        n, k, aa, budget, want = 5, 2, (2, 2), 16 * bps + 100, dict(frames_per_batch=2, batches=3, steps_per_pass=2, passes=1, carry=0)
    else:                                # 5 maps: (5 - 1) / 2 = 2 time steps per pass beside the carry, 5 are 2 + 2 + 1
        n, k, aa, budget, want = 1, 5, (2, 1), 5 * bps, dict(frames_per_batch=1, batches=1, steps_per_pass=2, passes=3, carry=1)
    env = dict(os.environ, MMHIP_CLIP_SHUTTER_BYTES=str(budget))
    r = subprocess.run([sys.executable, "-c", CHILD % ROOT, str(n), str(k), str(aa[0]), str(aa[1])], cwd=ROOT, env=env,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    res = json.loads(r.stdout.strip().splitlines()[-1])
    assert res["plan"] == dict(want, bytes_per_sample=bps), res["plan"]
    assert res["batches"] == want["batches"]
    assert res["native"] == ["shutter_combine_clip"] * (want["batches"] * want["passes"])
    flt, image = compiled("rotate")
    inv = invoke(flt, image)
    here = flt.clip_sampled_plan(W, H, W, k, aa, n)
    assert here["batches"] == 1 and here["passes"] == 1      # this process has the default budget
    single = inv.render_clip(frames=list(range(n)), ts=[0.1 + 0.2 * i for i in range(n)], shutter_samples=k, shutter_span=SPAN, aa=aa)
    assert res["sha"] == hashlib.sha256(single.tobytes()).hexdigest()


# ---- 5. state ----

@pytest.mark.parametrize("mode", MODES)
def test_the_callers_sampling_offset_is_put_back(mode):
    flt, image = compiled("rotate")
    inv, fresh = invoke(flt, image), invoke(flt, image)
    fresh.set_sampling_offset(-0.5, 0.25)
    want = fresh.render(t=0.3, frame=1)
    assert not np.array_equal(want, invoke(flt, image).render(t=0.3, frame=1))
    inv.set_sampling_offset(-0.5, 0.25)
    inv.render_clip(frames=FRAMES, ts=TS, aa=(2, 3), shutter_mode=mode)
    assert np.array_equal(inv.render(t=0.3, frame=1), want)


@pytest.mark.parametrize("mode", MODES)
def test_the_grid_replaces_the_callers_sampling_offset(mode):
    """On an invocation with a sampling offset a motion-blurred clip renders at that offset (its bytes:
    tests/test_gpu_clip_shutter.py), the grid clip behind it at the grid's own offsets -- the restatement's, which knows
    nothing of the caller's -- and a single render after both at the caller's offset again."""
    w = h = 17
    frames, ts, offset = [2, 0], [0.9, 0.1], (-0.5, 0.25)
    flt, image = compiled("rotate")
    inv, other, fresh = (invoke(flt, image, w, h) for _ in range(3))
    inv.set_sampling_offset(*offset)
    fresh.set_sampling_offset(*offset)
    inv.render_clip(frames=frames, ts=ts, shutter_samples=3, shutter_span=SPAN, shutter_mode=mode)
    got = inv.render_clip(frames=frames, ts=ts, aa=2, shutter_mode=mode)
    subs = sub_sample_maps(other, frames, ts, 1, 0.0, 2)
    for i in range(len(frames)):
        assert np.array_equal(got[i], G.combine(subs[i], bpp=4, floatmap=False)), (mode, i)
    assert np.array_equal(inv.render(t=0.3, frame=1), fresh.render(t=0.3, frame=1))
    assert not np.array_equal(inv.render(t=0.3, frame=1), other.render(t=0.3, frame=1))      # (left at offset 0)


def test_the_callers_sampling_offset_is_put_back_after_a_failed_call():
    """The nested clip fails behind the first change of the offset: a blur told to read the render's own frame of a
    sequence, at a frame number the sequence does not have."""
    flt = mm.Filter(P.BLUR)
    seq = P.SEQ[:, :H, :W]
    inv, fresh = flt.invoke(W, H), flt.invoke(W, H)
    for v in (inv, fresh):
        v.set_image("in", seq)
        v.set_native_input_frame("current")
        v.set_sampling_offset(0.25, -0.5)
    with pytest.raises(mm.MathMapError, match="frame"):
        inv.render_clip(frames=[1, 7], ts=[0.2, 0.4], aa=2)
    assert np.array_equal(inv.render(t=0.3, frame=1), fresh.render(t=0.3, frame=1))
    fresh.set_sampling_offset(0.0, 0.0)
    assert not np.array_equal(inv.render(t=0.3, frame=1), fresh.render(t=0.3, frame=1))


def test_plain_shutter_and_oversampled_clips_around_a_sampled_clip():
    flt = mm.Filter(ROTATE, supersampling=True)
    inv = invoke(flt, None)

    def others():
        return (inv.render_clip(frames=FRAMES, ts=TS), inv.render_clip(frames=FRAMES, ts=TS, shutter_samples=3, shutter_span=SPAN),
                inv.render_clip(frames=FRAMES, ts=TS, shutter_samples=3, shutter_span=SPAN, shutter_mode="fused"),
                inv.render_clip(frames=FRAMES, ts=TS, supersample=True))
    before = others()
    sampled = [inv.render_clip(frames=FRAMES, ts=TS, aa=2, shutter_mode=mode) for mode in MODES]
    assert np.array_equal(sampled[0], sampled[1])
    for b in before:
        assert not np.array_equal(sampled[0], b)
    for a, b in zip(others(), before):
        assert np.array_equal(a, b)
    assert np.array_equal(inv.render_clip(frames=FRAMES, ts=TS, aa=2), sampled[0])
    assert np.array_equal(inv.render_clip(frames=FRAMES, ts=TS, aa=1), before[0])


@pytest.mark.parametrize("name", ["blur", "closure", "wave"])
def test_filters_without_a_fused_variant_take_the_maps_path(name):
    flt, image = compiled(name)
    assert flt.clip_sampled_fused_plan(W, H, 2, 2, N)["fused"] == 0
    inv, other = invoke(flt, image), invoke(flt, image)
    got = inv.render_clip(frames=FRAMES, ts=TS, aa=2, shutter_samples=2, shutter_span=SPAN, shutter_mode="fused")
    assert inv.clip_sampled_fused_batches() == 0 and inv.clip_sampled_batches() == 1
    assert np.array_equal(got, other.render_clip(frames=FRAMES, ts=TS, aa=2, shutter_samples=2, shutter_span=SPAN))


# ---- 6. the command line ----

def test_cli_writes_the_python_result(tmp_path):
    src = "filter swirl (float k: 0-8 (3)) rgba:[0.5 + 0.5 * sin(k * r + t * 6), 0.5 + 0.5 * cos(a * 5 + t * 3), frame / 6, 1] end"
    want = mm.Filter(src).invoke(W, H).render_clip(num_frames=3, shutter_samples=3, shutter=0.5, aa=2)
    plain = mm.Filter(src).invoke(W, H).render_clip(num_frames=3, shutter_samples=3, shutter=0.5)
    assert not np.array_equal(want, plain)
    for mode in MODES:
        p = subprocess.run([CLI, "-F", "3", "--aa=2", "--shutter-samples=3", "--shutter=0.5", "--shutter-mode=" + mode, "--batch-frames=2",
                            "-s", "%dx%d" % (W, H), src, str(tmp_path / (mode + "%d.png"))], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                           text=True, timeout=300)
        assert p.returncode == 0, p.stderr
        for i in range(3):
            assert np.array_equal(read_png(str(tmp_path / ("%s%d.png" % (mode, i)))), want[i, :, :, :3]), (mode, i)
