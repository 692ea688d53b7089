"""Clip rendering of filters whose native calls are gaussian_blur: the blurs of a batch of frames run as one launch set
(k_iir_*_clip, one grid row per blur), where mmhip_render runs four launches and a host round trip per frame.

The yardstick is the single-frame path of the same build, by the method of tests/test_gpu_render_clip.py: two buffers
filled with sentinel bytes, the clip in one, a loop of single renders in the other, whole buffers equal and nothing
written outside the bands.  Byte for byte (float maps bit for bit), no tolerance: the batched sweeps are the single-frame
sweeps' own template code under -ffp-contract=off.  Frames of two filters are held against the oracle as well."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import mathmap_amd as mm
from oracle.ccgen import CpuFilter
from tests import filters as F
from tests import clip_native_probes as N
from tests.test_gpu_render_clip import FRAMES, TS, clip_and_loop, make

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 333, 207
COUNTS = [1, 2, 7, 40]


def clip_of(n):
    """n (frame, t) pairs: the clip tests' non-monotone lists, continued with times that do not repeat."""
    frames = [FRAMES[i % len(FRAMES)] + 7 * (i // len(FRAMES)) for i in range(n)]
    ts = [TS[i] if i < len(TS) else ((i * 37) % 101) / 101.0 for i in range(n)]
    return frames, ts


def counters(inv):
    return inv.clip_native_batches(), inv.clip_native_blurs(), inv.clip_native_direct_frames()


def assert_native_free_counters_untouched(inv):
    assert inv.clip_batched_launches() == 0 and inv.clip_prologue_frames() == 0


# ---- (a) the blur writes the frames' bytes itself ----

@pytest.mark.parametrize("n", COUNTS)
def test_direct_blur_with_sigma_following_t(n):
    flt, inv = make(N.DIRECT_T)
    frames, ts = clip_of(n)
    got = clip_and_loop(inv, frames, ts, what=("direct_t", n))
    assert counters(inv) == (1, n, n)
    assert_native_free_counters_untouched(inv)
    if n > 1:
        assert not np.array_equal(got[0], got[1])


def test_direct_blur_launches_no_pixel_kernel():
    """With timing on, every pixel launch of a clip leaves an event pair: the direct path leaves none."""
    flt, inv = make(N.DIRECT_T)
    inv.enable_timing(True)
    inv.render_clip(frames=FRAMES, ts=TS)
    assert inv.drain_kernel_ms() == []
    assert counters(inv) == (1, 7, 7)
    flt, inv = make(N.DISTORTED)
    inv.enable_timing(True)
    inv.render_clip(frames=FRAMES, ts=TS)
    assert len(inv.drain_kernel_ms()) == 1
    assert counters(inv) == (1, 7, 0)


# ---- (b) constant arguments: one blur for the whole clip ----

@pytest.mark.parametrize("n", COUNTS)
def test_constant_arguments_compute_one_blur(n):
    flt, inv = make("gauss_direct", uservals={"hdev": 0.03, "vdev": 0.025})
    frames, ts = clip_of(n)
    got = clip_and_loop(inv, frames, ts, what=("gauss_direct", n))
    assert inv.clip_native_batches() == 1 and inv.clip_native_blurs() == 1
    # frames that share a blur cannot each have it write their bytes: one frame alone can
    assert inv.clip_native_direct_frames() == (1 if n == 1 else 0)
    for i in range(1, n):
        assert np.array_equal(got[i], got[0])
    assert_native_free_counters_untouched(inv)


# ---- (c) .. (f): how the pixel reads the blur ----

SHAPES = [("distorted", N.DISTORTED), ("chain", N.CHAIN), ("chain_both", N.CHAIN_BOTH), ("conditional", N.CONDITIONAL),
          ("hoisted", N.HOISTED), ("plain", N.PLAIN)]


@pytest.mark.parametrize("n", COUNTS)
@pytest.mark.parametrize("case", SHAPES, ids=[c[0] for c in SHAPES])
def test_clip_equals_single_frames(case, n):
    name, src = case
    flt, inv = make(src)
    frames, ts = clip_of(n)
    got = clip_and_loop(inv, frames, ts, what=(name, n))
    batches, blurs, direct = counters(inv)
    assert batches == 1, name
    sites = flt.num_native_calls
    if name == "conditional":
        executing = sum(1 for t in ts if np.float32(t) > np.float32(0.5))
        assert 0 < executing < n or n < 3
        assert blurs == executing and direct == 0
    elif name == "chain":
        assert blurs == 2 * n and direct == n      # the second blur's bytes are the frame
    else:
        assert blurs == sites * n and direct == 0, name
    assert_native_free_counters_untouched(inv)
    if n > 1:
        assert not np.array_equal(got[0], got[1]), name


def test_frames_where_the_call_does_not_execute():
    """t <= 0.5: the frame is the input, and no blur is computed for it; a clip of such frames alone computes none."""
    flt, inv = make(N.CONDITIONAL)
    got = clip_and_loop(inv, [3, 4, 5], [0.1, 0.5, 0.25], what="none executes")
    assert counters(inv) == (1, 0, 0)
    assert np.array_equal(got[0], got[1]) and np.array_equal(got[0], got[2])      # the input itself, whatever t


# ---- (g) repeated (frame, t) pairs ----

def test_repeated_frames_share_their_blurs():
    flt, inv = make(N.DISTORTED)
    frames, ts = [5, 5, 0, 5, 9, 0], [0.9, 0.9, 0.5, 0.9, 0.9, 0.5]
    got = clip_and_loop(inv, frames, ts, what="repeats")
    assert counters(inv) == (1, 2, 0)          # the blur's arguments read t alone: two distinct times
    assert np.array_equal(got[0], got[1]) and np.array_equal(got[0], got[3]) and np.array_equal(got[2], got[5])
    flt, inv = make(N.CHAIN)
    clip_and_loop(inv, frames, ts, what="chain repeats")
    assert counters(inv) == (1, 4, 0)          # shared blurs write maps, the pixel kernel reads them
    flt, inv = make(N.DIRECT_T)
    clip_and_loop(inv, [1, 2, 3], [0.25, 0.5, 0.75], what="distinct")
    clip_and_loop(inv, [1, 2, 3], [0.25, 0.5, 0.25], what="one repeat")
    assert counters(inv) == (2, 5, 3)


# ---- (h) output shapes ----

@pytest.mark.parametrize("case", [("direct_t", N.DIRECT_T), ("distorted", N.DISTORTED)], ids=["direct_t", "distorted"])
def test_bands_regions_strides_formats(case):
    name, src = case
    flt, inv = make(src)
    frames, ts = clip_of(4)
    region = (21, 9, 235, 150)
    for rows in ((9, 159), (40, 41), (33, 120), (-5, 500)):
        clip_and_loop(inv, frames, ts, region=region, rows=rows, row_stride=235 * 4 + 52, frame_stride=160 * (235 * 4 + 52) + 1000, what=(name, rows))
    clip_and_loop(inv, frames, ts, rows=(50, 120), what=(name, "band of the full width"))
    # strides the direct output does not take (not multiples of 4): maps and the pixel kernel, the same bytes
    before = inv.clip_native_direct_frames()
    clip_and_loop(inv, frames, ts, row_stride=W * 4 + 6, frame_stride=H * (W * 4 + 6) + 77, what=(name, "frame stride % 4 != 0"))
    assert inv.clip_native_direct_frames() == before
    for bpp in (1, 2, 3):
        clip_and_loop(inv, frames[:3], ts[:3], bpp=bpp, what=(name, bpp))
        clip_and_loop(inv, frames[:3], ts[:3], bpp=bpp, row_stride=W * bpp + 5, frame_stride=H * (W * bpp + 5) + 77, what=(name, bpp, "padded"))
    got = clip_and_loop(inv, frames[:3], ts[:3], floatmap=True, what=(name, "float map"))
    assert got.dtype == np.float32 and np.isfinite(got).all()
    clip_and_loop(inv, frames[:3], ts[:3], floatmap=True, region=(21, 9, 100, 77), rows=(20, 60), frame_stride=40 * 16 * W + 4096, what=(name, "float-map region"))
    assert inv.clip_native_direct_frames() == before
    assert_native_free_counters_untouched(inv)


def test_direct_output_of_an_offset_region():
    flt, inv = make(N.DIRECT_T)
    frames, ts = clip_of(4)
    clip_and_loop(inv, frames, ts, region=(21, 9, 235, 150), rows=(33, 120), row_stride=235 * 4 + 52, frame_stride=160 * (235 * 4 + 52) + 1000, what="direct region")
    assert counters(inv) == (1, 4, 4)


# ---- (i) batches forced by the byte budget and by the frame cap ----

CHILD = r"""
import json, sys
sys.path.insert(0, %r)
from tests import clip_native_probes as N
from tests.test_gpu_render_clip import make, clip_and_loop, FRAMES, TS
out = {}
for name, src in (("direct_t", N.DIRECT_T), ("distorted", N.DISTORTED)):
    flt, inv = make(src)
    clip_and_loop(inv, FRAMES, TS, what=name)
    out[name] = [flt.clip_native_plan(333, 207, 7), inv.clip_native_batches(), inv.clip_native_blurs(), inv.clip_native_direct_frames(),
                 inv.clip_batched_launches()]
print(json.dumps(out))
"""


@pytest.mark.parametrize("knob", ["MMHIP_CLIP_NATIVE_BYTES", "MMHIP_CLIP_MAX_FRAMES"])
def test_three_batches(knob):
    value = str(3 * N.bytes_per_frame(W, H, 1) + 100) if knob == "MMHIP_CLIP_NATIVE_BYTES" else "3"
    env = dict(os.environ, **{knob: value})
    r = subprocess.run([sys.executable, "-c", CHILD % ROOT], cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert sorted(out) == ["direct_t", "distorted"]
    for name, (plan, batches, blurs, direct, native_free) in out.items():
        assert plan["frames_per_batch"] == 3 and plan["batches"] == 3, name
        assert batches == 3 and blurs == 7 and native_free == 0, name
        assert direct == (7 if name == "direct_t" else 0), name


# ---- (j) batches the batched blur does not take ----

def test_a_deviation_below_half_a_pixel_falls_back():
    """s * t at t = 0: the FIR path for that frame, so the whole batch is rendered by the loop -- the same bytes, no native batch counted."""
    flt, inv = make(N.FIR_AT_ZERO)
    assert flt.clip_native_plan(W, H, 4)["eligible"] == 1
    clip_and_loop(inv, [1, 2, 3, 4], [0.9, 0.0, 0.5, 1.0], what="fir frame")
    assert counters(inv) == (0, 0, 0)
    clip_and_loop(inv, [1, 2, 3, 4], [0.9, 0.7, 0.5, 1.0], what="iir frames")
    assert counters(inv) == (1, 4, 4)
    assert_native_free_counters_untouched(inv)


def test_an_input_of_another_size_falls_back():
    flt, inv = make(N.DIRECT_T, image=F.synthetic_image(200, 120, seed=9))
    clip_and_loop(inv, FRAMES[:3], TS[:3], what="another size")
    assert counters(inv) == (0, 0, 0)
    flt, inv = make(N.DISTORTED, image=F.synthetic_image(W + 1, H, seed=9))
    clip_and_loop(inv, FRAMES[:3], TS[:3], what="one column more")
    assert counters(inv) == (0, 0, 0)
    assert_native_free_counters_untouched(inv)


def test_ineligible_filters_keep_the_loop():
    for name, src, opts in (("in_loop", N.IN_LOOP, {}), ("tolerance", F.GAUSS_DIRECT, {"gauss_mode": "tolerance"})):
        flt, inv = make(src, **opts)
        clip_and_loop(inv, FRAMES[:3], TS[:3], what=name)
        assert counters(inv) == (0, 0, 0), name
    flt, inv = make(N.DIRECT_T)
    inv.set_native_row_margin(0)
    clip_and_loop(inv, FRAMES[:3], TS[:3], what="row margin")
    assert counters(inv) == (0, 0, 0)


# ---- (k) state ----

@pytest.mark.parametrize("case", [("direct_t", N.DIRECT_T), ("distorted", N.DISTORTED), ("chain_both", N.CHAIN_BOTH)], ids=["direct_t", "distorted", "chain_both"])
def test_single_clip_single_with_a_user_value_changed(case):
    """A clip leaves the single-frame path's maps, memo and image table alone, and a single render leaves nothing a clip
    could pick up: every result equals a fresh invocation's."""
    name, src = case
    flt, inv = make(src)
    fresh = lambda s: make(src, uservals={"s": s})[1]
    frames, ts = FRAMES[:3], TS[:3]
    ref, ref2 = fresh(0.02), fresh(0.035)
    single = inv.render(t=0.5, frame=0)
    assert np.array_equal(single, ref.render(t=0.5, frame=0))
    assert np.array_equal(inv.render(t=0.5, frame=0), single)      # (the second request for one argument set writes the map)
    a = inv.render_clip(frames=frames, ts=ts)
    for i in range(3):
        assert np.array_equal(a[i], ref.render(t=ts[i], frame=frames[i])), (name, i)
    assert np.array_equal(inv.render(t=0.5, frame=0), single)
    inv.set("s", 0.035)
    b = inv.render_clip(frames=frames, ts=ts)
    for i in range(3):
        assert np.array_equal(b[i], ref2.render(t=ts[i], frame=frames[i])), (name, i)
    assert not np.array_equal(a, b)
    assert np.array_equal(inv.render(t=0.9, frame=5), ref2.render(t=0.9, frame=5))
    inv.set("s", 0.02)
    assert np.array_equal(inv.render_clip(frames=frames, ts=ts), a)
    assert np.array_equal(inv.render(t=0.5, frame=0), single)
    assert inv.clip_native_batches() == 3


def test_a_new_input_image_is_what_the_next_clip_blurs():
    flt, inv = make(N.DIRECT_T)
    a = inv.render_clip(frames=FRAMES[:2], ts=TS[:2])
    other = F.synthetic_image(W, H, seed=77)
    inv.set_image("in", other)
    b = inv.render_clip(frames=FRAMES[:2], ts=TS[:2])
    ref = make(N.DIRECT_T, image=other)[1]
    for i in range(2):
        assert np.array_equal(b[i], ref.render(t=TS[i], frame=FRAMES[i])), i
    assert not np.array_equal(a, b)


# ---- (l) timing ----

def test_timing_drains_the_clip_labels():
    flt, inv = make(N.CHAIN)
    inv.enable_timing(True)
    inv.render_clip(frames=FRAMES, ts=TS)
    got = inv.drain_native_kernel_ms()
    labels = [name for name, ms in got]
    four = ["iir_causal_vertical_clip", "iir_anticausal_vertical_clip", "iir_causal_horizontal_clip", "iir_anticausal_horizontal_clip"]
    assert labels == four + four      # the first blur reads the drawable, the second its map: one group each
    assert all(ms > 0 for name, ms in got)
    inv.render(t=0.3)
    assert [name for name, ms in inv.drain_native_kernel_ms()] == [l[:-5] for l in four + four]


# ---- (m) against the oracle ----

@pytest.mark.parametrize("case", [("direct_t", N.DIRECT_T), ("chain", N.CHAIN)], ids=["direct_t", "chain"])
def test_float_maps_against_the_oracle(case):
    """The exact chain equals the oracle's blur bit for bit (tests/test_gpu_parity.py holds the single-frame path to
    that), and these filters' pixel is the blur's own value: so do the clip's float maps."""
    name, src = case
    w, h = 129, 65
    img = F.synthetic_image(w, h, seed=11)
    flt, inv = make(src, w, h, image=img)
    frames, ts = FRAMES[:3], TS[:3]
    got = clip_and_loop(inv, frames, ts, floatmap=True, what=name)
    assert inv.clip_native_batches() == 1
    cf = CpuFilter(flt.ir_json_raw)
    for i in range(3):
        want = cf.render(w, h, images={"in": img}, t=ts[i], frame=frames[i], floatmap=True)
        assert np.array_equal(got[i].view(np.int32), want.view(np.int32)), (name, i)


# ---- (n) native filters read the render's own frame of a sequence (opt-in) ----

RENDERED = "stretched filter rendered (stretched image in) rr = render(in); rr(xy * 0.9) end"
SEQ_N = 6
CURRENT_CASES = [
    ("iir", N.DIRECT_T, {}, (W, H)),
    ("fir", F.GAUSS_DIRECT, {"hdev": 0.001, "vdev": 0.03}, (W, H)),
    ("another size", N.DIRECT_T, {}, (200, 120)),
    ("render", RENDERED, {}, (W, H)),
]


def sequence(size, seed=21):
    w, h = size
    return np.stack([F.synthetic_image(w, h, seed=seed + k) for k in range(SEQ_N)])


@pytest.mark.parametrize("case", CURRENT_CASES, ids=[c[0] for c in CURRENT_CASES])
def test_current_mode_reads_the_renders_frame(case):
    """Frame n of a 6-frame input in `current` mode: what an invocation renders that has frame n bound as a single image."""
    name, src, uv, size = case
    seq = sequence(size)
    flt, inv = make(src, uservals=uv, image=seq)
    zero = inv.render(t=0.4, frame=3)
    assert np.array_equal(zero, make(src, uservals=uv, image=seq[0])[1].render(t=0.4, frame=3)), name      # the default: frame 0
    inv.set_native_input_frame("current")
    refs = [make(src, uservals=uv, image=seq[k])[1] for k in range(SEQ_N)]
    for n, t in ((3, 0.4), (0, 0.4), (5, 0.9), (3, 0.4)):
        assert np.array_equal(inv.render(t=t, frame=n), refs[n].render(t=t, frame=n)), (name, n)
    assert not np.array_equal(inv.render(t=0.4, frame=3), zero), name
    # frames A, B, A at one t: B's result never serves A, nor A's B (twice each: the second request writes the map)
    for n in (2, 4, 2, 2, 4, 4, 2):
        assert np.array_equal(inv.render(t=0.25, frame=n), refs[n].render(t=0.25, frame=n)), (name, "A B A", n)
    frames, ts = [0, 3, 5, 3, 0, 1], [0.9, 0.1, 0.5, 0.1, 0.33, 0.9]
    got = inv.render_clip(frames=frames, ts=ts)
    for i, n in enumerate(frames):
        assert np.array_equal(got[i], refs[n].render(t=ts[i], frame=n)), (name, "clip", i)
    clip_and_loop(inv, frames, ts, what=(name, "current"))
    if name == "iir":
        assert counters(inv) == (2, 10, 0)      # (3, 0.1) twice: five blurs per clip, shared, so maps and the pixel kernel
        clip_and_loop(inv, [5, 4, 3], [0.5, 0.5, 0.5], what=(name, "one t, three frames"))
        assert counters(inv) == (3, 13, 3)      # equal arguments, different frames: three blurs
    else:
        assert counters(inv) == (0, 0, 0), name
    inv.set_native_input_frame("zero")
    assert np.array_equal(inv.render(t=0.4, frame=3), zero), name


def test_current_mode_refuses_a_frame_the_sequence_does_not_have():
    flt, inv = make(N.DIRECT_T, image=sequence((W, H)))
    inv.render(t=0.1, frame=SEQ_N)      # the default reads frame 0 whatever the frame number
    inv.set_native_input_frame("current")
    for n in (SEQ_N, -1, 1000):
        with pytest.raises(mm.MathMapError, match=r"gaussian_blur: frame %d is outside" % n):
            inv.render(t=0.1, frame=n)
    with pytest.raises(mm.MathMapError, match=r"gaussian_blur: frame 6 is outside"):
        inv.render_clip(frames=[0, 6, 1], ts=[0.1, 0.2, 0.3])
    assert np.array_equal(inv.render(t=0.1, frame=5), make(N.DIRECT_T, image=sequence((W, H))[5])[1].render(t=0.1, frame=5))
    flt, inv = make(RENDERED, image=sequence((W, H)))
    inv.set_native_input_frame("current")
    with pytest.raises(mm.MathMapError, match=r"render\(\): frame 7 is outside"):
        inv.render(frame=7)
    with pytest.raises(mm.MathMapError, match="native input frame"):
        inv.set_native_input_frame("last")
    # a single image is not a sequence: any frame number
    flt, inv = make(N.DIRECT_T)
    inv.set_native_input_frame("current")
    assert np.array_equal(inv.render(t=0.1, frame=99), make(N.DIRECT_T)[1].render(t=0.1, frame=99))


# ---- (o) a clip of video frames ----

def test_24_frames_of_1920x1080():
    w, h = 1920, 1080
    flt, inv = make(N.DIRECT_T, w, h, image=F.synthetic_image(w, h, seed=5), uservals={"s": 0.006})
    frames = list(range(24))
    ts = [i / 24.0 for i in frames]
    clip_and_loop(inv, frames, ts, what="1080p")
    assert counters(inv) == (1, 24, 24)
    flt, inv = make(N.DISTORTED, w, h, image=F.synthetic_image(w, h, seed=5), uservals={"s": 0.006})
    clip_and_loop(inv, frames[:8], ts[:8], what="1080p distorted")
    assert counters(inv) == (1, 8, 0)
