"""Adaptively anti-aliased clips on the GPU (mmhip_render_clip_adaptive: the list path through k_aa_contrast_clip and
mm_pixels_refine, the select path through the full grid-supersampled clip).

Expected output everywhere is where(mask, aa_clip, plain): the mask is tests/adaptive_aa_reference.py applied to
render_clip(floatmap=True) of a *second* invocation, aa_clip is that invocation's render_clip(aa=...) and plain its
render_clip() in the format asked for -- three renders of code that predates the adaptive call.  Everything is compared
bit for bit in whole sentinel-filled buffers."""
import ctypes as C
import functools
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import mathmap_amd as mm
from mathmap_amd._lib import lib
from tests import adaptive_aa_reference as A
from tests import shutter_fused_probes as P
from tests.test_gpu_clip_sampled import Layout
from tests.test_gpu_clip_shutter import SENTINEL, device_filled, device_read, read_png, same_buffer

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "mathmap_amd", "mathmap_hip_cli")
f32 = np.float32
W, H, N = P.W, P.H, 3
FRAMES = [2, 0, 1]
TS = [0.9, 0.1, 0.5]
REFINES = ("list", "select")
ROW_SLICE = ("wave", "extreme")          # probes with a per-row slice: no refine variant, the select path under either mode
ELIGIBLE = [name for name in P.PROBES if name not in ROW_SLICE]
# One middle threshold per probe, chosen on the CPU: the oracle (oracle.ccgen.CpuFilter, floatmap=True) rendered the 97 x 61
# frames at FRAMES / TS, and the share of pixels whose largest clamped contrast to a neighbour exceeds the value was, per
# frame: pair .45 .51 .50, wave .55 .59 .50, sequence .49 .52 .54, shared .49 .70 .58, rand .61 .50 .61, recursive .68 .68
# .69, droste .55 (t is not read), mandelbrot .17 (t is not read), extreme .70 .29 .57.
MIDDLE = {"pair": 0.05, "wave": 0.15, "sequence": 0.5, "shared": 0.1, "rand": 0.7, "recursive": 0.1, "droste": 0.1,
          "mandelbrot": 0.05, "extreme": 0.05}
T_IS_NOT_READ = ("droste", "mandelbrot")   # their three frames are one picture, and so are their masks


def render(inv, lay, aa=1, threshold=None, refine="list", frames=FRAMES, ts=TS, region=None, rows=None, **more):
    dev = device_filled(lay.total)
    try:
        assert inv.render_clip(frames=frames, ts=ts, out_ptr=dev + lay.lead, rows=rows, region=region, row_stride=lay.stride,
                               frame_stride=lay.fstride, bpp=lay.bpp, floatmap=lay.floatmap, aa=aa, aa_threshold=threshold,
                               aa_refine=refine, **more) is None
        inv.sync()
        return device_read(dev, lay.total)
    finally:
        lib().mmhip_device_free(C.c_void_p(dev))


def pixels(buf, lay):
    """The frames of a buffer as [rows, region_w, 4] float32 or [rows, region_w, bpp] uint8 arrays."""
    out = []
    for i in range(lay.n):
        rows = [buf[lay.lead + i * lay.fstride + r * lay.row_step:][:lay.row_bytes] for r in range(lay.nrows)]
        px = np.stack(rows)
        out.append(px.view(f32).reshape(lay.nrows, lay.rw, 4) if lay.floatmap else px.reshape(lay.nrows, lay.rw, lay.bpp))
    return out


class Reference:
    """The three existing renders of one (filter, size, frames, region, rows), by an invocation of its own; each render
    is made once and shared by the tests that need it."""

    def __init__(self, flt, image, w, h, frames=FRAMES, ts=TS, region=None, rows=None):
        self.inv, self.w, self.frames, self.ts, self.region, self.rows = P.invoke(flt, image, w, h), w, list(frames), list(ts), region, rows
        rx, ry, self.rw, rh = region if region is not None else (0, 0, w, h)
        first, last = rows if rows is not None else (ry, ry + rh)
        self.nrows = min(last, ry + rh) - max(first, 0)
        self.cache = {}
        self.base = self.get(1, dict(floatmap=True))

    def layout(self, lay_args):
        return Layout(len(self.frames), self.rw, self.nrows, self.w, **lay_args)

    def get(self, aa, lay_args):
        key = (aa, tuple(sorted(lay_args.items())))
        if key not in self.cache:
            lay = self.layout(lay_args)
            self.cache[key] = pixels(render(self.inv, lay, aa, frames=self.frames, ts=self.ts, region=self.region, rows=self.rows), lay)
        return self.cache[key]

    def masks(self, threshold):
        return [A.mask(b, threshold) for b in self.base]

    def expected(self, aa, threshold, lay_args):
        """(the whole buffer, the masks)"""
        masks = self.masks(threshold)
        full, plain = self.get(aa, lay_args), self.get(1, lay_args)
        return self.layout(lay_args).expected([A.select(m, a, p) for m, a, p in zip(masks, full, plain)]), masks


@functools.lru_cache(maxsize=None)
def reference(name, size):
    flt, image = P.compiled(name)
    return Reference(flt, image, *size)


def adaptive(name, size, lay_args, aa, threshold, refine, ref=None, **kw):
    """(the buffer, the counts, the invocation) of one adaptive call by a fresh invocation"""
    flt, image = P.compiled(name)
    inv = P.invoke(flt, image, *size)
    ref = ref or reference(name, size)
    got = render(inv, ref.layout(lay_args), aa, threshold, refine, frames=ref.frames, ts=ref.ts, region=ref.region, rows=ref.rows, **kw)
    return got, inv.clip_adaptive_refined(), inv


# ---- 1. every probe, size, grid, path and format against where(mask, aa_clip, plain) ----

SIZES = [(1, 1), (2, 1), (16, 16), (17, 17), (97, 61)]
FORMATS = {"floatmap": dict(floatmap=True, gap=80), "bpp4": dict(bpp=4, gap=52)}


@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("name", list(P.PROBES))
def test_frames_equal_the_choice_between_two_existing_renders(name, size):
    ref = reference(name, size)
    flt, image = P.compiled(name)
    pixels_per_frame = size[0] * size[1]
    nan_frames = [bool(np.isnan(b).any()) for b in ref.base]
    for aa in (2, 3, (2, 1)):
        for threshold in (-1.0, float("inf"), MIDDLE[name]):
            masks = ref.masks(threshold)
            sums = [int(m.sum()) for m in masks]
            if threshold < 0:
                assert sums == [pixels_per_frame] * N
            elif threshold == float("inf"):          # nothing but a NaN contrast refines: frames with a NaN texel that has a neighbour
                assert [s > 0 for s in sums] == [nan and pixels_per_frame > 1 for nan in nan_frames], (name, size, sums)
                if min(size) > 1:                    # (a frame one pixel wide or high has NaN coordinates, whatever the filter)
                    assert any(nan_frames) == (name == "extreme"), (name, size)
            elif size == (97, 61):                   # neither an empty nor a full mask, in any frame
                for s in sums:
                    assert 0.05 * pixels_per_frame <= s <= 0.95 * pixels_per_frame, (name, threshold, sums)
                if name not in T_IS_NOT_READ:
                    assert not np.array_equal(masks[0], masks[1]) and not np.array_equal(masks[1], masks[2]), name
            out = {}
            for refine in REFINES:
                inv = P.invoke(flt, image, *size)
                for fmt, lay_args in FORMATS.items():
                    want, _ = ref.expected(aa, threshold, lay_args)
                    got = render(inv, ref.layout(lay_args), aa, threshold, refine)
                    assert same_buffer(got, want, lay_args.get("floatmap", False)), (name, size, aa, threshold, refine, fmt)
                    assert list(inv.clip_adaptive_refined()) == sums, (name, size, aa, threshold, refine, fmt)
                    if threshold < 0:                # the bytes of the full aa clip
                        assert same_buffer(got, ref.layout(lay_args).expected(ref.get(aa, lay_args)), lay_args.get("floatmap", False))
                    if threshold == float("inf") and sum(sums) == 0:         # the bytes of the plain clip
                        assert same_buffer(got, ref.layout(lay_args).expected(ref.get(1, lay_args)), lay_args.get("floatmap", False))
                    out[refine, fmt] = got
                listed = refine == "list" and name in ELIGIBLE
                assert inv.clip_adaptive_batches() == 2
                assert inv.clip_sampled_batches() == (0 if listed else 2), (name, refine)       # the select path's nested clips
                assert inv.clip_sampled_fused_batches() == 0 and inv.clip_shutter_batches() == 0
            for fmt in FORMATS:                      # list path against select path, byte for byte
                assert np.array_equal(out["list", fmt], out["select", fmt]), (name, size, aa, threshold, fmt)


# ---- 2. a frame with nothing refined and a frame with everything refined in one batch ----

ALL_OR_NOTHING = """filter all_or_nothing ()
  k = if t > 0.5 then 1 else 0 end;
  rgba:[rand(0, 1) * k, 0.25, 0.5, 1]
end
"""


@pytest.mark.parametrize("refine", REFINES)
def test_an_empty_and_a_full_list_in_one_batch(refine):
    flt = mm.Filter(ALL_OR_NOTHING)
    w, h = 33, 19
    ref = Reference(flt, None, w, h, frames=[0, 1, 2], ts=[0.75, 0.25, 0.9])
    for lay_args in FORMATS.values():
        want, masks = ref.expected(2, 0.0, lay_args)
        assert [int(m.sum()) for m in masks] == [w * h, 0, w * h]
        inv = flt.invoke(w, h)
        got = render(inv, ref.layout(lay_args), 2, 0.0, refine, frames=ref.frames, ts=ref.ts)
        assert same_buffer(got, want, lay_args.get("floatmap", False)), (refine, lay_args)
        assert list(inv.clip_adaptive_refined()) == [w * h, 0, w * h]
        assert inv.clip_adaptive_batches() == 1


# ---- 3. coverage pinned without the GPU's help ----

V_EDGE = "stretched filter v_edge () if x < 0.1 then rgba:[1, 1, 1, 1] else rgba:[0, 0, 0, 1] end end"
H_EDGE = "stretched filter h_edge () if y < 0.1 then rgba:[1, 1, 1, 1] else rgba:[0, 0, 0, 1] end end"


@pytest.mark.parametrize("refine", REFINES)
@pytest.mark.parametrize("which", ["vertical", "horizontal"])
def test_a_hard_edge_is_refined_on_its_two_lines_only(which, refine):
    """16 x 16, aa = 4, threshold 0.5, everything worked out in NumPy: the single sample at offset 0 is 1 on one side of
    the edge and 0 on the other, the two lines that touch it are refined (32 pixels), the one whose footprint the edge
    crosses is f32(0.75) and everything else is 1 or 0.  x grows with the column: columns 8 and 9.  y grows upwards, so
    the same edge at y = 0.1 lies between rows 7 and 6."""
    n = 16
    pos = np.arange(n, dtype=np.float64)
    o = np.array([(a + 0.5) / 4 - 0.5 for a in range(4)], np.float64).astype(f32).astype(np.float64)
    if which == "vertical":
        src, centre, coord = V_EDGE, ((pos - 7.5) / 7.5).astype(f32), ((pos[None, :] - 7.5 + o[:, None]) / 7.5).astype(f32)
    else:
        src, centre, coord = H_EDGE, ((-pos + 7.5) / 7.5).astype(f32), ((-pos[None, :] + 7.5 - o[:, None]) / 7.5).astype(f32)
    single = (centre < f32(0.1)).astype(f32)                                      # the base map along the axis
    refined = np.zeros(n, bool)
    refined[1:] |= np.abs(single[1:] - single[:-1]) > f32(0.5)
    refined[:-1] |= np.abs(single[1:] - single[:-1]) > f32(0.5)
    lines = list(np.flatnonzero(refined))
    assert lines == ([8, 9] if which == "vertical" else [6, 7])
    acc = np.zeros(n, f32)                                                        # 16 sub-samples in the order b * 4 + a
    for s in range(16):
        k = s % 4 if which == "vertical" else s // 4
        acc = (acc + (coord[k] < f32(0.1)).astype(f32)).astype(f32) if s else (coord[k] < f32(0.1)).astype(f32)
    mean = (acc * f32(1.0 / 16.0)).astype(f32)
    line = np.where(refined, mean, single).astype(f32)
    crossed = 8 if which == "vertical" else 7
    assert line[crossed] == f32(0.75) and set(np.delete(line, crossed)) == {f32(0), f32(1)}
    grey = np.broadcast_to(line[None, :] if which == "vertical" else line[:, None], (n, n))
    want_px = np.stack([grey, grey, grey, np.ones((n, n), f32)], axis=2).astype(f32)
    inv = mm.Filter(src).invoke(n, n)
    lay = Layout(1, n, n, n, floatmap=True)
    got = render(inv, lay, 4, 0.5, refine, frames=[0], ts=[0.0])
    assert same_buffer(got, lay.expected([want_px]), True), (which, refine)
    assert list(inv.clip_adaptive_refined()) == [32]


# ---- 4. formats, bands, regions, padded rows and frame gaps ----

@pytest.mark.parametrize("bpp", [1, 2, 3, 4])
def test_every_format_with_padded_rows_and_frame_gaps(bpp):
    lay_args = dict(bpp=bpp, row_pad=13, gap=101, lead=61 + bpp)
    ref = reference("pair", (W, H))
    want, masks = ref.expected((2, 3), MIDDLE["pair"], lay_args)
    lay = ref.layout(lay_args)
    for refine in REFINES:
        got, counts, _ = adaptive("pair", (W, H), lay_args, (2, 3), MIDDLE["pair"], refine)
        assert np.array_equal(got, want), (bpp, refine)
        assert list(counts) == [int(m.sum()) for m in masks]
        # gaps and sentinels untouched: in front, behind the first row, between the frames
        assert (got[:lay.lead] == SENTINEL).all() and (got[lay.lead + W * bpp:lay.lead + lay.stride] == SENTINEL).all()
        assert (got[lay.lead + H * lay.stride:lay.lead + lay.fstride] == SENTINEL).all()


@pytest.mark.parametrize("case", ["band", "region", "region and band"])
def test_bands_and_regions_look_at_their_own_rectangle(case):
    region, rows = {"band": (None, (5, 23)), "region": ((11, 7, 70, 41), None), "region and band": ((11, 7, 70, 41), (13, 40))}[case]
    flt, image = P.compiled("shared")
    ref = Reference(flt, image, W, H, frames=[1, 0], ts=[0.3, 0.8], region=region, rows=rows)
    for lay_args in (dict(floatmap=True, gap=32), dict(bpp=3, row_pad=5, gap=7)):
        want, masks = ref.expected((3, 2), MIDDLE["shared"], lay_args)
        assert all(0 < m.sum() < m.size for m in masks)
        for refine in REFINES:
            got, counts, _ = adaptive("shared", (W, H), lay_args, (3, 2), MIDDLE["shared"], refine, ref=ref)
            assert same_buffer(got, want, lay_args.get("floatmap", False)), (case, refine, lay_args)
            assert list(counts) == [int(m.sum()) for m in masks]


# ---- 5. filters without a refine variant, batches ----

@pytest.mark.parametrize("name", ["blur", "wave"])
def test_filters_without_a_refine_variant_take_the_select_path(name):
    flt, image = P.compiled(name)
    assert flt.clip_adaptive_plan(W, H, W, 2, N)["list_path"] == 0
    ref = Reference(flt, image, W, H)
    threshold = 0.15 if name == "wave" else 0.02
    want, masks = ref.expected(2, threshold, FORMATS["bpp4"])
    assert all(0 < m.sum() < m.size for m in masks), [int(m.sum()) for m in masks]
    inv = P.invoke(flt, image)
    got = render(inv, ref.layout(FORMATS["bpp4"]), 2, threshold, "list")
    assert np.array_equal(got, want), name
    assert inv.clip_adaptive_batches() == 1 and inv.clip_sampled_batches() == 1
    assert list(inv.clip_adaptive_refined()) == [int(m.sum()) for m in masks]


CHILD = r"""
import hashlib, json, sys
sys.path.insert(0, %r)
from tests import shutter_fused_probes as P
flt, image = P.compiled("shared")
inv = P.invoke(flt, image)
inv.enable_timing(True)
n = int(sys.argv[1])
frames, ts = list(range(n)), [0.1 + 0.2 * i for i in range(n)]
out = inv.render_clip(frames=[f %% 3 for f in frames], ts=ts, aa=2, aa_threshold=0.1, aa_refine=sys.argv[2])
print(json.dumps({"plan": flt.clip_adaptive_plan(P.W, P.H, P.W, 2, n), "batches": inv.clip_adaptive_batches(),
                  "native": [name for name, ms in inv.drain_native_kernel_ms()], "counts": [int(c) for c in inv.clip_adaptive_refined()],
                  "sha": hashlib.sha256(out.tobytes()).hexdigest()}))
"""


@pytest.mark.parametrize("refine", REFINES)
def test_three_batches_leave_the_bytes_alone(refine):
    n, per_frame = 5, H * 16 * W + 4 * W * H          # a base map and a list: two frames fit, 5 are 2 + 2 + 1
    env = dict(os.environ, MMHIP_CLIP_SHUTTER_BYTES=str(2 * per_frame + 100))
    r = subprocess.run([sys.executable, "-c", CHILD % ROOT, str(n), refine], cwd=ROOT, env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    res = json.loads(r.stdout.strip().splitlines()[-1])
    assert res["plan"] == dict(list_path=1, frames_per_batch=2, batches=3, bytes_per_frame=per_frame, refine_grid_x=(W * H + 255) // 256)
    assert res["batches"] == 3
    assert [name for name in res["native"] if name == "aa_contrast_clip"] == ["aa_contrast_clip"] * 3
    flt, image = P.compiled("shared")
    inv = P.invoke(flt, image)
    assert flt.clip_adaptive_plan(W, H, W, 2, n)["batches"] == 1      # this process has the default budget
    single = inv.render_clip(frames=[f % 3 for f in range(n)], ts=[0.1 + 0.2 * i for i in range(n)], aa=2, aa_threshold=0.1, aa_refine=refine)
    assert res["sha"] == hashlib.sha256(single.tobytes()).hexdigest()
    assert res["counts"] == list(inv.clip_adaptive_refined()) and 0 < min(res["counts"])


# ---- 6. state ----

@pytest.mark.parametrize("refine", REFINES)
def test_the_callers_sampling_offset_is_put_back_and_not_used(refine):
    flt, image = P.compiled("shared")
    inv, fresh = P.invoke(flt, image), P.invoke(flt, image)
    fresh.set_sampling_offset(-0.5, 0.25)
    want = fresh.render(t=0.3, frame=1)
    assert not np.array_equal(want, P.invoke(flt, image).render(t=0.3, frame=1))
    inv.set_sampling_offset(-0.5, 0.25)
    got = inv.render_clip(frames=FRAMES, ts=TS, aa=(2, 3), aa_threshold=0.1, aa_refine=refine)
    assert np.array_equal(inv.render(t=0.3, frame=1), want)
    # the base maps are rendered at offset 0 whatever the caller's: the frames are those of an invocation at offset 0
    assert np.array_equal(got, P.invoke(flt, image).render_clip(frames=FRAMES, ts=TS, aa=(2, 3), aa_threshold=0.1, aa_refine=refine))


def test_the_callers_sampling_offset_is_put_back_after_a_refused_call():
    """The nested render of the base maps fails behind the change of the offset: a blur told to read the render's own
    frame of a sequence, at a frame number the sequence does not have."""
    flt = mm.Filter(P.BLUR)
    seq = P.SEQ[:, :H, :W]
    inv, fresh = flt.invoke(W, H), flt.invoke(W, H)
    for v in (inv, fresh):
        v.set_image("in", seq)
        v.set_native_input_frame("current")
        v.set_sampling_offset(0.25, -0.5)
    with pytest.raises(mm.MathMapError, match="frame"):
        inv.render_clip(frames=[1, 7], ts=[0.2, 0.4], aa=2, aa_threshold=0.1)
    assert np.array_equal(inv.render(t=0.3, frame=1), fresh.render(t=0.3, frame=1))
    fresh.set_sampling_offset(0.0, 0.0)
    assert not np.array_equal(inv.render(t=0.3, frame=1), fresh.render(t=0.3, frame=1))


def test_plain_shutter_oversampled_and_full_aa_clips_around_an_adaptive_clip():
    from tests.test_gpu_clip_shutter import ROTATE
    flt = mm.Filter(ROTATE, supersampling=True)
    inv = P.invoke(flt, None)

    def others():
        return (inv.render_clip(frames=FRAMES, ts=TS), inv.render_clip(frames=FRAMES, ts=TS, shutter_samples=3, shutter_span=0.07),
                inv.render_clip(frames=FRAMES, ts=TS, shutter_samples=3, shutter_span=0.07, shutter_mode="fused"),
                inv.render_clip(frames=FRAMES, ts=TS, supersample=True), inv.render_clip(frames=FRAMES, ts=TS, aa=2),
                inv.render_clip(frames=FRAMES, ts=TS, aa=2, shutter_mode="fused"))
    before = others()
    counters = (inv.clip_shutter_batches(), inv.clip_shutter_fused_batches(), inv.clip_sampled_fused_batches(), inv.clip_supersampled_batches())
    got = [inv.render_clip(frames=FRAMES, ts=TS, aa=2, aa_threshold=0.05, aa_refine=refine) for refine in REFINES]
    assert np.array_equal(got[0], got[1])
    for b in before:
        assert not np.array_equal(got[0], b)
    assert counters == (inv.clip_shutter_batches(), inv.clip_shutter_fused_batches(), inv.clip_sampled_fused_batches(), inv.clip_supersampled_batches())
    for a, b in zip(others(), before):
        assert np.array_equal(a, b)
    assert np.array_equal(inv.render_clip(frames=FRAMES, ts=TS, aa=2, aa_threshold=-1.0), before[4])
    assert np.array_equal(inv.render_clip(frames=FRAMES, ts=TS, aa=1, aa_threshold=0.05), before[0])
    assert len(inv.clip_adaptive_refined()) == 0          # the call delegated


# ---- 7. the command line ----

def test_cli_writes_the_python_result(tmp_path):
    src = "filter swirl (float k: 0-8 (3)) rgba:[0.5 + 0.5 * sin(k * r + t * 6), 0.5 + 0.5 * cos(a * 5 + t * 3), frame / 6, 1] end"
    want = mm.Filter(src).invoke(W, H).render_clip(num_frames=3, aa=2, aa_threshold=0.05)
    assert not np.array_equal(want, mm.Filter(src).invoke(W, H).render_clip(num_frames=3, aa=2))
    assert not np.array_equal(want, mm.Filter(src).invoke(W, H).render_clip(num_frames=3))
    for refine in REFINES:
        p = subprocess.run([CLI, "-F", "3", "--aa=2", "--aa-threshold=0.05", "--aa-refine=" + refine, "--batch-frames=2", "-s", "%dx%d" % (W, H),
                            src, str(tmp_path / (refine + "%d.png"))], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
        assert p.returncode == 0, p.stderr
        for i in range(3):
            assert np.array_equal(read_png(str(tmp_path / ("%s%d.png" % (refine, i)))), want[i, :, :, :3]), (refine, i)
