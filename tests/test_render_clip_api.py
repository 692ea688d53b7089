"""Clip rendering (mmhip_render_clip) without a GPU: the entry points and their argument checks, the clip variant of the
kernel text (and that asking for it leaves the single-frame text alone), its gfx950 compile for one filter of every
kernel class, the clip launch geometry and the arithmetic that cuts a clip into launches."""
import ctypes as C
import json
import os
import re
import subprocess
import sys

import pytest

import mathmap_amd as mm
from mathmap_amd._lib import lib
from mathmap_amd.api import GEOMETRY_FIELDS
from tests import filters as F
from tests import sequence_probes as P
from tests.clip_probes import MEDIUM, WAVE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLIP_KERNELS = ("mm_prologue_clip(mm_args A", "mm_pixels_clip(mm_args A")


def err():
    return lib().mmhip_last_error().decode()


# ---- entry points ----

def test_entry_points_exist_and_are_declared():
    header = open(os.path.join(ROOT, "include", "mmhip.h")).read()
    for name in ("mmhip_render_clip", "mmhip_clip_batched_launches", "mmhip_clip_prologue_frames",
                 "mmhip_filter_clip_launch_geometry", "mmhip_filter_clip_batch_plan", "mmhip_filter_clip_kernel_source",
                 "mmhip_filter_jit_clip"):
        assert hasattr(lib(), name), name
        assert re.search(r"\b%s\s*\(" % name, header), name
    for name in ("clip_kernel_source", "jit_clip", "clip_launch_geometry", "clip_batch_plan"):
        assert hasattr(mm.Filter, name), name
    for name in ("render_clip", "clip_batched_launches"):
        assert hasattr(mm.api.Invocation, name), name


def test_render_clip_refuses_bad_arguments_with_a_message():
    """The argument checks come before anything touches the invocation: a null one will do."""
    frames = (C.c_int * 2)(0, 1)
    ts = (C.c_float * 2)(0.0, 0.5)
    call = lib().mmhip_render_clip

    def refused(num_frames, fr, tt, row_stride, frame_stride, floatmap=0, bpp=4):
        rc = call(None, num_frames, fr, tt, 0, 0, 64, 32, 0, 32, None, row_stride, frame_stride, bpp, floatmap, None)
        assert rc != 0
        return err()

    assert "num_frames" in refused(0, frames, ts, 256, 8192)
    assert "num_frames" in refused(-3, frames, ts, 256, 8192)
    assert "frames and ts" in refused(2, None, ts, 256, 8192)
    assert "frames and ts" in refused(2, frames, None, 256, 8192)
    assert "bpp" in refused(2, frames, ts, 256, 8192, bpp=5)
    assert "frame_stride" in refused(2, frames, ts, 256, 8191)      # 32 rows of 256 bytes: one byte short
    assert "frame_stride" in refused(2, frames, ts, 300, 31 * 300 + 255)


def test_geometry_and_plan_refuse_bad_arguments():
    flt = F.load("ident")
    with pytest.raises(mm.MathMapError, match="num_frames"):
        flt.clip_launch_geometry(64, 64, 0)
    with pytest.raises(mm.MathMapError, match="empty region"):
        flt.clip_launch_geometry(0, 64, 3)
    with pytest.raises(mm.MathMapError, match="num_frames"):
        flt.clip_batch_plan(64, 64, 0)


# ---- kernel text ----

@pytest.mark.parametrize("name", ["ident", "pond", "mandelbrot", "droste"])
def test_single_frame_text_is_untouched_by_the_clip_text(name):
    """kernel_source is byte for byte what a filter gives that was never asked for its clip text -- before and after."""
    untouched = F.load(name).kernel_source
    flt = F.load(name)
    before = flt.kernel_source
    clip = flt.clip_kernel_source
    assert before == untouched and flt.kernel_source == untouched
    assert clip != untouched
    for k in ("mm_prologue(mm_args A", "mm_pixels(mm_args A", "const int nwg = gridDim.x;"):
        assert k in untouched and k not in clip, k
    for k in CLIP_KERNELS + ("const int nwg = C.nwg;", "struct mm_clip {", "A.t = mm_cf.t; A.frame = mm_cf.frame;"):
        assert k in clip and k not in untouched, k


def body_of(text, kernel):
    """The statements of `kernel` behind its head: from its MM_INTERNALS to the next kernel (or the end)."""
    at = text.index(kernel + "(mm_args A")
    at = text.index("MM_INTERNALS", at)
    end = text.find('extern "C" __global__', at)
    return text[at:end if end >= 0 else len(text)]


@pytest.mark.parametrize("name", ["ident", "pond", "mandelbrot", "droste"])
def test_clip_bodies_are_the_single_frame_bodies(name):
    flt = F.load(name)
    one, clip = flt.kernel_source, flt.clip_kernel_source
    assert body_of(clip, "mm_prologue_clip") == body_of(one, "mm_prologue")
    assert body_of(clip, "mm_pixels_clip") == body_of(one, "mm_pixels").replace("const int nwg = gridDim.x;", "const int nwg = C.nwg;      // the frame's workgroups (gridDim.x is padded)")
    # everything in front of the first kernel (prelude, filter functions) is the same text, plus the clip's own struct
    head = one[:one.index('extern "C" __global__')]
    assert clip.startswith(head)


def class_filters():
    """(id, filter factory, what its kernel_source must show): one filter of each kernel class."""
    seq = lambda template, frame: (lambda: mm.Filter(P.text(template, frame)))
    return [
        ("pair-mandelbrot", lambda: F.load("mandelbrot").specialized(), lambda f: f.launch_geometry(64, 64)["pair_mode"] == 1),
        ("loop-mandelbrot", lambda: F.load("mandelbrot"), lambda f: f.launch_geometry(64, 64)["unroll"] == 1 and not f.launch_geometry(64, 64)["single_pixel"]),
        ("unroll4-pond", lambda: F.load("pond"), lambda f: f.launch_geometry(64, 64)["unroll"] == 4),
        ("unroll2-medium", lambda: mm.Filter(MEDIUM), lambda f: f.launch_geometry(64, 64)["unroll"] == 2 and not f.launch_geometry(64, 64)["pair_mode"]),
        ("single-pixel-droste", lambda: F.load("droste"), lambda f: f.launch_geometry(64, 64)["single_pixel"] == 1),
        ("row-slice-wave", lambda: mm.Filter(WAVE), lambda f: "mm_rows(mm_args A" in f.kernel_source),
        ("recursive-function", lambda: F.load("recursive_data"), lambda f: "mm_filter_0" in f.kernel_source),
        ("slit", seq(P.SLIT, P.SLIT_FRAME), lambda f: True),
        ("blend", seq(P.BLEND, ""), lambda f: True),
    ]


@pytest.mark.parametrize("case", class_filters(), ids=[c[0] for c in class_filters()])
def test_clip_text_compiles_for_gfx950(case):
    name, make, is_of_class = case
    flt = make()
    assert is_of_class(flt), name
    clip = flt.clip_kernel_source
    for k in CLIP_KERNELS:
        assert k in clip, (name, k)
    assert ("mm_rows_clip(mm_args A" in clip) == ("mm_rows(mm_args A" in flt.kernel_source)
    assert flt.jit_clip(load=False) > 0, name


# ---- geometry ----

SHAPES = [(1920, 1080), (512, 512), (8192, 8192), (333, 207), (96, 64), (17, 5), (4096, 16)]


@pytest.mark.parametrize("name", ["ident", "pond", "mandelbrot", "droste"])
def test_clip_geometry_of_one_frame_is_the_single_frame_geometry(name):
    flt = F.load(name)
    for w, h in SHAPES:
        assert flt.clip_launch_geometry(w, h, 1) == flt.launch_geometry(w, h), (name, w, h)


def test_rows_per_item_grow_with_the_clip():
    flt = F.load("ident")
    one, clip = flt.clip_launch_geometry(1920, 1080, 1), flt.clip_launch_geometry(1920, 1080, 120)
    assert set(one) == set(GEOMETRY_FIELDS)
    assert one["wg1"] == one["tiles_x"] * -(-1080 // one["tile_h"]) < 8192      # below the first cut: one frame alone gets no more rows per item
    assert one["ppt"] == one["unroll"]      # one row per work-item, rounded to the kernel's step
    assert clip["ppt"] > one["ppt"]
    assert clip["wg1"] == one["wg1"] and clip["nwg"] < one["nwg"]
    assert clip["tiles_y"] * clip["tile_h"] * clip["ppt"] >= 1080
    # a work-item's rows stay rows of its frame: no taller than the frame rounded up to a tile
    tiny = flt.clip_launch_geometry(4096, 16, 60000)
    assert tiny["tile_h"] * tiny["ppt"] <= max(tiny["tile_h"] * tiny["unroll"], (16 + tiny["tile_h"] - 1) // tiny["tile_h"] * tiny["tile_h"])
    # the large-body kernel renders one pixel per work-item whatever the clip's length
    assert F.load("droste").clip_launch_geometry(1920, 1080, 120)["ppt"] == 1


def test_forced_rows_per_item(monkeypatch):
    monkeypatch.setenv("MMHIP_PPT", "8")
    flt = F.load("ident")
    assert flt.clip_launch_geometry(1920, 1080, 120)["ppt"] == 8 == flt.launch_geometry(1920, 1080)["ppt"]


@pytest.mark.parametrize("name", ["ident", "pond", "mandelbrot", "droste"])
def test_batch_plan_honours_the_caps(name):
    flt = F.load(name)
    for w, h in SHAPES:
        for frames in (1, 2, 7, 120, 65535, 70000, 200000):
            g, p = flt.clip_launch_geometry(w, h, frames), flt.clip_batch_plan(w, h, frames)
            assert p["grid_x"] % 8 == 0 and 0 <= p["grid_x"] - g["nwg"] < 8, (name, w, h, frames)
            per = p["frames_per_batch"]
            assert 1 <= per <= 65535
            assert p["grid_x"] * min(per, frames) * 256 < 2 ** 31
            assert p["batches"] == -(-frames // per)
            # the largest batch the caps allow, not merely a legal one
            assert per == 65535 or p["grid_x"] * (per + 1) * 256 >= 2 ** 31


def test_shared_slot_where_the_frame_constants_do_not_read_time():
    """One frame-constant slot serves every frame exactly where the prologue reads neither t nor frame.  (Ident's does:
    its in(xy) is in(xy, t), and the frame number (int)t is a frame constant.)"""
    shared = {"mandelbrot": F.load("mandelbrot"), "select-0": mm.Filter(P.text(P.SELECT, "0"))}
    own = {"pond": F.load("pond"), "ident": F.load("ident"), "select-frame": mm.Filter(P.text(P.SELECT, "frame")), "wave": mm.Filter(WAVE)}
    for name, flt in shared.items():
        assert flt.clip_batch_plan(64, 64, 9)["shared_slot"] == 1, name
    for name, flt in own.items():
        assert flt.clip_batch_plan(64, 64, 9)["shared_slot"] == 0, name


def test_filters_with_native_calls_are_not_batched():
    for name in ("gauss_direct", "closure_timed_arg"):
        assert F.load(name).clip_batch_plan(64, 64, 3)["frames_per_batch"] == 0, name


def test_clip_max_frames_from_the_environment():
    """MMHIP_CLIP_MAX_FRAMES is read once per process: a child process each."""
    prog = ("import json, sys; sys.path.insert(0, %r); from tests import filters as F; f = F.load('ident'); "
            "print(json.dumps([f.clip_batch_plan(96, 64, n) for n in (1, 3, 7, 120)]))" % ROOT)
    for cap, want in (("3", [(1, 3), (1, 3), (3, 3), (40, 3)]), ("0", None), ("junk", None), ("100000", None)):
        env = dict(os.environ, MMHIP_CLIP_MAX_FRAMES=cap)
        out = subprocess.run([sys.executable, "-c", prog], env=env, check=True, capture_output=True, text=True).stdout
        plans = json.loads(out.strip().splitlines()[-1])
        if want is None:      # not a positive number, or above the grid's own limit: the default cap
            assert [p["frames_per_batch"] for p in plans] == [65535] * 4, cap
        else:
            assert [(p["batches"], p["frames_per_batch"]) for p in plans] == want, cap
