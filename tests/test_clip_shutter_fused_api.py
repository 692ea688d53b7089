"""Fused motion blur (mmhip_render_clip_shutter_fused, mm_pixels_shutter) without a GPU: the entry points, the argument
errors beside mmhip_render_clip_shutter's, shutter_mode in Python and on the command line, the arithmetic that cuts a clip
into batches, and the shutter variant's text: its kernels, its gfx950 compile, and that asking for it leaves the other two
texts alone."""
import ctypes as C
import json
import os
import re
import subprocess
import sys

import pytest

import mathmap_amd as mm
from mathmap_amd._lib import lib
from tests import shutter_fused_probes as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "mathmap_amd", "mathmap_hip_cli")
W, H = P.W, P.H


def err():
    return lib().mmhip_last_error().decode()


def active(name, flt):
    """The variant a render of the probe runs: the specialised one where the probe is compiled with specialize=True."""
    return flt.specialized() if P.PROBES[name][1].get("specialize") else flt


# ---- entry points ----

def test_entry_points_exist_and_are_declared():
    header = open(os.path.join(ROOT, "include", "mmhip.h")).read()
    for name in ("mmhip_render_clip_shutter_fused", "mmhip_filter_clip_shutter_fused_plan", "mmhip_clip_shutter_fused_batches",
                 "mmhip_filter_shutter_kernel_source", "mmhip_filter_jit_shutter"):
        assert hasattr(lib(), name), name
        assert re.search(r"\b%s\s*\(" % name, header), name
    from mathmap_amd.api import CLIP_SHUTTER_FUSED_PLAN_FIELDS
    assert CLIP_SHUTTER_FUSED_PLAN_FIELDS == ("fused", "frames_per_batch", "batches", "slots_per_batch", "grid_x")
    assert re.search(r"MMHIP_CLIP_SHUTTER_FUSED_PLAN_FIELDS\s*=\s*5\b", header)
    for attr in ("clip_shutter_fused_plan", "shutter_kernel_source", "jit_shutter"):
        assert hasattr(mm.Filter, attr), attr
    assert hasattr(mm.api.Invocation, "clip_shutter_fused_batches")


def test_the_fused_call_has_the_parameters_of_the_maps_call():
    header = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "mmhip.h")).read())
    maps = re.search(r"int mmhip_render_clip_shutter\((.*?)\);", header).group(1)
    fused = re.search(r"int mmhip_render_clip_shutter_fused\((.*?)\);", header).group(1)
    assert maps == fused
    assert lib().mmhip_render_clip_shutter_fused.argtypes == lib().mmhip_render_clip_shutter.argtypes


def test_argument_errors_are_the_maps_calls_case_for_case():
    """Checked before anything touches the invocation: a null one will do."""
    frames = (C.c_int * 2)(0, 1)
    ts = (C.c_float * 2)(0.0, 0.5)

    def refused(fn, samples=4, span=0.1, num_frames=2, fr=frames, tt=ts, row_stride=256, frame_stride=8192, bpp=4, w=64, h=32):
        rc = fn(None, num_frames, fr, tt, samples, span, 0, 0, w, h, 0, h, None, row_stride, frame_stride, bpp, 0, None)
        assert rc != 0
        return err()

    cases = [dict(samples=s) for s in (0, -1, 257)] + [dict(span=s) for s in (float("nan"), float("inf"), float("-inf"))]
    for samples in (4, 1):
        cases += [dict(samples=samples, num_frames=0), dict(samples=samples, num_frames=-3), dict(samples=samples, fr=None),
                  dict(samples=samples, tt=None), dict(samples=samples, bpp=5), dict(samples=samples, bpp=0),
                  dict(samples=samples, w=0), dict(samples=samples, h=0), dict(samples=samples, frame_stride=8191),
                  dict(samples=samples, row_stride=300, frame_stride=31 * 300 + 255)]
    for case in cases:
        maps = refused(lib().mmhip_render_clip_shutter, **case)
        fused = refused(lib().mmhip_render_clip_shutter_fused, **case)
        assert maps and fused == maps.replace("render_clip_shutter:", "render_clip_shutter_fused:"), (case, maps, fused)
    assert refused(lib().mmhip_render_clip_shutter_fused, samples=0).startswith("render_clip_shutter_fused: samples")


def test_plan_refuses_bad_arguments():
    flt, _ = P.compiled("pair")
    with pytest.raises(mm.MathMapError, match="num_frames"):
        flt.clip_shutter_fused_plan(64, 64, 4, 0)
    with pytest.raises(mm.MathMapError, match="region"):
        flt.clip_shutter_fused_plan(0, 64, 4, 3)
    with pytest.raises(mm.MathMapError, match="region"):
        flt.clip_shutter_fused_plan(64, 0, 4, 3)
    for samples in (0, -1, 257):
        with pytest.raises(mm.MathMapError, match="samples"):
            flt.clip_shutter_fused_plan(64, 64, samples, 3)


# ---- shutter_mode ----

def test_python_shutter_mode():
    """Refused before anything else is looked at (an invocation needs a GPU; the checks do not, so an unbound one will do)."""
    inv = mm.api.Invocation.__new__(mm.api.Invocation)
    for mode in ("fuse", "", None, "MAPS", 1):
        with pytest.raises(ValueError, match="shutter_mode"):
            inv.render_clip(num_frames=2, shutter_samples=4, shutter=0.5, shutter_mode=mode)
    # the other rules stand under either mode
    for mode in ("maps", "fused"):
        with pytest.raises(ValueError, match="supersample"):
            inv.render_clip(num_frames=2, supersample=True, shutter_samples=4, shutter=0.5, shutter_mode=mode)
        with pytest.raises(ValueError, match="not both"):
            inv.render_clip(num_frames=2, shutter_samples=4, shutter=0.5, shutter_span=0.1, shutter_mode=mode)
        with pytest.raises(ValueError, match="shutter is a fraction"):
            inv.render_clip(frames=[0, 1], ts=[0.0, 0.5], shutter_samples=4, shutter=0.5, shutter_mode=mode)
        with pytest.raises(ValueError, match="needs shutter"):
            inv.render_clip(num_frames=2, shutter_samples=4, shutter_mode=mode)


def test_cli_shutter_mode(tmp_path):
    p = subprocess.run([CLI, "--help"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=60)
    assert p.returncode == 0 and "--shutter-mode=MODE" in p.stdout
    src = "filter f () rgba:[t, 0, 0, 1] end"
    for extra, word in ((["--shutter-samples=4", "--shutter-mode=fast"], "--shutter-mode"), (["--shutter-mode="], "--shutter-mode"),
                        (["-o", "--shutter-samples=4", "--shutter-mode=fused"], "-o")):
        p = subprocess.run([CLI, "-F", "3", "-s", "8x8"] + extra + [src, str(tmp_path / "f%d.png")], stdout=subprocess.PIPE,
                           stderr=subprocess.PIPE, text=True, timeout=60)
        assert p.returncode != 0 and word in p.stderr, (extra, p.stderr)
    assert not list(tmp_path.iterdir())


# ---- plan arithmetic ----

def test_plans_worked_out_by_hand():
    flt, _ = P.compiled("pair")
    # 97 x 61 in 16 x 16 tiles: 7 x 4 = 28 workgroups, 32 with the padding; nothing but the clip's length bounds the batch
    assert flt.clip_shutter_fused_plan(W, H, 4, 3) == dict(fused=1, frames_per_batch=3, batches=1, slots_per_batch=12, grid_x=32)
    # 65 535 grid rows of the prologue: 255 frames of 256 sub-samples, 16 383 of 4, 21 845 of 3
    assert flt.clip_shutter_fused_plan(17, 17, 256, 300) == dict(fused=1, frames_per_batch=255, batches=2, slots_per_batch=255 * 256, grid_x=8)
    assert flt.clip_shutter_fused_plan(17, 17, 256, 255)["batches"] == 1
    assert flt.clip_shutter_fused_plan(17, 17, 4, 70000)["frames_per_batch"] == 65535 // 4
    assert flt.clip_shutter_fused_plan(17, 17, 3, 70000) == dict(fused=1, frames_per_batch=21845, batches=4, slots_per_batch=65535, grid_x=8)
    # 8192^2: 512 x 512 workgroups; 2^31 work-items are 2^23 workgroups of 256: 31 frames (32 would be 2^31 exactly)
    assert flt.clip_shutter_fused_plan(8192, 8192, 4, 100) == dict(fused=1, frames_per_batch=31, batches=4, slots_per_batch=124, grid_x=512 * 512)
    # 16384 x 16385: 1024 x 1025 workgroups, 7 frames
    assert flt.clip_shutter_fused_plan(16384, 16385, 2, 1) == dict(fused=1, frames_per_batch=1, batches=1, slots_per_batch=2, grid_x=1024 * 1025)
    assert flt.clip_shutter_fused_plan(16384, 16385, 2, 9)["frames_per_batch"] == (2 ** 23 - 1) // (1024 * 1025) == 7
    # the geometry is the single-pixel one whatever the filter's own kernel is: pair mode here, two rows per step
    assert flt.launch_geometry(W, H)["pair_mode"] == 1 and flt.launch_geometry(8192, 8192)["ppt"] > 1


def test_the_row_tables_of_a_batch_stay_below_2_31_floats():
    flt, _ = P.compiled("wave")             # two row values: a slot's row table is 2 * num_rows floats
    text = flt.shutter_kernel_source
    assert "mm_rows_clip" in text and "A.rowtab[1 * A.num_rows + rl] =" in text and "A.rowtab[2 * A.num_rows + rl] =" not in text
    assert (flt.launch_geometry(W, H)["tile_w"], flt.launch_geometry(W, H)["tile_h"]) == (64, 4)
    rows = 1000000
    # a column of 10^6 rows in tiles of 4 rows: 250 000 workgroups, 33 frames by work-items, 255 by grid rows -- and 256
    # row tables of 2 * 10^6 floats per frame: 4 frames are 2.048 * 10^9 floats, 5 would be beyond INT32_MAX
    assert flt.clip_shutter_fused_plan(1, rows, 256, 20) == dict(fused=1, frames_per_batch=4, batches=5, slots_per_batch=4 * 256, grid_x=250000)
    assert (2 ** 31 - 1) // (256 * 2 * rows) == 4 and (2 ** 23 - 1) // 250000 == 33
    # the shared-slot probe keeps one table whatever the batch: the bound does not apply
    shared, _ = P.compiled("shared")
    assert shared.clip_batch_plan(W, H, 3)["shared_slot"] == 1
    assert shared.clip_shutter_fused_plan(W, H, 4, 3) == dict(fused=1, frames_per_batch=3, batches=1, slots_per_batch=1, grid_x=32)
    assert shared.clip_shutter_fused_plan(1, rows, 256, 20)["frames_per_batch"] == 20


def test_plan_under_a_frame_cap_from_the_environment():
    """MMHIP_CLIP_MAX_FRAMES is read once: a child process."""
    prog = ("import json, sys; sys.path.insert(0, %r); from tests import shutter_fused_probes as P; f, _ = P.compiled('pair'); "
            "print(json.dumps([f.clip_shutter_fused_plan(97, 61, k, n) for k, n in ((3, 5), (8, 5), (9, 5), (2, 3))]))" % ROOT)
    env = dict(os.environ, MMHIP_CLIP_MAX_FRAMES="8")
    out = subprocess.run([sys.executable, "-c", prog], env=env, check=True, capture_output=True, text=True).stdout
    plans = json.loads(out.strip().splitlines()[-1])
    assert plans[0] == dict(fused=1, frames_per_batch=2, batches=3, slots_per_batch=6, grid_x=32)
    assert plans[1] == dict(fused=1, frames_per_batch=1, batches=5, slots_per_batch=8, grid_x=32)
    assert plans[2] == dict(fused=0, frames_per_batch=0, batches=0, slots_per_batch=0, grid_x=32)      # not one frame: the maps path
    assert plans[3] == dict(fused=1, frames_per_batch=3, batches=1, slots_per_batch=6, grid_x=32)


@pytest.mark.parametrize("name", list(P.FALLBACKS))
def test_filters_with_native_calls_or_closures_are_not_fused(name):
    flt, _ = P.compiled(name)
    assert flt.num_native_calls > 0
    assert (name == "closure") == (flt.num_closures > 0)
    plan = flt.clip_shutter_fused_plan(W, H, 4, 3)
    assert (plan["fused"], plan["frames_per_batch"], plan["batches"], plan["slots_per_batch"]) == (0, 0, 0, 0)
    with pytest.raises(mm.MathMapError, match="no shutter variant"):
        flt.shutter_kernel_source
    with pytest.raises(mm.MathMapError, match="no shutter variant"):
        flt.jit_shutter()


# ---- the shutter variant's text ----

def kernel_names(text):
    return re.findall(r'extern "C" __global__ void __launch_bounds__\(256\) (\w+)\(', text)


@pytest.mark.parametrize("name", list(P.PROBES))
def test_the_shutter_text_of_every_probe(name):
    flt, _ = P.compiled(name)
    flt = active(name, flt)
    before = (flt.kernel_source, flt.clip_kernel_source)
    text = flt.shutter_kernel_source
    rows = "mm_rows(" in before[0]
    assert kernel_names(text) == ["mm_prologue_clip"] + (["mm_rows_clip"] if rows else []) + ["mm_pixels_shutter"]
    assert rows == (name in ("wave", "extreme"))          # (extreme's exp(900 * (y - t)) is a row value too)
    assert "struct mm_shutter { int samples; float inv_k; };" in text and "#define MM_UNROLL 1\n" in text
    body = text[text.index("mm_pixels_shutter("):]
    assert "#pragma unroll 1\n  for (int mm_j = 0; mm_j < S.samples; ++mm_j) {" in body
    assert "(long long)fi * S.samples + mm_j" in body and "* S.inv_k;" in body
    assert body.count("mm_store_pixel(") == 1 and "_hot" not in body and "mm_pair" not in body
    # the prologue and the per-row slice are the clip variant's, head and body
    clip = before[1]
    assert text[text.index("struct mm_clip_frame"):text.index("struct mm_shutter")] == \
        clip[clip.index("struct mm_clip_frame"):clip.index('extern "C" __global__ void __launch_bounds__(256) mm_pixels_clip(')]
    assert flt.jit_shutter(load=False) > 0
    assert flt.shutter_kernel_source == text
    # asking for it, and compiling it, left the other texts alone: they are a fresh filter's
    fresh = active(name, P.compiled(name)[0])
    assert (flt.kernel_source, flt.clip_kernel_source) == before == (fresh.kernel_source, fresh.clip_kernel_source)
    assert fresh.shutter_kernel_source == text


def test_the_pair_probe_is_a_pair_mode_kernel_and_the_others_cover_the_shapes():
    shapes = {}
    for name in P.PROBES:
        flt = active(name, P.compiled(name)[0])
        g = flt.launch_geometry(W, H)
        shapes[name] = (g["pair_mode"], g["single_pixel"], g["unroll"])
    assert shapes["pair"][0] == 1 and shapes["mandelbrot"][0] == 1
    assert shapes["droste"][1] == 1
    assert shapes["sequence"][2] > 1 and shapes["wave"][2] > 1          # the unrolled loop with the hot fetch
