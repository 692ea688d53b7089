"""Grid-supersampled clips (mmhip_render_clip_sampled, mmhip_render_clip_sampled_fused) without a GPU: the entry points
and the header's statement of the semantics, the argument errors of both calls side by side, the delegation of the 1 x 1
grid, `aa` in Python and --aa on the command line, the offsets of csrc/mm_sample_grid.h (compiled for the host) against
the NumPy restatement of tests/sample_grid_reference.py, the arithmetic that cuts a clip into batches and passes, and the
sampled variant's text: its kernels, its gfx950 compile, and that asking for it leaves the other three texts alone."""
import ctypes as C
import hashlib
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import mathmap_amd as mm
from mathmap_amd._lib import lib
from tests import filters as F
from tests import sample_grid_reference as G
from tests import shutter_fused_probes as P
from tests import shutter_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "mathmap_amd", "mathmap_hip_cli")
W, H = P.W, P.H
f32 = np.float32
ROW_SLICE = ("wave", "extreme")          # probes with a per-row slice: no sampled variant, the maps path


def err():
    return lib().mmhip_last_error().decode()


def active(name, flt):
    return flt.specialized() if P.PROBES[name][1].get("specialize") else flt


# ---- entry points ----

def test_entry_points_exist_and_are_declared():
    header = open(os.path.join(ROOT, "include", "mmhip.h")).read()
    for name in ("mmhip_render_clip_sampled", "mmhip_filter_clip_sampled_plan", "mmhip_clip_sampled_batches",
                 "mmhip_render_clip_sampled_fused", "mmhip_filter_clip_sampled_fused_plan", "mmhip_clip_sampled_fused_batches",
                 "mmhip_filter_sampled_kernel_source", "mmhip_filter_jit_sampled"):
        assert hasattr(lib(), name), name
        assert re.search(r"\b%s\s*\(" % name, header), name
    from mathmap_amd.api import CLIP_SAMPLED_PLAN_FIELDS, SAMPLE_GRID_MAX
    assert CLIP_SAMPLED_PLAN_FIELDS == ("frames_per_batch", "batches", "steps_per_pass", "passes", "bytes_per_sample", "carry")
    assert re.search(r"MMHIP_CLIP_SAMPLED_PLAN_FIELDS\s*=\s*6\b", header) and re.search(r"MMHIP_CLIP_SAMPLED_FUSED_PLAN_FIELDS\s*=\s*5\b", header)
    assert re.search(r"MMHIP_SAMPLE_GRID_MAX\s*=\s*8\b", header) and SAMPLE_GRID_MAX == 8
    for attr in ("clip_sampled_plan", "clip_sampled_fused_plan", "sampled_kernel_source", "jit_sampled"):
        assert hasattr(mm.Filter, attr), attr
    for attr in ("clip_sampled_batches", "clip_sampled_fused_batches", "set_sampling_offset"):
        assert hasattr(mm.api.Invocation, attr), attr
    maps = re.search(r"int mmhip_render_clip_sampled\((.*?)\);", re.sub(r"\s+", " ", header)).group(1)
    fused = re.search(r"int mmhip_render_clip_sampled_fused\((.*?)\);", re.sub(r"\s+", " ", header)).group(1)
    assert maps == fused and lib().mmhip_render_clip_sampled_fused.argtypes == lib().mmhip_render_clip_sampled.argtypes


def test_the_header_states_the_semantics():
    header = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "mmhip.h")).read())
    for phrase in ("ox_a = (float)(((double)a + 0.5) / (double)sx - 0.5)",
                   "One point per axis is exactly 0",
                   "s = j * G + b * sx + a, a fastest",
                   "acc = f_0; acc = acc + f_s",
                   "inv_k = (float)(1.0 / (double)(K * G))",
                   "no fma",
                   "mm_shutter_sample_t(ts[i], span, j, K)",
                   "at sampling offset (ox_a, oy_b)",
                   "K * G is at most MMHIP_SHUTTER_MAX_SAMPLES (256)",
                   "put back on every return, failed calls included",
                   "Bytes between rows and between frames are not touched",
                   "grid_x = grid_y = 1 is mmhip_render_clip_shutter: the call delegates before anything else",
                   "grid_x = grid_y = 1 is mmhip_render_clip_shutter_fused",
                   "the layout [i][j][g]",
                   "steps_per_pass = max(1, (budget / bytes_per_sample - 1) / G)",
                   "G times per batch",
                   "without a per-row slice",
                   "shutter_combine_clip"):
        assert phrase in header, phrase


FRAMES2 = (C.c_int * 2)(0, 1)
TS2 = (C.c_float * 2)(0.0, 0.5)


def refused(fn, samples=2, span=0.1, gx=2, gy=2, num_frames=2, fr=FRAMES2, tt=TS2, row_stride=256, frame_stride=8192, bpp=4, w=64, h=32):
    """Checked before anything touches the invocation: a null one will do."""
    rc = fn(None, num_frames, fr, tt, samples, span, gx, gy, 0, 0, w, h, 0, h, None, row_stride, frame_stride, bpp, 0, None)
    assert rc != 0
    return err()


CASES = ([dict(gx=v) for v in (0, -1, 9)] + [dict(gy=v) for v in (0, -1, 9)] + [dict(samples=v) for v in (0, -1, 257)] +
         [dict(samples=65, gx=2, gy=2), dict(samples=5, gx=8, gy=8), dict(samples=129, gx=2, gy=1)] +
         [dict(span=v) for v in (float("nan"), float("inf"), float("-inf"))] + [dict(span=float("nan"), samples=1)] +
         [dict(num_frames=0), dict(num_frames=-3), dict(fr=None), dict(tt=None), dict(bpp=5), dict(bpp=0), dict(w=0), dict(h=0),
          dict(frame_stride=8191), dict(row_stride=300, frame_stride=31 * 300 + 255)])


def test_the_call_refuses_bad_arguments_with_a_message():
    fn = lib().mmhip_render_clip_sampled
    for v in (0, -1, 9):
        for axis in ("gx", "gy"):
            msg = refused(fn, **{axis: v})
            assert msg.startswith("render_clip_sampled: grid_x and grid_y must be 1 to 8") and str(v) in msg, msg
    for samples in (0, -1, 257):
        msg = refused(fn, samples=samples)
        assert "samples must be 1 to 256" in msg and str(samples) in msg, msg
    msg = refused(fn, samples=65, gx=2, gy=2)            # 260 sub-samples
    assert "samples * grid_x * grid_y" in msg and "256" in msg and "260" in msg, msg
    assert "257" not in refused(fn, samples=64, gx=2, gy=2, num_frames=0)       # 256 pass: the next check speaks
    assert "258" in refused(fn, samples=129, gx=2, gy=1)
    for span in (float("nan"), float("inf"), float("-inf")):
        assert refused(fn, span=span) == "render_clip_sampled: span must be finite"
    assert "span" in refused(fn, span=float("nan"), samples=1)                    # (NaN * 0 is NaN: refused with one instant too)
    assert "num_frames" in refused(fn, num_frames=0) and "frames and ts" in refused(fn, fr=None)
    assert "bpp" in refused(fn, bpp=5) and "empty region" in refused(fn, w=0)
    assert "frame_stride" in refused(fn, frame_stride=8191)


def test_the_fused_calls_messages_are_the_maps_calls_case_for_case():
    for case in CASES:
        maps = refused(lib().mmhip_render_clip_sampled, **case)
        fused = refused(lib().mmhip_render_clip_sampled_fused, **case)
        assert maps and fused == maps.replace("render_clip_sampled:", "render_clip_sampled_fused:"), (case, maps, fused)
    assert refused(lib().mmhip_render_clip_sampled_fused, gx=0).startswith("render_clip_sampled_fused: grid_x")


def test_the_1x1_grid_is_the_shutter_call_word_for_word():
    def shutter(fn, samples=4, span=0.1, num_frames=2, fr=FRAMES2, tt=TS2, row_stride=256, frame_stride=8192, bpp=4, w=64, h=32):
        rc = fn(None, num_frames, fr, tt, samples, span, 0, 0, w, h, 0, h, None, row_stride, frame_stride, bpp, 0, None)
        assert rc != 0
        return err()
    cases = [dict(samples=s) for s in (0, -1, 257)] + [dict(span=float("nan")), dict(span=float("inf"))]
    for samples in (4, 1):
        cases += [dict(samples=samples, num_frames=0), dict(samples=samples, fr=None), dict(samples=samples, bpp=5),
                  dict(samples=samples, w=0), dict(samples=samples, frame_stride=8191)]
    for case in cases:
        assert refused(lib().mmhip_render_clip_sampled, gx=1, gy=1, **dict(dict(samples=4), **case)) == \
            shutter(lib().mmhip_render_clip_shutter, **case), case
        assert refused(lib().mmhip_render_clip_sampled_fused, gx=1, gy=1, **dict(dict(samples=4), **case)) == \
            shutter(lib().mmhip_render_clip_shutter_fused, **case), case
    # one instant at one point is the plain clip: a NaN span is not looked at, the message is render_clip's
    assert refused(lib().mmhip_render_clip_sampled, gx=1, gy=1, samples=1, span=float("nan"), num_frames=0).startswith("render_clip:")


def test_plans_refuse_bad_arguments():
    flt, _ = P.compiled("pair")
    with pytest.raises(mm.MathMapError, match="num_frames"):
        flt.clip_sampled_plan(64, 64, 64, 2, 2, 0)
    with pytest.raises(mm.MathMapError, match="region"):
        flt.clip_sampled_plan(65, 64, 64, 2, 2, 3)
    with pytest.raises(mm.MathMapError, match="samples"):
        flt.clip_sampled_plan(64, 64, 64, 0, 2, 3)
    with pytest.raises(mm.MathMapError, match="samples \\* grid_x \\* grid_y"):
        flt.clip_sampled_plan(64, 64, 64, 5, 8, 3)
    with pytest.raises(mm.MathMapError, match="num_frames"):
        flt.clip_sampled_fused_plan(64, 64, 2, 2, 0)
    with pytest.raises(mm.MathMapError, match="region"):
        flt.clip_sampled_fused_plan(64, 0, 2, 2, 3)
    with pytest.raises(mm.MathMapError, match="samples \\* grid_x \\* grid_y"):
        flt.clip_sampled_fused_plan(64, 64, 129, (2, 1), 3)
    for aa in (0, 9, (2, 9), (0, 1), 2.0, "2", (1, 2, 3), None, True):
        with pytest.raises(ValueError, match="aa"):
            flt.clip_sampled_plan(64, 64, 64, 1, aa, 3)


# ---- aa in Python, --aa on the command line ----

def test_python_argument_errors():
    """Refused before anything else is looked at (an invocation needs a GPU; the checks do not, so an unbound one will do)."""
    inv = mm.api.Invocation.__new__(mm.api.Invocation)
    for aa in (0, -1, 9, (2, 9), (0, 2), (2,), (1, 2, 3), 2.5, "2", None):
        with pytest.raises(ValueError, match="aa"):
            inv.render_clip(num_frames=2, aa=aa)
    with pytest.raises(ValueError, match="256"):
        inv.render_clip(num_frames=2, aa=8, shutter_samples=5, shutter=0.5)
    with pytest.raises(ValueError, match="256"):
        inv.render_clip(num_frames=2, aa=(2, 1), shutter_samples=129, shutter=0.5)
    for mode in ("maps", "fused"):
        with pytest.raises(ValueError, match="aa is not combined with supersample"):
            inv.render_clip(num_frames=2, aa=2, supersample=True, shutter_mode=mode)
        with pytest.raises(ValueError, match="needs shutter"):                    # a shutter still needs its span
            inv.render_clip(num_frames=2, aa=2, shutter_samples=4, shutter_mode=mode)
    with pytest.raises(ValueError, match="shutter_mode"):
        inv.render_clip(num_frames=2, aa=2, shutter_mode="fast")
    # the rules of aa = 1 stand as they were
    with pytest.raises(ValueError, match="supersample=True is not combined with shutter_samples"):
        inv.render_clip(num_frames=2, aa=1, supersample=True, shutter_samples=4, shutter=0.5)
    from mathmap_amd.api import sample_grid
    assert sample_grid(3) == (3, 3) and sample_grid((2, 5)) == (2, 5) and sample_grid([8, 1]) == (8, 1) and sample_grid(np.int32(4)) == (4, 4)


def test_cli_help_and_argument_errors(tmp_path):
    p = subprocess.run([CLI, "--help"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=60)
    assert p.returncode == 0 and "--aa=N | SXxSY" in p.stdout and "--shutter-samples=K" in p.stdout
    src = "filter f () rgba:[t, 0, 0, 1] end"
    for extra, word in ((["--aa=0"], "--aa"), (["--aa=9"], "--aa"), (["--aa=2x"], "--aa"), (["--aa=x2"], "--aa"), (["--aa=2x9"], "--aa"),
                        (["--aa=2x2x2"], "--aa"), (["--aa="], "--aa"), (["--aa=two"], "--aa"), (["-o", "--aa=2"], "--aa"),
                        (["--aa=8", "--shutter-samples=5"], "256"), (["-o", "--shutter-samples=4", "--aa=2"], "-o")):
        p = subprocess.run([CLI, "-F", "3", "-s", "8x8"] + extra + [src, str(tmp_path / "f%d.png")], stdout=subprocess.PIPE,
                           stderr=subprocess.PIPE, text=True, timeout=60)
        assert p.returncode != 0 and word in p.stderr, (extra, p.stderr)
    assert not list(tmp_path.iterdir())


# ---- the offsets, compiled for the host ----

OFFSETS = r'''
#include <stdio.h>
#include "mm_sample_grid.h"

/* for every n in 1 .. MM_SAMPLE_GRID_MAX: the n offsets; then the index of every (j, b, a) of a 3 x sx x sy grid */
int main(int argc, char **argv) {
    if (argc != 4) return 2;
    FILE *out = fopen(argv[1], "wb");
    if (!out) return 2;
    for (int n = 1; n <= MM_SAMPLE_GRID_MAX; ++n)
        for (int a = 0; a < n; ++a) {
            const float o = mm_sample_grid_offset(a, n);
            if (fwrite(&o, sizeof o, 1, out) != 1) return 4;
        }
    int sx = 0, sy = 0;
    if (sscanf(argv[2], "%d", &sx) != 1 || sscanf(argv[3], "%d", &sy) != 1) return 2;
    for (int j = 0; j < 3; ++j)
        for (int b = 0; b < sy; ++b)
            for (int a = 0; a < sx; ++a) {
                const int s = mm_sample_grid_index(j, b, a, sx, sy);
                if (fwrite(&s, sizeof s, 1, out) != 1) return 4;
            }
    return fclose(out) != 0;
}
'''


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "sanitizers"])
def test_header_offsets_are_the_restatement(sanitize):
    """A stand-alone host program over the header the runtime includes; once under the address and undefined-behaviour
    sanitizers (host code only)."""
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    d = tempfile.mkdtemp(prefix="mm_grid_")
    try:
        open(os.path.join(d, "t.cpp"), "w").write(OFFSETS)
        flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else ["-O2"]
        exe = os.path.join(d, "t")
        subprocess.run([cxx, "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off"] + flags +
                       ["-I", os.path.join(ROOT, "mathmap_amd", "csrc"), "-o", exe, os.path.join(d, "t.cpp")], check=True)
        sx, sy = 3, 2
        r = subprocess.run([exe, os.path.join(d, "out.bin"), str(sx), str(sy)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
        raw = np.fromfile(os.path.join(d, "out.bin"), np.uint8)
    finally:
        shutil.rmtree(d, ignore_errors=True)
    at = 0
    for n in range(1, 9):
        got = raw[at:at + 4 * n].copy().view(f32)
        at += 4 * n
        want = G.offsets(n)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), n
        # the centres of n equal cells of the footprint: symmetric, inside it, 1 / n apart
        assert np.allclose(want, (np.arange(n) + 0.5) / n - 0.5, atol=1e-7) and abs(want).max() < 0.5
        assert np.array_equal(want, -want[::-1])
    assert G.offsets(1)[0] == 0 and G.offsets(2).tolist() == [-0.25, 0.25] and G.offsets(4).tolist() == [-0.375, -0.125, 0.125, 0.375]
    index = raw[at:].copy().view(np.int32)
    assert index.tolist() == list(range(3 * sx * sy))          # the program's loop nest is the restatement's order
    assert G.order(3, sx, sy)[7] == (1, 0, 1)
    runtime = open(os.path.join(ROOT, "mathmap_amd", "csrc", "runtime_clip.cpp")).read()
    assert '#include "mm_sample_grid.h"' in runtime and runtime.count("mm_sample_grid_offset(") >= 4


def test_the_restatements_order_and_mean():
    maps = np.arange(2 * 2 * 3 * 4, dtype=f32).reshape(2, 2, 3, 1, 4)          # [K, sy, sx, 1 pixel, 4]
    flat = maps.reshape(12, 1, 4)                                                # C order is j, b, a with a fastest
    assert R.same_floats(G.combine(maps, floatmap=True), R.mean(flat))
    assert G.grid(3) == (3, 3) and G.grid((2, 5)) == (2, 5)


# ---- plan arithmetic (MMHIP_CLIP_SHUTTER_BYTES is read once per process: a child process each) ----

def test_plan_with_the_default_budget():
    flt = F.load("ident")
    for w, rows, rw, k, aa, n in ((97, 61, 97, 1, 2, 3), (50, 20, 97, 4, (2, 3), 120), (1920, 1080, 1920, 4, 2, 8), (8192, 8192, 8192, 1, 2, 5),
                                  (1, 1, 1, 4, 8, 70000)):
        sx, sy = G.grid(aa)
        p = flt.clip_sampled_plan(w, rows, rw, k, aa, n)
        bps = rows * 16 * rw
        per = min((8 << 30) // (k * sx * sy * bps), 65535, n)
        assert per >= 1
        assert p == dict(frames_per_batch=per, batches=-(-n // per), steps_per_pass=k, passes=1, bytes_per_sample=bps, carry=0), (w, rows, k, aa, n, p)
    assert flt.clip_sampled_plan(8192, 8192, 8192, 1, 2, 5)["frames_per_batch"] == 2       # 4 GiB of maps per frame
    # 8192^2 at aa = 2 with K = 4: 16 GiB per frame -- one frame per batch, (8 - 1) / 4 = 1 time step per pass
    assert flt.clip_sampled_plan(8192, 8192, 8192, 4, 2, 1) == dict(frames_per_batch=1, batches=1, steps_per_pass=1, passes=4,
                                                                    bytes_per_sample=1 << 30, carry=1)


def test_plan_under_a_budget_from_the_environment():
    bps = 61 * 16 * 97
    prog = ("import json, sys; sys.path.insert(0, %r); from tests import filters as F; f = F.load('ident'); "
            "print(json.dumps([f.clip_sampled_plan(97, 61, 97, k, aa, n) for k, aa, n in ((1, (2, 2), 7), (3, (2, 1), 7), (5, (2, 2), 3), (1, (8, 8), 2))]))" % ROOT)

    def key(p):
        assert p["bytes_per_sample"] == bps
        return (p["frames_per_batch"], p["batches"], p["steps_per_pass"], p["passes"], p["carry"])

    cases = [
        # many frames per batch: 12 maps fit -- 3 frames of 4, 2 of 6; 20 and 64 do not: (12 - 1) / 4 = 2 steps per pass, and
        # for one step of 64 maps the soft minimum, one pass without a carry
        (12 * bps + 100, [(3, 3, 1, 1, 0), (2, 4, 3, 1, 0), (1, 3, 2, 3, 1), (1, 2, 1, 1, 0)]),
        # exactly one frame of 6: one of 4 too; 20 maps go in passes of (6 - 1) / 4 = 1 step
        (6 * bps, [(1, 7, 1, 1, 0), (1, 7, 3, 1, 0), (1, 3, 1, 5, 1), (1, 2, 1, 1, 0)]),
        # one byte short of it: 3 steps of 2 maps become (5 - 1) / 2 = 2 per pass, whole time steps only
        (6 * bps - 1, [(1, 7, 1, 1, 0), (1, 7, 2, 2, 1), (1, 3, 1, 5, 1), (1, 2, 1, 1, 0)]),
        # the soft minimum: less than one time step beside the carry -- one step per pass all the same
        (3 * bps, [(1, 7, 1, 1, 0), (1, 7, 1, 3, 1), (1, 3, 1, 5, 1), (1, 2, 1, 1, 0)]),
        (1, [(1, 7, 1, 1, 0), (1, 7, 1, 3, 1), (1, 3, 1, 5, 1), (1, 2, 1, 1, 0)]),
        # not a positive number: the default
        ("junk", [(7, 1, 1, 1, 0), (7, 1, 3, 1, 0), (3, 1, 5, 1, 0), (2, 1, 1, 1, 0)]),
    ]
    for budget, want in cases:
        env = dict(os.environ, MMHIP_CLIP_SHUTTER_BYTES=str(budget))
        out = subprocess.run([sys.executable, "-c", prog], env=env, check=True, capture_output=True, text=True).stdout
        plans = json.loads(out.strip().splitlines()[-1])
        assert [key(p) for p in plans] == want, budget


def test_fused_plans_worked_out_by_hand():
    flt, _ = P.compiled("pair")
    # the fused shutter's plan: K slots per frame, whatever the grid
    for aa in (2, (1, 8), (8, 8)):
        assert flt.clip_sampled_fused_plan(W, H, 1, aa, 3) == dict(fused=1, frames_per_batch=3, batches=1, slots_per_batch=3, grid_x=32)
    assert flt.clip_sampled_fused_plan(W, H, 3, 2, 3) == flt.clip_shutter_fused_plan(W, H, 3, 3)
    # K * G = 256 is taken: 16 slots per frame, 65 535 / 16 frames per launch
    assert flt.clip_sampled_fused_plan(17, 17, 16, (4, 4), 5000) == dict(fused=1, frames_per_batch=4095, batches=2, slots_per_batch=4095 * 16, grid_x=8)
    assert flt.clip_sampled_fused_plan(17, 17, 4, (8, 8), 2)["fused"] == 1
    # the 1 x 1 grid is the fused shutter's plan itself
    assert flt.clip_sampled_fused_plan(W, H, 4, 1, 3) == flt.clip_shutter_fused_plan(W, H, 4, 3)
    # one slot for the whole call where the frame constants read neither t nor frame
    shared, _ = P.compiled("shared")
    assert shared.clip_sampled_fused_plan(W, H, 4, 2, 3) == dict(fused=1, frames_per_batch=3, batches=1, slots_per_batch=1, grid_x=32)


@pytest.mark.parametrize("name", list(P.FALLBACKS) + list(ROW_SLICE))
def test_filters_that_are_not_fused(name):
    """Native calls and closure images, as for the shutter -- and the rule chosen for the per-row slice: its values follow
    y, so a filter that has one takes the maps path whatever the grid (its 1 x 1 grid is the fused shutter)."""
    flt, _ = P.compiled(name)
    if name in ROW_SLICE:
        assert "mm_rows(" in flt.kernel_source and flt.num_native_calls == 0
        assert flt.clip_shutter_fused_plan(W, H, 4, 3)["fused"] == 1 and flt.clip_sampled_fused_plan(W, H, 4, 1, 3)["fused"] == 1
    else:
        assert flt.num_native_calls > 0
    for aa in (2, (2, 1), (1, 2)):
        plan = flt.clip_sampled_fused_plan(W, H, 4, aa, 3)
        assert (plan["fused"], plan["frames_per_batch"], plan["batches"], plan["slots_per_batch"]) == (0, 0, 0, 0), (name, aa)
    with pytest.raises(mm.MathMapError, match="no sampled variant"):
        flt.sampled_kernel_source
    with pytest.raises(mm.MathMapError, match="no sampled variant"):
        flt.jit_sampled()
    assert flt.clip_sampled_plan(W, H, W, 4, 2, 3)["frames_per_batch"] == 3          # the maps path takes every filter


# ---- the sampled variant's text ----

def kernel_names(text):
    return re.findall(r'extern "C" __global__ void __launch_bounds__\(256\) (\w+)\(', text)


@pytest.mark.parametrize("name", list(P.PROBES))
def test_the_sampled_text_of_every_probe(name):
    flt = active(name, P.compiled(name)[0])
    before = (flt.kernel_source, flt.clip_kernel_source, flt.shutter_kernel_source)
    if name in ROW_SLICE:
        with pytest.raises(mm.MathMapError, match="per-row slice"):
            flt.sampled_kernel_source
        assert (flt.kernel_source, flt.clip_kernel_source, flt.shutter_kernel_source) == before
        return
    text = flt.sampled_kernel_source
    assert kernel_names(text) == ["mm_prologue_clip", "mm_pixels_sampled"]
    assert "struct mm_sampled { const float *offs; float *xtabs; float *ytabs; int samples; int gx; int gy; int total; float inv_k; int pad; };" in text
    assert "#define MM_UNROLL 1\n" in text and "struct mm_shutter" not in text
    pro = text[text.index("mm_prologue_clip("):text.index("mm_pixels_sampled(")]
    assert "mm_prologue_clip(mm_args A, char *XY, const mm_clip C, const mm_sampled S)" in pro
    # the tables are the expressions of every prologue, at the grid's offsets
    assert "S.xtabs[mm_a * A.region_width + gid] = CALC_VIRTUAL_X(gid + A.region_x, A.frame_render_width, S.offs[mm_a]);" in pro
    assert "S.ytabs[mm_b * A.num_rows + gid] = CALC_VIRTUAL_Y(A.first_row + gid, A.frame_render_height, S.offs[MM_SAMPLE_GRID_MAX + mm_b]);" in pro
    body = text[text.index("mm_pixels_sampled("):]
    assert "#pragma unroll 1\n  for (int mm_s = 0; mm_s < S.total; ++mm_s) {" in body
    assert "const float x = mm_xt[mm_xo];" in body and "const float y = mm_yt[mm_yo];" in body
    assert "long long mm_slot = (long long)fi * S.samples;" in body and "* S.inv_k;" in body
    loop = body[body.index("for (int mm_s"):]
    code = re.sub(r"//[^\n]*", "", loop)
    assert "CALC_VIRTUAL" not in code and not re.search(r"mm_s\s*[/%]", code)          # counters: no division decodes s, no f64 division per sub-sample
    assert body.count("mm_store_pixel(") == 1 and "_hot" not in body and "mm_pair" not in body
    # the pixel code between the heads is the shutter variant's, statement for statement
    shutter = before[2]
    ours = loop[loop.index("    MM_INTERNALS\n"):loop.index("    if (mm_s == 0) mm_acc = rt;")].replace("(void)XY; (void)x; (void)y; (void)mm_rand_ctr;", "(void)XY; (void)mm_rand_ctr;")
    theirs = shutter[shutter.index("    MM_INTERNALS\n", shutter.index("mm_pixels_shutter(")):shutter.index("    if (mm_j == 0) mm_acc = rt;")]
    assert ours == theirs
    assert flt.jit_sampled(load=False) > 0
    assert flt.sampled_kernel_source == text
    # asking for it, and compiling it, left the other texts alone: they are a fresh filter's
    fresh = active(name, P.compiled(name)[0])
    assert (flt.kernel_source, flt.clip_kernel_source, flt.shutter_kernel_source) == before
    assert before == (fresh.kernel_source, fresh.clip_kernel_source, fresh.shutter_kernel_source)
    assert fresh.sampled_kernel_source == text


def test_pinned_kernel_texts_keep_their_digests_around_the_variant():
    with open(os.path.join(ROOT, "tests", "golden", "clip_text_digests.json")) as f:
        want = json.load(f)["filters"]
    asked = 0
    for name, digests in want.items():
        flt = F.load(name)
        try:
            flt.sampled_kernel_source
            asked += 1
        except mm.MathMapError as e:
            assert "no sampled variant" in str(e)
        assert hashlib.sha256(flt.clip_kernel_source.encode()).hexdigest() == digests["clip_kernel_source_sha256"], name
        assert hashlib.sha256(flt.kernel_source.encode()).hexdigest() == digests["kernel_source_sha256"], name
    assert asked > 0
    from tools.kernel_body_digest import digests as body_digests
    with open(os.path.join(ROOT, "tests", "golden", "kernel_body_digests.json")) as f:
        assert body_digests() == json.load(f)["body_sha256"]
