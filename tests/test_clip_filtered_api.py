"""Filtered clips without a GPU (mmhip_render_clip_filtered, include/mmhip.h): the entry points and the header's
statement, the tap tables of mmhip_clip_filter_taps against tests/clip_filter_reference.py bit for bit, the two sums of
csrc/mm_clip_filter.h compiled for the host on a frame worked out by hand, the plan's arithmetic, every refusal by its
message, `aa_filter` in Python and --aa-filter on the command line."""
import ctypes as C
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
from tests import clip_filter_reference as X
from tests import filters as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "mathmap_amd", "mathmap_hip_cli")
f32, f64 = np.float32, np.float64
RADII = (0.5, 1.0, 1.5, 2.0, 2.5, 4.0)
POINTS = (1, 2, 3, 4, 8)


def err():
    return lib().mmhip_last_error().decode()


# ---- entry points and the statement ----

def test_entry_points_exist_and_are_declared():
    header = open(os.path.join(ROOT, "include", "mmhip.h")).read()
    for name in ("mmhip_render_clip_filtered", "mmhip_clip_filtered_batches", "mmhip_filter_clip_filtered_plan", "mmhip_clip_filter_taps"):
        assert hasattr(lib(), name), name
        assert re.search(r"\b%s\s*\(" % name, header), name
    for k, name in enumerate(("MMHIP_AA_BOX", "MMHIP_AA_TENT", "MMHIP_AA_GAUSSIAN", "MMHIP_AA_MITCHELL")):
        assert re.search(r"%s\s*=\s*%d\b" % (name, k), header), name
    assert re.search(r"MMHIP_CLIP_FILTERED_PLAN_FIELDS\s*=\s*8\b", header)
    from mathmap_amd import api
    assert api.CLIP_FILTERED_PLAN_FIELDS == api.CLIP_SAMPLED_PLAN_FIELDS + ("halo_columns", "halo_rows")
    assert api.AA_FILTERS == X.KERNELS and api.AA_FILTER_RADII == X.DEFAULT_RADII
    assert hasattr(mm.Filter, "clip_filtered_plan") and hasattr(api.Invocation, "clip_filtered_batches") and hasattr(api, "clip_filter_taps")
    # every parameter but kernel and radius is the sampled call's, in its place
    flat = re.sub(r"\s+", " ", header)
    sampled = re.search(r"int mmhip_render_clip_sampled\((.*?)\);", flat).group(1)
    filtered = re.search(r"int mmhip_render_clip_filtered\((.*?)\);", flat).group(1)
    assert filtered.replace("int grid_y, int kernel, float radius,", "int grid_y,") == sampled
    types = list(lib().mmhip_render_clip_sampled.argtypes)
    assert lib().mmhip_render_clip_filtered.argtypes == types[:8] + [C.c_int, C.c_float] + types[8:]
    from mathmap_amd._lib import SELFTEST_SYMBOLS
    assert "mmhip_selftest_filter_combine" in SELFTEST_SYMBOLS
    csrc = os.path.join(ROOT, "mathmap_amd", "csrc")
    assert "k_filter_combine_clip" in open(os.path.join(csrc, "clip_combine.hip")).read()
    assert "launch_filter_combine_clip" in open(os.path.join(csrc, "clip_kernels.h")).read()
    for text in (open(os.path.join(csrc, "clip_combine.hip")).read(), open(os.path.join(csrc, "runtime_clip.cpp")).read()):
        assert '#include "mm_clip_filter.h"' in text


def test_the_header_states_the_semantics():
    header = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "mmhip.h")).read())
    for phrase in ("0.5 <= radius <= 4",
                   "box 0.5, tent 1.0, Gaussian 1.5, Mitchell 2.0",
                   "D = (int)ceil(radius - 0.5)",
                   "d_x = (double)dx + (double)ox_a and d_y = (double)dy + (double)oy_b",
                   "tent: 1.0 - ad / R",
                   "Gaussian: exp(-2.0 * (d * d)) - exp(-2.0 * (R * R))",
                   "u = (2.0 * ad) / R",
                   "(((7.0 * u - 12.0) * u) * u + 16.0 / 3.0) / 6.0",
                   "((((-7.0 / 3.0) * u + 12.0) * u - 20.0) * u + 32.0 / 3.0) / 6.0",
                   "dx ascending, then a ascending",
                   "0 <= region_x + c + dx < render_width",
                   "The frame counts, not the region and not the rows asked for",
                   "w = (float)(k / n)",
                   "A tap with w == 0 is dropped: it is never read, whatever it holds",
                   "at most (D + 1)^2 tables per axis",
                   "each product rounded on its own; the first product starts the sum",
                   "acc = s_0; acc = acc + s_j for j = 1 .. K - 1; m = acc * (float)(1.0 / (double)K)",
                   "no fma, denormals kept",
                   "A 1 x 1 grid is allowed",
                   "Nothing delegates to another entry point",
                   "the association of the sum differs",
                   "[max(0, region_x - D), min(render_width, region_x + region_w + D))",
                   "[max(0, first_row - D), min(render_height, last_row + D))",
                   "the carry map holds the running acc of the output rectangle",
                   "put back on every return, failed calls included",
                   "One upload of the tap tables per call, one combine launch per pass",
                   "filter_combine_clip",
                   "a sub-sample map of the haloed rectangle beyond 4 GiB"):
        assert phrase in header, phrase


# ---- the tap tables ----

def library_taps(kernel, radius, n, lo, hi):
    out = np.full(9 * 8 + 4, 7.0, f32)
    got = lib().mmhip_clip_filter_taps(kernel, radius, n, lo, hi, out.ctypes.data_as(C.POINTER(C.c_float)))
    assert got == (2 * X.reach(radius) + 1) * n, (kernel, radius, n, lo, hi, err())
    assert (out[got:] == 7.0).all()
    return out[:got].reshape(-1, n)


@pytest.mark.parametrize("name", list(X.KERNELS))
def test_taps_equal_the_restatement(name):
    kernel = X.KERNELS[name]
    count = 0
    for radius in RADII:
        big_d = X.reach(radius)
        assert big_d == {0.5: 0, 1.0: 1, 1.5: 1, 2.0: 2, 2.5: 2, 4.0: 4}[radius]
        for n in POINTS:
            for lo in range(big_d + 1):
                for hi in range(big_d + 1):
                    got, want = library_taps(kernel, radius, n, lo, hi), X.taps(kernel, radius, n, lo, hi)
                    assert want is not None and got.shape == want.shape
                    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (name, radius, n, lo, hi)
                    # taps that do not exist are 0; the table sums to 1 within 2 float ulps per tap
                    assert (got[:big_d - lo] == 0).all() and (got[big_d + hi + 1:] == 0).all()
                    taps = np.count_nonzero(got)
                    assert taps >= 1 and abs(got.astype(f64).sum() - 1.0) <= 2 * float(np.finfo(f32).eps) * taps, (name, radius, n, lo, hi)
                    count += 1
    assert count == 5 * (1 + 4 + 4 + 9 + 9 + 25)
    assert np.array_equal(mm.api.clip_filter_taps(name, 3, 0, X.reach(X.DEFAULT_RADII[name])),
                          library_taps(kernel, X.DEFAULT_RADII[name], 3, 0, X.reach(X.DEFAULT_RADII[name])))


def test_tables_worked_out_by_hand():
    for n in (1, 2, 4, 8):                                   # box at radius 0.5: the pixel's own grid, 1 / n each
        assert library_taps(X.BOX, 0.5, n, 0, 0).tolist() == [[1.0 / n] * n]
    assert np.count_nonzero(library_taps(X.MITCHELL, 2.0, 4, 2, 2) < 0) > 0     # Mitchell's negative lobes
    # tent at radius 1 over two points per pixel: d = -1.25 (outside), -0.75 | -0.25, 0.25 | 0.75, 1.25 (outside)
    assert library_taps(X.TENT, 1.0, 2, 1, 1).tolist() == [[0.0, 0.125], [0.375, 0.375], [0.125, 0.0]]
    # ... and at the frame's first pixel: k = 0.75, 0.75, 0.25 over n = 1.75
    assert library_taps(X.TENT, 1.0, 2, 0, 1).tolist() == [[0.0, 0.0], [float(f32(0.75 / 1.75))] * 2, [float(f32(0.25 / 1.75)), 0.0]]
    # one point per pixel: the neighbours sit at the radius and have no weight
    assert library_taps(X.TENT, 1.0, 1, 1, 1).tolist() == [[0.0], [1.0], [0.0]]
    sym = library_taps(X.GAUSSIAN, 1.5, 3, 1, 1)
    assert np.array_equal(sym, sym[::-1, ::-1]) and (sym > 0).all()


def test_taps_refuse_bad_arguments():
    out = (C.c_float * 80)()
    for args, word in (((4, 1.0, 2, 0, 0), "kernel"), ((-1, 1.0, 2, 0, 0), "kernel"), ((1, 0.25, 2, 0, 0), "radius"), ((1, 4.5, 2, 0, 0), "radius"),
                       ((1, float("nan"), 2, 0, 0), "radius"), ((1, 1.0, 0, 0, 0), "n must be"), ((1, 1.0, 9, 0, 0), "n must be"),
                       ((1, 1.0, 2, 2, 0), "lo and hi"), ((1, 1.0, 2, 0, -1), "lo and hi")):
        assert lib().mmhip_clip_filter_taps(*args, out) == -1 and word in err(), (args, err())
    assert lib().mmhip_clip_filter_taps(1, 1.0, 2, 0, 0, None) == -1 and "out" in err()


# ---- the two sums, compiled for the host ----

SUMS = r'''
#include <stdio.h>
#include <vector>
#include "mm_clip_filter.h"
#include "mm_sample_grid.h"

/* a 5 x 4 frame, a 2 x 1 grid, tent at radius 1; map a holds 8 * (c + 1) + 64 * r + a * 4 in every channel but for the
   texels named on the command line: (a, c, r, kind) with kind 0 = NaN, 1 = inf */
int main(int argc, char **argv) {
    if (argc < 2 || (argc - 2) % 4 != 0) return 2;
    const int W = 5, H = 4, sx = 2, sy = 1;
    const double radius = 1.0;
    const int D = mm_clip_filter_reach(radius);
    if (D != 1) return 3;
    std::vector<float> map[2];
    for (int a = 0; a < sx; ++a) {
        map[a].resize(W * H * 4);
        for (int r = 0; r < H; ++r)
            for (int c = 0; c < W; ++c)
                for (int ch = 0; ch < 4; ++ch) map[a][(r * W + c) * 4 + ch] = (float)(8 * (c + 1) + 64 * r + a * 4);
    }
    for (int i = 2; i + 3 < argc; i += 4) {
        int a, c, r, kind;
        if (sscanf(argv[i], "%d", &a) != 1 || sscanf(argv[i + 1], "%d", &c) != 1 || sscanf(argv[i + 2], "%d", &r) != 1 || sscanf(argv[i + 3], "%d", &kind) != 1) return 2;
        for (int ch = 0; ch < 4; ++ch) map[a][(r * W + c) * 4 + ch] = kind ? __builtin_inff() : __builtin_nanf("");
    }
    float ox[MM_SAMPLE_GRID_MAX], oy[MM_SAMPLE_GRID_MAX];
    for (int a = 0; a < sx; ++a) ox[a] = mm_sample_grid_offset(a, sx);
    for (int b = 0; b < sy; ++b) oy[b] = mm_sample_grid_offset(b, sy);
    const int tx_n = mm_clip_filter_tap_count(D, sx), ty_n = mm_clip_filter_tap_count(D, sy);
    std::vector<float> tx((D + 1) * (D + 1) * tx_n), ty((D + 1) * (D + 1) * ty_n);
    for (int lo = 0; lo <= D; ++lo)
        for (int hi = 0; hi <= D; ++hi) {
            if (mm_clip_filter_taps(MM_CLIP_FILTER_TENT, radius, sx, ox, lo, hi, tx.data() + (lo * (D + 1) + hi) * tx_n) != 0) return 5;
            if (mm_clip_filter_taps(MM_CLIP_FILTER_TENT, radius, sy, oy, lo, hi, ty.data() + (lo * (D + 1) + hi) * ty_n) != 0) return 5;
        }
    if (mm_clip_filter_class(0, W, D) != 1 || mm_clip_filter_class(2, W, D) != 3 || mm_clip_filter_class(4, W, D) != 2) return 6;
    const float *maps[2] = {map[0].data(), map[1].data()};
    std::vector<float> h(sy * H * W * 4), s(H * W * 4);
    mm_clip_filter_step_host(maps, W, H, sx, sy, D, tx.data(), ty.data(), h.data(), s.data());
    FILE *out = fopen(argv[1], "wb");
    if (!out) return 2;
    if (fwrite(s.data(), sizeof(float), s.size(), out) != s.size()) return 4;
    return fclose(out) != 0;
}
'''


def sums_by_hand(special):
    """The frame of SUMS as the statement has it, written out tap by tap."""
    w, h = 5, 4
    maps = np.empty((2, h, w), f32)
    for a in range(2):
        for r in range(h):
            for c in range(w):
                maps[a, r, c] = 8 * (c + 1) + 64 * r + a * 4
    for a, c, r, kind in special:
        maps[a, r, c] = np.inf if kind else np.nan
    edge, far = f32(0.75 / 1.75), f32(0.25 / 1.75)
    out = np.empty((h, w), f32)
    with np.errstate(all="ignore"):
        for r in range(h):
            # the first column has no pixel before it, the last none after it: three existing non-zero taps each
            out[r, 0] = f32(f32(f32(edge * maps[0, r, 0]) + f32(edge * maps[1, r, 0])) + f32(far * maps[0, r, 1]))
            out[r, 4] = f32(f32(f32(far * maps[1, r, 3]) + f32(edge * maps[0, r, 4])) + f32(edge * maps[1, r, 4]))
            for c in (1, 2, 3):
                acc = f32(f32(0.125) * maps[1, r, c - 1])
                acc = f32(acc + f32(f32(0.375) * maps[0, r, c]))
                acc = f32(acc + f32(f32(0.375) * maps[1, r, c]))
                out[r, c] = f32(acc + f32(f32(0.125) * maps[0, r, c + 1]))
    # down the column the only tap is the pixel's own row, weight 1: s = 1 * h
    return out


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "sanitizers"])
def test_the_two_sums_on_a_frame_worked_out_by_hand(sanitize):
    """A stand-alone host program over the header the runtime and the kernel include; once under the address and
    undefined-behaviour sanitizers (host code only)."""
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    # NaN in map 0 at (2, 1): pixels (1, 1) and (2, 1) read it with a weight, pixel (3, 1) with weight 0 and rows 0 and 2
    # with weight 0: it spreads to the two and no further.  inf in map 1 at the last column of the last row: its own pixel
    # only -- pixel (3, 3) has it under the zero tap (1, 1), where 0 * inf would be NaN.  NaN in map 1 at (0, 0): under
    # the taps of pixels (0, 0) and (1, 0).
    special = [(0, 2, 1, 0), (1, 4, 3, 1), (1, 0, 0, 0)]
    d = tempfile.mkdtemp(prefix="mm_filter_")
    try:
        open(os.path.join(d, "t.cpp"), "w").write(SUMS)
        flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else ["-O2"]
        exe = os.path.join(d, "t")
        subprocess.run([cxx, "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off"] + flags +
                       ["-I", os.path.join(ROOT, "mathmap_amd", "csrc"), "-o", exe, os.path.join(d, "t.cpp")], check=True)
        got = {}
        for key, cells in (("plain", []), ("special", special)):
            path = os.path.join(d, key + ".bin")
            r = subprocess.run([exe, path] + [str(v) for cell in cells for v in cell], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
            assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
            got[key] = np.fromfile(path, f32).reshape(4, 5, 4)
    finally:
        shutil.rmtree(d, ignore_errors=True)
    from tests.shutter_reference import same_floats
    for key, cells in (("plain", []), ("special", special)):
        want = sums_by_hand(cells)
        for ch in range(4):
            assert same_floats(got[key][:, :, ch], want), (key, ch)
    plain, sp = got["plain"][:, :, 0], got["special"][:, :, 0]
    assert plain[1, 2] == 0.125 * 84 + 0.375 * 88 + 0.375 * 92 + 0.125 * 96               # an interior pixel, exact in float
    nan = np.isnan(sp)
    assert sorted(zip(*np.nonzero(nan))) == [(0, 0), (0, 1), (1, 1), (1, 2)]
    assert sorted(zip(*np.nonzero(np.isinf(sp)))) == [(3, 4)]
    rest = ~(nan | np.isinf(sp))
    assert np.array_equal(sp[rest], plain[rest])
    # the restatement makes the same frame of the same maps
    maps = np.empty((1, 2, 4, 5, 4), f32)
    for a in range(2):
        for r in range(4):
            for c in range(5):
                maps[0, a, r, c] = 8 * (c + 1) + 64 * r + a * 4
    for a, c, r, kind in special:
        maps[0, a, r, c] = np.inf if kind else np.nan
    assert same_floats(X.step(maps, X.TENT, 1.0), got["special"])


# ---- plans (MMHIP_CLIP_SHUTTER_BYTES is read once per process: a child process each) ----

def plan_key(p):
    return (p["frames_per_batch"], p["batches"], p["steps_per_pass"], p["passes"], p["carry"], p["bytes_per_sample"], p["halo_columns"], p["halo_rows"])


def test_plan_with_the_default_budget():
    flt = F.load("ident")
    # the whole 97 x 61 frame: the halo is clipped at all four edges
    assert plan_key(flt.clip_filtered_plan(97, 61, 97, 61, 1, 2, "tent", 3)) == (3, 1, 1, 1, 0, 61 * 16 * 97, 97, 61)
    # region (5, 3, 40, 30) under Mitchell at radius 2: two more columns and rows on every side
    assert plan_key(flt.clip_filtered_plan(40, 30, 97, 61, 3, (2, 1), "mitchell", 5, region_x=5, first_row=3)) == \
        (5, 1, 3, 1, 0, 34 * 16 * 97, 44, 34)
    # a region in the corner: the halo on two sides only
    assert plan_key(flt.clip_filtered_plan(10, 10, 97, 61, 1, 2, "gaussian", 1)) == (1, 1, 1, 1, 0, 11 * 16 * 97, 11, 11)
    assert plan_key(flt.clip_filtered_plan(10, 10, 97, 61, 1, 2, "gaussian", 1, region_x=87, first_row=51)) == (1, 1, 1, 1, 0, 11 * 16 * 97, 11, 11)
    # the band [7, 8) at radius 4: four rows either side; box at radius 0.5 has no halo at all
    assert plan_key(flt.clip_filtered_plan(97, 1, 97, 61, 1, 1, "tent", 2, aa_radius=4.0, first_row=7)) == (2, 1, 1, 1, 0, 9 * 16 * 97, 97, 9)
    assert plan_key(flt.clip_filtered_plan(40, 30, 97, 61, 1, 4, "box", 2, region_x=5, first_row=3)) == (2, 1, 1, 1, 0, 30 * 16 * 97, 40, 30)
    # 8192^2 at aa = 2: 4 GiB of maps per frame, two frames in the 8 GiB
    assert plan_key(flt.clip_filtered_plan(8192, 8192, 8192, 8192, 1, 2, "tent", 5))[:2] == (2, 3)
    for args, word in (((97, 61, 97, 61, 1, 2, "tent", 0), "num_frames"), ((98, 61, 97, 61, 1, 2, "tent", 1), "columns"),
                       ((97, 62, 97, 61, 1, 2, "tent", 1), "rows"), ((97, 61, 97, 61, 0, 2, "tent", 1), "samples"),
                       ((97, 61, 97, 61, 5, 8, "tent", 1), "samples \\* grid_x \\* grid_y"), ((0, 61, 97, 61, 1, 2, "tent", 1), "empty region")):
        with pytest.raises(mm.MathMapError, match=word):
            flt.clip_filtered_plan(*args)
    with pytest.raises(ValueError, match="aa_radius"):
        flt.clip_filtered_plan(97, 61, 97, 61, 1, 2, "tent", 1, aa_radius=5)
    with pytest.raises(ValueError, match="aa_filter"):
        flt.clip_filtered_plan(97, 61, 97, 61, 1, 2, "lanczos", 1)


def test_plan_under_a_budget_from_the_environment():
    rows = 34                                                # region (5, 3, 40, 30) at D = 2
    bps = rows * 16 * 97
    prog = ("import json, sys; sys.path.insert(0, %r); from tests import filters as F; f = F.load('ident'); "
            "print(json.dumps([f.clip_filtered_plan(40, 30, 97, 61, k, aa, 'mitchell', n, region_x=5, first_row=3) "
            "for k, aa, n in ((1, (2, 2), 7), (3, (2, 1), 7), (5, (2, 2), 3), (4, 1, 3))]))" % ROOT)
    cases = [
        # 12 maps of the haloed rectangle fit: 3 frames of 4, 2 of 6; 20 do not: (12 - 1) / 4 = 2 time steps per pass beside the
        # carry, 3 passes; a 1 x 1 grid of 4 steps: 3 frames
        (12 * bps + 100, [(3, 3, 1, 1, 0), (2, 4, 3, 1, 0), (1, 3, 2, 3, 1), (3, 1, 4, 1, 0)]),
        # one byte short of a frame of 6: (5 - 1) / 2 = 2 steps per pass; a frame of 4 single maps still fits
        (6 * bps - 1, [(1, 7, 1, 1, 0), (1, 7, 2, 2, 1), (1, 3, 1, 5, 1), (1, 3, 4, 1, 0)]),
        # the soft minimum: one time step per pass whatever the budget
        (1, [(1, 7, 1, 1, 0), (1, 7, 1, 3, 1), (1, 3, 1, 5, 1), (1, 3, 1, 4, 1)]),
    ]
    for budget, want in cases:
        env = dict(os.environ, MMHIP_CLIP_SHUTTER_BYTES=str(budget))
        out = subprocess.run([sys.executable, "-c", prog], env=env, check=True, capture_output=True, text=True).stdout
        plans = json.loads(out.strip().splitlines()[-1])
        assert [plan_key(p)[:5] for p in plans] == want, (budget, plans)
        assert all(plan_key(p)[5:] == (bps, 44, 34) for p in plans)


# ---- refusals ----

FRAMES2 = (C.c_int * 2)(0, 1)
TS2 = (C.c_float * 2)(0.0, 0.5)


def refused(samples=2, span=0.1, gx=2, gy=2, kernel=1, radius=1.0, num_frames=2, fr=FRAMES2, tt=TS2, row_stride=256, frame_stride=8192, bpp=4,
            w=64, h=32):
    """Checked before anything touches the invocation: a null one will do."""
    rc = lib().mmhip_render_clip_filtered(None, num_frames, fr, tt, samples, span, gx, gy, kernel, radius, 0, 0, w, h, 0, h, None, row_stride,
                                          frame_stride, bpp, 0, None)
    assert rc != 0
    return err()


def test_the_call_refuses_bad_arguments_with_a_message():
    for v in (0, -1, 9):
        for axis in ("gx", "gy"):
            msg = refused(**{axis: v})
            assert msg.startswith("render_clip_filtered: grid_x and grid_y must be 1 to 8") and str(v) in msg, msg
    for samples in (0, -1, 257):
        msg = refused(samples=samples)
        assert msg.startswith("render_clip_filtered: samples must be 1 to 256") and str(samples) in msg, msg
    msg = refused(samples=65, gx=2, gy=2)
    assert "samples * grid_x * grid_y" in msg and "256" in msg and "260" in msg, msg
    for kernel in (-1, 4, 100):
        msg = refused(kernel=kernel)
        assert msg.startswith("render_clip_filtered: kernel must be MMHIP_AA_BOX") and str(kernel) in msg, msg
    for radius in (0.0, 0.49, 4.01, -1.0, float("nan"), float("inf")):
        msg = refused(radius=radius)
        assert msg.startswith("render_clip_filtered: radius must be 0.5 to 4 pixels"), msg
    for span in (float("nan"), float("inf"), float("-inf")):
        assert refused(span=span) == "render_clip_filtered: span must be finite"
    assert refused(num_frames=0) == "render_clip_filtered: num_frames must be at least 1"
    assert "frames and ts" in refused(fr=None) and "frames and ts" in refused(tt=None)
    assert "bpp" in refused(bpp=5) and "empty region" in refused(w=0) and "empty region" in refused(h=0)
    assert refused(frame_stride=8191).startswith("render_clip_filtered: frame_stride 8191 is smaller")
    # a 1 x 1 grid with one sample delegates to nothing: the name stays, and the kernel is still looked at
    assert refused(gx=1, gy=1, samples=1, num_frames=0).startswith("render_clip_filtered:")
    assert "kernel" in refused(gx=1, gy=1, samples=1, kernel=7)
    # whatever the sampled call refuses, word for word under the other name
    for case in (dict(gx=0), dict(samples=257), dict(samples=129, gx=2, gy=1), dict(span=float("nan")), dict(num_frames=-3), dict(bpp=0),
                 dict(frame_stride=8191)):
        args = dict(dict(samples=2, span=0.1, gx=2, gy=2, num_frames=2, fr=FRAMES2, tt=TS2, row_stride=256, frame_stride=8192, bpp=4, w=64, h=32), **case)
        rc = lib().mmhip_render_clip_sampled(None, args["num_frames"], args["fr"], args["tt"], args["samples"], args["span"], args["gx"], args["gy"],
                                             0, 0, args["w"], args["h"], 0, args["h"], None, args["row_stride"], args["frame_stride"], args["bpp"], 0, None)
        assert rc != 0
        assert err().replace("render_clip_sampled:", "render_clip_filtered:") == refused(**case), case


# ---- aa_filter in Python, --aa-filter on the command line ----

def test_python_argument_errors():
    """Refused before anything else is looked at (an invocation needs a GPU; the checks do not, so an unbound one will do)."""
    inv = mm.api.Invocation.__new__(mm.api.Invocation)
    for name in ("lanczos", "Tent", "", 1, ("tent",)):
        with pytest.raises(ValueError, match="aa_filter"):
            inv.render_clip(num_frames=2, aa=2, aa_filter=name)
    for radius in (0.49, 4.5, 0, -1, float("nan"), float("inf"), "wide"):
        with pytest.raises(ValueError, match="aa_radius"):
            inv.render_clip(num_frames=2, aa=2, aa_filter="tent", aa_radius=radius)
    with pytest.raises(ValueError, match="aa_radius needs aa_filter"):
        inv.render_clip(num_frames=2, aa=2, aa_radius=1.0)
    with pytest.raises(ValueError, match="aa_filter is not combined with aa_threshold"):
        inv.render_clip(num_frames=2, aa=2, aa_filter="tent", aa_threshold=0.1)
    with pytest.raises(ValueError, match="aa_filter is not combined with supersample"):
        inv.render_clip(num_frames=2, aa=1, aa_filter="tent", supersample=True)
    with pytest.raises(ValueError, match="aa_filter is not combined with shutter_mode"):
        inv.render_clip(num_frames=2, aa=2, aa_filter="tent", shutter_mode="fused")
    with pytest.raises(ValueError, match="256"):
        inv.render_clip(num_frames=2, aa=8, aa_filter="tent", shutter_samples=5, shutter=0.5)
    with pytest.raises(ValueError, match="needs shutter"):                       # a shutter still needs its span
        inv.render_clip(num_frames=2, aa=2, aa_filter="tent", shutter_samples=4)
    with pytest.raises(ValueError, match="aa"):
        inv.render_clip(num_frames=2, aa=9, aa_filter="tent")
    from mathmap_amd.api import aa_filter_kernel
    assert aa_filter_kernel("box") == (0, 0.5) and aa_filter_kernel("tent") == (1, 1.0) and aa_filter_kernel("gaussian") == (2, 1.5)
    assert aa_filter_kernel("mitchell") == (3, 2.0) and aa_filter_kernel("mitchell", 0.5) == (3, 0.5) and aa_filter_kernel("box", 4) == (0, 4.0)


def test_cli_help_and_argument_errors(tmp_path):
    p = subprocess.run([CLI, "--help"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=60)
    assert p.returncode == 0 and "--aa-filter=NAME[:RADIUS]" in p.stdout and "--aa=N | SXxSY" in p.stdout
    src = "filter f () rgba:[t, 0, 0, 1] end"
    for extra, word in ((["--aa=2", "--aa-filter=lanczos"], "--aa-filter"), (["--aa=2", "--aa-filter="], "--aa-filter"),
                        (["--aa=2", "--aa-filter=tent:"], "--aa-filter"), (["--aa=2", "--aa-filter=tent:0.4"], "--aa-filter"),
                        (["--aa=2", "--aa-filter=tent:5"], "--aa-filter"), (["--aa=2", "--aa-filter=tent:1x"], "--aa-filter"),
                        (["--aa=2", "--aa-filter=tent:nan"], "--aa-filter"), (["--aa-filter=tent"], "goes with --aa"),
                        (["-o", "--aa=1", "--aa-filter=tent"], "-o"), (["--aa=2", "--aa-threshold=0.1", "--aa-filter=tent"], "--aa-threshold"),
                        (["--aa=2", "--shutter-mode=fused", "--aa-filter=tent"], "--shutter-mode=fused"),
                        (["--aa=8", "--shutter-samples=5", "--aa-filter=tent"], "256")):
        p = subprocess.run([CLI, "-F", "3", "-s", "8x8"] + extra + [src, str(tmp_path / "f%d.png")], stdout=subprocess.PIPE,
                           stderr=subprocess.PIPE, text=True, timeout=60)
        assert p.returncode != 0 and word in p.stderr, (extra, p.stderr)
    assert not list(tmp_path.iterdir())
