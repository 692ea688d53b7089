"""Adaptively anti-aliased clips (mmhip_render_clip_adaptive) without a GPU: the entry points and the header's statement of
the semantics, the argument errors, the delegation of the 1 x 1 grid, aa_threshold in Python and --aa-threshold on the
command line, the NumPy restatement of tests/adaptive_aa_reference.py against a map worked out by hand, the arithmetic
that cuts a clip into batches, and the refine variant's text: its kernels, what it shares with the sampled variant, its
gfx950 compile, and that asking for it leaves the other four texts alone."""
import ctypes as C
import hashlib
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import mathmap_amd as mm
from mathmap_amd._lib import lib
from tests import adaptive_aa_reference as A
from tests import filters as F
from tests import shutter_fused_probes as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "mathmap_amd", "mathmap_hip_cli")
W, H = P.W, P.H
f32 = np.float32
ROW_SLICE = ("wave", "extreme")          # probes with a per-row slice: neither a sampled nor a refine variant
NAN, INF = float("nan"), float("inf")


def err():
    return lib().mmhip_last_error().decode()


def active(name, flt):
    return flt.specialized() if P.PROBES[name][1].get("specialize") else flt


# ---- entry points ----

def test_entry_points_exist_and_are_declared():
    header = open(os.path.join(ROOT, "include", "mmhip.h")).read()
    for name in ("mmhip_render_clip_adaptive", "mmhip_filter_clip_adaptive_plan", "mmhip_clip_adaptive_batches", "mmhip_clip_adaptive_refined",
                 "mmhip_filter_refine_kernel_source", "mmhip_filter_jit_refine"):
        assert hasattr(lib(), name), name
        assert re.search(r"\b%s\s*\(" % name, header), name
    from mathmap_amd.api import AA_REFINE_MODES, CLIP_ADAPTIVE_PLAN_FIELDS
    assert CLIP_ADAPTIVE_PLAN_FIELDS == ("list_path", "frames_per_batch", "batches", "bytes_per_frame", "refine_grid_x")
    assert AA_REFINE_MODES == ("list", "select")
    assert re.search(r"MMHIP_CLIP_ADAPTIVE_PLAN_FIELDS\s*=\s*5\b", header)
    assert re.search(r"MMHIP_AA_REFINE_AUTO\s*=\s*0\b", header) and re.search(r"MMHIP_AA_REFINE_SELECT\s*=\s*1\b", header)
    for attr in ("clip_adaptive_plan", "refine_kernel_source", "jit_refine"):
        assert hasattr(mm.Filter, attr), attr
    for attr in ("clip_adaptive_batches", "clip_adaptive_refined"):
        assert hasattr(mm.api.Invocation, attr), attr
    flat = re.sub(r"\s+", " ", header)
    args = re.search(r"int mmhip_render_clip_adaptive\((.*?)\);", flat).group(1)
    assert args.startswith("mmhip_invocation *inv, int num_frames, const int *frames, const float *ts, int grid_x, int grid_y, float threshold, int mode, "
                           "int region_x, int region_y, int region_w, int region_h, int first_row, int last_row, void *out_device")
    assert "samples" not in args and "span" not in args          # spatial only


def test_the_header_states_the_semantics():
    header = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "mmhip.h")).read())
    for phrase in ("Every output pixel equals one of two existing renders, chosen by a mask computed from an existing render",
                   "c(v) = v < 0 ? 0 : (v > 1 ? 1 : v)",
                   "NaN stays NaN, +inf becomes 1 and -inf 0",
                   "!(fabsf(c(F[p][ch]) - c(F[q][ch])) <= threshold)",
                   "one f32 subtraction, no fma",
                   "a NaN contrast refines",
                   "Neighbours outside the rectangle are skipped",
                   "a 1 x 1 rectangle is refined by a negative threshold only",
                   "mmhip_render_clip_sampled(samples = 1, grid_x, grid_y)",
                   "summed in the order b * sx + a",
                   "mm_shutter_inv_k(G)",
                   "acc = f_0, times mm_shutter_inv_k(1), through mm_shutter_store_bytes",
                   "at sampling offset (0, 0)",
                   "put back on every return, failed calls included",
                   "NaN, which is refused before anything else is looked at",
                   "grid_x = grid_y = 1 is mmhip_render_clip",
                   "refines differently at the band seams",
                   "col | rl << 16",
                   "region_w and rows at most 65 535",
                   "the host never reads a count while rendering",
                   "It saves no time",
                   "MMHIP_CLIP_SHUTTER_BYTES",
                   "aa_contrast_clip",
                   "the sampled variant's mm_prologue_clip, text unchanged"):
        assert phrase in header, phrase


# ---- refusals (checked before anything touches the invocation: a null one will do) ----

FRAMES2 = (C.c_int * 2)(0, 1)
TS2 = (C.c_float * 2)(0.0, 0.5)


def refused(threshold=0.1, mode=0, gx=2, gy=2, num_frames=2, fr=FRAMES2, tt=TS2, row_stride=256, frame_stride=8192, bpp=4, w=64, h=32):
    rc = lib().mmhip_render_clip_adaptive(None, num_frames, fr, tt, gx, gy, threshold, mode, 0, 0, w, h, 0, h, None, row_stride, frame_stride, bpp, 0, None)
    assert rc != 0
    return err()


def sampled_refused(gx=2, gy=2, num_frames=2, fr=FRAMES2, tt=TS2, row_stride=256, frame_stride=8192, bpp=4, w=64, h=32):
    rc = lib().mmhip_render_clip_sampled(None, num_frames, fr, tt, 1, 0.0, gx, gy, 0, 0, w, h, 0, h, None, row_stride, frame_stride, bpp, 0, None)
    assert rc != 0
    return err()


def plain_refused(num_frames=2, fr=FRAMES2, tt=TS2, row_stride=256, frame_stride=8192, bpp=4, w=64, h=32):
    rc = lib().mmhip_render_clip(None, num_frames, fr, tt, 0, 0, w, h, 0, h, None, row_stride, frame_stride, bpp, 0, None)
    assert rc != 0
    return err()


def test_a_nan_threshold_is_refused_first():
    assert refused(threshold=NAN) == "render_clip_adaptive: threshold must not be NaN"
    for other in (dict(gx=0), dict(gx=1, gy=1, num_frames=0), dict(mode=7), dict(num_frames=0), dict(bpp=9)):
        assert refused(threshold=NAN, **other) == "render_clip_adaptive: threshold must not be NaN", other
    for threshold in (-1.0, 0.0, 1e30, INF, -INF):          # every other float passes: the next check speaks
        assert "num_frames" in refused(threshold=threshold, num_frames=0)


def test_the_grid_checks_are_the_sampled_calls_word_for_word():
    cases = ([dict(gx=v) for v in (0, -1, 9)] + [dict(gy=v) for v in (0, -1, 9)] + [dict(gx=9, gy=0)] +
             [dict(num_frames=0), dict(num_frames=-3), dict(fr=None), dict(tt=None), dict(bpp=5), dict(bpp=0), dict(w=0), dict(h=0),
              dict(frame_stride=8191), dict(row_stride=300, frame_stride=31 * 300 + 255)])
    for case in cases:
        theirs = sampled_refused(**case)
        assert theirs and refused(**case) == theirs.replace("render_clip_sampled:", "render_clip_adaptive:"), case
    assert refused(gx=0).startswith("render_clip_adaptive: grid_x and grid_y must be 1 to 8")
    for mode in (-1, 2):
        assert refused(mode=mode) == "render_clip_adaptive: mode must be 0 (auto) or 1 (select), not %d" % mode
    assert "grid_x" in refused(mode=2, gx=9)                 # the grid before the mode


def test_the_1x1_grid_is_render_clip_word_for_word():
    for case in (dict(num_frames=0), dict(fr=None), dict(tt=None), dict(bpp=5), dict(w=0), dict(frame_stride=8191)):
        msg = refused(gx=1, gy=1, **case)
        assert msg == plain_refused(**case) and not msg.startswith("render_clip_adaptive"), case
    assert refused(gx=1, gy=1, num_frames=0).startswith("render_clip:")
    assert refused(gx=1, gy=1, num_frames=0, mode=7).startswith("render_clip:")           # delegated right after the threshold
    assert refused(gx=1, gy=1, num_frames=0, threshold=NAN).startswith("render_clip_adaptive: threshold")


def test_plans_refuse_bad_arguments():
    flt, _ = P.compiled("pair")
    with pytest.raises(mm.MathMapError, match="num_frames"):
        flt.clip_adaptive_plan(64, 64, 64, 2, 0)
    with pytest.raises(mm.MathMapError, match="region"):
        flt.clip_adaptive_plan(65, 64, 64, 2, 3)
    with pytest.raises(mm.MathMapError, match="region"):
        flt.clip_adaptive_plan(64, 0, 64, 2, 3)
    for aa in (0, 9, (2, 9), "2", None):
        with pytest.raises(ValueError, match="aa"):
            flt.clip_adaptive_plan(64, 64, 64, aa, 3)


# ---- aa_threshold in Python, --aa-threshold on the command line ----

def test_python_argument_errors():
    """Refused before anything else is looked at (an invocation needs a GPU; the checks do not, so an unbound one will do)."""
    inv = mm.api.Invocation.__new__(mm.api.Invocation)
    with pytest.raises(ValueError, match="aa_threshold is not combined with supersample"):
        inv.render_clip(num_frames=2, aa=2, aa_threshold=0.05, supersample=True)
    with pytest.raises(ValueError, match="aa_threshold is not combined with shutter_samples"):
        inv.render_clip(num_frames=2, aa=2, aa_threshold=0.05, shutter_samples=4, shutter=0.5)
    with pytest.raises(ValueError, match="aa_threshold must not be NaN"):
        inv.render_clip(num_frames=2, aa=2, aa_threshold=NAN)
    for refine in ("auto", "fused", None, 1):
        with pytest.raises(ValueError, match="aa_refine"):
            inv.render_clip(num_frames=2, aa=2, aa_threshold=0.05, aa_refine=refine)
    with pytest.raises(ValueError, match="aa is an int or a pair"):
        inv.render_clip(num_frames=2, aa=9, aa_threshold=0.05)
    # without a threshold the new argument is not looked at, and the old rules speak as they did
    with pytest.raises(ValueError, match="aa is not combined with supersample"):
        inv.render_clip(num_frames=2, aa=2, supersample=True, aa_refine="junk")
    with pytest.raises(ValueError, match="needs shutter"):
        inv.render_clip(num_frames=2, aa=2, shutter_samples=4, aa_refine="junk")
    import inspect
    sig = inspect.signature(mm.api.Invocation.render_clip)
    assert sig.parameters["aa_threshold"].default is None and sig.parameters["aa_refine"].default == "list"


def test_cli_help_and_argument_errors(tmp_path):
    p = subprocess.run([CLI, "--help"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=60)
    assert p.returncode == 0 and "--aa-threshold=T" in p.stdout and "--aa-refine=MODE" in p.stdout and "--aa=N | SXxSY" in p.stdout
    src = "filter f () rgba:[t, 0, 0, 1] end"
    for extra, word in ((["--aa-threshold=0.05"], "--aa-threshold goes with --aa"), (["--aa=1", "--aa-threshold=0.05"], "--aa-threshold goes with --aa"),
                        (["-o", "--aa=2", "--aa-threshold=0.05"], "--aa-threshold is not combined with -o"),
                        (["--aa=2", "--aa-threshold=0.05", "--shutter-samples=4"], "--aa-threshold is not combined with --shutter-samples"),
                        (["--aa=2", "--aa-threshold=nan"], "--aa-threshold takes"), (["--aa=2", "--aa-threshold="], "--aa-threshold takes"),
                        (["--aa=2", "--aa-threshold=0.1x"], "--aa-threshold takes"), (["--aa=2", "--aa-threshold=0.05", "--aa-refine=fast"], "--aa-refine takes"),
                        (["--aa=2", "--aa-refine=select"], "--aa-refine goes with --aa-threshold")):
        p = subprocess.run([CLI, "-F", "3", "-s", "8x8"] + extra + [src, str(tmp_path / "f%d.png")], stdout=subprocess.PIPE,
                           stderr=subprocess.PIPE, text=True, timeout=60)
        assert p.returncode != 0 and word in p.stderr, (extra, p.stderr)
    assert not list(tmp_path.iterdir())


# ---- the restatement against a map worked out by hand ----

def test_the_restatement_on_a_hand_worked_map():
    assert A.clamp([-INF, -1.0, -0.0, 0.25, 1.0, 1.5, INF]).tolist() == [0.0, 0.0, 0.0, 0.25, 1.0, 1.0, 1.0]
    assert np.isnan(A.clamp([NAN]))[0] and A.clamp([0.25]).dtype == f32
    # channel 0 of a 3 x 3 map; the other channels are flat.  Clamped: NaN .25 .25 / .5 .5 1 / .5 .5 1 -- the inf and the 2
    # are both 1, so there is no contrast between them
    red = np.array([[NAN, 0.25, 0.25],
                    [0.5, 0.5, INF],
                    [0.5, 0.5, 2.0]], f32)
    base = np.stack([red, np.full((3, 3), 0.5, f32), np.full((3, 3), -7.0, f32), np.ones((3, 3), f32)], axis=2)
    # the largest contrast of every pixel to a neighbour inside the map, by hand: the four pixels that touch the NaN have a
    # NaN contrast; (0,2): |.25 - 1| = .75; (1,2): |1 - .25| = .75; (2,0): 0; (2,1): |.5 - 1| = .5; (2,2): |1 - .5| = .5
    nan_touched = np.array([[1, 1, 0], [1, 1, 0], [0, 0, 0]], bool)
    assert np.array_equal(A.mask(base, INF), nan_touched)                       # a NaN contrast refines whatever the threshold
    assert np.array_equal(A.mask(base, 0.0), np.array([[1, 1, 1], [1, 1, 1], [0, 1, 1]], bool))
    assert np.array_equal(A.mask(base, 0.5), np.array([[1, 1, 1], [1, 1, 1], [0, 0, 0]], bool))      # .5 <= .5 is not refined
    assert np.array_equal(A.mask(base, 0.75), nan_touched)
    assert np.array_equal(A.mask(base, 0.7499999), np.array([[1, 1, 1], [1, 1, 1], [0, 0, 0]], bool))
    assert A.mask(base, -1.0).all() and A.mask(base, -0.0).sum() == 8 and A.mask(base, -1e-30).all()
    # any of the four channels: the same numbers in alpha alone
    alpha = np.stack([np.zeros((3, 3), f32)] * 3 + [red], axis=2)
    for t in (INF, 0.0, 0.5, -1.0):
        assert np.array_equal(A.mask(alpha, t), A.mask(base, t)), t
    # neighbours outside the rectangle are skipped: a band of the map sees less, a single pixel nothing
    assert np.array_equal(A.mask(base[2:], 0.0), np.array([[0, 1, 1]], bool))
    assert np.array_equal(A.mask(base[:, :1], INF), np.array([[1], [1], [0]], bool))
    for t in (0.0, 0.5, INF):
        assert not A.mask(base[:1, :1], t).any() and not A.mask(base[1:2, 2:], t).any()
    assert A.mask(base[:1, :1], -1.0).all()
    # the choice
    aa_px, plain_px = np.full((3, 3, 4), 7, np.uint8), np.full((3, 3, 4), 9, np.uint8)
    chosen = A.select(nan_touched, aa_px, plain_px)
    assert (chosen[nan_touched] == 7).all() and (chosen[~nan_touched] == 9).all() and chosen.dtype == np.uint8


# ---- plan arithmetic (MMHIP_CLIP_SHUTTER_BYTES is read once per process: a child process each) ----

PLANS = ("import json, sys; sys.path.insert(0, %r); from tests import shutter_fused_probes as P; "
         "print(json.dumps([P.compiled(name)[0].clip_adaptive_plan(*args) for name, args in json.loads(sys.argv[1])]))" % ROOT)


def plans(cases, budget=None):
    env = dict(os.environ)
    env.pop("MMHIP_CLIP_SHUTTER_BYTES", None)
    env.pop("MMHIP_CLIP_MAX_FRAMES", None)
    if budget is not None:
        env["MMHIP_CLIP_SHUTTER_BYTES"] = str(budget)
    out = subprocess.run([sys.executable, "-c", PLANS, json.dumps(cases)], env=env, check=True, capture_output=True, text=True).stdout
    return json.loads(out.strip().splitlines()[-1])


def plan(list_path, per, batches, bytes_per_frame, grid_x):
    return dict(list_path=list_path, frames_per_batch=per, batches=batches, bytes_per_frame=bytes_per_frame, refine_grid_x=grid_x)


def test_plans_worked_out_by_hand():
    bps, cells = H * 16 * W, W * H            # 94 672 bytes of base map, 5 917 list entries
    per_frame = bps + 4 * cells                # 118 340
    got = plans([
        ["pair", [W, H, W, 2, 3]],
        # many frames: the budget holds 8 GiB / 118 340 = 72 587 frames, a launch 65 535
        ["pair", [W, H, W, 2, 70000]],
        # a region narrower than the frame: the map has the frame's width, the list the region's
        ["pair", [50, 20, W, [2, 3], 7]],
        # 65 535 columns fit a list entry, 65 536 do not: the select path, no list
        ["pair", [65535, 1, 65535, 2, 3]],
        ["pair", [65536, 1, 65536, 2, 3]],
        ["pair", [1, 65536, 1, 2, 3]],
        # a per-row slice, a native call: no refine variant
        ["wave", [W, H, W, 2, 3]],
        ["blur", [W, H, W, 2, 3]],
    ])
    assert got == [
        plan(1, 3, 1, per_frame, 24),
        plan(1, 65535, 2, per_frame, 24),
        plan(1, 7, 1, 20 * 16 * W + 4 * 50 * 20, 4),
        plan(1, 3, 1, 65535 * 20, 256),
        plan(0, 3, 1, 65536 * 16, 0),
        plan(0, 3, 1, 65536 * 16, 0),
        plan(0, 3, 1, bps, 0),
        plan(0, 3, 1, bps, 0),
    ], got
    # the budget forces one frame per batch: one byte short of a frame is still one frame, the soft minimum
    for budget, per in ((2 * per_frame + 100, 2), (per_frame, 1), (per_frame - 1, 1), (1, 1)):
        got = plans([["pair", [W, H, W, 2, 5]], ["wave", [W, H, W, 2, 5]]], budget)
        assert got[0] == plan(1, per, -(-5 // per), per_frame, 24), (budget, got)
        assert got[1] == plan(0, max(1, budget // bps), -(-5 // max(1, budget // bps)), bps, 0), (budget, got)


# ---- the refine variant's text ----

def kernel_names(text):
    return re.findall(r'extern "C" __global__ void __launch_bounds__\(256\) (\w+)\(', text)


def texts(flt):
    return (flt.kernel_source, flt.clip_kernel_source, flt.shutter_kernel_source, flt.sampled_kernel_source)


@pytest.mark.parametrize("name", [n for n in P.PROBES if n not in ROW_SLICE])
def test_the_refine_text_of_every_probe(name):
    flt = active(name, P.compiled(name)[0])
    before = texts(flt)
    sampled = before[3]
    text = flt.refine_kernel_source
    assert kernel_names(text) == ["mm_prologue_clip", "mm_pixels_refine"]
    assert kernel_names(sampled) == ["mm_prologue_clip", "mm_pixels_sampled"]
    assert text.count("struct mm_refine { const unsigned *list; const unsigned *counts; long long list_stride; };\n") == 1
    assert "mm_refine" not in sampled
    # everything in front of the pixel kernel -- preludes, functions, mm_prologue_clip with the per-offset tables -- is the
    # sampled variant's, byte for byte
    head = text[:text.index("struct mm_refine")]
    assert head == sampled[:sampled.rindex("\n", 0, sampled.index("mm_pixels_sampled(")) + 1]
    assert "mm_prologue_clip(mm_args A, char *XY, const mm_clip C, const mm_sampled S)" in head and "S.xtabs[mm_a * A.region_width + gid]" in head
    # the kernel's head: the list in place of the tile order
    body = text[text.index("mm_pixels_refine("):]
    assert body.startswith("mm_pixels_refine(mm_args A, const char *__restrict__ XY, const mm_clip C, const mm_sampled S, const mm_refine R) {\n")
    lead = body[:body.index("  const char *const mm_xy0 = XY;\n")]
    assert "const int fi = blockIdx.y;" in lead and "blockIdx.x * 256u + threadIdx.x;" in lead
    assert "if (mm_i >= R.counts[fi]) return;" in lead and "R.list[(long long)fi * R.list_stride + mm_i];" in lead
    assert "(mm_e & 0xffffu)" in lead and "(mm_e >> 16)" in lead and "A.out = (char *)A.out + (long long)fi * C.frame_stride;" in lead
    assert "tiles_x" not in lead and "C.nwg" not in lead and "row0" not in body
    # from there on -- the slot, the wave-uniform table counters, the loop, the pixel code between MM_INTERNALS and the
    # accumulate, the accumulators, the scale and the store -- the sampled kernel's, statement for statement
    theirs = sampled[sampled.index("mm_pixels_sampled("):]
    rest, their_rest = body[len(lead):], theirs[theirs.index("  const char *const mm_xy0 = XY;\n"):]
    assert rest == their_rest
    assert rest[rest.index("    MM_INTERNALS\n"):rest.index("    if (mm_s == 0) mm_acc = rt;")] == \
        their_rest[their_rest.index("    MM_INTERNALS\n"):their_rest.index("    if (mm_s == 0) mm_acc = rt;")]
    assert "mm_xo += A.region_width;" in rest and rest.count("mm_store_pixel(A, rl, col, mm_m);") == 1
    assert flt.jit_refine(load=False) > 0            # compiles for gfx950
    assert flt.refine_kernel_source == text
    # asking for it, and compiling it, left the other four texts alone: they are a fresh filter's
    fresh = active(name, P.compiled(name)[0])
    assert texts(flt) == before and before == texts(fresh)
    assert fresh.refine_kernel_source == text


@pytest.mark.parametrize("name", list(P.FALLBACKS) + list(ROW_SLICE))
def test_filters_without_a_refine_variant(name):
    flt, _ = P.compiled(name)
    before = (flt.kernel_source, flt.clip_kernel_source)
    with pytest.raises(mm.MathMapError, match="no refine variant"):
        flt.refine_kernel_source
    with pytest.raises(mm.MathMapError, match="no refine variant"):
        flt.jit_refine()
    assert (flt.kernel_source, flt.clip_kernel_source) == before
    assert flt.clip_adaptive_plan(W, H, W, 2, 3)["list_path"] == 0


def test_pinned_kernel_texts_keep_their_digests_around_the_variant():
    with open(os.path.join(ROOT, "tests", "golden", "clip_text_digests.json")) as f:
        want = json.load(f)["filters"]
    asked = 0
    for name, digests in want.items():
        flt = F.load(name)
        try:
            flt.refine_kernel_source
            asked += 1
        except mm.MathMapError as e:
            assert "no refine variant" in str(e)
        assert hashlib.sha256(flt.clip_kernel_source.encode()).hexdigest() == digests["clip_kernel_source_sha256"], name
        assert hashlib.sha256(flt.kernel_source.encode()).hexdigest() == digests["kernel_source_sha256"], name
    assert asked > 0
    from tools.kernel_body_digest import digests as body_digests
    with open(os.path.join(ROOT, "tests", "golden", "kernel_body_digests.json")) as f:
        assert body_digests() == json.load(f)["body_sha256"]
