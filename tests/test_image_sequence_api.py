"""Multi-frame input drawables, the part that needs no GPU: argument errors of the C ABI, the Python shape handling,
the command line's option errors, which fetch variant the generator picks for a site, and that the code generated for
the existing probe filters is what the parent commit generated."""
import ctypes as C
import hashlib
import json
import os
import re
import subprocess

import numpy as np
import pytest

import mathmap_amd as mm
from mathmap_amd import api
from mathmap_amd._lib import lib
from tests import filters as F
from tests import sequence_probes as P
from tools.kernel_body_digest import PROBES, body_text, digests

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "mathmap_amd", "mathmap_hip_cli")


def err():
    return lib().mmhip_last_error().decode()


# ---- C ABI: what is wrong with the arguments is reported before the invocation is looked at ----

@pytest.mark.parametrize("num_frames", [0, -1, -(1 << 31)])
def test_setters_reject_less_than_one_frame(num_frames):
    assert lib().mmhip_set_image_sequence_device(None, 0, None, 4, 4, num_frames) < 0
    assert "num_frames" in err()
    assert lib().mmhip_set_image_sequence_host(None, 0, None, 4, 4, 3, num_frames) < 0
    assert "num_frames" in err()


@pytest.mark.parametrize("w,h,n", [(1 << 30, 1 << 30, 1 << 30), ((1 << 31) - 1, (1 << 31) - 1, (1 << 31) - 1),
                                   (1 << 20, 1 << 20, 1 << 22), (-1, 4, 2), (4, -1, 2),
                                   # the generic fetch counts the rows of the whole sequence in an int
                                   (4, 1 << 20, 1 << 11), (1, 2, 1 << 30), (4, (1 << 31) - 1, 2)])
def test_setters_reject_sizes_that_overflow(w, h, n):
    assert lib().mmhip_set_image_sequence_device(None, 0, None, w, h, n) < 0
    assert "overflow" in err()
    assert lib().mmhip_set_image_sequence_host(None, 0, None, w, h, 4, n) < 0
    assert "overflow" in err()


def test_host_setter_checks_channels_like_the_single_image_one():
    assert lib().mmhip_set_image_sequence_host(None, 0, None, 4, 4, 2, 3) < 0
    assert "channels" in err()


def test_set_image_shapes():
    one = np.arange(5 * 7 * 3, dtype=np.uint8).reshape(5, 7, 3)
    a = api.as_image_sequence(one)
    assert a.shape == (1, 5, 7, 3) and a.flags["C_CONTIGUOUS"] and np.array_equal(a[0], one)
    seq = np.arange(4 * 5 * 7 * 4, dtype=np.uint8).reshape(4, 5, 7, 4)
    a = api.as_image_sequence(seq[:, :, ::-1])                  # a view: the upload wants it packed
    assert a.shape == (4, 5, 7, 4) and a.flags["C_CONTIGUOUS"] and np.array_equal(a, seq[:, :, ::-1])
    for bad in (np.zeros((5, 7), np.uint8), np.zeros((2, 2, 5, 7, 3), np.uint8), np.zeros((0, 5, 7, 3), np.uint8)):
        with pytest.raises(mm.MathMapError):
            api.as_image_sequence(bad)


def test_set_image_device_takes_num_frames():
    import inspect
    sig = inspect.signature(mm.Invocation.set_image_device)
    assert sig.parameters["num_frames"].default == 1


# ---- command line ----

def run_cli(*args):
    return subprocess.run([CLI] + list(args), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)


@pytest.mark.parametrize("value", ["0", "-2", "three", "2x", ""])
def test_cli_rejects_bad_frame_counts(value):
    p = run_cli("--input-frames=" + value, "-Din=a%d.png", P.PLAIN, "out.png")
    assert p.returncode == 1 and "--input-frames" in p.stderr, p.stderr


@pytest.mark.parametrize("name", ["a%s.png", "a%d_%d.png", "a%.png", "a%ld.png", "a%1234567d.png", "trailing%"])
def test_cli_rejects_patterns_it_cannot_print(name):
    p = run_cli("--input-frames=3", "-Din=" + name, P.PLAIN, "out.png")
    assert p.returncode == 1 and "conversion" in p.stderr, p.stderr


def test_cli_checks_only_image_defines_for_patterns():
    # a '%' in a value that is no image's file name is none of --input-frames' business: the run gets as far as the
    # missing input file (or, with a GPU, further)
    p = run_cli("--input-frames=2", "-Dnote=100%s", "-Din=/nonexistent/a%d.png", P.PLAIN, "out.png")
    assert "conversion" not in p.stderr and "a0.png" in p.stderr, p.stderr


def test_cli_help_lists_the_option_as_an_extension():
    out = run_cli("--help").stdout
    assert out.index("Extensions of the HIP command line") < out.index("--input-frames=NUM")


# ---- which fetch a site gets ----

def pixel_kernel(flt):
    body = body_text(flt.kernel_source)
    return body[body.index(" mm_pixels(mm_args A"):]


@pytest.mark.parametrize("intersample", [False, True])
def test_slit_scan_gets_the_per_pixel_hot_fetch(intersample, monkeypatch):
    src = P.text(P.SLIT, P.SLIT_FRAME)
    k = pixel_kernel(mm.Filter(src, intersample=intersample))
    hot, generic = k.split("if (mm_hot) {", 1)[1].split("if (mm_bad) break;", 1)
    assert re.search(r"mm_hot = mm_hot && mm_fetch_is_hot_any\(\w+_desc\);", k)
    assert ("mm_orig_val_sums_hotf(" if intersample else "mm_orig_val_hotf(") in hot and "mm_orig_val_d(" not in hot
    assert "hotf(" not in generic and "mm_orig_val_d(" in generic
    # the switch for the A/B: the site stays on the early-exit path, the kernel is the one from before sequences
    monkeypatch.setenv("MMHIP_FRAME_HOT", "0")
    k = pixel_kernel(mm.Filter(src, intersample=intersample))
    assert "hotf(" not in k and "mm_hot" not in k and "mm_orig_val_d(" in k


def test_frame_constant_sites_get_a_frame_view_per_work_item():
    # one frame per image: the hot test takes the frame number (it sets the descriptor's hot pointer), the fetch none
    k = pixel_kernel(mm.Filter(P.text(P.SELECT, P.FRAME_OF_ANIMATION)))
    tests = re.findall(r"mm_hot = mm_hot && mm_fetch_is_hot\((\w+), \(int\)\((\w+)\)\);", k)
    assert len(tests) == 1 and tests[0][0].endswith("_desc")
    assert "mm_orig_val_sums_hot(A, " in k and "hotf(" not in k and "mm_frame_view" not in k
    # three frames of one image: a view per site, each tested with its own frame number and read by its own fetch
    k = pixel_kernel(mm.Filter(P.BLEND))
    views = re.findall(r"const mm_image_desc (mm_fv\d) = mm_frame_view\((\w+_desc)\);", k)
    assert [v for v, _ in views] == ["mm_fv0", "mm_fv1", "mm_fv2"] and len({d for _, d in views}) == 1
    tests = re.findall(r"mm_hot = mm_hot && mm_fetch_is_hot\((mm_fv\d), \(int\)\((\w+)\)\);", k)
    assert [v for v, _ in tests] == ["mm_fv0", "mm_fv1", "mm_fv2"] and len({f for _, f in tests}) == 3
    hot = k.split("if (mm_hot) {", 1)[1].split("if (mm_bad) break;", 1)[0]
    assert [m for m in re.findall(r"mm_orig_val_hot\(A, [^;]*, (mm_fv\d), mm_bad\)", hot)] == ["mm_fv0", "mm_fv1", "mm_fv2"]


@pytest.mark.parametrize("intersample,pixel_inc", [(False, 1), (True, 1), (True, 3)])      # (the stride is the bilinear fetch's)
def test_slit_scan_compiles_for_gfx950(intersample, pixel_inc):
    flt = mm.Filter(P.text(P.SLIT, P.SLIT_FRAME), intersample=intersample, pixel_inc=pixel_inc)
    assert flt.jit(load=False) > 0


def test_blend_and_recursive_probes_compile_for_gfx950():
    for src in (P.BLEND, P.text(P.RECURSIVE, "n - 8"), P.text(P.CLOSURE, "n - 8")):
        assert mm.Filter(src).jit(load=False) > 0


# ---- the existing workloads' generated code ----

def test_generated_bodies_of_the_probe_filters_equal_the_parent_commits():
    with open(os.path.join(ROOT, "tests", "golden", "kernel_body_digests.json")) as f:
        golden = json.load(f)["body_sha256"]
    assert sorted(golden) == sorted("%s/%s" % (n, m) for n in PROBES for m in ("nearest", "bilinear"))
    assert digests() == golden


def test_body_text_is_the_part_after_the_prelude():
    src = F.load("ident").kernel_source
    body = body_text(src)
    assert " mm_prologue(mm_args A" in body and " mm_pixels(mm_args A" in body
    assert "MM_DEV color_t mm_get_pixel_cold" in src and "MM_DEV color_t mm_get_pixel_cold" not in body
    assert hashlib.sha256(body.encode()).hexdigest() == digests()["ident/bilinear"]
