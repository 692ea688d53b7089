"""Supersampled clips (mmhip_render_clip_supersampled) without a GPU: the entry points and their argument checks, the
arithmetic that cuts a clip into batches, the Python wrapper's argument errors, the combine kernel's word arithmetic
(csrc/mm_ss_combine.h, compiled for the host) against the per-byte formula, and that no kernel text changed."""
import ctypes as C
import hashlib
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile

import pytest

import mathmap_amd as mm
from mathmap_amd._lib import lib
from mathmap_amd.api import CLIP_SS_PLAN_FIELDS
from tests import filters as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(1, 1), (3, 1), (4, 2), (333, 207), (512, 512), (1920, 1080), (8192, 8192)]


def err():
    return lib().mmhip_last_error().decode()


# ---- entry points ----

def test_entry_points_exist_and_are_declared():
    header = open(os.path.join(ROOT, "include", "mmhip.h")).read()
    for name in ("mmhip_render_clip_supersampled", "mmhip_filter_clip_supersample_plan", "mmhip_clip_supersampled_batches"):
        assert hasattr(lib(), name), name
        assert re.search(r"\b%s\s*\(" % name, header), name
    assert re.search(r"MMHIP_CLIP_SS_PLAN_FIELDS\s*=\s*%d\b" % len(CLIP_SS_PLAN_FIELDS), header)
    assert hasattr(mm.Filter, "clip_supersample_plan") and hasattr(mm.api.Invocation, "clip_supersampled_batches")
    assert "Supersampling is not batched" not in header


def test_the_call_refuses_bad_arguments_with_a_message():
    """mmhip_render_clip's errors, checked before anything touches the invocation: a null one will do."""
    frames = (C.c_int * 2)(0, 1)
    ts = (C.c_float * 2)(0.0, 0.5)

    def refused(num_frames, fr, tt, row_stride, frame_stride, bpp=4):
        rc = lib().mmhip_render_clip_supersampled(None, num_frames, fr, tt, 0, 0, 64, 32, None, row_stride, frame_stride, bpp, None)
        assert rc != 0
        return err()

    assert "num_frames" in refused(0, frames, ts, 256, 8192)
    assert "num_frames" in refused(-3, frames, ts, 256, 8192)
    assert "frames and ts" in refused(2, None, ts, 256, 8192)
    assert "frames and ts" in refused(2, frames, None, 256, 8192)
    assert "bpp" in refused(2, frames, ts, 256, 8192, bpp=5)
    assert "bpp" in refused(2, frames, ts, 256, 8192, bpp=0)
    assert "frame_stride" in refused(2, frames, ts, 256, 8191)      # 32 rows of 256 bytes: one byte short
    assert "frame_stride" in refused(2, frames, ts, 300, 31 * 300 + 255)


def test_plan_refuses_bad_arguments():
    flt = F.load("ident")
    with pytest.raises(mm.MathMapError, match="num_frames"):
        flt.clip_supersample_plan(64, 64, 0)
    with pytest.raises(mm.MathMapError, match="empty region"):
        flt.clip_supersample_plan(0, 64, 3)
    with pytest.raises(mm.MathMapError, match="bpp"):
        flt.clip_supersample_plan(64, 64, 3, bpp=5)


def test_python_argument_errors():
    """The single-frame supersampled render has neither float maps nor row bands: refused before anything else is looked
    at (an invocation needs a GPU; the check does not, so an unbound one will do)."""
    inv = mm.api.Invocation.__new__(mm.api.Invocation)
    with pytest.raises(ValueError, match="floatmap"):
        inv.render_clip(num_frames=2, supersample=True, floatmap=True)
    with pytest.raises(ValueError, match="rows"):
        inv.render_clip(num_frames=2, supersample=True, rows=(0, 16))
    with pytest.raises(ValueError):
        inv.render_clip(num_frames=2, supersample=True, rows=(0, 16), out_ptr=4096)


# ---- plan arithmetic ----

@pytest.mark.parametrize("name", ["ident", "pond", "mandelbrot", "droste"])
def test_plan_arithmetic(name):
    flt = F.load(name, supersampling=True)
    for w, h in SHAPES:
        for bpp in (1, 2, 3, 4):
            for frames in (1, 7, 120):
                p = flt.clip_supersample_plan(w, h, frames, bpp=bpp)
                assert set(p) == set(CLIP_SS_PLAN_FIELDS)
                assert p["long_pitch"] % 16 == 0 and (w + 1) * bpp <= p["long_pitch"] < (w + 1) * bpp + 16, (w, h, bpp)
                assert p["bytes_per_frame"] == h * (p["long_pitch"] + w * bpp)
                assert p["rows_per_item"] >= 1 and p["pixels_per_item"] == 4
                # the largest batch the caps allow: the frames asked for, the byte budget (2 GiB), either slice's launch cap
                caps = [frames, 65535, (2 << 30) // p["bytes_per_frame"],
                        flt.clip_batch_plan(w + 1, h, frames)["frames_per_batch"], flt.clip_batch_plan(w, h, frames)["frames_per_batch"]]
                assert p["batched"] == 1 and p["frames_per_batch"] == min(caps), (name, w, h, bpp, frames, p, caps)
                assert p["batches"] == -(-frames // p["frames_per_batch"])
    # an 8192 x 8192 RGBA frame's slices are about 0.54 GB: three frames per batch
    p = flt.clip_supersample_plan(8192, 8192, 120)
    assert p["bytes_per_frame"] == 8192 * (32784 + 32768) and p["frames_per_batch"] == 3 and p["batches"] == 40


def test_the_launch_caps_hold_at_the_batch_actually_launched():
    """Fewer frames per launch can mean fewer rows per work-item and more workgroups: the cap is taken at the batch's own
    size, so that each nested clip call stays one launch."""
    flt = F.load("ident", supersampling=True)
    for w, h, frames in ((4096, 16, 200000), (96, 64, 70000), (17, 5, 65535)):
        p = flt.clip_supersample_plan(w, h, frames, bpp=1)
        per = p["frames_per_batch"]
        assert 1 <= per <= 65535
        for width in (w, w + 1):
            assert flt.clip_batch_plan(width, h, per)["frames_per_batch"] >= per, (w, h, frames, width)


def test_filters_with_native_calls_or_closures_take_the_loop():
    for name in ("gauss_direct", "closure_timed_arg"):
        p = F.load(name, supersampling=True).clip_supersample_plan(160, 121, 3)
        assert p["batched"] == 0 and p["frames_per_batch"] == 0 and p["batches"] == 0, name
        assert p["bytes_per_frame"] == 121 * (p["long_pitch"] + 160 * 4)


def test_batch_caps_from_the_environment():
    """MMHIP_CLIP_SS_BYTES and MMHIP_CLIP_MAX_FRAMES are read once per process: a child process each."""
    prog = ("import json, sys; sys.path.insert(0, %r); from tests import filters as F; f = F.load('ident', supersampling=True); "
            "print(json.dumps([f.clip_supersample_plan(333, 207, n) for n in (1, 3, 7, 120)]))" % ROOT)
    bpf = 207 * (1344 + 1332)
    assert F.load("ident", supersampling=True).clip_supersample_plan(333, 207, 7)["bytes_per_frame"] == bpf
    cases = [
        ({"MMHIP_CLIP_SS_BYTES": str(3 * bpf + 100)}, [(1, 1, 1), (1, 1, 3), (1, 3, 3), (1, 40, 3)]),
        ({"MMHIP_CLIP_SS_BYTES": str(bpf)}, [(1, 1, 1), (1, 3, 1), (1, 7, 1), (1, 120, 1)]),      # one frame per batch is still batched
        ({"MMHIP_CLIP_SS_BYTES": str(bpf - 1)}, [(0, 0, 0)] * 4),                                  # not even one frame fits: the loop
        ({"MMHIP_CLIP_MAX_FRAMES": "2"}, [(1, 1, 1), (1, 2, 2), (1, 4, 2), (1, 60, 2)]),
        ({"MMHIP_CLIP_SS_BYTES": "junk"}, [(1, 1, 1), (1, 1, 3), (1, 1, 7), (1, 1, 120)]),         # not a positive number: the default
    ]
    for extra, want in cases:
        env = dict(os.environ, **extra)
        out = subprocess.run([sys.executable, "-c", prog], env=env, check=True, capture_output=True, text=True).stdout
        plans = json.loads(out.strip().splitlines()[-1])
        assert [(p["batched"], p["batches"], p["frames_per_batch"]) for p in plans] == want, extra


# ---- the combine's word arithmetic, compiled for the host ----

ARITHMETIC = r'''
#include <stdio.h>
#include <stdint.h>
#include "mm_ss_combine.h"

static uint32_t lcg = 12345u;
static uint32_t next_word(void) {          /* two steps of a 32-bit LCG, high halves: every bit varies */
    lcg = lcg * 1664525u + 1013904223u;
    const uint32_t hi = lcg >> 16;
    lcg = lcg * 1664525u + 1013904223u;
    return (hi << 16) | (lcg >> 16);
}
static unsigned byte_of(uint32_t w, int k) { return (w >> (8 * k)) & 255u; }

/* the plain formula per byte lane against the word functions, for texels a b (long row r), c (short row), d e (long row r + 1) */
static long check(uint32_t a, uint32_t b, uint32_t c, uint32_t d, uint32_t e) {
    const uint32_t got = mm_ss_combine_word(mm_ss_pair_sum(a, b), mm_ss_pair_sum(d, e), c);
    long bad = 0;
    for (int k = 0; k < 4; ++k) {
        const unsigned want = (byte_of(a, k) + byte_of(b, k) + 2 * byte_of(c, k) + byte_of(d, k) + byte_of(e, k)) / 6;
        bad += byte_of(got, k) != want;
    }
    return bad;
}

int main(void) {
    long bad = 0, cases = 0;
    /* every sum 0 .. 1530: the divide alone, then through the word functions in each byte lane, the other lanes at 0 and at 255 */
    for (unsigned v = 0; v <= 1530; ++v) {
        bad += mm_ss_div6(v) != v / 6;
        bad += mm_ss_div6_halves(v | (v << 16)) != ((v / 6) | ((v / 6) << 16));
        /* split v into five bytes with weights 1 1 2 1 1 */
        unsigned rest = v, t[5];
        const unsigned weight[5] = {1, 1, 2, 1, 1};
        for (int i = 0; i < 5; ++i) {
            t[i] = rest / weight[i] > 255 ? 255 : rest / weight[i];
            rest -= t[i] * weight[i];
        }
        bad += rest != 0;        /* every v is five bytes' weighted sum */
        for (int k = 0; k < 4; ++k)
            for (unsigned other = 0; other <= 255; other += 255) {
                uint32_t w[5];
                for (int i = 0; i < 5; ++i) {
                    w[i] = other * 0x01010101u;
                    w[i] = (w[i] & ~(255u << (8 * k))) | (t[i] << (8 * k));
                }
                bad += check(w[0], w[1], w[2], w[3], w[4]);
                ++cases;
            }
    }
    /* corner values */
    const uint32_t corner[] = {0u, 255u, 0xffffffffu, 0x00ff00ffu, 0xff00ff00u, 0xff000000u, 0x01010101u, 0xfefefefeu};
    const int n = (int)(sizeof corner / sizeof corner[0]);
    for (int a = 0; a < n; ++a) for (int b = 0; b < n; ++b) for (int c = 0; c < n; ++c) for (int d = 0; d < n; ++d) for (int e = 0; e < n; ++e) {
        bad += check(corner[a], corner[b], corner[c], corner[d], corner[e]);
        ++cases;
    }
    for (int i = 0; i < 1000000; ++i) {
        const uint32_t a = next_word(), b = next_word(), c = next_word(), d = next_word(), e = next_word();
        bad += check(a, b, c, d, e);
        ++cases;
    }
    printf("%ld %ld\n", bad, cases);
    return bad != 0;
}
'''


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan-ubsan"])
def test_word_arithmetic_is_the_per_byte_formula(sanitize):
    """A stand-alone host program over the header the kernel includes: every sum 0 .. 1530 in each byte lane, the corner
    values, and 10^6 random word quintuples -- 0 differences.  Once more under the address and undefined-behaviour
    sanitizers (host code only)."""
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.cpp"), "w").write(ARITHMETIC)
        flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else ["-O2"]
        subprocess.run([cxx, "-std=c++17", "-Wall", "-Werror"] + flags + ["-I", os.path.join(ROOT, "mathmap_amd", "csrc"), "-o",
                        os.path.join(d, "t"), os.path.join(d, "t.cpp")], check=True)
        r = subprocess.run([os.path.join(d, "t")], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, (r.stdout, r.stderr[-2000:])
    bad, cases = (int(x) for x in r.stdout.split())
    assert bad == 0 and cases > 1000000 + 8 ** 5 + 1000


def test_the_kernel_includes_the_header_the_test_compiles():
    text = open(os.path.join(ROOT, "mathmap_amd", "csrc", "clip_combine.hip")).read()
    assert '#include "mm_ss_combine.h"' in text and "mm_ss_combine_word(" in text and "k_supersample_combine_clip" in text


# ---- nothing else changed ----

def test_kernel_texts_are_the_parents():
    with open(os.path.join(ROOT, "tests", "golden", "clip_text_digests.json")) as f:
        want = json.load(f)["filters"]
    for name, digests in want.items():
        flt = F.load(name)
        assert hashlib.sha256(flt.clip_kernel_source.encode()).hexdigest() == digests["clip_kernel_source_sha256"], name
        assert hashlib.sha256(flt.kernel_source.encode()).hexdigest() == digests["kernel_source_sha256"], name
    from tools.kernel_body_digest import digests as body_digests
    with open(os.path.join(ROOT, "tests", "golden", "kernel_body_digests.json")) as f:
        golden = json.load(f)["body_sha256"]
    assert body_digests() == golden
