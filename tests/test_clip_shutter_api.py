"""Motion-blurred clips (mmhip_render_clip_shutter) without a GPU: the entry points and their argument checks, the Python
wrapper's argument errors, the times of the sub-samples, the arithmetic that cuts a clip into batches and passes, the
combine kernel's per-pixel arithmetic (csrc/mm_shutter_combine.h, compiled for the host) against the NumPy restatement
of tests/shutter_reference.py, the command line's help, and that no kernel text changed."""
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
from tests import shutter_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "mathmap_amd", "mathmap_hip_cli")
f32 = np.float32


def err():
    return lib().mmhip_last_error().decode()


# ---- entry points ----

def test_entry_points_exist_and_are_declared():
    header = open(os.path.join(ROOT, "include", "mmhip.h")).read()
    for name in ("mmhip_render_clip_shutter", "mmhip_filter_clip_shutter_plan", "mmhip_clip_shutter_batches"):
        assert hasattr(lib(), name), name
        assert re.search(r"\b%s\s*\(" % name, header), name
    from mathmap_amd.api import CLIP_SHUTTER_PLAN_FIELDS, SHUTTER_MAX_SAMPLES
    assert re.search(r"MMHIP_SHUTTER_MAX_SAMPLES\s*=\s*256\b", header) and SHUTTER_MAX_SAMPLES == 256
    assert re.search(r"MMHIP_CLIP_SHUTTER_PLAN_FIELDS\s*=\s*%d\b" % len(CLIP_SHUTTER_PLAN_FIELDS), header)
    assert len(CLIP_SHUTTER_PLAN_FIELDS) == 6
    assert hasattr(mm.Filter, "clip_shutter_plan") and hasattr(mm.api.Invocation, "clip_shutter_batches")
    assert callable(mm.api.shutter_sample_ts)


def test_the_header_states_the_semantics():
    header = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "mmhip.h")).read())
    for phrase in ("t_ij = (float)((double)ts[i] + ((double)span * (double)j) / (double)K)",
                   "acc = f_0; acc = acc + f_j",
                   "inv_k = (float)(1.0 / (double)K)",
                   "no fma", "denormals kept",
                   "frames[i] -- the same for every j",
                   "samples = 1 is mmhip_render_clip",
                   "Bytes between rows and between frames are not touched",
                   "MMHIP_CLIP_SHUTTER_BYTES",
                   "Not combined with supersampling",
                   "shutter_combine_clip"):
        assert phrase in header, phrase


def test_the_call_refuses_bad_arguments_with_a_message():
    """Checked before anything touches the invocation: a null one will do."""
    frames = (C.c_int * 2)(0, 1)
    ts = (C.c_float * 2)(0.0, 0.5)

    def refused(samples=4, span=0.1, num_frames=2, fr=frames, tt=ts, row_stride=256, frame_stride=8192, bpp=4):
        rc = lib().mmhip_render_clip_shutter(None, num_frames, fr, tt, samples, span, 0, 0, 64, 32, 0, 32, None, row_stride,
                                             frame_stride, bpp, 0, None)
        assert rc != 0
        return err()

    for samples in (0, -1, 257):
        msg = refused(samples=samples)
        assert "samples" in msg and "256" in msg and str(samples) in msg, msg
    for span in (float("nan"), float("inf"), float("-inf")):
        assert "span" in refused(span=span)
    # mmhip_render_clip's own, with several sub-samples and with one (the call is mmhip_render_clip then)
    for samples in (4, 1):
        assert "num_frames" in refused(samples=samples, num_frames=0)
        assert "num_frames" in refused(samples=samples, num_frames=-3)
        assert "frames and ts" in refused(samples=samples, fr=None)
        assert "frames and ts" in refused(samples=samples, tt=None)
        assert "bpp" in refused(samples=samples, bpp=5)
        assert "bpp" in refused(samples=samples, bpp=0)
        assert "frame_stride" in refused(samples=samples, frame_stride=8191)      # 32 rows of 256 bytes: one byte short
        assert "frame_stride" in refused(samples=samples, row_stride=300, frame_stride=31 * 300 + 255)


def test_plan_refuses_bad_arguments():
    flt = F.load("ident")
    with pytest.raises(mm.MathMapError, match="num_frames"):
        flt.clip_shutter_plan(64, 64, 64, 4, 0)
    with pytest.raises(mm.MathMapError, match="region"):
        flt.clip_shutter_plan(0, 64, 64, 4, 3)
    with pytest.raises(mm.MathMapError, match="region"):
        flt.clip_shutter_plan(65, 64, 64, 4, 3)
    for samples in (0, -1, 257):
        with pytest.raises(mm.MathMapError, match="samples"):
            flt.clip_shutter_plan(64, 64, 64, samples, 3)


def test_python_argument_errors():
    """Refused before anything else is looked at (an invocation needs a GPU; the checks do not, so an unbound one will do)."""
    inv = mm.api.Invocation.__new__(mm.api.Invocation)
    with pytest.raises(ValueError, match="supersample"):
        inv.render_clip(num_frames=2, supersample=True, shutter_samples=4, shutter=0.5)
    with pytest.raises(ValueError, match="not both"):
        inv.render_clip(num_frames=2, shutter_samples=4, shutter=0.5, shutter_span=0.1)
    with pytest.raises(ValueError, match="shutter is a fraction"):
        inv.render_clip(frames=[0, 1], ts=[0.0, 0.5], shutter_samples=4, shutter=0.5)
    with pytest.raises(ValueError, match="shutter is a fraction"):
        inv.render_clip(num_frames=2, frames=[0, 1], ts=[0.0, 0.5], shutter_samples=4, shutter=0.5)
    with pytest.raises(ValueError, match="needs shutter"):
        inv.render_clip(num_frames=2, shutter_samples=4)
    with pytest.raises(ValueError):
        mm.api.shutter_sample_ts([0.0], 0, 0.1)
    with pytest.raises(ValueError):
        mm.api.shutter_sample_ts([0.0], 257, 0.1)


# ---- the times of the sub-samples ----

def test_shutter_sample_ts_is_the_formula():
    rng = np.random.default_rng(11)
    cases = [(rng.random(50).astype(f32), k, f32(span)) for k in (1, 2, 3, 4, 7, 8, 17, 256) for span in (0.07, -0.3, 0.0, 1.0 / 3.0, 1e-8, 5.0)]
    near_one = np.array([1.0, np.nextafter(f32(1), f32(0)), np.nextafter(f32(1), f32(2)), 0.99999, 0.0, -0.0, 1e-30, -2.5, 119.0 / 120.0], f32)
    cases += [(near_one, k, f32(span)) for k in (3, 7, 256) for span in (-1.0 / 120.0, 0.5 / 120.0, 1e-7, np.nextafter(f32(0), f32(1)))]
    for ts, k, span in cases:
        got = mm.api.shutter_sample_ts(ts, k, span)
        want = R.sample_ts(ts, k, span)
        assert got.dtype == np.float32 and got.shape == (len(ts), k)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (k, span)
    # a Python float span is taken as the C float the call receives
    assert np.array_equal(mm.api.shutter_sample_ts([0.25], 7, 0.1), R.sample_ts([0.25], 7, f32(0.1)))
    # product before quotient, in double: not ts + span * (j / K) in float
    t = R.sample_ts([f32(0.1)], 3, f32(0.1))
    assert t[0, 1] == f32(np.float64(f32(0.1)) + np.float64(f32(0.1)) * 1.0 / 3.0)


# ---- plan arithmetic (MMHIP_CLIP_SHUTTER_BYTES is read once per process: a child process each) ----

def test_plan_with_the_default_budget():
    flt = F.load("ident")
    from mathmap_amd.api import CLIP_SHUTTER_PLAN_FIELDS
    for w, rows, rw, k, n in ((97, 61, 97, 4, 3), (50, 20, 97, 8, 120), (1920, 1080, 1920, 4, 2), (8192, 8192, 8192, 8, 5), (1, 1, 1, 256, 70000)):
        p = flt.clip_shutter_plan(w, rows, rw, k, n)
        assert set(p) == set(CLIP_SHUTTER_PLAN_FIELDS)
        bps = rows * 16 * rw
        assert p["bytes_per_sample"] == bps
        per = min((8 << 30) // (k * bps), 65535, n)
        assert per >= 1
        assert (p["frames_per_batch"], p["batches"], p["samples_per_pass"], p["passes"], p["carry"]) == (per, -(-n // per), k, 1, 0), (w, rows, rw, k, n, p)
    # 8192^2 with 8 sub-samples: 1 GiB per sub-sample, one frame per batch
    assert flt.clip_shutter_plan(8192, 8192, 8192, 8, 5)["frames_per_batch"] == 1
    assert flt.clip_shutter_plan(8192, 8192, 8192, 4, 5)["frames_per_batch"] == 2


def test_plan_under_a_budget_from_the_environment():
    bps = 61 * 16 * 97
    prog = ("import json, sys; sys.path.insert(0, %r); from tests import filters as F; f = F.load('ident'); "
            "print(json.dumps([f.clip_shutter_plan(97, 61, 97, k, n) for k, n in ((4, 1), (4, 7), (8, 7), (17, 3))]))" % ROOT)

    def key(p):
        assert p["bytes_per_sample"] == bps
        return (p["frames_per_batch"], p["batches"], p["samples_per_pass"], p["passes"], p["carry"])

    cases = [
        # many frames per batch: 12 sub-samples fit -- 3 frames of 4, 1 of 8; 17 do not fit: passes of 11 beside the carry
        (12 * bps + 100, [(1, 1, 4, 1, 0), (3, 3, 4, 1, 0), (1, 7, 8, 1, 0), (1, 3, 11, 2, 1)]),
        # exactly one frame of 4; 8 and 17 are cut into passes of 3 (one slot goes to the carry map)
        (4 * bps, [(1, 1, 4, 1, 0), (1, 7, 4, 1, 0), (1, 7, 3, 3, 1), (1, 3, 3, 6, 1)]),
        # one byte short of a frame of 4: passes of 2
        (4 * bps - 1, [(1, 1, 2, 2, 1), (1, 7, 2, 2, 1), (1, 7, 2, 4, 1), (1, 3, 2, 9, 1)]),
        # the soft minimum: two maps, one map, less than one map -- one sub-sample per pass beside the carry
        (2 * bps, [(1, 1, 1, 4, 1), (1, 7, 1, 4, 1), (1, 7, 1, 8, 1), (1, 3, 1, 17, 1)]),
        (bps, [(1, 1, 1, 4, 1), (1, 7, 1, 4, 1), (1, 7, 1, 8, 1), (1, 3, 1, 17, 1)]),
        (1, [(1, 1, 1, 4, 1), (1, 7, 1, 4, 1), (1, 7, 1, 8, 1), (1, 3, 1, 17, 1)]),
        # not a positive number: the default
        ("junk", [(1, 1, 4, 1, 0), (7, 1, 4, 1, 0), (7, 1, 8, 1, 0), (3, 1, 17, 1, 0)]),
    ]
    for budget, want in cases:
        env = dict(os.environ, MMHIP_CLIP_SHUTTER_BYTES=str(budget))
        out = subprocess.run([sys.executable, "-c", prog], env=env, check=True, capture_output=True, text=True).stdout
        plans = json.loads(out.strip().splitlines()[-1])
        assert [key(p) for p in plans] == want, budget


# ---- the combine's per-pixel arithmetic, compiled for the host ----

ARITHMETIC = r'''
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "mm_shutter_combine.h"

/* in: K, then n pixels of K sub-samples of 4 floats.  out per pixel: the mean (4 floats), then the bytes at bpp 1, 2, 3, 4 (10) */
int main(int argc, char **argv) {
    if (argc != 5) return 2;
    const int k = atoi(argv[1]);
    const long n = atol(argv[2]);
    FILE *in = fopen(argv[3], "rb"), *out = fopen(argv[4], "wb");
    if (!in || !out || k < 1) return 2;
    float *f = (float *)malloc(sizeof(float) * 4 * k);
    const float inv_k = mm_shutter_inv_k(k);
    for (long p = 0; p < n; ++p) {
        if (fread(f, sizeof(float) * 4, k, in) != (size_t)k) return 3;
        float m[4];
        for (int c = 0; c < 4; ++c) {
            float acc = f[c];
            for (int j = 1; j < k; ++j) acc = mm_shutter_add(acc, f[4 * j + c]);
            m[c] = mm_shutter_scale(acc, inv_k);
        }
        unsigned char bytes[10];
        memset(bytes, 0xA5, sizeof bytes);
        mm_shutter_store_bytes(bytes, m[0], m[1], m[2], m[3], 1);
        mm_shutter_store_bytes(bytes + 1, m[0], m[1], m[2], m[3], 2);
        mm_shutter_store_bytes(bytes + 3, m[0], m[1], m[2], m[3], 3);
        mm_shutter_store_bytes(bytes + 6, m[0], m[1], m[2], m[3], 4);
        if (fwrite(m, sizeof(float), 4, out) != 4 || fwrite(bytes, 1, 10, out) != 10) return 4;
    }
    /* behind the pixels: the times of the k sub-samples for a fixed table of t and span */
    const float ts[] = {0.0f, 0.25f, 0.99999994f, 1.0f, -2.5f, 0.1f};
    const float spans[] = {0.07f, -0.3f, 0.0f, 0.0041666669f, 1e-8f};
    for (unsigned a = 0; a < sizeof ts / sizeof ts[0]; ++a)
        for (unsigned b = 0; b < sizeof spans / sizeof spans[0]; ++b)
            for (int j = 0; j < k; ++j) {
                const float t = mm_shutter_sample_t(ts[a], spans[b], j, k);
                if (fwrite(&t, sizeof t, 1, out) != 1) return 4;
            }
    free(f);
    fclose(in);
    return fclose(out) != 0;
}
'''
TIMES_T = np.array([0.0, 0.25, 0.99999994, 1.0, -2.5, 0.1], f32)
TIMES_SPAN = np.array([0.07, -0.3, 0.0, 0.0041666669, 1e-8], f32)


@pytest.fixture(scope="module")
def host_program():
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    d = tempfile.mkdtemp(prefix="mm_shutter_")
    open(os.path.join(d, "t.cpp"), "w").write(ARITHMETIC)
    built = {}

    def get(sanitize):
        if sanitize not in built:
            flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else ["-O2"]
            exe = os.path.join(d, "t_san" if sanitize else "t")
            subprocess.run([cxx, "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off"] + flags +
                           ["-I", os.path.join(ROOT, "mathmap_amd", "csrc"), "-o", exe, os.path.join(d, "t.cpp")], check=True)
            built[sanitize] = exe
        return d, built[sanitize]
    yield get
    shutil.rmtree(d, ignore_errors=True)


@pytest.mark.parametrize("k,sanitize", [(2, False), (3, False), (4, False), (5, False), (8, False), (17, False), (256, False), (5, True)],
                         ids=lambda v: str(v))
def test_header_arithmetic_is_the_restatement(host_program, k, sanitize):
    """A stand-alone host program over the header the kernel includes, on 10^5 random pixels and the special ones: the mean
    bit for bit (NaNs by position), the bytes at every bpp, the sub-sample times.  Once under the address and
    undefined-behaviour sanitizers (host code only)."""
    d, exe = host_program(sanitize)
    rng = np.random.default_rng(100 + k)
    n_random = 100000 if k <= 17 else 20000
    px = np.concatenate([rng.uniform(-0.25, 1.25, (n_random, k, 4)).astype(f32), R.special_pixels(k, rng)])
    n = len(px)
    src, dst = os.path.join(d, "in_%d.bin" % k), os.path.join(d, "out_%d.bin" % k)
    px.tofile(src)
    r = subprocess.run([exe, str(k), str(n), src, dst], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    raw = np.fromfile(dst, np.uint8)
    os.remove(src)
    os.remove(dst)
    rec = raw[:n * 26].reshape(n, 26)
    got_mean = rec[:, :16].copy().view(f32).reshape(n, 4)
    maps = px.transpose(1, 0, 2)                       # [k, n, 4]
    assert R.same_floats(got_mean, R.combine(maps, floatmap=True))
    at = 16
    for bpp in (1, 2, 3, 4):
        want = R.combine(maps, bpp=bpp)
        bad = np.flatnonzero((rec[:, at:at + bpp] != want).any(axis=1))
        assert bad.size == 0, (bpp, int(bad[0]), px[bad[0]].tolist(), rec[bad[0], at:at + bpp].tolist(), want[bad[0]].tolist())
        at += bpp
    times = raw[n * 26:].copy().view(f32).reshape(len(TIMES_T), len(TIMES_SPAN), k)
    for b, span in enumerate(TIMES_SPAN):
        assert np.array_equal(times[:, b, :].view(np.uint32), R.sample_ts(TIMES_T, k, span).view(np.uint32)), span


def test_the_restatement_on_values_worked_out_by_hand():
    # 0.1f + 0.2f + 0.3f in float32, in that order, times (float)(1/3)
    m = R.mean(np.array([[[0.1] * 4], [[0.2] * 4], [[0.3] * 4]], f32))
    assert m[0, 0] == f32(f32(f32(f32(0.1) + f32(0.2)) + f32(0.3)) * f32(1.0 / 3.0))
    # 1.0 is byte 255, the float below it 254; NaN and negatives are 0
    maps = np.array([[[1.0, np.nextafter(f32(1), f32(0)), np.nan, -0.5]]] * 2, f32)
    assert R.combine(maps, 4).tolist() == [[255, 254, 0, 0]]
    assert R.combine(maps, 3).tolist() == [[255, 254, 0]]
    grey = int((1.0 * 0.299 + float(np.nextafter(f32(1), f32(0))) * 0.587 + 0.0 * 0.114) * 255.0)
    assert R.combine(maps, 2).tolist() == [[grey, 0]] and R.combine(maps, 1).tolist() == [[grey]]
    # the sum overflows: inf, byte 255
    assert R.combine(np.full((2, 1, 4), 3e38, f32), 4).tolist() == [[255] * 4]
    # two halves of the smallest normal number
    assert R.mean(np.full((2, 1, 4), 5.877472e-39, f32))[0, 0] == f32(5.877472e-39)


def test_the_kernel_includes_the_header_the_test_compiles():
    text = open(os.path.join(ROOT, "mathmap_amd", "csrc", "clip_combine.hip")).read()
    assert '#include "mm_shutter_combine.h"' in text and "k_shutter_combine_clip" in text
    for fn in ("mm_shutter_add(", "mm_shutter_scale(", "mm_shutter_store_bytes("):
        assert fn in text, fn
    runtime = open(os.path.join(ROOT, "mathmap_amd", "csrc", "runtime_clip.cpp")).read()
    assert "mm_shutter_sample_t(" in runtime and "mm_shutter_inv_k(" in runtime
    makefile = open(os.path.join(ROOT, "mathmap_amd", "csrc", "Makefile")).read()
    assert re.search(r"HIPFLAGS\s*=.*-ffp-contract=off", makefile)


# ---- the command line ----

def test_cli_help_names_the_options():
    p = subprocess.run([CLI, "--help"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=60)
    assert p.returncode == 0
    assert "--shutter-samples=K" in p.stdout and "--shutter=FRACTION" in p.stdout


def test_cli_refuses_bad_shutter_options(tmp_path):
    src = "filter f () rgba:[t, 0, 0, 1] end"
    for extra, word in ((["--shutter-samples=0"], "--shutter-samples"), (["--shutter-samples=257"], "--shutter-samples"),
                        (["--shutter-samples=x"], "--shutter-samples"), (["--shutter-samples=4", "--shutter=nan"], "--shutter"),
                        (["--shutter-samples=4", "--shutter=fast"], "--shutter"), (["-o", "--shutter-samples=4"], "-o")):
        p = subprocess.run([CLI, "-F", "3", "-s", "8x8"] + extra + [src, str(tmp_path / "f%d.png")], stdout=subprocess.PIPE,
                           stderr=subprocess.PIPE, text=True, timeout=60)
        assert p.returncode != 0 and word in p.stderr, (extra, p.stderr)
    assert not list(tmp_path.iterdir())


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
