"""Float32 input drawables without a GPU (mmhip_options.deep_inputs, mmhip_set_image_sequence_float_*, include/mmhip.h):
the option's place in the options struct and its way through every compile entry point, its refusals, the kernel text
with and without it, the new symbols, the setters' refusals that need no device, the Python dtype dispatch, the probes
compiled for gfx950, and the restatement tests/deep_fetch_reference.py against tests/fetch_reference.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import mathmap_amd as mm
from mathmap_amd import _lib
from mathmap_amd._lib import Options, lib
from tests import deep_fetch_reference as D
from tests import fetch_reference as R
from tests import filters as F
from tests.test_gauss_mode_options import OLD_OFFSETS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCALED = "filter scaled (image in, float k: 0-2 (1))\n  in(xy * k, frame)\nend\n"
DEFINE = "#define MM_DEEP_INPUTS 1\n"


def err():
    return lib().mmhip_last_error().decode()


# ---- the option ----

def test_the_option_takes_the_first_reserved_int():
    assert C.sizeof(Options) == 52
    for name, off in OLD_OFFSETS.items():
        if name != "reserved":
            assert getattr(Options, name).offset == off, name
    assert Options.gauss_mode.offset == 28 and Options.deep_inputs.offset == 32
    assert Options.reserved.offset == 36 and Options.reserved.size == 16
    header = " ".join(open(os.path.join(ROOT, "include", "mmhip.h")).read().split())
    assert re.search(r"int gauss_mode; /\*.*?\*/ int deep_inputs; /\*.*?\*/ int reserved\[4\]; \} mmhip_options;", header)
    o = Options()
    o.deep_inputs = 7
    lib().mmhip_default_options(C.byref(o))
    assert o.deep_inputs == 0
    assert mm.Filter(SCALED).deep_inputs is False


@pytest.mark.parametrize("deep", [False, True])
def test_the_option_survives_every_compile_path(deep):
    flt = mm.Filter(SCALED, deep_inputs=deep)
    paths = {"source": flt,
             "specialised, source origin": flt.specialized({"k": 0.5}),
             "constants=": mm.Filter(SCALED, deep_inputs=deep, constants={"k": 0.5}),
             "IR": mm.Filter(ir_json=flt.ir_json_raw, deep_inputs=deep),
             "specialised, IR origin": mm.Filter(ir_json=flt.ir_json_raw, deep_inputs=deep).specialized({"k": 0.5}),
             "IR, constants=": mm.Filter(ir_json=flt.ir_json_raw, deep_inputs=deep, constants={"k": 0.5}),
             "the reference's example, from its IR": F.load("pond", deep_inputs=deep),
             "specialize=True": mm.Filter(SCALED, deep_inputs=deep, specialize=True)}
    for name, f in paths.items():
        assert f.deep_inputs is deep, name
        texts = [f.kernel_source, f.clip_kernel_source]
        if name != "the reference's example, from its IR":
            texts += [f.shutter_kernel_source, f.sampled_kernel_source, f.refine_kernel_source]
        for text in texts:
            assert (text.count(DEFINE) == 1) == deep and ("MM_DEEP_INPUTS" in text) == deep, name


@pytest.mark.parametrize("bad", [2, -1, 100])
def test_other_values_are_refused_by_every_compile_entry_point(bad):
    o = Options()
    lib().mmhip_default_options(C.byref(o))
    o.deep_inputs = bad
    raw = mm.Filter(SCALED).ir_json_raw
    assert not lib().mmhip_compile(SCALED.encode(), C.byref(o))
    assert "deep_inputs %d is neither 0 nor 1" % bad in err()
    assert not lib().mmhip_compile_ir_json(raw.encode(), C.byref(o))
    assert "deep_inputs %d is neither 0 nor 1" % bad in err()
    assert not lib().mmhip_compile_specialized(SCALED.encode(), C.byref(o), 0, None, None)
    assert "deep_inputs %d is neither 0 nor 1" % bad in err()


@pytest.mark.parametrize("inc", [2, 3])
def test_the_preview_stride_is_refused_with_the_option(inc):
    o = Options()
    lib().mmhip_default_options(C.byref(o))
    o.deep_inputs, o.pixel_inc = 1, inc
    raw = mm.Filter(SCALED).ir_json_raw
    for compiled in (lib().mmhip_compile(SCALED.encode(), C.byref(o)), lib().mmhip_compile_ir_json(raw.encode(), C.byref(o)),
                     lib().mmhip_compile_specialized(SCALED.encode(), C.byref(o), 0, None, None)):
        assert not compiled
        assert "deep_inputs with pixel_inc %d" % inc in err()
    with pytest.raises(mm.MathMapError, match="deep_inputs with pixel_inc"):
        mm.Filter(SCALED, deep_inputs=True, pixel_inc=inc)
    assert mm.Filter(SCALED, deep_inputs=True, pixel_inc=1).deep_inputs          # 0 and 1 are no stride
    assert mm.Filter(SCALED, pixel_inc=inc).deep_inputs is False


@pytest.mark.parametrize("name", ["ident", "pond", "droste", "mandelbrot", "gauss_direct", "closure_timed_arg"])
def test_the_text_without_the_option_is_the_plain_filters(name):
    """Off, the option leaves no trace; on, the text is the plain one with the define in front of the prelude and the
    prelude's two MM_DEEP_INPUTS regions -- the IR is the same either way."""
    plain, off, on = F.load(name), F.load(name, deep_inputs=False), F.load(name, deep_inputs=True)
    assert plain.kernel_source == off.kernel_source and plain.clip_kernel_source == off.clip_kernel_source
    assert "MM_DEEP_INPUTS" not in plain.kernel_source and "MM_IMG_DEEP" not in plain.kernel_source
    assert plain.ir_json == on.ir_json
    text = on.kernel_source
    assert text.count(DEFINE) == 1 and text.index(DEFINE) < text.index("#ifndef MM_DEVICE_H")
    cut = re.sub(r"^#if MM_DEEP_INPUTS\n.*?^#endif  // MM_DEEP_INPUTS\n", "", text.replace(DEFINE, "", 1), flags=re.M | re.S)
    assert cut == plain.kernel_source
    assert text.count("#if MM_DEEP_INPUTS\n") == 2 and text.count("d.kind == MM_IMG_DEEP") == 1
    body = text[text.index("#endif  // MM_DEVICE_H"):]
    assert body == plain.kernel_source[plain.kernel_source.index("#endif  // MM_DEVICE_H"):]


def test_the_hook_is_in_one_place():
    prelude = open(os.path.join(ROOT, "mathmap_amd", "csrc", "mm_device.h")).read()
    assert prelude.count("MM_IMG_DEEP") == 2          # the enum and the branch
    hook = prelude[prelude.index("MM_DEV mm_tup<4> mm_orig_val_d("):prelude.index("// The fetch of the kernel's hot variant")]
    assert ("    if (d.kind == MM_IMG_FLOATMAP) return mm_floatmap_pixel(d, x, y);\n#if MM_DEEP_INPUTS\n"
            "    if (d.kind == MM_IMG_DEEP) return mm_orig_val_deep(A, d, x, y, mm_f2i(f));\n#endif  // MM_DEEP_INPUTS\n") in hook
    assert "return d.kind == MM_IMG_DRAWABLE &&" in prelude          # mm_fetch_is_hot_any: a deep image is never hot
    deep = prelude[prelude.index("#if MM_DEEP_INPUTS\n"):prelude.index("#endif  // MM_DEEP_INPUTS\n")]
    code = re.sub(r"//[^\n]*", "", deep)          # the code of the region, without its comments
    assert "rintf" not in code and "255" not in code and "fma" not in code and "__fmul_rn" in code and "__fadd_rn" in code
    host = open(os.path.join(ROOT, "mathmap_amd", "csrc", "mm_host_abi.h")).read()
    assert "IMG_DRAWABLE = 0, IMG_FLOATMAP = 1, IMG_NULL = 2, IMG_DEEP = 3" in host and "enum { MM_IMG_DEEP = 3 };" in prelude
    assert "static_assert(sizeof(HImageDesc) == 56" in host


# ---- the entry points ----

def test_entry_points_exist_and_are_declared():
    flat = " ".join(open(os.path.join(ROOT, "include", "mmhip.h")).read().split())
    assert ("int mmhip_set_image_sequence_float_host(mmhip_invocation *inv, int index, const float *pixels, int width, int height, int channels, "
            "int num_frames);") in flat
    assert ("int mmhip_set_image_sequence_float_device(mmhip_invocation *inv, int index, const void *device_float4, int width, int height, "
            "int num_frames);") in flat
    assert "int mmhip_filter_deep_inputs(const mmhip_filter *f);" in flat
    for name in ("mmhip_set_image_sequence_float_host", "mmhip_set_image_sequence_float_device", "mmhip_filter_deep_inputs"):
        assert name in _lib.SYMBOLS and getattr(lib(), name) is not None, name
    assert lib().mmhip_set_image_sequence_float_host.argtypes == [C.c_void_p, C.c_int, C.c_void_p] + [C.c_int] * 4
    assert lib().mmhip_set_image_sequence_float_device.argtypes == [C.c_void_p, C.c_int, C.c_void_p] + [C.c_int] * 3
    assert hasattr(mm.api.Invocation, "set_image_device_float") and hasattr(mm.api.Filter, "deep_inputs")
    for words in ("as TUPLE_FROM_COLOR makes them", "No clamp and no rounding", "No texel is loaded before", "float inputs are not supported there",
                  "((p1 * p1fact + p2 * p2fact) + p3 * p3fact) + p4 * p4fact"):
        assert words in flat, words


def test_setter_refusals_that_need_no_device():
    """What is wrong with the arguments is said before the invocation is looked at: no device, nothing allocated."""
    host, dev = lib().mmhip_set_image_sequence_float_host, lib().mmhip_set_image_sequence_float_device
    px = np.zeros((2, 2, 4), np.float32)
    p = px.ctypes.data_as(C.c_void_p)

    def refused(rc, words):
        assert rc == -1 and words in err(), (rc, err())
    refused(host(None, 0, p, 2, 2, 5, 1), "set_image_sequence_float_host: channels must be 3 or 4, not 5")
    refused(host(None, 0, p, 2, 2, 2, 1), "channels must be 3 or 4, not 2")
    for w, h in ((0, 2), (2, 0), (-1, 2), (2, -3)):
        refused(host(None, 0, p, w, h, 4, 1), "set_image_sequence_float_host: width and height must be at least 1, not %d x %d" % (w, h))
        refused(dev(None, 0, 0x1000, w, h, 1), "set_image_sequence_float_device: width and height must be at least 1, not %d x %d" % (w, h))
    for n in (0, -2):
        refused(host(None, 0, p, 2, 2, 4, n), "set_image_sequence_float_host: num_frames must be at least 1")
        refused(dev(None, 0, 0x1000, 2, 2, n), "set_image_sequence_float_device: num_frames must be at least 1")
    refused(host(None, 0, None, 2, 2, 4, 1), "set_image_sequence_float_host: the pixels are a null pointer")
    refused(dev(None, 0, None, 2, 2, 1), "set_image_sequence_float_device: the pixels are a null pointer")
    for off in (4, 8, 12, 1):
        refused(dev(None, 0, 0x1000 + off, 2, 2, 1), "set_image_sequence_float_device: the device pointer is not 16-byte aligned")
    # 2**31 - 1 by 2**30 texels of 16 bytes: 2**65 bytes; and 2**31 rows in all, the 8-bit sequence's rule
    refused(dev(None, 0, 0x1000, 2 ** 31 - 1, 2 ** 30, 1), "set_image_sequence_float_device: the size overflows")
    refused(host(None, 0, p, 2 ** 31 - 1, 2 ** 30, 4, 1), "set_image_sequence_float_host: the size overflows")
    refused(dev(None, 0, 0x1000, 1, 2 ** 16, 2 ** 15), "the size overflows (fewer than 2^31 rows in all")
    refused(dev(None, 0, 0x1000, 1, 2 ** 30, 2), "the size overflows (fewer than 2^31 rows in all")
    # sound arguments reach the invocation
    refused(dev(None, 0, 0x1000, 1, 2 ** 16, 2 ** 15 - 1), "set_image_sequence_float_device: no invocation")
    refused(host(None, 0, p, 2, 2, 4, 1), "set_image_sequence_float_host: no invocation")


def _unbound_invocation(flt):
    """An Invocation without the library's half: enough for what Python refuses before it calls the library."""
    inv = object.__new__(mm.api.Invocation)
    inv.filter, inv._h, inv._keep = flt, None, []
    return inv


@pytest.mark.parametrize("dtype", [np.float64, np.float16, np.int32, np.int64, np.uint16, np.int8, bool, np.complex64])
def test_other_dtypes_are_a_value_error(dtype):
    inv = _unbound_invocation(mm.Filter(SCALED, deep_inputs=True))
    for shape in ((3, 5, 4), (2, 3, 5, 3)):
        with pytest.raises(ValueError, match="uint8 .* or float32 .*, not %s" % np.dtype(dtype).name):
            inv.set_image("in", np.zeros(shape, dtype))
    with pytest.raises(mm.MathMapError, match="no user value"):
        inv.set_image("out", np.zeros((3, 5, 4), dtype))


def test_the_shapes_of_a_float_image():
    a = mm.api.as_float_image_sequence(np.ones((3, 5, 4), np.float32)[:, ::2])
    assert a.shape == (1, 3, 3, 4) and a.flags["C_CONTIGUOUS"] and a.dtype == np.float32
    assert mm.api.as_float_image_sequence(np.ones((2, 3, 5, 3), np.float32)).shape == (2, 3, 5, 3)
    for shape in ((3, 5), (0, 3, 5, 4), (1, 2, 3, 5, 4)):
        with pytest.raises(mm.MathMapError, match="an image is"):
            mm.api.as_float_image_sequence(np.ones(shape, np.float32))
    # what has no dtype is converted to uint8, as before there were float images
    assert mm.api.as_image_sequence([[[1, 2, 3]]]).dtype == np.uint8


# ---- the probes compile for gfx950 with the option on ----

@pytest.mark.parametrize("intersample", [True, False], ids=["bilinear", "nearest"])
@pytest.mark.parametrize("edge", [(0, 0), (1, 2), (3, 3), (2, 1)], ids=lambda e: "edge%d%d" % e)
def test_the_probes_compile_for_gfx950(edge, intersample):
    opts = dict(intersample=intersample, edge_x=edge[0], edge_y=edge[1], deep_inputs=True)
    for src in (R.FETCH["default"], R.FETCH["stretched"], R.FETCH_FRAME.replace("{F}", R.FRAME_EXPR), R.WILD):
        flt = mm.Filter(src, **opts)
        assert flt.jit(load=False) > 0 and flt.jit_clip(load=False) > 0, src
    if edge in ((0, 0), (3, 3)):
        flt = mm.Filter(R.FETCH["default"], **opts)
        assert flt.jit_shutter(load=False) > 0 and flt.jit_sampled(load=False) > 0 and flt.jit_refine(load=False) > 0
        for text in (flt.shutter_kernel_source, flt.sampled_kernel_source, flt.refine_kernel_source):
            assert "ORIG_VAL(" in text[text.index("__global__"):] and DEFINE in text


# ---- the restatement against the 8-bit one ----

def _coordinates(frame, m):
    """p[0], p[1] of map m over a frame's pixels, as COORDS computes them from x and y (float products and sums)."""
    W, H = frame
    x = ((np.arange(W, dtype=np.float64) - (W - 1) / 2.0) / ((W - 1) / 2.0)).astype(np.float32)
    y = ((-np.arange(H, dtype=np.float64) + (H - 1) / 2.0) / ((H - 1) / 2.0)).astype(np.float32)
    x, y = np.broadcast_to(x[None, :], (H, W)), np.broadcast_to(y[:, None], (H, W))
    sx, sy, ox, oy = (np.float32(v) for v in m[1:])
    with np.errstate(all="ignore"):
        return x * sx + ox, y * sy + oy


@pytest.mark.parametrize("edge", R.EDGE_PAIRS, ids=lambda e: "edge%d%d" % e)
def test_the_restatement_on_bytes_is_the_8_bit_one(edge):
    """On images that are TUPLE_FROM_COLOR of bytes the nearest fetch equals fetch_reference's bit for bit, and the
    bilinear one differs from it by no more than BILINEAR_BYTE_BOUND (derived there); a bad frame and the edge colours
    are part of it."""
    worst = 0.0
    for iw, ih in ((1, 1), (2, 3), (13, 7), (53, 37)):
        seq = R.random_frames(3, iw, ih, iw * 100 + ih)
        deep = R._tuple_from_bytes(seq)
        assert deep.dtype == np.float32
        for flags in ("default", "stretched"):
            factors = R.resize_factors(iw, ih, flags)
            for m in R.maps_for(iw, ih, factors):
                x, y = _coordinates((40, 24), m)
                frame = R.frame_index(np.broadcast_to(np.linspace(-1, 1, 40, dtype=np.float32)[None, :], (24, 40)))
                for fr in (0, 2, frame):
                    want, ok = R.fetch_nearest(seq, x, y, edge, R.EDGE_COLOURS, factors=factors, frame=fr)
                    got, ok2 = D.fetch_nearest_deep(deep, x, y, edge, R.EDGE_COLOURS, factors=factors, frame=fr)
                    assert np.array_equal(ok, ok2) and ok.all()
                    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), ((iw, ih), flags, m)
                    want, ok = R.fetch_bilinear(seq, x, y, edge, R.EDGE_COLOURS, factors=factors, frame=fr)
                    got, ok2 = D.fetch_bilinear_deep(deep, x, y, edge, R.EDGE_COLOURS, factors=factors, frame=fr)
                    assert np.array_equal(ok, ok2) and ok.all()
                    diff = float(np.abs(got.astype(np.float64) - want.astype(np.float64)).max())
                    worst = max(worst, diff)
                    assert diff <= D.BILINEAR_BYTE_BOUND, ((iw, ih), flags, m, diff)
    print("largest |deep - 8-bit| bilinear difference: %.9f of a bound of %.9f" % (worst, D.BILINEAR_BYTE_BOUND))
    assert 0.5 / 255 < D.BILINEAR_BYTE_BOUND < 0.5 / 255 + 1e-6


def test_the_restatement_passes_floats_through():
    """No clamp, no rounding: a one-texel image of any float comes back as it is under the nearest fetch, NaN and all;
    the identity bilinear fetch on texel centres returns texels exactly (three of the four weights are 0)."""
    t = D.random_texels(2, 13, 7, 3)
    assert np.isnan(t).any() and np.isinf(t).any() and (t < 0).any() and (t > 1).any()
    assert ((t == 0) & np.signbit(t)).any() and ((np.abs(t) > 0) & (np.abs(t) < np.finfo(np.float32).tiny)).any()
    x = (np.arange(13, dtype=np.float32) - 6) / 6
    y = -(np.arange(7, dtype=np.float32) - 3) / 3
    x, y = np.broadcast_to(x[None, :], (7, 13)), np.broadcast_to(y[:, None], (7, 13))
    for k in (0, 1):
        got, ok = D.fetch_nearest_deep(t, x, y, (0, 0), R.EDGE_COLOURS, frame=k)
        assert ok.all() and np.array_equal(got.view(np.uint32), t[k].view(np.uint32))
    got, _ = D.fetch_nearest_deep(t, x, y, (0, 0), R.EDGE_COLOURS, frame=2)
    assert (got == 1.0).all()
    got, _ = D.fetch_nearest_deep(t, x * 3, y, (0, 0), R.EDGE_COLOURS, frame=5)          # an edge colour wins over a bad frame
    assert np.array_equal(got[0, 0], R._tuple_from_bytes([0x20, 0x40, 0x60, 0x80])) and (got[:, 6] == 1.0).all()
