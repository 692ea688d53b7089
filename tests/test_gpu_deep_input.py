"""Float32 input drawables on the GPU (mm_device.h mm_orig_val_deep behind mmhip_options.deep_inputs;
mmhip_set_image_sequence_float_host / _device) against the numpy restatement tests/deep_fetch_reference.py.

The rule is gauss_reference.same_maps on covered pixels: NaN in the same places, every other element the same bits.  The
tolerance is 0: the path is float + - *, floor and integer %, every operation rounded once.  The coordinate arrays the
restatement takes are the GPU's own renders of fetch_reference.COORDS (compared with the oracle's by
tests/test_gpu_fetch.py's helper, which is used here), so a difference in the coordinates is reported as such."""
import ctypes as C

import numpy as np
import pytest

import mathmap_amd as mm
from mathmap_amd._lib import lib
from tests import deep_fetch_reference as D
from tests import fetch_reference as R
from tests import gauss_reference as G
from tests import yuv10_reference as X10
from tests.gpu_util import render_device
from tests.test_gpu_clip_yuv_input import free_device_bytes
from tests.test_gpu_fetch import _coords, _Renderer

pytestmark = pytest.mark.gpu

FOUR = [(0, 0), (1, 2), (3, 3), (2, 1)]
IMAGES = [(1, 1), (2, 3), (13, 7), (53, 37)]
IDENTITY = ("identity", 1.0, 1.0, 0.0, 0.0)
SENTINEL, LEAD = 0xA5, 64
DEEP_CLIP = "filter deep_clip (image in)\n  in(xy, frame)\nend\n"
DEEP_CLIP_WIDE = "filter deep_clip_wide (image in)\n  in(xy * 1.5, frame)\nend\n"      # reaches beyond the image on every side
# the chain's second filter: stretched like its image, so that x and y are the image's own unit coordinates
CHAIN_B = "stretched filter chain_b (stretched image in)\n  in(xy, frame)\nend\n"
# a horizontal grey ramp of 2/255 of the range around 0.401 (tests/test_gpu_clip_yuv10.py's), a little brighter per frame
CHAIN_A = "filter chain_a () v = 0.401 + x / X / 255 + frame * 0.0003; rgba:[v, v, v, 1] end"
DRIFT = "filter drift (image in)\n  in(xy + xy:[t * 0.4, t * 0.1], frame)\nend\n"


def err():
    return lib().mmhip_last_error().decode()


def _deep(flt):
    assert flt.deep_inputs and "#define MM_DEEP_INPUTS 1\n" in flt.kernel_source


def _assert_same(got, want, what, covered=None):
    if covered is not None:
        got, want = got[covered], want[covered]
    assert G.same_maps(got, want), (what, G.describe_difference(got, want))


def _options(edge, intersample, **more):
    return dict(intersample=intersample, edge_x=edge[0], edge_y=edge[1], deep_inputs=True, **more)


def _fetch(intersample):
    return D.fetch_bilinear_deep if intersample else D.fetch_nearest_deep


def _invocation(src, frame, **opts):
    inv = mm.Filter(src, **opts).invoke(*frame)
    inv.set_edge_colors(*R.EDGE_COLOURS)
    return inv


def clip_float_maps(inv, **clip):
    """render_clip(floatmap=True) of whole frames into device memory, read back: float32 [N, h, w, 4]."""
    n = clip["num_frames"] if "num_frames" in clip else len(clip["frames"])
    w, h = inv.render_width, inv.render_height
    dev = lib().mmhip_device_alloc(n * w * h * 16)
    assert dev
    try:
        inv.render_clip(floatmap=True, out_ptr=dev, **clip)
        inv.sync()
        out = np.empty((n, h, w, 4), np.float32)
        assert lib().mmhip_copy_to_host(out.ctypes.data_as(C.c_void_p), C.c_void_p(dev), out.nbytes) == 0
    finally:
        lib().mmhip_device_free(C.c_void_p(dev))
    return out


# ---- 1. nearest and bilinear ----

@pytest.mark.parametrize("intersample", [True, False], ids=["bilinear", "nearest"])
@pytest.mark.parametrize("edge", R.EDGE_PAIRS, ids=lambda e: "edge%d%d" % e)
def test_deep_fetch(edge, intersample):
    """FETCH["default"] and FETCH["stretched"] over maps_for on random float texels with NaN, both infinities, -0,
    denormals, negatives and values above 1: every edge pair at 13 x 7 on 40 x 24, four of them at every size."""
    fetch = _fetch(intersample)
    renderers = {flags: _Renderer(R.FETCH[flags], {}, _deep, **_options(edge, intersample)) for flags in ("default", "stretched")}
    sizes = [(f, s) for f in R.FRAME_SIZES for s in IMAGES] if edge in FOUR else [((40, 24), (13, 7))]
    census = None
    for frame, (iw, ih) in sizes:
        img = D.random_texels(1, iw, ih, iw * 100 + ih)[0]
        for flags, r in renderers.items():
            factors = R.resize_factors(iw, ih, flags)
            for m in R.maps_for(iw, ih, factors):
                c = _coords(frame, m)
                want, covered = fetch(img, c[..., 0], c[..., 1], edge, R.EDGE_COLOURS, factors=factors)
                assert covered.all(), (frame, (iw, ih), flags, m)
                got = r.float_map(frame, img, R.map_uservals(m))
                _assert_same(got, want, (frame, (iw, ih), flags, m))
                if (iw, ih) == (13, 7) and m[0] == "identity" and frame == (40, 24) and flags == "default":      # (every texel is sampled)
                    census = G.special_census(got)
                    assert np.array_equal(r.rgba8(frame, img, R.map_uservals(m)), R.pack(want, 4))
    # the specials came through the fetch: none was clamped, rounded or flushed
    assert all(sum(census[k]) > 0 for k in ("nan", "+inf", "-inf")), census
    if not intersample:
        assert sum(census["-0"]) > 0 and sum(census["denormal"]) > 0, census


# ---- 2. sequences ----

@pytest.mark.parametrize("intersample", [True, False], ids=["bilinear", "nearest"])
@pytest.mark.parametrize("edge", FOUR, ids=lambda e: "edge%d%d" % e)
def test_per_pixel_frame_number(edge, intersample):
    """in(p, floor(x * 2 + 1.5)) on three frames: frames -1 and 3 give ones, but only where the edge tests let a tap
    through."""
    fetch = _fetch(intersample)
    r = _Renderer(R.FETCH_FRAME.replace("{F}", R.FRAME_EXPR), {}, _deep, **_options(edge, intersample))
    seen = {"ones": False, "edge colour first": False}
    for frame in R.FRAME_SIZES:
        for iw, ih in ((13, 7), (2, 3)):
            seq = D.random_texels(3, iw, ih, 5)
            factors = R.resize_factors(iw, ih, "default")
            for m in R.maps_for(iw, ih, factors)[:6]:
                c = _coords(frame, m)
                index = R.frame_index(c[..., 2])
                assert sorted(np.unique(index)) == [-1, 0, 1, 2, 3]
                want, covered = fetch(seq, c[..., 0], c[..., 1], edge, R.EDGE_COLOURS, factors=factors, frame=index)
                assert covered.all()
                _assert_same(r.float_map(frame, seq, R.map_uservals(m)), want, (frame, (iw, ih), m))
                bad, ones = (index < 0) | (index > 2), (want == 1.0).all(axis=-1)
                seen["ones"] |= bool((ones & bad).any())
                seen["edge colour first"] |= bool((~ones & bad).any())
    assert seen["ones"] and (seen["edge colour first"] or edge != (0, 0)), seen


@pytest.mark.parametrize("intersample", [True, False], ids=["bilinear", "nearest"])
def test_frame_constant_frame_number_under_render_clip(intersample):
    """in(xy * 1.5, frame) over the clip's frame numbers -1 .. 3 on three frames: the clip kernels' fetch.  The frame
    reaches beyond the image on every side, where the edge colour comes before the bad frame."""
    frame, edge = (40, 24), (0, 0)
    seq = D.random_texels(3, 13, 7, 11)
    inv = _invocation(DEEP_CLIP_WIDE, frame, **_options(edge, intersample))
    inv.set_image("in", seq)
    numbers = [-1, 0, 1, 2, 3]
    got = clip_float_maps(inv, frames=numbers, ts=[0.0] * 5)
    c = _coords(frame, IDENTITY)
    px, py = c[..., 2] * np.float32(1.5), c[..., 3] * np.float32(1.5)
    for k, number in enumerate(numbers):
        want, covered = _fetch(intersample)(seq, px, py, edge, R.EDGE_COLOURS, factors=R.resize_factors(13, 7, "default"), frame=number)
        assert covered.all()
        _assert_same(got[k], want, ("frame", number))
        if number in (-1, 3):
            ones = (want == 1.0).all(axis=-1)
            assert ones.any() and not ones.all()
    _assert_same(render_device(inv, 40, 24, floatmap=True, frame=1), got[2], "mmhip_render at frame 1")


# ---- 3. equivalence with the 8-bit path ----

@pytest.mark.parametrize("intersample", [True, False], ids=["bilinear", "nearest"])
def test_equivalence_with_the_8_bit_path(intersample):
    """The option changes nothing for an 8-bit image; a deep image of bytes / 255 gives the 8-bit image's float map --
    bit for bit under nearest, within deep_fetch_reference.BILINEAR_BYTE_BOUND (derived there) under bilinear."""
    worst = 0.0
    for edge in ((0, 0), (3, 1)):
        opts = _options(edge, intersample)
        on = _Renderer(R.FETCH["default"], {}, _deep, **opts)
        off = _Renderer(R.FETCH["default"], {}, lambda flt: None, **dict(opts, deep_inputs=False))
        deep = _Renderer(R.FETCH["default"], {}, _deep, **opts)
        for frame, (iw, ih) in (((40, 24), (13, 7)), ((5, 3), (2, 3)), ((40, 24), (53, 37))):
            img = R.random_frames(1, iw, ih, iw * 100 + ih)[0]
            texels = R._tuple_from_bytes(img)
            assert texels.dtype == np.float32
            for m in R.maps_for(iw, ih, R.resize_factors(iw, ih, "default")):
                uv = R.map_uservals(m)
                base = off.float_map(frame, img, uv)
                _assert_same(on.float_map(frame, img, uv), base, ("8-bit image, option on", frame, (iw, ih), m))
                assert np.array_equal(on.rgba8(frame, img, uv), off.rgba8(frame, img, uv))
                got = deep.float_map(frame, texels, uv)
                if not intersample:
                    _assert_same(got, base, ("bytes / 255, nearest", frame, (iw, ih), m))
                else:
                    diff = float(np.abs(got.astype(np.float64) - base.astype(np.float64)).max())
                    worst = max(worst, diff)
                    assert diff <= D.BILINEAR_BYTE_BOUND, (frame, (iw, ih), m, diff)
    print("largest |deep - 8-bit| difference on the device: %.9f (bound %.9f)" % (worst, D.BILINEAR_BYTE_BOUND))


# ---- 4. wild coordinates ----

@pytest.mark.parametrize("intersample", [True, False], ids=["bilinear", "nearest"])
@pytest.mark.parametrize("edge", FOUR, ids=lambda e: "edge%d%d" % e)
def test_wild_coordinates_stay_inside(edge, intersample):
    """NaN, +-inf, 2**31, 2**32 and 1e19 px: the render completes, the covered pixels are the restatement's, and of a
    sentinel-filled buffer only the rendered rows change."""
    w, h, first, last = 40, 24, 3, 21
    inv = _invocation(R.WILD, (w, h), **_options(edge, intersample))
    coords = _invocation(R.WILD_COORDS, (w, h))
    total = LEAD + w * h * 16 + LEAD
    dev = lib().mmhip_device_alloc(total)
    assert dev
    try:
        seen = {"covered": False, "not covered": False}
        for iw, ih in ((13, 7), (53, 37)):
            img = D.random_texels(1, iw, ih, iw + ih)[0]
            inv.set_image("in", img)
            for big in R.WILD_BIG:
                for vert in (0, 1):
                    for k, v in R.wild_uservals(big, vert).items():
                        inv.set(k, v)
                        coords.set(k, v)
                    c = render_device(coords, w, h, floatmap=True)
                    want, covered = _fetch(intersample)(img, c[..., 0], c[..., 1], edge, R.EDGE_COLOURS, factors=R.resize_factors(iw, ih, "default"))
                    fill = np.full(total, SENTINEL, np.uint8)
                    assert lib().mmhip_copy_to_device(C.c_void_p(dev), fill.ctypes.data_as(C.c_void_p), total) == 0
                    inv.render_rows(dev + LEAD + first * w * 16, first, last, floatmap=True)
                    inv.sync()
                    assert lib().mmhip_copy_to_host(fill.ctypes.data_as(C.c_void_p), C.c_void_p(dev), total) == 0
                    lo, hi = LEAD + first * w * 16, LEAD + last * w * 16
                    assert (fill[:lo] == SENTINEL).all() and (fill[hi:] == SENTINEL).all(), ("written outside the rows", (iw, ih), big, vert)
                    got = fill[lo:hi].view(np.float32).reshape(last - first, w, 4)
                    _assert_same(got, want[first:last], ("wild", (iw, ih), big, vert), covered[first:last])
                    seen["covered"] |= bool(covered[first:last].any())
                    seen["not covered"] |= bool((~covered[first:last]).any())
        assert seen["covered"] and seen["not covered"], seen
    finally:
        lib().mmhip_device_free(C.c_void_p(dev))


# ---- 5. the chain ----

@pytest.mark.parametrize("size", [(17, 9), (64, 8)], ids=lambda s: "%dx%d" % s)
def test_the_chain_stays_in_hbm(size):
    """Filter A's float frames (render_clip(floatmap=True, out_ptr=p)) are filter B's input (set_image_device_float(p)):
    B's float maps are the restatement's, which here returns every texel exactly, so B's 10-bit payload is A's own."""
    w, h = size
    a = mm.Filter(CHAIN_A).invoke(w, h)
    b = _invocation(CHAIN_B, size, **_options((0, 0), False))
    p = lib().mmhip_device_alloc(3 * w * h * 16)
    assert p
    try:
        a.render_clip(num_frames=3, floatmap=True, out_ptr=p)
        a.sync()
        frames = np.empty((3, h, w, 4), np.float32)
        assert lib().mmhip_copy_to_host(frames.ctypes.data_as(C.c_void_p), C.c_void_p(p), frames.nbytes) == 0
        assert len(np.unique((frames[0, 0, :, 0] * 255).astype(int))) <= 3 and len(np.unique(frames[0, 0, :, 0])) == w      # between byte levels
        b.set_image_device_float("in", p, w, h, num_frames=3)
        got = clip_float_maps(b, num_frames=3)
        c = _coords(size, IDENTITY, True)
        for k in range(3):
            want, covered = D.fetch_nearest_deep(frames, c[..., 2], c[..., 3], (0, 0), R.EDGE_COLOURS, frame=k)
            assert covered.all()
            assert np.array_equal(want.view(np.uint32), frames[k].view(np.uint32)), "the identity fetch returns each texel"
            _assert_same(got[k], want, ("chain", size, k))
        own = a.render_clip(num_frames=3, pixel_format="yuv420p10")
        assert np.array_equal(own, X10.frames(frames, ("bt709", "limited")))
        chained = b.render_clip(num_frames=3, pixel_format="yuv420p10")
        assert np.array_equal(chained, own)
        if size == (64, 8):
            # the same chain through RGBA8 loses the ramp: the figures of the 10-bit output's own ramp test
            b8 = _invocation(CHAIN_B, size, intersample=False)
            b8.set_image("in", a.render_clip(num_frames=3))
            through_bytes = b8.render_clip(num_frames=3, pixel_format="yuv420p10")
            y8 = mm.api.yuv420_planes(through_bytes, w, h)[0][0]
            y = mm.api.yuv420_planes(chained, w, h)[0][0]
            print("distinct Y codes over the ramp: %d through the float chain, %d through RGBA8" % (len(np.unique(y)), len(np.unique(y8))))
            assert len(np.unique(y8)) <= 3 and len(np.unique(y)) >= 8
    finally:
        b.sync()
        del b
        lib().mmhip_device_free(C.c_void_p(p))


# ---- 6. the host setter ----

def test_host_setter_channels_and_rebinding():
    """3 channels get alpha 1.0f; deep and 8-bit images replace each other on one index, either way round, through the
    host setters and the device setters."""
    frame, edge = (40, 24), (1, 2)
    inv = _invocation(R.FETCH["default"], frame, **_options(edge, True))
    t4 = D.random_texels(2, 13, 7, 21)
    rgb = np.ascontiguousarray(t4[..., :3])
    with_alpha = t4.copy()
    with_alpha[..., 3] = 1.0
    img8 = R.random_frames(1, 13, 7, 4)[0]
    c = _coords(frame, IDENTITY)
    factors = R.resize_factors(13, 7, "default")

    def deep_map(seq):
        return D.fetch_bilinear_deep(seq, c[..., 0], c[..., 1], edge, R.EDGE_COLOURS, factors=factors)[0]
    want8 = R.fetch_bilinear(img8, c[..., 0], c[..., 1], edge, R.EDGE_COLOURS, factors=factors)[0]
    inv.set_image("in", t4)
    _assert_same(render_device(inv, 40, 24, floatmap=True), deep_map(t4), "4 channels")
    inv.set_image("in", rgb)
    _assert_same(render_device(inv, 40, 24, floatmap=True), deep_map(with_alpha), "3 channels")
    inv.set_image("in", t4[0])                                # [H, W, 4]: one frame
    _assert_same(render_device(inv, 40, 24, floatmap=True), deep_map(t4[:1]), "one image")
    inv.set_image("in", img8)
    _assert_same(render_device(inv, 40, 24, floatmap=True), want8, "8-bit over deep")
    inv.set_image("in", t4)
    _assert_same(render_device(inv, 40, 24, floatmap=True), deep_map(t4), "deep over 8-bit")
    # the device setters, both ways over an upload the invocation owns
    words = (img8[..., 0].astype(np.uint32) << 24) | (img8[..., 1].astype(np.uint32) << 16) | (img8[..., 2].astype(np.uint32) << 8) | img8[..., 3]
    d8, df = lib().mmhip_device_alloc(words.nbytes), lib().mmhip_device_alloc(with_alpha.nbytes)
    assert d8 and df
    try:
        assert lib().mmhip_copy_to_device(C.c_void_p(d8), np.ascontiguousarray(words).ctypes.data_as(C.c_void_p), words.nbytes) == 0
        assert lib().mmhip_copy_to_device(C.c_void_p(df), with_alpha.ctypes.data_as(C.c_void_p), with_alpha.nbytes) == 0
        inv.set_image_device("in", d8, 13, 7)
        _assert_same(render_device(inv, 40, 24, floatmap=True), want8, "8-bit device pointer over a deep upload")
        inv.set_image_device_float("in", df, 13, 7, num_frames=2)
        _assert_same(render_device(inv, 40, 24, floatmap=True), deep_map(with_alpha), "deep device pointer")
        inv.set_image("in", img8)
        _assert_same(render_device(inv, 40, 24, floatmap=True), want8, "8-bit upload over a deep device pointer")
    finally:
        inv.sync()
        del inv
        lib().mmhip_device_free(C.c_void_p(d8))
        lib().mmhip_device_free(C.c_void_p(df))


def test_rebinding_frees_the_earlier_upload():
    """512 x 512 x 8 float texels: 32 MiB.  Twelve rebinds, deep and 8-bit in turn, that kept theirs would hold 240 MiB."""
    w, h, n = 512, 512, 8
    deep = np.random.default_rng(1).random((n, h, w, 4), np.float32)
    bytes8 = R.random_frames(n, w, h, 2)
    inv = mm.Filter(DEEP_CLIP, deep_inputs=True).invoke(w, h)
    inv.set_image("in", deep)
    first = inv.render(frame=5)
    inv.sync()
    before = free_device_bytes()
    for k in range(12):
        inv.set_image("in", bytes8 if k % 2 == 0 else deep)
    inv.sync()
    assert before - free_device_bytes() < 2 * deep.nbytes
    assert np.array_equal(inv.render(frame=5), first)


# ---- 7. refusals ----

def test_refusals_leave_nothing_bound():
    frame = (40, 24)
    texels = D.random_texels(1, 13, 7, 8)
    plain = _invocation(DEEP_CLIP, frame)                     # compiled without the option
    unbound = plain.render()
    with pytest.raises(mm.MathMapError, match="set_image_sequence_float_host: filter `deep_clip' was not compiled with deep_inputs"):
        plain.set_image("in", texels)
    p = lib().mmhip_device_alloc(texels.nbytes)
    assert p
    try:
        with pytest.raises(mm.MathMapError, match="set_image_sequence_float_device: filter `deep_clip' was not compiled with deep_inputs"):
            plain.set_image_device_float("in", p, 13, 7)
        assert np.array_equal(plain.render(), unbound)
        inv = _invocation(DEEP_CLIP, frame, deep_inputs=True)
        host, dev = lib().mmhip_set_image_sequence_float_host, lib().mmhip_set_image_sequence_float_device
        data = texels.ctypes.data_as(C.c_void_p)
        for call, words in ((lambda: host(inv._h, 0, data, 13, 7, 5, 1), "channels must be 3 or 4, not 5"),
                          (lambda: host(inv._h, 0, data, 0, 7, 4, 1), "width and height must be at least 1, not 0 x 7"),
                          (lambda: dev(inv._h, 0, p, 13, -1, 1), "width and height must be at least 1, not 13 x -1"),
                          (lambda: host(inv._h, 0, data, 13, 7, 4, 0), "num_frames must be at least 1"),
                          (lambda: dev(inv._h, 0, p, 13, 7, -3), "num_frames must be at least 1"),
                          (lambda: host(inv._h, 0, None, 13, 7, 4, 1), "the pixels are a null pointer"),
                          (lambda: dev(inv._h, 0, None, 13, 7, 1), "the pixels are a null pointer"),
                          (lambda: dev(inv._h, 0, p + 4, 13, 7, 1), "the device pointer is not 16-byte aligned"),
                          (lambda: dev(inv._h, 0, p, 2 ** 31 - 1, 2 ** 30, 1), "the size overflows"),
                          (lambda: dev(inv._h, 0, p, 1, 2 ** 16, 2 ** 15), "fewer than 2^31 rows in all"),
                          (lambda: dev(inv._h, 7, p, 13, 7, 1), "")):
            rc = call()
            assert rc == -1 and words in err(), (rc, words, err())
            assert np.array_equal(inv.render(), unbound), words
        with pytest.raises(ValueError, match="uint8 .* or float32"):
            inv.set_image("in", texels.astype(np.float64))
        assert np.array_equal(inv.render(), unbound)
        inv.sync()
    finally:
        lib().mmhip_device_free(C.c_void_p(p))


@pytest.mark.parametrize("call, who", [("gaussian_blur(in, 0.02, 0.02)", "gaussian_blur"), ("render(in)", "render()")],
                         ids=["gaussian_blur", "render"])
def test_a_native_filter_refuses_a_deep_image_by_name(call, who):
    """The render fails with the filter's name and the reason; the invocation stays usable, for an 8-bit image and for
    the next deep one."""
    src = "filter native_on_deep (image in)\n  b = %s;\n  b(xy)\nend\n" % call
    frame = (40, 24)
    img8 = R.random_frames(1, 40, 24, 6)[0]
    inv = _invocation(src, frame, deep_inputs=True)
    fresh = _invocation(src, frame, deep_inputs=True)
    fresh.set_image("in", img8)
    want = fresh.render()
    inv.set_image("in", D.random_texels(1, 40, 24, 6))
    message = r"%s: float inputs are not supported by native filters" % who.replace("(", r"\(").replace(")", r"\)")
    with pytest.raises(mm.MathMapError, match=message):
        inv.render()
    with pytest.raises(mm.MathMapError, match=message):
        inv.render_clip(num_frames=2)
    inv.set_image("in", img8)
    assert np.array_equal(inv.render(), want)
    inv.set_image("in", D.random_texels(1, 40, 24, 7))
    with pytest.raises(mm.MathMapError, match=message):
        inv.render()
    inv.set_image("in", img8)
    assert np.array_equal(inv.render_clip(num_frames=2)[1], want)


# ---- 8. the variants ----

@pytest.mark.parametrize("variant", ["shutter", "sampled", "refine"])
def test_the_variants_fetch_deep_images(variant):
    """The fused shutter, the fused grid and the refine list on a deep input give the bytes of the same call's maps path,
    and single-sample frames that are the restatement's."""
    frame = (40, 24)
    seq = np.random.default_rng(9).uniform(-0.25, 1.25, (3, 7, 13, 4)).astype(np.float32)
    inv = _invocation(DRIFT, frame, **_options((1, 2), True))
    inv.set_image("in", seq)
    calls = {"shutter": (dict(shutter_samples=4, shutter=0.5, shutter_mode="fused"), dict(shutter_samples=4, shutter=0.5, shutter_mode="maps"),
                         inv.clip_shutter_fused_batches),
             "sampled": (dict(aa=2, shutter_mode="fused"), dict(aa=2, shutter_mode="maps"), inv.clip_sampled_fused_batches),
             "refine": (dict(aa=2, aa_threshold=0.02, aa_refine="list"), dict(aa=2, aa_threshold=0.02, aa_refine="select"), inv.clip_adaptive_batches)}
    fused, maps, counter = calls[variant]
    got = inv.render_clip(num_frames=3, **fused)
    assert counter() > 0
    want = inv.render_clip(num_frames=3, **maps)
    assert np.array_equal(got, want), (variant, int((got != want).sum()))
    if variant == "refine":
        assert sum(inv.clip_adaptive_refined()) > 0
    # frame 0 at t = 0 without sub-samples is the plain fetch
    c = _coords(frame, IDENTITY)
    plain, covered = D.fetch_bilinear_deep(seq, c[..., 2], c[..., 3], (1, 2), R.EDGE_COLOURS, factors=R.resize_factors(13, 7, "default"), frame=0)
    assert covered.all()
    _assert_same(clip_float_maps(inv, num_frames=3)[0], plain, "frame 0")
