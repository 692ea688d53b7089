"""The image fetch and the pixel output of the HIP kernels (mm_device.h: mm_intersample_sums_hot, mm_get_pixel,
mm_taps_all_inside, the early-exit fetch and its two shortcuts, mm_select_frame, mm_pack_bytes, mm_floatmap_pixel,
mm_store_pixel; native_filters.hip: k_render_drawable, k_render_floatmap) against the numpy restatement of
tests/fetch_reference.py *and* the oracle.

The restatement is written from the reference's sources and pinned against the oracle by tests/test_fetch_reference.py
over the same case table, so every comparison here is one with two independent transcriptions of the reference.  The
rule is gauss_reference.same_maps: NaN in the same places, every other element the same bits.  The tolerance is 0: the
path is float + - * /, floor, rint and integer %, with contraction off, and there is no libm in it.  Float maps are
compared, so that no byte hides a wrong weight; RGBA8 bytes where the store is the subject.

The map comes in as float user values, so one compiled kernel per (edge pair, sampling mode, variant) serves every
image size and every map; every variant asserts from its kernel's text that it is what it claims.  The coordinate
arrays the restatement takes are the GPU's own render of fetch_reference.COORDS, compared with the oracle's first, so
that a difference in the coordinates is reported as such.  Wild coordinates (NaN, +-inf, 2**31, 2**32, 1e19) are not
covered by the restatement and are compared with the oracle alone."""
import contextlib
import ctypes as C
import os

import numpy as np
import pytest

import mathmap_amd as mm
from mathmap_amd._lib import lib
from tests import fetch_reference as R
from tests import gauss_reference as G
from tests.gpu_util import render_device

pytestmark = pytest.mark.gpu

KNOBS = ("MMHIP_NO_FETCHED_RESULT", "MMHIP_SINGLE_PIXEL", "MMHIP_NO_SAME_TAPS", "MMHIP_NO_OUTSIDE_SHORTCUT", "MMHIP_FRAME_HOT",
         "MMHIP_PAIR", "MMHIP_PAIR_PACK", "MMHIP_UNROLL")


@contextlib.contextmanager
def _environment(env):
    """The generator's hooks set to exactly `env` (they are read when a filter is compiled)."""
    saved = {k: os.environ.pop(k, None) for k in KNOBS}
    os.environ.update(env)
    try:
        yield
    finally:
        for k in KNOBS:
            os.environ.pop(k, None)
            if saved[k] is not None:
                os.environ[k] = saved[k]


def _body(flt):
    """The generated kernels without the prelude they are compiled with."""
    ks = flt.kernel_source
    return ks[ks.index("__global__"):]


def _defines(flt, name):
    return ("#define %s" % name) in flt.kernel_source


def _assert_same(got, want, what):
    assert G.same_maps(got, want), (what, G.describe_difference(got, want))


_COORD_FILTERS, _COORDS = {}, {}


def _coords(frame, m, stretched=False):
    """[h, w, 4] = (p[0], p[1], x, y) of map `m` on `frame`: the GPU's render of COORDS, equal to the oracle's."""
    key = (frame, m[1:], stretched)
    if key not in _COORDS:
        if stretched not in _COORD_FILTERS:
            with _environment({}):
                _COORD_FILTERS[stretched] = mm.Filter(R.COORDS[stretched])
        inv = _COORD_FILTERS[stretched].invoke(*frame)
        for k, v in R.map_uservals(m).items():
            inv.set(k, v)
        got = render_device(inv, frame[0], frame[1], floatmap=True)
        want = G.oracle(R.COORDS[stretched]).render(frame[0], frame[1], uservals=R.map_uservals(m), floatmap=True)
        _assert_same(got, want, ("coordinates", frame, m, stretched))
        _COORDS[key] = got
    return _COORDS[key]


def _oracle(src, frame, uv, img, **kw):
    return G.oracle(src).render(frame[0], frame[1], uservals=uv, images={"in": img}, edge_colors=R.EDGE_COLOURS, **kw)


class _Renderer:
    """One compiled filter, an invocation per frame size, images and user values set as the cases ask."""

    def __init__(self, src, env, claim, **opts):
        self.env = env
        with _environment(env):
            self.flt = mm.Filter(src, **opts)
        claim(self.flt)
        self.invs, self.bound = {}, {}

    def _invocation(self, frame, img, uv):
        if frame not in self.invs:
            self.invs[frame] = self.flt.invoke(*frame)
            self.invs[frame].set_edge_colors(*R.EDGE_COLOURS)
        inv = self.invs[frame]
        if self.bound.get(frame) is not img:
            inv.set_image("in", img)
            self.bound[frame] = img
        for k, v in uv.items():
            inv.set(k, v)
        return inv

    def float_map(self, frame, img, uv):
        with _environment(self.env):
            return render_device(self._invocation(frame, img, uv), frame[0], frame[1], floatmap=True)

    def rgba8(self, frame, img, uv):
        with _environment(self.env):
            return self._invocation(frame, img, uv).render()


# ---- the drawable fetch ------------------------------------------------------------------------------------------------

def _drawable_cases(edge, intersample, pixel_inc=1, big=2.5e8):
    """(frame, flags, image, map, reference) over the case table: the restatement's float map at the GPU's coordinates,
    every pixel covered, and equal to the oracle's."""
    fetch = R.fetch_bilinear if intersample else R.fetch_nearest
    more = {"pixel_inc": pixel_inc} if pixel_inc > 1 else {}
    cases = []
    for frame in R.FRAME_SIZES:
        for iw, ih in R.image_sizes_for(frame):
            img = R.random_frames(1, iw, ih, iw * 100 + ih)[0]
            for flags in ("default", "stretched"):
                factors = R.resize_factors(iw, ih, flags)
                for m in R.maps_for(iw, ih, factors, big=big):
                    c = _coords(frame, m)
                    want, covered = fetch(img, c[..., 0], c[..., 1], edge, R.EDGE_COLOURS, factors=factors, **more)
                    assert covered.all(), (frame, (iw, ih), flags, m)
                    _assert_same(want, _oracle(R.FETCH[flags], frame, R.map_uservals(m), img, floatmap=True, intersample=intersample,
                                               edge=edge, **more), ("restatement against oracle", frame, (iw, ih), flags, m))
                    cases.append((frame, flags, img, m, want))
    return cases


def _wild_cases(edge, intersample, **more):
    """(image, user values, the oracle's float map, the oracle's bytes) of WILD on 40 x 24."""
    cases = []
    for iw, ih in ((13, 7), (53, 37)):
        img = R.random_frames(1, iw, ih, iw * 100 + ih)[0]
        for big in R.WILD_BIG:
            for vert in (0, 1):
                uv = R.wild_uservals(big, vert)
                kw = dict(intersample=intersample, edge=edge, **more)
                cases.append((img, uv, _oracle(R.WILD, (40, 24), uv, img, floatmap=True, **kw), _oracle(R.WILD, (40, 24), uv, img, **kw)))
    return cases


def _hot_store_fetched(flt):
    assert "mm_store_fetched_pixel(A, rl_raw" in _body(flt) and "mm_orig_val_sums_hot(A," in _body(flt)


def _hot_tuple(flt):
    assert "mm_orig_val_hot(A," in _body(flt) and "mm_store_fetched_pixel(A, rl_raw" not in _body(flt)


def _cold(flt):
    assert "_hot(A," not in _body(flt) and "_hotf(A," not in _body(flt) and "ORIG_VAL(" in _body(flt)
    assert flt.launch_geometry(40, 24)["single_pixel"] == 1


def _cold_without_shortcuts(flt):
    _cold(flt)
    assert _defines(flt, "MM_NO_SAME_TAPS 1") and _defines(flt, "MM_NO_OUTSIDE_SHORTCUT 1")


def _cold_with_shortcuts(flt):
    _cold(flt)
    assert not _defines(flt, "MM_NO_SAME_TAPS") and not _defines(flt, "MM_NO_OUTSIDE_SHORTCUT")


SINGLE = {"MMHIP_SINGLE_PIXEL": "1"}
LONG_WAY = {"MMHIP_SINGLE_PIXEL": "1", "MMHIP_NO_SAME_TAPS": "1", "MMHIP_NO_OUTSIDE_SHORTCUT": "1"}


@pytest.mark.parametrize("intersample", [True, False], ids=["bilinear", "nearest"])
@pytest.mark.parametrize("edge", R.EDGE_PAIRS, ids=lambda e: "edge%d%d" % e)
def test_drawable_fetch(edge, intersample):
    """The whole case table through the hot fetch (a pure distortion: mm_store_fetched_pixel, as bytes and as a float
    map; with MMHIP_NO_FETCHED_RESULT=1 through the tuple) and the cold fetch (MMHIP_SINGLE_PIXEL=1, with its two
    wave-uniform shortcuts and the long way round), on a default and a stretched image; then the wild coordinates."""
    opts = dict(intersample=intersample, edge_x=edge[0], edge_y=edge[1])
    cases = _drawable_cases(edge, intersample)
    variants = [("hot", {}, _hot_store_fetched if intersample else _hot_tuple, ("default", "stretched"), True),
                ("cold", SINGLE, _cold_with_shortcuts, ("default", "stretched"), False)]
    if intersample:
        variants += [("hot, through the tuple", {"MMHIP_NO_FETCHED_RESULT": "1"}, _hot_tuple, ("default",), False),
                     ("cold, no shortcuts", LONG_WAY, _cold_without_shortcuts, ("default",), False)]
    for name, env, claim, flag_set, with_bytes in variants:
        renderers = {flags: _Renderer(R.FETCH[flags], env, claim, **opts) for flags in flag_set}
        for frame, flags, img, m, want in cases:
            if flags not in renderers:
                continue
            uv = R.map_uservals(m)
            _assert_same(renderers[flags].float_map(frame, img, uv), want, (name, frame, img.shape, flags, m))
            if with_bytes:
                got = renderers[flags].rgba8(frame, img, uv)
                assert np.array_equal(got, R.pack(want, 4)), (name, "bytes", frame, img.shape, flags, m)
    wild = _wild_cases(edge, intersample)
    for name, env, claim in (("hot", {}, lambda flt: None), ("cold", SINGLE, _cold)):
        r = _Renderer(R.WILD, env, claim, **opts)
        for img, uv, want_map, want_bytes in wild:
            _assert_same(r.float_map((40, 24), img, uv), want_map, ("wild", name, img.shape, uv))
            assert np.array_equal(r.rgba8((40, 24), img, uv), want_bytes), ("wild", name, "bytes", img.shape, uv)


@pytest.mark.parametrize("inc", [2, 3])
@pytest.mark.parametrize("edge", [(0, 0), (1, 2), (3, 3)], ids=lambda e: "edge%d%d" % e)
def test_strided_fetch(edge, inc):
    """pixel_inc 2 and 3, the preview's strided source: the hot and the cold fetch over the case table (the large
    scale is 1.5e8: the strided fetch's cap is 2**30 px), and the wild coordinates."""
    opts = dict(edge_x=edge[0], edge_y=edge[1], pixel_inc=inc)
    cases = _drawable_cases(edge, True, pixel_inc=inc, big=1.5e8)

    def strided(claim):
        def check(flt):
            claim(flt)
            assert _defines(flt, "MM_PIXEL_INC %d" % inc)
        return check
    for name, env, claim, flag_set in (("hot", {}, strided(_hot_store_fetched), ("default", "stretched")), ("cold", SINGLE, strided(_cold), ("default",))):
        renderers = {flags: _Renderer(R.FETCH[flags], env, claim, **opts) for flags in flag_set}
        for frame, flags, img, m, want in cases:
            if flags in renderers:
                _assert_same(renderers[flags].float_map(frame, img, R.map_uservals(m)), want, (name, frame, img.shape, flags, m))
    r = _Renderer(R.WILD, {}, lambda flt: None, **opts)
    for img, uv, want_map, _ in _wild_cases(edge, True, pixel_inc=inc):
        _assert_same(r.float_map((40, 24), img, uv), want_map, ("wild", img.shape, uv))


@pytest.mark.parametrize("intersample", [True, False], ids=["bilinear", "nearest"])
@pytest.mark.parametrize("edge", [(0, 0), (1, 2), (3, 3), (2, 1)], ids=lambda e: "edge%d%d" % e)
def test_per_pixel_frame_number(edge, intersample):
    """in(p, floor(x * 2 + 1.5)) on a sequence of three frames, hot (mm_select_frame) and with MMHIP_FRAME_HOT=0 (the
    generic fetch): frames -1 and 3 are white, but only where the edge tests let a tap through."""
    opts = dict(intersample=intersample, edge_x=edge[0], edge_y=edge[1])
    fetch = R.fetch_bilinear if intersample else R.fetch_nearest
    src = R.FETCH_FRAME.replace("{F}", R.FRAME_EXPR)

    def hot(flt):
        assert ("mm_orig_val_sums_hotf(A," if intersample else "mm_orig_val_hotf(A,") in _body(flt)

    def generic(flt):
        assert "_hotf(A," not in _body(flt)
    renderers = [("hot", _Renderer(src, {}, hot, **opts)), ("MMHIP_FRAME_HOT=0", _Renderer(src, {"MMHIP_FRAME_HOT": "0"}, generic, **opts))]
    seen = {"white": False, "edge colour first": False}
    for frame in R.FRAME_SIZES:
        for iw, ih in ((13, 7), (2, 3), (53, 37)):
            seq = R.random_frames(3, iw, ih, 5)
            factors = R.resize_factors(iw, ih, "default")
            for m in R.maps_for(iw, ih, factors)[:6]:
                c = _coords(frame, m)
                index = R.frame_index(c[..., 2])
                assert sorted(np.unique(index)) == [-1, 0, 1, 2, 3]
                want, covered = fetch(seq, c[..., 0], c[..., 1], edge, R.EDGE_COLOURS, factors=factors, frame=index)
                assert covered.all()
                pieces = R.frame_probe_oracle(lambda lit, k: _oracle(R.FETCH_FRAME.replace("{F}", lit), frame, R.map_uservals(m), seq[k], floatmap=True,
                                                                     intersample=intersample, edge=edge), index, 3)
                _assert_same(want, pieces, ("restatement against oracle", frame, (iw, ih), m))
                for name, r in renderers:
                    _assert_same(r.float_map(frame, seq, R.map_uservals(m)), want, (name, frame, (iw, ih), m))
                bad, white = (index < 0) | (index > 2), (want == 1.0).all(axis=-1)
                seen["white"] |= bool((white & bad).any())
                seen["edge colour first"] |= bool((~white & bad).any())
    assert seen["white"] and (seen["edge colour first"] or edge != (0, 0)), seen


# ---- render_image and the float-map fetch ------------------------------------------------------------------------------

@pytest.mark.parametrize("supersampling", [False, True], ids=["plain", "supersampling"])
@pytest.mark.parametrize("edge", [(0, 0), (1, 2), (3, 3), (2, 1)], ids=lambda e: "edge%d%d" % e)
def test_float_map_path(edge, supersampling):
    """b = gaussian_blur(in, 0, 0) is render_image's map of the drawable (k_render_drawable); b(p) samples it
    (mm_floatmap_pixel), as does c(p) for c = gaussian_blur(b, 0, 0) (a copy) and c = render(b) (k_render_floatmap).
    Frames with two pixels or more each way equal the restatement and the oracle; 1 x 7 and 9 x 1, whose maps divide
    by ax = 0, and the wild coordinates equal the oracle.  b = render(in) keeps the drawable's wrapper, so on a 13 x 7
    and a 9 x 30 image k_render_drawable samples beyond the edges: its own copy of the edge behaviours."""
    opts = dict(edge_x=edge[0], edge_y=edge[1], supersampling=supersampling)
    img = R.random_frames(1, 13, 7, 9)[0]
    kw = dict(floatmap=True, edge=edge, supersampling=supersampling)

    def claim(flt):
        assert _defines(flt, "MM_SUPERSAMPLING %d" % supersampling) and flt.num_native_calls >= 1
    renderers = {}
    tall = R.random_frames(1, 9, 30, 10)[0]
    for stretched, form, image in ((False, "blur", img), (True, "blur", img), (False, "blur_blur", img), (False, "blur_render", img),
                                 (False, "render", img), (False, "render", tall)):
        src = R.floatmap_probe(form, stretched)
        r = renderers[src] = renderers.get(src) or _Renderer(src, {}, claim, **opts)
        for frame in R.FLOATMAP_FRAMES:
            W, H = frame
            for m in R.maps_for(W, H, R.resize_factors(W, H, "stretched" if stretched else "default") if form != "render" else None):
                uv = R.map_uservals(m)
                want = _oracle(src, frame, uv, image, **kw)
                if W > 1 and H > 1:
                    c = _coords(frame, m, stretched)
                    ref, covered = R.floatmap_probe_reference(form, stretched, image, W, H, c[..., 0], c[..., 1], edge, R.EDGE_COLOURS, supersampling)
                    assert covered.all(), (frame, stretched, form, m)
                    _assert_same(ref, want, ("restatement against oracle", frame, stretched, form, m))
                _assert_same(r.float_map(frame, image, uv), want, (frame, stretched, form, m))
    # (k_render_floatmap's own conversion sees the new map's coordinates only: wild on the 1 x 7 and 9 x 1 frames above)
    src = R.floatmap_probe("blur", False, wild=True)
    r = _Renderer(src, {}, claim, **opts)
    for frame in ((40, 24), (5, 3)):
        for big in R.WILD_BIG:
            uv = {k: v for k, v in R.wild_uservals(big).items() if k != "vert"}
            _assert_same(r.float_map(frame, img, uv), _oracle(src, frame, uv, img, **kw), ("wild", frame, big))


# ---- the pixel store ---------------------------------------------------------------------------------------------------

def _render_padded(inv, w, h, bpp, pad, sentinel=0xA5):
    """The frame rendered at row_stride = w * bpp + pad into a buffer of sentinel bytes: (pixels [h, w, bpp], the rest)."""
    stride = w * bpp + pad
    size = h * stride + 64
    host = np.full(size, sentinel, np.uint8)
    dev = lib().mmhip_device_alloc(size)
    assert dev
    try:
        assert lib().mmhip_copy_to_device(C.c_void_p(dev), host.ctypes.data_as(C.c_void_p), size) == 0
        inv.render_rows(dev, 0, h, row_stride=stride, bpp=bpp)
        inv.sync()
        assert lib().mmhip_copy_to_host(host.ctypes.data_as(C.c_void_p), C.c_void_p(dev), size) == 0
    finally:
        lib().mmhip_device_free(C.c_void_p(dev))
    rows = host[:h * stride].reshape(h, stride)
    return rows[:, :w * bpp].reshape(h, w, bpp), np.concatenate([rows[:, w * bpp:].ravel(), host[h * stride:]])


@pytest.mark.parametrize("variant", ["scalar", "pair", "pair, MMHIP_PAIR_PACK=0"])
def test_output_bytes_of_the_ramp(variant):
    """RAMP's float map (every k / 255 as a grey, values around every byte boundary, below 0 and above 1, NaN, +-inf,
    -0) equals the oracle's, and the bytes at output_bpp 1 to 4 equal pack() of the GPU's own float map and the
    oracle's bytes: through mm_store_pixel, through the pair kernel's own pack (mm_store_pair) and through the pair
    kernel with MMHIP_PAIR_PACK=0, packed and with a padded row_stride whose sentinel bytes survive.  The frame holds
    white, which packs to grey 254, and every k at which a float32 evaluation of the grey sum would give another byte."""
    env = {"scalar": {"MMHIP_PAIR": "0"}, "pair": {"MMHIP_PAIR": "1"}, "pair, MMHIP_PAIR_PACK=0": {"MMHIP_PAIR": "1", "MMHIP_PAIR_PACK": "0"}}[variant]
    w, h = R.RAMP_SIZE
    with _environment(env):
        flt = mm.Filter(R.RAMP)
        assert flt.launch_geometry(w, h)["pair_mode"] == (variant != "scalar")
        assert ("mm_store_pair(A," in _body(flt)) == (variant == "pair")
        inv = flt.invoke(w, h)
        fmap = render_device(inv, w, h, floatmap=True)
        _assert_same(fmap, G.oracle(R.RAMP).render(w, h, floatmap=True), "the ramp's float map")
        census = G.special_census(fmap)
        assert all(census[k][c] >= w for k in ("nan", "-0", "+inf", "-inf") for c in range(4)), census
        unit = (np.arange(w) / 255.0).astype(np.float32)
        assert all(np.array_equal(fmap[row, :, c], unit) for row in range(3) for c in range(3))
        ks = R.grey_sensitive_ks()
        assert ks and 255 in ks
        for bpp in (1, 2, 3, 4):
            want = R.pack(fmap, bpp)
            assert np.array_equal(want, G.oracle(R.RAMP).render(w, h, bpp=bpp)), bpp
            got = render_device(inv, w, h, bpp=bpp)
            assert np.array_equal(got, want), (bpp, "packed rows", int((got != want).sum()), np.argwhere(got != want)[:4].tolist())
            padded, rest = _render_padded(inv, w, h, bpp, 12 if bpp == 4 else 5)
            assert np.array_equal(padded, want), (bpp, "padded rows", int((padded != want).sum()))
            assert (rest == 0xA5).all(), (bpp, "bytes between the rows were written")
            if bpp <= 2:
                single = np.trunc(R.grey_float32(unit, unit, unit).astype(np.float64)).astype(np.uint8)
                assert got[0, 255, 0] == 254 and all(got[row, k, 0] != single[k] for row in range(3) for k in ks), bpp
        assert np.array_equal(inv.render(), R.pack(fmap, 4))
