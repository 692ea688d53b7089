"""tests/fetch_reference.py against the CPU oracle: the numpy restatement of the image fetch (edge behaviours, the
nearest, bilinear and strided fetches, per-pixel frame numbers), of render_image's drawable branch with the float-map
fetch behind it, and of the pixel store, written from builtins.c / new_template.c.in, equals the oracle's float maps
and bytes bit for bit over the whole case table of tests/test_gpu_fetch.py, with every pixel of the table covered (the
wild coordinates, left to the oracle, are not in it).  That pins the helper and shows that two independent
transcriptions of the reference agree to the bit, which the HIP kernels are then held to.  It also computes the two
facts about the grey pack the GPU test relies on.  No GPU."""
import numpy as np
import pytest

from tests import fetch_reference as R
from tests import gauss_reference as G

_COORDS = {}


def _coords(frame, m, stretched=False):
    """The oracle's coordinate arrays of map `m` on `frame`: [h, w, 4] = (p[0], p[1], x, y)."""
    key = (frame, m[1:], stretched)
    if key not in _COORDS:
        _COORDS[key] = G.oracle(R.COORDS[stretched]).render(frame[0], frame[1], uservals=R.map_uservals(m), floatmap=True)
    return _COORDS[key]


def _oracle(src, frame, m, img, **kw):
    return G.oracle(src).render(frame[0], frame[1], uservals=R.map_uservals(m), images={"in": img}, floatmap=True,
                                edge_colors=R.EDGE_COLOURS, **kw)


def _assert_same(got, covered, want, what):
    assert covered.all(), (what, "not covered:", int((~covered).sum()))
    assert G.same_maps(got, want), (what, G.describe_difference(got, want))


@pytest.mark.parametrize("intersample", [True, False], ids=["bilinear", "nearest"])
@pytest.mark.parametrize("edge", R.EDGE_PAIRS, ids=lambda e: "edge%d%d" % e)
def test_fetch_equals_oracle_bit_for_bit(edge, intersample):
    """Both frames x every image size x default and stretched image x every map: the oracle's float map equals
    fetch_bilinear / fetch_nearest at the oracle's own coordinate arrays, every pixel covered."""
    fetch = R.fetch_bilinear if intersample else R.fetch_nearest
    for frame in R.FRAME_SIZES:
        for iw, ih in R.image_sizes_for(frame):
            img = R.random_frames(1, iw, ih, iw * 100 + ih)[0]
            for flags in ("default", "stretched"):
                factors = R.resize_factors(iw, ih, flags)
                for m in R.maps_for(iw, ih, factors):
                    c = _coords(frame, m)
                    got, covered = fetch(img, c[..., 0], c[..., 1], edge, R.EDGE_COLOURS, factors=factors)
                    want = _oracle(R.FETCH[flags], frame, m, img, intersample=intersample, edge=edge)
                    _assert_same(got, covered, want, (frame, (iw, ih), flags, m[0]))


def test_the_aspect_wrapper_and_the_edges_take_part():
    """What the table is for: a non-square image on a frame of another aspect has factors other than 1, leaving them
    out changes the result, and so does every edge behaviour, on either axis."""
    frame, (iw, ih) = (40, 24), (9, 30)
    factors = R.resize_factors(iw, ih, "default")
    assert factors[0] == np.float32(np.float32(30) / np.float32(9)) and factors[1] == 1.0 and R.resize_factors(iw, ih, "stretched") is None
    assert R.resize_factors(53, 37, "default") == (1.0, np.float32(np.float32(53) / np.float32(37)))
    img = R.random_frames(1, iw, ih, 1)[0]
    m = R.maps_for(iw, ih, factors)[4]
    assert m[0] == "affine"
    c = _coords(frame, m)
    maps = {}
    for edge in R.EDGE_PAIRS:
        maps[edge], _ = R.fetch_bilinear(img, c[..., 0], c[..., 1], edge, R.EDGE_COLOURS, factors=factors)
    assert len({v.tobytes() for v in maps.values()}) == 16
    bare, _ = R.fetch_bilinear(img, c[..., 0], c[..., 1], (0, 0), R.EDGE_COLOURS, factors=None)
    assert not np.array_equal(bare, maps[(0, 0)])
    assert np.array_equal(bare.view(np.uint32), _oracle(R.FETCH["stretched"], frame, m, img, edge=(0, 0)).view(np.uint32))


@pytest.mark.parametrize("edge", R.EDGE_PAIRS, ids=lambda e: "edge%d%d" % e)
def test_nearest_fetch_at_wild_coordinates_wraps_like_x86(edge):
    """The nearest fetch has no weights, so its restatement reaches past `covered`: NaN, +-inf and coordinates beyond
    2**31 px become INT_MIN (cvttsd2si), which REFLECT and ROTATE negate and mirror in wrapping ints -- INT_MIN % 13 is
    -11, outside the image, hence an edge colour.  The oracle must do the same whatever its compiler makes of the
    overflow (an image whose sides are powers of two cannot tell: INT_MIN % 2**k is 0)."""
    frame = (40, 24)
    for iw, ih in ((13, 7), (53, 37)):
        img = R.random_frames(1, iw, ih, iw * 100 + ih)[0]
        factors = R.resize_factors(iw, ih, "default")
        for big in R.WILD_BIG:
            for vert in (0, 1):
                uv = R.wild_uservals(big, vert)
                c = G.oracle(R.WILD_COORDS).render(frame[0], frame[1], uservals=uv, images={"in": img}, floatmap=True)
                got, covered = R.fetch_nearest(img, c[..., 0], c[..., 1], edge, R.EDGE_COLOURS, factors=factors)
                assert not covered.all()
                want = G.oracle(R.WILD).render(frame[0], frame[1], uservals=uv, images={"in": img}, floatmap=True, intersample=False,
                                               edge=edge, edge_colors=R.EDGE_COLOURS)
                assert G.same_maps(got, want), ((iw, ih), big, vert, G.describe_difference(got, want))


@pytest.mark.parametrize("inc", [2, 3])
@pytest.mark.parametrize("edge", [(0, 0), (1, 2), (3, 3)], ids=lambda e: "edge%d%d" % e)
def test_strided_fetch_equals_oracle_bit_for_bit(edge, inc):
    """pixel_inc 2 and 3 (builtins.c:186-216) over the same table; the large scale is 1.5e8, which keeps the 13-wide
    image's coordinate under the strided fetch's 2**30 px."""
    for frame in R.FRAME_SIZES:
        for iw, ih in R.image_sizes_for(frame):
            img = R.random_frames(1, iw, ih, iw * 100 + ih)[0]
            for flags in ("default", "stretched"):
                factors = R.resize_factors(iw, ih, flags)
                for m in R.maps_for(iw, ih, factors, big=1.5e8):
                    c = _coords(frame, m)
                    got, covered = R.fetch_bilinear(img, c[..., 0], c[..., 1], edge, R.EDGE_COLOURS, factors=factors, pixel_inc=inc)
                    want = _oracle(R.FETCH[flags], frame, m, img, edge=edge, pixel_inc=inc)
                    _assert_same(got, covered, want, (frame, (iw, ih), flags, m[0]))
    full, _ = R.fetch_bilinear(img, c[..., 0], c[..., 1], edge, R.EDGE_COLOURS, factors=factors)
    assert not np.array_equal(full, got)


@pytest.mark.parametrize("intersample", [True, False], ids=["bilinear", "nearest"])
@pytest.mark.parametrize("edge", [(0, 0), (1, 2), (3, 3), (2, 1)], ids=lambda e: "edge%d%d" % e)
def test_per_pixel_frame_number_equals_oracle(edge, intersample):
    """in(p, floor(x * 2 + 1.5)) on three frames: numbers -1 .. 3 across the frame.  The restatement, given the index
    array, equals the oracle's renders per frame number put together by that index; frames -1 and 3 are white only
    where the tap is inside the image (the edge colours come first)."""
    fetch = R.fetch_bilinear if intersample else R.fetch_nearest
    seen = {"white": False, "edge colour first": False}
    for frame in R.FRAME_SIZES:
        for iw, ih in ((13, 7), (2, 3), (53, 37)):
            seq = R.random_frames(3, iw, ih, 5)
            factors = R.resize_factors(iw, ih, "default")
            for m in R.maps_for(iw, ih, factors)[:6]:
                c = _coords(frame, m)
                index = R.frame_index(c[..., 2])
                assert sorted(np.unique(index)) == [-1, 0, 1, 2, 3]
                got, covered = fetch(seq, c[..., 0], c[..., 1], edge, R.EDGE_COLOURS, factors=factors, frame=index)
                want = R.frame_probe_oracle(lambda lit, k: _oracle(R.FETCH_FRAME.replace("{F}", lit), frame, m, seq[k],
                                                                   intersample=intersample, edge=edge), index, 3)
                _assert_same(got, covered, want, (frame, (iw, ih), m[0]))
                bad, white = (index < 0) | (index > 2), (got == 1.0).all(axis=-1)
                seen["white"] |= bool((white & bad).any())
                seen["edge colour first"] |= bool((~white & bad).any())
    assert seen["white"] and (seen["edge colour first"] or edge != (0, 0)), seen


@pytest.mark.parametrize("supersampling", [False, True], ids=["plain", "supersampling"])
@pytest.mark.parametrize("edge", [(0, 0), (1, 2), (3, 3), (2, 1)], ids=lambda e: "edge%d%d" % e)
def test_float_map_path_equals_oracle_bit_for_bit(edge, supersampling):
    """render_image of the drawable (the nearest fetch, with and without the + 0.5), then get_floatmap_pixel on that
    map, on its copy and on render()'s resampling of it, for a default and a stretched filter, on every frame size
    with two pixels or more each way (a frame one pixel wide or high divides by ax = 0: not covered, the oracle's alone).
    b = render(in) keeps the drawable's wrapper: on a 13 x 7 and a 9 x 30 image render_image samples beyond the edges."""
    img13, tall = R.random_frames(1, 13, 7, 9)[0], R.random_frames(1, 9, 30, 10)[0]
    img = img13
    for frame in R.FLOATMAP_FRAMES:
        W, H = frame
        for stretched in (False, True):
            wrapper = R.resize_factors(W, H, "stretched" if stretched else "default")
            for form, img in (("blur", img13), ("blur_blur", img13), ("blur_render", img13), ("render", img13), ("render", tall)):
                for m in R.maps_for(W, H, wrapper if form != "render" else None):
                    c = _coords(frame, m, stretched)
                    got, covered = R.floatmap_probe_reference(form, stretched, img, W, H, c[..., 0], c[..., 1], edge, R.EDGE_COLOURS, supersampling)
                    want = _oracle(R.floatmap_probe(form, stretched), frame, m, img, edge=edge, supersampling=supersampling)
                    if W > 1 and H > 1:
                        _assert_same(got, covered, want, (frame, stretched, form, m[0]))
                    else:
                        assert not covered.any(), (frame, form, m[0])
    b, ok = R.float_map_of(img, 40, 24, edge, R.EDGE_COLOURS, supersampling=supersampling)
    other, _ = R.float_map_of(img, 40, 24, edge, R.EDGE_COLOURS, supersampling=not supersampling)
    assert ok.all() and not np.array_equal(b, other)
    if edge != (3, 3):
        plain = {e: R.float_map_of(tall, 40, 24, e, R.EDGE_COLOURS, factors=R.resize_factors(9, 30, "default"))[0] for e in (edge, (3, 3))}
        assert not np.array_equal(plain[edge], plain[(3, 3)])      # the edge behaviour takes part in render(in)


def test_float_map_fetch_rounds_ties_to_even_and_is_black_outside():
    """lrintf on a 5 x 3 map: x = 0.25 is column 2.5 -> 2, x = 0.75 is column 3.5 -> 4, x = -1.25 is column -0.5 -> 0
    (-0 is inside), x = 1.25 is column 4.5 -> 4, x = 1.26 is outside: black, whatever the edge behaviour."""
    fmap = np.arange(60, dtype=np.float32).reshape(3, 5, 4) + 1
    x = np.array([0.25, 0.75, -1.25, 1.25, 1.26, -1.26], np.float32)
    got, covered = R.float_map_fetch(fmap, x, np.zeros(6, np.float32))
    assert covered.all() and got[:, 0].tolist() == [fmap[1, 2, 0], fmap[1, 4, 0], fmap[1, 0, 0], fmap[1, 4, 0], 0.0, 0.0]
    for wild in (np.inf, -np.inf, np.nan, 2.0 ** 31, 1e19):
        assert not R.float_map_fetch(fmap, np.array([wild], np.float32), np.zeros(1, np.float32))[1].any()


@pytest.mark.parametrize("bpp", [1, 2, 3, 4])
def test_pack_equals_oracle_on_the_ramp(bpp):
    """The ramp's bytes at every output_bpp equal pack() of the ramp's own float map; the map holds what it promises."""
    w, h = R.RAMP_SIZE
    ramp = G.oracle(R.RAMP).render(w, h, floatmap=True)
    census = G.special_census(ramp)
    assert all(census[k][c] >= w for k in ("nan", "-0", "+inf", "-inf") for c in range(4)), census
    assert ramp.min(initial=0, where=np.isfinite(ramp)) <= -1.0 and ramp.max(initial=0, where=np.isfinite(ramp)) >= 2.0
    unit = (np.arange(w) / 255.0).astype(np.float32)
    assert all(np.array_equal(ramp[row, :, c], unit) for row in range(3) for c in range(3))
    assert np.array_equal(R.pack(ramp, bpp), G.oracle(R.RAMP).render(w, h, bpp=bpp))


def test_grey_pack_facts():
    """White packs to grey 254 ((0.299 + 0.587 + 0.114) * 255.0 is 254.99999999999997 in double), and for some
    r = g = b = k / 255 a float32 evaluation of the sum gives another byte: the set the GPU test looks for."""
    one = np.ones(1, np.float32)
    assert R.grey_double(one, one, one)[0] < 255.0 and R.pack(np.ones((1, 1, 4), np.float32), 1)[0, 0, 0] == 254
    assert R.pack(np.ones((1, 1, 4), np.float32), 2).tolist() == [[[254, 255]]]
    ks = R.grey_sensitive_ks()
    print("float32-sensitive k:", ks)
    assert ks and 255 in ks
    special = np.array([[[np.nan, -0.0, np.inf, -np.inf], [2.0, -1.0, 0.5, np.nan]]], np.float32)
    assert R.pack(special, 4).tolist() == [[[0, 0, 255, 0], [255, 0, 127, 0]]]
    assert R.pack(special, 3).tolist() == [[[0, 0, 255], [255, 0, 127]]]
    assert R.pack(special, 2)[0, :, 1].tolist() == [0, 0]


def test_apply_edge_behaviour_is_c_arithmetic():
    """C's `%` keeps the dividend's sign, -INT_MIN is INT_MIN, and ROTATE's mirror of the other axis is seen by the
    second switch: against a scalar transcription of builtins.c:40-119 on values around the edges and at the int limits."""
    def scalar(x, y, w, h, ex, ey):
        def wrap(v):
            return (v + 2 ** 31) % 2 ** 32 - 2 ** 31

        def mod(a, n):
            return int(np.fmod(a, n))
        if ex == 1:
            x = mod(x, w) + w if x < 0 else (mod(x, w) if x >= w else x)
        elif ex in (2, 3):
            if x < 0 or x >= w:
                x = mod(wrap(-x), w) if x < 0 else (w - 1) - mod(x, w)
                if ex == 3:
                    y = wrap((h - 1) - y)
        if ey == 1:
            y = mod(y, h) + h if y < 0 else (mod(y, h) if y >= h else y)
        elif ey in (2, 3):
            if y < 0 or y >= h:
                y = mod(wrap(-y), h) if y < 0 else (h - 1) - mod(y, h)
                if ey == 3:
                    x = wrap((w - 1) - x)
        return x, y
    vals = np.array([-2 ** 31, -2 ** 31 + 1, -1000, -14, -13, -8, -7, -1, 0, 1, 6, 7, 12, 13, 14, 26, 1000, 2 ** 31 - 1], np.int64)
    xs, ys = [a.ravel() for a in np.meshgrid(vals, vals)]
    for w, h in ((13, 7), (1, 1), (2, 3)):
        for edge in R.EDGE_PAIRS:
            gx, gy = R.apply_edge_behaviour(xs, ys, w, h, edge)
            want = [scalar(int(x), int(y), w, h, *edge) for x, y in zip(xs, ys)]
            assert gx.tolist() == [v[0] for v in want] and gy.tolist() == [v[1] for v in want], (w, h, edge)
    assert R.apply_edge_behaviour(np.array([-1]), np.array([0]), 13, 7, (1, 0))[0][0] == 12      # -1 % 13 is -1 in C
    assert R.apply_edge_behaviour(np.array([13]), np.array([0]), 13, 7, (2, 0))[0][0] == 12      # (w - 1) - 13 % 13
