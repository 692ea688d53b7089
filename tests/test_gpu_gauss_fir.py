"""gaussian_blur on float maps: the FIR path (native_filters.hip: make_rle_curve, k_fir_same, k_fir_apply, gauss_rle,
render_input), and float-map inputs to both the FIR and the recursive path.

test_gauss_fir_path_matches_oracle compares RGBA8 bytes of one 333 x 251 drawable; a byte cannot see a wrong tap, a
window off by one at the clamped edge, a `same > 3n/4` switch off by one or a flushed denormal.  Here the float maps
themselves are compared with the oracle's, and on threshold_rows with the restatement of tests/gauss_reference.py
(pinned against the oracle by tests/test_gauss_reference.py), under one rule (gauss_reference.same_maps): NaN at the
same places, every other element the same bits, the sign of zero and denormals included.

Sizes: widths and heights of 1 and 2, lines shorter than the window (sigma 20 and 23 px on the other axis still take
the FIR path on both), odd sizes, more than one block of either kernel (257 x 3: 1028 line flags; 333 x 251).  Inputs:
random RGBA bytes (the full branch on every line), a flat image with steps (the encoded branch on its flat lines),
threshold_rows (both, the switch itself), a closure's map with inf, NaN, -0, mixed zeros and denormals, and a chained
blur's map.  State: one invocation through IIR and FIR frames in turn, as bytes and as float maps, and row bands."""
import numpy as np
import pytest

from tests import filters as F
from tests import gauss_reference as G
from tests.gpu_util import render_device

pytestmark = pytest.mark.gpu

_FILTERS = {}


def _filter(src):
    if src not in _FILTERS:
        import mathmap_amd as mm
        _FILTERS[src] = F.load(src) if src in F.NAMES else mm.Filter(src)
    return _FILTERS[src]


def _invocation(src, w, h, uv, img):
    inv = _filter(src).invoke(w, h)
    for k, v in uv.items():
        inv.set(k, v)
    inv.set_image("in", img)
    return inv


def _gpu_map(src, w, h, uv, img, rows=None):
    """The float map of a fresh invocation."""
    return render_device(_invocation(src, w, h, uv, img), w, h, rows=rows, floatmap=True)


def _oracle_map(src, w, h, uv, img):
    return G.oracle(src).render(w, h, uservals=uv, images={"in": img}, floatmap=True)


def _devs(w, h, hsig, vsig):
    hdev, vdev = G.devs_for(w, h, hsig, vsig)
    return {"hdev": hdev, "vdev": vdev}


def _assert_same(got, want, what):
    assert G.same_maps(got, want), (what, G.describe_difference(got, want))


@pytest.mark.parametrize("w,h", [(1, 1), (1, 7), (9, 1), (2, 2), (5, 3), (16, 16), (17, 33), (64, 48), (257, 3), (333, 251)])
def test_fir_drawable_input(w, h):
    """Sigma pairs in pixels (0.3, 0.2); (0.49, 20) and (23, 0.3), a window longer than the line at the small sizes;
    (0, 0.4), one pass skipped -- on random RGBA bytes and on a flat image with steps.  Bit for bit the oracle's map.
    The single pass of (0, 0.4) on the random bytes is also measured against the float64 evaluation and printed."""
    for name, img in (("random", G.random_rgba(w, h, w * 1000 + h)), ("stepped", G.stepped_flat(w, h))):
        for hsig, vsig in ((0.3, 0.2), (0.49, 20.0), (23.0, 0.3), (0.0, 0.4)):
            uv = _devs(w, h, hsig, vsig)
            hs, vs = G.sigmas(w, h, uv["hdev"], uv["vdev"])
            assert G.takes_fir(hs, vs)
            got = _gpu_map("gauss_direct", w, h, uv, img)
            _assert_same(got, _oracle_map("gauss_direct", w, h, uv, img), (name, w, h, hsig, vsig))
            if name == "random" and hsig == 0.0 and w > 1 and h > 1:
                dist, share, length = G.f64_distance(got, G.as_map(img), vs, 0)
                print("f64_distance", (w, h), "sigma %g axis 0 L %d:" % (vsig, length), "%.3f of at most %d," % (dist, G.f64_bound_units(length)), "covered", share)
                assert dist <= G.f64_bound_units(length), (w, h, dist)


@pytest.mark.parametrize("n", [4, 5, 7, 8, 16, 17])
def test_threshold_rows(n):
    """Rows with `same` at (3n)//4 - 1, (3n)//4, (3n)//4 + 1 and n, vdev = 0 so that rows are the lines: the map equals
    the oracle's and the restatement's, whose flags say that both branches ran and where the switch fell."""
    h = 8
    img = G.threshold_rows(n, h)
    for hsig in (0.3, 0.49, 6.0):
        uv = _devs(n, h, hsig, 0.0)
        hs, vs = G.sigmas(n, h, uv["hdev"], 0.0)
        want, flags = G.gauss_blur_map(G.as_map(img), hs, vs)
        assert list(flags) == [1] and not flags[1][0::4].any() and not flags[1][1::4].any() and flags[1][2::4].all() and flags[1][3::4].all()
        got = _gpu_map("gauss_direct", n, h, uv, img)
        _assert_same(got, _oracle_map("gauss_direct", n, h, uv, img), ("oracle", n, hsig))
        _assert_same(got, want, ("restatement", n, hsig))


@pytest.mark.parametrize("hsig,vsig", [(0.3, 0.4), (0.3, 3.0)])
def test_fir_float_map_with_special_values(hsig, vsig):
    """SPECIAL_CLOSURE at 40 x 24: the closure's map (+inf, -inf, NaN, a channel of -0, rows of mixed zeros,
    denormals, values beyond [0, 1]) reaches the FIR kernels as a float map.  The map at deviation 0 is the closure's
    own (the special values arrive); the blurred map has its NaN where the oracle's are and its bits elsewhere."""
    w, h = 40, 24
    img = G.random_rgba(w, h, 7)
    m0 = _gpu_map(G.SPECIAL_CLOSURE, w, h, {"hdev": 0.0, "vdev": 0.0}, img)
    _assert_same(m0, _oracle_map(G.SPECIAL_CLOSURE, w, h, {"hdev": 0.0, "vdev": 0.0}, img), "the closure's map")
    census = G.special_census(m0)
    assert census["+inf"][0] and census["-inf"][0] and census["nan"][1] and census["-0"][3] == w * h and census["-0"][2] and census["+0"][2] \
        and census["denormal"][2] > 100, census
    uv = _devs(w, h, hsig, vsig)
    assert G.takes_fir(*G.sigmas(w, h, uv["hdev"], uv["vdev"]))
    got = _gpu_map(G.SPECIAL_CLOSURE, w, h, uv, img)
    want = _oracle_map(G.SPECIAL_CLOSURE, w, h, uv, img)
    _assert_same(got, want, (hsig, vsig))
    out = G.special_census(got)
    assert out["denormal"][2] > 100 and out["+0"][3] == w * h and 0 < out["nan"][1] < w * h, out


def test_fir_on_a_chained_blur():
    """c = gaussian_blur(gaussian_blur(in, wide, wide), narrow, narrow), written as two statements; the inner blur is
    recursive, the outer one FIR: its input is a float map whose values are no k / 255."""
    w, h = 40, 24
    img = G.random_rgba(w, h, 8)
    uv = {"wide": 0.2, "narrow": 0.02}
    assert not G.takes_fir(*G.sigmas(w, h, uv["wide"], uv["wide"])) and G.takes_fir(*G.sigmas(w, h, uv["narrow"], uv["narrow"]))
    got = _gpu_map(G.CHAINED, w, h, uv, img)
    _assert_same(got, _oracle_map(G.CHAINED, w, h, uv, img), "chained")
    inner = _oracle_map(G.CHAINED, w, h, {"wide": 0.2, "narrow": 0.0}, img)
    assert not np.array_equal(np.round(inner * 255) / 255, inner)


@pytest.mark.parametrize("w,h", [(40, 24), (16, 16), (17, 33)])
def test_iir_float_map_with_special_values(w, h):
    """SPECIAL_CLOSURE at sigma (2.0, 1.5): the recursive path on a plain float map (MapSrc, which may hold -0 and is
    not known finite).  The channels that hold inf or NaN come out all NaN on both sides; blue (mixed zeros,
    denormals, values in [-3, 0]) and alpha (-0 throughout) equal the oracle's bit for bit."""
    img = G.random_rgba(w, h, 7)
    uv = _devs(w, h, 2.0, 1.5)
    assert not G.takes_fir(*G.sigmas(w, h, uv["hdev"], uv["vdev"]))
    got = _gpu_map(G.SPECIAL_CLOSURE, w, h, uv, img)
    want = _oracle_map(G.SPECIAL_CLOSURE, w, h, uv, img)
    for side in (got, want):
        assert np.isnan(side[..., :2]).all() and not np.isnan(side[..., 2:]).any()
    _assert_same(got, want, (w, h))
    assert want[..., 2].any() and not want[..., 3].any() and not np.signbit(got[..., 3]).any()


STATE_STEPS = [("iir", 3.0, 2.0), ("fir", 0.3, 0.4), ("iir again", 3.0, 2.0), ("fir again", 0.3, 0.4), ("deviations 0", 0.0, 0.0)]


def test_one_invocation_through_iir_and_fir_frames():
    """One gauss_direct invocation rendered IIR, FIR, IIR, FIR, deviations 0: once as bytes through render() (the IIR
    frames are packed by the blur itself, NativeDirectOut with skip_map; the FIR frames go through the map), once as
    float maps, once alternating the two.  Every frame equals a fresh invocation's and the oracle's."""
    w, h = 75, 51
    img = G.random_rgba(w, h, 61)
    orc = G.oracle("gauss_direct")
    want8, want32 = {}, {}
    for what, hsig, vsig in STATE_STEPS:
        uv = _devs(w, h, hsig, vsig)
        assert G.takes_fir(*G.sigmas(w, h, uv["hdev"], uv["vdev"])) == (not what.startswith("iir"))
        want8[what] = orc.render(w, h, uservals=uv, images={"in": img})
        want32[what] = _oracle_map("gauss_direct", w, h, uv, img)
        assert np.array_equal(_invocation("gauss_direct", w, h, uv, img).render(), want8[what]), (what, "fresh, bytes")
        _assert_same(_gpu_map("gauss_direct", w, h, uv, img), want32[what], (what, "fresh, float map"))
    assert not np.array_equal(want8["iir"], want8["fir"]) and not np.array_equal(want8["fir"], want8["deviations 0"])
    for mode in ("bytes", "float maps", "alternating"):
        inv = _invocation("gauss_direct", w, h, {}, img)
        for k, (what, hsig, vsig) in enumerate(STATE_STEPS):
            for name, v in _devs(w, h, hsig, vsig).items():
                inv.set(name, v)
            if mode == "bytes" or (mode == "alternating" and k % 2 == 0):
                assert np.array_equal(inv.render(), want8[what]), (mode, what)
            if mode == "float maps" or (mode == "alternating" and k % 2 == 1):
                _assert_same(render_device(inv, w, h, floatmap=True), want32[what], (mode, what))


def test_fir_frame_in_two_row_bands():
    """A FIR frame rendered as rows [0, h/2) and [h/2, h) equals the whole frame, as a float map and as bytes."""
    w, h = 75, 51
    img = G.random_rgba(w, h, 62)
    uv = _devs(w, h, 0.3, 0.4)
    bands = [(0, h // 2), (h // 2, h)]
    whole = _gpu_map("gauss_direct", w, h, uv, img)
    _assert_same(_gpu_map("gauss_direct", w, h, uv, img, rows=bands), whole, "float map")
    _assert_same(whole, _oracle_map("gauss_direct", w, h, uv, img), "oracle")
    inv = _invocation("gauss_direct", w, h, uv, img)
    assert np.array_equal(render_device(inv, w, h, rows=bands), _invocation("gauss_direct", w, h, uv, img).render())


def test_taps_larger_than_the_checkpoints():
    """64 x 64, hdev 0.01, vdev 76.3: about 2403 px on the vertical axis, a curve of length 8002.  Flags, taps and sums
    take 129064 bytes where the recursive path's checkpoints (and what used to be reserved for the FIR path) take
    102912: the plan reserves what the curve needs.  Bit for bit the oracle's map; the vertical pass alone is also
    measured against the float64 evaluation."""
    w, h = 64, 64
    img = G.random_rgba(w, h, 63)
    uv = {"hdev": 0.01, "vdev": 76.3}
    hs, vs = G.sigmas(w, h, uv["hdev"], uv["vdev"])
    assert G.takes_fir(hs, vs) and G.rle_curve(vs)[0] == 8002 and G.rle_curve(hs)[0] == 2
    assert max(w, h) * 16 + 2 * (2 * 8002 + 1) * 4 == 129064
    _assert_same(_gpu_map("gauss_direct", w, h, uv, img), _oracle_map("gauss_direct", w, h, uv, img), "both passes")
    uv["hdev"] = 0.0
    got = _gpu_map("gauss_direct", w, h, uv, img)
    _assert_same(got, _oracle_map("gauss_direct", w, h, uv, img), "vertical pass")
    dist, share, length = G.f64_distance(got, G.as_map(img), vs, 0)
    print("f64_distance", (w, h), "sigma %g axis 0 L %d:" % (vs, length), "%.3f of at most %d," % (dist, G.f64_bound_units(length)), "covered", share)
    assert share == 1.0 and dist <= G.f64_bound_units(length), (dist, share)
