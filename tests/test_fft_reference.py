"""tests/fft_reference.py against the CPU oracle: the numpy float64 restatements of convolve, half_convolve and
visualize_fft equal the float maps of the oracle's direct long-double DFT (oracle/mm_oracle_fft.c) within
assert_fft_close.  That pins the helper for the GPU tests, which use it at sizes the oracle cannot reach, and shows
that two independent exact implementations stay inside the conditions the GPU is then held to.  No GPU."""
import numpy as np
import pytest

from tests import fft_reference as R

SIZES = [(2, 2), (3, 5), (2, 9), (8, 2), (75, 51), (127, 61)]


def _images(name, w, h, seed, make=R.random_rgba):
    images = {"in": make(w, h, seed)}
    if R.SECOND_IMAGE[name]:
        images[R.SECOND_IMAGE[name]] = make(w, h, seed + 1)
    return images


@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("name", sorted(R.FLAGS))
def test_restatement_equals_oracle_on_random_rgba(name, w, h):
    """Dense random RGBA bytes, every flag combination, both parities of both dimensions, widths and heights of 2
    and 3 (where visualize_fft's two column ranges overlap) and prime lengths."""
    images = _images(name, w, h, seed=w * 1000 + h)
    for uv in R.FLAGS[name]:
        want = R.oracle(name).render(w, h, uservals=uv, images=images, floatmap=True)
        got = R.restated(name, uv, images)
        R.assert_fft_close(got, want, (name, w, h, uv))
        if uv.get("copy_alpha"):
            assert np.array_equal(want[..., 3], R.as_map(images["in"])[..., 3]), (name, w, h, uv)
        if uv.get("ignore_alpha"):
            assert np.array_equal(want[..., 3], np.ones((h, w), np.float32)), (name, w, h, uv)


@pytest.mark.parametrize("name", sorted(R.FLAGS))
def test_restatement_equals_oracle_on_smooth_inputs(name):
    """The smooth synthetic image with a textured alpha plane, and for convolve the Gaussian blob kernel of the
    byte-level parity test: spectra that fall off by many orders of magnitude, unlike random bytes."""
    w, h = 75, 51
    images = _images(name, w, h, seed=3, make=R.textured_rgba)
    if name == "convolve":
        images["kernel"] = R.blob_kernel(w, h)
    for uv in R.FLAGS[name]:
        want = R.oracle(name).render(w, h, uservals=uv, images=images, floatmap=True)
        R.assert_fft_close(R.restated(name, uv, images), want, (name, "smooth", uv))


def test_assert_fft_close_rejects_float_precision_slips():
    """The comparison itself: a map whose every element moved by one float ulp, one element moved by two ulps, a
    NaN at another place and a value where the reference holds zero are all refused; a handful of one-ulp
    differences and a 1e-15 where the reference holds 5e-18 pass."""
    rng = np.random.default_rng(5)
    want = rng.random((40, 50, 4)).astype(np.float32) + np.float32(0.5)
    want[3, 4, 1] = 0.75                                 # the poked element: mid-binade
    R.assert_fft_close(want.copy(), want, "same")
    few = want.copy()
    few[::20, ::25, 0] = np.nextafter(few[::20, ::25, 0], np.float32(4))       # 4 of 8000 elements
    R.assert_fft_close(few, want, "few")
    tiny, ref = want.copy(), want.copy()
    tiny[..., 3], ref[..., 3] = 1e-15, 5e-18
    ref[0, 0, 3] = tiny[0, 0, 3] = 2000.0
    with pytest.raises(AssertionError):
        R.assert_fft_close(tiny, ref, "tiny")            # passes the tolerance, but every alpha differs
    tiny[1:, :, 3] = ref[1:, :, 3]
    tiny[0, 9:, 3] = ref[0, 9:, 3]
    R.assert_fft_close(tiny, ref, "tiny, few")
    for what, edit in (("all one ulp", lambda m: np.nextafter(m, np.float32(4))),
                       ("one element two ulps", lambda m: _poke(m, np.nextafter(np.nextafter(m[3, 4, 1], np.float32(4)), np.float32(4)))),
                       ("nan", lambda m: _poke(m, np.nan)),
                       ("inf", lambda m: _poke(m, np.inf)),
                       ("nonzero at zero", None)):
        if edit is None:
            ref = want.copy()
            ref[3, 4, 1] = 0.0
            bad = ref.copy()
            bad[3, 4, 1] = 1e-9
        else:
            ref, bad = want, edit(want.copy())
        with pytest.raises(AssertionError):
            R.assert_fft_close(bad, ref, what)


def _poke(m, v):
    m[3, 4, 1] = v
    return m
