"""The FFT native filters (native_fft.hip: hipFFT in double plus seven hand-written kernels) on float maps.

test_fft_native_filters_match_oracle compares RGBA8 bytes of opaque RGB inputs within 1 LSB: half of its convolve
cases saturate every byte, alpha is 255 throughout, and 1 LSB admits relative errors of 1/255.  Here the float maps
themselves are compared, with RGBA inputs whose alpha plane carries a texture, against references far more exact
than the float they are stored into: the oracle's direct long-double DFT, and -- pinned against it by
tests/test_fft_reference.py -- numpy float64 restatements at the sizes the oracle cannot reach.  The conditions
(assert_fft_close: one float ulp, at most 0.1 % of the elements differing at all) are stated in
tests/fft_reference.py.

Sizes: both parities of both dimensions, widths and heights of 2 and 3 (where visualize_fft's two column ranges
overlap), prime lengths (127, 61, 251: rocFFT's non-radix path), one past the 262144 pixels at which the
normalisation sum starts its grid-stride loop, and width or height 1.  State: one invocation rendered many times
with changing arguments, sizes and images; two FFT calls with different channel counts in one frame; inputs of
another size than the canvas."""
import numpy as np
import pytest

from tests import filters as F
from tests import fft_reference as R
from tests.gpu_util import render_device

pytestmark = pytest.mark.gpu

ORACLE_MAX_PIXELS = 127 * 61          # above it the numpy restatement is the reference

# two FFT calls in one frame: a 3-channel convolve whose float map the 4-channel visualize_fft takes as it is
TWO_FFTS = """
filter two_ffts (image in, image kernel)
  c = convolve(in, kernel, 1, 1);
  v = visualize_fft(c, 0);
  p = v(xy);
  q = c(xy);
  rgba:[p[0], q[1], p[3], q[3]]
end
"""

_FILTERS = {}


def _filter(src):
    if src not in _FILTERS:
        import mathmap_amd as mm
        _FILTERS[src] = F.load(src) if src in F.NAMES else mm.Filter(src)
    return _FILTERS[src]


def _invocation(src, w, h, uv, images, render_size=None):
    inv = _filter(src).invoke(w, h)
    for k, v in uv.items():
        inv.set(k, v)
    for k, v in images.items():
        inv.set_image(k, v)
    if render_size:
        inv.set_render_size(*render_size)
    return inv


def _gpu_map(src, w, h, uv, images, render_size=None):
    """The float map of a fresh invocation."""
    rw, rh = render_size or (w, h)
    return render_device(_invocation(src, w, h, uv, images, render_size), rw, rh, floatmap=True)


def _oracle_map(src, w, h, uv, images, render_size=None):
    return R.oracle(src).render(w, h, uservals=uv, images=images, floatmap=True, render_size=render_size)


def _images(name, w, h, seed):
    images = {"in": R.random_rgba(w, h, seed)}
    if R.SECOND_IMAGE[name]:
        images[R.SECOND_IMAGE[name]] = R.random_rgba(w, h, seed + 1)
    return images


def _check_alpha(got, uv, images, what):
    if uv.get("copy_alpha"):
        assert np.array_equal(got[..., 3].view(np.uint32), R.as_map(images["in"])[..., 3].view(np.uint32)), (what, "alpha is not the input's")
    if uv.get("ignore_alpha"):
        assert np.array_equal(got[..., 3].view(np.uint32), np.ones(got.shape[:2], np.float32).view(np.uint32)), (what, "alpha is not 1.0")


@pytest.mark.parametrize("w,h", [(2, 2), (3, 5), (2, 9), (8, 2), (75, 51), (96, 64), (127, 61), (251, 129)])
@pytest.mark.parametrize("name", sorted(R.FLAGS))
def test_float_map_parity(name, w, h):
    """Every flag combination on random RGBA bytes: within assert_fft_close of the oracle (numpy above 127x61);
    with copy_alpha the alpha plane is the input's bit for bit, with ignore_alpha exactly 1.0.  Prints, per case,
    (largest distance in float ulps, share of elements that differ at all)."""
    images = _images(name, w, h, seed=w * 1000 + h)
    for uv in R.FLAGS[name]:
        what = (name, w, h, uv)
        got = _gpu_map(name, w, h, uv, images)
        want = _oracle_map(name, w, h, uv, images) if w * h <= ORACLE_MAX_PIXELS else R.restated(name, uv, images)
        print("fft_distance", what, R.fft_distance(got, want))
        R.assert_fft_close(got, want, what)
        _check_alpha(got, uv, images, what)


def test_normalisation_sum_past_the_grid_stride_threshold():
    """convolve with normalize at 640x420 = 268800 pixels: k_fft_chan_partial's 1024 blocks of 256 make a second
    trip.  A kernel normalised to sum 1 keeps each channel's mean: the result's mean equals the input's within
    2**-20 relative (the float store moves it by < 2**-24; a dropped or doubled partial sum by > 1 %)."""
    w, h = 640, 420
    assert w * h > 1024 * 256
    uv = {"normalize": 1, "copy_alpha": 0}
    images = _images("convolve", w, h, seed=11)
    got = _gpu_map("convolve", w, h, uv, images)
    want = R.restated("convolve", uv, images)
    print("fft_distance", ("convolve", w, h, uv), R.fft_distance(got, want))
    R.assert_fft_close(got, want, ("convolve", w, h, uv))
    a = R.as_map(images["in"]).astype(np.float64)
    for c in range(4):
        mean_in, mean_out = a[..., c].mean(), got[..., c].astype(np.float64).mean()
        assert abs(mean_out - mean_in * 1.0) <= 2.0 ** -20 * abs(mean_in), (c, mean_in, mean_out)


@pytest.mark.parametrize("w,h", [(1, 1), (1, 7), (9, 1)])
@pytest.mark.parametrize("name", sorted(R.FLAGS))
def test_width_or_height_one(name, w, h):
    """Frames one pixel wide or high: bytes and float maps equal the oracle's, NaN at the same places.  (The
    rendered input maps are zero at these sizes, so convolve gives zeros, and NaN with normalize: 1/sum is
    infinite.)"""
    images = _images(name, w, h, seed=w * 10 + h)
    for uv in R.FLAGS[name]:
        what = (name, w, h, uv)
        got = _gpu_map(name, w, h, uv, images)
        want = _oracle_map(name, w, h, uv, images)
        assert np.array_equal(np.isnan(got), np.isnan(want)), (what, got, want)
        assert np.array_equal(got, want, equal_nan=True), (what, got, want)
        got8 = _invocation(name, w, h, uv, images).render()
        want8 = R.oracle(name).render(w, h, uservals=uv, images=images)
        assert np.array_equal(got8, want8), (what, got8, want8)


def test_one_invocation_many_renders():
    """One invocation through changes of flags, render size and kernel image: every render equals the render of a
    fresh invocation with the same settings bit for bit (plans, workspace and the native-call memo carry nothing
    over), and is within assert_fft_close of the oracle."""
    w, h = 96, 64
    img, kern, other = R.random_rgba(w, h, 21), R.random_rgba(w, h, 22), R.random_rgba(w, h, 23)
    state = {"uv": {"normalize": 1, "copy_alpha": 1}, "images": {"in": img, "kernel": kern}, "size": None}
    inv = _invocation("convolve", w, h, state["uv"], state["images"])
    maps = []

    def step(what, uv=None, kernel=None, size=None):
        for k, v in (uv or {}).items():
            inv.set(k, v)
            state["uv"][k] = v
        if kernel is not None:
            inv.set_image("kernel", kernel)
            state["images"]["kernel"] = kernel
        if size is not None:
            inv.set_render_size(*size)
            state["size"] = size
        rw, rh = state["size"] or (w, h)
        got = render_device(inv, rw, rh, floatmap=True)
        fresh = _gpu_map("convolve", w, h, state["uv"], state["images"], state["size"])
        assert np.array_equal(got.view(np.uint32), fresh.view(np.uint32)), (what, "differs from a fresh invocation", R.fft_distance(got, fresh))
        R.assert_fft_close(got, _oracle_map("convolve", w, h, state["uv"], state["images"], state["size"]), what)
        maps.append(got)
        return got

    first = step("copy_alpha=1")
    first8 = inv.render()
    assert np.array_equal(inv.render(t=0.5), first8)            # nothing changed: the memo's map, the same bytes
    assert np.array_equal(render_device(inv, w, h, floatmap=True).view(np.uint32), first.view(np.uint32))
    step("copy_alpha=0", uv={"copy_alpha": 0})
    small = step("render size 75x51", size=(75, 51))
    assert small.shape == (51, 75, 4)
    back = step("render size 96x64 again", size=(w, h))
    assert np.array_equal(back.view(np.uint32), maps[1].view(np.uint32))
    before = step("normalize=0", uv={"normalize": 0})
    after = step("another kernel", kernel=other)
    assert not np.array_equal(after, before)
    again = step("the first configuration again", uv={"normalize": 1, "copy_alpha": 1}, kernel=kern)
    assert np.array_equal(again.view(np.uint32), first.view(np.uint32))
    assert np.array_equal(inv.render(), first8)


def test_two_fft_calls_in_one_frame():
    """convolve on 3 channels, then visualize_fft on 4 of the convolved map: the plans are remade in mid-frame, a
    float-map input is taken without a copy, and k_fft_store reads alpha from the rendered input map."""
    w, h = 75, 51
    images = {"in": R.random_rgba(w, h, 31), "kernel": R.random_rgba(w, h, 32)}
    got = _gpu_map(TWO_FFTS, w, h, {}, images)
    want = _oracle_map(TWO_FFTS, w, h, {}, images)
    print("fft_distance", ("two_ffts", w, h), R.fft_distance(got, want))
    R.assert_fft_close(got, want, ("two_ffts", w, h))
    assert np.array_equal(got[..., 3].view(np.uint32), R.as_map(images["in"])[..., 3].view(np.uint32))
    # the same from the restatements: the oracle's memo and float-map hand-over are not common to both sides
    c = R.convolve(R.as_map(images["in"]), R.as_map(images["kernel"]), 1, 1)
    v = R.visualize_fft(c, 0)
    R.assert_fft_close(got, np.stack([v[..., 0], c[..., 1], v[..., 3], c[..., 3]], axis=-1), ("two_ffts restated", w, h))


@pytest.mark.parametrize("name", ["convolve", "half_convolve"])
def test_inputs_of_another_size_than_the_canvas(name):
    """A 120x90 input and a 40x28 kernel or mask on a 75x51 canvas: both are resampled to the canvas (render_image)
    before the transforms."""
    w, h = 75, 51
    images = {"in": R.random_rgba(120, 90, 41), R.SECOND_IMAGE[name]: R.random_rgba(40, 28, 42)}
    for uv in R.FLAGS[name]:
        what = (name, "120x90 and 40x28 on 75x51", uv)
        got = _gpu_map(name, w, h, uv, images)
        want = _oracle_map(name, w, h, uv, images)
        print("fft_distance", what, R.fft_distance(got, want))
        R.assert_fft_close(got, want, what)


def test_rgb_inputs_equal_rgba_with_opaque_alpha():
    """[H,W,3] arrays give, bit for bit, what the same bytes with an explicit alpha plane of 255 give."""
    w, h = 75, 51
    uv = {"normalize": 1, "copy_alpha": 0}
    rgba = {"in": R.random_rgba(w, h, 51), "kernel": R.random_rgba(w, h, 52)}
    for a in rgba.values():
        a[..., 3] = 255
    rgb = {k: np.ascontiguousarray(a[..., :3]) for k, a in rgba.items()}
    got3, got4 = _gpu_map("convolve", w, h, uv, rgb), _gpu_map("convolve", w, h, uv, rgba)
    assert np.array_equal(got3.view(np.uint32), got4.view(np.uint32)), R.fft_distance(got3, got4)
    R.assert_fft_close(got3, _oracle_map("convolve", w, h, uv, rgba), ("convolve", "rgb", w, h))
