"""gaussian_blur's recursive path (native_filters.hip: k_iir_causal, k_iir_anticausal_T, their _clip twins, the segment
plans) against the float64 restatement of tests/gauss_iir_reference.py, written from gauss.c and pinned against the
oracle by tests/test_gauss_iir_reference.py.  One rule everywhere but the tolerance chain (gauss_reference.same_maps):
NaN at the same places, every other element the same bits.

Frames (gauss_iir_reference.FRAMES): lines of 2 and 4 steps (both sweeps' edge steps in one block), around one block and
one workgroup, the line lengths at which the anticausal sweep's all-fast groups start at each residue of its groups of
three blocks (128/129, 144/145, 160/161) and at which the causal sweep's first and second group of four become all-fast
(176/177, 240/241).  Deviations: the 0.5 px switch, below a pixel on one axis, far longer than the line.  Sources:
a drawable (DrawableSrc, then FiniteMapSrc) and a closure's float map (MapSrc twice).  Modes: whole frames, row windows
cut off by the frame's ends, forced segment counts at small frames, the clip kernels, the tolerance chain."""
import ctypes as C

import numpy as np
import pytest

from mathmap_amd._lib import lib, selftest_lib
from tests import clip_native_probes as N
from tests import filters as F
from tests import gauss_iir_reference as R
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
    return render_device(_invocation(src, w, h, uv, img), w, h, rows=rows, floatmap=True)


def _oracle_map(src, w, h, uv, img):
    return G.oracle(src).render(w, h, uservals=uv, images={"in": img}, floatmap=True)


def _case(w, h, hsig, vsig):
    """(user values, hs, vs) of a case given in pixels; the recursive path."""
    hdev, vdev = R.devs_at_least(w, h, hsig, vsig)
    hs, vs = G.sigmas(w, h, hdev, vdev)
    assert not G.takes_fir(hs, vs), (w, h, hs, vs)
    return {"hdev": hdev, "vdev": vdev}, hs, vs


def _assert_same(got, want, what):
    assert G.same_maps(got, want), (what, G.describe_difference(got, want))


def _id(*c):
    return "%dx%d_s%g_%g" % c[:4] + "".join("_%s" % v for v in c[4:])


DRAWABLE_CASES = [(w, h, hsig, vsig) for w, h in R.FRAMES for hsig, vsig in R.SIGMA_PAIRS]


@pytest.mark.parametrize("w,h,hsig,vsig", DRAWABLE_CASES, ids=[_id(*c) for c in DRAWABLE_CASES])
def test_exact_chain_on_a_drawable(w, h, hsig, vsig):
    """gauss_direct on random RGBA bytes: the float map equals iir_blur of the bytes / 255, and the oracle's."""
    img = G.random_rgba(w, h, R.case_seed(w, h))
    uv, hs, vs = _case(w, h, hsig, vsig)
    got = _gpu_map("gauss_direct", w, h, uv, img)
    _assert_same(got, R.iir_blur(G.as_map(img), hs, vs), ("restatement", w, h, hsig, vsig))
    _assert_same(got, _oracle_map("gauss_direct", w, h, uv, img), ("oracle", w, h, hsig, vsig))


MAP_CASES = [(w, h, hsig, vsig) for w, h in R.MAP_FRAMES for hsig, vsig in R.MAP_SIGMA_PAIRS]


@pytest.mark.parametrize("w,h,hsig,vsig", MAP_CASES, ids=[_id(*c) for c in MAP_CASES])
def test_exact_chain_on_a_float_map(w, h, hsig, vsig):
    """SPECIAL_CLOSURE: both passes read a plain float map (MapSrc: it may hold -0, and is not known finite).  The
    input is the closure's own map as the oracle renders it at deviation 0 (tests/test_gpu_gauss_fir.py shows the GPU
    delivers that map).  Blue (mixed zeros, denormals, values in [-3, 0]) and alpha (-0 throughout) equal the
    restatement bit for bit; red (inf) and green (NaN) are NaN throughout."""
    img = G.random_rgba(w, h, 7)
    uv, hs, vs = _case(w, h, hsig, vsig)
    m0 = _oracle_map(G.SPECIAL_CLOSURE, w, h, {"hdev": 0.0, "vdev": 0.0}, img)
    want = R.iir_blur(m0, hs, vs)
    got = _gpu_map(G.SPECIAL_CLOSURE, w, h, uv, img)
    for side in (got, want):
        assert np.isnan(side[..., :2]).all() and not np.isnan(side[..., 2:]).any(), (w, h, hsig, vsig)
    assert G.same_maps(got[..., 2:], want[..., 2:]), (w, h, hsig, vsig, G.describe_difference(got, want))
    assert want[..., 2].any()


@pytest.mark.parametrize("w,h,hsig,vsig", R.ROW_WINDOW_CASES, ids=[_id(*c) for c in R.ROW_WINDOW_CASES])
def test_row_windows_cut_off_by_the_frame(w, h, hsig, vsig):
    """Native row margin 0 and three bands: every band's blur covers its rows and a halo of 22.7 sigma + 2 rows, which
    the frame's top cuts off for the first band, its bottom for the last, and at the smaller frame both for the middle
    one.  The assembled map equals the whole-frame restatement bit for bit
    (test_gauss_row_stripes_with_local_halo_equal_full_frame's claim, at 640 x 1500 against the GPU's own frame)."""
    img = G.random_rgba(w, h, R.case_seed(w, h))
    uv, hs, vs = _case(w, h, hsig, vsig)
    inv = _invocation("gauss_direct", w, h, uv, img)
    inv.set_native_row_margin(0)
    bands = [(0, h // 3), (h // 3, 2 * h // 3), (2 * h // 3, h)]
    got = render_device(inv, w, h, rows=bands, floatmap=True)
    _assert_same(got, R.iir_blur(G.as_map(img), hs, vs), ("bands", w, h, bands))


def _segment_id(k, forced):
    said = ["%s%s" % (p, "-whole-line" if c == 1 else c) for p, c in zip("vh", R.SEGMENT_COUNTS[forced][k])]
    return _id(*R.SEGMENT_CASES[k]) + "_forced%s_%s_%s" % (forced, said[0], said[1])


SEGMENT_PARAMS = [(k, forced) for k in range(len(R.SEGMENT_CASES)) for forced in R.FORCED_SEGMENTS]


@pytest.mark.parametrize("k,forced", SEGMENT_PARAMS, ids=[_segment_id(*p) for p in SEGMENT_PARAMS])
def test_forced_segments(k, forced, monkeypatch):
    """MMHIP_GAUSS_SEGMENTS = 2, 3, 5 at small frames: the segment code (a sweep that starts inside the line, the
    warm-up branch of the anticausal sweep, checkpoints per segment) with the plan gaussian_blur reports for each pass
    (mmhip_selftest_gauss_line_plan).  A pass whose forced count the model refused runs whole lines (the id says which)
    and is restated by iir_pass; the others by iir_pass_segmented with the reported segment and halo.  Bit for bit."""
    w, h, hsig, vsig = R.SEGMENT_CASES[k]
    monkeypatch.setenv("MMHIP_GAUSS_SEGMENTS", forced)
    img = G.random_rgba(w, h, R.case_seed(w, h))
    uv, hs, vs = _case(w, h, hsig, vsig)
    pv, ph = R.frame_plans(w, h, hs, vs)
    assert (pv[2], ph[2]) == R.SEGMENT_COUNTS[forced][k], (pv, ph)
    assert sum(1 for cv, ch in R.SEGMENT_COUNTS[forced] if cv > 1 or ch > 1) >= 2
    got = _gpu_map("gauss_direct", w, h, uv, img)
    _assert_same(got, R.iir_blur_planned(G.as_map(img), hs, vs, pv, ph), ("segmented", w, h, forced, pv, ph))


def _clip_maps(inv, w, h, frames, ts):
    """render_clip's float maps, [N,h,w,4]."""
    n = len(frames)
    dev = lib().mmhip_device_alloc(n * w * h * 16)
    assert dev
    try:
        inv.render_clip(frames=frames, ts=ts, out_ptr=dev, floatmap=True)
        inv.sync()
        out = np.empty((n, h, w, 4), np.float32)
        assert lib().mmhip_copy_to_host(out.ctypes.data_as(C.c_void_p), C.c_void_p(dev), out.nbytes) == 0
    finally:
        lib().mmhip_device_free(C.c_void_p(dev))
    return out


CLIP_TS = [0.0, 0.5, 0.75]


@pytest.mark.parametrize("name", ["direct_t", "chain"])
@pytest.mark.parametrize("w,h", R.CLIP_FRAMES, ids=["%dx%d" % f for f in R.CLIP_FRAMES])
def test_clip_kernels(w, h, name):
    """k_iir_causal_clip / k_iir_anticausal_T_clip (another code shape of the same sweeps): three frames of DIRECT_T (a
    drawable source) and of CHAIN (the second blur reads the first one's map) in one batch, every frame against the
    restatement.  s is the smallest value that gives half a pixel on both axes at t = 0; the deviations follow t in
    float, in the filter's own order."""
    src = N.DIRECT_T if name == "direct_t" else N.CHAIN
    img = G.random_rgba(w, h, R.case_seed(w, h))
    s = np.float32(max(R.devs_at_least(w, h, 0.5, 0.5)))
    inv = _invocation(src, w, h, {"s": float(s)}, img)
    got = _clip_maps(inv, w, h, [0, 1, 2], CLIP_TS)
    assert inv.clip_native_batches() >= 1
    one, two = np.float32(1), np.float32(2)
    for i, t in enumerate(np.float32(CLIP_TS)):
        a, b = np.float32(s * np.float32(one + t)), np.float32(s * np.float32(one + np.float32(two * t)))
        if name == "direct_t":
            blurs = [(a, b)]
        else:
            blurs = [(a, s), (s, b)]
        want = G.as_map(img)
        for hdev, vdev in blurs:
            hs, vs = G.sigmas(w, h, hdev, vdev)
            assert not G.takes_fir(hs, vs), (w, h, t, hs, vs)
            want = R.iir_blur(want, hs, vs)
        _assert_same(got[i], want, (name, w, h, "frame %d" % i, float(t)))
    assert not np.array_equal(got[0], got[1])


@pytest.mark.parametrize("w,h,hsig,vsig", R.TOLERANCE_CASES, ids=[_id(*c) for c in R.TOLERANCE_CASES])
def test_tolerance_chain_against_the_restatement(w, h, hsig, vsig):
    """The tolerance chain's float map (fused steps, always split by its own plan) against iir_blur -- the reference,
    not the GPU's exact chain -- within the 2.5e-7 absolute tests/test_gpu_gauss_tolerance.py holds it to against the
    exact one.  Prints the largest distance."""
    img = np.ascontiguousarray(G.random_rgba(w, h, R.case_seed(w, h))[..., :3])
    uv, hs, vs = _case(w, h, hsig, vsig)
    tol = np.empty((h, w, 4), np.float32)
    st = selftest_lib()
    rc = st.mmhip_selftest_gauss_tolerance_map(img.ctypes.data_as(C.c_void_p), w, h, uv["hdev"], uv["vdev"], tol.ctypes.data_as(C.c_void_p))
    assert rc == 0, st.mmhip_selftest_error()
    want = R.iir_blur(G.as_map(img), hs, vs)
    err = np.abs(tol.astype(np.float64) - want.astype(np.float64))
    print("%dx%d sigma %g/%g, plans %s: max |tolerance chain - restatement| = %.3g, %d of %d values differ"
          % (w, h, hsig, vsig, R.frame_plans(w, h, hs, vs, tolerance=True), err.max(), np.count_nonzero(err), err.size))
    assert np.isfinite(tol).all() and err.max() <= R.TOLERANCE_BOUND, err.max()
