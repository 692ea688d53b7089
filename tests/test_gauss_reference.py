"""tests/gauss_reference.py against the CPU oracle: the restatement of gaussian_blur's FIR path written from gauss.c
equals the float maps of the oracle (oracle/mm_oracle_rt.c mmo_gauss_rle) bit for bit on both of its branches, the
oracle's full branch stays within the stated bound of a float64 evaluation, and the input builders give what they
promise.  That pins the helper for tests/test_gpu_gauss_fir.py and shows that two independent float32 transcriptions
of the reference agree to the bit, which is what the HIP kernels are then held to.  No GPU."""
import numpy as np
import pytest

from tests import gauss_reference as G

SIZES = [(1, 1), (1, 7), (9, 1), (2, 2), (5, 3), (16, 16), (17, 33), (64, 48)]
# sigma in pixels (horizontal, vertical): both below 0.5; one below 0.5 and the other 6 or 20 px, a window longer than
# the line at most of the sizes; one deviation 0 (its pass is skipped)
SIGMAS = [(0.3, 0.2), (0.49, 0.45), (0.49, 20.0), (6.0, 0.3), (20.0, 0.4), (0.3, 6.0), (0.0, 0.4), (0.3, 0.0)]


def _oracle_map(src, w, h, hdev, vdev, img):
    return G.oracle(src).render(w, h, uservals={"hdev": hdev, "vdev": vdev}, images={"in": img}, floatmap=True)


def _input_map(src, w, h, img):
    """The oracle's own sigma-0 map: what the blur is handed, through the identity sampling of `soft(xy)`.  For a
    drawable of two or more pixels each way that is the bytes / 255; a frame one pixel wide or high renders zeros."""
    m0 = _oracle_map(src, w, h, 0.0, 0.0, img)
    if src == "gauss_direct":
        if w > 1 and h > 1:
            assert np.array_equal(m0.view(np.uint32), G.as_map(img).view(np.uint32)), (w, h)
        else:
            assert not m0.any(), (w, h)
    return m0


def _inputs(w, h):
    const = np.empty((h, w, 4), np.uint8)
    const[...] = (255, 1, 128, 77)
    return [("random", G.random_rgba(w, h, w * 1000 + h)), ("threshold_rows", G.threshold_rows(w, h)), ("constant", const)]


@pytest.mark.parametrize("w,h", SIZES)
def test_restatement_equals_oracle_bit_for_bit(w, h):
    """Every sigma pair on random RGBA bytes, threshold_rows and a constant image: the oracle's float map equals
    gauss_blur_map of its own sigma-0 map, NaN nowhere, every bit the same."""
    for what, img in _inputs(w, h):
        m0 = _input_map("gauss_direct", w, h, img)
        for hsig, vsig in SIGMAS:
            hdev, vdev = G.devs_for(w, h, hsig, vsig)
            hs, vs = G.sigmas(w, h, hdev, vdev)
            assert G.takes_fir(hs, vs), (w, h, hsig, vsig)
            assert (hs > 0) == (hsig > 0 and w > 1) and (vs > 0) == (vsig > 0 and h > 1), (w, h, hs, vs)
            want = _oracle_map("gauss_direct", w, h, hdev, vdev, img)
            got, flags = G.gauss_blur_map(m0, hs, vs)
            assert not np.isnan(want).any()
            assert G.same_maps(got, want), (what, w, h, hsig, vsig, G.describe_difference(got, want))
            if what == "constant":
                assert all(f.all() for f in flags.values()), (w, h, hsig, vsig)      # the encoded branch on every line


@pytest.mark.parametrize("w,h", [(2, 2), (5, 3), (16, 16), (17, 33), (64, 48)])
def test_oracle_full_branch_within_the_float64_bound(w, h):
    """One pass at a time from the oracle's sigma-0 map of random RGBA bytes (frames one pixel wide or high render
    zeros and have nothing to measure): no line takes the encoded branch, and every element lies within
    f64_bound_units(L) * 2**-24 * max |line| of the float64 evaluation.  Prints the measured distance per case."""
    img = G.random_rgba(w, h, w * 1000 + h)
    m0 = _input_map("gauss_direct", w, h, img)
    for sig in (0.3, 0.49, 6.0, 20.0):
        for axis in (0, 1):
            hdev, vdev = G.devs_for(w, h, sig if axis == 1 else 0.0, sig if axis == 0 else 0.0)
            hs, vs = G.sigmas(w, h, hdev, vdev)
            got = _oracle_map("gauss_direct", w, h, hdev, vdev, img)
            dist, share, length = G.f64_distance(got, m0, vs if axis == 0 else hs, axis)
            print("f64_distance", (w, h), "sigma %g axis %d L %d:" % (sig, axis, length), "%.3f of at most %d," % (dist, G.f64_bound_units(length)),
                  "covered", share)
            assert share == 1.0, (w, h, sig, axis, share)
            assert dist <= G.f64_bound_units(length), (w, h, sig, axis, dist)


def test_rle_curve_types():
    """Lengths, symmetry, float32 storage, and the float32 running sum (which differs from a float64 sum rounded
    once at L = 67)."""
    for sigma, length in ((0.01, 1), (0.2, 1), (0.3, 1), (0.49, 2), (6.0, 20), (20.0, 67)):
        got, taps, csum, total = G.rle_curve(sigma)
        assert got == length and taps.dtype == csum.dtype == np.float32 and isinstance(total, np.float32), sigma
        assert taps.shape == csum.shape == (2 * length + 1,) and taps[length] == 1.0 and csum[0] == 0.0
        assert np.array_equal(taps, taps[::-1]) and (taps[:length] <= taps[1:length + 1]).all()
        run = np.float32(0)
        for i in range(2 * length):
            run = np.float32(run + taps[i])
            assert csum[i + 1] == run
        assert total == csum[2 * length]          # the last tap is not in the sums: gauss.c:295-302
    assert G.rle_curve(0.01)[1].tolist() == [0.0, 1.0, 0.0]
    _, taps, csum, total = G.rle_curve(20.0)
    assert total != np.float32(taps[:-1].astype(np.float64).sum())


@pytest.mark.parametrize("n", [4, 5, 7, 8, 16, 17])
def test_threshold_rows_take_both_branches(n):
    """threshold_rows(n, 8): every row has the `same` count it promises in every channel (counted here from the
    bytes, and by run_length_encode), the restatement's flags put the switch exactly between same == (3n)//4 and one
    more, both branches run, and the oracle agrees to the bit with rows as the lines (vdev = 0)."""
    h = 8
    img = G.threshold_rows(n, h)
    sames = G.threshold_sames(n)
    assert sames == [(3 * n) // 4 - 1, (3 * n) // 4, (3 * n) // 4 + 1, n]
    m = G.as_map(img)
    for r in range(h):
        for c in range(4):
            counted = 1 + int((img[r, :-1, c] == img[r, 1:, c]).sum())
            assert counted == sames[r % 4] == G.run_length_encode(m[r, :, c], 3)[0], (n, r, c)
    for hsig in (0.3, 0.49, 6.0):
        hdev, _ = G.devs_for(n, h, hsig, 0.0)
        hs, vs = G.sigmas(n, h, hdev, 0.0)
        assert vs == 0.0
        got, flags = G.gauss_blur_map(m, hs, vs)
        assert list(flags) == [1]
        for r in range(h):
            assert (flags[1][r] == (sames[r % 4] > (3 * n) // 4)).all(), (n, r)
        assert flags[1][0::4].sum() == 0 and flags[1][1::4].sum() == 0 and flags[1][2::4].all() and flags[1][3::4].all()
        want = _oracle_map("gauss_direct", n, h, hdev, 0.0, img)
        assert G.same_maps(got, want), (n, hsig, G.describe_difference(got, want))


def test_encoded_branch_keeps_the_reference_truncation():
    """A constant line comes out as value * total / (int)total on the encoded branch (1.0039 at L = 1, 1.073 at
    L = 10): gauss.c's int-typed sums, not an error of the restatement."""
    m = np.full((1, 12, 4), 0.5, np.float32)
    for sigma in (0.3, 3.0):
        length, _, _, total = G.rle_curve(sigma)
        out, flags = G.fir_pass_f32(m, sigma, 1)
        assert flags.all()
        assert np.array_equal(out, np.full_like(m, np.float32(np.float32(0.5) * total) / np.float32(int(total)))), (sigma, out[0, 0])
        assert out[0, 0, 0] > 0.5
    _, covered, _ = G.fir_pass_f64(m, 0.3, 1)
    assert not covered.any()


def test_stepped_flat_takes_the_encoded_branch():
    """stepped_flat: every line of the first pass is on the encoded branch, and lines of the second (which reads the
    first one's output, smeared at the steps) are too where the first was narrow; the oracle agrees to the bit."""
    for w, h in ((16, 16), (17, 33), (64, 48)):
        img = G.stepped_flat(w, h)
        assert len(np.unique(img.reshape(-1, 4), axis=0)) == 3
        for hsig, vsig in ((0.3, 0.2), (0.49, 20.0), (23.0, 0.3)):
            hdev, vdev = G.devs_for(w, h, hsig, vsig)
            got, flags = G.gauss_blur_map(G.as_map(img), *G.sigmas(w, h, hdev, vdev))
            assert flags[0].all() and (vsig > 0.5 or flags[1].mean() >= 0.5), (w, h, hsig, vsig, flags[0].mean(), flags[1].mean())
            assert G.same_maps(got, _oracle_map("gauss_direct", w, h, hdev, vdev, img)), (w, h, hsig, vsig)


def test_runs_of_mixed_zeros():
    """run_length_encode writes the run's value, taken at the line's far end, over every element of the run: where
    -0 precedes +0 the padded line holds +0.  Both branches read the padded line (gauss.c:552-559).  The result cannot
    show it: every sum starts at +0.0, every weight is >= 0 and +0 + -0 = +0, so a line of zeros of either sign
    comes out +0 whichever sign each product had."""
    line = np.array([-0.0, 0.0, -0.0, -0.0, 0.0, 0.0, -0.0, 1.0], np.float32)
    same, pix, rle = G.run_length_encode(line, 2)
    assert same == 7                       # the last element counts itself, six zeros repeat their successor
    assert np.signbit(pix[:9]).all() and pix[9] == pix[10] == pix[11] == 1.0     # the far end of the zero run is -0
    assert rle[:9] == [9, 8, 7, 6, 5, 4, 3, 2, 1]
    for zeros in (np.array([0.0, -0.0] * 6, np.float32), np.array([-0.0, 0.0] * 6, np.float32), np.full(12, -0.0, np.float32)):
        m = np.repeat(zeros[None, :, None], 4, axis=2)
        for sigma in (0.3, 3.0):
            out, flags = G.fir_pass_f32(m, sigma, 1)
            assert flags.all() and not out.any() and not np.signbit(out).any()
        mixed = m.copy()
        mixed[0, :7:2, :] = np.float32(1e-40) * np.arange(1, 5, dtype=np.float32)[:, None]      # below 3/4: the full branch
        out, flags = G.fir_pass_f32(mixed, 0.3, 1)
        assert not flags.any() and not np.signbit(out).any()


@pytest.mark.parametrize("hsig,vsig", [(0.3, 0.4), (0.3, 3.0)])
def test_special_values_through_the_oracle(hsig, vsig):
    """SPECIAL_CLOSURE at 40 x 24: the closure's map holds +inf, -inf, NaN, a channel of -0, rows of mixed zeros and
    denormals; the oracle's FIR result has its NaN where the restatement has them and equals it bit for bit everywhere
    else.  inf and NaN stay local, denormals come out as denormals, the -0 channel comes out +0, and both branches
    run on a float map."""
    w, h = 40, 24
    img = G.random_rgba(w, h, 7)
    m0 = _input_map(G.SPECIAL_CLOSURE, w, h, img)
    census = G.special_census(m0)
    assert census["+inf"][0] and census["-inf"][0] and census["nan"][1] and census["-0"][3] == w * h, census
    assert not (census["+inf"][2] or census["-inf"][2] or census["nan"][2]), census
    assert census["-0"][2] and census["+0"][2] and census["denormal"][2] > 100, census
    assert np.abs(m0[..., 2]).max() > 2.5 and m0[..., 0][np.isfinite(m0[..., 0])].min() < -0.9, census
    zero_rows = [r for r in range(h) if not m0[r, :, 2].any()]
    assert zero_rows and all(np.signbit(m0[r, :, 2]).any() and not np.signbit(m0[r, :, 2]).all() for r in zero_rows)
    hdev, vdev = G.devs_for(w, h, hsig, vsig)
    hs, vs = G.sigmas(w, h, hdev, vdev)
    assert G.takes_fir(hs, vs)
    want = _oracle_map(G.SPECIAL_CLOSURE, w, h, hdev, vdev, img)
    got, flags = G.gauss_blur_map(m0, hs, vs)
    assert np.array_equal(np.isnan(got), np.isnan(want)), G.describe_difference(got, want)
    assert G.same_maps(got, want), G.describe_difference(got, want)
    assert all(f.any() and not f.all() for f in flags.values())
    out = G.special_census(want)
    assert 0 < out["nan"][1] < w * h and 0 < out["+inf"][0] + out["-inf"][0] < w * h and out["nan"][2] == 0, out
    assert out["denormal"][2] > 100 and out["+0"][3] == w * h and out["-0"][3] == 0, out

