"""tests/gauss_iir_reference.py against the CPU oracle and on its own: the restatement of gaussian_blur's recursive path
written from gauss.c equals the float maps of the oracle (oracle/mm_oracle_rt.c mmo_gauss_iir) bit for bit -- two
independent transcriptions of the reference agree, which is what the scan kernels are then held to by
tests/test_gpu_gauss_iir.py --, it is a Gaussian blur (impulse response, sum, second moment, a constant line), and its
segmented form stays within the rule of MMHIP_GAUSS_SEGMENTS on the inputs the GPU test uses.  No GPU."""
import numpy as np
import pytest

from tests import gauss_iir_reference as R
from tests import gauss_reference as G


def _oracle_map(src, w, h, hdev, vdev, img):
    return G.oracle(src).render(w, h, uservals={"hdev": hdev, "vdev": vdev}, images={"in": img}, floatmap=True)


@pytest.mark.parametrize("w,h", R.FRAMES, ids=["%dx%d" % f for f in R.FRAMES])
def test_restatement_equals_oracle_bit_for_bit(w, h):
    """Every sigma pair on random RGBA bytes: the oracle's float map of gauss_direct equals iir_blur of the bytes / 255."""
    img = G.random_rgba(w, h, R.case_seed(w, h))
    for hsig, vsig in R.SIGMA_PAIRS:
        hdev, vdev = R.devs_at_least(w, h, hsig, vsig)
        hs, vs = G.sigmas(w, h, hdev, vdev)
        assert not G.takes_fir(hs, vs) and float(hs) >= hsig and float(vs) >= vsig, (w, h, hs, vs)
        assert float(hs) < hsig * 1.00001 and float(vs) < vsig * 1.00001, (w, h, hs, vs)
        want = _oracle_map("gauss_direct", w, h, hdev, vdev, img)
        got = R.iir_blur(G.as_map(img), hs, vs)
        assert not np.isnan(want).any()
        assert G.same_maps(got, want), (w, h, hsig, vsig, G.describe_difference(got, want))


@pytest.mark.parametrize("w,h", R.MAP_FRAMES, ids=["%dx%d" % f for f in R.MAP_FRAMES])
def test_float_map_input_equals_oracle(w, h):
    """SPECIAL_CLOSURE: the oracle's map at deviation 0 (inf in red, NaN in green, mixed zeros, denormals and values
    in [-3, 0] in blue, -0 in alpha -- no k / 255) as the input.  Red and green come out NaN throughout on both sides;
    blue and alpha equal the restatement bit for bit."""
    img = G.random_rgba(w, h, 7)
    m0 = _oracle_map(G.SPECIAL_CLOSURE, w, h, 0.0, 0.0, img)
    census = G.special_census(m0)
    assert census["+inf"][0] and census["nan"][1] and census["-0"][3] == w * h and census["-0"][2] and census["+0"][2], census
    assert np.isfinite(m0[..., 2:]).all() and not np.array_equal(np.round(m0[..., 2] * 255) / 255, m0[..., 2])
    for hsig, vsig in R.MAP_SIGMA_PAIRS:
        hdev, vdev = R.devs_at_least(w, h, hsig, vsig)
        hs, vs = G.sigmas(w, h, hdev, vdev)
        assert not G.takes_fir(hs, vs)
        want = _oracle_map(G.SPECIAL_CLOSURE, w, h, hdev, vdev, img)
        got = R.iir_blur(m0, hs, vs)
        for side in (got, want):
            assert np.isnan(side[..., :2]).all() and not np.isnan(side[..., 2:]).any(), (w, h, hsig, vsig)
        assert G.same_maps(got[..., 2:], want[..., 2:]), (w, h, hsig, vsig, G.describe_difference(got, want))
        assert want[..., 2].any() and not want[..., 3].any() and not np.signbit(want[..., 3]).any()


# What the restatement gives on one line of 40 sigma + 41 steps, measured here (x86-64, glibc), per sigma:
#   the response to a centred unit impulse against true_gaussian_line, max |difference| / peak;
#   |sum of the response - 1|;  |second-moment sigma of the response / sigma - 1|;
#   max |output - 0.7| on a constant line of (float)0.7.
# The recursion is a 4th-order fit to the Gaussian (gauss.c:52-54), not an identity: these are its own errors, and at
# 0.5 px, where the fit is poorest, they reach 1.5 % (impulse), 1.5 % (sum) and 7.4 % (sigma).  Every bound below is
# twice the measured value; the margin only guards against libm differences between hosts.
MEASURED = {
    0.5: (1.438380e-02, 1.469783e-02, 7.351349e-02, 1.028848e-02),
    0.75: (1.361976e-04, 1.049742e-04, 2.440051e-03, 7.349253e-05),
    1.0: (3.085862e-04, 2.129429e-04, 2.174467e-03, 1.490712e-04),
    2.0: (3.085829e-04, 1.445108e-04, 2.212906e-03, 1.011491e-04),
    5.0: (5.979641e-04, 2.473865e-04, 2.261589e-03, 1.731515e-04),
    20.0: (7.567627e-04, 2.857947e-04, 2.280794e-03, 2.000332e-04),
    60.0: (7.622669e-04, 2.883117e-04, 2.282049e-03, 2.018213e-04),
}


@pytest.mark.parametrize("sigma", R.PROPERTY_SIGMAS)
def test_restatement_is_a_gaussian_blur(sigma):
    """The restatement alone, so that agreeing with the oracle is not all it is known by."""
    n = int(40 * sigma + 41)
    centre = n // 2
    impulse = np.zeros((1, n, 4), np.float32)
    impulse[0, centre, :] = 1.0
    out = R.iir_pass(impulse, 1, sigma)
    assert all(np.array_equal(out[..., 0], out[..., c]) for c in range(1, 4))
    resp = out[0, :, 0].astype(np.float64)
    true = R.true_gaussian_line(n, centre, sigma)
    k = np.arange(n) - centre
    total = resp.sum()
    mean = (resp * k).sum() / total
    moment = np.sqrt((resp * k * k).sum() / total - mean ** 2)
    const = R.iir_pass(np.full((1, n, 4), 0.7, np.float32), 1, sigma)[0, :, 0].astype(np.float64)
    got = (np.abs(resp - true).max() / true.max(), abs(total - 1.0), abs(moment / sigma - 1.0), np.abs(const - float(np.float32(0.7))).max())
    print("sigma %g, n %d: impulse error / peak %.6e, |sum - 1| %.6e, |moment sigma / sigma - 1| %.6e, constant line off by %.6e" % ((sigma, n) + got))
    assert abs(mean) < 1e-3 * max(sigma, 1.0), mean               # the response is centred
    for what, value, measured in zip(("impulse", "sum", "moment sigma", "constant"), got, MEASURED[sigma]):
        assert value <= 2 * measured, (sigma, what, value, measured)
    if sigma >= 0.75:       # from 0.75 px on the fit holds to these round figures
        assert got[0] < 1e-3 and got[1] < 3e-4 and got[2] < 5e-3 and got[3] < 3e-4, (sigma, got)


@pytest.mark.parametrize("w,h", [(4, 17), (33, 48), (65, 63)])
def test_segments_that_see_the_whole_line_change_nothing(w, h):
    """One segment, or a halo that reaches both ends of the line from every segment: iir_pass itself."""
    m = G.as_map(G.random_rgba(w, h, R.case_seed(w, h)))
    for axis, n in ((0, h), (1, w)):
        for sigma in (0.5, 3.0):
            whole = R.iir_pass(m, axis, sigma)
            for seg, halo in ((n, 0), (n + 7, 16), (16, n), (16, n + 16), (5, 4 * n), (1, n)):
                assert G.same_maps(R.iir_pass_segmented(m, axis, sigma, seg, halo), whole), (w, h, axis, sigma, seg, halo)
    if h > 16:      # and without a halo a second segment shows
        assert not G.same_maps(R.iir_pass_segmented(m, 0, 3.0, 16, 0), R.iir_pass(m, 0, 3.0))


def forced_plans(monkeypatch, forced):
    """{case: (vertical plan, horizontal plan)} of SEGMENT_CASES under MMHIP_GAUSS_SEGMENTS = forced."""
    monkeypatch.setenv("MMHIP_GAUSS_SEGMENTS", forced)
    plans = {}
    for w, h, hsig, vsig in R.SEGMENT_CASES:
        hs, vs = G.sigmas(w, h, *R.devs_at_least(w, h, hsig, vsig))
        plans[(w, h, hsig, vsig)] = R.frame_plans(w, h, hs, vs)
    return plans


@pytest.mark.parametrize("forced", R.FORCED_SEGMENTS)
def test_segmented_restatement_stays_within_the_rule_of_the_mode(forced, monkeypatch):
    """The forced-segment cases of tests/test_gpu_gauss_iir.py, with the plans gaussian_blur makes for them: the
    segmented restatement differs from the whole-line one by at most 1 float32 ulp on at most max(2, 1e-5 * size)
    values, pass by pass and over both passes -- the rule test_gauss_iir_float_map_is_bit_exact holds the mode to.  A
    condition on the chosen inputs: the GPU test's zero tolerance against the segmented restatement then hides no drift
    of the mode itself.  The model refuses some forced counts (segments shorter than the halo, an empty last segment):
    at least two of the three frames split at least one pass under every forced value."""
    plans = forced_plans(monkeypatch, forced)
    assert [(pv[2], ph[2]) for pv, ph in plans.values()] == R.SEGMENT_COUNTS[forced], plans
    split = 0
    for (w, h, hsig, vsig), (pv, ph) in plans.items():
        for (seg, halo, count), n in ((pv, h), (ph, w)):
            assert count == -(-n // seg) and seg % R.IIR_BLOCK == 0 and halo % R.IIR_BLOCK == 0 and (count == 1 or halo >= R.IIR_BLOCK), (w, h, pv, ph)
            assert count in (1, int(forced)), (w, h, pv, ph)
        split += pv[2] > 1 or ph[2] > 1
        hs, vs = G.sigmas(w, h, *R.devs_at_least(w, h, hsig, vsig))
        m = G.as_map(G.random_rgba(w, h, R.case_seed(w, h)))
        first = R.iir_pass(m, 0, vs)
        pairs = [("vertical", R.iir_pass_segmented(m, 0, vs, pv[0], pv[1]), first),
                 ("horizontal", R.iir_pass_segmented(first, 1, hs, ph[0], ph[1]), R.iir_pass(first, 1, hs)),
                 ("both", R.iir_blur_planned(m, hs, vs, pv, ph), R.iir_blur(m, hs, vs))]
        for what, got, want in pairs:
            ulps, differing = R.ulp_distance(got, want)
            print("%dx%d sigma %g/%g forced %s, plans %s %s, %s: %d values differ, by at most %d ulp" % (w, h, hsig, vsig, forced, pv, ph, what, differing, ulps))
            assert ulps <= 1 and differing <= max(2, 1e-5 * got.size), (w, h, forced, what, ulps, differing)
    assert split >= 2, plans


def test_unforced_plan_is_one_segment(monkeypatch):
    """Without MMHIP_GAUSS_SEGMENTS every pass of the exact chain is one segment without a halo."""
    monkeypatch.delenv("MMHIP_GAUSS_SEGMENTS", raising=False)
    for w, h in R.FRAMES:
        for plan, n in zip(R.frame_plans(w, h, 3.0, 0.5), (h, w)):
            assert plan == (-(-n // R.IIR_BLOCK) * R.IIR_BLOCK, 0, 1), (w, h, plan)
