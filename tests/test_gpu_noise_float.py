"""The noise builtins on the GPU, float for float, against the reference's libnoise (the recording of tests/noise_probes.py):
lattice points and their negative side, coordinates at 2^24, 2^30, 2^31, 3e9 and 1e12, 1 to 30 octaves, lacunarity 0, odd,
negative and 1e10.  The bar is the one libnoise meets against itself: no differing value, NaN in the same places."""
import numpy as np
import pytest

import mathmap_amd as mm
from tests import noise_probes as N
from tests.gpu_util import render_device

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def recorded():
    return N.recorded()


@pytest.fixture(scope="module")
def filters():
    return {"full": mm.Filter(N.FULL), "simple": mm.Filter(N.SIMPLE)}


def gpu_map(flt, values):
    inv = flt.invoke(N.SIZE, N.SIZE)
    for k, v in N.uservals(values).items():
        inv.set(k, v)
    return render_device(inv, N.SIZE, N.SIZE, floatmap=True)


@pytest.mark.parametrize("kind", ["full", "simple"])
def test_noise_equals_libnoise_float_for_float(kind, recorded, filters):
    bad = []
    for name, k, values in N.cases():
        if k != kind:
            continue
        got = gpu_map(filters[kind], values)
        want = recorded[name]
        if kind == "simple":
            assert N.differing(got[..., 1:], np.repeat(got[..., :1], 3, axis=-1)) == (0, True)
            got = np.ascontiguousarray(got[..., 0])
        if kind == "full":
            per_channel = [N.differing(np.ascontiguousarray(got[..., c]), np.ascontiguousarray(want[..., c])) for c in range(4)]
            print(name, "perlin billow ridged voronoi:", per_channel)
        n, nan_ok = N.differing(got, want)
        if n or not nan_ok:
            bad.append((name, n, nan_ok))
    assert not bad, bad


def test_specialised_kernel_gives_the_same_floats(recorded):
    """user values baked in as literals: the octave count becomes a constant trip count"""
    names = ("full_unit_frac", "full_p31_int", "full_unit_frac_o30_p0_l3.1")
    generic = mm.Filter(N.FULL)
    found = []
    for name, kind, values in N.cases():
        if name in names:
            flt = generic.specialized(N.uservals(values))
            assert "USERVAL_FLOAT_ACCESS" not in flt.ir_json
            assert N.differing(gpu_map(flt, values), recorded[name]) == (0, True), name
            found.append(name)
    assert sorted(found) == sorted(names)
