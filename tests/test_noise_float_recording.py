"""The recording tests/golden/noise_float/ is what the oracle, with the reference's libnoise, renders now."""
import os

import numpy as np
import pytest

import mathmap_amd as mm
from oracle.ccgen import NOISE_LIB
from tests import noise_probes as N


def test_probes_reach_the_noise_builtins():
    assert N.IDS["full"] <= mm.Filter(N.FULL).builtin_ids
    assert N.IDS["simple"] <= mm.Filter(N.SIMPLE).builtin_ids
    for ident, expr in (("noise_perlin_full", "noise(oct, per, lac, p)"), ("noise_perlin_simple", "noise(p)")):
        assert expr in (N.FULL if "full" in ident else N.SIMPLE)


def test_cases_cover_every_parameter_value_and_edge():
    cs = N.cases()
    full = [c[2] for c in cs if c[1] == "full"]
    assert {v[4] for v in full} == set(N.OCTAVES) and {v[5] for v in full} == set(N.PERSISTENCE) and {v[6] for v in full} == set(N.LACUNARITY)
    assert {(v[4], v[6]) for v in full} == {(o, l) for o in N.OCTAVES for l in N.LACUNARITY}
    assert all(1 <= v[4] <= 30 for _, _, v in cs)          # libnoise throws outside
    for edge in (1.0, 255.0, 256.0, 2.0 ** 24, 2.0 ** 30, 2.0 ** 31, 3e9, 1e12):
        assert any(abs(v[1]) - v[0] <= edge <= abs(v[1]) + v[0] for v in full), edge
    assert sum(os.path.getsize(os.path.join(N.GOLDEN, f)) for f in os.listdir(N.GOLDEN)) < 4 << 20
    assert all(os.path.getsize(os.path.join(N.GOLDEN, f)) < 1 << 20 for f in os.listdir(N.GOLDEN))


def test_recording_equals_a_live_oracle_render():
    if not os.path.exists(NOISE_LIB):
        pytest.skip("the oracle's noise library (oracle/_ref/libmmnoise.so) is not built here")
    from tests.make_noise_float import live
    rec, now = N.recorded(), live()
    assert set(rec) == set(now)
    for name in sorted(rec):
        assert N.differing(now[name], rec[name]) == (0, True), name
    # the edges are in the frames: NaN where a coordinate overflowed, and finite values elsewhere
    assert np.isnan(rec["full_1e30_o30_l1e+10"][..., :3]).all()
    assert np.isfinite(rec["full_p31_frac"]).all()
