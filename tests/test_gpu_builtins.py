"""Every probe of tests/builtin_probes.py on the GPU, in float-map mode, for every user-value set: the generic kernel, the
kernel in pair mode where the generator takes the filter, and the variant specialised for that set (Filter.specialized: the
values baked in as literals), against the oracle (bit for bit, NaN in the same places; the restated GSL functions within
the ulps and the share of identical values of test_gsl_operators_match_restatement) and against the NumPy restatement of
tests/builtin_reference.py under the bound tests/test_builtin_reference.py holds the oracle to.  The specialised variant
is also held, bit for bit, to the oracle's evaluation of its own IR, which prints the literals independently; in the two
sets of INEXACT_FOLD_SETS to that alone (the reason stands there)."""
import numpy as np
import pytest

import mathmap_amd as mm
from oracle.ccgen import CpuFilter
from tests import builtin_probes as P
from tests import builtin_reference as R
from tests.gpu_util import float_ulps, render_device

pytestmark = pytest.mark.gpu


def render(flt, values, images):
    inv = flt.invoke(P.SIZE, P.SIZE)
    for k, v in P.uservals(values).items():
        inv.set(k, v)
    for k, v in images.items():
        inv.set_image(k, v)
    return render_device(inv, P.SIZE, P.SIZE, floatmap=True)


def check_against_oracle(ident, got, want, where):
    if ident in R.GSL_ULPS:
        ulps = float_ulps(got, want)
        print("%s %s: GPU vs oracle max %d ulps, %.5f identical" % (ident, where, int(ulps.max()) if ulps.size else 0,
                                                                     float((ulps == 0).mean()) if ulps.size else 1.0))
        if ulps.size:
            assert ulps.max() <= R.GSL_ULPS[ident] and (ulps == 0).mean() > 0.98, (ident, where, int(ulps.max()), float((ulps == 0).mean()))
    else:
        bad = P.same_bits(got, want)
        print("%s %s: GPU vs oracle %d values differ" % (ident, where, bad))
        assert bad == 0, (ident, where, bad)


@pytest.mark.parametrize("ident", [p.id for p in P.PROBES])
def test_probe_on_the_gpu(ident, monkeypatch):
    probe = P.BY_ID[ident]
    images = {"in": P.probe_image()} if probe.image else {}
    for text, idx in probe.texts():
        monkeypatch.delenv("MMHIP_PAIR", raising=False)
        generic = mm.Filter(text)
        assert ident in generic.builtin_ids
        monkeypatch.setenv("MMHIP_PAIR", "1")
        paired = mm.Filter(text)
        monkeypatch.delenv("MMHIP_PAIR", raising=False)
        variants = [("generic", generic)]
        if "mm_p += 2)" in paired.kernel_source:
            variants.append(("pair", paired))
        cf = CpuFilter(generic.ir_json_raw)
        frames = []
        for name, values in probe.sets.items():
            uv = P.uservals(values)
            want = cf.render(P.SIZE, P.SIZE, uservals=uv, images=images, floatmap=True)
            ref = None
            if ident not in R.SAME_AS:
                ref = np.stack([P.expected(probe, values)[i] for i in idx], axis=-1)
            for label, flt in variants:
                got = render(flt, values, images)
                check_against_oracle(ident, got, want, "%s %s %s" % (label, name, idx))
                if ref is not None:
                    P.compare(ident, got, ref, "%s %s %s" % (label, name, idx), P.magnitude_of(probe, values, idx))
                if label == "generic":
                    frames.append(got)
            # the variant with this set's values as literals: no user value is read at run time
            special = generic.specialized(uv)
            assert "USERVAL_FLOAT_ACCESS" not in special.ir_json, (ident, name)
            if probe.args:
                assert "USERVAL_FLOAT_ACCESS" in generic.ir_json and special.kernel_source != generic.kernel_source, (ident, name)
            got = render(special, values, images)
            own = CpuFilter(special.ir_json).render(P.SIZE, P.SIZE, uservals=uv, images=images, floatmap=True)
            check_against_oracle(ident, got, own, "specialised/own IR %s %s" % (name, idx))
            if name not in P.INEXACT_FOLD_SETS:
                check_against_oracle(ident, got, want, "specialised %s %s" % (name, idx))
                if ref is not None:
                    P.compare(ident, got, ref, "specialised %s %s" % (name, idx), P.magnitude_of(probe, values, idx))
        if not probe.image and len(frames) > 1 and ident != "print":
            assert any(frames[0].tobytes() != f.tobytes() for f in frames[1:]), ident      # evaluated at run time
