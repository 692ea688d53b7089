"""Every probe of tests/language_probes.py on the GPU, in float-map mode: the generic kernel (one pixel per step), the kernel in pair mode
where the generator takes the filter, and Filter.specialized(set), each against the oracle (bit for bit, NaN in the same places) and
against the NumPy restatement of tests/language_reference.py (bit for bit; r, a and pow under the bound builtin_probes.compare
holds those library functions to).  The specialised variant is also held to the oracle's evaluation of its own IR, and in a
probe's `inexact_sets` (a NaN user value) to that alone, as tests/test_gpu_builtins.py does.  The last test prints how many
probes and variants ran, how many in pair mode, and the largest distance seen for r and a."""
import numpy as np
import pytest

import mathmap_amd as mm
from oracle.ccgen import CpuFilter
from tests import builtin_probes as BP
from tests import language_probes as P
from tests.gpu_util import render_device
from tests.test_language_reference import expected, hold, oracle_uservals, render_oracle

pytestmark = pytest.mark.gpu

TALLY = {"probes": 0, "variants": 0, "pair": 0, "arithmetic_pair": 0, "renders": 0, "distances": []}


def render(flt, probe, case, sname):
    inv = flt.invoke(case.width, case.height)
    for k, v in probe.uservals(sname).items():
        inv.set(k, v)
    for n, (kind, table) in probe.tables.items():
        (inv.set_curve if kind == "curve" else inv.set_gradient)(n, table)
    out = render_device(inv, case.width, case.height, rows=[case.rows] if case.rows else None, floatmap=True, t=case.t, frame=case.frame)
    lo, hi = case.rows or (0, case.height)
    TALLY["renders"] += 1
    return out[lo:hi]


def same_as_oracle(got, want, where):
    bad = BP.same_bits(np.ascontiguousarray(got), np.ascontiguousarray(want))
    print("%s: GPU vs oracle %d values differ" % (where, bad))
    assert bad == 0, (where, bad)


def pair_mode(flt):
    return "mm_p += 2)" in flt.kernel_source


@pytest.mark.parametrize("name", [p.name for p in P.PROBES])
def test_probe_on_the_gpu(name, monkeypatch):
    probe = P.BY_NAME[name]
    monkeypatch.delenv("MMHIP_PAIR", raising=False)
    generic = mm.Filter(probe.text)
    monkeypatch.setenv("MMHIP_PAIR", "1")
    paired = mm.Filter(probe.text)
    monkeypatch.delenv("MMHIP_PAIR", raising=False)
    variants = [("generic", generic)]
    if pair_mode(paired):
        if pair_mode(generic):      # a small body is paired without being asked: then the one-pixel kernel is the other variant
            monkeypatch.setenv("MMHIP_PAIR", "0")
            variants = [("generic", mm.Filter(probe.text))]
            monkeypatch.delenv("MMHIP_PAIR", raising=False)
            assert not pair_mode(variants[0][1])
        variants.append(("pair", paired))
        TALLY["pair"] += 1
        TALLY["arithmetic_pair"] += 1 if probe.arithmetic else 0
    TALLY["probes"] += 1
    TALLY["variants"] += len(variants) + 1
    cf = CpuFilter(generic.ir_json_raw)
    frames = []
    specials = {}
    for case in probe.cases:
        for sname in probe.sets:
            where = "%s %s %s" % (name, case, sname)
            want, ref = render_oracle(cf, probe, case, sname), expected(probe, case, sname)
            for label, flt in variants:
                got = render(flt, probe, case, sname)
                same_as_oracle(got, want, "%s %s" % (label, where))
                hold(probe, got, ref, "%s %s %s" % (label, case, sname), TALLY["distances"])
                if label == "generic":
                    frames.append(got)
            # the variant with this set's values as literals: no scalar user value is read at run time
            if sname not in specials:
                special = generic.specialized(dict((k, v) for k, v in probe.uservals(sname).items() if not isinstance(v, tuple)))
                assert "USERVAL_FLOAT_ACCESS" not in special.ir_json and "USERVAL_INT_ACCESS" not in special.ir_json, where
                specials[sname] = (special, CpuFilter(special.ir_json))
            special, own = specials[sname]
            got = render(special, probe, case, sname)
            same_as_oracle(got, render_oracle(own, probe, case, sname), "specialised/own IR " + where)
            if sname not in probe.inexact_sets:
                same_as_oracle(got, want, "specialised " + where)
                hold(probe, got, ref, "specialised %s %s" % (case, sname), TALLY["distances"])
    first = frames[0]
    flat = first.reshape(-1, 4)
    assert any(f.shape != first.shape or f.tobytes() != first.tobytes() for f in frames[1:]) or \
        any(flat[0].tobytes() != q.tobytes() for q in flat[1:]), name      # evaluated at run time


def test_report():
    """prints the tally of this module's run (with -s); asserts only that the probes above ran"""
    d = TALLY["distances"]
    print("language probes on the GPU: %d probes, %d variants (%d in pair mode, %d of them arithmetic control flow), %d renders; "
          "largest distance for r, a and pow: %s ulp" % (TALLY["probes"], TALLY["variants"], TALLY["pair"], TALLY["arithmetic_pair"],
                                                          TALLY["renders"], max(d) if d else "none seen"))
    if TALLY["probes"]:
        assert TALLY["variants"] >= 2 * TALLY["probes"]
