"""The front end -- parser.cpp and lower.cpp -- stands on both sides of every HIP-against-oracle comparison, so it is held here
to an independent reference: each probe of tests/language_probes.py, evaluated by the oracle on the IR as lowered
(ir_json_raw), on the IR after the passes (ir_json) and on each user-value set's specialised IR, against the NumPy
restatement of tests/language_reference.py.  Bit for bit, NaN in the same places; r, a and pow under the bound
builtin_probes.compare holds those library functions to.  tests/test_gpu_language.py repeats it on the GPU."""
import os
import re

import numpy as np
import pytest

import mathmap_amd as mm
from oracle.ccgen import CpuFilter
from tests import builtin_probes as BP
from tests import language_probes as P
from tests import language_reference as L
from tests.conftest import ROOT

EXACT = "add_1"       # an id builtin_probes.compare holds bit for bit


def oracle_uservals(probe, name):
    """the set as CpuFilter.render takes it: scalars, colours, and the tables by name"""
    uv = dict(probe.uservals(name))
    for n, (kind, table) in probe.tables.items():
        uv[n] = table
    return uv


def render_oracle(cf, probe, case, name):
    out = cf.render(case.width, case.height, uservals=oracle_uservals(probe, name), t=case.t, frame=case.frame, floatmap=True, rows=case.rows)
    lo, hi = case.rows or (0, case.height)
    return out[lo:hi]


def hold(probe, got, want, where, distances=None):
    """`got` against the restatement `want`: bit for bit, but the probe's library channels under that function's bound"""
    channels = probe.libm[1] if probe.libm else ()
    exact = [c for c in range(4) if c not in channels]
    BP.compare(EXACT, np.ascontiguousarray(got[..., exact]), np.ascontiguousarray(want[..., exact]), "%s %s" % (probe.name, where))
    if channels:
        g, w = np.ascontiguousarray(got[..., list(channels)]), np.ascontiguousarray(want[..., list(channels)])
        BP.compare(probe.libm[0], g, w, "%s %s" % (probe.name, where))
        if distances is not None:
            fin = np.isfinite(g) & np.isfinite(w)
            if fin.any():
                distances.append(int(np.abs(g[fin].view(np.int32).astype(np.int64) - w[fin].view(np.int32).astype(np.int64)).max()))


_EXPECTED = {}


def expected(probe, case, name):
    """computed once, shared, never written to"""
    key = (probe.name, repr(case), name)
    if key not in _EXPECTED:
        e = probe.expected(case, name)
        e.setflags(write=False)
        _EXPECTED[key] = e
    return _EXPECTED[key]


def declared_internals():
    with open(os.path.join(ROOT, "mathmap_amd", "csrc", "parser.cpp")) as f:
        text = f.read()
    body = re.search(r"is_internal_name\(.*?names\[\]\s*=\s*\{(.*?)\};", text, re.S).group(1)
    names = re.findall(r'"([^"]+)"', body)
    assert len(names) >= 11
    return names


def test_every_grammar_rule_and_variable_has_a_probe():
    covered = set(c for p in P.PROBES for c in p.covers)
    rules, elsewhere = set(P.RULES), set(P.RULES_ELSEWHERE)
    assert len(rules) == len(P.RULES) and elsewhere <= rules and not covered & elsewhere
    assert rules - elsewhere <= covered, sorted(rules - elsewhere - covered)
    assert set(declared_internals()) <= set(P.VARIABLES), sorted(set(declared_internals()) - set(P.VARIABLES))
    assert set(P.VARIABLES) <= covered, sorted(set(P.VARIABLES) - covered)
    # every variable under every flag set
    for flags in L.FLAGS:
        seen = set(c for p in P.PROBES if p.flags == flags for c in p.covers)
        assert set(P.VARIABLES) <= seen, (flags, sorted(set(P.VARIABLES) - seen))


def test_a_probe_naming_a_rule_uses_it():
    """the words of a rule stand in the texts of the probes that name it"""
    marks = {"while": "while ", "do_while": "do ", "for": "for ", "if_then": "if ", "if_then_else": " else", "pow": "^", "mod": "%", "xor": " xor ",
             "or": "||", "and": "&&", "not": "!", "equal": "==", "notequal": "!=", "lessequal": "<=", "greaterequal": ">=", "cast": ":[",
             "subscript_range": "..", "else_semicolon": "; else", "end_semicolon": "; end", "type_curve": "curve ", "type_gradient": "gradient ",
             "type_bool": "bool ", "type_color": "color ", "type_image": "image ", "type_int": "int ", "div": " / ", "sub_assign": "] = "}
    for p in P.PROBES:
        for c in p.covers:
            if c in marks:
                assert marks[c] in p.text, (p.name, c)
            elif c in P.VARIABLES:
                assert re.search(r"(?<![A-Za-z_])%s(?![A-Za-z_0-9])" % re.escape(c), p.text.split(")\n", 1)[1]), (p.name, c)


def test_tag_conversion_is_refused():
    with pytest.raises(mm.MathMapError, match="not implemented"):
        mm.Filter("filter f () rgba:[1, 1, 1, 1] + xy::ra:[x, y][0] end")


def test_the_table_sets_hit_the_entries_they_name():
    idx = L.table_index(np.array([-0.5, 1.5, 1.0, np.nan, P._k(1), P._ulp(P._k(1), -1), P._k(512), P._ulp(P._k(512), -1), P._ulp(1.0, -1)], np.float32))
    assert list(idx[:4]) == [0, 1023, 1023, 0]
    assert idx[4] - idx[5] == 1 or idx[4] == idx[5] == 1 or idx[4] == idx[5] == 0     # a step of one entry at most
    assert 510 <= idx[6] <= 512 and idx[6] - idx[7] in (0, 1) and idx[8] == 1022
    cv, gr = P.curve_table(), P.gradient_table()
    assert len(set(cv.tolist())) == 1024 and (np.diff(cv) < 0).any() and (np.diff(cv) > 0).any()
    assert len(set((gr & 0xff).tolist())) > 64 and (gr[1:] != gr[:-1]).all()


@pytest.mark.parametrize("name", [p.name for p in P.PROBES])
def test_oracle_equals_the_restatement(name):
    probe = P.BY_NAME[name]
    flt = mm.Filter(probe.text)
    raw, passed = CpuFilter(flt.ir_json_raw), CpuFilter(flt.ir_json)
    frames = []
    for case in probe.cases:
        for sname in probe.sets:
            want = expected(probe, case, sname)
            got = render_oracle(raw, probe, case, sname)
            hold(probe, got, want, "raw %s %s" % (case, sname))
            hold(probe, render_oracle(passed, probe, case, sname), want, "passes %s %s" % (case, sname))
            frames.append(got)
            # the user values as literals: what a render with this set runs
            special = flt.specialized(dict((k, v) for k, v in probe.uservals(sname).items() if not isinstance(v, tuple)))
            assert "USERVAL_FLOAT_ACCESS" not in special.ir_json and "USERVAL_INT_ACCESS" not in special.ir_json, (name, sname)
            own = render_oracle(CpuFilter(special.ir_json), probe, case, sname)
            if sname not in probe.inexact_sets:      # a NaN literal meets the folds: the GPU test holds it to this IR's own oracle
                hold(probe, own, want, "specialised %s %s" % (case, sname))
    # evaluated at run time: not one value for every pixel and every set
    first = frames[0]
    varies = any(f.shape != first.shape or f.tobytes() != first.tobytes() for f in frames[1:])
    flat = first.reshape(-1, 4)
    varies = varies or any(flat[0].tobytes() != q.tobytes() for q in flat[1:])
    assert varies, name


def test_pair_mode_takes_the_arithmetic_control_flow(monkeypatch):
    """The pair generator takes every control-flow probe that is arithmetic alone (Probe.arithmetic) -- among them loops whose
    lanes, and whose two pixels of a pair, leave at different trips -- so tests/test_gpu_language.py runs them in pair mode.
    Generating a kernel's text needs no GPU."""
    arithmetic = [p for p in P.PROBES if p.arithmetic]
    assert len(arithmetic) == 7
    monkeypatch.setenv("MMHIP_PAIR", "1")
    taken = [p.name for p in arithmetic if "mm_p += 2)" in mm.Filter(p.text).kernel_source]
    monkeypatch.delenv("MMHIP_PAIR")
    assert taken == [p.name for p in arithmetic], sorted(set(p.name for p in arithmetic) - set(taken))
