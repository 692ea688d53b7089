"""Every builtin overload of mathmap_amd/csrc/builtins.cpp has a probe (tests/builtin_probes.py) that provably reaches it and
is held, through the oracle, to an independent NumPy restatement (tests/builtin_reference.py) -- or is a library function
that a named test covers.  The oracle evaluates the front end's IR, so this is the check of the front end's arithmetic;
tests/test_gpu_builtins.py repeats it on the GPU."""
import os
import re

import numpy as np
import pytest

import mathmap_amd as mm
from oracle.ccgen import CpuFilter
from tests import builtin_probes as P
from tests import builtin_reference as R
from tests.conftest import ROOT


def declared_ids():
    """the ids R.def and R.macro register"""
    with open(os.path.join(ROOT, "mathmap_amd", "csrc", "builtins.cpp")) as f:
        text = f.read()
    ids = re.findall(r'R\.def\("[^"]+",\s*"([^"]+)"', text)
    ids += ["macro_" + n for n in re.findall(r'R\.macro\("([^"]+)"', text)]
    assert len(ids) > 150
    return ids


def test_every_overload_has_a_probe_or_a_named_test():
    ids = declared_ids()
    defs = [i for i in ids if not i.startswith("macro_")]
    assert len(defs) == len(set(defs))
    probed, elsewhere = set(P.BY_ID), set(R.COVERED_ELSEWHERE)
    assert not probed & elsewhere
    assert probed | elsewhere == set(ids), (sorted(set(ids) - probed - elsewhere), sorted((probed | elsewhere) - set(ids)))
    assert probed == set(R.REF) | R.SAME_AS and not set(R.REF) & R.SAME_AS
    assert set(R.EVIDENCE) == elsewhere


def reach_of_test(path, name):
    """The source text the named test can take a filter from: the function with its decorators, and, transitively, every
    module-level assignment and function of its file whose name that text mentions (parameter tables, fixtures, texts)."""
    import ast
    with open(os.path.join(ROOT, path)) as f:
        source = f.read()
    tree = ast.parse(source)
    top = {}
    for node in tree.body:
        names = []
        if isinstance(node, (ast.FunctionDef, ast.ClassDef)):
            names = [node.name]
        elif isinstance(node, ast.Assign):
            names = [t.id for t in node.targets if isinstance(t, ast.Name)]
        lines = source.split("\n")
        first = min([d.lineno for d in getattr(node, "decorator_list", [])] + [node.lineno])
        for n in names:
            top[n] = "\n".join(lines[first - 1:node.end_lineno])
    assert name in top, (path, name)
    text, seen, grew = top[name], {name}, True
    while grew:
        grew = False
        for n, seg in top.items():
            if n not in seen and not n.startswith("test_") and re.search(r"\b%s\b" % re.escape(n), text):
                text, grew = text + "\n" + seg, True
                seen.add(n)
    return text


@pytest.mark.parametrize("ident", sorted(R.COVERED_ELSEWHERE))
def test_named_test_exercises_the_overload(ident):
    """The named test exists; the expression stands in what that test runs -- its own text and the tables, fixtures and
    filter texts of its file that it names, or a filter of another file that it names by `link` -- and the expression
    resolves to the id."""
    path, name = R.COVERED_ELSEWHERE[ident].split("::")
    reach = reach_of_test(path, name)
    expr, text, where, link = R.EVIDENCE[ident]
    if where == path:
        assert expr in reach, (path, name, expr)
    else:
        with open(os.path.join(ROOT, where)) as f:
            other = f.read()
        assert link in reach and link in other and expr in other, (where, link, expr)
    assert expr in text
    assert ident in mm.Filter(text).builtin_ids, (ident, sorted(mm.Filter(text).builtin_ids))


@pytest.mark.parametrize("ident", [p.id for p in P.PROBES])
def test_oracle_equals_the_numpy_restatement(ident):
    probe = P.BY_ID[ident]
    images = {"in": P.probe_image()} if probe.image else {}
    for text, idx in probe.texts():
        flt = mm.Filter(text)
        assert ident in flt.builtin_ids, (ident, sorted(flt.builtin_ids))
        cf = CpuFilter(flt.ir_json_raw)
        outs = {}
        for name, values in probe.sets.items():
            uv = P.uservals(values)
            got = cf.render(P.SIZE, P.SIZE, uservals=uv, images=images, floatmap=True)
            outs[name] = got
            if ident in R.SAME_AS:
                continue
            want = np.stack([P.expected(probe, values)[i] for i in idx], axis=-1)
            P.compare(ident, got, want, "%s %s" % (name, idx), P.magnitude_of(probe, values, idx))
        if not probe.image and len(outs) > 1:
            # nothing was folded away: the frame depends on the user values
            frames = list(outs.values())
            assert any(frames[0].tobytes() != f.tobytes() for f in frames[1:]) or ident == "print", ident
    if probe.same_as:
        other, call = probe.same_as
        for (text, idx), (text2, _) in zip(probe.texts(), probe.texts(call)):
            f2 = mm.Filter(text2)
            assert other in f2.builtin_ids and ident not in f2.builtin_ids
            a, b = CpuFilter(mm.Filter(text).ir_json_raw), CpuFilter(f2.ir_json_raw)
            for name, values in probe.sets.items():
                uv = P.uservals(values)
                ga = a.render(P.SIZE, P.SIZE, uservals=uv, floatmap=True)
                gb = b.render(P.SIZE, P.SIZE, uservals=uv, floatmap=True)
                assert np.array_equal(np.isnan(ga), np.isnan(gb)), (ident, name)
                assert np.array_equal(ga[~np.isnan(ga)].view(np.uint32), gb[~np.isnan(gb)].view(np.uint32)), (ident, name)


def test_the_nonfinite_set_makes_nan_and_both_infinities_in_the_first_scalar():
    s0 = P.scalar_values(P.SETS["nonfinite"])[0]
    assert np.isnan(s0).any() and np.isposinf(s0).any() and np.isneginf(s0).any() and np.isfinite(s0).any()
    one = P.scalar_values(P.SETS["generic"])[0]
    x, _ = P.coordinates()
    assert np.array_equal(one, x * np.float32(1.0) + np.float32(0.25))      # the second factor is exactly 1


def test_builtin_ids_of_a_filter():
    flt = mm.Filter("filter f (image in) p = in(xy); q = quat:[x, y, 1, 2] * quat:[y, x, 0, 1]; p * q[0] + abs(ri:[x, y]) end")
    assert {"mul_quat", "macro___origVal", "origValXY", "abs_ri", "mul_s", "add_s"} <= flt.builtin_ids
    assert "mul_n" not in flt.builtin_ids and "mul_cquat" not in flt.builtin_ids
    assert mm.Filter(ir_json=flt.ir_json_raw).builtin_ids == frozenset()
