"""The peeled first loop trip of specialised pair kernels (specialize.cpp peel_first_trips), the part that needs no GPU:
MMHIP_PAIR_PEEL=1 peels where the probe's case says so, the default (and MMHIP_PAIR_PEEL=0) is the unpeeled text, kernels that are not in
exit-driven pair mode keep theirs, `0 + x` stays an addition in the peeled trip, every probe of tests/pair_peel_probes.py
exercises its case (checked with the oracle alone) and assembles offline."""
import re

import numpy as np
import pytest

import mathmap_amd as mm
from oracle.ccgen import CpuFilter
from tests import filters as F
from tests.pair_peel_probes import PEEL_PROBES, by_name, count_channel


def functions(ks):
    return ks[ks.index('extern "C" __global__'):]


def texts(src, monkeypatch, **env):
    """(peeled, unpeeled) specialised kernel texts of a probe in forced pair mode"""
    monkeypatch.setenv("MMHIP_PAIR", "1")
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    monkeypatch.setenv("MMHIP_PAIR_PEEL", "1")
    on = mm.Filter(src).specialized({}).kernel_source
    monkeypatch.setenv("MMHIP_PAIR_PEEL", "0")
    off = mm.Filter(src).specialized({}).kernel_source
    monkeypatch.delenv("MMHIP_PAIR_PEEL")
    assert mm.Filter(src).specialized({}).kernel_source == off          # off is the default
    return on, off


def loop_count_starts(fn):
    """the literal starts of the loops' uniform counters (`int uv.. = N;` in front of each loop)"""
    return [int(v) for v in re.findall(r"\n\s+int uv\d+_\d+ = (-?\d+);", fn)]


@pytest.mark.parametrize("name,peeled", [(p[0], p[2]) for p in PEEL_PROBES])
def test_probe_is_peeled_where_its_case_says(name, peeled, monkeypatch):
    on, off = texts(by_name(name), monkeypatch)
    assert "mm_p += 2)" in on and "#define MM_PAIR_EXIT 1\n" in on
    if peeled == 0:
        assert on == off
        return
    if peeled < 0:          # the inner loop is peeled (its counter starts from 1 inside the outer loop), the outer one is not
        assert on != off and 1 in loop_count_starts(functions(on)) and 1 not in loop_count_starts(functions(off))
        return
    assert on != off
    # the induction variables start from 1 behind a peeled trip, from 0 without it
    assert loop_count_starts(functions(on)) == [1] * peeled and loop_count_starts(functions(off)) == [0] * peeled
    assert functions(on).count("while (mm_a") == functions(off).count("while (mm_a") == peeled


def test_mandelbrot_is_peeled_and_the_switch_restores_the_text(monkeypatch):
    monkeypatch.setenv("MMHIP_PAIR_PEEL", "1")
    on = F.load("mandelbrot").specialized({}).kernel_source
    fn = functions(on)
    # c = 0 * 0 + p of the first trip: the products fold, the additions of 0 stay (p may be -0)
    assert len(re.findall(r"= \(mm_vf\(0\.0f\) \+ mm_vf\(v\d+_\d+\)\);", fn)) == 2
    assert loop_count_starts(fn) == [1] and "mm_sqrt_f32(0.0)" not in fn          # and sqrt(0) < 2 of the entry test is gone
    monkeypatch.setenv("MMHIP_PAIR_PEEL", "0")
    off = F.load("mandelbrot").specialized({}).kernel_source
    assert loop_count_starts(functions(off)) == [0] and "mm_sqrt_f32(0.0)" in off and "mm_vf(0.0f) +" not in functions(off)
    # the generic kernel has no literals to fold: same text either way
    generic_off = F.load("mandelbrot").kernel_source
    monkeypatch.setenv("MMHIP_PAIR_PEEL", "1")
    assert F.load("mandelbrot").kernel_source == generic_off
    monkeypatch.delenv("MMHIP_PAIR_PEEL")
    assert F.load("mandelbrot").specialized({}).kernel_source == off          # off is the default


def test_only_exit_driven_pair_kernels_keep_a_peeled_trip(monkeypatch):
    """The same filter outside pair mode, and in pair mode with per-iteration selects, is the unpeeled text."""
    src = by_name("entered")
    for env in ({"MMHIP_PAIR": "0"}, {"MMHIP_PAIR": "1", "MMHIP_PAIR_EXIT": "0"}, {"MMHIP_PAIR": "1", "MMHIP_PAIR_MASKS": "0"}):
        for k in ("MMHIP_PAIR", "MMHIP_PAIR_EXIT", "MMHIP_PAIR_MASKS"):
            monkeypatch.delenv(k, raising=False)
        on, off = texts(src, monkeypatch, **env)
        assert on == off, env
    # unset MMHIP_PAIR: the probe is small enough for pair mode by itself
    for k in ("MMHIP_PAIR", "MMHIP_PAIR_EXIT", "MMHIP_PAIR_MASKS"):
        monkeypatch.delenv(k, raising=False)


@pytest.mark.parametrize("name", ["droste", "pond", "ident"])
def test_kernels_outside_pair_mode_keep_their_text(name, monkeypatch):
    monkeypatch.setenv("MMHIP_PAIR_PEEL", "0")
    off = F.load(name).specialized({}).kernel_source
    monkeypatch.setenv("MMHIP_PAIR_PEEL", "1")
    assert F.load(name).specialized({}).kernel_source == off


def test_peeled_trip_keeps_the_addition_of_zero(monkeypatch):
    on, _ = texts(by_name("minus_zero"), monkeypatch)
    assert re.search(r"= \(mm_vf\(0\.0f\) \+ mm_vf\(v\d+_\d+\)\);", functions(on))


# ---- the oracle's frames: each probe exercises its case ----
def oracle_frame(name, w=83, h=61, **kw):
    return CpuFilter(mm.Filter(by_name(name)).ir_json_raw).render(w, h, **kw)


def test_probe_entered():
    n = count_channel(oracle_frame("entered"))
    assert n.min() >= 2 and n.max() == 8 and len(np.unique(n)) >= 5 and (n[0:-1:2] != n[1::2]).any()


def test_probe_not_provably_entered():
    n = count_channel(oracle_frame("not_provably_entered"))
    assert (n == 0).sum() > 100 and n.max() == 8          # pixels that never enter, and pixels the bound stops


def test_probe_frame_constant_init():
    a, b = oracle_frame("frame_constant_init", t=0.3), oracle_frame("frame_constant_init", t=0.9)
    assert (a != b).any() and count_channel(a).min() >= 1          # the initial value follows t; every pixel enters


def test_probe_bound_one():
    f = oracle_frame("bound_one")
    assert (count_channel(f) == 1).all() and len(np.unique(f[..., 1])) > 32 and len(np.unique(f[..., 2])) > 16      # one trip, its values read


def test_probe_some_leave_at_once():
    n = count_channel(oracle_frame("some_leave_at_once"))
    assert (n == 1).sum() > 500 and (n > 1).sum() > 500 and n.max() == 8 and (n[0:-1:2] != n[1::2]).any()


def test_probe_if_in_body():
    f = oracle_frame("if_in_body")
    n, c = count_channel(f, 0), count_channel(f, 2)
    assert len(np.unique(n)) >= 4 and (c > 0).sum() > 100 and (c == 0).sum() > 100      # the `then` side is taken later, never in the first trip
    assert (c < n).all()


def test_probe_two_loops():
    f = oracle_frame("two_loops")
    n, m = count_channel(f, 0), count_channel(f, 1)
    assert len(np.unique(n)) >= 3 and len(np.unique(m)) >= 3 and n.min() >= 1 and m.min() >= 1


def test_probe_nested():
    f = oracle_frame("nested")
    s = count_channel(f)
    assert len(np.unique(s)) >= 4 and s.min() >= 1          # the inner loop runs once to three times per pixel, one to three trips each


def test_probe_minus_zero():
    f = CpuFilter(mm.Filter(by_name("minus_zero")).ir_json_raw).render(83, 61, floatmap=True)
    p, w = f[..., 2], f[..., 0]
    assert (p == 0).all() and np.signbit(p).sum() > 1000 and (~np.signbit(p)).sum() > 1000      # -0 in the left half
    assert (w == 0).all() and not np.signbit(w).any()                                            # 0 + -0 is +0


# ---- offline assembly ----
@pytest.mark.parametrize("name", [p[0] for p in PEEL_PROBES])
def test_probe_kernel_assembles_offline(name, monkeypatch):
    import os
    import shutil
    from tools import pair_loop_isa as T
    if not (os.path.exists(T.hipcc()) or shutil.which(T.hipcc())):
        pytest.skip("no hipcc")
    monkeypatch.setenv("MMHIP_PAIR", "1")
    monkeypatch.setenv("MMHIP_PAIR_PEEL", "1")
    assert T.assembly(mm.Filter(by_name(name)).specialized({}).kernel_source, to_object=True) == ""
