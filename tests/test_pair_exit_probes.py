"""Exit-driven pair-mode loops (hipgen_pair.cpp exit_driven_iteration), the part that needs no GPU: the off switch restores the
parent's kernel text, kernels outside pair mode do not change at all, and every probe of tests/pair_exit_probes.py
exercises the case it stands for (checked with the oracle alone)."""
import hashlib

import numpy as np
import pytest

import mathmap_amd as mm
from oracle.ccgen import CpuFilter
from tests import filters as F
from tests.pair_exit_probes import PROBES, by_name, count_channel

# sha256 of the specialised Mandelbrot kernel's functions (from the first `extern "C" __global__` on) as generated
# by the commit before the exit-driven loops (d0649bb): the per-iteration selects
PARENT_MANDELBROT_FUNCTIONS = "69fb4625447846cf1fb7947e734a9df5fef29d399c58e74fb4d0fdc93a14fc4e"


def functions_hash(source):
    return hashlib.sha256(source[source.index('extern "C" __global__'):].encode()).hexdigest()


def test_switch_off_restores_the_parent_kernel_functions(monkeypatch):
    monkeypatch.setenv("MMHIP_PAIR_EXIT", "0")
    off = F.load("mandelbrot").specialized({}).kernel_source
    assert functions_hash(off) == PARENT_MANDELBROT_FUNCTIONS
    assert "MM_PAIR_EXIT" not in off
    monkeypatch.delenv("MMHIP_PAIR_EXIT")
    on = F.load("mandelbrot").specialized({}).kernel_source
    assert functions_hash(on) != PARENT_MANDELBROT_FUNCTIONS
    assert "#define MM_PAIR_EXIT 1\n" in on and "mm_p += 2)" in on
    monkeypatch.setenv("MMHIP_PAIR_EXIT", "1")
    assert F.load("mandelbrot").specialized({}).kernel_source == on


def test_bool_pair_fallback_keeps_the_per_iteration_form(monkeypatch):
    """Only the lane-mask form has exit-driven loops: with MM_PAIR_MASKS 0 the text is the same under both settings."""
    monkeypatch.setenv("MMHIP_PAIR_MASKS", "0")
    texts = []
    for v in ("0", "1"):
        monkeypatch.setenv("MMHIP_PAIR_EXIT", v)
        texts.append(F.load("mandelbrot").specialized({}).kernel_source)
    assert texts[0] == texts[1] and "MM_PAIR_EXIT" not in texts[0]


@pytest.mark.parametrize("name", ["droste", "pond", "ident"])
def test_kernels_outside_pair_mode_keep_their_whole_text(name, monkeypatch):
    texts = []
    for v in ("0", "1"):
        monkeypatch.setenv("MMHIP_PAIR_EXIT", v)
        flt = F.load(name)
        texts += [flt.kernel_source, flt.specialized({}).kernel_source]
    assert "mm_p += 2)" not in texts[0]
    assert texts[0] == texts[2] and texts[1] == texts[3]
    assert "MM_PAIR_EXIT" not in texts[2] and "mm_xnotb" not in texts[3]


@pytest.mark.parametrize("name", [p[0] for p in PROBES])
def test_probe_runs_exit_driven_in_pair_mode(name, monkeypatch):
    monkeypatch.setenv("MMHIP_PAIR", "1")
    ks = mm.Filter(by_name(name)).kernel_source
    assert "mm_p += 2)" in ks and "#define MM_PAIR_EXIT 1\n" in ks and "} while (" in ks
    # the uniform bound is split off (one scalar comparison at the back edge) exactly where the condition has one
    assert ("s_cselect_b64" in ks[ks.index('extern "C" __global__'):]) == (name not in ("no_uniform_part",))
    monkeypatch.setenv("MMHIP_PAIR_EXIT", "0")
    ks = mm.Filter(by_name(name)).kernel_source
    assert "mm_p += 2)" in ks and "MM_PAIR_EXIT" not in ks and "} while (" not in ks[ks.index('extern "C" __global__'):]


def oracle_frame(name, w=83, h=61):
    return CpuFilter(mm.Filter(by_name(name)).ir_json_raw).render(w, h)


def test_probe_never_entered():
    f = oracle_frame("never_entered")
    assert (count_channel(f) == 0).all()
    assert len(np.unique(f[..., 1])) > 16          # the per-lane phi's initial value, x, reaches the result


def test_probe_one_iteration():
    assert (count_channel(oracle_frame("one_iteration")) == 1).all()


def test_probe_uniform_bound():
    f = oracle_frame("uniform_bound")
    assert (count_channel(f) == 7).all()           # the bound itself; no pixel escapes (|w| stays below 1.5)
    assert len(np.unique(f[..., 1])) > 16


def test_probe_lane_phi_and_iv():
    for name in ("lane_phi", "iv_and_lane_phi"):
        f = oracle_frame(name)
        assert len(np.unique(f[..., 1])) > 64 and len(np.unique(f[..., 0])) >= 8
    n = count_channel(oracle_frame("iv_and_lane_phi"))
    assert n.min() >= 1 and n.max() == 8 and len(np.unique(n)) == 8        # pixels leave at every back edge and at the bound
    # neighbours in a column leave at different back edges somewhere: the two pixels of a pair diverge
    assert (n[0:-1:2] != n[1::2]).any()


def test_probe_if_in_body():
    f = oracle_frame("if_in_body")
    n, c = count_channel(f, 0), count_channel(f, 2)
    assert len(np.unique(n)) >= 6 and len(np.unique(f[..., 1])) > 32
    # pixels that took both sides of the `if` while in the loop, pixels that took only one, and pairs that disagree
    assert ((c > 0) & (c < n)).sum() > 100 and (c == 0).any() and (c == n).any()
    assert (c[0:-1:2] != c[1::2]).any()


def test_probe_prestep_bound():
    f = oracle_frame("prestep_bound")
    n, m = count_channel(f, 0), count_channel(f, 2)
    # the bound is on m, which lags n by one step: pixels that never escape run 7 iterations (m = 0, 0, 1, ... 5 pass m < 6),
    # not the 6 that a test of the stepped counter would give
    assert n.max() == 7 and (n == 7).sum() > 100 and ((n == 7) == (m == 6)).all()
    assert len(np.unique(n)) >= 5


def test_probe_two_loops():
    f = oracle_frame("two_loops")
    n, m = count_channel(f, 0), count_channel(f, 1)
    assert len(np.unique(n)) >= 3 and len(np.unique(m)) >= 3
    assert (m <= n + 2).all() and (m == n + 2).any() and (m < n + 2).any()      # the second loop's bound is the first's exit value


def test_probe_uniform_in_if():
    f = oracle_frame("uniform_in_if")
    n = count_channel(f)
    assert len(np.unique(n)) >= 4 and len(np.unique(f[..., 1])) > 32
    # `n < 3` is true and later false while lanes are still active: many pixels run 5 iterations or more
    assert (n >= 5).sum() > 100 and (n <= 2).any()


def test_probe_no_uniform_part():
    n = count_channel(oracle_frame("no_uniform_part"))
    assert n.min() >= 1 and len(np.unique(n)) >= 4


def _hipcc_or_skip():
    import os
    import shutil
    from tools import pair_loop_isa as T
    if not (os.path.exists(T.hipcc()) or shutil.which(T.hipcc())):
        pytest.skip("no hipcc")
    return T


@pytest.mark.parametrize("name", [p[0] for p in PROBES])
def test_probe_kernel_assembles_offline(name, monkeypatch):
    """The generated text goes through the assembler with the JIT's options: lane masks that end up in vector registers
    only show there (and in the JIT)."""
    T = _hipcc_or_skip()
    monkeypatch.setenv("MMHIP_PAIR", "1")
    ks = mm.Filter(by_name(name)).kernel_source
    assert "#define MM_PAIR_EXIT 1\n" in ks
    assert T.assembly(ks, to_object=True) == ""


@pytest.mark.parametrize("seed", [27, 31])
def test_uniform_broadcast_stays_in_scalar_registers(seed, monkeypatch):
    """Two filters of the arithmetic fuzzer whose loops mix a non-literal wave-uniform truth value into per-lane logic: broadcast
    as a select between 64-bit constants it became a v_cndmask_b32 pair, the masks behind it sat in vector registers and the
    selects' mask operand did not assemble.  It goes through the ballot form (mm_bu)."""
    T = _hipcc_or_skip()
    from tests.fuzz_filters import make_filter_arith
    monkeypatch.setenv("MMHIP_PAIR", "1")
    ks = mm.Filter(make_filter_arith(seed)).kernel_source
    assert "#define MM_PAIR_EXIT 1\n" in ks
    assert T.assembly(ks, to_object=True) == ""


def test_mandelbrot_loop_counts_offline():
    """The likely path of the specialised Mandelbrot kernel's inner loop: 16 arithmetic instructions and 2 compares on the
    vector unit, at most 9 scalar and branch instructions (needs hipcc; profiles/r05_pair_loop_isa.txt is this tool's output)."""
    T = _hipcc_or_skip()
    res = T.analyse(T.assembly(F.load("mandelbrot").specialized({}).kernel_source), False)
    lp = res["likely path"]
    assert lp["valu"] <= 18 and lp["salu"] + lp["branch"] <= 9 and lp["mem"] == 0, lp
