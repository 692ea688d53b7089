"""Spread pair steps (hipgen_pair.cpp emit_pixel_loop, MMHIP_PAIR_SPREAD) on the GPU: bytes equal to the oracle's and to the same
frame rendered with MMHIP_PAIR_SPREAD=0, tolerance 0.  Frames with a partial last segment, with segments wholly past the end and
with one and several tile rows at 2, 4, 8 and 16 rows per work-item; exact multiples of a step and of a tile, where every step is a
fast one; a band with an odd first row between sentinel rows at a padded stride; output formats that take the step as it was; a
clip, whose text is untouched; the fused probes of tests/pair_fma_probes.py.  Every case is a process of its own (this file run as
a script with the case as JSON): the generator reads its switches per compile and the runtime MMHIP_PPT per launch, from the
environment the case sets."""
import ctypes as C
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:          # run as a script, for one case
    sys.path.insert(0, ROOT)
pytestmark = pytest.mark.gpu

SWITCHES = ("MMHIP_PAIR", "MMHIP_PAIR_EXIT", "MMHIP_PAIR_EXIT_TAIL", "MMHIP_PAIR_PACK", "MMHIP_PAIR_PEEL", "MMHIP_PAIR_FMA2", "MMHIP_PAIR_MASKS",
            "MMHIP_PAIR_STEP", "MMHIP_PAIR_SPREAD", "MMHIP_PPT")
# the Mandelbrot shape of tests/pair_fma_probes.py with a real part that moves with t: the frames of a clip differ
MOVING = """filter t ()
  n = 0; w = x; v = y; ca = x * 1.5 + t; cb = y * 1.5;
  while (w * w + v * v < 4) && (n < 9) do
    tt = w * v; u = w * w - v * v + ca; v = tt + tt + cb; w = u; n = n + 1
  end;
  rgba:[n * 0.0625, w * 0.2 + 0.5, v * 0.2 + 0.5, 1]
end
"""


def run_case(**case):
    env = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    done = subprocess.run([sys.executable, os.path.abspath(__file__), json.dumps(case)], cwd=ROOT, env=env, capture_output=True, text=True)
    print(done.stdout[-3000:])
    assert done.returncode == 0, done.stdout[-3000:] + done.stderr[-3000:]
    assert "CASE OK" in done.stdout


@pytest.mark.parametrize("ppt", [2, 4, 8, 16])
@pytest.mark.parametrize("size", [(67, 41), (67, 131), (333, 251), (16, 517)])
def test_mandelbrot_frames(size, ppt):
    """A partial last segment (every height here), segments wholly past the end (41 rows at 4 rows per work-item and more), one
    tile row and several (517 rows at 2 rows per work-item: 17)."""
    run_case(kind="frame", size=size, ppt=ppt)


@pytest.mark.parametrize("size", [(64, 64), (64, 256)])
def test_exact_multiples_of_a_step_and_of_a_tile(size):
    run_case(kind="frame", size=size, ppt=None, fast_only=True)
    run_case(kind="frame", size=size, ppt=4, fast_only=True)


def test_row_band_with_an_odd_first_row_between_sentinels():
    run_case(kind="band", size=(67, 131), rows=(5, 120), ppt=4, pad=20)


@pytest.mark.parametrize("bpp,floatmap", [(3, False), (4, True)])
def test_other_output_formats_take_the_step_as_it_was(bpp, floatmap):
    run_case(kind="format", size=(67, 131), bpp=bpp, floatmap=floatmap, ppt=4)


def test_clip_of_three_frames_is_untouched():
    run_case(kind="clip", size=(67, 131))


def _fused_probes():
    from tests.pair_fma_probes import FMA_PROBES
    return [p[0] for p in FMA_PROBES if p[2]]


@pytest.mark.parametrize("name", _fused_probes())
def test_fused_probes(name):
    run_case(kind="probe", name=name, size=(67, 131), ppt=4)


# ---- the case, in its own process ----
def _child(case):
    import numpy as np

    import mathmap_amd as mm
    from mathmap_amd._lib import lib
    from mathmap_amd.striping import animation_frame_t
    from oracle.ccgen import CpuFilter
    from tests import filters as F
    from tests.pair_fma_probes import by_name as fma_by_name

    for k in SWITCHES:
        os.environ.pop(k, None)
    w, h = case["size"]
    kind = case["kind"]

    def build(spread, make):
        os.environ["MMHIP_PAIR_SPREAD"] = spread
        flt = make()
        assert ("mm_nty" in flt.kernel_source) == (spread == "1"), spread
        assert "mm_store_step(" in flt.kernel_source and "mm_nty" not in flt.clip_kernel_source
        return flt

    def both(make):
        flts = [("spread", build("1", make)), ("consecutive", build("0", make))]
        del os.environ["MMHIP_PAIR_SPREAD"]
        return flts

    def render_band(flt, rows, row_stride=None, bpp=4, floatmap=False, fill=0, lead=0):
        """rows [first, last) through render_rows into device memory behind `lead` sentinel rows; the whole buffer as bytes"""
        first, last = rows
        px = 16 if floatmap else bpp
        stride = row_stride if row_stride is not None else w * px
        size = (last - first + 2 * lead) * stride
        dev = lib().mmhip_device_alloc(size)
        assert dev
        try:
            buf = np.full(size, fill, np.uint8)
            assert lib().mmhip_copy_to_device(C.c_void_p(dev), buf.ctypes.data_as(C.c_void_p), size) == 0
            inv = flt.invoke(w, h)
            inv.render_rows(dev + lead * stride, first, last, row_stride=None if floatmap else stride, bpp=bpp, floatmap=floatmap)
            inv.sync()
            assert lib().mmhip_copy_to_host(buf.ctypes.data_as(C.c_void_p), C.c_void_p(dev), size) == 0
        finally:
            lib().mmhip_device_free(dev)
        return buf.reshape(last - first + 2 * lead, stride)

    def set_ppt(flt):
        if case.get("ppt"):
            os.environ["MMHIP_PPT"] = str(case["ppt"])
            assert flt.launch_geometry(w, h)["ppt"] == case["ppt"]

    mandelbrot = lambda: F.load("mandelbrot").specialized({})
    if kind in ("frame", "band", "format"):
        cpu = CpuFilter(F.load("mandelbrot").ir_json_raw)
        flts = both(mandelbrot)
        set_ppt(flts[0][1])
        got = {}
        if kind == "frame":
            want = cpu.render(w, h)
            if case.get("fast_only"):
                g = flts[0][1].launch_geometry(w, h)
                assert h % (2 * g["tile_h"]) == 0 and w % g["tile_w"] == 0
            for label, flt in flts:
                got[label] = flt.invoke(w, h).render()
        elif kind == "band":
            lo, hi = case["rows"]
            assert lo % 2 == 1
            stride, lead = w * 4 + case["pad"], 3
            want = cpu.render(w, h)[lo:hi]
            for label, flt in flts:
                buf = render_band(flt, (lo, hi), row_stride=stride, fill=0xA5, lead=lead)
                assert (buf[:lead] == 0xA5).all() and (buf[-lead:] == 0xA5).all() and (buf[:, w * 4:] == 0xA5).all(), label
                got[label] = buf[lead:-lead, :w * 4].reshape(hi - lo, w, 4)
        else:
            bpp, floatmap = case["bpp"], case["floatmap"]
            want = cpu.render(w, h, bpp=bpp, floatmap=floatmap)
            if floatmap:
                want = want.view(np.uint32)
            for label, flt in flts:
                buf = render_band(flt, (0, h), bpp=bpp, floatmap=floatmap)
                got[label] = buf.view(np.uint32).reshape(h, w, 4) if floatmap else buf.reshape(h, w, bpp)
        for label in got:
            assert np.array_equal(got[label], want), (label, int((got[label] != want).sum()))
        assert np.array_equal(got["spread"], got["consecutive"])
    elif kind == "clip":
        os.environ["MMHIP_PAIR"] = "1"
        clips = []
        for label, flt in both(lambda: mm.Filter(MOVING).specialized({})):
            clip = flt.invoke(w, h).render_clip(num_frames=3)
            for i in range(3):
                one = flt.invoke(w, h).render(t=animation_frame_t(i, 3), frame=i)
                assert np.array_equal(clip[i], one), (label, i, int((clip[i] != one).sum()))
            assert (clip[0] != clip[2]).any()
            clips.append(clip)
        assert np.array_equal(clips[0], clips[1])
        want = CpuFilter(mm.Filter(MOVING).ir_json_raw).render(w, h, t=animation_frame_t(1, 3))
        assert np.array_equal(clips[0][1], want)
    elif kind == "probe":
        os.environ["MMHIP_PAIR"] = "1"
        src = fma_by_name(case["name"])
        want = CpuFilter(mm.Filter(src).ir_json_raw).render(w, h)
        flts = both(lambda: mm.Filter(src).specialized({}))
        set_ppt(flts[0][1])
        for label, flt in flts:
            got = flt.invoke(w, h).render()
            assert np.array_equal(got, want), (label, int((got != want).sum()))
    else:
        raise ValueError(kind)
    print("CASE OK", json.dumps(case))


if __name__ == "__main__":
    _child(json.loads(sys.argv[1]))
