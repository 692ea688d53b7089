"""The fast pair step (hipgen_pair.cpp emit_pixel_loop, MMHIP_PAIR_STEP) on the GPU: bytes equal to the oracle's and to the render
with MMHIP_PAIR_STEP=0, tolerance 0.  Small frames that put the step at its edges: a width that is no multiple of the tile's and
an odd height (the last pair's second row is past the end), one row, one column of two rows, a band with an odd first row, 1, 2
and 8 steps per work-item with the last one straddling the end of the frame, the launch geometry's first cut, a padded row
stride, the output formats that must take the step as it was, a clip against its frames one by one, and the probes of
tests/pair_fma_probes.py and tests/pair_count_probes.py under either value of the switch."""
import ctypes as C

import numpy as np
import pytest

import mathmap_amd as mm
from mathmap_amd._lib import lib
from mathmap_amd.striping import animation_frame_t
from oracle.ccgen import CpuFilter
from tests import filters as F
from tests import launch_sizes as LS
from tests.pair_count_probes import COUNT_PROBES, PACK_PROBES
from tests.pair_count_probes import by_name as count_by_name
from tests.pair_fma_probes import FMA_PROBES, RAGGED
from tests.pair_fma_probes import by_name as fma_by_name

pytestmark = pytest.mark.gpu

SWITCHES = ("MMHIP_PAIR", "MMHIP_PAIR_EXIT", "MMHIP_PAIR_EXIT_TAIL", "MMHIP_PAIR_PACK", "MMHIP_PAIR_PEEL", "MMHIP_PAIR_FMA2", "MMHIP_PAIR_MASKS",
            "MMHIP_PAIR_STEP", "MMHIP_PPT")
MODES = [("default", {}), ("step_off", {"MMHIP_PAIR_STEP": "0"})]
FUSED = dict((p[0], p[2]) for p in FMA_PROBES)
# the Mandelbrot shape of tests/pair_fma_probes.py with a real part that moves with t: the frames of a clip differ
MOVING = """filter t ()
  n = 0; w = x; v = y; ca = x * 1.5 + t; cb = y * 1.5;
  while (w * w + v * v < 4) && (n < 9) do
    tt = w * v; u = w * w - v * v + ca; v = tt + tt + cb; w = u; n = n + 1
  end;
  rgba:[n * 0.0625, w * 0.2 + 0.5, v * 0.2 + 0.5, 1]
end
"""


def clean(monkeypatch, **env):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def mandelbrots(monkeypatch):
    """[(mode, specialised Mandelbrot filter)]: the fast step, and the step as it was"""
    out = []
    for label, env in MODES:
        clean(monkeypatch, **env)
        flt = F.load("mandelbrot").specialized({})
        assert ("mm_store_step(" in flt.kernel_source) == (label == "default"), label
        out.append((label, flt))
    clean(monkeypatch)
    return out


@pytest.fixture(scope="module")
def oracle():
    flt = CpuFilter(F.load("mandelbrot").ir_json_raw)
    frames = {}

    def render(w, h, **kw):
        key = (w, h, tuple(sorted(kw.items())))
        if key not in frames:
            frames[key] = flt.render(w, h, **kw)
            frames[key].setflags(write=False)
        return frames[key]
    return render


def render_band(flt, w, h, rows, row_stride=None, bpp=4, floatmap=False, fill=None):
    """rows [first, last) of the frame through render_rows into device memory `row_stride` bytes apart; the whole buffer as bytes"""
    first, last = rows
    px = 16 if floatmap else bpp
    stride = row_stride if row_stride is not None else w * px
    size = (last - first) * stride
    dev = lib().mmhip_device_alloc(size)
    assert dev
    try:
        buf = np.full(size, 0 if fill is None else fill, np.uint8)
        assert lib().mmhip_copy_to_device(C.c_void_p(dev), buf.ctypes.data_as(C.c_void_p), size) == 0
        inv = flt.invoke(w, h)
        inv.render_rows(dev, first, last, row_stride=None if floatmap else stride, bpp=bpp, floatmap=floatmap)
        inv.sync()
        assert lib().mmhip_copy_to_host(buf.ctypes.data_as(C.c_void_p), C.c_void_p(dev), size) == 0
    finally:
        lib().mmhip_device_free(dev)
    return buf.reshape(last - first, stride)


@pytest.mark.parametrize("size", [(67, 41), (16, 1), (1, 2)])
def test_ragged_frames(size, monkeypatch, oracle):
    """67 x 41: the last tile column is partial and the last pair's second row is past the end; one row; one column of two rows."""
    w, h = size
    want = oracle(w, h)
    for label, flt in mandelbrots(monkeypatch):
        got = flt.invoke(w, h).render()
        assert np.array_equal(got, want), (label, int((got != want).sum()))


def test_band_with_an_odd_first_row(monkeypatch, oracle):
    """Rows (5, 38) of 67 x 41: the output pointer and the y table both start at the band."""
    w, h = RAGGED
    want = oracle(w, h)[5:38]
    for label, flt in mandelbrots(monkeypatch):
        got = render_band(flt, w, h, (5, 38)).reshape(33, w, 4)
        assert np.array_equal(got, want), (label, int((got != want).sum()))


@pytest.mark.parametrize("ppt", [2, 4, 16])
def test_steps_per_work_item(ppt, monkeypatch, oracle):
    """67 x 131 with 2, 4 and 16 rows per work-item: 1, 2 and 8 steps, the last of the frame straddling its end."""
    w, h = 67, 131
    want = oracle(w, h)
    for label, flt in mandelbrots(monkeypatch):
        monkeypatch.setenv("MMHIP_PPT", str(ppt))
        assert flt.launch_geometry(w, h)["ppt"] == ppt
        got = flt.invoke(w, h).render()
        monkeypatch.delenv("MMHIP_PPT")
        assert np.array_equal(got, want), (label, ppt, int((got != want).sum()))


def test_first_cut_of_the_launch_geometry(monkeypatch, oracle):
    flts = mandelbrots(monkeypatch)
    g = flts[0][1].launch_geometry(64, 64)
    (_, w, h, _), = LS.cut_sizes(g["tile_w"], g["tile_h"])[:1]
    want = oracle(w, h)
    for label, flt in flts:
        got = flt.invoke(w, h).render()
        assert np.array_equal(got, want), (label, w, h, int((got != want).sum()))


def test_padded_row_stride(monkeypatch, oracle):
    """Rows 67 * 4 + 20 bytes apart: the pixels are the oracle's and the padding keeps what it held."""
    w, h = RAGGED
    want = oracle(w, h)
    stride = w * 4 + 20
    for label, flt in mandelbrots(monkeypatch):
        buf = render_band(flt, w, h, (0, h), row_stride=stride, fill=0xA5)
        got = buf[:, :w * 4].reshape(h, w, 4)
        assert np.array_equal(got, want), (label, int((got != want).sum()))
        assert (buf[:, w * 4:] == 0xA5).all(), label


@pytest.mark.parametrize("bpp,floatmap", [(1, False), (2, False), (3, False), (4, True)])
def test_other_output_formats_take_the_step_as_it_was(bpp, floatmap, monkeypatch, oracle):
    w, h = RAGGED
    want = oracle(w, h, bpp=bpp, floatmap=floatmap)
    for label, flt in mandelbrots(monkeypatch):
        buf = render_band(flt, w, h, (0, h), bpp=bpp, floatmap=floatmap)
        if floatmap:
            same = np.array_equal(buf.view(np.uint32).reshape(h, w, 4), want.view(np.uint32))
        else:
            same = np.array_equal(buf.reshape(h, w, bpp), want)
        assert same, (label, bpp, floatmap)


def test_clip_of_three_frames_equals_its_frames(monkeypatch):
    w, h = RAGGED
    clips = []
    for label, env in MODES:
        clean(monkeypatch, MMHIP_PAIR="1", **env)
        flt = mm.Filter(MOVING).specialized({})
        assert ("mm_store_step(" in flt.clip_kernel_source) == (label == "default"), label
        inv = flt.invoke(w, h)
        clip = inv.render_clip(num_frames=3)
        for i in range(3):
            one = flt.invoke(w, h).render(t=animation_frame_t(i, 3), frame=i)
            assert np.array_equal(clip[i], one), (label, i, int((clip[i] != one).sum()))
        assert (clip[0] != clip[2]).any()
        clips.append(clip)
    assert np.array_equal(clips[0], clips[1])
    want = CpuFilter(mm.Filter(MOVING).ir_json_raw).render(w, h, t=animation_frame_t(1, 3))
    assert np.array_equal(clips[0][1], want)


def check_probe(src, fused, specialise, monkeypatch):
    oracle = CpuFilter(mm.Filter(src).ir_json_raw)
    g = None
    frames = {}
    for label, env in MODES:
        clean(monkeypatch, MMHIP_PAIR="1", **env)
        flt = mm.Filter(src).specialized({}) if specialise else mm.Filter(src)
        ks = flt.kernel_source
        assert "mm_p += 2)" in ks and ("mm_store_step(" in ks) == (label == "default" and fused > 0), label
        g = g or flt.launch_geometry(64, 64)
        for w, h in [RAGGED] + [(w, h) for _, w, h, _ in LS.cut_sizes(g["tile_w"], g["tile_h"])[:1]]:
            if (w, h) not in frames:
                frames[w, h] = oracle.render(w, h)
            got = flt.invoke(w, h).render()
            assert np.array_equal(got, frames[w, h]), (label, w, h, int((got != frames[w, h]).sum()))


@pytest.mark.parametrize("name", [p[0] for p in FMA_PROBES])
def test_fma_probe_matches_oracle_under_either_value(name, monkeypatch):
    """The fourteen probes of the fused doubling, specialised as tests/test_gpu_pair_fma.py renders them: a ragged frame and the first cut."""
    check_probe(fma_by_name(name), FUSED[name], True, monkeypatch)


@pytest.mark.parametrize("name", [p[0] for p in COUNT_PROBES + PACK_PROBES])
def test_count_and_pack_probe_matches_oracle_under_either_value(name, monkeypatch):
    """The probes of the counted back edge and of the result pack, as tests/test_gpu_pair_count.py renders them (nothing is fused in
    them: they keep the step as it was)."""
    check_probe(count_by_name(name), 0, False, monkeypatch)


def test_specialised_mandelbrot_equals_generic_and_oracle(monkeypatch, oracle):
    w, h = 256, 192
    want = oracle(w, h)
    clean(monkeypatch)
    generic = F.load("mandelbrot")
    assert "mm_fast" not in generic.kernel_source
    a = generic.invoke(w, h).render()
    assert int((a != want).sum()) == 0
    for label, flt in mandelbrots(monkeypatch):
        b = flt.invoke(w, h).render()
        assert int((a != b).sum()) == 0 and int((b != want).sum()) == 0, label
    assert len(np.unique(a[..., 0])) > 16          # the escape bands are there
