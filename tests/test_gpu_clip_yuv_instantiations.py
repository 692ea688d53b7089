"""Every instantiation of the four 4:2:0 converter kernels on the GPU: k_rgba8_to_yuv420_clip (8), k_float_to_yuv420p10_clip
(12), k_yuv420_to_rgba_clip (12) and k_yuv420p10_to_float_clip (24) -- each converter at centre and left siting (the input
pair in replicate mode too), on its aligned and on its per-block path, under every value of its environment knobs.

The yardstick is tests/yuv_sited_reference.py (with "center" the restatements of the four converter tests).  Everything is
compared bit for bit in whole sentinel-filled destination buffers.  Two frames a case, so the frame stride is used:
  24 x 5  the aligned path: three work-items a row pair at 8 columns, six at 4, twelve at 2 -- a first one whose left column
          clamps, a middle one, a last one whose right chroma column clamps; the last row pair has one row; packed frames of
          192 and 384 bytes keep every alignment
  7 x 3   the per-block path: the last block has one column and one row, with neighbours on both sides"""
import functools

import numpy as np
import pytest

from tests import test_gpu_clip_yuv_sited as T
from tests.test_gpu_clip_yuv_sited import inv  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu
MODE = ("bt709", "limited")
SHAPES = {"aligned": (24, 5), "block": (7, 3)}
FRAMES = 2
# direction, depth -> the knobs of the converter and every value the launcher tells apart
KNOBS = {("out", 8): {"MMHIP_YUV_LOADS": ("cached", "nt")},
         ("out", 10): {"MMHIP_YUV10_COLUMNS": ("4", "8"), "MMHIP_YUV10_LOADS": ("cached", "nt")},
         ("in", 8): {"MMHIP_YUV_IN_STORES": ("cached", "nt")},
         ("in", 10): {"MMHIP_YUV10_IN_COLUMNS": ("2", "4", "8"), "MMHIP_YUV10_IN_STORES": ("cached", "nt")}}
# what the chroma is: (chroma mode of the input pair, siting)
CHROMAS = {"out": (("bilinear", "center"), ("bilinear", "left")), "in": (("bilinear", "center"), ("bilinear", "left"), ("replicate", "left"))}


def settings(knobs):
    """Every combination of the knobs' values, as tuples of (name, value)."""
    combos = [()]
    for name, values in knobs.items():
        combos = [c + ((name, v),) for c in combos for v in values]
    return combos


CASES = [(direction, depth, chroma, siting, path, combo)
         for (direction, depth), knobs in KNOBS.items() for chroma, siting in CHROMAS[direction] for path in SHAPES for combo in settings(knobs)]


def case_id(case):
    direction, depth, chroma, siting, path, combo = case
    return "-".join([direction + str(depth), "replicate" if chroma == "replicate" else siting, path] + [v for _, v in combo])


@functools.lru_cache(maxsize=None)
def source(direction, depth, path):
    w, h = SHAPES[path]
    return (T.random_clip if direction == "out" else T.random_payloads)(depth, FRAMES, w, h, 31 * w + h + depth)


@functools.lru_cache(maxsize=None)
def expected(direction, depth, chroma, siting, path):
    """The restatement's whole destination buffer: computed once per (converter, chroma, shape), shared by the knob cases."""
    w, h = SHAPES[path]
    data = source(direction, depth, path)
    frames = T.out_frames(depth, data, MODE, siting) if direction == "out" else T.in_frames(depth, data, w, h, MODE, chroma, siting)
    want = T.in_whole(frames)
    want.setflags(write=False)
    return want


def test_the_cases_reach_every_instantiation():
    """Counted from the knobs: aligned instantiations per knob setting, per-block ones per setting of the load or store knob
    alone (the column knob picks no other kernel there)."""
    reached = set()
    for direction, depth, chroma, siting, path, combo in CASES:
        flavour = tuple(v for name, v in combo if not name.endswith("COLUMNS"))
        columns = tuple(v for name, v in combo if name.endswith("COLUMNS")) if path == "aligned" else ()
        sited = "center" if chroma == "replicate" else siting      # replicate mode ignores the siting
        reached.add((direction, depth, chroma, sited, path, columns, flavour))
    count = {key: sum(1 for r in reached if r[:2] == key) for key in KNOBS}
    assert count == {("out", 8): 8, ("out", 10): 12, ("in", 8): 12, ("in", 10): 24}


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_every_instantiation_equals_the_restatement(inv, monkeypatch, case):  # noqa: F811
    direction, depth, chroma, siting, path, combo = case
    for name, value in combo:
        monkeypatch.setenv(name, value)
    w, h = SHAPES[path]
    data = source(direction, depth, path)
    before = T.launches(inv)
    if direction == "out":
        got = T.convert_out(inv, depth, data, MODE, siting=siting)
    else:
        got = T.convert_in(inv, depth, data, w, h, MODE, chroma, siting=siting)
    assert np.array_equal(got, expected(direction, depth, chroma, siting, path)), case_id(case)
    if (direction, depth) != ("out", 8):      # (the RGBA8 out converter has no launch counter)
        assert T.moved(before, T.launches(inv), (direction, depth)) == ((1, 0) if path == "aligned" else (0, 1)), case_id(case)
