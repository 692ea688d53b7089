"""mmhip_options.gauss_mode (include/mmhip.h) without a GPU: the field's place in the options struct, its default, its
way through every compile entry point, refusal of unknown values, and that it stays out of the kernel source."""
import ctypes as C

import pytest

import mathmap_amd as mm
from mathmap_amd._lib import Options, lib
from tests import filters as F

# the options layout before gauss_mode took the first reserved int
OLD_OFFSETS = {"intersample": 0, "supersampling": 4, "edge_behaviour_x": 8, "edge_behaviour_y": 12, "tile_w": 16,
               "specialize_uservals": 20, "pixel_inc": 24, "reserved": 28}
SCALED_BLUR = """
filter scaled_blur (image in, float s: 0-1 (0.02), float k: 0-2 (1))
  b = gaussian_blur(in, s * k, s);
  b(xy)
end
"""


def test_default_options_are_exact():
    o = Options()
    o.gauss_mode = 9
    lib().mmhip_default_options(C.byref(o))
    assert o.gauss_mode == 0
    assert mm.Filter(F.GAUSS_DIRECT).gauss_mode == "exact"


def test_options_layout_is_unchanged():
    assert C.sizeof(Options) == 52
    for name, off in OLD_OFFSETS.items():
        if name != "reserved":
            assert getattr(Options, name).offset == off, name
    assert Options.gauss_mode.offset == OLD_OFFSETS["reserved"]
    assert Options.reserved.offset + Options.reserved.size == C.sizeof(Options)


@pytest.mark.parametrize("mode", ["exact", "tolerance"])
def test_mode_survives_every_compile_path(mode):
    flt = mm.Filter(SCALED_BLUR, gauss_mode=mode)
    assert flt.gauss_mode == mode
    assert flt.specialized({"k": 0.5}).gauss_mode == mode                  # mmhip_filter_specialized, source origin
    assert mm.Filter(SCALED_BLUR, gauss_mode=mode, constants={"k": 0.5}).gauss_mode == mode
    from_ir = mm.Filter(ir_json=flt.ir_json_raw, gauss_mode=mode)           # mmhip_compile_ir_json
    assert from_ir.gauss_mode == mode
    assert from_ir.specialized({"k": 0.5}).gauss_mode == mode               # mmhip_filter_specialized, IR origin
    assert mm.Filter(ir_json=flt.ir_json_raw, gauss_mode=mode, constants={"k": 0.5}).gauss_mode == mode
    assert F.load("gaussian_blur", gauss_mode=mode).gauss_mode == mode      # the reference's example, from its IR


@pytest.mark.parametrize("bad", [2, -1, 100])
def test_unknown_mode_is_refused_by_the_library(bad):
    o = Options()
    lib().mmhip_default_options(C.byref(o))
    o.gauss_mode = bad
    assert not lib().mmhip_compile(F.GAUSS_DIRECT.encode(), C.byref(o))
    assert b"gauss_mode" in lib().mmhip_last_error()
    raw = mm.Filter(F.GAUSS_DIRECT).ir_json_raw
    assert not lib().mmhip_compile_ir_json(raw.encode(), C.byref(o))
    assert b"gauss_mode" in lib().mmhip_last_error()
    assert not lib().mmhip_compile_specialized(F.GAUSS_DIRECT.encode(), C.byref(o), 0, None, None)
    assert b"gauss_mode" in lib().mmhip_last_error()


def test_unknown_mode_is_refused_by_python():
    with pytest.raises(mm.MathMapError, match="gauss_mode"):
        mm.Filter(F.GAUSS_DIRECT, gauss_mode="fast")


@pytest.mark.parametrize("name", ["gauss_direct", "gaussian_blur", "closure_timed_arg"])
def test_mode_is_not_part_of_the_kernel_source(name):
    exact, tol = F.load(name), F.load(name, gauss_mode="tolerance")
    assert exact.kernel_source == tol.kernel_source
    assert exact.ir_json == tol.ir_json
