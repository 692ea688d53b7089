"""The size tables of tests/launch_sizes.py land where they claim (no GPU: compiling a filter and reading its launch
geometry needs none).  A geometry test that never reaches its geometry must fail here rather than pass on the GPU."""
import pytest

from tests import launch_sizes as L


@pytest.fixture(scope="module")
def classes():
    return {c: L.class_filter(c) for c in L.CLASSES}


@pytest.mark.parametrize("name", L.CLASSES)
def test_class_filter_is_its_kernel_class(name, classes):
    flt = classes[name]
    assert L.class_errors(name, flt, flt.launch_geometry(64, 64)) == []


@pytest.mark.parametrize("name", L.CLASSES)
def test_size_table_lands_in_its_buckets(name, classes):
    flt = classes[name]
    g0 = flt.launch_geometry(64, 64)
    tw, th, un, single = g0["tile_w"], g0["tile_h"], g0["unroll"], bool(g0["single_pixel"])
    ppts, rems = set(), set()
    for lab, w, h in L.frame_cases(flt.launch_geometry):
        g = flt.launch_geometry(w, h)
        want = L.expected(lab, tw, th, un, single)
        assert want, lab
        # the launch covers the frame: tiles_x whole tile columns, tiles_y groups of tile_h * ppt rows
        assert g["tiles_x"] == -(-w // tw) and g["tiles_y"] == -(-h // (th * g["ppt"])), (lab, g)
        assert g["nwg"] == g["tiles_x"] * g["tiles_y"] and g["ppt"] % un == 0, (lab, g)
        if "wg1" in want:
            assert (g["wg1"], g["ppt"]) == (want["wg1"], want["ppt"]), (lab, w, h, g)
        if "xcd_rem" in want:
            m = (max(g["tiles_x"] - 1, 1)).bit_length()
            assert g["nwg"] % (1 << (m + 3)) == want["xcd_rem"] and g["xcd_full"] == g["nwg"] - want["xcd_rem"], (lab, g)
            assert g["ppt"] == (1 if single else L.round_up(4, un)), (lab, g)
            rems.add(want["xcd_rem"])
        if lab.startswith("wg1_") and g["tiles_x"] > 1:
            assert w % tw != 0, (lab, "no partial last tile column")
        if lab.startswith("wg1_") and h > 1:
            assert h % (th * g["ppt"]) != 0, (lab, "rows a multiple of tile_h * ppt")
        if lab in ("one_column", "one_row"):
            assert g["tiles_magic"] == 0, (lab, g)     # tiles_x = 1, or nwg * tiles_x >= 2^32: the plain division
        ppts.add(g["ppt"])
    want_ppts = {1} if single else {L.round_up(p, un) for p in (1, 2, 4, 8, 16)}
    assert ppts == want_ppts, (name, sorted(ppts))
    assert rems == {0, 1}
    # the multiply-high division is taken somewhere too (every wide case)
    assert any(flt.launch_geometry(w, h)["tiles_magic"] for _, w, h in L.frame_cases(flt.launch_geometry))


def test_one_row_frame_is_past_the_magic_range(classes):
    g = classes["pair"].launch_geometry(*[(w, h) for lab, w, h in L.frame_cases(classes["pair"].launch_geometry)
                                           if lab == "one_row"][0])
    assert g["nwg"] * g["tiles_x"] >= 1 << 32 and g["ppt"] == 16 and g["tiles_y"] == 1


def test_forced_rows_per_item_is_what_the_launch_takes(classes, monkeypatch):
    """MMHIP_PPT is read where the launch reads it, rounded up to MM_UNROLL; the single-pixel kernel stays at 1."""
    for p in (1, 3, 5, 16):
        monkeypatch.setenv("MMHIP_PPT", str(p))
        for name, flt in classes.items():
            g = flt.launch_geometry(333, 251)
            assert g["ppt"] == (1 if g["single_pixel"] else L.round_up(p, g["unroll"])), (name, p, g)


def test_closure_launch_geometry():
    """The closure image of tests/test_gpu_closures.py's BLUR_OF_CLOSURE: its own launch at the band test's frame size
    reaches ppt >= 4 (tests/test_gpu_launch_geometry.py)."""
    import mathmap_amd as mm
    from tests.test_gpu_closures import BLUR_OF_CLOSURE
    from tests.test_gpu_launch_geometry import CLOSURE_FRAME
    flt = mm.Filter(BLUR_OF_CLOSURE)
    assert flt.num_closures == 1
    g = flt.launch_geometry(*CLOSURE_FRAME, closure=0)
    assert g["ppt"] >= 4, g
    with pytest.raises(mm.MathMapError):
        flt.launch_geometry(64, 64, closure=1)


def test_geometry_table_exercised_in_the_gpu_suite():
    """The GPU module renders every class but the single-pixel one (tests/test_gpu_baseline_sizes.py's Droste)."""
    from tests import test_gpu_launch_geometry as G
    assert set(G.FRAME_CLASSES) == set(L.CLASSES) - {"single_pixel"}
