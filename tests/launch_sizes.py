"""Frame sizes that put the pixel kernel's launch geometry at its edges, one table per kernel class.

The geometry (mmhip_filter_launch_geometry, runtime.cpp launch_geometry) picks the rows per work-item `ppt` from the
workgroup count at one row per work-item, wg1 = tiles_x * ceil(rows / tile_h): 1 below 8192, 2 from 8192, 4 from
32768, 8 from 131072 and 16 from 262144, rounded up to a multiple of MM_UNROLL.  The sizes below sit on both sides of
every cut, leave a partial last tile column and a partial last row group, put the workgroup count exactly on a whole
round of XCD order 2's swizzle and one past it, and take the cheap extreme shapes (one column, one row) that reach
ppt 16 with few pixels.  They are derived from the tile shape of the filter's kernel; tests/test_launch_geometry_table.py
checks that each really lands where its label says (without a GPU), tests/test_gpu_launch_geometry.py renders them.
"""

CUTS = (8192, 32768, 131072, 262144)

# one filter per kernel class: (name, how to build it, class check on the kernel source and geometry)
PAIR_XY = "filter pair_xy () rgba:[x, y, x * y, 1] end"
FLIP = "filter flip (image in) in(xy:[-x, y]) end"
WAVE = "filter wave (image in, float amp: 0-1 (0.1)) in(xy + xy:[sin(y * 10 + t * 6) * amp, 0]) end"
CLASSES = ("pair", "unroll1", "short_fetch", "medium_fetch", "row_slice", "single_pixel")


def class_filter(name, **opts):
    """The filter standing for kernel class `name`."""
    import mathmap_amd as mm
    from tests import filters as F
    if name == "pair":
        return mm.Filter(PAIR_XY, **opts)
    if name == "unroll1":
        return F.load("mandelbrot", **opts)       # generic (not specialised): the unroll-1 arithmetic kernel
    if name == "short_fetch":
        return mm.Filter(FLIP, **opts)
    if name == "medium_fetch":
        return F.load("pond", **opts)
    if name == "row_slice":
        return mm.Filter(WAVE, **opts)
    if name == "single_pixel":
        return F.load("droste", **opts)
    raise KeyError(name)


def class_errors(name, flt, geo):
    """Why `flt` (launch geometry `geo`) is not the class `name` stands for; empty when it is."""
    ks = flt.kernel_source
    tw = "#define MM_TILE_W %d\n" % geo["tile_w"]
    un = "#define MM_UNROLL %d\n" % geo["unroll"]
    pair = "mm_p += 2)" in ks
    single = "A.ppt is 1 for this kernel" in ks
    hot = "if (mm_hot) {" in ks
    rows = "mm_rows(mm_args" in ks
    want = {
        "pair": dict(tile_w=16, unroll=2, pair=True, single=False, hot=False, rows=False),
        "unroll1": dict(tile_w=16, unroll=1, pair=False, single=False, hot=False, rows=False),
        "short_fetch": dict(tile_w=64, unroll=4, pair=False, single=False, hot=True, rows=False),
        "medium_fetch": dict(tile_w=16, unroll=4, pair=False, single=False, hot=True, rows=False),
        "row_slice": dict(tile_w=64, unroll=4, pair=False, single=False, hot=True, rows=True),
        "single_pixel": dict(tile_w=16, unroll=1, pair=False, single=True, rows=False),
    }[name]
    got = dict(tile_w=geo["tile_w"], unroll=geo["unroll"], pair=pair, single=single, hot=hot, rows=rows)
    errs = ["%s: %s is %r, not %r" % (name, k, got[k], v) for k, v in want.items() if got[k] != v]
    if tw not in ks or un not in ks:
        errs.append("%s: the kernel source does not define the geometry's tile width / unroll" % name)
    if bool(geo["pair_mode"]) != pair or bool(geo["single_pixel"]) != single:
        errs.append("%s: geometry and kernel source disagree on pair / single-pixel mode" % name)
    return errs


def raw_ppt(wg1):
    return 16 if wg1 >= 262144 else 8 if wg1 >= 131072 else 4 if wg1 >= 32768 else 2 if wg1 >= 8192 else 1


def round_up(p, u):
    return (p + u - 1) // u * u


def _largest_divisor(n, limit):
    return max(d for d in range(1, min(n, limit) + 1) if n % d == 0)


def cut_sizes(tile_w, tile_h):
    """(label, w, h, wg1) on both sides of every ppt cut, each with a partial last row group.  At the two lower cuts the
    frames are wide (up to 128 tile columns, the last one partial); at the upper ones narrow -- one column of 3 pixels,
    or two tile columns the second of which has one pixel -- so that a frame stays below 20 M pixels."""
    out = []
    for c in CUTS:
        for wg1 in (c - 1, c):
            cols_limit = 128 if c <= 32768 else 2 if wg1 == 131072 else 1
            tx = _largest_divisor(wg1, cols_limit)
            w = 3 if tx == 1 else tile_w + 1 if tx == 2 else (tx - 1) * tile_w + max(1, tile_w // 2 - 3)
            h = wg1 // tx * tile_h - min(tile_h - 1, 3)
            out.append(("wg1_%d" % wg1, w, h, wg1))
    return out


def extreme_sizes(tile_w, tile_h):
    """One column of tile_h * 262144 rows (tiles_x = 1: plain division, no swizzle round) and one row of
    262145 tile columns, the last of them one pixel wide (each tile has one real row of tile_h * ppt;
    nwg * tiles_x >= 2^32: plain division)."""
    return [("one_column", 1, tile_h * 262144, 262144), ("one_row", tile_w * 262144 + 1, 1, 262145)]


def xcd_sizes(tile_w, tile_h, unroll, single_pixel=False):
    """(label, w, h, remainder): three tile columns (m = 2, rounds of 2^(m+3) = 32 workgroups) at ppt 4 (raw), the
    workgroup count a whole number of rounds (remainder 0) and one workgroup past one (remainder 1)."""
    tx, out = 3, []
    w = 2 * tile_w + 5
    for rem in (0, 1):
        ppt = 1 if single_pixel else round_up(4, unroll)
        ty = 2731 * 4 // ppt                          # tx * ceil(rows / tile_h) >= 32768 from here on
        while (tx * ty) % 32 != rem:
            ty += 1
        h = ty * tile_h * ppt - 1
        out.append(("xcd_rem%d" % rem, w, h, rem))
    return out


def frame_cases(geo_of):
    """Every size for the kernel whose launch geometry `geo_of(w, h)` gives (Filter.launch_geometry): [(label, w, h)]."""
    g = geo_of(64, 64)
    tw, th, unroll, single = g["tile_w"], g["tile_h"], g["unroll"], bool(g["single_pixel"])
    cases = [(lab, w, h) for lab, w, h, _ in cut_sizes(tw, th)]
    cases += [(lab, w, h) for lab, w, h, _ in extreme_sizes(tw, th)]
    cases += [(lab, w, h) for lab, w, h, _ in xcd_sizes(tw, th, unroll, single)]
    return cases


def expected(label, tile_w, tile_h, unroll, single_pixel):
    """What the geometry of the case `label` must show: a dict of field -> value (wg1, ppt, ...)."""
    want = {}
    for lab, w, h, wg1 in cut_sizes(tile_w, tile_h) + extreme_sizes(tile_w, tile_h):
        if lab == label:
            want["wg1"] = wg1
            want["ppt"] = 1 if single_pixel else round_up(raw_ppt(wg1), unroll)
    for lab, w, h, rem in xcd_sizes(tile_w, tile_h, unroll, single_pixel):
        if lab == label:
            want["xcd_rem"] = rem
    return want


def pixels(cases):
    return sum(w * h for _, w, h in cases)
