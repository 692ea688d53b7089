"""A NumPy restatement of what the language core means, written from the reference's text and never from this project's parser,
lowering or oracle: the frame's variables as new_template.c.in and compiler.c:2338-2511 compute them, the table reads of
opmacros.h:192-193, filter calls (exprtree.c:820-935, compiler.c:1709-1773, 2165-2220, 2422-2465, opmacros.h:199-216), and small
helpers for the arithmetic of generated C.  tests/language_probes.py writes one expectation per probe with these;
tests/test_language_reference.py holds the oracle to them and tests/test_gpu_language.py the GPU.  No tests in here.

The generated C in short (backends/cc.c, ops.lisp, opmacros.h:37-47): every operator result is stored in a variable of type int
or float before it is used again, so each step rounds to float32; a float literal is printed as the double of its float value
(ops.lisp:348 g_ascii_dtostr), and + - * / of two floats computed in double and rounded once is the float32 operation.  ADD, SUB,
MUL and NEG take the larger of their argument types (ops.lisp:119-122, compiler.c:2763-2783), an int meeting a float is
converted by C, `/` is `(float)a / (float)b` and `%` is fmod in double, both of type float (ops.lisp:123-124).  A variable has the
largest type ever assigned to it, everywhere (compiler.c:2811-2865).  A value that no path defined reads as 0 (backends/cc.c:71-77).
"""
import numpy as np

F = np.float32
CURVE_POINTS = 1024           # userval.h USER_CURVE_POINTS
FLAGS = ("default", "pixel", "stretched")
OPTION_TEXT = {"default": "", "pixel": "pixel ", "stretched": "stretched "}      # mathmap_common.c:59-72: options before `filter`


class Limits:
    """W, H, X, Y of a filter with these flags on a width x height canvas (compiler.c:2338-2403).  The canvas sizes reach the
    code as internals, which are float (compiler.c:2760-2761), so everything here is a float32."""

    def __init__(self, width, height, flags):
        w, h = F(width), F(height)
        if flags == "pixel":                 # case 0: W = __canvasPixelW, X = (W - 1) / 2
            self.W, self.H = w, h
            self.X, self.Y = F(w - F(1)) / F(2), F(h - F(1)) / F(2)
        elif flags == "stretched":           # IMAGE_FLAG_UNIT: the int constants 2 and 1
            self.W = self.H = F(2)
            self.X = self.Y = F(1)
        else:                                # UNIT | SQUARE: X = W / max(W, H), W = X * 2
            assert flags == "default"
            m = w if h < w else h            # OP_MAX is MAX(a, b) of the two sizes
            self.X, self.Y = w / m, h / m
            self.W, self.H = self.X * F(2), self.Y * F(2)
        # the factors resize_image_if_necessary wraps an image in for code with these flags (compiler.c:1715-1773); None: no wrapper
        if flags == "pixel":
            self.factors = (F(2) / w, F(2) / h)
        elif flags == "stretched":
            self.factors = None
        else:
            m = w if h < w else h
            self.factors = (m / w, m / h)


def virtual_coordinates(width, height):
    """CALC_VIRTUAL_X / CALC_VIRTUAL_Y (opmacros.h:156-157) of every column and row with sampling offset 0: computed in double,
    stored in `float x`, `float y` (new_template.c.in:245,260).  A size of 1 divides 0.0 by 0.0: NaN."""
    with np.errstate(all="ignore"):
        col, row = np.arange(width, dtype=np.float64), np.arange(height, dtype=np.float64)
        xs = ((col - (width - 1) / 2.0 + 0.0) / np.float64((width - 1) / 2.0)).astype(F)
        ys = ((-row + (height - 1) / 2.0 - 0.0) / np.float64((height - 1) / 2.0)).astype(F)
    return xs, ys


def polar(x, y):
    """r and a of float32 arrays x, y (compiler.c:2467-2511): r = hypot(x, y); a = 0 where r == 0, else acos(x / r) with the
    quotient stored as a float; where y < 0, the float constant 2 * M_PI minus a.  hypot and acos are double functions of the
    promoted floats; NumPy's stand in for glibc's."""
    with np.errstate(all="ignore"):
        r = np.hypot(x.astype(np.float64), y.astype(np.float64)).astype(F)
        q = (x / r).astype(F)
        a = np.where(r == 0, F(0), np.arccos(q.astype(np.float64)).astype(F)).astype(F)
        two_pi = np.float64(F(2 * np.pi))
        a = np.where(y < 0, (two_pi - a.astype(np.float64)).astype(F), a).astype(F)
    return r, a


class Frame:
    """The variables of one frame: arrays [height, width] x y r a, scalars t frame R W H X Y pi e, I = (0, 1)."""

    def __init__(self, width, height, flags="default", t=0.0, frame=0):
        self.width, self.height, self.flags = width, height, flags
        self.limits = lim = Limits(width, height, flags)
        xs, ys = virtual_coordinates(width, height)
        xv, yv = np.meshgrid(xs, ys)
        with np.errstate(all="ignore"):
            # compiler.c:2405-2420: x = the template's x times X
            self.x, self.y = (xv * lim.X).astype(F), (yv * lim.Y).astype(F)
        self.r, self.a = polar(self.x, self.y)
        self.t, self.frame = F(t), F(frame)                 # `float t`, `int frame` read into a float internal
        self.R = F(np.sqrt(2.0))                            # mathmap_common.c:770: image_R = sqrt(2.0), whatever the size
        self.W, self.H, self.X, self.Y = lim.W, lim.H, lim.X, lim.Y
        self.pi, self.e, self.I = F(np.pi), F(np.e), (F(0), F(1))      # macros.c:122-135


# ---- the arithmetic of one pixel, on float32 scalars --------------------------------------------------------------------------
def div(a, b):
    """`/`: the builtin gives 0 for a zero divisor, else DIV (opmacros.h:41)"""
    with np.errstate(all="ignore"):
        return F(0) if b == 0 else F(F(a) / F(b))


def mod(a, b):
    """`%`: 0 for a zero divisor, else fmod in double (opmacros.h:42); fmod is exact"""
    with np.errstate(all="ignore"):
        return F(0) if b == 0 else F(np.fmod(np.float64(a), np.float64(b)))


def power(a, b):
    """`^`: 0 for 0 ^ (b <= 0), else pow in double"""
    with np.errstate(all="ignore"):
        return F(0) if (b <= 0 and a == 0) else F(np.power(np.float64(a), np.float64(b)))


def truth(c):
    return F(1) if c else F(0)


def is_true(v):
    """C's `if (v)`: anything but zero, NaN included"""
    return not (v == 0)


def c_floor_int(v):
    """floor(): (int) of the double floor, for values inside int"""
    return int(np.floor(np.float64(v)))


def int_to_float(i):
    """an int stored in a float"""
    return F(np.int64(i))


# ---- table reads ------------------------------------------------------------------------------------------------------------
def table_index(p):
    """(int)(CLAMP01(p) * (USER_CURVE_POINTS - 1)) of opmacros.h:192-193 for a float32 array p.  CLAMP01 is MAX(0, MIN(1, p))
    (opmacros.h:128) with glib's macros, `a > b ? a : b` and `a < b ? a : b`; the product is float times int, a float32
    product, and the cast truncates.  A NaN passes through glib's MAX and MIN and its conversion to int is undefined in C (x86
    gives INT_MIN, an index far outside the table), so the reference states nothing for it; this project reads entry 0 there, in
    bounds, and that choice is what the index says for NaN."""
    p = np.asarray(p, F)
    with np.errstate(all="ignore"):
        m = np.where(F(1) < p, F(1), p)
        c = np.where(F(0) > m, F(0), m).astype(F)
        scaled = (c * F(CURVE_POINTS - 1)).astype(F)
    return np.where(np.isnan(scaled), 0, np.trunc(np.where(np.isnan(scaled), 0, scaled))).astype(np.int64)


def apply_curve(table, p):
    """APPLY_CURVE: table is float32 [1024]"""
    return np.asarray(table, F)[table_index(p)]


def apply_gradient(table, p):
    """APPLY_GRADIENT: table is uint32 [1024] of 0xRRGGBBAA; TUPLE_FROM_COLOR (opmacros.h:176-181) divides each byte by 255.0 in
    double and stores a float.  Returns the four channels."""
    c = np.asarray(table, np.uint32)[table_index(p)]
    return [(((c >> s) & 0xff).astype(np.float64) / 255.0).astype(F) for s in (24, 16, 8, 0)]


def color_channels(rgba):
    """A colour user value set from four floats in 0..1: MAKE_RGBA_COLOR_FLOAT (color.h:38, userval.c:596) truncates each
    channel times 255.0 to a byte, and reading it divides the byte by 255.0 (opmacros.h:147-150)."""
    return [F(np.float64(int(np.float64(F(v)) * 255.0) & 0xff) / 255.0) for v in rgba]


# ---- filter calls -------------------------------------------------------------------------------------------------------------
def callee_position(x, y, caller_limits, callee_limits, through=()):
    """The callee's x and y when a filter whose limits are `caller_limits` calls another with the position (x, y): the closure
    image is wrapped in the caller's resize factors (compiler.c:2218-2219), ORIG_VAL multiplies the position by them
    (opmacros.h:199-207), and the callee multiplies what it is given by its own X and Y (compiler.c:2405-2420, 2451-2457).
    `through`: the limits of filters that took the image as an argument before the call and re-wrapped it with their own factors
    (compiler.c:2444-2445) -- STRIP_RESIZE drops the earlier wrapper, so only the last one counts."""
    wrapper = through[-1] if through else caller_limits
    with np.errstate(all="ignore"):
        if wrapper.factors is not None:
            x, y = F(F(x) * wrapper.factors[0]), F(F(y) * wrapper.factors[1])
        return F(F(x) * callee_limits.X), F(F(y) * callee_limits.Y)
