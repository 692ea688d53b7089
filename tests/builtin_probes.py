"""One probe filter per builtin overload id (mathmap_amd/csrc/builtins.cpp), for tests/test_builtin_reference.py (oracle
against the NumPy restatement of tests/builtin_reference.py) and tests/test_gpu_builtins.py (GPU against both).

A probe's arguments are built from per-pixel scalars s0, s1, ... = (term * u + u') * (diagonal * ug + uh) with terms in x and
y and float user values u, so the kernel evaluates the target at run time, 32 x 32 different argument sets per frame, and a
user-value set moves all of them to an edge: zeros, negative zeros, lattice points, 1e30 (products overflow, inf - inf is
NaN), 1e-30 (products are denormal or underflow) and, through the second factor, arguments that are +-inf and NaN
themselves (3e38 * term + 3e38 overflows, and inf * 0 is NaN where the diagonal term x - y or x + y is 0).  With ug = 0 and uh = 1 the second factor is exactly 1.  The result goes into rgba:[...] four elements at a time; a longer result takes several
filters.  Filter.builtin_ids proves that the text reached the id it names: overload resolution takes the first match."""
import numpy as np

from tests import builtin_reference as R

SIZE = 32
UV = ("ua", "ub", "uc", "ud", "ue", "uf", "ug", "uh")
HEAD = "filter probe (%s" + ", ".join("float %s: -4-4 (%s)" % (u, "1" if u == "uh" else "0" if u == "ug" else "0.5") for u in UV) + ")\n"

# (text, NumPy) of the per-pixel terms; scalar k is (TERMS[k % 6] * UV[MUL[k]] + UV[ADD[k]]) * (DIAGONAL[k % 2] * ug + uh)
TERMS = [("x", lambda x, y: x), ("y", lambda x, y: y), ("(x + y)", lambda x, y: x + y), ("(x - y)", lambda x, y: x - y),
         ("(x * y)", lambda x, y: x * y), ("(y * y - x)", lambda x, y: y * y - x)]
# zero on a diagonal of the frame; never the scalar's own term
DIAGONAL = [("(x - y)", lambda x, y: x - y), ("(x + y)", lambda x, y: x + y)]
NSCALARS = 20


def _mul_index(k):
    return (0, 2, 4)[(k // 6 + k) % 3]


def _add_index(k):
    return (1, 3, 5)[(k + k // 3) % 3]


def scalar_text(k):
    return "s%d = (%s * %s + %s) * (%s * ug + uh)" % (k, TERMS[k % 6][0], UV[_mul_index(k)], UV[_add_index(k)], DIAGONAL[k % 2][0])


def coordinates(size=SIZE):
    """x and y of every pixel of a size x size frame: pixel centres mapped to [-1, 1] in double, rounded to float"""
    c = ((np.arange(size) - (size - 1) / 2.0) / ((size - 1) / 2.0)).astype(np.float32)
    x, y = np.meshgrid(c, -c)
    return np.ascontiguousarray(x), np.ascontiguousarray(y)


def scalar_values(values, size=SIZE):
    """the arrays of s0 .. s19 for a user-value set (a tuple in UV's order), as the filter computes them in float32"""
    x, y = coordinates(size)
    v = [np.float32(u) for u in full_values(values)]
    with np.errstate(all="ignore"):
        return [((TERMS[k % 6][1](x, y) * v[_mul_index(k)] + v[_add_index(k)]) * (DIAGONAL[k % 2][1](x, y) * v[6] + v[7])).astype(np.float32)
                for k in range(NSCALARS)]


def full_values(values):
    """a set of six values with the second factor at exactly 1 (ug = 0, uh = 1), or a set of all eight"""
    return tuple(values) + (0.0, 1.0) if len(values) == 6 else tuple(values)


# user-value sets: (ua, ub, uc, ud, ue, uf), and (ug, uh) where they are not (0, 1)
SETS = {
    "generic": (1.0, 0.25, -0.75, 0.5, 2.0, -0.125),       # both signs, fractions, colours below 0 and above 1
    "zero": (0.0, 0.0, 0.0, 0.0, 0.0, 0.0),                # every argument +0 or -0 (x * 0 is -0 left of the centre)
    "negzero": (0.0, -0.0, 0.0, -0.0, 0.0, -0.0),          # -0 + -0 = -0, +0 + -0 = +0: divisors of either zero
    "equal": (1.0, 0.0, 1.0, 0.0, 1.0, 0.0),               # scalars of one term are equal; s0 = s1 on the diagonal
    "lattice": (15.5, 0.5, 15.5, 0.5, 15.5, 0.5),          # integers and halves: floor, ceil, %, hue sextants
    "grey": (0.0, 0.5, 0.0, 0.5, 0.0, 0.5),                # every scalar 0.5: grey colours, singular matrices
    "big": (1e30, 1e30, -1e30, 1e-30, 1e30, -1e-30),       # products overflow: inf, and NaN from inf - inf
    "tiny": (1e-30, -1e-30, 1e-30, 1e-30, -1e-30, 1e-30),  # products are denormal or 0
    # the arguments themselves: term * 3e38 + 3e38 is +inf right of term = 0.13 and finite left of it (-inf with uc, ud), times
    # the diagonal term: inf * 0 is NaN on the diagonal; the scalars multiplied by ue stay finite
    "nonfinite": (3e38, 3e38, -3e38, -3e38, 1.0, 0.25, 1.0, 0.0),
}


class Probe:
    def __init__(self, ident, args, call, nres, image=False, sets=None, same_as=None):
        """`args`: "tag:n" per argument ("nil:1": a plain scalar); `call`: the expression, {0} {1} ... the arguments;
        `nres`: elements of the result; `sets`: user-value sets of its own, name -> values (default: SETS);
        `same_as`: (id, call) -- another overload and an expression through it that must give the same bits"""
        self.id, self.args, self.call, self.nres, self.image = ident, args, call, nres, image
        self.sets = dict((k, full_values(v)) for k, v in (sets or SETS).items())
        self.same_as = same_as

    def arg_slices(self):
        out, k = [], 0
        for a in self.args:
            n = int(a.split(":")[1])
            out.append((a.split(":")[0], k, k + n))
            k += n
        assert k <= NSCALARS
        return out

    def texts(self, call=None):
        """[(filter text, the result elements its rgba holds)]; `call`: another expression in place of the probe's"""
        sl = self.arg_slices()
        nsc = max([hi for _, _, hi in sl] + [1])
        lines = ["  " + "; ".join(scalar_text(k) for k in range(nsc)) + ";"]
        names = []
        for i, (tag, lo, hi) in enumerate(sl):
            if tag == "nil" and hi - lo == 1:
                names.append("s%d" % lo)
            else:
                lines.append("  p%d = %s:[%s];" % (i, tag, ", ".join("s%d" % k for k in range(lo, hi))))
                names.append("p%d" % i)
        lines.append("  w = %s;" % (call or self.call).format(*names))
        out = []
        for first in range(0, self.nres, 4):
            idx = [min(first + j, self.nres - 1) for j in range(4)]
            elems = ["w" if self.nres == 1 else "w[%d]" % i for i in idx]
            head = HEAD % ("image in, " if self.image else "")
            out.append((head + "\n".join(lines) + "\n  rgba:[%s]\nend\n" % ", ".join(elems), idx))
        return out

    def arguments(self, values):
        s = scalar_values(values)
        return [s[lo:hi] for _, lo, hi in self.arg_slices()]


def _p(ident, args, call, nres, **kw):
    return Probe(ident, args.split(), call, nres, **kw)


PROBES = [
    _p("print", "nil:1", "print({0})", 1),
    _p("add_ri", "ri:2 ri:2", "{0} + {1}", 2), _p("add_ri_1", "ri:2 nil:1", "{0} + {1}", 2),
    _p("add_1_ri", "nil:1 ri:2", "{0} + {1}", 2), _p("add_1", "nil:1 nil:1", "{0} + {1}", 1),
    _p("add_s", "v3:3 nil:1", "{0} + {1}", 3), _p("add_n", "v3:3 v3:3", "{0} + {1}", 3),
    _p("sub_ri", "ri:2 ri:2", "{0} - {1}", 2), _p("sub_ri_1", "ri:2 nil:1", "{0} - {1}", 2),
    _p("sub_1_ri", "nil:1 ri:2", "{0} - {1}", 2), _p("sub_1", "nil:1 nil:1", "{0} - {1}", 1),
    _p("sub_s", "v3:3 nil:1", "{0} - {1}", 3), _p("sub_n", "v3:3 v3:3", "{0} - {1}", 3),
    _p("neg", "v3:3", "-{0}", 3),
    _p("mul_ri", "ri:2 ri:2", "{0} * {1}", 2), _p("mul_1_ri", "nil:1 ri:2", "{0} * {1}", 2),
    _p("mul_m2x2", "m2x2:4 m2x2:4", "{0} * {1}", 4), _p("mul_m3x3", "m3x3:9 m3x3:9", "{0} * {1}", 9),
    _p("mul_v2m2x2", "v2:2 m2x2:4", "{0} * {1}", 2), _p("mul_v3m3x3", "v3:3 m3x3:9", "{0} * {1}", 3),
    _p("mul_m2x2v2", "m2x2:4 v2:2", "{0} * {1}", 2), _p("mul_m3x3v3", "m3x3:9 v3:3", "{0} * {1}", 3),
    _p("mul_quat", "quat:4 quat:4", "{0} * {1}", 4), _p("mul_cquat", "cquat:4 cquat:4", "{0} * {1}", 4),
    _p("mul_hyper", "hyper:4 hyper:4", "{0} * {1}", 4),
    _p("mul_1", "nil:1 nil:1", "{0} * {1}", 1), _p("mul_s", "v3:3 nil:1", "{0} * {1}", 3), _p("mul_n", "v3:3 v3:3", "{0} * {1}", 3),
    _p("div_ri", "ri:2 ri:2", "{0} / {1}", 2), _p("div_1_ri", "nil:1 ri:2", "{0} / {1}", 2),
    _p("div_1", "nil:1 nil:1", "{0} / {1}", 1), _p("div_s", "v3:3 nil:1", "{0} / {1}", 3), _p("div_n", "v3:3 v3:3", "{0} / {1}", 3),
    _p("mod_1", "nil:1 nil:1", "{0} % {1}", 1), _p("mod_s", "v3:3 nil:1", "{0} % {1}", 3), _p("mod_n", "v3:3 v3:3", "{0} % {1}", 3),
    _p("pmod", "nil:1 nil:1", "pmod({0}, {1})", 1),
    _p("sqrt_1", "nil:1", "sqrt({0})", 1), _p("sum", "v3:3", "sum({0})", 1),
    _p("dotp", "v3:3 v3:3", "dotp({0}, {1})", 1), _p("crossp", "v3:3 v3:3", "crossp({0}, {1})", 3),
    _p("det_m2x2", "m2x2:4", "det({0})", 1), _p("det_m3x3", "m3x3:9", "det({0})", 1),
    _p("normalize", "v3:3", "normalize({0})", 3),
    _p("abs_ri", "ri:2", "abs({0})", 1), _p("abs_quat", "quat:4", "abs({0})", 1), _p("abs_cquat", "cquat:4", "abs({0})", 1),
    _p("abs_hyper", "hyper:4", "abs({0})", 1), _p("abs_v2", "v2:2", "abs({0})", 1), _p("abs_v3", "v3:3", "abs({0})", 1),
    _p("abs_1", "nil:1", "abs({0})", 1), _p("abs_n", "nil:3", "abs({0})", 3),
    _p("deg2rad", "nil:1", "deg2rad({0})", 1), _p("rad2deg", "nil:1", "rad2deg({0})", 1),
    _p("conj_ri", "ri:2", "conj({0})", 2),
    _p("floor", "nil:1", "floor({0})", 1), _p("ceil", "nil:1", "ceil({0})", 1), _p("sign_n", "v3:3", "sign({0})", 3),
    _p("min_n", "v3:3 v3:3", "min({0}, {1})", 3), _p("max_n", "v3:3 v3:3", "max({0}, {1})", 3),
    _p("clamp", "v3:3 v3:3 v3:3", "clamp({0}, {1}, {2})", 3),
    _p("lerp_1", "nil:1 v3:3 v3:3", "lerp({0}, {1}, {2})", 3), _p("lerp_n", "v3:3 v3:3 v3:3", "lerp({0}, {1}, {2})", 3),
    _p("scale", "v2:2 v2:2 v2:2 v2:2 v2:2", "scale({0}, {1}, {2}, {3}, {4})", 2),
    _p("not", "nil:1", "!{0}", 1), _p("or", "nil:1 nil:1", "{0} || {1}", 1), _p("and", "nil:1 nil:1", "{0} && {1}", 1),
    _p("xor", "nil:1 nil:1", "{0} xor {1}", 1),
    _p("equal_ri", "ri:2 ri:2", "{0} == {1}", 1), _p("equal_ri_1", "ri:2 nil:1", "{0} == {1}", 1),
    _p("equal_1_ri", "nil:1 ri:2", "{0} == {1}", 1), _p("equal", "nil:1 nil:1", "{0} == {1}", 1),
    _p("less", "nil:1 nil:1", "{0} < {1}", 1), _p("greater", "nil:1 nil:1", "{0} > {1}", 1),
    _p("lessequal", "nil:1 nil:1", "{0} <= {1}", 1), _p("greaterequal", "nil:1 nil:1", "{0} >= {1}", 1),
    _p("notequal", "nil:1 nil:1", "{0} != {1}", 1), _p("inintv", "nil:1 nil:1 nil:1", "inintv({0}, {1}, {2})", 1),
    _p("red", "rgba:4", "red({0})", 1), _p("green", "rgba:4", "green({0})", 1), _p("blue", "rgba:4", "blue({0})", 1),
    _p("alpha", "rgba:4", "alpha({0})", 1), _p("gray", "rgba:4", "gray({0})", 1),
    _p("rgbColor", "nil:1 nil:1 nil:1", "rgbColor({0}, {1}, {2})", 4),
    _p("rgbaColor", "nil:1 nil:1 nil:1 nil:1", "rgbaColor({0}, {1}, {2}, {3})", 4),
    _p("grayColor", "nil:1", "grayColor({0})", 4), _p("grayaColor", "nil:1 nil:1", "grayaColor({0}, {1})", 4),
    _p("toHSVA", "rgba:4", "toHSVA({0})", 4), _p("toRGBA", "hsva:4", "toRGBA({0})", 4),
    _p("toXY", "ra:2", "toXY({0})", 2), _p("toXY_trivial", "xy:2", "toXY({0})", 2),
    _p("toRA", "xy:2", "toRA({0})", 2), _p("toRA_trivial", "ra:2", "toRA({0})", 2),
    _p("asin", "nil:1", "asin({0})", 1), _p("acos", "nil:1", "acos({0})", 1), _p("log_1", "nil:1", "log({0})", 1),
    _p("pow_1", "nil:1 nil:1", "{0} ^ {1}", 1), _p("pow_s", "v3:3 nil:1", "{0} ^ {1}", 3),
    _p("asinh_1", "nil:1", "asinh({0})", 1), _p("acosh_1", "nil:1", "acosh({0})", 1), _p("atanh_1", "nil:1", "atanh({0})", 1),
    # beta, gamma and the complex Jacobi functions get sets of their own, inside the functions' domains: GSL is absent, so
    # what they give at poles (gamma(0), beta(0, b)), for m outside (0, 1) or for non-finite arguments is whatever the
    # restated algorithm does there -- the reference's value is not known, and scipy's is another library's choice.  The
    # guards the builtins put in front (negative arguments, a > 171) are inside the sets.
    _p("beta_1", "nil:1 nil:1", "beta({0}, {1})", 1, sets={"generic": SETS["generic"], "positive": (2.0, 2.5, 3.0, 3.5, 0.0, 0.0)}),
    # gamma(a) is 0 for a < 0 and for a > 171
    _p("gamma_1", "nil:1", "gamma({0})", 1, sets={"small": (3.0, 3.5, 0.0, 0.0, 0.0, 0.0), "wide": (100.0, 90.0, 0.0, 0.0, 0.0, 0.0)}),
    # a real exponent or base is the complex number with imaginary part 0
    _p("pow_ri_1", "ri:2 nil:1", "{0} ^ {1}", 2, same_as=("pow_ri", "{0} ^ ri:[{1}, 0]")),
    _p("pow_1_ri", "nil:1 ri:2", "{0} ^ {1}", 2, same_as=("pow_ri", "ri:[{0}, 0] ^ {1}")),
    # the parameter m = s2 stays inside (0, 1)
    _p("ell_jac_sn_ri", "ri:2 nil:1", "ell_jac_sn({0}, {1})", 2, sets={"unit": (1.5, 0.1, 1.0, -0.2, 0.2, 0.5)}),
    _p("ell_jac_dn_ri", "ri:2 nil:1", "ell_jac_dn({0}, {1})", 2, sets={"unit": (1.5, 0.1, 1.0, -0.2, 0.2, 0.5)}),
    # the size of the bound image in pixels: it has no scalar argument, so one set is all there is
    _p("pixelSize", "", "pixelSize(in)", 2, image=True, sets={"generic": SETS["generic"]}),
]
IMAGE_SIZE = (7, 5)      # width, height of the image bound to `in`

# The specialising JIT applies the reference's literal folds (x * 0 -> 0, x + 0 -> x, x - 0 -> x; specialize.cpp), which by
# design ignore the sign of a zero and a non-finite x.  In these sets a literal 0 meets such values, so the specialised kernel
# is held to the oracle's evaluation of the specialised IR alone; in every other set the folds are exact and it must also
# equal the generic oracle and the NumPy restatement.
INEXACT_FOLD_SETS = ("negzero", "nonfinite")

BY_ID = dict((p.id, p) for p in PROBES)
assert len(BY_ID) == len(PROBES)


def expected(probe, values):
    """the NumPy restatement's result elements for a user-value set"""
    if probe.id == "pixelSize":
        one = np.ones((SIZE, SIZE), np.float32)
        return [one * np.float32(IMAGE_SIZE[0]), one * np.float32(IMAGE_SIZE[1])]
    with np.errstate(all="ignore"):
        out = R.REF[probe.id](*probe.arguments(values))
    assert len(out) == probe.nres
    return [np.asarray(o, np.float32) for o in out]


def magnitude_of(probe, values, idx):
    if probe.id not in R.MAGNITUDE:
        return None
    with np.errstate(all="ignore"):
        m = R.MAGNITUDE[probe.id](*probe.arguments(values))
    return np.stack([np.asarray(m[i], np.float32) for i in idx], axis=-1)


def probe_image():
    w, h = IMAGE_SIZE
    return np.full((h, w, 4), 128, np.uint8)


def compare(ident, got, want, where, magnitude=None):
    """`got` against the restatement `want` (float32 arrays of one shape) under the id's bound; prints the figures first.
    `magnitude`: ulps are counted at max(|want|, magnitude) (builtin_reference.MAGNITUDE)"""
    nan_g, nan_w = np.isnan(got), np.isnan(want)
    same = (got.view(np.uint32) == want.view(np.uint32)) | (nan_g & nan_w)
    print("%s %s: %d of %d values differ, NaN %d / %d" % (ident, where, int((~same).sum()), same.size, int(nan_g.sum()), int(nan_w.sum())))
    assert np.array_equal(nan_g, nan_w), (ident, where, "NaN positions")
    if ident not in R.LIBM and ident not in R.GSL_ULPS:
        assert same.all(), (ident, where, int((~same).sum()), got[~same][:4], want[~same][:4])
        return
    assert np.array_equal(np.isinf(got), np.isinf(want)) and np.array_equal(got[np.isinf(got)], want[np.isinf(want)]), (ident, where)
    fin = np.isfinite(got)
    if not fin.any():
        return
    if magnitude is None:
        ulps = np.abs(got[fin].view(np.int32).astype(np.int64) - want[fin].view(np.int32).astype(np.int64))
    else:
        size = np.spacing(np.maximum(np.abs(want[fin]), magnitude[fin]).astype(np.float32)).astype(np.float64)
        ulps = np.abs(got[fin].astype(np.float64) - want[fin].astype(np.float64)) / size
    print("%s %s: max %g ulps, %.5f identical" % (ident, where, float(ulps.max()), float((ulps == 0).mean())))
    if ident in R.LIBM:
        assert ulps.max() <= 1 and (ulps == 0).mean() >= 0.999, (ident, where, int(ulps.max()))
    else:
        assert ulps.max() <= R.GSL_ULPS[ident], (ident, where, float(ulps.max()))


def uservals(values):
    """name -> float of a set, as both the oracle and the GPU take them"""
    return dict(zip(UV, [float(np.float32(v)) for v in full_values(values)]))


def same_bits(a, b):
    """NaN in the same places, the same bits everywhere else; returns the number of differing values"""
    if not np.array_equal(np.isnan(a), np.isnan(b)):
        return -1
    ok = ~np.isnan(a)
    return int((a[ok].view(np.uint32) != b[ok].view(np.uint32)).sum())
