"""An independent restatement of the builtin library (mathmap_amd/csrc/builtins.cpp) in NumPy.

One function per overload id whose semantics are plain arithmetic, written from the definition of the operation in
np.float32: one rounding per operation, no fused multiply-add, sums folded from the left, the guards the language
defines (a zero divisor gives 0, ...).  An argument is a list of float32 arrays, one per tuple element; so is the result.
The oracle cannot play this part: it evaluates the IR the front end produced, so a wrong overload is wrong on both sides
of every HIP-vs-oracle comparison.  tests/builtin_probes.py holds the filter text that reaches each id.

Number formats: every literal of a builtin is a float32 (or an int, promoted to float32 where it meets one); `floor` and
`ceil` yield a C int, which the conversion of an x86 (cvttsd2si) makes INT_MIN for NaN and everything outside int;
MIN(a, b) is a < b ? a : b and MAX(a, b) is a < b ? b : a, which decides what a NaN operand gives.

REF: id -> function.  LIBM: the ids of REF that call the C library (hypot, acos, sin, cos, ...): NumPy's double function
is not glibc's, so they are held to 1 ulp and 99.9 % identical values instead of equality.
COVERED_ELSEWHERE: id -> the existing test that exercises it, for builtins that are a library function (real and complex
libm, GSL, rand, the image operations, noise); EVIDENCE gives for each an expression quoted from that test's file and a
filter around it, which tests/test_builtin_reference.py compiles to prove that the expression reaches the id."""
import numpy as np

F = np.float32
PI_F = F(np.pi)


def _f(x):
    return np.asarray(x, dtype=np.float32)


def _lit(c, like):
    return np.full(like.shape, c, np.float32)


def _sum(terms):
    acc = terms[0]
    for t in terms[1:]:
        acc = acc + t
    return acc


def _min(a, b):
    return np.where(a < b, a, b)


def _max(a, b):
    return np.where(a < b, b, a)


def _clamp01(x):
    return _max(_lit(0, x), _min(_lit(1, x), x))


def _guard_zero(cond, value):
    """value where cond is false, 0 where it is true"""
    return np.where(cond, F(0), value).astype(np.float32)


def _c_int(d):
    """(int) of a double on x86-64, as a float32: NaN and anything outside int give INT_MIN"""
    d = np.asarray(d, np.float64)
    ok = np.isfinite(d) & (d > -2147483649.0) & (d < 2147483648.0)
    i = np.where(ok, np.trunc(np.where(ok, d, 0.0)), -2147483648.0)
    return i.astype(np.int64).astype(np.float32)


def _elementwise(op):
    return lambda a, b: [op(p, q) for p, q in zip(a, b)]


def _with_scalar(op):
    return lambda a, b: [op(p, b[0]) for p in a]


def _add(p, q):
    return p + q


def _sub(p, q):
    return p - q


def _mul(p, q):
    return p * q


def _div(p, q):
    return _guard_zero(q == 0, p / q)


def _mod(p, q):
    # fmod is exact, so the double fmod of two floats is a float
    return _guard_zero(q == 0, np.fmod(p.astype(np.float64), q.astype(np.float64)).astype(np.float32))


def _div_all(a, b):
    return [_guard_zero(b[0] == 0, p / b[0]) for p in a]


def _mod_all(a, b):
    return [_mod(p, b[0]) for p in a]


def _matmul(n):
    def f(a, b):
        return [_sum([a[i * n + k] * b[k * n + j] for k in range(n)]) for i in range(n) for j in range(n)]
    return f


def _vecmat(n):
    # row vector times matrix: result[i] = sum_j v[j] * M[j][i]
    return lambda v, m: [_sum([v[j] * m[j * n + i] for j in range(n)]) for i in range(n)]


def _matvec(n):
    # matrix times column vector: result[i] = sum_j M[i][j] * v[j]
    return lambda m, v: [_sum([m[i * n + j] * v[j] for j in range(n)]) for i in range(n)]


def _algebra(sign):
    """A four-dimensional algebra over the basis (1, i, j, k) in which e_p * e_q = sign[p][q] * e_(p xor q).  Component r
    of a product collects its four terms in the order the language's definition writes them: a_0 b_r first, a_r b_0
    second (for r > 0), then the other two by ascending left index; a negative term is the negated product."""
    def f(a, b):
        out = []
        for r in range(4):
            pairs = [(p, p ^ r) for p in range(4)]
            order = sorted(pairs, key=lambda pq: (0 if pq[0] == 0 else 1 if pq[1] == 0 else 2, pq[0]))
            terms = []
            for p, q in order:
                prod = a[p] * b[q]
                terms.append(-prod if sign[p][q] < 0 else prod)
            out.append(_sum(terms))
        return out
    return f


# quaternions: i i = j j = k k = -1, i j = k, j k = i, k i = j, and the reversed products negated
QUAT = [[1, 1, 1, 1], [1, -1, 1, -1], [1, -1, -1, 1], [1, 1, -1, -1]]
# hypercomplex numbers, commutative: i i = j j = -1, k = i j, hence k k = 1, i k = -j, j k = -i
HYPER = [[1, 1, 1, 1], [1, -1, 1, -1], [1, 1, -1, -1], [1, -1, -1, 1]]
# cquat, commutative, as the language defines it: i i = -1, j j = k k = 1, i j = -k, i k = -j, j k = i
CQUAT = [[1, 1, 1, 1], [1, -1, -1, -1], [1, -1, 1, 1], [1, -1, 1, 1]]


def _norm(a):
    return [np.sqrt(_sum([p * p for p in a]))]


def _div_ri(a, b):
    c = b[0] * b[0] + b[1] * b[1]
    zero = (b[0] == 0) & (b[1] == 0)
    re = (a[0] * b[0] + a[1] * b[1]) / c
    im = ((-a[0]) * b[1] + b[0] * a[1]) / c
    return [_guard_zero(zero, re), _guard_zero(zero, im)]


def _div_1_ri(a, b):
    c = b[0] * b[0] + b[1] * b[1]
    return [_guard_zero(c == 0, (a[0] * b[0]) / c), _guard_zero(c == 0, -((a[0] * b[1]) / c))]


def _pmod(a, b):
    m = np.fmod(a[0].astype(np.float64), b[0].astype(np.float64)).astype(np.float32)      # no guard: x % 0 is NaN
    return [np.where(a[0] < 0, m + b[0], m)]


def _det3(a):
    m = a[0]
    pos = (m[0] * m[4]) * m[8] + (m[1] * m[5]) * m[6] + (m[2] * m[3]) * m[7]
    neg = (m[2] * m[4]) * m[6] + (m[0] * m[5]) * m[7] + (m[1] * m[3]) * m[8]
    return [pos - neg]


def _normalize(a):
    l = _sum([p * p for p in a])
    return [_guard_zero(l == 0, p / np.sqrt(l)) for p in a]


def _sign(a):
    return [np.where(p < 0, F(-1), np.where(0 < p, F(1), F(0))) for p in a]


def _clamp(a, lo, hi):
    return [np.where(p < l, l, np.where(u < p, u, p)) for p, l, u in zip(a, lo, hi)]


def _lerp_1(p, a, b):
    l = F(1) - p[0]
    return [l * u + p[0] * v for u, v in zip(a, b)]


def _lerp_n(p, a, b):
    return [(F(1) - w) * u + w * v for w, u, v in zip(p, a, b)]


def _scale(a, fl, fu, tl, tu):
    out = []
    for p, l, u, m, n in zip(a, fl, fu, tl, tu):
        d = u - l
        out.append(_guard_zero(d == 0, ((p - l) / d) * (n - m) + m))
    return out


def _bool(c):
    return [np.where(c, F(1), F(0))]


def _to_hsva(c):
    r, g, b = _clamp01(c[0]), _clamp01(c[1]), _clamp01(c[2])
    alpha = _clamp01(c[3])
    mx = _max(r, _max(g, b))
    mn = _min(r, _min(g, b))
    delta = mx - mn
    h = np.where(r == mx, (g - b) / delta, np.where(g == mx, F(2) + (b - r) / delta, F(4) + (r - g) / delta))
    h = h / F(6)
    h = np.where(h < 0, h + F(1), h)
    return [_guard_zero(mx == 0, h), _guard_zero(mx == 0, delta / mx), mx, alpha]


def _to_rgba(c):
    s, v = _clamp01(c[1]), _clamp01(c[2])
    alpha = _clamp01(c[3])
    h = _max(_lit(0, c[0]), c[0])
    h = np.where(F(1) <= h, F(0), h * F(6))
    i = _c_int(np.floor(h.astype(np.float64)))
    f = h - i
    p = v * (F(1) - s)
    q = v * (F(1) - s * f)
    t = v * (F(1) - s * (F(1) - f))
    sextants = [(v, t, p), (q, v, p), (p, v, t), (p, q, v), (t, p, v)]
    out = []
    for ch in range(3):
        acc = (v, p, q)[ch]
        for k in range(4, -1, -1):
            acc = np.where(i == k, sextants[k][ch], acc)
        out.append(np.where(s == 0, v, acc))
    return out + [alpha]


def _to_xy(p):
    r, a = p[0], p[1].astype(np.float64)
    return [np.cos(a).astype(np.float32) * r, np.sin(a).astype(np.float32) * r]


def _to_ra(p):
    r = np.hypot(p[0].astype(np.float64), p[1].astype(np.float64)).astype(np.float32)
    a = np.arccos((p[0] / r).astype(np.float64)).astype(np.float32)
    ang = np.where(p[1] < 0, F(2) * PI_F - a, a)
    return [_guard_zero(r == 0, r), _guard_zero(r == 0, ang)]


def _libm1(fn, guard=None):
    def f(a):
        v = fn(a[0].astype(np.float64)).astype(np.float32)
        return [v if guard is None else _guard_zero(guard(a[0]), v)]
    return f


def _pow(p, q):
    return _guard_zero((q <= 0) & (p == 0), np.power(p.astype(np.float64), q.astype(np.float64)).astype(np.float32))


def _beta(a, b):
    from scipy.special import beta
    v = beta(a[0].astype(np.float64), b[0].astype(np.float64)).astype(np.float32)
    return [_guard_zero((a[0] < 0) | (b[0] < 0), v)]


def _gamma(a):
    from scipy.special import gamma
    v = gamma(a[0].astype(np.float64)).astype(np.float32)
    return [_guard_zero((a[0] < 0) | (a[0] > F(171.0)), v)]


def _jacobi_ri(which, magnitude=False):
    """sn, cn, dn of u = u0 + i u1 with parameter m from the real functions at (u0, m) and (u1, 1 - m), by the
    expressions the language defines (its dn is that expression, not the textbook's).  `magnitude`: not the elements but
    the sum of the absolute values of each numerator's terms over the denominator -- the imaginary part of dn is a
    difference, and where it cancels the error of its terms is what remains."""
    def f(u, m):
        from scipy.special import ellipj
        m32 = m[0]
        s, c, d, _ = ellipj(u[0].astype(np.float64), m32.astype(np.float64))
        s1, c1, d1, _ = ellipj(u[1].astype(np.float64), (F(1) - m32).astype(np.float64))
        mm_ = m32.astype(np.float64)
        denom = c1 * c1 + mm_ * ((s * s) * (s1 * s1))
        if which == "sn":
            re, im = s * d1, (c * d) * (s1 * c1)
        else:
            re, im = c1 * (d * d1), (s * s1) - (mm_ * c)
            if magnitude:
                re, im = np.abs(re), np.abs(s * s1) + np.abs(mm_ * c)
        return [(re / denom).astype(np.float32), (im / denom).astype(np.float32)]
    return f


REF = {
    "print": lambda a: [_lit(0, a[0])],
    "add_ri": _elementwise(_add),
    "add_ri_1": lambda a, b: [a[0] + b[0], a[1] + F(0)],
    "add_1_ri": lambda a, b: [b[0] + a[0], b[1] + F(0)],
    "add_1": _elementwise(_add), "add_s": _with_scalar(_add), "add_n": _elementwise(_add),
    "sub_ri": _elementwise(_sub),
    "sub_ri_1": lambda a, b: [a[0] - b[0], a[1] - F(0)],
    "sub_1_ri": lambda a, b: [a[0] - b[0], F(0) - b[1]],
    "sub_1": _elementwise(_sub), "sub_s": _with_scalar(_sub), "sub_n": _elementwise(_sub),
    "neg": lambda a: [-p for p in a],
    "mul_ri": lambda a, b: [a[0] * b[0] - a[1] * b[1], a[0] * b[1] + b[0] * a[1]],
    "mul_1_ri": lambda a, b: [a[0] * b[0], a[0] * b[1]],
    "mul_m2x2": _matmul(2), "mul_m3x3": _matmul(3),
    "mul_v2m2x2": _vecmat(2), "mul_v3m3x3": _vecmat(3),
    "mul_m2x2v2": _matvec(2), "mul_m3x3v3": _matvec(3),
    "mul_quat": _algebra(QUAT), "mul_cquat": _algebra(CQUAT), "mul_hyper": _algebra(HYPER),
    "mul_1": _elementwise(_mul), "mul_s": _with_scalar(_mul), "mul_n": _elementwise(_mul),
    "div_ri": _div_ri, "div_1_ri": _div_1_ri,
    "div_1": _elementwise(_div), "div_s": _div_all, "div_n": _elementwise(_div),
    "mod_1": _elementwise(_mod), "mod_s": _mod_all, "mod_n": _elementwise(_mod),
    "pmod": _pmod,
    "sqrt_1": lambda a: [np.sqrt(a[0])],
    "sum": lambda a: [_sum(a)],
    "dotp": lambda a, b: [_sum([p * q for p, q in zip(a, b)])],
    "crossp": lambda a, b: [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]],
    "det_m2x2": lambda m: [m[0] * m[3] - m[1] * m[2]],
    "det_m3x3": lambda m: _det3([m]),
    "normalize": _normalize,
    "abs_ri": lambda a: [np.hypot(a[0].astype(np.float64), a[1].astype(np.float64)).astype(np.float32)],
    "abs_quat": _norm, "abs_cquat": _norm, "abs_hyper": _norm, "abs_v2": _norm, "abs_v3": _norm,
    "abs_1": lambda a: [np.abs(a[0])], "abs_n": lambda a: [np.abs(p) for p in a],
    "deg2rad": lambda a: [a[0] * F(np.pi / 180.0)],
    "rad2deg": lambda a: [a[0] * F(180.0 / np.pi)],
    "conj_ri": lambda a: [a[0], -a[1]],
    "floor": lambda a: [_c_int(np.floor(a[0].astype(np.float64)))],
    "ceil": lambda a: [_c_int(np.ceil(a[0].astype(np.float64)))],
    "sign_n": _sign,
    "min_n": _elementwise(_min), "max_n": _elementwise(_max),
    "clamp": _clamp, "lerp_1": _lerp_1, "lerp_n": _lerp_n, "scale": _scale,
    "not": lambda a: _bool(a[0] == 0),
    "or": lambda a, b: _bool(~((a[0] == 0) & (b[0] == 0))),
    "and": lambda a, b: _bool(~((a[0] == 0) | (b[0] == 0))),
    "xor": lambda a, b: _bool((a[0] != 0) != (b[0] != 0)),
    "equal_ri": lambda a, b: _bool((a[0] == b[0]) & (a[1] == b[1])),
    "equal_ri_1": lambda a, b: _bool((a[0] == b[0]) & (a[1] == 0)),
    "equal_1_ri": lambda a, b: _bool((b[0] == a[0]) & (b[1] == 0)),
    "equal": lambda a, b: _bool(a[0] == b[0]),
    "less": lambda a, b: _bool(a[0] < b[0]),
    "greater": lambda a, b: _bool(b[0] < a[0]),
    "lessequal": lambda a, b: _bool(a[0] <= b[0]),
    "greaterequal": lambda a, b: _bool(b[0] <= a[0]),
    "notequal": lambda a, b: _bool(~(a[0] == b[0])),
    "inintv": lambda a, lo, hi: _bool((lo[0] <= a[0]) & (a[0] <= hi[0])),
    "red": lambda c: [c[0]], "green": lambda c: [c[1]], "blue": lambda c: [c[2]], "alpha": lambda c: [c[3]],
    "gray": lambda c: [F(0.299) * c[0] + F(0.587) * c[1] + F(0.114) * c[2]],
    "rgbColor": lambda r, g, b: [r[0], g[0], b[0], _lit(1, r[0])],
    "rgbaColor": lambda r, g, b, a: [r[0], g[0], b[0], a[0]],
    "grayColor": lambda g: [g[0], g[0], g[0], _lit(1, g[0])],
    "grayaColor": lambda g, a: [g[0], g[0], g[0], a[0]],
    "toHSVA": _to_hsva, "toRGBA": _to_rgba,
    "toXY": _to_xy, "toXY_trivial": lambda a: list(a),
    "toRA": _to_ra, "toRA_trivial": lambda a: list(a),
    # a guard in front of a C library function: the guard is the builtin's own
    "asin": _libm1(np.arcsin, lambda v: (v < -1) | (1 < v)),
    "acos": _libm1(np.arccos, lambda v: (v < -1) | (1 < v)),
    "log_1": _libm1(np.log, lambda v: v <= 0),
    "pow_1": lambda a, b: [_pow(a[0], b[0])],
    "pow_s": lambda a, b: [_pow(p, b[0]) for p in a],
    "asinh_1": _libm1(np.arcsinh), "acosh_1": _libm1(np.arccosh), "atanh_1": _libm1(np.arctanh),
    "beta_1": _beta, "gamma_1": _gamma,
    "ell_jac_sn_ri": _jacobi_ri("sn"), "ell_jac_dn_ri": _jacobi_ri("dn"),
    "pixelSize": None,      # the bound image's size: tests/builtin_probes.py IMAGE_SIZE
}

LIBM = {"abs_ri", "toXY", "toRA", "asin", "acos", "log_1", "pow_1", "pow_s", "asinh_1", "acosh_1", "atanh_1"}
# restated GSL special functions: the bound test_gsl_operators_match_restatement gives a real function of this kind
# (ell_int_Kcomp and its like: 4 ulps; the complex Jacobi functions: 16)
GSL_ULPS = {"beta_1": 4, "gamma_1": 4, "ell_jac_sn_ri": 16, "ell_jac_dn_ri": 16}
# Where an element is a sum of terms, the bound counts ulps of the terms' magnitude: every sn, cn, dn that goes in is the
# float result of the restated gsl_sf_elljac_e, itself within 4 ulps.
MAGNITUDE = {"ell_jac_dn_ri": _jacobi_ri("dn", magnitude=True)}
# held to another overload's bits by tests/builtin_probes.py (Probe.same_as), which an existing test holds to glibc's
SAME_AS = {"pow_ri_1", "pow_1_ri"}

_REAL = "tests/test_gpu_parity.py::test_real_math_float_ulps"
_CPLX = "tests/test_gpu_parity.py::test_complex_math_float_ulps"
_GSL = "tests/test_gpu_parity.py::test_gsl_operators_match_restatement"
_NOISE = "tests/test_gpu_noise_float.py::test_noise_equals_libnoise_float_for_float"

COVERED_ELSEWHERE = {}
# id -> (an expression the named test runs, a filter holding it, the file the expression stands in, the link to that file)
EVIDENCE = {}


def _cover(test, entries, body, where=None, link=None, head="filter e (image in, float k: 0-2 (1))"):
    """`where`: the file that holds the expression, where that is not the test's own, and `link`: the name by which the test
    takes the filter from that file"""
    for ident, expr in entries:
        COVERED_ELSEWHERE[ident] = test
        EVIDENCE[ident] = (expr, "%s %s end" % (head, body % expr), where or test.split("::")[0], link)


_cover(_REAL, [("sin", "sin(u*7)"), ("cos", "cos(v*7)"), ("tan", "tan(u)"), ("atan", "atan(u*9)"), ("atan2", "atan(u*9, v*9)"),
               ("exp_1", "exp(u*3)"), ("sinh_1", "sinh(u*2)"), ("cosh_1", "cosh(v*2)"), ("tanh_1", "tanh(u*2)")],
       "u = x; v = y; w = %s; grayColor(w)")
_cover(_CPLX, [("exp_ri", "exp(z)"), ("log_ri", "log(z)"), ("sqrt_ri", "sqrt(z)"), ("sin_ri", "sin(z)"), ("cos_ri", "cos(z)"),
               ("tan_ri", "tan(z)"), ("pow_ri", "z^ri:[1.3,0.4]"), ("sinh_ri", "sinh(z)"), ("cosh_ri", "cosh(z)"),
               ("tanh_ri", "tanh(z)"), ("asin_ri", "asin(z)"), ("acos_ri", "acos(z)"), ("atan_ri", "atan(z)"),
               ("asinh_ri", "asinh(z)"), ("acosh_ri", "acosh(z)"), ("atanh_ri", "atanh(z)"), ("gamma_ri", "gamma(z)")],
       "z = ri:[x, y]; w = %s; rgba:[w[0], w[1], 0, 1]")
_cover(_CPLX, [("arg_ri", "arg(z)")], "z = ri:[x, y]; w = %s; grayColor(w)")
_cover(_GSL, [("div_v2m2x2", "v2:[x + 2, y - 1] / m2x2:[x + 2.5, y, 0.3, y + 1.5]"),
              ("div_v3m3x3", "v3:[x, y, 1] / m3x3:[2 + x, y, 0.1, 0.3, 1.5 + y, x, 0.2, 0.1, 3]")],
       "q = %s; rgba:[q[0], q[1], 0, 1]")
_cover(_GSL, [("ell_jac_sn_1", "ell_jac_sn(x * 3, 0.5)"), ("ell_jac_cn_1", "ell_jac_cn(y * 3, 0.3)"),
              ("ell_jac_dn_1", "ell_jac_dn(x * y * 4, 0.8)"), ("ell_int_Kcomp", "ell_int_Kcomp(x * 0.99)"),
              ("ell_int_Ecomp", "ell_int_Ecomp(y * 0.99)"), ("ell_int_F", "ell_int_F(y * 4, x * 0.9)"),
              ("ell_int_E", "ell_int_E(y * 4, x * 0.9)"), ("ell_int_P", "ell_int_P(y * 4, x * 0.9, 0.3)"),
              ("ell_int_D", "ell_int_D(y * 4, x * 0.9, 0)"), ("ell_int_RC", "ell_int_RC(x + 1.2, y + 1.1)"),
              ("ell_int_RD", "ell_int_RD(x + 1.2, y + 1.1, 0.7)"), ("ell_int_RF", "ell_int_RF(x + 1.2, y + 1.1, 0.7)"),
              ("ell_int_RJ", "ell_int_RJ(x + 1.2, y + 1.1, 0.7, 2.5)")],
       "w = %s; grayColor(w)")
_cover(_GSL, [("ell_jac_cn_ri", "ell_jac_cn(ri:[x * 2, y * 2], 0.5)")], "w = %s; rgba:[w[0], w[1], 0, 1]")
_cover("tests/test_gpu_parity.py::test_rand_is_deterministic_and_stripe_invariant", [("rand", "rand(-2, 3)")],
       "w = %s; grayColor(w)")
_cover("tests/test_gpu_parity.py::test_per_row_slice_matches_oracle",
       [("origValXY", "in(xy + xy:[y * 0.1, 0])"), ("macro___origVal", "in(xy + xy:[y * 0.1, 0])")], "%s")
_cover("tests/test_gpu_closures.py::test_native_filter_on_closure_image", [("render", "render(inner(in, k))")],
       "rendered = %s; rendered(xy)", head="filter inner (image in, float k: 0-2 (1.0)) in(xy * k) end filter e (image in, float k: 0-2 (1))")
_cover("tests/test_gpu_parity.py::test_curve_and_gradient_user_values",
       [("apply_curve", "colors(tone(gray(p)))"), ("apply_gradient", "colors(tone(gray(p)))")],
       "p = in(xy); %s", where="tests/filters.py", link="curve_gradient", head="filter e (image in, curve tone, gradient colors)")
_cover(_NOISE, [("noise_perlin_simple", "noise(p)"), ("noise_perlin_full", "noise(oct, per, lac, p)"),
                ("noise_billow", "noiseBillow(oct, per, lac, p)"), ("noise_ridged_multi", "noiseRidgedMulti(oct, lac, p)"),
                ("noise_voronoi", "voronoiCells(p)")],
       "oct = 2; per = 0.5; lac = 2; p = xyz:[x, y, 0.5]; w = %s; grayColor(w)", where="tests/noise_probes.py", link="FULL")
