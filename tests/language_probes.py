"""Probes of the language core -- grammar, typing, control flow, order of evaluation, tuples, the frame's variables, curve and
gradient tables, filter calls and closures -- for tests/test_language_reference.py (the oracle against the restatement) and
tests/test_gpu_language.py (the GPU against both).

A probe is a filter text, user-value sets, the frames it is rendered at, and `pixel`, a Python function giving the four
channels of one pixel.  `pixel` is written from the reference's text (parser.y, scanner.c, exprtree.c, compiler.c, opmacros.h,
new_template.c.in; the lines are cited at each probe and in tests/language_reference.py) and evaluated on float32 scalars, so a
loop is a Python loop.  The operands are run-time values, va = x * ua + ub and its like, so the generic kernel folds nothing;
Filter.specialized bakes a set in and exercises the folds.  Four results share one rgba:[...], so a probe costs one JIT per
variant.  `covers` names the grammar alternatives of parser.y:170-262 (RULES) and the variables the probe exercises."""
import numpy as np

from tests import language_reference as L

F = np.float32
SIZE = (37, 21)               # odd and not square: a pixel with r == 0, rows with y < 0, more than one wave, pairs that split
UV = ("ua", "ub", "uc", "ud", "un", "k")
HEAD = ("filter probe (float ua: -4-4 (1), float ub: -4-4 (0.25), float uc: -4-4 (-0.75), float ud: -4-4 (0.5), "
        "float un: 0-8 (3), int k: 0-20000000 (3)%s)\n")
OPERANDS = "  va = x * ua + ub; vb = y * uc + ud; vc = (x + y) * ub + uc; vd = (x - y) * ud + ua;\n"
SETS = {
    "generic": dict(ua=1.0, ub=0.25, uc=-0.75, ud=0.5, un=3.0, k=3),
    "other": dict(ua=0.5, ub=-1.5, uc=2.0, ud=0.125, un=5.0, k=2),
}

# parser.y:170-262, one name per alternative
RULES = (
    "type_float", "type_int", "type_bool", "type_color", "type_gradient", "type_curve", "type_image",
    "int", "float", "ident", "tuple", "select_ident", "select_paren", "cast", "convert",
    "add", "sub", "mul", "div", "mod", "pow", "equal", "less", "greater", "lessequal", "greaterequal", "notequal",
    "or", "and", "xor", "neg", "not", "paren", "call", "assign", "sub_assign", "sequence",
    "if_then", "if_then_else", "while", "do_while", "for",
    "arglist_empty", "arglist", "exprlist", "subscripts", "subscript_expr", "subscript_range", "else_semicolon", "end_semicolon",
)
# alternatives without a probe: the test that has them instead, or why there is none
RULES_ELSEWHERE = {
    "convert": "tests/test_language_reference.py::test_tag_conversion_is_refused -- `::` is not implemented and says so; no example uses it",
    "arglist_empty": "a call without arguments resolves to nothing in the reference (exprtree.c:1064 reads args->result of no argument); no text reaches it",
}
# the variables of a frame: parser.cpp's internals and macros.c's variable macros
VARIABLES = ("x", "y", "r", "a", "t", "R", "frame", "X", "Y", "W", "H", "__canvasPixelW", "__canvasPixelH", "__renderPixelW",
             "__renderPixelH", "xy", "ra", "XY", "WH", "pi", "e", "I")


class Pixel:
    """what `pixel` sees: the frame's variables at one pixel as float32 scalars, the set `u`, the frame `fr`"""

    def __init__(self, fr, row, col, u, tables):
        self.fr, self.u, self.tables = fr, u, tables
        self.x, self.y, self.r, self.a = fr.x[row, col], fr.y[row, col], fr.r[row, col], fr.a[row, col]
        for n in ("t", "frame", "R", "W", "H", "X", "Y", "pi", "e", "I"):
            setattr(self, n, getattr(fr, n))

    def operands(self):
        u = self.u
        return (self.x * u["ua"] + u["ub"], self.y * u["uc"] + u["ud"], (self.x + self.y) * u["ub"] + u["uc"],
                (self.x - self.y) * u["ud"] + u["ua"])


class Case:
    """one frame a probe is rendered at: size, time, frame number, and the band of rows (None: all)"""

    def __init__(self, width, height, t=0.0, frame=0, rows=None):
        self.width, self.height, self.t, self.frame, self.rows = width, height, t, frame, rows

    def __repr__(self):
        band = "" if self.rows is None else " rows %d-%d" % (self.rows[0], self.rows[1] - 1)
        return "%dx%d t=%g frame=%d%s" % (self.width, self.height, self.t, self.frame, band)


WHOLE = (Case(*SIZE),)
# §6 of the probe list: the four sizes whole, and a band of 37x21 at another time and frame number
FRAME_CASES = (Case(32, 32), Case(37, 21), Case(21, 37), Case(5, 1), Case(37, 21, t=0.375, frame=7, rows=(5, 12)))
CALL_CASES = (Case(37, 21, t=0.125), Case(21, 37, t=0.125))


class Probe:
    def __init__(self, name, body, pixel, covers, extra_args="", sets=None, flags="default", cases=WHOLE, libm=None, helpers="",
                 operands=True, tables=None, inexact_sets=(), arithmetic=False):
        """`body`: the filter's text after the operands; `libm`: None (bit for bit) or (id, channels) -- those channels are held
        under builtin_probes.compare's bound for that builtin id, the others bit for bit; `helpers`: filters before the main
        one; `tables`: name -> (kind, array) of curve and gradient values; `inexact_sets`: sets with a NaN or a negative zero,
        where the specialised variant is held to the oracle's evaluation of its own IR alone (builtin_probes.INEXACT_FOLD_SETS);
        `arithmetic`: control flow over arithmetic alone, which the pair generator must take"""
        self.name, self.pixel, self.covers, self.flags, self.cases, self.libm = name, pixel, tuple(covers.split()), flags, cases, libm
        self.sets = dict(sets or SETS)
        self.tables = tables or {}
        self.inexact_sets, self.arithmetic = tuple(inexact_sets), arithmetic
        self.text = helpers + L.OPTION_TEXT[flags] + HEAD % extra_args + (OPERANDS if operands else "") + body.rstrip() + "\nend\n"
        for c in self.covers:
            assert c in RULES or c in VARIABLES, c

    def uservals(self, name):
        """the set as the oracle and the invocation take it (scalars and colours; tables go by `tables`)"""
        full = dict(SETS["generic"])
        full.update(self.sets[name])
        return full

    def expected(self, case, name):
        """float32 [rows, width, 4] of the case's band"""
        u = dict((k, (v if isinstance(v, (int, tuple, bool)) and not isinstance(v, float) else F(v))) for k, v in self.uservals(name).items())
        fr = L.Frame(case.width, case.height, self.flags, case.t, case.frame)
        lo, hi = case.rows or (0, case.height)
        out = np.zeros((hi - lo, case.width, 4), F)
        tables = dict((n, v[1]) for n, v in self.tables.items())
        with np.errstate(all="ignore"):
            for row in range(lo, hi):
                for col in range(case.width):
                    out[row - lo, col] = [F(v) for v in self.pixel(Pixel(fr, row, col, u, tables))]
        return out


PROBES = []


def probe(name, covers, body, **kw):
    def wrap(fn):
        PROBES.append(Probe(name, body, fn, covers, **kw))
        return fn
    return wrap


def _min(a, b):
    return a if a < b else b          # the builtins' min and max, held by the builtin probes


def _max(a, b):
    return b if a < b else a


def _t(c):
    return L.truth(bool(c))


# ---- 1. grammar: parser.y:52-61, the precedences, lowest first:  ;  =  || && xor  == < > <= >= !=  + -  * / %  ^  unary  :  [ ----------
@probe("assoc_sub_div_mod", "sub div mul mod ident", "  rgba:[va - vb - vc, va / vb * vc, va * vb % vc, va - vb * vc]")
def _(p):
    a, b, c, d = p.operands()          # %left: (a - b) - c, (a / b) * c, (a * b) % c;  * over -
    return [(a - b) - c, L.div(a, b) * c, L.mod(a * b, c), a - b * c]


@probe("mul_over_add_compare", "add mul less greater lessequal greaterequal",
       "  rgba:[va + vb * vc + vd, va + vb < vc * vd, va > vb + vc, (va <= vb) + (vc >= vd) * 2]")
def _(p):
    a, b, c, d = p.operands()          # + - over the comparisons, * over +
    return [(a + b * c) + d, _t((a + b) < (c * d)), _t((b + c) < a), _t(a <= b) + _t(d <= c) * 2]


# whole-number operands, so that pow is exact: pa is ub or ua + ub, ...
POW_SETS = {"ints": dict(ua=1.0, ub=2.0, uc=1.0, ud=2.0), "ints2": dict(ua=2.0, ub=1.0, uc=-1.0, ud=2.0)}


@probe("pow", "pow neg mul greater paren", "  pa = (x > 0) * ua + ub; pb = (y > 0) * uc + ud; pc = (x > y) * ua + ud;\n"
       "  rgba:[pa ^ pb ^ pc, -pa ^ pb, pa ^ -pb, pa * pb ^ pc]", sets=POW_SETS, libm=("pow_1", (0, 1, 2, 3)))
def _(p):
    u = p.u                            # %right '^', and UNARY above it: pa ^ (pb ^ pc), (-pa) ^ pb, pa ^ (-pb), pa * (pb ^ pc)
    pa, pb, pc = _t(p.x > 0) * u["ua"] + u["ub"], _t(p.y > 0) * u["uc"] + u["ud"], _t(p.x > p.y) * u["ua"] + u["ud"]
    return [L.power(pa, L.power(pb, pc)), L.power(-pa, pb), L.power(pa, -pb), pa * L.power(pb, pc)]


@probe("logic_and_compare", "not equal less notequal or and xor greater", "  ba = va > 0; bb = vb > 0; bc = vc > vd;\n"
       "  rgba:[!ba == bb, ba < bb == bc, (ba || bb && bc) + 2 * (ba != bb), ba xor bb || bc]")
def _(p):
    a, b, c, d = p.operands()          # unary over ==; < and == one level, left; || && xor one level, left
    ba, bb, bc = 0 < a, 0 < b, d < c
    return [_t((not ba) == bb), _t(_t(_t(ba) < _t(bb)) == _t(bc)), _t((ba or bb) and bc) + 2 * _t(ba != bb), _t((ba != bb) or bc)]


@probe("tag_binds_tighter", "cast tuple mul neg add select_paren select_ident",
       "  w = ri:[va, vb] * ri:[vc, vd]; n2 = -ri:[va, vb]; z = ri:[va, vb] + vc;\n  rgba:[w[0], w[1], n2[1], (z)[1]]")
def _(p):
    a, b, c, d = p.operands()          # %right ':' above the operators: a complex product, and ri + scalar adds to the real part
    return [a * c - b * d, a * d + c * b, -b, b + F(0)]


@probe("subscripts", "select_ident select_paren subscripts subscript_expr subscript_range tuple int",
       "  v = [va, vb, vc, vd];\n  rgba:[v[2], (v * vc)[1], (v[0,2])[1], (v[1..3])[2]]")
def _(p):
    a, b, c, d = p.operands()
    return [c, b * c, c, d]


@probe("assignment", "assign neg or less equal mul add",
       "  s = (aa = bb = va) + aa + bb; w = vb < vc || vd == va; m = vc * nn = vb + 1; q = -oo = vd;\n  rgba:[s, w, m + q, nn + oo]")
def _(p):
    a, b, c, d = p.operands()          # %right '=' below everything but ';':  vc * (nn = (vb + 1)),  -(oo = vd)
    return [(a + a) + a, _t(b < c or d == a), c * (b + 1) + -d, (b + 1) + d]


@probe("sequences_comments_literals", "sequence paren call tuple subscript_expr float else_semicolon end_semicolon if_then_else arglist exprlist",
       "  # a comment line\n  v = [va, vb, vc, vd];   # a comment after code\n  p1 = (kk = va; kk * 2);\n  q1 = min((kk = vb; kk + 1), vc);\n"
       "  t4 = [(kk = vc; kk), kk + .5, 5. * kk, 0];\n  s1 = v[(kk = 1; 2)];\n  i1 = if va < vb then vc; else vd; end;\n"
       "  rgba:[p1, q1, t4[1] + t4[2], s1 + i1]")
def _(p):
    a, b, c, d = p.operands()          # `;` inside ( ), arguments, elements and subscripts; `; else`, `; end`; # to the line's end
    return [a * 2, _min(b + 1, c), (c + F(0.5)) + F(5.0) * c, c + (c if a < b else d)]


# ---- 2. types ---------------------------------------------------------------------------------------------------------------------
@probe("int_and_float_literals", "int float div mod sub add mul paren", "  rgba:[7 / 2 * va, (7 % 3) * va, (2 - 5) * 3 * vb, va * (1 / 4) + (1 + 2)]")
def _(p):
    a, b, c, d = p.operands()          # `/` is the float quotient of two ints (opmacros.h:41); + - * of ints stay ints
    return [F(3.5) * a, F(1) * a, F(-9) * b, a * F(0.25) + F(3)]


INT_SETS = {"above_2_24": dict(k=16777217), "small": dict(k=5)}


@probe("int_user_value", "type_int type_float sub mod equal mul int", "  rgba:[k - 16777216, k % 2, (k == 16777217) + (k * 3 - 50331650), (k - 16777215) * va]",
       sets=INT_SETS)
def _(p):
    a, b, c, d = p.operands()          # USERVAL_INT_ACCESS is an int (opmacros.h:130): 16777217 is no float, so a float's trip shows
    k = p.u["k"]
    return [L.int_to_float(k - 16777216), L.mod(np.float64(k), 2), L.int_to_float(int(k == 16777217) + (k * 3 - 50331650)),
            L.int_to_float(k - 16777215) * a]


@probe("variable_of_two_types", "assign if_then greater sub mul",
       "  nn = 16777217; before = nn - 16777216; if va > vb then nn = 0.5 end; after = nn * 2;\n  rgba:[before, after, nn, va]")
def _(p):
    a, b, c, d = p.operands()          # compiler.c:2811-2865: nn is a float everywhere, so the int literal is rounded on the way in
    nn = F(16777217)
    before = nn - F(16777216)
    if b < a:
        nn = F(0.5)
    return [before, nn * 2, nn, a]


@probe("comparisons_as_numbers", "less equal mul add sub", "  rgba:[(va < vb) * 3 + 0.5, (va < vb) + (vc < vd) + (va == va), vb * (vc < vd), 1 - (va < vb)]")
def _(p):
    a, b, c, d = p.operands()
    return [_t(a < b) * 3 + F(0.5), _t(a < b) + _t(c < d) + _t(a == a), b * _t(c < d), 1 - _t(a < b)]


COLOR_SETS = {"on": dict(bv=True, col=(0.25, 0.5, 0.75, 1.0)), "off": dict(bv=False, col=(1.0, 0.125, 0.0, 0.375))}


@probe("bool_and_color_user_values", "type_bool type_color not mul add select_ident", "  rgba:[bv * va + !bv * vb, col[0], col[1] * va, col[2] + col[3]]",
       extra_args=", bool bv, color col", sets=COLOR_SETS)
def _(p):
    a, b, c, d = p.operands()          # a colour is four bytes read as byte / 255.0 (opmacros.h:147-150, 176-181)
    bv, col = _t(p.u["bv"]), L.color_channels(p.u["col"])
    return [bv * a + _t(bv == 0) * b, col[0], col[1] * a, col[2] + col[3]]


# ---- 3. control flow (compiler.c:2089-2138) ---------------------------------------------------------------------------------------------
@probe("if_values", "if_then if_then_else less assign mul",
       "  i1 = if va < vb then vc else vd end; i2 = if va < vb then vc end; if vb < vc then q1 = vd end;\n"
       "  q2 = va; if vc < vd then q2 = vb; q3 = q2 * 2 end;\n  rgba:[i1, i2, q1 + q2, q3]", arithmetic=True)
def _(p):
    a, b, c, d = p.operands()          # no else, or a variable of one branch: the other path reads 0 (backends/cc.c:71-77)
    i1, i2 = (c if a < b else d), (c if a < b else F(0))
    q1 = d if b < c else F(0)
    q2, q3 = a, F(0)
    if c < d:
        q2 = b
        q3 = q2 * 2
    return [i1, i2, q1 + q2, q3]


@probe("while_and_do", "while do_while less add mul greater end_semicolon",
       "  nn = 0; s = va;\n  w = while nn < un do s = s * vb + vc; nn = nn + 1 end;\n  m = 10; z = while m < un do zz = vd; m = m + 1; end;\n"
       "  dd = 0; do dd = dd + va while ud > 100 end;\n  rgba:[s + w, zz + m + z, dd, nn]", arithmetic=True)
def _(p):
    a, b, c, d = p.operands()          # a loop's value is the int 0; a zero-trip body's variable reads 0; do runs its body once first
    nn, s = 0, a
    while F(nn) < p.u["un"]:
        s = s * b + c
        nn += 1
    return [s + F(0), F(0) + F(10) + F(0), F(0) + a, F(nn)]


@probe("for_loops", "for assign add mul sub",
       "  s = 0; e1 = k;\n  for i = 0 .. e1 do s = s + va * i; e1 = e1 - 1 end;\n  f = 0; for g = 0.5 .. un do f = f + g * vb end;\n"
       "  rgba:[s, e1 + i * 100, f, g]", arithmetic=True)
def _(p):
    a, b, c, d = p.operands()          # exprtree.c:1354-1385: the end is read once, into a temporary; the counter ends one past it
    k = p.u["k"]
    s, e1, i = F(0), k, 0
    while i <= k:
        s = s + a * F(i)
        e1 -= 1
        i += 1
    f, g = F(0), F(0.5)
    while g <= p.u["un"]:
        f = f + g * b
        g = g + 1
    return [s, F(e1 + i * 100), f, g]


@probe("nested_for", "for add mul", "  s = 0;\n  for i = 0 .. k do for j = i .. k do s = s + va * j + i end end;\n  rgba:[s, i, j, vb]", arithmetic=True)
def _(p):
    a, b, c, d = p.operands()
    k, s, i, j = p.u["k"], F(0), 0, 0
    while i <= k:
        j = i
        while j <= k:
            s = (s + a * F(j)) + F(i)
            j += 1
        i += 1
    return [s, F(i), F(j), b]


@probe("three_loops_deep", "while less greater add mul",
       "  q = (x + y) * (x + y) * un; nn = (q > 0.5) + (q > 1) + (q > 2) + (q > 3) + (q > 5); s = vd; i = 0;\n  while i < k do\n    j = 0;\n    while j < 2 do\n      m = 0;\n"
       "      while m < nn do s = s * vb + vc + m; m = m + 1 end;\n      j = j + 1\n    end;\n    i = i + 1\n  end;\n  rgba:[s, nn, i + j, m]",
       sets={"generic": dict(SETS["generic"], un=3.2), "other": dict(SETS["other"], un=2.0)}, arithmetic=True)
def _(p):
    a, b, c, d = p.operands()          # the innermost trip count is 0 to 5 and changes from pixel to pixel
    q = (p.x + p.y) * (p.x + p.y) * p.u["un"]
    nn = _t(F(0.5) < q) + _t(1 < q) + _t(2 < q) + _t(3 < q) + _t(5 < q)
    s, i, j, m = d, 0, 0, 0
    while i < p.u["k"]:
        j = 0
        while j < 2:
            m = 0
            while F(m) < nn:
                s = (s * b + c) + F(m)
                m += 1
            j += 1
        i += 1
    return [s, nn, F(i + j), F(m)]


@probe("if_in_loop_in_if", "if_then if_then_else while greater less add mul",
       "  s = vd; nn = 0;\n  if va > vb then while nn < un do if s < vc then s = s + va else s = s * 0.5 end; nn = nn + 1 end end;\n  rgba:[s, nn, va, vb]",
       arithmetic=True)
def _(p):
    a, b, c, d = p.operands()
    s, nn = d, 0
    if b < a:
        while F(nn) < p.u["un"]:
            s = s + a if s < c else s * F(0.5)
            nn += 1
    return [s, F(nn), a, b]


@probe("swap_through_a_temporary", "while assign add less", "  pp = va; qq = vb; nn = 0;\n  while nn < un do tmp = pp; pp = qq; qq = tmp + vc; nn = nn + 1 end;\n  rgba:[pp, qq, tmp, nn]",
       arithmetic=True)
def _(p):
    a, b, c, d = p.operands()
    pp, qq, tmp, nn = a, b, F(0), 0
    while F(nn) < p.u["un"]:
        tmp = pp
        pp = qq
        qq = tmp + c
        nn += 1
    return [pp, qq, tmp, F(nn)]


# ---- 4. side effects and order: elements, arguments and subscripts are evaluated left to right (compiler.c:1794-1823, 1903-1958) -------
@probe("assignments_inside_expressions", "assign tuple call select_ident subscript_expr paren add",
       "  v = [va, vb, vc, vd];\n  t1 = [(q = va), q + 1]; m = max((q2 = vb), q2 + 1); s = v[(i = 1)] + i; w = (a2 = b2 = x) + a2 + b2;\n"
       "  rgba:[t1[0] * 2 + t1[1], m, s, w]")
def _(p):
    a, b, c, d = p.operands()
    return [a * 2 + (a + 1), _max(b, b + 1), b + 1, (p.x + p.x) + p.x]


# ---- 5. tuples ---------------------------------------------------------------------------------------------------------------------------
@probe("tuples", "select_ident subscripts subscript_range sub_assign cast call add",
       "  v = [va, vb, vc, vd];\n  m = v[0,2]; rng = v[1..3];\n  v[1] = va * 2; v[2,3] = [vb + 1, vc + 1];\n  sub = v[1 + 1];\n"
       "  tt = toXY(xy:ra:[va, vb]);\n  rgba:[m[1] + rng[2], v[1] + v[3], sub, tt[0]]")
def _(p):
    a, b, c, d = p.operands()          # a cast of a cast keeps the outer tag: toXY of an xy is the tuple itself
    return [c + d, a * 2 + (c + 1), b + 1, a]


# ---- 6. the variables of the frame, under the three flag sets --------------------------------------------------------------------------
def _frame_probes(flags):
    kw = dict(flags=flags, cases=FRAME_CASES, operands=False, sets={"generic": SETS["generic"]})
    probe("xyra_" + flags, "x y r a", "  rgba:[x, y, r, a]", libm=("toRA", (2, 3)), **kw)(lambda p: [p.x, p.y, p.r, p.a])
    probe("t_frame_R_" + flags, "t frame R xy", "  rgba:[t, frame, R, xy[0]]", **kw)(lambda p: [p.t, p.frame, p.R, p.x])
    probe("limits_" + flags, "W H X Y", "  rgba:[W, H * x, X, Y]", **kw)(lambda p: [p.W, p.H * p.x, p.X, p.Y])
    probe("macros_" + flags, "XY WH xy ra", "  rgba:[XY[0] + xy[1], XY[1], WH[0], WH[1] + ra[0]]", libm=("toRA", (3,)), **kw)(
        lambda p: [p.X + p.y, p.Y, p.W, p.H + p.r])
    probe("constants_" + flags, "pi e I ra", "  rgba:[pi, e, I[0] + ra[1], I[1]]", libm=("toRA", (2,)), **kw)(
        lambda p: [p.pi, p.e, p.I[0] + p.a, p.I[1]])
    probe("pixel_sizes_" + flags, "__canvasPixelW __canvasPixelH __renderPixelW __renderPixelH",
          "  rgba:[__canvasPixelW, __canvasPixelH * y, __renderPixelW, __renderPixelH]", **kw)(
        lambda p: [F(p.fr.width), F(p.fr.height) * p.y, F(p.fr.width), F(p.fr.height)])


for _flags in L.FLAGS:
    _frame_probes(_flags)


# ---- 7. curve and gradient user values with explicit tables (opmacros.h:192-194) ------------------------------------------------------
def curve_table():
    """not monotonic, and no two entries alike: an index off by one shows"""
    return (((np.arange(1024) * 37) % 1024) / 1024.0).astype(F)


def gradient_table():
    """0xRRGGBBAA; neighbours differ in every channel but blue, alpha varies"""
    i = np.arange(1024, dtype=np.uint32)
    return ((i & 255) << 24) | (((i * 7) & 255) << 16) | (((i >> 2) & 255) << 8) | ((i * 13) & 255)


def _ulp(v, n):
    v = F(v)
    for _ in range(abs(n)):
        v = np.nextafter(v, F(np.inf) if n > 0 else F(-np.inf))
    return float(v)


def _k(k):
    return float(F(k) / F(1023))


# with ua = 0 the argument x * ua + ub is ub itself (a zero of either sign plus ub)
TABLE_SETS = {
    "ramp": dict(ua=0.75, ub=0.5, uc=0.25, ud=0.75, un=1.0),                        # arguments from -0.5 to 1.75, pixel by pixel
    "outside": dict(ua=0.0, ub=-0.5, uc=1.5, ud=1.0, un=float("nan")),              # below 0, above 1, exactly 1, NaN
    "steps_low": dict(ua=0.0, ub=_k(1), uc=_ulp(_k(1), -1), ud=_ulp(_k(1), 1), un=_k(511)),
    "steps_mid": dict(ua=0.0, ub=_ulp(_k(511), -1), uc=_ulp(_k(511), 1), ud=_k(512), un=_ulp(_k(512), -1)),
    "steps_high": dict(ua=0.0, ub=_ulp(_k(1022), -1), uc=_k(1022), ud=_ulp(_k(1022), 1), un=_ulp(1.0, -1)),
}
_TABLES = {"cv": ("curve", curve_table()), "gr": ("gradient", gradient_table())}


def _table_arguments(p):
    u = p.u
    return [p.x * u["ua"] + u["ub"], p.y * u["ua"] + u["uc"], p.x * u["ua"] + u["ud"], p.y * u["ua"] + u["un"]]


@probe("curve_table", "type_curve call add mul", "  rgba:[cv(x * ua + ub), cv(y * ua + uc), cv(x * ua + ud), cv(y * ua + un)]",
       extra_args=", curve cv, gradient gr", sets=TABLE_SETS, tables=_TABLES, operands=False, inexact_sets=("outside",))
def _(p):
    return [L.apply_curve(p.tables["cv"], v) for v in _table_arguments(p)]


@probe("gradient_table", "type_gradient call select_ident add mul",
       "  g0 = gr(x * ua + ub); g1 = gr(y * ua + uc); g2 = gr(x * ua + ud); g3 = gr(y * ua + un);\n  rgba:[g0[0] + g0[3], g1[1] + g1[3], g2[2] + g2[3], g3[3]]",
       extra_args=", curve cv, gradient gr", sets=TABLE_SETS, tables=_TABLES, operands=False, inexact_sets=("outside",))
def _(p):
    g = [L.apply_gradient(p.tables["gr"], v) for v in _table_arguments(p)]
    return [g[0][0] + g[0][3], g[1][1] + g[1][3], g[2][2] + g[2][3], g[3][3]]


# ---- 8. filter calls and closures (exprtree.c:820-976) ----------------------------------------------------------------------------------
HELPER = "filter helper (float hk)\n  rgba:[x * hk, y + hk, t, x + y]\nend\n\n"


def _helper(hx, hy, hk, t):
    return [hx * hk, hy + hk, F(t), hx + hy]


@probe("calls_and_closures", "call ident cast tuple",
       "  c0 = helper(va);\n  v1 = c0(xy);\n  v2 = helper(vb, xy:[y, x]);\n  v3 = helper(vc, xy:[x * 0.5, y], 0.75);\n  v4 = c0(xy:[y, x], 0.75);\n"
       "  rgba:[v1[0] + v1[3], v2[1] + v2[0], v3[2] + v3[0], v4[0] + v4[2]]", helpers=HELPER, cases=CALL_CASES, sets={"generic": SETS["generic"]})
def _(p):
    a, b, c, d = p.operands()          # arguments only: a closure, kept and applied later; without a time the caller's t goes in
    lim = p.fr.limits
    v1 = _helper(*L.callee_position(p.x, p.y, lim, lim), a, p.t)
    v2 = _helper(*L.callee_position(p.y, p.x, lim, lim), b, p.t)
    v3 = _helper(*L.callee_position(p.x * F(0.5), p.y, lim, lim), c, 0.75)
    v4 = _helper(*L.callee_position(p.y, p.x, lim, lim), a, 0.75)
    return [v1[0] + v1[3], v2[1] + v2[0], v3[2] + v3[0], v4[0] + v4[2]]


@probe("closure_as_image_argument", "call type_image cast tuple",
       "  w = second(helper(va), vb, xy);\n  rgba:[w[0], w[1], w[2], w[3]]", cases=CALL_CASES, sets={"generic": SETS["generic"]},
       helpers=HELPER + "filter second (image im, float sk)\n  im(xy:[x * sk, y])\nend\n\n")
def _(p):
    a, b, c, d = p.operands()          # `second` wraps its image argument in its own factors (compiler.c:2444-2445)
    lim = p.fr.limits
    sx, sy = L.callee_position(p.x, p.y, lim, lim)
    hx, hy = L.callee_position(sx * b, sy, lim, lim, through=(lim,))
    return _helper(hx, hy, a, p.t)


@probe("pixel_helper_from_a_unit_filter", "call W X", "  w = inpixels(va, xy);\n  rgba:[w[0], w[1], w[2], w[3]]", cases=CALL_CASES,
       sets={"generic": SETS["generic"]}, helpers="pixel filter inpixels (float hk)\n  rgba:[x, y * hk, W, X]\nend\n\n")
def _(p):
    a, b, c, d = p.operands()          # the callee's x is the caller's, times the caller's factors, times the callee's own X
    inner = L.Limits(p.fr.width, p.fr.height, "pixel")
    hx, hy = L.callee_position(p.x, p.y, p.fr.limits, inner)
    return [hx, hy * a, inner.W, inner.X]


BY_NAME = dict((p.name, p) for p in PROBES)
assert len(BY_NAME) == len(PROBES)
