"""Probe filters for the peeled first loop trip of specialised pair kernels (specialize.cpp peel_first_trips), one per case.

Project text, arithmetic only; compiled specialised (`.specialized({})`) with MMHIP_PAIR=1.  An iteration count n is written
as n / 16, per-lane values as themselves.  `peeled`: how many loops the pass must peel.  tests/test_pair_peel_probes.py
checks the texts and, with the oracle alone, that each probe exercises its case; tests/test_gpu_pair_peel.py renders them."""

STEP = "u = w * w - v * v + x * 1.5; v = 2 * w * v + y * 1.5; w = u;"

# (name, text, peeled loops, what the case is)
PEEL_PROBES = [
    ("entered", """filter t ()
  n = 0; w = 0; v = 0;
  while (w * w + v * v < 4) && (n < 8) do %s n = n + 1 end;
  rgba:[n * 0.0625, w * 0.2 + 0.5, v * 0.2 + 0.5, 1]
end
""" % STEP, 1, "literal initial values and a first trip that is provably entered: the Mandelbrot shape"),
    ("not_provably_entered", """filter t ()
  n = 0; w = x * 2.5; v = 0;
  while (w * w + v * v < 4) && (n < 8) do %s n = n + 1 end;
  rgba:[n * 0.0625, w * 0.2 + 0.5, v * 0.2 + 0.5, 1]
end
""" % STEP, 0, "the entry condition depends on the pixel (some pixels never enter): no peel"),
    ("frame_constant_init", """filter t ()
  n = 0; w = t * 0.5; v = 0;
  while (w * w + v * v < 4) && (n < 8) do %s n = n + 1 end;
  rgba:[n * 0.0625, w * 0.2 + 0.5, v * 0.2 + 0.5, 1]
end
""" % STEP, 0, "an initial value that is no literal (a frame constant): the entry condition does not fold, no peel"),
    ("bound_one", """filter t ()
  n = 0; w = 0; v = 0;
  while (w * w + v * v < 4) && (n < 1) do %s n = n + 1 end;
  rgba:[n * 0.0625, w * 0.2 + 0.5, v * 0.2 + 0.5, 1]
end
""" % STEP, 1, "the loop ends right after the peeled trip; its phis are read after it"),
    ("some_leave_at_once", """filter t ()
  n = 0; w = 0; v = 0;
  while (w * w + v * v < 4) && (n < 8) do u = w * w - v * v + x * 3; v = 2 * w * v + y * 3; w = u; n = n + 1 end;
  rgba:[n * 0.0625, w * 0.1 + 0.5, v * 0.1 + 0.5, 1]
end
""", 1, "the peeled trip ends the loop for the pixels outside the circle of radius 2 / 3 only"),
    ("if_in_body", """filter t ()
  n = 0; w = 0; c = 0;
  while (w * w < 4) && (n < 8) do
    c = if w < 0 then c + 1 else c end;
    w = if w < 0 then w * w + y else w * 1.5 - x * y * 3 - 0.3 end;
    n = n + 1
  end;
  rgba:[n * 0.0625, w * 0.2 + 0.5, c * 0.0625, 1]
end
""", 1, "an `if` in the body whose condition folds in the peeled trip (w = 0 is not below 0) and not afterwards"),
    ("two_loops", """filter t ()
  n = 0; w = 0; v = 0;
  while (w * w + v * v < 4) && (n < 5) do %s n = n + 1 end;
  m = 0; q = 0;
  while (q * q < 3) && (m < 6) do q = q * q + w * 0.5 + 0.4; m = m + 1 end;
  rgba:[n * 0.0625, m * 0.0625, q * 0.2 + 0.5, 1]
end
""" % STEP, 2, "two loops in sequence, both peeled; the second reads the first's exit values"),
    ("nested", """filter t ()
  q = 0; s = 0; w = 0; v = 0;
  while (q < 1.5 + x) do
    n = 0; w = 0; v = 0;
    while (w * w + v * v < 4) && (n < 3) do u = w * w - v * v + x * 1.5 + q * 0.25; v = 2 * w * v + y * 1.5; w = u; n = n + 1 end;
    s = s + n; q = q + 1
  end;
  rgba:[s * 0.0625, w * 0.2 + 0.5, v * 0.2 + 0.5, 1]
end
""", -1, "a loop with literal initial values inside a per-pixel loop (-1: the inner loop is peeled, the outer one is not)"),
    ("minus_zero", """filter t ()
  p = x * 0.000000000000000000000000000001 * 0.000000000000000000000000000001;
  n = 0; w = 0;
  while (w * w < 4) && (n < 3) do w = w + p; n = n + 1 end;
  rgba:[w, n * 0.0625, p, 1]
end
""", 1, "the first trip adds p = -0 where x < 0 (x * 1e-30 * 1e-30 underflows to a signed zero): 0 + -0 is +0, so w is +0 for every "
        "pixel; folding `0 + p` to p would leave -0 in the left half.  The sign shows in float-map output, compared bit for bit "
        "(the language's `/` answers 0 for a zero divisor whatever its sign, and atan2 is not pair-mode arithmetic)"),
]

SIZES = [(83, 61), (37, 7), (16, 1), (131, 77)]


def by_name(name):
    for p in PEEL_PROBES:
        if p[0] == name:
            return p[1]
    raise KeyError(name)


def count_channel(frame, ch=0):
    """The counts a probe wrote as n * 0.0625 into channel `ch` (bytes floor(n * 15.9375))."""
    import numpy as np
    return np.ceil(frame[..., ch].astype(np.float64) / 15.9375 - 1e-9).astype(int)
