"""Probe filters for the counted back edge of exit-driven pair-mode loops (hipgen_pair.cpp plan_counted) and for the
kernel's own result pack (emit_store_pair), one per case of the code.

Like tests/pair_exit_probes.py: project text, arithmetic only, an iteration count n written as n / 16 (byte
round(n * 15.9375): distinct for n = 0..16), per-lane values as themselves.  `counted` says what the generator must
make of the probe's loop: "twin" (the bound is the counter's carry and the induction variable is computed from the
counter), "stepped" (counted, the induction variable keeps its own step) or "compare" (the earlier compare-and-mask
tail).  tests/test_pair_count_probes.py checks the texts and, with the oracle alone, that each probe exercises its
case; tests/test_gpu_pair_count.py renders them."""

BODY = "u = w * w - v * v + x * 1.5; v = 2 * w * v + y * 1.5; w = u;"
COND = "(w * w + v * v < 4)"

# (name, text, counted, what the case is)
COUNT_PROBES = [
    ("step_two", """filter t ()
  n = 0; w = x; v = y;
  while %s && (n < 9) do %s n = n + 2 end;
  rgba:[n * 0.0625, w * 0.2 + 0.5, v * 0.2 + 0.5, 1]
end
""" % (COND, BODY), "twin", "a step of 2 that jumps over the bound: n ends at 10"),
    ("less_equal", """filter t ()
  n = 0; w = x; v = y;
  while %s && (n <= 5) do %s n = n + 1 end;
  rgba:[n * 0.0625, w * 0.2 + 0.5, v * 0.2 + 0.5, 1]
end
""" % (COND, BODY), "twin", "`<=`: one trip more than `<`"),
    ("count_down", """filter t ()
  n = 13; w = x; v = y;
  while %s && (n > 1) do %s n = n - 3 end;
  rgba:[n * 0.0625, w * 0.2 + 0.5, v * 0.2 + 0.5, 1]
end
""" % (COND, BODY), "twin", "the induction variable counts down to a lower bound, in steps of 3"),
    ("negated", """filter t ()
  n = 0; w = x; v = y;
  while %s && !(n >= 6) do %s n = n + 1 end;
  rgba:[n * 0.0625, w * 0.2 + 0.5, v * 0.2 + 0.5, 1]
end
""" % (COND, BODY), "twin", "the bound as a negated comparison: the loop ends when it becomes true"),
    ("not_equal", """filter t ()
  n = 0; w = x; v = y;
  while %s && (n != 6) do %s n = n + 1 end;
  rgba:[n * 0.0625, w * 0.2 + 0.5, v * 0.2 + 0.5, 1]
end
""" % (COND, BODY), "twin", "`!=` with a step of one"),
    ("not_equal_step_two", """filter t ()
  n = 0; w = x; v = y;
  while %s && (n != 6) do %s n = n + 2 end;
  rgba:[n * 0.0625, w * 0.2 + 0.5, v * 0.2 + 0.5, 1]
end
""" % (COND, BODY), "compare", "`!=` with a step of two has no carry to test: the compare-and-mask tail"),
    ("register_bound", """filter t (int lim: 0-20 (7))
  n = 0; w = x; v = y;
  while %s && (n < lim) do %s n = n + 1 end;
  rgba:[n * 0.0625, w * 0.2 + 0.5, v * 0.2 + 0.5, 1]
end
""" % (COND, BODY), "stepped", "the bound is a frame constant in a scalar register: the counter starts from a run-time distance"),
    ("register_init", """filter t (int start: 0-20 (3))
  n = start; w = x; v = y;
  while %s && (n < 9) do %s n = n + 1 end;
  rgba:[n * 0.0625, w * 0.2 + 0.5, v * 0.2 + 0.5, 1]
end
""" % (COND, BODY), "stepped", "the induction variable starts from a frame constant"),
    ("counter_read_in_body", """filter t ()
  n = 0; w = x; v = y;
  while %s && (n < 8) do %s w = w + n * 0.03125; n = n + 1 end;
  rgba:[n * 0.0625, w * 0.2 + 0.5, v * 0.2 + 0.5, 1]
end
""" % (COND, BODY), "twin", "the body's arithmetic reads the induction variable, which is computed from the counter"),
]

# (name, text, distinct converted values, what the case is)
PACK_PROBES = [
    ("grey", """filter t ()
  g = x * y + 0.5;
  rgba:[g, g, g, 1]
end
""", 1, "one value in three channels, literal alpha 1"),
    ("two_equal", """filter t ()
  g = x * y + 0.5;
  rgba:[g, y * 0.5 + 0.5, g, 1]
end
""", 2, "two of three channels are the same value"),
    ("literal_alpha", """filter t ()
  rgba:[x * 0.5 + 0.5, y * 0.5 + 0.5, x * y + 0.5, 0.3]
end
""", 3, "three values and a literal alpha that is not 1 (byte floor(255 * 0.3f) = 76)"),
    ("four_values", """filter t ()
  rgba:[x * 0.5 + 0.5, y * 0.5 + 0.5, x * y + 0.5, x * x]
end
""", 4, "four different values"),
    ("out_of_range", """filter t ()
  rgba:[x * 3 + y, sqrt(x + y), 0.01 / (x * y), 2]
end
""", 3, "channels below 0 and above 1, NaN (the root of a negative sum), huge values of both signs, and a literal above 1"),
    ("literal_colour", """filter t ()
  rgba:[0.2, x * y + 0.5, 1.5, 0]
end
""", 1, "literal colour channels (bytes 51, 255 for 1.5, 0) around one value"),
]

SIZES = [(83, 61), (37, 7), (16, 1), (131, 77)]


def by_name(name):
    for p in COUNT_PROBES + PACK_PROBES:
        if p[0] == name:
            return p[1]
    raise KeyError(name)


def count_channel(frame, ch=0):
    """The counts a probe wrote as n * 0.0625 into channel `ch` (bytes floor(n * 15.9375))."""
    import numpy as np
    return np.ceil(frame[..., ch].astype(np.float64) / 15.9375 - 1e-9).astype(int)
