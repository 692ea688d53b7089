"""Probe filters for the fused doubling of exit-driven pair-mode loops (hipgen_pair.cpp plan_fusion: `d = t + t; r = d + b`
becomes r = fma(t, 2, b) under a guard on b), one per case of the code.

Like tests/pair_count_probes.py: project text, arithmetic only, an iteration count n written as n / 16, per-lane values as
themselves.  `fused`: how many statements of the probe the generator must fuse (each is two __builtin_fmaf, one per pixel
of the pair); `guarded`: whether the loop is printed twice under a guard (an addend that is no literal).
tests/test_pair_fma_probes.py checks the texts and, with the oracle alone, that each probe exercises its case;
tests/test_gpu_pair_fma.py renders them."""

# an escape-time loop whose imaginary part is the expression %s of tt = w * v and the pixel's b
SHAPE = """filter t ()
  n = 0; w = x; v = y; ca = x * 1.5; cb = y * 1.5;
  while (w * w + v * v < 4) && (n < 9) do
    tt = w * v; u = w * w - v * v + ca; v = %s; w = u; n = n + 1
  end;
  rgba:[n * 0.0625, w * 0.2 + 0.5, v * 0.2 + 0.5, 1]
end
"""

# 2^104 = (2^26)^4 and 2^101 = 2^26 * (2^25)^3 as exact float products; m: a small per-pixel integer, 1 to 4.
# The loop doubles q = 2^101, 2^103, ... -- 2^127 in the fourteenth trip, where q + q is +inf whatever b is while
# 2 * 2^127 - m * 2^104 is finite.  A pixel leaves after ceil((y + 1.5) * 8) trips, at most 14; r is what its last trip left.
OVERFLOW = """filter t ()
  k = 67108864.0;
  m = 1 + (if x > 0 then 1 else 0 end) + (if y > 0 then 2 else 0 end);
  cb = %s;
  q = k * 33554432.0 * 33554432.0 * 33554432.0;
  rr = 0; n = 0;
  while (n * 0.125 < y + 1.5) && (n < 14) do
    d = q + q; rr = d + cb; q = q * 4; n = n + 1
  end;
  rgba:[rr * 0.000000000000000000000000000001 * 0.000000001, n * 0.0625, m * 0.125, 1]
end
"""

# (name, text, fused statements, guarded, what the case is)
FMA_PROBES = [
    ("shape", SHAPE % "tt + tt + cb", 1, True, "(a) the Mandelbrot shape: t + t, then + b, b a pixel value from before the loop"),
    ("addend_first", SHAPE % "cb + (tt + tt)", 1, True, "(b) the addend on the left"),
    ("two_times", SHAPE % "2 * tt + cb", 1, True, "(b) 2 * t"),
    ("times_two", SHAPE % "tt * 2 + cb", 1, True, "(b) t * 2"),
    ("four_times", SHAPE % "4 * tt + cb", 1, True, "(b) 4 * t: a multiplier 2^2"),
    ("literal_addend", """filter t ()
  n = 0; w = x; v = y; ca = x * 1.5;
  while (w * w + v * v < 4) && (n < 9) do
    tt = w * v; u = w * w - v * v + ca; v = tt + tt + 0.25; w = u; n = n + 1
  end;
  rgba:[n * 0.0625, w * 0.2 + 0.5, v * 0.2 + 0.5, 1]
end
""", 1, False, "(b) a literal addend needs no guard: the loop is printed once, fused"),
    ("second_use", """filter t ()
  n = 0; w = x; v = y; s = 0; ca = x * 1.5; cb = y * 1.5;
  while (w * w + v * v < 4) && (n < 9) do
    tt = w * v; d = tt + tt; u = w * w - v * v + ca; v = d + cb; s = s + d * 0.125; w = u; n = n + 1
  end;
  rgba:[n * 0.0625, w * 0.2 + 0.5, v * 0.2 + 0.5, s * 0.2 + 0.5]
end
""", 0, False, "(c) the doubling is read a second time: not fused"),
    ("addend_in_loop", """filter t ()
  n = 0; w = x; v = y; ca = x * 1.5;
  while (w * w + v * v < 4) && (n < 9) do
    tt = w * v; c = w * 0.75; u = w * w - v * v + ca; v = tt + tt + c; w = u; n = n + 1
  end;
  rgba:[n * 0.0625, w * 0.2 + 0.5, v * 0.2 + 0.5, 1]
end
""", 0, False, "(d) the addend is defined inside the loop: not fused"),
    ("int_doubling", """filter t ()
  n = 0; w = x; v = y; j = 0; i = if x > 0 then 1 else 0 end; ca = x * 1.5; cb = y * 1.5;
  while (w * w + v * v < 4) && (n < 7) do
    u = w * w - v * v + ca; v = (w * v) * 3 + cb; w = u; j = j + j + i; n = n + 1
  end;
  rgba:[n * 0.0625, w * 0.2 + 0.5, j * 0.0078125, 1]
end
""", 0, False, "(e) an int doubling, and a multiplier that is no power of two: not fused"),
    ("overflow", OVERFLOW % "-(m * k * k * k * k)", 1, True,
     "(f) t + t overflows where 2t + b does not: |b| = m * 2^104 fails the guard in every wave"),
    ("overflow_half", OVERFLOW % "if x > 0 then -(m * k * k * k * k) else -m end", 1, True,
     "(g) the same with b large only for x > 0: the waves that straddle x = 0 are mixed, those left of it run fused"),
    ("zeros_denormals", """filter t ()
  z = x * 0.000000000000000000000000000001 * 0.000000000000000000000000000001;
  ee = y * 0.000000000000000000000000000001 * 0.0000000001;
  p = z; rr = 0; u = 0; n = 0;
  while (n * 0.25 < x + 1.25) && (n < 4) do
    d = p + p; rr = d + z; g = ee * 4; u = g + z; p = -p; ee = ee * 2; n = n + 1
  end;
  rgba:[rr, u, p, ee]
end
""", 2, True, "(h) t = -0 and b = -0 where x < 0 (x * 1e-30 * 1e-30 underflows to a signed zero), t of alternating sign, and a "
              "denormal t (y * 1e-40) times 4: signs and denormals show in float-map output"),
    ("two_statements", """filter t ()
  n = 0; w = x; v = y; ca = x * 1.5; cb = y * 1.5;
  while (w * w + v * v < 4) && (n < 9) do
    tt = w * v; hh = (w * w - v * v) * 0.5; u = hh + hh + ca; v = 2 * tt + cb; w = u; n = n + 1
  end;
  rgba:[n * 0.0625, w * 0.2 + 0.5, v * 0.2 + 0.5, 1]
end
""", 2, True, "(i) two fused statements in one loop, two addends in the guard"),
    ("nested", """filter t ()
  q = 0; s = 0; w = 0; v = 0;
  while (q < 1.5 + x) do
    n = 0; w = x; v = y; ca = x * 1.5 + q * 0.25; cb = y * 1.5 - q * 0.125;
    while (w * w + v * v < 4) && (n < 5) do tt = w * v; u = w * w - v * v + ca; v = tt + tt + cb; w = u; n = n + 1 end;
    s = s + n; q = q + 1
  end;
  rgba:[s * 0.0625, w * 0.2 + 0.5, v * 0.2 + 0.5, 1]
end
""", 1, True, "(j) a fused loop inside a per-pixel loop: the addend changes per outer trip, the guard is evaluated per entry"),
]

RAGGED = (67, 41)


def by_name(name):
    for p in FMA_PROBES:
        if p[0] == name:
            return p[1]
    raise KeyError(name)


def count_channel(frame, ch=0):
    """The counts a probe wrote as n * 0.0625 into channel `ch` (bytes floor(n * 15.9375))."""
    import numpy as np
    return np.ceil(frame[..., ch].astype(np.float64) / 15.9375 - 1e-9).astype(int)
