"""Probe filters for the exit-driven pair-mode loops (hipgen_pair.cpp exit_driven_iteration), one per case of the new code.

Each probe is project text, arithmetic only (so it runs in pair mode), and writes what tells its case apart into its
channels: an iteration count n as n / 8 (byte round(n * 31.875): distinct for n = 0..8), a per-lane value as itself.
`check` is what the oracle's frame must show for the probe to exercise its case (tests/test_pair_exit_probes.py checks
that without a GPU); tests/test_gpu_pair_exit.py renders them."""

# (name, text, what the case is)
PROBES = [
    ("never_entered",
     """filter t ()
  n = 0; w = x;
  while (w * w < -1) && (n < 6) do w = w * w + y; n = n + 1 end;
  rgba:[n * 0.125, w * 0.5 + 0.5, 0.25, 1]
end
""", "a loop no pixel enters: the exit copies keep the initial values"),
    ("one_iteration",
     """filter t ()
  n = 0; w = x;
  while (w * w < 4) && (n < 6) do w = w + 5; n = n + 1 end;
  rgba:[n * 0.125, (w - 4) * 0.5, 0.25, 1]
end
""", "every pixel leaves at the first back edge"),
    ("uniform_bound",
     """filter t ()
  n = 0; w = x;
  while (w * w < 100) && (n < 7) do w = w * 0.5 + y * 0.25; n = n + 1 end;
  rgba:[n * 0.125, w + 0.5, 0.25, 1]
end
""", "no pixel ever leaves by itself: the wave-uniform bound ends the loop for all of them"),
    ("lane_phi",
     """filter t ()
  n = 0; w = x; v = y;
  while (w * w + v * v < 4) && (n < 8) do u = w * w - v * v + x * 1.5; v = 2 * w * v + y * 1.5; w = u; n = n + 1 end;
  rgba:[w * 0.2 + 0.5, v * 0.2 + 0.5, 0.25, 1]
end
""", "per-lane float phis read after the loop, the induction variable not"),
    ("iv_and_lane_phi",
     """filter t ()
  n = 0; w = x; v = y;
  while (w * w + v * v < 4) && (n < 8) do u = w * w - v * v + x * 1.5; v = 2 * w * v + y * 1.5; w = u; n = n + 1 end;
  rgba:[n * 0.125, w * 0.2 + 0.5, v * 0.2 + 0.5, 1]
end
""", "the induction variable and per-lane phis all read after the loop"),
    ("if_in_body",
     """filter t ()
  n = 0; w = x; c = 0;
  while (w * w < 4) && (n < 8) do
    c = if w < 0 then c + 1 else c end;
    w = if w < 0 then w * w + y else w * 1.5 - x * y + 0.3 end;
    n = n + 1
  end;
  rgba:[n * 0.125, w * 0.2 + 0.5, c * 0.125, 1]
end
""", "an `if` with phis inside the loop body (c counts the iterations that took its `then` side)"),
    ("prestep_bound",
     """filter t ()
  n = 0; m = 0; w = x;
  while (w * w < 4) && (m < 6) do w = w * w + y; m = n; n = n + 1 end;
  rgba:[n * 0.125, w * 0.1 + 0.5, m * 0.125, 1]
end
""", "the uniform bound compares the induction variable's value from before its step (a loop phi as the operand of the "
     "comparison that is made at the back edge)"),
    ("two_loops",
     """filter t ()
  n = 0; w = x;
  while (w * w < 4) && (n < 5) do w = w * w + y * 1.2; n = n + 1 end;
  m = 0; q = w * 0.25;
  while (q * q < 3) && (m < n + 2) do q = q * q + x + 0.4; m = m + 1 end;
  rgba:[n * 0.125, m * 0.125, q * 0.2 + 0.5, 1]
end
""", "two loops in sequence, the second starting from and bounded by the first's exit values"),
    ("uniform_in_if",
     """filter t ()
  n = 0; w = x; q = 0;
  while (w * w < 4) && (n < 6) do
    q = if (n < 3) && (w < y) then q + w else q - 0.25 end;
    w = w * w + y; n = n + 1
  end;
  rgba:[n * 0.125, q * 0.1 + 0.5, w * 0.1, 1]
end
""", "a wave-uniform truth value that is not a literal, mixed with a per-lane one inside an `if` of the body"),
    ("no_uniform_part",
     """filter t ()
  n = 0; w = x * 1.2;
  while w * w < 4 do w = w * w + 0.5 + y * y; n = n + 1 end;
  rgba:[n * 0.125, w * 0.05, 0.25, 1]
end
""", "a loop condition with no uniform part"),
]

# ragged frames: the width leaves a partial last tile column (partial exec), the odd height a last pair whose second
# row is the clamped copy of the first
SIZES = [(83, 61), (37, 7), (16, 1), (131, 77)]


def by_name(name):
    for n, src, _ in PROBES:
        if n == name:
            return src
    raise KeyError(name)


def count_channel(frame, ch=0):
    """The iteration counts a probe wrote as n * 0.125 into channel `ch` (bytes round(n * 31.875), capped at 255)."""
    import numpy as np
    return np.rint(frame[..., ch].astype(np.float64) / 31.875).astype(int)
