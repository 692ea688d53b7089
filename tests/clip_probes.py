"""Probe filters of the clip-rendering tests (tests/test_render_clip_api.py, tests/test_gpu_render_clip.py)."""

# a wave distortion whose per-row slice reads t
WAVE = "filter wave (image in, float amp: 0-1 (0.1)) in(xy + xy:[sin(y * 10 + t * 6) * amp, 0]) end"
# a fetch behind 80 statements of exact arithmetic: past the generator's limit for four pixels per step, below the one for
# the large-body kernel (hipgen.cpp auto_unroll)
MEDIUM = "\n".join(["filter medium (image in)", "  a0 = x;"] + ["  a%d = a%d * 0.5 + %d * y * 0.0001;" % (i, i - 1, i % 7) for i in range(1, 80)] +
                   ["  in(xy * 1.1 + xy:[a79 * 0.01, t * 0.1])", "end"]) + "\n"
