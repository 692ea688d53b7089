"""Adaptive anti-aliasing (mmhip_render_clip_adaptive in include/mmhip.h) restated in NumPy: the clamp, the refine rule
over the 8 neighbours inside the rendered rectangle, and the choice between two renders.  float32 throughout."""
import numpy as np

f32 = np.float32


def clamp(v):
    """c(v) = v < 0 ? 0 : (v > 1 ? 1 : v): NaN stays NaN, +inf becomes 1, -inf 0."""
    v = np.asarray(v, f32)
    with np.errstate(invalid="ignore"):
        return np.where(v < 0, f32(0), np.where(v > 1, f32(1), v)).astype(f32)


def mask(base, threshold):
    """bool [rows, cols]: the refined pixels of the float map `base` [rows, cols, 4] -- the rendered rectangle, no more."""
    base = np.asarray(base, f32)
    rows, cols = base.shape[:2]
    thr = f32(threshold)
    assert thr == thr, "the threshold is not NaN"
    refined = np.full((rows, cols), bool(thr < 0))
    c = clamp(base)
    with np.errstate(invalid="ignore"):
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                if dx == 0 and dy == 0:
                    continue
                # p over [y0:y1, x0:x1], q = p + (dy, dx) inside the rectangle
                y0, y1, x0, x1 = max(0, -dy), rows - max(0, dy), max(0, -dx), cols - max(0, dx)
                if y1 <= y0 or x1 <= x0:
                    continue
                p, q = c[y0:y1, x0:x1], c[y0 + dy:y1 + dy, x0 + dx:x1 + dx]
                contrast = np.abs((p - q).astype(f32))                  # one f32 subtraction; NaN - anything is NaN
                refined[y0:y1, x0:x1] |= ~(contrast <= thr).all(axis=2)     # !(|..| <= T) in some channel: a NaN refines
    return refined


def select(refined, aa_px, plain_px):
    """where(mask, aa, plain) on pixels [rows, cols, channels]: floats or bytes."""
    return np.where(np.asarray(refined)[:, :, None], aa_px, plain_px)
