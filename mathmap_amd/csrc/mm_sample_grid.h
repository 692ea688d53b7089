// The sampling offsets of a grid-supersampled clip (mmhip_render_clip_sampled in include/mmhip.h states the semantics):
// a regular n-point grid inside a pixel's footprint, in the units of mmhip_set_sampling_offset.  Plain C++, so that the
// host paths, the table the fused kernel's prologue reads and a stand-alone test program (tests/test_clip_sampled_api.py)
// all take the offsets from the same text.
#pragma once

#if defined(__HIP__)
#define MM_SAMPLE_GRID_FN __attribute__((host)) __attribute__((device)) inline
#else
#define MM_SAMPLE_GRID_FN inline
#endif

enum { MM_SAMPLE_GRID_MAX = 8 };      // points per axis

// Offset a (0 <= a < n) of n along one axis: the centres of n equal cells of [-0.5, 0.5), double arithmetic, one rounding.
// n = 1 gives exactly 0.
MM_SAMPLE_GRID_FN float mm_sample_grid_offset(int a, int n) { return (float)(((double)a + 0.5) / (double)n - 0.5); }

// The index of sub-sample (j, b, a) of a frame with an sx x sy grid: a runs fastest, then b, then the shutter's j.
MM_SAMPLE_GRID_FN int mm_sample_grid_index(int j, int b, int a, int sx, int sy) { return (j * sy + b) * sx + a; }
