// What the four Y'CbCr 4:2:0 converters share (clip_yuv.hip, clip_yuv10.hip, clip_yuv_in.hip, clip_yuv10_in.hip; no other
// file includes this one): the vector types and the load and store helpers, the refusals they have in common, the
// work-item's place in a frame, and the tail of every launcher.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <cstring>
#include <string>

#include "mm_yuv.h"
#include "clip_kernels.h"

namespace mm {

typedef float yuv_f32x4 __attribute__((ext_vector_type(4)));
typedef unsigned yuv_u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned yuv_u32x2 __attribute__((ext_vector_type(2)));

// Non-temporal or plain, by the knob of the converter
template <bool NT, class T>
__device__ __forceinline__ T yuv_load(const T *p) {
    return NT ? __builtin_nontemporal_load(p) : *p;
}
template <bool NT, class T>
__device__ __forceinline__ void yuv_store(T v, T *p) {
    if (NT) __builtin_nontemporal_store(v, p);
    else *p = v;
}

// A work-item and its place: `item` of a frame's `items` (a kernel returns at once for one past the last), row pair `pair`
// of the band (of an input frame: its chroma row, first_row 0), `at` within the pair, the pair's upper pixel row r0 (even;
// a band ends on an even row or on the frame's last) and whether the frame has the lower one.  The two input kernels spell
// yuv_place out: behind it their clamped `cy - 1` compiles to other instructions than it did (DESIGN has the comparison).
struct YuvItem {
    unsigned pair, at, r0;
    bool two;
};
__device__ __forceinline__ unsigned yuv_item() { return blockIdx.x * 256u + threadIdx.x; }
__device__ __forceinline__ YuvItem yuv_place(unsigned item, unsigned per_pair, unsigned first_row, unsigned height) {
    YuvItem w;
    w.pair = item / per_pair;
    w.at = item - w.pair * per_pair;
    w.r0 = first_row + 2u * w.pair;
    w.two = w.r0 + 1u < height;
    return w;
}

// A refusal under the name of the entry point it speaks for: `return no("...")`
struct YuvRefusal {
    std::string who;
    std::string *err;
    YuvRefusal(const char *name, std::string *e) : who(std::string(name) + ": "), err(e) {}
    int operator()(const std::string &what) const {
        *err = who + what;
        return -1;
    }
};

// The refusals all four share, in their order: size, frames, matrix, range, the chroma mode where there is one (the input
// pair), siting.
inline int yuv_check_modes(const YuvRefusal &no, int width, int height, int frames, int matrix, int range, const int *chroma, int siting) {
    if (width < 1 || height < 1) return no("width and height must be at least 1, not " + std::to_string(width) + " x " + std::to_string(height));
    if (frames < 1) return no("num_frames must be at least 1");
    if (frames > 65535) return no("more than 65535 frames in one call (" + std::to_string(frames) + "); convert the clip in groups");
    if (matrix < 0 || matrix >= MM_YUV_MATRICES) return no("matrix must be MMHIP_YUV_BT601 or MMHIP_YUV_BT709 (0 or 1), not " + std::to_string(matrix));
    if (range < 0 || range >= MM_YUV_RANGES) return no("range must be MMHIP_YUV_LIMITED or MMHIP_YUV_FULL (0 or 1), not " + std::to_string(range));
    if (chroma && !mm_yuv_chroma_known(*chroma))
        return no("chroma must be MMHIP_YUV_CHROMA_BILINEAR or MMHIP_YUV_CHROMA_REPLICATE (0 or 1), not " + std::to_string(*chroma));
    if (!mm_yuv_siting_known(siting))
        return no("siting must be MMHIP_YUV_SITING_CENTER or MMHIP_YUV_SITING_LEFT (0 or 1), not " + std::to_string(siting));
    return 0;
}

// The band refusals of the out pair, after those: rows, an odd first_row, an odd last_row that is not the height.
inline int yuv_check_band(const YuvRefusal &no, const YuvOutJob &j) {
    if (j.first_row < 0 || j.last_row > j.height || j.first_row >= j.last_row)
        return no("rows [" + std::to_string(j.first_row) + ", " + std::to_string(j.last_row) + ") are not rows of a frame of " + std::to_string(j.height));
    if (j.first_row & 1) return no("first_row must be even, not " + std::to_string(j.first_row));
    if ((j.last_row & 1) && j.last_row != j.height)
        return no("last_row must be even or equal to height, not " + std::to_string(j.last_row) + " of " + std::to_string(j.height));
    return 0;
}

// A stride of `what` below the bytes it has to span
inline std::string yuv_short_stride(const char *stride, int64_t value, const char *what, int64_t bytes) {
    return std::string(stride) + " " + std::to_string(value) + " is smaller than one " + what + " (" + std::to_string(bytes) + " bytes)";
}

// A knob of the environment, read per call: whether `name` is set to `value`
inline bool yuv_knob_is(const char *name, const char *value) {
    const char *text = getenv(name);
    return text && !strcmp(text, value);
}

// The tail of every launcher: `items` work-items a frame in workgroups of 256 by `frames` grid rows, `launch(grid)` timed
// through ws.timed_launch as `label`, *path (may be null) 0 for the aligned path and 1 for the other.
template <class Launch>
int yuv_launch(const char *name, const char *label, unsigned items, int frames, bool aligned, NativeWorkspace &ws, hipStream_t s, int *path,
               std::string *err, Launch launch) {
    const dim3 grid((items + 255u) / 256u, (unsigned)frames);
    ws.timed_launch(label, s, [&] { launch(grid); });
    if (hipGetLastError() != hipSuccess) {
        *err = std::string(name) + ": kernel launch failed";
        return -1;
    }
    if (path) *path = aligned ? 0 : 1;
    return 0;
}

}  // namespace mm
