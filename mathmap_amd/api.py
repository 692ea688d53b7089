"""Python mirror of the reference's session interface for the per-pixel path.

Names follow the reference: a *filter* is compiled (``compile_mathmap``,
mathmap_common.c:503), *invoked* on a canvas size (``invoke_mathmap``, :746), user
values are set like the CLI's ``-Dname=value`` (mathmap_cmdline.c:756-796) and frames
are rendered (``call_invocation_parallel_and_join``, :1008).  All compute happens in
libmathmap_hip.so on the GPU.
"""
import ctypes as C
import json

import numpy as np

from ._lib import Options, UservalInfo, lib

UV_INT, UV_FLOAT, UV_BOOL, UV_COLOR, UV_CURVE, UV_GRADIENT, UV_IMAGE = range(7)
# mmhip_options.gauss_mode (include/mmhip.h)
GAUSS_MODES = {"exact": 0, "tolerance": 1}
# mmhip_set_native_input_frame's modes
NATIVE_INPUT_FRAMES = {"zero": 0, "current": 1}
EDGE_COLOR, EDGE_WRAP, EDGE_REFLECT, EDGE_ROTATE = range(4)
# mmhip_filter_launch_geometry's out[] (include/mmhip.h)
GEOMETRY_FIELDS = ("tiles_x", "tiles_y", "wg1", "nwg", "ppt", "tile_w", "tile_h", "unroll", "pair_mode", "single_pixel",
                   "xcd_order", "tiles_magic", "xcd_full")
# mmhip_filter_clip_batch_plan's out[]
CLIP_PLAN_FIELDS = ("grid_x", "frames_per_batch", "batches", "shared_slot")
# mmhip_filter_clip_native_plan's out[]
CLIP_NATIVE_PLAN_FIELDS = ("eligible", "frames_per_batch", "batches", "bytes_per_frame")
# mmhip_filter_clip_supersample_plan's out[]
CLIP_SS_PLAN_FIELDS = ("batched", "frames_per_batch", "batches", "bytes_per_frame", "long_pitch", "rows_per_item", "pixels_per_item")
# mmhip_filter_clip_shutter_plan's out[]
CLIP_SHUTTER_PLAN_FIELDS = ("frames_per_batch", "batches", "samples_per_pass", "passes", "bytes_per_sample", "carry")
SHUTTER_MAX_SAMPLES = 256
# mmhip_filter_clip_shutter_fused_plan's out[]
CLIP_SHUTTER_FUSED_PLAN_FIELDS = ("fused", "frames_per_batch", "batches", "slots_per_batch", "grid_x")
# render_clip's shutter_mode: the sub-sample maps of mmhip_render_clip_shutter, or mmhip_render_clip_shutter_fused
SHUTTER_MODES = ("maps", "fused")
AA_REFINE_MODES = ("list", "select")      # mmhip_render_clip_adaptive's mode 0 (auto) and 1
CLIP_ADAPTIVE_PLAN_FIELDS = ("list_path", "frames_per_batch", "batches", "bytes_per_frame", "refine_grid_x")
CLIP_SAMPLED_PLAN_FIELDS = ("frames_per_batch", "batches", "steps_per_pass", "passes", "bytes_per_sample", "carry")
SAMPLE_GRID_MAX = 8
# render_clip's aa_filter: mmhip_render_clip_filtered's kernels, and the radius (pixels) each has when none is given
AA_FILTERS = {"box": 0, "tent": 1, "gaussian": 2, "mitchell": 3}
AA_FILTER_RADII = {"box": 0.5, "tent": 1.0, "gaussian": 1.5, "mitchell": 2.0}
AA_RADIUS_MIN, AA_RADIUS_MAX = 0.5, 4.0
# mmhip_filter_clip_filtered_plan's out[]
CLIP_FILTERED_PLAN_FIELDS = CLIP_SAMPLED_PLAN_FIELDS + ("halo_columns", "halo_rows")
# render_clip's pixel_format, yuv_matrix and yuv_range: mmhip_clip_to_yuv420's modes; "yuv420p10" is
# mmhip_clip_float_to_yuv420p10's 10-bit form, one uint16 per sample
PIXEL_FORMATS = ("yuv420p", "yuv420p10")
YUV_MATRICES = {"bt601": 0, "bt709": 1}
YUV_RANGES = {"limited": 0, "full": 1}
# set_image_yuv420's and clip_from_yuv420's chroma: mmhip_clip_from_yuv420's modes
YUV_CHROMAS = {"bilinear": 0, "replicate": 1}
# the `chroma_siting` keyword: where a chroma sample lies in its 2 x 2 block (the mmhip_..._sited entry points)
YUV_SITINGS = {"center": 0, "left": 1}
# the RGBA8 staging buffer of render_clip(pixel_format=...) unless MMHIP_CLIP_YUV_BYTES says otherwise
CLIP_YUV_BYTES = 1 << 30


def sample_grid(aa):
    """render_clip's `aa` as the pair (sx, sy): an int n means (n, n).  ValueError outside 1 .. 8."""
    try:
        sx, sy = (aa, aa) if isinstance(aa, (int, np.integer)) and not isinstance(aa, bool) else aa
        ok = all(isinstance(v, (int, np.integer)) and not isinstance(v, bool) for v in (sx, sy))
    except (TypeError, ValueError):
        ok = False
    if not ok or not (1 <= sx <= SAMPLE_GRID_MAX and 1 <= sy <= SAMPLE_GRID_MAX):
        raise ValueError("render_clip: aa is an int or a pair (sx, sy) of ints from 1 to %d, not %r" % (SAMPLE_GRID_MAX, aa))
    return int(sx), int(sy)


class MathMapError(RuntimeError):
    pass


def aa_filter_kernel(aa_filter, aa_radius=None):
    """render_clip's `aa_filter` and `aa_radius` as mmhip_render_clip_filtered's (kernel, radius): the name's constant and
    the given radius, or the name's default.  ValueError for an unknown name and a radius outside 0.5 .. 4."""
    if not isinstance(aa_filter, str) or aa_filter not in AA_FILTERS:
        raise ValueError("render_clip: aa_filter must be one of %s, not %r" % (", ".join(AA_FILTERS), aa_filter))
    radius = AA_FILTER_RADII[aa_filter] if aa_radius is None else aa_radius
    try:
        radius = float(np.float32(radius))
    except (TypeError, ValueError):
        radius = float("nan")
    if not AA_RADIUS_MIN <= radius <= AA_RADIUS_MAX:
        raise ValueError("render_clip: aa_radius must be %g to %g pixels, not %r" % (AA_RADIUS_MIN, AA_RADIUS_MAX, aa_radius))
    return AA_FILTERS[aa_filter], radius


def clip_filter_taps(aa_filter, n, lo, hi, aa_radius=None):
    """The normalised float32 taps of one axis of render_clip(aa_filter=...) with n grid points, for a pixel with `lo`
    neighbours before it and `hi` after it inside the frame (mmhip_clip_filter_taps): an array [2 D + 1, n], entry [dx + D,
    a] the weight of tap (dx, a), 0 where the tap does not exist.  Needs no GPU."""
    kernel, radius = aa_filter_kernel(aa_filter, aa_radius)
    out = np.zeros(9 * SAMPLE_GRID_MAX, dtype=np.float32)
    got = lib().mmhip_clip_filter_taps(kernel, radius, int(n), int(lo), int(hi), out.ctypes.data_as(C.POINTER(C.c_float)))
    if got < 0:
        raise MathMapError(_err())
    return out[:got].reshape(-1, int(n)).copy()


def _err():
    return lib().mmhip_last_error().decode("utf-8", "replace")


def yuv_mode(yuv_matrix, yuv_range):
    """render_clip's `yuv_matrix` and `yuv_range` as mmhip_clip_to_yuv420's (matrix, range).  ValueError for an unknown name."""
    if not isinstance(yuv_matrix, str) or yuv_matrix not in YUV_MATRICES:
        raise ValueError("yuv_matrix must be one of %s, not %r" % (", ".join(YUV_MATRICES), yuv_matrix))
    if not isinstance(yuv_range, str) or yuv_range not in YUV_RANGES:
        raise ValueError("yuv_range must be one of %s, not %r" % (", ".join(YUV_RANGES), yuv_range))
    return YUV_MATRICES[yuv_matrix], YUV_RANGES[yuv_range]


def yuv_chroma(chroma):
    """set_image_yuv420's `chroma` as mmhip_clip_from_yuv420's mode.  ValueError for an unknown name."""
    if not isinstance(chroma, str) or chroma not in YUV_CHROMAS:
        raise ValueError("chroma must be one of %s, not %r" % (", ".join(YUV_CHROMAS), chroma))
    return YUV_CHROMAS[chroma]


def yuv_siting(chroma_siting):
    """The `chroma_siting` keyword as the mmhip_..._sited entry points' siting: "center" (C420jpeg, the default everywhere) or
    "left" (C420mpeg2, what video streams carry).  ValueError for another value.
    Callers take the _sited entry point only for "left": with "center" they make the call they always made, so that its
    refusals keep speaking with the unsited function's name (the bytes are the same either way)."""
    if not isinstance(chroma_siting, str) or chroma_siting not in YUV_SITINGS:
        raise ValueError("chroma_siting must be one of %s, not %r" % (", ".join(YUV_SITINGS), chroma_siting))
    return YUV_SITINGS[chroma_siting]


def _yuv_entry(name, siting, at):
    """mmhip_<name>, or for a `siting` other than centre mmhip_<name>_sited with the siting spliced in as argument `at` (the
    handle is argument 0): one call site for both."""
    if not siting:
        return getattr(lib(), "mmhip_" + name)
    sited = getattr(lib(), "mmhip_" + name + "_sited")
    return lambda *args: sited(*args[:at], siting, *args[at:])


def _pixel_format_of(who, buf, pixel_format):
    """The format of the frames `buf`: `pixel_format` where given, else by the dtype (uint16: "yuv420p10").  ValueError for an
    unknown name or a dtype the format does not have."""
    if pixel_format is None:
        pixel_format = "yuv420p10" if buf.dtype.kind == "u" and buf.dtype.itemsize == 2 else "yuv420p"
    if pixel_format not in PIXEL_FORMATS:
        raise ValueError("%s: pixel_format must be one of %s, not %r" % (who, ", ".join(PIXEL_FORMATS), pixel_format))
    return pixel_format


def yuv420_frame_bytes(w, h, pixel_format="yuv420p"):
    """The bytes of one w x h frame as planar 4:2:0 (mmhip_yuv420_frame_bytes): w * h + 2 * cw * ch, and twice that for
    `pixel_format`="yuv420p10" (mmhip_yuv420p10_frame_bytes).  Needs no GPU."""
    if pixel_format not in PIXEL_FORMATS:
        raise ValueError("yuv420_frame_bytes: pixel_format must be one of %s, not %r" % (", ".join(PIXEL_FORMATS), pixel_format))
    n = (lib().mmhip_yuv420p10_frame_bytes if pixel_format == "yuv420p10" else lib().mmhip_yuv420_frame_bytes)(int(w), int(h))
    if n < 0:
        raise MathMapError(_err())
    return n


def yuv420_planes(buf, w, h, pixel_format=None):
    """The planes of frames as render_clip(pixel_format="yuv420p") returns them: `buf` is uint8 [N, frame_bytes] (or one
    frame, [frame_bytes]); returns the views (Y [N, h, w], Cb [N, ch, cw], Cr [N, ch, cw]).  The frames of "yuv420p10" are
    uint16 [N, frame_bytes / 2]: told by the dtype, or by `pixel_format`, which the dtype must then agree with."""
    buf = np.asarray(buf)
    if buf.ndim == 1:
        buf = buf[None]
    cw, ch = (w + 1) >> 1, (h + 1) >> 1
    dtype = np.uint16 if _pixel_format_of("yuv420_planes", buf, pixel_format) == "yuv420p10" else np.uint8
    if buf.dtype.kind != "u" or buf.dtype.itemsize != np.dtype(dtype).itemsize or buf.ndim != 2 or buf.shape[1] < w * h + 2 * cw * ch:
        raise ValueError("yuv420_planes: %s [N, %d] for frames of %d x %d, not %s %r"
                         % (np.dtype(dtype).name, w * h + 2 * cw * ch, w, h, buf.dtype, buf.shape))
    n = buf.shape[0]
    y = buf[:, :w * h].reshape(n, h, w)
    cb = buf[:, w * h:w * h + cw * ch].reshape(n, ch, cw)
    cr = buf[:, w * h + cw * ch:w * h + 2 * cw * ch].reshape(n, ch, cw)
    return y, cb, cr


def y4m_header(w, h, fps=(25, 1), yuv_range="limited", pixel_format="yuv420p", chroma_siting="center"):
    """The stream header of a YUV4MPEG2 file (mmhip_y4m_header; for `pixel_format`="yuv420p10" mmhip_y4m_header_p10) as
    bytes.  Needs no GPU.  `chroma_siting`="left" tags an 8-bit stream C420mpeg2 (mmhip_y4m_header_sited); C420p10 has no
    tag for it and stays as it is."""
    siting = yuv_siting(chroma_siting)
    if yuv_range not in YUV_RANGES:
        raise ValueError("yuv_range must be one of %s, not %r" % (", ".join(YUV_RANGES), yuv_range))
    if pixel_format not in PIXEL_FORMATS:
        raise ValueError("y4m_header: pixel_format must be one of %s, not %r" % (", ".join(PIXEL_FORMATS), pixel_format))
    num, den = (fps, 1) if isinstance(fps, (int, np.integer)) else fps
    line = C.create_string_buffer(160)
    header = lib().mmhip_y4m_header_p10 if pixel_format == "yuv420p10" else lib().mmhip_y4m_header
    if siting:
        n = lib().mmhip_y4m_header_sited(line, 160, int(w), int(h), int(num), int(den), YUV_RANGES[yuv_range], 10 if pixel_format == "yuv420p10" else 8,
                                         siting)
    else:
        n = header(line, 160, int(w), int(h), int(num), int(den), YUV_RANGES[yuv_range])
    if n < 0:
        raise MathMapError(_err())
    return line.raw[:n]


def write_y4m(path_or_file, buf, w, h, fps=(25, 1), yuv_range="limited", pixel_format=None, chroma_siting="center"):
    """Writes frames as render_clip(pixel_format="yuv420p") returns them (uint8 [N, frame_bytes]) as one YUV4MPEG2 file:
    the header, then "FRAME\\n" and the payload per frame.  `path_or_file`: a file name, or a binary file object (which
    stays open).  `fps` = n or (n, d).  The colour matrix has no place in the format: tell the encoder.  The frames of
    "yuv420p10" (uint16 [N, frame_bytes / 2], told by the dtype or by `pixel_format`) go out as C420p10, every sample as
    two bytes, the low one first.  `chroma_siting` names the siting the frames were converted with: "left" writes the tag
    C420mpeg2 for 8-bit frames (y4m_header); the payloads are written as they are."""
    yuv_siting(chroma_siting)
    buf = np.asarray(buf)
    if buf.ndim == 1:
        buf = buf[None]
    pixel_format = _pixel_format_of("write_y4m", buf, pixel_format)
    dtype = np.uint16 if pixel_format == "yuv420p10" else np.uint8
    samples = yuv420_frame_bytes(w, h)
    if buf.dtype.kind != "u" or buf.dtype.itemsize != np.dtype(dtype).itemsize or buf.ndim != 2 or buf.shape[1] != samples:
        raise ValueError("write_y4m: %s [N, %d] for frames of %d x %d, not %s %r" % (np.dtype(dtype).name, samples, w, h, buf.dtype, buf.shape))
    if dtype == np.uint16:
        buf = buf.astype("<u2", copy=False)
    header = y4m_header(w, h, fps, yuv_range, pixel_format, chroma_siting)
    f = open(path_or_file, "wb") if isinstance(path_or_file, (str, bytes)) or hasattr(path_or_file, "__fspath__") else path_or_file
    try:
        f.write(header)
        for frame in buf:
            f.write(b"FRAME\n")
            f.write(np.ascontiguousarray(frame).tobytes())
    finally:
        if f is not path_or_file:
            f.close()


def y4m_parse_header(data):
    """The stream header at the start of `data` (bytes) of a YUV4MPEG2 file (mmhip_y4m_parse_header): (w, h, (fps_num,
    fps_den), yuv_range or None, header_len).  Needs no GPU.  ValueError, by name, for what the reader does not take."""
    data = bytes(data)
    out = [C.c_int(0) for _ in range(6)]
    if lib().mmhip_y4m_parse_header(data, len(data), *[C.byref(v) for v in out]) != 0:
        raise ValueError(_err())
    w, h, num, den, rng, header_len = [v.value for v in out]
    names = {v: k for k, v in YUV_RANGES.items()}
    return w, h, (num, den), names.get(rng), header_len


def y4m_parse_stream_header(data):
    """y4m_parse_header for streams of either depth (mmhip_y4m_parse_stream_header): (w, h, (fps_num, fps_den), yuv_range or
    None, header_len, pixel_format), the last "yuv420p" or, for the colour space C420p10, "yuv420p10".  Needs no GPU.
    ValueError, by name, for what the reader does not take."""
    data = bytes(data)
    out = [C.c_int(0) for _ in range(7)]
    if lib().mmhip_y4m_parse_stream_header(data, len(data), *[C.byref(v) for v in out]) != 0:
        raise ValueError(_err())
    w, h, num, den, rng, bits, header_len = [v.value for v in out]
    names = {v: k for k, v in YUV_RANGES.items()}
    return w, h, (num, den), names.get(rng), header_len, "yuv420p10" if bits == 10 else "yuv420p"


def y4m_chroma_siting(data_or_path):
    """The chroma siting a YUV4MPEG2 stream header states (mmhip_y4m_stream_siting): "left" for C420mpeg2, "center" for no C
    tag, C420, C420jpeg, C420paldv (not modelled) and C420p10 (which cannot say).  `data_or_path`: the stream's first bytes
    (bytes, bytearray or memoryview), or a file name, whose first line is read.  Needs no GPU.  ValueError, by name, for what
    y4m_parse_stream_header refuses."""
    if isinstance(data_or_path, (bytes, bytearray, memoryview)):
        data = bytes(data_or_path)
    else:
        with open(data_or_path, "rb") as f:
            data = f.readline(4096)
    siting = C.c_int(0)
    if lib().mmhip_y4m_stream_siting(data, len(data), C.byref(siting)) != 0:
        raise ValueError(_err())
    return {v: k for k, v in YUV_SITINGS.items()}[siting.value]


def read_y4m(path_or_file, max_frames=None, pixel_format="yuv420p"):
    """Reads a YUV4MPEG2 file of 8-bit 4:2:0 frames -- what write_y4m writes, and what video decoders emit: returns (yuv
    uint8 [N, frame_bytes], w, h, fps (num, den), yuv_range or None), the first value being what set_image_yuv420 takes
    and yuv_range "limited" or "full" where the header states XCOLORRANGE.  `path_or_file`: a file name, or a binary
    file object (which stays open; a pipe will do).  `max_frames` caps the frames read.  A FRAME line may carry
    parameters.  ValueError, by name: a header the reader does not take, a line that is not FRAME where a frame should
    begin, a truncated last frame, a file with no frames.
    `pixel_format`="yuv420p10" reads streams of colour space C420p10 only and returns uint16 [N, frame_bytes / 2], what
    set_image_yuv420p10 takes (the file's samples are little-endian whatever the host); an 8-bit stream is a ValueError
    then.  "any" reads either depth: the array's dtype tells which."""
    if max_frames is not None and int(max_frames) < 1:
        raise ValueError("read_y4m: max_frames must be at least 1, not %r" % (max_frames,))
    if pixel_format not in PIXEL_FORMATS + ("any",):
        raise ValueError("read_y4m: pixel_format must be one of %s, not %r" % (", ".join(PIXEL_FORMATS + ("any",)), pixel_format))
    f = open(path_or_file, "rb") if isinstance(path_or_file, (str, bytes)) or hasattr(path_or_file, "__fspath__") else path_or_file
    try:
        header = f.readline(4096)
        if pixel_format == "yuv420p":
            w, h, fps, yuv_range, _ = y4m_parse_header(header)
            found = "yuv420p"
        else:
            w, h, fps, yuv_range, _, found = y4m_parse_stream_header(header)
            if pixel_format == "yuv420p10" and found != "yuv420p10":
                raise ValueError("read_y4m: pixel_format=\"yuv420p10\" reads streams of colour space C420p10, and this one holds 8-bit samples")
        frame_bytes = yuv420_frame_bytes(w, h, found)
        frames = []
        while max_frames is None or len(frames) < int(max_frames):
            line = f.readline(4096)
            if not line:
                break
            if not (line.startswith(b"FRAME") and line.endswith(b"\n") and line[5:6] in (b" ", b"\n")):
                raise ValueError("read_y4m: frame %d does not begin with a FRAME line but with %r" % (len(frames), line[:16]))
            payload = bytearray()
            while len(payload) < frame_bytes:          # (a pipe may deliver less than asked for)
                piece = f.read(frame_bytes - len(payload))
                if not piece:
                    break
                payload += piece
            if len(payload) != frame_bytes:
                raise ValueError("read_y4m: frame %d is truncated: %d of %d bytes" % (len(frames), len(payload), frame_bytes))
            frames.append(np.frombuffer(bytes(payload), "<u2").astype(np.uint16) if found == "yuv420p10" else np.frombuffer(bytes(payload), np.uint8))
        if not frames:
            raise ValueError("read_y4m: the file has no frames")
        return np.stack(frames), w, h, fps, yuv_range
    finally:
        if f is not path_or_file:
            f.close()


def shutter_sample_ts(ts, samples, span):
    """The times of a motion-blurred clip's sub-samples (mmhip_render_clip_shutter): float32 [N, samples], entry [i, j] =
    (float)((double)ts[i] + ((double)span * (double)j) / (double)samples), with ts and span taken as float32."""
    samples = int(samples)
    if not 1 <= samples <= SHUTTER_MAX_SAMPLES:
        raise ValueError("shutter_sample_ts: samples must be 1 to %d, not %d" % (SHUTTER_MAX_SAMPLES, samples))
    ts = np.asarray(ts, dtype=np.float32).reshape(-1).astype(np.float64)
    j = np.arange(samples, dtype=np.float64)
    return (ts[:, None] + (np.float64(np.float32(span)) * j)[None, :] / np.float64(samples)).astype(np.float32)


class Filter:
    """A compiled .mm filter (front-end + IR + generated HIP kernel string)."""

    def __init__(self, source="", intersample=True, supersampling=False, edge_x=EDGE_COLOR, edge_y=EDGE_COLOR,
                 tile_w=0, specialize=False, constants=None, ir_json=None, _handle=None, pixel_inc=1, gauss_mode="exact",
                 deep_inputs=False):
        """`source`: .mm text; or `ir_json`: an IR dump (mmhip_filter_ir_json_raw / the reference-ABI importer's
        form) -- the IR-level entry point.  `constants` (name -> number) bakes scalar user values in as literals.
        `pixel_inc` > 1: the bilinear fetch interpolates over a source sampled at that stride (the GIMP preview's
        fast image source, builtins.c:186-216).  `gauss_mode`: "exact" (default), or "tolerance" -- gaussian_blur's
        faster chain, within 1 per RGBA8 channel of exact, where the render writes the blur's bytes directly (the
        conditions are stated at mmhip_options.gauss_mode in include/mmhip.h).  `deep_inputs`: the kernels can fetch
        float32 input drawables (Invocation.set_image with a float32 array, set_image_device_float); off by default,
        and then the generated text is what it is without the option."""
        if gauss_mode not in GAUSS_MODES:
            raise MathMapError("gauss_mode must be one of %s, not %r" % (", ".join(sorted(GAUSS_MODES)), gauss_mode))
        self._source = source
        self._kwargs = dict(intersample=intersample, supersampling=supersampling, edge_x=edge_x, edge_y=edge_y,
                            tile_w=tile_w, pixel_inc=pixel_inc, gauss_mode=gauss_mode, deep_inputs=deep_inputs)
        if _handle is not None:
            self._h = _handle
            return
        o = Options()
        lib().mmhip_default_options(C.byref(o))
        o.intersample = 1 if intersample else 0
        o.supersampling = 1 if supersampling else 0
        o.edge_behaviour_x, o.edge_behaviour_y = edge_x, edge_y
        o.tile_w = tile_w
        o.pixel_inc = pixel_inc
        o.specialize_uservals = 1 if specialize else 0
        o.gauss_mode = GAUSS_MODES[gauss_mode]
        o.deep_inputs = 1 if deep_inputs else 0
        if ir_json is not None:
            self._h = lib().mmhip_compile_ir_json(ir_json.encode(), C.byref(o))
        else:
            self._h = lib().mmhip_compile(source.encode(), C.byref(o))
        if not self._h:
            raise MathMapError(_err())
        if constants:
            # bake scalar user values in as literals (the variant the specialising JIT builds lazily)
            base, self._h = self._h, None
            try:
                self._h = self._specialized_handle(base, constants)
            finally:
                lib().mmhip_filter_free(base)

    @staticmethod
    def _specialized_handle(handle, constants):
        names = {}
        for i in range(lib().mmhip_filter_num_uservals(handle)):
            info = UservalInfo()
            lib().mmhip_filter_userval_info(handle, i, C.byref(info))
            names[info.name.decode()] = i
        for k in constants:
            if k not in names:
                raise MathMapError("filter has no user value `%s'" % k)
        idx = (C.c_int * len(constants))(*[names[k] for k in constants])
        val = (C.c_double * len(constants))(*[float(v) for v in constants.values()])
        h = lib().mmhip_filter_specialized(handle, len(constants), idx, val)
        if not h:
            raise MathMapError(_err())
        return h

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            lib().mmhip_filter_free(h)

    @property
    def name(self):
        return lib().mmhip_filter_name(self._h).decode()

    @property
    def uservals(self):
        out = []
        for i in range(lib().mmhip_filter_num_uservals(self._h)):
            info = UservalInfo()
            lib().mmhip_filter_userval_info(self._h, i, C.byref(info))
            out.append(dict(kind=info.kind, index=info.index, name=info.name.decode(),
                            int_min=info.int_min, int_max=info.int_max, int_default=info.int_default,
                            float_min=info.float_min, float_max=info.float_max, float_default=info.float_default,
                            bool_default=info.bool_default, image_flags=info.image_flags))
        return out

    @property
    def ir(self):
        return json.loads(lib().mmhip_filter_ir_json(self._h).decode())

    @property
    def ir_json(self):
        return lib().mmhip_filter_ir_json(self._h).decode()

    @property
    def ir_json_raw(self):
        """The IR before any optimisation pass (what mmhip_compile_ir_json takes and the test
        oracle prints): lowering output only."""
        return lib().mmhip_filter_ir_json_raw(self._h).decode()

    def specialized(self, values=None):
        """The variant with every int/float/bool user value baked in: the declared defaults,
        overridden by `values` (name -> number).  What a render with those values runs."""
        consts = {}
        for u in self.uservals:
            if u["kind"] == UV_INT:
                consts[u["name"]] = u["int_default"]
            elif u["kind"] == UV_FLOAT:
                consts[u["name"]] = u["float_default"]
            elif u["kind"] == UV_BOOL:
                consts[u["name"]] = u["bool_default"]
        for k, v in (values or {}).items():
            if k in consts:
                consts[k] = v
        return Filter(self._source, _handle=self._specialized_handle(self._h, consts), **self._kwargs)

    @property
    def kernel_source(self):
        return lib().mmhip_filter_kernel_source(self._h).decode()

    @property
    def gauss_mode(self):
        """The gauss_mode the library compiled this filter with: "exact" or "tolerance"."""
        mode = lib().mmhip_filter_gauss_mode(self._h)
        return {v: k for k, v in GAUSS_MODES.items()}[mode]

    @property
    def deep_inputs(self):
        """Whether the library compiled this filter's kernels with the float32 drawable fetch (mmhip_options.deep_inputs)."""
        return bool(lib().mmhip_filter_deep_inputs(self._h))

    @property
    def num_native_calls(self):
        return lib().mmhip_filter_num_native_calls(self._h)

    @property
    def builtin_ids(self):
        """The ids of the builtin overloads and macros the parser resolved for this filter's text (a frozenset;
        empty for a filter built from an IR dump)."""
        n = lib().mmhip_filter_builtin_ids(self._h, None, 0)
        buf = C.create_string_buffer(n)
        lib().mmhip_filter_builtin_ids(self._h, buf, n)
        return frozenset(buf.value.decode().split())

    def launch_geometry(self, region_w, num_rows, closure=None):
        """How the pixel kernel is launched over `num_rows` rows of a `region_w`-wide region (the geometry mmhip_render
        takes, MMHIP_PPT included) -- or, with `closure` = k, how closure image #k is launched over a region_w x
        num_rows frame.  A dict of the GEOMETRY_FIELDS."""
        if closure is None:
            return self._plan("mmhip_filter_launch_geometry", GEOMETRY_FIELDS, region_w, num_rows)
        return self._plan("mmhip_filter_closure_launch_geometry", GEOMETRY_FIELDS, closure, region_w, num_rows)

    def _plan(self, symbol, fields, *args):
        """What the library's plan function `symbol` writes for `args`: a dict of `fields`."""
        out = (C.c_int64 * len(fields))()
        if getattr(lib(), symbol)(self._h, *args, out) != 0:
            raise MathMapError(_err())
        return dict(zip(fields, out))

    def _variant(self, symbol, *args):
        """A module variant's text (decoded) or code-object size from the library function `symbol`; no text, or a
        negative size, is the library's refusal: MathMapError."""
        got = getattr(lib(), symbol)(self._h, *args)
        if got is None or (not isinstance(got, bytes) and got < 0):
            raise MathMapError(_err())
        return got.decode() if isinstance(got, bytes) else got

    def clip_launch_geometry(self, region_w, num_rows, frames):
        """The geometry of one frame of a `frames`-frame clip render (render_clip): GEOMETRY_FIELDS, with the
        rows per work-item chosen from the workgroups of all frames together; frames=1 is launch_geometry."""
        return self._plan("mmhip_filter_clip_launch_geometry", GEOMETRY_FIELDS, region_w, num_rows, frames)

    def clip_batch_plan(self, region_w, num_rows, frames):
        """How render_clip cuts a `frames`-frame clip into launches: a dict of the CLIP_PLAN_FIELDS
        (frames_per_batch 0: the filter is rendered frame by frame)."""
        return self._plan("mmhip_filter_clip_batch_plan", CLIP_PLAN_FIELDS, region_w, num_rows, frames)

    def clip_native_plan(self, region_w, num_rows, frames, render_w=None, render_h=None):
        """How render_clip batches the gaussian_blur calls of a `frames`-frame clip at render size render_w x render_h
        (default: the region's): a dict of the CLIP_NATIVE_PLAN_FIELDS (eligible 0: the filter's native calls are not
        batched; frames_per_batch 0: rendered frame by frame)."""
        rw, rh = region_w if render_w is None else render_w, num_rows if render_h is None else render_h
        return self._plan("mmhip_filter_clip_native_plan", CLIP_NATIVE_PLAN_FIELDS, region_w, num_rows, rw, rh, frames)

    def clip_shutter_plan(self, region_w, num_rows, render_w, samples, frames):
        """How render_clip(shutter_samples=samples) renders a `frames`-frame clip of num_rows rows of a region at render
        width render_w: a dict of the CLIP_SHUTTER_PLAN_FIELDS (carry 1: the sub-samples of a frame take several passes)."""
        return self._plan("mmhip_filter_clip_shutter_plan", CLIP_SHUTTER_PLAN_FIELDS, region_w, num_rows, render_w, samples, frames)

    def clip_shutter_fused_plan(self, region_w, num_rows, samples, frames):
        """How render_clip(shutter_samples=samples, shutter_mode="fused") renders a `frames`-frame clip of num_rows rows of
        a region_w-wide region: a dict of the CLIP_SHUTTER_FUSED_PLAN_FIELDS (fused 0: the filter takes the maps path)."""
        return self._plan("mmhip_filter_clip_shutter_fused_plan", CLIP_SHUTTER_FUSED_PLAN_FIELDS, region_w, num_rows, samples, frames)

    def clip_sampled_plan(self, region_w, num_rows, render_w, samples, aa, frames):
        """How render_clip(aa=aa, shutter_samples=samples) renders a `frames`-frame clip through sub-sample maps: a dict of
        the CLIP_SAMPLED_PLAN_FIELDS (steps_per_pass: time steps, of sx * sy maps each)."""
        sx, sy = sample_grid(aa)
        return self._plan("mmhip_filter_clip_sampled_plan", CLIP_SAMPLED_PLAN_FIELDS, region_w, num_rows, render_w, samples, sx, sy, frames)

    def clip_sampled_fused_plan(self, region_w, num_rows, samples, aa, frames):
        """How render_clip(aa=aa, shutter_samples=samples, shutter_mode="fused") renders a `frames`-frame clip: a dict of the
        CLIP_SHUTTER_FUSED_PLAN_FIELDS (fused 0: the filter takes the maps path)."""
        sx, sy = sample_grid(aa)
        return self._plan("mmhip_filter_clip_sampled_fused_plan", CLIP_SHUTTER_FUSED_PLAN_FIELDS, region_w, num_rows, samples, sx, sy, frames)

    def clip_adaptive_plan(self, region_w, num_rows, render_w, aa, frames):
        """How render_clip(aa=aa, aa_threshold=T) renders a `frames`-frame clip: a dict of the CLIP_ADAPTIVE_PLAN_FIELDS
        (list_path 0: the filter or the region takes the select path)."""
        sx, sy = sample_grid(aa)
        return self._plan("mmhip_filter_clip_adaptive_plan", CLIP_ADAPTIVE_PLAN_FIELDS, region_w, num_rows, render_w, sx, sy, frames)

    def clip_filtered_plan(self, region_w, num_rows, render_w, render_h, samples, aa, aa_filter, frames, aa_radius=None, region_x=0,
                           first_row=0):
        """How render_clip(aa=aa, aa_filter=aa_filter, aa_radius=aa_radius, shutter_samples=samples) renders a `frames`-frame
        clip of num_rows rows from first_row of the region_w columns from region_x of a render_w x render_h frame: a dict of
        the CLIP_FILTERED_PLAN_FIELDS (the sampled plan's over maps of the haloed rectangle, and that rectangle's size)."""
        sx, sy = sample_grid(aa)
        _, radius = aa_filter_kernel(aa_filter, aa_radius)
        return self._plan("mmhip_filter_clip_filtered_plan", CLIP_FILTERED_PLAN_FIELDS, region_x, region_w, first_row, first_row + num_rows,
                          render_w, render_h, samples, sx, sy, radius, frames)

    @property
    def refine_kernel_source(self):
        """The refine variant of kernel_source: kernels mm_prologue_clip (the sampled variant's) and mm_pixels_refine.  A
        filter without a sampled variant has none: MathMapError."""
        return self._variant("mmhip_filter_refine_kernel_source")

    def jit_refine(self, load=False):
        """hiprtc-compiles the refine variant for gfx950; returns the code-object size."""
        return self._variant("mmhip_filter_jit_refine", 1 if load else 0)

    @property
    def sampled_kernel_source(self):
        """The sampled variant of kernel_source: kernels mm_prologue_clip and mm_pixels_sampled.  A filter with native calls,
        closure images or a per-row slice has none: MathMapError."""
        return self._variant("mmhip_filter_sampled_kernel_source")

    def jit_sampled(self, load=False):
        """hiprtc-compiles the sampled variant for gfx950; returns the code-object size."""
        return self._variant("mmhip_filter_jit_sampled", 1 if load else 0)

    @property
    def shutter_kernel_source(self):
        """The shutter variant of kernel_source: kernels mm_prologue_clip, mm_rows_clip, mm_pixels_shutter.  A filter with
        native calls or closure images has none: MathMapError."""
        return self._variant("mmhip_filter_shutter_kernel_source")

    def jit_shutter(self, load=False):
        """hiprtc-compiles the shutter variant for gfx950; returns the code-object size."""
        return self._variant("mmhip_filter_jit_shutter", 1 if load else 0)

    def clip_supersample_plan(self, region_w, region_h, frames, bpp=4):
        """How render_clip(supersample=True) renders a `frames`-frame clip of a region: a dict of the CLIP_SS_PLAN_FIELDS
        (batched 0: the loop of single supersampled renders)."""
        return self._plan("mmhip_filter_clip_supersample_plan", CLIP_SS_PLAN_FIELDS, region_w, region_h, bpp, frames)

    @property
    def clip_kernel_source(self):
        """The clip variant of kernel_source: kernels mm_prologue_clip, mm_rows_clip, mm_pixels_clip."""
        return self._variant("mmhip_filter_clip_kernel_source")

    def jit_clip(self, load=False):
        """hiprtc-compiles the clip variant for gfx950; returns the code-object size."""
        return self._variant("mmhip_filter_jit_clip", 1 if load else 0)

    @property
    def num_closures(self):
        return lib().mmhip_filter_num_closures(self._h)

    def jit(self, load=False):
        """hiprtc-compiles the kernel string for gfx950; returns the code-object size."""
        return self._variant("mmhip_filter_jit", 1 if load else 0)

    @property
    def jit_seconds(self):
        return lib().mmhip_filter_jit_seconds(self._h)

    def invoke(self, width, height):
        return Invocation(self, width, height)


def as_image_sequence(array):
    """A host image ([H,W,3|4]) or image sequence ([N,H,W,3|4]) as the contiguous uint8 [N,H,W,C] array that
    mmhip_set_image_sequence_host takes."""
    a = np.ascontiguousarray(array, dtype=np.uint8)
    if a.ndim == 3:
        a = a[None]
    if a.ndim != 4 or a.shape[0] < 1:
        raise MathMapError("an image is [H,W,3|4], an image sequence [N,H,W,3|4] with N >= 1; got shape %s" % (tuple(np.shape(array)),))
    return a


IMAGE_DTYPES = "uint8 (an 8-bit drawable) or float32 (a float drawable; Filter(..., deep_inputs=True))"


def as_float_image_sequence(array):
    """A float32 host image ([H,W,3|4]) or sequence ([N,H,W,3|4]) as the contiguous [N,H,W,C] array that
    mmhip_set_image_sequence_float_host takes."""
    a = np.ascontiguousarray(array, dtype=np.float32)
    if a.ndim == 3:
        a = a[None]
    if a.ndim != 4 or a.shape[0] < 1:
        raise MathMapError("an image is [H,W,3|4], an image sequence [N,H,W,3|4] with N >= 1; got shape %s" % (tuple(np.shape(array)),))
    return a


class Invocation:
    """A filter bound to a canvas size, user values and input images (all in HBM)."""

    def __init__(self, flt, width, height):
        self.filter = flt
        self.width, self.height = width, height
        self.render_width, self.render_height = width, height
        self._h = lib().mmhip_invoke(flt._h, width, height)
        if not self._h:
            raise MathMapError(_err())
        self._keep = []

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            lib().mmhip_invocation_free(h)

    def _check(self, rc):
        if rc != 0:
            raise MathMapError(_err())

    def _index(self, name):
        for u in self.filter.uservals:
            if u["name"] == name:
                return u
        raise MathMapError("filter has no user value `%s'" % name)

    def set(self, name, value):
        """Sets a user value by name (the CLI's -Dname=value)."""
        u = self._index(name)
        k, i = u["kind"], u["index"]
        if k == UV_INT:
            self._check(lib().mmhip_set_int(self._h, i, int(value)))
        elif k == UV_FLOAT:
            self._check(lib().mmhip_set_float(self._h, i, float(value)))
        elif k == UV_BOOL:
            self._check(lib().mmhip_set_bool(self._h, i, int(bool(value))))
        elif k == UV_COLOR:
            r, g, b, a = value
            self._check(lib().mmhip_set_color(self._h, i, r, g, b, a))
        elif k == UV_IMAGE:
            self.set_image(name, value)
        else:
            raise MathMapError("cannot set user value `%s'" % name)

    def set_curve(self, name, values):
        """Sets a curve user value: 1024 floats, the sampled curve (userval.h:38,89-96)."""
        u = self._index(name)
        a = np.ascontiguousarray(values, dtype=np.float32)
        if a.shape != (1024,):
            raise MathMapError("a curve has 1024 samples")
        self._check(lib().mmhip_set_curve(self._h, u["index"], a.ctypes.data_as(C.c_void_p)))

    def set_gradient(self, name, rgba):
        """Sets a gradient user value: 1024 packed 0xRRGGBBAA colours (userval.h:39,98-101)."""
        u = self._index(name)
        a = np.ascontiguousarray(rgba, dtype=np.uint32)
        if a.shape != (1024,):
            raise MathMapError("a gradient has 1024 samples")
        self._check(lib().mmhip_set_gradient(self._h, u["index"], a.ctypes.data_as(C.c_void_p)))

    def set_image(self, name, array):
        """Binds a host uint8 array as input drawable (uploaded once to HBM): [H,W,3|4] is one image,
        [N,H,W,3|4] a sequence of N frames of one size.  in(xy, n) reads frame (int)n of it (plain
        in(xy): frame (int)t), and opaque white where there is no such frame; gaussian_blur, convolve
        and render() read frame 0 (set_native_input_frame("current"): the render's own frame).
        A float32 array of the same shapes is bound as a float drawable (mmhip_set_image_sequence_float_host: the
        texels are fetched as they are, unquantised; 3 channels get alpha 1.0) -- the filter must have been compiled
        with deep_inputs=True.  An array of any other dtype is a ValueError; what has no dtype (nested lists) is
        converted to uint8, as before."""
        u = self._index(name)
        dtype = getattr(array, "dtype", None)
        if dtype is not None and dtype == np.float32:
            a = as_float_image_sequence(array)
            n, h, w, c = a.shape
            self._check(lib().mmhip_set_image_sequence_float_host(self._h, u["index"], a.ctypes.data_as(C.c_void_p), w, h, c, n))
            return
        if dtype is not None and dtype != np.uint8:
            raise ValueError("set_image: the array's dtype must be %s, not %s" % (IMAGE_DTYPES, dtype))
        a = as_image_sequence(array)
        n, h, w, c = a.shape
        self._check(lib().mmhip_set_image_sequence_host(self._h, u["index"], a.ctypes.data_as(C.c_void_p), w, h, c, n))

    def set_image_yuv420(self, name, yuv, w, h, yuv_matrix="bt709", yuv_range="limited", chroma="bilinear", chroma_siting="center"):
        """Binds planar Y'CbCr 4:2:0 frames as input drawable: `yuv` is uint8 [N, frame_bytes] -- what read_y4m and
        render_clip(pixel_format="yuv420p") return -- or one frame, [frame_bytes], of `w` x `h` pixels.  The payloads go
        up as they are (1.5 bytes per pixel) and are expanded to the drawable's words on the GPU
        (mmhip_set_image_sequence_yuv420_host) in the mode `yuv_matrix`, `yuv_range`, with `chroma` "bilinear" (default)
        or "replicate"; alpha is 255.  From there on the sequence is what set_image binds.  `chroma_siting`="left" reads
        the chroma as co-sited with the even luma columns (C420mpeg2, what decoders emit;
        mmhip_set_image_sequence_yuv420_host_sited); "replicate" ignores it."""
        matrix, rng = yuv_mode(yuv_matrix, yuv_range)
        mode = yuv_chroma(chroma)
        siting = yuv_siting(chroma_siting)
        w, h = int(w), int(h)
        if w < 1 or h < 1:
            raise ValueError("set_image_yuv420: w and h must be at least 1, not %d x %d" % (w, h))
        frame_bytes = w * h + 2 * ((w + 1) >> 1) * ((h + 1) >> 1)
        a = np.asarray(yuv)
        if a.ndim == 1:
            a = a[None]
        if a.dtype != np.uint8 or a.ndim != 2 or a.shape[0] < 1 or a.shape[1] != frame_bytes:
            raise ValueError("set_image_yuv420: uint8 [N, %d] for frames of %d x %d, not %s %r" % (frame_bytes, w, h, a.dtype, a.shape))
        a = np.ascontiguousarray(a)
        u = self._index(name)
        self._check(_yuv_entry("set_image_sequence_yuv420_host", siting, 10)(self._h, u["index"], a.ctypes.data_as(C.c_void_p), frame_bytes, w, h,
                                                                             a.shape[0], matrix, rng, mode))

    def set_image_yuv420p10(self, name, yuv, w, h, yuv_matrix="bt709", yuv_range="limited", chroma="bilinear", chroma_siting="center"):
        """Binds 10-bit planar Y'CbCr 4:2:0 frames as float32 input drawable: `yuv` is uint16 [N, frame_bytes / 2] -- what
        read_y4m(pixel_format="yuv420p10") and render_clip(pixel_format="yuv420p10") return -- or one frame, of `w` x `h`
        pixels.  The payloads go up as they are (3 bytes per pixel) and are expanded to float4 texels on the GPU
        (mmhip_set_image_sequence_yuv420p10_host) in the mode `yuv_matrix`, `yuv_range`, with `chroma` "bilinear"
        (default) or "replicate": unclamped, alpha 1.0, no 8-bit step.  From there on the sequence is what set_image
        binds for a float32 array; the filter must have been compiled with deep_inputs=True.  `chroma_siting` as in
        set_image_yuv420 (mmhip_set_image_sequence_yuv420p10_host_sited)."""
        matrix, rng = yuv_mode(yuv_matrix, yuv_range)
        mode = yuv_chroma(chroma)
        siting = yuv_siting(chroma_siting)
        w, h = int(w), int(h)
        if w < 1 or h < 1:
            raise ValueError("set_image_yuv420p10: w and h must be at least 1, not %d x %d" % (w, h))
        samples = w * h + 2 * ((w + 1) >> 1) * ((h + 1) >> 1)
        a = np.asarray(yuv)
        if a.ndim == 1:
            a = a[None]
        if a.dtype.kind != "u" or a.dtype.itemsize != 2 or a.ndim != 2 or a.shape[0] < 1 or a.shape[1] != samples:
            raise ValueError("set_image_yuv420p10: uint16 [N, %d] for frames of %d x %d, not %s %r" % (samples, w, h, a.dtype, a.shape))
        a = np.ascontiguousarray(a, np.uint16)      # (the host's byte order, which the library reads)
        u = self._index(name)
        self._check(_yuv_entry("set_image_sequence_yuv420p10_host", siting, 10)(self._h, u["index"], a.ctypes.data_as(C.c_void_p), 2 * samples, w, h,
                                                                                a.shape[0], matrix, rng, mode))

    def clip_yuv10_input_groups(self):
        """The upload groups of the last set_image_yuv420p10 (mmhip_clip_yuv10_input_groups)."""
        return lib().mmhip_clip_yuv10_input_groups(self._h)

    def clip_from_yuv420p10_launches(self, path):
        """The launches of clip_from_yuv420p10's kernel on `path`: "aligned" or "samples" (mmhip_clip_from_yuv420p10_launches)."""
        if path not in ("aligned", "samples"):
            raise ValueError("clip_from_yuv420p10_launches: path must be \"aligned\" or \"samples\", not %r" % (path,))
        return lib().mmhip_clip_from_yuv420p10_launches(self._h, 0 if path == "aligned" else 1)

    def clip_yuv_input_groups(self):
        """The upload groups of the last set_image_yuv420 (mmhip_clip_yuv_input_groups)."""
        return lib().mmhip_clip_yuv_input_groups(self._h)

    def clip_from_yuv420_launches(self, path):
        """The launches of clip_from_yuv420's kernel on `path`: "aligned" or "bytes" (mmhip_clip_from_yuv420_launches)."""
        if path not in ("aligned", "bytes"):
            raise ValueError("path must be aligned or bytes, not %r" % (path,))
        return lib().mmhip_clip_from_yuv420_launches(self._h, 0 if path == "aligned" else 1)

    def set_image_device(self, name, device_ptr, width, height, keepalive=None, num_frames=1):
        """Binds a packed 0xRRGGBBAA uint32 image already resident in HBM; with num_frames > 1, that
        many frames of width x height one after the other ([N,H,W] uint32)."""
        u = self._index(name)
        self._check(lib().mmhip_set_image_sequence_device(self._h, u["index"], C.c_void_p(device_ptr), width, height, num_frames))
        if keepalive is not None:
            self._keep.append(keepalive)

    def set_image_device_float(self, name, device_ptr, width, height, num_frames=1, keepalive=None):
        """Binds float4 texels already resident in HBM as a float drawable: [num_frames, height, width] float4, 16-byte
        aligned, not copied (mmhip_set_image_sequence_float_device) -- the layout render_clip(floatmap=True, out_ptr=p)
        writes for whole frames.  The filter must have been compiled with deep_inputs=True."""
        u = self._index(name)
        self._check(lib().mmhip_set_image_sequence_float_device(self._h, u["index"], C.c_void_p(device_ptr), width, height, num_frames))
        if keepalive is not None:
            self._keep.append(keepalive)

    def set_native_row_margin(self, margin):
        """Striped frames: let native filters (gaussian_blur) fill only the rows a stripe render
        reads, +- `margin` rows, plus their own halo.  -1 restores whole maps."""
        self._check(lib().mmhip_set_native_row_margin(self._h, margin))

    def set_native_input_frame(self, mode):
        """Which frame of a bound image sequence native filters (gaussian_blur, render(), convolve, ...) read: "zero"
        (default, the reference's behaviour) or "current", the frame number of the render (frames[i] of a clip) -- a
        frame the sequence does not have is then an error."""
        if mode not in NATIVE_INPUT_FRAMES:
            raise MathMapError("native input frame must be one of %s, not %r" % (", ".join(sorted(NATIVE_INPUT_FRAMES)), mode))
        self._check(lib().mmhip_set_native_input_frame(self._h, NATIVE_INPUT_FRAMES[mode]))

    def set_render_size(self, render_width, render_height):
        """Renders the canvas at another pixel size (the GIMP preview, mathmap.c:2191-2223);
        `render()` then returns an array of that size."""
        self._check(lib().mmhip_set_render_size(self._h, render_width, render_height))
        self.render_width, self.render_height = render_width, render_height

    def set_sampling_offset(self, ox, oy):
        """The sub-pixel sampling offset of later renders, in pixels (mmhip_set_sampling_offset; the reference's -o renders
        its second slice at -0.5).  render_clip(aa=...) sets its own for the length of the call and puts this one back."""
        self._check(lib().mmhip_set_sampling_offset(self._h, float(ox), float(oy)))

    def set_edge_colors(self, cx, cy):
        self._check(lib().mmhip_set_edge_colors(self._h, cx, cy))

    def enable_timing(self, on=True):
        self._check(lib().mmhip_enable_timing(self._h, 1 if on else 0))

    def last_kernel_ms(self):
        return lib().mmhip_last_kernel_ms(self._h)

    def drain_kernel_ms(self, cap=4096):
        """Pixel-kernel durations (ms) of every timed launch since the last drain, oldest first."""
        buf = (C.c_double * cap)()
        n = lib().mmhip_drain_kernel_ms(self._h, buf, cap)
        if n < 0:
            raise MathMapError(_err())
        return [buf[i] for i in range(n)]

    def drain_native_kernel_ms(self, cap=4096):
        """(label, ms) of every kernel native filters launched themselves since the last drain (gaussian_blur's
        scan kernels), in launch order."""
        names = C.create_string_buffer(cap * 64)
        buf = (C.c_double * cap)()
        n = lib().mmhip_drain_native_kernel_ms(self._h, names, buf, cap)
        if n < 0:
            raise MathMapError(_err())
        return [(names.raw[i * 64:(i + 1) * 64].split(b"\0", 1)[0].decode(), buf[i]) for i in range(n)]

    def direct_native_launches(self):
        """Launches whose pixels a native filter wrote itself (pixel kernel skipped)."""
        return lib().mmhip_direct_native_launches(self._h)

    def tolerance_blur_launches(self):
        """Launches whose pixels gaussian_blur's tolerance chain wrote (Filter(gauss_mode="tolerance"))."""
        return lib().mmhip_tolerance_blur_launches(self._h)

    def prologue_launches(self):
        """Launches of the prologue kernel by render calls (a render whose frame constants stand adds none)."""
        return lib().mmhip_prologue_launches(self._h)

    def native_memo_hits(self):
        """Native filter calls of single-frame renders that were answered from the memo."""
        return lib().mmhip_native_memo_hits(self._h)

    def render(self, t=0.0, frame=0):
        """Renders the whole frame and returns it as a uint8 [H,W,4] array (RGBA)."""
        out = np.empty((self.render_height, self.render_width, 4), dtype=np.uint8)
        self._check(lib().mmhip_render_host(self._h, frame, t, out.ctypes.data_as(C.c_void_p)))
        return out

    def render_rows(self, out_ptr, first_row, last_row, t=0.0, frame=0, row_stride=None, bpp=4, floatmap=False,
                    stream=0, region=None):
        """Asynchronously renders rows [first_row,last_row) into device memory at out_ptr
        (the reference's calc_lines band, mathmap_common.c:837-846).  With `floatmap` the rows of the output are
        the frame's render width apart (16 * render_width bytes, new_template.c.in:297), whatever the region and row_stride."""
        rx, ry, rw, rh = region if region is not None else (0, 0, self.render_width, self.render_height)
        if row_stride is None:
            row_stride = rw * bpp
        self._check(lib().mmhip_render(self._h, frame, t, rx, ry, rw, rh, first_row, last_row, C.c_void_p(out_ptr),
                                       row_stride, bpp, 1 if floatmap else 0, C.c_void_p(stream)))

    def render_clip(self, num_frames=None, frames=None, ts=None, out_ptr=None, rows=None, region=None, row_stride=None,
                    frame_stride=None, bpp=4, floatmap=False, stream=0, supersample=False, shutter_samples=1, shutter_span=None,
                    shutter=None, shutter_mode="maps", aa=1, aa_threshold=None, aa_refine="list", aa_filter=None, aa_radius=None,
                    pixel_format=None, yuv_matrix="bt709", yuv_range="limited", chroma_siting=None):
        """Renders a clip in batched launches (mmhip_render_clip): frame i at frame number frames[i] and time ts[i].
        `num_frames`=N alone is the CLI's animation: frame = i, t = (float)i / (float)N.  `rows` = (first_row,
        last_row) and `region`, `row_stride`, `bpp`, `floatmap`, `stream` as in render_rows; frame i lands
        `frame_stride` bytes (default: one frame's band) behind frame i - 1.  Without `out_ptr` returns the frames as a
        uint8 [N,H,W,4] array; with it the call is asynchronous and the frames stay in HBM.
        `supersample`=True renders the CLI's -o frames (mmhip_render_clip_supersampled; compile the filter with
        supersampling=True): whole regions of bytes only, so `rows` or `floatmap` with it is a ValueError; without
        `out_ptr` it returns a uint8 [N,H,W,bpp] array.
        `shutter_samples`=K > 1 renders a motion-blurred clip (mmhip_render_clip_shutter): every frame is the mean of K
        sub-samples at frame number frames[i] and the times shutter_sample_ts(ts, K, span).  The span is `shutter_span`
        in units of t, or `shutter`, a fraction of the frame interval, in the `num_frames`=N form only: span =
        float32(float64(shutter) / N).  Giving both, `shutter` with explicit ts, K > 1 without either, or K > 1 with
        `supersample` is a ValueError.
        `shutter_mode`: "maps" (default) renders the sub-samples as float maps and averages them, "fused" sums them in the
        pixel kernel's registers (mmhip_render_clip_shutter_fused): the same bytes; filters with native calls or closure
        images take the maps path under either.  Any other value is a ValueError.
        `aa` = n or (sx, sy), 1 to 8 each, anti-aliases in space (mmhip_render_clip_sampled, with "fused"
        mmhip_render_clip_sampled_fused): every pixel is the mean, in float, of an sx x sy grid of sub-samples inside its
        footprint -- times the K shutter sub-samples where shutter_samples > 1, K * sx * sy being at most 256.  Without a
        shutter it needs no span.  Values outside the range, more than 256 sub-samples, or `aa` != 1 with
        `supersample` (the -o frames, which stay what they are) are a ValueError; aa=1 changes nothing.
        `aa_threshold` = T (default None: not adaptive, and `aa_refine` is not looked at) renders the adaptively
        anti-aliased clip (mmhip_render_clip_adaptive): a pixel gets the grid's mean only where a single-sample render,
        clamped to 0..1, differs by more than T from one of its 8 neighbours in some channel (T < 0: everywhere), and
        that render's value elsewhere.  `aa_refine`: "list" (default: the refined pixels alone are rendered, where the
        filter allows it) or "select" (the whole grid render, then the choice): the same bytes.  Spatial only:
        `aa_threshold` with `supersample` or shutter_samples > 1, a NaN, or another `aa_refine` is a ValueError.
        `aa_filter` = "box", "tent", "gaussian" or "mitchell" (default None: every path above exactly as it is) weights the
        grid's sub-samples with a reconstruction filter of `aa_radius` pixels, 0.5 to 4 (default: AA_FILTER_RADII), which
        reaches into the neighbour pixels (mmhip_render_clip_filtered); `aa` may be 1, and a shutter goes with it.  An
        unknown name, a radius out of range, `aa_radius` without `aa_filter`, or `aa_filter` with `aa_threshold`,
        `supersample` or shutter_mode="fused" is a ValueError.
        `pixel_format`="yuv420p" (default None: every call above exactly as it is) delivers the clip as planar Y'CbCr
        4:2:0 (mmhip_clip_to_yuv420) in the mode `yuv_matrix` ("bt709", "bt601") and `yuv_range` ("limited", "full"): the
        frames are rendered as above, in groups, into an RGBA8 staging buffer on the device -- at most
        MMHIP_CLIP_YUV_BYTES of it (default 1 GiB, read once per call) -- and every group is converted there; frame numbers
        and times are those of the ungrouped call.  Without `out_ptr` returns uint8 [N, frame_bytes], one Y4M payload per
        frame (yuv420_planes, write_y4m); with it the payloads land there, yuv420_frame_bytes apart, and nothing is
        copied to the host (the staging buffer's release waits for the device).  `rows` must begin on an even row and end
        on an even row or the last.  `floatmap`, another `bpp`, `region`, `row_stride` or `frame_stride` with it, or an
        unknown format, matrix or range, is a ValueError.
        `pixel_format`="yuv420p10" delivers 10-bit samples converted from the float pixels, before any 8-bit store
        (mmhip_clip_float_to_yuv420p10): the groups are rendered with floatmap=True into a float staging buffer, 16 bytes
        per pixel under the same budget, and converted there.  Without `out_ptr` returns uint16 [N, frame_bytes / 2]
        (little-endian, the value in the low 10 bits); with it the payloads land yuv420_frame_bytes(w, h, "yuv420p10")
        apart.  Everything else as with "yuv420p"; `supersample`=True with it is a ValueError (that path lands bytes).
        `chroma_siting`="center" (the default with a `pixel_format`: C420jpeg, every call above exactly as it is) or "left"
        (C420mpeg2, what video encoders assume: mmhip_clip_to_yuv420_sited, mmhip_clip_float_to_yuv420p10_sited) places the
        chroma samples of either YUV format.  Another value, or `chroma_siting` without a YUV `pixel_format`, is a
        ValueError."""
        from .striping import animation_frame_t
        if chroma_siting is not None:
            if pixel_format is None:
                raise ValueError("render_clip: chroma_siting goes with pixel_format=\"yuv420p\" or \"yuv420p10\"")
            yuv_siting(chroma_siting)
        if pixel_format is not None:
            keywords = dict(num_frames=num_frames, frames=frames, ts=ts, supersample=supersample, shutter_samples=shutter_samples,
                            shutter_span=shutter_span, shutter=shutter, shutter_mode=shutter_mode, aa=aa, aa_threshold=aa_threshold,
                            aa_refine=aa_refine, aa_filter=aa_filter, aa_radius=aa_radius)
            if pixel_format not in PIXEL_FORMATS:
                raise ValueError("render_clip: pixel_format must be one of %s, not %r" % (", ".join(PIXEL_FORMATS), pixel_format))
            for name, given in (("floatmap", floatmap), ("bpp", bpp != 4), ("region", region is not None), ("row_stride", row_stride is not None),
                                ("frame_stride", frame_stride is not None)):
                if given:
                    raise ValueError("render_clip: pixel_format is not combined with %s: whole RGBA8 frames are converted" % name)
            if pixel_format == "yuv420p10" and supersample:
                raise ValueError("render_clip: pixel_format=\"yuv420p10\" is not combined with supersample=True: that path lands bytes only")
            return self._render_clip_yuv420(yuv_mode(yuv_matrix, yuv_range), out_ptr, rows, stream, keywords, pixel_format,
                                            yuv_siting(chroma_siting) if chroma_siting is not None else 0)
        grid = sample_grid(aa)
        filtered = aa_filter is not None
        if aa_radius is not None and not filtered:
            raise ValueError("render_clip: aa_radius needs aa_filter")
        if filtered:
            kernel, radius = aa_filter_kernel(aa_filter, aa_radius)
            if aa_threshold is not None:
                raise ValueError("render_clip: aa_filter is not combined with aa_threshold")
            if supersample:
                raise ValueError("render_clip: aa_filter is not combined with supersample=True")
            if shutter_mode == "fused":
                raise ValueError("render_clip: aa_filter is not combined with shutter_mode=\"fused\"")
            if int(shutter_samples) >= 1 and int(shutter_samples) * grid[0] * grid[1] > 256:
                raise ValueError("render_clip: shutter_samples * sx * sy must be at most 256, not %d" % (int(shutter_samples) * grid[0] * grid[1]))
            if int(shutter_samples) == 1 and shutter is None and shutter_span is None:
                shutter_span = 0.0
        adaptive = aa_threshold is not None
        if adaptive:
            if supersample:
                raise ValueError("render_clip: aa_threshold is not combined with supersample=True")
            if int(shutter_samples) > 1:
                raise ValueError("render_clip: aa_threshold is not combined with shutter_samples")
            if aa_refine not in AA_REFINE_MODES:
                raise ValueError("render_clip: aa_refine must be one of %s, not %r" % (", ".join(AA_REFINE_MODES), aa_refine))
            aa_threshold = float(aa_threshold)
            if aa_threshold != aa_threshold:
                raise ValueError("render_clip: aa_threshold must not be NaN")
        if grid != (1, 1):
            if supersample:
                raise ValueError("render_clip: aa is not combined with supersample=True")
            if int(shutter_samples) >= 1 and int(shutter_samples) * grid[0] * grid[1] > 256:
                raise ValueError("render_clip: shutter_samples * sx * sy must be at most 256, not %d" % (int(shutter_samples) * grid[0] * grid[1]))
            if int(shutter_samples) == 1 and shutter is None and shutter_span is None:
                shutter_span = 0.0
        if shutter_mode not in SHUTTER_MODES:
            raise ValueError("render_clip: shutter_mode must be one of %s, not %r" % (", ".join(SHUTTER_MODES), shutter_mode))
        render_shutter = lib().mmhip_render_clip_shutter_fused if shutter_mode == "fused" else lib().mmhip_render_clip_shutter
        if grid != (1, 1):
            sampled = lib().mmhip_render_clip_sampled_fused if shutter_mode == "fused" else lib().mmhip_render_clip_sampled

            def render_shutter(h, n, fp, tp, samples, span, *rest):
                return sampled(h, n, fp, tp, samples, span, grid[0], grid[1], *rest)
        if adaptive:
            def render_shutter(h, n, fp, tp, samples, span, *rest):
                return lib().mmhip_render_clip_adaptive(h, n, fp, tp, grid[0], grid[1], aa_threshold, AA_REFINE_MODES.index(aa_refine), *rest)
        if filtered:
            def render_shutter(h, n, fp, tp, samples, span, *rest):
                return lib().mmhip_render_clip_filtered(h, n, fp, tp, samples, span, grid[0], grid[1], kernel, radius, *rest)
        if supersample and (floatmap or rows is not None):
            raise ValueError("render_clip: supersample=True renders whole regions of bytes: neither floatmap nor rows")
        shutter_samples = int(shutter_samples)
        if supersample and shutter_samples > 1:
            raise ValueError("render_clip: supersample=True is not combined with shutter_samples > 1")
        if shutter is not None and shutter_span is not None:
            raise ValueError("render_clip: give shutter or shutter_span, not both")
        if shutter is not None and (frames is not None or ts is not None or num_frames is None):
            raise ValueError("render_clip: shutter is a fraction of the frame interval of render_clip(num_frames=N); with frames and ts give shutter_span")
        if shutter_samples > 1 and shutter is None and shutter_span is None:
            raise ValueError("render_clip: shutter_samples > 1 needs shutter or shutter_span")
        if shutter is not None:
            if num_frames < 1:
                raise MathMapError("render_clip: num_frames must be at least 1")
            shutter_span = np.float32(np.float64(shutter) / np.float64(num_frames))
        shuttered = shutter_samples != 1 or shutter_span is not None or adaptive
        span = float(np.float32(shutter_span)) if shutter_span is not None else 0.0
        if frames is None and ts is None:
            if num_frames is None:
                raise MathMapError("render_clip: give num_frames, or frames and ts")
            frames = list(range(num_frames))
            ts = [animation_frame_t(i, num_frames) for i in frames]
        elif frames is None or ts is None:
            raise MathMapError("render_clip: frames and ts go together")
        frames = np.ascontiguousarray(frames, dtype=np.int32).reshape(-1)
        ts = np.ascontiguousarray(ts, dtype=np.float32).reshape(-1)
        if num_frames is None:
            num_frames = len(frames)
        if len(frames) != num_frames or len(ts) != num_frames:
            raise MathMapError("render_clip: frames and ts must have num_frames = %d entries" % num_frames)
        rx, ry, rw, rh = region if region is not None else (0, 0, self.render_width, self.render_height)
        first_row, last_row = rows if rows is not None else (ry, ry + rh)
        fp, tp = frames.ctypes.data_as(C.POINTER(C.c_int)), ts.ctypes.data_as(C.POINTER(C.c_float))
        if supersample:
            return self._render_clip_supersampled(num_frames, fp, tp, out_ptr, (rx, ry, rw, rh), row_stride, frame_stride, bpp, stream)

        def render(*landing):
            """The native call of this clip; landing: out, row_stride, frame_stride, bpp, floatmap, stream."""
            if shuttered:
                return render_shutter(self._h, num_frames, fp, tp, shutter_samples, span, rx, ry, rw, rh, first_row, last_row, *landing)
            return lib().mmhip_render_clip(self._h, num_frames, fp, tp, rx, ry, rw, rh, first_row, last_row, *landing)
        if out_ptr is not None:
            if row_stride is None:
                row_stride = rw * bpp
            if frame_stride is None:
                n_rows = max(min(last_row, ry + rh) - max(first_row, 0), 0)
                frame_stride = n_rows * (16 * self.render_width if floatmap else row_stride)
            self._check(render(C.c_void_p(out_ptr), row_stride, frame_stride, bpp, 1 if floatmap else 0, C.c_void_p(stream)))
            return None
        if rows is not None or region is not None or floatmap or bpp != 4 or row_stride is not None or frame_stride is not None:
            raise MathMapError("render_clip without out_ptr returns whole RGBA frames: pass out_ptr for bands, regions and other formats")
        out = np.empty((num_frames, self.render_height, self.render_width, 4), dtype=np.uint8)
        if num_frames < 1:
            raise MathMapError("render_clip: num_frames must be at least 1")
        dev = lib().mmhip_device_alloc(out.nbytes)
        if not dev:
            raise MathMapError(_err())
        try:
            self._check(render(C.c_void_p(dev), rw * 4, rw * 4 * rh, 4, 0, None))
            self.sync()
            self._check(lib().mmhip_copy_to_host(out.ctypes.data_as(C.c_void_p), C.c_void_p(dev), out.nbytes))
        finally:
            lib().mmhip_device_free(C.c_void_p(dev))
        return out

    def clip_to_yuv420(self, src_ptr, dst_ptr, num_frames, width=None, height=None, rows=None, src_row_stride=None, src_frame_stride=None,
                       dst_frame_stride=None, yuv_matrix="bt709", yuv_range="limited", stream=0, chroma_siting="center"):
        """Converts RGBA8 frames in device memory to planar Y'CbCr 4:2:0 payloads in device memory (mmhip_clip_to_yuv420),
        asynchronously.  `src_ptr` is the first converted row of frame 0 -- row rows[0] of the `rows` = (first_row,
        last_row) band, default the whole frame -- rows `src_row_stride` bytes apart (default 4 * width) and frames
        `src_frame_stride` (default: the band's rows); `dst_ptr` is the base of frame 0's payload, frames
        `dst_frame_stride` apart (default yuv420_frame_bytes).  The size defaults to the render size.
        `chroma_siting`="left" sites the chroma samples as C420mpeg2 does (mmhip_clip_to_yuv420_sited)."""
        matrix, rng = yuv_mode(yuv_matrix, yuv_range)
        siting = yuv_siting(chroma_siting)
        w = self.render_width if width is None else int(width)
        h = self.render_height if height is None else int(height)
        first_row, last_row = rows if rows is not None else (0, h)
        if src_row_stride is None:
            src_row_stride = 4 * w
        if src_frame_stride is None:
            src_frame_stride = max(last_row - first_row, 0) * src_row_stride
        if dst_frame_stride is None:
            dst_frame_stride = w * h + 2 * ((w + 1) >> 1) * ((h + 1) >> 1)
        self._check(_yuv_entry("clip_to_yuv420", siting, 11)(self._h, C.c_void_p(src_ptr), src_row_stride, src_frame_stride, w, h, first_row, last_row,
                                                             int(num_frames), matrix, rng, C.c_void_p(dst_ptr), dst_frame_stride, C.c_void_p(stream)))

    def clip_from_yuv420(self, src_ptr, dst_ptr, num_frames, width=None, height=None, src_frame_stride=None, dst_frame_stride=None,
                         yuv_matrix="bt709", yuv_range="limited", chroma="bilinear", stream=0, chroma_siting="center"):
        """Converts planar Y'CbCr 4:2:0 payloads in device memory to drawable words (0xRRGGBBAA, alpha 255) in device
        memory (mmhip_clip_from_yuv420), asynchronously: what set_image_device takes.  Payloads are `src_frame_stride`
        bytes apart (default yuv420_frame_bytes), frames of words `dst_frame_stride` (default 4 * width * height).  The
        size defaults to the render size.  `chroma_siting`="left" reads the chroma as C420mpeg2 sites it
        (mmhip_clip_from_yuv420_sited)."""
        matrix, rng = yuv_mode(yuv_matrix, yuv_range)
        mode = yuv_chroma(chroma)
        siting = yuv_siting(chroma_siting)
        w = self.render_width if width is None else int(width)
        h = self.render_height if height is None else int(height)
        if src_frame_stride is None:
            src_frame_stride = w * h + 2 * ((w + 1) >> 1) * ((h + 1) >> 1)
        if dst_frame_stride is None:
            dst_frame_stride = 4 * w * h
        self._check(_yuv_entry("clip_from_yuv420", siting, 9)(self._h, C.c_void_p(src_ptr), src_frame_stride, w, h, int(num_frames), matrix, rng, mode,
                                                              C.c_void_p(dst_ptr), dst_frame_stride, C.c_void_p(stream)))

    def clip_from_yuv420p10(self, src_ptr, dst_ptr, num_frames, width=None, height=None, src_frame_stride=None, dst_frame_stride=None,
                            yuv_matrix="bt709", yuv_range="limited", chroma="bilinear", stream=0, chroma_siting="center"):
        """Converts 10-bit planar Y'CbCr 4:2:0 payloads in device memory (16-bit samples) to float4 texels in device
        memory (mmhip_clip_from_yuv420p10), asynchronously: what set_image_device_float takes.  Payloads are
        `src_frame_stride` bytes apart (default yuv420_frame_bytes(w, h, "yuv420p10")), frames of texels
        `dst_frame_stride` (default 16 * width * height).  The size defaults to the render size.  `chroma_siting`="left"
        reads the chroma as C420mpeg2 sites it (mmhip_clip_from_yuv420p10_sited)."""
        matrix, rng = yuv_mode(yuv_matrix, yuv_range)
        mode = yuv_chroma(chroma)
        siting = yuv_siting(chroma_siting)
        w = self.render_width if width is None else int(width)
        h = self.render_height if height is None else int(height)
        if src_frame_stride is None:
            src_frame_stride = 2 * (w * h + 2 * ((w + 1) >> 1) * ((h + 1) >> 1))
        if dst_frame_stride is None:
            dst_frame_stride = 16 * w * h
        self._check(_yuv_entry("clip_from_yuv420p10", siting, 9)(self._h, C.c_void_p(src_ptr), src_frame_stride, w, h, int(num_frames), matrix, rng, mode,
                                                                 C.c_void_p(dst_ptr), dst_frame_stride, C.c_void_p(stream)))

    def clip_float_to_yuv420p10(self, src_ptr, dst_ptr, num_frames, width=None, height=None, rows=None, src_row_stride=None,
                                src_frame_stride=None, dst_frame_stride=None, yuv_matrix="bt709", yuv_range="limited", stream=0,
                                chroma_siting="center"):
        """Converts float frames in device memory (float4 RGBA, what floatmap=True lands) to 10-bit planar Y'CbCr 4:2:0
        payloads in device memory (mmhip_clip_float_to_yuv420p10), asynchronously.  The arguments are clip_to_yuv420's:
        rows are `src_row_stride` bytes apart (default 16 * width), frames `src_frame_stride` (default: the band's rows),
        payloads `dst_frame_stride` (default yuv420_frame_bytes(w, h, "yuv420p10")).  The size defaults to the render
        size.  `chroma_siting`="left" sites the chroma samples as C420mpeg2 does (mmhip_clip_float_to_yuv420p10_sited)."""
        matrix, rng = yuv_mode(yuv_matrix, yuv_range)
        siting = yuv_siting(chroma_siting)
        w = self.render_width if width is None else int(width)
        h = self.render_height if height is None else int(height)
        first_row, last_row = rows if rows is not None else (0, h)
        if src_row_stride is None:
            src_row_stride = 16 * w
        if src_frame_stride is None:
            src_frame_stride = max(last_row - first_row, 0) * src_row_stride
        if dst_frame_stride is None:
            dst_frame_stride = 2 * (w * h + 2 * ((w + 1) >> 1) * ((h + 1) >> 1))
        self._check(_yuv_entry("clip_float_to_yuv420p10", siting, 11)(self._h, C.c_void_p(src_ptr), src_row_stride, src_frame_stride, w, h, first_row,
                                                                      last_row, int(num_frames), matrix, rng, C.c_void_p(dst_ptr), dst_frame_stride,
                                                                      C.c_void_p(stream)))

    def clip_float_to_yuv420p10_launches(self, path):
        """The launches of clip_float_to_yuv420p10's kernel on `path`: "aligned" or "bytes" (mmhip_clip_float_to_yuv420p10_launches)."""
        if path not in ("aligned", "bytes"):
            raise ValueError("clip_float_to_yuv420p10_launches: path must be \"aligned\" or \"bytes\", not %r" % (path,))
        return lib().mmhip_clip_float_to_yuv420p10_launches(self._h, 0 if path == "aligned" else 1)

    def _render_clip_yuv420(self, mode, out_ptr, rows, stream, keywords, pixel_format="yuv420p", siting=0):
        """render_clip(pixel_format="yuv420p"): the clip of `keywords` in groups of frames through an RGBA8 staging buffer;
        with "yuv420p10" through a staging buffer of float maps."""
        import os
        from .striping import animation_frame_t
        matrix, rng = mode
        num_frames, frames, ts = keywords.pop("num_frames"), keywords.pop("frames"), keywords.pop("ts")
        shutter, shutter_span = keywords.pop("shutter"), keywords.pop("shutter_span")
        # what the ungrouped call would make of its arguments: every group gets its frames, its ts and the span
        if shutter is not None:
            if shutter_span is not None:
                raise ValueError("render_clip: give shutter or shutter_span, not both")
            if frames is not None or ts is not None or num_frames is None:
                raise ValueError("render_clip: shutter is a fraction of the frame interval of render_clip(num_frames=N); with frames and ts give shutter_span")
            if num_frames < 1:
                raise MathMapError("render_clip: num_frames must be at least 1")
            shutter_span = np.float32(np.float64(shutter) / np.float64(num_frames))
        if frames is None and ts is None:
            if num_frames is None:
                raise MathMapError("render_clip: give num_frames, or frames and ts")
            frames = list(range(num_frames))
            ts = [animation_frame_t(i, num_frames) for i in frames]
        elif frames is None or ts is None:
            raise MathMapError("render_clip: frames and ts go together")
        frames = np.ascontiguousarray(frames, dtype=np.int32).reshape(-1)
        ts = np.ascontiguousarray(ts, dtype=np.float32).reshape(-1)
        if num_frames is None:
            num_frames = len(frames)
        if len(frames) != num_frames or len(ts) != num_frames:
            raise MathMapError("render_clip: frames and ts must have num_frames = %d entries" % num_frames)
        if num_frames < 1:
            raise MathMapError("render_clip: num_frames must be at least 1")
        w, h = self.render_width, self.render_height
        first_row, last_row = (int(rows[0]), int(rows[1])) if rows is not None else (0, h)
        if not 0 <= first_row < last_row <= h:
            raise ValueError("render_clip: rows (%d, %d) are not rows of a frame of %d" % (first_row, last_row, h))
        if first_row % 2 or (last_row % 2 and last_row != h):
            raise ValueError("render_clip: with pixel_format, rows begin on an even row and end on an even row or the last, not (%d, %d) of %d"
                             % (first_row, last_row, h))
        if out_ptr is None:
            if rows is not None:
                raise MathMapError("render_clip without out_ptr returns whole frames: pass out_ptr for bands")
            stream = 0      # the invocation's, which the copy waits for
        deep = pixel_format == "yuv420p10"
        frame_bytes = yuv420_frame_bytes(w, h, pixel_format)
        pixel_bytes = 16 if deep else 4
        band_bytes = (last_row - first_row) * w * pixel_bytes
        convert = _yuv_entry("clip_float_to_yuv420p10" if deep else "clip_to_yuv420", siting, 11)
        try:
            budget = int(os.environ.get("MMHIP_CLIP_YUV_BYTES", "") or 0)
        except ValueError:
            budget = 0
        if budget <= 0:
            budget = CLIP_YUV_BYTES
        per_group = max(1, min(num_frames, 65535, budget // band_bytes))
        out = dst = None
        staging = lib().mmhip_device_alloc(per_group * band_bytes)
        if not staging:
            raise MathMapError(_err())
        try:
            if out_ptr is None:
                out = np.empty((num_frames, frame_bytes // 2), dtype="<u2") if deep else np.empty((num_frames, frame_bytes), dtype=np.uint8)
                dst = lib().mmhip_device_alloc(out.nbytes)
                if not dst:
                    raise MathMapError(_err())
            for g0 in range(0, num_frames, per_group):
                n = min(per_group, num_frames - g0)
                self.render_clip(frames=frames[g0:g0 + n], ts=ts[g0:g0 + n], out_ptr=staging, rows=rows, stream=stream,
                                 shutter_span=shutter_span, floatmap=deep, **keywords)
                self._check(convert(self._h, C.c_void_p(staging), w * pixel_bytes, band_bytes, w, h, first_row, last_row, n, matrix, rng,
                                    C.c_void_p((dst if out_ptr is None else out_ptr) + g0 * frame_bytes), frame_bytes, C.c_void_p(stream)))
            if out_ptr is None:
                self.sync()
                self._check(lib().mmhip_copy_to_host(out.ctypes.data_as(C.c_void_p), C.c_void_p(dst), out.nbytes))
        finally:
            lib().mmhip_device_free(C.c_void_p(staging))
            if dst:
                lib().mmhip_device_free(C.c_void_p(dst))
        return out

    def _render_clip_supersampled(self, num_frames, fp, tp, out_ptr, region, row_stride, frame_stride, bpp, stream):
        rx, ry, rw, rh = region
        if row_stride is None:
            row_stride = rw * bpp
        if frame_stride is None:
            frame_stride = rh * row_stride
        if out_ptr is not None:
            self._check(lib().mmhip_render_clip_supersampled(self._h, num_frames, fp, tp, rx, ry, rw, rh, C.c_void_p(out_ptr),
                                                             row_stride, frame_stride, bpp, C.c_void_p(stream)))
            return None
        if row_stride != rw * bpp or frame_stride != rh * rw * bpp:
            raise MathMapError("render_clip without out_ptr returns packed frames: pass out_ptr for padded rows and frames")
        if num_frames < 1:
            raise MathMapError("render_clip: num_frames must be at least 1")
        out = np.empty((num_frames, rh, rw, bpp), dtype=np.uint8)
        dev = lib().mmhip_device_alloc(out.nbytes)
        if not dev:
            raise MathMapError(_err())
        try:
            self._check(lib().mmhip_render_clip_supersampled(self._h, num_frames, fp, tp, rx, ry, rw, rh, C.c_void_p(dev),
                                                             row_stride, frame_stride, bpp, None))
            self.sync()
            self._check(lib().mmhip_copy_to_host(out.ctypes.data_as(C.c_void_p), C.c_void_p(dev), out.nbytes))
        finally:
            lib().mmhip_device_free(C.c_void_p(dev))
        return out

    def clip_shutter_batches(self):
        """Batches of motion-blurred frames render_clip(shutter_samples > 1) has combined so far."""
        return lib().mmhip_clip_shutter_batches(self._h)

    def clip_shutter_fused_batches(self):
        """Batches render_clip(shutter_samples > 1, shutter_mode="fused") rendered fused (0 for filters that take the maps path)."""
        return lib().mmhip_clip_shutter_fused_batches(self._h)

    def clip_sampled_batches(self):
        """Batches of grid-supersampled frames render_clip(aa != 1) has combined from sub-sample maps so far."""
        return lib().mmhip_clip_sampled_batches(self._h)

    def clip_sampled_fused_batches(self):
        """Batches render_clip(aa != 1, shutter_mode="fused") rendered fused (0 for filters that take the maps path)."""
        return lib().mmhip_clip_sampled_fused_batches(self._h)

    def clip_filtered_batches(self):
        """Batches render_clip(aa_filter=...) has combined so far."""
        return lib().mmhip_clip_filtered_batches(self._h)

    def clip_adaptive_batches(self):
        """Batches render_clip(aa_threshold=T) has rendered so far, on either path."""
        return lib().mmhip_clip_adaptive_batches(self._h)

    def clip_adaptive_refined(self):
        """The refined pixels of every frame of the last render_clip(aa_threshold=T) call: an int64 array (empty after a
        call with aa=1).  Waits for that call."""
        n = lib().mmhip_clip_adaptive_refined(self._h, None, 0)
        if n < 0:
            raise MathMapError(_err())
        out = np.zeros(n, dtype=np.int64)
        if n and lib().mmhip_clip_adaptive_refined(self._h, out.ctypes.data_as(C.POINTER(C.c_int64)), n) < 0:
            raise MathMapError(_err())
        return out

    def clip_supersampled_batches(self):
        """Batches render_clip(supersample=True) ran batched (0 for filters it renders frame by frame)."""
        return lib().mmhip_clip_supersampled_batches(self._h)

    def clip_batched_launches(self):
        """Batched pixel launches of render_clip so far (0 for filters it renders frame by frame)."""
        return lib().mmhip_clip_batched_launches(self._h)

    def clip_prologue_frames(self):
        """Frames whose frame constants render_clip's prologue evaluated (1 per call where they do not read t or frame)."""
        return lib().mmhip_clip_prologue_frames(self._h)

    def clip_native_batches(self):
        """Batches of render_clip whose gaussian_blur calls ran batched over the frames."""
        return lib().mmhip_clip_native_batches(self._h)

    def clip_native_blurs(self):
        """Blurs computed in those batches (frames with equal arguments share one)."""
        return lib().mmhip_clip_native_blurs(self._h)

    def clip_native_direct_frames(self):
        """Frames of those batches whose bytes a blur wrote itself (no pixel launch)."""
        return lib().mmhip_clip_native_direct_frames(self._h)

    def render_supersampled(self, out_ptr, t=0.0, frame=0, bpp=4, stream=0):
        """The CLI's -o (supersampling) for the whole frame, into device memory at out_ptr."""
        self._check(lib().mmhip_render_supersampled(self._h, frame, t, 0, 0, self.render_width, self.render_height,
                                                    C.c_void_p(out_ptr), self.render_width * bpp, bpp, C.c_void_p(stream)))

    def sync(self):
        self._check(lib().mmhip_sync(self._h))


def device_count():
    return lib().mmhip_device_count()


def set_device(ordinal):
    """One process per GPU: the device later invocations of this thread are created on."""
    if lib().mmhip_set_device(int(ordinal)) != 0:
        raise MathMapError(_err())
