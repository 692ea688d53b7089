"""A model of what an invocation's setters have set, and constructive walks over render paths and setters.

Pure Python: nothing here touches the library or a GPU.  tests/test_state_walk.py proves the census of the walks on the
CPU, tests/test_gpu_state_walk.py makes them: one living invocation takes every step, and after every step a fresh
invocation that got `apply(model, ...)` and nothing else must land the same bytes.

Settings and render calls are plain data ("ops": (method name, args, kwargs) of mathmap_amd.Invocation), so that the walk
can be counted without making it."""
import hashlib
import zlib

import numpy as np

CANVAS = (40, 24)            # width, height of every walk's canvas
SMALL = (17, 9)              # the render size of the "there and back" step
IMAGE = (13, 7)              # the input image: smaller than the canvas, so a native input is sampled beyond its edges
IMAGE_OTHER = (9, 30)        # "another image size": tall, so that render(in), which keeps the drawable's resize wrapper,
                             # samples it beyond its edges at the landscape canvas (as tests/test_gpu_fetch.py's 9 x 30 does)
SEQUENCE_FRAMES = 3
CLIP3 = ([2, 0, 1], [0.9, 0.1, 0.5])         # frame numbers and unequal ts of the clips
CLIP2 = ([1, 0], [0.3, 0.8])
SHUTTER = dict(shutter_samples=3, shutter_span=0.07)
DEFAULT_EDGE_COLORS = (0, 0)

IMAGE_KINDS = ("uint8", "uint8_sequence", "float32", "device_uint32", "device_float", "yuv420p", "yuv420p10")
# the order in which the "image_kind" setter of a deep filter binds them (uint8 stands for both uint8 kinds: the number of
# frames says which)
KIND_CYCLE = ("float32", "device_float", "device_uint32", "yuv420p10", "yuv420p", "uint8")
YUV_MODE, YUV_CHROMA = ("bt709", "limited"), "bilinear"         # Invocation.set_image_yuv420*'s defaults

# ---- the render paths ----
SINGLE_FRAME_PATHS = ("render", "rows_band", "rows_region_floatmap", "rows_bpp3", "render_supersampled")
CLIP_PATHS = ("clip", "clip_band_region", "shutter_maps", "shutter_fused", "aa_maps", "aa_fused", "adaptive_list", "adaptive_select",
              "aa_tent", "yuv420p", "yuv420p10", "clip_supersample")
PATHS = SINGLE_FRAME_PATHS + CLIP_PATHS
NEEDS_SUPERSAMPLING = ("render_supersampled", "clip_supersample")

# ---- the setters ----
SETTERS = ("float", "int", "bool", "color", "curve", "gradient", "image_contents", "image_size", "image_sequence", "image_kind", "edge_colors",
           "sampling_offset", "render_size", "native_input_frame", "timing", "refused")
# what mm_prologue cannot see (the timing flag lives on the host; a refused call is refused before any launch)
PROLOGUE_BLIND = ("timing", "refused")
# what a native call reads besides its own arguments: a change of these makes the memo stale
# (the edge colours too: render(in) samples a non-square drawable beyond its edges with them)
NATIVE_VISIBLE = ("float", "image_contents", "image_size", "image_sequence", "edge_colors", "render_size", "native_input_frame")

EDGE_COLOR_SETS = ((0x20406080, 0xC0A01055), (0xFF8000C0, 0x1122CCFF), (0x00FF40FF, 0x80808080))
SAMPLING_OFFSETS = ((0.25, -0.5), (-0.125, 0.375), (0.0, 0.0))


def image_pixels(size, frames, seed):
    """uint8 [frames, h, w, 4]: every texel and every alpha its own."""
    w, h = size
    return np.random.default_rng(1000 + seed).integers(0, 256, (frames, h, w, 4), dtype=np.uint8)


def curve_table(k):
    i = np.arange(1024, dtype=np.float32) / np.float32(1023)
    return (i ** np.float32(1 + k % 3) * np.float32(0.75) + np.float32(0.125 * (k % 2))).astype(np.float32)


def gradient_table(k):
    i = np.arange(1024, dtype=np.uint32)
    return (((i >> 2) ^ np.uint32(17 * k & 0xFF)) << 24) | (((1023 - i) >> 2) << 16) | np.uint32(((0x40 + 29 * k) & 0xFF) << 8) | np.uint32(0xFF)


class Model:
    """What the setters have set on an invocation of a filter with the user values `scalars` (name -> (kind, values to
    cycle through)), `tables` (name -> "curve" | "gradient") and one input image `in`."""

    def __init__(self, scalars=None, tables=None, image="in", canvas=CANVAS):
        self.canvas = tuple(canvas)
        self.scalar_sets = dict(scalars or {})
        self.table_kinds = dict(tables or {})
        self.image_name = image
        self.uservals = {}                   # name -> value, only what was set
        self.tables = {}                     # name -> (kind, table index)
        # the bound image: kind, size, frames, seed of the contents; device kinds carry (pointer, keepalive) in `device`
        self.image = dict(kind="uint8", size=IMAGE, frames=1, seed=0) if image else None
        self.device = None
        # device kinds: provide_device(image) -> (pointer, keepalive) of a buffer that holds the image's contents; whoever
        # makes the walk on a GPU supplies it, the census counts with a placeholder
        self.provide_device = lambda image: (0x1000 + 16 * (zlib.crc32(repr(sorted(image.items())).encode()) % 4096), None)
        self.edge_colors = DEFAULT_EDGE_COLORS
        self.sampling_offset = (0.0, 0.0)
        self.render_size = self.canvas
        self.native_input_frame = "zero"
        self.native_row_margin = -1
        self.timing = False
        self.refusals = 0                    # refused calls made: seen by the model, by nothing else
        self.native_scalars = None           # the scalar user values that are arguments of a native call (None: all)

    def digest(self):
        """Everything the model records, as one string: two models that differ give two digests."""
        h = hashlib.sha1()
        for part in (sorted(self.uservals.items()), sorted(self.tables.items()), sorted((self.image or {}).items()), self.device and self.device[0],
                     self.edge_colors, self.sampling_offset, self.render_size, self.native_input_frame, self.native_row_margin, self.timing,
                     self.refusals):
            h.update(repr(part).encode())
        return h.hexdigest()

    def native_key(self, frame):
        """What a native call of a single-frame render reads apart from its own arguments' bytes: the memo may answer
        only while this stands."""
        frame_key = frame if self.native_input_frame == "current" and self.image and self.image["frames"] > 1 else None
        arguments = tuple(sorted((k, v) for k, v in self.uservals.items() if self.native_scalars is None or k in self.native_scalars))
        return (arguments, tuple(sorted((self.image or {}).items())), self.edge_colors, self.render_size,
                self.native_input_frame, frame_key)

    # ---- the image as arrays ----
    def image_array(self):
        """uint8 [frames, h, w, 4] of the bound uint8 image or sequence."""
        im = self.image
        return image_pixels(im["size"], im["frames"], im["seed"])

    def oracle_image(self, frame):
        """The single uint8 image an oracle render of frame number `frame` at t < 1 reads, or None where the fetches of
        one render read different frames (in(xy) reads frame (int)t = 0, a native call under "current" frame `frame`)."""
        a = self.image_array()
        if self.image["frames"] > 1 and self.native_input_frame == "current" and frame != 0:
            return None
        return a[0]


def settings_ops(model):
    """The ops that put the model's settings, and only those, onto a fresh invocation."""
    ops = []
    for name, value in sorted(model.uservals.items()):
        ops.append(("set", (name, value), {}))
    for name, (kind, k) in sorted(model.tables.items()):
        ops.append(("set_curve", (name, curve_table(k)), {}) if kind == "curve" else ("set_gradient", (name, gradient_table(k)), {}))
    if model.image:
        ops.extend(image_ops(model))
    ops.append(("set_edge_colors", model.edge_colors, {}))
    ops.append(("set_sampling_offset", model.sampling_offset, {}))
    if model.render_size != model.canvas:
        ops.append(("set_render_size", model.render_size, {}))
    ops.append(("set_native_input_frame", (model.native_input_frame,), {}))
    if model.native_row_margin != -1:
        ops.append(("set_native_row_margin", (model.native_row_margin,), {}))
    ops.append(("enable_timing", (model.timing,), {}))
    return ops


def image_ops(model):
    im, name = model.image, model.image_name
    kind, (w, h), n = im["kind"], im["size"], im["frames"]
    if kind.startswith("device"):
        model.device = model.provide_device(im)
    if kind in ("uint8", "uint8_sequence"):
        a = model.image_array()
        return [("set_image", (name, a[0] if n == 1 else a), {})]
    if kind == "float32":
        return [("set_image", (name, float_pixels(im)), {})]
    if kind == "device_uint32":
        return [("set_image_device", (name, model.device[0], w, h), dict(num_frames=n))]
    if kind == "device_float":
        return [("set_image_device_float", (name, model.device[0], w, h), dict(num_frames=n))]
    if kind == "yuv420p":
        return [("set_image_yuv420", (name, yuv_payloads(im, 8), w, h), {})]
    if kind == "yuv420p10":
        return [("set_image_yuv420p10", (name, yuv_payloads(im, 10), w, h), {})]
    raise ValueError(kind)


def host_equivalent(im, read_device=None):
    """The array that, bound with set_image, must give what the image's own kind gives: the restated conversion of yuv
    payloads (tests/yuv_input_reference.py, tests/yuv10_input_reference.py), the bytes behind device words, the floats
    read back from a device float buffer (`read_device()` -> float32 [frames, h, w, 4])."""
    kind, (w, h), n = im["kind"], im["size"], im["frames"]
    if kind in ("uint8", "uint8_sequence", "device_uint32"):
        return image_pixels(im["size"], n, im["seed"])
    if kind == "float32":
        return float_pixels(im)
    if kind == "device_float":
        return read_device()
    if kind == "yuv420p":
        from tests import yuv_input_reference
        return np.ascontiguousarray(yuv_input_reference.rgba_frames(yuv_payloads(im, 8), w, h, YUV_MODE, YUV_CHROMA))
    if kind == "yuv420p10":
        from tests import yuv10_input_reference
        return np.ascontiguousarray(yuv10_input_reference.float_frames(yuv_payloads(im, 10), w, h, YUV_MODE, YUV_CHROMA), np.float32)
    raise ValueError(kind)


def float_pixels(im):
    """float32 [frames, h, w, 4] beyond 0..1 on both sides, every value its own."""
    w, h = im["size"]
    return np.random.default_rng(2000 + im["seed"]).uniform(-0.25, 1.25, (im["frames"], h, w, 4)).astype(np.float32)


def yuv_payloads(im, bits):
    """[frames, samples] planar 4:2:0 payloads: uint8, or uint16 with the value in the low 10 bits."""
    w, h = im["size"]
    samples = w * h + 2 * ((w + 1) >> 1) * ((h + 1) >> 1)
    rng = np.random.default_rng(3000 + im["seed"])
    return rng.integers(0, 256, (im["frames"], samples), dtype=np.uint8) if bits == 8 else rng.integers(0, 1024, (im["frames"], samples)).astype(np.uint16)


def run_ops(inv, ops):
    for method, args, kwargs in ops:
        getattr(inv, method)(*args, **kwargs)


def apply(model, invocation):
    """Replays the settings, and only the settings, onto an invocation."""
    run_ops(invocation, settings_ops(model))
    return invocation


# ---- setters: each changes the model and returns the ops that make the same change on the living invocation ----

def _cycle(values, current):
    values = list(values)
    return values[(values.index(current) + 1) % len(values)] if current in values else values[0]


def setters_of(model, natives, deep=False):
    """The setter kinds that apply to the model's filter (`natives`: it has native calls; `deep`: compiled with
    deep_inputs, so that every kind of image can be bound)."""
    # (what neither the prologue nor a native call can see comes first: the circuit takes the edges between the
    # single-frame paths at their first visits, and those steps are where a skip or a memo hit can be observed)
    out = (["image_kind"] if deep else []) + ["timing", "refused", "sampling_offset"]      # (image_kind: so that every kind meets a single-frame path)
    out += [k for k in ("float", "int", "bool", "color") if any(kind == k for kind, _ in model.scalar_sets.values())]
    out += [k for k in ("curve", "gradient") if k in model.table_kinds.values()]
    if model.image:
        out += ["image_contents", "image_size", "image_sequence"]
    out += ["edge_colors", "render_size"]
    if natives:
        out.append("native_input_frame")
    assert set(out) <= set(SETTERS)
    return out


def change(model, setter):
    """Applies setter kind `setter` to the model and returns the ops that make the same change on the living invocation
    before the step's render (what goes behind the render: `finish`)."""
    if setter in ("float", "int", "bool", "color"):
        ops = []
        for name, (kind, values) in sorted(model.scalar_sets.items()):
            if kind == setter:
                model.uservals[name] = _cycle(values, model.uservals.get(name))
                ops.append(("set", (name, model.uservals[name]), {}))
        return ops
    if setter in ("curve", "gradient"):
        ops = []
        for name, kind in sorted(model.table_kinds.items()):
            if kind == setter:
                k = model.tables.get(name, (kind, 0))[1] + 1
                model.tables[name] = (kind, k)
                ops.append(("set_curve", (name, curve_table(k)), {}) if kind == "curve" else ("set_gradient", (name, gradient_table(k)), {}))
        return ops
    if setter == "image_contents":
        model.image = dict(model.image, seed=model.image["seed"] + 1)
        return image_ops(model)
    if setter == "image_size":
        model.image = dict(model.image, size=IMAGE_OTHER if model.image["size"] == IMAGE else IMAGE)
        return image_ops(model)
    if setter == "image_sequence":
        single = model.image["frames"] == 1
        model.image = dict(model.image, frames=SEQUENCE_FRAMES if single else 1)
        if model.image["kind"].startswith("uint8"):
            model.image["kind"] = "uint8_sequence" if single else "uint8"
        return image_ops(model)
    if setter == "image_kind":
        current = "uint8" if model.image["kind"].startswith("uint8") else model.image["kind"]
        kind = _cycle(KIND_CYCLE, current)
        model.image = dict(model.image, kind="uint8_sequence" if kind == "uint8" and model.image["frames"] > 1 else kind)
        return image_ops(model)
    if setter == "edge_colors":
        model.edge_colors = _cycle(EDGE_COLOR_SETS, model.edge_colors)
        return [("set_edge_colors", model.edge_colors, {})]
    if setter == "sampling_offset":
        model.sampling_offset = _cycle(SAMPLING_OFFSETS, model.sampling_offset)
        return [("set_sampling_offset", model.sampling_offset, {})]
    if setter == "render_size":
        model.render_size = SMALL
        return [("set_render_size", SMALL, {})]
    if setter == "native_input_frame":
        model.native_input_frame = "current" if model.native_input_frame == "zero" else "zero"
        return [("set_native_input_frame", (model.native_input_frame,), {})]
    if setter == "timing":
        model.timing = not model.timing
        return [("enable_timing", (model.timing,), {})]
    if setter == "refused":
        model.refusals += 1
        return [("refused", refused_calls(model), {})]
    raise ValueError(setter)


def finish(model, setter):
    """The ops behind the step's render: the way back of "render size there and back"."""
    if setter == "render_size":
        model.render_size = model.canvas
        return [("set_render_size", model.canvas, {})]
    return []


def refused_calls(model):
    """Calls that the library must refuse and that must leave nothing behind, as (method, kwargs): a clip whose
    frame_stride is shorter than a frame, and -- where a sequence is read under "current" by a native call -- a render
    of a frame the sequence does not have.  ("out_ptr" is filled in by whoever makes the call.)"""
    calls = [("render_clip", dict(frames=CLIP2[0], ts=CLIP2[1], frame_stride=7, out_ptr="scratch"))]
    if model.image and model.image["frames"] > 1 and model.native_input_frame == "current":
        calls.append(("render", dict(t=0.25, frame=model.image["frames"] + 4)))
        calls.append(("render_clip", dict(frames=[1, model.image["frames"] + 4], ts=[0.2, 0.4], aa=2, aa_threshold=0.1)))
    return calls


# ---- render paths: what a path's call is at the model's render size ----

def path_call(path, model, index):
    """The call of `path` as data: `method`, `kwargs` (without out_ptr) and where the bytes land: `frames`, `region_w`,
    `rows` (first, last), `bpp`, `floatmap`, `row_pad`, `gap`; `yuv`: None, 8 or 10.  t and the frame number follow the
    step's index: steps 2k and 2k + 1 share them, the next two have others."""
    rw, rh = model.render_size
    t, frame = 0.125 + 0.125 * (index // 2 % 5), index // 2 % SEQUENCE_FRAMES
    land = dict(frames=1, region_w=rw, rows=(0, rh), bpp=4, floatmap=False, row_pad=0, gap=0, yuv=None)
    if path == "render":
        return dict(method="render", kwargs=dict(t=t, frame=frame), t=t, frame=frame, **land)
    if path == "rows_band":
        land.update(rows=(3, rh - 2), row_pad=5)
        return dict(method="render_rows", kwargs=dict(t=t, frame=frame), t=t, frame=frame, **land)
    if path == "rows_region_floatmap":
        land.update(rows=(2, rh - 3), region_w=rw - 5, floatmap=True)
        return dict(method="render_rows", kwargs=dict(t=t, frame=frame, region=(0, 0, rw - 5, rh)), t=t, frame=frame, **land)
    if path == "rows_bpp3":
        land.update(bpp=3)
        return dict(method="render_rows", kwargs=dict(t=t, frame=frame), t=t, frame=frame, **land)
    if path == "render_supersampled":
        return dict(method="render_supersampled", kwargs=dict(t=t, frame=frame), t=t, frame=frame, **land)
    frames, ts = CLIP3 if path in ("clip", "clip_band_region", "yuv420p", "yuv420p10") else CLIP2
    land.update(frames=len(frames), gap=12)
    kw = dict(frames=list(frames), ts=list(ts))
    if path == "clip_band_region":
        land.update(rows=(2, rh - 2), region_w=rw - 3, row_pad=3)
        kw.update(rows=(2, rh - 2), region=(1, 0, rw - 3, rh))
    elif path == "shutter_maps":
        kw.update(SHUTTER)
    elif path == "shutter_fused":
        kw.update(SHUTTER, shutter_mode="fused")
    elif path == "aa_maps":
        kw.update(aa=2)
    elif path == "aa_fused":
        kw.update(aa=2, shutter_mode="fused")
    elif path == "adaptive_list":
        kw.update(aa=2, aa_threshold=0.05, aa_refine="list")
    elif path == "adaptive_select":
        kw.update(aa=2, aa_threshold=0.05, aa_refine="select")
    elif path == "aa_tent":
        kw.update(aa=2, aa_filter="tent")
    elif path == "yuv420p":
        kw.update(pixel_format="yuv420p")
        land.update(yuv=8, gap=0)
    elif path == "yuv420p10":
        kw.update(pixel_format="yuv420p10")
        land.update(yuv=10, gap=0)
    elif path == "clip_supersample":
        kw.update(supersample=True)
    elif path != "clip":
        raise ValueError(path)
    return dict(method="render_clip", kwargs=kw, t=None, frame=None, **land)


def prologue_key(call, model, reads_t):
    """What the prologue skip of a single-frame render compares, as far as the model knows it: the geometry of the call,
    every setting the prologue can see, and t and the frame number where the prologue reads them.  For
    render_supersampled: the key its second nested render leaves, the short slice at sampling offsets 0."""
    region = call["kwargs"].get("region", (0, 0) + tuple(model.render_size))
    offset = (0.0, 0.0) if call["method"] == "render_supersampled" else model.sampling_offset
    return (region, call["rows"], model.render_size, offset, model.edge_colors, tuple(sorted(model.uservals.items())),
            tuple(sorted(model.tables.items())), tuple(sorted((model.image or {}).items())), (call["t"], call["frame"]) if reads_t else None)


# ---- the walk ----

def eulerian_circuit(n):
    """A closed walk 0 ... 0 over the complete directed graph with loops on n nodes that takes each of its n * n edges
    exactly once (Hierholzer; the out-edges of every node are taken in ascending order, so the circuit is always the same)."""
    nxt = [0] * n                      # the next out-edge of every node
    stack, circuit = [0], []
    while stack:
        v = stack[-1]
        if nxt[v] < n:
            stack.append(nxt[v])
            nxt[v] += 1
        else:
            circuit.append(stack.pop())
    circuit.reverse()
    assert len(circuit) == n * n + 1 and circuit[0] == circuit[-1] == 0
    return circuit


class Step:
    def __init__(self, index, previous, path, setter):
        self.index, self.previous, self.path, self.setter = index, previous, path, setter

    def __repr__(self):
        return "Step(%d, %s -> %s, %s)" % (self.index, self.previous, self.path, self.setter)


def walk(paths, setters):
    """The steps of a walk: step 0 renders the circuit's first path with no setter and no predecessor; behind it every
    ordered pair (previous path, next path) occurs exactly once.  In front of the j-th visit of each path stands slot
    j mod (|S| + 1) of (none, setters...): every (setter, next path) pair occurs whenever |P| >= |S| + 1."""
    paths, setters = list(paths), list(setters)
    circuit = eulerian_circuit(len(paths))
    steps = [Step(0, None, paths[circuit[0]], None)]
    visits = [0] * len(paths)
    for i in range(1, len(circuit)):
        node = circuit[i]
        slot = visits[node] % (len(setters) + 1)
        visits[node] += 1
        steps.append(Step(i, paths[circuit[i - 1]], paths[node], setters[slot - 1] if slot else None))
    return steps


def chunks(steps, n):
    """The steps in `n` runs of nearly equal length, in order."""
    size = (len(steps) + n - 1) // n
    return [steps[i:i + size] for i in range(0, len(steps), size)]


# ---- the walk filters ----
# (w1 names frame 0 in every fetch: a plain in(xy) reads frame (int)t, and a read of t anywhere is hoisted into the
# prologue, which would then run again for every new t; w1t multiplies its frame constant by t to that end)

W1_TEXT = """
filter w1 (image in, float fa: 0-1 (0.3), int ia: 1-8 (2), bool ba, color ca, curve cv, gradient gr)
  c = in(xy:[0.1, 0.2], 0)%s;
  d = in(xy:[1.3, 0.1], 0);
  s = sin(y * 10 + fa) * 0.05;
  p = in(xy + xy:[s, 0], 0);
  g = gr(cv(abs(x) * 0.5 * fa));
  q = if ba then p else g end;
  rgba:[q[0] * 0.5 + c[0] * 0.5, q[1] * 0.75 + ia * 0.01 + d[1] * 0.125, q[2] * ca[0] + ca[2] * 0.1 + c[2] * 0.1, 1]
end
"""
W3_TEXT = """
filter w3 (image in, float s: 0-1 (0.02))
  b = gaussian_blur(in, s, s);
  b(xy * 0.9) + in(xy * 1.2) * 0.25
end
"""
W3_RENDER_TEXT = """
filter w3_render (image in, float s: 0-1 (0.02))
  b = render(in);
  b(xy * 0.9) * (1 - s) + in(xy * 1.2) * 0.25
end
"""
# deep: float32 drawables of every kind; the constant fetches live in the prologue, every fetch names frame 0
W5_TEXT = """
filter w5 (image in, float fa: 0-1 (0.3))
  c = in(xy:[0.1, 0.2], 0);
  d = in(xy:[1.3, 0.1], 0);
  in(xy * (1 + fa), 0) * 0.75 + c * 0.125 + d * 0.125
end
"""
W4_TEXT = """
stretched filter w4 (stretched image in, float s: 0-1 (0.02))
  soft = gaussian_blur(in, s, s);
  soft(xy)
end
"""
# nonzero and finite, so that the literal folds of the specialising JIT are exact (builtin_probes.INEXACT_FOLD_SETS)
W1_SCALARS = {"fa": ("float", (0.3, 0.7)), "ia": ("int", (2, 5)), "ba": ("bool", (True, False)),
              "ca": ("color", ((0.25, 0.5, 0.75, 1.0), (0.9, 0.1, 0.4, 0.5)))}
W1_TABLES = {"cv": "curve", "gr": "gradient"}
# deviations on both sides of the 0.5 px FIR / IIR switch at the canvas
BLUR_SCALARS = {"s": ("float", (0.02, 0.08, 0.05))}

FILTERS = {
    "w1": dict(text=W1_TEXT % "", options=dict(intersample=False), scalars=W1_SCALARS, tables=W1_TABLES, natives=False, reads_t=False),
    "w1t": dict(text=(W1_TEXT % " * (0.5 + t * 0.5)").replace("filter w1 ", "filter w1t "), options=dict(intersample=False), scalars=W1_SCALARS,
                tables=W1_TABLES, natives=False, reads_t=True),
    "w2": dict(text=W1_TEXT % "", options=dict(intersample=False, specialize=True), scalars=W1_SCALARS, tables=W1_TABLES, natives=False,
               reads_t=False),
    "w1s": dict(text=(W1_TEXT % "").replace("filter w1 ", "filter w1s "), options=dict(intersample=False, supersampling=True), scalars=W1_SCALARS,
                tables=W1_TABLES, natives=False, reads_t=False),
    "w3": dict(text=W3_TEXT, options=dict(intersample=False, edge_x=0, edge_y=0), scalars=BLUR_SCALARS, tables={}, natives=True, reads_t=False),
    "w3_edges": dict(text=W3_TEXT, options=dict(intersample=False, edge_x=1, edge_y=2), scalars=BLUR_SCALARS, tables={}, natives=True,
                     reads_t=False),
    # (render(in) has no scalar argument: `s` reaches the pixel kernel alone, and the memo answers across its change)
    "w3_render": dict(text=W3_RENDER_TEXT, options=dict(intersample=False, edge_x=0, edge_y=0), scalars=BLUR_SCALARS, tables={}, natives=True,
                      reads_t=False, native_scalars=()),
    "w4": dict(text=W4_TEXT, options=dict(intersample=False), scalars=BLUR_SCALARS, tables={}, natives=True, reads_t=False),
    "w5": dict(text=W5_TEXT, options=dict(intersample=False, deep_inputs=True), scalars={"fa": ("float", (0.3, 0.7))}, tables={}, natives=False,
               reads_t=False),
}


def new_model(name):
    f = FILTERS[name]
    model = Model(scalars=f["scalars"], tables=f["tables"])
    model.native_scalars = f.get("native_scalars")
    return model


def paths_of(name):
    """The render paths the filter takes: the supersampled ones need a filter compiled with supersampling=True."""
    supersampling = FILTERS[name]["options"].get("supersampling", False)
    return [p for p in PATHS if supersampling or p not in NEEDS_SUPERSAMPLING]


def walk_of(name):
    return walk(paths_of(name), filter_setters(name))


def filter_setters(name):
    return setters_of(new_model(name), FILTERS[name]["natives"], FILTERS[name]["options"].get("deep_inputs", False))
