"""An invocation's history never shows in what it renders.

One living invocation per walk filter takes the steps of tests/state_walk.py's walk: a setter, then a render path, every
ordered pair of paths once.  After every step a fresh invocation that got the model's settings and nothing else makes the
same call; both land in sentinel-filled device buffers that are compared whole, bit for bit (NaN equals NaN in float
maps).  Single-frame steps are also held to the oracle, bit for bit: the walk filters fetch nearest (intersample=False),
so the bilinear fetch's bound is not needed.  No tolerance anywhere.

The counters prologue_launches() and native_memo_hits() prove that the walks take the paths they are about: the
prologue skip happens exactly where the model says nothing the prologue reads has changed, the memo answers exactly where
nothing a native call reads has changed.  Beside the walks: edge colours against native results, the prologue key field
by field, device images rebound at an unchanged pointer, refused calls."""
import ctypes as C

import numpy as np
import pytest

import mathmap_amd as mm
from mathmap_amd._lib import lib
from oracle.ccgen import CpuFilter, render_supersampled
from tests import state_walk as S
from tests.test_gpu_clip_sampled import Layout
from tests.test_gpu_clip_shutter import device_filled, device_read, same_buffer

pytestmark = pytest.mark.gpu
LEAD = 64
CHUNKS = 5
W, H = S.CANVAS


def compiled(name):
    f = S.FILTERS[name]
    return mm.Filter(f["text"], **f["options"])


def free(p):
    lib().mmhip_device_free(C.c_void_p(p))


def make(inv, call, model):
    """Makes the call into a sentinel-filled buffer and returns (the whole buffer, floatmap, layout).  The path `render`
    is Invocation.render itself (mmhip_render_host), which allocates its own device buffer and returns a host array: that
    array is what is compared; rows_bpp3 and rows_band land the same whole-frame geometry between sentinels."""
    rw, rh = model.render_size
    kw = call["kwargs"]
    if call["method"] == "render":
        return inv.render(**kw).reshape(-1), False, None
    first, last = call["rows"]
    if call["yuv"]:
        frame_bytes = mm.api.yuv420_frame_bytes(rw, rh, "yuv420p10" if call["yuv"] == 10 else "yuv420p")
        total = LEAD + call["frames"] * frame_bytes + LEAD
        dev = device_filled(total)
        try:
            assert inv.render_clip(out_ptr=dev + LEAD, **kw) is None
            inv.sync()
            return device_read(dev, total), False, None
        finally:
            free(dev)
    lay = Layout(call["frames"], call["region_w"], last - first, rw, bpp=call["bpp"], floatmap=call["floatmap"], row_pad=call["row_pad"],
                 gap=call["gap"], lead=LEAD)
    dev = device_filled(lay.total)
    try:
        if call["method"] == "render_rows":
            inv.render_rows(dev + lay.lead, first, last, row_stride=lay.stride, bpp=lay.bpp, floatmap=lay.floatmap, **kw)
        elif call["method"] == "render_supersampled":
            inv.render_supersampled(dev + lay.lead, bpp=lay.bpp, **kw)
        else:
            assert inv.render_clip(out_ptr=dev + lay.lead, row_stride=lay.stride, frame_stride=lay.fstride, bpp=lay.bpp, floatmap=lay.floatmap,
                                   **kw) is None
        inv.sync()
        return device_read(dev, lay.total), lay.floatmap, lay
    finally:
        free(dev)


def run_ops(inv, ops):
    """state_walk.run_ops, and the refused calls: each must raise and is made with a scratch buffer where it lands bytes."""
    for method, args, kwargs in ops:
        if method != "refused":
            getattr(inv, method)(*args, **kwargs)
            continue
        for refused, kw in args:
            kw = dict(kw)
            scratch = None
            if kw.get("out_ptr") == "scratch":
                scratch = kw["out_ptr"] = device_filled(1 << 16)
            try:
                with pytest.raises(mm.MathMapError):
                    getattr(inv, refused)(**kw)
                inv.sync()
                if scratch:
                    assert (device_read(scratch, 1 << 16) == 0xA5).all(), "a refused call wrote"
            finally:
                if scratch:
                    free(scratch)


def oracle_uservals(model):
    uv = dict(model.uservals)
    for name, (kind, k) in model.tables.items():
        uv[name] = S.curve_table(k) if kind == "curve" else S.gradient_table(k)
    return uv


def oracle_frame(cf, name, call, model):
    """The oracle's pixels of a single-frame call, [rows, region_w, bpp | 4], or None where one oracle render cannot
    read what the call reads (its fetches read different frames of a sequence)."""
    options = S.FILTERS[name]["options"]
    frame = call["frame"]
    images = host_equivalent(model)
    if images.dtype != np.uint8:        # a float drawable: no oracle form (the host-equivalent twin holds the restated conversion)
        return None
    image = images[0]
    if model.image["frames"] > 1 and model.native_input_frame == "current" and frame != 0:
        if name != "w4":                # w4 reads its image through the blur alone
            return None
        image = images[frame]
    rw, rh = model.render_size
    kw = dict(uservals=oracle_uservals(model), images={"in": image}, t=call["t"], frame=frame, intersample=options.get("intersample", True),
              edge=(options.get("edge_x", 0), options.get("edge_y", 0)), edge_colors=model.edge_colors)
    if call["method"] == "render_supersampled":
        # (the oracle's supersampling branch sizes its long slice by the canvas: at another render size it has no form)
        return render_supersampled(cf, W, H, **kw) if model.render_size == model.canvas else None
    kw.update(sampling_offset=model.sampling_offset, bpp=call["bpp"], floatmap=call["floatmap"], rows=call["rows"],
              supersampling=options.get("supersampling", False))
    if model.render_size != model.canvas:
        kw["render_size"] = model.render_size
    # (a region that begins at column 0 has the frame's own columns; the oracle's float map rows are a render width
    # apart whatever the region, so its whole rows are rendered and cut)
    if call["region_w"] != rw and not call["floatmap"]:
        kw["region_width"] = call["region_w"]
    want = cf.render(W, H, **kw)
    return want[call["rows"][0]:call["rows"][1], :call["region_w"]]


FEED = "filter feed (float k: 0-8 (1))\n  rgba:[x * k + t, y * 1.5 - 0.25, sin(x * 7 + k) * 2, 0.5 + t]\nend\n"
DEVICE = {}         # what the device kinds are bound to: image (as sorted items) -> device pointer, kept for the module's life


def device_image(image):
    """Model.provide_device: a device buffer with the image's contents.  device_uint32: the packed words of its bytes.
    device_float: float4 frames that a second invocation renders there with render_clip(floatmap=True, out_ptr=...) --
    filter A's float maps are filter B's drawable, values beyond 0..1 on both sides."""
    key = tuple(sorted(image.items()))
    if key not in DEVICE:
        (w, h), n = image["size"], image["frames"]
        if image["kind"] == "device_uint32":
            a = S.image_pixels(image["size"], n, image["seed"]).astype(np.uint32)
            words = np.ascontiguousarray((a[..., 0] << 24) | (a[..., 1] << 16) | (a[..., 2] << 8) | a[..., 3])
            dev = lib().mmhip_device_alloc(words.nbytes)
            assert dev and lib().mmhip_copy_to_device(C.c_void_p(dev), words.ctypes.data_as(C.c_void_p), words.nbytes) == 0
        else:
            dev = lib().mmhip_device_alloc(n * h * w * 16)
            assert dev
            feeder = mm.Filter(FEED).invoke(w, h)
            feeder.set("k", 1.0 + 0.5 * (image["seed"] % 7))
            feeder.render_clip(frames=list(range(n)), ts=[0.1 + 0.2 * i for i in range(n)], floatmap=True, out_ptr=dev)
            feeder.sync()
        DEVICE[key] = dev
    return DEVICE[key], None


def host_equivalent(model):
    im = model.image
    (w, h), n = im["size"], im["frames"]
    return S.host_equivalent(im, lambda: device_read(device_image(im)[0], n * h * w * 16).view(np.float32).reshape(n, h, w, 4).copy())


def host_twin(model, flt):
    """A fresh invocation with the model's settings whose image is bound from host memory with set_image: the bytes, the
    floats, or what the restated yuv conversion makes of the payloads."""
    inv = flt.invoke(W, H)
    for method, args, kwargs in S.settings_ops(model):
        if method.startswith("set_image"):
            method, args, kwargs = "set_image", (args[0], host_equivalent(model)), {}
        getattr(inv, method)(*args, **kwargs)
    return inv


class Walker:
    """The living invocation of one walk filter, its model, and what the counters must show."""

    def __init__(self, name):
        self.name = name
        self.spec = S.FILTERS[name]
        self.flt = compiled(name)
        self.cf = CpuFilter(self.flt.ir_json_raw)
        self.model = S.new_model(name)
        self.model.provide_device = device_image
        self.inv = S.apply(self.model, self.flt.invoke(W, H))
        self.steps = S.walk_of(name)
        n = len(self.steps)
        self.checkpoints = {n // 4, n // 2, 3 * n // 4}
        self.next = 0
        self.single_renders = self.single_launches = 0      # renders made by single-frame steps (two per render_supersampled), and their prologue launches
        self.skips = self.hits_seen = 0
        self.prologue_key = None          # of the previous step, where it was a single-frame step
        self.native_key = None
        self.previous_path = None
        self.broken = False

    def advance(self, last_index):
        assert not self.broken, "an earlier step of this walk failed"
        self.broken = True
        while self.next <= last_index:
            self.step(self.steps[self.next])
            self.next += 1
        self.broken = False

    def step(self, st):
        inv, model, where = self.inv, self.model, (self.name, st)
        settings = model.digest()
        run_ops(inv, S.change(model, st.setter) if st.setter else [])
        assert st.setter is None or model.digest() != settings, where
        call = S.path_call(st.path, model, st.index)
        pro, hits = inv.prologue_launches(), inv.native_memo_hits()
        got, floatmap, lay = make(inv, call, model)
        pro, hits = inv.prologue_launches() - pro, inv.native_memo_hits() - hits
        flt = compiled(self.name) if st.index in self.checkpoints else self.flt
        twin = S.apply(model, flt.invoke(W, H))
        want, _, _ = make(twin, call, model)
        assert same_buffer(got, want, floatmap), where + ("the fresh invocation differs", int((got != want).sum()))
        if self.spec["options"].get("deep_inputs") and model.image["kind"] not in ("uint8", "uint8_sequence", "float32"):
            want, _, _ = make(host_twin(model, flt), call, model)
            assert same_buffer(got, want, floatmap), where + ("the image bound from host memory differs", model.image["kind"])
        if st.path in S.SINGLE_FRAME_PATHS:
            px = oracle_frame(self.cf, self.name, call, model)
            if px is not None:
                expected = px.reshape(-1) if lay is None else lay.expected([px])
                assert same_buffer(got, np.ascontiguousarray(expected).view(np.uint8), floatmap), where + ("the oracle differs",)
            self.power(st, call, pro, hits)
        else:
            self.prologue_key = self.native_key = None          # a clip leaves pro_filter = nullptr; what it leaves the memo is not modelled
        self.previous_path = st.path
        run_ops(inv, S.finish(model, st.setter))

    def power(self, st, call, pro, hits):
        """The counters of a single-frame step against what the model says may be kept."""
        model, where = self.model, (self.name, st)
        nested = 2 if st.path == "render_supersampled" else 1      # the long slice at offsets -0.5, then the short one at 0
        self.single_renders += nested
        self.single_launches += pro
        key = S.prologue_key(call, model, self.spec["reads_t"])
        if self.spec["natives"]:
            assert pro == nested, where                 # a filter with native calls never skips its prologue
            nkey = model.native_key(call["frame"])
            if self.native_key is not None:
                if nkey != self.native_key:
                    assert hits == 0, where + ("the memo answered although what the call reads has changed",)
                elif self.name != "w4" or self.previous_path != "render":
                    # (w4's whole-frame render writes the pixels directly and keeps no map on the first use of a set)
                    assert hits == 1, where + ("the memo did not answer although nothing the call reads has changed",)
            self.hits_seen += hits
            self.native_key = nkey
        else:
            assert hits == 0, where
            # (the long slice of a supersampled render has a key of its own, one column wider: both nested renders launch)
            expected = 2 if nested == 2 else 0 if key == self.prologue_key else 1
            assert pro == expected, where + ("prologue launches", pro, "expected", expected)
            if st.setter is not None and st.setter not in S.PROLOGUE_BLIND:
                assert pro > 0, where
            self.skips += nested - pro
        self.prologue_key = key

    def finished(self):
        inv = self.inv
        assert self.next == len(self.steps)
        if self.spec["natives"]:
            assert inv.native_memo_hits() > 0 and self.hits_seen > 0, self.name
            if self.name == "w4":
                assert inv.direct_native_launches() > 0
        else:
            # over the whole walk the skip happened: fewer prologue launches than renders by the single-frame steps
            assert 0 < self.single_launches < self.single_renders, self.name
        assert self.single_launches == self.single_renders - self.skips and inv.prologue_launches() >= self.single_launches


WALKERS = {}


def walker(name):
    if name not in WALKERS:
        WALKERS[name] = Walker(name)
    return WALKERS[name]


@pytest.mark.parametrize("chunk", range(CHUNKS))
@pytest.mark.parametrize("name", list(S.FILTERS))
def test_walk(name, chunk):
    """Chunk `chunk` of the filter's walk, in circuit order on the one living invocation (a chunk run alone takes the
    steps before it first)."""
    w = walker(name)
    part = S.chunks(w.steps, CHUNKS)[chunk]
    w.advance(part[-1].index)
    if chunk == CHUNKS - 1:
        w.finished()


# ---- targeted cases ----

def fresh_pair(name, model=None):
    flt = compiled(name)
    model = model or S.new_model(name)
    model.provide_device = device_image
    return flt, model, S.apply(model, flt.invoke(W, H))


def twin_bytes(flt, model, call):
    return make(S.apply(model, flt.invoke(W, H)), call, model)[0]


EDGE_CASES = {
    # name: (text, size of `in`, the memo answers, the colours show in the picture)
    "w3": (S.W3_TEXT, S.IMAGE, True, True),                # ... through in(xy * 1.2) of the pixel kernel
    # render(in) keeps the drawable's resize wrapper: on the tall image k_render_drawable samples beyond the edges
    "render": ("filter e_render (image in, float s: 0-1 (0.02))\n  b = render(in);\n  b(xy * 0.9) * (1 - s)\nend\n", S.IMAGE_OTHER, True, True),
    "render_stretched": ("stretched filter e_render_s (image in, float s: 0-1 (0.02))\n  b = render(in);\n  b(xy * 0.9) * (1 - s)\nend\n",
                         S.IMAGE, True, True),
    # convolve strips the wrapper: its map of the drawable never leaves it
    "convolve": ("filter e_conv (image in, image kernel, float s: 0-1 (0.02))\n  b = convolve(in, kernel, 1, 1);\n  b(xy * 0.9) * (1 - s)\nend\n",
                 S.IMAGE, True, False),
    # a closure image whose body leaves the drawable: rendered anew for every call, never memoised
    "closure": ("filter wide (image in)\n  in(xy * 1.5)\nend\n"
                "filter e_closure (image in, float s: 0-1 (0.02))\n  b = gaussian_blur(wide(in), s, s);\n  b(xy * 0.9)\nend\n", S.IMAGE, False, True),
}


@pytest.mark.parametrize("path", ["render", "clip"])
@pytest.mark.parametrize("case", list(EDGE_CASES))
def test_edge_colours_make_native_results_stale(case, path):
    """render, set_edge_colors to what they are, render, set_edge_colors to two other colours, render.  The memo is on the
    path and answers while the colours stand, setting the current values included; a change of either colour makes the
    native results stale: the memo does not answer, and the frame is the fresh invocation's and the oracle's -- for
    render(in) on a tall image and in a stretched filter, where the native filter itself samples beyond the edges, a frame
    that differs from the first."""
    text, size, memoised, colours_show = EDGE_CASES[case]
    flt = mm.Filter(text, intersample=False, edge_x=0, edge_y=0)
    cf = CpuFilter(flt.ir_json_raw)
    images = {"in": S.image_pixels(size, 1, 0)[0]}
    if case == "convolve":
        kernel = np.zeros((3, 3, 4), np.uint8)
        kernel[..., :3] = np.array([[10, 30, 10], [30, 95, 30], [10, 30, 10]], np.uint8)[..., None]
        kernel[..., 3] = 255
        images["kernel"] = kernel

    def invocation(colors):
        inv = flt.invoke(W, H)
        for k, v in images.items():
            inv.set_image(k, v)
        inv.set_edge_colors(*colors)
        return inv

    def render(inv):
        if path == "render":
            return inv.render(t=0.25)
        return inv.render_clip(frames=S.CLIP2[0], ts=S.CLIP2[1])
    first_colors, second_colors = S.EDGE_COLOR_SETS[0], S.EDGE_COLOR_SETS[1]
    inv = invocation(first_colors)
    first = render(inv)
    assert np.array_equal(render(inv), first)
    hits = inv.native_memo_hits()
    if path == "render":
        assert hits == (1 if memoised else 0)      # the second render was answered from the memo: the memo is on the path
        inv.set_edge_colors(*first_colors)         # the values they have: still a hit
        assert np.array_equal(render(inv), first)
        assert inv.native_memo_hits() == hits + (1 if memoised else 0)
        hits = inv.native_memo_hits()
    inv.set_edge_colors(*second_colors)
    second = render(inv)
    if path == "render":
        assert inv.native_memo_hits() == hits      # stale: computed anew
    assert np.array_equal(second, render(invocation(second_colors)))
    assert np.array_equal(second, first) != colours_show
    for colors, got in ((first_colors, first), (second_colors, second)):
        for i, (frame, t) in enumerate([(0, 0.25)] if path == "render" else zip(*S.CLIP2)):
            want = cf.render(W, H, images=images, t=t, frame=frame, intersample=False, edge=(0, 0), edge_colors=colors)
            assert np.array_equal(got if path == "render" else got[i], want), (case, colors, i)


def hip_runtime():
    """The HIP runtime the library has loaded, for a second stream."""
    lib()
    hip = C.CDLL(next(line.split()[-1] for line in open("/proc/self/maps") if "libamdhip64" in line))      # as tests/test_gpu_clip_yuv_input.py finds it
    hip.hipStreamCreate.argtypes = [C.POINTER(C.c_void_p)]
    hip.hipStreamSynchronize.argtypes = hip.hipStreamDestroy.argtypes = [C.c_void_p]
    return hip


def key_items(model):
    """(setter, prologue launches of the render behind it) for every setter kind but the two that the test takes apart."""
    return [(setter, 0 if setter in S.PROLOGUE_BLIND else 1) for setter in S.setters_of(model, False) if setter not in ("refused", "render_size")]


@pytest.mark.parametrize("name", ["w1", "w1t"])
def test_the_prologue_key_field_by_field(name):
    """A first render; then for every item: the item, a render (+1 launch where the prologue can see the item, +0
    where the key blanks it) and the same render again (+0).  The bytes are the fresh invocation's every time."""
    flt, model, inv = fresh_pair(name)
    reads_t = S.FILTERS[name]["reads_t"]
    hip, stream = hip_runtime(), C.c_void_p()
    assert hip.hipStreamCreate(C.byref(stream)) == 0
    call = dict(method="render_rows", kwargs=dict(t=0.25, frame=0), t=0.25, frame=0, frames=1, region_w=W, rows=(0, H), bpp=4, floatmap=False,
                row_pad=0, gap=0, yuv=None)

    def render_twice(what, expected):
        for again, want_launches in ((False, expected), (True, 0)):
            before = inv.prologue_launches()
            got, floatmap, _ = make(inv, call, model)
            assert inv.prologue_launches() - before == want_launches, (name, what, "again" if again else "first")
            assert same_buffer(got, twin_bytes(flt, model, call), floatmap), (name, what, again)
    render_twice("first render", 1)
    for setter, launches in key_items(model):
        run_ops(inv, S.change(model, setter))
        render_twice(setter, launches)
    # t and the frame number: read by w1t's prologue only
    call["kwargs"] = dict(t=0.625, frame=0)
    call["t"] = 0.625
    render_twice("t", 1 if reads_t else 0)
    call["kwargs"] = dict(t=0.625, frame=2)
    call["frame"] = 2
    render_twice("frame", 1 if reads_t else 0)
    # the geometry: rows, region
    call["rows"] = (3, H - 2)
    render_twice("rows", 1)
    call["kwargs"]["region"] = (2, 1, W - 5, H - 3)
    call.update(region_w=W - 5, rows=(4, H - 4))
    render_twice("region", 1)
    del call["kwargs"]["region"]
    call.update(region_w=W, rows=(0, H))
    render_twice("whole frame again", 1)
    # what the key blanks: the bytes must still be right
    call["bpp"] = 3
    render_twice("bpp", 0)
    call["row_pad"] = 7
    render_twice("row_stride", 0)
    call.update(bpp=4, row_pad=0, floatmap=True)
    render_twice("floatmap", 0)
    call["floatmap"] = False
    # the render size, there and back
    run_ops(inv, S.change(model, "render_size"))
    call.update(region_w=S.SMALL[0], rows=(0, S.SMALL[1]))
    render_twice("render size", 1)
    run_ops(inv, S.finish(model, "render_size"))
    call.update(region_w=W, rows=(0, H))
    render_twice("render size back", 1)
    # another stream, and back
    call["kwargs"]["stream"] = stream.value
    try:
        render_twice("another stream", 1)
    finally:
        assert hip.hipStreamSynchronize(stream) == 0
    del call["kwargs"]["stream"]
    render_twice("the invocation's stream again", 1)
    assert hip.hipStreamDestroy(stream) == 0
    # a clip call in between
    inv.render_clip(frames=S.CLIP2[0], ts=S.CLIP2[1])
    render_twice("a clip in between", 1)
    # a refused call in between changes nothing
    run_ops(inv, S.change(model, "refused"))
    render_twice("a refused call", 0)
    # a band tall enough to grow the row table: a taller render size
    tall = (W, 4 * H)
    inv.set_render_size(*tall)
    model.render_size = tall
    call.update(rows=(0, tall[1]))
    render_twice("a taller row table", 1)


@pytest.mark.parametrize("name", ["w1", "w3"])
def test_rebinding_a_device_image_at_the_same_pointer_publishes_new_contents(name):
    """The rule of include/mmhip.h: contents rewritten behind a bound device pointer are published by calling the setter
    again with the same pointer -- to frame constants (w1's constant fetch) and native results (w3's blur) alike."""
    flt = compiled(name)
    w, h = S.IMAGE
    first, second = (S.image_pixels(S.IMAGE, 1, seed)[0] for seed in (0, 1))

    def words(a):
        a = a.astype(np.uint32)
        return np.ascontiguousarray((a[..., 0] << 24) | (a[..., 1] << 16) | (a[..., 2] << 8) | a[..., 3])
    dev = lib().mmhip_device_alloc(w * h * 4)
    assert dev
    try:
        def upload(a):
            p = words(a)
            assert lib().mmhip_copy_to_device(C.c_void_p(dev), p.ctypes.data_as(C.c_void_p), p.nbytes) == 0
        upload(first)
        inv = flt.invoke(W, H)
        inv.set_image_device("in", dev, w, h)
        a = inv.render(t=0.25)
        assert np.array_equal(inv.render(t=0.25), a)
        launches, hits = inv.prologue_launches(), inv.native_memo_hits()
        inv.sync()
        upload(second)
        inv.set_image_device("in", dev, w, h)          # the same pointer: publishes the new contents
        b = inv.render(t=0.25)
        assert inv.prologue_launches() == launches + 1 and inv.native_memo_hits() == hits
        twin = flt.invoke(W, H)
        twin.set_image("in", second)
        assert np.array_equal(b, twin.render(t=0.25))
        assert not np.array_equal(a, b)
        want = CpuFilter(flt.ir_json_raw).render(W, H, images={"in": second}, t=0.25, intersample=False,
                                                 edge=(S.FILTERS[name]["options"].get("edge_x", 0), S.FILTERS[name]["options"].get("edge_y", 0)))
        assert np.array_equal(b, want)
    finally:
        free(dev)


def test_rebinding_a_float_device_image_at_the_same_pointer_publishes_new_contents():
    """The same rule at set_image_device_float, the chain in HBM: w5's frame constants and pixels follow float texels
    rewritten behind the bound pointer once the setter is called again.  The texels are float32(byte / 255.0), what the
    8-bit fetch makes of a byte, so the oracle's render of the byte image is the reference."""
    flt = compiled("w5")
    w, h = S.IMAGE
    first, second = (S.image_pixels(S.IMAGE, 1, seed)[0] for seed in (0, 1))

    def texels(a):
        return np.ascontiguousarray((a / 255.0).astype(np.float32))
    dev = lib().mmhip_device_alloc(w * h * 16)
    assert dev
    try:
        def upload(a):
            p = texels(a)
            assert lib().mmhip_copy_to_device(C.c_void_p(dev), p.ctypes.data_as(C.c_void_p), p.nbytes) == 0
        upload(first)
        inv = flt.invoke(W, H)
        inv.set_image_device_float("in", dev, w, h)
        a = inv.render(t=0.25)
        assert np.array_equal(inv.render(t=0.25), a)
        launches = inv.prologue_launches()
        assert launches == 1                               # the second render kept its frame constants
        inv.sync()
        upload(second)
        inv.set_image_device_float("in", dev, w, h)        # the same pointer: publishes the new contents
        b = inv.render(t=0.25)
        assert inv.prologue_launches() == launches + 1
        twin = flt.invoke(W, H)
        twin.set_image("in", texels(second))
        assert np.array_equal(b, twin.render(t=0.25))
        assert not np.array_equal(a, b)
        cf = CpuFilter(flt.ir_json_raw)
        for image, got in ((first, a), (second, b)):
            assert np.array_equal(got, cf.render(W, H, images={"in": image}, t=0.25, intersample=False)), "the oracle on the byte image"
    finally:
        free(dev)


@pytest.mark.parametrize("name", ["w1", "w3", "w4"])
def test_a_refused_call_leaves_nothing_behind(name):
    """After every refusal the walk uses -- a short frame_stride; under "current", a frame the sequence does not have in
    a render and in the nested base render of an adaptive clip -- the next render of every path equals the fresh
    invocation's, the caller's sampling offset included, and the counters moved as a call that did nothing allows."""
    flt = compiled(name)
    model = S.new_model(name)
    S.change(model, "image_sequence")
    S.change(model, "sampling_offset")
    if S.FILTERS[name]["natives"]:
        S.change(model, "native_input_frame")
    inv = S.apply(model, flt.invoke(W, H))
    refusals = S.refused_calls(model)
    assert len(refusals) == (3 if S.FILTERS[name]["natives"] else 1)
    make(inv, S.path_call("render", model, 0), model)
    for k, refusal in enumerate(refusals):
        for index, path in enumerate(S.paths_of(name)):
            launches, hits = inv.prologue_launches(), inv.native_memo_hits()
            run_ops(inv, [("refused", [refusal], {})])
            # refused before its first launch, or behind the prologue of the render that then failed
            assert inv.prologue_launches() - launches in ((0,) if k == 0 else (0, 1)), (name, refusal)
            assert inv.native_memo_hits() == hits
            call = S.path_call(path, model, 3 * index)      # frame 0: inside the sequence
            got, floatmap, _ = make(inv, call, model)
            assert same_buffer(got, twin_bytes(flt, model, call), floatmap), (name, refusal, path)
