"""What the 10-bit planar Y'CbCr 4:2:0 output of a clip costs: its converter alone, and the whole path against the 8-bit one.

One process, after a warm-up, the legs alternating, medians of --rounds rounds with the spreads.
  kernel   k_float_to_yuv420p10_clip alone on random float frames in HBM at 1920x1080 x 120 and 3840x2160 x 30, timed by
           device events (mmhip_drain_native_kernel_ms, label yuv420p10_clip): the four variants MMHIP_YUV10_COLUMNS=4|8
           x MMHIP_YUV10_LOADS=nt|cached alternate, and k_rgba8_to_yuv420_clip (label yuv420_clip) runs on RGBA8 frames of
           the same size beside them.  Each is set against its traffic at the streaming rate: 19 bytes per pixel (16 read,
           3 written) for the 10-bit kernel, 5.5 for the 8-bit one.
  path     render_clip(pixel_format="yuv420p") against "yuv420p10" into an out_ptr plus the copy of the result into
           pinned host memory, for the specialised Mandelbrot and for Pond at 1920x1080 x 120, by the host clock between
           two device synchronisations.  The 10-bit leg renders float maps and moves 3 instead of 1.5 bytes per pixel
           over the link.

    python tools/clip_yuv10_cost.py --out profiles/r22_clip_yuv10_cost.json --commit <sha>
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from shutter_fused_cost import load, summary      # noqa: E402

STREAM_RATE = 6.29e12      # bytes/s, the achievable streaming rate the project measures against
KERNEL_CASES = {"1080x120": (1920, 1080, 120), "2160x30": (3840, 2160, 30)}
VARIANTS = [(columns, loads) for columns in ("4", "8") for loads in ("nt", "cached")]
PATH_FILTERS = ("mandelbrot+", "pond")                      # +: compiled with specialize=True
PATH_SIZE = (1920, 1080, 120)


def set_variant(columns, loads):
    os.environ["MMHIP_YUV10_COLUMNS"] = columns
    os.environ["MMHIP_YUV10_LOADS"] = loads


def clear_variant():
    os.environ.pop("MMHIP_YUV10_COLUMNS", None)
    os.environ.pop("MMHIP_YUV10_LOADS", None)


def measure_kernel(name, args):
    import torch
    import mathmap_amd as mm
    from mathmap_amd.api import yuv420_frame_bytes
    w, h, n = KERNEL_CASES[name]
    inv = mm.Filter("filter f () rgba:[t, 0, 0, 1] end").invoke(8, 8)
    g = torch.Generator(device="cuda").manual_seed(7)
    floats = torch.rand((n, h, w, 4), dtype=torch.float32, device="cuda", generator=g) * 1.2 - 0.1
    rgba = torch.randint(0, 256, (n, h, w, 4), dtype=torch.uint8, device="cuda", generator=g)
    bytes10, bytes8 = yuv420_frame_bytes(w, h, "yuv420p10"), yuv420_frame_bytes(w, h)
    out10 = torch.empty((n, bytes10 // 2), dtype=torch.int16, device="cuda")
    out8 = torch.empty((n, bytes8), dtype=torch.uint8, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream

    def run10():
        inv.clip_float_to_yuv420p10(floats.data_ptr(), out10.data_ptr(), n, width=w, height=h, stream=stream)

    def run8():
        inv.clip_to_yuv420(rgba.data_ptr(), out8.data_ptr(), n, width=w, height=h, stream=stream)
    inv.enable_timing(True)
    before = inv.clip_float_to_yuv420p10_launches("aligned")
    first = {}
    for _ in range(2):                    # warm-up
        for variant in VARIANTS:
            set_variant(*variant)
            run10()
            torch.cuda.synchronize()
            first.setdefault(variant, out10.clone())
        run8()
        torch.cuda.synchronize()
    same = all(bool((first[v] == first[VARIANTS[0]]).all()) for v in VARIANTS)
    inv.drain_native_kernel_ms()
    ms = {"c%s_%s" % v: [] for v in VARIANTS}
    ms["rgba8"] = []
    for _ in range(args.rounds):
        for variant in VARIANTS:
            set_variant(*variant)
            run10()
            torch.cuda.synchronize()
            ms["c%s_%s" % variant].append(sum(t for label, t in inv.drain_native_kernel_ms() if label == "yuv420p10_clip"))
        run8()
        torch.cuda.synchronize()
        ms["rgba8"].append(sum(t for label, t in inv.drain_native_kernel_ms() if label == "yuv420_clip"))
    clear_variant()
    inv.enable_timing(False)
    launches = inv.clip_float_to_yuv420p10_launches("aligned") - before
    pixels = w * h * n
    traffic10, traffic8 = 16 * pixels + bytes10 * n, 4 * pixels + bytes8 * n
    rec = {"width": w, "height": h, "frames": n, "the_variants_give_the_same_samples": same, "aligned_launches": launches,
           "bytes_10bit": traffic10, "at_the_rate_10bit_ms": traffic10 / STREAM_RATE * 1e3,
           "bytes_8bit": traffic8, "at_the_rate_8bit_ms": traffic8 / STREAM_RATE * 1e3}
    for key, values in ms.items():
        rec[key] = summary(values)
    for key in ms:
        floor = rec["at_the_rate_8bit_ms"] if key == "rgba8" else rec["at_the_rate_10bit_ms"]
        rec[key]["share_of_the_rate"] = floor / rec[key]["median_ms"]
    print(json.dumps({name: {key: [round(rec[key]["median_ms"], 4), round(rec[key]["spread_ms"], 4), round(rec[key]["share_of_the_rate"], 3)] for key in ms},
                      "same": same}), flush=True)
    return rec


def measure_path(which, args):
    import torch
    from mathmap_amd.api import yuv420_frame_bytes
    from tests import filters as F
    from tests import yuv10_reference as X
    w, h, n = PATH_SIZE
    flt = load(which)
    inv = flt.invoke(w, h)
    if F.image_names(flt):
        g = torch.Generator(device="cuda").manual_seed(7)
        image = torch.randint(-2 ** 31, 2 ** 31 - 1, (h, w), dtype=torch.int32, device="cuda", generator=g)
        inv.set_image_device("in", image.data_ptr(), w, h, keepalive=image)
    bytes10, bytes8 = yuv420_frame_bytes(w, h, "yuv420p10"), yuv420_frame_bytes(w, h)
    dev = {"yuv420p": torch.empty((n, bytes8), dtype=torch.uint8, device="cuda"), "yuv420p10": torch.empty((n, bytes10 // 2), dtype=torch.int16, device="cuda")}
    host = {k: torch.empty(v.shape, dtype=v.dtype, pin_memory=True) for k, v in dev.items()}
    stream = torch.cuda.current_stream().cuda_stream
    legs = ("yuv420p", "yuv420p10")

    def leg(fmt):
        inv.render_clip(num_frames=n, out_ptr=dev[fmt].data_ptr(), stream=stream, pixel_format=fmt)
        inv.sync()
        host[fmt].copy_(dev[fmt], non_blocking=True)
    for fmt in legs * 2:                  # warm-up: the modules are built, the copies' paths set up
        leg(fmt)
        torch.cuda.synchronize()
    ms = {fmt: [] for fmt in legs}
    for _ in range(args.rounds):
        for fmt in legs:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            leg(fmt)
            torch.cuda.synchronize()
            ms[fmt].append((time.perf_counter() - t0) * 1e3)
    # frame 0 against the restatement of the same call's float map
    floats = torch.empty((1, h, w, 4), dtype=torch.float32, device="cuda")
    inv.render_clip(frames=[0], ts=[0.0], out_ptr=floats.data_ptr(), floatmap=True, stream=stream)
    inv.sync()
    torch.cuda.synchronize()
    same = bool((X.frame(floats[0].cpu().numpy(), ("bt709", "limited")) == host["yuv420p10"][0].numpy().view("<u2")).all())
    rec = {"filter": which, "width": w, "height": h, "frames": n, "frame0_equals_the_restatement": same,
           "yuv420p_bytes_to_host": bytes8 * n, "yuv420p10_bytes_to_host": bytes10 * n}
    for fmt in legs:
        rec[fmt] = summary(ms[fmt])
    rec["yuv420p10_over_yuv420p"] = rec["yuv420p10"]["median_ms"] / rec["yuv420p"]["median_ms"]
    print(json.dumps({which: {fmt: [round(rec[fmt]["median_ms"], 3), round(rec[fmt]["spread_ms"], 3)] for fmt in legs}, "same": same}), flush=True)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--commit", default="unknown")
    ap.add_argument("--parts", default="kernel,path")
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    record = {}
    if os.path.exists(args.out):
        with open(args.out) as f:
            record = json.load(f)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    import torch
    record.update({"commit": args.commit, "device": torch.cuda.get_device_name(0), "rounds": args.rounds, "streaming_rate_bytes_per_s": STREAM_RATE,
                   "order": "kernel: c4_nt, c4_cached, c8_nt, c8_cached, rgba8, and again; path: yuv420p, yuv420p10, and again",
                   "timing": "kernel: device events around the launch (mmhip_drain_native_kernel_ms); path: host clock between two device "
                             "synchronisations around one render_clip call of the whole clip into device memory and the copy of its result "
                             "into pinned host memory"})

    def save():
        with open(args.out, "w") as f:
            json.dump(record, f, indent=1)
            f.write("\n")
    parts = args.parts.split(",")
    if "kernel" in parts:
        for name in KERNEL_CASES:
            record.setdefault("kernel", {})[name] = measure_kernel(name, args)
            save()
    if "path" in parts:
        for which in PATH_FILTERS:
            record.setdefault("path", {})[which.rstrip("+")] = measure_path(which, args)
            save()
    return 0


if __name__ == "__main__":
    sys.exit(main())
