"""What binding a clip of 10-bit planar Y'CbCr 4:2:0 frames as a float32 input drawable costs.

Clips of 1920x1080 x 60 frames and 3840x2160 x 15 frames of random payloads, in one process after a warm-up, the legs of
each part alternating for --rounds rounds:
  (a) the kernel alone (clip_from_yuv420p10 on payloads that lie in HBM), by device events through
      mmhip_drain_native_kernel_ms: both chroma modes; the aligned path with 2, 4 and 8 columns per work-item
      (MMHIP_YUV10_IN_COLUMNS) and the path of 2-byte loads (forced by a source base two bytes off); plain and
      non-temporal stores (MMHIP_YUV10_IN_STORES).  Its traffic is 19 bytes per pixel (3 read, 16 written), set against
      the achievable HBM rate.
  (b) the time to bind the same clip from host memory, by the host clock up to a device synchronisation:
      set_image(float32 [N, H, W, 4]) -- 16 bytes per pixel over the link, the only route before the converter -- against
      set_image_yuv420p10(uint16 [N, frame_bytes / 2]) -- 3 bytes per pixel over the link and the kernel of (a).

    python tools/clip_yuv10_input_cost.py --out profiles/r24_clip_yuv10_input_cost.json --commit <sha>
"""
import argparse
import ctypes as C
import json
import os
import sys
import time
from statistics import median

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_RATE = 6.29e12          # bytes/s: the achievable streaming rate of DESIGN section 3
CLIPS = {"1080p_60": (1920, 1080, 60), "2160p_15": (3840, 2160, 15)}
CHROMAS = ("bilinear", "replicate")
# path, columns per work-item (the path of 2-byte loads has one shape)
SHAPES = (("aligned", "2"), ("aligned", "4"), ("aligned", "8"), ("samples", "-"))
STORES = ("cached", "nt")
LABEL = "yuv420p10_to_float_clip"
IDENTITY = "filter identity (image in) in(xy, frame) end"


def summary(values):
    return {"ms": values, "median_ms": median(values), "spread_ms": max(values) - min(values)}


def measure_kernel(name, args):
    import numpy as np
    import mathmap_amd as mm
    from mathmap_amd._lib import lib
    from mathmap_amd.api import yuv420_frame_bytes
    w, h, n = CLIPS[name]
    fb = yuv420_frame_bytes(w, h, "yuv420p10")
    inv = mm.Filter(IDENTITY, deep_inputs=True).invoke(w, h)
    payloads = np.random.default_rng(1).integers(0, 1024, n * fb // 2 + 8).astype(np.uint16)
    src = lib().mmhip_device_alloc(payloads.nbytes)
    dst = lib().mmhip_device_alloc(n * w * h * 16)
    assert src and dst
    assert lib().mmhip_copy_to_device(C.c_void_p(src), payloads.ctypes.data_as(C.c_void_p), payloads.nbytes) == 0
    legs = [(chroma, path, columns, stores) for chroma in CHROMAS for path, columns in SHAPES for stores in STORES]

    def run(leg):
        chroma, path, columns, stores = leg
        os.environ["MMHIP_YUV10_IN_STORES"] = stores
        os.environ["MMHIP_YUV10_IN_COLUMNS"] = columns if path == "aligned" else "2"
        inv.clip_from_yuv420p10(src + (2 if path == "samples" else 0), dst, n, chroma=chroma)
        inv.sync()
    try:
        before = {p: inv.clip_from_yuv420p10_launches(p) for p in ("aligned", "samples")}
        for leg in legs * 2:                   # warm-up
            run(leg)
        taken = {p: inv.clip_from_yuv420p10_launches(p) - before[p] for p in before}
        assert taken == {"aligned": 2 * sum(leg[1] == "aligned" for leg in legs), "samples": 2 * sum(leg[1] == "samples" for leg in legs)}, taken
        inv.enable_timing(True)
        inv.drain_native_kernel_ms()
        ms = {leg: [] for leg in legs}
        for _ in range(args.rounds):
            for leg in legs:
                run(leg)
                ms[leg].append(sum(t for label, t in inv.drain_native_kernel_ms() if label == LABEL))
        inv.enable_timing(False)
    finally:
        os.environ.pop("MMHIP_YUV10_IN_STORES", None)
        os.environ.pop("MMHIP_YUV10_IN_COLUMNS", None)
        inv.sync()
        lib().mmhip_device_free(C.c_void_p(src))
        lib().mmhip_device_free(C.c_void_p(dst))
    traffic = n * (fb + 16 * w * h)
    rec = {"width": w, "height": h, "frames": n, "kernel_bytes": traffic, "bytes_per_pixel": traffic / (n * w * h),
           "kernel_at_the_hbm_rate_ms": traffic / HBM_RATE * 1e3, "kernel": {}}
    for leg in legs:
        s = summary(ms[leg])
        s["share_of_the_hbm_rate"] = rec["kernel_at_the_hbm_rate_ms"] / s["median_ms"]
        rec["kernel"]["-".join(leg)] = s
    print(json.dumps({name: {k: (round(v["median_ms"], 4), round(v["spread_ms"], 4), round(v["share_of_the_hbm_rate"], 3)) for k, v in rec["kernel"].items()}}),
          flush=True)
    return rec


def measure_bind(name, args):
    import numpy as np
    import mathmap_amd as mm
    from mathmap_amd.api import yuv420_frame_bytes
    w, h, n = CLIPS[name]
    fb = yuv420_frame_bytes(w, h, "yuv420p10")
    rng = np.random.default_rng(2)
    texels = rng.random((n, h, w, 4), dtype=np.float32)
    yuv = rng.integers(0, 1024, (n, fb // 2)).astype(np.uint16)
    inv = mm.Filter(IDENTITY, deep_inputs=True).invoke(w, h)

    def run(leg):
        if leg == "float32":
            inv.set_image("in", texels)
        else:
            inv.set_image_yuv420p10("in", yuv, w, h)
        inv.sync()
    legs = ("float32", "yuv420p10")
    for leg in legs:                           # warm-up
        run(leg)
    ms = {leg: [] for leg in legs}
    for _ in range(args.rounds):
        for leg in legs:
            inv.sync()
            t0 = time.perf_counter()
            run(leg)
            ms[leg].append((time.perf_counter() - t0) * 1e3)
    rec = {"float32_link_bytes": int(texels.nbytes), "yuv420p10_link_bytes": int(yuv.nbytes), "yuv420p10_groups": inv.clip_yuv10_input_groups()}
    for leg in legs:
        rec[leg] = summary(ms[leg])
    rec["yuv420p10_over_float32"] = rec["yuv420p10"]["median_ms"] / rec["float32"]["median_ms"]
    print(json.dumps({name + "_bind": {"float32_ms": rec["float32"]["median_ms"], "yuv420p10_ms": rec["yuv420p10"]["median_ms"],
                                       "yuv420p10_over_float32": rec["yuv420p10_over_float32"]}}), flush=True)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--commit", default="unknown")
    ap.add_argument("--clips", default=None, help="a subset (the record keeps the others)")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--no-bind", action="store_true", help="part (a) only")
    args = ap.parse_args()
    assert args.rounds >= 5, "at least 5 rounds"
    record = {}
    if os.path.exists(args.out):
        with open(args.out) as f:
            record = json.load(f)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    record.update({"commit": args.commit, "rounds": args.rounds, "hbm_rate_bytes_per_s": HBM_RATE,
                   "order": "every leg of a part once per round, in one process, after two warm-up passes (kernel) or one (bind)",
                   "timing": "kernel: device events around the launch (mmhip_drain_native_kernel_ms, label %s), MMHIP_YUV10_IN_COLUMNS and "
                             "MMHIP_YUV10_IN_STORES set per call; bind: host clock from the call to the end of a device synchronisation, "
                             "pageable host arrays" % LABEL})
    record.setdefault("clips", {})

    def save():
        with open(args.out, "w") as f:
            json.dump(record, f, indent=1)
            f.write("\n")
    for name in (args.clips.split(",") if args.clips else list(CLIPS)):
        rec = measure_kernel(name, args)
        if not args.no_bind:
            rec["bind"] = measure_bind(name, args)
        record["clips"][name] = rec
        save()
    return 0


if __name__ == "__main__":
    sys.exit(main())
