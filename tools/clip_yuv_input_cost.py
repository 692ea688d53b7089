"""What binding a clip of planar Y'CbCr 4:2:0 frames as an input drawable costs.

Clips of 1920x1080 x 120 frames and 3840x2160 x 30 frames of random payloads, in one process after a warm-up, the legs of
each part alternating for --rounds rounds:
  (a) the kernel alone (clip_from_yuv420 on payloads that lie in HBM), by device events through
      mmhip_drain_native_kernel_ms: both chroma modes, the aligned path and the byte path (forced by a source base one
      byte off), plain and non-temporal stores (MMHIP_YUV_IN_STORES).  Its traffic is 5.5 bytes per pixel (1.5 read, 4
      written), set against the achievable HBM rate.
  (b) the time to bind the same clip from host memory, by the host clock up to a device synchronisation:
      set_image(uint8 [N, H, W, 3]) -- a host loop over every texel and 4 bytes per pixel over the link -- against
      set_image_yuv420(uint8 [N, frame_bytes]) -- 1.5 bytes per pixel over the link and the kernel of (a).

    python tools/clip_yuv_input_cost.py --out profiles/r20_clip_yuv_input_cost.json --commit <sha>
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
CLIPS = {"1080p_120": (1920, 1080, 120), "2160p_30": (3840, 2160, 30)}
CHROMAS = ("bilinear", "replicate")
PATHS = ("aligned", "bytes")
STORES = ("cached", "nt")
LABEL = "yuv420_to_rgba_clip"
IDENTITY = "filter identity (image in) in(xy, frame) end"


def summary(values):
    return {"ms": values, "median_ms": median(values), "spread_ms": max(values) - min(values)}


def measure_kernel(name, args):
    import numpy as np
    import mathmap_amd as mm
    from mathmap_amd._lib import lib
    from mathmap_amd.api import yuv420_frame_bytes
    w, h, n = CLIPS[name]
    fb = yuv420_frame_bytes(w, h)
    inv = mm.Filter(IDENTITY).invoke(w, h)
    payloads = np.random.default_rng(1).integers(0, 256, n * fb + 16, dtype=np.uint8)
    src = lib().mmhip_device_alloc(payloads.nbytes)
    dst = lib().mmhip_device_alloc(n * w * h * 4)
    assert src and dst
    assert lib().mmhip_copy_to_device(C.c_void_p(src), payloads.ctypes.data_as(C.c_void_p), payloads.nbytes) == 0
    legs = [(chroma, path, stores) for chroma in CHROMAS for path in PATHS for stores in STORES]

    def run(leg):
        chroma, path, stores = leg
        os.environ["MMHIP_YUV_IN_STORES"] = stores
        inv.clip_from_yuv420(src + (1 if path == "bytes" else 0), dst, n, chroma=chroma)
        inv.sync()
    try:
        before = {p: inv.clip_from_yuv420_launches(p) for p in PATHS}
        for leg in legs * 2:                   # warm-up
            run(leg)
        taken = {p: inv.clip_from_yuv420_launches(p) - before[p] for p in PATHS}
        assert taken == {"aligned": len(legs), "bytes": len(legs)}, taken
        inv.enable_timing(True)
        inv.drain_native_kernel_ms()
        ms = {leg: [] for leg in legs}
        for _ in range(args.rounds):
            for leg in legs:
                run(leg)
                ms[leg].append(sum(t for label, t in inv.drain_native_kernel_ms() if label == LABEL))
        inv.enable_timing(False)
    finally:
        os.environ.pop("MMHIP_YUV_IN_STORES", None)
        inv.sync()
        lib().mmhip_device_free(C.c_void_p(src))
        lib().mmhip_device_free(C.c_void_p(dst))
    traffic = n * (fb + 4 * w * h)
    rec = {"width": w, "height": h, "frames": n, "kernel_bytes": traffic, "bytes_per_pixel": traffic / (n * w * h),
           "kernel_at_the_hbm_rate_ms": traffic / HBM_RATE * 1e3, "kernel": {}}
    for leg in legs:
        s = summary(ms[leg])
        s["share_of_the_hbm_rate"] = rec["kernel_at_the_hbm_rate_ms"] / s["median_ms"]
        rec["kernel"]["-".join(leg)] = s
    for chroma in CHROMAS:
        for path in PATHS:
            cached, nt = rec["kernel"]["%s-%s-cached" % (chroma, path)], rec["kernel"]["%s-%s-nt" % (chroma, path)]
            rec["kernel"]["%s-%s-nt_over_cached" % (chroma, path)] = nt["median_ms"] / cached["median_ms"]
    print(json.dumps({name: {k: (v["median_ms"], v["spread_ms"], v["share_of_the_hbm_rate"]) if isinstance(v, dict) else v
                             for k, v in rec["kernel"].items()}}), flush=True)
    return rec


def measure_bind(name, args):
    import numpy as np
    import mathmap_amd as mm
    from mathmap_amd.api import yuv420_frame_bytes
    w, h, n = CLIPS[name]
    fb = yuv420_frame_bytes(w, h)
    rng = np.random.default_rng(2)
    rgb = rng.integers(0, 256, (n, h, w, 3), dtype=np.uint8)
    yuv = rng.integers(0, 256, (n, fb), dtype=np.uint8)
    inv = mm.Filter(IDENTITY).invoke(w, h)

    def run(leg):
        if leg == "rgb":
            inv.set_image("in", rgb)
        else:
            inv.set_image_yuv420("in", yuv, w, h)
        inv.sync()
    legs = ("rgb", "yuv420")
    for leg in legs:                           # warm-up
        run(leg)
    ms = {leg: [] for leg in legs}
    for _ in range(args.rounds):
        for leg in legs:
            inv.sync()
            t0 = time.perf_counter()
            run(leg)
            ms[leg].append((time.perf_counter() - t0) * 1e3)
    rec = {"rgb_host_bytes": int(rgb.nbytes), "rgb_link_bytes": 4 * n * w * h, "yuv420_link_bytes": int(yuv.nbytes), "yuv420_groups": inv.clip_yuv_input_groups()}
    for leg in legs:
        rec[leg] = summary(ms[leg])
    rec["yuv420_over_rgb"] = rec["yuv420"]["median_ms"] / rec["rgb"]["median_ms"]
    print(json.dumps({name + "_bind": {"rgb_ms": rec["rgb"]["median_ms"], "yuv420_ms": rec["yuv420"]["median_ms"], "yuv420_over_rgb": rec["yuv420_over_rgb"]}}),
          flush=True)
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
                   "timing": "kernel: device events around the launch (mmhip_drain_native_kernel_ms, label %s), MMHIP_YUV_IN_STORES set per call; "
                             "bind: host clock from the call to the end of a device synchronisation, pageable host arrays" % LABEL})
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
