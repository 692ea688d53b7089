"""What a motion-blurred clip costs: the shutter combine kernel alone, and one mmhip_render_clip_shutter call against the
plain float-map clip of the same (frame, t) pairs.

Parts, each merged into the record at --out (stamped with --commit):

  --part combine  k_shutter_combine_clip on float maps in HBM (mmhip_selftest_shutter_combine, one frame, bpp 4, one
                  pass) at 1280x720, 1920x1080 and 8192^2 with K = 4 and 8: milliseconds of every round, the median,
                  achieved bytes/s at 16 K + 4 bytes per pixel against the streaming ceiling.  Beside it, from the same
                  run, k_supersample_combine_clip's figure (mmhip_selftest_combine_ms, 12 B/px).
  --part clip     Ident, the specialised Mandelbrot and Pond at the same sizes and K: render_clip(shutter_samples=K) of N
                  frames into RGBA8 against render_clip(floatmap=True) of the same N * K (frame, t) pairs -- the call the
                  shutter clip nests, whose code this feature does not touch --, alternating for --rounds rounds with
                  device events around each.  Per case the medians, the spreads and the difference per sub-sample frame,
                  beside what one more read of the sub-sample maps takes at the streaming ceiling.
  --part run      one variant of one case, --rounds times, untimed: what a kernel trace is collected from.

    python tools/clip_shutter_cost.py --part combine --out profiles/r12_clip_shutter_cost.json --commit <sha>
    python tools/clip_shutter_cost.py --part clip --out profiles/r12_clip_shutter_cost.json --commit <sha>
"""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from sequence_cost import median      # noqa: E402

STREAM_CEILING = 6.3e12      # bytes/s, DESIGN section 3
SIZES = {"720": (1280, 720), "1080": (1920, 1080), "8192": (8192, 8192)}
SAMPLES = (4, 8)
FRAMES = {"720": 8, "1080": 8, "8192": 1}       # output frames of a clip case (8192^2 with K = 8: 8 GiB of sub-samples)
SS_FRAMES = {"720": 32, "1080": 32, "8192": 3}
COMBINE_CASES = {"%s_k%d" % (s, k): (s, k) for s in SIZES for k in SAMPLES}
CASES = {"%s_%s_k%d" % (f.rstrip("+"), s, k): (f, s, k) for f in ("ident", "mandelbrot+", "pond") for s in SIZES for k in SAMPLES}


def summary(values):
    return {"values": values, "median": median(values), "spread": max(values) - min(values)}


def measure_combine(name, args):
    from mathmap_amd._lib import selftest_lib
    size, k = COMBINE_CASES[name]
    w, h = SIZES[size]
    ms = (C.c_double * args.rounds)()
    rc = selftest_lib().mmhip_selftest_shutter_combine(None, 1, k, h, w, w, 4, 0, w * 4, w * h * 4, 0, 0, None, w * h * 4, 0, args.rounds, ms)
    assert rc == 0, selftest_lib().mmhip_selftest_error()
    s = summary([ms[r] for r in range(args.rounds)])
    per_px = 16 * k + 4
    rec = {"width": w, "height": h, "samples": k, "bytes_per_px": per_px, "ms": s["values"], "median_ms": s["median"], "spread_ms": s["spread"],
           "bytes_per_s": per_px * w * h / (s["median"] * 1e-3)}
    rec["share_of_streaming_ceiling"] = rec["bytes_per_s"] / STREAM_CEILING
    frames = SS_FRAMES[size]
    ss = (C.c_double * (2 * args.rounds))()
    differ = selftest_lib().mmhip_selftest_combine_ms(w, h, 4, frames, args.rounds, ss)
    assert differ >= 0, selftest_lib().mmhip_selftest_error()
    t = summary([ss[2 * r + 1] / frames for r in range(args.rounds)])
    rec["supersample_combine_clip"] = {"frames": frames, "median_ms_per_frame": t["median"], "spread_ms": t["spread"],
                                       "bytes_per_s_at_12_B_per_px": 12.0 * w * h / (t["median"] * 1e-3)}
    rec["rate_over_supersample_combine_clip"] = rec["bytes_per_s"] / rec["supersample_combine_clip"]["bytes_per_s_at_12_B_per_px"]
    print(json.dumps({name: {"ms": rec["median_ms"], "TB_per_s": rec["bytes_per_s"] / 1e12, "share": rec["share_of_streaming_ceiling"],
                             "ss_TB_per_s": rec["supersample_combine_clip"]["bytes_per_s_at_12_B_per_px"] / 1e12}}), flush=True)
    return rec


class Case:
    def __init__(self, name):
        import numpy as np
        import torch
        from mathmap_amd.api import shutter_sample_ts
        from mathmap_amd.striping import animation_frame_t
        from tests import filters as F
        which, size, self.k = CASES[name]
        self.w, self.h = SIZES[size]
        self.n = FRAMES[size]
        self.flt = F.load(which.rstrip("+"), specialize=which.endswith("+"))
        self.inv = self.flt.invoke(self.w, self.h)
        if F.image_names(self.flt):
            g = torch.Generator(device="cuda").manual_seed(7)
            self.image = torch.randint(-2 ** 31, 2 ** 31 - 1, (self.h, self.w), dtype=torch.int32, device="cuda", generator=g)
            self.inv.set_image_device("in", self.image.data_ptr(), self.w, self.h, keepalive=self.image)
        self.frames = np.arange(self.n, dtype=np.int32)
        self.ts = np.array([animation_frame_t(i, self.n) for i in range(self.n)], dtype=np.float32)
        self.span = float(np.float32(0.5 / self.n))
        self.sub_frames = np.repeat(self.frames, self.k)
        self.sub_ts = shutter_sample_ts(self.ts, self.k, self.span).reshape(-1)
        self.out = torch.empty((self.n, self.h, self.w, 4), dtype=torch.uint8, device="cuda")
        self.maps = torch.empty((self.n * self.k, self.h, self.w, 4), dtype=torch.float32, device="cuda")
        self.stream = torch.cuda.current_stream().cuda_stream
        self.plan = self.flt.clip_shutter_plan(self.w, self.h, self.w, self.k, self.n)

    def shutter(self):
        self.inv.render_clip(frames=self.frames, ts=self.ts, out_ptr=self.out.data_ptr(), stream=self.stream, shutter_samples=self.k,
                             shutter_span=self.span)

    def maps_only(self):
        self.inv.render_clip(frames=self.sub_frames, ts=self.sub_ts, out_ptr=self.maps.data_ptr(), stream=self.stream, floatmap=True)


def measure_clip(name, args):
    import torch
    c = Case(name)
    for _ in range(2):
        c.maps_only()
        c.shutter()
    torch.cuda.synchronize()
    ms = {"maps_only": [], "shutter": []}
    for _ in range(args.rounds):
        for variant in ("maps_only", "shutter"):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            getattr(c, variant)()
            e1.record()
            torch.cuda.synchronize()
            ms[variant].append(e0.elapsed_time(e1))
    subs = c.n * c.k
    rec = {"filter": CASES[name][0], "width": c.w, "height": c.h, "frames": c.n, "samples": c.k, "plan": c.plan}
    for variant in ms:
        s = summary(ms[variant])
        rec[variant] = {"ms": s["values"], "median_ms": s["median"], "spread_ms": s["spread"]}
    rec["extra_ms_per_sub_sample"] = (rec["shutter"]["median_ms"] - rec["maps_only"]["median_ms"]) / subs
    rec["one_read_of_a_sub_sample_at_the_ceiling_ms"] = 16.0 * c.w * c.h / STREAM_CEILING * 1e3
    rec["shutter_over_maps_only"] = rec["shutter"]["median_ms"] / rec["maps_only"]["median_ms"]
    print(json.dumps({name: {"maps_only_ms": rec["maps_only"]["median_ms"], "shutter_ms": rec["shutter"]["median_ms"],
                             "extra_ms_per_sub_sample": rec["extra_ms_per_sub_sample"],
                             "one_read_ms": rec["one_read_of_a_sub_sample_at_the_ceiling_ms"]}}), flush=True)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", required=True, choices=["clip", "combine", "run"])
    ap.add_argument("--out", default=None)
    ap.add_argument("--commit", default="unknown")
    ap.add_argument("--cases", default=None, help="a subset (the record keeps the others)")
    ap.add_argument("--case", default="ident_1080_k4")
    ap.add_argument("--variant", default="shutter", choices=["shutter", "maps_only"])
    ap.add_argument("--rounds", type=int, default=7)
    args = ap.parse_args()
    import torch
    if args.part == "run":
        c = Case(args.case)
        for _ in range(args.rounds):
            getattr(c, args.variant)()
        torch.cuda.synchronize()
        return 0
    if not args.out:
        ap.error("--out is required")
    record = {}
    if os.path.exists(args.out):
        with open(args.out) as f:
            record = json.load(f)
    record["commit"] = args.commit
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)

    def save():
        with open(args.out, "w") as f:
            json.dump(record, f, indent=1)
            f.write("\n")
    if args.part == "combine":
        part = record.setdefault("combine_alone", {})
        part.update({"device": torch.cuda.get_device_name(0), "rounds": args.rounds, "bpp": 4, "streaming_ceiling_bytes_per_s": STREAM_CEILING,
                     "timing": "device events around one launch of k_shutter_combine_clip over one frame's K sub-sample maps (every "
                               "float 0.25); supersample_combine_clip: mmhip_selftest_combine_ms's clip kernel in the same process"})
        cases, measure = COMBINE_CASES, measure_combine
    else:
        part = record.setdefault("clip_against_its_sub_sample_maps", {})
        part.update({"device": torch.cuda.get_device_name(0), "rounds": args.rounds, "order": "maps_only, shutter, maps_only, shutter, ...",
                     "timing": "device events around one render_clip(floatmap=True) call of the N * K (frame, t) pairs, or one "
                               "render_clip(shutter_samples=K) call of the N frames into RGBA8"})
        cases, measure = CASES, measure_clip
    part.setdefault("cases", {})
    for name in (args.cases.split(",") if args.cases else list(cases)):
        part["cases"][name] = measure(name, args)
        save()
    return 0


if __name__ == "__main__":
    sys.exit(main())
