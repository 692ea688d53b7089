"""What batching supersampled clips costs and buys: one mmhip_render_clip_supersampled call against the loop of
mmhip_render_supersampled, and the clip's combine kernel against the single-frame one.

Parts, each merged into the record at --out (stamped with --commit):

  --part clip     the same N frames (frame = i, t = i / N) rendered supersampled by one render_clip(supersample=True) call
                  and by a loop of mmhip_render_supersampled calls into the same [N][H][W][4] buffer, on one invocation,
                  the two variants alternating for --rounds rounds with device events around each region.  N is --frames or
                  what one batch holds (the plan's frames_per_batch), whichever is smaller.  Cases: Ident, Pond and the
                  specialised Mandelbrot at 512^2, 1920x1080 and 8192^2.  Per case: ms per frame of every round, medians,
                  spreads (max - min), the loop / clip ratio, whether the clip is slower than the loop by more than the
                  loop's spread, and that the two buffers hold the same bytes.
  --part combine  k_supersample_combine_clip against launch_supersample_combine on the same slices of pseudo-random bytes
                  (mmhip_selftest_combine_ms), bpp 4, at 1920x1080 and 8192^2: microseconds per frame, achieved bytes/s at
                  12 B/px against the streaming ceiling, and whether the new kernel is slower than the old one by more
                  than the old one's spread.
  --part run      one variant of one case, --rounds times, untimed: what a kernel trace is collected from.

    python tools/clip_ss_cost.py --part clip --out profiles/r10_clip_ss_cost.json --commit <sha>
    python tools/clip_ss_cost.py --part combine --out profiles/r10_clip_ss_cost.json --commit <sha>
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
SIZES = {"512": (512, 512), "1080": (1920, 1080), "8192": (8192, 8192)}
CASES = {"%s_%s" % (f.rstrip("+"), s): (f, w, h) for f in ("ident", "pond", "mandelbrot+") for s, (w, h) in SIZES.items()}
COMBINE_CASES = {"1080": (1920, 1080, 32), "8192": (8192, 8192, 3)}      # width, height, frames


class Case:
    def __init__(self, name, frames):
        import numpy as np
        import torch
        from mathmap_amd._lib import lib
        from mathmap_amd.striping import animation_frame_t
        from tests import filters as F
        which, self.w, self.h = CASES[name]
        self.name = name
        self.flt = F.load(which.rstrip("+"), specialize=which.endswith("+"), supersampling=True)
        active = self.flt.specialized() if which.endswith("+") else self.flt
        self.plan = active.clip_supersample_plan(self.w, self.h, frames)
        self.n = max(1, min(frames, self.plan["frames_per_batch"]))
        self.inv = self.flt.invoke(self.w, self.h)
        if F.image_names(self.flt):
            g = torch.Generator(device="cuda").manual_seed(7)
            self.image = torch.randint(-2 ** 31, 2 ** 31 - 1, (self.h, self.w), dtype=torch.int32, device="cuda", generator=g)
            self.inv.set_image_device("in", self.image.data_ptr(), self.w, self.h, keepalive=self.image)
        self.frames = np.arange(self.n, dtype=np.int32)
        self.ts = np.array([animation_frame_t(i, self.n) for i in range(self.n)], dtype=np.float32)
        self.out = torch.empty((self.n, self.h, self.w, 4), dtype=torch.uint8, device="cuda")
        self.stream = torch.cuda.current_stream().cuda_stream
        self.frame_bytes = self.w * self.h * 4
        self.lib = lib()

    def clip(self):
        self.inv.render_clip(frames=self.frames, ts=self.ts, out_ptr=self.out.data_ptr(), stream=self.stream, supersample=True)

    def loop(self):
        base = self.out.data_ptr()
        for i in range(self.n):
            rc = self.lib.mmhip_render_supersampled(self.inv._h, i, float(self.ts[i]), 0, 0, self.w, self.h, C.c_void_p(base + i * self.frame_bytes),
                                                    self.w * 4, 4, C.c_void_p(self.stream))
            assert rc == 0, self.lib.mmhip_last_error()


def summary(values):
    return {"values": values, "median": median(values), "spread": max(values) - min(values)}


def measure_clip(name, args):
    import torch
    c = Case(name, args.frames)
    for _ in range(2):
        c.loop()
        c.clip()
    torch.cuda.synchronize()
    c.out.zero_()
    c.loop()
    torch.cuda.synchronize()
    want = c.out.clone()
    c.out.zero_()
    before = c.inv.clip_supersampled_batches()
    c.clip()
    torch.cuda.synchronize()
    same = bool(torch.equal(want, c.out))
    batches = c.inv.clip_supersampled_batches() - before
    del want
    ms = {"loop": [], "clip": []}
    for _ in range(args.rounds):
        for variant in ("loop", "clip"):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            getattr(c, variant)()
            e1.record()
            torch.cuda.synchronize()
            ms[variant].append(e0.elapsed_time(e1) / c.n)
    rec = {"filter": CASES[name][0], "width": c.w, "height": c.h, "frames": c.n, "plan": c.plan, "batches": batches, "clip_equals_loop": same}
    for variant in ms:
        s = summary(ms[variant])
        rec[variant] = {"ms_per_frame": s["values"], "median_ms": s["median"], "spread_ms": s["spread"]}
    rec["loop_over_clip"] = rec["loop"]["median_ms"] / rec["clip"]["median_ms"]
    rec["clip_slower_than_loop_by_more_than_its_spread"] = rec["clip"]["median_ms"] > rec["loop"]["median_ms"] + rec["loop"]["spread_ms"]
    print(json.dumps({name: {"frames": c.n, "loop_ms": rec["loop"]["median_ms"], "clip_ms": rec["clip"]["median_ms"],
                             "loop_over_clip": rec["loop_over_clip"], "spreads": [rec["loop"]["spread_ms"], rec["clip"]["spread_ms"]],
                             "slower": rec["clip_slower_than_loop_by_more_than_its_spread"], "same": same}}), flush=True)
    return rec


def measure_combine(name, args):
    from mathmap_amd._lib import selftest_lib
    w, h, frames = COMBINE_CASES[name]
    ms = (C.c_double * (2 * args.rounds))()
    differ = selftest_lib().mmhip_selftest_combine_ms(w, h, 4, frames, args.rounds, ms)
    assert differ >= 0, selftest_lib().mmhip_selftest_error()
    rec = {"width": w, "height": h, "frames": frames, "bytes_that_differ": differ}
    for k, variant in enumerate(("single_frame_kernel", "clip_kernel")):
        s = summary([ms[2 * r + k] * 1e3 / frames for r in range(args.rounds)])
        rec[variant] = {"us_per_frame": s["values"], "median_us": s["median"], "spread_us": s["spread"],
                        "bytes_per_s_at_12_B_per_px": 12.0 * w * h / (s["median"] * 1e-6)}
        rec[variant]["share_of_streaming_ceiling"] = rec[variant]["bytes_per_s_at_12_B_per_px"] / STREAM_CEILING
    old, new = rec["single_frame_kernel"], rec["clip_kernel"]
    rec["old_over_new"] = old["median_us"] / new["median_us"]
    rec["new_slower_than_old_by_more_than_its_spread"] = new["median_us"] > old["median_us"] + old["spread_us"]
    print(json.dumps({name: {"old_us": old["median_us"], "new_us": new["median_us"], "old_over_new": rec["old_over_new"],
                             "new_share_of_ceiling": new["share_of_streaming_ceiling"], "differ": differ}}), flush=True)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", required=True, choices=["clip", "combine", "run"])
    ap.add_argument("--out", default=None)
    ap.add_argument("--commit", default="unknown")
    ap.add_argument("--cases", default=None, help="a subset (the record keeps the others)")
    ap.add_argument("--case", default="ident_1080")
    ap.add_argument("--variant", default="clip", choices=["clip", "loop"])
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--frames", type=int, default=120)
    args = ap.parse_args()
    if args.part == "run":
        import torch
        c = Case(args.case, args.frames)
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
    import torch
    if args.part == "clip":
        part = record.setdefault("clip_against_loop", {})
        part.update({"device": torch.cuda.get_device_name(0), "rounds": args.rounds, "order": "loop, clip, loop, clip, ...",
                     "timing": "device events around the whole region -- one mmhip_render_clip_supersampled call, or N "
                               "mmhip_render_supersampled calls -- of the same N frames into the same buffer, per frame"})
        cases, measure = CASES, measure_clip
    else:
        part = record.setdefault("combine_alone", {})
        part.update({"device": torch.cuda.get_device_name(0), "rounds": args.rounds, "order": "old, new, old, new, ...", "bpp": 4,
                     "streaming_ceiling_bytes_per_s": STREAM_CEILING,
                     "timing": "device events around the combines of all frames: one launch of the single-frame kernel per frame, "
                               "or one launch of the clip kernel; the slices hold pseudo-random bytes"})
        cases, measure = COMBINE_CASES, measure_combine
    part.setdefault("cases", {})
    for name in (args.cases.split(",") if args.cases else list(cases)):
        part["cases"][name] = measure(name, args)
        save()
    return 0


if __name__ == "__main__":
    sys.exit(main())
