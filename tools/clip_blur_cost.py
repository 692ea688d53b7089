"""What batching gaussian_blur over the frames of a clip costs and buys: one render_clip call against the loop of single
renders it replaces, on one build and one invocation.

  --part clip  the same --frames frames (frame = i, t = i / N) by one render_clip call and by a loop of render_rows calls
               into the same [N][H][W][4] buffer, the two variants alternating for --rounds rounds, device events around
               each whole region (the host's round trips are inside where the GPU waits for them).  Cases: the direct blur
               (the blur's bytes are the frame) and the blur sampled at distorted coordinates, sigma 3 px and 20 px
               following t, at 512^2, 1280x720, 1920x1080, 3840x2160 and 8192^2.  A case takes as many frames as the
               native plan puts in one batch, at most --frames.  Per case: ms per frame of every round, medians, spreads,
               the loop / clip ratio, the native counters, per-kernel times of one extra timed round of each variant
               (mmhip_drain_native_kernel_ms), that the two buffers hold the same bytes, and whether the clip is slower
               than the loop by more than the loop's spread.
  --part run   one variant of one case, --rounds times, untimed: what a kernel trace is collected from.

    python tools/clip_blur_cost.py --part clip --out profiles/r08_clip_blur_cost.json --commit <sha>
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from sequence_cost import median      # noqa: E402

SIZES = {"512": (512, 512), "720": (1280, 720), "1080": (1920, 1080), "2160": (3840, 2160), "8192": (8192, 8192)}
# sigma in pixels = dev * (extent - 1) / 2 (gauss.c:659-660); the blur's deviations run from sigma to 1.25 sigma over the clip
DIRECT = "stretched filter blur_cost_direct (stretched image in, float sx: 0-1 (0.01), float sy: 0-1 (0.01))\n" \
         "  b = gaussian_blur(in, sx * (1 + t * 0.25), sy * (1 + t * 0.25));\n  b(xy)\nend\n"
DISTORTED = "stretched filter blur_cost_distorted (stretched image in, float sx: 0-1 (0.01), float sy: 0-1 (0.01))\n" \
            "  b = gaussian_blur(in, sx * (1 + t * 0.25), sy * (1 + t * 0.25));\n" \
            "  b(xy * 0.9 + xy:[0.05 * sin(t * 6), 0.02]) * 0.6 + in(xy) * 0.4\nend\n"
CASES = {"%s_%s_s%d" % (kind, size, sigma): (kind, size, sigma)
         for kind in ("direct", "distorted") for size in SIZES for sigma in (3, 20)}


class Case:
    def __init__(self, name, frames):
        import numpy as np
        import torch
        import mathmap_amd as mm
        from mathmap_amd.striping import animation_frame_t
        kind, size, sigma = CASES[name]
        self.w, self.h = SIZES[size]
        self.name = name
        self.flt = mm.Filter(DIRECT if kind == "direct" else DISTORTED)
        self.plan = self.flt.clip_native_plan(self.w, self.h, frames)
        self.n = max(1, min(frames, self.plan["frames_per_batch"] or frames))
        self.inv = self.flt.invoke(self.w, self.h)
        self.inv.set("sx", 2.0 * sigma / (self.w - 1))
        self.inv.set("sy", 2.0 * sigma / (self.h - 1))
        g = torch.Generator(device="cuda").manual_seed(7)
        self.image = torch.randint(-2 ** 31, 2 ** 31 - 1, (self.h, self.w), dtype=torch.int32, device="cuda", generator=g)
        self.inv.set_image_device("in", self.image.data_ptr(), self.w, self.h, keepalive=self.image)
        self.frames = np.arange(self.n, dtype=np.int32)
        self.ts = np.array([animation_frame_t(i, self.n) for i in range(self.n)], dtype=np.float32)
        self.out = torch.empty((self.n, self.h, self.w, 4), dtype=torch.uint8, device="cuda")
        self.stream = torch.cuda.current_stream().cuda_stream
        self.frame_bytes = self.w * self.h * 4

    def clip(self):
        self.inv.render_clip(frames=self.frames, ts=self.ts, out_ptr=self.out.data_ptr(), stream=self.stream)

    def loop(self):
        base = self.out.data_ptr()
        for i in range(self.n):
            self.inv.render_rows(base + i * self.frame_bytes, 0, self.h, t=float(self.ts[i]), frame=i, stream=self.stream)

    def counters(self):
        return [self.inv.clip_native_batches(), self.inv.clip_native_blurs(), self.inv.clip_native_direct_frames()]


def kernel_times(c, variant):
    """ms per frame by kernel label, from one timed run of the variant."""
    import torch
    c.inv.enable_timing(True)
    c.inv.drain_native_kernel_ms()
    getattr(c, variant)()
    torch.cuda.synchronize()
    got = c.inv.drain_native_kernel_ms()
    c.inv.drain_kernel_ms()
    c.inv.enable_timing(False)
    out = {}
    for label, ms in got:
        out[label] = out.get(label, 0.0) + ms / c.n
    return out


def measure(name, args):
    import torch
    c = Case(name, args.frames)
    for _ in range(2):
        c.loop()
        c.clip()
    torch.cuda.synchronize()
    c.out.zero_()
    c.loop()
    torch.cuda.synchronize()
    keep = min(c.n, max(1, (1 << 30) // c.frame_bytes))
    want = c.out[:keep].clone()
    c.out.zero_()
    before = c.counters()
    c.clip()
    torch.cuda.synchronize()
    same = bool(torch.equal(want, c.out[:keep]))
    per_call = [b - a for a, b in zip(before, c.counters())]
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
    rec = {"filter": CASES[name][0], "width": c.w, "height": c.h, "sigma_px": CASES[name][2], "frames": c.n, "native_plan": c.plan,
           "native_counters_per_call": dict(zip(("batches", "blurs", "direct_frames"), per_call)), "clip_equals_loop": same}
    for variant in ms:
        m = median(ms[variant])
        rec[variant] = {"ms_per_frame": ms[variant], "median_ms": m, "spread_ms": max(ms[variant]) - min(ms[variant]),
                        "mpix_s": c.w * c.h / (m * 1e-3) / 1e6, "kernel_ms_per_frame": kernel_times(c, variant)}
    rec["loop_over_clip"] = rec["loop"]["median_ms"] / rec["clip"]["median_ms"]
    rec["clip_slower_than_loop_by_more_than_its_spread"] = rec["clip"]["median_ms"] > rec["loop"]["median_ms"] + rec["loop"]["spread_ms"]
    print(json.dumps({name: {"frames": c.n, "loop_ms": rec["loop"]["median_ms"], "clip_ms": rec["clip"]["median_ms"],
                             "loop_over_clip": rec["loop_over_clip"], "spreads": [rec["loop"]["spread_ms"], rec["clip"]["spread_ms"]],
                             "counters": per_call, "same": same}}), flush=True)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", required=True, choices=["clip", "run"])
    ap.add_argument("--out", default=None)
    ap.add_argument("--commit", default="unknown")
    ap.add_argument("--cases", default=",".join(CASES), help="--part clip: a subset (the record keeps the others)")
    ap.add_argument("--case", default="direct_1080_s3")
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
    import torch
    clip = record.setdefault("clip_against_loop", {})
    clip.update({"device": torch.cuda.get_device_name(0), "rounds": args.rounds, "order": "loop, clip, loop, clip, ...",
                 "timing": "device events around the whole region -- one render_clip call, or N render_rows calls -- of the same N "
                           "frames into the same buffer, per frame; the host's round trips are inside where the GPU waits for them"})
    clip.setdefault("cases", {})
    for name in args.cases.split(","):
        clip["cases"][name] = measure(name, args)
        with open(args.out, "w") as f:
            json.dump(record, f, indent=1)
            f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
