"""What a reconstruction filter costs a grid-supersampled clip: render_clip(aa=n, aa_filter=...) against render_clip(aa=n)
of the same grid on the maps path, whose only differences are the halo's extra pixels and the wider combine.

Eight-frame clips of the specialised Mandelbrot and of Pond at 1920x1080 and 8192^2, aa = 2 and aa = 4, into RGBA8.  Per
case, in one process after a warm-up, the three calls alternate -- plain grid mean, tent at radius 1, Mitchell at radius 2
-- for --rounds rounds, each timed by the host clock between two stream synchronisations around the call.  Then, with
mmhip_enable_timing, --rounds more rounds whose combine launches are read through mmhip_drain_native_kernel_ms:
filter_combine_clip beside shutter_combine_clip, summed over the launches of a call.  The combine must read 16 G bytes per
pixel once and write the output; that is set against the streaming ceiling.

    python tools/clip_filter_cost.py --out profiles/r17_clip_filter_cost.json --commit <sha>
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from shutter_fused_cost import SIZES, STREAM_CEILING, load, summary      # noqa: E402

FRAMES = 8
FILTERS = ("mandelbrot+", "pond")                           # +: compiled with specialize=True
GRIDS = (2, 4)
MODES = {"mean": (None, None), "tent": ("tent", 1.0), "mitchell": ("mitchell", 2.0)}
CASES = {"%s_%s_aa%d" % (f.rstrip("+"), s, aa): (f, s, aa) for f in FILTERS for s in SIZES for aa in GRIDS}


class Case:
    def __init__(self, name):
        import numpy as np
        import torch
        from mathmap_amd.striping import animation_frame_t
        from tests import filters as F
        which, size, self.aa = CASES[name]
        self.w, self.h = SIZES[size]
        self.n = FRAMES
        self.flt = load(which)
        self.inv = self.flt.invoke(self.w, self.h)
        if F.image_names(self.flt):
            g = torch.Generator(device="cuda").manual_seed(7)
            self.image = torch.randint(-2 ** 31, 2 ** 31 - 1, (self.h, self.w), dtype=torch.int32, device="cuda", generator=g)
            self.inv.set_image_device("in", self.image.data_ptr(), self.w, self.h, keepalive=self.image)
        self.frames = np.arange(self.n, dtype=np.int32)
        self.ts = np.array([animation_frame_t(i, self.n) for i in range(self.n)], dtype=np.float32)
        self.out = torch.empty((self.n, self.h, self.w, 4), dtype=torch.uint8, device="cuda")
        self.stream = torch.cuda.current_stream().cuda_stream
        active = self.flt.specialized() if which.endswith("+") else self.flt
        self.plans = {"mean": active.clip_sampled_plan(self.w, self.h, self.w, 1, self.aa, self.n)}
        for mode, (aa_filter, radius) in MODES.items():
            if aa_filter:
                self.plans[mode] = active.clip_filtered_plan(self.w, self.h, self.w, self.h, 1, self.aa, aa_filter, self.n, aa_radius=radius)

    def render(self, mode):
        aa_filter, radius = MODES[mode]
        self.inv.render_clip(frames=self.frames, ts=self.ts, out_ptr=self.out.data_ptr(), stream=self.stream, aa=self.aa, aa_filter=aa_filter,
                             aa_radius=radius)


def measure(name, args):
    import torch
    c = Case(name)
    for mode in list(MODES) * 2:          # warm-up: the modules are built, the temporaries allocated
        c.render(mode)
        torch.cuda.synchronize()
    ms = {mode: [] for mode in MODES}
    for _ in range(args.rounds):
        for mode in MODES:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            c.render(mode)
            torch.cuda.synchronize()
            ms[mode].append((time.perf_counter() - t0) * 1e3)
    # the combine's own time: the launches of one call summed, per round
    c.inv.enable_timing(True)
    combine = {mode: [] for mode in MODES}
    launches = {}
    for _ in range(args.rounds):
        for mode in MODES:
            c.render(mode)
            torch.cuda.synchronize()
            c.inv.drain_kernel_ms()
            label = "filter_combine_clip" if MODES[mode][0] else "shutter_combine_clip"
            got = [t for n, t in c.inv.drain_native_kernel_ms() if n == label]
            launches[mode] = len(got)
            combine[mode].append(sum(got))
    c.inv.enable_timing(False)
    grid = c.aa * c.aa
    pixels = c.w * c.h * c.n
    rec = {"filter": CASES[name][0], "width": c.w, "height": c.h, "frames": c.n, "grid": [c.aa, c.aa], "plans": c.plans,
           "combine_launches": launches, "combine_bytes": (16 * grid + 4) * pixels,
           "combine_at_the_ceiling_ms": (16 * grid + 4) * pixels / STREAM_CEILING * 1e3}
    for mode in MODES:
        rec[mode] = summary(ms[mode])
        rec[mode]["combine"] = summary(combine[mode])
    line = {"mean_ms": rec["mean"]["median_ms"], "mean_combine_ms": rec["mean"]["combine"]["median_ms"], "ceiling_ms": rec["combine_at_the_ceiling_ms"]}
    for mode in ("tent", "mitchell"):
        rec[mode + "_over_mean"] = rec[mode]["median_ms"] / rec["mean"]["median_ms"]
        rec[mode + "_combine_over_mean_combine"] = rec[mode]["combine"]["median_ms"] / rec["mean"]["combine"]["median_ms"]
        line.update({mode + "_ms": rec[mode]["median_ms"], mode + "_combine_ms": rec[mode]["combine"]["median_ms"],
                     mode + "_over_mean": rec[mode + "_over_mean"], mode + "_combine_over_mean_combine": rec[mode + "_combine_over_mean_combine"]})
    print(json.dumps({name: line}), flush=True)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--commit", default="unknown")
    ap.add_argument("--cases", default=None, help="a subset (the record keeps the others)")
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    record = {}
    if os.path.exists(args.out):
        with open(args.out) as f:
            record = json.load(f)
    record["commit"] = args.commit
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    import torch
    record.update({"device": torch.cuda.get_device_name(0), "rounds": args.rounds, "order": "mean, tent, mitchell, mean, tent, mitchell, ...",
                   "streaming_ceiling_bytes_per_s": STREAM_CEILING,
                   "timing": "host clock between two stream synchronisations around one render_clip(aa=n[, aa_filter]) call of the 8 frames "
                             "into RGBA8, all modes into the same out_ptr; the combine from device events around its launches"})
    record.setdefault("cases", {})
    for name in (args.cases.split(",") if args.cases else list(CASES)):
        record["cases"][name] = measure(name, args)
        with open(args.out, "w") as f:
            json.dump(record, f, indent=1)
            f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
