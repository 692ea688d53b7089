"""What clip rendering costs and buys: the existing workloads against the parent commit, and one batched launch against
the loop of single renders.

Parts, each merged into the record at --out (stamped with --commit):

  --part ab    bench.py (default workload, ident, droste, pond) of a build of the parent commit (--parent DIR, a checkout
               of it built in place) and of this tree, alternating, --runs runs per side, one process per run: the A/B of
               tools/sequence_cost.py.  Nothing on these workloads' path changes with clip rendering.
  --part clip  the same --frames frames (frame = i, t = i / N: render_clip's and the command line's convention), rendered
               by one render_clip call and by a loop of render_rows calls into the same [N][H][W][4] buffer, on one
               invocation, the two variants alternating for --rounds rounds with device events around each region.  Cases:
               Ident and Pond at 512^2, 1920x1080 and 8192^2, Mandelbrot (generic and specialised) and a slit-scan over
               a 5-frame input at 1920x1080.  Per case: ms per frame of every round, medians, spreads, Mpixels/s, the
               rows per work-item of both geometries, the loop / clip ratio, and that the two buffers hold the same bytes.
               At 8192^2 the record also says whether the clip is slower than the loop by more than the loop's spread.
  --part run   one variant of one case, --rounds times, untimed: what a kernel trace is collected from
               (rocprofv3 --kernel-trace --stats -- python tools/clip_cost.py --part run --case ident_1080 --variant clip).

    python tools/clip_cost.py --part ab --parent <dir> --out profiles/r07_clip_cost.json --commit <sha>
    python tools/clip_cost.py --part clip --out profiles/r07_clip_cost.json --commit <sha>
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from sequence_cost import median, part_ab      # noqa: E402  (the A/B against the parent is that tool's)

K = 5
SLIT = "filter clip_cost_slit (image in)\n  in(xy, 2.5 + 2.5 * x)\nend\n"
# name -> (filter, width, height, frames of the bound input)
CASES = {
    "ident_512": ("ident", 512, 512, 1), "ident_1080": ("ident", 1920, 1080, 1), "ident_8192": ("ident", 8192, 8192, 1),
    "pond_512": ("pond", 512, 512, 1), "pond_1080": ("pond", 1920, 1080, 1), "pond_8192": ("pond", 8192, 8192, 1),
    "mandelbrot_1080": ("mandelbrot", 1920, 1080, 0), "mandelbrot_specialised_1080": ("mandelbrot+", 1920, 1080, 0),
    "slit_scan_1080": ("slit", 1920, 1080, K),
}


class Case:
    def __init__(self, name, frames):
        import numpy as np
        import torch
        import mathmap_amd as mm
        from mathmap_amd.striping import animation_frame_t
        from tests import filters as F
        which, self.w, self.h, in_frames = CASES[name]
        self.name, self.n = name, frames
        self.flt = mm.Filter(SLIT) if which == "slit" else F.load(which.rstrip("+"), specialize=which.endswith("+"))
        self.inv = self.flt.invoke(self.w, self.h)
        if in_frames:
            g = torch.Generator(device="cuda").manual_seed(7)
            self.image = torch.randint(-2 ** 31, 2 ** 31 - 1, (in_frames, self.h, self.w), dtype=torch.int32, device="cuda", generator=g)
            self.inv.set_image_device("in", self.image.data_ptr(), self.w, self.h, keepalive=self.image, num_frames=in_frames)
        self.frames = np.arange(frames, dtype=np.int32)
        self.ts = np.array([animation_frame_t(i, frames) for i in range(frames)], dtype=np.float32)
        self.out = torch.empty((frames, self.h, self.w, 4), dtype=torch.uint8, device="cuda")
        self.stream = torch.cuda.current_stream().cuda_stream
        self.frame_bytes = self.w * self.h * 4

    def clip(self):
        self.inv.render_clip(frames=self.frames, ts=self.ts, out_ptr=self.out.data_ptr(), stream=self.stream)

    def loop(self):
        base = self.out.data_ptr()
        for i in range(self.n):
            self.inv.render_rows(base + i * self.frame_bytes, 0, self.h, t=float(self.ts[i]), frame=i, stream=self.stream)

    def geometry(self):
        # (a specialising filter renders with the variant of its current values)
        active = self.flt.specialized() if CASES[self.name][0].endswith("+") else self.flt
        one, clip = active.launch_geometry(self.w, self.h), active.clip_launch_geometry(self.w, self.h, self.n)
        keys = ("ppt", "nwg", "wg1", "tile_w", "tile_h", "unroll", "pair_mode", "single_pixel", "xcd_order")
        return {"single": {k: one[k] for k in keys}, "clip": {k: clip[k] for k in keys},
                "plan": active.clip_batch_plan(self.w, self.h, self.n)}


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
    want = c.out.clone() if c.out.numel() <= (1 << 31) else c.out[:4].clone()
    c.out.zero_()
    before = c.inv.clip_batched_launches()
    c.clip()
    torch.cuda.synchronize()
    same = bool(torch.equal(want, c.out[:want.shape[0]]))
    batches = c.inv.clip_batched_launches() - before
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
    rec = {"filter": CASES[name][0], "width": c.w, "height": c.h, "frames": c.n, "geometry": c.geometry(), "batches": batches,
           "clip_equals_loop": same}
    for variant in ms:
        m = median(ms[variant])
        rec[variant] = {"ms_per_frame": ms[variant], "median_ms": m, "spread_ms": max(ms[variant]) - min(ms[variant]),
                        "mpix_s": c.w * c.h / (m * 1e-3) / 1e6}
    rec["loop_over_clip"] = rec["loop"]["median_ms"] / rec["clip"]["median_ms"]
    if c.w == 8192:
        rec["clip_slower_than_loop_by_more_than_its_spread"] = rec["clip"]["median_ms"] > rec["loop"]["median_ms"] + rec["loop"]["spread_ms"]
    print(json.dumps({name: {"loop_ms": rec["loop"]["median_ms"], "clip_ms": rec["clip"]["median_ms"], "loop_over_clip": rec["loop_over_clip"],
                             "spreads": [rec["loop"]["spread_ms"], rec["clip"]["spread_ms"]], "ppt": [rec["geometry"]["single"]["ppt"], rec["geometry"]["clip"]["ppt"]],
                             "same": same}}), flush=True)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", required=True, choices=["ab", "clip", "run"])
    ap.add_argument("--out", default=None)
    ap.add_argument("--commit", default="unknown")
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit (--part ab)")
    ap.add_argument("--workloads", default="mandelbrot,ident,droste,pond", help="--part ab: a subset (the record keeps the others)")
    ap.add_argument("--cases", default=",".join(CASES), help="--part clip: a subset (the record keeps the others)")
    ap.add_argument("--case", default="ident_1080")
    ap.add_argument("--variant", default="clip", choices=["clip", "loop"])
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--steps", type=int, default=240)
    ap.add_argument("--warmup", type=int, default=24)
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
    if args.part == "ab":
        for done in part_ab(args, record.get("existing_workloads", {})):       # saved after every workload
            record["existing_workloads"] = done
            save()
        return 0
    import torch
    clip = record.setdefault("clip_against_loop", {})
    clip.update({"device": torch.cuda.get_device_name(0), "rounds": args.rounds, "order": "loop, clip, loop, clip, ...",
                 "timing": "device events around the whole region -- one render_clip call, or N render_rows calls -- of the same N "
                           "frames into the same buffer, per frame; the host's launch cost is inside where the GPU waits for it"})
    clip.setdefault("cases", {})
    for name in args.cases.split(","):
        clip["cases"][name] = measure(name, args)
        save()
    return 0


if __name__ == "__main__":
    sys.exit(main())
