"""What fused motion blur costs against the path through sub-sample maps, and what its kernel takes in registers.

Parts, each merged into the record at --out (stamped with --commit):

  --part clip       Ident, the specialised Mandelbrot, Pond and Droste at 1920x1080 (8 frames) and 8192^2 (1 frame) with
                    K = 4 and 8: one render_clip(shutter_mode="fused") and one render_clip(shutter_mode="maps") of the
                    same frames into the same out_ptr (RGBA8), alternating for --rounds rounds, each timed by the host
                    clock between two stream synchronisations around the call.  Per case the medians, the spreads,
                    fused / maps, and the 32 K bytes per pixel the fused call does not move at the streaming ceiling.
  --part registers  no GPU needed: per filter the VGPR and SGPR counts and .private_segment_fixed_size of
                    mm_pixels_shutter, beside those of mm_pixels_clip in the single-pixel shape (the filter compiled
                    under MMHIP_SINGLE_PIXEL=1, in a child process), from the gfx950 assembly of both texts under the
                    JIT's options.
  --part run        one variant of one case, --rounds times, untimed: what a kernel trace is collected from.

    python tools/shutter_fused_cost.py --part clip --out profiles/r13_shutter_fused_cost.json --commit <sha>
    python tools/shutter_fused_cost.py --part registers --out profiles/r13_shutter_fused_cost.json --commit <sha>
"""
import argparse
import json
import os
import re
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from sequence_cost import median      # noqa: E402

STREAM_CEILING = 6.3e12      # bytes/s, DESIGN section 3
SIZES = {"1080": (1920, 1080), "8192": (8192, 8192)}
SAMPLES = (4, 8)
FRAMES = {"1080": 8, "8192": 1}       # output frames of a case (8192^2 with K = 8: 8 GiB of sub-sample maps)
FILTERS = ("ident", "mandelbrot+", "pond", "droste")          # +: compiled with specialize=True
CASES = {"%s_%s_k%d" % (f.rstrip("+"), s, k): (f, s, k) for f in FILTERS for s in SIZES for k in SAMPLES}


def summary(values):
    return {"ms": values, "median_ms": median(values), "spread_ms": max(values) - min(values)}


def load(which):
    from tests import filters as F
    return F.load(which.rstrip("+"), specialize=which.endswith("+"))


class Case:
    def __init__(self, name):
        import numpy as np
        import torch
        from mathmap_amd.striping import animation_frame_t
        from tests import filters as F
        which, size, self.k = CASES[name]
        self.w, self.h = SIZES[size]
        self.n = FRAMES[size]
        self.flt = load(which)
        self.inv = self.flt.invoke(self.w, self.h)
        if F.image_names(self.flt):
            g = torch.Generator(device="cuda").manual_seed(7)
            self.image = torch.randint(-2 ** 31, 2 ** 31 - 1, (self.h, self.w), dtype=torch.int32, device="cuda", generator=g)
            self.inv.set_image_device("in", self.image.data_ptr(), self.w, self.h, keepalive=self.image)
        self.frames = np.arange(self.n, dtype=np.int32)
        self.ts = np.array([animation_frame_t(i, self.n) for i in range(self.n)], dtype=np.float32)
        self.span = float(np.float32(0.5 / self.n))
        self.out = torch.empty((self.n, self.h, self.w, 4), dtype=torch.uint8, device="cuda")
        self.stream = torch.cuda.current_stream().cuda_stream
        active = self.flt.specialized() if which.endswith("+") else self.flt
        self.plans = {"fused": active.clip_shutter_fused_plan(self.w, self.h, self.k, self.n),
                      "maps": active.clip_shutter_plan(self.w, self.h, self.w, self.k, self.n)}
        self.geometry = active.clip_launch_geometry(self.w, self.h, self.n * self.k)

    def render(self, mode):
        self.inv.render_clip(frames=self.frames, ts=self.ts, out_ptr=self.out.data_ptr(), stream=self.stream, shutter_samples=self.k,
                             shutter_span=self.span, shutter_mode=mode)


def measure_clip(name, args):
    import torch
    c = Case(name)
    sums = {}
    for mode in ("maps", "fused", "maps", "fused"):          # warm-up: the modules are built, the temporaries allocated
        c.render(mode)
        torch.cuda.synchronize()
        sums[mode] = int(c.out.view(torch.int32).sum(dtype=torch.int64).item())
    assert sums["fused"] == sums["maps"], (name, "the two paths wrote other bytes")
    ms = {"fused": [], "maps": []}
    for _ in range(args.rounds):
        for mode in ("fused", "maps"):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            c.render(mode)
            torch.cuda.synchronize()
            ms[mode].append((time.perf_counter() - t0) * 1e3)
    rec = {"filter": CASES[name][0], "width": c.w, "height": c.h, "frames": c.n, "samples": c.k, "plans": c.plans,
           "maps_pixel_kernel": {k: c.geometry[k] for k in ("pair_mode", "single_pixel", "unroll", "ppt")},
           "fused_batches": c.inv.clip_shutter_fused_batches()}
    for mode in ms:
        rec[mode] = summary(ms[mode])
    rec["fused_over_maps"] = rec["fused"]["median_ms"] / rec["maps"]["median_ms"]
    rec["maps_minus_fused_ms"] = rec["maps"]["median_ms"] - rec["fused"]["median_ms"]
    rec["sub_sample_round_trip_at_the_ceiling_ms"] = 32.0 * c.k * c.w * c.h * c.n / STREAM_CEILING * 1e3
    print(json.dumps({name: {"fused_ms": rec["fused"]["median_ms"], "maps_ms": rec["maps"]["median_ms"], "fused_over_maps": rec["fused_over_maps"],
                             "round_trip_ms": rec["sub_sample_round_trip_at_the_ceiling_ms"]}}), flush=True)
    return rec


# ---- registers ----

def kernel_resources(asm, kernel):
    """vgpr_count, sgpr_count and private_segment_fixed_size of `kernel` from the metadata at the end of the assembly."""
    meta = asm[asm.index("amdhsa.kernels:"):]
    for entry in meta.split("\n  - ")[1:]:
        if not re.search(r"\.name:\s+%s\s*$" % re.escape(kernel), entry, re.M):
            continue
        return {field: int(re.search(r"\.%s:\s+(\d+)" % field, entry).group(1))
                for field in ("vgpr_count", "sgpr_count", "agpr_count", "private_segment_fixed_size")}
    raise KeyError(kernel)


def print_text(which, variant):
    flt = load(which)
    if which.endswith("+"):
        flt = flt.specialized()
    sys.stdout.write(flt.shutter_kernel_source if variant == "shutter" else flt.clip_kernel_source)


def measure_registers(which):
    from pair_loop_isa import assembly
    rec = {}
    for variant, kernel, env in (("shutter", "mm_pixels_shutter", {}), ("clip_single_pixel", "mm_pixels_clip", {"MMHIP_SINGLE_PIXEL": "1"})):
        text = subprocess.run([sys.executable, os.path.abspath(__file__), "--part", "text", "--filter", which, "--variant", variant],
                              env=dict(os.environ, **env), check=True, capture_output=True, text=True).stdout
        assert kernel + "(" in text
        rec[variant] = dict(kernel_resources(assembly(text), kernel), kernel=kernel)
    print(json.dumps({which: rec}), flush=True)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", required=True, choices=["clip", "registers", "run", "text"])
    ap.add_argument("--out", default=None)
    ap.add_argument("--commit", default="unknown")
    ap.add_argument("--cases", default=None, help="a subset (the record keeps the others)")
    ap.add_argument("--case", default="ident_1080_k4")
    ap.add_argument("--filter", default="ident")
    ap.add_argument("--variant", default="fused")
    ap.add_argument("--rounds", type=int, default=7)
    args = ap.parse_args()
    if args.part == "text":
        print_text(args.filter, args.variant)
        return 0
    if args.part == "run":
        import torch
        c = Case(args.case)
        for _ in range(args.rounds):
            c.render(args.variant)
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
    if args.part == "registers":
        part = record.setdefault("registers", {})
        part.update({"taken": "without a GPU, from the gfx950 assembly of the generated texts under the JIT's options",
                     "clip_single_pixel": "mm_pixels_clip of the filter compiled under MMHIP_SINGLE_PIXEL=1"})
        part.setdefault("filters", {})
        for which in (args.cases.split(",") if args.cases else FILTERS):
            part["filters"][which.rstrip("+")] = measure_registers(which)
            save()
        return 0
    import torch
    part = record.setdefault("fused_against_maps", {})
    part.update({"device": torch.cuda.get_device_name(0), "rounds": args.rounds, "order": "fused, maps, fused, maps, ...",
                 "streaming_ceiling_bytes_per_s": STREAM_CEILING,
                 "timing": "host clock between two stream synchronisations around one render_clip(shutter_samples=K) call of the N "
                           "frames into RGBA8, both modes into the same out_ptr"})
    part.setdefault("cases", {})
    for name in (args.cases.split(",") if args.cases else list(CASES)):
        part["cases"][name] = measure_clip(name, args)
        save()
    return 0


if __name__ == "__main__":
    sys.exit(main())
