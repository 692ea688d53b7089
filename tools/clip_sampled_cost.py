"""What fused grid supersampling costs against the path through sub-sample maps, and what its kernel takes in registers.

Parts, each merged into the record at --out (stamped with --commit):

  --part clip       Ident, the specialised Mandelbrot, Pond and Droste at 1920x1080 (8 frames) and 8192^2 (1 frame) with
                    aa = 2 at K = 1 and K = 4: one render_clip(aa=2, shutter_mode="fused") and one
                    render_clip(aa=2, shutter_mode="maps") of the same frames into the same out_ptr (RGBA8), alternating
                    for --rounds rounds, each timed by the host clock between two stream synchronisations around the call.
                    The yardstick is the maps path: existing kernels under a different host loop.  Per case the medians,
                    the spreads, fused / maps, and the 32 K G bytes per pixel the fused call does not move at the
                    streaming ceiling.
  --part registers  no GPU needed: per filter the VGPR and SGPR counts and .private_segment_fixed_size of
                    mm_pixels_sampled beside those of mm_pixels_shutter, from the gfx950 assembly of both texts under the
                    JIT's options.

    python tools/clip_sampled_cost.py --part clip --out profiles/r14_clip_sampled_cost.json --commit <sha>
    python tools/clip_sampled_cost.py --part registers --out profiles/r14_clip_sampled_cost.json --commit <sha>
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from shutter_fused_cost import FILTERS, FRAMES, SIZES, STREAM_CEILING, kernel_resources, load, summary      # noqa: E402

AA = 2
SAMPLES = (1, 4)
CASES = {"%s_%s_aa%d_k%d" % (f.rstrip("+"), s, AA, k): (f, s, k) for f in FILTERS for s in SIZES for k in SAMPLES}


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
        self.plans = {"fused": active.clip_sampled_fused_plan(self.w, self.h, self.k, AA, self.n),
                      "maps": active.clip_sampled_plan(self.w, self.h, self.w, self.k, AA, self.n)}

    def render(self, mode):
        self.inv.render_clip(frames=self.frames, ts=self.ts, out_ptr=self.out.data_ptr(), stream=self.stream, shutter_samples=self.k,
                             shutter_span=self.span, shutter_mode=mode, aa=AA)


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
    rec = {"filter": CASES[name][0], "width": c.w, "height": c.h, "frames": c.n, "samples": c.k, "grid": [AA, AA], "plans": c.plans,
           "fused_batches": c.inv.clip_sampled_fused_batches(), "maps_batches": c.inv.clip_sampled_batches()}
    for mode in ms:
        rec[mode] = summary(ms[mode])
    rec["fused_over_maps"] = rec["fused"]["median_ms"] / rec["maps"]["median_ms"]
    rec["maps_minus_fused_ms"] = rec["maps"]["median_ms"] - rec["fused"]["median_ms"]
    rec["sub_sample_round_trip_at_the_ceiling_ms"] = 32.0 * c.k * AA * AA * c.w * c.h * c.n / STREAM_CEILING * 1e3
    print(json.dumps({name: {"fused_ms": rec["fused"]["median_ms"], "maps_ms": rec["maps"]["median_ms"], "fused_over_maps": rec["fused_over_maps"],
                             "round_trip_ms": rec["sub_sample_round_trip_at_the_ceiling_ms"]}}), flush=True)
    return rec


def measure_registers(which):
    from pair_loop_isa import assembly
    flt = load(which)
    if which.endswith("+"):
        flt = flt.specialized()
    rec = {}
    for variant, kernel, text in (("sampled", "mm_pixels_sampled", flt.sampled_kernel_source), ("shutter", "mm_pixels_shutter", flt.shutter_kernel_source)):
        rec[variant] = dict(kernel_resources(assembly(text), kernel), kernel=kernel)
    print(json.dumps({which: rec}), flush=True)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", required=True, choices=["clip", "registers"])
    ap.add_argument("--out", required=True)
    ap.add_argument("--commit", default="unknown")
    ap.add_argument("--cases", default=None, help="a subset (the record keeps the others)")
    ap.add_argument("--rounds", type=int, default=7)
    args = ap.parse_args()
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
        part["taken"] = "without a GPU, from the gfx950 assembly of the generated texts under the JIT's options"
        part.setdefault("filters", {})
        for which in (args.cases.split(",") if args.cases else FILTERS):
            part["filters"][which.rstrip("+")] = measure_registers(which)
            save()
        return 0
    import torch
    part = record.setdefault("fused_against_maps", {})
    part.update({"device": torch.cuda.get_device_name(0), "rounds": args.rounds, "order": "fused, maps, fused, maps, ...",
                 "streaming_ceiling_bytes_per_s": STREAM_CEILING,
                 "timing": "host clock between two stream synchronisations around one render_clip(aa=2, shutter_samples=K) call of the N "
                           "frames into RGBA8, both modes into the same out_ptr"})
    part.setdefault("cases", {})
    for name in (args.cases.split(",") if args.cases else list(CASES)):
        part["cases"][name] = measure_clip(name, args)
        save()
    return 0


if __name__ == "__main__":
    sys.exit(main())
