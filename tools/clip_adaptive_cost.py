"""What adaptive anti-aliasing (render_clip(aa=n, aa_threshold=T)) costs against the full grid-supersampled clip and the
plain clip, and what its two kernels take in registers.

Parts, each merged into the record at --out (stamped with --commit):

  --part clip       Ident, the specialised Mandelbrot, Pond and Droste at 1920x1080 (8 frames) and 8192^2 (1 frame) with
                    aa = 2 and aa = 4: render_clip(aa, aa_threshold=0.05) and render_clip(aa, aa_threshold=inf) in auto
                    mode, the full render_clip(aa) in both shutter_modes and the plain render_clip, all of the same
                    frames into the same out_ptr (RGBA8), alternating for --rounds rounds, each timed by the host clock
                    between two stream synchronisations around the call.  The full aa clip and the plain clip run
                    kernels that predate the adaptive call: they are the yardsticks.  Per case the medians, the largest
                    spread, the refined share, adaptive / full aa, and the +inf case minus the plain clip -- what the
                    base map, the mask and the empty refine launch cost.
  --part registers  no GPU needed: per filter the VGPR and SGPR counts and .private_segment_fixed_size of
                    mm_pixels_refine beside those of mm_pixels_sampled, from the gfx950 assembly of both texts under the
                    JIT's options; and the same, with the LDS bytes, for every instance of k_aa_contrast_clip, from the
                    assembly of csrc/clip_combine.hip under the library's options.

    python tools/clip_adaptive_cost.py --part clip --out profiles/r15_clip_adaptive_cost.json --commit <sha>
    python tools/clip_adaptive_cost.py --part registers --out profiles/r15_clip_adaptive_cost.json --commit <sha>
"""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from shutter_fused_cost import FILTERS, FRAMES, SIZES, kernel_resources, load, summary      # noqa: E402

GRIDS = (2, 4)
THRESHOLD = 0.05
CASES = {"%s_%s_aa%d" % (f.rstrip("+"), s, aa): (f, s, aa) for f in FILTERS for s in SIZES for aa in GRIDS}
RENDERS = ("adaptive", "adaptive_inf", "full_maps", "full_fused", "plain")


class Case:
    def __init__(self, name):
        import numpy as np
        import torch
        from mathmap_amd.striping import animation_frame_t
        from tests import filters as F
        which, size, self.aa = CASES[name]
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
        self.out = torch.empty((self.n, self.h, self.w, 4), dtype=torch.uint8, device="cuda")
        self.stream = torch.cuda.current_stream().cuda_stream
        active = self.flt.specialized() if which.endswith("+") else self.flt
        self.plan = active.clip_adaptive_plan(self.w, self.h, self.w, self.aa, self.n)

    def render(self, what):
        kw = dict(frames=self.frames, ts=self.ts, out_ptr=self.out.data_ptr(), stream=self.stream)
        if what == "adaptive":
            self.inv.render_clip(aa=self.aa, aa_threshold=THRESHOLD, **kw)
        elif what == "adaptive_inf":
            self.inv.render_clip(aa=self.aa, aa_threshold=float("inf"), **kw)
        elif what == "full_maps":
            self.inv.render_clip(aa=self.aa, shutter_mode="maps", **kw)
        elif what == "full_fused":
            self.inv.render_clip(aa=self.aa, shutter_mode="fused", **kw)
        else:
            self.inv.render_clip(**kw)


def measure_clip(name, args):
    import torch
    c = Case(name)
    sums, refined = {}, {}
    for what in RENDERS + RENDERS:          # warm-up: the modules are built, the temporaries allocated
        c.render(what)
        torch.cuda.synchronize()
        sums[what] = int(c.out.view(torch.int32).sum(dtype=torch.int64).item())
        if what.startswith("adaptive"):
            refined[what] = [int(v) for v in c.inv.clip_adaptive_refined()]
    assert sums["full_fused"] == sums["full_maps"], (name, "the two full paths wrote other bytes")
    if sum(refined["adaptive_inf"]) == 0:
        assert sums["adaptive_inf"] == sums["plain"], (name, "nothing refined, and not the plain clip's bytes")
    ms = {what: [] for what in RENDERS}
    for _ in range(args.rounds):
        for what in RENDERS:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            c.render(what)
            torch.cuda.synchronize()
            ms[what].append((time.perf_counter() - t0) * 1e3)
    pixels = c.w * c.h * c.n
    rec = {"filter": CASES[name][0], "width": c.w, "height": c.h, "frames": c.n, "grid": [c.aa, c.aa], "threshold": THRESHOLD, "plan": c.plan,
           "refined_share": sum(refined["adaptive"]) / pixels, "refined_share_at_inf": sum(refined["adaptive_inf"]) / pixels}
    for what in ms:
        rec[what] = summary(ms[what])
    med = {what: rec[what]["median_ms"] for what in ms}
    rec["largest_spread_ms"] = max(rec[what]["spread_ms"] for what in ms)
    rec["adaptive_over_full_maps"] = med["adaptive"] / med["full_maps"]
    rec["adaptive_over_full_fused"] = med["adaptive"] / med["full_fused"]
    rec["inf_minus_plain_ms"] = med["adaptive_inf"] - med["plain"]
    print(json.dumps({name: dict(med, refined_share=rec["refined_share"], adaptive_over_full_maps=rec["adaptive_over_full_maps"],
                                 adaptive_over_full_fused=rec["adaptive_over_full_fused"], inf_minus_plain_ms=rec["inf_minus_plain_ms"],
                                 largest_spread_ms=rec["largest_spread_ms"])}), flush=True)
    return rec


def measure_registers(which):
    from pair_loop_isa import assembly
    flt = load(which)
    if which.endswith("+"):
        flt = flt.specialized()
    rec = {}
    for variant, kernel, text in (("refine", "mm_pixels_refine", flt.refine_kernel_source), ("sampled", "mm_pixels_sampled", flt.sampled_kernel_source)):
        rec[variant] = dict(kernel_resources(assembly(text), kernel), kernel=kernel)
    print(json.dumps({which: rec}), flush=True)
    return rec


def mask_kernel_registers():
    """Every instance of k_aa_contrast_clip in the assembly of clip_combine.hip, compiled as the library compiles it."""
    from pair_loop_isa import hipcc
    csrc = os.path.join(ROOT, "mathmap_amd", "csrc")
    with tempfile.TemporaryDirectory() as d:
        asm = os.path.join(d, "clip_combine.s")
        cmd = [hipcc(), "-std=c++17", "-O2", "-I", csrc, "-I", os.path.join(ROOT, "include"), "--offload-arch=gfx950", "-ffp-contract=off",
               "--cuda-device-only", "-S", "-o", asm, os.path.join(csrc, "clip_combine.hip")]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            sys.exit("compilation failed:\n" + r.stderr[-4000:])
        with open(asm) as f:
            text = f.read()
    meta = text[text.index("amdhsa.kernels:"):]
    modes = {0: "floatmap", 1: "bytes1", 2: "bytes2", 3: "bytes3", 4: "bytes4", 5: "words"}
    rec = {}
    for entry in meta.split("\n  - ")[1:]:
        m = re.search(r"\.name:\s+(\S*k_aa_contrast_clip\S*)\s*$", entry, re.M)
        if not m:
            continue
        inst = re.search(r"ILi(\d)ELb([01])E", m.group(1))
        label = "%s%s" % (modes[int(inst.group(1))], "_list" if inst.group(2) == "1" else "")
        rec[label] = {field: int(re.search(r"\.%s:\s+(\d+)" % field, entry).group(1))
                      for field in ("vgpr_count", "sgpr_count", "agpr_count", "private_segment_fixed_size", "group_segment_fixed_size")}
    assert len(rec) == 12, sorted(rec)
    print(json.dumps({"k_aa_contrast_clip": rec}), flush=True)
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
        part["taken"] = "without a GPU, from the gfx950 assembly of the generated texts under the JIT's options and of clip_combine.hip under the library's"
        part.setdefault("filters", {})
        for which in (args.cases.split(",") if args.cases else FILTERS):
            part["filters"][which.rstrip("+")] = measure_registers(which)
            save()
        part["k_aa_contrast_clip"] = mask_kernel_registers()
        save()
        return 0
    import torch
    part = record.setdefault("adaptive_against_full_and_plain", {})
    part.update({"device": torch.cuda.get_device_name(0), "rounds": args.rounds, "order": ", ".join(RENDERS) + ", ...",
                 "timing": "host clock between two stream synchronisations around one render_clip call of the N frames into RGBA8, "
                           "all five renders into the same out_ptr"})
    part.setdefault("cases", {})
    for name in (args.cases.split(",") if args.cases else list(CASES)):
        part["cases"][name] = measure_clip(name, args)
        save()
    return 0


if __name__ == "__main__":
    sys.exit(main())
