"""What left-sited chroma costs in the four 4:2:0 converters, and whether the centre-sited kernels are what they were.

Clips of 1920x1080 x 60 frames and 3840x2160 x 15 frames of random content, kernel time by device events through
mmhip_drain_native_kernel_ms, medians of --rounds rounds with max - min beside them:
  --part sited   each of the four kernels (RGBA8 -> 8 bit, float4 -> 10 bit, 8 bit -> words, 10 bit -> float4; the input
                 kernels in bilinear mode, everything on its aligned path with the defaults of its knobs), centre against
                 left siting, in one process after a warm-up, the legs alternating.  Each row carries its traffic set against
                 the achievable HBM rate, as the tables of the four converters compute it.
  --part parent  the centre and the left legs of this build against the same kernels of a build of the parent commit
                 (--parent DIR, a checkout built in place): one child process per side and round -- parent, new, parent,
                 new, ... -- each taking the median of --rounds launches after a warm-up.  A new median counts as within the
                 band where it lies within the parent's median +- the larger of the two sides' spreads.  --centre-only
                 times the centre legs alone, through the entry points without a siting: for a parent that has no others.
  --part ab      bench.py's default line, parent and this build alternating, --runs runs each (tools/sequence_cost.py's A/B).

    python tools/clip_yuv_siting_cost.py --part sited --out profiles/r25_clip_yuv_siting_cost.json --commit <sha>
    python tools/clip_yuv_siting_cost.py --part parent --parent <dir> --out profiles/r25_clip_yuv_siting_cost.json
    python tools/clip_yuv_siting_cost.py --part ab --parent <dir> --out profiles/r25_clip_yuv_siting_cost.json
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
from statistics import median

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

HBM_RATE = 6.29e12          # bytes/s: the achievable streaming rate of DESIGN section 3
CLIPS = {"1080p_60": (1920, 1080, 60), "2160p_15": (3840, 2160, 15)}
# kernel -> the label it is timed as, bytes read and written per pixel
KERNELS = {"rgba8_to_yuv420": ("yuv420_clip", 4, 1.5), "float_to_yuv420p10": ("yuv420p10_clip", 16, 3),
           "yuv420_to_rgba": ("yuv420_to_rgba_clip", 1.5, 4), "yuv420p10_to_float": ("yuv420p10_to_float_clip", 3, 16)}
SITINGS = ("center", "left")
IDENTITY = "filter identity (image in) in(xy, frame) end"


def summary(values):
    return {"ms": values, "median_ms": median(values), "spread_ms": max(values) - min(values)}


class Clip:
    """One clip's buffers in HBM and the four conversions over them.  `sited` False calls the entry points without the
    chroma_siting keyword: what a build of the parent commit has."""

    def __init__(self, name, sited):
        import numpy as np
        import mathmap_amd as mm
        from mathmap_amd._lib import lib
        self.lib, self.sited = lib(), sited
        w, h, n = self.size = CLIPS[name]
        samples = w * h + 2 * ((w + 1) >> 1) * ((h + 1) >> 1)
        self.inv = mm.Filter(IDENTITY, deep_inputs=True).invoke(w, h)
        rng = np.random.default_rng(1)
        # (one frame of random content repeated: the kernels read every frame from its own place in HBM all the same)
        host = {"rgba": np.tile(rng.integers(0, 256, w * h * 4, dtype=np.uint8), n),
                "floats": np.tile(rng.random(w * h * 4, dtype=np.float32), n),
                "yuv8": np.tile(rng.integers(0, 256, samples, dtype=np.uint8), n),
                "yuv10": np.tile(rng.integers(0, 1024, samples).astype(np.uint16), n)}
        self.dev = {}
        for key, array in host.items():
            self.dev[key] = self.alloc(array.nbytes)
            assert self.lib.mmhip_copy_to_device(C.c_void_p(self.dev[key]), array.ctypes.data_as(C.c_void_p), array.nbytes) == 0
        self.dev["out"] = self.alloc(n * w * h * 16)

    def alloc(self, size):
        p = self.lib.mmhip_device_alloc(size)
        assert p, "out of device memory"
        return p

    def run(self, kernel, siting):
        n = self.size[2]
        keywords = dict(chroma_siting=siting) if self.sited else {}
        assert self.sited or siting == "center"
        if kernel == "rgba8_to_yuv420":
            self.inv.clip_to_yuv420(self.dev["rgba"], self.dev["out"], n, **keywords)
        elif kernel == "float_to_yuv420p10":
            self.inv.clip_float_to_yuv420p10(self.dev["floats"], self.dev["out"], n, **keywords)
        elif kernel == "yuv420_to_rgba":
            self.inv.clip_from_yuv420(self.dev["yuv8"], self.dev["out"], n, chroma="bilinear", **keywords)
        else:
            self.inv.clip_from_yuv420p10(self.dev["yuv10"], self.dev["out"], n, chroma="bilinear", **keywords)
        self.inv.sync()

    def measure(self, legs, rounds):
        """ms per leg (kernel, siting): `rounds` values, the legs alternating, after two warm-up passes."""
        for leg in legs * 2:
            self.run(*leg)
        self.inv.enable_timing(True)
        self.inv.drain_native_kernel_ms()
        ms = {leg: [] for leg in legs}
        for _ in range(rounds):
            for leg in legs:
                self.run(*leg)
                ms[leg].append(sum(t for label, t in self.inv.drain_native_kernel_ms() if label == KERNELS[leg[0]][0]))
        self.inv.enable_timing(False)
        return ms

    def free(self):
        self.inv.sync()
        for p in self.dev.values():
            self.lib.mmhip_device_free(C.c_void_p(p))


def at_the_hbm_rate_ms(name, kernel):
    w, h, n = CLIPS[name]
    _, read, written = KERNELS[kernel]
    return n * w * h * (read + written) / HBM_RATE * 1e3


def part_sited(args, record):
    sys.path.insert(0, ROOT)
    record.setdefault("sited", {})
    for name in args.clips.split(","):
        clip = Clip(name, True)
        try:
            ms = clip.measure([(kernel, siting) for kernel in KERNELS for siting in SITINGS], args.rounds)
        finally:
            clip.free()
        rec = {"size": CLIPS[name], "kernels": {}}
        for kernel in KERNELS:
            floor = at_the_hbm_rate_ms(name, kernel)
            row = {"bytes_per_pixel": KERNELS[kernel][1] + KERNELS[kernel][2], "at_the_hbm_rate_ms": floor}
            for siting in SITINGS:
                row[siting] = summary(ms[kernel, siting])
                row[siting]["share_of_the_hbm_rate"] = floor / row[siting]["median_ms"]
            row["left_over_center"] = row["left"]["median_ms"] / row["center"]["median_ms"]
            rec["kernels"][kernel] = row
            print(json.dumps({name: {kernel: {s: (round(row[s]["median_ms"], 4), round(row[s]["spread_ms"], 4), round(row[s]["share_of_the_hbm_rate"], 3))
                                              for s in SITINGS}, "left_over_center": round(row["left_over_center"], 4)}}), flush=True)
        record["sited"][name] = rec
        yield record


def child(args):
    """One side of --part parent: the legs of every kernel in the tree --tree."""
    sys.path.insert(0, os.path.abspath(args.tree))
    sitings = SITINGS[:1] if args.centre_only else SITINGS
    out = {}
    for name in args.clips.split(","):
        clip = Clip(name, not args.centre_only)
        try:
            ms = clip.measure([(kernel, siting) for kernel in KERNELS for siting in sitings], args.rounds)
        finally:
            clip.free()
        out[name] = {kernel: {siting: median(ms[kernel, siting]) for siting in sitings} for kernel in KERNELS}
    print(json.dumps(out), flush=True)
    return 0


def part_parent(args, record):
    trees = (("parent", os.path.abspath(args.parent)), ("new", ROOT))
    sitings = SITINGS[:1] if args.centre_only else SITINGS
    series = {side: {name: {(kernel, siting): [] for kernel in KERNELS for siting in sitings} for name in args.clips.split(",")} for side, _ in trees}
    for _ in range(args.rounds):
        for side, tree in trees:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--tree", tree, "--clips", args.clips, "--rounds", str(args.rounds),
                                "--out", os.devnull] + (["--centre-only"] if args.centre_only else []), cwd=tree, stdout=subprocess.PIPE,
                               stderr=subprocess.PIPE, text=True, timeout=420)
            if p.returncode != 0:
                raise RuntimeError("the %s side failed: %s" % (side, p.stderr[-600:]))
            got = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])
            for name in got:
                for kernel, legs in got[name].items():
                    for siting, ms in legs.items():
                        series[side][name][kernel, siting].append(ms)
    rec = {"order": "parent, new, parent, new, ...: one process per side and round, each value the median of %d launches" % args.rounds, "clips": {}}
    for name in args.clips.split(","):
        rec["clips"][name] = {}
        for kernel, siting in series["new"][name]:
            row = {side: summary(series[side][name][kernel, siting]) for side, _ in trees}
            row["new_over_parent"] = row["new"]["median_ms"] / row["parent"]["median_ms"]
            band = max(row["parent"]["spread_ms"], row["new"]["spread_ms"])
            row["within_the_band"] = abs(row["new"]["median_ms"] - row["parent"]["median_ms"]) <= band
            rec["clips"][name].setdefault(kernel, {})[siting] = row
            print(json.dumps({name: {kernel: {siting: {"parent": round(row["parent"]["median_ms"], 4), "parent_spread": round(row["parent"]["spread_ms"], 4),
                                                       "new": round(row["new"]["median_ms"], 4), "new_spread": round(row["new"]["spread_ms"], 4),
                                                       "within_the_band": row["within_the_band"]}}}}), flush=True)
    record["against_parent"] = rec
    yield record


def part_ab(args, record):
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from sequence_cost import part_ab as bench_ab
    args.workloads = "mandelbrot"
    rec = record.setdefault("bench_default", {})
    for _ in bench_ab(args, rec):
        yield record


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=("sited", "parent", "ab"), default="sited")
    ap.add_argument("--out", required=True)
    ap.add_argument("--commit", default="unknown")
    ap.add_argument("--clips", default=",".join(CLIPS))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit (--part parent, --part ab)")
    ap.add_argument("--runs", type=int, default=5, help="bench.py runs per side (--part ab)")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--centre-only", action="store_true", help="--part parent: the centre legs alone, without a siting keyword")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--tree", default=ROOT, help=argparse.SUPPRESS)
    args = ap.parse_args()
    assert args.rounds >= 5, "at least 5 rounds"
    if args.child:
        return child(args)
    if args.part in ("parent", "ab") and not args.parent:
        ap.error("--part %s needs --parent" % args.part)
    record = {}
    if os.path.exists(args.out):
        with open(args.out) as f:
            record = json.load(f)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    record.update({"commit": args.commit if args.commit != "unknown" else record.get("commit", "unknown"), "rounds": args.rounds,
                   "hbm_rate_bytes_per_s": HBM_RATE,
                   "timing": "device events around the launch (mmhip_drain_native_kernel_ms), every leg once per round after two warm-up passes"})
    for _ in {"sited": part_sited, "parent": part_parent, "ab": part_ab}[args.part](args, record):
        with open(args.out, "w") as f:
            json.dump(record, f, indent=1)
            f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
