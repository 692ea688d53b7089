"""What delivering a clip to the host as planar Y'CbCr 4:2:0 costs against delivering it as RGBA8.

Clips of the specialised Mandelbrot and of Pond at 1920x1080 x 120 frames and at 8192^2 x 8 frames.  Per case, in one
process after a warm-up, two legs alternate for --rounds rounds, each timed by the host clock between two device
synchronisations:
  rgba    the parent's path: render_clip into an RGBA8 out_ptr, then the device-to-host copy of 4 bytes per pixel
  yuv     render_clip(pixel_format="yuv420p") into an out_ptr, then the device-to-host copy of 1.5 bytes per pixel
Both copy into pinned host memory.  Then, with mmhip_enable_timing, the conversion alone (clip_to_yuv420 on the frames the
rgba leg left in HBM) is read through mmhip_drain_native_kernel_ms, alternating MMHIP_YUV_LOADS=nt and =cached: its
traffic is 5.5 bytes per pixel (4 read, 1.5 written), set against the streaming ceiling.  With --cli, `-F 120` of the
Mandelbrot at 1080p through the command line, to PNG files and to one .y4m file, alternating, by the host clock.

    python tools/clip_yuv_cost.py --out profiles/r18_clip_yuv_cost.json --commit <sha> --cli
"""
import argparse
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from shutter_fused_cost import SIZES, STREAM_CEILING, load, summary      # noqa: E402

FRAMES = {"1080": 120, "8192": 8}
FILTERS = ("mandelbrot+", "pond")                           # +: compiled with specialize=True
CASES = {"%s_%s" % (f.rstrip("+"), s): (f, s) for f in FILTERS for s in SIZES}
LOADS = ("nt", "cached")
CLI = os.path.join(ROOT, "mathmap_amd", "mathmap_hip_cli")


class Case:
    def __init__(self, name):
        import torch
        from mathmap_amd.api import yuv420_frame_bytes
        from tests import filters as F
        which, size = CASES[name]
        self.w, self.h = SIZES[size]
        self.n = FRAMES[size]
        self.flt = load(which)
        self.inv = self.flt.invoke(self.w, self.h)
        if F.image_names(self.flt):
            g = torch.Generator(device="cuda").manual_seed(7)
            self.image = torch.randint(-2 ** 31, 2 ** 31 - 1, (self.h, self.w), dtype=torch.int32, device="cuda", generator=g)
            self.inv.set_image_device("in", self.image.data_ptr(), self.w, self.h, keepalive=self.image)
        self.frame_bytes = yuv420_frame_bytes(self.w, self.h)
        self.rgba = torch.empty((self.n, self.h, self.w, 4), dtype=torch.uint8, device="cuda")
        self.yuv = torch.empty((self.n, self.frame_bytes), dtype=torch.uint8, device="cuda")
        self.host_rgba = torch.empty(self.rgba.shape, dtype=torch.uint8, pin_memory=True)
        self.host_yuv = torch.empty(self.yuv.shape, dtype=torch.uint8, pin_memory=True)
        self.stream = torch.cuda.current_stream().cuda_stream

    def leg(self, which):
        if which == "rgba":
            self.inv.render_clip(num_frames=self.n, out_ptr=self.rgba.data_ptr(), stream=self.stream)
            self.inv.sync()
            self.host_rgba.copy_(self.rgba, non_blocking=True)
        else:
            self.inv.render_clip(num_frames=self.n, out_ptr=self.yuv.data_ptr(), stream=self.stream, pixel_format="yuv420p")
            self.inv.sync()
            self.host_yuv.copy_(self.yuv, non_blocking=True)

    def convert(self):
        self.inv.clip_to_yuv420(self.rgba.data_ptr(), self.yuv.data_ptr(), self.n, stream=self.stream)


def measure(name, args):
    import torch
    c = Case(name)
    legs = ("rgba", "yuv")
    for which in legs * 2:                 # warm-up: the modules are built, the copies' paths set up
        c.leg(which)
        torch.cuda.synchronize()
    ms = {which: [] for which in legs}
    for _ in range(args.rounds):
        for which in legs:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            c.leg(which)
            torch.cuda.synchronize()
            ms[which].append((time.perf_counter() - t0) * 1e3)
    # the restatement's bytes of frame 0, as a check that the legs deliver the same clip
    from tests import yuv_reference as X
    same = bool((X.frame(c.host_rgba[0].numpy(), ("bt709", "limited")) == c.host_yuv[0].numpy()).all())
    # the conversion alone, on the frames the rgba leg left in HBM
    c.inv.enable_timing(True)
    convert = {loads: [] for loads in LOADS}
    for loads in LOADS * 2:
        os.environ["MMHIP_YUV_LOADS"] = loads
        c.convert()
        torch.cuda.synchronize()
    c.inv.drain_native_kernel_ms()
    for _ in range(args.rounds):
        for loads in LOADS:
            os.environ["MMHIP_YUV_LOADS"] = loads
            c.convert()
            torch.cuda.synchronize()
            convert[loads].append(sum(t for label, t in c.inv.drain_native_kernel_ms() if label == "yuv420_clip"))
    del os.environ["MMHIP_YUV_LOADS"]
    c.inv.enable_timing(False)
    pixels = c.w * c.h * c.n
    traffic = 4 * pixels + c.frame_bytes * c.n
    rec = {"filter": CASES[name][0], "width": c.w, "height": c.h, "frames": c.n, "frame0_equals_the_restatement": same,
           "rgba_bytes_to_host": 4 * pixels, "yuv_bytes_to_host": c.frame_bytes * c.n,
           "conversion_bytes": traffic, "conversion_at_the_ceiling_ms": traffic / STREAM_CEILING * 1e3}
    for which in legs:
        rec[which] = summary(ms[which])
    for loads in LOADS:
        rec["conversion_" + loads] = summary(convert[loads])
    rec["yuv_over_rgba"] = rec["yuv"]["median_ms"] / rec["rgba"]["median_ms"]
    rec["conversion_over_ceiling"] = rec["conversion_nt"]["median_ms"] / rec["conversion_at_the_ceiling_ms"]
    rec["conversion_cached_over_nt"] = rec["conversion_cached"]["median_ms"] / rec["conversion_nt"]["median_ms"]
    print(json.dumps({name: {"rgba_ms": rec["rgba"]["median_ms"], "yuv_ms": rec["yuv"]["median_ms"], "yuv_over_rgba": rec["yuv_over_rgba"],
                             "conversion_nt_ms": rec["conversion_nt"]["median_ms"], "conversion_cached_ms": rec["conversion_cached"]["median_ms"],
                             "ceiling_ms": rec["conversion_at_the_ceiling_ms"], "same": same}}), flush=True)
    return rec


def measure_cli(args):
    """-F 120 of the Mandelbrot at 1920 x 1080 through the command line: 120 PNG files against one .y4m file."""
    flt = load("mandelbrot")
    d = tempfile.mkdtemp(prefix="mm_yuv_cli_")
    try:
        script = os.path.join(d, "mandelbrot.json")
        with open(script, "w") as f:
            f.write(flt.ir_json_raw)
        targets = {"png": os.path.join(d, "f%03d.png"), "y4m": os.path.join(d, "clip.y4m")}
        ms = {kind: [] for kind in targets}
        for _ in range(args.cli_rounds):
            for kind, target in targets.items():
                t0 = time.perf_counter()
                subprocess.run([CLI, "-F", "120", "-s", "1920x1080", "--batch-frames=120", "-f", script, target], check=True, timeout=900)
                ms[kind].append((time.perf_counter() - t0) * 1e3)
        rec = {"command": "mathmap_hip_cli -F 120 -s 1920x1080 --batch-frames=120 -f mandelbrot.json <outfile>", "rounds": args.cli_rounds,
               "timing": "host clock around the whole process, JIT and file writes into a temporary directory included, png and y4m alternating",
               "y4m_file_bytes": os.path.getsize(targets["y4m"]),
               "png_files_bytes": sum(os.path.getsize(os.path.join(d, n)) for n in os.listdir(d) if n.endswith(".png"))}
        for kind in targets:
            rec[kind] = summary(ms[kind])
        rec["y4m_over_png"] = rec["y4m"]["median_ms"] / rec["png"]["median_ms"]
        print(json.dumps({"cli": {"png_ms": rec["png"]["median_ms"], "y4m_ms": rec["y4m"]["median_ms"]}}), flush=True)
        return rec
    finally:
        shutil.rmtree(d, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--commit", default="unknown")
    ap.add_argument("--cases", default=None, help="a subset (the record keeps the others)")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--cli", action="store_true", help="also the command line end to end")
    ap.add_argument("--cli-rounds", type=int, default=2)
    args = ap.parse_args()
    record = {}
    if os.path.exists(args.out):
        with open(args.out) as f:
            record = json.load(f)
    record["commit"] = args.commit
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    import torch
    record.update({"device": torch.cuda.get_device_name(0), "rounds": args.rounds, "order": "rgba, yuv, rgba, yuv, ...; then nt, cached, nt, cached, ...",
                   "streaming_ceiling_bytes_per_s": STREAM_CEILING,
                   "timing": "host clock between two device synchronisations around one render_clip call of the whole clip into device memory "
                             "and the copy of its result into pinned host memory; the conversion from device events around its launch "
                             "(mmhip_drain_native_kernel_ms, label yuv420_clip), MMHIP_YUV_LOADS alternating"})
    record.setdefault("cases", {})

    def save():
        with open(args.out, "w") as f:
            json.dump(record, f, indent=1)
            f.write("\n")
    for name in (args.cases.split(",") if args.cases else list(CASES)):
        record["cases"][name] = measure(name, args)
        save()
    if args.cli:
        record["cli_1080p_mandelbrot"] = measure_cli(args)
        save()
    return 0


if __name__ == "__main__":
    sys.exit(main())
