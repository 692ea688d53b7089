"""What multi-frame input drawables cost: the existing workloads against the parent commit, and the new fetch paths.

Two parts, each merged into the record at --out (stamped with --commit and the kernel texts' hashes):

  --part ab   bench.py (default workload, ident, droste, pond) of a build of the parent commit (--parent DIR, a checkout
              of it built in place) and of this tree, alternating, --runs runs per side, one process per run.  The lean
              line is timed (--no-cpu-baseline --no-configs --no-generic: the timed region is the same --steps frames).
              Per workload: both series, medians, the parent's max - min spread, and whether the new median is below the
              parent's by more than that spread.
  --part new  8192^2, K = 8, bilinear, in one process, the variants alternating for --rounds rounds of --frames frames
              between device events: in(xy) on a single image, in(xy, frame) on the sequence, the slit-scan
              in(xy, 4 + 4 * x) with the per-pixel hot fetch and with MMHIP_FRAME_HOT=0 (the early-exit fetch), and Ident.
              ms per frame, Mpixels/s and the HBM fraction as bench.py computes it (8 algorithmic bytes per pixel over
              HBM_PEAK_GBS).

    python tools/sequence_cost.py --part ab --parent <dir> --out profiles/r06_sequence_cost.json --commit <sha>
    python tools/sequence_cost.py --part new --out profiles/r06_sequence_cost.json --commit <sha>
"""
import argparse
import hashlib
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WORKLOADS = ("mandelbrot", "ident", "droste", "pond")        # mandelbrot is bench.py's default
SIZE, K = 8192, 8
PLAIN = "filter seq_cost_plain (image in)\n  in(xy)\nend\n"
BY_FRAME = "filter seq_cost_frame (image in)\n  in(xy, frame)\nend\n"
SLIT = "filter seq_cost_slit (image in)\n  in(xy, 4 + 4 * x)\nend\n"


def median(v):
    s = sorted(v)
    return s[len(s) // 2] if len(s) % 2 else 0.5 * (s[len(s) // 2 - 1] + s[len(s) // 2])


def bench_once(tree, workload, steps, warmup):
    cmd = [sys.executable, os.path.join(tree, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup),
           "--no-cpu-baseline", "--no-configs", "--no-generic"]
    if workload != "mandelbrot":
        cmd += ["--workload", workload]
    p = subprocess.run(cmd, cwd=tree, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=420)
    if p.returncode != 0:
        raise RuntimeError("bench.py failed in %s (%s): %s" % (tree, workload, p.stderr[-600:]))
    line = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])
    return {"mpix_s": line["value"], "ms_per_step": line["ms_per_step"], "kernel_ms": line["per_rank_kernel_ms"][0]}


def part_ab(args, out):
    out.update({"runs_per_side": args.runs, "steps": args.steps, "warmup": args.warmup, "order": "parent, new, parent, new, ...",
           "bench_flags": "--gpus 1 --no-cpu-baseline --no-configs --no-generic"})
    out.setdefault("workloads", {})
    for wl in args.workloads.split(","):
        series = {"parent": [], "new": []}
        for _ in range(args.runs):
            for side, tree in (("parent", os.path.abspath(args.parent)), ("new", ROOT)):
                series[side].append(bench_once(tree, wl, args.steps, args.warmup))
        rec = {}
        for side in series:
            v = [r["mpix_s"] for r in series[side]]
            rec[side] = {"mpix_s": v, "kernel_ms": [r["kernel_ms"] for r in series[side]], "median_mpix_s": median(v),
                         "median_kernel_ms": median([r["kernel_ms"] for r in series[side]]), "spread_mpix_s": max(v) - min(v)}
        rec["new_over_parent"] = rec["new"]["median_mpix_s"] / rec["parent"]["median_mpix_s"]
        rec["within_parent_spread"] = rec["new"]["median_mpix_s"] >= rec["parent"]["median_mpix_s"] - rec["parent"]["spread_mpix_s"]
        out["workloads"][wl] = rec
        print(json.dumps({wl: {k: rec[k] for k in ("new_over_parent", "within_parent_spread")},
                          "parent": rec["parent"]["mpix_s"], "new": rec["new"]["mpix_s"]}), flush=True)
        yield out


def part_new(args):
    import torch
    import mathmap_amd as mm
    from bench import ALGO_BYTES_PER_PIXEL, HBM_PEAK_GBS
    from tests import filters as F

    stream = torch.cuda.current_stream().cuda_stream
    g = torch.Generator(device="cuda").manual_seed(6)
    seq = torch.randint(-2 ** 31, 2 ** 31 - 1, (K, SIZE, SIZE), dtype=torch.int32, device="cuda", generator=g)
    out = torch.empty((SIZE, SIZE, 4), dtype=torch.uint8, device="cuda")

    def variant(flt, frames, frame=0):
        inv = flt.invoke(SIZE, SIZE)
        inv.set_image_device("in", seq.data_ptr(), SIZE, SIZE, keepalive=seq, num_frames=frames)
        return {"inv": inv, "frame": frame, "ms": [], "kernel_sha256": hashlib.sha256(flt.kernel_source.encode()).hexdigest(),
                "geometry": flt.launch_geometry(SIZE, SIZE)}

    runs = {"plain_single_image": variant(mm.Filter(PLAIN), 1), "by_frame_sequence": variant(mm.Filter(BY_FRAME), K, frame=5),
            "slit_hot": variant(mm.Filter(SLIT), K), "ident_single_image": variant(F.load("ident"), 1)}
    os.environ["MMHIP_FRAME_HOT"] = "0"          # read when the kernel text is generated
    runs["slit_early_exit"] = variant(mm.Filter(SLIT), K)
    del os.environ["MMHIP_FRAME_HOT"]
    assert "hotf(" in mm.Filter(SLIT).kernel_source.split(" mm_pixels(mm_args A")[1]
    assert runs["slit_hot"]["kernel_sha256"] != runs["slit_early_exit"]["kernel_sha256"]

    def render(r):
        r["inv"].render_rows(out.data_ptr(), 0, SIZE, t=0.0, frame=r["frame"], stream=stream)

    for r in runs.values():
        for _ in range(3):
            render(r)
    torch.cuda.synchronize()
    # the two slit-scan kernels compute the same bytes
    render(runs["slit_hot"])
    a = out.clone()
    render(runs["slit_early_exit"])
    torch.cuda.synchronize()
    same = bool(torch.equal(a, out))
    del a
    for _ in range(args.rounds):
        for r in runs.values():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.frames):
                render(r)
            e1.record()
            torch.cuda.synchronize()
            r["ms"].append(e0.elapsed_time(e1) / args.frames)
    bpp = ALGO_BYTES_PER_PIXEL["ident"]
    rec = {"size": SIZE, "num_frames": K, "fetch": "bilinear", "rounds": args.rounds, "frames_per_round": args.frames,
           "device": torch.cuda.get_device_name(0), "slit_hot_equals_slit_early_exit": same,
           "timing": "device events around frames_per_round whole-frame render_rows calls (prologue + pixel kernel), per frame",
           "variants": {}}
    for name, r in runs.items():
        ms = median(r["ms"])
        rec["variants"][name] = {"ms_per_frame": r["ms"], "median_ms": ms, "spread_ms": max(r["ms"]) - min(r["ms"]),
                                 "mpix_s": SIZE * SIZE / (ms * 1e-3) / 1e6,
                                 "hbm_frac": SIZE * SIZE * bpp / (ms * 1e-3) / 1e9 / HBM_PEAK_GBS,
                                 "algorithmic_bytes_per_pixel": bpp, "kernel_sha256": r["kernel_sha256"],
                                 "unroll": r["geometry"]["unroll"], "ppt": r["geometry"]["ppt"], "tile_w": r["geometry"]["tile_w"]}
        print(json.dumps({name: rec["variants"][name]["median_ms"], "spread": rec["variants"][name]["spread_ms"]}), flush=True)
    v = rec["variants"]
    rec["ratios"] = {"by_frame_over_plain": v["by_frame_sequence"]["median_ms"] / v["plain_single_image"]["median_ms"],
                     "slit_hot_over_early_exit": v["slit_hot"]["median_ms"] / v["slit_early_exit"]["median_ms"],
                     "slit_hot_over_ident": v["slit_hot"]["median_ms"] / v["ident_single_image"]["median_ms"]}
    print(json.dumps(rec["ratios"]), flush=True)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", required=True, choices=["ab", "new"])
    ap.add_argument("--out", required=True)
    ap.add_argument("--commit", default="unknown")
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit (--part ab)")
    ap.add_argument("--workloads", default=",".join(WORKLOADS), help="--part ab: a subset (the record keeps the others)")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--steps", type=int, default=240)
    ap.add_argument("--warmup", type=int, default=24)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--frames", type=int, default=200)
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
    if args.part == "ab":
        for done in part_ab(args, record.get("existing_workloads", {})):       # saved after every workload
            record["existing_workloads"] = done
            save()
    else:
        record["new_paths"] = part_new(args)
        save()
    return 0


if __name__ == "__main__":
    sys.exit(main())
