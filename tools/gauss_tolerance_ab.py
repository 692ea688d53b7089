"""A/B of gaussian_blur's exact and tolerance chains (mmhip_options.gauss_mode) in one process.

For each shape it alternates the two filters for --rounds rounds, each round timing --frames frames in the bench's loop
shape (a new input generation by set_image_device, then render_rows over the whole frame into RGBA8), and reports the
region time per frame from device events, the per-kernel times of one extra frame from mmhip_drain_native_kernel_ms,
the spread across rounds, and the byte contract between the two chains' last timed frames (no channel apart by more than
1; the share of bytes that differ).  Writes the record as JSON (--out), stamped with --commit.

    python tools/gauss_tolerance_ab.py --out profiles/r04_ab_gauss_tolerance.json --commit <sha>
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [(16384, 20.0, 5), (2048, 3.0, 60), (2048, 20.0, 60), (1024, 20.0, 100)]     # (size, sigma px, frames per round)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--commit", default="unknown")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--sizes", default="", help="comma-separated subset of the shapes' sizes")
    args = ap.parse_args()
    import numpy as np
    import torch
    import mathmap_amd as mm
    from tests import filters as F

    stream = torch.cuda.current_stream().cuda_stream
    keep = {int(s) for s in args.sizes.split(",") if s}
    record = {"commit": args.commit, "device": torch.cuda.get_device_name(0), "rounds": args.rounds, "shapes": []}
    for size, sigma, frames in SHAPES:
        if keep and size not in keep:
            continue
        g = torch.Generator(device="cuda").manual_seed(size)
        img = torch.randint(0, 256, (size, size, 4), dtype=torch.uint8, device="cuda", generator=g)
        img[..., 0] = 255                                          # alpha: the low byte of 0xRRGGBBAA
        img32 = img.view(torch.int32)
        dev = float(np.float32(sigma / ((size - 1) / 2.0)))
        runs = {}
        for mode in ("exact", "tolerance"):
            inv = F.load("gauss_direct", gauss_mode=mode).invoke(size, size)
            inv.set("hdev", dev)
            inv.set("vdev", dev)
            out = torch.empty((size, size, 4), dtype=torch.uint8, device="cuda")
            runs[mode] = {"inv": inv, "out": out, "ms": []}

        def frame(r):
            r["inv"].set_image_device("in", img32.data_ptr(), size, size)
            r["inv"].render_rows(r["out"].data_ptr(), 0, size, stream=stream)

        for r in runs.values():                                    # warm-up: code objects, workspace
            frame(r)
            frame(r)
        torch.cuda.synchronize()
        for _ in range(args.rounds):
            for mode, r in runs.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(frames):
                    frame(r)
                e1.record()
                torch.cuda.synchronize()
                r["ms"].append(e0.elapsed_time(e1) / frames)
        a, b = runs["exact"]["out"], runs["tolerance"]["out"]
        d = (a.to(torch.int16) - b.to(torch.int16)).abs()
        contract = {"max_abs": int(d.max()), "n_diff": int((d > 0).sum()), "n_gt1": int((d > 1).sum()), "n_values": d.numel()}
        del d
        kernels = {}
        for mode, r in runs.items():
            r["inv"].enable_timing(True)
            launches = r["inv"].tolerance_blur_launches()
            frame(r)
            torch.cuda.synchronize()
            kernels[mode] = r["inv"].drain_native_kernel_ms()
            r["inv"].enable_timing(False)
            assert r["inv"].tolerance_blur_launches() - launches == (1 if mode == "tolerance" else 0), mode
        shape = {"size": size, "sigma_px": sigma, "frames_per_round": frames, "byte_contract_exact_vs_tolerance": contract}
        for mode, r in runs.items():
            ms = r["ms"]
            shape[mode] = {"region_ms_per_frame": ms, "median_ms": float(np.median(ms)),
                           "spread_pct": 100.0 * (max(ms) - min(ms)) / float(np.median(ms)),
                           "kernels_ms": [[n, round(t, 4)] for n, t in kernels[mode]],
                           "kernel_sum_ms": round(sum(t for _, t in kernels[mode]), 4)}
        shape["speedup_region"] = shape["exact"]["median_ms"] / shape["tolerance"]["median_ms"]
        record["shapes"].append(shape)
        print(json.dumps({k: v for k, v in shape.items()}), flush=True)
        del runs, img, img32
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(record, f, indent=1)
    ok = all(s["byte_contract_exact_vs_tolerance"]["n_gt1"] == 0 for s in record["shapes"])
    print("byte contract %s" % ("holds" if ok else "BROKEN"))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
