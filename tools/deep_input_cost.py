"""What a float32 input drawable costs against an 8-bit one (mmhip_options.deep_inputs, include/mmhip.h).

  clip       Ident (in(xy, frame)) and Pond at 1920x1080 x 120, each rendered by render_clip into device memory from
             a sequence of 120 frames of the frame's own size in three legs:
               rgba8        the 8-bit sequence, filter compiled without the option (the hot fetch);
               rgba8_opt    the same 8-bit sequence, filter compiled with deep_inputs (the hot fetch again: the option
                            only adds a branch to the generic fetch);
               deep         the float32 sequence of the same pixels (bytes / 255), filter compiled with deep_inputs
                            (the generic fetch, 16 bytes a texel against 4).
             One process, after a warm-up, the legs alternating, medians of --rounds rounds with the spreads; kernel
             time from the device events of the launches (mmhip_drain_kernel_ms), summed over the call's batches, and
             the host clock between two device synchronisations beside it.
  registers  no GPU needed: VGPRs, SGPRs, the private segment and the occupancy that follows from the VGPR count, for
             the clip kernels of the probe filters (tests/fetch_reference.py FETCH, FETCH_FRAME) and of Ident and Pond,
             compiled with the option on, nearest and bilinear.

    python tools/deep_input_cost.py --part clip --out profiles/r23_deep_input_cost.json --commit <sha>
    python tools/deep_input_cost.py --part registers --out profiles/r23_deep_input_cost.json
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from shutter_fused_cost import kernel_resources, summary      # noqa: E402

SIZE = (1920, 1080, 120)
IDENT = "filter ident_frames (image in)\n  in(xy, frame)\nend\n"
LEGS = ("rgba8", "rgba8_opt", "deep")


def filters(which, deep):
    import mathmap_amd as mm
    from tests import filters as F
    return mm.Filter(IDENT, deep_inputs=deep) if which == "ident" else F.load(which, deep_inputs=deep)


def measure_clip(which, args):
    import numpy as np
    import torch
    w, h, n = SIZE
    g = torch.Generator(device="cuda").manual_seed(7)
    rgba = torch.randint(0, 256, (n, h, w, 4), dtype=torch.uint8, device="cuda", generator=g)
    # 0xRRGGBBAA words of the same pixels, and bytes / 255 as the float drawable holds them
    b = rgba.to(torch.int32)
    words = ((b[..., 0] << 24) | (b[..., 1] << 16) | (b[..., 2] << 8) | b[..., 3]).contiguous()
    del b
    floats = (rgba.to(torch.float64) / 255.0).to(torch.float32).contiguous()
    out = torch.empty((n, h, w, 4), dtype=torch.uint8, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    invs = {}
    for leg in LEGS:
        inv = filters(which, leg != "rgba8").invoke(w, h)
        if leg == "deep":
            inv.set_image_device_float("in", floats.data_ptr(), w, h, num_frames=n, keepalive=floats)
        else:
            inv.set_image_device("in", words.data_ptr(), w, h, keepalive=words, num_frames=n)
        inv.enable_timing(True)
        invs[leg] = inv

    def render(leg):
        invs[leg].render_clip(num_frames=n, out_ptr=out.data_ptr(), stream=stream)
    sums = {}
    for leg in LEGS * 2:                  # warm-up: the modules are built, the launch buffers allocated
        render(leg)
        torch.cuda.synchronize()
        sums[leg] = int(out.view(torch.int32).sum(dtype=torch.int64).item())
        invs[leg].drain_kernel_ms()
    kernel, host = {leg: [] for leg in LEGS}, {leg: [] for leg in LEGS}
    for _ in range(args.rounds):
        for leg in LEGS:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            render(leg)
            torch.cuda.synchronize()
            host[leg].append((time.perf_counter() - t0) * 1e3)
            kernel[leg].append(float(np.sum(invs[leg].drain_kernel_ms())))
    pixels = w * h * n
    rec = {"filter": which, "width": w, "height": h, "frames": n, "intersample": True,
           "the_option_leaves_the_8_bit_bytes": sums["rgba8"] == sums["rgba8_opt"],
           "checksum_rgba8": sums["rgba8"], "checksum_deep": sums["deep"],
           "input_bytes": {"rgba8": 4 * pixels, "deep": 16 * pixels}, "output_bytes": 4 * pixels}
    for leg in LEGS:
        rec[leg] = {"kernel": summary(kernel[leg]), "host": summary(host[leg])}
    for leg in LEGS[1:]:
        rec[leg]["kernel_over_rgba8"] = rec[leg]["kernel"]["median_ms"] / rec["rgba8"]["kernel"]["median_ms"]
    print(json.dumps({which: {leg: [round(rec[leg]["kernel"]["median_ms"], 3), round(rec[leg]["kernel"]["spread_ms"], 3)] for leg in LEGS}}), flush=True)
    return rec


def occupancy(vgprs):
    """Waves per SIMD a kernel of 256 work-items reaches by its VGPR count alone (512 VGPRs per lane and SIMD, allocated
    in blocks of 8, at most 8 waves)."""
    return max(1, min(8, 512 // max(8, -(-vgprs // 8) * 8)))


def measure_registers():
    import mathmap_amd as mm
    from pair_loop_isa import assembly
    from tests import fetch_reference as R
    from tests import filters as F
    probes = {"fetch_default": R.FETCH["default"], "fetch_stretched": R.FETCH["stretched"], "fetch_frame": R.FETCH_FRAME.replace("{F}", R.FRAME_EXPR),
              "ident": IDENT, "pond": None}
    rec = {}
    for name, src in probes.items():
        for intersample in (True, False):
            for edge in ((0, 0), (3, 3)):
                opts = dict(intersample=intersample, edge_x=edge[0], edge_y=edge[1])
                row = {}
                for label, deep in (("plain", False), ("deep_inputs", True)):
                    flt = mm.Filter(src, deep_inputs=deep, **opts) if src else F.load(name, deep_inputs=deep, **opts)
                    res = kernel_resources(assembly(flt.clip_kernel_source), "mm_pixels_clip")
                    res["occupancy_waves_per_simd"] = occupancy(res["vgpr_count"])
                    row[label] = res
                rec["%s %s edge%d%d" % (name, "bilinear" if intersample else "nearest", edge[0], edge[1])] = row
                print(json.dumps({name: row, "intersample": intersample, "edge": edge}), flush=True)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", required=True, choices=["clip", "registers"])
    ap.add_argument("--out", required=True)
    ap.add_argument("--commit", default="unknown")
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    record = {}
    if os.path.exists(args.out):
        with open(args.out) as f:
            record = json.load(f)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)

    def save():
        with open(args.out, "w") as f:
            json.dump(record, f, indent=1)
            f.write("\n")
    if args.part == "registers":
        record["registers"] = {"kernel": "mm_pixels_clip of the clip variant (hot and generic body in one kernel)", "filters": measure_registers()}
        save()
        return 0
    import torch
    record.update({"commit": args.commit, "device": torch.cuda.get_device_name(0), "rounds": args.rounds,
                   "order": "rgba8, rgba8_opt, deep, and again",
                   "timing": "kernel: device events around the pixel kernel's launches (mmhip_drain_kernel_ms), summed over the batches of one "
                             "render_clip call of the whole clip into device memory; host: host clock between two device synchronisations around that call"})
    for which in ("ident", "pond"):
        record.setdefault("clip", {})[which] = measure_clip(which, args)
        save()
    return 0


if __name__ == "__main__":
    sys.exit(main())
