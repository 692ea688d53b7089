#!/usr/bin/env python3
"""How evenly the specialised Mandelbrot pair kernel fills the wave slots of an MI355X: a model in NumPy (no GPU, no library).

    python tools/pair_tail_model.py [--size 2048] [--scale 4] [--tile 4x4] [--ppt 16] [--rule consecutive|spread] [--json]

The frame (the examples' Mandelbrot at its default values: c = (x, y) over [-1, 1]^2, at most 31 trips, |z| < 2) is iterated in
float32 with the kernel's operations.  A workgroup is `tile` (columns x work-item rows) work-items, four waves one above the
other; a work-item renders two adjacent rows per step and --ppt rows in all, so a wave's step is a patch tile_w columns by
tile_h / 2 rows and runs as many trips as its slowest pixel.  The rule says which steps a workgroup owns:

    consecutive   the ppt / 2 steps of tile row ty follow each other: rows from ty * tile_h * ppt on
    spread        step k is step k * tiles_y + ty of the frame (MMHIP_PAIR_SPREAD): same columns, 1 / (ppt / 2) of the height apart

A wave costs --entry trips once and, per step, its trips plus --step (defaults 4.3 and 2.4: what the SQ counters of
profiles/r11_sq_counters_mandelbrot8192.json leave per wave and per step next to the loops' trips); a workgroup holds its slot
until its slowest wave is done.  Workgroups are dealt round-robin to 8 XCDs, mapped to tiles by the kernel's tile order 2, and
handed in order to whichever of an XCD's --slots workgroup slots (256: 32 CUs x 4 SIMDs x 8 waves / 4 waves) is free first.
Printed: iterations per pixel, wave trips per step, and per XCD the makespan over the ideal (the XCD's load / slots) and when
the first slot goes idle for good; then the launch's makespan over the ideal of the whole device.

The default arguments are the 8192 x 8192 launch (tile 16 x 16) scaled by four in both directions: the same 16 384 workgroups
over the same part of the plane, every pixel sampled at the middle of the 4 x 4 pixels it stands for (--scale).  `--size 8192
--scale 1 --tile 16x16` is the launch itself, a minute of NumPy."""
import argparse
import heapq
import json

import numpy as np


def iterations(size, scale=1, limit=31):
    """trips of the filter's loop per pixel, (rows, columns): z = z * z + c from 0 while |z| < 2 and fewer than `limit` trips.
    Pixel i stands for pixels i * scale ... of a frame `scale` times as large and is sampled at their middle, in that frame's
    coordinates (CALC_VIRTUAL_X: -1 and 1 at the first and last pixel's centres)"""
    half = (size * scale - 1) / 2.0
    ax = ((np.arange(size, dtype=np.float64) * scale + (scale - 1) / 2.0 - half) / half).astype(np.float32)
    cr = ax[None, :] + np.zeros((size, 1), np.float32)
    ci = (-ax)[:, None] + np.zeros((1, size), np.float32)
    zr, zi = np.zeros_like(cr), np.zeros_like(cr)
    n = np.zeros(cr.shape, np.int32)
    live = np.ones(cr.shape, bool)
    for _ in range(limit):
        zr, zi = np.where(live, (zr * zr - zi * zi) + cr, zr), np.where(live, np.float32(2.0) * (zr * zi) + ci, zi)
        n += live
        live &= zr * zr + zi * zi < np.float32(4.0)
        if not live.any():
            break
    return n


def tile_of(bid, tiles_x, nwg):
    """the kernel's tile order 2: workgroup -> tile number"""
    m = max(tiles_x - 1, 1).bit_length()
    full = (nwg >> (m + 3)) << (m + 3)
    q = bid >> 3
    return np.where(bid < full, ((((q >> m) << 3) + (bid & 7)) << m) + (q & ((1 << m) - 1)), bid)


def step_rows(rule, ty, k, tiles_y, nseg, step_h):
    """first row of step k of a workgroup in tile row ty"""
    if rule == "consecutive":
        return (ty * nseg + k) * step_h
    if rule == "spread":
        return (k * tiles_y + ty) * step_h
    raise ValueError(rule)


def model(size=2048, tile=(4, 4), ppt=16, rule="consecutive", entry=4.3, step=2.4, slots=256, xcds=8, scale=4):
    tw, th = tile
    n = iterations(size, scale)
    step_h, nseg = 2 * th, ppt // 2
    tiles_x, tiles_y = -(-size // tw), -(-size // (th * ppt))
    nwg = tiles_x * tiles_y
    # trips of every wave step of the frame: the slowest pixel of a patch tw columns by step_h / 4 rows
    ph = step_h // 4
    rows_p, cols_p = -(-size // ph) * ph, tiles_x * tw
    padded = np.zeros((rows_p, cols_p), np.int32)
    padded[:size, :size] = n
    trips = padded.reshape(rows_p // ph, ph, tiles_x, tw).max(axis=(1, 3))          # (wave step rows, tile columns)
    inside = (np.arange(rows_p // ph) * ph < size)
    bid = np.arange(nwg)
    t = tile_of(bid, tiles_x, nwg)
    ty, tx = t // tiles_x, t % tiles_x
    wave = np.full((nwg, 4), entry)
    owned = np.zeros(trips.shape[0], np.int32)
    for k in range(nseg):
        first = step_rows(rule, ty, k, tiles_y, nseg, step_h)
        for w in range(4):
            r = first // ph + w
            ok = (r < trips.shape[0]) & (first < size)
            rr = np.where(ok, r, 0)
            wave[:, w] += np.where(ok & inside[rr], trips[rr, tx] + step, 0.0)
            np.add.at(owned, rr[ok & (tx == 0)], 1)
    assert (owned[inside] == 1).all(), "a step row is owned more or less than once"
    cost = wave.max(axis=1)
    res = {"size": size, "scale": scale, "tile": [tw, th], "ppt": ppt, "rule": rule, "workgroups": int(nwg),
           "iterations_per_pixel": float(n.mean()), "wave_trips_per_step": float(trips[inside].mean()), "xcd": []}
    worst, idle = 0.0, float("inf")
    for x in range(xcds):
        c = cost[bid % xcds == x]
        free = [0.0] * slots
        heapq.heapify(free)
        for v in c:
            s = heapq.heappop(free)
            heapq.heappush(free, s + v)
        makespan, ideal = max(free), c.sum() / slots
        res["xcd"].append({"load": float(c.sum()), "makespan_over_ideal": makespan / ideal, "first_slot_idle_at": min(free) / makespan})
        worst, idle = max(worst, makespan), min(idle, min(free))
    res["makespan_over_ideal"] = worst / (cost.sum() / (slots * xcds))
    res["first_slot_idle_at"] = idle / worst
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--size", type=int, default=2048, help="frame edge in pixels")
    ap.add_argument("--scale", type=int, default=4, help="the frame this one stands for is that many times as large: a pixel is sampled at the middle of its block")
    ap.add_argument("--tile", default="4x4", help="workgroup shape, columns x work-item rows")
    ap.add_argument("--ppt", type=int, default=16, help="rows per work-item (even)")
    ap.add_argument("--rule", default="consecutive", choices=["consecutive", "spread"])
    ap.add_argument("--entry", type=float, default=4.3, help="trips charged per wave")
    ap.add_argument("--step", type=float, default=2.4, help="trips charged per step")
    ap.add_argument("--slots", type=int, default=256, help="workgroup slots per XCD")
    ap.add_argument("--json", action="store_true")
    a = ap.parse_args()
    tw, th = (int(v) for v in a.tile.split("x"))
    r = model(a.size, (tw, th), a.ppt, a.rule, a.entry, a.step, a.slots, scale=a.scale)
    if a.json:
        print(json.dumps(r))
        return
    print("%d x %d, tile %d x %d, %d rows per work-item, %s steps: %d workgroups" % (a.size, a.size, tw, th, a.ppt, a.rule, r["workgroups"]))
    print("iterations per pixel %.2f, wave trips per step %.2f" % (r["iterations_per_pixel"], r["wave_trips_per_step"]))
    for i, x in enumerate(r["xcd"]):
        print("XCD %d: load %.0f, makespan / ideal %.3f, first slot idle at %.2f" % (i, x["load"], x["makespan_over_ideal"], x["first_slot_idle_at"]))
    print("launch: makespan / ideal %.3f, first slot idle at %.2f" % (r["makespan_over_ideal"], r["first_slot_idle_at"]))


if __name__ == "__main__":
    main()
