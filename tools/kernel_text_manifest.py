"""Digests of everything the HIP generator writes, over a corpus of filters, options and environment hooks.  No GPU needed.

The generator's whole output is text (the translation unit, its clip variant and their keys) plus the few numbers of
KernelSource the launch geometry is computed from.  A change that is meant to leave the generated code alone -- a
refactor of hipgen*.cpp -- is checked by writing this manifest at both commits and comparing:

    python tools/kernel_text_manifest.py --repo <built checkout of the parent> --out parent.json
    python tools/kernel_text_manifest.py --out new.json
    python tools/kernel_text_manifest.py --compare parent.json new.json [--summary profiles/<record>.json]

`--repo` names the built tree `mathmap_amd` is imported from (default: this tree); the corpus (tests/) always comes
from this tree.  Per (configuration, case) the manifest holds the SHA-256 of kernel_source, of clip_kernel_source and
of .specialized({}).kernel_source, of the shutter, sampled and refine variants' texts (or the refusal's text), the launch
geometry at 640x480 and 8192x8192, the clip geometry for 8 frames, num_native_calls -- or the compile error's text.
Besides the texts it holds the host side's arithmetic: the eight clip plans of a few named filters at a few geometries,
under the default byte budgets and under small ones (a fresh process per budget set: the library reads them once).
`--compare` prints the differing cases and exits non-zero if there is one; `--summary` writes the per-configuration
counts and one digest per side.
"""
import argparse
import concurrent.futures
import glob
import gzip
import hashlib
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PAIR_MARK = "mm_p += 2)"                # the pair-mode pixel loop
EXIT_MARK = "#define MM_PAIR_EXIT 1"    # ... with exit-driven loops

# every hook of the generator alone, at each value its code distinguishes; then MMHIP_PAIR=1 with each pair-mode switch
ENVIRONMENTS = [{}] + [{k: v} for k, vs in [
    ("MMHIP_UNROLL", "124"), ("MMHIP_TILE_W", ["8", "64"]), ("MMHIP_SINGLE_PIXEL", "01"), ("MMHIP_PAIR", "01"),
    ("MMHIP_PAIR_MASKS", "0"), ("MMHIP_PAIR_EXIT", "0"), ("MMHIP_PAIR_EXIT_TAIL", "0"), ("MMHIP_PAIR_NO_UNIFORM", "1"),
    ("MMHIP_PAIR_SPREAD", "0"), ("MMHIP_NT_STORE", "01"), ("MMHIP_XCD_ORDER", "01"), ("MMHIP_WAVES_PER_EU", "2"), ("MMHIP_NO_FETCHED_RESULT", "1"),
    ("MMHIP_NO_SAME_TAPS", "1"), ("MMHIP_NO_OUTSIDE_SHORTCUT", "1"), ("MMHIP_FRAME_HOT", "01"), ("MMHIP_NO_ROW_SLICE", "1"),
    ("MMHIP_MAX_CALL_DEPTH", "4")] for v in vs] + [
    {"MMHIP_PAIR": "1", k: v} for k, v in [("MMHIP_PAIR_EXIT", "0"), ("MMHIP_PAIR_EXIT_TAIL", "0"), ("MMHIP_PAIR_MASKS", "0"),
                                           ("MMHIP_PAIR_NO_UNIFORM", "1"), ("MMHIP_PAIR_SPREAD", "0")]]


# the clip plans: byte budgets (read once per process), filters, (region_w, num_rows, render_w, frames), samples, aa
BUDGETS = [{}, {"MMHIP_CLIP_SHUTTER_BYTES": "3000000", "MMHIP_CLIP_SS_BYTES": "2000000", "MMHIP_CLIP_NATIVE_BYTES": "20000000"}]
PLAN_FILTERS = ("ident", "mandelbrot", "pond", "gaussian_blur")      # and the first named filter with a closure, and clip_probes.WAVE for its per-row slice
PLAN_GEOMETRIES = ((64, 64, 64, 64), (333, 207, 400, 7), (640, 480, 640, 8), (4096, 4096, 4096, 3))
PLAN_SAMPLES = (1, 4, 256)
PLAN_AA = (1, 2, (3, 2))


def env_name(env):
    return ",".join("%s=%s" % kv for kv in sorted(env.items())) or "default"


def corpus():
    """[(case id, sub-corpus, kwargs of mathmap_amd.Filter)]; sub-corpus "arith" is the pair-mode class."""
    from tests import clip_probes, filters as F, fuzz_filters as Z, pair_exit_probes, sequence_probes as S
    cases = []
    for d in ("ir_examples", "ir"):
        for path in sorted(glob.glob(os.path.join(ROOT, "tests", "golden", d, "*.json.gz"))):
            with gzip.open(path, "rt") as f:
                ir = f.read()
            for i in (False, True):
                cases.append(("%s/%s/%d" % (d, os.path.basename(path)[:-8], i), "fixture", dict(ir_json=ir, intersample=i)))

    def named(name, **options):
        kw = dict(ir_json=F.ir_text(name)) if name in F.REFERENCE_IR else dict(source=F.SOURCES[name])
        tag = ",".join("%s=%s" % kv for kv in sorted(options.items()))
        cases.append(("filters/%s/%s" % (name, tag), "named", dict(kw, **options)))
    for name in F.NAMES:
        named(name)
    for name in ("ident", "pond", "mandelbrot", "droste", "gaussian_blur", "recursive_data"):
        named(name, supersampling=True)
        for e in range(4):
            named(name, edge_x=e, edge_y=e)
        named(name, pixel_inc=2)
        named(name, tile_w=64)
    named("mandelbrot", specialize=True)
    named("droste", specialize=True)
    for s in range(400):
        cases.append(("fuzz/arith/%d" % s, "arith", dict(source=Z.make_filter_arith(s))))
    for s in range(120):
        cases.append(("fuzz/filter/%d" % s, "fuzz", dict(source=Z.make_filter(s)[0])))
    for s in range(40):
        src, _, opts = Z.make_filter_ex(s)
        cases.append(("fuzz/ex/%d" % s, "fuzz", dict(source=src, **opts)))
    for name, text, _ in pair_exit_probes.PROBES:
        cases.append(("pair_exit/%s" % name, "arith", dict(source=text)))
    frames = {"literal": "0", "animation": S.FRAME_OF_ANIMATION, "userval": S.FRAME_OF_USERVAL, "slit": S.SLIT_FRAME,
              "large": S.LARGE_FRAME}
    seq = {"%s/%s" % (t, f): S.text(getattr(S, t), frames[f])
           for t in ("SELECT", "SLIT", "RECURSIVE", "CLOSURE", "LARGE") for f in frames
           if (f != "userval" or t in ("SELECT", "RECURSIVE", "CLOSURE")) and (f != "large" or t == "LARGE")}
    for t in ("PLAIN", "SLIT_INDEX", "BLEND", "BLUR", "RENDER", "LARGE_INDEX"):
        seq[t] = getattr(S, t)
    seq["BLEND_ORACLE"] = S.BLEND_ORACLE.format(A=0, B=1000, C=0)
    for name, text in sorted(seq.items()):
        for i in (False, True):
            cases.append(("sequence/%s/%d" % (name, i), "probe", dict(source=text, intersample=i)))
        cases.append(("sequence/%s/pixel_inc" % name, "probe", dict(source=text, pixel_inc=2)))
    for name in ("WAVE", "MEDIUM"):
        for i in (False, True):
            cases.append(("clip/%s/%d" % (name, i), "probe", dict(source=getattr(clip_probes, name), intersample=i)))
    assert len(set(c[0] for c in cases)) == len(cases)
    return cases


def sha(text):
    return hashlib.sha256(text.encode()).hexdigest()


def attempt(mm, what):
    try:
        return what()
    except (mm.MathMapError, ValueError) as e:
        return {"error": str(e)}


def record(mm, kwargs):
    try:
        flt = mm.Filter(**kwargs)
    except mm.MathMapError as e:
        return {"error": str(e)}
    ks = flt.kernel_source
    rec = {"kernel": sha(ks), "clip": sha(flt.clip_kernel_source), "pair": PAIR_MARK in ks, "exit": EXIT_MARK in ks,
           "native_calls": flt.num_native_calls,
           "geometry": [list(flt.launch_geometry(w, h).values()) for w, h in ((640, 480), (8192, 8192))],
           "clip_geometry": list(flt.clip_launch_geometry(640, 480, 8).values()),
           "variants": {v: attempt(mm, lambda: sha(getattr(flt, v + "_kernel_source"))) for v in ("shutter", "sampled", "refine")}}
    try:
        sp = flt.specialized({})
        sks = sp.kernel_source
        rec["specialized"] = {"kernel": sha(sks), "clip": sha(sp.clip_kernel_source), "pair": PAIR_MARK in sks, "exit": EXIT_MARK in sks,
                              "geometry": list(sp.launch_geometry(8192, 8192).values())}
    except mm.MathMapError as e:
        rec["specialized"] = {"error": str(e)}
    return rec


def sweep(job):
    """One configuration: the hooks are set in this (worker) process, which the generator reads at every compile."""
    repo, env = job
    mm = import_from(repo)
    for k in [k for k in os.environ if k.startswith("MMHIP_")]:
        del os.environ[k]
    os.environ.update(env)
    return env_name(env), {cid: dict(record(mm, kwargs), sub=sub) for cid, sub, kwargs in corpus()}


def import_from(repo):
    """mathmap_amd of the built tree `repo`; tests/ stays this tree's."""
    if "mathmap_amd" not in sys.modules:
        sys.path.insert(0, repo)
        import mathmap_amd
        assert os.path.dirname(os.path.dirname(os.path.abspath(mathmap_amd.__file__))) == os.path.abspath(repo)
        sys.path.remove(repo)
        sys.path.insert(0, ROOT)
    import mathmap_amd as mm
    return mm


def plans_child(repo):
    """Prints the clip plans under this process's budgets as JSON: {filter: {geometry: {plan: fields or error}}}."""
    mm = import_from(repo)
    from tests import clip_probes, filters as F
    chosen = {name: F.load(name) for name in PLAN_FILTERS}
    closure = next(n for n in F.NAMES if F.load(n).num_closures > 0)
    chosen["closure:" + closure] = F.load(closure)
    chosen["row_slice:wave"] = mm.Filter(clip_probes.WAVE)
    assert "mm_rows(" in chosen["row_slice:wave"].kernel_source
    out = {}
    for name, flt in chosen.items():
        for w, rows, rw, frames in PLAN_GEOMETRIES:
            got = {"batch": attempt(mm, lambda: flt.clip_batch_plan(w, rows, frames)),
                   "native": attempt(mm, lambda: flt.clip_native_plan(w, rows, frames, rw, rows)),
                   "supersample": attempt(mm, lambda: flt.clip_supersample_plan(w, rows, frames))}
            for k in PLAN_SAMPLES:
                got["shutter/%d" % k] = attempt(mm, lambda: flt.clip_shutter_plan(w, rows, rw, k, frames))
                got["shutter_fused/%d" % k] = attempt(mm, lambda: flt.clip_shutter_fused_plan(w, rows, k, frames))
                for aa in PLAN_AA:
                    got["sampled/%d/%s" % (k, aa)] = attempt(mm, lambda: flt.clip_sampled_plan(w, rows, rw, k, aa, frames))
                    got["sampled_fused/%d/%s" % (k, aa)] = attempt(mm, lambda: flt.clip_sampled_fused_plan(w, rows, k, aa, frames))
            for aa in PLAN_AA:
                got["adaptive/%s" % (aa,)] = attempt(mm, lambda: flt.clip_adaptive_plan(w, rows, rw, aa, frames))
            out.setdefault(name, {})["%dx%d/%d/%d" % (w, rows, rw, frames)] = got
    json.dump(out, sys.stdout, sort_keys=True)


def clip_plans(repo):
    """{budget set: plans_child's record}, each from a process of its own."""
    plans = {}
    for budget in BUDGETS:
        env = dict({k: v for k, v in os.environ.items() if not k.startswith("MMHIP_")}, **budget)
        done = subprocess.run([sys.executable, os.path.abspath(__file__), "--plans-child", "--repo", repo], env=env, cwd=ROOT,
                              capture_output=True, text=True, check=True)
        plans[env_name(budget)] = json.loads(done.stdout)
    return plans


def write_manifest(repo, out, jobs):
    repo = os.path.abspath(repo)
    commit = subprocess.run(["git", "-C", repo, "rev-parse", "HEAD"], capture_output=True, text=True).stdout.strip()
    dirty = bool(subprocess.run(["git", "-C", repo, "status", "--porcelain", "--untracked-files=no"], capture_output=True, text=True).stdout.strip())
    with concurrent.futures.ProcessPoolExecutor(jobs) as pool:
        configs = dict(pool.map(sweep, [(repo, env) for env in ENVIRONMENTS]))
    with open(out, "w") as f:
        json.dump({"commit": commit, "modified": dirty, "configs": configs, "plans": clip_plans(repo)}, f, sort_keys=True)
    print("%s: %d configurations, %d cases each, clip plans under %d budget sets" % (out, len(configs), len(next(iter(configs.values()))), len(BUDGETS)))


def stats(cases):
    """Counts of one configuration's cases, and one SHA-256 over their sorted digests."""
    texts = [r for c in cases.values() for r in (c, c.get("specialized", {})) if "kernel" in r]
    arith = [c for c in cases.values() if c["sub"] == "arith" and "kernel" in c]
    fuzz = [c for c in cases.values() if c["sub"] in ("arith", "fuzz") and "kernel" in c]
    return {"texts": 2 * len(texts),      # each with its clip variant
            "texts_in_pair_mode": sum(r["pair"] for r in texts), "texts_exit_driven": sum(r["exit"] for r in texts),
            "arith_sources": len(arith), "arith_in_pair_mode": sum(c["pair"] for c in arith), "arith_exit_driven": sum(c["exit"] for c in arith),
            "fuzz_in_pair_mode": sum(c["pair"] for c in fuzz),
            "variant_texts": sum(not isinstance(d, dict) for r in texts for d in r.get("variants", {}).values()),
            "variant_refusals": sum(isinstance(d, dict) for r in texts for d in r.get("variants", {}).values()),
            "compile_failures": sum("error" in c for c in cases.values()) + sum("error" in c.get("specialized", {}) for c in cases.values()),
            "sha256": sha(json.dumps(sorted(cases.items()), sort_keys=True))}


def compare(path_a, path_b, summary):
    a, b = (json.load(open(p)) for p in (path_a, path_b))
    differing = 0
    configs = {}
    for name in sorted(set(a["configs"]) | set(b["configs"])):
        ca, cb = a["configs"].get(name, {}), b["configs"].get(name, {})
        for cid in sorted(set(ca) | set(cb)):
            if ca.get(cid) != cb.get(cid):
                differing += 1
                keys = sorted(k for k in set(ca.get(cid) or {}) | set(cb.get(cid) or {}) if (ca.get(cid) or {}).get(k) != (cb.get(cid) or {}).get(k))
                print("DIFFERENT %s %s: %s" % (name, cid, ", ".join(keys)))
        sa, sb = stats(ca), stats(cb)
        configs[name] = dict({k: v for k, v in sa.items() if k != "sha256"}, sha256_a=sa["sha256"], sha256_b=sb["sha256"],
                             equal=sa == sb)
        # the sweep must not pass vacuously: the pair-mode configurations are in pair mode
        want = []
        if "MMHIP_PAIR=1" in name:
            off = "MMHIP_PAIR_EXIT=0" in name or "MMHIP_PAIR_MASKS=0" in name
            want = [("arith_in_pair_mode", 400, None), ("arith_exit_driven", 0 if off else 400, 0 if off else None)]
        elif name == "default":
            want = [("fuzz_in_pair_mode", 120, None)]
        elif "MMHIP_PAIR_EXIT=0" in name or "MMHIP_PAIR_MASKS=0" in name:
            want = [("texts_exit_driven", 0, 0)]
        for key, lo, hi in want:
            for side, s in (("a", sa), ("b", sb)):
                if s[key] < lo or (hi is not None and s[key] > hi):
                    differing += 1
                    print("VACUOUS %s side %s: %s = %d" % (name, side, key, s[key]))
    # the clip plans: a case is one filter at one geometry under one budget set
    plans = {}
    for budget in sorted(set(a.get("plans", {})) | set(b.get("plans", {}))):
        pa, pb = a.get("plans", {}).get(budget, {}), b.get("plans", {}).get(budget, {})
        flat = [{"%s %s" % (name, geo): rec for name, geos in side.items() for geo, rec in geos.items()} for side in (pa, pb)]
        for cid in sorted(set(flat[0]) | set(flat[1])):
            if flat[0].get(cid) != flat[1].get(cid):
                differing += 1
                keys = sorted(k for k in set(flat[0].get(cid) or {}) | set(flat[1].get(cid) or {})
                              if (flat[0].get(cid) or {}).get(k) != (flat[1].get(cid) or {}).get(k))
                print("DIFFERENT plans under %s, %s: %s" % (budget, cid, ", ".join(keys)))
        plans[budget] = {"filters": sorted(pa), "cases": len(flat[0]), "plans": sum(len(r) for r in flat[0].values()),
                         "refusals": sum("error" in p for r in flat[0].values() for p in r.values()),
                         "sha256_a": sha(json.dumps(pa, sort_keys=True)), "sha256_b": sha(json.dumps(pb, sort_keys=True)), "equal": pa == pb}
        # not vacuous: both sides have plans, and the small budgets change some of them
        if not flat[0] or not flat[1] or (budget != "default" and pa == a["plans"].get("default")):
            differing += 1
            print("VACUOUS plans under %s" % budget)
    print("%d configurations, %d plan sets, %d differing cases" % (len(configs), len(plans), differing))
    if summary:
        old = json.load(open(summary)) if os.path.exists(summary) else {}
        old.update({"a": {"commit": a["commit"], "modified": a["modified"]}, "b": {"commit": b["commit"], "modified": b["modified"]},
                    "differing_cases": differing, "configurations": configs, "clip_plans": plans})
        with open(summary, "w") as f:
            json.dump(old, f, indent=1, sort_keys=True)
            f.write("\n")
    return 1 if differing else 0


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--repo", default=ROOT, help="built tree to import mathmap_amd from")
    ap.add_argument("--out", default="kernel_text_manifest.json")
    ap.add_argument("--jobs", type=int, default=min(16, os.cpu_count() or 1))
    ap.add_argument("--compare", nargs=2, metavar=("A", "B"))
    ap.add_argument("--summary", help="with --compare: JSON record to write the per-configuration counts into")
    ap.add_argument("--plans-child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.plans_child:
        sys.exit(plans_child(os.path.abspath(args.repo)))
    if args.compare:
        sys.exit(compare(args.compare[0], args.compare[1], args.summary))
    write_manifest(args.repo, args.out, args.jobs)
