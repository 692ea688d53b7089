"""Records the CPU oracle's renders of the example filters that call libnoise (perlin, billow, ridged_multi,
voronoi) as tests/golden/oracle_renders/<stem>.png, for tests/test_gpu_parity.py::test_reference_examples_on_gpu
on machines where the oracle's noise library (oracle/_ref/libmmnoise.so, built by oracle/build_ref.sh from the
reference's vendored libnoise) is not there.  Same case as the test: the IR fixture, default user values, every
image input bound to the 128x128 corner of marlene.png, t = 0.3.  Run after build() where oracle/_ref/libmmnoise.so
exists:  python tests/make_oracle_renders.py
"""
import gzip
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

GOLDEN = os.path.join(ROOT, "tests", "golden")
OUT = os.path.join(GOLDEN, "oracle_renders")
W = H = 128
T = 0.3


def uses_noise(ir):
    from oracle.ccgen import NOISE_OPS
    return any('"%s"' % op in ir for op in NOISE_OPS)


def example_case(stem, marlene):
    """(IR text, images) of one example as test_reference_examples_on_gpu renders it."""
    import mathmap_amd as mm
    ir = gzip.open(os.path.join(GOLDEN, "ir_examples", stem + ".json.gz"), "rt").read()
    img = np.ascontiguousarray(marlene[:H, :W])
    flt = mm.Filter("", ir_json=ir)
    return ir, {u["name"]: img for u in flt.uservals if u["kind"] == mm.api.UV_IMAGE}


def main():
    import json
    from PIL import Image
    from oracle.ccgen import CpuFilter
    from tests.conftest import load_png_rgb
    marlene = load_png_rgb("marlene.png")
    os.makedirs(OUT, exist_ok=True)
    for stem in json.load(open(os.path.join(GOLDEN, "ir_examples", "manifest.json"))):
        ir, images = example_case(stem, marlene)
        if not uses_noise(ir):
            continue
        rgba = CpuFilter(ir).render(W, H, images=images, t=T)
        Image.fromarray(rgba, "RGBA").save(os.path.join(OUT, stem + ".png"), optimize=True)
        print(stem)


if __name__ == "__main__":
    main()
