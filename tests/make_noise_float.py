"""Records the CPU oracle's float maps of the noise cases of tests/noise_probes.py as tests/golden/noise_float/*.npy.
Run after build() where oracle/_ref/libmmnoise.so exists:  python tests/make_noise_float.py"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def live(kinds=("full", "simple")):
    """name -> the oracle's render of every case of those kinds"""
    import mathmap_amd as mm
    from oracle.ccgen import CpuFilter
    from tests import noise_probes as N
    cf = {"full": CpuFilter(mm.Filter(N.FULL).ir_json_raw), "simple": CpuFilter(mm.Filter(N.SIMPLE).ir_json_raw)}
    out = {}
    for name, kind, values in N.cases():
        if kind in kinds:
            m = cf[kind].render(N.SIZE, N.SIZE, uservals=N.uservals(values), floatmap=True)
            out[name] = m if kind == "full" else np.ascontiguousarray(m[..., 0])
    return out


def main():
    from tests import noise_probes as N
    maps = live()
    os.makedirs(N.GOLDEN, exist_ok=True)
    full = [c[0] for c in N.cases() if c[1] == "full"]
    for i in range(0, len(full), N.PER_FILE):
        np.save(os.path.join(N.GOLDEN, "full_%d.npy" % (i // N.PER_FILE)), np.stack([maps[n] for n in full[i:i + N.PER_FILE]]))
    np.save(os.path.join(N.GOLDEN, "simple.npy"), np.stack([maps[c[0]] for c in N.cases() if c[1] == "simple"]))
    print("%d cases" % len(maps))


if __name__ == "__main__":
    main()
