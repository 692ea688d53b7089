"""SHA-256 of the generated kernel text of the probe filters, without the device prelude.

The translation unit hipgen.cpp writes is options, the math preludes, mm_device.h, then the text generated for the
filter.  `body_text` is that last part: what follows the last line of mm_device.h.  Run at a commit, this records what
that commit generates for Ident, Pond and Droste (nearest and bilinear), so that a later change of the prelude can show
that it left the generated code alone (tests/test_image_sequence_api.py).  No GPU needed.

    python tools/kernel_body_digest.py tests/golden/kernel_body_digests.json <commit>
"""
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PROBES = ("ident", "pond", "droste")


def body_text(kernel_source):
    with open(os.path.join(ROOT, "mathmap_amd", "csrc", "mm_device.h")) as f:
        last = f.read().rstrip().split("\n")[-1]
    lines = kernel_source.split("\n")
    at = max(i for i, line in enumerate(lines) if line == last)
    return "\n".join(lines[at + 1:])


def digests():
    from tests import filters as F
    out = {}
    for name in PROBES:
        for intersample in (False, True):
            src = F.load(name, intersample=intersample).kernel_source
            out["%s/%s" % (name, "bilinear" if intersample else "nearest")] = hashlib.sha256(body_text(src).encode()).hexdigest()
    return out


if __name__ == "__main__":
    with open(sys.argv[1], "w") as f:
        json.dump({"commit": sys.argv[2], "body_sha256": digests()}, f, indent=1, sort_keys=True)
        f.write("\n")
