#!/usr/bin/env python3
"""Record tests/golden/rowsum_bits.json: sha256 digests of the symmetric SpMV
kernels' products (cases and inputs: tests/test_gpu_rowsum_bits.py), taken
from the library KLE_LIBRARY names -- a build of the commit whose bits are to
be kept.  Needs a GPU.

    KLE_LIBRARY=/path/to/libkle.so python tools/record_product_bits.py [out.json]
"""
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "rowsum_bits.json")
    import pynama_amd as pa
    from pynama_amd import _lib
    import test_gpu_rowsum_bits as R
    pa.load()
    with tempfile.TemporaryDirectory() as tmp:
        rec = R.record(pa, tmp)
    with open(out, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"{out}: {len(rec['digests'])} cases from {_lib.LIBPATH}")


if __name__ == "__main__":
    main()
