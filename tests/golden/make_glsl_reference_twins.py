#!/usr/bin/env python3
"""Regenerates tests/golden/glsl_reference_twins.npz (run from the repo root, where the reference checkout is present:
python tests/golden/make_glsl_reference_twins.py).  Runs every case of tests/test_glsl_differential.py against the build of the reference's
shader functions (oracle/make_glsl_ref.py) and stores, per case, GOLDEN_ROWS evenly spaced inputs and what that build computed for them."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import test_glsl_differential as t  # noqa: E402
from oracle import make_glsl_ref  # noqa: E402

if __name__ == "__main__":
    if not make_glsl_ref.available():
        sys.exit("the reference checkout is not on this machine: nothing to record")
    t.RECORD = {}
    libs = t.libs.__wrapped__()
    t.test_triangle_tests_agree(libs)
    t.test_mnode_test_and_its_sorting_network_agree(libs)
    t.test_small_functions_agree(libs)
    for op, name in ((0, "BSDFEval"), (1, "BSDFPdf"), (2, "BSDFSample")):
        t.test_disney_bsdf_agrees(libs, op, name)
    np.savez_compressed(t.GOLDEN, **t.RECORD)
    print(t.GOLDEN, len(t.RECORD) // 2, "cases", os.path.getsize(t.GOLDEN), "bytes")
