#!/usr/bin/env python3
"""Writes tests/golden/ref_bits.npz and ref_bits.json: the answers of the reference's own code, compiled as it is into
oracle/_ref/libdd_ref_bits.so (`make -C oracle _ref`), on the inputs tests/test_ref_bits.py defines.  These ARE reference outputs:
run only with that library built from the reference tree.

    python tests/golden/make_ref_bits.py"""
import ctypes as C
import json
import os
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import numpy as np
from tests import test_ref_bits as t

with tempfile.TemporaryDirectory() as d:
    arrays, structs = t.reference_answers(C.CDLL(t.REF), d)
np.savez(t.GOLDEN + ".npz", **arrays)
with open(t.GOLDEN + ".json", "w") as f:
    json.dump(structs, f)
print({k: v.shape for k, v in arrays.items()}, len(structs["window_lines"]), "window files")
