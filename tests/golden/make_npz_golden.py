#!/usr/bin/env python3
"""Generates tests/golden/npz_cnpy_golden.json: what the reference's own .npz reader (cnpy::npz_load, built by oracle/Makefile into
oracle/_ref/libcnpy_ref.so where the reference tree is present) returns for each fixture of tests/test_npz_against_cnpy.py - per
member its word size, fortran_order flag, shape and the SHA-256 of its data bytes.  Usage: python tests/golden/make_npz_golden.py"""
import hashlib
import json
import os
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))
from avatar_amd import synth  # noqa: E402
import test_npz_against_cnpy as t  # noqa: E402


def main():
    assert os.path.exists(t.REF_SO), "oracle/_ref/libcnpy_ref.so not built: run `make -C oracle ref` where the reference tree is present"
    smpl = synth.load_model(0)
    lib = t._ref_lib()
    out = {}
    with tempfile.TemporaryDirectory() as td:
        for variant in t.VARIANTS:
            path = os.path.join(td, variant + ".npz")
            t.write_fixture(smpl, variant, path)
            out[variant] = {name: [ws, fo, list(shape), hashlib.sha256(raw.tobytes()).hexdigest()]
                            for name, (ws, fo, shape, raw) in sorted(t._load_ref(lib, path).items())}
    with open(t.GOLDEN, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print("wrote", t.GOLDEN, {v: len(m) for v, m in out.items()})


if __name__ == "__main__":
    main()
