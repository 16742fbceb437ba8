#!/usr/bin/env python3
"""Generates tests/golden/nn_golden_frame11.npz: the reference's own nanoflann KD-tree search (oracle/_ref, built by oracle/Makefile
where the reference tree is present) on frame seed 11, ~38 k queries, identity part map - the inputs of
tests/test_oracle_cpu.py::test_oracle_nn_live_against_reference_build, regenerated from the seed there (case_inputs of
make_nn_golden_full.py); only the index array is committed.  Usage: python tests/golden/make_nn_golden_frame11.py"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, HERE)
from avatar_amd import synth  # noqa: E402
from oracle import oracle as orc  # noqa: E402
import make_nn_golden_full as mk  # noqa: E402

CASE = dict(seed=11, dense=False, coarse=False)
PATH = os.path.join(HERE, "nn_golden_frame11.npz")


def main():
    assert orc.have_reference_nn(), "oracle/_ref not built: run `make -C oracle ref` where the reference tree is present"
    smpl = synth.load_model(0)
    om = orc.OracleModel(smpl)
    pm, npart, cloud, vis, data, labels = mk.case_inputs(smpl, om, CASE)
    idx, _ = orc.reference_nn(pm[om.main_joint()].astype(np.int32), cloud, vis, data, labels, npart)
    np.savez_compressed(PATH, idx=idx.astype(np.int32))
    print("wrote", PATH, os.path.getsize(PATH), "bytes;", len(labels), "queries,", int((idx >= 0).sum()), "matched")


if __name__ == "__main__":
    main()
