#!/usr/bin/env python3
"""Soak version of tests/test_gpu_parity.py::test_random_scenes_cameras_and_skies_bit_identical_to_oracle: 200 more seeds.
Two seeds in three run bounce 1 over the per-pixel leaf lists whatever the batch depth (the test's 1 .. 5 samples per pixel are below the default threshold), one of them
with a capacity of 1 .. 4 entries so that most lists overflow: RF_PRIMARY_LIST_MIN_SAMPLES / RF_PRIMARY_LIST_CAPACITY, read when the handle is made.  The pinhole cameras
(a third of the seeds) are the ones that can take the lists.  Where the lists run, bounce 1 is the fused kernel (kPrimaryFused, the default) for every other triple of
seeds and the three launches (RF_PRIMARY_FUSED=0) for the triples in between."""
import os, sys
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
os.chdir(ROOT)
import test_gpu_parity as T
first, count = (int(sys.argv[1]) if len(sys.argv) > 1 else 12), (int(sys.argv[2]) if len(sys.argv) > 2 else 200)
bad = 0
for seed in range(first, first + count):
    for k in ("RF_PRIMARY_LIST_MIN_SAMPLES", "RF_PRIMARY_LIST_CAPACITY", "RF_PRIMARY_FUSED"):
        os.environ.pop(k, None)
    if seed % 3 != 0:
        os.environ["RF_PRIMARY_LIST_MIN_SAMPLES"] = "1"
    if seed % 3 == 2:
        os.environ["RF_PRIMARY_LIST_CAPACITY"] = str(1 + seed % 4)
    if (seed // 3) % 2 == 1:
        os.environ["RF_PRIMARY_FUSED"] = "0"
    try:
        T.test_random_scenes_cameras_and_skies_bit_identical_to_oracle(seed)
    except AssertionError as e:
        bad += 1
        print("seed", seed, "FAILED", str(e)[:300])
print(f"seeds {first}..{first + count - 1}: {bad} failures")
