#!/usr/bin/env python3
"""Fixture of the (radius, temp, knn) sweep: the reference's own scripts/test/test_all.py ``main(args)`` run ONCE PER CONFIGURATION
of a small grid -- what its scripts/launch/launch_test_batch.sh does -- on the synthetic dataset-3 case of
``segment_ds3_correction_reverse`` (52-row radargram, 8 x 8 patches, overlap (4, 0), T = 8, three radargrams, N = 12, correction with
the forced change points [None, 5, None], reverse pass), through the plumbing of make_golden.py (``run_segment_case``).

Runs only where the reference is available (CRW_REFERENCE); writes ``sweep_ds3_correction_reverse.npz``: the inputs, the grid and,
per configuration in the shell script's loop order (radius outermost, knn innermost), the int8 map the script saves and the final
map its report is computed on.  Arrays only.

Usage:  python tests/golden/make_golden_sweep.py
"""
import os
import sys
import tempfile

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import numpy as np
import torch

import make_golden as mg

RADII, TEMPS, KNNS = (2, 4, 12), (0.1, 0.01), (3, 5)
CXT_SIZE = 4


def main():
    torch.set_num_threads(8)
    _, _, _, ref_dataset, _ = mg.import_reference()
    tmp = tempfile.mkdtemp()
    mg.HERE = tmp  # run_segment_case writes its one-configuration fixture there
    saved, final, first = [], [], None
    for r in RADII:
        for t in TEMPS:
            for k in KNNS:
                cfg = dict(CXT_SIZE=CXT_SIZE, RADIUS=r, TEMP=t, KNN=k)
                mg.run_segment_case(ref_dataset, "one", 3, 5, 8, (8, 8), 4, 52, 3, 2, cfg, True, True, [None, 5, None], 55)
                g = dict(np.load(os.path.join(tmp, "one.npz")))
                if first is None:
                    first = g
                assert np.array_equal(g["rg"], first["rg"]) and np.array_equal(g["seg"], first["seg"])
                saved.append(g["saved_map"])
                final.append(g["final_map"])
    keep = ("rg", "seg", "dataset_id", "nclasses", "T", "patch", "overlap", "cxt_size", "use_last", "correction", "forced_change")
    np.savez_compressed(os.path.join(HERE, "sweep_ds3_correction_reverse.npz"), **{k: first[k] for k in keep},
                        radii=np.int32(RADII), temps=np.float64(TEMPS), knns=np.int32(KNNS),
                        saved_maps=np.stack(saved).astype(np.int8), final_maps=np.stack(final).astype(np.int8))
    distinct = len({m.tobytes() for m in final})
    print(f"sweep_ds3_correction_reverse: {len(final)} configurations, maps {final[0].shape}, {distinct} distinct final maps")


if __name__ == "__main__":
    main()
