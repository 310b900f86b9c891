"""Prints the table of PARITY.md, section "Corner selection on a given response map": how ordinary images load the counters of the
selection kernels.  CPU only: the oracle's min-eigenvalue map of each image, the counters of tests/gftt_ref.py, minDistance 20.
Images: uniform noise = numpy default_rng(0).integers(0, 256), drawn 752 x 480 first and 1280 x 720 second from the same generator;
checkerboards and dots = tests/test_gftt_ref.py (grey levels 20 / 220).  Run from the repository root: python tools/gftt_counter_table.py"""
import os
import sys
import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import lvo                                             # noqa: E402
from tests import gftt_ref as R                                    # noqa: E402
from tests.test_gftt_ref import checker, dots                      # noqa: E402

rng = np.random.default_rng(0)
images = [("uniform noise", 752, 480, rng.integers(0, 256, (480, 752)).astype(np.uint8), 4096),
          ("uniform noise", 1280, 720, rng.integers(0, 256, (720, 1280)).astype(np.uint8), 4096),
          ("checkerboard, 4 px squares", 752, 480, checker(4, 752, 480), 500),
          ("2 x 2 dots, 6 px lattice", 752, 480, dots(752, 480), 4096),
          ("checkerboard, 2 px squares", 752, 480, checker(2, 752, 480), 500)]
print("| image | size | candidates | fullest tile | fullest bin | fullest group | oracle returns (asked) | = restatement |")
for name, w, h, img, maxc in images:
    p = lvo.LkPyramid(img, 21, 0)
    eig = p.min_eigen_map()
    vals, idx = R.candidates(eig, 0.01)
    bins, groups = R.bin_counts(vals)
    got = p.good_features(maxc, 0.01, 20.0)
    same = np.array_equal(got, R.select(eig, maxc, 0.01, 20.0))
    print(f"| {name} | {w} x {h} | {len(vals):,} | {R.tile_counts(idx, w, h).max():,} | {bins.max():,} | {groups.max():,} | {len(got)} ({maxc}) | {same} |")
