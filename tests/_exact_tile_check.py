"""Run as a script (subprocess of test_gpu_exact_contractions.py::test_exact_probes_under_forced_tiles): a ragged subset of the exact
probes (tests/exact_probes.py) with the tile choice forced through SKG_FORCE_BN, without the three-stage ring (SKG_NO_NS3) or with
another depth of the split-K ring (SKG_SPLIT_NS) - the library reads these once per process.  Same criterion: zero mismatching bits.
argv[1]: "tiles" (GEMM, every conv gather mode, epilogues; N % 320 == 0 so that every forced width applies) or "split"."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests import exact_probes as ep  # noqa: E402

what = sys.argv[1] if len(sys.argv) > 1 else "tiles"
bn = int(os.environ.get("SKG_FORCE_BN", "0")) or None
gemms, convs = ep.tile_check_cases(what)
n = 0
for case in gemms:      # (an AssertionError - a mismatch, a broken condition - ends the script with a non-zero status at the first one)
    for cls in case.classes:
        ep.run_gemm(case, cls, check_variant=False, bn=bn)
        n += 1
for case in convs:
    for cls in case.classes:
        ep.run_conv(case, cls, check_variant=False, bn=bn)
        n += 1
print(f"ALL OK ({n} probes, {what}, SKG_FORCE_BN={os.environ.get('SKG_FORCE_BN')}, SKG_NO_NS3={os.environ.get('SKG_NO_NS3')}, "
      f"SKG_SPLIT_NS={os.environ.get('SKG_SPLIT_NS')})")
