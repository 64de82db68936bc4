"""slk.PREDICT_PAIR_MIN_BATCH mirrors SLK_PREDICT_PAIR_MIN_BATCH of include/slk.h (the batch size from which the plain Msckf
predict route runs two filters per wave): the GPU tests read the Python value to place their batches on either side of it."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_python_constant_mirrors_the_header():
    from slkpkg import slk
    src = open(os.path.join(ROOT, "include", "slk.h")).read()
    found = re.findall(r"^#define\s+SLK_PREDICT_PAIR_MIN_BATCH\s+(\d+)\s*$", src, flags=re.M)
    assert len(found) == 1, found
    assert int(found[0]) == slk.PREDICT_PAIR_MIN_BATCH
    assert slk.PREDICT_PAIR_MIN_BATCH >= 2
