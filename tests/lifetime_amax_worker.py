"""Child process of test_hip_lifetime.py::test_max_abs_slot_array_growth_refused_in_the_hooks_library (not a test module): run with
XSD_LIB = the hooks library and XSD_TEST_AMAX_CAP=128, so that the training plan of the 4-block net in f16x3 counts more max-|x| slots than are
allocated and ensure_plan (csrc/xsd_engine.hip) grows the slot array right after the workspace.  Sweeps the refusal over both allocations."""
import os
import sys

root = sys.argv[1]
for p in (root, os.path.join(root, "xmm-superres-denoise_amd"), os.path.join(root, "tests"), os.path.join(root, "tests", "golden")):
    sys.path.insert(0, p)

import test_hip_lifetime as T  # noqa: E402

assert b"test-hooks" in T._L().xsd_version(), T._L().xsd_version()
fam = T._rrdb("dn", 1, 1, 32, 0, "f16x3", blocks=4)
T.sweep_growth(fam, None, fam.small, expect=1)                # a forward-only plan: the workspace alone (its slots fit the 128)
N = T.sweep_growth(fam, None, fam.small, run=fam.train, expect=2)      # a training plan: the workspace, then the slot array
print(f"slot array sweep OK: N = {N}")
