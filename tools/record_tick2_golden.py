"""Write the bit-level fixtures of a tick2 case module under tests/: tests/golden/<prefix>_<case>.npz, the results of the module's
run_case on the library that is loaded.  Case modules: tick2_ow_cases (tests/test_gpu_tick2_owner_waves.py, the default) and
tick2_loops_cases (tests/test_gpu_tick2_loops.py).  Run once on the GPU against a library built from the commit the fixtures are to
pin - never from the code under test:

    DUST_AMD_LIB=/path/to/that/commit's/libdust_amd.so python tools/record_tick2_golden.py [--cases MODULE] [case ...]

Every case is run twice and written only if the two runs agree bit for bit and went through tick2.hpp without a replay."""
import importlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np

args = sys.argv[1:]
module = "tick2_ow_cases"
if args[:1] == ["--cases"]:
    module, args = args[1], args[2:]
cases = importlib.import_module(module)

names = args or list(cases.CASES)
os.makedirs(cases.GOLDEN, exist_ok=True)
for name in names:
    out, stats = cases.run_case(name)
    again, _ = cases.run_case(name)
    assert stats["tick2"] == cases.tick2_launches(name) and stats["replayed"] == 0, (name, stats)
    assert out.keys() == again.keys() and all(np.array_equal(out[k], again[k]) for k in out), name
    assert all(np.isfinite(v).all() for v in out.values()), name
    np.savez_compressed(cases.golden_path(name), **out)
    print("%-36s %3d arrays  %7d bytes  %s" % (name, len(out), os.path.getsize(cases.golden_path(name)), stats), flush=True)
