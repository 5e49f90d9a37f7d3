"""Records `callers_platform.npz`: sha256 digests of `tests/test_reference_callers.py::platform_probe`'s outputs.

Run it ONLY on a host where the restated callers (`opt_plumbing.SeaOPTDecoderLayer`) reproduce every array of
`callers.npz` bit for bit:

    python tests/golden/make_golden_platform.py

The digests then name that host's fp32 CPU rounding; tests/test_reference_callers.py holds a host that reproduces them to
bit equality with the reference callers' outputs.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))

from test_reference_callers import PROBE, platform_digests  # noqa: E402

if __name__ == "__main__":
    d = platform_digests()
    np.savez(PROBE, **{k: np.array(v) for k, v in d.items()})
    print(f"wrote {PROBE}: {len(d)} digests")
