"""Child process of tests/test_gpu_sample_ahead.py: `sample_ahead_worker.py OUT.npz` runs the test's three clobbered steps in a fresh process —
the parent sets IVX_AHEAD_BLOCKS, which the library reads once — and writes what the last step left."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (os.path.dirname(HERE), HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import numpy as np

if __name__ == "__main__":
    from impact_amd.voxel import Context
    from test_gpu_sample_ahead import ahead_blocks_steps

    c = Context(0)
    try:
        np.savez(sys.argv[1], **ahead_blocks_steps(c)[2])
    finally:
        c.close()
