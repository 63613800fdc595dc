"""Generate tests/golden/resample.npz from the *imported reference* ``brever.io.resample``.

Runs only where the reference checkout is mounted (``BREVER_REFERENCE``, as for make_golden_mixture.py); nothing of the
reference is copied -- the fixture holds seeded inputs and recorded outputs. ``brever.io`` imports ``sofa`` and
``soundfile``, absent here and not part of the arithmetic: empty stand-ins go into ``sys.modules`` before the import.

    python tests/golden/make_golden_resample.py

Recorded per case ``<N>_<old_fs>_<new_fs>_<channels>`` of ``resample_ref.GOLDEN_CASES`` (the small ones; the large
cases of the GPU tests are checked against the NumPy restatement, which tests/test_resample_host.py pins to this
fixture and to scipy):
  x_<case>     the input, on the int16 grid as a decoded 16-bit WAV is (``resample_ref.case_input``)
  y_<case>     ``brever.io.resample(x, old_fs, new_fs)``, float64
and for every case of ``resample_ref.CASES``, the large ones included:
  yard_<case>  rel-L2 error of ``resample_ref.bluestein`` (the kernels' algorithm in NumPy complex128) against the
               case's reference: the yardstick the GPU value test scales its bound from (8 times it);
               tests/test_resample_host.py measures it again and prints it.
"""
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [HERE, os.path.dirname(HERE)]

import resample_ref as R  # noqa: E402
from make_golden_mixture import REF  # noqa: E402


def load_reference():
    for name in ('sofa', 'soundfile'):
        sys.modules.setdefault(name, types.ModuleType(name))
    sys.path.insert(0, REF)
    import brever.io
    return brever.io


def main():
    ref = load_reference()
    out = {}
    for case in R.GOLDEN_CASES:
        x = R.case_input(case)
        out['x_' + R.case_key(case)] = x
        out['y_' + R.case_key(case)] = np.asarray(ref.resample(x, case[1], case[2]), dtype=np.float64)
    np.savez_compressed(R.GOLDEN, **out)
    R.golden.cache_clear()
    for case in R.CASES:
        out['yard_' + R.case_key(case)] = np.float64(R.yardstick(case))
        print(case, out['yard_' + R.case_key(case)])
    np.savez_compressed(R.GOLDEN, **out)
    print(R.GOLDEN, os.path.getsize(R.GOLDEN), 'bytes')


if __name__ == '__main__':
    main()
