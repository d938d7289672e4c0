"""CPU restatement of dvmvs::gp_filter_step (csrc/gp_filter.hip) in numpy float64: one step of GP-MVS's Kalman filter over the
columns of the [2, N] state mean, as the reference's gpmvs/run-testing.py:185-193 does it for all N = 512 * 8 * 10 columns.
Columns are independent, so a subset of columns (the pinned ones of tests/golden/baselines_e2e.npz) can be advanced on its own."""
import numpy as np


def gp_filter_step(state, y, A, k, reset):
    """Returns (new state [2, n] float64, Z [n] float32).  ``A`` row-major [4] or [2,2], ``k`` [2]; ``reset`` starts from zero."""
    A = np.asarray(A, dtype=np.float64).reshape(2, 2)
    k = np.asarray(k, dtype=np.float64).reshape(2, 1)
    M = np.zeros_like(state) if reset else np.asarray(state, dtype=np.float64)
    M = A.dot(M)
    v = np.asarray(y, dtype=np.float32).astype(np.float64)[None, :] - M[0:1]
    M = M + k.dot(v)
    return M, np.maximum(M[0].astype(np.float32), np.float32(0.0))
