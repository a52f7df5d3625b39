"""The twin of the search-value targets (include/agz_value_target.h, include/agz.h agz_replay_set_value_target, DESIGN.md
§5n): the definition restated in numpy float64 -- a loop over np.float64 scalars, each product and each sum an operation of
its own (numpy has no fused multiply-add), and one cast through np.float32 at the end; the two corners the definition
returns as they stand (alpha = 0: the result; alpha = 1, lambda = 0: q_t) are returned as they stand here too.  tests/test_value_target.py holds the
header to it on the CPU, tests/test_gpu_value_target.py the replay kernel, the ring and host entries and train().  Test
infrastructure only."""
import numpy as np

# the (alpha, lambda) pairs both test files run: q alone, z through the formula, the plain z/q mix, TD(0.9) alone, a mix of
# all three terms, and off
PAIRS = [(1.0, 0.0), (1.0, 1.0), (0.5, 0.0), (1.0, 0.9), (0.25, 0.5), (0.0, 0.3)]


def value_target(qs, t, result, alpha, lam):
    """y_t of the record (qs[0..T-1] float32, result) as np.float32"""
    qs = np.asarray(qs, np.float32)
    T = len(qs)
    assert 0 <= t < T
    alpha, lam, one = np.float64(alpha), np.float64(lam), np.float64(1.0)
    z = np.float64(int(result))
    if alpha == 0.0:                    # the two corners the definition returns as they stand
        return np.float32(int(result))
    if alpha == 1.0 and lam == 0.0:     # (the loop would give the same value, with a q_t of -0.0 turned into +0.0)
        return qs[t]
    acc = z
    for k in range(T - 1, t - 1, -1):
        a = (one - lam) * np.float64(qs[k])
        b = lam * acc
        acc = a + b
    c = (one - alpha) * z
    d = alpha * acc
    return np.float32(c + d)


def value_targets(qs, result, alpha, lam):
    """y_0 .. y_{T-1} as a float32 vector"""
    return np.array([value_target(qs, t, result, alpha, lam) for t in range(len(qs))], np.float32)


def bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)
