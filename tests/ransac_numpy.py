"""What the restatements of the RANSAC solvers (tests/sim3_numpy.py, tests/pnp_numpy.py) share: glibc's rand() restated in Python
integers, a solver's samples drawn from it, and the end of SetRansacParameters."""
import math

import numpy as np

INT_MIN = -2147483648


# ------------------------------------------------------------------------------------------------------------------------------
# rand()
class GlibcRand:
    """glibc random_r TYPE_3: r[i] = r[i - 31] + r[i - 3] mod 2^32, output >> 1, seeded through the 16807 Lehmer step, 310
    outputs discarded"""

    def __init__(self, seed):
        seed = int(seed) & 0xFFFFFFFF
        w = seed if seed else 1
        if w >= 1 << 31:
            w -= 1 << 32
        r = [w & 0xFFFFFFFF]
        for _ in range(1, 31):
            hi, lo = int(w / 127773), int(math.fmod(w, 127773))      # C division truncates
            w = 16807 * lo - 2836 * hi
            if w < 0:
                w += 2147483647
            r.append(w & 0xFFFFFFFF)
        for i in range(31, 34):
            r.append(r[i - 31])
        for i in range(34, 344):
            r.append((r[i - 31] + r[i - 3]) & 0xFFFFFFFF)
        self.r = r

    def rand(self):
        v = (self.r[-31] + self.r[-3]) & 0xFFFFFFFF
        self.r.append(v)
        del self.r[0]
        return v >> 1

    def random_int(self, lo, hi):
        """DUtils::Random::RandomInt"""
        d = hi - lo + 1
        return int((float(self.rand()) / (2147483647.0 + 1.0)) * d) + lo


def sample_sets(seed, N, rows, k):
    """k distinct correspondences a row, each row from the full list of N"""
    rng = GlibcRand(seed)
    out = np.zeros((rows, k), np.int32)
    for h in range(rows):
        avail = list(range(N))
        for q in range(k):
            r = rng.random_int(0, len(avail) - 1)
            out[h, q] = avail[r]
            avail[r] = avail[-1]
            avail.pop()
    return out


# ------------------------------------------------------------------------------------------------------------------------------
# SetRansacParameters
def _clog(x):
    if x != x or x < 0:
        return math.nan
    return -math.inf if x == 0 else math.log(x)


def trunc32(v):
    """the int conversion of a NaN or an out-of-range float is INT_MIN"""
    v = float(v)
    return int(v) if (v == v and -2147483648.0 <= v < 2147483648.0) else INT_MIN


def iteration_count(single, eps, probability, max_iterations):
    """the clamped mRansacMaxIts from the float32 epsilon; single: mRansacMinInliers == N.  The cube of a float32 is finite in
    double, so math.pow does not raise."""
    if single:
        n_it = 1
    else:
        a, b = _clog(1 - float(probability)), _clog(1 - math.pow(float(eps), 3.0))
        with np.errstate(all="ignore"):
            v = float(np.ceil(np.float64(a) / np.float64(b)))
        n_it = trunc32(v)
    return max(1, min(n_it, int(max_iterations)))
