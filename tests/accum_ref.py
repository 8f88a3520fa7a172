"""A numpy reference of the accumulator (include/frt_device.h "Accumulator"), written from its definition and not from
the C pass, and the seeded samples the accumulator tests share.

Vectorised over pixels, one sample at a time; every ufunc call is one IEEE binary64 operation per element, nothing is
fused or reordered.
"""
import numpy as np


class Welford:
    def __init__(self, npixels):
        self.n = np.zeros(npixels, dtype=np.int32)
        self.mean = np.zeros((npixels, 4))
        self.m2 = np.zeros((npixels, 3))
        self.skipped = 0

    def add(self, x):
        x = np.asarray(x, dtype=np.float64).reshape(-1, 4)
        take = np.isfinite(x).all(axis=1)
        self.skipped += int((~take).sum())
        with np.errstate(all="ignore"):
            n = self.n + 1
            dn = n.astype(np.float64)[:, None]
            d = x - self.mean
            mean = self.mean + d / dn
            m2 = self.m2 + d[:, :3] * (x[:, :3] - mean[:, :3])
        self.n = np.where(take, n, self.n).astype(np.int32)
        self.mean = np.where(take[:, None], mean, self.mean)
        self.m2 = np.where(take[:, None], m2, self.m2)

    def resolve(self):
        """(mean (npixels, 4), var (npixels, 4))"""
        n = self.n
        mean = np.where((n == 0)[:, None], 0.0, self.mean)
        var = np.zeros((n.size, 4))
        with np.errstate(all="ignore"):
            nm1 = (n - 1).astype(np.float64)[:, None]
            v = (self.m2 / nm1) / n.astype(np.float64)[:, None]
        var[:, :3] = np.where((n < 2)[:, None], 0.0, v)
        var[:, 3] = n.astype(np.float64)
        return mean, var


def samples(npixels, count, seed):
    """`count` seeded samples of npixels x 4 in [0, 2). Where there is room, pixel 0 is never finite (n == 0), pixel 1
    is finite in sample 0 alone (n == 1), and a few other (sample, pixel) pairs hold a NaN or an infinity in one
    channel, the alpha included."""
    rng = np.random.default_rng(seed)
    out = rng.uniform(0.0, 2.0, (count, npixels, 4))
    if npixels >= 8:
        out[:, 0, rng.integers(0, 4)] = np.nan
        out[1:, 1, 2] = -np.inf
        for k in range(count):
            a, b = rng.choice(np.arange(2, npixels), 2, replace=False)
            out[k, a, rng.integers(0, 4)] = np.nan
            out[k, b, 3] = np.inf
    return out
