"""numpy f64 restatement of the noise estimator's arithmetic (include/pt/pt.h, pt_noise_*): every operation is
one IEEE f64 operation, in the header's order, so the kernels must agree with it in every bit.

    est = NoiseRef(n_start, mean_at_n_start)      # mean: (..., 3) float64
    est.update(samples, mean)                      # a snapshot after a pass; no fold when samples is unchanged
    est.rel2(y_floor), est.summary(tol, y_floor)
"""
import numpy as np

TOL, Y_FLOOR = np.float32(0.05), np.float32(0.01)   # pt_noise_defaults


class NoiseRef:
    def __init__(self, n_start=0, mean=None, shape=None):
        if mean is None:
            mean = np.zeros(tuple(shape) + (3,), dtype=np.float64)
        assert mean.dtype == np.float64 and mean.shape[-1] == 3
        self.prev = mean.copy()
        self.n0 = int(n_start)
        self.W = 0.0
        self.batches = 0
        self.mu = np.zeros(mean.shape[:-1], dtype=np.float64)
        self.m2 = np.zeros(mean.shape[:-1], dtype=np.float64)

    def update(self, samples, mean):
        n1 = int(samples)
        assert mean.dtype == np.float64 and mean.shape == self.prev.shape and n1 >= self.n0
        if n1 == self.n0:
            return False
        s = float(n1 - self.n0)
        b = (mean * float(n1) - self.prev * float(self.n0)) / s
        y = (0.2126 * b[..., 0] + 0.7152 * b[..., 1]) + 0.0722 * b[..., 2]
        Wn = self.W + s
        d = y - self.mu
        self.mu = self.mu + d * (s / Wn)
        self.m2 = self.m2 + (s * d) * (y - self.mu)
        self.prev = mean.copy()
        self.W, self.n0 = Wn, n1
        self.batches += 1
        return True

    def rel2(self, y_floor=Y_FLOOR):
        """f64 rel2 of every pixel (+inf before two batches)."""
        if self.batches < 2:
            return np.full(self.mu.shape, np.inf)
        with np.errstate(all="ignore"):
            var = self.m2 / (float(self.batches - 1) * self.W)
            yf = np.float64(np.float32(y_floor))
            den = np.where(self.mu > yf, self.mu, yf)          # max(y_floor, mu) = mu > y_floor ? mu : y_floor
            return var / (den * den)

    def error_map(self, y_floor=Y_FLOOR):
        with np.errstate(all="ignore"):
            return self.rel2(y_floor).astype(np.float32)

    def summary(self, tol=TOL, y_floor=Y_FLOOR, mask=None):
        """dict(batches, pixels, converged, hist[64]) over the pixels of `mask` (default: all)."""
        r2 = self.rel2(y_floor)
        if mask is None:
            mask = np.ones(r2.shape, dtype=bool)
        r2 = r2[mask]
        t = np.float64(np.float32(tol))
        with np.errstate(all="ignore"):
            converged = int(np.count_nonzero(r2 <= t * t))     # (NaN and inf compare false)
            hist = np.bincount(bins(r2.astype(np.float32)), minlength=64)
        return dict(batches=self.batches, pixels=int(r2.size), converged=converged, hist=[int(v) for v in hist])


def bins(r):
    """The histogram bin of each float32 r, tested in the header's order."""
    r = np.ascontiguousarray(r, dtype=np.float32)
    bits = r.view(np.uint32)
    with np.errstate(all="ignore"):
        e = np.clip(((bits >> 23) & 255).astype(np.int64) - 127 + 48, 1, 62)
        out = np.where(r != r, 63, np.where(~(r > 0), 0, np.where(np.isinf(r), 63, e)))
    return out.astype(np.int64).reshape(-1)
