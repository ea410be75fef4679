"""numpy f64 restatement of the noise estimator with per-pixel sample counts and of the adaptive loop
(include/pt/pt.h, "adaptive sampling"): every operation is one IEEE f64 operation, in the header's order, so the
kernels must agree with it in every bit.  With no pixel frozen it is noise_ref.NoiseRef bit for bit.

    est = AdaptiveRef(n_start, mean_at_n_start)       # mean: (..., 3) float64
    est.update(samples, counts, mean)                  # samples: the active pixels' count; counts: every pixel's
    est.rel2(y_floor), est.summary(tol, y_floor), est.converged(tol, y_floor)
    simulate(render, shape, ...)                       # the loop of pt_accum_add_adaptive over render(n) images
"""
import numpy as np

import noise_ref
from noise_ref import TOL, Y_FLOOR

# the loop case of tests/test_adaptive_host.py (its input condition, from the oracle) and tests/test_gpu_adaptive.py:
# cornell_blob, both integrators
LOOP = dict(pass_spp=4, cap=32, tol=0.2, quantile=1.0, min_batches=2)
LOOP_SHAPES = [(24, 16), (20, 13)]
SEED, BOUNCES = 1234, 3


class AdaptiveRef:
    def __init__(self, n_start=0, mean=None, shape=None):
        if mean is None:
            mean = np.zeros(tuple(shape) + (3,), dtype=np.float64)
        assert mean.dtype == np.float64 and mean.shape[-1] == 3
        self.prev = mean.copy()
        self.n0 = int(n_start)                                     # the scalar count at the last fold
        self.batches = 0                                           # the active pixels' batch count (the summary's)
        self.Wq = np.zeros(mean.shape[:-1], dtype=np.uint32)       # per pixel: window weight
        self.bq = np.zeros(mean.shape[:-1], dtype=np.uint32)       # per pixel: batches folded
        self.mu = np.zeros(mean.shape[:-1], dtype=np.float64)
        self.m2 = np.zeros(mean.shape[:-1], dtype=np.float64)

    def update(self, samples, counts, mean):
        """Fold at n1 = samples > n0: pixel q folds iff counts[q] > n0, with its own s = counts[q] - n0."""
        n1 = int(samples)
        counts = np.asarray(counts)
        assert mean.dtype == np.float64 and mean.shape == self.prev.shape and counts.shape == self.mu.shape
        assert n1 >= self.n0 and int(counts.max(initial=0)) <= n1
        if n1 == self.n0:
            return False
        fold = counts > self.n0
        nq = counts.astype(np.float64)
        n0 = float(self.n0)
        with np.errstate(all="ignore"):                            # (pixels that do not fold: s <= 0, discarded)
            s = nq - n0
            b = (mean * nq[..., None] - self.prev * n0) / s[..., None]
            y = (0.2126 * b[..., 0] + 0.7152 * b[..., 1]) + 0.0722 * b[..., 2]
            Wn = self.Wq.astype(np.float64) + s
            d = y - self.mu
            mu = self.mu + d * (s / Wn)
            m2 = self.m2 + (s * d) * (y - mu)
        self.mu = np.where(fold, mu, self.mu)
        self.m2 = np.where(fold, m2, self.m2)
        self.prev = np.where(fold[..., None], mean, self.prev)
        self.Wq = np.where(fold, self.Wq + (counts - self.n0).astype(np.uint32), self.Wq).astype(np.uint32)
        self.bq = np.where(fold, self.bq + np.uint32(1), self.bq).astype(np.uint32)
        self.n0 = n1
        self.batches += 1
        return True

    def rel2(self, y_floor=Y_FLOOR):
        """f64 rel2 of every pixel (+inf before the pixel's second batch)."""
        with np.errstate(all="ignore"):
            var = self.m2 / ((self.bq.astype(np.float64) - 1.0) * self.Wq.astype(np.float64))
            yf = np.float64(np.float32(y_floor))
            den = np.where(self.mu > yf, self.mu, yf)
            return np.where(self.bq < 2, np.inf, var / (den * den))

    def error_map(self, y_floor=Y_FLOOR):
        with np.errstate(all="ignore"):
            return self.rel2(y_floor).astype(np.float32)

    def converged(self, tol=TOL, y_floor=Y_FLOOR):
        """The pixels with rel2 <= tol*tol (the summary's count, and what pt_noise_freeze freezes among the active)."""
        t = np.float64(np.float32(tol))
        with np.errstate(all="ignore"):
            return self.rel2(y_floor) <= t * t

    def summary(self, tol=TOL, y_floor=Y_FLOOR, mask=None):
        r2 = self.rel2(y_floor)
        if mask is None:
            mask = np.ones(r2.shape, dtype=bool)
        conv = self.converged(tol, y_floor)[mask]
        with np.errstate(all="ignore"):
            hist = np.bincount(noise_ref.bins(r2[mask].astype(np.float32)), minlength=64)
        return dict(batches=self.batches, pixels=int(conv.size), converged=int(np.count_nonzero(conv)),
                    hist=[int(v) for v in hist])


def compose(render, counts):
    """The image whose pixel p is render(counts[p])[p] (0 at count 0): what an accumulator with these counts holds."""
    counts = np.asarray(counts)
    out = np.zeros(counts.shape + (3,), dtype=np.float64)
    for n in np.unique(counts):
        if n:
            out[counts == n] = render(int(n))[counts == n]
    return out


def simulate(render, shape, pass_spp, cap, tol, quantile=1.0, min_batches=2, y_floor=Y_FLOOR, mask=None):
    """pt_accum_add_adaptive from 0 samples over render(n) -> the (shape, 3) f64 image after n samples of every pixel.
    mask: the pixels of the accumulator's shard (default: all); the others are never sampled and count for nothing.
    Returns dict(counts, samples_total, passes, stopped_converged, active, est, summary)."""
    est = AdaptiveRef(0, shape=shape)
    mine = np.ones(shape, dtype=bool) if mask is None else np.asarray(mask, dtype=bool)
    frozen = ~mine
    counts = np.zeros(shape, dtype=np.uint32)
    samples, passes, stopped, summary = 0, 0, False, None
    while samples < cap and not frozen.all():
        samples += min(pass_spp, cap - samples)
        counts[~frozen] = samples
        est.update(samples, counts, compose(render, counts))
        passes += 1
        summary = est.summary(tol, y_floor, mine)
        if summary["batches"] < min_batches:
            continue
        frozen |= est.converged(tol, y_floor) & mine
        if frozen.all() or summary["converged"] >= int(np.ceil(np.float64(np.float32(quantile)) * summary["pixels"])):
            stopped = True
            break
    return dict(counts=counts, samples_total=int(counts.sum(dtype=np.uint64)), passes=passes, stopped_converged=stopped,
                active=int((~frozen).sum()), est=est, summary=summary)
