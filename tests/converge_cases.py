"""The case table of tests/test_converge_range.py: seeded accumulators of long renders (thousands to 2^24 paths per pixel), built as
float64 cumulative sums and rounded to fp32 once per batch, and two deliberately wrong variants of the restatement."""
import numpy as np

from tests import converge_ref as R

F = np.float32
LUM_FLOOR = 1.0 / 256
MEANS = (1e-4, 0.01, 1.0, 300.0)     # mean luminance per path; 1e-4 is below the floor
CVS = (0.0, 0.05, 1.0)               # per-path standard deviation over the mean
COMBOS = [(m, cv, col) for m in MEANS for cv in CVS for col in (False, True)]   # pixel i is COMBOS[i % 24]


def repeat_to(unit, end):
    """`unit` over and over until the path count is `end`; the last batch is cut to end there."""
    out, total = [], 0
    while total < end:
        b = min(unit[len(out) % len(unit)], end - total)
        out.append(b)
        total += b
    return out


PATTERNS = {
    "64x64": [64] * 64,
    "4096x64": [64] * 4096,
    "2^23+64x1": [1 << 23] + [1] * 64,
    "2^23+64x64": [1 << 23] + [64] * 64,
    "256x65536": [65536] * 256,              # ends exactly at 2^24
    "unequal": repeat_to([100, 3, 1, 7], 1 << 16),
}
assert sum(PATTERNS["256x65536"]) == R.MAX_PATHS


def b_min(sizes):
    """The smallest batch after the first."""
    return min(sizes[1:])


def batches(sizes, n, seed, copies=()):
    """Yields (acc32, sum64, total) per batch for n pixels: acc32 (n, 4) float32, the accumulator as the renderer would hold it had it
    summed without error and rounded once; sum64 (n, 3) the unrounded sums. A batch's sum per channel is a Gamma variate, the exact
    law of a sum of b independent Gamma paths of the pixel's mean and cv (never negative); cv 0 is the plain product. A grey pixel
    has three equal channels; a coloured one has its own channel weights (luminance still the pixel's mean) and independent channels.
    copies: (targets, source) index pairs: the target pixels are copies of the source (the planted groups of the device test)."""
    rng = np.random.default_rng(seed)
    mean = np.array([COMBOS[i % len(COMBOS)][0] for i in range(n)])
    cv = np.array([COMBOS[i % len(COMBOS)][1] for i in range(n)])
    col = np.array([COMBOS[i % len(COMBOS)][2] for i in range(n)])
    wts = rng.uniform(0.2, 1.8, (n, 3))
    wts /= R.lum64(wts)[:, None]                      # L(weights) = 1
    wts[~col] = 1.0 / R.lum64(np.ones(3))
    mu = mean[:, None] * wts                          # per-path mean per channel
    noisy = cv > 0
    shape1 = 1.0 / np.where(noisy, cv, 1.0) ** 2      # Gamma shape of one path
    scale = mu * np.where(noisy, cv, 1.0)[:, None] ** 2
    s64 = np.zeros((n, 3))
    total = 0
    for b in sizes:
        g = rng.standard_gamma((b * shape1)[:, None] * np.ones(3))
        g[~col] = g[~col][:, :1]
        step = np.where(noisy[:, None], g * scale, b * mu)
        for targets, source in copies:
            step[targets] = step[source]
        s64 = s64 + step
        total += b
        acc = np.zeros((n, 4), F)
        acc[:, :3] = s64.astype(F)
        acc[:, 3] = F(total)
        yield acc, s64, total


class Mutant(R.Estimator):
    """Two ways to get the update subtly wrong that agree with the right one for equal batches of a steady pixel:
    "prev_mean": prevL kept in the state as a rounded mean (L / total) instead of the sum, and scaled back for the difference;
    "r_batches": r = 1 / batches instead of b / total."""

    def __init__(self, kind):
        super().__init__()
        self.kind = kind

    def update(self, accum, paths_total):
        accum = np.asarray(accum, F)
        if self.state is None:
            self.state = np.zeros(accum.shape[:2] + (4,), F)
        b, Wn, Wp = F(paths_total - self.total), F(paths_total), F(self.total)
        r = b / Wn if self.kind == "prev_mean" else F(1) / F(self.batches + 1)
        mean, m2, prev = self.state[..., 0], self.state[..., 1], self.state[..., 2]
        with np.errstate(all="ignore"):
            Lk = R.lum(accum)
            prevL = prev * Wp if self.kind == "prev_mean" else prev
            y = (Lk - prevL) / b
            d = y - mean
            mean1 = mean + r * d
            m21 = m2 + (b * d) * (y - mean1)
            keep = Lk / Wn if self.kind == "prev_mean" else Lk
        self.state = np.stack([mean1, m21, keep, np.zeros_like(Lk)], -1).astype(F)
        self.total = paths_total
        self.batches += 1
        return self.state
