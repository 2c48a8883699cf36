"""NumPy float32 restatement of libgpuart_converge.so (include/gpuart_converge.h): the weighted batch-means update and the measure, every
operation in the header's order, so that the device's state, error map and summary can be compared bit for bit. It also keeps a
ledger of how often each branch of the measure is taken, so that a set of cases can be held to a floor."""
import numpy as np

from tests import denoise_ref

F = np.float32
MAX_PATHS = 1 << 24
LEDGER_KEYS = ("m2_pos", "m2_not_pos", "mean_above_floor", "mean_not_above_floor", "above", "not_above", "non_finite", "finite")


def new_ledger():
    return {k: 0 for k in LEDGER_KEYS}


def lum(a):
    """L(a) = (0.2126f*a.r + 0.7152f*a.g) + 0.0722f*a.b"""
    return denoise_ref.lum(np.asarray(a, F))


class Estimator:
    """The state of one handle. weighted=False is the variant that ignores the batch weight (every batch counts as one sample
    whatever its number of paths): what the tests show to be wrong for unequal batches."""

    def __init__(self, weighted=True):
        self.weighted = weighted
        self.reset()

    def reset(self):
        self.state = None   # (h, w, 4) float32 {mean, m2, prevL, 0}
        self.total = 0
        self.batches = 0

    def update(self, accum, paths_total):
        accum = np.asarray(accum, F)
        h, w = accum.shape[:2]
        if self.state is not None and self.state.shape[:2] != (h, w):
            raise ValueError("size")
        if paths_total <= self.total or paths_total > MAX_PATHS:
            raise ValueError("paths_total")
        if self.state is None:
            self.state = np.zeros((h, w, 4), F)
        b = F(paths_total - self.total)
        Wn = F(paths_total)
        r = b / Wn
        mean, m2, prevL = self.state[..., 0], self.state[..., 1], self.state[..., 2]
        with np.errstate(all="ignore"):
            Lk = lum(accum)
            y = (Lk - prevL) / b
            d = y - mean
            if self.weighted:
                mean1 = mean + r * d
                m21 = m2 + (b * d) * (y - mean1)
            else:
                mean1 = mean + (F(1) / F(self.batches + 1)) * d
                m21 = m2 + d * (y - mean1)
        self.state = np.stack([mean1, m21, Lk, np.zeros_like(Lk)], -1).astype(F)
        self.total = paths_total
        self.batches += 1
        return self.state

    def error(self, lum_floor, ledger=None):
        """e per pixel (h, w) float32."""
        if self.batches < 2:
            raise ValueError("a measure needs two batches")
        mean, m2 = self.state[..., 0], self.state[..., 1]
        lum_floor = F(lum_floor)
        with np.errstate(all="ignore"):
            v = np.where(m2 < 0, F(0), m2) / F(self.batches - 1)   # (a NaN m2 stays NaN)
            se = np.sqrt(v / F(self.total))
            e = se / np.where(mean > lum_floor, mean, lum_floor)
        assert e.dtype == F
        if ledger is not None:
            ledger["m2_pos"] += int((m2 > 0).sum())
            ledger["m2_not_pos"] += int((~(m2 > 0)).sum())
            ledger["mean_above_floor"] += int((mean > lum_floor).sum())
            ledger["mean_not_above_floor"] += int((~(mean > lum_floor)).sum())
        return e

    def measure(self, threshold, lum_floor, ledger=None):
        """(summary dict as binding.ConvergeSummary.as_dict, e)."""
        e = self.error(lum_floor, ledger)
        with np.errstate(all="ignore"):
            above = ~(e <= F(threshold))
        non_finite = ~np.isfinite(e)
        fin = e[~non_finite]
        if ledger is not None:
            ledger["above"] += int(above.sum())
            ledger["not_above"] += int((~above).sum())
            ledger["non_finite"] += int(non_finite.sum())
            ledger["finite"] += int((~non_finite).sum())
        return dict(pixels=e.size, above=int(above.sum()), non_finite=int(non_finite.sum()), max_error=float(fin.max()) if fin.size else 0.0,
                    batches=self.batches, total=self.total), e

    def variance(self):
        """m2 / (batches - 1) per pixel, in float64: the estimate of the per-path luminance variance."""
        return self.state[..., 1].astype(np.float64) / (self.batches - 1)


def reference64(lums, totals, lum_floor):
    """The same estimate in float64 and in another form: no recurrence, no running mean. lums: the luminance of the accumulator after
    every batch (any float type, any shape), totals: the path count after every batch. From the batch means y_k = (L_k - L_{k-1}) / b_k
    (L_0 = 0), two passes: mean = sum b_k y_k / sum b_k, m2 = sum b_k (y_k - mean)^2, e = sqrt(m2 / (nb - 1) / total) / max(mean, floor).
    Returns (e, mean, m2), float64."""
    nb = len(totals)
    if nb < 2 or len(lums) != nb:
        raise ValueError("a measure needs two batches")
    b = np.diff(np.concatenate([[0], np.asarray(totals, np.int64)])).astype(np.float64)
    if (b <= 0).any():
        raise ValueError("totals must rise")
    total = float(totals[-1])
    prev = np.zeros(np.shape(lums[0]), np.float64)
    ys = []
    for Lk, bk in zip(lums, b):
        Lk = np.asarray(Lk, np.float64)
        ys.append((Lk - prev) / bk)
        prev = Lk
    mean = sum(bk * y for bk, y in zip(b, ys)) / b.sum()
    m2 = sum(bk * (y - mean) ** 2 for bk, y in zip(b, ys))
    with np.errstate(all="ignore"):
        e = np.sqrt(m2 / (nb - 1) / total) / np.maximum(mean, float(lum_floor))
    return e, mean, m2


def lum64(a):
    """L of unrounded float64 sums: the fp32 coefficients, every operation in float64."""
    a = np.asarray(a, np.float64)
    return (float(F(0.2126)) * a[..., 0] + float(F(0.7152)) * a[..., 1]) + float(F(0.0722)) * a[..., 2]


def accumulator_floor(total, b_min):
    """What the fp32 accumulator alone can add to e (include/gpuart_converge.h, "The accumulator's floor"): every batch mean is a
    difference of two luminances that each carry a rounding error relative to the whole sum, spread over the batch's paths;
    2^-22 * sqrt(total / b_min) bounds the change of e for a pixel at or above lum_floor, b_min being the smallest batch after the first."""
    return 2.0 ** -22 * float(np.sqrt(float(total) / float(b_min)))


def batch_loop(rendered, cap, per_pass, batch_paths, seen, show, judge, render_pass=None):
    """The loop Renderer::RenderUntil and Renderer::RenderAdaptive share (Renderer::RenderBatches): `rendered` paths are in the accumulator,
    `cap` and `per_pass` are RestartPathTracing's. seen() is what the estimate has seen, (batches, total); show(rendered) gives it the
    accumulator as one more batch; judge() is asked from the second batch on and ends the loop when true; render_pass(rendered, n), if
    given, renders a pass of n paths. Paths the estimate has never seen are its first batch, of their own weight. Returns (whether
    judge ended the loop, paths rendered)."""
    per_pass = max(1, min(per_pass, cap))
    if seen()[0] == 0 and rendered > 0:
        show(rendered)
    while True:
        if rendered < cap:
            target = rendered + min(batch_paths, cap - rendered)
            while rendered < target:
                n = min(per_pass, cap - rendered)   # (a pass is clamped to the cap, not to the batch)
                if render_pass is not None:
                    render_pass(rendered, n)
                rendered += n
        if rendered > seen()[1]:
            show(rendered)
        if seen()[0] >= 2 and judge():
            return True, rendered
        if rendered >= cap:
            return False, rendered


def render_until(est, accum_at, rendered, cap, per_pass, batch_paths, threshold, max_above_share, lum_floor):
    """What one call of Renderer::RenderUntil does, on the Estimator `est` the earlier calls left (a reset one after anything that
    restarted the accumulation): `rendered` paths are in the accumulator, `cap` and `per_pass` are RestartPathTracing's, accum_at(total)
    is the raw accumulator after `total` paths. Returns (converged, the summary of the last measure or None, paths rendered)."""
    last = [None]

    def judge():
        last[0], _ = est.measure(threshold, lum_floor)
        return float(last[0]["above"]) <= float(F(max_above_share)) * float(last[0]["pixels"])

    converged, rendered = batch_loop(rendered, cap, per_pass, batch_paths, lambda: (est.batches, est.total),
                                     lambda total: est.update(accum_at(total), total), judge)
    return converged, last[0], rendered


def stops_at(accums, totals, threshold, max_above_share, lum_floor):
    """What Renderer::RenderUntil does with these accumulators, one per batch: (index of the batch after which it stops or None,
    the summary of its last measure or None)."""
    est = Estimator()
    s = None
    for k, (a, t) in enumerate(zip(accums, totals)):
        est.update(a, t)
        if est.batches >= 2:
            s, _ = est.measure(threshold, lum_floor)
            if float(s["above"]) <= float(F(max_above_share)) * float(s["pixels"]):
                return k, s
    return None, s
