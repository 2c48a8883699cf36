"""NumPy float32 restatement of libgpuart_adaptive.so (include/gpuart_adaptive.h) and of Renderer::RenderAdaptive's loop: the
convergence estimate kept per 8x8 block, the block rule and the normalisation by per-block path counts. The update and e are not
written again here: every group of blocks that shares (seen, paths) — or (batches, seen) — is handed to tests/converge_ref.py's
Estimator with those totals, so the formulas compared bit for bit with the device are the ones libgpuart_converge.so is held to."""
import numpy as np

from tests import converge_ref

F = np.float32
MAX_PATHS = converge_ref.MAX_PATHS


def block_grid(h, w):
    """(rows of blocks, blocks per row)."""
    return (h + 7) // 8, (w + 7) // 8


def pixel_blocks(h, w):
    """(h, w) array: the row-major index of every pixel's 8x8 block."""
    _, bw = block_grid(h, w)
    return (np.arange(h)[:, None] // 8) * bw + np.arange(w)[None, :] // 8


def block_mask(h, w, blocks):
    """(h, w) bool: the pixels of the listed blocks."""
    bh, bw = block_grid(h, w)
    listed = np.zeros(bh * bw, bool)
    listed[np.asarray(blocks, np.int64)] = True
    return listed[pixel_blocks(h, w)]


def block_pixels(h, w):
    """Pixels inside the image of every block (ragged edges)."""
    return np.bincount(pixel_blocks(h, w).ravel(), minlength=block_grid(h, w)[0] * block_grid(h, w)[1])


def normalize(accum, paths):
    """accum.rgb / float(paths[block] or 1), alpha copied."""
    accum = np.asarray(accum, F)
    h, w = accum.shape[:2]
    p = np.asarray(paths, np.uint32).reshape(-1)
    d = np.where(p == 0, 1, p).astype(F)[pixel_blocks(h, w)]
    out = accum.copy()
    out[..., :3] = accum[..., :3] / d[..., None]
    return out


class Estimator:
    """The state of one handle: `state` (h, w, 4) {mean, m2, prevL, 0}; per block seen, batches, active."""

    def __init__(self):
        self.reset()

    def reset(self):
        self.state = None
        self.seen = self.batches = self.active = None
        self.updates = 0   # update calls since the reset: what RenderAdaptive counts as batches

    def block_state(self):
        return np.stack([self.seen, self.batches, self.active.astype(np.uint32), np.zeros_like(self.seen)], -1).astype(np.uint32)

    def update(self, accum, paths):
        accum = np.asarray(accum, F)
        h, w = accum.shape[:2]
        paths = np.asarray(paths, np.int64).reshape(-1)
        nb = block_grid(h, w)[0] * block_grid(h, w)[1]
        if paths.size != nb or (self.state is not None and self.state.shape[:2] != (h, w)):
            raise ValueError("size")
        seen = np.zeros(nb, np.int64) if self.state is None else self.seen.astype(np.int64)
        if (paths > MAX_PATHS).any() or (paths < seen).any():
            raise ValueError("block_paths")
        if self.state is None:
            self.state = np.zeros((h, w, 4), F)
            self.seen, self.batches, self.active = np.zeros(nb, np.uint32), np.zeros(nb, np.uint32), np.ones(nb, bool)
        pb = pixel_blocks(h, w)
        moved = paths != seen
        new = self.state.copy()
        for s, p in sorted(set(zip(seen[moved].tolist(), paths[moved].tolist()))):
            one = converge_ref.Estimator()
            one.state, one.total, one.batches = self.state, s, 1    # (batches: the weighted update does not read it)
            sel = (moved & (seen == s) & (paths == p))[pb]
            new[sel] = one.update(accum, p)[sel]
        self.state = new
        self.seen = paths.astype(np.uint32)
        self.batches = self.batches + moved.astype(np.uint32)
        self.updates += 1
        return self.state

    def error(self, lum_floor):
        """e per pixel (h, w) float32; +inf where the block has fewer than two batches."""
        h, w = self.state.shape[:2]
        pb = pixel_blocks(h, w)
        e = np.full((h, w), np.inf, F)
        ok = self.batches >= 2
        for nbt, s in sorted(set(zip(self.batches[ok].tolist(), self.seen[ok].tolist()))):
            one = converge_ref.Estimator()
            one.state, one.total, one.batches = self.state, s, nbt
            sel = (ok & (self.batches == nbt) & (self.seen == s))[pb]
            e[sel] = one.error(lum_floor)[sel]
        return e

    def select(self, threshold, lum_floor, min_paths, e=None):
        """(ascending list of the blocks that stay active, summary dict as binding.AdaptiveSummary.as_dict, e). `e`: an error map to judge
        instead of the state's own (the block rule alone)."""
        h, w = self.state.shape[:2]
        if e is None:
            e = self.error(lum_floor)
        with np.errstate(all="ignore"):
            above = ~(e <= F(threshold))
        non_finite = ~np.isfinite(e)
        nb = self.seen.size
        any_above = np.bincount(pixel_blocks(h, w).ravel(), weights=above.ravel(), minlength=nb) > 0
        self.active = self.active & ((self.seen < min_paths) | (self.batches < 2) | any_above)
        blocks = np.nonzero(self.active)[0].astype(np.uint32)
        fin = e[~non_finite]
        s = dict(pixels=h * w, above=int(above.sum()), non_finite=int(non_finite.sum()),
                 paths_sum=int((block_pixels(h, w).astype(np.int64) * self.seen.astype(np.int64)).sum()), blocks=nb, active_blocks=int(blocks.size),
                 paths_min=int(self.seen.min()), paths_max=int(self.seen.max()), max_error=float(fin.max()) if fin.size else 0.0)
        return blocks, s, e


def render_adaptive(est, pass_colour, accum, counts, issued, cap, per_pass, batch_paths, threshold, min_paths, lum_floor, active=None):
    """What one call of Renderer::RenderAdaptive does on the Estimator `est` (a reset one after anything that restarted the accumulation).
    accum (h, w, 4) and counts (one per block) are what the accumulator holds, `issued` the paths issued so far (the largest count),
    pass_colour(k, n) the colour image (h, w, 4; alpha ignored) of the pass that starts at issued path k with n paths per pixel: a
    listed pass adds it, in fp32, to the pixels of the listed blocks. Returns (1 converged / 0 at the cap, summary of the last select or
    None, accum, counts, issued, active list)."""
    h, w = np.shape(accum)[:2]
    st = dict(accum=np.array(accum, F), counts=np.array(counts, np.int64).reshape(-1), summary=None)
    st["active"] = np.arange(st["counts"].size) if active is None else active

    def render_pass(k, n):
        if len(st["active"]):
            m = block_mask(h, w, st["active"])
            new = st["accum"].copy()
            new[..., :3] = st["accum"][..., :3] + np.asarray(pass_colour(k, n), F)[..., :3]
            st["accum"] = np.where(m[..., None], new, st["accum"])
            st["counts"][np.asarray(st["active"], np.int64)] += n

    def judge():
        st["active"], st["summary"], _ = est.select(threshold, lum_floor, min_paths)
        return not len(st["active"])

    # (the loop is the uniform estimate's, tests/converge_ref.py batch_loop: the batches are the update calls, the total the largest count)
    converged, issued = converge_ref.batch_loop(issued, cap, per_pass, batch_paths,
                                                lambda: (est.updates, int(est.seen.max()) if est.state is not None else 0),
                                                lambda total: est.update(st["accum"], st["counts"]), judge, render_pass)
    return int(converged), st["summary"], st["accum"], st["counts"], issued, st["active"]
