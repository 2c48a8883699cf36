"""Inputs of tests/test_converter.py: hand-assembled canonical trees, the table of minimal rejections, the seeded mutants, the big tree.

Trees are assembled from root-leaf pieces (compile_bvh with one level: the honest encoding and box of a few primitives) by the layout rule
of the reference's CompileFrom (src/bvh.cpp): node, lower subtree, upper subtree, contiguously; an interior box is the union of its children's.
"""
import functools

import numpy as np

from gpuart_amd import binding as B
from gpuart_amd import synth_scenes as S

LEAF, IS_LOWER, IS_ROOT = 1 << 31, 1 << 30, 1 << 29

SPH = (S.SPHERE, [0.25, 0.5, 0.75, 0.125])
SPH2 = (S.SPHERE, [-0.5, 0.25, 0.5, 0.25])
DSC = (S.DISC, [0.5, -0.25, 0.25, 0.0, 0.0, 1.0, 0.375])
TRI = (S.TRIANGLE, [0.0, 0.0, 0.5, 1.0, 0.0, 0.25, 0.0, 1.0, 0.75])
TRI2 = (S.TRIANGLE, [-1.0, 0.5, 0.25, -0.5, 1.0, 0.5, -0.75, 0.25, 1.0])
TRI3 = (S.TRIANGLE, [0.5, 0.5, 0.5, 0.75, 0.5, 0.5, 0.5, 0.75, 1.0])
CON = (S.CONE, [0.5, -0.75, 0.0, 0.5, -0.75, 0.375, 0.25, 0.125])


def piece(*descs):
    """A root leaf holding the primitives, as the host library compiles it."""
    tree, _ = B.compile_bvh(list(descs), max_levels=1)
    assert tree.view(np.uint32)[2, 0] & LEAF
    return tree


def assemble(node):
    """node: a piece, or (lower, upper) of nodes. -> (n, 4) float32 canonical tree."""
    out = []

    def emit(node, parent, flags):
        addr = len(out)
        if isinstance(node, np.ndarray):
            p = node.copy()
            u = p.view(np.uint32)
            u[2, 0] = (u[2, 0] & ~np.uint32(IS_LOWER | IS_ROOT)) | np.uint32(flags)
            u[2, 3] = parent
            out.extend(p)
            return p[0, :3], p[1, :3]
        out.extend(np.zeros((3, 4), np.float32))
        lmin, lmax = emit(node[0], addr, IS_LOWER)
        hi = len(out)
        hmin, hmax = emit(node[1], addr, 0)
        bmin, bmax = np.minimum(lmin, hmin), np.maximum(lmax, hmax)
        out[addr][:3], out[addr + 1][:3] = bmin, bmax
        out[addr + 2].view(np.uint32)[:] = (flags, addr + 3, hi, parent)
        return bmin, bmax

    emit(node, 0, IS_ROOT)
    return np.array(out, np.float32)


def chain(levels):
    """A hand-written chain: `levels` interior nodes, each with a one-sphere leaf below and the next link above, a leaf at the end — the
    deepest node lies at level `levels`."""
    leaf = piece(SPH)
    n = 8 * levels + 5
    t = np.zeros((n, 4), np.float32)
    u = t.view(np.uint32)
    for i in range(levels):
        a = 8 * i
        t[a, :3], t[a + 1, :3] = leaf[0, :3], leaf[1, :3]
        u[a + 2] = ((IS_ROOT if i == 0 else 0), a + 3, a + 8, max(a - 8, 0))
        t[a + 3:a + 8] = leaf
        u[a + 5, 0] |= IS_LOWER; u[a + 5, 0] &= ~np.uint32(IS_ROOT); u[a + 5, 3] = a
    t[n - 5:] = leaf
    u[n - 3, 0] &= ~np.uint32(IS_ROOT); u[n - 3, 3] = n - 13
    return t


@functools.lru_cache(None)
def small_trees():
    """The three trees the mutants are made of: a root leaf, the 19-quad two-leaf tree, a three-level mixed tree."""
    root_leaf = piece(SPH, TRI, DSC)
    two_leaf = assemble((piece(SPH), piece(TRI, TRI2)))
    assert len(two_leaf) == 19
    mixed = assemble(((piece(SPH, TRI), (piece(CON), piece(DSC, SPH2))), (piece(TRI, TRI2, TRI3), piece(TRI3))))
    return root_leaf, two_leaf, mixed


def rejections():
    """One minimal mutation per message: name -> (tree, nquads, message). All but the chain are edits of the 19-quad tree: the root at 0, a
    one-sphere leaf at 3, a two-triangle leaf at 8 (its primitives' headers at 11 and 15)."""
    base = small_trees()[1]

    def edit(quad, word, value):
        t = base.copy()
        t.view(np.uint32)[quad, word] = value
        return t

    return {
        "root cut off": (base, 2, "node address out of range"),
        "chain of 1025 levels": (chain(1025), None, "tree deeper than 1024 levels"),
        "a count of three in a leaf of two": (edit(10, 0, LEAF | 3), None, "primitive header out of range"),
        "type 4": (edit(11, 0, 4), None, "unknown primitive type"),
        "last data quad cut off": (base, 18, "primitive data out of range"),
        "lower child one quad late": (edit(2, 1, 4), None, "lower child does not follow its parent"),
        "upper child at nquads": (edit(2, 2, 19), None, "upper child address out of range"),
        "upper child not above the lower": (edit(2, 2, 3), None, "upper child address out of range"),
        "upper child one quad late": (edit(2, 2, 9), None, "upper child does not start where the lower subtree ends"),
        "upper child inside the lower subtree": (edit(2, 2, 5), None, "upper child does not start where the lower subtree ends"),
    }


NOT_REACHED = {"too many primitives", "too many nodes"}   # the two capacity limits: tens of millions of entries

N_MUTANTS = 20000
MUTANT_SEED = 20240


def mutants(n=N_MUTANTS, seed=MUTANT_SEED):
    """Yields (tree, nquads): one or two words of one of small_trees() replaced; one mutant in eight is also told of fewer quads than it has.
    Half of the words are drawn from all words, half from those that look like an integer (addresses, counts, types, flag words — and zero pads)."""
    rs = np.random.RandomState(seed)
    trees = small_trees()
    looks_int = []
    for t in trees:
        u = t.view(np.uint32).reshape(-1)
        looks_int.append(np.flatnonzero(((u & 0x1fffffff) < 65536)))
    for i in range(n):
        k = i % 3
        t = trees[k].copy()
        u = t.view(np.uint32).reshape(-1)
        nq = len(t)
        for _ in range(int(rs.randint(1, 3))):
            w = int(rs.randint(u.size)) if rs.rand() < 0.5 else int(looks_int[k][rs.randint(len(looks_int[k]))])
            kind = int(rs.randint(9))
            small = int(rs.randint(1, 9))
            u[w] = (0, small, nq - 1, nq, nq + 1, LEAF | int(rs.randint(0, 6)), LEAF | int(rs.choice([1000, 0x1fffffff, nq])), 0xffffffff,
                    int(u[w]) ^ (1 << int(rs.randint(32))))[kind]
        cut = int(rs.randint(1, nq)) if rs.randint(8) == 0 else nq
        yield t, cut


@functools.lru_cache(None)
def big_tree():
    """110 000 small primitives of all four types in [-1, 1]^2 x [0, 2]: a node table of at least 8 x 16384 entries, so that the fill pass
    really runs on up to eight threads."""
    rs = np.random.RandomState(7)
    n = 110000
    c = rs.uniform(-1, 1, (n, 3)).astype(np.float32); c[:, 2] += 1
    kind = rs.randint(0, 8, n)
    r = rs.uniform(0.002, 0.01, n).astype(np.float32)
    off = rs.uniform(-0.01, 0.01, (n, 6)).astype(np.float32)
    prims = []
    for i in range(n):
        x, y, z = (float(v) for v in c[i])
        if kind[i] < 3:
            prims.append((S.SPHERE, [x, y, z, float(r[i])]))
        elif kind[i] < 6:
            o = off[i]
            prims.append((S.TRIANGLE, [x, y, z, float(c[i, 0] + o[0]), float(c[i, 1] + o[1]), float(c[i, 2] + o[2]),
                                       float(c[i, 0] + o[3]), float(c[i, 1] + o[4]), float(c[i, 2] + o[5])]))
        elif kind[i] == 6:
            prims.append((S.DISC, [x, y, z, 0.0, 0.0, 1.0, float(r[i])]))
        else:
            prims.append((S.CONE, [x, y, z, x, y, float(c[i, 2] + np.float32(0.02)), float(r[i]), float(r[i] * np.float32(0.5))]))
    prims.append((S.DISC, [0, 0, 0, 0, 0, 1, 6]))
    tree, _ = B.compile_bvh(prims)
    return tree


if __name__ == "__main__":   # python -m tests.converter_cases: what the restatement makes of the mutant set (profiles/converter.txt)
    from tests import converter_ref as R
    counts = {}
    for tree, nq in mutants():
        v = R.verdict(tree, nq)
        counts[v] = counts.get(v, 0) + 1
    print("mutants (seed %d): %d, accepted %d = %.1f %%" % (MUTANT_SEED, N_MUTANTS, counts[None], 100.0 * counts[None] / N_MUTANTS))
    for v in sorted(k for k in counts if k):
        print("  %6d  %s" % (counts[v], v))
