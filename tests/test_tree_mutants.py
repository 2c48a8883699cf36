"""The tree cases are sharp: every rule of the refit, the Morton rebuild and the clustered rebuild that tests/tree_mutants.py breaks gives,
on some small case of tests/build_cases.py / tests/ploc_cases.py, a tree or a new_to_old other than the true restatement's — for every
operation the rule is part of. tests/test_build.py, tests/test_ploc.py and tests/test_refit.py hold the device to the true restatement's
bytes on these very cases, so a device library with one of these faults fails there. mesh20k does not count: a small scene must do.

The new cases themselves go through the checks of every case: they are in the tables tests/test_build_ref.py and tests/test_ploc_ref.py
are parametrised over."""
import numpy as np
import pytest

from tests import build_cases as BC
from tests import build_ref as BR
from tests import converter_ref as CR
from tests import ploc_cases as PC
from tests import ploc_ref as PR
from tests import refit_ref as RR
from tests import tree_mutants as TM

SMALL_PRIMS = 600


def small_cases(op):
    table = PC if op == TM.PLOC else BC
    return [n for n in table.SMALL if len(table.case(n)["prims"]) <= SMALL_PRIMS]


def run(op, name):
    """The bytes of what `op` makes of case `name` under the rules as they are patched now."""
    if op == TM.MORTON:
        out = BR.build(BC.case(name)["prims"])
    elif op == TM.PLOC:
        out = PR.build(PC.case(name)["prims"])
    else:
        cur, out = BC.case(name)["tree"], []
        for ordinals, payloads in BC.updates(name):
            cur = RR.refit(cur, ordinals, payloads)
            out.append(cur)
    return b"".join(np.ascontiguousarray(a).tobytes() for a in out)


_true = {}


def true_bytes(op, name):
    if (op, name) not in _true:
        _true[op, name] = run(op, name)
    return _true[op, name]


def killers(mutant, op):
    out = []
    for name in small_cases(op):
        exp = true_bytes(op, name)
        with mutant.apply():
            try:
                got = run(op, name)
            except (ValueError, AssertionError):   # no tree at all (more than 1024 iterations, say): noticed
                got = None
        if got != exp:
            out.append(name)
    return out


@pytest.mark.parametrize("which", sorted(TM.MUTANTS))
def test_a_small_case_notices_the_mutant(which):
    m = TM.MUTANTS[which]
    found = {op: killers(m, op) for op in m.ops}
    for op in m.ops:
        print("%s | %s | %s" % (which, op, ", ".join(found[op]) or "-"))
    assert all(found[op] for op in m.ops), {op: found[op] for op in m.ops if not found[op]}
    assert true_bytes(m.ops[0], "n5") == run(m.ops[0], "n5")   # the rule is back in place


@pytest.mark.parametrize("which", sorted(TM.EQUIVALENT))
def test_an_equivalent_mutant_is_noticed_by_no_case(which):
    """What the table in tests/tree_mutants.py argues, seen on the cases: were one of them to notice, the mutant belongs in MUTANTS."""
    m = TM.EQUIVALENT[which]
    assert len(TM.EQUIVALENT) <= 3 and not any(killers(m, op) for op in m.ops)


def test_the_mutants_are_those_of_the_list():
    assert len(TM.MUTANTS) == 24 and not set(TM.MUTANTS) & set(TM.EQUIVALENT)
    for must in ("ploc: distance flushed", "ploc: distance contracted", "key: reciprocal division", "key: no clamp",
                 "box: fold by fminf / fmaxf", "box: fold by <= / >="):
        assert must in TM.MUTANTS


def test_the_new_cases_are_small_and_in_every_table():
    """At most 64 primitives each, in the tables of both builds (tests/test_build_ref.py, tests/test_ploc_ref.py, tests/test_build.py
    and tests/test_ploc.py are parametrised over them) and of the device refit (tests/test_refit.py; read as text: importing a module
    of device tests is not for a CPU test)."""
    import os
    for name in BC.SHARP:
        assert name in BC.SMALL and name in PC.SMALL and len(BC.case(name)["prims"]) <= 64
    text = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "test_refit.py")).read()
    assert "BC.SHARP.items()" in text and "BC.updates(name)" in text
    assert set(BC.UPDATES) <= set(BC.SHARP)


def test_the_subnormal_cases_are_the_two_named():
    """tiny8 and denormal8 are the cases whose trees have planes below 2^-60, whichever build made them and after their update too;
    the uploader's slack for them is infinite."""
    from gpuart_amd import binding as B
    for name in BC.SMALL:
        c = BC.case(name)
        refitted = RR.refit(c["tree"], *BC.updates(name)[0])
        for tree in (c["tree"], c["built"], PC.case(name)["built"], refitted):
            assert CR.convert(tree)["subnormal"] == (name in BC.SUBNORMAL), name
            assert B.tree_slack(tree) == (np.inf, True) if name in BC.SUBNORMAL else not B.tree_slack(tree)[1]


def test_the_zeros_update_moves_a_plane_between_the_zeros():
    """zeros5's update: one point from +0 onto -0 at x and back — the second refit restores the tree, and the first one changes bytes
    that compare equal as numbers."""
    c = BC.case("zeros5")
    (o1, p1), (o2, p2) = BC.updates("zeros5")
    there = RR.refit(c["tree"], o1, p1)
    back = RR.refit(there, o2, p2)
    assert back.tobytes() == np.ascontiguousarray(c["tree"]).tobytes() and there.tobytes() != back.tobytes()
    with np.errstate(invalid="ignore"):
        assert ((there == back) | (np.isnan(there) & np.isnan(back))).all()
