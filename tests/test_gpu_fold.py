"""GPU: k_fold_r2 entered directly (sbmp_fold_r2_batch runs it through the planner's own launcher)
on every case of tests/fold_cases.py, against the numpy model (tests/fold_model.py) and against
the host twin (include/sbmp/r2_fold.h): R2Valid and R2Invalid equal element for element, no
tolerance.  A second call on the same tables must add the same counts again, and P ranks folded
into one table pair must give the single-rank fold of the global log.

What the cases reach in the kernel: a packed LDS half-word at its largest value, 65,280, in
either half (counter-*); the 8-key piece that straddles S at every offset, at a block border and
at the borders of the three ragged workgroups of a 131,072-key row, which lie inside a 256-slot
block (S-*); one to three workgroups per iteration (groups-*); histograms of fewer cells than
threads, of one flush round and one cell more, either side of the 64 KB dynamic-LDS opt-in and
at the largest nR2 (hist-*); the sink words (dropped-keys); ring rows that wrap, with stale
in-grid keys at and past every S and unexecuted iterations (window-*); the rank term of the
slot (ranks-*).
"""
import numpy as np
import pytest

import fold_cases as fc
from fold_cases import model, same, twin

pytestmark = pytest.mark.gpu


def device(c, **kw):
    from cudasbmp_amd import fold_r2_batch
    v, i = c.tables()
    kw.setdefault("R2Valid", v)
    kw.setdefault("R2Invalid", i)
    return fold_r2_batch(c.ring(), c.S, c.executed, c.tFirst, c.nR2, rank=c.rank, nranks=c.nranks, device=True, **kw)


def assert_tables(got, want, what):
    for g, w, table in zip(got, want, ("R2Valid", "R2Invalid")):
        g, w = np.asarray(g, dtype=np.int64), np.asarray(w, dtype=np.int64)
        bad = np.flatnonzero(g != w)
        assert bad.size == 0, (f"{what}: {table} differs at {bad.size} cells, first {bad[:8]}: "
                               f"kernel {g[bad[:8]]}, expected {w[bad[:8]]}")


@pytest.mark.parametrize("name", [c.name for c in fc.CASES])
def test_kernel_equals_model_and_twin(name):
    c = fc.BY_NAME[name]
    got = device(c)
    assert got[0].dtype == np.int32 and got[0].shape == (c.nR2,)
    assert_tables(got, model(name), f"{name} against the model")
    assert_tables(got, twin(name), f"{name} against the twin")


# a table past 2^31 - 1 is outside the rule: the cases that end exactly there fold once
@pytest.mark.parametrize("name", [c.name for c in fc.CASES if not c.name.endswith("-priorbig")])
def test_second_call_adds_the_same_counts_again(name):
    c = fc.BY_NAME[name]
    prior = [t.astype(np.int64) for t in c.tables()]
    once = model(name)
    assert_tables(device(c, repeat=2), [2 * a - p for a, p in zip(once, prior)], f"{name} twice")


@pytest.mark.parametrize("P", sorted(fc.RANK_GROUPS))
def test_rank_folds_add_up_to_the_global_fold(P):
    g, ranks = fc.RANK_GROUPS[P]
    v, i = g.tables()
    for c in ranks:
        v, i = device(c, R2Valid=v, R2Invalid=i)
    assert_tables((v, i), model(g.name), f"the sum of {P} ranks")
    assert same(device(g), model(g.name))
