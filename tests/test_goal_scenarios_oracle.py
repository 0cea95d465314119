"""Family I (tests/goal_scenarios.py) through the CPU oracle alone: the independent float32
model of the goal verdict against the oracle's own goal code, case by case and exactly, and
every coverage condition the cases claim -- the relation each disc has by its records' slots,
at least two candidates and no lower row inside, the winner's scan wave, the rank layout of
the sharded discs, the FMA-sensitivity of the verdict targets and how near a rounding
midpoint their square roots lie, that the D6 and D13 clamps bind in the logged iteration --
so that a change of seed, RNG or search fails here and not on the GPU.

A failure of the model against the oracle is a bug in one of the two; the GPU module
(tests/test_gpu_goal_scenarios.py) holds the HIP planner against both.
"""
import functools
from fractions import Fraction

import numpy as np
import pytest

from conftest import bits
from goal_scenarios import (BIG, CAPACITY_IDS, D6, D6_PARTIAL, D13, GROUPED, INSERT_IDS, KINDS, NOWHERE, S16, SHAPES,
                            THRESHOLD_IDS, TINY, VARIANTS, VERDICTS, capacity_cases, chain, cut_iteration, disc_params,
                            discs, distance, fl32, fused_distance, insert_cases, insert_inputs, midpoint_gap, model, pass0,
                            relation, scenario, threshold_cases, units, verdict)
from scenarios import make_oracle

F32 = np.float32
VERDICT_IDS = [f"{s}-it{it}" for s, it in VERDICTS]
DISC_PARAMS = disc_params()
DISC_IDS = [f"{s}-{n}" for s, n in DISC_PARAMS]
MIDPOINT_GAP = 1e-2     # ulps: how near a rounding midpoint a verdict target's exact sqrt(d2) must lie


@functools.lru_cache(maxsize=24)
def oracle_run(shape, goal, thr, limit=None):
    """The planned oracle of one case; read only."""
    return make_oracle(scenario(shape, goal, thr, limit))


def check_oracle(shape, goal, thr, limit=None):
    """The oracle's result and tree against the model on pass 0; returns the model's record."""
    p, e, o = pass0(shape), model(shape, goal, thr, limit), oracle_run(shape, goal, thr, limit)
    info = o.info()
    got = (info["goalIdx"], info["iterations"], info["treeSize"], int(F32(info["costToGoal"]).view(np.uint32)))
    assert got == (e.goalIndex, e.iterations, e.treeSize, e.cost_bits), f"oracle {got}, model {e}"
    s, par, c = o.tree()
    n = min(info["treeSize"], p.M)
    assert np.array_equal(bits(s[:n]), bits(p.samples[:n])) and np.array_equal(par[:n], p.parents[:n])
    assert np.array_equal(bits(c[:n]), bits(p.costs[:n])), "the run's rows are pass 0's, bit for bit"
    assert np.array_equal(o.iter_logs()[:, :8], p.logs[:e.iterations, :8])
    if e.goalIndex >= 0:
        assert e.path[0] == 0 and e.path[-1] == e.goalIndex and e.goalIndex < n
        assert o.iter_logs()[-1, 8] == e.goalIndex
    return e


@pytest.mark.parametrize("shape", SHAPES, ids=[s.name for s in SHAPES])
def test_pass0_rows(shape, oracle_lib):
    """The flagged children in slot order are the rows: row treeSizeBefore + j holds record j."""
    p = pass0(shape)
    assert np.array_equal(bits(p.samples[p.row, 0]), bits(p.x)) and np.array_equal(bits(p.samples[p.row, 1]), bits(p.y))
    assert len(p.row) == min(p.end[1], p.M) - 1 - (7 if shape in (D6, D6_PARTIAL) else 0)   # D6: 993 .. 999
    assert (np.diff(p.row) > 0).all() and (p.parents[p.row] < p.row).all() and (p.parents[p.row] >= 0).all()
    for k, i in enumerate(p.iters):
        assert (np.diff(i.slots) > 0).all() and i.ts + i.A == p.logs[k, 7]
    assert model(shape, NOWHERE, 1.0).goalIndex == -1
    check_oracle(shape, NOWHERE, 1.0)


# ---------------------------------------------------------------- I-verdict
@pytest.mark.parametrize("shape,it", VERDICTS, ids=VERDICT_IDS)
def test_verdict_target(shape, it, oracle_lib):
    p, v = pass0(shape), verdict(shape, it)
    k = int(np.nonzero(p.row == v.row)[0][0])
    x, y = p.x[k], p.y[k]
    assert p.it[k] == it == v.it and p.slot[k] == v.slot
    d = distance([x], [y], v.goal)[0]
    assert bits(d) == bits(F32(v.d)) and d > 0
    # FMA-sensitive, in exact arithmetic: the fused d2 rounds once, and its square root is another float
    dx, dy = F32(x) - F32(v.goal[0]), F32(y) - F32(v.goal[1])
    exact = Fraction(float(dx)) ** 2 + Fraction(float(F32(dy * dy)))
    unfused = F32(F32(dx * dx) + F32(dy * dy))
    assert abs(Fraction(float(fl32(exact))) - exact) <= abs(Fraction(float(unfused)) - exact) and fl32(exact) != unfused
    fused = fused_distance(x, y, v.goal)
    assert fused != d and fused == np.sqrt(fl32(exact), dtype=F32)
    gap = midpoint_gap(x, y, v.goal)
    print(f"{shape}-it{it}: row {v.row} slot {v.slot} d {float(d)!r} fused {float(fused)!r} "
          f"exact sqrt {gap:.3g} ulp from a rounding midpoint")
    assert 0 <= gap < MIDPOINT_GAP
    # nobody else within up(d) while the target's iteration lasts: the three thresholds decide on the target alone
    seen = np.nonzero((p.it <= it) & (p.row != v.row))[0]
    assert (distance(p.x[seen], p.y[seen], v.goal) > np.nextafter(d, F32(np.inf))).all()
    b = int(d.view(np.uint32))
    assert [int(F32(v.thr(k)).view(np.uint32)) for k in VARIANTS] == [b, b + 1, b - 1]
    if it > 1:   # many parents: the compacted-list parent path
        rows = p.row[p.it == it]
        assert len(set(p.parents[rows].tolist())) > 100 and p.parents[v.row] != 0
    else:
        assert p.parents[v.row] == 0


@pytest.mark.parametrize("shape,it", VERDICTS, ids=VERDICT_IDS)
def test_verdict_triple(shape, it, oracle_lib):
    v = verdict(shape, it)
    e_at, e_in, e_out = (check_oracle(shape, v.goal, v.thr(k)) for k in VARIANTS)
    assert e_in.goalIndex == v.row and e_in.iterations == it and e_in.path[-1] == v.row
    assert e_at == e_out and e_at.goalIndex != v.row
    assert e_at.iterations > it or (e_at.goalIndex == -1 and it == shape.passes)


@pytest.mark.parametrize("shape,it", VERDICTS[:2], ids=VERDICT_IDS[:2])
def test_iteration_limit(shape, it, oracle_lib):
    v = verdict(shape, it)
    last = check_oracle(shape, v.goal, v.thr("in"), limit=it)
    assert (last.goalIndex, last.iterations) == (v.row, it), "the row of the run's last iteration still ends it"
    short = check_oracle(shape, v.goal, v.thr("in"), limit=it - 1)
    assert (short.goalIndex, short.iterations) == (-1, it - 1), "the child is never created"


# ---------------------------------------------------------------- I-lowest
@pytest.mark.parametrize("shape,name", DISC_PARAMS, ids=DISC_IDS)
def test_disc(shape, name, oracle_lib):
    p, d = pass0(shape), discs(shape)[name]
    assert d.thr == shape.radius and len(d.rows) >= 2 and list(d.rows) == sorted(d.rows)
    # the candidates are all the rows inside, and all of iteration 1: no lower row, the lowest wins
    inside = np.nonzero(distance(p.x, p.y, d.goal) < F32(d.thr))[0]
    first = inside[p.it[inside] == 1]
    assert tuple(p.row[first]) == d.rows and tuple(p.slot[first]) == d.slots
    assert p.row[inside[0]] == d.rows[0] and p.it[inside[0]] == 1
    e = check_oracle(shape, d.goal, d.thr)
    assert (e.goalIndex, e.iterations) == (d.rows[0], 1)
    # the relation the disc claims, from the records' slots
    w, others = d.slots[0], d.slots[1:]
    assert all(s > w for s in others)
    assert KINDS[shape][name](w, others)
    rel = {relation(w, s) for s in others}
    uw = units(w)
    flagged = np.zeros(int(p.logs[0, 5]) // 256 + 1, dtype=np.int64)
    np.add.at(flagged, p.iters[0].slots // 256, 1)
    if name in ("lanes", "waves", "blocks", "threads"):
        assert name in rel
    elif name.startswith("scan-waves"):
        assert "scan-waves" in rel and uw["scan_wave"] == int(name[-1]) and int(p.logs[0, 5]) == 1024 * 256
    elif name == "threads-w3":
        assert "threads" in rel and uw["scan_wave"] == 3 and all(units(s)["scan_wave"] == 3 for s in others)
    elif name == "other-block":
        assert any(units(s)["block"] != uw["block"] for s in others) and int(p.logs[0, 5]) == 1025 * 256
    elif name == "last-block":
        assert uw["block"] < 1024 and max(units(s)["block"] for s in others) == 1024 == int(p.logs[0, 5] - 1) // 256
    elif name.startswith("P"):
        P = int(name[1])
        u = units(w, P)
        mates = [units(s, P) for s in others if units(s, P)["block_row"] == u["block_row"]]
        if name == "P2-rows":
            assert len(mates) < len(others)
        else:
            assert mates and u["rank"] == (0 if name == "P2-row-r0r1" else 1)
            later = 1 if name == "P2-row-r1" else u["rank"] + 1    # a group of 2 has no rank past 1
            assert any(m["rank"] == later for m in mates)
            # the ranks before the winner in its row hold flagged children: the walk adds their counts
            assert all(flagged[u["block_row"] * P + q] > 0 for q in range(u["rank"]))


def test_discs_cover_every_level(oracle_lib):
    assert set(discs(S16)) == set(KINDS[S16]) and set(discs(BIG)) == set(KINDS[BIG])
    winners = {units(d.slots[0])["scan_wave"] for d in discs(BIG).values()}
    assert winners == {0, 1, 2, 3}, "each scan wave holds the winner at least once"
    # one radius per shape, so one batch can carry the shape's discs as members
    assert len({d.thr for d in discs(S16).values()}) == 1


# ---------------------------------------------------------------- I-capacity
@pytest.mark.parametrize("k", range(len(CAPACITY_IDS)), ids=CAPACITY_IDS)
def test_capacity(k, oracle_lib):
    c = capacity_cases()[k]
    assert c.name == CAPACITY_IDS[k]
    p = pass0(c.shape)
    i = p.iters[c.it - 1]
    e = check_oracle(c.shape, c.goal, c.thr)
    assert c.thr == TINY and distance([i.xy[c.j, 0]], [i.xy[c.j, 1]], c.goal)[0] == 0
    assert bool(i.inserted[c.j]) == c.inserted and (c.j == 0 or bool(i.inserted[c.j - 1]))
    if c.shape is D13:
        # the capacity clamp binds in the logged iteration (the grid limit does not), and the tree ends full
        assert c.it == cut_iteration(D13) and i.ts < p.M < i.ts + i.A and i.nIns == i.A
        assert p.end == (c.it, i.ts + i.A) and c.j == p.M - i.ts - (1 if c.inserted else 0)
    else:
        # the grid limit binds: 999 flagged, 992 inserted, rows 993 .. 999 never written, the tree ends full
        assert (i.A, i.nIns, i.ts, p.M) == (999, 992, 1, 1000) and p.end == (1, 1000)
        assert c.j == i.nIns - (1 if c.inserted else 0)
    if c.row is not None:
        assert e.goalIndex == c.row
        assert (e.iterations, e.treeSize) == (c.it, i.ts + i.A), "found or not, the plan ends there with a full tree"
    else:
        assert 0 < e.goalIndex < i.ts and e.iterations < c.it
        assert bits(p.samples[e.goalIndex, :2]).tolist() == bits(F32(c.goal)).tolist()


def test_a_child_past_capacity_lies_on_a_lower_row(oracle_lib):
    """Why family I has no "goal on the first child capacity keeps out, not found": that child lies
    past the iteration's own batch, so it was inserted before (D6) and a lower row holds its float."""
    p = pass0(D13)
    i = p.iters[cut_iteration(D13) - 1]
    S = int(p.logs[cut_iteration(D13) - 1, 5])
    rows = {(int(a), int(b)) for a, b in bits(p.samples[1:i.ts, :2])}
    out = np.nonzero(~i.inserted)[0]
    assert len(out) and (i.slots[out] >= S).all() and S <= p.M - i.ts
    assert all((int(a), int(b)) in rows for a, b in bits(i.xy[out]))
    last = p.M - i.ts - 1   # while the last row takes a child of the batch itself, on nobody's float
    assert i.slots[last] < S and tuple(int(v) for v in bits(i.xy[last])) not in rows


# ---------------------------------------------------------------- I-threshold
@pytest.mark.parametrize("k", range(len(THRESHOLD_IDS)), ids=THRESHOLD_IDS)
def test_threshold(k, oracle_lib):
    name, goal, thr = threshold_cases()[k]
    assert name == THRESHOLD_IDS[k]
    e = check_oracle(S16, goal, thr)
    if name in ("zero", "minus-zero", "minus-one", "nan", "root-subnormal"):
        assert (e.goalIndex, e.iterations) == (-1, S16.passes)
    elif name == "inf":
        assert (e.goalIndex, e.iterations) == (1, 1)
    else:   # the goal on the root's own float: row 0 lies inside and is never tested
        assert distance([S16.initial[0]], [S16.initial[1]], goal)[0] == 0 and e.goalIndex > 0


# ---------------------------------------------------------------- updateG over a batch (the checker of sbmp_insert_batch)
def check_insert(shape, goal, thr, got):
    """One insert_batch result against the model: rows, inserted count and the goal row."""
    p = pass0(shape)
    samples, parent, costs, gnew, A, goal_row = got
    i = p.iters[0]
    e = model(shape, goal, thr, limit=1)
    assert (A, goal_row) == (i.A, e.goalIndex)
    n = 1 + int(i.inserted.sum())
    assert np.array_equal(bits(samples[:n]), bits(p.samples[:n])) and np.array_equal(parent[:n], p.parents[:n])
    assert np.array_equal(bits(costs[:n]), bits(p.costs[:n])) and not bits(samples[n:]).any()


@pytest.mark.parametrize("k", range(len(INSERT_IDS)), ids=INSERT_IDS)
def test_insert_batch_restatement(k, oracle_lib):
    from oracle.pyoracle import insert_batch
    name, shape, goal, thr = insert_cases()[k]
    assert name == INSERT_IDS[k]
    fix = bool(dict(fixGNewClear=True, **shape.kw)["fixGNewClear"])
    check_insert(shape, goal, thr, insert_batch(*insert_inputs(shape), goal, thr, fix))


def test_chain_is_the_parent_walk(oracle_lib):
    p, v = pass0(S16), verdict(S16, 3)
    path = chain(p, v.row)
    assert path[0] == 0 and path[-1] == v.row and len(path) == 4
    assert all(p.parents[b] == a for a, b in zip(path, path[1:]))
