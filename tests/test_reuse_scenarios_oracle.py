"""Every sequence of tests/reuse_scenarios.py through the CPU oracle alone: for every pair
(P, Q) of consecutive plans on one handle, fresh oracle runs of P and Q must show that P
leaves behind something Q is sensitive to -- the conditions the table claims for the pair --
so that a sequence which stops dirtying its successor's state fails here, without a GPU,
instead of silently testing nothing on the GPU.

    rows>        P's treeSize > Q's: Q's tree lies on stale rows
    slots>       P's largest S > Q's: stale unexplored slots and R2 keys past Q's S
    iterations>  P executed more iterations than Q: stale ctrl blocks and key-log entries
    cells>       P touched an R1 cell Q never touches, or P's R2Valid / R2Invalid is nonzero
                 where Q's is zero
    form         the obstacle form, the box count, the NaN flag or the step form differs
    parity       the executed iteration counts differ in parity (the odd / even buffers)
    rows<, slots<, iterations<, cells<   the same with P and Q exchanged: Q must also run
                 past everything its short predecessor wrote

These are conditions on the inputs (properties of the oracle's runs), not tolerances.
"""
import numpy as np
import pytest

import reuse_scenarios as rs
from reuse_scenarios import BATCHES, CONDITIONS, IDS, LOG, SEQUENCES, oracle_run

# What the building blocks were measured to do at the DEMO configuration (the figures the
# sequences were designed round): (iterations, treeSize, largest S)
MEASURED = {
    "LONG-free": (100, 29969, 23712),
    "LONG-demo": (100, 29960, 22360),
    "SHORT": (1, 32, 32),
    "DEMO": (15, 27436, None),
    "LDS-600": (100, 29210, None),
    "GRID-3000": (100, 29625, 26400),
    "GRID-2100": (100, 29336, 28100),
}


def stats(seq, i, plan=None):
    """What one plan of a sequence leaves behind, from a fresh oracle run of it alone."""
    plan = seq.plans[i] if plan is None else plan
    o = oracle_run(seq, plan, threads=16 if seq.config()[0]["maxTreeSize"] > rs.CACHE_ROWS else 8)
    log, info, reg = o.iter_logs(), o.info(), o.regions()
    return dict(rows=info["treeSize"], slots=int(log[:, LOG["S"]].max()) if len(log) else 0,
                iterations=len(log), r1=reg["R1"] > 0, r2=(reg["R2Valid"] > 0) | (reg["R2Invalid"] > 0),
                form=(plan.obstacle_form, len(plan.obstacles()), plan.nan, seq.step_form(i or 0)),
                log=log, valid=int(reg["R1Valid"].sum()), invalid=int(reg["R1Invalid"].sum()))


def holds(cond, p, q):
    if cond.endswith("<"):
        return holds(cond[:-1] + ">", q, p)
    if cond == "rows>":
        return p["rows"] > q["rows"]
    if cond == "slots>":
        return p["slots"] > q["slots"]
    if cond == "iterations>":
        return p["iterations"] > q["iterations"]
    if cond == "cells>":
        return bool((p["r1"] & ~q["r1"]).any() or (p["r2"] & ~q["r2"]).any())
    if cond == "form":
        return p["form"] != q["form"]
    if cond == "parity":
        return (p["iterations"] - q["iterations"]) % 2 == 1
    raise AssertionError(f"unknown condition {cond!r}")


def describe(p, q):
    return (f"rows {p['rows']} / {q['rows']}, S {p['slots']} / {q['slots']}, iterations {p['iterations']} / "
            f"{q['iterations']}, R1 cells {int(p['r1'].sum())} / {int(q['r1'].sum())}, form {p['form']} / {q['form']}")


@pytest.mark.parametrize("seq", SEQUENCES, ids=IDS)
def test_each_predecessor_dirties_its_successor(seq, oracle_lib):
    for i, claim in enumerate(seq.claims):
        p, q = stats(seq, i), stats(seq, i + 1)
        tags = f"{seq.name}: {seq.plans[i].tag} -> {seq.plans[i + 1].tag}"
        assert len(claim) >= 1, f"{tags} claims nothing"
        for cond in claim:
            assert cond in CONDITIONS, cond
            assert holds(cond, p, q), f"{tags} claims {cond}: {describe(p, q)}"


@pytest.mark.parametrize("seq", SEQUENCES, ids=IDS)
def test_no_plan_is_the_same_whatever_the_state(seq, oracle_lib):
    """Accepted and rejected children in one iteration, and valid and invalid children: a plan
    without them computes the same whatever the region tables and the accept words hold.  The
    one exception is S2's list with an all-NaN box, there for the obsNaN flag and the slow car
    loop it switches on: the reference's predicate meets that box everywhere, so every child is
    invalid and the plan stalls at its root (the table lists it under `stalls`)."""
    for i, plan in enumerate(seq.plans):
        s = stats(seq, i)
        if plan.tag in seq.stalls:
            assert s["rows"] == 1 and s["invalid"] > 0, f"{plan.tag} was to stall: {s['rows']} rows"
            continue
        S, A = s["log"][:, LOG["S"]], s["log"][:, LOG["A"]]
        assert ((A > 0) & (A < S)).any(), f"{seq.name} {plan.tag}: no iteration accepts some children and rejects others"
        assert s["valid"] > 0 and s["invalid"] > 0, f"{seq.name} {plan.tag}: valid {s['valid']}, invalid {s['invalid']}"


def test_every_condition_is_claimed_in_each_direction():
    claimed = {c for seq in SEQUENCES for claim in seq.claims for c in claim}
    assert claimed == set(CONDITIONS), sorted(set(CONDITIONS) - claimed)


def test_building_blocks_measure_as_designed(oracle_lib):
    s1 = next(s for s in SEQUENCES if s.name == "S1-long-short-long")
    s2 = next(s for s in SEQUENCES if s.name == "S2-every-obstacle-form")
    seen = {}
    for seq in (s1, s2):
        for i, plan in enumerate(seq.plans):
            seen[plan.tag] = stats(seq, i)
    for tag, (iters, rows, slots) in MEASURED.items():
        s = seen[tag]
        assert (s["iterations"], s["rows"]) == (iters, rows), f"{tag}: {s['iterations']} iterations, {s['rows']} rows"
        assert slots is None or s["slots"] == slots, f"{tag}: largest S {s['slots']}"
    assert int(seen["LONG-free"]["r1"].sum()) == 256 and int(seen["SHORT"]["r1"].sum()) == 5
    tiny = next(s for s in SEQUENCES if s.name == "S10-tiny")
    t = stats(tiny, 0)
    assert t["iterations"] == 50 and t["log"][:3, LOG["S"]].tolist() == [32, 640, 0], t["log"][:4]   # the k = 0 path
    assert t["rows"] == 402, t["rows"]
    assert (t["log"][:, LOG["k"]] == 0).any()


def test_shorter_grid_list_has_another_resolution():
    """GRID-2100 lives in the buffers GRID-3000 grew: its cell-start table must be of another
    size, so that a stale gridG or a stale tail of the table would be read."""
    from cudasbmp_amd import _native as nat
    from test_obstacle_grid import grid_free
    seg = np.array([[1.0, 1.0, 2.0, 2.0]], dtype=np.float32)
    (_, g3000), (_, g2100) = grid_free(nat, rs.grid_3000(), seg), grid_free(nat, rs.grid_2100(), seg)
    assert 1 < g2100 < g3000, (g3000, g2100)   # the resolution the planner picks (sbmp_obstacle_grid_query, g = 0)


def test_batch_rows_are_whole():
    for b in BATCHES:
        for row in b.plans:
            tag, boxes, form, roots, goals, seeds = row
            assert len(roots) == len(goals) == len(seeds) == b.count, (b.name, tag)
            assert len(set(zip(roots, seeds))) == b.count, "members differ in root or seed"
    # consecutive batch plans change the obstacle form (the packing depends on it)
    for b in BATCHES:
        forms = [r[2] for r in b.plans]
        assert all(x != y for x, y in zip(forms, forms[1:])), forms


@pytest.mark.parametrize("bs", BATCHES, ids=rs.BATCH_IDS)
def test_batch_members_dirty_their_successors(bs, oracle_lib):
    """S12: every member's consecutive plans through the oracle, as the single-handle sequences:
    the conditions the table claims for a pair of rows hold for every member, and every member
    plan has accepted and rejected, valid and invalid children (a root inside a box would not)."""
    seq = bs.member_sequence()
    assert len(bs.claims) == len(bs.plans) - 1
    for m in range(bs.count):
        st = [stats(seq, None, bs.member_plan(row, m)) for row in bs.plans]
        for row, s in zip(bs.plans, st):
            S, A = s["log"][:, LOG["S"]], s["log"][:, LOG["A"]]
            assert ((A > 0) & (A < S)).any() and s["valid"] > 0 and s["invalid"] > 0, f"{bs.name} {row[0]} member {m}"
        for k, claim in enumerate(bs.claims):
            assert len(claim) >= 1
            for cond in claim:
                assert cond in CONDITIONS and holds(cond, st[k], st[k + 1]), \
                    f"{bs.name} {bs.plans[k][0]} -> {bs.plans[k + 1][0]} member {m} claims {cond}: {describe(st[k], st[k + 1])}"
