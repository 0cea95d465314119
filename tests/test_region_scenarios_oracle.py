"""Family J (tests/region_scenarios.py) without a GPU: the independent float32 model of the
cell, counter, score and accept decisions against the CPU oracle on every iteration of every
case, exactly; every property a planted case claims, classified in exact rational arithmetic
(so another seed, RNG or search fails here and not on the GPU); the numpy XORWOW step
against rocRAND's known answers; the host entry sbmp_expand_batch_host child by child and at
equality of the accept comparison; and the altered models of DESIGN.md's power table, each of
which must fail on the case aimed at it.

Needs the built library only for sbmp_division_reciprocal (which division branch a width
takes) and sbmp_expand_batch_host.  tests/test_gpu_region_scenarios.py runs the HIP planner
on the same table.
"""
import functools
import json
import os
from fractions import Fraction

import numpy as np
import pytest

from conftest import GOLDEN
from region_scenarios import (ALTERED, CASE_IDS, CORNER, F32, FMA_N, GAP_N, N1, R1_SEARCHES, SMALL, U32, Y_TWINS, Model,
                              accept_draw, branch, cases, check_expand, check_trace, cub_sum, down, exact_quotient, expand_inputs,
                              local, r1_triples, root_case, scenario, score, sizes, to_cell, trace, unfused_local, up,
                              xorwow_step)
from scenarios import make_oracle

M32 = 0xFFFFFFFF


@functools.lru_cache(maxsize=6)
def oracle_run(name):
    """(the stepped oracle of one case at its end, its snapshots); read only."""
    c = cases()[name]
    o = make_oracle(scenario(c), plan=False)
    return o, tuple(trace(c, o))


def oracle_trace(name):
    return oracle_run(name)[1]


@functools.lru_cache(maxsize=None)
def seen_of(name):
    """The model's per-child view of every iteration of a case (the model holds against the oracle)."""
    return tuple(check_trace(cases()[name], oracle_trace(name)))


NAMES = CASE_IDS


def test_case_table(oracle_lib):
    assert tuple(cases()) == CASE_IDS


def frac(v) -> Fraction:
    return Fraction(float(F32(v)))


def target_xy(name):
    c = cases()[name]
    s = seen_of(name)[0]
    return F32(s.x[c.target]), F32(s.y[c.target])


# ---------------------------------------------------------------- the model's own parts
def test_xorwow_step_against_rocrand():
    """The numpy recurrence on rocRAND's seeding (subsequence 0) gives rocRAND's own draws."""
    kat = json.load(open(os.path.join(GOLDEN, "xorwow_rocrand_kat.json")))
    checked = 0
    for c in kat["cases"]:
        if c["subsequence"]:
            continue
        s0, s1 = (c["seed"] & M32) ^ 0x2C7F967F, ((c["seed"] >> 32) & M32) ^ 0xA03697CB
        t0, t1 = (1228688033 * s0) & M32, (2073658381 * s1) & M32
        st = np.array([[(123456789 + t0) & M32, 362436069 ^ t0, (521288629 + t1) & M32, 88675123 ^ t1,
                        (5783321 + t0) & M32, (6615241 + t1 + t0) & M32]], dtype=U32)
        draws = []
        for _ in range(8):
            x, st = xorwow_step(st)
            draws.append(int(x[0]))
        assert draws == c["draws"], c["seed"]
        checked += 1
    assert checked >= 5


def test_cub_sum_order():
    """D8's order differs from the index order on values that do not add exactly."""
    s = (np.arange(256, dtype=np.float64) * 0.37 + 1e-3).astype(F32) ** 3
    want = F32(0)
    t = s.reshape(8, 32).copy()
    for w in range(8):
        a = t[w].copy()
        for off in (1, 2, 4, 8, 16):
            for i in range(0, 32 - off, 2 * off):
                a[i] = F32(a[i] + a[i + off])
        want = a[0] if w == 0 else F32(want + a[0])
    assert cub_sum(s).view(U32) == want.view(U32)
    assert cub_sum(s) != ALTERED["index-order-sum"].total(s)


def test_score_of_a_single_cell_and_of_65536_children():
    """One available cell scores s / s = 1 whatever its counters, R1 = 65,536 included (1 + R1^2 = 1 + 2^32 is
    exact in double and the score stays a normal float)."""
    n = 4
    t = {k: np.zeros(256, dtype=np.int32) for k in ("R1", "R1Avail", "R1Valid", "R1Invalid")}
    t["R2Avail"] = np.zeros(256 * n * n, dtype=np.int32)
    t["R1"][68], t["R1Avail"][68], t["R1Valid"][68], t["R2Avail"][68 * 16 + 5] = 65536, 1, 65536, 1
    sc = score(t, n)
    assert sc[68] == 1 and (np.delete(sc, 68) == 1).all()
    t["R1"][3], t["R1Avail"][3], t["R1Valid"][3], t["R1Invalid"][3], t["R2Avail"][3 * 16] = 7, 1, 5, 2, 1
    sc = score(t, n)
    fv = F32(F32(F32(0.01) + F32(5)) / F32(F32(F32(0.01) + F32(5)) + F32(2)))
    s3 = F32(np.float64(F32(F32(fv * fv) * F32(fv * fv))) / (np.float64(F32(1) + F32(1 / 16)) * 50.0))
    s68 = F32(np.float64(F32(1)) / (np.float64(F32(1) + F32(1 / 16)) * (1.0 + 2.0 ** 32)))
    assert s68 > np.finfo(np.float32).tiny
    assert sc[3].view(U32) == F32(s3 / F32(s3 + s68)).view(U32) and sc[68].view(U32) == F32(s68 / F32(s3 + s68)).view(U32)


# ---------------------------------------------------------------- the model against the oracle, every case
@pytest.mark.parametrize("name", NAMES)
def test_model_against_oracle(name, oracle_lib):
    c = cases()[name]
    seen = seen_of(name)
    assert len(seen) == c.iterations, "every iteration is checked"
    assert seen[0].S == c.slots
    if not c.kind.startswith("conc"):
        assert c.iterations == 3 and c.slots == 16384 and seen[0].accept.any() and seen[1].S > 0
        assert c.root[3] != 0, "a moving root"


# ---------------------------------------------------------------- J-r1 and J-neglx
TRIPLES = [(tag, site) for tag, _, _, _ in R1_SEARCHES for site in ("small", "large")] + [("point", "small")]


@pytest.mark.parametrize("tag,site", TRIPLES, ids=[f"{t}-{s}" for t, s in TRIPLES])
def test_r1_triple(tag, site, oracle_lib):
    prefix = f"J-r1-{tag}-{site}-" if tag != "point" else "J-r1-point-"
    first = "on" if "pow2" in tag else "up"
    cu, cb, ca = (cases()[prefix + v] for v in (first, "below", "above"))
    c, axis, slot, n = cu.c, cu.axis, cu.target, cu.n
    assert (cb.c, cb.axis, cb.target, ca.c, ca.axis, ca.target) == (c, axis, slot, c, axis, slot)
    assert (c & (c - 1) == 0) == (first == "on") and axis == (1 if "y-" in tag else 0)
    v = target_xy(cu.name)[axis]
    for other in (cb, ca):
        assert target_xy(other.name)[axis].view(U32) == v.view(U32), "one child, three widths"
    assert all(seen_of(k.name)[0].valid[slot] for k in (cu, cb, ca))
    col = lambda case: int(seen_of(case.name)[0].r1[slot]) // N1 if axis else int(seen_of(case.name)[0].r1[slot]) % N1
    sub = lambda case: ((int(seen_of(case.name)[0].r2[slot]) % (n * n)) // n if axis
                        else int(seen_of(case.name)[0].r2[slot]) % n)
    # the first width: the real quotient below c (on c for a power of two), its float on c, cell c
    q = exact_quotient(v, cu.width)
    R1Size, R2Size = sizes(cu.width, n)
    assert (q < c if first == "up" else q == c) and F32(v / R1Size) == c and col(cu) == c
    assert Fraction(c) - q < Fraction(c) * Fraction(1, 2 ** 24)
    # J-neglx: lx = RN(x - c R1Size) < 0 (0 on the line), p in (-1, 0] truncates to sub-column 0
    lx = local(v, c, R1Size)
    assert -1 < F32(lx / R2Size) <= 0
    if first == "up":
        assert lx < 0 and F32(lx / R2Size) < 0 and frac(v) < c * frac(R1Size)
    else:
        assert lx == 0 and frac(v) == c * frac(R1Size)
    assert seen_of(cu.name)[0].r2[slot] >= 0 and sub(cu) == 0
    # one ulp wider: the float quotient is the float before c, cell c - 1, the last sub-column or the gap
    assert cb.width == float(up(cu.width))
    qb = F32(v / sizes(cb.width, n)[0])
    assert qb == down(c) and exact_quotient(v, cb.width) < c and col(cb) == c - 1
    # narrower: the real quotient above c, cell c
    assert ca.width < cu.width and exact_quotient(v, ca.width) > c and col(ca) == c
    assert branch(cu.width, n) == ("rcp" if site == "small" else "ieee")
    if tag == "point":
        assert cu.agent == "point" and seen_of(cu.name)[0].x[slot] != SMALL.root[0]


def test_triples_cover_the_lines(oracle_lib):
    odd = {t.c for t in r1_triples(SMALL, "car", 0, R1_SEARCHES[0][2])}
    assert len(odd) >= 3 and all(c % 2 for c in odd), "several odd lines have round-up children"
    assert {t.c % 2 for t in r1_triples(SMALL, "car", 1, R1_SEARCHES[1][2])} == {1}, "odd lines in y too"
    assert {t.first for t in r1_triples(SMALL, "car", 1, R1_SEARCHES[2][2])} == {"on"}
    assert any(cases()[k].n > 1 for k in cases() if k.endswith("-up")), "J-neglx needs n > 1"


# ---------------------------------------------------------------- J-minus1
@pytest.mark.parametrize("axis", (0, 1), ids=("x", "y"))
def test_minus_one(axis, oracle_lib):
    at, inn, out = (cases()[f"J-minus1-{'xy'[axis]}-{v}"] for v in ("at", "in", "out"))
    slot = at.target
    v = target_xy(at.name)[axis]
    assert v < 0 and target_xy(at.name)[1 - axis] > 0 and at.root == CORNER.root
    for k in (inn, out):
        assert target_xy(k.name)[axis].view(U32) == v.view(U32) and k.target == slot
    assert frac(at.width) == -16 * frac(v) and exact_quotient(v, at.width) == -1
    assert inn.width == float(up(at.width)) and -1 < exact_quotient(v, inn.width) < 0
    assert out.width == float(down(at.width)) and exact_quotient(v, out.width) < -1
    assert F32(v / sizes(inn.width, 1)[0]) > -1 and F32(v / sizes(out.width, 1)[0]) < -1
    s_at, s_in, s_out = (seen_of(k.name)[0] for k in (at, inn, out))
    assert not s_at.valid[slot] and not s_in.valid[slot] and not s_out.valid[slot]
    assert s_at.r1[slot] == -1 and s_out.r1[slot] == -1, "on -1.0 and below it the child is not counted"
    r1 = int(s_in.r1[slot])
    assert r1 >= 0 and (r1 // N1 if axis else r1 % N1) == 0, "inside (-1, 0) it is counted in column (row) 0"
    after = oracle_trace(inn.name)[1].regions
    assert after["R1Invalid"][r1] >= 1 and after["R2Invalid"][int(s_in.r2[slot])] >= 1


# ---------------------------------------------------------------- J-fma
def col_of(r1, axis):
    return int(r1) // N1 if axis else int(r1) % N1


def sub_of(r2, n, axis):
    return (int(r2) % (n * n)) // n if axis else int(r2) % n


PLANTED = {kind: [(site, f"n{n}") for site in ("small", "large") for n in ns]
           + [(site, f"y-n{n}") for site in ("small", "large") for k, n in Y_TWINS if k == kind]
           for kind, ns in (("fma", FMA_N), ("gap", GAP_N))}


@pytest.mark.parametrize("site,tag", PLANTED["fma"], ids=[f"{t}-{s}" for s, t in PLANTED["fma"]])
def test_contraction(site, tag, oracle_lib):
    c = cases()[f"J-fma-{tag}-{site}"]
    n = c.n
    assert c.axis == (1 if tag.startswith("y") else 0)
    s = seen_of(c.name)[0]
    v = target_xy(c.name)[c.axis]
    R1Size, R2Size = sizes(c.width, n)
    assert to_cell(F32(v / R1Size), N1) == c.c >= 1 and s.valid[c.target]
    prod = c.c * frac(R1Size)
    assert frac(F32(F32(c.c) * R1Size)) != prod, "c R1Size is inexact"
    fused, unfused = local(v, c.c, R1Size), unfused_local(v, c.c, R1Size)
    # the fused lx is the exact difference rounded once
    exact = frac(v) - prod
    assert abs(frac(fused) - exact) <= abs(frac(unfused) - exact) and fused != unfused
    pf, pu = int(to_cell(F32(fused / R2Size), n)), int(to_cell(F32(unfused / R2Size), n))
    assert pf != pu and 0 <= pf < n and 0 <= pu < n
    assert sub_of(s.r2[c.target], n, c.axis) == pf and col_of(s.r1[c.target], c.axis) == c.c
    assert branch(c.width, n) == ("rcp" if site == "small" else "ieee")


# ---------------------------------------------------------------- J-gap
@pytest.mark.parametrize("site,tag", PLANTED["gap"], ids=[f"{t}-{s}" for s, t in PLANTED["gap"]])
def test_r2_gap(site, tag, oracle_lib):
    c = cases()[f"J-gap-{tag}-{site}"]
    n = c.n
    assert c.axis == (1 if tag.startswith("y") else 0)
    s = seen_of(c.name)[0]
    v = target_xy(c.name)[c.axis]
    R1Size, R2Size = sizes(c.width, n)
    assert n & (n - 1) and n * frac(R2Size) < frac(R1Size), "R2Size was rounded down"
    assert s.valid[c.target] and col_of(s.r1[c.target], c.axis) == c.c and exact_quotient(v, c.width) < c.c + 1
    lx = local(v, c.c, R1Size)
    assert F32(lx / R2Size) >= n and frac(lx) < frac(R1Size)
    assert s.r2[c.target] == -1 and not s.accept[c.target], "accepted nowhere"
    # counted in the three R1 tables and in no R2 table: the R2 tables' rise is the other children's
    before, after = oracle_trace(c.name)[0].regions, oracle_trace(c.name)[1].regions
    gaps = int(((s.r1 >= 0) & (s.r2 < 0) & s.valid).sum())
    assert gaps >= 1 and (after["R1Valid"] - before["R1Valid"]).sum() == ((s.r1 >= 0) & s.valid).sum()
    assert (after["R2Valid"] - before["R2Valid"]).sum() == ((s.r1 >= 0) & s.valid).sum() - gaps
    assert branch(c.width, n) == ("rcp" if site == "small" else "ieee")


def test_both_division_branches(oracle_lib):
    """J-r1, J-neglx, J-fma and J-gap each run where bins_k takes the reciprocal and where it divides."""
    for kind in ("r1-up", "r1-on", "fma", "gap"):
        got = {branch(c.width, c.n) for c in cases().values() if c.kind == kind}
        assert got == {"rcp", "ieee"}, (kind, got)
    from cudasbmp_amd.kgmt import division_reciprocal
    assert division_reciprocal(1.25) == float(F32(0.8)) and division_reciprocal(float(2.0 ** 21)) == 0.0
    assert division_reciprocal(float("nan")) == 0.0 and division_reciprocal(0.0) == 0.0
    assert all(sizes(c.width, c.n)[0] > 2.0 ** 20 for c in cases().values() if c.site == "large")


# ---------------------------------------------------------------- J-conc
@pytest.mark.parametrize("n", (4, 12))
def test_concentration(n, oracle_lib):
    free, cov = cases()[f"J-conc-n{n}-free"], cases()[f"J-conc-n{n}-covered"]
    sf, sc = seen_of(free.name), seen_of(cov.name)
    assert [s.S for s in sf] == [65536, 65536] and [s.S for s in sc] == [65536, 0], "the covered run stalls (D7)"
    for s in sf + sc[:1]:
        assert len(set(s.r1.tolist())) == 1 and len(set(s.r2.tolist())) == 1 and s.r2[0] >= 0
    assert all(s.valid.all() and s.accept.all() for s in sf), "one available cell scores 1: every child is accepted"
    assert not sc[0].valid.any() and not sc[0].accept.any()
    r1 = int(sf[0].r1[0])
    t = oracle_trace(free.name)
    assert t[1].regions["R1"][r1] == 65537 and t[2].regions["R1"][r1] == 131073
    assert t[2].regions["R2Valid"][int(sf[0].r2[0])] == 131072
    tc = oracle_trace(cov.name)
    assert tc[1].regions["R1Invalid"][r1] == 65536 and tc[1].regions["R2Invalid"][int(sc[0].r2[0])] == 65536
    assert all(np.array_equal(tc[1].regions[k], tc[2].regions[k]) for k in tc[1].regions if k != "R1Score")
    assert 256 * n * n <= 32767 if n == 4 else 256 * n * n > 32767     # the key log, or direct atomics


def test_two_cells_carry_large_counts_through_the_score(oracle_lib):
    """J-conc-n4-two-cells: the scores of iterations 2 and 3 divide by 1 + R1^2 with R1 past 2^15 in one cell
    beside another available cell, so the quotient s / total is no longer 1 and shows the denominator's type."""
    name = "J-conc-n4-two-cells"
    seen, t = seen_of(name), oracle_trace(name)
    assert [s.S for s in seen][:2] == [65536] * 2 and seen[2].S > 32768
    for k in (1, 2):
        R1, avail = t[k].regions["R1"], t[k].regions["R1Avail"]
        assert avail.sum() >= 2 and R1.max() > 2 ** 15 and np.sort(R1)[-2] > 2 ** 10
        sc = seen[k].score[avail != 0]
        assert ((sc > 0) & (sc < 1)).all()
    assert t[2].regions["R1"].max() > 2 ** 16
    assert 0 < seen[2].accept.sum() < seen[2].S, "the score decides: neither all nor none are accepted"


# ---------------------------------------------------------------- sbmp_expand_batch_host: per child, and J-accept
EXPAND_NAMES = ["J-r1-x-odd-small-up", "J-r1-x-odd-large-up", "J-r1-y-odd-small-up", "J-r1-y-odd-large-up", "J-fma-y-n8-small", "J-r1-y-pow2-small-on", "J-minus1-x-in", "J-minus1-x-at",
                "J-fma-n3-small", "J-fma-n8-large", "J-gap-n11-small", "J-gap-n12-large", "J-r1-point-up"]


def expand(case, R1Score, R2Avail, device):
    from cudasbmp_amd.batch import expand_batch
    parents, rng = expand_inputs(case)
    got = expand_batch(parents, rng, np.zeros((0, 4), np.float32), width=case.width, height=case.height, n=case.n,
                       agent=case.agent, R1Score=R1Score, R2Avail=R2Avail, device=device)
    return got, rng


def check_expand_case(name, device):
    """Iteration 1 through the batch entry with the score and availability the planner had: the model
    child by child, and the same accept bits as the planner's iteration 1."""
    c = cases()[name]
    before = oracle_trace(name)[0].regions
    sc = score(before, c.n)
    got, rng = expand(c, sc, before["R2Avail"], device)
    s = check_expand(c, got, rng, sc, before["R2Avail"])
    first = seen_of(name)[0]
    assert np.array_equal(s.accept, first.accept) and np.array_equal(s.r2, first.r2)
    assert np.array_equal(got["children"].view(U32), oracle_trace(name)[1].unexplored[:c.slots].view(U32))


@pytest.mark.parametrize("name", EXPAND_NAMES)
def test_expand_batch_host(name, oracle_lib):
    check_expand_case(name, device=False)


def accept_at_equality(device):
    """R1Score[r1] on the target's own draw, one ulp above and one below: accept, accept, reject."""
    c = cases()["J-r1-x-odd-small-above"]
    parents, rng = expand_inputs(c)
    first = seen_of(c.name)[0]
    u = accept_draw(rng)[0]
    t = c.target
    assert first.valid[t] and first.r2[t] >= 0 and 0 < u[t] < 1
    avail = np.ones(256 * c.n * c.n, dtype=np.int32)        # every cell available: the score alone decides
    verdicts = []
    for thr in (u[t], up(u[t]), down(u[t])):
        sc = np.full(256, 0.5, dtype=np.float32)
        sc[first.r1[t]] = thr
        got, _ = expand(c, sc, avail, device)
        check_expand(c, got, rng, sc, avail)
        verdicts.append(bool(got["accept"][t]))
    assert verdicts == [True, True, False]


def test_accept_at_equality_host(oracle_lib):
    accept_at_equality(device=False)


# ---------------------------------------------------------------- J-root
def test_root_binning(oracle_lib):
    c = root_case()
    x = F32(c.root[0])
    R1Size, R2Size = sizes(c.width, c.n)
    assert exact_quotient(x, c.width) < c.c and F32(x / R1Size) == c.c and local(x, c.c, R1Size) < 0
    o = make_oracle(scenario(c), plan=False)
    check_root(c, o.regions())
    check_trace(c, trace(c, o))


def check_root(c, regions):
    R1Size, R2Size = sizes(c.width, c.n)
    cy = int(to_cell(F32(F32(c.root[1]) / R1Size), N1))
    py = int(to_cell(F32(local(c.root[1], cy, R1Size) / R2Size), c.n))
    r1 = cy * N1 + c.c
    assert np.nonzero(regions["R1Avail"])[0].tolist() == [r1] and regions["R1"][r1] == 1 and regions["R1Valid"][r1] == 1
    assert np.nonzero(regions["R2Avail"])[0].tolist() == [r1 * c.n * c.n + py * c.n + 0], "sub-column 0 of cell c"


# ---------------------------------------------------------------- power: every altered model fails where it is aimed
AIMED = {
    "floor": "J-minus1-x-in",               # floor(-0.x) = -1: the child would not be counted
    "real-quotient": "J-r1-x-odd-small-up",
    "unfused-lx": "J-fma-n3-small",
    "ge-minus-one": "J-minus1-x-at",
    "strict-accept": None,                  # only the batch entry can plant u == score: below
    "early-draw": "J-r1-x-odd-small-up",
    "index-order-sum": "J-r1-x-odd-small-up",
    "gap-counted-in-R2": "J-gap-n11-small",
    "float-denominator": "J-conc-n4-two-cells",
    "real-quotient-y": "J-r1-y-odd-small-up",
    "unfused-ly": "J-fma-y-n8-small",
}


def fails(name, m: Model) -> bool:
    try:
        check_trace(cases()[name], oracle_trace(name), m)
    except AssertionError:
        return True
    return False


@pytest.mark.parametrize("alteration", list(ALTERED))
def test_altered_model_fails(alteration, oracle_lib):
    assert set(AIMED) == set(ALTERED)
    m = ALTERED[alteration]
    if AIMED[alteration]:
        assert fails(AIMED[alteration], m), f"the model with {alteration} passes {AIMED[alteration]}"
        return
    # `<` for `<=`: against the oracle's own batch entry, with the score on the target's draw
    c = cases()["J-r1-x-odd-small-above"]
    parents, rng = expand_inputs(c)
    first = seen_of(c.name)[0]
    sc = np.full(256, 0.5, dtype=np.float32)
    sc[first.r1[c.target]] = accept_draw(rng)[0][c.target]
    avail = np.ones(256 * c.n * c.n, dtype=np.int32)
    from oracle.pyoracle import PlannerConfig, expand_batch
    cfg, extra = scenario(c).config()
    got = expand_batch(PlannerConfig(**cfg), np.zeros((0, 4), np.float32), parents, rng, sc, avail)
    check_expand(c, got, rng, sc, avail)
    with pytest.raises(AssertionError):
        check_expand(c, got, rng, sc, avail, m)
