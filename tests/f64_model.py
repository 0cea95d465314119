"""A float64 model of one KGMT expansion step, and an audit that holds a planner to it.

The planner tests of this suite compare the HIP kernels with the CPU oracle bit for
bit; both were written by the same hand and share headers.  This module states what
the operation *is*, independently, from the reference's description (SURVEY.md §8a
rows a6, a8, a9, a10, a4 and the reference's statePropagator.cu, collisionCheck.cu,
KGMT.cu getR1 / getR2 / updateR1 / propagateG / updateG):

  * an explicit-Euler kinematic bicycle (replay_car) and the build's holonomic point
    (replay_point), with the reference's update order and break semantics;
  * a per-step bounding-box test against axis-aligned boxes;
  * a truncating two-level binning (bins);
  * the region score (r1_scores);
  * the counters, the accept rule and the insertion, checked by audit_run.

Inputs are the float32 parent state and the child's *stored* float32 controls, widened
to float64, so the random number generator and the double-pi steering expression (D11)
stay out of the model.  Every float32 rounding the kernels may make is carried through
the same loop as a first-order error bound (u = 2^-24); a child whose verdict could
change within twice that bound is `borderline` and is excused from the sharp checks,
and audit_run caps the share of such children so the audit cannot excuse everything.

Plain numpy: no GPU, no oracle and no project code at import.
"""
from __future__ import annotations

import bisect

import numpy as np

U = 2.0 ** -24          # float32 unit roundoff
SINCOS_ULP = 4 * U      # 2 ulp at |value| <= 1: CUDA_ULP_BOUND of tests/test_math.py
TAN_REL = 10 * U        # (v / L) tan(steering): 4 ulp = 8u for tan, u for the quotient, u for the product
EPSILON = 0.01          # updateR1's epsilon (KGMT.cu:133)
PAIR_CHUNK = 1 << 21    # child x box pairs evaluated at once

LOG_BEFORE, LOG_S, LOG_A, LOG_AFTER = 1, 5, 6, 7   # columns of iter_log


# ---------------------------------------------------------------------------------------
# boxes
class _Boxes:
    """Boxes sorted by xmin so that one child only meets the boxes whose x range can reach
    its own: a box left out has `hi_x <= xmin` or `xmax <= lo_x` true by more than the margin,
    so it separates in the nominal, the pessimistic and the optimistic reading alike.
    Boxes with a non-finite coordinate are met by every child."""

    def __init__(self, boxes):
        b = np.asarray(boxes, dtype=np.float64).reshape(-1, 4)
        finite = np.isfinite(b).all(axis=1)
        self.always = b[~finite]
        b = b[finite]
        b = b[np.argsort(b[:, 0], kind="stable")]
        self.sorted = b
        self.xmin = np.ascontiguousarray(b[:, 0])
        self.wmax = float(max(0.0, (b[:, 2] - b[:, 0]).max())) if len(b) else 0.0

    @staticmethod
    def _verdicts(lx, hx, ly, hy, mx, my, box):
        x0, y0, x1, y1 = box[:, 0], box[:, 1], box[:, 2], box[:, 3]
        # four separate comparisons: a NaN coordinate never separates
        nominal = (hx <= x0) | (x1 <= lx) | (hy <= y0) | (y1 <= ly)
        sure = (hx + mx <= x0) | (x1 <= lx - mx) | (hy + my <= y0) | (y1 <= ly - my)
        maybe = (hx - mx <= x0) | (x1 <= lx + mx) | (hy - my <= y0) | (y1 <= ly + my)
        return nominal, sure, maybe

    def hits(self, lx, hx, ly, hy, mx, my):
        """Per child: (hit, surely hit, possibly hit) by any box; m = margin per axis.
        A child is borderline at this step when the two differ, that is when the step's verdict
        over all boxes is in doubt: a box in doubt beside one that surely hits excuses nothing."""
        n = len(lx)
        hit = np.zeros(n, bool)
        hit_sure = np.zeros(n, bool)
        hit_maybe = np.zeros(n, bool)
        for box in self.always:
            nominal, sure, maybe = self._verdicts(lx, hx, ly, hy, mx, my, box[None, :])
            hit |= ~nominal
            hit_sure |= ~maybe
            hit_maybe |= ~sure
        if not len(self.sorted) or not n:
            return hit, hit_sure, hit_maybe
        wild = ~(np.isfinite(lx) & np.isfinite(hx) & np.isfinite(mx))
        i0 = np.searchsorted(self.xmin, np.where(wild, -np.inf, lx - mx - self.wmax), side="left")
        i1 = np.searchsorted(self.xmin, np.where(wild, np.inf, hx + mx), side="right")
        cnt = np.maximum(i1 - i0, 0)
        ends = np.cumsum(cnt)
        first = 0
        while first < n:
            last = int(np.searchsorted(ends, (ends[first - 1] if first else 0) + PAIR_CHUNK, side="right"))
            last = max(last, first + 1)
            c = cnt[first:last]
            tot = int(c.sum())
            if tot:
                child = np.repeat(np.arange(first, last), c)
                offs = np.cumsum(c) - c
                box = np.arange(tot) + np.repeat(i0[first:last] - offs, c)
                nominal, sure, maybe = self._verdicts(lx[child], hx[child], ly[child], hy[child], mx[child],
                                                      my[child], self.sorted[box])
                hit |= np.bincount(child[~nominal], minlength=n).astype(bool)
                hit_sure |= np.bincount(child[~maybe], minlength=n).astype(bool)
                hit_maybe |= np.bincount(child[~sure], minlength=n).astype(bool)
            first = last
        return hit, hit_sure, hit_maybe


def _as_boxes(boxes):
    return boxes if isinstance(boxes, _Boxes) else _Boxes(boxes)


# ---------------------------------------------------------------------------------------
# propagation
ALTERATIONS = ("dt-over-steps-plus-one", "theta-before-x", "v-before-x", "no-tan", "swap-sin-cos", "strict-bounds")


def _bounds(x, y, ex, ey, W, H, strict=False):
    """x <= 0 or x >= W or y <= 0 or y >= H: (nominal, sure, possible); NaN is never outside."""
    mx, my = 2.0 * ex, 2.0 * ey
    if strict:   # an alteration: a child exactly on the wall stays valid
        return ((x < 0.0) | (x > W) | (y < 0.0) | (y > H), (x + mx < 0.0) | (x - mx > W) | (y + my < 0.0) | (y - my > H),
                (x - mx < 0.0) | (x + mx > W) | (y - my < 0.0) | (y + my > H))
    nominal = (x <= 0.0) | (x >= W) | (y <= 0.0) | (y >= H)
    sure = (x + mx <= 0.0) | (x - mx >= W) | (y + my <= 0.0) | (y - my >= H)
    maybe = (x - mx <= 0.0) | (x + mx >= W) | (y - my <= 0.0) | (y + my >= H)
    return nominal, sure, maybe


def _replay(kind, parents4, controls3, numDisc, L, W, H, boxes, alter=frozenset()):
    """`alter`: deliberate misreadings of the operation, for the tests that show the audit
    notices them (ALTERATIONS); empty for the model itself."""
    assert set(alter) <= set(ALTERATIONS), alter
    p = np.asarray(parents4, dtype=np.float64).reshape(-1, 4)
    c = np.asarray(controls3, dtype=np.float64).reshape(-1, 3)
    index = _as_boxes(boxes)
    W, H, L = float(np.float32(W)), float(np.float32(H)), float(np.float32(L))
    n = len(p)
    x, y, th, v = (p[:, i].copy() for i in range(4))
    c0, c1, T = c[:, 0], c[:, 1], c[:, 2]
    dt = T / (numDisc + 1 if "dt-over-steps-plus-one" in alter else numDisc)
    e_dt = U * np.abs(dt)                                   # the division that produces dt
    ex, ey, eth, ev = (np.zeros(n) for _ in range(4))
    live = np.ones(n, bool)
    valid = np.ones(n, bool)
    borderline = np.zeros(n, bool)
    if kind == "car":
        a = c0
        with np.errstate(all="ignore"):
            tan = np.tan(c1)                                # loop invariant (a8)
        if "no-tan" in alter:
            tan = c1
    with np.errstate(all="ignore"):
        for _ in range(numDisc):
            if not live.any():
                break
            # 1. x, y from the old theta and v
            if kind == "car":
                th_x = th + (v / L) * tan * dt if "theta-before-x" in alter else th
                v_x = v + a * dt if "v-before-x" in alter else v
                cos, sin = (np.sin(th_x), np.cos(th_x)) if "swap-sin-cos" in alter else (np.cos(th_x), np.sin(th_x))
                e_cs = eth + SINCOS_ULP
                ix, iy = v_x * cos * dt, v_x * sin * dt
                # the sensitivities to e_v and e_cos, the rounding of dt, of the two products
                e_ix = dt * (ev * np.abs(cos) + np.abs(v_x) * e_cs) + np.abs(v_x * cos) * e_dt + 2.0 * U * np.abs(ix)
                e_iy = dt * (ev * np.abs(sin) + np.abs(v_x) * e_cs) + np.abs(v_x * sin) * e_dt + 2.0 * U * np.abs(iy)
            else:
                ix, iy = c0 * dt, c1 * dt
                e_ix = np.abs(c0) * e_dt + U * np.abs(ix)
                e_iy = np.abs(c1) * e_dt + U * np.abs(iy)
            xn, yn = x + ix, y + iy
            exn = ex + e_ix + U * np.abs(xn)
            eyn = ey + e_iy + U * np.abs(yn)
            # 2. the workspace test: invalid and stop with the new (x, y), the old (theta, v)
            oob, oob_sure, oob_maybe = _bounds(xn, yn, exn, eyn, W, H, strict="strict-bounds" in alter)
            borderline |= live & (oob_sure != oob_maybe)
            out = live & oob
            go = live & ~oob
            xo, yo, exo, eyo = x, y, ex, ey
            x, y = np.where(live, xn, x), np.where(live, yn, y)
            ex, ey = np.where(live, exn, ex), np.where(live, eyn, ey)
            valid &= ~out
            live = go
            # 3. theta and v
            if kind == "car":
                dth = (v / L) * tan * dt
                # relative 10u on (v / L) tan, u on the product with dt, the sensitivity to e_v
                e_dth = np.abs(dth) * (TAN_REL + 2.0 * U) + (ev / abs(L)) * np.abs(tan) * dt
                thn = th + dth
                vn = v + a * dt
                ethn = eth + e_dth + U * np.abs(thn)
                evn = ev + 2.0 * U * np.abs(a * dt) + U * np.abs(vn)
                th, eth = np.where(go, thn, th), np.where(go, ethn, eth)
                v, ev = np.where(go, vn, v), np.where(go, evn, ev)
            # 4. the bounding box of the old and the new (x, y); 5. the boxes
            idx = np.nonzero(go)[0]
            if len(idx):
                lx, hx = np.minimum(xo[idx], x[idx]), np.maximum(xo[idx], x[idx])
                ly, hy = np.minimum(yo[idx], y[idx]), np.maximum(yo[idx], y[idx])
                # min / max drop a NaN operand: put it back, a NaN coordinate never separates
                bad_x, bad_y = np.isnan(xo[idx]) | np.isnan(x[idx]), np.isnan(yo[idx]) | np.isnan(y[idx])
                lx, hx = np.where(bad_x, np.nan, lx), np.where(bad_x, np.nan, hx)
                ly, hy = np.where(bad_y, np.nan, ly), np.where(bad_y, np.nan, hy)
                mx = 2.0 * np.maximum(exo[idx], ex[idx])
                my = 2.0 * np.maximum(eyo[idx], ey[idx])
                hit, hit_sure, hit_maybe = index.hits(lx, hx, ly, hy, mx, my)
                borderline[idx] |= hit_sure != hit_maybe
                valid[idx[hit]] = False
                live[idx[hit]] = False
    state = np.stack([x, y, th, v], axis=1)
    bound = np.stack([ex, ey, eth, ev], axis=1)
    return state, valid, bound, borderline


def replay_car(parents4, controls3, numDisc, L, W, H, boxes, alter=frozenset()):
    """Children of f32 parents (x, y, theta, v) under stored f32 controls (a, steering,
    duration), in float64: (state (n, 4), valid, first-order error bound (n, 4), borderline)."""
    return _replay("car", parents4, controls3, numDisc, L, W, H, boxes, alter)


def replay_point(parents4, controls3, numDisc, L, W, H, boxes):
    """The holonomic point: controls (vx, vy, duration), x += vx dt,
    y += vy dt, the same bounds and box tests; the child's theta and v are 0 whatever the parent's."""
    state, valid, bound, borderline = _replay("point", parents4, controls3, numDisc, L, W, H, boxes)
    state[:, 2:] = 0.0
    return state, valid, bound, borderline


# ---------------------------------------------------------------------------------------
# binning
def _axis(x, R1, R2, n, rnd):
    """One axis of getR1 / getR2: the nominal (R1 column, R2 column), whether float32 could
    have chosen a neighbour at either level, and the four candidate (column, sub-column) pairs.

    The R1 quotient x / R1Size carries one rounding; 4u |quotient| is allowed.
    The R2 quotient is (x - column * R1Size) / R2Size: the product and the difference each
    round at the size of x, so it moves by up to 2u |x| / R2Size + 4u |quotient|.  A quotient
    that is an integer exactly, from exactly representable operands, is no edge: float32
    division returns it unchanged (children that never moved off the root's cell corner)."""
    with np.errstate(all="ignore"):
        q = x / R1
        t = np.where(q == np.rint(q), 0.0, 4 * U * np.abs(q))
        col, col_lo, col_hi = rnd(q), rnd(q - t), rnd(q + t)

        def sub(c):
            q2 = (x - c * R1) / R2
            exact = (q2 == np.rint(q2)) & ((c * R1).astype(np.float32).astype(np.float64) == c * R1)
            t2 = np.where(exact, 0.0, 4 * U * np.abs(q2) + 2 * U * np.abs(x) / R2)
            return rnd(q2), rnd(q2 - t2), rnd(q2 + t2)

        s, s_lo, s_hi = sub(col)
        cands = []
        for c in (col_lo, col_hi):
            _, a, b = sub(c)
            cands += [(c, a), (c, b)]
    known = ~np.isnan(x)   # a NaN is outside at every rounding
    return col, s, (col_lo != col_hi) & known, (s_lo != s_hi) & known, cands


def _flat(cx, sx, cy, sy, N, n):
    with np.errstate(all="ignore"):
        in1 = (cx >= 0) & (cx < N) & (cy >= 0) & (cy < N)    # a NaN is outside
        in2 = in1 & (sx >= 0) & (sx < n) & (sy >= 0) & (sy < n)
        z = lambda a, m: np.where(m, a, 0.0)
        r1 = np.where(in1, z(cy, in1) * N + z(cx, in1), -1).astype(np.int64)
        r2 = np.where(in2, r1 * (n * n) + z(sy, in2) * n + z(sx, in2), -1).astype(np.int64)
    return r1, r2


def bin_candidates(x, y, W, N, n, trunc=np.trunc):
    """bins() plus the cells a float32 evaluation could have chosen instead:
    (r1, r2, edge at the R1 level, edge at either level, list of candidate (r1, r2) pairs)."""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    R1 = float(np.float32(W) / np.float32(N))                # the reference's R1Size / R2Size, float32
    R2 = float(np.float32(W) / np.float32(n * N))
    cx, sx, ex1, ex2, candx = _axis(x, R1, R2, n, trunc)     # trunc: toward zero, -0.3 lands in column 0
    cy, sy, ey1, ey2, candy = _axis(y, R1, R2, n, trunc)
    r1, r2 = _flat(cx, sx, cy, sy, N, n)
    corners = [_flat(ax, bx, ay, by, N, n) for ax, bx in candx for ay, by in candy]
    edge1 = ex1 | ey1
    return r1, r2, edge1, edge1 | ex2 | ey2, corners


def bins(x, y, W, N, n):
    """(r1, r2, edge): getR1 / getR2 with truncation toward zero, -1 outside [0, N) / [0, n);
    both cell sizes derive from the width alone (a10).  `edge`: a quotient lies within
    rounding of an integer, so float32 may have chosen the neighbouring cell."""
    r1, r2, _, edge, _ = bin_candidates(x, y, W, N, n)
    return r1, r2, edge


# ---------------------------------------------------------------------------------------
# score
def r1_scores(R1, R1Avail, R1Valid, R1Invalid, R2Avail, n):
    """updateR1 (a4): fv^4 / ((1 + covR) (1 + R1^2)) over the available cells, normalised by
    the sum over all cells; 1.0 where R1Avail is 0."""
    R1 = np.asarray(R1, np.float64)
    avail = np.asarray(R1Avail) != 0
    nv, ni = np.asarray(R1Valid, np.float64), np.asarray(R1Invalid, np.float64)
    cov = np.asarray(R2Avail, np.float64).reshape(len(R1), n * n).sum(axis=1) / (n * n)
    fv = (EPSILON + nv) / (EPSILON + nv + ni)
    score = np.where(avail, fv ** 4 / ((1.0 + cov) * (1.0 + R1 ** 2)), 0.0)
    with np.errstate(all="ignore"):
        return np.where(avail, score / score.sum(), 1.0)


# ---------------------------------------------------------------------------------------
# the audit
class Adapter:
    """The two spellings of the planner interface (the oracle's and cudasbmp_amd.KGMT's)."""

    def __init__(self, planner):
        self.p = planner

    def step(self):
        return self.p.step(1) if hasattr(self.p, "iter_log") else self.p.step()   # KGMT.step(iterations) / Oracle.step()

    def log(self):
        return self.p.iter_log() if hasattr(self.p, "iter_log") else self.p.iter_logs()

    def __getattr__(self, name):
        return getattr(self.p, name)


ALL_CHECKS = frozenset(("state", "counters", "accept", "score", "insert"))


def _count(cells, size):
    cells = cells[cells >= 0]
    return np.bincount(cells, minlength=size)[:size]


def _slack(corners, level, mask, size):
    """Per cell: the masked children that have the cell among their candidates."""
    cand = np.stack([c[level][mask] for c in corners], axis=1)
    out = np.zeros(size, np.int64)
    if cand.size:
        cand = np.sort(cand, axis=1)
        keep = np.ones_like(cand, bool)
        keep[:, 1:] = cand[:, 1:] != cand[:, :-1]
        out += _count(cand[keep], size)
    return out


def audit_run(planner, cfg, boxes, agent, max_iters, cap=0.005, checks=ALL_CHECKS, replay=None, bin_trunc=np.trunc,
              label=""):
    """Step `planner` (begun, not yet stepped) one iteration at a time for up to `max_iters`
    iterations and hold every iteration to the float64 model.  `cfg`: the planner's
    positional configuration (width, height, N, n, numDisc, agentLength).  `cap`: the
    largest share of borderline / edge children the audit may excuse.  `replay` / `bin_trunc`
    replace the model's propagation / quotient rounding (the power tests).  With "state"
    left out of `checks` the state comparison is measured and returned, not asserted.
    Returns the measured figures."""
    P = planner if isinstance(planner, Adapter) else Adapter(planner)
    replay = replay or (replay_point if agent == "point" else replay_car)
    W, H, N, n = cfg["width"], cfg["height"], cfg["N"], cfg["n"]
    index = _as_boxes(boxes)
    n1, n2 = N * N, N * N * n * n
    stats = dict(children=0, borderline=0, edge=0, state_rows=0, state_over=0, worst_ratio=0.0, accepted=0,
                 lottery_rows=0, lottery_accepted=0, lottery_mean=0.0, lottery_var=0.0, iterations=0, new_cell_rows=0)
    for _ in range(max_iters):
        rows_before = len(P.log())
        tree_s, tree_p, tree_c = (a.copy() for a in P.tree())
        reg0 = {k: v.copy() for k, v in P.regions().items()}
        P.step()
        log = P.log()
        if len(log) == rows_before:
            break
        row = log[-1]
        before, S, A, after = (int(row[i]) for i in (LOG_BEFORE, LOG_S, LOG_A, LOG_AFTER))
        stats["iterations"] += 1
        where = f"{label} iteration {int(row[0])}"
        reg1 = P.regions()
        if "score" in checks:
            want = r1_scores(reg0["R1"], reg0["R1Avail"], reg0["R1Valid"], reg0["R1Invalid"], reg0["R2Avail"], n)
            got = reg1["R1Score"].astype(np.float64)
            # 256 summands of the normalising sum plus under 44 other roundings
            assert np.all(np.abs(got - want) <= 300 * U * np.abs(want)), \
                f"score: {where}: worst relative error {np.max(np.abs(got - want) / want) / U:.1f} u"
        if S <= 0:
            continue
        un, up = P.unexplored()
        un, up = un[:S].copy(), up[:S].copy()
        assert (up >= 0).all() and (up < before).all(), f"insert: {where}: a slot's parent is not a tree row"
        state, valid, bound, borderline = replay(tree_s[up, :4], un[:, 4:7], cfg["numDisc"], cfg["agentLength"], W, H,
                                                 index)
        got4 = un[:, :4].astype(np.float64)
        r1, r2, edge1, edge, corners = bin_candidates(got4[:, 0], got4[:, 1], W, N, n, trunc=bin_trunc)
        stats["children"] += S
        stats["borderline"] += int(borderline.sum())
        stats["edge"] += int(edge.sum())

        # 1. state: non-borderline rows with finite bounds and e_theta < 0.1, 2 x bound per component
        ok = ~borderline & np.isfinite(bound).all(axis=1) & np.isfinite(state).all(axis=1) & (bound[:, 2] < 0.1)
        err, bnd = np.abs(got4[ok] - state[ok]), bound[ok]
        with np.errstate(all="ignore"):
            ratio = np.where(err == 0, 0.0, err / bnd)
        ratio = np.where(np.isnan(ratio), np.inf, ratio)
        over = (ratio > 2.0).any(axis=1)
        stats["state_rows"] += int(ok.sum())
        stats["state_over"] += int(over.sum())
        if ratio.size:
            stats["worst_ratio"] = max(stats["worst_ratio"], float(ratio.max()))
        if "state" in checks:
            assert not over.any(), (f"state: {where}: {int(over.sum())} of {int(ok.sum())} rows beyond twice the bound, "
                                    f"worst ratio {ratio.max():.3g}")

        # 2. counters, both directions, per cell
        if "counters" in checks:
            for lvl, cells, unsure, size, names in (
                    (0, r1, borderline | edge1, n1, ("R1Valid", "R1Invalid", "R1")),
                    (1, r2, borderline | edge, n2, ("R2Valid", "R2Invalid", None))):
                if lvl == 1 and n == 1:
                    continue
                sure_v = _count(cells[~unsure & valid], size)
                sure_i = _count(cells[~unsure & ~valid], size)
                slack = _slack(corners, lvl, unsure, size)
                for name, lo in zip(names, (sure_v, sure_i, sure_v + sure_i)):
                    if name is None:
                        continue
                    d = reg1[name].astype(np.int64) - reg0[name].astype(np.int64)
                    bad = np.nonzero((d < lo) | (d > lo + slack))[0]
                    assert not len(bad), (f"counters: {where}: {name} cell {int(bad[0])} rose by {int(d[bad[0]])}, the "
                                          f"model counts {int(lo[bad[0]])} + at most {int(slack[bad[0]])} ({len(bad)} cells)")
            # availability: a cell becomes available exactly when a valid child lands in it
            for name, cells, unsure, size in (("R1Avail", r1, borderline | edge1, n1), ("R2Avail", r2, borderline | edge, n2)):
                sure = _count(cells[~unsure & valid], size) > 0
                maybe = sure | (_slack(corners, 0 if name == "R1Avail" else 1, unsure, size) > 0)
                was, now = reg0[name] != 0, reg1[name] != 0
                assert np.all(now >= (was | sure)) and np.all(now <= (was | maybe)), f"counters: {where}: {name}"

        # 5. insert: rows [before, after) are the accepted slots' children in ascending slot order
        full = after - before != A
        new_s, new_p, new_c = P.tree()
        accepted = np.zeros(S, bool)
        if not full and A:
            key = lambda s, p: np.ascontiguousarray(
                np.concatenate([np.ascontiguousarray(s, np.float32).view(np.uint32), p.astype(np.uint32)[:, None]], axis=1))
            slots = {}
            for i, k in enumerate(key(un, up)):
                slots.setdefault(k.tobytes(), []).append(i)
            prev = -1
            for j, k in enumerate(key(new_s[before:after], new_p[before:after])):
                lst = slots.get(k.tobytes(), [])
                at = bisect.bisect_right(lst, prev)
                assert at < len(lst), f"insert: {where}: tree row {before + j} is no slot's child after slot {prev}"
                prev = lst[at]
                accepted[prev] = True
            if "insert" in checks:
                assert np.array_equal(tree_s[:before].view(np.uint32), new_s[:before].view(np.uint32)), \
                    f"insert: {where}: earlier rows changed"
                dur = new_s[before:after, 6].astype(np.float64)
                want = new_c[new_p[before:after]].astype(np.float64) + dur
                assert np.all(np.abs(new_c[before:after] - want) <= U * np.abs(want)), f"insert: {where}: cost"
        stats["accepted"] += int(accepted.sum())

        # 3. accept
        if "accept" in checks and not full:
            sure_invalid = ~borderline & ~valid
            in_grid = np.zeros(S, bool)
            for c1, c2 in corners:
                in_grid |= (c1 >= 0) & (c2 >= 0)
            in_grid |= (r1 >= 0) & (r2 >= 0)
            bad = accepted & (sure_invalid | ~in_grid)
            assert not bad.any(), f"accept: {where}: slot {int(np.nonzero(bad)[0][0])} accepted though invalid or outside the grid"
            clean = ~borderline & ~edge & valid & (r2 >= 0)
            new_cell = clean & (reg0["R2Avail"][np.where(r2 >= 0, r2, 0)] == 0)
            stats["new_cell_rows"] += int(new_cell.sum())
            miss = new_cell & ~accepted
            assert not miss.any(), (f"accept: {where}: slot {int(np.nonzero(miss)[0][0])} is valid, in a cell with "
                                    f"R2Avail == 0 and was not accepted")
            lottery = clean & ~new_cell
            p = np.minimum(reg1["R1Score"].astype(np.float64)[np.where(r1 >= 0, r1, 0)][lottery], 1.0)
            stats["lottery_rows"] += int(lottery.sum())
            stats["lottery_accepted"] += int((accepted & lottery).sum())
            stats["lottery_mean"] += float(p.sum())
            stats["lottery_var"] += float((p * (1.0 - p)).sum())

    total = max(1, stats["children"])
    stats["borderline_share"] = stats["borderline"] / total
    stats["edge_share"] = stats["edge"] / total
    stats["state_over_share"] = stats["state_over"] / max(1, stats["state_rows"])
    # the cap is a condition of the audit, not a figure: it keeps the slack from excusing everything
    excused = stats["borderline_share"] + stats["edge_share"]
    assert excused <= cap if cap < 1.0 else excused < 1.0 or not stats["children"], \
        f"cap: {label}: borderline {stats['borderline_share']:.4%}, edge {stats['edge_share']:.4%} of {stats['children']}"
    if "accept" in checks and stats["lottery_rows"]:
        # the draws of one run are independent Bernoulli(R1Score[r1]): the sum over the run, where
        # the normal approximation of 5 sigma holds, not each iteration's handful
        sigma = stats["lottery_var"] ** 0.5
        off = abs(stats["lottery_accepted"] - stats["lottery_mean"])
        stats["lottery_sigmas"] = off / sigma if sigma > 0 else (0.0 if off == 0 else float("inf"))
        assert off <= 5.0 * sigma, (f"accept: {label}: {stats['lottery_accepted']} accepted by the draw, expected "
                                    f"{stats['lottery_mean']:.1f} +- {sigma:.1f}")
    return stats


# ---------------------------------------------------------------------------------------
# one batch of children (expand_batch) and the goal row
def audit_batch(out, parents, boxes, agent, numDisc, L, W=20.0, H=20.0, N=16, n=8, R1Score=None, R2Avail=None,
                cap=0.005, special=None):
    """The result of an expand_batch (children (k, 7), valid, r1, r2, accept) against the model,
    child by child: valid, r1 and r2 directly outside borderline and edge rows, the state as in
    audit_run, the accept rule where scores were given.  `special`: rows counted apart from the
    cap (parents whose heading needs the Payne-Hanek reduction).  Returns the figures."""
    ch = np.asarray(out["children"], np.float32)
    par = np.asarray(parents, np.float32)
    k = len(ch)
    special = np.zeros(k, bool) if special is None else special
    replay = replay_point if agent == "point" else replay_car
    state, valid, bound, borderline = replay(par[:, :4], ch[:, 4:7], numDisc, L, W, H, boxes)
    got4 = ch[:, :4].astype(np.float64)
    r1, r2, _, edge, corners = bin_candidates(got4[:, 0], got4[:, 1], W, N, n)
    got_valid = np.asarray(out["valid"]) != 0
    sharp = ~borderline & ~edge
    assert np.array_equal(got_valid[~borderline], valid[~borderline]), "valid differs from the model"
    assert np.array_equal(np.asarray(out["r1"])[~edge], r1[~edge]), "r1 differs from the model"
    assert np.array_equal(np.asarray(out["r2"])[~edge], r2[~edge]), "r2 differs from the model"
    ok = ~borderline & np.isfinite(bound).all(axis=1) & np.isfinite(state).all(axis=1) & (bound[:, 2] < 0.1)
    err, bnd = np.abs(got4[ok] - state[ok]), bound[ok]
    with np.errstate(all="ignore"):
        ratio = np.where(err == 0, 0.0, err / bnd)
    ratio = np.where(np.isnan(ratio), np.inf, ratio)
    assert ok.sum() > k // 2 and not (ratio > 2.0).any(), f"state: worst ratio {ratio.max():.3g}"
    stats = dict(children=k, worst_ratio=float(ratio.max()), state_rows=int(ok.sum()),
                 borderline_share=float((borderline & ~special).sum()) / max(1, int((~special).sum())),
                 edge_share=float((edge & ~special).sum()) / max(1, int((~special).sum())),
                 special_share=float(((borderline | edge) & special).sum()) / max(1, int(special.sum())))
    assert stats["borderline_share"] <= cap and stats["edge_share"] <= cap, f"cap: {stats}"
    assert stats["special_share"] < 1.0 or not special.any(), f"cap: {stats}"
    if R1Score is not None:
        accept = np.asarray(out["accept"]) != 0
        in_grid = (np.asarray(out["r1"]) >= 0) & (np.asarray(out["r2"]) >= 0)
        assert not (accept & ~(got_valid & in_grid)).any(), "accept: an invalid or out-of-grid child accepted"
        clean = sharp & valid & (r2 >= 0)
        new_cell = clean & (np.asarray(R2Avail)[np.where(r2 >= 0, r2, 0)] == 0)
        assert new_cell.any() and accept[new_cell].all(), "accept: a valid child in an R2 cell with R2Avail == 0 rejected"
        lottery = clean & ~new_cell
        p = np.minimum(np.asarray(R1Score, np.float64)[np.where(r1 >= 0, r1, 0)][lottery], 1.0)
        sigma = float((p * (1 - p)).sum()) ** 0.5
        stats["lottery_sigmas"] = abs(int(accept[lottery].sum()) - float(p.sum())) / sigma
        assert stats["lottery_sigmas"] <= 5.0, f"accept: {int(accept[lottery].sum())} accepted, expected {p.sum():.1f} +- {sigma:.1f}"
    return stats


def audit_goal(tree, log, goal_idx, cost_to_goal, goal, radius):
    """A finished run that found a solution: the goal row lies inside the float64 goal radius
    and is the lowest row that does (the root is never tested, KGMT.cu:589), its parent chain
    reaches row 0 with falling indices, and its cost is the float64 sum of the durations on
    the chain within depth * u * cost.  Returns the chain, root first."""
    s, p, c = tree
    after = int(log[-1][LOG_AFTER])
    assert int(log[-1][LOG_BEFORE]) <= goal_idx < min(after, len(p)), "the goal row is not one of the last iteration's"
    r = float(np.float32(radius))
    d = np.hypot(s[:goal_idx + 1, 0].astype(np.float64) - float(np.float32(goal[0])),
                 s[:goal_idx + 1, 1].astype(np.float64) - float(np.float32(goal[1])))
    # float32: the two differences, the two squares, their sum and the root: under 4u relative
    assert d[goal_idx] < r * (1 + 4 * U), f"goal row {goal_idx} is {d[goal_idx]} from the goal"
    assert (d[1:goal_idx] >= r * (1 - 4 * U)).all(), f"row {1 + int(np.argmax(d[1:goal_idx] < r))} is inside the goal radius too"
    chain = [goal_idx]
    while chain[-1] != 0:
        nxt = int(p[chain[-1]])
        assert 0 <= nxt < chain[-1], f"parent of row {chain[-1]} is {nxt}"
        chain.append(nxt)
    chain = chain[::-1]
    total = float(s[chain[1:], 6].astype(np.float64).sum())
    depth = len(chain) - 1
    assert abs(float(c[goal_idx]) - total) <= depth * U * total, f"cost {c[goal_idx]} against {total}"
    assert float(np.float32(cost_to_goal)) == float(c[goal_idx])
    return chain
