"""GPU: solution paths resampled at a fixed period (k_resample_clock, k_path_resample;
include/sbmp/tree_resample.h).

Step level: sbmp_tree_resample_batch against the model (tests/tree_resample_model.py) and against
the host twin, bit for bit: grown trees, sample totals and request counts round the wave and the
workgroup sizes, the crafted chains, both v / L forms and the IEEE fallback, mixed statuses, 715
requests whose samples pass one sweep of k_path_resample's grid (524,288 samples at most), and one
path whose state array passes 2^32 bytes.  Planner level: KGMT.resample against the model over
tree(), between steps, on a local shard group and on a batch member.

A total of 1 sample cannot occur: a path has at least two samples (the rule's n = floor(T / period)
+ 2), so the totals start at 2.
"""
import ctypes

import numpy as np
import pytest

import tree_recheck_cases as tc
import tree_resample_cases as rc
from conftest import DEMO, DEMO_GOAL, DEMO_INITIAL, bits
from scenarios import BASE, BASE_SEED
from tree_paths_model import BROKEN, DEEP, NONE, OK, path_of, trace_model
from tree_recheck_model import tree_arrays
from tree_resample_model import assert_same_resample, resample_model

pytestmark = pytest.mark.gpu

EXTRA_KEYS = ("samplesPerIteration", "agent", "fixGNewClear", "batchRule")
SBMP_ERR_INVALID_ARGUMENT, SBMP_ERR_STATE = 1, 5
TOTALS = (2, 63, 64, 65, 255, 256, 257)


@pytest.fixture(scope="module", autouse=True)
def _oracle(oracle_lib):
    return oracle_lib


def _split(kw):
    cfg = dict(DEMO)
    kw = dict(kw)
    extra = {k: kw.pop(k) for k in EXTRA_KEYS if k in kw}
    cfg.update(kw)
    return cfg, extra


def _mk(_local_group=0, **kw):
    from cudasbmp_amd import KGMT
    cfg, extra = _split(kw)
    return KGMT(**cfg, **extra, _local_group=_local_group)


def _dev(obs):
    from cudasbmp_amd import DeviceBuffer
    return DeviceBuffer(obs)


def resample(case, nodes, period, depthBound=0, device=True):
    from cudasbmp_amd import tree_resample_batch
    return tree_resample_batch(case.state, case.ctrl, case.parent, nodes, period, depthBound=depthBound, device=device,
                               **rc.params_of(case))


def check(case, nodes, period, depthBound=0):
    want = resample_model(case.state, case.ctrl, case.parent, nodes, period, depth_bound=depthBound, details=True,
                          **rc.params_of(case))
    got = resample(case, nodes, period, depthBound)
    assert_same_resample(got, want, label=f"{case.name} device vs model")
    assert_same_resample(got, resample(case, nodes, period, depthBound, device=False), label=f"{case.name} device vs host")
    return got, want


# ---------------------------------------------------------------- step level
@pytest.mark.parametrize("period", rc.PERIODS, ids=rc.PERIOD_IDS)
@pytest.mark.parametrize("g", [tc.MAIN, ("car", 1.3, 13), ("point", 1.0, 10)], ids=["car-L1-D10", "car-L1.3-D13", "point-L1-D10"])
def test_resample_of_a_grown_tree(g, period):
    case = tc.grown(*g)
    got, _ = check(case, rc.nodes_of(case), period)
    assert np.all(got["status"] == OK) and len(got["times"]) > 1000


@pytest.mark.parametrize("total", TOTALS)
def test_sample_totals_round_the_wave_and_the_workgroup(total):
    case = rc.pow2(7)
    got, _ = check(case, [6], rc.period_for_total(6.0, total))
    assert got["counts"].tolist() == [total] and len(got["times"]) == total


@pytest.mark.parametrize("count", rc.COUNTS)
def test_request_counts_round_the_wave_and_the_workgroup(count):
    case = tc.star_case(257)
    nodes = np.random.default_rng(count).integers(-1, 257, count).astype(np.int32)
    nodes[-1] = 256
    got, _ = check(case, nodes, 0.05)
    assert np.array_equal(got["status"] == NONE, nodes == -1)


@pytest.mark.parametrize("L", rc.CHAIN_LENGTHS)
def test_chains_of_every_size_class(L):
    case = rc.chain(L)
    for period in rc.PERIODS[:2]:
        got, _ = check(case, [L - 1], period)
        assert got["status"].tolist() == [OK] and got["counts"][0] >= 2
        assert L == 1 or set(got["edges"].tolist()) == set(range(1, L))


@pytest.mark.parametrize("period", [0.05, 0.013, 0.3, 1e-3])
def test_bad_durations_add_no_time_and_are_never_selected(period):
    case = rc.bad_durations()
    got, want = check(case, [len(case.parent) - 1], period)
    assert not np.isin(got["edges"], rc.BAD_ROWS).any() and got["edges"][0] == rc.DENORMAL_ROW
    assert want["dt"][0] == 0.0 and want["j"][0] == case.params["numDisc"] - 1


@pytest.mark.parametrize("agent", ["car", "point"])
def test_power_of_two_durations_land_on_step_and_edge_boundaries(agent):
    case = rc.pow2(7, agent)
    steps, _ = trace_model(case.state, case.ctrl, case.parent, **case.params)
    stored = case.state if agent == "car" else case.state * np.array([1, 1, 0, 0], np.float32)
    got, want = check(case, [6], 0.125)
    assert got["counts"].tolist() == [50] and np.all(want["alpha"] == 0.0)
    for m in range(48):
        k, j = m // 8 + 1, m % 8
        assert got["edges"][m] == k and np.all(got["states"][m] == (stored[k - 1] if j == 0 else steps[k, j - 1])), m
    got, _ = check(case, [6], 1.0)
    assert got["edges"].tolist() == [1, 2, 3, 4, 5, 6, 6, 6] and np.all(got["states"][:6] == stored[:6])
    assert np.array_equal(bits(got["states"][6:]), bits(case.state[[6, 6]]))
    got, _ = check(case, [6], 100.0)                                   # a period longer than the path
    assert got["counts"].tolist() == [2] and np.all(got["states"][0] == stored[0])
    assert np.array_equal(bits(got["states"][1]), bits(case.state[6]))


def test_a_last_grid_time_that_rounds_past_the_path_is_an_end_sample():
    case = rc.rounding()
    m = rc.ROUNDING_GRID
    got, _ = check(case, [1], rc.ROUNDING_PERIOD)
    assert got["counts"].tolist() == [m + 2] and got["times"][m] == float(rc.ROUNDING_DURATION) > got["times"][m - 1]
    assert np.array_equal(bits(got["states"][m:]), bits(case.state[[1, 1]]))


@pytest.mark.parametrize("L", [1.0, 1.3, 2.0, 0.5])
def test_both_quotient_forms_and_the_ieee_fallback(L):
    """v / L as one multiply (L a power of two) and as the verified reciprocal (1.3); the star's
    root stands still, so every first step divides a v below 2^-100 and takes the IEEE division."""
    star = tc.star_case(257)
    assert star.state[0, 3] == 0.0
    case = star.with_(f"star-L{L:g}", params=dict(star.params, agentLength=L))
    check(case, np.arange(-1, 257, dtype=np.int32), 0.013)
    grown = tc.grown(*tc.MAIN).prefix(4097)
    case = grown.with_(f"grown-L{L:g}", params=dict(grown.params, agentLength=L))
    check(case, np.arange(0, 4097, 41, dtype=np.int32), 0.05)


def test_the_point_agent_on_a_star():
    star = tc.star_case(257)
    case = star.with_("star-point", params=dict(star.params, agent="point"))
    got, want = check(case, np.arange(0, 257, dtype=np.int32), 0.05)
    grid = want["from"] >= 0
    assert grid.sum() > 1000 and np.all(got["states"][grid][:, 2:] == 0.0)


def test_statuses_mixed_among_ok_requests():
    case = tc.parent_case("minus1")
    busiest = tc.busiest_row(*tc.MAIN)
    child = int(np.flatnonzero(tc.grown(*tc.MAIN).parent == busiest)[0])
    R = len(case.parent)
    high = next(r for r in range(R - 2, 0, -1) if path_of(case.parent.tolist(), r, R)[0] == OK)   # a late row with a path
    nodes = np.array([7, -1, busiest, 9, child, -1, 0, high], np.int32)
    got, _ = check(case, nodes, 0.05)
    assert got["status"].tolist() == [OK, NONE, BROKEN, OK, BROKEN, NONE, OK, OK]
    o = got["offsets"]
    assert np.all(got["counts"][[1, 2, 4, 5]] == 0) and o[1] == o[2] == o[3] and o[4] == o[5] == o[6]
    for i in (0, 3, 6, 7):                     # the ok requests' samples sit at their offsets
        assert got["edges"][o[i + 1] - 1] == nodes[i] and got["times"][o[i]] == 0.0
        assert np.array_equal(bits(got["states"][o[i + 1] - 1]), bits(case.state[nodes[i]]))
    deep = rc.chain(65)
    got, _ = check(deep, [64, 63, 64, 0], 0.05, depthBound=64)
    assert got["status"].tolist() == [DEEP, OK, DEEP, OK] and got["counts"][[0, 2]].tolist() == [0, 0]


def test_two_calls_give_identical_bytes():
    case = tc.grown(*tc.MAIN)
    nodes = np.arange(-1, len(case.parent), 53, dtype=np.int32)
    a, b = resample(case, nodes, 0.013), resample(case, nodes, 0.013)
    assert all(a[k].tobytes() == b[k].tobytes() for k in a) and len(a["times"]) > 10000


def test_many_requests_whose_samples_pass_one_grid_sweep():
    """About 700 requests, -1 and broken ones among them, 576,712 samples: k_path_resample's lanes
    of the second sweep bisect the sample offsets for the last twenty requests.  The picked form is
    taken (the full model takes 0.9 s on the CPU, several times any other test of this file): the
    model gives every request's first and last 64 samples, and every sample of the requests that
    hold the offsets SWEEP - 64 .. SWEEP + 64 and total - 64 .. total.  Every sample is compared
    with the host twin, which tests/test_tree_resample.py holds to the full model on this case."""
    case, nodes, period = rc.many_requests()
    kw = rc.params_of(case)
    ends = lambda n: sorted(set(range(min(64, n))) | set(range(max(0, n - 64), n)))
    want = resample_model(case.state, case.ctrl, case.parent, nodes, period, pick=ends, **kw)
    got = resample(case, nodes, period)
    assert_same_resample(got, resample(case, nodes, period, device=False), label="device vs host")
    off, total = want["offsets"], int(want["offsets"][-1])
    assert rc.SWEEP + 1000 <= total <= 1.2 * rc.SWEEP and len(got["times"]) == total

    def part(requests, samples):
        idx = np.concatenate(samples).astype(np.int64)
        n = got["counts"][requests]
        return {"counts": n, "status": got["status"][requests], "offsets": np.concatenate([[0], np.cumsum(n, dtype=np.int64)]),
                "states": got["states"][idx], "edges": got["edges"][idx], "times": got["times"][idx]}

    every = np.arange(len(nodes))
    picked = part(every, [off[i] + np.array(ends(int(want["counts"][i])), np.int64) for i in every])
    assert_same_resample(dict(picked, offsets=got["offsets"]), want, label="device vs model, the ends of every request")
    holds = lambda a, b: np.flatnonzero((off[:-1] <= b) & (off[1:] > a) & (want["counts"] > 0))
    whole = np.union1d(holds(rc.SWEEP - 64, rc.SWEEP + 64), holds(total - 64, total - 1))
    assert 2 <= len(whole) <= 4 and off[whole[0]] < rc.SWEEP - 64 and off[whole[-1] + 1] == total
    full = resample_model(case.state, case.ctrl, case.parent, nodes[whole], period, **kw)
    assert_same_resample(part(whole, [np.arange(off[i], off[i + 1]) for i in whole]), full, label="device vs model, whole requests")
    assert 650 <= len(nodes) <= 750 and len(np.unique(nodes[nodes >= 0])) == (nodes >= 0).sum()
    status = want["status"]
    assert (status == NONE).sum() >= 10 and (status == BROKEN).sum() >= 10 and (status == OK).sum() >= 600
    past = np.flatnonzero((want["offsets"][1:] > rc.SWEEP) & (want["counts"] > 0))      # requests with a sample past the sweep
    assert len(past) >= 10 and past[0] > 600 and (status[past[0]:] != OK).any()
    assert (want["counts"][past] >= 2).all() and want["offsets"][past[0]] < rc.SWEEP       # one request straddles it


class _DevArray:
    """A device copy of a numpy array."""

    def __init__(self, host):
        from cudasbmp_amd.batch import _Dev
        self._d = _Dev(host)
        self.ptr = self._d.ptr


def test_sample_offsets_past_4_gib():
    """One path of 2^28 + 1 samples through sbmp_tree_resample_batch with device outputs: the state
    array is 2^32 + 16 bytes, so its last entry lies past 2^32 bytes (with 32-bit byte offsets it
    would land on the first).  The first 4,096 and the last 4,096 samples of each array are copied
    back and compared with the model."""
    from cudasbmp_amd import _native as nat
    case = rc.pow2(7)
    N, K = 2 ** 28 + 1, 4096
    period = rc.period_for_total(6.0, N)
    want = resample_model(case.state, case.ctrl, case.parent, [6], period, **rc.params_of(case),
                          pick=lambda n: list(range(K)) + list(range(n - K, n)))
    assert want["counts"].tolist() == [N] and len(want["times"]) == 2 * K and N * 16 == 2 ** 32 + 16
    p = ctypes.c_void_p()
    try:
        nat.call("sbmp_device_alloc", N * 28, ctypes.byref(p))
    except nat.SbmpError as e:
        pytest.skip(f"no {N * 28 / 2 ** 30:.1f} GiB of device memory for the sample arrays: {e}")
    tree = [_DevArray(a) for a in (case.state, case.ctrl, case.parent)]
    try:
        states_ptr, times_ptr, edges_ptr = p.value, p.value + N * 16, p.value + N * 24
        a = nat.TreePathsArgs()
        a.state, a.ctrl, a.parent = (t.ptr for t in tree)
        a.rows, a.depthBound, a.agent, a.numDisc, a.agentLength = 7, 0, nat.SBMP_AGENT_CAR, 8, 1.0
        nodes, counts, status = np.array([6], np.int32), np.zeros(1, np.int32), np.zeros(1, np.uint8)
        total = ctypes.c_longlong()
        vp = lambda x: x.ctypes.data_as(ctypes.c_void_p)
        nat.call("sbmp_tree_resample_batch", ctypes.byref(a), vp(nodes), 1, ctypes.c_double(period), vp(counts), vp(status),
                 ctypes.c_void_p(states_ptr), ctypes.c_void_p(edges_ptr), ctypes.c_void_p(times_ptr), N,
                 ctypes.byref(total), None)
        assert total.value == N and counts.tolist() == [N] and status.tolist() == [OK]
        got = {"counts": counts, "status": status, "offsets": np.array([0, N], np.int64),
               "states": np.zeros((2 * K, 4), np.float32), "edges": np.zeros(2 * K, np.int32), "times": np.zeros(2 * K, np.float64)}
        for name, base, size in (("states", states_ptr, 16), ("edges", edges_ptr, 4), ("times", times_ptr, 8)):
            for half, first in ((0, 0), (1, N - K)):
                dst = got[name][half * K:(half + 1) * K]
                nat.call("sbmp_device_copy_from", vp(dst), ctypes.c_void_p(base + first * size), dst.nbytes)
        assert_same_resample(got, want, label="2^28 + 1 samples")
        assert got["edges"][-1] == 6 and got["times"][-1] == 6.0 and np.array_equal(bits(got["states"][-1]), bits(case.state[6]))
    finally:
        nat.call("sbmp_device_free", p)
        for t in tree:
            t._d.close()


# ---------------------------------------------------------------- planner level
def _tree_of(g):
    s, p, c = g.tree()
    return tree_arrays(s, p, c, g.result().treeSize)


def _model_of(g, nodes, period, numIterations, agent="car"):
    state, ctrl, parent = _tree_of(g)
    return resample_model(state, ctrl, parent, nodes, period, depth_bound=numIterations + 2, numDisc=g.numDisc_,
                          agentLength=g.agentLength_, agent=agent)


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_resample_of_the_demo_plan(seed, obstacles):
    g = _mk()
    r = g.plan(DEMO_INITIAL, DEMO_GOAL, _dev(obstacles), len(obstacles), seed=seed)
    assert r.goalIndex > 0
    goals = np.array([[DEMO_GOAL[0], DEMO_GOAL[1], 0.5], [5.0, 5.0, 0.5], [19.9, 0.1, 0.001], [12.0, 3.0, 2.0], [-3.0, -3.0, 0.5],
                      [9.0, 7.0, 0.5]], np.float32)
    best = g.query_goals(goals)["bestRow"]
    assert (best == -1).sum() >= 2 and (best >= 0).sum() >= 2
    got = g.resample(best, 0.01)
    assert_same_resample(got, _model_of(g, best, 0.01, DEMO["numIterations"]), label=f"seed {seed}")
    assert np.array_equal(got["status"] == NONE, best == -1) and np.all(got["status"][best >= 0] == OK)
    assert got["states"].shape == (got["offsets"][-1], 4) and got["times"].dtype == np.float64


def test_resample_between_steps_changes_nothing(obstacles):
    kw = dict(BASE)

    def run(ask):
        g = _mk(**kw)
        g.begin(DEMO_INITIAL, DEMO_GOAL, _dev(obstacles), len(obstacles), BASE_SEED)
        seen = []
        for _ in range(2):
            g.step(3)
            if ask:
                R = min(g.result().treeSize, g.M)
                nodes = np.arange(-1, R, 37, dtype=np.int32)
                got = g.resample(nodes, 0.05)
                assert_same_resample(got, _model_of(g, nodes, 0.05, BASE["numIterations"], kw.get("agent", "car")),
                                     label="between steps")
                seen.append(len(got["times"]))
        while g.step(4):
            pass
        return g, seen

    g0, _ = run(False)
    g1, seen = run(True)
    assert 1 < seen[0] < seen[1]
    assert g1.state_hash() == g0.state_hash()
    for x, y in zip(g1.tree(), g0.tree()):
        assert np.array_equal(bits(x), bits(y))
    r0, r1 = g0.result(), g1.result()
    assert (r1.iterations, r1.treeSize, r1.accepted) == (r0.iterations, r0.treeSize, r0.accepted)


def test_local_group_and_batch_member_answer_as_one_planner(obstacles):
    from cudasbmp_amd import KGMTBatch
    kw = dict(BASE)
    d = _dev(obstacles)
    single = _mk(**kw)
    single.plan(DEMO_INITIAL, DEMO_GOAL, d, len(obstacles), seed=BASE_SEED)
    R = min(single.result().treeSize, single.M)
    nodes = np.arange(-1, R, 101, dtype=np.int32)
    want = single.resample(nodes, 0.013)
    assert_same_resample(want, _model_of(single, nodes, 0.013, BASE["numIterations"], kw.get("agent", "car")), label="single")
    group = _mk(_local_group=2, **kw)
    group.plan(DEMO_INITIAL, DEMO_GOAL, d, len(obstacles), seed=BASE_SEED)
    got = group.resample(nodes, 0.013)
    assert all(got[k].tobytes() == want[k].tobytes() for k in want), "local group of 2"
    cfg, extra = _split(kw)
    b = KGMTBatch(2, **cfg, **extra)
    b.plan([DEMO_INITIAL] * 2, [DEMO_GOAL] * 2, d, len(obstacles), [BASE_SEED + 1, BASE_SEED])
    got = b[1].resample(nodes, 0.013)
    assert all(got[k].tobytes() == want[k].tobytes() for k in want), "batch member 1"


def test_state_and_argument_errors(obstacles):
    from cudasbmp_amd import SbmpError
    from cudasbmp_amd import _native as nat
    g = _mk(**BASE)
    d = _dev(obstacles)

    def status_of(f):
        with pytest.raises(SbmpError) as e:
            f()
        return e.value.status

    assert status_of(lambda: g.resample([0], 0.05)) == SBMP_ERR_STATE           # before the first begin()
    g.begin(DEMO_INITIAL, DEMO_GOAL, d, len(obstacles), BASE_SEED)
    g.step(3)
    R = min(g.result().treeSize, g.M)
    assert R > 1
    for bad in (0.0, -0.05, float("nan"), float("inf")):
        assert status_of(lambda: g.resample([0], bad)) == SBMP_ERR_INVALID_ARGUMENT
    assert status_of(lambda: g.resample([0, -2], 0.05)) == SBMP_ERR_INVALID_ARGUMENT
    assert status_of(lambda: g.resample([R], 0.05)) == SBMP_ERR_INVALID_ARGUMENT
    assert g.resample([R - 1, -1], 0.05)["status"].tolist() == [OK, NONE]
    assert len(g.resample([], 0.05)["times"]) == 0                               # count 0: a no-op
    L = nat.lib()
    total = ctypes.c_longlong(-1)
    nodes = np.array([R - 1, R - 1], np.int32)
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    assert L.sbmp_kgmt_resample_paths(g._h, vp(nodes), 2, 0.05, None, None, None, None, None, 0, ctypes.byref(total)) == 0
    T = total.value
    assert T >= 4
    small = np.zeros(T - 1, np.int32)
    total.value = -1
    assert L.sbmp_kgmt_resample_paths(g._h, vp(nodes), 2, 0.05, None, None, None, vp(small), None, T - 1,
                                      ctypes.byref(total)) == SBMP_ERR_INVALID_ARGUMENT
    assert total.value == T                                                      # set in every case
    assert L.sbmp_kgmt_resample_paths(g._h, vp(nodes), 2, 0.05, None, None, None, None, None, 0, None) == SBMP_ERR_INVALID_ARGUMENT
    # T / period at 2^31 - 2 and beyond, through both device entry points
    tiny = 1e-12
    assert status_of(lambda: g.resample([R - 1], tiny)) == SBMP_ERR_INVALID_ARGUMENT
    case = rc.chain(4)
    assert status_of(lambda: resample(case, [3], tiny)) == SBMP_ERR_INVALID_ARGUMENT
    assert status_of(lambda: resample(case, [4], 0.05)) == SBMP_ERR_INVALID_ARGUMENT
    assert status_of(lambda: resample(case, [-2], 0.05)) == SBMP_ERR_INVALID_ARGUMENT
    assert status_of(lambda: resample(case, [3], 0.0)) == SBMP_ERR_INVALID_ARGUMENT
