"""GPU: paths and traces of a grown tree (k_path_walk, k_tree_trace; include/sbmp/tree_paths.h).

Step level: sbmp_tree_trace_batch and sbmp_tree_paths_batch against the model
(tests/tree_paths_model.py: exact float32 numpy and an explicit parent walk) and against the
host twins, bit for bit: every grown tree of tests/tree_recheck_cases.py, row and request counts
round the wave and workgroup sizes, a star one row longer than a full sweep of the grid, both
v / L forms and the IEEE fallback, the crafted cases, and one trace whose output passes 2^32
bytes.  Planner level: KGMT.solution_paths / trace / trajectories against the existing
solution_path and tree(), between steps, on a local shard group and on a batch member.
"""
import ctypes

import numpy as np
import pytest

import tree_recheck_cases as tc
from conftest import DEMO, DEMO_GOAL, DEMO_INITIAL, bits
from scenarios import BASE, BASE_SEED
from tree_paths_model import (BROKEN, DEEP, FREE, NONE, OK, ORPHAN, STALE, assert_same_paths, assert_same_trace,
                              euler_steps, paths_model, trace_model)
from tree_recheck_model import depths, tree_arrays

pytestmark = pytest.mark.gpu

EXTRA_KEYS = ("samplesPerIteration", "agent", "fixGNewClear", "batchRule")
SBMP_ERR_INVALID_ARGUMENT, SBMP_ERR_STATE = 1, 5
COUNTS = (1, 63, 64, 65, 255, 256, 257)


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


def trace_params(case):
    return {k: case.params[k] for k in ("numDisc", "agentLength", "agent")}


def trace(case, rows=None, **kw):
    from cudasbmp_amd import tree_trace_batch
    return tree_trace_batch(case.state, case.ctrl, case.parent, rows, **trace_params(case), **kw)


def paths(case, nodes, depthBound=0, **kw):
    from cudasbmp_amd import tree_paths_batch
    return tree_paths_batch(case.state, case.ctrl, case.parent, nodes, depthBound=depthBound, **kw)


def _check_trace(case, rows=None, host=True):
    want = trace_model(case.state, case.ctrl, case.parent, rows, **case.params)
    got = trace(case, rows)
    assert_same_trace(got, want, label=f"{case.name} device vs model")
    if host:
        assert_same_trace(got, trace(case, rows, device=False), label=f"{case.name} device vs host")
    return got


def _check_paths(case, nodes, depthBound=0):
    want = paths_model(case.state, case.ctrl, case.parent, nodes, depthBound)
    got = paths(case, nodes, depthBound)
    assert_same_paths(got, want, label=f"{case.name} device vs model")
    assert_same_paths(got, paths(case, nodes, depthBound, device=False), label=f"{case.name} device vs host")
    return got


# ---------------------------------------------------------------- trace, step level
@pytest.mark.parametrize("g", tc.GROWN, ids=tc.GROWN_IDS)
def test_trace_of_every_row_of_a_grown_tree(g):
    case = tc.grown(*g)
    steps, status = _check_trace(case)
    assert np.all(status == FREE)
    assert np.array_equal(bits(steps[:, -1]), bits(case.state))
    rows = np.random.default_rng(7).permutation(len(case.parent)).astype(np.int32)
    listed = _check_trace(case, rows)
    assert np.array_equal(bits(listed[0]), bits(steps[rows]))


@pytest.mark.parametrize("rows", COUNTS)
def test_trace_row_counts_round_the_wave_and_the_workgroup(rows):
    _check_trace(tc.grown(*tc.MAIN).prefix(rows))


def test_trace_one_row_more_than_a_full_grid_sweep():
    # at most 8 workgroups of 256 rows on each of an MI355X's 256 CUs: the last row is the one
    # row of the grid-stride loop's second round
    case = tc.star_case(256 * 8 * 256 + 1)
    assert case.params["numDisc"] == 10
    steps, status = _check_trace(case, host=False)
    assert status[-1] in (FREE, STALE) and (status == FREE).sum() > len(status) // 2 and (status == STALE).sum() >= 1


@pytest.mark.parametrize("L", [1.0, 1.3, 2.0, 0.5])
def test_trace_both_quotient_forms_and_the_ieee_fallback(L):
    """v / L as one multiply (L a power of two) and as the verified reciprocal (1.3); the star's
    root stands still, so every first step divides a v below 2^-100 and takes the IEEE division."""
    star = tc.star_case(257)
    assert star.state[0, 3] == 0.0
    _check_trace(star.with_(f"star-L{L:g}", params=dict(star.params, agentLength=L)))
    grown = tc.grown(*tc.MAIN).prefix(4097)
    _check_trace(grown.with_(f"grown-L{L:g}", params=dict(grown.params, agentLength=L)))


@pytest.mark.parametrize("build", [lambda: tc.stale_case(0), lambda: tc.stale_case(2), tc.d6_case] +
                         [lambda k=k: tc.parent_case(k) for k in tc.PARENT_KINDS],
                         ids=["stale-x", "stale-theta", "d6"] + [f"parent-{k}" for k in tc.PARENT_KINDS])
def test_trace_of_the_crafted_cases(build):
    case = build()
    _, status = _check_trace(case)
    if case.name.startswith("parent"):
        assert np.array_equal(np.flatnonzero(status == ORPHAN), np.array(sorted(tc.parent_rows())))
    elif case.name == "d6":
        assert np.all(status[993:] == ORPHAN)
    else:
        assert status[tc.busiest_row(*tc.MAIN)] == STALE


class _DevArray:
    """A device copy of a numpy array behind the two members a torch tensor is asked for."""

    def __init__(self, host):
        from cudasbmp_amd.batch import _Dev
        self._d = _Dev(host)
        self.shape = host.shape
        self.is_cuda = True

    def data_ptr(self):
        return self._d.ptr


def test_trace_offsets_past_4_gib():
    """4,194,305 rows x 64 steps x 16 B = 4.29 GB of steps through sbmp_tree_trace_batch with
    device pointers for the tree and the output: the last plane ends past 2^32 bytes.  The
    controls are 1,024 distinct triples tiled, so the model is computed for 1,024 rows and tiled.
    The first plane, the last plane, every ninth plane between and all status bytes are compared
    (read back plane by plane)."""
    from cudasbmp_amd import _native as nat
    from cudasbmp_amd import tree_trace_batch
    D, K, R = 64, 1024, 4194305
    rng = np.random.default_rng(64)
    triples = np.stack([rng.uniform(-5, 5, K), rng.uniform(-3.1, 3.1, K), rng.uniform(0.06, 1.05, K)], axis=1).astype(np.float32)
    root = np.array([5.0, 5.0, 0.3, 1.0], np.float32)
    model = euler_steps(np.broadcast_to(root, (K, 4)), triples, D, 1.0, "car")       # (K, D, 4)
    model[7, -1, 0] = np.nextafter(model[7, -1, 0], np.float32(np.inf))               # one stored row a float off: STALE
    state = np.concatenate([root[None], np.tile(model[:, -1], ((R - 1) // K, 1))])
    model[7, -1, 0] = np.nextafter(model[7, -1, 0], np.float32(-np.inf))
    ctrl = np.zeros((R, 4), np.float32)
    ctrl[1:, :3] = np.tile(triples, ((R - 1) // K, 1))
    parent = np.zeros(R, np.int32)
    parent[0] = -1
    assert D * R * 16 - 2 ** 32 == 64 * 16     # the last plane's last 64 entries lie past 2^32 bytes: with 32-bit
    #                                            byte offsets they would land on the first plane's first 64
    tree = [_DevArray(a) for a in (state, ctrl, parent)]
    p = ctypes.c_void_p()
    nat.call("sbmp_device_alloc", D * R * 16 + R, ctypes.byref(p))
    try:
        steps_ptr, status_ptr = p.value, p.value + D * R * 16
        tree_trace_batch(*tree, numDisc=D, agentLength=1.0, agent="car", out=(steps_ptr, status_ptr))
        plane = np.zeros((R, 4), np.float32)
        for j in sorted(set([0, D - 1]) | set(range(0, D, 9))):
            nat.call("sbmp_device_copy_from", plane.ctypes.data_as(ctypes.c_void_p), ctypes.c_void_p(steps_ptr + j * R * 16),
                     plane.nbytes)
            assert np.array_equal(bits(plane[0]), bits(root)), f"plane {j}: the root"
            assert np.array_equal(bits(plane[1:]).reshape(-1, K, 4), np.broadcast_to(bits(model[:, j]), ((R - 1) // K, K, 4))), \
                f"plane {j}"
        status = np.zeros(R, np.uint8)
        nat.call("sbmp_device_copy_from", status.ctypes.data_as(ctypes.c_void_p), ctypes.c_void_p(status_ptr), R)
        want = np.zeros(R, np.uint8)
        want[8::K] = STALE
        assert np.array_equal(status, want)
    finally:
        nat.call("sbmp_device_free", p)
        for t in tree:
            t._d.close()


# ---------------------------------------------------------------- paths, step level
@pytest.mark.parametrize("depth", tc.CHAIN_DEPTHS)
def test_paths_depth_bound_at_the_chain_length_and_one_less(depth):
    case = tc.chain_case(depth, "last")
    got = _check_paths(case, [depth], depthBound=depth + 1)
    assert got["status"].tolist() == [OK] and np.array_equal(got["rows"], np.arange(depth + 1))
    short = _check_paths(case, [depth], depthBound=depth)
    assert short["status"].tolist() == [DEEP] and short["lengths"].tolist() == [0]


@pytest.mark.parametrize("count", COUNTS)
def test_paths_request_counts_round_the_wave_and_the_workgroup(count):
    case = tc.grown(*tc.MAIN)
    nodes = np.random.default_rng(count).integers(-1, len(case.parent), count).astype(np.int32)
    nodes[0] = int(np.argmax(depths(case.parent)))
    _check_paths(case, nodes)


def test_paths_of_every_row_at_once():
    case = tc.grown(*tc.MAIN)
    R = len(case.parent)
    got = _check_paths(case, np.arange(R, dtype=np.int32))
    assert R > 20000 and np.all(got["status"] == OK) and np.array_equal(got["lengths"], depths(case.parent) + 1)


@pytest.mark.parametrize("build", [tc.d6_case] + [lambda k=k: tc.parent_case(k) for k in tc.PARENT_KINDS],
                         ids=["d6"] + [f"parent-{k}" for k in tc.PARENT_KINDS])
def test_paths_of_the_crafted_cases(build):
    case = build()
    got = _check_paths(case, np.arange(-1, len(case.parent), dtype=np.int32))
    assert got["status"][0] == NONE and (got["status"] == BROKEN).sum() >= 4


def test_two_calls_give_identical_bytes():
    case = tc.parent_case("minus1")
    nodes = np.arange(-1, len(case.parent), dtype=np.int32)
    a, b = paths(case, nodes), paths(case, nodes)
    assert all(a[k].tobytes() == b[k].tobytes() for k in a)
    rows = np.random.default_rng(3).integers(0, len(case.parent), 30001).astype(np.int32)
    (s0, b0), (s1, b1) = trace(case, rows), trace(case, rows)
    assert np.ascontiguousarray(s0).tobytes() == np.ascontiguousarray(s1).tobytes() and b0.tobytes() == b1.tobytes()


# ---------------------------------------------------------------- planner level
def _tree_of(g):
    s, p, c = g.tree()
    return tree_arrays(s, p, c, g.result().treeSize)


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_paths_and_trajectories_of_the_demo_plan(seed, obstacles):
    g = _mk()
    r = g.plan(DEMO_INITIAL, DEMO_GOAL, _dev(obstacles), len(obstacles), seed=seed)
    assert r.goalIndex > 0
    state, ctrl, parent = _tree_of(g)
    R = len(parent)
    nodes = np.concatenate([[r.goalIndex, 0], np.random.default_rng(seed).integers(0, R, 64)]).astype(np.int32)
    got = g.solution_paths(nodes)
    assert_same_paths(got, paths_model(state, ctrl, parent, nodes, DEMO["numIterations"] + 2), label=f"seed {seed}")
    assert np.all(got["status"] == OK)
    for i, node in enumerate(nodes):
        rows, s, c = g.solution_path(int(node))
        a, b = got["offsets"][i], got["offsets"][i + 1]
        assert np.array_equal(got["rows"][a:b], rows), (i, node)
        assert np.array_equal(bits(got["samples"][a:b]), bits(s)) and np.array_equal(bits(got["costs"][a:b]), bits(c))
    # the whole tree's trace is the model's, and ends on tree()'s rows
    steps, status = g.trace()
    assert_same_trace((steps, status), trace_model(state, ctrl, parent, numDisc=DEMO["numDisc"], agentLength=DEMO["agentLength"]),
                      label=f"seed {seed} trace")
    assert np.all(status == FREE) and np.array_equal(bits(steps[:, -1]), bits(state))
    goals = np.array([[DEMO_GOAL[0], DEMO_GOAL[1], 0.5], [5.0, 5.0, 0.5], [19.9, 0.1, 0.001], [12.0, 3.0, 2.0], [-3.0, -3.0, 0.5],
                      [9.0, 7.0, 0.5]], np.float32)
    best = g.query_goals(goals)["bestRow"]
    assert (best == -1).sum() >= 2 and (best >= 0).sum() >= 2
    t = g.trajectories(best)
    assert np.array_equal(t["status"] == NONE, best == -1) and np.all(t["status"][best >= 0] == OK)
    assert t["steps"].shape == (len(t["rows"]), DEMO["numDisc"], 4) and np.all(t["step_status"] == FREE)
    for i, node in enumerate(best):
        if node >= 0:
            last = t["offsets"][i + 1] - 1
            assert t["rows"][last] == node and np.array_equal(bits(t["steps"][last, -1]), bits(state[node]))
    assert np.array_equal(bits(t["steps"]), bits(steps[t["rows"]]))


def test_paths_and_traces_between_steps_change_nothing(obstacles):
    kw = dict(BASE)

    def run(ask):
        g = _mk(**kw)
        g.begin(DEMO_INITIAL, DEMO_GOAL, _dev(obstacles), len(obstacles), BASE_SEED)
        seen = []
        for _ in range(2):
            g.step(3)
            if ask:
                state, ctrl, parent = _tree_of(g)
                nodes = np.arange(-1, len(parent), 37, dtype=np.int32)
                assert_same_paths(g.solution_paths(nodes), paths_model(state, ctrl, parent, nodes, BASE["numIterations"] + 2),
                                  label="between steps")
                got = g.trace()
                assert_same_trace(got, trace_model(state, ctrl, parent, numDisc=g.numDisc_, agentLength=g.agentLength_,
                                                   agent=kw.get("agent", "car")), label="between steps")
                seen.append(len(got[1]))
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
    state, ctrl, parent = _tree_of(single)
    nodes = np.arange(-1, len(parent), 101, dtype=np.int32)
    rows = nodes[1:][::-1].copy()
    want_p = single.solution_paths(nodes)
    want_t = single.trace(rows)
    assert_same_paths(want_p, paths_model(state, ctrl, parent, nodes, BASE["numIterations"] + 2), label="single")
    assert_same_trace(want_t, trace_model(state, ctrl, parent, rows, numDisc=single.numDisc_, agentLength=single.agentLength_,
                                          agent=kw.get("agent", "car")), label="single")
    group = _mk(_local_group=2, **kw)
    group.plan(DEMO_INITIAL, DEMO_GOAL, d, len(obstacles), seed=BASE_SEED)
    assert_same_paths(group.solution_paths(nodes), want_p, label="local group of 2")
    assert_same_trace(group.trace(rows), want_t, label="local group of 2")
    cfg, extra = _split(kw)
    b = KGMTBatch(2, **cfg, **extra)
    b.plan([DEMO_INITIAL] * 2, [DEMO_GOAL] * 2, d, len(obstacles), [BASE_SEED + 1, BASE_SEED])
    assert_same_paths(b[1].solution_paths(nodes), want_p, label="batch member 1")
    assert_same_trace(b[1].trace(rows), want_t, label="batch member 1")
    t = b[1].trajectories(nodes[1:4])
    assert np.array_equal(bits(t["steps"][:, -1]), bits(state[t["rows"]]))
    assert_same_trace(b[1].trace(), single.trace(), label="batch member 1, every row")


def test_state_and_argument_errors(obstacles):
    from cudasbmp_amd import SbmpError
    from cudasbmp_amd import _native as nat
    g = _mk(**BASE)
    d = _dev(obstacles)

    def status_of(f):
        with pytest.raises(SbmpError) as e:
            f()
        return e.value.status

    assert status_of(lambda: g.solution_paths([0])) == SBMP_ERR_STATE          # before the first begin()
    assert status_of(lambda: g.trace([0])) == SBMP_ERR_STATE
    g.begin(DEMO_INITIAL, DEMO_GOAL, d, len(obstacles), BASE_SEED)
    g.step(3)
    R = min(g.result().treeSize, g.M)
    assert R > 1
    assert status_of(lambda: g.solution_paths([0, -2])) == SBMP_ERR_INVALID_ARGUMENT
    assert status_of(lambda: g.solution_paths([R])) == SBMP_ERR_INVALID_ARGUMENT
    assert status_of(lambda: g.trace([R])) == SBMP_ERR_INVALID_ARGUMENT
    assert status_of(lambda: g.trace([-1])) == SBMP_ERR_INVALID_ARGUMENT
    assert g.solution_paths([R - 1, -1])["status"].tolist() == [OK, NONE]
    assert len(g.solution_paths([])["rows"]) == 0 and g.trace([])[0].shape == (0, g.numDisc_, 4)   # count 0: no-ops
    L = nat.lib()
    total = ctypes.c_longlong(-1)
    nodes = np.array([R - 1, R - 1], np.int32)
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    assert L.sbmp_kgmt_solution_paths(g._h, vp(nodes), 2, None, None, None, None, None, 0, ctypes.byref(total)) == 0
    T = total.value
    assert T >= 4
    small = np.zeros(T - 1, np.int32)
    total.value = -1
    assert L.sbmp_kgmt_solution_paths(g._h, vp(nodes), 2, None, None, vp(small), None, None, T - 1,
                                      ctypes.byref(total)) == SBMP_ERR_INVALID_ARGUMENT
    assert total.value == T                                                     # set in every case
    assert L.sbmp_kgmt_trace_rows(g._h, None, R + 1, vp(np.zeros(4, np.float32)), None) == SBMP_ERR_INVALID_ARGUMENT
    assert L.sbmp_kgmt_trace_rows(g._h, None, R, None, None) == SBMP_ERR_INVALID_ARGUMENT
