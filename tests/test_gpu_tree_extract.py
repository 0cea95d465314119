"""GPU: the tree extraction, prune and re-root (k_extract_mark, k_extract_jump, k_extract_count,
k_extract_offsets, k_extract_number, k_extract_gather; include/sbmp/tree_extract.h).

Step level: sbmp_tree_extract_batch against the model (tests/tree_extract_model.py) and against the
host twin, bit for bit, on the whole table of tests/tree_extract_cases.py: grown trees, chains, a
star, row counts round the wave, the workgroup, the tile and one full round of the offsets
workgroup, every mask, root and crafted parent; then the commutation laws through the device
entries, and two calls byte for byte.  Planner level: KGMT.extract against the model over tree(),
after a re-check, re-rooted on the solution path, between steps, on a local shard group and on a
batch member.

The table's rows-sweep+77, rows-2sweep+1, rows-tiles+1 and root-past-sweep cases take every
grid-stride loop of the six kernels past its first round (one sweep is at most 524,288 rows, 2,048
tiles; fewer resident workgroups only start the later rounds sooner) and k_extract_offsets to nine
rounds; tests/test_tree_pass_seams_oracle.py shows on the CPU which broken loops they catch.

Trees of 2^28 rows and more, where 16 x row passes 2^32, are not run here: they do not fit in a few
seconds.
"""
import ctypes

import numpy as np
import pytest

import tree_extract_cases as xc
import tree_extract_laws as laws
import tree_recheck_cases as tc
from conftest import DEMO, DEMO_GOAL, DEMO_INITIAL, bits
from scenarios import BASE, BASE_SEED, demo_plus
from tree_extract_model import assert_same_extract, extract_model, u32
from tree_recheck_model import depths, descendants, tree_arrays

pytestmark = pytest.mark.gpu

EXTRA_KEYS = ("samplesPerIteration", "agent", "fixGNewClear", "batchRule")
SBMP_ERR_INVALID_ARGUMENT, SBMP_ERR_STATE = 1, 5


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


def extract(c, device=True, **kw):
    from cudasbmp_amd import tree_extract_batch
    return tree_extract_batch(c.state, c.ctrl, c.parent, root=c.root, keep=c.keep, device=device, **kw)


# ---------------------------------------------------------------- step level
@pytest.mark.parametrize("cid", xc.IDS)
def test_device_is_the_model_and_the_twin(cid):
    c = xc.case(cid)
    got = extract(c)
    assert_same_extract(got, c.model, label=f"{c.name} device vs model")
    assert_same_extract(got, extract(c, device=False), label=f"{c.name} device vs host")


@pytest.mark.parametrize("cid", ("grown-car-L1-D10", "mask-alternating", "rows-round+1-masked", "root-busiest", "parent-int_min"))
def test_two_calls_give_identical_bytes(cid):
    c = xc.case(cid)
    a, b = extract(c), extract(c)
    assert all(a[k].tobytes() == b[k].tobytes() for k in ("state", "ctrl", "parent", "origin", "newRow"))
    assert {k: v for k, v in a["summary"].items() if k != "rootCost"} == {k: v for k, v in b["summary"].items() if k != "rootCost"}
    assert u32(np.float32(a["summary"]["rootCost"])) == u32(np.float32(b["summary"]["rootCost"]))


@pytest.mark.parametrize("cid", ("chain-257", "mask-chain-cut", "mask-null", "d6", "rows-tile+1-masked", "parent-int_max"))
def test_depth_bound_sets_the_passes_not_the_answer(cid):
    """A bound that holds for the input (the rows of its longest usable chain) gives the bytes of
    the default, so do larger ones, and it holds for the output: the extraction extracts to itself
    under it."""
    c = xc.case(cid)
    bound = int(depths(c.parent).max()) + 1
    for b in (bound, bound + 1, 2 * bound + 3, 1 << 20):
        assert_same_extract(extract(c, depthBound=b), c.model, label=f"{c.name} depthBound {b}")
    a = extract(c, depthBound=bound)
    k = a["summary"]["kept"]
    if k:
        assert int(depths(a["parent"]).max()) + 1 <= bound
        again = extract(xc.ExtractCase("again", a["state"], a["ctrl"], a["parent"]), depthBound=bound)
        want = dict(a, origin=np.arange(k, dtype=np.int32), newRow=np.arange(k, dtype=np.int32),
                    summary=dict(rows=k, kept=k, below=0, masked=0, detached=0, root=0, rootCost=a["ctrl"][0, 3]))
        assert_same_extract(again, want, label=f"{c.name} twice")


LAW_CASES = ("mask-null", "mask-alternating", "mask-bytes-2-0x80", "mask-no-busiest", "root-busiest",
             "grown-point-L1-D10", "grown-car-L1.3-D13", "parent-minus1", "star", "chain-257")


def _tree_of(cid):
    if cid.startswith("grown-"):
        return tc.grown(*tc.GROWN[tc.GROWN_IDS.index(cid[len("grown-"):])])
    if cid.startswith("parent-"):
        return tc.parent_case(cid[len("parent-"):])
    if cid == "star":
        return tc.star_case(257)
    if cid.startswith("chain-"):
        return tc.chain_case(int(cid[len("chain-"):]) - 1, "first")
    return tc.grown(*tc.MAIN)


def _some_members(c, n=64):
    m = c.model["origin"]
    return m[np.unique(np.linspace(0, len(m) - 1, n).astype(int))]


@pytest.mark.parametrize("cid", LAW_CASES)
def test_the_device_entries_commute_with_the_extraction(cid):
    c, tree = xc.case(cid), _tree_of(cid)
    assert np.array_equal(tree.parent, c.parent)
    ext = extract(c)
    want = laws.query_law(tree, ext, c.root, c.keep, device=True)
    assert (want["count"] > 0).any()
    nodes = _some_members(c)
    laws.paths_law(tree, ext, c.root, nodes, device=True)
    laws.trace_law(tree, ext, device=True)
    if c.root == 0:
        laws.resample_law(tree, ext, nodes, 0.05, device=True)


def test_an_extraction_by_the_alive_mask_is_alive_against_the_same_list():
    tree = tc.blocked(*tc.MAIN)
    ext, summary = laws.recheck_law(tree, device=True)
    assert 0 < summary["alive"] < summary["rows"] and summary["cut"] > 0
    assert_same_extract(ext, extract_model(tree.state, tree.ctrl, tree.parent, 0, tree.model[2]), label="alive mask")


def test_device_outputs_may_each_be_null_and_capacity_is_checked():
    """sbmp_tree_extract_batch with device pointers: the sizing call, one output at a time, and a
    capacity one short with out->kept still set."""
    from cudasbmp_amd import _native as nat
    from cudasbmp_amd.batch import _Dev
    c = xc.case("mask-chain-cut")
    kept = c.model["summary"]["kept"]
    devs = {k: _Dev(v) for k, v in (("state", c.state), ("ctrl", c.ctrl), ("parent", c.parent), ("keep", c.keep))}
    outs = {"state": _Dev(np.zeros((kept, 4), np.float32)), "ctrl": _Dev(np.zeros((kept, 4), np.float32)),
            "parent": _Dev(np.zeros(kept, np.int32)), "origin": _Dev(np.zeros(kept, np.int32)),
            "newRow": _Dev(np.full(c.rows, -7, np.int32))}
    try:
        a = nat.TreeExtractArgs()
        a.state, a.ctrl, a.parent, a.rows, a.depthBound = devs["state"].ptr, devs["ctrl"].ptr, devs["parent"].ptr, c.rows, 0
        L = nat.lib()
        s = nat.TreeExtract()

        def call(given, capacity, root=0):
            ptrs = [ctypes.c_void_p(outs[k].ptr) if k in given else None for k in ("state", "ctrl", "parent", "origin", "newRow")]
            return L.sbmp_tree_extract_batch(ctypes.byref(a), root, ctypes.c_void_p(devs["keep"].ptr), *ptrs, capacity,
                                             ctypes.byref(s), None)

        assert call((), 0) == 0 and (s.rows, s.kept, s.masked, s.detached) == (257, kept, 1, 128)
        for k in ("state", "ctrl", "parent", "origin"):
            s.kept = -1
            assert call((k,), kept - 1) == SBMP_ERR_INVALID_ARGUMENT and s.kept == kept
            assert call((k,), kept) == 0
            got = outs[k].get()
            want = c.model[k]
            assert got.tobytes() == np.ascontiguousarray(want).tobytes(), k
        assert call(("newRow",), 0) == 0 and np.array_equal(outs["newRow"].get(), c.model["newRow"])
        for root in (-1, 257):
            assert call((), 0, root=root) == SBMP_ERR_INVALID_ARGUMENT
    finally:
        for d in list(devs.values()) + list(outs.values()):
            d.close()


# ---------------------------------------------------------------- planner level
def _tree_of_plan(g):
    s, p, c = g.tree()
    return tree_arrays(s, p, c, g.result().treeSize)


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_extract_of_the_demo_plan(seed, obstacles):
    from cudasbmp_amd import tree_paths_batch, tree_query_batch
    g = _mk()
    r = g.plan(DEMO_INITIAL, DEMO_GOAL, _dev(obstacles), len(obstacles), seed=seed)
    assert r.goalIndex > 0
    state, ctrl, parent = _tree_of_plan(g)
    # the whole tree
    whole = g.extract()
    assert_same_extract(whole, extract_model(state, ctrl, parent), label=f"seed {seed} whole")
    # a box on the solution path's middle row, a re-check, and the alive part as a tree
    rows, ps, _ = g.solution_path()
    x, y = ps[len(rows) // 2, :2]
    boxes = demo_plus((x - 0.05, y - 0.05, x + 0.05, y + 0.05))
    status, summary = g.recheck(boxes)
    alive = (status == 0).astype(np.uint8)
    ext = g.extract(alive=True)
    assert_same_extract(ext, extract_model(state, ctrl, parent, 0, alive), label=f"seed {seed} alive")
    assert ext["summary"]["kept"] == summary["alive"] < summary["rows"]
    goals = np.array([[DEMO_GOAL[0], DEMO_GOAL[1], 0.5], [5.0, 5.0, 0.5], [x, y, 1.0], [12.0, 3.0, 2.0], [9.0, 7.0, 0.5]],
                     np.float32)
    a = tree_query_batch(ext["state"], ext["ctrl"], goals)
    b = g.query_goals(goals, alive=True)
    assert np.array_equal(a["count"], b["count"]) and (b["count"] > 0).sum() >= 2
    for k in ("bestCost", "nearestDistance"):
        assert np.array_equal(bits(a[k]), bits(b[k])), k
    for k in ("firstRow", "bestRow", "nearestRow"):
        assert np.array_equal(np.where(a[k] >= 0, ext["origin"][np.maximum(a[k], 0)], -1), b[k]), k
    # re-rooted on the solution path: the mapped goal row's path is the tail of solution_path
    for at in (1, len(rows) // 2, len(rows) - 1):
        root = int(rows[at])
        sub = g.extract(root=root)
        assert_same_extract(sub, extract_model(state, ctrl, parent, root), label=f"seed {seed} root {root}")
        node = sub["newRow"][r.goalIndex]
        assert node >= 0 and sub["summary"]["below"] == root
        p = tree_paths_batch(sub["state"], sub["ctrl"], sub["parent"], [node])
        assert p["status"].tolist() == [0] and np.array_equal(sub["origin"][p["rows"]], rows[at:])
        assert np.array_equal(bits(p["samples"]), bits(ps[at:]))


def test_extract_between_steps_changes_nothing(obstacles):
    kw = dict(BASE)

    def run(ask):
        g = _mk(**kw)
        g.begin(DEMO_INITIAL, DEMO_GOAL, _dev(obstacles), len(obstacles), BASE_SEED)
        seen = []
        for _ in range(2):
            g.step(3)
            if ask:
                state, ctrl, parent = _tree_of_plan(g)
                root = len(parent) // 7
                for rt in (0, root):
                    got = g.extract(root=rt)
                    assert_same_extract(got, extract_model(state, ctrl, parent, rt), label=f"between steps root {rt}")
                seen.append(len(parent))
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
    box = []                                   # one box on a row of the single planner's tree, set below

    def answers(g):
        other = demo_plus(tuple(box))
        R = min(g.result().treeSize, g.M)
        g.recheck(other)
        return [g.extract(), g.extract(root=R // 5), g.extract(alive=True)]

    def same(a, b):
        return all(x[k].tobytes() == y[k].tobytes() for x, y in zip(a, b) for k in ("state", "ctrl", "parent", "origin", "newRow")) \
            and all({k: v for k, v in x["summary"].items() if k != "rootCost"} == {k: v for k, v in y["summary"].items() if k != "rootCost"}
                    for x, y in zip(a, b))

    single = _mk(**kw)
    single.plan(DEMO_INITIAL, DEMO_GOAL, d, len(obstacles), seed=BASE_SEED)
    state, ctrl, parent = _tree_of_plan(single)
    busiest = int(np.argmax(np.where(depths(parent) >= 2, descendants(parent), -1)))
    x, y = state[busiest, :2]
    box += [x - 0.05, y - 0.05, x + 0.05, y + 0.05]
    want = answers(single)
    assert_same_extract(want[1], extract_model(state, ctrl, parent, len(parent) // 5), label="single")
    assert 0 < want[2]["summary"]["kept"] < want[0]["summary"]["kept"] == len(parent)
    group = _mk(_local_group=2, **kw)
    group.plan(DEMO_INITIAL, DEMO_GOAL, d, len(obstacles), seed=BASE_SEED)
    assert same(answers(group), want), "local group of 2"
    cfg, extra = _split(kw)
    b = KGMTBatch(2, **cfg, **extra)
    b.plan([DEMO_INITIAL] * 2, [DEMO_GOAL] * 2, d, len(obstacles), [BASE_SEED + 1, BASE_SEED])
    assert same(answers(b[1]), want), "batch member 1"


def test_state_and_argument_errors(obstacles):
    from cudasbmp_amd import SbmpError
    from cudasbmp_amd import _native as nat
    g = _mk(**BASE)
    d = _dev(obstacles)

    def status_of(f):
        with pytest.raises(SbmpError) as e:
            f()
        return e.value.status

    assert status_of(lambda: g.extract()) == SBMP_ERR_STATE                      # before the first begin()
    assert status_of(lambda: g.extract(alive=True)) == SBMP_ERR_STATE
    g.begin(DEMO_INITIAL, DEMO_GOAL, d, len(obstacles), BASE_SEED)
    g.step(3)
    R = min(g.result().treeSize, g.M)
    assert R > 1
    assert status_of(lambda: g.extract(alive=True)) == SBMP_ERR_STATE            # no re-check yet
    assert g.extract()["summary"]["kept"] == R
    assert status_of(lambda: g.extract(root=-1)) == SBMP_ERR_INVALID_ARGUMENT
    assert status_of(lambda: g.extract(root=R)) == SBMP_ERR_INVALID_ARGUMENT
    g.recheck(obstacles)
    assert g.extract(alive=True)["summary"]["kept"] == R
    g.step(3)
    assert min(g.result().treeSize, g.M) > R
    assert status_of(lambda: g.extract(alive=True)) == SBMP_ERR_STATE            # the tree grew
    assert g.extract()["summary"]["kept"] > R                                    # the unmasked form goes on
    K = g.recheck(obstacles)[1]["alive"]
    R = min(g.result().treeSize, g.M)
    L = nat.lib()
    s = nat.TreeExtract()
    small = np.zeros(K - 1, np.int32)
    assert L.sbmp_kgmt_extract_tree(g._h, 0, 1, None, None, None, None, None, 0, ctypes.byref(s)) == 0 and s.kept == K > 1
    s.kept = -1
    assert L.sbmp_kgmt_extract_tree(g._h, 0, 1, None, None, None, small.ctypes.data_as(ctypes.c_void_p), None, K - 1,
                                    ctypes.byref(s)) == SBMP_ERR_INVALID_ARGUMENT
    assert s.kept == K and s.rows == R                                           # set in every case
    assert L.sbmp_kgmt_extract_tree(g._h, 0, 0, None, None, None, None, None, 0, None) == SBMP_ERR_INVALID_ARGUMENT
    g.begin(DEMO_INITIAL, DEMO_GOAL, d, len(obstacles), BASE_SEED)
    assert status_of(lambda: g.extract(alive=True)) == SBMP_ERR_STATE            # a new plan
