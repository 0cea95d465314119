"""Goal queries against tree rows, the parts that need no GPU (include/sbmp/tree_query.h):

  sbmp_goal_radius_threshold   t(r), the value k_tree_query compares d2 with, against the
                               literal rule sqrtf(d2) < r at t and one float above it
  sbmp_tree_query_batch_host   the host loop over rows, against the numpy model
                               (tests/tree_query_model.py): random rows, the crafted cases the
                               GPU tests run (tests/tree_query_cases.py), the CPU oracle's demo tree
  sbmp_tree_query_alive_batch_host   the same loop with a mask, against the model over the alive
                               rows on every masked case; a null mask equals a mask of ones; any
                               non-zero byte is alive
  tests/tree_query_host_main.cpp   the loop over exact-size heap arrays, built stand-alone with
                               -fsanitize=address,undefined and run once
  the model's nearestRow       the keyed minimum equals np.argmin wherever no d2 is NaN
  the ABI                      the new symbols, the refused arguments

Every comparison is bit-exact.
"""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import DEMO, DEMO_GOAL, DEMO_INITIAL, ROOT
from tree_query_cases import MASKED_GOAL_COUNTS, MASKED_NAMES, NAMES, case, check_expect, masked_case
from tree_query_model import assert_same_answers, d2_of, model_of_rows, nearest_of, tree_rows

F32_MAX = np.finfo(np.float32).max
INF = np.float32(np.inf)


def _threshold(r):
    from cudasbmp_amd import goal_radius_threshold
    return goal_radius_threshold(float(r))


def _fixed_radii():
    tiny = np.float32(1e-45)
    r = [0.5, 1.0, 2.0, 0.25, 3.0, 10.0, 0.1, 0.3, 1.5, 1e-3, 1e-10, 1e-19, 1e-20, 1e-22, 1e-23, 1e-30, 1e-37, 1e10,
         1e18, 1e19, 1.8446743e19, 1.8446744e19, 1.8446746e19, 1e20, 1e30, 1e38, F32_MAX, np.inf,
         tiny, 2 * tiny, 3 * tiny, 1e-44, 1e-42, 1e-40, 5.8774704e-39, 1.1754942e-38, 1.17549435e-38,   # subnormals, FLT_MIN
         3.7433924e-23, 3.7433928e-23, 2.6469780e-23,   # around sqrt of the smallest subnormals
         1.0842022e-19, 1.0842021e-19]                  # around sqrt(FLT_MIN)
    one = np.float32(1.0)
    r += [np.nextafter(one, INF), np.nextafter(one, np.float32(0)), np.nextafter(np.float32(0.5), INF),
          np.nextafter(np.float32(0.5), np.float32(0)), np.nextafter(np.float32(F32_MAX), np.float32(0))]
    r += [np.float32(2.0) ** e for e in (-149, -126, -75, -74, -64, -63, -1, 1, 63, 64, 127)]
    r += [np.sqrt(np.float32(2.0)), np.sqrt(np.float32(3.0)), np.float32(np.pi), np.float32(7.0), np.float32(0.7),
          np.float32(123.456)]
    r = [np.float32(v) for v in r]
    assert len(r) == 64 and all(v > 0 for v in r)
    return r


def test_threshold_is_the_last_d2_inside():
    rng = np.random.default_rng(2024)
    random_r = rng.integers(1, 0x7f800000, size=10000, dtype=np.uint32).view(np.float32)   # every exponent
    assert random_r.min() < 1e-30 and random_r.max() > 1e30
    radii = np.concatenate([np.array(_fixed_radii(), np.float32), random_r])
    t = np.array([_threshold(r) for r in radii], np.float32)
    with np.errstate(all="ignore"):
        assert np.all(np.sqrt(t) < radii)
        above = np.nextafter(t, INF)
        outside = ~(np.sqrt(above) < radii)
    is_inf = np.isinf(radii)
    assert np.all(outside[~is_inf])
    assert is_inf.sum() == 1 and np.all(t[is_inf] == F32_MAX)   # sqrtf(inf) < inf is false: every finite d2 is inside
    for r, want in ((0.5, np.nextafter(np.float32(0.25), np.float32(0))), (1.0, np.nextafter(np.float32(1), np.float32(0))),
                    (1e-30, np.float32(0.0))):
        assert _threshold(r).view(np.uint32) == want.view(np.uint32)


@pytest.mark.parametrize("r", [0.0, -0.0, -1.0, -np.inf, np.nan])
def test_threshold_of_a_degenerate_radius_admits_nothing(r):
    t = _threshold(r)
    d2 = np.array([0.0, 1e-45, 1.0, F32_MAX, np.inf, np.nan], np.float32)
    with np.errstate(all="ignore"):
        assert not np.any(d2 <= t)
        assert not np.any(np.sqrt(d2) < np.float32(r))


@pytest.mark.parametrize("name", NAMES)
def test_host_twin_matches_model(name):
    from cudasbmp_amd import tree_query_batch
    state, ctrl, goals, expect, model = case(name)
    check_expect(model, expect, label=f"{name} (model)")
    host = tree_query_batch(state, ctrl, goals, device=False)
    assert_same_answers(host, model, label=name)
    check_expect(host, expect, label=name)


def _distinct_answers(model, Q):
    keys = {tuple(int(np.float32(model[k][q]).view(np.uint32)) if model[k].dtype == np.float32 else int(model[k][q])
                  for k in model) for q in range(Q)}
    return len(keys)


@pytest.mark.parametrize("Q", [1, 7, 8, 9, 63, 64, 65, 257])
def test_goal_count_cases_have_distinct_answers(Q):
    assert _distinct_answers(case(f"goals-{Q}")[4], Q) == Q


@pytest.mark.parametrize("name", MASKED_NAMES)
def test_masked_host_twin_matches_model(name):
    from cudasbmp_amd import tree_query_batch
    c = masked_case(name)   # its preconditions (where the mask must matter) are asserted as it is built
    check_expect(c.model, c.expect, label=f"{name} (model)")
    host = tree_query_batch(c.state, c.ctrl, c.goals, alive=c.mask, device=False)
    assert_same_answers(host, c.model, label=name)
    check_expect(host, c.expect, label=name)


@pytest.mark.parametrize("Q", MASKED_GOAL_COUNTS)
def test_masked_goal_count_cases_have_distinct_answers(Q):
    """A tile that wrote its answers at another goal's place could not pass."""
    c = masked_case(f"masked-goals-{Q}")
    assert _distinct_answers(c.model, Q) == Q
    assert 0.4 < c.mask.mean() < 0.6 and set(np.unique(c.mask).tolist()) == {0, 1}


def test_any_nonzero_byte_is_alive():
    from cudasbmp_amd import tree_query_batch
    b, z = masked_case("masked-bytes"), masked_case("masked-bytes-01")
    assert np.array_equal(b.mask != 0, z.mask == 1) and (b.mask > 1).sum() > 1000 and ((b.mask & 1) == 0).sum() > 1000
    assert_same_answers(b.model, z.model, label="the models")
    host = tree_query_batch(b.state, b.ctrl, b.goals, alive=b.mask, device=False)
    assert_same_answers(host, tree_query_batch(z.state, z.ctrl, z.goals, alive=z.mask, device=False), label="host twin")
    assert_same_answers(host, z.model, label="host twin vs the 0 / 1 model")


@pytest.mark.parametrize("name", NAMES)
def test_no_mask_is_a_mask_of_ones(name):
    from cudasbmp_amd import tree_query_batch
    state, ctrl, goals, _, model = case(name)
    for ones in (np.ones(len(state), np.uint8), np.full(len(state), 0xff, np.uint8)):
        assert_same_answers(tree_query_batch(state, ctrl, goals, alive=ones, device=False), model, label=name)
    assert_same_answers(model_of_rows(state, ctrl, goals, np.ones(len(state), np.uint8)), model, label=f"{name} (model)")


def test_the_empty_set_answer():
    from cudasbmp_amd import tree_query_batch
    c = masked_case("masked-none")
    host = tree_query_batch(c.state, c.ctrl, c.goals, alive=c.mask, device=False)
    assert not c.mask.any() and len(c.goals) == 13
    assert np.all(host["count"] == 0) and np.all(host["firstRow"] == -1) and np.all(host["bestRow"] == -1)
    assert np.all(host["bestCost"].view(np.uint32) == 0) and np.all(host["nearestRow"] == -1)
    assert np.all(host["nearestDistance"].view(np.uint32) == 0x7f800000)


@pytest.mark.parametrize("name", NAMES + MASKED_NAMES)
def test_keyed_nearest_equals_argmin_where_no_d2_is_nan(name):
    """nearest_of orders a NaN d2 above +inf, np.argmin below everything: they part only there."""
    if name in MASKED_NAMES:
        c = masked_case(name)
        state, goals = c.state[c.mask != 0], c.goals
    else:
        state, _, goals = case(name)[:3]
    nan_free = 0
    for gx, gy, _ in goals:
        d2 = d2_of(state[:, 0], state[:, 1], gx, gy)
        if len(d2) and not np.isnan(d2).any():
            assert nearest_of(d2) == int(np.argmin(d2))
            nan_free += 1
    assert nan_free == (0 if name in ("nonfinite", "masked-nonfinite", "masked-none") else len(goals))


def test_keyed_nearest_puts_nan_last():
    d2 = np.array([np.nan, np.inf, 3.0, 3.0, -np.nan], np.float32)
    assert nearest_of(d2) == 2 and int(np.argmin(d2)) == 0
    assert nearest_of(d2[:2]) == 1 and nearest_of(d2[:1]) == 0


def test_host_twin_on_the_oracle_demo_tree(oracle_lib, obstacles):
    from cudasbmp_amd import tree_query_batch
    o = oracle_lib.Oracle(oracle_lib.PlannerConfig(**DEMO), threads=4)
    o.plan(DEMO_INITIAL, DEMO_GOAL, obstacles, 1)
    info = o.info()
    s, p, c = o.tree()
    state, ctrl = tree_rows(s, c, info["treeSize"])
    R = len(state)
    assert R == min(info["treeSize"], DEMO["maxTreeSize"]) and info["goalIdx"] > 0
    goals = np.array([[DEMO_GOAL[0], DEMO_GOAL[1], 0.5], [5.0, 5.0, 0.5], [9.0, 7.0, 0.5], [19.5, 0.5, 2.0]], np.float32)
    host = tree_query_batch(state, ctrl, goals, device=False)
    assert_same_answers(host, model_of_rows(state, ctrl, goals), label="demo tree")
    # the planner's own answer (D4): the first inside row among the rows it inserted, 1 .. R - 1
    tail = tree_query_batch(state[1:], ctrl[1:], goals[:1], device=False)
    assert tail["firstRow"][0] + 1 == info["goalIdx"]
    assert host["firstRow"][0] == info["goalIdx"]          # the root (5, 5) is outside the demo's disc
    assert host["count"][0] >= 1
    assert host["bestCost"][0] <= np.float32(info["costToGoal"])
    assert host["firstRow"][1] == 0 and host["bestRow"][1] == 0   # the root is inside a disc round itself


def test_library_exports_the_query_symbols():
    from cudasbmp_amd import _native as nat
    L = nat.lib()
    for f in ("sbmp_kgmt_query_goals", "sbmp_tree_query_batch", "sbmp_tree_query_batch_host",
              "sbmp_tree_query_alive_batch", "sbmp_tree_query_alive_batch_host", "sbmp_goal_radius_threshold"):
        assert hasattr(L, f) and f in nat.EXPORTED_SYMBOLS
    assert ctypes.sizeof(nat.GoalQuery) == 12 and ctypes.sizeof(nat.GoalAnswer) == 24
    assert L.sbmp_abi_version() == 1


def _host_status(state, ctrl, rows, goals, count, out):
    from cudasbmp_amd import _native as nat
    p = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)
    return nat.lib().sbmp_tree_query_batch_host(p(state), p(ctrl), rows, p(goals), count, p(out))


def test_refused_arguments():
    from cudasbmp_amd import _native as nat
    from cudasbmp_amd.tree_query import ANSWER_DTYPE
    state, ctrl = case("ties")[:2]
    out = np.zeros(2, ANSWER_DTYPE)
    INVALID = 1   # SBMP_ERR_INVALID_ARGUMENT
    for bad in (np.nan, np.inf, -np.inf):
        for col in (0, 1):
            goals = np.array([[1.0, 2.0, 0.5], [1.0, 2.0, 0.5]], np.float32)
            goals[1, col] = bad
            assert _host_status(state, ctrl, len(state), goals, 2, out) == INVALID
            assert b"goal 1" in nat.lib().sbmp_last_error()
    goals = np.array([[1.0, 2.0, np.nan], [1.0, 2.0, -3.0]], np.float32)   # any radius is accepted
    assert _host_status(state, ctrl, len(state), goals, 2, out) == 0
    assert _host_status(state, ctrl, len(state), None, 2, out) == INVALID
    assert _host_status(state, ctrl, len(state), goals, 2, None) == INVALID
    assert _host_status(state, ctrl, len(state), goals, -1, out) == INVALID
    assert _host_status(None, ctrl, len(state), goals, 2, out) == INVALID
    assert _host_status(state, ctrl, 0, goals, 2, out) == INVALID
    t = ctypes.c_float()
    assert nat.lib().sbmp_goal_radius_threshold(ctypes.c_float(1.0), None) == INVALID
    assert nat.lib().sbmp_goal_radius_threshold(ctypes.c_float(1.0), ctypes.byref(t)) == 0


def _p(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def test_refused_arguments_of_the_masked_entries():
    """Those of the unmasked entry, plus a NULL mask.  The device entry checks its arguments
    before it touches the device, so its refusals need none."""
    from cudasbmp_amd import _native as nat
    from cudasbmp_amd.tree_query import ANSWER_DTYPE
    c = masked_case("masked-ties")
    state, ctrl, mask, R = c.state, c.ctrl, c.mask, len(c.state)
    out = np.zeros(2, ANSWER_DTYPE)
    L = nat.lib()
    INVALID = 1   # SBMP_ERR_INVALID_ARGUMENT
    host = lambda st, ct, al, rows, g, n, o: L.sbmp_tree_query_alive_batch_host(_p(st), _p(ct), _p(al), rows, _p(g), n, _p(o))
    dev = lambda st, ct, al, rows, g, n, o: L.sbmp_tree_query_alive_batch(_p(st), _p(ct), _p(al), rows, _p(g), n, _p(o), None)
    goals = np.array([[1.0, 2.0, np.nan], [1.0, 2.0, -3.0]], np.float32)   # any radius is accepted
    assert host(state, ctrl, mask, R, goals, 2, out) == 0
    for f in (host, dev):   # the device entry is given host pointers: every call below is refused before they are used
        for bad in (np.nan, np.inf, -np.inf):
            for col in (0, 1):
                g = np.array([[1.0, 2.0, 0.5], [1.0, 2.0, 0.5]], np.float32)
                g[1, col] = bad
                assert f(state, ctrl, mask, R, g, 2, out) == INVALID
                assert b"goal 1" in L.sbmp_last_error()
        assert f(state, ctrl, None, R, goals, 2, out) == INVALID
        assert b"alive" in L.sbmp_last_error()
        assert f(None, ctrl, mask, R, goals, 2, out) == INVALID
        assert f(state, None, mask, R, goals, 2, out) == INVALID
        assert f(state, ctrl, mask, R, None, 2, out) == INVALID
        assert f(state, ctrl, mask, R, goals, 2, None) == INVALID
        assert f(state, ctrl, mask, R, goals, -1, out) == INVALID
        assert f(state, ctrl, mask, 0, goals, 2, out) == INVALID
        assert f(state, ctrl, mask, 1 << 31, goals, 2, out) == INVALID
        assert f(state, ctrl, mask, R, None, 0, None) == 0   # count == 0 is a no-op
        assert f(state, ctrl, None, R, None, 0, None) == INVALID


def test_mask_length_is_checked():
    from cudasbmp_amd import tree_query_batch
    c = masked_case("masked-ties")
    with pytest.raises(ValueError):
        tree_query_batch(c.state, c.ctrl, c.goals, alive=c.mask[:-1], device=False)
    as_bool = tree_query_batch(c.state, c.ctrl, c.goals, alive=c.mask.astype(bool), device=False)
    assert_same_answers(as_bool, c.model, label="a bool mask")


def test_twin_standalone_under_sanitizers(tmp_path):
    """The masked and the unmasked loop over heap arrays sized to the byte (rows, mask, goals,
    answers), the all-dead mask and the one-row tree, as its own program under AddressSanitizer
    and UBSan: built from include/sbmp/tree_query.h alone."""
    cxx = next((c for c in (shutil.which("c++"), shutil.which("g++"), shutil.which("clang++"),
                            "/opt/rocm/llvm/bin/clang++") if c and os.path.exists(c)), None)
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "tree_query_host_main")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "tree_query_host_main.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ok" in r.stdout


def test_count_zero_is_accepted():
    from cudasbmp_amd import tree_query_batch
    state, ctrl = case("ties")[:2]
    assert _host_status(state, ctrl, len(state), None, 0, None) == 0
    out = tree_query_batch(state, ctrl, np.zeros((0, 3), np.float32), device=False)
    assert all(len(v) == 0 for v in out.values())
