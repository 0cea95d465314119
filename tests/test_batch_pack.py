"""sbmp_batch_pack: which batch members share a k_step_batch launch (host-only, no GPU).

A k_step workgroup waits in-kernel for its member's planner workgroup, so a launch may
hold members only while the sum of their workgroups (1 + blocks each) stays within what
the device holds at once.  The rule: members in index order into the
fewest launches that obey this; a member larger than the figure is not batchable.
"""
import ctypes

import numpy as np
import pytest


@pytest.fixture(scope="module")
def nat():
    from cudasbmp_amd import _native
    _native.lib()
    return _native


def _check(groups, resident):
    from cudasbmp_amd import batch_pack
    launch, n = batch_pack(groups, resident)
    assert len(launch) == len(groups)
    fit = [i for i, g in enumerate(groups) if g <= resident]
    # every member in exactly one launch (or reported as not batchable), in index order
    assert [i for i, l in enumerate(launch) if l >= 0] == fit
    ls = [launch[i] for i in fit]
    assert ls == sorted(ls) and (not ls or (ls[0] == 0 and ls[-1] == n - 1))
    assert set(ls) == set(range(n))
    for l in range(n):   # no launch exceeds the figure
        assert sum(g for g, x in zip(groups, launch) if x == l) <= resident
    return launch, n


def test_demo_members_share_launches():
    # the demo: 119 workgroups per member, 1,280 resident
    launch, n = _check([119] * 10, 1280)
    assert n == 1 and launch == [0] * 10
    launch, n = _check([119] * 11, 1280)
    assert n == 2 and launch == [0] * 10 + [1]


@pytest.mark.parametrize("B", [1, 2, 5, 10, 11, 23, 64])
@pytest.mark.parametrize("groups,resident", [(119, 1280), (119, 238), (119, 119), (2, 5), (1025, 1280), (1, 1)])
def test_equal_members_launch_count(B, groups, resident):
    _, n = _check([groups] * B, resident)
    per = resident // groups
    assert n == -(-B // per)   # ceil(B / floor(resident / groups))


def test_fewest_launches_for_mixed_members():
    rng = np.random.default_rng(11)
    for _ in range(200):
        B = int(rng.integers(1, 12))
        groups = [int(x) for x in rng.integers(1, 40, size=B)]
        resident = int(rng.integers(max(groups), 120))
        _, n = _check(groups, resident)
        # the fewest contiguous groups within the figure, by dynamic programming
        best = [0] + [10 ** 9] * B
        for j in range(1, B + 1):
            s = 0
            for i in range(j, 0, -1):
                s += groups[i - 1]
                if s > resident:
                    break
                best[j] = min(best[j], best[i - 1] + 1)
        assert n == best[B], (groups, resident)


def test_member_larger_than_the_device_is_not_batchable():
    launch, n = _check([119, 2000, 119, 119], 1280)
    assert launch[1] == -1 and n == 2 and launch == [0, -1, 1, 1]
    launch, n = _check([1281], 1280)
    assert launch == [-1] and n == 0
    launch, n = _check([5, 5], 0)
    assert launch == [-1, -1] and n == 0


def test_single_member():
    launch, n = _check([119], 1280)
    assert launch == [0] and n == 1
    launch, n = _check([1280], 1280)
    assert launch == [0] and n == 1


def test_pack_rejects_bad_arguments(nat):
    g = (ctypes.c_int * 2)(3, 3)
    out = (ctypes.c_int * 2)()
    n = ctypes.c_int()
    L = nat.lib()
    vp = ctypes.c_void_p
    ok = L.sbmp_batch_pack(ctypes.cast(g, vp), 2, 8, ctypes.cast(out, vp), ctypes.byref(n))
    assert ok == 0 and n.value == 1
    assert L.sbmp_batch_pack(None, 2, 8, ctypes.cast(out, vp), ctypes.byref(n)) == 1      # SBMP_ERR_INVALID_ARGUMENT
    assert L.sbmp_batch_pack(ctypes.cast(g, vp), 2, 8, None, ctypes.byref(n)) == 1
    assert L.sbmp_batch_pack(ctypes.cast(g, vp), 2, 8, ctypes.cast(out, vp), None) == 1
    assert L.sbmp_batch_pack(ctypes.cast(g, vp), 0, 8, ctypes.cast(out, vp), ctypes.byref(n)) == 1
    assert L.sbmp_batch_pack(ctypes.cast(g, vp), 2, -1, ctypes.cast(out, vp), ctypes.byref(n)) == 1
    bad = (ctypes.c_int * 2)(3, 0)
    assert L.sbmp_batch_pack(ctypes.cast(bad, vp), 2, 8, ctypes.cast(out, vp), ctypes.byref(n)) == 1


def test_batch_create_rejects_bad_arguments(nat):
    """The §3 error cases the library can answer without a device."""
    p = nat.KgmtParams()
    nat.call("sbmp_kgmt_default_params", ctypes.byref(p))
    h = ctypes.c_void_p()
    L = nat.lib()
    for count in (0, -3):
        assert L.sbmp_kgmt_batch_create(ctypes.byref(p), count, ctypes.byref(h)) == 1
        assert not h.value
    assert L.sbmp_kgmt_batch_create(None, 2, ctypes.byref(h)) == 1
    assert L.sbmp_kgmt_batch_create(ctypes.byref(p), 2, None) == 1
    # NULL handles
    assert L.sbmp_kgmt_batch_begin(None, None, None, None, 0, None) == 1
    assert L.sbmp_kgmt_batch_plan(None, None, None, None, 0, None, None) == 1
    assert L.sbmp_kgmt_batch_step(None, 1, None) == 1
    assert L.sbmp_kgmt_batch_info(None, None) == 1
    assert L.sbmp_kgmt_batch_member(None, 0, ctypes.byref(h)) == 1
    assert L.sbmp_kgmt_batch_destroy(None) == 0


def test_sharded_parameters_are_unsupported():
    from cudasbmp_amd import KGMTBatch, SbmpError
    from conftest import DEMO
    with pytest.raises(SbmpError) as e:
        KGMTBatch(2, **DEMO, _local_group=2)
    assert e.value.status == 6   # SBMP_ERR_UNSUPPORTED
    with pytest.raises(SbmpError) as e:
        KGMTBatch(2, **DEMO, _sharded=(b"\0" * 128, 2, 0))
    assert e.value.status == 6
