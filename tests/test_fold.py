"""The R2 key-log fold, the parts that need no GPU (include/sbmp/r2_fold.h):

  sbmp_fold_r2_batch_host   the host twin (the header's loop) against the model of
                            tests/fold_model.py on every case of tests/fold_cases.py, count for count
  the ranks                 P folds into one table pair equal the single-rank fold of the global log
  power                     every alteration of fold_model.ALTERATIONS differs from the twin on
                            each case named beside it
  sbmp_fold_r2_info         against the ceil / round-to-8 arithmetic written out here
  the ABI                   the new symbols, the refused arguments
  tests/fold_host_main.cpp  the header's loop over exact-size heap arrays, built stand-alone with
                            -fsanitize=address,undefined and run once
"""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import fold_cases as fc
from conftest import ROOT
from fold_cases import model, same, twin
from fold_model import ALTERATIONS, fold_model

INVALID = 1   # SBMP_ERR_INVALID_ARGUMENT


# ---------------------------------------------------------------- twin == model
@pytest.mark.parametrize("name", [c.name for c in fc.CASES])
def test_twin_equals_model(name):
    got, want = twin(name), model(name)
    for g, w, table in zip(got, want, ("R2Valid", "R2Invalid")):
        bad = np.flatnonzero(g.astype(np.int64) != w)
        assert bad.size == 0, f"{name}: {table} differs at cells {bad[:8]}: twin {g[bad[:8]]}, model {w[bad[:8]]}"


def test_twin_adds_again_on_a_second_call():
    for name in ("window-40-64", "ranks-P3-r1"):
        c = fc.BY_NAME[name]
        prior = [t.astype(np.int64) for t in c.tables()]
        once, twice = twin(name), twin(name, 2)
        for p, a, b in zip(prior, once, twice):
            assert np.array_equal(b.astype(np.int64) - a, a.astype(np.int64) - p) and np.any(a != p)


def test_counter_cases_reach_the_largest_packed_count():
    for kind, want in (("valid", (fc.KEYS, 0)), ("invalid", (0, fc.KEYS)), ("half", (fc.KEYS // 2, fc.KEYS // 2))):
        for cn, cell in (("cell0", 0), ("cellmax", 1023)):
            v, i = model(f"counter-{kind}-{cn}")
            assert (v[cell], i[cell]) == want and v.sum() + i.sum() == fc.KEYS
            v, i = model(f"counter-{kind}-{cn}-priorbig")
            assert max(v[cell], i[cell]) == fc.INT_MAX - fc.KEYS + max(want)
    assert fc.split(fc.KEYS) == (1, fc.KEYS)   # one workgroup takes all of them
    assert model("counter-two-iterations")[0][1023] == 2 * fc.KEYS > 0xffff


def test_dropped_keys_count_nowhere():
    c = fc.BY_NAME["dropped-keys"]
    row = c.ring()[0].astype(np.int64)
    for cell in fc.DROPPED_CELLS:
        for kind in (0, 0x8000):
            assert np.any(row == (cell | kind))
    v, i = model("dropped-keys")
    kept = (row & 0x7fff) < c.nR2
    assert 0 < kept.sum() < c.logSlots and v.sum() + i.sum() - 2 * c.nR2 == kept.sum()


def test_window_cases_hold_stale_keys_past_every_S():
    for name in ("window-0-64", "window-40-64", "window-31-64-holes"):
        c = fc.BY_NAME[name]
        ring = c.ring().astype(np.int64)
        assert {s % 8 for s in c.S} == set(range(8))
        stale = 0
        for (t, row), s, ex in zip(c.rows(), c.S, c.executed):
            past = ring[row, s:]
            assert np.all((past & 0x7fff) < c.nR2)   # the fill policy: whatever lies past S would count
            stale += past.size
        assert stale > 0 and min(c.S) == 0 and max(c.S) == c.logSlots
    c = fc.BY_NAME["window-40-64"]
    assert [r for _, r in c.rows()] == list(range(40, fc.WINDOW)) + list(range(40))
    c = fc.BY_NAME["window-none-executed"]
    assert not any(c.executed) and same(twin(c.name), c.tables())


# ---------------------------------------------------------------- ranks
@pytest.mark.parametrize("P", sorted(fc.RANK_GROUPS))
def test_rank_folds_add_up_to_the_global_fold(P):
    from cudasbmp_amd import fold_r2_batch
    g, ranks = fc.RANK_GROUPS[P]
    v, i = g.tables()
    for c in ranks:   # every rank into one table pair
        assert c.S == g.S and c.logSlots * P == g.logSlots
        v, i = fold_r2_batch(c.ring(), c.S, c.executed, c.tFirst, c.nR2, rank=c.rank, nranks=P, R2Valid=v,
                             R2Invalid=i, device=False)
    assert same((v, i), model(g.name))
    # S sits on a block of every rank at every offset
    for c in ranks:
        offs = {s % fc.BLOCK for s in g.S if (s // fc.BLOCK) % P == c.rank}
        assert offs == set(fc.RANK_OFFSETS)


# ---------------------------------------------------------------- power
@pytest.mark.parametrize("alter", sorted(ALTERATIONS))
def test_every_alteration_is_caught_by_its_named_cases(alter):
    for name in ALTERATIONS[alter]:
        c = fc.BY_NAME[name]
        v, i = c.tables()
        wrong = fold_model(c.ring(), c.S, c.executed, c.tFirst, c.nR2, rank=c.rank, nranks=c.nranks, R2Valid=v,
                           R2Invalid=i, alter=alter)
        assert not same(wrong, twin(name)), f"{alter} passes {name}"
        assert same(model(name), twin(name))


# ---------------------------------------------------------------- the info call
def test_info_is_the_arithmetic_written_out():
    from cudasbmp_amd import fold_r2_info
    for logSlots in sorted({c.logSlots for c in fc.CASES} | {fc.KEYS - fc.BLOCK, fc.KEYS + fc.BLOCK, 3 * fc.KEYS,
                                                            3 * fc.KEYS + fc.BLOCK, 262144}):
        i = fold_r2_info(logSlots)
        groups = -(-logSlots // i["keysPerGroup"])
        per = -(-(-(-logSlots // groups)) // 8) * 8
        assert (i["groups"], i["per"]) == (groups, per)
        assert per <= i["keysPerGroup"] < 1 << 16 and per * (groups - 1) < logSlots <= per * groups
        assert (i["window"], i["maxR2"], i["maxRanks"]) == (fc.WINDOW, fc.MAX_R2, fc.MAX_RANKS)
    assert fc.MAX_R2 == 0x7fff and fc.KEYS % 8 == 0
    # the three-group shape: a group border inside a 256-slot block, on an 8-key piece
    assert fc.BIG_GROUPS == 3 and fc.BIG_PER % fc.BLOCK != 0 and fc.BIG_PER % 8 == 0
    assert [fc.split(s)[0] for s in fc.GROUP_SHAPES] == [1, 1, 2, 2, 3, 3]
    assert fc.split(65536) == (2, 32768)


# ---------------------------------------------------------------- the stand-alone program
def test_rule_standalone_under_sanitizers(tmp_path):
    cxx = next((c for c in (shutil.which("c++"), shutil.which("g++"), shutil.which("clang++"),
                            "/opt/rocm/llvm/bin/clang++") if c and os.path.exists(c)), None)
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "fold_host_main")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "fold_host_main.cpp"),
                    "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ok" in r.stdout


# ---------------------------------------------------------------- the ABI
def test_library_exports_the_fold_symbols():
    from cudasbmp_amd import _native as nat
    L = nat.lib()
    for f in ("sbmp_fold_r2_info", "sbmp_fold_r2_batch", "sbmp_fold_r2_batch_host"):
        assert hasattr(L, f) and f in nat.EXPORTED_SYMBOLS
    assert L.sbmp_abi_version() == 1


def _call(L, fn, **kw):
    """One call of a fold entry on small valid arrays, with the named arguments replaced."""
    a = dict(ring=np.zeros((fc.WINDOW, 256), dtype=np.uint16), S=np.zeros(fc.WINDOW, dtype=np.int32),
             executed=np.zeros(fc.WINDOW, dtype=np.int32), tFirst=0, tLast=0, logSlots=256, nR2=16, rank=0, nranks=1,
             valid=np.zeros(16, dtype=np.int32), invalid=np.zeros(16, dtype=np.int32))
    a.update(kw)
    p = lambda x: None if x is None else x.ctypes.data_as(ctypes.c_void_p)
    args = [p(a["ring"]), p(a["S"]), p(a["executed"]), a["tFirst"], a["tLast"], a["logSlots"], a["nR2"], a["rank"],
            a["nranks"], p(a["valid"]), p(a["invalid"])]
    return getattr(L, fn)(*args, None) if fn == "sbmp_fold_r2_batch" else getattr(L, fn)(*args)


REFUSED = [dict(logSlots=0), dict(logSlots=-256), dict(logSlots=255), dict(logSlots=257), dict(logSlots=264),
           dict(nR2=0), dict(nR2=-1), dict(nR2=fc.MAX_R2 + 1), dict(tFirst=0, tLast=-1), dict(tFirst=3, tLast=1),
           dict(tFirst=0, tLast=fc.WINDOW), dict(tFirst=7, tLast=7 + fc.WINDOW), dict(tFirst=-1, tLast=0),
           dict(tFirst=-1, tLast=-1), dict(tFirst=-2**31, tLast=2**31 - 1), dict(rank=-1), dict(rank=1),
           dict(rank=2, nranks=2), dict(nranks=0), dict(nranks=-1), dict(nranks=fc.MAX_RANKS + 1), dict(ring=None),
           dict(S=None), dict(executed=None), dict(valid=None), dict(invalid=None)]


@pytest.mark.parametrize("entry", ["sbmp_fold_r2_batch_host", "sbmp_fold_r2_batch"])
def test_bad_arguments_are_refused(entry):
    """Both entries refuse before they touch a buffer or the device (the device entry is given
    host arrays here: a call that got past the checks would fail differently)."""
    from cudasbmp_amd import _native as nat
    L = nat.lib()
    for kw in REFUSED:
        assert _call(L, entry, **kw) == INVALID, kw
    assert _call(L, "sbmp_fold_r2_batch_host") == 0
    assert _call(L, "sbmp_fold_r2_batch_host", tFirst=7, tLast=6 + fc.WINDOW, nR2=fc.MAX_R2,
                 valid=np.zeros(fc.MAX_R2, dtype=np.int32), invalid=np.zeros(fc.MAX_R2, dtype=np.int32),
                 rank=fc.MAX_RANKS - 1, nranks=fc.MAX_RANKS) == 0


def test_info_refuses_what_it_cannot_split():
    from cudasbmp_amd import _native as nat
    L = nat.lib()
    info = nat.FoldInfo()
    for logSlots in (0, -256, 255, 257):
        assert L.sbmp_fold_r2_info(logSlots, ctypes.byref(info)) == INVALID
    assert L.sbmp_fold_r2_info(256, None) == INVALID
    assert L.sbmp_fold_r2_info(256, ctypes.byref(info)) == 0


def test_wrapper_checks_shapes():
    from cudasbmp_amd import fold_r2_batch
    ring = np.zeros((fc.WINDOW, 256), dtype=np.uint16)
    with pytest.raises(ValueError):
        fold_r2_batch(ring[:-1], [1], [1], 0, 16, device=False)
    with pytest.raises(ValueError):
        fold_r2_batch(ring, [1, 2], [1], 0, 16, device=False)
    with pytest.raises(ValueError):
        fold_r2_batch(ring, [1], [1], 0, 16, R2Valid=np.zeros(15), device=False)
    v, i = fold_r2_batch(ring, [3], [1], 0, 16, device=False)
    assert v.tolist() == [0] * 16 and i.tolist() == [3] + [0] * 15
