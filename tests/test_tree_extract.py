"""The tree extraction (prune and re-root), the parts that need no GPU
(include/sbmp/tree_extract.h):

  sbmp_tree_extract_batch_host   the host twin (extract_rows_host) against the model of
                                 tests/tree_extract_model.py, bit for bit, on the whole table of
                                 tests/tree_extract_cases.py
  the laws                       an extraction extracts to itself; a depthBound that held for the
                                 input holds for the output; the query, paths, trace, resample and
                                 re-check host twins commute with it (tests/tree_extract_laws.py)
  tests/tree_extract_host_main.cpp   the twin over exact-size heap arrays, built stand-alone with
                                 -fsanitize=address,undefined and run once
  the ABI                        the new symbols, the refused arguments, the capacity protocol
"""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import tree_extract_cases as xc
import tree_extract_laws as laws
import tree_recheck_cases as tc
from conftest import ROOT
from tree_extract_model import assert_same_extract, extract_model
from tree_recheck_model import depths

INVALID = 1   # SBMP_ERR_INVALID_ARGUMENT


@pytest.fixture(scope="module", autouse=True)
def _oracle(oracle_lib):
    return oracle_lib


def host(c, **kw):
    from cudasbmp_amd import tree_extract_batch
    return tree_extract_batch(c.state, c.ctrl, c.parent, root=c.root, keep=c.keep, device=False, **kw)


# ---------------------------------------------------------------- the table
@pytest.mark.parametrize("cid", xc.IDS)
def test_host_twin_is_the_model(cid):
    c = xc.case(cid)
    got = host(c)
    assert_same_extract(got, c.model, label=f"{c.name} host vs model")
    s = got["summary"]
    assert s["rows"] == c.rows == s["kept"] + s["below"] + s["masked"] + s["detached"] and s["below"] == c.root
    # every new parent is a lower new row, and the old order is kept
    k = s["kept"]
    if k:
        assert got["parent"][0] == -1 and np.all(got["parent"][1:] >= 0) and np.all(got["parent"][1:] < np.arange(1, k))
        assert got["origin"][0] == c.root and np.all(np.diff(got["origin"]) > 0)


def test_the_table_reaches_every_class_and_seam():
    tile, rnd = xc.layout()
    assert (tile, rnd) == (1024, 1024 * 256)
    seen = {k: 0 for k in ("kept", "below", "masked", "detached")}
    for cid in ("mask-chain-cut", "root-busiest", "mask-alternating", "root-masked", "mask-zero", "rows-round+1-masked"):
        for k in seen:
            seen[k] += xc.case(cid).model["summary"][k]
    assert all(v > 0 for v in seen.values()), seen
    cut = xc.case("mask-chain-cut").model["summary"]
    assert (cut["kept"], cut["masked"], cut["detached"]) == (128, 1, 128)
    assert xc.case("root-masked").model["summary"]["kept"] == 0 and xc.case("mask-zero").model["summary"]["kept"] == 0
    assert xc.case("mask-root-only").model["summary"]["kept"] == 1
    packed = xc.case("mask-packed-last-tile")
    assert packed.root == 3 * tile and packed.model["summary"]["kept"] == 17
    for which, hub in (("first", 0), ("last", 63)):
        c = xc.case(f"mask-{which}-lanes")
        assert np.array_equal(c.model["origin"] % 64, np.full(c.model["summary"]["kept"], hub)) and c.model["summary"]["kept"] > 30
    for r in xc.D6_ROWS:                      # counted, never written: nobody's parent, its own parent word is -1
        c = xc.case(f"root-d6-{r}")
        assert c.parent[r] == -1 and c.model["summary"]["kept"] == 1
    assert xc.case("rows-round+1").rows == rnd + 1 and xc.case("rows-round+1").model["summary"]["kept"] == rnd + 1


def test_the_table_passes_one_sweep_of_rows_and_of_tiles():
    """The cases past a sweep are what they are named for: members on both sides of row SWEEP, three,
    five and nine rounds of the offsets workgroup, one row in tile SWEEP_TILES, a packed case whose
    first tile round counts 1 per tile at most outside its last tile, a root past the sweep."""
    from cudasbmp_amd import tree_extract_info
    tile, rnd = xc.layout()
    assert xc.SWEEP == 256 * 8 * 256 and xc.SWEEP_TILES == 2048
    for what, tiles, rounds in (("sweep+77", 513, 3), ("2sweep+1", 1025, 5), ("tiles+1", 2049, 9)):
        rows = xc.past_sweep_rows(what)
        i = tree_extract_info(rows)
        assert (i["tiles"], i["rounds"]) == (tiles, rounds) and rows > xc.SWEEP
        for suffix in ("", "-masked"):
            c = xc.case(f"rows-{what}{suffix}")
            m, s = c.model["member"], c.model["summary"]
            assert c.rows == rows and m[:xc.SWEEP].sum() > 1000 and m[xc.SWEEP:].sum() >= 10
            assert (s["kept"] == rows) == (suffix == "") and (suffix == "" or (s["masked"] > 1000 and s["detached"] > 1000))
    assert xc.past_sweep_rows("tiles+1") == xc.SWEEP_TILES * tile + 1
    assert xc.case("rows-tiles+1").model["member"][-1]         # the one row of tile SWEEP_TILES (under the mask: counted, no member)
    p = xc.case("rows-tiles+1-packed-by-mask")
    first = xc.SWEEP_TILES * tile - 300
    per_tile = np.add.reduceat(p.model["member"].astype(np.int64), np.arange(0, p.rows, tile))
    assert per_tile[0] == 1 and not per_tile[1:-2].any() and per_tile[-2] == 300 and per_tile[-1] == 1
    assert p.model["summary"]["kept"] == 302 and p.parent[first] == 0 and p.model["origin"][1] == first
    for suffix in ("", "-masked"):
        r = xc.case(f"root-past-sweep{suffix}")
        s = r.model["summary"]
        assert r.root == xc.SWEEP + 5 == s["below"] and r.rows == 2 * xc.SWEEP + 1 and s["kept"] >= 1


# ---------------------------------------------------------------- laws
LAW_CASES = ("mask-null", "mask-alternating", "mask-bytes-2-0x80", "mask-no-busiest", "root-busiest",
             "root-busiest-alternating", "grown-point-L1-D10", "grown-car-L1.3-D13", "parent-minus1", "star", "chain-257")


@pytest.mark.parametrize("cid", LAW_CASES + ("rows-tile+1-masked", "d6", "mask-chain-cut"))
def test_extracting_an_extraction_returns_itself(cid):
    c = xc.case(cid)
    a = host(c)
    assert a["summary"]["kept"] > 0
    b = host(xc.ExtractCase("again", a["state"], a["ctrl"], a["parent"]))
    k = a["summary"]["kept"]
    want = dict(a, origin=np.arange(k, dtype=np.int32), newRow=np.arange(k, dtype=np.int32),
                summary=dict(rows=k, kept=k, below=0, masked=0, detached=0, root=0, rootCost=a["ctrl"][0, 3]))
    assert_same_extract(b, want, label=f"{c.name} twice")


@pytest.mark.parametrize("cid", LAW_CASES + ("d6", "parent-int_max", "rows-tile+1-masked"))
def test_a_depth_bound_of_the_input_holds_for_the_output(cid):
    c = xc.case(cid)
    bound = int(depths(c.parent).max()) + 1            # rows of the longest usable chain
    a = host(c, depthBound=bound)
    assert_same_extract(a, c.model, label=f"{c.name} depthBound {bound}")
    if a["summary"]["kept"]:
        assert int(depths(a["parent"]).max()) + 1 <= bound


def _tree_of(cid):
    """The tests/tree_recheck_cases.py Case (with params and boxes) a law case was taken from."""
    if cid.startswith("grown-"):
        g = tc.GROWN[tc.GROWN_IDS.index(cid[len("grown-"):])]
        return tc.grown(*g)
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
def test_the_host_twins_commute_with_the_extraction(cid):
    c, tree = xc.case(cid), _tree_of(cid)
    assert tree.parent is c.parent or np.array_equal(tree.parent, c.parent)
    ext = host(c)
    want = laws.query_law(tree, ext, c.root, c.keep, device=False)
    assert (want["count"] > 0).any()
    nodes = _some_members(c)
    if cid != "parent-minus1":
        laws.paths_law(tree, ext, c.root, nodes, device=False)
    laws.trace_law(tree, ext, device=False)
    if c.root == 0 and cid != "parent-minus1":
        laws.resample_law(tree, ext, nodes, 0.05, device=False)


def test_paths_law_on_a_tree_with_broken_chains():
    """parent-minus1 cuts rows off: the members' own paths are whole, and the law holds for them."""
    c, tree = xc.case("parent-minus1"), tc.parent_case("minus1")
    ext = host(c)
    assert ext["summary"]["detached"] > 0
    laws.paths_law(tree, ext, 0, _some_members(c), device=False)
    laws.resample_law(tree, ext, _some_members(c), 0.05, device=False)


@pytest.mark.parametrize("g", [tc.MAIN, ("point", 1.0, 10)], ids=["car-L1-D10", "point-L1-D10"])
def test_an_extraction_by_the_alive_mask_is_alive_against_the_same_list(g):
    tree = tc.blocked(*g)
    ext, summary = laws.recheck_law(tree, device=False)
    assert 0 < summary["alive"] < summary["rows"] and summary["cut"] > 0
    assert_same_extract(ext, extract_model(tree.state, tree.ctrl, tree.parent, 0, tree.model[2]), label="alive mask")


# ---------------------------------------------------------------- the stand-alone program
def test_twin_standalone_under_sanitizers(tmp_path):
    """The twin over exact-size heap arrays, every crafted parent and every row as the root, as its
    own program under AddressSanitizer and UBSan."""
    cxx = next((c for c in (shutil.which("c++"), shutil.which("g++"), shutil.which("clang++"),
                            "/opt/rocm/llvm/bin/clang++") if c and os.path.exists(c)), None)
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "tree_extract_host_main")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "tree_extract_host_main.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ok" in r.stdout


# ---------------------------------------------------------------- the ABI
def test_library_exports_the_extract_symbols():
    from cudasbmp_amd import _native as nat
    L = nat.lib()
    for f in ("sbmp_kgmt_extract_tree", "sbmp_tree_extract_batch", "sbmp_tree_extract_batch_host", "sbmp_tree_extract_info"):
        assert hasattr(L, f) and f in nat.EXPORTED_SYMBOLS
    assert L.sbmp_abi_version() == 1


def test_extract_info_is_the_ceil_arithmetic():
    from cudasbmp_amd import _native as nat, tree_extract_info
    base = tree_extract_info(0)
    T, P = base["tileRows"], base["roundTiles"]
    assert T % 256 == 0 and P >= 64 and base["tiles"] == 0 and base["rounds"] == 0
    for rows in (1, T - 1, T, T + 1, T * P, T * P + 1, 2 ** 24, 2 ** 31 - 1):
        i = tree_extract_info(rows)
        assert i["tiles"] == -(-rows // T) and i["rounds"] == -(-i["tiles"] // P), rows
    info = nat.TreeExtractLayout()
    L = nat.lib()
    assert L.sbmp_tree_extract_info(-1, ctypes.byref(info)) == INVALID
    assert L.sbmp_tree_extract_info(2 ** 31, ctypes.byref(info)) == INVALID
    assert L.sbmp_tree_extract_info(5, None) == INVALID


def test_refused_arguments_and_the_capacity_protocol():
    from cudasbmp_amd import _native as nat
    c = xc.case("mask-chain-cut")
    L = nat.lib()
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    out = nat.TreeExtract()

    def args(**changes):
        a = nat.TreeExtractArgs()
        a.state, a.ctrl, a.parent = c.state.ctypes.data, c.ctrl.ctypes.data, c.parent.ctypes.data
        a.rows, a.depthBound = c.rows, 0
        for k, v in changes.items():
            setattr(a, k, v)
        return a

    def call(root=0, keep=c.keep, outs=(None,) * 5, capacity=0, a=None, o=out):
        return L.sbmp_tree_extract_batch_host(ctypes.byref(a or args()), root, vp(keep) if keep is not None else None,
                                              *(vp(x) if x is not None else None for x in outs), capacity,
                                              ctypes.byref(o) if o is not None else None)

    # the sizing call: nothing given, everything counted
    assert call() == 0 and (out.rows, out.kept, out.masked, out.detached, out.below) == (257, 128, 1, 128, 0)
    kept = out.kept
    for root in (-1, 257, 2 ** 31 - 1, -(2 ** 31)):
        assert call(root=root) == INVALID
    assert call(a=args(rows=0)) == INVALID and call(a=args(rows=-3)) == INVALID
    for name in ("state", "ctrl", "parent"):
        assert call(a=args(**{name: None})) == INVALID
    assert call(o=None) == INVALID
    assert L.sbmp_tree_extract_batch_host(None, 0, None, None, None, None, None, None, 0, ctypes.byref(out)) == INVALID
    # capacity one short with each member-sized output alone: refused, and out->kept is set all the same
    bufs = [np.zeros((kept, 4), np.float32), np.zeros((kept, 4), np.float32), np.zeros(kept, np.int32), np.zeros(kept, np.int32)]
    newRow = np.full(257, -7, np.int32)
    for i in range(4):
        out.kept = -1
        outs = [None] * 5
        outs[i] = bufs[i]
        assert call(outs=outs, capacity=kept - 1) == INVALID and out.kept == kept
        assert call(outs=outs, capacity=kept) == 0
    # newRow alone needs no capacity
    assert call(outs=(None, None, None, None, newRow), capacity=0) == 0
    assert np.array_equal(newRow, c.model["newRow"])
    # a root that is not kept: an answer, not an error, even into arrays of no rows
    keep = c.keep.copy()
    keep[0] = 0
    newRow[:] = 5
    assert call(keep=keep, outs=(bufs[0], bufs[1], bufs[2], bufs[3], newRow), capacity=0) == 0
    assert (out.kept, out.masked, out.detached) == (0, 2, 255) and np.all(newRow == -1)
