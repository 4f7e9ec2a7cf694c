"""The node-table walk of the tree kernels on the device (tree.h tree_table + tree_scoring_mask), held
to one plain statement — apart from whole batches.

tree_scoring_mask is separate text from tree_shape.h's tree_eval (which tests/cpp/tree_shape_check.cpp
holds to a recursive walk on the host): it reads the records as packed words from LDS.
tests/probe/tree_probe.hip (test-only, never part of the library) compiles a query record and its
entries with tree_compile, UNMODIFIED, launches a kernel of kWideThreads threads with TreeOff::end
bytes of dynamic LDS that calls tree_table, a barrier and tree_scoring_mask for EVERY presence mask
p < 2^n_leaves, and returns beside the device's words the host's tree_eval of the same table.  The
probe is built twice by fixtures of this module — the g++ line of tests/sim/build_sim.sh with the
probe in place of the product source (test_*_twin) and hipcc for gfx950 with the library's flags
(test_*_gpu) — and both run the same table of trees.

The statement (statement()), in numpy over all masks at once, recursing over the FILTER OBJECTS, not
the table: a leaf matches iff its bit is set (leaf l = the l-th by_term in prefix order, negated ones
included); an And matches iff all its positive children match and no negated child does; an Or iff at
least max(1, min_match) of its children match; the scoring set of a matching node is the union of its
matching positive children's sets (a matching leaf's set is its bit); the result is 0 where the root
does not match."""
from __future__ import annotations

import ctypes as C
import fcntl
import shlex
import shutil
import subprocess
import tempfile
from pathlib import Path

import numpy as np
import pytest

from iresearch_amd import _lib, search
from iresearch_amd.search import BM25, And, Not, Or, by_term
from test_boolean_trees import T, chain, hand_queries, literal_entries, n_leaves, random_trees, unwrap

ROOT = Path(__file__).resolve().parents[1]
PROBE = ROOT / "tests" / "probe"
SRC = PROBE / "tree_probe.hip"
SIM_SO = PROBE / "libtree_probe_sim.so"
HIP_SO = PROBE / "libtree_probe_hip.so"
CSRC = ROOT / "iresearch_amd" / "csrc"

FILL32 = 0xEEEEEEEE
MAX_LEAVES = MAX_NODES = 16
N_RANDOM, RANDOM_SEED = 200, 77
TABLE = np.dtype([("node", [("pos_leaves", "<u2"), ("neg_leaves", "<u2"), ("pos_nodes", "<u2"), ("neg_nodes", "<u2"),
                            ("type", "u1"), ("min_match", "u1"), ("pad0", "<u2"), ("pad1", "<u4")], (MAX_NODES,)),
                  ("n_nodes", "<u4"), ("n_leaves", "<u4"), ("n_entries", "<u4"), ("leaf_at", "<u4", (MAX_LEAVES,)),
                  ("negated", "<u2"), ("unsupported", "u1"), ("pad", "u1")])
STATS = [search.SegmentStats(1000, 100_000, np.full(64, 10, np.int64))]


# ---- the two builds ------------------------------------------------------------------------------

def _stale(target: Path, deps) -> bool:
    return not target.exists() or any(d.stat().st_mtime > target.stat().st_mtime for d in deps)


def _locked():
    lock = open(PROBE / ".build.lock", "w")
    fcntl.flock(lock, fcntl.LOCK_EX)   # (pytest-xdist workers: one builds, the others wait)
    return lock


def _deps(hip_dir: Path):
    return [SRC, ROOT / "include" / "irs_hip.h"] + list(CSRC.glob("*.h")) + list(hip_dir.glob("*.h"))


def build_sim() -> Path:
    """The g++ line of tests/sim/build_sim.sh with the probe in place of the product source."""
    with _locked():
        sim = ROOT / "tests" / "sim"
        if _stale(SIM_SO, _deps(CSRC / "hip") + [sim / "sim_switch.S"] + list(sim.glob("*.h"))):
            text = (sim / "build_sim.sh").read_text().replace("\\\n", " ")
            line = [l for l in text.splitlines() if l.startswith("exec g++")]
            assert len(line) == 1, "build_sim.sh: one g++ line expected"
            cmd = shlex.split(line[0])[1:]
            assert "tests/sim/libirs_hip_sim.so" in cmd and "iresearch_amd/csrc/irs_hip.hip" in cmd
            cmd = [{"tests/sim/libirs_hip_sim.so": str(SIM_SO),
                    "iresearch_amd/csrc/irs_hip.hip": str(SRC)}.get(a, a) for a in cmd]
            subprocess.run(cmd, check=True, cwd=ROOT)
    return SIM_SO


def build_hip() -> Path:
    """hipcc for gfx950 with the flags of iresearch_amd/_build.py (cross-compiles without a GPU)."""
    from iresearch_amd import _build
    with _locked():
        if _stale(HIP_SO, _deps(CSRC / "hip")):
            hipcc = _build.hipcc_path()
            assert hipcc, "hipcc not found"
            with tempfile.TemporaryDirectory() as tmp:
                out = Path(tmp) / HIP_SO.name
                subprocess.run(
                    [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared", "-pthread",
                     "-ffp-contract=off", "-fno-gpu-rdc", "-Wall", "-Wno-unused-function",
                     "-I", str(ROOT / "include"), "-I", str(CSRC), "-I", str(CSRC / "hip"),
                     "-o", str(out), str(SRC)], check=True, cwd=tmp)
                shutil.copyfile(out, HIP_SO)
    return HIP_SO


def _bind(path: Path):
    P = C.CDLL(str(path))
    i, vp = C.c_uint32, C.c_void_p
    P.tp_arch.argtypes, P.tp_arch.restype = [C.c_char_p, C.c_size_t], C.c_int
    P.tp_layout.argtypes, P.tp_layout.restype = [vp], None
    P.tp_tree.argtypes, P.tp_tree.restype = [vp, vp, i, vp, vp, i, vp, vp, i], C.c_int
    lay = np.zeros(4, np.uint32)
    P.tp_layout(lay.ctypes.data)
    assert int(lay[0]) == TABLE.itemsize, ("TreeTable", lay, TABLE.itemsize)
    assert int(lay[2]) == int(lay[1]) + 16 * MAX_NODES and int(lay[3]) == 1024, lay
    return P


@pytest.fixture(scope="module")
def probe_sim():
    P = _bind(build_sim())
    buf = C.create_string_buffer(64)
    assert P.tp_arch(buf, 64) == 0 and buf.value == b"gfx950-sim"
    return P


@pytest.fixture(scope="module")
def probe_gpu():
    """The probe against the product headers on a real GPU; fails (does not skip) without one."""
    import torch  # noqa: F401  (one HIP runtime per process: iresearch_amd/_lib.py)
    P = _bind(build_hip())
    buf = C.create_string_buffer(64)
    assert P.tp_arch(buf, 64) == 0, "no usable HIP device"
    assert buf.value.decode().startswith("gfx950"), buf.value
    return P


def test_tree_probe_cross_compiles():
    """Compile only (no GPU): the gfx950 build of the probe, so that the GPU tier finds it built."""
    assert build_hip().exists()


# ---- the statement -------------------------------------------------------------------------------

def statement(flt, n):
    """uint32[2^n]: the scoring mask of every presence mask, by the module's docstring."""
    P = np.arange(1 << n, dtype=np.uint32)
    at = [0]

    def walk(f):
        """(matches bool[], scoring set uint32[] — 0 where the node does not match)"""
        if type(f) is by_term:
            l = at[0]
            at[0] += 1
            m = (P >> np.uint32(l)) & np.uint32(1) != 0
            return m, np.where(m, np.uint32(1 << l), np.uint32(0))
        assert type(f) in (And, Or), f
        pos, neg = [], []
        for s in f.subs:
            g, negated = unwrap(s)
            (neg if negated else pos).append(walk(g))      # (prefix order: the leaves number themselves)
        if type(f) is And:
            m = np.ones(P.size, bool)
            for cm, _ in pos:
                m &= cm
            for cm, _ in neg:
                m &= ~cm
        else:
            assert not neg
            m = sum(cm.astype(np.int64) for cm, _ in pos) >= max(1, int(f.min_match))
        sets = np.zeros(P.size, np.uint32)
        for cm, cs in pos:
            sets |= np.where(cm, cs, np.uint32(0))
        return m, np.where(m, sets, np.uint32(0))

    m, sets = walk(flt)
    assert at[0] == n
    assert ((sets != 0) == m).all(), "a matching node has a matching positive child"
    return sets


# ---- the table of trees --------------------------------------------------------------------------

def _nested(levels, top=And):
    """`levels` node entries inside one another under the root, 16 leaves: the root and every entry but
    the innermost hold one leaf beside their child, alternating And / Or; the innermost is an Or of one
    leaf."""
    node = Or([T(levels)])
    for i in range(levels - 1, -1, -1):
        node = (top if i % 2 == 0 else Or if top is And else And)([T(i), node])
    return node


def limit_trees():
    out = {}
    out["16 leaves"] = chain(list(range(16)))
    out["15 nested entries"] = _nested(15)
    out["15 nested entries, Or root"] = _nested(15, Or)
    for mm in (1, 2, 13, 14, 15):       # (15: more than it has — the And branch alone matches)
        out["min-match %d of 14" % mm] = Or([Or([T(t) for t in range(14)], min_match=mm), And([T(14), T(15)])])
    out["root min-match 13 of 14"] = Or([T(t) for t in range(13)] + [And([T(13), T(14)])], min_match=13)
    out["Not three levels down"] = And([T(0), Or([T(1), And([T(2), Or([T(3), And([T(4), Not(Or([T(5), And([T(6), T(7)])]))])])])])])
    out["one term twice"] = Or([And([T(0), T(2)]), And([T(0), Or([T(4), T(6)])])])
    out["Not leaf under the root"] = And([Not(T(0)), T(1), Or([T(2), And([T(3), T(4)])])])
    out["Not leaves and Not subtree under the root"] = And([T(0), Not(T(1)), Not(And([T(2), T(3)])), Not(T(4)),
                                                             Or([T(5), T(6)], min_match=2)])
    return out


def tree_table():
    trees = [("hand: " + n, f) for n, f in hand_queries().items()]
    trees += [("limit: " + n, f) for n, f in limit_trees().items()]
    trees += [("random %d" % i, f) for i, f in enumerate(random_trees(N_RANDOM, RANDOM_SEED))]
    return trees


def encode(flt):
    """(query record, entries) as test_boolean_trees.literal_arrays writes them, for one filter."""
    es = literal_entries(flt, BM25(), STATS)
    q = np.zeros(1, _lib.QUERY)
    mm = int(flt.min_match) if flt.op == _lib.OP_MINMATCH else 0
    q[0] = (flt.op, len(es), 0, 10, mm, search.MERGE_SUM)
    ents = np.zeros(len(es), _lib.TERM_SCORER)
    for j, (t, kind, c0, nc, nl, off) in enumerate(es):
        ents[j] = (_lib.NO_TERM if t is None else t, kind, c0, nc, nl, off)
    return q, ents


def probe_tree(P, flt, n_masks=None):
    """(status, TreeTable, device words, host words) of one filter."""
    q, ents = encode(flt)
    n = n_leaves(flt)
    n_masks = (1 << min(n, MAX_LEAVES)) if n_masks is None else n_masks
    status = C.c_int(-99)
    table = np.zeros(1, TABLE)
    dev = np.full(n_masks, 0x55555555, np.uint32)
    host = np.full(n_masks, 0x55555555, np.uint32)
    rc = P.tp_tree(q.ctypes.data, ents.ctypes.data, len(ents), C.addressof(status), table.ctypes.data,
                   TABLE.itemsize, dev.ctypes.data, host.ctypes.data, n_masks)
    return rc, status.value, table[0], dev, host


def case_walk(P):
    trees = tree_table()
    assert len(hand_queries()) >= 17 and len(trees) >= 17 + 13 + N_RANDOM
    seen_leaves, seen_nodes = set(), set()
    for name, flt in trees:
        n = n_leaves(flt)
        rc, status, tab, dev, host = probe_tree(P, flt)
        assert rc == 0 and status == _lib.OK, (name, rc, status)
        assert int(tab["n_leaves"]) == n and 1 <= int(tab["n_nodes"]) <= MAX_NODES, (name, tab)
        want = statement(flt, n)
        assert (want != 0).any() and (want == 0).any(), ("a tree needs a matching and a non-matching mask", name)
        assert want[0] == 0, name
        assert not (dev == FILL32).any(), ("a word the kernel did not write", name)
        bad = np.nonzero(host != want)[0]
        assert bad.size == 0, ("tree_eval", name, flt, hex(int(bad[0])), hex(int(host[bad[0]])), hex(int(want[bad[0]])))
        bad = np.nonzero(dev != want)[0]
        assert bad.size == 0, ("tree_scoring_mask", name, flt, hex(int(bad[0])), hex(int(dev[bad[0]])), hex(int(want[bad[0]])))
        assert not (want & np.uint32(int(tab["negated"]))).any(), ("a negated leaf scores", name)
        seen_leaves.add(n)
        seen_nodes.add(int(tab["n_nodes"]))
    assert MAX_LEAVES in seen_leaves and MAX_NODES in seen_nodes and min(seen_leaves) <= 4, (seen_leaves, seen_nodes)
    lim = limit_trees()
    # what the limits are: the tables the walk ran on
    tab = probe_tree(P, lim["15 nested entries"])[2]
    assert int(tab["n_entries"]) == 15 and int(tab["n_nodes"]) == 16 and int(tab["n_leaves"]) == 16
    assert [int(x) for x in tab["node"]["pos_nodes"]] == [0] + [1 << i for i in range(15)], "nested one inside the other"
    tab = probe_tree(P, lim["min-match 15 of 14"])[2]
    assert int(tab["node"][0]["min_match"]) == 15 and bin(int(tab["node"][0]["pos_leaves"])).count("1") == 14
    tab = probe_tree(P, lim["one term twice"])[2]
    assert int(tab["n_leaves"]) == 5      # the term's two entries are two leaves
    tab = probe_tree(P, lim["Not leaf under the root"])[2]
    assert int(tab["negated"]) == 1 and int(tab["node"][int(tab["n_nodes"]) - 1]["neg_leaves"]) == 1
    tab = probe_tree(P, lim["Not three levels down"])[2]
    assert sum(1 for x in tab["node"]["neg_nodes"] if x) == 1 and int(tab["negated"]) == 0
    # ... and just beyond them nothing is launched: the words stay the caller's
    for flt, n_masks in ((_nested(16), 1 << 16), (chain(list(range(17))), 1 << 16)):
        rc, status, tab, dev, host = probe_tree(P, flt, n_masks)
        assert rc == 0 and status == _lib.EUNSUPPORTED, (flt, rc, status)
        assert (dev == 0x55555555).all() and (host == 0x55555555).all()
    # the probe's own size check
    assert probe_tree(P, lim["one term twice"], 16)[0] == -1


def test_statement_by_hand():
    """The statement on masks worked out by hand: a AND (b OR (c AND d)); (a AND NOT b) OR c."""
    nest = statement(And([T(0), Or([T(1), And([T(2), T(3)])])]), 4)
    assert nest[0b0011] == 0b0011 and nest[0b1101] == 0b1101 and nest[0b1111] == 0b1111
    assert nest[0b0101] == 0 and nest[0b1110] == 0 and nest[0b0001] == 0
    assert nest[0b0111] == 0b0011, "c without d: its And is not active, c does not score"
    andnot = statement(Or([And([T(0), Not(T(1))]), T(2)]), 3)
    assert andnot[0b001] == 0b001 and andnot[0b011] == 0 and andnot[0b111] == 0b100 and andnot[0b101] == 0b101
    mm = statement(Or([T(0), T(1), T(2)], min_match=2), 3)
    assert [int(x) for x in mm] == [0, 0, 0, 3, 0, 5, 6, 7]


def test_tree_walk_twin(probe_sim):
    case_walk(probe_sim)


@pytest.mark.gpu
def test_tree_walk_gpu(probe_gpu):
    case_walk(probe_gpu)
