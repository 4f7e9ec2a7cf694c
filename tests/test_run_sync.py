"""Which waits the host half of a run asks for (batch.h: the named waits; run.h: the stages of a run;
pool.h: Pending).  The emulator is synchronous — its tests cannot see ORDER on the device — but
with IRS_SIM_SYNC_LOG it writes down every event_record, stream_wait and event_sync the host code
calls: `<op> e<event> s<stream>`, events numbered by first appearance.  The facts below are read
from that log.  The segment is test_join_score_lean's (2 x 16320 + 7000 docs, pairing forced): the
smallest at which a run takes the tail stream.

The caller's streams are integers the emulator never dereferences; the library's own (upload,
download, tail) are the small tokens its stream_create hands out.  Tail::done and the stream
cache's slabs belong to the device, not to a batch: what earlier tests of the session left there
shows up as waits for events this log has no record of, which no assertion here counts."""
from __future__ import annotations

import os
import subprocess
from pathlib import Path

import numpy as np
import pytest

from iresearch_amd import _lib
from test_join_slab_images import _Env
from test_tail_stream import _Lean

ROOT = Path(__file__).resolve().parents[1]
S, P, M, D = 0x5001, 0x5002, 0x5003, 0x5004   # caller streams: run, plan, match sets, copies out
K = 3


class _Log:
    """The sync log, read call by call: take() = the (op, event, stream) lines since the last one."""

    def __init__(self, path):
        self.path, self.at = str(path), 0

    def take(self):
        if not os.path.exists(self.path):
            return []
        with open(self.path) as f:
            f.seek(self.at)
            text = f.read()
            self.at = f.tell()
        out = []
        for line in text.splitlines():
            op, e, s = line.split()
            out.append((op, int(e[1:]), None if s == "s-" else int(s[1:])))
        return out


@pytest.fixture(scope="module")
def lean(simlib):
    w = _Lean(simlib)
    yield w
    w.close()


@pytest.fixture
def log(tmp_path, monkeypatch):
    path = tmp_path / "sync.log"
    monkeypatch.setenv("IRS_SIM_SYNC_LOG", str(path))
    return _Log(path)


def _batch(lean, i=0):
    # (the host half of run() on this thread: the log's lines in the order of the calls)
    return lean.batch(i, K).set_async(False)


def _recorded(lines):
    return {e for op, e, _ in lines if op == "record"}


def _tail_run(lines, st):
    """Of a tail run queued on `st`: (scored, tail stream, done, Tail::done)."""
    scored = [(i, e) for i, (op, e, s) in enumerate(lines[:-1])
              if op == "record" and s == st and lines[i + 1][:2] == ("wait", e) and lines[i + 1][2] != st]
    assert len(scored) == 1, lines
    i, ev = scored[0]
    ts = lines[i + 1][2]
    assert ts not in (None, 0, S, P, M, D)
    (op1, done, s1), (op2, dev_done, s2) = lines[-2:]
    assert (op1, s1, op2, s2) == ("record", ts, "record", ts) and len({ev, done, dev_done}) == 3, lines
    return ev, ts, done, dev_done


def test_tail_run_replay_and_first_run(lean, log):
    b = _batch(lean)
    b.configure(0, 0, 0)   # (a setter: quiesce)
    assert log.take() == []   # a batch that never ran: nothing to get behind
    b.run(S)
    first = log.take()
    assert b.tail_stream_used()
    # `scored` on the caller's stream, waited for on the tail stream; `done` (and the device's
    # Tail::done) recorded on the tail stream
    scored, ts, done, dev_done = _tail_run(first, S)
    b.run(S)
    replay = log.take()
    # the replay: S behind `done` before anything is recorded
    first_record = min(i for i, l in enumerate(replay) if l[0] == "record")
    assert ("wait", done, S) in replay[:first_record]
    assert _tail_run(replay, S) == (scored, ts, done, dev_done)   # (the same events again)
    # the first run waited for nothing of the batch's own from before: every event of the batch it
    # waited for was recorded earlier in that very run (the uploads, `scored`), and the host
    # waited for nothing
    own = _recorded(first + replay) - {dev_done}
    seen = set()
    for op, e, s in first:
        assert op != "sync"
        if op == "wait" and e in own:
            assert e in seen, (op, e, s)
        if op == "record":
            seen.add(e)
    lean.check(0, K, b.results())
    assert ("sync", done, None) in log.take()
    b.close()
    assert log.take() == [("sync", done, None)]   # destroy: `done`, nothing else was pending


def test_plan_ahead_then_run(lean, log):
    b = _batch(lean, 1)
    b.plan(P)
    planned = log.take()
    assert planned and planned[-1][0] == "record" and planned[-1][2] == P   # (behind the slabs' fills)
    plan = planned[-1][1]
    assert all(op != "sync" and s == P for op, _, s in planned)
    b.run(S)
    run = log.take()
    first_record = min(i for i, l in enumerate(run) if l[0] == "record")
    assert ("wait", plan, S) in run[:first_record]
    # the plan stage has sent every table staged since create, on P: this first run has nothing
    # left for the upload stream (so no stream but S waits for `plan`)
    assert all(s == S for op, e, s in run if e == plan)
    done = _tail_run(run, S)[2]
    b.run(S)
    assert all(e != plan for _, e, _ in log.take())   # the next run does not wait for it again
    # a plan queued and never used, then destroy: `done` and `plan`, each once
    b.plan(P)
    log.take()
    b.close()
    assert log.take() == [("sync", done, None), ("sync", plan, None)]


def test_match_sets_then_run_and_setter(lean, log):
    b = _batch(lean, 2)
    n_words = b.match_words()
    sets = np.zeros((len(lean.filters[2]), n_words), np.uint64)
    counts = np.zeros(len(lean.filters[2]), np.uint64)
    b.match_sets_to_device(sets.ctypes.data, n_words, counts.ctypes.data, M)
    queued = log.take()
    assert [l[0] for l in queued] == ["record"] and queued[0][2] == M
    matched = queued[0][1]
    b.run(S)
    run = log.take()
    first_record = min(i for i, l in enumerate(run) if l[0] == "record")
    assert ("wait", matched, S) in run[:first_record]
    done = run[-2][1]
    b.close()
    assert log.take() == [("sync", done, None)]   # destroy does not sync `matched`: the run settled it
    # ... followed by a setter instead: the host gets behind `matched`
    b = _batch(lean, 2)
    b.match_sets_to_device(sets.ctypes.data, n_words, counts.ctypes.data, M)
    matched = log.take()[0][1]
    b.set_path(_lib.PATH_JOINED)
    assert log.take() == [("sync", matched, None)]
    b.close()
    assert log.take() == []


def test_results_to_host_then_run(lean, log):
    b = _batch(lean)
    b.run(S)
    done = log.take()[-2][1]
    b.results_to_host(D)
    copy = log.take()
    assert copy[-2:] == [("wait", done, D), ("record", copy[-1][1], D)]
    host = copy[-1][1]
    b.host_results()
    b.host_results()   # (handed out again: the copy is through, the results stay)
    assert log.take() == [("sync", host, None)] * 2
    b.run(S)
    run = log.take()
    first_record = min(i for i, l in enumerate(run) if l[0] == "record")
    assert ("wait", host, S) in run[:first_record]
    with pytest.raises(_lib.IrsHipError) as e:   # stale from the run on, until the next copy
        b.host_results()
    assert e.value.status == _lib.EINVAL
    b.results_to_host(D)
    b.host_results()
    b.close()


def test_destroy_syncs_each_pending_once(lean, log):
    b = _batch(lean)
    b.run(S)
    done = log.take()[-2][1]
    hits = np.zeros((len(lean.filters[0]), K, 2), np.uint32)
    counts = np.zeros(len(lean.filters[0]), np.uint32)
    b.results_to_device(hits.ctypes.data, counts.ctypes.data, D)
    used = log.take()[-1]
    assert used[0] == "record" and used[2] == D
    b.results_to_host(D)
    host = log.take()[-1][1]
    n_words = b.match_words()
    sets = np.zeros((len(lean.filters[0]), n_words), np.uint64)
    b.match_sets_to_device(sets.ctypes.data, n_words, None, M)
    matched = log.take()[-1][1]
    b.plan(P)
    plan = log.take()[-1][1]
    assert len({done, used[1], host, matched, plan}) == 5
    b.close()
    assert log.take() == [("sync", e, None) for e in (done, plan, used[1], host, matched)]


def test_knob_off_names_no_tail_stream(lean, log):
    b = _batch(lean)
    b.run(S)
    _, ts, _, _ = _tail_run(log.take(), S)
    b.close()
    log.take()
    with _Env(IRS_HIP_TAIL_STREAM=0):
        b = _batch(lean)
        b.run(S).run(S)
        assert not b.tail_stream_used()
        b.results()
        b.close()
    lines = log.take()
    assert lines and all(s != ts for _, _, s in lines)
    assert [l for l in lines if l[0] == "record"][-1][2] == S   # `done` on the caller's stream


def test_pending_standalone(tmp_path):
    """tests/cpp/test_pending.cpp: Pending by itself against the emulator's rt::."""
    exe = tmp_path / "test_pending"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-I", str(ROOT / "tests" / "sim"),
           "-I", str(ROOT / "iresearch_amd" / "csrc"), str(ROOT / "tests" / "cpp" / "test_pending.cpp"),
           "-o", str(exe), "-pthread"]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    run = subprocess.run([str(exe), str(tmp_path / "pending.log")], capture_output=True, text=True,
                         timeout=120)
    assert run.returncode == 0, (run.stdout + run.stderr)[-3000:]
    assert "test_pending OK" in run.stdout
