"""tests/children.py itself, with sleeping and exiting CPU children only: time limits end a child and fail the test, a child
that aborted, was ended by a signal or ran out of time is recorded and nothing is started after it, a child that merely
fails is not recorded, and the one compile line treats warnings as errors.  No test here opens a GPU."""
import multiprocessing
import os
import signal
import sys
import time

import pytest

from tests import children
from tests.children import build_program, run_program, spawn_ranks

SLEEP = "import os, sys, time; open(sys.argv[1], 'w').write(str(os.getpid())); time.sleep(60)"


@pytest.fixture(autouse=True)
def fresh_record(monkeypatch):
    monkeypatch.setattr(children, "died", [])


def _gone(pid: int) -> bool:
    try:
        os.kill(pid, 0)
    except ProcessLookupError:
        return True
    return False


def _returns(rank, out_dir):
    open(os.path.join(out_dir, f"done{rank}"), "w").write("ok")


def _rank_one_raises(rank, out_dir):
    if rank == 1:
        raise ValueError("rank 1 says no")


def _rank_one_sleeps(rank, out_dir):
    time.sleep(60 if rank == 1 else 0)


def _rank_one_is_killed(rank, out_dir):
    if rank == 1:
        os.kill(os.getpid(), signal.SIGKILL)


def _never_started(rank, out_dir):
    open(os.path.join(out_dir, "started"), "w").write("yes")


def test_a_child_past_its_limit_is_ended_and_nothing_is_started_after_it(tmp_path):
    pid_file = tmp_path / "pid"
    start = time.monotonic()
    with pytest.raises(pytest.fail.Exception, match=r"did not end within 1 s"):
        run_program([sys.executable, "-c", SLEEP, pid_file], limit=1)
    assert time.monotonic() - start < 30
    assert _gone(int(pid_file.read_text()))
    assert len(children.died) == 1 and children.died[0].endswith("(timeout)")
    with pytest.raises(AssertionError, match=r"not started: .* died before"):
        run_program([sys.executable, "-c", f"open({str(tmp_path / 'started')!r}, 'w')"])
    with pytest.raises(AssertionError, match=r"not started: .* died before"):
        spawn_ranks(_never_started, (str(tmp_path),), 2)
    with pytest.raises(AssertionError, match=r"not started: .* died before"):
        build_program("plane_scan", tmp_path, library=False)
    assert not (tmp_path / "started").exists() and not (tmp_path / "plane_scan").exists()
    assert len(children.died) == 1                               # the first death stays the one on record


@pytest.mark.parametrize("code,status", [("import sys; sys.exit(134)", 134), ("import sys; sys.exit(139)", 139),
                                         ("import os, signal; os.kill(os.getpid(), signal.SIGTERM)", -15)])
def test_an_abort_status_or_a_signal_is_recorded(code, status):
    r = run_program([sys.executable, "-c", code])
    assert r.returncode == status
    assert len(children.died) == 1 and f"(exit status {status})" in children.died[0]


def test_a_child_that_merely_fails_is_not_recorded():
    r = run_program([sys.executable, "-c", "import sys; print('out'); print('err', file=sys.stderr); sys.exit(3)"])
    assert r.returncode == 3 and r.stdout == "out\n" and r.stderr == "err\n"
    assert children.died == []
    assert run_program([sys.executable, "-c", "pass"]).returncode == 0


def test_ranks_that_return_pass(tmp_path):
    spawn_ranks(_returns, (str(tmp_path),), 2)
    assert sorted(os.listdir(tmp_path)) == ["done0", "done1"] and children.died == []


def test_a_rank_that_raises_surfaces_as_with_a_plain_join_and_is_not_recorded(tmp_path):
    import torch.multiprocessing as mp

    with pytest.raises(mp.ProcessRaisedException, match="rank 1 says no"):
        spawn_ranks(_rank_one_raises, (str(tmp_path),), 2)
    assert children.died == []


def test_a_rank_ended_by_a_signal_is_recorded(tmp_path):
    import torch.multiprocessing as mp

    with pytest.raises(mp.ProcessExitedException):
        spawn_ranks(_rank_one_is_killed, (str(tmp_path),), 2)
    assert len(children.died) == 1 and "rank 1: exit status -9" in children.died[0]


def test_ranks_past_their_limit_are_all_ended_and_recorded(tmp_path):
    with pytest.raises(pytest.fail.Exception, match=r"the ranks did not end within 2 s"):
        spawn_ranks(_rank_one_sleeps, (str(tmp_path),), 2, limit=2)
    assert multiprocessing.active_children() == []               # (the ranks may not have got as far as a line of their own)
    assert len(children.died) == 1 and "_rank_one_sleeps" in children.died[0] and children.died[0].endswith("(timeout)")
    with pytest.raises(AssertionError, match=r"not started: .* died before"):
        run_program([sys.executable, "-c", "pass"])


def test_a_warning_fails_the_build(tmp_path):
    source = tmp_path / "careless.cpp"
    source.write_text("int main() { int unused = 3; return 0; }\n")
    with pytest.raises(AssertionError, match="unused"):
        build_program("careless", tmp_path, library=False, source=source)
    assert not (tmp_path / "careless").exists() and children.died == []


def test_a_stand_alone_program_builds_with_the_sanitizers_and_runs(tmp_path):
    exe = build_program("plane_scan", tmp_path, library=False, sanitize=True)
    r = run_program([exe])
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stderr[-2000:]
