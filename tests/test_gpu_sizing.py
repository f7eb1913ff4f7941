"""The sizing pass and the stages agree on every buffer of the stages behind pass 1 (csrc/bdx_api.hip: size_compact .. size_k6, called
by presize_stages and at the head of each stage): a fresh child process under BDX_ALLOC_TRACE=1 (read once per process, so not in this
one) reserves, pushes, runs and runs again, with a marker line on stderr between the phases.  What bdx_reserve sized, the first run must
not have to grow -- its prior for the anomalous reads is the first run's own enqueue-ahead guess, n / 32 + 4096 --, and the second run
must allocate nothing at all.  A size function that forgets a buffer, or a stage that wants more than its size function gave it, shows
as an allocation or a regrowth in the wrong phase."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu

LENGTH = 3_600_000   # 1.08 M reads at 30x: just above the 2^20 reads below which no sizing pass runs; 1 % of the pairs discordant
PHASES = ("reserve", "push", "first run", "second run")


def exercise():
    """bdx_reserve(n), one push of all reads, bdx_run twice; a marker on stderr behind each phase.  Returns the two tables"""
    import breakdancer_amd as bda
    from breakdancer_amd.api import LibraryConfig, Options
    from breakdancer_amd.synth import make_chromosome
    from test_gpu_lifetime import _table
    d = make_chromosome(length=LENGTH, seed=5)
    n = len(d["tid"])
    assert n >= 1 << 20

    def mark(phase):
        sys.stderr.write("== end of %s\n" % phase)
        sys.stderr.flush()
    bd = bda.BreakDancer(Options(), [LibraryConfig(400.0, 30.0, 490.0, 310.0, 100.0)], 1)
    bd._chk(bd.lib.bdx_reserve(bd.h, n), "bdx_reserve")
    mark(PHASES[0])
    bd.push_reads(d)
    mark(PHASES[1])
    out = {"n": n}
    bd.run()
    out["first"] = _table(bd)
    out["n_anomalous"] = int(bd.summary()["n_anomalous"])
    mark(PHASES[2])
    bd.run()
    out["second"] = _table(bd)
    mark(PHASES[3])
    bd.close()
    return out


def _phases(stderr):
    """{phase: the [bdx alloc] / [bdx free] lines written before its marker}"""
    out, cur = {}, []
    for line in stderr.splitlines():
        if line.startswith("== end of "):
            out[line[len("== end of "):]] = cur
            cur = []
        elif line.startswith("[bdx alloc]") or line.startswith("[bdx free]"):
            cur.append(line)
    return out


def test_a_run_grows_nothing_the_reserve_sized_and_a_second_run_allocates_nothing():
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    p = subprocess.run([sys.executable, os.path.abspath(__file__)], env=dict(os.environ, BDX_ALLOC_TRACE="1"), stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, timeout=600)
    err = p.stderr.decode()
    assert p.returncode == 0, err[-4000:]
    child = json.loads(p.stdout.decode().splitlines()[-1])
    ph = _phases(err)
    for name in PHASES:
        print(name, "allocations:", sum(l.startswith("[bdx alloc]") for l in ph[name]), "frees:", sum(l.startswith("[bdx free]") for l in ph[name]))
    reserved = [l for l in ph["reserve"] if l.startswith("[bdx alloc]")]
    assert len(reserved) > 40, reserved                       # the read store's columns and the later stages' buffers (an empty trace must not pass)
    assert any(" pinned " in l for l in reserved)
    # the first run: nothing regrown (a regrowth says so on its line, and frees first), so nothing of the reserve phase was too small
    for name in ("push", "first run"):
        assert not [l for l in ph[name] if "(regrown" in l or l.startswith("[bdx free]")], (name, ph[name])
    assert ph["second run"] == []
    # 1 % of the pairs discordant: inside the prior, so the first run was not repeated with exact sizes
    assert 0 < child["n_anomalous"] <= child["n"] // 32 + 4096
    here = json.loads(json.dumps(exercise()))
    assert len(here["first"]) > 100 and here["first"] == here["second"]
    assert child == here


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    print(json.dumps(exercise()))
