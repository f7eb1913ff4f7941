"""bdx_run's sizing routes with polling off: the waits for the region table, the pair groups and the final table then go through
events (ev_regions behind the join, ev_groups inside k6_then_walk, the stream for the table) instead of ready words.  The other
tests run "no_poll" with enqueue-ahead off only; here the event flavour stands behind an enqueue-ahead launch and behind its retry.

1.2 M reads is just above the 2^20 from which a first run takes the prior: the smallest size at which these routes exist."""
import pytest

from helpers import assert_same, context, snapshot

from breakdancer_amd.synth import make_chromosome

pytestmark = pytest.mark.gpu

N = 1_200_000
N_PREFIX = 600_000


def _cut(d, n):
    assert len(d["tid"]) >= n
    return {k: v[:n] for k, v in d.items()}


def _fresh(arrs, mode=0, **debug):
    bd = context(mode, **debug)
    bd.push_reads(arrs)
    snap = snapshot(bd.run())
    bd.close()
    return snap


@pytest.fixture(scope="module")
def reads():
    return _cut(make_chromosome(length=4_000_000, seed=21), N)


@pytest.fixture(scope="module")
def want(reads):
    """exact sizing with default polling, on a fresh context"""
    ref = _fresh(reads)
    assert ref["summary"]["n_reads"] == N
    assert ref["summary"]["n_anomalous"] > N // 4096 + 4096   # (the prior of spec_test is too small: the retry is taken)
    return ref


def test_prior_on_a_fresh_context_without_polling(reads, want):
    assert_same(_fresh(reads, mode=1, no_poll=1), want)


def test_retry_on_a_first_run_without_polling(reads, want):
    assert_same(_fresh(reads, mode=1, no_poll=1, spec_test=1), want)


def test_history_retry_and_a_changed_input_on_one_context(reads, want):
    bd = context(mode=2, no_poll=1)
    bd.push_reads(reads)
    assert_same(snapshot(bd.run()), want)      # no history: the prior
    assert_same(snapshot(bd.run()), want)      # sized from the previous run
    bd.set_debug("spec_test", 1)
    assert_same(snapshot(bd.run()), want)      # half of the previous run's count: run again
    # a changed input size drops the history: polling on again, the prefix is sized exactly (it is too short for a prior)
    bd.set_debug("no_poll", 0)
    bd.reset_reads()
    prefix = _cut(reads, N_PREFIX)
    bd.push_reads(prefix)
    assert_same(snapshot(bd.run()), _fresh(prefix))
    bd.close()
