"""The count of anomalous reads that finalize_kernel posts ahead of the pass-1 record (exact sizing, bdx_set_enqueue_ahead(0)):
one stamped 64-bit word per chunk of the anomalous column, read by the host while finalize2_kernel still runs.

A chunk is 4,096 super tiles = 16,384 tiles = 4,194,304 reads, so the chunk words can go wrong at that size and one read beyond it;
the debug switch "no_poll" is the route that waits for the record first, as every run did before."""
import numpy as np
import pytest

from helpers import OracleRun, assert_same, context, make_opts, snapshot
from runner import compare, oracle_case, product_from_oracle

from breakdancer_amd.synth import make_chromosome

pytestmark = pytest.mark.gpu

CHUNK_READS = 4096 * 4 * 256
CFG = "readgroup:rg1\tplatform:illumina\tmap:syn.bam\treadlen:100.00\tlib:lib1\tlower:310.00\tupper:490.00\tmean:400.00\tstd:30.00\n"


def _stream(d):
    return dict(tid=d["tid"], pos=d["pos"], mtid=d["mtid"], mpos=d["mpos"], isize=d["isize"], flag=d["flag"],
                qlen=d["qlen"].astype(np.int32), bdqual=d["mapq"], rg=["rg1"] * len(d["tid"]), name_id=d["name_key"])


def _cut(d, n):
    assert len(d["tid"]) >= n
    return {k: v[:n] for k, v in d.items()}


# ---- 1. small inputs against the oracle ----------------------------------------------------------------------------------------------

def _small(kind):
    if kind == "no reads":
        d = _cut(make_chromosome(length=20_000, seed=2), 0)
    elif kind == "no anomalous pair":
        d = make_chromosome(length=300_000, seed=3, discordant=0.0, std=5.0)   # (inserts 400 +- 5: none near a cutoff)
    elif kind == "one partial tile":
        d = _cut(make_chromosome(length=40_000, seed=4, discordant=0.05), 200)
    else:
        d = make_chromosome(length=40_000, seed=5, discordant=0.01, n_pairs=1300)   # 2,600 reads: ten full tiles and a partial one
    return d


@pytest.mark.parametrize("kind", ["no reads", "no anomalous pair", "one partial tile", "a few tiles"])
def test_small_inputs_match_the_oracle(kind, monkeypatch):
    monkeypatch.setenv("BDX_NO_SPECULATE", "1")   # product_from_oracle: set_enqueue_ahead(0)
    d = _small(kind)
    run = oracle_case(CFG, [_stream(d)], ["chrS"], make_opts(min_read_pair=2, score_threshold=-1))
    bd = product_from_oracle(run)
    s = compare(run, bd)
    if kind == "no reads":
        assert s["n_reads"] == 0 and s["n_anomalous"] == 0
    elif kind == "no anomalous pair":
        assert s["n_reads"] > 1000 and s["n_anomalous"] == 0 and s["n_svs"] == 0
    elif kind == "one partial tile":
        assert s["n_reads"] == 200
    else:
        assert s["n_reads"] == 2600 and s["n_anomalous"] > 0
    bd.close()


def fresh(arrs, mode=0, **debug):
    bd = context(mode, **debug)
    bd.push_reads(arrs)
    snap = snapshot(bd.run())
    bd.close()
    return snap


@pytest.fixture(scope="module")
def chromosome():
    """one chromosome of a little more than a chunk of reads; every input below is a prefix of it"""
    d = make_chromosome(length=15_000_000, seed=21)
    assert len(d["tid"]) >= CHUNK_READS + 300_000
    return d


@pytest.fixture(scope="module")
def old_route(chromosome):
    """results of the route that waits for the pass-1 record first, per input length, each computed once on a fresh context"""
    cache = {}

    def get(n):
        if n not in cache:
            cache[n] = fresh(_cut(chromosome, n), no_poll=1)
        return cache[n]
    return get


# ---- 2. the chunk boundary against the old route --------------------------------------------------------------------------------------

@pytest.mark.parametrize("n, debug", [(CHUNK_READS, {}), (CHUNK_READS + 1, {}), (CHUNK_READS + 1, {"max_chunks": 1})],
                         ids=["one full chunk", "two chunks, one tile in the second", "one chunk of two rounds"])
def test_chunk_boundary_equals_the_record_first_route(chromosome, old_route, n, debug):
    got = fresh(_cut(chromosome, n), **debug)
    assert got["summary"]["n_reads"] == n and got["summary"]["n_anomalous"] > 10_000 and got["summary"]["n_svs"] > 100
    assert_same(got, old_route(n))


# ---- 3. words of earlier runs -----------------------------------------------------------------------------------------------------------

def test_words_of_earlier_runs_do_not_satisfy_the_poll(chromosome, old_route):
    """one context over inputs of one, two and one chunks with different counts, then three times over the same input"""
    sizes = [1_000_000, CHUNK_READS + 300_000, 600_000]
    counts = [old_route(n)["summary"]["n_anomalous"] for n in sizes]
    assert len(set(counts)) == 3 and min(counts) > 0
    bd = context()
    for i, n in enumerate(sizes):
        if i:
            bd.reset_reads()
        bd.push_reads(_cut(chromosome, n))
        assert_same(snapshot(bd.run()), old_route(n))
    for _ in range(3):
        assert_same(snapshot(bd.run()), old_route(sizes[-1]))
    bd.close()


# ---- 4. the other modes ------------------------------------------------------------------------------------------------------------------

def test_enqueue_ahead_modes_give_the_same_tables(chromosome):
    n = 1_200_000   # (from 2^20 reads on a first run takes the prior)
    arrs = _cut(chromosome, n)
    want = fresh(arrs)
    assert want["summary"]["n_anomalous"] > n // 4096 + 4096   # (the prior of spec_test is too small)
    assert_same(fresh(arrs, mode=1), want)
    assert_same(fresh(arrs, mode=1, spec_test=1), want)        # guess too small on a first run
    bd = context(mode=2)
    bd.push_reads(arrs)
    assert_same(snapshot(bd.run()), want)                      # no history: the prior
    assert_same(snapshot(bd.run()), want)                      # sized from the previous run
    bd.set_debug("spec_test", 1)
    assert_same(snapshot(bd.run()), want)                      # half of the previous run's count: run again
    bd.close()
