"""The kernels behind K1 issue their loads before the stores that do not feed them: K2's fills leave as 16-byte
stores strided over the compacting workgroups, the join kernel forwards the region table four 16-byte words at a time, k6_emit_kernel fetches a region's parts four at
a time before it stores their host records, k6_score_kernel requests a stage entry before the list entries of the term before it
leave.  None of that may change a result: every case here is held to the CPU oracle, at the sizes where the reordered code takes
another path -- one workgroup and several, a full turn of the forwarding workgroups and one word more or less, a wave's 64 and a
workgroup's 256 candidates, regions with no part, one, a whole batch of four, one more, and more than two batches."""
import numpy as np
import pytest

from helpers import make_opts
from runner import apply_test_switches, compare, oracle_case, product_from_oracle, product_options

import breakdancer_amd as bda
from breakdancer_amd.api import LibraryConfig

pytestmark = pytest.mark.gpu

# (flag of the first-observed mate, flag of the second): both forward, both reverse, forward-reverse with an insert far above `upper`
KINDS = {"ff": (0x1 | 0x40, 0x1 | 0x40), "rr": (0x1 | 0x10 | 0x20 | 0x40, 0x1 | 0x10 | 0x20 | 0x40), "fr": (0x1 | 0x20 | 0x40, 0x1 | 0x10 | 0x80)}
NORMAL = (0x1 | 0x2 | 0x20 | 0x40, 0x1 | 0x2 | 0x10 | 0x80)
GAP = 5000        # between clusters: more than any window here, so every cluster is a region of its own
OPTS = dict(min_read_pair=1, min_len=-1, score_threshold=-1)


def _config(nlibs):
    return "".join("readgroup:rg%d\tplatform:illumina\tmap:x.bam\treadlen:100.00\tlib:lib%d\tlower:310.00\tupper:490.00\tmean:400.00\tstd:30.00\n"
                   % (i, i) for i in range(1, nlibs + 1))


def _case(clusters, nlibs=1, normals_after=0, normals_tail=0):
    """clusters: one list per cluster of (library, kind) per pair -- kind None: a read without a mate.  Both mates of a pair lie in
    their cluster, 4 bp apart; normals_after proper pairs (library 0) follow every cluster, normals_tail more the last one.  One
    position-sorted stream."""
    pos, mpos, flag, isize, lib, name = [], [], [], [], [], []
    at, next_name = 1000, 1
    for ci, c in enumerate(clusters):
        for p, (l, kind) in enumerate(c):
            for mate in ((0,) if kind is None else (0, 1)):
                pos.append(at + (2 * p + mate) * 4)
                mpos.append(pos[-1] + 5000)
                flag.append(KINDS[kind or "ff"][mate])
                isize.append(-5100 if (kind == "fr" and mate) else 5100)
                lib.append(l)
                name.append(next_name)
            next_name += 1
        at = (pos[-1] if pos else at) + GAP
        n_normal = normals_after + (normals_tail if ci == len(clusters) - 1 else 0)
        for q in range(n_normal):
            for mate in (0, 1):
                pos.append(at + 30 * q + 300 * mate)
                mpos.append(at + 30 * q + 300 * (1 - mate))
                flag.append(NORMAL[mate])
                isize.append(-400 if mate else 400)
                lib.append(0)
                name.append(next_name)
            next_name += 1
        if n_normal:
            at = at + 30 * n_normal + 300 + GAP
    return _stream(pos, mpos, flag, isize, lib, name, nlibs)


def _stream(pos, mpos, flag, isize, lib, name, nlibs):
    n = len(pos)
    order = np.argsort(np.array(pos, np.int64), kind="stable")
    pos = np.array(pos, np.int32)[order]
    flag = np.array(flag, np.uint16)[order]
    st = dict(tid=np.zeros(n, np.int32), pos=pos, mtid=np.zeros(n, np.int32), mpos=np.array(mpos, np.int32)[order], isize=np.array(isize, np.int32)[order],
              flag=flag, qlen=np.full(n, 100, np.int32), bdqual=np.full(n, 60, np.uint8),
              rg=["rg%d" % (lib[i] + 1) for i in order], name_id=np.array(name, np.uint64)[order])
    return _config(nlibs), [st], ["c1"]


def _span_case(specs, nlibs):
    """specs: per candidate (libraries of its pairs, libraries of the proper pairs between its two regions).  The first-observed mates
    of a candidate's pairs form one region, the second-observed ones another 2,000 bp on, and the proper pairs lie between the two:
    a candidate over two regions, with a Poisson term per library of its pairs and a copy number per counter key met in between."""
    pos, mpos, flag, isize, lib, name = [], [], [], [], [], []
    at, next_name = 1000, 1
    for pair_libs, normal_libs in specs:
        for p, l in enumerate(pair_libs):
            for mate in (0, 1):
                pos.append(at + 2000 * mate + 4 * p)
                mpos.append(pos[-1] + 5000)
                flag.append(KINDS["ff"][mate]); isize.append(5100); lib.append(l); name.append(next_name)
            next_name += 1
        for q, l in enumerate(normal_libs):
            for mate in (0, 1):
                pos.append(at + 600 + 20 * q + 300 * mate)
                mpos.append(at + 600 + 20 * q + 300 * (1 - mate))
                flag.append(NORMAL[mate]); isize.append(-400 if mate else 400); lib.append(l); name.append(next_name)
            next_name += 1
        at += 2000 + GAP
    return _stream(pos, mpos, flag, isize, lib, name, nlibs)


def _context_of(run):
    libs = [LibraryConfig(*[float(x) for x in run.lib_f[i]], min_mapping_quality=int(run.lib_i[i, 0]),
                          bam_file_index=int(run.lib_i[i, 1]), name=run.lib_names[i]) for i in range(run.nlibs)]
    return apply_test_switches(bda.BreakDancer(product_options(run.opts), libs, run.nbams, ntids=0, max_read_window_size=run.w0, device=0))


# ---- K2: the fills, 16 bytes a store ----------------------------------------------------------------------------------------------------

_FILL_RUNS = {}


def _fill_runs(n_reads):
    """(oracle run of an input of n_reads anomalous reads, oracle run of an input of n_reads reads of which a sixth are anomalous and
    n_anomalous % 4 == 2 -- the fills' last words go one at a time), computed once"""
    if n_reads not in _FILL_RUNS:
        many = _case([[(0, "ff")] * 6] * (n_reads // 12))
        k = n_reads // 36 | 1   # clusters of the second input: an odd number of six reads each
        after = (n_reads - 6 * k) // (2 * k)
        few = _case([[(0, "ff")] * 3] * k, normals_after=after, normals_tail=(n_reads - 6 * k) // 2 - after * k)
        runs = tuple(oracle_case(*c, make_opts(**OPTS)) for c in (many, few))
        assert runs[0].n_merged == runs[1].n_merged == n_reads
        _FILL_RUNS[n_reads] = runs
    return _FILL_RUNS[n_reads]


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("n_reads", [3072, 9216])
def test_k2_fills_clear_what_an_earlier_run_left(n_reads, mode):
    """One context, two runs, bdx_reset_reads between them.  The first input joins n_reads / 2 pairs: K4's slot table, partner[] and
    pair_lo[] are full of them.  The second has a sixth as many anomalous reads: every word its join and K3 look at must have been
    filled again by its own K2 -- a fill that is skipped or strides wrongly leaves a mate of the first run in place, which shows as
    a wrong join (or as a name seen three times).  3,072 reads are three super tiles, one compacting workgroup; 9,216 are three.
    Modes 1 and 2 are the enqueue-ahead settings: with an input of the same size as the run before, mode 2 sizes the second run from
    the first and launches k2_compact_side_kernel, whose last workgroup finalises pass 1, returns early and takes no part in the fills."""
    many, few = _fill_runs(n_reads)
    bd = _context_of(many)
    try:
        bd.set_enqueue_ahead(mode)
        for run in (many, few):
            bd.push_reads(run.merged_soa())
            bd.run()
            s = compare(run, bd)
            assert not bd.was_replayed()
            bd.reset_reads()
        assert s["n_anomalous"] % 4 == 2 and 0 < s["n_anomalous"] < n_reads // 4
    finally:
        bd.close()


# ---- K4: the forward of the region table ----------------------------------------------------------------------------------------------

# a turn of the forwarding workgroups: 32 workgroups x 256 lanes x 4 words of 16 bytes (kJoinForwardBlocks, kJoinForwardAhead in
# k4_join.hip); a region's record is 36 bytes
TURN_QUADS = 32 * 256 * 4
REGION_WORDS = 9
TURN_REGIONS = TURN_QUADS * 4 // REGION_WORDS   # 14,563 regions end three quads short of a full turn, 14,564 start the next one


@pytest.mark.parametrize("nkeys", [1, 2])
@pytest.mark.parametrize("n_regions", [2, 63, 64, 65, TURN_REGIONS - 1, TURN_REGIONS, TURN_REGIONS + 1])
def test_region_table_reaches_the_host_whole(n_regions, nkeys):
    """bdx_get_regions and the host walk read the table the join kernel's forwarding workgroups left in pinned memory: region counts
    around a wave, and around one turn of those workgroups (the last partial turn, the loop of whole ones).  With two counter keys
    (CN_lib, two libraries) the block of per-key counts behind the records is twice as wide.  (Entry 0 of the table is a placeholder, as in
    the reference: a table of 2 is the smallest there is, one region.)"""
    assert TURN_REGIONS * REGION_WORDS // 4 < TURN_QUADS <= (TURN_REGIONS + 1) * REGION_WORDS // 4
    clusters = [[(i % nkeys, "ff"), ((i // 2) % nkeys, "ff")] for i in range(n_regions - 1)]
    run = oracle_case(*_case(clusters, nlibs=nkeys), make_opts(cn_lib=1 if nkeys > 1 else 0, **OPTS))
    assert run.n_regions == n_regions and run.W < GAP
    bd = product_from_oracle(run, host_walk=True)
    try:
        compare(run, bd)
        assert bd.walk_split()[1] == run.n_svs   # every SV came from the host's walk over the forwarded table
    finally:
        bd.close()


# ---- k6_emit_kernel: the host's groups, four parts at a time --------------------------------------------------------------------------

def test_host_groups_of_regions_with_no_part_one_a_batch_and_more():
    """bdx_set_host_walk(1): every group goes to the host list.  A region's parts are its distinct (library, flag) combinations --
    none (reads without mates), 1, 4 (one batch), 5, 9 and 12 (more than two batches) -- and the walk's result is the oracle's."""
    combos = [(l, k) for k in ("ff", "rr", "fr") for l in range(4)]
    shapes = [[(0, None)] * 3, combos[:1] * 2, combos[:4], combos[:5] + combos[:2], combos[:9], combos]
    clusters = [shapes[i % len(shapes)] for i in range(40 * len(shapes))]   # 240 regions: several waves of the kernel
    run = oracle_case(*_case(clusters, nlibs=4), make_opts(**OPTS))
    assert run.n_regions == len(clusters) + 1   # (entry 0 is a placeholder)
    bd = product_from_oracle(run, host_walk=True)
    try:
        compare(run, bd)
        dev, host, groups = bd.walk_split()
        assert dev == 0 and host == run.n_svs and groups >= 40 * 5   # (at least a group per region that holds a pair)
    finally:
        bd.close()


# ---- k6_score_kernel: the two flat lists ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fisher", [0, 1])
@pytest.mark.parametrize("cn_lib", [0, 1])
@pytest.mark.parametrize("n_svs", [63, 64, 65, 257])
def test_score_lists_across_a_wave_and_a_workgroup(n_svs, cn_lib, fisher):
    """Four libraries; candidate i has pairs of 1 + i % 4 of them and proper pairs of i % 5 of them between its two regions, so a wave
    holds candidates with one term and with several side by side, and -- with CN_lib, a counter key per library -- with no copy-number
    entry, one and several (without it at most one).  63 / 64 / 65 candidates cross a wave, 257 a workgroup.  bdx_get_svs and
    bdx_get_sv_lists against the oracle; with -f the Fisher tail goes through ltail_host."""
    specs = [([(i + j) % 4 for j in range(1 + i % 4) for _ in range(2)], [(i + j) % 4 for j in range(i % 5) for _ in range(3)]) for i in range(n_svs)]
    run = oracle_case(*_span_case(specs, 4), make_opts(cn_lib=cn_lib, print_af=cn_lib, fisher=fisher, **OPTS))
    assert run.n_svs == n_svs and run.nlibs == 4
    bd = product_from_oracle(run)
    try:
        compare(run, bd)
        svs, (li, lp), (ck, cv) = bd.svs()
        assert set(svs["lib_count"].tolist()) == {1, 2, 3, 4} and len(li) == int(svs["lib_count"].sum())
        assert set(svs["cn_count"].tolist()) == ({0, 1, 2, 3, 4} if cn_lib else {0, 1}) and len(ck) == int(svs["cn_count"].sum())
    finally:
        bd.close()


# ---- early exits ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n_anomalous", [0, 1])
def test_no_anomalous_read_and_exactly_one(n_anomalous):
    """Every reordered kernel leaves early somewhere; with nothing to do, or one read, it must still fall through its stores."""
    clusters = [[(0, None)]] * n_anomalous + [[]]
    run = oracle_case(*_case(clusters, normals_after=700), make_opts(**OPTS))
    assert run.n_merged == 2 * 700 * len(clusters) + n_anomalous
    for host_walk in (False, True):
        bd = product_from_oracle(run, host_walk=host_walk)
        try:
            s = compare(run, bd)
            assert s["n_anomalous"] == n_anomalous
        finally:
            bd.close()
