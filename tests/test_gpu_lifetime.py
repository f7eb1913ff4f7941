"""Every device buffer, pinned buffer, stream and event of the three handles (bdx_ctx, bdx_bamdec, bdx_dist) and of the one-shot entry
points is handed back when its owner goes (csrc/bdx_buf.h): one fresh child process exercises each of them on small inputs under
BDX_ALLOC_TRACE=1 (read once per process, so not in this one), closes every handle and exits; its [bdx free] lines must balance its
[bdx alloc] lines, and what it computed must equal what the same calls return here, without the trace.  (Not a comparison of the
GPU's free memory: the machines are shared.)"""
import ctypes
import json
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu

LENGTHS = [300_000, 200_000]   # 75,000 reads at 15x: several K1 tiles, a few hundred regions, translocations between the two
LONG_RUN = 100                 # records planted at one (tid, pos): more than the 64 up to which KD's short-run path goes


def _inputs():
    from breakdancer_amd.synth import make_genome
    d = make_genome(LENGTHS, coverage=15.0, seed=7, n_translocations=20, threads=4)
    # a run of LONG_RUN records at one (tid, pos) -- a read of chromosome 0 and its copies under other names, and their mates alike
    i = int(np.flatnonzero((d["tid"] == 0) & (d["mtid"] == 0) & (d["mpos"] > d["pos"]))[1000])
    j = int(np.flatnonzero((d["name_key"] == d["name_key"][i]) & (np.arange(len(d["tid"])) != i))[0])
    extra = {k: np.concatenate([np.repeat(v[i:i + 1], LONG_RUN), np.repeat(v[j:j + 1], LONG_RUN)]) for k, v in d.items()}
    extra["name_key"] = np.tile(np.arange(LONG_RUN, dtype=np.uint64) + np.uint64(1 << 60), 2)
    dup = {k: np.concatenate([v, extra[k]]) for k, v in d.items()}
    order = np.lexsort(((dup["flag"] >> 4) & 1, dup["pos"], dup["tid"]))
    return d, {k: v[order] for k, v in dup.items()}


def _table(bd):
    sv = bd.svs()[0]
    return [[int(x) for x in (r["chr"][0], r["pos"][0], r["chr"][1], r["pos"][1], r["flag"], r["size"], r["score"], r["num_reads"])] for r in sv]


def exercise():
    """every handle and one-shot entry point once, all closed again; returns what they computed"""
    import breakdancer_amd as bda
    from breakdancer_amd import bamdec, dist
    from breakdancer_amd.api import LibraryConfig, Options, mark_duplicates, poisson_log_upper_tail
    from breakdancer_amd.bamwrite import write_bam
    out = {}
    d, dup = _inputs()
    opts = Options(transchr_rearrange=True)
    libs = [LibraryConfig(400.0, 30.0, 490.0, 310.0, 100.0)]

    # ---- the context ----
    bd = bda.BreakDancer(opts, libs, 1)
    bd.push_reads(d)
    bd.run()
    out["plain"] = _table(bd)
    out["n_regions"] = int(bd.summary()["n_regions"])
    sv = bd.svs()[0]
    out["junctions"] = bd.count_junction_pairs(sv["chr"][:8, 0], sv["pos"][:8, 0], sv["pos"][:8, 0] + 50).tolist()
    ctx = [r for r in sv if r["chr"][0] != r["chr"][1]][:4]
    ends = [sorted([(int(r["chr"][0]), int(r["pos"][0])), (int(r["chr"][1]), int(r["pos"][1]))]) for r in ctx]
    out["sites"] = bd.count_site_pairs([a + b + (1 << 8,) for a, b in ends], 500).tolist()
    bd.reset_reads()
    bd.collect_support()
    bd.push_reads(d)
    bd.run()
    out["second_run"] = _table(bd)
    out["support"] = int(bd.sv_support()[0][-1])
    bd.close()
    bd = bda.BreakDancer(opts, libs, 1).mark_duplicates()
    bd.push_reads(dup)
    bd.run()
    out["duplicates"] = list(bd.duplicates())
    out["marked_run"] = _table(bd)
    bd.close()
    held = bda.BreakDancer(opts, libs, 1)
    buf = bda._lib.bdx_batch_buf()
    held._chk(held.lib.bdx_acquire_batch(held.h, 1000, ctypes.byref(buf)), "bdx_acquire_batch")
    held.close()   # a batch acquired and not submitted

    # ---- the decoder ----
    with tempfile.TemporaryDirectory() as td:
        path = os.path.join(td, "few.bam")
        write_bam(path, {k: v[:600] for k, v in d.items()}, ["c0", "c1"], threads=1)
        kw = dict(rg_ids=["rg1"], rg_lib=[0], ring_bytes=1 << 20, batch_blocks=3, piece_blocks=2)
        cols, _, _ = bamdec.decode_file(path, **kw)
        out["decoded"] = [int(len(cols["pos"])), int(cols["pos"].astype(np.int64).sum()), int(cols["name_key"][-1])]
        sink = bda.BreakDancer(opts, libs, 1)
        bamdec.decode_file(path, sink=sink, **kw)
        sink.run()
        out["sink"] = [int(sink.summary()["n_reads"]), int(sink.read_class().astype(np.int64).sum())]
        sink.close()
        data = np.fromfile(path, dtype=np.uint8)
        members = bamdec.scan_bgzf(data)
        names, _, k, off = bamdec.bam_header(data, members)
        m = members[k:][members[k:]["inflated_len"] > 0]
        dec = bamdec.BamDecoder(len(names), rg_ids=["rg1"], rg_lib=[0], first_record_offset=off, ring_bytes=1 << 20, batch_blocks=1)
        dec.submit(data, m[:1], last=False)
        dec.submit(data, m[1:2], last=False)
        dec.close()    # with its batches launched, before finish
        inflated, status, _ = bamdec.inflate_blocks(data, m[:3])
        out["inflated"] = [int(len(inflated)), int(inflated.astype(np.int64).sum()), status.tolist()]

    # ---- the sharded run: one rank, twice (the result context borrows the rank's pinned table buffers and gives them back) ----
    rank = dist.DistRun.threads(opts, libs, 1, len(LENGTHS), 200, [0])[0]
    bounds = np.searchsorted(d["tid"], np.arange(len(LENGTHS) + 1))
    for t in range(len(LENGTHS)):
        rank.chromosome(t).push_reads({k: v[bounds[t]:bounds[t + 1]] for k, v in d.items()})
    out["sharded"] = []
    for _ in range(2):
        rank.run(release=False)
        out["sharded"].append(_table(rank.result()))
    rank.release_inputs()
    rank.close()

    # ---- the one-shot entry points ----
    out["poisson"] = poisson_log_upper_tail([3.0, 10.0, 0.5], [5, 2, 1]).tolist()
    mask, groups = mark_duplicates([0] * 6, [10, 10, 10, 50, 50, 90], [0] * 6, [300, 300, 300, 400, 400, 500], [0x63] * 6, [0] * 6, [1, 2, 3, 4, 5, 6])
    out["marks"] = [mask.astype(int).tolist(), int(groups)]
    stats = (ctypes.c_double * 18)()   # two bdx_insert_stats: six doubles and three 64-bit counts each
    x, off = np.arange(300, 340, dtype=np.float64), np.array([0, 25, 40], np.uint32)
    assert bda._lib.load().bdx_insert_size_stats(0, x.ctypes.data_as(ctypes.c_void_p), off.ctypes.data_as(ctypes.c_void_p), 2, stats) == 0
    out["insert_stats"] = [stats[0], stats[2], stats[9], stats[11]]
    out["excluded"] = bamdec.exclude_mask([0, 0, 1, 1], [5, 500, 5, 500], [0, 1, 1, 0], [700, 20, 900, 450], [(0, 400, 600), (1, 0, 10)]).tolist()
    return out


def _trace(stderr):
    """{kind: (lines, bytes)} of the [bdx alloc] and of the [bdx free] lines"""
    tot = {"alloc": {"device": [0, 0], "pinned": [0, 0]}, "free": {"device": [0, 0], "pinned": [0, 0]}}
    for line in stderr.splitlines():
        f = line.split()
        if len(f) >= 5 and f[0] == "[bdx" and f[1] in ("alloc]", "free]") and f[4] == "B":
            t = tot[f[1][:-1]][f[2]]
            t[0] += 1
            t[1] += int(f[3])
    return tot


def test_every_buffer_a_process_allocates_is_freed_when_its_owner_goes():
    p = subprocess.run([sys.executable, os.path.abspath(__file__)], env=dict(os.environ, BDX_ALLOC_TRACE="1"), stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, timeout=600)
    err = p.stderr.decode()
    assert p.returncode == 0, err[-4000:]
    child = json.loads(p.stdout.decode().splitlines()[-1])
    here = json.loads(json.dumps(exercise()))
    assert len(here["plain"]) > 20 and here["n_regions"] > 0 and here["duplicates"][0] >= LONG_RUN - 1
    assert any(r[0] != r[2] for r in here["plain"])            # translocations among the SVs
    assert here["sharded"][0] == here["sharded"][1] and here["plain"] == here["second_run"]
    assert child == here
    t = _trace(err)
    print("trace:", t)
    for kind in ("device", "pinned"):
        assert t["alloc"][kind][0] > 0, kind                    # (an empty trace must not pass)
        assert t["free"][kind] == t["alloc"][kind], (kind, t)


if __name__ == "__main__":
    print(json.dumps(exercise()))
