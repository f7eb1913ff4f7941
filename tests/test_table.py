"""CPU tests of the table formatter (host/table.cpp) through bin/bdx-table-check, which links neither libbdx nor the GPU:

1. the CPU oracle's SV records and lists of the chr21 fixture, for every option set of test_gpu_cli.py, formatted by 1, 2 and 5 threads,
   against the rows of the oracle's own text (the oracle's printer is the independent side);
2. a Python restatement of one row -- "%g" with six digits until the first copy number has gone through the stream, "%.2f" behind it,
   "-nan" -- held to those oracle texts and then used on
3. synthetic tables of 8-40 rows that put the first row leaving the stream `fixed` at every place relative to a thread's slice, at thread
   counts 1, 2, 3, 5, the row count and above it; a Python model of the slice rule with each of three slips shows that the tables tell
   the slips apart;
4. all of it again on the tool built with -fsanitize=address,undefined, and the several-thread cases on a -fsanitize=thread build."""
import os
import struct
import subprocess

import pytest

from helpers import GOLDEN, ROOT, load_chr21, make_opts

HOST = os.path.join(ROOT, "breakdancer_amd", "host")
SOURCES = [os.path.join(HOST, f) for f in ("table_check_main.cpp", "table.cpp", "options.cpp", "config.cpp")]
CHR21_CONFIG = os.path.join(GOLDEN, "chr21", "inv_del_bam_config")
CTX = 8                                    # BDX_ARP_CTX
TYPES = {False: {1: "INV", 2: "DEL", 3: "INS", 4: "ITX", 5: "INV", 8: "CTX"}, True: {1: "INV", 3: "INS", 4: "DEL", 5: "INV", 8: "CTX"}}   # Options::sv_type, -l
NAN_NEG, NAN_POS = 0xFFC00000, 0x7FC00000


def bits(x):
    return struct.unpack("<I", struct.pack("<f", x))[0]


def value(b):
    return struct.unpack("<f", struct.pack("<I", b))[0]


# ---------------------------------------------------------------------------------------------------------------------------------
# the tool
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tools(tmp_path_factory):
    """bin/bdx-table-check, and its sources built again under ASan + UBSan and under TSan"""
    plain = os.path.join(ROOT, "bin", "bdx-table-check")
    if not os.path.exists(plain):
        subprocess.check_call(["make", "-C", ROOT, "bin/bdx-table-check"], stdout=subprocess.DEVNULL)
    d = tmp_path_factory.mktemp("san")
    out = {"plain": plain}
    compiles = []
    for name, flag in (("asan", "-fsanitize=address,undefined"), ("tsan", "-fsanitize=thread")):
        out[name] = str(d / ("bdx-table-check-" + name))
        compiles.append(subprocess.Popen(["g++", "-O1", "-g", "-std=c++17", flag, "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-pthread",
                                          "-I" + os.path.join(ROOT, "include"), "-o", out[name]] + SOURCES))
    assert [c.wait() for c in compiles] == [0, 0]
    return out


def table_file(path, config, args, targets, rows):
    with open(path, "w") as f:
        f.write("config %s\nargs %s\ntargets %s\n" % (config, " ".join(args), " ".join(targets)))
        for r in rows:
            f.write("sv %s %08x %d %d %s %s\n" % (" ".join(str(v) for v in r["ints"]), r["af"], len(r["libs"]), len(r["cn"]),
                                                 " ".join("%d %d" % lp for lp in r["libs"]), " ".join("%d %08x" % kc for kc in r["cn"])))


def run_tool(exe, path, threads, fixed=False):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1", TSAN_OPTIONS="halt_on_error=1")
    p = subprocess.run([exe, str(path), str(threads)] + (["fixed"] if fixed else []), stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env)
    err = p.stderr.decode()
    assert p.returncode == 0 and "Sanitizer" not in err and "runtime error" not in err, (exe, threads, err)
    lines = p.stdout.decode().split("\n")
    assert lines[-1] == "" and lines[-2].startswith("#state ")
    return lines[:-2], lines[-2]


def builds_for(tools, threads):
    """every build runs every case, the thread-sanitized one the cases that start threads"""
    return [tools["plain"], tools["asan"]] + ([tools["tsan"]] if threads > 1 else [])


# ---------------------------------------------------------------------------------------------------------------------------------
# one row, restated (BreakDancer.cpp:395-497): `state` is the stream's [fixed, precision], which a printed copy number changes for good
# ---------------------------------------------------------------------------------------------------------------------------------
def through_stream(b, state):
    x = value(b)
    if x != x:
        return "-nan" if b >> 31 else "nan"
    return ("%.*f" if state[0] else "%.*g") % (state[1], x)


def row_text(r, state, cfg, by_lib, with_af, long_insert, targets):
    """cfg: (library names, library -> BAM path, number of BAMs)"""
    lib_names, lib_bam, nbams = cfg
    chr0, pos0, fwd0, rev0, chr1, pos1, fwd1, rev1, flag, size, score, nreads = r["ints"]
    cn = dict(r["cn"])
    if by_lib:
        sp = ":".join("%s|%d,%s" % (lib_names[lib], pairs, "%.2f" % value(cn[lib]) if flag != CTX and lib in cn else "NA") for lib, pairs in r["libs"])
    else:
        per_bam = {}
        for lib, pairs in r["libs"]:
            per_bam[lib_bam[lib]] = per_bam.get(lib_bam[lib], 0) + pairs
        sp = ":".join("%s|%d" % kv for kv in sorted(per_bam.items())) or "NA"
    name = lambda t: targets[t] if 0 <= t < len(targets) else str(t)
    out = [name(chr0), str(pos0), "%d+%d-" % (fwd0, rev0), name(chr1), str(pos1), "%d+%d-" % (fwd1, rev1), TYPES[long_insert].get(flag, ""),
           str(size), str(score), str(nreads), sp]
    if with_af:
        out.append(through_stream(r["af"], state))
    if not by_lib and flag != CTX:
        for b in range(nbams):
            if b in cn:
                state[0], state[1] = True, 2
                out.append(through_stream(cn[b], state))
            else:
                out.append("NA")
    return "\t".join(out)


def sets_fixed(r, nbams, by_lib):
    return not by_lib and r["ints"][8] != CTX and any(0 <= k < nbams for k, _ in r["cn"])


def table_text(rows, threads, start, slip=None, **kw):
    """The rows as `threads` slices give them, each slice starting in the state the sequential loop would have reached, and the state the
    stream is left in.  threads == 1 IS the sequential loop.  slip: one of the three mistakes the tables below are there to catch."""
    nbams, by_lib = kw["cfg"][2], kw["by_lib"]
    if threads <= 1:
        state = list(start)
        return [row_text(r, state, **kw) for r in rows], state
    flip = None if start[0] else next((k for k, r in enumerate(rows) if sets_fixed(r, nbams, by_lib)), None)
    out = []
    for t in range(threads):
        k0, k1 = len(rows) * t // threads, len(rows) * (t + 1) // threads
        state = [start[0], 6] if slip == "precision" else list(start)
        if flip is not None and (k0 >= flip if slip == ">=" else k0 > flip):
            state = [True, 2]
        out += [row_text(r, state, **kw) for r in rows[k0:k1]]
    return out, ([True, 2] if flip is not None and slip != "final" else list(start))


def state_line(state):
    return "#state %d %d" % (int(state[0]), state[1])


# ---------------------------------------------------------------------------------------------------------------------------------
# 1, 2: the oracle's records against the oracle's text
# ---------------------------------------------------------------------------------------------------------------------------------
def _cli_cases():
    import test_gpu_cli as T
    out = []
    for _, args in T.CASES:
        out.append((args, dict(cn_lib=int("-a" in args), print_af=int("-h" in args), chr_tid=22 if "-o" in args else -1)))
    return out + [(args, kw) for args, kw in T.OPTSETS]


CLI_CASES = _cli_cases()
_oracle_runs = {}


def oracle_case(i):
    """(the oracle's run, its printed SVs as rows for the tool, the rows of its text), computed once per case"""
    if i not in _oracle_runs:
        run = load_chr21(make_opts(**CLI_CASES[i][1])).run()
        lib_off = [0] + run.sv_i[:, 13].cumsum().tolist()
        cn_off = [0] + run.sv_i[:, 14].cumsum().tolist()
        rows = []
        for k in range(run.n_svs):
            if not run.sv_i[k, 12]:
                continue
            rows.append(dict(ints=run.sv_i[k, :12].tolist(), af=bits(run.sv_d[k, 1]),
                             libs=[tuple(run.sv_lib[j].tolist()) for j in range(lib_off[k], lib_off[k + 1])],
                             cn=[(int(run.sv_cn_key[j]), bits(run.sv_cn_val[j])) for j in range(cn_off[k], cn_off[k + 1])]))
        text_rows = [l for l in run.text.splitlines() if not l.startswith("#")]
        _oracle_runs[i] = (run, rows, text_rows)
    return _oracle_runs[i]


@pytest.mark.parametrize("i", range(len(CLI_CASES)), ids=[" ".join(c[0]) or "default" for c in CLI_CASES])
def test_oracle_records_formatted_by_threads_equal_the_oracle_text(i, tools, tmp_path):
    run, rows, text_rows = oracle_case(i)
    assert len(rows) == len(text_rows)
    f = tmp_path / "table.txt"
    table_file(f, CHR21_CONFIG, CLI_CASES[i][0], run.targets, rows)
    for threads in (1, 2, 5):
        for exe in builds_for(tools, threads):
            got, _ = run_tool(exe, f, threads)
            assert got == text_rows, (exe, threads)


@pytest.mark.parametrize("i", range(len(CLI_CASES)), ids=[" ".join(c[0]) or "default" for c in CLI_CASES])
def test_the_restated_row_gives_the_oracle_text(i):
    run, rows, text_rows = oracle_case(i)
    kw = CLI_CASES[i][1]
    cfg = (run.lib_names, [run.bam_names[run.lib_i[l, 1]] for l in range(run.nlibs)], run.nbams)
    for threads in (1, 2, 5):
        got, _ = table_text(rows, threads, [False, 6], cfg=cfg, by_lib=bool(kw.get("cn_lib")), with_af=bool(kw.get("print_af")),
                            long_insert=bool(kw.get("illumina_long_insert")), targets=run.targets)
        assert got == text_rows, threads


# ---------------------------------------------------------------------------------------------------------------------------------
# 3: synthetic tables.  Three libraries over two BAMs: libA -> a.bam, libB and libC -> dir/b.bam
# ---------------------------------------------------------------------------------------------------------------------------------
SYN_CONFIG = "".join("readgroup:rg%d\tplatform:illumina\tmap:%s\treadlen:90\tlib:%s\tnum:100\tlower:200\tupper:500\tmean:400\tstd:30\n" % (i, m, l)
                     for i, (m, l) in enumerate((("dir/b.bam", "libB"), ("a.bam", "libA"), ("dir/b.bam", "libC"))))
SYN_CFG = (["libA", "libB", "libC"], ["a.bam", "dir/b.bam", "dir/b.bam"], 2)
SYN_TARGETS = ["c0", "c1", "c2"]
AFS = [0.123456, 0.5, 1.0, 0.0333333, 2.5e-05, 0.987654321, 12.3456789]     # "%.6g" and "%.2f" of every one differ


def plain_row(k, flag=2, cn=(), af=None):
    """row k: no copy number unless given; an allele frequency whose six-digit and two-decimal texts differ"""
    return dict(ints=[k % 3, 100 + 7 * k, k % 5, k % 4, (k + (flag == CTX)) % 3 if k % 11 else 7, 900 + 7 * k, k % 3, k % 6, flag, 800 - k, 40 + k, 2 + k % 9],
                af=bits(AFS[k % len(AFS)]) if af is None else af, libs=[(k % 3, 2 + k % 4)] + ([((k + 1) % 3, 1)] if k % 2 else []), cn=list(cn))


def with_flip_at(n, flip, args=("-h",), **kw):
    """n rows of which row `flip` is the first (and only) one to print a copy number through the stream"""
    return dict(args=list(args), rows=[plain_row(k, cn=[(0, bits(1.5)), (1, bits(0.25))] if k == flip else ()) for k in range(n)], **kw)


def synthetic_tables():
    t = {"empty": dict(args=["-h"], rows=[]),
         "flip-at-row-0": with_flip_at(12, 0),
         "flip-at-last-row": with_flip_at(13, 12),
         "no-flip": with_flip_at(11, None),
         # 20 rows on 5 threads: slices start at 0, 4, 8, 12, 16; on 2 at 0, 10; on 3 at 0, 6, 13
         "flip-at-k0-minus-1": with_flip_at(20, 7), "flip-at-k0": with_flip_at(20, 8), "flip-at-k0-plus-1": with_flip_at(20, 9),
         "flip-at-k0-of-two-threads": with_flip_at(20, 10),
         "stream-arrives-fixed": with_flip_at(16, 9, fixed=True), "stream-arrives-fixed-no-copy-number": with_flip_at(9, None, fixed=True),
         "without-af": with_flip_at(14, 5, args=())}
    # CTX rows carry copy numbers without printing them: they must not count as the flip (the real one is row 9)
    rows = [plain_row(k, flag=CTX if k in (2, 3, 8) else 2, cn=[(0, bits(2.0))] if k in (2, 3, 8, 9) else ()) for k in range(16)]
    t["ctx-rows-with-copy-numbers"] = dict(args=["-h"], rows=rows)
    # -a: the copy numbers are formatted on the side, the stream never turns fixed
    rows = [plain_row(k, flag=CTX if k == 4 else 1 + k % 5, cn=[(k % 3, bits(0.75 + k)), (2, bits(1e-3))] if k % 3 else ()) for k in range(18)]
    t["by-library"] = dict(args=["-a", "-h"], rows=rows)
    # keys outside [0, num_bams) print nothing and leave the stream alone: row 6 is the flip, rows 1-4 are not
    rows = [plain_row(k, cn=[(-1, bits(1.0)), (2, bits(3.0))] if k in (1, 2, 3, 4) else [(5, bits(1.0)), (1, bits(0.5))] if k == 6 else ()) for k in range(15)]
    t["copy-number-keys-out-of-range"] = dict(args=["-h"], rows=rows)
    # the NaN with the sign bit set (and the one without) on both sides of the flip, 40 rows, several flips, -l types
    rows = [plain_row(k, flag=1 + k % 5, af=NAN_NEG if k in (3, 30) else NAN_POS if k in (4, 31) else None,
                      cn=[(1, NAN_NEG)] if k == 17 else [(0, bits(0.125))] if k in (21, 39) else ()) for k in range(40)]
    t["nan-on-both-sides"] = dict(args=["-h", "-l"], rows=rows)
    return t


SYNTHETIC = synthetic_tables()
SLIPS = (">=", "final", "precision")


def syn_kw(table):
    a = table["args"]
    return dict(cfg=SYN_CFG, by_lib="-a" in a, with_af="-h" in a, long_insert="-l" in a, targets=SYN_TARGETS)


def syn_threads(table):
    n = len(table["rows"])
    return sorted({1, 2, 3, 5, max(n, 1), n + 3})


@pytest.mark.parametrize("label", sorted(SYNTHETIC))
def test_synthetic_table_by_any_number_of_threads_is_the_sequential_text(label, tools, tmp_path):
    table = SYNTHETIC[label]
    assert label == "empty" or 8 <= len(table["rows"]) <= 40
    start = [True, 2] if table.get("fixed") else [False, 6]
    (tmp_path / "cfg").write_text(SYN_CONFIG)
    f = tmp_path / "table.txt"
    table_file(f, tmp_path / "cfg", table["args"], SYN_TARGETS, table["rows"])
    want, want_state = table_text(table["rows"], 1, start, **syn_kw(table))
    for threads in syn_threads(table):
        assert table_text(table["rows"], threads, start, **syn_kw(table)) == (want, want_state)      # the rule as written down above ...
        for exe in builds_for(tools, threads):                                                         # ... and as built
            got, got_state = run_tool(exe, f, threads, fixed=bool(table.get("fixed")))
            assert got == want, (exe, threads)
            assert got_state == state_line(want_state), (exe, threads)


@pytest.mark.parametrize("slip", SLIPS)
def test_the_synthetic_tables_tell_each_slip_apart(slip):
    """a slice that starts AT the flip row starting fixed (">="), the stream not left fixed behind the table ("final"), a slice's stream
    starting at six digits whatever the stream it stands in for had ("precision"): each changes some table's text or final state"""
    caught = []
    for label, table in SYNTHETIC.items():
        start = [True, 2] if table.get("fixed") else [False, 6]
        want = table_text(table["rows"], 1, start, **syn_kw(table))
        for threads in syn_threads(table):
            if table_text(table["rows"], threads, start, slip=slip, **syn_kw(table)) != want:
                caught.append((label, threads))
    assert caught, slip
    if slip == ">=":
        assert ("flip-at-k0", 5) in caught and ("flip-at-k0-minus-1", 5) not in caught and ("flip-at-k0-plus-1", 5) not in caught
    if slip == "precision":
        assert {l for l, _ in caught} == {"stream-arrives-fixed", "stream-arrives-fixed-no-copy-number"}


def test_the_oracle_cases_print_rows():
    """(-t finds nothing on one chromosome; every other option set prints rows, with copy numbers and, where asked for, allele frequencies)"""
    counts = {" ".join(CLI_CASES[i][0]): len(oracle_case(i)[1]) for i in range(len(CLI_CASES))}
    assert all(n >= 1 for k, n in counts.items() if k != "-t"), counts


def test_every_allele_frequency_of_the_tables_reads_differently_fixed():
    for x in AFS:
        assert "%.6g" % value(bits(x)) != "%.2f" % value(bits(x))
