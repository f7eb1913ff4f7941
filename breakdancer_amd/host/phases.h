// The phases of one breakdancer-max run behind its inputs (inputs.h), in the order main.cpp's run() calls them, and the one owner of
// what the run holds on the GPU.  Each phase sees its inputs by const reference (but see --estimate below) and returns what it produced by value.
#pragma once
#include <chrono>
#include <future>
#include <memory>
#include <string>
#include <thread>
#include <vector>

#include "bdx.h"
#include "dumps.h"
#include "inputs.h"
#include "producer.h"
#include "table.h"
#include "vcf.h"

namespace bdhost {

using Clock = std::chrono::steady_clock;
inline double secs(Clock::time_point a, Clock::time_point b) { return std::chrono::duration<double>(b - a).count(); }

// What the run holds on the GPU: the single context (created on a helper thread) or the ranks of a sharded run, and the thread that
// hands the pinned result tables back while the table is printed.  The destructor is the only teardown, and its order is the one
// the pieces need: the pending bdx_create has returned and the trimmer has left the context before anything is destroyed; the kept
// device decoders go before their sink (a decoder borrows its context's streams); a sharded run's result context belongs to rank 0
// and goes with the ranks.  Only _exit may skip it.
struct Session {
    bdx_ctx* ctx = nullptr;            // the single context, or a sharded run's result context (rank 0's)
    std::vector<bdx_dist*> ranks;      // a sharded run's ranks (empty: ctx is owned here)
    std::future<int> ctx_ready;        // the bdx_create in flight
    std::thread trimmer;

    Session() = default;
    Session(const Session&) = delete;
    Session& operator=(const Session&) = delete;
    ~Session();
    void start_trimmer();              // (must not run beside another call on the context)
};

// what feeding and running produced, on either route
struct Fed {
    size_t n_reads = 0;
    std::vector<std::string> targets;  // the first file's sequence names
    std::vector<int> rank_of;          // (sharded runs) chromosome -> rank
    bool device_decoded = false;       // BGZF inflate and record decode ran on the GPU
    Clock::time_point t_decoded, t_ran;
};
// (--estimate: between "fed" and "run" the histograms of the store are taken -- every rank's summed on the host --, the libraries estimated,
// in.apply_estimate called and the contexts given the run's libraries: bdx_set_libs / bdx_dist_set_libs.  The only phases that change `in`)
Fed feed_and_run_single(Inputs& in, const Env& env, Session& s, Clock::time_point t_start);
Fed feed_and_run_sharded(Inputs& in, const Env& env, Session& s, Clock::time_point t_start);

struct Statistics {
    bdx_summary sum{};
    TableCounters counters;
    uint64_t dup_marked = 0, dup_groups = 0;   // --mark-dup: over all ranks
};
Statistics fetch_statistics(const Inputs& in, const Session& s);
// -C <cache>: what a later "-R <cache>" run needs (ConfigLoader.cpp:34-42)
void write_pass1_cache(const Inputs& in, const Statistics& st);

struct Calls {
    std::vector<bdx_sv> svs;
    SvLists lists;
    std::vector<size_t> printed_rows;  // indices into svs of the rows the table prints
};
Calls fetch_calls(const Session& s, size_t n_svs);

// --vcf / --sites / --ci / --depth / --mapq: the counts over the records the run holds
struct Genotypes {
    std::vector<VcfRecord> vcf_rows, site_rows;
};
Genotypes count_on_store(const Inputs& in, const Env& env, const Session& s, const Fed& fed, const Calls& calls);

// --mini: the windowed insert-size tests over the records the run holds, written to the file the inputs opened (mini.h).  Like
// count_on_store it runs before the trimmer starts
void call_mini(Inputs& in, const Env& env, const Session& s, const Fed& fed);

// --anchor: the windowed split of the one-end-anchored reads the run holds, written to the file the inputs opened (anchor.h).  Behind
// call_mini, before the trimmer starts
void call_anchor(Inputs& in, const Env& env, const Session& s, const Fed& fed);

// -g / -d: the supporting reads of the printed SVs and the opened dump files
struct Support {
    std::vector<uint32_t> off;
    std::vector<uint64_t> idx, wanted;
    std::vector<uint8_t> flag;
    std::vector<SupportRead> reads;
    std::unique_ptr<BedDump> bed;
    std::unique_ptr<FastqDump> fastq;
};
Support fetch_support(const Inputs& in, const Session& s, const Fed& fed, const Calls& calls);

void write_table(const Inputs& in, const Env& env, const TableFormat& table, const Calls& calls, Support& sup);
void write_vcfs(const Inputs& in, Genotypes& gt);
void print_timing(const Inputs& in, const Session& s, const Fed& fed, const Statistics& st, Clock::time_point t_start);

}  // namespace bdhost
