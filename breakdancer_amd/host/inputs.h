// What a run is given, settled before the GPU is touched: the BDX_* environment knobs, the options (or the -R cache's), the
// configuration, and the opened or parsed option inputs (--vcf, --exclude, --sites, --ci, --mapq, --estimate-config, --mini, --anchor).  bdx-dump-reads shares the two helpers.
#pragma once
#include <cstdint>
#include <fstream>
#include <memory>
#include <string>
#include <vector>

#include "bdx.h"
#include "cache.h"
#include "config.h"
#include "estimate.h"
#include "exclude.h"
#include "options.h"
#include "sites.h"
#include "vcf.h"

namespace bdhost {

// the configuration file at `path`; text (may be null) receives its contents, which the -C cache keeps
BamConfig open_config(const std::string& path, int cut_sd, std::string* text = nullptr);

// Reference sequences of the first BAM of the configuration, the one -o, --exclude and --sites are resolved against.  The header is
// parsed when first asked for and once only: a run that needs no names opens no file here.
class FirstHeader {
public:
    explicit FirstHeader(const BamConfig& cfg) : cfg_(cfg) {}
    const std::vector<std::string>& names() const { load(); return names_; }
    const std::vector<uint32_t>& lengths() const { load(); return lengths_; }

private:
    void load() const;
    const BamConfig& cfg_;
    mutable bool loaded_ = false;
    mutable std::vector<std::string> names_;
    mutable std::vector<uint32_t> lengths_;
};

// --exclude: the BED file at `path` ("": none, an empty pointer) -- a malformed line fails with FILE:LINE
std::unique_ptr<ExcludeTable> open_exclude(const std::string& path, const FirstHeader& header);

// Every BDX_* knob of the command, read once (README.md's table).
struct Env {
    std::vector<int> gpus;       // BDX_GPUS: "4" -> devices 0,1,2,3; "0,2,5" -> that list (a device may repeat: several ranks then share it)
    bool decode_host = false;    // BDX_DECODE=host
    int threads = 0;             // BDX_THREADS (0: not set)
    int read_threads = 0;        // BDX_READ_THREADS (0: not set)
    bool timing = false;         // BDX_TIMING
    bool keep_results = false;   // BDX_TRIM=0
    bool format_threads_set = false;
    int format_threads = 0;      // BDX_FORMAT_THREADS
    bool foreground = false;     // BDX_FOREGROUND
    bool clean_exit = false;     // BDX_CLEAN_EXIT
    size_t batch_records = 0;    // BDX_BATCH_RECORDS: records per batch of the host producer (0: its default, 2^20; tests force several batches)
};
Env read_env();

struct Inputs {
    // Fails in this order, each before the GPU is touched: option parsing, -R / config, (no BAM files: see no_bams), --vcf open, --exclude
    // parse, --sites-vcf open and --sites parse, --ci window, --mapq window, --estimate-config open, --mini open and window, --anchor open and window.
    Inputs(int argc, char** argv, const Env& env);
    Inputs(const Inputs&) = delete;
    Inputs& operator=(const Inputs&) = delete;

    Pass1Cache cache;            // -R <cache>: options, configuration and pass-1 statistics of the run that wrote the cache (ConfigLoader.cpp:19-23)
    bool restored = false;
    Options opts;
    std::string config_text;
    BamConfig cfg;
    FirstHeader header;
    bool no_bams = false;        // the configuration names no BAM file: nothing below was opened or parsed
    bool want_dumps = false;     // -g / -d
    std::unique_ptr<VcfWriter> vcf;            // --vcf: opened at once -- an unwritable path fails here
    std::unique_ptr<ExcludeTable> exclude;     // --exclude
    std::unique_ptr<VcfWriter> sites_vcf;      // --sites-vcf, --sites: likewise opened and parsed here
    SiteTable site_table;
    int32_t sites_window = 0;
    int32_t ci_window = 0;       // --ci: without a finite cutoff the run ends here
    int32_t mapq_window = 0;     // --mapq: likewise
    int32_t clip_window = 0;     // --clip: the largest finite cutoff, at most BDX_CLIP_WINDOW_MAX (that without a finite cutoff)
    unsigned io_threads = 0;     // decode threads of the host producer
    std::vector<bdx_lib> libs;
    std::vector<int> devices;    // BDX_GPUS
    bool sharded = false;        // ONE whole-genome run with the chromosomes spread over several GPUs
    std::ofstream estimate_config;   // --estimate-config: opened at once -- an unwritable path fails here

    std::ofstream mini_out;          // --mini: opened at once -- an unwritable path fails here; without --mini-window (and without --estimate,
                                     // which brings means of its own) a configuration with no finite positive mean insert size fails here too

    std::ofstream anchor_out;        // --anchor: opened at once, likewise; without --anchor-window (and without --estimate, which brings cutoffs of
                                     // its own) a configuration with no finite positive uppercutoff fails here too

    // --estimate, the one change a run makes to its inputs (between "fed" and "run"): the estimated values replace the configuration's in
    // cfg and libs, so that everything behind the feed prints and uses the run's libraries; the windows of --sites / --ci / --mapq / --clip that
    // the command line did not give are computed again from them; --estimate-config is written and closed
    void apply_estimate(const EstimatePlan& plan);
};

// CPUs this process can use: hardware threads, capped by the cgroup v2 / v1 CPU quota if one is set
unsigned usable_cpus();

}  // namespace bdhost
