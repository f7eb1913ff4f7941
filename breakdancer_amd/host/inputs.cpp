#include "inputs.h"

#include <getopt.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <stdexcept>
#include <thread>

#include "anchor.h"
#include "mini.h"
#include "producer.h"
#include "store_counts.h"

namespace bdhost {

BamConfig open_config(const std::string& path, int cut_sd, std::string* text) {
    std::ifstream in(path.c_str());
    if (!in.is_open()) throw std::runtime_error("unable to open config file '" + path + "'");
    std::stringstream ss;
    ss << in.rdbuf();
    std::istringstream parsed(ss.str());
    if (text) *text = parsed.str();
    return BamConfig(parsed, cut_sd);
}

void FirstHeader::load() const {
    if (loaded_) return;
    read_targets(cfg_, names_, lengths_);
    loaded_ = true;
}

std::unique_ptr<ExcludeTable> open_exclude(const std::string& path, const FirstHeader& header) {
    std::unique_ptr<ExcludeTable> table;
    if (path.empty()) return table;
    table.reset(new ExcludeTable);
    read_exclude_bed(path, header.names(), *table);
    return table;
}

Env read_env() {
    Env e;
    if (const char* g = getenv("BDX_GPUS")) {
        const std::string s(g);
        if (s.empty()) {
        } else if (s.find(',') == std::string::npos) {
            for (int i = 0; i < atoi(g); ++i) e.gpus.push_back(i);
        } else {
            size_t p = 0;
            while (p <= s.size()) {
                const size_t q = s.find(',', p);
                e.gpus.push_back(atoi(s.substr(p, q == std::string::npos ? std::string::npos : q - p).c_str()));
                if (q == std::string::npos) break;
                p = q + 1;
            }
        }
    }
    if (const char* d = getenv("BDX_DECODE")) e.decode_host = !strcmp(d, "host");
    if (const char* t = getenv("BDX_THREADS")) e.threads = std::max(1, atoi(t));
    if (const char* t = getenv("BDX_READ_THREADS")) e.read_threads = std::max(1, atoi(t));
    if (const char* t = getenv("BDX_BATCH_RECORDS")) e.batch_records = (size_t)std::max(1, atoi(t));
    e.timing = getenv("BDX_TIMING") != nullptr;
    if (const char* t = getenv("BDX_TRIM")) e.keep_results = !strcmp(t, "0");
    if (const char* t = getenv("BDX_FORMAT_THREADS")) { e.format_threads_set = true; e.format_threads = atoi(t); }
    e.foreground = getenv("BDX_FOREGROUND") != nullptr;
    e.clean_exit = getenv("BDX_CLEAN_EXIT") != nullptr;
    return e;
}

unsigned usable_cpus() {
    unsigned n = std::max(1u, std::thread::hardware_concurrency());
    if (FILE* f = fopen("/sys/fs/cgroup/cpu.max", "r")) {
        char quota[64] = {0};
        long period = 0;
        if (fscanf(f, "%63s %ld", quota, &period) == 2 && period > 0 && quota[0] != 'm')
            n = std::min<unsigned>(n, (unsigned)std::max(1L, (atol(quota) + period - 1) / period));
        fclose(f);
    } else {
        long q = -1, per = 0;
        if (FILE* g = fopen("/sys/fs/cgroup/cpu/cpu.cfs_quota_us", "r")) { if (fscanf(g, "%ld", &q) != 1) q = -1; fclose(g); }
        if (FILE* g = fopen("/sys/fs/cgroup/cpu/cpu.cfs_period_us", "r")) { if (fscanf(g, "%ld", &per) != 1) per = 0; fclose(g); }
        if (q > 0 && per > 0) n = std::min<unsigned>(n, (unsigned)std::max(1L, (q + per - 1) / per));
    }
    return n;
}

namespace {

// the command line's options, or with -R <cache> those of the run that wrote the cache
Options parse_options(int argc, char** argv, Pass1Cache& cache, bool& restored) {
    Options opts(argc, argv);
    restored = !opts.restore_file.empty();
    if (!restored) return opts;
    cache = read_cache(opts.restore_file);
    std::vector<char*> av;
    for (auto& a : cache.argv) av.push_back(&a[0]);
    optind = 1;
    return Options((int)av.size(), av.data());
}

BamConfig parse_config(bool restored, const Options& opts, const Pass1Cache& cache, std::string& config_text) {
    if (!restored) return open_config(opts.bam_config_path, opts.o.cut_sd, &config_text);
    config_text = cache.config_text;
    std::istringstream in(config_text);
    return BamConfig(in, opts.o.cut_sd);
}

}  // namespace

Inputs::Inputs(int argc, char** argv, const Env& env)
    : opts(parse_options(argc, argv, cache, restored)), cfg(parse_config(restored, opts, cache, config_text)), header(cfg) {
    want_dumps = !opts.prefix_fastq.empty() || !opts.dump_BED.empty();
    if (restored && ((int)cfg.num_libs() != cache.nlibs || (int)cfg.num_bams() != cache.nbams))
        throw std::runtime_error("Failed to load restore file: statistics do not fit its configuration");
    no_bams = cfg.num_bams() == 0;
    if (no_bams) return;
    if (!opts.vcf.empty()) vcf.reset(new VcfWriter(opts.vcf));
    exclude = open_exclude(opts.exclude, header);   // (names are those of the first BAM's header, the one -o is resolved against)
    sites_window = opts.sites_window;
    if (!opts.sites.empty()) {
        sites_vcf.reset(new VcfWriter(opts.sites_vcf));
        std::vector<std::pair<std::string, uint32_t>> type_masks;
        for (const char* t : kSiteTypes) type_masks.emplace_back(t, opts.sv_flag_mask(t));
        read_sites(opts.sites, header.names(), type_masks, site_table);
        if (sites_window < 0) sites_window = cutoff_window(cfg, "--sites");
    }
    ci_window = !opts.ci ? 0 : opts.ci_window >= 0 ? opts.ci_window : cutoff_window(cfg, "--ci");
    mapq_window = !opts.mapq ? 0 : opts.mapq_window >= 0 ? opts.mapq_window : cutoff_window(cfg, "--mapq");
    clip_window = !opts.clip ? 0 : opts.clip_window >= 0 ? opts.clip_window : clip_default_window(cfg);
    // Decode threads: the work is CPU-bound on zlib (~375 MB/s of inflated bytes per core), so what counts is the number of
    // cores this process may really use -- the cgroup's CPU quota when there is one (a container with "16 CPUs" on a
    // 256-thread host: 16 threads 0.64 s, 32 0.55 s, 64 0.70 s for 15 M records), else the hardware threads.  Twice that
    // many threads keep the cores busy across their waits; BDX_THREADS overrides.
    io_threads = env.threads ? (unsigned)env.threads : std::min(std::max(2 * usable_cpus(), 4u), 64u);
    libs = cfg.abi_libs();
    devices = env.gpus;
    sharded = devices.size() > 1 && opts.chr.empty();
    if (!opts.estimate_config.empty()) {
        estimate_config.open(opts.estimate_config.c_str());
        if (!estimate_config.is_open()) throw std::runtime_error("unable to open --estimate-config file '" + opts.estimate_config + "' for writing");
    }
    if (!opts.mini.empty()) {
        mini_out.open(opts.mini.c_str());
        if (!mini_out.is_open()) throw std::runtime_error("unable to open --mini file '" + opts.mini + "' for writing");
        if (opts.mini_window < 0 && !opts.estimate) (void)mini_mean_window(libs);
    }
    if (!opts.anchor.empty()) {
        anchor_out.open(opts.anchor.c_str());
        if (!anchor_out.is_open()) throw std::runtime_error("unable to open --anchor file '" + opts.anchor + "' for writing");
        if (opts.anchor_window < 0 && !opts.estimate) (void)anchor_default_window(libs);
    }
}

void Inputs::apply_estimate(const EstimatePlan& plan) {
    cfg.set_insert_sizes(plan.libs, plan.window);
    libs = cfg.abi_libs();
    if (!opts.sites.empty() && opts.sites_window < 0) sites_window = cutoff_window(cfg, "--sites");
    if (opts.ci && opts.ci_window < 0) ci_window = cutoff_window(cfg, "--ci");
    if (opts.mapq && opts.mapq_window < 0) mapq_window = cutoff_window(cfg, "--mapq");
    if (opts.clip && opts.clip_window < 0) clip_window = clip_default_window(cfg);
    if (estimate_config.is_open()) {
        estimate_config << plan.config_text;
        estimate_config.close();
        if (estimate_config.fail()) throw std::runtime_error("unable to write --estimate-config file '" + opts.estimate_config + "'");
    }
}

}  // namespace bdhost
