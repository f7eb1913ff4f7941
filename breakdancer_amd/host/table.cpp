#include "table.h"

#include <iomanip>
#include <map>
#include <sstream>
#include <thread>

namespace bdhost {

namespace {

const int kPrintedFlagValue[BDX_NUM_FLAGS] = {0, 1, 2, 3, 4, 8, 18, 20, 32, 64, 192};  // common/ReadFlags.cpp:4-14

std::string base_name(const std::string& path) {
    const size_t p = path.rfind("/");
    return p != std::string::npos ? path.substr(p + 1) : path;
}

}  // namespace

std::vector<std::string> sample_names(const Options& opts, const BamConfig& cfg) {
    std::vector<std::string> samples;
    if (opts.o.cn_lib)
        for (size_t i = 0; i < cfg.num_libs(); ++i) samples.push_back(cfg.library_config(i).name);
    else
        for (auto const& b : cfg.bam_files()) samples.push_back(base_name(b));
    return samples;
}

void TableFormat::header(std::ostream& os, const TableCounters& c) const {
    os << "#Software: breakdancer-max-mi355x (libbdx)" << std::endl;
    os << "#Command: ";
    for (auto const& a : opts_.orig_argv) os << a << " ";
    os << std::endl;
    os << "#Library Statistics:" << std::endl;
    const uint32_t covered = c.covered_ref_len;
    for (size_t i = 0; i < cfg_.num_libs(); ++i) {  // BreakDancerMax.cpp:83-137
        const LibraryConfig& lc = cfg_.library_config(i);
        const float physical_coverage = float(c.lib_count[i] * lc.mean_insertsize) / covered / 2;
        os << "#" << lc.bam_file << "\tmean:" << lc.mean_insertsize << "\tstd:" << lc.std_insertsize
           << "\tuppercutoff:" << lc.uppercutoff << "\tlowercutoff:" << lc.lowercutoff << "\treadlen:" << lc.readlens
           << "\tlibrary:" << lc.name << "\treflen:" << covered << "\tseqcov:" << c.seqcov[i] << "\tphycov:" << physical_coverage;
        for (int f = 0; f < BDX_NUM_FLAGS; ++f) {
            const uint32_t n = c.flag_hist[i * BDX_NUM_FLAGS + f];
            if (n) os << "\t" << kPrintedFlagValue[f] << ":" << n;
        }
        os << "\n";
    }
    os << "#Chr1\tPos1\tOrientation1\tChr2\tPos2\tOrientation2\tType\tSize\tScore\tnum_Reads\tnum_Reads_lib";
    if (opts_.o.print_af) os << "\tAllele_frequency";
    if (!opts_.o.cn_lib)
        for (auto const& name : sample_names(opts_, cfg_)) os << "\t" << name;
    os << "\n";
}

void TableFormat::row(std::ostream& os, const bdx_sv& s, const SvLists& l) const {
    std::map<int, float> cn;  // key -> copy number
    for (int i = 0; i < s.cn_count; ++i) cn[l.cn_key[s.cn_begin + i]] = l.cn_value[s.cn_begin + i];
    std::string sptype;
    if (opts_.o.cn_lib) {
        for (int i = 0; i < s.lib_count; ++i) {
            const int lib = l.lib_index[s.lib_begin + i];
            std::string cn_str = "NA";
            if (s.flag != BDX_ARP_CTX) {
                auto f = cn.find(lib);
                if (f != cn.end()) {
                    std::stringstream ss;
                    ss << std::fixed << std::setprecision(2) << f->second;
                    cn_str = ss.str();
                }
            }
            if (!sptype.empty()) sptype += ":";
            sptype += cfg_.library_config(lib).name + "|" + std::to_string(l.lib_pairs[s.lib_begin + i]) + "," + cn_str;
        }
    } else {
        std::map<std::string, int> bam_rc;
        for (int i = 0; i < s.lib_count; ++i) bam_rc[cfg_.library_config(l.lib_index[s.lib_begin + i]).bam_file] += l.lib_pairs[s.lib_begin + i];
        for (auto const& kv : bam_rc) {
            if (!sptype.empty()) sptype += ":";
            sptype += kv.first + "|" + std::to_string(kv.second);
        }
        if (sptype.empty()) sptype = "NA";
    }
    os << target_name(s.chr[0]) << "\t" << s.pos[0] << "\t" << s.fwd[0] << "+" << s.rev[0] << "-"
       << "\t" << target_name(s.chr[1]) << "\t" << s.pos[1] << "\t" << s.fwd[1] << "+" << s.rev[1] << "-"
       << "\t" << opts_.sv_type(s.flag) << "\t" << s.size << "\t" << s.score << "\t" << s.num_reads << "\t" << sptype;
    if (opts_.o.print_af) os << "\t" << s.allele_frequency;
    if (!opts_.o.cn_lib && s.flag != BDX_ARP_CTX) {
        for (size_t b = 0; b < cfg_.num_bams(); ++b) {
            auto f = cn.find((int)b);
            if (f == cn.end()) os << "\tNA";
            else {
                // the reference never resets these manipulators on cout: later allele frequencies print
                // fixed with two decimals as well (BreakDancer.cpp:492-493)
                os << "\t";
                os << std::fixed;
                os << std::setprecision(2) << f->second;
            }
        }
    }
    os << "\n";
}

bool TableFormat::sets_fixed(const bdx_sv& s, const SvLists& l) const {
    if (opts_.o.cn_lib || s.flag == BDX_ARP_CTX) return false;
    for (int i = 0; i < s.cn_count; ++i)
        if (l.cn_key[s.cn_begin + i] >= 0 && (size_t)l.cn_key[s.cn_begin + i] < cfg_.num_bams()) return true;
    return false;
}

// A large table (a genome's: tens of thousands of rows, 0.7 us each through the stream's formatting) is written by several threads,
// each into its own string stream that starts in the state the sequential loop would have reached at its first row; the strings
// leave in order.
void TableFormat::write_rows(std::ostream& os, const std::vector<bdx_sv>& svs, const std::vector<size_t>& printed_rows, const SvLists& l, size_t threads) const {
    if (threads <= 1) {
        for (size_t r : printed_rows) row(os, svs[r], l);
        return;
    }
    os.flush();
    const size_t none = (size_t)-1;
    size_t flip_row = none;   // the first printed row that leaves the stream printing fixed (the rows behind it start that way)
    const bool fixed_already = (os.flags() & std::ios_base::fixed) != 0;
    for (size_t k = 0; k < printed_rows.size() && !fixed_already; ++k)
        if (sets_fixed(svs[printed_rows[k]], l)) { flip_row = k; break; }
    std::vector<std::string> parts(threads);
    std::vector<std::thread> workers;
    for (size_t t = 0; t < threads; ++t)
        workers.emplace_back([&, t] {
            const size_t k0 = printed_rows.size() * t / threads, k1 = printed_rows.size() * (t + 1) / threads;
            std::ostringstream part;
            part.flags(os.flags());
            part.precision(os.precision());
            if (flip_row != none && k0 > flip_row) { part << std::fixed; part << std::setprecision(2); }
            for (size_t k = k0; k < k1; ++k) row(part, svs[printed_rows[k]], l);
            parts[t] = part.str();
        });
    for (auto& w : workers) w.join();
    for (auto const& part : parts) os.write(part.data(), (std::streamsize)part.size());
    if (flip_row != none) { os << std::fixed; os << std::setprecision(2); }
}

}  // namespace bdhost
