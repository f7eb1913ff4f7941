// bdx-table-check: the table formatter (table.cpp) on its own, for tests/test_table.py -- no GPU and no libbdx.
//   bdx-table-check FILE THREADS [fixed]
// writes the rows FILE describes with TableFormat::write_rows on THREADS threads (`fixed`: the stream arrives printing fixed with two
// decimals, as behind an earlier table), then one line "#state <fixed 0|1> <precision>" with what the stream was left in.  FILE:
//   config PATH                 the bam2cfg configuration
//   args OPTION...              the command line's options (the configuration path is appended)
//   targets NAME...             sequence names of the first BAM
//   sv chr0 pos0 fwd0 rev0 chr1 pos1 fwd1 rev1 flag size score num_reads AF nlib ncn (lib pairs)*nlib (key CN)*ncn
// one `sv` line per row; AF and CN are floats as hex bit patterns (a NaN keeps its sign).
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iomanip>
#include <iostream>
#include <sstream>
#include <stdexcept>

#include "config.h"
#include "options.h"
#include "table.h"

// (options.cpp asks libbdx for the numeric defaults; the table reads none of them, only the -a, -h and -l flags)
void bdx_opts_default(bdx_opts* o) { memset(o, 0, sizeof *o); }

namespace {

float float_of_bits(const std::string& hex) {
    const uint32_t bits = (uint32_t)strtoul(hex.c_str(), nullptr, 16);
    float f;
    memcpy(&f, &bits, sizeof f);
    return f;
}

}  // namespace

int main(int argc, char** argv) {
    try {
        if (argc < 3) throw std::runtime_error("usage: bdx-table-check FILE THREADS [fixed]");
        std::ifstream file(argv[1]);
        if (!file.is_open()) throw std::runtime_error(std::string("unable to open '") + argv[1] + "'");
        std::string config_path, line, word;
        std::vector<std::string> args{"bdx-table-check"}, targets;
        std::vector<bdx_sv> svs;
        bdhost::SvLists lists;
        while (std::getline(file, line)) {
            std::istringstream in(line);
            if (!(in >> word)) continue;
            if (word == "config") in >> config_path;
            else if (word == "args") { while (in >> word) args.push_back(word); }
            else if (word == "targets") { while (in >> word) targets.push_back(word); }
            else if (word == "sv") {
                bdx_sv s{};
                std::string af;
                in >> s.chr[0] >> s.pos[0] >> s.fwd[0] >> s.rev[0] >> s.chr[1] >> s.pos[1] >> s.fwd[1] >> s.rev[1] >> s.flag >> s.size >> s.score >> s.num_reads >> af
                   >> s.lib_count >> s.cn_count;
                s.allele_frequency = float_of_bits(af);
                s.printed = 1;
                s.lib_begin = (int32_t)lists.lib_index.size();
                s.cn_begin = (int32_t)lists.cn_key.size();
                for (int i = 0; i < s.lib_count; ++i) {
                    int32_t lib = 0, pairs = 0;
                    in >> lib >> pairs;
                    lists.lib_index.push_back(lib); lists.lib_pairs.push_back(pairs);
                }
                for (int i = 0; i < s.cn_count; ++i) {
                    int32_t key = 0;
                    std::string cn;
                    in >> key >> cn;
                    lists.cn_key.push_back(key); lists.cn_value.push_back(float_of_bits(cn));
                }
                if (!in) throw std::runtime_error("malformed sv line: " + line);
                svs.push_back(s);
            } else throw std::runtime_error("unknown line: " + line);
        }
        args.push_back(config_path);
        std::vector<char*> av;
        for (auto& a : args) av.push_back(&a[0]);
        const bdhost::Options opts((int)av.size(), av.data());
        std::ifstream cfg_stream(config_path.c_str());
        if (!cfg_stream.is_open()) throw std::runtime_error("unable to open config file '" + config_path + "'");
        const bdhost::BamConfig cfg(cfg_stream, opts.o.cut_sd);
        std::vector<size_t> rows(svs.size());
        for (size_t i = 0; i < rows.size(); ++i) rows[i] = i;
        if (argc > 3 && !strcmp(argv[3], "fixed")) std::cout << std::fixed << std::setprecision(2);
        const bdhost::TableFormat table(opts, cfg, targets);
        table.write_rows(std::cout, svs, rows, lists, (size_t)std::max(1, atoi(argv[2])));
        const bool fixed = (std::cout.flags() & std::ios_base::fixed) != 0;
        std::cout << "#state " << (fixed ? 1 : 0) << " " << std::cout.precision() << "\n";
    } catch (std::exception const& e) {
        std::cerr << "ERROR: " << e.what() << "\n";
        return 1;
    }
    return 0;
}
