// bdx-clip-store: the clip column as a breakdancer-max run with --clip leaves it in the store(s), for tests (tests/test_gpu_clip.py).
// Same command line and environment as breakdancer-max (--clip and a --vcf / --sites-vcf file are required as there; BDX_DECODE, BDX_GPUS,
// BDX_BATCH_RECORDS choose the route exactly as there): the inputs are opened and the reads fed and run by the CLI's own phases
// (phases.cpp feed_and_run_single / feed_and_run_sharded), then every context's column is read back with bdx_get_clips and printed:
//   #route device|host
//   #rank_of r0 r1 ...            (a sharded run: the rank of every sequence)
//   #context k n                  then n lines, one clip word each, in store order; k = 0 for the single context, else the rank
// Needs a GPU.
#include <cstdio>
#include <iostream>
#include <stdexcept>
#include <vector>

#include "bdx.h"
#include "inputs.h"
#include "phases.h"

using namespace bdhost;

namespace {

// bdx_get_clips hands out min(cap, records held) words and does not say how many: two reads over buffers filled with different values
// agree exactly on the rows that were written
std::vector<uint32_t> column_of(bdx_ctx* c, size_t cap) {
    std::vector<uint32_t> a(cap, 0xFFFFFFFFu), b(cap, 0xFFFFFFFEu);
    int rc = bdx_get_clips(c, a.data(), cap);
    if (rc == BDX_ESTATE) return {};   // (a rank that got no reads never switched its column on)
    if (rc == BDX_OK) rc = bdx_get_clips(c, b.data(), cap);
    if (rc != BDX_OK) throw std::runtime_error(std::string("bdx_get_clips: ") + bdx_strerror(rc) + " (" + bdx_last_error(c) + ")");
    size_t n = 0;
    while (n < cap && a[n] == b[n]) ++n;
    a.resize(n);
    return a;
}

void print_context(int k, const std::vector<uint32_t>& w) {
    printf("#context %d %zu\n", k, w.size());
    for (uint32_t x : w) printf("%u\n", x);
}

}  // namespace

int main(int argc, char** argv) {
    const Env env = read_env();
    Session s;
    try {
        Inputs in(argc, argv, env);
        if (in.no_bams || !in.opts.clip) throw std::runtime_error("a configuration with BAM files and --clip are needed");
        const Fed fed = in.sharded ? feed_and_run_sharded(in, env, s, Clock::now()) : feed_and_run_single(in, env, s, Clock::now());
        printf("#route %s\n", fed.device_decoded ? "device" : "host");
        if (in.sharded) {
            printf("#rank_of");
            for (int r : fed.rank_of) printf(" %d", r);
            printf("\n");
            for (size_t r = 0; r < s.ranks.size(); ++r) {
                bdx_ctx* c = bdx_dist_chromosome(s.ranks[r], (int)fed.rank_of.size() - 1);   // (the rank's one context, as store_counts.cpp asks for it)
                if (!c) throw std::runtime_error(std::string("bdx_dist_chromosome: ") + bdx_dist_last_error(s.ranks[r]));
                print_context((int)r, column_of(c, fed.n_reads + 1));
            }
        } else {
            print_context(0, column_of(s.ctx, fed.n_reads + 1));
        }
    } catch (std::exception const& e) {
        std::cerr << "ERROR: " << e.what() << "\n";
        return 1;
    }
    return 0;
}
