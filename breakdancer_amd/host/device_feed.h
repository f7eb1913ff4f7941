// One file of the configuration through a device-side decoder (bdx_bamdec_*, include/bdx.h): this side reads the file into the
// decoder's pinned staging buffers (several threads), finds the BGZF members and submits them.  The sizes the decoder is created
// with and the cut into members are feed_plan.h's; producer.cpp's device routes are the callers.
#pragma once
#include <cstdint>
#include <memory>
#include <string>
#include <vector>

#include "bdx.h"
#include "config.h"
#include "exclude.h"

namespace bdhost {

// Decoders that have done their work.  Releasing one (a 3 GiB ring, four batches' buffers, pinned staging, streams) takes the
// driver tens of milliseconds, and the clustering run does not need the memory back: they are kept until
// release_device_decoders(), which the CLI calls only when it walks its destructors.
void retire(bdx_bamdec* d);
struct RetireDecoder { void operator()(bdx_bamdec* d) const { retire(d); } };
using OwnedDecoder = std::unique_ptr<bdx_bamdec, RetireDecoder>;   // whoever holds one lets go of it by retiring it

struct DecodeJob {
    const BamConfig& cfg;
    size_t bam_index = 0;
    // what of the file: a -o region in samtools syntax (empty: everything), or -- sharded runs, whole_tid >= 0 -- ALL records of that
    // sequence through the index, which must be there; span_bytes: what the sequence takes of the file (sizes the decoder's buffers
    // and the sink's store instead of "the rest of the file")
    std::string region;
    int whole_tid = -1;
    size_t span_bytes = 0;
    const ExcludeTable* exclude = nullptr;   // --exclude, handed to a new decoder (it keeps it when it is armed again)
    int threads = 1;                         // readers of the file
    int device = 0;
    // With a sink the records go into its store (and are classified as they arrive); without, they stay in the decoder's own columns
    // for the merge (bdx_merge_decoded / bdx_append_decoded).
    bdx_ctx* sink = nullptr;
    // sharded runs: a finished decoder of the same file and sink, armed again (bdx_bamdec_rearm) instead of a new one being set up;
    // sized_for: the largest span the decoder -- new or armed again -- will be used for (its buffers are sized once)
    bdx_bamdec* rearm = nullptr;
    size_t sized_for = 0;
    bool clips = false;                          // a decoder without a sink keeps the records' clip words (its gather target has bdx_use_clips on)
    bool may_be_unsupported = false;             // the caller can take `unsupported` for an answer (else it is an exception)
    std::vector<std::string>* targets = nullptr; // receives the file's sequence names
};

struct DecodeResult {
    size_t n = 0;               // records (with a sink: what its store holds now)
    uint64_t excluded = 0;      // records the --exclude table dropped
    bool unsupported = false;   // a stretch the device path leaves to the host reader; nothing counts
    OwnedDecoder decoder;       // the decoder this call set up; null when job.rearm was used: that one stays its holder's
};

DecodeResult decode_on_device(const DecodeJob& job);

}  // namespace bdhost
