// The clip word of a record: what its CIGAR says about soft / hard clips at its two ends and about the reference bases it covers, in
// 32 bits (the rule in words: include/bdx.h, bdx_clip_word).  One function for every reader -- the device decode (kb_records.hip), the
// host reader (host/bam_reader.cpp) and the exported bdx_clip_word -- so that the column is the same whichever route filled it.
//
//   word = left | right << 8 | span << 16
//
// The CIGAR is read through clip_ld32, byte by byte: inside a BAM record it is not aligned.
#pragma once
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define BDX_CLIP_HD __host__ __device__
#else
#define BDX_CLIP_HD
#endif

namespace bdx {

constexpr uint32_t kClipLenMax = 255;       // left / right saturate here
constexpr uint32_t kClipSpanCap = 65535;    // span saturates here

BDX_CLIP_HD inline uint32_t clip_ld32(const uint8_t* p) {
    return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
}
BDX_CLIP_HD inline bool clip_is_clip(uint32_t op) { return op == 4 || op == 5; }   // S, H
BDX_CLIP_HD inline bool clip_takes_reference(uint32_t op) { return op == 0 || op == 2 || op == 3 || op == 7 || op == 8; }   // M D N = X (bam_calend)

// cigar: n_cigar little-endian words (len << 4 | op), any alignment; the caller has checked that 4 n_cigar bytes are there
BDX_CLIP_HD inline uint32_t clip_word(const uint8_t* cigar, uint32_t n_cigar, int32_t l_seq, uint32_t flag) {
    if (n_cigar == 0 || (flag & 0x4u)) return 0;
    if (n_cigar == 2) {   // htslib's placeholder of a CIGAR too long for the field: <l_seq>S<n>N, the real one is in the CG tag
        const uint32_t a = clip_ld32(cigar), b = clip_ld32(cigar + 4);
        if ((a & 15) == 4 && l_seq >= 0 && (a >> 4) == (uint32_t)l_seq && (b & 15) == 3) return 0;
    }
    uint64_t left = 0, span = 0;
    uint32_t lead = 0;   // operations of the leading run
    while (lead < n_cigar) {
        const uint32_t w = clip_ld32(cigar + 4 * (uint64_t)lead);
        if (!clip_is_clip(w & 15)) break;
        left += w >> 4;
        ++lead;
    }
    for (uint32_t k = lead; k < n_cigar; ++k) {
        const uint32_t w = clip_ld32(cigar + 4 * (uint64_t)k);
        if (clip_takes_reference(w & 15)) span += w >> 4;
    }
    uint64_t right = 0;   // the trailing run, only behind some other operation: a CIGAR of clips alone has none
    for (uint32_t k = n_cigar; k > lead; --k) {
        const uint32_t w = clip_ld32(cigar + 4 * (uint64_t)(k - 1));
        if (!clip_is_clip(w & 15)) break;
        right += w >> 4;
    }
    if (span > kClipSpanCap) { span = kClipSpanCap; right = 0; }   // (where the right clip stands is unknown then)
    const uint32_t l = left > kClipLenMax ? kClipLenMax : (uint32_t)left, r = right > kClipLenMax ? kClipLenMax : (uint32_t)right;
    return l | (r << 8) | ((uint32_t)span << 16);
}

}  // namespace bdx
