// The BAM container as the host reads it, in one place: little-endian words, a mapped file, the BGZF member header
// (RFC 1952 with the BC extra field, SAM specification 4.1), one member through zlib, and the walk of the BAM header to
// the first record (SAM specification 4.2).  Header-only: the readers and the tools include it, no link line changes.
// oracle/bd_oracle_bam.cpp and breakdancer_amd/bamdec.py keep parsers of their own: the tests hold this one against them.
#pragma once
#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>
#include <zlib.h>

#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

namespace bdhost {

inline uint16_t le16(const uint8_t* p) { return (uint16_t)(p[0] | (p[1] << 8)); }
inline uint32_t le32(const uint8_t* p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24); }

// a positive number from the environment (the readers' test knobs), else dflt
inline size_t env_or(const char* name, size_t dflt) {
    const char* v = getenv(name);
    const long long x = v ? atoll(v) : 0;
    return x > 0 ? (size_t)x : dflt;
}

// a file mapped read-only for the object's lifetime (an empty file: data() == nullptr, size() == 0)
class MappedFile {
public:
    explicit MappedFile(const std::string& path, bool advise_sequential = true) {
        const int fd = open(path.c_str(), O_RDONLY);
        if (fd < 0) throw std::runtime_error("Failed to open samfile " + path);
        struct stat st;
        if (fstat(fd, &st) != 0) { close(fd); throw std::runtime_error("Failed to open samfile " + path); }
        size_ = (size_t)st.st_size;
        if (size_) {
            void* m = mmap(nullptr, size_, PROT_READ, MAP_PRIVATE, fd, 0);
            if (m == MAP_FAILED) { close(fd); throw std::runtime_error("Failed to map samfile " + path); }
            data_ = (const uint8_t*)m;
            if (advise_sequential) madvise(m, size_, MADV_SEQUENTIAL);
        }
        close(fd);
    }
    ~MappedFile() { if (data_) munmap((void*)data_, size_); }
    MappedFile(const MappedFile&) = delete;
    MappedFile& operator=(const MappedFile&) = delete;
    const uint8_t* data() const { return data_; }
    size_t size() const { return size_; }

private:
    const uint8_t* data_ = nullptr;
    size_t size_ = 0;
};

enum class BgzfStatus {
    kMember,     // *m describes a whole member
    kEnd,        // avail == 0
    kNeedBytes,  // what is there may open a member, but its header or its end lies behind avail
    kNotBgzf,    // no gzip magic / deflate method / FEXTRA flag
    kNoBsize,    // the extra field holds no BC subfield
    kBadBsize,   // BSIZE is smaller than the member's own header and footer
    kTooLarge,   // ISIZE > 64 KiB
};

struct BgzfMember {      // offsets relative to the member's first byte
    size_t total;        // the whole member: header, payload, CRC-32, ISIZE
    size_t payload_off, payload_len;
    uint32_t ulen;       // ISIZE: what the payload inflates to
};

// The member that starts at p, of which avail bytes may be looked at.  Never reads p[i] for i >= avail, never throws.
inline BgzfStatus bgzf_parse(const uint8_t* p, size_t avail, BgzfMember* m) {
    if (avail == 0) return BgzfStatus::kEnd;
    if (avail < 12) return BgzfStatus::kNeedBytes;
    if (p[0] != 31 || p[1] != 139 || p[2] != 8 || !(p[3] & 4)) return BgzfStatus::kNotBgzf;
    const size_t hdr = (size_t)12 + le16(p + 10);
    if (avail < hdr) return BgzfStatus::kNeedBytes;
    int bsize = -1;
    for (size_t x = 12; x + 4 <= hdr;) {
        const size_t slen = le16(p + x + 2);
        if (x + 4 + slen > hdr) break;  // (a subfield that runs out of the extra field does not count)
        if (p[x] == 'B' && p[x + 1] == 'C' && slen == 2) bsize = le16(p + x + 4);
        x += 4 + slen;
    }
    if (bsize < 0) return BgzfStatus::kNoBsize;
    m->total = (size_t)bsize + 1;
    if (m->total < hdr + 8) return BgzfStatus::kBadBsize;
    if (avail < m->total) return BgzfStatus::kNeedBytes;
    m->payload_off = hdr;
    m->payload_len = m->total - hdr - 8;
    m->ulen = le32(p + m->total - 4);
    return m->ulen > 65536 ? BgzfStatus::kTooLarge : BgzfStatus::kMember;
}

// the error a reader reports for a status that is neither a member nor the end
[[noreturn]] inline void bgzf_throw(BgzfStatus s, const std::string& path) {
    switch (s) {
        case BgzfStatus::kNotBgzf: throw std::runtime_error("not a BGZF file: " + path);
        case BgzfStatus::kNoBsize: throw std::runtime_error("BGZF block without BC field: " + path);
        case BgzfStatus::kTooLarge: throw std::runtime_error("BGZF block larger than 64 KiB: " + path);
        default: throw std::runtime_error("truncated BGZF file: " + path);
    }
}

// the member at offset off of a whole file image; false at the end of the file
inline bool bgzf_member_at(const uint8_t* map, size_t size, size_t off, const std::string& path, BgzfMember* m) {
    if (off >= size) return false;
    const BgzfStatus s = bgzf_parse(map + off, size - off, m);
    if (s != BgzfStatus::kMember) bgzf_throw(s, path);
    return true;
}

// one member's payload (raw deflate) through zlib; false unless it inflates to exactly ulen bytes
inline bool bgzf_try_inflate_zlib(const uint8_t* payload, size_t clen, uint8_t* dst, size_t ulen) {
    z_stream zs;
    memset(&zs, 0, sizeof(zs));
    if (inflateInit2(&zs, -15) != Z_OK) return false;
    zs.next_in = const_cast<Bytef*>(payload);
    zs.avail_in = (uInt)clen;
    zs.next_out = dst;
    zs.avail_out = (uInt)ulen;
    const int rc = inflate(&zs, Z_FINISH);
    inflateEnd(&zs);
    return rc == Z_STREAM_END && zs.avail_out == 0;
}

inline void bgzf_inflate_zlib(const uint8_t* payload, size_t clen, uint8_t* dst, size_t ulen, const std::string& path) {
    if (!bgzf_try_inflate_zlib(payload, clen, dst, ulen)) throw std::runtime_error("corrupt BGZF block in " + path);
}

struct BamHeader {
    std::string text;                      // the SAM header (@HD/@SQ/@RG ... lines)
    std::vector<std::string> target_names;
    std::vector<uint32_t> target_lengths;
    size_t first_member_offset = 0;        // file offset of the member that holds the first record
    uint64_t first_record_offset = 0;      // the record's offset in that member's inflated bytes
};

// Magic, SAM text and reference names, inflated member by member with zlib (a header is a few members).  If the header
// ends a member, the first record opens the next one: that member's offset -- the file's size if none follows -- and 0.
inline BamHeader read_bam_header(const uint8_t* map, size_t size, const std::string& path) {
    BamHeader out;
    std::vector<uint8_t> h;
    std::vector<std::pair<size_t, size_t>> starts;  // (file offset, inflated offset) of every member read so far
    size_t off = 0;
    auto need = [&](size_t n) {
        while (h.size() < n) {
            BgzfMember m;
            if (!bgzf_member_at(map, size, off, path, &m)) throw std::runtime_error(path + " is not a valid bam file");
            starts.emplace_back(off, h.size());
            const size_t at = h.size();
            h.resize(at + m.ulen);
            if (m.ulen) bgzf_inflate_zlib(map + off + m.payload_off, m.payload_len, h.data() + at, m.ulen, path);
            off += m.total;
        }
    };
    need(12);
    if (memcmp(h.data(), "BAM\1", 4) != 0) throw std::runtime_error(path + " is not a valid bam file");
    const uint32_t l_text = le32(h.data() + 4);
    size_t p = 8 + (size_t)l_text;
    need(p + 4);
    out.text.assign((const char*)h.data() + 8, l_text);
    const uint32_t n_ref = le32(h.data() + p);
    p += 4;
    for (uint32_t i = 0; i < n_ref; ++i) {
        need(p + 4);
        const uint32_t l = le32(h.data() + p);
        need(p + 4 + (size_t)l + 4);
        out.target_names.emplace_back((const char*)h.data() + p + 4, l ? l - 1 : 0);
        out.target_lengths.push_back(le32(h.data() + p + 4 + (size_t)l));
        p += 4 + (size_t)l + 4;
    }
    size_t k = starts.size();
    while (k > 0 && starts[k - 1].second > p) --k;
    if (k > 0 && p < h.size()) {
        out.first_member_offset = starts[k - 1].first;
        out.first_record_offset = p - starts[k - 1].second;
    } else {
        out.first_member_offset = off;
    }
    return out;
}

}  // namespace bdhost
