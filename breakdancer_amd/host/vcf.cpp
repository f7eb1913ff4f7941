#include "vcf.h"

#include <algorithm>
#include <cmath>
#include <stdexcept>

namespace bdhost {

Genotype call_genotype(int64_t dr, int64_t dv) {
    Genotype g;
    if (dr < 0 || dv < 0 || dr + dv == 0) return g;
    static const double kAltP[3] = {0.01, 0.5, 0.99};
    double l[3], best = -INFINITY;
    for (int i = 0; i < 3; ++i) {
        l[i] = (double)dv * std::log10(kAltP[i]) + (double)dr * std::log10(1.0 - kAltP[i]);
        best = std::max(best, l[i]);
    }
    for (int i = 0; i < 3; ++i) g.pl[i] = (int64_t)std::round(-10.0 * (l[i] - best));
    for (int i = 1; i < 3; ++i)
        if (g.pl[i] < g.pl[g.gt]) g.gt = i;
    int64_t s[3] = {g.pl[0], g.pl[1], g.pl[2]};
    std::sort(s, s + 3);
    g.gq = (int)std::min<int64_t>(99, s[1]);
    g.called = true;
    return g;
}

CiOffsets ci_offsets(int64_t lo, int64_t hi, int64_t P) {
    CiOffsets c;
    c.a = std::min({lo, hi, P}) - P;
    c.b = std::max({lo, hi, P}) - P;
    return c;
}

DepthSpans depth_spans(int64_t pos1, int64_t pos2, int64_t flank, int64_t contig_len) {
    const int64_t len = std::max<int64_t>(contig_len, 0);
    auto clamp = [&](int64_t p) { return std::min(std::max<int64_t>(p, 1), len + 1); };   // (1-based; len + 1: the end of a half-open bound)
    const int64_t lo = std::min(pos1, pos2), hi = std::max(pos1, pos2);
    DepthSpans s;
    s.in_beg = clamp(lo) - 1; s.in_end = clamp(hi) - 1;
    s.left_beg = clamp(lo - flank) - 1; s.left_end = s.in_beg;
    s.right_beg = s.in_end; s.right_end = clamp(hi + flank) - 1;
    return s;
}

std::string depth_ratio(int64_t rci, int64_t rcf, int64_t len_in, int64_t len_flank) {
    if (rci < 0 || rcf <= 0 || len_in <= 0 || len_flank <= 0) return ".";
    char buf[64];
    snprintf(buf, sizeof buf, "%.3f", (double)rci * (double)len_flank / ((double)len_in * (double)rcf));
    return buf;
}

std::string mapq_info(const EndQuality& e1, const EndQuality& e2, bool swapped) {
    const EndQuality* e[2] = {swapped ? &e2 : &e1, swapped ? &e1 : &e2};
    auto key = [&](const char* name, auto entry) {
        std::string s = std::string(";") + name + "=";
        for (int k = 0; k < 2; ++k) s += (k ? "," : "") + (e[k]->held ? entry(*e[k]) : std::string("."));
        return s;
    };
    auto quality = [](unsigned EndQuality::*q) { return [q](const EndQuality& x) { return x.n ? std::to_string(x.*q) : std::string("."); }; };
    auto count = [](uint32_t EndQuality::*c) { return [c](const EndQuality& x) { return std::to_string(x.*c); }; };
    return key("SQN", count(&EndQuality::n)) + key("SQMIN", quality(&EndQuality::qmin)) + key("SQQ1", quality(&EndQuality::q1)) +
           key("SQMED", quality(&EndQuality::median)) + key("SQMAX", quality(&EndQuality::qmax)) + key("LQA", count(&EndQuality::n_all)) +
           key("LQN", count(&EndQuality::n_low)) + key("LQF", [](const EndQuality& x) {
               if (!x.n_all) return std::string(".");
               char buf[32];
               snprintf(buf, sizeof buf, "%.3f", (double)x.n_low / (double)x.n_all);
               return std::string(buf);
           });
}

ClipWinner clip_winner(const EndClips& e) {
    ClipWinner w;
    if (!e.peak_left && !e.peak_right) return w;
    const int64_t dl = e.pos_left > e.pos ? e.pos_left - e.pos : e.pos - e.pos_left, dr = e.pos_right > e.pos ? e.pos_right - e.pos : e.pos - e.pos_right;
    const bool right = e.peak_right > e.peak_left || (e.peak_right == e.peak_left && dr < dl);
    w.side = right ? 'R' : 'L';
    w.pos = right ? e.pos_right : e.pos_left;
    w.peak = right ? e.peak_right : e.peak_left;
    return w;
}

std::string clip_info(const EndClips& e1, const EndClips& e2, bool swapped, uint32_t support) {
    const EndClips* e[2] = {swapped ? &e2 : &e1, swapped ? &e1 : &e2};
    auto key = [&](const char* name, auto entry) {
        std::string s = std::string(";") + name + "=";
        for (int k = 0; k < 2; ++k) s += (k ? "," : "") + (e[k]->held ? entry(*e[k]) : std::string("."));
        return s;
    };
    auto of_winner = [support](auto field) {
        return [support, field](const EndClips& x) {
            const ClipWinner w = clip_winner(x);
            return w.side && w.peak >= support ? field(w) : std::string(".");
        };
    };
    return key("CLN", [](const EndClips& x) { return std::to_string((uint64_t)x.n_left + x.n_right); }) +
           key("CLPOS", of_winner([](const ClipWinner& w) { return std::to_string(w.pos); })) +
           key("CLSUP", of_winner([](const ClipWinner& w) { return std::to_string(w.peak); })) +
           key("CLSIDE", of_winner([](const ClipWinner& w) { return std::string(1, w.side); }));
}

VcfWriter::VcfWriter(const std::string& path) : path_(path) {
    f_ = fopen(path.c_str(), "w");
    if (!f_) throw std::runtime_error("unable to open VCF output file '" + path + "'");
}

VcfWriter::~VcfWriter() {
    if (f_) fclose(f_);
}

void VcfWriter::write(const std::vector<std::string>& argv, const std::vector<std::string>& contigs, const std::vector<uint32_t>& lengths,
                      const std::vector<std::string>& samples, std::vector<VcfRecord> records, const std::string& exclude,
                      const VcfSites* sites, bool mark_dup, const VcfCi* ci, const VcfDepth* depth, const VcfMapq* mapq, bool estimate, const VcfClip* clip) {
    if (!f_) throw std::runtime_error("VCF output file '" + path_ + "' is already closed");
    FILE* f = f_;
    fprintf(f, "##fileformat=VCFv4.2\n##source=breakdancer-max-mi355x\n##command=");
    for (size_t i = 0; i < argv.size(); ++i) fprintf(f, "%s%s", i ? " " : "", argv[i].c_str());
    fprintf(f, "\n");
    if (!exclude.empty()) fprintf(f, "##exclude=%s\n", exclude.c_str());
    if (sites) fprintf(f, "##sites=%s\n##sites_window=%d\n", sites->file.c_str(), sites->window);
    if (mark_dup) fprintf(f, "##mark_dup=1\n");
    if (estimate) fprintf(f, "##estimate=1\n");
    if (ci) fprintf(f, "##ci_window=%d\n", ci->window);
    if (depth) fprintf(f, "##depth_flank=%d\n", depth->flank);
    if (mapq) fprintf(f, "##mapq_window=%d\n", mapq->window);
    if (clip) fprintf(f, "##clip_window=%d\n##clip_min=%d\n##clip_support=%d\n", clip->window, clip->min_clip, clip->support);
    for (size_t t = 0; t < contigs.size(); ++t)
        fprintf(f, "##contig=<ID=%s,length=%u>\n", contigs[t].c_str(), t < lengths.size() ? lengths[t] : 0u);
    fputs("##FILTER=<ID=PASS,Description=\"All filters passed\">\n"
          "##ALT=<ID=DEL,Description=\"Deletion\">\n"
          "##ALT=<ID=INS,Description=\"Insertion\">\n"
          "##ALT=<ID=INV,Description=\"Inversion\">\n"
          "##ALT=<ID=ITX,Description=\"Intra-chromosomal translocation\">\n"
          "##ALT=<ID=CTX,Description=\"Inter-chromosomal translocation\">\n"
          "##INFO=<ID=IMPRECISE,Number=0,Type=Flag,Description=\"Imprecise structural variation: breakpoints from read-pair clusters\">\n"
          "##INFO=<ID=SVTYPE,Number=1,Type=String,Description=\"Type of structural variant (the table's Type column)\">\n"
          "##INFO=<ID=CHR2,Number=1,Type=String,Description=\"Chromosome of the second breakpoint (Chr2)\">\n"
          "##INFO=<ID=POS2,Number=1,Type=Integer,Description=\"Position of the second breakpoint (Pos2)\">\n"
          "##INFO=<ID=END,Number=1,Type=Integer,Description=\"End position of the variant (Pos2; same chromosome, Pos2 >= Pos1 only)\">\n"
          "##INFO=<ID=SVLEN,Number=1,Type=Integer,Description=\"Difference in length between REF and ALT alleles (-Size; DEL and INS only)\">\n",
          f);
    if (!sites)
        fputs("##INFO=<ID=ORI1,Number=1,Type=String,Description=\"Reads on the + and - strand at the first breakpoint (Orientation1)\">\n"
              "##INFO=<ID=ORI2,Number=1,Type=String,Description=\"Reads on the + and - strand at the second breakpoint (Orientation2)\">\n"
              "##INFO=<ID=NREADS,Number=1,Type=Integer,Description=\"Read pairs supporting the call (num_Reads)\">\n"
              "##INFO=<ID=BDAF,Number=1,Type=Float,Description=\"BreakDancer allele frequency (Allele_frequency)\">\n",
              f);
    if (ci)
        fputs("##INFO=<ID=CIPOS,Number=2,Type=Integer,Description=\"Confidence interval around POS: the breakpoint interval the supporting pairs' reads allow (read start, strand, library uppercutoff)\">\n"
              "##INFO=<ID=CIEND,Number=2,Type=Integer,Description=\"Confidence interval around END, likewise\">\n"
              "##INFO=<ID=CIPOS2,Number=2,Type=Integer,Description=\"Confidence interval around POS2, likewise (records without END)\">\n"
              "##INFO=<ID=CIN,Number=1,Type=Integer,Description=\"Read pairs the confidence intervals come from: those with one mate starting within ci_window of each breakpoint\">\n",
              f);
    if (mapq)
        fputs("##INFO=<ID=SQN,Number=2,Type=Integer,Description=\"Reads supporting the first and the second printed breakpoint: passing reads of the record's type that start within mapq_window of it with their mate within mapq_window of the other (all samples pooled)\">\n"
              "##INFO=<ID=SQMIN,Number=2,Type=Integer,Description=\"Smallest mapping quality among those reads (the AM tag if present, else MAPQ)\">\n"
              "##INFO=<ID=SQQ1,Number=2,Type=Integer,Description=\"Lower quartile of their mapping qualities: the smallest q that ceil(SQN / 4) of them do not exceed\">\n"
              "##INFO=<ID=SQMED,Number=2,Type=Integer,Description=\"Lower median of their mapping qualities: the smallest q that ceil(SQN / 2) of them do not exceed\">\n"
              "##INFO=<ID=SQMAX,Number=2,Type=Integer,Description=\"Largest mapping quality among them\">\n"
              "##INFO=<ID=LQA,Number=2,Type=Integer,Description=\"Mapped reads that start within mapq_window of the breakpoint, whatever their class\">\n"
              "##INFO=<ID=LQN,Number=2,Type=Integer,Description=\"Those among LQA whose mapping quality does not exceed their library's minimum (-q, or the configuration's mapqual)\">\n"
              "##INFO=<ID=LQF,Number=2,Type=Float,Description=\"LQN / LQA\">\n",
              f);
    if (clip)
        fputs("##INFO=<ID=CLN,Number=2,Type=Integer,Description=\"Clipped reads at the first and the second printed breakpoint: passing reads soft- or hard-clipped by clip_min bases or more whose clip stands within clip_window of it, left and right clips together (all samples pooled)\">\n"
              "##INFO=<ID=CLPOS,Number=2,Type=Integer,Description=\"Where most of them are clipped, 1-based: with CLSIDE L the first aligned base of reads clipped on their left (the junction lies between CLPOS - 1 and CLPOS), with R the last aligned base of reads clipped on their right (between CLPOS and CLPOS + 1); '.' below clip_support reads\">\n"
              "##INFO=<ID=CLSUP,Number=2,Type=Integer,Description=\"Reads clipped at CLPOS on that side\">\n"
              "##INFO=<ID=CLSIDE,Number=2,Type=String,Description=\"L or R: the side of the reads that is clipped at CLPOS (the larger pile; ties: the nearer to the breakpoint, then L)\">\n",
              f);
    fputs("##FORMAT=<ID=GT,Number=1,Type=String,Description=\"Genotype\">\n"
          "##FORMAT=<ID=GQ,Number=1,Type=Integer,Description=\"Genotype quality: second-smallest PL, capped at 99\">\n"
          "##FORMAT=<ID=PL,Number=G,Type=Integer,Description=\"Phred-scaled genotype likelihoods (binomial, alt-read probability 0.01/0.5/0.99)\">\n"
          "##FORMAT=<ID=DR,Number=1,Type=Integer,Description=\"Normal read pairs whose fragment covers a breakpoint junction\">\n",
          f);
    fputs(sites ? "##FORMAT=<ID=DV,Number=1,Type=Integer,Description=\"Read pairs of the site's type with one mate starting within sites_window of each breakpoint\">\n"
                : "##FORMAT=<ID=DV,Number=1,Type=Integer,Description=\"Read pairs supporting the call (the dominant type's pairs)\">\n",
          f);
    if (depth)
        fputs("##FORMAT=<ID=RCI,Number=1,Type=Integer,Description=\"Read starts inside the record: reads that passed the caller's filters and start at min(POS, POS2) <= p < max(POS, POS2) (a read-start count, not a per-base depth)\">\n"
              "##FORMAT=<ID=RCF,Number=1,Type=Integer,Description=\"Read starts in the record's two flanks of depth_flank bases each, clamped to the contig\">\n"
              "##FORMAT=<ID=RDR,Number=1,Type=Float,Description=\"Read-start density inside the record over that of its flanks: (RCI / inside length) / (RCF / flank length)\">\n",
              f);
    fprintf(f, "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT");
    for (auto const& s : samples) fprintf(f, "\t%s", s.c_str());
    fprintf(f, "\n");
    std::stable_sort(records.begin(), records.end(),
                     [](const VcfRecord& x, const VcfRecord& y) { return x.chr1 != y.chr1 ? x.chr1 < y.chr1 : x.pos1 < y.pos1; });
    auto name = [&](int t) { return t >= 0 && (size_t)t < contigs.size() ? contigs[t] : std::to_string(t); };
    for (auto const& r : records) {
        const std::string type = r.type.empty() ? "." : r.type;
        const std::string qual = sites ? "." : std::to_string(r.score);
        fprintf(f, "%s\t%d\t%s%zu\tN\t%s\t%s\tPASS\tIMPRECISE;SVTYPE=%s;CHR2=%s;POS2=%d", name(r.chr1).c_str(), r.pos1, sites ? "SITE" : "BDX", r.row,
                r.type.empty() ? "." : ("<" + r.type + ">").c_str(), qual.c_str(), type.c_str(), name(r.chr2).c_str(), r.pos2);
        if (r.chr2 == r.chr1 && r.pos2 >= r.pos1) fprintf(f, ";END=%d", r.pos2);
        if ((r.type == "DEL" || r.type == "INS") && r.has_size) fprintf(f, ";SVLEN=%lld", -(long long)r.size);
        if (!sites) {
            fprintf(f, ";ORI1=%s;ORI2=%s;NREADS=%d;BDAF=", r.ori1.c_str(), r.ori2.c_str(), r.nreads);
            if (std::isfinite(r.af)) fprintf(f, "%.6g", (double)r.af);
            else fputs(".", f);
        }
        if (ci && r.has_ci) {
            const CiOffsets c1 = ci_offsets(r.ci_lo1, r.ci_hi1, r.pos1), c2 = ci_offsets(r.ci_lo2, r.ci_hi2, r.pos2);
            fprintf(f, ";CIPOS=%lld,%lld;%s=%lld,%lld;CIN=%u", (long long)c1.a, (long long)c1.b, r.chr2 == r.chr1 && r.pos2 >= r.pos1 ? "CIEND" : "CIPOS2",
                    (long long)c2.a, (long long)c2.b, r.ci_n);
        }
        if (mapq && r.has_mapq) fputs(mapq_info(r.mq[0], r.mq[1], r.mq_swapped).c_str(), f);
        if (clip && r.has_clip) fputs(clip_info(r.cl[0], r.cl[1], r.cl_swapped, (uint32_t)clip->support).c_str(), f);
        fputs(depth ? "\tGT:GQ:PL:DR:DV:RCI:RCF:RDR" : "\tGT:GQ:PL:DR:DV", f);
        for (size_t k = 0; k < samples.size(); ++k) {
            const int64_t dr = k < r.dr.size() ? r.dr[k] : -1, dv = k < r.dv.size() ? r.dv[k] : 0;
            const Genotype g = call_genotype(dr, dv);
            static const char* kGt[3] = {"0/0", "0/1", "1/1"};
            if (g.called)
                fprintf(f, "\t%s:%d:%lld,%lld,%lld:", kGt[g.gt], g.gq, (long long)g.pl[0], (long long)g.pl[1], (long long)g.pl[2]);
            else
                fputs("\t./.:.:.:", f);
            if (dr < 0) fputs(".:", f);
            else fprintf(f, "%lld:", (long long)dr);
            if (dv < 0) fputs(".", f);
            else fprintf(f, "%lld", (long long)dv);
            if (depth) {
                const int64_t rci = r.has_depth && k < r.rci.size() ? r.rci[k] : -1, rcf = r.has_depth && k < r.rcf.size() ? r.rcf[k] : -1;
                if (rci < 0 || rcf < 0) fputs(":.:.:.", f);
                else fprintf(f, ":%lld:%lld:%s", (long long)rci, (long long)rcf, depth_ratio(rci, rcf, r.spans.len_in(), r.spans.len_flank()).c_str());
            }
        }
        fputs("\n", f);
    }
    const bool bad = ferror(f) != 0;
    const int rc = fclose(f);
    f_ = nullptr;
    if (bad || rc != 0) throw std::runtime_error("writing VCF output file '" + path_ + "' failed");
}

}  // namespace bdhost
