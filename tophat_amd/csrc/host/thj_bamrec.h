// thj_bamrec.h -- the output records of long_spanning_reads on the host: print_bamhit for one alignment and for a batch.
// Needs include/thj.h (thj_aln, thj_md_string*), BamWriter and RefTable only, so the CPU test build (tests/hostio) holds it
// to BamWriter::encode without a device.
#pragma once
#include "thj_hostio.h"

namespace thjh {

// names, bases and qualities of a read from its own BAM record
inline void read_from_raw(const Read& rd, Read& out) {
    static const char nt16[] = "=ACMGRSVTWYHKDBN";
    const BamRawRec r(rd.raw);
    out.id = rd.id; out.raw = rd.raw;
    out.name.assign(r.name, r.l_read_name ? r.l_read_name - 1 : 0);
    out.seq.resize(r.l_seq); out.qual.resize(r.l_seq);
    for (uint32_t k = 0; k < r.l_seq; ++k) { out.seq[k] = nt16[r.base(k)]; out.qual[k] = (char)(r.qual[k] + 33); }
}

// print_bamhit for a plain (one-record) alignment whose read came as a BAM record: name, packed bases and qualities are copied
// (reversed / complemented nibble-wise for an antisense alignment) instead of going through strings.  Byte for byte what
// BamWriter::encode writes for the same record; false = take the general path.
inline bool encode_plain_from_raw(const BamWriter& bw, const RefTable& rt, const thj_aln& a, const Read& rd, int rlen, int indel, bool spliced,
                                  std::vector<uint8_t>& d, std::vector<uint32_t>& sizes, std::vector<long>& rids) {
    static const uint8_t bamop[16] = {0, 0, 0, 1, 1, 2, 2, 0, 0, 0, 0, 3, 3, 4, 5, 6};
    static const uint8_t comp16[16] = {15, 8, 4, 15, 2, 15, 15, 15, 1, 15, 15, 15, 15, 15, 15, 15};    // A<->T, C<->G, anything else N
    const BamRawRec r(rd.raw);
    const uint32_t lseq = r.l_seq, l_rn = r.l_read_name;
    if ((int)lseq != rlen || l_rn == 0) return false;
    const bool anti = (a.flags & THJ_HIT_ANTISENSE) != 0;
    const size_t at = d.size();
    const int32_t tid = bw.tid_of(rt.names[a.ref_id - 1]);
    const int32_t pos = a.left + 1 <= 0 ? -1 : a.left;
    int end = pos;
    for (int i = 0; i < a.n_cigar; ++i) { const uint32_t c = a.cigar[i], op = bamop[c >> 28]; if (op == 0 || op == 2 || op == 3) end += (int)(c & 0x0FFFFFFF); }
    const uint32_t bin = (uint32_t)reg2bin(pos, a.n_cigar == 0 ? pos + 1 : end);
    const size_t seq_b = (lseq + 1) >> 1;
    d.resize(at + 36 + l_rn + 4 * (size_t)a.n_cigar + seq_b + lseq);
    uint8_t* o = d.data() + at;
    auto w32 = [&](size_t off, uint32_t v) { memcpy(o + off, &v, 4); };
    w32(4, (uint32_t)tid); w32(8, (uint32_t)pos); w32(12, (bin << 16) | (255u << 8) | l_rn);
    w32(16, ((anti ? 0x10u : 0u) << 16) | (uint32_t)a.n_cigar); w32(20, lseq); w32(24, (uint32_t)-1); w32(28, (uint32_t)-1); w32(32, 0);
    memcpy(o + 36, r.name, l_rn);
    uint8_t* oc = o + 36 + l_rn;
    for (int i = 0; i < a.n_cigar; ++i) { const uint32_t v = ((a.cigar[i] & 0x0FFFFFFF) << 4) | bamop[a.cigar[i] >> 28]; memcpy(oc + 4 * i, &v, 4); }
    uint8_t* os = oc + 4 * (size_t)a.n_cigar;
    uint8_t* oq = os + seq_b;
    if (!anti) {                                      // (decoding a nibble to its letter and encoding it again is the identity)
        memcpy(os, r.seq, seq_b);
        if (lseq & 1) os[seq_b - 1] &= 0xF0;
        memcpy(oq, r.qual, lseq);
    } else {                                          // reverse_complement (reads.cpp:189-207): anything but A C G T becomes N
        memset(os, 0, seq_b);
        for (uint32_t k = 0; k < lseq; ++k) {
            const uint32_t j = lseq - 1 - k;
            os[k >> 1] |= (uint8_t)(comp16[r.base(j)] << ((k & 1) ? 0 : 4));
            oq[k] = r.qual[j];
        }
    }
    // aux: AS XM XO XG MD NM [XS]
    put_aux_int(d, 'A', 'S', (int)a.AS); put_aux_int(d, 'X', 'M', (int)a.XM); put_aux_int(d, 'X', 'O', (int)a.XO); put_aux_int(d, 'X', 'G', (int)a.XG);
    d.push_back('M'); d.push_back('D'); d.push_back('Z'); d.insert(d.end(), a.md, a.md + a.md_len); d.push_back(0);
    put_aux_int(d, 'N', 'M', (int)a.mismatches + indel);
    if (spliced) { d.push_back('X'); d.push_back('S'); d.push_back('A'); d.push_back((a.flags & THJ_HIT_ANTISENSE_SPLICE) ? '-' : '+'); }
    const uint32_t bs = (uint32_t)(d.size() - at - 4);
    memcpy(d.data() + at, &bs, 4);
    sizes.push_back((uint32_t)(d.size() - at));
    rids.push_back(r.read_id());
    return true;
}

// print_bamhit (bwt_map.cpp:1888-2093) for one alignment: one record, or -- a fusion alignment -- the two partial records of
// extract_partial_hits (:2148-2347), each carrying the whole alignment in XF:Z.  Appends (size, read id) per record.
inline void encode_aln(const BamWriter& bw, const RefTable& rt, const thj_aln& a, const Read& rd, std::vector<uint8_t>& d,
                       std::vector<uint32_t>& sizes, std::vector<long>& rids) {
    int rlen = 0, indel = 0; bool spliced = false;
    int fi = -1;
    for (int k = 0; k < a.n_cigar; ++k) {
        uint32_t op = a.cigar[k] >> 28, len = a.cigar[k] & 0x0FFFFFFF;
        if (op == 1 || op == 2 || op == 3 || op == 4 || op == 13) rlen += (int)len;
        if (op >= 3 && op <= 6) indel += (int)len;
        if (op == 11 || op == 12) spliced = true;
        if (op >= THJ_CIG_FUSION_FF && op <= THJ_CIG_FUSION_RR && fi < 0) fi = k;
    }
    if (rd.raw && fi < 0 && a.md_len != THJ_MD_ON_HOST && encode_plain_from_raw(bw, rt, a, rd, rlen, indel, spliced, d, sizes, rids)) return;
    Read tmp;
    const Read& rdx = rd.raw && rd.seq.empty() ? (read_from_raw(rd, tmp), tmp) : rd;
    std::string seq = rdx.seq, qual = rdx.qual;
    seq.resize((size_t)rlen); qual.resize((size_t)rlen);
    uint32_t flag = 0;
    if (a.flags & THJ_HIT_ANTISENSE) { flag |= 0x10; reverse_complement(seq); std::reverse(qual.begin(), qual.end()); }
    const uint32_t ref_id2 = fi >= 0 ? a.cigar[15] : a.ref_id;
    std::vector<std::string> aux;
    aux.push_back("AS:i:" + std::to_string((int)a.AS));
    aux.push_back("XM:i:" + std::to_string((int)a.XM));
    aux.push_back("XO:i:" + std::to_string((int)a.XO));
    aux.push_back("XG:i:" + std::to_string((int)a.XG));
    if (a.md_len == THJ_MD_ON_HOST) {                       // longer than a device record holds: rebuilt here from the same inputs
        char md[2048];
        const std::string& ref = const_cast<RefTable&>(rt).text(a.ref_id);
        const std::string& ref2 = const_cast<RefTable&>(rt).text(ref_id2);
        const int n = fi >= 0 ? thj_md_string2(ref.data(), (int64_t)ref.size(), ref2.data(), (int64_t)ref2.size(), seq.data(), (int32_t)seq.size(), a.left,
                                               a.cigar, a.n_cigar, md, (int32_t)sizeof md)
                              : thj_md_string(ref.data(), (int64_t)ref.size(), seq.data(), (int32_t)seq.size(), a.left, a.cigar, a.n_cigar, md, (int32_t)sizeof md);
        if (n < 0) die("Error: %s\n", thj_last_error());
        aux.push_back("MD:Z:" + std::string(md, (size_t)n));
    } else aux.push_back("MD:Z:" + std::string(a.md, a.md_len));
    aux.push_back("NM:i:" + std::to_string((int)a.mismatches + indel));
    if (spliced) aux.push_back(std::string("XS:A:") + ((a.flags & THJ_HIT_ANTISENSE_SPLICE) ? '-' : '+'));
    const long rid = atol(rdx.name.c_str());
    size_t before = d.size();
    if (fi < 0) {
        bw.encode(d, rdx.name, flag, rt.names[a.ref_id - 1], a.left + 1, a.cigar, a.n_cigar, seq, qual, aux);
        sizes.push_back((uint32_t)(d.size() - before)); rids.push_back(rid);
        return;
    }
    // ---- fusion alignment
    static const char letter[16] = {0, 'M', 'm', 'I', 'i', 'D', 'd', 'F', 'F', 'F', 'F', 'N', 'n', 'S', 0, 0};
    const uint32_t fdir = a.cigar[fi] >> 28;
    std::string full;
    int right = a.left, fusion_left = -1, fusion_right = -1;
    size_t left_part_len = 0;
    for (int k = 0; k < a.n_cigar; ++k) {
        const uint32_t op = a.cigar[k] >> 28, len = a.cigar[k] & 0x0FFFFFFF;
        full += std::to_string(op >= 7 && op <= 10 ? len + 1 : len); full += letter[op];
        if (op == 1 || op == 11 || op == 5) right += (int)len;
        else if (op == 2 || op == 12 || op == 6) right -= (int)len;
        else if (op >= 7 && op <= 10) { fusion_left = (op == 7 || op == 8) ? right - 1 : right + 1; fusion_right = right = (int)len; }
        if (k < fi && (op == 1 || op == 2 || op == 3 || op == 4)) left_part_len += len;
    }
    auto upper = [](uint32_t c) { const uint32_t op = c >> 28; return (op == 2 || op == 4 || op == 6 || op == 12) ? (((op - 1) << 28) | (c & 0x0FFFFFFF)) : c; };
    uint32_t c1[16], c2[16]; int n1 = 0, n2 = 0;
    if (fdir == 7 || fdir == 8) for (int k = 0; k < fi; ++k) c1[n1++] = upper(a.cigar[k]);
    else for (int k = fi - 1; k >= 0; --k) c1[n1++] = upper(a.cigar[k]);
    if (fdir == 7 || fdir == 9) for (int k = fi + 1; k < a.n_cigar; ++k) c2[n2++] = upper(a.cigar[k]);
    else for (int k = a.n_cigar - 1; k > fi; --k) c2[n2++] = upper(a.cigar[k]);
    if (left_part_len > seq.size()) left_part_len = seq.size();
    std::string seq1 = seq.substr(0, left_part_len), qual1 = qual.substr(0, left_part_len);
    std::string seq2 = seq.substr(left_part_len), qual2 = qual.substr(left_part_len);
    if (fdir == 9 || fdir == 10) { reverse_complement(seq1); std::reverse(qual1.begin(), qual1.end()); }
    if (fdir == 8 || fdir == 10) { reverse_complement(seq2); std::reverse(qual2.begin(), qual2.end()); }
    const int left1 = (fdir == 7 || fdir == 8) ? a.left : fusion_left;
    const int left2 = (fdir == 7 || fdir == 9) ? fusion_right : right + 1;
    const std::string& n1s = rt.names[a.ref_id - 1];
    const std::string& n2s = rt.names[ref_id2 - 1];
    const std::string xf = " " + n1s + "-" + n2s + " " + std::to_string(a.left + 1) + " " + full + " " + seq + " " + qual;
    aux.push_back("XF:Z:1" + xf);
    bw.encode(d, rdx.name, flag, n1s, left1 + 1, c1, n1, seq1, qual1, aux);
    sizes.push_back((uint32_t)(d.size() - before)); rids.push_back(rid);
    before = d.size();
    aux.back() = "XF:Z:2" + xf;
    bw.encode(d, rdx.name, flag, n2s, left2 + 1, c2, n2, seq2, qual2, aux);
    sizes.push_back((uint32_t)(d.size() - before)); rids.push_back(rid);
}

inline void encode_batch(const BamWriter& bw, const RefTable& rt, const thj_aln* alns, const size_t n, const std::vector<Read>& reads, int threads,
                         BamWriter::Encoded& e) {
    int T = threads;
    if ((size_t)T > n / 256 + 1) T = (int)(n / 256 + 1);
    std::vector<std::vector<uint8_t>> part((size_t)T);
    std::vector<std::vector<uint32_t>> psize((size_t)T);
    std::vector<std::vector<long>> prid((size_t)T);
    auto work = [&](int t) {
        const size_t a = n * (size_t)t / (size_t)T, b = n * (size_t)(t + 1) / (size_t)T;
        std::vector<uint8_t>& d = part[(size_t)t];
        d.reserve((b - a) * 256);
        psize[(size_t)t].reserve(b - a); prid[(size_t)t].reserve(b - a);
        for (size_t i = a; i < b; ++i) encode_aln(bw, rt, alns[i], reads[alns[i].read_idx], d, psize[(size_t)t], prid[(size_t)t]);
    };
    if (T > 1) { std::vector<std::thread> th; for (int t = 0; t < T; ++t) th.emplace_back(work, t); for (auto& x : th) x.join(); }
    else work(0);
    size_t total = 0, nrec = 0;
    for (auto& d : part) total += d.size();
    for (auto& v : psize) nrec += v.size();
    e.bytes.reserve(total); e.size.reserve(nrec); e.rid.reserve(nrec);
    for (size_t t = 0; t < (size_t)T; ++t) {
        e.bytes.insert(e.bytes.end(), part[t].begin(), part[t].end()); std::vector<uint8_t>().swap(part[t]);
        e.size.insert(e.size.end(), psize[t].begin(), psize[t].end());
        e.rid.insert(e.rid.end(), prid[t].begin(), prid[t].end());
    }
}

}  // namespace thjh
