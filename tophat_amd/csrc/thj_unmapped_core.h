// thj_unmapped_core.h -- what tophat_reports does with the READS files: which reads go to unmapped_left_0.bam / unmapped_right_0.bam, the
// record GetReadProc::writeUnmapped makes of one, and the fifteen SAlignStats counters behind align_summary.txt:
//
//   CReadProc::process (a read the walk passes: no alignment group)        tophat_reports.cpp:2197-2219
//   write_singleton_alignments (a read with a group that goes alone)        tophat_reports.cpp:2229-2322
//   the worker loop (an insert with both groups) and the trailing getQRead   tophat_reports.cpp:2324-2611
//   SAlignStats, print_alnStats                                             tophat_reports.cpp:312-356, :2119-2195
//   matenum from 0x40 / 0x80, trashCode from ZT                             reads.h:149-176
//   writeUnmapped                                                           reads.h:235-258
//   bam2Read (alt_name from ZN:Z), getQRead                                 reads.cpp:508-525, :632-676
//   GBamRecord's constructor, set_cigar without a CIGAR, add_sequence, add_quals, seqData   common.cpp:974-998, :1025-1109, :1249-1337
//   InsertAlignmentGrade::concordant()                                      inserts.h:222-225
//
// The reference walks each reads file once beside the two hit streams and decides per read as it passes it.  Whether a read is written and
// what it counts is a function of that read and of its own alignment group (single-end) or insert (paired) alone, so here the finish leaves
// one word per read / insert and every record of a reads file is decided on its own: decide().  emit() makes the record; with a sink that
// only counts it gives the size (a lane per record), with a sink over a wave it writes (thj_unmapped.hip), with a sink over plain memory
// tests/unmappedsim runs it on the CPU.
//
// Not here: -p > 1, FASTQ reads files, the ReadBufSize reordering of unsorted reads, quality bytes 223 and 232 (their text is a NUL / a TAB
// for the reference's strings; they are copied like every other byte).
#pragma once
#include <stdint.h>

#include "thj_accepted_core.h"

namespace um {

// what ends the call, with a message that names the case; never another answer
enum { LOUD_MALFORMED = 1u,     // the header or a tag does not fit the record, a tag of no BAM type
       LOUD_QNAME = 2u,         // a QNAME that is not 1 .. 18 digits
       LOUD_ZERO = 4u,          // read number 0 ("no read" to the reference)
       LOUD_ORDER = 8u,         // a number that falls or repeats
       LOUD_LSEQ = 16u,         // l_seq over 65535
       LOUD_ZN = 32u,           // a ZN tag that is no string, or one of more than 254 characters (l_qname is a byte)
       LOUD_UNPAIRED = 64u };   // paired run: a read without mate bits whose insert has a side of which only records over the read filter's limits are left

inline const char* loud_text(uint32_t loud) {
    if (loud & LOUD_MALFORMED) return "a malformed read record (its header or a tag does not fit its block_size, or a tag of no BAM type)";
    if (loud & LOUD_QNAME) return "a QNAME that is not digits (1 .. 18 of them): the reads file is not prep_reads' output";
    if (loud & LOUD_ZERO) return "read number 0";
    if (loud & LOUD_ORDER) return "read numbers that fall or repeat";
    if (loud & LOUD_LSEQ) return "a read of more than 65535 bases (l_seq)";
    if (loud & LOUD_ZN) return "a ZN tag that is no string, or one of more than 254 characters";
    if (loud & LOUD_UNPAIRED) return "a read without mate bits in a paired run whose insert has a side with nothing but records over the read filter's limits left: not built";
    return "";
}

// SAlignStats' fields in their order
enum { AL_L, UM_L, MULTI_L, XMULTI_L, AL_R, UM_R, MULTI_R, XMULTI_R, PAIRS, PAIRS_MULTI, PAIRS_DISC, AL_U, UM_U, MULTI_U, XMULTI_U, N_STATS = 15 };
// the four counters of a kind: the left read's, the right read's, the unpaired ones (write_singleton_alignments, :2234-2264)
enum { SET_L = 0, SET_R = 1, SET_U = 2 };
THJ_HD uint32_t aligned(uint32_t set) { return set == SET_L ? AL_L : set == SET_R ? AL_R : AL_U; }
THJ_HD uint32_t unmapped(uint32_t set) { return set == SET_L ? UM_L : set == SET_R ? UM_R : UM_U; }
THJ_HD uint32_t multi(uint32_t set) { return set == SET_L ? MULTI_L : set == SET_R ? MULTI_R : MULTI_U; }
THJ_HD uint32_t xmulti(uint32_t set) { return set == SET_L ? XMULTI_L : set == SET_R ? XMULTI_R : XMULTI_U; }

// read_best_alignments' return code with final_report, from what is left of a read at its best score (n) : 1 a valid mapping, 4 several,
// 16 over --max-multihits (:170-212)
enum { RC_ALIGNED = 1u, RC_MULTI = 4u, RC_OVER = 16u };
THJ_HD uint32_t read_code(uint32_t n, uint32_t max_multihits, bool suppress) {
    const bool over = n > max_multihits;
    const uint32_t left = over ? (suppress ? 0u : max_multihits) : n;
    return (left > 0u ? RC_ALIGNED : 0u) | (left > 1u ? RC_MULTI : 0u) | (over ? RC_OVER : 0u);
}

// An insert's word (paired input): which sides have an alignment group, and the way the worker loop takes (:2388-2594).
//   W_PAIRED     the insert stays in the paired branch (:2495-2564): the counters are the sides' own, whatever the reads' mate bits say
//   W_P_ANY / W_P_MULTI / W_P_OVER   pair_best_alignments' code: 3, 12, 48 from the list's length before the cap (:526-536)
//   W_P_EMPTY    best_hits is empty at :2534 (no pair, or --suppress-hits over the cap)
//   W_DISC       (flags & 3) == 3 && !grade.concordant(), :2485-2487 -- counted also when the pairs are then given up for the sides
//   W_ROUTED_x   side x goes through write_singleton_alignments (its counters are chosen by the read's mate bits); otherwise a side
//                with a group counts num_unmapped_<side> and is written (:2572-2584)
//   W_AMBIG      a side has nothing live left but records over the read filter's limits: whether the reference's hit group is empty
//                there (exclude_hits_on_filtered_junctions looks at those records too, :2426-2435) is not known here.  It changes
//                nothing for a read with mate bits; a read without them is LOUD_UNPAIRED
enum { W_HAS_L = 1u, W_HAS_R = 2u, W_PAIRED = 4u, W_P_ANY = 8u, W_P_MULTI = 16u, W_P_OVER = 32u, W_P_EMPTY = 64u, W_DISC = 128u, W_AMBIG = 256u,
       W_ROUTED_L = 512u, W_ROUTED_R = 1024u };
// live: records that compete are left (under the limits, not excluded); gone: records over the limits; n_list: the pair list's length after
// std::unique, before the cap; best_fusion / best_conc: grade.fusion and grade.concordant() of the best grade
THJ_HD uint32_t insert_word(bool has_l, bool has_r, bool live_l, bool live_r, bool gone_l, bool gone_r, uint32_t n_list, bool best_fusion, bool best_conc,
                            uint32_t max_multihits, bool suppress, bool mixed, bool discordant) {
    uint32_t w = (has_l ? W_HAS_L : 0u) | (has_r ? W_HAS_R : 0u);
    if (!has_l || !has_r) return w | (has_l ? W_ROUTED_L : 0u) | (has_r ? W_ROUTED_R : 0u);      // a singleton: :2396-2418
    const bool hits_l = live_l || gone_l, hits_r = live_r || gone_r;
    if ((!live_l && gone_l) || (!live_r && gone_r)) w |= W_AMBIG;
    if (hits_l && hits_r) {
        const uint32_t n = live_l && live_r ? n_list : 0u;
        const bool any = n > 0u, over = n > max_multihits, empty = !any || (over && suppress);
        if (any && !best_conc) w |= W_DISC;
        const bool paired = !(mixed && (empty || (best_fusion && !discordant)));                  // :2488-2493
        if (paired) return w | W_PAIRED | (any ? W_P_ANY : 0u) | (n > 1u ? W_P_MULTI : 0u) | (over ? W_P_OVER : 0u) | (empty ? W_P_EMPTY : 0u);
        return w | W_ROUTED_L | W_ROUTED_R;
    }
    return w | (hits_l ? W_ROUTED_L : 0u) | (hits_r ? W_ROUTED_R : 0u);
}

// the run: paired = right maps are there (PE_reads); mixed = --report-mixed-alignments
struct Run { uint8_t paired, mixed; };
// what one record of a reads file does: the counters it adds one to (bit k = SAlignStats field k), whether it is written
struct Decision { uint32_t counters; uint32_t write; uint32_t loud; };

// side: 0 the left (or only) reads file, 1 the right one.  found: the read's number has an alignment group (single-end) or an insert
// (paired) -- word = the insert's word; code = read_best_alignments' code of the read itself (single-end; a side that goes alone under
// --report-mixed-alignments).  zt: the ZT:A value, 0 without; matenum: 1 / 2 from 0x40 / 0x80, else 0
THJ_HD Decision decide(const Run& run, uint32_t side, bool found, uint32_t word, uint32_t code, uint8_t zt, uint32_t matenum) {
    Decision d{0u, 0u, 0u};
    // the counters write_singleton_alignments picks (:2234-2264) and CReadProc is given (:2378-2386)
    const uint32_t set = !run.paired ? SET_L : matenum == 0u ? SET_U : side ? SET_R : SET_L;
    const uint32_t own = side ? SET_R : SET_L;
    const bool has_group = found && (!run.paired || (word & (side ? W_HAS_R : W_HAS_L)));
    if (!has_group) {                                           // CReadProc::process with found == false
        if (zt != (uint8_t)'M') { d.write = 1u; d.counters |= 1u << unmapped(set); }
        else d.counters |= 1u << xmulti(set);
        return d;
    }
    auto singleton = [&](bool by_code) {                        // write_singleton_alignments
        if (!by_code) { d.write = 1u; d.counters |= 1u << unmapped(set); return; }             // :2266-2280
        if (code & RC_MULTI) d.counters |= 1u << multi(set);
        if (code & RC_OVER) d.counters |= 1u << xmulti(set);
        if (code & RC_ALIGNED) d.counters |= 1u << aligned(set);
        else { d.counters |= 1u << unmapped(set); d.write = 1u; }
    };
    if (!run.paired) { singleton(true); return d; }
    if ((word & W_AMBIG) && matenum == 0u) { d.loud = LOUD_UNPAIRED; return d; }
    if (side == 0u && (word & W_DISC)) d.counters |= 1u << PAIRS_DISC;
    if (word & W_PAIRED) {                                      // :2534-2563
        if (!(word & W_P_EMPTY)) { d.counters |= 1u << aligned(own); if (side == 0u) d.counters |= 1u << PAIRS; }
        else d.counters |= 1u << unmapped(own);
        if (word & W_P_MULTI) { d.counters |= 1u << multi(own); if (side == 0u) d.counters |= 1u << PAIRS_MULTI; }
        if (word & W_P_OVER) d.counters |= 1u << xmulti(own);
        if (!(word & W_P_ANY)) d.write = 1u;
        return d;
    }
    if (word & (side ? W_ROUTED_R : W_ROUTED_L)) { singleton(run.mixed != 0); return d; }
    d.write = 1u; d.counters |= 1u << unmapped(own);            // :2572-2584
    return d;
}

// ---- one record of a reads file (prep_reads' unaligned BAM): what writeUnmapped and the walk read of it
struct Read {
    uint64_t number;            // atol(QNAME)
    uint32_t flag, l_seq, matenum;
    uint32_t zn_at, zn_len;     // the ZN value inside the record, cut at its last '/' when fewer than 4 characters remain from there (reads.h:237-240)
    uint32_t seq_at, qual_at;
    uint8_t zt;                 // bam_aux2A of the first ZT tag: its value when its type is A, else 0
    uint32_t loud;
};

// QNAME -> number: digits only (the reference's atol would take "12abc" as 12: not guessed)
THJ_HD bool parse_number(const uint8_t* rec, uint32_t bs, uint64_t& number) {
    number = 0;
    if (bs < 32u) return false;
    const uint32_t l_qname = rec[8];
    if (l_qname < 2u || l_qname > 19u || 32u + l_qname > bs || rec[32u + l_qname - 1u] != 0u) return false;
    for (uint32_t k = 0; k + 1u < l_qname; ++k) {
        const uint8_t ch = rec[32u + k];
        if (ch < (uint8_t)'0' || ch > (uint8_t)'9') return false;
        number = number * 10u + (uint64_t)(ch - (uint8_t)'0');
    }
    return true;
}

// rec: the record behind its block_size field, bs bytes
THJ_HD void parse(const uint8_t* rec, uint32_t bs, Read& r) {
    r = Read{};
    if (bs < 32u) { r.loud = LOUD_MALFORMED; return; }
    const uint32_t l_qname = rec[8], n_cigar = acc::rd16(rec + 12), l_seq = acc::rd32(rec + 16);
    r.flag = acc::rd16(rec + 14); r.l_seq = l_seq;
    r.matenum = (r.flag & 0x40u) ? 1u : (r.flag & 0x80u) ? 2u : 0u;                     // reads.h:169-172: 0x1 is not looked at
    if (l_seq > 65535u) { r.loud = LOUD_LSEQ; return; }
    const uint64_t fixed = 32ull + l_qname + 4ull * n_cigar + (l_seq + 1u) / 2u + l_seq;
    if (l_qname < 1u || fixed > bs) { r.loud = LOUD_MALFORMED; return; }
    if (!parse_number(rec, bs, r.number)) { r.loud = LOUD_QNAME; return; }
    if (r.number == 0u) { r.loud = LOUD_ZERO; return; }
    r.seq_at = 32u + l_qname + 4u * n_cigar; r.qual_at = r.seq_at + (l_seq + 1u) / 2u;
    // bam_aux_get: the first tag of a name
    bool have_zn = false, have_zt = false;
    uint32_t p = (uint32_t)fixed;
    while (p < bs) {
        if (p + 3u > bs) { r.loud = LOUD_MALFORMED; return; }
        const uint8_t k0 = rec[p], k1 = rec[p + 1u], ty = rec[p + 2u];
        uint32_t v = p + 3u, len = 0;
        if (ty == 'A' || ty == 'c' || ty == 'C') len = 1;
        else if (ty == 's' || ty == 'S') len = 2;
        else if (ty == 'i' || ty == 'I' || ty == 'f') len = 4;
        else if (ty == 'd') len = 8;
        else if (ty == 'Z' || ty == 'H') { while (v + len < bs && rec[v + len]) ++len; if (v + len >= bs) { r.loud = LOUD_MALFORMED; return; } ++len; }
        else if (ty == 'B') {
            if (v + 5u > bs) { r.loud = LOUD_MALFORMED; return; }
            const uint8_t et = rec[v]; const uint32_t cnt = acc::rd32(rec + v + 1u);
            const uint32_t es = (et == 'c' || et == 'C') ? 1u : (et == 's' || et == 'S') ? 2u : (et == 'i' || et == 'I' || et == 'f') ? 4u : 0u;
            if (!es || (uint64_t)cnt * es > (uint64_t)bs) { r.loud = LOUD_MALFORMED; return; }
            len = 5u + cnt * es;
        } else { r.loud = LOUD_MALFORMED; return; }
        if ((uint64_t)v + len > bs) { r.loud = LOUD_MALFORMED; return; }
        if (k0 == 'Z' && k1 == 'N' && !have_zn) {
            have_zn = true;
            if ((ty != 'Z' && ty != 'H') || len - 1u > 254u) { r.loud = LOUD_ZN; return; }
            r.zn_at = v; r.zn_len = len - 1u;
            for (uint32_t k = r.zn_len; k > 0u; --k)
                if (rec[v + k - 1u] == (uint8_t)'/') { if (r.zn_len - (k - 1u) < 4u) r.zn_len = k - 1u; break; }
        }
        if (k0 == 'Z' && k1 == 'T' && !have_zt) { have_zt = true; r.zt = ty == 'A' ? rec[v] : (uint8_t)0; }
        p = v + len;
    }
}

// seqData's complement of a 4-bit base (common.cpp:1250)
THJ_HD uint32_t comp_nibble(uint32_t v) {
    const uint64_t table = 0xF7B3D561E9A2C480ull;               // { 0, 8, 4, 12, 2, 10, 9, 14, 1, 6, 5, 13, 3, 11, 7, 15 }, entry k at bits 4k
    return (uint32_t)(table >> (4u * v)) & 15u;
}
THJ_HD uint32_t nibble_at(const uint8_t* seq, uint32_t k) { return (seq[k >> 1] >> ((k & 1u) ? 0u : 4u)) & 15u; }
// output byte j of SEQ for a 0x10 input of l bases: bases 2j and 2j + 1 of the reverse complement (the spare nibble of an odd length is 0)
THJ_HD uint8_t revcomp_byte(const uint8_t* seq, uint32_t l, uint32_t j) {
    const uint32_t hi = comp_nibble(nibble_at(seq, l - 1u - 2u * j));
    const uint32_t lo = 2u * j + 1u < l ? comp_nibble(nibble_at(seq, l - 2u - 2u * j)) : 0u;
    return (uint8_t)((hi << 4) | lo);
}
// a quality byte through seqData's text and add_quals: 0xff reads as 'I' (common.cpp:1317-1319), every other byte comes back as it was
THJ_HD uint8_t qual_byte(uint8_t q) { return q == 0xFFu ? (uint8_t)('I' - 33) : q; }

// plain memory (the CPU's sink)
struct MemSink : acc::MemSink {
    THJ_HD void seq_fwd(uint32_t at, const uint8_t* src, uint32_t l) {
        for (uint32_t k = 0; k < l / 2u; ++k) o[at + k] = src[k];
        if (l & 1u) o[at + l / 2u] = (uint8_t)(src[l / 2u] & 0xF0u);
    }
    THJ_HD void seq_rev(uint32_t at, const uint8_t* src, uint32_t l) { for (uint32_t j = 0; j < (l + 1u) / 2u; ++j) o[at + j] = revcomp_byte(src, l, j); }
    THJ_HD void qual(uint32_t at, const uint8_t* src, uint32_t l, bool rev) { for (uint32_t j = 0; j < l; ++j) o[at + j] = qual_byte(src[rev ? l - 1u - j : j]); }
};
struct NullSink : acc::NullSink {
    THJ_HD void seq_fwd(uint32_t, const uint8_t*, uint32_t) {}
    THJ_HD void seq_rev(uint32_t, const uint8_t*, uint32_t) {}
    THJ_HD void qual(uint32_t, const uint8_t*, uint32_t, bool) {}
};

THJ_HD uint32_t record_size(const Read& r) { return 4u + 32u + r.zn_len + 1u + (r.l_seq + 1u) / 2u + r.l_seq + (r.zt ? 4u : 0u); }

// writeUnmapped's record, its block_size field included -> its size.  tid = mtid = -1, pos = mpos = -1, bin = bam_reg2bin(-1, 0), MAPQ 0,
// no CIGAR, FLAG 0x4 plus the mate bits, TLEN 0; SEQ and QUAL through seqData's text (a 0x10 input is reversed and complemented); QUAL is
// 0xff throughout when its text is "*" (one base of quality 9: add_quals, common.cpp:1104-1107); ZT:A when the input had one
template <class Sink>
THJ_HD uint32_t emit(const uint8_t* rec, const Read& r, Sink& out) {
    const uint32_t size = record_size(r), l = r.l_seq;
    const uint32_t flag = 0x4u | (r.matenum ? 0x1u | (r.matenum == 1u ? 0x40u : 0x80u) : 0u);
    out.put(0u, size - 4u, 4u);
    out.put(4u, 0xFFFFFFFFu, 4u); out.put(8u, 0xFFFFFFFFu, 4u);
    out.put(12u, ((acc::reg2bin(0xFFFFFFFFu, 0u) & 0xFFFFu) << 16) | (r.zn_len + 1u), 4u);      // (core.bin is a 16-bit field: 4680)
    out.put(16u, flag << 16, 4u);
    out.put(20u, l, 4u);
    out.put(24u, 0xFFFFFFFFu, 4u); out.put(28u, 0xFFFFFFFFu, 4u); out.put(32u, 0u, 4u);
    uint32_t o = 36u;
    if (r.zn_len) out.copy(o, rec + r.zn_at, r.zn_len);
    o += r.zn_len;
    out.put(o, 0u, 1u); ++o;
    const bool rev = (r.flag & 0x10u) != 0u;
    if (l) { if (rev) out.seq_rev(o, rec + r.seq_at, l); else out.seq_fwd(o, rec + r.seq_at, l); }
    o += (l + 1u) / 2u;
    if (l == 1u && rec[r.qual_at] == 9u) out.fill(o, 0xFFu, 1u);
    else if (l) out.qual(o, rec + r.qual_at, l, rev);
    o += l;
    if (r.zt) { out.put(o, (uint32_t)'Z' | ((uint32_t)'T' << 8) | ((uint32_t)'A' << 16) | ((uint32_t)r.zt << 24), 4u); o += 4u; }
    return o;
}

}  // namespace um
