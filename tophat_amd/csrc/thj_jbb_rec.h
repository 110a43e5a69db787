// thj_jbb_rec.h -- what the choice among a read's alignments keeps of every record until finish (thj_juncbed_best_impl.h writes it,
// the accepted-hits pass of thj_accepted.hip reads it again)
#pragma once
#include <stdint.h>

enum : uint8_t { JBB_FIRST = 1, JBB_GONE = 2, JBB_DUP1 = 4, JBB_ANTI = 8, JBB_FUSED = 16,       // first record of its read; dropped by the read filter; pass-1 duplicate; antisense_align; it has a fusion op
                 JBB_SPLICED = 32, JBB_ANTI_SPLICE = 64 };     // not contiguous() (anything but one MATCH operation); antisense_splice(): what happy() of an insert's grade asks
// jfirst / nj: the record's junction occurrences (thj_k_jb_add fills them in)
struct alignas(8) JbbRec { unsigned long long jfirst; uint32_t ref_id, ref_id2; int32_t left, right; uint32_t rank; int16_t AS; uint16_t read_len; uint8_t mismatches, edit_dist, n_cigar, nj, flags; };
static_assert(sizeof(JbbRec) == 40, "kept record layout");
// an insert of a consensus whose inserts are graded (thj_juncbed_pair_impl.h writes them; thj_unmapped.hip finds a read's insert again)
struct JbpIns { unsigned long long first, coff; uint32_t nl, nr; };           // records [first, first + nl) left, [first + nl, first + nl + nr) right; its list at cand[coff ..]
