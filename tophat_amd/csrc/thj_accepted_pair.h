// thj_accepted_pair.h -- what the two halves of thj_juncbed_report_pairs_bam hand each other: thj_accepted_pair_impl.h (beside the insert
// lists, in thj_juncbed_impl.h's translation unit) lays the output records of the inserts out, thj_accepted.hip rewrites them.
#pragma once
#include <stdint.h>
#include "thj_accepted_core.h"

struct thj_ctx;
// one output record: the record of the consensus it is written from (its ordinal), that record's left(), and what emit() is handed.
// slot.out = its place among the output records of the add call.
struct AccPairOut { uint32_t rec; int32_t left; acc::Slot slot; acc::Mate mate; };
// a list of more than acc::SORT_BY_COUNTING entries: its output records [base, base + n) lie in `hits` order (a pair's right record, then its
// left one) until the host has run std::sort on it (acc::sort_places)
struct AccPairBig { uint32_t base, n, pairs; };

// inserts [g0, g0 + ng) of the consensus, after thj_juncbed_finish.  d_cnt[k] (DEVICE, ng entries) = the output records of insert g0 + k:
// two per reported pair, or the reported records of its sides on the single-end way.
int thj_accp_count(thj_ctx* c, int64_t g0, int64_t ng, uint32_t* d_cnt);
// d_base = the exclusive sums of d_cnt; d_out (DEVICE) takes the records; d_big / d_nbig: the lists for the host (*d_nbig zeroed by the caller)
int thj_accp_layout(thj_ctx* c, int64_t g0, int64_t ng, const unsigned long long* d_base, AccPairOut* d_out, AccPairBig* d_big, uint32_t big_cap, unsigned int* d_nbig);
