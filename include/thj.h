/*
 * thj.h -- C ABI of libthj_hip.so: the MI355X-native junction-discovery hot path
 * that sits behind TopHat's `segment_juncs` and `long_spanning_reads` binaries.
 *
 * The reference (DaehwanKimLab/tophat v2.1.2) has no plugin / FFI surface for
 * this path: its boundary is process + argv + files (tophat.py:3070-3129 and
 * :3133-3200).  The drop-in executables keep that boundary; this header is the
 * thin C ABI between their C++ host code and the HIP kernels, and it is what a
 * binding in any other host language would bind.  Each entry point names the
 * reference code it replaces.
 *
 * Conventions: extern "C"; plain pointers and sizes; every function returns 0
 * on success and a negative THJ_E* code on failure with a message available
 * from thj_last_error() (thread-local); opaque handles; caller-owned buffers;
 * one context per (host thread, device); no global state.  Functions whose
 * name ends in _async only enqueue work on the context's HIP stream.
 * Pointers documented as DEVICE pointers must be HIP device allocations on the
 * context's device (e.g. hipMalloc or a torch tensor's data_ptr()).
 */
#ifndef THJ_H
#define THJ_H
#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define THJ_OK            0
#define THJ_EINVAL       -1   /* bad argument / unsupported parameter value */
#define THJ_ENOMEM       -2
#define THJ_EHIP         -3   /* a HIP runtime call failed */
#define THJ_EOVERFLOW    -4   /* an event table filled up; re-configure larger and re-run */
#define THJ_ESTATE       -5   /* call sequence violated (e.g. run before genome upload) */
#define THJ_ERETRY       -7   /* a device pool was too small for this pass and has been enlarged: make the same calls again */
#define THJ_EFALLBACK    -6   /* the device-side ingest cannot take this input (records straddle BGZF members, reads > 256 bases ...):
                                 nothing was done, use the host readers */

typedef struct thj_ctx thj_ctx;

/* One alignment record: the fields of BowtieHit (bwt_map.h:36-536) the path
 * reads, produced by BAMHitFactory::get_hit_from_buf (bwt_map.cpp:1101-1452).
 * `right` = BowtieHit::right() (bwt_map.h:213-243), `read_len` =
 * BowtieHit::read_len() (bwt_map.h:141-163). 16 bytes. */
typedef struct {
    uint32_t ref_id;      /* 1-based, @SQ order of --sam-header (bwt_map.h:608-632) */
    int32_t  left;
    int32_t  right;
    uint8_t  flags;       /* THJ_HIT_* */
    uint8_t  edit_dist;
    uint8_t  mismatches;
    uint8_t  read_len;
} thj_hit;

#define THJ_HIT_ANTISENSE 1u   /* BowtieHit::antisense_align() */
#define THJ_HIT_END       2u   /* BowtieHit::end() (bwt_map.cpp:1133-1140) */

/* The globals of common.cpp:79-180 that change hot-path results (SURVEY.md
 * Appendix A).  All int32, same order as tophat_amd/params.py. */
typedef struct {
    int32_t segment_length;
    int32_t segment_mismatches;
    int32_t min_segment_intron;
    int32_t max_segment_intron;
    int32_t max_insertion_length;
    int32_t max_deletion_length;
    int32_t max_seg_multihits;
    int32_t inner_dist_mean;
    int32_t inner_dist_std_dev;
    int32_t library_type;          /* common.h:155-167 */
    int32_t bowtie2;
    int32_t read_side;             /* segments.h:13-18: 1 READ_LEFT, 2 READ_RIGHT */
    int32_t min_report_intron;
    int32_t max_report_intron;
    int32_t min_anchor_len;
    int32_t read_mismatches;
    int32_t read_gap_length;
    int32_t read_edit_dist;
    int32_t bowtie2_max_penalty;
    int32_t bowtie2_min_penalty;
    int32_t bowtie2_penalty_for_N;
    int32_t bowtie2_read_gap_open;
    int32_t bowtie2_read_gap_cont;
    int32_t bowtie2_ref_gap_open;
    int32_t bowtie2_ref_gap_cont;
    int32_t fusion_anchor_length;  /* common.cpp:172 */
    int32_t fusion_min_dist;       /* common.cpp:173 */
    int32_t fusion_search;         /* common.cpp:171 (--fusion-search); long_spanning_reads only: thj_span_run_async */
} thj_params;

/* Fills `p` with the defaults of common.cpp:79-180. */
void thj_params_default(thj_params* p);

const char* thj_last_error(void);
const char* thj_version(void);

/* ------------------------------------------------------------ context */

/* Number of HIP devices visible to the process (< 0: error). */
int  thj_device_count(void);
/* `stream` is a hipStream_t to launch on (e.g. torch's current stream) or NULL
 * to let the context create its own non-blocking stream.  Work that runs beside that stream (the side chains of
 * thj_segjuncs_run*_async and thj_span_run*_async) runs on two side streams of the context's own, made at the first such
 * call and chosen by a ~2 ms measurement so that they do not share a hardware queue with `stream` or each other (HIP maps
 * streams to GPU_MAX_HW_QUEUES queues round robin); every call returns with its work joined on `stream` again. */
int  thj_ctx_create(int device, void* stream, thj_ctx** out);
/* Loads the kernels of the named parts now (an empty launch from each translation unit) instead of at their first use; blocks
 * until they are there.  For a process that has something else to do meanwhile.  No effect on results. */
#define THJ_WARM_SEGJUNCS 1   /* stage 1, event sets, juncs_db gather, exchange */
#define THJ_WARM_SPAN     2   /* stage 2, junction consensus */
#define THJ_WARM_INGEST   4   /* BGZF inflate, BAM parse */
#define THJ_WARM_BAMOUT   8   /* BAM record encoding, DEFLATE */
int  thj_ctx_warm(thj_ctx* ctx, int parts);
/* The side streams in use and what the measurement found for each: independent[k] = 1 when side stream k was measured to run beside
 * `stream` and the side streams before it; ratio[k] = (a 150 us spin kernel on each of them at once) / (one alone): 1.0 beside each
 * other, 2.0 one hardware queue shared, 0 not made yet.  The measurement happens inside the first thj_segjuncs_run*_async /
 * thj_span_run*_async / thj_span_tier0_pair_async call that needs a side stream (and again when a pair call needs the second):
 * that call BLOCKS the host for the ~2 ms it takes (it synchronises `stream` and runs spin kernels on it), so `stream` must not be
 * under graph capture then -- call thj_ctx_probe_streams first in such a setting.  A stream that shares a queue is still used
 * (same results, the sides partly one after the other); a warning goes to stderr and independent[k] stays 0. */
int  thj_ctx_stream_info(thj_ctx* ctx, int32_t* n_side, int32_t* independent /*[3]*/, double* ratio /*[3]*/);
/* Makes and measures `need` (1 or 2) side streams now, blocking, instead of inside the first run call. */
int  thj_ctx_probe_streams(thj_ctx* ctx, int32_t need);
/* ABI revision of this header: bumped whenever an entry point's argument layout changes (2: thj_span_tier_counts writes 5 int64,
 * thj_profile_span 8 doubles).  A caller built against another revision must not call in. */
#define THJ_ABI_VERSION 2
int  thj_abi_version(void);
void thj_ctx_destroy(thj_ctx* ctx);
int  thj_ctx_sync(thj_ctx* ctx);            /* hipStreamSynchronize on the context stream */
void* thj_ctx_stream(thj_ctx* ctx);         /* the hipStream_t in use */

/* ------------------------------------------------------------- genome */
/* Replaces RefSequenceTable + get_seqs (bwt_map.h:579-788,
 * segment_juncs.cpp:64-88): the whole reference as one HBM-resident array of
 * 32-byte blocks of 64 bases {lo bit-plane, hi bit-plane, N-mask, 0}; A=00 C=01
 * G=10 T=11, N has lo=hi=0 and its N-mask bit set, so dropping the mask gives the
 * Dna5->Dna "N becomes A" view the window copies use (segment_juncs.cpp:2157)
 * and keeping it gives the Dna5 view (:2417, long_spanning_reads.cpp:1146).
 * Contig i (ref_id i+1) starts at block contig_blk[i]; one zero guard block
 * follows every contig.  lens[i] == 0 marks an @SQ entry with no FASTA record
 * (rt.get_seq() == NULL, segment_juncs.cpp:2105-2108). */

/* Number of 32-byte blocks the packed genome needs. */
int thj_genome_layout(int32_t n_contigs, const int64_t* lens, uint32_t* contig_blk /*[n_contigs+1]*/,
                      int64_t* n_blocks);
/* Packs ASCII contigs (acgtACGT, anything else = N; seqs[i] may be NULL when
 * lens[i]==0) into `blocks` (4*n_blocks uint64, host memory). */
int thj_genome_pack(int32_t n_contigs, const char* const* seqs, const int64_t* lens,
                    const uint32_t* contig_blk, uint64_t* blocks, int64_t n_blocks);
/* Copies a packed genome to the device (H2D) and keeps it resident. */
int thj_genome_upload(thj_ctx* ctx, const uint64_t* blocks, int64_t n_blocks,
                      const uint32_t* contig_blk, const int64_t* lens, int32_t n_contigs);
/* Adopts an already device-resident packed genome (DEVICE pointer `d_blocks`,
 * not owned); contig_blk/lens are host arrays. */
int thj_genome_adopt(thj_ctx* ctx, const void* d_blocks, int64_t n_blocks,
                     const uint32_t* contig_blk, const int64_t* lens, int32_t n_contigs);

/* -------------------------------------------------------------- reads */
/* Replaces ReadStream::getRead's product (reads.cpp:528-630): read r becomes
 * 3*W uint64 {lo[W], hi[W], N[W]} bit-planes (base i = bit i%64 of word i/64)
 * plus its length.  Characters other than ACGT are N. */
int thj_reads_pack(int64_t n_reads, const int64_t* read_off, const char* bases,
                   int32_t words_per_plane, uint64_t* planes /*[n*3*W]*/, uint16_t* lens /*[n]*/);

/* ------------------------------------------------ segment_juncs batch */
/* The hits_for_read vectors that look_for_hit_group / process_next_hit_group
 * (segment_juncs.cpp:3823-4123) hand to the finders, for reads in visiting
 * (increasing id) order.  All array pointers are DEVICE pointers. */
typedef struct {
    int32_t n_reads;
    int32_t nseg;                /* number of segment maps (hits_for_read.size()): 1..16 */
    int32_t words_per_plane;     /* W of thj_reads_pack: 1..8 (reads of up to 512 bases) */
    int32_t reserved;
    const uint32_t* seg_off;     /* [n_reads*nseg+1] CSR into hits, index r*nseg+s */
    const thj_hit*  hits;
    const uint64_t* read_planes; /* [n_reads*3*W] */
    const uint16_t* read_len;    /* [n_reads] */
    const uint32_t* mate_off;    /* [n_reads+1] CSR into mate_hits, or NULL: no mates */
    const thj_hit*  mate_hits;   /* partner_hit_group of find_gaps (segment_juncs.cpp:3321-3348) */
    uint32_t ordinal_base;       /* visiting ordinal of read 0 (first-inserted-wins priority of
                                    std::set<Insertion>, insertions.h:52-67) */
    uint32_t reserved2;
} thj_seg_batch;

/* Convenience: allocates device memory for a batch given HOST arrays, copies
 * (H2D, on the context stream) and returns a device-resident descriptor that
 * thj_batch_free releases.  n_hits / n_mate_hits are the CSR totals. */
int thj_batch_upload(thj_ctx* ctx, const thj_seg_batch* host, int64_t n_hits, int64_t n_mate_hits,
                     thj_seg_batch** out);
int thj_batch_free(thj_ctx* ctx, thj_seg_batch* dev);

/* Capacity (entries, rounded up to a power of two) of the device event tables;
 * default 1<<24 junctions, 1<<20 each for deletions and insertions.  Resets. */
int thj_segjuncs_configure(thj_ctx* ctx, int64_t junc_capacity, int64_t indel_capacity);
/* Empties the event tables (start of a segment_juncs run). */
int thj_segjuncs_reset_async(thj_ctx* ctx);
/* find_insertions_and_deletions + find_gaps + juncs_from_ref_segs<RecordSegmentJuncs>
 * x {GT-AG, GC-AG, AT-AC} (segment_juncs.cpp:2807-2942, :3293-3650, :2052-2377)
 * for every read of the batch; events accumulate in the context's tables the
 * way the reference accumulates into its std::sets (:4911-4916). */
int thj_segjuncs_run_async(thj_ctx* ctx, const thj_params* p, const thj_seg_batch* dev_batch);
/* Two batches (the two sides of a pass: find_gaps over left_segmap_fnames, then over right_segmap_fnames,
 * segment_juncs.cpp:4911-4916) as one call.  The events are those of two thj_segjuncs_run_async calls in this
 * order; the second batch's kernels do not wait for the first batch's side chains. */
int thj_segjuncs_run_pair_async(thj_ctx* ctx, const thj_params* p0, const thj_seg_batch* dev_batch0,
                                const thj_params* p1, const thj_seg_batch* dev_batch1);

typedef struct { uint32_t ref_id, left, right, antisense; } thj_junction;   /* junctions.h:27-57 */
typedef struct { uint32_t ref_id, left; char seq[8]; uint64_t prio; } thj_insertion; /* insertions.h:31-67 */

typedef struct {
    int64_t n_juncs, n_deletions, n_insertions;
    int64_t n_windows;        /* RefSeg windows scanned */
    int64_t n_indel_pairs;    /* hit pairs sent to detect_small_insertion/deletion */
    int64_t n_rescue_pairs;   /* (hit, mate hit) pairs scanned by map_read_to_contig */
    int64_t n_overflow_blocks;/* workgroups that fell back to un-queued processing */
    int64_t n_hits_read;      /* thj_hit records the kernels were handed */
} thj_segjuncs_counts;

/* Compacts + sorts the tables into the order of the reference's sets
 * (junctions.h:39-57; insertions.h:52-67) and synchronises the stream.
 * Returns THJ_EOVERFLOW if a table overflowed during the runs. */
int thj_segjuncs_finish(thj_ctx* ctx, thj_segjuncs_counts* counts);
/* Copies the sorted events to host arrays sized from thj_segjuncs_finish's counts. */
int thj_segjuncs_download(thj_ctx* ctx, thj_junction* juncs, thj_junction* deletions, thj_insertion* insertions);
/* DEVICE pointers to the sorted packed 64-bit event keys after finish (for
 * on-device merging / RCCL all-gather): kind 0 junctions, 1 deletions. */
int thj_segjuncs_device_keys(thj_ctx* ctx, int kind, const uint64_t** d_keys, int64_t* n);
/* Inserts packed keys (DEVICE pointer) produced by another context/rank into this
 * context's table: the merge step of segment_juncs.cpp:4911-4916 across GPUs.
 * Precondition: the keys were made on a context holding the SAME genome layout (their position field lies below this
 * genome's n_blocks * 64 + 2): thj_segjuncs_finish sorts the event lists on as many key bits as this genome's positions
 * need, and a key beyond them would be mis-sorted silently. */
int thj_segjuncs_merge_keys_async(thj_ctx* ctx, int kind, const uint64_t* d_keys, int64_t n);

/* The sorted insertion table after finish: packed keys and values (value = first-wins
 * priority << 20 | bases), DEVICE pointers; and its merge counterpart (atomicMin on the
 * value = "earlier insertion wins", insertions.h:52-67 + std::set::insert). */
int thj_segjuncs_device_insertions(thj_ctx* ctx, const uint64_t** d_keys, const uint64_t** d_vals, int64_t* n);
int thj_segjuncs_merge_insertions_async(thj_ctx* ctx, const uint64_t* d_keys, const uint64_t* d_vals, int64_t n);

/* ------------------------------------------------ fusion search (--fusion-search) */
typedef struct { uint32_t ref_id1, ref_id2, left, right, dir, count, edit_dist, reserved; } thj_fusion;   /* fusions.h:24-116 */
#define THJ_FUSION_FF 7u
#define THJ_FUSION_FR 8u
#define THJ_FUSION_RF 9u
#define THJ_FUSION_RR 10u
/* find_fusions + detect_fusion (segment_juncs.cpp:2976-3291, :2629-2805) for every read of the batch -- which for
 * this call must hold ALL visited reads, including those whose only mapped segment is the first
 * (:3994-4028).  Candidate events accumulate on the device. */
int thj_fusion_reset_async(thj_ctx* ctx);
/* --fusion-ignore-chromosomes (segment_juncs.cpp:3214-3231): hit pairs touching one of these contigs (1-based ref ids)
 * are not examined.  Stays in force until called again (n = 0 clears). */
int thj_fusion_set_ignored(thj_ctx* ctx, const uint32_t* ref_ids, int32_t n);
int thj_fusion_run_async(thj_ctx* ctx, const thj_params* p, const thj_seg_batch* dev_batch);
/* Synchronises and reduces the events to the FusionSimpleSet (count, smallest edit distance) in
 * Fusion::operator< order (fusions.h:38-69).  THJ_ERETRY: a batch had more raw candidates than the buffer held (it grows between batches,
 * ahead of the count); the buffer now has the room the count asked for: thj_fusion_reset_async, the run calls and this again. */
int thj_fusion_finish(thj_ctx* ctx, int64_t* n_fusions);
int thj_fusion_download(thj_ctx* ctx, thj_fusion* out);

/* Average durations (ms) of the kernels of a run, measured with HIP events on the stream each runs on (the reads
 * with several hits a segment have streams of their own beside the flat reads' kernels), over the runs since the
 * last call (a pair call counts as two).  avg_ms[8]: `thj_k_sj_flat`; `thj_k_sj_general`, first instance; second
 * instance; `thj_k_segjuncs_shared`; `thj_k_segjuncs_rescue` + `_rescue_shared`; `thj_k_sj_tasks_list`;
 * `thj_k_sj_rescue_flat` (one kernel since round 16; the tools that name the slot still call it `thj_k_sj_rescue_scan` +
 * `thj_k_sj_rescue_flat`); `thj_k_sj_tasks`.  stats[4] (may be null), averages over the
 * launches whose lists are still there: reads given to `thj_k_segjuncs_shared`, to the second instance of
 * `thj_k_sj_general`, tasks `thj_k_sj_tasks_list` ran, flat rescue pairs.  Enables event recording when `enable` != 0. */
int thj_profile_segjuncs(thj_ctx* ctx, int enable, double* avg_ms, int64_t* launches, double* stats);
/* Measurement aid: with `on` != 0 the stage calls of this context launch every kernel on the context's stream, one after the
 * other (no side streams) -- the durations thj_profile_segjuncs / thj_profile_span then report are each kernel's own, not those of
 * kernels sharing the GPU.  Results are the same either way.  Default 0. */
int thj_profile_serial(thj_ctx* ctx, int on);


/* --------------------------------------------------- juncs_db
 * The step between the two executables (juncs_db.cpp:73-233): FASTA records of the sequence around every junction /
 * deletion / insertion / fusion, cut from the genome.  The resident bit-plane genome makes this a gather: the caller
 * lists the pieces it wants, the device writes their bases as ASCII (A C G T N; reverse-complemented when asked, N
 * stays N) at the byte offsets given, and the caller interleaves its header lines. */
typedef struct thj_piece {
    uint32_t ref_id;      /* 1-based */
    int32_t  start;       /* 0-based first base */
    int32_t  len;         /* bases; the piece must lie inside the contig */
    uint32_t flags;       /* THJ_PIECE_RC */
} thj_piece;
#define THJ_PIECE_RC 1u
/* HOST arrays in, HOST bytes out: out[out_off[i] .. out_off[i] + pieces[i].len) receives piece i.  Synchronous. */
int thj_genome_gather(thj_ctx* ctx, const thj_piece* pieces, int64_t n, const int64_t* out_off, char* out, int64_t out_bytes);

/* --------------------------------------------------- long_spanning_reads */

/* CigarOpCode values of bwt_map.h:36-55, packed as (op << 28) | length. */
#define THJ_CIG_MATCH     1u
#define THJ_CIG_INS       3u
#define THJ_CIG_DEL       5u
#define THJ_CIG_REF_SKIP 11u
#define THJ_CIG_SOFT_CLIP 13u
/* --fusion-search: the lower-case (running down the genome) forms and the four fusion ops, whose length is the 0-based
 * position on the second contig (bwt_map.h:36-55; print_bamhit writes them as m / i / d / n and <pos + 1>F) */
#define THJ_CIG_mATCH     2u
#define THJ_CIG_iNS       4u
#define THJ_CIG_dEL       6u
#define THJ_CIG_FUSION_FF 7u
#define THJ_CIG_FUSION_FR 8u
#define THJ_CIG_FUSION_RF 9u
#define THJ_CIG_FUSION_RR 10u
#define THJ_CIG_rEF_SKIP 12u

/* A segment alignment with its CIGAR: BowtieHit as produced by BAMHitFactory /
 * SplicedBAMHitFactory (bwt_map.cpp:1101-1452, :1469-1770). 32 bytes. */
typedef struct {
    uint32_t ref_id;
    int32_t  left;
    uint8_t  flags;        /* THJ_HIT_ANTISENSE | THJ_HIT_END | THJ_HIT_ANTISENSE_SPLICE */
    uint8_t  mismatches;
    uint8_t  edit_dist;
    uint8_t  n_cigar;      /* 1..5 */
    uint32_t cigar[5];
} thj_span_hit;
#define THJ_HIT_ANTISENSE_SPLICE 4u
/* A segment hit on a fusion contig of the junction database (SplicedBAMHitFactory, bwt_map.cpp:1655-1760) has a fusion op in
 * its cigar, at most 4 ops, and its second contig (ref_id2) in cigar[4].  On rf / rr contigs antisense_align is the opposite
 * of the record's strand flag (:1744-1745): THJ_HIT_STRAND_FLIPPED says so, i.e. the record's SEQ is the read piece
 * reverse-complemented iff THJ_HIT_ANTISENSE xor THJ_HIT_STRAND_FLIPPED. */
#define THJ_HIT_STRAND_FLIPPED 8u
#define THJ_HIT_FUSED 16u          /* the hit's cigar holds a fusion op (set by whoever builds the record; the stitch kernels route on it) */

/* Per-read segment hit lists of JoinSegmentsWorker (long_spanning_reads.cpp:2669-2845):
 * for every read with a hit in the first segment map, segment s holds the contig
 * hits then the spliced hits (:2706-2765, :87-163).  DEVICE pointers. */
typedef struct {
    int32_t n_reads;
    int32_t nseg;
    int32_t words_per_plane;
    int32_t qual_stride;         /* bytes between consecutive reads' quality strings */
    const uint32_t*     seg_off;     /* [n_reads*nseg+1] */
    const thj_span_hit* hits;
    const uint64_t*     read_planes; /* [n_reads*3*W] (thj_reads_pack) */
    const uint16_t*     read_len;
    const uint8_t*      quals;       /* phred+33, qual_stride bytes per read */
    const void*         hit_heads;   /* the first 16 bytes of every hit record, densely (contig, position, flags, first cigar op: all
                                      * the first stitch tier reads of a hit, so it streams 16 B per hit).  Every batch this library
                                      * makes has one -- thj_span_batch_upload derives it once at upload, the device-side ingest
                                      * writes it beside the records; NULL is accepted from other producers (the tier then reads
                                      * the 32-byte records) */
} thj_span_batch;

/* One output record: the fields print_bamhit + bowtie_sam_extra write
 * (bwt_map.cpp:1888-2093, :2467-2648). 128 bytes. */
typedef struct {
    uint32_t read_idx;     /* index of the read in its batch */
    uint32_t ref_id;
    int32_t  left;         /* POS - 1 */
    uint8_t  flags;        /* THJ_HIT_ANTISENSE (-> FLAG 0x10) | THJ_HIT_ANTISENSE_SPLICE (-> XS:A:-) */
    uint8_t  mismatches;   /* NM = mismatches + indel lengths */
    uint8_t  edit_dist;
    uint8_t  n_cigar;
    int16_t  AS;
    uint8_t  XM, XO, XG, md_len;
    uint16_t order;        /* rank among the read's records (BowtieHit::operator<, bwt_map.h:180-207) */
    uint32_t cigar[16];    /* a fusion alignment (one of its ops is THJ_CIG_FUSION_*) has at most 15 ops and its second contig,
                              ref_id2, in cigar[15] */
    char     md[40];       /* MD:Z value, md_len characters; md_len == THJ_MD_ON_HOST: longer than the record holds -- thj_md_string */
} thj_aln;
#define THJ_MD_ON_HOST 255
/* MD:Z of one alignment as bowtie_sam_extra writes it (bwt_map.cpp:2467-2648), on the host: ref = the contig's bases (any
 * case, non-ACGT = N), seq = the read bases in the orientation of the alignment, cigar = op << 28 | length.  Writes a
 * NUL-terminated string, returns its length (< 0: error).  For the records the device flags with THJ_MD_ON_HOST. */
int thj_md_string(const char* ref, int64_t ref_len, const char* seq, int32_t seq_len, int32_t left, const uint32_t* cigar, int32_t n_cigar,
                  char* out, int32_t out_cap);
/* The same for an alignment that may run down the genome (lower-case ops) and change contigs at a fusion op: ref2 = the
 * second contig (= ref for a plain alignment). */
int thj_md_string2(const char* ref, int64_t ref_len, const char* ref2, int64_t ref2_len, const char* seq, int32_t seq_len, int32_t left,
                   const uint32_t* cigar, int32_t n_cigar, char* out, int32_t out_cap);

/* The junction (+deletion) and insertion sets long_spanning_reads loads from its list
 * files (long_spanning_reads.cpp:2897-2980).  juncs: sorted unique in Junction::operator<
 * order, deletions already merged in as Junction(left, right, '+'); insertions: n_ins rows
 * of 4 uint32 {ref_id, left, length, bases 3 bits each (A,C,G,T,N = 0..4)} sorted by
 * (ref_id, left, length).  HOST pointers. */
int thj_span_sets_upload(thj_ctx* ctx, const thj_junction* juncs, int64_t n_juncs, const uint32_t* insertions, int64_t n_ins);
/* Same, taken device-to-device from the context's own finished segment_juncs tables. */
int thj_span_sets_from_segjuncs(thj_ctx* ctx);
/* The same for --fusion-search: the fusion list thj_fusion_finish left in this context (segment_juncs' .fusions output, what
 * long_spanning_reads reads back with --fusion-search) becomes the spanning stage's list without leaving the device.  Replaces
 * thj_fusion_download + thj_span_fusions_upload when both stages run in one process. */
int thj_span_fusions_from_segjuncs(thj_ctx* ctx);

/* --fusion-search: the .fusions list long_spanning_reads loads (long_spanning_reads.cpp:2998-3040), sorted unique in
 * Fusion::operator< order (fusions.h:44-71); dir = THJ_CIG_FUSION_*.  HOST pointer.  thj_span_run_async consults it when
 * thj_params.fusion_search is set; the reads that are not plain runs of abutting single hits then go through the fusion
 * branches of dfs_seg_hits / merge_chain (:2222-2610, :805-2038) in thj_k_stitch_fusion. */
typedef struct { uint32_t ref_id1, ref_id2, left, right, dir; } thj_span_fusion;
int thj_span_fusions_upload(thj_ctx* ctx, const thj_span_fusion* fusions, int64_t n);

int thj_span_batch_upload(thj_ctx* ctx, const thj_span_batch* host, int64_t n_hits, thj_span_batch** out);
int thj_span_batch_free(thj_ctx* ctx, thj_span_batch* dev);
/* d_heads[i] = first 16 bytes of d_hits[i] (device buffers, n_hits * 16 bytes out): the optional hit_heads array of a batch */
int thj_span_hit_heads_async(thj_ctx* ctx, const thj_span_hit* d_hits, int64_t n_hits, void* d_heads);

int thj_span_reset_async(thj_ctx* ctx);
/* join_segments_for_read + sort/unique + filters + bowtie_sam_extra for every read of the
 * batch (long_spanning_reads.cpp:2612-2667, :2767-2831); records accumulate in HBM. */
int thj_span_run_async(thj_ctx* ctx, const thj_params* p, const thj_span_batch* dev_batch);
/* Two batches -- the left and the right reads of a pass, or two shards of one side -- as one call: the same records in the same
 * slots as thj_span_run_async(batch0) followed by thj_span_run_async(batch1), with the kernels of the two batches running beside
 * each other on streams of the context's own (the latency-bound kernels of one batch overlap the bandwidth-bound ones of the
 * other).  Joined on the context's stream before it returns. */
int thj_span_run_pair_async(thj_ctx* ctx, const thj_params* p, const thj_span_batch* dev_batch0, const thj_span_batch* dev_batch1);
/* Optional, before thj_span_run_pair_async on the same two batches (after thj_span_reset_async): the part of the pair's work
 * that needs the batches and nothing else -- the reads whose segment hits abut end to end, two thirds of all -- is enqueued
 * now; the run then only does what is behind it.  Stage 2's junction / indel sets need not exist yet: a caller that holds both
 * stages resident calls this before thj_segjuncs_finish, and the GPU has that work while the host waits for stage 1's counts
 * and the event lists are sorted.  Same records as without the call.  Does nothing (the run does everything) for an empty
 * batch, under --fusion-search or THJ_SPAN_SERIAL.  THJ_ESTATE when anything but that run follows. */
int thj_span_tier0_pair_async(thj_ctx* ctx, const thj_params* p, const thj_span_batch* dev_batch0, const thj_span_batch* dev_batch1);
/* Synchronises and returns the record count.  THJ_EOVERFLOW when a device limit was hit (message says which); THJ_ERETRY when
 * a pool or workspace had to be enlarged (extra records of multihit reads; reads with more joined alignments than a thread keeps):
 * run the pass again.
 * On the device the records sit in BAM order already: one slot per read of the pass (run order, then read order)
 * holding the read's first record, a per-read count, and the few extra records of multihit reads keyed by
 * (slot << 16 | rank) -- rank = BowtieHit::operator< order inside the read (bwt_map.h:180-207). */
int thj_span_finish(thj_ctx* ctx, int64_t* n_alns);
/* Compact ordered host copy of the n_alns records. */
int thj_span_download(thj_ctx* ctx, thj_aln* out);
/* A record as the stitch kernels leave it in HBM: the same 128 bytes as thj_aln in two 64-byte lines, ordered so that an
 * ordinary alignment needs only the first.  The lead line: the 24-byte header of thj_aln, cigar ops 0..3, MD characters 0..23.
 * The tail line: cigar ops 4..15, MD characters 24..39 -- written, and THJ_SLOT_TAIL set in `flags`, only for a record with more
 * than four cigar ops, an MD string of more than 24 characters, or a fusion alignment; otherwise its bytes are undefined
 * (left over from an earlier pass) and the fields it would hold are zero.  thj_span_download converts to thj_aln. */
typedef struct {
    uint32_t read_idx, ref_id; int32_t left;
    uint8_t  flags, mismatches, edit_dist, n_cigar;
    int16_t  AS; uint8_t XM, XO, XG, md_len; uint16_t order;
    uint32_t cigar_lo[4];  char md_lo[24];     /* lead line ends here (64 bytes) */
    uint32_t cigar_hi[12]; char md_hi[16];     /* tail line: valid only with THJ_SLOT_TAIL */
} thj_aln_slot;
#define THJ_SLOT_TAIL 0x80u
/* The device-resident layout described above (DEVICE pointers), for consumers that stay on the GPU. */
int thj_span_device_records(thj_ctx* ctx, const thj_aln_slot** d_slots, const uint8_t** d_counts, int64_t* n_reads,
                            const thj_aln_slot** d_extra, const uint64_t** d_extra_keys, int64_t* n_extra);
/* Of the batch launched last: counts[0] = reads sent to the closure kernels (as chain entries to thj_k_join / thj_k_finish, or to
 * thj_k_stitch), counts[1] = to the multihit kernel thj_k_stitch_pack, counts[2] = on to the general kernel thj_k_stitch_generic,
 * counts[3] = those of counts[0] that travelled as chain entries, counts[4] = those of counts[1] whose chains thj_k_chains turned into
 * chain entries (joined and finished by thj_k_join / thj_k_finish instead of the packed tier); the rest were finished by
 * thj_k_stitch_contig. */
int thj_span_tier_counts(thj_ctx* ctx, int64_t* counts /*[5]*/);
/* Average durations (ms) of the stitch kernels since the last call -- avg_ms[0] thj_k_stitch_contig, [1] thj_k_chains, [2] thj_k_join,
 * [3] thj_k_join_closure, [4] thj_k_finish, [5] thj_k_stitch, [6] thj_k_stitch_pack, [7] thj_k_stitch_generic or, with --fusion-search,
 * thj_k_stitch_fusion -- from HIP events on the stream each runs on (kernels of batches that run beside each other share the GPU:
 * their durations overlap). */
int thj_profile_span(thj_ctx* ctx, int enable, double* avg_ms /*[8]*/, int64_t* launches);

/* ---- coverage search of segment_juncs (segment_juncs.cpp:4268-4543 capture_island_ends and what it calls: the
 * coverage map of build_coverage_map :4140-4176, the extension table of index_read_mers :548-571,
 * juncs_from_ref_segs<RecordExtendableJuncs> :2052-2377 with RecordExtendableJuncs::record :1568-1626).
 * Call order inside one segment_juncs pass: thj_covsearch_reset_async; thj_covsearch_add_hits_async for every uploaded
 * batch of both sides (the segment maps `all_segmap_fnames`, :4929-4935); thj_covsearch_add_reads for the initially
 * unmapped reads (--ium-reads; planes in the thj_reads_pack layout and lengths, host buffers or -- on_device != 0 -- device
 * buffers; only the first 32 bases of a read are used, :425); thj_covsearch_run_async finds the junctions; thj_covsearch_finish adds them to
 * the pass's junction set -- all of them, or, when there are more than max_cov_juncs (:56), the max_cov_juncs smallest by
 * (skip count, junction) as the reference's capped set keeps them (:1611-1621) -- and returns how many; it goes before
 * thj_segjuncs_finish. */
int thj_covsearch_reset_async(thj_ctx* ctx);
int thj_covsearch_add_hits_async(thj_ctx* ctx, const thj_seg_batch* device_batch);
int thj_covsearch_add_reads(thj_ctx* ctx, int64_t n_reads, int32_t words_per_plane, const uint64_t* planes, const uint16_t* lens,
                            int32_t on_device);
/* The same for a piece (whole BGZF members; thj_bam_piece below) of an UNALIGNED BAM of reads -- what tophat.py passes as --ium-reads --:
 * inflated and parsed on the device (thj_bgzf_inflate's kernels, the record walk of the ingest), every record a read
 * (ReadStream::get_direct).  *n_reads = records taken.  THJ_EFALLBACK as for thj_ingest_*: read the piece on the host.  Synchronous. */
/* Room for n_reads more unmapped reads in the extension table now (a caller that knows roughly how many are coming: the table otherwise
 * grows by half whenever it is full, each time a copy of what it holds). */
int thj_covsearch_reserve_reads(thj_ctx* ctx, int64_t n_reads);
struct thj_bam_piece;
int thj_covsearch_add_reads_bam(thj_ctx* ctx, const struct thj_bam_piece* reads, int64_t* n_reads);
int thj_covsearch_run_async(thj_ctx* ctx, int32_t min_cov_length, int32_t min_coverage_intron, int32_t max_coverage_intron);
int thj_covsearch_finish(thj_ctx* ctx, int64_t max_cov_juncs, int64_t* n_found);
/* Butterfly search (--butterfly-search; replaces prune_extension_table + compact_extension_table + pair_covered_sites with
 * juncs_from_ref_segs<RecordButterflyJuncs>, segment_juncs.cpp:466-501, :4178-4249, :1698-2049): works from the same state as the
 * coverage search -- the coverage map of thj_covsearch_add_hits_async and the extension table of thj_covsearch_add_reads (after
 * thj_covsearch_allgather when ranks share the reads); neither is changed.  Every island of the coverage map, widened by 45 bases,
 * is searched for GT / CT and AG / AC; a donor and an acceptor min..max_coverage_intron apart make a junction when an unmapped read's
 * seed next to the one and a seed next to the other show the same twelve bases across the gap.  The junctions -- all, or the
 * max_cov_juncs with the shortest introns (the capped set of :2031-2041) -- are added to the pass's junction set; *n_found = their
 * number.  Synchronous.  Run it after thj_covsearch_finish (when the coverage search runs at all: they share buffers) and before
 * thj_segjuncs_finish. */
int thj_butterfly_run(thj_ctx* ctx, int32_t min_coverage_intron, int32_t max_coverage_intron, int64_t max_cov_juncs, int64_t* n_found);
/* Microexon search (segment_juncs.cpp:3737-3941; replaces align_microexon_segs and the window registration inside look_for_hit_group).
 * A read whose first segment has no hit while every other segment has some may begin in a microexon: every hit of its second segment
 * registers a window of 2000 bases beside it with the read's first segment_length bases.  thj_microexon_collect finds those
 * candidates on the device for an uploaded / ingested batch (read_side 1 = left, 2 = right; ordinals = the batch's ordinal_base + row);
 * thj_microexon_candidates hands all of them to the host (malloc'd: free()), which merges overlapping windows in the reference's
 * visiting order -- sequential std::map logic, csrc/host/thj_mx_host.h; thj_microexon_run then builds every window's own extension
 * table, pairs the GT / CT sites of a window with its AG / AC sites (one wave per window), applies the max_cov_juncs cut
 * (segment_juncs.cpp:5021-5024) and adds the junctions to the pass's set.  Run it after thj_covsearch_finish (they share buffers).
 * str = the 2-bit string, first base most significant; strings of a window in the order the reference pooled them (the table is a set:
 * the order does not matter).  segment_length 10..32. */
typedef struct { uint32_t ordinal; uint16_t rank; uint8_t side, len; uint32_t ref_id; int32_t left, right; uint32_t reserved; uint64_t str; } thj_mx_cand;
typedef struct { uint32_t ref_id; int32_t left, right; int32_t side; } thj_mx_window;
int thj_microexon_reset_async(thj_ctx* ctx);
int thj_microexon_collect(thj_ctx* ctx, const thj_params* p, const thj_seg_batch* device_batch, int32_t read_side);
int thj_microexon_candidates(thj_ctx* ctx, thj_mx_cand** out, int64_t* n);
int thj_microexon_run(thj_ctx* ctx, const thj_mx_window* windows, int64_t n_windows, const uint64_t* strs, const uint8_t* str_len, const uint32_t* str_window,
                      int64_t n_strs, int32_t min_coverage_intron, int32_t library_type, int64_t max_cov_juncs, int64_t* n_found);

/* Reads sharded over GPUs: the coverage map of the whole run is the OR of the ranks' maps and the
 * extension table that of all their unmapped reads.  thj_covsearch_device_state exposes a rank's state (device
 * pointers: n_words coverage words, one size per contig, n_ext read records -- d_ext_keys[i] = min(length, 32) of read i,
 * d_ext_vals[i] = its first 32 bases as a 2-bit string, first base most significant: the table's entries are made from the
 * records when a pass builds the table) for the caller to all-gather;
 * thj_covsearch_merge_async folds another rank's state in; then every rank runs thj_covsearch_run_async. */
int thj_covsearch_device_state(thj_ctx* ctx, const uint64_t** d_cov_bits, int64_t* n_words, const int32_t** d_cov_size,
                               const uint32_t** d_ext_keys, const uint64_t** d_ext_vals, int64_t* n_ext);
int thj_covsearch_merge_async(thj_ctx* ctx, const uint64_t* d_other_bits, const int32_t* d_other_size,
                              const uint32_t* d_other_keys, const uint64_t* d_other_vals, int64_t n_other_ext);

/* ---------------------------------------------------------------- device-side ingest
 * BGZF members (samtools-0.1.18 bgzf.c) are independent DEFLATE streams of at most 64 KiB; thj_bgzf_inflate inflates many of
 * them at once on the GPU (one workgroup per member, tables and window in LDS).  in_off / in_len address a member's DEFLATE
 * payload (after its 18-byte header, before the 8-byte CRC32 / ISIZE trailer) inside `comp`.  Member b's bytes land at
 * out + b * 65536, out_len[b] = their number (0xFFFFFFFF: corrupt stream).  on_device == 0: host arrays, synchronous;
 * != 0: device arrays, the call only enqueues on the context stream. */
typedef struct { uint64_t in_off; uint32_t in_len; uint32_t reserved; } thj_bgzf_block;
int thj_bgzf_inflate(thj_ctx* ctx, const uint8_t* comp, int64_t comp_bytes, const thj_bgzf_block* blocks, int64_t n_blocks,
                     uint8_t* out, uint32_t* out_len, int32_t on_device);

/* One input file's share of a read-id shard, still compressed: `comp` = comp_bytes bytes of the BAM file starting at a BGZF member
 * (HOST memory, e.g. a mapping of the file) and ending at a member boundary; first_skip = bytes of the first member that come
 * before the shard's first record (the low 16 bits of the .index offset, or the end of the BAM header); tid2ref[t] = ref_id of
 * the file's target t (0: a contig the run does not know). */
typedef struct thj_bam_piece { const uint8_t* comp; int64_t comp_bytes; uint32_t first_skip; int32_t n_tid; const uint32_t* tid2ref; } thj_bam_piece;
/* The whole ingest of one shard of one side of segment_juncs on the device: inflates the pieces, parses their records
 * (BAMHitFactory::get_hit_from_buf, bwt_map.cpp:1101-1452; reads: SEQ -> bit planes), keeps read ids in [begin_id, end_id),
 * merges the nseg segment maps by read id into the visiting set of look_for_hit_group (segment_juncs.cpp:3823-4123; reads whose
 * highest mapped segment is the first are left out unless include_top0), joins the mate's hits (whole-read map, else last
 * segment map: find_gaps :3321-3348) and the reads, and returns a device-resident batch for thj_segjuncs_run_async /
 * thj_fusion_run_async / thj_covsearch_add_hits_async (thj_batch_free releases it).  *out == NULL with THJ_OK: the shard is
 * empty.  THJ_EFALLBACK: see above.  mate_full / mate_last may be NULL.  Synchronous. */
/* THJ_INGEST_TIMING=1 in the environment: the ingest calls time their phases (with a stream synchronisation at every mark: a
 * diagnosis mode), this prints the sums to stderr. */
void thj_ingest_timing_report(void);
int thj_ingest_seg_batch(thj_ctx* ctx, const thj_params* p, int32_t nseg, const thj_bam_piece* segs, const thj_bam_piece* mate_full,
                         const thj_bam_piece* mate_last, const thj_bam_piece* reads, uint32_t begin_id, uint32_t end_id, int32_t include_top0,
                         uint32_t ordinal_base, thj_seg_batch** out, int64_t* n_reads);

/* long_spanning_reads: the contig segment maps of one shard on the device -> a batch whose per-(read, segment) hit lists are
 * set, for the reads with a hit in the FIRST segment map (the groups JoinSegmentsWorker iterates over,
 * long_spanning_reads.cpp:2706-2765).  *row_ids (HOST, malloc'd: free() it) = their read ids in row order; the caller fetches
 * those reads -- it needs names, bases and qualities for the BAM records anyway -- and completes the batch with
 * thj_span_batch_attach_reads (HOST arrays in the layouts of thj_reads_pack / thj_span_batch) before thj_span_run_async.
 * thj_span_batch_free releases the batch.  *out == NULL with THJ_OK: nothing to do in this shard. */
int thj_ingest_span_hits(thj_ctx* ctx, const thj_params* p, int32_t nseg, const thj_bam_piece* segs, uint32_t begin_id, uint32_t end_id,
                         thj_span_batch** out, uint32_t** row_ids, int64_t* n_rows);
/* The same with the shard's piece of the READS file (unaligned BAM, id-sorted) riding along: its members are inflated and its
 * records located with the maps', the batch leaves complete (read planes, lengths and quality strings written on the device:
 * no thj_span_batch_attach_reads), and the inflated read records come back for the BAM output -- *reads_infl (HOST, page-locked,
 * from thj_pinned_alloc: thj_pinned_free() it): reads_infl_bytes bytes, BGZF member m of the piece at m << 16; row_loc[r] (HOST, malloc'd) = (m << 16 | offset)
 * of the block_size field of row r's record.  Replaces ReadStream::getRead per row (reads.cpp:528-630). */
/* Page-locked host buffers from a pool of the process (locking pages is slow, copies from and to them are plain DMA): for what a
 * caller hands to thj_ingest_* (thj_bam_piece.comp may point into one) and for what thj_ingest_span_batch hands back. */
void* thj_pinned_alloc(size_t bytes);
void thj_pinned_free(void* p);
/* From now on buffers are unlocked and released when they are handed back (and the idle ones at once) instead of kept for the next
 * caller: a process calls this when it has started its last piece of work, so that taking its page-locked memory apart (0.11 s per
 * GB on this driver) runs beside that work and not after the process's last instruction. */
void thj_pinned_drain(void);
int thj_ingest_span_batch(thj_ctx* ctx, const thj_params* p, int32_t nseg, const thj_bam_piece* segs, const thj_bam_piece* reads,
                          uint32_t begin_id, uint32_t end_id, thj_span_batch** out, uint32_t** row_ids, int64_t* n_rows,
                          uint8_t** reads_infl, int64_t* reads_infl_bytes, uint32_t** row_loc);
/* ---- junction-db ("spliced") segment maps on the device (SplicedBAMHitFactory::get_hit_from_buf + spliceCigar + getBAMmismatches,
 * bwt_map.cpp:1469-1770, :681-883, :410-475).  A junction-db map's header names one target per junction / deletion / insertion /
 * fusion contig, `name|left|l-r|right|type|strand` (juncs_db.cpp:99, :143); the name is tokenised once per run into one of these.
 * ref_id = the genomic contig (0: one the run does not know -- its records are dropped), ref_id2 = the second contig of a fusion
 * contig (0 otherwise), left = where the contig window starts, lsp = the left splice position, second = the right splice position
 * (junction, deletion) or the number of inserted bases (insertion).  A name that does not parse (fewer than six fields, `l-r` not
 * two parts, an unknown strand word on anything but an insertion) is THJ_JUNCDB_INVALID: its records are dropped. */
typedef struct {
    uint32_t ref_id, ref_id2;
    int32_t  left, lsp, second;
    uint8_t  type;         /* THJ_JUNCDB_JUNC .. THJ_JUNCDB_INVALID */
    uint8_t  strand;       /* THJ_JUNCDB_FWD .. THJ_JUNCDB_OTHER */
    uint16_t reserved;
} thj_juncdb_target;
enum { THJ_JUNCDB_JUNC = 0, THJ_JUNCDB_DEL = 1, THJ_JUNCDB_INS = 2, THJ_JUNCDB_FUS = 3, THJ_JUNCDB_INVALID = 4 };
enum { THJ_JUNCDB_FWD = 0, THJ_JUNCDB_REV = 1, THJ_JUNCDB_FF = 2, THJ_JUNCDB_FR = 3, THJ_JUNCDB_RF = 4, THJ_JUNCDB_RR = 5, THJ_JUNCDB_OTHER = 6 };
/* The target table of the run's junction-db maps (HOST array, target t of their common header at [t]); it stays on the context
 * until the next upload -- a junction database has millions of targets, so it does not travel with every shard the way
 * thj_bam_piece.tid2ref does.  n == 0 takes the table away.  Synchronous. */
int thj_span_juncdb_upload(thj_ctx* ctx, const thj_juncdb_target* targets, int64_t n);
/* Fusion contigs (THJ_JUNCDB_FUS targets, bwt_map.cpp:1664-1759) on the device as well: on != 0 and their records become fused hits
 * (THJ_HIT_FUSED, the FUSION_xx operation in the cigar, the second contig in cigar[4], at most four operations) instead of sending
 * the shard back.  The switch belongs to the uploaded table: every thj_span_juncdb_upload turns it off, so every call sequence
 * without this call gives what it gave before.  THJ_ESTATE: no table.  A table without such a target is read by the same kernel
 * whatever the switch says. */
int thj_span_juncdb_fusion_contigs(thj_ctx* ctx, int32_t on);
/* thj_ingest_span_batch with the shard's pieces of the junction-db maps: spliced[s] (s < n_spliced <= nseg) belongs to segment s.
 * Cell (read, s) of the batch holds the contig map's hits, then the spliced map's, each in file order (long_spanning_reads.cpp:125-147,
 * :2738-2744); the rows are the reads with a hit in EITHER first-segment map.  n_spliced == 0: exactly thj_ingest_span_batch.
 * reads may be NULL (then as thj_ingest_span_hits).  THJ_ESTATE: n_spliced > 0 and no table uploaded.  THJ_EFALLBACK also for a
 * record on a fusion contig -- unless thj_span_juncdb_fusion_contigs turned them on for this table -- and for one of more than 128
 * bases: the host factory takes the shard.  A sixth CIGAR operation after the splice is THJ_EINVAL, as a sixth operation in a contig
 * map is; so is the fifth of a fused hit (the host factory ends the run there too).  thj_bam_piece.tid2ref of a spliced piece is
 * not looked at. */
int thj_ingest_span_batch_spliced(thj_ctx* ctx, const thj_params* p, int32_t nseg, const thj_bam_piece* segs, int32_t n_spliced,
                                  const thj_bam_piece* spliced, const thj_bam_piece* reads, uint32_t begin_id, uint32_t end_id,
                                  thj_span_batch** out, uint32_t** row_ids, int64_t* n_rows, uint8_t** reads_infl, int64_t* reads_infl_bytes,
                                  uint32_t** row_loc);
int thj_span_batch_attach_reads(thj_ctx* ctx, thj_span_batch* batch, int32_t words_per_plane, int32_t qual_stride, const uint64_t* planes,
                                const uint16_t* lens, const uint8_t* quals);
/* reads_infl, reads_infl_bytes and row_loc may all three be NULL: the read records then stay on the device with the batch only
 * (thj_span_bam_encode reads them there).  A caller that needs the host copy after all asks for it here (same buffers as above). */
int thj_span_batch_reads_host(thj_ctx* ctx, const thj_span_batch* batch, uint8_t** reads_infl, int64_t* reads_infl_bytes, uint32_t** row_loc);

/* ---------------------------------------------------------------- the BAM writer's device side (the output format)
 * long_spanning_reads prints every alignment with print_bamhit (bwt_map.cpp:1888-2093: GBamRecord with the mate fields "*", 0, 0,
 * MAPQ 255 and the tags AS XM XO XG MD NM [XS], add_aux common.cpp:1092-1173) through bam_write1 -> bgzf_write -> deflate_block
 * (samtools-0.1.18 bam.c:207-236, bgzf.c:287-349, :587-623).  Here the records are built and deflated where the alignments already
 * are; the host decides where BGZF members end (bam_write1's bgzf_flush_try rule needs record sizes only), wraps the deflated
 * members in their 18 + 8 bytes and writes them.
 *
 * thj_span_bam_encode: after thj_span_finish.  The pass's alignments (thj_span_finish's count n, thj_span_download's order) as BAM
 *   records, block_size fields included, back to back in a buffer the context keeps until the next call.  batch: the pass's batch
 *   from thj_ingest_span_batch (it holds the reads' own BAM records, where names, bases and qualities are copied from);
 *   tid_of_ref[ref_id - 1] = the contig's index in the output header; rec_size[i] / rec_id[i] (HOST, n entries) = byte count and
 *   read id (atol of the name) of record i; *total_bytes = the stream's length.  THJ_EFALLBACK: a record of the pass needs the host
 *   encoder (a fusion alignment: two records with XF:Z; an MD string the device record does not hold; a read whose length differs
 *   from the alignment's) or the batch has no read records -- nothing was encoded, thj_span_download still works.
 * thj_span_bam_encode_records: thj_span_bam_encode that also takes fusion alignments, as the two records print_bamhit writes for one
 *   (extract_partial_hits, bwt_map.cpp:2148-2347: the ops before the fusion op on contig ref_id, the ops after it on cigar[15], each with
 *   its piece of the read and XF:Z:<1|2> <name1>-<name2> <left + 1> <cigar text> <SEQ> <QUAL>).  rec_size / rec_id hold one entry per
 *   RECORD (HOST, rec_cap >= 2 * thj_span_finish's count always suffices), *n_records = how many.  The contig names come from
 *   thj_bam_contig_names_upload (HOST array of n_ref NUL-terminated names, names[ref_id - 1]; kept on the context until the next
 *   upload; n_ref == 0 takes them away).  THJ_EFALLBACK as for thj_span_bam_encode for what stays with the host encoder (an MD string
 *   the device record does not hold; a read whose length differs from the alignment's; a fusion alignment of more than 15 ops, with a
 *   second fusion op or with cigar[15] outside 1..n_ref), and for a fusion alignment when no names are uploaded for these n_ref contigs.
 * thj_bgzf_deflate: the context's stream cut at member_end[k] (exclusive, rising; every member 1..65536 bytes).  comp (HOST,
 *   comp_cap bytes) receives the members' raw DEFLATE streams back to back, comp_len[k] bytes each; crc[k] = CRC-32 of member k's
 *   bytes.  One dynamic-Huffman block per member.  THJ_EFALLBACK: a member's DEFLATE stream exceeds 65536 - 26 bytes
 *   (incompressible data; bgzf.c then shrinks the member, which moves every later cut -- the caller replays on the host).
 * thj_bam_stream_upload / _download: set / fetch the context's stream (other producers; the host fallback; tests). */
int thj_span_bam_encode(thj_ctx* ctx, const thj_span_batch* batch, const int32_t* tid_of_ref, int32_t n_ref, uint32_t* rec_size, int64_t* rec_id,
                        int64_t* total_bytes);
int thj_bam_contig_names_upload(thj_ctx* ctx, const char* const* names, int32_t n_ref);
int thj_span_bam_encode_records(thj_ctx* ctx, const thj_span_batch* batch, const int32_t* tid_of_ref, int32_t n_ref, int64_t rec_cap,
                                uint32_t* rec_size, int64_t* rec_id, int64_t* n_records, int64_t* total_bytes);
int thj_bgzf_deflate(thj_ctx* ctx, int64_t n_members, const int64_t* member_end, uint8_t* comp, int64_t comp_cap, uint32_t* comp_len, uint32_t* crc,
                     int64_t* comp_bytes);
int thj_bam_stream_upload(thj_ctx* ctx, const uint8_t* bytes, int64_t n);
int thj_bam_stream_download(thj_ctx* ctx, uint8_t* bytes);
/* thj_bam_stream_sort: the context's stream put into the order `samtools sort` (the vendored 0.1.18, by position) gives a file of these
 *   records -- what tophat.py runs over tophat_reports' part file to make accepted_hits.bam (tophat.py:2745-2779).  Not a plain stable
 *   sort: the reference collects records until their bytes (4 + block_size each) reach max_mem (500000000 unless -m is given), sorts
 *   every such block stably by (uint64_t)tid << 32 | (pos + 1) (bam1_lt, bam_sort.c:302-308) and, when a block ever ended, merges the
 *   blocks with a heap whose key also holds the strand (bam_merge_core, bam_sort.c:41, :207, :232); tophat_amd/csrc/thj_bamsort_core.h
 *   and DESIGN.md hold the rule and the closed form the device computes.  rec_size (HOST): in, the n_records sizes in stream order,
 *   each with its 4-byte block_size field; out, the sizes in the new order.  *n_blocks = how many blocks the reference would have
 *   written (1: no merge).  The stream must hold exactly these records back to back: the sizes add up to the stream's bytes, every
 *   record's 4 + block_size is its size and block_size >= 32 -- otherwise THJ_EINVAL with a message, the stream and rec_size unchanged.
 *   THJ_EINVAL too for max_mem < 1, for more than 2^31 - 17 records and for a pos below -1 or of 2^31 - 1 (the two keys order those
 *   differently).  n_records == 0: THJ_OK, nothing done.  Works on any stream: behind thj_juncbed_report_bam /
 *   thj_juncbed_report_pairs_bam (before thj_bgzf_deflate, which then deflates the sorted stream) or behind thj_bam_stream_upload.
 *   Synchronous.  Peak device memory: twice the stream (the sorted copy is written into the deflater's scratch, grown to the stream's
 *   size; the two buffers are swapped) plus 32 bytes a record (keys and indices twice over, which the tail pass and the new sizes and
 *   offsets reuse, and the records' offsets), freed before the call returns. */
int thj_bam_stream_sort(thj_ctx* ctx, uint32_t* rec_size /*HOST, in: sizes in stream order; out: in sorted order*/, int64_t n_records, int64_t max_mem,
                        int64_t* n_blocks);

/* ---------------------------------------------------------------- junction consensus
 * What tophat_reports does with the reported alignments to get junctions.bed: every REF_SKIP is a junction observation
 * (junctions_from_spliced_hit, junctions.cpp:19-97), observations of one junction merge (support adds up, extents take the
 * maximum: JunctionStats::merge_with, junctions.h:87-101), filter_junctions (accept_if_valid + knockout_shadow_junctions,
 * junctions.cpp:192-330) judges the set, alignments on a rejected junction are dropped and the rest make the final set
 * (tophat_reports.cpp:1182-1230), minus junctions whose extents stay below 8 (:2974-2984).  tophat_reports' choice of which
 * alignments of a read to report is made only after thj_juncbed_best_alignments (below; single-end: no pair grading, no realign_reads);
 * without that call every record handed in counts.
 * Call order: reset; add (any number of times); finish; download. */
typedef struct { uint32_t ref_id, left, right, antisense, left_extent, right_extent, support, reserved; } thj_juncstat;
/* Capacity (distinct junctions) of the device table; default: four times the candidate set of the spanning pass, >= 2^20. */
int thj_juncbed_configure(thj_ctx* ctx, int64_t junction_capacity);
int thj_juncbed_reset_async(thj_ctx* ctx);
/* The records of the last long_spanning_reads pass, still resident on the device (after thj_span_finish). */
int thj_juncbed_add_span_async(thj_ctx* ctx);
/* Any alignment records (HOST array, or DEVICE array when on_device != 0): ref_id, left, flags & THJ_HIT_ANTISENSE_SPLICE,
 * n_cigar and cigar are read (after thj_juncbed_read_filter also mismatches; after thj_juncbed_collect_fusions read_idx and edit_dist;
 * after thj_juncbed_best_alignments read_idx, AS, mismatches and flags & THJ_HIT_ANTISENSE). */
int thj_juncbed_add_records(thj_ctx* ctx, const thj_aln* recs, int64_t n, int32_t on_device);
/* Filters, second pass, final set in Junction::operator< order; synchronises.  min_anchor_len = --min-anchor (common.cpp:105). */
int thj_juncbed_finish(thj_ctx* ctx, int32_t min_anchor_len, int64_t* n_juncs);
int thj_juncbed_download(thj_ctx* ctx, thj_juncstat* out);
/* insertions.bed and deletions.bed come from the same second pass (tophat_reports.cpp:2286-2313: what
 * exclude_hits_on_filtered_junctions keeps -- a record without a REF_SKIP always, one with junctions when all of them were accepted --
 * goes through update_insertions_and_deletions): every DEL / dEL is a deletion observation (deletions_from_spliced_hit,
 * deletions.cpp:83-151; Deletion = Junction with antisense false), every INS / iNS an insertion observation with the letters SEQ holds
 * there (insertions_from_spliced_hit, insertions.cpp:109-180); observations of one indel merge like junctions do.  Two insertions of
 * equal length at one place are ONE entry (Insertion::operator< compares contig, left and the LENGTH of the sequence,
 * insertions.h:52-67) and the first one added keeps its letters: "first" = the order of the add calls and, inside a call, of the
 * records (resident records: thj_span_download's order).  Off unless asked for; every call sequence without
 * thj_juncbed_collect_indels gives what it gave before.  read_mismatches / read_gap_length / read_edit_dist are applied only after
 * thj_juncbed_read_filter (below); without that call every record handed in counts.
 * An insertion is held up to 16 bases of A, C, G, T, N; a longer one is an error, never a shortened letter string. */
typedef struct { uint32_t ref_id, left, len, support, left_extent, right_extent; char bases[16]; } thj_insstat;
/* Between thj_juncbed_reset_async and the first add (THJ_ESTATE afterwards); a reset turns it off again. */
int thj_juncbed_collect_indels(thj_ctx* ctx, int32_t on);
/* thj_juncbed_add_records for HOST records plus the ASCII letters of their INS / iNS ops: record i's are ins_bases[ins_off[i] ..
 * ins_off[i + 1]), op after op in cigar order (ins_off has n + 1 entries, ins_off[0] == 0).  THJ_EINVAL, nothing counted: the letters
 * do not add up to the cigar's insertions, an insertion of more than 16 bases, a letter other than ACGTN.  While indels are collected
 * thj_juncbed_add_records itself takes only records without insertions (THJ_EINVAL otherwise; deletions need no letters) and
 * thj_juncbed_add_span_async none at all. */
int thj_juncbed_add_records_seq(thj_ctx* ctx, const thj_aln* recs, int64_t n, const int64_t* ins_off, const char* ins_bases);
/* thj_juncbed_add_span_async with the pass's batch (as thj_span_bam_encode takes it; one batch per pass): the letters are read on the
 * device from the batch's read planes -- read_idx, THJ_HIT_ANTISENSE (SEQ is then the read reverse-complemented), the offset in SEQ.
 * The records are put in thj_span_download's order first (THJ_EFALLBACK when that cannot be done on the device); synchronises.  An
 * insertion of more than 16 bases or a record that points outside the batch raises a flag on the device: thj_juncbed_finish then
 * returns THJ_EINVAL and says which.  Without thj_juncbed_collect_indels: thj_juncbed_add_span_async. */
int thj_juncbed_add_span_seq_async(thj_ctx* ctx, const thj_span_batch* batch);
/* After thj_juncbed_finish (which returns THJ_EOVERFLOW for a full indel table exactly as for the junction table: each indel table
 * has the junction table's capacity): the sizes of the two sets, and the sets -- insertions in Insertion::operator< order (contig,
 * left, length), deletions in Junction::operator< order; support is the full count (print_insertions caps what it prints at 1000,
 * insertions.cpp:90-93; print_deletions does not).  There is no extent filter for indels. */
int thj_juncbed_indel_counts(thj_ctx* ctx, int64_t* n_ins, int64_t* n_del);
int thj_juncbed_indel_download(thj_ctx* ctx, thj_insstat* ins, thj_juncstat* dels);
/* fusions.out comes from the same two passes (update_fusions, tophat_reports.cpp:1156-1180; fusions.cpp).  Per read, both passes:
 * a read with more than `multireads` alignments is skipped, and of the rest an alignment with edit_dist > `read_mismatches`; a fusion
 * alignment is one record.  The fusion of an alignment: fusions_from_spliced_hit with auto_sort (fusions.cpp:441-495) -- key (ref_id1,
 * ref_id2, left, right, dir), contig order = contig number; it counts when its fusion op is neither first nor last and at least
 * `anchor_len` bases (M, N, D of either case) lie on each side (:141-194).  Pass 1 takes every record and only builds the reference set;
 * pass 2 takes the records the junction filter keeps, group sizes counted among those: count, left_ext / right_ext (maximum),
 * left_bases[k] / right_bases[k] = alignments with more than k bases on that side, and at a fusion's first sight two 100-base strings
 * around the break with five difference() values (n_diffs = 5; near a contig end no strings, n_diffs = 0).  unsupport: alignments
 * without fusion op and REF_SKIP, read_len() >= 40, that cover an end of a pass-1 fusion by 20 bases on each side (:287-343).  Not
 * reproduced: pair_support (it needs tophat_reports' mate pairing): fusions.out prints 0, 0 and an empty pair list, which is what the
 * reference prints for single-end input.
 * With collection on the add calls read thj_aln.read_idx and thj_aln.edit_dist: read_idx numbers the reads of ONE add call; for host
 * records it must be below the call's n (THJ_EINVAL otherwise, nothing counted), resident records use the pass's reads.  Off unless asked
 * for; a reset turns it off; every call sequence without thj_juncbed_collect_fusions gives what it gave before. */
typedef struct {
    uint32_t ref_id1, ref_id2, left, right, dir;   /* dir: THJ_CIG_FUSION_FF .. _RR (7..10) */
    uint32_t count, unsupport, left_ext, right_ext, n_diffs;
    uint32_t diffs[5];
    uint32_t left_bases[50], right_bases[50];
    char seq1[100], seq2[100];
} thj_fusstat;   /* n_diffs 0 or 5; 0 = no strings */
/* Between thj_juncbed_reset_async and the first add (THJ_ESTATE afterwards), like thj_juncbed_collect_indels.  The fusion table has the
 * junction table's capacity; a full one is THJ_EOVERFLOW from thj_juncbed_finish (configure, reset, add again). */
int thj_juncbed_collect_fusions(thj_ctx* ctx, int32_t on, int32_t anchor_len, int32_t read_mismatches, int32_t multireads);
/* After thj_juncbed_finish: the number of rows (fusions with count > 0) and the rows in Fusion::operator< order (fusions.h:39-67). */
int thj_juncbed_fusion_count(thj_ctx* ctx, int64_t* n);
int thj_juncbed_fusion_download(thj_ctx* ctx, thj_fusstat* out);
/* The two inputs of tophat_reports' consensus beside the alignments.  Both calls: between thj_juncbed_reset_async and the first add
 * (THJ_ESTATE afterwards), a reset turns both off, every call sequence without them gives what it gave before.
 *
 * The annotated junctions (tophat_reports --gtf-juncs): HOST array of thj_junction, any order, duplicates allowed; n == 0 turns it off.
 * filter_junctions accepts a junction of the annotation whatever its extents, length and support (junctions.cpp:305-318: no
 * accept_if_valid, so no min_anchor_len test and no "> 50000" rule), and knockout_shadow_junctions leaves it alone (:270) -- as a
 * neighbour of another junction it still competes with its support.  Records on such junctions therefore reach the second pass, and
 * their other junctions, indels and fusions with them.  The final extent filter (< 8, support 0) applies as ever.  An entry no record
 * shows adds nothing (the reference gives it support 0 and erases it at the end).  Entries that can equal no junction of a record are
 * ignored: ref_id 0 or beyond the resident genome, right - left outside 1 .. 2^29 - 1, left outside its contig. */
int thj_juncbed_known_junctions(thj_ctx* ctx, const thj_junction* juncs, int64_t n);
/* read_best_alignments / exclude_hits_on_filtered_junctions' filter (tophat_reports.cpp:133-136, :1202-1205): a record with
 *   mismatches > read_mismatches || gap_length > read_gap_length || edit_dist > read_edit_dist
 * is dropped before anything else looks at it: it has no junction, indel or fusion occurrence in either pass and is no member of its
 * read's group for --fusion-multireads.  The three quantities as BAMHitFactory makes them (bwt_map.cpp:1175-1188, :1362-1365,
 * :1429-1430, :32-43): mismatches = thj_aln.mismatches, for which both record parsers (thj_junctions' host reader, thj_juncbed_add_bam)
 * put (uint8)((uint8)NM - the lengths of the cigar's I and D ops), no NM counting as 0 -- the wrap is the reference's: an indel record
 * without NM has 256 - length mismatches and is dropped; gap_length = the lengths of the cigar's I, i, D and d ops; edit_dist =
 * (uint8)(mismatches + gap_length).  For a fusion alignment the reference rebuilds the cigar from XF:Z and subtracts over THAT
 * cigar's I and D (:1282-1285) -- the lower-case i and d of pieces that run down the genome are not subtracted, though gap_length
 * counts them -- and never over the CIGAR column of either of its two records; so do the parsers here.  Resident records of
 * long_spanning_reads and arrays handed to thj_juncbed_add_records(_seq) carry their maker's thj_aln.mismatches.  thj_aln.edit_dist is
 * not read by the filter (it keeps NM itself, clamped to 0..255, for the fusion set).
 * With paired input the reference's FIRST pass takes the alignments of an insert of which no pair is kept unfiltered
 * (tophat_reports.cpp:2075-2079): thj_juncbed_pair_alignments (below) reproduces that; without it no pairing is made and every record is
 * filtered in both passes: exact for single-end input, and for the second pass always.  on == 0 turns it off. */
int thj_juncbed_read_filter(thj_ctx* ctx, int32_t on, int32_t read_mismatches, int32_t read_gap_length, int32_t read_edit_dist);
/* tophat_reports' choice among the alignments of a read, the single-end half: read_best_alignments in both of its modes
 * (tophat_reports.cpp:113-208), the AlignStatus score (align_status.cpp:40-284) and the --max-multihits cap with the reference's own
 * random trimming.  Between thj_juncbed_reset_async and the first add (THJ_ESTATE afterwards), a reset turns it off, every call sequence
 * without it gives what it gave before.  max_multihits >= 1, bowtie2_max_penalty >= 0.
 * A read = the records of ONE add call that follow each other under one thj_aln.read_idx; every read is treated as a singleton, which is
 * exact for single-end input.  The add calls then read read_idx and AS as well: for host arrays read_idx must be below n and must not
 * fall (THJ_EINVAL otherwise, nothing counted); thj_juncbed_add_bam numbers the reads itself, keeps every mapped record on a known contig
 * (records without a REF_SKIP compete too) and keeps a read's run in one call exactly as with fusions collected (more_follows, the resume
 * point); a record without AS:i, or with one outside int16, is THJ_EINVAL with nothing counted -- the score the reference derives for
 * such a record from MD and the qualities (bwt_map.cpp:1287-1292, :1377-1405) is not built and never guessed.
 *   first pass: the records under the read filter's limits (when it is on), sorted by BowtieHit::operator< (bwt_map.h:180-207), std::unique
 *     by cmp_read_equal (tophat_reports.cpp:94-111): only the first of equal ones feeds the first-pass junction statistics.
 *   second pass, from the raw records again: the limits; exclude_hits_on_filtered_junctions; the score = AS, + 2 per junction of the
 *     annotation, - bowtie2_max_penalty per junction the first pass does not know (looked up under the alignment's FIRST contig, also
 *     behind a fusion op), else - (int)((bowtie2_max_penalty + 2) * f) with f = 1 below 5 supporting hits, 0.5 when a first-pass extent is
 *     below min(read_len / 4, 10), else 0 (the reference's coverage term is 0: its update_coverage calls are commented out); the records at
 *     the maximum, sorted and made unique again; more than max_multihits left: none with suppress_hits, else entries are erased at
 *     rng() % size until max_multihits are left -- boost::mt19937 seeded 1, reads visited in input order (add call after add call, record
 *     order inside), one further draw per read of which anything is reported (tophat_reports.cpp:1005-1007).  This reproduces
 *     tophat_reports -p 1 over one id-sorted single-end input.
 * What is left feeds the final junction, insertion and deletion sets.  Works with thj_juncbed_collect_indels, thj_juncbed_known_junctions
 * and thj_juncbed_read_filter in any combination.  Not built, and THJ_EINVAL with a message that says so, never another answer:
 * thj_juncbed_add_span_async / _seq_async (the resident slot layout) and the combination with thj_juncbed_collect_fusions.  Not built at
 * all: realign_reads (tophat_reports.cpp:1231-1770), --report-secondary-alignments.  Pairs: thj_juncbed_pair_alignments, below. */
int thj_juncbed_best_alignments(thj_ctx* ctx, int32_t on, int32_t max_multihits, int32_t suppress_hits, int32_t bowtie2_max_penalty);
/* After thj_juncbed_finish with best alignments chosen: counts[0] reads, [1] reads that lost records to the choice (before the cap),
 * [2] reads over the cap, [3] records dropped as duplicates in the first pass.  Zeros otherwise. */
int thj_juncbed_best_counts(thj_ctx* ctx, int64_t* counts /*[4]*/);
/* The paired half of that choice: pair_best_alignments in both of its modes (tophat_reports.cpp:358-576) with its callers (:2051-2096,
 * :2388-2594), the InsertAlignmentGrade score (inserts.h:72-184; operator<, inserts.cpp:22-46, orders two mapped ends by the score alone),
 * pair_distances (inserts.cpp:105-132), is_fusion_insert_alignment and set_insert_alignment_grade (tophat_reports.cpp:217-261).
 * thj_juncbed_pair_alignments: between thj_juncbed_reset_async and the first add, after thj_juncbed_best_alignments (THJ_ESTATE otherwise;
 *   its max_multihits, suppress_hits and bowtie2_max_penalty hold for pairs too); a reset, and thj_juncbed_best_alignments called again, turn
 *   it off; every call sequence without it gives what it gave before.  inner_dist_std_dev < 1 is THJ_EINVAL (the grade divides by it),
 *   fusion_min_dist < 0 too.  The records of such a consensus come through thj_juncbed_add_pairs alone: every other add call is THJ_ESTATE,
 *   and thj_juncbed_add_pairs without the switch is THJ_ESTATE.
 * thj_juncbed_add_pairs: HOST arrays of the left and of the right reads' records (the fields thj_juncbed_best_alignments reads).  read_idx =
 *   the insert's number inside the call: it must not fall within a side and stays below n_left + n_right (THJ_EINVAL otherwise, nothing
 *   counted).  An insert = the left and the right records under one number; an insert on one side only is a singleton.  The call visits
 *   them as the reference's merge does (:2002-2097, :2388-2594) -- by number; an insert's left records, then its right records -- and several
 *   calls continue that order.  This reproduces tophat_reports -p 1 over one id-sorted file per side.
 *   The grade of a candidate (left record, right record): not allowed when both have a fusion op.  A "fusion" pair: either has a fusion op,
 *   the contigs differ, the strands are equal, or the signed distance of the two left()s (:233-239: left() on purpose) is negative or above
 *   fusion_min_dist.  Score = score(left) + score(right); a fusion pair: - bowtie2_max_penalty (fusion_search is false: --fusion-search
 *   grading is not built).  Otherwise, with the inner distance of pair_distances (0 when one hit contains the other): above mean + sd
 *   ("too far") - bowtie2_max_penalty, or half of it (integer) when inner - (mean + sd) < sd; below mean - sd - min(bowtie2_max_penalty / 2,
 *   (mean - sd - inner) / sd + 1); equal strands - bowtie2_max_penalty.  A too-far pair stops being too far when some junction on the left
 *   record's contig with FIRST-pass support >= 10 lies in the gap (inner1 <= left, right <= inner2) and leaves a distance inside [mean - sd,
 *   mean + sd] (inserts.h:111-150); the second pass searches the whole first-pass set, accepted or rejected; the first pass searches the
 *   annotation, whose entries have support 0: no rescue there.
 *   Per side the candidates come from the first 2 * max_multihits + 1 records under the read filter's limits (second pass: that
 *   exclude_hits_on_filtered_junctions keeps), left-major.
 *   first pass (scores = AS): every allowed candidate is kept, except a fusion pair unless report_discordant; std::sort by score descending,
 *     std::unique of neighbours by cmp_pair_equal (cmp_read_equal on both sides).  Every kept pair adds its left and its right record to the
 *     first-pass statistics: a record in k pairs counts k times.  No pair kept: all records of both reads count once each, the ones over the
 *     read filter's limits too (:2075-2079).  A singleton takes the single-end first pass.
 *   second pass: a singleton, and a read whose mate has nothing left, contributes nothing (write_singleton_alignments, :2266-2280) unless
 *     report_mixed: then it takes the single-end second pass.  Both sides non-empty: the reference's sequential list (:441-468) -- the
 *     running best rises on every allowed candidate, also on a fusion candidate that is then skipped (no report_discordant); a candidate that
 *     is not skipped enters an emptied list when it raises the best and the list when it equals it, so the list can hold two scores -- sorted,
 *     made unique; more than max_multihits left: none with suppress_hits, else the cap walk of :538-571 (the score at place max_multihits - 1,
 *     the pairs above it, rng() % size among its ties) with the generator of the single-end choice, visited in the same order, and one
 *     further draw per insert of which a pair is reported (print_sam_for_pair, :1055-1056).  With report_mixed an insert whose list is
 *     empty, or whose best grade is a fusion grade without report_discordant, sends both sides down the single-end way, left first.  Every
 *     reported pair adds its two records to the final junction, insertion and deletion sets: a record in k pairs counts k times.  Which of
 *     two insertions of equal place and length keeps its letters is settled by the reference's order of observation: inserts in visit order,
 *     and per insert the left records in pair-list order, then the right records in pair-list order (:2502-2519).
 *   std::sort is libstdc++'s: up to 16 candidates it is an insertion sort, ties stand in generation order, and the device finds every
 *   candidate's place by counting; a longer list is handed to the host, which runs std::sort itself on the same sequence of scores with the
 *   same comparator and returns the order -- the order is the reference's wherever both are built with the same libstdc++ (as for
 *   thj_juncbed_report_bam's index_vector).
 *   Works with thj_juncbed_known_junctions, thj_juncbed_read_filter and thj_juncbed_collect_indels.  Not built, THJ_EINVAL with a message
 *   that says "not built": beside thj_juncbed_collect_fusions, thj_juncbed_collect_accepted (print_sam_for_pair), and the resident span records.
 * thj_juncbed_add_pairs_seq: thj_juncbed_add_pairs plus the ASCII letters of the records' INS / iNS ops, per side as
 *   thj_juncbed_add_records_seq takes them (ins_off has n + 1 entries, ins_off[0] == 0; the same THJ_EINVAL cases, nothing counted).  While
 *   indels are collected thj_juncbed_add_pairs itself takes only records without insertions.  Not built at all: --fusion-search grading, realign_reads,
 *   --report-secondary-alignments, BamMerge of several files per side (the unmapped-read files and the align-summary counters:
 *   thj_juncbed_collect_unmapped, below).  After a paired finish
 *   thj_juncbed_best_counts counts every side as a read of its own and is of no use.
 * thj_juncbed_pair_counts: after thj_juncbed_finish: counts[0] inserts with both sides, [1] inserts of which a pair is reported, [2]
 *   inserts over the cap, [3] singletons, [4] reads that have alignments left but contribute nothing because their mate has none (or is
 *   absent) and report_mixed is off.  Zeros otherwise. */
int thj_juncbed_pair_alignments(thj_ctx* ctx, int32_t on, int32_t inner_dist_mean, int32_t inner_dist_std_dev, int32_t fusion_min_dist, int32_t report_mixed,
                                int32_t report_discordant);
int thj_juncbed_add_pairs(thj_ctx* ctx, const thj_aln* left, int64_t n_left, const thj_aln* right, int64_t n_right);
int thj_juncbed_add_pairs_seq(thj_ctx* ctx, const thj_aln* left, int64_t n_left, const int64_t* left_ins_off, const char* left_ins_bases, const thj_aln* right,
                              int64_t n_right, const int64_t* right_ins_off, const char* right_ins_bases);
int thj_juncbed_pair_counts(thj_ctx* ctx, int64_t* counts /*[5]*/);
/* An add call straight from the bytes of a BAM file of reported alignments (a spanning BAM of long_spanning_reads, a whole-read map, an
 * accepted_hits file): `piece` = whole BGZF members (thj_bam_piece: first_skip = where the first record begins in the first member,
 * tid2ref[tid] = contig number, 0 = unknown).  The members are inflated and the records parsed on the device, exactly as thj_junctions'
 * host reader parses them: unmapped records and records on unknown contigs are skipped; a record without a REF_SKIP is kept only when
 * indels are collected and it has an I or D, or when fusions are collected; a fusion alignment (XF:Z) is rebuilt from the first of its two
 * records, its contigs looked up by NAME (thj_bam_contig_names_upload first: THJ_ESTATE without; N / n longer than max_report_intron
 * drops it); edit_dist = NM clamped to 0..255, mismatches = what thj_juncbed_read_filter reads; inserted letters come from SEQ (a fusion alignment: from the tag).  Records are added in
 * file order.  With fusions collected a read's alignments are the kept records that follow each other under one QNAME and one pair of
 * 0x40 / 0x80 bits, and they must go into ONE add call: with more_follows != 0 the piece's last such run is left out and *resume_member
 * (member index inside the piece, empty members counted) / *resume_skip say where it begins -- the next piece starts at that member with
 * first_skip = *resume_skip; otherwise everything is taken and the resume point is the piece's end (member count, 0).
 * *n_records = records counted.  THJ_EINVAL, nothing counted, with a message that says which: a malformed record, a fusion alignment of
 * more than 15 operations, a kept alignment of more than 16, an insertion outside the record's bases, of more than 16 bases, or with a
 * letter other than ACGTN.  THJ_EFALLBACK, nothing counted (read the file on the host): records straddle members, more than 65535
 * members, or -- more_follows -- the piece's only run of kept records is its last.  Synchronous. */
int thj_juncbed_add_bam(thj_ctx* ctx, const thj_bam_piece* piece, int32_t max_report_intron, int32_t more_follows, int64_t* n_records,
                        uint32_t* resume_member, uint32_t* resume_skip);
/* accepted_hits.bam: the alignments thj_juncbed_best_alignments chose, rewritten as print_sam_for_single / rewrite_sam_record write them
 * (tophat_reports.cpp:985-1025, :656-781, :580-654), single-end (every read FRAG_UNPAIRED; tophat_reports -p 1 over id-sorted input).
 *
 * thj_juncbed_collect_accepted: between thj_juncbed_reset_async and the first add, after thj_juncbed_best_alignments (THJ_ESTATE
 *   otherwise); a reset turns it off.  It makes the context keep what the rewrite needs after thj_juncbed_finish -- what is kept of every
 *   record, the keep flags, the second pass's scores, and per reporting read the generator output the choice walk used to throw away
 *   (rng() % hits.size(), the primary alignment) -- and remember the records of every thj_juncbed_add_bam call.  library_type:
 *   thj_params.library_type's numbers (2 fr-firststrand, 3 fr-secondstrand make XS:A; every other value none); rg_id: --rg-id, NULL or ""
 *   for none; tid_of_ref[ref_id - 1] = the contig's index in the OUTPUT header, n_ref = the genome's contigs.
 * thj_juncbed_report_bam: after thj_juncbed_finish, called with the same pieces in the same order as the thj_juncbed_add_bam calls of this
 *   consensus (only those calls may have added records: THJ_ESTATE otherwise, as for a call too many or before the finish).  The piece is
 *   inflated and parsed again and the rewritten records of its reported alignments are APPENDED to the context's BAM stream (the first
 *   piece empties it), back to back with their block_size fields: reads in input order, a read's records in index_vector order.
 *   rec_size[0 .. *n_records) (HOST, rec_cap entries; a piece reports at most as many records as it added) = their sizes in that order,
 *   *total_bytes = the stream's length; resume_* as thj_juncbed_add_bam gives them.  The host cuts the stream into BGZF members from the
 *   sizes (bam_write1's bgzf_flush_try rule) and deflates it with thj_bgzf_deflate.
 *   Per read of which anything is reported: hits = its reported alignments in BowtieHit::operator< order, n their number; index_vector =
 *   0 .. n - 1 under std::sort by (contig, left) -- up to 16 entries libstdc++'s std::sort is an insertion sort, ties stand in hits order,
 *   and the device finds every record's place by counting; a read of more than 16 is handed to the host, which runs std::sort itself on
 *   the same sequence with the same comparator: the order is the reference's wherever both are built with the same libstdc++.  The primary
 *   record is hits[draw % n], every other record gets flag 0x100.  Per record: QNAME cut at its last '/' when fewer than 4 characters
 *   remain from there on; tid from tid_of_ref; MAPQ 50 for n = 1, else (int)(-10 log10(1 - 1/n)): 3, 1, 1, 0 ...; = and X become M; the bin
 *   is recomputed; SEQ as it is (the spare nibble of an odd length 0); QUAL as it is, or 0xff throughout when its first byte is 0xff; mate
 *   fields as they are.  Tags in the input's order through the reference's text round trip: integers re-encoded in the smallest type
 *   under add_aux's own bounds (c down to -127, s down to -32767, then i; C, S, I), A and Z as they are, every tag named AS becomes
 *   AS:i:min(0, score) with the second pass's AlignStatus score, a tag whose text holds NH:i: or XS:i: anywhere (inside a Z value too) is
 *   dropped; then NH:i:n, CC:Z (= or the next record's contig) and CP:i (its left + 1) when a record follows, XS:A when no tag's text
 *   holds XS:A: and the library type is stranded (fr-firststrand: antisense +, else -; fr-secondstrand the other way), HI:i:<place> when
 *   n > 1, RG:Z when given.
 *   THJ_EINVAL with a message that names the case, nothing appended: the pieces do not line up with the add calls (the record count or the
 *   read runs differ), a record with mtid >= 0 or flag 0x1 ("paired records: not built" here: paired input goes through
 *   thj_juncbed_collect_accepted_pairs and thj_juncbed_report_pairs_bam as two sides of single-end records), a tag named XF (a fusion alignment: not built), a
 *   tag of type f, d, H or B, an empty Z value or one with a TAB, l_seq == 0, a cigar whose query length is not l_seq, a contig without a
 *   target in the output header, a rewritten record over 64 KiB.  THJ_EFALLBACK as thj_juncbed_add_bam.  Synchronous. */
int thj_juncbed_collect_accepted(thj_ctx* ctx, int32_t on, int32_t library_type, const char* rg_id, const int32_t* tid_of_ref, int32_t n_ref);
/* accepted_hits.bam for PAIRED input: thj_juncbed_collect_accepted_pairs -- thj_juncbed_collect_accepted's arguments and rules -- beside
 * thj_juncbed_pair_alignments (either first).  thj_juncbed_collect_accepted itself beside graded inserts stays THJ_EINVAL in either order,
 * as it was: a caller that arms the single-end file is never handed the paired one.  The context then keeps,
 * from thj_juncbed_finish until the next reset, what print_sam_for_pair needs and the finish used to throw away: every insert's candidate
 * list and its order, its flags (pairs are reported; happy() of its best grade), the cap's mask of an insert over --max-multihits, and the
 * generator's draw for every insert of which a pair is reported (beside the draws of the reads that go alone) -- on the device 20 bytes an
 * insert, 16 a candidate of its list (at most (2 max_multihits + 1)^2), 4 a candidate of a list of more than 16; on the host 8 bytes an
 * insert.  Nothing more is kept when the switch is off.
 *
 * thj_juncbed_report_pairs_bam: after thj_juncbed_finish, once per thj_juncbed_add_pairs[_seq] call of this consensus and in the same
 *   order.  left_recs / right_recs (HOST) hold the raw BAM records, each behind its block_size field, of exactly the records that add
 *   call was given, in its order; record i of a side lies at [off[i], off[i + 1]) (n + 1 entries, off[0] = 0).  The records are rewritten
 *   on the device from these bytes and APPENDED to the context's BAM stream (the first call empties it); rec_size[0 .. *n_records)
 *   (HOST, rec_cap entries) = their sizes in output order, *total_bytes = the stream's length; cut into members and deflated as
 *   thj_juncbed_report_bam's.  rec_size == NULL: the call only counts -- *n_records, *total_bytes = the bytes of this call's records --
 *   nothing is appended and the call is not used up; the caller then sizes rec_cap (the counting call uploads and lays out everything the
 *   writing call does again: a caller that knows its inserts does better with a bound -- two records per reported pair, at most
 *   max_multihits pairs an insert, or the insert's own records -- as thj_junctions does).  A record that is in k reported pairs is written k times.
 *   Output order (tophat_reports.cpp:2388-2594, -p 1): inserts in visit order.  An insert that reports pairs (print_sam_for_pair, :1027-1089):
 *   n = best_hits.size() after the cap; index_vector = 0 .. n - 1 under std::sort by (contig, left) of the RIGHT records (counted on the
 *   device up to 16 entries, the host's std::sort beyond, as for a read); for i in that order the right record of pair i, then its left one;
 *   the primary pair is draw % n.  Written with its partner (rewrite_sam_record's paired overload, :783-960): FLAG |= 0x1, 0x40 (left) or
 *   0x80 (right), 0x100 unless primary, 0x2 when the insert's best grade is happy() (both mapped, opposite strands, not both spliced or
 *   their splice strands equal, not too far after the junction rescue: inserts.h:72-221 -- the grade of the first candidate in generation
 *   order that raised the running best, a skipped fusion candidate too), 0x20 when the partner is antisense; mate contig = the record's own
 *   target for an equal contig, else the partner's; mate pos = partner.left; TLEN as :864-875 (one branch when the record contains its
 *   partner and is strictly longer, one for the converse, else partner.right - left or partner.left - right), 0 on two contigs; MAPQ, NH,
 *   HI from n; CC / CP name the SAME side's record of the next pair; XS:A for a right record takes the opposite sign (add_auxData); no XP:Z
 *   (fusion_search is false).  An insert whose sides take the single-end way (--report-mixed-alignments) and a singleton: the left read's
 *   records as thj_juncbed_report_bam orders a read's, then the right read's, through the unpaired overload with their side: FLAG |= 0x1,
 *   0x40 / 0x80, 0x8; mate fields as they are.  Everything else as thj_juncbed_report_bam writes it.  A side is left or right by the
 *   array it came in; QNAME is the record's own.
 *   THJ_ESTATE: a call too many, before the finish, without both switches, or a consensus that took records any other way.  THJ_EINVAL
 *   with a message that names the case, nothing appended: the counts per side differ from the add call's; a record that does not fill
 *   its offsets; an input record that already has a mate (mtid >= 0 or flag 0x1) or an XF tag; the other loud cases of
 *   thj_juncbed_report_bam.  Not built: realign_reads, --report-secondary-alignments, fusion alignments (the unmapped-read files and the
 *   align-summary counters: thj_juncbed_collect_unmapped, below).  Synchronous. */
int thj_juncbed_collect_accepted_pairs(thj_ctx* ctx, int32_t on, int32_t library_type, const char* rg_id, const int32_t* tid_of_ref, int32_t n_ref);
int thj_juncbed_report_pairs_bam(thj_ctx* ctx, const uint8_t* left_recs, const int64_t* left_off, int64_t n_left, const uint8_t* right_recs, const int64_t* right_off,
                                 int64_t n_right, uint32_t* rec_size, int64_t rec_cap, int64_t* n_records, int64_t* total_bytes);
int thj_juncbed_report_bam(thj_ctx* ctx, const thj_bam_piece* piece, int32_t max_report_intron, int32_t more_follows, int64_t* n_records,
                           uint32_t* resume_member, uint32_t* resume_skip, uint32_t* rec_size, int64_t rec_cap, int64_t* total_bytes);

/* The unmapped-read files and align_summary.txt: what tophat_reports does with its READS files beside the alignments (the worker loop and
 * its two trailing getQRead calls, tophat_reports.cpp:2324-2611; CReadProc::process, :2197-2219; write_singleton_alignments, :2229-2322;
 * GetReadProc::writeUnmapped, reads.h:235-258; SAlignStats, :312-356).  The reference walks each reads file once, in rising read number,
 * beside the hit streams; whether a read is written and what it counts depends on that read and on its own alignment group (single-end)
 * or insert (paired) alone, so the records of an unmapped file stand in the order of the reads file.  Scope: -p 1; reads files that are
 * prep_reads' unaligned BAM -- QNAME = the read number, optional ZN:Z (the read's name) and ZT:A tags, 0x200 records taken too (ignoreQC).
 *
 * thj_juncbed_collect_unmapped: between thj_juncbed_reset_async and the first add, after thj_juncbed_best_alignments (THJ_ESTATE otherwise;
 *   its max_multihits and suppress_hits hold here too); a reset, and thj_juncbed_best_alignments called again, turn it off; every call
 *   sequence without it gives what it gave before.  Works beside thj_juncbed_pair_alignments (either first), thj_juncbed_collect_accepted[_pairs],
 *   thj_juncbed_collect_indels, thj_juncbed_read_filter and thj_juncbed_known_junctions.  max_report_intron: what concordant() compares an
 *   insert's inner distance with (inserts.h:222-225).  The context then keeps, from thj_juncbed_finish until the next reset, what the finish
 *   used to throw away: read_best_alignments' return code of every read (a byte a record), the way every insert takes through the worker loop
 *   (a word an insert), and the read numbers (8 bytes a record, or an insert when inserts are graded).  Nothing more is kept when it is off.
 *   A read has a group exactly when one of its alignment records survives the parser (what thj_juncbed_add_bam keeps with best alignments
 *   chosen: every mapped record on a known contig -- HitStream::next_read_hits, bwt_map.h:1155-1220, drops the same ones).
 * Where the numbers come from: thj_juncbed_add_bam reads them from the QNAMEs of the records it keeps, on the device (1 .. 18 digits, nothing
 *   else).  A host-array add call -- thj_juncbed_add_records[_seq], thj_juncbed_add_pairs[_seq] -- is followed at once by
 *   thj_juncbed_read_numbers: numbers[0 .. n) (HOST) = the numbers of that call's reads (runs under one read_idx), or inserts, in visit order;
 *   the next add call before it is THJ_ESTATE.  Numbers rise strictly across all add calls and 0 is no number (it is "no read" to the
 *   reference): THJ_EINVAL otherwise with a message that says which, nothing kept (a piece: nothing of it counted).  Not built, THJ_EINVAL:
 *   thj_juncbed_add_records with device arrays.
 * thj_juncbed_report_unmapped_bam: after thj_juncbed_finish, with pieces of ONE side's reads file in file order (side 0: the left or only
 *   file, 1: the right one, only with inserts graded; a side's pieces follow each other).  piece: whole BGZF members as for thj_juncbed_add_bam,
 *   n_tid / tid2ref not read.  The piece is inflated on the device, every record is looked up by its number and decided:
 *     no group: ZT:A:M -> counted xmulti, not written; else counted unmapped and written (process(), found == false);
 *     single-end, a group: read_best_alignments' code -- & 4 multi, & 16 xmulti, & 1 aligned, else unmapped and written (whatever ZT says;
 *       under suppress_hits a read over the cap is xmulti and unmapped and written);
 *     paired, :2388-2594 as written: the insert with a pair list counts the sides' own counters from pair_best_alignments' code (3, 12, 48
 *       from the list's length before the cap; emptied by suppress_hits: both unmapped, neither written), num_aligned_pairs[_multi] with the
 *       left read, num_aligned_pairs_disc when (code & 3) == 3 and the best grade is not concordant() -- also when report_mixed then sends the
 *       sides down the single-end way; a side that goes alone takes write_singleton_alignments: without report_mixed written and unmapped,
 *       with it its own code; a read without mate bits (matenum from 0x40 / 0x80 alone) counts the UNPAIRED counters there, not in the
 *       paired branch and not at :2572-2584.  Whether an insert's hit group is empty after exclude_hits_on_filtered_junctions is not known
 *       for a side of which only records over the read filter's limits are left: it changes nothing for a read with mate bits, a read
 *       without them on such an insert is THJ_EINVAL ("not built").
 *   The written records are APPENDED to the context's BAM stream (the first piece of a side empties it) as writeUnmapped makes them: QNAME =
 *   the ZN value cut at its last '/' when fewer than 4 characters remain from there (empty without ZN), tid = mtid = pos = mpos = -1, MAPQ 0,
 *   no CIGAR, bin 4680, FLAG 0x4 | (0x1 | 0x40 or 0x80 by matenum), TLEN 0, SEQ and QUAL through seqData's text (a 0x10 record reversed and
 *   complemented, the spare nibble 0, a quality byte 0xff read as 'I'; QUAL 0xff throughout when its text is "*": one base of quality 9),
 *   ZT:A:<code> when the input had one, no other tag.  rec_size[0 .. *n_records) (HOST, rec_cap entries) = their sizes, *total_bytes = the
 *   stream's length; the host cuts (bam_write1's rule) and deflates (thj_bgzf_deflate) as for thj_juncbed_report_bam.  rec_size == NULL: the
 *   call only counts -- *n_records, *total_bytes = the bytes of this piece's records -- and nothing is kept of it.  more_follows == 0 ends the
 *   side.  resume_*: the piece's end (every record stands alone).
 *   THJ_EINVAL with a message that names the case, nothing appended or counted: numbers that fall or repeat (across pieces too), number 0, a
 *   QNAME that is not digits, l_seq over 65535, a ZN tag that is no string or has more than 254 characters, a malformed record.
 *   THJ_EFALLBACK as thj_juncbed_add_bam.  THJ_ESTATE: before the finish, without the switch, reads without numbers, a side that has ended.
 * thj_juncbed_align_stats: after every side has ended: stats[0 .. 15) = SAlignStats' fields in their order (num_aligned_left, num_unmapped_left,
 *   num_aligned_left_multi, num_aligned_left_xmulti; the same four of right; num_aligned_pairs, _multi, _disc; num_aligned_unpaired,
 *   num_unmapped_unpaired, num_aligned_unpaired_multi, _xmulti).  THJ_EINVAL with a message when a read with a group was met in no reads file
 *   (the reference warns "Should never happen" and goes on; this build does not guess).  THJ_ESTATE before that point or without the switch.
 * Not built: -p > 1, FASTQ reads files, the ReadBufSize reordering of reads files that are not sorted, quality bytes 223 and 232 (copied as
 *   they are, not loud), realign_reads, --report-secondary-alignments, --fusion-search grading.  Synchronous. */
int thj_juncbed_collect_unmapped(thj_ctx* ctx, int32_t on, int32_t max_report_intron);
int thj_juncbed_read_numbers(thj_ctx* ctx, const uint64_t* numbers, int64_t n);
int thj_juncbed_report_unmapped_bam(thj_ctx* ctx, int32_t side, const thj_bam_piece* piece, int32_t more_follows, int64_t* n_records, uint32_t* resume_member,
                                    uint32_t* resume_skip, uint32_t* rec_size, int64_t rec_cap, int64_t* total_bytes);
int thj_juncbed_align_stats(thj_ctx* ctx, int64_t* stats /*[15]*/);

/* ---------------------------------------------------------------- multi-GPU exchange step
 * Reads shard over GPUs (contiguous read-id ranges, the reference's own thread partition: utils.cpp:22-170,
 * segment_juncs.cpp:4793-4810), the genome is replicated, and the per-rank event sets are united ONCE before
 * long_spanning_reads -- what segment_juncs.cpp:4911-4922 does with its per-thread sets -- by one RCCL all-gather
 * over xGMI.  A communicator binds one rank to one context (its device and stream).  Every rank's collective calls
 * must be made by its own host thread or process, in the same order on all ranks. */
typedef struct thj_comm thj_comm;
#define THJ_COMM_ID_BYTES 128
#define THJ_COMM_SELF      0   /* one rank, no transport */
#define THJ_COMM_RCCL      1   /* ncclAllGather on the context stream */
#define THJ_COMM_LOOPBACK  2   /* ranks of one process sharing a device: stream-ordered device copies (functional tests on a 1-GPU box) */
/* ncclGetUniqueId: made by one rank, handed to the others by the caller's own means (file, pipe, MPI, torch.distributed) */
int thj_comm_unique_id(uint8_t* id /*[THJ_COMM_ID_BYTES]*/);
/* One rank per process (or thread): ncclCommInitRank.  id == NULL with n_ranks == 1 gives a transport-less communicator. */
int thj_comm_create(thj_ctx* ctx, const uint8_t* id, int32_t n_ranks, int32_t rank, thj_comm** out);
/* All ranks inside this process, rank i on ctxs[i]: RCCL when the contexts sit on distinct GPUs, loopback otherwise. */
int thj_comm_create_local(thj_ctx* const* ctxs, int32_t n, thj_comm** out /*[n]*/);
void thj_comm_destroy(thj_comm* comm);
/* stats: [0] exchange steps enqueued, [1] of them repeats with larger message sections, [2] bytes one rank sends per step,
 * [3] junction-section capacity (keys) */
int thj_comm_info(const thj_comm* comm, int32_t* n_ranks, int32_t* rank, int32_t* transport, int64_t* stats /*[4]*/);

/* After this rank's thj_segjuncs_run_async calls (and thj_covsearch_finish), before thj_segjuncs_finish: packs the distinct
 * junction / deletion / insertion events, all-gathers them and inserts the other ranks' events into this rank's tables --
 * all enqueued on the context stream, no host synchronisation.  thj_segjuncs_finish then returns the united sets on every
 * rank (and repeats the step by itself if a message section or a table turned out too small). */
int thj_events_allgather_async(thj_ctx* ctx, thj_comm* comm);
/* After thj_fusion_finish: every rank's FusionSimpleSet becomes the merge_with() of all of them (fusions.cpp:975-990:
 * counts add up, the smallest edit distance wins); *n_fusions = size of the merged set, which thj_fusion_download then
 * copies out.  Synchronous. */
int thj_fusion_allgather(thj_ctx* ctx, thj_comm* comm, int64_t* n_fusions);
/* Before thj_covsearch_run_async: the coverage map becomes the OR of the ranks' maps, the contig extents their maximum, the
 * extension table the concatenation of their entries; every rank then runs the same coverage search.  Synchronous. */
int thj_covsearch_allgather(thj_ctx* ctx, thj_comm* comm);

#ifdef __cplusplus
}
#endif
#endif /* THJ_H */
