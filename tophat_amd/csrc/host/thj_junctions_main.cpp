// thj_junctions -- the junction consensus of tophat_reports as a program: reads the alignments
// tophat_reports would report from BAM files (the spanning BAMs of long_spanning_reads, whole-read maps, an accepted_hits
// file ...), reduces their REF_SKIPs to the JunctionSet on the device (thj_juncbed_*, include/thj.h) and prints junctions.bed
// exactly as print_junctions does (junctions.cpp:100-120, :330-350).  With --insertions-out / --deletions-out the same second
// pass also gives insertions.bed and deletions.bed (print_insertions, insertions.cpp:87-101; print_deletions, deletions.cpp:36-45),
// with --fusions-out fusions.out (print_fusions, fusions.cpp:347-433; --fusion-anchor-length, --fusion-read-mismatches and
// --fusion-multireads as tophat_reports reads them).
//
// With --gtf-juncs FILE the junctions of the annotation (the list tophat.py makes from -G) are accepted whatever their anchors, length and
// support, and no neighbour on the other strand knocks them out (filter_junctions, junctions.cpp:270, :305-318); records on them reach
// the second pass, their other junctions, indels and fusions with them.  With --read-filters a record with more than --read-mismatches
// mismatches, --read-gap-length gap bases or --read-edit-dist of both (defaults 2 / 2 / 2) is passed over in both passes
// (tophat_reports.cpp:133-136, :1202-1205; mismatches = NM less the lengths of I and D, thj_jbknown_core.h); without the switch the
// three options have no effect here.
//
// With --best-alignments only each read's best alignments count (thj_juncbed_best_alignments, include/thj.h): read_best_alignments in
// both of its modes -- the first pass counts equal-looking alignments of a read once, the second keeps the alignments with the top
// AlignStatus score (AS:i, + 2 per annotated junction, less a penalty per junction the first pass knows badly or not at all) -- and of
// those at most --max-multihits (20), trimmed with the reference's own generator, or none with --suppress-hits;
// --bowtie2-max-penalty (6) sets the penalty.  A read's alignments are the records that follow each other in a file under one QNAME and
// one pair of 0x40 / 0x80 bits, and every read is treated as a singleton: this reproduces tophat_reports -p 1 over one id-sorted
// single-end input; several inputs are visited one after the other in the order given, each in file order.  A record without AS:i
// ends the run.  One line on stderr counts the reads, the reads that lost records to the choice, the reads over the cap and the
// records dropped as duplicates in the first pass.
//
// With --accepted-hits-out FILE (beside --best-alignments and --sam-header; the run says which is missing) the chosen alignments are also
// written as accepted_hits.bam, the single-end half: after the finish the inputs are replayed piece for piece and every reported record
// is rewritten on the device as print_sam_for_single / rewrite_sam_record write it (thj_juncbed_collect_accepted, thj_juncbed_report_bam,
// include/thj.h: order inside a read, primary alignment, MAPQ, bin, the tags' text round trip, NH, CC / CP, XS:A by --library-type, HI,
// RG:Z from --rg-id); the host cuts the stream into BGZF members from the record sizes (bam_write1's bgzf_flush_try rule), the device
// deflates them (a member that does not fit 64 KiB deflated: the stream comes down and the host deflates it), the header is made from
// --sam-header as long_spanning_reads makes it, the file ends with the empty member, there is no .index.  The switch takes the device
// reader for both passes; THJ_HOST_INGEST=1, SAM input, records that straddle members or any THJ_EFALLBACK end the run ("accepted hits
// need BAM inputs of whole BGZF members"): no host rewrite path is built.  Paired records, fusion alignments (XF:Z), tags of type f, d, H
// or B, empty Z values and records without bases end the run with a message that names the case.  The bed outputs are byte for byte what
// they are without the switch.
//
// With --accepted-pairs-out FILE beside --right-maps (--accepted-hits-out beside it stays refused) the file is the paired one (print_sam_for_pair; thj_juncbed_report_pairs_bam, include/thj.h): the host readers keep the
// bytes of every record they keep, a side each; after the bed outputs the device lays every insert's reported records out -- per reported
// pair in index_vector order its right record, then its left one, each with its mate's contig, position, TLEN and flag bits; the sides that
// --report-mixed-alignments sends down the single-end way with 0x1, their side and 0x8 -- and rewrites them from those bytes.  SAM text
// beside the two switches ends the run ("accepted hits need BAM inputs").  A side is left or right by the option its file came under.
//
// With --sort-bam beside --accepted-hits-out or --accepted-pairs-out the file is the one tophat.py leaves the user: `samtools sort` (the vendored
// 0.1.18, tophat.py:2745-2779) over the part file above.  The records are sorted where they lie, on the device, between the last report call
// and the cut / deflate / wrap tail (thj_bam_stream_sort, include/thj.h: blocks of --sort-max-mem N bytes -- samtools sort's -m, 500000000 unless
// given -- sorted by (tid, pos + 1) and merged as bam_merge_core merges them, which is not a plain stable sort); the tail gets the sizes in the
// new order, the header is unchanged (0.1.18 does not touch @HD SO:).  One line on stderr gives records, blocks and the sort's milliseconds.
// Without an accepted-hits output the switch ends the run; without the switch every output is byte for byte what it was.
//
// With --left-reads FILE (and --right-reads FILE beside --right-maps; needs --best-alignments and --sam-header) the reads files -- prep_reads'
// unaligned BAM: QNAME = the read number, ZN:Z the read's name, ZT:A why it was trashed -- are walked after the finish as tophat_reports'
// worker walks them (thj_juncbed_collect_unmapped, thj_juncbed_report_unmapped_bam, thj_juncbed_align_stats, include/thj.h): every read is decided
// on the device from what the finish chose for its alignment group or insert, --unmapped-left-out / --unmapped-right-out FILE take the
// records GetReadProc::writeUnmapped writes (unmapped_left_0.bam / unmapped_right_0.bam, through the cut / deflate / wrap tail of the accepted
// hits) and --align-summary-out FILE takes align_summary.txt, formatted as print_alnStats formats it.  The alignments' QNAMEs are then read
// numbers on the single-end route too.  Not built, and the run says so: FASTQ reads files, SAM inputs beside these options, THJ_HOST_INGEST=1
// (the reads files are inflated and parsed on the device only), -p > 1, reads files that are not sorted by number.
//
//   thj_junctions [--min-anchor N] [--sam-header hdr.sam] [--gtf-juncs FILE] [--read-filters] [--best-alignments] [--right-maps r1.bam[,...]] [--accepted-hits-out FILE] [--accepted-pairs-out FILE] [--sort-bam [--sort-max-mem N]] [--insertions-out FILE] [--deletions-out FILE] [--fusions-out FILE] <ref.fa> <junctions.bed> <in1.bam[,in2.bam,...]>
//
// With --right-maps r1.bam[,r2.bam,...] beside --best-alignments the positional inputs are the left reads' alignments and inserts are graded
// (thj_juncbed_pair_alignments, thj_juncbed_add_pairs; --inner-dist-mean, --inner-dist-std-dev, --fusion-min-dist, --report-mixed-alignments,
// --report-discordant-pair-alignments as tophat_reports reads them).  A read's number is its QNAME cut at a trailing /1 or /2.
// Not tophat_reports: realign_reads, --report-secondary-alignments and the
// score of a record without AS:i are not built; without --best-alignments every record of the inputs that passes --read-filters counts as
// reported.  Records without a REF_SKIP cannot touch junctions.bed and are skipped while reading (with --best-alignments they compete and
// are kept); with one of the two indel options every mapped record that has an N, I or D is kept, and its inserted bases with it.
// With --fusions-out every mapped record is kept: a read's alignments (the records that follow each other in a file under one QNAME
// and one pair of 0x40 / 0x80 bits) are counted, edit_dist comes from NM:i.  The two pair-support columns of fusions.out are 0 and its
// pair list is empty (pair_support needs the mate pairing tophat_reports decides): what the reference prints for single-end input.
//
// Where the records are read.  Host route (the default): zlib on host threads and parse_record below, one thj_aln array per input,
// beside the context's creation.  Device route (THJ_DEVICE_INGEST=1, when every input is a BAM file of whole BGZF members): the files
// are mapped, cut into pieces of THJ_PIECE_MEMBERS members (default 4096) and handed to thj_juncbed_add_bam, which inflates, parses
// and adds them on the device; when it declines an input (records that straddle members, a read with more alignments than a piece
// holds) the run is redone on the host route.  THJ_HOST_INGEST=1 overrides the request.  Both routes give the same output files; one
// line on stderr says which was taken.  The device route is opt-in because it measured no faster (profiles/thj_junctions_device_ingest_10M.txt).
#include "thj_hostio.h"
#include "../thj_jb_walk.h"
#include "../thj_jbknown_core.h"

using namespace thjh;

// the records of one input (or of one reader thread's share of it): ins_n[i] inserted bases of record i, one after the other in `bases`
struct RecSet {
    std::vector<thj_aln> recs; std::vector<uint32_t> ins_n; std::string bases;
    std::vector<std::string> reads;     // --fusions-out: QNAME and mate bits of every record, what tells one read's alignments from the next's
    // --accepted-pairs-out: the bytes of every record kept, each behind its block_size field, and their lengths
    std::vector<uint8_t> raw; std::vector<uint32_t> raw_len;
    std::vector<uint64_t> numbers;      // --left-reads: the number of every read of the input, in file order (single-end)
    void append(const RecSet& o) {
        recs.insert(recs.end(), o.recs.begin(), o.recs.end()); ins_n.insert(ins_n.end(), o.ins_n.begin(), o.ins_n.end()); bases += o.bases;
        reads.insert(reads.end(), o.reads.begin(), o.reads.end());
        raw.insert(raw.end(), o.raw.begin(), o.raw.end()); raw_len.insert(raw_len.end(), o.raw_len.begin(), o.raw_len.end());
    }
    void clear() { recs.clear(); ins_n.clear(); bases.clear(); reads.clear(); raw.clear(); raw_len.clear(); numbers.clear(); }
};

// align_summary.txt as print_alnStats prints it (tophat_reports.cpp:2119-2195), its own formats and divisions (an empty input divides by
// zero there too); st = SAlignStats' fields in their order
static void print_align_summary(FILE* f, const int64_t* st, int max_multihits) {
    const long al_l = st[0], um_l = st[1], multi_l = st[2], xmulti_l = st[3], al_r = st[4], um_r = st[5], multi_r = st[6], xmulti_r = st[7];
    const long pairs = st[8], pairs_multi = st[9], pairs_disc = st[10], al_u = st[11], um_u = st[12], multi_u = st[13], xmulti_u = st[14];
    const long total_left = al_l + um_l, total_right = al_r + um_r, total_unpaired = al_u + um_u;
    auto block = [&](const char* title, long total, long al, long multi, long xmulti) {
        fprintf(f, "%s:\n", title);
        fprintf(f, "          Input     : %9ld\n", total);
        double perc = (100.0 * al) / total;
        fprintf(f, "           Mapped   : %9ld (%4.1f%% of input)\n", al, perc);
        if (al && multi > 0) {
            perc = (100.0 * multi) / al;
            fprintf(f, "            of these: %9ld (%4.1f%%) have multiple alignments (%ld have >%d)\n", multi, perc, xmulti, max_multihits);
        }
    };
    block(total_right == 0 ? "Reads" : "Left reads", total_left, al_l, multi_l, xmulti_l);
    long total_mapped = al_l, total_input = total_left, total_pairs = 0;
    if (total_right) {
        block("Right reads", total_right, al_r, multi_r, xmulti_r);
        total_input += total_right; total_mapped += al_r;
        total_pairs = total_right < total_left ? total_right : total_left;
        if (total_unpaired) { block("Unpaired reads", total_unpaired, al_u, multi_u, xmulti_u); total_input += total_unpaired; total_mapped += al_u; }
    }
    double perc = (100.0 * total_mapped) / total_input;
    fprintf(f, "%4.1f%% overall read mapping rate.\n", perc);
    if (pairs) {
        fprintf(f, "\nAligned pairs: %9ld\n", pairs);
        if (pairs_multi > 0) { perc = (100.0 * pairs_multi) / pairs; fprintf(f, "     of these: %9ld (%4.1f%%) have multiple alignments\n", pairs_multi, perc); }
        if (pairs_disc > 0) { perc = (100.0 * pairs_disc) / pairs; fprintf(f, "               %9ld (%4.1f%%) are discordant alignments\n", pairs_disc, perc); }
        perc = (100.0 * (pairs - pairs_disc)) / total_pairs;
        fprintf(f, "%4.1f%% concordant pair alignment rate.\n", perc);
    }
}

static void usage() { fprintf(stderr, "Usage:   thj_junctions [--min-anchor N] [--sam-header hdr.sam] [--gtf-juncs FILE] [--read-filters] [--best-alignments] [--right-maps r1.bam[,...]] [--accepted-hits-out FILE] [--accepted-pairs-out FILE] [--sort-bam [--sort-max-mem N]] [--insertions-out FILE] [--deletions-out FILE] [--fusions-out FILE] <ref.fa> <junctions.bed> <alignments1.bam[,alignments2.bam,...]>\n"
                                      "         --fusions-out FILE   fusions.out of the alignments (--fusion-anchor-length, --fusion-read-mismatches, --fusion-multireads apply);\n"
                                      "                              its two pair-support columns are 0 and its pair list is empty, as for single-end input\n"
                                      "         --gtf-juncs FILE     junctions of the annotation (name, left, right, orientation; TAB-separated): accepted whatever\n"
                                      "                              their anchors, length and support, and not knocked out by the other strand\n"
                                      "         --read-filters       pass over alignments with more than --read-mismatches mismatches, --read-gap-length gap\n"
                                      "                              bases or --read-edit-dist of both (2 / 2 / 2); without it the three have no effect\n"
                                      "         --best-alignments    only each read's best alignments count (read_best_alignments, the AlignStatus score from AS:i), at most\n"
                                      "                              --max-multihits (20) of them, none with --suppress-hits; --bowtie2-max-penalty (6) applies.  Without --right-maps\n"
                                      "                              reads are singletons: tophat_reports -p 1 over one id-sorted single-end input; several inputs are visited in the\n"
                                      "                              order given, each in file order.  Not built: realign_reads, --report-secondary-alignments,\n"
                                      "                              --fusions-out beside it, records without AS:i (they end the run)\n"
                                      "         --right-maps r1.bam[,r2.bam,...]   with --best-alignments: the positional inputs are the left reads' alignments, these the right\n"
                                      "                              reads'; inserts are graded (pair_best_alignments; --inner-dist-mean (200), --inner-dist-std-dev (20),\n"
                                      "                              --fusion-min-dist, --report-mixed-alignments, --report-discordant-pair-alignments apply).  Read names are the\n"
                                      "                              numbers prep_reads writes (a trailing /1 or /2 is cut); the files of a side are taken in the order given and\n"
                                      "                              their numbers must not fall (BamMerge is not built).  Read on the host.  Not built beside it: --fusions-out, --accepted-hits-out,\n"
                                      "                              --fusion-search grading\n"
                                      "         --accepted-hits-out FILE   the chosen alignments as accepted_hits.bam (single-end; needs --best-alignments and --sam-header;\n"
                                      "                              --library-type, --rg-id, --max-multihits, --suppress-hits apply).  The inputs are read on the device both\n"
                                      "                              times: BAM files of whole BGZF members only.  Not built: input records that already have a mate, fusion alignments, tags of type\n"
                                      "                              f, d, H, B (they end the run), original read names\n"
                                      "         --accepted-pairs-out FILE  beside --right-maps: accepted_hits.bam of the inserts (print_sam_for_pair: mates, TLEN, 0x1 / 0x2 / 0x8 /\n"
                                      "                              0x20 / 0x40 / 0x80; needs --best-alignments and --sam-header); the inputs are read on the host, BAM only\n"
                                      "         --sort-bam [--sort-max-mem N]   beside --accepted-hits-out / --accepted-pairs-out: the file in the order samtools 0.1.18's sort gives it\n"
                                      "                              (what tophat.py calls accepted_hits.bam), sorted on the device; N = samtools sort's -m (500000000)\n"
                                      "         --left-reads FILE [--right-reads FILE]   the reads files (prep_reads' unaligned BAM; the right one beside --right-maps): with\n"
                                      "                              --unmapped-left-out FILE / --unmapped-right-out FILE the unmapped reads as tophat_reports writes them, with\n"
                                      "                              --align-summary-out FILE align_summary.txt (needs --best-alignments and --sam-header; -p 1).  Not built:\n"
                                      "                              FASTQ reads files, SAM inputs, THJ_HOST_INGEST=1 beside them\n"
                                      "         THJ_DEVICE_INGEST=1 inflates and parses the alignment BAMs on the device, in pieces of THJ_PIECE_MEMBERS BGZF members\n"
                                      "         (default 4096); THJ_HOST_INGEST=1 keeps the host readers whatever else is set.  One line on stderr says which route was taken.\n"); }

static int real_main(int argc, char** argv) {
    Opts o;
    int rc = parse_options(argc, argv, o, usage);
    if (rc) return rc;
    std::vector<std::string> pos;
    for (int i = optind; i < argc; ++i) pos.push_back(argv[i]);
    if (pos.size() < 3) { usage(); return 1; }
    std::future<thj_ctx*> fut = std::async(std::launch::async, []() {
        thj_ctx* c = nullptr;
        if (thj_ctx_create(getenv("THJ_DEVICE") ? atoi(getenv("THJ_DEVICE")) : 0, nullptr, &c)) die("Error: %s\n", thj_last_error());
        return c;
    });
    RefTable rt;
    rt.load_sam_header(o.sam_header);
    rt.load_fasta(pos[0]);
    std::vector<std::string> inputs = split(pos[2], ',');
    // --right-maps: the positional inputs are the left reads' alignments and these the right reads'; the right files are read behind the left ones
    const size_t n_left_inputs = inputs.size();
    const bool paired = !o.right_maps.empty();
    if (paired) for (auto& f : split(o.right_maps, ',')) inputs.push_back(f);
    for (auto& f : inputs) register_targets(f, rt);
    rt.freeze();
    // --gtf-juncs: the annotation's junctions, which the filter stage accepts as they are (junctions.cpp:305-318)
    std::vector<thj_junction> gtf;
    if (!o.gtf_juncs.empty()) gtf = load_gtf_juncs(o.gtf_juncs, rt);
    // ---- spliced records -> thj_aln (only the fields the reduce reads).  BGZF members inflate independently, so every input is cut
    // into runs of members, one per host thread; a run must end on a record boundary (true of every BAM written through
    // bgzf_flush_try: samtools 0.1.18's writer, this build's) -- if one does not, that input is read again by the sequential reader.
    std::vector<RecSet> recs(inputs.size());
    const bool indels = !o.insertions_out.empty() || !o.deletions_out.empty();
    const bool fusions = !o.fusions_out.empty();
    const bool best = o.best_alignments;
    if (best && fusions) die("Error: --best-alignments beside --fusions-out is not built (the fusion set of the chosen alignments)\n");
    if (best && o.report_secondary) die("Error: --best-alignments beside --report-secondary-alignments is not built\n");
    if (paired && !best) die("Error: --right-maps needs --best-alignments (grading inserts is that choice for pairs)\n");
    if (paired && fusions) die("Error: --fusions-out beside --right-maps is not built (pair_support)\n");
    if (paired && !o.accepted_hits_out.empty()) die("Error: --accepted-hits-out beside --right-maps is not built (that switch writes the single-end file; the paired one, print_sam_for_pair, is --accepted-pairs-out FILE)\n");
    if (!paired && !o.accepted_pairs_out.empty()) die("Error: --accepted-pairs-out needs --right-maps (single-end input: --accepted-hits-out)\n");
    if (paired && o.fusion_search) die("Error: --fusion-search grading of pairs is not built\n");
    // --accepted-hits-out: the chosen alignments as accepted_hits.bam; the records are rewritten on the device from the inputs' own bytes
    const std::string& accepted_out = paired ? o.accepted_pairs_out : o.accepted_hits_out;
    const bool accepted = !accepted_out.empty();
    if (accepted && !best) die("Error: %s needs --best-alignments (the reported alignments are that choice)\n", paired ? "--accepted-pairs-out" : "--accepted-hits-out");
    if (accepted && o.sam_header.empty()) die("Error: %s needs --sam-header (the output's header)\n", paired ? "--accepted-pairs-out" : "--accepted-hits-out");
    if (o.sort_bam && !accepted) die("Error: --sort-bam needs --accepted-hits-out FILE or (beside --right-maps) --accepted-pairs-out FILE: it sorts that file's records\n");
    if (o.sort_bam && o.sort_max_mem < 1) die("Error: --sort-max-mem needs a number of bytes of at least 1\n");
    // --left-reads / --right-reads: the unmapped-read files and align_summary.txt
    const bool unmapped = !o.left_reads.empty() || !o.right_reads.empty() || !o.unmapped_left_out.empty() || !o.unmapped_right_out.empty() || !o.align_summary_out.empty();
    if (unmapped && !best) die("Error: --left-reads, --unmapped-left-out and --align-summary-out need --best-alignments (which reads are unmapped is that choice)\n");
    if (unmapped && o.sam_header.empty()) die("Error: --left-reads, --unmapped-left-out and --align-summary-out need --sam-header (the outputs' header)\n");
    if (unmapped && o.left_reads.empty()) die("Error: --unmapped-left-out, --unmapped-right-out and --align-summary-out need --left-reads FILE (the reads file, prep_reads' BAM)\n");
    if (!paired && (!o.right_reads.empty() || !o.unmapped_right_out.empty())) die("Error: --right-reads and --unmapped-right-out need --right-maps (single-end input has one reads file)\n");
    if (unmapped && paired && o.right_reads.empty()) die("Error: --left-reads beside --right-maps needs --right-reads FILE (both reads files are walked)\n");
    if (unmapped && getenv("THJ_HOST_INGEST")) die("Error: --left-reads beside THJ_HOST_INGEST=1 is not built (the reads files are inflated and parsed on the device only)\n");
    const char* const ACC_NEEDS = paired ? "--accepted-pairs-out: accepted hits need BAM inputs of whole BGZF members" : "--accepted-hits-out: accepted hits need BAM inputs of whole BGZF members";
    // One record -> thj_aln, or nothing.  A fusion alignment comes as two records that both carry the whole alignment in an XF:Z tag
    // ("1|2 <contig1>-<contig2> <pos> <cigar with an F op> <bases> <qualities>", print_bamhit, bwt_map.cpp:2047-2083): the first one is
    // rebuilt from the tag the way BAMHitFactory::get_hit_from_buf does (bwt_map.cpp:1208-1318 -- lower-case ops for pieces that run down
    // the genome, F = position on the second contig + 1, its direction FF / FR / RF / RR from the ops around it), the second is dropped.
    const int max_report_intron = o.p.max_report_intron;
    // keeps record a; with the indel outputs asked for, its inserted letters too: SEQ[position in the read ..) as insertions_from_spliced_hit
    // reads them (the walk: jbw::inss) -- letter(k) = base k of what BowtieHit::seq() holds for the record
    const bool keep_raw = accepted && paired;                  // thj_juncbed_report_pairs_bam rewrites the records from their own bytes
    auto keep = [indels, fusions, best, keep_raw](const thj_aln& a, RecSet& out, size_t seq_len, const std::function<char(size_t)>& letter, const uint8_t* d, int32_t bs) {
        out.recs.push_back(a);
        if (keep_raw) {
            uint8_t len[4]; memcpy(len, &bs, 4);
            out.raw.insert(out.raw.end(), len, len + 4); out.raw.insert(out.raw.end(), d, d + bs); out.raw_len.push_back((uint32_t)bs + 4u);
        }
        if (fusions || best) {                                 // QNAME + the 0x40 / 0x80 bits
            uint32_t bin_mq_nl, flag_nc; memcpy(&bin_mq_nl, d + 8, 4); memcpy(&flag_nc, d + 12, 4);
            std::string key((const char*)d + 32, strnlen((const char*)d + 32, bin_mq_nl & 0xFF));
            key.push_back((char)('0' + ((flag_nc >> 22) & 3)));
            out.reads.push_back(std::move(key));
        }
        if (!indels) return;
        uint32_t n = 0;
        jbw::inss(a.cigar, a.n_cigar, a.left, a.ref_id, [&](uint32_t, uint32_t, uint32_t len, uint32_t rpos, uint32_t, uint32_t, int) {
            if ((size_t)rpos + len > seq_len) die("Error: an alignment whose insertion lies outside its %zu bases\n", seq_len);
            for (uint32_t k = 0; k < len; ++k) out.bases.push_back(letter(rpos + k));
            n += len;
        });
        out.ins_n.push_back(n);
    };
    auto parse_record = [&rt, max_report_intron, indels, fusions, best, &keep](const uint8_t* d, int32_t bs, const std::vector<uint32_t>& tid2ref, RecSet& out) {
        static const uint32_t OPS[9] = {THJ_CIG_MATCH, THJ_CIG_INS, THJ_CIG_DEL, THJ_CIG_REF_SKIP, THJ_CIG_SOFT_CLIP, 14u, 15u, THJ_CIG_MATCH, THJ_CIG_MATCH};
        int32_t tid, p0; uint32_t bin_mq_nl, flag_nc; int32_t l_seq;
        memcpy(&tid, d, 4); memcpy(&p0, d + 4, 4); memcpy(&bin_mq_nl, d + 8, 4); memcpy(&flag_nc, d + 12, 4); memcpy(&l_seq, d + 16, 4);
        if (!bam_record_shape_ok(d, bs)) die("Error: malformed BAM record (its header does not fit its %d bytes)\n", (int)bs);
        const uint32_t l_rn = bin_mq_nl & 0xFF, n_cig = flag_nc & 0xFFFF;
        if (tid < 0 || ((flag_nc >> 16) & 4)) return;
        thj_aln a; memset(&a, 0, sizeof a);
        bool spliced = false, gapped = false;
        size_t pp = 32 + l_rn;
        for (uint32_t i = 0; i < n_cig; ++i) { uint32_t c; memcpy(&c, d + pp, 4); pp += 4; const uint32_t op = (c & 0xF) < 9 ? OPS[c & 0xF] : 15u; if (op == THJ_CIG_REF_SKIP) spliced = true; if (op == THJ_CIG_INS || op == THJ_CIG_DEL) gapped = true; if (i < 16) a.cigar[i] = (op << 28) | (c >> 4); }
        const uint8_t* seq4 = d + pp;                         // the 4-bit SEQ (bam1_seqi / bam_nt16_rev_table, bwt_map.cpp:1158-1165)
        pp += (size_t)(l_seq + 1) / 2 + (size_t)l_seq;
        char xs = 0; const char* xf = nullptr;
        int64_t nm = 0, as = 0;                                // NM:i, AS:i in whatever width the writer chose (bam_aux2i); no NM: 0
        bool has_as = false;
        auto int_tag = [&](char t0, char t1, int64_t v) { if (t0 == 'N' && t1 == 'M') nm = v; if (t0 == 'A' && t1 == 'S') { as = v; has_as = true; } };
        while (pp + 3 <= (size_t)bs) {                        // XS:A, XF:Z
            const char t0 = (char)d[pp], t1 = (char)d[pp + 1], ty = (char)d[pp + 2];
            pp += 3;
            if (bam_aux_fixed_size(ty) > (size_t)bs - pp) die("Error: malformed BAM record (a tag runs past its end)\n");
            switch (ty) {
            case 'A': if (t0 == 'X' && t1 == 'S') xs = (char)d[pp]; pp += 1; break;
            case 'c': int_tag(t0, t1, (int8_t)d[pp]); pp += 1; break;
            case 'C': int_tag(t0, t1, d[pp]); pp += 1; break;
            case 's': { int16_t v; memcpy(&v, d + pp, 2); int_tag(t0, t1, v); } pp += 2; break;
            case 'S': { uint16_t v; memcpy(&v, d + pp, 2); int_tag(t0, t1, v); } pp += 2; break;
            case 'i': { int32_t v; memcpy(&v, d + pp, 4); int_tag(t0, t1, v); } pp += 4; break;
            case 'I': { uint32_t v; memcpy(&v, d + pp, 4); int_tag(t0, t1, v); } pp += 4; break;
            case 'f': pp += 4; break;
            case 'd': pp += 8; break;
            case 'Z': case 'H': { const size_t at = pp; while (pp < (size_t)bs && d[pp]) ++pp; if (pp < (size_t)bs && ty == 'Z' && t0 == 'X' && t1 == 'F') xf = (const char*)d + at; ++pp; break; }
            case 'B': { char st = (char)d[pp]; int32_t cnt; memcpy(&cnt, d + pp + 1, 4); if (cnt < 0 || (int64_t)cnt > (int64_t)bs) die("Error: malformed BAM record (an array tag runs past its end)\n");
                        pp += 5 + (size_t)cnt * ((st == 'c' || st == 'C') ? 1 : (st == 's' || st == 'S') ? 2 : 4); break; }
            default: pp = (size_t)bs; break;
            }
        }
        a.flags = (uint8_t)(xs == '-' ? THJ_HIT_ANTISENSE_SPLICE : 0);
        a.edit_dist = (uint8_t)(nm < 0 ? 0 : nm > 255 ? 255 : nm);
        // --best-alignments: the score starts from AS:i; what the reference makes up for a record without one is not built
        auto take_as = [&]() {
            if (!best) return;
            if (!has_as || as < -32768 || as > 32767) die("Error: --best-alignments: alignment %.*s has no AS:i tag, or one outside -32768 .. 32767\n", (int)l_rn, (const char*)d + 32);
            a.AS = (int16_t)as;
            if ((flag_nc >> 16) & 0x10u) a.flags |= THJ_HIT_ANTISENSE;     // antisense_align(): BowtieHit::operator< and cmp_read_equal compare it
        };
        if (xf) {
            if (xf[0] == '2') return;                          // "ignore the second part of a fusion alignment" (:1214-1216)
            std::vector<std::string> f = split(xf, ' ');
            if (f.size() < 4) return;
            std::vector<std::string> cs = split(f[1], '-');
            // fewer than two names in the contig field: the reference keeps the record's own target as the first contig and an empty name as
            // the second (bwt_map.cpp:1219-1225: text_name / text_name2 stay as they were) and goes on; so does this
            const uint32_t r1 = cs.size() >= 2 ? rt.get_id(cs[0]) : ((size_t)tid < tid2ref.size() ? tid2ref[(size_t)tid] : 0), r2 = cs.size() >= 2 ? rt.get_id(cs[1]) : rt.get_id(std::string());
            if (!r1 || !r2) return;
            int n = 0; bool spl = false, gap = false;
            uint32_t op[16];
            for (const char* q = f[3].c_str(); *q;) {
                char* t; const long len0 = strtol(q, &t, 10); long len = len0;
                if (len <= 0) return;
                uint32_t code;
                switch (*t) {
                case 'M': code = 1; break; case 'm': code = 2; break; case 'I': code = 3; gap = true; break; case 'i': code = 4; gap = true; break;
                case 'D': code = 5; gap = true; break; case 'd': code = 6; gap = true; break;
                case 'N': case 'n': if (len > max_report_intron) return; code = *t == 'N' ? 11 : 12; spl = true; break;
                case 'F': code = 7; len = len - 1; break;
                case 'S': code = 13; break; case 'H': code = 14; break; case 'P': code = 15; break;
                default: return;
                }
                q = t + 1;
                if (n >= 15) die("Error: a fusion alignment of more than 15 CIGAR operations (XF:Z:%s)\n", xf);
                op[n++] = code << 28 | ((uint32_t)len & 0x0FFFFFFFu);
                if (n >= 3 && (op[n - 2] >> 28) == 7) {         // the direction of the fusion from the pieces around it (:1283-1301)
                    auto up = [](uint32_t c) { c >>= 28; return c == 1 || c == 5 || c == 3 || c == 11; };
                    const bool i1 = up(op[n - 3]), i2 = up(op[n - 1]);
                    const uint32_t dir = (i1 && !i2) ? 8u : (!i1 && i2) ? 9u : (!i1 && !i2) ? 10u : 7u;
                    op[n - 2] = dir << 28 | (op[n - 2] & 0x0FFFFFFFu);
                }
            }
            if (!spl && !(indels && gap) && !fusions && !best) return;
            memset(a.cigar, 0, sizeof a.cigar);
            for (int i = 0; i < n; ++i) a.cigar[i] = op[i];
            a.cigar[15] = r2;
            a.ref_id = r1; a.left = atoi(f[2].c_str()) - 1; a.n_cigar = (uint8_t)n;
            a.mismatches = jbk::mismatches(nm, n, jbw::ArrayCigar{a.cigar});       // NM less the I and D of XF:Z's cigar (bwt_map.cpp:1282-1285)
            take_as();
            const std::string fseq = f.size() > 4 ? f[4] : std::string();                 // seq() of a fusion record: the tag's bases (:1231-1232)
            keep(a, out, fseq.size(), [&fseq](size_t k) { return fseq[k]; }, d, bs);
            return;
        }
        if (!(spliced && n_cig >= 3) && !(indels && gapped) && !((fusions || best) && !spliced)) return;
        // a spliced alignment the consensus cannot hold must not vanish from the support counts silently
        if (n_cig > 16) die("Error: %s alignment of %u CIGAR operations (at most 16 are supported)\n", spliced ? "a spliced" : "an", n_cig);
        a.ref_id = (size_t)tid < tid2ref.size() ? tid2ref[(size_t)tid] : 0;
        if (!a.ref_id) return;
        a.left = p0; a.n_cigar = (uint8_t)n_cig;
        a.mismatches = jbk::mismatches(nm, (int)n_cig, jbw::ArrayCigar{a.cigar});  // NM less the I and D of the cigar (bwt_map.cpp:1362-1365)
        take_as();
        keep(a, out, (size_t)(l_seq > 0 ? l_seq : 0), [seq4](size_t k) { return "=ACMGRSVTWYHKDBN"[(seq4[k >> 1] >> ((~k & 1) << 2)) & 15]; }, d, bs);
    };
    auto read_parallel = [&](const std::string& fn, RecSet& out) -> bool {
        BamFile bf;
        if (getenv("THJ_SEQUENTIAL_READ") || !bf.open(fn, rt)) return false;
        std::vector<size_t> moff;
        for (size_t off = (size_t)(bf.first_rec_voff >> 16); off < bf.size;) {
            const uint32_t bs = BamFile::member_size(bf.data + off, bf.size - off);
            if (!bs || off + bs > bf.size) return false;
            moff.push_back(off); off += bs;
        }
        const size_t nm = moff.size();
        if (!nm) return true;
        const size_t T = std::min<size_t>((size_t)std::max(1, host_threads()), nm);
        std::vector<RecSet> part(T);
        std::vector<char> bad(T, 0);
        std::vector<std::thread> th;
        for (size_t t = 0; t < T; ++t) th.emplace_back([&, t]() {
            std::vector<uint8_t> buf; size_t have = 0;
            z_stream zs; memset(&zs, 0, sizeof zs);
            if (inflateInit2(&zs, -15) != Z_OK) { bad[t] = 1; return; }
            for (size_t m = nm * t / T; m < nm * (t + 1) / T && !bad[t]; ++m) {
                const uint8_t* d = bf.data + moff[m];
                const uint32_t bs = BamFile::member_size(d, bf.size - moff[m]), xlen = d[10] | (d[11] << 8);
                uint32_t isz; memcpy(&isz, d + bs - 4, 4);
                if (buf.size() < have + isz) buf.resize(have + isz + 65536);
                inflateReset(&zs);
                zs.next_in = const_cast<uint8_t*>(d + 12 + xlen); zs.avail_in = bs - 12 - xlen - 8;
                zs.next_out = buf.data() + have; zs.avail_out = isz;
                if (inflate(&zs, Z_FINISH) != Z_STREAM_END && isz) { bad[t] = 1; break; }
                size_t end = have + isz;
                size_t pos = m == 0 ? (size_t)(bf.first_rec_voff & 0xFFFF) : 0;      // the first member may still hold the end of the header
                if (m == 0 && pos > end) { bad[t] = 1; break; }
                while (pos + 4 <= end) {
                    int32_t rs; memcpy(&rs, buf.data() + pos, 4);
                    if (rs < 32) { bad[t] = 1; break; }
                    if (pos + 4 + (size_t)rs > end) break;
                    parse_record(buf.data() + pos + 4, rs, bf.tid2ref, part[t]);
                    pos += 4 + (size_t)rs;
                }
                have = end - pos;
                if (have) memmove(buf.data(), buf.data() + pos, have);
            }
            inflateEnd(&zs);
            if (have) bad[t] = 1;                                  // a record straddles the end of this run
        });
        for (auto& x : th) x.join();
        for (char b : bad) if (b) return false;
        size_t tot = 0;
        for (auto& v : part) tot += v.recs.size();
        out.recs.reserve(tot);
        for (auto& v : part) out.append(v);
        return true;
    };
    auto read_on_host = [&]() {
    std::vector<std::thread> th;
    for (size_t k = 0; k < inputs.size(); ++k) th.emplace_back([&, k]() {
        if (read_parallel(inputs[k], recs[k])) return;
        recs[k].clear();
        AlnReader rd;
        if (!rd.open(inputs[k])) die("Error: cannot open %s\n", inputs[k].c_str());
        if (!rd.is_bam() && unmapped) die("Error: --left-reads beside SAM inputs is not built (%s is no BAM file)\n", inputs[k].c_str());
        if (!rd.is_bam() && keep_raw) die("Error: %s (%s is no BAM file)\n", ACC_NEEDS, inputs[k].c_str());
        if (!rd.is_bam()) die("Error: %s: BAM input expected\n", inputs[k].c_str());
        std::vector<uint32_t> tid2ref;
        for (auto& t : rd.targets()) tid2ref.push_back(rt.get_id(t));
        int32_t bs = 0;
        while (const uint8_t* d = rd.next_raw(bs)) parse_record(d, bs, tid2ref, recs[k]);
    });
    for (auto& t : th) t.join();
    // read_idx: one number per run of records of one read, counted over the whole input (a run may straddle two reader threads' shares,
    // so the numbers are given after the shares are joined); an add call takes read_idx below its number of records
    // --right-maps: a read's number is its QNAME, cut at a trailing /1 or /2, read as a decimal (what prep_reads writes)
    if (paired)
        for (auto& v : recs) {
            for (size_t i = 0; i < v.recs.size(); ++i) {
                std::string q = v.reads[i].substr(0, v.reads[i].size() - 1);
                if (q.size() > 2 && q[q.size() - 2] == '/' && (q.back() == '1' || q.back() == '2')) q.resize(q.size() - 2);
                char* e = nullptr;
                const unsigned long long num = q.empty() ? 0 : strtoull(q.c_str(), &e, 10);
                if (q.empty() || *e || q[0] < '0' || q[0] > '9') die("Error: --right-maps: read name %s is no read number (prep_reads writes numbers)\n", v.reads[i].substr(0, v.reads[i].size() - 1).c_str());
                if (num > 0xFFFFFFFFull || q.size() > 19) die("Error: --right-maps: read number %s is too large (read numbers up to 4294967295 are held)\n", q.c_str());
                v.recs[i].read_idx = (uint32_t)num;
            }
            std::vector<std::string>().swap(v.reads);
        }
    else if (fusions || best)
        for (auto& v : recs) {
            uint32_t run = 0;
            for (size_t i = 0; i < v.recs.size(); ++i) {
                if (i && v.reads[i] != v.reads[i - 1]) ++run;
                v.recs[i].read_idx = run;
                if (unmapped && (!i || v.reads[i] != v.reads[i - 1])) {      // --left-reads: a read's number is its QNAME, digits only
                    const std::string q = v.reads[i].substr(0, v.reads[i].size() - 1);
                    if (q.empty() || q.size() > 18 || q.find_first_not_of("0123456789") != std::string::npos) die("Error: --left-reads: read name %s is no read number (prep_reads writes numbers)\n", q.c_str());
                    v.numbers.push_back(strtoull(q.c_str(), nullptr, 10));
                }
            }
            std::vector<std::string>().swap(v.reads);
        }
    };
    // ---- the device route (THJ_DEVICE_INGEST=1): every input is mapped and cut at BGZF member boundaries into pieces of THJ_PIECE_MEMBERS members
    // (default 4096); thj_juncbed_add_bam inflates a piece, parses its records and adds them on the device, and says where the next
    // piece begins (with --fusions-out a read's alignments must not be split between two calls).  Inputs in argv order, as on the host.
    // THJ_HOST_INGEST=1, an input that is no BAM file of whole members, or any THJ_EFALLBACK (records that straddle members, a read with
    // more alignments than a piece holds): the consensus is reset and the whole run is read by the host readers above.
    struct DevInput { BamFile bf; std::vector<size_t> moff; };
    std::vector<std::unique_ptr<DevInput>> dev;
    std::string host_reason;
    // Measured on the 10 M-pair mix's spanning BAMs (profiles/thj_junctions_device_ingest_10M.txt) the device route does not beat the host
    // readers, which inflate while the context is being created: it is taken on request only.
    if (paired) { if (getenv("THJ_DEVICE_INGEST") && !getenv("THJ_HOST_INGEST")) fprintf(stderr, "paired input is read on the host (device ingest of paired BAMs is not built)\n"); host_reason = "paired input"; }
    else if (getenv("THJ_HOST_INGEST")) host_reason = "THJ_HOST_INGEST";
    else if (!accepted && !getenv("THJ_DEVICE_INGEST")) host_reason = "THJ_DEVICE_INGEST is not set";
    const size_t piece_members = getenv("THJ_PIECE_MEMBERS") && atoll(getenv("THJ_PIECE_MEMBERS")) > 0 ? (size_t)atoll(getenv("THJ_PIECE_MEMBERS")) : 4096;
    auto open_dev = [&rt](const std::string& fn, std::string& why) -> std::unique_ptr<DevInput> {
        std::unique_ptr<DevInput> in(new DevInput);
        if (!in->bf.open(fn, rt)) { why = fn + " is no BAM file that can be mapped"; return nullptr; }
        size_t off = (size_t)(in->bf.first_rec_voff >> 16);
        while (off < in->bf.size) {
            const uint32_t bs = BamFile::member_size(in->bf.data + off, in->bf.size - off);
            if (!bs || off + bs > in->bf.size) { why = fn + " is not a run of whole BGZF members"; return nullptr; }
            in->moff.push_back(off); off += bs;
        }
        in->moff.push_back(in->bf.size);
        // empty members at the end (the EOF marker) hold no records: nothing follows the last member that has some
        while (in->moff.size() > 1) { uint32_t isz; memcpy(&isz, in->bf.data + in->moff.back() - 4, 4); if (isz) break; in->moff.pop_back(); }
        return in;
    };
    for (size_t k = 0; k < inputs.size() && host_reason.empty(); ++k) {
        std::unique_ptr<DevInput> in = open_dev(inputs[k], host_reason);
        if (in) dev.push_back(std::move(in));
    }
    // --left-reads / --right-reads: the reads files, mapped; a FASTQ file is no BAM file
    std::vector<std::unique_ptr<DevInput>> reads_in;
    if (unmapped)
        for (const std::string* fn : {&o.left_reads, &o.right_reads}) {
            if (fn->empty()) continue;
            std::string why;
            std::unique_ptr<DevInput> in = open_dev(*fn, why);
            if (!in) die("Error: --left-reads / --right-reads: %s; FASTQ reads files are not built (prep_reads' unaligned BAM of whole BGZF members is read)\n", why.c_str());
            reads_in.push_back(std::move(in));
        }
    if (accepted && !paired && !host_reason.empty()) die("Error: %s (%s)\n", ACC_NEEDS, host_reason.c_str());
    bool device = host_reason.empty(), route_said = false, host_read = false;
    if (!device) { host_read = true; read_on_host(); }          // (beside the context's creation, as ever)
    thj_ctx* ctx = fut.get();
    rt.upload(ctx);
    if (device || keep_raw) {
        std::vector<const char*> names;
        for (auto& n : rt.names) names.push_back(n.c_str());
        if (thj_bam_contig_names_upload(ctx, names.data(), (int32_t)names.size())) die("Error: %s\n", thj_last_error());
    }
    size_t dev_pieces = 0;
    // all inputs, piece after piece, each handed to call(piece, more_follows, inflated bytes, &resume member, &resume skip) -> the ABI's
    // return code; false: a piece wants the host readers (host_reason says why)
    typedef std::function<int(const thj_bam_piece&, int32_t, size_t, uint32_t*, uint32_t*)> PieceCall;
    auto walk_list = [&](std::vector<std::unique_ptr<DevInput>>& list, size_t first, size_t last, const PieceCall& call) -> bool {
        dev_pieces = 0;
        for (size_t which = first; which < last; ++which) {
            auto& in = list[which];
            const size_t nm = in->moff.size() - 1;
            size_t m = 0, seen = 0; uint32_t skip = (uint32_t)(in->bf.first_rec_voff & 0xFFFF);
            while (m < nm) {
                // every piece covers piece_members members of new ground; what the piece before left out (a read's last run) rides in front
                size_t end = seen;
                for (size_t fresh = 0; end < nm && fresh < piece_members; ++end) {      // (an empty member in the middle of a file is no new ground)
                    uint32_t isz; memcpy(&isz, in->bf.data + in->moff[end + 1] - 4, 4);
                    fresh += isz != 0;
                }
                size_t inflated = 0;
                for (size_t k = m; k < end; ++k) { uint32_t isz; memcpy(&isz, in->bf.data + in->moff[k + 1] - 4, 4); inflated += isz; }
                const int32_t more = end < nm ? 1 : 0;
                thj_bam_piece pc;
                pc.comp = in->bf.data + in->moff[m]; pc.comp_bytes = (int64_t)(in->moff[end] - in->moff[m]); pc.first_skip = skip;
                pc.n_tid = (int32_t)in->bf.tid2ref.size(); pc.tid2ref = in->bf.tid2ref.data();
                uint8_t* stage = stage_pieces({{&in->bf, &pc}});
                uint32_t rm = 0, rs = 0;
                const int r = call(pc, more, inflated, &rm, &rs);
                if (stage) thj_pinned_free(stage);
                if (r == THJ_EFALLBACK) { host_reason = thj_last_error(); return false; }
                if (r) die("Error: %s\n", thj_last_error());
                ++dev_pieces;
                if (!more) break;
                m += rm; skip = rs; seen = end;
            }
        }
        return true;
    };
    auto walk_pieces = [&](const PieceCall& call) -> bool { return walk_list(dev, 0, dev.size(), call); };
    auto add_on_device = [&]() -> bool {
        return walk_pieces([&](const thj_bam_piece& pc, int32_t more, size_t, uint32_t* rm, uint32_t* rs) { int64_t n = 0; return thj_juncbed_add_bam(ctx, &pc, max_report_intron, more, &n, rm, rs); });
    };
    // --accepted-hits-out: the output header's target of every contig (the @SQ lines of --sam-header, in file order)
    std::vector<int32_t> tid_of_ref;
    if (accepted) for (const std::string& name : rt.names) {
        int32_t t = -1;
        for (size_t k = 0; k < rt.sq.size() && t < 0; ++k) if (rt.sq[k].first == name) t = (int32_t)k;
        tid_of_ref.push_back(t);
    }
    // --accepted-hits-out, behind either replay: the context's BAM stream (total bytes, the records' sizes in p.size) is cut into BGZF members
    // from the sizes (bam_write1's bgzf_flush_try rule), deflated on the device and wrapped here; a member that does not deflate into 64 KiB:
    // the stream comes down and the host deflates it
    auto accepted_tail = [&](BamWriter& bw, BamWriter::Prepared& p, int64_t total) {
        const size_t n_rec = p.size.size();
        if (total) {
            p.device = true; p.rid.assign(n_rec, 0);
            BamWriter::plan_cuts_closed(p.size, p.cuts);
            std::vector<int64_t> ends(p.cuts.begin(), p.cuts.end());
            std::vector<uint32_t> clen(p.cuts.size()), crc(p.cuts.size());
            uint8_t* comp = (uint8_t*)thj_pinned_alloc(p.cuts.size() * (size_t)65536 + 64);
            if (!comp) die("Error: out of memory\n");
            int64_t comp_bytes = 0;
            const int erc = thj_bgzf_deflate(ctx, (int64_t)p.cuts.size(), ends.data(), comp, (int64_t)(p.cuts.size() * (size_t)65536), clen.data(), crc.data(), &comp_bytes);
            if (erc == THJ_OK) {
                p.members.resize(p.cuts.size());
                size_t at = 0;
                for (size_t i = 0; i < p.cuts.size(); ++i) {
                    BamWriter::wrap_member(comp + at, clen[i], crc[i], (uint32_t)(p.cuts[i] - (i ? p.cuts[i - 1] : 0)), p.members[i]);
                    at += clen[i];
                }
                bw.commit(p);
            } else if (erc == THJ_EFALLBACK) {
                fprintf(stderr, "accepted hits: a member does not deflate into a BGZF block on the device (%s); deflating on the host\n", thj_last_error());
                BamWriter::Encoded e;
                e.bytes.resize((size_t)total);
                if (thj_bam_stream_download(ctx, e.bytes.data())) die("Error: %s\n", thj_last_error());
                e.size = p.size; e.rid.assign(n_rec, 0);
                bw.write_encoded(e);
            } else die("Error: %s\n", thj_last_error());
            thj_pinned_free(comp);
        }
        bw.close();
        fprintf(stderr, "accepted hits: %zu records, %lld bytes of BAM records in %zu BGZF members\n", n_rec, (long long)total, p.cuts.size());
    };
    // --sort-bam, between the last report call and the tail: the stream's records in `samtools sort` order, their sizes with them
    auto sort_stream = [&](BamWriter::Prepared& p) {
        const auto t0 = std::chrono::steady_clock::now();
        int64_t n_blocks = 1;
        if (thj_bam_stream_sort(ctx, p.size.data(), (int64_t)p.size.size(), (int64_t)o.sort_max_mem, &n_blocks)) die("Error: %s\n", thj_last_error());
        fprintf(stderr, "sort bam: %zu records in %lld block%s (--sort-max-mem %lld), %.3f ms\n", p.size.size(), (long long)n_blocks, n_blocks == 1 ? "" : "s", o.sort_max_mem,
                std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
    };
    int64_t cap = 0, acc_bound = 0;                             // acc_bound: no more output records than this (--accepted-pairs-out)
    for (int attempt = 0;; ++attempt) {
        if (cap && thj_juncbed_configure(ctx, cap)) die("Error: %s\n", thj_last_error());
        if (thj_juncbed_reset_async(ctx)) die("Error: %s\n", thj_last_error());
        if (indels && thj_juncbed_collect_indels(ctx, 1)) die("Error: %s\n", thj_last_error());
        if (fusions && thj_juncbed_collect_fusions(ctx, 1, o.p.fusion_anchor_length, o.fusion_read_mismatches, o.fusion_multireads)) die("Error: %s\n", thj_last_error());
        // (every reset turns these two off: they are set again on every way through here, the host readers' second try included)
        if (!gtf.empty() && thj_juncbed_known_junctions(ctx, gtf.data(), (int64_t)gtf.size())) die("Error: %s\n", thj_last_error());
        if (o.read_filters && thj_juncbed_read_filter(ctx, 1, o.p.read_mismatches, o.p.read_gap_length, o.p.read_edit_dist)) die("Error: %s\n", thj_last_error());
        if (best && thj_juncbed_best_alignments(ctx, 1, o.max_multihits, o.suppress_hits ? 1 : 0, o.p.bowtie2_max_penalty)) die("Error: %s\n", thj_last_error());
        if (paired && thj_juncbed_pair_alignments(ctx, 1, o.p.inner_dist_mean, o.p.inner_dist_std_dev, o.p.fusion_min_dist, o.report_mixed ? 1 : 0, o.report_discordant ? 1 : 0)) die("Error: %s\n", thj_last_error());
        if (unmapped && thj_juncbed_collect_unmapped(ctx, 1, max_report_intron)) die("Error: %s\n", thj_last_error());
        if (accepted && (paired ? thj_juncbed_collect_accepted_pairs : thj_juncbed_collect_accepted)(ctx, 1, o.p.library_type, o.rg_id.c_str(), tid_of_ref.data(), (int32_t)tid_of_ref.size())) die("Error: %s\n", thj_last_error());
        if (device && !add_on_device()) {
            if (accepted) die("Error: %s (%s)\n", ACC_NEEDS, host_reason.c_str());
            device = false; --attempt; continue;               // a half-added input is never kept: reset, and the host readers
        }
        if (!route_said) {
            route_said = true;
            if (device) fprintf(stderr, "alignment records: parsed on the device for %zu piece%s\n", dev_pieces, dev_pieces == 1 ? "" : "s");
            else fprintf(stderr, "alignment records: read on the host (%s)\n", host_reason.c_str());
        }
        if (!device && !host_read) { host_read = true; read_on_host(); }
        if (paired) {
            // the files of a side in the order given; the numbers must not fall (the reference's BamMerge of several id-sorted files is not built);
            // the call takes the inserts' places in the merge of both sides' numbers
            std::vector<thj_aln> side[2];
            std::vector<int64_t> ioff[2]; std::string ibases[2];    // --insertions-out / --deletions-out: the inserted letters per side
            ioff[0].push_back(0); ioff[1].push_back(0);
            for (size_t k = 0; k < recs.size(); ++k) {
                const int sd = k < n_left_inputs ? 0 : 1;
                side[sd].insert(side[sd].end(), recs[k].recs.begin(), recs[k].recs.end());
                if (indels) { ibases[sd] += recs[k].bases; for (uint32_t x : recs[k].ins_n) ioff[sd].push_back(ioff[sd].back() + x); }
            }
            for (int sd = 0; sd < 2; ++sd)
                for (size_t i = 1; i < side[sd].size(); ++i)
                    if (side[sd][i].read_idx < side[sd][i - 1].read_idx)
                        die("Error: --right-maps: read number %u after %u on the %s side: the inputs of a side must be sorted by read number over all its files (BamMerge is not built)\n",
                            side[sd][i].read_idx, side[sd][i - 1].read_idx, sd ? "right" : "left");
            uint32_t place = 0;
            acc_bound = 0;
            std::vector<uint64_t> ins_numbers;                  // --left-reads: the inserts' numbers in visit order
            for (size_t i = 0, j = 0; i < side[0].size() || j < side[1].size(); ++place) {
                const uint64_t a = i < side[0].size() ? side[0][i].read_idx : ~0ull, b = j < side[1].size() ? side[1][j].read_idx : ~0ull, id = a < b ? a : b;
                const size_t i0 = i, j0 = j;
                if (unmapped) ins_numbers.push_back(id);
                for (; i < side[0].size() && side[0][i].read_idx == id; ++i) side[0][i].read_idx = place;
                for (; j < side[1].size() && side[1][j].read_idx == id; ++j) side[1][j].read_idx = place;
                // --accepted-pairs-out: an insert writes two records per reported pair (at most --max-multihits pairs), or its sides' records
                const uint64_t nl = i - i0, nr = j - j0, prs = std::min<uint64_t>(nl * nr, (uint64_t)o.max_multihits);
                acc_bound += (int64_t)std::max<uint64_t>(2 * prs, nl + nr);
            }
            if (indels ? thj_juncbed_add_pairs_seq(ctx, side[0].data(), (int64_t)side[0].size(), ioff[0].data(), ibases[0].c_str(), side[1].data(), (int64_t)side[1].size(), ioff[1].data(), ibases[1].c_str())
                       : thj_juncbed_add_pairs(ctx, side[0].data(), (int64_t)side[0].size(), side[1].data(), (int64_t)side[1].size())) die("Error: %s\n", thj_last_error());
            if (unmapped && thj_juncbed_read_numbers(ctx, ins_numbers.data(), (int64_t)ins_numbers.size())) die("Error: %s\n", thj_last_error());
        } else
        if (!device) for (auto& v : recs) {
            if (!indels) { if (thj_juncbed_add_records(ctx, v.recs.data(), (int64_t)v.recs.size(), 0)) die("Error: %s\n", thj_last_error()); }
            else {
                std::vector<int64_t> off(v.recs.size() + 1, 0);
                for (size_t i = 0; i < v.recs.size(); ++i) off[i + 1] = off[i] + v.ins_n[i];
                if (thj_juncbed_add_records_seq(ctx, v.recs.data(), (int64_t)v.recs.size(), off.data(), v.bases.data())) die("Error: %s\n", thj_last_error());
            }
            if (unmapped && thj_juncbed_read_numbers(ctx, v.numbers.data(), (int64_t)v.numbers.size())) die("Error: %s\n", thj_last_error());
        }
        int64_t n = 0;
        rc = thj_juncbed_finish(ctx, o.p.min_anchor_len, &n);
        if (rc == THJ_EOVERFLOW && attempt < 6) { cap = cap ? cap * 4 : (int64_t)1 << 22; continue; }     // more distinct junctions than the table holds
        if (rc) die("Error: %s\n", thj_last_error());
        if (paired) {
            int64_t pc[5] = {0, 0, 0, 0, 0};
            if (thj_juncbed_pair_counts(ctx, pc)) die("Error: %s\n", thj_last_error());
            fprintf(stderr, "paired alignments: %lld inserts with both sides, %lld with a pair reported, %lld over --max-multihits %d%s, %lld singletons, %lld reads without a mate's alignment left out%s\n",
                    (long long)pc[0], (long long)pc[1], (long long)pc[2], o.max_multihits, o.suppress_hits ? " (suppressed)" : "", (long long)pc[3], (long long)pc[4],
                    o.report_mixed ? "" : " (no --report-mixed-alignments)");
        } else if (best) {
            int64_t bc[4] = {0, 0, 0, 0};
            if (thj_juncbed_best_counts(ctx, bc)) die("Error: %s\n", thj_last_error());
            fprintf(stderr, "best alignments: %lld reads, %lld lost alignments to the choice, %lld over --max-multihits %d%s, %lld alignments counted once as first-pass duplicates\n",
                    (long long)bc[0], (long long)bc[1], (long long)bc[2], o.max_multihits, o.suppress_hits ? " (suppressed)" : "", (long long)bc[3]);
        }
        std::vector<thj_juncstat> js((size_t)n + 1);
        if (thj_juncbed_download(ctx, js.data())) die("Error: %s\n", thj_last_error());
        FILE* f = fopen(pos[1].c_str(), "w");
        if (!f) die("Error: cannot open %s for writing\n", pos[1].c_str());
        fprintf(f, "track name=junctions description=\"TopHat junctions\"\n");
        for (int64_t i = 0; i < n; ++i) {
            const thj_juncstat& j = js[(size_t)i];
            const int start = (int)j.left + 1 - (int)j.left_extent, end = (int)j.right + (int)j.right_extent;
            fprintf(f, "%s\t%d\t%d\tJUNC%08d\t%d\t%c\t%d\t%d\t255,0,0\t2\t%d,%d\t0,%d\n", rt.names[j.ref_id - 1].c_str(), start, end, (int)(i + 1), (int)j.support,
                    j.antisense ? '-' : '+', start, end, (int)j.left_extent, (int)j.right_extent, (int)j.right - start);
        }
        close_output(f, "junctions.bed");
        if (indels) {
            int64_t n_ins = 0, n_del = 0;
            if (thj_juncbed_indel_counts(ctx, &n_ins, &n_del)) die("Error: %s\n", thj_last_error());
            std::vector<thj_insstat> ins((size_t)n_ins + 1);
            std::vector<thj_juncstat> dels((size_t)n_del + 1);
            if (thj_juncbed_indel_download(ctx, ins.data(), dels.data())) die("Error: %s\n", thj_last_error());
            if (!o.insertions_out.empty()) {
                FILE* fi = fopen(o.insertions_out.c_str(), "w");
                if (!fi) die("Error: cannot open %s for writing\n", o.insertions_out.c_str());
                fprintf(fi, "track name=insertions description=\"TopHat insertions\"\n");
                for (int64_t i = 0; i < n_ins; ++i) {
                    const thj_insstat& x = ins[(size_t)i];
                    fprintf(fi, "%s\t%d\t%d\t%.*s\t%d\n", rt.names[x.ref_id - 1].c_str(), (int)x.left, (int)x.left, (int)x.len, x.bases, (int)(x.support > 1000 ? 1000 : x.support));
                }
                close_output(fi, "insertions.bed");
            }
            if (!o.deletions_out.empty()) {
                FILE* fd = fopen(o.deletions_out.c_str(), "w");
                if (!fd) die("Error: cannot open %s for writing\n", o.deletions_out.c_str());
                fprintf(fd, "track name=deletions description=\"TopHat deletions\"\n");
                for (int64_t i = 0; i < n_del; ++i) {
                    const thj_juncstat& x = dels[(size_t)i];
                    fprintf(fd, "%s\t%d\t%d\t-\t%d\n", rt.names[x.ref_id - 1].c_str(), (int)(x.left + 1), (int)x.right, (int)x.support);
                }
                close_output(fd, "deletions.bed");
            }
        }
        if (fusions) {
            int64_t n_fus = 0;
            if (thj_juncbed_fusion_count(ctx, &n_fus)) die("Error: %s\n", thj_last_error());
            std::vector<thj_fusstat> fs((size_t)n_fus + 1);
            if (thj_juncbed_fusion_download(ctx, fs.data())) die("Error: %s\n", thj_last_error());
            FILE* ff = fopen(o.fusions_out.c_str(), "w");
            if (!ff) die("Error: cannot open %s for writing\n", o.fusions_out.c_str());
            for (int64_t i = 0; i < n_fus; ++i) {               // print_fusions, fusions.cpp:347-433
                const thj_fusstat& x = fs[(size_t)i];
                float symm = 0.0f;
                for (int k = 0; k < 50; ++k) { const float term = ((int)x.left_bases[k] - (int)x.right_bases[k]) / (float)(int)x.count; symm += (term * term); }
                fprintf(ff, "%s-%s\t%d\t%d\t%s\t%d\t%d\t%d\t%d\t%d\t%d\t%.6f", rt.names[x.ref_id1 - 1].c_str(), rt.names[x.ref_id2 - 1].c_str(), (int)x.left, (int)x.right,
                        x.dir == THJ_CIG_FUSION_FF ? "ff" : x.dir == THJ_CIG_FUSION_FR ? "fr" : x.dir == THJ_CIG_FUSION_RF ? "rf" : "rr", (int)x.count, 0, 0, (int)x.unsupport,
                        (int)x.left_ext, (int)x.right_ext, symm);
                fprintf(ff, "\t@\t");
                for (uint32_t k = 0; k < x.n_diffs && k < 5; ++k) fprintf(ff, "%d ", (int)x.diffs[k]);
                fprintf(ff, "\t@\t");
                const int half = x.n_diffs ? 50 : 0;             // the two strings, each as two halves; none near a contig end
                fprintf(ff, "%.*s %.*s\t@\t", half, x.seq1, half, x.seq1 + half);
                fprintf(ff, "%.*s %.*s\t@\t", half, x.seq2, half, x.seq2 + half);
                for (int k = 0; k < 50; ++k) fprintf(ff, "%d ", (int)x.left_bases[k]);
                fprintf(ff, "\t@\t");
                for (int k = 0; k < 50; ++k) fprintf(ff, "%d ", (int)x.right_bases[k]);
                fprintf(ff, "\t@\t\n");                         // the pair list: empty
            }
            close_output(ff, "fusions.out");
        }
        if (accepted && paired) {
            // the records the add call was given, a side each, from their own bytes (kept while reading): the device lays the inserts' reported
            // records out, rewrites them into the context's BAM stream and hands back their sizes.  One call: the room for the sizes comes from a
            // bound worked out while the inserts were merged (the call that only counts would upload and lay out everything a second time)
            std::vector<uint8_t> raw[2]; std::vector<int64_t> roff[2];
            roff[0].push_back(0); roff[1].push_back(0);
            for (size_t k = 0; k < recs.size(); ++k) {
                const int sd = k < n_left_inputs ? 0 : 1;
                raw[sd].insert(raw[sd].end(), recs[k].raw.begin(), recs[k].raw.end());
                for (uint32_t len : recs[k].raw_len) roff[sd].push_back(roff[sd].back() + (int64_t)len);
            }
            BamWriter bw;
            if (!bw.open(accepted_out, rt, "")) die("Error: cannot open %s for writing\n", accepted_out.c_str());
            BamWriter::Prepared p;
            int64_t total = 0, n_out = 0;
            const int64_t nl = (int64_t)roff[0].size() - 1, nr = (int64_t)roff[1].size() - 1;
            if (nl + nr > 0) {
                p.size.resize((size_t)acc_bound + 1);
                if (thj_juncbed_report_pairs_bam(ctx, raw[0].data(), roff[0].data(), nl, raw[1].data(), roff[1].data(), nr, p.size.data(), acc_bound + 1, &n_out, &total)) die("Error: %s\n", thj_last_error());
                p.size.resize((size_t)n_out);
            }
            if (o.sort_bam) sort_stream(p);
            accepted_tail(bw, p, total);
        } else if (accepted) {
            // the inputs once more, piece for piece as they were added: the device rewrites the reported records into the context's BAM
            // stream and hands back their sizes
            BamWriter bw;
            if (!bw.open(accepted_out, rt, "")) die("Error: cannot open %s for writing\n", accepted_out.c_str());
            BamWriter::Prepared p;
            int64_t total = 0;
            const bool all = walk_pieces([&](const thj_bam_piece& pc, int32_t more, size_t inflated, uint32_t* rm, uint32_t* rs) {
                const size_t at = p.size.size(), room = inflated / 36 + 1;       // a record takes its block_size and 32 fixed bytes at least
                p.size.resize(at + room);
                int64_t n_out = 0;
                const int r = thj_juncbed_report_bam(ctx, &pc, max_report_intron, more, &n_out, rm, rs, p.size.data() + at, (int64_t)room, &total);
                p.size.resize(at + (r ? 0 : (size_t)n_out));
                return r;
            });
            if (!all) die("Error: %s (%s)\n", ACC_NEEDS, host_reason.c_str());
            if (o.sort_bam) sort_stream(p);
            accepted_tail(bw, p, total);
        }
        if (unmapped) {
            // the reads files, a side after the other, piece for piece: the device decides every read, counts it and writes the unmapped ones into
            // the context's BAM stream; the stream goes out through the accepted hits' tail when the side has an output file
            for (size_t sd = 0; sd < reads_in.size(); ++sd) {
                BamWriter::Prepared p;
                int64_t total = 0;
                bool called = false;
                const bool all = walk_list(reads_in, sd, sd + 1, [&](const thj_bam_piece& pc, int32_t more, size_t inflated, uint32_t* rm, uint32_t* rs) {
                    const size_t at = p.size.size(), room = inflated / 36 + 1;
                    p.size.resize(at + room);
                    int64_t n_out = 0;
                    called = true;
                    const int r = thj_juncbed_report_unmapped_bam(ctx, (int32_t)sd, &pc, more, &n_out, rm, rs, p.size.data() + at, (int64_t)room, &total);
                    p.size.resize(at + (r ? 0 : (size_t)n_out));
                    return r;
                });
                if (!all) die("Error: --left-reads / --right-reads: the reads file's records straddle BGZF members; reading it on the host is not built (%s)\n", host_reason.c_str());
                if (!called) {                                  // a reads file without a record: the side ends all the same
                    thj_bam_piece none; memset(&none, 0, sizeof none);
                    int64_t n_out = 0; uint32_t rm = 0, rs = 0; uint32_t room = 0;
                    if (thj_juncbed_report_unmapped_bam(ctx, (int32_t)sd, &none, 0, &n_out, &rm, &rs, &room, 1, &total)) die("Error: %s\n", thj_last_error());
                }
                const std::string& out = sd ? o.unmapped_right_out : o.unmapped_left_out;
                fprintf(stderr, "%s reads: %zu unmapped records\n", sd ? "right" : "left", p.size.size());
                if (out.empty()) continue;
                BamWriter bw;
                if (!bw.open(out, rt, "")) die("Error: cannot open %s for writing\n", out.c_str());
                accepted_tail(bw, p, total);
            }
            int64_t st[15];
            if (thj_juncbed_align_stats(ctx, st)) die("Error: %s\n", thj_last_error());
            if (!o.align_summary_out.empty()) {
                FILE* fa = fopen(o.align_summary_out.c_str(), "w");
                if (!fa) die("Error: cannot open %s for writing\n", o.align_summary_out.c_str());
                print_align_summary(fa, st, o.max_multihits);
                close_output(fa, "align_summary.txt");
            }
        }
        break;
    }
    finish_outputs_complete(0);
}

int main(int argc, char** argv) { return run_with_handoff(argc, argv, real_main); }
