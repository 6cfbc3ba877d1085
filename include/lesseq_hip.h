/*
 * lesseq_hip.h -- C ABI of the MI355X-native count + solve path of LESSeq.
 *
 * The reference (gersteinlab/LESSeq) has no plugin / FFI seam: its `count` and `solve`
 * programs are monolithic main() bodies (count/count.cpp:88-501, solve/solve.cpp:102-856).
 * This header is the seam a maintainer would cut: each entry point replaces a contiguous
 * stretch of those main() bodies, cited per function.  INTEGRATION.md shows the call sites.
 *
 * Conventions: plain C, caller-owned buffers, no exceptions across the boundary (every entry
 * point that can allocate catches what is thrown below it and returns LSQ_E_INTERNAL; helper
 * threads are joined on every way out).  Every
 * function returns LSQ_OK (0) or a negative lsq_status; lsq_last_error() gives the text for
 * the calling thread.  Coordinates are 0-based half-open, as the reference holds them after
 * `start - 1` (count/count.cpp:319,323).  One lsq_ctx per GPU, used from one host thread.
 *
 * Two groups:
 *   host-only  (no GPU touched): annotation loading, event compilation, MRF parsing,
 *              text formatting, the synthetic workload generator;
 *   device     (HIP, gfx950):    context, uploads, the count and EM kernels, result fetch.
 * There is no CPU implementation of the device group: without a usable GPU these calls
 * fail with LSQ_E_DEVICE.  (Two things inside the device group do run on the host, on reads that were
 * filtered and pooled on the device: the exact-order EM of guard-band events, and genes beyond the
 * kernel limits below -- lesseq_amd/csrc/lsq_replay.hip.)
 */
#ifndef LESSEQ_HIP_H
#define LESSEQ_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LSQ_ABI_VERSION 2

typedef enum {
	LSQ_OK = 0,
	LSQ_E_ARG = -1,          /* bad argument / malformed table */
	LSQ_E_IO = -2,           /* file cannot be opened / read */
	LSQ_E_FORMAT = -3,       /* unknown file format / read type literal (reference: exit 1) */
	LSQ_E_PARSE = -4,        /* lexical_cast failure (reference: exit 1) */
	LSQ_E_RANGE = -5,        /* coordinate or size outside what the device tables hold */
	LSQ_E_UNSUPPORTED = -6,  /* event shape outside the device kernels' limits */
	LSQ_E_DEVICE = -7,       /* HIP error, or no gfx950 device */
	LSQ_E_STATE = -8,        /* call order violated (e.g. count before uploads) */
	LSQ_E_INTERNAL = -9,     /* out of memory, or a C++ exception caught at the boundary (never thrown across it) */
	LSQ_E_TIMEOUT = -10      /* lsq_ctx_synchronize_for: the context's streams had not drained when the time was up */
} lsq_status;

/* kernel limits (what the count and EM kernels hold in registers / LDS per event) */
#define LSQ_MAX_SEGMENTS 32   /* atomic exon segments per event (LESSeq local events: <= 4) */
#define LSQ_MAX_ISOFORMS 6    /* isoforms per event (LESSeq local events: 2) */
#define LSQ_MAX_METHODS 8     /* read files ("sampling methods") per run */
/* Genes beyond the two kernel limits above are not refused: they are evaluated on the host inside lsq_count / lsq_solve
 * (same rules, the reference's own per-read EM; those calls then block).  The hard limits are 64 segments and: */
#define LSQ_HOST_MAX_ISOFORMS 16

const char *lsq_last_error(void);
int lsq_abi_version(void);
/* The library's own warnings (e.g. "the exception list of read file m overflowed: every read was counted again") go to stderr in
 * the reference's log format (jsc/util/log.hpp:22-79, "[LOG date time WARNING] text") when level >= 1; default 2, like the
 * reference's reporting level; the executables pass their log_level argument on. */
void lsq_set_log_level(int level);

/* ------------------------------------------------------------------------------------
 * Host-only group
 * ------------------------------------------------------------------------------------ */

typedef struct lsq_annotation lsq_annotation;   /* selected genes + their isoform records */
typedef struct lsq_events lsq_events;           /* compiled event tables (host copy) */
typedef struct lsq_reads lsq_reads;             /* parsed reads of one MRF file, file order */

/* Replaces count/count.cpp:135-216 and solve/solve.cpp:152-329: loads the isoforms and the
 * gene -> isoform map, selects genes whose index in the bytewise-sorted gene-name set lies in
 * [gene_begin_idx, gene_end_idx).  Isoform formats: "LH_GENE_TXT" (the only one `count` and
 * `classify` take), and solve's "UCSC_GENE_TXT" (jsc/bioinfo/gene_anno.hpp:59-117),
 * "UCSC_GFF", "WORMBASE_GFF2", "GENELETS_GFF3" (one line per exon; an isoform's exons are
 * merged with interval_list::add_interval in file order, solve/solve.cpp:160-296).  Map
 * formats: "UCSC_GENE2ISOFORM", and solve's "WORMBASE_GENE2ISOFORMS" (gene iso1;iso2;...).
 * Any other literal gives LSQ_E_FORMAT; the executables keep count/classify to their two. */
int lsq_annotation_load(const char *isoform_format, const char *isoforms_path,
                        const char *g2i_format, const char *g2i_path,
                        uint64_t gene_begin_idx, uint64_t gene_end_idx,
                        lsq_annotation **out);
void lsq_annotation_free(lsq_annotation *a);
int64_t lsq_annotation_num_genes(const lsq_annotation *a);      /* selected genes */
int64_t lsq_annotation_num_isoforms_loaded(const lsq_annotation *a);
int64_t lsq_annotation_num_genes_loaded(const lsq_annotation *a);

/* Replaces count/count.cpp:231-258 + the per-gene ARS construction at :394-416
 * (common/splicing_graph.h:88-169,235-252,318-361; common/accessible_read_starts.h:48-89,
 * 221-274; jsc/util/interval_list.hpp:462-503): atomic segments, isoform masks, event
 * spans, per-chromosome covered regions, and for each of the n_methods read files the
 * per-isoform ARS total.  read_types[m] is "SHORT_READ" or "MEDIUM_READ" (LSQ_E_FORMAT
 * otherwise, the reference's unknown_readtype_err). */
int lsq_events_compile(const lsq_annotation *a, int n_methods, const char *const *read_types,
                       const uint64_t *expected_read_lengths, lsq_events **out);
/* The library type of a job.  Unstranded: a read counts for every event it overlaps, whatever their strands --
 * the reference's behaviour, and what lsq_events_compile gives.  Forward and reverse: a read has a transcript strand
 *   t = s XOR (library == reverse) XOR mate2
 * (s: the alignment strand -- the strand column of an MRF block, which must be exactly "+" or "-", FLAG & 0x10 of a SAM / BAM
 * record; mate2: (FLAG & 0x1) && (FLAG & 0x80) of a SAM / BAM record, false for every other format) and counts only for events
 * of that strand: the job's table is, row by row, the table of the unstranded job of the plus genes on the t = "+" reads and of
 * the unstranded job of the minus genes on the t = "-" reads.  A read without a transcript strand (a strand string that is
 * neither "+" nor "-") makes no read.  forward is htseq-count's -s yes, reverse its -s reverse (the dUTP protocols). */
#define LSQ_LIBRARY_UNSTRANDED 0
#define LSQ_LIBRARY_FORWARD 1
#define LSQ_LIBRARY_REVERSE 2
/* "unstranded", "forward" or "reverse" to its number; -1 for any other string. */
int lsq_library_from_name(const char *name);
/* lsq_events_compile for a job of the given library type.  The library type is a property of the compiled events: in a
 * stranded compile the covered regions, the clusters, the buckets and the loader's tables are kept per (chromosome, strand),
 * so that events of opposite strands never share a bucket and everything behind the loader runs as it does unstranded.  A
 * selected gene whose isoforms do not all carry the same one of "+" / "-" cannot be placed: LSQ_E_UNSUPPORTED, the message
 * names the first such gene and says how many there are (an unstranded compile takes them).  LSQ_E_RANGE beyond 32 767
 * chromosomes.  LSQ_LIBRARY_UNSTRANDED: exactly lsq_events_compile.
 * Every upload call of a context that holds stranded events (lsq_reads_upload, lsq_reads_upload_mrf, lsq_reads_upload_text...)
 * routes by transcript strand; wherever the pipeline uses a read's strand, the read then carries its transcript strand's string.
 * Parsed arrays have no room for the mate bits, so under stranded events lsq_sam_parse, lsq_bam_parse(_checked) and
 * lsq_mrf_parse_device write s XOR mate2 as a SAM / BAM record's strand -- what the record's MRF form holds -- and
 * lsq_reads_upload derives t from the strand id of a read's first block (an id other than those of "+" and "-": no read).
 * lsq_reads_parse drops, for the name-keyed formats, the lines the containment filter of the line's transcript strand drops, and
 * makes a name whose lines lie on both transcript strands a read per strand (an upload routes a read by one strand). */
int lsq_events_compile_library(const lsq_annotation *a, int n_methods, const char *const *read_types,
                               const uint64_t *expected_read_lengths, int library, lsq_events **out);
int lsq_events_library(const lsq_events *e);
void lsq_events_free(lsq_events *e);

/* read-only views into compiled events, in output order (bytewise-sorted gene names) */
int64_t lsq_events_count(const lsq_events *e);
int64_t lsq_events_total_isoforms(const lsq_events *e);
const char *lsq_events_gene_name(const lsq_events *e, int64_t ev);
const char *lsq_events_chrom(const lsq_events *e, int64_t ev);
const char *lsq_events_strand(const lsq_events *e, int64_t ev);
int lsq_events_num_isoforms(const lsq_events *e, int64_t ev);
int lsq_events_num_segments(const lsq_events *e, int64_t ev);
const char *lsq_events_isoform_name(const lsq_events *e, int64_t ev, int iso);
/* segment n of the event as [start,end); isoform mask bit n set iff the isoform holds it */
int lsq_events_segment(const lsq_events *e, int64_t ev, int n, int64_t *start, int64_t *end);
uint64_t lsq_events_isoform_mask(const lsq_events *e, int64_t ev, int iso);
uint64_t lsq_events_isoform_length(const lsq_events *e, int64_t ev, int iso);
uint64_t lsq_events_ars(const lsq_events *e, int method, int64_t ev, int iso);
int lsq_events_span(const lsq_events *e, int64_t ev, int64_t *gene_start, int64_t *gene_end);
int64_t lsq_events_num_buckets(const lsq_events *e);
int64_t lsq_events_lds_table_bytes(const lsq_events *e);   /* largest bucket image + histogram */
int64_t lsq_events_host_genes(const lsq_events *e);        /* genes beyond the kernel limits below: evaluated on the host (lsq_host_evaluated) */
/* Restricts the device plan to events [first_event, first_event + n_events) of the output order
 * (the reference's own scale-out unit, count/count.cpp:204-215) while the covered regions -- and so
 * the load-time read filter -- stay those of the whole selected range: every shard then gives
 * exactly the rows the unsharded run gives for its events.  Call before lsq_events_upload. */
int lsq_events_set_shard(lsq_events *e, uint64_t first_event, uint64_t n_events);

/* Replaces count/count.cpp:279-336 (== solve/solve.cpp:429-486) minus the containment
 * filter: parses an MRF_SINGLE file into blocks in file order.  A lexical_cast failure
 * gives LSQ_E_PARSE; a format literal other than "MRF_SINGLE" LSQ_E_FORMAT.  Chromosome and
 * strand strings are interned against the events' dictionaries (unknown chromosomes get an
 * id that matches no covered region). n_threads <= 0 picks the host's core count. */
int lsq_mrf_parse(const char *read_format, const char *path, lsq_events *e,
                  int n_threads, lsq_reads **out);
/* The same for any read format the reference's `solve` takes (solve/solve.cpp:413-634): "MRF_SINGLE"
 * (this is then lsq_mrf_parse), and the name-keyed "UCSC_GFF" (a line per block), "UCSC_BED" (a line
 * per read, kept or dropped as a whole by its span) and "WORMBASE_GFF3" (a line per read with an
 * optional intron).  Lines of one name make one read; its names decide span-start ties against gene
 * names (solve/solve.cpp:70-98).  `count` takes MRF_SINGLE only, as in the reference. */
int lsq_reads_parse(const char *read_format, const char *path, lsq_events *e, int n_threads, lsq_reads **out);
/* "SAM_SINGLE": alignments as an aligner writes them, taken wherever "MRF_SINGLE" is (lsq_reads_parse, lsq_reads_upload_mrf,
 * lsq_reads_upload_text, lsq_reads_upload_text_at, lsq_mrf_parse_device, the read_format slot of count and solve).  The format
 * is DEFINED by its MRF_SINGLE equivalent (lesseq_amd/csrc/lsq_sam_line.hpp is the one statement of the
 * rules): SAM line k, every line counted, is the read "read-<k>"; '@' lines, records with FLAG & skip_flags, MAPQ <
 * min_mapq, RNAME "*", POS 0, CIGAR "*" or no block make no read; M = X D extend a block, N splits, I S move the query
 * only, H P do nothing; the strand is FLAG & 0x10.  Every record is a read of its own (mates are not paired).
 * lsq_sam_parse replaces what a foreign sam2mrf run followed by count/count.cpp:279-336 does: the arrays lsq_mrf_parse
 * gives for the equivalent MRF file.  LSQ_E_PARSE with "#<k>:<line>" for the first malformed line (fewer than six fields,
 * FLAG / MAPQ / POS not an unsigned decimal in range, a CIGAR of another shape, a reference end beyond 2^31-1).
 * lsq_reads_parse("SAM_SINGLE") calls it with the defaults below. */
#define LSQ_SAM_DEFAULT_SKIP_FLAGS 0x904u   /* unmapped, secondary, supplementary */
#define LSQ_SAM_DEFAULT_MIN_MAPQ 0u
int lsq_sam_parse(const char *path, lsq_events *e, unsigned skip_flags, unsigned min_mapq, int n_threads, lsq_reads **out);
/* Defines the equivalence: the MRF_SINGLE text of a SAM text -- "AlignmentBlocks", then one line per SAM line that ends
 * in '\n': "#" for a line that makes no read, else its blocks RNAME:<strand>:<s>:<e>:<qs>:<qe> joined by ','.  The
 * reference's count and solve on that text are what count and solve here print for the SAM file.  *mrf_text is malloc'd
 * and NUL-terminated (lsq_free); *mrf_len (may be null) its length.  Status as lsq_sam_parse.  The sam2mrf executable
 * wraps this call. */
int lsq_sam_to_mrf(const void *sam_bytes, uint64_t len, unsigned skip_flags, unsigned min_mapq, char **mrf_text, uint64_t *mrf_len);
/* "BAM_SINGLE": the same alignments as aligners and `samtools sort` hand them over, taken wherever "SAM_SINGLE" is.  The
 * format is DEFINED by its SAM equivalent (lesseq_amd/csrc/lsq_bam_record.hpp): the text `samtools view -h`
 * prints -- the lines of the header text, then a line per record in file order, RNAME the name of refID ("*" for -1), POS
 * pos + 1, CIGAR from the operations ("*" for none) -- under the rules and the two filters of SAM_SINGLE.  Record i (from 0) is
 * the read "read-<h + i + 1>", h the lines of the header text.  The BGZF blocks are inflated by the library's own decoder (no
 * zlib).  The CRC32 of a block and the end-of-file marker are checked where a caller asks for it -- the _checked entries below,
 * the context option "bam_verify", lsq_bam_check -- and nowhere else.  LSQ_E_FORMAT, naming the block's file offset, for a file that is not BGZF or BAM (bad
 * magic, no BC subfield, BSIZE past the end, an invalid deflate stream, other than ISIZE bytes); LSQ_E_PARSE with
 * "#<k>:<BAM record at byte N of the inflated stream>" for the first malformed record (block_size < 32, l_read_name 0, name and
 * CIGAR beyond block_size, refID outside -1 .. n_ref-1, an operation code above 8, a record past the end of the stream, POS or
 * a reference end beyond 2^31-1).  A CIGAR kept in the CG tag (more than 65 535 operations) is read as stored and makes no
 * read; CRAM and mate pairing are out of scope.  lsq_reads_parse("BAM_SINGLE") calls lsq_bam_parse with the SAM defaults. */
int lsq_bam_parse(const char *path, lsq_events *e, unsigned skip_flags, unsigned min_mapq, int n_threads, lsq_reads **out);
/* The MRF_SINGLE text of a BAM file's bytes, as lsq_sam_to_mrf gives it for the equivalent SAM text ("#" for every header line).
 * The bam2mrf executable wraps this call. */
int lsq_bam_to_mrf(const void *bam_bytes, uint64_t len, unsigned skip_flags, unsigned min_mapq, char **mrf_text, uint64_t *mrf_len);
/* The same two calls with the file verified on the way, as samtools and htslib do: behind the block chain and the deflate
 * streams, and ahead of the header and the records, LSQ_E_FORMAT with "CRC32 mismatch (stored 0x%08x, computed 0x%08x) in the
 * BGZF block at file offset N: ..." for the first block in file order whose bytes do not give the CRC-32 it stores, then with
 * "no end-of-file marker in the BGZF block at file offset <file length>: ..." for a file whose last 28 bytes are not the empty
 * BGZF block (a file cut at a block boundary).  On the device chain (lsq_reads_upload_mrf, lsq_reads_upload_text,
 * lsq_mrf_parse_device with "BAM_SINGLE") lsq_ctx_set_option("bam_verify", 1) asks for the same checks, same order, same
 * messages: a pass of its own behind the inflate ("bgzf_crc32" in lsq_last_ingest_stages), a wave a BGZF block.  Default 0:
 * nothing is checked and the stage list is the unverified one. */
int lsq_bam_parse_checked(const char *path, lsq_events *e, unsigned skip_flags, unsigned min_mapq, int n_threads, lsq_reads **out);
int lsq_bam_to_mrf_checked(const void *bam_bytes, uint64_t len, unsigned skip_flags, unsigned min_mapq, char **mrf_text, uint64_t *mrf_len);
/* A whole BAM file checked without an annotation (the bamcheck executable): block chain, deflate streams, CRC32s, end-of-file
 * marker, header, every record -- the statuses and messages above, always verifying.  records / reads / read_blocks: the lines
 * lsq_bam_to_mrf prints behind the header's, those of them that are not "#", and their blocks, under the context's
 * sam_skip_flags / sam_min_mapq (lsq_bam_check_host: the defaults).  lsq_bam_check runs the device chain on a context that
 * needs no events; blocks_repaired as lsq_last_bam_paths (0 from lsq_bam_check_host). */
typedef struct { uint64_t file_bytes, blocks, inflated_bytes, header_lines, references, records, reads, read_blocks, blocks_repaired; } lsq_bam_report;
int lsq_bam_check_host(const char *path, int n_threads, lsq_bam_report *r);
/* Wraps caller-made arrays as a read set without copying (the arrays must outlive it).
 * blk_off has n_reads+1 entries; blocks are 0-based half-open; chrom_id / strand_id index
 * lsq_events_chrom_id() / lsq_events_strand_id() dictionaries; line_no is the 1-based line
 * number after the header (read name "read-<line_no>", count/count.cpp:293-295). */
int lsq_reads_wrap(uint64_t n_reads, const uint64_t *blk_off, const uint32_t *line_no,
                   const int32_t *blk_start, const int32_t *blk_end,
                   const uint16_t *blk_chrom_id, const uint8_t *blk_strand_id, lsq_reads **out);
void lsq_reads_free(lsq_reads *r);
uint64_t lsq_reads_count(const lsq_reads *r);
uint64_t lsq_reads_num_blocks(const lsq_reads *r);
int lsq_events_chrom_id(lsq_events *e, const char *chrom);     /* interns; >= 0 */
int lsq_events_strand_id(lsq_events *e, const char *strand);   /* interns; >= 0 */
const char *lsq_events_strand_name(const lsq_events *e, int strand_id);   /* NULL when unknown */
/* The arrays of a read set (lsq_reads_wrap's layout); they live as long as the read set. */
int lsq_reads_arrays(const lsq_reads *r, const uint64_t **blk_off, const uint32_t **line_no,
                     const int32_t **blk_start, const int32_t **blk_end,
                     const uint16_t **blk_chrom_id, const uint8_t **blk_strand_id);

/* ------------------------------------------------------------------------------------
 * Device group
 * ------------------------------------------------------------------------------------ */

typedef struct lsq_ctx lsq_ctx;

int lsq_ctx_create(int device_id, lsq_ctx **out);
/* The same with flags.  LSQ_CTX_LANES_IN_BACKGROUND: only the upload stream is made before the call returns; the step lanes' streams
 * and events (0.04 s of runtime calls) are made by a helper thread, which the first call that needs a lane -- lsq_events_upload
 * comes ahead of all of them -- or lsq_ctx_destroy joins.  lsq_text_stage needs no lane: an executable copies its reads to HBM meanwhile. */
#define LSQ_CTX_LANES_IN_BACKGROUND 1u
int lsq_ctx_create_with(int device_id, unsigned flags, lsq_ctx **out);
void lsq_ctx_destroy(lsq_ctx *c);
/* The context works on HIP streams of its own.  Uploads and ingest run on one (returned here as hipStream_t in a
 * void*).  A step -- lsq_count, lsq_solve, the hand-off of its results -- runs on one of two LANES that consecutive
 * lsq_count calls take in turn: a lane has a count stream (the streaming kernels), a result stream (exception pass, EM,
 * lsq_results_copy_device / lsq_results_pack_device, behind an event recorded after the count), a counter set and the
 * EM's output arrays.  These calls only submit work; step k+1's count runs beside step k's EM.  Hence two rules for a
 * host that submits steps without waiting in between:
 *   - lsq_ctx_result_stream names the LATEST count's lane: ask again after every lsq_count, never cache it;
 *   - the device buffers handed to consecutive unsynchronised steps (d_block / d_gathered of lsq_step_gather, the
 *     arguments of lsq_results_copy_device) must be DISTINCT -- two of each, alternated, as the lanes are: step k+1's
 *     pack runs on the other lane and is not ordered behind a collective that still reads step k's block.
 * lsq_ctx_synchronize waits for all of the context's streams; the host-side result getters do so themselves. */
void *lsq_ctx_stream(lsq_ctx *c);
int lsq_ctx_synchronize(lsq_ctx *c);
/* The same with a time limit (seconds): LSQ_E_TIMEOUT when work is still queued after it -- e.g. a collective of a
 * multi-GPU job (lesseq_rccl.h) whose peer never arrived; the caller then aborts the communicator (lsq_comm_abort)
 * instead of waiting for ever.  Polls the streams; nothing is cancelled by the call itself. */
int lsq_ctx_synchronize_for(lsq_ctx *c, double seconds);

/* Uploads the compiled tables: per-bucket LDS images (bin directory, event records,
 * segments, isoform masks), tie-break records and G = 1/ARS. */
int lsq_events_upload(lsq_ctx *c, lsq_events *e);

/* Replaces the retained-read state the reference builds at count/count.cpp:319-324 and
 * :348-364.  The parsed blocks are copied to the device as they are; HIP kernels apply the
 * per-block containment filter against the covered regions, merge kept blocks with
 * interval_list::add_interval semantics, and store each retained read in the bucket of its
 * first kept base, split into 1-block / 2-block / n-block pools (structure-of-arrays in
 * HBM).  A read may keep at most 16 separate blocks (LSQ_E_RANGE beyond).  method in
 * [0, n_methods). */
int lsq_reads_upload(lsq_ctx *c, int method, const lsq_reads *r);
/* The same, from the MRF_SINGLE text itself: replaces count/count.cpp:279-336 and :348-364 in one
 * call.  The file's bytes are copied to HBM and parsed there (newline scan, one lane per line, the
 * reference's find/substr field arithmetic and lexical_cast<long> rules), then ingested as above;
 * no parsed array ever exists on the host.  Status as lsq_mrf_parse (LSQ_E_FORMAT, LSQ_E_PARSE with
 * the first failing line in lsq_last_error(), LSQ_E_IO); LSQ_E_UNSUPPORTED when the file holds a
 * strand string longer than 7 bytes (lsq_mrf_parse + lsq_reads_upload take those). */
int lsq_reads_upload_mrf(lsq_ctx *c, int method, const char *read_format, const char *path);
/* The same in two steps, for callers that want the copy under way before the event tables exist (the
 * executables start it on a second thread while the annotation is still being read):
 * lsq_text_stage copies the file's bytes to HBM and needs only the context; lsq_reads_upload_text
 * parses and ingests them (status as lsq_reads_upload_mrf).  The text may be freed afterwards. */
typedef struct lsq_text lsq_text;
int lsq_text_stage(lsq_ctx *c, const char *path, lsq_text **out);
void lsq_text_free(lsq_text *t);
int lsq_reads_upload_text(lsq_ctx *c, int method, const char *read_format, lsq_text *t);
/* A slice of a file for one of several processes that share it (lesseq_amd/dist.py::run_read_sharded):
 * the bytes [byte_begin, byte_end), which must start on a line boundary; lsq_text_lines counts its
 * newlines (so that every process can work out the file-wide number of its first line: read names are
 * "read-<line>", count/count.cpp:293-295); lsq_reads_upload_text_at parses it with has_header = 1 only
 * for the slice that holds the file's first line, first_line = the number of its first data line. */
int lsq_text_stage_range(lsq_ctx *c, const char *path, uint64_t byte_begin, uint64_t byte_end, lsq_text **out);
int lsq_text_lines(lsq_ctx *c, lsq_text *t, uint64_t *n_newlines);
int lsq_reads_upload_text_at(lsq_ctx *c, int method, const char *read_format, lsq_text *t, int has_header, uint64_t first_line);
/* The device parser's blocks copied back to the host (same arrays lsq_mrf_parse makes; for tools
 * and tests).  Needs lsq_events_upload first. */
int lsq_mrf_parse_device(lsq_ctx *c, const char *read_format, const char *path, lsq_reads **out);
/* milliseconds of the last device parse: host-to-device copy of the text, and the parse kernels */
int lsq_last_mrf_timing(lsq_ctx *c, float *h2d_ms, float *parse_ms);
/* The loader as a chain of device passes (what replaces count/count.cpp:279-364 on the device): newline count, route
 * (parse + containment filter + block merge + bucket), partition count, partition scatter, group classify, group
 * offsets, group place.  lsq_ingest_stage_count / _name list them; lsq_last_ingest_stages gives, for the latest
 * lsq_reads_upload* of the context, the device milliseconds of every pass (HIP events on the library's stream around the
 * pass's launches) and the bytes the pass has to move at least (its input read once, its output written once) -- the
 * two halves of a per-pass HBM roofline.  `capacity` entries of `ms` / `bytes` are written at most (either may be null). */
int lsq_ingest_stage_count(void);
const char *lsq_ingest_stage_name(int stage);
int lsq_last_ingest_stages(const lsq_ctx *c, float *ms, uint64_t *bytes, int capacity);
/* The name of pass `stage` as the latest lsq_reads_upload* of the context ran it: lsq_ingest_stage_name's, except that the
 * routing pass over SAM_SINGLE text is "sam_route" (other kernels than "route": lsq_sam_device.hpp). */
const char *lsq_last_ingest_stage_name(const lsq_ctx *c, int stage);
/* The passes of the latest lsq_reads_upload* of the context: lsq_ingest_stage_count(), except after a BAM_SINGLE file, whose
 * chain begins with three passes of its own in place of the newline count and the route -- "bgzf_inflate", "bam_record_starts",
 * "bam_route" (lsq_bam_device.hpp) -- and so has one more.  lsq_last_ingest_stages and lsq_last_ingest_stage_name index the
 * passes of that ingest, in order. */
int lsq_last_ingest_stage_count(const lsq_ctx *c);
/* Which of the SAM parse's kernels the latest SAM_SINGLE text of the context went through: lines the tile kernel handed to
 * the fall-back kernel (a head longer than the tile kernel's window), and whether the whole file went through the
 * byte-walking form (the line list ran over, or LSQ_SAM_SLOW is set).  Either pointer may be null. */
int lsq_last_sam_paths(const lsq_ctx *c, uint32_t *lines_listed, uint32_t *all_slow);
/* How the record starts of the latest BAM_SINGLE file of the context were found: its BGZF blocks, and how many of them the
 * repair pass walked again because a record did not begin with the block (0 for a file as htslib writes it).  Either may be null. */
int lsq_last_bam_paths(const lsq_ctx *c, uint64_t *n_blocks, uint64_t *blocks_repaired);
/* The whole-file check of a BAM file on the device chain, always verifying (lsq_bam_report and lsq_bam_check_host, above); the
 * context needs no events. */
int lsq_bam_check(lsq_ctx *c, const char *path, lsq_bam_report *r);
uint64_t lsq_reads_retained(const lsq_ctx *c, int method);      /* "loaded N reads" log line */
/* The library report of the latest read file of `method` in a stranded job: out[0] / out[1] the reads the file made with
 * transcript strand "+" / "-", out[2] the records that would have made a read but have no transcript strand, out[3] / out[4]
 * how many of the first two the load-time filter retained.  A library type chosen wrongly shows here: nearly every read of
 * one strand is then tested against the other strand's genes and dropped.  LSQ_E_STATE for unstranded events. */
int lsq_last_library_report(const lsq_ctx *c, int method, uint64_t out[5]);
uint64_t lsq_reads_retained_blocks(const lsq_ctx *c, int method);
/* Of the retained reads, those kept in the pools: reads whose first base lies in the span of an event planned on this
 * context.  Without a shard that is every retained read; with lsq_events_set_shard the slice's share (a read that starts
 * in no event of the slice is a candidate of none of them, count/count.cpp:429-432,463, and is dropped at ingest). */
uint64_t lsq_reads_pooled(const lsq_ctx *c, int method);
uint64_t lsq_reads_pooled_blocks(const lsq_ctx *c, int method);      /* ... and their blocks: what one lsq_count streams */
/* How the one- and two-block reads of a read file lie in HBM.  *compact = 1: 4 bytes a block -- 22 bits of offset (the
 * first block's from the first base of its bucket of events minus 2 Mi, the second block's from the end of the first) and
 * 10 bits of length; a read with a block of 1 024 bases or more, or an offset that does not fit, is kept with the
 * many-block reads, blocks in full.  *compact = 0 (more than 1 in 16 one- and two-block reads would not fit, or option
 * "compact_pools" 0): (start, end) per block, 8 bytes.  Either way every read takes part in lsq_count with its own
 * coordinates.  *pool_bytes: bytes of block coordinates resident in HBM; pool_reads[3]: reads kept as one-block records,
 * as two-block records, with the many-block reads.  Null: not wanted. */
int lsq_reads_pool_format(const lsq_ctx *c, int method, int *compact, uint64_t *pool_bytes, uint64_t *pool_reads);

/* Replaces the per-gene candidate scan + Read::build + compatibility + validity + counting
 * (count/count.cpp:420-482 == solve/solve.cpp:719-793; common/read.h:44-79,198-274): one
 * pass over every uploaded method's reads; fills per-(method, event, compatibility class)
 * read counts and matched-base sums on the device.  Asynchronous on the context stream. */
int lsq_count(lsq_ctx *c);
/* Per read file of the latest lsq_count (arrays of n_methods, either may be NULL; synchronises): the
 * (read, event) pairs the streaming kernel handed to the exception pass -- span-start ties that the
 * strand / name order decides (count/count.cpp:64-85), two blocks that touch -- and whether that list
 * overflowed, in which case two kernels behind the exception pass on the result stream zeroed the
 * method's tables and counted every read again (slow, complete).  The decision is taken on the
 * device, so every table that leaves the context -- also through lsq_results_copy_device in a loop
 * that never synchronises -- is whole. */
int lsq_count_status(lsq_ctx *c, uint32_t *exceptions, uint32_t *recounted);
/* How the latest lsq_count launched its streaming kernel: one-block reads a lane settles per look at the tables (4:
 * lsq_count_fast_kernel<.., 2>, 8: lsq_count_fast_kernel<true, 4>) and resident workgroups per compute unit.  Either
 * pointer may be null. */
int lsq_count_launch_info(lsq_ctx *c, uint32_t *reads_per_look, uint32_t *workgroups_per_cu);
/* What the latest lsq_count evaluated on the HOST: genes beyond the kernel limits above (more than LSQ_MAX_ISOFORMS isoforms
 * or LSQ_MAX_SEGMENTS segments, or a cluster of overlapping genes too large for the LDS) and the reads their clusters held.
 * Results are the reference's either way; throughput is not (host threads: LSQ_THREADS), so a caller may want to say so --
 * the executables do at log level 1.  Either pointer may be null. */
int lsq_host_evaluated(const lsq_ctx *c, uint64_t *n_genes, uint64_t *n_reads);
/* Tuning knobs; results never depend on them.  "grid_multiplier" (workgroups per resident slot of the
 * count kernel's grid, 0 = chosen from the read set's skew), "exception_capacity" (entries of a read
 * file's exception list, 0 = a quarter of its reads and at least 65 536; applies to read sets uploaded
 * afterwards), "recount_every_read" (1: every count is redone by the one-lane-per-read kernel, a
 * self-check), "em_guard_band" (lsq_set_em_guard_band), "snap_shares" (0: the count kernel's workgroup
 * shares are cut at even cost instead of at bucket ends), "share_weighted" (default 1: the shares are equal in estimated cost
 * -- "share_cost_two_block": a two-block record in one-block records, default 4.3; "share_cost_parked": one look of the general
 * walk at a read the streaming loops leave to it, default 9, counted per bucket by the ingest; "share_cost_visit": a bucket's
 * staging and flush, default 7 000; "share_cost_hot": extra cost of a record of a cell or junction group of 8 192 records or more,
 * default 0.5 (a deep gene's reads all add to the same few LDS counters) -- and fall off in size along the grid, "share_taper": the last share as a fraction of the
 * first, 0 = automatic, 0.5 for evenly deep read sets and 0.25 for skewed ones; 0: shares equal in reads), "compact_pools" (0: wide pool records for read sets
 * uploaded afterwards, see lsq_reads_pool_format), "em_regroup" (0: lsq_solve keeps the
 * placement of events in its grid chosen at lsq_events_upload; default 1: each of the two step lanes
 * re-sorts the placement by the iteration counts of one of its own earlier solves, refreshed every
 * sixteenth solve, so that events of similar cost share a wavefront), "count_streams" (1: every lsq_count on one
 * stream; default 2: a stream per step lane, so that a count may begin while the tail of the one before still runs),
 * "counter_sets" (default 3: consecutive counts take three sets of counters and exception lists in turn, so that a count waits for
 * the readers of the step three back and two counts are in flight at a time; 2: the rotation of two, where a count waits for the
 * result chain of the step before last, and the default of a context made with LSQ_CTX_LANES_IN_BACKGROUND, whose step streams share
 * hardware queues; LSQ_E_STATE unless every stream of the context has drained, lsq_ctx_synchronize),
 * "reads_per_look" (0 = automatic: eight one-block reads per lane and table look where the count kernel is held to five
 * workgroups a compute unit and the pools are compact, else four; 4; 8), "workgroups_per_cu" (resident workgroups of the count kernel per compute unit: 0 = as many as fit, default -1 = five
 * when the EM runs its one-lane-per-event kernel beside it and the read set is evenly deep, else as many as fit), "em_flat_min_events" (default 16 384: with at
 * least that many two-isoform events the ones that converged within 32 iterations last time are solved one lane per
 * event instead of four -- fewer instructions, longer passes), "sam_skip_flags" (default 0x904) and "sam_min_mapq" (default 0): which records of SAM_SINGLE
 * read files uploaded afterwards make no read -- these two do decide results; the executables also take them from LSQ_SAM_SKIP_FLAGS and LSQ_SAM_MIN_MAPQ), "bam_verify" (0 or 1, default 0; 1: BAM_SINGLE read files uploaded or parsed on the
 * device afterwards have every block's CRC32 and the end-of-file marker checked -- it decides which files are accepted, never a result; LSQ_BAM_VERIFY in the executables), "em_closed_form" (default 0; 1: two-isoform events with one read
 * file run six ordinary EM iterations and finish in the closed form of their EM map -- the step of read.h:592-618 is then a
 * Moebius map of theta_0, theta after m more iterations one exponential away, and the iteration at which read.h:659 stops
 * is found by search: the same iteration counts, theta within 1e-13; pays where the slowest events take hundreds of
 * iterations and little else runs beside the EM, e.g. a rank of an event-sharded job), "bootstrap_chunk" (default 0: lsq_bootstrap
 * resamples and solves as many replicates per launch as keep their count buffers below 256 MiB -- fewer where the device's free
 * memory asks for it; n in 1 .. 4096: n replicates per launch; a replicate's numbers never depend on it).  LSQ_E_ARG for an unknown name.  The executables
 * pass LSQ_OPTIONS="name=value,..." from the environment through this call. */
int lsq_ctx_set_option(lsq_ctx *c, const char *name, double value);

/* Replaces solve/solve.cpp:796-806,823-826 (common/read.h:592-660): batched EM over the
 * class counts, one event per lane, fp64.  Needs lsq_count first.  Asynchronous. */
int lsq_solve(lsq_ctx *c);

/* Result fetch (synchronises the stream).  Arrays are in output order; class c (1 <= c <
 * 2^K) of an event is the set of isoforms j with bit j set, and its slot is
 * class_off[ev] + c - 1 where class_off is the exclusive prefix sum of (2^K - 1).
 *   class_count[m * n_classes + slot], class_bases[...]: uint64
 *   theta[iso_off[ev] + j], logll[ev], em_iters[ev], em_flags[ev]
 * em_flags bit 0: the stop criterion |1 - old_ll/ll| came within the guard band (1e-11 unless
 * lsq_set_em_guard_band changed it) of the 1e-6 threshold at some iteration, so the kernel's sums over
 * compatibility classes could stop an iteration apart from the reference's sums over reads.  Such an event
 * is solved again in the reference's own order -- its valid reads in index order (count/count.cpp:64-85),
 * per-read sums as common/read.h:592-660 forms them, IEEE fp64, libm's log, on the host -- by
 * lsq_solve_finalize, which lsq_results_solve runs first; bit 2 (value 4) marks an event whose numbers
 * come from that replay.  bit 1: the iteration cap was reached. */
int64_t lsq_results_num_classes(const lsq_ctx *c);
int lsq_results_class_offsets(const lsq_ctx *c, uint64_t *class_off /* n_events+1 */);
int lsq_results_counts(lsq_ctx *c, uint64_t *class_count, uint64_t *class_bases);
/* The inverse: class counts and matched bases in that layout become the context's counts (e.g. the
 * sums over several processes that each counted a slice of the reads); lsq_solve then runs on them. */
int lsq_results_set_counts(lsq_ctx *c, const uint64_t *class_count, const uint64_t *class_bases);
/* The same exchange without the host: lsq_counts_export_device copies the latest count's class counts and matched bases
 * as they lie on the device -- lsq_counts_device_words() 8-byte words, the same order on every context that holds the
 * same events -- into a device buffer, on the result stream; lsq_counts_import_device takes such a buffer (the sum over
 * the ranks of a read-sharded job, count/count.cpp:378,467-482 add reads in any order) as the counts lsq_solve and the
 * getters work on.  The caller orders its collective against the result stream (lsq_ctx_result_stream). */
uint64_t lsq_counts_device_words(const lsq_ctx *c);
int lsq_counts_export_device(lsq_ctx *c, void *d_words);
int lsq_counts_import_device(lsq_ctx *c, const void *d_words);
int lsq_results_solve(lsq_ctx *c, double *theta, double *logll, uint32_t *em_iters, uint8_t *em_flags);
/* The exact-order replay on its own, for callers that take the results through lsq_results_copy_device:
 * waits for the latest lsq_solve, redoes every flagged event as described above and writes theta, logll,
 * iteration count and flag bit 2 back to the device arrays; *n_replayed (may be NULL) = events redone.
 * Events of counts that came from lsq_results_set_counts are left as they are (the reads behind such sums
 * are not all on this device).  common/read.h:592-660, solve/solve.cpp:720-748,767-806. */
int lsq_solve_finalize(lsq_ctx *c, uint32_t *n_replayed);
/* Width of the band around the 1e-6 stop threshold (common/read.h:659) inside which an event is flagged
 * and replayed; default 1e-11, i.e. ~100x the difference between the two summation orders.  A wider band
 * replays more events (1.0: every event with an EM loop), never changes which result is right. */
int lsq_set_em_guard_band(lsq_ctx *c, double band);

/* Optional: the expected Fisher information of theta_1..theta_{K-1} per read at the solved theta,
 * and the two variance estimates made from it -- common/fim.h:115-158,320-367 (bruteforce_fim / ofim:
 * the sum over every accessible read start of every isoform), :58-93 (estimate_mle_variance_by_diag,
 * _by_inv) with common/linalg.h:28-71's inverse.  PARITY UNPINNED: the reference never includes these
 * headers, no reference binary prints these numbers; the project's tests are the only pin: tests/fim_ref.py
 * states the headers' definition in exact rational arithmetic (one accessible read start at a time, exact
 * inverse, derived rounding bounds), tests/test_fim_reference_host.py holds it against the oracle's
 * double-precision restatement, tests/test_fim_direct_gpu.py the HIP path against it on events and class
 * counts chosen by hand, tests/test_parity_gpu.py the HIP path against the oracle on the golden inputs.
 * One matrix per event and read file, (K-1) x (K-1), row-major; events
 * in output order at lsq_results_fim_offsets (n_events + 1 values; K = 1: empty matrix, variances 0).
 * Call after lsq_solve.  fim: [method][lsq_results_fim_size], variances: [method][n_events]. */
int lsq_fim(lsq_ctx *c);
int64_t lsq_results_fim_size(const lsq_ctx *c);
int lsq_results_fim_offsets(const lsq_ctx *c, uint64_t *fim_off /* n_events+1 */);
int lsq_results_fim(lsq_ctx *c, double *fim, double *var_by_diag, double *var_by_inverse);

/* Optional (not in the reference): the read bootstrap of theta -- how far the library's depth lets one trust lsq_solve's number
 * (DESIGN 4.14).  A replicate resamples the counted reads of each (read file m, event e) with replacement, keeping that pair's
 * total: with cnt[m][e][c] the class counts (c = 1 .. 2^K - 1, the layout of lsq_results_counts) and n their sum, replicate b
 * draws i = 0 .. n - 1.  Random numbers: Philox4x32-10 (multipliers 0xD2511F53 and 0xCD9E8D57, key increments 0x9E3779B9 and
 * 0xBB67AE85, ten rounds, the key bumped before rounds 2 to 10) with key = (seed low word, seed high word) and counter =
 * (j low word, j high word, e, (m << 24) | b), j = i >> 1, e the event's index in the output order of the compiled events (not
 * of a shard), b < 2^24.  Of the block's words x0..x3 even i uses u = x0 | x1 << 32, odd i uses u = x2 | x3 << 32.  The draw is
 * r = (u * n) >> 64 (a 64 x 64 -> high 64 multiply), the class drawn the smallest c whose inclusive cumulative count exceeds r;
 * the replicate's counts are the histogram of the n draws, all zeros for n = 0.  All integer arithmetic: the result does not
 * depend on how the draws are split over lanes, tiles, chunks or devices.  Matched bases are not resampled.
 * Each replicate's counts are solved as lsq_solve solves counts given through lsq_results_set_counts with "em_regroup" 0 and
 * no closed form: four lanes an event for the lean places, the general kernel for the others, the context's guard band, the
 * same iteration cap; no host replay -- flag bit 0 may be set and the kernel's numbers stand.  Replicates carry theta only.
 * Summaries per isoform over the replicates whose theta is finite: n_ok, the mean, sd (two-pass, denominator n_ok - 1, no
 * number for n_ok < 2) and the quantiles 0.025, 0.5, 0.975 by linear interpolation on the sorted values v at h = (n_ok - 1) p:
 * v[floor h] + (h - floor h)(v[floor h + 1] - v[floor h]) (R type 7, numpy's default).  Events evaluated on the host (beyond
 * LSQ_MAX_ISOFORMS / LSQ_MAX_SEGMENTS / the LDS) are not resampled: n_ok 0 and no number -- a documented limit.
 * lsq_bootstrap: n_replicates in 1 .. 4096, else LSQ_E_ARG; needs lsq_count (or counts set from outside) and lsq_solve first,
 * else LSQ_E_STATE; runs on the result stream behind the latest solve, in chunks of replicates ("bootstrap_chunk") that never
 * change a result, and leaves the point estimate's arrays as they were.  The theta of every replicate stays on the device
 * until the next lsq_bootstrap, the next lsq_events_upload or lsq_ctx_destroy; if it and one chunk exceed the free device
 * memory: LSQ_E_RANGE, the text names the bytes.  Blocks until the replicates are done.
 * lsq_results_bootstrap: the six summaries, n_iso entries each in output order (theta's layout in lsq_results_solve).
 * lsq_results_bootstrap_theta: every replicate's theta, [n_replicates][n_iso].
 * lsq_bootstrap_replicate: replicate b alone through the same kernels (counts in the layout of lsq_results_counts, the rest as
 * lsq_results_solve; iters and flags may be NULL); the stored replicates are left alone.
 * lsq_bootstrap_tile: draws of one work item of the resampling kernel (tests place their cases around it). */
int lsq_bootstrap(lsq_ctx *c, uint32_t n_replicates, uint64_t seed);
int lsq_results_bootstrap(lsq_ctx *c, uint32_t *n_ok, double *mean, double *sd, double *q025, double *q500, double *q975);
int lsq_results_bootstrap_theta(lsq_ctx *c, double *theta /* [n_replicates][n_iso] */);
int lsq_bootstrap_replicate(lsq_ctx *c, uint64_t seed, uint32_t b, uint64_t *class_count, double *theta, double *logll, uint32_t *iters, uint8_t *flags);
int lsq_bootstrap_tile(void);
/* Host-only, no GPU: replicate b's counts of n_events events' class counts -- class_off (n_events + 1 values) and
 * class_count[m * class_off[n_events] + slot] as lsq_results_class_offsets and lsq_results_counts give them, event e being
 * the e-th of them -- into out, same layout, by the same code the device runs (csrc/lsq_philox.hpp).  One draw at a time on
 * one thread: meant for checks and small inputs. */
int lsq_bootstrap_resample_host(int n_methods, uint64_t n_events, const uint64_t *class_off, const uint64_t *class_count, uint64_t seed, uint32_t b,
                                uint64_t *out);

/* Copies the raw device-order results into caller-provided DEVICE buffers (e.g. tensors of a
 * framework that will run a collective on them), asynchronously on the context's RESULT stream (the
 * one the EM runs on, not lsq_ctx_stream's: lsq_ctx_synchronize waits for all of them), behind the count's
 * exception pass -- and its recount, should the exception list have overflowed -- and the EM, so the
 * tables are complete.  theta / logll are the kernel's numbers; an event inside the EM guard band
 * (rare; em_flags bit 0) gets the reference's exact-order numbers from lsq_solve_finalize.
 * d_class_count [n_methods * n_classes] uint64, d_theta [n_isoforms] f64, d_logll [n_events]
 * f64; any may be NULL.  lsq_results_device_order() gives, per device-order event, its output
 * index, so a gathered buffer can be put in output order on the receiving side. */
int lsq_results_copy_device(lsq_ctx *c, void *d_class_count, void *d_theta, void *d_logll);
/* The stream those hand-offs run on (hipStream_t in a void*): a caller that launches its own work on the
 * handed-over buffers -- a collective, say -- orders it behind an event recorded here.  It is the result stream of the
 * latest lsq_count's lane, so it changes with every lsq_count (see lsq_ctx_stream above): query it per step. */
void *lsq_ctx_result_stream(lsq_ctx *c);

/* ---- one job over several GPUs: events sharded by index, per-event records gathered -------------------
 * The reference's scale-out unit is a slice gene_begin_idx..gene_end_idx of the sorted gene list, one process
 * per slice, outputs concatenated (count/count.cpp:204-215).  Here: every process compiles the WHOLE selected
 * range (so the load-time read filter is the unsharded one), takes its slice with lsq_events_set_shard --
 * lsq_shard_bounds cuts the list into `world` contiguous slices of equal weight, e.g. reads per event from a
 * first unsharded count -- counts and solves it, packs its per-event records in output order
 * (lsq_results_pack_device: lsq_record_words(e, first, count) words of 8 bytes -- class counts
 * [method][class], matched bases [method][class], theta, log-likelihood -- asynchronously on the result
 * stream), the blocks are all-gathered (RCCL: ncclAllGather of blocks padded to the longest; liblesseq_rccl's
 * lsq_gather does that for a C host, torch.distributed for lesseq_amd/dist.py and bench.py) and
 * lsq_gathered_unpack lays them out as the whole job's tables for lsq_format_count / lsq_format_solve. */
int lsq_shard_bounds(const lsq_events *e, int world, const double *weights /* per event, or NULL */,
                     uint64_t *first /* world */, uint64_t *count /* world */);
uint64_t lsq_record_words(const lsq_events *e, uint64_t first, uint64_t count);
int lsq_results_pack_device(lsq_ctx *c, void *d_block);
/* Device buffers for a host without HIP of its own (zeroed; lsq_device_read waits for all streams of the context). */
int lsq_device_alloc(lsq_ctx *c, uint64_t bytes, void **out);
void lsq_device_free(lsq_ctx *c, void *p);
int lsq_device_read(lsq_ctx *c, void *host_dst, const void *device_src, uint64_t bytes);
int lsq_device_write(lsq_ctx *c, void *device_dst, const void *host_src, uint64_t bytes);      /* blocking, after the context's streams */
int lsq_gathered_unpack(const lsq_events *e, int world, const uint64_t *first, const uint64_t *count,
                        const uint64_t *blocks, uint64_t stride_words,
                        uint64_t *class_count, uint64_t *class_bases, double *theta, double *logll);
int lsq_results_device_order(const lsq_ctx *c, int32_t *dev2out /* n_events */);

/* Device timing, for bench.py and the developer tools.  Off by default: the event records between
 * the kernels of a step hold the queue up (measured: 0.343 -> 0.317 ms per count+solve step on the
 * 100 M-read workload without them).  lsq_set_timing(ctx, 1) makes the following lsq_count /
 * lsq_solve calls record HIP events on the context stream around their launches; the getters
 * return LSQ_E_STATE for a call that ran without. */
int lsq_set_timing(lsq_ctx *c, int on);
/* Duration of the last lsq_count / lsq_solve (ms), kernels only. */
int lsq_last_timing(lsq_ctx *c, float *count_ms, float *solve_ms);
/* Duration of the last lsq_count's lsq_count_fast_kernel launches alone (summed over read files),
 * from HIP events recorded immediately around each launch. */
int lsq_last_fast_kernel_ms(lsq_ctx *c, float *ms);

/* ------------------------------------------------------------------------------------
 * Output rows (host): replaces count/count.cpp:486-492 and solve/solve.cpp:808-847
 * ------------------------------------------------------------------------------------ */

/* Formats the count table from fetched class counts into a malloc'd NUL-terminated buffer
 * (free with lsq_free). */
int lsq_format_count(const lsq_events *e, int n_methods, const uint64_t *class_count, char **out_text);
int lsq_format_solve(const lsq_events *e, int n_methods, const uint64_t *class_count,
                     const uint64_t *class_bases, const double *theta, const double *logll,
                     const double *total_read_bases, char **out_text);
void lsq_free(void *p);

/* Whole executables in-process: argv as the reference's (argv[0] ignored).  tool is
 * "count", "solve", "classify", "test_as" (bin/Test_AS.r; lsq_as_* below), "events" (bin/Events.r; lsq_le_*), "parseGencode" or
 * "gencodeIsoformMap" (lsq_gtf_*; one optional argument names a file to read instead of standard input), "sam2mrf", "bam2mrf", "bamcheck", "junctions" (lsq_jn_*), "coverage" (lsq_cov_*), "exonbins" (lsq_xb_*), "psi" (lsq_ps_*), "evidence" (lsq_fe_*), "sites" (lsq_ss_*), "retention" (lsq_ir_*), "clusters" (lsq_cl_*) or "libtype" (lsq_lt_*).  stdout text is returned in *out_text (malloc'd), the
 * return value is the process exit status the reference would give (0, 1). */
int lsq_cli_run(const char *tool, int argc, const char *const *argv, char **out_text);
/* The same for an executable's main(): writes the table to stdout itself and returns the exit status.  A successful
 * count / solve run leaves the process (_exit) as soon as its table is written and flushed -- the pools, the helper
 * threads and the runtime are the operating system's to reclaim, which takes it a fraction of the time an orderly
 * teardown of several gigabytes of HBM takes (0.1-0.2 s of a 0.7 s run); LSQ_CLI_TEARDOWN=1 in the environment keeps
 * the orderly way.  A null tool means "choose by argv[0]": the first tool, in the precedence of the library's table of tools, whose
 * name is a substring of the program's base name, else count.  Not for use inside a host process: call lsq_cli_run there. */
int lsq_cli_main(const char *tool, int argc, const char *const *argv);

/* ------------------------------------------------------------------------------------
 * Differential splicing tests: step 4 of the pipeline, bin/Test_AS.r ("Differential splicing tests")
 * ------------------------------------------------------------------------------------ */

/* Device group (HIP, FP64).  Host arrays in and out; NaN stands for R's NA.  Each call allocates its device buffers on
 * the context's device, runs on the context's stream and frees them before it returns. */
/* Replaces Test_AS.r:34-47: fisher.test(two.sided) per 2x2 table, cells [n][4] = A B C D (R's matrix(c(A,B,C,D), 2)),
 * rounded half-to-even.  A table with an NA, negative, infinite or above-2^40 cell gets p = NA (R stops the script). */
int lsq_as_fisher(lsq_ctx *c, uint64_t n_tables, const double *cells /* [n][4]: A B C D */, double *p);
/* Replaces Test_AS.r:89-131: per row the Poisson glm log(mu) ~ tissue + rep + offset and ~ rep + offset (tissue, rep
 * numeric; y = round(count) + 1, offset = log(round(total) + 1)), lrtest's statistic and chi-square p.  NA in a cell
 * (the first: the script's own rule; any other, or a negative or infinite one: a divergence) gives stat = p = NA; a
 * non-finite log-likelihood stat = 0, p = 1.  count / total: [n][n1+n2], condition 1 first.  1 <= n1, n2 <= 4096. */
int lsq_as_lrt(lsq_ctx *c, uint64_t n_rows, int n1, int n2, const double *count, const double *total /* [n][n1+n2] each */,
               double *stat, double *p);
/* No counterpart in Test_AS.r: the replicate-aware test.  Per row y_j ~ BetaBinomial(n_j, mu_g, rho) with y = round(count),
 * n = round(total) (no +1), one mean per condition in the full model, one in the reduced, and one dispersion rho shared by the
 * samples of the row, both maximised over mu in [0, 1], rho in [0, 0.999] (DESIGN.md 4.6 has the likelihood); stat =
 * max(0, 2 (l_full - l_reduced)), p its chi-square tail (one degree of freedom), mu1 / mu2 / rho the full model's maximum
 * (rho = 0: the samples agree as well as binomial draws; where a maximum is attained on a set, one point of it).  A sample
 * with n = 0 is left out.  NA in all five outputs: a rounded cell that is NA, negative, infinite or above 2^40, y > n in a
 * sample, a condition without a sample of n > 0, fewer than 3 such samples in the row.  1 <= n1, n2 <= 4096, n1 + n2 >= 3. */
int lsq_as_betabin(lsq_ctx *c, uint64_t n_rows, int n1, int n2, const double *count, const double *total /* [n][n1+n2] each */,
                   double *mu1, double *mu2, double *rho, double *stat, double *p);
/* Replaces Test_AS.r:162-175: diff = mean(condition 1) - mean(condition 2), p = wilcox.test(x, y)'s (two-sided,
 * correct = TRUE; non-finite values dropped; an empty group gives NA, the script's try-error).  value: [n][n1+n2]. */
int lsq_as_wilcox(lsq_ctx *c, uint64_t n_rows, int n1, int n2, const double *value /* [n][n1+n2] */, double *diff, double *p);
/* Replaces Test_AS.r:45,129,173: p.adjust(p, "bonferroni") and p.adjust(p, "BH") over the non-NA values (NA stays NA;
 * with at most one non-NA value p comes back unchanged).  LSQ_E_ARG for a negative p-value. */
int lsq_as_adjust(lsq_ctx *c, uint64_t n, const double *p, double *p_bonferroni, double *p_bh);

/* Host-only: the inputs of one test ("fisher", "lrt", "wilcox", "betabin"), read and checked (no GPU touched).  "betabin"
 * reads what "lrt" reads, by the same rules, and wants n1+n2 >= 3 (LSQ_E_ARG otherwise).
 * lsq_as_read_matrix reads the script's own files -- a header line, then an ID and the same number of values per line;
 * a value is a number, NA / NaN / nan / -nan or Inf / -Inf / inf / -inf: "fisher" one file of 2 value columns, rows
 * taken in pairs (the ID is the second row's, an odd last row is ignored); "lrt" the count_one and count_all files of
 * n1+n2 columns with the same IDs in the same order; "wilcox" one file of n1+n2 columns.
 * lsq_as_read_tables reads this project's tables, one per sample: count tables for "fisher" (two) and "lrt", solve
 * tables for "wilcox" (n1+n2 each).  With M read files a count table has M+3 columns and a solve table M+5; the form ID
 * is column M+2, the event total the sum of columns 2..M+1, the value column M+3.  "fisher" takes the events (runs of
 * one gene name) with exactly two forms, cells as above with the second form's ID (lsq_as_input_left_out: the others).
 * Input errors (LSQ_E_IO, LSQ_E_PARSE, LSQ_E_ARG) name the file and line: a ragged row, a duplicate ID, a field that is
 * not a number, mismatched IDs, n1+n2 not the number of columns or tables, a negative count for "fisher" or "lrt". */
typedef struct lsq_as_input lsq_as_input;
int lsq_as_read_matrix(const char *test, int n_paths, const char *const *paths, int n1, int n2, lsq_as_input **out);
int lsq_as_read_tables(const char *test, int n_paths, const char *const *paths, int n1, int n2, lsq_as_input **out);
void lsq_as_input_free(lsq_as_input *in);
uint64_t lsq_as_input_rows(const lsq_as_input *in);
int lsq_as_input_columns(const lsq_as_input *in);                 /* 4 for "fisher", n1+n2 otherwise */
const char *lsq_as_input_id(const lsq_as_input *in, uint64_t row);
const double *lsq_as_input_values(const lsq_as_input *in);        /* [rows][columns]: cells, counts or values */
const double *lsq_as_input_totals(const lsq_as_input *in);        /* "lrt", "betabin": [rows][columns] totals; NULL otherwise */
uint64_t lsq_as_input_left_out(const lsq_as_input *in);
/* R's as.character(v): 15 significant digits, trailing zeros dropped, fixed unless scientific is strictly shorter
 * ("1e-04", "0.001", "1e+05", "123456"), NaN as "NA".  32 bytes always suffice. */
int lsq_as_format_number(double v, char *buf, size_t cap);

/* ------------------------------------------------------------------------------------
 * Splice junctions of a read file: the table step 1 of the pipeline ("refining gene models using RNA-Seq data") starts from
 * (DESIGN.md 4.12); what STAR writes as SJ.out.tab and `regtools junctions extract` prints
 * ------------------------------------------------------------------------------------ */

/* The definition, on the arrays the parsers above give (lsq_reads_parse / lsq_sam_parse / lsq_bam_parse, lsq_mrf_parse_device):
 *   chromosomes  the distinct chromosome strings of the annotation's isoform lines (every line it loaded, selected or not).  A
 *                block on another chromosome, or with a coordinate outside +-2^30, has no chromosome (the parsers' own rule).
 *   occurrence   two consecutive blocks k, k+1 of one read, unmerged, file order, 0-based half-open: both with the same chromosome
 *                (not none), start[k+1] > end[k], and min(end[k]-start[k], end[k+1]-start[k+1]) >= min_overhang.  The junction is
 *                (chromosome, end[k], start[k+1]).  Abutting, overlapping or descending blocks, and a pair across two chromosomes, make none.
 *   per junction reads: its occurrences; plus / minus: those whose block k carries the strand string "+" / "-"; max_overhang:
 *                the largest of the minima above.
 *   ann          per isoform line the union of its exons with end > start (the first exonCount of the line; order, overlap and
 *                empty exons do not matter); its introns are the gaps between consecutive maximal intervals of that union.  '.': no
 *                isoform on the chromosome has the junction as an intron; '+' / '-': every isoform that has it carries that strand
 *                string; '*' otherwise.
 *   rows         ascending in chromosome name (bytewise), start, end.  Text: chrom TAB start+1 TAB end TAB ann TAB reads TAB plus
 *                TAB minus TAB max_overhang NL -- the intron's first and last base, 1-based inclusive, as STAR prints it; no header.
 *   report       reads in the file, blocks in the file, occurrences counted, block pairs dropped by the overhang (same chromosome,
 *                a gap, a flank too short), block pairs in which a block has no chromosome.
 * Events are not involved and none of lsq_events_compile's limits applies.  More than 2^32-1 occurrences: LSQ_E_RANGE. */
typedef struct lsq_jn_index lsq_jn_index;       /* chromosome and strand dictionaries ("+" = 0, "-" = 1), the sorted distinct introns with their ann */
typedef struct lsq_jn_table lsq_jn_table;
int lsq_jn_index_build(const lsq_annotation *a, lsq_jn_index **out);      /* LSQ_E_RANGE beyond 65 535 chromosomes */
void lsq_jn_index_free(lsq_jn_index *ix);
int64_t lsq_jn_index_num_chroms(const lsq_jn_index *ix);
const char *lsq_jn_index_chrom_name(const lsq_jn_index *ix, int64_t chrom);      /* NULL when out of range */
int64_t lsq_jn_index_num_introns(const lsq_jn_index *ix);
/* The index's dictionaries as the lsq_events the host parsers intern against (owned by the index; it holds no event and cannot be
 * uploaded): lsq_reads_parse(..., lsq_jn_index_dictionaries(ix), ...) gives the arrays lsq_jn_host_reads takes. */
lsq_events *lsq_jn_index_dictionaries(lsq_jn_index *ix);
/* Host-only: the table from the host parsers' arrays.  read_format: whatever lsq_reads_parse takes (the name-keyed formats: the
 * lines of one name, in file order, are the blocks of one read; a line on a chromosome the annotation does not name is dropped by
 * that parser); skip_flags / min_mapq apply to SAM_SINGLE and BAM_SINGLE.  Statuses and messages are the parser's.  The index's
 * strand dictionary grows by the strings the file introduces.  lsq_jn_host_reads: the same from arrays parsed against the index
 * (tools: the host path without the parse). */
int lsq_jn_host(lsq_jn_index *ix, const char *read_format, const char *path, unsigned skip_flags, unsigned min_mapq,
                uint32_t min_overhang, int n_threads, lsq_jn_table **out);
int lsq_jn_host_reads(lsq_jn_index *ix, const lsq_reads *r, uint32_t min_overhang, int n_threads, lsq_jn_table **out);
/* Device (HIP, gfx950): "MRF_SINGLE", "SAM_SINGLE" or "BAM_SINGLE", parsed from the file's own bytes as lsq_mrf_parse_device parses
 * it (the context's "sam_skip_flags" / "sam_min_mapq" / "bam_verify"; the statuses and messages of lsq_reads_upload_mrf for a
 * malformed file), then extract, sort, reduce, annotate on device arrays; the distinct rows alone come back.  The context needs
 * no events, and its events, reads and counters are as they were afterwards. */
int lsq_jn_device(lsq_ctx *c, lsq_jn_index *ix, const char *read_format, const char *path, uint32_t min_overhang, lsq_jn_table **out);
void lsq_jn_table_free(lsq_jn_table *t);
int64_t lsq_jn_table_rows(const lsq_jn_table *t);
/* The rows' arrays (they live as long as the table; any pointer may be null): chrom indexes lsq_jn_index_chrom_name. */
int lsq_jn_table_arrays(const lsq_jn_table *t, const uint32_t **chrom, const int32_t **start, const int32_t **end, const uint8_t **ann,
                        const uint32_t **reads, const uint32_t **plus, const uint32_t **minus, const uint32_t **max_overhang);
int lsq_jn_table_report(const lsq_jn_table *t, uint64_t report[5]);
/* Device milliseconds per phase of the lsq_jn_device call that made the table -- extract, sort, reduce, annotate, copy-back --
 * from HIP events on the library's stream (zeros from the host path); the parse ahead of them: lsq_last_mrf_timing. */
int lsq_jn_table_times(const lsq_jn_table *t, float ms[5]);
/* The text of the rows with reads >= min_reads and, with novel_only, ann '.'; malloc'd, NUL-terminated (lsq_free). */
int lsq_jn_format(const lsq_jn_table *t, uint32_t min_reads, int novel_only, char **out_text);
int lsq_jn_sort_tile(void);      /* records a workgroup of the device sort takes (tests place their cases around it) */

/* ------------------------------------------------------------------------------------
 * Splice-site usage and read-through per junction of a read file: of the blocks that reach a splice site, how
 * many are spliced there, to which partner, and how many run straight through it -- the integers behind psi5 / psi3 and the
 * completeness-of-splicing index (Pervouchine et al. 2013, bam2ssj) and behind the boundary-spanning reads of IRFinder
 * ------------------------------------------------------------------------------------ */

/* The definition; inputs, coordinates, chromosomes, the occurrence rule and `ann` are the junction table's above.
 *   rows           the distinct junctions of the file -- lsq_jn_*'s rows under the same min_overhang, with the same ann -- united
 *                  with every intron of the annotation (lsq_jn_index_build's distinct introns): an annotated intron that no read
 *                  supports is a row with reads 0.  Ascending in chromosome name (bytewise), start, end.  min_overhang may be 0
 *                  here: the occurrence rule then asks nothing of the flanks.
 *   boundaries     (chromosome, p): the place between base p-1 and base p.  A row has the left boundary p = start and the right
 *                  boundary p = end; the distinct boundaries of all rows form one set a chromosome, and the start of one row and
 *                  the end of another may be one boundary and then share its count.
 *   through[p]     the blocks [s, e) on p's chromosome (with a chromosome, not empty) with s + m <= p <= e - m, m = max(min_overhang, 1):
 *                  m bases on either side.  Every block counts on its own, whatever read it belongs to and in whatever order: for
 *                  aligner output -- a read's blocks are disjoint -- that is reads, for a name-keyed format with overlapping lines
 *                  it is blocks.  Nothing overflows for m up to 2^32-1.
 *   spliced        left_spliced / right_spliced of a row: the sum of reads over all rows with the same (chromosome, start) /
 *                  (chromosome, end).
 *   text           chrom TAB start+1 TAB end TAB ann TAB reads TAB left_spliced TAB left_through TAB right_spliced TAB right_through
 *                  NL, the first three as lsq_jn_format prints them; no header.  With ratios four more columns: psi_left =
 *                  reads / left_spliced, psi_right = reads / right_spliced, cosi_left = left_spliced / (left_spliced + left_through),
 *                  cosi_right likewise -- on the host in double from the integers, %.6f, NA where the denominator is 0.  left and
 *                  right are genomic: which is donor and which acceptor follows from ann where it is '+' or '-'.
 *   report         eight: lsq_jn_table_report's five, then the distinct boundaries, the sum of all boundary counts, the rows with reads 0.
 * Limits: lsq_jn_*'s, and 2^32-2 boundaries.  Beyond a limit: LSQ_E_RANGE. */
typedef struct lsq_ss_index lsq_ss_index;       /* an lsq_jn_index: the dictionaries and the sorted distinct introns */
typedef struct lsq_ss_table lsq_ss_table;
int lsq_ss_index_build(const lsq_annotation *a, lsq_ss_index **out);
void lsq_ss_index_free(lsq_ss_index *ix);
int64_t lsq_ss_index_num_chroms(const lsq_ss_index *ix);
const char *lsq_ss_index_chrom_name(const lsq_ss_index *ix, int64_t chrom);      /* NULL when out of range */
int64_t lsq_ss_index_num_introns(const lsq_ss_index *ix);
lsq_events *lsq_ss_index_dictionaries(lsq_ss_index *ix);                  /* as lsq_jn_index_dictionaries */
/* Host-only, threaded: the table from the host parsers' arrays; read_format, skip_flags, min_mapq, statuses and messages as for
 * lsq_jn_host (the name-keyed formats included).  lsq_ss_host_reads: from arrays parsed against the index. */
int lsq_ss_host(lsq_ss_index *ix, const char *read_format, const char *path, unsigned skip_flags, unsigned min_mapq, uint32_t min_overhang, int n_threads,
                lsq_ss_table **out);
int lsq_ss_host_reads(lsq_ss_index *ix, const lsq_reads *r, uint32_t min_overhang, int n_threads, lsq_ss_table **out);
/* Device (HIP, gfx950): "MRF_SINGLE", "SAM_SINGLE" or "BAM_SINGLE", parsed exactly as lsq_jn_device parses it; the junction rows by
 * lsq_jn_device's passes, the rows and boundaries put together on the host and uploaded, one count kernel over the device arrays;
 * the boundaries' counters alone come back.  The context needs no events, and its events, reads and counters are as they were
 * afterwards.  LSQ_SS_GRID in the environment bounds the count's workgroups (tests). */
int lsq_ss_device(lsq_ctx *c, lsq_ss_index *ix, const char *read_format, const char *path, uint32_t min_overhang, lsq_ss_table **out);
void lsq_ss_table_free(lsq_ss_table *t);
int64_t lsq_ss_table_rows(const lsq_ss_table *t);
/* The rows' arrays (they live as long as the table; any pointer may be null): chrom indexes lsq_ss_index_chrom_name. */
int lsq_ss_table_arrays(const lsq_ss_table *t, const uint32_t **chrom, const int32_t **start, const int32_t **end, const uint8_t **ann, const uint64_t **reads,
                        const uint64_t **left_spliced, const uint64_t **left_through, const uint64_t **right_spliced, const uint64_t **right_through);
int lsq_ss_table_report(const lsq_ss_table *t, uint64_t report[8]);
/* Device milliseconds per phase of the lsq_ss_device call that made the table -- junctions (the sum of lsq_jn_table_times' five),
 * index (host work and upload), through, copy-back -- from HIP events on the library's stream (zeros from the host path). */
int lsq_ss_table_times(const lsq_ss_table *t, float ms[4]);
/* The text of the rows with reads >= min_reads and, with novel_only, ann '.'; malloc'd, NUL-terminated (lsq_free). */
int lsq_ss_format(const lsq_ss_table *t, uint32_t min_reads, int novel_only, int ratios, char **out_text);
int lsq_ss_lds_slots(void);      /* boundary ids a workgroup of the device count keeps in LDS (tests place their cases around it) */

/* ------------------------------------------------------------------------------------
 * Intron retention of a read file: per intron of the annotation its splice-site counts and the depth over the
 * bases of its body that belong to no exon, summarised by order statistics that a local pile-up cannot move -- the integers behind
 * IRFinder's IR ratio (Middleton et al. 2017)
 * ------------------------------------------------------------------------------------ */

/* The definition; inputs, coordinates, chromosomes and columns 1-9 are the sites table's above, the depth is the coverage table's below.
 *   rows           one per distinct intron of the annotation: the rows of lsq_ss_*'s table under the same min_overhang whose ann is
 *                  not '.', in that table's order.  A novel junction makes no row; it counts in the spliced sums of the sites it shares.
 *   body           an intron (a, b) -- the end of the left exon interval, the start of the right one -- has the body [a, b).
 *   clean bases    the bases of [a, b) in no exon of any isoform line on that chromosome, on either strand (exons with end > start,
 *                  the first exonCount of a line, coordinates clamped to +-2^30).  They form maximal intervals, the intron's pieces;
 *                  an intron wholly covered by other lines' exons has none.
 *   depth          d(x) of lsq_cov_* with strand 0: every counted block on its own, 0 where no row lies.
 *   clean          n, the number of clean bases; covered: those with d >= 1; depth_sum: the sum of d over them (64 bits).
 *   q25 q50 q75    the n clean bases' depths sorted ascending, zeros included, d(1) <= ... <= d(n): column q (1, 2, 3) is d(k) with
 *                  k = (q n + 3) div 4 = ceil(q n / 4); all three 0 when n is 0.  No interpolation: exact integers.
 *   text           the sites row's nine columns, then TAB clean TAB covered TAB depth_sum TAB q25 TAB q50 TAB q75 NL; no header.  With
 *                  ratios three more columns: mean = depth_sum / clean, coverage = covered / clean, ir_ratio = q50 / (q50 +
 *                  max(left_spliced, right_spliced)) -- on the host in double from the integers, %.6f, NA where the denominator is
 *                  0; with clean 0 all three are NA.
 *   report         thirteen: lsq_ss_table_report's eight, then the rows (introns), the rows with clean 0, the pieces, the depth rows
 *                  of the file, and lsq_cov_table_report's bases.
 * Limits: lsq_ss_*'s and lsq_cov_*'s, and 2^32-2 pieces.  Beyond a limit: LSQ_E_RANGE. */
typedef struct lsq_ir_index lsq_ir_index;       /* an lsq_ss_index and every chromosome's exon union */
typedef struct lsq_ir_table lsq_ir_table;
int lsq_ir_index_build(const lsq_annotation *a, lsq_ir_index **out);
void lsq_ir_index_free(lsq_ir_index *ix);
int64_t lsq_ir_index_num_chroms(const lsq_ir_index *ix);
const char *lsq_ir_index_chrom_name(const lsq_ir_index *ix, int64_t chrom);      /* NULL when out of range */
int64_t lsq_ir_index_num_introns(const lsq_ir_index *ix);
lsq_events *lsq_ir_index_dictionaries(lsq_ir_index *ix);                  /* as lsq_jn_index_dictionaries */
/* Host-only, threaded: the table from the host parsers' arrays; read_format, skip_flags, min_mapq, statuses and messages as for
 * lsq_jn_host (the name-keyed formats included).  min_overhang is lsq_ss_host's, 0 included; the depth does not depend on it.
 * lsq_ir_host_reads: from arrays parsed against the index. */
int lsq_ir_host(lsq_ir_index *ix, const char *read_format, const char *path, unsigned skip_flags, unsigned min_mapq, uint32_t min_overhang, int n_threads,
                lsq_ir_table **out);
int lsq_ir_host_reads(lsq_ir_index *ix, const lsq_reads *r, uint32_t min_overhang, int n_threads, lsq_ir_table **out);
/* Device (HIP, gfx950): "MRF_SINGLE", "SAM_SINGLE" or "BAM_SINGLE", parsed once exactly as lsq_jn_device parses it; on those arrays
 * lsq_ss_device's passes, then lsq_cov_device's extract, sort, reduce and scan, emit -- the depth rows stay on the device -- the
 * pieces put together on the host and uploaded, and the selection: a wave an intron, the order statistics by bisection on the
 * depth.  One entry an intron of five arrays comes back.  The context needs no events, and its events, reads and counters are as
 * they were afterwards.  LSQ_IR_GRID in the environment bounds the selection's workgroups (tests). */
int lsq_ir_device(lsq_ctx *c, lsq_ir_index *ix, const char *read_format, const char *path, uint32_t min_overhang, lsq_ir_table **out);
void lsq_ir_table_free(lsq_ir_table *t);
int64_t lsq_ir_table_rows(const lsq_ir_table *t);
/* The rows' arrays (they live as long as the table; any pointer may be null): chrom indexes lsq_ir_index_chrom_name. */
int lsq_ir_table_arrays(const lsq_ir_table *t, const uint32_t **chrom, const int32_t **start, const int32_t **end, const uint8_t **ann, const uint64_t **reads,
                        const uint64_t **left_spliced, const uint64_t **left_through, const uint64_t **right_spliced, const uint64_t **right_through,
                        const uint64_t **clean, const uint64_t **covered, const uint64_t **depth_sum, const uint32_t **q25, const uint32_t **q50, const uint32_t **q75);
int lsq_ir_table_report(const lsq_ir_table *t, uint64_t report[13]);
/* Device milliseconds per phase of the lsq_ir_device call that made the table -- sites (the sum of lsq_ss_table_times' four), depth
 * (the sum of lsq_cov_table_times' extract, sort, reduce and scan, emit), index (host work and upload), select, copy-back -- from
 * HIP events on the library's stream (zeros from the host path). */
int lsq_ir_table_times(const lsq_ir_table *t, float ms[5]);
/* The text of all rows; malloc'd, NUL-terminated (lsq_free). */
int lsq_ir_format(const lsq_ir_table *t, int ratios, char **out_text);

/* ------------------------------------------------------------------------------------
 * Intron clusters of several read files: the junctions of all samples pooled, introns that share a splice site
 * joined into clusters, a count table per sample with the same rows in every one -- LeafCutter's clustering, applied once; the
 * rows `test_as lrt --tables` and `test_as betabin --tables` read
 * ------------------------------------------------------------------------------------ */

/* The definition.  A sample is the rows of one junction table (lsq_jn_*: chromosome index, start, end, reads; 0-based half-open),
 * all samples under one index.
 *   pooled introns the distinct (chromosome, start, end) over all samples.  r_k(j): the reads of intron j in sample k (rows of one
 *                  sample with one intron add up; 0 without a row), reads(j) their sum over k in 64 bits, samples(j) the number of
 *                  k with r_k(j) > 0, ann from the index as lsq_jn_* gives it.
 *   row filters    long: max_intron != 0 and end - start > max_intron.  weak: reads(j) < min_reads.  A row that is both is long.
 *                  The others are kept.
 *   links          two kept rows on one chromosome with the same start, or with the same end.  A start equal to another row's
 *                  end, and equal coordinates on two chromosomes, are no link; strand plays no part.
 *   clusters       the connected components of the kept rows.  One row: a singleton.  Two or more whose reads sum below
 *                  min_cluster_reads: weak.  The others are printed, numbered 1, 2, ... by the table order of their first row.
 *   status         per distinct intron: 0 printed, 1 weak row, 2 long row, 3 singleton, 4 weak cluster; cluster: its number, 0
 *                  unless status is 0.
 *   rows           every distinct intron, ascending in chromosome name (bytewise), start, end.  counts: [rows][samples], r_k(j).
 *   text           the printed rows by (cluster number, table order).  lsq_cl_format: clu_<n> TAB chrom TAB start+1 TAB end TAB ann
 *                  TAB reads TAB samples NL.  lsq_cl_format_sample (sample: 0-based, the order the samples were added in): clu_<n>
 *                  TAB total TAB chrom:start+1:end TAB r_k(j) NL, total the sum of r_k over the cluster's rows -- the four columns of
 *                  a count table of one read file; the same rows for every sample, zeros included.  No header.
 *   report         eleven: samples, pooled input rows, distinct introns, long rows, weak rows, kept rows, components, singletons,
 *                  weak clusters, printed clusters, printed rows.
 * Limits: 65 535 samples, 2^32-1 pooled rows, 2^32-1 for the sum of one sample's reads, rows x samples at most 2^31.  Beyond a
 * limit: LSQ_E_RANGE. */
typedef struct lsq_cl_pool lsq_cl_pool;         /* the samples' rows, and the chromosomes and introns of the index it was made from (copied) */
typedef struct lsq_cl_table lsq_cl_table;
int lsq_cl_pool_create(const lsq_jn_index *ix, lsq_cl_pool **out);
void lsq_cl_pool_free(lsq_cl_pool *p);
int64_t lsq_cl_pool_samples(const lsq_cl_pool *p);
int64_t lsq_cl_pool_rows(const lsq_cl_pool *p);      /* pooled input rows */
/* One more sample; a call that fails adds nothing.  lsq_cl_pool_add_table: the rows of a junction table of the same index
 * (LSQ_E_ARG for another dictionary of chromosomes).  lsq_cl_pool_add_rows: from arrays -- LSQ_E_ARG for a chromosome that is no
 * index of the dictionary or a row with start >= end, LSQ_E_RANGE for a coordinate outside (-2^30, 2^30); n may be 0.
 * lsq_cl_pool_add_text: a file as lsq_jn_format printed it (any min_reads, novel or not); the chromosome is looked up by name and
 * ann is not taken from the file -- LSQ_E_IO for a file that does not open, LSQ_E_PARSE with "<path>: #<line>:<text>" for a name
 * the index lacks or a line that is not eight columns of the right kinds. */
int lsq_cl_pool_add_table(lsq_cl_pool *p, const lsq_jn_table *t);
int lsq_cl_pool_add_rows(lsq_cl_pool *p, uint64_t n, const uint32_t *chrom, const int32_t *start, const int32_t *end, const uint32_t *reads);
int lsq_cl_pool_add_text(lsq_cl_pool *p, const char *path);
/* Host-only, the sort threaded: a sort of the pooled rows, then a union-find over the kept rows.  The pool may be solved again,
 * under other thresholds or with more samples.  max_intron < 2^31. */
int lsq_cl_host(const lsq_cl_pool *p, uint64_t min_reads, uint32_t max_intron, uint64_t min_cluster_reads, int n_threads, lsq_cl_table **out);
/* Device (HIP, gfx950): the pooled rows uploaded as two-word records and sorted (the library's radix sort), equal keys reduced to
 * the distinct introns and the count matrix, the row filters and the compaction of the kept rows, the links to a kept row's
 * predecessor by start and by end, connected components by hooking onto the smaller label with pointer jumping -- a round is two
 * launches, the host reads one word a round, no workgroup waits for another --, and per component its size, its reads and its
 * sums per sample.  Statuses, numbering and texts are made on the host as for lsq_cl_host; both give the same table.  The
 * context needs no events, and its events, reads and counters are as they were afterwards. */
int lsq_cl_device(lsq_ctx *c, const lsq_cl_pool *p, uint64_t min_reads, uint32_t max_intron, uint64_t min_cluster_reads, lsq_cl_table **out);
void lsq_cl_table_free(lsq_cl_table *t);
int64_t lsq_cl_table_rows(const lsq_cl_table *t);             /* distinct introns */
int64_t lsq_cl_table_samples(const lsq_cl_table *t);
const char *lsq_cl_table_chrom_name(const lsq_cl_table *t, int64_t chrom);      /* NULL when out of range */
/* The rounds of the components loop of the lsq_cl_device call that made the table, the last one -- which changes nothing --
 * included; it grows with the logarithm of the longest chain of links.  0 from the host path, and where no row is kept. */
int64_t lsq_cl_table_rounds(const lsq_cl_table *t);
/* The rows' arrays (they live as long as the table; any pointer may be null): chrom indexes lsq_cl_table_chrom_name. */
int lsq_cl_table_arrays(const lsq_cl_table *t, const uint32_t **chrom, const int32_t **start, const int32_t **end, const uint8_t **ann, const uint64_t **reads,
                        const uint32_t **samples, const uint32_t **cluster, const uint8_t **status);
int lsq_cl_table_counts(const lsq_cl_table *t, const uint32_t **counts);      /* [rows][samples] */
int lsq_cl_table_report(const lsq_cl_table *t, uint64_t report[11]);
/* Device milliseconds per phase of the lsq_cl_device call that made the table -- upload, sort, reduce, filter, links, components,
 * totals, copy-back -- from HIP events on the library's stream (zeros from the host path). */
int lsq_cl_table_times(const lsq_cl_table *t, float ms[8]);
/* The two texts; malloc'd, NUL-terminated (lsq_free).  LSQ_E_ARG for a sample out of range. */
int lsq_cl_format(const lsq_cl_table *t, char **out_text);
int lsq_cl_format_sample(const lsq_cl_table *t, int64_t sample, char **out_text);

/* ------------------------------------------------------------------------------------
 * Per-base read depth of a read file: what `bedtools genomecov -bg -split` prints, and the depth of every
 * isoform line of the annotation passed (an events .interval file: of every event form)
 * ------------------------------------------------------------------------------------ */

/* The definition, on the arrays the parsers above give (per read blk_off; per block start, end, chromosome, strand):
 *   chromosomes    as for lsq_jn_index: the distinct chromosome strings of the annotation's isoform lines.  A block on another
 *                  chromosome, or with a coordinate outside +-2^30, has no chromosome (the parsers' own rule).
 *   counted block  a block with a chromosome and end > start; with strand '+' or '-' its strand string must be that one too (the
 *                  alignment strand, as the parsers deliver it).  Every block is classified by the first rule it fails, in this order.
 *   depth          at base x of a chromosome: the number of counted blocks, 0-based half-open, that contain x.  Every block counts on
 *                  its own: two overlapping blocks of one read count twice, mates are two reads.  A uint32.
 *   rows           the maximal intervals [start, end) of constant depth > 0: two adjacent intervals of equal depth are one row (a
 *                  position where as many blocks end as begin is no boundary).  Ascending in chromosome name (bytewise), start.
 *                  Text (bedGraph): chrom TAB start TAB end TAB depth NL, 0-based half-open; no header.
 *   regions        one per isoform line of the annotation, every line loaded, in file order: the union of the line's exons with
 *                  end > start (the first exonCount of the line).  bases: the size of the union; covered: its bases with depth >=
 *                  min_depth; depth_sum: the sum of depth over its bases (64 bits).  Text: name TAB chrom TAB strand TAB bases TAB
 *                  covered TAB depth_sum TAB mean NL, mean = depth_sum / bases as %.4f, 0.0000 when bases is 0.
 *   report         reads in the file, blocks in the file, counted blocks, blocks without a chromosome, empty or descending blocks,
 *                  blocks of the other strand, bases: the summed length of the counted blocks = the sum of (end - start) * depth
 *                  over the rows.  With an annotation that names every chromosome of the file, bases is solve's total_read_bases.
 * More than 2^32-1 sort records (two per counted block): LSQ_E_RANGE. */
typedef struct lsq_cov_index lsq_cov_index;     /* chromosome and strand dictionaries ("+" = 0, "-" = 1), every line's exon union */
typedef struct lsq_cov_table lsq_cov_table;
int lsq_cov_index_build(const lsq_annotation *a, lsq_cov_index **out);    /* LSQ_E_RANGE beyond 65 535 chromosomes */
void lsq_cov_index_free(lsq_cov_index *ix);
int64_t lsq_cov_index_num_chroms(const lsq_cov_index *ix);
const char *lsq_cov_index_chrom_name(const lsq_cov_index *ix, int64_t chrom);    /* NULL when out of range */
int64_t lsq_cov_index_num_regions(const lsq_cov_index *ix);
lsq_events *lsq_cov_index_dictionaries(lsq_cov_index *ix);                /* as lsq_jn_index_dictionaries */
/* Host-only, threaded: the tables from the host parsers' arrays; read_format, skip_flags, min_mapq, statuses and messages as for
 * lsq_jn_host (the name-keyed formats included).  strand: 0 (every block), '+' or '-'.  lsq_cov_host_reads: from arrays parsed
 * against the index. */
int lsq_cov_host(lsq_cov_index *ix, const char *read_format, const char *path, unsigned skip_flags, unsigned min_mapq,
                 int strand, uint32_t min_depth, int n_threads, lsq_cov_table **out);
int lsq_cov_host_reads(lsq_cov_index *ix, const lsq_reads *r, int strand, uint32_t min_depth, int n_threads, lsq_cov_table **out);
/* Device (HIP, gfx950): "MRF_SINGLE", "SAM_SINGLE" or "BAM_SINGLE", parsed exactly as lsq_jn_device parses it, then extract, sort,
 * reduce and scan, emit, regions on device arrays; the rows and the regions' sums alone come back.  The context needs no events,
 * and its events, reads and counters are as they were afterwards.  LSQ_COV_EXTRACT_GRID in the environment bounds the extract's
 * workgroups (tests). */
int lsq_cov_device(lsq_ctx *c, lsq_cov_index *ix, const char *read_format, const char *path, int strand, uint32_t min_depth, lsq_cov_table **out);
void lsq_cov_table_free(lsq_cov_table *t);
int64_t lsq_cov_table_rows(const lsq_cov_table *t);
int64_t lsq_cov_table_regions(const lsq_cov_table *t);
/* The arrays (they live as long as the table; any pointer may be null): chrom indexes lsq_cov_index_chrom_name. */
int lsq_cov_table_arrays(const lsq_cov_table *t, const uint32_t **chrom, const int32_t **start, const int32_t **end, const uint32_t **depth);
int lsq_cov_table_region_arrays(const lsq_cov_table *t, const uint32_t **chrom, const uint64_t **bases, const uint64_t **covered, const uint64_t **depth_sum);
const char *lsq_cov_table_region_name(const lsq_cov_table *t, int64_t region);      /* NULL when out of range */
const char *lsq_cov_table_region_strand(const lsq_cov_table *t, int64_t region);
int lsq_cov_table_report(const lsq_cov_table *t, uint64_t report[7]);
/* Device milliseconds per phase of the lsq_cov_device call that made the table -- extract, sort, reduce and scan, emit, regions,
 * copy-back -- from HIP events on the library's stream (zeros from the host path); the parse ahead of them: lsq_last_mrf_timing. */
int lsq_cov_table_times(const lsq_cov_table *t, float ms[6]);
/* The bedGraph text of the rows with depth >= min_depth; the regions' text; malloc'd, NUL-terminated (lsq_free). */
int lsq_cov_format(const lsq_cov_table *t, uint32_t min_depth, char **out_text);
int lsq_cov_format_regions(const lsq_cov_table *t, char **out_text);
int lsq_cov_sort_tile(void);     /* records a workgroup of the device sort takes (tests place their cases around it) */

/* ------------------------------------------------------------------------------------
 * Reads per exon bin and per gene of a read file: the table dexseq_count / featureCounts -f -O print, in the
 * four columns `test_as lrt --tables` reads
 * ------------------------------------------------------------------------------------ */

/* The definition, on the arrays the parsers above give (blocks 0-based half-open, in file order, unmerged):
 *   chromosomes    as for lsq_jn_index: the distinct chromosome strings of the annotation's isoform lines.  A block on another
 *                  chromosome, or with a coordinate outside +-2^30, has no chromosome (the parsers' own rule).
 *   genes          the groups of the gene->isoform file, every gene the annotation holds, in the loader's order (the order in which
 *                  count prints them).  A gene whose isoform lines name more than one chromosome: LSQ_E_UNSUPPORTED, the message names
 *                  the first such gene.  A gene's strand is its lines' strand string when they all agree, else ".".
 *   bins           of a gene: every exon with end > start of every isoform line of the gene (the first exonCount of a line); the
 *                  distinct exon starts and ends sorted; a stretch between two neighbouring boundaries is a bin when at least one of
 *                  those exons covers it.  Numbered 1, 2, ... ascending; the id is <gene>:<k>, k unpadded.  The bins of one gene are
 *                  disjoint, bins of different genes may overlap.
 *   hit            a read hits a bin when some block of it with end > start lies on the bin's chromosome and has block_start <
 *                  bin_end && block_end > bin_start; it hits a gene when it hits at least one of its bins.
 *   counts         reads[bin]: the reads that hit the bin; total[gene]: the reads that hit the gene.  A read counts once per bin and
 *                  once per gene, however many of its blocks hit and in whatever order they come; a read that hits several genes
 *                  counts in each.  Strand plays no part.  Both are uint64.
 *   report         reads in the file, blocks in the file, blocks without a chromosome or empty, reads that hit no gene, reads that hit
 *                  more than one gene, the sum of all reads[bin].
 *   table          a row per bin, genes in gene order, a gene's bins ascending, zeros included:
 *                  gene TAB total[gene] TAB gene:k TAB reads[bin] NL -- a count table of `test_as lrt --tables`.
 *   bins texts     the bins as an annotation: an LH_GENE_TXT line per bin -- gene:k chrom strand start end 1 start end, TABs between --
 *                  and a gene->isoform line per bin, gene TAB gene:k.
 * Limits: 2^32-1 bins, 2^32-1 entries of the lookup below (the sum over the bins of the cells a bin spans), 65 535 chromosomes; any
 * number of exons and isoforms per gene (no event is compiled).  Beyond a limit: LSQ_E_RANGE. */
typedef struct lsq_xb_index lsq_xb_index;       /* the dictionaries, the bins gene-major, per chromosome the cells between bin boundaries with their bins */
typedef struct lsq_xb_table lsq_xb_table;
int lsq_xb_index_build(const lsq_annotation *a, lsq_xb_index **out);
/* Stranded counting: the library type (LSQ_LIBRARY_*) belongs to the index; LSQ_LIBRARY_UNSTRANDED is exactly
 * lsq_xb_index_build.  A read has the transcript strand t = s XOR (library == reverse) XOR mate2 of its first block (lsq_events_compile_library's
 * rule; a read whose first block's strand string is neither "+" nor "-" has none, counts for nothing and is tallied), and the table is,
 * row by row, the unstranded table of the plus genes alone on the reads with t = + and that of the minus genes alone on the reads
 * with t = -, in the rows' usual order.  The bins and the bins texts do not change.  Every gene needs a strand of its own ("+" or
 * "-" on all of its isoform lines): LSQ_E_UNSUPPORTED otherwise, the message names the first such gene and says how many there are.
 * The report keeps its six entries: reads, blocks and blocks without a chromosome or empty are those of the unstranded run on the
 * whole annotation; no gene / several genes / bin hits count hits of the read's own strand, and a read without t is in none of them.
 * lsq_xb_table_library_report: reads with t = +, with t = -, without t, and of the first two those that hit a gene (+, then -);
 * all zeros and LSQ_E_STATE for the table of an unstranded index. */
int lsq_xb_index_build_library(const lsq_annotation *a, int library, lsq_xb_index **out);
int lsq_xb_index_library(const lsq_xb_index *ix);
int lsq_xb_table_library_report(const lsq_xb_table *t, uint64_t report[5]);
void lsq_xb_index_free(lsq_xb_index *ix);
int64_t lsq_xb_index_num_chroms(const lsq_xb_index *ix);
int64_t lsq_xb_index_num_genes(const lsq_xb_index *ix);
int64_t lsq_xb_index_num_bins(const lsq_xb_index *ix);
const char *lsq_xb_index_chrom_name(const lsq_xb_index *ix, int64_t chrom);      /* NULL when out of range */
const char *lsq_xb_index_gene_name(const lsq_xb_index *ix, int64_t gene);
const char *lsq_xb_index_gene_strand(const lsq_xb_index *ix, int64_t gene);
lsq_events *lsq_xb_index_dictionaries(lsq_xb_index *ix);                  /* as lsq_jn_index_dictionaries */
/* The bins (the arrays live as long as the index; any pointer may be null): per bin start, end and gene; per gene its first bin
 * (num_genes + 1 entries) and its chromosome (0xFFFFFFFF: a gene without an isoform line). */
int lsq_xb_index_arrays(const lsq_xb_index *ix, const int64_t **bin_start, const int64_t **bin_end, const uint32_t **bin_gene,
                        const uint32_t **gene_first_bin, const uint32_t **gene_chrom);
/* Host-only, threaded: the table from the host parsers' arrays; read_format, skip_flags, min_mapq, statuses and messages as for
 * lsq_jn_host (the name-keyed formats included).  lsq_xb_host_reads: from arrays parsed against the index. */
int lsq_xb_host(lsq_xb_index *ix, const char *read_format, const char *path, unsigned skip_flags, unsigned min_mapq, int n_threads, lsq_xb_table **out);
int lsq_xb_host_reads(lsq_xb_index *ix, const lsq_reads *r, int n_threads, lsq_xb_table **out);
/* Device (HIP, gfx950): "MRF_SINGLE", "SAM_SINGLE" or "BAM_SINGLE", parsed exactly as lsq_jn_device parses it, then one count kernel
 * over the device arrays; the counters alone come back.  The context needs no events, and its events, reads and counters are as
 * they were afterwards.  LSQ_XB_GRID in the environment bounds the count's workgroups (tests). */
int lsq_xb_device(lsq_ctx *c, lsq_xb_index *ix, const char *read_format, const char *path, lsq_xb_table **out);
void lsq_xb_table_free(lsq_xb_table *t);
/* reads[num_bins], total[num_genes] (they live as long as the table; either pointer may be null) */
int lsq_xb_table_arrays(const lsq_xb_table *t, const uint64_t **reads, const uint64_t **total);
int lsq_xb_table_report(const lsq_xb_table *t, uint64_t report[6]);
/* Device milliseconds per phase of the lsq_xb_device call that made the table -- index upload, count, copy-back -- from HIP events
 * on the library's stream (zeros from the host path); the parse ahead of them: lsq_last_mrf_timing. */
int lsq_xb_table_times(const lsq_xb_table *t, float ms[3]);
/* The table's text; the two bins texts of an index; malloc'd, NUL-terminated (lsq_free). */
int lsq_xb_format(const lsq_xb_table *t, char **out_text);
int lsq_xb_format_bins(const lsq_xb_index *ix, char **interval_text, char **map_text);

/* ------------------------------------------------------------------------------------
 * Which library type is this read file?: what an infer_experiment-style check reports, for --library above
 * ------------------------------------------------------------------------------------ */

/* The definition:
 *   index     per chromosome of the annotation and strand, the union of all exons of that strand's genes there (the first
 *             exonCount exons of every isoform line, end > start), as sorted disjoint intervals clamped to +-2^30.  A gene has a
 *             strand when all its isoform lines carry the same one of "+" / "-"; genes without one are left out and counted.
 *   reads     parsed as under a stranded index: every read with a first-mate strand r = s XOR mate2 (lsq_xb_index_build_library's
 *             s and mate2) of its first block.  P: some block of the read with end > start on a chromosome of the annotation shares
 *             at least one base with the plus union of that chromosome; M: the same for the minus union.
 *   counts    [0] reads; [1] reads without r; [2..5] r = +: neither, P only, M only, both; [6..9] r = -: the same; [10] genes left out.
 *   derived   sense = (+, P only) + (-, M only); antisense = (+, M only) + (-, P only); ambiguous: both; no_gene: neither;
 *             forward_fraction = sense / (sense + antisense) in double (has_fraction 0 when the denominator is 0).
 *   library   sense + antisense < 100: "undetermined"; fraction >= 0.9: "forward"; <= 0.1: "reverse"; 0.4 <= fraction <= 0.6:
 *             "unstranded"; anything else "undetermined" (a static string).
 *   text      key TAB value lines: reads, no_strand, plus_none, plus_plus, plus_minus, plus_both, minus_none, minus_plus,
 *             minus_minus, minus_both, sense, antisense, ambiguous, no_gene, unplaced_genes, forward_fraction (%.6f or NA), library.
 * Host, device, formats, options, statuses and messages as for lsq_xb_host / lsq_xb_host_reads / lsq_xb_device; LSQ_LT_GRID in the
 * environment bounds the count's workgroups (tests).  Times: index upload, count, copy-back. */
typedef struct lsq_lt_index lsq_lt_index;
typedef struct lsq_lt_table lsq_lt_table;
int lsq_lt_index_build(const lsq_annotation *a, lsq_lt_index **out);
void lsq_lt_index_free(lsq_lt_index *ix);
int64_t lsq_lt_index_num_chroms(const lsq_lt_index *ix);
const char *lsq_lt_index_chrom_name(const lsq_lt_index *ix, int64_t chrom);
lsq_events *lsq_lt_index_dictionaries(lsq_lt_index *ix);
int64_t lsq_lt_index_num_intervals(const lsq_lt_index *ix);
int64_t lsq_lt_index_unplaced_genes(const lsq_lt_index *ix);
int lsq_lt_host(lsq_lt_index *ix, const char *read_format, const char *path, unsigned skip_flags, unsigned min_mapq, int n_threads, lsq_lt_table **out);
int lsq_lt_host_reads(lsq_lt_index *ix, const lsq_reads *r, int n_threads, lsq_lt_table **out);
int lsq_lt_device(lsq_ctx *c, lsq_lt_index *ix, const char *read_format, const char *path, lsq_lt_table **out);
void lsq_lt_table_free(lsq_lt_table *t);
int lsq_lt_table_counts(const lsq_lt_table *t, uint64_t counts[11]);
int lsq_lt_table_times(const lsq_lt_table *t, float ms[3]);
int lsq_lt_table_verdict(const lsq_lt_table *t, double *forward_fraction, int *has_fraction, const char **library);
int lsq_lt_format(const lsq_lt_table *t, char **out_text);

/* ------------------------------------------------------------------------------------
 * Junction reads per event form of a read file: the junction counts of rMATS, the junction-read PSI of MISO and
 * SUPPA, in count's four columns -- a count table of `test_as fisher --tables` and `test_as lrt --tables`
 * ------------------------------------------------------------------------------------ */

/* The definition, on the arrays the parsers above give (blocks 0-based half-open, in file order, unmerged):
 *   annotation     any isoform file with its gene->isoform file, normally the pair `events` writes.  An event is a gene of the map,
 *                  its forms are its isoform lines; events in the loader's order, an event's forms in the order of its lines in the
 *                  map: the order in which count prints them.  No event is compiled: any number of forms and exons.  An event the
 *                  map gives no isoform (WORMBASE_GENE2ISOFORMS allows it) has no form and no row; an isoform the map names that
 *                  has no line is the loader's error, as for every tool.
 *   chromosomes    as for lsq_jn_index: the distinct chromosome strings of the annotation's isoform lines.  A block on another
 *                  chromosome, or with a coordinate outside +-2^30, has no chromosome (the parsers' own rule).
 *   introns        of a form: the gaps between the maximal intervals of the union of the line's exons with end > start (the first
 *                  exonCount of them), exactly lsq_jn_index_build's; keyed (chromosome, end of the left interval, start of the right
 *                  one).  An intron with an end outside (-2^30, 2^30) matches nothing and is none.
 *   informative    D(f): the introns of form f that are not introns of every form of its event.  An event of one form has none.
 *   junctions      of a read, S(r): exactly lsq_jn's rule -- blocks b and b + 1 in file order, both on a chromosome and on the same one,
 *                  start[b + 1] > end[b], min(length of b, length of b + 1) >= min_overhang (at least 1, else LSQ_E_ARG); the
 *                  junction is (chromosome, end[b], start[b + 1]).  Strand plays no part.
 *   counts         reads[form]: the reads r whose S(r) meets D(f), each once however many of its junctions do; total[event]: the
 *                  reads whose S(r) meets the union of the event's D(f), each once.  An intron may be informative in many forms
 *                  and many events: the read counts in each.  Both are uint64.
 *   report         reads in the file, blocks in the file, junction occurrences that pass the rule, block pairs below the overhang,
 *                  block pairs with a block on no chromosome, occurrences found among the informative introns, reads counted for at
 *                  least one event, reads counted for more than one.
 *   table          a row per form, events in order, zeros included: event TAB total[event] TAB form TAB reads[form] NL.
 *   psi            with_psi appends TAB introns TAB psi, introns = |D(f)|.  On the host, in double, from the integers, in this order:
 *                  x_f = reads_f / introns_f; den = the sum of x_g over the event's forms in row order; psi_f = x_f / den, printed
 *                  %.6f.  Every form of an event prints NA when any of its forms has introns 0 or when den is 0: retained-intron and
 *                  tandem-UTR events, whose one form has no intron of its own, always do.
 * Limits: 2^32-2 forms, 2^32-2 (form, informative intron) pairs, 65 535 chromosomes.  Beyond a limit: LSQ_E_RANGE. */
typedef struct lsq_ps_index lsq_ps_index;       /* the dictionaries, the forms event-major, per chromosome the informative introns with their forms */
typedef struct lsq_ps_table lsq_ps_table;
int lsq_ps_index_build(const lsq_annotation *a, lsq_ps_index **out);
/* Stranded counting, as lsq_xb_index_build_library: the library type belongs to the index, a read has the transcript
 * strand of its first block, and the table is, row by row, the unstranded table of the plus events alone on the reads with t = +
 * and that of the minus events alone on the reads with t = -, in the rows' usual order; introns and --psi's columns follow from
 * the same integers.  Every event needs a strand of its own: LSQ_E_UNSUPPORTED otherwise, naming the first and their number.  The
 * report keeps its eight entries: reads, blocks, occurrences, pairs below the overhang and pairs with a block on no chromosome are
 * those of the unstranded run on the whole annotation; occurrences found, reads counted and reads counted for several events
 * count matches among the events of the read's own strand.  lsq_ps_table_library_report: as lsq_xb_table_library_report. */
int lsq_ps_index_build_library(const lsq_annotation *a, int library, lsq_ps_index **out);
int lsq_ps_index_library(const lsq_ps_index *ix);
int lsq_ps_table_library_report(const lsq_ps_table *t, uint64_t report[5]);
void lsq_ps_index_free(lsq_ps_index *ix);
int64_t lsq_ps_index_num_chroms(const lsq_ps_index *ix);
int64_t lsq_ps_index_num_events(const lsq_ps_index *ix);
int64_t lsq_ps_index_num_forms(const lsq_ps_index *ix);
int64_t lsq_ps_index_num_introns(const lsq_ps_index *ix);                 /* the distinct informative introns */
const char *lsq_ps_index_chrom_name(const lsq_ps_index *ix, int64_t chrom);      /* NULL when out of range */
const char *lsq_ps_index_event_name(const lsq_ps_index *ix, int64_t event);
const char *lsq_ps_index_form_name(const lsq_ps_index *ix, int64_t form);
lsq_events *lsq_ps_index_dictionaries(lsq_ps_index *ix);                  /* as lsq_jn_index_dictionaries */
/* Per event its first form (num_events + 1 entries), per form |D(f)| (the arrays live as long as the index; either pointer may be null) */
int lsq_ps_index_arrays(const lsq_ps_index *ix, const uint32_t **event_first_form, const uint32_t **form_introns);
/* Host-only, threaded: the table from the host parsers' arrays; read_format, skip_flags, min_mapq, statuses and messages as for
 * lsq_jn_host (the name-keyed formats included).  lsq_ps_host_reads: from arrays parsed against the index. */
int lsq_ps_host(lsq_ps_index *ix, const char *read_format, const char *path, unsigned skip_flags, unsigned min_mapq, uint32_t min_overhang, int n_threads,
                lsq_ps_table **out);
int lsq_ps_host_reads(lsq_ps_index *ix, const lsq_reads *r, uint32_t min_overhang, int n_threads, lsq_ps_table **out);
/* Device (HIP, gfx950): "MRF_SINGLE", "SAM_SINGLE" or "BAM_SINGLE", parsed exactly as lsq_jn_device parses it, then one count kernel
 * over the device arrays; the counters alone come back.  The context needs no events, and its events, reads and counters are as
 * they were afterwards.  LSQ_PS_GRID in the environment bounds the count's workgroups (tests). */
int lsq_ps_device(lsq_ctx *c, lsq_ps_index *ix, const char *read_format, const char *path, uint32_t min_overhang, lsq_ps_table **out);
void lsq_ps_table_free(lsq_ps_table *t);
/* reads[num_forms], total[num_events] (they live as long as the table; either pointer may be null) */
int lsq_ps_table_arrays(const lsq_ps_table *t, const uint64_t **reads, const uint64_t **total);
int lsq_ps_table_report(const lsq_ps_table *t, uint64_t report[8]);
/* Device milliseconds per phase of the lsq_ps_device call that made the table -- index upload, count, copy-back -- from HIP events
 * on the library's stream (zeros from the host path); the parse ahead of them: lsq_last_mrf_timing. */
int lsq_ps_table_times(const lsq_ps_table *t, float ms[3]);
/* psi[num_forms] as the text prints it before rounding, NaN where it prints NA */
int lsq_ps_table_psi(const lsq_ps_table *t, double *psi);
/* The table's text, four columns or (with_psi) six; malloc'd, NUL-terminated (lsq_free). */
int lsq_ps_format(const lsq_ps_table *t, int with_psi, char **out_text);

/* ------------------------------------------------------------------------------------
 * Form evidence: junction and exon-body reads per event form of a read file -- the junction counts plus exon counts
 * (JCEC) of rMATS, in count's four columns: a count table of `test_as fisher --tables` and `test_as lrt --tables`.  Beside lsq_ps_*,
 * which stays as it is: a retained-intron event, whose retaining form has no intron of its own, gets its evidence here.
 * ------------------------------------------------------------------------------------ */

/* The definition.  Annotation, chromosomes, events, forms and their order, a form's exon union U(f), its introns, the informative
 * introns D(f) and the junctions S(r) of a read under min_overhang are lsq_ps_*'s above, to the letter.  New:
 *   common bases   C(e): the bases that lie in U(g) of every form g of event e (none where two forms lie on different chromosomes).
 *   body           B(f) = U(f) \ C(e) as maximal intervals, the form's regions.  An event of one form has none.  The regions of one
 *                  form are disjoint and never abut.  Coordinates are clamped to [-2^30, 2^30], as the exon-bin index clamps; a
 *                  region that is empty after clamping is none.
 *   body hit       block b of a read hits region [a, z) of form f when the block is on the form's chromosome (a chromosome of the
 *                  dictionaries: coordinates inside (-2^30, 2^30)), start < end, and min(end_b, z) - max(start_b, a) >= min_body
 *                  (at least 1, else LSQ_E_ARG).  Strand plays no part.
 *   counts         reads[form]: the reads r with a junction of S(r) in D(f) or a block that hits a region of f, each once however
 *                  much of either; total[event]: the reads that count for any form of the event, each once.  A region or intron
 *                  that is informative in several forms or events counts the read in each.  Both are uint64.
 *   report         eleven: reads, blocks, junction occurrences that pass the rule, block pairs below the overhang, block pairs with a
 *                  block on no chromosome, occurrences found among the informative introns (lsq_ps_*'s first six); skipped blocks
 *                  (on no chromosome, out of range or empty); body hits, the (block, region) couples that pass the rule; reads
 *                  counted for at least one event; for more than one; reads counted for an event none of whose junctions is an
 *                  informative intron (counted by body alone).
 *   table          a row per form, events in order, zeros included: event TAB total[event] TAB form TAB reads[form] NL.
 *   positions      of form f under a read length L (1 <= L < 2^18): take every start s of an ungapped L-base read laid along the
 *                  form's own concatenated exon union; its blocks are the pieces of the union's intervals it covers; positions(f)
 *                  is the number of starts at which the counts' rule counts the read for f, 0 when the form is shorter than L.
 *                  Equally: the size of the union, clipped to [0, T - L] (T the form's length), of the windows
 *                  [t - L + min_overhang, t - min_overhang] for each informative intron at transcript offset t whose two neighbouring
 *                  union intervals are both at least min_overhang long, and [a - L + min_body, z - min_body] for each region [a, z) in
 *                  transcript coordinates with z - a >= min_body (none when L < min_body).  A form with an exon beyond +-2^30 is
 *                  enumerated, a piece that leaves the range being a block on no chromosome.
 *   psi            with_psi appends TAB introns TAB body TAB positions TAB psi: |D(f)|, the bases of B(f), positions(f) under the
 *                  table's own min_overhang and min_body.  On the host, in double, from the integers, in this order:
 *                  x_f = reads_f / positions_f; den = the sum of x_g over the event's forms in row order; psi_f = x_f / den, printed
 *                  %.6f.  Every form of an event prints NA when any of its forms has positions 0 or when den is 0.  A tandem-UTR
 *                  event still does: its short form is a subset of the long one, no single read can show it.
 * Limits: lsq_ps_*'s, and 2^32-2 regions.  Beyond a limit: LSQ_E_RANGE. */
typedef struct lsq_fe_index lsq_fe_index;       /* an lsq_ps_index, the regions form-major, per chromosome the cells with the regions that cover them */
typedef struct lsq_fe_table lsq_fe_table;
int lsq_fe_index_build(const lsq_annotation *a, lsq_fe_index **out);
/* Stranded counting, as lsq_xb_index_build_library and lsq_ps_index_build_library: junction and body evidence are
 * sought among the events of the read's transcript strand alone; introns, body, positions and the regions do not change.  The
 * report keeps its eleven entries: reads, blocks, occurrences, pairs below the overhang, pairs with a block on no chromosome and
 * blocks skipped are those of the unstranded run on the whole annotation; occurrences found, body hits, reads counted, counted
 * for several events and counted by body alone count matches among the events of the read's own strand. */
int lsq_fe_index_build_library(const lsq_annotation *a, int library, lsq_fe_index **out);
int lsq_fe_index_library(const lsq_fe_index *ix);
int lsq_fe_table_library_report(const lsq_fe_table *t, uint64_t report[5]);
void lsq_fe_index_free(lsq_fe_index *ix);
int64_t lsq_fe_index_num_chroms(const lsq_fe_index *ix);
int64_t lsq_fe_index_num_events(const lsq_fe_index *ix);
int64_t lsq_fe_index_num_forms(const lsq_fe_index *ix);
int64_t lsq_fe_index_num_introns(const lsq_fe_index *ix);                 /* the distinct informative introns */
int64_t lsq_fe_index_num_regions(const lsq_fe_index *ix);                 /* the regions over all forms */
const char *lsq_fe_index_chrom_name(const lsq_fe_index *ix, int64_t chrom);      /* NULL when out of range */
const char *lsq_fe_index_event_name(const lsq_fe_index *ix, int64_t event);
const char *lsq_fe_index_form_name(const lsq_fe_index *ix, int64_t form);
lsq_events *lsq_fe_index_dictionaries(lsq_fe_index *ix);                  /* as lsq_jn_index_dictionaries */
/* Per event its first form (num_events + 1 entries), per form |D(f)| and the bases of B(f) (the arrays live as long as the index; any pointer may be null) */
int lsq_fe_index_arrays(const lsq_fe_index *ix, const uint32_t **event_first_form, const uint32_t **form_introns, const uint64_t **form_body);
/* positions[num_forms] under a read length and the two thresholds */
int lsq_fe_index_positions(const lsq_fe_index *ix, uint32_t read_length, uint32_t min_overhang, uint32_t min_body, uint64_t *positions);
/* Host-only, threaded: the table from the host parsers' arrays; read_format, skip_flags, min_mapq, statuses and messages as for
 * lsq_jn_host (the name-keyed formats included).  lsq_fe_host_reads: from arrays parsed against the index. */
int lsq_fe_host(lsq_fe_index *ix, const char *read_format, const char *path, unsigned skip_flags, unsigned min_mapq, uint32_t min_overhang, uint32_t min_body, int n_threads,
                lsq_fe_table **out);
int lsq_fe_host_reads(lsq_fe_index *ix, const lsq_reads *r, uint32_t min_overhang, uint32_t min_body, int n_threads, lsq_fe_table **out);
/* Device (HIP, gfx950): "MRF_SINGLE", "SAM_SINGLE" or "BAM_SINGLE", parsed exactly as lsq_jn_device parses it, then one count kernel
 * over the device arrays; the counters alone come back.  The context needs no events, and its events, reads and counters are as
 * they were afterwards.  LSQ_FE_GRID in the environment bounds the count's workgroups (tests). */
int lsq_fe_device(lsq_ctx *c, lsq_fe_index *ix, const char *read_format, const char *path, uint32_t min_overhang, uint32_t min_body, lsq_fe_table **out);
void lsq_fe_table_free(lsq_fe_table *t);
/* reads[num_forms], total[num_events] (they live as long as the table; either pointer may be null) */
int lsq_fe_table_arrays(const lsq_fe_table *t, const uint64_t **reads, const uint64_t **total);
int lsq_fe_table_report(const lsq_fe_table *t, uint64_t report[11]);
/* Device milliseconds per phase of the lsq_fe_device call that made the table -- index upload, count, copy-back -- from HIP events
 * on the library's stream (zeros from the host path); the parse ahead of them: lsq_last_mrf_timing. */
int lsq_fe_table_times(const lsq_fe_table *t, float ms[3]);
/* psi[num_forms] under read_length as the text prints it before rounding, NaN where it prints NA */
int lsq_fe_table_psi(const lsq_fe_table *t, uint32_t read_length, double *psi);
/* The table's text, four columns or (with_psi, under read_length) eight; malloc'd, NUL-terminated (lsq_free). */
int lsq_fe_format(const lsq_fe_table *t, int with_psi, uint32_t read_length, char **out_text);

/* ------------------------------------------------------------------------------------
 * Local events: step 2 of the pipeline, bin/Events.r
 * ------------------------------------------------------------------------------------ */

/* Host-only: the splicing graphs of the genes Events.r walks, in its order, read and checked (no GPU touched).
 * lsq_le_load_matrices reads the gene list (group_path, UCSC_GENE2ISOFORM; read.table + table(): ids convert to
 * integers or doubles when all of them do, and sort numerically then, strings sort in byte order; the ids with more
 * than one line are taken) and <matrix_prefix><id>.matrix for each (classify's files; prefix pasted on as it is).
 * lsq_le_load_annotation does classify in memory instead: every gene with two or more isoforms, named and ordered as
 * the map's ids are.  Input errors (LSQ_E_IO, LSQ_E_PARSE, LSQ_E_ARG, LSQ_E_FORMAT) name the file and line: a missing
 * matrix, a malformed header or row, a coordinate beyond R's integer, an id R reads as NA / logical / hexadecimal, no
 * gene with more than one line.  A gene of fewer than 3 columns is kept (its line is printed) and gives no events. */
typedef struct lsq_le_graphs lsq_le_graphs;
typedef struct lsq_le_result lsq_le_result;
int lsq_le_load_matrices(const char *matrix_prefix, const char *group_path, lsq_le_graphs **out);
int lsq_le_load_annotation(const char *isoform_format, const char *isoforms_path, const char *g2i_format, const char *g2i_path,
                           lsq_le_graphs **out);
void lsq_le_graphs_free(lsq_le_graphs *g);
int64_t lsq_le_num_genes(const lsq_le_graphs *g);
const char *lsq_le_gene_name(const lsq_le_graphs *g, int64_t gene);          /* as Events.r prints it */
int lsq_le_gene_shape(const lsq_le_graphs *g, int64_t gene, int *n_columns, int *n_isoforms);
/* The gene's pos[1..2N] (Events.r:53, the header's digit runs) at *pos; returns 2N (0 for a gene of < 3 columns) */
int64_t lsq_le_gene_positions(const lsq_le_graphs *g, int64_t gene, const int32_t **pos);
/* Device group: Events.r:57-156 for every gene (one wave per gene; any number of columns and isoforms).  The result
 * refers to g, which must outlive it. */
int lsq_le_detect(lsq_ctx *c, const lsq_le_graphs *g, lsq_le_result **out);
void lsq_le_result_free(lsq_le_result *r);
/* type: 0 ES, 1 RI, 2 A5SS, 3 A3SS, 4 MXE, 5 AFE, 6 ALE, 7 T3.  Event q of a type has counter q + 1 and writes two
 * lines to each file; *code is the script's column i (ES .. MXE), the block (AFE / ALE: 0 first-exon, 1 last-exon) or
 * the form (T3: 0 +, 1 -). */
const char *lsq_le_type_name(int type);
int64_t lsq_le_num_events(const lsq_le_result *r, int type);
int lsq_le_event(const lsq_le_result *r, int type, int64_t event, int64_t *gene, int32_t *code);
/* Milliseconds of the detection by HIP events: ms[0] upload, [1] count kernel + scan, [2] emit kernel, [3] download
 * (0 where no event was found and the emit pass did not run) */
int lsq_le_result_times(const lsq_le_result *r, double *ms /* [4] */);
/* The text Events.r appends to <out_prefix><TYPE>.interval and <TYPE>.map (malloc'd; lsq_free) */
int lsq_le_format(const lsq_le_result *r, int type, char **interval_text, char **map_text);
/* Appends both files of every type that has events (none: no file), as the script's write(..., append = T) does */
int lsq_le_write(const lsq_le_result *r, const char *out_prefix);

/* ------------------------------------------------------------------------------------
 * Annotation from GTF: what comes before step 2 of the pipeline, bin/parseGencode and bin/gencodeIsoformMap
 * ------------------------------------------------------------------------------------ */

/* Device group.  Replaces `cat annotation.gtf | parseGencode` (a prebuilt binary; its rules were probed): the
 * GTF's bytes are copied to HBM and every per-byte and per-line step runs there -- the nine TAB-separated fields, the
 * `exon` filter on field 3, atoi of fields 4 and 5, gene_id and transcript_id of field 9 -- and one record per `exon` line
 * comes back; the host orders the transcripts (gene id, then transcript id, bytewise) and sorts each one's starts and
 * ends.  LSQ_E_PARSE with the reference's own "PROBLEM: ..." line in lsq_last_error() for the first line (of any feature)
 * without gene_id or transcript_id or with an unquoted one, and for a line of fewer than nine fields (the reference dies
 * there); lines that are empty or begin with '#' are skipped with a warning (the reference dies there too).
 * lsq_gtf_parse_text takes the bytes from memory (standard input of the executable).  A line may be of any length and the
 * last one needs no newline. */
typedef struct lsq_gtf lsq_gtf;
int lsq_gtf_parse(lsq_ctx *c, const char *path, lsq_gtf **out);
int lsq_gtf_parse_text(lsq_ctx *c, const void *bytes, uint64_t len, lsq_gtf **out);
void lsq_gtf_free(lsq_gtf *g);
int64_t lsq_gtf_num_transcripts(const lsq_gtf *g);        /* output lines of parseGencode: distinct (gene id, transcript id) */
int64_t lsq_gtf_num_genes(const lsq_gtf *g);              /* distinct gene ids */
int64_t lsq_gtf_num_exon_lines(const lsq_gtf *g);         /* `exon` lines of the GTF */
/* Transcript i in output order: "<gene_id>|<transcript_id>", chromosome and strand of its first `exon` line in file order */
const char *lsq_gtf_transcript_name(const lsq_gtf *g, int64_t i);
const char *lsq_gtf_transcript_chrom(const lsq_gtf *g, int64_t i);
const char *lsq_gtf_transcript_strand(const lsq_gtf *g, int64_t i);
/* Its exon starts (field 4 minus 1) and ends (field 5), each list sorted on its own as parseGencode prints them; returns
 * the number of exons (-1: no such transcript).  The arrays live as long as g. */
int64_t lsq_gtf_transcript_exons(const lsq_gtf *g, int64_t i, const int32_t **starts, const int32_t **ends);
/* Replaces parseGencode's output and `cut -f1 x.interval | gencodeIsoformMap`: the LH_GENE_TXT text and the
 * UCSC_GENE2ISOFORM text (malloc'd; lsq_free; either pointer may be null) */
int lsq_gtf_format(const lsq_gtf *g, char **interval_text, char **map_text);
/* Milliseconds of the parse by HIP events: ms[0] copy of the text to HBM, [1] newline scan, [2] parse kernels, [3] download */
int lsq_gtf_result_times(const lsq_gtf *g, double *ms /* [4] */);
/* Host-only (no GPU touched).  Replaces bin/gencodeIsoformMap: every line of names_text behind a counter and a TAB; the
 * counter starts at 1 and goes up where the text before the line's first '|' differs from the line before.  Empty lines
 * are dropped, "\r\n" ends a line as "\n" does, the last line needs no newline.  LSQ_E_PARSE, naming the line, for a line
 * without '|' among others (the reference dies there; it prints such a line when it is the only one, and so does this). */
int lsq_gtf_isoform_map(const char *names_text, uint64_t len, char **map_text);
/* GTF -> annotation -> classify, all in memory: the graphs lsq_le_load_annotation makes from the two files that
 * parseGencode and gencodeIsoformMap write for the same GTF.  Device group (the parse). */
int lsq_le_load_gtf(lsq_ctx *c, const char *path, lsq_le_graphs **out);

/* ------------------------------------------------------------------------------------
 * Synthetic workload; deterministic in (seed, sizes).  Host-only.
 * ------------------------------------------------------------------------------------ */
typedef struct {
	uint64_t seed;
	uint64_t n_events;
	uint64_t n_reads;
	uint32_t read_length;
	uint32_t n_chrom;          /* chr1..chrN */
	uint32_t event_types;      /* bit t set: type t allowed (SE RI A5SS A3SS MXE AFE ALE T3) */
	uint32_t zipf;             /* 0: uniform depth; 1: Zipf(1.1) depth over events */
	double overlap_frac;       /* fraction of events that overlap their left neighbour */
	uint64_t first_read;       /* reads are numbered first_read .. first_read+n_reads-1 in the spec's
	                              read stream (counter-based), so chunks of one stream can be made */
	uint32_t sorted;           /* 1: the reads in coordinate order (chromosome, first base, then their number in the stream) -- what an
	                              aligner's sorted output looks like -- instead of the stream's own (shuffled) order; line numbers follow the file */
	uint32_t reserved;
} lsq_synth_spec;

/* Writes <stem>.interval, <stem>.map and (if write_mrf) <stem>.mrf under dir. */
int lsq_synth_write(const lsq_synth_spec *s, const char *dir, const char *stem, int write_mrf);
/* Generates the reads directly as a read set against already compiled events made from
 * lsq_synth_write's annotation with the same spec (no text round trip). */
int lsq_synth_reads(const lsq_synth_spec *s, lsq_events *e, int n_threads, lsq_reads **out);
/* Writes <stem>.interval, <stem>.map and <stem>.sam: the reads of lsq_synth_write as SAM_SINGLE -- "@HD" / "@SQ" / "@PG" lines
 * first (so read k of the MRF file is line k + 2 + n_chrom here), CIGARs of M and N, NH / NM tag columns, SEQ and QUAL of the
 * read length. */
int lsq_synth_write_sam(const lsq_synth_spec *s, const char *dir, const char *stem);

#ifdef __cplusplus
}
#endif
#endif
