/*
 * besst_amd.h - C ABI of the MI355X scaffold-graph construction library (libbesst_amd.so)
 *
 * This is the drop-in boundary for BESST's hot path
 *     bam_parser -> libmetrics/find_bimodality -> CreateGraph/e_nr_links
 * The reference has no plugin registry: the seam is two Python calls per library,
 *     libmetrics.get_metrics(bam_file, param, Information)          runBESST:168
 *     CreateGraph.PE(Contigs, Scaffolds, Information, C_dict, param,
 *                    small_contigs, small_scaffolds, bam_file)      runBESST:182
 * and its only native precedent is a ctypes call with a caller-allocated result struct and
 * an int return (BESST/diploid/wrapper_sw.py:12-24, swmodule.cpp:20-28,44).  The entry points
 * below follow that convention: extern "C", plain pointers and sizes, int status (0 = ok),
 * never throw, never exit.  besst_amd/_lib.py binds them with ctypes; INTEGRATION.md shows
 * the stub a BESST maintainer would add.
 *
 * Two layers:
 *   besst_ctx_*  host-buffer API.  The context owns all device memory; inputs are host
 *                (numpy) buffers, results come back in caller-allocated host buffers sized by
 *                a preceding *_count call.  This is what the Python drop-in uses.
 *   besst_dev_*  device-pointer API.  Every pointer is an HBM pointer owned by the caller
 *                (e.g. a torch tensor's data_ptr()), work is enqueued on the given hipStream_t
 *                and nothing is allocated or synchronised.  Used by bench.py and by the
 *                multi-GPU path, where the RCCL exchange sits between two besst_dev_ stages.
 *
 * Threading: one caller thread per context (like the reference's single-threaded loop).
 */
#ifndef BESST_AMD_H
#define BESST_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 1: rounds 1-4.  2: + the sharded-scan and BAM-slice entry points of round 5 and the log-normal scoring entry points of
 * round 6 (additions only: a caller built against 1 keeps working).  3: besst_lib_params grew by `mate_bits` (a caller
 * built against 2 passes a shorter struct: recompile), + besst_dev_mate_bits.  Added since without a new version
 * (additions only): the scaffold-output entry points besst_{dev,host}_seq_overlaps / besst_{dev,host}_emit_scaffolds; the
 * FASTA reader besst_dev_fasta_workspace_bytes / besst_dev_fasta_scan / besst_dev_fasta_pack; the text of the output stage
 * besst_dev_text_workspace_bytes / besst_dev_text_measure / besst_dev_text_emit / besst_dev_wrap_fasta,
 * besst_dev_bgzf_deflate_bound / besst_dev_bgzf_deflate_workspace_bytes / besst_dev_bgzf_deflate / besst_bgzf_deflate_device;
 * the inflate of a BGZF file in device memory besst_bgzf_walk / besst_bgzf_scan_chunk /
 * besst_dev_bgzf_inflate_workspace_bytes / besst_dev_bgzf_inflate; of a plain gzip member besst_dev_gzip_plan_workspace_bytes /
 * besst_dev_gzip_plan / besst_dev_gzip_inflate_workspace_bytes / besst_dev_gzip_inflate, of a gzip file of several members
 * besst_dev_gzip_members_plan_workspace_bytes / besst_dev_gzip_members_plan / besst_dev_gzip_members_inflate_workspace_bytes /
 * besst_dev_gzip_members_inflate; the run bits of the record layout besst_dev_record_bits
 * with the trailing member besst_lib_params.tid_bits (see there); the candidate side stream besst_cand_stream with
 * besst_dev_candidate_offsets_bytes / besst_dev_candidate_stream_bytes / besst_dev_candidate_offsets /
 * besst_dev_candidate_stream, the trailing member besst_lib_params.cand_stream, and besst_dev_record_loop_form; the layout
 * a device ingest leaves beside the columns: besst_ctx_layout_state / besst_ctx_fetch_layout; the line cutter of a
 * streamed compressed SAM besst_dev_sam_lines. */
#define BESST_ABI_VERSION 3

/* status codes */
#define BESST_OK 0
#define BESST_ERR_ARG 1     /* bad argument (null pointer, misaligned column, size out of range) */
#define BESST_ERR_HIP 2     /* a HIP runtime call failed; see besst_last_error() */
#define BESST_ERR_STATE 3   /* call order violated (e.g. build before set_library) */
#define BESST_ERR_NOMEM 4
#define BESST_ERR_UNSUPPORTED 5 /* valid input in a form this entry point does not handle; nothing was changed - the
                                * comment of the function names the general one to call instead */

/* Stage 2 (besst_dev_reduce*) reports a table it could not build in the size word the caller reads anyway: *n_rows is
 * one of these instead of a row count, and no other output of the call is valid.  (The besst_ctx_* layer turns the first
 * into BESST_ERR_HIP and handles the second itself.) */
#define BESST_ROWS_SORT_FAILED 0xFFFFFFFFu  /* a wait between workgroups inside a sort launch gave up (chained-scan look-back
                                             * for the predecessor tile; small streams: a partition tile for the others' counts) */
#define BESST_ROWS_RUN_OVERFLOW 0xFFFFFFFEu /* run-grouped form: more runs of equal keys than its buffers hold (a stream
                                             * whose keys do not cluster); repeat the call with BESST_REDUCE_NO_RUNS   */
/* flags of besst_dev_reduce_flags / besst_presort.flags */
#define BESST_REDUCE_NO_RUNS 1u             /* large streams: sort the tuples (chained-scan passes), not runs of them   */

/* contig classes (membership in Contigs / small_contigs, CreateGraph.py:127-130) */
#define BESST_CLS_ABSENT 0
#define BESST_CLS_LARGE 1
#define BESST_CLS_SMALL 2

/* edge-table membership bits: which graph(s) CreateEdge was called for (CreateGraph.py:170-206) */
#define BESST_MASK_G 1u
#define BESST_MASK_GPRIME 2u

/* Per-library constants of the record loop.  Mirrors the fields CreateGraph.PE / CreateEdge read
 * from Parameter.parameter (CreateGraph.py:138,169,175-184,830-840). */
typedef struct besst_lib_params {
    double read_len;           /* param.read_len: may be fractional when inferred (libmetrics.py:265) */
    double ins_size_threshold; /* param.ins_size_threshold (-T), float when inferred                 */
    int32_t min_mapq;          /* param.min_mapq (--min_mapq, default 11)                            */
    int32_t orientation;       /* 0 = 'fr' (PosDirCalculatorPE), 1 = 'rf' (PosDirCalculatorMP)       */
    int32_t detect_duplicate;  /* param.detect_duplicate (-d, default on)                            */
    int32_t extend_paths;      /* param.extend_paths (-y, default on)                                */
    int32_t no_score;          /* param.no_score (--no_score)                                        */
    int32_t record_path;       /* which form of the record loop runs (results are identical): 0 = two passes, the
                                * second over the tid != mtid records only (paired-end libraries: ~1 % of the
                                * records); 1 = one fused pass (mate-pair libraries: ~20 %); pick it from
                                * besst_dev_candidate_density() - the besst_ctx_* layer does that itself          */
    const void* mate_bits;     /* besst_dev_* layer (the besst_ctx_* layer keeps its own): one bit per record of the stream
                                * the call is given - bit i % 8 of byte i / 8 set iff tid[i] != mtid[i] -, made by
                                * besst_dev_mate_bits when the records became resident; the record loop then reads `mtid`
                                * only for the lanes that hold such a record (CreateGraph.py:141-169: everything but the
                                * coverage sum asks for contig1 != contig2).  NULL: the loop compares the columns itself.
                                * (ABI version 3: the struct grew by this member.)                                 */
    const void* tid_bits;      /* besst_dev_* layer: one bit per record, same packing - set iff i == 0 or tid[i] != tid[i-1] -,
                                * made with mate_bits by besst_dev_record_bits.  The fused loop (record_path 1) then reads
                                * `tid` only in the 256-record sub-tiles that hold such a record: in a coordinate-sorted
                                * stream a contig's records are one run.  Only honoured together with mate_bits; NULL: the
                                * loop reads `tid` of every record.  (The struct grew by this trailing member and
                                * BESST_ABI_VERSION stays 3: a caller that zero-fills the struct it passes - every binding
                                * here does - gets NULL, the earlier behaviour; a caller compiled against the shorter
                                * struct must recompile, as at 2 -> 3.)                                           */
    const struct besst_cand_stream* cand_stream;
                               /* besst_dev_* layer: the candidate side stream of the records the call is given (see
                                * besst_cand_stream below), made by besst_dev_candidate_offsets + besst_dev_candidate_stream.
                                * The fused loop then reads pos / mpos / mtid / flag of no record: its evaluation rounds
                                * read the stream's entries.  Only honoured together with mate_bits AND tid_bits, and only
                                * when the stream's n_refs equals the call's n_contigs and its n_records the call's
                                * n_records; otherwise, or NULL, or with BESST_CAND_STREAM=0 in the environment: the loop
                                * runs as with the two bit planes.  (Trailing member, same rule as tid_bits.)       */
} besst_lib_params;

/* The candidate side stream: the eleventh column group of the resident record layout.  A compacted copy, in record
 * order, of the records that can reach an evaluation round of the record loop.  Record i is in the set iff
 *     tid[i] != mtid[i]  and  ( (flag & 0x80 and not flag & 0x4)  or  (flag & 0x4 and flag & 0x40)
 *                               or  (uint32) mtid[i] >= n_refs )
 * - read 2 and mapped, or the unmapped-read-1 quirk, or a mate reference outside the header (so that every
 * mate-elsewhere record OUTSIDE the set has 0 <= mtid < n_refs).  The rule takes no library parameter; n_refs is the
 * number of header references the stream was made for.  Everything here lies in device memory and is derived from the
 * record columns: IT MUST BE MADE AGAIN WHEN ANY OF tid, mtid, pos, mpos, flag, mapq, qlen CHANGES.
 *   set_bits   one bit per record, packed like mate_bits: the record is in the set; bits behind the last record 0
 *   offsets    n_blocks + 1 values, n_blocks = ceil(n_records / 16384): block b (records 16384 b ...) owns the
 *              entries [offsets[b], offsets[b + 1]); offsets[n_blocks] == n_entries
 *   columns    per entry: tid, mtid, pos, mpos (int32), flag_qlen (uint32: flag | qlen << 16), mapq (uint8) - 21 bytes;
 *              each column holds at least one entry more than n_entries (idle lanes of the loop read it) */
typedef struct besst_cand_stream {
    int64_t n_refs;
    int64_t n_records;
    int64_t n_entries;
    const void* offsets;
    const void* set_bits;
    const void* tid;
    const void* mtid;
    const void* pos;
    const void* mpos;
    const void* flag_qlen;
    const void* mapq;
} besst_cand_stream;

/* Tallies of the record loop: Parameter.counters (Parameter.py:113-124) plus the fishy-read count
 * `ctr` of CreateGraph.py:100,163 and the sizes of the emitted tuple stream. */
typedef struct besst_counters {
    int64_t count;                      /* counter.count ("USEFUL READS", per CreateEdge call)      */
    int64_t non_unique;                 /* counter.non_unique                                        */
    int64_t non_unique_for_scaf;        /* counter.non_unique_for_scaf                               */
    int64_t nr_of_duplicates;           /* counter.nr_of_duplicates                                  */
    int64_t reads_with_too_long_insert; /* counter.reads_with_too_long_insert                        */
    int64_t fishy_reads;                /* ctr                                                       */
    int64_t n_tuples;                   /* link + fishy tuples written to the sort buffer            */
    int64_t n_reach;                    /* records that reached CreateEdge                           */
    int32_t prev_obs1;                  /* counter.prev_obs1 after the last record                   */
    int32_t prev_obs2;                  /* counter.prev_obs2                                         */
} besst_counters;

/* Library-statistics sampling pass (libmetrics.py:49-131,283-304).  All counts are over the scanned
 * prefix of the stream, honouring the reference's 1,000,000-sample cut-offs in stream order. */
typedef struct besst_metrics_counts {
    int64_t n_isize;        /* observations collected for the insert-size sample (<= 1,000,000)     */
    int64_t n_contam;       /* opposite-orientation fragments collected (contamination_reads)       */
    int64_t counter_total;  /* mapped records on the 1000 longest contigs within the cut-off       */
    int64_t sample_counter; /* records on the 1000 longest contigs within the cut-off (<= 1,000,000) */
    int64_t records_scanned;
} besst_metrics_counts;

typedef struct besst_ctx besst_ctx;

/* ------------------------------------------------------------------------------------------------
 * library
 * ---------------------------------------------------------------------------------------------- */
int besst_abi_version(void);
/* Last error text of the calling thread's most recent failing call (never NULL). */
const char* besst_last_error(void);

/* The pinned staging buffers of besst_ctx_push_bam / besst_ctx_push_bam_device are kept in a process-wide pool between
 * calls (pinning and unpinning host memory costs ~90 ms per GB: a third of the ingest of a 40 M-record file); at most 1 GiB
 * stays cached.  This call frees what is idle in the pool (a long-lived host process that is done reading files). */
void besst_release_cached_memory(void);

/* Number of visible HIP devices, or a negative status. */
int besst_device_count(void);

/* Per-kernel timing with HIP events recorded on the launch stream (bench.py's roofline numbers).
 * Off by default; slot_mask selects the kernels to time (bit i = slot i, 0 = off).
 * besst_prof_collect synchronises the recorded events, sums elapsed milliseconds and
 * launch counts per slot (besst_prof_slots() entries, names from besst_prof_slot_name) and resets.
 * besst_prof_sample_every(n) times only every n-th launch of an enabled slot: an event pair costs the stream
 * ~3 us, which a 120 us step notices when every launch is timed. */
void besst_prof_enable(uint32_t slot_mask);
void besst_prof_sample_every(uint32_t n);
int besst_prof_slots(void);
const char* besst_prof_slot_name(int slot);
int besst_prof_collect(int n_slots, double* ms, int64_t* launches);

/* ------------------------------------------------------------------------------------------------
 * host-buffer API (context owns HBM)
 * ---------------------------------------------------------------------------------------------- */
besst_ctx* besst_ctx_create(int device);
void besst_ctx_destroy(besst_ctx* ctx);

/* Contig table, one row per BAM header entry (tid order).  Replaces the Contigs / small_contigs /
 * Scaffolds / small_scaffolds lookups of the record loop (CreateGraph.py:127-130,144-174,819-829).
 * scaf_id must be in [1, 2^28). */
int besst_ctx_set_contigs(besst_ctx* ctx, int64_t n_contigs, const int32_t* scaf_id,
                          const int32_t* scaf_len, const int32_t* ctg_pos, const int32_t* ctg_len,
                          const uint8_t* direction, const uint8_t* cls);

int besst_ctx_set_library(besst_ctx* ctx, const besst_lib_params* params);

/* Drop all records held by the context (start of a new library). */
int besst_ctx_clear_records(besst_ctx* ctx);

/* Append a batch of alignment records (SoA columns = the pysam attributes the hot path reads:
 * rname mrnm pos mpos tlen flag mapq qlen).  Records stay resident in HBM. */
int besst_ctx_push_records(besst_ctx* ctx, int64_t n, const int32_t* tid, const int32_t* mtid,
                           const int32_t* pos, const int32_t* mpos, const int32_t* tlen,
                           const uint16_t* flag, const uint8_t* mapq, const uint16_t* qlen);

/* The resident records back on the host (any column pointer may be NULL): what a caller that ingested a file straight
 * into HBM (below) needs to look at the records themselves; also how the tests compare the two ingest forms. */
int besst_ctx_record_count(besst_ctx* ctx, int64_t* n_records);
/* The resident columns where they lie: eight HBM pointers (tid mtid pos mpos tlen flag mapq qlen) for the besst_dev_*
 * layer - a rank of the sharded build works on the slice its besst_ctx_push_bam_device_part left here, no copy.  Valid
 * until the context's records change or the context is destroyed. */
int besst_ctx_record_pointers(besst_ctx* ctx, int64_t* n_records, uint64_t* ptrs);
int besst_ctx_fetch_records(besst_ctx* ctx, int64_t first, int64_t n, int32_t* tid, int32_t* mtid, int32_t* pos,
                            int32_t* mpos, int32_t* tlen, uint16_t* flag, uint8_t* mapq, uint16_t* qlen);

/* The same from a BAM file, streamed (replaces `pysam.Samfile(param.bamfile, 'rb')` + the iteration of runBESST:162,
 * CreateGraph.py:111, libmetrics.py:63,257,293): the reader's host threads inflate and decode chunk k + 1 into pinned
 * staging columns while chunk k's asynchronous copies travel to HBM.  `bam` is an open besst_bam (below) positioned at
 * its first unread record; reads to the end of the file.  The first head_records records' rlen / alen / qlen - all
 * libmetrics' read-length step looks at (libmetrics.py:246-273: 1000 records) - are returned in the head_* arrays.
 * chunk_records <= 0 picks 4 Mi records (two staging sets of 19 B per record). */
typedef struct besst_bam besst_bam;
typedef struct {
    int64_t records;             /* records appended to the context */
    int64_t chunks;
    int64_t bytes_h2d;
    double seconds;              /* wall time of the call */
    double decode_seconds;       /* of which the calling thread spent in the reader (inflate + record decode; device form:
                                  * copying the compressed bytes off the mapping into pinned staging) */
    double copy_wait_seconds;    /* and blocked on copies (device form: and kernels) that had not finished */
    int64_t inflated_bytes;      /* device form: bytes the BGZF blocks inflated to */
    int64_t blocks;              /* device form: BGZF blocks */
    int32_t on_device;           /* 1: inflate + record decode ran on the GPU (bytes_h2d = the compressed bytes) */
    int32_t starts_repaired;     /* device form: blocks whose guessed first record start the verification replaced (0 in htslib's layout) */
} besst_ingest_stats;
int besst_ctx_push_bam(besst_ctx* ctx, besst_bam* bam, int64_t chunk_records, int64_t head_records, int32_t* head_rlen,
                       int32_t* head_alen, uint16_t* head_qlen, besst_ingest_stats* stats);

/* The same with BGZF inflate, record walk and record decode ON THE GPU (csrc/bgzf_gpu.hip): the file's compressed bytes
 * are what crosses PCIe - staged through pinned memory chunk by chunk (chunk_blocks BGZF blocks, <= 0: 8192), chunk
 * j + 1 uploaded while chunk j inflates (one wave per block).  ANY block layout: htslib's (samtools, bwa | samtools, this
 * library's writer), where every BGZF block begins with a record, and htsjdk's / Picard's, where blocks are cut wherever
 * 64 KiB of data end - a chunk's blocks are inflated back to back, the first record start of every block is guessed from
 * the bytes and VERIFIED from block to block (a wrong guess is replaced by what the block before it says and the block
 * is walked again), and the record that a chunk does not finish travels in front of the next chunk's first block (at most
 * 4 MiB).  Returns BESST_ERR_UNSUPPORTED - context and reader unchanged - for a block the device does not inflate or
 * whose CRC-32 does not match its gzip trailer and for record starts that cannot be established: call besst_ctx_push_bam
 * then (which checks the CRC-32 too and reports the file as corrupt, as htslib would). */
int besst_ctx_push_bam_device(besst_ctx* ctx, besst_bam* bam, int64_t chunk_blocks, int64_t head_records, int32_t* head_rlen,
                              int32_t* head_alen, uint16_t* head_qlen, besst_ingest_stats* stats);

/* The same for one PART of the file's records - multi-GPU ingest: rank r of W calls it with (r, W) and holds the r-th
 * contiguous slice of the stream, the slice phase 1 of the sharded graph build works on.  The file is
 * cut at the BGZF block boundaries nearest to part / parts of its bytes; every caller finds the same boundaries on its own
 * (gzip magic + BC subfield + two chained blocks behind it).  The head_* arrays describe the part's first records.
 * parts > 1 needs htslib's layout, where every block boundary is a record boundary: BESST_ERR_UNSUPPORTED (context and
 * reader unchanged) for a file whose records straddle blocks - such files take besst_ctx_push_bam_device_slice. */
int besst_ctx_push_bam_device_part(besst_ctx* ctx, besst_bam* bam, int32_t part, int32_t parts, int64_t chunk_blocks,
                                   int64_t head_records, int32_t* head_rlen, int32_t* head_alen, uint16_t* head_qlen,
                                   besst_ingest_stats* stats);

/* Slice `part` of `parts` of a file in ANY block layout (multi-GPU ingest of files whose records straddle BGZF blocks:
 * htsjdk / Picard).  The slices are cut at block boundaries as above, and a record belongs to the slice it BEGINS in.  Where
 * a slice's first record begins is the one thing a rank cannot know alone:
 *   first_skip < 0   the rank guesses (the heuristics of the block-to-block verification; everything behind the guess is
 *                    verified as usual);
 *   first_skip >= 0  the first record begins that many inflated bytes behind the slice's first block's first byte.
 * boundary[0] reports the offset used, boundary[1] how many bytes of the slice's last record lie in the next slice (they
 * are read from the blocks that follow, at most 4 MiB).  The callers exchange the two numbers: slice r is right iff
 * boundary[0] of slice r equals boundary[1] of slice r - 1 (slice 0 begins behind the header and is always right); a slice
 * whose guess was wrong is read again - into a fresh context - with first_skip = boundary[1] of the slice before
 * (besst_amd.distributed.ingest_slice runs this protocol).  In htslib's layout both numbers are 0. */
int besst_ctx_push_bam_device_slice(besst_ctx* ctx, besst_bam* bam, int32_t part, int32_t parts, int64_t chunk_blocks,
                                    int64_t first_skip, int64_t* boundary, int64_t head_records, int32_t* head_rlen,
                                    int32_t* head_alen, uint16_t* head_qlen, besst_ingest_stats* stats);

/* What a context holds of the ninth to eleventh column groups of its resident records - the mate-elsewhere and run planes
 * (besst_dev_record_bits) and the candidate side stream (besst_cand_stream) - and who made it.  The three device forms
 * above write all of it WHILE THEY DECODE, bit for bit what the makers would write from the finished columns (the stream
 * for n_refs = the file's reference count), and move the watermarks to the last record; besst_ctx_build_graph then
 * launches no maker and waits for no entry count.  besst_ctx_push_bam and besst_ctx_push_records leave the watermarks
 * where they are, and the next build extends planes and stream from there.  A device form continues only what stands at
 * the context's last record when it is called; entries that do not fit the columns reserved for them (sized from the
 * record reservation: an entry per record at first, the share of records with an entry so far plus a quarter wherever the
 * record columns grow, cut back to the entries made + 4096 at the end; BESST_INGEST_ENTRY_ROOM=<entries> in the environment
 * replaces the first), or whose buffers cannot be allocated, leave cs_upto where it was, and the build makes the stream.
 * BESST_INGEST_LAYOUT=0 in the environment, read at every call: the device forms write the eight columns alone.
 *   out[0] n_records       out[1] bits_upto: records the mate-elsewhere plane is valid for       out[2] the same, run plane
 *   out[3] cs_upto: records the side stream is valid for      out[4] its n_entries     out[5] its n_refs  (0 0 without one)
 *   out[6] entries each entry column has room for
 *   out[7] maker launches (planes, offsets, entries: one each) by besst_ctx_build_graph since the context was created */
int besst_ctx_layout_state(besst_ctx* ctx, int64_t* out);
/* The valid prefix of that layout back on the host, for tests and tools (any pointer may be NULL; the bits behind a
 * watermark in the byte that holds it come back 0): (bits_upto + 7) / 8 and (tid_bits_upto + 7) / 8 bytes of the two planes; with a stream (cs_upto > 0) (cs_upto + 7) / 8 bytes of the set plane,
 * ceil(cs_upto / 16384) + 1 offsets and n_entries values of each of the six entry columns. */
int besst_ctx_fetch_layout(besst_ctx* ctx, uint8_t* mate_bits, uint8_t* tid_bits, uint8_t* set_bits, uint32_t* offsets,
                           int32_t* tid, int32_t* mtid, int32_t* pos, int32_t* mpos, uint32_t* flag_qlen, uint8_t* mapq);

/* Test hook of the device inflate: the BGZF blocks of `bgzf` (n_bytes, host) inflated on `device`, their output
 * concatenated in out (capacity out_cap, length in *out_len).  BESST_ERR_UNSUPPORTED when a block does not inflate
 * (its index and status in besst_last_error()). */
int besst_bgzf_inflate_device(int device, const void* bgzf, size_t n_bytes, void* out, size_t out_cap, size_t* out_len);

/* ---- BGZF inflate from device memory into device memory (csrc/bgzf_gpu.hip; GenerateOutput.py: SequenceStore.from_fasta) --
 * What a BGZF block is here (csrc/bgzf_scan.h): a gzip member with FEXTRA whose FIRST extra subfield is BC (further
 * subfields may follow it), BSIZE that fits, ISIZE <= 65536.  Empty blocks may stand anywhere; no EOF block is needed.
 *   besst_bgzf_walk        (host, no GPU) the chain of blocks from bgzf[0] on, max_blocks at most (< 0: all): their number,
 *                          the sum of their ISIZE, and *end: the offset of the first byte that is no whole BGZF block
 *                          (n_bytes: the range is BGZF to its last byte).  Always BESST_OK but for null pointers.
 *   besst_bgzf_scan_chunk  (host, no GPU) the descriptors of the blocks of window[from, n_bytes), max_blocks at most, laid
 *                          back to back from inflated offset dst0 on; src_off counts from window[0].  more_follows != 0:
 *                          the window is a part of a file and a block cut by its end stops the scan in front of it
 *                          (0: such a block is an error).  *comp_bytes: bytes of the window the blocks take, from `from`.
 *                          BESST_ERR_ARG: bytes that are no BGZF block where one should begin (the counts are not
 *                          written; `blocks` may hold the blocks in front of that place).
 *   besst_dev_bgzf_inflate_workspace_bytes  status words and symbol buffer of one launch of n_blocks blocks (<= 2^24) that
 *                          inflate to inflated_bytes (<= 65536 n_blocks); 0: arguments out of range.
 *   besst_dev_bgzf_inflate enqueues on `stream`: the inflate of the n_blocks blocks (device descriptors; payloads in comp,
 *                          4-byte aligned, with 4096 readable bytes behind the last payload) to dst + their dst_off, every
 *                          dst_off + dst_len within inflated_bytes; the CRC-32 check; and the reduction of the blocks'
 *                          statuses into *first_bad (device): the minimum, over this and every earlier launch, of
 *                          (block_base + index of the block) << 8 | reason - reason 1..8: the DEFLATE data is not what the
 *                          kernel takes, BESST_BGZF_BAD_SIZE: inflated length != ISIZE, BESST_BGZF_BAD_CRC.  The caller
 *                          sets *first_bad to all ones once per file; it still is when every block was good.  Up to 15
 *                          bytes in front of dst + dst_off (never across a 16-byte boundary) and behind the block's end
 *                          are read by the CRC check and not used.  BESST_ERR_ARG without touching the device: a null
 *                          pointer, n_blocks or block_base < 0, sizes out of range, a workspace smaller than asked for. */
#define BESST_BGZF_BAD_SIZE 9
#define BESST_BGZF_BAD_CRC 10
typedef struct besst_bgzf_block {
    uint32_t src_off, src_len;       /* the DEFLATE payload in the compressed bytes */
    uint32_t dst_off_lo, dst_off_hi; /* where its inflated bytes go */
    uint32_t dst_len, crc;           /* ISIZE and CRC-32 of the gzip trailer */
} besst_bgzf_block;
int besst_bgzf_walk(const void* bgzf, size_t n_bytes, int64_t max_blocks, int64_t* n_blocks, int64_t* inflated_bytes,
                    size_t* end);
int besst_bgzf_scan_chunk(const void* window, size_t n_bytes, size_t from, int32_t more_follows, int64_t max_blocks,
                          uint64_t dst0, besst_bgzf_block* blocks, int64_t* n_blocks, size_t* comp_bytes,
                          int64_t* inflated_bytes);
size_t besst_dev_bgzf_inflate_workspace_bytes(int64_t n_blocks, int64_t inflated_bytes);
int besst_dev_bgzf_inflate(void* stream, const void* comp, const besst_bgzf_block* blocks, int64_t n_blocks,
                           int64_t block_base, int64_t inflated_bytes, void* dst, void* workspace, size_t workspace_bytes,
                           uint64_t* first_bad);

/* ---- a plain gzip member inflated from device memory into device memory (csrc/gzip_stream.hip; GenerateOutput.py:
 * SequenceStore.from_fasta(gzip_on_gpu=True)) ---------------------------------------------------------------------------
 * The file (comp_bytes, 4-byte aligned, readable up to the dword that holds its last byte) is ONE gzip member whose DEFLATE
 * data begins at byte data_off (the caller parses the gzip header) and whose last eight bytes are the trailer.  The data is
 * cut into chunks of chunk_bytes (a multiple of 16 in 256..2^24); DESIGN.md section 11.2 has the scheme.  Two calls with one
 * read of `info` between them (the text's size is not known before):
 *   besst_dev_gzip_plan_workspace_bytes     the per-chunk words of a file of that geometry; 0: arguments out of range
 *                          (comp_bytes < data_off + 8, comp_bytes > 2^35, a chunk size that is none).
 *   besst_dev_gzip_plan    enqueues on `stream`: the probe (a candidate block start per chunk), the count (a wave per chunk:
 *                          where it lands, the bytes until there) and the link (the live chunks and their places).  Leaves
 *                          info[0..8) (device): BESST_GZIP_INFO_STATUS (0, or the reason the member is not taken: 1..8 the
 *                          DEFLATE data of a live chunk, BESST_GZIP_BAD_SIZE the text is not ISIZE bytes modulo 2^32,
 *                          BESST_GZIP_TRAILING the final block's trailer is not the file's end - another member follows),
 *                          _TEXT (bytes the member inflates to), _CHUNKS, _CANDIDATES (chunks behind the first that hold a
 *                          block start), _LIVE (chunks on the chain from chunk 0), _END_BIT, _BAD_CHUNK.
 *   besst_dev_gzip_inflate_workspace_bytes  two bytes per byte of text (the symbols), a status per live chunk, the CRC's
 *                          partial values; 0: arguments out of range (n_live < 1).
 *   besst_dev_gzip_inflate enqueues on `stream`, for the plan in plan_workspace and the n_live and text_bytes read from its
 *                          info: the decode into symbols, the windows, the translation into text[0, text_bytes) (16-byte
 *                          aligned) and the CRC-32 against the trailer.  info[BESST_GZIP_INFO_STATUS] (device) is still 0
 *                          when the text is good; BESST_GZIP_BAD_CRC, or 1..9 from the decode, when it is not (the text's
 *                          bytes mean nothing then).  No byte outside the buffers is touched whatever the data holds.
 * steps: 0 = every step; else a bit mask of the steps to enqueue (plan: 1 probe, 2 count, 4 link; inflate: 1 decode,
 * 2 windows, 4 translate, 8 CRC) - for timing them one by one, in order, on the same buffers.
 * BESST_ERR_ARG without touching the device: a null pointer, sizes out of range, a misaligned buffer, a workspace smaller
 * than asked for. */
#define BESST_GZIP_BAD_SIZE 9
#define BESST_GZIP_BAD_CRC 10
#define BESST_GZIP_TRAILING 11
#define BESST_GZIP_INFO_WORDS 8
#define BESST_GZIP_INFO_STATUS 0
#define BESST_GZIP_INFO_TEXT 1
#define BESST_GZIP_INFO_CHUNKS 2
#define BESST_GZIP_INFO_CANDIDATES 3
#define BESST_GZIP_INFO_LIVE 4
#define BESST_GZIP_INFO_END_BIT 5
#define BESST_GZIP_INFO_BAD_CHUNK 6
#define BESST_GZIP_INFO_CRC 7
size_t besst_dev_gzip_plan_workspace_bytes(int64_t comp_bytes, int64_t data_off, int64_t chunk_bytes);
int besst_dev_gzip_plan(void* stream, const void* comp, int64_t comp_bytes, int64_t data_off, int64_t chunk_bytes,
                        int32_t steps, void* workspace, size_t workspace_bytes, uint64_t* info);
size_t besst_dev_gzip_inflate_workspace_bytes(int64_t text_bytes, int64_t n_live);
int besst_dev_gzip_inflate(void* stream, const void* comp, int64_t comp_bytes, int64_t data_off, int64_t chunk_bytes,
                           int32_t steps, const void* plan_workspace, int64_t n_live, int64_t text_bytes, void* text,
                           void* workspace, size_t workspace_bytes, uint64_t* info);

/* ---- a gzip file of SEVERAL members (RFC 1952: `cat a.gz b.gz`, multi-member compressors, `gzip -c >>`, a BGZF chain behind
 * or in front of a foreign member), inflated the same way into one text.  The four calls above, member-aware; the file's
 * first member begins at byte 0 and its DEFLATE data at data_off, every later member is found on the device:
 *   - every byte offset behind the first that reads 1f 8b 08 and a FLG without reserved bits is a MEMBER CANDIDATE; the
 *     list holds member_cap of them (0..2^28; GenerateOutput.py asks for comp_bytes / 256 + 4096).  More than that:
 *     BESST_GZIP_TOO_MANY_MEMBERS, and nothing else is looked at.  A candidate's header is parsed on the device (CM = 8;
 *     FEXTRA, FNAME, FCOMMENT - 65536 bytes each at most - and FHCRC skipped), and its first blocks are walked by a wave
 *     of its own.  Candidates that are no member (in compressed data, a stored block, another header) are never asked for.
 *   - the link passes from a member's final block over its trailer (ISIZE against the member's own bytes) to the candidate
 *     that begins at the next byte; none there, or no header: BESST_GZIP_TRAILING.  What is live is a SEGMENT (the walk
 *     from a chunk's candidate or from a member's first block): n_live may exceed the number of chunks.
 *   - a match may reach its member's first byte and not one further (BESST status 6), and every member's CRC-32 is held
 *     against its own trailer; the first bad member by file order is the one reported.
 * info[0..16) (device): the words above (_CRC: the last member's), then _MEMBERS (members on the chain), _MEMBER_CANDIDATES
 * (as counted, also when they are too many), _BAD_MEMBER (index by file order of the member the status is about, ~0: none)
 * and _BAD_MEMBER_OFFSET (its first byte in the file); the rest is 0.  Still one read of info between plan and inflate:
 * n_live, n_members and text_bytes come from it.  On a file of one member chunks, candidates, live and text are what
 * besst_dev_gzip_plan leaves. */
#define BESST_GZIP_TOO_MANY_MEMBERS 12
#define BESST_GZIP_MEMBER_INFO_WORDS 16
#define BESST_GZIP_INFO_MEMBERS 8
#define BESST_GZIP_INFO_MEMBER_CANDIDATES 9
#define BESST_GZIP_INFO_BAD_MEMBER 10
#define BESST_GZIP_INFO_BAD_MEMBER_OFFSET 11
size_t besst_dev_gzip_members_plan_workspace_bytes(int64_t comp_bytes, int64_t data_off, int64_t chunk_bytes, int64_t member_cap);
int besst_dev_gzip_members_plan(void* stream, const void* comp, int64_t comp_bytes, int64_t data_off, int64_t chunk_bytes,
                                int64_t member_cap, int32_t steps, void* workspace, size_t workspace_bytes, uint64_t* info);
size_t besst_dev_gzip_members_inflate_workspace_bytes(int64_t text_bytes, int64_t n_live, int64_t n_members);
int besst_dev_gzip_members_inflate(void* stream, const void* comp, int64_t comp_bytes, int64_t data_off, int64_t chunk_bytes,
                                   int64_t member_cap, int32_t steps, const void* plan_workspace, int64_t n_live,
                                   int64_t n_members, int64_t text_bytes, void* text, void* workspace, size_t workspace_bytes,
                                   uint64_t* info);

/* libmetrics sampling (replaces the three `for read in bam_file` scans, libmetrics.py:63,257,293).
 * top_mask[tid] != 0 marks the 1000 longest references.  orientation/min_mapq/read_len as in
 * besst_lib_params.  isize_out / contam_out receive |tlen| of the qualifying records in stream order
 * (capacity 1,000,000 each); the host adds 2*read_len where the reference does. */
int besst_ctx_metrics_sample(besst_ctx* ctx, const uint8_t* top_mask, int32_t orientation,
                             int32_t min_mapq, double read_len, int32_t want_isize,
                             int32_t* isize_out, int32_t* contam_out, besst_metrics_counts* counts);

/* Is the resident stream sorted by coordinate?  Replaces the reference's index check - `bam_file.fetch(cont_names[0])`
 * raising for a BAM without an index, BESST/libmetrics.py:237-241; an index exists only for a coordinate-sorted file.
 * *first_unsorted: -1, or the index of the first record whose (reference id, position) lies in front of its predecessor's
 * (reference -1 sorts last, as `samtools sort` leaves it).  The graph build is exact on any order but several times slower
 * on an unsorted stream; libmetrics.get_metrics turns a hit into the reference's message as a WARNING.  first_key /
 * last_key (each 2 x int32, may be NULL): (tid, pos) of the first and last resident record, for the slices of a sharded
 * stream to compare across ranks.  besst_dev_stream_order: the same pass on caller-owned columns, *first_unsorted on the
 * device. */
int besst_ctx_stream_order(besst_ctx* ctx, int64_t* first_unsorted, int32_t* first_key, int32_t* last_key);
int besst_dev_stream_order(void* stream, int64_t n, const int32_t* tid, const int32_t* pos, int64_t* first_unsorted);

/* The BAM report: what the resident record columns hold, counted over ALL records in one pass (csrc/report.hip) - the
 * numbers of `samtools flagstat` and `samtools idxstats`, the mapq / aligned-length / insert-size distributions and a
 * digest of the columns.  The result is besst_dev_library_report_words(n_refs, isize_bins) 64-bit words, every one an
 * exact sum over the records (word 39 an xor), so reports of the slices of a stream add up to the report of the stream:
 *   [0, 32)   flag census, row r at 2 r (QC-pass) and 2 r + 1 (QC-fail, flag & 0x200), rows in samtools flagstat's order:
 *             0 total, 1 primary, 2 secondary, 3 supplementary, 4 duplicates, 5 primary duplicates, 6 mapped,
 *             7 primary mapped, 8 paired in sequencing, 9 read1, 10 read2, 11 properly paired, 12 with itself and mate
 *             mapped, 13 singletons, 14 with mate mapped to a different chr, 15 the same with mapQ >= 5.
 *             secondary: 0x100; supplementary: 0x800 without 0x100; primary: neither; mapped: not 0x4; rows 8-15 count
 *             primary records with 0x1: read1 0x40, read2 0x80, properly paired 0x2 and not 0x4, singletons 0x8 and not
 *             0x4, itself and mate mapped neither 0x4 nor 0x8, different chr: of those, tid != mtid
 *   32        unplaced: records with tid < 0            33   tid_out_of_range: records with tid >= n_refs
 *   [34, 38)  pairs on one reference by class - innie, outie, tandem, other - each pair counted once, from its record with
 *             primary, 0x1, 0x80, not 0x4, not 0x8, tid == mtid, 0 <= tid < n_refs.  rev = 0x10, mrev = 0x20:
 *             tandem rev == mrev; else other tlen == 0; else innie (rev and tlen < 0) or (mrev and tlen > 0); else outie
 *   38, 39    digest: sum (mod 2^64) and xor over the records of
 *                 h = splitmix64(splitmix64(splitmix64(splitmix64(a) ^ b) ^ c) ^ mapq)
 *                 a = (u32)tid | (u64)(u32)mtid << 32, b = (u32)pos | (u64)(u32)mpos << 32,
 *                 c = (u32)tlen | (u64)flag << 32 | (u64)qlen << 48
 *                 splitmix64(x): x += 0x9e3779b97f4a7c15; x = (x ^ x >> 30) * 0xbf58476d1ce4e5b9;
 *                                x = (x ^ x >> 27) * 0x94d049bb133111eb; return x ^ x >> 31
 *   [40, 296)          mapq histogram of the records without 0x4
 *   [296, 65832)       qlen (stored aligned query length, clamped at 65535) histogram of the records without 0x4
 *   [65832, + n_refs)  mapped[i]: records with tid == i without 0x4;  then n_refs words placed_unmapped[i]: with 0x4
 *   then 3 x (isize_bins + 1) words: |tlen| histogram of the innie pairs, of the outie pairs, of the tandem pairs; bin
 *   isize_bins of each counts |tlen| >= isize_bins (|tlen| in 64 bits: INT32_MIN lands there)
 * besst_dev_library_report: caller-owned device columns at any element-aligned address (a slice of a stream), `out` a
 * device buffer of out_words >= besst_dev_library_report_words(...) words that the call zeroes on `stream`; nothing is
 * allocated or synchronised.  tid_bits: optional, the run-bit plane of the records (besst_lib_params.tid_bits); a hint
 * only - the present kernel reads tid itself, the result never depends on it.  0 <= n_records < 2^32, 0 <= n_refs < 2^31,
 * 1 <= isize_bins <= 2^20.
 * besst_ctx_library_report: the same over the context's resident records (n_refs: the contig count of set_contigs), on the
 * context's stream, fetched into out_host (out_words words).  It only reads: no watermark, plane or side stream moves. */
#define BESST_REPORT_CENSUS 0
#define BESST_REPORT_UNPLACED 32
#define BESST_REPORT_TID_OUT_OF_RANGE 33
#define BESST_REPORT_PAIR_CLASSES 34
#define BESST_REPORT_DIGEST_SUM 38
#define BESST_REPORT_DIGEST_XOR 39
#define BESST_REPORT_MAPQ 40
#define BESST_REPORT_QLEN 296
#define BESST_REPORT_REFS 65832
#define BESST_REPORT_MAX_ISIZE_BINS (1 << 20)
typedef struct besst_report_args {
    const int32_t* tid;
    const int32_t* mtid;
    const int32_t* pos;
    const int32_t* mpos;
    const int32_t* tlen;
    const uint16_t* flag;
    const uint8_t* mapq;
    const uint16_t* qlen;
    const void* tid_bits;
    int64_t n_records;
    int64_t n_refs;
    int64_t isize_bins;
    int64_t out_words;
} besst_report_args;
int64_t besst_dev_library_report_words(int64_t n_refs, int64_t isize_bins);
int besst_dev_library_report(void* stream, const besst_report_args* args, uint64_t* out);
int besst_ctx_library_report(besst_ctx* ctx, int64_t isize_bins, uint64_t* out_host, int64_t out_words);

/* Count-per-value histogram of a sample on the device (input to find_bimodality.split_distribution,
 * find_bimodality.py:109-132).  hist_out has n_bins entries; values >= n_bins are counted in
 * *overflow. */
int besst_ctx_value_histogram(besst_ctx* ctx, const int32_t* values, int64_t n, int64_t n_bins,
                              int64_t* hist_out, int64_t* overflow);

/* Record loop + CreateEdge + edge-table reduction (CreateGraph.py:111-211,812-871) over every record
 * pushed so far. */
int besst_ctx_build_graph(besst_ctx* ctx);

/* Sizes of the result: edge rows (distinct (node pair, fishy) keys) and link/fishy tuples. */
int besst_ctx_edge_count(besst_ctx* ctx, int64_t* n_rows, int64_t* n_tuples);

/* Edge rows sorted by key.  key = ((min_node << node_bits) | max_node) << 1 | is_fishy with
 * node = scaffold_id * 2 + (side == 'R').  For link rows: n = nr_links, sum_obs = obs,
 * sum_obs_sq = obs_sq, mask = BESST_MASK_* bits; for fishy rows n = fishy count.  first_idx is the
 * position of the row's first tuple in the emitted tuple stream (monotone in BAM order), offset the
 * start of the row's slice in the observation arrays. */
int besst_ctx_fetch_edges(besst_ctx* ctx, uint64_t* key, uint32_t* mask, uint32_t* n,
                          int64_t* sum_obs, int64_t* sum_obs_sq, uint32_t* first_idx,
                          uint32_t* offset, int32_t* node_bits);

/* Per-tuple observations grouped by edge row, BAM order inside a row: obs_lo belongs to the row's
 * min node, obs_hi to its max node; observations[i] = obs_lo[i] + obs_hi[i] (CreateGraph.py:842-862). */
int besst_ctx_fetch_observations(besst_ctx* ctx, int32_t* obs_lo, int32_t* obs_hi);
/* The same as ONE column: out[i] = obs_lo[i] + obs_hi[i], the entries of an edge's `observations` list
 * (BESST/CreateGraph.py:849,862) - summed on the device, half the bytes across PCIe.  It works on a stream and a buffer of
 * its own and is the one call of the ctx layer that may run on a second host thread while the caller's thread goes on with
 * besst_ctx_score_edges / the other fetches (the Python drop-in starts it in the background when the table has been built
 * and joins it when an edge's observations are first read, or the session closes). */
int besst_ctx_fetch_observation_sums(besst_ctx* ctx, int32_t* out);

/* cont_aligned_len numerators (CreateGraph.py:138-139), one int64 per tid. */
int besst_ctx_fetch_coverage(besst_ctx* ctx, int64_t* aligned);

int besst_ctx_fetch_counters(besst_ctx* ctx, besst_counters* out);

/* GiveScoreOnEdges, normal-distribution branch (CreateGraph.py:498-614), for n_edges rows of the
 * table built by the last besst_ctx_build_graph.  row[i] indexes the edge table; swap[i] != 0 means
 * the graph iterates the edge as (max_node, min_node), i.e. l1 comes from obs_hi; len1/len2 are the
 * scaffold lengths of the first/second endpoint in that orientation.  Outputs per edge:
 *   gap      int(gap)                      (CreateGraph.py:511-541)
 *   sd0      expected std-dev tr_sk_std_dev or 2^32 (:548-558)
 *   ks_h     integer h with KS statistic = h / n (:582-606)
 *   flags    bit0: both scaffolds > 2 sigma (ML gap used), bit1: -gap > len (score forced to 0) */
int besst_ctx_score_edges(besst_ctx* ctx, int64_t n_edges, const uint32_t* row, const uint8_t* swap,
                          const int32_t* len1, const int32_t* len2, double mean, double sigma,
                          double read_len, double* gap, double* sd0, int32_t* ks_h, uint8_t* flags);

/* GiveScoreOnEdges, log-normal branch (param.lognormal: a skewed library; CreateGraph.py:485-494,522-531,549-553).  As
 * besst_ctx_score_edges, but an edge whose scaffolds are both longer than 2 sigma gets the gap of
 * mathstats.log_normal_param_est.GapEstimator(ln_mu, ln_sigma, read_len, observations, len1, c2_len=len2) (CreateGraph.py:526;
 * un-vendored, restated in besst_amd/mathstats_compat.py): the integer d maximising
 *     L(d) = sum_i log f(o_i + d) - n log g(d),   f = log-normal pmf on 1 .. x_max,   g(d) = sum_x w(x; d) f(x)
 * over the gaps that keep every o_i + d inside the support - coarse scan with stride 64, then the 129 gaps around the
 * coarse optimum - clamped to max_gap = len(conditional_stddevs) - 1 (:527-528).  The pmf's prefix and tail tables are built on
 * the device at the first call and kept while (ln_mu, ln_sigma, x_max) stay the same.  x_max is passed in (the caller's
 * int(min(exp(ln_mu + 6 ln_sigma), 4e6))) so that host and device agree on the support.  There is no sd0 output: the
 * caller indexes the conditional sigma table (besst_ctx_conditional_stddevs) with the gap (:549-553). */
int besst_ctx_score_edges_lognormal(besst_ctx* ctx, int64_t n_edges, const uint32_t* row, const uint8_t* swap,
                                    const int32_t* len1, const int32_t* len2, double mean, double sigma,
                                    double read_len, double ln_mu, double ln_sigma, int64_t x_max, int32_t max_gap,
                                    double* gap, int32_t* ks_h, uint8_t* flags);

/* get_conditional_stddevs (CreateGraph.py:436-469): out[k] = sigma of the density f(x) * max(0, x - steps[k] + 1) over
 * x = 0 .. max_isize, where density[x] = f(x) is param.empirical_distribution laid out densely (0 where it has no entry).
 * The caller repeats out[k] for the gaps up to the next step as the reference does.  Host pointers. */
int besst_ctx_conditional_stddevs(besst_ctx* ctx, const double* density, int64_t max_isize, const int32_t* steps,
                                  int32_t n_steps, double* out);

/* ------------------------------------------------------------------------------------------------
 * BAM front-end (host): BGZF inflate + record decode into the SoA columns, replacing the
 * `pysam.Samfile(param.bamfile, 'rb')` iteration of runBESST:162 / CreateGraph.py:111 /
 * libmetrics.py:63,257,293.  qlen = query_alignment_length, rlen = query_length, alen = reference_length
 * (pysam 0.8 attribute names).  n_threads inflate workers (libdeflate if present, else zlib).
 * ---------------------------------------------------------------------------------------------- */
besst_bam* besst_bam_open(const char* path, int n_threads);
void besst_bam_close(besst_bam* bam);
int64_t besst_bam_n_references(const besst_bam* bam);
const char* besst_bam_reference_name(const besst_bam* bam, int64_t index);
/* All names at once, NUL-terminated and back to back (a header of 2 M contigs is 2 M calls otherwise): returns the bytes
 * needed; buf is filled when cap is at least that. */
int64_t besst_bam_reference_names(const besst_bam* bam, char* buf, int64_t cap);
int besst_bam_reference_lengths(const besst_bam* bam, int32_t* out);
/* Returns the number of records decoded (0 at end of file) or a negative status.  qlen is a 16-bit column: an aligned
 * query longer than 65535 bases (no paired short read is) is stored as 65535 and counted. */
int64_t besst_bam_clamped_records(const besst_bam* bam);
int64_t besst_bam_read_records(besst_bam* bam, int64_t max_records, int32_t* tid, int32_t* mtid, int32_t* pos,
                               int32_t* mpos, int32_t* tlen, uint16_t* flag, uint8_t* mapq, uint16_t* qlen,
                               int32_t* rlen, int32_t* alen);
/* Test / bench scaffolding, not part of the graph path: the columns as a BAM file in htslib's block layout (name
 * "r<index>", CIGAR [clip S] qlen M, rlen bases) - what tests and bench.py read back through the reader above.
 * level: zlib's 0..9; + 16: pseudo-random bases and slowly changing qualities (a file that compresses like a sequencer's,
 * ~3 x) instead of constant bytes (~13 x). */
int besst_bam_write_records(const char* path, int64_t n_ref, const char* const* ref_names, const int32_t* ref_lengths,
                            int64_t n, const int32_t* tid, const int32_t* mtid, const int32_t* pos, const int32_t* mpos,
                            const int32_t* tlen, const uint16_t* flag, const uint8_t* mapq, const uint16_t* qlen,
                            const int32_t* rlen, int n_threads, int level);

/* ------------------------------------------------------------------------------------------------
 * Host float finishing of libmetrics (no GPU): the statistics on the <= 1,000,000 sampled insert sizes,
 * replayed in the reference's exact operation order (libmetrics.py:22-28,88-110,141-223,316-343) so the
 * doubles are bit-identical to CPython's.  values = abs(tlen) in BAM order; is_float/offset select the
 * float form abs(tlen) + offset (offset = 2*read_len).
 * ---------------------------------------------------------------------------------------------- */
int besst_host_isize_stats(const int32_t* values, int64_t n, int32_t is_float, double offset,
                           int64_t* kept_out, int64_t* n_kept, double* stats_out /* [5] */);
int besst_host_contam_stats(const int32_t* values, int64_t n, int32_t is_float, double offset,
                            int64_t* n_final, double* stats_out /* [4] */);
int besst_host_getdistr(const int32_t* values, const int64_t* kept, int64_t n_kept, int32_t is_float,
                        double offset, const int32_t* contig_lengths, int64_t n_contigs,
                        double* adjusted_out, int64_t adjusted_cap, int64_t* n_adjusted,
                        double* out /* [26] */);

/* ------------------------------------------------------------------------------------------------
 * device-pointer API (caller owns HBM; all pointers are device pointers unless noted)
 * ---------------------------------------------------------------------------------------------- */

/* Scratch bytes needed by besst_dev_classify / besst_dev_reduce for up to n records / tuples. */
size_t besst_dev_classify_workspace_bytes(int64_t n_records);
size_t besst_dev_reduce_workspace_bytes(int64_t n_tuples);

/* Pack the contig table into the 16-byte rows the kernels gather from, followed by one class byte per
 * contig (host pointers in, device pointer out; table must hold besst_dev_contig_table_bytes(n) bytes). */
size_t besst_dev_contig_table_bytes(int64_t n_contigs);
/* dst[0, bytes) <- src[0, bytes), both on the device and 16-byte aligned, in one small launch: how a pass's state block
 * (coverage numerators | counters | carry, zero / (-1, -1) at the head of every pass: BESST/CreateGraph.py:89-99) is
 * restored from a template. */
int besst_dev_restore_state(void* stream, void* dst, const void* src, int64_t bytes);
int besst_dev_pack_contigs(void* stream, int64_t n_contigs, const int32_t* h_scaf_id,
                           const int32_t* h_scaf_len, const int32_t* h_ctg_pos,
                           const int32_t* h_ctg_len, const uint8_t* h_direction,
                           const uint8_t* h_cls, void* d_table);

/* Stage 1: per-record classification, coverage accumulation, CreateEdge semantics (duplicate
 * chain, acceptance), ordered emission of link/fishy tuples.
 *   carry   int32[2] device: counter.prev_obs1/2 entering the batch, updated on exit
 *   aligned int64[n_contigs] device, accumulated into (zero it before the first batch)
 *   keys / payload  uint64[capacity >= n] device: emitted tuples in BAM order
 *   n_out   uint32 device: number of tuples emitted by this call
 *   counters  besst_counters device struct, accumulated into
 * Columns must be 16-byte aligned. */
int besst_dev_classify(void* stream, int64_t n, const int32_t* tid, const int32_t* mtid,
                       const int32_t* pos, const int32_t* mpos, const uint16_t* flag,
                       const uint8_t* mapq, const uint16_t* qlen, int64_t n_contigs,
                       const void* contig_table, const besst_lib_params* h_params, int32_t node_bits,
                       int32_t* carry, int64_t* aligned, uint64_t* keys, uint64_t* payload,
                       uint32_t* n_out, besst_counters* counters, void* workspace,
                       size_t workspace_bytes);

/* Share of the records whose mate lies on another contig (tid != mtid) - the only records the record loop does more
 * than add coverage for (CreateGraph.py:141-206) - counted over evenly spaced 1024-record tiles covering about
 * `sample_records` records; SYNCHRONISES the stream.  *record_path = the besst_lib_params.record_path to use
 * (1 from BESST_DENSE_CANDIDATE_SHARE on).  counts_scratch: 16 bytes of device memory. */
#define BESST_DENSE_CANDIDATE_SHARE 0.05
int besst_dev_candidate_density(void* stream, int64_t n, const int32_t* tid, const int32_t* mtid,
                                int64_t sample_records, void* counts_scratch, double* h_share,
                                int32_t* h_record_path);

/* Stage 2: sort of the tuples by (key, position in the stream) - observably a stable sort by key - and segmented
 * reduction into edge rows (up to 4 M tuples: one MSD partition + per-bucket sort and reduction; beyond, up to 2^30:
 * run-grouped - every 512 consecutive tuples are grouped into runs of equal keys and the runs are sorted - or, with
 * BESST_REDUCE_NO_RUNS, chained-scan radix passes over the tuples).  *n_rows may come back as BESST_ROWS_*.
 *   n_tuples  uint32 device: number of valid tuples in keys/payload (<= capacity)
 *   key_base  a lower bound of every key (0 is always valid).  Scaffold ids keep growing across passes
 *             (param.scaffold_indexer, MakeScaffolds.py:276), so from the second library on all keys share a long
 *             common prefix; with key_base = ((2 * min scaffold id) << node_bits) << 1 the sort works on key - key_base
 *   key_bits  number of significant bits of key - key_base (2 * node_bits + 1 with key_base 0)
 * Payload: obs1 >= 0 in the low 32 bits, obs2 in bits 32..61 (30 bits), the graph mask in the top 2 (a row's mask is
 *   its first tuple's).  obs1 + obs2 is formed in 32 bits and must stay below 2^32; the tuples the record loop emits
 *   have obs1 + obs2 < 2^30 (ins_size_threshold is refused from 2^30 on).  Squares and a row's sums are 64-bit: sum obs
 *   and sum obs^2 are exact while they fit 63 bits (row_sum / row_sum_sq are int64).
 * Outputs (capacity entries each): row_* arrays, obs_lo/obs_hi grouped by row, n_rows (uint32). */
int besst_dev_reduce(void* stream, int64_t capacity, const uint32_t* n_tuples, int32_t key_bits,
                     const uint64_t* keys, const uint64_t* payload, uint64_t* row_key,
                     uint32_t* row_mask, uint32_t* row_n, int64_t* row_sum, int64_t* row_sum_sq,
                     uint32_t* row_first, uint32_t* row_offset, int32_t* obs_lo, int32_t* obs_hi,
                     uint32_t* n_rows, void* workspace, size_t workspace_bytes, const uint32_t* first_map,
                     uint64_t key_base);
/* the same with BESST_REDUCE_* flags (besst_dev_reduce passes 0) */
int besst_dev_reduce_flags(void* stream, int64_t capacity, const uint32_t* n_tuples, int32_t key_bits,
                           const uint64_t* keys, const uint64_t* payload, uint64_t* row_key,
                           uint32_t* row_mask, uint32_t* row_n, int64_t* row_sum, int64_t* row_sum_sq,
                           uint32_t* row_first, uint32_t* row_offset, int32_t* obs_lo, int32_t* obs_hi,
                           uint32_t* n_rows, void* workspace, size_t workspace_bytes, const uint32_t* first_map,
                           uint64_t key_base, uint32_t flags);

/* A test and diagnosis accessor, not part of a graph build: what besst_dev_reduce_flags with this capacity / key_bits /
 * flags selects, and what the last such call left in `workspace`.  SYNCHRONISES the stream, copies the bucket tables
 * out of the workspace and counts on the host; launches no kernel.  h_out: 8 host words.
 *   h_out[0]  the form: 0 = MSD partition + buckets, 1 = run-grouped, 2 = chained scan + buckets,
 *             3 = chained scan + tile reduction (the launcher's own tests, not a copy of them)
 *   form 2:   h_out[1..5] = top-16-bit buckets that were empty / finished by the wave kernel / by the wave kernel's digit
 *             passes / by a workgroup in LDS (<= 4096 words) / by a workgroup in global memory
 *   form 0:   h_out[1..4] = 11-bit buckets of <= 1, 2..256, 257..4096 and > 4096 words (an empty stream partitions
 *             nothing: the counts are then those of the call before)
 *   other forms and the remaining words: 0 */
int besst_dev_reduce_census(void* stream, int64_t capacity, int32_t key_bits, uint32_t flags, const void* workspace,
                            size_t workspace_bytes, int64_t* h_out);

/* Stage 1 + 2 on buffers that stay allocated (a resident builder): the large-stream form of stage 2 starts with a
 * histogram read of the whole key stream, which stage 1 can take on its way out (it has every key in registers when it
 * writes the ordered stream).  besst_dev_reduce_presort describes that hand-over for a given stage-2 call: it returns
 * 1 and fills *out when besst_dev_reduce with this capacity / key_bits / key_base / workspace would take its
 * histograms from `out->table` (a region of that workspace), 0 when it would not (small streams, keys that do not
 * pack).  besst_dev_classify_presort is besst_dev_classify that also fills the table (presort may be NULL);
 * besst_dev_reduce_presorted is besst_dev_reduce that trusts it (h_presort: the structure that classify call filled in;
 * keys may be NULL when it says `segmented`) - same workspace, same capacity, same key range, and the tuples of
 * exactly that classify call.  (Replaces nothing in the reference: it is the seam between
 * CreateGraph.py:141-206, where links are found, and :842-862, where they are summed per edge.) */
typedef struct besst_presort {
    uint32_t* table;      /* device: [rows][2][256] counters inside the stage-2 workspace */
    int32_t rows;         /* power of two */
    int32_t shift;        /* digits of key - key_base at shift and shift + 8 */
    uint64_t key_base;
    uint32_t capacity;    /* tuples at or beyond it are not counted (stage 2 ignores them too) */
    uint32_t flags;       /* in, read by besst_dev_reduce_presorted: BESST_REDUCE_* */
    /* The tuple stream itself can be handed over as the record loop leaves it - one segment per 16 384-record block,
     * ordered by the block offsets of the stitch - when stage 2's first stream pass can read it that way:
     * besst_dev_reduce_presort sets `segmented` to say so, besst_dev_classify_presort leaves it 1 (and fills the seg_*
     * fields) when it did NOT write the dense keys / payload, and besst_dev_reduce_presorted then reads the segments and -
     * in_record_loop 1 only - writes the dense payload (the `payload` argument of both calls) itself.  With in_record_loop 2
     * or 3 NEITHER dense column exists after the pass: stage 2 works on the segments and writes the row columns and the
     * observations only; `keys` / `payload` keep whatever an earlier pass left there (a caller that wants the dense tuple
     * stream classifies with BESST_REDUCE_NO_RUNS in `flags`, or without a presort).  in_record_loop (out): 1 = the record loop
     * counted the digits while it emitted; 2 = it handed its segments over without counting, because `flags` did not carry
     * BESST_REDUCE_NO_RUNS and stage 2 then groups runs and reads no histogram; 3 = as 2, and the record loop grouped the
     * runs of equal keys itself while it emitted: the key segments then hold run tables and a run byte per tuple instead
     * of keys (seg_run_* below), and stage 2 only sorts the list of runs and places the observations.  After 2 or 3 a
     * repeat of besst_dev_reduce_presorted WITH that flag (after BESST_ROWS_RUN_OVERFLOW) needs a repeat of the classify
     * call with it first. */
    int32_t segmented;
    int32_t in_record_loop;
    const uint64_t* seg_keys;
    const uint64_t* seg_payload;
    const uint32_t* seg_offsets;
    const uint32_t* seg_skip;
    uint32_t seg_blocks;
    uint32_t seg_tile;
    uint64_t* payload_out;
    const uint32_t* seg_chunk_first; /* per 512 positions of the ordered stream: the block the first of them lies in */
    /* in_record_loop == 3 only (else NULL / 0): per block the place of its first run in the stream-ordered run list, the
     * record loop's block summaries (planes of seg_summ_stride words) and the word that says a block's run tables overflowed */
    const uint32_t* seg_run_offsets;
    const uint32_t* seg_summ;
    uint32_t seg_summ_stride;
    const uint32_t* seg_run_status;
} besst_presort;
int besst_dev_reduce_presort(int64_t capacity, int32_t key_bits, uint64_t key_base, void* workspace,
                             size_t workspace_bytes, besst_presort* h_out);
int besst_dev_classify_presort(void* stream, int64_t n, const int32_t* tid, const int32_t* mtid,
                               const int32_t* pos, const int32_t* mpos, const uint16_t* flag,
                               const uint8_t* mapq, const uint16_t* qlen, int64_t n_contigs,
                               const void* contig_table, const besst_lib_params* h_params, int32_t node_bits,
                               int32_t* carry, int64_t* aligned, uint64_t* keys, uint64_t* payload,
                               uint32_t* n_out, besst_counters* counters, void* workspace,
                               size_t workspace_bytes, besst_presort* h_presort);
int besst_dev_reduce_presorted(void* stream, int64_t capacity, const uint32_t* n_tuples, int32_t key_bits,
                               const uint64_t* keys, const uint64_t* payload, uint64_t* row_key,
                               uint32_t* row_mask, uint32_t* row_n, int64_t* row_sum, int64_t* row_sum_sq,
                               uint32_t* row_first, uint32_t* row_offset, int32_t* obs_lo, int32_t* obs_hi,
                               uint32_t* n_rows, void* workspace, size_t workspace_bytes,
                               const uint32_t* first_map, uint64_t key_base, const besst_presort* h_presort);

/* ---- multi-GPU path ----------------------------------------------------
 * Ranks own contiguous slices of the (tid,pos)-sorted stream.  The duplicate chain of CreateEdge
 * (CreateGraph.py:835-838,869-870) crosses slice boundaries, so stage 1 is split in three phases:
 *   scan  - the per-record kernel on the local slice (independent of the incoming prev_obs)
 *   tail  - {has, obs1, obs2, 0} of the slice's last record that reached CreateEdge  -> all_gather
 *   emit  - resolve block/slice heads against the true incoming prev_obs and write the ordered tuples
 * besst_dev_classify_emit picks the incoming prev_obs of `rank` from the gathered tails (world x 4 int32; pass
 * NULL for a single slice) - the tail of the nearest earlier rank that has one, else what `carry` holds, i.e. the
 * prev_obs entering rank 0; besst_dev_resolve_carry does only that step.
 * Then tuples are stably partitioned by owner rank (besst_owner_of_scaffold of the key's min scaffold)
 * into `world` fixed-capacity regions for ONE equal-split all-to-all; besst_dev_unpack rebuilds an
 * ordered stream on the receiver with a global emit index per tuple (first_map of besst_dev_reduce)
 * and raises *overflow if any region was truncated (retry with a larger pair_capacity). */
int besst_dev_classify_scan(void* stream, int64_t n, const int32_t* tid, const int32_t* mtid,
                            const int32_t* pos, const int32_t* mpos, const uint16_t* flag,
                            const uint8_t* mapq, const uint16_t* qlen, int64_t n_contigs,
                            const void* contig_table, const besst_lib_params* h_params, int32_t node_bits,
                            int64_t* aligned, besst_counters* counters, void* workspace,
                            size_t workspace_bytes);
int besst_dev_classify_tail(void* stream, int64_t n, int32_t* tail, void* workspace, size_t workspace_bytes);
int besst_dev_resolve_carry(void* stream, const int32_t* tails, int32_t rank, int32_t* carry);
int besst_dev_classify_emit(void* stream, int64_t n, int32_t detect_duplicate, int32_t* carry, uint64_t* keys,
                            uint64_t* payload, uint32_t* n_out, besst_counters* counters, void* workspace,
                            size_t workspace_bytes, int64_t n_contigs, const void* contig_table,
                            int64_t* aligned, const int32_t* tails, int32_t rank, int32_t* slice_info);
/* out[i] = d + sigma^2 g'(d) / g(d) at d = d_lower + i, i < n, for two contigs of length contig_len: the left-hand side of
 * the GapEst ML condition over a run of gaps.  mathstats' PreCalcMLvaluesOfdLongContigs (MakeScaffolds.py:68) rounds
 * these values and inverts the map into its {observation -> gap} table; besst_amd/mathstats_compat.py does that on the
 * host from this array.  _dev: device pointer out, nothing synchronised; _ctx: host pointer out. */
int besst_dev_gap_condition_table(void* stream, double mean, double sigma, double read_len, double contig_len,
                                  int32_t d_lower, int32_t n, double* out);
int besst_ctx_gap_condition_table(besst_ctx* ctx, double mean, double sigma, double read_len, double contig_len,
                                  int32_t d_lower, int32_t n, double* h_out);

/* Per-edge scoring on caller-owned device buffers (the device-pointer form of besst_ctx_score_edges;
 * CreateGraph.py:498-614): ML gap by bisection, expected sigma, KS numerator h = max|#{l1 <= x} - #{l2 <= x}| on the
 * centred per-end observations.  In the sharded build every rank scores the rows it owns.
 *   row / swap / len1 / len2   one entry per scored edge (device): row index into the edge table, whether the
 *                              edge's first scaffold is the key's max node, the two scaffold lengths
 *   row_n .. obs_hi            the edge table of besst_dev_reduce
 *   workspace                  [ uint64 big_off[n_edges] | int32 scratch ]: big_off[e] = start (in ints) of edge e's
 *                              2 * next_pow2(n) scratch ints when next_pow2(n) > 8192, else ignored; the scratch
 *                              part follows at the next 256-byte boundary after the offsets */
int besst_dev_score_edges(void* stream, int64_t n_edges, const uint32_t* row, const uint8_t* swap,
                          const int32_t* len1, const int32_t* len2, const uint32_t* row_n,
                          const int64_t* row_sum, const uint32_t* row_offset, const int32_t* obs_lo,
                          const int32_t* obs_hi, double mean, double sigma, double read_len, double* gap,
                          double* sd0, int32_t* ks_h, uint8_t* flags, void* workspace, size_t workspace_bytes);

/* The mate-elsewhere bit column of a resident record stream (part of the record layout, made once when the records arrive:
 * by the ingest, by whoever uploads columns): bits[i / 8] bit i % 8 = (tid[i] != mtid[i]), besst_dev_mate_bits_bytes(n)
 * bytes.  Passed to the record loop in besst_lib_params.mate_bits. */
size_t besst_dev_mate_bits_bytes(int64_t n_records);
int besst_dev_mate_bits(void* stream, int64_t n_records, const int32_t* tid, const int32_t* mtid, void* bits);
/* Both bit columns of the layout in the one pass over `tid` and `mtid`: mate_bits as above, and the run bits
 * tid_bits[i / 8] bit i % 8 = (i == 0 || tid[i] != tid[i - 1]), same size (besst_dev_mate_bits_bytes), bits behind the last
 * record 0.  Passed to the record loop in besst_lib_params.mate_bits / .tid_bits. */
int besst_dev_record_bits(void* stream, int64_t n_records, const int32_t* tid, const int32_t* mtid, void* mate_bits,
                          void* tid_bits);
/* The candidate side stream (besst_cand_stream above), made in two calls because its size depends on the records:
 *   1. besst_dev_candidate_offsets: the set plane (besst_dev_mate_bits_bytes(n) bytes, 16-byte aligned) and the entry
 *      offsets (besst_dev_candidate_offsets_bytes(n) bytes); where mate_bits / tid_bits are not NULL it also writes the two
 *      planes of besst_dev_record_bits from the same read of `tid` / `mtid` (both or neither).  Two launches: a count per
 *      16384-record block and a scan of the counts.
 *   2. read n_entries = offsets[n_blocks] (a device word; synchronise the stream first), allocate
 *      besst_dev_candidate_stream_bytes(n_entries) bytes, and
 *   3. besst_dev_candidate_stream: the ordered write of the entries into `entries` (one launch; no workgroup waits for
 *      another in any of the three) and the host-side descriptor *out, whose column pointers lie inside `entries`.
 * The descriptor goes to the record loop in besst_lib_params.cand_stream; it, set_bits, offsets and entries must stay
 * alive and unchanged while it is in use. */
size_t besst_dev_candidate_offsets_bytes(int64_t n_records);
size_t besst_dev_candidate_stream_bytes(int64_t n_entries);
int besst_dev_candidate_offsets(void* stream, int64_t n_records, int64_t n_refs, const int32_t* tid, const int32_t* mtid,
                                const uint16_t* flag, void* set_bits, void* offsets, void* mate_bits, void* tid_bits);
int besst_dev_candidate_stream(void* stream, int64_t n_records, int64_t n_refs, const int32_t* tid, const int32_t* mtid,
                               const int32_t* pos, const int32_t* mpos, const uint16_t* flag, const uint8_t* mapq,
                               const uint16_t* qlen, const void* set_bits, const void* offsets, int64_t n_entries,
                               void* entries, size_t entries_bytes, besst_cand_stream* out);
/* Which form of the record loop the last besst_dev_classify* / besst_ctx_build_graph call of this process launched:
 * -1 none yet or record_path 0; record_path 1: 0 = it read every column, 1 = with mate_bits, 2 = with tid_bits as well,
 * 3 = with the candidate side stream.  (Tests and tools; results do not depend on the form.)  ONE word per process,
 * written by every call: with two contexts or streams classifying at the same time it names whichever call came last -
 * read it only where one thread of the process classifies. */
int besst_dev_record_loop_form(void);

/* The log-normal branch on caller-owned device buffers (device-pointer forms of besst_ctx_score_edges_lognormal and
 * besst_ctx_conditional_stddevs).
 *   besst_dev_lognormal_tables   F0[k] = sum_{x <= k} f(x), F1[k] = sum_{x <= k} x f(x) for k = 0 .. x_max (x_max + 1
 *                                doubles each), f the pmf of LogNormal(mu, sigma) on the integers; workspace:
 *                                besst_dev_lognormal_tables_workspace_bytes(x_max)
 *   besst_dev_score_edges_lognormal   workspace as for besst_dev_score_edges plus, at its end, 2 x [8 bytes x (x_max + 1),
 *                                rounded up to 256] + besst_dev_lognormal_tables_workspace_bytes(x_max) (the tail sums
 *                                of the pmf above its median, built there on every call: a segment of the upper tail
 *                                is not taken as a difference of two prefix sums near the total mass) and one more
 *                                [8 bytes x n_edges, rounded up to 256] */
size_t besst_dev_lognormal_tables_workspace_bytes(int64_t x_max);
int besst_dev_lognormal_tables(void* stream, double mu, double sigma, int64_t x_max, double* F0, double* F1,
                               void* workspace, size_t workspace_bytes);
int besst_dev_score_edges_lognormal(void* stream, int64_t n_edges, const uint32_t* row, const uint8_t* swap,
                                    const int32_t* len1, const int32_t* len2, const uint32_t* row_n,
                                    const int64_t* row_sum, const uint32_t* row_offset, const int32_t* obs_lo,
                                    const int32_t* obs_hi, double mean, double sigma, double read_len, double ln_mu,
                                    double ln_sigma, int64_t x_max, const double* F0, const double* F1, int32_t max_gap,
                                    double* gap, int32_t* ks_h, uint8_t* flags, void* workspace, size_t workspace_bytes);
int besst_dev_conditional_stddevs(void* stream, const double* density, int64_t max_isize, const int32_t* steps,
                                  int32_t n_steps, double* out);

/* libmetrics sampling on caller-owned device columns (the device-pointer form of besst_ctx_metrics_sample;
 * libmetrics.py:63-84,293-303).  `state` is 6 x int64 on the device, in/out:
 *   [0] records so far that qualify for the insert-size sample   (is_proper_aligned_unique_innie/outie on a top contig)
 *   [1] records so far on a top contig                            (the contamination scan's sample_counter)
 *   [2] contamination observations so far
 *   [3] counter_total, [4] n_contam - both only over records inside the first-1,000,000 cut-off, [5] records scanned
 * A record's sample slot is its running count, so a slice of the stream whose state[0..2] was preset to the
 * counts of the slices before it writes exactly its share of the two 1,000,000-entry sample buffers (everything
 * else stays untouched): with zeroed buffers, an all-reduce(sum) over the slices' buffers is the ordered sample
 * of the whole stream.  count_only != 0 advances state[0..2] only (first phase of a sharded scan) and
 * leaves them exact; the sampling form leaves [0..2] exact up to the cut-offs and at least 1,000,000 beyond them (the
 * call works in parts of 64 Mi records and does not look at a part that begins with both samples full).
 * n is limited to 2^36 records per call (a C5 library is 2.67 x 10^9); workspace: besst_dev_metrics_workspace_bytes(n) - the tile counts and, for
 * min(n, 64 Mi) records, 8 bytes of sample staging per record. */
size_t besst_dev_metrics_workspace_bytes(int64_t n_records);
int besst_dev_metrics_sample(void* stream, int64_t n, const int32_t* tid, const int32_t* mtid,
                             const int32_t* tlen, const uint16_t* flag, const uint8_t* mapq,
                             int64_t n_contigs, const uint8_t* top_mask, int32_t orientation,
                             int32_t min_mapq, double read_len, int32_t count_only, int32_t* isize_out,
                             int32_t* contam_out, int64_t* state, void* workspace, size_t workspace_bytes);
size_t besst_dev_exchange_region_bytes(int64_t pair_capacity);
/* Speculative slice heads (the sharded build's default, no tail exchange): besst_dev_classify_emit with
 * `slice_info` (8 x int32, device) instead of `tails` leaves the slice's first record that reaches CreateEdge
 * unresolved and fills slice_info = { any reaching record, tail obs1, tail obs2, head present, head obs1, head obs2,
 * head flags (1 accept, 2 double call, 4 mapq 0, 8 tuple emitted), position of the head's tuple or -1 };
 * besst_dev_partition(..., slice_info) copies it into words 4..11 of every region header and records where the head's
 * tuple went (words 12, 13); besst_dev_unpack(..., speculative_heads = 1, rank, detect_duplicate, all_slice_info,
 * counters) replays the chain over the sources (CreateGraph.py:835-870), corrects the summed counters, drops a
 * duplicate head's tuple at its owner and shifts the global emit indexes; all_slice_info (world x 8, device, may be
 * null) receives every source's description.
 * A region may be followed by a RIDER: `rider_bytes` (multiple of 8) of 64-bit words that every source copies behind
 * the tuples of each of its regions (besst_dev_partition) and every receiver sums over its sources
 * (besst_dev_unpack, written to `rider_sum`).  The sharded build sends the coverage numerators and counters of
 * small assemblies this way instead of all-reducing them: one collective less per step.  The exchange
 * then moves besst_dev_exchange_stride_bytes(pair_capacity, rider_bytes) bytes per (source, destination) pair;
 * rider_bytes = 0: no rider, stride = region. */
size_t besst_dev_exchange_stride_bytes(int64_t pair_capacity, int64_t rider_bytes);
uint32_t besst_owner_of_scaffold(uint32_t scaffold_id, uint32_t world);
/* What the two calls define, word by word (tests/exchange_design.py holds both against a byte-for-byte model):
 *   besst_dev_partition writes, per region, header words 0..3 = { tuples sent = min(wanted, pair_capacity), tuples
 *   wanted, min(*n_tuples, capacity), 0 }, words 4..11 ONLY where slice_info is given, words 12 and 13 ONLY where
 *   slice_info[7] names a tuple of the stream (0 <= slice_info[7] < min(*n_tuples, capacity); 13 may be at or beyond
 *   pair_capacity when the owner's region overflowed), the first `sent` entries of the three columns and the rider.
 *   Words 14 and 15, words 4..13 in the other cases and the column slots behind `sent` keep whatever the buffer held.
 *   besst_dev_unpack writes keys / payload / gidx up to *n_out and nothing behind it; it only ever SETS *overflow (the
 *   caller clears it before the call); with speculative heads the counter corrections are added to `counters` when
 *   rider_bytes is 0 and to the last eight words of rider_sum otherwise (`counters` is then left alone, but must still be
 *   given; rider_bytes 8..56 is refused); all_slice_info is written only with speculative heads.
 *   Both return an error before any launch for a world outside [1, 256], a pair_capacity that is not positive (partition:
 *   and even), a rider that is not a multiple of 8 bytes, and - unpack, speculative heads - a rank outside the world. */
/* workspace: besst_dev_reduce_workspace_bytes(capacity) */
int besst_dev_partition(void* stream, int64_t capacity, const uint32_t* n_tuples, int32_t node_bits,
                        int32_t world, const uint64_t* keys, const uint64_t* payload, int64_t pair_capacity,
                        void* send_buffer, void* workspace, size_t workspace_bytes, const void* rider,
                        int64_t rider_bytes, const int32_t* slice_info);
int besst_dev_unpack(void* stream, int32_t world, int64_t pair_capacity, const void* recv_buffer, uint64_t* keys,
                     uint64_t* payload, uint32_t* gidx, uint32_t* n_out, uint32_t* overflow, void* rider_sum,
                     int64_t rider_bytes, int32_t speculative_heads, int32_t rank, int32_t detect_duplicate,
                     int32_t* all_slice_info, besst_counters* counters);

/* ---- Scaffold-graph linearisation on the scored edge table -----------------------------------
 * Steps 1-4 of MakeScaffolds.Algorithm (MakeScaffolds.py:75-82) in one call:
 *   step 1/3  RemoveIsolatedContigs            (MakeScaffolds.py:134-144)
 *   step 2    RemoveAmbiguousRegionsUsingScore (MakeScaffolds.py:206-241) with remove_edges (:156-204)
 *   step 4    RemoveLoops                      (MakeScaffolds.py:248-274)
 * Nodes are compact ids: scaffold k has the nodes 2k ('L') and 2k+1 ('R').
 *   steps            mask of the steps to run: 1 = step 1, 2 = step 2, 4 = step 3, 8 = step 4 (15 = all, in the order of
 *                    MakeScaffolds.Algorithm).  Without step 2 every edge counts as a link edge whatever its score;
 *                    step 4 then requires at most one link edge per node (BESST_ERR_STATE otherwise)
 *   a, b, score      the link edges of G that carry a score, in G.edges() order (a = edge[0], b = edge[1]); the
 *                    order decides ties between equal scores exactly as Python's stable sort does (:216-217)
 *   edge_alive       out, n_edges: 1 = the edge survives step 2
 *   scaffold_removed_by  out, n_scaffolds: 0 = the scaffold survives; 1 / 3 / 4 = the step that removed it
 *   node_ambivalent  out, 2 * n_scaffolds: 1 = the node printed 'SCORES AMBVIVALENT' (:183); node_top / node_second
 *                    hold the two scores it printed, node_best_edge the edge of the node's first visit (events are
 *                    replayed in visiting order by sorting on (score desc, node_best_edge asc, is-edge[1]))
 *   counters         out, HOST array of 8: [0] scaffolds removed by step 1, [1] by step 3, [2] cycles found by
 *                    step 4, [3] ambivalent nodes, [4] rounds step 2 took
 * besst_linearize takes host pointers (copies in, runs, copies out, like the besst_ctx_* calls);
 * besst_dev_linearize takes device pointers for everything but `counters` and synchronises the stream. */
int besst_linearize(int device, int32_t steps, int64_t n_scaffolds, int64_t n_edges, const int32_t* a, const int32_t* b,
                    const double* score, uint8_t* edge_alive, uint8_t* scaffold_removed_by,
                    uint8_t* node_ambivalent, double* node_top, double* node_second,
                    uint32_t* node_best_edge, int64_t* counters);
size_t besst_dev_linearize_workspace_bytes(int64_t n_scaffolds, int64_t n_edges);
int besst_dev_linearize(void* stream, int32_t steps, int64_t n_scaffolds, int64_t n_edges, const int32_t* a, const int32_t* b,
                        const double* score, void* workspace, size_t workspace_bytes, uint8_t* edge_alive,
                        uint8_t* scaffold_removed_by, uint8_t* node_ambivalent, double* node_top,
                        double* node_second, uint32_t* node_best_edge, int64_t* counters);

/* ---- chain extraction of the linearised scaffold graph (the rest of SURVEY 8(f) rank 3) ----------------------------
 * The data-parallel part of MakeScaffolds.NewContigsScaffolds / UpdateInfo (MakeScaffolds.py:270-341, 344-482): after
 * steps 1-4 every scaffold end has at most one link edge, i.e. the graph is a set of paths, and the reference walks each
 * path from one end.  Nodes: 2 * scaffold + (side == 'R'), scaffolds numbered in node order.
 *   link[2n]             the node at the other end of a node's link edge, -1 without one
 *   gap[2n]              the gap the walk adds when it crosses that edge (max(1, int(avg_gap)), MakeScaffolds.py:468-471)
 *   scaffold_length[n]   s_length of every scaffold;  node_order[2n]  position of every node in G.nodes()
 * Out, per node h (walking OUT of the scaffold through end h):
 *   terminal[2n]         the end of the path on that side (h itself when h has no link)
 *   beyond[2n]           lengths of the scaffolds beyond h on that side + the gaps in between (int64)
 *   lowest_order[2n]     smallest node_order among the nodes beyond h (INT32_MAX when there are none)
 * The host mirror (besst_amd/MakeScaffolds.py) turns these into the reference's Scaffolds / Contigs state.
 * besst_chain_scaffolds takes host pointers; besst_dev_chain_scaffolds device pointers (it synchronises the stream
 * between its doubling passes to find out when nothing moves any more); *passes = doubling passes run. */
size_t besst_dev_chain_workspace_bytes(int64_t n_scaffolds);
int besst_dev_chain_scaffolds(void* stream, int64_t n_scaffolds, const int32_t* link, const int32_t* gap,
                              const int32_t* scaffold_length, const int32_t* node_order, void* workspace,
                              size_t workspace_bytes, int32_t* terminal, int64_t* beyond, int32_t* lowest_order,
                              int32_t* h_passes);
int besst_chain_scaffolds(int device, int64_t n_scaffolds, const int32_t* link, const int32_t* gap,
                          const int32_t* scaffold_length, const int32_t* node_order, int32_t* terminal, int64_t* beyond,
                          int32_t* lowest_order, int32_t* passes);

/* ---- ScorePaths on the link graph -------------------------------------------------------------
 * Connectivity weights of a batch of candidate paths: calculate_connectivity / calculate_connectivity_contamination
 * of ScorePaths (ExtendLargeScaffolds.py:29-130); the path search itself stays on the host.
 *   n_nodes, row_ptr, col, weight   CSR of the LINK edges of the graph in both directions (node = 2 * scaffold +
 *                                   (side == 'R'); weight = nr_links); row_ptr has n_nodes + 1 entries
 *   n_paths, path_ptr, path_nodes   CSR of the paths (lists of nodes), path_ptr has n_paths + 1 entries
 *   contamination                   0: calculate_connectivity (:33-69), 1: the contamination variant (:72-105)
 *   good, bad                       out, n_paths: good_link_weight (BEFORE the division by two of :94) and
 *                                   bad_link_weight; score = good / float(bad) is formed by the caller (:63-67)
 * besst_score_paths takes host pointers; besst_dev_score_paths device pointers and only enqueues on `stream`. */
int besst_score_paths(int device, int64_t n_nodes, const int64_t* row_ptr, const int32_t* col,
                      const int32_t* weight, int64_t n_paths, const int64_t* path_ptr, const int32_t* path_nodes,
                      int32_t contamination, int64_t* good, int64_t* bad);
int besst_dev_score_paths(void* stream, int64_t n_nodes, const int64_t* row_ptr, const int32_t* col,
                          const int32_t* weight, int64_t n_paths, const int64_t* path_ptr,
                          const int32_t* path_nodes, int32_t contamination, int64_t* good, int64_t* bad);

/* ---- scaffold output: the sequence work of GenerateOutput.PrintOutput (GenerateOutput.py:88-234) ---------------------
 * The contigs of a run lie end to end in one byte pool (one byte per base, as read: case and IUPAC codes survive);
 * contig i is pool[ctg_off[i] .. ctg_off[i] + ctg_len[i]).  Device pools (besst_dev_*) must have BESST_EMIT_PAD readable
 * bytes before `pool` and after pool + pool_bytes, and so must `literals`: the kernels read whole aligned dwords around
 * the bytes they need.  The host-pointer twins add the pads themselves.
 *
 * besst_*_seq_overlaps: check_kmer_overlap (:110-116) for n junctions.  Junction c joins contig left[c] to contig
 * right[c]; forward[c] bit 0 / bit 1: the left / right contig is written as stored (else reverse-complemented).
 *   overlap[c]   the largest i >= 1 for which the last i bytes of the last max_overlap bytes of the oriented left contig
 *                equal the first i bytes of the first max_overlap bytes of the oriented right one, else 0 (bytes
 *                compare as bytes; a window shorter than max_overlap is the whole contig); -1 for a junction whose
 *                contig indices or pool range are invalid (device layer; the host layer refuses those up front)
 *   err[0]       min over the junctions whose reversed RIGHT window holds a byte without a complement of
 *                (c << 32 | position of that byte in the oriented window); the caller sets it to all ones
 * max_overlap: 0..BESST_MAX_CONTIG_OVERLAP.
 *
 * besst_*_emit_scaffolds: bytes [begin, end) of the output, written to out[0 .. end - begin).  Piece p supplies the output
 * bytes [out_off[p], out_off[p + 1]) (out_off: n_pieces + 1 entries, the exclusive prefix sum of len, out_off[0] = 0):
 *   BESST_PIECE_COPY     pool[src_off .. src_off + len)
 *   BESST_PIECE_REVCOMP  the same bytes reverse-complemented (the table of GenerateOutput.rev_nuc)
 *   BESST_PIECE_FILL_N   len times 'N' (src_off unused)
 *   BESST_PIECE_LITERAL  literals[src_off .. src_off + len): headers, '\n', 'n'
 *   err[0]       min over the REVCOMP bytes without a complement of (p << 32 | position in the piece's output); the
 *                reference raises KeyError there.  The call completes; such bytes come out as 0.
 *   err[1]       min p of the rows that point outside their pool (device layer; their bytes come out as '?')
 * The caller sets both words to all ones before the first range.  `out` of the device form is 16-byte aligned.
 * besst_host_complement_table: the 256-entry complement table, 0 = no complement. */
#define BESST_MAX_CONTIG_OVERLAP 4096
#define BESST_EMIT_PAD 32
#define BESST_PIECE_COPY 0
#define BESST_PIECE_REVCOMP 1
#define BESST_PIECE_FILL_N 2
#define BESST_PIECE_LITERAL 3
const uint8_t* besst_host_complement_table(void);
int besst_dev_seq_overlaps(void* stream, const uint8_t* pool, int64_t pool_bytes, int64_t n_contigs,
                           const int64_t* ctg_off, const int32_t* ctg_len, int64_t n, const int32_t* left,
                           const int32_t* right, const uint8_t* forward, int32_t max_overlap, int32_t* overlap,
                           uint64_t* err);
int besst_host_seq_overlaps(int device, const uint8_t* pool, int64_t pool_bytes, int64_t n_contigs, const int64_t* ctg_off,
                            const int32_t* ctg_len, int64_t n, const int32_t* left, const int32_t* right,
                            const uint8_t* forward, int32_t max_overlap, int32_t* overlap, uint64_t* err);
int besst_dev_emit_scaffolds(void* stream, const uint8_t* pool, int64_t pool_bytes, const uint8_t* literals,
                             int64_t literal_bytes, int64_t n_pieces, const int64_t* src_off, const int64_t* len,
                             const uint8_t* mode, const int64_t* out_off, int64_t begin, int64_t end, uint8_t* out,
                             uint64_t* err);
int besst_host_emit_scaffolds(int device, const uint8_t* pool, int64_t pool_bytes, const uint8_t* literals,
                              int64_t literal_bytes, int64_t n_pieces, const int64_t* src_off, const int64_t* len,
                              const uint8_t* mode, const int64_t* out_off, int64_t begin, int64_t end, uint8_t* out,
                              uint64_t* err);

/* ---- the contig FASTA -> the sequence pool above: ReadInContigseqs (runBESST:45-74) on the bytes of the file ----------
 * `text`: the whole file in HBM, 16-byte aligned, with BESST_EMIT_PAD readable bytes behind its end.  '\n' and '\r' each
 * end a line.  A line whose first byte is '>' is a header; its name is the first whitespace-delimited token behind the
 * '>'.  Every other line is stripped of leading and trailing whitespace (bytes 9-13 and 28-32; interior whitespace
 * stays) and appended to the current contig.  Text in front of the first header belongs to the first contig; a file
 * without a header is one contig with an empty name.  Rows are in file order, names may repeat.
 *
 * tile_bytes: the text is parsed in tiles of that many bytes; 0 = 16384, else a multiple of 1024 in 1024..65536 (the
 * same value in all three calls).
 *   besst_dev_fasta_workspace_bytes   scratch for a text of that size; 0: tile_bytes not accepted
 *   besst_dev_fasta_scan              leaves in info[0..BESST_FASTA_INFO_WORDS): [0] n_contigs, [1] pool_bytes,
 *                                     [2] names_bytes, [3] first_error: the smallest file offset of a byte >= 0x80 or of
 *                                     the '>' of a header without a name (all ones: none), [4] set by _pack, [5] header
 *                                     lines.  The workspace carries the tile offsets on to _pack.
 *   besst_dev_fasta_pack              n_contigs, pool_bytes, names_bytes as the scan left them.  pool (16-byte aligned,
 *                                     padded as above) receives the sequences end to end, ctg_off[n_contigs] /
 *                                     ctg_len[n_contigs] their place, names the names end to end,
 *                                     name_off[n_contigs + 1] theirs.  info[4]: the first row of 2^31 bases or more (all
 *                                     ones: none; its ctg_len is 0).
 * Like every besst_dev_* call: device memory and stream are the caller's, work is only enqueued. */
#define BESST_FASTA_INFO_WORDS 6
size_t besst_dev_fasta_workspace_bytes(int64_t text_bytes, int64_t tile_bytes);
int besst_dev_fasta_scan(void* stream, const uint8_t* text, int64_t text_bytes, int64_t tile_bytes, void* workspace,
                         size_t workspace_bytes, int64_t* info);
int besst_dev_fasta_pack(void* stream, const uint8_t* text, int64_t text_bytes, int64_t tile_bytes, const void* workspace,
                         size_t workspace_bytes, int64_t* info, int64_t n_contigs, int64_t pool_bytes,
                         int64_t names_bytes, uint8_t* pool, int64_t* ctg_off, int32_t* ctg_len, uint8_t* names,
                         int64_t* name_off);

/* ---- the text of the output stage: info-pass<n>.agp / .gff (GenerateOutput.py:156-195, 208-221) and the wrapped FASTA of
 * repeats.fa / low_coverage_contigs.fa (:47-53, 68-74), formatted on the device ------------------------------------------
 * besst_text_columns: the contigs of all scaffolds in output order (scaffolds as reversed(F), each sorted by position).
 * Contig i lies at pos[i] with len[i] bases, is written as stored where forward[i] is not 0, belongs to scaffold
 * scaffold[i] (0-based ordinal; the file says ordinal + 1), whose first contig is scaffold_start[ordinal], and is named
 * names[name_off[row[i]] .. name_off[row[i] + 1]) (name_off: n_names + 1 entries).  Scaffold k is named
 * scaffold_<k + 1>_uid_<unique_id>.  Per contig: a gap line if it is not the first of its scaffold and
 * pos[i] - (pos[i-1] + len[i-1]) > 0, then its own line; the component number counts both and starts at 1 per scaffold.
 * Numbers are signed decimals; |pos|, |len| below 2^62.
 *   besst_dev_text_workspace_bytes   scratch for n_contigs contigs (0: n_contigs out of range); 256-byte aligned
 *   besst_dev_text_measure           fills the workspace (component numbers, the offsets of every contig's lines in both
 *                                    files) and info[0..BESST_TEXT_INFO_WORDS): [0] bytes of the AGP file, [1] of the GFF
 *                                    file, [2] the first contig whose row, name range or scaffold is invalid (all ones:
 *                                    none; its name is written empty)
 *   besst_dev_text_emit              bytes [begin, end) of file `which` to out[0 .. end - begin) (16-byte aligned), from
 *                                    the same columns and the workspace as measured; bytes past the file's end are 0
 * The kernels work in units that tests aim at: BESST_TEXT_THREADS contigs per workgroup of the flag and measure passes,
 * BESST_TEXT_SCAN_CHUNK entries per turn of the scans, BESST_TEXT_TILE_BYTES file bytes per workgroup of the emission.
 *
 * besst_dev_wrap_fasta: record r is contig rows[r] of the pool above: '>' name '\n', then the sequence in lines of 60
 * bytes, each followed by '\n' (the last, shorter one too; an empty sequence has the header line only).  rec_off:
 * n_rows + 1 entries, the exclusive prefix sum of 1 + |name| + 1 + len + ceil(len / 60).  Bytes [begin, end) of that file
 * go to out (16-byte aligned), BESST_WRAP_TILE_BYTES per workgroup.  err[0]: min r of the records whose row, name, pool
 * range or size in rec_off is wrong (their bytes come out as '?'); the caller sets it to all ones.  rows may repeat.
 * Like every besst_dev_* call: device memory and stream are the caller's, work is only enqueued. */
typedef struct besst_text_columns {
    int64_t n_contigs, n_scaffolds, unique_id, n_names, names_bytes;
    const int64_t* pos;
    const int64_t* len;
    const int64_t* row;
    const uint8_t* forward;
    const int32_t* scaffold;
    const int64_t* scaffold_start;
    const uint8_t* names;
    const int64_t* name_off;
} besst_text_columns;
#define BESST_TEXT_AGP 0
#define BESST_TEXT_GFF 1
#define BESST_TEXT_INFO_WORDS 3
#define BESST_TEXT_THREADS 256
#define BESST_TEXT_SCAN_CHUNK 4096
#define BESST_TEXT_TILE_BYTES 16384
#define BESST_WRAP_TILE_BYTES 16384
size_t besst_dev_text_workspace_bytes(int64_t n_contigs);
int besst_dev_text_measure(void* stream, const besst_text_columns* cols, void* workspace, size_t workspace_bytes,
                           int64_t* info);
int besst_dev_text_emit(void* stream, const besst_text_columns* cols, const void* workspace, size_t workspace_bytes,
                        int32_t which, int64_t begin, int64_t end, uint8_t* out, int64_t* info);
int besst_dev_wrap_fasta(void* stream, const uint8_t* pool, int64_t pool_bytes, int64_t n_contigs, const int64_t* ctg_off,
                         const int32_t* ctg_len, const uint8_t* names, int64_t names_bytes, const int64_t* name_off,
                         int64_t n_rows, const int64_t* rows, const int64_t* rec_off, int64_t begin, int64_t end,
                         uint8_t* out, uint64_t* err);

/* ---- BGZF compression of device bytes (csrc/bgzf_deflate.hip; GenerateOutput.py: param.outputs_bgzf) -------------------
 * n_bytes of device memory become a BGZF file: blocks of block_payload input bytes (1..BESST_BGZF_BLOCK_PAYLOAD; only the
 * last may be shorter; none for n_bytes = 0), each an 18-byte header (1f 8b 08 04 00 00 00 00 00 ff 06 00 42 43 02 00,
 * BSIZE - 1), ONE final DEFLATE block, CRC-32 and ISIZE.  The DEFLATE block is dynamic Huffman over literals and matches
 * of distance 1 that never reach in front of the block - or stored, where that would not be smaller than payload + 5
 * bytes: a block is at most payload + 31 bytes.  with_eof appends the 28-byte EOF block.  The same input gives the same
 * bytes.
 *   besst_dev_bgzf_deflate_bound            n_bytes + 31 * ceil(n_bytes / block_payload) (+ 28): what `out` must hold
 *                                           (0: block_payload out of range).  Needs no GPU.
 *   besst_dev_bgzf_deflate_workspace_bytes  scratch of one call: a slot of 64 KiB per block, sizes and offsets (0 as above)
 *   besst_dev_bgzf_deflate                  three kernels on `stream`; out_bytes (device): the file's length; block_off
 *                                           (device, n_blocks + 1 entries, or null): where every block begins, and the end of
 *                                           the last.  BESST_ERR_ARG without touching the device: a null pointer, a
 *                                           block_payload out of range, a workspace or output smaller than the two sizes.
 *                                           The kernels read src in aligned 4-byte words: up to 3 bytes in front of a src
 *                                           that is no multiple of four and up to 3 behind src + n_bytes are read (never
 *                                           across a page) and not used.
 *   besst_bgzf_deflate_device               host buffers in and out (the counterpart of besst_bgzf_inflate_device) */
#define BESST_BGZF_BLOCK_PAYLOAD 65280
size_t besst_dev_bgzf_deflate_bound(int64_t n_bytes, int32_t block_payload, int32_t with_eof);
size_t besst_dev_bgzf_deflate_workspace_bytes(int64_t n_bytes, int32_t block_payload);
int besst_dev_bgzf_deflate(void* stream, const void* src, int64_t n_bytes, int32_t block_payload, int32_t with_eof,
                           void* workspace, size_t workspace_bytes, void* out, size_t out_cap, int64_t* out_bytes,
                           int64_t* block_off);
int besst_bgzf_deflate_device(int device, const void* src, size_t n_bytes, int32_t block_payload, int32_t with_eof, void* out,
                              size_t out_cap, size_t* out_len);

/* ---- SAM text -> the context's record columns (csrc/sam.hip; the per-record rules: csrc/sam_core.h) ---------------------
 * A chunk of record lines in HBM - it begins at a line start and ends at a line end or at the end of the file; 16-byte
 * aligned, below 2^32 - 16 bytes, with 16 readable bytes behind its end - is parsed on the device and its records are
 * appended to the context's columns with exactly what the BAM of the same records gives.  '\n' ends a line, a '\r' in
 * front of it belongs to the terminator, a last line without '\n' is a line.  A record is the first eleven tab-separated
 * fields: FLAG [0-9]+ <= 65535; RNAME '*' -> -1, else its row among the references; POS / PNEXT [0-9]+ <= 2^31 - 1, stored
 * less one; MAPQ <= 255; RNEXT '=' -> tid, '*' -> -1; TLEN -?[0-9]+ within int32; l_seq the length of SEQ ('*': 0); qlen /
 * alen / rlen from CIGAR (operations MIDNSHP=X, counts below 2^28, '*': none) and l_seq as besst_bam_read_records derives
 * them.  QUAL and the optional fields are never read.
 *   besst_ctx_set_sam_references   the header's names end to end (name r: names[name_off[r]] .. names[name_off[r + 1]]),
 *                                  once per file: an open-addressing table of >= 2 n_ref slots is built on the host and
 *                                  uploaded with the names.  BESST_ERR_ARG: an empty or a repeated name.
 *   besst_dev_sam_workspace_bytes  tile scratch the context keeps for a chunk of that size (the rows, 20 bytes per
 *                                  line, come on top); 0: tile_bytes or text_bytes not accepted.  Needs no GPU.
 *   besst_ctx_push_sam_text        tile_bytes: 0 = 16384, else a multiple of 1024 in 1024..65536.  Kernels run on `stream`
 *                                  (null: the context's); the call returns when the chunk is decoded.  info[0] records of
 *                                  the chunk, [1] records whose qlen was saturated at 65535, [2] the smallest file offset
 *                                  (file_offset + offset in the chunk) of the first byte of a line that cannot be read
 *                                  (-1: none), [3] that line's BESST_SAM_* reason.  With an error the records of the chunk
 *                                  are NOT appended.  head_rlen / head_alen / head_qlen (host, head_records entries): the
 *                                  values of the context's first head_records records, filled on across calls.
 *                                  The mate / run planes and the candidate side stream are not written: the watermarks
 *                                  stay where they are, as after besst_ctx_push_records.
 *                                  BESST_ERR_ARG without touching the device: a null context, a tile_bytes out of range,
 *                                  a misaligned text.
 *   besst_ctx_sam_expect_text      optional, before a file's first chunk: the bytes of record text the pushes that follow
 *                                  will bring in all.  When the columns have to grow they then grow once, to what the rest
 *                                  of that text needs at the records per byte seen so far (plus 3 %; at most a record per
 *                                  22 bytes), instead of chunk after chunk; without it they double.
 *   besst_ctx_sam_pass_times       measurement (tools/time_sam_ingest.py): ms[0..4), where given, receives the device time
 *                                  of the flags, state, index (with the rows' memset) and decode passes summed over the
 *                                  pushes since the last call, by events; the sums are cleared and the events switched on
 *                                  or off for the pushes that follow.
 *   besst_dev_sam_lines            the line cutter of a reader that fills a device buffer with inflated text (a compressed
 *                                  SAM, bamio.ResidentSam): one pass over text[0, n_bytes) - 16-byte aligned, n_bytes below
 *                                  2^32 - 16, 16 readable bytes behind the end, bytes behind n_bytes masked as the parser
 *                                  masks them - enqueued on `stream` leaves in out (device, four words)
 *                                    out[0] the offset behind the last '\n' of the text (0: none)
 *                                    out[1] with want_header_end != 0, the smallest line start whose byte is not '@'; a
 *                                           line start is byte 0 and every byte behind a '\n' that lies inside the text.
 *                                           -1: none (and without want_header_end, and for an empty text); n_bytes: every
 *                                           line is a header line and the last one is complete
 *                                    out[2] the number of '\n' in text[0, count_upto)
 *                                    out[3] 0
 *                                  A wave reduces by shuffles and adds at most one 64-bit atomic per word.  BESST_ERR_ARG
 *                                  without touching the device: a null pointer, a misaligned text, n_bytes or count_upto
 *                                  (0..n_bytes) out of range. */
#define BESST_SAM_INFO_WORDS 4
#define BESST_SAM_FEW_FIELDS 1
#define BESST_SAM_EMPTY_LINE 2
#define BESST_SAM_HEADER_LINE 3
#define BESST_SAM_BAD_FLAG 4
#define BESST_SAM_BAD_POS 5
#define BESST_SAM_BAD_MAPQ 6
#define BESST_SAM_BAD_PNEXT 7
#define BESST_SAM_BAD_TLEN 8
#define BESST_SAM_BAD_RNAME 9
#define BESST_SAM_BAD_RNEXT 10
#define BESST_SAM_BAD_CIGAR 11
int besst_ctx_set_sam_references(besst_ctx* ctx, const uint8_t* names, const int64_t* name_off, int64_t n_ref);
size_t besst_dev_sam_workspace_bytes(int64_t text_bytes, int64_t tile_bytes);
int besst_ctx_push_sam_text(besst_ctx* ctx, void* stream, const uint8_t* text, int64_t text_bytes, int64_t file_offset,
                            int64_t tile_bytes, int64_t head_records, int32_t* head_rlen, int32_t* head_alen,
                            uint16_t* head_qlen, int64_t* info);
int besst_ctx_sam_expect_text(besst_ctx* ctx, int64_t text_bytes);
int besst_ctx_sam_pass_times(besst_ctx* ctx, int enable, double* ms);
int besst_dev_sam_lines(void* stream, const uint8_t* text, int64_t n_bytes, int32_t want_header_end, int64_t count_upto,
                        int64_t* out);

/* ---- the sequence census: what a byte string holds, counted where it lies (csrc/seq_census.hip, seq_census_core.h) ------
 * The census of one byte string is BESST_CENSUS_WORDS words of int64:
 *   LEN        bytes seen
 *   A C G T    counts, case folded
 *   N          'N' or 'n'
 *   IUPAC      YRKMBVHDSW in either case, and upper-case X
 *   OTHER      every other byte value: the bytes besst_host_complement_table has no complement for, so OTHER > 0 says that
 *              writing the string reversed raises the reference's KeyError
 *   LOWER      bytes 'a'..'z', whatever their class
 *   PRE        length of the run of N that starts at byte 0 (LEN if the string is all N)
 *   SUF        length of the run of N that ends at the last byte (LEN if all N)
 *   RUNS       closed runs of N: those that touch neither end
 *   GAPS       ... of length >= min_gap;  GAP_BASES: the sum of their lengths;  LONGEST: the longest closed run
 *   word 15    0
 * Merge of neighbours a·b (census_merge): an empty side yields the other; words 0-8, RUNS, GAPS and GAP_BASES add, LONGEST
 * is the maximum; PRE = a is all N ? a.LEN + b.PRE : a.PRE; SUF = b is all N ? a.SUF + b.LEN : b.SUF; if neither side is
 * all N and a.SUF + b.PRE > 0 that joined run is closed.  The rule is associative, so a string may be counted in pieces
 * of any size.  Finalise (census_finalise, the caller's, after the last merge): an all-N string closes one run of LEN,
 * otherwise PRE and SUF are each closed if they are not zero.
 *
 * besst_dev_seq_census: buf[0 .. n) is a window of a longer byte stream and begins at stream position `origin`; row i of
 * the table is the stream bytes [seq_off[i], seq_off[i] + seq_len[i]), rows ascending and disjoint (rows of length 0
 * anywhere).  For every row that intersects the window the call counts the intersection and merges it into acc as the
 * right-hand neighbour, acc[i] = merge(acc[i], part); rows that do not intersect keep their words bit for bit.  The caller
 * zeroes acc before the first window and hands the windows of a stream over in ascending order on one stream.  The rows
 * are found by a search of the window's bounds in seq_off: the work is that of the window, whatever n_seq is.
 *   Reads: only aligned 16-byte groups that hold a byte of the window (any address of buf; a buffer that is readable in
 *   whole 16-byte groups - the sequence pool with its BESST_EMIT_PAD, an output buffer of whole groups - satisfies it).
 *   workspace: besst_dev_seq_census_workspace_bytes(n, n_seq) bytes for windows of up to n bytes, 16-byte aligned;
 *   the tile partials of the rows that cross a border of besst_dev_seq_census_tile_bytes() bytes live there.
 *   status[0]: min over the rows the call walked (every row from the one the search finds to the first one behind the
 *   window, each held against its predecessor) of the rows that begin in front of their predecessor's end or have a
 *   negative field; the caller sets both words to -1 (all ones) before the first window.  Such a table makes the
 *   result meaningless, never a read or a write outside the buffers.  status[1]: min over the walked rows of those with
 *   a negative offset or length (they are counted as empty), -1 if there is none.
 *   Nothing is allocated, nothing waits.  n == 0 or n_seq == 0: nothing is launched.
 * besst_host_seq_census: the same on host memory with the same rules, byte by byte (BESST_ERR_ARG and the row in
 * besst_last_error for a table that is out of order). */
#define BESST_CENSUS_WORDS 16
#define BESST_CENSUS_LEN 0
#define BESST_CENSUS_A 1
#define BESST_CENSUS_C 2
#define BESST_CENSUS_G 3
#define BESST_CENSUS_T 4
#define BESST_CENSUS_N 5
#define BESST_CENSUS_IUPAC 6
#define BESST_CENSUS_OTHER 7
#define BESST_CENSUS_LOWER 8
#define BESST_CENSUS_PRE 9
#define BESST_CENSUS_SUF 10
#define BESST_CENSUS_RUNS 11
#define BESST_CENSUS_GAPS 12
#define BESST_CENSUS_GAP_BASES 13
#define BESST_CENSUS_LONGEST 14
#define BESST_CENSUS_TILE_BYTES 8192
size_t besst_dev_seq_census_workspace_bytes(int64_t window_bytes, int64_t n_seq);
int64_t besst_dev_seq_census_tile_bytes(void);
int besst_dev_seq_census(void* stream, const uint8_t* buf, int64_t origin, int64_t n, int64_t n_seq, const int64_t* seq_off,
                         const int64_t* seq_len, int64_t min_gap, void* workspace, int64_t* acc, int64_t* status);
int besst_host_seq_census(const uint8_t* buf, int64_t origin, int64_t n, int64_t n_seq, const int64_t* seq_off,
                          const int64_t* seq_len, int64_t min_gap, int64_t* acc);

#ifdef __cplusplus
}
#endif
#endif /* BESST_AMD_H */
