/* include/lrsc.h -- C ABI of the MI355X-native PacBio self-correction hot path.
 *
 * This is the drop-in boundary: the C++ host side (longreadselfcorrect_amd/host,
 * which mirrors the reference's SequenceProcessFramework / PacBioSelfCorrectionProcess
 * interface) and any foreign binding call ONLY these entry points.  Plain pointers and
 * sizes; no C++ or torch types.  Every function returns 0 (LRSC_OK) or a negative
 * lrsc_status and never calls exit(); the caller owns every buffer it passes.
 *
 * Reference interface each group replaces (paths relative to the reference tree):
 *   lrsc_index_*          RLBWT::RLBWT(file) + initializeFMIndex   SuffixTools/RLBWT.cpp:23-32,109-248
 *                         (loaded at StriDe/PacBioSelfCorrection.cpp:155-172)
 *   lrsc_rank             RLBWT::getOcc / getPC                    SuffixTools/RLBWT.h:118-140
 *   lrsc_bwt_chars        RLBWT::getChar                           SuffixTools/RLBWT.h:42-63
 *   lrsc_index_locate_*,  SampledSuffixArray::build / buildLexicoIndex / calcSA    SuffixTools/SampledSuffixArray.cpp:44-190
 *   lrsc_index_lexico_order, lrsc_locate
 *   lrsc_find_kmers       BWTAlgorithms::findInterval/findBiInterval  SuffixTools/BWTAlgorithms.cpp:14-38
 *   lrsc_kmer_grid        KmerFeature grid of LongReadProbe::getSeqAttribute
 *                         PacBio/LongReadProbe.cpp:139-150, PacBio/KmerFeature.h:37-64,92-99
 *   lrsc_find_seeds       LongReadProbe::searchSeedsWithHybridKmers   PacBio/LongReadProbe.cpp:34-117,187-227
 *   lrsc_extend_walks     LongReadSelfCorrectByOverlap ctor + extendOverlap
 *                         PacBio/LongReadCorrectByOverlap.cpp:17-95,155-211
 *   lrsc_correct_batch    PacBioSelfCorrectionProcess::process     PacBio/PacBioSelfCorrectionProcess.cpp:23-206
 *
 * Threading: an lrsc_index is immutable after lrsc_index_upload and may be shared;
 * an lrsc_ctx is single-threaded (one per host worker / per device) and every call on it
 * is synchronous with respect to the caller unless stated otherwise.
 */
#ifndef LRSC_H
#define LRSC_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LRSC_ABI_VERSION 2

typedef enum lrsc_status {
    LRSC_OK = 0,
    LRSC_ERR_IO = -1,          /* cannot open / short read                      */
    LRSC_ERR_FORMAT = -2,      /* "BWT file is not properly formatted"          */
    LRSC_ERR_ARG = -3,         /* bad argument (null, range, non-ACGT base ...)  */
    LRSC_ERR_NOMEM = -4,
    LRSC_ERR_DEVICE = -5,      /* HIP runtime error, no device, not uploaded     */
    LRSC_ERR_CAPACITY = -6,    /* caller-provided output buffer too small        */
    LRSC_ERR_UNSUPPORTED = -7,
    LRSC_ERR_LIMIT = -8           /* an internal capacity of the device implementation was exceeded (see lrsc_last_error) */
} lrsc_status;

typedef struct lrsc_index lrsc_index;   /* both strands' FM-index: host image + per-device copies */
typedef struct lrsc_ctx lrsc_ctx;       /* per-device execution context (stream, scratch, params)  */

/* BWTInterval (SuffixTools/BWTInterval.h:19-81): lower > upper == invalid */
typedef struct lrsc_interval { int64_t lower, upper; } lrsc_interval;
/* BiBWTInterval (BWTInterval.h:82-100): fwd = interval of reverse(w) in the .rbwt index,
 * rvc = interval of reverse-complement(w) in the .bwt index */
typedef struct lrsc_biinterval { lrsc_interval fwd, rvc; } lrsc_biinterval;

/* which strand's index a raw rank / char query addresses */
enum { LRSC_BWT = 0, LRSC_RBWT = 1 };

typedef struct lrsc_rank_query {
    int64_t idx;       /* position in the BWT, -1 allowed (Occ == 0), < num_symbols */
    uint8_t base;      /* 'A','C','G','T' */
    uint8_t strand;    /* LRSC_BWT or LRSC_RBWT */
    uint8_t pad[6];
} lrsc_rank_query;

typedef struct lrsc_index_info {
    uint64_t num_strings;        /* reads in the index                        */
    uint64_t num_symbols;        /* BWT length per strand (bases + num_strings) */
    uint64_t num_runs[2];        /* RL units on disk (.bwt, .rbwt); 0 for an index made by lrsc_index_build */
    uint64_t pred_count[2][5];   /* C[$ACGT] per strand                         */
    uint32_t block_bytes;        /* bytes of one device rank block              */
    uint32_t block_symbols;      /* BWT symbols covered by one rank block       */
    uint64_t device_bytes;       /* HBM bytes of both strands once uploaded     */
} lrsc_index_info;

/* Parameters of the correction path: a POD mirror of PacBioSelfCorrectionParameters +
 * FMextendParameters + ProbeParameters (PacBio/PacBioSelfCorrectionProcess.h:24-53,
 * LongReadCorrectByOverlap.h:28-47, LongReadProbe.h:7-40) AFTER the driver's derivation
 * step (StriDe/PacBioSelfCorrection.cpp:195-206).  Fill with lrsc_params_default(). */
typedef struct lrsc_params {
    int32_t pb_coverage;        /* -c, default 90                                  */
    double  error_rate;         /* -e, default 0.15                                */
    int32_t start_kmer_len;     /* derived from -g: {5:17, 10:19, 100:21}          */
    int32_t offset[3];          /* static k-mer size offset per mode (0,1,2)       */
    int32_t mode;               /* -m, default 1 (only used when manual != 0)      */
    int32_t manual;             /* -k/-u/-r given                                  */
    int32_t scan_kmer_len;      /* 19  (LongReadProbe.h:27)                        */
    int32_t kmer_len_up_bound;  /* 50  (LongReadProbe.h:28)                        */
    int32_t radius;             /* 100 (LongReadProbe.h:32)                        */
    float   hh_ratio;           /* 0.6f (LongReadProbe.h:33)                       */
    int32_t next_target;        /* -n, default 1                                   */
    int32_t max_leaves;         /* -l, default 32; 1..256 (above 32: the walks that outgrow 32 leaves run again in a
                                 * wide launch with room for -l leaves, LRSC_K_EXTEND_WIDE)                       */
    int32_t idmer_len;          /* -i, default 9                                   */
    int32_t min_kmer_len;       /* -s, default 13                                  */
    int32_t split;              /* --split                                         */
    int32_t no_dp;              /* --nodp                                          */
} lrsc_params;

/* genome = 5, 10 or 100 (the -g option); coverage = -c.  Reproduces the derivation at
 * StriDe/PacBioSelfCorrection.cpp:195-200. Returns LRSC_ERR_ARG for another genome value. */
int lrsc_params_default(int genome, int coverage, lrsc_params* out);

/* ---- index ------------------------------------------------------------------------ */
/* Parse <prefix>.bwt and <prefix>.rbwt (binary RL format, Appendix C of SURVEY.md) and
 * build the HBM rank-block image on the host. */
int lrsc_index_open(const char* bwt_path, const char* rbwt_path, lrsc_index** out);
/* Same, from RL-unit strings already in memory (units: (rank<<5)|run_len). */
int lrsc_index_from_units(const uint8_t* bwt_units, uint64_t n_bwt_units,
                          const uint8_t* rbwt_units, uint64_t n_rbwt_units,
                          uint64_t num_strings, uint64_t num_symbols, lrsc_index** out);
/* lrsc_index_open / lrsc_index_from_units with the decode on `device`: what RLBWT::RLBWT(file) + initializeFMIndex
 * (SuffixTools/RLBWT.cpp:23-32,109-248) do with the units that BWTReaderBinary.cpp:55-85 reads.  The RL units of one strand
 * after the other go to the device as they are and are packed into rank blocks there; no host pass over the symbols.
 * Same checks, statuses and messages as the host route; on an error nothing stays allocated and *out is untouched.
 * On return the index is resident on `device` (lrsc_index_upload(idx, device) is a no-op) with its k-mer tables, and carries
 * a host image, so lrsc_index_upload to any other device works as for an opened index. */
int lrsc_index_open_device(const char* bwt_path, const char* rbwt_path, int device, lrsc_index** out);
int lrsc_index_from_units_device(const uint8_t* bwt_units, uint64_t n_bwt_units,
                                 const uint8_t* rbwt_units, uint64_t n_rbwt_units,
                                 uint64_t num_strings, uint64_t num_symbols, int device, lrsc_index** out);
int lrsc_index_info_get(const lrsc_index* idx, lrsc_index_info* out);
/* Copy both strands into `device`'s HBM (idempotent per device). */
int lrsc_index_upload(lrsc_index* idx, int device);
void lrsc_index_close(lrsc_index* idx);

/* ---- index construction (the `stride index -a ropebwt2` step; StriDe/index.cpp:164-213,
 *      SuffixTools/BWTCARopebwt.cpp:160-247) ------------------------------------------------ */
/* Builds the multi-string BWT of the reads (reverse_reads == 0 -> the .bwt payload) or of the
 * reversed reads (reverse_reads != 0 -> the .rbwt payload) on `device` by suffix sorting, sentinels in
 * input order, and returns it as the reference's RL units ((rank<<5)|run, runs <= 31,
 * BWTWriterBinary.cpp:50-71).  *units_out is malloc'ed: release with lrsc_buffer_free.
 * num_symbols == read_off[n_reads] + n_reads. */
int lrsc_build_bwt(const char* reads, const uint64_t* read_off, uint32_t n_reads, int reverse_reads, int device,
                   uint8_t** units_out, uint64_t* n_units_out);
void lrsc_buffer_free(void* p);
/* Both strands' FM-index of the reads, built and packed on `device`; no files.  On return the index is resident on
 * `device` (lrsc_index_upload(idx, device) is a no-op) with its k-mer tables, and carries a host image, so
 * lrsc_index_upload to any other device works as for an opened index.  Same read checks and messages as lrsc_build_bwt. */
int lrsc_index_build(const char* reads, const uint64_t* read_off, uint32_t n_reads, int device, lrsc_index** out);
/* The index of a's reads followed by b's, merged on `device` from the two resident copies; byte for byte what
 * lrsc_index_build makes of the concatenated reads.  a and b need a copy on `device` (LRSC_ERR_DEVICE otherwise), are not
 * modified and stay usable; a == b is allowed (every read twice).  The result is resident on `device` with its k-mer tables
 * and carries a host image, as a built index does; num_runs is 0 as for a built index.
 * dollar_origin (may be NULL): 2 * (n_a + n_b) bytes; entry s * (n_a + n_b) + k is 1 when the k-th '$' row of strand s of
 * the merged BWT is a row of b, else 0 (what merging the .sai/.rsai lists needs).
 * LRSC_ERR_UNSUPPORTED for 2^32 reads or more in total and for the packer's block limit; on an error nothing stays
 * allocated and *out is untouched. */
int lrsc_index_merge(lrsc_index* a, lrsc_index* b, int device, lrsc_index** out, uint8_t* dollar_origin);
/* 30-byte header + units, the reference's binary .bwt/.rbwt format (BWTWriterBinary.cpp:28-46,82-93). */
int lrsc_write_bwt_file(const char* path, const uint8_t* units, uint64_t n_units, uint64_t num_strings,
                        uint64_t num_symbols);
/* RL units of one strand's BWT (BWTWriterBinary::writeBWChar's rule), encoded on `device` from the index's resident copy there.
 * *units_out is malloc'ed (lrsc_buffer_free).  Works on any index, built or opened, that has a copy on `device`
 * (LRSC_ERR_DEVICE otherwise); the index itself is not modified. */
int lrsc_index_units(lrsc_index* idx, int strand, int device, uint8_t** units_out, uint64_t* n_units_out);
/* Both strands through lrsc_index_units and lrsc_write_bwt_file's header and layout. */
int lrsc_index_write(lrsc_index* idx, int device, const char* bwt_path, const char* rbwt_path);

/* ---- locate: which read and offset a BWT row belongs to (SuffixTools/SampledSuffixArray.cpp) -------------------------- */
/* SAElem (SuffixTools/SampledSuffixArray.h): SA[row] = the suffix of `read` that starts at `pos` (pos == the read's length at
 * its sentinel row, 0 at its '$' row) */
typedef struct lrsc_sa_elem { uint32_t read, pos; } lrsc_sa_elem;
/* Builds both strands' locate tables on `device` from the resident copy and keeps them with that copy: order (k-th '$' row ->
 * read), read lengths, and for sample_rate > 0 the SA of every row that is a multiple of sample_rate
 * (SampledSuffixArray::build, SampledSuffixArray.cpp:90-155; 0 = the lexicographic index only, as SSA_FT_SAI /
 * buildLexicoIndex, :158-190).  (num_symbols / sample_rate + 1) * 8 bytes per strand plus 8 bytes per read.
 * A no-op when tables of the same rate are there; LRSC_ERR_ARG ("already prepared with rate R") for another rate: contexts may
 * be using the tables.  LRSC_ERR_DEVICE if the index has no copy on `device`, LRSC_ERR_FORMAT for an index whose backward walks
 * do not end (no BWT of a string set), LRSC_ERR_NOMEM when the tables do not fit; on an error nothing stays allocated.
 * lrsc_index_close frees the tables. */
int lrsc_index_locate_prepare(lrsc_index* idx, int device, uint32_t sample_rate);
/* The .sai (strand LRSC_BWT) / .rsai (LRSC_RBWT) content, SampledSuffixArray::buildLexicoIndex + writeLexicoIndex
 * (SampledSuffixArray.cpp:158-190,248-258): order[k] = the read of the k-th '$' row, read_len[i] = the length of read i
 * (may be NULL); num_strings entries each.  Prepares with rate 0 if not prepared. */
int lrsc_index_lexico_order(lrsc_index* idx, int strand, int device, uint32_t* order, uint32_t* read_len);

/* ---- context ------------------------------------------------------------------------ */
int lrsc_ctx_create(const lrsc_index* idx, const lrsc_params* params, int device, lrsc_ctx** out);
void lrsc_ctx_destroy(lrsc_ctx* ctx);

/* ---- FM primitives (host buffers in, host buffers out) --------------------------------- */
/* out[i] = Occ(base, idx) = #base in BWT[0..idx] of the chosen strand (RLBWT::getOcc). */
int lrsc_rank(lrsc_ctx* ctx, const lrsc_rank_query* q, uint64_t n, uint64_t* out);
/* out[i] = BWT[idx[i]] of `strand` as '$','A','C','G','T' (RLBWT::getChar). */
int lrsc_bwt_chars(lrsc_ctx* ctx, int strand, const uint64_t* idx, uint64_t n, char* out);
/* n fixed-length k-mers, concatenated (n*k bytes, ACGT). out[i] = findBiInterval(kmer_i):
 * fwd searched in the rbwt with reverse(w), rvc in the bwt with revcomp(w), each stopping at
 * the first invalid interval exactly as BWTAlgorithms.cpp:14-31. */
int lrsc_find_kmers(lrsc_ctx* ctx, const char* kmers, uint32_t k, uint64_t n, lrsc_biinterval* out);

/* SampledSuffixArray::calcSA (SuffixTools/SampledSuffixArray.cpp:44-81) for n rows of `strand` (rows < num_symbols, LRSC_ERR_ARG
 * otherwise), on the ctx's device, from the tables lrsc_index_locate_prepare left there (LRSC_ERR_DEVICE if there are none).
 * For strand LRSC_RBWT, pos counts in the reversed read.  Counted under LRSC_K_LOCATE; rank_queries = LF steps. */
int lrsc_locate(lrsc_ctx* ctx, int strand, const uint64_t* rows, uint64_t n, lrsc_sa_elem* out);

/* ---- duplicate check and read removal: `stride filter` (Algorithm/QCProcess.cpp:206-265, StriDe/filter.cpp) ----------------- */
/* QCProcess::performDuplicateCheck's DuplicateCheckResult, plus LRSC_DUP_ABSENT: neither the read nor its reverse complement is
 * a read of the index (the reference then tests bit INT64_MAX of its bit vector; here the bit vector is left alone). */
enum lrsc_dup_class { LRSC_DUP_UNIQUE = 0, LRSC_DUP_SUBSTRING = 1, LRSC_DUP_FULL_LENGTH = 2, LRSC_DUP_ABSENT = 3 };
typedef struct lrsc_dup_result {
    lrsc_interval fwd_dollar;   /* ranks among the '$' rows of .bwt of the reads equal to w (interval[0] after updateBothL(.., '$')); lower > upper: none ({0, -1}) */
    lrsc_interval rvc_dollar;   /* the same for reverseComplement(w) */
    int32_t cls; uint32_t pad;
} lrsc_dup_result;
typedef struct lrsc_dupcheck lrsc_dupcheck;      /* the shared bit vector of filterMain (num_strings bits), on the ctx's device, all clear */
/* The bit vector and a 32-bit word per read of the index (the read that claims a slot within one call).  The ctx must outlive it. */
int  lrsc_dupcheck_create(lrsc_ctx* ctx, lrsc_dupcheck** out);
/* performDuplicateCheck for n_reads reads (concatenated ACGT bytes, n_reads + 1 offsets) against the ctx's index.  A read w with
 * reverse complement rc is SUBSTRING when w or rc is a proper substring of a read of the index, ABSENT when neither is a read of
 * it; otherwise its canonical index is the smaller valid lower of the two '$' intervals, and it is UNIQUE when that bit is clear
 * (it sets the bit) and FULL_LENGTH when the bit is set.  Both '$' intervals are filled for every class.
 * The order is that of the reference's serial mode (-t 1): within a call in read order, across the calls of one lrsc_dupcheck in
 * call order.  The reference with threads lets a compare-and-swap race decide which copy of a duplicate survives; this
 * implementation does not race: the result is the serial one however the device schedules its lanes.
 * LRSC_ERR_ARG for an empty read (the reference reads w[-1]) and for a base other than A,C,G,T; on an error the bit vector is
 * as it was.  The search launches are counted under LRSC_K_FIND. */
int  lrsc_dupcheck_reads(lrsc_dupcheck* dc, const char* reads, const uint64_t* read_off, uint32_t n_reads, lrsc_dup_result* out);
void lrsc_dupcheck_destroy(lrsc_dupcheck* dc);
/* The index of idx's reads whose drop[] byte is 0, in their order; byte for byte what lrsc_index_build makes of those reads.
 * Made on `device` from idx's copy there (LRSC_ERR_DEVICE without one) with no suffix sort: the rows of the dropped reads are
 * marked by backward walks and the rest is compacted and packed.  idx is not modified and stays usable.  The result is resident
 * on `device` with its k-mer tables and carries a host image, as a built index does; num_runs is 0.
 * LRSC_ERR_ARG if n_reads != num_strings or nothing is kept, LRSC_ERR_FORMAT if a walk does not end at a '$' row or the marked
 * rows are not the dropped reads' (an index that is no BWT of a string set), LRSC_ERR_UNSUPPORTED at the packer's and locate's
 * limits; on an error nothing stays allocated and *out is untouched. */
int lrsc_index_remove(lrsc_index* idx, const uint8_t* drop, uint64_t n_reads, int device, lrsc_index** out);

/* ---- k-mer read correction: `stride correct -a kmer` (Algorithm/ErrorCorrectProcess.cpp:287-438, 488-544) --------------------- */
typedef struct lrsc_kcorrect_params { int32_t kmer_length, kmer_threshold, kmer_rounds, quality_cutoff; } lrsc_kcorrect_params; /* -k 31, -x 3, -i 10, 20 */
typedef struct lrsc_kcorrect_result { uint32_t kmer_qc, n_changed, passes, pad; } lrsc_kcorrect_result;
/* ErrorCorrectProcess::kmerCorrection for n_reads reads (concatenated ACGT bytes, n_reads + 1 offsets) against the ctx's index;
 * the result is that of the reference's serial run, byte for byte.  The count of a k-mer is the size of its interval in .bwt plus
 * that of its reverse complement's (BWTAlgorithms::countSequenceOccurrences).  A k-mer marks its bases solid when its count
 * reaches the support of the lowest phred among them: kmer_threshold at quality_cutoff or above, else kmer_threshold + 1
 * (Util/CorrectionThresholds.cpp:26-39); phred = one score per base (quality character - 33), NULL = 15 everywhere.  While a
 * base is unsolid, the first unsolid base from the left for which attemptKmerCorrection succeeds with its leftmost or else its
 * rightmost covering k-mer is replaced: by the last base in A,C,G,T order whose k-mer count is at least twice max(the k-mer's
 * count, the support of the base's phred), if that is not the base itself.  `if(rounds++ > maxAttempts) break;` allows
 * kmer_rounds + 1 corrections and kmer_rounds + 2 counting passes.
 * corrected = the reads after it, at the same offsets: a read that ended all solid as edited with kmer_qc = 1, any other one,
 * and a read shorter than kmer_length, unedited with kmer_qc = 0.  passes = the counting passes made (0 for a read shorter than
 * kmer_length), n_changed = the bases of corrected that differ from the read.
 * LRSC_ERR_ARG for kmer_length, kmer_threshold or kmer_rounds <= 0, for an empty read and for a base other than A,C,G,T;
 * LRSC_ERR_FORMAT when an interval leaves the strand (an index that is no BWT of a string set); on an error corrected and out
 * are untouched.  n_reads == 0 does nothing.  The launches are counted under LRSC_K_FIND; a backward-search step is two of its
 * rank_queries. */
int lrsc_kmer_correct(lrsc_ctx* ctx, const char* reads, const uint64_t* read_off, uint32_t n_reads,
                      const uint8_t* phred /* one per base, NULL = 15 everywhere */,
                      const lrsc_kcorrect_params* p, char* corrected /* same offsets as reads */, lrsc_kcorrect_result* out);

/* ---- paired-end reads merged by an FM-index walk: `stride fmwalk -a merge` (FMIndexWalk/FMIndexWalkProcess.cpp:153-226, 825-870;
 * FMIndexWalk/SAIntervalTree.cpp:20-56, 103-170, 248-449, 494-507) ---------------------------------------------------------- */
typedef struct lrsc_fmwalk_params { int32_t kmer_length, kmer_threshold, min_overlap, max_overlap /* -1: from the lengths */, max_insert, max_leaves; } lrsc_fmwalk_params; /* -k 31 -x 3 -m 81 -M -1 -I 400 -L 32 */
typedef struct lrsc_fmwalk_result { uint32_t merged, length; int32_t status[2]; uint32_t max_used_leaves[2]; uint64_t coverage[2]; uint32_t trimmed_length[2]; } lrsc_fmwalk_result;
/* The kernel's limits: LRSC_ERR_UNSUPPORTED above them. */
#define LRSC_FMWALK_MAX_LEAVES 64
#define LRSC_FMWALK_MAX_INSERT 2000
#define LRSC_FMWALK_MAX_MIN_OVERLAP 255
#define LRSC_FMWALK_MAX_KMER 255
/* FMIndexWalkProcess::MergePairedReads for n_pairs pairs against the ctx's index, reads 2i and 2i + 1 (concatenated ACGT bytes,
 * 2 * n_pairs + 1 offsets) being pair i; the result is that of the reference's serial run, byte for byte.  Both reads are trimmed
 * (trimRead: a head or tail kmer_length-mer that no base extends outwards is cut back to the first position that two or more
 * bases extend); a pair with a trimmed read shorter than min_overlap is not merged, status = {0, 0}.  Otherwise two walks
 * (SAIntervalTree::mergeTwoReads) go from the first min_overlap bases of one trimmed read to the reverse complement of the
 * other's, walk 0 from the first read and walk 1 from the second: a breadth-first frontier of at most max_leaves leaves that
 * extends by every base whose k-mer occurs kmer_threshold times on both strands together, the k-mer growing from min_overlap to
 * max_overlap (-1: 0.9 * the mean of the two untrimmed lengths) and falling back, until a leaf's interval lies within the
 * target's or the string is longer than max_insert.  Of a walk's results the one with the strictly greatest coverage (the sum
 * of the occurrences of its min_overlap-mers at stride min_overlap / 2) is its string.  The pair is merged when one walk has a
 * string, or both have one of the same length (then walk 0's if its coverage is greater, else walk 1's, which reads on the other
 * strand).
 * out[i]: merged, the string's length, and per walk status (1 found, -1 the frontier emptied, -2 depth, -3 leaves, -4 otherwise),
 * max_used_leaves, coverage (getKmerCoverage()); trimmed_length per read.  A read shorter than kmer_length, on which the
 * reference throws, leaves its pair unmerged with trimmed_length 0.  merged + i * stride holds pair i's string when it is merged
 * and is not written otherwise.
 * LRSC_ERR_ARG for a parameter <= 0 other than max_overlap == -1, min_overlap < 2, an empty read, a base other than A,C,G,T and
 * a stride below max(max_insert + 1, min_overlap); LRSC_ERR_UNSUPPORTED above the limits; LRSC_ERR_FORMAT when an interval leaves
 * the strand (an index that is no BWT of a string set); on an error merged and out are untouched.  n_pairs == 0 does nothing.  The
 * launches are counted under LRSC_K_FIND; a backward-search step is two of its rank_queries. */
int lrsc_fmwalk_merge(lrsc_ctx* ctx, const char* reads, const uint64_t* read_off, uint32_t n_pairs /* reads 2i, 2i+1 */,
                      const lrsc_fmwalk_params* p, char* merged /* n_pairs * stride */, uint64_t stride /* >= max(max_insert + 1, min_overlap) */,
                      lrsc_fmwalk_result* out);

/* ---- fmwalk's hybrid and kmerize algorithms: reads cut at their unreliable k-mers (FMIndexWalk/FMIndexWalkProcess.cpp:29-150,
 * 229-267, 394-477, 555-609, 855-881; FMIndexWalkProcess.h:61-130) and the sampled k-mer counts that hybrid's repeat gate reads
 * (StriDe/FMIndexWalk.cpp:147-154; SuffixTools/BWTAlgorithms.cpp:135-141, 396-402, 454-469, 527-539) ---------------------------- */
/* One piece of a read (an element of splitRead's kmerReads): read[start .. start + length) of the untrimmed read; kept = 0 when
 * hybrid's isLowComplexity or maxCon filter drops it. */
typedef struct lrsc_fmwalk_piece { uint32_t start, length, kept; } lrsc_fmwalk_piece;
/* What the algorithms leave of one read: kmerize (FMIndexWalkResult::kmerize or kmerize2); the trimmed read is read[head .. head
 * + length) (hybrid; kmerize does not trim: 0 and the read's length, or 0 and 0 for a read shorter than kmer_length); its
 * n_pieces pieces in read order; main_piece = splitRead's mainSeedIdx, -1 for none; whole = the [k, m] length gate has set
 * correctSequence to the whole trimmed read.  correctSequence is the main piece when there is one and it is kept, else the
 * trimmed read when whole, else empty; kmerizedReads are the other kept pieces in order. */
typedef struct lrsc_fmwalk_read_result { uint32_t kmerize; int32_t head; uint32_t length, n_pieces; int32_t main_piece; uint32_t whole; } lrsc_fmwalk_read_result;
typedef struct lrsc_fmwalk_hybrid_result { lrsc_fmwalk_result walk; lrsc_fmwalk_read_result read[2]; } lrsc_fmwalk_hybrid_result;
#define LRSC_KMER_SAMPLE_MAX_LENGTH 4096
/* BWTAlgorithms::sampleKmerCounts (BWTAlgorithms.cpp:527-539) without its rand(): for each of the n rows, rows[i] < the index's
 * strings, extractString(pRBWT, rows[i], len) (454-469: up to len LF steps from the '$' row, ending at '$') and
 * countSequenceOccurrences of that string in .rbwt (135-141), to counts[i] (saturating at 2^32 - 1).  LRSC_ERR_ARG for len == 0 or
 * a row that is none of the '$' rows, LRSC_ERR_UNSUPPORTED for len above LRSC_KMER_SAMPLE_MAX_LENGTH; on an error counts is
 * untouched.  n == 0 does nothing.  The launch is counted under LRSC_K_FIND. */
int lrsc_kmer_sample_counts(lrsc_ctx* ctx, const uint64_t* rows, uint32_t n, uint32_t len, uint32_t* counts);
/* FMIndexWalkProcess::KmerizeReads (FMIndexWalkProcess.cpp:229-267) for n_reads single reads: no trim, no filters.  A read is cut
 * (splitRead(KmerContext&), 555-609) at every boundary between two k-mers that are not both solid (kmer_threshold occurrences
 * in .bwt or more of the k-mer and as many of its reverse complement) and whose link is not simple (isSimple, 873-881: exactly
 * one base extends the left k-mer to the right and exactly one the right k-mer to the left, counted on both strands together with
 * a threshold of 1).  The main piece is the first of the pieces with the most k-mers among those that hold a solid k-mer and have
 * more than one k-mer.  Read i's
 * pieces stand from pieces[slot_i] on, slot_i = the sum over the reads j < i of max(len_j - kmer_length + 1, 0); n_piece_slots
 * is the size of pieces and at least that sum over all reads (LRSC_ERR_ARG below it).  A read shorter than kmer_length gives
 * nothing (kmerize 0).  Errors as lrsc_fmwalk_merge; on an error out and pieces are untouched; entries of pieces beyond a read's
 * n_pieces are never written. */
int lrsc_fmwalk_kmerize(lrsc_ctx* ctx, const char* reads, const uint64_t* read_off, uint32_t n_reads, int32_t kmer_length, int32_t kmer_threshold,
                        lrsc_fmwalk_read_result* out, lrsc_fmwalk_piece* pieces, uint64_t n_piece_slots);
/* FMIndexWalkProcess::MergeAndKmerize (FMIndexWalkProcess.cpp:29-150) for n_pairs pairs, reads and merged as lrsc_fmwalk_merge's.
 * Both reads are trimmed; when a trimmed length lies in [kmer_length, min_overlap] both reads are marked kmerized with their
 * whole trimmed reads, and the pair goes on; otherwise a pair with a trimmed read shorter than kmer_length ends there.  The pair
 * is walked (isSuitableForFMWalk, 394-415) when both trimmed reads reach min_overlap and the first min_overlap-mer of each occurs
 * fewer than repeat_kmer_freq times in .bwt on both strands together; the walks are lrsc_fmwalk_merge's with the constructor's
 * default threshold of 3 whatever kmer_threshold says, and max_overlap -1 standing for 0.95 of the mean untrimmed length.  It is
 * merged when one walk alone has a string and neither used more than one leaf, or both have one and one is the other's reverse
 * complement (then walk 0's if its coverage is greater).  Otherwise both trimmed reads of kmer_length bases or more are split as
 * by lrsc_fmwalk_kmerize, with the pieces' filters: isLowComplexity (418-445: a base makes up 0.9 of the piece or more, as a float
 * quotient against the double 0.9, so exactly nine tenths is kept) and maxCon(piece) * 3 > length (448-477).
 * out[i].walk is lrsc_fmwalk_merge's record (status 0 for a pair that is not walked); out[i].read[] as above, kmerize and whole as
 * the gate left them even when the pair is merged.  The pieces' slots are computed from the untrimmed lengths.  A read shorter than
 * kmer_length, on which the reference throws, counts as trimmed to nothing.  Errors as lrsc_fmwalk_merge; on an error merged, out
 * and pieces are untouched. */
int lrsc_fmwalk_hybrid(lrsc_ctx* ctx, const char* reads, const uint64_t* read_off, uint32_t n_pairs /* reads 2i, 2i+1 */, const lrsc_fmwalk_params* p,
                       uint64_t repeat_kmer_freq, char* merged /* n_pairs * stride */, uint64_t stride, lrsc_fmwalk_hybrid_result* out,
                       lrsc_fmwalk_piece* pieces, uint64_t n_piece_slots);

/* ---- fmwalk's validate algorithm: single reads validated by walks inside them (FMIndexWalk/FMIndexWalkProcess.cpp:269-391
 * ValidateReads, 613-722 splitRead(std::string&), 418-445 and 855-881 isLowComplexity, numNextKmer, isSimple; FMIndexWalk/
 * SAIntervalTree.cpp:59-94 the single-read constructor, 173-237 validate(), 248-350 and 397-507 what they call) ------------------- */
/* What validate leaves of one read: merged (FMIndexWalkResult::merge) and, when it is set, the sequence's length; per walk status,
 * max_used_leaves and coverage as lrsc_fmwalk_result's and walk_length, the length of the walk's string (0: none); chosen = the
 * walk whose string is the sequence, or -1 when the sequence is the read itself or the read is not merged; read = kmerize, the
 * pieces and the main one as lrsc_fmwalk_kmerize leaves them (head 0, length the read's), whole = correctSequence is the read. */
typedef struct lrsc_fmwalk_validate_result { uint32_t merged, length; int32_t status[2]; uint32_t max_used_leaves[2]; uint64_t coverage[2]; uint32_t walk_length[2]; int32_t chosen /* 0, 1: that walk's string; -1: the read itself or none */; lrsc_fmwalk_read_result read; } lrsc_fmwalk_validate_result;
/* FMIndexWalkProcess::ValidateReads for n_reads single reads against the ctx's index, byte for byte the reference's serial run.
 * n = a read's length, m = min_overlap, k = kmer_length, T = kmer_threshold, which is the reference's `threshold`
 * (getRequiredSupport(0) - 1, the value of -x) as in lrsc_fmwalk_merge; max_insert is ignored.
 * 1. n <= m: no walk.  correctSequence is the read (whole = 1) and kmerize = !isLowComplexity(read), the float quotient against
 *    the double 0.9 (418-445).
 * 2. Otherwise two walks (SAIntervalTree::validate: mergeTwoReads without isTwoReadsOverlap, so the terminal is looked for only
 *    after the first extension and a read whose first and last m-mers are equal is still walked): walk 0 on the read, walk 1 on its
 *    reverse complement, each from the string's first m bases to its last m.  Depth limit (size_t)(n * 1.1), max overlap max_overlap
 *    or, for -1, (size_t)(n * 0.9), both in double arithmetic; max_leaves leaves; an extension needs T occurrences on both strands
 *    together.  Of a walk's results the one with the strictly greatest calculateKmerCoverage(.., m, pBWT) is its string; status 1,
 *    -1, -2, -3, -4 as lrsc_fmwalk_merge's.
 * 3. The decision (318-352), diffN = (double)lenN / n: only walk 0 has a string and walk 1's status is not -2: merged, the sequence
 *    is walk 0's string if diff0 >= 1, else the read; the same with the walks exchanged; both have a string: merged, walk 0's if
 *    diff0 >= 1, else walk 1's if diff1 >= 1, else the read.  Walk 1's string reads on the reverse strand and is given as it is.
 * 4. Everything else, "one string, but the other walk ran out of depth" included, is split: splitRead(std::string&) with the
 *    threshold (size_t)T - 1, unsigned (T = 1: 0, every k-mer qualifies; a T of 0, which this entry refuses, would wrap so that none
 *    does).  A k-mer qualifies by the sum of its occurrences and its reverse complement's (the reference's growing interval with its
 *    restarts gives that sum); a boundary p is examined unless k-mers p - 1 and p both qualify, and splits when
 *    !isSimple(k-mer p - 1, k-mer p, 1).  The main piece is the first piece with the strictly greatest span last - first, a span of
 *    0 never, and needs no solid k-mer.  kmerize is set when there is any piece; pieces of low complexity are dropped (kept = 0),
 *    the main one too, and correctSequence is then empty.  correctSequence is the main piece when it is kept, kmerizedReads are
 *    the other kept pieces in order.  Pieces and slots as lrsc_fmwalk_kmerize's.
 * 5. m < n < k: the reference asserts.  Here the walks run; a read they do not merge gives merged = 0, kmerize = 0, an empty
 *    sequence and no pieces.
 * merged + i * stride holds read i's sequence when it is merged and is not written otherwise.  LRSC_ERR_ARG as lrsc_fmwalk_merge
 * (max_insert apart), for fewer piece slots than the reads' k-mers and for a stride below (size_t)(1.1 * the longest read) + 1;
 * LRSC_ERR_UNSUPPORTED above the limits of lrsc_fmwalk_merge and when the longest string a read's walk can leave, (size_t)(n * 1.1)
 * + 1 bases, exceeds LRSC_FMWALK_MAX_INSERT (reads of up to 1818 bases are taken); LRSC_ERR_FORMAT when an interval leaves the
 * strand; on an error merged, out and pieces are untouched.  n_reads == 0 does nothing.  The launches are counted under
 * LRSC_K_FIND: one for the walks when a read is longer than m, one more when a read is split. */
int lrsc_fmwalk_validate(lrsc_ctx* ctx, const char* reads, const uint64_t* read_off, uint32_t n_reads, const lrsc_fmwalk_params* p /* max_insert ignored */,
                         char* merged /* n_reads * stride */, uint64_t stride, lrsc_fmwalk_validate_result* out, lrsc_fmwalk_piece* pieces, uint64_t n_piece_slots);

/* ---- exact irreducible read overlaps: `stride overlap` in its default mode (StriDe/overlap.cpp:126-413 without -e; Concurrency/
 * OverlapProcess.cpp:32-109; Algorithm/OverlapAlgorithm.cpp:22-44, 270-389, 419-487, 1043-1193, 1423-1444; Algorithm/OverlapBlock.cpp:
 * 40-70, 128-160, 182-360; BWTAlgorithms::initIntervalPair / updateBothL / updateBothR / getExtCount) ---- */
/* One final OverlapBlock of a read (Algorithm/OverlapBlock.h): lower..upper are the inclusive ranges.interval[0], rows of the '$'
 * interval, i.e. places in the lexicographic order of the reads (lrsc_index_lexico_order of LRSC_BWT, or of LRSC_RBWT when
 * target_rev); the AlignFlags; contained = the block is a containment (overlap_len is the read's length).  isTargetSubstring,
 * which the reference leaves uninitialised on this path, is 0 and not given. */
typedef struct lrsc_overlap_block { int64_t lower, upper; uint32_t overlap_len; uint8_t target_rev, query_rev, query_comp, contained; } lrsc_overlap_block;
/* OverlapResult of a read (Algorithm/OverlapAlgorithm.h) and its blocks[first_block .. first_block + n_blocks), in the order of
 * overlapReadExact's output list (OverlapAlgorithm.cpp:270-344).  status: 0, or LRSC_OVERLAP_OVERFLOW when the read's lists
 * outgrow the kernel's workspace (n_blocks is then 0). */
typedef struct lrsc_overlap_read { uint32_t is_substring, n_blocks, status, pad; uint64_t first_block; } lrsc_overlap_read;
#define LRSC_OVERLAP_OVERFLOW 1
/* The kernel's limits: LRSC_ERR_UNSUPPORTED above them. */
#define LRSC_OVERLAP_MAX_READ 2000
#define LRSC_OVERLAP_MAX_MIN_OVERLAP 2000
/* OverlapAlgorithm::overlapRead (OverlapAlgorithm.cpp:22-44) in exact mode with irreducible edges only, of n_reads reads (ASCII
 * bases back to back, n_reads + 1 offsets) against the ctx's index, which holds the same reads after `stride filter`.  A read
 * shorter than min_overlap has no blocks and is_substring 0.  The blocks of all reads stand in `blocks` in read order.
 * LRSC_ERR_ARG for min_overlap < 2, an empty read and a base other than A,C,G,T; LRSC_ERR_UNSUPPORTED above the limits;
 * LRSC_ERR_FORMAT when an interval leaves the strand (an index that is no BWT of a string set): on these the outputs are
 * untouched.  LRSC_ERR_CAPACITY when block_cap is too small: *n_blocks_out is then the number of blocks needed and nothing else
 * is written.  n_reads == 0 launches nothing.  Two launches per workspace chunk of reads, counted under LRSC_K_FIND; an interval
 * step is two of its rank_queries. */
int lrsc_overlap_exact(lrsc_ctx* ctx, const char* reads, const uint64_t* read_off, uint32_t n_reads, int32_t min_overlap,
                       lrsc_overlap_read* per_read, lrsc_overlap_block* blocks, uint64_t block_cap, uint64_t* n_blocks_out);

/* ---- unambiguous read merging: `stride fm-merge` (StriDe/fm-merge.cpp:60-221; Algorithm/FMMergeProcess.cpp:30-230 process, 233-251
 * checkCandidate, 253-310 addCandidates, 313-329 FMMergePostProcess; Algorithm/OverlapBlock.cpp:119-160 getEdgeDir, toOverlap;
 * Bigraph/Bigraph.cpp:162-220 merge, 452-524 simplify; Bigraph/Vertex.cpp:30-75 Vertex::merge) ---- */
/* A read's place: sequence `seq` holds it at `offset`, as its reverse complement when LRSC_FMMERGE_REVERSED.  A read with
 * LRSC_FMMERGE_DROPPED is used by sequence `seq` but absent from it (below), its offset is 0.  LRSC_FMMERGE_SELF_LINK: the only
 * block on one of its ends is the read itself, where the reference asserts; that end has no link. */
typedef struct lrsc_fmmerge_read { uint32_t seq, flags; uint64_t offset; } lrsc_fmmerge_read;
#define LRSC_FMMERGE_REVERSED 1
#define LRSC_FMMERGE_DROPPED 2
#define LRSC_FMMERGE_SELF_LINK 4
/* Sequence i, "merged-i": bases[offset .. offset + length), made of n_reads reads, on the forward strand of read `root`. */
typedef struct lrsc_fmmerge_seq { uint64_t offset, length; uint32_t n_reads, root, circular, pad; } lrsc_fmmerge_seq;
/* lrsc_fmmerge refuses more reads (LRSC_ERR_UNSUPPORTED): a node, 2 * read + end, is a 32-bit number.  Distances are 64 bits. */
#define LRSC_FMMERGE_MAX_READS 0x7FFFFFFFu
/* FMMergeProcess::process over all reads of the ctx's index at once: every run of reads that overlap unambiguously becomes one
 * sequence.  An end of a read (ED_SENSE for query_rev == 0, ED_ANTISENSE for query_rev == 1) has a link when exactly one final
 * non-containment block of lrsc_overlap_exact stands on it; the link is mutual when the target's end has exactly one block and
 * that block leads back.  Reads joined by mutual links form chains, paths or cycles, and a chain is merged along its overlaps.
 * Three things the reference leaves to the iteration order of a hash map, or to an assertion, are decided here:
 *   - a sequence reads on the forward strand of `root`, the chain's lowest-numbered read that is in the sequence; a cycle starts
 *     with that read whole and runs towards its sense end, once round, so it ends with the closing overlap (circular = 1).
 *     Sequences come in the order of their lowest-numbered used read.
 *   - a candidate that checkCandidate refuses stays red although the other arm of the search accepted it: where the end of a
 *     path links to the other end Q of the same path and Q's end there has several blocks (a cycle with a read leading into it
 *     at Q), Q is used but absent from the output: LRSC_FMMERGE_DROPPED.
 *   - an end whose only block is the read itself has no link: LRSC_FMMERGE_SELF_LINK.
 * n_reads must be the index's num_strings and the reads those of the index (LRSC_ERR_ARG); the lexicographic orders are
 * prepared as by lrsc_index_locate_prepare(rate 0) when the device has none.  LRSC_ERR_ARG "fm-merge requires `stride filter`
 * first" with the first such read when a block or a read's own interval has more than one row or a read is a substring;
 * LRSC_ERR_ARG when a read's own row is not in its interval (another index); LRSC_ERR_LIMIT when a read's overlap status is
 * LRSC_OVERLAP_OVERFLOW; LRSC_ERR_FORMAT when a read's blocks lie outside the pool; otherwise the errors of lrsc_overlap_exact.  On
 * all of these the outputs are untouched.  The four above show in a read's final blocks, so after the three launches of its chunk:
 * the call ends with the first chunk that shows one, without the overlap of the chunks behind it.  Everything else is refused before
 * the first launch.
 * LRSC_ERR_CAPACITY when bases_cap is too small: *n_bases_out is then the bases needed and nothing else is written.
 * per_read and seqs hold n_reads records.  n_reads == 0 launches nothing.
 * Launches, all counted under LRSC_K_FIND: 3 per chunk of reads (the overlap's two and the links), the chunk being
 * min(32768, 2^28 / (4 * (48 * (longest read - min_overlap) + 64)) rounded down to a multiple of 16) reads; then, with
 * R = ceil(log2(2 n)), the chain phase's 2 * (1 + R) + 1 (two rankings by pointer doubling over the 2 n (read, exit end) nodes, the
 * cut of cycles and dropped reads between them), 2 for the placement, 3 for the prefix sums and 1 for the bases: together
 * 3 * chunks + 2 * R + 9 (the last two are not made when bases_cap is too small).  No launch walks a chain link by link; the state
 * on the device is O(n_reads) beside the bases.  With LRSC_FMMERGE_PROFILE set in the environment the entry prints one line to
 * stderr, the kernels' milliseconds by phase (overlap, links, chains, place, assemble), as LRSC_BWT_PROFILE does for the index
 * entries; tools/fm_merge_rate.py reads it. */
int lrsc_fmmerge(lrsc_ctx* ctx, const char* reads, const uint64_t* read_off, uint32_t n_reads, int32_t min_overlap, lrsc_fmmerge_read* per_read,
                 lrsc_fmmerge_seq* seqs, uint32_t* n_seqs_out, char* bases, uint64_t bases_cap, uint64_t* n_bases_out);

/* ---- LongReadProbe k-mer feature grid -------------------------------------------------- */
/* reads: concatenated ACGT bytes, read_off: n_reads+1 offsets.  ks: ascending k-mer sizes
 * (the "pool", e.g. {5,9,15,17,19}), n_k <= 8.  For read r, position p, pool slot j the record
 * index is (read_off[r] + p) * n_k + j.
 *   out_iv[rec]      bi-interval of the KmerFeature (base slot by findBiInterval, larger slots by
 *                    expand(); KmerFeature.h:37-64,92-99)
 *   out_size[rec]    KmerFeature::size (shorter than ks[j] near the read end: "fake")
 *   out_count[rec*4] base-composition counters A,C,G,T accumulated during the search
 * Any of the three outputs may be NULL. */
int lrsc_kmer_grid(lrsc_ctx* ctx, const char* reads, const uint64_t* read_off, uint32_t n_reads,
                   const uint8_t* ks, uint32_t n_k,
                   lrsc_biinterval* out_iv, uint8_t* out_size, uint8_t* out_count);

/* ---- resident batches (inputs already in HBM; what bench.py times) ---------------------- */
typedef struct lrsc_batch lrsc_batch;
/* Upload a batch of reads to the ctx's device; validates ACGT. */
int lrsc_batch_create(lrsc_ctx* ctx, const char* reads, const uint64_t* read_off, uint32_t n_reads,
                      lrsc_batch** out);
void lrsc_batch_destroy(lrsc_batch* b);
/* Run the k-mer grid kernel over the whole resident batch, keeping results on the device
 * (compact per-position features only).  Timed internally with HIP events on the ctx stream. */
int lrsc_batch_kmer_grid(lrsc_ctx* ctx, lrsc_batch* b);

/* ---- LongReadProbe seeds ------------------------------------------------------------------ */
/* SeedFeature (PacBio/SeedFeature.h:35-45) as searchSeedsWithHybridKmers leaves it, i.e. after
 * estimateBestKmerSize and removeHitchhikingSeeds.  seedStr == read[start, start+len). */
typedef struct lrsc_seed {
    int32_t start;                /* seedStartPos (seedEndPos = start + len - 1) */
    int32_t len;                  /* seedLen                                      */
    int32_t max_fixed_mer_freq;   /* maxFixedMerFreq                              */
    int32_t is_repeat;            /* isRepeat                                     */
    int32_t start_best_kmer_size; /* startBestKmerSize                            */
    int32_t end_best_kmer_size;   /* endBestKmerSize                              */
    int32_t start_kmer_freq;      /* startKmerFreq                                */
    int32_t end_kmer_freq;        /* endKmerFreq                                  */
} lrsc_seed;
/* KmerThreshold table (PacBio/KmerThreshold.cpp:43-79) for `coverage`: out[mode*52 + k], mode 0..2, k 0..51. */
int lrsc_kmer_thresholds(int coverage, float* out);
/* The same table for k up to `end` (KmerThreshold::initialize(s, end, coverage, ""), e.g. `stride kmerfreq`: end = 100):
 * out[mode*(end+2) + k], k 0..end+1. */
int lrsc_kmer_thresholds_range(int coverage, int end, float* out);
/* Seeds of every read of a resident batch: k-mer grid, LongReadProbe::getSeqAttribute,
 * searchSeedsWithHybridKmers (PacBio/LongReadProbe.cpp:34-227), all on the device. */
int lrsc_batch_find_seeds(lrsc_ctx* ctx, lrsc_batch* b);
/* Copy the result of lrsc_batch_find_seeds to the host: seed_count[n_reads]; seeds (read order, then
 * position order; may be NULL) with capacity `cap` records; *n_seeds = total; attribute (optional) one
 * byte per base: 1 unique, 2 repeat (getSeqAttribute). LRSC_ERR_CAPACITY if cap is too small. */
int lrsc_batch_seeds(lrsc_ctx* ctx, lrsc_batch* b, uint32_t* seed_count, lrsc_seed* seeds, uint64_t cap,
                     uint64_t* n_seeds, int8_t* attribute);
/* Convenience: upload, find, fetch, release. */
int lrsc_find_seeds(lrsc_ctx* ctx, const char* reads, const uint64_t* read_off, uint32_t n_reads,
                    uint32_t* seed_count, lrsc_seed* seeds, uint64_t cap, uint64_t* n_seeds, int8_t* attribute);

/* ---- diagnostics of --debugseed / --onlyseed ---------------------------------------------------------------- */
/* What the reference writes per read under <out>/seed and <out>/extend when DebugSeed is set
 * (LongReadProbe.cpp:109-113,123-175,220-225; PacBioSelfCorrectionProcess.cpp:71-75,130-140).  Collection is off by
 * default and costs nothing then; switch it on for a batch BEFORE lrsc_batch_find_seeds. */
enum {
    LRSC_DEBUG_OUTCASTS = 1,   /* seeds dropped by removeHitchhikingSeeds        -> seed/error/<read>.seed */
    LRSC_DEBUG_WALKS    = 2,   /* FM walks that failed, DP fallbacks that failed -> extend/<read>.ext, .dp */
    LRSC_DEBUG_RATIO    = 4    /* getSeqAttribute's repeat ratio per position    -> extend/<read>.log      */
};
int lrsc_batch_set_debug(lrsc_batch* b, int flags);
/* Dropped seeds, laid out like lrsc_batch_seeds (initial-seed order within a read). */
int lrsc_batch_outcast_seeds(lrsc_ctx* ctx, lrsc_batch* b, uint32_t* outcast_count, lrsc_seed* seeds, uint64_t cap,
                             uint64_t* n_seeds);
/* ratio[total_bases]: the value getSeqAttribute compares with 0.02 (undefined for reads shorter than start_kmer_len). */
int lrsc_batch_repeat_ratio(lrsc_ctx* ctx, lrsc_batch* b, float* ratio);
/* After lrsc_batch_correct: one byte per seed in lrsc_batch_seeds order.  For seed i >= 1 of a read, 0 = the walk that
 * targets it succeeded by FM-extension (or it was skipped as a next-target); otherwise bits 0-3 = firstFMExtensionType + 4
 * (3 high error, 2 exceed depth, 1 exceed leaves) and bit 4 = the DP/MSA fallback failed too.  The walk's source is seed i-1. */
int lrsc_batch_walk_log(lrsc_ctx* ctx, lrsc_batch* b, uint8_t* log, uint64_t cap);

/* ---- seed-to-seed FM-extend ----------------------------------------------------------------------- */
/* One LongReadSelfCorrectByOverlap(sourceSeed, strBetweenSrcTarget, targetSeed, disBetweenSrcTarget,
 * initkmersize, maxOverlap, FM_params, min_SA_threshold).extendOverlap(result) call
 * (PacBio/LongReadCorrectByOverlap.cpp:17-95,155-211; built at PacBioSelfCorrectionProcess.cpp:186-190).
 * The three strings are ASCII ACGT, concatenated at seq + seq_off. */
typedef struct lrsc_walk_desc {
    uint64_t seq_off;
    uint32_t src_len;            /* sourceSeed length (>= init_kmer; its last init_kmer bases start the walk) */
    uint32_t path_len;           /* strBetweenSrcTarget length                                                */
    uint32_t trg_len;            /* targetSeed length                                                         */
    int32_t  dis;                /* disBetweenSrcTarget                                                       */
    uint32_t init_kmer;          /* initkmersize                                                              */
    uint32_t max_overlap;        /* maxOverlap                                                                */
    uint32_t min_sa_threshold;   /* min_SA_threshold                                                          */
    uint32_t pad;
} lrsc_walk_desc;
typedef struct lrsc_walk_result {
    int32_t  code;               /* extendOverlap's return value: 1, or -1 high error, -2 depth, -3 leaves, -4 */
    uint32_t steps;              /* iterations of the extension loop (accounting)                              */
    uint64_t out_off;            /* FMWalkResult2::mergedSeq at out_arena + out_off (code > 0 only)            */
    uint32_t out_len;
    uint32_t pad;
} lrsc_walk_result;
/* Runs n independent walks on the device.  out_arena receives the merged sequences back to back
 * (*arena_used bytes); LRSC_ERR_CAPACITY if arena_cap is too small (then *arena_used = bytes needed). */
int lrsc_extend_walks(lrsc_ctx* ctx, const char* seq, uint64_t seq_len, const lrsc_walk_desc* walks, uint32_t n,
                      lrsc_walk_result* results, char* out_arena, uint64_t arena_cap, uint64_t* arena_used);

/* ---- the whole per-read path ------------------------------------------------------------------------ */
/* PacBioSelfCorrectionResult (PacBio/PacBioSelfCorrectionProcess.h:58-94) without the wall-clock timers;
 * correctedStrs = pieces [piece_first, piece_first + n_pieces). */
typedef struct lrsc_read_result {
    int32_t  merge;              /* !pieceVec.empty(): record goes to correct.fa, else the raw read to discard.fa */
    uint32_t n_pieces;           /* 1, or more with --split                                                       */
    uint64_t piece_first;
    int64_t  total_reads_len, corrected_len, total_seed_num, total_walk_num, high_error_num, exceed_depth_num,
             exceed_leave_num, fm_num, dp_num, seed_dis;
    int32_t  status;             /* LRSC_READ_OK, or why this one read could not be corrected (the rest of the batch is unaffected):
                                  * the read then comes back uncorrected (merge = 0, no pieces, counters 0)                 */
    int32_t  pad;
} lrsc_read_result;
/* per-read status: an internal capacity of the device path was exceeded by this read alone.  The reference has no such
 * bounds (its containers grow); a caller that must not lose the read can route it to a CPU path. */
enum lrsc_read_status {
    LRSC_READ_OK = 0,
    LRSC_READ_WALK_QUERY_TOO_LONG = 1,   /* a walk's query (k-mer + gap between two seeds + target seed) >= 65535 bases  */
    LRSC_READ_TOO_LONG = 2,              /* the read's output slot would exceed 4 GB                                     */
    LRSC_READ_FRONTIER_LIMIT = 3,        /* more than 160 terminated lineages (5 x max_leaves above 32) in one walk      */
    LRSC_READ_GEOMETRY = 4,              /* seeds overlap / an extension k-mer above 59 or below the idmer size          */
    LRSC_READ_DP_LIMIT = 5,              /* DP fallback: a pile-up beyond its column / consensus capacity (a long query is not a
                                          * limit: alignments beyond the kernel's LDS stage run from a global workspace)   */
    LRSC_READ_OUTPUT_LIMIT = 6,          /* the corrected string outgrew its slot                                        */
    LRSC_READ_INTERNAL = 7               /* FM-extension returned a code the reference treats as impossible (it exits)   */
};
/* PacBioSelfCorrectionProcess::process for every read of the batch (PacBioSelfCorrectionProcess.cpp:23-245): seeds, the chain of
 * seed-to-seed FM-extensions, the DP/MSA fallback of correctByMSAlignment (unless params.no_dp) and the stitching, all on the
 * device, with the ctx's parameters.  Piece p is out[piece_off[p] .. piece_off[p+1]).
 * LRSC_ERR_CAPACITY (with *n_pieces / *out_used = what is needed) if piece_cap / out_cap are too small.  A read that exceeds a
 * per-read capacity does not fail the call: see lrsc_read_result.status. */
int lrsc_correct_reads(lrsc_ctx* ctx, const char* reads, const uint64_t* read_off, uint32_t n_reads,
                       lrsc_read_result* results, uint64_t* piece_off, uint64_t piece_cap, char* out, uint64_t out_cap,
                       uint64_t* n_pieces, uint64_t* out_used);
/* The same, for a batch that is already resident on the device (lrsc_batch_create): seeds, every seed-to-seed
 * walk of the batch at once from its predicted source k-mer, one DP round for the failed ones, and a per-read
 * stitch pass that replays initCorrect's chain and re-queues the walks whose source was not the predicted one
 * (bit-identical to running the chain in order) -- all on the device; only the corrected strings and the
 * counters come back.  lrsc_correct_reads is this call on a temporary batch. */
int lrsc_batch_correct(lrsc_ctx* ctx, lrsc_batch* batch, lrsc_read_result* results, uint64_t* piece_off,
                       uint64_t piece_cap, char* out, uint64_t out_cap, uint64_t* n_pieces, uint64_t* out_used);
int lrsc_ctx_get_params(const lrsc_ctx* ctx, lrsc_params* out);

/* ---- DP/MSA fallback: Overlapper::extendMatch ------------------------------------------------------------- */
/* One banded alignment (Thirdparty/overlapper.cpp:421-701): s1 = seq[s1_off .. +s1_len) (the query, DP columns),
 * s2 = seq[s2_off .. +s2_len) (DP rows); start1/start2 = the seed match that centres the band. */
typedef struct lrsc_dp_job {
    uint64_t s1_off, s2_off;
    uint32_t s1_len, s2_len;
    int32_t  start1, start2;
} lrsc_dp_job;
typedef struct lrsc_dp_result {      /* SequenceOverlap (Thirdparty/overlapper.h:69-125) */
    int32_t  match0_start, match0_end, match1_start, match1_end;
    int32_t  score, edit_distance, total_columns;
    uint32_t cigar_len;              /* EXPANDED cigar ('M','I','D' per column) at cigar_arena + cigar_off */
    uint64_t cigar_off;
} lrsc_dp_result;
/* n alignments on the device, one wavefront each.  LRSC_ERR_CAPACITY (with *arena_used = bytes needed) if
 * arena_cap is too small. */
int lrsc_dp_align(lrsc_ctx* ctx, const char* seq, uint64_t seq_len, const lrsc_dp_job* jobs, uint32_t n, int band_width,
                  int match_score, int gap_penalty, int mismatch_penalty, lrsc_dp_result* results, char* cigar_arena,
                  uint64_t arena_cap, uint64_t* arena_used);

/* ---- DP/MSA fallback: buildMultipleAlignment + calculateBaseConsensus ---------------------------------------- */
/* One correctByMSAlignment-style call (PacBio/LongReadOverlap.cpp:17-55 + Thirdparty/multiple_alignment.cpp:517-594):
 * query = seq[seq_off .. +len); reads overlapping its first / last kmer_len bases are retrieved from the index
 * (at most params.pb_coverage rows per interval), aligned to the query (band 200, +1/-1/-8), filtered by
 * min_overlap / min_identity, piled up and the base consensus (min_call_coverage, no trimming) is called. */
typedef struct lrsc_msa_query {
    uint64_t seq_off;
    uint32_t len, kmer_len;
    uint32_t min_overlap;
    int32_t  min_call_coverage;
    double   min_identity;
} lrsc_msa_query;
typedef struct lrsc_msa_result {
    uint32_t n_rows;             /* MultipleAlignment::getNumRows(): 1 + accepted overlaps                    */
    uint32_t n_retrieved;        /* strings LF-walked out of the index                                         */
    uint32_t cons_len;           /* consensus at arena + cons_off                                              */
    uint32_t rows_by_step_walk;  /* diagnostic: rows the kernel added one cigar step at a time (corner cases, or
                                    all of them with LRSC_MSA_BATCH=0) instead of in wavefront-wide passes          */
    uint64_t cons_off;
} lrsc_msa_result;
int lrsc_dp_consensus(lrsc_ctx* ctx, const char* seq, uint64_t seq_len, const lrsc_msa_query* queries, uint32_t n,
                      lrsc_msa_result* results, char* arena, uint64_t arena_cap, uint64_t* arena_used);

/* ---- DP/MSA fallback building blocks ------------------------------------------------------------------- */
/* LongReadOverlap::retrieveStr's LF-walks (PacBio/LongReadOverlap.cpp:696-749): job i starts at BWT row
 * rows[i] of strand[i] and emits at most max_steps[i] characters (stops at a '$' row).  Job i's characters
 * ("ACGT", in walk order) land at out + out_off[i]; out_len[i] receives how many. */
int lrsc_lf_walk(lrsc_ctx* ctx, const uint64_t* rows, const uint8_t* strand, const uint32_t* max_steps,
                 const uint64_t* out_off, uint64_t n, char* out, uint64_t out_cap, uint32_t* out_len);

/* ---- hash-guided seed-pair merge: SAIPBSelfCorrectTree ------------------------------------------------------ */
/* One job is one tree object of the reference (PacBio/SAIPBSelfCTree.h:140-287): the constructor's rawSeq, an ordered list of
 * addHashBySingleSeed calls (.cpp:704-787) and one mergeTwoSeedsUsingHash call (.cpp:91-256).  (The reference never instantiates
 * the class; its commented-out call site is PacBioHybridCorrectionProcess.cpp:1074-1130.)  Strings are ASCII ACGT spans of seq. */
typedef struct lrsc_saipb_seed {     /* addHashBySingleSeed(seedStr, largeKmerSize, job.hash_kmer, maxLength, skipRepeat, expectedLength) */
    uint64_t seq_off;
    uint32_t len;                /* seedStr length (>= large_kmer, >= the job's hash_kmer)                          */
    uint32_t large_kmer;         /* largeKmerSize                                                                   */
    uint32_t max_length;         /* maxLength                                                                       */
    int32_t  expected_length;    /* expectedLength, -1 = the default (source side)                                  */
    uint32_t skip_repeat;        /* skipRepeat                                                                      */
    uint32_t pad;
} lrsc_saipb_seed;
typedef struct lrsc_saipb_job {
    uint64_t raw_off;            /* rawSeq (not empty)                                                              */
    uint64_t src_off;            /* mergeTwoSeedsUsingHash's src                                                    */
    uint64_t dest_off;           /* ... and dest                                                                    */
    uint32_t raw_len, src_len, dest_len;   /* src_len, dest_len >= hash_kmer                                        */
    uint32_t seed_first, n_seeds;          /* the job's addHashBySingleSeed calls, in call order: seeds[seed_first ..) */
    uint32_t hash_kmer;          /* every seed's smallKmerSize and the merge's hashKmerSize, 2..31                  */
    uint32_t max_leaves;         /* maxLeaves, 1..64                                                                */
    uint32_t min_length, max_length, expected_length;
    uint32_t min_sa_threshold;   /* the constructor's min_SA_threshold                                              */
    uint32_t pad;
} lrsc_saipb_job;
typedef struct lrsc_saipb_result {
    int32_t  code;               /* mergeTwoSeedsUsingHash's return value: 1, or -1 .. -5 (0 when status != 0)      */
    int32_t  status;             /* LRSC_SAIPB_OK, or the per-job capacity this job alone outgrew: no numbers then  */
    uint32_t steps;              /* iterations of the extension loop                                                */
    uint32_t max_used_leaves;    /* widest frontier at the start of a step                                          */
    uint32_t n_results;          /* terminated lineages collected                                                   */
    uint32_t hash_entries;       /* distinct k-mers collected                                                       */
    uint64_t out_off;            /* mergedseq at out_arena + out_off (code 1 only)                                  */
    uint32_t out_len;
    uint32_t pad;
} lrsc_saipb_result;
enum lrsc_saipb_status {
    LRSC_SAIPB_OK = 0,
    LRSC_SAIPB_HASH_LIMIT = 1,     /* this job's workspace (mostly its k-mer table) would exceed the per-job limit
                                    * (LRSC_SAIPB_JOB_KB, in KiB, default 262144 = 256 MiB)                          */
    LRSC_SAIPB_RESULT_LIMIT = 2,   /* more than 32 terminated lineages                                              */
    LRSC_SAIPB_PATH_LIMIT = 3,     /* the path store / the child list of one step overflowed                        */
    LRSC_SAIPB_INTERNAL = 4
};
/* n_jobs independent jobs on the device, one wavefront each, in chunks that fit the workspace budget (LRSC_SAIPB_CHUNK_MB,
 * default 1024); seed_freq[i] (may be NULL) = what addHashBySingleSeed returns for seeds[i].  out_arena receives the merged
 * sequences back to back (*arena_used bytes); LRSC_ERR_CAPACITY if arena_cap is too small (then *arena_used = bytes needed).
 * LRSC_ERR_ARG where the reference would throw or divide by zero (a seed shorter than its large_kmer or than hash_kmer, src /
 * dest shorter than hash_kmer, an empty rawSeq); LRSC_ERR_UNSUPPORTED for hash_kmer outside 2..31, max_leaves outside 1..64, a
 * string or max_length beyond 32000 bases, or raw_len + max_length + dest_len beyond 65534 (the alignment's column count).
 * The merge launches are counted under LRSC_K_SAIPB (lrsc_ctx_stats). */
int lrsc_saipb_merge(lrsc_ctx* ctx, const char* seq, uint64_t seq_len, const lrsc_saipb_seed* seeds, uint32_t n_seeds,
                     const lrsc_saipb_job* jobs, uint32_t n_jobs, lrsc_saipb_result* results, uint64_t* seed_freq,
                     char* out_arena, uint64_t arena_cap, uint64_t* arena_used);

/* ---- measurement ------------------------------------------------------------------------- */
typedef struct lrsc_kernel_stats {
    uint64_t launches;          /* launches since the last reset                        */
    double   total_ms;          /* sum of HIP-event durations on the ctx stream          */
    uint64_t rank_queries;      /* Occ queries issued (algorithmic count)                */
    uint64_t block_loads;       /* rank-block loads (lower-1/upper in one block count 1) */
    uint64_t table_loads;       /* k-mer interval table look-ups (one 64-byte line each)  */
} lrsc_kernel_stats;
/* LRSC_K_EXTEND_WIDE: the wide walk launches of max_leaves above 32 (one per round with escalated walks; none at <= 32)
 * LRSC_K_SAIPB: lrsc_saipb_merge's merge launches, one per workspace chunk; total_ms spans a call's chunks together, the query
 *   counters are not kept for it
 * LRSC_K_LOCATE: lrsc_locate's launches; rank_queries = the LF steps taken */
enum { LRSC_K_RANK = 0, LRSC_K_FIND = 1, LRSC_K_GRID = 2, LRSC_K_SEEDS = 3, LRSC_K_EXTEND = 4, LRSC_K_LF = 5, LRSC_K_DP = 6, LRSC_K_MSA = 7,
       LRSC_K_EXTEND_WIDE = 8, LRSC_K_SAIPB = 9, LRSC_K_LOCATE = 10, LRSC_K_COUNT = 11 };
int lrsc_ctx_stats(lrsc_ctx* ctx, int kernel, lrsc_kernel_stats* out);
int lrsc_ctx_stats_reset(lrsc_ctx* ctx);
/* Block until everything queued on the ctx stream is done. */
int lrsc_ctx_sync(lrsc_ctx* ctx);

const char* lrsc_strerror(int status);
/* last detailed message for the calling thread (e.g. the HIP error string) */
const char* lrsc_last_error(void);
int lrsc_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif /* LRSC_H */
