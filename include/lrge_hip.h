/*
 * lrge_hip.h -- C ABI of the MI355X-native overlap engine (liblrge_hip.so).
 *
 * Drop-in boundary for liblrge's overlap hot path.  The reference crosses its FFI seam once per
 * read (mm_map); a GPU wants batches, so each entry point below replaces a *group* of reference
 * calls.  All functions return 0 on success or a negative LRGE_ERR_* code; the message for the
 * last failure on a context is returned by lrge_hip_last_error().  Caller owns every input and
 * output buffer; the library owns the ctx / seqset / index handles (free with *_free/_destroy).
 * No callee-allocated memory crosses the ABI.  A ctx serves one call at a time.
 *
 * Reference interfaces replaced (paths under /root/reference/liblrge/src):
 *   lrge_hip_ctx_create        <- ThreadLocalBuffer / mm_tbuf_init (minimap2/thread_buf.rs:7-42)
 *   lrge_hip_seqset_upload     <- the (name, seq) records fed to Aligner::map / the FASTA read by
 *                                 mm_idx_reader_read (twoset.rs:216-241, minimap2/aligner.rs:171-185)
 *   lrge_hip_index_build       <- AlignerWrapper::new -> Aligner::builder/preset/dual/with_index
 *                                 (minimap2/aligner.rs:310-328, :53-122, :144-197): mm_set_opt,
 *                                 mm_idx_reader_open/read/close, mm_mapopt_update
 *   lrge_hip_overlap_twoset    <- TwoSetStrategy::align_reads (twoset.rs:204-367): per-read
 *                                 Aligner::map (aligner.rs:204-303) + distinct-target counting
 *   lrge_hip_overlap_inverse   <- TwoSetStrategy::align_reads_inverse (twoset.rs:370-584)
 *   lrge_hip_overlap_ava       <- AvaStrategy::align_reads (ava.rs:165-366)
 *   lrge_hip_estimates         <- estimate::per_read_estimate (estimate.rs:142-157)
 *   lrge_hip_median            <- estimate::median + calculate_quantile (estimate.rs:80-132)
 *   lrge_hip_unique_random_set <- unique_random_set (lib.rs:189-204): StdRng::seed_from_u64 +
 *                                 rand::seq::index::sample (rand 0.9.4 / rand_chacha 0.9.0, Cargo.lock:1001-1029)
 *   lrge_hip_chains            <- the Vec<PafRecord> of Aligner::map (aligner.rs:244-291,
 *                                 minimap2/mapping.rs:10-54), batched
 */
#ifndef LRGE_HIP_H
#define LRGE_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* error codes map 1:1 onto LrgeError variants (error.rs:6-33) */
#define LRGE_OK                 0
#define LRGE_ERR_IO            -1  /* IoError */
#define LRGE_ERR_PARSE         -2  /* FastqParseError */
#define LRGE_ERR_TOO_MANY      -3  /* TooManyReadsError */
#define LRGE_ERR_TOO_FEW       -4  /* TooFewReadsError */
#define LRGE_ERR_DEVICE        -5  /* ThreadError class: HIP runtime / device failures */
#define LRGE_ERR_MAP           -6  /* MapError: "No index" / "Sequence is empty" (aligner.rs:210-216) */
#define LRGE_ERR_DUPLICATE_ID  -7  /* DuplicateReadIdentifier (ava.rs:195-199, twoset.rs:439-449) */
#define LRGE_ERR_PAF_WRITE     -8  /* PafWriteError */
#define LRGE_ERR_INVALID       -9  /* bad argument (no reference equivalent: would not compile in Rust) */
#define LRGE_ERR_UNPROVEN -10   /* the device cannot prove this input: take lrge_hip_read_records* (no reference equivalent) */

#define LRGE_PRESET_AVA_ONT 0   /* Preset::AvaOnt, "-k15 -Xw5 -e0 -m100 -r2k" (preset.rs:26) */
#define LRGE_PRESET_AVA_PB  1   /* Preset::AvaPb,  "-Hk19 -Xw5 -e0 -m100"     (preset.rs:24) */

typedef struct lrge_hip_ctx    lrge_hip_ctx;
typedef struct lrge_hip_seqset lrge_hip_seqset;
typedef struct lrge_hip_index  lrge_hip_index;
typedef struct lrge_hip_comm   lrge_hip_comm;

/* Builder knobs that reach the hot path (twoset/builder.rs:41-185, ava/builder.rs:38-153). */
typedef struct {
    int32_t remove_internal;     /* -F: drop overlaps the reference calls "internal" */
    float   max_overhang_ratio;  /* --max-overhang-ratio, default 0.2 (cli.rs:7) */
} lrge_hip_params;

/* One chain = one mm_reg1_t = one PafRecord (aligner.rs:253-290). */
typedef struct {
    uint32_t query;      /* index of the query read in its seqset */
    uint32_t target;     /* rid: index of the target read in the indexed seqset */
    int32_t  rev;        /* strand: 0 '+', 1 '-' */
    int32_t  score;      /* s1 */
    int32_t  cnt;        /* cm */
    int32_t  qs, qe;     /* query_start / query_end */
    int32_t  rs, re;     /* target_start / target_end */
    int32_t  mlen, blen; /* match_len / block_len */
    int32_t  n_seeds;    /* kept query seeds spanned by the chain: n_tot of mm_est_err before its two end
                            corrections; with cnt (= n_match) and the query's avg_k it gives dv */
} lrge_hip_chain;

/* Stage timings of the last overlap/index call on a ctx, in milliseconds (HIP event pairs recorded on the
   stream each stage runs on).  Index into the array with LRGE_T_*.  LRGE_T_CHAIN spans the whole chain stage
   (k_chain_hw beside k_chain_lpg, fork to join); LRGE_T_CHAIN_LPG is k_chain_lpg alone, on its side stream;
   LRGE_T_RS_SCATTER sums every k_rs_scatter launch of the call (they also count inside the sort stages). */
enum {
    LRGE_T_PACK = 0, LRGE_T_SKETCH, LRGE_T_INDEX_SORT, LRGE_T_INDEX_TABLE, LRGE_T_QFILTER,
    LRGE_T_LOOKUP, LRGE_T_EXPAND, LRGE_T_ANCHOR_SORT, LRGE_T_GROUP, LRGE_T_CHAIN,
    LRGE_T_CHAIN_GLB /* (unused: retired kernel) */, LRGE_T_COUNT, LRGE_T_TOTAL,
    LRGE_T_CHAIN_LPG, LRGE_T_RS_SCATTER, LRGE_T_K_LOOKUP /* k_lookup alone (it also counts inside LRGE_T_LOOKUP) */,
    LRGE_T_INDEX_RESTRICT /* lrge_hip_index_build_for: entry filter + global occurrence statistics */,
    LRGE_T_K_SKETCH /* the one-pass index sketch kernel alone (k_sketch_wave, or k_sketch_direct: see the two launch counters; they also count inside LRGE_T_SKETCH) */, LRGE_T_N
};
/* Work counters of the last overlap call (for the roofline's algorithmic bytes). */
enum {
    LRGE_C_QUERY_BASES = 0, LRGE_C_QUERY_MINIMIZERS, LRGE_C_ANCHORS, LRGE_C_GROUPS,
    LRGE_C_GROUPS_CHAINED, LRGE_C_CHAIN_LAUNCHES, LRGE_C_BATCHES,
    LRGE_C_CHAIN_ANCHORS /* anchors in chained groups */, LRGE_C_CHAIN_GLB_LAUNCHES, LRGE_C_CHAIN_GLB_ANCHORS,
    LRGE_C_LPG_LAUNCHES, LRGE_C_LPG_ANCHORS /* of those, anchors chained by k_chain_lpg */,
    LRGE_C_RS_SCATTER_LAUNCHES, LRGE_C_RS_SCATTER_ITEMS /* items moved by k_rs_scatter */,
    LRGE_C_RS_SCATTER_BYTES /* bytes those launches had to read + write: 32 per (key, value) pair, 16 per packed
                               key, 24 in the unpacking pass */,
    LRGE_C_LPG_SPLIT /* group size above which the last batch used k_chain_hw instead of k_chain_lpg */,
    LRGE_C_LOOKUP_LAUNCHES /* k_lookup launches (one per pass over a streamed set / index part) */,
    LRGE_C_TABLE_DISP_SUM /* last index build: sum over the distinct keys of their distance from the home slot in the ordered
                             table; divided by the number of keys it is ~0.5 at load 1/2 when the home slots are uniform */,
    LRGE_C_ANCHORS_KEPT /* of LRGE_C_ANCHORS (every seed hit expanded: minimap2's n_a), the anchors that left the expansion: the
                           dead-pair filter of count-only runs drops those of (target, strand) pairs too small to chain */,
    LRGE_C_INDEX_PARTS /* parts of the (partitioned) index the last overlap call went through, 0 = one index: LRGE_C_QUERY_MINIMIZERS and
                          LRGE_C_LOOKUP_LAUNCHES count every streamed minimizer once PER PART */,
    LRGE_C_SKETCH_LAUNCHES /* k_sketch_direct launches of the last index build / overlap call (LRGE_T_K_SKETCH) */,
    LRGE_C_SKETCH_WAVE_LAUNCHES /* k_sketch_wave launches (the wave-dense form of the index sketch; LRGE_T_K_SKETCH times whichever ran) */,
    LRGE_C_SHARED_NAME_PAIRS /* forward two-set against a partitioned index whose parts share target names: (query, name) pairs the parts
                                emitted for such names instead of counting them part by part; 0 when no name is shared across parts */,
    LRGE_C_SHARED_NAME_DISTINCT /* of those, the distinct ones: what the call added to the counts for names shared across parts */,
    LRGE_C_N
};

int  lrge_hip_device_count(int *n);
int  lrge_hip_ctx_create(int device, lrge_hip_ctx **out);
void lrge_hip_ctx_destroy(lrge_hip_ctx *ctx);
const char *lrge_hip_last_error(const lrge_hip_ctx *ctx);
/* Tuning / test options of a context (names and meanings: INTEGRATION.md section 6).  They are read from the environment
   exactly once, when the context is created (LRGE_HIP_<NAME>=value), and can be changed here afterwards; value NULL clears
   an option.  No entry point reads the environment per call.  The DEBUG_* options (fault injection, overrides of
   minimap2's chaining heuristics for the parity tests) are accepted through this call only, never from the environment. */
int  lrge_hip_ctx_set_option(lrge_hip_ctx *ctx, const char *name, const char *value);

/*
 * Upload a read set and pack it 2-bit (+ ambiguity mask) in HBM.
 *   bases     concatenated ASCII sequence bytes, offsets[n] bytes
 *   offsets   n+1 byte offsets into bases
 *   name_rank n lexicographic ranks of the read identifiers (header up to first whitespace,
 *             io.rs:199-204) computed over the UNION of all sets that will meet in one overlap
 *             call; equal names <=> equal rank.  Replaces strcmp(qname, tname) in minimap2's
 *             skip_seed and the name keys of liblrge's HashSet/HashMap.  NULL = all distinct.
 */
int  lrge_hip_seqset_upload(lrge_hip_ctx *ctx, const char *bases, const uint64_t *offsets,
                            uint32_t n, const uint32_t *name_rank, lrge_hip_seqset **out);
/*
 * The same without waiting for the transfer: the copy and the 2-bit pack are queued on the context's copy stream and the
 * call returns; every later call that consumes the set orders itself behind them on the device.  So a second set travels
 * over PCIe while the first one is being indexed (the reference's producer thread / bounded channel, twoset.rs:216-241,
 * does the same for its per-read stream).  `bases` may be
 *   - pinned host memory (lrge_hip_host_alloc, hipHostMalloc/hipHostRegister): one DMA straight from the caller's buffer,
 *     which must stay valid and unchanged until a call that consumes the set has returned or lrge_hip_seqset_wait(s);
 *   - pageable host memory: staged through the context's pinned buffers (copied out before the call returns);
 *   - device memory (reads already resident in HBM as ASCII): packed in place, no transfer.
 * `offsets` and `name_rank` are copied before the call returns in every case.  lrge_hip_seqset_upload accepts the same
 * three kinds of `bases`.
 */
int  lrge_hip_seqset_upload_async(lrge_hip_ctx *ctx, const char *bases, const uint64_t *offsets,
                                  uint32_t n, const uint32_t *name_rank, lrge_hip_seqset **out);
int  lrge_hip_seqset_wait(lrge_hip_seqset *s);          /* host-side wait for an async upload */
/* Pinned host memory for read buffers (what the record reader of io.rs:186-249 would fill): DMA source without staging. */
int  lrge_hip_host_alloc(size_t bytes, void **out);
void lrge_hip_host_free(void *p);
void lrge_hip_seqset_free(lrge_hip_seqset *s);
uint32_t lrge_hip_seqset_size(const lrge_hip_seqset *s);

/* Build the minimizer index over `targets` with the given preset (also fixes mid_occ). */
int  lrge_hip_index_build(lrge_hip_ctx *ctx, const lrge_hip_seqset *targets, int preset,
                          lrge_hip_index **out);
/*
 * The index of a multi-GPU run (and optionally of a single GPU): built for ONE streamed set.  It holds the entries of the
 * minimizers that occur in `streamed` -- complete position lists, so mm_idx_get answers every question that set can ask
 * exactly as the full index would -- while mid_occ, n_keys and n_minimizers are those of the whole target set
 * (mm_idx_cal_max_occ over all distinct keys).  Only `streamed` (or the library's own views of it) may be streamed against
 * it: the other overlap calls fail with LRGE_ERR_INVALID.
 *   comm == NULL  one GPU: the occurrence statistics are counted here.
 *   comm != NULL  collective call: every rank passes the SAME target set and ITS OWN range of the streamed reads; each rank
 *                 counts a 1/world share of the hash space and one small all-reduce completes the histogram.  No index
 *                 data crosses the links.
 * What it replaces: AlignerWrapper::new (aligner.rs:310-328) called once per process in a run sharded by query
 * (twoset.rs:266-334).  streamed == NULL and comm == NULL is lrge_hip_index_build.
 */
int  lrge_hip_index_build_for(lrge_hip_ctx *ctx, const lrge_hip_seqset *targets, int preset,
                              lrge_hip_seqset *streamed, lrge_hip_comm *comm, lrge_hip_index **out);
/*
 * The same index with the TARGET SKETCH sharded as well: a collective call in which every rank passes
 * ITS OWN contiguous share of the target reads -- reads [shard_first, shard_first + size(target_shard)) of the whole target
 * set, whose lengths and name ranks every rank knows (all_target_lens / all_target_ranks, n_targets entries; ranks may be
 * NULL) -- and its own range of the streamed reads.  Rank r sketches only its share; three exchanges complete the picture:
 * an all-gather of the ranks' key sets (Bloom filters), a variable-size all-to-all that sends every entry to the ranks whose
 * streamed reads carry its key (complete position lists wherever they are asked for), and one that sends every hash to the
 * rank that owns it for the occurrence statistics (one small all-reduce then fixes mid_occ, n_keys, n_minimizers globally).
 * The result answers the rank's streamed set exactly as the one index over all targets would.  The shares must be handed out
 * in rank order (rank 0 holds the first reads) so that position lists keep the order of the one index.
 * Replaces: AlignerWrapper::new (aligner.rs:310-328) in a run sharded by query (twoset.rs:266-334), with mm_idx_gen's
 * pipeline (mm2:index.c) itself spread over the ranks.
 */
int  lrge_hip_index_build_sharded(lrge_hip_ctx *ctx, const uint32_t *all_target_lens, const uint32_t *all_target_ranks,
                                  uint32_t n_targets, const lrge_hip_seqset *target_shard, uint32_t shard_first, int preset,
                                  lrge_hip_seqset *streamed, lrge_hip_comm *comm, lrge_hip_index **out);
/* The forward strategy over several GPUs with the TARGETS sharded (round 4; replaces, as the default multi-GPU form of
   twoset.rs:204-367, the query-sharded builds above -- those still stand).  Rank r indexes ITS contiguous share of the target
   reads (`target_shard`, uploaded on this context) and the caller maps ALL query reads against it with lrge_hip_overlap_twoset:
   the shards hold disjoint targets, so the per-query counts of the one index (aligner.rs:111-120) are the SUM of the ranks'
   counts (one lrge_hip_comm_allreduce_u32 of the count vector, and of has_mapping), bit for bit.  What is made global here is
   what mm_idx_cal_max_occ / mm_mapopt_update see (aligner.rs:189): every rank sends (hash, local count) per distinct key of its
   table to the hash's owner rank, the owners add up, one small all-reduce yields n_keys / n_minimizers / mid_occ of the whole
   target set (lrge_hip_index_stats reports those), and the keys above mid_occ are dropped in every rank's table.  No index entry
   crosses a link.  Collective: every rank of `comm` calls it; a failure on one rank fails it on all (the build ends with an
   agreement: no rank leaves with LRGE_OK alone).
   PRECONDITION the caller checks (it holds every target's name rank; lrge_amd/parallel.py: cross_shard_duplicates, the Rust shim):
   no target identifier occurs in two DIFFERENT shards -- or call lrge_hip_overlap_twoset_tsharded, which counts such a name once.
   The reference counts distinct target NAMES (twoset.rs:286-317) and never rejects a duplicate id in this mode; a duplicate inside
   one shard is counted once, one across shards would be counted once per shard by lrge_hip_overlap_twoset and the caller's sum.
   (The parts of a partitioned single-GPU index -- of one rank's share here as well -- have no such limit:
   lrge_hip_overlap_twoset counts a name its parts share once per query.) */
int  lrge_hip_index_build_tsharded(lrge_hip_ctx *ctx, const lrge_hip_seqset *target_shard, int preset, lrge_hip_comm *comm,
                                   lrge_hip_index **out);
/* Two-set forward over the ranks of a target-sharded world, whatever names the shards share: collective.  Every rank of `comm`
   calls it with the index lrge_hip_index_build_tsharded gave it on that communicator and with the SAME query set in the same order;
   on return every rank holds counts[] and has_mapping[] (0 / 1) of the WHOLE job -- the all-reduce that closes the step is inside.
   The result is what one index over all targets gives, bit for bit: the reference inserts target_name into a HashSet per query
   (twoset.rs:286-317), so a name borne by reads of two shards counts once.  The ranks find the names that occur in two or more
   shards (an all-gather of every shard's distinct name ranks); a kept mapping onto a bearer of such a name leaves a
   (query, name) pair instead of a count, the distinct pairs travel to the rank that owns the query (contiguous query ranges in
   rank order, one variable-size all-to-all) and are counted there once.  When no name is shared across shards nothing of this
   runs: the call is lrge_hip_overlap_twoset between two small all-gathers and the closing all-reduce.
   LRGE_C_SHARED_NAME_PAIRS: pairs this rank emitted; LRGE_C_SHARED_NAME_DISTINCT: distinct pairs this rank counted as owner.
   A failure on one rank fails the call on every rank (the call ends with an all-reduce that carries a status word; no rank is
   left waiting).  LRGE_ERR_INVALID, on every rank: `ix` belongs to another context or is not this communicator's target-sharded
   index on some rank, some shards were uploaded with name ranks and others without (NULL ranks = all distinct: shares nothing),
   the query sets differ in size.  ONE refusal cannot travel: a NULL `comm` or a `comm` of another context is LRGE_ERR_INVALID
   on that rank alone, before any collective (there is no communicator of this context to say it through) -- the caller MUST then
   call lrge_hip_comm_abort on the communicator its peers are using, or they wait in the first all-gather.  LRGE_ERR_TOO_MANY: 2^32
   pairs at one owner.  Inverse and all-vs-all keep LRGE_ERR_DUPLICATE_ID: the reference rejects duplicates there. */
int  lrge_hip_overlap_twoset_tsharded(lrge_hip_ctx *ctx, const lrge_hip_index *ix, const lrge_hip_seqset *queries,
                                      const lrge_hip_params *p, lrge_hip_comm *comm,
                                      uint32_t *counts, uint32_t *has_mapping);
/* Exchange volumes of the last lrge_hip_index_build_sharded on this context: {key-set bytes contributed, entries sketched here,
   entries sent to other ranks, entries received from other ranks, hashes sent, hashes received, bytes per entry | bytes per hash << 8
   (4 when the hash has at most 32 bits: k = 15), entries kept}. */
int  lrge_hip_last_shard_stats(const lrge_hip_ctx *ctx, uint64_t out[8]);
void lrge_hip_index_free(lrge_hip_index *ix);
int  lrge_hip_index_stats(const lrge_hip_index *ix, uint64_t *n_minimizers, uint64_t *n_keys,
                          int32_t *mid_occ);

/*
 * Two-set forward (dual = yes).  counts[q] = number of distinct target names among the kept
 * mappings of query q (twoset.rs:286-302); has_mapping[q] = 1 unless mappings.is_empty()
 * (twoset.rs:303-309).  Both arrays have lrge_hip_seqset_size(queries) entries.
 * A zero-length query is LRGE_ERR_MAP ("Sequence is empty").
 */
int  lrge_hip_overlap_twoset(lrge_hip_ctx *ctx, const lrge_hip_index *ix,
                             const lrge_hip_seqset *queries, const lrge_hip_params *p,
                             uint32_t *counts, uint32_t *has_mapping);
/*
 * Inverse two-set (--use-min-ref): `ix` indexes the QUERY set, `streamed` is the target set.
 * counts[i] (one per indexed read) += 1 for every streamed read with a kept mapping onto it
 * (twoset.rs:485-524).  Duplicate identifiers among the indexed reads: LRGE_ERR_DUPLICATE_ID.
 */
int  lrge_hip_overlap_inverse(lrge_hip_ctx *ctx, const lrge_hip_index *ix,
                              const lrge_hip_seqset *streamed, const lrge_hip_params *p,
                              uint32_t *counts);
/*
 * All-vs-all (dual = no): `reads` is the indexed set itself, or a SHARD of it (any subset, uploaded with name ranks
 * taken over the whole set; multi-GPU runs give every rank one shard).  counts[] has one entry per INDEXED read:
 * the symmetric overlap count (ava.rs:271-306) when `reads` is the whole set, this call's contribution to it
 * when it is a shard -- the sum over a partition of the reads is the all-vs-all result (NO_DUAL lets exactly one
 * read of every pair see it).  Duplicate identifiers: LRGE_ERR_DUPLICATE_ID.
 */
int  lrge_hip_overlap_ava(lrge_hip_ctx *ctx, const lrge_hip_index *ix,
                          const lrge_hip_seqset *reads, const lrge_hip_params *p,
                          uint32_t *counts);

/* Every chain of every query (the PafRecord stream), unordered.  *n_out receives the number of
   chains found; only the first `cap` are written.  dual: 1 = two-set flags, 0 = AVA flags. */
int  lrge_hip_chains(lrge_hip_ctx *ctx, const lrge_hip_index *ix, const lrge_hip_seqset *queries,
                     int dual, lrge_hip_chain *out, uint64_t cap, uint64_t *n_out);

/* Per-query seed statistics that complete the PafRecord tags (aligner.rs:262-270): rep_len = rl
   (query bases covered by seeds whose index occurrence exceeds mid_occ), and sum_span / n_kept, whose
   ratio (as f32) is mm_est_err's avg_k.  dv = n_match >= n_tot ? 0 : (float)(1.0 - pow((double)n_match /
   n_tot, 1.0 / avg_k)) with n_match = cnt and n_tot = n_seeds + [qs > avg_k && rs > avg_k] +
   [qlen - qs > avg_k && tlen - re > avg_k]  (mm2:esterr.c).  Arrays have one entry per query. */
int  lrge_hip_paf_stats(lrge_hip_ctx *ctx, const lrge_hip_index *ix, const lrge_hip_seqset *queries,
                        int32_t *rep_len, uint64_t *sum_span, uint32_t *n_kept);

/* overlaps.paf written on the device: the lines lrge::paf_lines (include/lrge_hip.hpp) formats on the host from
   lrge_hip_chains + lrge_hip_paf_stats, each with its line feed, byte for byte -- or nothing.  The statistics run once, the chains job
   runs with its records kept in HBM (chain_hint: room for that many records; 0: option PAF_CHAINS_FIRST, default 64, times the number
   of queries; a second run with the exact count when that was too few), every line is measured (dv code, its proof, the length), and
   the text is written in slices of at most option PAF_PIECE_BYTES (default 64 MiB) that reach `sink` one call per slice, whole lines
   each, in the run's record order (undefined, as in the reference).  q_names / q_name_off: the identifiers of `queries` back to back,
   uint64_t[n + 1] offsets; t_names / t_name_off: those of the indexed set.
   LRGE_ERR_UNPROVEN, nothing delivered: an identifier above option PAF_NAME_MAX_BYTES (default 1024; before any device work), or "dv of
   N lines not proven on the device" -- the host takes glibc's pow, the device its own, and a chain whose dv lies so close to a rounding
   boundary of "%.4f" that the two libraries' error bounds straddle it is not decided here: the caller writes lrge::paf_lines.
   LRGE_ERR_INVALID, before any device work: offsets that do not ascend, no sink.  LRGE_ERR_PAF_WRITE: the sink returned nonzero (what
   it took before is the caller's to discard).  No chains, or an empty set: LRGE_OK and the sink is never called.  A partitioned index
   and its refusals: as lrge_hip_chains; the records of ALL parts are held in one device buffer (48 bytes per chain of the whole call, not
   of one part) and the text is measured and written once, behind the last part -- not after every part -- because only so does an
   unproven chain of a later part still end the call with nothing delivered.
   Which model: dv follows lrge_amd/paf.py: chain_dv, whose n_tot and end differences are wide integers (64-bit here); lrge::paf_lines
   computes them in int.  The two agree on every record the chain kernels can produce (n_seeds + 2 and read lengths below 2^31); on
   others (tests feed INT32_MAX) the device gives the Python model's bytes.
   lrge_hip_last_paf_stats: {lines, text bytes, chain runs, slices, pieces handed to the sink, records held on the device, unproven
   chains, microseconds of measuring + writing + delivering}.
   BENCH ONLY, no part of what a caller needs (tools/paf_bench.py is their one user; they may change with it):
   lrge_hip_last_paf_phases, the host clock of the call in microseconds, {statistics, chains, measure, write (scan + kernel), waiting
   for copies, inside the sink, total, setup (device text blocks and pinned pieces taken)}; and option PAF_SERIAL, with which every
   slice is written, copied and delivered before the next is begun, so that the phases add up instead of overlapping (same bytes,
   same order, slower). */
int  lrge_hip_paf_text(lrge_hip_ctx *ctx, const lrge_hip_index *ix, const lrge_hip_seqset *queries, int dual,
                       const char *q_names, const uint64_t *q_name_off, const char *t_names, const uint64_t *t_name_off,
                       uint64_t chain_hint, int (*sink)(void *user, const void *bytes, uint64_t n), void *user);
int  lrge_hip_last_paf_stats(const lrge_hip_ctx *ctx, uint64_t out[8]);
int  lrge_hip_last_paf_phases(const lrge_hip_ctx *ctx, uint64_t out[8]);

/*
 * Multi-GPU: one context per GPU, every rank owns a range of the streamed reads end to end.  A
 * communicator carries the two exchanges of the path -- a SUM all-reduce of small integer vectors (the global
 * minimizer-occurrence histogram of lrge_hip_index_build_for; the per-indexed-read counts of the all-vs-all and inverse
 * strategies, ava.rs:300-301, twoset.rs:520-523) and an all-gather of the per-read estimates (the `estimates` vector of
 * twoset.rs:319-331).  Two transports:
 *   lrge_hip_comm_create        RCCL over xGMI, one PROCESS per GPU: rank 0 calls lrge_hip_comm_unique_id and hands the
 *                               128 bytes to the other ranks by whatever means the host has (a file, a socket, MPI,
 *                               torch.distributed's store); every rank then calls lrge_hip_comm_create collectively.
 *   lrge_hip_comm_create_local  the ranks are THREADS of one process (what a host that drives the GPUs from a thread
 *                               pool wants): buffers meet in host memory behind a barrier.  All ranks share one group
 *                               handle; collectives must be called by every rank, each from its own thread.
 * Collectives are blocking and must be entered by all ranks in the same order.  Host-buffer forms below; the library
 * itself uses the device forms inside lrge_hip_index_build_for.
 */
#define LRGE_HIP_COMM_ID_BYTES 128
int  lrge_hip_comm_unique_id(void *id128);
int  lrge_hip_comm_create(lrge_hip_ctx *ctx, int rank, int world, const void *id128, lrge_hip_comm **out);
int  lrge_hip_comm_local_group_create(int world, void **group);
void lrge_hip_comm_local_group_destroy(void *group);
int  lrge_hip_comm_create_local(lrge_hip_ctx *ctx, int rank, void *group, lrge_hip_comm **out);
/*   lrge_hip_comm_create_host   the host's own collectives (MPI, gloo, ...): the library stages its small vectors through host
 *                               memory and calls back.  allreduce: in-place SUM of n elements of elem_bytes (4: u32, 8: u64);
 *                               allgather: recv holds world * bytes; both return 0 on success. */
typedef int (*lrge_hip_host_allreduce_fn)(void *user, void *inout, size_t n, int elem_bytes);
typedef int (*lrge_hip_host_allgather_fn)(void *user, const void *send, size_t bytes, void *recv);
int  lrge_hip_comm_create_host(lrge_hip_ctx *ctx, int rank, int world, lrge_hip_host_allreduce_fn allreduce,
                               lrge_hip_host_allgather_fn allgather, void *user, lrge_hip_comm **out);
void lrge_hip_comm_destroy(lrge_hip_comm *c);
int  lrge_hip_comm_rank(const lrge_hip_comm *c);
int  lrge_hip_comm_world(const lrge_hip_comm *c);
int  lrge_hip_comm_allreduce_u32(lrge_hip_comm *c, uint32_t *inout, size_t n);                 /* in-place sum */
int  lrge_hip_comm_allgather(lrge_hip_comm *c, const void *send, size_t bytes, void *recv);    /* recv: world * bytes */
/* Variable-size all-to-all: this rank sends elements [send_off[d], send_off[d + 1]) of `send` to rank d and finds rank s's
   share at element recv_off[s] of `recv` (world + 1 prefix sums each, in elements of elem_bytes bytes; the receive counts are
   the other ranks' send counts -- exchange them with lrge_hip_comm_allgather first).  RCCL: one send / receive pair per
   peer in a group (point-to-point over xGMI); local groups copy device to device; host callbacks fall back to an all-gather.
   The exchange lrge_hip_index_build_sharded runs on device buffers. */
int  lrge_hip_comm_alltoallv(lrge_hip_comm *c, const void *send, const uint64_t *send_off, void *recv, const uint64_t *recv_off,
                             size_t elem_bytes);
/* Ranks RCCL itself counts in this communicator (ncclCommCount); 0 for the local / host transports. */
/* A rank that cannot go on between two collectives (a failed upload before a collective index build, a failed overlap call before
 * the all-reduce that closes the step) calls this instead of leaving its peers waiting for it: the reference's workers propagate a
 * MapError by ending the whole run (twoset.rs:279-284).  local: the group is aborted -- every rank blocked in, or later entering, one
 * of its collectives returns LRGE_ERR_DEVICE; RCCL: ncclCommAbort on this rank's communicator (its peers end with their own
 * processes: the launcher's job); host callbacks: the caller owns the collectives.  Afterwards every collective on c fails at once;
 * lrge_hip_comm_destroy is still to be called. */
int  lrge_hip_comm_abort(lrge_hip_comm *c);
int  lrge_hip_comm_rccl_ranks(const lrge_hip_comm *c, int *n);
/* librccl data-path calls (collectives, send / receive groups) made through c so far.  With LRGE_HIP_RCCL_WORLD1=1 (read when the RCCL
   communicator is created) a world of ONE goes through librccl for every collective instead of the world-1 shortcuts -- what lets a
   1-GPU box execute the RCCL branches with the shapes the sharded builds use (tests). */
int  lrge_hip_comm_rccl_ops(const lrge_hip_comm *c, uint64_t *n);
/* Timing emulation of a world on ONE GPU (local groups only): with serialize on, the ranks of the group take turns -- a rank
   computes between lrge_hip_comm_local_turn(c, 1) and (c, 0) and hands the GPU over whenever it waits for the others inside
   a collective; lrge_hip_comm_busy_ms returns the time it held the turn (what its share of the job takes on a GPU of its
   own, link transfers aside).  Results are unaffected.  on = 2: a rank that hands the GPU over also returns the idle segments of its
   device arena to the runtime (N arenas each sized for a whole GPU do not fit one), and the time inside the device allocator
   -- which a warm arena on a GPU of its own does not pay -- is kept out of busy_ms. */
int  lrge_hip_comm_local_group_serialize(void *group, int on);
int  lrge_hip_comm_local_turn(lrge_hip_comm *c, int begin);
double lrge_hip_comm_busy_ms(lrge_hip_comm *c, int reset);
/* (local groups) of that time, the part spent in the device-to-device copies that stand in for the link transfers of the
   variable-size all-gather (lrge_hip_seqset_presketch_sharded): on a node the links deliver into HBM and no copy is paid, so a
   projection takes busy - standin and adds the link model's time for the same bytes. */
double lrge_hip_comm_standin_ms(lrge_hip_comm *c, int reset);

/* per_read_estimate over n reads on the device (f32, no contraction). out[i] = +inf if counts[i]==0 */
int  lrge_hip_estimates(lrge_hip_ctx *ctx, const uint32_t *counts, const uint32_t *read_lens,
                        uint32_t n, float avg_target_len, uint64_t n_target_reads,
                        uint32_t overlap_thresh, float *out);
/* Host tail: median and optional quantiles of the (finite) estimates.  has_* mirror Option<f32>.
   out = {lower, median, upper}, ok[i] = 1 if that slot is Some. */
int  lrge_hip_median(const float *estimates, uint64_t n, int finite, int has_lower, float lower_q,
                     int has_upper, float upper_q, float out[3], int ok[3]);

/* Optional hint, results unchanged: sketch `s` ahead of the overlap call that will stream it.  The request is picked up
   by the NEXT lrge_hip_index_build on this context, which queues the set's sketch on a side stream right behind the
   index's own sketch, so that this VALU-bound work runs beside the index's memory-bound sort and table passes (mm_map
   sketches each query inside the call, mm2:map.c:mm_map_frag; here the set is known before the index exists).  The
   next lrge_hip_overlap_* call that streams `s` against an index of the same preset consumes the result (once); any
   other use simply sketches in line.  LRGE_HIP_NO_PRESKETCH=1 ignores the hint. */
int  lrge_hip_seqset_presketch(lrge_hip_ctx *ctx, lrge_hip_seqset *s, int preset);
/* The streamed set's sketch made ONCE per world instead of once per rank (round 6; the target-sharded forward strategy above has
   every rank map ALL queries, so every rank used to sketch all of them).  Collective: every rank of `comm` passes the SAME read set
   (same reads, same order: the ranks cut it by bases from the lengths they all hold); rank r runs mm_sketch (mm2:sketch.c, called per
   query by mm2:map.c collect_minimizers under Aligner::map, aligner.rs:231-241; twoset.rs:266-334 maps the queries independently of
   each other, so where a query is sketched is free) over its share only and the minimizers are all-gathered -- 16 bytes each, in read
   order, exactly the stream one rank's sketch of the whole set yields.  The result is attached to `s` like lrge_hip_seqset_presketch's
   and consumed (once) by the next lrge_hip_overlap_* call that streams `s` against an index of the same preset.  A failure on one rank
   fails the call on every rank (it ends with an agreement).  Sets of 2^32 bases or more: LRGE_ERR_TOO_MANY (they are streamed in views
   and sketched per view). */
int  lrge_hip_seqset_presketch_sharded(lrge_hip_ctx *ctx, lrge_hip_seqset *s, int preset, lrge_hip_comm *comm);

/* Host only: every record of an input file in any format liblrge accepts (io.rs:35-184: FASTA / FASTQ, SAM, unaligned BAM, unaligned
   CRAM 3.0; plain, gzip, bzip2, xz, zstd) through cb(user, name, name length, bases, base count) -- the C++ readers of
   include/lrge_io.hpp / lrge_cram.hpp behind a C entry point, for hosts that do not parse a format themselves.  A mapped record
   is refused with the reference's message (io.rs:162-167).  LRGE_ERR_IO: the file cannot be read; LRGE_ERR_PARSE: malformed
   input; the message goes to errbuf (may be NULL). */
int  lrge_hip_read_records(const char *path, void (*cb)(void *user, const char *name, uint64_t name_len, const char *bases, uint64_t n_bases),
                           void *user, char *errbuf, uint64_t errcap);

/* BGZF input decompressed on the device (k_inflate: one wavefront per block, CRC32 and ISIZE checked there).
   lrge_hip_bgzf_scan, host only: LRGE_OK when every gzip member of comp[0, comp_len) is a BGZF block (FEXTRA with a `BC`
   subfield, ISIZE <= 65536) and the blocks tile the buffer exactly; *n_blocks and *out_len (either may be NULL) receive the
   block count and the decompressed size.  Anything else (plain or multi-member gzip without BC, trailing bytes): LRGE_ERR_PARSE.
   lrge_hip_bgzf_inflate: every block into out[0, *out_len of the scan) (caller-owned, out_len at least that); a bad block is
   LRGE_ERR_PARSE and the message names its file offset; no host fallback.  Chunks of at most option INFLATE_CHUNK_BYTES
   (compressed + decompressed, default 256 MiB) are staged through pinned buffers, so device memory stays bounded.
   lrge_hip_read_records_gpu: the records, order and errors of lrge_hip_read_records; BGZF input is decompressed on the device,
   every other input -- and a file with a block the device rejects -- by the unchanged host path (its messages, through
   lrge_hip_last_error(ctx)).  *used_device (may be NULL): 1 if the device produced the bytes.  LRGE_ERR_DEVICE: a runtime failure. */
int  lrge_hip_bgzf_scan(const void *comp, uint64_t comp_len, uint64_t *n_blocks, uint64_t *out_len);
int  lrge_hip_bgzf_inflate(lrge_hip_ctx *ctx, const void *comp, uint64_t comp_len, void *out, uint64_t out_len);
int  lrge_hip_read_records_gpu(lrge_hip_ctx *ctx, const char *path,
                               void (*cb)(void *user, const char *name, uint64_t name_len, const char *bases, uint64_t n_bases),
                               void *user, int *used_device);

/* Plain and multi-member gzip decompressed on the device (speculative parallel inflate, DESIGN section 11: k_gz_find,
   k_gz_decode, k_gz_window, k_gz_resolve).  lrge_hip_gzip_inflate accepts any gzip buffer, BGZF included, and delivers the
   decompressed bytes in order through `sink` (a nonzero return stops the call with LRGE_ERR_IO).  On a non-OK return the bytes
   delivered so far are void.  Every member's CRC32 and ISIZE are checked, and the buffer must end exactly after the last
   member's trailer.  LRGE_ERR_PARSE: damaged or trailing data (the message names a file offset); LRGE_ERR_TOO_MANY: a chunk
   decodes to more than its slot holds even after one retry with 4x (option GZIP_SLOT_RATIO), callers take the host path;
   LRGE_ERR_DEVICE: a runtime failure.  Options GZIP_CHUNK_BYTES (default 512 KiB) and GZIP_ROUND_BYTES (default 256 MiB)
   set the nominal chunk and the compressed bytes per round.  *stats (may be NULL) receives the counts of the call.
   lrge_hip_read_records_gpu_ex: lrge_hip_read_records_gpu with a choice of device paths.  LRGE_GPU_INFLATE_BGZF reproduces
   lrge_hip_read_records_gpu; | LRGE_GPU_INFLATE_GZIP also sends every other gzip input to lrge_hip_gzip_inflate (BGZF keeps
   k_inflate).  Anything the device cannot prove falls back to the unchanged host path and its messages. */
typedef struct lrge_hip_gzip_stats {
    uint64_t members;            /* gzip members whose CRC32 and ISIZE were checked */
    uint64_t chunks;             /* nominal chunks over all rounds */
    uint64_t speculative_starts; /* chunks decoded from a finder candidate (not a round's first) */
    uint64_t rejected_starts;    /* candidates the chain walk rejected */
    uint64_t redecoded_chunks;   /* chunks decoded again from their predecessor's true end */
    uint64_t overflow_retries;   /* chunks decoded again with a 4x slot */
    uint64_t bytes_out;          /* decompressed bytes */
} lrge_hip_gzip_stats;
#define LRGE_GPU_INFLATE_BGZF 1
#define LRGE_GPU_INFLATE_GZIP 2
int  lrge_hip_gzip_inflate(lrge_hip_ctx *ctx, const void *comp, uint64_t comp_len, int (*sink)(void *user, const void *bytes, uint64_t n),
                           void *user, lrge_hip_gzip_stats *stats);
int  lrge_hip_read_records_gpu_ex(lrge_hip_ctx *ctx, const char *path, int flags,
                                  void (*cb)(void *user, const char *name, uint64_t name_len, const char *bases, uint64_t n_bases),
                                  void *user, int *used_device);

/* bzip2 decompressed on the device (k_bz_find, k_bz_decode, k_bz_scatter, k_bz_walk, k_bz_rle_count,
   k_bz_rle_write): the blocks of one stream are found by their 48-bit magic at every bit offset and decoded in parallel; a chain
   from bit 32 accepts a block only where the block in front of it ended.  lrge_hip_bzip2_inflate has the contract of
   lrge_hip_gzip_inflate: the bytes arrive in order through `sink` (a nonzero return stops the call with LRGE_ERR_IO); on a non-OK
   return the bytes delivered so far are void; there is no host fall-back inside the call.  The device accepts exactly what the
   host reader takes, the first stream: one header "BZh1".."BZh9", blocks, the end-of-stream magic, a correct combined CRC, at most
   7 padding bits and nothing behind them.  LRGE_ERR_PARSE (the message names a byte offset): a second stream or any trailing
   byte, a randomised block, nGroups outside 2..6, a selector or a code length out of range, more bytes than the level's block
   size, origPtr outside the block, a missing end-of-block symbol, a block that stops behind four equal bytes where their count belongs, a wrong block or stream
   CRC, a truncated file.
   LRGE_ERR_DEVICE: a runtime failure.  Option BZIP2_ROUND_BLOCKS: candidates decoded per round (default: what half of the free
   device memory plus the context's idle arena bytes holds, at most 4096).  *stats (may be NULL) receives the counts of the call.
   lrge_hip_read_records_gpu_ex | LRGE_GPU_INFLATE_BZIP2 sends bzip2 input to this decoder and falls back to the unchanged host
   path for anything it does not accept; lrge_hip_reads_open* | LRGE_GPU_INFLATE_BZIP2 keeps the text in HBM. */
typedef struct lrge_hip_bzip2_stats {
    uint64_t blocks;              /* accepted blocks, each with its CRC checked */
    uint64_t candidates;          /* bit offsets that carry the block magic */
    uint64_t rejected_candidates; /* candidates the chain did not arrive at */
    uint64_t rounds;              /* rounds of at most BZIP2_ROUND_BLOCKS candidates */
    uint64_t bytes_out;           /* decompressed bytes */
} lrge_hip_bzip2_stats;
#define LRGE_GPU_INFLATE_BZIP2 16
int  lrge_hip_bzip2_inflate(lrge_hip_ctx *ctx, const void *comp, uint64_t comp_len, int (*sink)(void *user, const void *bytes, uint64_t n),
                            void *user, lrge_hip_bzip2_stats *stats);

/* Zstandard decompressed on the device (k_zs_heads, k_zs_literals, k_zs_sequences, k_zs_execute, k_zs_resolve,
   k_zs_xxh64): the host hops over frame and block headers; the blocks of a round are entropy-decoded in parallel, every table
   rebuilt from the block that states it; the round's blocks are executed at once, a byte whose source lies in front of its block
   is recorded and read once the blocks in front are final; a frame's content checksum is XXH64 over its text.
   lrge_hip_zstd_inflate has the contract of lrge_hip_bzip2_inflate: the bytes arrive in order through `sink` (a nonzero return
   stops the call with LRGE_ERR_IO); on a non-OK return the bytes delivered so far are void; there is no host fall-back inside the
   call.  The device accepts a subset of what the host reader takes, and returns the same bytes: one or more frames back to back,
   skippable frames between them, with or without Frame_Content_Size, window descriptor and checksum; raw, RLE and compressed
   blocks; every literals type and sequence mode.  LRGE_ERR_PARSE (the message names a byte offset): a dictionary ID other than 0,
   a reserved bit, block type 3, a block or its output above Block_Maximum_Size, a window above 2^27 bytes, an accuracy log above
   the format's limits, Huffman weights that do not sum to a power of two, a bitstream that is not consumed exactly, treeless
   literals or a repeat mode with nothing in front of it in the frame, too few literals, an offset of 0, beyond the frame's bytes
   or beyond the window, a content-size mismatch, a wrong checksum, a truncated file, bytes behind the last frame.
   LRGE_ERR_TOO_MANY: the text of the call does not fit the device budget (the default of INGEST_MAX_BYTES: half of the free device
   memory plus the context's idle arena bytes; the text stays on the device until the call ends, because a match may reach back
   through the whole frame); the caller takes the host.  LRGE_ERR_DEVICE: a runtime failure.  Options ZSTD_ROUND_BLOCKS: blocks
   decoded per round (default: what half of the free device memory plus the idle arena bytes holds, at most 4096); ZSTD_CHECKSUM
   (default 1): 0 skips the checksums.  *stats (may be NULL) receives the counts of the call.
   lrge_hip_read_records_gpu_ex | LRGE_GPU_INFLATE_ZSTD sends Zstandard input to this decoder and falls back to the unchanged host
   path for anything it does not accept; lrge_hip_reads_open* | LRGE_GPU_INFLATE_ZSTD keeps the text in HBM.  Known limit: zstd
   input is never windowed -- LRGE_GPU_INGEST_WINDOWED leaves it resident, and text above INGEST_MAX_BYTES is LRGE_ERR_UNPROVEN. */
typedef struct lrge_hip_zstd_stats {
    uint64_t frames;              /* Zstandard frames */
    uint64_t skippable_frames;    /* skippable frames hopped over */
    uint64_t blocks;              /* blocks of every type */
    uint64_t raw_blocks;
    uint64_t rle_blocks;
    uint64_t sequences;           /* Number_of_Sequences summed over the compressed blocks */
    uint64_t checksums_checked;   /* frames whose content checksum was computed and compared (0 with ZSTD_CHECKSUM=0) */
    uint64_t rounds;              /* rounds of at most ZSTD_ROUND_BLOCKS blocks */
    uint64_t bytes_out;           /* decompressed bytes */
    uint64_t checksum_us;         /* microseconds spent in k_zs_xxh64, launch to result */
} lrge_hip_zstd_stats;
#define LRGE_GPU_INFLATE_ZSTD 128
int  lrge_hip_zstd_inflate(lrge_hip_ctx *ctx, const void *comp, uint64_t comp_len, int (*sink)(void *user, const void *bytes, uint64_t n),
                           void *user, lrge_hip_zstd_stats *stats);

/* xz decompressed on the device (k_xz_decode, k_xz_check): the host walks the stream footers, the indexes, the
   block headers and the LZMA2 chunk headers, which gives every block's place in the text before a byte is decoded and verifies
   the whole container; the blocks of a round are decoded at once, one wavefront per block, the adaptive range decoder serial
   inside a block; a block's check is CRC32 or CRC64 over its text.
   lrge_hip_xz_inflate has the contract of lrge_hip_zstd_inflate: the bytes arrive in order through `sink` (a nonzero return stops
   the call with LRGE_ERR_IO); on a non-OK return the bytes delivered so far are void; there is no host fall-back inside the call.
   The device accepts a subset of what the host reader takes (liblzma with LZMA_CONCATENATED), and returns the same bytes: one or
   more streams, stream padding in multiples of four bytes between and behind them, streams of no block, block headers with or
   without the size fields, the filter chain of LZMA2 alone at any dictionary size, the checks none, CRC32 and CRC64, every LZMA2
   control byte.  LRGE_ERR_PARSE (`xz data at file offset N: <status name>`): another filter or more than one, a SHA-256 or
   reserved check, reserved bits, a wrong header, footer, index or block header CRC32, flags that differ, a bad index or padding,
   sizes that do not agree, a first chunk without a dictionary reset, an LZMA chunk with no properties in force, lc + lp > 4, a
   distance beyond the dictionary or its size, the end marker, a match that crosses its chunk, a range decoder whose first byte is
   not 0 or that does not end with code 0 exactly at the chunk's compressed size, a wrong check, truncation, bytes that are neither
   a stream nor padding, fewer blocks than XZ_MIN_BLOCKS.  LRGE_ERR_TOO_MANY: the text of one round does not fit the device budget
   (half of the free device memory plus the context's idle arena bytes); the caller takes the host.  LRGE_ERR_DEVICE: a runtime
   failure.  Options XZ_ROUND_BLOCKS: blocks decoded per round (default: what half of the free device memory plus the idle arena
   bytes holds, at most 4096); XZ_LAUNCH_BYTES: the text a block may produce per kernel launch, in whole chunks, one chunk at
   least (default 2 MiB, the format's largest chunk, so no launch runs longer than one chunk per wavefront); XZ_CHECK (default 1):
   0 skips the block checks; XZ_MIN_BLOCKS (default 64, the measured
   break-even against liblzma on one thread: BASELINE section 13): a file with fewer blocks is refused.  *stats (may be NULL) receives the
   counts of the call.  lrge_hip_read_records_gpu_ex | LRGE_GPU_INFLATE_XZ sends xz input to this decoder and falls back to the
   unchanged host path for anything it does not accept; lrge_hip_reads_open* | LRGE_GPU_INFLATE_XZ keeps the text in HBM, and with
   LRGE_GPU_INGEST_WINDOWED every finished round passes through the windows (a block needs no earlier text).  Not verified: text
   of 4 GiB or more. */
typedef struct lrge_hip_xz_stats {
    uint64_t streams;             /* .xz streams */
    uint64_t blocks;              /* blocks decoded */
    uint64_t chunks;              /* LZMA2 chunks of the file */
    uint64_t raw_chunks;          /* of them uncompressed chunks */
    uint64_t checks_checked;      /* blocks whose CRC32 / CRC64 was computed and compared (0 with XZ_CHECK=0) */
    uint64_t rounds;              /* rounds of at most XZ_ROUND_BLOCKS blocks */
    uint64_t launches;            /* launches of k_xz_decode */
    uint64_t bytes_out;           /* decompressed bytes */
    uint64_t check_us;            /* microseconds spent in k_xz_check, launch to result */
    uint64_t decode_us;           /* microseconds spent in k_xz_decode, launch to result */
    uint64_t walk_us;             /* microseconds of the host's walk over the container */
} lrge_hip_xz_stats;
#define LRGE_GPU_INFLATE_XZ 256
int  lrge_hip_xz_inflate(lrge_hip_ctx *ctx, const void *comp, uint64_t comp_len, int (*sink)(void *user, const void *bytes, uint64_t n),
                         void *user, lrge_hip_xz_stats *stats);

/* Read sets built on the device from FASTA / FASTQ text (k_fx_census, k_fx_summary, k_fx_scatter, k_fx_records,
   k_fx_names, k_fx_gather) and from unaligned BAM (k_bam_header, k_bam_find, k_bam_walk, k_bam_records,
   k_bam_gather; SAM, DESIGN section 14: k_sam_mark, k_sam_records): the device-side form of the record reader (io.rs:154-184) and of the read selection that feeds the
   strategies (twoset.rs:122-201).  The file's bytes are decompressed into HBM and stay there; the records are found there; only
   the identifiers and the sequence lengths come back.
   lrge_hip_reads_open (io.rs:154-184) reads `path` into memory and calls lrge_hip_reads_open_mem (io.rs:154-184), which takes the
   bytes of a whole file.  `flags`: LRGE_GPU_INFLATE_BGZF | LRGE_GPU_INFLATE_GZIP | LRGE_GPU_INFLATE_BZIP2 | LRGE_GPU_INFLATE_ZSTD | LRGE_GPU_INFLATE_XZ choose the device decoders as in
   lrge_hip_read_records_gpu_ex; with neither, only uncompressed input is taken.  | LRGE_GPU_INGEST_BAM: text that starts with
   the BAM magic is scanned as unaligned BAM (every record with flag 4, found by a speculative walk of the length chain that
   is proven from the end of the header); without the flag BAM is unproven, as it was before the flag existed.
   | LRGE_GPU_INGEST_SAM: text that starts with "@HD", "@SQ" or "@RG" is scanned as unaligned SAM (every line that is neither
   empty nor starts with '@' has ten tabs and a flag of 1 to 9 digits with bit 2 set); without the flag SAM is unproven.  The records
   equal those of lrge_hip_read_records on the same file, one for one.  LRGE_ERR_UNPROVEN: the device does not prove this input
   and produces no parse error of its own -- anything but FASTA, strict four-line FASTQ or (with its flag) well-formed unaligned
   BAM (an empty line between records, a truncated record, a missing '+', CRAM without LRGE_GPU_INGEST_CRAM or in a layout that flag does not prove (below), BAM without LRGE_GPU_INGEST_BAM, a BAM
   with a mapped record, a damaged header or record, or bytes behind the last record, SAM without LRGE_GPU_INGEST_SAM, a SAM
   record line with fewer than ten tabs, with a flag that is not plain digits or with a mapped flag), a compressed format without its flag or other than gzip, (with LRGE_GPU_INFLATE_BZIP2) bzip2, (with LRGE_GPU_INFLATE_ZSTD) Zstandard and (with LRGE_GPU_INFLATE_XZ) xz, a damaged gzip file, a bzip2, Zstandard or xz file the device decoder does not accept, text above option INGEST_MAX_BYTES
   (default: half of the free device memory plus the context's idle arena bytes); the caller takes lrge_hip_read_records*, which
   parses the file or gives the reference's message.  LRGE_ERR_TOO_MANY: 2^32 records or more, or a sequence of 2^32 bases or
   more.  LRGE_ERR_IO: the file cannot be read.  An empty file is LRGE_OK with a count of 0.
   | LRGE_GPU_INGEST_WINDOWED (k_fx_store): FASTA / FASTQ text larger than option INGEST_WINDOW_BYTES (default 1 GiB,
   at most a quarter of INGEST_MAX_BYTES) passes through HBM in windows that are cut between records, and only the bases stay, dense
   and in file order; INGEST_MAX_BYTES then bounds the bases plus the window, so a FASTQ about twice the cap can be taken.  The
   records are those of the resident scan and of lrge_hip_read_records, or the call is LRGE_ERR_UNPROVEN (a window the scan does
   not prove, a window of another format than the first, a window of 2^32 bytes or more, 2^32 records or 4 GiB of identifiers in
   all); for text that is not well formed (empty
   lines between records) the verdict may depend on the window.  Text within one window, BAM and SAM stay resident as without the flag; so does Zstandard text of any size without LRGE_GPU_INGEST_WINDOWED_ZSTD (below).
   | LRGE_GPU_INGEST_WINDOWED_ALN (k_bam_spans, k_bam_store; effective only beside LRGE_GPU_INGEST_WINDOWED and the
   format's own flag): unaligned BAM and SAM above INGEST_WINDOW_BYTES pass through in windows too.  A BAM window is cut at the
   first record start of the chain proven from its front that the block does not hold whole, a SAM window directly behind its
   last line feed.  BAM's bases stay packed as the file has them, 4 bits each, (l_seq + 1) / 2 bytes a record; SAM's stay as
   ASCII.  The same outcomes: the records of lrge_hip_read_records, or LRGE_ERR_UNPROVEN for the whole call (a mapped record in
   any window leaves no earlier record behind).
   lrge_hip_reads_count / _name_bytes / _text_bytes (io.rs:154-184): records, total identifier bytes, decompressed bytes (all
   that was scanned, whether or not it stayed).
   lrge_hip_reads_window_stats (io.rs:154-184): out[0] windows flushed (0: the text stayed resident), out[1] bytes in the store (the
   bases for FASTA / FASTQ / SAM, the packed bytes of the records for BAM), out[2] the largest window in bytes, out[3] bytes
   carried over cuts into the next window.
   lrge_hip_reads_table (io.rs:154-184): seq_len[n], name_off[n + 1] and the identifiers back to back in names[name_bytes]
   (identifier i is names[name_off[i], name_off[i + 1]); any of the three may be NULL).
   lrge_hip_reads_timings (io.rs:154-184): milliseconds of the open call -- text to HBM, record scan, identifiers and lengths to the
   host, total (for BAM the record scan covers the candidate search, the walks, the repair rounds and the table).
   lrge_hip_reads_bam_stats (io.rs:154-184): the counts of the BAM record scan of `reads` (option BAM_SEGMENT_BYTES, default 256 KiB,
   at least 64, sets the segment), for a windowed handle summed over its windows (the segments of a window start at its front,
   and those behind its cut do not count); LRGE_ERR_INVALID when `reads` was not scanned as BAM.
   lrge_hip_seqset_from_reads (twoset.rs:122-201): reads idx[0..n) of `reads`, in that order (any order, repeats allowed; an entry
   out of range is LRGE_ERR_INVALID), as an ordinary read set: their bases are gathered on the device and packed by the
   device-source path of lrge_hip_seqset_upload, so the set is bit-identical to an upload of the same sequences.  name_rank as
   there.  The handle must outlive the call only; lrge_hip_reads_free (io.rs:154-184) releases the text. */
typedef struct lrge_hip_reads lrge_hip_reads;
typedef struct lrge_hip_bam_stats {
    uint64_t segments;           /* segments of BAM_SEGMENT_BYTES the records area was cut into */
    uint64_t empty_segments;     /* segments no record starts in: a record spans them */
    uint64_t speculative_starts; /* segments behind the first that were walked from a candidate of the finder */
    uint64_t rejected_starts;    /* candidates the chain from the header did not reach */
    uint64_t repair_rounds;      /* rounds of walks from the landing of the segment in front */
    uint64_t rewalked_segments;  /* segments walked in those rounds */
} lrge_hip_bam_stats;
#define LRGE_GPU_INGEST_BAM 4
#define LRGE_GPU_INGEST_SAM 8
#define LRGE_GPU_INGEST_WINDOWED 32
#define LRGE_GPU_INGEST_WINDOWED_ALN 64
int      lrge_hip_reads_open(lrge_hip_ctx *ctx, const char *path, int flags, lrge_hip_reads **out);
int      lrge_hip_reads_open_mem(lrge_hip_ctx *ctx, const void *file_bytes, uint64_t len, int flags, lrge_hip_reads **out);
uint64_t lrge_hip_reads_count(const lrge_hip_reads *reads);
uint64_t lrge_hip_reads_name_bytes(const lrge_hip_reads *reads);
uint64_t lrge_hip_reads_text_bytes(const lrge_hip_reads *reads);
int      lrge_hip_reads_table(const lrge_hip_reads *reads, uint32_t *seq_len, uint64_t *name_off, char *names);
int      lrge_hip_reads_timings(const lrge_hip_reads *reads, float ms[4]);
int      lrge_hip_reads_bam_stats(const lrge_hip_reads *reads, lrge_hip_bam_stats *out);
int      lrge_hip_reads_window_stats(const lrge_hip_reads *reads, uint64_t out[4]);
int      lrge_hip_seqset_from_reads(lrge_hip_ctx *ctx, const lrge_hip_reads *reads, const uint32_t *idx, uint32_t n,
                                    const uint32_t *name_rank, lrge_hip_seqset **out);
void     lrge_hip_reads_free(lrge_hip_reads *reads);

/* The device ingest of a sample (k_fx_bases, k_fx_pick, k_fx_keep): the tool never uses more than a sample of
   its input, so the reference reads the file twice -- count_records (io.rs:140-145) gives n, unique_random_set (lib.rs:189-204)
   draws the indices, and a second pass writes only the drawn reads (twoset.rs:122-201).  These entries are the two passes on the
   device, for FASTA / FASTQ text from every source whose text passes through windows (plain, BGZF, gzip, bzip2, xz).  In both the
   whole text goes through the windows of INGEST_WINDOW_BYTES with the cuts of lrge_hip_reads_open* | LRGE_GPU_INGEST_WINDOWED,
   with or without that flag, and every window is proven by the record scan; a text within one window is the last window.
   lrge_hip_reads_census* (replaces io.rs:140-145): nothing is stored and no identifier leaves the device.  out[0] records, out[1]
   the sum of their sequence lengths, out[2] text bytes, out[3] windows flushed.  The count is that of lrge_hip_read_records on
   the same bytes, or the call is LRGE_ERR_UNPROVEN.
   lrge_hip_reads_open_selected* (replaces twoset.rs:122-201 behind lib.rs:189-204): sel[0, k) are strictly ascending record
   ordinals (file order, 0-based).  Only their identifiers come to the host and only their bases go to the store: the handle is
   an ordinary windowed-store handle of k reads in file order, read j being record sel[j] of lrge_hip_read_records, and
   lrge_hip_reads_count (k) / _table / _timings / _window_stats / _name_ranks / lrge_hip_seqset_from_reads (indices 0..k-1) /
   lrge_hip_reads_free work unchanged.  INGEST_MAX_BYTES bounds the chosen bases plus the block; 2^32 records and a window of 2^32
   bytes are LRGE_ERR_UNPROVEN as for the windowed open, 4 GiB of identifiers counts the chosen ones only.  k = 0 is legal: an
   empty handle, and the pass still proves the file.  LRGE_ERR_INVALID, before any handle is handed out: ordinals that are not
   strictly ascending; an ordinal at or above the number of records the pass saw (the message names the ordinal and the count).
   LRGE_ERR_UNPROVEN for both, whatever the flags: text whose first bytes say BAM, SAM or CRAM ("selected ingest takes FASTA /
   FASTQ only"; BAM is taken with LRGE_GPU_INGEST_SELECT_ALN beside LRGE_GPU_INGEST_BAM, SAM with LRGE_GPU_INGEST_SELECT_SAM beside
   LRGE_GPU_INGEST_SAM, CRAM with LRGE_GPU_INGEST_SELECT_CRAM beside LRGE_GPU_INGEST_CRAM, below), Zstandard input (its text is never
   windowed without LRGE_GPU_INGEST_WINDOWED_ZSTD, below); everything else as lrge_hip_reads_open*.
   lrge_hip_reads_select_stats: out[0] records seen, out[1] records kept, out[2] sequence bases seen, out[3] bases kept by the
   pass that made the handle; zeros for a handle of lrge_hip_reads_open*. */
int      lrge_hip_reads_census(lrge_hip_ctx *ctx, const char *path, int flags, uint64_t out[4]);
int      lrge_hip_reads_census_mem(lrge_hip_ctx *ctx, const void *file_bytes, uint64_t len, int flags, uint64_t out[4]);
int      lrge_hip_reads_open_selected(lrge_hip_ctx *ctx, const char *path, int flags, const uint32_t *sel, uint32_t k,
                                      lrge_hip_reads **out);
int      lrge_hip_reads_open_selected_mem(lrge_hip_ctx *ctx, const void *file_bytes, uint64_t len, int flags, const uint32_t *sel,
                                          uint32_t k, lrge_hip_reads **out);
int      lrge_hip_reads_select_stats(const lrge_hip_reads *reads, uint64_t out[4]);

/* The sampled ingest with a seek map (k_fx_seek, k_fx_runs): the reference's count pass (io.rs count_records,
   io.rs:140-145) reads the whole file, and so must the census, but its second reading (the two-pass reading of twoset.rs:122-201
   and ava.rs, which write only the drawn reads) needs only the places where drawn reads lie.  Opt-in: every call above does what it
   did.
   lrge_hip_reads_census_map*: lrge_hip_reads_census* (the same out[4], the same refusals with the same texts) that also leaves a
   map: the text is cut into cells of option INGEST_SEEK_STRIDE_BYTES (default 65536, at least 1), and every cell in which a record
   starts (at the '>' or '@' of its header line) gets one point -- the first such record's ordinal, its text offset and, for BGZF,
   the block that holds that offset.  Free the map with lrge_hip_read_map_free; it belongs to no context.
   lrge_hip_read_map_stats: out[0] records, out[1] points, out[2] the stride, out[3] text bytes.  lrge_hip_read_map_points: the first
   `cap` points copied out (any of the arrays may be NULL): ordinal, text offset, file offset of the BGZF block (0 for plain input).
   lrge_hip_reads_open_mapped*: lrge_hip_reads_open_selected* of the input the map was made of.  For plain and BGZF input only the
   runs that hold chosen records (from the last point at or below an ordinal to the first point above it; runs that touch are merged)
   are brought: the path form reads only those file ranges, BGZF decodes only their blocks (CRC and ISIZE checked as always).  The
   runs, concatenated, are scanned and proven like any text, and the handle is the one lrge_hip_reads_open_selected* gives -- the
   same reads, text_bytes and select_stats (seen / bases_seen are the file's, taken from the map).  A map of xz input
   runs the full selected pass.  Plain and multi-member gzip is entered (k_gz_entry, k_gz_win_pick): the census
   keeps an entry table -- entry 0 the start of the file, then every accepted chunk of the speculative decode whose text offset is at
   least option INGEST_SEEK_GZIP_BYTES (default 1 MiB, at least 1) behind the previous entry's: its bit offset, text offset, member
   state, the length and CRC-32 of the text up to the next entry and the 32 KiB window in front of it.  The windows are host memory
   outside INGEST_MAX_BYTES, 32 KiB an entry (1.6 % of the text at the defaults).  A point's c_off is the byte of the entry that holds
   its offset; the mapped open reads only the file ranges of the entries the runs touch and decodes each from its seed, and an entry that
   ends elsewhere or with another length or CRC-32 is "the map does not fit the input".  A single entry whose text does not fit
   INGEST_MAX_BYTES is the selected open's "text above INGEST_MAX_BYTES".
   A gzip map whose only entry is the file's start although the census walked several chunks (a text below the spacing) is not
   entered: its kind is 2 and the mapped open runs the full selected pass.
   bzip2 under LRGE_GPU_INFLATE_BZIP2 is entered too (k_bz_walk_rec, k_bz_rle_write_rec, k_bz_marks_text), FASTA / FASTQ
   text only.  The census keeps every accepted block -- its bit offset and end bit, the bytes in front of the run-length layer, origPtr,
   the stored CRC, its text offset and length -- and 64 marks of 16 bytes a block, which let a second decode enter the block's inverse
   BWT and run-length layer at 64 places (1 KiB a block of host memory outside INGEST_MAX_BYTES).  Entries are groups of whole
   consecutive blocks: a new one opens at the first block whose text offset is at least option INGEST_SEEK_BZIP2_BYTES (default 512 KiB,
   at least 1) behind the previous entry's.  A point's c_off is the first byte of the entry that holds its offset; the mapped open reads
   only the file ranges of the entries the runs touch, and a block whose entropy decode gives another length, origPtr, CRC or end than
   the map's, or that does not arrive where its marks say, is "the map does not fit the input".  A map whose only entry spans several
   blocks is not entered (kind 2); a file of one block is.
   lrge_hip_read_map_entries: out[0] entries, out[1] window bytes (bzip2: mark bytes) held, out[2] the map's kind (0 plain, 1 BGZF, 2 a container that is
   not entered, 3 CRAM, 4 gzip, 5 bzip2), out[3] the spacing in force (0: neither a gzip nor a bzip2 map).  LRGE_ERR_INVALID, before any device work: ordinals not strictly ascending; "the map is of another
   input" (file length, text bytes, block count or container differ); an ordinal at or above the map's records; and, path form, a
   file range that does not hold the blocks the map names.  LRGE_ERR_UNPROVEN "the map does not fit the input": the runs are not
   proven or hold another number of records than the map says -- the caller may take lrge_hip_reads_open_selected*.
   lrge_hip_reads_seek_stats: out[0] runs, out[1] text bytes brought, out[2] file bytes read, out[3] BGZF blocks or gzip / bzip2 entries decoded by
   lrge_hip_reads_open_mapped*; zeros for a handle of every other open. */
typedef struct lrge_hip_read_map lrge_hip_read_map;
int      lrge_hip_reads_census_map(lrge_hip_ctx *ctx, const char *path, int flags, uint64_t out[4], lrge_hip_read_map **map);
int      lrge_hip_reads_census_map_mem(lrge_hip_ctx *ctx, const void *file_bytes, uint64_t len, int flags, uint64_t out[4],
                                       lrge_hip_read_map **map);
void     lrge_hip_read_map_free(lrge_hip_read_map *map);
int      lrge_hip_read_map_stats(const lrge_hip_read_map *map, uint64_t out[4]);
int      lrge_hip_read_map_points(const lrge_hip_read_map *map, uint64_t *ord, uint64_t *text_off, uint64_t *c_off, uint64_t cap);
int      lrge_hip_read_map_entries(const lrge_hip_read_map *map, uint64_t out[4]);
int      lrge_hip_reads_open_mapped(lrge_hip_ctx *ctx, const char *path, int flags, const lrge_hip_read_map *map, const uint32_t *sel,
                                    uint32_t k, lrge_hip_reads **out);
int      lrge_hip_reads_open_mapped_mem(lrge_hip_ctx *ctx, const void *file_bytes, uint64_t len, int flags, const lrge_hip_read_map *map,
                                        const uint32_t *sel, uint32_t k, lrge_hip_reads **out);
int      lrge_hip_reads_seek_stats(const lrge_hip_reads *reads, uint64_t out[4]);

/* The sampled ingest of unaligned BAM (k_bam_keep beside k_fx_bases, k_fx_pick, k_bam_spans, k_fx_seek): uBAM is
   what PacBio HiFi and dorado write, and two thirds of its text are qualities and tags the tool never reads (io.rs:93, 154-184).
   | LRGE_GPU_INGEST_SELECT_ALN (opt-in; it has effect only beside LRGE_GPU_INGEST_BAM and only in lrge_hip_reads_census*,
   _open_selected*, _census_map* and _open_mapped*; without it every call does what it did, the refusal text included): text whose
   first bytes are "BAM\1" is a BAM run in those six calls.  It passes through the windows of DESIGN section 18 whatever
   LRGE_GPU_INGEST_WINDOWED / _WINDOWED_ALN say, from the sources of the FASTA / FASTQ sampled calls (plain, BGZF, gzip, bzip2, xz);
   SAM (without LRGE_GPU_INGEST_SELECT_SAM, below), CRAM (without LRGE_GPU_INGEST_SELECT_CRAM, below) and Zstandard stay refused with the same texts.  The count and the records sel[j] are those of lrge_hip_read_records on
   the same bytes, or the call is LRGE_ERR_UNPROVEN (a mapped record, a damaged record, 1-3 trailing bytes, in whichever window) and
   hands out no handle.  A header that ends the text is an empty census and an empty handle.  The handle is the windowed BAM handle
   restricted to the chosen reads: (l_seq + 1) / 2 packed bytes a chosen record, dense, in file order, the pad nibble as it is;
   lrge_hip_seqset_from_reads, _name_ranks, _table, _window_stats and _bam_stats (summed over the windows the pass flushed; a mapped
   open: those of the sub-text) work unchanged.  select_stats out[2] / out[3] count bases; window_stats out[1] and INGEST_MAX_BYTES
   count store bytes.  A point of the seek map is a record's block_size field, the first point record 0 behind the header; a mapped
   open of a BAM map without both flags is refused as the census is. */
#define LRGE_GPU_INGEST_SELECT_ALN 1024

/* The sampled ingest of unaligned SAM (the windows of section 18 in the keep modes, k_fx_bases behind k_sam_records,
   k_fx_pick, k_fx_keep, k_fx_seek; no kernel of its own): what samtools and dorado write as text (io.rs:92-96, 154-184).
   | LRGE_GPU_INGEST_SELECT_SAM (opt-in; it has effect only beside LRGE_GPU_INGEST_SAM and only in lrge_hip_reads_census*,
   _open_selected*, _census_map* and _open_mapped*; without it every call does what it did, the refusal text included): text that
   starts with "@HD", "@SQ" or "@RG" is a SAM run in those calls.  It passes through the windows of DESIGN section 18 whatever
   LRGE_GPU_INGEST_WINDOWED / _WINDOWED_ALN say, from the sources of the FASTA / FASTQ sampled calls (plain, BGZF, gzip, bzip2, xz,
   sliding Zstandard).  The count and the records sel[j] are those of lrge_hip_read_records on the same bytes, or the call is
   LRGE_ERR_UNPROVEN (a record line with fewer than ten tabs, a bad flag, a mapped record, in whichever window) and hands out no
   handle.  A header that ends the text is an empty census and an empty handle.  The handle is the windowed SAM handle restricted to
   the chosen reads: their bases as ASCII, dense, in file order ("*" is length 0); lrge_hip_seqset_from_reads, _name_ranks, _table,
   _window_stats, _select_stats and _seek_stats work unchanged.  A point of the seek map is the first byte of a record's line, so
   header, @CO and empty lines lie in front of whichever point follows them; a run is whole lines, and the runs of a mapped open are
   scanned as a SAM text without a header.  Plain and BGZF input is entered; a map of gzip, bzip2, xz or Zstandard input runs the full
   selected pass.  A mapped open of a SAM map without both flags is refused as the census is. */
#define LRGE_GPU_INGEST_SELECT_SAM 4096

/* The sampled ingest of unaligned CRAM (k_rans_decode into a scratch of a round's size, k_fx_runs for the chosen
   reads; no kernel of its own).  CRAM does not pass through the windows: every BA block is independent and its place is known from
   the walk, so the four calls are the pipeline of LRGE_GPU_INGEST_CRAM (below) with another sink.
   | LRGE_GPU_INGEST_SELECT_CRAM (opt-in; it has effect only beside LRGE_GPU_INGEST_CRAM and only in lrge_hip_reads_census*,
   _open_selected*, _census_map* and _open_mapped*; without it every call does what it did, the refusal text included): input that
   starts with "CRAM" is walked on the host as in lrge_hip_reads_open*, the walk keeping only the chosen ordinals' identifiers
   (none for a census).  lrge_hip_reads_census*: every BA block is decoded and nothing kept, so a damaged body in any slice is
   LRGE_ERR_UNPROVEN as in the full open; out[0] records, out[1] the sum of the lengths, out[2] what lrge_hip_reads_text_bytes of the
   full open reports (the bases), out[3] 0.  lrge_hip_reads_open_selected*: the same over every block, the chosen reads' ranges
   copied to a store of exactly the chosen bases; k = 0 is legal.  lrge_hip_reads_census_map*: the census and a map whose points are
   the slices in which a record starts (lrge_hip_read_map_points: that record's ordinal, the slice's base offset, the file offset of
   its BA block; lrge_hip_read_map_stats: out[2], the stride, is 0).  lrge_hip_reads_open_mapped*: "the map is of another input"
   (LRGE_ERR_INVALID) on another file length, record count, base count or slice count; the walk again (identifiers, lengths and the
   mapped-record refusal are the host's; slices that are not the map's: "the map does not fit the input"); then only the BA blocks of
   slices that hold a chosen read with bases are decoded, and a refused head is found only there.  lrge_hip_reads_seek_stats: out[0]
   stretches of consecutive slices decoded, out[1] raw bytes decoded, out[2] compressed BA bytes uploaded, out[3] BA blocks decoded.
   The path forms read the whole file.  Everything the walk and the stream heads refuse is refused with the texts of the full open,
   and CRAM_MIN_BLOCKS is tested against the file's BA blocks in all four calls.  INGEST_MAX_BYTES bounds the chosen bases plus the
   largest round's compressed and raw bytes (the transform scratch is not counted): the rounds are those of option CRAM_ROUND_BYTES,
   halved until they fit; "chosen bases and one round of CRAM blocks above INGEST_MAX_BYTES" (LRGE_ERR_UNPROVEN) when a single block
   does not.  The handle is the CRAM handle restricted to the k chosen reads in file order: lrge_hip_reads_text_bytes is the file's,
   select_stats = (records, k, bases of the file, bases kept); in lrge_hip_reads_cram_stats containers, slices and records are the
   file's, the block and byte counts those of the blocks the pass decoded; window_stats out[0] is 0 and out[1] the bytes of the store. */
#define LRGE_GPU_INGEST_SELECT_CRAM 8192

/* The windowed and the sampled ingest of Zstandard (k_zs_xxh64_part, k_zs_slide): a match reaches back at most
   Window_Size bytes, so the decoder needs no more of the earlier text than the last min(frame bytes so far, window) bytes of the
   frame that is open when a round starts.
   | LRGE_GPU_INGEST_WINDOWED_ZSTD (opt-in; it has effect only beside LRGE_GPU_INFLATE_ZSTD; without it every call does what it did,
   the refusal texts included): lrge_hip_reads_open* | LRGE_GPU_INGEST_WINDOWED passes Zstandard text above INGEST_WINDOW_BYTES
   through the windows as gzip, bzip2 and xz text, and lrge_hip_reads_census*, _open_selected*, _census_map* and _open_mapped* take
   Zstandard input (a map of it runs the full selected pass, as one of gzip, bzip2 or xz).  The rounds are decoded in a work block of
   history plus one round (option ZSTD_ROUND_BLOCKS; its default then keeps a round's text within INGEST_WINDOW_BYTES), sized once
   from the block headers; INGEST_MAX_BYTES bounds the store, the window block and that work block together ("text above
   INGEST_MAX_BYTES" when the work block alone does not fit).  Frames, skippable frames, checksums (a frame that spans rounds is
   hashed in parts) and refusals are those of the resident route.  Text of 4 GiB or more is not verified.
   lrge_hip_reads_zstd_stats: out[0] rounds, out[1] the largest history carried into a round, out[2] the largest work text (history
   plus round), out[3] bytes of history moved; zeros for a handle whose call did not slide. */
#define LRGE_GPU_INGEST_WINDOWED_ZSTD 2048
int      lrge_hip_reads_zstd_stats(const lrge_hip_reads *reads, uint64_t out[4]);

/* The streamed first pass (no kernel of its own): without this flag lrge_hip_reads_open, _census, _open_selected and
   _census_map read the whole file into host memory before the first kernel runs, so the host holds as many bytes as the file has.
   | LRGE_GPU_INGEST_STREAM (opt-in; without it every call does what it did, the message texts included): those four calls read the
   file by range, in pieces of option INGEST_STREAM_BYTES (P; default 64 MiB, at least 1), into two pinned buffers.  The _mem forms
   accept and ignore the flag.  lrge_hip_reads_open needs LRGE_GPU_INGEST_WINDOWED beside it (LRGE_ERR_INVALID, the message names both
   flags): the size of the text is not known before the last piece, so every text passes through the windows whatever its size, as
   in the sampled calls, and there is no resident route.  BAM or SAM text, found by the first window's sniff, needs
   LRGE_GPU_INGEST_WINDOWED_ALN as always; without it the call is LRGE_ERR_UNPROVEN and says so.
   Plain text: pieces of min(P, window) bytes through two buffers, one filled while the other's copy is in flight (the first buffer is
   made before the container is known and has a BGZF buffer's size, min(P, file length) + 64 KiB; the second holds a piece); every file
   byte is read once.
   BGZF (unaligned BAM included): a buffer holds up to P compressed bytes behind the partial member the buffer before it ended in (it
   grows to hold one whole member where P is smaller); the block walk runs piece by piece under the rules of lrge_hip_bgzf_scan, the
   whole members are decoded from where they lie, and every file byte is read once.  Whether a file is BGZF is decided by its first
   member: a later member that is no BGZF block, a truncated member or trailing bytes end the call with LRGE_ERR_UNPROVEN and a
   message that gives the file offset and says to open without the flag (the whole-file route gives such a file to the gzip decoder;
   windows have been delivered by then, so the streamed call cannot start again).  That is the one difference in outcome, and it is
   a refusal, never other records.  With a seek map the whole block table is kept, about 40 bytes a block of ordinary host memory
   outside out[2] below; without one only the current buffer's blocks are.
   Plain and multi-member gzip: the rounds, loads and prefetches are the ranges of the whole-file route, read from the file as they
   are staged; text, statuses and the entries of a seek map are the same by construction.  The bytes read exceed the file length by
   the overhang every round reads again, and the pinned staging is a round's (option GZIP_ROUND_BYTES), not P: out[2] is then the
   capacity of the staging buffer the context keeps across calls -- at least this call's largest round, and an earlier, larger file's
   where there was one.
   bzip2, Zstandard, xz and CRAM take the flag and are read whole as without it.  lrge_hip_reads_open_mapped with a map that is not
   entered (kind 2) streams its full selected pass under the flag.  A path that cannot be opened or read by range, a short read and a
   file that shrank are LRGE_ERR_IO; no partial result is handed out.
   lrge_hip_last_stream_stats: the reading of the last of those path calls on `ctx` -- out[0] read calls issued, out[1] file bytes
   read, out[2] pinned host bytes held for file bytes at the peak, out[3] 1 if the pass streamed, 0 if it read the file whole. */
#define LRGE_GPU_INGEST_STREAM 16384
int      lrge_hip_last_stream_stats(const lrge_hip_ctx *ctx, uint64_t out[4]);

/* Read sets built on the device from unaligned CRAM 3.0 / 3.1 (k_rans_decode): | LRGE_GPU_INGEST_CRAM (opt-in:
   no other flag implies it, and without it every call does what it did) sends input that starts with "CRAM" to a host walk of the
   containers -- the record loop of lrge_hip_read_records under a policy that reads no base, so identifiers, lengths and flags are
   the host reader's one for one -- and to a device decode of the BA (bases) block of every slice, straight into the dense base
   store a windowed FASTA handle has: lrge_hip_reads_count / _table / _timings / lrge_hip_seqset_from_reads /
   lrge_hip_reads_name_ranks work unchanged, text_bytes is the sum of the BA raw sizes, window_stats()[0] is 0.  Taken on the
   device: raw BA blocks, rANS 4x8 (orders 0 and 1), rANS Nx16 (orders 0 and 1, 4 or 32 states, shift 1..12, CAT, NOSZ, PACK, RLE,
   PACK with RLE).  LRGE_ERR_UNPROVEN, with a text that names the reason, and never a parse error of its own: BA not EXTERNAL, its
   content id read by another series or tag, two BA blocks in a slice, read lengths of a slice that do not add up to the BA block's
   raw size, RN not preserved, a mapped record (the reference's message), a BA block in gzip, bzip2, lzma, arith, fqzcomp, tok3 or
   in the STRIPE form of rANS Nx16, a rANS 4x8 table whose frequencies do not sum to 4096 (the host reader tolerates a short one)
   or that lists a symbol twice, any error the host reader raises during the walk, a block whose status is not OK on the device
   (compressed data exhausted, a state below the lower bound, a bad end state, an order-1 context without a table, run lengths that
   do not fit), fewer BA blocks than option CRAM_MIN_BLOCKS (default 32: the measured break-even against lrge_hip_read_records plus an upload, rounded up to a power of two), bases plus
   one round above INGEST_MAX_BYTES; compressed input is not looked into for a CRAM (it takes the route it took, and CRAM text is
   unproven there).  LRGE_ERR_TOO_MANY: 2^32 records or more.  Option CRAM_ROUND_BYTES (default 256 MiB): the BA blocks whose
   compressed bytes fit go up and are decoded by one launch; only the BA byte ranges are uploaded.
   lrge_hip_reads_cram_stats: the counts of the call; LRGE_ERR_INVALID for a handle that was not opened as CRAM.
   lrge_hip_rans_decode: n independent streams of comp, stream i = (method 0 raw / 4 rANS 4x8 / 5 rANS Nx16, offset, length, raw
   size) as a CRAM block body, decoded into out, stream i at the sum of the raw sizes before it (out_cap at least their sum);
   streams[i].status: 0, one of the block statuses 1..5 (exhausted, state, end, no table, runs), or 16: the stream head was refused
   on the host (lrge_hip_last_error keeps the first reason); the bytes of such a stream are zero.  LRGE_ERR_INVALID: a stream
   outside comp, a raw size of 2^31 or more, out_cap too small. */
typedef struct lrge_hip_cram_stats {
    uint64_t containers;          /* data containers */
    uint64_t slices;
    uint64_t records;
    uint64_t ba_raw;              /* BA blocks stored raw (copied) */
    uint64_t ba_rans4x8;
    uint64_t ba_ransnx16;
    uint64_t order1_blocks;       /* entropy-coded blocks of order 1 */
    uint64_t global_table_blocks; /* blocks whose model did not fit LDS: its frequencies were read from global memory */
    uint64_t comp_bytes;          /* the BA blocks' compressed bytes: all that was uploaded of the file */
    uint64_t raw_bytes;           /* the bases */
    uint64_t rounds;              /* launches of k_rans_decode */
    uint64_t walk_us;             /* microseconds of the host walk */
    uint64_t decode_us;           /* microseconds of the rounds: upload, launch, status words back */
} lrge_hip_cram_stats;
typedef struct lrge_hip_rans_stream { uint64_t offset; uint32_t length, raw_size, method, status; } lrge_hip_rans_stream;
#define LRGE_GPU_INGEST_CRAM 512
int      lrge_hip_reads_cram_stats(const lrge_hip_reads *reads, lrge_hip_cram_stats *out);
int      lrge_hip_rans_decode(lrge_hip_ctx *ctx, const void *comp, uint64_t comp_len, lrge_hip_rans_stream *streams, uint32_t n, void *out,
                              uint64_t out_cap, lrge_hip_cram_stats *stats);

/* Identifier ranks on the device (k_nl_key, k_nl_heads, k_nl_starts, k_nl_rank between radix_sort_pairs and
   scan_exclusive_u32): the `name_rank` every upload takes, i.e. the stand-in for the reference's name comparisons -- the duplicate
   check of all-vs-all (ava.rs:195-199), the self-overlap test and the pair key (ava.rs:369-382), the target names counted once per
   query and the duplicate check of the inverse direction (twoset.rs:286-302, 439-449) -- computed by a fixed number of stable LSD
   sorts instead of a comparison sort on one host thread.
   lrge_hip_name_ranks (ava.rs:369-382): `names` and name_off[n_names + 1] are laid out as lrge_hip_reads_table returns them
   (identifier i is names[name_off[i], name_off[i + 1])).  idx[0..n): the selected identifiers (any order, repeats allowed); idx == NULL
   means every identifier in order, and n must then equal n_names (else LRGE_ERR_INVALID; n == 0 is an empty selection either way).  rank_out[i]: the rank of idx[i] among
   the n selected entries -- the number of selected entries whose identifier is strictly smaller, byte-wise on unsigned bytes, a
   proper prefix being smaller; equal identifiers (a repeated index included) share a rank.  Two sets that meet in one call are
   ranked by concatenating their index lists, queries then targets, and splitting rank_out.  The host gathers only the selected
   identifiers into one padded block, so the transfer is proportional to the selection, not to the file; one sort by length and
   one 64-bit sort per 8 bytes of the longest selected identifier follow, and the ranks come back in one transfer at the end.
   n < 2 returns without touching the device.  stats (may be NULL): [0] sorts run, [1] W = ceil(longest selected identifier / 8),
   [2] distinct identifiers among the selection, [3] microseconds of the call.
   LRGE_ERR_TOO_MANY: n >= 2^32.  LRGE_ERR_INVALID: an idx entry out of range, offsets that are not monotone, an identifier of 2^32
   bytes or more.  LRGE_ERR_UNPROVEN: the longest selected identifier exceeds option NAME_RANK_MAX_BYTES (default 256: the cost is
   W + 1 sorts of all entries, so one long identifier must not stretch it without bound); the caller takes its host sort.
   LRGE_ERR_DEVICE: a runtime failure, memory that cannot be had.
   lrge_hip_reads_name_ranks (twoset.rs:286-302, 439-449): the same over the identifiers a lrge_hip_reads handle keeps on the host
   (resident or windowed alike), in the handle's own context; idx indexes the handle's records. */
int  lrge_hip_name_ranks(lrge_hip_ctx *ctx, const char *names, const uint64_t *name_off, uint64_t n_names,
                         const uint32_t *idx, uint64_t n, uint32_t *rank_out, uint64_t stats[4]);
int  lrge_hip_reads_name_ranks(const lrge_hip_reads *reads, const uint32_t *idx, uint64_t n, uint32_t *rank_out, uint64_t stats[4]);

/* Host only: which side packs the reads of a set that starts in host memory when `ranks_on_host` ranks share this host's CPUs (option
   LRGE_HIP_RANKS_ON_HOST, set by the launcher; LRGE_HIP_PACK = host | device overrides): 1 = the host (2-bit pack with AVX2, packed words
   over PCIe), 0 = the device (ASCII over the rank's own PCIe link, k_pack).  *granted_cpus (may be NULL) receives the CPUs the host
   grants this process (affinity mask and cgroup bandwidth).  The rule: one rank -> host; several -> host only if every rank has 8 CPUs. */
int  lrge_hip_pack_choice(int ranks_on_host, double *granted_cpus);

/* Host only: the k distinct indices in [0, n) that liblrge's sub-sampling draws (lib.rs:189-204), in the order
   rand 0.9.4's index::sample returns them (split_into_hashsets, twoset.rs:632-652, takes the LAST target_num_reads
   of them as targets).  has_seed = 0 seeds the generator from OS entropy.  Restated in include/lrge_rand.hpp.
   LRGE_ERR_INVALID if k > n (the reference panics) or out is NULL with k > 0. */
int  lrge_hip_unique_random_set(uint64_t k, uint32_t n, int has_seed, uint64_t seed, uint32_t *out);
/* One ChaCha block of that generator (key = 8 LE words, 64-bit counter, stream 0): known-answer tests. */
int  lrge_hip_chacha_block(const uint32_t key[8], uint64_t counter, int rounds, uint32_t out[16]);

/* Stage-level introspection (parity tests, profiling). */
int  lrge_hip_sketch_dump(lrge_hip_ctx *ctx, const lrge_hip_seqset *s, int preset, uint64_t *x,
                          uint64_t *y, uint64_t cap, uint64_t *n_out);
int  lrge_hip_index_dump(lrge_hip_ctx *ctx, const lrge_hip_index *ix, uint64_t *keys,
                         uint64_t *pos, uint64_t cap, uint64_t *n_out);
int  lrge_hip_anchors_dump(lrge_hip_ctx *ctx, const lrge_hip_index *ix,
                           const lrge_hip_seqset *queries, int dual, uint32_t query, uint64_t *x,
                           uint64_t *y, uint64_t cap, uint64_t *n_out);
/* How much of a call is timed with HIP events: 0 = LRGE_T_TOTAL, LRGE_T_CHAIN, LRGE_T_CHAIN_LPG only; 1 (default) = every
   stage; 2 = also a pair around every k_rs_scatter launch (LRGE_T_RS_SCATTER: ~14 more pairs per call, ~2 % of a C2
   step in host work between launches).  Untimed slots read 0.  LRGE_HIP_TIMERS=<level> sets the initial level. */
int  lrge_hip_set_timer_level(lrge_hip_ctx *ctx, int level);
int  lrge_hip_last_timings(const lrge_hip_ctx *ctx, float ms[LRGE_T_N]);
int  lrge_hip_last_counters(const lrge_hip_ctx *ctx, uint64_t c[LRGE_C_N]);
const char *lrge_hip_version(void);

#ifdef __cplusplus
}
#endif
#endif
