/* irs_hip.h — C ABI of the MI355X-native IResearch query-execution path.
 *
 * This is the drop-in boundary: plain pointers and sizes, no
 * exceptions, no STL, no torch types.  A C++ adapter deriving
 * irs::postings_reader / irs::filter::prepared binds these entry points (see
 * INTEGRATION.md); each function below names the reference interface it
 * replaces (paths relative to the IResearch tree, v1.3).
 *
 * Device: AMD gfx950 (MI355X) only.  Every entry point fails with
 * IRS_HIP_EHIP when no such device is usable — there is no CPU fallback.
 */
#ifndef IRS_HIP_H
#define IRS_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define IRS_HIP_ABI_VERSION 12
#define IRS_HIP_BLOCK_SIZE 128u  /* postings per block, formats_10.cpp:90 */
#define IRS_HIP_MAX_TERMS 16u    /* terms per boolean query               */
#define IRS_HIP_MAX_WIDE_TERMS 64u /* entries of one IRS_HIP_OP_MULTITERM query */
#define IRS_HIP_MAX_K 4096u      /* largest top-k                         */
#define IRS_HIP_MAX_PHRASE_TERMS 8u /* terms (parts) of one by_phrase query */
#define IRS_HIP_MAX_PHRASE_ENTRIES 16u /* included entries of one variadic by_phrase,
                                           every member of every part counted        */
#define IRS_HIP_MAX_EXCLUDED 16u /* IRS_HIP_EXCLUDE entries of one query   */
#define IRS_HIP_NO_TERM 0xFFFFFFFFu
#define IRS_HIP_POS_OFFSETS 1u
#define IRS_HIP_POS_PAYLOADS 2u
#define IRS_HIP_NORM2 0u
#define IRS_HIP_NORM_LEGACY 1u
/* irs::Scorer::WandType (scorer.hpp:196-201) of the scorer a field's wand data was written by */
#define IRS_HIP_WAND_NONE 0u      /* unknown / no wand data                               */
#define IRS_HIP_WAND_DIV_NORM 1u  /* TFIDF with norms, BM11: (freq, norm) of the doc with the
                                     largest freq / norm (wand_writer.hpp:181-186)         */
#define IRS_HIP_WAND_MAX_FREQ 2u  /* BM15, TFIDF without norms: the largest frequency      */
#define IRS_HIP_WAND_MIN_NORM 3u  /* BM25: largest frequency, smallest norm                */

/* Errors replace the reference's exceptions (io_error / index_error,
 * formats_10.cpp:158-160, 3410-3415): never thrown across this boundary. */
typedef enum irs_hip_status {
  IRS_HIP_OK = 0,
  IRS_HIP_EINVAL = -1,       /* illegal_argument                          */
  IRS_HIP_ECORRUPT = -2,     /* index_error: malformed `.doc` bytes       */
  IRS_HIP_ENOMEM = -3,
  IRS_HIP_EHIP = -4,         /* HIP runtime failure / no gfx950 device    */
  IRS_HIP_EOVERFLOW = -5,    /* candidates exceed the memory budget even after the exact re-run */
  IRS_HIP_EUNSUPPORTED = -6,
  IRS_HIP_EPEER = -7         /* a batch with a communicator (irs_hip_batch_set_comm): ANOTHER rank
                              * could not re-execute its batch; no rank did, the results are not
                              * valid (this rank's own failure is reported as what it was) */
} irs_hip_status;

typedef enum irs_hip_layout {
  IRS_HIP_LAYOUT_SCALAR = 0, /* formats "1_0".."1_5": format_traits, formats_10.cpp:86-131   */
  IRS_HIP_LAYOUT_SIMD4 = 1   /* "1_2simd".."1_5simd": format_traits_sse4, :4122-4157         */
} irs_hip_layout;

/* irs::version10::term_meta — core/formats/formats_10_attributes.hpp:30-50,
 * as filled by postings_reader_base::decode (formats_10.cpp:3421-3456). */
typedef struct irs_hip_term_meta {
  uint32_t docs_count;   /* irs::term_meta::docs_count */
  uint32_t freq;         /* irs::term_meta::freq       */
  uint64_t doc_start;
  uint64_t pos_start;
  uint64_t pos_end;
  uint64_t pay_start;
  uint64_t e_skip_start; /* union { doc_id_t e_single_doc; uint64_t e_skip_start; } */
} irs_hip_term_meta;

/* What postings_reader::prepare (formats_10.cpp:3352-3419) and the Norm2
 * column reader (norm.hpp:210-251, columnstore2.cpp:650-789) see of one
 * segment.  All pointers are HOST pointers borrowed for the call only. */
typedef struct irs_hip_segment_desc {
  int32_t device;           /* HIP device ordinal                                  */
  int32_t layout;           /* irs_hip_layout                                      */
  const uint8_t* doc_file;  /* whole `.doc` file: index_input::read_buffer(0, len,  */
  uint64_t doc_file_len;    /*   BufferHint::PERSISTENT) (data_input.hpp:136-137)  */
  uint32_t num_docs;        /* docs in the segment; ids are 1..num_docs            */
  uint32_t has_freq;        /* field indexed with IndexFeatures::FREQ              */
  const uint8_t* norms;     /* dense Norm2 column bytes (big-endian values), or NULL */
  uint32_t norm_width;      /* 1, 2 or 4 (Norm2Header::num_bytes, norm.hpp:83-125) */
  uint32_t norm_min_doc;    /* header.min: doc id of norms[0] (normally 1)         */
  uint64_t norm_count;      /* number of values in `norms`                         */
  const irs_hip_term_meta* terms; /* the field's term table (term dictionary walk) */
  uint32_t num_terms;
  uint32_t wand_count;      /* scorers the field was indexed with — the `wand_count` the
                             * reference passes to postings_reader::iterator()
                             * (formats.hpp:160-168): formats 1_4/1_5 interleave that many
                             * (size byte, payload) pairs of "wand data" in front of short
                             * lists' tails (formats_10.cpp:686-688, skipped as :2298-2301)
                             * and inside the skip data (never read here). 0..16. */
  const uint8_t* pos_file;  /* whole `.pos` file of a field with IndexFeatures::POS (and no
                             * offsets / payloads); zero-based (formats 1_3+) or one-based
                             * (1_0..1_2) position storage is told from the file's version
                             * (formats_10.cpp:283-304) — what postings_reader::prepare opens
                             * as pos_in_ (:3369-3381); NULL: no positions, no phrase queries */
  uint64_t pos_file_len;
  uint32_t pos_features;    /* what else the field stores per position: IRS_HIP_POS_OFFSETS
                             * (IndexFeatures::OFFS), IRS_HIP_POS_PAYLOADS (IndexFeatures::PAY).
                             * Both change the vint tail of `.pos` (formats_10.cpp:728-760) and
                             * are answered with IRS_HIP_EUNSUPPORTED for now instead of being
                             * mis-read; 0 = positions only */
  uint32_t norm_kind;       /* IRS_HIP_NORM2 (0): `norms` are Norm2 values, big-endian integers of
                             * norm_width bytes (norm.hpp:128-251) — the field length in tokens.
                             * IRS_HIP_NORM_LEGACY (1): the legacy `Norm` feature (norm.hpp:46-70):
                             * one little-endian float per doc, 1/sqrt(length) (norm_width 4; the
                             * adapter decodes the sparse zvfloat column into this dense array,
                             * Norm::DEFAULT() = 1 for docs without a value) */
  uint32_t wand_type;       /* IRS_HIP_WAND_*: what scorer 0 of the field's wand data wrote
                             * (Scorer::wand_type of the scorer the field was indexed with).  Only
                             * MAX_FREQ and MIN_NORM pairs bound every score function
                             * (Scorer::compatible, scorer.cpp:31-64: a DivNorm index is refused
                             * for MaxFreq / MinNorm queries) — those are read from the index;
                             * with DIV_NORM or NONE the per-block (max freq, min norm) pairs
                             * are derived from the postings, which is always sound. */
  const uint32_t* doc_mask; /* the segment's DocumentMask: ids of its deleted docs, in any order, as
                             * index_utils::ReadDocumentMask (index_utils.cpp:476) fills it from the
                             * `.doc_mask` file (DocumentMaskReader::read, formats_10.cpp:3275-3312);
                             * NULL / 0: none.  The reference filters every iterator a caller wraps
                             * with SegmentReaderImpl::mask (segment_reader_impl.cpp:69-101, 286:
                             * MaskDocIterator skips the docs the mask contains); a batch cannot be
                             * wrapped afterwards — it only yields the k best docs — so the mask
                             * belongs to the segment here: no query of a batch (Or / And /
                             * min-match / by_phrase) returns, counts or scores a masked doc, and
                             * irs_hip_bit_union does not set its bit.  The postings-level surfaces
                             * (irs_hip_decode_term / _positions / _term_directory: what
                             * postings_reader::iterator yields) are not filtered, and neither are
                             * the statistics of the scorers (the reference's are index statistics
                             * too).  Ids outside 1..num_docs are ignored. */
  uint64_t doc_mask_count;
} irs_hip_segment_desc;

typedef struct irs_hip_segment irs_hip_segment; /* opaque, immutable after open */

/* Replaces postings_reader::prepare + the per-iterator reopen()/seek()
 * (formats_10.cpp:3352-3419, 2251-2262): stages the `.doc` bytes and the norm
 * column into HBM and builds the per-term block directory ON THE GPU by
 * walking block headers (bitpack.hpp:52-69).  Validates the file header
 * (format_utils.cpp:74-105) and that `layout` matches its version. */
int irs_hip_segment_open(const irs_hip_segment_desc* desc, irs_hip_segment** out);
void irs_hip_segment_close(irs_hip_segment* seg);

/* postings_reader::CountMappedMemory analogue: bytes resident in HBM.  Grows after open by the
 * tables a segment builds on first use and keeps: the block-max pairs of irs_hip_batch_set_wand
 * (8 bytes per 128-posting block) and the posting-order copy of a 1-byte Norm2 column (one byte
 * per posting of the whole segment — built by the first batch that joins posting streams, or whose
 * conjunctions / phrases score with norms). */
uint64_t irs_hip_segment_device_bytes(const irs_hip_segment* seg);
/* SubReader::live_docs_count (index_reader.hpp): num_docs minus the docs of doc_mask. */
uint64_t irs_hip_segment_live_docs(const irs_hip_segment* seg);

/* Replaces `postings_reader::iterator(...)` + `while (it->next())`
 * (formats_10.cpp:3491-3533, 2089-2119): decodes the whole posting list of
 * term ordinal `term` bit-exactly into host arrays. freqs may be NULL
 * (iterator requested without IndexFeatures::FREQ). */
int irs_hip_decode_term(irs_hip_segment* seg, uint32_t term, uint32_t* docs,
                        uint32_t* freqs, uint32_t cap, uint32_t* count);

/* Replaces draining the `position` attribute behind `while (it->next())`
 * (position::next, formats_10.cpp:1606-1633, fed by doc_iterator::next :2106-2113):
 * every position of every doc of term ordinal `term`, doc after doc — term_meta::freq
 * values in all (freqs from irs_hip_decode_term say where each doc's run ends).
 * Needs a segment opened with pos_file. */
int irs_hip_decode_positions(irs_hip_segment* seg, uint32_t term, uint32_t* positions,
                             uint64_t cap, uint64_t* count);

/* postings_reader::bit_union (core/formats/formats_10.cpp:3716-3806; virtual at
 * core/formats/formats.hpp:182-190): ORs bit `doc` into the caller's bitset
 * (`size_t* set` in the reference: 64-bit little-endian words, bit index = doc id,
 * so the set needs num_docs + 1 bits) for every posting of every listed term (of every doc that
 * is not in the segment's doc_mask);
 * freq blocks are skipped.  IRS_HIP_NO_TERM entries are ignored.  *count receives
 * what the reference returns: the SUM of the terms' docs_count (not a popcount).
 * Docs at or beyond 64 * n_words are not representable and are dropped. */
int irs_hip_bit_union(irs_hip_segment* seg, const uint32_t* terms, uint32_t n_terms,
                      uint64_t* set, uint64_t n_words, uint64_t* count);

/* The POPULATIONS of several such unions in one call, the bitsets never leaving the device: set i
 * is the union of the postings of terms[offsets[i] .. offsets[i + 1]) over doc ids 1..num_docs
 * (deleted docs left out), counts[i] its number of docs — the `hits` of a multi-term filter
 * (MultiTermQuery::execute, multiterm_query.cpp:112-184: scored iterators + one
 * lazy_bitset_iterator over the unscored terms; index-search counts what the iterator yields,
 * utils/index-search.cpp:745-779) when its top k comes from the scored terms' disjunction and
 * only the count is wanted from the rest: 8 bytes per filter cross PCIe instead of a bit per doc. */
int irs_hip_bit_union_counts(irs_hip_segment* seg, const uint32_t* terms, const uint32_t* offsets,
                             uint32_t n_sets, uint64_t* counts);

/* The block directory of one term, for inspection/tests: absolute last doc id
 * and `.doc` byte offset of every full 128-doc block — the information the
 * reference keeps in skip level 0 (formats_10.cpp:501-533). */
int irs_hip_term_directory(irs_hip_segment* seg, uint32_t term,
                           uint32_t* last_docs, uint64_t* offsets, uint32_t cap,
                           uint32_t* count);

/* ------------------------------------------------------------ queries -- */

typedef enum irs_hip_op {
  IRS_HIP_OP_OR = 0, /* irs::Or / by_term: disjunction.hpp MakeDisjunction :1411-1467 */
  IRS_HIP_OP_AND = 1, /* irs::And: conjunction.hpp MakeConjunction :436-490 — executed block
                         by block of the rarest term (Conjunction::converge :207-223)    */
  IRS_HIP_OP_MINMATCH = 2, /* irs::Or with min_match_count: MinMatchQuery::execute
                             (boolean_query.cpp:212-247) -> min_match_iterator =
                             block_disjunction<kMinMatch> (disjunction.hpp:1378-1383)   */
  IRS_HIP_OP_PHRASE = 3,  /* irs::by_phrase of plain terms: FixedPhraseQuery::execute
                             (phrase_query.cpp:44-111) -> PhraseIterator<Conjunction,
                             FixedPhraseFrequency> (phrase_iterator.hpp:75-166, 540-626).
                             terms[first_term + i] = i-th phrase term with its
                             phrase_offset; every entry carries the SAME scorer values: the
                             phrase's one stats blob, into which every term's statistics
                             were finished (phrase_filter.cpp:281-287: idf sums), times
                             the filter boost.  score = that scorer at tf = phrase
                             frequency.  An absent term empties the query in that segment.
                             A batch holds phrase queries only, or none.
                             Variadic phrases (a part standing for a set of terms,
                             VariadicPhraseQuery): IRS_HIP_PHRASE_ALT below; a phrase
                             plus required terms (an And of a by_phrase and by_terms):
                             IRS_HIP_PHRASE_REQUIRED below.                            */
  IRS_HIP_OP_MULTITERM = 4 /* a scored set of up to IRS_HIP_MAX_WIDE_TERMS (term, boost) with
                             min_match — see below                                        */
} irs_hip_op;

/* IRS_HIP_OP_MULTITERM: irs::by_terms (by_terms_options: a set of (term, boost) and min_match,
 * core/search/terms_filter.cpp:110-153), executed as MultiTermQuery::execute does
 * (core/search/multiterm_query.cpp:114-181): a min_match_iterator over one scored iterator per
 * term.  It is also what the scored part of by_range / by_prefix / by_wildcard becomes beyond
 * IRS_HIP_MAX_TERMS states (scored_terms_limit{1024}, core/search/range_filter.hpp:58; the
 * reference's benchmark passes --scored-terms-limit=16, scripts/search-benchmark.sh:14) and what
 * by_edit_distance needs once its terms are visited (max_terms = 50, utils/index-search.cpp:413).
 *   n_terms   1..IRS_HIP_MAX_WIDE_TERMS included entries, each with its own scorer values (c0
 *             holds term boost x filter boost) and validated like any by_term entry; more than
 *             IRS_HIP_MAX_WIDE_TERMS is IRS_HIP_EUNSUPPORTED
 *   min_match 1..n_terms; 0 or more than n_terms is IRS_HIP_EINVAL
 *   merge     IRS_HIP_MERGE_SUM; MAX / MIN is IRS_HIP_EUNSUPPORTED
 * Per segment d matches iff at least min_match of the PRESENT entries hold d, minus the segment's
 * deleted docs; score(d) = the sum of the scores of the entries holding d; total_hits counts the
 * matching docs.  An absent entry (IRS_HIP_NO_TERM or no docs) adds nothing and counts for
 * nothing; fewer than min_match present entries empty the query in that segment.  The same term
 * twice scores twice (it is decoded once).  A zero boost matches with score 0.
 * Refused at create with IRS_HIP_EUNSUPPORTED (the entries of such a query are postings decoded
 * once per batch into 4-byte records, scored through tables): a term with a frequency above 255;
 * a scorer outside the table family (BM25 / BM15 / TF-IDF over a 1-byte Norm2 column or none:
 * wide and legacy norm columns are outside) or more than 4 distinct (kind, norm_const,
 * norm_length) in one query; IRS_HIP_EXCLUDE entries.  Refused on a batch that holds such a query,
 * IRS_HIP_EUNSUPPORTED: irs_hip_batch_set_doc_sets / _host, irs_hip_batch_set_comm,
 * irs_hip_batch_match_sets / _to_device (the unscored union of many terms is irs_hip_bit_union).
 * The units run exhaustively on kernels of their own (k_wide_pilot, k_wide_score: one lane per
 * term, 64-bit fixed-point sums whose low 7 bits count the terms on a doc) over the batch's decoded
 * posting streams — a term shared with another query, or held by the device's stream cache, is
 * decoded once or not at all; irs_hip_batch_stream_counts counts these streams too.
 * irs_hip_batch_set_wand, _set_path and _set_paired_tiles leave them as they are,
 * irs_hip_batch_set_shared_threshold leaves each a threshold of its own, irs_hip_batch_configure's
 * tile_docs is ignored by them; cand_cap, pilot_stride, min scores, results, re-runs, profile and
 * timings (their kernels count into the PILOT and SCORE stages) behave as for any batch.  A batch
 * may mix these queries with any non-phrase queries: the others give bit for bit what they give in
 * a batch of their own, on the path they would take there.  A compatible addition to ABI 12: the
 * op was IRS_HIP_EINVAL before. */

/* Which ScoreFunction Scorer::prepare_scorer would have built. */
typedef enum irs_hip_scorer_kind {
  IRS_HIP_SCORE_BM25 = 0,      /* bm25.cpp:321-364; norm path by segment norm_width (:466-476),
                                  legacy Norm column => :333-337, 242-249;
                                  no norm column => norm == 1 (:487-489)               */
  IRS_HIP_SCORE_BM15 = 1,      /* bm25.cpp:288-319 (b == 0)                            */
  IRS_HIP_SCORE_BM1 = 2,       /* bm25.cpp:262-286 (k == 0): constant                  */
  IRS_HIP_SCORE_TFIDF = 3,     /* tfidf.cpp:185-187, 251                                */
  IRS_HIP_SCORE_TFIDF_NORM = 4 /* tfidf.cpp:253, normalize() == true                   */
} irs_hip_scorer_kind;
/* Not a scorer: the `kind` of an EXCLUDED term — a by_term under irs::Not in an And
 * (boolean_filter.cpp:92-135, boolean_query.cpp:121-141: the included part wrapped in
 * exclusion(incl, disjunction(excluded)), exclusion.hpp).  Docs that contain the term are removed
 * from the query's matches; the term scores nothing and changes no statistic.  Such entries follow
 * the included ones in [first_term, first_term + n_terms), at most IRS_HIP_MAX_EXCLUDED of them,
 * and at least one included entry precedes them.  c0, norm_* and phrase_offset are ignored;
 * IRS_HIP_NO_TERM means absent in this segment (no effect, boolean_query.cpp:131-134); a batch
 * over several segments carries each segment's own ordinal, as for included terms.  The op,
 * min_match and merge apply to the included entries only.  For every op (OR, AND, MINMATCH,
 * PHRASE) the matches are the included part's, minus deleted docs, minus every doc of an
 * excluded term: scores and order are unchanged, total_hits counts what remains and the top k
 * is drawn from it.  Which path such a unit takes: irs_hip_batch_set_path. */
#define IRS_HIP_EXCLUDE 0x100

/* OR-ed into the `kind` of an IRS_HIP_OP_PHRASE entry: one more member of the phrase part opened by
 * the nearest preceding entry without the flag — a by_phrase_options part of by_terms / by_prefix /
 * by_wildcard / by_range (phrase_filter.hpp:41-47), whose visitor yields a set of terms in
 * dictionary order (VariadicPrepareCollect, phrase_filter.cpp:295-432).  The entry's
 * phrase_offset equals its part's; the first included entry never carries the flag; the same term
 * twice in one part is IRS_HIP_EINVAL; every entry carries the phrase's one scorer, as for plain
 * phrases.  At most IRS_HIP_MAX_PHRASE_TERMS parts and IRS_HIP_MAX_PHRASE_ENTRIES included entries
 * (more: IRS_HIP_EUNSUPPORTED); IRS_HIP_EXCLUDE entries may follow.  Per segment an absent member
 * (IRS_HIP_NO_TERM or no docs) is dropped, and a part without a present member empties the query.
 * Phrase frequency (VariadicPhraseFrequency, phrase_iterator.hpp:197-364), parts P_0..P_n-1 at
 * offsets off_i (off_0 = 0):
 *   freq(d) = sum over t in P_0 of #{p in pos(t, d) : for every i >= 1 some u in P_i has
 *             p + off_i in pos(u, d)}
 * — members of the first part add up, a later part needs one member at the position.  Score: the
 * scorer at tf = freq(d), as for plain phrases.  A compatible addition to ABI 12: without the flag
 * an entry means what it always did, and a kind with the flag was IRS_HIP_EINVAL before. */
#define IRS_HIP_PHRASE_ALT 0x200

/* OR-ed into the `kind` of an included IRS_HIP_OP_PHRASE entry: a REQUIRED TERM — a by_term child
 * of the irs::And that also holds this phrase, `+"new york" +hotel` (And::prepare ->
 * make_conjunction over {PhraseIterator, term iterators}: boolean_filter.cpp:150-210,
 * boolean_query.cpp:60-145, conjunction.hpp:436-490; every child is prepared on its own and the
 * And's merger sums the children's scores).  Entry order in [first_term, first_term + n_terms):
 * the phrase's entries (at least 2), then 1 or more entries with this flag, then 0 to
 * IRS_HIP_MAX_EXCLUDED IRS_HIP_EXCLUDE entries.  An entry without the flag behind one with it, or
 * fewer than 2 phrase entries in front of the first flagged one, is IRS_HIP_EINVAL; so is the flag
 * on an OR / AND / MINMATCH entry.  A flagged entry carries its OWN scorer values (kind, c0,
 * norm_const, norm_length — the by_term's statistics and boost x the And's boost), validated like
 * any by_term entry; its phrase_offset is ignored; it may name a term that is also a phrase word.
 * Phrase entries + flagged entries <= IRS_HIP_MAX_PHRASE_TERMS (more: IRS_HIP_EUNSUPPORTED); a
 * query with both IRS_HIP_PHRASE_ALT and flagged entries, and a batch that holds variadic phrases
 * next to queries with flagged entries, are IRS_HIP_EUNSUPPORTED; merge stays IRS_HIP_MERGE_SUM.
 * Per segment:
 *   d matches iff the phrase frequency pf(d) > 0 and every required term holds d (minus deleted
 *   docs and IRS_HIP_EXCLUDE terms);
 *   score(d) = s_phrase(tf = pf(d), norm(d)) + sum over the required terms of s_j(tf_j(d), norm(d)),
 *   in float32, the children in cost order as Conjunction sorts them (conjunction.hpp:450-453): the
 *   phrase costs the smallest docs_count of its words (the front of its approx_ conjunction,
 *   phrase_iterator.hpp:545-560), a term its docs_count; ties in entry order.
 * An absent phrase word or required term (IRS_HIP_NO_TERM or no docs) empties the query in that
 * segment.  total_hits, the top k and every batch control behave as for any phrase batch; a batch
 * with such a query runs all its phrases on k_phrase_and, plain phrases giving bit for bit what
 * they give in a batch of their own.  A compatible addition to ABI 12: without the flag an entry
 * means what it always did, and a kind with the flag was IRS_HIP_EINVAL before. */
#define IRS_HIP_PHRASE_REQUIRED 0x400

/* OR-ed into the `kind` of an included IRS_HIP_OP_PHRASE entry: an OPTIONAL TERM — a by_term child
 * of the irs::Or that also holds this phrase, `"new york" hotel cheap` (Or::prepare prepares every
 * child on its own, boolean_filter.cpp:150-210; MakeDisjunction over {PhraseIterator, term
 * iterators}, disjunction.hpp:1411-1467; min_match <= 1, merge SUM).  Entry order in [first_term,
 * first_term + n_terms): the phrase's entries (at least 2), then 1 or more entries with this flag,
 * then 0 to IRS_HIP_MAX_EXCLUDED IRS_HIP_EXCLUDE entries.  An entry without the flag behind one with
 * it, the flag on the first entry (fewer than 2 phrase entries in front of the first flagged one),
 * or the flag on an OR / AND / MINMATCH entry is IRS_HIP_EINVAL.  A flagged entry carries its OWN
 * scorer values (the by_term's statistics and boost x the Or's boost), validated like any by_term
 * entry; its phrase_offset is ignored; the word entries carry the phrase's one scorer as always.
 * Phrase entries + flagged entries <= IRS_HIP_MAX_PHRASE_TERMS (more: IRS_HIP_EUNSUPPORTED); a
 * query or a batch that mixes this flag with IRS_HIP_PHRASE_ALT or IRS_HIP_PHRASE_REQUIRED is
 * IRS_HIP_EUNSUPPORTED; merge stays IRS_HIP_MERGE_SUM.  Per segment:
 *   d matches iff the phrase frequency pf(d) > 0 OR at least one optional term holds d (minus
 *   deleted docs and IRS_HIP_EXCLUDE terms);
 *   score(d) = [pf(d) > 0] s_phrase(tf = pf(d), norm(d)) + sum over the optional terms holding d of
 *   s_j(tf_j(d), norm(d)), in float32, entry order.
 * An absent phrase word (IRS_HIP_NO_TERM or no docs) empties the phrase child only: the terms still
 * match; an absent optional term adds nothing; everything absent empties the query in that
 * segment.  Execution is two passes over disjoint doc sets (the phrase's matches on k_phrase_or,
 * every other doc of the terms as a plain disjunction masked by the first pass's docs) and a merge
 * of their top k; total_hits, the top k, re-runs (irs_hip_batch_reruns counts both passes),
 * irs_hip_batch_configure, irs_hip_batch_set_shared_threshold, irs_hip_batch_set_min_scores and
 * the match sets (the union) behave as for any batch; irs_hip_batch_plan queues the first pass's
 * plan stage.  irs_hip_batch_set_doc_sets / _host and irs_hip_batch_set_comm on a batch with such a
 * query are IRS_HIP_EUNSUPPORTED (the second pass's doc sets are the first pass's output), and
 * irs_hip_batch_set_wand leaves both passes unpruned.  A batch with such
 * a query runs all its phrases on k_phrase_or, plain phrases giving bit for bit what they give in
 * a batch of their own.  A compatible addition to ABI 12: without the flag an entry means what it
 * always did, and a kind with the flag was IRS_HIP_EINVAL before (batch_create's scorer switch
 * took 0x800 | kind for an unknown scorer under every op). */
#define IRS_HIP_PHRASE_OPTIONAL 0x800

/* OR-ed into the `kind` of an included IRS_HIP_OP_PHRASE entry: that entry is the FIRST WORD OF A
 * FURTHER PHRASE — the query is the irs::And of its phrases, plus its required terms, minus its
 * excluded terms, `+"new york" +"real estate"` (And::prepare -> make_conjunction over
 * PhraseIterators and term iterators: boolean_filter.cpp:150-210, boolean_query.cpp:60-145,
 * conjunction.hpp:436-490).  Entry order in [first_term, first_term + n_terms):
 *   [words of phrase 1] [words of phrase 2, the first with this flag] ... [by_term children,
 *   IRS_HIP_PHRASE_REQUIRED] [IRS_HIP_EXCLUDE entries]
 * Every phrase has at least 2 words and the included entries are at most IRS_HIP_MAX_PHRASE_TERMS in
 * all (so at most four phrases; more entries: IRS_HIP_EUNSUPPORTED); up to IRS_HIP_MAX_EXCLUDED
 * excluded entries.  The phrase_offsets of a phrase are relative to its own first word, which
 * carries 0.  The words of ONE phrase carry one scorer (that phrase's FixedPrepareCollect blob, its
 * boost x the And's); different phrases may carry different values and kinds.
 * IRS_HIP_EINVAL: the flag under another op; on entry 0; on an entry that also carries
 * IRS_HIP_PHRASE_ALT, IRS_HIP_PHRASE_REQUIRED, IRS_HIP_PHRASE_OPTIONAL or is IRS_HIP_EXCLUDE; a
 * flagged entry with phrase_offset != 0; a phrase of one word; the flag behind an
 * IRS_HIP_PHRASE_REQUIRED entry; words of one phrase with differing scorer values; a merge other
 * than IRS_HIP_MERGE_SUM.  IRS_HIP_EUNSUPPORTED: more than IRS_HIP_MAX_PHRASE_TERMS included
 * entries; an IRS_HIP_PHRASE_ALT or IRS_HIP_PHRASE_OPTIONAL entry anywhere in such a query; such a
 * query in a batch that also holds variadic phrases or queries with optional terms, in either
 * order; a segment without positions.  Per segment:
 *   d matches iff every phrase has phrase frequency pf_i(d) > 0, every required term holds d, d is
 *   not deleted, lies in the unit's doc set if one is given, and no excluded term holds it;
 *   score(d) = the float32 sum over the And's children of s_phrase_i(tf = pf_i(d), norm(d)) resp.
 *   s_j(tf_j(d), norm(d)), the children in cost order as Conjunction sorts them
 *   (conjunction.hpp:450-453): a phrase costs the smallest docs_count of its words, a term its
 *   docs_count; ties in entry order — the rule IRS_HIP_PHRASE_REQUIRED states for one phrase.
 * An absent word or required term (IRS_HIP_NO_TERM or no docs) empties the query in that segment;
 * an absent excluded term changes nothing.  total_hits = the matching docs.  Such a query may share
 * a batch with plain phrases and with phrases plus required terms: the whole batch then runs on
 * k_phrases_and (irs_hip_batch_phrase_conj_units), a query with one phrase giving bit for bit what
 * it gives in a batch without such a query; every batch control behaves as for a batch with
 * required terms.  A query without the flag is untouched by all of this.  A compatible addition to
 * ABI 12: a kind with 0x2000 was IRS_HIP_EINVAL before (an unknown scorer). */
#define IRS_HIP_PHRASE_NEXT 0x2000

/* OR-ed into the `kind` of an included IRS_HIP_OP_PHRASE entry: that entry is the FIRST WORD OF AN
 * ALTERNATIVE PHRASE — the query is the irs::Or of its phrases, minus its excluded terms,
 * `"new york" OR "los angeles"` (Or::prepare prepares every child on its own,
 * boolean_filter.cpp:150-210; MakeDisjunction over PhraseIterators: basic_disjunction for two,
 * small_disjunction for up to five, disjunction.hpp:1411-1467, :208-350, :374-).  Entry order in
 * [first_term, first_term + n_terms):
 *   [words of phrase 1] [words of phrase 2, the first with this flag] ... [IRS_HIP_EXCLUDE entries]
 * Two to four phrases, each of at least 2 plain words, the included entries at most
 * IRS_HIP_MAX_PHRASE_TERMS in all; up to IRS_HIP_MAX_EXCLUDED excluded entries.  The phrase_offsets
 * of a phrase are relative to its own first word, which carries 0.  The words of ONE phrase carry one
 * scorer (that phrase's FixedPrepareCollect blob, its boost x the Or's); different phrases may carry
 * different values and kinds.
 * IRS_HIP_EINVAL: the flag under another op; on entry 0; on an IRS_HIP_EXCLUDE entry; a flagged
 * entry with phrase_offset != 0; a phrase of one word; words of one phrase with differing scorer
 * values; a merge other than IRS_HIP_MERGE_SUM.  IRS_HIP_EUNSUPPORTED: more than
 * IRS_HIP_MAX_PHRASE_TERMS included entries; an IRS_HIP_PHRASE_ALT, IRS_HIP_PHRASE_REQUIRED,
 * IRS_HIP_PHRASE_OPTIONAL or IRS_HIP_PHRASE_NEXT entry anywhere in such a query; such a query in a
 * batch that also holds a query with one of those four flags, in either order (plain phrases may
 * share the batch); a segment without positions.  Per segment:
 *   a phrase with an absent word (IRS_HIP_NO_TERM or no docs) is dropped in that segment — the other
 *   phrases go on matching; every phrase dropped: the unit is empty;
 *   d matches iff some present phrase has phrase frequency pf_i(d) > 0, d is not deleted, lies in the
 *   unit's doc set if one is given, and no excluded term holds it;
 *   score(d) = the float32 sum, in entry order, over the phrases with pf_i(d) > 0 of
 *   s_phrase_i(tf = pf_i(d), norm(d)); the sum starts from the first such phrase's value;
 *   total_hits = the matching docs, each counted once.
 * An absent excluded term changes nothing.  A batch with such a query runs all its phrase units on
 * k_phrases_or (irs_hip_batch_phrase_disj_units), a plain phrase giving bit for bit what it gives in a
 * batch without such a query; every batch control (doc sets, comm, shared threshold, min scores,
 * configure) behaves as for a batch of plain phrases.  irs_hip_batch_set_wand leaves these units
 * unpruned: a lead piece could be skipped only against a bound on the whole unit's score, and none is
 * kept per block.  A query without the flag is untouched by all of this.  A compatible addition to
 * ABI 12: a kind with 0x4000 was IRS_HIP_EINVAL before (an unknown scorer). */
#define IRS_HIP_PHRASE_OR 0x4000

/* The same bit OR-ed into the `kind` of an included IRS_HIP_OP_AND entry: one more member of the
 * group opened by the nearest preceding included entry without the flag — an And whose children
 * are Ors of by_term (And::prepare -> make_conjunction over the children, an Or child being its
 * own make_disjunction; boolean_filter.cpp:150-210, boolean_query.cpp:60-145).  A group is an Or
 * of its members (a plain by_term child is a group of one).  Per doc:
 *   d matches iff every group has a member holding d (minus deleted docs and IRS_HIP_EXCLUDE terms);
 *   group score s_g(d) = the sum of the scores of its members holding d (the inner Or merges
 *   with SUM); doc score = the query's `merge` (SUM / MAX / MIN) over the s_g(d), groups in cost
 *   order (the sum of their members' docs_count, as Conjunction sorts its children).
 * Boosts are the callers': each entry's c0 carries its term boost x Or boost x And boost.  At most
 * IRS_HIP_MAX_TERMS included entries in all; IRS_HIP_EXCLUDE entries may follow.  The flag on the
 * first included entry, on an IRS_HIP_EXCLUDE entry or on an OR / MINMATCH entry is IRS_HIP_EINVAL.
 * A term may appear in several groups; a term twice in one group scores once per appearance (an Or
 * of the same by_term twice).  Per segment an absent member (IRS_HIP_NO_TERM or no docs) is
 * dropped, and a group without a present member empties the query.  Such a query runs block driven
 * on k_conj_any (see irs_hip_batch_set_path for what the batch controls do with it).  A compatible
 * addition to ABI 12: a non-phrase kind with the flag was IRS_HIP_EINVAL before. */
#define IRS_HIP_GROUP_ALT IRS_HIP_PHRASE_ALT

/* OR-ed into the `kind` of an included IRS_HIP_OP_OR or IRS_HIP_OP_MINMATCH entry: one more REQUIRED
 * member of the clause opened by the nearest preceding included entry without the flag — an Or
 * whose children are by_term filters and Ands of by_term, `(a AND b) OR c` (Or::prepare prepares
 * every child on its own with ctx.boost x child boost, an And child becomes a conjunction, the Or a
 * disjunction or min-match disjunction over the children; boolean_filter.cpp:150-210,
 * boolean_query.cpp:60-145 and :212-247, conjunction.hpp:436-490, disjunction.hpp:1411-1467).  A
 * clause is one child of the Or (a plain by_term child is a clause of one).  Per segment, minus its
 * deleted docs:
 *   a clause matches d iff every one of its entries holds d; a clause with an absent entry
 *   (IRS_HIP_NO_TERM or no docs) is empty in that segment;
 *   d matches iff at least max(1, min_match) clauses match it (IRS_HIP_OP_OR: one); total hits
 *   counts these docs;
 *   score(d) = the sum, over the clauses matching d, of the sum of their entries' scores (SUM at
 *   both levels).
 * Boosts are the callers': each entry's c0 carries its term boost x And boost x Or boost; a zero
 * boost matches with score 0.  A term may stand in several clauses: it scores once per matched
 * clause that holds it and is decoded once.  Under IRS_HIP_OP_MINMATCH `min_match` counts CLAUSES:
 * 0 is IRS_HIP_EUNSUPPORTED as for every MINMATCH query, and a query with fewer non-empty clauses
 * than min_match (more than it has clauses, too) is empty in that segment.
 * IRS_HIP_EINVAL: the flag on the first included entry, on an IRS_HIP_EXCLUDE entry, on an AND,
 * PHRASE or MULTITERM entry.  IRS_HIP_EUNSUPPORTED: more than IRS_HIP_MAX_TERMS included entries;
 * a `merge` other than SUM; IRS_HIP_EXCLUDE entries; and what an entry scored from decoded streams
 * cannot be: a frequency above 255 in its term, a scorer outside the table family (BM1's constant
 * is taken) or more than 4 distinct (kind, norm_const, norm_length), wide or legacy norm columns.
 * Such a query runs on k_clause_pilot / k_clause_score (irs_hip_batch_clause_units), over the
 * streams the batch's joined units read, with 64-bit sums and a threshold of its own.  A batch that
 * holds one refuses irs_hip_batch_set_doc_sets / _host, irs_hip_batch_set_comm and
 * irs_hip_batch_match_sets* (IRS_HIP_EUNSUPPORTED); set_wand, set_path, set_paired_tiles and the
 * tile size leave these units as they are; its other (non-phrase) queries give bit for bit what they
 * give in a batch of their own.  A compatible addition to ABI 12: a kind with 0x1000 was
 * IRS_HIP_EINVAL before (an unknown scorer). */
#define IRS_HIP_CLAUSE_AND 0x1000

/* The `kind` of a NODE ENTRY: IRS_HIP_TREE_NODE | node op [| IRS_HIP_EXCLUDE].  A query whose entries
 * hold at least one node entry is a TREE QUERY — a boolean filter nested to any depth over by_term
 * leaves: `a AND (b OR (c AND d))`, `(a AND NOT b) OR c`, `+a +(b c d)~2` (And::prepare / Or::prepare
 * prepare every child on its own with ctx.boost x child boost, boolean_filter.cpp:55-312; an And
 * becomes a conjunction with its Not children as an exclusion, an Or a disjunction or min-match
 * disjunction: boolean_query.cpp:127-247, conjunction.hpp:436-490, disjunction.hpp:1411-1467,
 * exclusion.hpp).
 *   query.op      IRS_HIP_OP_OR, IRS_HIP_OP_AND or IRS_HIP_OP_MINMATCH: the ROOT's operator, and
 *                 query.min_match the root's
 *   entries       [first_term, first_term + n_terms): the root's children in prefix order; n_terms
 *                 counts every entry, node entries included
 *   a leaf        an ordinary scorer entry (by_term)
 *   a negated leaf  an IRS_HIP_EXCLUDE entry (Not(by_term)); under the tree flag it may stand wherever
 *                 a direct child of an And may, not only behind the included entries
 *   a node entry  opens a subtree: kind = IRS_HIP_TREE_NODE | node op (one of the three op values,
 *                 in the low byte), | IRS_HIP_EXCLUDE for Not(subtree); phrase_offset =
 *                 span | (min_match << 16), span = the entries of the subtree that follow the node
 *                 entry, min_match that of an IRS_HIP_OP_MINMATCH node (0 on the others); term, c0
 *                 and the norm fields are ignored
 * Per segment, minus its deleted docs, bottom up:
 *   a positive leaf matches the docs of its term; an absent term (IRS_HIP_NO_TERM or no docs)
 *   matches nothing;
 *   an And matches d iff every positive child matches d and no negated child does;
 *   an Or matches d iff at least max(1, min_match) of its children match d;
 *   d is a hit iff the root matches it; total hits counts these docs;
 *   score(d) is summed from the root down: a matching node contributes the scores of its positive
 *   children that match d — for an Or or min-match node EVERY matching child, not only min_match of
 *   them; negated children contribute nothing (SUM at every level).
 * So an And with an absent member is empty in that segment, an Or drops it, a min-match with too few
 * present children is empty, a Not of an absent term has no effect.  Boosts are the callers': a
 * leaf's c0 carries its boost times every ancestor's; a zero boost matches with score 0.  The same
 * term in two branches scores once per matching branch and is decoded once.
 * IRS_HIP_EINVAL: a span of 0 or one that runs past its parent; a node op outside the three; a
 * nonzero min_match on a node that is not IRS_HIP_OP_MINMATCH; a negated child of an Or / MINMATCH
 * node entry; a node entry under IRS_HIP_OP_PHRASE or IRS_HIP_OP_MULTITERM; the flag together with
 * any other flag but IRS_HIP_EXCLUDE, or any other flag on a leaf of such a query.
 * IRS_HIP_EUNSUPPORTED: more than 16 leaves (positive and negated together) or more than 15 node
 * entries; a `merge` other than SUM; an And (root or node) without a positive child; a negated
 * child of a root Or / MINMATCH; min_match 0 on a MINMATCH root or node, as for every MINMATCH
 * query; and what an entry scored from decoded streams cannot be (IRS_HIP_CLAUSE_AND above), the
 * frequencies of a negated leaf's term included.
 * Such a query runs on k_tree_pilot / k_tree_score (irs_hip_batch_tree_units), over the streams the
 * batch's joined units read, with 64-bit sums and a threshold of its own.  A batch that holds one
 * refuses irs_hip_batch_set_doc_sets / _host, irs_hip_batch_set_comm and irs_hip_batch_match_sets*
 * (IRS_HIP_EUNSUPPORTED); set_wand, set_path, set_paired_tiles and the tile size leave these units
 * as they are; its other (non-phrase) queries give bit for bit what they give in a batch of their
 * own.  A query without a node entry is validated exactly as before.  A compatible addition to
 * ABI 12: a kind with 0x8000 was IRS_HIP_EINVAL before (an unknown scorer). */
#define IRS_HIP_TREE_NODE 0x8000

/* One query term = the (term cookie, stats blob, boost) triple TermQuery::execute
 * hands to postings()/CompileScore (term_query.cpp:35-74), flattened. */
typedef struct irs_hip_term_scorer {
  uint32_t term;      /* ordinal in the segment's term table; IRS_HIP_NO_TERM = absent here */
  int32_t kind;       /* irs_hip_scorer_kind                                            */
  float c0;           /* BM25: boost*(k+1)*idf (bm25.cpp:201); TFIDF: boost*idf (tfidf.cpp:199) */
  float norm_const;   /* BM25Stats::norm_const  (bm25.hpp:52)                            */
  float norm_length;  /* BM25Stats::norm_length (bm25.hpp:54)                            */
  uint32_t phrase_offset; /* IRS_HIP_OP_PHRASE: position of the term relative to the phrase's
                             first term (FixedPhraseQuery::positions_t, phrase_filter.cpp
                             :279-284; 0 for the first); ignored by the other ops          */
} irs_hip_term_scorer;

/* boolean_filter::merge_type() — irs::ScoreMergeType (scorer.hpp:224-236) of an Or / And:
 * how the scores of the sub-queries on one doc combine.  The mergers are the reference's
 * (scorer.hpp:390-423), including what kMin does in a disjunction: it merges with the 0 of
 * every sub-query that is not on the doc, so an Or of two scores min(a, b) where both match
 * and 0 elsewhere, and an Or of three or more (block_disjunction's zeroed score buffer,
 * disjunction.hpp:1308-1351) scores 0 everywhere.  kNoop (no scores) is not offered. */
typedef enum irs_hip_merge {
  IRS_HIP_MERGE_SUM = 0,
  IRS_HIP_MERGE_MAX = 1,
  IRS_HIP_MERGE_MIN = 2
} irs_hip_merge;

typedef struct irs_hip_query {
  int32_t op;          /* irs_hip_op                                   */
  uint32_t n_terms;    /* included entries: 1..IRS_HIP_MAX_TERMS (PHRASE: ..IRS_HIP_MAX_PHRASE_TERMS;
                          with IRS_HIP_PHRASE_ALT members ..IRS_HIP_MAX_PHRASE_ENTRIES;
                          MULTITERM: ..IRS_HIP_MAX_WIDE_TERMS),
                          then 0..IRS_HIP_MAX_EXCLUDED IRS_HIP_EXCLUDE entries */
  uint32_t first_term; /* index of the first entry in the `terms` array */
  uint32_t k;          /* top-k, 1..IRS_HIP_MAX_K (index-search --topN) */
  uint32_t min_match;  /* IRS_HIP_OP_MINMATCH: Or::min_match_count(); IRS_HIP_OP_MULTITERM:
                          by_terms_options::min_match; else ignored */
  uint32_t merge;      /* irs_hip_merge (OR / AND / MINMATCH); PHRASE: IRS_HIP_MERGE_SUM */
} irs_hip_query;

/* (score, segment-local doc) exactly as utils/index-search.cpp:745-787 keeps. */
typedef struct irs_hip_hit {
  float score;
  uint32_t doc;
} irs_hip_hit;

typedef struct irs_hip_batch irs_hip_batch; /* opaque: one batch of queries on one segment */

/* Replaces, for a whole batch of prepared queries on one segment,
 *   filter::prepared::execute(ExecutionContext{segment, scorers, wand}) and the
 *   harness loop `while (docs->next()) { score; heap }` + final sort
 *   (filter.hpp:52-78, utils/index-search.cpp:719-787).
 * create : validates, uploads descriptors, sizes scratch (no query work).
 * run    : enqueues every kernel of the batch on `stream` (a hipStream_t, may
 *          be NULL = default stream); asynchronous.
 * results: waits for the stream and copies the per-query top-k to the host:
 *          hits[q * k_stride + i], i < counts[q], ordered (score desc, doc asc);
 *          total_hits[q] = number of matching docs (index-search `hits=`).
 * Results are deterministic: ties are broken by ascending doc id.
 * Lifetime / threading: a segment is immutable after open and may be shared by any
 * number of threads; a batch belongs to one thread at a time and must be destroyed
 * before its segment is closed.  results / results_to_device also verify the run
 * (candidate buffer, threshold estimate) and transparently re-execute the batch when
 * that check fails — irs_hip_batch_reruns counts those; results are exact either way. */
int irs_hip_batch_create(irs_hip_segment* seg, const irs_hip_query* queries,
                         uint32_t n_queries, const irs_hip_term_scorer* terms,
                         uint32_t n_term_entries, irs_hip_batch** out);
/* The same batch of queries over SEVERAL segments of one device in one go — what the
 * harness loop `for (auto& segment : reader)` (utils/index-search.cpp:719-779) does
 * segment after segment.  Every kernel is launched once for all (segment, query) pairs, so
 * small segments do not pay per-segment launch tails.  `terms` holds n_segs consecutive
 * arrays of n_term_entries entries: the same scorers (statistics are index-global,
 * term_filter.cpp:102-125) with each segment's own term ordinals.  All result calls then
 * index by unit = segment * n_queries + query: hits[unit * k_stride + i], counts[unit],
 * total_hits[unit]; irs_hip_merge_topk turns the per-segment lists into the global top-k.
 * Segments must live on the same device and use the same block layout. */
int irs_hip_batch_create_multi(irs_hip_segment* const* segs, uint32_t n_segs,
                               const irs_hip_query* queries, uint32_t n_queries,
                               const irs_hip_term_scorer* terms, uint32_t n_term_entries,
                               irs_hip_batch** out);
/* Executes the batch on `stream` (NULL: the default stream).  Asynchronous twice over: the
 * kernels are only queued, and the host half of a run — dealing the units to the kernels, building
 * the batch's posting streams and work lists, queueing uploads and launches (about 1 ms per 1000
 * queries) — is handed to a worker thread of the library (one per device), so that a serving loop
 * prepares batch i + 1 while batch i is being queued and batch i - 1 executes (the reference runs
 * its tasks on --threads workers, index-search.cpp:673-722).  Every other call on the batch waits
 * for that hand-over first; a failure of the run is returned by the next such call (results,
 * device_results, timings, destroy ...).  IRS_HIP_ASYNC_RUN=0 in the environment, or
 * irs_hip_batch_set_async(batch, 0) for one batch, keeps the host half on the caller's thread
 * (and the status in this call's return value).
 * What asynchronous means for the caller's own work on `stream`: when this returns, nothing of
 * the run may be on the stream yet.  An event the caller records, a kernel it launches or a
 * hipStreamSynchronize it makes right after is NOT ordered behind the run — get behind it with a
 * call on the batch (irs_hip_batch_device_results waits for the run; irs_hip_batch_results_to_device
 * / _to_host queue their copies behind it), or switch the hand-over off for that batch.  The same
 * holds for a device pointer obtained from irs_hip_batch_device_results BEFORE a re-run of the
 * batch: use it only behind a later call on the batch.
 * Nor is the END of a run ordered by `stream`: the library may queue the last kernels of a run on
 * a stream of its own.  A batch whose whole score stage is one paired launch of plain disjunctions
 * (no conjunction, phrase, multi-term or grouped unit, no shared threshold, no communicator) runs
 * its rescoring pass, its top-k selection and its status copy on the device's TAIL stream, beside
 * the pilot pass of the next batch queued on `stream`; the score launch of every later run on the
 * device waits for that tail.  irs_hip_batch_results* (also _to_device / _to_host, which queue
 * their copies behind the run's end), irs_hip_batch_device_results, irs_hip_batch_timings and
 * irs_hip_batch_destroy get behind the whole run, a hipStreamSynchronize(stream) does not.
 * IRS_HIP_TAIL_STREAM=0 in the environment when a batch is created keeps its runs on `stream`
 * from end to end (A/B runs, tests); the results are the same either way.
 * irs_hip_batch_tail_stream_used: whether the batch's last run took the tail stream. */
int irs_hip_batch_run(irs_hip_batch* batch, void* stream);
int irs_hip_batch_tail_stream_used(irs_hip_batch* batch, int* used);
/* Per batch: 1 = hand the host half of irs_hip_batch_run to the library's worker thread, 0 = keep
 * it on the caller's thread, -1 = the process default (on; IRS_HIP_ASYNC_RUN=0 turns it off).  A
 * batch with a communicator (irs_hip_batch_set_comm) issues its collectives — also those of a
 * recovery re-run — in the order of the calls made on this device either way. */
int irs_hip_batch_set_async(irs_hip_batch* batch, int enable);
/* Optional: queue the PLANNING stage of the batch's next run (tile tables, work items: what
 * building the iterator tree is to filter::prepared::execute) on `stream` now; the next
 * irs_hip_batch_run then only waits for it (an event) and starts with scoring.  The stage reads
 * and writes nothing another batch's run touches, so with two streams a caller overlaps the
 * planning of batch i+1 with the scoring kernels of batch i.  Without this call run() plans
 * inline, as before. */
int irs_hip_batch_plan(irs_hip_batch* batch, void* stream);
int irs_hip_batch_results(irs_hip_batch* batch, irs_hip_hit* hits,
                          uint32_t k_stride, uint32_t* counts,
                          uint64_t* total_hits);
/* Device-resident results for a caller that merges on the GPU (RCCL path): waits for
 * and verifies the run like `results`, then hands out the batch's own buffers:
 * d_hits is [n_queries][k_max] irs_hip_hit, d_counts [n_queries] uint32. */
int irs_hip_batch_device_results(irs_hip_batch* batch, void** d_hits,
                                 void** d_counts, uint32_t* k_max);
/* Same, copied (device to device, async on `stream`) into caller-owned device
 * buffers: d_hits [n_queries][k_max] irs_hip_hit, d_counts [n_queries] uint32. */
int irs_hip_batch_results_to_device(irs_hip_batch* batch, void* d_hits,
                                    void* d_counts, void* stream);
void irs_hip_batch_destroy(irs_hip_batch* batch);

/* Convenience: create + run + results + destroy. */
int irs_hip_query_batch(irs_hip_segment* seg, const irs_hip_query* queries,
                        uint32_t n_queries, const irs_hip_term_scorer* terms,
                        uint32_t n_term_entries, irs_hip_hit* hits,
                        uint32_t k_stride, uint32_t* counts,
                        uint64_t* total_hits);

/* The checked results of the batch's last run on their way to page-locked HOST memory owned by
 * the batch — where the reference's harness ends (index-search.cpp:782-807) — without stalling the
 * caller: results_to_host verifies the run (like irs_hip_batch_device_results) and queues the copy on
 * `stream` (NULL: the device's download stream) behind the batch's own kernels only, so the hits of
 * batch i cross PCIe while batch i + 1 executes; host_results waits for that copy and hands out the
 * arrays: hits [n_queries][*k_stride] (score desc, doc asc; counts[q] valid entries), counts
 * [n_queries], total_hits [n_queries].  They stay valid until the batch is destroyed, run again or
 * copied again. */
int irs_hip_batch_results_to_host(irs_hip_batch* batch, void* stream);
int irs_hip_batch_host_results(irs_hip_batch* batch, const irs_hip_hit** hits, uint32_t* k_stride,
                               const uint32_t** counts, const uint64_t** total_hits);

/* Tuning knobs (0 keeps the default). tile_docs in {4096, 6144, 8192, 12288}: docs
 * per LDS accumulator tile (default: the largest one that lets two workgroups share
 * a compute unit's LDS, 12288 with 32-bit and 6144 with 64-bit accumulators);
 * pilot_stride P: every P-th doc tile is scored first to bound the k-th score
 * (P == 1: exact two-pass); cand_cap: candidate slots per query.  Results do not
 * depend on any of them. */
int irs_hip_batch_configure(irs_hip_batch* batch, uint32_t tile_docs,
                            uint32_t pilot_stride, uint32_t cand_cap);

/* How the doc-tile units of a batch (Or / by_term / min-match, conjunctions that qualify)
 * execute — a tuning / test knob; the hits of plain disjunctions are BIT-IDENTICAL on every path
 * (units with match counts — conjunctions, min-match — differ by the rounding of their counting
 * accumulators when they join, within the parity tolerance):
 *   IRS_HIP_PATH_ITEMS   every query decodes the blocks of its own terms (work items);
 *   IRS_HIP_PATH_JOINED  every DISTINCT (segment, term) of the batch is decoded once per run
 *                        into streams of entries which the queries then only accumulate — what
 *                        block_disjunction::refill (disjunction.hpp:1240-1351) does per query,
 *                        shared by the queries of a batch (what AUTO takes when it joins).
 *                        For sum-merged units with table-family
 *                        scorers (BM25 / BM15 / TF-IDF over 1-byte norms or none), frequencies
 *                        < 256 — plain disjunctions, and conjunctions / min-match disjunctions of
 *                        at most 15 terms whose counting accumulators stay within the parity
 *                        tolerance; units that do not qualify run as ITEMS whatever was asked —
 *                        so does every unit with excluded terms (IRS_HIP_EXCLUDE): its own
 *                        mask of docs cannot ride on streams shared with other units (an
 *                        Or / min-match unit runs as work items, an And block driven, a
 *                        phrase on its phrase kernel) — and every unit restricted to a doc set
 *                        (irs_hip_batch_set_doc_sets), whose mask is one more of that kind;
 *   IRS_HIP_PATH_AUTO    (default) by measured cost: plain disjunctions join when the batch's
 *                        streams are shared enough or its units many enough to pay for decoding
 *                        every distinct stream once (2.9 ps per distinct posting against 0.67 ps
 *                        per referenced posting + 2.4 ns per (unit, doc tile) saved —
 *                        tools/cost_sweep.py); a conjunction joins when walking every entry of
 *                        its terms beats decoding only the blocks its rarest term's docs fall
 *                        into.
 * Grouped conjunctions (IRS_HIP_GROUP_ALT) never join posting streams: like units with excluded
 * terms they run block driven (k_conj_any) whatever the path, and the other units of the batch
 * choose their paths as they would without them.  irs_hip_batch_set_wand leaves them exhaustive (no
 * block-max pruning: the top k is exact and total_hits the full count);
 * irs_hip_batch_set_min_scores applies to them; under irs_hip_batch_set_shared_threshold /
 * irs_hip_batch_set_comm they keep thresholds of their own; irs_hip_batch_work / _touched
 * account for them as for block-driven conjunctions.
 * Call before the batch's first run (or after a configure). */
enum { IRS_HIP_PATH_AUTO = 0, IRS_HIP_PATH_ITEMS = 1, IRS_HIP_PATH_JOINED = 2 };
int irs_hip_batch_set_path(irs_hip_batch* batch, int path);
/* Which one the batch's last run used (IRS_HIP_PATH_ITEMS / IRS_HIP_PATH_JOINED). */
int irs_hip_batch_path(irs_hip_batch* batch, int* path);

/* Paired doc tiles for the joined plain disjunctions (ABI 12; on by default) — a tuning / test
 * knob like set_path: a visit of k_join_score then covers two consecutive doc tiles whose sums
 * share an accumulator word (16 bits each, contributions rounded up), which only PICKS the docs;
 * their exact 32-bit sums are formed afterwards from the streams (k_join_rescore) with the
 * arithmetic of the unpaired kernel, so hits, scores, order and totals are BIT-IDENTICAL either
 * way.  enable = 1 (default): taken where it pays — the visits saved (doc tiles per unit) against
 * the look-ups added (about min(3 k / units sharing the threshold, k) docs per term): a 10 M-doc
 * segment at k = 1000 pairs, a lone 1.25 M-doc segment does not — unless a segment of the batch's
 * plain joined units has deleted documents; enable = 2: whatever the size (tests); enable = 0:
 * never — the units run on 32-bit tiles.  Whatever enable says, a launch one of whose terms has no
 * bound image (irs_hip_join_bound_rule: IRS_HIP_EUNSUPPORTED for its scorer signature; a segment
 * without frequencies) keeps its 32-bit tiles: enable = 2 asks for pairs, it does not guarantee
 * them.  Units with excluded terms (IRS_HIP_EXCLUDE) never join
 * and so never take paired tiles; the other units of their batch decide as without them.
 * irs_hip_batch_paired_tiles: whether the last run took them. */
int irs_hip_batch_set_paired_tiles(irs_hip_batch* batch, int enable);
int irs_hip_batch_paired_tiles(irs_hip_batch* batch, int* used);

/* A batch over several segments (irs_hip_batch_create_multi) whose per-segment lists the caller
 * MERGES into one top k per query — what the harness does with its segments
 * (index-search.cpp:719-787) and what irs_hip_merge_topk does here: with `enable` the units of a
 * query share ONE score threshold, chosen so that the segments TOGETHER yield the k best docs
 * (plus the usual margin) instead of every segment its own k.  A segment's list then holds every
 * doc of it at or above the shared threshold — possibly fewer than k although more matched — and
 * the merged top k is exactly what it is without the option; total_hits are unchanged.  The
 * candidate volume, which is what small segments spend their time on, drops by the number of
 * segments.  Applies to units on joined posting streams whose scorers bound the score alike in
 * every segment (BM25 family); other units keep their own thresholds.  Off by default; call
 * before the batch's first run (or after a configure). */
int irs_hip_batch_set_shared_threshold(irs_hip_batch* batch, int enable);

/* ExecutionContext::wand (filter.hpp:52-78; utils/index-search --search-mode wand): lets the
 * batch SKIP posting blocks that cannot reach the top k.  The bound of a block is the query
 * term's own score function on the block's (max freq, min norm) — what the wanderator
 * evaluates per skip entry (formats_10.cpp:2498-2528, wand_writer.hpp:302-342) — summed over
 * the terms of a conjunction for the blocks overlapping one doc range (BlockConjunction,
 * conjunction.hpp:380-426); the threshold is the pilot pass's lower bound of the k-th score.
 * The top k (docs, scores, order) is the one the exhaustive run returns
 * (tests/search/wand_test.cpp:231-241); total_hits only counts the docs that were evaluated,
 * as with the reference's wand mode.  The per-block (max freq, min norm) are derived from the
 * postings on first use (every block gets them, also the last one of a list, for which the
 * skip data has no entry) and kept with the segment.  Applies to IRS_HIP_OP_AND queries on the
 * block-driven kernel and to whole doc tiles of OR queries on the work-item kernel; a unit the
 * cost rules put on joined posting streams (irs_hip_batch_set_path) is executed exhaustively —
 * its top k is the exhaustive one by construction, its total_hits the full count.  Call before
 * the batch's first run. */
int irs_hip_batch_set_wand(irs_hip_batch* batch, int enable);

/* irs::score::Min (score_function.hpp:42-142): the threshold the harness pushes into the
 * iterator once its heap is full — the k-th best score so far, carried over from the segments
 * it executed before (utils/index-search.cpp:737, 756, 777).  min_scores: [n_queries] floats
 * >= 0 (0 = none), or NULL to clear.  A doc scoring below min_scores[q] is not competitive: the
 * batch may drop it (pruning then starts from that bound instead of from the pilot pass's
 * estimate alone), so a query returns exactly the docs scoring at or above its threshold,
 * at most k of them, in the usual order — possibly fewer than k (the kernels drop by score bin,
 * the final selection by the score itself); total_hits still counts every match.  May be
 * called between runs. */
int irs_hip_batch_set_min_scores(irs_hip_batch* batch, const float* min_scores);
/* The block-max data of one term, for inspection/tests (computed as for set_wand): largest
 * frequency and smallest non-zero norm of every full 128-doc block. */
int irs_hip_term_blockmax(irs_hip_segment* seg, uint32_t term, uint32_t* max_freqs,
                          uint32_t* min_norms, uint32_t cap, uint32_t* count);
/* Where the block-max pairs of a segment come from: blocks whose pair was READ from the index's
 * own wand data — the payload of scorer 0 in the level-0 skip entries (FreqNormSource::Read,
 * wand_writer.hpp:318-334), present when the field was indexed with scorers
 * (irs_hip_segment_desc.wand_count > 0) — out of all full blocks; the others (every block of an
 * index written without wand data, the last block of every list, the norm where the payload
 * only carries a frequency) are derived from the postings.  A field with positions must have
 * been opened with its `.pos` for the entries to be read (they carry position fields). */
int irs_hip_segment_wand_source(irs_hip_segment* seg, uint64_t* from_index, uint64_t* total);

/* Kernel timing with HIP events recorded on the batch's own stream.
 * When enabled, every run() brackets each kernel launch with events;
 * timings() waits for the stream and returns the durations (ms) of the last run. */
enum {
  IRS_HIP_K_PLAN = 0,   /* block-range planning per (query, term) + work items; joined path:
                           the decode + norm join of the batch's distinct terms (k_join);
                           the masks of units with excluded terms (k_excl_mask) */
  IRS_HIP_K_PILOT = 1,  /* pilot tiles -> per-query score threshold */
  IRS_HIP_K_SCORE = 2,  /* decode + score + accumulate + candidates (phrase batches: k_phrase) */
  IRS_HIP_K_SELECT = 3, /* exact top-k of the candidates            */
  IRS_HIP_K_COUNT = 4
};
/* enable: bit 0 = time the kernels (below); bit 1 = let the block-driven kernels count what
 * they decode (irs_hip_batch_touched) — a diagnostic run: the counting costs atomics. */
int irs_hip_batch_profile(irs_hip_batch* batch, int enable);
int irs_hip_batch_timings(irs_hip_batch* batch, float ms[IRS_HIP_K_COUNT]);
/* Work accounting for the roofline: algorithmic bytes A(q)
 * summed over the batch = posting bytes of every query term (excluded terms included: their
 * doc blocks are read) + 1 norm byte per scored posting (norm_width) + 8*k result bytes
 * + (num_docs + 7) / 8 bytes per unit restricted to a doc set (its row is read); and the
 * number of scored postings. */
int irs_hip_batch_work(irs_hip_batch* batch, uint64_t* algorithmic_bytes,
                       uint64_t* postings);
/* What the last run of a conjunction / phrase batch really read, next to the algorithmic
 * bytes above ("report both A(q) and bytes actually touched"): encoded bytes of
 * the `.doc` blocks it decoded plus the norm bytes it read, and the number of positions it
 * read from `.pos`.  (Doc-tile batches read every block of every term: A(q).)  Needs
 * irs_hip_batch_profile(batch, 2 | ...) before the run. */
int irs_hip_batch_touched(irs_hip_batch* batch, uint64_t* doc_bytes, uint64_t* positions);
/* How many times fetching results had to re-execute the batch so far: the pilot's
 * estimated threshold left fewer than k candidates for some query (re-run with the
 * provable threshold), or the candidate buffer overflowed (exact re-run, then a
 * larger buffer).  Results are exact either way; this only tells what it cost. */
int irs_hip_batch_reruns(irs_hip_batch* batch, uint32_t* count);

/* The doc mask unit `unit` (= segment * n_queries + query) ran with in the batch's last run, for
 * inspection/tests, in irs_hip_bit_union's layout (bit `doc` of 64-bit little-endian words,
 * n_words of them, docs beyond dropped): the segment's deleted docs plus every doc of the unit's
 * excluded terms plus — for a unit restricted to a doc set (irs_hip_batch_set_doc_sets) — every doc
 * 1..num_docs that is not in its row; just the deleted docs for a unit without excluded terms and
 * without a doc set (an empty set when the segment has none).  Waits for the run. */
int irs_hip_batch_unit_mask(irs_hip_batch* batch, uint32_t unit, uint64_t* set, uint64_t n_words);

/* filter::prepared::execute with Scorers::kUnordered (core/search/filter.hpp:52-78): the docs every
 * unit of the batch matches, all of them, unscored — what a search without a sort, a count and
 * proxy_filter's cached bitsets (proxy_filter.hpp, bitset_doc_iterator.hpp) run.
 * Unit u = segment * n_queries + query, as for irs_hip_batch_unit_mask.  `sets` is
 * [n_units][n_words] in irs_hip_bit_union's layout (64-bit little-endian words, bit index = doc
 * id): every word of every row is written, nothing is OR-ed into old content.  `counts` is
 * [n_units], the population of each row — the total_hits a scored run of the batch reports.
 * n_words must cover the largest segment of the batch, 64 * n_words > num_docs, else
 * IRS_HIP_EINVAL.  Either output may be NULL (sets == NULL: only 8 bytes per unit leave the
 * device); both NULL is IRS_HIP_EINVAL.
 * A doc matches as in a scored run — Or: an entry holds it; And: every group has a member that
 * holds it; min-match: at least min_match entries hold it — and is neither deleted nor a doc of an
 * excluded term (IRS_HIP_EXCLUDE).  Scorer values, k, merge and every setter of the batch
 * (set_wand, set_min_scores, set_path, set_paired_tiles, shared thresholds, set_comm) play no part;
 * the sets are this rank's, nothing is gathered.  The call may come before, after or without
 * irs_hip_batch_run and leaves the batch's results, irs_hip_batch_reruns and later runs as they
 * would have been.  A phrase matches where its phrase frequency is > 0.  (A segment without
 * frequencies has no batch: irs_hip_batch_create refuses it, IRS_HIP_EUNSUPPORTED.)
 * Synchronous, like irs_hip_bit_union_counts; the staging memory comes from the pool
 * (IRS_HIP_ENOMEM when it cannot be had). */
int irs_hip_batch_match_sets(irs_hip_batch* batch, uint64_t* sets, uint64_t n_words, uint64_t* counts);
/* The same into device memory (d_sets [n_units][n_words] u64, d_counts [n_units] u64; either may
 * be NULL), queued on `stream` as irs_hip_batch_results_to_device queues its copies: the
 * disjunction's doc set handed to a consumer on the device (bitset_doc_iterator.hpp). */
int irs_hip_batch_match_sets_to_device(irs_hip_batch* batch, void* d_sets, uint64_t n_words,
                                       void* d_counts, void* stream);

/* doc_iterator::seek(target) + score for docs the CALLER names (formats_10.cpp:2304-2365; a
 * conjunction seeks its other children to the lead's doc, conjunction.hpp:207-223) — a compatible
 * addition to ABI 12.  What a GPU-backed query needs to sit under a host conjunction whose other child
 * this library never runs, and what scores the candidates another retriever returned.
 * Unit u = segment * n_queries + query.  Unit u's docs are docs[offsets[u] .. offsets[u + 1]),
 * strictly ascending, each in 1..num_docs of the unit's segment; `offsets` has n_units + 1 entries,
 * offsets[0] == 0, non-decreasing (an empty list is allowed).
 *   scores[i]   the score irs_hip_batch_run gives doc i under its unit, 0 where it does not match
 *   matched[i]  1 / 0 (matched may be NULL)
 * Matching and score are exactly what the unit's scored run defines for that doc: the segment's
 * deleted docs, the unit's IRS_HIP_EXCLUDE entries and its doc set (irs_hip_batch_set_doc_sets) do
 * not match; an absent term behaves as in a run (an And with one is empty, an Or drops it); the
 * merge is the unit's (a kMin disjunction of three or more scores 0); a zero boost matches with
 * score 0.  k, min scores, wand, the path, paired tiles, a shared threshold and a communicator play
 * no part.  Like irs_hip_batch_match_sets the call may come before, after or without
 * irs_hip_batch_run and leaves the batch's results, irs_hip_batch_reruns and later runs as they
 * would have been.
 * Units taken: every unit of at most IRS_HIP_MAX_TERMS rows — OR / AND / MINMATCH with SUM / MAX /
 * MIN, IRS_HIP_GROUP_ALT, IRS_HIP_CLAUSE_AND, IRS_HIP_TREE_NODE, with or without IRS_HIP_EXCLUDE
 * entries, on one or several segments.  Clause and tree units, whose runs sum 64-bit fixed point,
 * are summed in float32 here: equal within the 1e-5 the scores are held to.
 * IRS_HIP_EUNSUPPORTED: a batch that holds IRS_HIP_OP_PHRASE or IRS_HIP_OP_MULTITERM units; more
 * than 2^31 docs in all.  IRS_HIP_EINVAL: a NULL batch, docs, offsets or scores; offsets[0] != 0;
 * decreasing offsets; a doc of 0, a doc above its segment's num_docs, a list that does not ascend
 * strictly.  Synchronous; the staging memory comes from the pool (IRS_HIP_ENOMEM). */
int irs_hip_batch_score_docs(irs_hip_batch* batch, const uint32_t* docs, const uint64_t* offsets,
                             float* scores, uint8_t* matched);
/* The same on device memory (d_docs u32[n_docs], d_offsets u64[n_units + 1], d_scores f32[n_docs],
 * d_matched u8[n_docs] or NULL), queued on `stream`; n_docs = offsets[n_units].  The host cannot
 * validate what it does not read: the kernel reports every doc of 0 or above its segment's num_docs
 * as unmatched, and every doc of a chunk (at most 128 consecutive docs of one list) that does not
 * ascend strictly as unmatched; no address is ever formed from an unverified doc or offset —
 * offsets that are not 0-based, non-decreasing and <= n_docs leave outputs unwritten, nothing more.
 * The call returns IRS_HIP_OK in all these cases.  d_docs and d_offsets stay valid and unchanged
 * until the stream has run the call. */
int irs_hip_batch_score_docs_to_device(irs_hip_batch* batch, const void* d_docs, const void* d_offsets,
                                       uint64_t n_docs, void* d_scores, void* d_matched, void* stream);

/* ByNestedFilter, the block join (core/search/nested_filter.{hpp,cpp}) — a compatible addition to
 * ABI 12.  Child documents are stored in front of their parent; the batch's queries are the CHILD
 * filter; the hits are the parents whose block of children satisfies a match rule, scored by a merge
 * of their children's scores.
 * Inputs.  Unit u = segment * n_queries + query, as everywhere.  d_parents: per segment of the batch
 * one row of a device bitset, [n_segs][n_words] u64 in irs_hip_bit_union's layout (bit index = doc
 * id); bit 0 and the bits above the segment's num_docs are ignored.
 * Blocks.  P = the parent docs of the unit's segment, prev(p) = the largest parent below p (0 if
 * none): the block of p is the docs in (prev(p), p) — ChildToParentJoin::FirstChildApprox /
 * SeekInternal, nested_filter.cpp:165-186.  Docs above the last parent belong to nobody.
 * The unit's child set C is what irs_hip_batch_match_sets returns for the unit — so without the
 * segment's deleted docs, the unit's IRS_HIP_EXCLUDE terms and its doc set — with EVERY PARENT DOC
 * REMOVED.  That is a definition made here: the reference assumes the child filter matches no
 * parent, and its matchers disagree about what happens when it does (AnyMatcher::Accept :272-276
 * skips such a hit, RangeMatcher / MinMatcher :393-440, :474-522 count it).
 * Matching.  c(p) = |C ∩ block(p)|.  A parent is a hit iff it is not deleted in the segment and
 * match_min <= c(p) <= match_max; match_max = IRS_HIP_NESTED_NO_MAX: no maximum.  A deleted parent
 * still delimits blocks.
 *   {0, 0}       kMatchNone :242-263   c(p) == 0; every hit scores none_boost
 *   {1, none}    kMatchAny  :265-299   c(p) >= 1
 *   {min, none}  MinMatcher :461-555   c(p) >= min; min == 0: every live parent
 *   {min, max}   RangeMatcher :377-459 min <= c(p) <= max
 * Score of a hit (except under {0, 0}): the merge (IRS_HIP_MERGE_SUM / MAX / MIN) over the scores of
 * the children in C ∩ block(p), each what irs_hip_batch_score_docs gives it under the unit, merged in
 * float32 in ascending doc order, the value starting from the first child's score (child_score(res)
 * then merger(res, temp), :292-296, :426-436).  A hit with c(p) == 0 scores 0.  A quirk kept: under
 * {0, none} the buffer starts from 0 (:477-485, :539-547) — SUM and MAX are unaffected, MIN scores 0
 * for every parent.
 * Results.  total_hits[u] = the hit parents; the top k is the unit's query's own k, ordered (score
 * desc, doc asc).  k, min scores, wand, the path, paired tiles, a shared threshold and a communicator
 * of the child batch play no part.  Like irs_hip_batch_match_sets the calls may come before, after or
 * without irs_hip_batch_run and leave the batch's results, irs_hip_batch_reruns and later runs as
 * they would have been.  Nothing is pruned (the reference prunes nothing either: :644).
 * Not offered: the predicate form of `match` (PredMatcher), kNoop merges.
 * IRS_HIP_EINVAL: a NULL batch, descriptor or d_parents; 64 * n_words <= num_docs of a segment of the
 * batch or n_words > 2^26; match_min > match_max; a merge outside the three; a negative or non-finite
 * none_boost; k_stride below the batch's largest k; every output NULL.  IRS_HIP_EUNSUPPORTED, all
 * calls: what irs_hip_batch_match_sets refuses (IRS_HIP_OP_MULTITERM, IRS_HIP_CLAUSE_AND,
 * IRS_HIP_TREE_NODE units); _topk in addition: what irs_hip_batch_score_docs refuses
 * (IRS_HIP_OP_PHRASE units) — except under {0, 0}, which needs no child score; a unit with 2^31 or
 * more hit parents, or children under them.  IRS_HIP_ENOMEM: the pool cannot serve the scratch (the
 * child rows, [n_units][n_words] u64; for _topk the hit rows too, and per group of units the
 * children's lists, their scores and the candidate keys: IRS_HIP_NESTED_SCRATCH_MB, read per call,
 * default 256, bounds a group — a batch that exceeds it runs in several groups, never fails for it). */
#define IRS_HIP_NESTED_NO_MAX 0xFFFFFFFFu
typedef struct irs_hip_nested {
  const void* d_parents;  /* device, [n_segs][n_words] u64; borrowed for the call */
  uint64_t n_words;       /* 64 * n_words > num_docs of every segment of the batch, <= 2^26 */
  uint32_t match_min, match_max;
  uint32_t merge;         /* irs_hip_merge */
  float none_boost;       /* used under {0, 0} only; >= 0 */
} irs_hip_nested;
/* The hit parents of every unit, unscored: rows [n_units][n_words] (every word written, those beyond
 * the segment as 0) and / or their populations; either output may be NULL, not both.  Synchronous. */
int irs_hip_batch_nested_sets(irs_hip_batch* batch, const irs_hip_nested* nested, uint64_t* sets,
                              uint64_t* counts);
/* The same into device memory (d_sets [n_units][n_words] u64, d_counts [n_units] u64), on `stream`,
 * so that a nested filter chains into irs_hip_batch_set_doc_sets of a parent-level batch without the
 * rows crossing to the host.  The child rows are scratch of the call: it returns when the stream has
 * run it. */
int irs_hip_batch_nested_sets_to_device(irs_hip_batch* batch, const irs_hip_nested* nested, void* d_sets,
                                        void* d_counts, void* stream);
/* The k best hit parents of every unit: hits[u * k_stride + i], counts[u], total_hits[u] (any of
 * them may be NULL, not all).  Synchronous. */
int irs_hip_batch_nested_topk(irs_hip_batch* batch, const irs_hip_nested* nested, irs_hip_hit* hits,
                              uint32_t k_stride, uint32_t* counts, uint64_t* total_hits);

/* Doc-set filters (a compatible addition to ABI 12): the units of a batch restricted to doc sets on
 * the device — the conjunction of a scored query with an UNSCORED child: the bitset_doc_iterator a
 * multi-term query builds from its unscored terms (multiterm_query.cpp:36-87, 133-166), a
 * column-existence filter, proxy_filter's cached bitset.  MakeConjunction leaves such a child out
 * of the score (conjunction.hpp:461-467): it only decides which docs match.
 *   d_sets       device memory, [n_rows][n_words] u64 in irs_hip_bit_union's layout (64-bit
 *                little-endian words, bit index = doc id) — what irs_hip_batch_match_sets_to_device
 *                and irs_hip_bit_union produce.  The row stride is n_words and may be larger than a
 *                segment needs; bit 0 and the bits of docs beyond a segment's num_docs are ignored.
 *   row_of_unit  host array [n_units], unit = segment * n_queries + query as for
 *                irs_hip_batch_unit_mask; copied.  IRS_HIP_NO_DOC_SET: the unit is unrestricted.
 * row_of_unit == NULL or n_rows == 0 clears the filters.  IRS_HIP_EINVAL: a row index >= n_rows;
 * 64 * n_words <= num_docs of a segment that has a restricted unit; n_words > 2^26 (no segment has
 * that many docs: the limit irs_hip_batch_match_sets puts on its rows) while a row is referenced;
 * d_sets == NULL while a row is referenced.
 * A restricted unit matches what it matches without the filter (the included part, minus deleted
 * docs, minus the docs of IRS_HIP_EXCLUDE terms) intersected with its row: scores, order and merge
 * do not change, total_hits counts what remains and the top k is drawn from it — for every op (OR,
 * AND incl. IRS_HIP_GROUP_ALT, MINMATCH, PHRASE incl. IRS_HIP_PHRASE_ALT / IRS_HIP_PHRASE_REQUIRED)
 * and for irs_hip_batch_match_sets*: a filtered batch's match sets are the intersections, so
 * filters chain.  Scorer statistics are the caller's and do not change (the reference's are index
 * statistics).
 * The device form BORROWS d_sets: the words are read by the stage that builds the unit masks —
 * irs_hip_batch_plan if the caller uses it, else irs_hip_batch_run — on that call's stream, and
 * again in every recovery re-run, so they must stay valid and unchanged until the batch's results
 * have been fetched or the filters are replaced or cleared.  A producer queued earlier on the same
 * stream is seen without a host synchronisation.  The host form copies the rows into pool memory of
 * the batch (IRS_HIP_ENOMEM when it cannot be had: the batch is then left without filters).
 * Call before the batch's first run or between runs; the units are dealt again as after
 * irs_hip_batch_configure.  A restricted unit takes the path of a unit with excluded terms
 * (irs_hip_batch_set_path) and is treated like one by set_wand, set_min_scores, shared thresholds
 * and set_comm; the unrestricted units of the batch choose their paths and give their results bit
 * for bit as without the filters.  Whole doc tiles in which a restricted work-item unit can match
 * nothing get no work items and are not visited; its count stays exact. */
#define IRS_HIP_NO_DOC_SET 0xFFFFFFFFu
int irs_hip_batch_set_doc_sets(irs_hip_batch* batch, const void* d_sets, uint64_t n_rows,
                               uint64_t n_words, const uint32_t* row_of_unit);
int irs_hip_batch_set_doc_sets_host(irs_hip_batch* batch, const uint64_t* sets, uint64_t n_rows,
                                    uint64_t n_words, const uint32_t* row_of_unit);
/* What the doc sets let the batch's last run skip (waits for it).  tiles / tiles_skipped: the doc
 * tiles of the restricted units that ran as work items, and how many of them held no doc their
 * unit's mask leaves (no work items, no visit) — exact.  leads / leads_skipped: lead pieces (the
 * lead-item records: blocks of the lead term, or their pieces) of the restricted block-driven and
 * phrase units in the last run's full pass, and how many ended after their own decode because none
 * of their docs was left — counted only under irs_hip_batch_profile bit 1 (the counting mode: it
 * costs atomics), 0 otherwise.  Any output may be NULL. */
int irs_hip_batch_doc_set_stats(irs_hip_batch* batch, uint64_t* tiles, uint64_t* tiles_skipped,
                                uint64_t* leads, uint64_t* leads_skipped);

/* Multi-segment / multi-GPU merge: merges `n_lists` per-query
 * top-k lists (device pointers, each [n_queries][k] hits + [n_queries] counts,
 * list i belonging to segment ordinal seg_ids[i]) into the global top-k ordered
 * (score desc, segment asc, doc asc) — the order tests/search/wand_test.cpp:72-86
 * defines.  Outputs are device pointers: d_out [n_queries][k] hits,
 * d_out_seg [n_queries][k] uint32, d_out_counts [n_queries]. */
int irs_hip_merge_topk(int32_t device, const void* const* d_lists,
                       const void* const* d_counts, const uint32_t* seg_ids,
                       uint32_t n_lists, uint32_t n_queries, uint32_t k,
                       void* d_out, void* d_out_seg, void* d_out_counts,
                       void* stream);

/* ---- the collective of the multi-GPU exchange --------------------------
 * One process per GPU.  The per-segment top-k lists of a step — [n_queries][k] hits and
 * [n_queries] counts per local segment, written by irs_hip_batch_results_to_device straight
 * into one send buffer — are exchanged with ONE all-gather over RCCL (xGMI); every rank then
 * merges them with irs_hip_merge_topk.  What the harness loop `for (auto& segment : reader)`
 * into one heap (utils/index-search.cpp:719-779) becomes when the segments live on different
 * GPUs.  irs_hip_comm_unique_id: on one rank; the caller distributes the 128 bytes to the
 * others by whatever it has (MPI, a file, a socket), exactly as with ncclUniqueId. */
/* Device buffers for a host that drives the exchange without a HIP toolchain of its own (the
 * C++ layer iresearch_amd/cpp/irs_hip.hpp): plain hipMalloc / hipMemcpy / hipStreamSynchronize. */
int irs_hip_device_alloc(int32_t device, uint64_t bytes, void** d_out);
void irs_hip_device_free(int32_t device, void* d_ptr);
int irs_hip_device_upload(int32_t device, void* d_dst, const void* h_src, uint64_t bytes);
int irs_hip_device_download(int32_t device, void* h_dst, const void* d_src, uint64_t bytes);
int irs_hip_device_sync(int32_t device, void* stream);
/* The library recycles the device and page-locked memory of destroyed batches (hipMalloc /
 * hipFree / hipHostMalloc cost more than a batch's kernels, and hipFree synchronises the device):
 * up to 64 GB of device memory and 4 GB of page-locked host memory per device stay with the
 * library (IRS_HIP_POOL_MB / IRS_HIP_PINNED_POOL_MB override); a closed segment's memory is freed
 * at once.  This hands all of it back to the runtime — postings_reader::CountMappedMemory's
 * counterpart for callers that watch their memory (formats.hpp:190). */
int irs_hip_device_trim(int32_t device);

/* Decoded posting streams kept across batches.  The joined path (IRS_HIP_PATH_JOINED, k_join)
 * decodes every distinct (segment, term) of a batch into 4-byte entries; those are a function of
 * the segment alone — no scorer, no query —, so the device keeps them, and a later batch that
 * references a stream it already holds decodes nothing for it.  A batch pins the streams it
 * references until irs_hip_batch_destroy; unpinned ones are evicted least recently used first when
 * the byte budget is reached, what does not fit is decoded into the batch's own memory as before:
 * the cache never makes a batch fail and never changes a result.  irs_hip_segment_close drops the
 * segment's streams, irs_hip_device_trim every unpinned one.
 * The budget: an eighth of the device's memory, IRS_HIP_STREAM_CACHE_MB (process-wide, read once)
 * or this call; 0 switches the cache off (what is held and unpinned is dropped).  The memory comes
 * from and goes back to the library's pool. */
int irs_hip_device_set_stream_cache(int32_t device, uint64_t bytes);
typedef struct irs_hip_stream_cache_stats {
  uint64_t bytes_held; /* device memory of the streams in the cache                       */
  uint64_t budget;     /* bytes_held stays at or below it                                 */
  uint64_t streams;    /* (segment, term) streams it can serve                            */
  uint64_t hits;       /* look-ups of batches (one per distinct stream of a deal) served  */
  uint64_t misses;     /* ... not served: decoded by the batch                            */
  uint64_t evictions;  /* streams dropped for room                                        */
} irs_hip_stream_cache_stats;
int irs_hip_device_stream_cache_stats(int32_t device, irs_hip_stream_cache_stats* out);
/* The distinct (segment, term) streams the batch's joined units reference, and how many of them its
 * last run (or the irs_hip_batch_plan it used) decoded itself: all of them with the cache off,
 * none when every stream was held, none for a replayed run of a batch whose first run filled the
 * cache.  A batch without joined units reports 0, 0.  IRS_HIP_EINVAL before the first run. */
int irs_hip_batch_stream_counts(irs_hip_batch* batch, uint32_t* distinct, uint32_t* decoded);
/* The batch's IRS_HIP_OP_MULTITERM units ((segment, query) pairs), whatever they hold in their
 * segment. */
int irs_hip_batch_wide_units(irs_hip_batch* batch, uint32_t* units);
/* ... and its units with IRS_HIP_CLAUSE_AND entries (k_clause_pilot / k_clause_score). */
int irs_hip_batch_clause_units(irs_hip_batch* batch, uint32_t* units);
/* ... and its units of tree queries (IRS_HIP_TREE_NODE entries: k_tree_pilot / k_tree_score). */
int irs_hip_batch_tree_units(irs_hip_batch* batch, uint32_t* units);
/* ... and its units with an IRS_HIP_PHRASE_NEXT entry (several phrases in one And; k_phrases_and). */
int irs_hip_batch_phrase_conj_units(irs_hip_batch* batch, uint32_t* units);
/* ... and its units with an IRS_HIP_PHRASE_OR entry (several phrases in one Or; k_phrases_or). */
int irs_hip_batch_phrase_disj_units(irs_hip_batch* batch, uint32_t* units);
/* Bound images: where a batch's plain disjunctions run on paired doc tiles, the kernel reads, per
 * (segment, term, scorer signature), a second array in posting order whose entries carry a 16-bit
 * upper bound of the posting's score factor instead of (tf, norm).  Images are made from the
 * decoded streams, cached with them under the same budget (bytes_held counts both; streams, hits,
 * misses and evictions keep counting decoded streams only) and dropped with them.
 * irs_hip_batch_image_counts: the distinct images the batch reads and how many its last run (or
 * the plan it used) made itself; 0, 0 for a batch that does not pair.  irs_hip_device_image_count:
 * the images the cache can serve.
 * irs_hip_join_bound_rule: THE rule, for tests — u[tf * 256 + norm] for tf, norm in 0 .. 255 under
 * the signature (kind: the library's scorer kind; tf_bound: the term's largest frequency), the
 * scale U with T U <= u <= T U + slack for the factor T the exact kernels multiply by the term's
 * weight, and the docs per paired tile.  IRS_HIP_EUNSUPPORTED: no image for this signature (a
 * reciprocal-form scorer whose factor never reaches 1/8, a table value that is negative or not
 * finite).  A diagnostic entry: what both test tiers reach the rule through.
 * irs_hip_batch_rescore_paths: how the units of the last run's paired launch turned their staged
 * docs into candidates — paths[0] units looked up only the docs within the window of the k-th
 * 16-bit sum, paths[1] every staged doc because the window held more docs than are looked up at
 * once (many ties), paths[2] every staged doc because no more than k were staged.  Zeros for a run
 * that did not pair.
 * irs_hip_join_half_rule: the integer weight k = ceil(cs 2^-15 / scale 2^16) (at least 1) the paired
 * kernel multiplies an image entry's u by, for a term weight cs (the exact kernels' fixed-point
 * weight) and an image's scale U.  irs_hip_join_half_probe: the kernel's own per-posting helper,
 * run by one workgroup over n entries (u: the low 16 bits) under k — out[i] = ((u k) >> 16) + 2 in
 * the low 16 bits (high_half = 0) or the high 16 bits of the word.  Diagnostic entries. */
int irs_hip_join_half_rule(float cs, float scale, uint32_t* k);
int irs_hip_join_half_probe(int32_t device, const uint32_t* entries, uint32_t n, uint32_t k,
                            uint32_t high_half, uint32_t* out);
int irs_hip_batch_image_counts(irs_hip_batch* batch, uint32_t* distinct, uint32_t* built);
int irs_hip_batch_rescore_paths(irs_hip_batch* batch, uint32_t paths[3]);
int irs_hip_device_image_count(int32_t device, uint64_t* images);
int irs_hip_join_bound_rule(int32_t kind, float norm_const, float norm_length, uint32_t tf_bound,
                            uint16_t* u, float* scale, float* slack, uint32_t* tile_docs);

typedef struct irs_hip_comm irs_hip_comm;
#define IRS_HIP_COMM_ID_BYTES 128u
int irs_hip_comm_unique_id(uint8_t id[IRS_HIP_COMM_ID_BYTES]);
int irs_hip_comm_init_rank(int32_t device, const uint8_t id[IRS_HIP_COMM_ID_BYTES], int32_t n_ranks,
                           int32_t rank, irs_hip_comm** out);
void irs_hip_comm_destroy(irs_hip_comm* comm);
/* Which RCCL the collective runs on (diagnostics): the library's path, prefixed "mapped:" when
 * the process had it loaded already — a host that also uses torch.distributed has torch's
 * bundled librccl.so mapped, and the communicator then binds THAT copy instead of loading a
 * second RCCL next to it.  EHIP when no RCCL could be bound. */
int irs_hip_comm_library(char* buf, size_t cap);
/* d_send: bytes_per_rank bytes on the device; d_recv: n_ranks * bytes_per_rank, rank r's block
 * at r * bytes_per_rank.  Asynchronous on `stream` (a hipStream_t). */
int irs_hip_topk_allgather(irs_hip_comm* comm, const void* d_send, void* d_recv,
                           uint64_t bytes_per_rank, void* stream);

/* ONE threshold per query across RANKS — the harness keeps one heap over all segments of the
 * index (utils/index-search.cpp:719-779); with the segments sharded over processes that is one
 * threshold for a query's units on every rank.  With a communicator attached, every run of the
 * batch sums the pilot histograms of each query over the ranks (one all-reduce of
 * n_queries * 514 counters between the pilot and the scoring kernels) and picks the threshold
 * from the sum, so that all segments of the index TOGETHER yield the k best docs (plus the usual
 * margin); a second, small all-reduce behind the selection sums what each group listed and
 * matched, so that every rank reaches the same verdict on the estimate and re-runs (or not) in
 * step with the others.  The merged top k over all ranks' lists is exactly what it is without
 * the option; a rank's list holds its docs at or above the shared threshold, possibly fewer
 * than k.  Requirements: the SAME queries in the same order on every rank (statistics are
 * index-global anyway), every rank runs its batches in the same order, and nothing else uses
 * `comm` concurrently — give the top-k exchange its own communicator when it overlaps the next
 * batch.  Applies to units on joined posting streams scored by the BM25 family (their score
 * bound is the same on every segment); other units keep thresholds of their own while the rank
 * still takes part in the collectives.  Implies irs_hip_batch_set_shared_threshold for the
 * rank's own segments.  NULL detaches.  Call before the batch's first run; `comm` must outlive
 * the batch. */
int irs_hip_batch_set_comm(irs_hip_batch* batch, irs_hip_comm* comm);

const char* irs_hip_strerror(int status);
uint32_t irs_hip_abi_version(void);
/* Name of the device the library would use, e.g. "gfx950"; EHIP when none. */
int irs_hip_device_arch(int32_t device, char* buf, size_t cap);

#ifdef __cplusplus
}
#endif
#endif /* IRS_HIP_H */
