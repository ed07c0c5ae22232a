/*
 * mygram_gpu.h — C ABI of libmygram_gpu.so: MygramDB's in-memory query hot path on AMD MI355X (gfx950).
 *
 * This is the ONLY boundary HIP code is reached through. There is no FFI around this path in the reference; the
 * seam it replaces is the set of public C++ methods below (paths relative to the reference tree). The C++17 shim in
 * mygram-db_amd/csrc/shim/ re-exposes them with the reference's exact signatures on top of this ABI.
 *
 *   Index::SearchAnd            src/index/index.h:127-128  (impl src/index/index.cpp:199-368)   -> mgx_and / mgx_batch_*
 *   Index::FilterByNgrams       src/index/index.h:138-139  (impl index.cpp:370-416)             -> mgx_retain
 *   Index::SearchOr             src/index/index.h:147      (impl index.cpp:418-448)             -> mgx_or
 *   Index::SearchNot            src/index/index.h:156-157  (impl index.cpp:450-486)             -> mgx_not
 *   Index::SearchByThreshold    src/index/index.h:172      (impl index.cpp:488-578)             -> mgx_threshold
 *   Index::EstimatePostingSize  src/index/index.h:286      (impl index.cpp:756-759)             -> mgx_posting_size
 *   BM25Scorer::ScoreDocuments  src/index/bm25_scorer.h:79-82 (impl bm25_scorer.cpp:47-99)      -> mgx_score_documents
 *   ResultSorter::SortByScore   src/query/result_sorter.h:75-76 (impl result_sorter.cpp:661-716)-> mgx_sort_by_score
 *   search_pipeline::Execute    src/server/search_pipeline.h:121-124 (impl search_pipeline.cpp:795-869),
 *     + BM25 glue src/server/handlers/search_handler.cpp:405-470                                -> mgx_batch_* (batched; new)
 *
 * House style follows the reference's own C API (src/client/mygramclient_c.h:5-16,49-60,186-223): every function
 * returns 0 on success and a non-zero mygram::utils::ErrorCode value (src/utils/error.h:35+) on failure;
 * mgx_last_error() returns a thread-local message; handles are opaque; descriptor structs carry
 * struct_size/version; library-allocated outputs are released with the matching free; on failure pointer
 * out-parameters are NULL and numeric ones zero; no C++ exception crosses this ABI.
 *
 * There is NO CPU fallback behind these entry points: if no gfx950 device is usable they fail with
 * MGX_ERR_INTERNAL and a message. Document ids are uint32 (src/types/doc_id.h:31); result lists are ascending and
 * unique unless stated otherwise.
 */
#ifndef MYGRAM_GPU_H_
#define MYGRAM_GPU_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MGX_ABI_VERSION 5U

/* Values of mygram::utils::ErrorCode used on this path (src/utils/error.h:37-48,100). */
#define MGX_OK 0
#define MGX_ERR_INVALID_ARGUMENT 2
#define MGX_ERR_OUT_OF_RANGE 3
#define MGX_ERR_NOT_IMPLEMENTED 4
#define MGX_ERR_INTERNAL 5
#define MGX_ERR_INDEX_NOT_FOUND 4000

int mgx_abi_version(void);
/* Thread-local message of the last failing call on this thread; valid until that thread's next failing call. */
const char* mgx_last_error(void);
/* Releases any buffer this library returned through an out-pointer (docid/score arrays). NULL is allowed. */
void mgx_free(void* p);
/* Number of usable gfx950 devices (0 when there is none; never fails). */
int mgx_device_count(void);

/* =====================================================================================================
 * Host-side column builder: normalized texts -> the column arrays the device index is made of.
 * Restates what Index::AddDocument (index.cpp:39-74) + BM25 ingest bookkeeping
 * (src/mysql/binlog_event_processor.cpp:98-99) produce, plus the build-owned tf column that makes
 * BM25Scorer::CountTermOccurrences (bm25_scorer.cpp:27-45) a lookup for terms that are exactly one n-gram long.
 * Pure host code (multi-threaded); no device needed.
 * ===================================================================================================== */

typedef struct mgx_columns mgx_columns;

typedef struct mgx_build_params {
  uint32_t struct_size; /* sizeof(mgx_build_params) */
  uint32_t version;     /* MGX_ABI_VERSION */
  int32_t ngram_size;           /* Index(ngram_size, ...) */
  int32_t kanji_ngram_size;     /* <=0 => ngram_size (index.cpp:31) */
  int32_t cross_boundary_ngrams;
  int32_t n_threads;            /* 0 => hardware concurrency */
} mgx_build_params;

typedef struct mgx_columns_view {
  uint64_t n_grams;
  const uint8_t* key_bytes;  /* gram keys, concatenated, sorted bytewise ascending; gram id = rank */
  const uint32_t* key_off;   /* n_grams+1 */
  const uint64_t* offsets;   /* n_grams+1, CSR into docids/tf */
  const uint32_t* docids;    /* ascending per gram */
  const uint8_t* tf;         /* non-overlapping occurrence count of the gram's bytes in the doc text; 255 = "255 or more,
                              * see tf_overflow" */
  uint64_t n_postings;
  uint32_t first_doc_id;     /* doc d has local slot d - first_doc_id */
  uint64_t n_docs;           /* slots */
  const uint32_t* doc_len;   /* n_docs: CountCodePoints(text) (string_utils.cpp:655-669); 0 for empty text */
  uint64_t bm25_doc_count;   /* docs with non-empty text (server_types.h:157-193) */
  uint64_t bm25_total_len;   /* sum of their doc_len */
  /* postings whose count does not fit the byte column: their index into docids/tf (ascending) and the true count, so
   * that BM25 sees exactly what CountTermOccurrences (bm25_scorer.cpp:27-45) returns for any document */
  const uint64_t* tf_overflow_pos;
  const uint32_t* tf_overflow_val;
  uint64_t n_tf_overflow;
} mgx_columns_view;

/* Docs are first_doc_id, first_doc_id+1, ...; doc i's normalized text is text_bytes[text_off[i] .. text_off[i+1]). */
int mgx_columns_build(const mgx_build_params* params, const uint8_t* text_bytes, const uint64_t* text_off,
                      uint32_t first_doc_id, uint64_t n_docs, mgx_columns** out);
/* The same columns, built on HIP device `device`: every array and scalar of the result's view equals what
 * mgx_columns_build returns for the same inputs, padding included, and every call that takes an mgx_columns takes it.
 * params->n_threads is ignored. Nothing is read past text_bytes[text_off[n_docs]]. Safe to call from many threads.
 * Refusals, in this order: NULL arguments, bad struct_size / version: MGX_ERR_INVALID_ARGUMENT; doc ids past uint32:
 * MGX_ERR_OUT_OF_RANGE; ngram_size > 3 or an effective kanji_ngram_size > 3 (a gram is packed into 64 bits on the
 * device): MGX_ERR_NOT_IMPLEMENTED; text_off that descends: MGX_ERR_INVALID_ARGUMENT; no HIP device: MGX_ERR_INTERNAL
 * (there is no CPU fallback behind this call); 4 GiB of text or more, or temporary storage beyond the device's free
 * memory (the message states both numbers; nothing stays allocated): MGX_ERR_OUT_OF_RANGE. After NOT_IMPLEMENTED or
 * OUT_OF_RANGE, mgx_columns_build builds the same columns on the host. */
int mgx_columns_build_device(const mgx_build_params* params, const uint8_t* text_bytes, const uint64_t* text_off,
                             uint32_t first_doc_id, uint64_t n_docs, int device, mgx_columns** out);
/* The reference's index dump ("MGIX" v1..v4: Index::SaveToStream / LoadFromData, src/index/index_serialization.cpp:113-194,
 * :260-420; posting lists as fixed-width deltas or Roaring portable bytes, src/index/posting_list.cpp:973-1073) ->
 * columns. The CRC32 trailer (v2+) is verified. A dump holds doc ids only: the view's tf / doc_len are NULL (an index
 * created from it answers everything but SORT _score). n_docs == 0: the doc range is the span of the ids found. */
typedef struct mgx_mgix_info {
  uint32_t version;
  int32_t ngram_size, kanji_ngram_size, cross_boundary_ngrams;
  int32_t normalize_nfkc, normalize_lower;
  char normalize_width[16];
  uint64_t n_terms;
} mgx_mgix_info;
int mgx_columns_from_mgix(const uint8_t* data, uint64_t len, uint32_t first_doc_id, uint64_t n_docs, mgx_columns** out,
                          mgx_mgix_info* info /* may be NULL */);
/* The reference's table dump ("MGDB" version 2: what DUMP SAVE writes, src/storage/dump_format_v2.cpp:520-770) -> one
 * table's columns, normalized texts and filter values: the MGIX index stream (as mgx_columns_from_mgix) AND the document
 * store stream ("MGDS", src/storage/document_store_persistence.cpp:59-175). File and section CRC32s are verified. When the
 * store kept the normalized texts (memory.verify_text on: what BM25 needs in the reference too) the columns are built from
 * them — tf and doc lengths included, so the loaded index ranks — and must agree with the dump's own index gram by gram and
 * list by list; otherwise the columns hold the index's doc ids alone. `table`: NULL or "" = the first table of the dump. */
typedef struct mgx_dump mgx_dump;
typedef struct mgx_dump_view {
  const char* table_name;
  mgx_mgix_info index_info;
  uint32_t first_doc_id; /* the range spans every doc id the store or the index mentions */
  uint64_t n_docs;
  uint64_t n_existing;   /* documents in the store (DocumentStore::Size) */
  const uint8_t* exists; /* n_docs: 1 = the store holds this id (DocumentStore::GetAllDocIds, the NOT universe) */
  const uint8_t* text_bytes; /* normalized texts by slot (mgx_index_attach_text takes them as they are) */
  const uint64_t* text_off;  /* n_docs + 1 */
  uint32_t n_filter_columns;
  int32_t has_texts;
} mgx_dump_view;
typedef struct mgx_dump_filter_column {
  const char* name;
  uint32_t value_type;   /* the storage::FilterValue alternative (src/storage/document_store.h:73-87): 1 bool .. 12 double */
  const uint64_t* values;     /* n_docs, widened as mgx_filter_column_desc wants them (strings: unused) */
  const uint8_t* is_null;     /* n_docs */
  const uint8_t* string_bytes; /* value_type 11: doc i's string is string_bytes[string_off[i] .. string_off[i+1]) */
  const uint64_t* string_off;
} mgx_dump_filter_column;
int mgx_dump_open(const uint8_t* data, uint64_t len, const char* table, mgx_dump** out);
int mgx_dump_view_get(const mgx_dump* dump, mgx_dump_view* out);
int mgx_dump_filter_column_get(const mgx_dump* dump, uint32_t i, mgx_dump_filter_column* out);
/* The documents' primary keys by doc slot of the dump's range (mgx_dump_view.first_doc_id, n_docs): key i is
 * bytes[off[i] .. off[i + 1]); a slot mgx_dump_view.exists marks 0 holds no document and no bytes. The arrays are the
 * dump's: they live until mgx_dump_destroy. What mgx_index_set_primary_keys takes, with `exists` as has_key. */
int mgx_dump_primary_keys_get(const mgx_dump* dump, const uint8_t** bytes, const uint64_t** off);
/* The documents' original texts, likewise by doc slot (the store section's "MGDS" v3 writes one per document,
 * src/storage/document_store_persistence.cpp:159-167; length 0: the store holds none for that document, as in a v2
 * stream). What HIGHLIGHT answers with where there is one (mgx_index_attach_original_text, after the caller built the
 * documents' maps). */
int mgx_dump_original_texts_get(const mgx_dump* dump, const uint8_t** bytes, const uint64_t** off);
/* Hands the table's columns to the caller (release with mgx_columns_destroy); a second call returns NULL. */
int mgx_dump_take_columns(mgx_dump* dump, mgx_columns** out);
void mgx_dump_destroy(mgx_dump* dump);
int mgx_columns_view_get(const mgx_columns* cols, mgx_columns_view* out);
/* Gram dictionary lookup (host-side replacement of Index::TakePostingSnapshot's map lookup, index.cpp:728-747).
 * *found = 0 and *gram_id = 0 for an unknown gram. */
int mgx_columns_lookup(const mgx_columns* cols, const uint8_t* gram, size_t len, uint32_t* gram_id, int* found);
void mgx_columns_destroy(mgx_columns* cols);

/* =====================================================================================================
 * Device index
 * ===================================================================================================== */

typedef struct mgx_index mgx_index;

typedef struct mgx_index_desc {
  uint32_t struct_size; /* sizeof(mgx_index_desc) */
  uint32_t version;     /* MGX_ABI_VERSION */
  int32_t device;       /* HIP device ordinal */
  uint32_t tile_shift;  /* log2 docids per tile; 0 => default (14) */
  /* the doc-id range this index (or shard) owns: local slot = doc_id - first_doc_id, 0 <= slot < n_docs */
  uint32_t first_doc_id;
  uint64_t n_docs;
  uint64_t n_grams;
  const uint64_t* offsets; /* host, n_grams+1 */
  const uint32_t* docids;  /* host, offsets[n_grams]; every id inside the owned range, ascending per gram */
  const uint8_t* tf;       /* host, parallel to docids; NULL => BM25 scoring unavailable */
  const uint32_t* doc_len; /* host, n_docs; NULL => BM25 scoring unavailable */
  /* posting lists at least this dense (|L| / n_docs) are ALSO kept as precomputed bitmaps in HBM and read in that
   * form by the set-algebra kernels (what Roaring bitset containers are to the reference, posting_list.cpp:800-834).
   * 0 => default (1/256: at most 8x the bytes of the u32 list, bought for latency: bitmap operands need no scatter
   * and BM25 runs on the wave-autonomous kernel); >= 2 => disabled. */
  double dense_threshold;
  /* side table of the tf bytes that read 255 (mgx_columns_view.tf_overflow_*): posting indices ascending; may be
   * NULL / 0 (then 255 is taken literally) */
  const uint64_t* tf_overflow_pos;
  const uint32_t* tf_overflow_val;
  uint64_t n_tf_overflow;
} mgx_index_desc;

/* Host arrays are copied; the caller keeps ownership. */
int mgx_index_create(const mgx_index_desc* desc, mgx_index** out);
/* A serving index from normalized texts in one call, the postings never on the host: the device builder's docids / tf
 * columns, doc lengths and (attach_text) the texts stay in device memory after the texts' single upload and become the
 * index's own arrays. *index_out is indistinguishable from what mgx_index_create makes of mgx_columns_build's columns of
 * the same texts (with mgx_index_attach_text(the same buffers) applied when attach_text is set): every device array holds
 * the same bytes, mgx_index_memory_bytes is equal. *dictionary_out holds what a host caller reads: the keys
 * (mgx_columns_lookup works), offsets, n_postings, first_doc_id, n_docs, doc_len, the BM25 statistics and the tf overflow
 * lists, each equal to the host builder's; its view has docids == NULL and tf == NULL, so mgx_index_create over it answers
 * MGX_ERR_INVALID_ARGUMENT. Release both as usual (mgx_columns_destroy, mgx_index_destroy).
 * Refusals, answered on the host before any device work, in this order: those of mgx_columns_build_device up to the
 * descending text_off (a bad struct_size / version of either struct: MGX_ERR_INVALID_ARGUMENT); a tile_shift
 * mgx_index_create refuses: MGX_ERR_NOT_IMPLEMENTED; n_docs == 0: MGX_ERR_OUT_OF_RANGE; no HIP device: MGX_ERR_INTERNAL;
 * a bad device: MGX_ERR_INVALID_ARGUMENT; 4 GiB of text or more, or no room on the device for the temporary storage and
 * the index's arrays: MGX_ERR_OUT_OF_RANGE. On any failure both outputs are NULL and nothing stays allocated. After
 * NOT_IMPLEMENTED for the gram size or OUT_OF_RANGE for the text or the memory, mgx_columns_build + mgx_index_create build
 * the same index through the host. Safe to call from many threads. */
typedef struct mgx_index_build_desc {
  uint32_t struct_size; /* sizeof(mgx_index_build_desc) */
  uint32_t version;     /* MGX_ABI_VERSION */
  int32_t device;       /* as mgx_index_desc */
  uint32_t tile_shift;  /* as mgx_index_desc */
  double dense_threshold; /* as mgx_index_desc */
  uint32_t attach_text; /* 1: the index keeps the normalized texts, exactly as after mgx_index_attach_text(same buffers) */
  uint32_t reserved;    /* 0 */
} mgx_index_build_desc;
int mgx_index_build_device(const mgx_build_params* params, const mgx_index_build_desc* desc, const uint8_t* text_bytes,
                           const uint64_t* text_off, uint32_t first_doc_id, uint64_t n_docs, mgx_columns** dictionary_out,
                           mgx_index** index_out);
/* One gram's posting list as the index holds it in device memory: its doc ids and tf bytes (either buffer may be NULL;
 * both NULL: only *n). An index made without tf fills doc ids only. An unknown gram: MGX_ERR_OUT_OF_RANGE; capacity (in
 * postings) below the list's length: MGX_ERR_OUT_OF_RANGE with *n set to the length. */
int mgx_index_read_postings(mgx_index* idx, uint32_t gram_id, uint32_t* docids, uint8_t* tf, uint64_t capacity, uint64_t* n);
void mgx_index_destroy(mgx_index* idx);
int mgx_posting_size(const mgx_index* idx, uint32_t gram_id, uint64_t* out);
/* Device bytes held by the index (postings, tf, doc_len, skip tables, dense bitmaps). */
int mgx_index_memory_bytes(const mgx_index* idx, uint64_t* out);
/* Registers one FilterIndex (column,value) doc set (src/storage/filter_index.h:39-124) as a device bitmap usable
 * as a filter operand; docids ascending, inside the owned range. */
int mgx_index_add_filter_bitmap(mgx_index* idx, const uint32_t* docids, uint64_t n, uint32_t* out_bitmap_id);
/* Typed filter columns (DocumentStore filter values, src/storage/document_store.h:73-87): what FILTER conditions other
 * than a caller-resolved bitmap, and FACET, are evaluated on. Values by local doc slot, widened to 8 bytes:
 * MGX_FC_SIGNED (bool, int8..int64, TimeValue seconds) as int64, MGX_FC_UNSIGNED (uint8..uint64; strings as their rank in
 * the caller's bytewise-sorted dictionary) as uint64, MGX_FC_DOUBLE as IEEE bits. is_null (may be NULL: none) marks NULLs.
 * value_ids (may be NULL: FACET unavailable on this column): the dense id < n_values of every doc's value, 0xFFFFFFFF
 * for NULL — FilterIndex keeps one bitmap per distinct value (filter_index.h:39-124); the ids are their device form. */
#define MGX_FC_SIGNED 0u
#define MGX_FC_UNSIGNED 1u
#define MGX_FC_DOUBLE 2u
typedef struct mgx_filter_column_desc {
  uint32_t struct_size; /* sizeof(mgx_filter_column_desc) */
  uint32_t version;     /* MGX_ABI_VERSION */
  uint32_t value_class; /* MGX_FC_* */
  uint32_t n_values;    /* distinct non-NULL values (value_ids) */
  const void* values;   /* n_docs x 8 bytes */
  const uint8_t* is_null;
  const uint32_t* value_ids;
} mgx_filter_column_desc;
int mgx_index_add_filter_column(mgx_index* idx, const mgx_filter_column_desc* desc, uint32_t* out_column_id);
/* One FilterCondition (src/query/query_parser.h:123-127) on a typed column -> a filter bitmap usable like the ones of
 * mgx_index_add_filter_bitmap: the docs whose stored value compares true against the literal (given in the column's
 * class: literal_bits = the int64 / uint64 / double bit pattern). op: MGX_CMP_*. eq_epsilon > 0: = and != on doubles
 * test |stored - literal| against it (CompareDoubleValues, src/utils/comparison_utils.h:56-70: the per-document path of
 * ApplyFilters, search_pipeline.cpp:1098-1194); 0: exact (the FilterIndex bitmap path compares serialized keys,
 * :1021-1094). null_matches: NULL docs are members (the per-document path lets NULL pass != only, :1151-1157).
 * never_matches: the literal has no interpretation in the column's type — no non-NULL doc matches (:1167,1172,1177,1182). */
#define MGX_CMP_EQ 0u
#define MGX_CMP_NE 1u
#define MGX_CMP_LT 2u
#define MGX_CMP_LE 3u
#define MGX_CMP_GT 4u
#define MGX_CMP_GE 5u
int mgx_index_filter_compare(mgx_index* idx, uint32_t column_id, uint32_t op, uint64_t literal_bits, double eq_epsilon,
                             int null_matches, int never_matches, uint32_t* out_bitmap_id);
/* How batches that are in flight at the same time (one stream per batch object) share the device.
 * MGX_ORDER_FIFO (default): the main kernels of a batch start when those of the batch enqueued before it on this index
 * have finished — first in, first out, so a batch's latency is its own kernel time plus what was queued ahead of it;
 * uploads, clears, merges and result copies still overlap the previous batch. MGX_ORDER_CONCURRENT: no ordering — the
 * device time-slices all batches in flight (a few percent more throughput at four batches in flight, every batch
 * finishing after roughly depth x kernel time). */
#define MGX_ORDER_FIFO 0u
#define MGX_ORDER_CONCURRENT 1u
int mgx_index_set_batch_order(mgx_index* idx, uint32_t order);
/* Keeps the NORMALIZED text of the shard's docs resident in HBM (what DocumentStore::VisitNormalizedTextsFor hands
 * to BM25Scorer::ScoreDocuments, document_store_retrieval.cpp:289-322), by local slot: doc first_doc_id + i is
 * text_bytes[text_off[i] .. text_off[i+1]). Needed by text-level scored terms (mgx_term.text). Host arrays are copied. */
int mgx_index_attach_text(mgx_index* idx, const uint8_t* text_bytes, const uint64_t* text_off);

/* =====================================================================================================
 * Batched search (new: the reference executes one query per request, request_dispatcher.cpp:93-193)
 * ===================================================================================================== */

#define MGX_SORT_DOCID 0u /* no SORT _score: docid order; `reverse` selects descending (SearchAnd limit/reverse) */
#define MGX_SORT_SCORE 1u /* SORT _score: BM25 + ResultSorter::SortByScore */
/* SORT <filter column> ASC|DESC (ResultSorter::SortAndPaginate, result_sorter.cpp:489-650): the result set ordered by
 * the column mgx_query.sort_column (an id from mgx_index_add_filter_column) before offset / limit. `reverse` = 1: DESC.
 * The order is that of the reference's string keys (FilterValueToSortKey, :187-217) restated in 64 bits: signed values
 * (bool, int8..int64, TimeValue) by value; doubles by their bits in IEEE total order (-0.0 before +0.0, NaNs by their
 * bits); unsigned values v as v + 2^63 up to INT64_MAX and as v above it (the reference's own rule, :205-212, kept);
 * NULL first in ASC and last in DESC; ties by doc id in the sort's own direction (:43-54). Any limit (0 = all) and any
 * offset; scores come back 0.0; totals and funnel counters as without SORT.
 * MGX_SORT_COLUMN_RANK: the same on an MGX_FC_UNSIGNED column that holds ranks in the caller's bytewise-sorted string
 * dictionary: the key is rank + sort_key_bias, bias 0 when the dictionary holds the empty string (which then ties with
 * NULL as in the reference, both keys being ""), otherwise 1. The ranks of two dictionaries do not compare: a table with
 * a delta index sorts by such a column only after it is compacted.
 * Refused: an unknown column MGX_ERR_OUT_OF_RANGE; sort_key_bias above 1, or non-zero with MGX_SORT_COLUMN,
 * MGX_ERR_INVALID_ARGUMENT; MGX_SORT_COLUMN_RANK on a column of another class MGX_ERR_INVALID_ARGUMENT. With
 * MGX_ERR_NOT_IMPLEMENTED and a message: a column that holds NULLs beside a value whose key is also 0 (INT64_MIN; the
 * double whose bits are all ones), which 64 bits cannot tell apart (mgx_index_add_filter_column marks it; without NULLs
 * such a column sorts exactly; mgx_batch_merge_local refuses the same way when the main index's and the delta's column
 * hold the two between them); the sharded entry points (mgx_batch_export_topk / _export_buffer, _merge_shards,
 * _exchange, _execute_gather, _execute_sharded); a highlighted batch that holds such a query. */
#define MGX_SORT_COLUMN 2u
#define MGX_SORT_COLUMN_RANK 3u
/* SORT by primary key: the reference's order for every query without a SORT clause (primary key DESC,
 * result_sorter.cpp:502-510), for SORT id and for SORT <primary key column> (:239-262). `reverse` = 1: DESC. The sort
 * key of a document is its primary key as mgx_index_set_primary_keys took it: a non-empty string of ASCII digits that
 * fits a uint64_t counts as that number zero-padded to 20 characters, any other key as its bytes, a document without a
 * key as its doc id zero-padded to 20 characters; keys compare as std::string::compare (unsigned bytes, a proper prefix
 * first), ties go to the doc id in the sort's own direction. On an index without keys the page is therefore the docid
 * page in that direction. Any limit (0 = all) and any offset; scores come back 0.0; totals and funnel counters as
 * without SORT. sort_column and sort_key_bias must be 0 (MGX_ERR_INVALID_ARGUMENT). mgx_batch_merge_local merges the
 * runs of a main index and its delta by the key strings (by the numbers when both indexes hold numeric keys only).
 * Where the keys of an index never decrease with the doc slot, a query with offset 0 runs as the docid page it equals
 * (see mgx_index_set_primary_key_shortcut; the environment variable MGX_PK_SORT_GENERAL=1 turns that off).
 * Refused with MGX_ERR_NOT_IMPLEMENTED and a message, like MGX_SORT_COLUMN: the sharded entry points; a highlighted
 * batch that holds such a query. */
#define MGX_SORT_PRIMARY_KEY 4u

#define MGX_MAX_TERMS 64u /* query_parser.h:270-272 */
/* Gram id of an n-gram the TABLE knows but this doc-range shard holds no posting for: an empty doc set. (A gram the
 * whole table lacks never reaches the device, see mgx_term.) Keeps the batch layout identical on every shard. */
#define MGX_GRAM_ABSENT 0xFFFFFFFFu

/* One search term = the AND of its (deduplicated) n-grams, as search_pipeline::GenerateTermInfos leaves it
 * (search_pipeline.cpp:569-603). Unknown grams must be resolved by the caller: a positive term with an unknown
 * gram makes the whole query empty before it reaches the device (Execute :804-810), a NOT term with one is dropped. */
typedef struct mgx_term {
  const uint32_t* gram_ids;
  uint32_t n_grams;
  /* FUZZY terms (search_pipeline.cpp:1697-1702): docs in at least `threshold` of the distinct grams;
   * 0 => plain AND of all grams. */
  uint32_t threshold;
  double idf; /* BM25Scorer::ComputeIDF(N, df) for MGX_SORT_SCORE when the term is exactly one n-gram (text == NULL):
               * its tf is the gram's tf column, its df the posting count */
  /* Text-level scored term (a search term that spans several n-grams, or differs from its single gram): the
   * normalized term bytes. In a MGX_SORT_SCORE query tf is then BM25Scorer::CountTermOccurrences over the doc text
   * (bm25_scorer.cpp:27-45) and df is counted per execute as PopulateTermDocumentFrequency does
   * (search_pipeline.cpp:542-565: docs of the gram AND whose text contains the term); idf = ComputeIDF(total_docs,
   * df) is evaluated by the library and the `idf` field is ignored. Needs mgx_index_attach_text. NULL otherwise.
   * n_grams == 0 with a text: a term shorter than one n-gram — its doc set is every doc whose stored text contains it
   * (query::SearchNormalizedSubstring, src/query/substring_search.h:24-42, reached from SearchTermDocuments,
   * search_pipeline.cpp:438-446), found by a text scan on the device; as a scored term its df is 0, as the reference's
   * is (PopulateTermDocumentFrequency returns before counting, search_pipeline.cpp:546-549). */
  const uint8_t* text;
  uint32_t text_len;
} mgx_term;

typedef struct mgx_filter {
  uint32_t bitmap_id; /* from mgx_index_add_filter_bitmap */
  uint32_t negate;    /* 0: EQ (AND), 1: NE (ANDNOT) — search_pipeline.cpp:1196-1237 */
} mgx_filter;

/* One FilterCondition evaluated by the batch itself: the doc set mgx_index_filter_compare(column_id, op, literal_bits,
 * eq_epsilon, null_matches, never_matches) would register, bit for bit, but held in a row of an arena the BATCH OBJECT
 * owns — no row of the index's filter pool, no synchronisation at planning time. Every execute of the batch starts
 * with one launch (filter_compare_batch_kernel) that evaluates the batch's distinct conditions (two conditions are the
 * same when every field but `negate` is equal) against the resident typed columns; the arena is kept across
 * mgx_batch_reset and grows only when a batch holds more distinct conditions than any before it. A batch whose
 * distinct conditions would need more than MGX_CONDITION_ARENA_MAX_BYTES of rows (one row = the index's filter row:
 * n_docs bits rounded up to 16384-doc tiles, plus padding) is refused with MGX_ERR_OUT_OF_RANGE. */
#define MGX_CONDITION_ARENA_MAX_BYTES (1ull << 30)
typedef struct mgx_condition {
  uint32_t column_id;    /* from mgx_index_add_filter_column; unknown: MGX_ERR_OUT_OF_RANGE */
  uint32_t op;           /* MGX_CMP_*; unknown: MGX_ERR_INVALID_ARGUMENT */
  uint64_t literal_bits; /* as mgx_index_filter_compare */
  double eq_epsilon;
  uint32_t null_matches; /* as mgx_index_filter_compare */
  uint32_t never_matches;
  uint32_t negate;       /* as mgx_filter.negate: 1 = ANDNOT the set */
  uint32_t reserved;     /* 0 */
} mgx_condition;

/* Boolean expression over the positive terms (query::QueryNode, src/query/query_ast.h:52-83), in POSTFIX order.
 * Evaluated like EvaluateBooleanAstExpanded (src/server/search_pipeline.cpp:327-378): TERM = the term's doc set,
 * AND = intersection of its children, OR = union, NOT = universe minus child, where the universe is
 * DocumentStore::GetAllDocIds() (document_store_retrieval.cpp:242-258). */
#define MGX_EXPR_TERM 0u  /* arg = index into mgx_query.terms */
#define MGX_EXPR_EMPTY 1u /* a term the caller already knows to match nothing (unknown gram). Constant FALSE for the text
                           * filter of an expression too (exact_text / fuzzy_verify_distance with n_expr > 0): with that
                           * filter on, use it only for a term whose normalized text is empty, and send every other empty
                           * leaf as a TERM whose only gram is MGX_GRAM_ABSENT and which carries its `text` */
#define MGX_EXPR_AND 2u   /* arg = number of children (>= 1), already on the stack */
#define MGX_EXPR_OR 3u    /* arg = number of children (>= 1) */
#define MGX_EXPR_NOT 4u   /* one child */
typedef struct mgx_expr_token {
  uint32_t op, arg;
} mgx_expr_token;

typedef struct mgx_query {
  /* positive terms, ALREADY in the order search_pipeline.cpp:2012-2014 leaves them (estimated_size ascending):
   * BM25 sums term contributions in this order (bm25_scorer.cpp:77-86) */
  const mgx_term* terms;
  uint32_t n_terms;
  const mgx_term* not_terms; /* ApplyNotFilter, search_pipeline.cpp:871-932 */
  uint32_t n_not_terms;
  const mgx_filter* filters;
  uint32_t n_filters;
  uint32_t sort;    /* MGX_SORT_* */
  uint32_t limit;   /* 0 => all */
  uint32_t offset;  /* MGX_SORT_SCORE, MGX_SORT_COLUMN / _RANK and MGX_SORT_PRIMARY_KEY */
  uint32_t reverse; /* MGX_SORT_DOCID: descending docids; MGX_SORT_SCORE / _COLUMN / _PRIMARY_KEY: 1 => SortOrder::DESC */
  uint32_t sort_column; /* MGX_SORT_COLUMN / _RANK: the column's id. (It and sort_key_bias fill what was padding: no other
                         * field moves and the struct keeps its size, so MGX_ABI_VERSION stays; a zero-initialised
                         * struct means what it meant.) */
  double k1, b;     /* BM25Params (bm25_scorer.h:20-23) */
  uint64_t total_docs;    /* BM25Stats::doc_count; only documents the caller's idf values already encode */
  double avg_doc_length;  /* BM25Stats::avg_doc_length() */
  /* Optional boolean expression (ExecuteWithBooleanAst, search_pipeline.cpp:1408-1578). When n_expr > 0 the positive
   * part of the query is the expression instead of the plain AND of `terms`; NOT terms and filters still apply to its
   * result. The NOT universe is the doc-id range [universe_first, universe_first + universe_count) clipped to the
   * index (universe_count 0 => every slot of the index). */
  const mgx_expr_token* expr;
  uint32_t n_expr;
  uint32_t universe_first;
  uint64_t universe_count;
  /* Exact-text post-filter (PostFilterByText, search_pipeline.cpp:1239-1246): after NOT terms and filters, keep only
   * the docs whose text contains EVERY positive term. The caller sets it when the reference would: memory.verify_text
   * says so (ShouldApplyVerifyText :42-66), or a mixed-script term has a code point no query n-gram covers
   * (RequiresExactTextForHybridFragments :138-150). Every positive term must then carry its normalized `text`;
   * needs mgx_index_attach_text. after_filters still counts the docs before this filter, `total` those after it.
   * With n_expr > 0 the rule is the TREE's (PostFilterByBooleanText, :404-416): a candidate stays when `expr` evaluates to
   * true over its text, a TERM leaf being text.find(term), EMPTY false, AND / OR / NOT as written — the filter only
   * narrows the set-algebra result. Every term a TERM token names must carry its `text` (1..4096 bytes); setting
   * fuzzy_verify_distance as well is MGX_ERR_INVALID_ARGUMENT (one filter, d = 0 here). At most 64 operands may be
   * pending in the postfix at once (MGX_ERR_OUT_OF_RANGE). Runs like a fuzzy_verify_distance query. */
  uint32_t exact_text;
  uint32_t sort_key_bias; /* MGX_SORT_COLUMN_RANK: 0 or 1, see there */
  /* MGX_SORT_SCORE: which terms BM25 sums, as indices into `terms`, in summation order (bm25_scorer.cpp:77-86); a term
   * may be listed more than once (ScoreDocuments adds a repeated term's contribution each time). NULL => every positive
   * term in order (the plain conjunctive query). An expression query lists the TERM leaves that are not under a NOT, in
   * tree order (CollectAstScoringTerms, search_pipeline.cpp:232-254; search_handler.cpp:428-456 scores exactly those:
   * reference vector tests/server/search_pipeline_test.cpp:1350-1392); a FUZZY query its terms in the order given. A
   * listed term may match none of a result's text (an OR branch, a fuzzy neighbour): its tf is then 0 and it adds
   * nothing, as in the reference. */
  const uint32_t* score_terms;
  uint32_t n_score_terms;
  /* FUZZY verify_text post-filter (PostFilterByFuzzyText, search_pipeline.cpp:1746-1755), next to exact_text: 0 = off;
   * 1 or 2 = the query's FUZZY distance d. After NOT terms and filters (and before the exact_text filter), keep only the
   * docs whose text holds EVERY positive term exactly (text.find) or within d edits (ContainsFuzzyMatch,
   * src/utils/edit_distance.cpp:199-296: per whitespace-delimited word, U+3000 / U+00A0 count as spaces; code-point
   * windows inside non-ASCII words). The caller sets it when ExecuteWithFuzzy would (:1722-1731:
   * ShouldApplyVerifyText(memory.verify_text, terms)). Every positive term must carry its normalized `text`; needs
   * mgx_index_attach_text. after_filters still counts the docs before this filter, `total` those after it. The query
   * runs on the general kernel, in a launch of its own.
   * With n_expr > 0 the rule is the TREE's with FUZZY leaves (ExecuteWithBooleanAst, :1538-1555): as exact_text above,
   * a TERM leaf being "found exactly or within d edits". */
  uint32_t fuzzy_verify_distance;
  /* FILTER conditions the batch evaluates itself (mgx_condition), applied after `filters` in the same funnel step
   * (after_filters counts the docs that passed both). n_filters + n_conditions <= MGX_MAX_TERMS, else
   * MGX_ERR_OUT_OF_RANGE. NULL / 0: none — the batch then launches and allocates nothing for them. */
  const mgx_condition* conditions;
  uint32_t n_conditions;
} mgx_query;

typedef struct mgx_batch mgx_batch;

typedef struct mgx_query_result {
  uint64_t total;             /* results.size() before pagination (search_handler.cpp:471) */
  uint64_t total_candidates;  /* SearchPipelineResult funnel (search_pipeline.h:58-65) */
  uint64_t after_intersection;
  uint64_t after_not;
  uint64_t after_filters;
  uint32_t n_docs;            /* entries returned for this query */
  uint32_t docs_begin;        /* index of its first entry in mgx_result_view.docs / .scores */
} mgx_query_result;

typedef struct mgx_result_view {
  uint32_t n_queries;
  const mgx_query_result* queries;
  const uint32_t* docs;   /* concatenated per query, in rank order */
  const double* scores;   /* parallel to docs for MGX_SORT_SCORE queries (0.0 otherwise) */
} mgx_result_view;

/* Compiles and uploads a batch; the batch can be executed any number of times. */
int mgx_batch_prepare(mgx_index* idx, const mgx_query* queries, uint32_t n_queries, mgx_batch** out);
/* Re-compiles `batch` in place for a NEW set of queries (a serving loop: every step is a fresh batch). Equivalent to
 * mgx_batch_destroy + mgx_batch_prepare on the same index, but the object keeps its device arenas, pinned result
 * block and events, so the steady state allocates nothing. The last execute of the old contents must have completed
 * (mgx_batch_fetch returned, or its stream was synchronized). On failure the batch is empty but still usable. */
int mgx_batch_reset(mgx_batch* batch, const mgx_query* queries, uint32_t n_queries);
/* A non-blocking stream the batch object owns (created on first request, kept across mgx_batch_reset): batch objects
 * are independent pipeline slots, and a host layer without HIP headers passes this to execute / export / merge. */
int mgx_batch_stream(mgx_batch* batch, void** hip_stream);
/* Enqueues the whole batch on `hip_stream` (a hipStream_t; NULL = the default stream). Asynchronous; ends with the copy
 * of the result block to pinned host memory behind an event, so mgx_batch_fetch waits for THIS batch only. The batch's
 * input arrays (built in pinned host memory by prepare/reset) are shipped by the first execute, on this stream. */
int mgx_batch_execute(mgx_batch* batch, void* hip_stream);
/* Waits for the last execute and copies the (small) results to host memory owned by the batch. */
int mgx_batch_fetch(mgx_batch* batch, mgx_result_view* out);
/* ---- HIGHLIGHT (SEARCH ... HIGHLIGHT [TAG <open> <close>] [SNIPPET_LEN n] [MAX_FRAGMENTS n]: GenerateHighlightSnippets on
 * the page, src/server/handlers/search_handler.cpp:473-482; query::Highlighter::Generate, src/query/highlighter.cpp:114-309)
 * The snippet material of every page entry of the highlighted queries is produced ON THE DEVICE, by one more kernel on the
 * batch's stream behind the kernel that finalises the page (after mgx_batch_execute's last kernel; on a table with a delta
 * once more after mgx_batch_merge_local, where an entry's text comes from the index that holds the live document: the
 * delta's doc map is searched first). It reads the page's doc ids from the device result block and its records ride the
 * same event as the page. A batch without a highlighted query launches and copies nothing.
 *
 * mgx_batch_set_highlight attaches the requests to a prepared or reset batch, BEFORE its first execute; requests[i]
 * belongs to query i (n_queries = the batch's); mgx_batch_reset drops them. `terms` is the query's already-built term list
 * (search_pipeline::BuildHighlightTerms, search_pipeline.cpp:712-745: normalized, pieces added, sorted, deduplicated) as
 * byte strings; empty terms are skipped as the reference skips them. max_text_bytes: the longest document text a page
 * entry can have, 0 = the longest text of the batch's own index (a table with a delta passes the larger of the two,
 * mgx_index_max_text_bytes).
 * Refused: snippet_length outside 1..10000 or max_fragments outside 1..100 (the parser's ranges,
 * query_parser_clauses.cpp:372-431) and more than MGX_HIGHLIGHT_MAX_TERMS terms: MGX_ERR_OUT_OF_RANGE; a highlighted query
 * with limit 0 or offset + limit above 1024 (the fused top-k page bound; docid pages: limit above 1024):
 * MGX_ERR_OUT_OF_RANGE; an index without mgx_index_attach_text: MGX_ERR_INVALID_ARGUMENT; a batch whose records could,
 * in the worst case, exceed MGX_HIGHLIGHT_ARENA_CAP bytes: MGX_ERR_OUT_OF_RANGE (the message names the option to lower).
 * The worst case of one entry is min(4 * snippet_length * max_fragments, max_text_bytes) text bytes, as many match spans
 * as fit, and max_fragments windows. A sharded table (mgx_batch_exchange) cannot be highlighted: the page's texts live on
 * other ranks (MGX_ERR_NOT_IMPLEMENTED from mgx_batch_export_topk / _export_buffer, mgx_batch_merge_shards,
 * mgx_batch_exchange, mgx_batch_execute_gather and mgx_batch_execute_sharded, a host's own transport included).
 *
 * The texts are normalizer output, so valid UTF-8; a code point is a byte that is not 10xxxxxx. On other input the device
 * stays inside the text's bounds and the record's capacities, and the snippet is unspecified. */
#define MGX_HIGHLIGHT_ARENA_CAP (256ull << 20)
#define MGX_HIGHLIGHT_MAX_TERMS 256u
typedef struct mgx_highlight_request {
  uint32_t enabled;        /* 0: the query is not highlighted (the other fields are ignored) */
  uint32_t snippet_length; /* HighlightOptions::snippet_length (query_parser.h:158-163), code points per fragment */
  uint32_t max_fragments;
  uint32_t n_terms;
  const uint8_t* const* terms; /* term t = terms[t][0 .. term_lens[t]) */
  const uint32_t* term_lens;
} mgx_highlight_request;
int mgx_batch_set_highlight(mgx_batch* batch, const mgx_highlight_request* requests, uint32_t n_queries,
                            uint32_t max_text_bytes);
/* defer != 0: the batch's page is not final after mgx_batch_execute because mgx_batch_merge_local follows (the primary
 * batch of a table with a delta): execute then leaves the highlight kernel and the copy of its records to the merge,
 * which would otherwise repeat them. Call after mgx_batch_set_highlight; mgx_batch_reset clears it. */
int mgx_batch_defer_highlight(mgx_batch* batch, int defer);
/* What the host needs to render one page entry: the kept windows (byte ranges of the document, in order), the matches
 * inside them (byte ranges of the document, ascending; spans [windows[i-1].span_end, windows[i].span_end) belong to
 * window i and are clipped to it when rendered), and the windows' text (window i's bytes start at bytes + bytes_begin). */
#define MGX_HL_LEADING_DOTS 1u  /* "..." before the first window */
#define MGX_HL_TRAILING_DOTS 2u /* "..." after the last window */
#define MGX_HL_OVERFLOW 4u      /* a capacity cut the record short (mgx_batch_fetch_highlight refuses such a batch) */
typedef struct mgx_highlight_window {
  uint32_t start, end; /* bytes of the document */
  uint32_t span_end;
  uint32_t bytes_begin;
} mgx_highlight_window;
typedef struct mgx_highlight_span {
  uint32_t start, end;
} mgx_highlight_span;
typedef struct mgx_highlight_entry {
  uint32_t n_windows, flags, n_spans, n_bytes;
  const mgx_highlight_window* windows;
  const mgx_highlight_span* spans;
  const uint8_t* bytes;
} mgx_highlight_entry;
typedef struct mgx_highlight_view {
  uint32_t n_entries; /* = the docs of the last mgx_batch_fetch; entry i belongs to mgx_result_view.docs[i] */
  const mgx_highlight_entry* entries; /* queries that are not highlighted: all-zero entries */
} mgx_highlight_view;
/* After mgx_batch_fetch of the same execute: no further wait, no further copy. The view stays valid until the batch's
 * next execute, reset or destroy. */
int mgx_batch_fetch_highlight(mgx_batch* batch, mgx_highlight_view* out);
/* The host's share: tags and "..." around the record's bytes (GenerateWithPositions' rendering loop,
 * highlighter.cpp:188-222). Writes at most `cap` bytes to `out` and the snippet's full length to *out_len. Tags are at
 * most 256 bytes each (query_parser.h:276), else MGX_ERR_OUT_OF_RANGE. */
int mgx_highlight_render(const mgx_highlight_entry* entry, const uint8_t* open_tag, size_t open_len,
                         const uint8_t* close_tag, size_t close_len, uint8_t* out, size_t cap, size_t* out_len);
/* Length in bytes of the longest text attached to the index (0 without mgx_index_attach_text). */
int mgx_index_max_text_bytes(const mgx_index* idx, uint32_t* out);

/* ---- HIGHLIGHT from original texts (query::Highlighter::GenerateOriginal, src/query/highlighter.cpp:311-356; the
 * normal path of SearchHandler::GenerateHighlightSnippets, search_handler.cpp:277-307, for a document whose store holds
 * the text as the user wrote it). Matches are found in the NORMALIZED text, as always; each is translated to code points
 * of the original through a map the host builds once per document (one (cp_start, cp_end) pair per normalized code
 * point: the original segment it came from, :328-336), and the windows, spans and bytes of such an entry's record are
 * ranges and bytes of the ORIGINAL. Its `flags` carries MGX_HL_ORIGINAL. No Unicode work happens on the device.
 *
 * mgx_index_attach_original_text, after mgx_index_attach_text: arrays by doc slot; off has n_docs + 1 entries (bytes),
 * map_off n_docs + 1 entries counted in PAIRS of map_pairs (two uint32_t each); only MGX_ORIG_MAPPED documents have
 * pairs, so an index whose normalizer only folds case stores none. Everything is checked on the host, in one pass,
 * MGX_ERR_INVALID_ARGUMENT naming the slot: a kind above 3; pairs on a document that is not MAPPED; an original of kind
 * 1-3 that is not valid UTF-8 (render such a document on the host and attach it as MGX_ORIG_NONE); an IDENTITY document
 * whose code points differ in number from its normalized text's; a MAPPED document whose pairs differ in number from its
 * normalized text's code points, or hold a pair that is not start < end <= the original's code points, or whose starts
 * or ends decrease. Calling it again replaces the originals; mgx_index_attach_text called again drops them (they were
 * checked against the texts it replaces): attach them again after it.
 * mgx_batch_set_highlight(max_text_bytes = 0) sizes the records from the longer of the two texts; a table with a delta
 * passes the largest of mgx_index_max_text_bytes and mgx_index_max_original_text_bytes over both indexes. A batch on
 * indexes without originals launches the kernel it always launched. */
#define MGX_ORIG_NONE 0u       /* the document has no original: Generate over the normalized text */
#define MGX_ORIG_IDENTITY 1u   /* normalized code point i <-> original code points [i, i + 1): no map stored */
#define MGX_ORIG_MAPPED 2u     /* an explicit (cp_start, cp_end) pair per normalized code point */
#define MGX_ORIG_UNMAPPABLE 3u /* :342-344: the no-match window over the original, whatever the terms */
#define MGX_HL_ORIGINAL 8u     /* mgx_highlight_entry.flags: the entry was built from the document's original */
int mgx_index_attach_original_text(mgx_index* idx, const uint8_t* bytes, const uint64_t* off, const uint8_t* kind,
                                   const uint32_t* map_pairs, const uint64_t* map_off);
/* Length in bytes of the longest original attached to the index (0 without mgx_index_attach_original_text). */
int mgx_index_max_original_text_bytes(const mgx_index* idx, uint32_t* out);

/* ---- FACET in a batch (FACET <column> of many queries and columns per execute; mgx_facet_counts serves one query and
 * one column per call and waits for the device each time).
 * mgx_batch_set_facets attaches the requests to a prepared or reset batch, BEFORE its first execute and once;
 * requests[i] belongs to query i (n_queries = the batch's); mgx_batch_reset drops them. A faceted query (n_columns != 0)
 * must be MGX_SORT_DOCID with limit 0, the shape mgx_facet_counts forces. It returns NO page (n_docs = 0); its total and
 * its funnel counters are what the same query reports without the request. counts[v] of an entry is the number of
 * documents of the query's whole result set (terms or expression, NOT terms, filters, conditions, text post-filters, the
 * live row) whose value id in the column is v; NULLs are not counted. One more kernel (facet_batch_kernel) runs behind
 * the batch's others on the batch's stream: it reads each faceted query's result bitmap once, whatever the number of its
 * columns, after a memset of the counts; the counts ride the batch's result copy and its event. A batch without a
 * faceted query allocates, launches and copies nothing. The counts' device memory and pinned block are kept across
 * mgx_batch_reset and only grow. mgx_batch_merge_local leaves the counts per index, like the funnel counters: the caller
 * fetches the facets of both batches and adds them by value.
 * Refused: null arguments, a wrong n_queries, a second call, a call after the first execute, a faceted query of another
 * sort or with a limit, a column added without value_ids: MGX_ERR_INVALID_ARGUMENT; an unknown column, more than
 * MGX_FACET_MAX_COLUMNS columns in one request, counts above MGX_FACET_ARENA_CAP bytes in the batch: MGX_ERR_OUT_OF_RANGE
 * (the message names the query). A faceted batch handed to a sharded entry point (mgx_batch_export_topk /
 * _export_buffer, mgx_batch_merge_shards, mgx_batch_exchange, mgx_batch_execute_gather, mgx_batch_execute_sharded):
 * MGX_ERR_NOT_IMPLEMENTED, before anything is touched. */
#define MGX_FACET_MAX_COLUMNS 8u
#define MGX_FACET_ARENA_CAP (256ull << 20)
#define MGX_FACET_LDS_BINS 8192u /* 32-bit bins of the kernel's LDS histogram; columns past them count in global memory */
typedef struct mgx_facet_request {
  uint32_t n_columns;          /* 0: the query is not faceted */
  uint32_t reserved;           /* 0 */
  const uint32_t* column_ids;  /* ids from mgx_index_add_filter_column; the same id may appear twice */
} mgx_facet_request;
int mgx_batch_set_facets(mgx_batch* batch, const mgx_facet_request* requests, uint32_t n_queries);
typedef struct mgx_facet_entry {
  uint32_t query, column_id, n_values, reserved;
  const uint64_t* counts;      /* n_values */
} mgx_facet_entry;
typedef struct mgx_facet_view {
  uint32_t n_entries;          /* in query order, then in request order */
  const mgx_facet_entry* entries;
} mgx_facet_view;
/* After mgx_batch_fetch of the same execute: no further wait, no further copy. The view stays valid until the batch's
 * next execute, reset or destroy. */
int mgx_batch_fetch_facets(mgx_batch* batch, mgx_facet_view* out);

/* ---- Page documents (what turns a page into a response: DocumentStore::GetPrimaryKeysBatch behind the TCP handler's
 * "OK RESULTS <total> <pk> ...", response_formatter.cpp:280-332, and DocumentStore::GetDocumentsBatch behind the HTTP
 * handler's {primary_key, filters} objects, http_server.cpp:1396-1424) ----
 * mgx_index_attach_primary_key_bytes keeps the raw key bytes resident by local doc slot: key i is
 * bytes[off[i] .. off[i + 1]), off has n_docs + 1 ascending entries, has_key (n_docs bytes, may be NULL: every document
 * has a key) marks the documents that have one. The host copies are not kept. It is independent of
 * mgx_index_set_primary_keys (which keeps the keys' SORT form only: "007" and "7" are one value there); an index that
 * never calls it uses no more memory. Calling it again replaces the bytes. mgx_index_max_primary_key_bytes: the longest
 * attached key (0 without keys).
 * mgx_batch_set_documents attaches the requests to a prepared or reset batch, BEFORE its first execute and once;
 * requests[i] belongs to query i (n_queries = the batch's); mgx_batch_reset drops them. A requesting query (enabled != 0)
 * may have any sort, forward or reverse, and any offset, with 0 < limit <= 1024. column_ids are ids of
 * mgx_index_add_filter_column, repeats allowed, or MGX_DOC_NO_COLUMN: a column this index does not hold, NULL for every
 * document; n_columns 0: keys only. max_key_bytes sizes the records' key room: 0 = the longest key of the batch's own
 * index; a table with a delta passes the larger of the two indexes'. One more kernel (document_gather_kernel) runs behind
 * the kernel that finalises each page — in the execute for the score and doc-page groups, in mgx_batch_merge_local for
 * those groups of a table with a delta, and where mgx_batch_fetch cuts the pages of the bitmap group (deep SORT _score,
 * column and key sorts) — and adds no host synchronisation. A batch without a request allocates, launches and copies
 * nothing. The records' device memory and pinned block are kept across mgx_batch_reset and only grow.
 * mgx_batch_defer_documents(batch, 1): the execute skips the kernel and mgx_batch_merge_local runs it over the merged
 * page (the primary batch of a table with a delta; the delta's batch carries a request of the same shape, whose column
 * ids are the delta index's: same n_columns, same order).
 * Refused, each message naming the query: null arguments, a wrong n_queries, a second call, a call after the first
 * execute, a request on a faceted query, an index without attached key bytes, mgx_batch_fetch_documents before
 * mgx_batch_fetch: MGX_ERR_INVALID_ARGUMENT; limit 0 or above 1024, an unknown column id, more than MGX_DOC_MAX_COLUMNS
 * columns, a batch whose records could exceed MGX_DOC_ARENA_CAP bytes (the message names what to lower):
 * MGX_ERR_OUT_OF_RANGE. With MGX_ERR_NOT_IMPLEMENTED, before anything is touched: every sharded entry point
 * (mgx_batch_export_topk / _export_buffer, mgx_batch_merge_shards, mgx_batch_exchange, mgx_batch_execute_gather /
 * _sharded), because the rows live on other ranks; mgx_batch_merge_local over anything but one main index and one
 * delta. */
#define MGX_DOC_MAX_COLUMNS 32u
#define MGX_DOC_MAX_LIMIT 1024u
#define MGX_DOC_ARENA_CAP (256ull << 20)
#define MGX_DOC_NO_COLUMN 0xFFFFFFFFu
#define MGX_DOC_FOUND 1u   /* the doc id resolved to a slot of one of the batch's indexes */
#define MGX_DOC_HAS_KEY 2u
#define MGX_DOC_MAPPED 4u  /* the row came from the index that names documents through a doc map (the delta): a string
                            * rank in `values` belongs to that index's dictionary */
int mgx_index_attach_primary_key_bytes(mgx_index* idx, const uint8_t* bytes, const uint64_t* off, const uint8_t* has_key);
int mgx_index_max_primary_key_bytes(mgx_index* idx, uint32_t* out);
typedef struct mgx_document_request {
  uint32_t enabled;
  uint32_t n_columns;          /* <= MGX_DOC_MAX_COLUMNS; 0: keys only */
  const uint32_t* column_ids;  /* n_columns */
} mgx_document_request;
int mgx_batch_set_documents(mgx_batch* batch, const mgx_document_request* requests, uint32_t n_queries,
                            uint32_t max_key_bytes);
int mgx_batch_defer_documents(mgx_batch* batch, int defer);
typedef struct mgx_document_entry {
  uint32_t flags;      /* MGX_DOC_* */
  uint32_t key_len;
  uint32_t null_mask;  /* bit c: values[c] is NULL */
  uint32_t n_columns;
  const uint8_t* key;      /* key_len bytes */
  const uint64_t* values;  /* n_columns: the column's stored 8 bytes (int64, uint64, rank or double bits) */
} mgx_document_entry;
typedef struct mgx_document_view {
  uint32_t n_entries;  /* = the docs of the fetched view: entry i belongs to mgx_result_view.docs[i]; all zero for the
                        * queries without a request and for a doc id that no index of the batch holds */
  const mgx_document_entry* entries;
} mgx_document_view;
/* After mgx_batch_fetch of the same execute: no further wait, no further copy. The view stays valid until the batch's
 * next execute, reset or destroy. */
int mgx_batch_fetch_documents(mgx_batch* batch, mgx_document_view* out);
/* The same rows without a batch (DocumentStore::GetPrimaryKeysBatch / GetDocumentsBatch over a caller's id list,
 * document_store_retrieval.cpp:37-103): one pass of document_gather_kernel over doc_ids on a leased stand-alone call, like
 * the single operators; safe from many threads at once. `mapped`: NULL, or the table's delta index (mgx_index_set_doc_map)
 * on the same device, searched first; mapped_column_ids are its ids for the same n_columns columns (MGX_DOC_NO_COLUMN
 * on either side: NULL). *records_out (malloc: mgx_free) holds n_docs records of *stride_out bytes, record i for
 * doc_ids[i]: [mgx_document_record_header | n_columns x uint64_t values | key bytes], all zero for an id neither index
 * holds. max_key_bytes 0: the longest key of the indexes given. Refused: null arguments, an index without attached key
 * bytes, a `mapped` that is no delta: MGX_ERR_INVALID_ARGUMENT; an unknown column id, more than MGX_DOC_MAX_COLUMNS
 * columns, records above MGX_DOC_ARENA_CAP bytes, a key longer than max_key_bytes: MGX_ERR_OUT_OF_RANGE. */
typedef struct mgx_document_record_header {
  uint32_t flags;      /* MGX_DOC_* */
  uint32_t key_len;
  uint32_t null_mask;
  uint32_t n_columns;
} mgx_document_record_header;
int mgx_documents_gather(mgx_index* idx, mgx_index* mapped, const uint32_t* doc_ids, uint64_t n_docs, uint32_t n_columns,
                         const uint32_t* column_ids, const uint32_t* mapped_column_ids, uint32_t max_key_bytes,
                         uint8_t** records_out, uint64_t* stride_out);

/* Multi-GPU exchange (one rank per doc-range shard). The batch must be all MGX_SORT_SCORE, or all docid-ordered
 * pages (MGX_SORT_DOCID with 0 < limit <= 16384): a page is a best-first list under the key "doc id" (or its
 * complement for ascending order), so the same two calls serve both.
 * Copies this shard's per-query top-(offset+limit) of the last execute into two CALLER-owned DEVICE blobs on
 * `hip_stream`, laid out so that ONE all-gather per blob moves everything:
 *   blob64[n_queries*stride + n_queries] : keys (order-preserving u64 of the fp64 score, best first, `stride` per
 *                                           query), then this shard's match count per query;
 *   blob32[n_queries*stride + n_queries] : doc ids parallel to the keys, then the number of valid entries per query.
 * Call with both blobs NULL to only learn *stride. */
int mgx_batch_export_topk(mgx_batch* batch, uint64_t* blob64, uint32_t* blob32, uint32_t* stride, void* hip_stream);
/* Zero-copy form of the export for MGX_SORT_SCORE batches: the library keeps the shard's result in the exchange layout
 * already; *device_blob is that buffer (blob64 at offset 0, blob32 at *offset32 bytes, *bytes in all, a multiple of 8),
 * valid once the execute it belongs to has completed on its stream. NULL for other batches (use
 * mgx_batch_export_topk). */
int mgx_batch_export_buffer(mgx_batch* batch, void** device_blob, uint64_t* bytes, uint64_t* offset32);
/* Merges the blobs of `n_shards` ranks into the final page and total of every query, on `hip_stream`; read the
 * result with mgx_batch_fetch. Rank r's 64-bit blob starts at blob64 + r*pitch64 (u64 elements), its 32-bit blob at
 * blob32 + r*pitch32 (u32 elements); pitch 0 = the blob's own size (blobs gathered separately, rank after rank).
 * With explicit pitches a rank can export both blobs into ONE buffer (blob32 right behind blob64) and a single
 * all-gather moves everything: pitch64 = bytes_per_rank/8, pitch32 = bytes_per_rank/4. */
int mgx_batch_merge_shards(mgx_batch* batch, uint32_t n_shards, const uint64_t* blob64, uint64_t pitch64,
                           const uint32_t* blob32, uint64_t pitch32, void* hip_stream);
/* The collective of the sharded path behind this ABI (RCCL, loaded on first use): one communicator per rank of a table
 * whose shards are doc ranges, one rank per GPU. Rank 0 draws the id (mgx_comm_unique_id), the host layer hands its
 * MGX_COMM_ID_BYTES bytes to every rank by whatever channel it has (the reference has none to replace: it is a single
 * process), every rank calls mgx_comm_create — collectively.
 * mgx_batch_exchange, after mgx_batch_execute on the same stream: all-gathers every shard's per-query top-(offset+limit)
 * (ONE ncclAllGather of the batch's exchange blob) and merges them (mgx_batch_merge_shards); mgx_batch_fetch then
 * returns the table-wide page and total on every rank. mgx_batch_exchange_df, BEFORE mgx_batch_execute: the df pass of
 * the batch's text-level terms + ONE ncclAllReduce of their counts (no-op without such terms). Every rank must call
 * the same sequence of exchanges on its communicator, in the same order. */
#define MGX_COMM_ID_BYTES 128
typedef struct mgx_comm mgx_comm;
int mgx_comm_unique_id(uint8_t* id /* [MGX_COMM_ID_BYTES] */);
int mgx_comm_create(const uint8_t* id, int rank, int world, int device, mgx_comm** out);
void mgx_comm_destroy(mgx_comm* comm);
/* ncclCommAbort: this rank leaves the communicator NOW — its enqueued collectives are cancelled instead of waited for, and
 * every later exchange on `comm` fails with MGX_ERR_INTERNAL. What a rank must do when it cannot issue a batch's
 * collectives (a local failure between compile and exchange): its peers have issued theirs and would otherwise wait for
 * ever; with this rank gone their collectives fail or time out under the job's own watchdog, and the process exits
 * non-zero. The handle stays valid for mgx_comm_destroy. */
int mgx_comm_abort(mgx_comm* comm);
int mgx_batch_exchange_df(mgx_batch* batch, mgx_comm* comm, void* hip_stream);
int mgx_batch_exchange(mgx_batch* batch, mgx_comm* comm, void* hip_stream);
/* mgx_batch_execute for a shard of a table (every rank calls it for the same batch, in the same order; follow it with
 * mgx_batch_exchange): SORT _score batches run their seed items first, all-gather the seeds' best keys (ONE small
 * ncclAllGather: offset+limit keys per query and rank) and raise every query's pruning bound to the (offset+limit)-th best
 * key of the union before the rest of the batch runs — a shard's own matches give a weak bound (top-k is a property of
 * the whole table). The shard's LOCAL page may then hold fewer than offset+limit docs: those it lacks are on no rank's
 * share of the table-wide page; totals and funnel counters are unaffected. Other batches: as mgx_batch_execute. The
 * exchange runs from four ranks up (MGX_SEED_EXCHANGE=0 / 1 in every rank's environment forces it off / on; otherwise
 * this call is mgx_batch_execute) and is entered by every rank or by none: the decision uses the queries and the world
 * size only (shards of a million docs and more, MGX_SEED_EXCHANGE_MIN_DOCS). */
int mgx_batch_execute_sharded(mgx_batch* batch, mgx_comm* comm, void* hip_stream);
/* The same with the caller's transport (a test's gloo all-gather, MPI, ...): `gather` must fill all[r * bytes ..] with
 * rank r's `mine` for every rank (both are DEVICE buffers of the batch; the call may enqueue on hip_stream or block) and
 * return MGX_OK. */
typedef int (*mgx_gather_fn)(void* user, const void* mine, void* all, uint64_t bytes, void* hip_stream);
int mgx_batch_execute_gather(mgx_batch* batch, int world, mgx_gather_fn gather, void* user, void* hip_stream);
/* Text-level terms across shards: df must be table-wide before idf is taken. mgx_batch_count_df enqueues only the df
 * pass of the batch's text-level terms; mgx_batch_df_buffer exposes the DEVICE array of their counts (u64 per DISTINCT
 * term of the batch, in order of first appearance — the same on every shard), which the caller sums over ranks in place (one RCCL all-reduce); the next
 * mgx_batch_execute then uses those counts instead of running its own df pass. *n == 0: nothing to exchange. */
int mgx_batch_count_df(mgx_batch* batch, void* hip_stream);
int mgx_batch_df_buffer(mgx_batch* batch, uint64_t** device_counts, uint32_t* n);
/* Algorithmic bytes of one execute (4*sum|L_i| + R*(T+4) + 12*min(k,R), summed over queries); R is
 * taken from the last fetched execute. */
int mgx_batch_algorithmic_bytes(mgx_batch* batch, uint64_t* list_bytes, uint64_t* score_bytes, uint64_t* topk_bytes);
/* Average duration (ms) of the dominant kernel over the executes since the last call, measured with HIP events on
 * the stream the kernel ran on; *n receives how many launches were averaged. Enables event recording from now on. */
int mgx_batch_kernel_time_ms(mgx_batch* batch, double* avg_ms, uint32_t* n);
/* Reads the batch's index: destroy every batch of an index before mgx_index_destroy. */
void mgx_batch_destroy(mgx_batch* batch);

/* =====================================================================================================
 * Single operators (what the shim's Index / BM25Scorer / ResultSorter methods call)
 * ===================================================================================================== */

/* Index::SearchAnd(terms, limit, reverse): every gram known (the caller returns {} otherwise). */
int mgx_and(mgx_index* idx, const uint32_t* gram_ids, uint32_t n, uint64_t limit, int reverse, uint32_t** out_docs,
            uint64_t* out_n);
/* Index::SearchOr: unknown grams already dropped by the caller. */
int mgx_or(mgx_index* idx, const uint32_t* gram_ids, uint32_t n, uint32_t** out_docs, uint64_t* out_n);
/* Index::SearchNot(all_docs, terms): all_docs ascending. */
int mgx_not(mgx_index* idx, const uint32_t* all_docs, uint64_t n_all, const uint32_t* gram_ids, uint32_t n,
            uint32_t** out_docs, uint64_t* out_n);
/* Index::SearchByThreshold over DISTINCT known grams (the caller dedupes and handles the delegate/empty rules,
 * index.cpp:489-523). */
int mgx_threshold(mgx_index* idx, const uint32_t* gram_ids, uint32_t n, uint32_t threshold, uint32_t** out_docs,
                  uint64_t* out_n);
/* Index::FilterByNgrams: keeps caller order and duplicates. */
int mgx_retain(mgx_index* idx, const uint32_t* candidates, uint64_t n_cand, const uint32_t* gram_ids, uint32_t n,
               uint32_t** out_docs, uint64_t* out_n);
/* FACET (ExecuteFacetPipeline, src/server/search_pipeline.cpp:2061-2153): counts_out[v] = how many docs of the query's
 * result set hold value id v of the column (FilterIndex::GetColumnValueCountsFiltered, filter_index.cpp:284-312 — a
 * histogram of the column's value ids over the result bitmap); *matched = the size of the result set. `query` is the
 * search part (terms / expression, NOT terms, filters; sort, limit and offset are ignored: the whole result set counts);
 * the caller orders the values by count and pages them. counts_out has room for the column's n_values. */
int mgx_facet_counts(mgx_index* idx, const mgx_query* query, uint32_t column_id, uint64_t* counts_out, uint64_t* matched);

/* ---- mutable tables (the binlog applier's Index::AddDocument / UpdateDocument / RemoveDocument,
 * src/index/index.cpp:39-233, after the index was built) -------------------------------------------------------------
 * The column arrays of an mgx_index are immutable. A table that changes is TWO indexes on one device: the MAIN index as
 * built, with a LIVE row (a filter bitmap whose bits are cleared as documents are removed or superseded), and a small
 * DELTA index over the documents added or changed since, numbered 1..n in ascending order of their table ids with a doc
 * map back to those ids. A batch is compiled against both (same queries, table-wide statistics in both: the df the
 * planner passes, total_docs, avg_doc_length), both are executed on ONE stream, and the delta's pages are merged into
 * the main batch — the exchange of a sharded table without the wire. The host layer (mygram_shim: Index::AddDocument &
 * co.) owns the bookkeeping and rebuilds the delta when it changes; when the delta has grown it rebuilds the main index.
 *
 * mgx_index_set_live_bitmap: every batched query (and every df query of a text-level term) on `idx` is ANDed with this
 *   filter row right after its first term, so candidates, totals and funnel counters count live documents only; the
 *   single-operator entry points (mgx_and ...) do NOT apply it. enable = 0 turns it off.
 * mgx_index_update_filter_bitmap: sets / clears bits of a filter row in place (ids are table doc ids of this index's
 *   range). Not ordered against batches in flight: call it between batches (mgx_index_synchronize) when a batch must see
 *   either all or none of an update.
 * mgx_index_set_doc_map: table id of every doc slot (ascending) — mgx_batch_merge_local reports this index's documents
 *   under these ids.
 * mgx_index_invalidate_statistics: drops everything the index cached per (total_docs, avg_doc_length, idf): contribution
 *   tables, length norms, block-max bounds, df counts. Call when the table-wide statistics changed, with NO batch of this
 *   index compiled or in flight (compiled batches hold table addresses); it waits for the device.
 * mgx_batch_df_merge_local, before the executes: df pass of the text-level terms on every batch, summed, the sum handed
 *   to every batch (mgx_batch_exchange_df without the all-reduce).
 * mgx_batch_merge_local, after the executes, all on `hip_stream`: merges the others' top-(offset+limit) per query into
 *   `primary` (mgx_batch_exchange without the all-gather); mgx_batch_fetch(primary) then returns the table-wide page
 *   and total. Funnel counters stay per index: fetch the others too and add them. Unlike the exchange, a batch may mix
 *   SORT _score pages, docid pages and queries without a page bound (limit 0, docid pages past 16384, SORT _score past
 *   offset+limit 1024); each group is merged on its own. The last group's page sizes are known only once the totals
 *   are on the host, so merge_local records the (one) other batch and mgx_batch_fetch(primary) merges it there: each
 *   side materialises what the page can need, and a rank merge on the device cuts the page of the two sorted runs.
 *   mgx_batch_fetch(other) then returns that batch's funnel counters and its own total, with n_docs = 0 for those
 *   queries. The others must stay untouched until primary has been fetched. */
/* Compaction of a mutable table (the main index is rebuilt from the table's current documents): the texts the index holds
 * (mgx_index_attach_text) and a filter column's arrays back on the host. mgx_index_copy_text with both buffers NULL only
 * reports *total_bytes; text_off has room for n_docs + 1 entries (offsets start at 0). */
int mgx_index_copy_text(mgx_index* idx, uint8_t* text_bytes, uint64_t capacity, uint64_t* text_off, uint64_t* total_bytes);
int mgx_index_filter_column_export(mgx_index* idx, uint32_t column_id, uint64_t* values, uint8_t* is_null,
                                   uint32_t* value_ids /* may be NULL */);
/* One document's text (text NULL: only *len). */
int mgx_index_read_text(mgx_index* idx, uint32_t doc_id, uint8_t* text, uint64_t capacity, uint64_t* len);
/* One document's stored value of a filter column, as it was given to mgx_index_add_filter_column (a document that moves
 * to the delta index takes its filter values along). value_id may be NULL. */
int mgx_index_filter_column_read(mgx_index* idx, uint32_t column_id, uint32_t doc_id, uint64_t* value_bits, int* is_null,
                                 uint32_t* value_id);
/* enable: 0 off, 1 on, MGX_LIVE_BITMAPS_CLEAN: on, and the caller also takes every dead document out of the bitmap form of
 * its dense grams (mgx_index_clear_postings with the document's distinct n-grams, BEFORE clearing its live bit): a query
 * whose first term is made of bitmap-form grams only then holds live documents by construction and gets no live-row operand
 * (the benchmark's 3-term AND keeps its three operands). */
#define MGX_LIVE_BITMAPS_CLEAN 3
int mgx_index_set_live_bitmap(mgx_index* idx, uint32_t bitmap_id, int enable);
/* Clears posting (docids[i], gram_ids[i]) in the gram's bitmap form, if it has one (list-form grams are left alone: queries
 * that read them keep the live-row operand). Same ordering rule as mgx_index_update_filter_bitmap. */
int mgx_index_clear_postings(mgx_index* idx, const uint32_t* docids, const uint32_t* gram_ids, uint64_t n);
int mgx_index_update_filter_bitmap(mgx_index* idx, uint32_t bitmap_id, const uint32_t* set_docids, uint64_t n_set,
                                   const uint32_t* clear_docids, uint64_t n_clear);
int mgx_index_set_doc_map(mgx_index* idx, const uint32_t* table_ids, uint64_t n);
int mgx_index_invalidate_statistics(mgx_index* idx);
int mgx_index_synchronize(mgx_index* idx);
/* The primary keys of an index by local doc slot, for MGX_SORT_PRIMARY_KEY: key i is bytes[off[i] .. off[i + 1]), off has
 * n_docs + 1 entries; has_key (NULL: every document has a key) marks the documents that have one, the others sort by
 * their table doc id. The library derives the sort keys, stores 8 bytes per slot (the number when every key of the index
 * is numeric, else the key's rank among the index's distinct keys plus that dictionary) and copies what it needs: the
 * arrays may be freed after the call. Calling it again replaces the keys; no batch of this index may be between execute
 * and fetch then (the call waits for the device and frees the old column). On a delta index call it after
 * mgx_index_set_doc_map, which names the table ids the documents without a key fall back to.
 * mgx_index_set_primary_key_shortcut: enable = 0 keeps MGX_SORT_PRIMARY_KEY queries of this index from running as docid
 * pages; the owner of a table does that on the main index while a delta index exists, since the two sides' runs are
 * then merged by key. An index with a doc map never takes the shortcut. Default: enabled. */
int mgx_index_set_primary_keys(mgx_index* idx, const uint8_t* bytes, const uint64_t* off, const uint8_t* has_key);
int mgx_index_set_primary_key_shortcut(mgx_index* idx, int enable);
int mgx_batch_df_merge_local(mgx_batch* primary, mgx_batch* const* others, uint32_t n_others, void* hip_stream);
int mgx_batch_merge_local(mgx_batch* primary, mgx_batch* const* others, uint32_t n_others, void* hip_stream);

/* BM25Scorer::ScoreDocuments for single-gram terms: one score per candidate, in candidate order. A candidate
 * outside the index or with empty text scores 0.0 (bm25_scorer.cpp:73-89). */
int mgx_score_documents(mgx_index* idx, const uint32_t* candidates, uint64_t n_cand, const uint32_t* gram_ids,
                        const double* idfs, uint32_t n_terms, double avg_doc_length, double k1, double b,
                        double* scores_out);
/* BM25Scorer::ScoreDocuments for terms of any length: tf counted in the doc text as the reference does
 * (CountTermOccurrences, bm25_scorer.cpp:27-45). Terms are normalized bytes, term t = term_bytes[term_off[t] ..
 * term_off[t+1]). Needs mgx_index_attach_text. */
int mgx_score_documents_text(mgx_index* idx, const uint32_t* candidates, uint64_t n_cand, const uint8_t* term_bytes,
                             const uint32_t* term_off, const double* idfs, uint32_t n_terms, double avg_doc_length,
                             double k1, double b, double* scores_out);
/* ResultSorter::SortByScore, any length, any page (limit 0 = all): a bounded page (offset+limit <= 1024) of a long
 * array is selected by per-wave top-k scans + a merge, everything else by a full device sort of the (score, docid)
 * pairs (the reference is benchmarked with OFFSET 10000, docs/releases/v1.3.5.md:238). n < 2^32. */
int mgx_sort_by_score(mgx_index* idx, const uint32_t* results, const double* scores, uint64_t n, int descending,
                      uint32_t limit, uint32_t offset, uint32_t** out_docs, uint64_t* out_n);

#ifdef __cplusplus
}
#endif
#endif /* MYGRAM_GPU_H_ */
