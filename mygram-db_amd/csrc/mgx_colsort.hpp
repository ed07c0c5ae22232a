// mgx_colsort.hpp — SORT <filter column> ASC|DESC (ResultSorter::SortAndPaginate, result_sorter.cpp:489-650): the 64-bit
// restatement of the reference's string sort key, the collision scan of a column, and the launchers of mgx_colsort.hip.
// Host and device share the key transform; the host part compiles without a HIP header (the stand-alone checks do).
#pragma once
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#define MGX_CS_HD __host__ __device__
#else
#define MGX_CS_HD
#endif

namespace mgx {
namespace colsort {

// value classes of a filter column (MGX_FC_* of mygram_gpu.h) and how an unsigned column's values are read
constexpr uint32_t kSigned = 0, kUnsigned = 1, kDouble = 2;
constexpr uint64_t kSignBit = 1ull << 63;

// T(v): unsigned order of T = the order of FilterValueToSortKey's strings (result_sorter.cpp:187-217). NULL is 0 (the
// empty key, :192). ranks: the column holds dictionary ranks of strings (the key is the string itself, :195-196):
// rank + bias, bias 0 when the dictionary holds "" (which then ties with NULL, both keys being ""), else 1.
MGX_CS_HD inline uint64_t KeyOf(uint32_t value_class, bool ranks, uint64_t bias, uint64_t v, bool is_null) {
  if (is_null) return 0;
  if (value_class == kSigned) return v ^ kSignBit;                    // ToZeroPaddedSignedString, :116-119
  if (value_class == kDouble) return (v >> 63) ? ~v : (v ^ kSignBit);  // ToZeroPaddedDoubleString, :136-148
  if (ranks) return v + bias;
  return v <= (kSignBit - 1) ? (v | kSignBit) : v;  // :205-212 (the reference's own rule: 0 and 2^63 share a key)
}

// The carried pair, ordered by better(): (T, doc) for DESC, (~T, ~doc) for ASC — ties go to the larger doc id in DESC and
// to the smaller in ASC (CompareDocIdTie, :43-45).
MGX_CS_HD inline uint64_t PairKey(uint64_t t, bool descending) { return descending ? t : ~t; }
MGX_CS_HD inline uint32_t PairDoc(uint32_t doc, bool descending) { return descending ? doc : ~doc; }
MGX_CS_HD inline bool Better(uint64_t ka, uint32_t da, uint64_t kb, uint32_t db) {
  return ka > kb || (ka == kb && da > db);
}

// A non-NULL value whose T is 0 (INT64_MIN; the double whose bits are all ones) cannot be told from NULL in 64 bits. One
// pass over the values mgx_index_add_filter_column is handed finds both ingredients; a column that has both — or, on a
// table with a delta index, a pair of columns that has both between them, since their runs are merged by key — is not
// sortable. (Unsigned: T >= 2^63, never 0; ranks: "" is meant to tie with NULL.)
struct KeyScan {
  bool any_null = false;  // a NULL
  bool any_zero = false;  // a non-NULL value whose T is 0
};
inline KeyScan ScanKeys(uint32_t value_class, const uint64_t* values, const uint8_t* is_null, uint64_t n) {
  KeyScan k;
  for (uint64_t i = 0; i < n; ++i) {
    if (is_null != nullptr && is_null[i]) k.any_null = true;
    else if (value_class != kUnsigned && KeyOf(value_class, false, 0, values[i], false) == 0) k.any_zero = true;
  }
  return k;
}
inline bool KeysCollide(const KeyScan& a, const KeyScan& b) { return (a.any_null || b.any_null) && (a.any_zero || b.any_zero); }
inline bool HasKeyCollision(uint32_t value_class, const uint64_t* values, const uint8_t* is_null, uint64_t n) {
  const KeyScan k = ScanKeys(value_class, values, is_null, n);
  return KeysCollide(k, k);
}

constexpr uint32_t kMaxNeeded = 1024;   // offset + limit the fused selection serves
constexpr uint32_t kTopkBlock = 256;    // four waves
constexpr uint32_t kTopkMaxGroups = 16;  // workgroups per (query, side)

// One (query, side) of a fused selection.
struct TopkJob {
  const uint64_t* rbits;   // the side's result bitmaps [slot][tile][256 words]
  const uint64_t* values;  // the column by local doc slot
  const uint8_t* is_null;  // or nullptr: no NULLs
  const uint32_t* doc_map; // local slot -> table id (a merge), or nullptr: first_doc_id + slot
  uint64_t word_begin;     // the query's first word in rbits
  uint64_t out_off;        // the job's sorted run in the key / docid' buffers
  uint64_t list_off;       // its per-workgroup lists [n_groups][needed] in the list buffers
  uint32_t n_words;        // 256 * n_tiles
  uint32_t n_docs, first_doc_id;
  uint32_t needed;         // pairs wanted: min(total, offset + limit), 1..kMaxNeeded
  uint32_t cap;            // power of two >= max(needed, 64)
  uint32_t n_groups;       // workgroups of this job
  uint32_t group_begin;    // its first workgroup among the launch's
  uint32_t value_class, ranks, bias, descending;
};

}  // namespace colsort
}  // namespace mgx

#if defined(__HIPCC__) || defined(MGX_COLSORT_LAUNCHERS)
#include <hip/hip_runtime_api.h>
namespace mgx {
// (key, docid') pairs of an expanded doc array (first_doc_id + local slot, as expand_kernel writes it); doc_map: as in
// TopkJob. docs is left as it is.
int LaunchColumnKeys(const uint32_t* docs, uint64_t n, const uint64_t* values, const uint8_t* is_null,
                     const uint32_t* doc_map, uint32_t first_doc_id, uint32_t n_docs, uint32_t value_class,
                     uint32_t ranks, uint32_t bias, int descending, uint64_t* keys, uint32_t* dprime, hipStream_t s);
// Every job's best `needed` pairs, sorted best first, at keys/dprime + out_off. jobs: device array; n_groups_total: the
// sum of n_groups; max_cap: the largest cap (sizes the LDS); max_job_elems: the largest n_groups * needed; list_keys/list_docs: scratch for the per-workgroup lists.
int LaunchColumnTopk(const colsort::TopkJob* jobs, uint32_t n_jobs, uint32_t n_groups_total, uint32_t max_cap,
                     uint32_t max_job_elems, uint64_t* list_keys, uint32_t* list_docs, uint32_t* list_n, uint64_t* keys,
                     uint32_t* dprime, hipStream_t s);
uint32_t ColumnTopkLdsBytes(uint32_t cap);
}  // namespace mgx
#endif
