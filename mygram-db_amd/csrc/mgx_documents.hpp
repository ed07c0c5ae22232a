// mgx_documents.hpp — page documents (mgx_batch_set_documents): the host-side record and arena plan of one batch's
// document requests, the descriptors document_gather_kernel reads, and the launcher of mgx_documents.hip. The plan and
// the host restatement of the gather are plain C++ and compile without a HIP header (tests/cpp/documents_plan_check.cpp
// pins them under the sanitizers); mgx_api.cpp calls the plan and restates nothing.
//
//   record   one per (requesting query, page entry), a fixed stride per query:
//              [Header 16 B | values n_columns x u64 | key bytes, key_cap rounded up to 8]
//            entry j of a query is at rec_off + j * rec_stride: no prefix sum, every record 8-byte aligned
//   arena    the worst case, `limit` entries per requesting query, at most kArenaCap bytes. The queries whose page is
//            final behind the execute (score group, doc-page group: `late` = 0) come first, in request order, so that one
//            copy of [0, early_bytes) brings them; the queries of the bitmap group (`late` = 1: their page sizes are known
//            on the host when the page is cut) follow, and are packed by their actual sizes at fetch time inside
//            [early_bytes, arena_bytes)
//   resolve  a doc id names a slot of the mapped index (ascending doc map, binary search) or else of the plain index
//            (doc - first_doc_id); a doc id neither holds is not found and nothing of either index is read for it
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

#if defined(__HIPCC__)
#define MGX_DOC_HD __host__ __device__
#else
#define MGX_DOC_HD
#endif

namespace mgx {
namespace documents {

constexpr uint32_t kMaxColumns = 32;          // MGX_DOC_MAX_COLUMNS (one bit each in the 32-bit null mask)
constexpr uint32_t kMaxLimit = 1024;          // the largest page a request rides (the reference's LIMIT ends at 1000)
constexpr uint64_t kArenaCap = 256ull << 20;  // MGX_DOC_ARENA_CAP
constexpr uint32_t kNoColumn = 0xFFFFFFFFu;   // MGX_DOC_NO_COLUMN
constexpr uint32_t kFound = 1u, kHasKey = 2u, kMapped = 4u;  // MGX_DOC_FOUND / _HAS_KEY / _MAPPED
constexpr uint32_t kTruncated = 0x80000000u;  // internal: the key is longer than the records' key capacity

struct Header {
  uint32_t flags, key_len, null_mask, n_columns;
};
static_assert(sizeof(Header) == 16, "a record's header is two 8-byte words");

inline uint64_t RecordStride(uint32_t n_columns, uint32_t key_cap) {
  return sizeof(Header) + 8ull * n_columns + ((static_cast<uint64_t>(key_cap) + 7) & ~7ull);
}

struct Request {
  uint32_t query = 0;      // batch index
  uint32_t limit = 0;      // the query's page size
  uint32_t n_columns = 0;
  uint32_t late = 0;       // 1: the page is cut at fetch time (bitmap group)
};

struct QueryPlan {
  uint32_t query = 0, limit = 0, n_columns = 0, late = 0;
  uint32_t col_begin = 0;    // its columns in the batch's column arrays
  uint32_t entry_begin = 0;  // early queries: its first entry among the early entries
  uint64_t rec_off = 0, rec_stride = 0;
};

struct Plan {
  std::vector<QueryPlan> queries;  // in request order
  uint32_t key_cap = 0;
  uint32_t n_columns = 0;      // of all queries together
  uint32_t early_entries = 0;  // sum of the early queries' limits
  uint64_t early_bytes = 0, arena_bytes = 0;
};

enum Status { kOk = 0, kTooManyColumns = 1, kBadLimit = 2, kArenaTooLarge = 3 };

// Plans the requests of one batch. On a refusal *bad names the request's position. kArenaTooLarge fires exactly when
// the sum of limit * RecordStride over the requests passes kArenaCap, at the first request (in request order) with
// which the running sum does.
inline Status Build(const std::vector<Request>& requests, uint32_t key_cap, Plan* out, size_t* bad) {
  Plan p;
  p.key_cap = key_cap;
  p.queries.resize(requests.size());
  uint64_t sum = 0, early = 0;
  uint32_t cols = 0;
  for (size_t r = 0; r < requests.size(); ++r) {
    const Request& rq = requests[r];
    if (rq.n_columns > kMaxColumns) {
      if (bad) *bad = r;
      return kTooManyColumns;
    }
    if (rq.limit == 0 || rq.limit > kMaxLimit) {
      if (bad) *bad = r;
      return kBadLimit;
    }
    QueryPlan& q = p.queries[r];
    q.query = rq.query;
    q.limit = rq.limit;
    q.n_columns = rq.n_columns;
    q.late = rq.late ? 1u : 0u;
    q.col_begin = cols;
    cols += rq.n_columns;
    q.rec_stride = RecordStride(rq.n_columns, key_cap);
    sum += q.rec_stride * rq.limit;
    if (sum > kArenaCap) {
      if (bad) *bad = r;
      return kArenaTooLarge;
    }
    if (!q.late) early += q.rec_stride * rq.limit;
  }
  uint64_t at_early = 0, at_late = early;
  for (QueryPlan& q : p.queries) {
    uint64_t& at = q.late ? at_late : at_early;
    q.rec_off = at;
    at += q.rec_stride * q.limit;
    if (!q.late) {
      q.entry_begin = p.early_entries;
      p.early_entries += q.limit;
    }
  }
  p.n_columns = cols;
  p.early_bytes = early;
  p.arena_bytes = sum;
  *out = std::move(p);
  return kOk;
}

// ---- what the kernel reads (device memory; the host restatement below reads host arrays through the same structs) ----
struct DevColumn {
  const uint64_t* values;   // by local doc slot; null: the index does not hold the column (NULL for every document)
  const uint8_t* is_null;   // or null: no NULLs
};
// One index of the batch: its resident key bytes, its doc map and the requested columns of every query.
struct DevSource {
  const uint8_t* key_bytes;   // null: no such source
  const uint64_t* key_off;    // [n_docs + 1]
  const uint8_t* has_key;     // [n_docs] or null: every document has a key
  const uint32_t* doc_map;    // [n_docs] ascending table ids (the mapped source), or null
  const DevColumn* columns;   // [Plan::n_columns]
  uint32_t first_doc_id, n_docs;
};
// One requesting query. Its page is read where the batch's last kernel left it: page_docs[j], j < the page's entry
// count = *page_n (SORT _score), min(*total, limit) of a doc-id page (total_exec after an execute, total_merged after
// mgx_batch_merge_local), or `count` (bitmap group: known on the host).
struct DevQuery {
  const uint32_t* page_docs;
  const uint32_t* page_n;
  const unsigned long long* total_exec;
  const unsigned long long* total_merged;
  uint32_t limit, entry_begin;
  uint32_t n_columns, col_begin;
  uint32_t count, reserved;
  uint64_t rec_off, rec_stride;
};
struct DevBatch {
  const DevQuery* queries;
  uint32_t n_queries, n_entries;
  uint8_t* arena;
  DevSource mapped, plain;
  uint32_t key_cap, merged;
};

// Which slot of which source a doc id names: 0 = neither, 1 = mapped, 2 = plain. Reads doc_map[0, n_docs) only.
MGX_DOC_HD inline uint32_t Resolve(const DevSource& mapped, const DevSource& plain, uint32_t doc, uint32_t* slot) {
  if (mapped.key_off && mapped.doc_map) {
    uint32_t a = 0, b = mapped.n_docs;  // first slot with doc_map[slot] >= doc
    while (a < b) {
      const uint32_t mid = a + ((b - a) >> 1);
      if (mapped.doc_map[mid] < doc) a = mid + 1;
      else b = mid;
    }
    if (a < mapped.n_docs && mapped.doc_map[a] == doc) {
      *slot = a;
      return 1;
    }
  }
  if (plain.key_off && doc >= plain.first_doc_id && doc - plain.first_doc_id < plain.n_docs) {
    *slot = doc - plain.first_doc_id;
    return 2;
  }
  return 0;
}

// The key of `slot`: its bytes' begin in key_bytes and its length cut to key_cap (*truncated says so). Reads
// key_off[slot], key_off[slot + 1] and has_key[slot]; the bytes it names lie inside [off[slot], off[slot + 1]).
MGX_DOC_HD inline bool KeyOf(const DevSource& src, uint32_t slot, uint32_t key_cap, uint64_t* begin, uint32_t* len,
                             bool* truncated) {
  *begin = 0;
  *len = 0;
  *truncated = false;
  if (src.has_key && src.has_key[slot] == 0) return false;
  const uint64_t k0 = src.key_off[slot], k1 = src.key_off[slot + 1];
  const uint64_t n = k1 > k0 ? k1 - k0 : 0;
  *begin = k0;
  *truncated = n > key_cap;
  *len = *truncated ? key_cap : static_cast<uint32_t>(n);
  return true;
}

// Host restatement of one entry of the gather, lane by lane what the wave does: the record of `doc` into
// rec[0, RecordStride(n_columns, key_cap)).
inline void GatherEntryHost(const DevSource& mapped, const DevSource& plain, uint32_t doc, uint32_t n_columns,
                            uint32_t col_begin, uint32_t key_cap, uint8_t* rec) {
  Header h{0, 0, 0, 0};
  uint32_t slot = 0;
  const uint32_t which = Resolve(mapped, plain, doc, &slot);
  if (which != 0) {
    const DevSource& src = which == 1 ? mapped : plain;
    h.flags = kFound | (which == 1 ? kMapped : 0u);
    h.n_columns = n_columns;
    for (uint32_t c = 0; c < n_columns; ++c) {
      const DevColumn col = src.columns[col_begin + c];
      const bool nul = !col.values || (col.is_null && col.is_null[slot] != 0);
      const uint64_t v = nul ? 0 : col.values[slot];
      std::memcpy(rec + sizeof(Header) + 8ull * c, &v, 8);
      if (nul) h.null_mask |= 1u << c;
    }
    uint64_t begin = 0;
    bool cut = false;
    if (KeyOf(src, slot, key_cap, &begin, &h.key_len, &cut)) h.flags |= kHasKey;
    if (cut) h.flags |= kTruncated;
    for (uint32_t o = 0; o < h.key_len; ++o) rec[sizeof(Header) + 8ull * n_columns + o] = src.key_bytes[begin + o];
  }
  std::memcpy(rec, &h, sizeof(h));
}

}  // namespace documents
}  // namespace mgx

#if defined(__HIPCC__) || defined(MGX_DOCUMENTS_LAUNCHERS)
#include <hip/hip_runtime_api.h>
namespace mgx {
// One wave per entry of [0, n_entries); no launch when there is none.
int LaunchDocumentGather(const documents::DevBatch& batch, hipStream_t s);
}  // namespace mgx
#endif
