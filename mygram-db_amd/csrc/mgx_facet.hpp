// mgx_facet.hpp — FACET in a batch (mgx_batch_set_facets): the host-side plan of one batch's facet requests, the
// descriptors facet_batch_kernel reads, and the launcher of mgx_facet.hip. The planner is plain C++ and compiles without
// a HIP header (tests/cpp/facet_plan_check.cpp pins it under the sanitizers); mgx_api.cpp calls it and restates nothing.
//
//   counts arena   per (faceted query, column) a run of n_values u64, in query order then request order, runs back to back
//                  (every run starts 8-byte aligned); at most kArenaCap bytes
//   LDS bins       a workgroup counts into u32 bins in LDS and flushes its non-zero bins once. A query's columns take
//                  their n_values bins in request order while the running sum stays within kLdsBins; a column that does
//                  not fit counts straight into its run with 64-bit global atomics (a later, smaller column may still fit)
//   ballot path    in a dense round (64 documents in the 64 lanes) a column of at most `ballot_max` values is counted by
//                  one ballot + popcount per value and one add per wave and value instead of 64 lanes adding into two
//                  bins. Measured on 64 universe queries over 1M documents: 168 us against 197 us at 2 values, but 194
//                  against 158 at 4 and worse above: the threshold is 2
//   work items     one (faceted query, range of result-bitmap words) per workgroup: whole tiles, about kTargetGroups
//                  workgroups in the launch, every word of a query's row in exactly one item
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

namespace mgx {
namespace facet {

constexpr uint32_t kMaxColumns = 8;            // MGX_FACET_MAX_COLUMNS
constexpr uint64_t kArenaCap = 256ull << 20;   // MGX_FACET_ARENA_CAP
constexpr uint32_t kLdsBins = 8192;            // MGX_FACET_LDS_BINS: 32 KiB of u32 bins, four workgroups in a CU's 160 KiB
constexpr uint32_t kBlock = 256;               // four waves
constexpr uint32_t kWordsPerTile = 256;        // 64-bit words of a result-bitmap tile (mgx::kWordsPerTile)
constexpr uint32_t kTargetGroups = 8192;       // workgroups of a launch, as column_topk_kernel's (32 per CU)
constexpr uint32_t kBallotMaxValues = 2;       // columns of at most this many values take the ballot path (measured: DESIGN.md)
constexpr uint32_t kNoBins = 0xFFFFFFFFu;

// One requested column of one faceted query.
struct ColumnPlan {
  uint32_t query = 0;      // batch index of the query
  uint32_t column_id = 0;
  uint32_t n_values = 0;
  uint32_t lds_begin = kNoBins;  // first of its n_values LDS bins, or kNoBins: global atomics
  uint32_t ballot = 0;           // 1: ballot + popcount per value
  uint64_t count_off = 0;        // its run in the counts arena, in u64 elements
};

struct QueryPlan {
  uint32_t query = 0;      // batch index
  uint32_t row = 0;        // its row of the result bitmap: the query's position in the bitmap group
  uint32_t col_begin = 0, n_cols = 0;  // its columns in Plan::columns
  uint32_t lds_bins = 0;   // bins its columns hold together (<= kLdsBins)
};

// One workgroup's share: words [word_begin, word_begin + n_words) of the row of faceted query `fq`.
struct Item {
  uint32_t fq = 0;
  uint32_t word_begin = 0;
  uint32_t n_words = 0;
  uint32_t reserved = 0;
};

struct Request {
  uint32_t query = 0, row = 0;
  std::vector<uint32_t> column_ids, n_values;  // parallel
};

struct Plan {
  std::vector<QueryPlan> queries;
  std::vector<ColumnPlan> columns;
  std::vector<Item> items;
  uint64_t arena_bytes = 0;
  uint32_t tiles_per_item = 0;
};

enum Status { kOk = 0, kTooManyColumns = 1, kArenaTooLarge = 2 };

// Plans the faceted queries of one batch over an index of n_tiles tiles. On a refusal *bad names the request's position.
inline Status Build(const std::vector<Request>& requests, uint32_t n_tiles, uint32_t ballot_max, Plan* out, size_t* bad) {
  Plan p;
  uint64_t values = 0;  // u64 elements of the arena so far
  p.queries.reserve(requests.size());
  p.columns.reserve(requests.size() * 2);
  for (size_t r = 0; r < requests.size(); ++r) {
    const Request& rq = requests[r];
    if (rq.column_ids.size() > kMaxColumns) {
      if (bad) *bad = r;
      return kTooManyColumns;
    }
    QueryPlan q;
    q.query = rq.query;
    q.row = rq.row;
    q.col_begin = static_cast<uint32_t>(p.columns.size());
    q.n_cols = static_cast<uint32_t>(rq.column_ids.size());
    for (size_t c = 0; c < rq.column_ids.size(); ++c) {
      ColumnPlan col;
      col.query = rq.query;
      col.column_id = rq.column_ids[c];
      col.n_values = rq.n_values[c];
      col.count_off = values;
      values += col.n_values;
      if (values * 8 > kArenaCap) {
        if (bad) *bad = r;
        return kArenaTooLarge;
      }
      if (col.n_values != 0 && col.n_values <= kLdsBins - q.lds_bins) {
        col.lds_begin = q.lds_bins;
        q.lds_bins += col.n_values;
      }
      col.ballot = (col.n_values != 0 && col.n_values <= ballot_max) ? 1u : 0u;
      p.columns.push_back(col);
    }
    p.queries.push_back(q);
  }
  p.arena_bytes = values * 8;
  const size_t n = p.queries.size();
  if (n != 0 && n_tiles != 0) {
    const uint64_t want = (kTargetGroups + n - 1) / n;  // workgroups per query
    p.tiles_per_item = static_cast<uint32_t>((n_tiles + want - 1) / want);
    p.items.reserve(n * ((n_tiles + p.tiles_per_item - 1) / p.tiles_per_item));
    for (size_t fq = 0; fq < n; ++fq)
      for (uint32_t t = 0; t < n_tiles; t += p.tiles_per_item) {
        Item it;
        it.fq = static_cast<uint32_t>(fq);
        it.word_begin = t * kWordsPerTile;
        it.n_words = (n_tiles - t < p.tiles_per_item ? n_tiles - t : p.tiles_per_item) * kWordsPerTile;
        p.items.push_back(it);
      }
  }
  *out = std::move(p);
  return kOk;
}

// What the kernel reads (device memory).
struct DevColumn {
  const uint32_t* value_ids;   // by local doc slot; 0xFFFFFFFF = NULL
  unsigned long long* counts;  // its run in the counts arena
  uint32_t n_values;
  uint32_t lds_begin;          // or kNoBins
  uint32_t ballot;
  uint32_t reserved;
};
struct DevQuery {
  uint64_t row_word;  // the first word of its row in the result bitmaps
  uint32_t col_begin, n_cols;
  uint32_t lds_bins, reserved;
};
struct DevBatch {
  const uint64_t* rbits;
  const DevQuery* queries;
  const DevColumn* columns;
  const Item* items;
  uint32_t n_items;
  uint32_t n_docs;
};

}  // namespace facet
}  // namespace mgx

#if defined(__HIPCC__) || defined(MGX_FACET_LAUNCHERS)
#include <hip/hip_runtime_api.h>
namespace mgx {
// One workgroup per item; the counts must have been zeroed on `s`. No launch when there is no item.
int LaunchFacetBatch(const facet::DevBatch& batch, hipStream_t s);
}  // namespace mgx
#endif
