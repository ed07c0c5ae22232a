// mgx_documents.hip — page documents on the device: the primary key bytes and the requested filter-column values of every
// (requesting query, page entry) of a batch, gathered behind the kernel that finalised the page.
//
// One wave per entry, four waves per workgroup, no LDS and no barrier (waves are independent and leave early). The wave
//   1. finds its query (the last with entry_begin <= entry), reads the entry's doc id from the page and resolves it to a
//      slot of the mapped index (doc map, binary search) or of the plain index (documents::Resolve, every lane alike);
//   2. lanes [0, n_columns) each load one column's value and NULL byte of that slot and store the value into the
//      record: n_columns consecutive 8-byte words, one store instruction; a ballot of the NULL lanes is the null mask;
//   3. the lanes copy the key bytes side by side, 64 consecutive bytes per step, never past the slot's
//      [off[slot], off[slot + 1]) nor past the record's key capacity;
//   4. lane 0 stores the 16-byte header.
// A doc id that no index holds gets a zero header and reads nothing of either index. Every store is a vector store of
// one lane, inside the entry's own record (documents::RecordStride).
#include <hip/hip_runtime.h>

#include "mgx_documents.hpp"

namespace mgx {

namespace dc = documents;

constexpr int kDocWaves = 4;

__global__ __launch_bounds__(kDocWaves * 64) void document_gather_kernel(const dc::DevBatch db) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint32_t entry = blockIdx.x * kDocWaves + wave;
  if (entry >= db.n_entries || db.n_queries == 0) return;
  uint32_t lo = 0, hi = db.n_queries;
  while (hi - lo > 1) {
    const uint32_t mid = (lo + hi) >> 1;
    if (db.queries[mid].entry_begin <= entry) lo = mid;
    else hi = mid;
  }
  const dc::DevQuery q = db.queries[lo];
  const uint32_t j = entry - q.entry_begin;
  if (j >= q.limit) return;
  uint32_t count;
  if (q.page_n) {
    count = *q.page_n;
  } else if (q.total_exec) {
    const unsigned long long total = db.merged ? *q.total_merged : *q.total_exec;
    // (a doc-id page carries no offset: the compiler zeroes it, so min(total, limit) is the host's n_docs of the page. A
    // doc-id page with an offset would need the offset here too)
    count = total < q.limit ? static_cast<uint32_t>(total) : q.limit;
  } else {
    count = q.count;
  }
  if (j >= count) return;  // (the host reads the records of the page's entries only)
  const uint32_t doc = q.page_docs[j];

  uint8_t* rec = db.arena + q.rec_off + static_cast<uint64_t>(j) * q.rec_stride;
  dc::Header* g_head = reinterpret_cast<dc::Header*>(rec);
  uint64_t* g_values = reinterpret_cast<uint64_t*>(rec + sizeof(dc::Header));
  uint8_t* g_key = rec + sizeof(dc::Header) + 8ull * q.n_columns;

  uint32_t slot = 0;
  const uint32_t which = dc::Resolve(db.mapped, db.plain, doc, &slot);
  if (which == 0) {
    if (lane == 0) *g_head = dc::Header{0, 0, 0, 0};
    return;
  }
  const dc::DevSource& src = which == 1 ? db.mapped : db.plain;
  uint32_t flags = dc::kFound | (which == 1 ? dc::kMapped : 0u);

  // ---- 2. the columns: one lane each ----
  const uint32_t n_cols = q.n_columns < dc::kMaxColumns ? q.n_columns : dc::kMaxColumns;
  bool nul = false;
  if (lane < n_cols) {
    const dc::DevColumn col = src.columns[q.col_begin + lane];
    nul = !col.values || (col.is_null && col.is_null[slot] != 0);
    g_values[lane] = nul ? 0ull : col.values[slot];
  }
  const uint32_t null_mask = static_cast<uint32_t>(__ballot(nul));

  // ---- 3. the key ----
  uint64_t begin = 0;
  uint32_t key_len = 0;
  bool cut = false;
  if (dc::KeyOf(src, slot, db.key_cap, &begin, &key_len, &cut)) flags |= dc::kHasKey;
  if (cut) flags |= dc::kTruncated;
  const uint8_t* key = src.key_bytes + begin;
  for (uint32_t o = lane; o < key_len; o += 64) g_key[o] = key[o];

  // ---- 4. the header ----
  if (lane == 0) *g_head = dc::Header{flags, key_len, null_mask, n_cols};
}

int LaunchDocumentGather(const dc::DevBatch& batch, hipStream_t s) {
  if (batch.n_entries == 0 || batch.n_queries == 0) return 0;
  const uint32_t grid = (batch.n_entries + kDocWaves - 1) / kDocWaves;
  hipLaunchKernelGGL(document_gather_kernel, dim3(grid), dim3(kDocWaves * 64), 0, s, batch);
  return static_cast<int>(hipGetLastError());
}

}  // namespace mgx
