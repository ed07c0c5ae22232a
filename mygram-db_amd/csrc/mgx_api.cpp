// mgx_api.cpp — host side of libmygram_gpu.so: the C ABI of include/mygram_gpu.h.
//
// Responsibilities: device index construction (upload + skip rows + dense bitmaps), compiling queries into tile
// programs (the planning rules of search_pipeline::Execute, src/server/search_pipeline.cpp:795-869, and
// ApplyNotFilter :871-932 / ApplyFiltersWithBitmap :1196-1237 become instruction sequences), launching the kernels
// of mgx_kernels.hip, and returning results in the reference's shapes. No CPU compute path exists here: every
// operator either runs on the device or fails.
#include <hip/hip_runtime.h>

#include <dlfcn.h>
#include <pthread.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <condition_variable>
#include <map>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <tuple>
#include <unordered_map>
#include <vector>

#include "../../include/mygram_gpu.h"
#include "mgx_compile.hpp"
#include "mgx_highlight.hpp"
#include "mgx_colsort.hpp"
#include "mgx_pkey.hpp"
#include "mgx_pages.hpp"
#include "mgx_facet.hpp"
#include "mgx_documents.hpp"
#include "mgx_build.hpp"
#include "mgx_host.hpp"
#include "mgx_internal.hpp"
#include "mgx_launch.hpp"
#include "mgx_text.hpp"
#include "mygram_tools.h"

namespace mgx {

static thread_local std::string g_last_error;
void SetError(const std::string& msg) { g_last_error = msg; }
int Fail(int code, const std::string& msg) {
  g_last_error = msg;
  return code;
}

#define MGX_HIP(expr)                                                                             \
  do {                                                                                            \
    hipError_t e__ = (expr);                                                                      \
    if (e__ != hipSuccess)                                                                        \
      return ::mgx::Fail(MGX_ERR_INTERNAL, std::string(#expr) + ": " + hipGetErrorString(e__));   \
  } while (0)
#define MGX_LAUNCH(expr)                                                                                    \
  do {                                                                                                      \
    int e__ = (expr);                                                                                       \
    if (e__ != 0)                                                                                           \
      return ::mgx::Fail(MGX_ERR_INTERNAL,                                                                  \
                         std::string(#expr) + ": " + hipGetErrorString(static_cast<hipError_t>(e__)));      \
  } while (0)

// Every device allocation of the library goes through here. The test hook (include/mygram_tools.h,
// mgxt_fail_device_allocs) makes chosen allocations fail, the way the reference injects Roaring allocation failures
// (MYGRAMDB_INDEX_TEST_HOOKS, posting_list.h:217-246): the failure must surface as an error code, never as an empty
// result.
static std::atomic<int> g_fail_after{-1};  // allocations still to succeed before the injected failures; -1 = hook off
static std::atomic<int> g_fail_count{0};   // how many allocations then fail
static hipError_t DeviceMalloc(void** p, size_t n) {
  if (g_fail_after.load(std::memory_order_relaxed) >= 0) {
    if (g_fail_after.load() == 0) {
      if (g_fail_count.fetch_sub(1) > 0) {
        if (g_fail_count.load() <= 0) g_fail_after.store(-1);
        *p = nullptr;
        return hipErrorOutOfMemory;
      }
      g_fail_after.store(-1);
    } else {
      g_fail_after.fetch_sub(1);
    }
  }
  return hipMalloc(p, n);
}

// Device memory handed out in pieces that never move, optionally mirrored in pinned host memory. A batch builds all
// of its (small) input arrays in the mirror and ships them with ONE asynchronous copy per chunk on the execute stream;
// its device-only outputs come from a second arena. Chunks are kept when the arena is reset, so a serving loop that
// re-prepares a batch object (mgx_batch_reset) allocates nothing in steady state.
struct Arena {
  struct Chunk {
    char* dev = nullptr;
    char* host = nullptr;  // pinned mirror (mirrored arenas only)
    size_t cap = 0, used = 0;
  };
  std::vector<Chunk> chunks;
  bool mirrored = false;
  size_t chunk_bytes = 4u << 20;
  explicit Arena(bool m) : mirrored(m) {}
  Arena(const Arena&) = delete;
  Arena& operator=(const Arena&) = delete;
  ~Arena() {
    for (Chunk& c : chunks) {
      if (c.dev) (void)hipFree(c.dev);
      if (c.host) (void)hipHostFree(c.host);
    }
  }
  void Reset() {
    for (Chunk& c : chunks) c.used = 0;
  }
  // 256-byte aligned piece of n bytes; *mirror receives its host twin (mirrored arenas)
  hipError_t Alloc(size_t n, void** dev, void** mirror) {
    n = (std::max<size_t>(n, 16) + 255) & ~static_cast<size_t>(255);
    for (Chunk& c : chunks) {
      if (c.cap - c.used >= n) {
        *dev = c.dev + c.used;
        if (mirror) *mirror = c.host ? c.host + c.used : nullptr;
        c.used += n;
        return hipSuccess;
      }
    }
    Chunk c;
    c.cap = std::max(n, chunk_bytes);
    hipError_t e = DeviceMalloc(reinterpret_cast<void**>(&c.dev), c.cap);
    if (e != hipSuccess) return e;
    if (mirrored) {
      e = hipHostMalloc(reinterpret_cast<void**>(&c.host), c.cap, hipHostMallocDefault);
      if (e != hipSuccess) {
        (void)hipFree(c.dev);
        return e;
      }
    }
    c.used = n;
    *dev = c.dev;
    if (mirror) *mirror = c.host;
    chunks.push_back(c);
    return hipSuccess;
  }
};

// What a batch object keeps across mgx_batch_reset: its arenas, the pinned block its results are copied into, events.
struct BatchResources {
  Arena upload{true}, out{false};
  bool uploaded = false;
  void* h_down[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};  // pinned result blocks (score group, docid-page group, highlight records, facet counts, document records)
  size_t h_down_cap[5] = {0, 0, 0, 0, 0};
  hipEvent_t fork_ev = nullptr, join_ev = nullptr;  // fork/join of the side-stream launch
  // A batch object is one pipeline slot: with a NULL stream argument it runs on its own non-blocking stream, and the
  // copy of its (small) result block to pinned memory is part of the execute, fenced by done_ev — so fetching batch i
  // waits for batch i alone while batch i+1 already runs.
  hipStream_t stream = nullptr;
  hipEvent_t done_ev = nullptr;
  hipEvent_t main_ev = nullptr;  // recorded behind the score group's main launches: the next batch's main launches wait for it
  bool copy_issued = false;
  // mgx_batch_exchange: this rank's blob (docid pages only) and every rank's. They belong to the slot, not to one batch:
  // a hipFree / hipMalloc per reset would synchronise the device once per step.
  void* xchg[4] = {nullptr, nullptr, nullptr, nullptr};  // 0/1: the top-k exchange, 2/3: the seed-bound exchange
  size_t xchg_cap[4] = {0, 0, 0, 0};
  hipError_t Exchange(int which, size_t bytes, void** out_ptr) {
    if (xchg_cap[which] < bytes) {
      if (xchg[which]) (void)hipFree(xchg[which]);
      xchg[which] = nullptr;
      xchg_cap[which] = 0;
      const size_t cap = bytes + bytes / 4;
      hipError_t e = DeviceMalloc(&xchg[which], cap);
      if (e != hipSuccess) return e;
      xchg_cap[which] = cap;
    }
    *out_ptr = xchg[which];
    return hipSuccess;
  }
  // The rows the batch's own FILTER conditions are evaluated into (mgx_query.conditions): grown when a batch needs more
  // rows than any before it, never shrunk, kept across mgx_batch_reset like the arenas.
  void* cond = nullptr;
  size_t cond_cap = 0;
  hipError_t Conditions(size_t bytes, void** out_ptr) {
    if (cond_cap < bytes) {
      if (cond) (void)hipFree(cond);
      cond = nullptr;
      cond_cap = 0;
      hipError_t e = DeviceMalloc(&cond, bytes);
      if (e != hipSuccess) return e;
      cond_cap = bytes;
    }
    *out_ptr = cond;
    return hipSuccess;
  }
  ~BatchResources() {
    if (cond) (void)hipFree(cond);
    for (void* x : xchg)
      if (x) (void)hipFree(x);
    if (stream) (void)hipStreamDestroy(stream);
    if (done_ev) (void)hipEventDestroy(done_ev);
    if (main_ev) (void)hipEventDestroy(main_ev);
    for (void* h : h_down)
      if (h) (void)hipHostFree(h);
    if (fork_ev) (void)hipEventDestroy(fork_ev);
    if (join_ev) (void)hipEventDestroy(join_ev);
  }
  hipError_t Pinned(int which, size_t bytes, void** out_ptr) {
    if (h_down_cap[which] < bytes) {
      if (h_down[which]) (void)hipHostFree(h_down[which]);
      h_down[which] = nullptr;
      h_down_cap[which] = 0;
      const size_t cap = std::max<size_t>(bytes + bytes / 2, 1u << 16);
      hipError_t e = hipHostMalloc(&h_down[which], cap, hipHostMallocDefault);
      if (e != hipSuccess) return e;
      h_down_cap[which] = cap;
    }
    *out_ptr = h_down[which];
    return hipSuccess;
  }
  void Reset() {
    upload.Reset();
    out.Reset();
    uploaded = false;
    copy_issued = false;
  }
};
// The resources DevBuf::Alloc / Upload draw from while a batch is being prepared on this thread (null: own hipMalloc).
static thread_local BatchResources* tl_res = nullptr;
struct ResourceScope {
  BatchResources* prev;
  explicit ResourceScope(BatchResources* r) : prev(tl_res) { tl_res = r; }
  ~ResourceScope() { tl_res = prev; }
};

// Device buffer: owns its memory (hipMalloc), or is a piece of the current batch's arena.
struct DevBuf {
  void* p = nullptr;
  size_t bytes = 0;
  bool owned = true;
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  DevBuf(DevBuf&& o) noexcept : p(o.p), bytes(o.bytes), owned(o.owned) { o.p = nullptr; o.bytes = 0; }
  DevBuf& operator=(DevBuf&& o) noexcept {
    if (this != &o) {
      Free();
      p = o.p;
      bytes = o.bytes;
      owned = o.owned;
      o.p = nullptr;
      o.bytes = 0;
    }
    return *this;
  }
  ~DevBuf() { Free(); }
  void Free() {
    if (p && owned) (void)hipFree(p);
    p = nullptr;
    bytes = 0;
    owned = true;
  }
  hipError_t Alloc(size_t n) {
    Free();
    bytes = n;
    if (tl_res) {
      owned = false;
      return tl_res->out.Alloc(n, &p, nullptr);
    }
    return DeviceMalloc(&p, n ? n : 16);
  }
  template <typename T>
  T* as() const { return static_cast<T*>(p); }
};

template <typename T>
static hipError_t Upload(DevBuf& b, const T* host, size_t count, size_t pad_count = 0) {
  if (tl_res) {  // into the batch's upload arena: shipped by the first execute
    b.Free();
    b.bytes = (count + pad_count) * sizeof(T);
    b.owned = false;
    void* mirror = nullptr;
    hipError_t e = tl_res->upload.Alloc(b.bytes, &b.p, &mirror);
    if (e != hipSuccess) return e;
    if (count) std::memcpy(mirror, host, count * sizeof(T));
    if (pad_count) std::memset(static_cast<char*>(mirror) + count * sizeof(T), 0xFF, pad_count * sizeof(T));
    return hipSuccess;
  }
  hipError_t e = b.Alloc((count + pad_count) * sizeof(T));
  if (e != hipSuccess) return e;
  if (pad_count) {
    e = hipMemset(static_cast<char*>(b.p) + count * sizeof(T), 0xFF, pad_count * sizeof(T));
    if (e != hipSuccess) return e;
  }
  if (count) e = hipMemcpy(b.p, host, count * sizeof(T), hipMemcpyHostToDevice);
  return e;
}

}  // namespace mgx

using mgx::DevBuf;

// =================================================================================================================
// index
// =================================================================================================================

struct mgx_index {
  int device = 0;
  hipStream_t stream = nullptr;
  hipStream_t side_stream = nullptr;  // the few queries the wave kernel cannot take run here, beside the main launch
  std::mutex mu;  // filter registration (rows / columns of the filter pool), text attachment
  // The single-operator entry points (Index::SearchAnd & co. through the shim: what an UNMODIFIED call site uses, from
  // every worker thread of the server at once, command_handler.cpp:66) each lease one of these for the call: its own
  // arenas, pinned block and stream — no lock is held while the operator runs, nothing is allocated in steady state.
  std::mutex pool_mu;
  std::vector<std::unique_ptr<mgx::BatchResources>> single_pool;  // free ones
  mgx::DevIndex dev{};
  DevBuf d_offsets, d_docids, d_tf, d_doc_len, d_skip_row, d_tile_off, d_gram_bitmaps, d_filter_bitmaps;
  DevBuf d_text, d_text_off;  // mgx_index_attach_text
  uint32_t max_text_bytes = 0;  // the longest attached text (sizes the highlight records)
  // mgx_index_attach_original_text: the texts as the user wrote them, their kinds and the mapped documents' maps
  DevBuf d_orig, d_orig_off, d_orig_kind, d_orig_map, d_orig_map_off;
  mgx::highlight::DevOriginals originals{};  // all null without them
  uint32_t max_original_bytes = 0;
  DevBuf d_dl8, d_tfnib, d_tf_ovf_pos, d_tf_ovf_val;
  DevBuf d_dev_index;  // `dev` in device memory: what out-of-line device functions take a pointer to (SyncDevIndex)
  std::vector<uint64_t> h_offsets;
  std::vector<uint32_t> h_skip_row;  // per gram
  std::vector<uint32_t> h_bm_row;    // per gram
  uint32_t n_filter_rows = 0, filter_cap_rows = 0;
  struct FilterColumn {  // mgx_index_add_filter_column
    uint32_t value_class = 0, n_values = 0;
    mgx::colsort::KeyScan sort_keys;  // has a NULL / has a non-NULL value whose sort key is 0 too (mgx_colsort.hpp): a
                                      // column, or the two columns of a table with a delta, with both is not sortable
    DevBuf d_values, d_null, d_value_ids;
  };
  std::vector<std::unique_ptr<FilterColumn>> filter_columns;
  std::atomic<uint32_t> n_filter_columns{0};  // = filter_columns.size(), for readers that hold no lock (CompileQuery)
  std::vector<DevBuf> retired_filter_pools;
  uint64_t n_grams = 0;
  bool can_score = false;
  uint64_t words_per_row = 0;  // n_tiles * 256
  uint64_t filter_row_stride = 0;  // words; words_per_row + padding
  // BM25 contribution tables of the fast scoring path: idf*tf*(k1+1)/(tf + k1*(1-b+b*dl/avgdl)) for tf 0..14 and every
  // doc length below table_dl, one table per (dense gram, idf, k1, b, avgdl). These are table constants (idf comes from
  // the gram's posting count and N), so they are built once on first use and a query carries their addresses.
  struct TableKey {
    uint32_t row;
    uint64_t idf, k1, b, avg;
    bool operator==(const TableKey& o) const { return row == o.row && idf == o.idf && k1 == o.k1 && b == o.b && avg == o.avg; }
  };
  struct TableKeyHash {
    size_t operator()(const TableKey& k) const {
      uint64_t h = k.row * 0x9E3779B97F4A7C15ull;
      for (uint64_t v : {k.idf, k.k1, k.b, k.avg}) h = (h ^ v) * 0xFF51AFD7ED558CCDull + (h >> 29);
      return static_cast<size_t>(h);
    }
  };
  std::mutex table_mu;
  std::unordered_map<TableKey, uint32_t, TableKeyHash> table_slot;
  DevBuf d_table_pool;
  uint32_t table_cap = 0, table_used = 0, table_dl = 0;
  // New tables are built ON THE DEVICE (build_contrib_tables_kernel) on the index's table stream: the compile step of a
  // batch only reserves the slot and queues a 40-byte job (a fresh serving process meets new (gram, idf) pairs in almost
  // every batch until its working set exists; 3840 divisions + a blocking 30 KB copy per table were most of those
  // batches' compile time). The next execute ships the queued jobs through a pinned ring, launches the build and waits
  // for table_ev on its own stream — a no-op once the tables are there.
  hipStream_t table_stream = nullptr;
  hipEvent_t table_ev = nullptr;
  mgx::TableJob* job_ring = nullptr;  // pinned, kJobRing jobs; the device twin holds the same offsets
  DevBuf d_job_ring;
  uint32_t job_ring_at = 0;
  std::vector<mgx::TableJob> pending_jobs;  // under table_mu
  // Batches of a serving loop run on their own streams, and the device would time-slice the main kernels of all batches
  // in flight: every batch then finishes after (batches in flight) x (kernel time). The main launches of a batch
  // therefore wait for the main launches of the batch enqueued before it on this index (chain_ev: that batch's
  // BatchResources::main_ev) — first in, first out; uploads, clears, the merge and the result copy still overlap the
  // previous batch's kernels. Guarded by table_mu.
  hipEvent_t chain_ev = nullptr;
  std::atomic<int> fifo{1};  // mgx_index_set_batch_order
  bool table_ev_recorded = false;
  static constexpr uint32_t kJobRing = 4096;
  size_t table_doubles() const { return static_cast<size_t>(mgx::kFastPoolTf + 1) * table_dl; }
  // K[dl] = k1 * (1 - b + b * dl / avgdl), dl 0..255, per (k1, b, avgdl) of a batch (group_score_kernel)
  struct NormTable {
    uint64_t k1, b, avg;
    DevBuf d;
  };
  std::vector<std::unique_ptr<NormTable>> norm_tables;
  // block-max bytes of the dense grams' BM25 term factor per (k1, b, avgdl) (build_blockmax_kernel): top-k pruning
  struct BlockMax {
    uint64_t k1, b, avg;
    double step;
    DevBuf d, d_fine;
  };
  std::vector<std::unique_ptr<BlockMax>> block_max;
  // df of text-level terms seen so far: (term bytes, N) -> THIS SHARD's count (a shard of a table sums the ranks' counts
  // per batch, mgx_batch_exchange_df). The index is static, so the count never changes: the df pass (a text scan over
  // every candidate of the term) runs once per distinct term, not once per batch.
  std::unordered_map<std::string, uint64_t> df_cache;
  uint32_t n_bitmap_rows = 0, n_fine_rows = 0;
  // Mutable tables (mgx_index_set_live_bitmap): the filter row every batched query is ANDed with right after its first
  // term — the documents of this index that are still live (removed / superseded ones cleared) — or kNoRow.
  std::atomic<uint32_t> live_row{mgx::kNoRow};
  // the bitmap form of every dense gram excludes the dead documents too (mgx_index_clear_postings was called for each of
  // them): a term whose grams are all bitmap-form is live by construction and takes no live-row operand
  std::atomic<bool> bitmaps_clean{false};
  DevBuf d_doc_map;  // mgx_index_set_doc_map: local slot -> table doc id (a delta index), or empty
  std::vector<uint32_t> h_doc_map;  // the same on the host: the key of a document without a primary key is its table id
  // mgx_index_set_primary_keys (MGX_SORT_PRIMARY_KEY, mgx_pkey.hpp): one value per doc slot and, for kKeyRanks, the
  // dictionary of the index's distinct keys. Without it (has_pkeys false) every document's key is its table doc id:
  // kind numeric, no column. Guarded by mu; the atomics are what ViewOf reads without it.
  bool has_pkeys = false;
  uint32_t pk_kind = mgx::pkey::kKeyNumeric;
  bool pk_any_missing = false;
  DevBuf d_pk_values, d_pk_off, d_pk_bytes;
  // mgx_index_attach_primary_key_bytes (page documents, mgx_documents.hpp): the raw key bytes by doc slot. Guarded by mu.
  DevBuf d_pkb_bytes, d_pkb_off, d_pkb_has;
  bool has_pk_bytes = false;
  uint32_t max_pk_bytes = 0;  // the longest attached key (sizes the document records)
  std::atomic<bool> pk_monotone{true};  // the keys never decrease with the slot (true without keys: doc ids ascend)
  std::atomic<bool> pk_shortcut{true};  // mgx_index_set_primary_key_shortcut
  std::atomic<bool> has_doc_map{false};  // d_doc_map is set (a delta index: its keys are never in doc-id order of a table)
  DevBuf d_fine_rows;                 // fine row -> bitmap row
  std::vector<uint32_t> h_fine_map;   // bitmap row -> fine row (kNoRow: none)
};

namespace mgx {
// RCCL's by-value types, restated (rccl.h:40-41, :259-270) so that the library needs no RCCL header to build
struct RcclId {
  char internal[128];
};
constexpr int kRcclUint8 = 1, kRcclUint64 = 5, kRcclSum = 0;
static inline uint64_t Bits(double d) {
  uint64_t u;
  std::memcpy(&u, &d, 8);
  return u;
}

// Keeps the device-memory copy of idx->dev current (after creation and whenever a pointer inside it changes).
static hipError_t SyncDevIndex(mgx_index* idx) {
  if (!idx->d_dev_index.p) {
    ResourceScope none(nullptr);
    hipError_t e = idx->d_dev_index.Alloc(sizeof(DevIndex));
    if (e != hipSuccess) return e;
  }
  return hipMemcpy(idx->d_dev_index.p, &idx->dev, sizeof(DevIndex), hipMemcpyHostToDevice);
}

// Device address of the contribution table of (dense gram row, idf, k1, b, avgdl); built and uploaded on first use.
// 0 when the pool is exhausted (the query then runs on the general path).
static uint64_t GetContributionTable(mgx_index* idx, uint32_t bm_row, double idf, double k1, double b, double avgdl) {
  if (idx->table_cap == 0) return 0;
  const mgx_index::TableKey key{bm_row, Bits(idf), Bits(k1), Bits(b), Bits(avgdl)};
  std::lock_guard<std::mutex> lock(idx->table_mu);
  const auto hit = idx->table_slot.find(key);
  const size_t nd = idx->table_doubles();
  if (hit != idx->table_slot.end())
    return reinterpret_cast<uint64_t>(idx->d_table_pool.as<double>() + static_cast<size_t>(hit->second) * nd);
  if (idx->table_used == idx->table_cap) return 0;
  const uint32_t slot = idx->table_used;
  double* dst = idx->d_table_pool.as<double>() + static_cast<size_t>(slot) * nd;
  idx->pending_jobs.push_back(TableJob{idf, k1, b, avgdl, slot, 0});  // built by the next execute (FlushTableJobs)
  idx->table_used++;
  idx->table_slot.emplace(key, slot);
  return reinterpret_cast<uint64_t>(dst);
}

// Ships the queued table jobs and launches their build on the table stream; the caller then waits for table_ev on its
// own stream. Called with table_mu held.
static hipError_t FlushTableJobs(mgx_index* idx) {
  if (idx->pending_jobs.empty()) return hipSuccess;
  hipError_t e;
  if (!idx->job_ring) {
    ResourceScope none(nullptr);
    if ((e = hipHostMalloc(reinterpret_cast<void**>(&idx->job_ring), mgx_index::kJobRing * sizeof(TableJob),
                           hipHostMallocDefault)) != hipSuccess ||
        (e = idx->d_job_ring.Alloc(mgx_index::kJobRing * sizeof(TableJob))) != hipSuccess ||
        (e = hipStreamCreateWithFlags(&idx->table_stream, hipStreamNonBlocking)) != hipSuccess ||
        (e = hipEventCreateWithFlags(&idx->table_ev, hipEventDisableTiming)) != hipSuccess)
      return e;
  }
  size_t done = 0;
  while (done < idx->pending_jobs.size()) {
    const uint32_t n = static_cast<uint32_t>(std::min<size_t>(idx->pending_jobs.size() - done, mgx_index::kJobRing));
    if (idx->job_ring_at + n > mgx_index::kJobRing) {  // wrap: the ring's earlier copies must have left
      if ((e = hipStreamSynchronize(idx->table_stream)) != hipSuccess) return e;
      idx->job_ring_at = 0;
    }
    TableJob* stage = idx->job_ring + idx->job_ring_at;
    TableJob* dev = idx->d_job_ring.as<TableJob>() + idx->job_ring_at;
    std::memcpy(stage, idx->pending_jobs.data() + done, n * sizeof(TableJob));
    if ((e = hipMemcpyAsync(dev, stage, n * sizeof(TableJob), hipMemcpyHostToDevice, idx->table_stream)) != hipSuccess) return e;
    const int le = LaunchBuildContribTables(dev, n, idx->table_dl, idx->d_table_pool.as<double>(), idx->table_stream);
    if (le != 0) return static_cast<hipError_t>(le);
    idx->job_ring_at += n;
    done += n;
  }
  idx->pending_jobs.clear();
  if ((e = hipEventRecord(idx->table_ev, idx->table_stream)) != hipSuccess) return e;
  idx->table_ev_recorded = true;
  return hipSuccess;
}

// Device address of K[0..255], K[dl] = k1 * ((1 - b) + b * dl / max(avgdl, 1)): the doc-length half of the BM25
// denominator (bm25_scorer.cpp:80-84), evaluated on the host operation by operation so that tf + K[dl] is the
// reference's denominator bit for bit. nullptr when it cannot be built (the queries then take the table-based path).
static const double* GetLengthNormTable(mgx_index* idx, double k1, double b, double avgdl) {
  std::lock_guard<std::mutex> lock(idx->table_mu);
  for (const auto& t : idx->norm_tables)
    if (t->k1 == Bits(k1) && t->b == Bits(b) && t->avg == Bits(avgdl)) return t->d.as<double>();
  if (idx->norm_tables.size() >= 64) return nullptr;
  double h[256];
  const double one_minus_b = 1.0 - b, avg = std::max(avgdl, 1.0);
  for (uint32_t dli = 0; dli < 256; ++dli) {
    const double length_norm = one_minus_b + b * static_cast<double>(dli) / avg;
    h[dli] = k1 * length_norm;
  }
  auto t = std::make_unique<mgx_index::NormTable>();
  t->k1 = Bits(k1);
  t->b = Bits(b);
  t->avg = Bits(avgdl);
  ResourceScope none(nullptr);  // index-owned memory, not a batch arena
  if (hipSetDevice(idx->device) != hipSuccess || t->d.Alloc(sizeof(h)) != hipSuccess ||
      hipMemcpy(t->d.p, h, sizeof(h), hipMemcpyHostToDevice) != hipSuccess) {
    (void)hipGetLastError();
    return nullptr;
  }
  idx->norm_tables.push_back(std::move(t));
  return idx->norm_tables.back()->d.as<double>();
}

// Block-max bytes of the index for (k1, b, avgdl), built on first use (one pass over the tf-nibble rows and doc
// lengths: a few ms, ~9 bytes per 64 docs per dense gram... 1 byte per word per row). nullptr when pruning is off for
// these parameters (it needs k1 > 0 and 0 <= b <= 1: the term factor must grow with tf and shrink with dl), when the
// index has no tf columns, or when the few parameter sets an index keeps are taken.
static const uint8_t* GetBlockMax(mgx_index* idx, double k1, double b, double avgdl, double* step, const uint8_t** fine) {
  *fine = nullptr;
  static const bool off = std::getenv("MGX_NO_PRUNE") != nullptr && atoi(std::getenv("MGX_NO_PRUNE")) != 0;
  if (off || !idx->can_score || idx->n_bitmap_rows == 0 || !(k1 > 0.0) || !(b >= 0.0 && b <= 1.0) || !(avgdl >= 0.0))
    return nullptr;
  {
    std::lock_guard<std::mutex> lock(idx->table_mu);
    for (const auto& t : idx->block_max)
      if (t->k1 == Bits(k1) && t->b == Bits(b) && t->avg == Bits(avgdl)) {
        *step = t->step;
        *fine = t->d_fine.as<uint8_t>();
        return t->d.as<uint8_t>();
      }
    if (idx->block_max.size() >= 4) return nullptr;
  }
  const double* ktab = GetLengthNormTable(idx, k1, b, avgdl);
  if (!ktab) return nullptr;
  std::lock_guard<std::mutex> lock(idx->table_mu);
  for (const auto& t : idx->block_max)  // (another planner thread may have built it meanwhile)
    if (t->k1 == Bits(k1) && t->b == Bits(b) && t->avg == Bits(avgdl)) {
      *step = t->step;
      *fine = t->d_fine.as<uint8_t>();
      return t->d.as<uint8_t>();
    }
  auto t = std::make_unique<mgx_index::BlockMax>();
  t->k1 = Bits(k1);
  t->b = Bits(b);
  t->avg = Bits(avgdl);
  t->step = (k1 + 1.0) / 253.0;  // the supremum k1 + 1 lands on 254 (build_blockmax_kernel: floor + 1)
  ResourceScope none(nullptr);
  const size_t bytes = static_cast<size_t>(idx->dev.n_tiles) * idx->n_bitmap_rows * 256u;
  if (hipSetDevice(idx->device) != hipSuccess || t->d.Alloc(bytes) != hipSuccess) {
    (void)hipGetLastError();
    return nullptr;
  }
  const size_t fine_bytes = static_cast<size_t>(idx->dev.n_tiles) * idx->n_fine_rows * 1024u;
  if (fine_bytes && t->d_fine.Alloc(fine_bytes) != hipSuccess) {
    (void)hipGetLastError();
    return nullptr;
  }
  if (LaunchBuildBlockMax(idx->dev.tfnib, idx->dev.nib_row_stride, idx->dev.dl8, ktab, k1 + 1.0, 1.0 / t->step, nullptr,
                          idx->n_bitmap_rows, idx->dev.n_tiles, false, t->d.p, idx->stream) != 0 ||
      LaunchBuildBlockMax(idx->dev.tfnib, idx->dev.nib_row_stride, idx->dev.dl8, ktab, k1 + 1.0, 1.0 / t->step,
                          idx->d_fine_rows.as<uint32_t>(), idx->n_fine_rows, idx->dev.n_tiles, true, t->d_fine.p,
                          idx->stream) != 0 ||
      hipStreamSynchronize(idx->stream) != hipSuccess) {
    (void)hipGetLastError();
    return nullptr;
  }
  *step = t->step;
  *fine = t->d_fine.as<uint8_t>();
  idx->block_max.push_back(std::move(t));
  return idx->block_max.back()->d.as<uint8_t>();
}
}  // namespace mgx


extern "C" {

int mgx_abi_version(void) { return MGX_ABI_VERSION; }
const char* mgx_last_error(void) { return mgx::g_last_error.c_str(); }
void mgx_free(void* p) { std::free(p); }

int mgx_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) {
    (void)hipGetLastError();
    return 0;
  }
  return n;
}

// ---- columns ----------------------------------------------------------------------------------------------------

int mgx_columns_build(const mgx_build_params* params, const uint8_t* text_bytes, const uint64_t* text_off,
                      uint32_t first_doc_id, uint64_t n_docs, mgx_columns** out) {
  if (out) *out = nullptr;
  if (!params || !out || !text_off || (n_docs && !text_bytes && text_off[n_docs] != 0))
    return mgx::Fail(MGX_ERR_INVALID_ARGUMENT, "mgx_columns_build: null argument");
  if (params->struct_size < sizeof(mgx_build_params) || params->version != MGX_ABI_VERSION)
    return mgx::Fail(MGX_ERR_INVALID_ARGUMENT, "mgx_columns_build: bad struct_size/version");
  if (static_cast<uint64_t>(first_doc_id) + n_docs > 0xFFFFFFFFull)
    return mgx::Fail(MGX_ERR_OUT_OF_RANGE, "mgx_columns_build: doc ids exceed uint32");
  try {
    mgx::Columns* c = nullptr;
    std::string err;
    int rc = mgx::BuildColumns(*params, text_bytes, text_off, first_doc_id, n_docs, &c, &err);
    if (rc != MGX_OK) return mgx::Fail(rc, err);
    *out = reinterpret_cast<mgx_columns*>(c);
    return MGX_OK;
  } catch (const std::exception& e) {
    return mgx::Fail(MGX_ERR_INTERNAL, std::string("mgx_columns_build: ") + e.what());
  }
}

int mgx_columns_build_device(const mgx_build_params* params, const uint8_t* text_bytes, const uint64_t* text_off,
                             uint32_t first_doc_id, uint64_t n_docs, int device, mgx_columns** out) {
  if (out) *out = nullptr;
  // ---- host-only checks first: they answer without a device ---------------------------------------------------------------
  if (!params || !out || !text_off || (n_docs && !text_bytes && text_off[n_docs] != text_off[0]))
    return mgx::Fail(MGX_ERR_INVALID_ARGUMENT, "mgx_columns_build_device: null argument");
  if (params->struct_size < sizeof(mgx_build_params) || params->version != MGX_ABI_VERSION)
    return mgx::Fail(MGX_ERR_INVALID_ARGUMENT, "mgx_columns_build_device: bad struct_size/version");
  if (static_cast<uint64_t>(first_doc_id) + n_docs > 0xFFFFFFFFull)
    return mgx::Fail(MGX_ERR_OUT_OF_RANGE, "mgx_columns_build_device: doc ids exceed uint32");
  const int kanji_n = params->kanji_ngram_size > 0 ? params->kanji_ngram_size : params->ngram_size;
  if (params->ngram_size > mgx::build::kMaxGram || kanji_n > mgx::build::kMaxGram)
    return mgx::Fail(MGX_ERR_NOT_IMPLEMENTED,
                     "mgx_columns_build_device: n-grams of more than 3 code points are not built on the device (a gram is "
                     "packed into 64 bits); use mgx_columns_build");
  for (uint64_t d = 0; d < n_docs; ++d)
    if (text_off[d + 1] < text_off[d])
      return mgx::Fail(MGX_ERR_INVALID_ARGUMENT, "mgx_columns_build_device: text_off descends");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
    (void)hipGetLastError();
    return mgx::Fail(MGX_ERR_INTERNAL, "no HIP device available: libmygram_gpu has no CPU fallback");
  }
  if (device < 0 || device >= ndev) return mgx::Fail(MGX_ERR_INVALID_ARGUMENT, "mgx_columns_build_device: bad device");
  if (text_off[n_docs] - text_off[0] > mgx::build::kMaxTextBytes)
    return mgx::Fail(MGX_ERR_OUT_OF_RANGE, "mgx_columns_build_device: " + std::to_string(text_off[n_docs] - text_off[0]) +
                                               " bytes of text, the device builder takes " +
                                               std::to_string(mgx::build::kMaxTextBytes) + "; use mgx_columns_build");
  try {
    mgx::build::PackedColumns packed;
    std::string err;
    const int rc = mgx::build::BuildOnDevice(*params, text_bytes, text_off, first_doc_id, n_docs, device, &packed, &err);
    if (rc != MGX_OK) return mgx::Fail(rc, err);
    *out = reinterpret_cast<mgx_columns*>(mgx::ColumnsFromPacked(*params, text_off, first_doc_id, n_docs, std::move(packed)));
    return MGX_OK;
  } catch (const std::exception& e) {
    return mgx::Fail(MGX_ERR_INTERNAL, std::string("mgx_columns_build_device: ") + e.what());
  }
}

int mgx_columns_from_mgix(const uint8_t* data, uint64_t len, uint32_t first_doc_id, uint64_t n_docs, mgx_columns** out,
                          mgx_mgix_info* info) {
  if (out) *out = nullptr;
  if (!data || !out) return mgx::Fail(MGX_ERR_INVALID_ARGUMENT, "mgx_columns_from_mgix: null argument");
  if (static_cast<uint64_t>(first_doc_id) + n_docs > 0xFFFFFFFFull)
    return mgx::Fail(MGX_ERR_OUT_OF_RANGE, "mgx_columns_from_mgix: doc ids exceed uint32");
  try {
    mgx::Columns* c = nullptr;
    std::string err;
    const int rc = mgx::ColumnsFromMgix(data, len, first_doc_id, n_docs, &c, info, &err);
    if (rc != MGX_OK) return mgx::Fail(rc, err);
    *out = reinterpret_cast<mgx_columns*>(c);
    return MGX_OK;
  } catch (const std::exception& e) {
    return mgx::Fail(MGX_ERR_INTERNAL, std::string("mgx_columns_from_mgix: ") + e.what());
  }
}

int mgx_dump_open(const uint8_t* data, uint64_t len, const char* table, mgx_dump** out) {
  if (out) *out = nullptr;
  if (!data || !out) return mgx::Fail(MGX_ERR_INVALID_ARGUMENT, "mgx_dump_open: null argument");
  try {
    mgx::DumpData* d = nullptr;
    std::string err;
    const int rc = mgx::DumpOpen(data, len, table, &d, &err);
    if (rc != MGX_OK) return mgx::Fail(rc, err);
    *out = reinterpret_cast<mgx_dump*>(d);
    return MGX_OK;
  } catch (const std::exception& e) {
    return mgx::Fail(MGX_ERR_INTERNAL, std::string("mgx_dump_open: ") + e.what());
  }
}
int mgx_dump_view_get(const mgx_dump* dump, mgx_dump_view* out) {
  if (!dump || !out) return mgx::Fail(MGX_ERR_INVALID_ARGUMENT, "mgx_dump_view_get: null argument");
  mgx::DumpView(reinterpret_cast<const mgx::DumpData*>(dump), out);
  return MGX_OK;
}
int mgx_dump_filter_column_get(const mgx_dump* dump, uint32_t i, mgx_dump_filter_column* out) {
  if (!dump || !out) return mgx::Fail(MGX_ERR_INVALID_ARGUMENT, "mgx_dump_filter_column_get: null argument");
  if (!mgx::DumpFilterColumn(reinterpret_cast<const mgx::DumpData*>(dump), i, out))
    return mgx::Fail(MGX_ERR_OUT_OF_RANGE, "mgx_dump_filter_column_get: no such column");
  return MGX_OK;
}
int mgx_dump_primary_keys_get(const mgx_dump* dump, const uint8_t** bytes, const uint64_t** off) {
  if (!dump || !bytes || !off) return mgx::Fail(MGX_ERR_INVALID_ARGUMENT, "mgx_dump_primary_keys_get: null argument");
  mgx::DumpPrimaryKeys(reinterpret_cast<const mgx::DumpData*>(dump), bytes, off);
  return MGX_OK;
}
int mgx_dump_original_texts_get(const mgx_dump* dump, const uint8_t** bytes, const uint64_t** off) {
  if (!dump || !bytes || !off) return mgx::Fail(MGX_ERR_INVALID_ARGUMENT, "mgx_dump_original_texts_get: null argument");
  mgx::DumpOriginalTexts(reinterpret_cast<const mgx::DumpData*>(dump), bytes, off);
  return MGX_OK;
}
int mgx_dump_take_columns(mgx_dump* dump, mgx_columns** out) {
  if (out) *out = nullptr;
  if (!dump || !out) return mgx::Fail(MGX_ERR_INVALID_ARGUMENT, "mgx_dump_take_columns: null argument");
  *out = reinterpret_cast<mgx_columns*>(mgx::DumpTakeColumns(reinterpret_cast<mgx::DumpData*>(dump)));
  return MGX_OK;
}
void mgx_dump_destroy(mgx_dump* dump) { mgx::DumpDestroy(reinterpret_cast<mgx::DumpData*>(dump)); }

int mgx_columns_view_get(const mgx_columns* cols, mgx_columns_view* out) {
  if (!cols || !out) return mgx::Fail(MGX_ERR_INVALID_ARGUMENT, "mgx_columns_view_get: null argument");
  mgx::ColumnsView(reinterpret_cast<const mgx::Columns*>(cols), out);
  return MGX_OK;
}

int mgx_columns_lookup(const mgx_columns* cols, const uint8_t* gram, size_t len, uint32_t* gram_id, int* found) {
  if (gram_id) *gram_id = 0;
  if (found) *found = 0;
  if (!cols || !gram_id || !found || (!gram && len))
    return mgx::Fail(MGX_ERR_INVALID_ARGUMENT, "mgx_columns_lookup: null argument");
  uint32_t id = 0;
  if (mgx::ColumnsLookup(reinterpret_cast<const mgx::Columns*>(cols), gram, len, &id)) {
    *gram_id = id;
    *found = 1;
  }
  return MGX_OK;
}

void mgx_columns_destroy(mgx_columns* cols) { mgx::DestroyColumns(reinterpret_cast<mgx::Columns*>(cols)); }

// ---- index ------------------------------------------------------------------------------------------------------

// An index is made in two parts. The first brings the postings to the device: IndexCreateImpl takes them from the caller
// (validate, then upload), mgx_index_build_device adopts the arrays the device builder left there. The second,
// IndexDeriveRest, is shared: everything else comes from the resident columns and the host's copy of `offsets`.
static int IndexOpenStreams(mgx_index* idx);
static int IndexDeriveRest(mgx_index* idx, uint32_t first_doc_id, uint64_t n_docs, double dense_threshold,
                           uint64_t n_tf_overflow, uint32_t max_doc_len);

static int IndexCreateImpl(const mgx_index_desc* d, mgx_index** out) {
  auto idx = std::make_unique<mgx_index>();
  idx->device = d->device;
  const uint64_t G = d->n_grams;
  const uint64_t P = G ? d->offsets[G] : 0;
  const uint64_t n_docs = d->n_docs;
  if (n_docs == 0 || n_docs > 0xFFFFFFFFull || static_cast<uint64_t>(d->first_doc_id) + n_docs > 0x100000000ull)
    return mgx::Fail(MGX_ERR_OUT_OF_RANGE, "mgx_index_create: n_docs must be in [1, 2^32) and ids fit uint32");
  // The contract of the descriptor is checked, not assumed: the build kernels turn every doc id into a bit / nibble
  // address without a bounds guard, so one id outside the owned range (a shard given the wrong first_doc_id) would be
  // an out-of-bounds device write. One host pass over the postings (threads over gram ranges).
  {
    for (uint64_t g = 0; g < G; ++g)
      if (d->offsets[g + 1] < d->offsets[g])
        return mgx::Fail(MGX_ERR_INVALID_ARGUMENT, "mgx_index_create: offsets must be non-decreasing");
    const uint64_t lo_id = d->first_doc_id, hi_id = lo_id + n_docs;  // [lo_id, hi_id)
    const unsigned hw = std::max(1u, std::min(16u, std::thread::hardware_concurrency()));
    const unsigned n_thr = P < (1u << 22) ? 1u : hw;
    std::vector<int> bad(n_thr, 0);
    auto check = [&](unsigned t) {
      // thread t takes the grams whose postings start in its share of [0, P)
      const uint64_t p_lo = P * t / n_thr, p_hi = P * (t + 1) / n_thr;
      uint64_t g = static_cast<uint64_t>(std::lower_bound(d->offsets, d->offsets + G, p_lo) - d->offsets);
      for (; g < G && d->offsets[g] < p_hi; ++g) {
        const uint64_t a = d->offsets[g], b = d->offsets[g + 1];
        uint64_t prev = 0;
        for (uint64_t p = a; p < b; ++p) {
          const uint64_t id = d->docids[p];
          if (id < lo_id || id >= hi_id) bad[t] = MGX_ERR_OUT_OF_RANGE;
          else if (p > a && id <= prev) bad[t] = bad[t] ? bad[t] : MGX_ERR_INVALID_ARGUMENT;
          prev = id;
        }
      }
    };
    if (n_thr == 1) {
      check(0);
    } else {
      std::vector<std::thread> pool;
      for (unsigned t = 0; t < n_thr; ++t) pool.emplace_back(check, t);
      for (auto& th : pool) th.join();
    }
    for (int b : bad) {
      if (b == MGX_ERR_OUT_OF_RANGE)
        return mgx::Fail(b, "mgx_index_create: a doc id lies outside [first_doc_id, first_doc_id + n_docs)");
      if (b) return mgx::Fail(b, "mgx_index_create: doc ids must ascend strictly inside every posting list");
    }
  }
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
    (void)hipGetLastError();
    return mgx::Fail(MGX_ERR_INTERNAL, "no HIP device available: libmygram_gpu has no CPU fallback");
  }
  if (d->device < 0 || d->device >= ndev) return mgx::Fail(MGX_ERR_INVALID_ARGUMENT, "mgx_index_create: bad device");
  if (const int rc = IndexOpenStreams(idx.get())) return rc;
  const uint32_t n_tiles = static_cast<uint32_t>((n_docs + mgx::kTileDocs - 1) >> mgx::kTileShift);
  idx->n_grams = G;
  idx->h_offsets.assign(d->offsets, d->offsets + G + 1);
  idx->words_per_row = static_cast<uint64_t>(n_tiles) * mgx::kWordsPerTile;
  idx->can_score = d->tf != nullptr && d->doc_len != nullptr;

  MGX_HIP(mgx::Upload(idx->d_offsets, d->offsets, G + 1));
  MGX_HIP(mgx::Upload(idx->d_docids, d->docids, P, 4));
  uint32_t max_doc_len = 0;
  if (idx->can_score) {
    if (d->n_tf_overflow) {
      if (!d->tf_overflow_pos || !d->tf_overflow_val || d->n_tf_overflow > 0xFFFFFFFFull)
        return mgx::Fail(MGX_ERR_INVALID_ARGUMENT, "mgx_index_create: bad tf overflow table");
      for (uint64_t i = 0; i < d->n_tf_overflow; ++i)
        if (d->tf_overflow_pos[i] >= P || (i && d->tf_overflow_pos[i] <= d->tf_overflow_pos[i - 1]) ||
            d->tf[d->tf_overflow_pos[i]] != 255 || d->tf_overflow_val[i] < 255)
          return mgx::Fail(MGX_ERR_INVALID_ARGUMENT,
                           "mgx_index_create: tf overflow entries must ascend, point at tf bytes of 255 and hold counts >= 255");
      MGX_HIP(mgx::Upload(idx->d_tf_ovf_pos, d->tf_overflow_pos, d->n_tf_overflow));
      MGX_HIP(mgx::Upload(idx->d_tf_ovf_val, d->tf_overflow_val, d->n_tf_overflow));
    }
    MGX_HIP(mgx::Upload(idx->d_tf, d->tf, P, 4));
    MGX_HIP(mgx::Upload(idx->d_doc_len, d->doc_len, n_docs));
    for (uint64_t i = 0; i < n_docs; ++i) max_doc_len = std::max(max_doc_len, d->doc_len[i]);
    // padded to whole tiles (zeros): group_score_kernel copies a tile's 16 KiB into LDS whole
    std::vector<uint8_t> dl8((n_docs + mgx::kTileDocs - 1) / mgx::kTileDocs * mgx::kTileDocs, 0);
    for (uint64_t i = 0; i < n_docs; ++i) dl8[i] = static_cast<uint8_t>(std::min<uint32_t>(d->doc_len[i], 255u));
    MGX_HIP(mgx::Upload(idx->d_dl8, dl8.data(), dl8.size(), 16));
  }
  if (const int rc = IndexDeriveRest(idx.get(), d->first_doc_id, n_docs, d->dense_threshold,
                                     idx->can_score ? d->n_tf_overflow : 0, max_doc_len))
    return rc;
  *out = idx.release();
  return MGX_OK;
}

static int IndexOpenStreams(mgx_index* idx) {
  MGX_HIP(hipSetDevice(idx->device));
  MGX_HIP(hipStreamCreateWithFlags(&idx->stream, hipStreamNonBlocking));
  // The side stream (the few queries the main launch does not take: cand_kernel, the list-operand and general kernels)
  // is created at the device's highest priority. At the default priority it shared a hardware queue with the batch
  // streams, so its launch — a few dozen workgroups for ~0.27 ms on the benchmark batch — ran BEFORE the main launch
  // instead of beside it; a high-priority stream gets a queue of its own.
  int prio_least = 0, prio_greatest = 0;
  MGX_HIP(hipDeviceGetStreamPriorityRange(&prio_least, &prio_greatest));
  MGX_HIP(hipStreamCreateWithPriority(&idx->side_stream, hipStreamNonBlocking, prio_greatest));
  return MGX_OK;
}

// idx holds: device, streams, n_grams, h_offsets, words_per_row, can_score, and on the device offsets, docids and, when
// it scores, tf, doc_len, dl8 and the tf overflow table.
static int IndexDeriveRest(mgx_index* idx, uint32_t first_doc_id, uint64_t n_docs, double dense_threshold,
                           uint64_t n_tf_overflow, uint32_t max_doc_len) {
  const uint64_t G = idx->n_grams;
  const uint64_t* offsets = idx->h_offsets.data();
  const uint32_t n_tiles = static_cast<uint32_t>((n_docs + mgx::kTileDocs - 1) >> mgx::kTileShift);
  // which grams get a skip row / a dense bitmap
  double dense_thr = dense_threshold == 0.0 ? 1.0 / 256.0 : dense_threshold;
  const uint64_t skip_min = std::max<uint64_t>(64, static_cast<uint64_t>(n_tiles) + 1);
  idx->h_skip_row.assign(G, mgx::kNoRow);
  idx->h_bm_row.assign(G, mgx::kNoRow);
  std::vector<uint32_t> skip_grams, bm_grams;
  std::vector<uint64_t> bm_lo, bm_hi;
  for (uint64_t g = 0; g < G; ++g) {
    const uint64_t len = offsets[g + 1] - offsets[g];
    if (len > 0xFFFFFFFFull) return mgx::Fail(MGX_ERR_OUT_OF_RANGE, "a posting list exceeds 2^32 entries");
    const bool dense = len > 0 && static_cast<double>(len) >= dense_thr * static_cast<double>(n_docs);
    if (dense) {
      idx->h_bm_row[g] = static_cast<uint32_t>(bm_grams.size());
      bm_grams.push_back(static_cast<uint32_t>(g));
      bm_lo.push_back(offsets[g]);
      bm_hi.push_back(offsets[g + 1]);
    }
    if (dense || len >= skip_min) {
      idx->h_skip_row[g] = static_cast<uint32_t>(skip_grams.size());
      skip_grams.push_back(static_cast<uint32_t>(g));
    }
  }
  MGX_HIP(mgx::Upload(idx->d_skip_row, idx->h_skip_row.data(), G));
  {
    DevBuf d_rows;
    MGX_HIP(mgx::Upload(d_rows, skip_grams.data(), skip_grams.size()));
    MGX_HIP(idx->d_tile_off.Alloc(skip_grams.size() * (static_cast<size_t>(n_tiles) + 1) * sizeof(uint32_t)));
    MGX_LAUNCH(mgx::LaunchBuildTileOff(idx->d_offsets.as<uint64_t>(), idx->d_docids.as<uint32_t>(),
                                       d_rows.as<uint32_t>(), static_cast<uint32_t>(skip_grams.size()), n_tiles,
                                       first_doc_id, idx->d_tile_off.as<uint32_t>(), idx->stream));
    MGX_HIP(hipStreamSynchronize(idx->stream));
  }
  if (!bm_grams.empty()) {
    DevBuf d_lo, d_hi;
    MGX_HIP(mgx::Upload(d_lo, bm_lo.data(), bm_lo.size()));
    MGX_HIP(mgx::Upload(d_hi, bm_hi.data(), bm_hi.size()));
    MGX_HIP(idx->d_gram_bitmaps.Alloc(bm_grams.size() * idx->words_per_row * sizeof(uint64_t)));
    MGX_HIP(hipMemsetAsync(idx->d_gram_bitmaps.p, 0, idx->d_gram_bitmaps.bytes, idx->stream));
    MGX_LAUNCH(mgx::LaunchBuildBitmaps(idx->d_docids.as<uint32_t>(), d_lo.as<uint64_t>(), d_hi.as<uint64_t>(),
                                       static_cast<uint32_t>(bm_grams.size()), first_doc_id, 0,
                                       /*tile_stride=*/bm_grams.size() * mgx::kWordsPerTile,
                                       /*row_stride=*/mgx::kWordsPerTile, idx->d_gram_bitmaps.as<uint64_t>(),
                                       idx->stream));
    MGX_HIP(hipStreamSynchronize(idx->stream));
    if (idx->can_score) {
      // tf of the dense grams by doc slot (4 bits per doc); rows padded off power-of-two strides
      const uint64_t stride = static_cast<uint64_t>(n_tiles) * (mgx::kTileDocs / 2) + 4352;
      MGX_HIP(idx->d_tfnib.Alloc(bm_grams.size() * stride + 256));
      MGX_HIP(hipMemsetAsync(idx->d_tfnib.p, 0, idx->d_tfnib.bytes, idx->stream));
      MGX_LAUNCH(mgx::LaunchBuildTfNib(idx->d_docids.as<uint32_t>(), idx->d_tf.as<uint8_t>(), d_lo.as<uint64_t>(),
                                       d_hi.as<uint64_t>(), static_cast<uint32_t>(bm_grams.size()), first_doc_id,
                                       stride, idx->d_tfnib.as<uint8_t>(), idx->stream));
      MGX_HIP(hipStreamSynchronize(idx->stream));
      idx->dev.nib_row_stride = stride;
    }
  }
  if (idx->can_score) {  // (sparse scored grams get tables too: keyed by gram id, see UploadGroup)
    idx->table_dl = mgx::FastTableDl(max_doc_len);
    idx->table_cap = static_cast<uint32_t>(std::min<uint64_t>(2 * bm_grams.size() + 4096, 1u << 20));
    MGX_HIP(idx->d_table_pool.Alloc(static_cast<size_t>(idx->table_cap) * idx->table_doubles() * sizeof(double)));
  }

  mgx::DevIndex& v = idx->dev;
  v.offsets = idx->d_offsets.as<uint64_t>();
  v.docids = idx->d_docids.as<uint32_t>();
  v.tf = idx->d_tf.as<uint8_t>();
  v.tf_ovf_pos = idx->d_tf_ovf_pos.as<uint64_t>();
  v.tf_ovf_val = idx->d_tf_ovf_val.as<uint32_t>();
  v.n_tf_ovf = idx->can_score ? static_cast<uint32_t>(n_tf_overflow) : 0u;
  v.doc_len = idx->d_doc_len.as<uint32_t>();
  v.dl8 = idx->d_dl8.as<uint8_t>();
  v.tfnib = idx->d_tfnib.as<uint8_t>();
  v.skip_row = idx->d_skip_row.as<uint32_t>();
  v.tile_off = idx->d_tile_off.as<uint32_t>();
  v.gram_bitmaps = idx->d_gram_bitmaps.as<uint64_t>();
  v.gb_tile_stride = bm_grams.size() * mgx::kWordsPerTile;
  idx->n_bitmap_rows = static_cast<uint32_t>(bm_grams.size());
  if (idx->can_score && !bm_grams.empty()) {
    // the grams held by more than a twentieth of the docs get block-max bytes per 16-doc quarter (GetBlockMax):
    // measured on the benchmark batch, 0.05 beats 0.2 (1.55 vs 1.62 ms) and no fine rows at all (1.97 ms)
    static const double kFineDensity = std::getenv("MGX_FINE_DENSITY") ? atof(std::getenv("MGX_FINE_DENSITY")) : 0.05;
    std::vector<uint32_t> fine_map(bm_grams.size(), mgx::kNoRow), fine_rows;
    for (size_t r = 0; r < bm_grams.size(); ++r) {
      const uint64_t sz = offsets[bm_grams[r] + 1] - offsets[bm_grams[r]];
      if (static_cast<double>(sz) > kFineDensity * static_cast<double>(n_docs)) {
        fine_map[r] = static_cast<uint32_t>(fine_rows.size());
        fine_rows.push_back(static_cast<uint32_t>(r));
      }
    }
    idx->n_fine_rows = static_cast<uint32_t>(fine_rows.size());
    idx->h_fine_map = fine_map;
    MGX_HIP(mgx::Upload(idx->d_fine_rows, fine_rows.data(), fine_rows.size(), 1));
  }
  if (std::getenv("MGX_VERBOSE"))
    fprintf(stderr, "[mgx] index: %u tiles, block-max bounds per quarter for %u of %u bitmap rows\n", n_tiles, idx->n_fine_rows,
            idx->n_bitmap_rows);
  v.gb_row_stride = mgx::kWordsPerTile;
  idx->filter_row_stride = idx->words_per_row + 32 * ((n_tiles % 2) ? 1 : 3);  // 256 B / 768 B of padding
  v.fb_tile_stride = mgx::kWordsPerTile;
  v.fb_row_stride = idx->filter_row_stride;
  v.filter_bitmaps = nullptr;
  v.first_doc_id = first_doc_id;
  v.n_docs = static_cast<uint32_t>(n_docs);
  v.n_tiles = n_tiles;
  v.max_doc_len = max_doc_len;
  MGX_HIP(mgx::SyncDevIndex(idx));
  return MGX_OK;
}

int mgx_index_create(const mgx_index_desc* desc, mgx_index** out) {
  if (out) *out = nullptr;
  if (!desc || !out) return mgx::Fail(MGX_ERR_INVALID_ARGUMENT, "mgx_index_create: null argument");
  if (desc->struct_size < sizeof(mgx_index_desc) || desc->version != MGX_ABI_VERSION)
    return mgx::Fail(MGX_ERR_INVALID_ARGUMENT, "mgx_index_create: bad struct_size/version");
  if (desc->tile_shift != 0 && desc->tile_shift != static_cast<uint32_t>(mgx::kTileShift))
    return mgx::Fail(MGX_ERR_NOT_IMPLEMENTED, "mgx_index_create: only tile_shift 14 is built");
  if (!desc->offsets || (desc->n_grams && desc->offsets[desc->n_grams] && !desc->docids))
    return mgx::Fail(MGX_ERR_INVALID_ARGUMENT, "mgx_index_create: null posting arrays");
  try {
    return IndexCreateImpl(desc, out);
  } catch (const std::exception& e) {
    return mgx::Fail(MGX_ERR_INTERNAL, std::string("mgx_index_create: ") + e.what());
  }
}

int mgx_index_build_device(const mgx_build_params* params, const mgx_index_build_desc* desc, const uint8_t* text_bytes,
                           const uint64_t* text_off, uint32_t first_doc_id, uint64_t n_docs, mgx_columns** dictionary_out,
                           mgx_index** index_out) {
  if (dictionary_out) *dictionary_out = nullptr;
  if (index_out) *index_out = nullptr;
  // ---- host-only checks first: mgx_columns_build_device's, then mgx_index_create's; they answer without a device ---------
  if (!params || !desc || !dictionary_out || !index_out || !text_off ||
      (n_docs && !text_bytes && text_off[n_docs] != text_off[0]))
    return mgx::Fail(MGX_ERR_INVALID_ARGUMENT, "mgx_index_build_device: null argument");
  if (params->struct_size < sizeof(mgx_build_params) || params->version != MGX_ABI_VERSION ||
      desc->struct_size < sizeof(mgx_index_build_desc) || desc->version != MGX_ABI_VERSION)
    return mgx::Fail(MGX_ERR_INVALID_ARGUMENT, "mgx_index_build_device: bad struct_size/version");
  if (static_cast<uint64_t>(first_doc_id) + n_docs > 0xFFFFFFFFull)
    return mgx::Fail(MGX_ERR_OUT_OF_RANGE, "mgx_index_build_device: doc ids exceed uint32");
  const int kanji_n = params->kanji_ngram_size > 0 ? params->kanji_ngram_size : params->ngram_size;
  if (params->ngram_size > mgx::build::kMaxGram || kanji_n > mgx::build::kMaxGram)
    return mgx::Fail(MGX_ERR_NOT_IMPLEMENTED,
                     "mgx_index_build_device: n-grams of more than 3 code points are not built on the device (a gram is "
                     "packed into 64 bits); use mgx_columns_build and mgx_index_create");
  for (uint64_t d = 0; d < n_docs; ++d)
    if (text_off[d + 1] < text_off[d])
      return mgx::Fail(MGX_ERR_INVALID_ARGUMENT, "mgx_index_build_device: text_off descends");
  if (desc->tile_shift != 0 && desc->tile_shift != static_cast<uint32_t>(mgx::kTileShift))
    return mgx::Fail(MGX_ERR_NOT_IMPLEMENTED, "mgx_index_build_device: only tile_shift 14 is built");
  if (n_docs == 0) return mgx::Fail(MGX_ERR_OUT_OF_RANGE, "mgx_index_build_device: n_docs must be in [1, 2^32) and ids fit uint32");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
    (void)hipGetLastError();
    return mgx::Fail(MGX_ERR_INTERNAL, "no HIP device available: libmygram_gpu has no CPU fallback");
  }
  if (desc->device < 0 || desc->device >= ndev) return mgx::Fail(MGX_ERR_INVALID_ARGUMENT, "mgx_index_build_device: bad device");
  if (text_off[n_docs] - text_off[0] > mgx::build::kMaxTextBytes)
    return mgx::Fail(MGX_ERR_OUT_OF_RANGE, "mgx_index_build_device: " + std::to_string(text_off[n_docs] - text_off[0]) +
                                               " bytes of text, the device builder takes " +
                                               std::to_string(mgx::build::kMaxTextBytes) + "; use mgx_columns_build");
  mgx_index* made = nullptr;
  mgx::Columns* cols = nullptr;
  auto undo = [&](int rc) {
    if (made) mgx_index_destroy(made);
    if (cols) mgx::DestroyColumns(cols);
    return rc;
  };
  static const bool kTrace = std::getenv("MGX_TRACE_HOST") != nullptr;
  const auto t0 = std::chrono::steady_clock::now();
  try {
    const bool attach = desc->attach_text != 0;
    mgx::build::PackedColumns packed;
    mgx::build::ResidentArrays res;
    std::string err;
    const int rc = mgx::build::BuildOnDevice(*params, text_bytes, text_off, first_doc_id, n_docs, desc->device, &packed, &err,
                                             &res, attach);
    if (rc != MGX_OK) return mgx::Fail(rc, err);
    const auto t1 = std::chrono::steady_clock::now();
    cols = mgx::ColumnsFromPacked(*params, text_off, first_doc_id, n_docs, std::move(packed));
    mgx_columns_view cv;
    mgx::ColumnsView(cols, &cv);
    const auto t2 = std::chrono::steady_clock::now();

    // ---- the index adopts the builder's arrays: what IndexCreateImpl uploads is there already -----------------------------
    auto idx = std::make_unique<mgx_index>();
    idx->device = desc->device;
    auto adopt = [](DevBuf& b, void*& p, uint64_t bytes) {
      b.Free();
      b.p = p;
      b.bytes = static_cast<size_t>(bytes);
      b.owned = true;
      p = nullptr;
    };
    adopt(idx->d_docids, res.docids, res.plan.docids);
    adopt(idx->d_tf, res.tf, res.plan.tf);
    adopt(idx->d_doc_len, res.doc_len, res.plan.doc_len);
    adopt(idx->d_dl8, res.dl8, res.plan.dl8);
    if (attach) {
      adopt(idx->d_text, res.text, res.plan.text);
      adopt(idx->d_text_off, res.text_off, res.plan.text_off);
    }
    made = idx.release();
    if (const int e = IndexOpenStreams(made)) return undo(e);
    const uint64_t G = cv.n_grams;
    const uint32_t n_tiles = static_cast<uint32_t>((n_docs + mgx::kTileDocs - 1) >> mgx::kTileShift);
    made->n_grams = G;
    made->h_offsets.assign(cv.offsets, cv.offsets + G + 1);
    made->words_per_row = static_cast<uint64_t>(n_tiles) * mgx::kWordsPerTile;
    made->can_score = true;
    auto up = [&](hipError_t e, const char* what) {
      if (e == hipSuccess) return 0;
      (void)hipGetLastError();
      return mgx::Fail(MGX_ERR_INTERNAL, std::string("mgx_index_build_device: ") + what + ": " + hipGetErrorString(e));
    };
    if (const int e = up(mgx::Upload(made->d_offsets, cv.offsets, G + 1), "offsets")) return undo(e);
    if (cv.n_tf_overflow) {
      if (const int e = up(mgx::Upload(made->d_tf_ovf_pos, cv.tf_overflow_pos, cv.n_tf_overflow), "tf overflow")) return undo(e);
      if (const int e = up(mgx::Upload(made->d_tf_ovf_val, cv.tf_overflow_val, cv.n_tf_overflow), "tf overflow")) return undo(e);
    }
    uint32_t max_doc_len = 0;
    for (uint64_t i = 0; i < n_docs; ++i) max_doc_len = std::max(max_doc_len, cv.doc_len[i]);
    if (attach) {  // what mgx_index_attach_text leaves behind
      uint64_t longest = 0;
      for (uint64_t i = 0; i < n_docs; ++i) longest = std::max<uint64_t>(longest, text_off[i + 1] - text_off[i]);
      made->max_text_bytes = static_cast<uint32_t>(longest);
      made->dev.text = made->d_text.as<uint8_t>();
      made->dev.text_off = made->d_text_off.as<uint64_t>();
    }
    if (const int e = IndexDeriveRest(made, first_doc_id, n_docs, desc->dense_threshold, cv.n_tf_overflow, max_doc_len))
      return undo(e);
    if (kTrace) {
      const auto ms = [](auto a, auto b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
      fprintf(stderr, "[mgx] resident build of %llu docs: device build and copies %.2f ms, dictionary %.2f ms, rest of the index %.2f ms\n",
              static_cast<unsigned long long>(n_docs), ms(t0, t1), ms(t1, t2), ms(t2, std::chrono::steady_clock::now()));
    }
    *dictionary_out = reinterpret_cast<mgx_columns*>(cols);
    *index_out = made;
    return MGX_OK;
  } catch (const std::exception& e) {
    return undo(mgx::Fail(MGX_ERR_INTERNAL, std::string("mgx_index_build_device: ") + e.what()));
  }
}

int mgx_index_read_postings(mgx_index* idx, uint32_t gram_id, uint32_t* docids, uint8_t* tf, uint64_t capacity, uint64_t* n) {
  if (!idx || !n) return mgx::Fail(MGX_ERR_INVALID_ARGUMENT, "mgx_index_read_postings: null argument");
  *n = 0;
  std::lock_guard<std::mutex> lock(idx->mu);
  if (gram_id >= idx->n_grams) return mgx::Fail(MGX_ERR_OUT_OF_RANGE, "mgx_index_read_postings: unknown gram id");
  const uint64_t lo = idx->h_offsets[gram_id], len = idx->h_offsets[gram_id + 1] - lo;
  *n = len;
  if (len == 0 || (!docids && !tf)) return MGX_OK;  // size query
  if (capacity < len) return mgx::Fail(MGX_ERR_OUT_OF_RANGE, "mgx_index_read_postings: buffer too small (*n holds the count)");
  MGX_HIP(hipSetDevice(idx->device));
  if (docids) MGX_HIP(hipMemcpy(docids, idx->d_docids.as<uint32_t>() + lo, len * 4, hipMemcpyDeviceToHost));
  if (tf && idx->can_score) MGX_HIP(hipMemcpy(tf, idx->d_tf.as<uint8_t>() + lo, len, hipMemcpyDeviceToHost));
  return MGX_OK;
}

void mgx_index_destroy(mgx_index* idx) {
  if (!idx) return;
  (void)hipSetDevice(idx->device);
  if (idx->stream) (void)hipStreamDestroy(idx->stream);
  if (idx->side_stream) (void)hipStreamDestroy(idx->side_stream);
  if (idx->table_stream) {
    (void)hipStreamSynchronize(idx->table_stream);
    (void)hipStreamDestroy(idx->table_stream);
  }
  if (idx->table_ev) (void)hipEventDestroy(idx->table_ev);
  if (idx->job_ring) (void)hipHostFree(idx->job_ring);
  delete idx;
}

int mgx_posting_size(const mgx_index* idx, uint32_t gram_id, uint64_t* out) {
  if (out) *out = 0;
  if (!idx || !out) return mgx::Fail(MGX_ERR_INVALID_ARGUMENT, "mgx_posting_size: null argument");
  if (gram_id >= idx->n_grams) return mgx::Fail(MGX_ERR_OUT_OF_RANGE, "mgx_posting_size: unknown gram id");
  *out = idx->h_offsets[gram_id + 1] - idx->h_offsets[gram_id];
  return MGX_OK;
}

int mgx_index_memory_bytes(const mgx_index* idx, uint64_t* out) {
  if (out) *out = 0;
  if (!idx || !out) return mgx::Fail(MGX_ERR_INVALID_ARGUMENT, "mgx_index_memory_bytes: null argument");
  *out = idx->d_offsets.bytes + idx->d_docids.bytes + idx->d_tf.bytes + idx->d_doc_len.bytes +
         idx->d_skip_row.bytes + idx->d_tile_off.bytes + idx->d_gram_bitmaps.bytes + idx->d_filter_bitmaps.bytes +
         idx->d_text.bytes + idx->d_text_off.bytes + idx->d_dl8.bytes + idx->d_tfnib.bytes + idx->d_table_pool.bytes +
         idx->d_tf_ovf_pos.bytes + idx->d_tf_ovf_val.bytes + idx->d_orig.bytes + idx->d_orig_off.bytes +
         idx->d_orig_kind.bytes + idx->d_orig_map.bytes + idx->d_orig_map_off.bytes;
  {  // the per-(k1, b, avgdl) pruning arrays built so far
    std::lock_guard<std::mutex> lock(const_cast<mgx_index*>(idx)->table_mu);
    for (const auto& t : idx->block_max) *out += t->d.bytes + t->d_fine.bytes;
    for (const auto& t : idx->norm_tables) *out += t->d.bytes;
  }
  return MGX_OK;
}

int mgx_index_set_batch_order(mgx_index* idx, uint32_t order) {
  if (!idx || order > MGX_ORDER_CONCURRENT) return mgx::Fail(MGX_ERR_INVALID_ARGUMENT, "mgx_index_set_batch_order: bad argument");
  idx->fifo.store(order == MGX_ORDER_FIFO ? 1 : 0);
  return MGX_OK;
}

int mgx_index_attach_text(mgx_index* idx, const uint8_t* text_bytes, const uint64_t* text_off) {
  if (!idx || !text_off) return mgx::Fail(MGX_ERR_INVALID_ARGUMENT, "mgx_index_attach_text: null argument");
  const uint64_t n = idx->dev.n_docs;
  for (uint64_t i = 0; i < n; ++i)
    if (text_off[i + 1] < text_off[i] || text_off[i + 1] - text_off[i] > 0xFFFFFFFFull)
      return mgx::Fail(MGX_ERR_INVALID_ARGUMENT, "mgx_index_attach_text: offsets must ascend");
  const uint64_t total = text_off[n] - text_off[0];
  if (total && !text_bytes) return mgx::Fail(MGX_ERR_INVALID_ARGUMENT, "mgx_index_attach_text: null text");
  std::lock_guard<std::mutex> lock(idx->mu);
  MGX_HIP(hipSetDevice(idx->device));
  std::vector<uint64_t> rel(n + 1);
  for (uint64_t i = 0; i <= n; ++i) rel[i] = text_off[i] - text_off[0];
  // (the text scan reads aligned 16-byte chunks up to 48 bytes past a doc's end)
  MGX_HIP(mgx::Upload(idx->d_text, text_bytes ? text_bytes + text_off[0] : nullptr, total, 128));
  MGX_HIP(mgx::Upload(idx->d_text_off, rel.data(), rel.size()));
  idx->dev.text = idx->d_text.as<uint8_t>();
  idx->dev.text_off = idx->d_text_off.as<uint64_t>();
  uint64_t longest = 0;
  for (uint64_t i = 0; i < n; ++i) longest = std::max<uint64_t>(longest, text_off[i + 1] - text_off[i]);
  idx->max_text_bytes = static_cast<uint32_t>(longest);
  // originals and maps were checked against the texts they replace: attach them again after new texts
  idx->d_orig.Free();
  idx->d_orig_off.Free();
  idx->d_orig_kind.Free();
  idx->d_orig_map.Free();
  idx->d_orig_map_off.Free();
  idx->originals = mgx::highlight::DevOriginals{};
  idx->max_original_bytes = 0;
  MGX_HIP(mgx::SyncDevIndex(idx));
  return MGX_OK;
}

int mgx_index_max_text_bytes(const mgx_index* idx, uint32_t* out) {
  if (out) *out = 0;
  if (!idx || !out) return mgx::Fail(MGX_ERR_INVALID_ARGUMENT, "mgx_index_max_text_bytes: null argument");
  *out = idx->dev.text ? idx->max_text_bytes : 0;
  return MGX_OK;
}

int mgx_index_attach_original_text(mgx_index* idx, const uint8_t* bytes, const uint64_t* off, const uint8_t* kind,
                                   const uint32_t* map_pairs, const uint64_t* map_off) {
  namespace hl = mgx::highlight;
  if (!idx || !off || !kind || !map_off)
    return mgx::Fail(MGX_ERR_INVALID_ARGUMENT, "mgx_index_attach_original_text: null argument");
  if (!idx->dev.text)
    return mgx::Fail(MGX_ERR_INVALID_ARGUMENT, "mgx_index_attach_original_text: call mgx_index_attach_text first");
  const uint64_t n = idx->dev.n_docs;
  for (uint64_t i = 0; i < n; ++i) {
    if (off[i + 1] < off[i] || off[i + 1] - off[i] > 0x7FFFFF00ull)
      return mgx::Fail(MGX_ERR_INVALID_ARGUMENT, "mgx_index_attach_original_text: offsets must ascend (slot " + std::to_string(i) + ")");
    if (map_off[i + 1] < map_off[i])
      return mgx::Fail(MGX_ERR_INVALID_ARGUMENT, "mgx_index_attach_original_text: map offsets must ascend (slot " + std::to_string(i) + ")");
  }
  const uint64_t total = off[n] - off[0], total_pairs = map_off[n] - map_off[0];
  if ((total && !bytes) || (total_pairs && !map_pairs))
    return mgx::Fail(MGX_ERR_INVALID_ARGUMENT, "mgx_index_attach_original_text: null text or map");
  try {
    std::lock_guard<std::mutex> lock(idx->mu);
    MGX_HIP(hipSetDevice(idx->device));
    // the normalized texts' code points, from the resident copy (attach time only: no query reads anything back), in
    // pieces of whole documents of about 64 MiB so that the host never holds the corpus twice
    std::vector<uint64_t> t_off(n + 1);
    MGX_HIP(hipMemcpy(t_off.data(), idx->d_text_off.p, (n + 1) * 8, hipMemcpyDeviceToHost));
    constexpr uint64_t kPiece = 64ull << 20;
    std::vector<uint8_t> norm;
    uint64_t piece_begin = 0, piece_end = 0;  // the documents [piece_begin, piece_end) are in `norm`
    uint64_t longest = 0;
    for (uint64_t i = 0; i < n; ++i) {
      if (i >= piece_end) {
        piece_begin = i;
        piece_end = i + 1;
        while (piece_end < n && t_off[piece_end + 1] - t_off[piece_begin] <= kPiece) ++piece_end;
        const uint64_t bytes = t_off[piece_end] - t_off[piece_begin];
        norm.resize(bytes);
        if (bytes) MGX_HIP(hipMemcpy(norm.data(), idx->d_text.as<uint8_t>() + t_off[piece_begin], bytes, hipMemcpyDeviceToHost));
      }
      const std::string who = "mgx_index_attach_original_text: slot " + std::to_string(i) + ": ";
      const uint64_t pairs = map_off[i + 1] - map_off[i];
      if (kind[i] > MGX_ORIG_UNMAPPABLE) return mgx::Fail(MGX_ERR_INVALID_ARGUMENT, who + "unknown kind " + std::to_string(kind[i]));
      if (kind[i] != MGX_ORIG_MAPPED && pairs) return mgx::Fail(MGX_ERR_INVALID_ARGUMENT, who + "only a MGX_ORIG_MAPPED document has map pairs");
      if (kind[i] == MGX_ORIG_NONE) continue;
      const uint8_t* o = bytes + off[i];
      const uint64_t len = off[i + 1] - off[i];
      uint64_t cps = 0;
      for (uint64_t p = 0; p < len; ++cps) {
        uint32_t cp = 0;
        const int k = mgx::text::ParseUtf8(o + p, len - p, &cp);
        if (k <= 0) return mgx::Fail(MGX_ERR_INVALID_ARGUMENT, who + "the original is not valid UTF-8");
        p += static_cast<uint64_t>(k);
      }
      longest = std::max(longest, len);
      if (kind[i] == MGX_ORIG_UNMAPPABLE) continue;
      const uint64_t norm_cps = hl::CountCps(norm.data() + (t_off[i] - t_off[piece_begin]), t_off[i + 1] - t_off[i]);
      if (kind[i] == MGX_ORIG_IDENTITY) {
        if (cps != norm_cps)
          return mgx::Fail(MGX_ERR_INVALID_ARGUMENT, who + "an identity original has " + std::to_string(cps) + " code points, its normalized text " + std::to_string(norm_cps));
        continue;
      }
      if (pairs != norm_cps)
        return mgx::Fail(MGX_ERR_INVALID_ARGUMENT, who + "the map has " + std::to_string(pairs) + " pairs, the normalized text " + std::to_string(norm_cps) + " code points");
      const uint32_t* m = map_pairs + 2 * map_off[i];
      for (uint64_t p = 0; p < pairs; ++p) {
        if (!(m[2 * p] < m[2 * p + 1] && m[2 * p + 1] <= cps))
          return mgx::Fail(MGX_ERR_INVALID_ARGUMENT, who + "map pair " + std::to_string(p) + " is not start < end <= the original's code points");
        if (p && (m[2 * p] < m[2 * p - 2] || m[2 * p + 1] < m[2 * p - 1]))
          return mgx::Fail(MGX_ERR_INVALID_ARGUMENT, who + "map pair " + std::to_string(p) + ": starts and ends must not decrease");
      }
    }
    std::vector<uint64_t> rel(n + 1), mrel(n + 1);
    for (uint64_t i = 0; i <= n; ++i) {
      rel[i] = off[i] - off[0];
      mrel[i] = map_off[i] - map_off[0];
    }
    MGX_HIP(mgx::Upload(idx->d_orig, bytes ? bytes + off[0] : nullptr, total, 128));
    MGX_HIP(mgx::Upload(idx->d_orig_off, rel.data(), rel.size()));
    MGX_HIP(mgx::Upload(idx->d_orig_kind, kind, n, 16));
    MGX_HIP(mgx::Upload(idx->d_orig_map, map_pairs ? map_pairs + 2 * map_off[0] : nullptr, 2 * total_pairs, 16));
    MGX_HIP(mgx::Upload(idx->d_orig_map_off, mrel.data(), mrel.size()));
    idx->originals = hl::DevOriginals{idx->d_orig.as<uint8_t>(), idx->d_orig_off.as<uint64_t>(), idx->d_orig_kind.as<uint8_t>(),
                                      idx->d_orig_map.as<hl::MapPair>(), idx->d_orig_map_off.as<uint64_t>()};
    idx->max_original_bytes = static_cast<uint32_t>(longest);
    return MGX_OK;
  } catch (const std::exception& e) {
    return mgx::Fail(MGX_ERR_INTERNAL, std::string("mgx_index_attach_original_text: ") + e.what());
  }
}

int mgx_index_max_original_text_bytes(const mgx_index* idx, uint32_t* out) {
  if (out) *out = 0;
  if (!idx || !out) return mgx::Fail(MGX_ERR_INVALID_ARGUMENT, "mgx_index_max_original_text_bytes: null argument");
  *out = idx->originals.kind ? idx->max_original_bytes : 0;
  return MGX_OK;
}

// A fresh, zeroed row of the filter bitmap pool (the pool doubles when full). Called with idx->mu held; the row is
// counted (n_filter_rows) by the caller once its bits are in place.
static int NewFilterRow(mgx_index* idx, uint32_t* row_out) {
  if (idx->n_filter_rows == idx->filter_cap_rows) {
    const uint32_t ncap = idx->filter_cap_rows ? idx->filter_cap_rows * 2 : 8;
    DevBuf nb;
    MGX_HIP(nb.Alloc(static_cast<size_t>(ncap) * idx->filter_row_stride * sizeof(uint64_t)));
    if (idx->n_filter_rows)
      MGX_HIP(hipMemcpy(nb.p, idx->d_filter_bitmaps.p,
                        static_cast<size_t>(idx->n_filter_rows) * idx->filter_row_stride * sizeof(uint64_t),
                        hipMemcpyDeviceToDevice));
    // (rows are added while batches run — a FILTER condition becomes a row the first time it is seen — and a kernel in
    // flight still reads the old pool: it is retired, not freed; doubling keeps the waste below the pool's own size)
    idx->retired_filter_pools.push_back(std::move(idx->d_filter_bitmaps));
    idx->d_filter_bitmaps = std::move(nb);
    idx->filter_cap_rows = ncap;
    idx->dev.filter_bitmaps = idx->d_filter_bitmaps.as<uint64_t>();
    MGX_HIP(mgx::SyncDevIndex(idx));
  }
  const uint32_t row = idx->n_filter_rows;
  uint64_t* dst = idx->d_filter_bitmaps.as<uint64_t>() + static_cast<uint64_t>(row) * idx->filter_row_stride;
  MGX_HIP(hipMemsetAsync(dst, 0, idx->filter_row_stride * sizeof(uint64_t), idx->stream));
  *row_out = row;
  return MGX_OK;
}

int mgx_index_add_filter_column(mgx_index* idx, const mgx_filter_column_desc* d, uint32_t* out_column_id) {
  if (out_column_id) *out_column_id = 0;
  if (!idx || !d || !out_column_id || !d->values)
    return mgx::Fail(MGX_ERR_INVALID_ARGUMENT, "mgx_index_add_filter_column: null argument");
  if (d->struct_size < sizeof(mgx_filter_column_desc) || d->version != MGX_ABI_VERSION)
    return mgx::Fail(MGX_ERR_INVALID_ARGUMENT, "mgx_index_add_filter_column: bad struct_size/version");
  if (d->value_class > MGX_FC_DOUBLE) return mgx::Fail(MGX_ERR_INVALID_ARGUMENT, "mgx_index_add_filter_column: unknown value class");
  const uint64_t n = idx->dev.n_docs;
  if (d->value_ids)
    for (uint64_t i = 0; i < n; ++i)
      if (d->value_ids[i] != 0xFFFFFFFFu && d->value_ids[i] >= d->n_values)
        return mgx::Fail(MGX_ERR_OUT_OF_RANGE, "mgx_index_add_filter_column: a value id is not below n_values");
  try {
    std::lock_guard<std::mutex> lock(idx->mu);
    MGX_HIP(hipSetDevice(idx->device));
    auto col = std::make_unique<mgx_index::FilterColumn>();
    col->value_class = d->value_class;
    col->n_values = d->value_ids ? d->n_values : 0;
    col->sort_keys = mgx::colsort::ScanKeys(d->value_class, static_cast<const uint64_t*>(d->values), d->is_null, n);
    MGX_HIP(mgx::Upload(col->d_values, static_cast<const uint64_t*>(d->values), n));
    if (d->is_null) MGX_HIP(mgx::Upload(col->d_null, d->is_null, n));
    if (d->value_ids) MGX_HIP(mgx::Upload(col->d_value_ids, d->value_ids, n));
    idx->filter_columns.push_back(std::move(col));
    idx->n_filter_columns.store(static_cast<uint32_t>(idx->filter_columns.size()), std::memory_order_release);
    *out_column_id = static_cast<uint32_t>(idx->filter_columns.size() - 1);
    return MGX_OK;
  } catch (const std::exception& e) {
    return mgx::Fail(MGX_ERR_INTERNAL, std::string("mgx_index_add_filter_column: ") + e.what());
  }
}

int mgx_index_filter_compare(mgx_index* idx, uint32_t column_id, uint32_t op, uint64_t literal_bits, double eq_epsilon,
                             int null_matches, int never_matches, uint32_t* out_bitmap_id) {
  if (out_bitmap_id) *out_bitmap_id = 0;
  if (!idx || !out_bitmap_id) return mgx::Fail(MGX_ERR_INVALID_ARGUMENT, "mgx_index_filter_compare: null argument");
  if (op > MGX_CMP_GE) return mgx::Fail(MGX_ERR_INVALID_ARGUMENT, "mgx_index_filter_compare: unknown operator");
  try {
    std::lock_guard<std::mutex> lock(idx->mu);
    if (column_id >= idx->filter_columns.size())
      return mgx::Fail(MGX_ERR_OUT_OF_RANGE, "mgx_index_filter_compare: unknown filter column");
    MGX_HIP(hipSetDevice(idx->device));
    const mgx_index::FilterColumn& col = *idx->filter_columns[column_id];
    uint32_t row = 0;
    int rc = NewFilterRow(idx, &row);
    if (rc) return rc;
    uint64_t* dst = idx->d_filter_bitmaps.as<uint64_t>() + static_cast<uint64_t>(row) * idx->filter_row_stride;
    MGX_LAUNCH(mgx::LaunchFilterCompare(col.d_values.as<uint64_t>(), col.d_null.as<uint8_t>(), idx->dev.n_docs,
                                        col.value_class, op, literal_bits, eq_epsilon, null_matches ? 1u : 0u,
                                        never_matches ? 1u : 0u, dst, idx->stream));
    MGX_HIP(hipStreamSynchronize(idx->stream));
    idx->n_filter_rows++;
    *out_bitmap_id = row;
    return MGX_OK;
  } catch (const std::exception& e) {
    return mgx::Fail(MGX_ERR_INTERNAL, std::string("mgx_index_filter_compare: ") + e.what());
  }
}

int mgx_index_add_filter_bitmap(mgx_index* idx, const uint32_t* docids, uint64_t n, uint32_t* out_bitmap_id) {
  if (out_bitmap_id) *out_bitmap_id = 0;
  if (!idx || !out_bitmap_id || (n && !docids))
    return mgx::Fail(MGX_ERR_INVALID_ARGUMENT, "mgx_index_add_filter_bitmap: null argument");
  std::lock_guard<std::mutex> lock(idx->mu);
  MGX_HIP(hipSetDevice(idx->device));
  for (uint64_t i = 0; i < n; ++i) {
    if (docids[i] < idx->dev.first_doc_id || docids[i] - idx->dev.first_doc_id >= idx->dev.n_docs)
      return mgx::Fail(MGX_ERR_OUT_OF_RANGE, "mgx_index_add_filter_bitmap: doc id outside the index range");
  }
  uint32_t row = 0;
  {
    const int rc = NewFilterRow(idx, &row);
    if (rc) return rc;
  }
  if (n) {
    DevBuf d_ids, d_lo, d_hi;
    MGX_HIP(mgx::Upload(d_ids, docids, n));
    const uint64_t lo = 0, hi = n;
    MGX_HIP(mgx::Upload(d_lo, &lo, 1));
    MGX_HIP(mgx::Upload(d_hi, &hi, 1));
    MGX_LAUNCH(mgx::LaunchBuildBitmaps(d_ids.as<uint32_t>(), d_lo.as<uint64_t>(), d_hi.as<uint64_t>(), 1,
                                       idx->dev.first_doc_id, row, /*tile_stride=*/mgx::kWordsPerTile,
                                       /*row_stride=*/idx->filter_row_stride, idx->d_filter_bitmaps.as<uint64_t>(),
                                       idx->stream));
    MGX_HIP(hipStreamSynchronize(idx->stream));
  } else {
    MGX_HIP(hipStreamSynchronize(idx->stream));
  }
  idx->n_filter_rows++;
  *out_bitmap_id = row;
  return MGX_OK;
}

int mgx_index_update_filter_bitmap(mgx_index* idx, uint32_t bitmap_id, const uint32_t* set_docids, uint64_t n_set,
                                   const uint32_t* clear_docids, uint64_t n_clear) {
  if (!idx || (n_set && !set_docids) || (n_clear && !clear_docids))
    return mgx::Fail(MGX_ERR_INVALID_ARGUMENT, "mgx_index_update_filter_bitmap: null argument");
  if (n_set + n_clear > 0xFFFFFFFFull) return mgx::Fail(MGX_ERR_OUT_OF_RANGE, "mgx_index_update_filter_bitmap: too many ids");
  try {
    std::lock_guard<std::mutex> lock(idx->mu);
    if (bitmap_id >= idx->n_filter_rows) return mgx::Fail(MGX_ERR_OUT_OF_RANGE, "mgx_index_update_filter_bitmap: unknown bitmap id");
    std::vector<uint32_t> slots;
    slots.reserve(n_set + n_clear);
    for (int part = 0; part < 2; ++part) {
      const uint32_t* ids = part == 0 ? set_docids : clear_docids;
      const uint64_t n = part == 0 ? n_set : n_clear;
      for (uint64_t i = 0; i < n; ++i) {
        if (ids[i] < idx->dev.first_doc_id || ids[i] - idx->dev.first_doc_id >= idx->dev.n_docs)
          return mgx::Fail(MGX_ERR_OUT_OF_RANGE, "mgx_index_update_filter_bitmap: doc id outside the index range");
        slots.push_back(ids[i] - idx->dev.first_doc_id);
      }
    }
    if (slots.empty()) return MGX_OK;
    MGX_HIP(hipSetDevice(idx->device));
    DevBuf d_slots;
    MGX_HIP(mgx::Upload(d_slots, slots.data(), slots.size()));
    uint64_t* row = idx->d_filter_bitmaps.as<uint64_t>() + static_cast<uint64_t>(bitmap_id) * idx->filter_row_stride;
    MGX_LAUNCH(mgx::LaunchUpdateBitmap(row, d_slots.as<uint32_t>(), static_cast<uint32_t>(n_set),
                                       static_cast<uint32_t>(slots.size()), idx->stream));
    MGX_HIP(hipStreamSynchronize(idx->stream));
    if (idx->live_row.load() == bitmap_id) {  // the live set changed: df counts of text-level terms are stale
      std::lock_guard<std::mutex> tl(idx->table_mu);
      idx->df_cache.clear();
    }
    return MGX_OK;
  } catch (const std::exception& e) {
    return mgx::Fail(MGX_ERR_INTERNAL, std::string("mgx_index_update_filter_bitmap: ") + e.what());
  }
}

int mgx_index_copy_text(mgx_index* idx, uint8_t* text_bytes, uint64_t capacity, uint64_t* text_off, uint64_t* total_bytes) {
  if (!idx || !total_bytes) return mgx::Fail(MGX_ERR_INVALID_ARGUMENT, "mgx_index_copy_text: null argument");
  *total_bytes = 0;
  std::lock_guard<std::mutex> lock(idx->mu);
  if (!idx->d_text_off.p) return mgx::Fail(MGX_ERR_INVALID_ARGUMENT, "mgx_index_copy_text: the index holds no texts (mgx_index_attach_text)");
  MGX_HIP(hipSetDevice(idx->device));
  const uint64_t n = idx->dev.n_docs;
  uint64_t total = 0;
  MGX_HIP(hipMemcpy(&total, idx->d_text_off.as<uint64_t>() + n, 8, hipMemcpyDeviceToHost));
  *total_bytes = total;
  if (!text_off && !text_bytes) return MGX_OK;  // size query
  if (!text_off || (total && !text_bytes)) return mgx::Fail(MGX_ERR_INVALID_ARGUMENT, "mgx_index_copy_text: null buffer");
  if (capacity < total) return mgx::Fail(MGX_ERR_OUT_OF_RANGE, "mgx_index_copy_text: buffer too small (*total_bytes holds the size)");
  MGX_HIP(hipMemcpy(text_off, idx->d_text_off.p, (n + 1) * 8, hipMemcpyDeviceToHost));
  if (total) MGX_HIP(hipMemcpy(text_bytes, idx->d_text.p, total, hipMemcpyDeviceToHost));
  return MGX_OK;
}

int mgx_index_read_text(mgx_index* idx, uint32_t doc_id, uint8_t* text, uint64_t capacity, uint64_t* len) {
  if (!idx || !len) return mgx::Fail(MGX_ERR_INVALID_ARGUMENT, "mgx_index_read_text: null argument");
  *len = 0;
  std::lock_guard<std::mutex> lock(idx->mu);
  if (!idx->d_text_off.p) return mgx::Fail(MGX_ERR_INVALID_ARGUMENT, "mgx_index_read_text: the index holds no texts (mgx_index_attach_text)");
  if (doc_id < idx->dev.first_doc_id || doc_id - idx->dev.first_doc_id >= idx->dev.n_docs)
    return mgx::Fail(MGX_ERR_OUT_OF_RANGE, "mgx_index_read_text: doc id outside the index range");
  MGX_HIP(hipSetDevice(idx->device));
  const uint32_t slot = doc_id - idx->dev.first_doc_id;
  uint64_t off[2] = {0, 0};
  MGX_HIP(hipMemcpy(off, idx->d_text_off.as<uint64_t>() + slot, 16, hipMemcpyDeviceToHost));
  *len = off[1] - off[0];
  if (*len == 0 || !text) return MGX_OK;
  if (capacity < *len) return mgx::Fail(MGX_ERR_OUT_OF_RANGE, "mgx_index_read_text: buffer too small (*len holds the size)");
  MGX_HIP(hipMemcpy(text, idx->d_text.as<uint8_t>() + off[0], *len, hipMemcpyDeviceToHost));
  return MGX_OK;
}

int mgx_index_filter_column_export(mgx_index* idx, uint32_t column_id, uint64_t* values, uint8_t* is_null, uint32_t* value_ids) {
  if (!idx || !values || !is_null) return mgx::Fail(MGX_ERR_INVALID_ARGUMENT, "mgx_index_filter_column_export: null argument");
  std::lock_guard<std::mutex> lock(idx->mu);
  if (column_id >= idx->filter_columns.size()) return mgx::Fail(MGX_ERR_OUT_OF_RANGE, "mgx_index_filter_column_export: unknown filter column");
  const mgx_index::FilterColumn& col = *idx->filter_columns[column_id];
  const uint64_t n = idx->dev.n_docs;
  MGX_HIP(hipSetDevice(idx->device));
  MGX_HIP(hipMemcpy(values, col.d_values.p, n * 8, hipMemcpyDeviceToHost));
  if (col.d_null.p) MGX_HIP(hipMemcpy(is_null, col.d_null.p, n, hipMemcpyDeviceToHost));
  else std::memset(is_null, 0, n);
  if (value_ids) {
    if (col.d_value_ids.p) MGX_HIP(hipMemcpy(value_ids, col.d_value_ids.p, n * 4, hipMemcpyDeviceToHost));
    else std::memset(value_ids, 0xFF, n * 4);
  }
  return MGX_OK;
}

int mgx_index_filter_column_read(mgx_index* idx, uint32_t column_id, uint32_t doc_id, uint64_t* value_bits, int* is_null,
                                 uint32_t* value_id) {
  if (!idx || !value_bits || !is_null) return mgx::Fail(MGX_ERR_INVALID_ARGUMENT, "mgx_index_filter_column_read: null argument");
  std::lock_guard<std::mutex> lock(idx->mu);
  if (column_id >= idx->filter_columns.size()) return mgx::Fail(MGX_ERR_OUT_OF_RANGE, "mgx_index_filter_column_read: unknown filter column");
  if (doc_id < idx->dev.first_doc_id || doc_id - idx->dev.first_doc_id >= idx->dev.n_docs)
    return mgx::Fail(MGX_ERR_OUT_OF_RANGE, "mgx_index_filter_column_read: doc id outside the index range");
  const uint32_t slot = doc_id - idx->dev.first_doc_id;
  const mgx_index::FilterColumn& col = *idx->filter_columns[column_id];
  MGX_HIP(hipSetDevice(idx->device));
  uint8_t nul = 0;
  uint32_t vid = 0xFFFFFFFFu;
  MGX_HIP(hipMemcpy(value_bits, col.d_values.as<uint64_t>() + slot, 8, hipMemcpyDeviceToHost));
  if (col.d_null.p) MGX_HIP(hipMemcpy(&nul, col.d_null.as<uint8_t>() + slot, 1, hipMemcpyDeviceToHost));
  if (col.d_value_ids.p) MGX_HIP(hipMemcpy(&vid, col.d_value_ids.as<uint32_t>() + slot, 4, hipMemcpyDeviceToHost));
  *is_null = nul ? 1 : 0;
  if (value_id) *value_id = vid;
  return MGX_OK;
}

int mgx_index_clear_postings(mgx_index* idx, const uint32_t* docids, const uint32_t* gram_ids, uint64_t n) {
  if (!idx || (n && (!docids || !gram_ids))) return mgx::Fail(MGX_ERR_INVALID_ARGUMENT, "mgx_index_clear_postings: null argument");
  if (n > 0xFFFFFFFFull) return mgx::Fail(MGX_ERR_OUT_OF_RANGE, "mgx_index_clear_postings: too many postings in one call");
  try {
    std::vector<uint32_t> slots, rows;
    for (uint64_t i = 0; i < n; ++i) {
      if (docids[i] < idx->dev.first_doc_id || docids[i] - idx->dev.first_doc_id >= idx->dev.n_docs)
        return mgx::Fail(MGX_ERR_OUT_OF_RANGE, "mgx_index_clear_postings: doc id outside the index range");
      if (gram_ids[i] >= idx->n_grams) return mgx::Fail(MGX_ERR_OUT_OF_RANGE, "mgx_index_clear_postings: unknown gram id");
      const uint32_t row = idx->h_bm_row[gram_ids[i]];
      if (row == mgx::kNoRow) continue;  // (a list-form gram: its queries keep the live-row operand)
      slots.push_back(docids[i] - idx->dev.first_doc_id);
      rows.push_back(row);
    }
    if (slots.empty()) return MGX_OK;
    std::lock_guard<std::mutex> lock(idx->mu);
    MGX_HIP(hipSetDevice(idx->device));
    DevBuf d_slots, d_rows;
    MGX_HIP(mgx::Upload(d_slots, slots.data(), slots.size()));
    MGX_HIP(mgx::Upload(d_rows, rows.data(), rows.size()));
    MGX_LAUNCH(mgx::LaunchClearGramBits(idx->d_gram_bitmaps.as<uint64_t>(), idx->dev.gb_tile_stride, idx->dev.gb_row_stride,
                                        d_slots.as<uint32_t>(), d_rows.as<uint32_t>(), static_cast<uint32_t>(slots.size()),
                                        idx->stream));
    MGX_HIP(hipStreamSynchronize(idx->stream));
    return MGX_OK;
  } catch (const std::exception& e) {
    return mgx::Fail(MGX_ERR_INTERNAL, std::string("mgx_index_clear_postings: ") + e.what());
  }
}

int mgx_index_set_live_bitmap(mgx_index* idx, uint32_t bitmap_id, int enable) {
  if (!idx) return mgx::Fail(MGX_ERR_INVALID_ARGUMENT, "mgx_index_set_live_bitmap: null index");
  std::lock_guard<std::mutex> lock(idx->mu);
  if (enable && bitmap_id >= idx->n_filter_rows)
    return mgx::Fail(MGX_ERR_OUT_OF_RANGE, "mgx_index_set_live_bitmap: unknown bitmap id");
  idx->live_row.store(enable ? bitmap_id : mgx::kNoRow);
  idx->bitmaps_clean.store(enable == MGX_LIVE_BITMAPS_CLEAN);
  std::lock_guard<std::mutex> tl(idx->table_mu);
  idx->df_cache.clear();
  return MGX_OK;
}

int mgx_index_set_doc_map(mgx_index* idx, const uint32_t* table_ids, uint64_t n) {
  if (!idx || !table_ids) return mgx::Fail(MGX_ERR_INVALID_ARGUMENT, "mgx_index_set_doc_map: null argument");
  if (n != idx->dev.n_docs) return mgx::Fail(MGX_ERR_INVALID_ARGUMENT, "mgx_index_set_doc_map: one id per doc slot of the index");
  for (uint64_t i = 1; i < n; ++i)
    if (table_ids[i] <= table_ids[i - 1])
      return mgx::Fail(MGX_ERR_INVALID_ARGUMENT, "mgx_index_set_doc_map: ids must ascend with the slot (rank order is kept by that)");
  try {
    std::lock_guard<std::mutex> lock(idx->mu);
    MGX_HIP(hipSetDevice(idx->device));
    if (idx->has_pkeys && idx->pk_any_missing)
      return mgx::Fail(MGX_ERR_INVALID_ARGUMENT, "mgx_index_set_doc_map: the index holds primary keys that fell back to "
                                                 "doc ids: set the doc map before mgx_index_set_primary_keys");
    MGX_HIP(mgx::Upload(idx->d_doc_map, table_ids, n));
    idx->h_doc_map.assign(table_ids, table_ids + n);
    idx->has_doc_map.store(true, std::memory_order_release);
    return MGX_OK;
  } catch (const std::exception& e) {
    return mgx::Fail(MGX_ERR_INTERNAL, std::string("mgx_index_set_doc_map: ") + e.what());
  }
}

int mgx_index_set_primary_keys(mgx_index* idx, const uint8_t* bytes, const uint64_t* off, const uint8_t* has_key) {
  if (!idx || !off) return mgx::Fail(MGX_ERR_INVALID_ARGUMENT, "mgx_index_set_primary_keys: null argument");
  const uint64_t n = idx->dev.n_docs;
  for (uint64_t i = 0; i < n; ++i)
    if (off[i + 1] < off[i]) return mgx::Fail(MGX_ERR_INVALID_ARGUMENT, "mgx_index_set_primary_keys: offsets must ascend");
  if (off[n] != off[0] && !bytes) return mgx::Fail(MGX_ERR_INVALID_ARGUMENT, "mgx_index_set_primary_keys: null key bytes");
  try {
    std::lock_guard<std::mutex> lock(idx->mu);
    MGX_HIP(hipSetDevice(idx->device));
    const mgx::pkey::KeyColumn col = mgx::pkey::BuildKeyColumn(
        bytes, off, has_key, n, idx->h_doc_map.empty() ? nullptr : idx->h_doc_map.data(), idx->dev.first_doc_id);
    if (idx->has_pkeys) MGX_HIP(hipDeviceSynchronize());  // (a replaced column may still be read by a fetch's kernels)
    MGX_HIP(mgx::Upload(idx->d_pk_values, col.values.data(), n));
    idx->d_pk_off.Free();
    idx->d_pk_bytes.Free();
    if (col.kind == mgx::pkey::kKeyRanks) {
      MGX_HIP(mgx::Upload(idx->d_pk_off, col.off.data(), col.off.size()));
      // (one byte of padding: an index whose only key is "" has an empty dictionary and still needs an address)
      const std::vector<uint8_t> pad(1, 0);
      MGX_HIP(mgx::Upload(idx->d_pk_bytes, col.bytes.empty() ? pad.data() : col.bytes.data(), std::max<size_t>(1, col.bytes.size())));
    }
    idx->pk_kind = col.kind;
    idx->pk_any_missing = col.any_missing;
    idx->has_pkeys = true;
    idx->pk_monotone.store(col.monotone, std::memory_order_release);
    return MGX_OK;
  } catch (const std::exception& e) {
    return mgx::Fail(MGX_ERR_INTERNAL, std::string("mgx_index_set_primary_keys: ") + e.what());
  }
}

int mgx_index_set_primary_key_shortcut(mgx_index* idx, int enable) {
  if (!idx) return mgx::Fail(MGX_ERR_INVALID_ARGUMENT, "mgx_index_set_primary_key_shortcut: null index");
  idx->pk_shortcut.store(enable != 0, std::memory_order_relaxed);
  return MGX_OK;
}

int mgx_index_attach_primary_key_bytes(mgx_index* idx, const uint8_t* bytes, const uint64_t* off, const uint8_t* has_key) {
  if (!idx || !off) return mgx::Fail(MGX_ERR_INVALID_ARGUMENT, "mgx_index_attach_primary_key_bytes: null argument");
  const uint64_t n = idx->dev.n_docs;
  uint64_t longest = 0;
  for (uint64_t i = 0; i < n; ++i) {
    if (off[i + 1] < off[i]) return mgx::Fail(MGX_ERR_INVALID_ARGUMENT, "mgx_index_attach_primary_key_bytes: offsets must ascend");
    if (!has_key || has_key[i]) longest = std::max(longest, off[i + 1] - off[i]);
  }
  if (off[n] != off[0] && !bytes) return mgx::Fail(MGX_ERR_INVALID_ARGUMENT, "mgx_index_attach_primary_key_bytes: null key bytes");
  if (longest > 0x7FFFFF00ull) return mgx::Fail(MGX_ERR_OUT_OF_RANGE, "mgx_index_attach_primary_key_bytes: a key exceeds 2 GiB");
  try {
    std::lock_guard<std::mutex> lock(idx->mu);
    MGX_HIP(hipSetDevice(idx->device));
    if (idx->has_pk_bytes) MGX_HIP(hipDeviceSynchronize());  // (the replaced bytes may still be read by a batch's kernel)
    // the offsets are kept relative to the first key's, the bytes from there (one byte of padding: an index whose keys
    // are all empty still needs an address)
    std::vector<uint64_t> rel(n + 1);
    for (uint64_t i = 0; i <= n; ++i) rel[i] = off[i] - off[0];
    const std::vector<uint8_t> pad(1, 0);
    MGX_HIP(mgx::Upload(idx->d_pkb_off, rel.data(), rel.size()));
    MGX_HIP(mgx::Upload(idx->d_pkb_bytes, rel[n] ? bytes + off[0] : pad.data(), std::max<size_t>(1, rel[n])));
    idx->d_pkb_has.Free();
    if (has_key) MGX_HIP(mgx::Upload(idx->d_pkb_has, has_key, n));
    idx->max_pk_bytes = static_cast<uint32_t>(longest);
    idx->has_pk_bytes = true;
    return MGX_OK;
  } catch (const std::exception& e) {
    return mgx::Fail(MGX_ERR_INTERNAL, std::string("mgx_index_attach_primary_key_bytes: ") + e.what());
  }
}

int mgx_index_max_primary_key_bytes(mgx_index* idx, uint32_t* out) {
  if (!idx || !out) return mgx::Fail(MGX_ERR_INVALID_ARGUMENT, "mgx_index_max_primary_key_bytes: null argument");
  std::lock_guard<std::mutex> lock(idx->mu);
  *out = idx->has_pk_bytes ? idx->max_pk_bytes : 0;
  return MGX_OK;
}

int mgx_index_invalidate_statistics(mgx_index* idx) {
  if (!idx) return mgx::Fail(MGX_ERR_INVALID_ARGUMENT, "mgx_index_invalidate_statistics: null index");
  MGX_HIP(hipSetDevice(idx->device));
  MGX_HIP(hipDeviceSynchronize());  // nothing in flight reads the tables that go
  std::lock_guard<std::mutex> lock(idx->table_mu);
  idx->table_slot.clear();
  idx->table_used = 0;
  idx->pending_jobs.clear();
  idx->norm_tables.clear();
  idx->block_max.clear();
  idx->df_cache.clear();
  return MGX_OK;
}

int mgx_index_synchronize(mgx_index* idx) {
  if (!idx) return mgx::Fail(MGX_ERR_INVALID_ARGUMENT, "mgx_index_synchronize: null index");
  MGX_HIP(hipSetDevice(idx->device));
  MGX_HIP(hipDeviceSynchronize());
  return MGX_OK;
}

}  // extern "C"

// =================================================================================================================
// batch
// =================================================================================================================

struct mgx_batch {
  mgx_index* idx = nullptr;
  std::unique_ptr<mgx::BatchResources> res_owned;  // kept across mgx_batch_reset
  mgx::BatchResources* res = nullptr;              // = res_owned.get(), or the index's single-operator resources
  uint32_t n_queries = 0;
  std::vector<mgx::QuerySpec> specs;
  // One launch of a group: the group's descriptor with the items of one route (mgx::Route), in launch order
  struct RouteLaunch {
    mgx::DevBatch dev{};
    DevBuf d_items;
  };
  // per mode: the queries of that mode, in batch order
  struct Group {
    std::vector<uint32_t> qids;  // batch index of each member
    mgx::DevBatch dev{};         // queries, tables and outputs, without items: every RouteLaunch adds its own
    mgx::LdsPlan plan{};
    mgx::WavePlan wplan{};
    // The routes' launches run over disjoint item lists into the same outputs.
    RouteLaunch block;           // general kernel
    uint32_t n_items_plain = 0;  // block items [0, n_items_plain): queries of bitmap-form operands only (LaunchTileEval)
    uint32_t n_items_fz = 0;     // the last n_items_fz block items: queries with kOpVerifyFuzzy / kOpVerifyTree (a launch of their own)
    // wave kernel: flat programs (score mode: dense or sparse scored operands, contribution tables in d_tables)
    RouteLaunch wave;
    DevBuf d_tables;
    // score mode: wave-kernel queries with a sorted-list operand (bigger LDS plan, launched beside the others)
    mgx::WavePlan wplan_lists{};
    RouteLaunch wave_lists;
    // score mode, fast path (bitmap_score_kernel<T>): resolved query descriptors and one launch per number of scored terms
    mgx::FastPlan fplan{};
    RouteLaunch fast[mgx::kFastMaxScore];
    uint32_t n_seed_fast[mgx::kFastMaxScore] = {0, 0, 0, 0, 0};  // seed items at the front of fast[t]
    uint32_t seed_k = 0;       // keys per query in the seed-bound exchange (0: none; rank-independent, see ScheduleItems)
    uint64_t seed_table_docs = 0;  // table-wide doc count of those queries (BM25 N): the exchange pays on large shards only
    DevBuf d_has_seed;         // [n] u8: the query's first candidate list is a seed item's
    DevBuf d_fast_queries;
    // selective flat queries (a sparse posting list drives: cand_kernel), score and docid-page groups
    RouteLaunch cand;
    DevBuf d_cand_skip;  // [n] u8: the query is candidate-driven (docid-page group)
    uint32_t cand_leaves = 0, cand_instr = 0, cand_cap = 0;
    // SORT _score over long sorted posting arrays (merge_score_kernel: the driver's tile segments against staged bitmaps)
    RouteLaunch merge;
    uint32_t merge_leaves = 0, merge_instr = 0, merge_ops = 0, merge_cap = 0;
    // docid-page group: the page pass runs one workgroup per query; flat programs on the wave kernel
    RouteLaunch page_wave, page_block;
    uint32_t n_page_fz = 0;  // the same as n_items_fz at the end of page_block
    DevBuf d_queries, d_leaves, d_prog, d_score, d_explicit, d_counters, d_ident, d_list_begin;
    std::vector<unsigned long long> h_counters;
  };
  Group score, bitmap;
  // df pass of the text-level scored terms: one kModeTextDf query per term (the AND of its grams + a text scan)
  Group textdf;
  std::vector<mgx::QuerySpec> df_specs;
  DevBuf d_patterns, d_text_terms, d_text_idf, d_text_df, d_verify_terms, d_verify_prog;
  // d_text_df is the array ranks all-reduce in place (table-wide df after the reduction); d_text_df_local keeps this
  // shard's own counts — the only thing the index's df cache ever holds, so what a rank contributes to the reduction is
  // the same whether a term's count came from the cache or from the df pass
  DevBuf d_text_df_local, d_text_df_known;
  std::vector<uint64_t> h_text_df, h_text_df_local, text_total_docs;
  std::vector<uint64_t> text_df_known;      // per text term: its cached LOCAL df, or ~0ull (the df query then counts it)
  std::vector<std::string> text_df_key;     // per text term: the cache key
  std::vector<double> h_text_idf;
  // the batch's distinct conditions, sorted by column, and the columns' groups (filter_compare_batch_kernel); their rows
  // live in res->cond
  DevBuf d_cond_groups, d_conds;
  uint32_t n_cond_groups = 0;
  uint64_t* cond_arena = nullptr;
  bool df_ready = false;  // mgx_batch_count_df ran (and the caller summed the counts) for the next execute
  // score group outputs
  DevBuf d_cand_keys, d_cand_docs, d_cand_n;
  // This shard's merged top-(offset+limit) per query in the exchange layout of mgx_batch_export_topk, written in place
  // by the merge kernel: [keys n*S u64 | totals n u64 | docs n*S u32 | counts n u32]  (S = top_stride)
  DevBuf d_export;
  size_t ex_off32 = 0, ex_bytes = 0;
  uint64_t* ex_keys() const { return d_export.as<uint64_t>(); }
  uint64_t* ex_totals(size_t n) const { return d_export.as<uint64_t>() + n * top_stride; }
  uint32_t* ex_docs() const { return reinterpret_cast<uint32_t*>(static_cast<char*>(d_export.p) + ex_off32); }
  uint32_t* ex_counts(size_t n) const { return ex_docs() + n * top_stride; }
  // Everything mgx_batch_fetch needs from a score group sits in ONE device block, copied with one async memcpy into
  // pinned host memory: [counters n*9 u64 | total_override n u64 | page_scores n*L f64 | page_docs n*L u32 | page_n n u32]
  DevBuf d_score_out;
  void* h_score_out = nullptr;  // pinned (BatchResources)
  size_t so_override = 0, so_scores = 0, so_docs = 0, so_n = 0, so_bytes = 0;
  unsigned long long* sc_counters() const { return d_score_out.as<unsigned long long>(); }
  uint64_t* sc_override() const { return reinterpret_cast<uint64_t*>(static_cast<char*>(d_score_out.p) + so_override); }
  double* sc_scores() const { return reinterpret_cast<double*>(static_cast<char*>(d_score_out.p) + so_scores); }
  uint32_t* sc_docs() const { return reinterpret_cast<uint32_t*>(static_cast<char*>(d_score_out.p) + so_docs); }
  uint32_t* sc_n() const { return reinterpret_cast<uint32_t*>(static_cast<char*>(d_score_out.p) + so_n); }
  uint32_t top_stride = 0, page_stride = 0;
  bool merged_shards = false;
  // bitmap group outputs
  DevBuf d_rbits, d_tile_cnt, d_tile_start, d_totals, d_take, d_out_off, d_reverse;
  // mutable tables (mgx_batch_merge_local): the bitmap group's sizes are known only at fetch time, so the merge of that
  // group runs inside mgx_batch_fetch(primary). merge_other: on the primary, the batch whose bitmap-group queries the
  // fetch merges in; merged_away: on that other batch, its bitmap-group pages went into the primary's result.
  mgx_batch* merge_other = nullptr;
  bool merged_away = false;
  hipStream_t merge_stream = nullptr;
  DevBuf d_merge;  // scratch of the bitmap group's fetch: runs, keys, page, run descriptors (grown, never shrunk)
  // docid-page group (kModeDocPage): per-tile counts / rank offsets, and one packed result block
  // [counters n*8 u64 | totals n u64 | page docs n*stride u32] mirrored in pinned host memory
  Group page;
  DevBuf d_ptile_cnt, d_ptile_start, d_page_out, d_page_scratch;
  void* h_page_out = nullptr;
  size_t po_totals = 0, po_docs = 0, po_bytes = 0;
  uint32_t doc_page_stride = 0;
  // HIGHLIGHT (mgx_batch_set_highlight): the highlighted queries' descriptors, their terms, and the records the kernel
  // fills, one per (highlighted query, page entry), copied to pinned memory behind the page
  struct Highlight {
    std::vector<mgx::DevHlQuery> queries;  // in batch order
    std::vector<int32_t> of_query;         // batch query -> index into `queries`, or -1
    DevBuf d_queries, d_terms, d_patterns, d_arena;
    void* h_arena = nullptr;  // pinned (BatchResources)
    size_t bytes = 0;
    uint32_t n_entries = 0;
    bool defer = false;  // mgx_batch_defer_highlight: mgx_batch_merge_local runs the kernel, execute does not
    std::vector<mgx_highlight_entry> entries;  // of the last fetch
    bool on() const { return !queries.empty(); }
  };
  Highlight hl;
  // FACET in a batch (mgx_batch_set_facets): the plan of mgx_facet.hpp, its descriptors on the device, and the counts
  // facet_batch_kernel fills behind the bitmap group, copied to pinned memory with the batch's results
  struct Facets {
    mgx::facet::Plan plan;
    std::vector<int32_t> of_query;  // batch query -> index into plan.queries, or -1
    DevBuf d_queries, d_columns, d_items, d_counts;
    void* h_counts = nullptr;  // pinned (BatchResources)
    std::vector<mgx_facet_entry> entries;  // of the last fetch
    bool on() const { return !plan.queries.empty(); }
    bool faceted(uint32_t qi) const { return on() && of_query[qi] >= 0; }
  };
  Facets fc;
  // Page documents (mgx_batch_set_documents): the plan of mgx_documents.hpp, the requested columns of the batch's own
  // index, and the records document_gather_kernel fills behind the kernel that finalises each page
  struct Documents {
    mgx::documents::Plan plan;
    std::vector<int32_t> of_query;  // batch query -> index into plan.queries, or -1
    std::vector<mgx::documents::DevQuery> early;  // the score / doc-page group's queries, in request order
    std::vector<mgx::documents::DevQuery> late;   // the bitmap group's, built where its pages are cut
    DevBuf d_early, d_columns, d_late, d_arena;
    void* h_arena = nullptr;  // pinned (BatchResources)
    std::vector<uint64_t> fetch_off;  // per plan query: where the last fetch's records begin in h_arena
    bool defer = false;  // mgx_batch_defer_documents: mgx_batch_merge_local runs the kernel, execute does not
    std::vector<mgx_document_entry> entries;  // of the last fetch
    bool on() const { return !plan.queries.empty(); }
    bool requested(uint32_t qi) const { return on() && of_query[qi] >= 0; }
  };
  Documents doc;
  bool fetched = false;  // mgx_batch_fetch assembled h_results for the last execute
  // host results
  std::vector<mgx_query_result> h_results;
  std::vector<uint32_t> h_docs;
  std::vector<double> h_scores;
  bool executed = false;
  hipStream_t last_stream = nullptr;
  // kernel timing
  bool timing = false;
  std::vector<std::pair<hipEvent_t, hipEvent_t>> events;
  uint64_t list_bytes = 0;
};

namespace mgx {

// MGX_TRACE_HOST: where a batch's host time goes (microseconds per section, printed by mgx_batch_reset every 64 batches)
constexpr int kSections = 7;
static std::atomic<uint64_t> g_section_us[kSections];
static const char* const kSectionNames[kSections] = {"queries+leaves", "routes", "table uploads", "result blocks",
                                                      "items", "launch order", "descriptors+items"};
struct SectionTimer {
  static bool On() {
    static const bool on = std::getenv("MGX_TRACE_HOST") != nullptr;
    return on;
  }
  std::chrono::steady_clock::time_point t;
  SectionTimer() { if (On()) t = std::chrono::steady_clock::now(); }
  void Mark(int section) {
    if (!On()) return;
    const auto now = std::chrono::steady_clock::now();
    g_section_us[section] += std::chrono::duration_cast<std::chrono::nanoseconds>(now - t).count();
    t = now;
  }
};

using Group = mgx_batch::Group;
using RouteLaunch = mgx_batch::RouteLaunch;

// The kernel path of one query of a group (each route has its own item list and launch)
enum class Route : uint8_t {
  kBlock,      // tile_eval_kernel, the general workgroup kernel
  kWave,       // wave_score_kernel (score), wave_count_kernel + wave_page_kernel (docid page, df)
  kWaveLists,  // wave_score_lists_kernel: score-mode wave queries with a sorted-list operand
  kFast,       // bitmap_score_kernel<T>, T = the number of scored terms
  kCand,       // cand_kernel: a sparse posting list drives, the rest is probed per candidate
  kMerge,      // merge_score_kernel: a long driver's tile segments against staged bitmaps
};

static bool EnvZero(const char* name) { return std::getenv(name) && atoi(std::getenv(name)) == 0; }
// Which kernel paths a group may take, read on every UploadGroup call (tests flip them inside one process).
// MGX_FORCE_BLOCK_KERNEL puts every query on the general kernel.
struct PathSwitches {
  const bool wave = std::getenv("MGX_FORCE_BLOCK_KERNEL") == nullptr;
  const bool fast = wave && !EnvZero("MGX_FAST_PATH"), cand = wave && !EnvZero("MGX_CAND");
  const bool merge = wave && !EnvZero("MGX_MERGE");
};

// A group's host-side plan, filled by UploadGroup's steps in order.
struct GroupPlan {
  GroupPlan(uint32_t n_, uint32_t mode)
      : n(n_), score_mode(mode == kModeScore), df_mode(mode == kModeTextDf), page_mode(mode == kModeDocPage) {}
  const uint32_t n;
  const bool score_mode, df_mode, page_mode;
  std::vector<DevQuery> dq;  // (a) the DevQuery rows and the pools they index
  std::vector<DevLeaf> leaves;
  std::vector<uint32_t> prog;
  std::vector<DevScoreTerm> score;
  std::vector<uint32_t> expl;
  uint32_t max_limit = 1, max_needed = 1;  // the largest page, and offset + limit, of the group's queries
  std::vector<Route> route;  // (b) each query's route, and what it resolved ([n] or empty)
  std::vector<DevFastQuery> fastq;
  std::vector<uint64_t> wave_tables;  // [n][kWaveScoreSlots] the scored terms' contribution tables (score-mode wave)
  std::vector<uint32_t> cand_driver;
  std::vector<DevItem> items;  // (d) grouped by query, (e) in launch order; query i's lists [list_begin[i], list_begin[i + 1])
  std::vector<uint32_t> list_begin, item_begin;
  std::vector<DevItem> block, wave, wave_lists, fast[kFastMaxScore], cand, merge;  // (e) each route's, in launch order
  std::vector<uint8_t> seed_cut;  // (d) [n] the query's first item is a seed item
  std::vector<uint8_t> has_seed;
};

// (a) DevQuery rows, the leaf / program / score / explicit-id pools they index, and the general kernel's LDS plan.
static int LayOutQueries(mgx_batch* b, Group& g, const std::vector<QuerySpec>& specs, GroupPlan& p) {
  std::vector<DevLeaf>& leaves = p.leaves;
  std::vector<uint32_t>& expl = p.expl;
  p.dq.resize(p.n);
  uint32_t max_leaves = 0, max_lds_leaves = 0, max_score = 0, max_stack = 0, max_instr = 0, max_cap = 64;
  for (uint32_t i = 0; i < p.n; ++i) {
    const QuerySpec& s = specs[g.qids[i]];
    DevQuery& q = p.dq[i];
    std::memset(&q, 0, sizeof(q));
    q.leaf_begin = static_cast<uint32_t>(leaves.size());
    q.n_leaves = static_cast<uint32_t>(s.leaves.size());
    q.prog_begin = static_cast<uint32_t>(p.prog.size());
    q.n_instr = static_cast<uint32_t>(s.prog.size());
    q.score_begin = static_cast<uint32_t>(p.score.size());
    q.n_score = static_cast<uint32_t>(s.score.size());
    q.mode = s.mode;
    q.limit = s.limit;
    q.offset = s.offset;
    // (offset + limit fits 32 bits only where it is bounded: score mode enforces needed <= kMaxNeeded; docid pages
    // carry limit alone — a caller's SearchAnd(terms, UINT32_MAX) must not wrap, nor spin a doubling loop forever)
    q.needed = static_cast<uint32_t>(std::min<uint64_t>(static_cast<uint64_t>(s.offset) + s.limit, 0xFFFFFFFFull));
    uint32_t cap = 64;
    if (s.mode == kModeScore)
      while (cap < q.needed && cap < (1u << 30)) cap <<= 1;
    q.cap = cap;
    q.descending = s.reverse;
    q.stack_depth = s.stack_depth;
    q.out_slot = i;
    q.pat_off = s.pat_off;
    q.pat_len = s.pat_len;
    q.vt_begin = s.vt_begin;
    q.vt_count = static_cast<uint32_t>(s.verify_patterns.size());
    q.fz_distance = s.fz_distance;
    q.vp_begin = s.vp_begin;
    q.k1 = s.k1;
    q.b = s.b;
    q.one_minus_b = 1.0 - s.b;
    q.k1_plus_1 = s.k1 + 1.0;
    q.avgdl_clamped = std::max(s.avgdl, 1.0);  // bm25_scorer.cpp:81
    const uint32_t ebase = static_cast<uint32_t>(expl.size());
    // LDS residency (general kernel): sorted-list operands are scattered into an LDS bitmap, scored operands are
    // probed there by other threads; bitmap-form operands are read straight from HBM and take no LDS
    uint32_t n_lds = 0;
    for (size_t li = 0; li < s.leaves.size(); ++li) {
      DevLeaf lf = s.leaves[li];
      if (lf.kind == kLeafExplicit) lf.a += ebase;
      bool resident = lf.kind == kLeafList || lf.kind == kLeafExplicit;
      for (const DevScoreTerm& st : s.score) resident = resident || st.leaf == li;
      lf.lds = resident ? n_lds++ : kNoRow;
      leaves.push_back(lf);
    }
    if (n_lds > kMaxLdsLeaves)
      return Fail(MGX_ERR_NOT_IMPLEMENTED,
                  "query " + std::to_string(g.qids[i]) + ": more than 64 sorted-list / scored operands in one query");
    max_lds_leaves = std::max(max_lds_leaves, n_lds);
    p.prog.insert(p.prog.end(), s.prog.begin(), s.prog.end());
    p.score.insert(p.score.end(), s.score.begin(), s.score.end());
    expl.insert(expl.end(), s.explicit_ids.begin(), s.explicit_ids.end());
    while (expl.size() % 4) expl.push_back(0xFFFFFFFFu);
    max_leaves = std::max(max_leaves, q.n_leaves);
    max_score = std::max(max_score, q.n_score);
    max_stack = std::max(max_stack, q.stack_depth);
    max_instr = std::max(max_instr, q.n_instr);
    max_cap = std::max(max_cap, q.cap);
    p.max_limit = std::max(p.max_limit, q.limit);
    p.max_needed = std::max(p.max_needed, q.needed);
    if (!p.df_mode) b->list_bytes += 4 * s.list_postings;
  }
  g.plan = PlanLds(max_leaves, max_lds_leaves, max_score, max_stack, max_instr, max_cap, p.score_mode || p.df_mode);
  return MGX_OK;
}

// Fast path: the query's resolved bitmap_score_kernel descriptor; false when the query does not fit the path.
static bool ResolveFast(mgx_index* idx, const uint64_t* cond_arena, const QuerySpec& s, const DevQuery& q, DevFastQuery* out) {
  DevFastQuery& f = *out;
  for (uint32_t ins : s.prog) {
    const uint32_t op = ins >> 24, arg = ins & 0xFFFFFFu;
    if (op == kOpCount) {
      if (f.n_ops == 0) return false;
      f.ops[f.n_ops - 1].code |= arg << 8;
      continue;
    }
    const DevLeaf& lf = s.leaves[arg];
    if (f.n_ops == static_cast<uint32_t>(kFastMaxOps) || (op == kOpLoad) != (f.n_ops == 0)) return false;
    FastOp o{};
    uint64_t stride = 0;
    if (lf.kind == kLeafGramBitmap) {
      o.base = reinterpret_cast<uint64_t>(idx->dev.gram_bitmaps + static_cast<uint64_t>(lf.b) * idx->dev.gb_row_stride);
      stride = idx->dev.gb_tile_stride * 8;
    } else if (lf.kind == kLeafFilterBitmap) {  // rows are appended at run time and may move: relative to the base
      o.base = static_cast<uint64_t>(lf.b) * idx->dev.fb_row_stride * 8;
      stride = idx->dev.fb_tile_stride * 8;
      o.code |= 16u;
    } else if (lf.kind == kLeafCondBitmap) {  // the batch's arena stays where it is for as long as the batch is prepared
      o.base = reinterpret_cast<uint64_t>(cond_arena + static_cast<uint64_t>(lf.b) * idx->dev.fb_row_stride);
      stride = idx->dev.fb_tile_stride * 8;
    } else {
      return false;
    }
    if (stride > 0xFFFFFFFFull) return false;
    o.tile_stride = static_cast<uint32_t>(stride);
    o.code |= (op == kOpLoad || op == kOpOr) ? kFastOr : op == kOpAnd ? kFastAnd : kFastAndNot;
    f.ops[f.n_ops++] = o;
  }
  if (f.n_ops == 0) return false;
  for (size_t t = 0; t < s.score.size(); ++t) {
    const DevLeaf& lf = s.leaves[s.score[t].leaf];
    if (lf.kind != kLeafGramBitmap) return false;
    FastScore& fs = f.score[t];
    fs.nib = reinterpret_cast<uint64_t>(idx->dev.tfnib + static_cast<uint64_t>(lf.b) * idx->dev.nib_row_stride);
    fs.idf = s.score[t].idf;
    fs.gram = lf.a;
    fs.skip_row = lf.row;
  }
  if (s.reverse != 0) {  // SORT _score DESC: top-k pruning by block-max bounds
    double step = 0.0;
    f.blockmax = GetBlockMax(idx, s.k1, s.b, s.avgdl, &step, &f.blockmax_fine);
    if (f.blockmax) {
      f.bm_tile_stride = idx->n_bitmap_rows * 256u;
      f.bmf_tile_stride = idx->n_fine_rows * 1024u;
      // integer form of the bound: unit = step * (largest idf / 255); W_i = ceil(idf_i / (largest idf / 255))
      double idf_max = 0.0;
      for (size_t t = 0; t < s.score.size(); ++t) idf_max = std::max(idf_max, s.score[t].idf);
      const double wunit = idf_max > 0.0 ? idf_max * (1.0 + 0x1p-40) / 255.0 : 1.0;
      f.bm_inv_unit = 1.0 / (wunit * step);
      f.bm_wpack = f.bm_w4 = f.bm_cint = 0;
      for (size_t t = 0; t < s.score.size(); ++t) {
        const uint32_t w = static_cast<uint32_t>(std::min(255.0, std::ceil(s.score[t].idf / wunit)));
        if (t < 4) f.bm_wpack |= w << (8 * t); else f.bm_w4 = w;
      }
      for (size_t t = 0; t < s.score.size(); ++t) {
        const DevLeaf& lf = s.leaves[s.score[t].leaf];
        FastScore& fs = f.score[t];
        const uint32_t frow = f.blockmax_fine ? idx->h_fine_map[lf.b] : kNoRow;
        fs.bm_mode = frow != kNoRow ? 2u : 1u;
        fs.bm_off = frow != kNoRow ? frow * 1024u : lf.b * 256u;
      }
    }
  }
  f.n_score = static_cast<uint32_t>(s.score.size());
  f.needed = q.needed;
  f.cap = q.cap;
  f.descending = q.descending;
  f.k1 = q.k1;
  f.b = q.b;
  f.one_minus_b = q.one_minus_b;
  f.k1_plus_1 = q.k1_plus_1;
  f.avgdl_clamped = q.avgdl_clamped;
  return true;
}

// (b) score and docid-page groups, selective queries: candidate-driven (cand_kernel). The smallest positive operand
// drives when it is a sorted posting array (a gram too sparse for a bitmap row) that the program loads before its first
// COUNT — terms arrive smallest-first (search_pipeline.cpp:2012-2014), so that is a gram of the first term and every
// funnel counter is a count of candidates. Everything else of the query is probed per candidate.
static void RouteCandMerge(mgx_batch* b, Group& g, const std::vector<QuerySpec>& specs, const PathSwitches& sw,
                           GroupPlan& p) {
  static const uint64_t kMaxPerTile = std::getenv("MGX_CAND_MAX_PER_TILE") ? static_cast<uint64_t>(atoll(std::getenv("MGX_CAND_MAX_PER_TILE"))) : 64ull;
  const mgx_index* idx = b->idx;
  for (uint32_t i = 0; sw.cand && i < p.n; ++i) {
    const QuerySpec& s = specs[g.qids[i]];
    if (p.route[i] == Route::kFast || !s.flat || s.prog.empty()) continue;
    if (p.score_mode && (!s.fast_score_ok || s.score.empty())) continue;
    bool ok = true, counted = false;
    uint32_t driver = kNoLeaf;
    uint64_t best = ~0ull, longest_list = 0;
    for (size_t pc = 0; ok && pc < s.prog.size(); ++pc) {
      const uint32_t op = s.prog[pc] >> 24, arg = s.prog[pc] & 0xFFFFFFu;
      if (op == kOpCount) {
        counted = true;
        continue;
      }
      if ((op == kOpLoad) != (pc == 0) || (op != kOpLoad && op != kOpAnd && op != kOpAndNot)) { ok = false; break; }
      const DevLeaf& lf = s.leaves[arg];
      if (lf.kind != kLeafList && lf.kind != kLeafGramBitmap && !IsFilterKind(lf.kind)) { ok = false; break; }
      if (lf.kind == kLeafList) longest_list = std::max<uint64_t>(longest_list, idx->h_offsets[lf.a + 1] - idx->h_offsets[lf.a]);
      // any positive gram loaded before the first COUNT makes every counter a count of candidates; the smallest of them
      // drives (with terms in the reference's order that is the smallest gram of the whole query)
      if (op == kOpAndNot || IsFilterKind(lf.kind) || counted) continue;
      const uint64_t sz = idx->h_offsets[lf.a + 1] - idx->h_offsets[lf.a];
      if (sz < best) {
        best = sz;
        driver = arg;
      }
    }
    if (!ok || driver == kNoLeaf || s.leaves[driver].kind != kLeafList) continue;
    for (uint32_t ins : s.prog)  // NOT of the driver's own gram: the tile program handles it (the result is empty)
      if ((ins >> 24) == kOpAndNot && (ins & 0xFFFFFFu) == driver) ok = false;
    if (p.score_mode)
      for (const DevScoreTerm& st : s.score)
        ok = ok && st.leaf != kNoLeaf && (s.leaves[st.leaf].kind == kLeafList || s.leaves[st.leaf].kind == kLeafGramBitmap);
    if (!ok) continue;
    DevQuery& q = p.dq[i];
    // probing a LONG sorted list costs a binary search of its tile segment per candidate (14 dependent loads on a segment
    // of 16384): such operands are staged per tile instead (the merge kernel), whatever the driver's size
    const bool long_probe = longest_list > 8 * kMaxPerTile * idx->dev.n_tiles;
    if (best > kMaxPerTile * idx->dev.n_tiles || long_probe) {
      // a LONG driver: too many candidates to probe one by one — the tile-synchronous merge (SORT _score only; docid
      // pages of such queries stay on the counting kernels, which have no per-match work)
      uint32_t staged = 0;
      for (size_t li = 0; li < s.leaves.size(); ++li) staged += li != driver ? 1u : 0u;
      if (!p.score_mode || !sw.merge || staged > kMergeMaxOps || q.cap > 256) continue;
      q.pat_off = driver;  // (unused by score-mode queries otherwise: where the kernel finds its driver)
      p.route[i] = Route::kMerge;
      g.merge_leaves = std::max(g.merge_leaves, q.n_leaves);
      g.merge_instr = std::max(g.merge_instr, q.n_instr);
      g.merge_ops = std::max(g.merge_ops, staged);
      g.merge_cap = std::max(g.merge_cap, q.cap);
      continue;
    }
    if (p.cand_driver.empty()) p.cand_driver.assign(p.n, kNoLeaf);
    p.cand_driver[i] = driver;
    p.route[i] = Route::kCand;
    g.cand_leaves = std::max(g.cand_leaves, q.n_leaves);
    g.cand_instr = std::max(g.cand_instr, q.n_instr);
    g.cand_cap = std::max(g.cand_cap, q.cap);
  }
  if (CandLdsBytes(g.cand_leaves, g.cand_instr, p.score_mode ? g.cand_cap : 0) > 150 * 1024) {
    for (Route& r : p.route)
      if (r == Route::kCand) r = Route::kBlock;  // (a page of a thousand entries with many operands: the general kernel takes these)
    p.cand_driver.clear();
  }
  if (MergeLdsBytes(g.merge_leaves, g.merge_instr, g.merge_ops, g.merge_cap) > 150 * 1024)
    for (Route& r : p.route)
      if (r == Route::kMerge) r = Route::kBlock;
}

// (b) Every query's route: each path with its plan and its LDS-capacity fallback; then the shapes no kernel can hold.
static int ChooseRoutes(mgx_batch* b, Group& g, const std::vector<QuerySpec>& specs, const PathSwitches& sw,
                        GroupPlan& p) {
  mgx_index* idx = b->idx;
  p.route.assign(p.n, Route::kBlock);
  if (p.score_mode) {
    // fast path (bitmap_score_kernel): flat programs over bitmap-form operands, 1..5 scored terms that are dense
    // grams, a page of at most 128 entries, one (k1, b, avgdl) for the whole set (they are table constants)
    uint32_t fcap = 64;
    bool have_params = false;
    double pk1 = 0, pb = 0, pavg = 0;
    for (uint32_t i = 0; sw.fast && i < p.n; ++i) {
      const QuerySpec& s = specs[g.qids[i]];
      if (!s.flat || !s.fast_score_ok || s.score.empty() || s.score.size() > static_cast<size_t>(kFastMaxScore)) continue;
      if (p.dq[i].cap > 128) continue;
      if (have_params && (Bits(s.k1) != Bits(pk1) || Bits(s.b) != Bits(pb) || Bits(s.avgdl) != Bits(pavg))) continue;
      DevFastQuery f{};
      if (!ResolveFast(idx, b->cond_arena, s, p.dq[i], &f)) continue;
      if (!have_params) {
        pk1 = s.k1;
        pb = s.b;
        pavg = s.avgdl;
        have_params = true;
      }
      if (p.fastq.empty()) p.fastq.resize(p.n);
      p.fastq[i] = f;
      p.route[i] = Route::kFast;
      fcap = std::max(fcap, f.cap);
    }
    if (have_params) {
      const double* ktab = GetLengthNormTable(idx, pk1, pb, pavg);
      g.fplan = PlanFast(fcap, ktab);
      if (ktab == nullptr || g.fplan.bytes > 64 * 1024)
        for (Route& r : p.route) r = Route::kBlock;
    }

    // wave kernel: the remaining queries it can run, with their scored terms' contribution tables
    uint32_t wl = 0, wsc = 0, wi = 0, wc = 64;
    for (uint32_t i = 0; i < p.n; ++i) {
      if (p.route[i] == Route::kFast) continue;
      const QuerySpec& s = specs[g.qids[i]];
      bool ok = sw.wave && s.wave_ok;
      // scored terms: dense grams (tf nibbles by doc slot) or sparse ones (exact posting lookup per match)
      for (const DevScoreTerm& st : s.score)
        ok = ok && (s.leaves[st.leaf].kind == kLeafGramBitmap || s.leaves[st.leaf].kind == kLeafList);
      if (!ok) continue;
      // A sorted-list operand needs the per-wave scatter scratch (16 KB per workgroup: 2 instead of 3 workgroups per
      // CU), so queries with one are launched separately and the all-bitmap majority keeps the small LDS plan.
      // the scored terms' contribution tables come from the index's pool (a sparse gram has no bitmap row: its table is
      // keyed by the gram id above the bitmap rows); without one the query runs on the general kernel
      uint64_t tabs[kWaveScoreSlots] = {0, 0, 0};
      for (size_t t = 0; ok && t < s.score.size(); ++t) {
        const DevLeaf& lf = s.leaves[s.score[t].leaf];
        const uint32_t key = lf.kind == kLeafGramBitmap ? lf.b : 0x80000000u | lf.a;
        tabs[t] = GetContributionTable(idx, key, s.score[t].idf, s.k1, s.b, s.avgdl);
        ok = tabs[t] != 0;
      }
      if (!ok) continue;
      if (p.wave_tables.empty()) p.wave_tables.assign(static_cast<size_t>(p.n) * kWaveScoreSlots, 0);
      for (int t = 0; t < kWaveScoreSlots; ++t) p.wave_tables[static_cast<size_t>(i) * kWaveScoreSlots + t] = tabs[t];
      bool lists = false;
      for (const DevLeaf& lf : s.leaves) lists = lists || lf.kind == kLeafList || lf.kind == kLeafExplicit;
      p.route[i] = lists ? Route::kWaveLists : Route::kWave;
      wl = std::max<uint32_t>(wl, p.dq[i].n_leaves);
      wsc = std::max<uint32_t>(wsc, p.dq[i].n_score);
      wi = std::max<uint32_t>(wi, p.dq[i].n_instr);
      wc = std::max<uint32_t>(wc, p.dq[i].cap);
    }
    g.wplan = PlanWave(wl, wsc, wi, wc, idx->dev.max_doc_len, false);
    g.wplan_lists = PlanWave(wl, wsc, wi, wc, idx->dev.max_doc_len, true);
    if (g.wplan_lists.bytes > 160 * 1024)
      for (Route& r : p.route)
        if (r != Route::kFast) r = Route::kBlock;
  }
  if (p.page_mode || p.df_mode) {
    // flat programs count on the wave kernel (registers only, two tiles in flight per wave); the df pass of a
    // text-level term (always a flat AND of its grams) enumerates and scans its candidates there too
    uint32_t wl = 1, wi = 1;
    bool has_list = false;
    for (uint32_t i = 0; i < p.n; ++i) {
      const QuerySpec& s = specs[g.qids[i]];
      if (!(sw.wave && s.wave_ok)) continue;
      p.route[i] = Route::kWave;
      for (const DevLeaf& lf : s.leaves) has_list = has_list || lf.kind == kLeafList || lf.kind == kLeafExplicit;
      wl = std::max<uint32_t>(wl, p.dq[i].n_leaves);
      wi = std::max<uint32_t>(wi, p.dq[i].n_instr);
    }
    g.wplan = WavePlan{wl, 0, wi, 0, 0, has_list ? 1u : 0u, 0};
  }
  g.cand_leaves = g.cand_instr = g.cand_cap = 0;
  g.merge_leaves = g.merge_instr = g.merge_ops = g.merge_cap = 0;
  if (p.score_mode || p.page_mode) RouteCandMerge(b, g, specs, sw, p);
  if (g.plan.bytes > 160 * 1024)
    return Fail(MGX_ERR_NOT_IMPLEMENTED, "query shape exceeds the 160 KiB LDS of a CU");
  for (uint32_t i = 0; i < p.n; ++i)
    if (specs[g.qids[i]].fz_op && g.plan.bytes + kFzLdsBytes > 160 * 1024)
      return Fail(MGX_ERR_NOT_IMPLEMENTED, "query shape with the fuzzy text filter exceeds the 160 KiB LDS of a CU");
  return MGX_OK;
}

// (c) The query tables (section 2), then the result blocks of the group's mode and the identity query map.
static int UploadTables(mgx_batch* b, Group& g, const GroupPlan& p, SectionTimer& sec) {
  const uint32_t n = p.n;
  MGX_HIP(Upload(g.d_queries, p.dq.data(), p.dq.size()));
  MGX_HIP(Upload(g.d_leaves, p.leaves.data(), p.leaves.size()));
  MGX_HIP(Upload(g.d_prog, p.prog.data(), p.prog.size()));
  MGX_HIP(Upload(g.d_score, p.score.data(), p.score.size()));
  MGX_HIP(Upload(g.d_explicit, p.expl.data(), p.expl.size(), 4));
  sec.Mark(2);
  // [n][8] counters followed by [n] pruning bounds: one memset clears both before every execute
  if (p.score_mode) {
    const size_t max_limit = p.max_limit;
    b->so_override = static_cast<size_t>(n) * 9 * 8;
    b->so_scores = b->so_override + static_cast<size_t>(n) * 8;
    b->so_docs = b->so_scores + static_cast<size_t>(n) * max_limit * 8;
    b->so_n = b->so_docs + static_cast<size_t>(n) * max_limit * 4;
    b->so_bytes = b->so_n + static_cast<size_t>(n) * 4;
    MGX_HIP(b->d_score_out.Alloc(b->so_bytes));
    MGX_HIP(b->res->Pinned(0, b->so_bytes, &b->h_score_out));
  } else if (p.page_mode) {
    const size_t max_limit = p.max_limit;
    b->doc_page_stride = p.max_limit;
    b->po_totals = static_cast<size_t>(n) * 8 * 8;
    b->po_docs = b->po_totals + static_cast<size_t>(n) * 8;
    b->po_bytes = b->po_docs + static_cast<size_t>(n) * max_limit * 4;
    MGX_HIP(b->d_page_out.Alloc(b->po_bytes));
    MGX_HIP(b->res->Pinned(1, b->po_bytes, &b->h_page_out));
    const size_t tiles = b->idx->dev.n_tiles;
    MGX_HIP(b->d_ptile_cnt.Alloc(static_cast<size_t>(n) * tiles * 4));
    MGX_HIP(b->d_ptile_start.Alloc(static_cast<size_t>(n) * tiles * 8));
  } else {
    MGX_HIP(g.d_counters.Alloc(static_cast<size_t>(n) * 9 * sizeof(unsigned long long)));
  }
  g.h_counters.assign(static_cast<size_t>(n) * 8, 0);
  std::vector<uint32_t> ident(n);
  for (uint32_t i = 0; i < n; ++i) ident[i] = i;
  MGX_HIP(Upload(g.d_ident, ident.data(), n));
  return MGX_OK;
}

// (d) Work items: every query cut into runs of tiles of about equal estimated cost, grouped by query.
// Cost of one tile ~ 1 (operand fetch, program) + matches/128 (enumeration + scoring); a workgroup gets ~48 units.
static void CutItems(const mgx_batch* b, const Group& g, const std::vector<QuerySpec>& specs, GroupPlan& p) {
  static const double kMatchesPerUnit = std::getenv("MGX_ITEM_MATCHES") ? atof(std::getenv("MGX_ITEM_MATCHES")) : 256.0;
  static const double kItemCost = std::getenv("MGX_ITEM_COST") ? atof(std::getenv("MGX_ITEM_COST")) : 192.0;
  static const uint32_t kMaxTiles = std::getenv("MGX_MAX_ITEM_TILES") ? static_cast<uint32_t>(atoi(std::getenv("MGX_MAX_ITEM_TILES"))) : static_cast<uint32_t>(kMaxTilesPerItem);
  static const uint64_t want_items = std::getenv("MGX_WANT_ITEMS") ? static_cast<uint64_t>(atoll(std::getenv("MGX_WANT_ITEMS"))) : 4ull * 768ull;  // ~4 rounds of the 768 workgroups a launch keeps resident
  static const uint32_t kSeedTiles = std::getenv("MGX_SEED_TILES") ? static_cast<uint32_t>(atoi(std::getenv("MGX_SEED_TILES"))) : 16u;
  const uint32_t n = p.n, n_tiles = b->idx->dev.n_tiles;
  p.list_begin.assign(n + 1, 0);
  p.item_begin.assign(n + 1, 0);  // a query's own items (none for the members of a group)
  p.seed_cut.assign(n, 0);
  uint32_t n_lists = 0;
  for (uint32_t i = 0; i < n; ++i) {
    const QuerySpec& s = specs[g.qids[i]];
    const Route route = p.route[i];
    p.item_begin[i] = static_cast<uint32_t>(p.items.size());
    // The fast path prunes most matches once a query has a k-th best score, and a longer item keeps that bound in the
    // workgroup: 4x the tiles per item (measured on the benchmark batch: 1.55 -> 1.49 ms; 8x loses to the tail).
    const bool fast = route == Route::kFast;
    const double per_tile = 1.0 + (p.score_mode || p.df_mode ? s.est_density * kTileDocs / (fast ? kMatchesPerUnit / 2 : kMatchesPerUnit) : 0.0);
    // (a text scan per candidate costs about what scoring a match does)
    // (a small shard wants shorter items than a whole table: 2x..4x the base cost as the tile count goes 77 -> 611,
    // measured at 1.25M docs — 0.47 -> 0.39 ms — and at 10M)
    const double fast_scale = std::min(4.0, std::max(2.0, static_cast<double>(n_tiles) / 150.0));
    uint32_t tiles = static_cast<uint32_t>((fast ? fast_scale * kItemCost : kItemCost) / per_tile);
    tiles = std::max<uint32_t>(8, std::min<uint32_t>(tiles, fast ? 2 * kMaxTiles : kMaxTiles)) & ~7u;  // whole rounds of the waves of a workgroup
    // a small shard (few tiles per query) still wants a few workgroups per CU slot, or the launch is one ragged round
    if (p.score_mode) {
      const uint64_t cap = std::max<uint64_t>(8, (static_cast<uint64_t>(n_tiles) * n / want_items + 7) & ~7ull);
      tiles = static_cast<uint32_t>(std::min<uint64_t>(tiles, cap));
    }
    // the workgroup kernel walks its tiles one after the other (~4 us each): short items keep the few queries it
    // serves from becoming the tail of the step
    if (p.score_mode && route == Route::kBlock) tiles = 8;
    p.list_begin[i] = n_lists;
    if (route == Route::kCand) {  // one workgroup holds the whole query (tile_begin = the driver's leaf)
      p.items.push_back(DevItem{i, p.cand_driver[i], 0, n_lists++});
      continue;
    }
    uint32_t t0 = 0;
    // Fast path: a short "seed" item first (two tiles per wave), launched ahead of everything else (ScheduleItems): it
    // scores its tiles unpruned and publishes the query's first k-th best score, so the long items start pruning at once.
    const uint32_t seed_tiles = std::min<uint32_t>(kSeedTiles, (n_tiles / 8) & ~7u);  // (8 on a 77-tile shard)
    if (fast && seed_tiles && n_tiles > 4 * seed_tiles) {
      p.items.push_back(DevItem{i, 0, seed_tiles, n_lists++});
      p.seed_cut[i] = 1;
      t0 = seed_tiles;
    }
    for (uint32_t t = t0; t < n_tiles; t += tiles) {
      DevItem it{i, t, std::min(tiles, n_tiles - t), n_lists++};  // candidate lists stay grouped by query
      p.items.push_back(it);
    }
  }
  p.list_begin[n] = n_lists;
  p.item_begin[n] = static_cast<uint32_t>(p.items.size());
}

// (e) Launch order, then the items of each route in that order with the fast path's seed items at the front of theirs,
// then the shape of the seed-key exchange. Launch order: by doc band (kSortTiles tiles), so concurrent workgroups share
// operand tiles in L2/MALL; inside a band by the query's largest gram (its bitmap and tf column are the lines the band
// re-reads most), dealt so that workgroup j — which runs on XCD j % 8 under round-robin dispatch, every XCD with its own
// L2 — gets a contiguous eighth of that order. One bucket pass (counts, offsets, scatter): a fresh batch is scheduled
// per step, and two stable sorts of ~12,000 items were a third of the host's compile time.
static int ScheduleItems(const mgx_batch* b, Group& g, const std::vector<QuerySpec>& specs, GroupPlan& p) {
  static const uint32_t kSortTiles = std::getenv("MGX_SORT_TILES") ? static_cast<uint32_t>(atoi(std::getenv("MGX_SORT_TILES"))) : 16u;
  static const bool kXcdAffinity = std::getenv("MGX_XCD_AFFINITY") ? atoi(std::getenv("MGX_XCD_AFFINITY")) != 0 : true;
  static const double kHeavyDensity = std::getenv("MGX_HEAVY_DENSITY") ? atof(std::getenv("MGX_HEAVY_DENSITY")) : 0.05;
  static const double kSqueezeEnv = std::getenv("MGX_HEAVY_SQUEEZE") ? atof(std::getenv("MGX_HEAVY_SQUEEZE")) : -1.0;
  const uint32_t n = p.n, n_tiles = b->idx->dev.n_tiles;
  const bool deal = kXcdAffinity && p.score_mode;
  std::vector<uint32_t> order(n);  // queries in the order they appear inside a band
  for (uint32_t i = 0; i < n; ++i) order[i] = i;
  if (deal) {
    std::vector<uint32_t> heavy(n, 0);
    for (uint32_t i = 0; i < n; ++i) {
      uint64_t best = 0;
      for (const DevLeaf& lf : specs[g.qids[i]].leaves) {
        if (lf.kind != kLeafGramBitmap && lf.kind != kLeafList) continue;
        const uint64_t sz = b->idx->h_offsets[lf.a + 1] - b->idx->h_offsets[lf.a];
        if (sz > best) {
          best = sz;
          heavy[i] = lf.a;
        }
      }
    }
    std::stable_sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) { return heavy[x] < heavy[y]; });
  }
  const uint32_t n_bands = n_tiles / kSortTiles + 1;
  // A heavy query's items (thousands of matches per tile: tens of microseconds per tile visit, where most take one or
  // two) are pulled forward in the launch order — its last bands would otherwise start when the launch is nearly over
  // and finish alone, the tail of the step. They stay in doc order, so the query's bound still grows from band to band.
  // (measured: 0.346 -> 0.327 ms on a 77-tile shard at 0.6; on the 611-tile table the tail is a smaller share of the
  // step and a later start of the query's last bands — a better bound — is worth as much: neutral, left in order)
  const double kHeavySqueeze = kSqueezeEnv >= 0.0 ? kSqueezeEnv : 0.6 + 0.4 * std::min(1.0, n_tiles / 600.0);
  auto band_of = [&](const DevItem& it) {
    const Route route = p.route[it.query];
    if (route == Route::kCand) return 0u;  // (the item covers the whole query; tile_begin holds its driver)
    const uint32_t band = it.tile_begin / kSortTiles;
    if (p.score_mode && route == Route::kFast && specs[g.qids[it.query]].est_density >= kHeavyDensity)
      return static_cast<uint32_t>(band * kHeavySqueeze);
    return band;
  };
  std::vector<uint32_t> band_at(n_bands + 1, 0);
  for (const DevItem& it : p.items) band_at[band_of(it) + 1]++;
  for (uint32_t k = 0; k < n_bands; ++k) band_at[k + 1] += band_at[k];
  std::vector<DevItem> sorted(p.items.size());
  {
    std::vector<uint32_t> cur(band_at.begin(), band_at.end() - 1);
    for (uint32_t oi = 0; oi < n; ++oi) {
      const uint32_t i = order[oi];
      for (uint32_t k = p.item_begin[i]; k < p.item_begin[i + 1]; ++k) sorted[cur[band_of(p.items[k])]++] = p.items[k];
    }
  }
  if (deal) {
    for (uint32_t k = 0; k < n_bands; ++k) {
      const size_t lo = band_at[k], m = band_at[k + 1] - lo, per = (m + 7) / 8;
      size_t w = lo;
      for (size_t r = 0; r < per; ++r)
        for (size_t x = 0; x < 8; ++x)
          if (x * per + r < m) p.items[w++] = sorted[lo + x * per + r];
    }
  } else {
    p.items.swap(sorted);
  }
  p.has_seed.assign(n, 0);
  for (int pass = 0; pass < 2; ++pass) {  // pass 0: the fast path's seed items (a query's first list), then the rest
    for (const DevItem& it : p.items) {
      const Route route = p.route[it.query];
      // (what CutItems cut as one: a first item that merely is short — a table too small for seeds, MGX_SEED_TILES=0 —
      // is an ordinary item and stays in band order)
      const bool seed = route == Route::kFast && p.seed_cut[it.query] != 0 && it.list == p.list_begin[it.query];
      if (seed != (pass == 0)) continue;
      switch (route) {
        case Route::kBlock: p.block.push_back(it); break;
        case Route::kWave: p.wave.push_back(it); break;
        case Route::kWaveLists: p.wave_lists.push_back(it); break;
        case Route::kFast: p.fast[p.fastq[it.query].n_score - 1].push_back(it); break;
        case Route::kCand: p.cand.push_back(it); break;
        case Route::kMerge: p.merge.push_back(it); break;
      }
      if (seed && p.fastq[it.query].blockmax != 0) p.has_seed[it.query] = 1;  // (a query that prunes: its seed's keys are worth sharing)
    }
    if (pass == 0)
      for (int t = 0; t < kFastMaxScore; ++t) g.n_seed_fast[t] = static_cast<uint32_t>(p.fast[t].size());
  }
  // The shape of the seed-key exchange of a sharded table must be the same on every rank, whatever this shard's own
  // index looks like (a gram may be a bitmap here and a list there, a shard a tile shorter): it is made from the QUERIES
  // alone — keys per query = the largest page of the group's SORT _score DESC queries that fit the fast path's lists —
  // and a query without a seed on this rank contributes zeros.
  g.seed_k = 0;
  g.seed_table_docs = 0;
  for (uint32_t i = 0; p.score_mode && i < n; ++i) {
    const QuerySpec& sp = specs[g.qids[i]];
    if (sp.reverse != 0 && p.dq[i].needed != 0 && p.dq[i].needed <= 128u) {
      g.seed_k = std::max(g.seed_k, p.dq[i].needed);
      g.seed_table_docs = std::max<uint64_t>(g.seed_table_docs, sp.total_docs);
    }
  }
  if (g.seed_k) MGX_HIP(Upload(g.d_has_seed, p.has_seed.data(), p.has_seed.size()));
  return MGX_OK;
}

// One route's launch: the group's descriptor over these items.
static hipError_t MakeRoute(RouteLaunch& r, const DevBatch& base, const std::vector<DevItem>& items) {
  r.dev = base;
  r.dev.n_items = static_cast<uint32_t>(items.size());
  const hipError_t e = Upload(r.d_items, items.data(), items.size());
  r.dev.items = r.d_items.as<DevItem>();
  return e;
}

// (f, g) Block-kernel items: queries whose operands are all bitmap-form first (plain instantiation), then the queries
// with a sorted list, an explicit id list or a slot range among their operands (the instantiation that skips / jumps
// over tiles), and last the queries with kOpVerifyFuzzy or kOpVerifyTree (the FZ instantiation, launched apart). Then the group's
// descriptor with the outputs sized by its candidate lists, and one launch per route over it.
static int UploadItems(mgx_batch* b, Group& g, const std::vector<QuerySpec>& specs, GroupPlan& p) {
  const uint32_t n = p.n;
  std::vector<uint8_t> listlike(n, 0);
  for (uint32_t i = 0; i < n; ++i) {
    for (const DevLeaf& lf : specs[g.qids[i]].leaves)
      if (lf.kind == kLeafList || lf.kind == kLeafExplicit || lf.kind == kLeafRange) listlike[i] = 1;
    if (specs[g.qids[i]].fz_op) listlike[i] = 2;
  }
  std::stable_partition(p.block.begin(), p.block.end(), [&](const DevItem& it) { return listlike[it.query] == 0; });
  if (std::find(listlike.begin(), listlike.end(), 2) != listlike.end())
    std::stable_partition(p.block.begin(), p.block.end(), [&](const DevItem& it) { return listlike[it.query] != 2; });
  g.n_items_plain = g.n_items_fz = 0;
  for (const DevItem& it : p.block) {
    g.n_items_plain += listlike[it.query] == 0 ? 1u : 0u;
    g.n_items_fz += listlike[it.query] == 2 ? 1u : 0u;
  }
  DevBatch& d = g.dev;
  d.queries = g.d_queries.as<DevQuery>();
  d.leaves = g.d_leaves.as<DevLeaf>();
  d.prog = g.d_prog.as<uint32_t>();
  d.score_terms = g.d_score.as<DevScoreTerm>();
  d.explicit_pool = g.d_explicit.as<uint32_t>();
  d.patterns = b->d_patterns.as<uint8_t>();
  d.text_terms = b->d_text_terms.as<DevTextTerm>();
  d.text_idf = b->d_text_idf.as<double>();
  d.verify_terms = b->d_verify_terms.as<DevTextTerm>();
  d.verify_prog = b->d_verify_prog.as<uint32_t>();
  d.n_queries = n;
  d.counters = p.score_mode  ? b->sc_counters()
               : p.page_mode ? b->d_page_out.as<unsigned long long>()
                             : g.d_counters.as<unsigned long long>();
  if (p.page_mode) {
    d.tile_cnt = b->d_ptile_cnt.as<uint32_t>();
    d.tile_start = b->d_ptile_start.as<uint64_t>();
    d.totals = reinterpret_cast<const uint64_t*>(static_cast<const char*>(b->d_page_out.p) + b->po_totals);
    d.page_docs = reinterpret_cast<uint32_t*>(static_cast<char*>(b->d_page_out.p) + b->po_docs);
    d.page_stride = b->doc_page_stride;
  }
  d.bounds = p.score_mode ? d.counters + static_cast<size_t>(n) * 8 : nullptr;
#ifdef MGX_ABLATION
  d.debug_skip = std::getenv("MGX_DEBUG_SKIP") ? static_cast<uint32_t>(atoi(std::getenv("MGX_DEBUG_SKIP"))) : 0u;
#endif
  if (p.score_mode) {
    const size_t n_lists = p.list_begin[n], max_needed = p.max_needed;
    d.cand_stride = b->top_stride = p.max_needed;
    b->page_stride = p.max_limit;
    MGX_HIP(b->d_cand_keys.Alloc(n_lists * max_needed * 8));
    MGX_HIP(b->d_cand_docs.Alloc(n_lists * max_needed * 4));
    MGX_HIP(b->d_cand_n.Alloc(n_lists * 4));
    {
      const size_t elems = static_cast<size_t>(n) * max_needed + n;
      b->ex_off32 = elems * 8;
      b->ex_bytes = (elems * 12 + 7) / 8 * 8;
      MGX_HIP(b->d_export.Alloc(b->ex_bytes));
    }
    d.cand_keys = b->d_cand_keys.as<uint64_t>();
    d.cand_docs = b->d_cand_docs.as<uint32_t>();
    d.cand_n = b->d_cand_n.as<uint32_t>();
  } else if (!p.df_mode && !p.page_mode) {
    const size_t tiles = b->idx->dev.n_tiles;
    MGX_HIP(b->d_rbits.Alloc(static_cast<size_t>(n) * tiles * kWordsPerTile * 8));
    MGX_HIP(b->d_tile_cnt.Alloc(static_cast<size_t>(n) * tiles * 4));
    MGX_HIP(b->d_tile_start.Alloc(static_cast<size_t>(n) * tiles * 8));
    MGX_HIP(b->d_totals.Alloc(static_cast<size_t>(n) * 8));
    MGX_HIP(b->d_take.Alloc(static_cast<size_t>(n) * 8));
    MGX_HIP(b->d_out_off.Alloc(static_cast<size_t>(n) * 8));
    std::vector<uint32_t> rev(n);
    for (uint32_t i = 0; i < n; ++i) rev[i] = (specs[g.qids[i]].deep_score || specs[g.qids[i]].col_sort) ? 0u : specs[g.qids[i]].reverse;
    MGX_HIP(Upload(b->d_reverse, rev.data(), n));
    d.rbits = b->d_rbits.as<uint64_t>();
    d.tile_cnt = b->d_tile_cnt.as<uint32_t>();
  }
  if (p.score_mode && !p.wave_tables.empty()) {
    MGX_HIP(Upload(g.d_tables, p.wave_tables.data(), p.wave_tables.size()));
    d.wave_tables = g.d_tables.as<uint64_t>();
  }
  if (!p.fastq.empty()) MGX_HIP(Upload(g.d_fast_queries, p.fastq.data(), p.fastq.size()));
  d.fast_queries = g.d_fast_queries.as<DevFastQuery>();
  d.dev_index = b->idx->d_dev_index.as<DevIndex>();
  d.cond_bitmaps = b->cond_arena;
  for (int t = 0; t < kFastMaxScore; ++t) MGX_HIP(MakeRoute(g.fast[t], d, p.fast[t]));
  MGX_HIP(MakeRoute(g.wave_lists, d, p.wave_lists));
  MGX_HIP(MakeRoute(g.cand, d, p.cand));
  MGX_HIP(MakeRoute(g.merge, d, p.merge));
  if (p.page_mode && !p.cand.empty()) {
    std::vector<uint8_t> skip(n, 0);
    for (uint32_t i = 0; i < n; ++i) skip[i] = p.route[i] == Route::kCand ? 1 : 0;
    MGX_HIP(Upload(g.d_cand_skip, skip.data(), skip.size()));
  }
  MGX_HIP(MakeRoute(g.block, d, p.block));
  MGX_HIP(MakeRoute(g.wave, d, p.wave));
  MGX_HIP(Upload(g.d_list_begin, p.list_begin.data(), p.list_begin.size()));
  if (p.page_mode) {
    // the page pass: one item per query (cand_kernel writes its own pages); kOpVerifyFuzzy / kOpVerifyTree queries last in page_block,
    // on the general kernel's FZ launch
    std::vector<DevItem> pw, pb;
    for (uint32_t i = 0; i < n; ++i)
      if (p.route[i] != Route::kCand && !specs[g.qids[i]].fz_op)
        (p.route[i] == Route::kWave ? pw : pb).push_back(DevItem{i, 0, 0, 0});
    g.n_page_fz = 0;
    for (uint32_t i = 0; i < n; ++i)
      if (specs[g.qids[i]].fz_op) {
        pb.push_back(DevItem{i, 0, 0, 0});
        ++g.n_page_fz;
      }
    MGX_HIP(MakeRoute(g.page_wave, d, pw));
    MGX_HIP(MakeRoute(g.page_block, d, pb));
  }
  return MGX_OK;
}

// Plans one group of the batch (the queries of one mode) and ships its tables: query layout, each query's route, the
// work items and their launch order, then one descriptor per launch.
static int UploadGroup(mgx_batch* b, Group& g, uint32_t mode, const std::vector<QuerySpec>& specs) {
  GroupPlan p(static_cast<uint32_t>(g.qids.size()), mode);
  if (p.n == 0) return MGX_OK;
  const PathSwitches sw;
  SectionTimer sec;
  if (const int rc = LayOutQueries(b, g, specs, p)) return rc;
  sec.Mark(0);
  if (const int rc = ChooseRoutes(b, g, specs, sw, p)) return rc;
  sec.Mark(1);
  if (const int rc = UploadTables(b, g, p, sec)) return rc;
  sec.Mark(3);
  CutItems(b, g, specs, p);
  sec.Mark(4);
  if (const int rc = ScheduleItems(b, g, specs, p)) return rc;
  sec.Mark(5);
  if (const int rc = UploadItems(b, g, specs, p)) return rc;
  sec.Mark(6);
  if (std::getenv("MGX_VERBOSE")) {
    size_t fast_queries = 0;
    for (Route r : p.route) fast_queries += r == Route::kFast ? 1 : 0;
    // the fast path's schedule: its seed items, the most items one query was cut into, the longest item in tiles
    uint32_t fast_seeds = 0, fast_most = 0, fast_longest = 0;
    std::vector<uint32_t> per_query(p.n, 0);
    for (int t = 0; t < kFastMaxScore; ++t) {
      fast_seeds += g.n_seed_fast[t];
      for (const DevItem& it : p.fast[t]) {
        fast_most = std::max(fast_most, ++per_query[it.query]);
        fast_longest = std::max(fast_longest, it.n_tiles);
      }
    }
    fprintf(stderr,
            "[mgx] %s group: %u queries; fast path %zu items (%zu queries, lds %u B, ring %u), wave kernel %zu items "
            "(lds %u B, lists %zu), block kernel %zu items (lds %u B), candidate-driven %zu queries, list merge %zu "
            "items; fast schedule: %u seed items, at most %u items per query, longest item %u tiles\n",
            p.score_mode ? "score" : p.page_mode ? "docid-page" : p.df_mode ? "df" : "bitmap", p.n,
            p.fast[0].size() + p.fast[1].size() + p.fast[2].size() + p.fast[3].size() + p.fast[4].size(), fast_queries,
            g.fplan.bytes, g.fplan.ring, p.wave.size() + p.wave_lists.size(), g.wplan.bytes, p.wave_lists.size(),
            p.block.size(), g.plan.bytes, p.cand.size(), p.merge.size(), fast_seeds, fast_most, fast_longest);
  }
  return MGX_OK;
}

// The host facts the query compiler reads (mgx_compile.hpp): one per CompileAll, single-operator call and df pass.
static CompileView ViewOf(const mgx_index* idx) {
  CompileView v;
  v.offsets = idx->h_offsets.data();
  v.skip_row = idx->h_skip_row.data();
  v.bm_row = idx->h_bm_row.data();
  v.n_grams = idx->n_grams;
  v.n_docs = idx->dev.n_docs;
  v.first_doc_id = idx->dev.first_doc_id;
  v.has_text = idx->dev.text != nullptr;
  v.can_score = idx->can_score;
  v.n_filter_rows = idx->n_filter_rows;
  v.n_filter_columns = idx->n_filter_columns.load(std::memory_order_acquire);
  v.live_row = idx->live_row.load(std::memory_order_relaxed);
  v.bitmaps_clean = idx->bitmaps_clean.load(std::memory_order_relaxed);
  static const bool pk_general = [] {
    const char* e = std::getenv("MGX_PK_SORT_GENERAL");
    return e != nullptr && e[0] != '\0' && e[0] != '0';
  }();
  v.pk_docid_order = !pk_general && !idx->has_doc_map.load(std::memory_order_acquire) && idx->pk_monotone.load(std::memory_order_acquire) &&
                     idx->pk_shortcut.load(std::memory_order_relaxed);
  return v;
}

// queries [a, b) into their specs, up to the first that fails: its code, and "query i: <its message>" as the last error
static int CompileRange(const CompileView& view, const mgx_query* queries, std::vector<QuerySpec>* specs, uint32_t a, uint32_t b) {
  for (uint32_t i = a; i < b; ++i) {
    (*specs)[i].Clear();
    if (const int rc = CompileQuery(view, queries[i], &(*specs)[i])) return Fail(rc, "query " + std::to_string(i) + ": " + g_last_error);
  }
  return MGX_OK;
}

// CompileQuery over a whole batch. Queries are independent, so batches of a few hundred and more are cut into chunks for
// a small process-wide helper pool (MGX_COMPILE_THREADS helpers, default 3, beside the calling thread): on a doc-range
// shard the device finishes a batch in a fraction of a millisecond and the host's per-batch compile is what a rank's
// throughput hangs on. One caller at a time uses the pool; a second concurrent caller compiles inline.
struct CompilePool {
  std::mutex mu, gate;
  std::condition_variable cv_work, cv_done;
  std::vector<std::thread> helpers;
  const CompileView* view = nullptr;
  const mgx_query* queries = nullptr;
  std::vector<QuerySpec>* specs = nullptr;
  uint32_t next = 0, end = 0, pending = 0;
  int rc = MGX_OK;
  std::string error;
  bool stop = false;
  static constexpr uint32_t kChunk = 64;

  void Run(std::unique_lock<std::mutex>& lock) {  // called with mu held; works until the queue is empty
    while (next < end) {
      const uint32_t a = next, b = std::min(end, a + kChunk);
      next = b;
      lock.unlock();
      const int local = CompileRange(*view, queries, specs, a, b);
      lock.lock();
      if (local && rc == MGX_OK) {
        rc = local;
        error = g_last_error;
      }
      pending -= b - a;
    }
  }
  void Helper() {
    std::unique_lock<std::mutex> lock(mu);
    for (;;) {
      cv_work.wait(lock, [&] { return stop || next < end; });
      if (stop) return;
      Run(lock);
      if (pending == 0) cv_done.notify_all();
    }
  }
  CompilePool() {
    const int n = std::getenv("MGX_COMPILE_THREADS") ? atoi(std::getenv("MGX_COMPILE_THREADS")) : 3;
    for (int i = 0; i < n; ++i)
      helpers.emplace_back([this] {
        pthread_setname_np(pthread_self(), "mgx-compile");
        Helper();
      });
  }
  ~CompilePool() {
    {
      std::lock_guard<std::mutex> lock(mu);
      stop = true;
    }
    cv_work.notify_all();
    for (auto& t : helpers) t.join();
  }
};

// SORT <filter column>: what the compiler cannot see of the column (its class, the mark of mgx_index_add_filter_column)
static int CheckSortColumns(const mgx_index* idx, const std::vector<QuerySpec>& specs) {
  bool any = false;
  for (const QuerySpec& sp : specs) any = any || (sp.col_sort && !sp.pk_sort);
  if (!any) return MGX_OK;
  std::lock_guard<std::mutex> lock(const_cast<mgx_index*>(idx)->mu);
  for (size_t i = 0; i < specs.size(); ++i) {
    const QuerySpec& sp = specs[i];
    if (!sp.col_sort || sp.pk_sort) continue;  // (the primary keys are no filter column and hold no NULL)
    const std::string who = "query " + std::to_string(i) + ": ";
    if (sp.sort_column >= idx->filter_columns.size()) return Fail(MGX_ERR_OUT_OF_RANGE, who + "sort_column: unknown filter column");
    const mgx_index::FilterColumn& col = *idx->filter_columns[sp.sort_column];
    if (sp.sort_ranks && col.value_class != MGX_FC_UNSIGNED)
      return Fail(MGX_ERR_INVALID_ARGUMENT, who + "MGX_SORT_COLUMN_RANK needs an MGX_FC_UNSIGNED column of dictionary ranks");
    if (colsort::KeysCollide(col.sort_keys, col.sort_keys))
      return Fail(MGX_ERR_NOT_IMPLEMENTED,
                  who + "SORT by this column is not implemented: it holds NULLs beside a value whose 64-bit sort key is "
                        "NULL's (INT64_MIN, or the double whose bits are all ones)");
  }
  return MGX_OK;
}

// The key scan of a filter column (false: no such column), read under the index's lock
static bool SortKeysOf(const mgx_index* idx, uint32_t column, colsort::KeyScan* out) {
  std::lock_guard<std::mutex> lock(const_cast<mgx_index*>(idx)->mu);
  if (column >= idx->filter_columns.size()) return false;
  *out = idx->filter_columns[column]->sort_keys;
  return true;
}

static int CompileQueries(const mgx_index* idx, const mgx_query* queries, uint32_t n, std::vector<QuerySpec>* specs);
static int CompileAll(const mgx_index* idx, const mgx_query* queries, uint32_t n, std::vector<QuerySpec>* specs) {
  if (const int rc = CompileQueries(idx, queries, n, specs)) return rc;
  return CheckSortColumns(idx, *specs);
}

static int CompileQueries(const mgx_index* idx, const mgx_query* queries, uint32_t n, std::vector<QuerySpec>* specs) {
  // one pool per calling thread: an executor's dispatcher threads compile different batches at the same time, and a
  // shared pool handed its helpers to one of them while the other compiled its 1024 queries alone (4x the time)
  static thread_local CompilePool pool;
  const CompileView view = ViewOf(idx);
  std::unique_lock<std::mutex> gate(pool.gate, std::try_to_lock);
  if (n < 4 * CompilePool::kChunk || pool.helpers.empty() || !gate.owns_lock()) return CompileRange(view, queries, specs, 0, n);
  std::unique_lock<std::mutex> lock(pool.mu);
  pool.view = &view;
  pool.queries = queries;
  pool.specs = specs;
  pool.next = 0;
  pool.end = pool.pending = n;
  pool.rc = MGX_OK;
  pool.cv_work.notify_all();
  pool.Run(lock);  // the caller compiles too
  pool.cv_done.wait(lock, [&] { return pool.pending == 0; });
  pool.end = 0;
  if (pool.rc) SetError(pool.error);
  return pool.rc;
}

// The batch's FILTER conditions (mgx_query.conditions): every distinct one (all fields but `negate`) gets one row of the
// batch's condition arena, its operands get that row, and the descriptors the first launch of every execute reads —
// the conditions sorted by column, one group per column — go into the upload arena. Nothing here touches the device
// beyond growing the arena when this batch holds more distinct conditions than any before it.
static int LayOutConditions(mgx_batch* b) {
  mgx_index* idx = b->idx;
  size_t n_refs = 0;
  for (const QuerySpec& s : b->specs) n_refs += s.conds.size();
  if (n_refs == 0) return MGX_OK;
  using Key = std::tuple<uint32_t, uint32_t, uint64_t, uint64_t, uint32_t, uint32_t>;  // column first: the map is the kernel's order
  std::map<Key, uint32_t> rows;
  for (QuerySpec& s : b->specs)
    for (DevLeaf& lf : s.leaves) {
      if (lf.kind != kLeafCondBitmap) continue;
      const mgx_condition& c = s.conds[lf.a];
      const Key key{c.column_id, c.op, c.literal_bits, Bits(c.eq_epsilon), c.null_matches ? 1u : 0u, c.never_matches ? 1u : 0u};
      lf.b = rows.emplace(key, static_cast<uint32_t>(rows.size())).first->second;
      lf.a = 0;
    }
  const uint64_t row_bytes = idx->dev.fb_row_stride * sizeof(uint64_t);
  if (idx->dev.fb_row_stride % kCondBlockWords != 0)  // (the condition pass covers a row in whole workgroups)
    return Fail(MGX_ERR_INTERNAL, "filter row stride is not a multiple of the condition pass's block");
  if (rows.size() * row_bytes > MGX_CONDITION_ARENA_MAX_BYTES)
    return Fail(MGX_ERR_OUT_OF_RANGE, "the batch holds " + std::to_string(rows.size()) + " distinct conditions of " +
                                          std::to_string(row_bytes) + " bytes each: more than the " +
                                          std::to_string(MGX_CONDITION_ARENA_MAX_BYTES) +
                                          " bytes (MGX_CONDITION_ARENA_MAX_BYTES) a batch's condition arena may take");
  void* arena = nullptr;
  MGX_HIP(b->res->Conditions(rows.size() * row_bytes, &arena));
  b->cond_arena = static_cast<uint64_t*>(arena);
  std::vector<DevCondition> conds;
  std::vector<DevCondGroup> groups;
  conds.reserve(rows.size());
  {
    std::lock_guard<std::mutex> lock(idx->mu);  // (columns are added under mu; the objects themselves never move)
    uint32_t last_column = 0;
    for (const auto& kv : rows) {
      const uint32_t column = std::get<0>(kv.first);
      if (groups.empty() || column != last_column) {
        last_column = column;
        const mgx_index::FilterColumn& col = *idx->filter_columns[column];
        DevCondGroup g{};
        g.values = col.d_values.as<uint64_t>();
        g.is_null = col.d_null.as<uint8_t>();
        g.value_class = col.value_class;
        g.cond_begin = g.cond_end = static_cast<uint32_t>(conds.size());
        groups.push_back(g);
      }
      DevCondition d{};
      d.literal = std::get<2>(kv.first);
      __builtin_memcpy(&d.eq_epsilon, &std::get<3>(kv.first), 8);
      d.op = std::get<1>(kv.first);
      d.null_matches = std::get<4>(kv.first);
      d.never_matches = std::get<5>(kv.first);
      d.row = kv.second;
      conds.push_back(d);
      groups.back().cond_end = static_cast<uint32_t>(conds.size());
    }
  }
  if (groups.size() > 65535) return Fail(MGX_ERR_OUT_OF_RANGE, "conditions on more than 65535 columns in one batch");
  MGX_HIP(Upload(b->d_conds, conds.data(), conds.size()));
  MGX_HIP(Upload(b->d_cond_groups, groups.data(), groups.size()));
  b->n_cond_groups = static_cast<uint32_t>(groups.size());
  return MGX_OK;
}

// Text-level scored terms: numbered across the batch and deduplicated — the df of a term depends on the term (and on
// N), not on the query around it — their bytes pooled, and one df query compiled per distinct term (b->df_specs).
static int NumberTextTerms(mgx_batch* b, std::string* pool, std::vector<DevTextTerm>* tts) {
  mgx_index* idx = b->idx;
  const CompileView view = ViewOf(idx);
  std::map<std::pair<std::string, uint64_t>, uint32_t> seen;
  for (QuerySpec& s : b->specs) {
    for (const QuerySpec::TextTerm& tt : s.text_terms) {
      const auto ins = seen.emplace(std::make_pair(tt.pattern, s.total_docs), static_cast<uint32_t>(tts->size()));
      const uint32_t id = ins.first->second;
      if (s.deep_score) s.deep_grams[tt.score_index] = kDeepText | id;
      else s.score[tt.score_index].text_term = id;
      if (!ins.second) continue;
      const DevTextTerm d{static_cast<uint32_t>(pool->size()), static_cast<uint32_t>(tt.pattern.size())};
      *pool += tt.pattern;
      tts->push_back(d);
      b->text_total_docs.push_back(s.total_docs);
      std::string ckey = tt.pattern + '\0' + std::to_string(s.total_docs);
      uint64_t known = ~0ull;
      {
        std::lock_guard<std::mutex> lock(idx->table_mu);
        const auto hit = idx->df_cache.find(ckey);
        if (hit != idx->df_cache.end()) known = hit->second;
      }
      b->text_df_known.push_back(tt.grams.empty() ? 0ull : known);
      b->text_df_key.push_back(std::move(ckey));
      QuerySpec ds;
      if (const int rc = CompileTextDf(view, tt.grams, tt.grams.empty() || known != ~0ull, d.pat_off, d.pat_len, &ds)) return rc;
      b->df_specs.push_back(std::move(ds));
    }
  }
  return MGX_OK;
}

// The patterns of the exact-text / FUZZY / tree filters share the pool; the tree filters' verify programs one array.
static void PoolVerifyPatterns(mgx_batch* b, std::string* pool, std::vector<DevTextTerm>* vts, std::vector<uint32_t>* vprog) {
  for (QuerySpec& s : b->specs) {
    s.vt_begin = static_cast<uint32_t>(vts->size());
    s.vp_begin = static_cast<uint32_t>(vprog->size());
    vprog->insert(vprog->end(), s.verify_prog.begin(), s.verify_prog.end());
    for (const std::string& pat : s.verify_patterns) {
      vts->push_back(DevTextTerm{static_cast<uint32_t>(pool->size()), static_cast<uint32_t>(pat.size())});
      *pool += pat;
    }
  }
}

// Compiles `specs` into batch object `b` (fresh, or just emptied by ResetBatch): every device array comes from the
// batch's arenas, nothing is copied to the device here — the first execute ships the upload arena.
static int PrepareInto(mgx_batch* b, mgx_index* idx, std::vector<QuerySpec>&& specs) {
  ResourceScope scope(b->res);
  b->idx = idx;
  b->n_queries = static_cast<uint32_t>(specs.size());
  b->specs = std::move(specs);
  for (uint32_t i = 0; i < b->n_queries; ++i) {
    const uint32_t m = b->specs[i].mode;
    (m == kModeScore ? b->score : m == kModeDocPage ? b->page : b->bitmap).qids.push_back(i);
  }
  MGX_HIP(hipSetDevice(idx->device));
  if (const int rc = LayOutConditions(b)) return rc;
  std::string pool;  // the bytes of every pattern of the batch: text-level scored terms, then verify patterns
  std::vector<DevTextTerm> tts, vts;
  std::vector<uint32_t> vprog;
  if (const int rc = NumberTextTerms(b, &pool, &tts)) return rc;
  PoolVerifyPatterns(b, &pool, &vts, &vprog);
  if (!vprog.empty()) MGX_HIP(Upload(b->d_verify_prog, vprog.data(), vprog.size()));
  if (!vts.empty()) MGX_HIP(Upload(b->d_verify_terms, vts.data(), vts.size()));
  if (!pool.empty()) MGX_HIP(Upload(b->d_patterns, reinterpret_cast<const uint8_t*>(pool.data()), pool.size(), 16));
  const uint32_t n_tt = static_cast<uint32_t>(tts.size());
  if (n_tt != 0) {
    MGX_HIP(Upload(b->d_text_terms, tts.data(), tts.size()));
    MGX_HIP(b->d_text_idf.Alloc(static_cast<size_t>(n_tt) * sizeof(double)));
    MGX_HIP(b->d_text_df.Alloc(static_cast<size_t>(n_tt) * sizeof(uint64_t)));
    MGX_HIP(b->d_text_df_local.Alloc(static_cast<size_t>(n_tt) * sizeof(uint64_t)));
    MGX_HIP(Upload(b->d_text_df_known, b->text_df_known.data(), b->text_df_known.size()));
    b->h_text_df.assign(n_tt, 0);
    b->h_text_df_local.assign(n_tt, 0);
    b->h_text_idf.assign(n_tt, 0.0);
    for (uint32_t i = 0; i < n_tt; ++i) b->textdf.qids.push_back(i);
  }
  int rc = UploadGroup(b, b->score, kModeScore, b->specs);
  if (rc) return rc;
  rc = UploadGroup(b, b->bitmap, kModeBitmap, b->specs);
  if (rc) return rc;
  rc = UploadGroup(b, b->textdf, kModeTextDf, b->df_specs);
  if (rc) return rc;
  rc = UploadGroup(b, b->page, kModeDocPage, b->specs);
  if (rc) return rc;
  b->h_results.assign(b->n_queries, mgx_query_result{});
  return MGX_OK;
}

static int PrepareFromSpecs(mgx_index* idx, std::vector<QuerySpec>&& specs, mgx_batch** out) {
  auto b = std::make_unique<mgx_batch>();
  b->res_owned = std::make_unique<BatchResources>();
  b->res = b->res_owned.get();
  int rc = PrepareInto(b.get(), idx, std::move(specs));
  if (rc) return rc;
  *out = b.release();
  return MGX_OK;
}

// Empties a batch object for re-use; its resources (arena chunks, pinned result blocks, events) stay.
static void ResetBatch(mgx_batch* b) {
  std::unique_ptr<BatchResources> owned = std::move(b->res_owned);
  BatchResources* res = b->res;
  for (auto& ev : b->events) {
    (void)hipEventDestroy(ev.first);
    (void)hipEventDestroy(ev.second);
  }
  const bool timing = b->timing;
  b->~mgx_batch();
  new (b) mgx_batch();
  b->res_owned = std::move(owned);
  b->res = res;
  b->timing = timing;
  if (res) res->Reset();
}

// Result blocks of the score / docid-page groups -> pinned host memory, fenced by the batch's done event.
static int IssueResultCopy(mgx_batch* b, hipStream_t s) {
  if (!b->res) return MGX_OK;
  if (!b->page.qids.empty())
    MGX_HIP(hipMemcpyAsync(b->h_page_out, b->d_page_out.p, b->po_bytes, hipMemcpyDeviceToHost, s));
  if (!b->score.qids.empty())
    MGX_HIP(hipMemcpyAsync(b->h_score_out, b->d_score_out.p, b->so_bytes, hipMemcpyDeviceToHost, s));
  if (!b->res->done_ev) {
    MGX_HIP(hipEventCreateWithFlags(&b->res->done_ev, hipEventDisableTiming));
  }
  MGX_HIP(hipEventRecord(b->res->done_ev, s));
  b->res->copy_issued = true;
  return MGX_OK;
}

// hip_stream as given by the caller (NULL = the default stream, as everywhere in HIP).
static int BatchStream(mgx_batch* b, void* hip_stream, hipStream_t* out) {
  (void)b;
  *out = static_cast<hipStream_t>(hip_stream);
  return MGX_OK;
}

// The batch's input arrays travel on the stream of its first execute (or df pass): one copy per arena chunk.
static int EnsureUploaded(mgx_batch* b, hipStream_t s) {
  if (!b->res || b->res->uploaded) return MGX_OK;
  for (const Arena::Chunk& c : b->res->upload.chunks)
    if (c.used) MGX_HIP(hipMemcpyAsync(c.dev, c.host, c.used, hipMemcpyHostToDevice, s));
  b->res->uploaded = true;
  return MGX_OK;
}

// df pass of the text-level terms: counts land in d_text_df[term]
static int CountDfImpl(mgx_batch* b, hipStream_t s) {
  mgx_index* idx = b->idx;
  mgx_batch::Group& g = b->textdf;
  if (g.qids.empty()) return MGX_OK;
  MGX_HIP(hipSetDevice(idx->device));
  {
    int rc = EnsureUploaded(b, s);
    if (rc) return rc;
  }
  MGX_HIP(hipMemsetAsync(g.d_counters.p, 0, g.d_counters.bytes, s));
  MGX_LAUNCH(LaunchWaveCount(idx->dev, g.wave.dev, g.wplan, true, s));
  MGX_LAUNCH(LaunchTileEval(kModeTextDf, idx->dev, g.block.dev, g.plan, s, g.n_items_plain));
  // counter slot 5 of every df query (or the cached local count) -> the local array and the buffer ranks all-reduce
  MGX_LAUNCH(LaunchGatherDf(g.d_counters.as<unsigned long long>(), b->d_text_df_known.as<uint64_t>(),
                            static_cast<uint32_t>(g.qids.size()), b->d_text_df_local.as<uint64_t>(),
                            b->d_text_df.as<uint64_t>(), s));
  return MGX_OK;
}

// Sharded tables: between a score group's seed launch and its main launch, every rank's seed keys are all-gathered (by
// the caller's transport: RCCL in mgx_batch_execute_sharded, anything in mgx_batch_execute_gather) and each query's bound
// is raised to the needed-th best of their union.
struct SeedGather {
  int world = 1;
  mgx_gather_fn fn = nullptr;
  void* user = nullptr;
};
static int SeedBoundExchange(mgx_batch* b, mgx_batch::Group& g, const SeedGather& sg, hipStream_t s);

// Fork of the side stream (idx->side_stream): it waits for what `s` has queued so far. A group joins it by recording
// res->join_ev on the side stream after its side launches, and `s` waits for that event where the group needs them.
static int ForkSide(mgx_batch* b, hipStream_t s) {
  if (!b->res->fork_ev) {
    MGX_HIP(hipEventCreateWithFlags(&b->res->fork_ev, hipEventDisableTiming));
    MGX_HIP(hipEventCreateWithFlags(&b->res->join_ev, hipEventDisableTiming));
  }
  MGX_HIP(hipEventRecord(b->res->fork_ev, s));
  MGX_HIP(hipStreamWaitEvent(b->idx->side_stream, b->res->fork_ev, 0));
  return MGX_OK;
}

// HIGHLIGHT: the records of the highlighted queries' page entries, behind the kernel that finalised the page, and their
// copy to pinned memory (the caller records the batch's done event after it). `mapped`: the index whose documents the
// page names by table id through its doc map (the delta of a mutable table), `plain`: the index whose own ids it holds.
static int RunHighlight(mgx_batch* b, hipStream_t s, bool merged, const mgx_index* mapped, const mgx_index* plain) {
  mgx_batch::Highlight& h = b->hl;
  DevHlBatch hb{};
  hb.queries = h.d_queries.as<DevHlQuery>();
  hb.n_queries = static_cast<uint32_t>(h.queries.size());
  hb.n_entries = h.n_entries;
  hb.terms = h.d_terms.as<DevHlTerm>();
  hb.patterns = h.d_patterns.as<uint8_t>();
  hb.arena = h.d_arena.as<uint8_t>();
  auto source = [](const mgx_index* ix, bool with_map) {
    DevHlSource src{};
    if (!ix) return src;
    src.text = ix->dev.text;
    src.text_off = ix->dev.text_off;
    src.doc_map = with_map ? ix->d_doc_map.as<uint32_t>() : nullptr;
    src.first_doc_id = ix->dev.first_doc_id;
    src.n_docs = ix->dev.n_docs;
    return src;
  };
  hb.mapped = source(mapped, true);
  hb.plain = source(plain, false);
  hb.merged = merged ? 1u : 0u;
  // an index with originals: the kernel that reads them; else what a batch has always launched
  const highlight::DevOriginals none{};
  const highlight::DevOriginals& om = mapped ? mapped->originals : none;
  const highlight::DevOriginals& op = plain ? plain->originals : none;
  if (om.kind || op.kind) MGX_LAUNCH(LaunchHighlightOriginal(hb, om, op, s));
  else MGX_LAUNCH(LaunchHighlight(hb, s));
  MGX_HIP(hipMemcpyAsync(h.h_arena, h.d_arena.p, h.bytes, hipMemcpyDeviceToHost, s));
  return MGX_OK;
}

// FACET in a batch: the counts of every (faceted query, column) from the bitmap group's result bitmaps, behind the
// group's kernels, and their copy to pinned memory (the caller records the batch's done event after it).
static int RunFacets(mgx_batch* b, hipStream_t s) {
  mgx_batch::Facets& f = b->fc;
  if (f.plan.arena_bytes == 0) return MGX_OK;  // (every requested column is empty: there is nothing to count)
  MGX_HIP(hipMemsetAsync(f.d_counts.p, 0, f.plan.arena_bytes, s));
  facet::DevBatch fb{};
  fb.rbits = b->bitmap.dev.rbits;
  fb.queries = f.d_queries.as<facet::DevQuery>();
  fb.columns = f.d_columns.as<facet::DevColumn>();
  fb.items = f.d_items.as<facet::Item>();
  fb.n_items = static_cast<uint32_t>(f.plan.items.size());
  fb.n_docs = b->idx->dev.n_docs;
  MGX_LAUNCH(LaunchFacetBatch(fb, s));
  MGX_HIP(hipMemcpyAsync(f.h_counts, f.d_counts.p, f.plan.arena_bytes, hipMemcpyDeviceToHost, s));
  return MGX_OK;
}

// Page documents: what document_gather_kernel reads of one index. `cols`: the requested columns of that index, resolved by
// the batch that was prepared on it (device memory once that batch's inputs are uploaded).
static documents::DevSource DocumentSource(const mgx_index* ix, const mgx_batch* cols, bool with_map) {
  documents::DevSource src{};
  if (!ix) return src;
  src.key_bytes = ix->d_pkb_bytes.as<uint8_t>();
  src.key_off = ix->d_pkb_off.as<uint64_t>();
  src.has_key = ix->d_pkb_has.as<uint8_t>();
  src.doc_map = with_map ? ix->d_doc_map.as<uint32_t>() : nullptr;
  src.columns = cols->doc.d_columns.as<documents::DevColumn>();
  src.first_doc_id = ix->dev.first_doc_id;
  src.n_docs = ix->dev.n_docs;
  return src;
}

// The batches of a merged page by how their index names its documents: `mapped` by table id through its doc map (the
// delta of a mutable table), `plain` by its own ids (the main index). False: a second batch of either kind.
static bool MainAndDelta(const mgx_batch* primary, mgx_batch* const* others, uint32_t n_others, const mgx_batch** mapped,
                         const mgx_batch** plain) {
  *mapped = *plain = nullptr;
  for (uint32_t j = 0; j <= n_others; ++j) {
    const mgx_batch* x = j == 0 ? primary : others[j - 1];
    const mgx_batch*& slot = x->idx->d_doc_map.p ? *mapped : *plain;
    if (slot) return false;
    slot = x;
  }
  return true;
}

// A table with a delta: the two batches carry requests of the same shape (each with its own index's column ids), and both
// indexes hold key bytes.
static int CheckDocumentSides(const mgx_batch* primary, const mgx_batch* other, const char* entry) {
  const mgx_batch::Documents& a = primary->doc;
  const mgx_batch::Documents& o = other->doc;
  bool same = o.on() && o.plan.queries.size() == a.plan.queries.size() && o.of_query == a.of_query;
  for (size_t i = 0; same && i < a.plan.queries.size(); ++i)
    same = a.plan.queries[i].n_columns == o.plan.queries[i].n_columns;
  if (!same)
    return Fail(MGX_ERR_INVALID_ARGUMENT, std::string(entry) + ": page documents need a request of the same shape (the same queries, "
                                          "the same number of columns) on every batch");
  if (!primary->idx->has_pk_bytes || !other->idx->has_pk_bytes)
    return Fail(MGX_ERR_INVALID_ARGUMENT, std::string(entry) + ": page documents need mgx_index_attach_primary_key_bytes on every index");
  return MGX_OK;
}

// Page documents of the score and doc-page groups: the records of the requesting queries' page entries, behind the
// kernel that finalised the page, and their copy to pinned memory (the caller records the batch's done event after it).
// `mapped` / `plain`: as RunHighlight's, each with the batch prepared on it.
static int RunDocuments(mgx_batch* b, hipStream_t s, bool merged, const mgx_batch* mapped, const mgx_batch* plain) {
  mgx_batch::Documents& d = b->doc;
  if (d.early.empty()) return MGX_OK;
  documents::DevBatch db{};
  db.queries = d.d_early.as<documents::DevQuery>();
  db.n_queries = static_cast<uint32_t>(d.early.size());
  db.n_entries = d.plan.early_entries;
  db.arena = d.d_arena.as<uint8_t>();
  db.mapped = DocumentSource(mapped ? mapped->idx : nullptr, mapped, true);
  db.plain = DocumentSource(plain ? plain->idx : nullptr, plain, false);
  db.key_cap = d.plan.key_cap;
  db.merged = merged ? 1u : 0u;
  MGX_LAUNCH(LaunchDocumentGather(db, s));
  MGX_HIP(hipMemcpyAsync(d.h_arena, d.d_arena.p, d.plan.early_bytes, hipMemcpyDeviceToHost, s));
  return MGX_OK;
}

// Page documents of the bitmap group, where its pages are cut (FetchBitmapPages): the page sizes are known on the host,
// so the records are packed by them behind the early queries' and one copy brings exactly those. `pdocs`: the group's
// pages on the device, query i's as the plan places it. The caller's synchronisation covers kernel and copy.
static int RunLateDocuments(mgx_batch* a, hipStream_t s, const pages::Plan& plan, const uint32_t* pdocs) {
  mgx_batch::Documents& d = a->doc;
  mgx_batch* const other = a->merge_other;
  const mgx_batch* mapped = nullptr;
  const mgx_batch* plain = a;  // (one index: its own ids)
  if (other) {
    if (!MainAndDelta(a, &other, 1, &mapped, &plain))
      return Fail(MGX_ERR_NOT_IMPLEMENTED, "mgx_batch_fetch: page documents read one main index and one delta");
    const int rc = CheckDocumentSides(a, other, "mgx_batch_fetch");
    if (rc) return rc;
  }
  std::vector<documents::DevQuery>& late = d.late;  // (a member: the copy below may read it after this returns)
  late.clear();
  uint64_t at = d.plan.early_bytes;
  uint32_t n_entries = 0;
  const mgx_batch::Group& g = a->bitmap;
  for (size_t i = 0; i < g.qids.size(); ++i) {
    if (!d.requested(g.qids[i])) continue;
    const size_t pi = static_cast<size_t>(d.of_query[g.qids[i]]);
    const documents::QueryPlan& qp = d.plan.queries[pi];
    d.fetch_off[pi] = at;
    const uint32_t n = static_cast<uint32_t>(std::min<uint64_t>(plan.queries[i].page_n, qp.limit));
    if (n == 0) continue;
    documents::DevQuery q{};
    q.page_docs = pdocs + plan.queries[i].page_off;
    q.limit = n;
    q.count = n;
    q.entry_begin = n_entries;
    q.n_columns = qp.n_columns;
    q.col_begin = qp.col_begin;
    q.rec_off = at;
    q.rec_stride = qp.rec_stride;
    at += qp.rec_stride * n;
    n_entries += n;
    late.push_back(q);
  }
  if (late.empty()) return MGX_OK;
  if (at > d.plan.arena_bytes) return Fail(MGX_ERR_INTERNAL, "page documents: the records exceed their arena");
  if (d.d_late.bytes < late.size() * sizeof(documents::DevQuery)) return Fail(MGX_ERR_INTERNAL, "page documents: descriptor room");
  MGX_HIP(hipMemcpyAsync(d.d_late.p, late.data(), late.size() * sizeof(documents::DevQuery), hipMemcpyHostToDevice, s));
  documents::DevBatch db{};
  db.queries = d.d_late.as<documents::DevQuery>();
  db.n_queries = static_cast<uint32_t>(late.size());
  db.n_entries = n_entries;
  db.arena = d.d_arena.as<uint8_t>();
  db.mapped = DocumentSource(mapped ? mapped->idx : nullptr, mapped, true);
  db.plain = DocumentSource(plain ? plain->idx : nullptr, plain, false);
  db.key_cap = d.plan.key_cap;
  MGX_LAUNCH(LaunchDocumentGather(db, s));
  const uint64_t e0 = d.plan.early_bytes;
  MGX_HIP(hipMemcpyAsync(static_cast<char*>(d.h_arena) + e0, d.d_arena.as<char>() + e0, at - e0, hipMemcpyDeviceToHost, s));
  return MGX_OK;
}

static int ExecuteImpl(mgx_batch* b, hipStream_t s, const SeedGather* sg = nullptr) {
  mgx_index* idx = b->idx;
  MGX_HIP(hipSetDevice(idx->device));
  {
    int rc = EnsureUploaded(b, s);
    if (rc) return rc;
  }
  // the batch's own conditions into their arena rows, before anything reads an operand: one launch, none without conditions
  MGX_LAUNCH(LaunchFilterCompareBatch(b->d_cond_groups.as<DevCondGroup>(), b->n_cond_groups, b->d_conds.as<DevCondition>(),
                                      idx->dev.n_docs, idx->dev.fb_row_stride, b->cond_arena, s));
  b->merged_shards = false;
  b->merge_other = nullptr;
  b->merged_away = false;
  {  // contribution tables built while this (or any earlier) batch was compiled travel on the index's table stream
    std::lock_guard<std::mutex> lock(idx->table_mu);
    MGX_HIP(FlushTableJobs(idx));
    if (idx->table_ev_recorded) MGX_HIP(hipStreamWaitEvent(s, idx->table_ev, 0));
  }
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  if (b->timing) {
    MGX_HIP(hipEventCreate(&ev0));
    MGX_HIP(hipEventCreate(&ev1));
  }
  bool timed = false;
  if (!b->textdf.qids.empty()) {
    // text-level terms: df pass (unless the caller ran and reduced it), then idf on the host — log() of the host libm,
    // like the reference and the oracle, so that scores stay bit-identical — and back to the device
    if (!b->df_ready) {
      int rc = CountDfImpl(b, s);
      if (rc) return rc;
    }
    b->df_ready = false;
    const size_t n_tt = b->h_text_df.size();
    MGX_HIP(hipMemcpyAsync(b->h_text_df.data(), b->d_text_df.p, n_tt * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
    MGX_HIP(hipMemcpyAsync(b->h_text_df_local.data(), b->d_text_df_local.p, n_tt * sizeof(uint64_t),
                           hipMemcpyDeviceToHost, s));
    MGX_HIP(hipStreamSynchronize(s));
    {
      // h_text_df is what idf is taken from (summed over the ranks when the caller reduced it); the cache learns this
      // shard's own counts only, and a cached count is never put in the place of a reduced one
      std::lock_guard<std::mutex> lock(idx->table_mu);
      for (size_t i = 0; i < n_tt; ++i)
        if (b->text_df_known[i] == ~0ull && idx->df_cache.size() < (1u << 20))
          idx->df_cache.emplace(b->text_df_key[i], b->h_text_df_local[i]);
    }
    for (size_t i = 0; i < n_tt; ++i) {
      // BM25Scorer::ComputeIDF, bm25_scorer.cpp:14-25
      const uint64_t total = b->text_total_docs[i];
      const uint64_t dfc = std::min<uint64_t>(b->h_text_df[i], total);
      const double nn = static_cast<double>(total), df = static_cast<double>(dfc);
      b->h_text_idf[i] = total == 0 ? 0.0 : std::log((nn - df + 0.5) / (df + 0.5) + 1.0);
    }
    MGX_HIP(hipMemcpyAsync(b->d_text_idf.p, b->h_text_idf.data(), n_tt * sizeof(double), hipMemcpyHostToDevice, s));
  }
  if (!b->score.qids.empty()) {
    mgx_batch::Group& g = b->score;
    size_t clear_bytes = b->so_override;
#ifdef MGX_ABLATION
    // (timing experiment: keep the pruning bounds of the batch's previous execute = "the final bound known from the start")
    if (std::getenv("MGX_KEEP_BOUNDS")) clear_bytes = b->score.qids.size() * 8 * 8;
#endif
    MGX_HIP(hipMemsetAsync(b->d_score_out.p, 0, clear_bytes, s));
    if (b->timing) {
      MGX_HIP(hipEventRecord(ev0, s));
    }
    static const bool kChainEnv = !(std::getenv("MGX_CHAIN") && atoi(std::getenv("MGX_CHAIN")) == 0);
    const bool kChain = kChainEnv && idx->fifo.load(std::memory_order_relaxed) != 0;
    if (kChain && b->res_owned) {
      if (!b->res->main_ev) MGX_HIP(hipEventCreateWithFlags(&b->res->main_ev, hipEventDisableTiming));
      std::lock_guard<std::mutex> lock(idx->table_mu);
      if (idx->chain_ev && idx->chain_ev != b->res->main_ev) MGX_HIP(hipStreamWaitEvent(s, idx->chain_ev, 0));
    }
    uint32_t n_fast = 0;
    for (int t = 0; t < kFastMaxScore; ++t) n_fast += g.fast[t].dev.n_items;
    const bool main_work = n_fast != 0 || g.wave.dev.n_items != 0 || g.merge.dev.n_items != 0;
    const bool side_work = g.block.dev.n_items != 0 || g.wave_lists.dev.n_items != 0 || g.cand.dev.n_items != 0;
    hipStream_t side = s;
    if (main_work && side_work) {
      // fork: the (small) shares of the general kernel and of the list-operand plan run on the side stream while the
      // main launch fills the chip
      if (const int rc = ForkSide(b, s)) return rc;
      side = idx->side_stream;
    }
    MGX_LAUNCH(LaunchCand(kModeScore, idx->dev, g.cand.dev, g.cand_leaves, g.cand_instr, g.cand_cap, side));
    MGX_LAUNCH(LaunchWaveScore(idx->dev, g.wave_lists.dev, g.wplan_lists, side));
    MGX_LAUNCH(LaunchTileEval(kModeScore, idx->dev, g.block.dev, g.plan, side, g.n_items_plain, g.n_items_fz));
    // (both conditions are the same on every rank: the collective is entered by all or by none)
    static const uint64_t kMinShardDocs = std::getenv("MGX_SEED_EXCHANGE_MIN_DOCS") ? static_cast<uint64_t>(atoll(std::getenv("MGX_SEED_EXCHANGE_MIN_DOCS"))) : 1000000ull;
    if (sg && sg->fn && g.seed_k != 0 && g.seed_table_docs / static_cast<uint64_t>(sg->world) >= kMinShardDocs) {
      // doc-range shards: a shard's own matches give a weak bound (a 1.25M-doc shard scores 22 % of its matches where
      // the whole table scores 7 %); the seeds of ALL shards together are a sample of the whole table
      for (int t = 0; t < kFastMaxScore; ++t) {
        DevBatch seeds = g.fast[t].dev;
        seeds.n_items = g.n_seed_fast[t];
        MGX_LAUNCH(LaunchBitmapScore(static_cast<uint32_t>(t + 1), idx->dev, seeds, g.fplan, s));
      }
      {
        const int rc = SeedBoundExchange(b, g, *sg, s);
        if (rc) return rc;
      }
      for (int t = 0; t < kFastMaxScore; ++t) {
        DevBatch rest = g.fast[t].dev;
        rest.items += g.n_seed_fast[t];
        rest.n_items -= g.n_seed_fast[t];
        MGX_LAUNCH(LaunchBitmapScore(static_cast<uint32_t>(t + 1), idx->dev, rest, g.fplan, s));
      }
    } else {
      for (int t = 0; t < kFastMaxScore; ++t)
        MGX_LAUNCH(LaunchBitmapScore(static_cast<uint32_t>(t + 1), idx->dev, g.fast[t].dev, g.fplan, s));
    }
    MGX_LAUNCH(LaunchWaveScore(idx->dev, g.wave.dev, g.wplan, s));
    MGX_LAUNCH(LaunchMergeScore(idx->dev, g.merge.dev, g.merge_leaves, g.merge_instr, g.merge_ops, g.merge_cap, s));
    if (side != s) {
      MGX_HIP(hipEventRecord(b->res->join_ev, side));
      MGX_HIP(hipStreamWaitEvent(s, b->res->join_ev, 0));
    }
    if (b->timing) {
      MGX_HIP(hipEventRecord(ev1, s));
      timed = true;
    }
    if (kChain && b->res_owned) {
      std::lock_guard<std::mutex> lock(idx->table_mu);
      MGX_HIP(hipEventRecord(b->res->main_ev, s));
      idx->chain_ev = b->res->main_ev;
    }
    const uint32_t n = static_cast<uint32_t>(g.qids.size());
    MGX_LAUNCH(LaunchMergeTopK(g.dev.queries, g.d_ident.as<uint32_t>(), n, 0, g.dev.cand_keys, g.dev.cand_docs,
                               g.dev.cand_n, /*kq=*/0, /*kj=*/g.dev.cand_stride, /*dj=*/g.dev.cand_stride, /*cq=*/0,
                               /*cj=*/1,
                               b->ex_keys(), b->ex_docs(), b->ex_counts(n), b->top_stride, b->sc_docs(),
                               b->sc_scores(), b->sc_n(), b->page_stride, g.d_list_begin.as<uint32_t>(),
                               b->sc_counters(), b->ex_totals(n), s));
  }
  if (!b->bitmap.qids.empty()) {
    mgx_batch::Group& g = b->bitmap;
    MGX_HIP(hipMemsetAsync(g.d_counters.p, 0, g.d_counters.bytes, s));
    if (b->timing && !timed) {
      MGX_HIP(hipEventRecord(ev0, s));
    }
    MGX_LAUNCH(LaunchTileEval(kModeBitmap, idx->dev, g.block.dev, g.plan, s, g.n_items_plain, g.n_items_fz));
    if (b->timing && !timed) {
      MGX_HIP(hipEventRecord(ev1, s));
      timed = true;
    }
    MGX_LAUNCH(LaunchScanTiles(g.dev.tile_cnt, static_cast<uint32_t>(g.qids.size()), idx->dev.n_tiles,
                               b->d_tile_start.as<uint64_t>(), b->d_totals.as<uint64_t>(), s));
  }
  if (!b->page.qids.empty()) {
    mgx_batch::Group& g = b->page;
    const uint32_t n = static_cast<uint32_t>(g.qids.size());
    MGX_HIP(hipMemsetAsync(b->d_page_out.p, 0, b->po_docs, s));  // counters + totals
    if (b->timing && !timed) {
      MGX_HIP(hipEventRecord(ev0, s));
    }
    // candidate-driven queries (selective: a sparse list drives) beside the tile passes, on the side stream: they write
    // their totals and pages themselves
    const bool cand_side = g.cand.dev.n_items != 0 && (g.wave.dev.n_items != 0 || g.block.dev.n_items != 0) && b->res_owned;
    if (cand_side) {
      if (const int rc = ForkSide(b, s)) return rc;
      MGX_LAUNCH(LaunchCand(kModeDocPage, idx->dev, g.cand.dev, g.cand_leaves, g.cand_instr, 0, idx->side_stream));
      MGX_HIP(hipEventRecord(b->res->join_ev, idx->side_stream));
    }
    MGX_LAUNCH(LaunchWaveCount(idx->dev, g.wave.dev, g.wplan, false, s));
    MGX_LAUNCH(LaunchTileEval(kModeDocCount, idx->dev, g.block.dev, g.plan, s, g.n_items_plain, g.n_items_fz));
    if (b->timing && !timed) {
      MGX_HIP(hipEventRecord(ev1, s));
      timed = true;
    }
    MGX_LAUNCH(LaunchScanTiles(g.dev.tile_cnt, n, idx->dev.n_tiles, b->d_ptile_start.as<uint64_t>(),
                               const_cast<uint64_t*>(g.dev.totals), s, g.d_cand_skip.as<uint8_t>()));
    if (!cand_side) MGX_LAUNCH(LaunchCand(kModeDocPage, idx->dev, g.cand.dev, g.cand_leaves, g.cand_instr, 0, s));
    MGX_LAUNCH(LaunchWavePage(idx->dev, g.page_wave.dev, g.wplan, s));
    MGX_LAUNCH(LaunchTileEval(kModeDocPage, idx->dev, g.page_block.dev, g.plan, s, 0xFFFFFFFFu, g.n_page_fz));
    if (cand_side) MGX_HIP(hipStreamWaitEvent(s, b->res->join_ev, 0));
  }
  if (b->timing) {
    if (timed) {
      b->events.emplace_back(ev0, ev1);
    } else {
      (void)hipEventDestroy(ev0);
      (void)hipEventDestroy(ev1);
    }
  }
  if (b->hl.on() && !b->hl.defer) {
    const int rc = RunHighlight(b, s, /*merged=*/false, nullptr, idx);  // (a page of one index holds that index's own ids)
    if (rc) return rc;
  }
  if (b->fc.on()) {
    const int rc = RunFacets(b, s);
    if (rc) return rc;
  }
  if (b->doc.on() && !b->doc.defer) {
    const int rc = RunDocuments(b, s, /*merged=*/false, nullptr, b);  // (a page of one index holds that index's own ids)
    if (rc) return rc;
  }
  {
    int rc = IssueResultCopy(b, s);
    if (rc) return rc;
  }
  b->executed = true;
  b->fetched = false;
  b->last_stream = s;
  return MGX_OK;
}

// Deep SORT _score: the idf of every scored term in scored-term order (text-level terms: from the batch's df pass).
static std::vector<double> DeepIdfs(const mgx_batch* b, const QuerySpec& sp) {
  std::vector<double> idfs = sp.deep_idfs;
  for (size_t k = 0; k < idfs.size(); ++k)
    if (sp.deep_grams[k] != kNoRow && (sp.deep_grams[k] & kDeepText) != 0)
      idfs[k] = b->h_text_idf[sp.deep_grams[k] & ~kDeepText];
  return idfs;
}

// The bitmap group (limit 0, docid pages past 16384, deep SORT _score): for every query its total and its page, from
// one index, or on a mutable table's primary batch from two (mgx_batch_merge_local: merge_other, the delta's batch)
// with exactly the page an index built from the table's current documents returns.
//   - one synchronisation brings the funnel counters and every side's totals; each side then materialises what the page
//     can need (min(total, limit) in page order for docid pages, every match for limit 0 and for deep SORT _score);
//   - deep SORT _score: each side scores its matches with its own index's columns on local slots; when two sides merge,
//     the delta's slots then become table ids; each side's (key, docid') run is sorted by the bitonic network;
//   - SORT <filter column>: each side's run is its best min(total, offset + limit) (key, docid') pairs under the column's
//     key (mgx_colsort.hpp), docid' already a table id: from column_topk_kernel, which reads the side's result bitmap,
//     when offset + limit <= 1024; otherwise (and under MGX_COLSORT_FULL=1) every match is expanded, keyed by
//     column_keys_kernel and sorted by the bitonic network;
//   - SORT by primary key: the same two paths over the index's key column (mgx_pkey.hpp; an index without keys has no
//     column and the kernels take the table doc id as the value);
//   - rank_merge_kernel cuts every query's page from its sorted, disjoint runs (one per side), in one launch; the pages
//     sorted by primary key come from key_merge_kernel instead when two sides merge and not both hold numeric keys
//     only: their values are ranks in two dictionaries, or a rank and a number, and compare as key strings.
// Everything lives in the batch's d_merge scratch. On the delta's batch of a merge (merged_away) every page is empty:
// the primary's fetch returned them. All sizes, offsets and run descriptors come from pages::Build (mgx_pages.hpp, host
// only); FetchBitmapPages reads the totals, fills the plan's inputs and runs the steps below in the order of this list.
struct BitmapPages {
  std::vector<uint64_t> total, page_off, page_n;
  std::vector<uint32_t> docs;
  std::vector<double> scores;  // (deep SORT _score pages only)
};

// What the steps of one fetch share: its sides, its stream and, once the plan is uploaded, the typed arrays of d_merge.
struct SortCol {
  const uint64_t* values;
  const uint8_t* is_null;
  uint32_t value_class;
};
struct PageSide {
  mgx_batch* batch = nullptr;
  const uint32_t* doc_map = nullptr;  // a merge: local slot -> table id; one index returns its own ids
  // SORT by primary key: the index's key column (no keys set: no values, the value is the table doc id)
  pkey::KeySide keys{pkey::kKeyNumeric, nullptr, nullptr};
  const uint64_t* key_values = nullptr;
  std::map<uint32_t, SortCol> columns;  // every sort column its queries name (pages::kKeyColumn: the key column), looked up once
  std::vector<uint64_t> take, out_off;  // (sources of ExpandSides' copies: they live until the fetch has synchronised)
  const QuerySpec& spec(size_t i) const { return batch->specs[batch->bitmap.qids[i]]; }
};
struct PageFetch {
  mgx_batch* a = nullptr;
  int n_side = 1;
  size_t n = 0;  // queries of the group
  hipStream_t s = nullptr;
  PageSide side[2];
  std::vector<char> up;  // (source of UploadPlan's copy, likewise)
  char* base = nullptr;
  uint32_t *docs = nullptr, *dprime = nullptr, *pdocs = nullptr;
  uint64_t* keys = nullptr;
  double *scores = nullptr, *pscores = nullptr;
  template <typename T>
  T* at(uint64_t off) const { return reinterpret_cast<T*>(base + off); }
};

// [n, cap) of a run of (key, docid') pairs: padding (0, 0) that sorts to the tail.
static int PadPairs(uint64_t* keys, uint32_t* dprime, uint64_t n, uint64_t cap, hipStream_t s) {
  if (cap > n) {
    MGX_HIP(hipMemsetAsync(keys + n, 0, (cap - n) * 8, s));
    MGX_HIP(hipMemsetAsync(dprime + n, 0, (cap - n) * 4, s));
  }
  return MGX_OK;
}

// One scored run as (key, docid') pairs sorted best first by the bitonic network: keys/dprime[0, n) from docs and
// scores, [n, n2) padding (n2: pages::SortCapacity(n)).
static int SortRun(const uint32_t* docs, const double* scores, uint64_t n, uint64_t n2, int descending, uint64_t* keys,
                   uint32_t* dprime, hipStream_t s) {
  if (const int rc = PadPairs(keys, dprime, n, n2, s)) return rc;
  MGX_LAUNCH(LaunchMakeSortKeys(docs, scores, n, descending, keys, dprime, s));
  MGX_LAUNCH(LaunchSortPairs(keys, dprime, n2, s));
  return MGX_OK;
}

// The one synchronisation of the group: counters of the primary, totals of every side (side k's at totals[k * n]).
static int ReadTotals(const PageFetch& f, std::vector<uint64_t>* totals) {
  mgx_batch::Group& g = f.a->bitmap;
  totals->assign(f.n_side * f.n, 0);
  MGX_HIP(hipMemcpyAsync(g.h_counters.data(), g.d_counters.p, f.n * 8 * sizeof(unsigned long long), hipMemcpyDeviceToHost, f.s));
  for (int k = 0; k < f.n_side; ++k)
    MGX_HIP(hipMemcpyAsync(totals->data() + k * f.n, f.side[k].batch->d_totals.p, f.n * 8, hipMemcpyDeviceToHost, f.s));
  MGX_HIP(hipStreamSynchronize(f.s));
  return MGX_OK;
}

// What pages::Build reads of the two batches. Each side's key column and sort columns are read under that index's lock
// (a column is immutable once added; the vector that holds them may grow).
static pages::Input PlanInput(PageFetch& f, const std::vector<uint64_t>& totals) {
  const mgx_batch* a = f.a;
  const mgx_batch::Group& g = a->bitmap;
  pages::Input in;
  in.n_side = f.n_side;
  in.merged_away = a->merged_away;
  const char* const full_env = std::getenv("MGX_COLSORT_FULL");
  in.colsort_full = full_env != nullptr && full_env[0] != '\0' && full_env[0] != '0';
  in.queries.resize(f.n);
  bool any_pk = false;
  for (size_t i = 0; i < f.n; ++i) {
    const QuerySpec& sp = a->specs[g.qids[i]];
    pages::Query& q = in.queries[i];
    q.deep_score = sp.deep_score;
    q.col_sort = sp.col_sort;
    q.pk_sort = sp.pk_sort;
    q.faceted = a->fc.faceted(g.qids[i]);
    q.reverse = sp.reverse;
    q.offset = sp.offset;
    q.limit = sp.limit;
    q.funnel_total = g.h_counters[i * 8 + 4];
    any_pk = any_pk || (sp.pk_sort && sp.col_sort);
  }
  for (int k = 0; k < f.n_side; ++k) {
    PageSide& x = f.side[k];
    const mgx_index* ix = x.batch->idx;
    std::lock_guard<std::mutex> lock(const_cast<mgx_index*>(ix)->mu);
    in.side[k] = pages::Side{ix->dev.n_tiles, ix->dev.n_docs, ix->dev.first_doc_id};
    if (any_pk && ix->has_pkeys) {
      x.keys = pkey::KeySide{ix->pk_kind, ix->d_pk_off.as<uint64_t>(), ix->d_pk_bytes.as<uint8_t>()};
      x.key_values = ix->d_pk_values.as<uint64_t>();
    }
    for (size_t i = 0; i < f.n; ++i) {
      const QuerySpec& ks = x.spec(i);
      pages::SideQuery& sq = in.queries[i].side[k];
      sq.total = totals[k * f.n + i];
      sq.n_terms = static_cast<uint32_t>(ks.deep_grams.size());
      sq.sort_column = ks.pk_sort ? pages::kKeyColumn : ks.sort_column;
      sq.sort_ranks = ks.sort_ranks;
      sq.sort_bias = ks.sort_bias;
      if (!ks.col_sort) continue;
      if (ks.pk_sort) {
        x.columns[pages::kKeyColumn] = SortCol{x.key_values, nullptr, colsort::kUnsigned};
      } else if (!x.columns.count(ks.sort_column) && ks.sort_column < ix->filter_columns.size()) {
        const mgx_index::FilterColumn& c = *ix->filter_columns[ks.sort_column];
        x.columns[ks.sort_column] = SortCol{c.d_values.as<uint64_t>(), c.d_null.as<uint8_t>(), c.value_class};
      }
    }
  }
  // two sides whose values do not compare as numbers: those pages are merged by key string
  in.merge_by_string = f.n_side == 2 && !(f.side[0].keys.kind == pkey::kKeyNumeric && f.side[1].keys.kind == pkey::kKeyNumeric);
  return in;
}

// Grows d_merge to the plan's layout and uploads its first part as one block: the plan's runs and jobs, with what only
// the batches know filled in (each deep run's terms and idfs, each job's device arrays).
static int UploadPlan(PageFetch& f, const pages::Plan& plan) {
  const pages::Scratch& o = plan.at;
  if (f.a->d_merge.bytes < o.bytes) MGX_HIP(f.a->d_merge.Alloc(o.bytes));
  f.base = static_cast<char*>(f.a->d_merge.p);
  f.docs = f.at<uint32_t>(o.docs);
  f.scores = f.at<double>(o.scores);
  f.keys = f.at<uint64_t>(o.keys);
  f.dprime = f.at<uint32_t>(o.dprime);
  f.pdocs = f.at<uint32_t>(o.pdocs);
  f.pscores = f.at<double>(o.pscores);
  f.up.assign(o.up_bytes, 0);
  char* const up = f.up.data();
  for (size_t i = 0; i < f.n; ++i) {
    std::memcpy(up + i * sizeof(DevMergeRun), &plan.queries[i].run, sizeof(DevMergeRun));
    for (int k = 0; k < f.n_side; ++k) {
      const pages::SidePlan& sp = plan.queries[i].side[k];
      const QuerySpec& ks = f.side[k].spec(i);
      if (sp.key_cap == 0 || !f.side[0].spec(i).deep_score || ks.deep_grams.empty()) continue;
      const std::vector<double> idfs = DeepIdfs(f.side[k].batch, ks);
      std::memcpy(up + o.terms + sp.term_off * 4, ks.deep_grams.data(), ks.deep_grams.size() * 4);
      std::memcpy(up + o.idfs + sp.term_off * 8, idfs.data(), idfs.size() * 8);
    }
  }
  std::memcpy(up + o.run_start, plan.run_start.data(), plan.run_start.size() * 8);
  for (size_t j = 0; j < plan.jobs.size(); ++j) {
    const PageSide& x = f.side[plan.jobs[j].side];
    const auto col = x.columns.find(plan.jobs[j].column);
    if (col == x.columns.end()) return Fail(MGX_ERR_INTERNAL, "sort column vanished");
    colsort::TopkJob job = plan.jobs[j].job;
    job.rbits = x.batch->bitmap.dev.rbits;
    job.doc_map = x.doc_map;
    job.values = col->second.values;
    job.is_null = col->second.is_null;
    job.value_class = col->second.value_class;
    std::memcpy(up + o.jobs + j * sizeof(job), &job, sizeof(job));
  }
  if (!plan.kruns.empty()) std::memcpy(up + o.kruns, plan.kruns.data(), plan.kruns.size() * sizeof(pkey::KeyMergeRun));
  std::memcpy(up + o.krun_start, plan.krun_start.data(), plan.krun_start.size() * 8);
  MGX_HIP(hipMemcpyAsync(f.base, up, o.up_bytes, hipMemcpyHostToDevice, f.s));
  return MGX_OK;
}

// Each side materialises its part (expand_kernel, page order: ascending, or descending for reverse docid pages).
static int ExpandSides(PageFetch& f, const pages::Plan& plan) {
  for (int k = 0; k < f.n_side; ++k) {
    PageSide& x = f.side[k];
    mgx_batch* b = x.batch;
    for (const pages::QueryPlan& qp : plan.queries) {
      x.take.push_back(qp.side[k].take);
      x.out_off.push_back(qp.side[k].docs_off);
    }
    MGX_HIP(hipMemcpyAsync(b->d_take.p, x.take.data(), f.n * 8, hipMemcpyHostToDevice, f.s));
    MGX_HIP(hipMemcpyAsync(b->d_out_off.p, x.out_off.data(), f.n * 8, hipMemcpyHostToDevice, f.s));
    if (plan.expanded[k])
      MGX_LAUNCH(LaunchExpand(b->bitmap.dev.rbits, b->d_tile_start.as<uint64_t>(), b->d_totals.as<uint64_t>(),
                              b->d_take.as<uint64_t>(), b->d_out_off.as<uint64_t>(), b->d_reverse.as<uint32_t>(),
                              static_cast<uint32_t>(f.n), b->idx->dev.n_tiles, b->idx->dev.first_doc_id, f.docs, f.s));
  }
  return MGX_OK;
}

// Deep SORT _score: scores on each side's own columns, by local slot.
static int ScoreDeepRuns(const PageFetch& f, const pages::Plan& plan) {
  const uint32_t* d_terms = f.at<const uint32_t>(plan.at.terms);
  const double* d_idfs = f.at<const double>(plan.at.idfs);
  for (size_t i = 0; i < f.n; ++i)
    for (int k = 0; k < f.n_side; ++k) {
      const pages::SidePlan& sp = plan.queries[i].side[k];
      if (sp.key_cap == 0 || !f.side[0].spec(i).deep_score) continue;
      const mgx_batch* x = f.side[k].batch;
      const QuerySpec& ks = f.side[k].spec(i);
      MGX_LAUNCH(LaunchScoreCandidatesMixed(x->idx->dev, f.docs + sp.docs_off, sp.take, d_terms + sp.term_off,
                                            d_idfs + sp.term_off, static_cast<uint32_t>(ks.deep_grams.size()),
                                            x->d_patterns.as<uint8_t>(), x->d_text_terms.as<DevTextTerm>(), ks.k1, ks.b,
                                            ks.avgdl, f.scores + sp.score_off, f.s));
    }
  return MGX_OK;
}

// SORT <filter column | primary key>, offset + limit <= 1024: the fused selection from the result bitmaps.
static int SelectColumnTopk(const PageFetch& f, const pages::Plan& plan) {
  if (plan.jobs.empty()) return MGX_OK;
  MGX_LAUNCH(LaunchColumnTopk(f.at<const colsort::TopkJob>(plan.at.jobs), static_cast<uint32_t>(plan.jobs.size()),
                              plan.n_groups_total, plan.max_cap, plan.max_job_elems, f.at<uint64_t>(plan.at.lkeys),
                              f.at<uint32_t>(plan.at.ldocs), f.at<uint32_t>(plan.at.ln), f.keys, f.dprime, f.s));
  return MGX_OK;
}

// ... past that: the expanded runs' pairs from local slots, their docid' a table id already (the doc map is read here:
// the slots are gone once RemapToTableIds has run), each run sorted whole.
static int KeyAndSortFullRuns(const PageFetch& f, const pages::Plan& plan) {
  for (size_t i = 0; i < f.n; ++i)
    for (int k = 0; k < f.n_side; ++k) {
      const PageSide& x = f.side[k];
      const pages::SidePlan& sp = plan.queries[i].side[k];
      const QuerySpec& ks = x.spec(i);
      if (!ks.col_sort || sp.key_cap == 0) continue;
      const auto col = x.columns.find(ks.pk_sort ? pages::kKeyColumn : ks.sort_column);
      if (col == x.columns.end()) return Fail(MGX_ERR_INTERNAL, "sort column vanished");
      const SortCol& c = col->second;
      const mgx_index* ix = x.batch->idx;
      uint64_t* keys = f.keys + sp.key_off;
      uint32_t* dprime = f.dprime + sp.key_off;
      if (const int rc = PadPairs(keys, dprime, sp.take, sp.key_cap, f.s)) return rc;
      MGX_LAUNCH(LaunchColumnKeys(f.docs + sp.docs_off, sp.take, c.values, c.is_null, x.doc_map, ix->dev.first_doc_id,
                                  ix->dev.n_docs, c.value_class, ks.sort_ranks, ks.sort_bias,
                                  plan.queries[i].run.descending, keys, dprime, f.s));
      MGX_LAUNCH(LaunchSortPairs(keys, dprime, sp.key_cap, f.s));
    }
  return MGX_OK;
}

// A merge: local slots -> table ids (a delta index numbers its documents in ascending table-id order; one index's fetch
// returns its own ids).
static int RemapToTableIds(const PageFetch& f, const pages::Plan& plan) {
  for (int k = 0; k < f.n_side && f.n_side == 2; ++k) {
    const mgx_index* ix = f.side[k].batch->idx;
    if (ix->d_doc_map.p && plan.expanded[k])
      MGX_LAUNCH(LaunchRemapDocs(f.docs + (k == 0 ? 0 : plan.expanded[0]), plan.expanded[k], ix->d_doc_map.as<uint32_t>(),
                                 ix->dev.first_doc_id, ix->dev.n_docs, f.s));
  }
  return MGX_OK;
}

// Deep SORT _score: (key, docid') runs, each sorted best first.
static int SortDeepRuns(const PageFetch& f, const pages::Plan& plan) {
  for (size_t i = 0; i < f.n; ++i)
    for (int k = 0; k < f.n_side; ++k) {
      const pages::SidePlan& sp = plan.queries[i].side[k];
      if (sp.key_cap == 0 || !f.side[0].spec(i).deep_score) continue;
      const int rc = SortRun(f.docs + sp.docs_off, f.scores + sp.score_off, sp.take, sp.key_cap,
                             plan.queries[i].run.descending, f.keys + sp.key_off, f.dprime + sp.key_off, f.s);
      if (rc) return rc;
    }
  return MGX_OK;
}

// Every query's page from its runs: by rank, or (SORT by primary key across two dictionaries) by key string.
static int CutPages(const PageFetch& f, const pages::Plan& plan) {
  MGX_LAUNCH(LaunchRankMerge(f.at<const DevMergeRun>(0), f.at<const uint64_t>(plan.at.run_start), static_cast<uint32_t>(f.n),
                             plan.elems, f.docs, f.keys, f.dprime, f.pdocs, f.pscores, f.s));
  MGX_LAUNCH(LaunchKeyMerge(f.at<const pkey::KeyMergeRun>(plan.at.kruns), f.at<const uint64_t>(plan.at.krun_start),
                            static_cast<uint32_t>(plan.kruns.size()), plan.kelems, f.side[0].keys, f.side[1].keys, f.keys,
                            f.dprime, f.pdocs, f.pscores, f.s));
  return MGX_OK;
}

static int FetchBitmapPages(mgx_batch* a, BitmapPages* m) {
  PageFetch f;
  f.a = a;
  f.n_side = a->merge_other ? 2 : 1;
  f.n = a->bitmap.qids.size();
  f.s = f.n_side == 2 ? a->merge_stream : a->last_stream;
  f.side[0].batch = a;
  f.side[1].batch = a->merge_other;
  for (int k = 0; k < f.n_side; ++k) {
    if (f.n_side == 2) f.side[k].doc_map = f.side[k].batch->idx->d_doc_map.as<uint32_t>();
    if (f.side[k].batch->last_stream != f.s) MGX_HIP(hipStreamSynchronize(f.side[k].batch->last_stream));
  }
  std::vector<uint64_t> totals;
  if (const int rc0 = ReadTotals(f, &totals)) return rc0;
  const pages::Plan plan = pages::Build(PlanInput(f, totals));
  for (const pages::QueryPlan& qp : plan.queries) {
    m->total.push_back(qp.total);
    m->page_off.push_back(qp.page_off);
    m->page_n.push_back(qp.page_n);
  }
  if (plan.status == pages::kEmpty) return MGX_OK;  // every page is empty
  if (plan.status == pages::kTooLarge) return Fail(MGX_ERR_OUT_OF_RANGE, "batch result exceeds 2^32 doc ids");
  if (std::getenv("MGX_VERBOSE")) {
    if (!plan.jobs.empty() || plan.full_runs)
      fprintf(stderr, "[mgx] column sort: %zu fused runs in %u workgroups, %zu full-sort runs\n", plan.jobs.size(),
              plan.n_groups_total, plan.full_runs);
    if (!plan.kruns.empty())
      fprintf(stderr, "[mgx] key merge: %zu queries, %llu elements\n", plan.kruns.size(), static_cast<unsigned long long>(plan.kelems));
  }
  int rc = UploadPlan(f, plan);
  if (!rc) rc = ExpandSides(f, plan);
  if (!rc) rc = ScoreDeepRuns(f, plan);
  if (!rc) rc = SelectColumnTopk(f, plan);
  if (!rc) rc = KeyAndSortFullRuns(f, plan);
  if (!rc) rc = RemapToTableIds(f, plan);
  if (!rc) rc = SortDeepRuns(f, plan);
  if (!rc) rc = CutPages(f, plan);
  if (!rc && a->doc.on()) rc = RunLateDocuments(a, f.s, plan, f.pdocs);  // behind the kernels that cut the pages
  if (rc) return rc;
  m->docs.resize(plan.pages);
  if (plan.pages) MGX_HIP(hipMemcpyAsync(m->docs.data(), f.pdocs, plan.pages * 4, hipMemcpyDeviceToHost, f.s));
  if (plan.pages && plan.n_keys) {  // (scores: a deep SORT _score page is in the batch)
    m->scores.resize(plan.pages);
    MGX_HIP(hipMemcpyAsync(m->scores.data(), f.pscores, plan.pages * 8, hipMemcpyDeviceToHost, f.s));
  }
  MGX_HIP(hipStreamSynchronize(f.s));
  return MGX_OK;
}

static int FetchImpl(mgx_batch* b, mgx_result_view* out) {
  mgx_index* idx = b->idx;
  MGX_HIP(hipSetDevice(idx->device));
  hipStream_t s = b->last_stream;
  // ---- score group: one async copy of the packed result block, then the only synchronisation of the step ----
  const uint32_t* page_n = nullptr;
  const uint32_t* page_docs = nullptr;
  const double* page_scores = nullptr;
  const unsigned long long* override_tot = nullptr;
  if (b->res && b->res->copy_issued) {
    // the copies were enqueued behind the kernels: wait for THIS batch's event only (a later batch may be running).
    // hipEventSynchronize keeps a core busy for the whole wait (with or without hipEventBlockingSync on this runtime:
    // measured 0.85 ms of CPU per 0.85 ms step); a serving loop keeps several batches in flight, so the collecting
    // thread naps between queries of the event instead — tens of microseconds of added latency per batch, no CPU.
    // MGX_WAIT_POLICY=spin restores the busy wait (a caller with one batch in flight who wants the last microseconds).
    static const bool spin = std::getenv("MGX_WAIT_POLICY") != nullptr && std::string(std::getenv("MGX_WAIT_POLICY")) == "spin";
    if (spin) {
      MGX_HIP(hipEventSynchronize(b->res->done_ev));
    } else {
      for (;;) {
        const hipError_t q = hipEventQuery(b->res->done_ev);
        if (q == hipSuccess) break;
        if (q != hipErrorNotReady) return Fail(MGX_ERR_INTERNAL, std::string("hipEventQuery: ") + hipGetErrorString(q));
        std::this_thread::sleep_for(std::chrono::microseconds(20));
      }
    }
  } else {
    if (!b->page.qids.empty())
      MGX_HIP(hipMemcpyAsync(b->h_page_out, b->d_page_out.p, b->po_bytes, hipMemcpyDeviceToHost, s));
    if (!b->score.qids.empty())
      MGX_HIP(hipMemcpyAsync(b->h_score_out, b->d_score_out.p, b->so_bytes, hipMemcpyDeviceToHost, s));
    MGX_HIP(hipStreamSynchronize(s));
  }
  if (!b->score.qids.empty()) {
    mgx_batch::Group& g = b->score;
    const size_t n = g.qids.size();
    const char* h = static_cast<const char*>(b->h_score_out);
    const unsigned long long* hc = reinterpret_cast<const unsigned long long*>(h);
    for (size_t i = 0; i < n * 8; ++i) g.h_counters[i] = hc[i];
    override_tot = reinterpret_cast<const unsigned long long*>(h + b->so_override);
    page_scores = reinterpret_cast<const double*>(h + b->so_scores);
    page_docs = reinterpret_cast<const uint32_t*>(h + b->so_docs);
    page_n = reinterpret_cast<const uint32_t*>(h + b->so_n);
  }
  // ---- bitmap group: totals -> page sizes -> pages ----
  BitmapPages bm;
  if (!b->bitmap.qids.empty()) {
    int rc = FetchBitmapPages(b, &bm);
    if (rc) return rc;
  }
  const uint32_t* dp_docs = nullptr;
  const unsigned long long* dp_totals = nullptr;
  if (!b->page.qids.empty()) {
    const char* h = static_cast<const char*>(b->h_page_out);
    const unsigned long long* hc = reinterpret_cast<const unsigned long long*>(h);
    for (size_t i = 0; i < b->page.qids.size() * 8; ++i) b->page.h_counters[i] = hc[i];
    dp_docs = reinterpret_cast<const uint32_t*>(h + b->po_docs);
    dp_totals = reinterpret_cast<const unsigned long long*>(h + b->po_totals);
  }
  // ---- assemble in batch order ----
  std::vector<uint32_t> pos_in_group(b->n_queries, 0);
  for (size_t i = 0; i < b->score.qids.size(); ++i) pos_in_group[b->score.qids[i]] = static_cast<uint32_t>(i);
  for (size_t i = 0; i < b->bitmap.qids.size(); ++i) pos_in_group[b->bitmap.qids[i]] = static_cast<uint32_t>(i);
  for (size_t i = 0; i < b->page.qids.size(); ++i) pos_in_group[b->page.qids[i]] = static_cast<uint32_t>(i);
  // two passes: sizes first, then bulk copies (a page-mode batch returns ~10^6 doc ids per fetch)
  uint64_t n_out = 0;
  for (uint32_t qi = 0; qi < b->n_queries; ++qi) {
    mgx_query_result& r = b->h_results[qi];
    const uint32_t gi = pos_in_group[qi];
    const bool sc = b->specs[qi].mode == kModeScore, pg = b->specs[qi].mode == kModeDocPage;
    const unsigned long long* c =
        (sc ? b->score : pg ? b->page : b->bitmap).h_counters.data() + static_cast<size_t>(gi) * 8;
    r.total_candidates = c[0];
    r.after_intersection = c[1];
    r.after_not = c[2];
    r.after_filters = c[3];
    r.total = c[4];
    if (sc && b->merged_shards) r.total = override_tot[gi];
    if (pg && b->merged_shards) r.total = dp_totals[gi];
    if (!sc && !pg) r.total = bm.total[gi];
    r.n_docs = sc   ? page_n[gi]
               : pg ? static_cast<uint32_t>(std::min<uint64_t>(r.total, b->specs[qi].limit))
                    : static_cast<uint32_t>(bm.page_n[gi]);
    r.docs_begin = static_cast<uint32_t>(n_out);
    n_out += r.n_docs;
  }
  if (n_out > 0xFFFFFFFFull) return Fail(MGX_ERR_OUT_OF_RANGE, "batch result exceeds 2^32 doc ids");
  b->h_docs.resize(n_out);
  b->h_scores.assign(n_out, 0.0);
  for (uint32_t qi = 0; qi < b->n_queries; ++qi) {
    const mgx_query_result& r = b->h_results[qi];
    if (r.n_docs == 0) continue;
    const uint32_t gi = pos_in_group[qi];
    const uint32_t mode = b->specs[qi].mode;
    uint32_t* dst = b->h_docs.data() + r.docs_begin;
    if (mode == kModeScore) {
      std::memcpy(dst, page_docs + static_cast<size_t>(gi) * b->page_stride, r.n_docs * sizeof(uint32_t));
      std::memcpy(b->h_scores.data() + r.docs_begin, page_scores + static_cast<size_t>(gi) * b->page_stride,
                  r.n_docs * sizeof(double));
    } else if (mode == kModeDocPage) {
      std::memcpy(dst, dp_docs + static_cast<size_t>(gi) * b->doc_page_stride, r.n_docs * sizeof(uint32_t));
    } else {
      std::memcpy(dst, bm.docs.data() + bm.page_off[gi], r.n_docs * sizeof(uint32_t));
      if (b->specs[qi].deep_score)
        std::memcpy(b->h_scores.data() + r.docs_begin, bm.scores.data() + bm.page_off[gi], r.n_docs * sizeof(double));
    }
  }
  out->n_queries = b->n_queries;
  out->queries = b->h_results.data();
  out->docs = b->h_docs.data();
  out->scores = b->h_scores.data();
  b->fetched = true;
  return MGX_OK;
}

}  // namespace mgx

extern "C" {

int mgx_batch_prepare(mgx_index* idx, const mgx_query* queries, uint32_t n_queries, mgx_batch** out) {
  if (out) *out = nullptr;
  if (!idx || !out || (n_queries && !queries))
    return mgx::Fail(MGX_ERR_INVALID_ARGUMENT, "mgx_batch_prepare: null argument");
  try {
    std::vector<mgx::QuerySpec> specs(n_queries);
    const int rc = mgx::CompileAll(idx, queries, n_queries, &specs);
    if (rc) return rc;
    return mgx::PrepareFromSpecs(idx, std::move(specs), out);
  } catch (const std::exception& e) {
    return mgx::Fail(MGX_ERR_INTERNAL, std::string("mgx_batch_prepare: ") + e.what());
  }
}

int mgx_batch_reset(mgx_batch* batch, const mgx_query* queries, uint32_t n_queries) {
  if (!batch || (n_queries && !queries)) return mgx::Fail(MGX_ERR_INVALID_ARGUMENT, "mgx_batch_reset: null argument");
  try {
    mgx_index* idx = batch->idx;
    std::vector<mgx::QuerySpec> specs = std::move(batch->specs);  // (their vectors' storage is compiled into again)
    specs.resize(n_queries);
    int rc = MGX_OK;
    static const bool kTrace = std::getenv("MGX_TRACE_HOST") != nullptr;
    const auto t0 = std::chrono::steady_clock::now();
    rc = mgx::CompileAll(idx, queries, n_queries, &specs);
    const auto t1 = std::chrono::steady_clock::now();
    MGX_HIP(hipSetDevice(idx->device));
    mgx::ResetBatch(batch);
    if (rc) return rc;  // (the batch is empty but usable)
    rc = mgx::PrepareInto(batch, idx, std::move(specs));
    if (kTrace) {
      static std::atomic<uint64_t> n{0};
      static std::atomic<uint64_t> us_compile{0}, us_into{0};
      const auto t2 = std::chrono::steady_clock::now();
      us_compile += std::chrono::duration_cast<std::chrono::microseconds>(t1 - t0).count();
      us_into += std::chrono::duration_cast<std::chrono::microseconds>(t2 - t1).count();
      static const uint64_t period = std::max(1, atoi(std::getenv("MGX_TRACE_HOST")) > 1 ? atoi(std::getenv("MGX_TRACE_HOST")) : 64);
      if (++n % period == 0) {
        const double per = static_cast<double>(period);
        fprintf(stderr, "[mgx] reset x%llu: CompileQuery loop %.3f ms, reset + PrepareInto %.3f ms per batch\n",
                static_cast<unsigned long long>(period), us_compile.exchange(0) / (per * 1e3), us_into.exchange(0) / (per * 1e3));
        for (int k = 0; k < mgx::kSections; ++k)
          fprintf(stderr, "[mgx]   %-24s %.3f ms\n", mgx::kSectionNames[k], mgx::g_section_us[k].exchange(0) / (per * 1e6));
      }
    }
    return rc;
  } catch (const std::exception& e) {
    return mgx::Fail(MGX_ERR_INTERNAL, std::string("mgx_batch_reset: ") + e.what());
  }
}

int mgx_batch_stream(mgx_batch* batch, void** hip_stream) {
  if (hip_stream) *hip_stream = nullptr;
  if (!batch || !hip_stream || !batch->res) return mgx::Fail(MGX_ERR_INVALID_ARGUMENT, "mgx_batch_stream: null argument");
  if (!batch->res->stream) {
    MGX_HIP(hipSetDevice(batch->idx->device));
    MGX_HIP(hipStreamCreateWithFlags(&batch->res->stream, hipStreamNonBlocking));
  }
  *hip_stream = batch->res->stream;
  return MGX_OK;
}

int mgx_batch_execute(mgx_batch* batch, void* hip_stream) {
  if (!batch) return mgx::Fail(MGX_ERR_INVALID_ARGUMENT, "mgx_batch_execute: null batch");
  try {
    hipStream_t s = nullptr;
    int rc = mgx::BatchStream(batch, hip_stream, &s);
    if (rc) return rc;
    return mgx::ExecuteImpl(batch, s);
  } catch (const std::exception& e) {
    return mgx::Fail(MGX_ERR_INTERNAL, std::string("mgx_batch_execute: ") + e.what());
  }
}

int mgx_batch_fetch(mgx_batch* batch, mgx_result_view* out) {
  if (out) std::memset(out, 0, sizeof(*out));
  if (!batch || !out) return mgx::Fail(MGX_ERR_INVALID_ARGUMENT, "mgx_batch_fetch: null argument");
  if (!batch->executed) return mgx::Fail(MGX_ERR_INVALID_ARGUMENT, "mgx_batch_fetch: batch was never executed");
  try {
    return mgx::FetchImpl(batch, out);
  } catch (const std::exception& e) {
    return mgx::Fail(MGX_ERR_INTERNAL, std::string("mgx_batch_fetch: ") + e.what());
  }
}

int mgx_batch_set_highlight(mgx_batch* batch, const mgx_highlight_request* requests, uint32_t n_queries,
                            uint32_t max_text_bytes) {
  namespace hl = mgx::highlight;
  if (!batch || (n_queries && !requests)) return mgx::Fail(MGX_ERR_INVALID_ARGUMENT, "mgx_batch_set_highlight: null argument");
  if (!batch->res_owned) return mgx::Fail(MGX_ERR_INVALID_ARGUMENT, "mgx_batch_set_highlight: not a prepared batch object");
  if (n_queries != batch->n_queries)
    return mgx::Fail(MGX_ERR_INVALID_ARGUMENT, "mgx_batch_set_highlight: one request per query of the batch");
  if (batch->res->uploaded || batch->executed || batch->hl.on())
    return mgx::Fail(MGX_ERR_INVALID_ARGUMENT, "mgx_batch_set_highlight: call it once, after prepare / reset and before the first execute");
  {
    bool any_hl = false;
    for (uint32_t qi = 0; qi < n_queries; ++qi) any_hl = any_hl || requests[qi].enabled;
    if (any_hl)
      for (const mgx::QuerySpec& sp : batch->specs)
        if (sp.col_sort || sp.pk_sort)
          return mgx::Fail(MGX_ERR_NOT_IMPLEMENTED, "mgx_batch_set_highlight: a highlighted batch that holds a query sorted by a filter column or by the primary key is not implemented");
  }
  try {
    mgx_index* idx = batch->idx;
    std::vector<mgx::DevHlQuery> queries;
    std::vector<int32_t> of_query(n_queries, -1);
    std::vector<mgx::DevHlTerm> terms;
    std::string pool;
    std::vector<uint32_t> pos_in_group(n_queries, 0);
    for (size_t i = 0; i < batch->score.qids.size(); ++i) pos_in_group[batch->score.qids[i]] = static_cast<uint32_t>(i);
    for (size_t i = 0; i < batch->page.qids.size(); ++i) pos_in_group[batch->page.qids[i]] = static_cast<uint32_t>(i);
    const uint32_t longest =
        max_text_bytes ? max_text_bytes : std::max(idx->max_text_bytes, idx->originals.kind ? idx->max_original_bytes : 0u);
    uint64_t arena = 0;
    uint32_t n_entries = 0;
    for (uint32_t qi = 0; qi < n_queries; ++qi) {
      const mgx_highlight_request& r = requests[qi];
      if (!r.enabled) continue;
      const std::string who = "mgx_batch_set_highlight: query " + std::to_string(qi) + ": ";
      if (!idx->dev.text) return mgx::Fail(MGX_ERR_INVALID_ARGUMENT, who + "highlight without mgx_index_attach_text");
      if (r.snippet_length < 1 || r.snippet_length > hl::kMaxSnippetLength)
        return mgx::Fail(MGX_ERR_OUT_OF_RANGE, who + "snippet_length must be 1..10000");
      if (r.max_fragments < 1 || r.max_fragments > hl::kMaxFragments)
        return mgx::Fail(MGX_ERR_OUT_OF_RANGE, who + "max_fragments must be 1..100");
      if (r.n_terms && (!r.terms || !r.term_lens)) return mgx::Fail(MGX_ERR_INVALID_ARGUMENT, who + "null term list");
      const mgx::QuerySpec& sp = batch->specs[qi];
      if (sp.limit == 0) return mgx::Fail(MGX_ERR_OUT_OF_RANGE, who + "a highlighted query needs a page (limit 0 returns every match)");
      const bool score = sp.mode == mgx::kModeScore, page = sp.mode == mgx::kModeDocPage;
      if ((!score && !page) || static_cast<uint64_t>(sp.offset) + sp.limit > mgx::kMaxNeeded)
        return mgx::Fail(MGX_ERR_OUT_OF_RANGE, who + "a highlighted query's offset + limit must not exceed 1024");
      mgx::DevHlQuery q{};
      const uint32_t gi = pos_in_group[qi];
      if (score) {
        q.page_docs = batch->sc_docs() + static_cast<size_t>(gi) * batch->page_stride;
        q.page_n = batch->sc_n() + gi;
      } else {
        q.page_docs = batch->page.dev.page_docs + static_cast<size_t>(gi) * batch->doc_page_stride;
        q.total_exec = static_cast<const unsigned long long*>(batch->d_page_out.p) + static_cast<size_t>(gi) * 8 + 4;
        q.total_merged = reinterpret_cast<const unsigned long long*>(batch->page.dev.totals) + gi;
      }
      q.limit = sp.limit;
      q.entry_begin = n_entries;
      q.snippet_length = r.snippet_length;
      q.max_fragments = r.max_fragments;
      q.term_begin = static_cast<uint32_t>(terms.size());
      uint32_t shortest = 0xFFFFFFFFu;
      for (uint32_t t = 0; t < r.n_terms; ++t) {
        const uint32_t len = r.term_lens[t];
        if (len == 0) continue;  // (highlighter.cpp:257-259)
        if (!r.terms[t]) return mgx::Fail(MGX_ERR_INVALID_ARGUMENT, who + "null term");
        if (len > longest) continue;  // longer than every text (:260-262)
        terms.push_back(mgx::DevHlTerm{static_cast<uint32_t>(pool.size()), len, hl::CountCps(r.terms[t], len), 0});
        pool.append(reinterpret_cast<const char*>(r.terms[t]), len);
        shortest = std::min(shortest, len);
      }
      q.n_terms = static_cast<uint32_t>(terms.size()) - q.term_begin;
      if (q.n_terms > MGX_HIGHLIGHT_MAX_TERMS)
        return mgx::Fail(MGX_ERR_OUT_OF_RANGE, who + "more than 256 highlight terms");
      if (pool.size() > 0x7FFFFFFFull) return mgx::Fail(MGX_ERR_OUT_OF_RANGE, who + "highlight terms exceed 2 GiB");
      // worst case of one entry: its windows are disjoint pieces of one text, max_fragments of them, of snippet_length
      // code points (4 bytes at most) each; a window of L code points holds at most L matches, and non-overlapping
      // matches of terms of `shortest` bytes or more are at most text bytes / shortest
      const uint64_t fl = static_cast<uint64_t>(r.snippet_length) * r.max_fragments;
      q.byte_cap = static_cast<uint32_t>(std::min<uint64_t>(4 * fl, longest));
      q.span_cap = q.n_terms ? static_cast<uint32_t>(std::min<uint64_t>(fl, longest / shortest)) : 0;
      q.rec_off = arena;
      q.rec_stride = sizeof(hl::Header) + sizeof(hl::Window) * q.max_fragments + sizeof(hl::Span) * q.span_cap +
                     ((static_cast<uint64_t>(q.byte_cap) + 7) & ~7ull);
      arena += q.rec_stride * q.limit;
      if (arena > MGX_HIGHLIGHT_ARENA_CAP)
        return mgx::Fail(MGX_ERR_OUT_OF_RANGE,
                         "mgx_batch_set_highlight: the batch's highlight records can exceed MGX_HIGHLIGHT_ARENA_CAP (256 MiB) "
                         "in the worst case; lower snippet_length (or max_fragments, or limit), or highlight fewer queries "
                         "per batch (query " + std::to_string(qi) + " needs " + std::to_string(q.rec_stride) + " bytes per page entry)");
      n_entries += q.limit;
      of_query[qi] = static_cast<int32_t>(queries.size());
      queries.push_back(q);
    }
    if (queries.empty()) return MGX_OK;  // nothing is highlighted: the batch launches and copies nothing new
    mgx::ResourceScope scope(batch->res);
    MGX_HIP(hipSetDevice(idx->device));
    mgx_batch::Highlight& h = batch->hl;
    MGX_HIP(mgx::Upload(h.d_queries, queries.data(), queries.size()));
    MGX_HIP(mgx::Upload(h.d_terms, terms.data(), terms.size(), 1));
    MGX_HIP(mgx::Upload(h.d_patterns, reinterpret_cast<const uint8_t*>(pool.data()), pool.size(), 16));
    MGX_HIP(h.d_arena.Alloc(arena));
    MGX_HIP(batch->res->Pinned(2, arena, &h.h_arena));
    h.bytes = arena;
    h.n_entries = n_entries;
    h.of_query = std::move(of_query);
    h.queries = std::move(queries);
    return MGX_OK;
  } catch (const std::exception& e) {
    return mgx::Fail(MGX_ERR_INTERNAL, std::string("mgx_batch_set_highlight: ") + e.what());
  }
}

int mgx_batch_defer_highlight(mgx_batch* batch, int defer) {
  if (!batch) return mgx::Fail(MGX_ERR_INVALID_ARGUMENT, "mgx_batch_defer_highlight: null batch");
  batch->hl.defer = defer != 0;
  return MGX_OK;
}

int mgx_batch_fetch_highlight(mgx_batch* batch, mgx_highlight_view* out) {
  namespace hl = mgx::highlight;
  if (out) std::memset(out, 0, sizeof(*out));
  if (!batch || !out) return mgx::Fail(MGX_ERR_INVALID_ARGUMENT, "mgx_batch_fetch_highlight: null argument");
  if (!batch->executed || !batch->fetched)
    return mgx::Fail(MGX_ERR_INVALID_ARGUMENT, "mgx_batch_fetch_highlight: call mgx_batch_fetch for this execute first");
  try {
    mgx_batch::Highlight& h = batch->hl;
    h.entries.assign(batch->h_docs.size(), mgx_highlight_entry{});
    for (uint32_t qi = 0; qi < batch->n_queries && h.on(); ++qi) {
      if (h.of_query[qi] < 0) continue;
      const mgx::DevHlQuery& q = h.queries[h.of_query[qi]];
      const mgx_query_result& r = batch->h_results[qi];
      for (uint32_t j = 0; j < r.n_docs && j < q.limit; ++j) {
        const uint8_t* rec = static_cast<const uint8_t*>(h.h_arena) + q.rec_off + static_cast<uint64_t>(j) * q.rec_stride;
        hl::Header head;
        std::memcpy(&head, rec, sizeof(head));
        if ((head.flags & hl::kFlagOverflow) || head.n_windows > q.max_fragments || head.n_spans > q.span_cap ||
            head.n_bytes > q.byte_cap)
          return mgx::Fail(MGX_ERR_OUT_OF_RANGE,
                           "mgx_batch_fetch_highlight: a page entry's text is longer than the max_text_bytes the records "
                           "were sized for (or is not valid UTF-8)");
        mgx_highlight_entry& e = h.entries[r.docs_begin + j];
        e.n_windows = head.n_windows;
        e.flags = head.flags;
        e.n_spans = head.n_spans;
        e.n_bytes = head.n_bytes;
        e.windows = reinterpret_cast<const mgx_highlight_window*>(rec + sizeof(hl::Header));
        e.spans = reinterpret_cast<const mgx_highlight_span*>(rec + sizeof(hl::Header) + sizeof(hl::Window) * q.max_fragments);
        e.bytes = reinterpret_cast<const uint8_t*>(e.spans) + sizeof(hl::Span) * q.span_cap;
      }
    }
    out->n_entries = static_cast<uint32_t>(h.entries.size());
    out->entries = h.entries.data();
    return MGX_OK;
  } catch (const std::exception& e) {
    return mgx::Fail(MGX_ERR_INTERNAL, std::string("mgx_batch_fetch_highlight: ") + e.what());
  }
}

static_assert(sizeof(mgx_highlight_window) == sizeof(mgx::highlight::Window) &&
                  offsetof(mgx_highlight_window, start) == offsetof(mgx::highlight::Window, start) &&
                  offsetof(mgx_highlight_window, end) == offsetof(mgx::highlight::Window, end) &&
                  offsetof(mgx_highlight_window, span_end) == offsetof(mgx::highlight::Window, span_end) &&
                  offsetof(mgx_highlight_window, bytes_begin) == offsetof(mgx::highlight::Window, aux) &&
                  sizeof(mgx_highlight_span) == sizeof(mgx::highlight::Span) &&
                  offsetof(mgx_highlight_span, start) == offsetof(mgx::highlight::Span, start) &&
                  offsetof(mgx_highlight_span, end) == offsetof(mgx::highlight::Span, end),
              "the ABI's record structs are the shared header's, field by field");

int mgx_batch_set_facets(mgx_batch* batch, const mgx_facet_request* requests, uint32_t n_queries) {
  namespace fc = mgx::facet;
  if (!batch || (n_queries && !requests)) return mgx::Fail(MGX_ERR_INVALID_ARGUMENT, "mgx_batch_set_facets: null argument");
  if (!batch->res_owned) return mgx::Fail(MGX_ERR_INVALID_ARGUMENT, "mgx_batch_set_facets: not a prepared batch object");
  if (n_queries != batch->n_queries)
    return mgx::Fail(MGX_ERR_INVALID_ARGUMENT, "mgx_batch_set_facets: one request per query of the batch");
  if (batch->res->uploaded || batch->executed || batch->fc.on())
    return mgx::Fail(MGX_ERR_INVALID_ARGUMENT, "mgx_batch_set_facets: call it once, after prepare / reset and before the first execute");
  try {
    mgx_index* idx = batch->idx;
    std::vector<uint32_t> pos_in_group(n_queries, 0);
    for (size_t i = 0; i < batch->bitmap.qids.size(); ++i) pos_in_group[batch->bitmap.qids[i]] = static_cast<uint32_t>(i);
    std::vector<fc::Request> reqs;
    std::vector<const uint32_t*> value_ids;  // of every requested column, in plan order
    for (uint32_t qi = 0; qi < n_queries; ++qi) {
      const mgx_facet_request& r = requests[qi];
      if (r.n_columns == 0) continue;
      const std::string who = "mgx_batch_set_facets: query " + std::to_string(qi) + ": ";
      if (!r.column_ids) return mgx::Fail(MGX_ERR_INVALID_ARGUMENT, who + "null column list");
      if (r.n_columns > MGX_FACET_MAX_COLUMNS)
        return mgx::Fail(MGX_ERR_OUT_OF_RANGE, who + "more than MGX_FACET_MAX_COLUMNS (8) facet columns");
      const mgx::QuerySpec& sp = batch->specs[qi];
      if (sp.mode != mgx::kModeBitmap || sp.limit != 0 || sp.deep_score || sp.col_sort)
        return mgx::Fail(MGX_ERR_INVALID_ARGUMENT,
                         who + "a faceted query must be MGX_SORT_DOCID with limit 0 (it returns counts, not a page)");
      fc::Request rq;
      rq.query = qi;
      rq.row = pos_in_group[qi];
      std::lock_guard<std::mutex> lock(idx->mu);  // (columns are added under mu; the objects themselves never move)
      for (uint32_t c = 0; c < r.n_columns; ++c) {
        const uint32_t id = r.column_ids[c];
        if (id >= idx->filter_columns.size())
          return mgx::Fail(MGX_ERR_OUT_OF_RANGE, who + "unknown filter column " + std::to_string(id));
        const mgx_index::FilterColumn& col = *idx->filter_columns[id];
        if (!col.d_value_ids.p)
          return mgx::Fail(MGX_ERR_INVALID_ARGUMENT, who + "filter column " + std::to_string(id) + " was added without value ids");
        rq.column_ids.push_back(id);
        rq.n_values.push_back(col.n_values);
        value_ids.push_back(col.d_value_ids.as<uint32_t>());
      }
      reqs.push_back(std::move(rq));
    }
    if (reqs.empty()) return MGX_OK;  // nothing is faceted: the batch allocates, launches and copies nothing new
    // MGX_FACET_BALLOT_MAX: the largest column the ballot path takes (tools/bench_facet.py times the paths against each other)
    static const char* const ballot_env = std::getenv("MGX_FACET_BALLOT_MAX");
    const uint32_t ballot_max =
        ballot_env ? std::min<uint32_t>(static_cast<uint32_t>(std::max(0, atoi(ballot_env))), 63u) : fc::kBallotMaxValues;
    fc::Plan plan;
    size_t bad = 0;
    const fc::Status st = fc::Build(reqs, idx->dev.n_tiles, ballot_max, &plan, &bad);
    if (st == fc::kTooManyColumns)
      return mgx::Fail(MGX_ERR_OUT_OF_RANGE, "mgx_batch_set_facets: query " + std::to_string(reqs[bad].query) +
                                                 ": more than MGX_FACET_MAX_COLUMNS (8) facet columns");
    if (st == fc::kArenaTooLarge)
      return mgx::Fail(MGX_ERR_OUT_OF_RANGE,
                       "mgx_batch_set_facets: the batch's counts exceed MGX_FACET_ARENA_CAP (256 MiB) at query " +
                           std::to_string(reqs[bad].query) + "; facet fewer queries or columns per batch");
    mgx::ResourceScope scope(batch->res);
    MGX_HIP(hipSetDevice(idx->device));
    mgx_batch::Facets& f = batch->fc;
    MGX_HIP(f.d_counts.Alloc(plan.arena_bytes));
    MGX_HIP(batch->res->Pinned(3, plan.arena_bytes, &f.h_counts));
    const uint64_t row_words = static_cast<uint64_t>(idx->dev.n_tiles) * mgx::kWordsPerTile;
    std::vector<fc::DevQuery> dq(plan.queries.size());
    std::vector<fc::DevColumn> dc(plan.columns.size());
    std::vector<int32_t> of_query(n_queries, -1);
    for (size_t i = 0; i < plan.queries.size(); ++i) {
      const fc::QueryPlan& q = plan.queries[i];
      of_query[q.query] = static_cast<int32_t>(i);
      dq[i] = fc::DevQuery{q.row * row_words, q.col_begin, q.n_cols, q.lds_bins, 0};
    }
    for (size_t i = 0; i < plan.columns.size(); ++i) {
      const fc::ColumnPlan& c = plan.columns[i];
      dc[i] = fc::DevColumn{value_ids[i], f.d_counts.as<unsigned long long>() + c.count_off, c.n_values, c.lds_begin,
                            c.ballot, 0};
    }
    MGX_HIP(mgx::Upload(f.d_queries, dq.data(), dq.size()));
    MGX_HIP(mgx::Upload(f.d_columns, dc.data(), dc.size()));
    MGX_HIP(mgx::Upload(f.d_items, plan.items.data(), plan.items.size()));
    f.of_query = std::move(of_query);
    f.plan = std::move(plan);
    return MGX_OK;
  } catch (const std::exception& e) {
    return mgx::Fail(MGX_ERR_INTERNAL, std::string("mgx_batch_set_facets: ") + e.what());
  }
}

int mgx_batch_fetch_facets(mgx_batch* batch, mgx_facet_view* out) {
  if (out) std::memset(out, 0, sizeof(*out));
  if (!batch || !out) return mgx::Fail(MGX_ERR_INVALID_ARGUMENT, "mgx_batch_fetch_facets: null argument");
  if (!batch->executed || !batch->fetched)
    return mgx::Fail(MGX_ERR_INVALID_ARGUMENT, "mgx_batch_fetch_facets: call mgx_batch_fetch for this execute first");
  try {
    mgx_batch::Facets& f = batch->fc;
    f.entries.clear();
    for (const mgx::facet::ColumnPlan& c : f.plan.columns) {
      mgx_facet_entry e{};
      e.query = c.query;
      e.column_id = c.column_id;
      e.n_values = c.n_values;
      e.counts = c.n_values ? static_cast<const uint64_t*>(f.h_counts) + c.count_off : nullptr;
      f.entries.push_back(e);
    }
    out->n_entries = static_cast<uint32_t>(f.entries.size());
    out->entries = f.entries.data();
    return MGX_OK;
  } catch (const std::exception& e) {
    return mgx::Fail(MGX_ERR_INTERNAL, std::string("mgx_batch_fetch_facets: ") + e.what());
  }
}

int mgx_batch_set_documents(mgx_batch* batch, const mgx_document_request* requests, uint32_t n_queries,
                            uint32_t max_key_bytes) {
  namespace dc = mgx::documents;
  if (!batch || (n_queries && !requests)) return mgx::Fail(MGX_ERR_INVALID_ARGUMENT, "mgx_batch_set_documents: null argument");
  if (!batch->res_owned) return mgx::Fail(MGX_ERR_INVALID_ARGUMENT, "mgx_batch_set_documents: not a prepared batch object");
  if (n_queries != batch->n_queries)
    return mgx::Fail(MGX_ERR_INVALID_ARGUMENT, "mgx_batch_set_documents: one request per query of the batch");
  if (batch->res->uploaded || batch->executed || batch->doc.on())
    return mgx::Fail(MGX_ERR_INVALID_ARGUMENT, "mgx_batch_set_documents: call it once, after prepare / reset and before the first execute");
  try {
    mgx_index* idx = batch->idx;
    std::vector<dc::Request> reqs;
    std::vector<int32_t> of_query(n_queries, -1);
    std::vector<dc::DevColumn> columns;
    uint32_t longest = max_key_bytes;
    {
      std::lock_guard<std::mutex> lock(idx->mu);  // (a column is immutable once added; the vector that holds them may grow)
      for (uint32_t qi = 0; qi < n_queries; ++qi) {
        const mgx_document_request& r = requests[qi];
        if (!r.enabled) continue;
        const std::string who = "mgx_batch_set_documents: query " + std::to_string(qi) + ": ";
        if (!idx->has_pk_bytes)
          return mgx::Fail(MGX_ERR_INVALID_ARGUMENT, who + "page documents without mgx_index_attach_primary_key_bytes");
        if (r.n_columns > MGX_DOC_MAX_COLUMNS)
          return mgx::Fail(MGX_ERR_OUT_OF_RANGE, who + "more than MGX_DOC_MAX_COLUMNS (32) columns");
        if (r.n_columns && !r.column_ids) return mgx::Fail(MGX_ERR_INVALID_ARGUMENT, who + "null column list");
        if (batch->fc.faceted(qi))
          return mgx::Fail(MGX_ERR_INVALID_ARGUMENT, who + "a faceted query returns counts, not a page: no documents");
        const mgx::QuerySpec& sp = batch->specs[qi];
        if (sp.limit == 0 || sp.limit > MGX_DOC_MAX_LIMIT)
          return mgx::Fail(MGX_ERR_OUT_OF_RANGE, who + "page documents need a page of 1..1024 entries (limit)");
        for (uint32_t c = 0; c < r.n_columns; ++c) {
          const uint32_t id = r.column_ids[c];
          dc::DevColumn col{nullptr, nullptr};
          if (id != MGX_DOC_NO_COLUMN) {
            if (id >= idx->filter_columns.size()) return mgx::Fail(MGX_ERR_OUT_OF_RANGE, who + "unknown filter column");
            const mgx_index::FilterColumn& fc = *idx->filter_columns[id];
            col.values = fc.d_values.as<uint64_t>();
            col.is_null = fc.d_null.as<uint8_t>();
          }
          columns.push_back(col);
        }
        dc::Request rq;
        rq.query = qi;
        rq.limit = sp.limit;
        rq.n_columns = r.n_columns;
        rq.late = (sp.mode == mgx::kModeScore || sp.mode == mgx::kModeDocPage) ? 0u : 1u;
        of_query[qi] = static_cast<int32_t>(reqs.size());
        reqs.push_back(rq);
      }
      if (longest == 0) longest = idx->max_pk_bytes;
    }
    if (reqs.empty()) return MGX_OK;  // nothing is requested: the batch allocates, launches and copies nothing new
    dc::Plan plan;
    size_t bad = 0;
    switch (dc::Build(reqs, longest, &plan, &bad)) {
      case dc::kOk:
        break;
      case dc::kTooManyColumns:
        return mgx::Fail(MGX_ERR_OUT_OF_RANGE, "mgx_batch_set_documents: query " + std::to_string(reqs[bad].query) +
                                                   ": more than MGX_DOC_MAX_COLUMNS (32) columns");
      case dc::kBadLimit:
        return mgx::Fail(MGX_ERR_OUT_OF_RANGE, "mgx_batch_set_documents: query " + std::to_string(reqs[bad].query) +
                                                   ": page documents need a page of 1..1024 entries (limit)");
      case dc::kArenaTooLarge:
        return mgx::Fail(MGX_ERR_OUT_OF_RANGE,
                         "mgx_batch_set_documents: the batch's records can exceed MGX_DOC_ARENA_CAP (256 MiB) at query " +
                             std::to_string(reqs[bad].query) + " (" +
                             std::to_string(dc::RecordStride(reqs[bad].n_columns, longest)) +
                             " bytes per page entry); lower limit (or max_key_bytes, or the columns), or request the "
                             "documents of fewer queries per batch");
    }
    std::vector<uint32_t> pos_in_group(n_queries, 0);
    for (size_t i = 0; i < batch->score.qids.size(); ++i) pos_in_group[batch->score.qids[i]] = static_cast<uint32_t>(i);
    for (size_t i = 0; i < batch->page.qids.size(); ++i) pos_in_group[batch->page.qids[i]] = static_cast<uint32_t>(i);
    std::vector<dc::DevQuery> early;
    size_t n_late = 0;
    for (const dc::QueryPlan& qp : plan.queries) {
      if (qp.late) {
        ++n_late;
        continue;
      }
      const mgx::QuerySpec& sp = batch->specs[qp.query];
      const uint32_t gi = pos_in_group[qp.query];
      dc::DevQuery q{};
      if (sp.mode == mgx::kModeScore) {
        q.page_docs = batch->sc_docs() + static_cast<size_t>(gi) * batch->page_stride;
        q.page_n = batch->sc_n() + gi;
      } else {
        q.page_docs = batch->page.dev.page_docs + static_cast<size_t>(gi) * batch->doc_page_stride;
        q.total_exec = static_cast<const unsigned long long*>(batch->d_page_out.p) + static_cast<size_t>(gi) * 8 + 4;
        q.total_merged = reinterpret_cast<const unsigned long long*>(batch->page.dev.totals) + gi;
      }
      q.limit = qp.limit;
      q.entry_begin = qp.entry_begin;
      q.n_columns = qp.n_columns;
      q.col_begin = qp.col_begin;
      q.rec_off = qp.rec_off;
      q.rec_stride = qp.rec_stride;
      early.push_back(q);
    }
    mgx::ResourceScope scope(batch->res);
    MGX_HIP(hipSetDevice(idx->device));
    mgx_batch::Documents& d = batch->doc;
    if (!early.empty()) MGX_HIP(mgx::Upload(d.d_early, early.data(), early.size()));
    MGX_HIP(mgx::Upload(d.d_columns, columns.data(), columns.size(), 1));
    if (n_late) MGX_HIP(d.d_late.Alloc(n_late * sizeof(dc::DevQuery)));
    MGX_HIP(d.d_arena.Alloc(plan.arena_bytes));
    MGX_HIP(batch->res->Pinned(4, plan.arena_bytes, &d.h_arena));
    d.fetch_off.resize(plan.queries.size());
    for (size_t i = 0; i < plan.queries.size(); ++i) d.fetch_off[i] = plan.queries[i].rec_off;
    d.of_query = std::move(of_query);
    d.early = std::move(early);
    d.plan = std::move(plan);
    return MGX_OK;
  } catch (const std::exception& e) {
    return mgx::Fail(MGX_ERR_INTERNAL, std::string("mgx_batch_set_documents: ") + e.what());
  }
}

int mgx_batch_defer_documents(mgx_batch* batch, int defer) {
  if (!batch) return mgx::Fail(MGX_ERR_INVALID_ARGUMENT, "mgx_batch_defer_documents: null batch");
  batch->doc.defer = defer != 0;
  return MGX_OK;
}

int mgx_batch_fetch_documents(mgx_batch* batch, mgx_document_view* out) {
  namespace dc = mgx::documents;
  if (out) std::memset(out, 0, sizeof(*out));
  if (!batch || !out) return mgx::Fail(MGX_ERR_INVALID_ARGUMENT, "mgx_batch_fetch_documents: null argument");
  if (!batch->executed || !batch->fetched)
    return mgx::Fail(MGX_ERR_INVALID_ARGUMENT, "mgx_batch_fetch_documents: call mgx_batch_fetch for this execute first");
  try {
    mgx_batch::Documents& d = batch->doc;
    d.entries.assign(batch->h_docs.size(), mgx_document_entry{});
    for (uint32_t qi = 0; qi < batch->n_queries && d.on(); ++qi) {
      if (d.of_query[qi] < 0) continue;
      const size_t pi = static_cast<size_t>(d.of_query[qi]);
      const dc::QueryPlan& q = d.plan.queries[pi];
      const mgx_query_result& r = batch->h_results[qi];
      for (uint32_t j = 0; j < r.n_docs && j < q.limit; ++j) {
        const uint8_t* rec = static_cast<const uint8_t*>(d.h_arena) + d.fetch_off[pi] + static_cast<uint64_t>(j) * q.rec_stride;
        dc::Header head;
        std::memcpy(&head, rec, sizeof(head));
        if ((head.flags & dc::kTruncated) || head.key_len > d.plan.key_cap || head.n_columns > q.n_columns)
          return mgx::Fail(MGX_ERR_OUT_OF_RANGE,
                           "mgx_batch_fetch_documents: query " + std::to_string(qi) + ": a page entry's key is longer than "
                           "the max_key_bytes the records were sized for");
        if (!(head.flags & dc::kFound)) continue;  // (a doc id no index of the batch holds: a zero entry)
        mgx_document_entry& e = d.entries[r.docs_begin + j];
        e.flags = head.flags;
        e.key_len = head.key_len;
        e.null_mask = head.null_mask;
        e.n_columns = head.n_columns;
        e.values = reinterpret_cast<const uint64_t*>(rec + sizeof(dc::Header));
        e.key = rec + sizeof(dc::Header) + 8ull * q.n_columns;
      }
    }
    out->n_entries = static_cast<uint32_t>(d.entries.size());
    out->entries = d.entries.data();
    return MGX_OK;
  } catch (const std::exception& e) {
    return mgx::Fail(MGX_ERR_INTERNAL, std::string("mgx_batch_fetch_documents: ") + e.what());
  }
}

static_assert(MGX_DOC_MAX_COLUMNS == mgx::documents::kMaxColumns && MGX_DOC_MAX_LIMIT == mgx::documents::kMaxLimit &&
                  MGX_DOC_ARENA_CAP == mgx::documents::kArenaCap && MGX_DOC_NO_COLUMN == mgx::documents::kNoColumn &&
                  MGX_DOC_FOUND == mgx::documents::kFound && MGX_DOC_HAS_KEY == mgx::documents::kHasKey &&
                  MGX_DOC_MAPPED == mgx::documents::kMapped,
              "the header's constants are the planner's");

int mgx_highlight_render(const mgx_highlight_entry* entry, const uint8_t* open_tag, size_t open_len,
                         const uint8_t* close_tag, size_t close_len, uint8_t* out, size_t cap, size_t* out_len) {
  namespace hl = mgx::highlight;
  if (out_len) *out_len = 0;
  if (!entry || !out_len || (cap && !out) || (open_len && !open_tag) || (close_len && !close_tag))
    return mgx::Fail(MGX_ERR_INVALID_ARGUMENT, "mgx_highlight_render: null argument");
  if (open_len > hl::kMaxTagBytes || close_len > hl::kMaxTagBytes)
    return mgx::Fail(MGX_ERR_OUT_OF_RANGE, "mgx_highlight_render: a tag is at most 256 bytes");
  if ((entry->n_windows && !entry->windows) || (entry->n_spans && !entry->spans) || (entry->n_bytes && !entry->bytes))
    return mgx::Fail(MGX_ERR_INVALID_ARGUMENT, "mgx_highlight_render: null record array");
  for (uint32_t i = 0; i < entry->n_windows; ++i) {  // every window's bytes lie inside the record's byte area
    const mgx_highlight_window& w = entry->windows[i];
    if (w.end < w.start || w.bytes_begin > entry->n_bytes || w.end - w.start > entry->n_bytes - w.bytes_begin)
      return mgx::Fail(MGX_ERR_INVALID_ARGUMENT, "mgx_highlight_render: a window's bytes lie outside the record");
  }
  const hl::Header head{entry->n_windows, entry->flags, entry->n_spans, entry->n_bytes};
  *out_len = hl::Render(head, reinterpret_cast<const hl::Window*>(entry->windows),
                        reinterpret_cast<const hl::Span*>(entry->spans), entry->bytes, false, open_tag, open_len, close_tag,
                        close_len, out, cap);
  return MGX_OK;
}

int mgx_batch_count_df(mgx_batch* batch, void* hip_stream) {
  if (!batch) return mgx::Fail(MGX_ERR_INVALID_ARGUMENT, "mgx_batch_count_df: null batch");
  try {
    hipStream_t s = nullptr;
    int rc = mgx::BatchStream(batch, hip_stream, &s);
    if (rc) return rc;
    rc = mgx::CountDfImpl(batch, s);
    if (rc) return rc;
    batch->df_ready = true;
    return MGX_OK;
  } catch (const std::exception& e) {
    return mgx::Fail(MGX_ERR_INTERNAL, std::string("mgx_batch_count_df: ") + e.what());
  }
}

int mgx_batch_df_buffer(mgx_batch* batch, uint64_t** device_counts, uint32_t* n) {
  if (device_counts) *device_counts = nullptr;
  if (n) *n = 0;
  if (!batch || !device_counts || !n) return mgx::Fail(MGX_ERR_INVALID_ARGUMENT, "mgx_batch_df_buffer: null argument");
  *device_counts = batch->d_text_df.as<uint64_t>();
  *n = static_cast<uint32_t>(batch->h_text_df.size());
  return MGX_OK;
}

// One group of a batch (its SORT _score queries, or its docid-ordered pages) in the exchange layout. The public entry
// points below take uniform batches (one all-gather moves one blob); the local merge of a mutable table takes each group
// of a mixed batch in turn.
// SORT <filter column> on a sharded table: the ranks of a page need every shard's column values
static bool HasColumnSort(const mgx_batch* batch) {
  for (const mgx::QuerySpec& sp : batch->specs)
    if (sp.col_sort || sp.pk_sort) return true;
  return false;
}
static int RefuseColumnSort(const mgx_batch* batch, const char* entry) {
  if (!HasColumnSort(batch)) return MGX_OK;
  return mgx::Fail(MGX_ERR_NOT_IMPLEMENTED, std::string(entry) + ": SORT by a filter column or by the primary key on a sharded table is not implemented: a page's order needs every shard's column values");
}

// (the counts of a sharded table's facets would need an all-reduce across the ranks: out of scope)
// (the rows of a sharded table's page live on other ranks: out of scope)
static int RefuseDocuments(const char* entry) {
  return mgx::Fail(MGX_ERR_NOT_IMPLEMENTED, std::string(entry) + ": page documents (mgx_batch_set_documents) on a sharded table are not implemented: the page's rows live on other ranks");
}
static int RefuseFacets(const char* entry) {
  return mgx::Fail(MGX_ERR_NOT_IMPLEMENTED, std::string(entry) + ": facets (mgx_batch_set_facets) on a sharded table are not implemented: the counts of the shards are not reduced");
}

static int ExportGroup(mgx_batch* batch, bool pages, uint64_t* blob64, uint32_t* blob32, uint32_t* stride, void* hip_stream);
static int MergeGroup(mgx_batch* batch, bool pages, uint32_t n_shards, const uint64_t* blob64, uint64_t pitch64,
                      const uint32_t* blob32, uint64_t pitch32, void* hip_stream);

int mgx_batch_export_topk(mgx_batch* batch, uint64_t* blob64, uint32_t* blob32, uint32_t* stride,
                          void* hip_stream) {
  if (!batch || !stride) return mgx::Fail(MGX_ERR_INVALID_ARGUMENT, "mgx_batch_export_topk: null argument");
  if (batch->fc.on()) return RefuseFacets("mgx_batch_export_topk");
  if (batch->doc.on()) return RefuseDocuments("mgx_batch_export_topk");
  if (batch->hl.on()) return mgx::Fail(MGX_ERR_NOT_IMPLEMENTED, "mgx_batch_export_topk: highlight on a sharded table is not implemented: the page's texts live on other ranks");
  if (const int rc_cs = RefuseColumnSort(batch, "mgx_batch_export_topk")) return rc_cs;
  const bool pages = batch->score.qids.empty() && batch->bitmap.qids.empty() && !batch->page.qids.empty();
  if (!pages && (!batch->bitmap.qids.empty() || !batch->page.qids.empty() || batch->score.qids.empty()))
    return mgx::Fail(MGX_ERR_INVALID_ARGUMENT,
                     "mgx_batch_export_topk: the batch must be all MGX_SORT_SCORE or all docid-ordered pages "
                     "(0 < limit <= 16384)");
  return ExportGroup(batch, pages, blob64, blob32, stride, hip_stream);
}

static int ExportGroup(mgx_batch* batch, bool pages, uint64_t* blob64, uint32_t* blob32, uint32_t* stride, void* hip_stream) {
  *stride = pages ? batch->doc_page_stride : batch->top_stride;
  if (!blob64 && !blob32) return MGX_OK;  // size query
  if (!blob64 || !blob32) return mgx::Fail(MGX_ERR_INVALID_ARGUMENT, "mgx_batch_export_topk: null blob");
  if (!batch->executed) return mgx::Fail(MGX_ERR_INVALID_ARGUMENT, "mgx_batch_export_topk: not executed");
  hipStream_t s = nullptr;
  {
    int rc_s = mgx::BatchStream(batch, hip_stream, &s);
    if (rc_s) return rc_s;
  }
  if (pages) {
    const mgx_batch::Group& g = batch->page;
    MGX_HIP(hipSetDevice(batch->idx->device));
    MGX_LAUNCH(mgx::LaunchExportPages(g.dev.queries, static_cast<uint32_t>(g.qids.size()), batch->doc_page_stride,
                                      g.dev.page_docs, g.dev.totals, blob64, blob32, s));
    return MGX_OK;
  }
  const size_t n = batch->score.qids.size();
  const size_t ks = n * batch->top_stride;
  MGX_HIP(hipSetDevice(batch->idx->device));
  MGX_HIP(hipMemcpyAsync(blob64, batch->ex_keys(), (ks + n) * 8, hipMemcpyDeviceToDevice, s));
  MGX_HIP(hipMemcpyAsync(blob32, batch->ex_docs(), (ks + n) * 4, hipMemcpyDeviceToDevice, s));
  return MGX_OK;
}

int mgx_batch_export_buffer(mgx_batch* batch, void** device_blob, uint64_t* bytes, uint64_t* offset32) {
  if (device_blob) *device_blob = nullptr;
  if (bytes) *bytes = 0;
  if (offset32) *offset32 = 0;
  if (!batch || !device_blob || !bytes || !offset32)
    return mgx::Fail(MGX_ERR_INVALID_ARGUMENT, "mgx_batch_export_buffer: null argument");
  if (batch->fc.on()) return RefuseFacets("mgx_batch_export_buffer");
  if (batch->doc.on()) return RefuseDocuments("mgx_batch_export_buffer");
  if (batch->hl.on())
    return mgx::Fail(MGX_ERR_NOT_IMPLEMENTED, "mgx_batch_export_buffer: highlight on a sharded table is not implemented: the page's texts live on other ranks");
  if (const int rc_cs = RefuseColumnSort(batch, "mgx_batch_export_buffer")) return rc_cs;
  if (!batch->bitmap.qids.empty() || !batch->page.qids.empty() || batch->score.qids.empty()) return MGX_OK;  // none
  *device_blob = batch->d_export.p;
  *bytes = batch->ex_bytes;
  *offset32 = batch->ex_off32;
  return MGX_OK;
}

int mgx_batch_merge_shards(mgx_batch* batch, uint32_t n_shards, const uint64_t* blob64, uint64_t pitch64,
                           const uint32_t* blob32, uint64_t pitch32, void* hip_stream) {
  if (!batch || !blob64 || !blob32 || n_shards == 0)
    return mgx::Fail(MGX_ERR_INVALID_ARGUMENT, "mgx_batch_merge_shards: null argument");
  if (batch->fc.on()) return RefuseFacets("mgx_batch_merge_shards");
  if (batch->doc.on()) return RefuseDocuments("mgx_batch_merge_shards");
  if (batch->hl.on()) return mgx::Fail(MGX_ERR_NOT_IMPLEMENTED, "mgx_batch_merge_shards: highlight on a sharded table is not implemented: the page's texts live on other ranks");
  if (const int rc_cs = RefuseColumnSort(batch, "mgx_batch_merge_shards")) return rc_cs;
  const bool pages = batch->score.qids.empty() && batch->bitmap.qids.empty() && !batch->page.qids.empty();
  if (!pages && (!batch->bitmap.qids.empty() || !batch->page.qids.empty() || batch->score.qids.empty()))
    return mgx::Fail(MGX_ERR_INVALID_ARGUMENT,
                     "mgx_batch_merge_shards: the batch must be all MGX_SORT_SCORE or all docid-ordered pages");
  return MergeGroup(batch, pages, n_shards, blob64, pitch64, blob32, pitch32, hip_stream);
}

static int MergeGroup(mgx_batch* batch, bool pages, uint32_t n_shards, const uint64_t* blob64, uint64_t pitch64,
                      const uint32_t* blob32, uint64_t pitch32, void* hip_stream) {
  hipStream_t s = nullptr;
  {
    int rc_s = mgx::BatchStream(batch, hip_stream, &s);
    if (rc_s) return rc_s;
  }
  if (pages) {
    // shards hold disjoint doc ranges, but the merge needs no such knowledge: pages are best-first lists by doc id
    mgx_batch::Group& g = batch->page;
    const uint32_t n = static_cast<uint32_t>(g.qids.size());
    const uint32_t stride = batch->doc_page_stride;
    if (pitch64 == 0) pitch64 = static_cast<uint64_t>(n) * stride + n;  // blobs laid rank after rank
    if (pitch32 == 0) pitch32 = static_cast<uint64_t>(n) * stride + n;
    MGX_HIP(hipSetDevice(batch->idx->device));
    if (batch->d_page_scratch.bytes == 0)
      MGX_HIP(batch->d_page_scratch.Alloc(static_cast<size_t>(n) * stride * 8 + static_cast<size_t>(n) * 4));
    double* scratch_scores = batch->d_page_scratch.as<double>();
    uint32_t* scratch_n = reinterpret_cast<uint32_t*>(scratch_scores + static_cast<size_t>(n) * stride);
    MGX_LAUNCH(mgx::LaunchMergeTopK(g.dev.queries, g.d_ident.as<uint32_t>(), n, n_shards, blob64, blob32,
                                    blob32 + static_cast<uint64_t>(n) * stride, /*kq=*/stride, /*kj=*/pitch64,
                                    /*dj=*/pitch32, /*cq=*/1, /*cj=*/pitch32, nullptr, nullptr, nullptr, 0,
                                    g.dev.page_docs, scratch_scores, scratch_n, stride, nullptr, nullptr, nullptr, s));
    MGX_LAUNCH(mgx::LaunchSumTotals(blob64 + static_cast<uint64_t>(n) * stride, n_shards, n, pitch64,
                                    const_cast<uint64_t*>(g.dev.totals), s));
    batch->merged_shards = true;
    batch->last_stream = s;
    return mgx::IssueResultCopy(batch, s);  // (the merged page replaces the shard's own in the pinned block)
  }
  const uint32_t n = static_cast<uint32_t>(batch->score.qids.size());
  if (pitch64 == 0) pitch64 = static_cast<uint64_t>(n) * batch->top_stride + n;  // blobs laid rank after rank
  if (pitch32 == 0) pitch32 = static_cast<uint64_t>(n) * batch->top_stride + n;
  MGX_HIP(hipSetDevice(batch->idx->device));
  MGX_LAUNCH(mgx::LaunchMergeTopK(batch->score.dev.queries, batch->score.d_ident.as<uint32_t>(), n, n_shards, blob64,
                                  blob32, blob32 + static_cast<uint64_t>(n) * batch->top_stride,
                                  /*kq=*/batch->top_stride, /*kj=*/pitch64, /*dj=*/pitch32, /*cq=*/1, /*cj=*/pitch32,
                                  nullptr, nullptr, nullptr, 0, batch->sc_docs(), batch->sc_scores(), batch->sc_n(),
                                  batch->page_stride, nullptr, nullptr, nullptr, s));
  MGX_LAUNCH(mgx::LaunchSumTotals(blob64 + static_cast<uint64_t>(n) * batch->top_stride, n_shards, n, pitch64,
                                  batch->sc_override(), s));
  batch->merged_shards = true;
  batch->last_stream = s;
  return mgx::IssueResultCopy(batch, s);
}

// Mutable tables: a table is its main index plus a small delta index on the same device (documents added or changed
// since the main index was built). The same batch is compiled against both; the two calls below are the exchange of a
// sharded table with the wire taken out.
int mgx_batch_df_merge_local(mgx_batch* primary, mgx_batch* const* others, uint32_t n_others, void* hip_stream) {
  if (!primary || (n_others && !others)) return mgx::Fail(MGX_ERR_INVALID_ARGUMENT, "mgx_batch_df_merge_local: null argument");
  try {
    const uint32_t n = static_cast<uint32_t>(primary->h_text_df.size());
    for (uint32_t j = 0; j < n_others; ++j)
      if (!others[j] || others[j]->h_text_df.size() != n || others[j]->idx->device != primary->idx->device)
        return mgx::Fail(MGX_ERR_INVALID_ARGUMENT, "mgx_batch_df_merge_local: the batches do not hold the same text-level terms");
    if (n == 0) return MGX_OK;
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    int rc = mgx_batch_count_df(primary, hip_stream);
    if (rc) return rc;
    for (uint32_t j = 0; j < n_others; ++j) {
      rc = mgx_batch_count_df(others[j], hip_stream);
      if (rc) return rc;
      MGX_LAUNCH(mgx::LaunchAddU64(primary->d_text_df.as<uint64_t>(), others[j]->d_text_df.as<uint64_t>(), n, s));
    }
    for (uint32_t j = 0; j < n_others; ++j)
      MGX_HIP(hipMemcpyAsync(others[j]->d_text_df.p, primary->d_text_df.p, static_cast<size_t>(n) * 8, hipMemcpyDeviceToDevice, s));
    return MGX_OK;
  } catch (const std::exception& e) {
    return mgx::Fail(MGX_ERR_INTERNAL, std::string("mgx_batch_df_merge_local: ") + e.what());
  }
}

int mgx_batch_merge_local(mgx_batch* primary, mgx_batch* const* others, uint32_t n_others, void* hip_stream) {
  if (!primary || (n_others && !others)) return mgx::Fail(MGX_ERR_INVALID_ARGUMENT, "mgx_batch_merge_local: null argument");
  if (primary->n_queries == 0) return MGX_OK;
  if (!primary->res) return mgx::Fail(MGX_ERR_INVALID_ARGUMENT, "mgx_batch_merge_local: not a prepared batch object");
  if (!primary->bitmap.qids.empty() && n_others > 1)
    return mgx::Fail(MGX_ERR_NOT_IMPLEMENTED,
                     "mgx_batch_merge_local: a query without a page bound (limit 0 or > 16384, deep SORT _score) merges "
                     "two batches, not more");
  try {
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    // SORT by primary key: a side that ran such a query as a docid page (the shortcut of monotone keys) cannot be merged
    // by key with one that did not
    for (uint32_t j = 0; j < n_others; ++j)
      for (uint32_t qi = 0; others[j] && others[j]->n_queries == primary->n_queries && qi < primary->n_queries; ++qi)
        if (primary->specs[qi].pk_sort && others[j]->specs[qi].pk_sort &&
            !(primary->specs[qi].col_sort && others[j]->specs[qi].col_sort))
          return mgx::Fail(MGX_ERR_INVALID_ARGUMENT,
                           "mgx_batch_merge_local: query " + std::to_string(qi) + " is sorted by primary key and ran as a "
                           "docid page on one index: call mgx_index_set_primary_key_shortcut(index, 0) on a main index "
                           "that has a delta, before its batches are prepared");
    for (uint32_t j = 0; j < n_others; ++j)
      if (!others[j] || others[j] == primary || others[j]->n_queries != primary->n_queries ||
          others[j]->idx->device != primary->idx->device ||
          others[j]->score.qids.size() != primary->score.qids.size() ||
          others[j]->page.qids.size() != primary->page.qids.size() ||
          others[j]->bitmap.qids != primary->bitmap.qids || !others[j]->executed)
        return mgx::Fail(MGX_ERR_INVALID_ARGUMENT, "mgx_batch_merge_local: the batches do not hold the same queries");
    if (n_others == 1) {
      // SORT <filter column> across two indexes: their runs are merged by key, so a NULL on one side ties with a value
      // whose key is 0 (INT64_MIN, the all-ones double) on the other, which neither column's own mark can see
      for (uint32_t qi = 0; qi < primary->n_queries; ++qi) {
        const mgx::QuerySpec& sa = primary->specs[qi];
        const mgx::QuerySpec& sb = others[0]->specs[qi];
        if (!sa.col_sort || sa.pk_sort) continue;  // (the primary keys hold no NULL)
        mgx::colsort::KeyScan ka, kb;
        if (!sb.col_sort || !mgx::SortKeysOf(primary->idx, sa.sort_column, &ka) || !mgx::SortKeysOf(others[0]->idx, sb.sort_column, &kb))
          return mgx::Fail(MGX_ERR_INVALID_ARGUMENT, "mgx_batch_merge_local: the batches do not hold the same queries");
        if (mgx::colsort::KeysCollide(ka, kb))
          return mgx::Fail(MGX_ERR_NOT_IMPLEMENTED,
                           "mgx_batch_merge_local: query " + std::to_string(qi) + ": SORT by this column is not implemented "
                           "on a table with a delta index: between them the two indexes hold NULLs beside a value whose "
                           "64-bit sort key is NULL's (INT64_MIN, or the double whose bits are all ones)");
      }
    }
    // page documents: one main index (its own ids) and one delta (table ids through its doc map), before anything is touched
    const mgx_batch* doc_mapped = nullptr;
    const mgx_batch* doc_plain = nullptr;
    if (primary->doc.on()) {
      if (n_others > 1 || !mgx::MainAndDelta(primary, others, n_others, &doc_mapped, &doc_plain))
        return mgx::Fail(MGX_ERR_NOT_IMPLEMENTED, "mgx_batch_merge_local: page documents read one main index and one delta");
      if (n_others == 1) {
        const int rc = mgx::CheckDocumentSides(primary, others[0], "mgx_batch_merge_local");
        if (rc) return rc;
      }
    }
    MGX_HIP(hipSetDevice(primary->idx->device));
    if (!primary->bitmap.qids.empty() && n_others == 1) {
      // the bitmap group's page sizes need the totals on the host: its merge runs inside mgx_batch_fetch(primary)
      primary->merge_other = others[0];
      primary->merge_stream = s;
      others[0]->merged_away = true;
    }
    if (primary->score.qids.empty() && primary->page.qids.empty()) return MGX_OK;
    // a mixed batch has two groups (SORT _score queries, docid-ordered pages): each is exported, remapped and merged on its own
    uint64_t need = 0;
    for (int pass = 0; pass < 2; ++pass) {
      const bool pages = pass == 1;
      const uint64_t n = pages ? primary->page.qids.size() : primary->score.qids.size();
      if (n == 0) continue;
      const uint64_t stride = pages ? primary->doc_page_stride : primary->top_stride;
      need += ((n * stride + n) * 12 + 7) / 8 * 8 * (1ull + n_others);
    }
    void* recv = nullptr;
    MGX_HIP(primary->res->Exchange(1, need, &recv));
    char* g = static_cast<char*>(recv);
    int rc = MGX_OK;
    for (int pass = 0; pass < 2; ++pass) {
      const bool pages = pass == 1;
      const uint32_t n = static_cast<uint32_t>(pages ? primary->page.qids.size() : primary->score.qids.size());
      if (n == 0) continue;
      uint32_t stride = 0;
      rc = ExportGroup(primary, pages, nullptr, nullptr, &stride, hip_stream);
      if (rc) return rc;
      for (uint32_t j = 0; j < n_others; ++j) {
        uint32_t st = 0;
        rc = ExportGroup(others[j], pages, nullptr, nullptr, &st, hip_stream);
        if (rc) return rc;
        if (st != stride) return mgx::Fail(MGX_ERR_INVALID_ARGUMENT, "mgx_batch_merge_local: the batches do not hold the same queries");
      }
      const uint64_t elems = static_cast<uint64_t>(n) * stride + n;
      const uint64_t off32 = elems * 8, bytes = (elems * 12 + 7) / 8 * 8;
      for (uint32_t j = 0; j <= n_others; ++j) {
        mgx_batch* b = j == 0 ? primary : others[j - 1];
        uint64_t* b64 = reinterpret_cast<uint64_t*>(g + bytes * j);
        uint32_t* b32 = reinterpret_cast<uint32_t*>(g + bytes * j + off32);
        uint32_t st = 0;
        rc = ExportGroup(b, pages, b64, b32, &st, hip_stream);
        if (rc) return rc;
        const mgx_index* ix = b->idx;
        if (ix->d_doc_map.p) {
          const mgx_batch::Group& grp = pages ? b->page : b->score;
          MGX_LAUNCH(mgx::LaunchRemapBlobDocs(grp.dev.queries, n, stride, ix->d_doc_map.as<uint32_t>(), ix->dev.first_doc_id,
                                              ix->dev.n_docs, pages ? b64 : nullptr, b32, s));
        }
      }
      rc = MergeGroup(primary, pages, n_others + 1, reinterpret_cast<const uint64_t*>(g), bytes / 8,
                      reinterpret_cast<const uint32_t*>(g + off32), bytes / 4, hip_stream);
      if (rc) return rc;
      g += bytes * (1ull + n_others);
    }
    if (primary->hl.on()) {
      // the merged page names every document by its table id: the delta's through its doc map, the main index's own
      const mgx_batch *hl_mapped = nullptr, *hl_plain = nullptr;
      if (!mgx::MainAndDelta(primary, others, n_others, &hl_mapped, &hl_plain))
        return mgx::Fail(MGX_ERR_NOT_IMPLEMENTED, "mgx_batch_merge_local: highlight reads one main index and one delta");
      const mgx_index* mapped = hl_mapped ? hl_mapped->idx : nullptr;
      const mgx_index* plain = hl_plain ? hl_plain->idx : nullptr;
      if ((mapped && !mapped->dev.text) || (plain && !plain->dev.text))
        return mgx::Fail(MGX_ERR_INVALID_ARGUMENT, "mgx_batch_merge_local: highlight needs mgx_index_attach_text on every index");
      rc = mgx::RunHighlight(primary, s, /*merged=*/true, mapped, plain);
      if (rc) return rc;
      MGX_HIP(hipEventRecord(primary->res->done_ev, s));  // (the records replace those of the primary's own page)
    }
    if (primary->doc.on()) {
      // the same for page documents: the delta's rows through its doc map and its own batch's column ids
      rc = mgx::RunDocuments(primary, s, /*merged=*/true, doc_mapped, doc_plain);
      if (rc) return rc;
      MGX_HIP(hipEventRecord(primary->res->done_ev, s));
    }
    return MGX_OK;
  } catch (const std::exception& e) {
    return mgx::Fail(MGX_ERR_INTERNAL, std::string("mgx_batch_merge_local: ") + e.what());
  }
}

// =================================================================================================================
// RCCL exchange (one rank per doc-range shard): the collective of the sharded path lives behind the C ABI
// =================================================================================================================
// librccl is loaded on first use (dlopen), so the library itself loads on hosts without it; the five entry points
// below are RCCL's own (rccl.h: ncclGetUniqueId :187, ncclCommInitRank :220, ncclAllReduce :611, ncclAllGather :678).
namespace mgx {
struct Rccl {
  void* lib = nullptr;
  int (*GetUniqueId)(void*) = nullptr;
  int (*CommInitRank)(void**, int, RcclId, int) = nullptr;
  int (*CommDestroy)(void*) = nullptr;
  int (*CommAbort)(void*) = nullptr;
  int (*AllGather)(const void*, void*, size_t, int, void*, hipStream_t) = nullptr;
  int (*AllReduce)(const void*, void*, size_t, int, int, void*, hipStream_t) = nullptr;
  const char* (*GetErrorString)(int) = nullptr;
  std::string error;
};
static Rccl& LoadRccl() {
  static Rccl r;
  static std::once_flag once;
  std::call_once(once, [] {
    for (const char* name : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"}) {
      r.lib = dlopen(name, RTLD_NOW | RTLD_GLOBAL);
      if (r.lib) break;
    }
    if (!r.lib) {
      r.error = std::string("librccl.so not found: ") + dlerror();
      return;
    }
    auto sym = [&](const char* n) {
      void* p = dlsym(r.lib, n);
      if (!p && r.error.empty()) r.error = std::string("librccl.so lacks ") + n;
      return p;
    };
    r.GetUniqueId = reinterpret_cast<decltype(r.GetUniqueId)>(sym("ncclGetUniqueId"));
    r.CommInitRank = reinterpret_cast<decltype(r.CommInitRank)>(sym("ncclCommInitRank"));
    r.CommDestroy = reinterpret_cast<decltype(r.CommDestroy)>(sym("ncclCommDestroy"));
    r.CommAbort = reinterpret_cast<decltype(r.CommAbort)>(sym("ncclCommAbort"));
    r.AllGather = reinterpret_cast<decltype(r.AllGather)>(sym("ncclAllGather"));
    r.AllReduce = reinterpret_cast<decltype(r.AllReduce)>(sym("ncclAllReduce"));
    r.GetErrorString = reinterpret_cast<decltype(r.GetErrorString)>(sym("ncclGetErrorString"));
  });
  return r;
}
static int RcclFail(const char* what, int rc) {
  Rccl& r = LoadRccl();
  return Fail(MGX_ERR_INTERNAL, std::string(what) + ": " + (r.GetErrorString ? r.GetErrorString(rc) : "RCCL error") +
                                    " (" + std::to_string(rc) + ")");
}
}  // namespace mgx

struct mgx_comm {
  void* comm = nullptr;
  int rank = 0, world = 1, device = 0;
};

int mgx_comm_unique_id(uint8_t* id) {
  if (!id) return mgx::Fail(MGX_ERR_INVALID_ARGUMENT, "mgx_comm_unique_id: null argument");
  mgx::Rccl& r = mgx::LoadRccl();
  if (!r.error.empty()) return mgx::Fail(MGX_ERR_INTERNAL, r.error);
  mgx::RcclId uid{};
  const int rc = r.GetUniqueId(&uid);
  if (rc != 0) return mgx::RcclFail("ncclGetUniqueId", rc);
  std::memcpy(id, uid.internal, MGX_COMM_ID_BYTES);
  return MGX_OK;
}

int mgx_comm_create(const uint8_t* id, int rank, int world, int device, mgx_comm** out) {
  if (out) *out = nullptr;
  if (!id || !out || world < 1 || rank < 0 || rank >= world)
    return mgx::Fail(MGX_ERR_INVALID_ARGUMENT, "mgx_comm_create: bad argument");
  mgx::Rccl& r = mgx::LoadRccl();
  if (!r.error.empty()) return mgx::Fail(MGX_ERR_INTERNAL, r.error);
  MGX_HIP(hipSetDevice(device));
  mgx::RcclId uid{};
  std::memcpy(uid.internal, id, MGX_COMM_ID_BYTES);
  auto c = std::make_unique<mgx_comm>();
  c->rank = rank;
  c->world = world;
  c->device = device;
  const int rc = r.CommInitRank(&c->comm, world, uid, rank);
  if (rc != 0) return mgx::RcclFail("ncclCommInitRank", rc);
  *out = c.release();
  return MGX_OK;
}

void mgx_comm_destroy(mgx_comm* comm) {
  if (!comm) return;
  if (comm->comm) (void)mgx::LoadRccl().CommDestroy(comm->comm);
  delete comm;
}

int mgx_comm_abort(mgx_comm* comm) {
  if (!comm) return mgx::Fail(MGX_ERR_INVALID_ARGUMENT, "mgx_comm_abort: null argument");
  if (!comm->comm) return MGX_OK;  // (already aborted)
  mgx::Rccl& r = mgx::LoadRccl();
  void* c = comm->comm;
  comm->comm = nullptr;
  const int rc = r.CommAbort ? r.CommAbort(c) : r.CommDestroy(c);
  return rc != 0 ? mgx::RcclFail("ncclCommAbort", rc) : MGX_OK;
}

int mgx_batch_exchange_df(mgx_batch* batch, mgx_comm* comm, void* hip_stream) {
  if (!batch || !comm) return mgx::Fail(MGX_ERR_INVALID_ARGUMENT, "mgx_batch_exchange_df: null argument");
  if (!comm->comm) return mgx::Fail(MGX_ERR_INTERNAL, "mgx_batch_exchange_df: the communicator was aborted");
  uint64_t* counts = nullptr;
  uint32_t n = 0;
  int rc = mgx_batch_df_buffer(batch, &counts, &n);
  if (rc || n == 0) return rc;
  rc = mgx_batch_count_df(batch, hip_stream);
  if (rc) return rc;
  hipStream_t s = nullptr;
  rc = mgx::BatchStream(batch, hip_stream, &s);
  if (rc) return rc;
  // PopulateTermDocumentFrequency over every shard's candidates: the per-shard counts are summed before any rank takes idf
  const int nrc = mgx::LoadRccl().AllReduce(counts, counts, n, mgx::kRcclUint64, mgx::kRcclSum, comm->comm, s);
  if (nrc != 0) return mgx::RcclFail("ncclAllReduce", nrc);
  return MGX_OK;
}

int mgx_batch_exchange(mgx_batch* batch, mgx_comm* comm, void* hip_stream) {
  if (batch && batch->fc.on()) return RefuseFacets("mgx_batch_exchange");  // (before anything else is looked at)
  if (batch && batch->doc.on()) return RefuseDocuments("mgx_batch_exchange");
  if (!batch || !comm) return mgx::Fail(MGX_ERR_INVALID_ARGUMENT, "mgx_batch_exchange: null argument");
  if (batch->hl.on()) return mgx::Fail(MGX_ERR_NOT_IMPLEMENTED, "mgx_batch_exchange: highlight on a sharded table is not implemented: the page's texts live on other ranks");
  if (const int rc_cs = RefuseColumnSort(batch, "mgx_batch_exchange")) return rc_cs;
  if (!comm->comm) return mgx::Fail(MGX_ERR_INTERNAL, "mgx_batch_exchange: the communicator was aborted");
  if (batch->n_queries == 0) return MGX_OK;
  if (!batch->executed) return mgx::Fail(MGX_ERR_INVALID_ARGUMENT, "mgx_batch_exchange: not executed");
  hipStream_t s = nullptr;
  int rc = mgx::BatchStream(batch, hip_stream, &s);
  if (rc) return rc;
  MGX_HIP(hipSetDevice(batch->idx->device));
  if (!batch->res) return mgx::Fail(MGX_ERR_INVALID_ARGUMENT, "mgx_batch_exchange: not a prepared batch object");
  void* blob = nullptr;
  uint64_t bytes = 0, off32 = 0;
  rc = mgx_batch_export_buffer(batch, &blob, &bytes, &off32);
  if (rc) return rc;
  if (!blob) {  // docid-ordered pages: exported by copy into the exchange layout
    uint32_t stride = 0;
    rc = mgx_batch_export_topk(batch, nullptr, nullptr, &stride, s);
    if (rc) return rc;
    const uint64_t elems = static_cast<uint64_t>(batch->n_queries) * stride + batch->n_queries;
    off32 = elems * 8;
    bytes = (elems * 12 + 7) / 8 * 8;
    MGX_HIP(batch->res->Exchange(0, bytes, &blob));
    rc = mgx_batch_export_topk(batch, static_cast<uint64_t*>(blob),
                               reinterpret_cast<uint32_t*>(static_cast<char*>(blob) + off32), &stride, s);
    if (rc) return rc;
  }
  const uint64_t need = bytes * static_cast<uint64_t>(comm->world);
  void* recv = nullptr;
  MGX_HIP(batch->res->Exchange(1, need, &recv));
  // one all-gather moves every rank's keys, totals, doc ids and counts (both blobs sit in one buffer per rank)
  const int nrc = mgx::LoadRccl().AllGather(blob, recv, bytes, mgx::kRcclUint8, comm->comm, s);
  if (nrc != 0) return mgx::RcclFail("ncclAllGather", nrc);
  char* g = static_cast<char*>(recv);
  return mgx_batch_merge_shards(batch, static_cast<uint32_t>(comm->world), reinterpret_cast<const uint64_t*>(g),
                                bytes / 8, reinterpret_cast<const uint32_t*>(g + off32), bytes / 4, s);
}

namespace mgx {
static int SeedBoundExchange(mgx_batch* b, mgx_batch::Group& g, const SeedGather& sg, hipStream_t s) {
  const uint32_t n = static_cast<uint32_t>(g.qids.size()), k = g.seed_k;
  const uint64_t bytes = static_cast<uint64_t>(n) * k * 8;
  void* mine = nullptr;
  void* all = nullptr;
  MGX_HIP(b->res->Exchange(2, bytes, &mine));
  MGX_HIP(b->res->Exchange(3, bytes * static_cast<uint64_t>(sg.world), &all));
  MGX_LAUNCH(LaunchPackSeedKeys(g.d_list_begin.as<uint32_t>(), g.d_has_seed.as<uint8_t>(), g.dev.cand_keys, g.dev.cand_n,
                                g.dev.cand_stride, n, k, static_cast<uint64_t*>(mine), s));
  if (std::getenv("MGX_VERBOSE"))
    fprintf(stderr, "[mgx] seed-bound exchange: %u queries x %u keys, world %d\n", n, k, sg.world);
  const int grc = sg.fn(sg.user, mine, all, bytes, s);
  if (grc != MGX_OK) return grc == MGX_ERR_INTERNAL && !g_last_error.empty() ? grc : Fail(grc, "the seed-key all-gather failed");
  MGX_LAUNCH(LaunchApplySeedBounds(static_cast<const uint64_t*>(all), static_cast<uint32_t>(sg.world), n, k, g.dev.queries,
                                   g.dev.bounds, s));
  return MGX_OK;
}
static int RcclGather(void* user, const void* mine, void* all, uint64_t bytes, void* hip_stream) {
  const int nrc = LoadRccl().AllGather(mine, all, bytes, kRcclUint8, user, static_cast<hipStream_t>(hip_stream));
  return nrc != 0 ? RcclFail("ncclAllGather (seed keys)", nrc) : MGX_OK;
}
}  // namespace mgx

int mgx_batch_execute_gather(mgx_batch* batch, int world, mgx_gather_fn gather, void* user, void* hip_stream) {
  if (!batch || !gather || world < 1) return mgx::Fail(MGX_ERR_INVALID_ARGUMENT, "mgx_batch_execute_gather: bad argument");
  if (batch->fc.on()) return RefuseFacets("mgx_batch_execute_gather");
  if (batch->doc.on()) return RefuseDocuments("mgx_batch_execute_gather");
  if (batch->hl.on()) return mgx::Fail(MGX_ERR_NOT_IMPLEMENTED, "mgx_batch_execute_gather: highlight on a sharded table is not implemented: the page's texts live on other ranks");
  if (const int rc_cs = RefuseColumnSort(batch, "mgx_batch_execute_gather")) return rc_cs;
  try {
    hipStream_t s = nullptr;
    int rc = mgx::BatchStream(batch, hip_stream, &s);
    if (rc) return rc;
    mgx::SeedGather sg;
    sg.world = world;
    sg.fn = gather;
    sg.user = user;
    // Splitting the launch costs ~0.03 ms per batch on a 1.25M-doc shard (the main items wait for every seed, two small
    // kernels, the collective: 0.375 -> 0.405 ms per step measured with one rank) and buys a bound made from world x 8
    // tiles instead of 8. What a better start is worth was measured on one GPU with the bounds of a finished pass
    // injected (ablation build, MGX_KEEP_BOUNDS): 0.27 -> 0.20 ms on that shard, 24 % of its kernel. Eight ranks' seeds
    // together cover 64 of a shard's 77 tiles' worth of documents — a bound close to the finished pass's — so the
    // exchange nets about 0.07 x 0.8 - 0.03 = +0.03 ms of 0.27 (10 %) at eight shards, less than its cost at two.
    // Default: ON from four ranks up (shards of a million docs and more, see ExecuteImpl); MGX_SEED_EXCHANGE=0 / 1
    // forces it off / on for every world size.
    static const int forced = std::getenv("MGX_SEED_EXCHANGE") ? atoi(std::getenv("MGX_SEED_EXCHANGE")) : -1;
    const bool on = forced >= 0 ? forced != 0 : world >= 4;
    return mgx::ExecuteImpl(batch, s, on ? &sg : nullptr);
  } catch (const std::exception& e) {
    return mgx::Fail(MGX_ERR_INTERNAL, std::string("mgx_batch_execute_gather: ") + e.what());
  }
}

int mgx_batch_execute_sharded(mgx_batch* batch, mgx_comm* comm, void* hip_stream) {
  if (batch && batch->fc.on()) return RefuseFacets("mgx_batch_execute_sharded");
  if (batch && batch->doc.on()) return RefuseDocuments("mgx_batch_execute_sharded");
  if (!batch || !comm) return mgx::Fail(MGX_ERR_INVALID_ARGUMENT, "mgx_batch_execute_sharded: null argument");
  if (!comm->comm) return mgx::Fail(MGX_ERR_INTERNAL, "mgx_batch_execute_sharded: the communicator was aborted");
  return mgx_batch_execute_gather(batch, comm->world, &mgx::RcclGather, comm->comm, hip_stream);
}

int mgx_batch_algorithmic_bytes(mgx_batch* batch, uint64_t* list_bytes, uint64_t* score_bytes,
                                uint64_t* topk_bytes) {
  if (!batch || !list_bytes || !score_bytes || !topk_bytes)
    return mgx::Fail(MGX_ERR_INVALID_ARGUMENT, "mgx_batch_algorithmic_bytes: null argument");
  *list_bytes = batch->list_bytes;
  uint64_t sb = 0, tb = 0;
  for (uint32_t qi = 0; qi < batch->n_queries; ++qi) {
    const mgx::QuerySpec& sp = batch->specs[qi];
    const uint64_t R = batch->h_results[qi].total;
    if (sp.mode == mgx::kModeScore) {
      sb += R * (sp.score.size() + 4);
      tb += 12 * std::min<uint64_t>(R, static_cast<uint64_t>(sp.offset) + sp.limit);
    } else {
      tb += 4 * std::min<uint64_t>(R, sp.limit ? sp.limit : R);
    }
  }
  *score_bytes = sb;
  *topk_bytes = tb;
  return MGX_OK;
}

int mgx_batch_kernel_time_ms(mgx_batch* batch, double* avg_ms, uint32_t* n) {
  if (avg_ms) *avg_ms = 0.0;
  if (n) *n = 0;
  if (!batch || !avg_ms || !n) return mgx::Fail(MGX_ERR_INVALID_ARGUMENT, "mgx_batch_kernel_time_ms: null argument");
  MGX_HIP(hipSetDevice(batch->idx->device));
  double sum = 0.0;
  uint32_t cnt = 0;
  for (auto& ev : batch->events) {
    MGX_HIP(hipEventSynchronize(ev.second));
    float ms = 0.f;
    MGX_HIP(hipEventElapsedTime(&ms, ev.first, ev.second));
    sum += ms;
    ++cnt;
    (void)hipEventDestroy(ev.first);
    (void)hipEventDestroy(ev.second);
  }
  batch->events.clear();
  batch->timing = true;
  *avg_ms = cnt ? sum / cnt : 0.0;
  *n = cnt;
  return MGX_OK;
}

void mgx_batch_destroy(mgx_batch* batch) {
  if (!batch) return;
  (void)hipSetDevice(batch->idx->device);
  for (auto& ev : batch->events) {
    (void)hipEventDestroy(ev.first);
    (void)hipEventDestroy(ev.second);
  }
  if (batch->res_owned && batch->res_owned->main_ev) {  // (the index must not chain a later batch to a dead event)
    std::lock_guard<std::mutex> lock(batch->idx->table_mu);
    if (batch->idx->chain_ev == batch->res_owned->main_ev) batch->idx->chain_ev = nullptr;
  }
  delete batch;
}

}  // extern "C"

// =================================================================================================================
// single operators
// =================================================================================================================

namespace {
// One set of batch resources (arenas, pinned result block, stream) leased from the index for the duration of a call.
struct SingleLease {
  mgx_index* idx;
  std::unique_ptr<mgx::BatchResources> res;
  hipStream_t stream = nullptr;
  explicit SingleLease(mgx_index* i) : idx(i) {
    {
      std::lock_guard<std::mutex> lock(idx->pool_mu);
      if (!idx->single_pool.empty()) {
        res = std::move(idx->single_pool.back());
        idx->single_pool.pop_back();
      }
    }
    if (!res) res = std::make_unique<mgx::BatchResources>();
    res->Reset();
  }
  ~SingleLease() {
    std::lock_guard<std::mutex> lock(idx->pool_mu);
    if (idx->single_pool.size() < 64) idx->single_pool.push_back(std::move(res));
  }
  hipError_t OpenStream() {
    if (!res->stream) {
      const hipError_t e = hipStreamCreateWithFlags(&res->stream, hipStreamNonBlocking);
      if (e != hipSuccess) return e;
    }
    stream = res->stream;
    return hipSuccess;
  }
  // ships what Upload() staged in the lease's pinned mirror (calls that do not go through a batch's execute)
  hipError_t Ship() {
    for (const mgx::Arena::Chunk& c : res->upload.chunks)
      if (c.used) {
        const hipError_t e = hipMemcpyAsync(c.dev, c.host, c.used, hipMemcpyHostToDevice, stream);
        if (e != hipSuccess) return e;
      }
    res->uploaded = true;
    return hipSuccess;
  }
  // copies a result back to the host behind the call's kernels and waits for it
  hipError_t CopyBack(void* host, const void* dev, size_t bytes) {
    const hipError_t e = hipMemcpyAsync(host, dev, bytes, hipMemcpyDeviceToHost, stream);
    return e != hipSuccess ? e : hipStreamSynchronize(stream);
  }
};

// Every single operator's failure handling: an exception out of `body` becomes MGX_ERR_INTERNAL "<name>: <what>".
template <class Body>
int Guarded(const char* name, Body&& body) {
  try {
    return body();
  } catch (const std::exception& e) {
    return mgx::Fail(MGX_ERR_INTERNAL, std::string(name) + ": " + e.what());
  }
}

// body(lease) on the index's device with a lease and its open stream. arenas: DevBuf::Alloc / Upload in `body` draw
// from the lease's arenas (uploads go out with lease.Ship()); otherwise from their own hipMalloc (a batch run on the
// lease takes the lease's resources itself, as mgx_batch::res).
template <class Body>
int WithLease(mgx_index* idx, const char* name, bool arenas, Body&& body) {
  return Guarded(name, [&] {
    MGX_HIP(hipSetDevice(idx->device));
    SingleLease lease(idx);
    MGX_HIP(lease.OpenStream());
    mgx::ResourceScope scope(arenas ? lease.res.get() : nullptr);
    return body(lease);
  });
}

// Prepares and executes one compiled query as a batch of one on the lease.
int ExecuteSingle(SingleLease& lease, mgx::QuerySpec&& spec, mgx_batch* b) {
  std::vector<mgx::QuerySpec> specs;
  specs.push_back(std::move(spec));
  b->res = lease.res.get();
  const int rc = mgx::PrepareInto(b, lease.idx, std::move(specs));
  return rc ? rc : mgx::ExecuteImpl(b, lease.stream);
}

// mgx_and / mgx_or / mgx_not / mgx_threshold: emit(c, q) compiles the query (nonzero: its argument error); within the
// leaf limit it runs as a batch of one, and *out_docs (malloc) gets its ids.
template <class Emit>
int RunSingle(mgx_index* idx, const char* name, uint32_t** out_docs, uint64_t* out_n, Emit&& emit) {
  return Guarded(name, [&] {
    mgx::QuerySpec q;
    const mgx::CompileView view = mgx::ViewOf(idx);
    mgx::Compiler c{&view, &q, 0};
    const int rc = emit(c, q);
    if (rc) return rc;
    if (q.leaves.size() > mgx::kMaxLeaves)
      return mgx::Fail(MGX_ERR_NOT_IMPLEMENTED, std::string(name) + ": more than 192 lists");
    return WithLease(idx, name, false, [&](SingleLease& lease) {
      mgx_batch b;
      int rc = ExecuteSingle(lease, std::move(q), &b);
      if (rc) return rc;
      mgx_result_view v{};
      rc = mgx::FetchImpl(&b, &v);
      if (rc) return rc;
      const uint32_t n = v.queries[0].n_docs;
      uint32_t* o = static_cast<uint32_t*>(std::malloc((n ? n : 1) * sizeof(uint32_t)));
      if (!o) return mgx::Fail(MGX_ERR_INTERNAL, "out of host memory");
      if (n) std::memcpy(o, v.docs, n * sizeof(uint32_t));
      *out_docs = o;
      *out_n = n;
      return MGX_OK;
    });
  });
}

// out-parameters cleared, then the arguments of every operator on gram ids checked
int CheckSingle(const char* name, const mgx_index* idx, const uint32_t* g, uint32_t n, uint32_t** out_docs,
                uint64_t* out_n) {
  if (out_docs) *out_docs = nullptr;
  if (out_n) *out_n = 0;
  if (!idx || !out_docs || !out_n) return mgx::Fail(MGX_ERR_INVALID_ARGUMENT, std::string(name) + ": null argument");
  if (n && !g) return mgx::Fail(MGX_ERR_INVALID_ARGUMENT, std::string(name) + ": null gram ids");
  for (uint32_t i = 0; i < n; ++i)
    if (g[i] >= idx->n_grams) return mgx::Fail(MGX_ERR_OUT_OF_RANGE, std::string(name) + ": unknown gram id");
  return MGX_OK;
}
}  // namespace

extern "C" {

int mgx_facet_counts(mgx_index* idx, const mgx_query* query, uint32_t column_id, uint64_t* counts_out, uint64_t* matched) {
  if (matched) *matched = 0;
  if (!idx || !query || !counts_out || !matched)
    return mgx::Fail(MGX_ERR_INVALID_ARGUMENT, "mgx_facet_counts: null argument");
  return WithLease(idx, "mgx_facet_counts", false, [&](SingleLease& lease) {
    // the search part as a materialising query: the result bitmap of every tile, then a histogram of the column's value
    // ids over it (what roaring_bitmap_and_cardinality per value bitmap adds up to, filter_index.cpp:300-306)
    mgx_query q = *query;
    q.sort = MGX_SORT_DOCID;
    q.limit = 0;
    q.offset = 0;
    q.reverse = 0;
    q.score_terms = nullptr;
    q.n_score_terms = 0;
    mgx::QuerySpec spec;
    int rc = mgx::CompileQuery(mgx::ViewOf(idx), q, &spec);
    if (rc) return rc;
    const mgx_index::FilterColumn* colp = nullptr;
    {
      std::lock_guard<std::mutex> lock(idx->mu);  // (columns are added under mu; the objects themselves never move)
      if (column_id >= idx->filter_columns.size())
        return mgx::Fail(MGX_ERR_OUT_OF_RANGE, "mgx_facet_counts: unknown filter column");
      colp = idx->filter_columns[column_id].get();
    }
    const mgx_index::FilterColumn& col = *colp;
    if (!col.d_value_ids.p) return mgx::Fail(MGX_ERR_INVALID_ARGUMENT, "mgx_facet_counts: the column was added without value ids");
    mgx_batch b;
    rc = ExecuteSingle(lease, std::move(spec), &b);
    if (rc) return rc;
    if (b.bitmap.qids.size() != 1) return mgx::Fail(MGX_ERR_INTERNAL, "mgx_facet_counts: the query did not compile to a result bitmap");
    DevBuf d_counts;  // (own memory: no arena scope here)
    MGX_HIP(d_counts.Alloc(std::max<size_t>(col.n_values, 1) * sizeof(unsigned long long)));
    MGX_HIP(hipMemsetAsync(d_counts.p, 0, d_counts.bytes, lease.stream));
    MGX_LAUNCH(mgx::LaunchFacetCount(b.d_rbits.as<uint64_t>(), idx->dev.n_tiles * mgx::kWordsPerTile,
                                     col.d_value_ids.as<uint32_t>(), idx->dev.n_docs, col.n_values,
                                     d_counts.as<unsigned long long>(), lease.stream));
    uint64_t total = 0;
    if (col.n_values)
      MGX_HIP(hipMemcpyAsync(counts_out, d_counts.p, static_cast<size_t>(col.n_values) * 8, hipMemcpyDeviceToHost,
                             lease.stream));
    MGX_HIP(lease.CopyBack(&total, b.d_totals.p, 8));
    *matched = total;
    return MGX_OK;
  });
}

int mgx_and(mgx_index* idx, const uint32_t* gram_ids, uint32_t n, uint64_t limit, int reverse, uint32_t** out_docs,
            uint64_t* out_n) {
  if (int rc = CheckSingle("mgx_and", idx, gram_ids, n, out_docs, out_n)) return rc;
  if (n == 0) return mgx::Fail(MGX_ERR_INVALID_ARGUMENT, "mgx_and: no grams (the caller returns {} for empty terms)");
  if (limit > 0xFFFFFFFFull) limit = 0;
  return RunSingle(idx, "mgx_and", out_docs, out_n, [&](mgx::Compiler& c, mgx::QuerySpec& q) {
    c.Emit(mgx::kOpLoad, c.GramLeaf(gram_ids[0]));
    for (uint32_t i = 1; i < n; ++i) c.Emit(mgx::kOpAnd, c.GramLeaf(gram_ids[i]));
    q.limit = static_cast<uint32_t>(limit);
    q.reverse = reverse ? 1 : 0;
    return MGX_OK;
  });
}

int mgx_or(mgx_index* idx, const uint32_t* gram_ids, uint32_t n, uint32_t** out_docs, uint64_t* out_n) {
  if (int rc = CheckSingle("mgx_or", idx, gram_ids, n, out_docs, out_n)) return rc;
  if (n == 0) return mgx::Fail(MGX_ERR_INVALID_ARGUMENT, "mgx_or: no grams");
  return RunSingle(idx, "mgx_or", out_docs, out_n, [&](mgx::Compiler& c, mgx::QuerySpec&) {
    c.Emit(mgx::kOpLoad, c.GramLeaf(gram_ids[0]));
    for (uint32_t i = 1; i < n; ++i) c.Emit(mgx::kOpOr, c.GramLeaf(gram_ids[i]));
    return MGX_OK;
  });
}

int mgx_not(mgx_index* idx, const uint32_t* all_docs, uint64_t n_all, const uint32_t* gram_ids, uint32_t n,
            uint32_t** out_docs, uint64_t* out_n) {
  if (int rc = CheckSingle("mgx_not", idx, gram_ids, n, out_docs, out_n)) return rc;
  if (n_all && !all_docs) return mgx::Fail(MGX_ERR_INVALID_ARGUMENT, "mgx_not: null all_docs");
  if (n_all > 0xFFFFFFFFull) return mgx::Fail(MGX_ERR_OUT_OF_RANGE, "mgx_not: too many docs");
  // ids outside the index range cannot be in any posting list: they pass through untouched, in order
  std::vector<uint32_t> below, above;
  uint32_t* mid = nullptr;
  uint64_t n_mid = 0;
  const int rc = RunSingle(idx, "mgx_not", &mid, &n_mid, [&](mgx::Compiler& c, mgx::QuerySpec& q) {
    const uint64_t lo = idx->dev.first_doc_id, hi = lo + idx->dev.n_docs;
    for (uint64_t i = 0; i < n_all; ++i) {
      if (i && all_docs[i] <= all_docs[i - 1])
        return mgx::Fail(MGX_ERR_INVALID_ARGUMENT, "mgx_not: all_docs must be strictly ascending");
      if (all_docs[i] < lo) below.push_back(all_docs[i]);
      else if (all_docs[i] >= hi) above.push_back(all_docs[i]);
      else q.explicit_ids.push_back(all_docs[i]);
    }
    c.Emit(mgx::kOpLoad, c.Leaf(mgx::kLeafExplicit, 0, static_cast<uint32_t>(q.explicit_ids.size())));
    for (uint32_t i = 0; i < n; ++i) c.Emit(mgx::kOpAndNot, c.GramLeaf(gram_ids[i]));
    return MGX_OK;
  });
  if (rc) return rc;
  if (below.empty() && above.empty()) {
    *out_docs = mid;
    *out_n = n_mid;
    return MGX_OK;
  }
  const uint64_t tot = below.size() + n_mid + above.size();
  uint32_t* o = static_cast<uint32_t*>(std::malloc((tot ? tot : 1) * 4));
  if (!o) {
    std::free(mid);
    return mgx::Fail(MGX_ERR_INTERNAL, "out of host memory");
  }
  std::copy(below.begin(), below.end(), o);
  std::copy(mid, mid + n_mid, o + below.size());
  std::copy(above.begin(), above.end(), o + below.size() + n_mid);
  std::free(mid);
  *out_docs = o;
  *out_n = tot;
  return MGX_OK;
}

int mgx_threshold(mgx_index* idx, const uint32_t* gram_ids, uint32_t n, uint32_t threshold, uint32_t** out_docs,
                  uint64_t* out_n) {
  if (int rc = CheckSingle("mgx_threshold", idx, gram_ids, n, out_docs, out_n)) return rc;
  if (n == 0 || threshold == 0 || threshold > n)
    return mgx::Fail(MGX_ERR_INVALID_ARGUMENT, "mgx_threshold: need 1 <= threshold <= number of distinct grams");
  if (n > 127) return mgx::Fail(MGX_ERR_OUT_OF_RANGE, "mgx_threshold: more than 127 grams");
  return RunSingle(idx, "mgx_threshold", out_docs, out_n, [&](mgx::Compiler& c, mgx::QuerySpec& q) {
    c.Emit(mgx::kOpThreshBegin);
    for (uint32_t i = 0; i < n; ++i) c.Emit(mgx::kOpThreshAdd, c.GramLeaf(gram_ids[i]));
    c.Emit(mgx::kOpThreshEnd, threshold);
    if (q.leaves.size() != n) return mgx::Fail(MGX_ERR_INVALID_ARGUMENT, "mgx_threshold: grams must be distinct");
    return MGX_OK;
  });
}

int mgx_retain(mgx_index* idx, const uint32_t* candidates, uint64_t n_cand, const uint32_t* gram_ids, uint32_t n,
               uint32_t** out_docs, uint64_t* out_n) {
  if (int rc = CheckSingle("mgx_retain", idx, gram_ids, n, out_docs, out_n)) return rc;
  if (n_cand && !candidates) return mgx::Fail(MGX_ERR_INVALID_ARGUMENT, "mgx_retain: null candidates");
  return WithLease(idx, "mgx_retain", true, [&](SingleLease& lease) {
    std::vector<uint8_t> keep(n_cand, 1);
    if (n_cand && n) {
      DevBuf d_c, d_g, d_k;
      MGX_HIP(mgx::Upload(d_c, candidates, n_cand));
      MGX_HIP(mgx::Upload(d_g, gram_ids, n));
      MGX_HIP(d_k.Alloc(n_cand));
      MGX_HIP(lease.Ship());
      MGX_LAUNCH(mgx::LaunchRetain(idx->dev, d_c.as<uint32_t>(), n_cand, d_g.as<uint32_t>(), n, d_k.as<uint8_t>(),
                                   lease.stream));
      MGX_HIP(lease.CopyBack(keep.data(), d_k.p, n_cand));
    }
    uint32_t* o = static_cast<uint32_t*>(std::malloc((n_cand ? n_cand : 1) * 4));
    if (!o) return mgx::Fail(MGX_ERR_INTERNAL, "out of host memory");
    uint64_t k = 0;
    for (uint64_t i = 0; i < n_cand; ++i)
      if (keep[i]) o[k++] = candidates[i];
    *out_docs = o;
    *out_n = k;
    return MGX_OK;
  });
}

int mgx_score_documents(mgx_index* idx, const uint32_t* candidates, uint64_t n_cand, const uint32_t* gram_ids,
                        const double* idfs, uint32_t n_terms, double avg_doc_length, double k1, double b,
                        double* scores_out) {
  if (!idx || (n_cand && (!candidates || !scores_out)) || (n_terms && (!gram_ids || !idfs)))
    return mgx::Fail(MGX_ERR_INVALID_ARGUMENT, "mgx_score_documents: null argument");
  if (!idx->can_score) return mgx::Fail(MGX_ERR_NOT_IMPLEMENTED, "index was created without tf/doc_len columns");
  // (an id with bit 31 set would read as a text-level term (kDeepText): nothing bounds n_grams below 2^31)
  for (uint32_t i = 0; i < n_terms; ++i)
    if (gram_ids[i] != mgx::kNoRow && (gram_ids[i] >= idx->n_grams || (gram_ids[i] & mgx::kDeepText) != 0))
      return mgx::Fail(MGX_ERR_OUT_OF_RANGE, "mgx_score_documents: unknown gram id");
  if (n_cand == 0) return MGX_OK;
  return WithLease(idx, "mgx_score_documents", true, [&](SingleLease& lease) {
    DevBuf d_c, d_g, d_i, d_s;
    MGX_HIP(mgx::Upload(d_c, candidates, n_cand));
    MGX_HIP(mgx::Upload(d_g, gram_ids, n_terms));
    MGX_HIP(mgx::Upload(d_i, idfs, n_terms));
    MGX_HIP(d_s.Alloc(n_cand * 8));
    MGX_HIP(lease.Ship());
    MGX_LAUNCH(mgx::LaunchScoreCandidatesMixed(idx->dev, d_c.as<uint32_t>(), n_cand, d_g.as<uint32_t>(),
                                               d_i.as<double>(), n_terms, nullptr, nullptr, k1, b, avg_doc_length,
                                               d_s.as<double>(), lease.stream));
    MGX_HIP(lease.CopyBack(scores_out, d_s.p, n_cand * 8));
    return MGX_OK;
  });
}

// Page documents without a batch: one pass of document_gather_kernel over the caller's id list, on a lease.
int mgx_documents_gather(mgx_index* idx, mgx_index* mapped, const uint32_t* doc_ids, uint64_t n_docs, uint32_t n_columns,
                         const uint32_t* column_ids, const uint32_t* mapped_column_ids, uint32_t max_key_bytes,
                         uint8_t** records_out, uint64_t* stride_out) {
  namespace dc = mgx::documents;
  if (records_out) *records_out = nullptr;
  if (stride_out) *stride_out = 0;
  if (!idx || !records_out || !stride_out || (n_docs && !doc_ids) || (n_columns && (!column_ids || (mapped && !mapped_column_ids))))
    return mgx::Fail(MGX_ERR_INVALID_ARGUMENT, "mgx_documents_gather: null argument");
  if (n_columns > MGX_DOC_MAX_COLUMNS)
    return mgx::Fail(MGX_ERR_OUT_OF_RANGE, "mgx_documents_gather: more than MGX_DOC_MAX_COLUMNS (32) columns");
  if (mapped && (mapped == idx || mapped->device != idx->device || !mapped->d_doc_map.p || idx->d_doc_map.p))
    return mgx::Fail(MGX_ERR_INVALID_ARGUMENT, "mgx_documents_gather: `mapped` is a delta index (mgx_index_set_doc_map) on the device of `idx`, which is none");
  // each index's requested columns and longest key, read under that index's lock
  std::vector<dc::DevColumn> cols[2];
  uint32_t longest = 0;
  mgx_index* const side[2] = {idx, mapped};
  const uint32_t* const ids[2] = {column_ids, mapped_column_ids};
  for (int k = 0; k < 2; ++k) {
    mgx_index* ix = side[k];
    if (!ix) continue;
    std::lock_guard<std::mutex> lock(ix->mu);
    if (!ix->has_pk_bytes)
      return mgx::Fail(MGX_ERR_INVALID_ARGUMENT, "mgx_documents_gather: page documents without mgx_index_attach_primary_key_bytes");
    longest = std::max(longest, ix->max_pk_bytes);
    for (uint32_t c = 0; c < n_columns; ++c) {
      dc::DevColumn col{nullptr, nullptr};
      if (ids[k][c] != MGX_DOC_NO_COLUMN) {
        if (ids[k][c] >= ix->filter_columns.size()) return mgx::Fail(MGX_ERR_OUT_OF_RANGE, "mgx_documents_gather: unknown filter column");
        const mgx_index::FilterColumn& fc = *ix->filter_columns[ids[k][c]];
        col.values = fc.d_values.as<uint64_t>();
        col.is_null = fc.d_null.as<uint8_t>();
      }
      cols[k].push_back(col);
    }
  }
  const uint32_t key_cap = max_key_bytes ? max_key_bytes : longest;
  const uint64_t stride = dc::RecordStride(n_columns, key_cap);
  *stride_out = stride;
  if (n_docs == 0) return MGX_OK;
  if (n_docs > 0xFFFFFFFFull || n_docs * stride > MGX_DOC_ARENA_CAP)
    return mgx::Fail(MGX_ERR_OUT_OF_RANGE, "mgx_documents_gather: the records exceed MGX_DOC_ARENA_CAP (256 MiB): pass fewer ids per call "
                                           "(or lower max_key_bytes, or the columns)");
  uint8_t* host = static_cast<uint8_t*>(std::malloc(n_docs * stride));
  if (!host) return mgx::Fail(MGX_ERR_INTERNAL, "mgx_documents_gather: out of memory");
  const int rc = WithLease(idx, "mgx_documents_gather", true, [&](SingleLease& lease) {
    DevBuf d_ids, d_query, d_cols[2], d_arena;
    MGX_HIP(mgx::Upload(d_ids, doc_ids, n_docs));
    for (int k = 0; k < 2; ++k) MGX_HIP(mgx::Upload(d_cols[k], cols[k].data(), cols[k].size(), 1));
    MGX_HIP(d_arena.Alloc(n_docs * stride));
    dc::DevQuery q{};
    q.page_docs = d_ids.as<uint32_t>();
    q.limit = q.count = static_cast<uint32_t>(n_docs);
    q.n_columns = n_columns;
    q.rec_stride = stride;
    MGX_HIP(mgx::Upload(d_query, &q, 1));
    MGX_HIP(lease.Ship());
    auto source = [&](const mgx_index* ix, int k) {
      dc::DevSource src{};
      if (!ix) return src;
      src.key_bytes = ix->d_pkb_bytes.as<uint8_t>();
      src.key_off = ix->d_pkb_off.as<uint64_t>();
      src.has_key = ix->d_pkb_has.as<uint8_t>();
      src.doc_map = k == 1 ? ix->d_doc_map.as<uint32_t>() : nullptr;
      src.columns = d_cols[k].as<dc::DevColumn>();
      src.first_doc_id = ix->dev.first_doc_id;
      src.n_docs = ix->dev.n_docs;
      return src;
    };
    dc::DevBatch db{};
    db.queries = d_query.as<dc::DevQuery>();
    db.n_queries = 1;
    db.n_entries = static_cast<uint32_t>(n_docs);
    db.arena = d_arena.as<uint8_t>();
    db.plain = source(idx, 0);
    db.mapped = source(mapped, 1);
    db.key_cap = key_cap;
    MGX_LAUNCH(mgx::LaunchDocumentGather(db, lease.stream));
    MGX_HIP(lease.CopyBack(host, d_arena.p, n_docs * stride));
    return MGX_OK;
  });
  if (rc == MGX_OK)
    for (uint64_t i = 0; i < n_docs; ++i) {
      dc::Header h;
      std::memcpy(&h, host + i * stride, sizeof(h));
      if (h.flags & dc::kTruncated) {
        std::free(host);
        return mgx::Fail(MGX_ERR_OUT_OF_RANGE, "mgx_documents_gather: a key is longer than max_key_bytes");
      }
    }
  if (rc != MGX_OK) {
    std::free(host);
    return rc;
  }
  *records_out = host;
  return MGX_OK;
}

int mgx_score_documents_text(mgx_index* idx, const uint32_t* candidates, uint64_t n_cand, const uint8_t* term_bytes,
                             const uint32_t* term_off, const double* idfs, uint32_t n_terms, double avg_doc_length,
                             double k1, double b, double* scores_out) {
  if (!idx || (n_cand && (!candidates || !scores_out)) || (n_terms && (!term_off || !idfs)))
    return mgx::Fail(MGX_ERR_INVALID_ARGUMENT, "mgx_score_documents_text: null argument");
  if (!idx->can_score) return mgx::Fail(MGX_ERR_NOT_IMPLEMENTED, "index was created without tf/doc_len columns");
  if (!idx->dev.text) return mgx::Fail(MGX_ERR_INVALID_ARGUMENT, "mgx_score_documents_text: no text attached");
  for (uint32_t i = 0; i < n_terms; ++i)
    if (term_off[i + 1] < term_off[i]) return mgx::Fail(MGX_ERR_INVALID_ARGUMENT, "term offsets must ascend");
  if (n_terms && term_off[n_terms] > term_off[0] && !term_bytes)
    return mgx::Fail(MGX_ERR_INVALID_ARGUMENT, "mgx_score_documents_text: null term bytes");
  if (n_cand == 0) return MGX_OK;
  return WithLease(idx, "mgx_score_documents_text", true, [&](SingleLease& lease) {
    // the mixed scorer with text-level terms only: term t is kDeepText | t, its bytes at term_off[t] - term_off[0]
    std::vector<uint32_t> terms(n_terms);
    std::vector<mgx::DevTextTerm> text_terms(n_terms);
    for (uint32_t t = 0; t < n_terms; ++t) {
      terms[t] = mgx::kDeepText | t;
      text_terms[t] = {term_off[t] - term_off[0], term_off[t + 1] - term_off[t]};
    }
    const uint64_t n_bytes = n_terms ? term_off[n_terms] - term_off[0] : 0;
    DevBuf d_c, d_t, d_p, d_tt, d_i, d_s;
    MGX_HIP(mgx::Upload(d_c, candidates, n_cand));
    MGX_HIP(mgx::Upload(d_t, terms.data(), n_terms));
    MGX_HIP(mgx::Upload(d_p, n_bytes ? term_bytes + term_off[0] : term_bytes, n_bytes, 16));
    MGX_HIP(mgx::Upload(d_tt, text_terms.data(), n_terms));
    MGX_HIP(mgx::Upload(d_i, idfs, n_terms));
    MGX_HIP(d_s.Alloc(n_cand * 8));
    MGX_HIP(lease.Ship());
    MGX_LAUNCH(mgx::LaunchScoreCandidatesMixed(idx->dev, d_c.as<uint32_t>(), n_cand, d_t.as<uint32_t>(),
                                               d_i.as<double>(), n_terms, d_p.as<uint8_t>(),
                                               d_tt.as<mgx::DevTextTerm>(), k1, b, avg_doc_length, d_s.as<double>(),
                                               lease.stream));
    MGX_HIP(lease.CopyBack(scores_out, d_s.p, n_cand * 8));
    return MGX_OK;
  });
}

int mgx_sort_by_score(mgx_index* idx, const uint32_t* results, const double* scores, uint64_t n, int descending,
                      uint32_t limit, uint32_t offset, uint32_t** out_docs, uint64_t* out_n) {
  if (out_docs) *out_docs = nullptr;
  if (out_n) *out_n = 0;
  if (!idx || !out_docs || !out_n || (n && (!results || !scores)))
    return mgx::Fail(MGX_ERR_INVALID_ARGUMENT, "mgx_sort_by_score: null argument");
  if (n > 0xFFFFFFFFull) return mgx::Fail(MGX_ERR_OUT_OF_RANGE, "mgx_sort_by_score: more than 2^32 - 1 entries");
  const uint64_t start = std::min<uint64_t>(offset, n);
  const uint64_t end = limit == 0 ? n : std::min<uint64_t>(start + limit, n);
  // (owned here until the call has succeeded: out-parameters stay NULL/0 on every failure path)
  std::unique_ptr<uint32_t, void (*)(void*)> page(
      static_cast<uint32_t*>(std::malloc(((end - start) ? (end - start) : 1) * 4)), std::free);
  if (!page) return mgx::Fail(MGX_ERR_INTERNAL, "out of host memory");
  if (end > start) {
    const bool bounded_page = limit != 0 && static_cast<uint64_t>(offset) + limit <= mgx::kMaxNeeded;
    const int rc = WithLease(idx, "mgx_sort_by_score", true, [&](SingleLease& lease) {
      const hipStream_t stream = lease.stream;
      DevBuf d_r, d_s, d_o;
      MGX_HIP(mgx::Upload(d_r, results, n));
      MGX_HIP(mgx::Upload(d_s, scores, n));
      if (n > 4096 && !(bounded_page && n > 65536)) {
        // the full-sort fallback (result_sorter.cpp:661-716 sorts whatever it is given; deep OFFSETs are benchmarked,
        // docs/releases/v1.3.5.md:238): every pair sorted best first by the bitonic network, then the page is cut out
        // of the one sorted run by rank_merge_kernel (an element's rank is its index in the run)
        const uint64_t n2 = mgx::pages::SortCapacity(n);
        mgx::DevMergeRun run{};
        run.kind = mgx::kMergeScore;
        run.descending = descending ? 1u : 0u;
        run.a_n = static_cast<uint32_t>(n);
        run.lo = static_cast<uint32_t>(start);
        run.hi = static_cast<uint32_t>(end);
        const uint64_t run_start[2] = {0, n};
        DevBuf d_run, d_start, d_k, d_d, d_ps;
        MGX_HIP(mgx::Upload(d_run, &run, 1));
        MGX_HIP(mgx::Upload(d_start, run_start, 2));
        MGX_HIP(d_k.Alloc(n2 * 8));
        MGX_HIP(d_d.Alloc(n2 * 4));
        MGX_HIP(d_o.Alloc((end - start) * 4));
        MGX_HIP(d_ps.Alloc((end - start) * 8));  // (the page's scores: written, not returned)
        MGX_HIP(lease.Ship());
        const int rc = mgx::SortRun(d_r.as<uint32_t>(), d_s.as<double>(), n, n2, descending, d_k.as<uint64_t>(),
                                    d_d.as<uint32_t>(), stream);
        if (rc) return rc;
        MGX_LAUNCH(mgx::LaunchRankMerge(d_run.as<mgx::DevMergeRun>(), d_start.as<uint64_t>(), 1, n, nullptr,
                                        d_k.as<uint64_t>(), d_d.as<uint32_t>(), d_o.as<uint32_t>(), d_ps.as<double>(),
                                        stream));
      } else if (n > 65536) {
        // long arrays: per-wave top-(offset+limit) over strided shares, then the merge kernel of the batch path
        const uint32_t needed = static_cast<uint32_t>(std::min<uint64_t>(static_cast<uint64_t>(offset) + limit, n));
        uint32_t cap = 64;
        while (cap < needed) cap <<= 1;
        const uint32_t n_blocks = static_cast<uint32_t>(std::min<uint64_t>(256, (n + 16383) / 16384));
        const uint32_t n_lists = n_blocks * (mgx::kBlock / 64);
        mgx::DevQuery q{};
        q.needed = needed;
        q.cap = cap;
        q.limit = limit;
        q.offset = offset;
        q.descending = descending ? 1 : 0;
        const uint32_t zero = 0;
        DevBuf d_k, d_d, d_ck, d_cd, d_cn, d_q, d_id, d_ps, d_pn;
        MGX_HIP(mgx::Upload(d_q, &q, 1));
        MGX_HIP(mgx::Upload(d_id, &zero, 1));
        MGX_HIP(d_k.Alloc(n * 8));
        MGX_HIP(d_d.Alloc(n * 4));
        MGX_HIP(d_ck.Alloc(static_cast<size_t>(n_lists) * needed * 8));
        MGX_HIP(d_cd.Alloc(static_cast<size_t>(n_lists) * needed * 4));
        MGX_HIP(d_cn.Alloc(static_cast<size_t>(n_lists) * 4));
        MGX_HIP(d_o.Alloc(static_cast<size_t>(limit) * 4));
        MGX_HIP(d_ps.Alloc(static_cast<size_t>(limit) * 8));
        MGX_HIP(d_pn.Alloc(4));
        MGX_HIP(lease.Ship());
        MGX_LAUNCH(mgx::LaunchMakeSortKeys(d_r.as<uint32_t>(), d_s.as<double>(), n, descending, d_k.as<uint64_t>(),
                                           d_d.as<uint32_t>(), stream));
        MGX_LAUNCH(mgx::LaunchTopKScan(d_k.as<uint64_t>(), d_d.as<uint32_t>(), n, needed, cap, descending, n_blocks,
                                       d_ck.as<uint64_t>(), d_cd.as<uint32_t>(), d_cn.as<uint32_t>(), stream));
        MGX_LAUNCH(mgx::LaunchMergeTopK(d_q.as<mgx::DevQuery>(), d_id.as<uint32_t>(), 1, n_lists, d_ck.as<uint64_t>(),
                                        d_cd.as<uint32_t>(), d_cn.as<uint32_t>(), /*kq=*/0, /*kj=*/needed,
                                        /*dj=*/needed, /*cq=*/0, /*cj=*/1, nullptr, nullptr, nullptr, 0,
                                        d_o.as<uint32_t>(), d_ps.as<double>(), d_pn.as<uint32_t>(), limit, nullptr,
                                        nullptr, nullptr, stream));
      } else {
        DevBuf d_k, d_d;
        MGX_HIP(d_k.Alloc(n * 8));
        MGX_HIP(d_d.Alloc(n * 4));
        MGX_HIP(d_o.Alloc((end - start) * 4));
        MGX_HIP(lease.Ship());
        MGX_LAUNCH(mgx::LaunchSortByScore(d_r.as<uint32_t>(), d_s.as<double>(), n, descending,
                                          static_cast<uint32_t>(start), static_cast<uint32_t>(end), d_k.as<uint64_t>(),
                                          d_d.as<uint32_t>(), d_o.as<uint32_t>(), stream));
      }
      MGX_HIP(lease.CopyBack(page.get(), d_o.p, (end - start) * 4));
      return MGX_OK;
    });
    if (rc) return rc;
  }
  *out_docs = page.release();
  *out_n = end - start;
  return MGX_OK;
}

}  // extern "C"

extern "C" void mgxt_fail_device_allocs(int after, int count) {
  mgx::g_fail_count.store(count > 0 ? count : 0);
  mgx::g_fail_after.store(count > 0 && after >= 0 ? after : -1);
}

extern "C" int mgxt_measure_read_bandwidth(int device, uint64_t bytes, int iters, double* gb_per_s) {
  if (!gb_per_s || bytes < (1ull << 20) || iters < 1) return mgx::Fail(MGX_ERR_INVALID_ARGUMENT, "read probe: bad arguments");
  *gb_per_s = 0.0;
  MGX_HIP(hipSetDevice(device));
  bytes &= ~static_cast<uint64_t>(15);
  void* buf = nullptr;
  uint32_t* sink = nullptr;
  MGX_HIP(hipMalloc(&buf, bytes));
  if (hipMalloc(reinterpret_cast<void**>(&sink), 4) != hipSuccess) {
    (void)hipFree(buf);
    return mgx::Fail(MGX_ERR_INTERNAL, "read probe: hipMalloc failed");
  }
  hipEvent_t e0 = nullptr, e1 = nullptr;
  int rc = MGX_OK;
  float best = 0.f;
  do {
    if (hipMemset(buf, 0x5A, bytes) != hipSuccess || hipEventCreate(&e0) != hipSuccess ||
        hipEventCreate(&e1) != hipSuccess) {
      rc = mgx::Fail(MGX_ERR_INTERNAL, "read probe: setup failed");
      break;
    }
    for (int i = 0; i < iters + 1 && rc == MGX_OK; ++i) {  // first launch is a warm-up
      (void)hipEventRecord(e0, nullptr);
      if (mgx::LaunchReadProbe(buf, bytes, sink, nullptr) != 0) rc = mgx::Fail(MGX_ERR_INTERNAL, "read probe: launch failed");
      (void)hipEventRecord(e1, nullptr);
      if (hipEventSynchronize(e1) != hipSuccess) rc = mgx::Fail(MGX_ERR_INTERNAL, "read probe: kernel failed");
      float ms = 0.f;
      (void)hipEventElapsedTime(&ms, e0, e1);
      if (i > 0 && ms > 0.f && (best == 0.f || ms < best)) best = ms;
    }
  } while (false);
  if (e0) (void)hipEventDestroy(e0);
  if (e1) (void)hipEventDestroy(e1);
  (void)hipFree(sink);
  (void)hipFree(buf);
  if (rc == MGX_OK && best > 0.f) *gb_per_s = static_cast<double>(bytes) / (best * 1e-3) / 1e9;
  return rc;
}
