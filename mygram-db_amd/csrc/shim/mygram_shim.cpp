// mygram_shim.cpp — host C++17 implementation of mygram_shim.hpp over the C ABI of libmygram_gpu.so.
// Host-side rules are cited from the reference (paths relative to its tree); all posting work goes to the device.
#include "mygram_shim.hpp"

#include "../mgx_highlight.hpp"
#include "../mgx_text.hpp"

#include <algorithm>
#include <atomic>
#include <charconv>
#include <chrono>
#include <cstring>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <condition_variable>
#include <deque>
#include <functional>
#include <future>
#include <iterator>
#include <map>
#include <mutex>
#include <set>
#include <thread>
#include <unordered_map>

#include <pthread.h>

namespace mygramdb {

using mygram::utils::Error;
using mygram::utils::ErrorCode;
using mygram::utils::Expected;
using mygram::utils::MakeError;
using mygram::utils::MakeUnexpected;

namespace {

// ---- n-gram rules over the shared text implementation (../mgx_text.hpp: UTF-8 decode string_utils.cpp:94-218,
//      IsCJKIdeograph :441-448, window rule :452-509) -------------------------------------------------------------------

struct CodePoints {
  std::vector<uint32_t> cp;
  std::vector<std::pair<uint32_t, uint32_t>> span;  // byte [begin, end) of every decoded code point
};

CodePoints Decode(std::string_view text) {
  CodePoints out;
  mgx::text::Decode(reinterpret_cast<const uint8_t*>(text.data()), text.size(), &out.cp, &out.span);
  return out;
}

using mgx::text::IsCjkIdeographPipeline;

// src/server/search_pipeline.cpp:80-136 HasUncoveredHybridFragment: a mixed-script term with a code point that no
// query n-gram covers (windows here follow the pipeline's own, wider ideograph predicate)
bool HasUncoveredHybridFragment(std::string_view normalized, int ngram_size, int kanji_ngram_size, bool cross) {
  if (normalized.empty() || kanji_ngram_size <= 0) return false;
  const int ascii_n = ngram_size > 0 ? ngram_size : 2;
  const CodePoints cps = Decode(normalized);
  const size_t n = cps.cp.size();
  if (n < 2) return false;
  bool has_cjk = false, has_other = false;
  for (uint32_t c : cps.cp) (IsCjkIdeographPipeline(c) ? has_cjk : has_other) = true;
  if (!has_cjk || !has_other) return false;
  std::vector<bool> covered(n, false);
  for (size_t i = 0; i < n; ++i) {
    const bool start_is_cjk = IsCjkIdeographPipeline(cps.cp[i]);
    const int w = start_is_cjk ? kanji_ngram_size : ascii_n;
    if (w <= 0 || i + static_cast<size_t>(w) > n) continue;
    bool crossed = false;
    if (!cross)
      for (int j = 1; j < w; ++j) crossed = crossed || IsCjkIdeographPipeline(cps.cp[i + j]) != start_is_cjk;
    if (crossed) continue;
    for (int j = 0; j < w; ++j) covered[i + j] = true;
  }
  for (bool c : covered)
    if (!c) return true;
  return false;
}

// bytes of code points [a, b): contiguous in the source when no invalid byte sits between them; re-assembled from the
// decoded spans otherwise (CodepointsToUtf8 :241-272 re-encodes, which is the same bytes for valid input)
std::string Window(std::string_view text, const CodePoints& cps, size_t a, size_t b) {
  std::string s;
  for (size_t i = a; i < b; ++i) s.append(text.substr(cps.span[i].first, cps.span[i].second - cps.span[i].first));
  return s;
}

std::vector<std::string> GenerateNgrams(std::string_view text, int n) {  // :382-423
  std::vector<std::string> out;
  const CodePoints cps = Decode(text);
  if (cps.cp.empty() || n <= 0 || cps.cp.size() < static_cast<size_t>(n)) return out;
  for (size_t i = 0; i + static_cast<size_t>(n) <= cps.cp.size(); ++i) out.push_back(Window(text, cps, i, i + n));
  return out;
}

std::vector<std::string> GenerateHybridNgrams(std::string_view text, int ascii_n, int kanji_n, bool cross) {  // :452-509
  std::vector<std::string> out;
  if (ascii_n <= 0 || kanji_n <= 0) return out;
  const CodePoints cps = Decode(text);
  for (size_t i = 0; i < cps.cp.size(); ++i) {
    const int w = mgx::text::WindowAt(cps.cp, i, ascii_n, kanji_n, cross);  // the builder's own window rule
    if (w != 0) out.push_back(Window(text, cps, i, i + static_cast<size_t>(w)));
  }
  return out;
}

std::vector<std::string> GenerateQueryNgrams(std::string_view normalized, int ngram, int kanji, bool cross) {  // :639-653
  if (kanji > 0) return GenerateHybridNgrams(normalized, ngram > 0 ? ngram : 2, kanji, cross);
  if (ngram == 0) return GenerateHybridNgrams(normalized, 2, 1, true);
  return GenerateNgrams(normalized, ngram);
}

void DeduplicateSorted(std::vector<std::string>& v) {  // string_utils.h:192-196
  std::sort(v.begin(), v.end());
  v.erase(std::unique(v.begin(), v.end()), v.end());
}

std::vector<storage::DocId> Take(uint32_t* p, uint64_t n) {
  std::vector<storage::DocId> v(p, p + n);
  mgx_free(p);
  return v;
}

}  // namespace

// =================================================================================================================
// storage::FilterValue keys
// =================================================================================================================

namespace storage {

std::string SerializeFilterValue(const FilterValue& value) {  // src/storage/filter_index.cpp:177-258 (little-endian host)
  return std::visit(
      [](const auto& val) -> std::string {
        using T = std::decay_t<decltype(val)>;
        auto raw = [](char tag, const void* p, size_t n) {
          std::string r(1 + n, '\0');
          r[0] = tag;
          std::memcpy(&r[1], p, n);
          return r;
        };
        if constexpr (std::is_same_v<T, std::monostate>) return std::string(1, '\x00');
        else if constexpr (std::is_same_v<T, bool>) return std::string{'\x01', val ? '\x01' : '\x00'};
        else if constexpr (std::is_same_v<T, std::string>) return std::string(1, '\x0B') + val;
        else if constexpr (std::is_same_v<T, double>) return raw('\x0C', &val, sizeof(double));
        else if constexpr (std::is_same_v<T, TimeValue>) return raw('\x0A', &val.seconds, sizeof(int64_t));
        else if constexpr (std::is_same_v<T, int8_t>) return raw('\x02', &val, 1);
        else if constexpr (std::is_same_v<T, uint8_t>) return raw('\x03', &val, 1);
        else if constexpr (std::is_same_v<T, int16_t>) return raw('\x04', &val, 2);
        else if constexpr (std::is_same_v<T, uint16_t>) return raw('\x05', &val, 2);
        else if constexpr (std::is_same_v<T, int32_t>) return raw('\x06', &val, 4);
        else if constexpr (std::is_same_v<T, uint32_t>) return raw('\x07', &val, 4);
        else if constexpr (std::is_same_v<T, int64_t>) return raw('\x08', &val, 8);
        else return raw('\x09', &val, 8);  // uint64_t
      },
      value);
}

std::string FilterValueToDisplayString(const FilterValue& value) {  // DeserializeToDisplayString, filter_index.cpp:314-407
  return std::visit(
      [](const auto& val) -> std::string {
        using T = std::decay_t<decltype(val)>;
        if constexpr (std::is_same_v<T, std::monostate>) return "NULL";
        else if constexpr (std::is_same_v<T, bool>) return val ? "true" : "false";
        else if constexpr (std::is_same_v<T, std::string>) return val;
        else if constexpr (std::is_same_v<T, TimeValue>) return std::to_string(val.seconds);
        else if constexpr (std::is_same_v<T, double>) {
          char buf[32];
          auto [ptr, ec] = std::to_chars(buf, buf + sizeof(buf), val);
          return ec != std::errc() ? std::string() : std::string(buf, ptr);
        } else return std::to_string(val);
      },
      value);
}

}  // namespace storage

// =================================================================================================================
// index::Index
// =================================================================================================================

namespace index {

namespace {
// the Index whose device this thread touched last, and the one finalised last in the process: where the index-less
// ResultSorter::SortByScore (the reference's signature) runs
thread_local const Index* tl_last_index = nullptr;
std::atomic<const Index*> g_last_finalized{nullptr};
thread_local std::string tl_device_error;
// every std::vector-returning method: cleared on entry ...
void ClearDeviceError() { tl_device_error.clear(); }
}  // namespace
const std::string& LastDeviceError() { return tl_device_error; }
const Index* LastUsedIndex() { return tl_last_index ? tl_last_index : g_last_finalized.load(); }
// ... and set where the C ABI (or the index build) reports a failure
static void SetDeviceError(const std::string& msg) { tl_device_error = msg.empty() ? "device failure" : msg; }
void ClearDeviceErrorForSorter() { ClearDeviceError(); }

struct Index::Impl {
  int device = 0;
  double dense_threshold = 0.0;
  std::atomic<int> build_mode{Index::kHost};  // SetBuildMode / SetDeviceBuild: who builds a generation's column arrays
  // BuildCounters: generations built per mode since creation. A delta index is an Index of its own: its generations are
  // counted where `built_sink` points, the table's array.
  std::atomic<uint64_t> built[3] = {{0}, {0}, {0}};
  std::atomic<uint64_t>* built_sink = built;
  int query_kanji = 0;  // table-config kanji size used for QUERY n-grams (the Index itself keeps kanji = ngram if 0)
  mutable std::mutex mu;
  mutable std::map<DocId, std::string> pending;  // documents recorded before the first search
  // The primary key of every document of the table that has one (AddDocument(..., primary_key), a dump's keys): what
  // SORT by primary key orders by. Kept here for the table's lifetime, as the reference's DocumentStore keeps them: every
  // index built from the table's documents (main, delta, a compacted main) takes its slots' keys from it. Under mu.
  mutable std::map<DocId, std::string> primary_keys;
  // the device index that holds the table's raw key bytes (mgx_index_attach_primary_key_bytes; page documents): not `dev`
  // until the first batch that asks for documents, and again after Compact() installed a new one. Under mu.
  mutable mgx_index* pk_bytes_dev = nullptr;
  // a delta index: the table id of each of its slots (its doc map), kept with the index itself so that a batch that still
  // runs on this delta after the table built a newer one can attach its key bytes. Written once, before the delta is shared.
  std::vector<DocId> doc_map_ids;
  std::string primary_key_column;  // SetPrimaryKeyColumn
  // The original text of every document of the table that has one (AddDocument(..., original_text)), kept like the keys
  // and for the same span; `invalid_originals`: those that are not valid UTF-8, which the host renders. Under mu.
  mutable std::map<DocId, std::string> originals;
  mutable std::set<DocId> invalid_originals;
  mutable mgx_columns* cols = nullptr;
  mutable mgx_index* dev = nullptr;
  mutable mgx_columns_view view{};
  mutable bool finalized = false;
  mutable std::string last_error;
  mutable bool has_gaps = false;       // ids inside [first, last] that were never added
  mutable uint32_t exists_bitmap = 0;  // filter bitmap of the ids that were (only when has_gaps)

  bool internal = false;  // a delta index BuildDelta made: never the index the index-less SortByScore resolves to
  // doc-range shards: table-wide statistics (empty / 0: this index is the whole table)
  std::vector<uint64_t> global_sizes;
  uint64_t global_docs = 0;
  double global_avgdl = 0.0;

  // One generation of the main index. `cols` / `dev` above are the current generation's; a compaction publishes a new one,
  // and whoever still holds batch objects compiled on the old device index (an executor's slots) keeps the old generation
  // alive through its own reference until those objects are gone.
  struct Handles {
    mgx_columns* cols = nullptr;
    mgx_index* dev = nullptr;
    bool owns = true;
    ~Handles() {
      if (dev && owns) mgx_index_destroy(dev);
      if (cols && owns) mgx_columns_destroy(cols);
    }
  };
  mutable std::shared_ptr<Handles> handles;
  bool Lookup(std::string_view gram, uint32_t* id) const {
    int found = 0;
    if (!cols) return false;
    mgx_columns_lookup(cols, reinterpret_cast<const uint8_t*>(gram.data()), gram.size(), id, &found);
    return found != 0;
  }
  // posting size the planner sees (EstimatePostingSize / df): table-wide when the index is one shard of a table
  uint64_t Size(uint32_t id) const {
    return global_sizes.empty() ? view.offsets[id + 1] - view.offsets[id] : global_sizes[id];
  }
  // The planner's view of a gram: its id for the device and its table-wide size. A gram some OTHER shard holds resolves to
  // MGX_GRAM_ABSENT (an empty operand here) with that table-wide size, so every rank plans the same batch.
  bool Resolve(std::string_view gram, uint32_t* id, uint64_t* size) const {
    if (Lookup(gram, id)) {
      *size = Size(*id);
      return true;
    }
    if (!absent_grams.empty()) {
      const auto it = absent_grams.find(std::string(gram));
      if (it != absent_grams.end()) {
        *id = MGX_GRAM_ABSENT;
        *size = it->second;
        return true;
      }
    }
    if (fallback != nullptr) {  // a delta index: the main index's dictionary says what the rest of the table holds
      uint32_t mid = 0;
      if (fallback->Lookup(gram, &mid)) {
        *id = MGX_GRAM_ABSENT;
        *size = fallback->Size(mid);
        return true;
      }
    }
    return false;
  }
  std::unordered_map<std::string, uint64_t> absent_grams;  // grams of the table this shard has no posting for -> size
  const Impl* fallback = nullptr;

  // ---- mutable tables: changes recorded after the index was built (all under mu) ------------------------------------------
  // What one application works from: how much of the recorded state it covers. It reads that state and consumes nothing;
  // CommitMutations does, once the device has taken it all.
  struct Snapshot {
    uint64_t recorded = 0;           // Mutable::recorded when it was taken
    size_t n_clear = 0, n_dead = 0;  // the prefix of pending_clear / pending_dead_* it covers
    bool delta_changed = false;      // the delta's documents changed since the last application
    uint64_t main_docs = 0, main_len = 0;
  };
  struct BuiltDelta {
    bool rebuilt = false;
    std::shared_ptr<Index> delta;  // nullptr with rebuilt: the delta is empty now
    std::shared_ptr<const std::vector<DocId>> ids;
    std::string error;
  };
  struct Mutable {
    bool active = false;  // a change was ever recorded (the bookkeeping below exists)
    // every recording call bumps `recorded`; the device has seen the changes up to `applied` (behind: recorded != applied);
    // delta_recorded is `recorded` as of the last change to delta_docs / delta_filters (the delta changed: > applied)
    uint64_t recorded = 0, applied = 0, delta_recorded = 0;
    void Record(bool delta) {
      ++recorded;
      if (delta) delta_recorded = recorded;
    }
    bool retry = false;  // the last application failed: the next entry point applies in its own call, whatever the bound
    std::vector<uint64_t> main_live;            // live documents of the main index, by slot
    // append-only between applications (an application covers a prefix, CommitMutations erases it):
    std::vector<DocId> pending_clear;           // main documents removed / superseded since the last apply
    std::vector<uint32_t> pending_dead_grams;   // their distinct n-grams (main gram ids): one posting less each
    std::vector<DocId> pending_dead_docs;       // parallel to pending_dead_grams: the document of each posting
    std::map<DocId, std::string> delta_docs;    // documents of the delta index: table id -> normalized text
    std::map<DocId, storage::FilterMap> delta_filters;
    uint64_t main_docs = 0, main_len = 0;       // BM25Stats share of the main index's live documents
    uint64_t removed = 0, epoch = 0;
    std::chrono::microseconds staleness{0};                 // SetMutationStaleness
    std::chrono::steady_clock::time_point last_apply{};     // when the device state was last brought up to date
    uint32_t live_bitmap = 0;
    bool have_live = false;                     // the device holds row live_bitmap (made by the first install, tried or done)
    std::vector<uint64_t> applied_live;         // main_live as of the last application: what the DEVICE's live row says
    // background application (SetMutationStaleness > 0): the delta of build_snapshot is built by a thread of its own (it
    // needs no lock: BuildDelta) while queries keep running on the old state; the first entry point that finds the future
    // ready installs it
    std::future<BuiltDelta> build;
    Snapshot build_snapshot;
    std::shared_ptr<Index> delta;               // the delta index the device holds (nullptr: none)
    std::shared_ptr<const std::vector<DocId>> delta_ids;  // its doc map: local id - 1 -> table id, ascending
    std::vector<std::pair<uint32_t, uint64_t>> delta_contrib;  // (main gram id, the delta's posting count) inside global_sizes
  };
  mutable Mutable mut;
  mutable std::vector<uint64_t> exists_bits;  // has_gaps: the ids that were added, by slot
  bool LiveInMain(DocId doc) const {
    if (!mut.active || doc < view.first_doc_id || doc - view.first_doc_id >= view.n_docs) return false;
    const uint64_t slot = doc - view.first_doc_id;
    return (mut.main_live[slot >> 6] >> (slot & 63)) & 1;
  }
  // ... as the device's live row has it (changes recorded but not yet applied do not count): what the single operators
  // must filter by, so that they agree with the delta index the device holds
  bool LiveApplied(DocId doc) const {
    if (!mut.active || doc < view.first_doc_id || doc - view.first_doc_id >= view.n_docs) return false;
    const uint64_t slot = doc - view.first_doc_id;
    return (mut.applied_live[slot >> 6] >> (slot & 63)) & 1;
  }

  // ---- filter columns (DocumentStore filter values + FilterIndex, on the device by doc slot) -------------------------
  struct FilterColumn {
    std::string name;
    size_t type = 0;      // index of the FilterValue alternative every non-NULL value holds (0: the column is all NULL)
    uint32_t device_id = 0;
    std::vector<storage::FilterValue> dict;  // distinct non-NULL values, ascending (strings bytewise): value id = position
  };
  mutable std::mutex filter_mu;  // columns, the condition cache
  mutable std::vector<FilterColumn> filter_columns;
  mutable std::unordered_map<std::string, std::pair<uint32_t, bool>> condition_cache;  // key -> (bitmap id, negate)
  mutable std::map<DocId, storage::FilterMap> pending_filters;  // AddDocument(..., filters) before the first search
  mutable uint32_t empty_bitmap = 0;
  mutable bool have_empty_bitmap = false;

  // One generation of the main index as BuildGeneration makes it, off to the side: nothing of an Impl refers to it until
  // Install publishes all of it in one step (mu held; filter_mu is taken here, in the order every writer uses).
  struct Generation {
    std::shared_ptr<Handles> handles;
    mgx_columns_view view{};
    bool has_gaps = false;
    uint32_t exists_bitmap = 0;
    std::vector<uint64_t> exists_bits;
    std::vector<FilterColumn> filter_columns;
  };
  void Install(Generation&& g) const {
    std::lock_guard<std::mutex> fl(filter_mu);
    handles = std::move(g.handles);
    cols = handles->cols;
    dev = handles->dev;
    view = g.view;
    has_gaps = g.has_gaps;
    exists_bitmap = g.exists_bitmap;
    exists_bits = std::move(g.exists_bits);
    filter_columns = std::move(g.filter_columns);
    condition_cache.clear();
    have_empty_bitmap = false;
    pk_bytes_dev = nullptr;
  }

  // FilterIndex::ResolveColumnName (filter_index.cpp:122-147): exact name first, else the one unambiguous ASCII
  // case-insensitive match
  const FilterColumn* ResolveColumn(std::string_view name) const {
    const FilterColumn* hit = nullptr;
    for (const auto& c : filter_columns)
      if (c.name == name) return &c;
    for (const auto& c : filter_columns) {
      if (c.name.size() != name.size()) continue;
      bool same = true;
      for (size_t i = 0; same && i < name.size(); ++i)
        same = std::tolower(static_cast<unsigned char>(c.name[i])) == std::tolower(static_cast<unsigned char>(name[i]));
      if (!same) continue;
      if (hit) return nullptr;
      hit = &c;
    }
    return hit;
  }
};

Index::Index(int ngram_size, int kanji_ngram_size, double roaring_threshold, bool cross_boundary_ngrams,
             bool normalize_nfkc, const std::string& normalize_width, bool normalize_lower, int device)
    : ngram_size_(ngram_size),
      kanji_ngram_size_(kanji_ngram_size > 0 ? kanji_ngram_size : ngram_size),  // index.cpp:31
      cross_boundary_(cross_boundary_ngrams),
      normalize_nfkc_(normalize_nfkc),
      normalize_width_(normalize_width),
      normalize_lower_(normalize_lower),
      impl_(std::make_unique<Impl>()) {
  impl_->device = device;
  impl_->dense_threshold = roaring_threshold;
  impl_->query_kanji = kanji_ngram_size;
}

namespace {
storage::FilterValue FilterValueFromBits(size_t type, uint64_t w, const std::vector<storage::FilterValue>& dict) {
  switch (type) {
    case 1: return w != 0;
    case 2: return static_cast<int8_t>(static_cast<int64_t>(w));
    case 3: return static_cast<uint8_t>(w);
    case 4: return static_cast<int16_t>(static_cast<int64_t>(w));
    case 5: return static_cast<uint16_t>(w);
    case 6: return static_cast<int32_t>(static_cast<int64_t>(w));
    case 7: return static_cast<uint32_t>(w);
    case 8: return static_cast<int64_t>(w);
    case 9: return static_cast<uint64_t>(w);
    case 10: return storage::TimeValue{static_cast<int64_t>(w)};
    case 11: return w < dict.size() ? dict[w] : storage::FilterValue{};  // strings are stored as dictionary ranks
    case 12: {
      double d;
      std::memcpy(&d, &w, 8);
      return d;
    }
    default: return storage::FilterValue{};
  }
}

// widened device value of a non-NULL FilterValue (strings: their dictionary rank, filled in by the caller)
uint64_t WidenFilterValue(const storage::FilterValue& v) {
  return std::visit(
      [](const auto& val) -> uint64_t {
        using T = std::decay_t<decltype(val)>;
        if constexpr (std::is_same_v<T, std::monostate> || std::is_same_v<T, std::string>) return 0;
        else if constexpr (std::is_same_v<T, storage::TimeValue>) return static_cast<uint64_t>(val.seconds);
        else if constexpr (std::is_same_v<T, double>) {
          uint64_t u;
          std::memcpy(&u, &val, 8);
          return u;
        } else if constexpr (std::is_signed_v<T> || std::is_same_v<T, bool>) return static_cast<uint64_t>(static_cast<int64_t>(val));
        else return static_cast<uint64_t>(val);
      },
      v);
}
uint32_t FilterClassOf(size_t type) {  // MGX_FC_* of a FilterValue alternative
  switch (type) {
    case 12: return MGX_FC_DOUBLE;
    case 3: case 5: case 7: case 9: case 11: return MGX_FC_UNSIGNED;
    default: return MGX_FC_SIGNED;  // bool, int8/16/32/64, TimeValue
  }
}

// One filter column on a device index of n_docs doc slots: its dictionary and the device column. Touches no Impl.
std::string BuildFilterColumn(mgx_index* dev, uint64_t n_docs, const std::string& name,
                              const std::vector<storage::FilterValue>& values, Index::Impl::FilterColumn* out) {
  if (values.size() != n_docs) return "AddFilterColumn: one value per doc slot of the index";
  Index::Impl::FilterColumn col;
  col.name = name;
  for (const auto& v : values) {
    if (v.index() == 0) continue;
    if (col.type == 0) col.type = v.index();
    if (v.index() != col.type) return "AddFilterColumn: the values of one column must hold one type";
  }
  std::vector<storage::FilterValue> nn;
  for (const auto& v : values)
    if (v.index() != 0) nn.push_back(v);
  std::sort(nn.begin(), nn.end());
  nn.erase(std::unique(nn.begin(), nn.end()), nn.end());
  col.dict = std::move(nn);
  const size_t n = values.size();
  std::vector<uint64_t> wide(n, 0);
  std::vector<uint8_t> nul(n, 0);
  std::vector<uint32_t> ids(n, 0xFFFFFFFFu);
  for (size_t i = 0; i < n; ++i) {
    if (values[i].index() == 0) {
      nul[i] = 1;
      continue;
    }
    const auto it = std::lower_bound(col.dict.begin(), col.dict.end(), values[i]);
    ids[i] = static_cast<uint32_t>(it - col.dict.begin());
    wide[i] = col.type == 11 ? ids[i] : WidenFilterValue(values[i]);  // strings compare by their bytewise rank
  }
  mgx_filter_column_desc d{sizeof(mgx_filter_column_desc), MGX_ABI_VERSION, FilterClassOf(col.type),
                           static_cast<uint32_t>(col.dict.size()), wide.data(), nul.data(), ids.data()};
  if (mgx_index_add_filter_column(dev, &d, &col.device_id) != MGX_OK) return mgx_last_error();
  *out = std::move(col);
  return "";
}

// Filter values recorded per document as one value vector of n slots per column name: `names` first, then every other
// name a document carries, in the order met. slot(doc) is the document's place in the vectors (>= n: it has none).
using NamedValues = std::vector<std::pair<std::string, std::vector<storage::FilterValue>>>;
template <class SlotOf>
NamedValues ValuesByName(const std::map<DocId, storage::FilterMap>& filters, std::vector<std::string> names, uint64_t n,
                         SlotOf slot) {
  for (const auto& kv : filters)
    for (const auto& f : kv.second)
      if (std::find(names.begin(), names.end(), f.first) == names.end()) names.push_back(f.first);
  NamedValues out;
  for (auto& name : names) out.emplace_back(std::move(name), std::vector<storage::FilterValue>(n));
  for (const auto& kv : filters) {
    const uint64_t s = slot(kv.first);
    if (s >= n) continue;
    for (auto& col : out) {
      const auto fv = kv.second.find(col.first);
      if (fv != kv.second.end()) col.second[s] = fv->second;
    }
  }
  return out;
}

// What a generation of the main index is built from.
struct GenerationSpec {
  int device = 0;
  double dense_threshold = 0.0;
  int ngram = 2, kanji = 1;
  bool cross = true;
  mgx_columns* cols = nullptr;          // column arrays that exist already (a dump's: taken over); else built from the texts
  const uint8_t* text_bytes = nullptr;  // the texts by doc slot, 16 bytes of padding behind them (nullptr: none are kept)
  const uint64_t* text_off = nullptr;
  DocId first = 1;
  uint64_t n = 0;
  int build_mode = Index::kHost;  // Index::BuildMode: kDeviceColumns builds the column arrays on `device`, kDeviceResident
                                  // the device index with them (the host builds what the device builder declines)
  std::atomic<uint64_t>* built = nullptr;  // [3], by the mode that did build the generation (BuildCounters)
  const std::vector<DocId>* existing = nullptr;  // the ids that exist, when some of [first, first + n) do not
  const NamedValues* columns = nullptr;          // filter values by doc slot
  const std::map<DocId, std::string>* primary_keys = nullptr;  // the table's (those of [first, first + n) are taken)
  const std::map<DocId, std::string>* originals = nullptr;     // likewise; needs text_bytes and `normalizer`
  std::function<std::string(std::string_view)> normalizer = nullptr;  // the index's NormalizeText
};

// The original texts of an index's doc slots to the device (mgx_index_attach_original_text), with the map of each
// (query::BuildOriginalMap). doc_of(slot): the slot's table id, ascending; text_bytes / text_off: the normalized texts by
// slot. An original that is not valid UTF-8 is left out (kind "none": the host renders that document's entries). An
// index none of whose documents has an original gets none and keeps launching the kernel it always launched.
template <class DocOf>
std::string UploadOriginals(mgx_index* dev, const std::map<DocId, std::string>& originals, uint64_t n, DocOf doc_of,
                            const uint8_t* text_bytes, const uint64_t* text_off,
                            const std::function<std::string(std::string_view)>& normalizer) {
  if (originals.empty() || !text_bytes || !normalizer) return "";
  std::vector<uint8_t> bytes, kind(n + 1, MGX_ORIG_NONE);
  std::vector<uint32_t> pairs;
  std::vector<uint64_t> off(n + 1, 0), map_off(n + 1, 0);
  bool any = false;
  auto it = n ? originals.lower_bound(doc_of(0)) : originals.end();
  for (uint64_t slot = 0; slot < n; ++slot) {
    const DocId doc = doc_of(slot);
    while (it != originals.end() && it->first < doc) ++it;
    if (it != originals.end() && it->first == doc && mygram::utils::IsValidUtf8(it->second)) {
      const std::string_view normalized(reinterpret_cast<const char*>(text_bytes) + text_off[slot], text_off[slot + 1] - text_off[slot]);
      query::OriginalMap m = query::BuildOriginalMap(it->second, normalized, normalizer);
      kind[slot] = static_cast<uint8_t>(m.kind);
      bytes.insert(bytes.end(), it->second.begin(), it->second.end());
      pairs.insert(pairs.end(), m.pairs.begin(), m.pairs.end());
      any = true;
    }
    off[slot + 1] = bytes.size();
    map_off[slot + 1] = pairs.size() / 2;
  }
  if (!any) return "";
  bytes.push_back(0);  // (an address even when every original is empty)
  pairs.push_back(0);
  return mgx_index_attach_original_text(dev, bytes.data(), off.data(), kind.data(), pairs.data(), map_off.data()) == MGX_OK
             ? "" : mgx_last_error();
}

// The primary keys of an index's doc slots to the device (mgx_index_set_primary_keys). doc_of(slot): the slot's table id,
// ascending with the slot (one walk over the table's keys).
// An index none of whose documents has a key gets none: its documents then sort by doc id, which is what each would do.
template <class DocOf>
std::string UploadPrimaryKeys(mgx_index* dev, const std::map<DocId, std::string>& keys, uint64_t n, DocOf doc_of) {
  if (keys.empty()) return "";
  std::vector<uint8_t> bytes, has(n, 0);
  std::vector<uint64_t> off(n + 1, 0);
  bool any = false;
  auto it = n ? keys.lower_bound(doc_of(0)) : keys.end();
  for (uint64_t slot = 0; slot < n; ++slot) {
    const DocId doc = doc_of(slot);
    while (it != keys.end() && it->first < doc) ++it;
    if (it != keys.end() && it->first == doc) {
      bytes.insert(bytes.end(), it->second.begin(), it->second.end());
      has[slot] = 1;
      any = true;
    }
    off[slot + 1] = bytes.size();
  }
  if (!any) return "";
  bytes.push_back(0);  // (an address even when every key is empty)
  return mgx_index_set_primary_keys(dev, bytes.data(), off.data(), has.data()) == MGX_OK ? "" : mgx_last_error();
}

// One generation of the main index: column arrays, device index, texts, the exists row, every filter column. It touches
// no Impl (Impl::Install publishes the result); when it fails, what it made is freed and `out` is as it was.
std::string BuildGeneration(const GenerationSpec& in, Index::Impl::Generation* out) {
  static const bool kTrace = std::getenv("MGX_TRACE_HOST") != nullptr;
  Index::Impl::Generation g;
  g.handles = std::make_shared<Index::Impl::Handles>();  // (owns what follows: gone with `g` on every early return)
  g.handles->cols = in.cols;
  const auto t0 = std::chrono::steady_clock::now();
  bool on_device = false, resident = false;
  if (!g.handles->cols) {
    mgx_build_params bp{sizeof(mgx_build_params), MGX_ABI_VERSION, in.ngram, in.kanji, in.cross ? 1 : 0, 0};
    int rc = MGX_ERR_NOT_IMPLEMENTED;
    if (in.build_mode == Index::kDeviceResident && in.text_bytes) {
      // columns, device index and attached texts with one call: the postings and the texts stay on the device. The
      // generation's columns are the dictionary (view.docids / view.tf are null; nothing below reads them). Declined
      // builds fall to the host like the device builder's.
      mgx_index_build_desc bd{sizeof(mgx_index_build_desc), MGX_ABI_VERSION, in.device, 0, in.dense_threshold, 1, 0};
      rc = mgx_index_build_device(&bp, &bd, in.text_bytes, in.text_off, in.first, in.n, &g.handles->cols, &g.handles->dev);
      resident = rc == MGX_OK;
      if (rc != MGX_OK) {
        g.handles->cols = nullptr;
        g.handles->dev = nullptr;
        if (rc != MGX_ERR_NOT_IMPLEMENTED && rc != MGX_ERR_OUT_OF_RANGE) return mgx_last_error();
      }
    } else if (in.build_mode != Index::kHost) {
      // what the device builder declines (grams of more than 3 code points, no room on the device) the host builds: the
      // result is the same by contract. Every other error is the caller's.
      rc = mgx_columns_build_device(&bp, in.text_bytes, in.text_off, in.first, in.n, in.device, &g.handles->cols);
      on_device = rc == MGX_OK;
      if (rc != MGX_OK && rc != MGX_ERR_NOT_IMPLEMENTED && rc != MGX_ERR_OUT_OF_RANGE) {
        g.handles->cols = nullptr;
        return mgx_last_error();
      }
    }
    if (rc != MGX_OK && mgx_columns_build(&bp, in.text_bytes, in.text_off, in.first, in.n, &g.handles->cols) != MGX_OK) {
      g.handles->cols = nullptr;
      return mgx_last_error();
    }
    if (in.built) in.built[resident ? Index::kDeviceResident : on_device ? Index::kDeviceColumns : Index::kHost]++;
  }
  const auto t1 = std::chrono::steady_clock::now();
  mgx_columns_view_get(g.handles->cols, &g.view);
  const auto& v = g.view;
  if (!resident) {
    mgx_index_desc d{sizeof(mgx_index_desc), MGX_ABI_VERSION, in.device, 0, v.first_doc_id, v.n_docs, v.n_grams,
                     v.offsets,               v.docids,        v.tf,      v.doc_len, in.dense_threshold,
                     v.tf_overflow_pos,       v.tf_overflow_val, v.n_tf_overflow};
    if (mgx_index_create(&d, &g.handles->dev) != MGX_OK) {
      g.handles->dev = nullptr;
      return mgx_last_error();
    }
  }
  mgx_index* dev = g.handles->dev;
  const auto t2 = std::chrono::steady_clock::now();
  // the shim's Index is also the DocumentStore of the texts it was given: BM25 terms longer than one n-gram are
  // counted in the text on the device
  if (!resident && in.text_bytes && mgx_index_attach_text(dev, in.text_bytes, in.text_off) != MGX_OK) return mgx_last_error();
  if (kTrace)
    fprintf(stderr, "[shim] generation of %llu docs: columns (%s) %.2f ms, device index %.2f ms, texts %.2f ms\n",
            static_cast<unsigned long long>(v.n_docs),
            in.cols ? "given" : resident ? "resident" : on_device ? "device builder" : "host builder",
            std::chrono::duration<double, std::milli>(t1 - t0).count(),
            std::chrono::duration<double, std::milli>(t2 - t1).count(),
            std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t2).count());
  // DocumentStore::GetAllDocIds (the NOT universe of boolean expressions) is the set of ids that were added (deleted ids
  // leave gaps in the range). As the index's live row it is ANDed into every query before the first funnel counter (a gap
  // holds no posting, so the bitmap forms are clean by construction): a NOT node's complement, total_candidates,
  // after_intersection and after_not count stored documents only, as ExecuteWithBooleanAst's all_docs does
  // (search_pipeline.cpp:1469, :1477).
  if (in.existing) {
    g.has_gaps = true;
    g.exists_bits.assign((v.n_docs + 63) / 64, 0);
    for (DocId doc : *in.existing) {
      const uint64_t slot = doc - v.first_doc_id;
      g.exists_bits[slot >> 6] |= 1ull << (slot & 63);
    }
    if (mgx_index_add_filter_bitmap(dev, in.existing->data(), in.existing->size(), &g.exists_bitmap) != MGX_OK ||
        mgx_index_set_live_bitmap(dev, g.exists_bitmap, MGX_LIVE_BITMAPS_CLEAN) != MGX_OK)
      return mgx_last_error();
  }
  if (in.primary_keys) {
    const std::string err = UploadPrimaryKeys(dev, *in.primary_keys, v.n_docs, [&](uint64_t slot) { return v.first_doc_id + static_cast<DocId>(slot); });
    if (!err.empty()) return err;
  }
  if (in.originals) {
    const std::string err = UploadOriginals(dev, *in.originals, v.n_docs, [&](uint64_t slot) { return v.first_doc_id + static_cast<DocId>(slot); },
                                            in.text_bytes, in.text_off, in.normalizer);
    if (!err.empty()) return err;
  }
  if (in.columns)
    for (const auto& c : *in.columns) {
      g.filter_columns.emplace_back();
      const std::string err = BuildFilterColumn(dev, v.n_docs, c.first, c.second, &g.filter_columns.back());
      if (!err.empty()) return err;
    }
  *out = std::move(g);
  return "";
}
}  // namespace

Index::~Index() {
  if (impl_->mut.build.valid()) impl_->mut.build.wait();  // (a delta build in flight reads this object's configuration)
  if (tl_last_index == this) tl_last_index = nullptr;
  const Index* me = this;
  g_last_finalized.compare_exchange_strong(me, nullptr);
}

std::unique_ptr<Index> Index::Adopt(mgx_columns* columns, mgx_index* device_index, int ngram_size,
                                    int kanji_ngram_size, bool cross_boundary_ngrams) {
  auto idx = std::make_unique<Index>(ngram_size, kanji_ngram_size, 0.0, cross_boundary_ngrams);
  Impl* im = idx->impl_.get();
  im->handles = std::make_shared<Impl::Handles>();
  im->handles->cols = im->cols = columns;
  im->handles->dev = im->dev = device_index;
  im->handles->owns = false;
  im->finalized = true;
  if (mgx_columns_view_get(columns, &im->view) != MGX_OK) im->last_error = mgx_last_error();
  g_last_finalized.store(idx.get());
  return idx;
}

std::unique_ptr<Index> Index::FromDump(const void* data, size_t len, const std::string& table, std::string* error,
                                       int device) {
  auto fail = [&](const std::string& msg) {
    if (error) *error = msg;
    return std::unique_ptr<Index>();
  };
  mgx_dump* dump = nullptr;
  if (mgx_dump_open(static_cast<const uint8_t*>(data), len, table.empty() ? nullptr : table.c_str(), &dump) != MGX_OK)
    return fail(mgx_last_error());
  std::unique_ptr<mgx_dump, void (*)(mgx_dump*)> guard(dump, mgx_dump_destroy);
  mgx_dump_view v{};
  mgx_dump_view_get(dump, &v);
  const mgx_mgix_info& info = v.index_info;
  auto idx = std::make_unique<Index>(info.ngram_size, info.kanji_ngram_size, 0.0, info.cross_boundary_ngrams != 0,
                                     info.normalize_nfkc != 0, std::string(info.normalize_width), info.normalize_lower != 0, device);
  Impl* im = idx->impl_.get();
  im->finalized = true;
  GenerationSpec spec;
  spec.device = device;
  if (mgx_dump_take_columns(dump, &spec.cols) != MGX_OK || spec.cols == nullptr) return fail(mgx_last_error());
  mgx_columns_view cv{};
  mgx_columns_view_get(spec.cols, &cv);
  if (cv.n_docs == 0) {
    mgx_columns_destroy(spec.cols);
    return fail("the dump's table holds no document");
  }
  if (v.has_texts) {
    spec.text_bytes = v.text_bytes;
    spec.text_off = v.text_off;
  }
  // DocumentStore::GetAllDocIds: the ids the store holds
  std::vector<DocId> existing;
  if (v.n_existing != v.n_docs) {
    for (uint64_t i = 0; i < v.n_docs; ++i)
      if (v.exists[i]) existing.push_back(v.first_doc_id + static_cast<DocId>(i));
    spec.existing = &existing;
  }
  NamedValues columns;
  for (uint32_t c = 0; c < v.n_filter_columns; ++c) {
    mgx_dump_filter_column fc{};
    if (mgx_dump_filter_column_get(dump, c, &fc) != MGX_OK) {
      mgx_columns_destroy(spec.cols);
      return fail(mgx_last_error());
    }
    std::vector<storage::FilterValue> vals(v.n_docs);
    for (uint64_t i = 0; i < v.n_docs; ++i) {
      if (fc.is_null[i]) continue;
      if (fc.value_type == 11)  // (strings come from the dump's byte pool, not from a dictionary)
        vals[i] = std::string(reinterpret_cast<const char*>(fc.string_bytes + fc.string_off[i]),
                              static_cast<size_t>(fc.string_off[i + 1] - fc.string_off[i]));
      else
        vals[i] = FilterValueFromBits(fc.value_type, fc.values[i], {});
    }
    columns.emplace_back(fc.name, std::move(vals));
  }
  spec.columns = &columns;
  // DocumentStore::LoadFromStream restores every document's primary key (document_store_persistence.cpp)
  std::map<DocId, std::string> keys;
  {
    const uint8_t* pk_bytes = nullptr;
    const uint64_t* pk_off = nullptr;
    if (mgx_dump_primary_keys_get(dump, &pk_bytes, &pk_off) != MGX_OK) {
      mgx_columns_destroy(spec.cols);
      return fail(mgx_last_error());
    }
    for (uint64_t i = 0; i < v.n_docs; ++i)
      if (v.exists[i])
        keys.emplace_hint(keys.end(), v.first_doc_id + static_cast<DocId>(i),
                          std::string(reinterpret_cast<const char*>(pk_bytes + pk_off[i]), static_cast<size_t>(pk_off[i + 1] - pk_off[i])));
  }
  spec.primary_keys = &keys;
  // ... and every document's original text where the store holds one (MGDS v3)
  std::map<DocId, std::string> originals;
  {
    const uint8_t* o_bytes = nullptr;
    const uint64_t* o_off = nullptr;
    if (mgx_dump_original_texts_get(dump, &o_bytes, &o_off) != MGX_OK) {
      mgx_columns_destroy(spec.cols);
      return fail(mgx_last_error());
    }
    for (uint64_t i = 0; i < v.n_docs; ++i)
      if (v.exists[i] && o_off[i + 1] > o_off[i])
        originals.emplace_hint(originals.end(), v.first_doc_id + static_cast<DocId>(i),
                               std::string(reinterpret_cast<const char*>(o_bytes + o_off[i]), static_cast<size_t>(o_off[i + 1] - o_off[i])));
  }
  spec.originals = &originals;
  const Index* self = idx.get();
  spec.normalizer = [self](std::string_view t) { return self->NormalizeText(t); };
  Impl::Generation gen;
  const std::string err = BuildGeneration(spec, &gen);
  if (!err.empty()) return fail(err);
  {
    std::lock_guard<std::mutex> lock(im->mu);
    im->Install(std::move(gen));
    im->primary_keys = std::move(keys);
    for (const auto& kv : originals)
      if (!mygram::utils::IsValidUtf8(kv.second)) im->invalid_originals.insert(kv.first);
    im->originals = std::move(originals);
  }
  g_last_finalized.store(idx.get());
  return idx;
}

namespace {
// Everything the first recorded change needs: which documents of the main index are live, its share of BM25Stats, and
// table-wide posting sizes the planner reads instead of the columns' own. Called with im->mu held, index finalised.
std::string EnsureMutable(Index::Impl* im) {
  Index::Impl::Mutable& m = im->mut;
  if (m.active) return "";
  if (!im->dev) return im->last_error.empty() ? "no device index" : im->last_error;
  if (!im->global_sizes.empty() || !im->absent_grams.empty() || im->fallback)
    return "a shard of a sharded table (SetGlobalStats) is static";
  const uint64_t n = im->view.n_docs;
  if (im->has_gaps) {
    m.main_live = im->exists_bits;
  } else {
    m.main_live.assign((n + 63) / 64, ~0ull);
    if (n & 63) m.main_live.back() = (1ull << (n & 63)) - 1;
  }
  m.applied_live = m.main_live;
  m.main_docs = im->view.bm25_doc_count;
  m.main_len = im->view.bm25_total_len;
  im->global_sizes.resize(im->view.n_grams);
  for (uint64_t g = 0; g < im->view.n_grams; ++g) im->global_sizes[g] = im->view.offsets[g + 1] - im->view.offsets[g];
  im->global_docs = m.main_docs;
  im->global_avgdl = m.main_docs ? static_cast<double>(m.main_len) / static_cast<double>(m.main_docs) : 0.0;
  // SORT by primary key: from now on a delta index may stand beside this one, and the two sides' runs are merged by key —
  // the main index must not answer such a query with a docid page (a compacted main index starts with the shortcut again)
  if (mgx_index_set_primary_key_shortcut(im->dev, 0) != MGX_OK) return mgx_last_error();
  m.active = true;
  return "";
}
}  // namespace

namespace {
// Both forms of AddDocument, in one critical section: the text and its filter values are recorded together or not at all.
// im->mu held: the document's original becomes `original` (nullptr: it has none).
void SetOriginalLocked(Index::Impl* im, DocId doc_id, const std::string_view* original) {
  im->originals.erase(doc_id);
  im->invalid_originals.erase(doc_id);
  if (!original) return;
  im->originals[doc_id] = std::string(*original);
  if (!mygram::utils::IsValidUtf8(*original)) im->invalid_originals.insert(doc_id);
}

bool AddDocumentLocked(const Index& index, DocId doc_id, std::string_view text, const storage::FilterMap* filters,
                       const std::string_view* primary_key = nullptr, const std::string_view* original = nullptr) {
  Index::Impl* im = index.impl();
  std::lock_guard<std::mutex> lock(im->mu);
  if (im->finalized) {  // index.cpp:39-74 on a built index: the document joins the delta
    const std::string err = EnsureMutable(im);
    if (!err.empty()) {
      im->last_error = "AddDocument: " + err;
      return false;
    }
    if (im->LiveInMain(doc_id) || im->mut.delta_docs.count(doc_id)) {
      im->last_error = "AddDocument: the document id is live (UpdateDocument changes a document's text)";
      return false;
    }
    im->mut.delta_docs[doc_id] = std::string(text);
    if (filters) im->mut.delta_filters[doc_id] = *filters;
    im->mut.Record(/*delta=*/true);
  } else {
    im->pending[doc_id] = std::string(text);
    if (filters) im->pending_filters[doc_id] = *filters;
  }
  if (primary_key) im->primary_keys[doc_id] = std::string(*primary_key);
  else im->primary_keys.erase(doc_id);  // (an id added again without a key has none)
  SetOriginalLocked(im, doc_id, original);
  return !GenerateHybridNgrams(text, index.GetNgramSize(), index.GetKanjiNgramSize(), index.GetCrossBoundaryNgrams()).empty();
}
}  // namespace

bool Index::AddDocument(DocId doc_id, std::string_view text) { return AddDocumentLocked(*this, doc_id, text, nullptr); }
bool Index::AddDocument(DocId doc_id, std::string_view text, const storage::FilterMap& filters) {
  return AddDocumentLocked(*this, doc_id, text, &filters);
}
bool Index::AddDocument(DocId doc_id, std::string_view text, const storage::FilterMap& filters, std::string_view primary_key) {
  return AddDocumentLocked(*this, doc_id, text, &filters, &primary_key);
}
bool Index::AddDocument(DocId doc_id, std::string_view text, const storage::FilterMap& filters,
                        std::optional<std::string_view> primary_key, std::string_view original_text) {
  return AddDocumentLocked(*this, doc_id, text, &filters, primary_key ? &*primary_key : nullptr, &original_text);
}
void Index::SetPrimaryKeyColumn(const std::string& name) {
  std::lock_guard<std::mutex> lock(impl_->mu);
  impl_->primary_key_column = name;
}

namespace {
// RemoveDocument's bookkeeping (index.cpp:148-197: every distinct n-gram of the text loses the posting). im->mu held.
void RemoveLocked(const Index& index, Index::Impl* im, DocId doc_id, std::string_view text) {
  Index::Impl::Mutable& m = im->mut;
  const auto it = m.delta_docs.find(doc_id);
  if (it != m.delta_docs.end()) {
    m.delta_docs.erase(it);
    m.delta_filters.erase(doc_id);
    m.Record(/*delta=*/true);
    return;
  }
  if (!im->LiveInMain(doc_id)) return;  // not a document of the table
  const uint64_t slot = doc_id - im->view.first_doc_id;
  m.main_live[slot >> 6] &= ~(1ull << (slot & 63));
  m.pending_clear.push_back(doc_id);
  auto grams = GenerateHybridNgrams(text, index.GetNgramSize(), index.GetKanjiNgramSize(), index.GetCrossBoundaryNgrams());
  DeduplicateSorted(grams);
  for (const auto& g : grams) {
    uint32_t id = 0;
    if (im->Lookup(g, &id)) {
      m.pending_dead_grams.push_back(id);
      m.pending_dead_docs.push_back(doc_id);
    }
  }
  const uint32_t dl = im->view.doc_len[slot];
  if (dl > 0) {  // BM25Stats::RemoveDocument (binlog_event_processor.cpp:140-142)
    m.main_docs -= 1;
    m.main_len -= dl;
  }
  m.removed += 1;
  m.Record(/*delta=*/false);
}
}  // namespace

void Index::RemoveDocument(DocId doc_id, std::string_view text) {
  Finalize();
  std::lock_guard<std::mutex> lock(impl_->mu);
  const std::string err = EnsureMutable(impl_.get());
  if (!err.empty()) {
    impl_->last_error = "RemoveDocument: " + err;
    return;
  }
  RemoveLocked(*this, impl_.get(), doc_id, text);
  impl_->primary_keys.erase(doc_id);  // (UpdateDocument and UpdateFilters go through RemoveLocked and keep the key)
  SetOriginalLocked(impl_.get(), doc_id, nullptr);
}

void Index::UpdateDocument(DocId doc_id, std::string_view old_text, std::string_view new_text) {
  Finalize();
  FlushPendingFilterColumns();
  std::lock_guard<std::mutex> lock(impl_->mu);
  Impl* im = impl_.get();
  const std::string err = EnsureMutable(im);
  if (!err.empty()) {
    im->last_error = "UpdateDocument: " + err;
    return;
  }
  // the document keeps its filter values (the reference changes them through DocumentStore::UpdateDocument, a separate
  // call): a delta document has them on the host, a document of the main index has them in the device columns
  storage::FilterMap keep;
  const auto df = im->mut.delta_filters.find(doc_id);
  if (df != im->mut.delta_filters.end()) {
    keep = df->second;
  } else if (im->LiveInMain(doc_id)) {
    std::lock_guard<std::mutex> fl(im->filter_mu);
    for (const auto& col : im->filter_columns) {
      uint64_t w = 0;
      int nul = 1;
      if (mgx_index_filter_column_read(im->dev, col.device_id, doc_id, &w, &nul, nullptr) != MGX_OK) {
        im->last_error = mgx_last_error();
        continue;
      }
      if (!nul && col.type != 0) keep[col.name] = FilterValueFromBits(col.type, w, col.dict);
    }
  }
  RemoveLocked(*this, im, doc_id, old_text);
  im->mut.delta_docs[doc_id] = std::string(new_text);
  if (!keep.empty()) im->mut.delta_filters[doc_id] = std::move(keep);
  SetOriginalLocked(im, doc_id, nullptr);  // (the old original no longer belongs to the new text)
  im->mut.Record(/*delta=*/true);
}

namespace {
void UpdateDocumentWithFilters(const Index& index, DocId doc_id, std::string_view old_text, std::string_view new_text,
                               const storage::FilterMap& filters, const std::string_view* original) {
  index.Finalize();
  Index::Impl* im = index.impl();
  std::lock_guard<std::mutex> lock(im->mu);
  const std::string err = EnsureMutable(im);
  if (!err.empty()) {
    im->last_error = "UpdateDocument: " + err;
    return;
  }
  RemoveLocked(index, im, doc_id, old_text);
  im->mut.delta_docs[doc_id] = std::string(new_text);
  im->mut.delta_filters[doc_id] = filters;
  SetOriginalLocked(im, doc_id, original);  // (none given: the old one no longer belongs to the new text)
  im->mut.Record(/*delta=*/true);
}
}  // namespace

void Index::UpdateDocument(DocId doc_id, std::string_view old_text, std::string_view new_text,
                           const storage::FilterMap& filters) {
  UpdateDocumentWithFilters(*this, doc_id, old_text, new_text, filters, nullptr);
}
void Index::UpdateDocument(DocId doc_id, std::string_view old_text, std::string_view new_text,
                           const storage::FilterMap& filters, std::string_view original_text) {
  UpdateDocumentWithFilters(*this, doc_id, old_text, new_text, filters, &original_text);
}

bool Index::UpdateFilters(DocId doc_id, const storage::FilterMap& filters) {
  Finalize();
  std::lock_guard<std::mutex> lock(impl_->mu);
  Impl* im = impl_.get();
  const std::string err = EnsureMutable(im);
  if (!err.empty()) {
    im->last_error = "UpdateFilters: " + err;
    return false;
  }
  if (im->mut.delta_docs.count(doc_id)) {
    im->mut.delta_filters[doc_id] = filters;
    im->mut.Record(/*delta=*/true);
    return true;
  }
  if (!im->LiveInMain(doc_id)) {
    im->last_error = "UpdateFilters: not a live document";
    return false;
  }
  uint64_t len = 0;
  if (mgx_index_read_text(im->dev, doc_id, nullptr, 0, &len) != MGX_OK) {
    im->last_error = std::string("UpdateFilters: ") + mgx_last_error();
    return false;
  }
  std::string text(len, '\0');
  if (len && mgx_index_read_text(im->dev, doc_id, reinterpret_cast<uint8_t*>(text.data()), len, &len) != MGX_OK) {
    im->last_error = std::string("UpdateFilters: ") + mgx_last_error();
    return false;
  }
  RemoveLocked(*this, im, doc_id, text);
  im->mut.delta_docs[doc_id] = std::move(text);
  im->mut.delta_filters[doc_id] = filters;
  im->mut.Record(/*delta=*/true);
  return true;
}

Index::MutationStats Index::GetMutationStats() const {
  std::lock_guard<std::mutex> lock(impl_->mu);
  MutationStats st;
  const auto& m = impl_->mut;
  st.main_documents = m.active ? m.main_docs : impl_->view.bm25_doc_count;
  st.delta_documents = m.delta_docs.size();
  st.removed_from_main = m.removed;
  st.epoch = m.epoch;
  return st;
}

// The recorded changes reach the device: live row, delta index, table-wide statistics. The caller guarantees that no
// batch of this Index is being planned, compiled or run by another thread (header note).
namespace {
using Snapshot = Index::Impl::Snapshot;
using BuiltDelta = Index::Impl::BuiltDelta;

Snapshot TakeSnapshot(const Index::Impl::Mutable& m) {  // im->mu held
  Snapshot snap;
  snap.recorded = m.recorded;
  snap.n_clear = m.pending_clear.size();
  snap.n_dead = m.pending_dead_grams.size();
  snap.delta_changed = m.delta_recorded > m.applied;
  snap.main_docs = m.main_docs;
  snap.main_len = m.main_len;
  return snap;
}

std::vector<std::string> ColumnNames(const Index::Impl* im) {
  std::lock_guard<std::mutex> fl(im->filter_mu);
  std::vector<std::string> names;
  for (const auto& c : im->filter_columns) names.push_back(c.name);
  return names;
}

// The delta index over `docs`: column build, device index, doc map, filter columns. Touches nothing of `self` that changes
// (its configuration only), so it runs with or without the index lock — in a builder thread when changes may wait.
// The primary keys of the delta's documents: a copy, for a build that runs without the index lock. im->mu held.
std::map<DocId, std::string> DeltaKeys(const Index::Impl* im) {
  std::map<DocId, std::string> keys;
  if (im->primary_keys.empty()) return keys;
  for (const auto& kv : im->mut.delta_docs) {
    const auto it = im->primary_keys.find(kv.first);
    if (it != im->primary_keys.end()) keys.emplace_hint(keys.end(), *it);
  }
  return keys;
}

// Likewise the originals of the delta's documents. im->mu held.
std::map<DocId, std::string> DeltaOriginals(const Index::Impl* im) {
  std::map<DocId, std::string> out;
  if (im->originals.empty()) return out;
  for (const auto& kv : im->mut.delta_docs) {
    const auto it = im->originals.find(kv.first);
    if (it != im->originals.end()) out.emplace_hint(out.end(), *it);
  }
  return out;
}

BuiltDelta BuildDelta(const Index& self, const std::map<DocId, std::string>& docs,
                      const std::map<DocId, storage::FilterMap>& filters, std::vector<std::string> column_names,
                      const std::map<DocId, std::string>& primary_keys, const std::map<DocId, std::string>& originals) {
  BuiltDelta out;
  out.rebuilt = true;
  if (docs.empty()) return out;
  Index::Impl* im = self.impl();
  auto nd = std::make_shared<Index>(self.GetNgramSize(), im->query_kanji, im->dense_threshold, self.GetCrossBoundaryNgrams(),
                                    self.GetNormalizeNfkc(), self.GetNormalizeWidth(), self.GetNormalizeLower(), im->device);
  nd->impl()->internal = true;
  nd->impl()->build_mode = im->build_mode.load();
  nd->impl()->built_sink = im->built_sink;
  std::vector<DocId> ids;
  ids.reserve(docs.size());
  DocId local = 1;
  for (const auto& kv : docs) {  // (ascending table id -> ascending local id: rank order and ties are kept)
    nd->AddDocument(local, kv.second);
    const auto orig = originals.find(kv.first);  // (by local id: the delta's own generation uploads them)
    if (orig != originals.end()) nd->impl()->originals.emplace(local, orig->second);
    ++local;
    ids.push_back(kv.first);
  }
  const std::string err = nd->Finalize();
  if (!err.empty() || !nd->impl()->dev) {
    out.error = "the delta index failed to build: " + err;
    return out;
  }
  if (mgx_index_set_doc_map(nd->impl()->dev, ids.data(), ids.size()) != MGX_OK) {
    out.error = mgx_last_error();
    return out;
  }
  nd->impl()->doc_map_ids = ids;
  out.error = UploadPrimaryKeys(nd->impl()->dev, primary_keys, ids.size(), [&](uint64_t slot) { return ids[slot]; });  // (after the doc map)
  if (!out.error.empty()) return out;
  const NamedValues columns = ValuesByName(filters, std::move(column_names), ids.size(), [&](DocId doc) {
    return static_cast<uint64_t>(std::lower_bound(ids.begin(), ids.end(), doc) - ids.begin());  // (every key is a delta document)
  });
  for (const auto& c : columns) {
    out.error = nd->AddFilterColumn(c.first, c.second);
    if (!out.error.empty()) return out;
  }
  nd->impl()->fallback = im;
  out.delta = std::move(nd);
  out.ids = std::make_shared<const std::vector<DocId>>(std::move(ids));
  return out;
}

struct Laps {  // MGX_TRACE_HOST: what each part of an application took
  std::chrono::steady_clock::time_point t_prev = std::chrono::steady_clock::now();
  void operator()(const char* what) {
    static const bool kTrace = std::getenv("MGX_TRACE_HOST") != nullptr;
    if (!kTrace) return;
    const auto t = std::chrono::steady_clock::now();
    fprintf(stderr, "[shim] ApplyMutations %s: %.2f ms\n", what, std::chrono::duration<double, std::milli>(t - t_prev).count());
    t_prev = t;
  }
};

void ClearLive(std::vector<uint64_t>* live, DocId first, const std::vector<DocId>& docs, size_t n) {
  for (size_t i = 0; i < n; ++i) {
    const uint64_t slot = docs[i] - first;
    (*live)[slot >> 6] &= ~(1ull << (slot & 63));
  }
}

// Every device call of an application, and nothing else: the host's picture of the table changes in CommitMutations, which
// runs only after this returned "". What the calls do to a device that has seen part of them already is nothing (they
// clear bits that are cleared), so after a failure the same snapshot, or a later one, is simply installed again.
// im->mu held; no batch of this Index is planned, compiled or in flight (the callers' contract).
std::string InstallMutations(Index::Impl* im, const Snapshot& snap, const BuiltDelta& built, Laps& lap) {
  Index::Impl::Mutable& m = im->mut;
  auto fail = [&](const std::string& msg) {
    im->last_error = "ApplyMutations: " + msg;
    return im->last_error;
  };
  if (!built.error.empty()) return fail(built.error);
  if (mgx_index_synchronize(im->dev) != MGX_OK) return fail(mgx_last_error());
  // ---- the dead documents' postings leave the bitmap form of their dense grams (a query over bitmap-form grams then
  // needs no live-row operand), then their live bits go --------------------------------------------------------------
  if (snap.n_dead > 0 &&
      mgx_index_clear_postings(im->dev, m.pending_dead_docs.data(), m.pending_dead_grams.data(), snap.n_dead) != MGX_OK)
    return fail(mgx_last_error());
  // ---- the live row of the main index ---------------------------------------------------------------------------------
  if (!m.have_live) {
    std::vector<uint64_t> bits = m.applied_live;
    ClearLive(&bits, im->view.first_doc_id, m.pending_clear, snap.n_clear);
    std::vector<DocId> live;
    live.reserve(im->view.n_docs);
    for (uint64_t slot = 0; slot < im->view.n_docs; ++slot)
      if ((bits[slot >> 6] >> (slot & 63)) & 1) live.push_back(im->view.first_doc_id + static_cast<DocId>(slot));
    if (mgx_index_add_filter_bitmap(im->dev, live.data(), live.size(), &m.live_bitmap) != MGX_OK) return fail(mgx_last_error());
    m.have_live = true;  // (a fact about the device, not about the table: a retry updates this row, it makes no second one)
  } else if (snap.n_clear > 0) {
    if (mgx_index_update_filter_bitmap(im->dev, m.live_bitmap, nullptr, 0, m.pending_clear.data(), snap.n_clear) != MGX_OK)
      return fail(mgx_last_error());
  }
  if (mgx_index_set_live_bitmap(im->dev, m.live_bitmap, MGX_LIVE_BITMAPS_CLEAN) != MGX_OK) return fail(mgx_last_error());
  lap("sync + live row + cleaned bitmaps");
  // ---- the statistics tables of both indexes go: the next batch computes them from what the commit publishes -------------
  const Index* delta = built.rebuilt ? built.delta.get() : m.delta.get();
  if (delta && mgx_index_invalidate_statistics(delta->impl()->dev) != MGX_OK) return fail(mgx_last_error());
  if (mgx_index_invalidate_statistics(im->dev) != MGX_OK) return fail(mgx_last_error());
  return "";
}

// The one place recorded changes are marked applied: the covered prefix of the pending lists goes (what a writer appended
// behind it while a background build ran stays), the delta's handles and the table-wide statistics of both indexes are
// published. Host work only, nothing here fails. im->mu held, InstallMutations(snap, built) returned "".
void CommitMutations(Index::Impl* im, const Snapshot& snap, BuiltDelta&& built, Laps& lap) {
  Index::Impl::Mutable& m = im->mut;
  ClearLive(&m.applied_live, im->view.first_doc_id, m.pending_clear, snap.n_clear);
  im->has_gaps = false;  // (the live row is also the NOT universe: ids never added are not in it)
  // ---- posting sizes: the main index's live postings, then the delta's on top -------------------------------------------
  for (const auto& c : m.delta_contrib) im->global_sizes[c.first] -= c.second;
  m.delta_contrib.clear();
  for (size_t i = 0; i < snap.n_dead; ++i)
    if (im->global_sizes[m.pending_dead_grams[i]] > 0) im->global_sizes[m.pending_dead_grams[i]] -= 1;
  m.pending_clear.erase(m.pending_clear.begin(), m.pending_clear.begin() + static_cast<std::ptrdiff_t>(snap.n_clear));
  m.pending_dead_docs.erase(m.pending_dead_docs.begin(), m.pending_dead_docs.begin() + static_cast<std::ptrdiff_t>(snap.n_dead));
  m.pending_dead_grams.erase(m.pending_dead_grams.begin(), m.pending_dead_grams.begin() + static_cast<std::ptrdiff_t>(snap.n_dead));
  // ---- the delta index ------------------------------------------------------------------------------------------------
  if (built.rebuilt) {
    m.delta = std::move(built.delta);
    m.delta_ids = std::move(built.ids);
  }
  lap("delta index handles");
  // ---- table-wide statistics in both ------------------------------------------------------------------------------------
  uint64_t n_docs = snap.main_docs, total_len = snap.main_len;
  im->absent_grams.clear();
  std::vector<uint64_t> delta_sizes;
  if (m.delta) {
    const mgx_columns_view& dv = m.delta->impl()->view;
    n_docs += dv.bm25_doc_count;
    total_len += dv.bm25_total_len;
    delta_sizes.resize(dv.n_grams);
    for (uint64_t g = 0; g < dv.n_grams; ++g) {
      const std::string_view key(reinterpret_cast<const char*>(dv.key_bytes) + dv.key_off[g], dv.key_off[g + 1] - dv.key_off[g]);
      const uint64_t sz = dv.offsets[g + 1] - dv.offsets[g];
      uint32_t mid = 0;
      if (im->Lookup(key, &mid)) {
        im->global_sizes[mid] += sz;
        m.delta_contrib.emplace_back(mid, sz);
        delta_sizes[g] = im->global_sizes[mid];
      } else {
        im->absent_grams.emplace(std::string(key), sz);
        delta_sizes[g] = sz;
      }
    }
  }
  im->global_docs = n_docs;
  im->global_avgdl = n_docs ? static_cast<double>(total_len) / static_cast<double>(n_docs) : 0.0;
  if (m.delta) {
    Index::Impl* dm = m.delta->impl();
    dm->global_sizes = std::move(delta_sizes);
    dm->global_docs = im->global_docs;
    dm->global_avgdl = im->global_avgdl;
  }
  lap("statistics");
  m.applied = snap.recorded;
  m.retry = false;
  m.epoch += 1;
  m.last_apply = std::chrono::steady_clock::now();
}

// What an entry point would do about the recorded changes now (im->mu held): nothing; kick a background build of them
// (nothing changes on the device yet); or install — something changes on the device in this call, so nothing of the
// caller may be being planned or compiled meanwhile. With no staleness bound, the first time, when forced and after a
// failed application, everything recorded so far is applied by the call itself.
enum class MutationStep { kNothing, kKick, kInstall };
MutationStep NextMutationStep(const Index::Impl::Mutable& m, bool force) {
  const bool immediate = force || m.retry || m.staleness.count() == 0 || m.epoch == 0;
  if (m.build.valid()) {  // a build is under way: its result is installed once it is there (a forced call waits for it)
    const bool ready = m.build.wait_for(std::chrono::seconds(0)) == std::future_status::ready;
    return immediate || ready ? MutationStep::kInstall : MutationStep::kNothing;
  }
  if (m.recorded == m.applied) return MutationStep::kNothing;
  if (immediate) return MutationStep::kInstall;
  return std::chrono::steady_clock::now() - m.last_apply >= m.staleness ? MutationStep::kKick : MutationStep::kNothing;
}

// With no staleness bound (and always the first time): snapshot, build, install, commit — in this call, under the lock (a
// writer thread recording a change meanwhile waits, and is not marked applied). With a bound: the snapshot's delta is
// built by a thread while queries keep running on the old state, and installed by the first entry point that finds it
// ready — the stall a steady writer causes is the few milliseconds of the installation, not the delta build. im->mu held.
std::string ApplyLocked(const Index& self, bool force) {
  Index::Impl* im = self.impl();
  Index::Impl::Mutable& m = im->mut;
  for (;;) {
    switch (NextMutationStep(m, force)) {
      case MutationStep::kNothing: return "";
      case MutationStep::kKick: {
        m.build_snapshot = TakeSnapshot(m);
        const bool changed = m.build_snapshot.delta_changed;  // (false: removals only, nothing to copy or build)
        m.build = std::async(std::launch::async, [&self, changed, docs = changed ? m.delta_docs : decltype(m.delta_docs)(),
                                                  filters = changed ? m.delta_filters : decltype(m.delta_filters)(),
                                                  names = ColumnNames(im),
                                                  keys = changed ? DeltaKeys(im) : std::map<DocId, std::string>(),
                                                  originals = changed ? DeltaOriginals(im) : std::map<DocId, std::string>()] {
          pthread_setname_np(pthread_self(), "mgx-delta");
          return changed ? BuildDelta(self, docs, filters, names, keys, originals) : BuiltDelta{};
        });
        return "";
      }
      case MutationStep::kInstall: {
        Snapshot snap;
        BuiltDelta built;
        if (m.build.valid()) {
          snap = m.build_snapshot;
          built = m.build.get();
        } else {
          snap = TakeSnapshot(m);
          if (snap.delta_changed) built = BuildDelta(self, m.delta_docs, m.delta_filters, ColumnNames(im), DeltaKeys(im), DeltaOriginals(im));
        }
        Laps lap;
        const std::string err = InstallMutations(im, snap, built, lap);
        if (!err.empty()) {
          m.retry = true;
          return err;
        }
        CommitMutations(im, snap, std::move(built), lap);
      }
    }
  }
}
}  // namespace

void Index::SetDeviceBuild(bool on) { impl_->build_mode = on ? kDeviceColumns : kHost; }
void Index::SetBuildMode(BuildMode mode) { impl_->build_mode = mode; }
Index::BuildCounts Index::BuildCounters() const {
  return {impl_->built[kHost].load(), impl_->built[kDeviceColumns].load(), impl_->built[kDeviceResident].load()};
}

void Index::SetMutationStaleness(std::chrono::microseconds max_staleness) {
  std::lock_guard<std::mutex> lock(impl_->mu);
  impl_->mut.staleness = max_staleness;
}

std::string Index::ApplyMutations(bool force) const {
  std::lock_guard<std::mutex> lock(impl_->mu);
  return ApplyLocked(*this, force);
}

// The main index rebuilt from the table's current documents: live documents of the old main index (their texts come back
// from the device, where BM25 keeps them) + the delta's. The index lock is held from the forced application to the swap:
// the new generation, filter columns included, is built off to the side and published in one step, so a writer or another
// thread's ApplyMutations sees the table before or after the compaction, and a failure leaves it as it was, still serving.
// Batch objects an executor compiled on the old device index stay valid until that executor lets go of them
// (Impl::Handles).
std::string Index::Compact() const {
  Finalize();
  FlushPendingFilterColumns();
  Impl* im = impl_.get();
  std::lock_guard<std::mutex> lock(im->mu);
  Impl::Mutable& m = im->mut;
  if (!m.active) return "";  // the table never changed
  {
    const std::string e = ApplyLocked(*this, /*force=*/true);
    if (!e.empty()) return e;
  }
  auto fail = [&](const std::string& msg) {
    im->last_error = "Compact: " + msg;
    return im->last_error;
  };
  const uint64_t n_old = im->view.n_docs;
  uint64_t total = 0;
  if (mgx_index_copy_text(im->dev, nullptr, 0, nullptr, &total) != MGX_OK) return fail(mgx_last_error());
  std::vector<uint8_t> old_bytes(total + 16);
  std::vector<uint64_t> old_off(n_old + 1);
  if (mgx_index_copy_text(im->dev, old_bytes.data(), total, old_off.data(), &total) != MGX_OK) return fail(mgx_last_error());
  const DocId old_first = im->view.first_doc_id;
  DocId first = old_first, last = old_first + static_cast<DocId>(n_old) - 1;
  if (!m.delta_docs.empty()) {
    first = std::min(first, m.delta_docs.begin()->first);
    last = std::max(last, m.delta_docs.rbegin()->first);
  }
  const uint64_t n2 = static_cast<uint64_t>(last) - first + 1;
  std::vector<uint8_t> bytes;
  bytes.reserve(total + 1024);
  std::vector<uint64_t> off(n2 + 1, 0);
  std::vector<DocId> existing;
  {
    auto dit = m.delta_docs.begin();
    for (uint64_t i = 0; i < n2; ++i) {
      const DocId doc = first + static_cast<DocId>(i);
      while (dit != m.delta_docs.end() && dit->first < doc) ++dit;
      if (dit != m.delta_docs.end() && dit->first == doc) {
        bytes.insert(bytes.end(), dit->second.begin(), dit->second.end());
        existing.push_back(doc);
      } else if (im->LiveInMain(doc)) {
        const uint64_t slot = doc - old_first;
        bytes.insert(bytes.end(), old_bytes.begin() + static_cast<std::ptrdiff_t>(old_off[slot]),
                     old_bytes.begin() + static_cast<std::ptrdiff_t>(old_off[slot + 1]));
        existing.push_back(doc);
      }
      off[i + 1] = bytes.size();
    }
  }
  bytes.resize(bytes.size() + 16);
  std::vector<uint8_t>().swap(old_bytes);
  // ---- filter columns of the new generation: a document of the delta has the values recorded with it, a live document of
  // the old main index keeps its value (the old generation's columns, by doc slot) ------------------------------------------
  std::vector<Impl::FilterColumn> old_cols;
  {
    std::lock_guard<std::mutex> fl(im->filter_mu);
    old_cols = im->filter_columns;
  }
  std::vector<std::string> names;
  for (const auto& c : old_cols) names.push_back(c.name);
  NamedValues columns = ValuesByName(m.delta_filters, std::move(names), n2, [&](DocId doc) { return static_cast<uint64_t>(doc - first); });
  std::vector<uint64_t> old_values(n_old);
  std::vector<uint8_t> old_nul(n_old);
  for (size_t c = 0; c < old_cols.size(); ++c) {  // (columns[c] is old_cols[c]'s: the old names come first)
    const Impl::FilterColumn& oc = old_cols[c];
    if (oc.type == 0) continue;
    if (mgx_index_filter_column_export(im->dev, oc.device_id, old_values.data(), old_nul.data(), nullptr) != MGX_OK)
      return fail(mgx_last_error());
    for (uint64_t slot = 0; slot < n_old; ++slot) {
      if (!((m.main_live[slot >> 6] >> (slot & 63)) & 1) || old_nul[slot]) continue;
      columns[c].second[static_cast<uint64_t>(old_first - first) + slot] = FilterValueFromBits(oc.type, old_values[slot], oc.dict);
    }
  }
  // ---- the new generation ----------------------------------------------------------------------------------------------
  GenerationSpec spec{im->device, im->dense_threshold, ngram_size_, kanji_ngram_size_, cross_boundary_, nullptr,
                      bytes.data(), off.data(),    first,       n2};
  spec.build_mode = im->build_mode.load();
  spec.built = im->built_sink;
  if (existing.size() != n2) spec.existing = &existing;
  spec.columns = &columns;
  spec.primary_keys = &im->primary_keys;  // (removed documents' keys are gone from it: a gap of the new range has none)
  spec.originals = &im->originals;        // (likewise)
  spec.normalizer = [this](std::string_view t) { return NormalizeText(t); };
  Impl::Generation gen;
  const std::string err = BuildGeneration(spec, &gen);
  if (!err.empty()) return fail(err);
  // ---- swap ----------------------------------------------------------------------------------------------------------------
  const std::shared_ptr<Impl::Handles> old_gen = im->handles;  // (let go at the end of this call, or by the last executor slot)
  im->Install(std::move(gen));
  im->global_sizes.clear();
  im->absent_grams.clear();
  im->global_docs = 0;
  im->global_avgdl = 0.0;
  const uint64_t epoch = m.epoch + 1;
  const auto staleness = m.staleness;
  m = Impl::Mutable{};  // (no build is in flight: the forced application above took it)
  m.epoch = epoch;
  m.staleness = staleness;
  return "";
}

uint64_t Index::DeviceMemoryBytes() const {
  uint64_t n = 0;
  if (impl_->dev == nullptr || mgx_index_memory_bytes(impl_->dev, &n) != MGX_OK) return 0;
  return n;
}

std::string Index::AddFilterColumn(const std::string& name, const std::vector<storage::FilterValue>& values) const {
  Finalize();
  Impl* im = impl_.get();
  std::lock_guard<std::mutex> lock(im->mu);  // (then filter_mu: the order UpdateDocument and Compact use)
  if (!im->dev) return im->last_error.empty() ? "AddFilterColumn: no device index" : im->last_error;
  Impl::FilterColumn col;
  const std::string err = BuildFilterColumn(im->dev, im->view.n_docs, name, values, &col);
  if (!err.empty()) return err;
  std::lock_guard<std::mutex> fl(im->filter_mu);
  for (auto& c : im->filter_columns)
    if (c.name == name) {
      c = std::move(col);  // (replaced: cached conditions of the old column are dropped)
      im->condition_cache.clear();
      return "";
    }
  im->filter_columns.push_back(std::move(col));
  return "";
}

void Index::AddDocumentBatch(const std::vector<DocumentItem>& documents) {
  for (const auto& d : documents) {
    if (d.original_text)
      AddDocument(d.doc_id, d.text, {}, d.primary_key ? std::optional<std::string_view>(*d.primary_key) : std::nullopt, *d.original_text);
    else if (d.primary_key) AddDocument(d.doc_id, d.text, {}, *d.primary_key);
    else AddDocument(d.doc_id, d.text);
  }
}

std::string Index::Finalize() const {
  if (!impl_->internal) tl_last_index = this;  // (every search / scoring entry point passes through here)
  std::lock_guard<std::mutex> lock(impl_->mu);
  if (impl_->finalized) return impl_->last_error;
  impl_->finalized = true;
  if (!impl_->internal) g_last_finalized.store(this);
  // dense id range [first, last]; ids never added are documents without text
  const DocId first = impl_->pending.empty() ? 1 : impl_->pending.begin()->first;
  const DocId last = impl_->pending.empty() ? 1 : impl_->pending.rbegin()->first;
  const uint64_t n = static_cast<uint64_t>(last) - first + 1;
  std::vector<uint8_t> bytes;
  std::vector<uint64_t> off(n + 1, 0);
  std::vector<DocId> existing;
  {
    auto it = impl_->pending.begin();
    for (uint64_t i = 0; i < n; ++i) {
      if (it != impl_->pending.end() && it->first == first + i) {
        bytes.insert(bytes.end(), it->second.begin(), it->second.end());
        existing.push_back(it->first);
        ++it;
      }
      off[i + 1] = bytes.size();
    }
  }
  bytes.resize(bytes.size() + 16);
  impl_->pending.clear();
  GenerationSpec spec{impl_->device, impl_->dense_threshold, ngram_size_, kanji_ngram_size_, cross_boundary_, nullptr,
                      bytes.data(),  off.data(),             first,       n};
  spec.build_mode = impl_->build_mode.load();
  spec.built = impl_->built_sink;
  if (existing.size() != n && !existing.empty()) spec.existing = &existing;
  spec.primary_keys = &impl_->primary_keys;
  spec.originals = &impl_->originals;
  spec.normalizer = [this](std::string_view t) { return NormalizeText(t); };
  Impl::Generation gen;
  impl_->last_error = BuildGeneration(spec, &gen);
  if (!impl_->last_error.empty()) return impl_->last_error;
  impl_->Install(std::move(gen));
  pending_columns_ready_ = !impl_->pending_filters.empty();
  return "";
}

// The filter values recorded by AddDocument(doc, text, filters) become device columns (outside impl_->mu: AddFilterColumn
// takes it).
void Index::FlushPendingFilterColumns() const {
  std::map<DocId, storage::FilterMap> pending;
  DocId first = 0;
  uint64_t n = 0;
  {
    std::lock_guard<std::mutex> lock(impl_->mu);
    if (!pending_columns_ready_) return;
    pending_columns_ready_ = false;
    pending.swap(impl_->pending_filters);
    first = impl_->view.first_doc_id;
    n = impl_->view.n_docs;
  }
  for (const auto& c : ValuesByName(pending, {}, n, [&](DocId doc) { return doc >= first ? uint64_t{doc} - first : n; })) {
    const std::string err = AddFilterColumn(c.first, c.second);
    if (!err.empty()) impl_->last_error = err;
  }
}

const std::string& Index::LastError() const { return impl_->last_error; }

void Index::SetNormalization(bool nfkc, const std::string& width, bool lower) {
  normalize_nfkc_ = nfkc;
  normalize_width_ = width;
  normalize_lower_ = lower;
}

uint64_t Index::PostingSize(std::string_view term) const {  // index.cpp:580-584
  Finalize();
  bool mutable_table = false;
  {
    std::lock_guard<std::mutex> lock(impl_->mu);
    mutable_table = impl_->mut.active;
  }
  // (the live postings of both indexes: what Count() is in the reference; a failed application: 0, LastError() says why)
  if (mutable_table && !ApplyMutations().empty()) return 0;
  uint32_t id = 0;
  uint64_t size = 0;
  return impl_->Resolve(term, &id, &size) ? size : 0;
}
uint64_t Index::EstimatePostingSize(std::string_view term) const { return PostingSize(term); }  // index.cpp:756-759

void Index::SetAbsentGrams(std::unordered_map<std::string, uint64_t> grams) { impl_->absent_grams = std::move(grams); }

std::string Index::SetGlobalStats(uint64_t total_docs, double avg_doc_length, std::vector<uint64_t> global_posting_sizes) {
  Finalize();
  if (global_posting_sizes.size() != impl_->view.n_grams) return "SetGlobalStats: one size per gram of this shard";
  impl_->global_sizes = std::move(global_posting_sizes);
  impl_->global_docs = total_docs;
  impl_->global_avgdl = avg_doc_length;
  return "";
}

uint64_t Index::Bm25DocCount() const {
  Finalize();
  return impl_->global_sizes.empty() ? impl_->view.bm25_doc_count : impl_->global_docs;
}
double Index::Bm25AvgDocLength() const {  // server_types.h:182-187
  Finalize();
  if (!impl_->global_sizes.empty()) return impl_->global_avgdl;
  return impl_->view.bm25_doc_count
             ? static_cast<double>(impl_->view.bm25_total_len) / static_cast<double>(impl_->view.bm25_doc_count)
             : 0.0;
}

Expected<uint32_t, Error> Index::AddFilterBitmap(const std::vector<DocId>& docs) const {
  Finalize();
  if (!impl_->dev) return MakeUnexpected(MakeError(ErrorCode::kInternalError, impl_->last_error));
  uint32_t id = 0;
  const int rc = mgx_index_add_filter_bitmap(impl_->dev, docs.data(), docs.size(), &id);
  if (rc != MGX_OK) return MakeUnexpected(MakeError(static_cast<ErrorCode>(rc), mgx_last_error()));
  return id;
}

// ---- single operators on a mutable table ---------------------------------------------------------------------------------
// The operators below answer from the column arrays of ONE device index. A table with recorded changes answers with the
// main index's result minus its dead documents plus the delta index's result under table ids — both ascending and
// disjoint, so one std::merge; the set semantics are per document, so evaluating each index on its own is exact.
namespace {
thread_local bool tl_raw_operators = false;  // inside OverBoth: the operators answer from this index's arrays alone
struct RawScope {
  bool prev;
  RawScope() : prev(tl_raw_operators) { tl_raw_operators = true; }
  ~RawScope() { tl_raw_operators = prev; }
};

bool IsMutable(const Index& index) {
  if (tl_raw_operators) return false;
  Index::Impl* im = index.impl();
  std::lock_guard<std::mutex> lock(im->mu);
  return im->mut.active;
}

struct DeltaView {
  std::shared_ptr<Index> delta;
  std::shared_ptr<const std::vector<DocId>> ids;
};
DeltaView ViewOfDelta(const Index& index) {
  Index::Impl* im = index.impl();
  std::lock_guard<std::mutex> lock(im->mu);
  return DeltaView{im->mut.delta, im->mut.delta_ids};
}

// op(index) -> ascending doc ids of that one index
template <typename Op>
std::vector<DocId> OverBoth(const Index& index, Op op) {
  const std::string err = index.ApplyMutations();
  if (!err.empty()) {
    SetDeviceError(err);
    return {};
  }
  RawScope raw;
  std::vector<DocId> a = op(index);
  if (!tl_device_error.empty()) return {};
  Index::Impl* im = index.impl();
  {
    std::lock_guard<std::mutex> lock(im->mu);
    a.erase(std::remove_if(a.begin(), a.end(), [&](DocId d) { return !im->LiveApplied(d); }), a.end());
  }
  const DeltaView dv = ViewOfDelta(index);
  if (!dv.delta) return a;
  std::vector<DocId> b = op(*dv.delta);
  if (!tl_device_error.empty()) return {};
  for (DocId& d : b) d = (*dv.ids)[d - 1];
  std::vector<DocId> out(a.size() + b.size());
  std::merge(a.begin(), a.end(), b.begin(), b.end(), out.begin());
  return out;
}

// The candidates of a caller's list by the index that holds them: documents of the main index that are live, documents of
// the delta index under its local ids; anything else is not a document of the table. ApplyMutations has run.
struct SplitCandidates {
  DeltaView view;
  std::vector<DocId> main_docs, delta_docs;
  std::vector<size_t> main_pos, delta_pos;  // positions in the caller's list
  SplitCandidates(const Index& index, const std::vector<DocId>& candidates) : view(ViewOfDelta(index)) {
    Index::Impl* im = index.impl();
    std::lock_guard<std::mutex> lock(im->mu);
    for (size_t i = 0; i < candidates.size(); ++i) {
      const DocId c = candidates[i];
      if (im->LiveApplied(c)) {
        main_docs.push_back(c);
        main_pos.push_back(i);
      } else if (view.ids) {
        const auto it = std::lower_bound(view.ids->begin(), view.ids->end(), c);
        if (it != view.ids->end() && *it == c) {
          delta_docs.push_back(static_cast<DocId>(it - view.ids->begin()) + 1);
          delta_pos.push_back(i);
        }
      }
    }
  }
  // `kept` is `given` with some documents taken out (every copy of a document, or none): mark what stayed
  static void MarkKept(const std::vector<DocId>& given, const std::vector<size_t>& pos, const std::vector<DocId>& kept,
                       std::vector<uint8_t>* keep) {
    size_t k = 0;
    for (size_t i = 0; i < given.size() && k < kept.size(); ++i)
      if (given[i] == kept[k]) {
        (*keep)[pos[i]] = 1;
        ++k;
      }
  }
};

// PostingList::GetTopN / the tail of Index::SearchAnd (posting_list.cpp:476-514, index.cpp:352-366) over an ascending list
std::vector<DocId> FinishTopN(std::vector<DocId> all, size_t limit, bool reverse) {
  if (limit > 0 && all.size() > limit) {
    if (reverse) {
      all.erase(all.begin(), all.begin() + static_cast<std::ptrdiff_t>(all.size() - limit));
      std::reverse(all.begin(), all.end());
    } else {
      all.resize(limit);
    }
  } else if (reverse) {
    std::reverse(all.begin(), all.end());
  }
  return all;
}

// The tail of every single-operator call: call(&out, &n) runs the mgx_* operator; its ids, or on failure {} and its
// error recorded for the index and the thread.
template <class Call>
std::vector<DocId> DeviceIds(std::string* last_error, Call&& call) {
  uint32_t* out = nullptr;
  uint64_t n = 0;
  if (call(&out, &n) != MGX_OK) {
    *last_error = mgx_last_error();
    SetDeviceError(*last_error);
    return {};
  }
  return Take(out, n);
}
}  // namespace

std::vector<DocId> Index::SearchAnd(const std::vector<std::string>& terms, size_t limit, bool reverse) const {
  ClearDeviceError();
  if (terms.empty()) return {};  // index.cpp:203
  Finalize();
  if (!impl_->dev) {
    SetDeviceError(impl_->last_error);
    return {};
  }
  if (IsMutable(*this))
    return FinishTopN(OverBoth(*this, [&](const Index& ix) { return ix.SearchAnd(terms, 0, false); }), limit, reverse);
  std::vector<uint32_t> ids;
  for (const auto& t : terms) {
    uint32_t id = 0;
    if (!impl_->Lookup(t, &id)) return {};  // :211-215 unknown term
    ids.push_back(id);
  }
  return DeviceIds(&impl_->last_error, [&](uint32_t** out, uint64_t* n) {
    return mgx_and(impl_->dev, ids.data(), static_cast<uint32_t>(ids.size()), limit, reverse ? 1 : 0, out, n);
  });
}

std::vector<DocId> Index::SearchOr(const std::vector<std::string>& terms) const {  // index.cpp:418-448
  ClearDeviceError();
  if (terms.empty()) return {};
  Finalize();
  if (!impl_->dev) {
    SetDeviceError(impl_->last_error);
    return {};
  }
  if (IsMutable(*this)) return OverBoth(*this, [&](const Index& ix) { return ix.SearchOr(terms); });
  std::vector<uint32_t> ids;
  for (const auto& t : terms) {
    uint32_t id = 0;
    if (impl_->Lookup(t, &id)) ids.push_back(id);  // unknown terms are skipped
  }
  std::sort(ids.begin(), ids.end());
  ids.erase(std::unique(ids.begin(), ids.end()), ids.end());
  if (ids.empty()) return {};
  return DeviceIds(&impl_->last_error, [&](uint32_t** out, uint64_t* n) {
    return mgx_or(impl_->dev, ids.data(), static_cast<uint32_t>(ids.size()), out, n);
  });
}

std::vector<DocId> Index::SearchNot(const std::vector<DocId>& all_docs, const std::vector<std::string>& terms) const {
  ClearDeviceError();
  if (terms.empty()) return all_docs;  // index.cpp:451-453
  Finalize();
  if (!impl_->dev) {
    SetDeviceError(impl_->last_error);
    return {};
  }
  if (IsMutable(*this)) {  // index.cpp:456-484 as written: the union of the terms' lists, then std::set_difference
    const std::vector<DocId> uni = OverBoth(*this, [&](const Index& ix) { return ix.SearchOr(terms); });
    if (!tl_device_error.empty()) return {};
    std::vector<DocId> res;
    std::set_difference(all_docs.begin(), all_docs.end(), uni.begin(), uni.end(), std::back_inserter(res));
    return res;
  }
  std::vector<uint32_t> ids;
  for (const auto& t : terms) {
    uint32_t id = 0;
    if (impl_->Lookup(t, &id)) ids.push_back(id);
  }
  std::sort(ids.begin(), ids.end());
  ids.erase(std::unique(ids.begin(), ids.end()), ids.end());
  if (ids.empty()) return all_docs;
  // std::set_difference (index.cpp:480-484) accepts a sorted all_docs WITH repeats: of m copies of a doc the union
  // holds, m - 1 survive; of a doc it does not hold, all m. The device takes the distinct ids; repeats are put back here.
  const bool repeats = std::adjacent_find(all_docs.begin(), all_docs.end()) != all_docs.end();
  std::vector<DocId> distinct;
  if (repeats) std::unique_copy(all_docs.begin(), all_docs.end(), std::back_inserter(distinct));
  const std::vector<DocId>& in = repeats ? distinct : all_docs;
  std::vector<DocId> kept = DeviceIds(&impl_->last_error, [&](uint32_t** out, uint64_t* n) {
    return mgx_not(impl_->dev, in.data(), in.size(), ids.data(), static_cast<uint32_t>(ids.size()), out, n);
  });
  if (!repeats || !tl_device_error.empty()) return kept;  // (a device failure: {})
  std::vector<DocId> res;
  size_t k = 0;
  for (size_t i = 0; i < all_docs.size();) {
    size_t j = i;
    while (j < all_docs.size() && all_docs[j] == all_docs[i]) ++j;
    while (k < kept.size() && kept[k] < all_docs[i]) ++k;
    const bool survives = k < kept.size() && kept[k] == all_docs[i];
    res.insert(res.end(), survives ? j - i : j - i - 1, all_docs[i]);
    i = j;
  }
  return res;
}

std::vector<DocId> Index::SearchByThreshold(const std::vector<std::string>& terms, size_t threshold) const {
  ClearDeviceError();
  if (terms.empty() || threshold == 0) return {};  // index.cpp:489-491
  std::vector<std::string> uniq = terms;
  DeduplicateSorted(uniq);                         // :496-497
  if (threshold > uniq.size()) return {};          // :499-501
  if (threshold == uniq.size()) return SearchAnd(uniq);  // :504-506
  Finalize();
  if (!impl_->dev) {
    SetDeviceError(impl_->last_error);
    return {};
  }
  if (IsMutable(*this)) return OverBoth(*this, [&](const Index& ix) { return ix.SearchByThreshold(terms, threshold); });
  std::vector<uint32_t> ids;
  for (const auto& t : uniq) {
    uint32_t id = 0;
    if (impl_->Lookup(t, &id)) ids.push_back(id);  // missing lists do not count (:512-518)
  }
  if (ids.size() < threshold) return {};           // :521-523
  return DeviceIds(&impl_->last_error, [&](uint32_t** out, uint64_t* n) {
    return mgx_threshold(impl_->dev, ids.data(), static_cast<uint32_t>(ids.size()), static_cast<uint32_t>(threshold),
                         out, n);
  });
}

std::vector<DocId> Index::FilterByNgrams(const std::vector<DocId>& candidates,
                                         const std::vector<std::string>& terms) const {
  ClearDeviceError();
  if (candidates.empty()) return {};  // index.cpp:372-374
  if (terms.empty()) return candidates;  // :378-380
  Finalize();
  if (!impl_->dev) {
    SetDeviceError(impl_->last_error);
    return {};
  }
  if (IsMutable(*this)) {
    // every candidate belongs to one index (or to neither: not a live document); each index filters its own, and the
    // caller's order — repeats included — is put back from the two answers, which are subsequences of what they were given
    const std::string err = ApplyMutations();
    if (!err.empty()) {
      SetDeviceError(err);
      return {};
    }
    RawScope raw;
    SplitCandidates split(*this, candidates);
    std::vector<uint8_t> keep(candidates.size(), 0);
    const std::vector<DocId> km = split.main_docs.empty() ? std::vector<DocId>() : FilterByNgrams(split.main_docs, terms);
    if (!tl_device_error.empty()) return {};
    split.MarkKept(split.main_docs, split.main_pos, km, &keep);
    if (split.view.delta && !split.delta_docs.empty()) {
      const std::vector<DocId> kd = split.view.delta->FilterByNgrams(split.delta_docs, terms);
      if (!tl_device_error.empty()) return {};
      split.MarkKept(split.delta_docs, split.delta_pos, kd, &keep);
    }
    std::vector<DocId> out;
    for (size_t i = 0; i < candidates.size(); ++i)
      if (keep[i]) out.push_back(candidates[i]);
    return out;
  }
  std::vector<uint32_t> ids;
  for (const auto& t : terms) {
    uint32_t id = 0;
    if (!impl_->Lookup(t, &id)) return {};  // :381-385
    ids.push_back(id);
  }
  return DeviceIds(&impl_->last_error, [&](uint32_t** out, uint64_t* n) {
    return mgx_retain(impl_->dev, candidates.data(), candidates.size(), ids.data(), static_cast<uint32_t>(ids.size()),
                      out, n);
  });
}

// ---- BM25Scorer ---------------------------------------------------------------------------------------------------

double BM25Scorer::ComputeIDF(uint64_t total_docs, uint64_t doc_freq) {  // bm25_scorer.cpp:14-25
  if (total_docs == 0) return 0.0;
  if (doc_freq > total_docs) doc_freq = total_docs;
  const auto n = static_cast<double>(total_docs);
  const auto df = static_cast<double>(doc_freq);
  return std::log((n - df + 0.5) / (df + 0.5) + 1.0);
}

Expected<std::vector<ScoredDoc>, Error> BM25Scorer::ScoreDocuments(const std::vector<DocId>& candidates,
                                                                  const std::vector<std::string>& search_terms,
                                                                  const std::vector<uint64_t>& term_doc_freqs,
                                                                  const Index& index, uint64_t total_docs,
                                                                  double avg_doc_length, const BM25Params& params) {
  if (search_terms.size() != term_doc_freqs.size()) {  // bm25_scorer.cpp:51-55
    return MakeUnexpected(MakeError(ErrorCode::kInvalidArgument,
                                    "BM25 search_terms and term_doc_freqs must have identical lengths"));
  }
  index.Finalize();
  Index::Impl* im = index.impl();
  if (!im->dev) return MakeUnexpected(MakeError(ErrorCode::kInternalError, im->last_error));
  if (IsMutable(index)) {
    // a document's score comes from its own text (tf, length) and the caller's statistics: each index scores its own
    // candidates; an id that is no live document scores 0.0, like a document the store does not hold (bm25_scorer.cpp:73-76)
    const std::string err = index.ApplyMutations();
    if (!err.empty()) return MakeUnexpected(MakeError(ErrorCode::kInternalError, err));
    RawScope raw;
    SplitCandidates split(index, candidates);
    std::vector<ScoredDoc> out;
    out.reserve(candidates.size());
    for (DocId c : candidates) out.push_back({c, 0.0});
    if (!split.main_docs.empty()) {
      auto r = ScoreDocuments(split.main_docs, search_terms, term_doc_freqs, index, total_docs, avg_doc_length, params);
      if (!r) return r;
      for (size_t i = 0; i < r->size(); ++i) out[split.main_pos[i]].score = (*r)[i].score;
    }
    if (split.view.delta && !split.delta_docs.empty()) {
      auto r = ScoreDocuments(split.delta_docs, search_terms, term_doc_freqs, *split.view.delta, total_docs, avg_doc_length, params);
      if (!r) return r;
      for (size_t i = 0; i < r->size(); ++i) out[split.delta_pos[i]].score = (*r)[i].score;
    }
    return out;
  }
  std::vector<uint32_t> ids;
  std::vector<double> idfs;
  bool all_single_gram = true;
  for (size_t i = 0; i < search_terms.size(); ++i) {
    uint32_t id = 0xFFFFFFFFu;  // a term no document contains: tf = 0 everywhere
    auto grams = GenerateQueryNgrams(search_terms[i], index.GetNgramSize(), im->query_kanji,
                                     index.GetCrossBoundaryNgrams());
    DeduplicateSorted(grams);
    if (grams.size() != 1 || grams[0] != search_terms[i]) all_single_gram = false;
    im->Lookup(search_terms[i], &id) || (id = 0xFFFFFFFFu);
    ids.push_back(id);
    idfs.push_back(ComputeIDF(total_docs, term_doc_freqs[i]));
  }
  std::vector<double> scores(candidates.size(), 0.0);
  int rc;
  if (all_single_gram) {  // every term is one n-gram: its tf column holds CountTermOccurrences already
    rc = mgx_score_documents(im->dev, candidates.data(), candidates.size(), ids.data(), idfs.data(),
                             static_cast<uint32_t>(ids.size()), avg_doc_length, params.k1, params.b, scores.data());
  } else {  // bm25_scorer.cpp:71-91 literally: every term counted in the text
    std::vector<uint8_t> bytes;
    std::vector<uint32_t> off(search_terms.size() + 1, 0);
    for (size_t i = 0; i < search_terms.size(); ++i) {
      bytes.insert(bytes.end(), search_terms[i].begin(), search_terms[i].end());
      off[i + 1] = static_cast<uint32_t>(bytes.size());
    }
    bytes.resize(bytes.size() + 16);
    rc = mgx_score_documents_text(im->dev, candidates.data(), candidates.size(), bytes.data(), off.data(),
                                  idfs.data(), static_cast<uint32_t>(search_terms.size()), avg_doc_length, params.k1,
                                  params.b, scores.data());
  }
  if (rc != MGX_OK) return MakeUnexpected(MakeError(static_cast<ErrorCode>(rc), mgx_last_error()));
  std::vector<ScoredDoc> out;
  out.reserve(candidates.size());
  for (size_t i = 0; i < candidates.size(); ++i) out.push_back({candidates[i], scores[i]});
  return out;
}

}  // namespace index

// =================================================================================================================
// query::ResultSorter
// =================================================================================================================

namespace query {

namespace {
namespace hl = mgx::highlight;
// The terms FindMatchPositions scans for: empty ones and those longer than the text are skipped (highlighter.cpp:257-262).
std::vector<hl::Term> HighlightScanTerms(std::string_view text, const std::vector<std::string>& search_terms) {
  std::vector<hl::Term> tv;
  for (const auto& t : search_terms) {
    if (t.empty() || t.size() > text.size()) continue;
    const auto* b = reinterpret_cast<const uint8_t*>(t.data());
    tv.push_back(hl::Term{b, static_cast<uint32_t>(t.size()), hl::CountCps(b, t.size())});
  }
  return tv;
}
}  // namespace

std::vector<std::pair<uint32_t, uint32_t>> Highlighter::FindMatchPositions(std::string_view normalized_text,
                                                                           const std::vector<std::string>& search_terms) {
  std::vector<std::pair<uint32_t, uint32_t>> positions;
  if (normalized_text.size() > 0x7FFFFFFFu) return positions;
  const std::vector<hl::Term> tv = HighlightScanTerms(normalized_text, search_terms);
  std::vector<uint32_t> scratch(tv.size() + 1);
  hl::Scanner sc;
  sc.Init(reinterpret_cast<const uint8_t*>(normalized_text.data()), static_cast<uint32_t>(normalized_text.size()),
          tv.data(), static_cast<uint32_t>(tv.size()), scratch.data());
  uint32_t ms, me, bs, be;
  while (sc.Next(&ms, &me, &bs, &be)) positions.emplace_back(ms, me);
  return positions;
}

HighlightResult Highlighter::Generate(std::string_view normalized_text, const std::vector<std::string>& search_terms,
                                      const HighlightOptions& options) {
  HighlightResult result;
  if (normalized_text.empty() || normalized_text.size() > 0x7FFFFFFFu) return result;  // (:301-305)
  if (options.snippet_length < 1 || options.snippet_length > hl::kMaxSnippetLength || options.max_fragments < 1 ||
      options.max_fragments > hl::kMaxFragments || options.open_tag.size() > hl::kMaxTagBytes ||
      options.close_tag.size() > hl::kMaxTagBytes)
    return result;
  const auto* text = reinterpret_cast<const uint8_t*>(normalized_text.data());
  const uint32_t n = static_cast<uint32_t>(normalized_text.size());
  const std::vector<hl::Term> tv = HighlightScanTerms(normalized_text, search_terms);
  std::vector<uint32_t> scratch(tv.size() + 1);
  std::vector<hl::Window> win(options.max_fragments);
  const size_t span_cap = std::min<size_t>(static_cast<size_t>(options.max_fragments) * options.snippet_length, n);
  std::vector<hl::Span> spans(span_cap + 1);
  hl::Scanner sc;
  sc.Init(text, n, tv.data(), static_cast<uint32_t>(tv.size()), scratch.data());
  hl::Builder bd;
  bd.Init(options.snippet_length, options.max_fragments, win.data(), spans.data(), static_cast<uint32_t>(span_cap));
  uint32_t ms, me, bs, be;
  while (!bd.done && sc.Next(&ms, &me, &bs, &be)) bd.Feed(ms, me, bs, be, true);
  const uint32_t total = bd.done ? hl::kNoTotal : hl::CountCps(text, n);
  bd.Finish(total, true);
  hl::FinalizeWindows(win.data(), bd.n_win, bd.matched, options.snippet_length, total, &bd.flags);
  hl::Header h{bd.n_win, bd.flags, bd.n_spans, 0};
  h.n_bytes = hl::WindowsToBytes(text, n, win.data(), bd.n_win);
  const auto* ot = reinterpret_cast<const uint8_t*>(options.open_tag.data());
  const auto* ct = reinterpret_cast<const uint8_t*>(options.close_tag.data());
  const size_t len = hl::Render(h, win.data(), spans.data(), text, true, ot, options.open_tag.size(), ct,
                                options.close_tag.size(), nullptr, 0);
  result.snippet.resize(len);
  hl::Render(h, win.data(), spans.data(), text, true, ot, options.open_tag.size(), ct, options.close_tag.size(),
             reinterpret_cast<uint8_t*>(result.snippet.data()), len);
  return result;
}

OriginalMap BuildOriginalMap(std::string_view original_text, std::string_view normalized_text,
                             const std::function<std::string(std::string_view)>& normalizer) {
  OriginalMap m;
  bool identity = true;
  uint32_t total = 0;
  for (const auto& seg : mygram::utils::SegmentOriginalText(original_text)) {  // (:329-336)
    const std::string piece = normalizer(original_text.substr(seg.byte_begin, seg.byte_end - seg.byte_begin));
    const uint32_t n = hl::CountCps(reinterpret_cast<const uint8_t*>(piece.data()), piece.size());
    for (uint32_t i = 0; i < n; ++i) {
      identity = identity && seg.cp_begin == m.pairs.size() / 2 && seg.cp_end == seg.cp_begin + 1;
      m.pairs.push_back(seg.cp_begin);
      m.pairs.push_back(seg.cp_end);
    }
    total = seg.cp_end;
  }
  const size_t normalized_cps = hl::CountCps(reinterpret_cast<const uint8_t*>(normalized_text.data()), normalized_text.size());
  if (m.pairs.size() / 2 != normalized_cps) {  // (:342-344)
    m.kind = MGX_ORIG_UNMAPPABLE;
    m.pairs.clear();
  } else if (identity && total == normalized_cps) {
    m.kind = MGX_ORIG_IDENTITY;
    m.pairs.clear();
  } else {
    m.kind = MGX_ORIG_MAPPED;
  }
  return m;
}

HighlightResult Highlighter::GenerateOriginal(std::string_view original_text,
                                              const std::vector<std::string>& normalized_search_terms,
                                              const std::function<std::string(std::string_view)>& normalizer,
                                              const HighlightOptions& options) {
  HighlightResult result;
  if (original_text.empty() || original_text.size() > 0x7FFFFFFFu) return result;  // (:315-319)
  if (options.snippet_length < 1 || options.snippet_length > hl::kMaxSnippetLength || options.max_fragments < 1 ||
      options.max_fragments > hl::kMaxFragments || options.open_tag.size() > hl::kMaxTagBytes ||
      options.close_tag.size() > hl::kMaxTagBytes)
    return result;
  std::string normalized;
  OriginalMap m;
  m.kind = MGX_ORIG_UNMAPPABLE;  // (no terms, :323-325: the no-match window; nothing is normalized)
  if (!normalized_search_terms.empty()) {
    normalized = normalizer(original_text);  // (:327)
    if (normalized.size() > 0x7FFFFFFFu) return result;
    m = BuildOriginalMap(original_text, normalized, normalizer);
  }
  const auto* original = reinterpret_cast<const uint8_t*>(original_text.data());
  const auto* text = reinterpret_cast<const uint8_t*>(normalized.data());
  const uint32_t on = static_cast<uint32_t>(original_text.size()), n = static_cast<uint32_t>(normalized.size());
  const std::vector<hl::Term> tv = HighlightScanTerms(normalized, normalized_search_terms);
  std::vector<uint32_t> scratch(tv.size() + 1);
  std::vector<hl::Window> win(options.max_fragments);
  const size_t span_cap = std::min<size_t>(static_cast<size_t>(options.max_fragments) * options.snippet_length, n);
  std::vector<hl::Span> spans(span_cap + 1);
  const hl::Header h = hl::GenerateOriginalRecord(
      original, on, text, n, m.kind, reinterpret_cast<const hl::MapPair*>(m.pairs.data()),
      static_cast<uint32_t>(m.pairs.size() / 2), tv.data(), static_cast<uint32_t>(tv.size()), options.snippet_length,
      options.max_fragments, win.data(), spans.data(), static_cast<uint32_t>(span_cap), scratch.data());
  const auto* ot = reinterpret_cast<const uint8_t*>(options.open_tag.data());
  const auto* ct = reinterpret_cast<const uint8_t*>(options.close_tag.data());
  const size_t len = hl::Render(h, win.data(), spans.data(), original, true, ot, options.open_tag.size(), ct,
                                options.close_tag.size(), nullptr, 0);
  result.snippet.resize(len);
  hl::Render(h, win.data(), spans.data(), original, true, ot, options.open_tag.size(), ct, options.close_tag.size(),
             reinterpret_cast<uint8_t*>(result.snippet.data()), len);
  return result;
}

std::vector<DocId> ResultSorter::SortByScore(const index::Index& index, const std::vector<DocId>& results,
                                             const std::vector<double>& scores, SortOrder order, uint32_t limit,
                                             uint32_t offset) {
  index::ClearDeviceErrorForSorter();
  if (results.empty()) return {};  // result_sorter.cpp:663-665
  index.Finalize();
  index::Index::Impl* im = index.impl();
  if (!im->dev) {
    index::SetDeviceError(im->last_error);
    return {};
  }
  uint32_t* out = nullptr;
  uint64_t n = 0;
  if (mgx_sort_by_score(im->dev, results.data(), scores.data(), results.size(), order == SortOrder::DESC ? 1 : 0, limit,
                        offset, &out, &n) != MGX_OK) {
    im->last_error = mgx_last_error();
    index::SetDeviceError(im->last_error);
    return {};
  }
  return Take(out, n);
}

std::vector<DocId> ResultSorter::SortByScore(const std::vector<DocId>& results, const std::vector<double>& scores,
                                             SortOrder order, uint32_t limit, uint32_t offset) {
  index::ClearDeviceErrorForSorter();
  if (results.empty()) return {};
  const index::Index* idx = index::LastUsedIndex();
  if (idx == nullptr) {
    index::SetDeviceError("ResultSorter::SortByScore: no Index has been used in this process (the sort runs on its device)");
    return {};
  }
  return SortByScore(*idx, results, scores, order, limit, offset);
}

}  // namespace query

namespace storage {
size_t DocumentStore::Size() const { return static_cast<size_t>(index_->Bm25DocCount()); }
}  // namespace storage

// =================================================================================================================
// search_pipeline::ExecuteBatch / BatchExecutor
// =================================================================================================================

namespace search_pipeline {

namespace {
// The gram ids of one term: a query term is a handful of n-grams, so they live inside the object (no heap traffic on the
// planner's hot path — it plans a million terms a second); a long term spills to the heap.
class IdVec {
 public:
  IdVec() = default;
  IdVec(const IdVec& o) { assign(o.data(), o.size()); }
  IdVec(IdVec&& o) noexcept { steal(o); }
  IdVec& operator=(const IdVec& o) {
    if (this != &o) assign(o.data(), o.size());
    return *this;
  }
  IdVec& operator=(IdVec&& o) noexcept {
    if (this != &o) steal(o);
    return *this;
  }
  void push_back(uint32_t v) {
    if (!heap_.empty()) {
      heap_.push_back(v);
    } else if (n_ < kInline) {
      inl_[n_] = v;
    } else {
      heap_.assign(inl_, inl_ + n_);
      heap_.push_back(v);
    }
    ++n_;
  }
  void assign(const uint32_t* p, size_t n) {
    clear();
    for (size_t i = 0; i < n; ++i) push_back(p[i]);
  }
  void assign(size_t n, uint32_t v) {
    clear();
    for (size_t i = 0; i < n; ++i) push_back(v);
  }
  void clear() {
    heap_.clear();
    n_ = 0;
  }
  [[nodiscard]] const uint32_t* data() const { return heap_.empty() ? inl_ : heap_.data(); }
  [[nodiscard]] size_t size() const { return n_; }
  [[nodiscard]] bool empty() const { return n_ == 0; }
  [[nodiscard]] const uint32_t* begin() const { return data(); }
  [[nodiscard]] const uint32_t* end() const { return data() + n_; }

 private:
  static constexpr size_t kInline = 8;
  void steal(IdVec& o) {
    heap_ = std::move(o.heap_);
    std::copy(o.inl_, o.inl_ + kInline, inl_);
    n_ = o.n_;
    o.clear();
  }
  uint32_t inl_[kInline] = {0};
  size_t n_ = 0;
  std::vector<uint32_t> heap_;
};

struct TermInfo {  // search_pipeline.h:44-55
  IdVec gram_ids;
  size_t n_grams = 0;
  uint64_t estimated_size = 0;  // UINT64_MAX = no n-grams
  uint64_t df = 0;
  bool is_gram = false;  // the term is exactly one n-gram
  std::string normalized;
};

// One query planned on the host the way ExecuteFullPipeline's regular branch (search_pipeline.cpp:2002-2030) or its
// boolean branch (:1842-1913) plans it: everything the C ABI's mgx_query points at lives in this object.
struct PlannedQuery {
  mgx_query q{};
  bool sort_string = false;        // BatchQuery::sort_column names a string column (dictionary ranks)
  bool on_device = false;          // false: resolved on the host (empty_term_detected) or failed
  bool empty_term_detected = false;
  ErrorCode error = ErrorCode::kSuccess;
  std::string error_message;
  std::vector<mgx_term> terms, not_terms;
  std::vector<IdVec> ids;       // (reserved before the first mgx_term points into it: elements must not move)
  std::vector<TermInfo> tis;    // scratch of PlanQuery, kept for its storage
  std::vector<mgx_filter> filters;
  std::vector<mgx_condition> conditions;  // FILTER conditions the batch evaluates itself (ResolveCondition's routing)
  std::vector<mgx_expr_token> expr;
  std::vector<uint32_t> score_list;  // mgx_query::score_terms of expression / FUZZY queries
  bool has_score_list = false;
  std::deque<std::string> texts;  // normalized text-level terms (addresses stay valid as the deque grows)
  // BatchQuery::facet_columns resolved against this index, one per name: its device column and its values (ascending)
  struct FacetColumn {
    bool found = false;
    uint32_t device_id = 0;
    std::vector<storage::FilterValue> dict;
  };
  bool faceted = false;
  std::vector<FacetColumn> facets;
  // Back to the freshly constructed state WITHOUT giving memory back: an executor slot re-plans a thousand of these
  // per batch, and constructing one allocates (the deque's map and first node alone are two mallocs).
  void Reset() {
    q = mgx_query{};
    on_device = empty_term_detected = false;
    error = ErrorCode::kSuccess;
    error_message.clear();
    terms.clear();
    not_terms.clear();
    ids.clear();
    tis.clear();
    filters.clear();
    conditions.clear();
    expr.clear();
    score_list.clear();
    has_score_list = false;
    texts.clear();
    faceted = false;
    facets.clear();
  }
};

TermInfo MakeInfo(const index::Index& index, const index::Index::Impl* im, const std::string& raw) {
  // GenerateTermInfos, search_pipeline.cpp:569-603
  TermInfo ti;
  ti.normalized = index.NormalizeText(raw);
  {
    // the commonest term of an n-gram index is exactly one n-gram of ASCII letters / digits: GenerateQueryNgrams would
    // return that one string (no whitespace to split at, no CJK run for the kanji size) — same answers without building
    // a vector of strings
    const int n = index.GetNgramSize();
    bool one_gram = n > 0 && ti.normalized.size() == static_cast<size_t>(n);
    for (size_t i = 0; one_gram && i < ti.normalized.size(); ++i) {
      const unsigned char c = static_cast<unsigned char>(ti.normalized[i]);
      one_gram = (c >= '0' && c <= '9') || (c >= 'a' && c <= 'z') || (c >= 'A' && c <= 'Z');
    }
    if (one_gram) {
      uint32_t id = 0;
      uint64_t ps = 0;
      if (!im->Resolve(ti.normalized, &id, &ps)) ps = 0;
      ti.n_grams = 1;
      if (ps > 0) ti.gram_ids.push_back(id);
      ti.estimated_size = ps;
      ti.is_gram = true;
      ti.df = ps;
      return ti;
    }
  }
  auto grams = GenerateQueryNgrams(ti.normalized, index.GetNgramSize(), im->query_kanji, index.GetCrossBoundaryNgrams());
  DeduplicateSorted(grams);
  ti.n_grams = grams.size();
  uint64_t mn = UINT64_MAX;
  for (const auto& g : grams) {
    uint32_t id = 0;
    uint64_t ps = 0;
    if (!im->Resolve(g, &id, &ps)) ps = 0;
    if (ps > 0) {
      mn = std::min(mn, ps);
      ti.gram_ids.push_back(id);
    } else {
      mn = 0;
      break;
    }
  }
  ti.estimated_size = mn;
  // a term that IS its one n-gram: df = |posting list|, tf = the gram's tf column; any other term is counted in the
  // text on the device (PopulateTermDocumentFrequency / CountTermOccurrences)
  ti.is_gram = grams.size() == 1 && grams[0] == ti.normalized;
  ti.df = (ti.is_gram && mn != UINT64_MAX) ? mn : 0;
  return ti;
}

void Fail(PlannedQuery* p, ErrorCode code, const char* msg) {
  p->error = code;
  p->error_message = msg;
}

// ---- FILTER conditions -> device bitmaps -------------------------------------------------------------------------------
template <typename T>
bool ParseWhole(const std::string& s, T* out) {  // std::from_chars over the whole string (search_pipeline.cpp:962-991)
  const char* end = s.data() + s.size();
  T v{};
  auto [ptr, ec] = std::from_chars(s.data(), end, v);
  if (ec != std::errc() || ptr != end) return false;
  *out = v;
  return true;
}

struct ResolvedFilter {
  bool skip = false;     // the condition holds for every document
  bool is_condition = false;  // `condition` travels with the batch (mgx_query.conditions); otherwise row `bitmap` of the index
  uint32_t bitmap = 0;
  bool negate = false;
  mgx_condition condition{};
};

// One FilterCondition against the table's columns. bitmap_mode: every condition of the query is EQ / NE (the FilterIndex
// path, ApplyFiltersWithBitmap search_pipeline.cpp:1196-1237); otherwise the per-document semantics of ApplyFilters
// (:1098-1194) for every condition of the query. Returns an error message or "".
std::string ResolveCondition(const index::Index& index, const query::FilterCondition& cond, bool bitmap_mode,
                             ResolvedFilter* out) {
  index.FlushPendingFilterColumns();
  index::Index::Impl* im = index.impl();
  std::lock_guard<std::mutex> lock(im->filter_mu);
  const index::Index::Impl::FilterColumn* col = im->ResolveColumn(cond.column);
  auto remember = [&](uint32_t bitmap, bool negate, bool skip) {
    out->bitmap = bitmap;
    out->negate = negate;
    out->skip = skip;
  };
  auto empty_bitmap = [&](uint32_t* id) -> std::string {
    if (!im->have_empty_bitmap) {
      if (mgx_index_add_filter_bitmap(im->dev, nullptr, 0, &im->empty_bitmap) != MGX_OK) return mgx_last_error();
      im->have_empty_bitmap = true;
    }
    *id = im->empty_bitmap;
    return "";
  };
  const bool is_ne = cond.op == query::FilterOp::NE;
  // a column no document has: every stored value is NULL — nothing equals or orders against it, != holds everywhere
  // (bitmap path: OrEqBitmapInto finds no column, :107-109; per-document path: NULL passes != only, :1151-1157)
  if (col == nullptr || col->type == 0) {
    if (is_ne) {
      remember(0, false, true);
      return "";
    }
    uint32_t id = 0;
    const std::string err = empty_bitmap(&id);
    if (!err.empty()) return err;
    remember(id, false, false);
    return "";
  }
  const size_t type = col->type;
  const std::string& v = cond.value;
  uint64_t lit = 0;
  bool valid = false;
  uint32_t op = 0;
  double eps = 0.0;
  if (type == 11) {  // string column: ranks in the column's bytewise-sorted dictionary
    const storage::FilterValue needle{v};
    const auto lb = std::lower_bound(col->dict.begin(), col->dict.end(), needle);
    const auto ub = std::upper_bound(col->dict.begin(), col->dict.end(), needle);
    const uint64_t lbi = static_cast<uint64_t>(lb - col->dict.begin()), ubi = static_cast<uint64_t>(ub - col->dict.begin());
    valid = true;
    switch (cond.op) {
      case query::FilterOp::EQ:
      case query::FilterOp::NE:
        op = MGX_CMP_EQ;  // (NE: the EQ set, negated below / by the null rule)
        lit = lb != ub ? lbi : ~0ull;  // a literal no document holds equals no rank
        break;
      case query::FilterOp::LT: op = MGX_CMP_LT; lit = lbi; break;   // stored <  v  <=> rank <  lower_bound
      case query::FilterOp::LTE: op = MGX_CMP_LT; lit = ubi; break;  // stored <= v  <=> rank <  upper_bound
      case query::FilterOp::GT: op = MGX_CMP_GE; lit = ubi; break;   // stored >  v  <=> rank >= upper_bound
      default: op = MGX_CMP_GE; lit = lbi; break;                     // stored >= v  <=> rank >= lower_bound
    }
  } else {
    switch (cond.op) {
      case query::FilterOp::EQ: case query::FilterOp::NE: op = MGX_CMP_EQ; break;
      case query::FilterOp::LT: op = MGX_CMP_LT; break;
      case query::FilterOp::LTE: op = MGX_CMP_LE; break;
      case query::FilterOp::GT: op = MGX_CMP_GT; break;
      default: op = MGX_CMP_GE; break;
    }
    if (type == 1) {  // bool
      if (bitmap_mode) {  // BuildTypeUnionBitmap :1043-1048
        valid = v == "1" || v == "true" || v == "0" || v == "false";
        lit = (v == "1" || v == "true") ? 1 : 0;
      } else {  // ParseFilterValue :957: anything but "1" / "true" reads as false
        valid = true;
        lit = (v == "1" || v == "true") ? 1 : 0;
      }
    } else if (type == 12) {  // double
      double d = 0.0;
      valid = ParseWhole(v, &d);
      std::memcpy(&lit, &d, 8);
      if (!bitmap_mode) eps = 1e-9;  // mygram::constants::kFilterValueEpsilon (src/utils/constants.h:104)
    } else if (type == 3 || type == 5 || type == 7 || type == 9) {  // unsigned
      uint64_t u = 0;
      valid = ParseWhole(v, &u);
      lit = u;
      if (bitmap_mode && valid) {  // the literal must be representable in the column's type (:1078-1089)
        const uint64_t mx = type == 3 ? 0xFFull : type == 5 ? 0xFFFFull : type == 7 ? 0xFFFFFFFFull : ~0ull;
        valid = u <= mx;
      }
    } else {  // signed integers, TimeValue
      int64_t i = 0;
      valid = ParseWhole(v, &i);
      lit = static_cast<uint64_t>(i);
      if (bitmap_mode && valid) {  // :1057-1067
        const int64_t lo = type == 2 ? INT8_MIN : type == 4 ? INT16_MIN : type == 6 ? INT32_MIN : INT64_MIN;
        const int64_t hi = type == 2 ? INT8_MAX : type == 4 ? INT16_MAX : type == 6 ? INT32_MAX : INT64_MAX;
        valid = i >= lo && i <= hi;
      }
    }
  }
  uint32_t id = 0;
  // EQ: AND the union of the literal's interpretations; NE: ANDNOT it (NULL documents are in no value bitmap: they
  // pass NE, fail EQ). No interpretation in this column's type: the union is empty.
  if (bitmap_mode && !valid) {
    if (is_ne) {
      remember(0, false, true);
      return "";
    }
    const std::string err = empty_bitmap(&id);
    if (!err.empty()) return err;
    remember(id, false, false);
    return "";
  }
  // The condition as the device evaluates it. bitmap path: the EQ set, ANDed or (NE) ANDNOTed; per-document path: the set
  // of documents that PASS the condition, ANDed.
  mgx_condition c{};
  c.column_id = col->device_id;
  c.literal_bits = lit;
  if (bitmap_mode) {
    c.op = MGX_CMP_EQ;
    c.negate = is_ne ? 1u : 0u;
  } else {
    c.op = is_ne ? static_cast<uint32_t>(MGX_CMP_NE) : op;
    c.eq_epsilon = eps;
    c.null_matches = is_ne ? 1u : 0u;
    c.never_matches = valid ? 0u : 1u;
  }
  // Routing. A persistent row of the index only where the column's cardinality bounds how many there can be: = / != against
  // a value the column's dictionary holds. Everything else — every range operator, a literal no document holds (request
  // ids, timestamps) — travels with the batch as a condition: planning it touches no device state and leaves nothing behind.
  bool in_dict = false;
  if (valid && (cond.op == query::FilterOp::EQ || is_ne)) {
    if (type == 11) {
      in_dict = lit != ~0ull;
    } else {
      const storage::FilterValue fv = index::FilterValueFromBits(type, lit, col->dict);
      bool ordered = true;
      if (type == 12) {
        double d;
        std::memcpy(&d, &lit, 8);
        ordered = d == d;  // (NaN orders against nothing: no dictionary search)
      }
      in_dict = ordered && index::WidenFilterValue(fv) == lit && std::binary_search(col->dict.begin(), col->dict.end(), fv);
    }
  }
  if (!in_dict) {
    out->is_condition = true;
    out->condition = c;
    return "";
  }
  std::string key;
  key.push_back(bitmap_mode ? 'b' : 'f');
  key.push_back(static_cast<char>('0' + static_cast<int>(cond.op)));  // (= and != share the EQ set on the bitmap path, not `negate`)
  key += col->name;
  key.push_back('\0');
  key.append(reinterpret_cast<const char*>(&lit), 8);
  const auto hit = im->condition_cache.find(key);
  if (hit != im->condition_cache.end()) {
    remember(hit->second.first, hit->second.second, false);
    return "";
  }
  if (mgx_index_filter_compare(im->dev, c.column_id, c.op, c.literal_bits, c.eq_epsilon, static_cast<int>(c.null_matches),
                               static_cast<int>(c.never_matches), &id) != MGX_OK)
    return mgx_last_error();
  remember(id, c.negate != 0, false);
  im->condition_cache.emplace(key, std::make_pair(id, c.negate != 0));
  return "";
}

void PlanQueryBody(const index::Index& index, const BatchQuery& q, uint64_t total_docs, double avgdl, PlannedQuery* p);

// PlanQueryBody, and BatchQuery::sort_column resolved against the index's columns: the device query then asks for
// MGX_SORT_COLUMN / _RANK with the pagination offset.
// The search part of a FACET (ExecuteFacetPipeline): the query's own, or — FACET without search terms — every document
// (GetAllDocIds, :2118) narrowed by its NOT terms and filters: the expression NOT(<empty>) is the universe. No order, no
// page: limit and offset page the values.
BatchQuery FacetSearchPart(const BatchQuery& query) {
  BatchQuery q = query;
  q.sort_by_score = false;
  q.sort_column.clear();
  q.facet_columns.clear();
  q.limit = 0;
  q.offset = 0;
  if (q.terms.empty() && !q.ast) {
    auto all = std::make_shared<query::QueryNode>(query::NodeType::NOT);
    all->children.push_back(std::make_unique<query::QueryNode>(std::string()));
    q.ast = std::move(all);
  }
  return q;
}

// BatchQuery::facet_columns: the names resolved against this index (a name it does not know is left to the caller: on a
// table with a delta the other index may hold it), and the search part planned as a limit-0 doc-id query.
void PlanFacetQuery(const index::Index& index, const BatchQuery& q, uint64_t total_docs, double avgdl, PlannedQuery* p) {
  if (q.highlight) return Fail(p, ErrorCode::kInvalidArgument, "facet_columns and highlight: a faceted query returns counts, not a page");
  if (q.return_documents) return Fail(p, ErrorCode::kInvalidArgument, "facet_columns and return_documents: a faceted query returns counts, not a page");
  if (q.facet_columns.size() > MGX_FACET_MAX_COLUMNS)
    return Fail(p, ErrorCode::kOutOfRange, "more than MGX_FACET_MAX_COLUMNS (8) facet columns in one query");
  index.FlushPendingFilterColumns();
  const index::Index::Impl* im = index.impl();
  std::vector<PlannedQuery::FacetColumn> cols(q.facet_columns.size());
  {
    std::lock_guard<std::mutex> lock(im->filter_mu);
    for (size_t c = 0; c < cols.size(); ++c) {
      const index::Index::Impl::FilterColumn* col = im->ResolveColumn(q.facet_columns[c]);
      if (col == nullptr) continue;
      cols[c].found = true;
      cols[c].device_id = col->device_id;
      cols[c].dict = col->dict;
    }
  }
  PlanQueryBody(index, FacetSearchPart(q), total_docs, avgdl, p);
  p->faceted = true;
  p->facets = std::move(cols);
}

// BatchQuery::sort_column names the table's primary-key column (EqualsIgnoreCase, result_sorter.cpp:239). A delta index
// asks the main index it stands beside: the name is the table's.
bool IsPrimaryKeyColumn(const index::Index::Impl* im, const std::string& name) {
  const std::string& pk = im->fallback ? im->fallback->primary_key_column : im->primary_key_column;
  if (name.empty() || pk.size() != name.size()) return false;
  for (size_t i = 0; i < name.size(); ++i)
    if (std::tolower(static_cast<unsigned char>(pk[i])) != std::tolower(static_cast<unsigned char>(name[i]))) return false;
  return true;
}

void PlanQuery(const index::Index& index, const BatchQuery& q, uint64_t total_docs, double avgdl, PlannedQuery* p) {
  p->sort_string = false;
  if (!q.facet_columns.empty()) return PlanFacetQuery(index, q, total_docs, avgdl, p);
  const index::Index::Impl* im = index.impl();
  if (q.sort_primary_key || IsPrimaryKeyColumn(im, q.sort_column)) {
    // GetSortKey's first branch (result_sorter.cpp:239): the empty ORDER BY column, or the primary-key column's name —
    // before any filter column of that name is looked for
    if (q.sort_by_score) return Fail(p, ErrorCode::kInvalidArgument, "sort_primary_key and sort_by_score are two orders: set one of them");
    PlanQueryBody(index, q, total_docs, avgdl, p);
    if (p->error != ErrorCode::kSuccess || !p->on_device) return;
    p->q.sort = MGX_SORT_PRIMARY_KEY;
    p->q.sort_column = 0;
    p->q.sort_key_bias = 0;
    p->q.offset = q.offset;
    return;
  }
  if (q.sort_column.empty()) return PlanQueryBody(index, q, total_docs, avgdl, p);
  if (q.sort_by_score) return Fail(p, ErrorCode::kInvalidArgument, "sort_column and sort_by_score are two orders: set one of them");
  index.FlushPendingFilterColumns();
  uint32_t device_column = 0, bias = 0;
  bool is_string = false;
  {
    std::lock_guard<std::mutex> lock(im->filter_mu);
    const index::Index::Impl::FilterColumn* col = im->ResolveColumn(q.sort_column);
    if (col == nullptr) {  // result_sorter.cpp:549-552
      p->error = ErrorCode::kQueryInvalidSort;
      p->error_message = "Sort column '" + q.sort_column +
                         "' not found. Column does not exist as filter column or primary key. Check column name spelling.";
      return;
    }
    device_column = col->device_id;
    is_string = col->type == 11;
    // the key of a string is the string: the empty one ties with NULL (both keys are ""), so its rank 0 stays 0
    if (is_string) bias = (!col->dict.empty() && std::get<std::string>(col->dict.front()).empty()) ? 0u : 1u;
  }
  PlanQueryBody(index, q, total_docs, avgdl, p);
  p->sort_string = is_string;
  if (p->error != ErrorCode::kSuccess || !p->on_device) return;
  p->q.sort = is_string ? MGX_SORT_COLUMN_RANK : MGX_SORT_COLUMN;
  p->q.sort_column = device_column;
  p->q.sort_key_bias = bias;
  p->q.offset = q.offset;
}

void PlanQueryBody(const index::Index& index, const BatchQuery& q, uint64_t total_docs, double avgdl, PlannedQuery* p) {
  const index::Index::Impl* im = index.impl();
  // FILTER clauses: caller-resolved bitmaps, then the parsed conditions (resolved here, cached by the Index)
  auto add_filters = [&]() -> bool {
    for (const auto& f : q.filters) p->filters.push_back(mgx_filter{f.first, f.second ? 1u : 0u});
    bool bitmap_mode = true;  // AllFiltersHaveBitmapSupport, search_pipeline.cpp:996-1003
    for (const auto& c : q.filter_conditions)
      bitmap_mode = bitmap_mode && (c.op == query::FilterOp::EQ || c.op == query::FilterOp::NE);
    for (const auto& c : q.filter_conditions) {
      ResolvedFilter rf;
      const std::string err = ResolveCondition(index, c, bitmap_mode, &rf);
      if (!err.empty()) {
        p->error = ErrorCode::kInternalError;
        p->error_message = err;
        return false;
      }
      if (rf.skip) continue;
      if (rf.is_condition) p->conditions.push_back(rf.condition);
      else p->filters.push_back(mgx_filter{rf.bitmap, rf.negate ? 1u : 0u});
    }
    if (p->filters.size() + p->conditions.size() > MGX_MAX_TERMS) {
      p->error = ErrorCode::kInvalidArgument;
      p->error_message = "more than 64 filters in one query";
      return false;
    }
    return true;
  };
  auto finish = [&](uint32_t sort) {
    mgx_query& m = p->q;
    m.terms = p->terms.data();
    m.n_terms = static_cast<uint32_t>(p->terms.size());
    m.not_terms = p->not_terms.data();
    m.n_not_terms = static_cast<uint32_t>(p->not_terms.size());
    m.filters = p->filters.data();
    m.n_filters = static_cast<uint32_t>(p->filters.size());
    m.conditions = p->conditions.data();
    m.n_conditions = static_cast<uint32_t>(p->conditions.size());
    m.sort = sort;
    m.limit = q.limit;
    m.reverse = q.order == query::SortOrder::DESC ? 1 : 0;
    m.k1 = q.bm25.k1;
    m.b = q.bm25.b;
    m.total_docs = total_docs;
    m.avg_doc_length = avgdl;
    if (p->has_score_list) {  // (non-NULL even when empty: "no term is scored" is not "every term is")
      static const uint32_t kNone = 0;
      m.score_terms = p->score_list.empty() ? &kNone : p->score_list.data();
      m.n_score_terms = static_cast<uint32_t>(p->score_list.size());
    }
    p->on_device = true;
  };
  auto add_not_terms = [&]() -> bool {  // ApplyNotFilter :871-932
    for (const auto& t : q.not_terms) {
      TermInfo ti = MakeInfo(index, im, t);
      if (ti.n_grams == 0) {
        // shorter than one n-gram: the docs whose text contains it (SearchTermDocuments :438-446); "" matches nothing
        if (ti.normalized.empty()) continue;
        p->texts.push_back(ti.normalized);
        p->not_terms.push_back(mgx_term{nullptr, 0, 0, 0.0, reinterpret_cast<const uint8_t*>(p->texts.back().data()),
                                        static_cast<uint32_t>(p->texts.back().size())});
        continue;
      }
      if (ti.estimated_size == 0) continue;  // an unknown gram: the NOT term matches nothing
      p->ids.push_back(ti.gram_ids);
      p->not_terms.push_back(mgx_term{p->ids.back().data(), static_cast<uint32_t>(p->ids.back().size()), 0, 0.0, nullptr, 0});
    }
    return true;
  };
  if (q.ast) {
    // ---- boolean expression: distinct TERM leaves in first-use order, tree in postfix -----------------------------
    if (!q.terms.empty())
      return Fail(p, ErrorCode::kNotImplemented, "an expression query takes its terms from the tree");
    std::vector<std::string> leaves;
    std::vector<TermInfo> tis;
    bool bad = false;
    // One distinct leaf as the tree's set algebra and its text filter see it.
    struct Leaf {
      bool substring = false;  // plain only: shorter than one n-gram — the documents whose text contains it
      bool empty = false;      // the empty doc set
      bool scored = false;     // may add to a score: every n-gram known (else it occurs in no text: tf = df = 0)
      uint32_t threshold = 0;  // FUZZY: "at least theta of its known grams" (0: all of them)
    };
    std::vector<Leaf> lvs;
    const uint32_t fz = q.fuzzy_max_distance;
    // verify_text (search_pipeline.cpp:1505-1578): the tree is re-evaluated over each candidate's text, so every leaf
    // carries its normalized text; an empty leaf still counts there (under a NOT), only "" is false on every text
    const bool tree_verify = q.verify_text;
    auto make_leaf = [&](TermInfo& ti) {
      Leaf lf;
      const bool known_all = ti.n_grams != 0 && ti.estimated_size != 0 && ti.estimated_size != UINT64_MAX;
      lf.scored = known_all;
      if (fz == 0) {
        // a term with an unknown gram is an empty doc set inside the tree; a term shorter than one n-gram is the documents
        // whose text contains it (regular_term_search -> SearchTermDocuments, search_pipeline.cpp:1446-1455, :438-446)
        lf.substring = ti.n_grams == 0 && !ti.normalized.empty();
        lf.empty = !lf.substring && !known_all;
        return lf;
      }
      // FUZZY d: every leaf is fuzzy_term_search (:1424-1445) — no n-grams: the empty set (:1431-1433); else theta and the
      // known grams exactly as ExecuteWithFuzzy's terms below (Index::SearchByThreshold skips unknown grams)
      auto grams = GenerateQueryNgrams(ti.normalized, index.GetNgramSize(), im->query_kanji, index.GetCrossBoundaryNgrams());
      DeduplicateSorted(grams);
      if (grams.empty()) {
        lf.empty = true;
        return lf;
      }
      size_t n_eff = index.GetNgramSize() > 0 ? static_cast<size_t>(index.GetNgramSize()) : 2;
      if (im->query_kanji > 0) {
        size_t short_count = 0;
        for (const auto& g : grams) short_count += g.size() <= 3 ? 1 : 0;
        if (short_count > grams.size() / 2) n_eff = static_cast<size_t>(im->query_kanji);
      }
      const size_t drop = static_cast<size_t>(fz) * n_eff;
      const size_t theta = grams.size() > drop ? grams.size() - drop : 1;
      IdVec known;
      for (const auto& g : grams) {
        uint32_t id = 0;
        uint64_t ps = 0;
        if (im->Resolve(g, &id, &ps) && ps > 0) known.push_back(id);
      }
      lf.empty = known.empty() || (theta == grams.size() ? known.size() != grams.size() : known.size() < theta);
      lf.scored = !lf.empty && known.size() == grams.size();
      lf.threshold = (lf.empty || theta >= known.size()) ? 0u : static_cast<uint32_t>(theta);
      ti.gram_ids = std::move(known);
      return lf;
    };
    // SORT _score: the TERM leaves that are not under a NOT, in tree order, repeats kept (CollectAstScoringTerms,
    // search_pipeline.cpp:232-254; search_handler.cpp:428-456 scores exactly those, whatever branch matched)
    p->has_score_list = q.sort_by_score;
    std::function<void(const query::QueryNode&, bool)> walk = [&](const query::QueryNode& nd, bool under_not) {
      if (nd.type == query::NodeType::TERM) {
        size_t k = 0;
        while (k < leaves.size() && leaves[k] != nd.term) ++k;
        if (k == leaves.size()) {
          leaves.push_back(nd.term);
          tis.push_back(MakeInfo(index, im, nd.term));
          lvs.push_back(make_leaf(tis.back()));
        }
        const bool as_term = !lvs[k].empty || (tree_verify && !tis[k].normalized.empty());
        p->expr.push_back(as_term ? mgx_expr_token{MGX_EXPR_TERM, static_cast<uint32_t>(k)} : mgx_expr_token{MGX_EXPR_EMPTY, 0});
        // (a leaf with an unknown gram occurs in no text: tf = df = 0, it adds nothing to any score)
        if (q.sort_by_score && !under_not && !lvs[k].empty && (lvs[k].scored || lvs[k].substring))
          p->score_list.push_back(static_cast<uint32_t>(k));
        return;
      }
      if (nd.children.empty() || (nd.type == query::NodeType::NOT && nd.children.size() != 1)) {
        bad = true;
        return;
      }
      for (const auto& c : nd.children) walk(*c, under_not || nd.type == query::NodeType::NOT);
      const uint32_t op = nd.type == query::NodeType::AND ? MGX_EXPR_AND
                          : nd.type == query::NodeType::OR ? MGX_EXPR_OR
                                                           : MGX_EXPR_NOT;
      p->expr.push_back(mgx_expr_token{op, static_cast<uint32_t>(nd.children.size())});
    };
    walk(*q.ast, false);
    if (bad || leaves.empty() || leaves.size() > MGX_MAX_TERMS)
      return Fail(p, ErrorCode::kInvalidArgument, "malformed expression tree");
    p->ids.reserve(leaves.size() + q.not_terms.size());
    for (size_t k = 0; k < tis.size(); ++k) {
      TermInfo& ti = tis[k];
      const Leaf& lf = lvs[k];
      if (lf.substring) {  // a text scan on the device
        p->ids.emplace_back();
        p->texts.push_back(ti.normalized);
        p->terms.push_back(mgx_term{nullptr, 0, 0, 0.0, reinterpret_cast<const uint8_t*>(p->texts.back().data()),
                                    static_cast<uint32_t>(p->texts.back().size())});
        continue;
      }
      // an EMPTY leaf's placeholder; under tree_verify the leaf is a TERM of the absent gram (the empty set) with its text
      if (lf.empty) ti.gram_ids.assign(1, tree_verify ? MGX_GRAM_ABSENT : 0u);
      p->ids.push_back(ti.gram_ids);
      mgx_term mt{p->ids.back().data(), static_cast<uint32_t>(p->ids.back().size()), lf.threshold, 0.0, nullptr, 0};
      bool with_text = tree_verify && !ti.normalized.empty();
      if (q.sort_by_score && !lf.empty && lf.scored) {
        // (with the text attached for the filter a single-gram term is scored from its text, like a FUZZY verify_text
        // term: tf = CountTermOccurrences, which its gram's tf column holds, and df = its posting count, the same idf)
        if (ti.is_gram) mt.idf = index::BM25Scorer::ComputeIDF(total_docs, ti.df);
        else with_text = true;  // tf / df from the text on the device
      }
      if (with_text) {
        p->texts.push_back(ti.normalized);
        mt.text = reinterpret_cast<const uint8_t*>(p->texts.back().data());
        mt.text_len = static_cast<uint32_t>(p->texts.back().size());
      }
      p->terms.push_back(mt);
    }
    if (!add_not_terms()) return;
    if (!add_filters()) return;
    // (NOT universe = added ids: a table with gaps carries its exists bitmap as the device index's live row)
    finish(q.sort_by_score ? MGX_SORT_SCORE : MGX_SORT_DOCID);
    p->q.offset = q.sort_by_score ? q.offset : 0;
    p->q.expr = p->expr.data();
    p->q.n_expr = static_cast<uint32_t>(p->expr.size());
    if (tree_verify) (fz != 0 ? p->q.fuzzy_verify_distance : p->q.exact_text) = fz != 0 ? fz : 1u;
    return;
  }
  if (q.terms.empty() || q.terms.size() > MGX_MAX_TERMS || q.not_terms.size() > MGX_MAX_TERMS)
    return Fail(p, ErrorCode::kInvalidArgument, "query needs 1..64 terms");
  if (q.fuzzy_max_distance > 0) {
    // ---- ExecuteWithFuzzy (search_pipeline.cpp:1659-1744): no size sort; theta per term; unknown grams are skipped by
    // Index::SearchByThreshold (index.cpp:512-523) unless theta asks for every gram (then it is SearchAnd) ------------
    p->ids.reserve(q.terms.size() + q.not_terms.size());
    p->has_score_list = q.sort_by_score;
    for (const auto& raw : q.terms) {
      const std::string normalized = index.NormalizeText(raw);
      auto grams = GenerateQueryNgrams(normalized, index.GetNgramSize(), im->query_kanji, index.GetCrossBoundaryNgrams());
      DeduplicateSorted(grams);
      if (grams.empty()) {  // :1676-1682
        p->empty_term_detected = true;
        return;
      }
      size_t n_eff = index.GetNgramSize() > 0 ? static_cast<size_t>(index.GetNgramSize()) : 2;  // :1685-1698
      if (im->query_kanji > 0) {
        size_t short_count = 0;
        for (const auto& g : grams) short_count += g.size() <= 3 ? 1 : 0;
        if (short_count > grams.size() / 2) n_eff = static_cast<size_t>(im->query_kanji);
      }
      const size_t drop = static_cast<size_t>(q.fuzzy_max_distance) * n_eff;  // :1700-1703
      const size_t theta = grams.size() > drop ? grams.size() - drop : 1;
      IdVec known;
      for (const auto& g : grams) {
        uint32_t id = 0;
        uint64_t ps = 0;
        if (im->Resolve(g, &id, &ps) && ps > 0) known.push_back(id);
      }
      const bool empty = theta == grams.size() ? known.size() != grams.size() : known.size() < theta;
      if (empty || known.empty()) known.assign(1, MGX_GRAM_ABSENT);  // the empty doc set, as an operand
      p->ids.push_back(std::move(known));
      const auto& ids = p->ids.back();
      const uint32_t thr = (empty || theta >= ids.size()) ? 0u : static_cast<uint32_t>(theta);
      mgx_term mt{ids.data(), static_cast<uint32_t>(ids.size()), thr, 0.0, nullptr, 0};
      // SORT _score: the EXACT term is scored (GenerateTermInfos' infos, search_pipeline.cpp:1895-1899 ->
      // search_handler.cpp:428-456). A term with an unknown n-gram occurs in no text (tf = df = 0): left out.
      bool with_text = q.verify_text;  // PostFilterByFuzzyText (:1722-1731, :1746-1755) checks every normalized term
      if (q.sort_by_score && !empty && ids.size() == grams.size()) {
        p->score_list.push_back(static_cast<uint32_t>(p->terms.size()));
        if (grams.size() == 1 && grams[0] == normalized) {
          uint32_t gid = 0;
          uint64_t ps = 0;
          im->Resolve(grams[0], &gid, &ps);
          // (with the text attached for the filter the term is scored from its text: tf = CountTermOccurrences, which
          // is what its gram's tf column holds, and df = its posting count, the same idf)
          mt.idf = index::BM25Scorer::ComputeIDF(total_docs, ps);
        } else {
          with_text = true;
        }
      }
      if (with_text) {
        p->texts.push_back(normalized);
        mt.text = reinterpret_cast<const uint8_t*>(p->texts.back().data());
        mt.text_len = static_cast<uint32_t>(p->texts.back().size());
      }
      p->terms.push_back(mt);
    }
    if (!add_not_terms()) return;
    if (!add_filters()) return;
    finish(q.sort_by_score ? MGX_SORT_SCORE : MGX_SORT_DOCID);
    p->q.offset = q.sort_by_score ? q.offset : 0;
    p->q.fuzzy_verify_distance = q.verify_text ? q.fuzzy_max_distance : 0u;
    return;
  }
  std::vector<TermInfo>& tis = p->tis;
  tis.reserve(q.terms.size());
  for (const auto& t : q.terms) tis.push_back(MakeInfo(index, im, t));
  // search_pipeline.cpp:2012-2014 (std::sort on <=16 elements is an insertion sort: equal keys keep their order)
  // (a stable insertion sort by hand: std::stable_sort asks the heap for a merge buffer on every call, and this runs a
  // million times a second)
  for (size_t i = 1; i < tis.size(); ++i)
    for (size_t j = i; j > 0 && tis[j].estimated_size < tis[j - 1].estimated_size; --j) std::swap(tis[j], tis[j - 1]);
  for (const auto& ti : tis)  // Execute :804-810
    if ((ti.estimated_size == 0 || ti.estimated_size == UINT64_MAX) && (ti.n_grams != 0 || ti.normalized.empty())) {
      p->empty_term_detected = true;
      return;
    }
  p->ids.reserve(q.terms.size() + q.not_terms.size());
  // exact-text post-filter: the caller's verify_text decision, or a mixed-script term with an uncovered fragment
  // (search_pipeline.cpp:856-866)
  bool exact = q.verify_text;
  for (const auto& ti : tis)
    exact = exact || HasUncoveredHybridFragment(ti.normalized, index.GetNgramSize(), im->query_kanji,
                                                index.GetCrossBoundaryNgrams());
  for (auto& ti : tis) {
    p->ids.push_back(std::move(ti.gram_ids));  // (the plan owns the ids from here on: no copy)
    mgx_term mt{p->ids.back().data(), static_cast<uint32_t>(p->ids.back().size()), 0, 0.0, nullptr, 0};
    if (q.sort_by_score && ti.is_gram) mt.idf = index::BM25Scorer::ComputeIDF(total_docs, ti.df);
    // (a term shorter than one n-gram has no grams at all: the device scans the texts for it, SearchNormalizedSubstring)
    if (exact || ti.n_grams == 0 || (q.sort_by_score && !ti.is_gram)) {
      p->texts.push_back(ti.normalized);
      mt.text = reinterpret_cast<const uint8_t*>(p->texts.back().data());
      mt.text_len = static_cast<uint32_t>(p->texts.back().size());
    }
    p->terms.push_back(mt);
  }
  if (!add_not_terms()) return;
  if (!add_filters()) return;
  finish(q.sort_by_score ? MGX_SORT_SCORE : MGX_SORT_DOCID);
  p->q.offset = q.offset;
  p->q.exact_text = exact ? 1u : 0u;
}

// results of one fetched batch -> BatchResult objects, in the order the queries were given
void Collect(const std::vector<PlannedQuery>& plans, const mgx_result_view& v, std::vector<BatchResult>* out,
             const mgx_result_view* delta_view = nullptr) {
  out->resize(plans.size());  // (elements a caller hands back keep their vectors' storage: WaitInto)
  size_t k = 0;
  for (size_t qi = 0; qi < plans.size(); ++qi) {
    BatchResult& o = (*out)[qi];
    o.results.clear();
    o.scores.clear();
    o.total = 0;
    o.total_candidates = o.after_intersection = o.after_not = o.after_filters = 0;
    o.empty_term_detected = false;
    o.snippets.clear();
    o.facets.clear();
    o.documents.clear();
    o.document_words.clear();
    o.document_null_masks.clear();
    if (!plans[qi].on_device) {
      o.empty_term_detected = plans[qi].empty_term_detected;
      continue;
    }
    const mgx_query_result& r = v.queries[k];
    o.total = r.total;
    o.total_candidates = r.total_candidates;
    o.after_intersection = r.after_intersection;
    o.after_not = r.after_not;
    o.after_filters = r.after_filters;
    if (delta_view != nullptr && delta_view->queries != nullptr) {
      // a mutable table: page and total were merged on the device; the funnel counters are each index's own
      const mgx_query_result& d = delta_view->queries[k];
      o.total_candidates += d.total_candidates;
      o.after_intersection += d.after_intersection;
      o.after_not += d.after_not;
      o.after_filters += d.after_filters;
    }
    ++k;
    o.results.assign(v.docs + r.docs_begin, v.docs + r.docs_begin + r.n_docs);
    o.scores.assign(v.scores + r.docs_begin, v.scores + r.docs_begin + r.n_docs);
  }
}

// ---- HIGHLIGHT -------------------------------------------------------------------------------------------------------
// The requests of one batch's device queries (mgx_batch_set_highlight) and everything they point at.
struct HighlightRequests {
  std::vector<mgx_highlight_request> reqs;
  std::vector<std::vector<std::string>> terms;
  std::vector<std::vector<const uint8_t*>> ptrs;
  std::vector<std::vector<uint32_t>> lens;
};

bool AnyHighlight(const std::vector<BatchQuery>& queries) {
  for (const auto& q : queries)
    if (q.highlight) return true;
  return false;
}

void CollectScoringLeaves(const query::QueryNode& node, bool under_not, std::vector<std::string>* out) {
  // CollectAstScoringTerms, search_pipeline.cpp:232-254
  if (node.type == query::NodeType::TERM) {
    if (!under_not) out->push_back(node.term);
    return;
  }
  for (const auto& c : node.children)
    if (c) CollectScoringLeaves(*c, under_not || node.type == query::NodeType::NOT, out);
}

// The reference's all_search_terms of a query through BuildHighlightTerms.
std::vector<std::string> HighlightTermsOf(const BatchQuery& q, const index::Index& index) {
  std::vector<std::string> all;
  if (q.ast) CollectScoringLeaves(*q.ast, false, &all);
  all.insert(all.end(), q.terms.begin(), q.terms.end());
  return BuildHighlightTerms(all, &index);
}

// After prepare / reset and before the execute. `delta`: the table's delta index (its texts can be the longest).
Error AttachHighlight(const index::Index& index, const index::Index* delta, const std::vector<BatchQuery>& queries,
                    const std::vector<PlannedQuery>& plans, mgx_batch* batch, HighlightRequests* h) {
  h->reqs.clear();
  if (!AnyHighlight(queries)) return Error{ErrorCode::kSuccess, ""};
  size_t n_dev = 0;
  for (const auto& p : plans) n_dev += p.on_device ? 1 : 0;
  h->reqs.assign(n_dev, mgx_highlight_request{});
  h->terms.resize(n_dev);
  h->ptrs.resize(n_dev);
  h->lens.resize(n_dev);
  size_t k = 0;
  for (size_t qi = 0; qi < queries.size(); ++qi) {
    if (!plans[qi].on_device) continue;
    const BatchQuery& q = queries[qi];
    const size_t at = k++;
    if (!q.highlight) continue;
    h->terms[at] = HighlightTermsOf(q, index);
    h->ptrs[at].clear();
    h->lens[at].clear();
    for (const std::string& t : h->terms[at]) {
      h->ptrs[at].push_back(reinterpret_cast<const uint8_t*>(t.data()));
      h->lens[at].push_back(static_cast<uint32_t>(t.size()));
    }
    mgx_highlight_request& r = h->reqs[at];
    r.enabled = 1;
    r.snippet_length = q.highlight->snippet_length;
    r.max_fragments = q.highlight->max_fragments;
    r.n_terms = static_cast<uint32_t>(h->terms[at].size());
    r.terms = h->ptrs[at].data();
    r.term_lens = h->lens[at].data();
    if (q.highlight->open_tag.size() > 256 || q.highlight->close_tag.size() > 256)  // query_parser.h:276
      return MakeError(ErrorCode::kOutOfRange, "highlight: a tag is at most 256 bytes");
  }
  uint32_t longest = 0, dl = 0;  // over both texts of both indexes
  (void)mgx_index_max_text_bytes(index.impl()->dev, &longest);
  (void)mgx_index_max_original_text_bytes(index.impl()->dev, &dl);
  longest = std::max(longest, dl);
  if (delta != nullptr && delta->impl()->dev != nullptr) {
    (void)mgx_index_max_text_bytes(delta->impl()->dev, &dl);
    longest = std::max(longest, dl);
    (void)mgx_index_max_original_text_bytes(delta->impl()->dev, &dl);
    longest = std::max(longest, dl);
  }
  int rc = mgx_batch_set_highlight(batch, h->reqs.data(), static_cast<uint32_t>(h->reqs.size()), longest);
  // (with a delta the page is final only after mgx_batch_merge_local: the kernel runs once, there)
  if (rc == MGX_OK && delta != nullptr) rc = mgx_batch_defer_highlight(batch, 1);
  return rc == MGX_OK ? Error{ErrorCode::kSuccess, ""} : MakeError(static_cast<ErrorCode>(rc), mgx_last_error());
}

// After mgx_batch_fetch: the snippets of the highlighted queries' pages (the host adds tags and "...").
// A document whose original is not valid UTF-8 is on the device without it: its entries are rendered here, from the
// table's own copy, as the reference renders them (Highlighter::GenerateOriginal).
int CollectSnippets(const index::Index& index, const std::vector<BatchQuery>& queries, const std::vector<PlannedQuery>& plans,
                    mgx_batch* batch, const mgx_result_view& v, std::vector<BatchResult>* out) {
  if (!AnyHighlight(queries) || batch == nullptr || v.queries == nullptr) return MGX_OK;
  std::map<DocId, std::string> on_host;
  {
    index::Index::Impl* im = index.impl();
    std::lock_guard<std::mutex> lock(im->mu);
    if (!im->invalid_originals.empty())  // (the common case: nothing is copied)
      for (DocId d : im->invalid_originals) on_host.emplace(d, im->originals[d]);
  }
  mgx_highlight_view hv{};
  int rc = mgx_batch_fetch_highlight(batch, &hv);
  if (rc != MGX_OK) return rc;
  size_t k = 0;
  for (size_t qi = 0; qi < plans.size(); ++qi) {
    if (!plans[qi].on_device) continue;
    const mgx_query_result& r = v.queries[k++];
    if (!queries[qi].highlight) continue;
    const query::HighlightOptions& o = *queries[qi].highlight;
    std::vector<std::string>& sn = (*out)[qi].snippets;
    sn.resize(r.n_docs);  // (strings a caller hands back keep their storage: WaitInto)
    for (uint32_t j = 0; j < r.n_docs; ++j) {
      const mgx_highlight_entry& e = hv.entries[r.docs_begin + j];
      const size_t cap = e.n_bytes + static_cast<size_t>(e.n_spans) * (o.open_tag.size() + o.close_tag.size()) +
                         3 * (static_cast<size_t>(e.n_windows) + 1);
      sn[j].resize(cap);
      size_t len = 0;
      rc = mgx_highlight_render(&e, reinterpret_cast<const uint8_t*>(o.open_tag.data()), o.open_tag.size(),
                                reinterpret_cast<const uint8_t*>(o.close_tag.data()), o.close_tag.size(),
                                reinterpret_cast<uint8_t*>(sn[j].data()), cap, &len);
      if (rc != MGX_OK) return rc;
      sn[j].resize(std::min(len, cap));
      if (!on_host.empty()) {
        const auto it = on_host.find(v.docs[r.docs_begin + j]);
        if (it != on_host.end())
          sn[j] = query::Highlighter::GenerateOriginal(it->second, HighlightTermsOf(queries[qi], index),
                                                       [&](std::string_view t) { return index.NormalizeText(t); }, o).snippet;
      }
    }
  }
  return MGX_OK;
}

// The counts of a mutable table's two indexes meet by value, not by per-index id: (dict, counts) of the main index (found:
// it has the column) and of the delta -> the merged pair, values ascending.
void MergeFacetValues(bool* found, std::vector<storage::FilterValue>* dict, std::vector<uint64_t>* counts,
                      const std::vector<storage::FilterValue>& ddict, const std::vector<uint64_t>& dcounts) {
  std::vector<storage::FilterValue> merged;
  std::vector<uint64_t> mcounts;
  size_t i = 0, j = 0;
  const size_t ni = *found ? dict->size() : 0;
  while (i < ni || j < ddict.size()) {
    if (j == ddict.size() || (i < ni && (*dict)[i] < ddict[j])) {
      merged.push_back((*dict)[i]);
      mcounts.push_back((*counts)[i]);
      ++i;
    } else if (i == ni || ddict[j] < (*dict)[i]) {
      merged.push_back(ddict[j]);
      mcounts.push_back(dcounts[j]);
      ++j;
    } else {
      merged.push_back((*dict)[i]);
      mcounts.push_back((*counts)[i] + dcounts[j]);
      ++i;
      ++j;
    }
  }
  dict->swap(merged);
  counts->swap(mcounts);
  *found = true;
}

Error FacetColumnNotFound(const std::string& column) {  // search_pipeline.cpp:2089-2092
  return MakeError(ErrorCode::kIndexNotFound, "Facet column \"" + column + "\" not found");
}

// The values with a non-zero count, count descending (:307), then offset and limit (:2141-2148).
void PageFacetValues(const std::vector<storage::FilterValue>& dict, const std::vector<uint64_t>& counts, uint32_t limit,
                     uint32_t offset, FacetOutput* out) {
  std::vector<size_t> order;
  for (size_t v = 0; v < dict.size(); ++v)
    if (counts[v] > 0) order.push_back(v);
  std::stable_sort(order.begin(), order.end(), [&](size_t a, size_t b) { return counts[a] > counts[b]; });
  out->total_values = order.size();
  const size_t first = std::min<size_t>(offset, order.size());
  const size_t last = std::min<size_t>(order.size(), first + static_cast<size_t>(limit));
  for (size_t k = first; k < last; ++k) {
    out->value_counts.emplace_back(storage::SerializeFilterValue(dict[order[k]]), counts[order[k]]);
    out->display.push_back(storage::FilterValueToDisplayString(dict[order[k]]));
  }
}

// ---- page documents ---------------------------------------------------------------------------------------------------
// The requests of one batch's device queries (mgx_batch_set_documents), the ids they point at and the column names the
// ids stand for (the same list for the main index's batch and the delta's).
struct DocumentRequests {
  std::vector<mgx_document_request> reqs;
  std::vector<std::vector<uint32_t>> ids;
  std::vector<std::vector<std::string>> names;
};

bool AnyDocuments(const std::vector<BatchQuery>& queries) {
  for (const auto& q : queries)
    if (q.return_documents) return true;
  return false;
}

// BatchQuery::document_columns, or every filter column of the table: the main index's, then those only the delta holds.
std::vector<std::string> DocumentColumnsOf(const index::Index& index, const index::Index* delta, const BatchQuery& q) {
  if (!q.document_columns.empty()) return q.document_columns;
  std::vector<std::string> names;
  for (const index::Index* ix : {&index, delta}) {
    if (ix == nullptr) continue;
    const index::Index::Impl* im = ix->impl();
    std::lock_guard<std::mutex> lock(im->filter_mu);
    for (const auto& c : im->filter_columns)
      if (std::find(names.begin(), names.end(), c.name) == names.end()) names.push_back(c.name);
  }
  return names;
}

// The table's raw key bytes on the device, by doc slot, for every index of the table that does not hold them yet: the
// first batch that asks for documents, and again after a delta rebuild or Compact() made a new device index.
Error EnsureKeyBytes(const index::Index& index, const index::Index* delta) {
  index::Index::Impl* im = index.impl();
  std::lock_guard<std::mutex> lock(im->mu);
  auto attach = [&](index::Index::Impl* target, uint64_t n, auto doc_of) -> std::string {
    const std::map<DocId, std::string>& keys = im->primary_keys;  // (the table's: a delta's documents are in it too)
    if (keys.empty()) {
      // a table that was given no keys here (an adopted device index): what its owner attached through the C ABI stays
      // (the gather of no ids succeeds exactly when the index holds key bytes)
      uint8_t* none = nullptr;
      uint64_t stride = 0;
      if (mgx_documents_gather(target->dev, nullptr, nullptr, 0, 0, nullptr, nullptr, 0, &none, &stride) == MGX_OK) {
        target->pk_bytes_dev = target->dev;
        return "";
      }
    }
    std::vector<uint8_t> bytes, has(n, 0);
    std::vector<uint64_t> off(n + 1, 0);
    auto it = n ? keys.lower_bound(doc_of(0)) : keys.end();
    for (uint64_t slot = 0; slot < n; ++slot) {
      const DocId doc = doc_of(slot);
      while (it != keys.end() && it->first < doc) ++it;
      if (it != keys.end() && it->first == doc) {
        bytes.insert(bytes.end(), it->second.begin(), it->second.end());
        has[slot] = 1;
      }
      off[slot + 1] = bytes.size();
    }
    bytes.push_back(0);  // (an address even when every key is empty)
    if (mgx_index_attach_primary_key_bytes(target->dev, bytes.data(), off.data(), has.data()) != MGX_OK) return mgx_last_error();
    target->pk_bytes_dev = target->dev;
    return "";
  };
  std::string err;
  if (im->pk_bytes_dev != im->dev) {
    const DocId first = im->view.first_doc_id;
    err = attach(im, im->view.n_docs, [first](uint64_t slot) { return first + static_cast<DocId>(slot); });
  }
  if (err.empty() && delta != nullptr) {
    index::Index::Impl* dim = delta->impl();
    if (dim->pk_bytes_dev != dim->dev) {
      // (the delta's own doc map: the table may have built a newer delta since the batch took this one; the keys are the
      // table's current ones, so a document removed in between has none)
      const std::vector<DocId>& ids = dim->doc_map_ids;
      if (ids.size() != dim->view.n_docs)
        return MakeError(ErrorCode::kInternalError, "page documents: the delta index holds no doc map");
      err = attach(dim, ids.size(), [&ids](uint64_t slot) { return ids[slot]; });
    }
  }
  return err.empty() ? Error{ErrorCode::kSuccess, ""} : MakeError(ErrorCode::kInternalError, err);
}

Error DocumentColumnNotFound(const std::string& column) {
  return MakeError(ErrorCode::kIndexNotFound, "Document column \"" + column + "\" not found");
}

// After prepare / reset and before the execute, once for the main index's batch (`own` = the main index) and once for
// the delta's (`own` = the delta): the same names, each batch with its own index's column ids; a column the own index
// does not hold is MGX_DOC_NO_COLUMN. `plans`: those of `batch`.
Error AttachDocuments(const index::Index& index, const index::Index* delta, const index::Index& own,
                      const std::vector<BatchQuery>& queries, const std::vector<PlannedQuery>& plans, mgx_batch* batch,
                      DocumentRequests* d) {
  d->reqs.clear();
  if (!AnyDocuments(queries)) return Error{ErrorCode::kSuccess, ""};
  index.FlushPendingFilterColumns();
  {
    const Error e = EnsureKeyBytes(index, delta);
    if (e.code() != ErrorCode::kSuccess) return e;
  }
  size_t n_dev = 0;
  for (const auto& p : plans) n_dev += p.on_device ? 1 : 0;
  d->reqs.assign(n_dev, mgx_document_request{});
  d->ids.resize(n_dev);
  d->names.resize(n_dev);
  size_t k = 0;
  for (size_t qi = 0; qi < queries.size(); ++qi) {
    if (!plans[qi].on_device) continue;
    const BatchQuery& q = queries[qi];
    const size_t at = k++;
    if (!q.return_documents) continue;
    d->names[at] = DocumentColumnsOf(index, delta, q);
    d->ids[at].clear();
    for (const std::string& name : d->names[at]) {
      bool known = false;
      uint32_t id = MGX_DOC_NO_COLUMN;
      for (const index::Index* ix : {&index, delta}) {
        if (ix == nullptr) continue;
        const index::Index::Impl* im = ix->impl();
        std::lock_guard<std::mutex> lock(im->filter_mu);
        const index::Index::Impl::FilterColumn* col = im->ResolveColumn(name);
        if (col == nullptr) continue;
        known = true;
        if (ix == &own) id = col->device_id;
      }
      if (!known) return DocumentColumnNotFound(name);
      d->ids[at].push_back(id);
    }
    mgx_document_request& r = d->reqs[at];
    r.enabled = 1;
    r.n_columns = static_cast<uint32_t>(d->ids[at].size());
    r.column_ids = d->ids[at].data();
  }
  uint32_t longest = 0, dl = 0;  // over both indexes: the merged page's records hold either's keys
  (void)mgx_index_max_primary_key_bytes(index.impl()->dev, &longest);
  if (delta != nullptr && delta->impl()->dev != nullptr) {
    (void)mgx_index_max_primary_key_bytes(delta->impl()->dev, &dl);
    longest = std::max(longest, dl);
  }
  int rc = mgx_batch_set_documents(batch, d->reqs.data(), static_cast<uint32_t>(d->reqs.size()), longest);
  // (with a delta the page is final only after mgx_batch_merge_local: the kernel runs once, there or in the fetch)
  if (rc == MGX_OK && delta != nullptr) rc = mgx_batch_defer_documents(batch, 1);
  return rc == MGX_OK ? Error{ErrorCode::kSuccess, ""} : MakeError(static_cast<ErrorCode>(rc), mgx_last_error());
}

// After mgx_batch_fetch: BatchResult::documents of the requesting queries' pages. A value comes back in its column's own
// type, a string through the dictionary of the index the row came from (MGX_DOC_MAPPED: the delta).
int CollectDocuments(const index::Index& index, const index::Index* delta, const std::vector<BatchQuery>& queries,
                     const std::vector<PlannedQuery>& plans, mgx_batch* batch, const mgx_result_view& v,
                     const DocumentRequests& d, std::vector<BatchResult>* out) {
  if (!AnyDocuments(queries) || batch == nullptr || v.queries == nullptr) return MGX_OK;
  mgx_document_view dv{};
  const int rc = mgx_batch_fetch_documents(batch, &dv);
  if (rc != MGX_OK) return rc;
  const index::Index::Impl* im = index.impl();
  const index::Index::Impl* dim = delta != nullptr ? delta->impl() : nullptr;
  std::unique_lock<std::mutex> ml(im->filter_mu), dl;
  if (dim != nullptr) dl = std::unique_lock<std::mutex>(dim->filter_mu);
  std::vector<const index::Index::Impl::FilterColumn*> mcols, dcols;
  size_t k = 0;
  for (size_t qi = 0; qi < plans.size(); ++qi) {
    if (!plans[qi].on_device) continue;
    const size_t at = k;
    const mgx_query_result& r = v.queries[k++];
    if (!queries[qi].return_documents) continue;
    const std::vector<std::string>& names = d.names[at];
    mcols.assign(names.size(), nullptr);
    dcols.assign(names.size(), nullptr);
    for (size_t c = 0; c < names.size(); ++c) {
      mcols[c] = im->ResolveColumn(names[c]);
      if (dim != nullptr) dcols[c] = dim->ResolveColumn(names[c]);
    }
    std::vector<std::optional<storage::Document>>& docs = (*out)[qi].documents;
    docs.assign(r.n_docs, std::nullopt);
    const bool raw = !queries[qi].document_columns.empty();  // (the caller named the columns: their words by position)
    std::vector<uint64_t>& words = (*out)[qi].document_words;
    std::vector<uint32_t>& masks = (*out)[qi].document_null_masks;
    if (raw) {
      words.assign(static_cast<size_t>(r.n_docs) * names.size(), 0);
      masks.assign(r.n_docs, names.size() >= 32 ? 0xFFFFFFFFu : (1u << names.size()) - 1u);
    }
    for (uint32_t j = 0; j < r.n_docs; ++j) {
      const mgx_document_entry& e = dv.entries[r.docs_begin + j];
      if ((e.flags & MGX_DOC_FOUND) == 0) continue;
      if (raw) {
        masks[j] = e.null_mask;
        for (uint32_t c = 0; c < e.n_columns && c < names.size(); ++c) words[j * names.size() + c] = e.values[c];
      }
      storage::Document doc;
      doc.doc_id = v.docs[r.docs_begin + j];
      if (e.flags & MGX_DOC_HAS_KEY) doc.primary_key.assign(reinterpret_cast<const char*>(e.key), e.key_len);
      const auto& cols = (e.flags & MGX_DOC_MAPPED) ? dcols : mcols;
      for (uint32_t c = 0; c < e.n_columns && c < cols.size(); ++c) {
        if (((e.null_mask >> c) & 1u) != 0 || cols[c] == nullptr || cols[c]->type == 0) continue;
        doc.filters[cols[c]->name] = index::FilterValueFromBits(cols[c]->type, e.values[c], cols[c]->dict);
      }
      docs[j] = std::move(doc);
    }
  }
  return MGX_OK;
}

// ---- FACET in a batch -------------------------------------------------------------------------------------------------
// The requests of one batch's device queries (mgx_batch_set_facets) and the ids they point at.
struct FacetRequests {
  std::vector<mgx_facet_request> reqs;
  std::vector<std::vector<uint32_t>> ids;
};

bool AnyFacets(const std::vector<BatchQuery>& queries) {
  for (const auto& q : queries)
    if (!q.facet_columns.empty()) return true;
  return false;
}

// A facet column must exist in the table: in the main index or, on a table with a delta, in the delta (ExecuteFacet's rule).
Error CheckFacetColumns(const std::vector<BatchQuery>& queries, const std::vector<PlannedQuery>& plans,
                        const std::vector<PlannedQuery>* dplans) {
  for (size_t qi = 0; qi < plans.size(); ++qi) {
    if (!plans[qi].faceted) continue;
    for (size_t c = 0; c < plans[qi].facets.size(); ++c) {
      const bool in_delta = dplans != nullptr && c < (*dplans)[qi].facets.size() && (*dplans)[qi].facets[c].found;
      if (!plans[qi].facets[c].found && !in_delta) return FacetColumnNotFound(queries[qi].facet_columns[c]);
    }
  }
  return Error{ErrorCode::kSuccess, ""};
}

// After prepare / reset and before the execute, next to the highlight requests; `plans` are those the batch was compiled
// from (the main index's, or the delta's for the delta's batch). A column this index does not hold is left out.
Error AttachFacets(const std::vector<PlannedQuery>& plans, mgx_batch* batch, FacetRequests* f) {
  f->reqs.clear();
  size_t n_dev = 0;
  bool any = false;
  for (const auto& p : plans) {
    n_dev += p.on_device ? 1 : 0;
    any = any || (p.on_device && p.faceted);
  }
  if (!any) return Error{ErrorCode::kSuccess, ""};
  f->reqs.assign(n_dev, mgx_facet_request{});
  f->ids.resize(n_dev);
  size_t k = 0;
  for (const auto& p : plans) {
    if (!p.on_device) continue;
    const size_t at = k++;
    f->ids[at].clear();
    if (!p.faceted) continue;
    for (const auto& c : p.facets)
      if (c.found) f->ids[at].push_back(c.device_id);
    f->reqs[at].n_columns = static_cast<uint32_t>(f->ids[at].size());
    f->reqs[at].column_ids = f->ids[at].data();
  }
  const int rc = mgx_batch_set_facets(batch, f->reqs.data(), static_cast<uint32_t>(f->reqs.size()));
  return rc == MGX_OK ? Error{ErrorCode::kSuccess, ""} : MakeError(static_cast<ErrorCode>(rc), mgx_last_error());
}

// After mgx_batch_fetch (of both batches on a table with a delta) and Collect: BatchResult::facets of the faceted queries,
// what ExecuteFacet returns per column. batch / dbatch: nullptr when no query reached the device.
Error CollectFacets(const std::vector<BatchQuery>& queries, const std::vector<PlannedQuery>& plans,
                  const std::vector<PlannedQuery>* dplans, mgx_batch* batch, mgx_batch* dbatch,
                  std::vector<BatchResult>* out) {
  if (!AnyFacets(queries)) return Error{ErrorCode::kSuccess, ""};
  mgx_facet_view fv{}, dfv{};
  int rc = batch != nullptr ? mgx_batch_fetch_facets(batch, &fv) : MGX_OK;
  if (rc == MGX_OK && dbatch != nullptr) rc = mgx_batch_fetch_facets(dbatch, &dfv);
  if (rc != MGX_OK) return MakeError(static_cast<ErrorCode>(rc), mgx_last_error());
  uint32_t e = 0, de = 0, k = 0;  // the next entry of each view; the device query's position in its batch
  // the counts of column c of one index's plan, by that index's value ids
  auto take = [](const PlannedQuery& p, size_t c, const mgx_facet_view& view, uint32_t* next, uint32_t dev_query,
                 std::vector<uint64_t>* counts) {
    const PlannedQuery::FacetColumn& col = p.facets[c];
    counts->assign(std::max<size_t>(col.dict.size(), 1), 0);
    if (!p.on_device || !col.found) return true;
    if (*next >= view.n_entries) return false;
    const mgx_facet_entry& en = view.entries[(*next)++];
    if (en.query != dev_query || en.column_id != col.device_id) return false;
    for (uint32_t v = 0; v < en.n_values && v < counts->size(); ++v) (*counts)[v] = en.counts[v];
    return true;
  };
  for (size_t qi = 0; qi < plans.size(); ++qi) {
    const PlannedQuery& p = plans[qi];
    if (p.faceted) {
      const PlannedQuery* d = dplans != nullptr ? &(*dplans)[qi] : nullptr;
      BatchResult& o = (*out)[qi];
      o.results.clear();  // (counts, not a page)
      o.scores.clear();
      o.facets.resize(p.facets.size());
      for (size_t c = 0; c < p.facets.size(); ++c) {
        std::vector<uint64_t> counts, dcounts;
        if (!take(p, c, fv, &e, k, &counts) || (d != nullptr && !take(*d, c, dfv, &de, k, &dcounts))) {
          return MakeError(ErrorCode::kInternalError, "the batch's facet entries do not match its requests");
        }
        bool found = p.facets[c].found;
        std::vector<storage::FilterValue> dict = p.facets[c].dict;
        if (d != nullptr && d->facets[c].found) MergeFacetValues(&found, &dict, &counts, d->facets[c].dict, dcounts);
        FacetOutput& fo = o.facets[c];
        fo = FacetOutput{};
        fo.matched_documents = o.total;
        PageFacetValues(dict, counts, queries[qi].limit, queries[qi].offset, &fo);
      }
    }
    if (p.on_device) ++k;
  }
  return Error{ErrorCode::kSuccess, ""};
}
}  // namespace

std::vector<std::string> BuildHighlightTerms(const std::vector<std::string>& search_terms, const index::Index* index) {
  std::vector<std::string> terms;
  terms.reserve(search_terms.size());
  for (const auto& term : search_terms) {
    std::string normalized = index != nullptr ? index->NormalizeText(term) : term;
    if (normalized.empty()) continue;
    terms.push_back(normalized);
    size_t i = 0;
    const auto space = [](char c) { return c == ' ' || (c >= '\t' && c <= '\r'); };  // what `stream >> piece` skips
    while (i < normalized.size()) {
      while (i < normalized.size() && space(normalized[i])) ++i;
      size_t j = i;
      while (j < normalized.size() && !space(normalized[j])) ++j;
      if (j > i && j - i != normalized.size()) terms.push_back(normalized.substr(i, j - i));
      i = j;
    }
  }
  DeduplicateSorted(terms);
  return terms;
}

namespace {
// A mutable table's delta index as the device holds it now (nullptr: none). ApplyMutations has run.
std::shared_ptr<index::Index> DeltaOf(const index::Index& index) {
  index::Index::Impl* im = index.impl();
  std::lock_guard<std::mutex> lock(im->mu);
  return im->mut.delta;
}

// The same query planned against the delta index: must run where the main plan runs (both see table-wide sizes).
bool PlanForDelta(const index::Index& delta, const BatchQuery& q, uint64_t total_docs, double avgdl,
                  const PlannedQuery& main_plan, PlannedQuery* p) {
  if (!q.filters.empty()) {
    Fail(p, ErrorCode::kNotImplemented,
         "BatchQuery::filters (raw bitmap ids) belong to one device index: a table with a delta takes filter_conditions");
    return false;
  }
  PlanQuery(delta, q, total_docs, avgdl, p);
  if (p->error != ErrorCode::kSuccess) return false;
  if (main_plan.sort_string || p->sort_string) {
    Fail(p, ErrorCode::kNotImplemented,
         "SORT by a string column on a table with a delta index is not implemented: the ranks of the two indexes' "
         "dictionaries do not compare (Compact() the table)");
    return false;
  }
  if (p->on_device != main_plan.on_device) {
    Fail(p, ErrorCode::kInternalError, "the main and the delta index plan a query differently");
    return false;
  }
  return true;
}

// df pass + execute of both batches and the merge, all on the main batch's stream
int RunWithDelta(mgx_batch* main_batch, mgx_batch* delta_batch, void* stream) {
  mgx_batch* others[1] = {delta_batch};
  int rc = mgx_batch_df_merge_local(main_batch, others, 1, stream);
  if (rc == MGX_OK) rc = mgx_batch_execute(main_batch, stream);
  if (rc == MGX_OK) rc = mgx_batch_execute(delta_batch, stream);
  if (rc == MGX_OK) rc = mgx_batch_merge_local(main_batch, others, 1, stream);
  return rc;
}
}  // namespace

Expected<std::vector<BatchResult>, Error> ExecuteBatch(const index::Index& index,
                                                       const std::vector<BatchQuery>& queries) {
  index.Finalize();
  index::Index::Impl* im = index.impl();
  if (!im->dev) return MakeUnexpected(MakeError(ErrorCode::kInternalError, im->last_error));
  {
    const std::string merr = index.ApplyMutations();
    if (!merr.empty()) return MakeUnexpected(MakeError(ErrorCode::kInternalError, merr));
  }
  const std::shared_ptr<index::Index> delta = DeltaOf(index);
  const uint64_t total_docs = index.Bm25DocCount();
  const double avgdl = index.Bm25AvgDocLength();
  std::vector<PlannedQuery> plans(queries.size()), dplans(delta ? queries.size() : 0);
  std::vector<mgx_query> mq, dq;
  for (size_t qi = 0; qi < queries.size(); ++qi) {
    PlanQuery(index, queries[qi], total_docs, avgdl, &plans[qi]);
    if (plans[qi].error != ErrorCode::kSuccess)
      return MakeUnexpected(MakeError(plans[qi].error, plans[qi].error_message));
    if (plans[qi].on_device) mq.push_back(plans[qi].q);
    if (delta) {
      if (!PlanForDelta(*delta, queries[qi], total_docs, avgdl, plans[qi], &dplans[qi]))
        return MakeUnexpected(MakeError(dplans[qi].error, dplans[qi].error_message));
      if (dplans[qi].on_device) dq.push_back(dplans[qi].q);
    }
  }
  {
    const Error fe = CheckFacetColumns(queries, plans, delta ? &dplans : nullptr);
    if (fe.code() != ErrorCode::kSuccess) return MakeUnexpected(fe);
  }
  std::vector<BatchResult> out;
  mgx_result_view v{};
  if (mq.empty()) {
    Collect(plans, v, &out);
    const Error fe = CollectFacets(queries, plans, delta ? &dplans : nullptr, nullptr, nullptr, &out);
    if (fe.code() != ErrorCode::kSuccess) return MakeUnexpected(fe);
    return out;
  }
  mgx_batch* batch = nullptr;
  int rc = mgx_batch_prepare(im->dev, mq.data(), static_cast<uint32_t>(mq.size()), &batch);
  if (rc != MGX_OK) return MakeUnexpected(MakeError(static_cast<ErrorCode>(rc), mgx_last_error()));
  std::unique_ptr<mgx_batch, void (*)(mgx_batch*)> guard(batch, mgx_batch_destroy);
  HighlightRequests hreq;
  FacetRequests freq, dfreq;
  DocumentRequests docreq, ddocreq;
  {
    const Error he = AttachHighlight(index, delta.get(), queries, plans, batch, &hreq);
    if (he.code() != ErrorCode::kSuccess) return MakeUnexpected(he);
    const Error fe = AttachFacets(plans, batch, &freq);
    if (fe.code() != ErrorCode::kSuccess) return MakeUnexpected(fe);
    const Error de = AttachDocuments(index, delta.get(), index, queries, plans, batch, &docreq);
    if (de.code() != ErrorCode::kSuccess) return MakeUnexpected(de);
  }
  if (delta) {
    mgx_batch* dbatch = nullptr;
    rc = mgx_batch_prepare(delta->impl()->dev, dq.data(), static_cast<uint32_t>(dq.size()), &dbatch);
    if (rc != MGX_OK) return MakeUnexpected(MakeError(static_cast<ErrorCode>(rc), mgx_last_error()));
    std::unique_ptr<mgx_batch, void (*)(mgx_batch*)> dguard(dbatch, mgx_batch_destroy);
    {
      const Error fe = AttachFacets(dplans, dbatch, &dfreq);  // both batches carry the requests
      if (fe.code() != ErrorCode::kSuccess) return MakeUnexpected(fe);
      const Error de = AttachDocuments(index, delta.get(), *delta, queries, dplans, dbatch, &ddocreq);
      if (de.code() != ErrorCode::kSuccess) return MakeUnexpected(de);
    }
    void* stream = nullptr;
    rc = mgx_batch_stream(batch, &stream);
    if (rc == MGX_OK) rc = RunWithDelta(batch, dbatch, stream);
    if (rc != MGX_OK) return MakeUnexpected(MakeError(static_cast<ErrorCode>(rc), mgx_last_error()));
    mgx_result_view dv{};
    rc = mgx_batch_fetch(batch, &v);
    if (rc == MGX_OK) rc = mgx_batch_fetch(dbatch, &dv);
    if (rc != MGX_OK) return MakeUnexpected(MakeError(static_cast<ErrorCode>(rc), mgx_last_error()));
    Collect(plans, v, &out, &dv);
    rc = CollectSnippets(index, queries, plans, batch, v, &out);
    if (rc == MGX_OK) rc = CollectDocuments(index, delta.get(), queries, plans, batch, v, docreq, &out);
    if (rc != MGX_OK) return MakeUnexpected(MakeError(static_cast<ErrorCode>(rc), mgx_last_error()));
    const Error fe = CollectFacets(queries, plans, &dplans, batch, dbatch, &out);
    if (fe.code() != ErrorCode::kSuccess) return MakeUnexpected(fe);
    return out;
  }
  rc = mgx_batch_execute(batch, nullptr);
  if (rc != MGX_OK) return MakeUnexpected(MakeError(static_cast<ErrorCode>(rc), mgx_last_error()));
  rc = mgx_batch_fetch(batch, &v);
  if (rc != MGX_OK) return MakeUnexpected(MakeError(static_cast<ErrorCode>(rc), mgx_last_error()));
  Collect(plans, v, &out);
  rc = CollectSnippets(index, queries, plans, batch, v, &out);
  if (rc == MGX_OK) rc = CollectDocuments(index, nullptr, queries, plans, batch, v, docreq, &out);
  if (rc != MGX_OK) return MakeUnexpected(MakeError(static_cast<ErrorCode>(rc), mgx_last_error()));
  const Error fe = CollectFacets(queries, plans, nullptr, batch, nullptr, &out);
  if (fe.code() != ErrorCode::kSuccess) return MakeUnexpected(fe);
  return out;
}

namespace {
// FACET over one device index: the column's distinct values (ascending) and how many documents of the query's result set
// hold each. found = false: this index has no such column.
Error FacetOne(const index::Index& index, const BatchQuery& query, const std::string& column, bool* found,
               std::vector<storage::FilterValue>* dict, std::vector<uint64_t>* counts, uint64_t* matched) {
  index.FlushPendingFilterColumns();
  index::Index::Impl* im = index.impl();
  uint32_t device_column = 0;
  *found = false;
  *matched = 0;
  {
    std::lock_guard<std::mutex> lock(im->filter_mu);
    const index::Index::Impl::FilterColumn* col = im->ResolveColumn(column);
    if (col != nullptr) {
      *found = true;
      device_column = col->device_id;
      *dict = col->dict;
    }
  }
  // the search part: the query's own, or — FACET without search terms — every document (GetAllDocIds, :2118) narrowed by
  // its NOT terms and filters: the expression NOT(<empty>) is the universe
  const BatchQuery q = FacetSearchPart(query);
  PlannedQuery plan;
  PlanQuery(index, q, index.Bm25DocCount(), index.Bm25AvgDocLength(), &plan);
  if (plan.error != ErrorCode::kSuccess) return MakeError(plan.error, plan.error_message);
  counts->assign(std::max<size_t>(dict->size(), 1), 0);
  if (plan.on_device && *found) {
    if (mgx_facet_counts(im->dev, &plan.q, device_column, counts->data(), matched) != MGX_OK)
      return MakeError(ErrorCode::kInternalError, mgx_last_error());
  }
  return Error{ErrorCode::kSuccess, ""};
}
}  // namespace

Expected<FacetOutput, Error> ExecuteFacet(const index::Index& index, const BatchQuery& query, const std::string& column) {
  index.Finalize();
  index::Index::Impl* im = index.impl();
  if (!im->dev) return MakeUnexpected(MakeError(ErrorCode::kInternalError, im->last_error));
  {
    const std::string merr = index.ApplyMutations();
    if (!merr.empty()) return MakeUnexpected(MakeError(ErrorCode::kInternalError, merr));
  }
  const std::shared_ptr<index::Index> delta = DeltaOf(index);
  if (delta && !query.filters.empty())
    return MakeUnexpected(MakeError(ErrorCode::kNotImplemented,
                                    "BatchQuery::filters (raw bitmap ids) belong to one device index: a table with a delta takes filter_conditions"));
  bool found = false, dfound = false;
  std::vector<storage::FilterValue> dict, ddict;
  std::vector<uint64_t> counts, dcounts;
  FacetOutput out;
  Error e = FacetOne(index, query, column, &found, &dict, &counts, &out.matched_documents);
  if (e.code() != ErrorCode::kSuccess) return MakeUnexpected(e);
  if (delta) {  // a mutable table: the delta's documents count too; values meet by value, not by per-index id
    uint64_t dmatched = 0;
    e = FacetOne(*delta, query, column, &dfound, &ddict, &dcounts, &dmatched);
    if (e.code() != ErrorCode::kSuccess) return MakeUnexpected(e);
    out.matched_documents += dmatched;
    if (dfound) MergeFacetValues(&found, &dict, &counts, ddict, dcounts);
  }
  if (!found) return MakeUnexpected(FacetColumnNotFound(column));
  PageFacetValues(dict, counts, query.limit, query.offset, &out);
  return out;
}

// ---- BatchExecutor ------------------------------------------------------------------------------------------------
//
// Submit only queues: a pool of workers plans the batch in chunks of queries (several batches at once when several are
// queued); dispatcher threads (three) compile planned batches (mgx_batch_reset: host work, one object per slot) and put
// them on the device strictly in ticket order — on a sharded table each execute is followed by a collective that every
// rank must issue in the same order. Wait blocks until its ticket is on the device, then fetches.

struct BatchExecutor::Impl {
  using clock = std::chrono::steady_clock;
  const index::Index& index;
  Options opt;
  uint64_t total_docs = 0;
  double avgdl = 0.0;
  enum State { kFree, kFilling, kPlanning, kPlanned, kCompiling, kCompiled, kEnqueued, kFailed };
  struct Slot {
    mgx_batch* batch = nullptr;
    std::vector<BatchQuery> queries;
    std::vector<PlannedQuery> plans;
    std::vector<mgx_query> mq;
    // a mutable table: the delta index this batch was submitted against, the same queries planned for it, and the batch
    // object compiled on it (bound to dbatch_index: a rebuilt delta gets a new object)
    std::shared_ptr<index::Index::Impl::Handles> handles;  // the generation of the main index `batch` was compiled on
    std::shared_ptr<index::Index> delta, dbatch_index;
    std::vector<PlannedQuery> dplans;
    std::vector<mgx_query> dq;
    HighlightRequests hreq;  // mgx_batch_set_highlight of this batch (storage re-used from batch to batch)
    FacetRequests freq, dfreq;  // mgx_batch_set_facets of the batch and of the delta's batch
    DocumentRequests docreq, ddocreq;  // mgx_batch_set_documents likewise
    mgx_batch* dbatch = nullptr;
    uint64_t total_docs = 0;  // BM25Stats the batch is planned with (a mutable table's change between batches)
    double avgdl = 0.0;
    uint64_t ticket = 0;
    State state = kFree;
    size_t chunks_left = 0;  // under mu
    Error error{ErrorCode::kSuccess, ""};
    Timing timing;
    clock::time_point t_submit, t_planned, t_compiled;
  };
  struct Chunk {
    Slot* slot;
    size_t begin, end;
  };
  static constexpr size_t kChunk = 64;
  std::vector<Slot> slots;
  uint64_t next_ticket = 1, next_compile = 1, next_enqueue = 1;
  std::vector<std::thread> workers;
  std::vector<std::thread> dispatchers;
  std::mutex mu;  // slots' state, the chunk queue, the enqueue turn
  std::condition_variable cv_work, cv_state;
  std::deque<Chunk> chunks;
  bool stop = false;
  bool enqueuing = false;  // a dispatcher is inside EnqueueReady's loop (guarded by mu)
  // Sharded tables: every rank issues the same collectives in the same order. A rank that cannot (a ticket that failed to
  // plan or compile here, an exchange call that returned an error) has left that lock-step: its peers have enqueued this
  // ticket's all-gather and would pair it with the NEXT ticket's. The communicator is then poisoned: aborted
  // (mgx_comm_abort: this rank's enqueued collectives are cancelled, the peers' fail or time out instead of pairing
  // wrongly), and every later ticket fails at once with the first error — the process is expected to exit non-zero.
  bool comm_poisoned = false;  // guarded by mu
  std::string poison_message;

  Impl(const index::Index& ix, Options o) : index(ix), opt(o) {}

  Slot* ByTicket(uint64_t ticket) {
    for (auto& s : slots)
      if (s.state != kFree && s.state != kFilling && s.ticket == ticket) return &s;
    return nullptr;
  }

  // host side of one batch after planning: the device queries, compiled into the slot's batch object
  void Compile(Slot* slot) {
    index::Index::Impl* im = index.impl();
    static const bool kTrace = std::getenv("MGX_TRACE_HOST") != nullptr;
    const auto t_in = clock::now();
    slot->mq.clear();
    for (const auto& p : slot->plans) {
      if (p.error != ErrorCode::kSuccess) {
        slot->error = MakeError(p.error, p.error_message);
        return;
      }
      if (p.on_device) slot->mq.push_back(p.q);
    }
    slot->timing.device_queries = static_cast<uint32_t>(slot->mq.size());
    slot->dq.clear();
    if (slot->delta) {
      for (const auto& p : slot->dplans) {
        if (p.error != ErrorCode::kSuccess) {
          slot->error = MakeError(p.error, p.error_message);
          return;
        }
        if (p.on_device) slot->dq.push_back(p.q);
      }
    }
    slot->error = CheckFacetColumns(slot->queries, slot->plans, slot->delta ? &slot->dplans : nullptr);
    if (slot->error.code() != ErrorCode::kSuccess) return;
    if (slot->mq.empty()) return;
    if (kTrace) {
      static std::atomic<uint64_t> n{0}, us{0};
      us += std::chrono::duration_cast<std::chrono::microseconds>(clock::now() - t_in).count();
      if (++n % 64 == 0) fprintf(stderr, "[shim] gather of the planned queries: %.3f ms per batch\n", us.exchange(0) / 64e3);
    }
    int rc;
    {
      std::shared_ptr<index::Index::Impl::Handles> cur;
      {
        std::lock_guard<std::mutex> il(im->mu);
        cur = im->handles;
      }
      if (slot->batch && slot->handles != cur) {  // the main index was compacted: the object belongs to the old generation
        mgx_batch_destroy(slot->batch);
        slot->batch = nullptr;
      }
      slot->handles = std::move(cur);
    }
    if (!slot->batch)
      rc = mgx_batch_prepare(im->dev, slot->mq.data(), static_cast<uint32_t>(slot->mq.size()), &slot->batch);
    else
      rc = mgx_batch_reset(slot->batch, slot->mq.data(), static_cast<uint32_t>(slot->mq.size()));
    if (rc != MGX_OK) {
      slot->error = MakeError(static_cast<ErrorCode>(rc), mgx_last_error());
      return;
    }
    slot->error = AttachHighlight(index, slot->delta.get(), slot->queries, slot->plans, slot->batch, &slot->hreq);
    if (slot->error.code() != ErrorCode::kSuccess) return;
    slot->error = AttachFacets(slot->plans, slot->batch, &slot->freq);
    if (slot->error.code() != ErrorCode::kSuccess) return;
    slot->error = AttachDocuments(index, slot->delta.get(), index, slot->queries, slot->plans, slot->batch, &slot->docreq);
    if (slot->error.code() != ErrorCode::kSuccess) return;
    if (slot->dbatch && slot->dbatch_index != slot->delta) {  // the delta index was rebuilt (or went away)
      mgx_batch_destroy(slot->dbatch);
      slot->dbatch = nullptr;
      slot->dbatch_index.reset();
    }
    if (!slot->delta) return;
    if (!slot->dbatch) {
      rc = mgx_batch_prepare(slot->delta->impl()->dev, slot->dq.data(), static_cast<uint32_t>(slot->dq.size()), &slot->dbatch);
      if (rc == MGX_OK) slot->dbatch_index = slot->delta;
    } else {
      rc = mgx_batch_reset(slot->dbatch, slot->dq.data(), static_cast<uint32_t>(slot->dq.size()));
    }
    if (rc != MGX_OK) {
      slot->error = MakeError(static_cast<ErrorCode>(rc), mgx_last_error());
      return;
    }
    slot->error = AttachFacets(slot->dplans, slot->dbatch, &slot->dfreq);
    if (slot->error.code() != ErrorCode::kSuccess) return;
    slot->error = AttachDocuments(index, slot->delta.get(), *slot->delta, slot->queries, slot->dplans, slot->dbatch, &slot->ddocreq);
  }

  // device side, in ticket order. Called with mu held; the HIP calls themselves (they only enqueue, but a batch is a
  // dozen of them: ~0.1 ms) run with mu RELEASED — planners, Submit and Wait all take mu — and `enqueuing` keeps them in
  // one thread at a time: whoever finds it set leaves its batch to that thread, which looks again (under mu) after
  // every batch it has put on the device.
  void EnqueueReady(std::unique_lock<std::mutex>& lock) {
    if (enqueuing) return;
    enqueuing = true;
    for (;;) {
      Slot* slot = ByTicket(next_enqueue);
      if (!slot || (slot->state != kCompiled && slot->state != kFailed)) break;
      if (opt.comm && comm_poisoned && slot->state == kCompiled) {
        slot->error = MakeError(ErrorCode::kInternalError, "the table's communicator was aborted after an earlier failure: " + poison_message);
        slot->state = kFailed;
      } else if (opt.comm && slot->state == kFailed && !comm_poisoned) {
        comm_poisoned = true;  // (this ticket never reached its collectives on this rank)
        poison_message = slot->error.message();
        (void)mgx_comm_abort(opt.comm);
      }
      if (slot->state == kCompiled && !slot->mq.empty()) {
        lock.unlock();
        const auto t0 = clock::now();
        void* stream = nullptr;  // the batch object's own stream: slots overlap on the device
        int rc = mgx_batch_stream(slot->batch, &stream);
        mgx_comm* comm = opt.comm;
        if (rc == MGX_OK && slot->delta) {
          rc = RunWithDelta(slot->batch, slot->dbatch, stream);  // both indexes + the merge, on this one stream
        } else {
          static const bool kTrace = std::getenv("MGX_TRACE_HOST") != nullptr;
          const auto e0 = clock::now();
          if (rc == MGX_OK && comm) rc = mgx_batch_exchange_df(slot->batch, comm, stream);  // table-wide df before idf
          const auto e1 = clock::now();
          if (rc == MGX_OK)                                                                 // asynchronous
            rc = comm ? mgx_batch_execute_sharded(slot->batch, comm, stream) : mgx_batch_execute(slot->batch, stream);
          const auto e2 = clock::now();
          if (rc == MGX_OK && comm) rc = mgx_batch_exchange(slot->batch, comm, stream);     // all-gather + merge
          if (kTrace) {
            static std::atomic<uint64_t> n{0}, a{0}, b{0}, c{0};
            a += std::chrono::duration_cast<std::chrono::nanoseconds>(e1 - e0).count();
            b += std::chrono::duration_cast<std::chrono::nanoseconds>(e2 - e1).count();
            c += std::chrono::duration_cast<std::chrono::nanoseconds>(clock::now() - e2).count();
            if (++n % 64 == 0)
              fprintf(stderr, "[shim] enqueue per batch: exchange_df %.1f us, execute %.1f us, exchange %.1f us\n",
                      a.exchange(0) / 64e3, b.exchange(0) / 64e3, c.exchange(0) / 64e3);
          }
        }
        if (rc != MGX_OK) slot->error = MakeError(static_cast<ErrorCode>(rc), mgx_last_error());
        slot->timing.enqueue_ms = std::chrono::duration<double, std::milli>(clock::now() - t0).count();
        lock.lock();
        if (rc != MGX_OK && comm && !comm_poisoned) {
          comm_poisoned = true;
          poison_message = slot->error.message();
          (void)mgx_comm_abort(comm);
        }
      }
      slot->state = slot->error.code() == ErrorCode::kSuccess && slot->state == kCompiled ? kEnqueued : kFailed;
      ++next_enqueue;
      cv_state.notify_all();
    }
    enqueuing = false;
  }

  void Work() {
    std::unique_lock<std::mutex> lock(mu);
    for (;;) {
      cv_work.wait(lock, [&] { return stop || !chunks.empty(); });
      if (stop) return;
      const Chunk c = chunks.front();
      chunks.pop_front();
      lock.unlock();
      for (size_t i = c.begin; i < c.end; ++i) {
        c.slot->plans[i].Reset();  // (the slot's plans are re-used from batch to batch)
        PlanQuery(index, c.slot->queries[i], c.slot->total_docs, c.slot->avgdl, &c.slot->plans[i]);
        if (c.slot->delta) {
          c.slot->dplans[i].Reset();
          if (c.slot->plans[i].error == ErrorCode::kSuccess)
            PlanForDelta(*c.slot->delta, c.slot->queries[i], c.slot->total_docs, c.slot->avgdl, c.slot->plans[i],
                         &c.slot->dplans[i]);
        }
      }
      lock.lock();
      if (--c.slot->chunks_left != 0) continue;
      c.slot->t_planned = clock::now();
      c.slot->state = kPlanned;
      cv_state.notify_all();
    }
  }

  // Dedicated threads compile, ticket after ticket (the compile step walks the same arenas and pinned blocks every time:
  // on whichever planner finished last it cost 2-3x). Three of them take tickets in turn — compiling a batch is ~0.5 ms
  // of one thread, which on a small shard (0.3 ms of device per batch) was the step — and whoever finishes puts every
  // batch that is ready on the device IN TICKET ORDER (EnqueueReady: one thread at a time): the order a sharded table's
  // collectives need identical on every rank.
  void Dispatch() {
    std::unique_lock<std::mutex> lock(mu);
    for (;;) {
      Slot* slot = nullptr;
      cv_state.wait(lock, [&] {
        slot = ByTicket(next_compile);
        return stop || (slot && slot->state == kPlanned);
      });
      if (stop) return;
      slot->state = kCompiling;
      ++next_compile;
      lock.unlock();
      const auto t_begin = clock::now();  // (a planned batch may have waited for this thread: not compile time)
      Compile(slot);
      slot->t_compiled = clock::now();
      slot->timing.plan_ms = std::chrono::duration<double, std::milli>(slot->t_planned - slot->t_submit).count();
      slot->timing.compile_ms = std::chrono::duration<double, std::milli>(slot->t_compiled - t_begin).count();
      lock.lock();
      slot->state = slot->error.code() == ErrorCode::kSuccess ? kCompiled : kFailed;
      EnqueueReady(lock);
    }
  }
};

BatchExecutor::BatchExecutor(const index::Index& index, Options options) : impl_(std::make_unique<Impl>(index, options)) {
  index.Finalize();
  impl_->total_docs = index.Bm25DocCount();
  impl_->avgdl = index.Bm25AvgDocLength();
  impl_->slots.resize(static_cast<size_t>(std::max(1, options.depth)));
  // (threads are named so that a profile — or bench.py's per-thread CPU accounting over /proc/self/task — can tell the
  // roles apart)
  for (int t = 0; t < std::max(1, options.planner_threads); ++t)
    impl_->workers.emplace_back([this] {
      pthread_setname_np(pthread_self(), "mgx-plan");
      impl_->Work();
    });
  static const int kDispatchers = std::getenv("MGX_DISPATCHERS") ? atoi(std::getenv("MGX_DISPATCHERS")) : 3;
  const int n_dispatchers = std::max(1, std::min(kDispatchers, std::max(1, options.depth)));
  for (int t = 0; t < n_dispatchers; ++t)
    impl_->dispatchers.emplace_back([this] {
      pthread_setname_np(pthread_self(), "mgx-dispatch");
      impl_->Dispatch();
    });
}

BatchExecutor::~BatchExecutor() {
  {
    std::unique_lock<std::mutex> lock(impl_->mu);
    // batches still in the pipeline reach the device first: a collective half-issued would hang the other ranks
    impl_->cv_state.wait(lock, [&] {
      for (auto& s : impl_->slots)
        if (s.state == Impl::kPlanning || s.state == Impl::kPlanned || s.state == Impl::kCompiling ||
            s.state == Impl::kCompiled)
          return false;
      return true;
    });
    impl_->stop = true;
  }
  impl_->cv_work.notify_all();
  impl_->cv_state.notify_all();
  for (auto& w : impl_->workers) w.join();
  for (auto& d : impl_->dispatchers) d.join();
  for (auto& s : impl_->slots) {
    if (s.state == Impl::kEnqueued && s.batch && !s.mq.empty()) {
      mgx_result_view v{};
      (void)mgx_batch_fetch(s.batch, &v);  // (drain the device before the object goes)
    }
    if (s.dbatch) mgx_batch_destroy(s.dbatch);
    if (s.batch) mgx_batch_destroy(s.batch);
  }
}

Expected<uint64_t, Error> BatchExecutor::Submit(std::vector<BatchQuery>&& queries) {
  index::Index::Impl* im = impl_->index.impl();
  if (!im->dev) return MakeUnexpected(MakeError(ErrorCode::kInternalError, im->last_error));
  // a mutable table: what ApplyMutations would do now (NextMutationStep). An install changes the device, so nothing of
  // this executor may be being planned or compiled meanwhile (batches already on the device finish first: the install
  // waits for them); a kick only starts a background build.
  index::MutationStep step;
  bool mutable_table = false;
  {
    std::lock_guard<std::mutex> il(im->mu);
    step = index::NextMutationStep(im->mut, /*force=*/false);
    mutable_table = im->mut.active;
  }
  if (step == index::MutationStep::kInstall) {
    if (impl_->opt.comm)
      return MakeUnexpected(MakeError(ErrorCode::kNotImplemented, "a sharded table (Options::comm) is static"));
    std::unique_lock<std::mutex> lock(impl_->mu);
    impl_->cv_state.wait(lock, [&] {
      for (auto& s : impl_->slots)
        if (s.state == Impl::kPlanning || s.state == Impl::kPlanned || s.state == Impl::kCompiling || s.state == Impl::kCompiled)
          return false;
      return true;
    });
  }
  if (step != index::MutationStep::kNothing) {
    const std::string merr = impl_->index.ApplyMutations();
    if (!merr.empty()) return MakeUnexpected(MakeError(ErrorCode::kInternalError, merr));
  }
  if (mutable_table) {  // (another entry point may have applied the changes: the statistics are read per batch)
    impl_->total_docs = impl_->index.Bm25DocCount();
    impl_->avgdl = impl_->index.Bm25AvgDocLength();
  }
  if (impl_->opt.comm && AnyFacets(queries))
    return MakeUnexpected(MakeError(ErrorCode::kNotImplemented,
                                    "facet_columns on a sharded table (Options::comm) is not implemented: the counts of "
                                    "the shards are not reduced"));
  if (impl_->opt.comm && AnyDocuments(queries))
    return MakeUnexpected(MakeError(ErrorCode::kNotImplemented,
                                    "return_documents on a sharded table (Options::comm) is not implemented: the page's "
                                    "rows live on other ranks"));
  if (impl_->opt.comm && AnyHighlight(queries))
    return MakeUnexpected(MakeError(ErrorCode::kNotImplemented,
                                    "highlight on a sharded table (Options::comm) is not implemented: the page's texts "
                                    "live on other ranks"));
  Impl::Slot* slot = nullptr;
  {
    std::lock_guard<std::mutex> lock(impl_->mu);
    for (auto& s : impl_->slots)
      if (s.state == Impl::kFree) {
        slot = &s;
        break;
      }
    if (!slot)
      return MakeUnexpected(MakeError(ErrorCode::kInvalidArgument,
                                      "BatchExecutor: every slot holds an unfetched batch (Wait for one first)"));
    slot->state = Impl::kFilling;  // reserved: nobody else touches it until its chunks are queued
  }
  // (outside the lock: freeing the slot's previous queries and plans and sizing the new ones is a few thousand
  // allocations, and the planner threads take the same lock for every chunk)
  slot->queries.swap(queries);  // (the caller gets the slot's previous batch back: storage to build its next one in)
  slot->plans.resize(slot->queries.size());  // (elements are reset by the planner that takes them)
  slot->total_docs = impl_->total_docs;
  slot->avgdl = impl_->avgdl;
  slot->delta = DeltaOf(impl_->index);
  if (slot->delta) slot->dplans.resize(slot->queries.size());
  slot->error = Error{ErrorCode::kSuccess, ""};
  slot->timing = Timing{};
  slot->t_submit = Impl::clock::now();
  const size_t n = slot->queries.size();
  std::lock_guard<std::mutex> lock(impl_->mu);
  slot->ticket = impl_->next_ticket++;
  slot->state = Impl::kPlanning;
  slot->chunks_left = std::max<size_t>(1, (n + Impl::kChunk - 1) / Impl::kChunk);
  if (n == 0) impl_->chunks.push_back(Impl::Chunk{slot, 0, 0});
  for (size_t a = 0; a < n; a += Impl::kChunk) impl_->chunks.push_back(Impl::Chunk{slot, a, std::min(n, a + Impl::kChunk)});
  impl_->cv_work.notify_all();
  return slot->ticket;
}

Expected<uint64_t, Error> BatchExecutor::Submit(const std::vector<BatchQuery>& queries) {
  return Submit(std::vector<BatchQuery>(queries));
}

Expected<std::vector<BatchResult>, Error> BatchExecutor::Wait(uint64_t ticket, Timing* timing) {
  std::vector<BatchResult> out;
  const Error e = WaitInto(ticket, &out, timing);
  if (e.code() != ErrorCode::kSuccess) return MakeUnexpected(e);
  return out;
}

Error BatchExecutor::Warm(const std::vector<BatchQuery>& sample, int rounds) {
  const size_t depth = impl_->slots.size();
  std::vector<uint64_t> tickets;
  std::vector<BatchResult> sink;
  for (int r = 0; r < std::max(1, rounds); ++r) {
    tickets.clear();
    for (size_t k = 0; k < depth; ++k) {  // all slots in flight at once: each one is touched in every round
      auto t = Submit(sample);
      if (!t) return t.error();
      tickets.push_back(*t);
    }
    for (uint64_t t : tickets) {
      const Error e = WaitInto(t, &sink);
      if (e.code() != ErrorCode::kSuccess) return e;
    }
  }
  return Error{ErrorCode::kSuccess, ""};
}

Error BatchExecutor::WaitInto(uint64_t ticket, std::vector<BatchResult>* results, Timing* timing) {
  std::vector<BatchResult>& out = *results;
  std::unique_lock<std::mutex> lock(impl_->mu);
  Impl::Slot* s = ticket ? impl_->ByTicket(ticket) : nullptr;
  if (!s) return MakeError(ErrorCode::kInvalidArgument, "BatchExecutor::Wait: unknown ticket");
  impl_->cv_state.wait(lock, [&] { return s->state == Impl::kEnqueued || s->state == Impl::kFailed; });
  if (s->state == Impl::kFailed) {
    const Error e = s->error;
    s->state = Impl::kFree;
    return e;
  }
  lock.unlock();  // (the slot is this caller's until it is freed below)
  mgx_result_view v{}, dv{};
  const auto t0 = Impl::clock::now();
  if (!s->mq.empty()) {
    int rc = mgx_batch_fetch(s->batch, &v);
    if (rc == MGX_OK && s->delta) rc = mgx_batch_fetch(s->dbatch, &dv);
    if (rc != MGX_OK) {
      const Error e = MakeError(static_cast<ErrorCode>(rc), mgx_last_error());
      lock.lock();
      s->state = Impl::kFree;
      return e;
    }
  }
  Collect(s->plans, v, &out, s->delta ? &dv : nullptr);
  if (!s->mq.empty()) {
    int rc = CollectSnippets(impl_->index, s->queries, s->plans, s->batch, v, &out);
    if (rc == MGX_OK) rc = CollectDocuments(impl_->index, s->delta.get(), s->queries, s->plans, s->batch, v, s->docreq, &out);
    if (rc != MGX_OK) {
      const Error e = MakeError(static_cast<ErrorCode>(rc), mgx_last_error());
      lock.lock();
      s->state = Impl::kFree;
      return e;
    }
  }
  {
    const bool dev = !s->mq.empty();
    const Error fe = CollectFacets(s->queries, s->plans, s->delta ? &s->dplans : nullptr, dev ? s->batch : nullptr,
                                   dev && s->delta ? s->dbatch : nullptr, &out);
    if (fe.code() != ErrorCode::kSuccess) {
      lock.lock();
      s->state = Impl::kFree;
      return fe;
    }
  }
  s->timing.wait_ms = std::chrono::duration<double, std::milli>(Impl::clock::now() - t0).count();
  if (timing) *timing = s->timing;
  lock.lock();
  s->state = Impl::kFree;
  return Error{ErrorCode::kSuccess, ""};
}

// ---- MicroBatcher --------------------------------------------------------------------------------------------------

struct MicroBatcher::Impl {
  using clock = std::chrono::steady_clock;
  struct Waiter {  // one blocked Search() call
    std::mutex mu;
    std::condition_variable cv;
    bool done = false;
    Expected<BatchResult, Error> result{MakeUnexpected(MakeError(ErrorCode::kInternalError, "unanswered"))};
  };
  struct InFlight {
    uint64_t ticket = 0;
    std::vector<Waiter*> waiters;
    Error submit_error{ErrorCode::kSuccess, ""};
  };
  Options opt;
  BatchExecutor executor;
  std::mutex mu;  // the forming batch, the in-flight queue, stats
  std::condition_variable cv_pending, cv_inflight, cv_room;
  std::vector<BatchQuery> pending;
  std::vector<Waiter*> pending_waiters;
  clock::time_point first_arrival;
  std::deque<InFlight> inflight;
  Stats stats;
  bool stop = false;
  std::thread former, completer;

  Impl(const index::Index& index, Options o) : opt(o), executor(index, o.executor) {}

  static void Answer(Waiter* w, Expected<BatchResult, Error>&& r) {
    std::lock_guard<std::mutex> lock(w->mu);
    w->result = std::move(r);
    w->done = true;
    w->cv.notify_one();
  }

  void Form() {
    std::unique_lock<std::mutex> lock(mu);
    for (;;) {
      cv_pending.wait(lock, [&] { return stop || !pending.empty(); });
      if (pending.empty()) return;  // (stop, and nothing left to answer)
      // the batch closes when it is full or when its first query has waited max_delay
      const auto deadline = first_arrival + opt.max_delay;
      const bool full = cv_pending.wait_until(lock, deadline, [&] { return stop || pending.size() >= opt.max_batch; });
      // no more batches in flight than the executor has slots
      cv_room.wait(lock, [&] { return inflight.size() < static_cast<size_t>(std::max(1, opt.executor.depth)); });
      InFlight f;
      std::vector<BatchQuery> batch;
      const size_t take = std::min(pending.size(), opt.max_batch);
      batch.assign(std::make_move_iterator(pending.begin()), std::make_move_iterator(pending.begin() + take));
      f.waiters.assign(pending_waiters.begin(), pending_waiters.begin() + take);
      pending.erase(pending.begin(), pending.begin() + take);
      pending_waiters.erase(pending_waiters.begin(), pending_waiters.begin() + take);
      if (!pending.empty()) first_arrival = clock::now();  // (what did not fit starts the next batch now)
      ++stats.batches;
      stats.queries += take;
      ++(full && take == opt.max_batch ? stats.closed_full : stats.closed_by_delay);
      lock.unlock();
      auto t = executor.Submit(std::move(batch));
      lock.lock();
      if (t) f.ticket = *t; else f.submit_error = t.error();
      inflight.push_back(std::move(f));
      cv_inflight.notify_one();
    }
  }

  void Complete() {
    std::unique_lock<std::mutex> lock(mu);
    for (;;) {
      cv_inflight.wait(lock, [&] { return !inflight.empty() || (stop && pending.empty() && former_done); });
      if (inflight.empty()) return;
      InFlight f = std::move(inflight.front());
      lock.unlock();
      if (f.ticket == 0) {
        for (Waiter* w : f.waiters) Answer(w, MakeUnexpected(f.submit_error));
      } else {
        auto r = executor.Wait(f.ticket);
        if (!r) {
          for (Waiter* w : f.waiters) Answer(w, MakeUnexpected(r.error()));
        } else {
          for (size_t i = 0; i < f.waiters.size(); ++i) Answer(f.waiters[i], std::move((*r)[i]));
        }
      }
      lock.lock();
      inflight.pop_front();  // (the slot is free again only now: Wait has returned)
      cv_room.notify_one();
    }
  }
  bool former_done = false;
};

MicroBatcher::MicroBatcher(const index::Index& index, Options options) : impl_(std::make_unique<Impl>(index, options)) {
  impl_->former = std::thread([this] {
    impl_->Form();
    std::lock_guard<std::mutex> lock(impl_->mu);
    impl_->former_done = true;
    impl_->cv_inflight.notify_all();
  });
  impl_->completer = std::thread([this] { impl_->Complete(); });
}

MicroBatcher::~MicroBatcher() {
  {
    std::lock_guard<std::mutex> lock(impl_->mu);
    impl_->stop = true;
  }
  impl_->cv_pending.notify_all();
  impl_->cv_inflight.notify_all();
  impl_->former.join();
  impl_->completer.join();
}

Expected<BatchResult, Error> MicroBatcher::Search(BatchQuery query) {
  Impl::Waiter w;
  {
    std::lock_guard<std::mutex> lock(impl_->mu);
    if (impl_->stop) return MakeUnexpected(MakeError(ErrorCode::kInvalidArgument, "MicroBatcher is shutting down"));
    if (impl_->pending.empty()) impl_->first_arrival = Impl::clock::now();
    impl_->pending.push_back(std::move(query));
    impl_->pending_waiters.push_back(&w);
    if (impl_->pending.size() == 1 || impl_->pending.size() >= impl_->opt.max_batch) impl_->cv_pending.notify_all();
  }
  std::unique_lock<std::mutex> lock(w.mu);
  w.cv.wait(lock, [&] { return w.done; });
  return std::move(w.result);
}

MicroBatcher::Stats MicroBatcher::GetStats() const {
  std::lock_guard<std::mutex> lock(impl_->mu);
  return impl_->stats;
}

}  // namespace search_pipeline

// ---- storage::DocumentStore::GetDocumentsBatch / GetPrimaryKeysBatch ------------------------------------------------------
namespace {
using storage::DocId;
// The rows of an id list from the device: one mgx_documents_gather over the main index and the table's delta. `with_filters`:
// every filter column of the table. nullopt for an id the table does not hold: no slot in either index, a gap of the main
// index's range, or a main document removed or superseded (the device's live row, as the single operators read it).
std::vector<std::optional<storage::Document>> GatherDocuments(const index::Index& index, const std::vector<DocId>& doc_ids,
                                                              bool with_filters) {
  using search_pipeline::DeltaOf;
  index::ClearDeviceError();
  std::vector<std::optional<storage::Document>> out(doc_ids.size());
  auto fail = [&](const std::string& msg) {
    index::SetDeviceError(msg);
    out.assign(doc_ids.size(), std::nullopt);
    return out;
  };
  index.Finalize();
  index::Index::Impl* im = index.impl();
  if (!im->dev) return fail(im->last_error);
  {
    const std::string merr = index.ApplyMutations();
    if (!merr.empty()) return fail(merr);
  }
  if (doc_ids.empty()) return out;
  const std::shared_ptr<index::Index> delta = DeltaOf(index);
  index.FlushPendingFilterColumns();
  {
    const mygram::utils::Error e = search_pipeline::EnsureKeyBytes(index, delta.get());
    if (e.code() != mygram::utils::ErrorCode::kSuccess) return fail(e.message());
  }
  const index::Index::Impl* dim = delta ? delta->impl() : nullptr;
  search_pipeline::BatchQuery all;  // (no names: every column of the table)
  const std::vector<std::string> names =
      with_filters ? search_pipeline::DocumentColumnsOf(index, delta.get(), all) : std::vector<std::string>();
  if (names.size() > MGX_DOC_MAX_COLUMNS) return fail("GetDocumentsBatch: the table holds more than 32 filter columns");
  std::vector<uint32_t> mids(names.size(), MGX_DOC_NO_COLUMN), dids(names.size(), MGX_DOC_NO_COLUMN);
  {
    std::lock_guard<std::mutex> lock(im->filter_mu);
    for (size_t c = 0; c < names.size(); ++c)
      if (const auto* col = im->ResolveColumn(names[c])) mids[c] = col->device_id;
  }
  if (dim != nullptr) {
    std::lock_guard<std::mutex> lock(dim->filter_mu);
    for (size_t c = 0; c < names.size(); ++c)
      if (const auto* col = dim->ResolveColumn(names[c])) dids[c] = col->device_id;
  }
  uint8_t* records = nullptr;
  uint64_t stride = 0;
  if (mgx_documents_gather(im->dev, dim ? dim->dev : nullptr, doc_ids.data(), doc_ids.size(), static_cast<uint32_t>(names.size()),
                           mids.data(), dids.data(), 0, &records, &stride) != MGX_OK)
    return fail(mgx_last_error());
  std::unique_ptr<uint8_t, void (*)(void*)> guard(records, mgx_free);
  std::vector<uint8_t> live(doc_ids.size(), 1);
  {
    std::lock_guard<std::mutex> lock(im->mu);
    const DocId first = im->view.first_doc_id;
    for (size_t i = 0; i < doc_ids.size(); ++i) {
      const DocId d = doc_ids[i];
      if (d < first || d - first >= im->view.n_docs) continue;  // (not a slot of the main index)
      const uint64_t slot = d - first;
      if (im->has_gaps && slot / 64 < im->exists_bits.size() && ((im->exists_bits[slot >> 6] >> (slot & 63)) & 1) == 0) live[i] = 0;
      if (im->mut.active && !im->LiveApplied(d)) live[i] = 0;
    }
  }
  std::unique_lock<std::mutex> ml(im->filter_mu), dl;
  if (dim != nullptr) dl = std::unique_lock<std::mutex>(dim->filter_mu);
  std::vector<const index::Index::Impl::FilterColumn*> mcols(names.size(), nullptr), dcols(names.size(), nullptr);
  for (size_t c = 0; c < names.size(); ++c) {
    mcols[c] = im->ResolveColumn(names[c]);
    if (dim != nullptr) dcols[c] = dim->ResolveColumn(names[c]);
  }
  for (size_t i = 0; i < doc_ids.size(); ++i) {
    const uint8_t* rec = records + i * stride;
    mgx_document_record_header h;
    std::memcpy(&h, rec, sizeof(h));
    if ((h.flags & MGX_DOC_FOUND) == 0) continue;
    const bool mapped = (h.flags & MGX_DOC_MAPPED) != 0;
    if (!mapped && !live[i]) continue;
    storage::Document doc;
    doc.doc_id = doc_ids[i];
    const uint8_t* key = rec + sizeof(h) + 8ull * names.size();
    if (h.flags & MGX_DOC_HAS_KEY) doc.primary_key.assign(reinterpret_cast<const char*>(key), h.key_len);
    const auto& cols = mapped ? dcols : mcols;
    for (uint32_t c = 0; c < h.n_columns && c < cols.size(); ++c) {
      if (((h.null_mask >> c) & 1u) != 0 || cols[c] == nullptr || cols[c]->type == 0) continue;
      uint64_t w;
      std::memcpy(&w, rec + sizeof(h) + 8ull * c, 8);
      doc.filters[cols[c]->name] = index::FilterValueFromBits(cols[c]->type, w, cols[c]->dict);
    }
    out[i] = std::move(doc);
  }
  return out;
}
}  // namespace

std::vector<std::optional<storage::Document>> storage::DocumentStore::GetDocumentsBatch(const std::vector<DocId>& doc_ids) const {
  return GatherDocuments(*index_, doc_ids, true);
}

std::vector<std::optional<std::string>> storage::DocumentStore::GetPrimaryKeysBatch(const std::vector<DocId>& doc_ids) const {
  const std::vector<std::optional<storage::Document>> docs = GatherDocuments(*index_, doc_ids, false);
  std::vector<std::optional<std::string>> out(docs.size());
  for (size_t i = 0; i < docs.size(); ++i)
    if (docs[i]) out[i] = docs[i]->primary_key;
  return out;
}
}  // namespace mygramdb
