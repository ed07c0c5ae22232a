// documents_test.cpp — page documents through the C++17 shim: BatchQuery::return_documents / document_columns through
// ExecuteBatch, BatchExecutor (two batches in flight) and MicroBatcher, on a mutable table of 3,000 documents.
// BatchResult::documents must equal a std::map model of what the table was given ({doc_id, primary_key, the non-NULL
// filter values}), after the build, after adds, UpdateDocument, UpdateFilters and RemoveDocument (a delta index: a moved
// document brings its key and its new values from the delta, strings through the delta's dictionary) and after Compact().
// Page shapes: the default order (primary key DESC), SORT _score, a numeric column sort, a doc-id page.
// storage::DocumentStore::GetDocumentsBatch / GetPrimaryKeysBatch over an id list with unknown and removed ids, in every phase.
// Needs a GPU; built and run by tests/test_gpu_documents_shim.py.
#include <algorithm>
#include <cctype>
#include <cstdint>
#include <cstdio>
#include <map>
#include <memory>
#include <optional>
#include <string>
#include <utility>
#include <vector>

#include "../../mygram-db_amd/csrc/shim/mygram_shim.hpp"

using mygram::utils::ErrorCode;
using mygramdb::index::DocId;
using mygramdb::index::Index;
using mygramdb::query::SortOrder;
using mygramdb::storage::Document;
using mygramdb::storage::FilterMap;
using mygramdb::storage::FilterValue;
using namespace mygramdb::search_pipeline;

static int g_failed = 0, g_checked = 0;
#define EXPECT(cond)                                              \
  do {                                                            \
    ++g_checked;                                                  \
    if (!(cond)) {                                                \
      ++g_failed;                                                 \
      std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); \
    }                                                             \
  } while (0)

struct Row {
  std::string text;
  std::optional<std::string> pk;
  FilterMap filters;
};
using Docs = std::map<DocId, Row>;

static const char* const kCities[] = {"", "osaka", "tokyo", "kyoto", "\x80\xff raw"};

static std::string Text(DocId d, bool delta) {
  std::string t = "w" + std::to_string(d);
  if (d % 5 != 0) t += " alpha";
  if (d % 2 == 0) t += " beta";
  t += delta ? " deltaword" : " mainword";
  return t;
}

// The values a document is given: NULLs are simply absent (a FilterMap holds the non-NULL values).
static FilterMap Filters(DocId d, bool delta) {
  FilterMap f;
  if (d % 4 != 0) f["status"] = static_cast<int32_t>(d % 11) - 5;
  if (d % 3 != 0) f["score"] = d % 9 == 0 ? -0.0 : static_cast<double>(d) / 7.0;
  if (d % 6 != 0) f["city"] = std::string(delta && d % 2 == 0 ? "zurich" : kCities[d % 5]);  // "zurich": the delta's dictionary only
  f["big"] = d % 13 == 0 ? UINT64_MAX : static_cast<uint64_t>(d) << 33;
  return f;
}

static std::optional<std::string> Key(DocId d) {
  if (d == 7) return "007";
  if (d == 2803) return "7";
  if (d % 97 == 0) return std::nullopt;
  if (d % 31 == 0) return std::string();
  if (d % 41 == 0) return std::string(200 + d % 70, 'k') + std::to_string(d);  // longer than a 256-byte row, some of them
  return "pk" + std::to_string((static_cast<uint64_t>(d) * 7919u) % 100003u);
}

static std::vector<BatchQuery> Queries() {
  std::vector<BatchQuery> qs(8);
  qs[0].terms = {"alpha"};  // the reference's default order: primary key DESC
  qs[0].sort_primary_key = true;
  qs[0].order = SortOrder::DESC;
  qs[0].limit = 100;
  qs[1].terms = {"alpha"};  // SORT _score
  qs[1].sort_by_score = true;
  qs[1].limit = 50;
  qs[2].terms = {"beta"};   // a numeric column sort, with an offset
  qs[2].sort_column = "big";
  qs[2].order = SortOrder::ASC;
  qs[2].limit = 80;
  qs[2].offset = 10;
  qs[3].terms = {"alpha"};  // a doc-id page, two named columns (one in another letter case), one of them twice
  qs[3].limit = 30;
  qs[3].document_columns = {"CITY", "status", "city"};
  qs[4].terms = {"deltaword"};  // the delta's documents only (none before the changes)
  qs[4].sort_primary_key = true;
  qs[4].order = SortOrder::ASC;
  qs[4].limit = 1000;
  qs[4].document_columns = {"city"};
  qs[5].terms = {"beta"};   // no request beside the others
  qs[5].limit = 20;
  qs[6].terms = {"changed"};  // the documents UpdateDocument moved (none before the changes)
  qs[6].limit = 10;
  qs[7].terms = {"w30"};    // document 30 among them: UpdateFilters moves it
  qs[7].limit = 50;
  for (size_t i = 0; i < qs.size(); ++i) qs[i].return_documents = i != 5;
  return qs;
}

static bool SameDocument(const Docs& docs, const BatchQuery& q, DocId id, const std::optional<Document>& got) {
  const auto it = docs.find(id);
  if (it == docs.end() || !got) return false;  // (a removed document never appears; a page entry is always found)
  FilterMap want;
  if (q.document_columns.empty()) {
    want = it->second.filters;
  } else {
    for (std::string name : q.document_columns) {
      for (char& c : name) c = static_cast<char>(std::tolower(static_cast<unsigned char>(c)));
      const auto f = it->second.filters.find(name);
      if (f != it->second.filters.end()) want[name] = f->second;
    }
  }
  return got->doc_id == id && got->primary_key == it->second.pk.value_or("") && got->filters == want;
}

static void Check(const Docs& docs, const std::vector<BatchQuery>& qs, const std::vector<BatchResult>& got, const char* what) {
  EXPECT(got.size() == qs.size());
  for (size_t i = 0; i < qs.size() && i < got.size(); ++i) {
    const BatchResult& r = got[i];
    if (!qs[i].return_documents) {
      EXPECT(r.documents.empty());
      continue;
    }
    EXPECT(r.documents.size() == r.results.size());
    size_t bad = 0;
    for (size_t j = 0; j < r.results.size() && j < r.documents.size(); ++j)
      bad += SameDocument(docs, qs[i], r.results[j], r.documents[j]) ? 0 : 1;
    EXPECT(bad == 0);
    if (bad) std::printf("  %s: query %zu: %zu of %zu documents differ from the model\n", what, i, bad, r.results.size());
  }
}

constexpr DocId kMain = 2500, kDeltaFirst = 2501, kDeltaLast = 3000;

// storage::DocumentStore::GetDocumentsBatch / GetPrimaryKeysBatch over an id list that holds known ids of both indexes,
// removed ids, ids never added (below, inside and far above the table's range) and one id twice: the model's rows, and
// nullopt for every id the model does not hold.
static void CheckStore(const Docs& docs, const Index& table, const char* what) {
  std::vector<DocId> ids = {0, 1, 7, 20, 22, 30, 31, 40, 41, 82, 97, 2500, 2501, 2510, 2542, 2600, 2803, 3000, 3001, 3002,
                            999999, 4000000000u, 7};
  for (DocId d = 100; d < 400; d += 3) ids.push_back(d);
  for (DocId d = 2700; d < 2900; d += 7) ids.push_back(d);
  const mygramdb::storage::DocumentStore store(table);
  const auto rows = store.GetDocumentsBatch(ids);
  EXPECT(mygramdb::index::LastDeviceError().empty());
  const auto keys = store.GetPrimaryKeysBatch(ids);
  EXPECT(mygramdb::index::LastDeviceError().empty());
  EXPECT(rows.size() == ids.size() && keys.size() == ids.size());
  if (rows.size() != ids.size() || keys.size() != ids.size()) return;
  const BatchQuery every_column;
  size_t bad = 0, known = 0, unknown = 0;
  for (size_t i = 0; i < ids.size(); ++i) {
    const auto it = docs.find(ids[i]);
    if (it == docs.end()) {
      bad += (rows[i].has_value() ? 1 : 0) + (keys[i].has_value() ? 1 : 0);
      ++unknown;
      continue;
    }
    ++known;
    bad += SameDocument(docs, every_column, ids[i], rows[i]) ? 0 : 1;
    bad += keys[i].has_value() && *keys[i] == it->second.pk.value_or("") ? 0 : 1;
  }
  EXPECT(bad == 0 && known > 50 && unknown >= 4);
  if (bad) std::printf("  %s: DocumentStore: %zu rows or keys differ from the model (%zu known ids, %zu unknown)\n", what, bad, known, unknown);
  EXPECT(store.GetDocumentsBatch({}).empty() && store.GetPrimaryKeysBatch({}).empty());
}

int main() {
  Docs docs;
  Index table(2, 0, 0.0, false);
  table.SetPrimaryKeyColumn("id");
  auto add = [&](DocId d, bool delta) {
    docs[d] = Row{Text(d, delta), Key(d), Filters(d, delta)};
    const Row& r = docs[d];
    if (r.pk) EXPECT(table.AddDocument(d, r.text, r.filters, *r.pk));
    else EXPECT(table.AddDocument(d, r.text, r.filters));
  };
  for (DocId d = 1; d <= kMain; ++d) add(d, false);
  const std::vector<BatchQuery> qs = Queries();
  {  // ---- after the build: one index ----
    auto got = ExecuteBatch(table, qs);
    EXPECT(got.has_value());
    if (!got) {
      std::printf("  static: %s\n", got.error().message().c_str());
      return 1;
    }
    Check(docs, qs, *got, "static table");
    EXPECT((*got)[0].results.size() == 100 && (*got)[1].results.size() == 50 && (*got)[2].results.size() == 80);
    EXPECT((*got)[3].results.size() == 30 && (*got)[4].results.empty() && (*got)[4].documents.empty());
    EXPECT((*got)[6].results.empty() && !(*got)[7].results.empty());
    CheckStore(docs, table, "static table");
  }
  {  // ---- refusals ----
    BatchQuery q = qs[3];
    q.document_columns = {"status", "no_such_column"};
    auto bad = ExecuteBatch(table, {qs[1], q});
    EXPECT(!bad.has_value() && bad.error().code() == ErrorCode::kIndexNotFound);
    EXPECT(!bad.has_value() && bad.error().message().find("no_such_column") != std::string::npos);
    q = qs[3];
    q.limit = 0;
    bad = ExecuteBatch(table, {q});
    EXPECT(!bad.has_value() && bad.error().code() == ErrorCode::kOutOfRange);
    q.limit = 1025;
    bad = ExecuteBatch(table, {q});
    EXPECT(!bad.has_value() && bad.error().code() == ErrorCode::kOutOfRange);
    q = qs[3];
    q.facet_columns = {"city"};
    bad = ExecuteBatch(table, {q});
    EXPECT(!bad.has_value() && bad.error().code() == ErrorCode::kInvalidArgument);
    auto good = ExecuteBatch(table, {qs[3]});  // the table serves as before
    EXPECT(good.has_value());
    if (good) Check(docs, {qs[3]}, *good, "after the refusals");
  }
  // ---- changes: new documents; a new text; new filter values; removals on both sides ----
  for (DocId d = kDeltaFirst; d <= kDeltaLast; ++d) add(d, true);
  docs[20].text = Text(20, false) + " changed";
  table.UpdateDocument(20, Text(20, false), docs[20].text);  // moves to the delta with its key and its values
  docs[22].text = Text(22, false) + " changed";
  docs[22].filters = FilterMap{{"city", std::string("zurich")}, {"status", static_cast<int32_t>(99)}};
  table.UpdateDocument(22, Text(22, false), docs[22].text, docs[22].filters);
  docs[30].filters = FilterMap{{"big", static_cast<uint64_t>(12345)}, {"city", std::string("osaka")}};  // status, score: NULL now
  EXPECT(table.UpdateFilters(30, docs[30].filters));
  docs[2600].filters = FilterMap{{"status", static_cast<int32_t>(-77)}};  // a document of the delta changes again
  EXPECT(table.UpdateFilters(2600, docs[2600].filters));
  table.RemoveDocument(40, docs[40].text);
  docs.erase(40);
  table.RemoveDocument(2510, docs[2510].text);
  docs.erase(2510);
  auto got = ExecuteBatch(table, qs);  // (applies the mutations)
  EXPECT(got.has_value());
  if (!got) {
    std::printf("  with a delta: %s\n", got.error().message().c_str());
    return 1;
  }
  EXPECT(table.GetMutationStats().delta_documents == kDeltaLast - kDeltaFirst + 3);  // 500 added - 1 removed + 3 moved
  Check(docs, qs, *got, "with a delta");
  CheckStore(docs, table, "with a delta");
  {
    EXPECT((*got)[0].results.size() == 100 && (*got)[2].results.size() == 80);
    const std::vector<DocId>& d = (*got)[4].results;  // every document of the delta, with the delta's strings
    EXPECT(d.size() == kDeltaLast - kDeltaFirst);  // 500 added - 1 removed
    size_t zurich = 0;
    for (const auto& doc : (*got)[4].documents) {
      if (!doc) continue;
      const auto f = doc->filters.find("city");
      zurich += f != doc->filters.end() && f->second == FilterValue(std::string("zurich"));
    }
    EXPECT(zurich > 100);
    EXPECT(std::find(d.begin(), d.end(), DocId(2510)) == d.end());
    EXPECT(((*got)[6].results == std::vector<DocId>{22, 20}));  // the moved documents, from the delta
    const std::vector<DocId>& w = (*got)[7].results;
    EXPECT(std::find(w.begin(), w.end(), DocId(30)) != w.end());
    const std::vector<DocId>& page = (*got)[0].results;  // the default order's page holds documents of both indexes
    const size_t from_delta = std::count_if(page.begin(), page.end(), [](DocId x) { return x >= kDeltaFirst; });
    EXPECT(from_delta > 0 && from_delta < page.size());
  }
  {  // BatchExecutor with two batches in flight
    BatchExecutor::Options o;
    o.depth = 2;
    BatchExecutor ex(table, o);
    std::vector<BatchQuery> other = {qs[1], qs[5], qs[0]};
    auto ta = ex.Submit(qs);
    auto tb = ex.Submit(other);
    EXPECT(ta.has_value() && tb.has_value());
    if (ta && tb) {
      auto ra = ex.Wait(*ta);
      auto rb = ex.Wait(*tb);
      EXPECT(ra.has_value() && rb.has_value());
      if (!ra) std::printf("  BatchExecutor: %s\n", ra.error().message().c_str());
      if (ra && rb) {
        Check(docs, qs, *ra, "BatchExecutor a");
        Check(docs, other, *rb, "BatchExecutor b");
        for (size_t i = 0; i < qs.size(); ++i) EXPECT((*ra)[i].results == (*got)[i].results);
      }
      auto tc = ex.Submit(qs);  // the slot's batch object again, after mgx_batch_reset
      EXPECT(tc.has_value());
      if (tc) {
        auto rc = ex.Wait(*tc);
        EXPECT(rc.has_value());
        if (rc) Check(docs, qs, *rc, "BatchExecutor c");
      }
    }
  }
  {
    MicroBatcher::Options mo;
    MicroBatcher mb(table, mo);
    for (size_t i : {size_t(0), size_t(1), size_t(3), size_t(5), size_t(6)}) {
      auto r = mb.Search(qs[i]);
      EXPECT(r.has_value());
      if (r) {
        Check(docs, {qs[i]}, {*r}, "MicroBatcher");
        EXPECT(r->results == (*got)[i].results);
      }
    }
  }
  // ---- Compact(): the key bytes are attached to the rebuilt index, the documents stay ----
  EXPECT(table.Compact().empty());
  EXPECT(table.GetMutationStats().delta_documents == 0);
  auto after = ExecuteBatch(table, qs);
  EXPECT(after.has_value());
  if (!after) std::printf("  after Compact: %s\n", after.error().message().c_str());
  if (after) {
    Check(docs, qs, *after, "after Compact");
    CheckStore(docs, table, "after Compact");
    for (size_t i = 0; i < qs.size(); ++i) EXPECT(i == 1 || (*after)[i].results == (*got)[i].results);
  }
  // ---- and a document added after Compact() starts a new delta ----
  add(3001, true);
  auto again = ExecuteBatch(table, qs);
  EXPECT(again.has_value());
  if (again) {
    Check(docs, qs, *again, "a new delta");
    CheckStore(docs, table, "a new delta");
    const std::vector<DocId>& d = (*again)[4].results;
    EXPECT(std::find(d.begin(), d.end(), DocId(3001)) != d.end());
  }
  std::printf("%d checks, %d failed\n", g_checked, g_failed);
  return g_failed == 0 ? 0 : 1;
}
