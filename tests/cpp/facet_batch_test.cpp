// facet_batch_test.cpp — FACET in a batch through the C++17 shim: BatchQuery::facet_columns through ExecuteBatch,
// BatchExecutor (two batches in flight) and MicroBatcher must return, per (query, column), exactly what ExecuteFacet
// returns for that column: matched_documents, total_values, value_counts and display, with limit and offset of the values.
// On a static table; after UpdateDocument, AddDocument, RemoveDocument and UpdateFilters (a delta index exists); after
// Compact(). An unknown column, highlight beside facet_columns and a sharded executor are refused.
// Needs a GPU; built and run by tests/test_gpu_facet_batch_shim.py.
#include <cstdint>
#include <cstdio>
#include <map>
#include <memory>
#include <string>
#include <utility>
#include <vector>

#include "../../mygram-db_amd/csrc/shim/mygram_shim.hpp"

using mygram::utils::ErrorCode;
using mygramdb::index::DocId;
using mygramdb::index::Index;
using mygramdb::query::NodeType;
using mygramdb::query::QueryNode;
using mygramdb::storage::FilterMap;
using mygramdb::storage::TimeValue;
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

static uint64_t g_rng = 4242;
static uint32_t Next() {
  g_rng = g_rng * 6364136223846793005ull + 1442695040888963407ull;
  return static_cast<uint32_t>(g_rng >> 33);
}

static const char* const kWords[] = {"alpha", "beta", "gamma", "delta", "omega", "theta", "lambda", "sigma", "kappa"};
static const char* const kNames[] = {"", "ann", "Ann", "bob", "zoe", "\xC3\xA9mile"};

struct DocRow {
  std::string text;
  FilterMap filters;
};
using Docs = std::map<DocId, DocRow>;

static DocRow Row(const char* extra = nullptr) {
  DocRow r;
  const uint32_t n = 2 + Next() % 5;
  for (uint32_t i = 0; i < n; ++i) {
    if (!r.text.empty()) r.text += ' ';
    r.text += kWords[Next() % 9];
  }
  if (extra) r.text += std::string(" ") + extra;
  r.filters["flag"] = Next() % 2 == 0;                                                        // two values, no NULL
  if (Next() % 10 < 7) r.filters["status"] = int32_t(Next() % 10);                            // ten values, ~30 % NULL
  if (Next() % 6 != 0) r.filters["name"] = std::string(kNames[Next() % 6]);                   // strings
  r.filters["serial"] = int64_t(Next() % 3000);                                               // many values
  r.filters["ts"] = TimeValue{static_cast<int64_t>(Next() % 40) - 20};
  return r;
}

static std::unique_ptr<QueryNode> Term(const char* t) { return std::make_unique<QueryNode>(std::string(t)); }
static std::unique_ptr<QueryNode> Node(NodeType t, std::unique_ptr<QueryNode> a, std::unique_ptr<QueryNode> b = nullptr) {
  auto n = std::make_unique<QueryNode>(t);
  n->children.push_back(std::move(a));
  if (b) n->children.push_back(std::move(b));
  return n;
}

// (query, columns): search parts of every kind, value pages of every kind
static std::vector<BatchQuery> Queries() {
  std::vector<BatchQuery> qs;
  auto add = [&](BatchQuery q, std::vector<std::string> cols, uint32_t limit, uint32_t offset) {
    q.facet_columns = std::move(cols);
    q.limit = limit;
    q.offset = offset;
    qs.push_back(std::move(q));
  };
  BatchQuery a;
  a.terms = {"alpha"};
  add(a, {"flag"}, 100, 0);
  add(a, {"status", "flag", "name"}, 100, 0);
  add(a, {"serial", "status"}, 7, 3);          // limit and offset page the values
  add(a, {"serial"}, 5, 100000);               // an offset past the values
  add(a, {"FLAG", "Status"}, 100, 0);          // names resolve as ExecuteFacet resolves them
  BatchQuery sorted = a;                        // sort fields are ignored
  sorted.sort_by_score = true;
  add(sorted, {"status"}, 3, 1);
  sorted.sort_by_score = false;
  sorted.sort_column = "serial";
  add(sorted, {"ts", "ts"}, 100, 0);           // the same column twice
  BatchQuery b;
  b.terms = {"beta", "gamma"};
  b.not_terms = {"kappa"};
  add(b, {"name", "serial", "flag", "ts"}, 10, 0);
  BatchQuery e;
  e.ast = Node(NodeType::AND, Node(NodeType::OR, Term("alpha"), Term("gamma")), Node(NodeType::NOT, Term("omega")));
  add(e, {"status", "serial"}, 100, 2);
  BatchQuery all;                               // no terms: every document
  add(all, {"flag", "status", "name", "serial", "ts", "flag", "status", "name"}, 100, 0);  // eight columns
  BatchQuery cond;
  cond.terms = {"delta"};
  cond.filter_conditions.push_back({"status", mygramdb::query::FilterOp::GT, "4"});
  add(cond, {"status", "flag"}, 100, 0);
  BatchQuery fz;
  fz.terms = {"alphq"};
  fz.fuzzy_max_distance = 1;
  add(fz, {"flag", "serial"}, 20, 0);
  BatchQuery none;                              // resolved on the host: an empty result
  none.terms = {"zzqx9"};
  add(none, {"flag", "status"}, 100, 0);
  return qs;
}

static bool SameFacet(const FacetOutput& got, const FacetOutput& want) {
  return got.matched_documents == want.matched_documents && got.total_values == want.total_values &&
         got.value_counts == want.value_counts && got.display == want.display;
}

// every (query, column) of `got` against ExecuteFacet on the same table
static void CheckAgainstExecuteFacet(const Index& table, const std::vector<BatchQuery>& qs, const std::vector<BatchResult>& got,
                                     const char* what) {
  EXPECT(got.size() == qs.size());
  if (got.size() != qs.size()) return;
  size_t with_values = 0;
  for (size_t i = 0; i < qs.size(); ++i) {
    EXPECT(got[i].results.empty() && got[i].scores.empty() && got[i].snippets.empty());
    EXPECT(got[i].facets.size() == qs[i].facet_columns.size());
    if (got[i].facets.size() != qs[i].facet_columns.size()) continue;
    for (size_t c = 0; c < qs[i].facet_columns.size(); ++c) {
      BatchQuery single = qs[i];
      single.facet_columns.clear();
      auto want = ExecuteFacet(table, single, qs[i].facet_columns[c]);
      EXPECT(want.has_value());
      if (!want) continue;
      const bool same = SameFacet(got[i].facets[c], *want) && got[i].total == want->matched_documents;
      EXPECT(same);
      if (!same)
        std::printf("  %s: query %zu column %s differs: matched %llu/%llu (total %llu), values %llu/%llu, page %zu/%zu\n", what, i,
                    qs[i].facet_columns[c].c_str(), static_cast<unsigned long long>(got[i].facets[c].matched_documents),
                    static_cast<unsigned long long>(want->matched_documents), static_cast<unsigned long long>(got[i].total),
                    static_cast<unsigned long long>(got[i].facets[c].total_values),
                    static_cast<unsigned long long>(want->total_values), got[i].facets[c].value_counts.size(),
                    want->value_counts.size());
      with_values += want->value_counts.empty() ? 0 : 1;
    }
  }
  EXPECT(with_values >= 20);
}

static void CheckEveryPath(const Index& table, const char* what) {
  const std::vector<BatchQuery> qs = Queries();
  auto got = ExecuteBatch(table, qs);
  EXPECT(got.has_value());
  if (!got) {
    std::printf("  %s: %s\n", what, got.error().message().c_str());
    return;
  }
  CheckAgainstExecuteFacet(table, qs, *got, what);
  EXPECT((*got)[9].total > 0 && (*got)[9].facets[0].matched_documents == (*got)[9].total);  // every document
  EXPECT((*got).back().total == 0 && (*got).back().facets[0].total_values == 0);             // the host-resolved one
  {
    // two batches in flight, faceted queries beside pages
    BatchExecutor::Options o;
    o.depth = 2;
    BatchExecutor ex(table, o);
    std::vector<BatchQuery> mixed = qs;
    BatchQuery page;
    page.terms = {"alpha"};
    page.sort_by_score = true;
    page.limit = 10;
    mixed.push_back(page);
    auto ta = ex.Submit(mixed);
    auto tb = ex.Submit(qs);
    EXPECT(ta.has_value() && tb.has_value());
    if (ta && tb) {
      auto ra = ex.Wait(*ta);
      auto rb = ex.Wait(*tb);
      EXPECT(ra.has_value() && rb.has_value());
      if (!ra) std::printf("  %s, BatchExecutor: %s\n", what, ra.error().message().c_str());
      if (ra && rb) {
        EXPECT(ra->back().results.size() == 10 && ra->back().facets.empty());
        ra->pop_back();
        CheckAgainstExecuteFacet(table, qs, *ra, "BatchExecutor a");
        CheckAgainstExecuteFacet(table, qs, *rb, "BatchExecutor b");
      }
      auto tc = ex.Submit(std::vector<BatchQuery>{page});  // the slot's next batch holds no request
      EXPECT(tc.has_value());
      if (tc) {
        auto rc = ex.Wait(*tc);
        EXPECT(rc.has_value() && rc->size() == 1 && (*rc)[0].results.size() == 10 && (*rc)[0].facets.empty());
      }
    }
  }
  {
    MicroBatcher::Options mo;
    MicroBatcher mb(table, mo);
    for (size_t i : {size_t(1), size_t(2), size_t(9), qs.size() - 1}) {
      auto r = mb.Search(qs[i]);
      EXPECT(r.has_value());
      if (!r) continue;
      EXPECT(r->facets.size() == (*got)[i].facets.size() && r->total == (*got)[i].total && r->results.empty());
      for (size_t c = 0; c < r->facets.size() && c < (*got)[i].facets.size(); ++c) EXPECT(SameFacet(r->facets[c], (*got)[i].facets[c]));
    }
    BatchQuery bad;
    bad.terms = {"alpha"};
    bad.facet_columns = {"flag", "nope"};
    auto r = mb.Search(bad);
    EXPECT(!r.has_value() && r.error().code() == ErrorCode::kIndexNotFound);
  }
}

static void Refusals(const Index& table) {
  BatchQuery q;
  q.terms = {"alpha"};
  q.facet_columns = {"flag", "no_such_column"};
  auto unknown = ExecuteBatch(table, {q});
  EXPECT(!unknown.has_value() && unknown.error().code() == ErrorCode::kIndexNotFound);
  if (!unknown) EXPECT(unknown.error().message() == "Facet column \"no_such_column\" not found");  // ExecuteFacet's
  auto single = ExecuteFacet(table, q, "no_such_column");
  EXPECT(!single.has_value() && !unknown.has_value() && single.error().message() == unknown.error().message());
  BatchQuery none = q;  // also when the query never reaches the device
  none.terms = {"zzqx9"};
  auto unknown_host = ExecuteBatch(table, {none});
  EXPECT(!unknown_host.has_value() && unknown_host.error().code() == ErrorCode::kIndexNotFound);
  q.facet_columns = {"flag"};
  q.highlight = mygramdb::query::HighlightOptions{};
  auto hl = ExecuteBatch(table, {q});
  EXPECT(!hl.has_value() && hl.error().code() == ErrorCode::kInvalidArgument);
  q.highlight.reset();
  q.facet_columns.assign(9, "flag");
  auto nine = ExecuteBatch(table, {q});
  EXPECT(!nine.has_value() && nine.error().code() == ErrorCode::kOutOfRange);
  {
    BatchExecutor ex(table);
    q.facet_columns = {"nope"};
    auto t = ex.Submit(std::vector<BatchQuery>{q});
    EXPECT(t.has_value());
    if (t) {
      auto r = ex.Wait(*t);
      EXPECT(!r.has_value() && r.error().code() == ErrorCode::kIndexNotFound);
    }
  }
  {
    // a sharded executor: refused before anything reaches the communicator
    BatchExecutor::Options so;
    so.comm = reinterpret_cast<mgx_comm*>(&so);  // (never dereferenced: Submit refuses first)
    BatchExecutor ex(table, so);
    q.facet_columns = {"flag"};
    auto t = ex.Submit(std::vector<BatchQuery>{q});
    EXPECT(!t.has_value() && t.error().code() == ErrorCode::kNotImplemented);
  }
}

int main() {
  Docs docs;
  Index table(2, 0, 0.0, false);
  for (DocId d = 1; d <= 6000; ++d) {
    docs[d] = Row();
    table.AddDocument(d, docs[d].text, docs[d].filters);
  }
  CheckEveryPath(table, "static");
  Refusals(table);
  // ---- changes: removed, updated (text and filters), filters alone, added past the range and into gaps ----
  for (int k = 0; k < 120; ++k) {
    const DocId d = 1 + Next() % 6000;
    if (!docs.count(d)) continue;
    table.RemoveDocument(d, docs[d].text);
    docs.erase(d);
  }
  for (int k = 0; k < 150; ++k) {
    const DocId d = 1 + Next() % 6000;
    if (!docs.count(d)) continue;
    DocRow nr = Row();
    if (k % 3 == 0) nr.filters["serial"] = int64_t(5000 + k);  // values the main index's dictionary does not hold
    table.UpdateDocument(d, docs[d].text, nr.text, nr.filters);
    docs[d] = nr;
  }
  for (int k = 0; k < 150; ++k) {
    const DocId d = 1 + Next() % 6000;
    if (!docs.count(d)) continue;
    const DocRow nr = Row();
    EXPECT(table.UpdateFilters(d, nr.filters));
    docs[d].filters = nr.filters;
  }
  for (DocId d = 7001; d <= 7120; ++d) {
    docs[d] = Row();
    EXPECT(table.AddDocument(d, docs[d].text, docs[d].filters));
  }
  {
    auto applied = ExecuteBatch(table, Queries());  // (applies the mutations)
    EXPECT(applied.has_value());
    EXPECT(table.GetMutationStats().delta_documents > 0);
    CheckEveryPath(table, "with a delta");
    EXPECT(table.GetMutationStats().delta_documents > 0);
    Refusals(table);
    // the table against an index rebuilt from its current documents: the counts meet by value
    Index fresh(2, 0, 0.0, false);
    for (const auto& d : docs) fresh.AddDocument(d.first, d.second.text, d.second.filters);
    const std::vector<BatchQuery> qs = Queries();
    auto got = ExecuteBatch(table, qs);
    auto want = ExecuteBatch(fresh, qs);
    EXPECT(got.has_value() && want.has_value());
    if (got && want)
      for (size_t i = 0; i < qs.size(); ++i) {
        EXPECT((*got)[i].total == (*want)[i].total && (*got)[i].facets.size() == (*want)[i].facets.size());
        for (size_t c = 0; c < (*got)[i].facets.size() && c < (*want)[i].facets.size(); ++c) {
          const bool same = SameFacet((*got)[i].facets[c], (*want)[i].facets[c]);
          EXPECT(same);
          if (!same) std::printf("  delta vs rebuilt: query %zu column %s differs\n", i, qs[i].facet_columns[c].c_str());
        }
      }
  }
  EXPECT(table.Compact().empty());
  EXPECT(table.GetMutationStats().delta_documents == 0);
  CheckEveryPath(table, "after Compact");
  std::printf("%d checks, %d failed\n", g_checked, g_failed);
  return g_failed == 0 ? 0 : 1;
}
