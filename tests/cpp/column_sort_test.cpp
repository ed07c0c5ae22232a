// column_sort_test.cpp — SORT <filter column> through the C++17 shim: BatchQuery::sort_column through ExecuteBatch,
// BatchExecutor (two batches in flight) and MicroBatcher; the reference's own vectors (tests/query/result_sorter_test.cpp,
// restated below with their lines) as tables; name resolution and kQueryInvalidSort; a table with added, updated, removed
// and UpdateFilters-changed documents against an index rebuilt from the current documents; the string-column refusal on a
// delta and its return after Compact(). Expected pages come from the reference's STRING keys (FilterValueToSortKey,
// src/query/result_sorter.cpp:187-217, restated in KeyString) over the result set of the same query without SORT.
// Needs a GPU; built and run by tests/test_gpu_column_sort_shim.py.
#include <algorithm>
#include <climits>
#include <cstdint>
#include <cstdio>
#include <cstring>
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
using mygramdb::query::SortOrder;
using mygramdb::storage::FilterMap;
using mygramdb::storage::FilterValue;
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

static uint64_t g_rng = 777;
static uint32_t Next() {
  g_rng = g_rng * 6364136223846793005ull + 1442695040888963407ull;
  return static_cast<uint32_t>(g_rng >> 33);
}

// ---- the reference's string keys --------------------------------------------------------------------------------------
static std::string Padded(uint64_t v) {  // ToZeroPaddedString, width 20 (:67-92)
  char buf[32];
  std::snprintf(buf, sizeof buf, "%020llu", static_cast<unsigned long long>(v));
  return buf;
}
static std::string KeyString(const FilterValue& val) {  // FilterValueToSortKey (:187-217)
  return std::visit(
      [](const auto& a) -> std::string {
        using T = std::decay_t<decltype(a)>;
        if constexpr (std::is_same_v<T, std::monostate>) return "";
        else if constexpr (std::is_same_v<T, bool>) return a ? "1" : "0";
        else if constexpr (std::is_same_v<T, std::string>) return a;
        else if constexpr (std::is_same_v<T, TimeValue>) return Padded(static_cast<uint64_t>(a.seconds) ^ (1ull << 63));
        else if constexpr (std::is_same_v<T, double>) {
          uint64_t bits;
          std::memcpy(&bits, &a, 8);
          return Padded((bits >> 63) ? ~bits : bits ^ (1ull << 63));
        } else if constexpr (std::is_signed_v<T>) return Padded(static_cast<uint64_t>(static_cast<int64_t>(a)) ^ (1ull << 63));
        else {
          const uint64_t v = static_cast<uint64_t>(a);
          return v <= static_cast<uint64_t>(INT64_MAX) ? Padded(v ^ (1ull << 63)) : Padded(v);
        }
      },
      val);
}

struct DocRow {
  std::string text;
  FilterMap filters;
};
using Docs = std::map<DocId, DocRow>;

// CompareSortEntries (:47-54) + ApplyOffsetLimit (:227-232); limit 0 = all on this layer
static std::vector<DocId> Model(const Docs& docs, const std::vector<DocId>& result_set, const std::string& column, SortOrder order,
                                uint32_t limit, uint32_t offset) {
  std::vector<std::pair<std::string, DocId>> e;
  for (DocId d : result_set) {
    const auto& f = docs.at(d).filters;
    const auto it = f.find(column);
    e.emplace_back(it == f.end() ? std::string() : KeyString(it->second), d);
  }
  std::sort(e.begin(), e.end());
  if (order == SortOrder::DESC) std::reverse(e.begin(), e.end());
  const size_t lo = std::min<size_t>(offset, e.size());
  const size_t hi = limit == 0 ? e.size() : std::min<size_t>(lo + limit, e.size());
  std::vector<DocId> out;
  for (size_t i = lo; i < hi; ++i) out.push_back(e[i].second);
  return out;
}

static BatchQuery Q(std::vector<std::string> terms, const std::string& column, SortOrder order, uint32_t limit, uint32_t offset = 0) {
  BatchQuery q;
  q.terms = std::move(terms);
  q.sort_column = column;
  q.order = order;
  q.limit = limit;
  q.offset = offset;
  return q;
}

static std::unique_ptr<QueryNode> Term(const char* t) { return std::make_unique<QueryNode>(std::string(t)); }
static std::unique_ptr<QueryNode> Node(NodeType t, std::unique_ptr<QueryNode> a, std::unique_ptr<QueryNode> b = nullptr) {
  auto n = std::make_unique<QueryNode>(t);
  n->children.push_back(std::move(a));
  if (b) n->children.push_back(std::move(b));
  return n;
}

// ---- the reference's vectors as tables ----------------------------------------------------------------------------------
struct Vector {
  int line;  // tests/query/result_sorter_test.cpp
  std::vector<FilterValue> values;  // documents 1..n
  SortOrder order;
  uint32_t limit, offset;
  std::vector<DocId> expect;
  int expect_size;  // -1: `expect` is the page
};

static void GoldenVectors() {
  const double nz = -0.0;
  std::vector<FilterValue> hundred;
  for (int i = 1; i <= 100; ++i) hundred.push_back(int32_t(i));
  const std::vector<FilterValue> ext = {int64_t(INT64_MAX), int64_t(0), int64_t(INT64_MIN), int64_t(-1), int64_t(1)};
  const std::vector<Vector> vs = {
      {99, {int32_t(100), int32_t(50), int32_t(200)}, SortOrder::DESC, 10, 0, {3, 1, 2}, -1},
      {131, {int32_t(10), int32_t(10), int32_t(10)}, SortOrder::ASC, 10, 0, {1, 2, 3}, -1},
      {674, hundred, SortOrder::ASC, 100, UINT32_MAX - 50, {}, -1},
      {674, hundred, SortOrder::ASC, 1, UINT32_MAX, {}, -1},
      {674, hundred, SortOrder::ASC, 5, 10, {}, 5},
      {1013, {-20.0, -5.0, -1.0}, SortOrder::ASC, 100, 0, {1, 2, 3}, -1},
      {1040, {-20.0, -5.0, -1.0}, SortOrder::DESC, 100, 0, {3, 2, 1}, -1},
      {1067, {-10.0, 0.0, 5.0, -3.0, 100.0}, SortOrder::ASC, 100, 0, {1, 4, 2, 3, 5}, -1},
      {1098, {nz, 0.0}, SortOrder::ASC, 100, 0, {1, 2}, -1},
      {1138, ext, SortOrder::ASC, 100, 0, {3, 4, 2, 5, 1}, -1},
      {1138, ext, SortOrder::DESC, 100, 0, {1, 5, 2, 4, 3}, -1},
      {1183, {int32_t(INT32_MAX), int32_t(0), int32_t(INT32_MIN)}, SortOrder::ASC, 100, 0, {3, 2, 1}, -1},
      {1210, {int64_t(-999), int64_t(50), int64_t(-100), int64_t(999), int64_t(0), int64_t(-1)}, SortOrder::ASC, 100, 0,
       {1, 3, 6, 5, 2, 4}, -1},
  };
  for (const Vector& v : vs) {
    Index table(2, 0, 0.0, false);
    for (size_t i = 0; i < v.values.size(); ++i) table.AddDocument(static_cast<DocId>(i + 1), "test doc", {{"score", v.values[i]}});
    auto r = ExecuteBatch(table, {Q({"test"}, "score", v.order, v.limit, v.offset)});
    EXPECT(r.has_value());
    if (!r) {
      std::printf("  vector :%d: %s\n", v.line, r.error().message().c_str());
      continue;
    }
    const bool ok = v.expect_size >= 0 ? (*r)[0].results.size() == static_cast<size_t>(v.expect_size) : (*r)[0].results == v.expect;
    EXPECT(ok);
    if (!ok) std::printf("  vector :%d differs\n", v.line);
    EXPECT((*r)[0].total == v.values.size());
  }
  {  // :422 InvalidColumn, and the name rules of :516-520
    Index table(2, 0, 0.0, false);
    table.AddDocument(1, "test doc", {{"score", int32_t(100)}});
    table.AddDocument(2, "test doc", {{"score", int32_t(50)}});
    auto bad = ExecuteBatch(table, {Q({"test"}, "nonexistent_column", SortOrder::DESC, 10)});
    EXPECT(!bad.has_value() && bad.error().code() == ErrorCode::kQueryInvalidSort);
    if (!bad) {
      EXPECT(bad.error().message().find("not found") != std::string::npos);
      EXPECT(bad.error().message().find("nonexistent_column") != std::string::npos);
    }
    auto ci = ExecuteBatch(table, {Q({"test"}, "SCORE", SortOrder::DESC, 10), Q({"test"}, "score", SortOrder::ASC, 10)});
    EXPECT(ci.has_value() && (*ci)[0].results == std::vector<DocId>({1, 2}) && (*ci)[1].results == std::vector<DocId>({2, 1}));
    // FACET ignores the sort fields (ExecuteFacetPipeline), a misspelt sort column included
    auto facet = ExecuteFacet(table, Q({"test"}, "nonexistent_column", SortOrder::DESC, 10), "score");
    EXPECT(facet.has_value() && facet->matched_documents == 2);
    BatchQuery both = Q({"test"}, "score", SortOrder::DESC, 10);
    both.sort_by_score = true;
    auto two = ExecuteBatch(table, {both});
    EXPECT(!two.has_value() && two.error().code() == ErrorCode::kInvalidArgument);
  }
}

// ---- a larger table ---------------------------------------------------------------------------------------------------------
static const char* const kWords[] = {"alpha", "beta", "gamma", "delta", "omega", "theta", "lambda", "sigma", "kappa"};
static const char* const kNames[] = {"", "ann", "Ann", "bob", "zoe", "\xC3\xA9mile"};
static const char* const kColumns[] = {"score", "price", "flag", "ts", "big", "name"};

static DocRow Row(const char* extra = nullptr) {
  DocRow r;
  const uint32_t n = 2 + Next() % 5;
  for (uint32_t i = 0; i < n; ++i) {
    if (!r.text.empty()) r.text += ' ';
    r.text += kWords[Next() % 9];
  }
  if (extra) r.text += std::string(" ") + extra;
  if (Next() % 10 != 0) r.filters["score"] = int32_t(static_cast<int32_t>(Next() % 7) - 3);  // heavy ties, some NULL
  static const double prices[] = {0.0, -0.0, 1.5, -1.5, 1e300, -1e300, 5e-324};
  if (Next() % 8 != 0) r.filters["price"] = prices[Next() % 7];
  r.filters["flag"] = Next() % 2 == 0;
  r.filters["ts"] = TimeValue{static_cast<int64_t>(Next() % 2000) - 1000};
  static const uint64_t bigs[] = {0, 1, static_cast<uint64_t>(INT64_MAX), static_cast<uint64_t>(INT64_MAX) + 1, UINT64_MAX};
  r.filters["big"] = bigs[Next() % 5];
  if (Next() % 6 != 0) r.filters["name"] = std::string(kNames[Next() % 6]);
  return r;
}

static std::vector<BatchQuery> Shapes() {  // without SORT, limit 0, ascending doc ids: the result sets
  std::vector<BatchQuery> qs;
  BatchQuery a;
  a.terms = {"alpha"};
  qs.push_back(a);
  BatchQuery b;
  b.terms = {"beta"};
  b.not_terms = {"kappa"};
  qs.push_back(b);
  BatchQuery e;
  e.ast = Node(NodeType::AND, Node(NodeType::OR, Term("alpha"), Term("gamma")), Node(NodeType::NOT, Term("omega")));
  qs.push_back(e);
  BatchQuery z;
  z.terms = {"zzqx"};
  qs.push_back(z);
  for (BatchQuery& q : qs) {
    q.limit = 0;
    q.order = SortOrder::ASC;
  }
  return qs;
}

static const std::pair<uint32_t, uint32_t> kPages[] = {{10, 0}, {100, 7}, {0, 0}, {1024, 0}, {1000, 24}, {1000, 25}, {50, 100000}};

static std::vector<BatchQuery> Sorted(const std::vector<const char*>& columns) {
  std::vector<BatchQuery> qs;
  for (const BatchQuery& shape : Shapes())
    for (const char* col : columns)
      for (SortOrder o : {SortOrder::ASC, SortOrder::DESC})
        for (const auto& page : kPages) {
          BatchQuery q = shape;
          q.sort_column = col;
          q.order = o;
          q.limit = page.first;
          q.offset = page.second;
          qs.push_back(std::move(q));
        }
  return qs;
}

// every sorted page of `got` against the model over the result sets `base` (the same table, no SORT)
static void CheckAgainstModel(const Docs& docs, const std::vector<BatchQuery>& qs, const std::vector<BatchResult>& got,
                              const std::vector<BatchResult>& base, size_t per_shape, const char* what) {
  size_t nonempty = 0;
  for (size_t i = 0; i < qs.size(); ++i) {
    const BatchResult& b = base[i / per_shape];
    const std::vector<DocId> want = Model(docs, b.results, qs[i].sort_column, qs[i].order, qs[i].limit, qs[i].offset);
    const bool same = got[i].results == want && got[i].total == b.total && got[i].total_candidates == b.total_candidates &&
                      got[i].after_intersection == b.after_intersection && got[i].after_not == b.after_not &&
                      got[i].after_filters == b.after_filters;
    EXPECT(same);
    if (!same)
      std::printf("  %s: query %zu (%s %s limit %u offset %u) differs: %zu/%zu docs, total %llu/%llu\n", what, i,
                  qs[i].sort_column.c_str(), qs[i].order == SortOrder::ASC ? "ASC" : "DESC", qs[i].limit, qs[i].offset,
                  got[i].results.size(), want.size(), static_cast<unsigned long long>(got[i].total),
                  static_cast<unsigned long long>(b.total));
    bool zero = true;
    for (double s : got[i].scores) zero = zero && s == 0.0;
    EXPECT(zero);
    nonempty += want.empty() ? 0 : 1;
  }
  EXPECT(nonempty * 2 > qs.size());
}

static std::unique_ptr<Index> Fresh(const Docs& docs) {
  auto fresh = std::make_unique<Index>(2, 0, 0.0, false);
  for (const auto& d : docs) fresh->AddDocument(d.first, d.second.text, d.second.filters);
  return fresh;
}

// A NULL on one side of a table with a delta and a value whose 64-bit key is NULL's (INT64_MIN; the all-ones double)
// on the other: neither column is marked by itself, their merged runs would tie the two. Refused while both are there,
// in either arrangement; exact again once one of the two ingredients is gone, with the delta and after Compact(). (A
// table that keeps both is refused after Compact() too: then the one column holds both.)
static void CrossSideCollision() {
  double ones;
  const uint64_t all = ~0ull;
  std::memcpy(&ones, &all, 8);
  for (int arrangement = 0; arrangement < 4; ++arrangement) {
    const bool zero_in_main = arrangement % 2 == 0, as_double = arrangement >= 2;
    const FilterValue zero = as_double ? FilterValue(ones) : FilterValue(int64_t(INT64_MIN));
    auto plain = [&](DocId d) { return as_double ? FilterValue(static_cast<double>(d % 7) - 3.0) : FilterValue(int64_t(d % 7) - 3); };
    Docs docs;
    Index table(2, 0, 0.0, false);
    for (DocId d = 1; d <= 300; ++d) {
      DocRow r;
      r.text = "alpha beta";
      if (d == 10) {
        if (zero_in_main) r.filters["v"] = zero;  // main: the zero key, no NULL | main: a NULL, no zero key
      } else {
        r.filters["v"] = plain(d);
      }
      docs[d] = r;
      table.AddDocument(d, r.text, r.filters);
    }
    const std::vector<BatchQuery> qs = {Q({"alpha"}, "v", SortOrder::ASC, 10), Q({"alpha"}, "v", SortOrder::DESC, 10),
                                        Q({"alpha"}, "v", SortOrder::ASC, 0), Q({"alpha"}, "v", SortOrder::DESC, 2000, 3)};
    auto check = [&](const char* what) {
      std::vector<BatchQuery> shape = {Q({"alpha"}, "", SortOrder::ASC, 0)};
      auto base = ExecuteBatch(table, shape);
      auto got = ExecuteBatch(table, qs);
      EXPECT(base.has_value() && got.has_value());
      if (!got) std::printf("  collision %d, %s: %s\n", arrangement, what, got.error().message().c_str());
      if (!base || !got) return;
      for (size_t i = 0; i < qs.size(); ++i) {
        const bool same = (*got)[i].results == Model(docs, (*base)[0].results, "v", qs[i].order, qs[i].limit, qs[i].offset);
        EXPECT(same);
        if (!same) std::printf("  collision %d, %s: query %zu differs\n", arrangement, what, i);
      }
    };
    check("static");  // one ingredient only: exact
    // the other ingredient arrives in the delta: document 7 moves there by UpdateFilters
    FilterMap other;
    if (!zero_in_main) other["v"] = zero;  // (zero_in_main: no value at all = NULL)
    EXPECT(table.UpdateFilters(7, other));
    docs[7].filters = other;
    auto refused = ExecuteBatch(table, qs);
    EXPECT(table.GetMutationStats().delta_documents > 0);
    EXPECT(!refused.has_value() && refused.error().code() == ErrorCode::kNotImplemented);
    if (!refused) EXPECT(refused.error().message().find("INT64_MIN") != std::string::npos);
    {
      BatchExecutor ex(table);
      auto t = ex.Submit(qs);
      EXPECT(t.has_value());
      if (t) {
        auto r = ex.Wait(*t);
        EXPECT(!r.has_value() && r.error().code() == ErrorCode::kNotImplemented);
      }
    }
    auto unsorted = ExecuteBatch(table, {Q({"alpha"}, "", SortOrder::ASC, 0)});  // the table itself still serves
    EXPECT(unsorted.has_value() && (*unsorted)[0].total == 300);
    // the delta's document takes an ordinary value: nothing collides any more
    FilterMap fine;
    fine["v"] = plain(7);
    EXPECT(table.UpdateFilters(7, fine));
    docs[7].filters = fine;
    check("with a delta");
    EXPECT(table.GetMutationStats().delta_documents > 0);
    EXPECT(table.Compact().empty());
    check("after Compact");
  }
}

int main() {
  GoldenVectors();
  CrossSideCollision();
  Docs docs;
  Index table(2, 0, 0.0, false);
  for (DocId d = 1; d <= 6000; ++d) {
    docs[d] = Row();
    table.AddDocument(d, docs[d].text, docs[d].filters);
  }
  const std::vector<const char*> all(kColumns, kColumns + 6), numeric(kColumns, kColumns + 5);
  const size_t per_all = 6 * 2 * 7, per_numeric = 5 * 2 * 7;
  {  // ---- a static table: ExecuteBatch, BatchExecutor with two batches in flight, MicroBatcher ----
    auto base = ExecuteBatch(table, Shapes());
    const std::vector<BatchQuery> qs = Sorted(all);
    auto got = ExecuteBatch(table, qs);
    EXPECT(base.has_value() && got.has_value());
    if (!got) std::printf("  static: %s\n", got.error().message().c_str());
    if (!base || !got) return 1;
    EXPECT((*base)[0].total > 1100);  // pages past 1024 exist
    CheckAgainstModel(docs, qs, *got, *base, per_all, "ExecuteBatch");
    {
      BatchExecutor::Options o;
      o.depth = 2;
      BatchExecutor ex(table, o);
      std::vector<BatchQuery> mixed = qs;  // column-sorted pages beside score and doc-id pages
      BatchQuery s;
      s.terms = {"alpha"};
      s.sort_by_score = true;
      s.limit = 10;
      mixed.push_back(s);
      auto ta = ex.Submit(mixed);
      auto tb = ex.Submit(qs);
      EXPECT(ta.has_value() && tb.has_value());
      if (ta && tb) {
        auto ra = ex.Wait(*ta);
        auto rb = ex.Wait(*tb);
        EXPECT(ra.has_value() && rb.has_value());
        if (ra && rb) {
          EXPECT(ra->back().results.size() == 10 && ra->back().scores.size() == 10 && ra->back().scores[0] > 0.0);
          ra->pop_back();
          CheckAgainstModel(docs, qs, *ra, *base, per_all, "BatchExecutor a");
          CheckAgainstModel(docs, qs, *rb, *base, per_all, "BatchExecutor b");
        }
      }
    }
    {
      MicroBatcher::Options mo;
      MicroBatcher mb(table, mo);
      for (size_t i : {size_t(0), size_t(17), qs.size() - 3}) {
        auto r = mb.Search(qs[i]);
        EXPECT(r.has_value() && r->results == (*got)[i].results && r->total == (*got)[i].total);
      }
      auto bad = mb.Search(Q({"alpha"}, "nope", SortOrder::ASC, 10));
      EXPECT(!bad.has_value() && bad.error().code() == ErrorCode::kQueryInvalidSort);
    }
  }
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
    const DocRow nr = Row(k % 4 == 0 ? "zzqx" : nullptr);
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
    docs[d] = Row(d % 5 == 0 ? "zzqx" : nullptr);
    EXPECT(table.AddDocument(d, docs[d].text, docs[d].filters));
  }
  int back = 0;
  for (DocId d = 1; d <= 6000 && back < 10; ++d)
    if (!docs.count(d)) {
      docs[d] = Row();
      EXPECT(table.AddDocument(d, docs[d].text, docs[d].filters));
      ++back;
    }
  {
    auto base = ExecuteBatch(table, Shapes());  // (applies the mutations)
    EXPECT(base.has_value());
    EXPECT(table.GetMutationStats().delta_documents > 0);
    const std::vector<BatchQuery> qs = Sorted(numeric);
    auto got = ExecuteBatch(table, qs);
    const std::unique_ptr<Index> fresh = Fresh(docs);
    auto want = ExecuteBatch(*fresh, qs);
    EXPECT(got.has_value() && want.has_value());
    if (!got) std::printf("  changed table: %s\n", got.error().message().c_str());
    if (base && got && want) {
      for (size_t i = 0; i < qs.size(); ++i) {
        const bool same = (*got)[i].results == (*want)[i].results && (*got)[i].total == (*want)[i].total;
        EXPECT(same);
        if (!same) std::printf("  changed table: query %zu (%s) differs from the rebuilt index\n", i, qs[i].sort_column.c_str());
      }
      CheckAgainstModel(docs, qs, *got, *base, per_numeric, "changed table");
      BatchExecutor ex(table);
      auto t = ex.Submit(qs);
      EXPECT(t.has_value());
      if (t) {
        auto r = ex.Wait(*t);
        EXPECT(r.has_value());
        if (r) CheckAgainstModel(docs, qs, *r, *base, per_numeric, "changed table, BatchExecutor");
      }
    }
    // a string column across a delta: the two dictionaries' ranks do not compare
    auto refused = ExecuteBatch(table, {Q({"alpha"}, "name", SortOrder::ASC, 10)});
    EXPECT(!refused.has_value() && refused.error().code() == ErrorCode::kNotImplemented);
    EXPECT(table.Compact().empty());
    EXPECT(table.GetMutationStats().delta_documents == 0);
    auto base2 = ExecuteBatch(table, Shapes());
    const std::vector<BatchQuery> qa = Sorted(all);
    auto after = ExecuteBatch(table, qa);
    EXPECT(base2.has_value() && after.has_value());
    if (!after) std::printf("  after Compact: %s\n", after.error().message().c_str());
    if (base2 && after) CheckAgainstModel(docs, qa, *after, *base2, per_all, "after Compact");
  }
  std::printf("%d checks, %d failed\n", g_checked, g_failed);
  return g_failed == 0 ? 0 : 1;
}
