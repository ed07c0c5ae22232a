// primary_key_sort_test.cpp — SORT by primary key through the C++17 shim: BatchQuery::sort_primary_key (and sort_column
// given as the primary-key column's name) through ExecuteBatch, BatchExecutor (two batches in flight) and MicroBatcher, on
// a table with a delta index and after Compact(). Three tables: main and delta with numeric keys only (the runs merge as
// numbers), a numeric main index beside a delta that holds one string key (merged by key string, the main side's digits
// derived from the number), and string keys on both sides (two dictionaries). Expected pages come from the reference's
// string keys (GetSortKey's primary-key branch, src/query/result_sorter.cpp:239-262, restated in KeyOf) over the result
// set of the same query without SORT, on the table's current documents.
// Needs a GPU; built and run by tests/test_gpu_primary_key_sort_shim.py.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <functional>
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
using mygramdb::query::NodeType;
using mygramdb::query::QueryNode;
using mygramdb::query::SortOrder;
using mygramdb::storage::FilterMap;
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

// ---- the reference's key (:239-262) ----
static std::string Padded(uint64_t v) {  // ToZeroPaddedString, width 20 (:67-92)
  char buf[32];
  std::snprintf(buf, sizeof buf, "%020llu", static_cast<unsigned long long>(v));
  return buf;
}
static std::string KeyOf(DocId doc, const std::optional<std::string>& pk) {
  if (!pk) return Padded(doc);  // :258-261
  bool digits = !pk->empty();
  for (unsigned char c : *pk) digits = digits && c >= '0' && c <= '9';
  if (digits) {  // :247-253
    unsigned __int128 v = 0;
    bool fits = true;
    for (unsigned char c : *pk) {
      v = v * 10 + (c - '0');
      if (v > UINT64_MAX) {
        fits = false;
        break;
      }
    }
    if (fits) return Padded(static_cast<uint64_t>(v));
  }
  return *pk;  // :256
}

struct DocRow {
  std::string text;
  std::optional<std::string> pk;
};
using Docs = std::map<DocId, DocRow>;

// CompareSortEntries (:47-54) + ApplyOffsetLimit (:227-232); limit 0 = all on this layer
static std::vector<DocId> Model(const Docs& docs, const std::vector<DocId>& result_set, SortOrder order, uint32_t limit, uint32_t offset) {
  std::vector<std::pair<std::string, DocId>> e;
  for (DocId d : result_set) e.emplace_back(KeyOf(d, docs.at(d).pk), d);
  std::sort(e.begin(), e.end());
  if (order == SortOrder::DESC) std::reverse(e.begin(), e.end());
  const size_t lo = std::min<size_t>(offset, e.size());
  const size_t hi = limit == 0 ? e.size() : std::min<size_t>(lo + limit, e.size());
  std::vector<DocId> out;
  for (size_t i = lo; i < hi; ++i) out.push_back(e[i].second);
  return out;
}

static std::unique_ptr<QueryNode> Term(const char* t) { return std::make_unique<QueryNode>(std::string(t)); }

// the search parts: most documents of both sides; main-only and delta-only words (one side's run empty); a tree
static std::vector<BatchQuery> Shapes() {
  std::vector<BatchQuery> qs(4);
  qs[0].terms = {"alpha"};
  qs[1].terms = {"mainword"};
  qs[2].terms = {"deltaword"};
  auto tree = std::make_shared<QueryNode>(NodeType::OR);
  tree->children.push_back(Term("alpha"));
  tree->children.push_back(Term("beta"));
  qs[3].ast = std::move(tree);
  for (BatchQuery& q : qs) {
    q.order = SortOrder::ASC;
    q.limit = 0;
  }
  return qs;
}
// limit, offset: unbounded; a small page; a window that straddles both sides inside the fused selection; the full sort
static const std::pair<uint32_t, uint32_t> kPages[] = {{0, 0}, {10, 0}, {400, 290}, {1000, 700}, {10, 100000}};
static std::vector<BatchQuery> Sorted(bool by_name) {
  std::vector<BatchQuery> qs;
  for (const BatchQuery& s : Shapes())
    for (SortOrder order : {SortOrder::ASC, SortOrder::DESC})
      for (const auto& page : kPages) {
        BatchQuery q = s;
        if (by_name) q.sort_column = "ID";  // the primary-key column's name in another letter case
        else q.sort_primary_key = true;
        q.order = order;
        q.limit = page.first;
        q.offset = page.second;
        qs.push_back(std::move(q));
      }
  return qs;
}
static void Check(const Docs& docs, const std::vector<BatchQuery>& qs, const std::vector<BatchResult>& got,
                  const std::vector<BatchResult>& base, const char* what) {
  const size_t per = 2 * (sizeof kPages / sizeof kPages[0]);
  EXPECT(got.size() == qs.size());
  for (size_t i = 0; i < qs.size() && i < got.size(); ++i) {
    const BatchResult& b = base[i / per];
    const std::vector<DocId> want = Model(docs, b.results, qs[i].order, qs[i].limit, qs[i].offset);
    const bool same = got[i].results == want && got[i].total == b.total;
    EXPECT(same);
    if (!same)
      std::printf("  %s: query %zu (shape %zu, %s, limit %u, offset %u): %zu ids, %zu wanted\n", what, i, i / per,
                  qs[i].order == SortOrder::ASC ? "ASC" : "DESC", qs[i].limit, qs[i].offset, got[i].results.size(), want.size());
    for (double s : got[i].scores) EXPECT(s == 0.0);
  }
}

static std::string Text(DocId d, bool delta) {
  std::string t = "w" + std::to_string(d);
  if (d % 5 != 0) t += " alpha";
  if (d % 2 == 0) t += " beta";
  t += delta ? " deltaword" : " mainword";
  return t;
}

using KeyFn = std::function<std::optional<std::string>(DocId)>;
constexpr DocId kMain = 1500, kDeltaFirst = 2001, kDeltaLast = 2500;

static void Variant(const char* name, const KeyFn& main_key, const KeyFn& delta_key) {
  std::printf("-- %s\n", name);
  Docs docs;
  Index table(2, 0, 0.0, false);
  table.SetPrimaryKeyColumn("id");
  auto add = [&](DocId d, bool delta, const std::optional<std::string>& pk) {
    docs[d] = DocRow{Text(d, delta), pk};
    if (pk) EXPECT(table.AddDocument(d, docs[d].text, {}, *pk));
    else EXPECT(table.AddDocument(d, docs[d].text));
  };
  for (DocId d = 1; d <= kMain; ++d) add(d, false, main_key(d));
  const std::vector<BatchQuery> qs = Sorted(false), by_name = Sorted(true);
  {  // ---- one index ----
    auto base = ExecuteBatch(table, Shapes());
    auto got = ExecuteBatch(table, qs);
    EXPECT(base.has_value() && got.has_value());
    if (!got) std::printf("  static: %s\n", got.error().message().c_str());
    if (!base || !got) return;
    EXPECT((*base)[0].total > 1100);
    Check(docs, qs, *got, *base, "static table");
  }
  // ---- changes: a delta of new documents; updated main documents keep their keys; removals on both sides ----
  for (DocId d = kDeltaFirst; d <= kDeltaLast; ++d) add(d, true, delta_key(d));
  docs[20].text = Text(20, false) + " changed";
  table.UpdateDocument(20, Text(20, false), docs[20].text);  // moves to the delta, with its key
  EXPECT(table.UpdateFilters(30, FilterMap{}));               // so does a document whose filter values change
  table.RemoveDocument(40, docs[40].text);
  docs.erase(40);
  table.RemoveDocument(2010, docs[2010].text);
  docs.erase(2010);
  auto base = ExecuteBatch(table, Shapes());  // (applies the mutations)
  EXPECT(base.has_value());
  if (!base) return;
  EXPECT(table.GetMutationStats().delta_documents == kDeltaLast - kDeltaFirst + 2);  // 500 added - 1 removed + the two updated
  EXPECT((*base)[0].total > 1500 && (*base)[1].total >= 300 && (*base)[2].total >= 300);  // >= 300 matches on each side
  auto got = ExecuteBatch(table, qs);
  EXPECT(got.has_value());
  if (!got) {
    std::printf("  with a delta: %s\n", got.error().message().c_str());
    return;
  }
  Check(docs, qs, *got, *base, "with a delta");
  {  // "007" in the main index (doc 7) and "7" in the delta (doc 2003): one sort key, neighbours, ordered by table id
    EXPECT(docs.at(7).pk == std::optional<std::string>("007") && docs.at(2003).pk == std::optional<std::string>("7"));
    const size_t per = sizeof kPages / sizeof kPages[0];
    const std::vector<DocId>& asc = (*got)[0].results;         // shape 0, ASC, limit 0
    const std::vector<DocId>& desc = (*got)[per].results;      // shape 0, DESC, limit 0
    const auto a = std::find(asc.begin(), asc.end(), DocId(7));
    const auto d = std::find(desc.begin(), desc.end(), DocId(2003));
    EXPECT(a != asc.end() && a + 1 != asc.end() && *(a + 1) == 2003);
    EXPECT(d != desc.end() && d + 1 != desc.end() && *(d + 1) == 7);
    // the window [290, 690) holds documents of both sides
    const std::vector<DocId>& window = (*got)[2].results;
    const size_t from_delta = std::count_if(window.begin(), window.end(), [](DocId x) { return x >= kDeltaFirst || x == 20 || x == 30; });
    EXPECT(window.size() == 400 && from_delta > 0 && from_delta < window.size());
  }
  {  // the primary-key column by name, in another letter case: the same pages
    auto named = ExecuteBatch(table, by_name);
    EXPECT(named.has_value());
    if (named)
      for (size_t i = 0; i < qs.size(); ++i) EXPECT((*named)[i].results == (*got)[i].results && (*named)[i].total == (*got)[i].total);
    BatchQuery both = qs[1];
    both.sort_by_score = true;
    auto bad = ExecuteBatch(table, {both});
    EXPECT(!bad.has_value() && bad.error().code() == ErrorCode::kInvalidArgument);
    both = by_name[1];
    both.sort_by_score = true;
    bad = ExecuteBatch(table, {both});
    EXPECT(!bad.has_value() && bad.error().code() == ErrorCode::kInvalidArgument);
  }
  {  // BatchExecutor with two batches in flight, key-sorted pages beside a score page and a doc-id page
    BatchExecutor::Options o;
    o.depth = 2;
    BatchExecutor ex(table, o);
    std::vector<BatchQuery> mixed = qs;
    BatchQuery s;
    s.terms = {"alpha"};
    s.sort_by_score = true;
    s.limit = 10;
    mixed.push_back(s);
    BatchQuery p;
    p.terms = {"alpha"};
    p.limit = 20;
    mixed.push_back(p);
    auto ta = ex.Submit(mixed);
    auto tb = ex.Submit(qs);
    EXPECT(ta.has_value() && tb.has_value());
    if (ta && tb) {
      auto ra = ex.Wait(*ta);
      auto rb = ex.Wait(*tb);
      EXPECT(ra.has_value() && rb.has_value());
      if (!ra) std::printf("  BatchExecutor: %s\n", ra.error().message().c_str());
      if (ra && rb) {
        EXPECT(ra->back().results.size() == 20 && ra->back().results[0] == kDeltaLast - 1);  // (doc 2500 holds no "alpha")
        ra->pop_back();
        EXPECT(ra->back().results.size() == 10 && ra->back().scores.size() == 10 && ra->back().scores[0] > 0.0);
        ra->pop_back();
        Check(docs, qs, *ra, *base, "BatchExecutor a");
        Check(docs, qs, *rb, *base, "BatchExecutor b");
      }
    }
  }
  {
    MicroBatcher::Options mo;
    MicroBatcher mb(table, mo);
    for (size_t i : {size_t(0), size_t(7), qs.size() - 3}) {
      auto r = mb.Search(qs[i]);
      EXPECT(r.has_value() && r->results == (*got)[i].results && r->total == (*got)[i].total);
    }
    auto r = mb.Search(by_name[2]);
    EXPECT(r.has_value() && r->results == (*got)[2].results);
  }
  // ---- Compact(): the keys go into the rebuilt index, the pages stay ----
  EXPECT(table.Compact().empty());
  EXPECT(table.GetMutationStats().delta_documents == 0);
  auto base2 = ExecuteBatch(table, Shapes());
  auto after = ExecuteBatch(table, qs);
  EXPECT(base2.has_value() && after.has_value());
  if (!after) std::printf("  after Compact: %s\n", after.error().message().c_str());
  if (base2 && after) {
    Check(docs, qs, *after, *base2, "after Compact");
    for (size_t i = 0; i < qs.size(); ++i) EXPECT((*after)[i].results == (*got)[i].results);
  }
}

int main() {
  auto shuffled = [](DocId d) { return std::to_string((static_cast<uint64_t>(d) * 7919u) % 100003u + 10); };
  const KeyFn numeric_main = [&](DocId d) -> std::optional<std::string> {
    if (d == 7) return "007";
    if (d == 11) return "18446744073709551615";
    if (d == 12) return "9223372036854775808";
    if (d % 97 == 0) return std::nullopt;  // no key: the doc id
    return shuffled(d);
  };
  const KeyFn numeric_delta = [&](DocId d) -> std::optional<std::string> {
    if (d == 2003) return "7";
    if (d == 2005) return "0";
    if (d % 89 == 0) return std::nullopt;
    return shuffled(d);
  };
  Variant("numeric main index, numeric delta", numeric_main, numeric_delta);
  Variant("numeric main index, a delta with one string key", numeric_main, [&](DocId d) -> std::optional<std::string> {
    if (d == 2100) return "pk2100";
    return numeric_delta(d);
  });
  auto strings = [&](DocId d) -> std::optional<std::string> {
    switch (d % 7) {
      case 0: return "pk" + std::to_string(d);           // "pk10" before "pk9"
      case 1: return std::string("\x80\xff") + std::to_string(d % 50);  // bytes past 0x7f, with ties
      case 2: return "18446744073709551616";             // overflows: raw, and tied across the table
      case 3: return std::string();                      // ""
      case 4: return "pk";                               // a prefix of the others
      case 5: return std::nullopt;
      default: return shuffled(d);                       // numeric keys inside a dictionary of strings
    }
  };
  Variant("string keys on both sides",
          [&](DocId d) -> std::optional<std::string> { return d == 7 ? std::optional<std::string>("007") : strings(d); },
          [&](DocId d) -> std::optional<std::string> { return d == 2003 ? std::optional<std::string>("7") : strings(d); });
  std::printf("%d checks, %d failed\n", g_checked, g_failed);
  return g_failed == 0 ? 0 : 1;
}
