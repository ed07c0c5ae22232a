// batch_conditions_test.cpp — FILTER conditions whose literal changes with every request, through BatchExecutor: range
// conditions with a fresh threshold per query and `=` with literals the column lacks are evaluated per batch (the main
// index's device memory stays where it was), `=` on a string value that exists keeps ONE cached row, and the same range
// conditions on a table with a delta return what an index rebuilt from the current documents returns. Results are checked
// per document from the host values (ApplyFilters semantics). Needs a GPU; built and run by
// tests/test_gpu_batch_conditions_shim.py.
#include <cstdint>
#include <cstdio>
#include <map>
#include <string>
#include <utility>
#include <vector>

#include "../../mygram-db_amd/csrc/shim/mygram_shim.hpp"

using mygramdb::index::DocId;
using mygramdb::index::Index;
using mygramdb::query::FilterCondition;
using mygramdb::query::FilterOp;
using mygramdb::query::SortOrder;
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

static uint64_t g_rng = 777;
static uint32_t Next() {
  g_rng = g_rng * 6364136223846793005ull + 1442695040888963407ull;
  return static_cast<uint32_t>(g_rng >> 33);
}
static const char* const kWords[] = {"alpha", "beta", "gamma", "delta", "omega", "theta"};
static const char* const kCats[] = {"tech", "food", "music"};

struct Doc {
  std::string text;
  int64_t stamp = 0;
  std::string cat;
};
static Doc MakeDoc() {
  Doc d;
  const uint32_t n = 2 + Next() % 4;
  for (uint32_t i = 0; i < n; ++i) d.text += std::string(i ? " " : "") + kWords[Next() % 6];
  d.stamp = static_cast<int64_t>(Next() % 100000) - 20000;
  d.cat = kCats[Next() % 3];
  return d;
}
static FilterMap Filters(const Doc& d) { return FilterMap{{"stamp", FilterValue{d.stamp}}, {"cat", FilterValue{d.cat}}}; }

static BatchQuery Q(const char* term, std::vector<FilterCondition> conds) {
  BatchQuery q;
  q.terms = {term};
  q.order = SortOrder::ASC;
  q.limit = 0;
  q.filter_conditions = std::move(conds);
  return q;
}

// what ApplyFilters leaves of the documents that contain `term`, ascending
static std::vector<DocId> Want(const std::map<DocId, Doc>& docs, const std::string& term, int64_t at_least, const char* cat_eq,
                               const int64_t* stamp_eq) {
  std::vector<DocId> out;
  for (const auto& kv : docs) {
    const Doc& d = kv.second;
    if ((" " + d.text + " ").find(" " + term + " ") == std::string::npos) continue;
    if (d.stamp < at_least) continue;
    if (cat_eq && d.cat != cat_eq) continue;
    if (stamp_eq && d.stamp != *stamp_eq) continue;
    out.push_back(kv.first);
  }
  return out;
}

int main() {
  std::map<DocId, Doc> docs;
  Index table(2, 0, 0.0, false);
  for (DocId d = 1; d <= 20000; ++d) {
    docs[d] = MakeDoc();
    table.AddDocument(d, docs[d].text, Filters(docs[d]));
  }
  BatchExecutor::Options opt;
  BatchExecutor ex(table, opt);
  auto run = [&](std::vector<BatchQuery> qs) {
    auto t = ex.Submit(std::move(qs));
    EXPECT(t.has_value());
    auto r = ex.Wait(*t);
    EXPECT(r.has_value());
    if (!r) std::printf("  Wait: %s\n", r.error().message().c_str());
    return r ? std::move(*r) : std::vector<BatchResult>{};
  };
  // builds the index; the cached rows of `cat = tech` appear here (one per resolution semantics: alone it is the
  // FilterIndex set, beside a range condition the per-document one)
  auto first = run({Q("alpha", {{"cat", FilterOp::EQ, "tech"}}), Q("beta", {{"stamp", FilterOp::GTE, "0"}}),
                    Q("gamma", {{"cat", FilterOp::EQ, "tech"}, {"stamp", FilterOp::GTE, "-5"}})});
  EXPECT(first.size() == 3 && first[0].results == Want(docs, "alpha", INT64_MIN, "tech", nullptr));
  EXPECT(first.size() == 3 && first[1].results == Want(docs, "beta", 0, nullptr, nullptr));
  EXPECT(first.size() == 3 && first[2].results == Want(docs, "gamma", -5, "tech", nullptr));
  const uint64_t before = table.DeviceMemoryBytes();
  EXPECT(before > 0);
  size_t nonempty = 0;
  for (int b = 0; b < 50; ++b) {
    std::vector<BatchQuery> qs;
    std::vector<std::vector<DocId>> want;
    for (int i = 0; i < 64; ++i) {
      const char* term = kWords[(b + i) % 6];
      if (i % 8 == 7) {  // `=` with a literal the column lacks (stamps lie in [-20000, 80000))
        const int64_t lit = 1000000 + b * 64 + i;
        qs.push_back(Q(term, {{"stamp", FilterOp::EQ, std::to_string(lit)}}));
        want.push_back(Want(docs, term, INT64_MIN, nullptr, &lit));
      } else if (i % 8 == 3) {  // a cached string row beside a fresh range condition
        const int64_t t = static_cast<int64_t>(Next() % 100000) - 20000;
        qs.push_back(Q(term, {{"cat", FilterOp::EQ, "tech"}, {"stamp", FilterOp::GTE, std::to_string(t)}}));
        want.push_back(Want(docs, term, t, "tech", nullptr));
      } else {
        const int64_t t = static_cast<int64_t>(Next() % 100000) - 20000;
        qs.push_back(Q(term, {{"stamp", FilterOp::GTE, std::to_string(t)}}));
        want.push_back(Want(docs, term, t, nullptr, nullptr));
      }
    }
    const auto got = run(std::move(qs));
    EXPECT(got.size() == want.size());
    for (size_t i = 0; i < got.size() && i < want.size(); ++i) {
      EXPECT(got[i].results == want[i] && got[i].total == want[i].size());
      nonempty += want[i].empty() ? 0 : 1;
    }
  }
  EXPECT(nonempty > 2000);
  // 3200 fresh literals later the index holds what it held: no row per literal, no retired pool
  EXPECT(table.DeviceMemoryBytes() == before);
  // `=` on a string value that exists is served from its one cached row: a second batch adds none
  run({Q("gamma", {{"cat", FilterOp::EQ, "tech"}}), Q("delta", {{"cat", FilterOp::NE, "tech"}})});
  const uint64_t cached = table.DeviceMemoryBytes();
  const auto again = run({Q("gamma", {{"cat", FilterOp::EQ, "tech"}}), Q("delta", {{"cat", FilterOp::NE, "tech"}})});
  EXPECT(table.DeviceMemoryBytes() == cached);
  EXPECT(again.size() == 2 && again[0].results == Want(docs, "gamma", INT64_MIN, "tech", nullptr));

  // the same range conditions on a table with a delta: equal to an index rebuilt from the current documents
  for (int k = 0; k < 120; ++k) {
    const DocId d = 1 + Next() % 20000;
    if (!docs.count(d)) continue;
    if (k % 3 == 0) {
      table.RemoveDocument(d, docs[d].text);
      docs.erase(d);
    } else {
      Doc nd = MakeDoc();
      nd.stamp = docs[d].stamp;  // (an update keeps the document's filter values)
      nd.cat = docs[d].cat;
      table.UpdateDocument(d, docs[d].text, nd.text);
      docs[d] = nd;
    }
  }
  for (DocId d = 21001; d <= 21100; ++d) {
    docs[d] = MakeDoc();
    EXPECT(table.AddDocument(d, docs[d].text, Filters(docs[d])));
  }
  Index fresh(2, 0, 0.0, false);
  for (const auto& kv : docs) fresh.AddDocument(kv.first, kv.second.text, Filters(kv.second));
  std::vector<BatchQuery> qs;
  std::vector<std::vector<DocId>> want;
  for (int i = 0; i < 48; ++i) {
    const int64_t t = static_cast<int64_t>(Next() % 100000) - 20000;
    qs.push_back(Q(kWords[i % 6], {{"stamp", FilterOp::GTE, std::to_string(t)}}));
    if (i % 2) {
      qs.back().sort_by_score = true;
      qs.back().order = SortOrder::DESC;
      qs.back().limit = 10;
    }
    want.push_back(Want(docs, kWords[i % 6], t, nullptr, nullptr));
  }
  auto rebuilt = ExecuteBatch(fresh, qs);
  EXPECT(rebuilt.has_value());
  const auto got = run(std::move(qs));
  EXPECT(table.GetMutationStats().delta_documents > 0);
  for (size_t i = 0; rebuilt && i < got.size(); ++i) {
    EXPECT(got[i].results == (*rebuilt)[i].results && got[i].scores == (*rebuilt)[i].scores && got[i].total == (*rebuilt)[i].total);
    EXPECT(got[i].total == want[i].size());
    if (i % 2 == 0) EXPECT(got[i].results == want[i]);
  }
  std::printf("%d checks, %d failed\n", g_checked, g_failed);
  return g_failed == 0 ? 0 : 1;
}
