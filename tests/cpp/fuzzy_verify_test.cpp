// fuzzy_verify_test.cpp — FUZZY with verify_text through the C++17 shim (ExecuteBatch, BatchExecutor, a table with a
// delta index): the edit-distance post-filter PostFilterByFuzzyText (src/server/search_pipeline.cpp:1746-1755) runs on
// the device. Needs a GPU; built and run by tests/test_gpu_fuzzy_verify_shim.py.
#include <cstdio>
#include <string>
#include <utility>
#include <vector>

#include "../../mygram-db_amd/csrc/shim/mygram_shim.hpp"

using mygramdb::index::DocId;
using mygramdb::index::Index;
using mygramdb::query::SortOrder;
using namespace mygramdb::search_pipeline;

static int g_failed = 0, g_checked = 0;
#define EXPECT(cond)                                                      \
  do {                                                                    \
    ++g_checked;                                                          \
    if (!(cond)) {                                                        \
      ++g_failed;                                                         \
      std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond);         \
    }                                                                     \
  } while (0)
using V = std::vector<DocId>;

static BatchQuery Fuzzy(std::vector<std::string> terms, uint32_t d, bool score = false) {
  BatchQuery q;
  q.terms = std::move(terms);
  q.fuzzy_max_distance = d;
  q.verify_text = true;
  q.sort_by_score = score;
  q.order = score ? SortOrder::DESC : SortOrder::ASC;
  q.limit = 100;
  return q;
}

static bool Same(const BatchResult& a, const BatchResult& b) {
  return a.results == b.results && a.scores == b.scores && a.total == b.total &&
         a.total_candidates == b.total_candidates && a.after_intersection == b.after_intersection &&
         a.after_not == b.after_not && a.after_filters == b.after_filters;
}

int main() {
  {  // tests/server/search_pipeline_test.cpp:916-951 (fixture), :2034-2052 FuzzySearchPath with verify_text = "all"
    Index index(2, 0, 0.0, false);
    index.AddDocument(1, "machine learning basics");
    index.AddDocument(2, "deep learning techniques");
    index.AddDocument(3, "old article about cats");
    std::vector<BatchQuery> qs = {Fuzzy({"learnig"}, 1), Fuzzy({"learnig"}, 1, true)};
    auto r = ExecuteBatch(index, qs);
    EXPECT(r.has_value());
    if (r) {
      EXPECT((*r)[0].results == (V{1, 2}) && (*r)[0].total == 2 && (*r)[0].after_filters == 2);
      EXPECT((*r)[1].total == 2 && (*r)[1].results.size() == 2 && (*r)[1].scores.size() == 2);
    } else {
      std::printf("ExecuteBatch(fuzzy, verify_text) error: %s\n", r.error().message().c_str());
    }
    // the same through BatchExecutor, two batches in flight
    BatchExecutor ex(index);
    auto t1 = ex.Submit(qs);
    auto t2 = ex.Submit(std::vector<BatchQuery>{Fuzzy({"learnig", "machin"}, 1)});
    EXPECT(t1.has_value() && t2.has_value());
    if (t1 && t2) {
      auto w1 = ex.Wait(*t1);
      auto w2 = ex.Wait(*t2);
      EXPECT(w1.has_value() && w2.has_value());
      if (w1 && r) EXPECT(Same((*w1)[0], (*r)[0]) && Same((*w1)[1], (*r)[1]));
      if (w2) EXPECT((*w2)[0].results == (V{1}));
    }
  }
  {  // a table with a delta index: the result equals the one over an index rebuilt from the current documents
    const std::vector<std::pair<DocId, std::string>> base = {
        {1, "machine learning basics"}, {2, "deep learning techniques"}, {3, "old article about cats"},
        {4, "the databases are big"}};
    const std::vector<std::pair<DocId, std::string>> added = {
        {5, "a dataset of learnin notes"}, {6, "date of birth"}, {9, "yearning lean earnings"}, {12, "tall tales"}};
    Index table(2, 0, 0.0, false);
    for (const auto& d : base) table.AddDocument(d.first, d.second);
    std::vector<BatchQuery> qs = {Fuzzy({"learnig"}, 1), Fuzzy({"data"}, 1), Fuzzy({"lerning"}, 2),
                                  Fuzzy({"data"}, 1, true), Fuzzy({"learnig"}, 2, true), Fuzzy({"dta", "lrning"}, 2)};
    qs[1].not_terms = {"big"};
    auto before = ExecuteBatch(table, qs);  // (builds the main index)
    EXPECT(before.has_value());
    for (const auto& d : added) EXPECT(table.AddDocument(d.first, d.second));
    table.RemoveDocument(2, "deep learning techniques");
    EXPECT(table.GetMutationStats().delta_documents == added.size());
    auto got = ExecuteBatch(table, qs);
    Index fresh(2, 0, 0.0, false);
    for (const auto& d : base)
      if (d.first != 2) fresh.AddDocument(d.first, d.second);
    for (const auto& d : added) fresh.AddDocument(d.first, d.second);
    auto want = ExecuteBatch(fresh, qs);
    EXPECT(got.has_value() && want.has_value());
    if (got && want) {
      for (size_t i = 0; i < qs.size(); ++i) {
        EXPECT(Same((*got)[i], (*want)[i]));
        if (!Same((*got)[i], (*want)[i])) std::printf("  query %zu differs after the delta\n", i);
      }
      EXPECT((*want)[0].results == (V{1, 5}));     // "learning", and "learnin" one edit away
      EXPECT((*want)[1].results == (V{5, 6}));     // a substring of "dataset"; "date"; doc 4 is NOT'd
      EXPECT((*want)[1].after_filters > 2);        // ("tall tales" holds "ta": a candidate the filter drops)
      EXPECT((*want)[3].total == 3);               // 4, 5, 6
    }
  }
  std::printf("%d checks, %d failed\n", g_checked, g_failed);
  return g_failed == 0 ? 0 : 1;
}
