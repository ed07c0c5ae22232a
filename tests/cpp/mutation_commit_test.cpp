// mutation_commit_test.cpp — recorded changes of a mutable table are committed in one step: a failed application or
// compaction loses nothing and changes nothing, a failure is reported until it is cured, writers may run beside queries
// and compactions, and the delta index never becomes the index the index-less ResultSorter::SortByScore resolves to.
// Every case compares the table with a control: a second Index that received the same documents and the same changes
// with no failure injected. Needs a GPU; built and run by tests/test_gpu_mutation_commit_cpp.py.
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <map>
#include <memory>
#include <string>
#include <thread>
#include <vector>

#include "../../include/mygram_tools.h"
#include "../../mygram-db_amd/csrc/shim/mygram_shim.hpp"

using mygramdb::index::DocId;
using mygramdb::index::Index;
using mygramdb::index::LastDeviceError;
using mygramdb::query::FilterOp;
using mygramdb::query::ResultSorter;
using mygramdb::query::SortOrder;
using mygramdb::storage::FilterMap;
using mygramdb::storage::FilterValue;
using namespace mygramdb::search_pipeline;
using V = std::vector<DocId>;

static int g_failed = 0, g_checked = 0;
#define EXPECT(cond)                                                      \
  do {                                                                    \
    ++g_checked;                                                          \
    if (!(cond)) {                                                        \
      ++g_failed;                                                         \
      std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond);         \
    }                                                                     \
  } while (0)

static const char* const kWords[] = {"ab", "cd", "ef", "gh", "ij"};
static std::string Text(uint32_t seed) {  // three of the five words
  return std::string(kWords[seed % 5]) + " " + kWords[(seed / 5) % 5] + " " + kWords[(seed / 25 + seed) % 5];
}
static FilterMap Filters(uint32_t seed) {
  return FilterMap{{"stamp", FilterValue{static_cast<int64_t>(seed % 7)}}, {"cat", FilterValue{std::string("c") + char('0' + seed % 3)}}};
}

constexpr DocId kDocs = 300;
// The table of every case: 300 documents of three two-letter words, two filter columns; built by one batch.
struct Table {
  Index index{2, 0, 0.0, false};
  std::map<DocId, std::string> text;
  Table() {
    for (DocId d = 1; d <= kDocs; ++d) Add(d, d * 11 + 3);
  }
  void Add(DocId d, uint32_t seed) {
    text[d] = Text(seed);
    index.AddDocument(d, text[d], Filters(seed));
  }
  void Update(DocId d, uint32_t seed) {  // the three-argument form: the document keeps its filter values
    const std::string t = Text(seed);
    index.UpdateDocument(d, text[d], t);
    text[d] = t;
  }
  void Remove(DocId d) {
    index.RemoveDocument(d, text[d]);
    text.erase(d);
  }
};

static std::vector<BatchQuery> Queries() {
  std::vector<BatchQuery> qs(4);
  qs[0].terms = {"ab"};  // a docid page
  qs[0].order = SortOrder::ASC;
  qs[0].limit = 50;
  qs[1].terms = {"ab", "cd"};  // a SORT _score page
  qs[1].sort_by_score = true;
  qs[1].limit = 20;
  qs[2].terms = {"cd"};  // FILTER conditions on both columns: the bitmap path, then the per-document path
  qs[2].order = SortOrder::ASC;
  qs[2].filter_conditions = {{"cat", FilterOp::EQ, "c1"}, {"stamp", FilterOp::NE, "3"}};
  qs[3].terms = {"ef"};
  qs[3].order = SortOrder::ASC;
  qs[3].filter_conditions = {{"stamp", FilterOp::GTE, "2"}, {"cat", FilterOp::NE, "c0"}};
  return qs;
}

// "equals the control": the single operators, one batch (pages, totals, funnel counters, scores bit for bit) and the
// mutation statistics (`stats` false: not those — they say how the table is split into main and delta and how often it was applied).
static bool Same(const Index& table, const Index& control, const char* what, bool stats = true) {
  bool same = true;
  auto differ = [&](const char* part) {
    std::printf("  %s: %s differs from the control\n", what, part);
    same = false;
  };
  if (table.SearchAnd({"ab", "cd"}) != control.SearchAnd({"ab", "cd"}) || !LastDeviceError().empty()) differ("SearchAnd");
  if (table.SearchOr({"ab", "ef", "ij"}) != control.SearchOr({"ab", "ef", "ij"}) || !LastDeviceError().empty()) differ("SearchOr");
  for (const char* term : {"ab", "cd", "gh"})
    if (table.Count(term) != control.Count(term)) differ("Count");
  const auto got = ExecuteBatch(table, Queries());
  const auto want = ExecuteBatch(control, Queries());
  if (!got || !want) {
    differ(!got ? got.error().message().c_str() : want.error().message().c_str());
    return false;
  }
  for (size_t i = 0; i < want->size(); ++i) {
    const BatchResult &a = (*got)[i], &b = (*want)[i];
    if (a.results != b.results || a.scores != b.scores || a.total != b.total) differ("a page");
    if (a.total_candidates != b.total_candidates || a.after_intersection != b.after_intersection || a.after_not != b.after_not ||
        a.after_filters != b.after_filters)
      differ("a funnel counter");
    if (b.results.empty()) differ("(an empty page proves nothing)");
  }
  const auto s = table.GetMutationStats(), c = control.GetMutationStats();
  if (stats && (s.main_documents != c.main_documents || s.delta_documents != c.delta_documents ||
                s.removed_from_main != c.removed_from_main || s.epoch != c.epoch))
    differ("GetMutationStats");
  return same;
}

// call() under the allocation-failure hook at after = 0, 1, 2, ... until it returns ""; after every failing step
// failed_step() runs with the hook off. Returns the number of failed steps, or -1 when `cap` steps were not enough.
template <class Call, class AfterFailure>
static int Sweep(int cap, Call call, AfterFailure failed_step) {
  for (int after = 0; after < cap; ++after) {
    mgxt_fail_device_allocs(after, 1000);
    const std::string err = call();
    mgxt_fail_device_allocs(0, 0);
    if (err.empty()) return after;
    failed_step();
  }
  return -1;
}

static void FailedApplicationLosesNothing() {
  Table t, c;
  EXPECT(ExecuteBatch(t.index, Queries()).has_value() && ExecuteBatch(c.index, Queries()).has_value());
  for (Table* x : {&t, &c}) {
    x->Remove(5);
    x->Update(9, 1234);
    x->Add(kDocs + 1, 77);
  }
  EXPECT(c.index.ApplyMutations(true).empty());
  const uint64_t epoch = t.index.GetMutationStats().epoch;
  const int failed = Sweep(256, [&] { return t.index.ApplyMutations(true); },
                           [&] { EXPECT(t.index.GetMutationStats().epoch == epoch); });
  std::printf("case 1: %d failed applications\n", failed);
  EXPECT(failed >= 2);
  EXPECT(Same(t.index, c.index, "case 1"));
}

static void FailedRemovalLosesNothing() {
  Table t, c;
  EXPECT(ExecuteBatch(t.index, Queries()).has_value() && ExecuteBatch(c.index, Queries()).has_value());
  t.Remove(17);
  c.Remove(17);
  EXPECT(c.index.ApplyMutations(true).empty());
  const uint64_t epoch = t.index.GetMutationStats().epoch;
  const int failed = Sweep(256, [&] { return t.index.ApplyMutations(true); },
                           [&] { EXPECT(t.index.GetMutationStats().epoch == epoch); });
  std::printf("case 2: %d failed applications\n", failed);
  EXPECT(failed >= 0);
  EXPECT(Same(t.index, c.index, "case 2"));
}

static void FailureIsReportedUntilCured() {
  Table t, c;
  for (Table* x : {&t, &c}) {
    EXPECT(ExecuteBatch(x->index, Queries()).has_value());
    x->Update(9, 1234);
    EXPECT(ExecuteBatch(x->index, Queries()).has_value());  // (an application succeeded before: a staleness bound would count)
  }
  // one column, two types: the delta index cannot be built
  t.text[kDocs + 1] = Text(1);
  t.text[kDocs + 2] = Text(2);
  EXPECT(t.index.AddDocument(kDocs + 1, t.text[kDocs + 1], FilterMap{{"stamp", FilterValue{int64_t{4}}}}));
  EXPECT(t.index.AddDocument(kDocs + 2, t.text[kDocs + 2], FilterMap{{"stamp", FilterValue{std::string("four")}}}));
  c.text[kDocs + 1] = Text(1);
  EXPECT(c.index.AddDocument(kDocs + 1, c.text[kDocs + 1], FilterMap{{"stamp", FilterValue{int64_t{4}}}}));
  const uint64_t epoch = t.index.GetMutationStats().epoch;
  for (int i = 0; i < 3; ++i) EXPECT(!ExecuteBatch(t.index, Queries()).has_value());
  t.index.SetMutationStaleness(std::chrono::hours(1));  // the retry does not wait for the bound
  for (int i = 0; i < 3; ++i) EXPECT(!ExecuteBatch(t.index, Queries()).has_value());
  EXPECT(t.index.SearchAnd({"ab", "cd"}).empty() && !LastDeviceError().empty());
  EXPECT(t.index.GetMutationStats().epoch == epoch);
  t.Remove(kDocs + 2);  // the cure
  EXPECT(ExecuteBatch(t.index, Queries()).has_value());
  t.index.SetMutationStaleness(std::chrono::microseconds(0));
  EXPECT(Same(t.index, c.index, "case 3"));
}

static void FailedCompactChangesNothing() {
  Table t, c;
  for (Table* x : {&t, &c}) {
    EXPECT(ExecuteBatch(x->index, Queries()).has_value());
    x->Remove(5);
    for (DocId d = 20; d < 40; ++d) x->Update(d, d * 13);
    x->Add(kDocs + 3, 91);
    EXPECT(x->index.ApplyMutations(true).empty());
  }
  EXPECT(t.index.GetMutationStats().delta_documents == 21);
  const int failed = Sweep(512, [&] { return t.index.Compact(); }, [&] { EXPECT(Same(t.index, c.index, "case 4, after a failed Compact")); });
  std::printf("case 4: %d failed compactions\n", failed);
  EXPECT(failed >= 0);
  EXPECT(t.index.GetMutationStats().delta_documents == 0);
  EXPECT(c.index.Compact().empty());
  EXPECT(Same(t.index, c.index, "case 4"));
}

// The 200 calls of case 5's writer, in order.
static void WriterCalls(Table* x) {
  for (uint32_t i = 0; i < 200; ++i) {
    const DocId d = 1 + (i * 37) % kDocs;
    if (i % 10 == 9) x->Add(kDocs + 1 + i, i);
    else if (i % 5 == 3) x->index.UpdateFilters(d, Filters(i));
    else x->Update(d, 1000 + i);
  }
}

static void WritersAndCompact() {
  Table t, c;
  for (Table* x : {&t, &c}) {
    EXPECT(ExecuteBatch(x->index, Queries()).has_value());
    x->Update(1, 999);
    EXPECT(x->index.ApplyMutations(true).empty());
  }
  t.index.SetMutationStaleness(std::chrono::milliseconds(1));
  std::thread writer([&] { WriterCalls(&t); });
  for (int round = 0; round < 3; ++round) {  // (queries and compactions stay on this thread)
    EXPECT(ExecuteBatch(t.index, Queries()).has_value());
    EXPECT(t.index.Compact().empty());
  }
  writer.join();
  WriterCalls(&c);
  EXPECT(t.index.ApplyMutations(true).empty() && c.index.ApplyMutations(true).empty());
  EXPECT(Same(t.index, c.index, "case 5", /*stats=*/false));  // (the two differ in how often they were compacted)
  // once both are folded, every document is in the main index
  EXPECT(t.index.Compact().empty() && c.index.Compact().empty());
  const auto st = t.index.GetMutationStats(), sc = c.index.GetMutationStats();
  EXPECT(st.main_documents == sc.main_documents && st.delta_documents == 0 && sc.delta_documents == 0);
  // every document still answers its filter_conditions query: each (cat, stamp) pair selects the same documents
  std::vector<BatchQuery> qs;
  for (int cat = 0; cat < 3; ++cat)
    for (int stamp = 0; stamp < 7; ++stamp) {
      BatchQuery q;
      auto root = std::make_shared<mygramdb::query::QueryNode>(mygramdb::query::NodeType::OR);
      for (const char* w : kWords) root->children.push_back(std::make_unique<mygramdb::query::QueryNode>(std::string(w)));
      q.ast = std::move(root);
      q.order = SortOrder::ASC;
      q.limit = 0;
      q.filter_conditions = {{"cat", FilterOp::EQ, std::string("c") + char('0' + cat)}, {"stamp", FilterOp::EQ, std::to_string(stamp)}};
      qs.push_back(std::move(q));
    }
  const auto got = ExecuteBatch(t.index, qs), want = ExecuteBatch(c.index, qs);
  EXPECT(got.has_value() && want.has_value());
  uint64_t with_values = 0;
  for (size_t i = 0; got && want && i < qs.size(); ++i) {
    EXPECT((*got)[i].results == (*want)[i].results && (*got)[i].total == (*want)[i].total);
    with_values += (*want)[i].total;
  }
  EXPECT(with_values == st.main_documents);  // (every document of the table carries both values)
  EXPECT(Same(t.index, c.index, "case 5, compacted", /*stats=*/false));
}

static void SorterKeepsTheMainIndex() {
  Table t;  // (the Index finalised last in the process from here on)
  EXPECT(ExecuteBatch(t.index, Queries()).has_value());
  V docs;
  std::vector<double> scores;
  for (DocId d = 1; d <= 64; ++d) {
    docs.push_back(d);
    scores.push_back(static_cast<double>((d * 29) % 17));
  }
  auto check = [&](const char* state) {
    auto one = [&] {
      const V want = ResultSorter::SortByScore(t.index, docs, scores, SortOrder::DESC, 10, 3);
      EXPECT(want.size() == 10 && LastDeviceError().empty());
      const V got = ResultSorter::SortByScore(docs, scores, SortOrder::DESC, 10, 3);
      EXPECT(got == want && LastDeviceError().empty());
      if (got != want) std::printf("  case 6, %s: %s\n", state, LastDeviceError().c_str());
    };
    one();                          // the thread that applied the mutations
    std::thread(one).join();        // a thread that has used no Index
  };
  t.Update(3, 555);
  EXPECT(t.index.ApplyMutations(true).empty());
  check("a delta was built");
  t.Update(4, 556);
  EXPECT(t.index.ApplyMutations(true).empty());
  check("the delta was replaced");
  EXPECT(t.index.Compact().empty());
  check("the delta went away in Compact");
}

int main() {
  FailedApplicationLosesNothing();
  FailedRemovalLosesNothing();
  FailureIsReportedUntilCured();
  FailedCompactChangesNothing();
  WritersAndCompact();
  SorterKeepsTheMainIndex();
  std::printf("mutation_commit_test: %d checks, %d failed\n", g_checked, g_failed);
  return g_failed == 0 ? 0 : 1;
}
