// mutable_pages_test.cpp — queries without a page bound on a table with a delta index, through
// search_pipeline::ExecuteBatch: limit 0 (the full result vector), docid pages past 16384, deep SORT _score pages, on
// term, expression (ast) and FUZZY queries with and without verify_text; the SORT _score pages (bounded, deep, limit 0)
// once more at two BM25 parameter sets other than the defaults. The bar: a changed table returns what an Index built from
// the same current documents returns (docs, totals, scores bit for bit). Needs a GPU; built and run by
// tests/test_gpu_mutable_pages_cpp.py.
#include <cstdint>
#include <cstdio>
#include <map>
#include <memory>
#include <string>
#include <utility>
#include <vector>

#include "../../mygram-db_amd/csrc/shim/mygram_shim.hpp"

using mygramdb::index::DocId;
using mygramdb::index::Index;
using mygramdb::query::NodeType;
using mygramdb::query::QueryNode;
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

static uint64_t g_rng = 12345;
static uint32_t Next() {
  g_rng = g_rng * 6364136223846793005ull + 1442695040888963407ull;
  return static_cast<uint32_t>(g_rng >> 33);
}

static const char* const kWords[] = {"alpha", "beta", "gamma", "delta", "omega", "theta", "lambda", "sigma", "kappa"};

static std::string Doc(const char* extra = nullptr) {
  std::string s;
  const uint32_t n = 2 + Next() % 5;
  for (uint32_t i = 0; i < n; ++i) {
    if (!s.empty()) s += ' ';
    s += kWords[Next() % 9];
  }
  if (extra) s += std::string(" ") + extra;
  return s;
}

static BatchQuery Terms(std::vector<std::string> terms, bool score, SortOrder order, uint32_t limit, uint32_t offset = 0) {
  BatchQuery q;
  q.terms = std::move(terms);
  q.sort_by_score = score;
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

static std::vector<BatchQuery> Queries() {
  std::vector<BatchQuery> qs;
  for (SortOrder o : {SortOrder::ASC, SortOrder::DESC}) {
    qs.push_back(Terms({"alpha"}, false, o, 0));                    // limit 0: every match
    qs.push_back(Terms({"ta"}, false, o, 20000));                   // one n-gram, limit > 16384
    qs.push_back(Terms({"gamma", "ta"}, true, o, 0));               // SORT _score, every match
    qs.push_back(Terms({"ta"}, true, o, 50, 1500));                 // deep SORT _score, one-gram term
    qs.push_back(Terms({"delta", "ma"}, true, o, 40, 1100));        // deep, text-level + one-gram terms
    qs.push_back(Terms({"zzqx"}, false, o, 0));                     // a word only changed documents hold
    qs.push_back(Terms({"zzqx", "alpha"}, true, o, 0));
    BatchQuery n = Terms({"sigma"}, true, o, 30, 1200);
    n.not_terms = {"kappa"};
    qs.push_back(std::move(n));
    // expression queries: (alpha OR beta) AND NOT omega; NOT gamma
    BatchQuery e = Terms({}, false, o, 0);
    e.ast = Node(NodeType::AND, Node(NodeType::OR, Term("alpha"), Term("beta")), Node(NodeType::NOT, Term("omega")));
    qs.push_back(e);
    e.sort_by_score = true;
    e.limit = 60;
    e.offset = 1100;
    qs.push_back(e);
    BatchQuery e2 = Terms({}, false, o, 20000);
    e2.ast = Node(NodeType::NOT, Term("gamma"));
    qs.push_back(e2);
    // FUZZY, without and with verify_text
    for (bool verify : {false, true}) {
      BatchQuery f = Terms({"lambda", "sigmq"}, false, o, 0);
      f.fuzzy_max_distance = 1;
      f.verify_text = verify;
      qs.push_back(f);
      f.sort_by_score = true;
      f.limit = 25;
      f.offset = 1030;
      qs.push_back(f);
    }
  }
  return qs;
}

// Every SORT _score query of Queries() plus bounded pages, at (k1, b) (BatchQuery::bm25).
static std::vector<BatchQuery> ScoredAt(double k1, double b) {
  std::vector<BatchQuery> qs;
  for (BatchQuery& q : Queries())
    if (q.sort_by_score) qs.push_back(std::move(q));
  for (SortOrder o : {SortOrder::ASC, SortOrder::DESC}) {
    qs.push_back(Terms({"gamma", "ta"}, true, o, 10));
    qs.push_back(Terms({"ta", "ma"}, true, o, 100, 7));
    qs.push_back(Terms({"alpha", "ta", "ma"}, true, o, 1));
    qs.push_back(Terms({"zzqx", "ta"}, true, o, 10));
  }
  for (BatchQuery& q : qs) {
    q.bm25.k1 = k1;
    q.bm25.b = b;
  }
  return qs;
}

static bool SamePage(const BatchResult& a, const BatchResult& b) {
  return a.results == b.results && a.scores == b.scores && a.total == b.total;
}
static bool SameCounters(const BatchResult& a, const BatchResult& b) {
  return a.total == b.total && a.total_candidates == b.total_candidates && a.after_intersection == b.after_intersection &&
         a.after_not == b.after_not && a.after_filters == b.after_filters;
}

static void Compare(Index& table, const std::map<DocId, std::string>& docs, const char* round) {
  const std::vector<BatchQuery> qs = Queries();
  auto got = ExecuteBatch(table, qs);
  Index fresh(2, 0, 0.0, false);
  for (const auto& d : docs) fresh.AddDocument(d.first, d.second);
  auto want = ExecuteBatch(fresh, qs);
  EXPECT(got.has_value() && want.has_value());
  if (!got) std::printf("  %s: ExecuteBatch(changed table): %s\n", round, got.error().message().c_str());
  if (!got || !want) return;
  size_t nonempty = 0;
  for (size_t i = 0; i < qs.size(); ++i) {
    const bool same = SamePage((*got)[i], (*want)[i]);
    EXPECT(same);
    if (!same)
      std::printf("  %s: query %zu differs: total %llu/%llu, %zu/%zu docs\n", round, i,
                  static_cast<unsigned long long>((*got)[i].total), static_cast<unsigned long long>((*want)[i].total),
                  (*got)[i].results.size(), (*want)[i].results.size());
    // the four funnel counters too: the sum of the main index's and the delta's equals a fresh index's only when the
    // main index counts live documents alone and both plan the terms in the order of the table's current posting sizes
    const bool counters = SameCounters((*got)[i], (*want)[i]);
    EXPECT(counters);
    if (!counters)
      std::printf("  %s: query %zu counters differ: %llu %llu %llu %llu / %llu %llu %llu %llu\n", round, i,
                  static_cast<unsigned long long>((*got)[i].total_candidates),
                  static_cast<unsigned long long>((*got)[i].after_intersection),
                  static_cast<unsigned long long>((*got)[i].after_not),
                  static_cast<unsigned long long>((*got)[i].after_filters),
                  static_cast<unsigned long long>((*want)[i].total_candidates),
                  static_cast<unsigned long long>((*want)[i].after_intersection),
                  static_cast<unsigned long long>((*want)[i].after_not),
                  static_cast<unsigned long long>((*want)[i].after_filters));
    nonempty += (*got)[i].results.empty() ? 0 : 1;
  }
  EXPECT(nonempty + 2 >= qs.size());  // (every shape returns a page; zzqx may be absent from the delta after compaction)
  // the scored pages at parameters other than the defaults: the table's statistics (main + delta) and the merge of main
  // and delta pages carry k1 and b through
  for (const auto& kb : {std::make_pair(0.3, 1.0), std::make_pair(20.0, 0.0)}) {
    const std::vector<BatchQuery> sq = ScoredAt(kb.first, kb.second);
    auto g = ExecuteBatch(table, sq);
    auto w = ExecuteBatch(fresh, sq);
    auto d = ExecuteBatch(table, ScoredAt(1.2, 0.75));
    EXPECT(g.has_value() && w.has_value() && d.has_value());
    if (!g || !w || !d) continue;
    size_t differ = 0;
    for (size_t i = 0; i < sq.size(); ++i) {
      const bool same = SamePage((*g)[i], (*w)[i]);
      EXPECT(same);
      if (!same)
        std::printf("  %s: k1 %g b %g: query %zu differs: total %llu/%llu, %zu/%zu docs\n", round, kb.first, kb.second, i,
                    static_cast<unsigned long long>((*g)[i].total), static_cast<unsigned long long>((*w)[i].total),
                    (*g)[i].results.size(), (*w)[i].results.size());
      differ += (*g)[i].scores != (*d)[i].scores ? 1 : 0;
    }
    EXPECT(differ + 2 >= sq.size());  // (the parameters reached the device: scores other than the defaults' ones)
  }
  EXPECT((*want)[0].results.size() == (*want)[0].total && (*want)[0].total > 1000);  // limit 0: the full vector
  // a limit-0 query's funnel counters equal those of the same query with limit 10, on the same table
  std::vector<BatchQuery> pair = {Terms({"alpha"}, false, SortOrder::ASC, 0), Terms({"alpha"}, false, SortOrder::ASC, 10)};
  pair.push_back(qs[qs.size() / 2 + 8]);  // the expression query, limit 0, DESC
  pair.push_back(qs[qs.size() / 2 + 8]);
  pair.back().limit = 10;
  auto c = ExecuteBatch(table, pair);
  EXPECT(c.has_value());
  if (c) {
    EXPECT(SameCounters((*c)[0], (*c)[1]) && (*c)[0].results.size() == (*c)[0].total && (*c)[1].results.size() == 10);
    EXPECT(SameCounters((*c)[2], (*c)[3]) && (*c)[3].results.size() == 10);
  }
}

int main() {
  std::map<DocId, std::string> docs;
  Index table(2, 0, 0.0, false);
  for (DocId d = 1; d <= 12000; ++d) {
    docs[d] = Doc();
    table.AddDocument(d, docs[d]);
  }
  {
    auto first = ExecuteBatch(table, Queries());  // builds the main index; every shape runs on a static table too
    EXPECT(first.has_value());
    if (!first) std::printf("  static: %s\n", first.error().message().c_str());
  }
  // changes: updates interleave main's ids, adds lie past the build range, removed ids come back, zzqx is new
  for (int k = 0; k < 150; ++k) {
    const DocId d = 1 + Next() % 12000;
    if (!docs.count(d)) continue;
    table.RemoveDocument(d, docs[d]);
    docs.erase(d);
  }
  for (int k = 0; k < 200; ++k) {
    const DocId d = 1 + Next() % 12000;
    if (!docs.count(d)) continue;
    const std::string nt = Doc(k % 4 == 0 ? "zzqx" : nullptr);
    table.UpdateDocument(d, docs[d], nt);
    docs[d] = nt;
  }
  for (DocId d = 13001; d <= 13150; ++d) {
    docs[d] = Doc(d % 5 == 0 ? "zzqx" : nullptr);
    EXPECT(table.AddDocument(d, docs[d]));
  }
  int back = 0;
  for (DocId d = 1; d <= 12000 && back < 10; ++d)
    if (!docs.count(d)) {
      docs[d] = Doc();
      EXPECT(table.AddDocument(d, docs[d]));
      ++back;
    }
  EXPECT(table.GetMutationStats().delta_documents > 0);
  Compare(table, docs, "round 1");
  // documents of the delta change and leave
  int n = 0;
  for (auto it = docs.lower_bound(13001); it != docs.end() && n < 30; ++n) {
    if (n % 2 == 0) {
      table.RemoveDocument(it->first, it->second);
      it = docs.erase(it);
    } else {
      const std::string nt = Doc();
      table.UpdateDocument(it->first, it->second, nt);
      it->second = nt;
      ++it;
    }
  }
  Compare(table, docs, "round 2");
  std::printf("%d checks, %d failed\n", g_checked, g_failed);
  return g_failed == 0 ? 0 : 1;
}
