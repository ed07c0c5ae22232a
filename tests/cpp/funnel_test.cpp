// funnel_test.cpp — the four funnel counters of a table that changed after its build, against expectations computed by
// the CPU oracle over the table's CURRENT documents. BatchResult sums the counters of the main index and of the delta
// index; the sum is right only when the main index counts live documents alone and both indexes plan the terms in the
// order of the table's current posting sizes. A wrong order, or a main index that counts removed documents, changes
// total_candidates and nothing else.
//
// Replays a case file written by tests/test_gpu_funnel_cpp.py (line-oriented, the text last on every line):
//   doc <id> <stamp> <text>      initial document (filter column "stamp", int64)
//   build                        one query: the main index is built
//   add <id> <stamp> <text> | update <id> <new text> | remove <id> | compact
//   checkpoint <name>            the queries up to `run` are one batch on the table as it stands
//   q <label> / term <t> / notterm <t> / ast <prefix tokens: & | ! T:term> / fuzzy <d> / cond <stamp at least>
//   expect <empty_term_detected> <total> <4 counters> <every doc id, ascending> / end
//   run
// Every query runs as a docid page of 10, with limit 0 and as SORT _score top 10. Needs a GPU.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <map>
#include <memory>
#include <sstream>
#include <string>
#include <vector>

#include "../../mygram-db_amd/csrc/shim/mygram_shim.hpp"

using mygramdb::index::DocId;
using mygramdb::index::Index;
using mygramdb::query::FilterCondition;
using mygramdb::query::FilterOp;
using mygramdb::query::NodeType;
using mygramdb::query::QueryNode;
using mygramdb::query::SortOrder;
using mygramdb::storage::FilterMap;
using mygramdb::storage::FilterValue;
using namespace mygramdb::search_pipeline;

struct Expect {
  std::string label;
  bool empty = false;
  uint64_t total = 0, counters[4] = {0, 0, 0, 0};
  std::vector<DocId> ids;
};

static std::unique_ptr<QueryNode> ParseAst(std::istringstream& in) {
  std::string tok;
  if (!(in >> tok)) return nullptr;
  if (tok.rfind("T:", 0) == 0) return std::make_unique<QueryNode>(tok.substr(2));
  auto n = std::make_unique<QueryNode>(tok == "&" ? NodeType::AND : tok == "|" ? NodeType::OR : NodeType::NOT);
  n->children.push_back(ParseAst(in));
  if (tok != "!") n->children.push_back(ParseAst(in));
  return n;
}

static int g_failed = 0, g_compared = 0;

static void Fail(const std::string& where, const Expect& e, const BatchResult& r, const char* what) {
  if (++g_failed > 1) return;  // the first differing query, with both tuples
  std::printf("FAIL %s: query '%s' (%s)\n  got  empty %d total %llu counters %zu %zu %zu %zu (%zu docs)\n"
              "  want empty %d total %llu counters %llu %llu %llu %llu (%zu docs)\n",
              where.c_str(), e.label.c_str(), what, r.empty_term_detected ? 1 : 0, static_cast<unsigned long long>(r.total),
              r.total_candidates, r.after_intersection, r.after_not, r.after_filters, r.results.size(), e.empty ? 1 : 0,
              static_cast<unsigned long long>(e.total), static_cast<unsigned long long>(e.counters[0]),
              static_cast<unsigned long long>(e.counters[1]), static_cast<unsigned long long>(e.counters[2]),
              static_cast<unsigned long long>(e.counters[3]), e.ids.size());
}

static void Run(Index& table, const std::string& name, const std::vector<BatchQuery>& base, const std::vector<Expect>& want) {
  // page shapes: docid ASC limit 10, limit 0, SORT _score top 10
  std::vector<BatchQuery> qs;
  for (const BatchQuery& b : base)
    for (int shape = 0; shape < 3; ++shape) {
      BatchQuery q = b;
      q.order = shape == 2 ? SortOrder::DESC : SortOrder::ASC;
      q.limit = shape == 1 ? 0 : 10;
      q.sort_by_score = shape == 2;
      qs.push_back(std::move(q));
    }
  auto got = ExecuteBatch(table, qs);
  if (!got) {
    ++g_failed;
    std::printf("FAIL %s: ExecuteBatch: %s\n", name.c_str(), got.error().message().c_str());
    return;
  }
  for (size_t i = 0; i < qs.size(); ++i) {
    const Expect& e = want[i / 3];
    const BatchResult& r = (*got)[i];
    const int shape = static_cast<int>(i % 3);
    ++g_compared;
    if (r.empty_term_detected != e.empty) { Fail(name, e, r, "empty_term_detected"); continue; }
    if (r.total != e.total) { Fail(name, e, r, "total"); continue; }
    if (!e.empty && (r.total_candidates != e.counters[0] || r.after_intersection != e.counters[1] ||
                     r.after_not != e.counters[2] || r.after_filters != e.counters[3])) {
      Fail(name, e, r, "counters");
      continue;
    }
    const size_t n = shape == 1 ? e.ids.size() : std::min<size_t>(10, e.ids.size());
    bool page = r.results.size() == n;
    if (page && shape != 2) page = std::equal(r.results.begin(), r.results.end(), e.ids.begin());
    if (page && shape == 2)
      for (DocId d : r.results) page = page && std::binary_search(e.ids.begin(), e.ids.end(), d);
    if (!page) Fail(name, e, r, shape == 2 ? "score page" : "docid page");
  }
}

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  std::ifstream in(argv[1]);
  if (!in) return 2;
  Index table(2, 0, 0.0, false);
  std::map<DocId, std::string> docs;
  std::vector<BatchQuery> qs;
  std::vector<Expect> want;
  std::string line, checkpoint;
  size_t n_checkpoints = 0;
  while (std::getline(in, line)) {
    std::istringstream ls(line);
    std::string op;
    ls >> op;
    auto rest = [&]() {
      std::string s;
      std::getline(ls, s);
      return s.empty() ? s : s.substr(1);
    };
    if (op == "doc" || op == "add") {
      DocId id;
      int64_t stamp;
      ls >> id >> stamp;
      docs[id] = rest();
      if (!table.AddDocument(id, docs[id], FilterMap{{"stamp", FilterValue{stamp}}})) {
        std::printf("FAIL AddDocument %u\n", id);
        return 1;
      }
    } else if (op == "update") {
      DocId id;
      ls >> id;
      const std::string nt = rest();
      table.UpdateDocument(id, docs[id], nt);
      docs[id] = nt;
    } else if (op == "remove") {
      DocId id;
      ls >> id;
      table.RemoveDocument(id, docs[id]);
      docs.erase(id);
    } else if (op == "build") {
      BatchQuery q;
      q.terms = {"alpha"};
      if (!ExecuteBatch(table, {q})) return 1;
    } else if (op == "compact") {
      const std::string err = table.Compact();
      if (!err.empty()) {
        std::printf("FAIL Compact: %s\n", err.c_str());
        return 1;
      }
    } else if (op == "checkpoint") {
      checkpoint = rest();
      qs.clear();
      want.clear();
    } else if (op == "q") {
      qs.emplace_back();
      want.emplace_back();
      want.back().label = rest();
    } else if (op == "term") {
      qs.back().terms.push_back(rest());
    } else if (op == "notterm") {
      qs.back().not_terms.push_back(rest());
    } else if (op == "ast") {
      qs.back().ast = std::shared_ptr<const QueryNode>(ParseAst(ls).release());
    } else if (op == "fuzzy") {
      ls >> qs.back().fuzzy_max_distance;
    } else if (op == "cond") {
      qs.back().filter_conditions.push_back(FilterCondition{"stamp", FilterOp::GTE, rest()});
    } else if (op == "expect") {
      Expect& e = want.back();
      int empty = 0;
      ls >> empty >> e.total >> e.counters[0] >> e.counters[1] >> e.counters[2] >> e.counters[3];
      e.empty = empty != 0;
      DocId d;
      while (ls >> d) e.ids.push_back(d);
    } else if (op == "run") {
      Run(table, checkpoint, qs, want);
      ++n_checkpoints;
    }
  }
  std::printf("%zu checkpoints, %d results compared, %d failed\n", n_checkpoints, g_compared, g_failed);
  return g_failed == 0 && n_checkpoints >= 3 ? 0 : 1;
}
