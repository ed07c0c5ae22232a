// compile_test.cpp — the query compiler (mygram-db_amd/csrc/mgx_compile.cpp) on the CPU, nothing else of the library
// linked: a fixed catalogue of queries is compiled against a hand-filled CompileView under five view variants, and every
// field of every resulting QuerySpec (or the return code and message) is printed as one canonical listing on stdout.
// tests/test_compile_cpu.py compares the listing with tests/cpp/compile_test.expected, which was produced by the
// compiler as it stood inside mgx_api.cpp before it became a unit of its own. A few entries are asserted by hand here as
// well, so the listing is not its own judge. Exit status 0: the hand assertions held.
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <deque>
#include <string>
#include <vector>

#include "mgx_compile.hpp"
#include "mgx_host.hpp"

namespace mgx {
static std::string g_error;
void SetError(const std::string& msg) { g_error = msg; }
int Fail(int code, const std::string& msg) {
  g_error = msg;
  return code;
}
}  // namespace mgx

using namespace mgx;

namespace {

// ---- the synthetic index: 8 named grams (0-3 bitmap-form, 4-7 list-form, distinct posting counts) and 192 one-posting
// list-form fillers (only the operand-limit refusals name them); 40,000 docs = three tiles, first doc id 1000 ----------
constexpr uint32_t kNamed = 8, kGrams = 200;
const uint64_t kCounts[kNamed] = {20000, 15000, 12000, 9000, 700, 300, 40, 5};
std::vector<uint64_t> g_offsets;
std::vector<uint32_t> g_skip, g_bm;

CompileView BaseView() {
  if (g_offsets.empty()) {
    g_offsets.push_back(0);
    for (uint32_t g = 0; g < kGrams; ++g) {
      g_offsets.push_back(g_offsets.back() + (g < kNamed ? kCounts[g] : 1));
      g_bm.push_back(g < 4 ? g : kNoRow);
      g_skip.push_back(g < 6 ? g : kNoRow);  // (the rarest lists have no skip row)
    }
  }
  CompileView v;
  v.offsets = g_offsets.data();
  v.skip_row = g_skip.data();
  v.bm_row = g_bm.data();
  v.n_grams = kGrams;
  v.n_docs = 40000;
  v.first_doc_id = 1000;
  v.has_text = true;
  v.can_score = true;
  v.n_filter_rows = 4;
  v.n_filter_columns = 2;
  return v;
}

// ---- query builder --------------------------------------------------------------------------------------------------
struct Q {
  std::deque<std::vector<uint32_t>> grams;  // (a deque: the terms keep pointers into it)
  std::vector<mgx_term> terms, nots;
  std::vector<mgx_filter> filters;
  std::vector<mgx_condition> conds;
  std::vector<mgx_expr_token> expr;
  std::vector<uint32_t> score_terms;
  mgx_query q{};
  Q() {
    q.sort = MGX_SORT_DOCID;
    q.limit = 20;
    q.k1 = 1.5;
    q.b = 0.5;
    q.avg_doc_length = 37.25;
    q.total_docs = 123456;
  }
  mgx_term Term(std::vector<uint32_t> g, uint32_t threshold, const char* text) {
    grams.push_back(std::move(g));
    mgx_term t{};
    t.gram_ids = grams.back().empty() ? nullptr : grams.back().data();
    t.n_grams = static_cast<uint32_t>(grams.back().size());
    t.threshold = threshold;
    t.idf = 1.0 + 0.25 * static_cast<double>(terms.size() + nots.size());
    t.text = reinterpret_cast<const uint8_t*>(text);
    t.text_len = text ? static_cast<uint32_t>(std::strlen(text)) : 0;
    return t;
  }
  Q& T(std::vector<uint32_t> g, uint32_t threshold = 0, const char* text = nullptr) {
    terms.push_back(Term(std::move(g), threshold, text));
    return *this;
  }
  Q& N(std::vector<uint32_t> g, uint32_t threshold = 0, const char* text = nullptr) {
    nots.push_back(Term(std::move(g), threshold, text));
    return *this;
  }
  Q& F(uint32_t row, uint32_t negate = 0) {
    filters.push_back(mgx_filter{row, negate});
    return *this;
  }
  Q& C(uint32_t column, uint32_t op, uint64_t literal, uint32_t negate = 0) {
    mgx_condition c{};
    c.column_id = column;
    c.op = op;
    c.literal_bits = literal;
    c.eq_epsilon = 0.125;
    c.null_matches = negate;
    c.negate = negate;
    conds.push_back(c);
    return *this;
  }
  Q& E(uint32_t op, uint32_t arg = 0) {
    expr.push_back(mgx_expr_token{op, arg});
    return *this;
  }
  Q& Score(uint32_t limit = 10, uint32_t offset = 0) {
    q.sort = MGX_SORT_SCORE;
    q.limit = limit;
    q.offset = offset;
    return *this;
  }
  Q& Docid(uint32_t limit, uint32_t reverse = 0) {
    q.sort = MGX_SORT_DOCID;
    q.limit = limit;
    q.reverse = reverse;
    return *this;
  }
  Q& ScoreTerms(std::vector<uint32_t> s) {
    score_terms = std::move(s);
    return *this;
  }
  template <class Fn>
  Q& Set(Fn&& fn) {
    fn(q);
    return *this;
  }
  const mgx_query& Done() {
    if (!terms.empty()) {
      q.terms = terms.data();
      q.n_terms = static_cast<uint32_t>(terms.size());
    }
    if (!nots.empty()) {
      q.not_terms = nots.data();
      q.n_not_terms = static_cast<uint32_t>(nots.size());
    }
    if (!filters.empty()) {
      q.filters = filters.data();
      q.n_filters = static_cast<uint32_t>(filters.size());
    }
    if (!conds.empty()) {
      q.conditions = conds.data();
      q.n_conditions = static_cast<uint32_t>(conds.size());
    }
    if (!expr.empty()) {
      q.expr = expr.data();
      q.n_expr = static_cast<uint32_t>(expr.size());
    }
    if (!score_terms.empty()) {
      q.score_terms = score_terms.data();
      q.n_score_terms = static_cast<uint32_t>(score_terms.size());
    }
    return q;
  }
};

// ---- the listing ----------------------------------------------------------------------------------------------------
const char* const kOpNames[] = {"LOAD", "AND", "OR", "ANDNOT", "PUSH", "POPAND", "POPOR", "POPANDNOT", "COUNT",
                                "THRBEGIN", "THRADD", "THREND", "VTEXT", "VFUZZY", "VTREE"};
const char* const kLeafNames[] = {"list", "gram", "filter", "range", "explicit", "cond"};
static_assert(kOpLoad == 0 && kOpPush == 4 && kOpCount == 8 && kOpThreshEnd == 11 && kOpVerifyTree == 14, "kOpNames follows Op");
static_assert(kLeafList == 0 && kLeafRange == 3 && kLeafCondBitmap == 5, "kLeafNames follows LeafKind");

void PrintSpec(const QuerySpec& s) {
  printf("mode=%u limit=%u offset=%u reverse=%u stack_depth=%u k1=%.17g b=%.17g avgdl=%.17g total_docs=%" PRIu64 "\n", s.mode,
         s.limit, s.offset, s.reverse, s.stack_depth, s.k1, s.b, s.avgdl, s.total_docs);
  printf("list_postings=%" PRIu64 " wave_ok=%d flat=%d fast_score_ok=%d est_density=%.17g deep_score=%d\n", s.list_postings,
         s.wave_ok, s.flat, s.fast_score_ok, s.est_density, s.deep_score);
  printf("pat_off=%u pat_len=%u vt_begin=%u vp_begin=%u fz_distance=%u fz_op=%d\n", s.pat_off, s.pat_len, s.vt_begin,
         s.vp_begin, s.fz_distance, s.fz_op);
  printf("leaves:");
  for (const DevLeaf& l : s.leaves)
    printf(" %s(a=%u b=%u slot=%u row=%d lds=%u)", kLeafNames[l.kind], l.a, l.b, l.score_slot, static_cast<int>(l.row), l.lds);
  printf("\nprog:");
  for (uint32_t w : s.prog) printf(" %s:%x", kOpNames[w >> 24], w & 0xFFFFFFu);
  printf("\nscore:");
  for (const DevScoreTerm& t : s.score) printf(" (leaf=%d text_term=%u idf=%.17g)", static_cast<int>(t.leaf), t.text_term, t.idf);
  printf("\nexplicit_ids:");
  for (uint32_t id : s.explicit_ids) printf(" %u", id);
  printf("\nconds:");
  for (const mgx_condition& c : s.conds)
    printf(" (col=%u op=%u lit=%" PRIu64 " eps=%.17g null=%u never=%u negate=%u reserved=%u)", c.column_id, c.op, c.literal_bits,
           c.eq_epsilon, c.null_matches, c.never_matches, c.negate, c.reserved);
  printf("\ntext_terms:");
  for (const QuerySpec::TextTerm& t : s.text_terms) {
    printf(" (\"%s\" score_index=%u grams=", t.pattern.c_str(), t.score_index);
    for (uint32_t g : t.grams) printf("%d,", static_cast<int>(g));
    printf(")");
  }
  printf("\nverify_patterns:");
  for (const std::string& p : s.verify_patterns) printf(" \"%s\"", p.c_str());
  printf("\nverify_prog:");
  for (uint32_t w : s.verify_prog) printf(" %u:%u", w >> 24, w & 0xFFFFFFu);
  printf("\ndeep:");
  for (size_t i = 0; i < s.deep_grams.size(); ++i) printf(" (gram=%x idf=%.17g)", s.deep_grams[i], s.deep_idfs[i]);
  printf("\n");
}

int g_failures = 0;
void Expect(bool ok, const char* view, const char* name, const char* what) {
  if (ok) return;
  ++g_failures;
  fprintf(stderr, "FAILED %s/%s: %s\n", view, name, what);
}

struct Run {
  const char* view_name;
  CompileView view;
  QuerySpec last;
  int rc = 0;
  // compiles, lists, and keeps the spec for the hand assertions
  void operator()(const char* name, Q& q) {
    last = QuerySpec();
    g_error.clear();
    rc = CompileQuery(view, q.Done(), &last);
    printf("== %s/%s\n", view_name, name);
    if (rc) printf("rc=%d error=%s\n", rc, g_error.c_str());
    else PrintSpec(last);
  }
  void operator()(const char* name, Q&& q) { (*this)(name, q); }
  // a refusal: code and message asserted here as well
  void Refuse(const char* name, Q& q, int code, const char* message) {
    (*this)(name, q);
    Expect(rc == code && g_error == message, view_name, name, "return code / message");
  }
  void Refuse(const char* name, Q&& q, int code, const char* message) { Refuse(name, q, code, message); }
  void Df(const char* name, const std::vector<uint32_t>& grams, bool known_or_empty) {
    last = QuerySpec();
    g_error.clear();
    rc = CompileTextDf(view, grams, known_or_empty, 48, 7, &last);
    printf("== %s/%s\n", view_name, name);
    if (rc) printf("rc=%d error=%s\n", rc, g_error.c_str());
    else PrintSpec(last);
  }
};

std::vector<uint32_t> Fillers(uint32_t first, uint32_t n) {
  std::vector<uint32_t> g;
  for (uint32_t i = 0; i < n; ++i) g.push_back(kNamed + first + i);
  return g;
}

void Pages(Run& run, const char* name, Q (*make)()) {
  const std::string n(name);
  run((n + "/docid-page").c_str(), make().Docid(20));
  run((n + "/docid-page-reverse").c_str(), make().Docid(16384, 1));
  run((n + "/docid-unbounded").c_str(), make().Docid(0));
  run((n + "/docid-over-page").c_str(), make().Docid(16385));
  run((n + "/score-top10").c_str(), make().Score(10));
  run((n + "/score-1024").c_str(), make().Score(1000, 24));
  run((n + "/score-deep-1025").c_str(), make().Score(1000, 25));
  run((n + "/score-unbounded").c_str(), make().Score(0, 3));
}

void Catalogue(Run& run) {
  // flat AND of 1, 3 and 5 one-gram terms under every page shape
  Pages(run, "and1", [] { return std::move(Q().T({1})); });
  Pages(run, "and3", [] { return std::move(Q().T({0}).T({1}).T({2})); });
  Pages(run, "and3-list-first", [] { return std::move(Q().T({5}).T({1}).T({2})); });
  Pages(run, "and5", [] { return std::move(Q().T({6}).T({4}).T({3}).T({1}).T({0})); });
  // scored-term shapes
  run("score/repeated-gram", Q().T({2}).T({1}).T({2}).Score());
  run("score/repeated-gram-deep", Q().T({2}).T({1}).T({2}).Score(0));
  run("score/absent", Q().T({1}).T({MGX_GRAM_ABSENT}).Score());
  run("score/absent-twice", Q().T({MGX_GRAM_ABSENT}).T({1}).T({MGX_GRAM_ABSENT}).Score());
  run("score/absent-deep", Q().T({1}).T({MGX_GRAM_ABSENT}).Score(2000));
  run("docid/absent", Q().T({1}).T({MGX_GRAM_ABSENT, 2}));
  run("score/score-terms", Q().T({0}).T({1}).T({2}).ScoreTerms({2, 0, 2}).Score());
  run("score/score-terms-deep", Q().T({0}).T({1}).T({2}).ScoreTerms({2, 0, 2}).Score(0));
  run("score/fourth-term", Q().T({0}).T({1}).T({2}).T({3}).Score());
  run("score/six-terms", Q().T({0}).T({1}).T({2}).T({3}).T({4}).T({5}).Score());
  // threshold terms
  run("threshold/union", Q().T({4, 5, 6}, 1));
  run("threshold/union-score-text", Q().T({4, 5, 6}, 1, "abcd").Score());
  run("threshold/middle", Q().T({0, 1, 2, 4}, 2));
  run("threshold/all", Q().T({0, 1, 2}, 3));
  run("threshold/second", Q().T({1}).T({0, 2, 4}, 2).T({3}));
  run("threshold/union-second", Q().T({1}).T({4, 5}, 1));
  run("term/several-grams", Q().T({0, 1}).T({1, 2, 4}));
  // substring terms (no gram)
  run("substring/first", Q().T({}, 0, "a").T({1}));
  run("substring/second", Q().T({1}).T({}, 0, "b").T({2}));
  run("substring/only-scored", Q().T({}, 0, "a").Score());
  // NOT terms
  run("not/one-gram", Q().T({0}).N({4}));
  run("not/several-grams", Q().T({0}).N({1, 4}).N({5}));
  run("not/threshold", Q().T({0}).N({1, 2, 4}, 2).N({2}, 1));
  run("not/substring", Q().T({0}).N({}, 0, "zz"));
  run("not/score", Q().T({0}).T({1}).N({2}).Score());
  // filters and conditions
  run("filter/plain", Q().T({0}).F(2));
  run("filter/negated", Q().T({0}).F(1, 1).F(1));
  run("condition/plain", Q().T({0}).C(1, MGX_CMP_LT, 77));
  run("condition/negated", Q().T({0}).C(0, MGX_CMP_GE, 5, 1).C(0, MGX_CMP_GE, 5));
  run("filter+condition/score", Q().T({0}).T({1}).F(3).C(1, MGX_CMP_EQ, 9).N({4}).Score());
  // text-level scored terms, exact_text, FUZZY verify
  run("text-term/fused", Q().T({0, 1}, 0, "abc").T({2}).Score());
  run("text-term/deep", Q().T({0, 1}, 0, "abc").T({2}).Score(0));
  run("text-term/one-gram-with-text", Q().T({1}, 0, "ab").Score());
  run("text-term/twice", Q().T({0, 1}, 0, "abc").T({0, 1}, 0, "abc").Score(1100));
  run("exact-text", Q().T({0, 1}, 0, "abc").T({2}, 0, "cd").Set([](mgx_query& q) { q.exact_text = 1; }));
  run("exact-text/score", Q().T({0, 1}, 0, "abc").Set([](mgx_query& q) { q.exact_text = 1; }).Score());
  run("fuzzy-verify/1", Q().T({0, 1, 4}, 1, "abcd").Set([](mgx_query& q) { q.fuzzy_verify_distance = 1; }));
  run("fuzzy-verify/2", Q().T({0, 1, 4}, 2, "abcd").T({2}, 0, "ef").Set([](mgx_query& q) { q.fuzzy_verify_distance = 2; }).Score());
  run("fuzzy-verify+exact", Q().T({0, 1}, 0, "abc").Set([](mgx_query& q) { q.fuzzy_verify_distance = 1, q.exact_text = 1; }));
  run("substring+exact", Q().T({1}, 0, "bc").T({}, 0, "b").Set([](mgx_query& q) { q.exact_text = 1; }));
  // expressions
  run("expr/and-or", Q().T({0}).T({1}).T({4}).E(0, 0).E(0, 1).E(MGX_EXPR_OR, 2).E(0, 2).E(MGX_EXPR_AND, 2));
  run("expr/not-empty", Q().T({0}).T({1}).E(0, 0).E(MGX_EXPR_EMPTY).E(MGX_EXPR_OR, 2).E(0, 1).E(MGX_EXPR_NOT).E(MGX_EXPR_AND, 2)
                            .E(MGX_EXPR_EMPTY).E(MGX_EXPR_NOT).E(MGX_EXPR_OR, 2));
  run("expr/lone-not-universe", Q().T({4}).E(0, 0).E(MGX_EXPR_NOT).Set([](mgx_query& q) { q.universe_first = 1500, q.universe_count = 2000; }));
  run("expr/universe-below", Q().T({4}).E(0, 0).E(MGX_EXPR_NOT).Set([](mgx_query& q) { q.universe_first = 10, q.universe_count = 500; }));
  run("expr/universe-past-end", Q().T({4}).E(0, 0).E(MGX_EXPR_NOT).Set([](mgx_query& q) { q.universe_first = 900, q.universe_count = 1ull << 33; }));
  run("expr/single-term", Q().T({0, 1}).E(0, 0));
  run("expr/three-way-and", Q().T({0}).T({1}).T({2}).E(0, 0).E(0, 1).E(0, 2).E(MGX_EXPR_AND, 3).N({4}).F(0).Score().ScoreTerms({0, 1, 2}));
  run("expr/threshold-substring-leaves", Q().T({0, 1, 4}, 2).T({}, 0, "x").E(0, 0).E(0, 1).E(MGX_EXPR_OR, 2));
  run("expr/tree-exact-term-twice", Q().T({0}, 0, "ab").T({1}, 0, "cd").E(0, 0).E(0, 1).E(MGX_EXPR_AND, 2).E(0, 0).E(MGX_EXPR_NOT)
                                        .E(MGX_EXPR_OR, 2).Set([](mgx_query& q) { q.exact_text = 1; }));
  run("expr/tree-fuzzy", Q().T({0}, 0, "ab").T({MGX_GRAM_ABSENT}, 0, "zz").E(0, 0).E(0, 1).E(MGX_EXPR_EMPTY).E(MGX_EXPR_OR, 3)
                             .Set([](mgx_query& q) { q.fuzzy_verify_distance = 2; }).Score().ScoreTerms({0, 1}));
  run("expr/tree-exact-after-substring", Q().T({}, 0, "q").T({1}, 0, "cd").E(0, 0).E(0, 1).E(MGX_EXPR_AND, 2)
                                             .Set([](mgx_query& q) { q.exact_text = 1; }));
  // df queries of text-level terms
  run.Df("df/grams", {0, 1, 2}, false);
  run.Df("df/list-gram", {1, 5}, false);
  run.Df("df/absent-gram", {1, MGX_GRAM_ABSENT}, false);
  run.Df("df/no-gram", {}, true);
  run.Df("df/known", {0, 5}, true);
}

void Refusals(Run& run) {
  const int kArg = MGX_ERR_INVALID_ARGUMENT, kRange = MGX_ERR_OUT_OF_RANGE, kNotImpl = MGX_ERR_NOT_IMPLEMENTED;
  run.Refuse("refuse/no-terms", Q(), kArg, "query without positive terms");
  run.Refuse("refuse/too-many-not-terms", Q().T({0}).Set([](mgx_query& q) { q.n_not_terms = 65; }), kRange,
             "more than 64 terms / NOT terms / filters (query_parser.h:270-272)");
  run.Refuse("refuse/filters+conditions", Q().T({0}).Set([](mgx_query& q) { q.n_filters = 40, q.n_conditions = 30; }), kRange,
             "more than 64 filters and conditions together (query_parser.h:270-272)");
  run.Refuse("refuse/conditions-null", Q().T({0}).Set([](mgx_query& q) { q.n_conditions = 1; }), kArg, "n_conditions without conditions");
  run.Refuse("refuse/condition-operator", Q().T({0}).C(0, MGX_CMP_GE + 1, 1), kArg, "condition: unknown operator");
  run.Refuse("refuse/condition-column", Q().T({0}).C(2, MGX_CMP_EQ, 1), kRange, "condition: unknown filter column");
  run.Refuse("refuse/substring-no-text", Q().T({}), kArg, "term: a term without grams needs its normalized text (1..4096 bytes)");
  run.Refuse("refuse/substring-long-text", Q().T({0}).N({}, 0, std::string(4097, 'a').c_str()), kArg,
             "NOT term: a term without grams needs its normalized text (1..4096 bytes)");
  run.Refuse("refuse/null-grams", Q().T({0}).Set([](mgx_query& q) { static mgx_term t{}; t.n_grams = 1; q.not_terms = &t, q.n_not_terms = 1; }),
             kArg, "NOT term: term without grams");
  run.Refuse("refuse/128-grams", Q().T(Fillers(0, 128)), kRange, "term: more than 127 grams in a term");
  run.Refuse("refuse/unknown-gram", Q().T({0, kGrams}), kRange, "term: unknown gram id");
  run.Refuse("refuse/expr-null", Q().T({0}).Set([](mgx_query& q) { q.n_expr = 1; }), kArg, "n_expr without expr");
  {
    Q q;
    q.T({0});
    for (int i = 0; i < 513; ++i) q.E(0, 0);
    run.Refuse("refuse/expr-513", std::move(q), kRange, "expression longer than 512 tokens");
  }
  run.Refuse("refuse/expr-term-index", Q().T({0}).E(0, 1), kRange, "expression refers to a term that is not given");
  run.Refuse("refuse/expr-arity", Q().T({0}).E(0, 0).E(MGX_EXPR_AND, 2), kArg, "malformed postfix expression");
  run.Refuse("refuse/expr-arity-0", Q().T({0}).E(0, 0).E(MGX_EXPR_OR, 0), kArg, "malformed postfix expression");
  run.Refuse("refuse/expr-token", Q().T({0}).E(5, 0), kArg, "unknown expression token");
  run.Refuse("refuse/expr-two-results", Q().T({0}).E(0, 0).E(0, 0), kArg, "postfix expression does not reduce to one result");
  {
    Q q;  // AND(t, AND(t, ... )) 42 levels deep: every level holds one pushed accumulator
    q.T({0});
    for (int i = 0; i < 43; ++i) q.E(0, 0);
    for (int i = 0; i < 42; ++i) q.E(MGX_EXPR_AND, 2);
    run.Refuse("refuse/expr-depth-41", std::move(q), kRange, "expression nests deeper than 40 levels");
  }
  run.Refuse("refuse/filter-id", Q().T({0}).F(3).F(4), kRange, "unknown filter bitmap id");
  run.Refuse("refuse/tree-both-filters", Q().T({0}, 0, "ab").E(0, 0).Set([](mgx_query& q) { q.exact_text = 1, q.fuzzy_verify_distance = 1; }),
             kArg, "expression: exact_text and fuzzy_verify_distance are one filter, set one of them");
  run.Refuse("refuse/tree-distance-3", Q().T({0}, 0, "ab").E(0, 0).Set([](mgx_query& q) { q.fuzzy_verify_distance = 3; }), kArg,
             "fuzzy_verify_distance must be 0, 1 or 2");
  run.Refuse("refuse/tree-term-text", Q().T({0}, 0, "ab").T({1}).E(0, 0).E(0, 1).E(MGX_EXPR_OR, 2).Set([](mgx_query& q) { q.exact_text = 1; }),
             kArg, "expression with a text filter: every TERM token's term needs its normalized text (1..4096 bytes)");
  {
    Q q;  // 65 operands pending before the one AND
    q.T({0}, 0, "ab");
    for (int i = 0; i < 65; ++i) q.E(0, 0);
    q.E(MGX_EXPR_AND, 65).Set([](mgx_query& m) { m.exact_text = 1; });
    run.Refuse("refuse/tree-65-pending", std::move(q), kRange, "expression with a text filter: more than 64 pending operands");
  }
  run.Refuse("refuse/fuzzy-distance-3", Q().T({0}, 0, "ab").Set([](mgx_query& q) { q.fuzzy_verify_distance = 3; }), kArg,
             "fuzzy_verify_distance must be 0, 1 or 2");
  run.Refuse("refuse/fuzzy-term-text", Q().T({0}, 0, "ab").T({1}).Set([](mgx_query& q) { q.fuzzy_verify_distance = 1; }), kArg,
             "fuzzy_verify_distance: every positive term needs its normalized text (1..4096 bytes)");
  run.Refuse("refuse/exact-term-text", Q().T({0}, 0, "ab").T({1}, 0, "").Set([](mgx_query& q) { q.exact_text = 1; }), kArg,
             "exact_text: every positive term needs its normalized text (1..4096 bytes)");
  run.Refuse("refuse/score-terms-index", Q().T({0}).ScoreTerms({0, 1}).Score(), kRange, "score_terms refers to a term that is not given");
  run.Refuse("refuse/deep-text-empty", Q().T({0}, 0, "").Score(0), kRange, "text-level scored term: length must be 1..4096 bytes");
  run.Refuse("refuse/fused-text-long", Q().T({0}, 0, std::string(4097, 'b').c_str()).Score(), kRange,
             "text-level scored term: length must be 1..4096 bytes");
  run.Refuse("refuse/deep-several-grams", Q().T({0, 1}).Score(0), kArg,
             "a scored term of several n-grams needs its text (mgx_term.text) for tf and df");
  run.Refuse("refuse/fused-several-grams", Q().T({0}).T({0, 1}).Score(), kArg,
             "a scored term of several n-grams needs its text (mgx_term.text) for tf and df");
  run.Refuse("refuse/deep-193-operands", Q().T({0}).T(Fillers(0, 96)).T(Fillers(96, 96)).ScoreTerms({0}).Score(0), kNotImpl,
             "more than 192 distinct operands in one query");
  run.Refuse("refuse/fused-193-operands", Q().T({0}).T(Fillers(0, 96)).T(Fillers(96, 96)).ScoreTerms({0}).Score(), kNotImpl,
             "more than 192 distinct operands in one query");
  run.Refuse("refuse/docid-193-operands", Q().T({0}).T(Fillers(0, 96)).T(Fillers(96, 96)), kNotImpl,
             "more than 192 distinct operands in one query");
  run("limit/192-operands", Q().T(Fillers(0, 96)).T(Fillers(96, 96)));
  {
    Q q;
    q.T({0});
    q.ScoreTerms(std::vector<uint32_t>(65, 0)).Score();
    run.Refuse("refuse/65-scored-terms", std::move(q), kNotImpl, "more than 64 scored terms");
  }
  run.Refuse("refuse/sort", Q().T({0}).Set([](mgx_query& q) { q.sort = 7; }), kArg, "unknown sort");
  std::vector<uint32_t> many = Fillers(0, 192);
  many.push_back(0);
  run.Df("refuse/df-193-grams", many, false);
  Expect(run.rc == kNotImpl && g_error == "more than 192 distinct n-grams in one text-level term", run.view_name, "refuse/df-193-grams",
         "return code / message");
}

// the refusals that depend on the view
void ViewRefusals(Run& notext, Run& noscore) {
  const int kArg = MGX_ERR_INVALID_ARGUMENT;
  notext.Refuse("refuse/substring-no-attach", Q().T({}, 0, "a"), kArg,
                "term: a term without grams (substring search) needs mgx_index_attach_text");
  notext.Refuse("refuse/tree-no-attach", Q().T({0}, 0, "ab").E(0, 0).Set([](mgx_query& q) { q.exact_text = 1; }), kArg,
                "expression with exact_text / fuzzy_verify_distance without mgx_index_attach_text");
  notext.Refuse("refuse/fuzzy-no-attach", Q().T({0}, 0, "ab").Set([](mgx_query& q) { q.fuzzy_verify_distance = 1; }), kArg,
                "fuzzy_verify_distance without mgx_index_attach_text");
  notext.Refuse("refuse/exact-no-attach", Q().T({0}, 0, "ab").Set([](mgx_query& q) { q.exact_text = 1; }), kArg,
                "exact_text without mgx_index_attach_text");
  notext.Refuse("refuse/deep-text-no-attach", Q().T({0}, 0, "ab").Score(0), kArg, "text-level scored term without mgx_index_attach_text");
  notext.Refuse("refuse/fused-text-no-attach", Q().T({0}, 0, "ab").Score(), kArg, "text-level scored term without mgx_index_attach_text");
  noscore.Refuse("refuse/cannot-score", Q().T({0}).Score(), MGX_ERR_NOT_IMPLEMENTED, "index was created without tf/doc_len columns");
}

// LOAD g0, COUNT mask 0x1, AND g1, AND g2, COUNT mask 0xE, written out by hand
bool IsPlainAnd3(const QuerySpec& s, bool live_after_load, uint32_t first_kind) {
  std::vector<uint32_t> want = {MakeInstr(kOpLoad, 0)};
  if (live_after_load) want.push_back(MakeInstr(kOpAnd, 1));
  const uint32_t g1 = live_after_load ? 2 : 1;
  want.insert(want.end(), {MakeInstr(kOpCount, 0x1), MakeInstr(kOpAnd, g1), MakeInstr(kOpAnd, g1 + 1), MakeInstr(kOpCount, 0xE)});
  if (s.prog != want || !s.wave_ok || !s.flat || s.leaves.size() != (live_after_load ? 4u : 3u)) return false;
  if (live_after_load && (s.leaves[1].kind != kLeafFilterBitmap || s.leaves[1].b != 3)) return false;
  return s.leaves[0].kind == first_kind && s.leaves[g1].kind == kLeafGramBitmap && s.leaves[g1].a == 1 &&
         s.leaves[g1 + 1].kind == kLeafGramBitmap && s.leaves[g1 + 1].a == 2;
}

}  // namespace

int main() {
  Run base{"base", BaseView(), {}, 0}, notext = base, live = base, clean = base, noscore = base;
  notext.view_name = "no-text";
  notext.view.has_text = false;
  live.view_name = "live";
  live.view.live_row = 3;
  clean.view_name = "live-clean";
  clean.view.live_row = 3;
  clean.view.bitmaps_clean = true;
  noscore.view_name = "no-score";
  noscore.view.can_score = false;
  for (Run* r : {&base, &notext, &live, &clean, &noscore}) Catalogue(*r);
  Refusals(base);
  ViewRefusals(notext, noscore);

  printf("== by hand\n");
  base("hand/and3", Q().T({0}).T({1}).T({2}));
  Expect(base.rc == 0 && IsPlainAnd3(base.last, false, kLeafGramBitmap) && base.last.leaves[0].a == 0, "base", "hand/and3",
         "LOAD g0, COUNT 0x1, AND g1, AND g2, COUNT 0xE; wave_ok, flat");
  const std::vector<uint32_t> plain = base.last.prog;
  clean("hand/and3", Q().T({0}).T({1}).T({2}));
  Expect(clean.rc == 0 && clean.last.prog == plain && clean.last.leaves.size() == 3, "live-clean", "hand/and3",
         "clean bitmaps: the program of the index without a live row");
  clean("hand/and3-list-first", Q().T({5}).T({1}).T({2}));
  Expect(clean.rc == 0 && IsPlainAnd3(clean.last, true, kLeafList) && clean.last.leaves[0].a == 5, "live-clean", "hand/and3-list-first",
         "one AND filter(live_row) directly after the LOAD");
  live("hand/and3", Q().T({0}).T({1}).T({2}));
  Expect(live.rc == 0 && IsPlainAnd3(live.last, true, kLeafGramBitmap), "live", "hand/and3",
         "bitmaps not clean: AND filter(live_row) after the LOAD");
  if (g_failures) fprintf(stderr, "%d hand assertions failed\n", g_failures);
  return g_failures ? 1 : 0;
}
