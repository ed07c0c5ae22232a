// mgx_compile.cpp — mgx_query -> tile program: search_pipeline::Execute (src/server/search_pipeline.cpp:795-869),
// ApplyNotFilter (:871-932) and ApplyFiltersWithBitmap (:1196-1237) as instruction sequences. Host code only.
#include "mgx_compile.hpp"

#include <algorithm>

#include "mgx_host.hpp"

namespace mgx {

uint32_t Compiler::Leaf(uint32_t kind, uint32_t a, uint32_t b) {
  q->leaves.push_back(DevLeaf{kind, a, b, /*score_slot*/ kNoSlot, /*row*/ kNoRow, /*lds*/ 0});
  return static_cast<uint32_t>(q->leaves.size() - 1);
}

uint32_t Compiler::GramLeaf(uint32_t g) {
  // (a query has a handful of operands: a scan beats a hash map and allocates nothing)
  for (uint32_t i = 0; i < q->leaves.size(); ++i) {
    const DevLeaf& l = q->leaves[i];
    if (g == MGX_GRAM_ABSENT ? (l.kind == kLeafRange && l.row == kNoRow && l.a == 0 && l.b == 0 && l.score_slot == kAbsentMark)
                             : ((l.kind == kLeafList || l.kind == kLeafGramBitmap) && l.a == g))
      return i;
  }
  if (g == MGX_GRAM_ABSENT) {  // known to the table, no posting in this shard: the empty slot range
    const uint32_t id = Leaf(kLeafRange, 0, 0);
    q->leaves[id].score_slot = kAbsentMark;  // (tells this operand from the expression compiler's own empty ranges)
    return id;
  }
  const bool bitmap = v->bm_row[g] != kNoRow;
  const uint32_t id = Leaf(bitmap ? kLeafGramBitmap : kLeafList, g, bitmap ? v->bm_row[g] : 0);
  q->leaves[id].row = v->skip_row[g];
  q->list_postings += v->offsets[g + 1] - v->offsets[g];
  return id;
}

void Compiler::Emit(Op op, uint32_t arg) {
  if (op == kOpCount) {
    arg = 1u << arg;  // slot -> mask; consecutive counts of the same accumulator share one instruction
    if (!q->prog.empty() && (q->prog.back() >> 24) == kOpCount) {
      q->prog.back() |= arg;
      return;
    }
  }
  q->prog.push_back(MakeInstr(op, arg));
  if (op != kOpLoad && op != kOpAnd && op != kOpOr && op != kOpAndNot && op != kOpCount) q->wave_ok = q->flat = false;
  if (op == kOpPush) {
    ++sp;
    q->stack_depth = std::max(q->stack_depth, sp);
  } else if (op == kOpPopAnd || op == kOpPopOr || op == kOpPopAndNot) {
    --sp;
  }
}

// The term-text check: a term used as text carries 1..4096 normalized bytes, and the index its documents' texts
static int NeedText(const mgx_term& t, int code, const char* message) {
  return t.text && t.text_len != 0 && t.text_len <= 4096 ? MGX_OK : Fail(code, message);
}
static int NeedAttachedText(const CompileView& v, const char* message) {
  return v.has_text ? MGX_OK : Fail(MGX_ERR_INVALID_ARGUMENT, message);
}

// the shortest posting list among the grams (an absent gram: 0); no gram: ~0
static uint64_t MinPostings(const CompileView& v, const uint32_t* grams, uint32_t n) {
  uint64_t mn = ~0ull;
  for (uint32_t i = 0; i < n; ++i)
    mn = std::min<uint64_t>(mn, grams[i] == MGX_GRAM_ABSENT ? 0 : v.offsets[grams[i] + 1] - v.offsets[grams[i]]);
  return mn;
}
static double DocFraction(const CompileView& v, uint64_t docs) {
  return static_cast<double>(docs) / static_cast<double>(std::max<uint32_t>(v.n_docs, 1));
}

// A mutable table's main index: only its live documents exist (a removed document is in no posting list of the
// reference, index.cpp:148-197). An AND of bitmap-form grams of an index that keeps its bitmaps clean holds no other.
static bool LiveByConstruction(const CompileView& v, const uint32_t* grams, uint32_t n, uint32_t threshold) {
  if (!v.bitmaps_clean || n == 0 || (threshold != 0 && threshold < n)) return false;
  for (uint32_t i = 0; i < n; ++i)
    if (grams[i] != MGX_GRAM_ABSENT && v.bm_row[grams[i]] == kNoRow) return false;
  return true;
}

static int ValidateTerm(const CompileView& v, const mgx_term& t, const char* what) {
  if (t.n_grams == 0) {  // substring term: needs its text and the docs' texts
    if (int rc = NeedText(t, MGX_ERR_INVALID_ARGUMENT, (std::string(what) + ": a term without grams needs its normalized text (1..4096 bytes)").c_str())) return rc;
    return NeedAttachedText(v, (std::string(what) + ": a term without grams (substring search) needs mgx_index_attach_text").c_str());
  }
  if (!t.gram_ids) return Fail(MGX_ERR_INVALID_ARGUMENT, std::string(what) + ": term without grams");
  if (t.n_grams > 127) return Fail(MGX_ERR_OUT_OF_RANGE, std::string(what) + ": more than 127 grams in a term");
  for (uint32_t i = 0; i < t.n_grams; ++i)
    if (t.gram_ids[i] >= v.n_grams && t.gram_ids[i] != MGX_GRAM_ABSENT)
      return Fail(MGX_ERR_OUT_OF_RANGE, std::string(what) + ": unknown gram id");
  return MGX_OK;
}

namespace {
bool IsThreshold(const mgx_term& t) { return t.threshold != 0 && t.threshold < t.n_grams; }

// One query on its way to a QuerySpec: the steps of CompileQuery, in the order it runs them.
struct QueryCompiler : Compiler {
  const mgx_query& in;
  QueryCompiler(const CompileView& view, QuerySpec* spec, const mgx_query& query) : Compiler{&view, spec, 0}, in(query) {}
  int CheckArguments() {
    if (in.n_terms == 0 || !in.terms) return Fail(MGX_ERR_INVALID_ARGUMENT, "query without positive terms");
    if (in.n_terms > MGX_MAX_TERMS || in.n_not_terms > MGX_MAX_TERMS || in.n_filters > MGX_MAX_TERMS)
      return Fail(MGX_ERR_OUT_OF_RANGE, "more than 64 terms / NOT terms / filters (query_parser.h:270-272)");
    if (static_cast<uint64_t>(in.n_filters) + in.n_conditions > MGX_MAX_TERMS)
      return Fail(MGX_ERR_OUT_OF_RANGE, "more than 64 filters and conditions together (query_parser.h:270-272)");
    if (in.n_conditions != 0 && !in.conditions) return Fail(MGX_ERR_INVALID_ARGUMENT, "n_conditions without conditions");
    for (uint32_t i = 0; i < in.n_conditions; ++i) {
      if (in.conditions[i].op > MGX_CMP_GE) return Fail(MGX_ERR_INVALID_ARGUMENT, "condition: unknown operator");
      if (in.conditions[i].column_id >= v->n_filter_columns) return Fail(MGX_ERR_OUT_OF_RANGE, "condition: unknown filter column");
    }
    for (uint32_t i = 0; i < in.n_terms; ++i)
      if (int rc = ValidateTerm(*v, in.terms[i], "term")) return rc;
    for (uint32_t i = 0; i < in.n_not_terms; ++i)
      if (int rc = ValidateTerm(*v, in.not_terms[i], "NOT term")) return rc;
    return MGX_OK;
  }
  // the estimated fraction of docs that match: every term as selective as its rarest gram, terms independent
  void EstimateDensity() {
    double dens = 1.0;
    for (uint32_t i = 0; i < in.n_terms; ++i) {
      const mgx_term& t = in.terms[i];  // (a substring term filters, it does not narrow the estimate)
      dens *= DocFraction(*v, t.n_grams ? MinPostings(*v, t.gram_ids, t.n_grams) : v->n_docs);
    }
    q->est_density = dens;
  }
  // one more verify pattern of the query (the term's text): its index among them
  uint32_t AddPattern(const mgx_term& t) {
    q->verify_patterns.emplace_back(reinterpret_cast<const char*>(t.text), t.text_len);
    return static_cast<uint32_t>(q->verify_patterns.size() - 1);
  }
  // acc = the term's doc set: AND of its grams, or "at least threshold of them"
  // (SearchTermDocuments, search_pipeline.cpp:438-446; fuzzy terms :1697-1702)
  void LoadTerm(const mgx_term& t) {
    if (t.n_grams == 0) {
      // a term shorter than one n-gram: query::SearchNormalizedSubstring (src/query/substring_search.h:24-42) — every
      // doc whose stored text contains it (SearchTermDocuments, search_pipeline.cpp:438-446)
      Emit(kOpLoad, Leaf(kLeafRange, 0, v->n_docs));
      Emit(kOpVerifyText, AddPattern(t) | (1u << 12));  // (argument: first pattern | count << 12)
    } else if (IsThreshold(t) && t.threshold != 1) {
      Emit(kOpThreshBegin);
      for (uint32_t i = 0; i < t.n_grams; ++i) Emit(kOpThreshAdd, GramLeaf(t.gram_ids[i]));
      Emit(kOpThreshEnd, t.threshold);
    } else {
      // "at least one of its n-grams" is their union (FUZZY on a short term: theta = max(1, n - d * n_eff),
      // search_pipeline.cpp:1700-1703): a flat program like the AND, which the wave kernels take
      const Op join = IsThreshold(t) ? kOpOr : kOpAnd;
      Emit(kOpLoad, GramLeaf(t.gram_ids[0]));
      for (uint32_t i = 1; i < t.n_grams; ++i) Emit(join, GramLeaf(t.gram_ids[i]));
    }
  }
  // acc &= the live documents (every funnel counter counts those only); first_term: the term acc holds, if one
  void AndLive(const mgx_term* first_term) {
    if (v->live_row == kNoRow) return;
    if (first_term && LiveByConstruction(*v, first_term->gram_ids, first_term->n_grams, first_term->threshold)) return;
    Emit(kOpAnd, Leaf(kLeafFilterBitmap, 0, v->live_row));
  }
  // the flat term list: acc = terms[0] (counter 0), then every further term ANDed into it (counter 1)
  int Positive() {
    if (in.n_expr > 0) return Expression();
    LoadTerm(in.terms[0]);
    AndLive(&in.terms[0]);
    Emit(kOpCount, 0);
    for (uint32_t i = 1; i < in.n_terms; ++i) {
      const mgx_term& t = in.terms[i];
      if (t.n_grams == 0) {  // substring term: the accumulator's docs whose text contains it (search_pipeline.cpp:817-826)
        Emit(kOpVerifyText, AddPattern(t) | (1u << 12));
      } else if (IsThreshold(t)) {
        Emit(kOpPush);
        LoadTerm(t);
        Emit(kOpPopAnd);
      } else {
        for (uint32_t g = 0; g < t.n_grams; ++g) Emit(kOpAnd, GramLeaf(t.gram_ids[g]));
      }
    }
    Emit(kOpCount, 1);
    return MGX_OK;
  }
  // ExecuteWithBooleanAst: the positive part is a boolean tree over the terms. Postfix -> tree -> accumulator code.
  struct Node {
    uint32_t op, arg;
    std::vector<int> kids;
  };
  std::vector<Node> nodes;
  uint64_t ulo = 0, uhi = 0;                   // the NOT universe: the caller's doc-id range clipped to this shard's slots
  uint32_t universe = kNoRow, empty = kNoRow;  // its operand and the empty set's: slot ranges, made on first use
  int Expression() {
    if (!in.expr) return Fail(MGX_ERR_INVALID_ARGUMENT, "n_expr without expr");
    if (in.n_expr > 512) return Fail(MGX_ERR_OUT_OF_RANGE, "expression longer than 512 tokens");
    std::vector<int> st;
    for (uint32_t k = 0; k < in.n_expr; ++k) {
      const mgx_expr_token tk = in.expr[k];
      Node n{tk.op, tk.arg, {}};
      if (tk.op == MGX_EXPR_TERM) {
        if (tk.arg >= in.n_terms) return Fail(MGX_ERR_OUT_OF_RANGE, "expression refers to a term that is not given");
      } else if (tk.op == MGX_EXPR_AND || tk.op == MGX_EXPR_OR || tk.op == MGX_EXPR_NOT) {
        const uint32_t nk = tk.op == MGX_EXPR_NOT ? 1u : tk.arg;
        if (nk == 0 || nk > st.size()) return Fail(MGX_ERR_INVALID_ARGUMENT, "malformed postfix expression");
        n.kids.assign(st.end() - nk, st.end());
        st.resize(st.size() - nk);
      } else if (tk.op != MGX_EXPR_EMPTY) {
        return Fail(MGX_ERR_INVALID_ARGUMENT, "unknown expression token");
      }
      nodes.push_back(std::move(n));
      st.push_back(static_cast<int>(nodes.size()) - 1);
    }
    if (st.size() != 1) return Fail(MGX_ERR_INVALID_ARGUMENT, "postfix expression does not reduce to one result");
    const uint64_t base = v->first_doc_id, span = v->n_docs;
    uhi = span;
    if (in.universe_count != 0) {
      const uint64_t a = in.universe_first, b2 = a + in.universe_count;
      ulo = a > base ? std::min(a - base, span) : 0;
      uhi = b2 > base ? std::min(b2 - base, span) : 0;
    }
    EmitNode(st[0]);
    if (q->stack_depth > 40) return Fail(MGX_ERR_OUT_OF_RANGE, "expression nests deeper than 40 levels");
    AndLive(nullptr);
    Emit(kOpCount, 0);
    Emit(kOpCount, 1);
    return MGX_OK;
  }
  void EmitNode(int ni) {  // acc = the node's value
    const Node& n = nodes[ni];
    switch (n.op) {
      case MGX_EXPR_TERM: LoadTerm(in.terms[n.arg]); break;
      case MGX_EXPR_EMPTY:
        if (empty == kNoRow) empty = Leaf(kLeafRange, 0, 0);
        Emit(kOpLoad, empty);
        break;
      case MGX_EXPR_AND:
      case MGX_EXPR_OR:
        EmitNode(n.kids[0]);
        for (size_t k = 1; k < n.kids.size(); ++k) {
          Emit(kOpPush);
          EmitNode(n.kids[k]);
          Emit(n.op == MGX_EXPR_AND ? kOpPopAnd : kOpPopOr);
        }
        break;
      default:  // NOT: universe & ~child
        if (universe == kNoRow) universe = Leaf(kLeafRange, static_cast<uint32_t>(ulo), static_cast<uint32_t>(uhi));
        Emit(kOpLoad, universe);
        Emit(kOpPush);
        EmitNode(n.kids[0]);
        Emit(kOpPopAndNot);
        break;
    }
  }
  // ApplyNotFilter: acc &= ~term for every NOT term (counter 2)
  void NotTerms() {
    for (uint32_t i = 0; i < in.n_not_terms; ++i) {
      const mgx_term& t = in.not_terms[i];
      if (t.n_grams == 1 && !IsThreshold(t)) {
        Emit(kOpAndNot, GramLeaf(t.gram_ids[0]));
      } else {
        Emit(kOpPush);
        LoadTerm(t);
        Emit(kOpPopAndNot);
      }
    }
    Emit(kOpCount, 2);
  }
  // ApplyFiltersWithBitmap: the registered filter rows, then the batch's own conditions (counter 3)
  int Filters() {
    for (uint32_t i = 0; i < in.n_filters; ++i) {
      if (in.filters[i].bitmap_id >= v->n_filter_rows) return Fail(MGX_ERR_OUT_OF_RANGE, "unknown filter bitmap id");
      Emit(in.filters[i].negate ? kOpAndNot : kOpAnd, Leaf(kLeafFilterBitmap, 0, in.filters[i].bitmap_id));
    }
    for (uint32_t i = 0; i < in.n_conditions; ++i) {  // a filter row in all but where it lives: the batch's own arena
      q->conds.push_back(in.conditions[i]);
      Emit(in.conditions[i].negate ? kOpAndNot : kOpAnd, Leaf(kLeafCondBitmap, static_cast<uint32_t>(q->conds.size() - 1), 0));
    }
    Emit(kOpCount, 3);
    return MGX_OK;
  }
  // The text post-filters: no flat ops (kOpVerifyText: general workgroup kernel; the other two: its FZ instantiation)
  int TextPostFilter() {
    if (in.n_expr > 0) return (in.exact_text || in.fuzzy_verify_distance != 0) ? VerifyTree() : MGX_OK;
    if (in.fuzzy_verify_distance != 0) {
      // PostFilterByFuzzyText (search_pipeline.cpp:1746-1755), before the exact-text rule of :1733-1741
      if (in.fuzzy_verify_distance > 2) return Fail(MGX_ERR_INVALID_ARGUMENT, "fuzzy_verify_distance must be 0, 1 or 2");
      if (int rc = VerifyAllTerms(kOpVerifyFuzzy, "fuzzy_verify_distance without mgx_index_attach_text",
                                  "fuzzy_verify_distance: every positive term needs its normalized text (1..4096 bytes)"))
        return rc;
      q->fz_distance = in.fuzzy_verify_distance;
      q->fz_op = true;
    }
    if (!in.exact_text) return MGX_OK;
    return VerifyAllTerms(kOpVerifyText, "exact_text without mgx_index_attach_text",
                          "exact_text: every positive term needs its normalized text (1..4096 bytes)");
  }
  // acc &= docs whose text holds every positive term; argument: first pattern | count << 12
  int VerifyAllTerms(Op op, const char* no_texts, const char* no_text) {
    if (int rc = NeedAttachedText(*v, no_texts)) return rc;
    const uint32_t first = static_cast<uint32_t>(q->verify_patterns.size());
    for (uint32_t i = 0; i < in.n_terms; ++i) {
      if (int rc = NeedText(in.terms[i], MGX_ERR_INVALID_ARGUMENT, no_text)) return rc;
      AddPattern(in.terms[i]);
    }
    Emit(op, first | (in.n_terms << 12));
    return MGX_OK;
  }
  // The text post-filter of ExecuteWithBooleanAst (search_pipeline.cpp:1505-1578): the TREE is re-evaluated over each
  // candidate's text, a TERM leaf being text.find(term), or that or ContainsFuzzyMatch(text, term, d).
  int VerifyTree() {
    if (in.exact_text && in.fuzzy_verify_distance != 0)
      return Fail(MGX_ERR_INVALID_ARGUMENT, "expression: exact_text and fuzzy_verify_distance are one filter, set one of them");
    if (in.fuzzy_verify_distance > 2) return Fail(MGX_ERR_INVALID_ARGUMENT, "fuzzy_verify_distance must be 0, 1 or 2");
    if (int rc = NeedAttachedText(*v, "expression with exact_text / fuzzy_verify_distance without mgx_index_attach_text")) return rc;
    const uint32_t first_pat = static_cast<uint32_t>(q->verify_patterns.size());
    std::vector<uint32_t> pat_of(in.n_terms, kNoRow);  // term -> its pattern: a term is matched once however often it is named
    uint32_t depth = 0;
    for (uint32_t k = 0; k < in.n_expr; ++k) {  // (arity and term indices were checked when the set program was built)
      const mgx_expr_token tk = in.expr[k];
      switch (tk.op) {
        case MGX_EXPR_TERM:
          if (int rc = NeedText(in.terms[tk.arg], MGX_ERR_INVALID_ARGUMENT,
                                "expression with a text filter: every TERM token's term needs its normalized text (1..4096 bytes)"))
            return rc;
          if (pat_of[tk.arg] == kNoRow) pat_of[tk.arg] = AddPattern(in.terms[tk.arg]) - first_pat;
          q->verify_prog.push_back((kVerifyTerm << 24) | pat_of[tk.arg]);
          ++depth;
          break;
        case MGX_EXPR_EMPTY:
          q->verify_prog.push_back(kVerifyFalse << 24);
          ++depth;
          break;
        case MGX_EXPR_NOT: q->verify_prog.push_back(kVerifyNot << 24); break;
        default:
          q->verify_prog.push_back(((tk.op == MGX_EXPR_AND ? kVerifyAnd : kVerifyOr) << 24) | tk.arg);
          depth -= tk.arg - 1;
          break;
      }
      if (depth > kMaxVerifyDepth) return Fail(MGX_ERR_OUT_OF_RANGE, "expression with a text filter: more than 64 pending operands");
    }
    static_assert(MGX_MAX_TERMS <= kMaxVerifyPatterns && kMaxVerifyTokens == 512, "patterns are bits of a u64; n_expr <= 512");
    Emit(kOpVerifyTree, first_pat | (in.n_expr << 12));  // argument: first pattern | tokens << 12
    q->fz_distance = in.fuzzy_verify_distance;
    q->fz_op = true;
    return MGX_OK;
  }
  // SORT _score. The scored terms are the caller's list (expression / FUZZY queries: search_handler.cpp:428-456 scores
  // the positive terms of the tree or query, whatever branch produced the result set), or every positive term in order.
  // They become DevScoreTerms, or on a deep page (QuerySpec::deep_score) deep_grams / deep_idfs.
  int SortByScore() {
    if (!v->can_score) return Fail(MGX_ERR_NOT_IMPLEMENTED, "index was created without tf/doc_len columns");
    const uint32_t n_scored = in.score_terms ? in.n_score_terms : in.n_terms;
    auto scored_index = [&](uint32_t k) { return in.score_terms ? in.score_terms[k] : k; };
    for (uint32_t k = 0; k < n_scored; ++k)
      if (scored_index(k) >= in.n_terms) return Fail(MGX_ERR_OUT_OF_RANGE, "score_terms refers to a term that is not given");
    const bool deep = in.limit == 0 || static_cast<uint64_t>(in.offset) + in.limit > kMaxNeeded;
    if (!deep && n_scored > kMaxScoreTerms) return Fail(MGX_ERR_NOT_IMPLEMENTED, "more than 64 scored terms");
    q->deep_score = deep;
    q->mode = deep ? kModeBitmap : kModeScore;
    q->total_docs = in.total_docs;
    if (!deep && in.score_terms) q->wave_ok = q->fast_score_ok = false;  // (a listed term need not be an AND operand of the result: the general kernel tests membership)
    for (uint32_t k = 0; k < n_scored; ++k) {
      const mgx_term& t = in.terms[scored_index(k)];
      if (t.text != nullptr) {
        if (int rc = ScoreTextTerm(t, k, deep)) return rc;
      } else if (t.n_grams != 1) {
        return Fail(MGX_ERR_INVALID_ARGUMENT, "a scored term of several n-grams needs its text (mgx_term.text) for tf and df");
      } else if (deep) {  // the term is one n-gram: tf from its tf column, idf from the caller
        q->deep_grams.push_back(t.gram_ids[0] == MGX_GRAM_ABSENT ? kNoRow : t.gram_ids[0]);
        q->deep_idfs.push_back(t.idf);
      } else {
        ScoreGram(t, k);
      }
    }
    return MGX_OK;
  }
  // Scored term k is a text-level term (N1: not one n-gram), which PrepareInto numbers. A FUZZY term is scored as the
  // exact term: tf = its occurrences in the text, df = the candidates of the AND of ALL its n-grams whose text contains
  // it — PopulateTermDocumentFrequency does not know about the threshold.
  int ScoreTextTerm(const mgx_term& t, uint32_t k, bool deep) {
    if (int rc = NeedAttachedText(*v, "text-level scored term without mgx_index_attach_text")) return rc;
    if (int rc = NeedText(t, MGX_ERR_OUT_OF_RANGE, "text-level scored term: length must be 1..4096 bytes")) return rc;
    q->text_terms.push_back({std::string(reinterpret_cast<const char*>(t.text), t.text_len),
                             std::vector<uint32_t>(t.gram_ids, t.gram_ids + t.n_grams), /*score_index*/ k});
    if (deep) {
      q->deep_grams.push_back(kDeepText);
      q->deep_idfs.push_back(0.0);
    } else {
      DevScoreTerm st{};
      st.leaf = kNoLeaf;
      q->wave_ok = q->fast_score_ok = false;  // the wave kernels score from tf columns only
      q->score.push_back(st);
    }
    return MGX_OK;
  }
  // scored term k of the fused path reads gram t's tf column through the gram's operand
  void ScoreGram(const mgx_term& t, uint32_t k) {
    const DevScoreTerm st{GramLeaf(t.gram_ids[0]), /*text_term*/ 0, t.idf};
    // the same gram scored twice (a repeated term) keeps the first slot; the block kernel handles that shape
    if (t.gram_ids[0] == MGX_GRAM_ABSENT)
      q->wave_ok = q->fast_score_ok = false;  // an empty operand: never a member, contributes nothing
    else if (q->leaves[st.leaf].score_slot == kNoSlot && k < static_cast<uint32_t>(kWaveScoreSlots))
      q->leaves[st.leaf].score_slot = k;
    else
      q->wave_ok = false;
    q->score.push_back(st);
  }
};
}  // namespace

int CompileQuery(const CompileView& v, const mgx_query& in, QuerySpec* out) {
  QueryCompiler c(v, out, in);
  if (int rc = c.CheckArguments()) return rc;
  c.EstimateDensity();
  if (int rc = c.Positive()) return rc;
  c.NotTerms();
  if (int rc = c.Filters()) return rc;
  if (int rc = c.TextPostFilter()) return rc;
  out->limit = in.limit;
  out->offset = in.offset;
  out->reverse = in.reverse;
  out->k1 = in.k1;
  out->b = in.b;
  out->avgdl = in.avg_doc_length;
  if (in.sort == MGX_SORT_SCORE) {
    if (int rc = c.SortByScore()) return rc;
  } else if (in.sort == MGX_SORT_DOCID) {  // a bounded page needs no materialised result bitmap: count pass + page pass
    out->mode = (in.limit != 0 && in.limit <= kMaxDocPage) ? kModeDocPage : kModeBitmap;
    out->offset = 0;  // (pagination offset belongs to SORT _score, search_handler.cpp:469-470)
  } else if (in.sort == MGX_SORT_COLUMN || in.sort == MGX_SORT_COLUMN_RANK) {
    // SORT <filter column>: always the bitmap group (totals and funnel counters as an unbounded docid query has them);
    // the fetch ranks the matches by the column's key (mgx_colsort.hpp)
    if (in.sort_column >= v.n_filter_columns) return Fail(MGX_ERR_OUT_OF_RANGE, "sort_column: unknown filter column");
    if (in.sort_key_bias > 1) return Fail(MGX_ERR_INVALID_ARGUMENT, "sort_key_bias must be 0 or 1");
    if (in.sort == MGX_SORT_COLUMN && in.sort_key_bias != 0)
      return Fail(MGX_ERR_INVALID_ARGUMENT, "sort_key_bias belongs to a column of string ranks (MGX_SORT_COLUMN_RANK)");
    out->mode = kModeBitmap;
    out->col_sort = true;
    out->sort_column = in.sort_column;
    out->sort_ranks = in.sort == MGX_SORT_COLUMN_RANK ? 1u : 0u;
    out->sort_bias = in.sort_key_bias;
  } else if (in.sort == MGX_SORT_PRIMARY_KEY) {
    if (in.sort_column != 0 || in.sort_key_bias != 0)
      return Fail(MGX_ERR_INVALID_ARGUMENT, "MGX_SORT_PRIMARY_KEY takes no sort_column and no sort_key_bias: both must be 0");
    out->pk_sort = true;
    if (v.pk_docid_order && in.offset == 0) {
      // the keys never decrease with the doc slot: the page is the docid page in the same direction, the cheapest path
      out->mode = (in.limit != 0 && in.limit <= kMaxDocPage) ? kModeDocPage : kModeBitmap;
    } else {
      // the key column is a column of values (numeric keys) or of dictionary ranks, both ordered as they are: KeyOf's
      // rank branch with bias 0 is the identity
      out->mode = kModeBitmap;
      out->col_sort = true;
      out->sort_ranks = 1;
    }
  } else {
    return Fail(MGX_ERR_INVALID_ARGUMENT, "unknown sort");
  }
  if (out->leaves.size() > kMaxLeaves) return Fail(MGX_ERR_NOT_IMPLEMENTED, "more than 192 distinct operands in one query");
  return MGX_OK;
}

int CompileTextDf(const CompileView& v, const std::vector<uint32_t>& grams, bool known_or_empty, uint32_t pat_off,
                  uint32_t pat_len, QuerySpec* out) {
  const uint32_t n = static_cast<uint32_t>(grams.size());
  out->mode = kModeTextDf;
  out->pat_off = pat_off;
  out->pat_len = pat_len;
  Compiler c{&v, out, 0};
  if (known_or_empty) {
    // nothing to count: a term shorter than one n-gram has df 0 (PopulateTermDocumentFrequency returns before counting,
    // search_pipeline.cpp:546-549), a term seen before has this shard's count in the index's cache — the query runs over
    // no document and the known LOCAL value takes its place on the device (gather_df_kernel), before any rank sums
    c.Emit(kOpLoad, c.Leaf(kLeafRange, 0, 0));
  } else {
    c.Emit(kOpLoad, c.GramLeaf(grams[0]));
    for (uint32_t k = 1; k < n; ++k) c.Emit(kOpAnd, c.GramLeaf(grams[k]));
    if (v.live_row != kNoRow && !LiveByConstruction(v, grams.data(), n, 0))  // (df counts live documents only)
      c.Emit(kOpAnd, c.Leaf(kLeafFilterBitmap, 0, v.live_row));
  }
  out->est_density = DocFraction(v, known_or_empty ? 0 : MinPostings(v, grams.data(), n));
  if (out->leaves.size() > kMaxLeaves) return Fail(MGX_ERR_NOT_IMPLEMENTED, "more than 192 distinct n-grams in one text-level term");
  return MGX_OK;
}

}  // namespace mgx
