// mgx_compile.hpp — the query compiler: an mgx_query becomes a tile program (QuerySpec) for the kernels of
// mgx_kernels.hip. Host code only (no HIP header), tested without a GPU (tests/test_compile_cpu.py).
#pragma once

#include <cstdint>
#include <string>
#include <vector>

#include "../../include/mygram_gpu.h"
#include "mgx_internal.hpp"

namespace mgx {

// What the compiler knows about an index (ViewOf, mgx_api.cpp): taken once per batch, so all its queries compile against
// ONE value of live_row / bitmaps_clean / n_filter_columns, not one read per query — visible only to a racing writer.
struct CompileView {
  const uint64_t* offsets = nullptr;   // [n_grams + 1] posting offsets
  const uint32_t* skip_row = nullptr;  // [n_grams] row in tile_off, or kNoRow
  const uint32_t* bm_row = nullptr;    // [n_grams] row in gram_bitmaps, or kNoRow: a list-form gram
  uint64_t n_grams = 0;
  uint32_t n_docs = 0, first_doc_id = 0;
  bool has_text = false;   // mgx_index_attach_text was called
  bool can_score = false;  // the index has tf / doc_len columns
  uint32_t n_filter_rows = 0, n_filter_columns = 0;
  uint32_t live_row = kNoRow;  // mgx_index_set_live_bitmap: the filter row of the live documents, or kNoRow
  bool bitmaps_clean = false;  // ... and the bitmap-form grams hold live documents only
  bool pk_docid_order = false;  // primary-key order is doc-id order on this index, and the shortcut is allowed
};

// One compiled query, before upload.
struct QuerySpec {
  std::vector<DevLeaf> leaves;
  std::vector<uint32_t> prog;
  std::vector<DevScoreTerm> score;
  std::vector<uint32_t> explicit_ids;  // for kLeafExplicit leaves (offsets are relative to this vector)
  std::vector<mgx_condition> conds;    // for kLeafCondBitmap leaves (a = index here until LayOutConditions gives them rows)
  uint32_t mode = kModeBitmap;
  uint32_t limit = 0, offset = 0, reverse = 0;
  uint32_t stack_depth = 0;
  double k1 = 1.2, b = 0.75, avgdl = 0.0;
  uint64_t list_postings = 0;  // sum of |L| over gram operands (algorithmic bytes = 4x)
  bool wave_ok = true;         // flat program + every scored term in its own register slot
  bool flat = true;            // LOAD/AND/OR/ANDNOT/COUNT only
  bool fast_score_ok = true;   // every scored term reads a dense gram's tf column (no text-level / absent terms)
  double est_density = 0.0;    // estimated fraction of docs that match (work per tile grows with it)
  // text-level scored terms (mgx_term.text): pattern bytes and the grams whose AND is the term's candidate set
  struct TextTerm {
    std::string pattern;
    std::vector<uint32_t> grams;
    uint32_t score_index = 0;  // position among the query's scored terms
  };
  std::vector<TextTerm> text_terms;
  std::vector<std::string> verify_patterns;  // kOpVerifyText: every positive term's text
  uint64_t total_docs = 0;       // N of ComputeIDF for the text-level terms
  // SORT _score pages the fused top-k does not hold (offset + limit > kMaxNeeded, or limit 0 = all): every match is
  // materialised, scored and fully sorted (ResultSorter::SortByScore's own shape, result_sorter.cpp:661-716)
  bool deep_score = false;
  std::vector<uint32_t> deep_grams;  // the scored terms' gram ids (kNoRow: a gram this shard lacks)
  std::vector<double> deep_idfs;
  // SORT <filter column> (MGX_SORT_COLUMN / _RANK): the bitmap group's fetch ranks the matches by the column's key
  bool col_sort = false;
  uint32_t sort_column = 0, sort_ranks = 0, sort_bias = 0;
  // MGX_SORT_PRIMARY_KEY: with col_sort, the "column" is the index's key column (mgx_index_set_primary_keys); without,
  // the query took the doc-id shortcut and is an ordinary docid page
  bool pk_sort = false;
  uint32_t pat_off = 0, pat_len = 0;  // kModeTextDf specs: the term in the batch's pattern pool
  uint32_t vt_begin = 0;              // first of the query's verify patterns in the batch-wide array
  uint32_t fz_distance = 0;           // kOpVerifyFuzzy / kOpVerifyTree: d
  bool fz_op = false;                 // the program has one of those two ops: the query runs the FZ instantiation of the general kernel
  std::vector<uint32_t> verify_prog;  // kOpVerifyTree: the tree as postfix VerifyTok tokens over the op's patterns
  uint32_t vp_begin = 0;              // its first token in the batch-wide array
  // back to the freshly constructed state, keeping the vectors' storage (a re-prepared batch object compiles its new
  // queries into the specs of the old ones)
  void Clear() {
    leaves.clear();
    prog.clear();
    score.clear();
    explicit_ids.clear();
    conds.clear();
    text_terms.clear();
    verify_patterns.clear();
    deep_score = col_sort = pk_sort = false;
    sort_column = sort_ranks = sort_bias = 0;
    deep_grams.clear();
    deep_idfs.clear();
    mode = kModeBitmap;
    limit = offset = reverse = stack_depth = 0;
    k1 = 1.2;
    b = 0.75;
    avgdl = 0.0;
    list_postings = 0;
    wave_ok = flat = fast_score_ok = true;
    est_density = 0.0;
    total_docs = 0;
    pat_off = pat_len = vt_begin = fz_distance = vp_begin = 0;
    fz_op = false;
    verify_prog.clear();
  }
};

// Appends operands and instructions to one QuerySpec: CompileQuery's steps and the stand-alone operators (mgx_and & co.)
struct Compiler {
  const CompileView* v;
  QuerySpec* q;
  uint32_t sp = 0;
  uint32_t Leaf(uint32_t kind, uint32_t a, uint32_t b);  // one more operand (no score slot, no skip row): its index
  uint32_t GramLeaf(uint32_t g);                         // the operand of gram g, shared by every use of g in the query
  void Emit(Op op, uint32_t arg = 0);
};

// search_pipeline::Execute (:812-853) as a tile program. Counter slots: 0 total_candidates, 1 after_intersection,
// 2 after_not, 3 after_filters. `out` is a fresh or Clear()ed spec.
int CompileQuery(const CompileView& v, const mgx_query& in, QuerySpec* out);

// The df query of one text-level scored term into the fresh spec `out`: the AND of its grams (live documents only).
// known_or_empty: the index's df cache has the count, or the term has no gram (df 0) — the query runs over no document.
int CompileTextDf(const CompileView& v, const std::vector<uint32_t>& grams, bool known_or_empty, uint32_t pat_off,
                  uint32_t pat_len, QuerySpec* out);

}  // namespace mgx
