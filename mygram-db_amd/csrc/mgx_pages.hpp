// mgx_pages.hpp — the page plan of the bitmap group's fetch (FetchBitmapPages, mgx_api.cpp): from every side's totals,
// what each side materialises, the sorted runs and top-k jobs, every query's page and the layout of the d_merge scratch
// block. Plain C++ over plain inputs: it compiles without a HIP header (tests/cpp/pages_plan_check.cpp pins it under the
// sanitizers); mgx_api.cpp fills the inputs, calls Build and restates nothing.
//
//   page     docid order: ranks [0, min(total, limit)) (limit 0: every match; no offset, see Compile); deep SORT _score
//            and SORT <column | primary key>: ranks [min(offset, total), min(offset + limit, total)); faceted: none
//   side     one index of the table (1), or its main index and its delta (2). Per (query, side) a docid page expands the
//            side's first min(total, hi) ids in page order; a score page scores every match; a column page either selects
//            its best min(total, hi) pairs from the result bitmap (a TopkJob: hi <= colsort::kMaxNeeded) or expands, keys
//            and sorts every match. A sorted run lives in the (key, docid') buffers, padded to SortCapacity
//   merge    rank_merge_kernel cuts every page from its two runs; the pages sorted by primary key whose sides' values
//            compare only as strings (merge_by_string) go to key_merge_kernel and leave the rank merge two empty runs
//   scratch  [runs | run_start | terms | idfs | jobs | kruns | krun_start] uploaded as one block, then device-only arrays
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "mgx_colsort.hpp"
#include "mgx_internal.hpp"
#include "mgx_pkey.hpp"

namespace mgx {
namespace pages {

constexpr uint32_t kKeyColumn = 0xFFFFFFFFu;  // SideQuery::sort_column of SORT by primary key: the index's key column

inline uint64_t Align8(uint64_t x) { return (x + 7) & ~7ull; }
// The padded length of a run the bitonic network sorts (LaunchSortPairs): a power of two, at least one LDS run.
inline uint64_t SortCapacity(uint64_t n) {
  uint64_t cap = 2048;
  while (cap < n) cap <<= 1;
  return cap;
}

// ---- inputs ----
struct SideQuery {
  uint64_t total = 0;        // the side's matches
  uint32_t n_terms = 0;      // deep SORT _score: its scored terms
  uint32_t sort_column = 0;  // SORT <column>: the side's column id, or kKeyColumn
  uint32_t sort_ranks = 0, sort_bias = 0;
};
struct Query {
  // (one order per query: deep_score and col_sort exclude each other; pk_sort without col_sort is a docid page)
  bool deep_score = false, col_sort = false, pk_sort = false, faceted = false;
  uint32_t reverse = 0, offset = 0, limit = 0;
  uint64_t funnel_total = 0;  // slot 4 of the primary's funnel counters: what one index reports
  SideQuery side[2];
};
struct Side {
  uint32_t n_tiles = 0, n_docs = 0, first_doc_id = 0;
};
struct Input {
  int n_side = 1;
  bool merged_away = false;      // the delta's batch of a merge: every page is empty
  bool colsort_full = false;     // MGX_COLSORT_FULL: no fused selection
  bool merge_by_string = false;  // two sides whose primary-key values do not compare as numbers
  Side side[2];
  std::vector<Query> queries;
};

// ---- the plan ----
struct SidePlan {
  uint64_t take = 0;       // ids the side expands (expand_kernel) ...
  uint64_t docs_off = 0;   // ... and where, among both sides' expanded ids (side 1 behind all of side 0)
  uint64_t run_n = 0;      // the length of its run
  uint64_t key_off = 0;    // sorted runs: its pairs in the (key, docid') buffers ...
  uint64_t key_cap = 0;    // ... padded to this many (0: a docid run, or a top-k job's exact run)
  uint64_t score_off = 0;  // deep SORT _score: its scores
  uint64_t term_off = 0;   // and its terms / idfs among the uploaded slots
};
struct QueryPlan {
  uint64_t total = 0, page_off = 0, page_n = 0;
  DevMergeRun run{};
  SidePlan side[2];
};
struct Job {
  colsort::TopkJob job{};  // rbits, doc_map, values, is_null, value_class: null, the caller's
  int side = 0;
  uint32_t column = 0;     // SideQuery::sort_column
};
struct Scratch {
  uint64_t run_start = 0, terms = 0, idfs = 0, jobs = 0, kruns = 0, krun_start = 0;  // (runs: at 0)
  uint64_t up_bytes = 0;  // the uploaded part ends here
  uint64_t docs = 0, scores = 0, keys = 0, dprime = 0, pdocs = 0, pscores = 0, lkeys = 0, ldocs = 0, ln = 0;
  uint64_t bytes = 0;
};
enum Status { kOk = 0, kEmpty = 1, kTooLarge = 2 };  // kEmpty: every page is empty, nothing to launch

struct Plan {
  Status status = kOk;
  std::vector<QueryPlan> queries;
  std::vector<uint64_t> run_start;  // [n + 1] prefix sums of a_n + b_n
  std::vector<Job> jobs;            // SORT <column> pages the fused selection serves, one per (query, side)
  std::vector<pkey::KeyMergeRun> kruns;
  std::vector<uint64_t> krun_start;  // [kruns + 1]
  uint64_t expanded[2] = {0, 0};     // ids each side expands
  uint64_t n_scores = 0, n_keys = 0, n_lists = 0, n_terms = 0, pages = 0, elems = 0, kelems = 0;
  uint32_t n_groups_total = 0, max_cap = 0, max_job_elems = 0;
  size_t full_runs = 0;  // SORT <column> runs keyed and sorted whole
  Scratch at;
};

inline Scratch LayOut(const Plan& p) {
  const uint64_t n = p.queries.size();
  Scratch o;
  o.run_start = Align8(n * sizeof(DevMergeRun));
  o.terms = o.run_start + (n + 1) * 8;
  o.idfs = Align8(o.terms + p.n_terms * 4);
  o.jobs = o.idfs + p.n_terms * 8;
  o.kruns = Align8(o.jobs + p.jobs.size() * sizeof(colsort::TopkJob));
  o.krun_start = o.kruns + p.kruns.size() * sizeof(pkey::KeyMergeRun);
  o.up_bytes = o.krun_start + p.krun_start.size() * 8;
  o.docs = Align8(o.up_bytes);
  o.scores = Align8(o.docs + (p.expanded[0] + p.expanded[1]) * 4);
  o.keys = o.scores + p.n_scores * 8;
  o.dprime = o.keys + p.n_keys * 8;
  o.pdocs = Align8(o.dprime + p.n_keys * 4);
  o.pscores = Align8(o.pdocs + p.pages * 4);
  o.lkeys = o.pscores + p.pages * 8;
  o.ldocs = o.lkeys + p.n_lists * 8;
  o.ln = Align8(o.ldocs + p.n_lists * 4);
  o.bytes = o.ln + static_cast<uint64_t>(p.n_groups_total) * 4;
  return o;
}

inline Plan Build(const Input& in) {
  const size_t n = in.queries.size();
  Plan p;
  p.queries.resize(n);
  p.run_start.resize(n + 1);
  for (size_t i = 0; i < n; ++i) {
    const Query& q = in.queries[i];
    QueryPlan& qp = p.queries[i];
    uint64_t t = 0;
    for (int k = 0; k < in.n_side && !in.merged_away; ++k) t += q.side[k].total;  // (merged_away: sizes the empty page only)
    const bool sorted = q.deep_score || q.col_sort;
    uint64_t lo = 0, hi = 0;
    if (q.faceted) {
      // a faceted query returns its counts, no page: nothing is expanded for it
    } else if (sorted) {
      lo = std::min<uint64_t>(q.offset, t);
      hi = q.limit == 0 ? t : std::min<uint64_t>(lo + q.limit, t);
    } else {
      hi = q.limit == 0 ? t : std::min<uint64_t>(t, q.limit);  // (docid order: no offset, see Compile)
    }
    // one index reports the funnel's count (slot 4) like the other groups; a merge, the table-wide sum
    qp.total = in.n_side == 2 ? t : q.funnel_total;
    qp.page_off = p.pages;
    qp.page_n = hi - lo;
    p.pages += hi - lo;
    DevMergeRun& r = qp.run;
    r.kind = sorted ? kMergeScore : q.reverse ? kMergeDocDesc : kMergeDocAsc;
    r.descending = q.reverse ? 1u : 0u;
    r.lo = static_cast<uint32_t>(lo);
    r.hi = static_cast<uint32_t>(hi);
    r.out_off = qp.page_off;
    // the fused selection holds offset + limit <= 1024 pairs per side; past that every match is sorted
    const bool col_topk = q.col_sort && !in.colsort_full && hi <= colsort::kMaxNeeded;
    for (int k = 0; k < in.n_side; ++k) {
      const SideQuery& sq = q.side[k];
      SidePlan& sp = qp.side[k];
      // a docid page needs each side's first hi ids in page order; a score page needs every match
      sp.take = hi == lo ? 0 : sorted ? sq.total : std::min<uint64_t>(sq.total, hi);
      sp.run_n = sp.take;
      if (col_topk && sp.take != 0) {  // nothing is expanded: the run comes from the side's result bitmap
        sp.run_n = std::min<uint64_t>(sq.total, hi);
        sp.take = 0;
        sp.key_off = p.n_keys;
        p.n_keys += sp.run_n;
        Job jb;
        jb.side = k;
        jb.column = sq.sort_column;
        colsort::TopkJob& j = jb.job;
        j.n_words = in.side[k].n_tiles * kWordsPerTile;
        j.word_begin = static_cast<uint64_t>(i) * j.n_words;
        j.out_off = sp.key_off;
        j.list_off = p.n_lists;
        j.n_docs = in.side[k].n_docs;
        j.first_doc_id = in.side[k].first_doc_id;
        j.needed = static_cast<uint32_t>(sp.run_n);
        j.cap = 64;
        while (j.cap < j.needed) j.cap <<= 1;
        // workgroups per job: about 8192 in the launch (32 per CU), so that a query with ten times the matches of the
        // others is spread over several and the launch has no long tail; a workgroup covers at least two tiles
        const uint32_t want = static_cast<uint32_t>((8192 + n - 1) / n);
        j.n_groups = std::max<uint32_t>(1, std::min<uint32_t>({want, colsort::kTopkMaxGroups, (in.side[k].n_tiles + 1) / 2}));
        j.group_begin = p.n_groups_total;
        j.ranks = sq.sort_ranks;
        j.bias = sq.sort_bias;
        j.descending = r.descending;
        p.n_groups_total += j.n_groups;
        p.n_lists += static_cast<uint64_t>(j.n_groups) * j.needed;
        p.max_cap = std::max(p.max_cap, j.cap);
        p.max_job_elems = std::max(p.max_job_elems, j.n_groups * j.needed);
        p.jobs.push_back(jb);
      }
      sp.docs_off = p.expanded[k];  // (side 1: moved behind side 0's below)
      p.expanded[k] += sp.take;
      if (sorted && sp.take != 0) {  // every match, keyed (or scored) and sorted whole
        sp.key_cap = SortCapacity(sp.take);
        sp.key_off = p.n_keys;
        p.n_keys += sp.key_cap;
        if (q.col_sort) ++p.full_runs;
      }
      if (q.deep_score && sp.take != 0) {
        sp.score_off = p.n_scores;
        p.n_scores += sp.take;
        sp.term_off = p.n_terms;
        p.n_terms += sq.n_terms;
      }
    }
    r.a_n = static_cast<uint32_t>(qp.side[0].run_n);
    r.b_n = static_cast<uint32_t>(qp.side[1].run_n);  // (one index: 0, so an element's rank is its index in its own run)
    if (q.pk_sort && q.col_sort && in.merge_by_string) {  // key_merge_kernel's query: the rank merge sees two empty runs
      p.krun_start.push_back(p.kelems);
      p.kelems += qp.side[0].run_n + qp.side[1].run_n;
      p.kruns.push_back(pkey::KeyMergeRun{qp.side[0].key_off, qp.side[1].key_off, r.out_off, r.a_n, r.b_n, r.lo, r.hi, r.descending, 0});
      r.a_n = r.b_n = 0;
    }
    p.run_start[i] = p.elems;
    p.elems += static_cast<uint64_t>(r.a_n) + r.b_n;
  }
  p.run_start[n] = p.elems;
  p.krun_start.push_back(p.kelems);
  for (QueryPlan& qp : p.queries) {
    qp.side[1].docs_off += p.expanded[0];
    const bool keyed = qp.run.kind == kMergeScore;
    qp.run.a_off = keyed ? qp.side[0].key_off : qp.side[0].docs_off;
    qp.run.b_off = keyed ? qp.side[1].key_off : qp.side[1].docs_off;
  }
  p.at = LayOut(p);
  if (p.elems + p.kelems == 0) p.status = kEmpty;
  else if (p.elems > 0xFFFFFFFFull || p.kelems > 0xFFFFFFFFull || p.pages > 0xFFFFFFFFull || p.n_keys > 0xFFFFFFFFull ||
           p.n_lists > 0xFFFFFFFFull)
    p.status = kTooLarge;
  return p;
}

}  // namespace pages
}  // namespace mgx
