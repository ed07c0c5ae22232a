// Stand-alone check of the bitmap group's page plan (mgx_pages.hpp): no HIP, no GPU. Built by
// tests/test_pages_plan_cpu.py and `make pages-host-asan` with -fsanitize=address,undefined.
//   cases       the hand-stated ones below: docid pages, a faceted query, deep SORT _score, SORT <column> (fused job or
//               full sort, job capacity and workgroups), two sides, merged_away, primary key by string, the 2^32 refusal
//   invariants  over those and over kRandomInputs seeded random inputs (up to 6 queries, 1-2 sides, totals 0..5000, limits
//               0..3000, every sort order the compiler produces): the scratch regions are 8-byte aligned, in order,
//               disjoint and inside `bytes`; every expanded range, run, job output, list and page lies inside its region and
//               none overlaps another; the page sizes sum to the pdocs region; run_start is the prefix sum of a_n + b_n;
//               pages and takes equal a model worked out independently
// Every plan that is built is also recorded (g_inputs), so that a second program can replay the same inputs.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <utility>
#include <vector>

#include "../../mygram-db_amd/csrc/mgx_pages.hpp"

namespace pg = mgx::pages;

static long g_checks = 0;
static long g_shapes = 0;
static const char* g_case = "";
#define CHECK(cond)                                                                              \
  do {                                                                                           \
    ++g_checks;                                                                                  \
    if (!(cond)) {                                                                               \
      std::fprintf(stderr, "%s:%d: CHECK(%s) failed (%s, plan %ld)\n", __FILE__, __LINE__, #cond, g_case, g_shapes); \
      std::exit(1);                                                                              \
    }                                                                                            \
  } while (0)

constexpr uint64_t kMax32 = 0xFFFFFFFFull;
constexpr int kRandomInputs = 4000;
static std::vector<pg::Input> g_inputs;

static bool Pow2(uint64_t x) { return x != 0 && (x & (x - 1)) == 0; }

struct Span {
  uint64_t begin, end;
};
static void CheckDisjoint(std::vector<Span> spans, uint64_t region) {
  std::sort(spans.begin(), spans.end(), [](const Span& a, const Span& b) { return a.begin < b.begin; });
  uint64_t at = 0;
  for (const Span& s : spans) {
    CHECK(s.begin >= at && s.end >= s.begin);
    at = s.end;
  }
  CHECK(at <= region);
}

static void CheckInvariants(const pg::Input& in, const pg::Plan& p) {
  const size_t n = in.queries.size();
  CHECK(p.queries.size() == n && p.run_start.size() == n + 1 && p.krun_start.size() == p.kruns.size() + 1);
  // ---- the scratch block: regions in order, aligned, inside bytes ----
  const pg::Scratch& o = p.at;
  const uint64_t expanded = p.expanded[0] + p.expanded[1];
  const Span regions[] = {
      {0, n * sizeof(mgx::DevMergeRun)},
      {o.run_start, o.run_start + (n + 1) * 8},
      {o.terms, o.terms + p.n_terms * 4},
      {o.idfs, o.idfs + p.n_terms * 8},
      {o.jobs, o.jobs + p.jobs.size() * sizeof(mgx::colsort::TopkJob)},
      {o.kruns, o.kruns + p.kruns.size() * sizeof(mgx::pkey::KeyMergeRun)},
      {o.krun_start, o.krun_start + p.krun_start.size() * 8},
      {o.docs, o.docs + expanded * 4},
      {o.scores, o.scores + p.n_scores * 8},
      {o.keys, o.keys + p.n_keys * 8},
      {o.dprime, o.dprime + p.n_keys * 4},
      {o.pdocs, o.pdocs + p.pages * 4},
      {o.pscores, o.pscores + p.pages * 8},
      {o.lkeys, o.lkeys + p.n_lists * 8},
      {o.ldocs, o.ldocs + p.n_lists * 4},
      {o.ln, o.ln + static_cast<uint64_t>(p.n_groups_total) * 4},
  };
  uint64_t at = 0;
  for (const Span& r : regions) {
    CHECK(r.begin % 8 == 0);
    CHECK(r.begin >= at && r.begin < at + 8);  // (back to back but for the alignment)
    at = r.end;
  }
  CHECK(o.bytes == at);
  CHECK(o.up_bytes == regions[6].end && o.docs >= o.up_bytes);
  // ---- queries: pages, expanded ranges, runs ----
  std::vector<Span> key_spans, list_spans;
  uint64_t pages = 0, elems = 0, kelems = 0, exp_at[2] = {0, p.expanded[0]}, scores = 0, terms = 0;
  size_t n_kruns = 0, n_jobs = 0, full_runs = 0;
  for (size_t i = 0; i < n; ++i) {
    const pg::Query& q = in.queries[i];
    const pg::QueryPlan& qp = p.queries[i];
    const mgx::DevMergeRun& r = qp.run;
    const bool sorted = q.deep_score || q.col_sort;
    // the model: the page and what each side takes
    uint64_t t = 0;
    for (int k = 0; k < in.n_side; ++k) t += in.merged_away ? 0 : q.side[k].total;
    uint64_t lo = 0, hi = q.limit == 0 ? t : std::min<uint64_t>(t, static_cast<uint64_t>(sorted ? q.offset : 0) + q.limit);
    if (sorted) lo = std::min<uint64_t>(q.offset, t);
    if (q.faceted) lo = hi = 0;
    CHECK(qp.total == (in.n_side == 2 ? t : q.funnel_total));
    CHECK(qp.page_off == pages && qp.page_n == hi - lo && r.out_off == pages && r.lo == lo && r.hi == hi);
    pages += qp.page_n;
    CHECK(r.kind == (sorted ? mgx::kMergeScore : q.reverse ? mgx::kMergeDocDesc : mgx::kMergeDocAsc));
    CHECK(r.descending == (q.reverse ? 1u : 0u));
    const bool by_string = q.pk_sort && q.col_sort && in.merge_by_string;
    uint64_t run_sum = 0;
    for (int k = 0; k < 2; ++k) {
      const pg::SidePlan& sp = qp.side[k];
      if (k >= in.n_side) {
        CHECK(sp.take == 0 && sp.run_n == 0 && sp.key_cap == 0);
        continue;
      }
      const uint64_t tk = q.side[k].total;
      const bool job = q.col_sort && !in.colsort_full && hi <= 1024 && hi != lo && tk != 0;
      CHECK(sp.run_n == (hi == lo ? 0 : sorted && !job ? tk : std::min(tk, hi)));
      CHECK(sp.take == (job ? 0 : sp.run_n));
      run_sum += sp.run_n;
      if (sp.take != 0) {  // its expanded ids: each side's back to back, side 1 behind side 0
        CHECK(sp.docs_off == exp_at[k]);
        exp_at[k] += sp.take;
      }
      if (sp.key_cap != 0) {
        CHECK(sorted && sp.take != 0 && Pow2(sp.key_cap) && sp.key_cap >= 2048 && sp.key_cap >= sp.take);
        CHECK(sp.key_cap == 2048 || sp.key_cap / 2 < sp.take);
        key_spans.push_back({sp.key_off, sp.key_off + sp.key_cap});
        full_runs += q.col_sort ? 1 : 0;
      } else {
        CHECK(!sorted || sp.take == 0);
      }
      if (q.deep_score && sp.take != 0) {
        CHECK(sp.score_off == scores && sp.term_off == terms);
        scores += sp.take;
        terms += q.side[k].n_terms;
      }
      if (job) {
        CHECK(n_jobs < p.jobs.size());
        const pg::Job& jb = p.jobs[n_jobs++];
        const mgx::colsort::TopkJob& j = jb.job;
        CHECK(jb.side == k && jb.column == q.side[k].sort_column);
        CHECK(j.rbits == nullptr && j.values == nullptr && j.is_null == nullptr && j.doc_map == nullptr);
        CHECK(j.needed == sp.run_n && j.needed >= 1 && j.needed <= 1024 && j.out_off == sp.key_off);
        CHECK(Pow2(j.cap) && j.cap >= 64 && j.cap >= j.needed && (j.cap == 64 || j.cap / 2 < j.needed) && j.cap <= p.max_cap);
        const uint32_t want = static_cast<uint32_t>((8192 + n - 1) / n);
        CHECK(j.n_groups == std::max(1u, std::min({want, 16u, (in.side[k].n_tiles + 1) / 2})));
        CHECK(j.n_groups * j.needed <= p.max_job_elems && j.group_begin + j.n_groups <= p.n_groups_total);
        CHECK(j.n_words == in.side[k].n_tiles * 256 && j.word_begin == static_cast<uint64_t>(i) * j.n_words);
        CHECK(j.n_docs == in.side[k].n_docs && j.first_doc_id == in.side[k].first_doc_id);
        CHECK(j.ranks == q.side[k].sort_ranks && j.bias == q.side[k].sort_bias && j.descending == r.descending);
        key_spans.push_back({j.out_off, j.out_off + j.needed});
        list_spans.push_back({j.list_off, j.list_off + static_cast<uint64_t>(j.n_groups) * j.needed});
      }
    }
    CHECK(qp.page_n <= run_sum);  // the runs cover the page
    if (by_string) {
      CHECK(r.a_n == 0 && r.b_n == 0 && n_kruns < p.kruns.size());
      const mgx::pkey::KeyMergeRun& kr = p.kruns[n_kruns];
      CHECK(p.krun_start[n_kruns] == kelems);
      CHECK(kr.a_n == qp.side[0].run_n && kr.b_n == qp.side[1].run_n && kr.lo == lo && kr.hi == hi);
      CHECK(kr.a_off == qp.side[0].key_off && kr.b_off == qp.side[1].key_off && kr.out_off == qp.page_off);
      CHECK(kr.descending == r.descending && kr.pad == 0);
      kelems += run_sum;
      ++n_kruns;
    } else {
      CHECK(r.a_n == qp.side[0].run_n && r.b_n == qp.side[1].run_n);
      if (sorted) {
        CHECK(r.a_off == qp.side[0].key_off && r.b_off == qp.side[1].key_off);
        CHECK(r.a_off + r.a_n <= p.n_keys && r.b_off + r.b_n <= p.n_keys);
      } else {
        CHECK(r.a_off == qp.side[0].docs_off && r.a_off + r.a_n <= p.expanded[0]);
        CHECK(r.b_off == qp.side[1].docs_off && r.b_off >= p.expanded[0] && r.b_off + r.b_n <= expanded);
      }
    }
    CHECK(p.run_start[i] == elems);
    elems += static_cast<uint64_t>(r.a_n) + r.b_n;
  }
  CHECK(p.run_start[n] == elems && p.elems == elems);
  CHECK(p.krun_start[n_kruns] == kelems && p.kelems == kelems && n_kruns == p.kruns.size());
  CHECK(pages == p.pages && n_jobs == p.jobs.size() && full_runs == p.full_runs);
  CHECK(exp_at[0] == p.expanded[0] && exp_at[1] == expanded && scores == p.n_scores && terms == p.n_terms);
  CheckDisjoint(key_spans, p.n_keys);
  CheckDisjoint(list_spans, p.n_lists);
  uint32_t groups = 0;
  for (const pg::Job& jb : p.jobs) {
    CHECK(jb.job.group_begin == groups);
    groups += jb.job.n_groups;
  }
  CHECK(groups == p.n_groups_total);
  CHECK(p.status == (elems + kelems == 0 ? pg::kEmpty : pg::kOk));
}

// Builds, records the input and, for a plan that is not refused, checks the invariants.
static pg::Plan Checked(const pg::Input& in) {
  ++g_shapes;
  g_inputs.push_back(in);
  pg::Plan p = pg::Build(in);
  if (p.status != pg::kTooLarge) CheckInvariants(in, p);
  return p;
}

// ---- inputs in few words ----
enum Order { kDocid, kDeep, kColumn, kPrimaryKey };
static pg::Query Q(Order order, uint32_t limit, uint64_t total0, uint64_t total1 = 0, uint32_t offset = 0) {
  pg::Query q;
  q.deep_score = order == kDeep;
  q.col_sort = order == kColumn || order == kPrimaryKey;
  q.pk_sort = order == kPrimaryKey;
  q.limit = limit;
  q.offset = offset;
  q.side[0].total = total0;
  q.side[1].total = total1;
  q.funnel_total = total0 + total1;
  for (pg::SideQuery& s : q.side) {
    s.n_terms = order == kDeep ? 2 : 0;
    s.sort_column = order == kPrimaryKey ? pg::kKeyColumn : order == kColumn ? 3 : 0;
    s.sort_ranks = order == kPrimaryKey ? 1 : 0;
  }
  return q;
}
static pg::Input In(int n_side, std::vector<pg::Query> queries, uint32_t n_tiles = 4) {
  pg::Input in;
  in.n_side = n_side;
  for (int k = 0; k < n_side; ++k) in.side[k] = pg::Side{n_tiles, n_tiles * 16384 - 5, k == 0 ? 100u : 0u};
  in.queries = std::move(queries);
  return in;
}

static void DocidPages() {
  g_case = "docid pages";
  pg::Plan p = Checked(In(1, {Q(kDocid, 0, 7), Q(kDocid, 10, 7), Q(kDocid, 3, 7), Q(kDocid, 3, 7, 0, /*offset=*/5)}));
  CHECK(p.status == pg::kOk);
  const uint64_t want_n[4] = {7, 7, 3, 3}, want_off[4] = {0, 7, 14, 17};  // (the offset is ignored)
  for (int i = 0; i < 4; ++i) {
    CHECK(p.queries[i].page_n == want_n[i] && p.queries[i].page_off == want_off[i] && p.queries[i].total == 7);
    CHECK(p.queries[i].side[0].take == want_n[i] && p.queries[i].side[0].docs_off == want_off[i]);
    CHECK(p.queries[i].run.kind == mgx::kMergeDocAsc && p.queries[i].run.lo == 0 && p.queries[i].run.a_off == want_off[i]);
  }
  CHECK(p.pages == 20 && p.expanded[0] == 20 && p.elems == 20 && p.n_keys == 0 && p.jobs.empty());
  pg::Input rev = In(1, {Q(kDocid, 3, 7)});
  rev.queries[0].reverse = 1;
  p = Checked(rev);
  CHECK(p.queries[0].run.kind == mgx::kMergeDocDesc && p.queries[0].run.descending == 1);
  // one index reports the funnel's count, whatever the totals say
  pg::Input funnel = In(1, {Q(kDocid, 3, 7)});
  funnel.queries[0].funnel_total = 9;
  CHECK(Checked(funnel).queries[0].total == 9);
}

static void FacetedQuery() {
  g_case = "faceted";
  pg::Input in = In(1, {Q(kDocid, 0, 7), Q(kDocid, 0, 5)});
  in.queries[0].faceted = true;
  const pg::Plan p = Checked(in);
  CHECK(p.queries[0].page_n == 0 && p.queries[0].side[0].take == 0 && p.queries[0].total == 7);
  CHECK(p.queries[1].page_n == 5 && p.queries[1].page_off == 0 && p.pages == 5);
  in.queries[1].faceted = true;
  CHECK(Checked(in).status == pg::kEmpty);
}

static void DeepScore() {
  g_case = "deep score";
  pg::Plan p = Checked(In(1, {Q(kDeep, 10, 7, 0, /*offset=*/7), Q(kDeep, 10, 7, 0, /*offset=*/9), Q(kDeep, 2, 7, 0, /*offset=*/3)}));
  CHECK(p.queries[0].page_n == 0 && p.queries[0].side[0].take == 0);  // offset >= total
  CHECK(p.queries[1].page_n == 0 && p.queries[1].side[0].take == 0);
  const pg::SidePlan& s = p.queries[2].side[0];
  CHECK(p.queries[2].page_n == 2 && p.queries[2].run.lo == 3 && p.queries[2].run.hi == 5 && s.take == 7 && s.run_n == 7);
  CHECK(s.key_cap == 2048 && s.key_off == 0 && s.score_off == 0 && s.term_off == 0 && p.n_terms == 2 && p.n_scores == 7);
  CHECK(p.queries[2].run.kind == mgx::kMergeScore && p.queries[2].run.a_n == 7);
  const uint64_t takes[3] = {1, 2048, 2049}, caps[3] = {2048, 2048, 4096};
  for (int c = 0; c < 3; ++c) {
    p = Checked(In(1, {Q(kDeep, 0, takes[c])}));
    CHECK(p.queries[0].side[0].take == takes[c] && p.queries[0].side[0].key_cap == caps[c] && p.n_keys == caps[c]);
    CHECK(pg::SortCapacity(takes[c]) == caps[c]);
  }
}

static void ColumnSort() {
  g_case = "column sort";
  pg::Plan p = Checked(In(1, {Q(kColumn, 1000, 3000, 0, /*offset=*/24)}));  // hi = 1024: a job, nothing expanded
  CHECK(p.jobs.size() == 1 && p.expanded[0] == 0 && p.full_runs == 0 && p.queries[0].side[0].take == 0);
  CHECK(p.queries[0].side[0].run_n == 1024 && p.jobs[0].job.needed == 1024 && p.jobs[0].job.cap == 1024 && p.jobs[0].column == 3);
  CHECK(p.queries[0].page_n == 1000 && p.n_keys == 1024);
  p = Checked(In(1, {Q(kColumn, 1001, 3000, 0, /*offset=*/24)}));  // hi = 1025: the full sort
  CHECK(p.jobs.empty() && p.full_runs == 1 && p.queries[0].side[0].take == 3000 && p.queries[0].side[0].key_cap == 4096);
  pg::Input full = In(1, {Q(kColumn, 1, 3000)});
  full.colsort_full = true;
  p = Checked(full);  // forced at hi = 1
  CHECK(p.jobs.empty() && p.full_runs == 1 && p.queries[0].side[0].take == 3000 && p.queries[0].page_n == 1);
  const uint32_t needed[4] = {1, 64, 65, 1024}, caps[4] = {64, 64, 128, 1024};
  for (int c = 0; c < 4; ++c) {
    p = Checked(In(1, {Q(kColumn, needed[c], 3000)}));
    CHECK(p.jobs.size() == 1 && p.jobs[0].job.needed == needed[c] && p.jobs[0].job.cap == caps[c] && p.max_cap == caps[c]);
  }
  // workgroups per job: 1 with one tile; want = 8192 at one query, capped by kTopkMaxGroups and by the tiles; want = 1
  // at 8192 queries
  CHECK(Checked(In(1, {Q(kColumn, 10, 3000)}, /*n_tiles=*/1)).jobs[0].job.n_groups == 1);
  CHECK(Checked(In(1, {Q(kColumn, 10, 3000)}, /*n_tiles=*/100)).jobs[0].job.n_groups == mgx::colsort::kTopkMaxGroups);
  CHECK(Checked(In(1, {Q(kColumn, 10, 3000)}, /*n_tiles=*/9)).jobs[0].job.n_groups == 5);
  p = Checked(In(1, std::vector<pg::Query>(8192, Q(kColumn, 10, 30)), /*n_tiles=*/100));
  CHECK(p.jobs.size() == 8192 && p.jobs[0].job.n_groups == 1 && p.jobs[8191].job.n_groups == 1 && p.n_groups_total == 8192);
  p = Checked(In(1, std::vector<pg::Query>(8191, Q(kColumn, 10, 30)), /*n_tiles=*/100));
  CHECK(p.jobs[0].job.n_groups == 2 && p.n_lists == 8191ull * 2 * 10 && p.max_job_elems == 20);
}

static void TwoSides() {
  g_case = "two sides";
  pg::Input in = In(2, {Q(kDocid, 4, 6, 3), Q(kDocid, 0, 0, 2), Q(kColumn, 5, 0, 9), Q(kDeep, 0, 3, 0)});
  in.queries[0].funnel_total = 1000;
  pg::Plan p = Checked(in);
  CHECK(p.queries[0].total == 9 && p.queries[1].total == 2);  // the sum, not funnel slot 4
  CHECK(p.queries[0].side[0].take == 4 && p.queries[0].side[1].take == 3 && p.queries[0].page_n == 4);
  CHECK(p.queries[1].side[0].take == 0 && p.queries[1].side[1].take == 2);
  // side 0 expands 4 + 0 + 0 + 3 ids: side 1's first id follows them
  CHECK(p.expanded[0] == 7 && p.queries[0].side[1].docs_off == 7 && p.queries[1].side[1].docs_off == 10);
  CHECK(p.queries[0].run.a_off == 0 && p.queries[0].run.b_off == 7 && p.queries[1].run.a_n == 0 && p.queries[1].run.b_off == 10);
  // a side without matches: no job, no run
  CHECK(p.jobs.size() == 1 && p.jobs[0].side == 1 && p.queries[2].side[0].run_n == 0 && p.queries[2].run.a_n == 0);
  CHECK(p.queries[3].side[1].key_cap == 0 && p.queries[3].side[1].take == 0 && p.n_keys == 5 + 2048 && p.n_terms == 2);
}

static void OtherStates() {
  g_case = "merged away";
  pg::Input away = In(1, {Q(kDocid, 0, 7), Q(kDeep, 0, 7), Q(kColumn, 5, 7)});
  away.merged_away = true;
  pg::Plan p = Checked(away);
  CHECK(p.status == pg::kEmpty && p.pages == 0 && p.jobs.empty() && p.expanded[0] == 0 && p.n_keys == 0);
  for (const pg::QueryPlan& qp : p.queries) CHECK(qp.page_n == 0 && qp.total == 7);  // (one index: the funnel's count)
  g_case = "primary key by string";
  pg::Input in = In(2, {Q(kPrimaryKey, 5, 3, 4), Q(kPrimaryKey, 2000, 3000, 10), Q(kDocid, 2, 5, 5)});
  in.merge_by_string = true;
  p = Checked(in);
  CHECK(p.kruns.size() == 2 && p.krun_start.size() == 3 && p.krun_start[0] == 0 && p.krun_start[1] == 7 && p.krun_start[2] == 3017);
  CHECK(p.kruns[0].a_n == 3 && p.kruns[0].b_n == 4 && p.kruns[0].hi == 5 && p.kruns[0].a_off == 0 && p.kruns[0].b_off == 3);
  CHECK(p.kruns[1].a_n == 3000 && p.kruns[1].b_n == 10 && p.kruns[1].out_off == 5 && p.kruns[1].b_off == 7 + 4096);
  CHECK(p.queries[0].run.a_n == 0 && p.queries[0].run.b_n == 0 && p.queries[1].run.a_n == 0 && p.queries[1].run.b_n == 0);
  CHECK(p.elems == 4 && p.kelems == 3017 && p.jobs.size() == 2 && p.jobs[0].column == pg::kKeyColumn && p.full_runs == 2);
  in.merge_by_string = false;  // numeric keys on both sides: the rank merge takes them
  p = Checked(in);
  CHECK(p.kruns.empty() && p.krun_start.size() == 1 && p.queries[0].run.a_n == 3 && p.queries[0].run.b_n == 4);
}

// The five sums the fetch refuses past 2^32 - 1. elems, pages and n_keys can pass it alone. kelems cannot: every string-
// merged run also lies in the key buffers (n_keys >= kelems). n_lists cannot below 2^22 queries: a job's lists hold
// n_groups * needed <= 16 * 1024 pairs, n_groups > 1 needs fewer than 8192 queries (at most 2^28 pairs in all), and with
// one workgroup per job n_lists is the jobs' part of n_keys.
static void Refusal() {
  g_case = "refusal: elems";
  const uint64_t b30 = 1ull << 30, b31 = 1ull << 31;
  pg::Input in = In(2, {Q(kDocid, 1u << 30, b30, b30), Q(kDocid, 1u << 30, b30, b30 - 1)});
  pg::Plan p = Checked(in);
  CHECK(p.status == pg::kOk && p.elems == kMax32);  // just below
  in.queries[1].side[1].total = b30;
  p = Checked(in);
  CHECK(p.status == pg::kTooLarge && p.elems == kMax32 + 1 && p.pages <= kMax32 && p.n_keys == 0 && p.n_lists == 0 && p.kelems == 0);
  // (one query whose two runs together pass 2^32: the sum is taken in 64 bits. Not recorded: the replay is of sums below)
  p = pg::Build(In(2, {Q(kDocid, 1u << 31, b31, b31)}));
  CHECK(p.status == pg::kTooLarge && p.elems == kMax32 + 1 && p.pages == b31);
  g_case = "refusal: pages";
  in = In(2, {Q(kDocid, 0, b31 - 1), Q(kPrimaryKey, 0, b31)});
  in.merge_by_string = true;
  p = Checked(in);
  CHECK(p.status == pg::kOk && p.pages == kMax32);
  in.queries[0].side[0].total = b31;
  p = Checked(in);
  CHECK(p.status == pg::kTooLarge && p.pages == kMax32 + 1 && p.elems == b31 && p.kelems == b31 && p.n_keys == b31 && p.n_lists == 0);
  g_case = "refusal: n_keys";
  std::vector<pg::Query> qs;
  for (int e = 31; e >= 11; --e) qs.push_back(Q(kDeep, 0, 1ull << e));
  p = Checked(In(1, qs));  // the largest sum of capacities below 2^32
  CHECK(p.status == pg::kOk && p.n_keys == kMax32 + 1 - 2048);
  qs.push_back(Q(kDeep, 0, 1));
  p = Checked(In(1, qs));
  CHECK(p.status == pg::kTooLarge && p.n_keys == kMax32 + 1 && p.elems <= kMax32 && p.pages <= kMax32);
  p = Checked(In(1, {Q(kDeep, 0, b31 + 1)}));  // one run whose capacity alone is 2^32
  CHECK(p.status == pg::kTooLarge && p.n_keys == kMax32 + 1 && p.elems == b31 + 1);
  g_case = "refusal: kelems";
  in = In(2, {Q(kPrimaryKey, 0, b30, b30), Q(kPrimaryKey, 0, b30, b30)});
  in.merge_by_string = true;
  p = Checked(in);
  CHECK(p.status == pg::kTooLarge && p.kelems == kMax32 + 1 && p.elems == 0 && p.n_keys == kMax32 + 1);
}

static pg::Input RandomInput(std::mt19937_64& rng) {
  auto pick = [&](uint64_t below) { return static_cast<uint64_t>(rng() % below); };
  pg::Input in;
  in.n_side = 1 + static_cast<int>(pick(2));
  in.merged_away = in.n_side == 1 && pick(16) == 0;
  in.colsort_full = pick(8) == 0;
  in.merge_by_string = in.n_side == 2 && pick(2) == 0;
  for (int k = 0; k < in.n_side; ++k) {
    in.side[k].n_tiles = 1 + static_cast<uint32_t>(pick(40));
    in.side[k].n_docs = in.side[k].n_tiles * 16384 - static_cast<uint32_t>(pick(16384));
    in.side[k].first_doc_id = static_cast<uint32_t>(pick(3)) * 1000;
  }
  in.queries.resize(1 + pick(6));
  for (pg::Query& q : in.queries) {
    // the orders the compiler produces: docid (SORT by primary key's shortcut included), _score, column, primary key
    const uint64_t order = pick(5);
    q.deep_score = order == 1;
    q.col_sort = order == 2 || order == 3;
    q.pk_sort = order == 3 || order == 4;
    q.reverse = static_cast<uint32_t>(pick(2));
    q.faceted = pick(8) == 0;
    q.limit = pick(4) == 0 ? 0 : static_cast<uint32_t>(pick(2) ? pick(3001) : pick(40));
    q.offset = pick(2) ? 0 : static_cast<uint32_t>(pick(2) ? pick(3001) : pick(40));
    q.funnel_total = pick(5001);
    for (int k = 0; k < in.n_side; ++k) {
      pg::SideQuery& s = q.side[k];
      s.total = pick(3) == 0 ? 0 : pick(2) ? pick(5001) : pick(30);
      s.n_terms = q.deep_score ? static_cast<uint32_t>(pick(6)) : 0;
      s.sort_column = q.pk_sort ? pg::kKeyColumn : static_cast<uint32_t>(pick(4));
      s.sort_ranks = q.pk_sort ? 1 : static_cast<uint32_t>(pick(2));
      s.sort_bias = s.sort_ranks && !q.pk_sort ? static_cast<uint32_t>(pick(2)) : 0;
    }
  }
  return in;
}

int main() {
  DocidPages();
  FacetedQuery();
  DeepScore();
  ColumnSort();
  TwoSides();
  OtherStates();
  Refusal();
  g_case = "random";
  std::mt19937_64 rng(20240229);
  for (int i = 0; i < kRandomInputs; ++i) Checked(RandomInput(rng));
  std::printf("pages plan ok: %ld plans, %ld checks\n", g_shapes, g_checks);
  return 0;
}
