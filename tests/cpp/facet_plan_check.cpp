// Stand-alone check of the FACET-in-a-batch planner (mgx_facet.hpp): no HIP, no GPU. Built by tests/test_facet_plan_cpu.py
// with -fsanitize=address,undefined. For every shape of (queries 1..300) x (columns 1..8) x (n_values of {0, 1, 2,
// kLdsBins - 1, kLdsBins, kLdsBins + 1, 100000}: the same for every column, or mixed) x (n_tiles of {1, 3, 611}):
//   - the count runs are disjoint, 8-byte aligned and sum to the reported arena size;
//   - every column's LDS range lies inside the budget and no two ranges of a query overlap; a column without bins is one
//     that did not fit behind the columns before it;
//   - the items of each query cover every word of its row exactly once, in whole tiles;
//   - the plan is refused exactly when the counts exceed the arena's cap, at the request that passes it.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../mygram-db_amd/csrc/mgx_facet.hpp"

namespace fc = mgx::facet;

static long g_checks = 0;
#define CHECK(cond)                                                                  \
  do {                                                                               \
    ++g_checks;                                                                      \
    if (!(cond)) {                                                                   \
      std::fprintf(stderr, "%s:%d: CHECK(%s) failed (%s)\n", __FILE__, __LINE__, #cond, g_shape); \
      std::exit(1);                                                                  \
    }                                                                                \
  } while (0)
static char g_shape[160];

// columns: also check the count runs and the LDS ranges (they do not depend on n_tiles: once per request list is enough)
static void CheckShape(const std::vector<fc::Request>& reqs, uint32_t n_tiles, uint32_t ballot_max, bool columns = true) {
  // what the planner must decide, worked out independently
  uint64_t values = 0;
  size_t refuse_at = reqs.size();
  for (size_t r = 0; r < reqs.size() && refuse_at == reqs.size(); ++r)
    for (uint32_t nv : reqs[r].n_values) {
      values += nv;
      if (values * 8 > fc::kArenaCap) {
        refuse_at = r;
        break;
      }
    }
  fc::Plan plan;
  size_t bad = ~static_cast<size_t>(0);
  const fc::Status st = fc::Build(reqs, n_tiles, ballot_max, &plan, &bad);
  if (refuse_at != reqs.size()) {
    CHECK(st == fc::kArenaTooLarge);
    CHECK(bad == refuse_at);
    return;
  }
  CHECK(st == fc::kOk);
  CHECK(plan.queries.size() == reqs.size());
  // count runs: back to back from 0 in (query, request) order, hence disjoint; u64 elements, hence 8-byte aligned
  uint64_t at = 0;
  size_t col = 0;
  for (size_t r = 0; r < reqs.size() && columns; ++r) {
    const fc::QueryPlan& q = plan.queries[r];
    CHECK(q.query == reqs[r].query && q.row == reqs[r].row);
    CHECK(q.col_begin == col && q.n_cols == reqs[r].column_ids.size());
    std::vector<std::pair<uint32_t, uint32_t>> ranges;
    uint32_t running = 0;
    for (size_t c = 0; c < q.n_cols; ++c, ++col) {
      const fc::ColumnPlan& p = plan.columns[col];
      CHECK(p.query == reqs[r].query && p.column_id == reqs[r].column_ids[c] && p.n_values == reqs[r].n_values[c]);
      CHECK(p.count_off == at);
      CHECK((p.count_off * 8) % 8 == 0 && p.count_off * 8 + static_cast<uint64_t>(p.n_values) * 8 <= plan.arena_bytes);
      at += p.n_values;
      CHECK(p.ballot == ((p.n_values != 0 && p.n_values <= ballot_max) ? 1u : 0u));
      const bool fits = p.n_values != 0 && static_cast<uint64_t>(running) + p.n_values <= fc::kLdsBins;
      if (fits) {
        CHECK(p.lds_begin == running);  // request order, the running sum within the budget
        CHECK(static_cast<uint64_t>(p.lds_begin) + p.n_values <= fc::kLdsBins);
        ranges.emplace_back(p.lds_begin, p.lds_begin + p.n_values);
        running += p.n_values;
      } else {
        CHECK(p.lds_begin == fc::kNoBins);
      }
    }
    CHECK(q.lds_bins == running && q.lds_bins <= fc::kLdsBins);
    std::sort(ranges.begin(), ranges.end());
    for (size_t i = 1; i < ranges.size(); ++i) CHECK(ranges[i - 1].second <= ranges[i].first);
  }
  CHECK(!columns || col == plan.columns.size());
  CHECK((!columns || at * 8 == plan.arena_bytes) && plan.arena_bytes <= fc::kArenaCap);
  // items: grouped by query in order; each query's ranges are whole tiles, contiguous from word 0 to the row's end
  size_t it = 0;
  for (size_t fq = 0; fq < plan.queries.size(); ++fq) {
    uint64_t word = 0;
    while (it < plan.items.size() && plan.items[it].fq == fq) {
      const fc::Item& x = plan.items[it++];
      CHECK(x.word_begin == word);
      CHECK(x.n_words >= fc::kWordsPerTile && x.n_words % fc::kWordsPerTile == 0);
      word += x.n_words;
    }
    CHECK(word == static_cast<uint64_t>(n_tiles) * fc::kWordsPerTile);
  }
  CHECK(it == plan.items.size());
  // about kTargetGroups workgroups: never more than one per tile and query, never more than the target plus one per query
  CHECK(plan.items.size() <= static_cast<uint64_t>(n_tiles) * plan.queries.size());
  CHECK(plan.items.size() <= fc::kTargetGroups + plan.queries.size());
  if (static_cast<uint64_t>(n_tiles) * plan.queries.size() <= fc::kTargetGroups)
    CHECK(plan.items.size() == static_cast<uint64_t>(n_tiles) * plan.queries.size());  // one tile per item until then
}

int main() {
  const uint32_t kValues[7] = {0, 1, 2, fc::kLdsBins - 1, fc::kLdsBins, fc::kLdsBins + 1, 100000};
  const uint32_t kTiles[3] = {1, 3, 611};
  long shapes = 0, refused = 0;
  for (uint32_t n_queries = 1; n_queries <= 300; ++n_queries)
    for (uint32_t n_cols = 1; n_cols <= 8; ++n_cols)
      for (int variant = 0; variant < 8; ++variant) {  // 0..6: every column kValues[variant]; 7: mixed
        std::vector<fc::Request> reqs(n_queries);
        uint64_t values = 0;
        for (uint32_t r = 0; r < n_queries; ++r) {
          reqs[r].query = 2 * r + 1;  // (batch positions with gaps: unfaceted queries in between)
          reqs[r].row = r;
          reqs[r].column_ids.reserve(n_cols);
          reqs[r].n_values.reserve(n_cols);
          for (uint32_t c = 0; c < n_cols; ++c) {
            reqs[r].column_ids.push_back((c * 5 + r) % 11);  // (repeats allowed)
            reqs[r].n_values.push_back(variant < 7 ? kValues[variant] : kValues[(c + 3 * r + n_queries) % 7]);
            values += reqs[r].n_values.back();
          }
        }
        for (uint32_t n_tiles : kTiles) {
          std::snprintf(g_shape, sizeof(g_shape), "queries %u, columns %u, variant %d, tiles %u", n_queries, n_cols,
                        variant, n_tiles);
          CheckShape(reqs, n_tiles, (n_queries + variant) % 2 ? fc::kBallotMaxValues : 0, n_tiles == kTiles[(n_queries + n_cols) % 3]);
          ++shapes;
          refused += values * 8 > fc::kArenaCap ? 1 : 0;
        }
      }
  // the cap itself: 64 queries x 8 columns x 65536 values x 8 bytes = 256 MiB exactly passes; one more value does not
  {
    std::vector<fc::Request> reqs(64);
    for (uint32_t r = 0; r < 64; ++r) {
      reqs[r].query = reqs[r].row = r;
      reqs[r].column_ids.assign(8, 0);
      reqs[r].n_values.assign(8, 65536);
    }
    std::snprintf(g_shape, sizeof(g_shape), "exactly the cap");
    fc::Plan plan;
    size_t bad = 0;
    CHECK(fc::Build(reqs, 3, 16, &plan, &bad) == fc::kOk && plan.arena_bytes == fc::kArenaCap);
    CheckShape(reqs, 3, 16);
    fc::Request one;
    one.query = one.row = 64;
    one.column_ids.assign(1, 0);
    one.n_values.assign(1, 1);
    reqs.push_back(one);
    std::snprintf(g_shape, sizeof(g_shape), "one value above the cap");
    CHECK(fc::Build(reqs, 3, 16, &plan, &bad) == fc::kArenaTooLarge && bad == 64);
    CheckShape(reqs, 3, 16);
    // more than kMaxColumns columns in one request
    reqs.resize(2);
    reqs[1].column_ids.assign(9, 0);
    reqs[1].n_values.assign(9, 1);
    CHECK(fc::Build(reqs, 3, 16, &plan, &bad) == fc::kTooManyColumns && bad == 1);
  }
  CHECK(refused > 0 && refused < shapes);
  std::printf("facet plan ok: %ld shapes (%ld above the arena cap), %ld checks\n", shapes, refused, g_checks);
  return 0;
}
