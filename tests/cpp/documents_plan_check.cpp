// Stand-alone check of the page-documents planner and of the host restatement of the gather (mgx_documents.hpp): no HIP,
// no GPU. Built by tests/test_documents_plan_cpu.py and `make documents-host-asan` with -fsanitize=address,undefined.
//   plan    for (queries of {1, 2, 7, 64, 1024}) x (limits of {1, 10, 1000, 1024}, the same for every query or mixed) x
//           (columns 0..32) x (key capacities of {0, 1, 7, 8, 9, 63, 64, 65, 255, 256, 257, 300}) x (late pattern: none,
//           all, every third): the records of all (query, entry) pairs are disjoint, 8-byte aligned and inside the arena;
//           the early queries' records fill [0, early_bytes) and the late ones' [early_bytes, arena_bytes); the column
//           ranges are back to back; limit 0, limit 1025 and 33 columns are refused at their request;
//   cap     the refusal fires exactly where the running sum of limit * stride passes 256 MiB, worked out independently;
//   gather  over small tables whose every array is a heap allocation of its exact size (so that the sanitizer sees a read
//           outside any of them): mapped + plain sources, has_key or not, columns with and without NULL arrays and
//           absent columns, key capacities below, at and above the keys' lengths, doc ids below, inside, between and
//           above both indexes' ranges. Every record must equal a model built from the same arrays by doc id.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <string>
#include <vector>

#include "../../mygram-db_amd/csrc/mgx_documents.hpp"

namespace dc = mgx::documents;

static long g_checks = 0;
static char g_shape[200];
#define CHECK(cond)                                                                               \
  do {                                                                                            \
    ++g_checks;                                                                                   \
    if (!(cond)) {                                                                                \
      std::fprintf(stderr, "%s:%d: CHECK(%s) failed (%s)\n", __FILE__, __LINE__, #cond, g_shape); \
      std::exit(1);                                                                               \
    }                                                                                             \
  } while (0)

static long g_shapes = 0;

static void CheckPlan(const std::vector<dc::Request>& reqs, uint32_t key_cap) {
  ++g_shapes;
  // what the planner must decide, worked out independently
  size_t refuse_at = reqs.size();
  dc::Status want = dc::kOk;
  uint64_t sum = 0;
  for (size_t r = 0; r < reqs.size(); ++r) {
    if (reqs[r].n_columns > 32) { refuse_at = r; want = dc::kTooManyColumns; break; }
    if (reqs[r].limit == 0 || reqs[r].limit > 1024) { refuse_at = r; want = dc::kBadLimit; break; }
    const uint64_t stride = 16 + 8ull * reqs[r].n_columns + (static_cast<uint64_t>(key_cap) + 7) / 8 * 8;
    sum += stride * reqs[r].limit;
    if (sum > (256ull << 20)) { refuse_at = r; want = dc::kArenaTooLarge; break; }
  }
  dc::Plan plan;
  size_t bad = ~static_cast<size_t>(0);
  const dc::Status st = dc::Build(reqs, key_cap, &plan, &bad);
  CHECK(st == want);
  if (want != dc::kOk) {
    CHECK(bad == refuse_at);
    return;
  }
  CHECK(plan.queries.size() == reqs.size());
  CHECK(plan.arena_bytes == sum && plan.arena_bytes <= dc::kArenaCap && plan.key_cap == key_cap);
  std::vector<std::pair<uint64_t, uint64_t>> spans;  // [begin, end) of every query's records
  uint32_t cols = 0, entries = 0;
  uint64_t early = 0;
  for (size_t r = 0; r < reqs.size(); ++r) {
    const dc::QueryPlan& q = plan.queries[r];
    CHECK(q.query == reqs[r].query && q.limit == reqs[r].limit && q.n_columns == reqs[r].n_columns);
    CHECK(q.late == (reqs[r].late ? 1u : 0u));
    CHECK(q.col_begin == cols);
    cols += q.n_columns;
    CHECK(q.rec_stride == dc::RecordStride(q.n_columns, key_cap));
    CHECK(q.rec_stride % 8 == 0 && q.rec_off % 8 == 0);
    CHECK(q.rec_stride >= sizeof(dc::Header) + 8ull * q.n_columns + key_cap);  // header, values and a full key fit
    const uint64_t end = q.rec_off + q.rec_stride * q.limit;
    CHECK(end <= plan.arena_bytes);
    if (q.late) {
      CHECK(q.rec_off >= plan.early_bytes);
    } else {
      CHECK(end <= plan.early_bytes);
      CHECK(q.entry_begin == entries);
      entries += q.limit;
      early += q.rec_stride * q.limit;
    }
    spans.emplace_back(q.rec_off, end);
  }
  CHECK(cols == plan.n_columns && entries == plan.early_entries && early == plan.early_bytes);
  // disjoint: sorted by begin, each begins where the one before ends or later; records inside a span are disjoint by
  // their stride
  std::sort(spans.begin(), spans.end());
  for (size_t i = 1; i < spans.size(); ++i) CHECK(spans[i].first >= spans[i - 1].second);
}

static void SweepPlans() {
  const uint32_t n_queries[] = {1, 2, 7, 64, 1024};
  const uint32_t limits[] = {1, 10, 1000, 1024};
  const uint32_t key_caps[] = {0, 1, 7, 8, 9, 63, 64, 65, 255, 256, 257, 300};
  for (uint32_t nq : n_queries)
    for (int mixed = 0; mixed < 2; ++mixed)
      for (uint32_t lim : limits)
        for (uint32_t nc = 0; nc <= 32; ++nc)
          for (uint32_t kc : key_caps)
            for (int late = 0; late < 3; ++late) {
              std::snprintf(g_shape, sizeof g_shape, "queries %u mixed %d limit %u columns %u key_cap %u late %d", nq, mixed,
                            lim, nc, kc, late);
              std::vector<dc::Request> reqs(nq);
              for (uint32_t i = 0; i < nq; ++i) {
                reqs[i].query = i * 2 + 1;
                reqs[i].limit = mixed ? limits[(i + lim) % 4] : lim;
                reqs[i].n_columns = mixed ? (nc + i) % 33 : nc;
                reqs[i].late = late == 1 || (late == 2 && i % 3 == 0);
              }
              CheckPlan(reqs, kc);
            }
  // the refusals of one request, in the middle of a list
  for (uint32_t bad_limit : {0u, 1025u, 0xFFFFFFFFu}) {
    std::snprintf(g_shape, sizeof g_shape, "limit %u", bad_limit);
    std::vector<dc::Request> reqs(5);
    for (uint32_t i = 0; i < 5; ++i) reqs[i] = dc::Request{i, 10, 2, 0};
    reqs[3].limit = bad_limit;
    CheckPlan(reqs, 16);
  }
  {
    std::snprintf(g_shape, sizeof g_shape, "33 columns");
    std::vector<dc::Request> reqs(5);
    for (uint32_t i = 0; i < 5; ++i) reqs[i] = dc::Request{i, 10, 2, 0};
    reqs[2].n_columns = 33;
    CheckPlan(reqs, 16);
  }
  // the cap, at its edge: q queries of limit 1024 whose records are (256 MiB / 1024 / q) bytes exactly fill the arena; one
  // more byte of key capacity per record (rounded up to 8) passes it, at the last request
  for (uint32_t q : {1u, 4u, 64u, 512u}) {
    const uint64_t stride = (256ull << 20) / 1024 / q;  // a multiple of 8
    for (int over = 0; over < 2; ++over) {
      const uint32_t nc = 32;
      const uint32_t kc = static_cast<uint32_t>(stride - 16 - 8 * nc) + (over ? 1 : 0);
      std::snprintf(g_shape, sizeof g_shape, "cap edge: %u queries, key_cap %u", q, kc);
      std::vector<dc::Request> reqs(q);
      for (uint32_t i = 0; i < q; ++i) reqs[i] = dc::Request{i, 1024, nc, i & 1u};
      dc::Plan plan;
      size_t bad = 0;
      const dc::Status st = dc::Build(reqs, kc, &plan, &bad);
      if (over) {
        CHECK(st == dc::kArenaTooLarge);
      } else {
        CHECK(st == dc::kOk && plan.arena_bytes == dc::kArenaCap);
      }
      CheckPlan(reqs, kc);
    }
  }
}

// ---- the gather over exact-size heap arrays ----
template <typename T>
static std::unique_ptr<T[]> Exact(const std::vector<T>& v) {
  std::unique_ptr<T[]> p(new T[v.size()]);  // (size 0: a valid pointer no read may touch)
  std::copy(v.begin(), v.end(), p.get());
  return p;
}

struct HostIndex {
  std::vector<std::string> keys;
  std::vector<uint8_t> has;
  std::vector<uint32_t> doc_map;
  uint32_t first = 0;
  std::vector<std::vector<uint64_t>> values;
  std::vector<std::vector<uint8_t>> nulls;  // empty vector: no NULL array
  // exact-size copies
  std::unique_ptr<uint8_t[]> d_bytes, d_has;
  std::unique_ptr<uint64_t[]> d_off;
  std::unique_ptr<uint32_t[]> d_map;
  std::vector<std::unique_ptr<uint64_t[]>> d_values;
  std::vector<std::unique_ptr<uint8_t[]>> d_nulls;
  std::unique_ptr<dc::DevColumn[]> d_cols;

  dc::DevSource Source(const std::vector<int>& request, bool with_has, bool with_map) {
    std::vector<uint8_t> bytes;
    std::vector<uint64_t> off(1, 0);
    for (const std::string& k : keys) {
      bytes.insert(bytes.end(), k.begin(), k.end());
      off.push_back(bytes.size());
    }
    d_bytes = Exact(bytes);
    d_off = Exact(off);
    d_has = Exact(has);
    d_map = Exact(doc_map);
    d_values.clear();
    d_nulls.clear();
    for (size_t c = 0; c < values.size(); ++c) {
      d_values.push_back(Exact(values[c]));
      d_nulls.push_back(Exact(nulls[c]));
    }
    std::vector<dc::DevColumn> cols;
    for (int c : request) {
      if (c < 0) cols.push_back(dc::DevColumn{nullptr, nullptr});
      else cols.push_back(dc::DevColumn{d_values[c].get(), nulls[c].empty() ? nullptr : d_nulls[c].get()});
    }
    d_cols = Exact(cols);
    dc::DevSource s{};
    s.key_bytes = d_bytes.get();
    s.key_off = d_off.get();
    s.has_key = with_has ? d_has.get() : nullptr;
    s.doc_map = with_map ? d_map.get() : nullptr;
    s.columns = d_cols.get();
    s.first_doc_id = first;
    s.n_docs = static_cast<uint32_t>(keys.size());
    return s;
  }
};

static HostIndex MakeIndex(uint32_t n, uint32_t first, uint32_t seed, bool mapped) {
  HostIndex ix;
  ix.first = first;
  uint32_t id = first;
  for (uint32_t i = 0; i < n; ++i) {
    const uint32_t len = (i * 7 + seed) % 5 == 0 ? 0 : (i * 13 + seed) % 21;
    std::string k;
    for (uint32_t b = 0; b < len; ++b) k.push_back(static_cast<char>(0x80 + (i + b + seed) % 0x7F));
    ix.keys.push_back(k);
    ix.has.push_back((i + seed) % 4 != 0);
    id += 1 + (mapped ? (i * 5 + seed) % 3 : 0);
    ix.doc_map.push_back(id);
  }
  ix.values.resize(3);
  ix.nulls.resize(3);
  for (uint32_t c = 0; c < 3; ++c)
    for (uint32_t i = 0; i < n; ++i) {
      ix.values[c].push_back(0x9E3779B97F4A7C15ull * (i + 1) + c + seed);
      if (c != 1) ix.nulls[c].push_back((i + c + seed) % 3 == 0);  // column 1 has no NULL array
    }
  return ix;
}

static void SweepGather() {
  const std::vector<std::vector<int>> requests = {{}, {0}, {1, 1}, {2, -1, 0}, {0, 1, 2, -1, 2, 1, 0, 0}};
  std::vector<int> wide;
  for (int c = 0; c < 32; ++c) wide.push_back(c % 4 - 1);
  for (uint32_t n_plain : {0u, 1u, 17u})
    for (uint32_t n_mapped : {0u, 1u, 9u})
      for (int with_has = 0; with_has < 2; ++with_has)
        for (uint32_t key_cap : {0u, 1u, 7u, 8u, 20u, 21u})
          for (size_t ri = 0; ri <= requests.size(); ++ri) {
            const std::vector<int>& request = ri < requests.size() ? requests[ri] : wide;
            std::snprintf(g_shape, sizeof g_shape, "gather: plain %u mapped %u has %d key_cap %u request %zu", n_plain,
                          n_mapped, with_has, key_cap, ri);
            ++g_shapes;
            HostIndex plain = MakeIndex(n_plain, 5, 1, false);
            HostIndex mapped = MakeIndex(n_mapped, 2, 2, true);
            const dc::DevSource sp = plain.Source(request, with_has != 0, false);
            dc::DevSource sm = mapped.Source(request, with_has != 0, true);
            if (n_mapped == 0) sm = dc::DevSource{};  // (no delta at all)
            const uint32_t nc = static_cast<uint32_t>(request.size());
            const uint64_t stride = dc::RecordStride(nc, key_cap);
            std::unique_ptr<uint8_t[]> rec(new uint8_t[stride]);
            for (uint32_t doc = 0; doc < 60; ++doc) {
              std::memset(rec.get(), 0xCD, stride);
              dc::GatherEntryHost(sm, sp, doc, nc, 0, key_cap, rec.get());
              dc::Header h;
              std::memcpy(&h, rec.get(), sizeof h);
              // the model: the mapped index by its doc map first, then the plain index by doc - first
              const HostIndex* src = nullptr;
              uint32_t slot = 0;
              if (n_mapped != 0)
                for (uint32_t i = 0; i < n_mapped; ++i)
                  if (mapped.doc_map[i] == doc) { src = &mapped; slot = i; }
              if (!src && doc >= plain.first && doc - plain.first < n_plain) { src = &plain; slot = doc - plain.first; }
              if (!src) {
                CHECK(h.flags == 0 && h.key_len == 0 && h.null_mask == 0 && h.n_columns == 0);
                continue;
              }
              CHECK((h.flags & dc::kFound) != 0);
              CHECK(((h.flags & dc::kMapped) != 0) == (src == &mapped));
              CHECK(h.n_columns == nc);
              const bool has = !with_has || src->has[slot] != 0;
              CHECK(((h.flags & dc::kHasKey) != 0) == has);
              const std::string& k = src->keys[slot];
              if (has) {
                const bool cut = k.size() > key_cap;
                CHECK(((h.flags & dc::kTruncated) != 0) == cut);
                CHECK(h.key_len == (cut ? key_cap : k.size()));
                CHECK(std::memcmp(rec.get() + 16 + 8ull * nc, k.data(), h.key_len) == 0);
              } else {
                CHECK(h.key_len == 0);
              }
              for (uint32_t c = 0; c < nc; ++c) {
                const int col = request[c];
                const bool nul = col < 0 || (!src->nulls[col].empty() && src->nulls[col][slot] != 0);
                CHECK(((h.null_mask >> c) & 1u) == (nul ? 1u : 0u));
                uint64_t v;
                std::memcpy(&v, rec.get() + 16 + 8ull * c, 8);
                CHECK(v == (nul ? 0 : src->values[col][slot]));
              }
              // nothing behind the key's bytes was written
              for (uint64_t o = 16 + 8ull * nc + h.key_len; o < stride; ++o) CHECK(rec[o] == 0xCD);
            }
          }
}

int main() {
  SweepPlans();
  SweepGather();
  std::printf("documents plan ok: %ld shapes, %ld checks\n", g_shapes, g_checks);
  return 0;
}
