// build_host_check.cpp — the host-compiled pieces of the device column builder (mygram-db_amd/csrc/mgx_build.hpp and the
// device-usable helpers of mgx_text.hpp), stand-alone: g++ -std=c++17 [-fsanitize=address,undefined], no GPU, no HIP header.
//   1  key packing: integer order of the packed keys == order of the 128-bit host keys (bytewise order of the UTF-8
//      strings, shorter prefix first), injective, width and fields come back
//   2  the pointer form of WindowAt == the vector form
//   3  the byte-parallel decode rule of mgx_build.hip: a byte starts a code point exactly when it is no continuation byte
//      and ParseUtf8 accepts the sequence that begins there within the document == text::Decode
//   4  the storage plan and the out-of-memory verdict
// Exits non-zero at the first property that fails; prints "build host ok: <checks>".
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "../../mygram-db_amd/csrc/mgx_build.hpp"
#include "../../mygram-db_amd/csrc/mgx_text.hpp"

namespace {

using Key = unsigned __int128;
unsigned long long g_checks = 0;

#define CHECK(cond)                                                      \
  do {                                                                   \
    ++g_checks;                                                          \
    if (!(cond)) {                                                       \
      std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond);    \
      std::exit(1);                                                      \
    }                                                                    \
  } while (0)

// the host builder's key (mgx_columns.cpp MakeKey), restated
Key MakeKey(const uint8_t* b, size_t n) {
  Key k = 0;
  for (size_t i = 0; i < n; ++i) k |= static_cast<Key>(b[i]) << (8 * (15 - i));
  return k | static_cast<Key>(n);
}

struct Gram {
  uint32_t cp[3];
  int w;
  uint64_t packed;
  Key host;
};

Gram MakeGram(const uint32_t* cp, int w) {
  Gram g{};
  uint8_t buf[12];
  size_t nb = 0;
  for (int j = 0; j < w; ++j) {
    g.cp[j] = cp[j];
    nb += mgx::text::EncodeUtf8(cp[j], buf + nb);
  }
  g.w = w;
  g.packed = mgx::build::PackKey(cp, w);
  g.host = MakeKey(buf, nb);
  return g;
}

void CheckPacking() {
  const uint32_t edges[] = {0x0,    0x1,    0x7F,   0x80,    0x7FF,   0x800,    0xD7FF,  0xE000, 0xFFFF,
                            0x10000, 0x10FFFF, 0x41,  0x3042,  0x4E00,  0x9FFF,   0x20000};
  const size_t ne = sizeof(edges) / sizeof(edges[0]);
  std::vector<Gram> grams;
  for (size_t a = 0; a < ne; ++a) {
    grams.push_back(MakeGram(&edges[a], 1));
    for (size_t b = 0; b < ne; ++b) {
      const uint32_t two[2] = {edges[a], edges[b]};
      grams.push_back(MakeGram(two, 2));
      for (size_t c = 0; c < ne; ++c) {
        const uint32_t three[3] = {edges[a], edges[b], edges[c]};
        grams.push_back(MakeGram(three, 3));
      }
    }
  }
  std::mt19937_64 rng(7);
  auto any_cp = [&]() {
    for (;;) {
      const uint32_t r = static_cast<uint32_t>(rng());
      const uint32_t c = (r & 3) == 0 ? r % 0x80 : (r & 3) == 1 ? r % 0x800 : (r & 3) == 2 ? r % 0x10000 : r % 0x110000;
      if (c < 0xD800 || c > 0xDFFF) return c;
    }
  };
  for (int i = 0; i < 140000; ++i) {
    uint32_t cp[3] = {any_cp(), any_cp(), any_cp()};
    grams.push_back(MakeGram(cp, 1 + static_cast<int>(rng() % 3)));
  }
  for (const Gram& g : grams) {
    CHECK(g.packed < mgx::build::kNoWindow);
    CHECK(g.packed >> mgx::build::kSortBits == 0);
    CHECK(mgx::build::KeyWidth(g.packed) == g.w);
    for (int j = 0; j < 3; ++j) CHECK(mgx::build::KeyField(g.packed, j) == (j < g.w ? g.cp[j] + 1 : 0u));
  }
  std::sort(grams.begin(), grams.end(), [](const Gram& a, const Gram& b) { return a.packed < b.packed; });
  for (size_t i = 1; i < grams.size(); ++i) {
    const Gram &a = grams[i - 1], &b = grams[i];
    if (a.packed == b.packed) CHECK(a.host == b.host);  // the same gram drawn twice
    else CHECK(a.host < b.host);                        // order kept, and distinct stays distinct
  }
}

void CheckWindowAt() {
  std::mt19937 rng(11);
  const uint32_t pool[] = {'a', 'b', ' ', 0x3042, 0x30AB, 0x4E00, 0x6771, 0x20000, 0x3400, 0xF900, 0x10FFFF, 0};
  for (int it = 0; it < 4000; ++it) {
    std::vector<uint32_t> cps(rng() % 9);
    for (auto& c : cps) c = pool[rng() % (sizeof(pool) / sizeof(pool[0]))];
    for (int an = 0; an <= 3; ++an)
      for (int kn = 0; kn <= 3; ++kn)
        for (int cross = 0; cross < 2; ++cross)
          for (size_t p = 0; p < cps.size(); ++p) {
            const int want = mgx::text::WindowAt(cps, p, an, kn, cross != 0);
            CHECK(mgx::text::WindowAt(cps.data(), cps.size(), p, an, kn, cross != 0) == want);
            // as gram_windows_kernel calls it: the (at most 3) code points from p on, p = 0
            uint32_t c[3] = {0, 0, 0};
            const size_t left = cps.size() - p;
            for (size_t j = 0; j < 3 && j < left; ++j) c[j] = cps[p + j];
            CHECK(mgx::text::WindowAt(c, left < 3 ? left : 3, 0, an, kn, cross != 0) == want);
          }
  }
}

void CheckByteParallelDecode() {
  std::mt19937 rng(13);
  const uint8_t interesting[] = {0x00, 0x41, 0x7F, 0x80, 0xBF, 0xC0, 0xC1, 0xC2, 0xDF, 0xE0, 0xE1, 0xED, 0xEF,
                                 0xF0, 0xF4, 0xF5, 0xFF, 0xA0, 0x90, 0x8F, 0x9F};
  for (int it = 0; it < 60000; ++it) {
    std::vector<uint8_t> t(rng() % 24);
    for (auto& b : t) b = (rng() % 4) ? interesting[rng() % sizeof(interesting)] : static_cast<uint8_t>(rng());
    std::vector<uint32_t> want, got;
    mgx::text::Decode(t.data(), t.size(), &want);
    for (size_t i = 0; i < t.size(); ++i) {
      if ((t[i] & 0xC0) == 0x80) continue;
      uint8_t b[4] = {0xAA, 0xAA, 0xAA, 0xAA};  // (what lies behind the document must not matter: continuation bytes here)
      for (size_t j = 0; j < 4 && i + j < t.size(); ++j) b[j] = t[i + j];
      uint32_t cp = 0;
      if (mgx::text::ParseUtf8(b, t.size() - i, &cp) > 0) got.push_back(cp);
    }
    CHECK(got == want);
  }
}

void CheckPlan() {
  using namespace mgx::build;
  const uint64_t docs[] = {0, 1, 63, 8000, 24000, 1000000};
  const uint64_t bytes[] = {0, 1, 15, 16, 17, 4095, 4096, 4097, 1000000, 3000000000ull, kMaxTextBytes};
  uint64_t prev_needed = 0;
  for (uint64_t nd : docs) {
    prev_needed = 0;
    for (uint64_t nb : bytes) {
      const Layout l = PlanLayout(nd, nb);
      CHECK(l.n_lanes * kLaneBytes >= nb && (l.n_lanes == 0 || (l.n_lanes - 1) * kLaneBytes < nb));
      CHECK(l.n_blocks * kBlockThreads >= l.n_lanes);
      const uint64_t offs[] = {l.text,    l.text_off, l.lane_mask, l.lane_prefix, l.block_count, l.block_base, l.doc_cp_off,
                               l.doc_len, l.cps,      l.cp_doc,    l.key0,        l.key1,        l.val0,       l.val1,
                               l.gram_keys, l.gram_off, l.overflow, l.counters,   l.bytes};
      const uint64_t rec = nb + 1, lanes = l.n_blocks * kBlockThreads;
      const uint64_t need[] = {lanes * kLaneBytes + 20, (nd + 1) * 8, lanes * 2, lanes * 4, (l.n_blocks + 1) * 4,
                               (l.n_blocks + 1) * 4,    (nd + 1) * 4, nd * 4,    rec * 4,   rec * 4,
                               rec * 8,                 rec * 8,      rec * 8,   rec * 8,   nb * 8,
                               nb * 8,                  (nb / 255 + 1) * 8, 8};
      for (size_t i = 0; i + 1 < sizeof(offs) / sizeof(offs[0]); ++i) {
        CHECK(offs[i] % 256 == 0);
        CHECK(offs[i] + need[i] <= offs[i + 1]);  // in order, room for what the kernels write, no overlap
      }
      const Budget exact = PlanBudget(nd, nb, 0);
      CHECK(!exact.fits && exact.needed == l.bytes + kLibrarySlack + nb);
      CHECK(PlanBudget(nd, nb, exact.needed).fits);
      CHECK(!PlanBudget(nd, nb, exact.needed - 1).fits);
      CHECK(PlanBudget(nd, nb, ~0ull).fits);
      CHECK(exact.needed >= prev_needed);  // more text never needs less
      prev_needed = exact.needed;
    }
  }
  // the figures a reader can check by hand: per text byte 1 (text) + 3/8 (lane mask and prefix) + 8 (code point, its
  // document) + 32 (two buffers of key and value) + 16 (gram keys and offsets) + 1 (library calls) = 58.4 B, and 64 MiB
  const Budget b = PlanBudget(8000, 1000000, 0);
  CHECK(b.needed > 58ull * 1000000 + kLibrarySlack && b.needed < 59ull * 1000000 + kLibrarySlack);
}

}  // namespace

int main() {
  CheckPacking();
  CheckWindowAt();
  CheckByteParallelDecode();
  CheckPlan();
  std::printf("build host ok: %llu checks\n", g_checks);
  return 0;
}
