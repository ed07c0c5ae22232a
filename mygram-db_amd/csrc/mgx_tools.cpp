// mgx_tools.cpp — deterministic synthetic corpus generator (bench/test tooling, see include/mygram_tools.h).
#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "../../include/mygram_tools.h"
#include "mgx_fuzzy.hpp"
#include "mgx_highlight.hpp"

namespace {

inline uint64_t SplitMix64(uint64_t& x) {
  uint64_t z = (x += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

struct Xoshiro {
  uint64_t s[4];
  explicit Xoshiro(uint64_t seed) {
    for (auto& v : s) v = SplitMix64(seed);
  }
  static inline uint64_t Rotl(uint64_t x, int k) { return (x << k) | (x >> (64 - k)); }
  inline uint64_t Next() {
    const uint64_t r = Rotl(s[1] * 5, 7) * 9, t = s[1] << 17;
    s[2] ^= s[0];
    s[3] ^= s[1];
    s[1] ^= s[2];
    s[0] ^= s[3];
    s[2] ^= t;
    s[3] = Rotl(s[3], 45);
    return r;
  }
  inline double Uniform() { return static_cast<double>(Next() >> 11) * (1.0 / 9007199254740992.0); }
};

constexpr int kVocab = 20000;

struct Vocab {
  std::vector<std::string> words;
  std::vector<double> cdf;  // Zipf(s=1) over ranks 1..kVocab
  explicit Vocab(uint64_t seed) {
    static const char kLetters[] = "etaoinshrdlcumwfgypbvkjxqz";
    double lw[26], lsum = 0;
    for (int i = 0; i < 26; ++i) lsum += (lw[i] = 1.0 / (i + 1));
    double lcdf[26], acc = 0;
    for (int i = 0; i < 26; ++i) lcdf[i] = (acc += lw[i] / lsum);
    Xoshiro rng(seed ^ 0x5EEDC0DE5EEDC0DEull);
    words.reserve(kVocab);
    for (int w = 0; w < kVocab; ++w) {
      const int len = 2 + static_cast<int>(rng.Next() % 9);
      std::string s;
      for (int i = 0; i < len; ++i) {
        const double u = rng.Uniform();
        int k = 0;
        while (k < 25 && u > lcdf[k]) ++k;
        s.push_back(kLetters[k]);
      }
      words.push_back(std::move(s));
    }
    cdf.resize(kVocab);
    double zsum = 0;
    for (int r = 1; r <= kVocab; ++r) zsum += 1.0 / r;
    acc = 0;
    for (int r = 1; r <= kVocab; ++r) cdf[r - 1] = (acc += (1.0 / r) / zsum);
    cdf[kVocab - 1] = 1.0;
  }
};

}  // namespace

struct mgxt_corpus {
  std::vector<uint8_t> bytes;
  std::vector<uint64_t> off;
  uint64_t n_docs = 0;
};

extern "C" {

int mgxt_corpus_generate(uint64_t seed, uint64_t global_first, uint64_t n_docs, int n_threads, mgxt_corpus** out) {
  if (!out) return 2;
  *out = nullptr;
  try {
    const Vocab vocab(seed);
    unsigned hw = std::thread::hardware_concurrency();
    const unsigned nt = n_threads > 0 ? static_cast<unsigned>(n_threads) : (hw ? hw : 4);
    const uint64_t n_chunks = std::max<uint64_t>(1, std::min<uint64_t>((n_docs + 8191) / 8192, nt * 8ull));
    const uint64_t chunk = (n_docs + n_chunks - 1) / n_chunks;
    std::vector<std::vector<uint8_t>> cb(n_chunks);
    std::vector<std::vector<uint32_t>> cl(n_chunks);
    std::atomic<uint64_t> next{0};
    std::vector<std::thread> th;
    for (unsigned t = 0; t < nt; ++t) {
      th.emplace_back([&]() {
        for (;;) {
          const uint64_t c = next.fetch_add(1);
          if (c >= n_chunks) break;
          const uint64_t d0 = c * chunk, d1 = std::min(n_docs, d0 + chunk);
          auto& b = cb[c];
          auto& l = cl[c];
          b.reserve((d1 - d0) * 72);
          l.reserve(d1 - d0);
          for (uint64_t d = d0; d < d1; ++d) {
            uint64_t s = seed * 0xD1342543DE82EF95ull + (global_first + d) * 0x9E3779B97F4A7C15ull + 1;
            Xoshiro rng(s);
            const int n_words = 4 + static_cast<int>(rng.Next() % 13);
            const size_t start = b.size();
            for (int w = 0; w < n_words; ++w) {
              const double u = rng.Uniform();
              const size_t r = std::lower_bound(vocab.cdf.begin(), vocab.cdf.end(), u) - vocab.cdf.begin();
              const std::string& word = vocab.words[std::min<size_t>(r, kVocab - 1)];
              if (w) b.push_back(' ');
              b.insert(b.end(), word.begin(), word.end());
            }
            l.push_back(static_cast<uint32_t>(b.size() - start));
          }
        }
      });
    }
    for (auto& t : th) t.join();
    auto c = new mgxt_corpus();
    c->n_docs = n_docs;
    c->off.resize(n_docs + 1);
    uint64_t total = 0;
    for (auto& b : cb) total += b.size();
    c->bytes.resize(total + 16);
    uint64_t at = 0, d = 0;
    c->off[0] = 0;
    for (uint64_t k = 0; k < n_chunks; ++k) {
      if (!cb[k].empty()) std::memcpy(c->bytes.data() + at, cb[k].data(), cb[k].size());
      uint64_t o = at;
      for (uint32_t len : cl[k]) {
        o += len;
        c->off[++d] = o;
      }
      at += cb[k].size();
      std::vector<uint8_t>().swap(cb[k]);
    }
    *out = c;
    return 0;
  } catch (...) {
    return 5;
  }
}

int mgxt_corpus_view(const mgxt_corpus* c, const uint8_t** text_bytes, const uint64_t** text_off, uint64_t* n_docs) {
  if (!c || !text_bytes || !text_off || !n_docs) return 2;
  *text_bytes = c->bytes.data();
  *text_off = c->off.data();
  *n_docs = c->n_docs;
  return 0;
}

void mgxt_corpus_destroy(mgxt_corpus* c) { delete c; }

}  // extern "C"

extern "C" int mgxt_contains_fuzzy_match(const uint8_t* text, size_t text_len, const uint8_t* term, size_t term_len,
                                         uint32_t max_distance) {
  if ((text == nullptr && text_len != 0) || (term == nullptr && term_len != 0)) return -1;
  return mgx::fuzzy::ContainsFuzzyMatchD(text, text_len, term, term_len, max_distance);
}

// ---- highlighter: the host build of mgx_highlight.hpp ---------------------------------------------------------------
namespace {

namespace hl = mgx::highlight;

bool HighlightTerms(const uint8_t* text, size_t text_len, const uint8_t* const* terms, const size_t* term_lens,
                    uint32_t n_terms, std::vector<hl::Term>* out) {
  if ((text == nullptr && text_len != 0) || (n_terms != 0 && (!terms || !term_lens)) || text_len > 0x7FFFFFFFu) return false;
  for (uint32_t t = 0; t < n_terms; ++t) {
    if (terms[t] == nullptr && term_lens[t] != 0) return false;
    if (term_lens[t] == 0 || term_lens[t] > text_len) continue;  // (:257-262)
    const uint32_t len = static_cast<uint32_t>(term_lens[t]);
    out->push_back(hl::Term{terms[t], len, hl::CountCps(terms[t], len)});
  }
  return true;
}

}  // namespace

extern "C" int mgxt_highlight_match_positions(const uint8_t* text, size_t text_len, const uint8_t* const* terms,
                                              const size_t* term_lens, uint32_t n_terms, uint32_t* out_pairs,
                                              size_t cap_pairs, size_t* n_pairs) {
  if (n_pairs) *n_pairs = 0;
  std::vector<hl::Term> tv;
  if (!n_pairs || (cap_pairs != 0 && !out_pairs) || !HighlightTerms(text, text_len, terms, term_lens, n_terms, &tv)) return 2;
  std::vector<uint32_t> scratch(tv.size() + 1);
  hl::Scanner sc;
  sc.Init(text, static_cast<uint32_t>(text_len), tv.data(), static_cast<uint32_t>(tv.size()), scratch.data());
  size_t n = 0;
  uint32_t ms, me, bs, be;
  while (sc.Next(&ms, &me, &bs, &be)) {
    if (n < cap_pairs) {
      out_pairs[2 * n] = ms;
      out_pairs[2 * n + 1] = me;
    }
    ++n;
  }
  *n_pairs = n;
  return 0;
}

extern "C" int mgxt_highlight_generate(const uint8_t* text, size_t text_len, const uint8_t* const* terms,
                                       const size_t* term_lens, uint32_t n_terms, uint32_t snippet_length,
                                       uint32_t max_fragments, const uint8_t* open_tag, size_t open_len,
                                       const uint8_t* close_tag, size_t close_len, uint8_t* out, size_t cap,
                                       size_t* out_len) {
  if (out_len) *out_len = 0;
  std::vector<hl::Term> tv;
  if (!out_len || (cap != 0 && !out) || (open_len != 0 && !open_tag) || (close_len != 0 && !close_tag) ||
      !HighlightTerms(text, text_len, terms, term_lens, n_terms, &tv))
    return 2;
  if (snippet_length < 1 || snippet_length > hl::kMaxSnippetLength || max_fragments < 1 ||
      max_fragments > hl::kMaxFragments || open_len > hl::kMaxTagBytes || close_len > hl::kMaxTagBytes)
    return 3;
  if (text_len == 0) return 0;  // an empty text gives an empty snippet (:301-305)
  const uint32_t n = static_cast<uint32_t>(text_len);
  std::vector<uint32_t> scratch(tv.size() + 1);
  std::vector<hl::Window> win(max_fragments);
  std::vector<hl::Span> spans;
  // (a window of L code points holds at most L matches of one code point or more)
  const size_t span_cap = std::min<size_t>(static_cast<size_t>(max_fragments) * snippet_length, text_len);
  spans.resize(span_cap + 1);
  hl::Scanner sc;
  sc.Init(text, n, tv.data(), static_cast<uint32_t>(tv.size()), scratch.data());
  hl::Builder bd;
  bd.Init(snippet_length, max_fragments, win.data(), spans.data(), static_cast<uint32_t>(span_cap));
  uint32_t ms, me, bs, be;
  while (!bd.done && sc.Next(&ms, &me, &bs, &be)) bd.Feed(ms, me, bs, be, true);
  const uint32_t total = bd.done ? hl::kNoTotal : hl::CountCps(text, text_len);
  bd.Finish(total, true);
  hl::FinalizeWindows(win.data(), bd.n_win, bd.matched, snippet_length, total, &bd.flags);
  hl::Header h{bd.n_win, bd.flags, bd.n_spans, 0};
  h.n_bytes = hl::WindowsToBytes(text, n, win.data(), bd.n_win);
  *out_len = hl::Render(h, win.data(), spans.data(), text, true, open_tag, open_len, close_tag, close_len, out, cap);
  return 0;
}

// Highlighter::GenerateOriginal (:311-356) with the map given instead of a normalizer: the scalar path of the source
// highlight_original_kernel runs (translation, the pending-range filter, Builder, the code point -> byte walk).
extern "C" int mgxt_highlight_generate_original(const uint8_t* original, size_t original_len, const uint8_t* normalized,
                                                size_t normalized_len, uint32_t kind, const uint32_t* map_pairs,
                                                size_t n_pairs, const uint8_t* const* terms, const size_t* term_lens,
                                                uint32_t n_terms, uint32_t snippet_length, uint32_t max_fragments,
                                                const uint8_t* open_tag, size_t open_len, const uint8_t* close_tag,
                                                size_t close_len, uint8_t* out, size_t cap, size_t* out_len) {
  if (kind == hl::kOrigNone)
    return mgxt_highlight_generate(normalized, normalized_len, terms, term_lens, n_terms, snippet_length, max_fragments,
                                   open_tag, open_len, close_tag, close_len, out, cap, out_len);
  if (out_len) *out_len = 0;
  std::vector<hl::Term> tv;
  if (!out_len || (cap != 0 && !out) || (open_len != 0 && !open_tag) || (close_len != 0 && !close_tag) ||
      (original == nullptr && original_len != 0) || original_len > 0x7FFFFFFFu || kind > hl::kOrigUnmappable ||
      (n_pairs != 0 && !map_pairs) || n_pairs > 0x7FFFFFFFu ||
      !HighlightTerms(normalized, normalized_len, terms, term_lens, n_terms, &tv))
    return 2;
  if (snippet_length < 1 || snippet_length > hl::kMaxSnippetLength || max_fragments < 1 ||
      max_fragments > hl::kMaxFragments || open_len > hl::kMaxTagBytes || close_len > hl::kMaxTagBytes)
    return 3;
  if (original_len == 0) return 0;  // an empty original gives an empty snippet (:315-319)
  const uint32_t on = static_cast<uint32_t>(original_len);
  const uint32_t n = static_cast<uint32_t>(normalized_len);
  const hl::MapPair* map = reinterpret_cast<const hl::MapPair*>(map_pairs);
  std::vector<uint32_t> scratch(tv.size() + 1);
  std::vector<hl::Window> win(max_fragments);
  // (a window of L code points holds at most L matches, and every match is one of the normalized text's)
  const size_t span_cap = std::min<size_t>(static_cast<size_t>(max_fragments) * snippet_length, normalized_len);
  std::vector<hl::Span> spans(span_cap + 1);
  const hl::Header h = hl::GenerateOriginalRecord(original, on, normalized, n, kind, map, static_cast<uint32_t>(n_pairs),
                                                  tv.data(), static_cast<uint32_t>(tv.size()), snippet_length,
                                                  max_fragments, win.data(), spans.data(),
                                                  static_cast<uint32_t>(span_cap), scratch.data());
  *out_len = hl::Render(h, win.data(), spans.data(), original, true, open_tag, open_len, close_tag, close_len, out, cap);
  return 0;
}

// The pending-range filter of the same source over a list of (start, end) pairs with non-decreasing starts and ends.
extern "C" int mgxt_highlight_filter_ranges(const uint32_t* pairs, size_t n_pairs, uint32_t* out_pairs, size_t* n_out) {
  if (n_out) *n_out = 0;
  if (!n_out || (n_pairs != 0 && (!pairs || !out_pairs))) return 2;
  *n_out = hl::FilterRanges(reinterpret_cast<const hl::MapPair*>(pairs), n_pairs, reinterpret_cast<hl::MapPair*>(out_pairs));
  return 0;
}
