// highlight_original_host_check.cpp — the host build of mgx_highlight.hpp's original-text path (TranslateMatch, the
// pending-range filter, Builder, the code point -> byte walk, Render) as a stand-alone program, without a GPU and without
// Python in between. Reads lines
//   gen <original hex|-> <normalized hex|-> <kind> <n_pairs> (<start> <end>) x n_pairs <n_terms> <term hex|-> x n_terms
//       <snippet_length> <max_fragments> <open tag hex|-> <close tag hex|-> <expected snippet hex|->
//   flt <n> (<start> <end>) x n <m> (<start> <end>) x m        (ranges in, the ranges RemoveOverlappingMatchPositions keeps)
// written by tests/test_highlight_original_cpu.py from the Python restatement and checks every one.
// `make highlight-original-host-asan` builds it with -fsanitize=address,undefined.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../mygram-db_amd/csrc/mgx_highlight.hpp"

namespace hl = mgx::highlight;

static bool ReadHex(std::FILE* f, std::vector<uint8_t>* out) {
  static char buf[1 << 20];
  out->clear();
  if (std::fscanf(f, "%1048575s", buf) != 1) return false;
  if (std::strcmp(buf, "-") == 0) return true;
  const size_t n = std::strlen(buf);
  if (n % 2) return false;
  for (size_t i = 0; i < n; i += 2) {
    unsigned v = 0;
    if (std::sscanf(buf + i, "%2x", &v) != 1) return false;
    out->push_back(static_cast<uint8_t>(v));
  }
  return true;
}

static bool ReadPairs(std::FILE* f, std::vector<hl::MapPair>* out) {
  size_t n = 0;
  if (std::fscanf(f, "%zu", &n) != 1) return false;
  out->resize(n);
  for (size_t i = 0; i < n; ++i)
    if (std::fscanf(f, "%u %u", &(*out)[i].first, &(*out)[i].second) != 2) return false;
  return true;
}

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  std::FILE* f = std::fopen(argv[1], "r");
  if (!f) return 2;
  char what[8];
  int lines = 0, bad = 0;
  while (std::fscanf(f, "%7s", what) == 1) {
    ++lines;
    if (std::strcmp(what, "gen") == 0) {
      std::vector<uint8_t> original, normalized, open_tag, close_tag, want;
      std::vector<hl::MapPair> pairs;
      unsigned kind = 0, n_terms = 0, L = 0, F = 0;
      if (!ReadHex(f, &original) || !ReadHex(f, &normalized) || std::fscanf(f, "%u", &kind) != 1 || !ReadPairs(f, &pairs) ||
          std::fscanf(f, "%u", &n_terms) != 1)
        return 2;
      std::vector<std::vector<uint8_t>> term_bytes(n_terms);
      for (auto& t : term_bytes)
        if (!ReadHex(f, &t)) return 2;
      if (std::fscanf(f, "%u %u", &L, &F) != 2 || !ReadHex(f, &open_tag) || !ReadHex(f, &close_tag) || !ReadHex(f, &want))
        return 2;
      std::vector<hl::Term> terms;
      for (const auto& t : term_bytes) {
        if (t.empty() || t.size() > normalized.size()) continue;  // (:257-262)
        terms.push_back(hl::Term{t.data(), static_cast<uint32_t>(t.size()), hl::CountCps(t.data(), t.size())});
      }
      std::vector<uint8_t> got;
      if (!original.empty()) {
        // exact-size arrays, so that a sanitizer sees any step outside them
        std::vector<hl::Window> win(F);
        const size_t span_cap = std::min<size_t>(static_cast<size_t>(F) * L, normalized.size());
        std::vector<hl::Span> spans(span_cap);
        std::vector<uint32_t> scratch(terms.size() + 1);
        const hl::Header h = hl::GenerateOriginalRecord(
            original.data(), static_cast<uint32_t>(original.size()), normalized.data(),
            static_cast<uint32_t>(normalized.size()), kind, pairs.data(), static_cast<uint32_t>(pairs.size()), terms.data(),
            static_cast<uint32_t>(terms.size()), L, F, win.data(), spans.data(), static_cast<uint32_t>(span_cap),
            scratch.data());
        const size_t n = hl::Render(h, win.data(), spans.data(), original.data(), true, open_tag.data(), open_tag.size(),
                                    close_tag.data(), close_tag.size(), nullptr, 0);
        got.resize(n);
        hl::Render(h, win.data(), spans.data(), original.data(), true, open_tag.data(), open_tag.size(), close_tag.data(),
                   close_tag.size(), got.data(), got.size());
        if (!(h.flags & hl::kFlagOriginal) || (h.flags & hl::kFlagOverflow)) {
          ++bad;
          std::printf("line %d: flags %u\n", lines, h.flags);
        }
      }
      if (got != want) {
        ++bad;
        std::printf("line %d: snippet differs\n", lines);
      }
    } else if (std::strcmp(what, "flt") == 0) {
      std::vector<hl::MapPair> in, want;
      if (!ReadPairs(f, &in) || !ReadPairs(f, &want)) return 2;
      std::vector<hl::MapPair> out(in.size());
      out.resize(hl::FilterRanges(in.data(), in.size(), out.data()));
      bool same = out.size() == want.size();
      for (size_t i = 0; same && i < out.size(); ++i)
        same = out[i].first == want[i].first && out[i].second == want[i].second;
      if (!same) {
        ++bad;
        std::printf("line %d: kept ranges differ\n", lines);
      }
    } else {
      return 2;
    }
  }
  std::fclose(f);
  std::printf("%d lines, %d bad\n", lines, bad);
  return bad ? 1 : 0;
}
