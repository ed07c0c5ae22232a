// mgx_fuzzy.hpp — ContainsFuzzyMatch (src/utils/edit_distance.cpp:199-296, with :75-156) for one (text, term, d):
// the ONE implementation of the FUZZY verify_text post-filter (PostFilterByFuzzyText, search_pipeline.cpp:1746-1755).
// The tile kernel (kOpVerifyFuzzy, mgx_kernels.hip) compiles it for the device and mgx_tools.cpp (g++) exports the host
// build as mgxt_contains_fuzzy_match, the hook the CPU differential test calls. Paths are relative to the reference tree.
//
// The rules, as the reference applies them:
//   * U+3000 and U+00A0 are read as a space (NormalizeUnicodeWhitespace :24-47, a byte-level scan), words are split on
//     space, \t, \r, \n;
//   * an all-ASCII word matches when its code-point Levenshtein distance to the term is <= d;
//   * any other word matches when some code-point window of it, of length in [max(1, m-d), min(m+d, word length)]
//     (m = term length in code points), is within d of the term (ContainsFuzzyCodepointWindow :129-156);
//   * words and the term are decoded like Utf8ToCodepoints (invalid bytes skipped).
//
// Every distance is decided by ONE banded dynamic program: an alignment of cost <= d never leaves the diagonals
// |i - j| <= d, so a row of the term-by-word matrix has 2d+1 live cells (5 for d = 2), kept in registers. Rows follow the
// term's code points and the band's word code points slide along, both decoded as they are needed, so neither side has
// a length limit and nothing is staged in memory. The window rule runs the program once per start position of the word:
// the last row then holds the distances of the windows of every admissible length at once. A row whose cells all exceed
// d ends the program (the row minimum never decreases, :111-117).
#pragma once

#include <cstddef>
#include <cstdint>

#include "mgx_text.hpp"

#if defined(__HIPCC__)
#define MGX_FZ_HD __host__ __device__ inline
#else
#define MGX_FZ_HD inline
#endif
#if defined(__clang__)
#define MGX_FZ_UNROLL _Pragma("unroll")
#else
#define MGX_FZ_UNROLL
#endif

namespace mgx::fuzzy {

constexpr uint32_t kNoCp = 0xFFFFFFFFu;  // past the end of a word; equal to no decoded code point

// The next code point of b[pos, end), invalid bytes skipped (Utf8ToCodepoints, string_utils.cpp:199-218), or kNoCp.
MGX_FZ_HD uint32_t NextCp(const uint8_t* b, size_t end, size_t& pos) {
  while (pos < end) {
    uint32_t c = 0;
    const int k = text::ParseUtf8(b + pos, end - pos, &c);
    if (k > 0) {
      pos += static_cast<size_t>(k);
      return c;
    }
    ++pos;
  }
  return kNoCp;
}

MGX_FZ_HD uint32_t CountCps(const uint8_t* b, size_t begin, size_t end) {
  uint32_t n = 0;
  while (NextCp(b, end, begin) != kNoCp) ++n;
  return n;
}

// Bytes of the separator at t[i] after NormalizeUnicodeWhitespace, or 0 for a word byte.
MGX_FZ_HD uint32_t SeparatorAt(const uint8_t* t, size_t n, size_t i) {
  const uint8_t c = t[i];
  if (c == ' ' || c == '\t' || c == '\r' || c == '\n') return 1;
  if (c == 0xE3 && i + 2 < n && t[i + 1] == 0x80 && t[i + 2] == 0x80) return 3;  // U+3000
  if (c == 0xC2 && i + 1 < n && t[i + 1] == 0xA0) return 2;                      // U+00A0
  return 0;
}

// Banded Levenshtein program of the term (m code points, rows) against the word's code points from byte `wpos` on
// (`avail` of them before `wend`, columns). whole: is the distance to all `avail` code points <= D? Otherwise: is some
// prefix of length j in [max(1, m-D), min(m+D, avail)] within D (one start position of the window rule)?
template <int D>
MGX_FZ_HD bool BandWithin(const uint8_t* w, size_t wpos, size_t wend, uint32_t avail, const uint8_t* term, size_t tlen,
                          uint32_t m, bool whole) {
  constexpr int B = 2 * D + 1;
  constexpr uint32_t kInf = 0x40000000u;
  uint32_t cell[B];  // row i: cell[k] = distance(term[0, i), word[0, i + k - D))
  uint32_t win[B];   // row i: win[k] = word code point i + k - D - 1 (the column's own), kNoCp outside the word
  MGX_FZ_UNROLL
  for (int k = 0; k < B; ++k) {
    const int j = k - D;
    cell[k] = (j >= 0 && static_cast<uint32_t>(j) <= avail) ? static_cast<uint32_t>(j) : kInf;
  }
  size_t p = wpos;
  MGX_FZ_UNROLL
  for (int k = 0; k < B; ++k) win[k] = k < D ? kNoCp : NextCp(w, wend, p);
  size_t tp = 0;
  for (uint32_t i = 1; i <= m; ++i) {
    const uint32_t tc = NextCp(term, tlen, tp);
    uint32_t row_min = kInf;
    uint32_t left = kInf;
    MGX_FZ_UNROLL
    for (int k = 0; k < B; ++k) {
      const int64_t j = static_cast<int64_t>(i) + k - D;
      uint32_t v = kInf;
      if (j == 0) {
        v = i;
      } else if (j > 0 && j <= static_cast<int64_t>(avail)) {
        v = cell[k] + (win[k] == tc ? 0u : 1u);           // substitute / match: (i-1, j-1)
        if (k + 1 < B && cell[k + 1] + 1 < v) v = cell[k + 1] + 1;  // (i-1, j)
        if (left + 1 < v) v = left + 1;                   // (i, j-1)
      }
      if (v > kInf) v = kInf;
      cell[k] = v;  // (cell[k] of row i-1 is not read again: the next cell reads cell[k+1] of row i-1)
      left = v;
      if (v < row_min) row_min = v;
    }
    if (row_min > static_cast<uint32_t>(D)) return false;
    MGX_FZ_UNROLL
    for (int k = 0; k + 1 < B; ++k) win[k] = win[k + 1];
    win[B - 1] = NextCp(w, wend, p);
  }
  if (whole) {
    const int64_t k = static_cast<int64_t>(avail) - m + D;
    bool ok = false;
    MGX_FZ_UNROLL
    for (int kk = 0; kk < B; ++kk) ok = ok || (kk == k && cell[kk] <= static_cast<uint32_t>(D));
    return ok;
  }
  bool ok = false;
  MGX_FZ_UNROLL
  for (int k = 0; k < B; ++k) {
    const int64_t j = static_cast<int64_t>(m) + k - D;
    ok = ok || (j >= 1 && j <= static_cast<int64_t>(avail) && cell[k] <= static_cast<uint32_t>(D));
  }
  return ok;
}

// ContainsFuzzyMatch(text, term, D), edit_distance.cpp:199-296.
template <int D>
MGX_FZ_HD bool ContainsFuzzyMatch(const uint8_t* text, size_t n, const uint8_t* term, size_t tlen) {
  if (tlen == 0) return true;
  if (n == 0) return false;
  const uint32_t m = CountCps(term, 0, tlen);
  size_t i = 0;
  while (i < n) {
    const uint32_t sep = SeparatorAt(text, n, i);
    if (sep) {
      i += sep;
      continue;
    }
    const size_t ws = i;
    bool ascii = true;
    while (i < n && SeparatorAt(text, n, i) == 0) {
      ascii = ascii && text[i] < 0x80;
      ++i;
    }
    const size_t we = i;
    if (ascii) {  // the whole word (:254-266, :281-287)
      const uint32_t len = static_cast<uint32_t>(we - ws);
      const uint32_t diff = len > m ? len - m : m - len;
      if (diff <= static_cast<uint32_t>(D) && BandWithin<D>(text, ws, we, len, term, tlen, m, true)) return true;
    } else {  // code-point windows (:276-280)
      const uint32_t len = CountCps(text, ws, we);
      if (len == 0 || len + D < m) continue;  // (no window reaches max(1, m - D) code points)
      size_t p = ws;
      for (uint32_t s = 0; s < len; ++s) {
        if (BandWithin<D>(text, p, we, len - s, term, tlen, m, false)) return true;
        NextCp(text, we, p);
      }
    }
  }
  return false;
}

// d = 0..2 (the parser's FUZZY takes 1 or 2, query_parser_clauses.cpp:444-464): 1 / 0, or -1 for another d.
MGX_FZ_HD int ContainsFuzzyMatchD(const uint8_t* text, size_t n, const uint8_t* term, size_t tlen, uint32_t d) {
  switch (d) {
    case 0: return ContainsFuzzyMatch<0>(text, n, term, tlen) ? 1 : 0;
    case 1: return ContainsFuzzyMatch<1>(text, n, term, tlen) ? 1 : 0;
    case 2: return ContainsFuzzyMatch<2>(text, n, term, tlen) ? 1 : 0;
    default: return -1;
  }
}

}  // namespace mgx::fuzzy
