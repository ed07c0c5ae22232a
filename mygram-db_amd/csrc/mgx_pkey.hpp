// mgx_pkey.hpp — SORT by primary key (the reference's default order: ResultSorter::SortAndPaginate without an ORDER BY
// column, result_sorter.cpp:502-510; GetSortKey's primary-key branch, :239-262). One rule, stated once for host and
// device: how a primary key becomes a sort key, how an index stores it in 8 bytes per doc slot, and how two keys of
// (possibly) different indexes compare. The host part compiles without a HIP header (the stand-alone checks do).
//
//   numeric key  a non-empty string of ASCII digits that parses into a uint64_t: that number zero-padded to 20 characters
//   raw key      any other primary key, its bytes ("" and digit strings past 2^64 - 1 included)
//   no key       the doc id zero-padded to 20 characters
//   comparison   std::string::compare: unsigned bytes, a proper prefix first; ties go to the doc id in the sort's
//                direction ("007" and "7" share the key 00000000000000000007 and tie)
//
// An index stores one value per doc slot and a kind:
//   kKeyNumeric  every key of the index is a 20-digit form: the value is the number (unsigned order = key order)
//   kKeyRanks    the value is the rank of the doc's key among the index's distinct keys, sorted bytewise; the dictionary
//                (off[] + bytes, numeric keys in their 20-character form) travels with the column
#pragma once
#include <cstddef>
#include <cstdint>

#include "mgx_colsort.hpp"

#include <algorithm>
#include <string>
#include <vector>

namespace mgx {
namespace pkey {

constexpr uint32_t kKeyNumeric = 0, kKeyRanks = 1;
constexpr uint32_t kNumericWidth = 20;  // kNumericWidth of result_sorter.cpp: the digits of 2^64 - 1

// What a comparison needs of one index's keys.
struct KeySide {
  uint32_t kind;         // kKeyNumeric | kKeyRanks
  const uint64_t* off;   // kKeyRanks: [n_keys + 1] byte offsets of the sorted distinct keys
  const uint8_t* bytes;  // kKeyRanks: their bytes
};

MGX_CS_HD inline uint64_t Pow10(uint32_t e) {  // e <= 19
  uint64_t p = 1;
  for (uint32_t i = 0; i < e; ++i) p *= 10u;
  return p;
}
MGX_CS_HD inline uint32_t KeyLength(const KeySide& s, uint64_t v) {
  return s.kind == kKeyNumeric ? kNumericWidth : static_cast<uint32_t>(s.off[v + 1] - s.off[v]);
}
// Byte i (below KeyLength) of the key a stored value stands for.
MGX_CS_HD inline uint32_t KeyByte(const KeySide& s, uint64_t v, uint32_t i) {
  if (s.kind == kKeyNumeric) return '0' + static_cast<uint32_t>((v / Pow10(kNumericWidth - 1 - i)) % 10u);
  return s.bytes[s.off[v] + i];
}
// std::string::compare of the two keys: negative, 0 or positive.
MGX_CS_HD inline int CompareKeys(const KeySide& sa, uint64_t va, const KeySide& sb, uint64_t vb) {
  if (sa.kind == kKeyNumeric && sb.kind == kKeyNumeric) return va < vb ? -1 : va > vb ? 1 : 0;  // equal widths
  const uint32_t la = KeyLength(sa, va), lb = KeyLength(sb, vb);
  const uint32_t n = la < lb ? la : lb;
  for (uint32_t i = 0; i < n; ++i) {
    const uint32_t a = KeyByte(sa, va, i), b = KeyByte(sb, vb, i);
    if (a != b) return a < b ? -1 : 1;
  }
  return la < lb ? -1 : la > lb ? 1 : 0;
}
// The carried pairs of two runs (colsort::PairKey / PairDoc: complemented for ASC): does x come before y in the page?
// DESC: the larger key, then the larger doc id; ASC: the smaller key, then the smaller doc id (CompareDocIdTie, :43-54).
MGX_CS_HD inline bool PairBefore(const KeySide& sx, uint64_t kx, uint32_t dx, const KeySide& sy, uint64_t ky, uint32_t dy,
                                 bool descending) {
  const uint64_t vx = descending ? kx : ~kx, vy = descending ? ky : ~ky;
  const uint32_t ix = descending ? dx : ~dx, iy = descending ? dy : ~dy;
  const int c = CompareKeys(sx, vx, sy, vy);
  if (c != 0) return descending ? c > 0 : c < 0;
  return descending ? ix > iy : ix < iy;
}

// One query of the merge by key string (key_merge_kernel): DevMergeRun's fields, for runs of (value, docid') pairs.
struct KeyMergeRun {
  uint64_t a_off, b_off, out_off;
  uint32_t a_n, b_n, lo, hi;
  uint32_t descending, pad;
};

// ---- host only: derivation and the column of an index ----
struct SortKey {
  bool numeric = false;
  uint64_t value = 0;  // numeric
  std::string raw;     // not numeric
};
inline SortKey NumericKey(uint64_t v) {
  SortKey k;
  k.numeric = true;
  k.value = v;
  return k;
}
// GetSortKey's primary-key branch for a document that has a key (:247-256).
inline SortKey DeriveKey(const uint8_t* p, size_t n) {
  bool digits = n != 0;
  for (size_t i = 0; i < n && digits; ++i) digits = p[i] >= '0' && p[i] <= '9';  // std::isdigit on bytes, C locale
  if (digits) {
    uint64_t v = 0;
    bool fits = true;
    for (size_t i = 0; i < n && fits; ++i) {  // std::from_chars: result_out_of_range past 2^64 - 1
      const uint64_t d = p[i] - '0';
      fits = v <= (UINT64_MAX - d) / 10u;
      v = v * 10u + d;
    }
    if (fits) return NumericKey(v);
  }
  SortKey k;
  k.raw.assign(reinterpret_cast<const char*>(p), n);
  return k;
}
inline std::string KeyString(const SortKey& k) {
  if (!k.numeric) return k.raw;
  std::string s(kNumericWidth, '0');
  uint64_t v = k.value;
  for (uint32_t i = kNumericWidth; i-- > 0 && v != 0; v /= 10u) s[i] = static_cast<char>('0' + v % 10u);
  return s;
}

// The column of one index. doc_ids: the table id of every slot (the key of a document without one), or nullptr:
// first_doc_id + slot. has_key: nullptr = every document has one.
struct KeyColumn {
  uint32_t kind = kKeyNumeric;
  bool monotone = true;     // keys never decrease with the slot: key order is doc-id order, in both directions
  bool any_missing = false;  // some document fell back to its doc id
  std::vector<uint64_t> values;  // by slot
  std::vector<uint64_t> off;     // kKeyRanks
  std::vector<uint8_t> bytes;    // kKeyRanks
};
inline KeyColumn BuildKeyColumn(const uint8_t* bytes, const uint64_t* off, const uint8_t* has_key, uint64_t n,
                                const uint32_t* doc_ids, uint32_t first_doc_id) {
  KeyColumn c;
  std::vector<SortKey> keys(n);
  bool all_numeric = true;
  for (uint64_t i = 0; i < n; ++i) {
    if (has_key == nullptr || has_key[i]) {
      keys[i] = DeriveKey(bytes + off[i], static_cast<size_t>(off[i + 1] - off[i]));
    } else {
      keys[i] = NumericKey(doc_ids ? doc_ids[i] : first_doc_id + static_cast<uint32_t>(i));
      c.any_missing = true;
    }
    all_numeric = all_numeric && keys[i].numeric;
  }
  c.values.resize(n);
  if (all_numeric) {
    for (uint64_t i = 0; i < n; ++i) {
      c.values[i] = keys[i].value;
      if (i != 0 && c.values[i] < c.values[i - 1]) c.monotone = false;
    }
    return c;
  }
  c.kind = kKeyRanks;
  std::vector<std::string> strs(n);
  for (uint64_t i = 0; i < n; ++i) strs[i] = KeyString(keys[i]);
  std::vector<uint32_t> order(n);
  for (uint64_t i = 0; i < n; ++i) order[i] = static_cast<uint32_t>(i);
  // (std::string's operator< is compare() over unsigned bytes: char_traits<char>::lt)
  std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return strs[a] < strs[b]; });
  c.off.push_back(0);
  for (uint64_t j = 0; j < n; ++j) {
    const std::string& s = strs[order[j]];
    if (j == 0 || s != strs[order[j - 1]]) {
      c.bytes.insert(c.bytes.end(), s.begin(), s.end());
      c.off.push_back(c.bytes.size());
    }
    c.values[order[j]] = c.off.size() - 2;
  }
  for (uint64_t i = 1; i < n; ++i)
    if (c.values[i] < c.values[i - 1]) c.monotone = false;
  return c;
}

}  // namespace pkey
}  // namespace mgx

#if defined(__HIPCC__) || defined(MGX_COLSORT_LAUNCHERS)
namespace mgx {
// Every query's page from its two runs of (value, docid') pairs, merged by key string: run A's values belong to side a,
// run B's to side b. Writes ranks [lo, hi) of each run pair at out_docs / out_scores (0.0) + out_off.
int LaunchKeyMerge(const pkey::KeyMergeRun* runs, const uint64_t* run_start, uint32_t n_runs, uint64_t n_elems,
                   pkey::KeySide a, pkey::KeySide b, const uint64_t* keys, const uint32_t* dprime, uint32_t* out_docs,
                   double* out_scores, hipStream_t s);
}  // namespace mgx
#endif
