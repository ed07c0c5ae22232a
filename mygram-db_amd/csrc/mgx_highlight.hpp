// mgx_highlight.hpp — query::Highlighter::Generate (src/query/highlighter.cpp:114-309) over one normalized text: the
// window, merge, clamp and render rules, compiled ONCE for the host and the device. highlight_kernel (mgx_highlight.hip)
// feeds it the matches its wave scanner finds; mgx_tools.cpp (g++) feeds it the matches of the scalar scanner below and
// exports the result as mgxt_highlight_generate / mgxt_highlight_match_positions, the hooks the CPU differential test
// calls; mgx_highlight_render (mgx_api.cpp) renders a fetched record with Render(). Paths are relative to the reference tree.
//
// Contract: the text is normalizer output, so valid UTF-8. A code point is a byte that is not 10xxxxxx; code point c
// starts at the c-th such byte and reaches to the next one (or the end of the text). On other input every routine stays
// inside the text and inside the capacities it is given; what it then produces is unspecified.
//
// The rules, in the order a match stream meets them (matches arrive ascending and non-overlapping, which is what
// FindMatchPositions returns after RemoveOverlappingMatchPositions :227-248):
//   * a match [s, e) asks for the window [s - L/2 (or 0), min(total, e + L/2)) (GenerateWithPositions :174-180);
//   * a window that starts at or before the open window's end extends it, any other one closes it (MergeWindows
//     :115-131; the windows of ascending non-overlapping matches are already sorted);
//   * a closed window longer than L is cut by ClampWindows (:138-158) around its first match;
//   * only the first max_fragments windows are kept (:184-186), so the scan may stop once that many are closed;
//   * a match of a window is emitted clipped to it (:199-215). A match that starts L code points or more behind the
//     window's start cannot be inside the clamped window and is not recorded.
// The no-match path (:165-172) is one window [0, min(total, L)) without a leading "...".
#pragma once

#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#define MGX_HL_HD __host__ __device__ inline
#else
#define MGX_HL_HD inline
#endif

namespace mgx::highlight {

// the parser's ranges (query_parser_clauses.cpp:372-431, query_parser.h:276)
constexpr uint32_t kMaxSnippetLength = 10000;
constexpr uint32_t kMaxFragments = 100;
constexpr uint32_t kMaxTagBytes = 256;
constexpr uint32_t kDefaultSnippetLength = 100;  // query_parser.h:158-163
constexpr uint32_t kDefaultMaxFragments = 3;

constexpr uint32_t kFlagLeadingDots = 1u;   // "..." before the first window (:194-196)
constexpr uint32_t kFlagTrailingDots = 2u;  // "..." after the last one (:219-221)
constexpr uint32_t kFlagOverflow = 4u;      // the record's span or byte capacity was reached (never on valid UTF-8)
constexpr uint32_t kNoTotal = 0xFFFFFFFFu;  // the scan stopped before the end of the text: more text follows

// One kept window. While the windows are built, start / end are code points and `aux` is the window's anchor (its first
// match's start); a finished record holds byte offsets into the document and `aux` = where the window's bytes start in
// the record's byte area.
struct Window {
  uint32_t start, end;
  uint32_t span_end;  // spans [previous window's span_end, span_end) belong to this window
  uint32_t aux;
};
// One match inside a window, as byte offsets into the document (the renderer clips it to the window's bytes).
struct Span {
  uint32_t start, end;
};
struct Header {
  uint32_t n_windows, flags, n_spans, n_bytes;
};

MGX_HL_HD bool IsLead(uint8_t b) { return (b & 0xC0u) != 0x80u; }

MGX_HL_HD uint32_t CountCps(const uint8_t* t, size_t n) {
  uint32_t c = 0;
  for (size_t i = 0; i < n; ++i) c += IsLead(t[i]) ? 1u : 0u;
  return c;
}

// The match stream -> windows (code points) and spans. Every member is wave-uniform on the device; `writer` is false on
// the lanes that must not store.
struct Builder {
  uint32_t L, F, r;
  Window* win;
  Span* spans;
  uint32_t span_cap;
  uint32_t n_win, n_spans, flags;
  uint32_t ws, we, anchor;
  bool open, done, matched;

  MGX_HL_HD void Init(uint32_t snippet_length, uint32_t max_fragments, Window* w, Span* s, uint32_t s_cap) {
    L = snippet_length;
    F = max_fragments;
    r = snippet_length / 2;
    win = w;
    spans = s;
    span_cap = s_cap;
    n_win = n_spans = flags = 0;
    ws = we = anchor = 0;
    open = done = matched = false;
  }

  MGX_HL_HD void Close(bool writer) {
    if (writer) {
      win[n_win].start = ws;
      win[n_win].end = we;
      win[n_win].span_end = n_spans;
      win[n_win].aux = anchor;
    }
    ++n_win;
    open = false;
  }

  // One kept match: code points [ms, me), bytes [bs, be) of the document.
  MGX_HL_HD void Feed(uint32_t ms, uint32_t me, uint32_t bs, uint32_t be, bool writer) {
    if (done) return;
    const uint32_t win_s = ms > r ? ms - r : 0;
    const uint32_t win_e = me + r;  // (clipped to the text's code points in Finish)
    if (open && win_s <= we) {
      if (win_e > we) we = win_e;
    } else {
      if (open) {
        Close(writer);
        if (n_win == F) {  // the windows after this one are dropped (:184-186); this match proves there is more text
          done = true;
          return;
        }
      }
      open = true;
      ws = win_s;
      we = win_e;
      anchor = ms;
    }
    if (ms - ws >= L) return;  // behind the clamped window's end (ws + L at most)
    if (n_spans >= span_cap) {
      flags |= kFlagOverflow;
      return;
    }
    if (writer) {
      spans[n_spans].start = bs;
      spans[n_spans].end = be;
    }
    ++n_spans;
  }

  // End of the stream. total = the text's code points, or kNoTotal when the scan stopped early (`done`).
  MGX_HL_HD void Finish(uint32_t total, bool writer) {
    if (open) Close(writer);
    matched = n_win != 0;
    if (!matched) {  // the no-match path (:165-172)
      ws = 0;
      we = total < L ? total : L;
      anchor = 0;
      Close(writer);
      if (we < total) flags |= kFlagTrailingDots;
    }
  }
};

// The windows of a finished stream, still in code points: clip to the text, ClampWindows, the "..." flags. Run by ONE
// thread (after the writer's stores are visible to it).
MGX_HL_HD void FinalizeWindows(Window* win, uint32_t n_win, bool matched, uint32_t L, uint32_t total, uint32_t* flags) {
  if (!matched || n_win == 0) return;  // (the no-match window is final)
  for (uint32_t i = 0; i < n_win; ++i) {
    uint32_t win_start = win[i].start;
    uint32_t win_end = win[i].end < total ? win[i].end : total;
    if (win_end - win_start > L) {  // ClampWindows :141-157
      const uint32_t anchor = win[i].aux;
      const uint32_t left_context = L / 2;
      uint32_t clamped_start = anchor > left_context ? anchor - left_context : 0;
      if (total != kNoTotal && clamped_start + L > total) clamped_start = total > L ? total - L : 0;
      if (clamped_start > win_start) win_start = clamped_start;
      if (win_start + L < win_end) win_end = win_start + L;
    }
    win[i].start = win_start;
    win[i].end = win_end;
  }
  if (win[0].start > 0) *flags |= kFlagLeadingDots;
  if (win[n_win - 1].end < total) *flags |= kFlagTrailingDots;
}

// Byte offset of code point `cp` (CpToByte :78-93 on valid UTF-8): scalar form, continuing from (*byte, *seen) = a
// position at a code point's first byte and the code points before it. Targets must ascend between calls.
MGX_HL_HD uint32_t CpToByteFrom(const uint8_t* t, uint32_t n, uint32_t cp, uint32_t* byte, uint32_t* seen) {
  uint32_t i = *byte, c = *seen;
  while (i < n) {
    if (IsLead(t[i])) {
      if (c == cp) break;
      ++c;
    }
    ++i;
  }
  // (c counts the lead bytes before i; i == n: the target is at or past the end of the text)
  *byte = i;
  *seen = c;
  return i;
}

// ---- original texts: Highlighter::GenerateOriginal (:311-356) --------------------------------------------------------
// A document may carry the text the user wrote next to its normalized text. Matches are still found in the normalized
// text; each kept match [s, e) of normalized code points is translated to code points of the ORIGINAL through the map
// the host built per document (one (cp_start, cp_end) pair per normalized code point: the original segment the code
// point came from, :328-336), the translated ranges pass RemoveOverlappingMatchPositions once more (:355), and the
// windows, the clamp, the "..." and the bytes are all the original's.
//
// Contract (checked by mgx_index_attach_original_text): the original is valid UTF-8; an identity document has as many
// code points as its normalized text; a mapped document has one pair per normalized code point, start < end <= the
// original's code points, starts and ends non-decreasing. On other input every routine stays inside what it is given.
constexpr uint32_t kOrigNone = 0;        // no original: Generate over the normalized text
constexpr uint32_t kOrigIdentity = 1;    // normalized code point i <-> original code points [i, i + 1): no map stored
constexpr uint32_t kOrigMapped = 2;      // an explicit pair per normalized code point
constexpr uint32_t kOrigUnmappable = 3;  // :342-344: the no-match window over the original, whatever the terms
constexpr uint32_t kFlagOriginal = 8u;   // the record's windows, spans and bytes are the ORIGINAL text's

struct MapPair {
  uint32_t first, second;  // code points [first, second) of the original
};

// Where a device index keeps its originals (by doc slot; all null on an index without them).
struct DevOriginals {
  const uint8_t* bytes;
  const uint64_t* off;      // [n_docs + 1]
  const uint8_t* kind;      // [n_docs] kOrig*
  const MapPair* map;       // the kOrigMapped documents' pairs
  const uint64_t* map_off;  // [n_docs + 1], in pairs
};

// One kept match [s, e) of normalized code points -> code points of the original (:349-354). False: the match is
// dropped as the reference drops it (outside the map).
MGX_HL_HD bool TranslateMatch(uint32_t kind, const MapPair* map, uint32_t n_pairs, uint32_t s, uint32_t e, uint32_t* xs,
                              uint32_t* xe) {
  if (kind == kOrigIdentity) {
    *xs = s;
    *xe = e;
    return true;
  }
  if (s >= n_pairs || e == 0 || e > n_pairs) return false;
  *xs = map[s].first;
  *xe = map[e - 1].second;
  return true;
}

// RemoveOverlappingMatchPositions (:227-248) as a stream with one range of look-ahead. The translated ranges arrive with
// non-decreasing starts and non-decreasing ends (the segments are in text order), so the sort is the arrival order except
// inside a run of equal starts, where the longest is the last: a range that shares the held one's start replaces it, one
// that starts inside the held one is dropped, any other one releases it. Every member is wave-uniform on the device.
struct PendingRange {
  uint32_t s, e;
  bool held;

  MGX_HL_HD void Init() {
    s = e = 0;
    held = false;
  }
  // True: a range leaves the filter in (*os, *oe).
  MGX_HL_HD bool Push(uint32_t xs, uint32_t xe, uint32_t* os, uint32_t* oe) {
    if (!held) {
      held = true;
      s = xs;
      e = xe;
      return false;
    }
    if (xs == s) {  // the longest for a shared start (:232-237)
      if (xe > e) e = xe;
      return false;
    }
    if (xs < e) return false;  // starts inside the kept range (:242-244)
    *os = s;
    *oe = e;
    s = xs;
    e = xe;
    return true;
  }
  MGX_HL_HD bool Flush(uint32_t* os, uint32_t* oe) {
    if (!held) return false;
    held = false;
    *os = s;
    *oe = e;
    return true;
  }
};

// ---- host scanner + whole Generate (scalar) -------------------------------------------------------------------------

struct Term {
  const uint8_t* bytes;
  uint32_t len;
  uint32_t cps;  // CountCps(bytes, len)
};

// FindMatchPositions :252-297 as a stream: the next kept match at or after byte `from`. Per term the matches are
// leftmost and non-overlapping (next_ok[t] = the byte its next match may start at); across terms the one that starts
// first wins, the longest on a shared start, and a match that starts before the last kept end is dropped (:227-248).
// `cp_at` / `cp_seen` carry the code-point count up to the match (ascending). Returns false at the end of the text.
struct Scanner {
  const uint8_t* text;
  uint32_t n;
  const Term* terms;
  uint32_t n_terms;
  uint32_t* next_pos;  // [n_terms] start of the term's next match at or after its next_ok, or n when there is none
  uint32_t last_end_cp;
  uint32_t cp_byte, cp_seen;

  MGX_HL_HD static uint32_t Find(const uint8_t* t, uint32_t n, const Term& term, uint32_t from) {
    if (term.len == 0 || term.len > n) return n;
    for (uint32_t i = from; i + term.len <= n; ++i) {
      uint32_t k = 0;
      while (k < term.len && t[i + k] == term.bytes[k]) ++k;
      if (k == term.len) return i;
    }
    return n;
  }

  MGX_HL_HD void Init(const uint8_t* t, uint32_t len, const Term* tm, uint32_t nt, uint32_t* scratch) {
    text = t;
    n = len;
    terms = tm;
    n_terms = nt;
    next_pos = scratch;
    last_end_cp = 0;
    cp_byte = cp_seen = 0;
    for (uint32_t k = 0; k < nt; ++k) next_pos[k] = Find(t, len, tm[k], 0);
  }

  MGX_HL_HD bool Next(uint32_t* ms, uint32_t* me, uint32_t* bs, uint32_t* be) {
    for (;;) {
      uint32_t pos = n, best = 0, best_cps = 0;
      bool any = false;
      for (uint32_t k = 0; k < n_terms; ++k) {
        if (next_pos[k] >= n) continue;
        const uint32_t cps = terms[k].cps;
        if (!any || next_pos[k] < pos || (next_pos[k] == pos && cps > best_cps)) {
          any = true;
          pos = next_pos[k];
          best = k;
          best_cps = cps;
        }
      }
      if (!any) return false;
      // every term that matches here moves on past its own match (its matches do not depend on the other terms')
      for (uint32_t k = 0; k < n_terms; ++k)
        if (next_pos[k] == pos) next_pos[k] = Find(text, n, terms[k], pos + terms[k].len);
      // code points before `pos`
      while (cp_byte < pos) {
        cp_seen += IsLead(text[cp_byte]) ? 1u : 0u;
        ++cp_byte;
      }
      const uint32_t s = cp_seen;
      if (s < last_end_cp) continue;
      last_end_cp = s + best_cps;
      *ms = s;
      *me = s + best_cps;
      *bs = pos;
      *be = pos + terms[best].len;
      return true;
    }
  }
};

// Code-point windows -> byte windows, and where each window's bytes start in a record's byte area.
MGX_HL_HD uint32_t WindowsToBytes(const uint8_t* text, uint32_t n, Window* win, uint32_t n_win) {
  uint32_t byte = 0, seen = 0, out = 0;
  for (uint32_t i = 0; i < n_win; ++i) {
    const uint32_t b0 = CpToByteFrom(text, n, win[i].start, &byte, &seen);
    const uint32_t b1 = CpToByteFrom(text, n, win[i].end, &byte, &seen);
    win[i].start = b0;
    win[i].end = b1;
    win[i].aux = out;
    out += b1 - b0;
  }
  return out;
}

// The same for a record built from an original text, whose spans are code points too (the matches were translated, so
// their bytes are not known while they are found): windows and spans both ascend, one walk serves both. A span bound
// behind the last window's end stops there — the renderer clips a span to its window. Scalar form of the kernel's step.
MGX_HL_HD uint32_t OriginalToBytes(const uint8_t* text, uint32_t n, Window* win, uint32_t n_win, Span* spans,
                                   uint32_t n_spans) {
  const uint32_t last = n_win ? win[n_win - 1].end : 0;
  uint32_t byte = 0, seen = 0, wi = 0, si = 0;
  while (wi < 2 * n_win || si < 2 * n_spans) {
    uint32_t tw = 0, ts = 0;
    if (wi < 2 * n_win) tw = wi & 1u ? win[wi >> 1].end : win[wi >> 1].start;
    if (si < 2 * n_spans) {
      ts = si & 1u ? spans[si >> 1].end : spans[si >> 1].start;
      if (ts > last) ts = last;
    }
    if (si < 2 * n_spans && (wi >= 2 * n_win || ts <= tw)) {
      const uint32_t b = CpToByteFrom(text, n, ts, &byte, &seen);
      (si & 1u ? spans[si >> 1].end : spans[si >> 1].start) = b;
      ++si;
    } else {
      const uint32_t b = CpToByteFrom(text, n, tw, &byte, &seen);
      (wi & 1u ? win[wi >> 1].end : win[wi >> 1].start) = b;
      ++wi;
    }
  }
  uint32_t out = 0;
  for (uint32_t i = 0; i < n_win; ++i) {
    win[i].aux = out;
    out += win[i].end - win[i].start;
  }
  return out;
}

// PendingRange over a whole list (the test hook's form): writes the ranges that leave the filter, returns their number.
MGX_HL_HD size_t FilterRanges(const MapPair* in, size_t n, MapPair* out) {
  PendingRange pr;
  pr.Init();
  size_t m = 0;
  uint32_t os, oe;
  for (size_t i = 0; i < n; ++i)
    if (pr.Push(in[i].first, in[i].second, &os, &oe)) out[m++] = MapPair{os, oe};
  if (pr.Flush(&os, &oe)) out[m++] = MapPair{os, oe};
  return m;
}

// GenerateOriginal (:311-356) over one document, scalar: the record of a non-empty original of kind 1..3, windows and
// spans as byte offsets of the ORIGINAL. win[max_fragments], spans[span_cap], scratch[n_terms + 1] are the caller's.
MGX_HL_HD Header GenerateOriginalRecord(const uint8_t* original, uint32_t on, const uint8_t* normalized, uint32_t n,
                                        uint32_t kind, const MapPair* map, uint32_t n_pairs, const Term* terms,
                                        uint32_t n_terms, uint32_t snippet_length, uint32_t max_fragments, Window* win,
                                        Span* spans, uint32_t span_cap, uint32_t* scratch) {
  Builder bd;
  bd.Init(snippet_length, max_fragments, win, spans, span_cap);
  if (kind != kOrigUnmappable && n_terms != 0) {  // (:323-325, :342-344: else the no-match window)
    Scanner sc;
    sc.Init(normalized, n, terms, n_terms, scratch);
    PendingRange pr;
    pr.Init();
    uint32_t ms, me, bs, be, xs, xe, os, oe;
    while (!bd.done && sc.Next(&ms, &me, &bs, &be))
      if (TranslateMatch(kind, map, n_pairs, ms, me, &xs, &xe) && pr.Push(xs, xe, &os, &oe)) bd.Feed(os, oe, os, oe, true);
    if (!bd.done && pr.Flush(&os, &oe)) bd.Feed(os, oe, os, oe, true);
  }
  const uint32_t total = bd.done ? kNoTotal : CountCps(original, on);
  bd.Finish(total, true);
  FinalizeWindows(win, bd.n_win, bd.matched, snippet_length, total, &bd.flags);
  Header h{bd.n_win, bd.flags | kFlagOriginal, bd.n_spans, 0};
  h.n_bytes = OriginalToBytes(original, on, win, bd.n_win, spans, bd.n_spans);
  return h;
}

// GenerateWithPositions' rendering loop (:188-222) over a finished record. `bytes`: the windows' text; window i's
// byte b of the document is bytes[win[i].aux + (b - win[i].start)] — pass the document itself and doc_relative = true
// to read window i at bytes[b]. Writes at most `cap` bytes and returns the length the snippet has.
MGX_HL_HD size_t Render(const Header& h, const Window* win, const Span* spans, const uint8_t* bytes, bool doc_relative,
                        const uint8_t* open_tag, size_t open_len, const uint8_t* close_tag, size_t close_len,
                        uint8_t* out, size_t cap) {
  size_t n = 0;
  auto put = [&](const uint8_t* p, size_t len) {
    for (size_t i = 0; i < len; ++i, ++n)
      if (n < cap) out[n] = p[i];
  };
  const uint8_t dots[3] = {'.', '.', '.'};
  uint32_t sp = 0;
  for (uint32_t wi = 0; wi < h.n_windows; ++wi) {
    const Window& w = win[wi];
    if (wi > 0) put(dots, 3);
    if (wi == 0 && (h.flags & kFlagLeadingDots)) put(dots, 3);
    // byte b of the document, b in [w.start, w.end), is bytes[at(b)]
    const auto at = [&](uint32_t b) -> size_t { return doc_relative ? b : static_cast<size_t>(w.aux) + (b - w.start); };
    uint32_t cursor = w.start;
    const uint32_t sp_end = w.span_end < h.n_spans ? w.span_end : h.n_spans;
    for (; sp < sp_end; ++sp) {
      uint32_t s = spans[sp].start, e = spans[sp].end;
      if (e <= w.start || s >= w.end) continue;
      if (s < cursor) s = cursor;  // (a record's spans ascend; this keeps the bytes read ascending on any input)
      if (e > w.end) e = w.end;
      if (s >= e) continue;
      put(bytes + at(cursor), s - cursor);
      put(open_tag, open_len);
      put(bytes + at(s), e - s);
      put(close_tag, close_len);
      cursor = e;
    }
    sp = sp_end;
    if (cursor < w.end) put(bytes + at(cursor), w.end - cursor);
    if (wi + 1 == h.n_windows && (h.flags & kFlagTrailingDots)) put(dots, 3);
  }
  return n;
}

}  // namespace mgx::highlight
