// mgx_highlight.hip — HIGHLIGHT on the device: the snippet material of every (highlighted query, page entry) of a batch.
//
// One wave per entry, four waves per workgroup, no workgroup barrier (waves are independent and leave early). The wave
//   1. reads the entry's doc id from the batch's result block and finds the text (delta doc map first, else main slot);
//   2. walks the text in 64-byte chunks, one lane per byte position: per term a ballot of the positions the term matches
//      at, the leftmost non-overlapping choice on that wave-uniform mask (carried across chunks as the byte the term's
//      next match may start at, one LDS word per term), the longest term per position, and code-point positions from a
//      running popcount of lead bytes; the kept matches go, in ascending order, through mgx::highlight::Builder — the
//      window / merge / clamp rules the host build runs too (mgx_highlight.hpp). The walk stops once max_fragments
//      windows are closed;
//   3. walks the text once more up to the last window's end and turns the windows' code-point bounds into byte offsets
//      (the k-th lead byte of a chunk is one ballot);
//   4. copies the windows' bytes into the entry's record, lanes side by side, and writes the record's header and windows.
// Every store is a vector store of one lane. Reads of the text stay inside [0, n) of the document, writes inside the
// record's capacities (Header::flags says when a capacity cut the record short: never on valid UTF-8).
//
// highlight_original_kernel is the same wave program for a batch whose indexes carry original texts
// (mgx_index_attach_original_text; Highlighter::GenerateOriginal, highlighter.cpp:311-356). For an entry whose document
// has an original, step 2 still scans the NORMALIZED text, but every kept match is translated to code points of the
// original (TranslateMatch) and passes the pending-range filter (PendingRange) before Builder sees it, so the spans are
// code points too; step 3 walks the ORIGINAL and turns windows and spans into byte offsets in one pass; step 4 copies the
// original's bytes and sets kFlagOriginal. A document without an original takes the steps above unchanged. Reads of the
// original, its kind and its map stay inside what mgx_index_attach_original_text checked and uploaded.
#include <hip/hip_runtime.h>

#include "mgx_highlight.hpp"
#include "mgx_launch.hpp"

namespace mgx {

namespace hl = highlight;

constexpr int kHlWaves = 4;

// Hand-off of LDS words inside ONE wave (a lane's stores read by the other lanes): the wave's DS operations execute in
// order, so no wait is needed; the fence keeps the compiler from moving LDS accesses across the hand-off.
__device__ __forceinline__ void hl_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ unsigned long long hl_below(uint32_t p) {  // bits [0, p), p <= 64
  return p >= 64 ? ~0ull : ((1ull << p) - 1ull);
}

// The originals of the batch's two text sources (highlight_original_kernel only).
struct DevHlOriginals {
  hl::DevOriginals mapped, plain;
};

// Code points of text[0, n), counted by the wave; the walk stops once the count exceeds `stop_above`.
__device__ __forceinline__ uint32_t hl_count_cps(const uint8_t* text, uint32_t n, uint32_t stop_above, uint32_t lane) {
  uint32_t c = 0;
  for (uint32_t base = 0; base < n && c <= stop_above; base += 64) {
    const uint32_t pos = base + lane;
    c += static_cast<uint32_t>(__popcll(__ballot(pos < n && hl::IsLead(text[pos]))));
  }
  return c;
}

// One page entry, by one wave. kOrig = false is highlight_kernel as it always was; kOrig = true (an index of the batch
// carries originals) adds, for an entry whose document has one: the matches found in the normalized text are translated
// to code points of the original and pass the pending-range filter before Builder sees them, the windows AND the spans
// are turned into byte offsets by a walk over the ORIGINAL, and the record's bytes are the original's.
template <bool kOrig>
__device__ __forceinline__ void hl_entry(const DevHlBatch& hb, const DevHlOriginals* ho) {
  __shared__ hl::Window s_win[kHlWaves][hl::kMaxFragments];
  __shared__ uint32_t s_next[kHlWaves][kHlMaxTerms];
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint32_t entry = blockIdx.x * kHlWaves + wave;
  if (entry >= hb.n_entries) return;
  // the query whose entries hold this one: the last with entry_begin <= entry
  uint32_t lo = 0, hi = hb.n_queries;
  while (hi - lo > 1) {
    const uint32_t mid = (lo + hi) >> 1;
    if (hb.queries[mid].entry_begin <= entry) lo = mid;
    else hi = mid;
  }
  const DevHlQuery q = hb.queries[lo];
  const uint32_t j = entry - q.entry_begin;
  if (j >= q.limit) return;
  uint32_t count;
  if (q.page_n) {
    count = *q.page_n;
  } else {
    const unsigned long long total = hb.merged ? *q.total_merged : *q.total_exec;
    count = total < q.limit ? static_cast<uint32_t>(total) : q.limit;
  }
  if (j >= count) return;  // (the host reads the records of the page's entries only)
  const uint32_t doc = q.page_docs[j];

  uint8_t* rec = hb.arena + q.rec_off + static_cast<uint64_t>(j) * q.rec_stride;
  hl::Header* g_head = reinterpret_cast<hl::Header*>(rec);
  hl::Window* g_win = reinterpret_cast<hl::Window*>(rec + sizeof(hl::Header));
  hl::Span* g_spans = reinterpret_cast<hl::Span*>(rec + sizeof(hl::Header) + sizeof(hl::Window) * q.max_fragments);
  uint8_t* g_bytes = reinterpret_cast<uint8_t*>(g_spans) + sizeof(hl::Span) * q.span_cap;

  // ---- 1. the text ----
  const uint8_t* text = nullptr;
  uint32_t n = 0;
  const uint8_t* otext = nullptr;  // (kOrig) the original, its kind and its map
  uint32_t on = 0, kind = hl::kOrigNone, n_pairs = 0;
  const hl::MapPair* map = nullptr;
  {
    const uint8_t* src_text = nullptr;
    const uint64_t* src_off = nullptr;
    uint32_t slot = 0;
    if (hb.mapped.text && hb.mapped.doc_map) {
      uint32_t a = 0, b = hb.mapped.n_docs;  // first slot with doc_map[slot] >= doc
      while (a < b) {
        const uint32_t mid = (a + b) >> 1;
        if (hb.mapped.doc_map[mid] < doc) a = mid + 1;
        else b = mid;
      }
      if (a < hb.mapped.n_docs && hb.mapped.doc_map[a] == doc) {
        src_text = hb.mapped.text;
        src_off = hb.mapped.text_off;
        slot = a;
      }
    }
    if (!src_text && hb.plain.text && doc >= hb.plain.first_doc_id && doc - hb.plain.first_doc_id < hb.plain.n_docs) {
      src_text = hb.plain.text;
      src_off = hb.plain.text_off;
      slot = doc - hb.plain.first_doc_id;
    }
    if (src_text) {
      const uint64_t t0 = src_off[slot], t1 = src_off[slot + 1];
      const uint64_t len = t1 > t0 ? t1 - t0 : 0;
      n = len > 0x7FFFFF00ull ? 0x7FFFFF00u : static_cast<uint32_t>(len);
      text = src_text + t0;
      if constexpr (kOrig) {  // the document's original, in the index its text came from
        const hl::DevOriginals& o = src_text == hb.mapped.text ? ho->mapped : ho->plain;
        if (o.kind) kind = o.kind[slot];
        if (kind > hl::kOrigUnmappable) kind = hl::kOrigNone;
        if (kind != hl::kOrigNone) {
          const uint64_t o0 = o.off[slot], o1 = o.off[slot + 1];
          const uint64_t olen = o1 > o0 ? o1 - o0 : 0;
          on = olen > 0x7FFFFF00ull ? 0x7FFFFF00u : static_cast<uint32_t>(olen);
          otext = o.bytes + o0;
        }
        if (kind == hl::kOrigMapped) {
          const uint64_t m0 = o.map_off[slot], m1 = o.map_off[slot + 1];
          const uint64_t pairs = m1 > m0 ? m1 - m0 : 0;
          n_pairs = pairs > 0x7FFFFF00ull ? 0x7FFFFF00u : static_cast<uint32_t>(pairs);
          map = o.map + m0;
        }
      }
    }
  }
  const bool om = kOrig && kind != hl::kOrigNone;  // this entry is built from an original
  if (om ? on == 0 : n == 0) {  // an empty text gives an empty snippet (highlighter.cpp:301-305, :315-319)
    if (lane == 0) *g_head = hl::Header{0, om ? hl::kFlagOriginal : 0u, 0, 0};
    return;
  }

  // ---- 2. matches -> windows (code points) + spans (bytes) ----
  hl::Window* win = s_win[wave];
  uint32_t* next_ok = s_next[wave];
  const DevHlTerm* terms = hb.terms + q.term_begin;
  const uint32_t n_terms = q.n_terms < kHlMaxTerms ? q.n_terms : kHlMaxTerms;
  for (uint32_t t = lane; t < n_terms; t += 64) next_ok[t] = 0;
  hl_wave_sync();
  const bool writer = lane == 0;
  hl::Builder bd;
  bd.Init(q.snippet_length, q.max_fragments, win, g_spans, q.span_cap);
  const unsigned long long lt_mask = hl_below(lane);
  uint32_t cp_base = 0, last_end = 0;
  uint32_t n_scan = n;
  hl::PendingRange pr;
  pr.Init();
  if constexpr (kOrig) {  // an unmappable original, or no usable term: the no-match window (:323-325, :342-344)
    if (om && (kind == hl::kOrigUnmappable || n_terms == 0)) n_scan = 0;
  }
  for (uint32_t base = 0; base < n_scan && !bd.done; base += 64) {
    const uint32_t pos = base + lane;
    const bool inb = pos < n;
    const uint8_t c = inb ? text[pos] : static_cast<uint8_t>(0x80);
    const unsigned long long lead = __ballot(inb && hl::IsLead(c));
    uint32_t best = 0, best_len = 0;  // the longest term matching at this lane's byte: code points + 1, bytes
    for (uint32_t t = 0; t < n_terms; ++t) {
      const DevHlTerm tm = terms[t];
      if (tm.len > n) continue;  // (:260-262)
      uint32_t nxt = next_ok[t];
      if (nxt >= base + 64) continue;  // the term's last match covers the whole chunk
      const uint8_t* pat = hb.patterns + tm.off;
      bool ok = inb && pos >= nxt && n - pos >= tm.len && c == pat[0];
      if (ok) {
        for (uint32_t k = 1; k < tm.len; ++k)
          if (text[pos + k] != pat[k]) {
            ok = false;
            break;
          }
      }
      unsigned long long m = __ballot(ok);
      if (m == 0) continue;
      unsigned long long acc = 0;
      while (m) {  // leftmost, non-overlapping (:277-293)
        const uint32_t p = static_cast<uint32_t>(__builtin_ctzll(m));
        acc |= 1ull << p;
        nxt = base + p + tm.len;
        m &= ~hl_below(p + tm.len > 64 ? 64 : p + tm.len);
      }
      if (writer) next_ok[t] = nxt;
      if (((acc >> lane) & 1ull) && tm.cps + 1 > best) {
        best = tm.cps + 1;
        best_len = tm.len;
      }
    }
    unsigned long long any = __ballot(best != 0);
    while (any) {  // across terms, ascending starts: RemoveOverlappingMatchPositions (:227-248)
      const uint32_t p = static_cast<uint32_t>(__builtin_ctzll(any));
      any &= any - 1;
      const uint32_t ms = cp_base + static_cast<uint32_t>(__popcll(lead & hl_below(p)));
      const uint32_t b_cps = static_cast<uint32_t>(__shfl(static_cast<int>(best), static_cast<int>(p))) - 1;
      const uint32_t b_len = static_cast<uint32_t>(__shfl(static_cast<int>(best_len), static_cast<int>(p)));
      if (ms < last_end) continue;
      last_end = ms + b_cps;
      if constexpr (kOrig) {
        if (om) {  // (the spans are code points of the original until step 3 walks it)
          uint32_t xs, xe, os, oe;
          if (hl::TranslateMatch(kind, map, n_pairs, ms, ms + b_cps, &xs, &xe) && pr.Push(xs, xe, &os, &oe))
            bd.Feed(os, oe, os, oe, writer);
          if (bd.done) break;
          continue;
        }
      }
      bd.Feed(ms, ms + b_cps, base + p, base + p + b_len, writer);
      if (bd.done) break;
    }
    cp_base += static_cast<uint32_t>(__popcll(lead));
    hl_wave_sync();  // (the writer's next_ok words, read by every lane in the next chunk)
  }
  uint32_t total = bd.done ? hl::kNoTotal : cp_base;
  if constexpr (kOrig) {
    if (om && !bd.done) {
      uint32_t os, oe;
      if (pr.Flush(&os, &oe)) bd.Feed(os, oe, os, oe, writer);
      // the clamp and the trailing "..." need the ORIGINAL's code points: an identity document's are the normalized
      // text's; the no-match window only asks whether there are more than snippet_length
      if (bd.done) total = hl::kNoTotal;
      else if (n_scan == 0) total = hl_count_cps(otext, on, q.snippet_length, lane);
      else if (kind != hl::kOrigIdentity) total = hl_count_cps(otext, on, hl::kNoTotal, lane);
    }
  }
  bd.Finish(total, writer);
  uint32_t flags = bd.flags;
  const uint32_t n_win = bd.n_win;
  if (writer) hl::FinalizeWindows(win, n_win, bd.matched, q.snippet_length, total, &flags);
  flags = static_cast<uint32_t>(__shfl(static_cast<int>(flags), 0));
  hl_wave_sync();  // (the windows, written by the writer)

  // ---- 3. window bounds: code points -> bytes (targets ascend: start0 <= end0 <= start1 ...) ----
  if (om) {
    if constexpr (kOrig) {
      // over the ORIGINAL, and the spans with them: both ascend, so the next target is the smaller of the two heads. A
      // span bound behind the last window's end stops there (the renderer clips a span to its window). The spans are
      // in the record, written and read back by the writer lane alone.
      const uint32_t n_wt = 2 * n_win, n_st = 2 * bd.n_spans;
      const uint32_t last = n_win ? win[n_win - 1].end : 0;
      uint32_t wi = 0, si = 0, cps = 0;
      uint32_t sp_at = 0xFFFFFFFFu, sp_s = 0, sp_e = 0;  // the span whose bounds are in sp_s / sp_e
      for (uint32_t base = 0; wi < n_wt || si < n_st; base += 64) {
        if (base >= on) {  // at or past the end of the text
          for (; wi < n_wt; ++wi)
            if (writer) (wi & 1u ? win[wi >> 1].end : win[wi >> 1].start) = on;
          for (; si < n_st; ++si)
            if (writer) (si & 1u ? g_spans[si >> 1].end : g_spans[si >> 1].start) = on;
          break;
        }
        const uint32_t pos = base + lane;
        const bool is_lead = pos < on && hl::IsLead(otext[pos]);
        const unsigned long long lead = __ballot(is_lead);
        const uint32_t rank = static_cast<uint32_t>(__popcll(lead & lt_mask));
        const uint32_t cnt = static_cast<uint32_t>(__popcll(lead));
        while (wi < n_wt || si < n_st) {
          const bool hw = wi < n_wt, hs = si < n_st;
          const uint32_t tw = hw ? (wi & 1u ? win[wi >> 1].end : win[wi >> 1].start) : 0u;
          uint32_t ts = 0;
          if (hs) {
            if (sp_at != (si >> 1)) {
              sp_at = si >> 1;
              uint32_t a = 0, b = 0;
              if (writer) {
                a = g_spans[sp_at].start;
                b = g_spans[sp_at].end;
              }
              sp_s = static_cast<uint32_t>(__shfl(static_cast<int>(a), 0));
              sp_e = static_cast<uint32_t>(__shfl(static_cast<int>(b), 0));
            }
            ts = si & 1u ? sp_e : sp_s;
            if (ts > last) ts = last;
          }
          const bool take_span = hs && (!hw || ts <= tw);
          const uint32_t tc = take_span ? ts : tw;
          if (tc - cps >= cnt) break;  // (tc >= cps: targets ascend)
          const unsigned long long sel = __ballot(is_lead && rank == tc - cps);
          const uint32_t byte = base + static_cast<uint32_t>(__builtin_ctzll(sel));
          if (take_span) {
            if (writer) (si & 1u ? g_spans[si >> 1].end : g_spans[si >> 1].start) = byte;
            ++si;
          } else {
            if (writer) (wi & 1u ? win[wi >> 1].end : win[wi >> 1].start) = byte;
            ++wi;
            hl_wave_sync();
          }
        }
        cps += cnt;
      }
    }
  } else {
    uint32_t ti = 0;
    const uint32_t n_tgt = 2 * n_win;
    uint32_t cps = 0;
    for (uint32_t base = 0; ti < n_tgt; base += 64) {
      if (base >= n) {  // at or past the end of the text
        for (; ti < n_tgt; ++ti)
          if (writer) (ti & 1u ? win[ti >> 1].end : win[ti >> 1].start) = n;
        break;
      }
      const uint32_t pos = base + lane;
      const bool is_lead = pos < n && hl::IsLead(text[pos]);
      const unsigned long long lead = __ballot(is_lead);
      const uint32_t rank = static_cast<uint32_t>(__popcll(lead & lt_mask));
      const uint32_t cnt = static_cast<uint32_t>(__popcll(lead));
      while (ti < n_tgt) {
        const uint32_t tc = ti & 1u ? win[ti >> 1].end : win[ti >> 1].start;
        if (tc - cps >= cnt) break;  // (tc >= cps: targets ascend)
        const unsigned long long sel = __ballot(is_lead && rank == tc - cps);
        const uint32_t byte = base + static_cast<uint32_t>(__builtin_ctzll(sel));
        if (writer) (ti & 1u ? win[ti >> 1].end : win[ti >> 1].start) = byte;
        ++ti;
        hl_wave_sync();
      }
      cps += cnt;
    }
  }

  // ---- 4. the record ----
  hl_wave_sync();
  const uint8_t* src = om ? otext : text;  // the windows' bytes: the original's where there is one
  const uint32_t sn = om ? on : n;
  if (om) flags |= hl::kFlagOriginal;
  uint32_t out = 0;
  for (uint32_t i = 0; i < n_win; ++i) {
    const uint32_t bs = win[i].start < sn ? win[i].start : sn;
    uint32_t be = win[i].end < sn ? win[i].end : sn;
    if (be < bs) be = bs;
    uint32_t len = be - bs;
    if (len > q.byte_cap - out) {
      len = q.byte_cap - out;
      flags |= hl::kFlagOverflow;
    }
    for (uint32_t o = lane; o < len; o += 64) g_bytes[out + o] = src[bs + o];
    if (writer) g_win[i] = hl::Window{bs, bs + len, win[i].span_end, out};
    out += len;
  }
  if (writer) *g_head = hl::Header{n_win, flags, bd.n_spans, out};
}

__global__ __launch_bounds__(kHlWaves * 64) void highlight_kernel(const DevHlBatch hb) { hl_entry<false>(hb, nullptr); }

__global__ __launch_bounds__(kHlWaves * 64) void highlight_original_kernel(const DevHlBatch hb, const DevHlOriginals ho) {
  hl_entry<true>(hb, &ho);
}

int LaunchHighlight(const DevHlBatch& hb, hipStream_t s) {
  if (hb.n_entries == 0) return 0;
  const uint32_t grid = (hb.n_entries + kHlWaves - 1) / kHlWaves;
  hipLaunchKernelGGL(highlight_kernel, dim3(grid), dim3(kHlWaves * 64), 0, s, hb);
  return static_cast<int>(hipGetLastError());
}

int LaunchHighlightOriginal(const DevHlBatch& hb, const hl::DevOriginals& mapped, const hl::DevOriginals& plain,
                            hipStream_t s) {
  if (hb.n_entries == 0) return 0;
  const uint32_t grid = (hb.n_entries + kHlWaves - 1) / kHlWaves;
  hipLaunchKernelGGL(highlight_original_kernel, dim3(grid), dim3(kHlWaves * 64), 0, s, hb, DevHlOriginals{mapped, plain});
  return static_cast<int>(hipGetLastError());
}

}  // namespace mgx
