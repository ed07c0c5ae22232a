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

__global__ __launch_bounds__(kHlWaves * 64) void highlight_kernel(const DevHlBatch hb) {
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
    }
  }
  if (n == 0) {  // an empty text gives an empty snippet (highlighter.cpp:301-305)
    if (lane == 0) *g_head = hl::Header{0, 0, 0, 0};
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
  for (uint32_t base = 0; base < n && !bd.done; base += 64) {
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
      bd.Feed(ms, ms + b_cps, base + p, base + p + b_len, writer);
      if (bd.done) break;
    }
    cp_base += static_cast<uint32_t>(__popcll(lead));
    hl_wave_sync();  // (the writer's next_ok words, read by every lane in the next chunk)
  }
  const uint32_t total = bd.done ? hl::kNoTotal : cp_base;
  bd.Finish(total, writer);
  uint32_t flags = bd.flags;
  const uint32_t n_win = bd.n_win;
  if (writer) hl::FinalizeWindows(win, n_win, bd.matched, q.snippet_length, total, &flags);
  flags = static_cast<uint32_t>(__shfl(static_cast<int>(flags), 0));
  hl_wave_sync();  // (the windows, written by the writer)

  // ---- 3. window bounds: code points -> bytes (targets ascend: start0 <= end0 <= start1 ...) ----
  {
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
  uint32_t out = 0;
  for (uint32_t i = 0; i < n_win; ++i) {
    const uint32_t bs = win[i].start < n ? win[i].start : n;
    uint32_t be = win[i].end < n ? win[i].end : n;
    if (be < bs) be = bs;
    uint32_t len = be - bs;
    if (len > q.byte_cap - out) {
      len = q.byte_cap - out;
      flags |= hl::kFlagOverflow;
    }
    for (uint32_t o = lane; o < len; o += 64) g_bytes[out + o] = text[bs + o];
    if (writer) g_win[i] = hl::Window{bs, bs + len, win[i].span_end, out};
    out += len;
  }
  if (writer) *g_head = hl::Header{n_win, flags, bd.n_spans, out};
}

int LaunchHighlight(const DevHlBatch& hb, hipStream_t s) {
  if (hb.n_entries == 0) return 0;
  const uint32_t grid = (hb.n_entries + kHlWaves - 1) / kHlWaves;
  hipLaunchKernelGGL(highlight_kernel, dim3(grid), dim3(kHlWaves * 64), 0, s, hb);
  return static_cast<int>(hipGetLastError());
}

}  // namespace mgx
