// mgx_build.hip — the device column builder: normalized texts -> gram dictionary, CSR postings, tf, doc_len, equal to
// what mgx_columns.cpp builds on the host.
//
// The work is mapped to BYTES of the text, not to documents. A byte starts a code point exactly when it is no
// continuation byte and TryParseUtf8Char accepts the sequence that begins there inside its own document: the sequential
// decode (text::Decode) steps over continuation bytes only inside an accepted sequence, so it reaches every other byte.
// Every lane therefore decodes its own 16 bytes without looking at what came before, one long document spreads over
// as many lanes as its bytes need, and no lane waits for a neighbour's document.
//
//   1  gram_decode_count_kernel   16 bytes per lane: which bytes start a code point (a 16-bit mask per lane), per-block count
//   2  exclusive scan of the block counts (rocprim)                              -> N code points
//   3  gram_decode_emit_kernel    the lanes' masks -> positions; decodes again and writes cps[q], cp_doc[q]
//   4  gram_docs_kernel           one lane per document: its first code point, doc_len
//   5  gram_windows_kernel        one lane per code point: the window that starts there -> record (key, slot << 32 | p)
//   6  one stable radix sort of the records by key (rocprim): equal keys stay in (doc, p) order
//   7  gram_heads_kernel          heads of (key, doc) runs and of keys, as two counters in one u64; exclusive scan
//   8  gram_tf_kernel             one lane per run: left-greedy tf, docids / tf / overflow; one lane per key: offsets, keys
// The texts are read twice (1 and 3, 16-byte loads); the second read of a delta-sized text comes from the L2.
//
// Two endings. mgx_columns_build_device copies every column down into host arrays. mgx_index_build_device (the resident
// ending) copies down what a host caller reads (keys, offsets, doc_len, overflow entries, counters) and leaves docids, tf,
// doc_len and the texts on the device, copied device to device into exactly sized allocations the index adopts:
//   9  resident_rows_kernel       four doc slots per lane: the tile-padded dl8 row, the text offsets rebased to 0
#include <hip/hip_runtime.h>

#include <algorithm>
#include <mutex>
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#include "mgx_build.hpp"
#include "mgx_internal.hpp"
#include "mgx_text.hpp"

namespace mgx {
namespace build {

namespace {

// The code points that start in lane t's 16 bytes: emit(cp, doc slot) in text order; returns the mask of their bytes.
// `text` is the build's own padded copy: the 20 bytes loaded lie inside it. What ParseUtf8 may USE is bounded by the
// end of the byte's own document (`avail`), never by the next document's bytes.
template <class Emit>
__device__ inline uint32_t DecodeLane(const uint8_t* __restrict__ text, const uint64_t* __restrict__ off, uint64_t base,
                                      uint64_t n_docs, uint64_t n_bytes, uint64_t t, Emit&& emit) {
  const uint64_t i0 = t * kLaneBytes;
  if (i0 >= n_bytes) return 0;
  const uint4 v = *reinterpret_cast<const uint4*>(text + i0);
  const uint32_t wd[5] = {v.x, v.y, v.z, v.w, *reinterpret_cast<const uint32_t*>(text + i0 + kLaneBytes)};
  // the document of byte i0: the last d with off[d] <= i0 (documents without bytes are stepped over)
  uint64_t lo = 0, hi = n_docs;
  while (hi - lo > 1) {
    const uint64_t mid = (lo + hi) >> 1;
    if (off[mid] - base <= i0) lo = mid; else hi = mid;
  }
  uint64_t d = lo, end = off[d + 1] - base;
  uint32_t mask = 0;
#pragma unroll
  for (int j = 0; j < static_cast<int>(kLaneBytes); ++j) {
    const uint64_t i = i0 + j;
    if (i >= n_bytes) break;
    while (i >= end) {  // (i < n_bytes = off[n_docs] - base: d + 1 stays <= n_docs)
      ++d;
      end = off[d + 1] - base;
    }
    const int sh = 8 * (j & 3);
    const uint32_t w4 = sh ? (wd[j >> 2] >> sh) | (wd[(j >> 2) + 1] << (32 - sh)) : wd[j >> 2];
    const uint8_t b[4] = {static_cast<uint8_t>(w4), static_cast<uint8_t>(w4 >> 8), static_cast<uint8_t>(w4 >> 16),
                          static_cast<uint8_t>(w4 >> 24)};
    if ((b[0] & 0xC0) == 0x80) continue;
    uint32_t cp = 0;
    if (text::ParseUtf8(b, static_cast<size_t>(end - i), &cp) > 0) {
      mask |= 1u << j;
      emit(cp, static_cast<uint32_t>(d));
    }
  }
  return mask;
}

// inclusive scan of one value per thread over the block
__device__ inline uint32_t BlockInclusiveScan(uint32_t v, uint32_t* s) {
  const uint32_t tid = threadIdx.x;
  s[tid] = v;
  __syncthreads();
  for (uint32_t o = 1; o < kBlockThreads; o <<= 1) {
    const uint32_t add = tid >= o ? s[tid - o] : 0;
    __syncthreads();
    s[tid] += add;
    __syncthreads();
  }
  return s[tid];
}

__global__ __launch_bounds__(kBlockThreads) void gram_decode_count_kernel(
    const uint8_t* __restrict__ text, const uint64_t* __restrict__ off, uint64_t base, uint64_t n_docs, uint64_t n_bytes,
    uint16_t* __restrict__ lane_mask, uint32_t* __restrict__ block_count) {
  __shared__ uint32_t s[kBlockThreads];
  const uint64_t t = static_cast<uint64_t>(blockIdx.x) * kBlockThreads + threadIdx.x;
  const uint32_t mask = DecodeLane(text, off, base, n_docs, n_bytes, t, [](uint32_t, uint32_t) {});
  lane_mask[t] = static_cast<uint16_t>(mask);
  const uint32_t incl = BlockInclusiveScan(static_cast<uint32_t>(__popc(mask)), s);
  if (threadIdx.x == kBlockThreads - 1) block_count[blockIdx.x] = incl;
}

__global__ __launch_bounds__(kBlockThreads) void gram_decode_emit_kernel(
    const uint8_t* __restrict__ text, const uint64_t* __restrict__ off, uint64_t base, uint64_t n_docs, uint64_t n_bytes,
    const uint16_t* __restrict__ lane_mask, const uint32_t* __restrict__ block_base, uint32_t* __restrict__ lane_prefix,
    uint32_t* __restrict__ cps, uint32_t* __restrict__ cp_doc, uint32_t n_cps) {
  __shared__ uint32_t s[kBlockThreads];
  const uint64_t t = static_cast<uint64_t>(blockIdx.x) * kBlockThreads + threadIdx.x;
  const uint32_t cnt = static_cast<uint32_t>(__popc(static_cast<uint32_t>(lane_mask[t])));
  const uint32_t incl = BlockInclusiveScan(cnt, s);
  uint32_t q = block_base[blockIdx.x] + incl - cnt;
  lane_prefix[t] = q;
  const uint32_t q_end = q + cnt;
  DecodeLane(text, off, base, n_docs, n_bytes, t, [&](uint32_t cp, uint32_t d) {
    if (q < q_end && q < n_cps) {  // (what the count pass found; the bound keeps a store inside the arrays whatever happens)
      cps[q] = cp;
      cp_doc[q] = d;
    }
    ++q;
  });
}

// the code points in front of byte `o` of the text
__device__ inline uint32_t CodePointsBefore(uint64_t o, uint64_t n_bytes, uint32_t n_cps, const uint16_t* lane_mask,
                                            const uint32_t* lane_prefix) {
  if (o >= n_bytes) return n_cps;
  const uint64_t t = o / kLaneBytes;
  const uint32_t below = (1u << (o % kLaneBytes)) - 1u;
  return lane_prefix[t] + static_cast<uint32_t>(__popc(static_cast<uint32_t>(lane_mask[t]) & below));
}

__global__ __launch_bounds__(kBlockThreads) void gram_docs_kernel(
    const uint64_t* __restrict__ off, uint64_t base, uint64_t n_docs, uint64_t n_bytes, uint32_t n_cps,
    const uint16_t* __restrict__ lane_mask, const uint32_t* __restrict__ lane_prefix, uint32_t* __restrict__ doc_cp_off,
    uint32_t* __restrict__ doc_len) {
  const uint64_t d = static_cast<uint64_t>(blockIdx.x) * kBlockThreads + threadIdx.x;
  if (d > n_docs) return;
  const uint32_t a = CodePointsBefore(off[d] - base, n_bytes, n_cps, lane_mask, lane_prefix);
  doc_cp_off[d] = a;
  if (d < n_docs) doc_len[d] = CodePointsBefore(off[d + 1] - base, n_bytes, n_cps, lane_mask, lane_prefix) - a;
}

__global__ __launch_bounds__(kBlockThreads) void gram_windows_kernel(
    const uint32_t* __restrict__ cps, const uint32_t* __restrict__ cp_doc, const uint32_t* __restrict__ doc_cp_off,
    uint32_t n_cps, int ascii_n, int kanji_n, int cross, uint64_t* __restrict__ keys, uint64_t* __restrict__ vals) {
  const uint64_t q = static_cast<uint64_t>(blockIdx.x) * kBlockThreads + threadIdx.x;
  if (q >= n_cps) return;
  const uint32_t d = cp_doc[q];
  const uint32_t begin = doc_cp_off[d], doc_end = doc_cp_off[d + 1];
  const uint32_t end = doc_end < n_cps ? doc_end : n_cps;
  // code points from q to the document's end: >= 1 (the clamps keep the loads below inside cps[0, n_cps) whatever happens)
  const uint32_t left = end > q ? end - static_cast<uint32_t>(q) : 1u;
  const uint32_t c[kMaxGram] = {cps[q], left > 1 ? cps[q + 1] : 0u, left > 2 ? cps[q + 2] : 0u};
  const int w = (ascii_n > 0 && kanji_n > 0)
                    ? text::WindowAt(c, left < static_cast<uint32_t>(kMaxGram) ? left : kMaxGram, 0, ascii_n, kanji_n, cross != 0)
                    : 0;
  keys[q] = w > 0 ? PackKey(c, w) : kNoWindow;
  vals[q] = (static_cast<uint64_t>(d) << 32) | (static_cast<uint32_t>(q) - begin);
}

// flags[i]: low word 1 = record i opens a (key, doc) run, high word 1 = it opens a key; flags[n] = 0 closes the scan
__global__ __launch_bounds__(kBlockThreads) void gram_heads_kernel(const uint64_t* __restrict__ keys,
                                                                   const uint64_t* __restrict__ vals, uint32_t n,
                                                                   uint64_t* __restrict__ flags) {
  const uint64_t i = static_cast<uint64_t>(blockIdx.x) * kBlockThreads + threadIdx.x;
  if (i > n) return;
  uint64_t f = 0;
  if (i < n) {
    const uint64_t k = keys[i];
    if (k != kNoWindow) {
      const bool key_head = i == 0 || keys[i - 1] != k;
      const bool run_head = key_head || (vals[i - 1] >> 32) != (vals[i] >> 32);
      f = (run_head ? 1ull : 0ull) | (key_head ? 1ull << 32 : 0ull);
    }
  }
  flags[i] = f;
}

__global__ __launch_bounds__(kBlockThreads) void gram_tf_kernel(
    const uint64_t* __restrict__ keys, const uint64_t* __restrict__ vals, const uint64_t* __restrict__ flags,
    const uint64_t* __restrict__ scan, uint32_t n, uint32_t first_doc_id, uint32_t* __restrict__ docids,
    uint8_t* __restrict__ tf, uint64_t* __restrict__ gram_keys, uint64_t* __restrict__ gram_off,
    uint64_t* __restrict__ overflow, uint32_t overflow_cap, uint32_t* __restrict__ n_overflow) {
  const uint64_t i = static_cast<uint64_t>(blockIdx.x) * kBlockThreads + threadIdx.x;
  if (i >= n) return;
  const uint64_t f = flags[i];
  if (!(f & 1ull)) return;
  const uint64_t k = keys[i], sc = scan[i];
  const uint32_t pos = static_cast<uint32_t>(sc), slot = static_cast<uint32_t>(vals[i] >> 32);
  // BM25Scorer::CountTermOccurrences over this gram's window positions of this document: left-greedy, non-overlapping
  const uint64_t w = static_cast<uint64_t>(KeyWidth(k));
  uint32_t count = 0;
  uint64_t next_ok = 0;
  for (uint64_t j = i; j < n; ++j) {
    const uint64_t v = vals[j];
    if (keys[j] != k || static_cast<uint32_t>(v >> 32) != slot) break;
    const uint64_t p = v & 0xFFFFFFFFull;
    if (p >= next_ok) {
      ++count;
      next_ok = p + w;
    }
  }
  docids[pos] = first_doc_id + slot;
  tf[pos] = static_cast<uint8_t>(count >= 255u ? 255u : count);
  if (count >= 255u) {
    const uint32_t at = atomicAdd(n_overflow, 1u);
    if (at < overflow_cap) overflow[at] = (static_cast<uint64_t>(pos) << 32) | count;
  }
  if (f >> 32) {
    const uint32_t g = static_cast<uint32_t>(sc >> 32);
    gram_keys[g] = k;
    gram_off[g] = pos;
  }
}

// The two rows an index derives from the build's doc_len and text offsets (the resident ending): dl8[slot] =
// min(doc_len[slot], 255) with zeros from n_docs up to the tile boundary, and text_off[d] = off[d] - base. A lane takes
// kResidentSlotsPerLane consecutive slots: one 16-byte load of doc_len, one 4-byte store of the packed bytes; a wave
// reads 1 KiB and writes 256 bytes in a row. dl8_slots is a multiple of the slots per lane, doc_len is 16-byte aligned
// and its allocation is rounded up to 256 bytes, so the full-width load of a lane below n_docs lies inside it.
static_assert(kResidentSlotsPerLane == 4 && kResidentTileDocs % kResidentSlotsPerLane == 0, "one u32 store per lane");
__global__ __launch_bounds__(kBlockThreads) void resident_rows_kernel(
    const uint32_t* __restrict__ doc_len, const uint64_t* __restrict__ off, uint64_t base, uint64_t n_docs, uint64_t dl8_slots,
    uint8_t* __restrict__ dl8, uint64_t* __restrict__ text_off) {
  const uint64_t s0 = (static_cast<uint64_t>(blockIdx.x) * kBlockThreads + threadIdx.x) * kResidentSlotsPerLane;
  if (s0 < dl8_slots) {
    uint32_t len[kResidentSlotsPerLane] = {0, 0, 0, 0};
    if (s0 + kResidentSlotsPerLane <= n_docs) {
      const uint4 v = *reinterpret_cast<const uint4*>(doc_len + s0);
      len[0] = v.x, len[1] = v.y, len[2] = v.z, len[3] = v.w;
    } else {
#pragma unroll
      for (uint32_t j = 0; j < kResidentSlotsPerLane; ++j)
        if (s0 + j < n_docs) len[j] = doc_len[s0 + j];
    }
    uint32_t packed = 0;
#pragma unroll
    for (uint32_t j = 0; j < kResidentSlotsPerLane; ++j) packed |= (len[j] < 255u ? len[j] : 255u) << (8 * j);
    *reinterpret_cast<uint32_t*>(dl8 + s0) = packed;
  }
  if (text_off) {
#pragma unroll
    for (uint32_t j = 0; j < kResidentSlotsPerLane; ++j)
      if (s0 + j <= n_docs) text_off[s0 + j] = off[s0 + j] - base;
  }
}

// The device allocation of a finished build is kept for the next one when it is small, so that the delta rebuilds of a
// writer do not pay an allocation each; kept allocations are leased, concurrent callers get their own. The STREAM is made
// for the call and destroyed with it: a stream that stays alive holds a hardware queue, and the streams of every device
// index created later (a delta, a compacted main index) would be spread over the queues differently than without it.
struct Slot {
  int device = -1;
  void* arena = nullptr;
  uint64_t arena_bytes = 0;
};
constexpr uint64_t kKeepArena = 1ull << 30;
constexpr size_t kKeepSlots = 4;
std::mutex g_slots_mu;
std::vector<Slot> g_slots;

struct Lease {
  Slot s;
  hipStream_t stream = nullptr;
  bool ok = false;
  explicit Lease(int device) {
    s.device = device;
    ok = hipStreamCreateWithFlags(&stream, hipStreamNonBlocking) == hipSuccess;
    if (!ok) {
      (void)hipGetLastError();
      return;
    }
    std::lock_guard<std::mutex> lk(g_slots_mu);
    for (size_t i = 0; i < g_slots.size(); ++i)
      if (g_slots[i].device == device) {
        s = g_slots[i];
        g_slots.erase(g_slots.begin() + static_cast<long>(i));
        return;
      }
  }
  void DropArena() {
    if (s.arena) (void)hipFree(s.arena);
    s.arena = nullptr;
    s.arena_bytes = 0;
  }
  ~Lease() {
    if (!ok) return;
    (void)hipStreamSynchronize(stream);
    (void)hipStreamDestroy(stream);
    if (s.arena_bytes > kKeepArena) DropArena();
    if (s.arena) {
      std::lock_guard<std::mutex> lk(g_slots_mu);
      if (g_slots.size() < kKeepSlots) {
        g_slots.push_back(s);
        return;
      }
    }
    DropArena();
  }
  Lease(const Lease&) = delete;
  Lease& operator=(const Lease&) = delete;
};

inline unsigned Blocks(uint64_t n) { return static_cast<unsigned>((n + kBlockThreads - 1) / kBlockThreads); }

// The resident ending: exactly sized allocations of the index's own, filled device to device on the build's stream, which
// is synchronised before this returns (the arena may go to another thread right after). Null sources stand for a build
// without text bytes: no postings, every length and offset 0. *no_room: an allocation failed for lack of memory.
hipError_t FillResident(hipStream_t st, uint64_t n_postings, uint64_t n_docs, uint64_t n_bytes, uint64_t base,
                        const uint32_t* s_docids, const uint8_t* s_tf, const uint32_t* s_doc_len, const uint8_t* s_text,
                        const uint64_t* s_off, bool attach_text, ResidentArrays* r, bool* no_room) {
  const ResidentPlan pl = PlanResident(n_docs, n_postings, n_bytes, attach_text);
  r->plan = pl;
  *no_room = false;
#define MGX_RES_TRY(expr)                  \
  do {                                     \
    const hipError_t e__ = (expr);         \
    if (e__ != hipSuccess) return e__;     \
  } while (0)
  auto alloc = [&](void** p, uint64_t bytes) {
    const hipError_t e = hipMalloc(p, bytes ? bytes : 16);
    if (e != hipSuccess) {
      *p = nullptr;
      *no_room = e == hipErrorOutOfMemory;
    }
    return e;
  };
  MGX_RES_TRY(alloc(&r->docids, pl.docids));
  MGX_RES_TRY(alloc(&r->tf, pl.tf));
  MGX_RES_TRY(alloc(&r->doc_len, pl.doc_len));
  MGX_RES_TRY(alloc(&r->dl8, pl.dl8));
  if (attach_text) {
    MGX_RES_TRY(alloc(&r->text, pl.text));
    MGX_RES_TRY(alloc(&r->text_off, pl.text_off));
  }
  uint8_t* docids = static_cast<uint8_t*>(r->docids);
  uint8_t* tf = static_cast<uint8_t*>(r->tf);
  uint8_t* dl8 = static_cast<uint8_t*>(r->dl8);
  if (n_postings) MGX_RES_TRY(hipMemcpyAsync(docids, s_docids, n_postings * 4, hipMemcpyDeviceToDevice, st));
  MGX_RES_TRY(hipMemsetAsync(docids + n_postings * 4, 0xFF, kResidentIdPad * 4, st));
  if (n_postings) MGX_RES_TRY(hipMemcpyAsync(tf, s_tf, n_postings, hipMemcpyDeviceToDevice, st));
  MGX_RES_TRY(hipMemsetAsync(tf + n_postings, 0xFF, kResidentIdPad, st));
  MGX_RES_TRY(hipMemsetAsync(dl8 + pl.dl8_slots, 0xFF, kResidentDl8Pad, st));
  if (attach_text) {
    uint8_t* text = static_cast<uint8_t*>(r->text);
    if (n_bytes) MGX_RES_TRY(hipMemcpyAsync(text, s_text, n_bytes, hipMemcpyDeviceToDevice, st));
    MGX_RES_TRY(hipMemsetAsync(text + n_bytes, 0xFF, kResidentTextPad, st));
  }
  if (s_doc_len) {
    MGX_RES_TRY(hipMemcpyAsync(r->doc_len, s_doc_len, n_docs * 4, hipMemcpyDeviceToDevice, st));
    resident_rows_kernel<<<Blocks(pl.lanes), kBlockThreads, 0, st>>>(s_doc_len, s_off, base, n_docs, pl.dl8_slots, dl8,
                                                                     static_cast<uint64_t*>(r->text_off));
    MGX_RES_TRY(hipGetLastError());
  } else {
    MGX_RES_TRY(hipMemsetAsync(r->doc_len, 0, n_docs * 4, st));
    MGX_RES_TRY(hipMemsetAsync(dl8, 0, pl.dl8_slots, st));
    if (attach_text) MGX_RES_TRY(hipMemsetAsync(r->text_off, 0, pl.text_off, st));
  }
  return hipStreamSynchronize(st);
#undef MGX_RES_TRY
}

}  // namespace

static_assert(kResidentTileDocs == mgx::kTileDocs, "dl8 is padded to the index's tiles");

void ResidentArrays::Free() {
  for (void** p : {&docids, &tf, &doc_len, &dl8, &text, &text_off}) {
    if (*p) (void)hipFree(*p);
    *p = nullptr;
  }
}

int BuildOnDevice(const mgx_build_params& bp, const uint8_t* text_bytes, const uint64_t* text_off, uint32_t first_doc_id,
                  uint64_t n_docs, int device, PackedColumns* out, std::string* err, ResidentArrays* resident,
                  bool attach_text) {
  hipStream_t st = nullptr;
  const std::string who = resident ? "mgx_index_build_device: " : "mgx_columns_build_device: ";
  auto hip_fail = [&](const char* what, hipError_t e) {
    (void)hipGetLastError();
    if (st) (void)hipStreamSynchronize(st);  // (no copy into *out is in flight when the caller gets it back)
    if (resident) resident->Free();
    *err = who + what + ": " + hipGetErrorString(e);
    return MGX_ERR_INTERNAL;
  };
  // the resident ending over the build's arrays (all null: a build without text bytes)
  auto fill_resident = [&](uint64_t n_postings, uint64_t n_bytes, uint64_t base, const uint32_t* s_docids, const uint8_t* s_tf,
                           const uint32_t* s_doc_len, const uint8_t* s_text, const uint64_t* s_off) {
    bool no_room = false;
    const hipError_t e = FillResident(st, n_postings, n_docs, n_bytes, base, s_docids, s_tf, s_doc_len, s_text, s_off,
                                      attach_text, resident, &no_room);
    if (e == hipSuccess) return static_cast<int>(MGX_OK);
    if (!no_room) return hip_fail("the index's arrays", e);
    (void)hipGetLastError();
    (void)hipStreamSynchronize(st);
    const uint64_t needed = resident->plan.total();
    resident->Free();
    *err = who + "the index's arrays need " + std::to_string(needed) + " bytes of device memory and device " +
           std::to_string(device) + " has no room for them; build with mgx_columns_build";
    return static_cast<int>(MGX_ERR_OUT_OF_RANGE);
  };
#define MGX_BUILD_TRY(expr)                                    \
  do {                                                         \
    const hipError_t e__ = (expr);                             \
    if (e__ != hipSuccess) return hip_fail(#expr, e__);        \
  } while (0)

  const uint64_t base = text_off[0], n_bytes = text_off[n_docs] - base;
  const int ascii_n = bp.ngram_size, kanji_n = bp.kanji_ngram_size > 0 ? bp.kanji_ngram_size : bp.ngram_size;
  out->doc_len.assign(n_docs, 0);
  out->offsets.assign(1, 0);
  if (n_docs == 0 || n_bytes == 0) {  // nothing to decode: the columns of an empty index
    if (resident) {
      MGX_BUILD_TRY(hipSetDevice(device));
      Lease lease(device);
      if (!lease.ok) {
        *err = who + "no stream";
        return MGX_ERR_INTERNAL;
      }
      st = lease.stream;
      return fill_resident(0, 0, base, nullptr, nullptr, nullptr, nullptr, nullptr);
    }
    out->docids.assign(4, 0xFFFFFFFFu);
    out->tf.assign(4, 0);
    return MGX_OK;
  }
  MGX_BUILD_TRY(hipSetDevice(device));
  const Layout lay = PlanLayout(n_docs, n_bytes);
  Lease lease(device);
  if (!lease.ok) {
    *err = who + "no stream";
    return MGX_ERR_INTERNAL;
  }
  st = lease.stream;

  // ---- what the library calls ask for (size queries: nothing runs) -----------------------------------------------------
  const uint64_t rec_cap = n_bytes;
  size_t sort_tmp = 0, scan_tmp = 0, block_tmp = 0;
  {
    rocprim::double_buffer<uint64_t> k(nullptr, nullptr), v(nullptr, nullptr);
    MGX_BUILD_TRY(rocprim::radix_sort_pairs(nullptr, sort_tmp, k, v, static_cast<size_t>(rec_cap), 0u, kSortBits, st));
    MGX_BUILD_TRY(rocprim::exclusive_scan(nullptr, scan_tmp, static_cast<uint64_t*>(nullptr), static_cast<uint64_t*>(nullptr),
                                          uint64_t{0}, static_cast<size_t>(rec_cap + 1), rocprim::plus<uint64_t>(), st));
    MGX_BUILD_TRY(rocprim::exclusive_scan(nullptr, block_tmp, static_cast<uint32_t*>(nullptr), static_cast<uint32_t*>(nullptr),
                                          uint32_t{0}, static_cast<size_t>(lay.n_blocks + 1), rocprim::plus<uint32_t>(), st));
  }
  const uint64_t lib_tmp = Align256(std::max<uint64_t>({sort_tmp, scan_tmp, block_tmp, 256}));
  if (lib_tmp > kLibrarySlack + n_bytes) {
    *err = who + "the sort asks for " + std::to_string(lib_tmp) + " bytes of temporary storage, more than the " +
           std::to_string(kLibrarySlack + n_bytes) + " planned for it; build with mgx_columns_build";
    return MGX_ERR_OUT_OF_RANGE;
  }
  const uint64_t arena_bytes = lay.bytes + lib_tmp;
  if (lease.s.arena_bytes < arena_bytes) {
    lease.DropArena();
    size_t free_b = 0, total_b = 0;
    MGX_BUILD_TRY(hipMemGetInfo(&free_b, &total_b));
    Budget budget = PlanBudget(n_docs, n_bytes, free_b);
    if (resident) {  // (at most one posting per text byte)
      budget.needed += PlanResident(n_docs, n_bytes, n_bytes, attach_text).total();
      budget.fits = budget.needed <= free_b;
    }
    if (!budget.fits) {
      *err = who + "the build needs " + std::to_string(budget.needed) + " bytes of temporary device storage, device " +
             std::to_string(device) + " has " + std::to_string(free_b) + " bytes free; build with mgx_columns_build";
      return MGX_ERR_OUT_OF_RANGE;
    }
    const hipError_t e = hipMalloc(&lease.s.arena, arena_bytes);
    if (e != hipSuccess) {
      lease.s.arena = nullptr;
      return hip_fail("hipMalloc of the build's temporary storage", e);
    }
    lease.s.arena_bytes = arena_bytes;
  }
  uint8_t* A = static_cast<uint8_t*>(lease.s.arena);
  auto at = [&](uint64_t o) { return A + o; };
  uint8_t* d_text = at(lay.text);
  uint64_t* d_off = reinterpret_cast<uint64_t*>(at(lay.text_off));
  uint16_t* d_mask = reinterpret_cast<uint16_t*>(at(lay.lane_mask));
  uint32_t* d_prefix = reinterpret_cast<uint32_t*>(at(lay.lane_prefix));
  uint32_t* d_bcount = reinterpret_cast<uint32_t*>(at(lay.block_count));
  uint32_t* d_bbase = reinterpret_cast<uint32_t*>(at(lay.block_base));
  uint32_t* d_doc_cp = reinterpret_cast<uint32_t*>(at(lay.doc_cp_off));
  uint32_t* d_doc_len = reinterpret_cast<uint32_t*>(at(lay.doc_len));
  uint32_t* d_cps = reinterpret_cast<uint32_t*>(at(lay.cps));
  uint32_t* d_cp_doc = reinterpret_cast<uint32_t*>(at(lay.cp_doc));
  uint64_t* d_gkeys = reinterpret_cast<uint64_t*>(at(lay.gram_keys));
  uint64_t* d_goff = reinterpret_cast<uint64_t*>(at(lay.gram_off));
  uint64_t* d_ovf = reinterpret_cast<uint64_t*>(at(lay.overflow));
  uint32_t* d_counters = reinterpret_cast<uint32_t*>(at(lay.counters));
  void* d_tmp = at(lay.bytes);
  size_t tmp_bytes = lib_tmp;
  const uint32_t nb = static_cast<uint32_t>(lay.n_blocks);

  // ---- texts up; 1-3: code points -------------------------------------------------------------------------------------------
  const uint64_t text_cap = lay.n_blocks * kBlockBytes + 2 * kLaneBytes;
  MGX_BUILD_TRY(hipMemcpyAsync(d_text, text_bytes + base, n_bytes, hipMemcpyHostToDevice, st));
  MGX_BUILD_TRY(hipMemsetAsync(d_text + n_bytes, 0, text_cap - n_bytes, st));
  MGX_BUILD_TRY(hipMemcpyAsync(d_off, text_off, (n_docs + 1) * 8, hipMemcpyHostToDevice, st));
  MGX_BUILD_TRY(hipMemsetAsync(d_bcount, 0, (lay.n_blocks + 1) * 4, st));
  MGX_BUILD_TRY(hipMemsetAsync(d_counters, 0, 64, st));
  gram_decode_count_kernel<<<nb, kBlockThreads, 0, st>>>(d_text, d_off, base, n_docs, n_bytes, d_mask, d_bcount);
  MGX_BUILD_TRY(hipGetLastError());
  MGX_BUILD_TRY(rocprim::exclusive_scan(d_tmp, tmp_bytes, d_bcount, d_bbase, uint32_t{0}, static_cast<size_t>(lay.n_blocks + 1),
                                        rocprim::plus<uint32_t>(), st));
  uint32_t n_cps = 0;
  MGX_BUILD_TRY(hipMemcpyAsync(&n_cps, d_bbase + lay.n_blocks, 4, hipMemcpyDeviceToHost, st));
  MGX_BUILD_TRY(hipStreamSynchronize(st));
  if (n_cps > rec_cap) {
    *err = who + "more code points than bytes";
    return MGX_ERR_INTERNAL;
  }
  gram_decode_emit_kernel<<<nb, kBlockThreads, 0, st>>>(d_text, d_off, base, n_docs, n_bytes, d_mask, d_bbase, d_prefix, d_cps,
                                                        d_cp_doc, n_cps);
  MGX_BUILD_TRY(hipGetLastError());
  gram_docs_kernel<<<Blocks(n_docs + 1), kBlockThreads, 0, st>>>(d_off, base, n_docs, n_bytes, n_cps, d_mask, d_prefix, d_doc_cp,
                                                                 d_doc_len);
  MGX_BUILD_TRY(hipGetLastError());
  MGX_BUILD_TRY(hipMemcpyAsync(out->doc_len.data(), d_doc_len, n_docs * 4, hipMemcpyDeviceToHost, st));
  uint64_t G = 0, P = 0;
  uint32_t n_ovf = 0;
  uint32_t* d_docids = d_cps;  // (the columns take the place of the code points once the records are sorted)
  uint8_t* d_tf = reinterpret_cast<uint8_t*>(d_cp_doc);
  if (n_cps > 0) {
    // ---- 5-6: records, sorted --------------------------------------------------------------------------------------------
    rocprim::double_buffer<uint64_t> keys(reinterpret_cast<uint64_t*>(at(lay.key0)), reinterpret_cast<uint64_t*>(at(lay.key1)));
    rocprim::double_buffer<uint64_t> vals(reinterpret_cast<uint64_t*>(at(lay.val0)), reinterpret_cast<uint64_t*>(at(lay.val1)));
    gram_windows_kernel<<<Blocks(n_cps), kBlockThreads, 0, st>>>(d_cps, d_cp_doc, d_doc_cp, n_cps, ascii_n, kanji_n,
                                                                 bp.cross_boundary_ngrams != 0 ? 1 : 0, keys.current(), vals.current());
    MGX_BUILD_TRY(hipGetLastError());
    tmp_bytes = lib_tmp;
    MGX_BUILD_TRY(rocprim::radix_sort_pairs(d_tmp, tmp_bytes, keys, vals, static_cast<size_t>(n_cps), 0u, kSortBits, st));
    // ---- 7-8: heads, tf, columns (flags and their scan live in the sort's other buffers; docids / tf in cps / cp_doc) -----
    uint64_t* d_flags = keys.alternate();
    uint64_t* d_scan = vals.alternate();
    gram_heads_kernel<<<Blocks(static_cast<uint64_t>(n_cps) + 1), kBlockThreads, 0, st>>>(keys.current(), vals.current(), n_cps, d_flags);
    MGX_BUILD_TRY(hipGetLastError());
    tmp_bytes = lib_tmp;
    MGX_BUILD_TRY(rocprim::exclusive_scan(d_tmp, tmp_bytes, d_flags, d_scan, uint64_t{0}, static_cast<size_t>(n_cps) + 1,
                                          rocprim::plus<uint64_t>(), st));
    const uint32_t ovf_cap = static_cast<uint32_t>(n_bytes / 255 + 1);
    gram_tf_kernel<<<Blocks(n_cps), kBlockThreads, 0, st>>>(keys.current(), vals.current(), d_flags, d_scan, n_cps, first_doc_id,
                                                            d_docids, d_tf, d_gkeys, d_goff, d_ovf, ovf_cap, d_counters);
    MGX_BUILD_TRY(hipGetLastError());
    uint64_t totals = 0;
    MGX_BUILD_TRY(hipMemcpyAsync(&totals, d_scan + n_cps, 8, hipMemcpyDeviceToHost, st));
    MGX_BUILD_TRY(hipMemcpyAsync(&n_ovf, d_counters, 4, hipMemcpyDeviceToHost, st));
    MGX_BUILD_TRY(hipStreamSynchronize(st));
    P = totals & 0xFFFFFFFFull;
    G = totals >> 32;
    if (P > n_cps || G > P || n_ovf > ovf_cap) {
      *err = who + "inconsistent counts";
      return MGX_ERR_INTERNAL;
    }
    out->keys.resize(G);
    out->offsets.resize(G + 1);
    out->overflow.resize(n_ovf);
    if (G) MGX_BUILD_TRY(hipMemcpyAsync(out->keys.data(), d_gkeys, G * 8, hipMemcpyDeviceToHost, st));
    if (G) MGX_BUILD_TRY(hipMemcpyAsync(out->offsets.data(), d_goff, G * 8, hipMemcpyDeviceToHost, st));
    if (!resident) {
      out->docids.assign(P + 4, 0xFFFFFFFFu);
      out->tf.assign(P + 4, 0);
      if (P) MGX_BUILD_TRY(hipMemcpyAsync(out->docids.data(), d_docids, P * 4, hipMemcpyDeviceToHost, st));
      if (P) MGX_BUILD_TRY(hipMemcpyAsync(out->tf.data(), d_tf, P, hipMemcpyDeviceToHost, st));
    }
    if (n_ovf) MGX_BUILD_TRY(hipMemcpyAsync(out->overflow.data(), d_ovf, n_ovf * 8ull, hipMemcpyDeviceToHost, st));
  } else if (!resident) {
    out->docids.assign(4, 0xFFFFFFFFu);
    out->tf.assign(4, 0);
  }
  if (resident) {  // (synchronises the stream: the copies above have landed too)
    const int rc = fill_resident(P, n_bytes, base, d_docids, d_tf, d_doc_len, d_text, d_off);
    if (rc != MGX_OK) return rc;
  } else {
    MGX_BUILD_TRY(hipStreamSynchronize(st));
  }
  out->offsets[G] = P;
  std::sort(out->overflow.begin(), out->overflow.end());  // (appended in any order; the posting index is the high word)
  return MGX_OK;
#undef MGX_BUILD_TRY
}

}  // namespace build
}  // namespace mgx
