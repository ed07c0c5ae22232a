// mgx_build.hpp — the device column builder (mgx_columns_build_device, mgx_index_build_device): what mgx_build.hip and its
// callers share.
//
//   key      a gram of at most kMaxGram code points packed into a u64: code point j as `cp + 1` in the 21-bit field at
//            bits [42 - 21 j, 63 - 21 j), absent positions 0. Integer order of the packed keys == bytewise order of the
//            grams' UTF-8 strings, shorter prefix first (UTF-8 preserves code-point order, and the +1 puts "absent" below
//            U+0000), and the packing is injective. tests/cpp/build_host_check.cpp pins both against the 128-bit host key.
//   record   (key, (doc slot << 32) | code-point position), one per code point of the texts; a code point at which no
//            window starts carries kNoWindow, which sorts behind every key
//   plan     the temporary device storage of one build as a function of (documents, text bytes), and the verdict
//            against the free memory of the device. Plain arithmetic: it compiles without a HIP header.
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/mygram_gpu.h"

#if defined(__HIPCC__)
#define MGX_BUILD_HD __host__ __device__ inline
#else
#define MGX_BUILD_HD inline
#endif

namespace mgx {
namespace build {

constexpr int kMaxGram = 3;                        // code points per gram that a packed key holds
constexpr uint64_t kNoWindow = (1ull << 63) - 1;   // > every packed key: field 0 is at most 0x110000 < 2^21 - 1
constexpr uint32_t kSortBits = 63;
constexpr uint32_t kLaneBytes = 16;                // text bytes per lane of the decode kernels
constexpr uint32_t kBlockThreads = 256;
constexpr uint32_t kBlockBytes = kLaneBytes * kBlockThreads;
// every index of the pipeline (code point, record, posting) is a u32
constexpr uint64_t kMaxTextBytes = 0xFFFFFFFFull - 2 * kBlockBytes;
constexpr uint64_t kLibrarySlack = 64ull << 20;    // + 1 byte per text byte: what the sort and the scans may ask for

MGX_BUILD_HD uint64_t PackKey(const uint32_t* cps, int w) {
  uint64_t k = 0;
  for (int j = 0; j < w; ++j) k |= static_cast<uint64_t>(cps[j] + 1u) << (42 - 21 * j);
  return k;
}
MGX_BUILD_HD uint32_t KeyField(uint64_t key, int j) { return static_cast<uint32_t>(key >> (42 - 21 * j)) & 0x1FFFFFu; }
// the window size in code points: the filled fields (a filled field is never 0)
MGX_BUILD_HD int KeyWidth(uint64_t key) {
  return (KeyField(key, 0) ? 1 : 0) + (KeyField(key, 1) ? 1 : 0) + (KeyField(key, 2) ? 1 : 0);
}

inline uint64_t Align256(uint64_t v) { return (v + 255) & ~255ull; }

// Where every temporary array of one build lies inside its single device allocation (byte offsets, 256-aligned).
// N, the number of code points, is known only on the device; N <= text bytes bounds every per-record array.
struct Layout {
  uint64_t n_lanes = 0, n_blocks = 0;
  uint64_t text = 0, text_off = 0, lane_mask = 0, lane_prefix = 0, block_count = 0, block_base = 0, doc_cp_off = 0,
           doc_len = 0, cps = 0, cp_doc = 0, key0 = 0, key1 = 0, val0 = 0, val1 = 0, gram_keys = 0, gram_off = 0,
           overflow = 0, counters = 0;
  uint64_t bytes = 0;  // without the sort / scan library's own temporary storage
};

inline Layout PlanLayout(uint64_t n_docs, uint64_t text_bytes) {
  Layout l;
  l.n_lanes = (text_bytes + kLaneBytes - 1) / kLaneBytes;
  l.n_blocks = (l.n_lanes + kBlockThreads - 1) / kBlockThreads;
  const uint64_t lanes = l.n_blocks * kBlockThreads, rec = text_bytes + 1;
  uint64_t at = 0;
  auto take = [&](uint64_t bytes) {
    const uint64_t o = at;
    at += Align256(bytes);
    return o;
  };
  l.text = take(lanes * kLaneBytes + 2 * kLaneBytes);  // (the decode loads whole 16-byte words and 4 bytes behind them)
  l.text_off = take((n_docs + 1) * 8);
  l.lane_mask = take(lanes * 2);
  l.lane_prefix = take(lanes * 4);
  l.block_count = take((l.n_blocks + 1) * 4);
  l.block_base = take((l.n_blocks + 1) * 4);
  l.doc_cp_off = take((n_docs + 1) * 4);
  l.doc_len = take((n_docs + 1) * 4);
  l.cps = take(rec * 4);     // later: the docids column
  l.cp_doc = take(rec * 4);  // later: the tf column
  l.key0 = take(rec * 8);
  l.key1 = take(rec * 8);
  l.val0 = take(rec * 8);
  l.val1 = take(rec * 8);
  l.gram_keys = take(rec * 8);
  l.gram_off = take(rec * 8);
  l.overflow = take((text_bytes / 255 + 1) * 8);  // an overflow entry stands for >= 255 records of its own
  l.counters = take(64);
  l.bytes = at;
  return l;
}

struct Budget {
  uint64_t needed = 0;  // bytes of device memory one build asks for at the most
  bool fits = false;
};

// The verdict of the out-of-memory refusal: the layout plus what the library calls may ask for, against `free_bytes`.
inline Budget PlanBudget(uint64_t n_docs, uint64_t text_bytes, uint64_t free_bytes) {
  Budget b;
  b.needed = PlanLayout(n_docs, text_bytes).bytes + kLibrarySlack + text_bytes;
  b.fits = b.needed <= free_bytes;
  return b;
}

// What the device hands back: the columns in host memory, grams still as packed keys.
struct PackedColumns {
  std::vector<uint64_t> keys;      // G, ascending
  std::vector<uint64_t> offsets;   // G + 1
  std::vector<uint32_t> docids;    // P + 4 (the host builder's padding)
  std::vector<uint8_t> tf;         // P + 4
  std::vector<uint32_t> doc_len;   // n_docs
  std::vector<uint64_t> overflow;  // (posting index << 32) | true tf, ascending
};

// ---- the resident ending (mgx_index_build_device) ---------------------------------------------------------------------
// The arrays a device index owns after a build that never brings the postings to the host: exactly the allocations
// mgx_index_create and mgx_index_attach_text make for the same columns, byte for byte, their padding included.
constexpr uint64_t kResidentTileDocs = 16384;   // mgx::kTileDocs (mgx_build.hip asserts it): dl8 is padded to whole tiles
constexpr uint64_t kResidentIdPad = 4;          // entries of 0xFF behind docids and tf
constexpr uint64_t kResidentDl8Pad = 16;        // bytes of 0xFF behind dl8
constexpr uint64_t kResidentTextPad = 128;      // bytes of 0xFF behind the texts
constexpr uint32_t kResidentSlotsPerLane = 4;   // doc slots one lane of resident_rows_kernel packs into one store

struct ResidentPlan {
  uint64_t dl8_slots = 0;  // n_docs rounded up to whole tiles
  uint64_t docids = 0, tf = 0, doc_len = 0, dl8 = 0, text = 0, text_off = 0;  // bytes of each allocation
  uint64_t lanes = 0;      // of resident_rows_kernel: covers dl8_slots and, with texts, the n_docs + 1 offsets
  uint64_t total() const { return docids + tf + doc_len + dl8 + text + text_off; }
};

inline ResidentPlan PlanResident(uint64_t n_docs, uint64_t n_postings, uint64_t text_bytes, bool attach_text) {
  ResidentPlan r;
  r.dl8_slots = (n_docs + kResidentTileDocs - 1) / kResidentTileDocs * kResidentTileDocs;
  r.docids = (n_postings + kResidentIdPad) * 4;
  r.tf = n_postings + kResidentIdPad;
  r.doc_len = n_docs * 4;
  r.dl8 = r.dl8_slots + kResidentDl8Pad;
  r.text = attach_text ? text_bytes + kResidentTextPad : 0;
  r.text_off = attach_text ? (n_docs + 1) * 8 : 0;
  const uint64_t slots = attach_text && n_docs + 1 > r.dl8_slots ? n_docs + 1 : r.dl8_slots;
  r.lanes = (slots + kResidentSlotsPerLane - 1) / kResidentSlotsPerLane;
  return r;
}

// Device allocations handed from the build to the index that adopts them (mgx_api.cpp); what is still here when the
// object goes is freed.
struct ResidentArrays {
  ResidentPlan plan;
  void *docids = nullptr, *tf = nullptr, *doc_len = nullptr, *dl8 = nullptr, *text = nullptr, *text_off = nullptr;
  ResidentArrays() = default;
  ResidentArrays(const ResidentArrays&) = delete;
  ResidentArrays& operator=(const ResidentArrays&) = delete;
  ~ResidentArrays() { Free(); }
  void Free();  // mgx_build.hip
};

// mgx_build.hip. text_off[0 .. n_docs] ascends (the caller checked). Returns an MGX_* code and fills *err.
// `resident` null: every column comes back in *out. Otherwise (n_docs >= 1): out->docids and out->tf stay empty, and the
// postings, tf, doc_len, the padded dl8 row and, with attach_text, the texts and their offsets from 0 are left in
// *resident, copied device to device out of the build's temporary storage.
int BuildOnDevice(const mgx_build_params& bp, const uint8_t* text_bytes, const uint64_t* text_off, uint32_t first_doc_id,
                  uint64_t n_docs, int device, PackedColumns* out, std::string* err, ResidentArrays* resident = nullptr,
                  bool attach_text = false);

}  // namespace build

struct Columns;
// mgx_columns.cpp: packed keys -> key bytes / 128-bit keys, BM25 statistics from doc_len and the texts' byte lengths
Columns* ColumnsFromPacked(const mgx_build_params& bp, const uint64_t* text_off, uint32_t first_doc_id, uint64_t n_docs,
                           build::PackedColumns&& p);

}  // namespace mgx
