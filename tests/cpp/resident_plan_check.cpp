// resident_plan_check.cpp — the plain arithmetic of the resident ending of the device builder (mgx_index_build_device:
// mygram-db_amd/csrc/mgx_build.hpp, PlanResident), stand-alone: g++ -std=c++17 [-fsanitize=address,undefined], no GPU.
//   1  every allocation has the size mgx_index_create / mgx_index_attach_text give the same array (restated here)
//   2  the lanes of resident_rows_kernel, restated lane by lane over exactly sized host arrays: every dl8 slot and every
//      text offset is written exactly once, nothing outside the arrays is touched (the sanitizer's part), and the rows
//      hold min(doc_len, 255) with zeros up to the tile boundary and the offsets rebased to 0
//   3  sizes near 2^32 documents and 4 GiB of text do not wrap
// Exits non-zero at the first property that fails; prints "resident plan ok: <checks>".
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "../../mygram-db_amd/csrc/mgx_build.hpp"

namespace {

using namespace mgx::build;
unsigned long long g_checks = 0;

#define CHECK(cond)                                                      \
  do {                                                                   \
    ++g_checks;                                                          \
    if (!(cond)) {                                                       \
      std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond);    \
      std::exit(1);                                                      \
    }                                                                    \
  } while (0)

void CheckSizes(uint64_t n_docs, uint64_t postings, uint64_t bytes, bool attach) {
  const ResidentPlan p = PlanResident(n_docs, postings, bytes, attach);
  const uint64_t tiles = (n_docs + 16383) / 16384;
  CHECK(p.dl8_slots == tiles * 16384 && p.dl8_slots >= n_docs && p.dl8_slots - n_docs < 16384);
  CHECK(p.docids == (postings + 4) * 4);  // Upload(d_docids, docids, P, 4)
  CHECK(p.tf == postings + 4);            // Upload(d_tf, tf, P, 4)
  CHECK(p.doc_len == n_docs * 4);         // Upload(d_doc_len, doc_len, n_docs)
  CHECK(p.dl8 == tiles * 16384 + 16);     // Upload(d_dl8, dl8, whole tiles, 16)
  CHECK(p.text == (attach ? bytes + 128 : 0));           // Upload(d_text, text, total, 128)
  CHECK(p.text_off == (attach ? (n_docs + 1) * 8 : 0));  // Upload(d_text_off, rel, n_docs + 1)
  CHECK(p.total() == p.docids + p.tf + p.doc_len + p.dl8 + p.text + p.text_off);
  // the lanes cover every dl8 slot and, with texts, every offset; not a lane more than that needs
  const uint64_t need = attach && n_docs + 1 > p.dl8_slots ? n_docs + 1 : p.dl8_slots;
  CHECK(p.lanes * kResidentSlotsPerLane >= need && (p.lanes - 1) * kResidentSlotsPerLane < need);
  CHECK((p.lanes + kBlockThreads - 1) / kBlockThreads <= 0xFFFFFFFFull);  // the grid's block count is a u32
}

// resident_rows_kernel, one lane at a time (the launch rounds the lanes up to whole blocks)
void CheckRows(uint64_t n_docs, bool attach, std::mt19937_64& rng) {
  const uint64_t base = rng() % 1000;
  std::vector<uint32_t> doc_len(n_docs);
  std::vector<uint64_t> off(n_docs + 1);
  off[0] = base;
  for (uint64_t d = 0; d < n_docs; ++d) {
    const uint64_t r = rng();
    doc_len[d] = r % 5 == 0 ? 0 : r % 7 == 0 ? 255 + static_cast<uint32_t>(r % 70000) : static_cast<uint32_t>(r % 300);
    off[d + 1] = off[d] + doc_len[d];
  }
  const ResidentPlan p = PlanResident(n_docs, 0, off[n_docs] - base, attach);
  std::vector<uint8_t> dl8(p.dl8, 0xEE);
  std::vector<uint64_t> text_off(p.text_off / 8, ~0ull);
  std::vector<uint8_t> dl8_writes(p.dl8, 0), off_writes(text_off.size(), 0);
  const uint64_t launched = (p.lanes + kBlockThreads - 1) / kBlockThreads * kBlockThreads;
  for (uint64_t lane = 0; lane < launched; ++lane) {
    const uint64_t s0 = lane * kResidentSlotsPerLane;
    if (s0 < p.dl8_slots) {
      uint32_t len[kResidentSlotsPerLane] = {0, 0, 0, 0};
      if (s0 + kResidentSlotsPerLane <= n_docs) {
        for (uint32_t j = 0; j < kResidentSlotsPerLane; ++j) len[j] = doc_len.at(s0 + j);  // the 16-byte load
      } else {
        for (uint32_t j = 0; j < kResidentSlotsPerLane; ++j)
          if (s0 + j < n_docs) len[j] = doc_len.at(s0 + j);
      }
      for (uint32_t j = 0; j < kResidentSlotsPerLane; ++j) {  // the 4-byte store
        dl8.at(s0 + j) = static_cast<uint8_t>(len[j] < 255u ? len[j] : 255u);
        dl8_writes.at(s0 + j)++;
      }
    }
    if (attach)
      for (uint32_t j = 0; j < kResidentSlotsPerLane; ++j)
        if (s0 + j <= n_docs) {
          text_off.at(s0 + j) = off.at(s0 + j) - base;
          off_writes.at(s0 + j)++;
        }
  }
  for (uint64_t s = 0; s < p.dl8_slots; ++s) {
    CHECK(dl8_writes[s] == 1);
    CHECK(dl8[s] == (s < n_docs ? (doc_len[s] < 255 ? doc_len[s] : 255) : 0));
  }
  for (uint64_t s = p.dl8_slots; s < p.dl8; ++s) CHECK(dl8_writes[s] == 0 && dl8[s] == 0xEE);  // the pad is the memset's
  if (attach) {
    CHECK(text_off.size() == n_docs + 1);
    for (uint64_t d = 0; d <= n_docs; ++d) CHECK(off_writes[d] == 1 && text_off[d] == off[d] - base);
    CHECK(text_off[0] == 0);
  }
}

}  // namespace

int main() {
  static_assert(kResidentTileDocs % kResidentSlotsPerLane == 0, "a lane's slots lie in one tile");
  std::mt19937_64 rng(20);
  const uint64_t docs[] = {1,     2,     3,     4,     5,         255,       256,        257,           16383,         16384,
                           16385, 16461, 32767, 32768, 32769,     1000000,   10000000,   0xFFFFFFFEull, 0xFFFF0000ull, 49152};
  const uint64_t sizes[] = {0, 1, 3, 4, 255, 4096, 1ull << 20, 231ull << 20, kMaxTextBytes - 1, kMaxTextBytes};
  for (uint64_t n : docs)
    for (uint64_t bytes : sizes)
      for (uint64_t postings : {uint64_t{0}, bytes / 2, bytes})
        for (bool attach : {false, true}) CheckSizes(n, postings, bytes, attach);
  for (int i = 0; i < 2000; ++i) CheckSizes(1 + rng() % 0xFFFFFFFEull, rng() % kMaxTextBytes, rng() % kMaxTextBytes, i % 2 == 0);
  // the budget's bound: at most one posting per text byte
  for (uint64_t n : docs)
    for (uint64_t bytes : sizes)
      CHECK(PlanResident(n, bytes / 3, bytes, true).total() <= PlanResident(n, bytes, bytes, true).total());
  for (uint64_t n : {1ull, 2ull, 3ull, 4ull, 5ull, 7ull, 8ull, 63ull, 1023ull, 1024ull, 1025ull, 16383ull, 16384ull, 16385ull, 16461ull,
                     32768ull, 32769ull})
    for (bool attach : {false, true}) CheckRows(n, attach, rng);
  std::printf("resident plan ok: %llu checks\n", g_checks);
  return 0;
}
