// colsort_host_check.cpp — the host-side pieces of mgx_colsort.hpp (the key transform KeyOf, the carried pair, the
// collision scan HasKeyCollision) as a stand-alone program, without a GPU and without Python in between. Reads lines
//   key <class> <ranks> <bias> <bits hex> <is_null> <descending> <doc> <T hex> <pair key hex> <pair doc hex>
//   col <class> <marked> <n> (<bits hex> <is_null>) x n      (is_null = 2 on every entry: the column has no NULL array)
// written by tests/test_column_sort_cpu.py from the Python model and checks every one. `make colsort-host-asan` builds it
// with -fsanitize=address,undefined.
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../mygram-db_amd/csrc/mgx_colsort.hpp"

namespace cs = mgx::colsort;

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  std::FILE* f = std::fopen(argv[1], "r");
  if (!f) return 2;
  char kind[8];
  int lines = 0, bad = 0;
  while (std::fscanf(f, "%7s", kind) == 1) {
    ++lines;
    if (std::strcmp(kind, "key") == 0) {
      unsigned cls, ranks, bias, nul, desc;
      uint32_t doc, want_doc;
      uint64_t bits, want_t, want_key;
      if (std::fscanf(f, "%u %u %u %" SCNx64 " %u %u %" SCNu32 " %" SCNx64 " %" SCNx64 " %" SCNx32, &cls, &ranks, &bias, &bits, &nul,
                      &desc, &doc, &want_t, &want_key, &want_doc) != 10)
        return 2;
      const uint64_t t = cs::KeyOf(cls, ranks != 0, bias, bits, nul != 0);
      if (t != want_t || cs::PairKey(t, desc != 0) != want_key || cs::PairDoc(doc, desc != 0) != want_doc) {
        ++bad;
        std::printf("line %d: key differs\n", lines);
      }
      // better(): a pair beats every pair with a smaller key, and at equal keys the one with the smaller docid'
      if (!cs::Better(want_key, want_doc, want_key, want_doc - 1) && want_doc != 0) ++bad;
      if (cs::Better(want_key, want_doc, want_key, want_doc)) ++bad;
    } else if (std::strcmp(kind, "col") == 0) {
      unsigned cls, marked;
      size_t n;
      if (std::fscanf(f, "%u %u %zu", &cls, &marked, &n) != 3) return 2;
      std::vector<uint64_t> values(n);
      std::vector<uint8_t> nulls(n);
      bool no_null_array = n != 0;
      for (size_t i = 0; i < n; ++i) {
        unsigned nul;
        if (std::fscanf(f, "%" SCNx64 " %u", &values[i], &nul) != 2) return 2;
        no_null_array = no_null_array && nul == 2;
        nulls[i] = nul == 1;
      }
      const bool got = cs::HasKeyCollision(cls, values.data(), no_null_array ? nullptr : nulls.data(), n);
      if (got != (marked != 0)) {
        ++bad;
        std::printf("line %d: collision mark differs\n", lines);
      }
    } else {
      return 2;
    }
  }
  std::fclose(f);
  std::printf("%d lines, %d bad\n", lines, bad);
  return bad == 0 && lines > 0 ? 0 : 1;
}
