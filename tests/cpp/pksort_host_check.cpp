// pksort_host_check.cpp — the host side of mgx_pkey.hpp (key derivation, the key column of an index, and the comparator
// key_merge_kernel runs: CompareKeys / PairBefore are one __host__ __device__ function) as a stand-alone program, without
// a GPU and without Python in between. Reads blocks written by tests/test_primary_key_sort_cpu.py and prints what the
// header makes of them; the test compares that with the Python model. A key is written in hex, "-" for the empty string.
//   derive <n>, then n lines  <has_key> <doc id> <hex>
//       -> n lines  key <numeric 0|1> <value> <key string hex>
//   sort <descending> <n>, then n lines  <side 0|1> <doc id> <has_key> <hex>      (doc ids ascend within a side)
//       -> one line  order <doc id> ...: every document, each side a key column of its own, ordered by PairBefore
//          and  kinds <kind of side 0> <kind of side 1> <monotone 0> <monotone 1>
//   matrix <n> <n_extra>, then n + n_extra lines  <hex>
//       -> n lines  row <n characters '<' '=' '>'>: CompareKeys(key i, key j), the same under every pairing of the
//          forms a key has (rank in the dictionary of the n keys, rank in the dictionary of all n + n_extra keys, the
//          number itself when the key is numeric); a pairing that disagrees ends the program with status 1
// `make pksort-host-asan` builds it with -fsanitize=address,undefined.
#include <algorithm>
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../mygram-db_amd/csrc/mgx_pkey.hpp"

namespace pk = mgx::pkey;
namespace cs = mgx::colsort;

static bool ReadHex(std::FILE* f, std::string* out) {
  char buf[4096];
  if (std::fscanf(f, "%4095s", buf) != 1) return false;
  out->clear();
  if (std::strcmp(buf, "-") == 0) return true;
  const size_t n = std::strlen(buf);
  if (n % 2 != 0) return false;
  for (size_t i = 0; i < n; i += 2) {
    unsigned v;
    if (std::sscanf(buf + i, "%2x", &v) != 1) return false;
    out->push_back(static_cast<char>(v));
  }
  return true;
}
static std::string Hex(const std::string& s) {
  if (s.empty()) return "-";
  std::string h;
  char b[3];
  for (unsigned char c : s) {
    std::snprintf(b, sizeof b, "%02x", c);
    h += b;
  }
  return h;
}

struct Packed {  // keys in the layout mgx_index_set_primary_keys takes
  std::vector<uint8_t> bytes;
  std::vector<uint64_t> off{0};
  std::vector<uint8_t> has;
  void Add(const std::string& s, bool has_key) {
    if (has_key) bytes.insert(bytes.end(), s.begin(), s.end());
    off.push_back(bytes.size());
    has.push_back(has_key ? 1 : 0);
  }
};
static pk::KeySide SideOf(const pk::KeyColumn& c) { return pk::KeySide{c.kind, c.off.data(), c.bytes.data()}; }

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  std::FILE* f = std::fopen(argv[1], "r");
  if (!f) return 2;
  char kind[16];
  int blocks = 0;
  while (std::fscanf(f, "%15s", kind) == 1) {
    ++blocks;
    if (std::strcmp(kind, "derive") == 0) {
      size_t n;
      if (std::fscanf(f, "%zu", &n) != 1) return 2;
      for (size_t i = 0; i < n; ++i) {
        unsigned has;
        uint32_t doc;
        std::string s;
        if (std::fscanf(f, "%u %" SCNu32, &has, &doc) != 2 || !ReadHex(f, &s)) return 2;
        const pk::SortKey k = has ? pk::DeriveKey(reinterpret_cast<const uint8_t*>(s.data()), s.size()) : pk::NumericKey(doc);
        std::printf("key %d %" PRIu64 " %s\n", k.numeric ? 1 : 0, k.value, Hex(pk::KeyString(k)).c_str());
      }
    } else if (std::strcmp(kind, "sort") == 0) {
      unsigned desc;
      size_t n;
      if (std::fscanf(f, "%u %zu", &desc, &n) != 2) return 2;
      Packed in[2];
      std::vector<uint32_t> ids[2];
      for (size_t i = 0; i < n; ++i) {
        unsigned side, has;
        uint32_t doc;
        std::string s;
        if (std::fscanf(f, "%u %" SCNu32 " %u", &side, &doc, &has) != 3 || side > 1 || !ReadHex(f, &s)) return 2;
        in[side].Add(s, has != 0);
        ids[side].push_back(doc);
      }
      pk::KeyColumn col[2];
      pk::KeySide sides[2];
      struct Elem {
        int side;
        uint64_t key;
        uint32_t doc;
      };
      std::vector<Elem> all;
      for (int k = 0; k < 2; ++k) {
        col[k] = pk::BuildKeyColumn(in[k].bytes.data(), in[k].off.data(), in[k].has.data(), ids[k].size(), ids[k].data(), 0);
        sides[k] = SideOf(col[k]);
        for (size_t i = 0; i < ids[k].size(); ++i)  // the carried pair, as the selection kernels write it
          all.push_back(Elem{k, cs::PairKey(cs::KeyOf(cs::kUnsigned, true, 0, col[k].values[i], false), desc != 0),
                             cs::PairDoc(ids[k][i], desc != 0)});
      }
      std::sort(all.begin(), all.end(), [&](const Elem& x, const Elem& y) {
        return pk::PairBefore(sides[x.side], x.key, x.doc, sides[y.side], y.key, y.doc, desc != 0);
      });
      std::printf("order");
      for (const Elem& e : all) std::printf(" %" PRIu32, desc ? e.doc : ~e.doc);
      std::printf("\nkinds %u %u %d %d\n", col[0].kind, col[1].kind, col[0].monotone ? 1 : 0, col[1].monotone ? 1 : 0);
    } else if (std::strcmp(kind, "matrix") == 0) {
      size_t n, n_extra;
      if (std::fscanf(f, "%zu %zu", &n, &n_extra) != 2) return 2;
      Packed small, large;
      std::vector<pk::SortKey> keys;
      for (size_t i = 0; i < n + n_extra; ++i) {
        std::string s;
        if (!ReadHex(f, &s)) return 2;
        if (i < n) {
          small.Add(s, true);
          keys.push_back(pk::DeriveKey(reinterpret_cast<const uint8_t*>(s.data()), s.size()));
        }
        large.Add(s, true);
      }
      const pk::KeyColumn c_small = pk::BuildKeyColumn(small.bytes.data(), small.off.data(), nullptr, n, nullptr, 0);
      const pk::KeyColumn c_large = pk::BuildKeyColumn(large.bytes.data(), large.off.data(), nullptr, n + n_extra, nullptr, 0);
      if (c_small.kind != pk::kKeyRanks || c_large.kind != pk::kKeyRanks) return 2;  // (the test sends raw keys too)
      const pk::KeySide forms[3] = {SideOf(c_small), SideOf(c_large), pk::KeySide{pk::kKeyNumeric, nullptr, nullptr}};
      auto value = [&](size_t i, int form) { return form == 0 ? c_small.values[i] : form == 1 ? c_large.values[i] : keys[i].value; };
      for (size_t i = 0; i < n; ++i) {
        std::string row;
        for (size_t j = 0; j < n; ++j) {
          int first = 2;
          for (int fa = 0; fa < 3; ++fa)
            for (int fb = 0; fb < 3; ++fb) {
              if ((fa == 2 && !keys[i].numeric) || (fb == 2 && !keys[j].numeric)) continue;
              const int c = pk::CompareKeys(forms[fa], value(i, fa), forms[fb], value(j, fb));
              const int sign = c < 0 ? -1 : c > 0 ? 1 : 0;
              if (first == 2) first = sign;
              if (sign != first) {
                std::printf("keys %zu and %zu: forms %d, %d disagree with the first pairing\n", i, j, fa, fb);
                return 1;
              }
            }
          row.push_back(first < 0 ? '<' : first > 0 ? '>' : '=');
        }
        std::printf("row %s\n", row.c_str());
      }
    } else {
      return 2;
    }
  }
  std::fclose(f);
  return blocks > 0 ? 0 : 1;
}
