// mgx_colsort.hip — SORT <filter column> ASC|DESC on the device (ResultSorter::SortAndPaginate, result_sorter.cpp:489-650).
//
//   column_keys_kernel   an expanded doc array -> (key, docid') pairs; the bitonic network of mgx_kernels.hip sorts them
//                        (pages past offset + limit = 1024, unbounded pages, MGX_COLSORT_FULL=1)
//   column_topk_kernel   the bounded page: reads a query's result bitmap, gathers the column under every set bit and keeps
//                        the best `needed` pairs; no expansion, no full sort
//   column_merge_kernel  the per-workgroup lists of a (query, side) -> one sorted run of `needed` pairs
//   key_merge_kernel     SORT by primary key on a table with a delta index: the page of two runs whose values are ranks
//                        in two different key dictionaries, merged by the key strings (mgx_pkey.hpp)
//
// The pair and its order are those of make_sort_keys_kernel / better() (mgx_colsort.hpp restates them: this unit shares no
// code object with the others). Every store is a vector store of one lane.
//
// column_topk_kernel: one workgroup of four waves per (query, side, range of bitmap words). A wave takes 64 words at a
// time, one per lane (512 contiguous bytes). Where they are dense (no word holds fewer bits than there are non-zero
// words) it takes one non-zero word per round, the lanes its 64 docs: the loads of values[slot] (and is_null[slot]) are
// 512 (64) contiguous bytes. Where they are sparse every lane walks its own word's bits, as many rounds as the fullest
// word has bits: a gather, which a sparse result is anyway. Each wave keeps its candidates in an
// LDS buffer of 2 * cap pairs (cap: a power of two >= needed): survivors are appended; when the next 64 could overflow, the
// buffer is sorted (bitonic, in the wave), cut to `needed`, and the needed-th pair becomes the bound later docs must beat.
// At the end the four buffers, adjacent in LDS, are sorted as one by the workgroup and its best `needed` leave as a list.
// LDS: 4 waves * 2 * cap * 12 bytes = 96 KiB at cap 1024 of the CU's 160 KiB (one workgroup per CU there; 12 KiB and
// full occupancy at cap 128, the usual page).
#include <hip/hip_runtime.h>

#define MGX_COLSORT_LAUNCHERS
#include "mgx_colsort.hpp"
#include "mgx_pkey.hpp"

namespace mgx {

namespace cs = colsort;

// Hand-off of LDS words inside ONE wave: its DS operations execute in order; the fences keep the compiler from moving LDS
// accesses across the hand-off.
__device__ __forceinline__ void cs_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ void cs_cmpxchg(uint64_t* k, uint32_t* d, uint32_t i, uint32_t l, bool best_first) {
  const uint64_t ki = k[i], kl = k[l];
  const uint32_t di = d[i], dl = d[l];
  const bool swap = best_first ? cs::Better(kl, dl, ki, di) : cs::Better(ki, di, kl, dl);
  if (swap) {
    k[i] = kl; d[i] = dl;
    k[l] = ki; d[l] = di;
  }
}

// Bitonic sort of n (a power of two) pairs in LDS, best first, by `threads` threads of which this is `t`; Sync() makes
// one stage's stores visible to the next (a wave hand-off or a workgroup barrier).
template <class Sync>
__device__ __forceinline__ void cs_sort(uint64_t* k, uint32_t* d, uint32_t n, uint32_t t, uint32_t threads, Sync sync) {
  for (uint32_t kk = 2; kk <= n; kk <<= 1) {
    for (uint32_t j = kk >> 1; j > 0; j >>= 1) {
      for (uint32_t p = t; p < n / 2; p += threads) {
        const uint32_t i = 2 * p - (p & (j - 1));  // the lower index of pair p at stride j
        cs_cmpxchg(k, d, i, i + j, (i & kk) == 0);
      }
      sync();
    }
  }
}

struct CsWaveList {
  uint64_t* keys;
  uint32_t* docs;
  uint32_t cap, needed, have;
  bool bounded;
  uint64_t bound_key;
  uint32_t bound_doc;
};

// Sorts the wave's buffer, keeps the best `needed`; [have, 2 * cap) is padding (0, 0), which loses to every real pair (a
// real pair (0, 0) is the same pair: `have` counts it).
__device__ __forceinline__ void cs_truncate(CsWaveList& t, uint32_t lane) {
  const uint32_t n = 2 * t.cap;
  for (uint32_t i = t.have + lane; i < n; i += 64) {
    t.keys[i] = 0;
    t.docs[i] = 0;
  }
  cs_wave_sync();
  cs_sort(t.keys, t.docs, n, lane, 64u, [] { cs_wave_sync(); });
  if (t.have >= t.needed) {
    t.have = t.needed;
    t.bounded = true;
    t.bound_key = t.keys[t.needed - 1];
    t.bound_doc = t.docs[t.needed - 1];
  }
}

__device__ __forceinline__ void cs_offer(CsWaveList& t, uint32_t lane, bool valid, uint64_t key, uint32_t doc) {
  bool surv = valid && (!t.bounded || cs::Better(key, doc, t.bound_key, t.bound_doc));
  unsigned long long m = __ballot(surv);
  if (m == 0) return;
  if (t.have + static_cast<uint32_t>(__popcll(m)) > 2 * t.cap) {
    cs_truncate(t, lane);  // (then have <= needed <= cap, and 64 more fit: cap >= 64)
    surv = surv && (!t.bounded || cs::Better(key, doc, t.bound_key, t.bound_doc));
    m = __ballot(surv);
    if (m == 0) return;
  }
  const uint32_t pos = t.have + static_cast<uint32_t>(__popcll(m & ((1ull << lane) - 1ull)));
  if (surv) {
    t.keys[pos] = key;
    t.docs[pos] = doc;
  }
  t.have += static_cast<uint32_t>(__popcll(m));
  cs_wave_sync();
}

__global__ __launch_bounds__(cs::kTopkBlock) void column_topk_kernel(const cs::TopkJob* __restrict__ jobs, uint32_t n_jobs,
                                                                     uint64_t* __restrict__ list_keys,
                                                                     uint32_t* __restrict__ list_docs,
                                                                     uint32_t* __restrict__ list_n) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  __shared__ uint32_t s_have[4];
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  uint32_t lo = 0, hi = n_jobs;  // the job whose workgroups hold this one: the last with group_begin <= blockIdx.x
  while (hi - lo > 1) {
    const uint32_t mid = (lo + hi) >> 1;
    if (jobs[mid].group_begin <= blockIdx.x) lo = mid;
    else hi = mid;
  }
  const cs::TopkJob job = jobs[lo];
  const uint32_t group = blockIdx.x - job.group_begin;
  const uint32_t cap = job.cap;
  uint64_t* const all_keys = reinterpret_cast<uint64_t*>(smem);                                  // [4][2 * cap]
  uint32_t* const all_docs = reinterpret_cast<uint32_t*>(smem + static_cast<size_t>(8) * cap * 8);  // [4][2 * cap]
  CsWaveList t;
  t.keys = all_keys + static_cast<size_t>(wave) * 2 * cap;
  t.docs = all_docs + static_cast<size_t>(wave) * 2 * cap;
  t.cap = cap;
  t.needed = job.needed;
  t.have = 0;
  t.bounded = false;
  t.bound_key = 0;
  t.bound_doc = 0;
  const bool desc = job.descending != 0;
  const uint32_t n_chunks = job.n_words / 64;  // (n_words = 256 per tile)
  const uint32_t per = (n_chunks + job.n_groups - 1) / job.n_groups;
  const uint32_t c_begin = group * per;
  const uint32_t c_end = c_begin + per < n_chunks ? c_begin + per : n_chunks;
  for (uint32_t c = c_begin + wave; c < c_end; c += 4) {
    const unsigned long long word = job.rbits[job.word_begin + static_cast<uint64_t>(c) * 64 + lane];
    const unsigned long long nz_mask = __ballot(word != 0);
    if (nz_mask == 0) continue;
    uint32_t most = static_cast<uint32_t>(__popcll(word));  // the fullest word of the 64
    for (int o = 32; o > 0; o >>= 1) {
      const uint32_t other = static_cast<uint32_t>(__shfl_xor(static_cast<int>(most), o));
      most = other > most ? other : most;
    }
    auto offer_slot = [&](bool set, uint64_t slot64) {
      const bool valid = set && slot64 < job.n_docs;
      const uint32_t slot = static_cast<uint32_t>(slot64);
      uint64_t key = 0;
      uint32_t doc = 0;
      if (valid) {
        const bool nul = job.is_null != nullptr && job.is_null[slot] != 0;
        const uint32_t table_doc = job.doc_map ? job.doc_map[slot] : job.first_doc_id + slot;
        const uint64_t v = job.values ? job.values[slot] : table_doc;  // (no column: an index without primary keys)
        key = cs::PairKey(cs::KeyOf(job.value_class, job.ranks != 0, job.bias, v, nul), desc);
        doc = cs::PairDoc(table_doc, desc);
      }
      cs_offer(t, lane, valid, key, doc);
    };
    if (most < static_cast<uint32_t>(__popcll(nz_mask))) {
      // sparse: every lane walks the bits of its own word — `most` rounds instead of one per non-zero word (a gather)
      unsigned long long bits = word;
      for (uint32_t it = 0; it < most; ++it) {
        const bool set = bits != 0;
        const uint32_t b = set ? static_cast<uint32_t>(__builtin_ctzll(bits)) : 0u;
        bits &= bits - 1;
        offer_slot(set, (static_cast<uint64_t>(c) * 64 + lane) * 64 + b);
      }
    } else {
      // dense: one non-zero word per round, its 64 docs side by side in the lanes — the column is read in 512-byte rows
      unsigned long long nz = nz_mask;
      while (nz) {
        const uint32_t w = static_cast<uint32_t>(__builtin_ctzll(nz));
        nz &= nz - 1;
        const unsigned long long bits = __shfl(word, static_cast<int>(w));
        offer_slot(((bits >> lane) & 1ull) != 0, (static_cast<uint64_t>(c) * 64 + w) * 64 + lane);
      }
    }
  }
  cs_truncate(t, lane);  // the wave's best min(have, needed), sorted; the rest of its buffer padding
  if (t.have > t.needed) t.have = t.needed;
  for (uint32_t i = t.have + lane; i < 2 * cap; i += 64) {
    t.keys[i] = 0;
    t.docs[i] = 0;
  }
  if (lane == 0) s_have[wave] = t.have;
  __syncthreads();
  cs_sort(all_keys, all_docs, 8 * cap, threadIdx.x, cs::kTopkBlock, [] { __syncthreads(); });
  uint32_t total = s_have[0] + s_have[1] + s_have[2] + s_have[3];
  if (total > job.needed) total = job.needed;
  const uint64_t out = job.list_off + static_cast<uint64_t>(group) * job.needed;
  for (uint32_t i = threadIdx.x; i < total; i += cs::kTopkBlock) {
    list_keys[out + i] = all_keys[i];
    list_docs[out + i] = all_docs[i];
  }
  if (threadIdx.x == 0) list_n[blockIdx.x] = total;
}

// Rank of every list element among the job's lists (its index in its own list + the elements of the other lists that
// beat it: a binary search each; the pairs of one side are distinct): ranks below `needed` are the run.
__global__ __launch_bounds__(256) void column_merge_kernel(const cs::TopkJob* __restrict__ jobs, uint32_t job_begin,
                                                           const uint64_t* __restrict__ list_keys,
                                                           const uint32_t* __restrict__ list_docs,
                                                           const uint32_t* __restrict__ list_n,
                                                           uint64_t* __restrict__ keys, uint32_t* __restrict__ dprime) {
  const cs::TopkJob job = jobs[job_begin + blockIdx.y];
  const uint32_t e = blockIdx.x * 256 + threadIdx.x;
  if (e >= job.n_groups * job.needed) return;
  const uint32_t g = e / job.needed, i = e - g * job.needed;
  if (i >= list_n[job.group_begin + g]) return;
  const uint64_t own = job.list_off + static_cast<uint64_t>(g) * job.needed;
  const uint64_t k = list_keys[own + i];
  const uint32_t d = list_docs[own + i];
  uint32_t rank = i;
  for (uint32_t o = 0; o < job.n_groups && rank < job.needed; ++o) {
    if (o == g) continue;
    const uint64_t other = job.list_off + static_cast<uint64_t>(o) * job.needed;
    uint32_t lo = 0, hi = list_n[job.group_begin + o];
    while (lo < hi) {
      const uint32_t mid = (lo + hi) >> 1;
      if (cs::Better(list_keys[other + mid], list_docs[other + mid], k, d)) lo = mid + 1;
      else hi = mid;
    }
    rank += lo;
  }
  if (rank >= job.needed) return;
  keys[job.out_off + rank] = k;
  dprime[job.out_off + rank] = d;
}

__global__ __launch_bounds__(256) void column_keys_kernel(const uint32_t* __restrict__ docs, uint64_t n,
                                                          const uint64_t* __restrict__ values,
                                                          const uint8_t* __restrict__ is_null,
                                                          const uint32_t* __restrict__ doc_map, uint32_t first_doc_id,
                                                          uint32_t n_docs, uint32_t value_class, uint32_t ranks,
                                                          uint32_t bias, int descending, uint64_t* __restrict__ keys,
                                                          uint32_t* __restrict__ dprime) {
  const uint64_t i = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint32_t doc = docs[i];
  const uint32_t slot = doc - first_doc_id;
  if (slot >= n_docs) {  // (expand_kernel writes slots of the index only)
    keys[i] = 0;
    dprime[i] = 0;
    return;
  }
  const bool nul = is_null != nullptr && is_null[slot] != 0;
  const uint32_t table_doc = doc_map ? doc_map[slot] : doc;
  const uint64_t v = values ? values[slot] : table_doc;  // (no column: an index without primary keys)
  keys[i] = cs::PairKey(cs::KeyOf(value_class, ranks != 0, bias, v, nul), descending != 0);
  dprime[i] = cs::PairDoc(table_doc, descending != 0);
}

// SORT by primary key across a main index and its delta: rank_merge_kernel's shape (one thread per element, flat over
// the batch via run_start; a binary search in the other side's run; merged rank = own index + lo; only ranks in
// [lo, hi) are written), with pkey::PairBefore as the order: the values of run A are side a's, those of run B side b's.
// The two runs hold different documents, so no two elements compare equal and the ranks are 0..a_n+b_n-1, each once.
// A wave's lanes mostly share a query, hence the side kinds; the byte loop's trip count differs per lane (common
// prefixes), its loads are single bytes at unrelated addresses: the kernel is latency-bound on 2 * (offset + limit)
// elements per query.
__global__ __launch_bounds__(256) void key_merge_kernel(const pkey::KeyMergeRun* __restrict__ runs,
                                                        const uint64_t* __restrict__ run_start, uint32_t n_runs,
                                                        pkey::KeySide side_a, pkey::KeySide side_b,
                                                        const uint64_t* __restrict__ keys,
                                                        const uint32_t* __restrict__ dprime,
                                                        uint32_t* __restrict__ out_docs, double* __restrict__ out_scores) {
  const uint64_t e = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (e >= run_start[n_runs]) return;
  uint32_t qlo = 0, qhi = n_runs;  // the run q with run_start[q] <= e < run_start[q + 1]
  while (qhi - qlo > 1) {
    const uint32_t mid = (qlo + qhi) >> 1;
    if (run_start[mid] <= e) qlo = mid;
    else qhi = mid;
  }
  const pkey::KeyMergeRun r = runs[qlo];
  const uint32_t j = static_cast<uint32_t>(e - run_start[qlo]);
  const bool from_a = j < r.a_n;
  const uint32_t k = from_a ? j : j - r.a_n;
  const uint64_t own = from_a ? r.a_off : r.b_off, other = from_a ? r.b_off : r.a_off;
  const uint32_t other_n = from_a ? r.b_n : r.a_n;
  const pkey::KeySide& s_own = from_a ? side_a : side_b;
  const pkey::KeySide& s_other = from_a ? side_b : side_a;
  const bool desc = r.descending != 0;
  const uint64_t kx = keys[own + k];
  const uint32_t x = dprime[own + k];
  uint32_t lo = 0, hi = other_n;
  while (lo < hi) {
    const uint32_t mid = (lo + hi) >> 1;
    if (pkey::PairBefore(s_other, keys[other + mid], dprime[other + mid], s_own, kx, x, desc)) lo = mid + 1;
    else hi = mid;
  }
  const uint32_t rank = k + lo;
  if (rank < r.lo || rank >= r.hi) return;
  const uint64_t o = r.out_off + (rank - r.lo);
  out_docs[o] = desc ? x : ~x;
  out_scores[o] = 0.0;
}

int LaunchColumnKeys(const uint32_t* docs, uint64_t n, const uint64_t* values, const uint8_t* is_null,
                     const uint32_t* doc_map, uint32_t first_doc_id, uint32_t n_docs, uint32_t value_class,
                     uint32_t ranks, uint32_t bias, int descending, uint64_t* keys, uint32_t* dprime, hipStream_t s) {
  if (n == 0) return 0;
  hipLaunchKernelGGL(column_keys_kernel, dim3(static_cast<uint32_t>((n + 255) / 256)), dim3(256), 0, s, docs, n, values,
                     is_null, doc_map, first_doc_id, n_docs, value_class, ranks, bias, descending, keys, dprime);
  return static_cast<int>(hipGetLastError());
}

int LaunchKeyMerge(const pkey::KeyMergeRun* runs, const uint64_t* run_start, uint32_t n_runs, uint64_t n_elems,
                   pkey::KeySide a, pkey::KeySide b, const uint64_t* keys, const uint32_t* dprime, uint32_t* out_docs,
                   double* out_scores, hipStream_t s) {
  if (n_runs == 0 || n_elems == 0) return 0;
  hipLaunchKernelGGL(key_merge_kernel, dim3(static_cast<uint32_t>((n_elems + 255) / 256)), dim3(256), 0, s, runs,
                     run_start, n_runs, a, b, keys, dprime, out_docs, out_scores);
  return static_cast<int>(hipGetLastError());
}

uint32_t ColumnTopkLdsBytes(uint32_t cap) { return 8u * cap * 12u; }

int LaunchColumnTopk(const cs::TopkJob* jobs, uint32_t n_jobs, uint32_t n_groups_total, uint32_t max_cap,
                     uint32_t max_job_elems, uint64_t* list_keys, uint32_t* list_docs, uint32_t* list_n, uint64_t* keys,
                     uint32_t* dprime, hipStream_t s) {
  if (n_jobs == 0 || n_groups_total == 0) return 0;
  if (max_cap < 64 || max_cap > cs::kMaxNeeded || (max_cap & (max_cap - 1)) != 0) return static_cast<int>(hipErrorInvalidValue);
  const uint32_t lds = ColumnTopkLdsBytes(max_cap);
  if (lds > 48u * 1024u) {
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&column_topk_kernel),
                                             hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(lds));
    if (e != hipSuccess) return static_cast<int>(e);
  }
  hipLaunchKernelGGL(column_topk_kernel, dim3(n_groups_total), dim3(cs::kTopkBlock), lds, s, jobs, n_jobs, list_keys,
                     list_docs, list_n);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return static_cast<int>(e);
  if (max_job_elems == 0 || max_job_elems > cs::kTopkMaxGroups * cs::kMaxNeeded) return static_cast<int>(hipErrorInvalidValue);
  const uint32_t gx = (max_job_elems + 255) / 256;
  for (uint32_t j0 = 0; j0 < n_jobs; j0 += 65535u) {  // (grid.y holds 65535)
    const uint32_t nj = n_jobs - j0 < 65535u ? n_jobs - j0 : 65535u;
    hipLaunchKernelGGL(column_merge_kernel, dim3(gx, nj), dim3(256), 0, s, jobs, j0, list_keys, list_docs, list_n, keys,
                       dprime);
    e = hipGetLastError();
    if (e != hipSuccess) return static_cast<int>(e);
  }
  return 0;
}

}  // namespace mgx
