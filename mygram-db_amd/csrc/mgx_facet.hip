// mgx_facet.hip — FACET in a batch (mgx_batch_set_facets): the value counts of many queries and columns in one launch.
//
//   facet_batch_kernel   one workgroup of four waves per work item (mgx_facet.hpp): a faceted query and a range of whole
//                        tiles of its row of the bitmap group's result bitmaps
//
// The item's words are read once, whatever the number of columns. A wave takes 64 words at a time, one per lane (512
// contiguous bytes), the way column_topk_kernel does: where they are dense (no word holds fewer bits than there are
// non-zero words) it takes one non-zero word per round with the lanes as its 64 documents, so value_ids[slot] of every
// column comes in 256-byte rows; where they are sparse every lane walks its own word's bits (a gather, which a sparse
// result is anyway). Per round and column the lanes hold a value id each:
//   - in a dense round, a column of at most two values (DevColumn::ballot): one ballot + popcount per value, lane v keeps
//     value v's count and adds it once — to the LDS bin, or to the global count when the column holds no bins. No two
//     lanes meet on a bin. (Sparse rounds have few lanes at work: plain atomics are as fast there.)
//   - any other column with LDS bins: one u32 LDS atomic per lane (a workgroup covers fewer than 2^32 documents);
//   - a column without bins: one 64-bit global atomic per lane.
// At the end the workgroup adds its non-zero bins to the counts with one 64-bit atomic per bin. Ids at or above n_values
// (0xFFFFFFFF: NULL) are not counted. Every store is an atomic or a vector store from plain C++.
#include <hip/hip_runtime.h>

#define MGX_FACET_LAUNCHERS
#include "mgx_facet.hpp"

namespace mgx {

namespace fc = facet;

template <bool kDenseRound>
__device__ __forceinline__ void fc_count(const fc::DevColumn& col, uint32_t* __restrict__ bins, uint32_t lane, bool set,
                                         uint32_t slot) {
  const uint32_t id = set ? col.value_ids[slot] : fc::kNoBins;  // (n_values < 2^32 - 1: kNoBins is never counted)
  const bool counted = id < col.n_values;
  if (kDenseRound && col.ballot != 0) {
    uint32_t mine = 0;
    for (uint32_t v = 0; v < col.n_values; ++v) {  // (n_values < 64: one lane per value)
      const uint32_t c = static_cast<uint32_t>(__popcll(__ballot(counted && id == v)));
      mine = lane == v ? c : mine;
    }
    if (mine != 0) {
      if (col.lds_begin != fc::kNoBins) atomicAdd(&bins[col.lds_begin + lane], mine);
      else atomicAdd(&col.counts[lane], static_cast<unsigned long long>(mine));
    }
  } else if (counted) {
    if (col.lds_begin != fc::kNoBins) atomicAdd(&bins[col.lds_begin + id], 1u);
    else atomicAdd(&col.counts[id], 1ull);
  }
}

__global__ __launch_bounds__(fc::kBlock) void facet_batch_kernel(const fc::DevBatch batch) {
  __shared__ uint32_t bins[fc::kLdsBins];
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (blockIdx.x >= batch.n_items) return;
  const fc::Item item = batch.items[blockIdx.x];
  const fc::DevQuery q = batch.queries[item.fq];
  const fc::DevColumn* __restrict__ cols = batch.columns + q.col_begin;
  for (uint32_t i = threadIdx.x; i < q.lds_bins; i += fc::kBlock) bins[i] = 0;
  __syncthreads();
  const uint64_t* __restrict__ row = batch.rbits + q.row_word;
  const uint32_t c_begin = item.word_begin / 64, c_end = (item.word_begin + item.n_words) / 64;  // (whole tiles: 4 chunks each)
  for (uint32_t c = c_begin + wave; c < c_end; c += 4) {
    const unsigned long long word = row[static_cast<uint64_t>(c) * 64 + lane];
    const unsigned long long nz_mask = __ballot(word != 0);
    if (nz_mask == 0) continue;
    uint32_t most = static_cast<uint32_t>(__popcll(word));  // the fullest word of the 64
    for (int o = 32; o > 0; o >>= 1) {
      const uint32_t other = static_cast<uint32_t>(__shfl_xor(static_cast<int>(most), o));
      most = other > most ? other : most;
    }
    if (most < static_cast<uint32_t>(__popcll(nz_mask))) {
      // sparse: every lane walks the bits of its own word, `most` rounds
      unsigned long long bits = word;
      for (uint32_t it = 0; it < most; ++it) {
        const bool has = bits != 0;
        const uint32_t b = has ? static_cast<uint32_t>(__builtin_ctzll(bits)) : 0u;
        bits &= bits - 1;
        const uint64_t slot = (static_cast<uint64_t>(c) * 64 + lane) * 64 + b;
        const bool set = has && slot < batch.n_docs;
        for (uint32_t k = 0; k < q.n_cols; ++k) fc_count<false>(cols[k], bins, lane, set, static_cast<uint32_t>(slot));
      }
    } else {
      // dense: one non-zero word per round, its 64 documents side by side in the lanes
      unsigned long long nz = nz_mask;
      while (nz) {
        const uint32_t w = static_cast<uint32_t>(__builtin_ctzll(nz));
        nz &= nz - 1;
        const unsigned long long bits = __shfl(word, static_cast<int>(w));
        const uint64_t slot = (static_cast<uint64_t>(c) * 64 + w) * 64 + lane;
        const bool set = ((bits >> lane) & 1ull) != 0 && slot < batch.n_docs;
        for (uint32_t k = 0; k < q.n_cols; ++k) fc_count<true>(cols[k], bins, lane, set, static_cast<uint32_t>(slot));
      }
    }
  }
  __syncthreads();
  for (uint32_t k = 0; k < q.n_cols; ++k) {
    const fc::DevColumn col = cols[k];
    if (col.lds_begin == fc::kNoBins) continue;
    for (uint32_t v = threadIdx.x; v < col.n_values; v += fc::kBlock) {
      const uint32_t n = bins[col.lds_begin + v];
      if (n != 0) atomicAdd(&col.counts[v], static_cast<unsigned long long>(n));
    }
  }
}

int LaunchFacetBatch(const fc::DevBatch& batch, hipStream_t s) {
  if (batch.n_items == 0) return 0;
  hipLaunchKernelGGL(facet_batch_kernel, dim3(batch.n_items), dim3(fc::kBlock), 0, s, batch);
  return static_cast<int>(hipGetLastError());
}

}  // namespace mgx
