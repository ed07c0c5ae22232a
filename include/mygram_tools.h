/*
 * mygram_tools.h — bench/test tooling exported by libmygram_gpu.so next to the product ABI (mygram_gpu.h).
 * Not a reference interface: the reference benchmarks against a MySQL-loaded table (support/seed/benchmark.py,
 * e2e/lib/data_generator.py); with no database here the corpus is synthetic, deterministic (seed 42 by default,
 * like e2e/lib/data_generator.py:26) and identical for every consumer (device index, CPU oracle, every rank).
 */
#ifndef MYGRAM_TOOLS_H_
#define MYGRAM_TOOLS_H_
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef struct mgxt_corpus mgxt_corpus;

/* Documents global_first .. global_first+n_docs-1 of the infinite synthetic ASCII corpus `seed`:
 * doc = 4..16 words, word = Zipf(s=1) rank over a 20,000-word vocabulary (word length 2..10, letters Zipf-weighted),
 * single spaces, already normalized (lower-case ASCII). A doc's text depends only on (seed, its global number), so
 * any shard of the corpus can be generated independently. */
int mgxt_corpus_generate(uint64_t seed, uint64_t global_first, uint64_t n_docs, int n_threads, mgxt_corpus** out);
int mgxt_corpus_view(const mgxt_corpus* c, const uint8_t** text_bytes, const uint64_t** text_off, uint64_t* n_docs);
void mgxt_corpus_destroy(mgxt_corpus* c);

/* Streaming-read bandwidth of `device` in GB/s: a read-only kernel over a `bytes`-sized buffer (larger than the
 * 256 MiB Infinity Cache), best of `iters` timed launches (HIP events). bench.py reports it next to the datasheet peak
 * as the measured roofline denominator. */
int mgxt_measure_read_bandwidth(int device, uint64_t bytes, int iters, double* gb_per_s);

/* Test hook (the counterpart of the reference's MYGRAMDB_INDEX_TEST_HOOKS allocation-failure injection,
 * src/index/posting_list.h:217-246): after `after` more successful device allocations, the next `count` allocations of
 * the library fail with an out-of-memory error. count <= 0 switches the hook off. Process-wide. */
void mgxt_fail_device_allocs(int after, int count);

/* Test hook: the host build of the matcher the FUZZY verify_text post-filter runs on the device (kOpVerifyFuzzy, one
 * source: mygram-db_amd/csrc/mgx_fuzzy.hpp) — ContainsFuzzyMatch(text, term, max_distance) of the reference
 * (src/utils/edit_distance.cpp:199-296). 1 / 0, or -1 for max_distance > 2. */
int mgxt_contains_fuzzy_match(const uint8_t* text, size_t text_len, const uint8_t* term, size_t term_len,
                              uint32_t max_distance);

/* Test hooks: the host build of the highlighter the batch path runs on the device (highlight_kernel, one source for the
 * window / merge / clamp / render rules: mygram-db_amd/csrc/mgx_highlight.hpp) — query::Highlighter::Generate and
 * FindMatchPositions of the reference (src/query/highlighter.cpp:252-309) over one NORMALIZED text. Terms are byte
 * strings: term t = terms[t][0 .. term_lens[t]). snippet_length 1..10000, max_fragments 1..100, tags <= 256 bytes (the
 * parser's ranges), else MGX_ERR_OUT_OF_RANGE (3). The text must be valid UTF-8 (normalizer output); on other input the
 * calls stay inside the buffers and the output is unspecified.
 * mgxt_highlight_generate writes at most `cap` bytes of the snippet to `out` and its full length to *out_len.
 * mgxt_highlight_match_positions writes at most `cap_pairs` (start, end) code-point pairs and their number to *n_pairs. */
int mgxt_highlight_generate(const uint8_t* text, size_t text_len, const uint8_t* const* terms, const size_t* term_lens,
                            uint32_t n_terms, uint32_t snippet_length, uint32_t max_fragments, const uint8_t* open_tag,
                            size_t open_len, const uint8_t* close_tag, size_t close_len, uint8_t* out, size_t cap,
                            size_t* out_len);
int mgxt_highlight_match_positions(const uint8_t* text, size_t text_len, const uint8_t* const* terms,
                                   const size_t* term_lens, uint32_t n_terms, uint32_t* out_pairs, size_t cap_pairs,
                                   size_t* n_pairs);
/* query::Highlighter::GenerateOriginal (src/query/highlighter.cpp:311-356) with the normalized-to-original map given
 * instead of a normalizer: the scalar path of the source highlight_original_kernel runs. `kind` is a MGX_ORIG_* value
 * of mygram_gpu.h and map_pairs holds n_pairs (cp_start, cp_end) pairs (MGX_ORIG_MAPPED only), as
 * mgx_index_attach_original_text takes them for one document; MGX_ORIG_NONE is mgxt_highlight_generate over the
 * normalized text. The arguments are trusted as the device trusts an attached document; on input that breaks the
 * contract the call stays inside the buffers and the output is unspecified. */
int mgxt_highlight_generate_original(const uint8_t* original, size_t original_len, const uint8_t* normalized,
                                     size_t normalized_len, uint32_t kind, const uint32_t* map_pairs, size_t n_pairs,
                                     const uint8_t* const* terms, const size_t* term_lens, uint32_t n_terms,
                                     uint32_t snippet_length, uint32_t max_fragments, const uint8_t* open_tag,
                                     size_t open_len, const uint8_t* close_tag, size_t close_len, uint8_t* out,
                                     size_t cap, size_t* out_len);
/* RemoveOverlappingMatchPositions (:227-248) as the stream GenerateOriginal's translated ranges pass on the device and in
 * mgxt_highlight_generate_original: n_pairs (start, end) pairs with non-decreasing starts and non-decreasing ends in,
 * the kept ones out (out_pairs holds up to n_pairs pairs), their number in *n_out. */
int mgxt_highlight_filter_ranges(const uint32_t* pairs, size_t n_pairs, uint32_t* out_pairs, size_t* n_out);

#ifdef __cplusplus
}
#endif
#endif
