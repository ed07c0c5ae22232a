/* Replays boolean-AST vectors through oracle/mygram_oracle.c without any binding in between: a stand-alone program, so
 * that it can also be built with -fsanitize=address,undefined (`make -C oracle replay-asan`).
 *
 * Input: a line-oriented case file (tests/test_funnel_queries_cpu.py writes it from tests/golden/pipeline.json), the
 * text last on every line so that it may hold spaces:
 *   case <id> | config <index ngram> <index kanji> <query ngram> <query kanji> <cross> | doc <id> <text> | leaf <text>
 *   node <type> <term> <first_kid> <n_kids> | kid <node> | and <text> | not <text> | fuzzy <d> | expect <ids...>
 *   scoring <leaf indexes...> | run
 * Exit status 0 and "<n> cases ok" when every case matches. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "mygram_oracle.h"

#define MAX_ITEMS 256

typedef struct {
  uint8_t bytes[8192];
  uint32_t off[MAX_ITEMS + 1];
  size_t n;
} strs;

static void strs_push(strs* s, const char* text) {
  size_t len = strlen(text);
  if (s->n >= MAX_ITEMS || s->off[s->n] + len > sizeof(s->bytes)) {
    fprintf(stderr, "case file too large\n");
    exit(2);
  }
  memcpy(s->bytes + s->off[s->n], text, len);
  s->off[s->n + 1] = s->off[s->n] + (uint32_t)len;
  ++s->n;
}

static size_t parse_ids(const char* p, uint32_t* out) {
  size_t n = 0;
  char* end;
  for (;;) {
    unsigned long v = strtoul(p, &end, 10);
    if (end == p) break;
    if (n < MAX_ITEMS) out[n++] = (uint32_t)v;
    p = end;
  }
  return n;
}

int main(int argc, char** argv) {
  if (argc != 2) {
    fprintf(stderr, "usage: %s <case file>\n", argv[0]);
    return 2;
  }
  FILE* f = fopen(argv[1], "r");
  if (!f) {
    perror(argv[1]);
    return 2;
  }
  static char line[4096], id[256];
  static strs leaves, ands, nots;
  static orc_ast_node nodes[MAX_ITEMS];
  static uint32_t kids[MAX_ITEMS + 1], all_docs[MAX_ITEMS], expect[MAX_ITEMS], scoring[MAX_ITEMS], got_sc[MAX_ITEMS];
  size_t n_nodes = 0, n_kids = 0, n_all = 0, n_expect = 0, n_scoring = 0;
  int has_scoring = 0, q_ngram = 2, q_kanji = 0, cross = 0, fuzzy = 0, n_ok = 0, n_bad = 0;
  orc_index* idx = NULL;
  orc_docstore* ds = NULL;
  while (fgets(line, sizeof(line), f)) {
    size_t len = strlen(line);
    while (len && (line[len - 1] == '\n' || line[len - 1] == '\r')) line[--len] = 0;
    char* arg = strchr(line, ' ');
    if (arg) *arg++ = 0; else arg = line + len;
    if (!strcmp(line, "case")) {
      snprintf(id, sizeof(id), "%s", arg);
      leaves.n = ands.n = nots.n = 0;
      n_nodes = n_kids = n_all = n_expect = n_scoring = 0;
      has_scoring = fuzzy = 0;
    } else if (!strcmp(line, "config")) {
      int i_ngram, i_kanji;
      if (sscanf(arg, "%d %d %d %d %d", &i_ngram, &i_kanji, &q_ngram, &q_kanji, &cross) != 5) return 2;
      idx = orc_index_create(i_ngram, i_kanji, 1);
      ds = orc_docstore_create();
    } else if (!strcmp(line, "doc")) {
      char* text;
      unsigned long d = strtoul(arg, &text, 10);
      if (*text == ' ') ++text;
      orc_index_add_document(idx, (uint32_t)d, (const uint8_t*)text, strlen(text));
      orc_docstore_add(ds, (uint32_t)d, (const uint8_t*)text, strlen(text), 1);
      if (n_all < MAX_ITEMS) all_docs[n_all++] = (uint32_t)d;
    } else if (!strcmp(line, "leaf")) {
      strs_push(&leaves, arg);
    } else if (!strcmp(line, "and")) {
      strs_push(&ands, arg);
    } else if (!strcmp(line, "not")) {
      strs_push(&nots, arg);
    } else if (!strcmp(line, "node")) {
      orc_ast_node* n = &nodes[n_nodes < MAX_ITEMS ? n_nodes++ : MAX_ITEMS - 1];
      if (sscanf(arg, "%u %u %u %u", &n->type, &n->term, &n->first_kid, &n->n_kids) != 4) return 2;
    } else if (!strcmp(line, "kid")) {
      if (n_kids < MAX_ITEMS) kids[n_kids++] = (uint32_t)strtoul(arg, NULL, 10);
    } else if (!strcmp(line, "fuzzy")) {
      fuzzy = atoi(arg);
    } else if (!strcmp(line, "expect")) {
      n_expect = parse_ids(arg, expect);
    } else if (!strcmp(line, "scoring")) {
      n_scoring = parse_ids(arg, scoring);
      has_scoring = 1;
    } else if (!strcmp(line, "run")) {
      orc_pipeline_result r;
      int rc = orc_execute_boolean_ast(idx, ds, nodes, n_nodes, kids, leaves.bytes, leaves.off, leaves.n, ands.bytes,
                                       ands.off, ands.n, nots.bytes, nots.off, nots.n, NULL, 0, all_docs, n_all,
                                       fuzzy > 0, (uint32_t)fuzzy, q_ngram, q_kanji, cross, &r);
      int ok = rc == 0 && r.n_results == n_expect && r.after_filters == n_expect && !r.empty_term_detected;
      for (size_t i = 0; ok && i < n_expect; ++i) ok = r.results[i] == expect[i];
      if (ok && has_scoring) {
        size_t n = orc_collect_ast_scoring_terms(nodes, n_nodes, kids, got_sc, MAX_ITEMS);
        ok = n == n_scoring;
        for (size_t i = 0; ok && i < n; ++i) ok = got_sc[i] == scoring[i];
      }
      if (ok) {
        ++n_ok;
      } else {
        ++n_bad;
        printf("case %s: rc %d, %zu results (want %zu), funnel %zu %zu %zu %zu\n", id, rc, rc ? 0 : r.n_results,
               n_expect, r.total_candidates, r.after_intersection, r.after_not, r.after_filters);
      }
      if (rc == 0) orc_pipeline_result_free(&r);
      orc_index_destroy(idx);
      orc_docstore_destroy(ds);
      idx = NULL;
      ds = NULL;
    }
  }
  fclose(f);
  if (n_bad) return 1;
  printf("%d cases ok\n", n_ok);
  return 0;
}
