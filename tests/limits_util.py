"""Corpora, queries and coverage conditions of the capacity-limit tests (test_gpu_limits.py on the device,
test_limits_cpu.py with the oracle alone). Nothing here needs a device: a `side` is a gpu_util.OracleSide (or a Pair).

Every limit the tile program declares is a constant its kernels' correctness rests on: 127 grams per threshold term (7-bit
bit-sliced counters), 40 stack levels, 512 expression tokens, 192 distinct operands, 64 LDS-resident operands, 64 scored
terms, 160 KiB of LDS. The generators here build the shapes AT each limit and one past it, on indexes that are the
smallest at which the kernels can go wrong: three tiles with a partial last tile and a last word that is not full
(2 * 16384 + 77 documents), and a two-tile lists-only index (16384 + 300 documents, dense_threshold=2.0)."""
import numpy as np

import funnel_util as FU
from pkg import mg

Query = mg.engine.Query
TILE = 16384
BITMAP_DOCS, LISTS_DOCS = FU.BITMAP_DOCS, FU.LISTS_DOCS
OUT_OF_RANGE, NOT_IMPLEMENTED = 3, 4  # MGX_ERR_*

# ---- A. threshold counters: the hand-built corpora ------------------------------------------------------------------------
# two-letter tokens xy, x in a..m and y in n..z: space-separated tokens form no other token's bigram ("y " and " x" only)
TOKENS = sorted(x + y for x in "abcdefghijklm" for y in "nopqrstuvwxyz")
GRAMS, SPARE = TOKENS[:127], TOKENS[127:]
RARE_FROM = 100  # GRAMS[RARE_FROM:] stay below n_docs / 256 postings on the bitmap corpus: sorted-list operands
THRESHOLD_T = (7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 126, 127)
LISTS_MAX_T = 64  # a lists-only index holds 64 operands in LDS: T = 65 is refused
LAST_TILE_TOP = (124, 125, 126, 127)  # the counts above 66 that the 77-document last tile holds


def thetas(T):
    """2, every 2^k - 1, 2^k and 2^k + 1 below T, T - 1, and the two that compile to other code: 1 (a union) and T (an AND)."""
    s = {1, 2, T - 1, T}
    k = 1
    while (1 << k) - 1 < T:
        s.update(v for v in ((1 << k) - 1, 1 << k, (1 << k) + 1) if v < T)
        k += 1
    return sorted(v for v in s if 1 <= v <= T)


def _texts(held, spare):
    g, s = np.asarray(GRAMS, object), np.asarray(SPARE, object)
    return [" ".join(list(g[held[i]]) + list(s[spare[i]])) for i in range(len(held))]


def threshold_corpus_bitmap(seed=301):
    """-> (texts, held [n, 127] bool). Random documents hold every gram below RARE_FROM with a probability of their own
    (0 .. 0.6) and the rare grams almost never; LADDERS of prefix documents (the first c grams, c ascending) sit word-aligned
    in every tile: c = 0..63, 32..95 and 64..127 in three consecutive words of the two full tiles (so that c - 1, c, c + 1
    share a word for every c), and c = 0..66 plus 124..127 in the 77 documents of the last tile, whose last document
    (the top bit of the partial last word) holds all 127."""
    n = BITMAP_DOCS
    rng = np.random.default_rng(seed)
    held = rng.random((n, len(GRAMS))) < (rng.random(n) * 0.6)[:, None]
    held[:, RARE_FROM:] = rng.random((n, len(GRAMS) - RARE_FROM)) < 0.0006
    spare = rng.random((n, len(SPARE))) < 0.3

    def prefix(slot, c):
        held[slot] = False
        held[slot, :c] = True
        spare[slot] = c == len(GRAMS)

    for tile in (0, 1):
        base = tile * TILE + 64 * (3 + 100 * tile)
        for w, lo in enumerate((0, 32, 64)):
            for j in range(64):
                prefix(base + 64 * w + j, lo + j)
    for j in range(64):
        prefix(2 * TILE + j, j)
    for j, c in enumerate((64, 65, 66) + LAST_TILE_TOP):
        prefix(n - 7 + j, c)
    return _texts(held, spare), held


def threshold_corpus_lists(seed=302):
    """-> (texts, held). The lists-only corpus: GRAMS[:64] occur in the second tile only (300 documents: ladders
    c = 0..63 and 1..64 in its first two words, random subsets after them), GRAMS[64:] in the first tile only (a ladder
    over GRAMS[64:] in its fourth word, random subsets elsewhere): a query over GRAMS[:T] finds a whole tile without a
    posting, and a query that mixes both halves finds tiles that hold only some of its lists."""
    n = LISTS_DOCS
    rng = np.random.default_rng(seed)
    held = rng.random((n, len(GRAMS))) < (rng.random(n) * 0.2)[:, None]
    held[:TILE, :64] = False
    held[TILE:, 64:] = False
    held[TILE:] &= rng.random((n - TILE, len(GRAMS))) < 0.5
    spare = np.zeros((n, len(SPARE)), bool)
    for j in range(64):
        held[3 * 64 + j] = False
        held[3 * 64 + j, 64:64 + j] = True
        for w, lo in enumerate((0, 1)):
            held[TILE + 64 * w + j] = False
            held[TILE + 64 * w + j, :lo + j] = True
    return _texts(held, spare), held


# (T, theta, grams) of queries that mix the halves of the lists-only corpus: in the first tile exactly theta of the T lists
# have a posting (tile_may_match's `cnt >= arg` at equality), or exactly T - 1 = theta of them (a threshold term requires
# none of its operands unless it asks for all of them: tile_jump_setup)
def mixed_threshold_cases():
    out = []
    for T, th in ((16, 8), (40, 8), (64, 33), (9, 8), (33, 32), (64, 63), (5, 2)):
        out.append((T, th, GRAMS[64:64 + th] + GRAMS[:T - th]))
    return out


def threshold_coverage(held, n_tiles_full, lists=False):
    """Conditions (i) and (ii), asserted from the membership columns. -> the T values checked."""
    n = len(held)
    ts = [T for T in THRESHOLD_T if not lists or T <= LISTS_MAX_T]
    cum = np.cumsum(held, axis=1)
    for T in ts:
        cnt = cum[:, T - 1]
        if lists:
            tiles = [cnt[TILE:]]  # (the grams in use live in the second tile alone)
        else:
            tiles = [cnt[t * TILE:(t + 1) * TILE] for t in range(n_tiles_full)]
        for c in tiles:
            assert set(range(T + 1)) <= set(c.tolist()), (T, sorted(set(range(T + 1)) - set(c.tolist())))
        if not lists:
            # the 77 documents of the last tile cannot take 127 values: every value up to 66, and for the larger T every
            # count next to a threshold in use
            last = set(cnt[n_tiles_full * TILE:].tolist())
            want = set(range(min(T, 66) + 1))
            for th in thetas(T):
                want |= {v for v in (th - 1, th, th + 1) if v <= T}
            assert want <= last, (T, sorted(want - last))
        words = [set(cnt[w:w + 64].tolist()) for w in range(0, n, 64)]
        for th in thetas(T):
            need = {v for v in (th - 1, th, th + 1) if v <= T}
            assert any(need <= w for w in words), (T, th)
    return ts


# ---- A. FUZZY on long words ------------------------------------------------------------------------------------------------
ALPHABET = "abcdefghijklmnop"
LONG_DOCS = TILE + 77
PREFIX_GRAMS = (8, 16, 17, 32, 33, 64, 65, 127)


def master_string(seed=11):
    """128 letters over 16 in which no bigram repeats: 127 distinct grams (a walk that never takes an edge twice)."""
    rng = np.random.default_rng(seed)
    used, s = set(), [0]
    while len(s) < 128:
        nxt = [int(c) for c in rng.permutation(16) if (s[-1], int(c)) not in used]
        # prefer a letter that still has many unused edges out of it, so that the walk does not strand
        nxt.sort(key=lambda c: sum((c, d) in used for d in range(16)))
        assert nxt, "the walk stranded: another seed"
        used.add((s[-1], nxt[0]))
        s.append(nxt[0])
    m = "".join(ALPHABET[c] for c in s)
    assert len({m[i:i + 2] for i in range(127)}) == 127
    return m


def long_word_corpus(seed=12):
    """LONG_DOCS documents: the master string with k = i mod 41 substituted letters (from the alphabet, or 'z')."""
    m = np.frombuffer(master_string().encode(), np.uint8)
    rng = np.random.default_rng(seed)
    texts = []
    letters = np.frombuffer((ALPHABET + "z").encode(), np.uint8)
    for i in range(LONG_DOCS):
        d = m.copy()
        k = i % 41
        if k:
            d[rng.choice(128, size=k, replace=False)] = letters[rng.integers(0, len(letters), k)]
        texts.append(d.tobytes().decode())
    return texts


def long_word_terms(side):
    """-> (accepted terms, the refused 129-letter term): the master string, its prefixes, the master string with a typo
    ('q' in the middle: two unknown grams), and the master string plus one letter whose last bigram the index knows."""
    m = master_string()
    typo = m[:60] + "q" + m[61:]
    terms = [m[:g + 1] for g in PREFIX_GRAMS] + [typo]
    extra = [c for c in ALPHABET if m[-1] + c not in m and side.columns.lookup(m[-1] + c) is not None]
    assert extra, "no known 128th gram"
    return terms, m + extra[0]


def long_word_specs(side):
    """Every accepted term at FUZZY 1 and 2: a materialised docid result, a docid page, SORT _score, a two-term query (the
    second term behind PUSH / POP) and an expression with FUZZY leaves."""
    terms, _ = long_word_terms(side)
    specs = []
    for i, t in enumerate(terms):
        other = terms[(i + 3) % len(terms)]
        for d in (1, 2):
            specs.append(FU.Spec("fuzzy", terms=[t], fuzzy=d, page=dict(limit=0, descending=False)))
            specs.append(FU.Spec("fuzzy", terms=[t], fuzzy=d, page=dict(limit=17)))
            specs.append(FU.Spec("fuzzy", terms=[t], fuzzy=d, page=dict(sort_score=True, limit=10)))
            specs.append(FU.Spec("fuzzy", terms=[terms[0], t], fuzzy=d, page=dict(limit=17, descending=False)))
            specs.append(FU.Spec("expr", expr=("or", ("and", t, ("not", other)), terms[0][:5]), fuzzy=d,
                                 page=dict(limit=0, descending=False)))
            specs.append(FU.Spec("expr", expr=("and", other, ("not", t)), fuzzy=d, page=dict(sort_score=True, limit=10)))
    return specs


# ---- B. nesting depth and program length -----------------------------------------------------------------------------------
DEPTHS = (4, 8, 31, 32, 33, 39, 40)
SHAPES = ("and-or", "not", "and-not")


def stack_depth(e):
    """The operand-stack depth of the tree's program: the first child of AND / OR is evaluated in the accumulator, every
    later child behind a PUSH; NOT pushes the universe."""
    if isinstance(e, str):
        return 0
    if e[0] == "not":
        return 1 + stack_depth(e[1])
    return max([stack_depth(e[1])] + [1 + stack_depth(k) for k in e[2:]])


def n_tokens(e):
    return 1 if isinstance(e, str) else 1 + sum(n_tokens(k) for k in e[1:])


def chain(side, shape, d):
    """A tree of stack depth d. The AND levels cycle through three dense grams and the OR levels through four mid grams, so
    that documents exist that hold every AND term and no OR term: for those the innermost term decides."""
    v = FU.vocabulary(side)
    ands, ors, bottom = v["dense"][:3], v["mid"][1:5], v["mid"][0]
    if shape == "not":
        e = v["words"][0]
        for _ in range(d):
            e = ("not", e)
        return e
    e = bottom
    for i in reversed(range(d)):
        if shape == "and-or":
            e = ("and", ands[(i // 2) % 3], e) if i % 2 == 0 else ("or", ors[(i // 2) % 4], e)
        else:
            e = ("and", ands[(i // 2) % 3], e) if i % 2 == 0 else ("not", e)
    return e


def halves_chain(d):
    """("or", a, ("and", b1, ("and", b2, ...))) of stack depth d over the lists-only threshold corpus: `a` has postings in
    the first tile alone and every b in the second alone. In the first tile the deep right side is empty and `a` decides —
    its presence is the bottom entry of tile_may_match's bit stack while 1 .. d - 1 entries lie above it."""
    e = GRAMS[d % 16]
    for i in reversed(range(1, d)):
        e = ("and", GRAMS[i % 16], e)
    return ("or", GRAMS[64], e)


def drop_innermost(e, unknown):
    """The tree without its innermost term: its parent AND / OR keeps the other child; under a NOT the empty set remains."""
    kid = e[-1]
    if isinstance(kid, str):
        if e[0] == "not":
            return ("not", unknown)
        return e[1] if len(e) == 3 else e[:-1]
    return e[:-1] + (drop_innermost(kid, unknown),)


def wide_trees(side, distinct=64):
    """-> (OR of 511 children over `distinct` sparse grams, AND of 511 children over three dense grams): 512 tokens."""
    v = FU.vocabulary(side)
    c = side.columns
    sizes = np.diff(c.offsets.astype(np.int64))
    sparse = [c.gram(int(g)).decode() for g in np.argsort(sizes, kind="stable") if b" " not in c.gram(int(g)) and sizes[g] >= 3]
    sparse = sparse[:distinct]
    assert len(sparse) == distinct
    return (("or",) + tuple(sparse[i % distinct] for i in range(511)),
            ("and",) + tuple(v["dense"][i % 3] for i in range(511)))


def tree_queries(tree, **kw):
    return [Query(expr=tree, **dict(page, **kw)) for page in FU.PAGES]


def check_tree_coverage(side, tree, chain_shape=True):
    """Every tree has a non-empty result smaller than the table; a chain has a document whose membership flips when the
    innermost term is dropped."""
    total = side.oracle_query(Query(expr=tree, limit=0, descending=False))[0]
    assert 0 < total < side.columns.n_docs, (total, tree)
    if chain_shape:
        v = FU.vocabulary(side)
        without = drop_innermost(tree, v["unknown"][0])
        a = side.oracle_query(Query(expr=tree, limit=0, descending=False))[1]
        b = side.oracle_query(Query(expr=without, limit=0, descending=False))[1]
        assert set(a.tolist()) != set(b.tolist()), tree
    return total
