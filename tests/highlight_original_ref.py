"""The checker for HIGHLIGHT over original texts: a line-by-line Python restatement of Highlighter::GenerateOriginal.

Every function names the lines it restates (paths relative to the reference tree). Texts and terms are `bytes`, positions
are code points. The segmentation of the original (SegmentOriginalText, src/query/highlighter.cpp:31-75: ICU character
breaks, else one segment per parsed character) and the normalizer are INPUTS here: a case gives the original's segments as
(bytes of the segment, the segment's normalized bytes) in text order, and the normalized form of the whole text. The rest
(windows, merge, clamp, rendering) is tests/highlight_ref.py. Nothing here is shared with the code under test:
tests/test_highlight_original_cpu.py first pins this file on tests/golden/highlight_original.json (the reference's own
unit-test vectors), then compares the library against it.
"""
import highlight_ref as R

ORIG_NONE, ORIG_IDENTITY, ORIG_MAPPED, ORIG_UNMAPPABLE = 0, 1, 2, 3
HL_ORIGINAL = 8


def remove_overlapping_match_positions(positions):
    """RemoveOverlappingMatchPositions, highlighter.cpp:227-248 (the sort-based original)."""
    positions = sorted(positions, key=lambda p: (p[0], -p[1]))          # :232-237
    deduped = []
    for pos in positions:                                               # :241-246
        if deduped and pos[0] < deduped[-1][1]:
            continue
        deduped.append(pos)
    return deduped


def segment_map(segments):
    """The loop of GenerateOriginal, highlighter.cpp:328-336: every code point of a segment's normalized piece maps to the
    segment's (cp_start, cp_end). segments: [(original bytes of the segment, its normalized bytes)]."""
    normalized_to_original = []
    cp_start = 0
    for piece, normalized_piece in segments:
        cp_end = cp_start + R.count_code_points(piece)                  # :50 / :70 (one per parsed character)
        for _ in range(R.count_code_points(normalized_piece)):          # :332-335
            normalized_to_original.append((cp_start, cp_end))
        cp_start = cp_end
    return normalized_to_original


def generate_original(original, normalized_text, segments, terms, snippet_length=R.DEFAULT_SNIPPET_LENGTH,
                      max_fragments=R.DEFAULT_MAX_FRAGMENTS, open_tag=R.DEFAULT_OPEN, close_tag=R.DEFAULT_CLOSE):
    """Highlighter::GenerateOriginal, highlighter.cpp:311-356. normalized_text = normalizer(original)."""
    if len(original) == 0:                                              # :315-319
        return b""
    if not terms:                                                       # :323-325
        return R.generate_with_positions(original, [], snippet_length, max_fragments, open_tag, close_tag)
    normalized_to_original = segment_map(segments)                      # :328-336
    if len(normalized_to_original) != R.count_code_points(normalized_text):   # :342-344
        return R.generate_with_positions(original, [], snippet_length, max_fragments, open_tag, close_tag)
    normalized_matches = R.find_match_positions(normalized_text, terms)  # :346
    original_matches = []
    for start, end in normalized_matches:                               # :349-354
        if start >= len(normalized_to_original) or end == 0 or end > len(normalized_to_original):
            continue
        original_matches.append((normalized_to_original[start][0], normalized_to_original[end - 1][1]))
    return R.generate_with_positions(original, remove_overlapping_match_positions(original_matches), snippet_length,
                                     max_fragments, open_tag, close_tag)   # :355


def translated_matches(normalized_text, segments, terms):
    """The ranges GenerateOriginal hands to RemoveOverlappingMatchPositions (:346-354), in the order it builds them."""
    m = segment_map(segments)
    return [(m[s][0], m[e - 1][1]) for s, e in R.find_match_positions(normalized_text, terms)
            if not (s >= len(m) or e == 0 or e > len(m))]


def split_characters(text):
    """SegmentOriginalText's per-character branch (:62-74) on valid UTF-8: one segment per character."""
    out, i = [], 0
    while i < len(text):
        c = text[i]
        n = 1 if c < 0x80 else 2 if (c & 0xE0) == 0xC0 else 3 if (c & 0xF0) == 0xE0 else 4
        out.append(text[i:i + n])
        i += n
    return out


def build_map(original, normalized_text, segments):
    """What a host hands to mgx_index_attach_original_text for one document: (kind, [(cp_start, cp_end)] or None).
    IDENTITY when pair i is (i, i + 1) for every normalized code point and the original has as many code points."""
    m = segment_map(segments)
    if len(m) != R.count_code_points(normalized_text):
        return ORIG_UNMAPPABLE, None
    if len(m) == R.count_code_points(original) and all(p == (i, i + 1) for i, p in enumerate(m)):
        return ORIG_IDENTITY, None
    return ORIG_MAPPED, m
