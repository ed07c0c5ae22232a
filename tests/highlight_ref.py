"""The checker for HIGHLIGHT: a line-by-line Python restatement of the reference's highlighter.

Every function names the lines it restates (paths relative to the reference tree). Texts and terms are `bytes`, as the
reference's std::string / std::string_view are; positions are code points. Nothing here is shared with the code under
test: tests/test_highlight_cpu.py first pins this file on tests/golden/highlight.json (the reference's own unit-test
vectors), then compares the library against it.
"""

DEFAULT_OPEN = b"<em>"        # src/query/query_parser.h:158-163 (HighlightOptions)
DEFAULT_CLOSE = b"</em>"
DEFAULT_SNIPPET_LENGTH = 100
DEFAULT_MAX_FRAGMENTS = 3


def count_code_points(b):
    """mygram::utils::CountCodePoints, src/utils/string_utils.cpp:655-669: the bytes that are not 10xxxxxx."""
    return sum(1 for c in b if (c & 0xC0) != 0x80)


def cp_to_byte(text, cp_offset):
    """CpToByte, src/query/highlighter.cpp:78-93 (valid UTF-8: every TryParseUtf8Char succeeds)."""
    byte_pos = 0
    cp_count = 0
    n = len(text)
    while byte_pos < n and cp_count < cp_offset:
        c = text[byte_pos]
        length = 1 if c < 0x80 else 2 if (c & 0xE0) == 0xC0 else 3 if (c & 0xF0) == 0xE0 else 4
        byte_pos += length
        cp_count += 1
    return byte_pos


def substr_by_code_points(text, cp_start, cp_end):
    """SubstrByCodePoints, highlighter.cpp:102-112."""
    byte_start = min(cp_to_byte(text, cp_start), len(text))
    byte_end = min(cp_to_byte(text, cp_end), len(text))
    return text[byte_start:byte_end] if byte_end > byte_start else b""


def merge_windows(windows):
    """MergeWindows, highlighter.cpp:115-131."""
    if not windows:
        return []
    windows = sorted(windows)
    merged = [list(windows[0])]
    for first, second in windows[1:]:
        last = merged[-1]
        if first <= last[1]:
            last[1] = max(last[1], second)
        else:
            merged.append([first, second])
    return merged


def clamp_windows(windows, matches, snippet_length, total_cp):
    """ClampWindows, highlighter.cpp:138-158 (in place)."""
    for w in windows:
        win_start, win_end = w
        if win_end - win_start <= snippet_length:
            continue
        first_match = next((m for m in matches if m[1] > win_start and m[0] < win_end), None)
        anchor = first_match[0] if first_match is not None else win_start
        left_context = snippet_length // 2
        clamped_start = anchor - left_context if anchor > left_context else 0
        if clamped_start + snippet_length > total_cp:
            clamped_start = total_cp - snippet_length if total_cp > snippet_length else 0
        win_start = max(win_start, clamped_start)
        win_end = min(win_end, win_start + snippet_length)
        w[0], w[1] = win_start, win_end


def generate_with_positions(text, match_positions, snippet_length, max_fragments, open_tag, close_tag):
    """GenerateWithPositions, highlighter.cpp:160-225."""
    total_cp = count_code_points(text)
    if not match_positions:                                             # :165-172
        snippet_end = min(total_cp, snippet_length)
        snippet = substr_by_code_points(text, 0, snippet_end)
        if snippet_end < total_cp:
            snippet += b"..."
        return snippet
    context_radius = snippet_length // 2                                # :174-180
    windows = []
    for start, end in match_positions:
        win_start = start - context_radius if start > context_radius else 0
        win_end = min(total_cp, end + context_radius)
        windows.append((win_start, win_end))
    merged = merge_windows(windows)                                     # :182-186
    clamp_windows(merged, match_positions, snippet_length, total_cp)
    if len(merged) > max_fragments:
        merged = merged[:max_fragments]
    snippet = b""                                                       # :188-222
    for wi, (win_start, win_end) in enumerate(merged):
        if wi > 0:
            snippet += b"..."
        if win_start > 0 and wi == 0:
            snippet += b"..."
        cursor = win_start
        for m_start, m_end in match_positions:
            if m_end <= win_start or m_start >= win_end:
                continue
            if m_start > cursor:
                snippet += substr_by_code_points(text, cursor, m_start)
            clipped_start = max(m_start, win_start)
            clipped_end = min(m_end, win_end)
            if clipped_start >= clipped_end:
                continue
            snippet += open_tag
            snippet += substr_by_code_points(text, clipped_start, clipped_end)
            snippet += close_tag
            cursor = clipped_end
        if cursor < win_end:
            snippet += substr_by_code_points(text, cursor, win_end)
        if win_end < total_cp and wi == len(merged) - 1:
            snippet += b"..."
    return snippet


def remove_overlapping_match_positions(positions):
    """RemoveOverlappingMatchPositions, highlighter.cpp:227-248."""
    positions = sorted(positions, key=lambda p: (p[0], -p[1]))
    deduped = []
    for pos in positions:
        if deduped and pos[0] < deduped[-1][1]:
            continue
        deduped.append(pos)
    return deduped


def find_match_positions(text, terms):
    """Highlighter::FindMatchPositions, highlighter.cpp:252-297."""
    positions = []
    for term in terms:
        if len(term) == 0:                                              # :257-259
            continue
        if len(term) > len(text):                                       # :260-262
            continue
        term_cp_count = count_code_points(term)
        prev_byte_pos = 0
        prev_cp_pos = 0
        search_start = 0
        while search_start <= len(text) - len(term):                    # :277-293
            byte_pos = text.find(term, search_start)
            if byte_pos < 0:
                break
            prev_cp_pos += count_code_points(text[prev_byte_pos:byte_pos])
            prev_byte_pos = byte_pos
            positions.append((prev_cp_pos, prev_cp_pos + term_cp_count))
            search_start = byte_pos + len(term)
    return remove_overlapping_match_positions(positions)


def generate(text, terms, snippet_length=DEFAULT_SNIPPET_LENGTH, max_fragments=DEFAULT_MAX_FRAGMENTS,
             open_tag=DEFAULT_OPEN, close_tag=DEFAULT_CLOSE):
    """Highlighter::Generate, highlighter.cpp:299-309."""
    if len(text) == 0:
        return b""
    return generate_with_positions(text, find_match_positions(text, terms), snippet_length, max_fragments, open_tag,
                                   close_tag)


_SPACES = b" \t\n\v\f\r"  # what `std::istringstream >> piece` skips in the "C" locale


def build_highlight_terms(search_terms, normalize=None):
    """search_pipeline::BuildHighlightTerms, src/server/search_pipeline.cpp:712-745, without the synonym branch
    (:733-741): normalize, skip empty terms, add the whitespace-separated pieces, sort and dedupe."""
    terms = []
    for term in search_terms:
        normalized = normalize(term) if normalize is not None else term   # :718
        if len(normalized) == 0:                                          # :719-721
            continue
        terms.append(normalized)
        piece = b""
        for c in normalized + b" ":                                       # :724-730
            if bytes([c]) in _SPACES:
                if piece and piece != normalized:
                    terms.append(piece)
                piece = b""
            else:
                piece += bytes([c])
    return sorted(set(terms))                                             # :743 (DeduplicateSorted)
