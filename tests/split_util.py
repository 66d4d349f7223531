"""Host-side reference for find_smems_split: cut a read at its breaks and ask the CPU oracle for each segment's SMEMs
(BWA traversal), shifted to positions in the whole read.  A break is a code > 3 or a base the reference lacks."""
import numpy as np


def present_mask(ref_codes):
    """Bit b set: base b occurs in the reference."""
    m = 0
    for b in np.unique(np.asarray(ref_codes, np.uint8)):
        m |= 1 << int(b)
    return m


def segments(read, present=0xF):
    """[(start, length)] of the maximal runs of positions that are not breaks, in read order."""
    read = np.asarray(read, np.uint8)
    good = (read < 4) & ((present >> np.minimum(read, 3).astype(np.int64)) & 1).astype(bool)
    out, i, n = [], 0, read.size
    while i < n:
        if not good[i]:
            i += 1
            continue
        j = i
        while j < n and good[j]:
            j += 1
        out.append((i, j - i))
        i = j
    return out


def split_rows(oracle, read, min_len=1, present=0xF):
    """int32 [S, 4] (start, end, lo, hi): every segment's oracle rows, segment offset added, segments in read order."""
    read = np.asarray(read, np.uint8)
    parts = []
    for s, l in segments(read, present):
        rc, rows = oracle.find_smems("bwa", read[s:s + l], min_len)
        assert rc >= 0, (rc, s, l)
        rows = rows.copy()
        rows[:, :2] += s
        parts.append(rows)
    return np.concatenate(parts).astype(np.int32) if parts else np.zeros((0, 4), np.int32)
