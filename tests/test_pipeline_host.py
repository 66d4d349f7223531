"""CPU: the composed host pipeline of tests/pipeline_util.py -- the stage brute forces chained from the reads to the SAM bytes --
on the two simulated batches, against checks that share no code with it: cigar_util.check_result and select_util.check_result,
which hold whatever the tie-breaks, check_sam on the text with all five tags, the scenario assertions that make the batches
worth having, the truth table of the simulator, and corrupted text that check_sam must refuse.  tests/test_pipeline_gpu.py
compares the device with the same host runs."""
import re

import numpy as np
import pytest

import cigar_util as CG
import pair_util as PU
import pipeline_util as P
import select_util as SU

RUNS = [("library", "plain"), ("library", "rescue"), ("library", "estimate"), ("hard", "plain"), ("hard", "rescue"), ("hard", "any")]


def _quals(b):
    return [bytes(b.quals[b.read_offsets[r]:b.read_offsets[r + 1]]) for r in range(len(b.truth))]


def _text(name, option_set, tags=P.ALL_TAGS):
    T, b = P.batch(name)
    run = P.host_run(name, option_set)
    return P.made((name, option_set, "text", tags), lambda: P.host_sam_text(run.result, T, P.TABLE, (b.bases, b.read_offsets), b.names,
                                                                             P.CONTIG_NAMES, b.quals, tags))


@pytest.mark.parametrize("name, option_set", RUNS)
def test_composition_against_independent_checks(name, option_set):
    T, b = P.batch(name)
    run = P.host_run(name, option_set)
    last = run.last
    n = CG.check_result(last["batch"], run.align_params, T, last["aln"], run.cigars, last["select"]["sel"])
    assert n == run.result[0].shape[0] > len(b.truth) // 2          # every record has a CIGAR that scores what its alignment says
    for st in (run.first, run.second):
        if st is not None:
            SU.check_result(st["select_batch"], SU.DEFAULTS._replace(**b.options.get("select_options", {})), st["select"])
    assert len(run.result) == 7 + P.OPTION_SETS[option_set]["rescue"] + ("insert_size" in P.OPTION_SETS[option_set])
    text, line_offsets, totals = _text(name, option_set)
    lines = P.check_sam(text, line_offsets, T, P.TABLE, P.CONTIG_NAMES, b.reads(), b.names, run.align_params, quals=_quals(b))
    assert lines == totals[0] == run.result[0].shape[0] + int((np.diff(run.result[1]) == 0).sum())


def test_the_hard_batch_holds_its_scenarios():
    """Counts on the host result (42 pairs, rescue on): the widest read has 24 candidate chains (> GENIE_SELECT_LANE_MAX = 8) and
    the widest pair 13 x 13 = 169 record combinations (> GENIE_PAIR_LANE_MAX = 64), 91 of them concordant; 15 records carry an S,
    4 an I, 4 a D and 2 an X; 4 records are supplementary (the chimeric mates and the mates across the boundary of a and b); 17
    pairs are proper after the first pass and 19 after rescue, the two more being the planted diverged mates; 14 mates stay
    unmapped: the 4 unreachable ones, the 6 random ones, the 2 short and the 2 empty ones."""
    T, b = P.batch("hard")
    labels = {t.label for t in b.truth}
    assert labels == {"dup", "tandem", "overhang", "boundary", "chimeric", "deletion", "insertion", "n_run", "short_insert", "same_start",
                      "rf", "same_strand", "two_contigs", "far", "random_mate", "random_both", "short_mate", "empty_mate", "diverged",
                      "unreachable"}
    for label in labels:                                             # every scenario with its affected mate on either strand
        mates = [t for r, t in enumerate(b.truth) if t.label == label and (t.contig < 0 if label == "empty_mate" else r % 2 == 1)]
        assert len(b.pairs_of(label)) >= 2 and {t.strand for t in mates} == {0, 1}, (label, mates)
    plain, run = P.host_run("hard", "plain"), P.host_run("hard", "rescue")
    records, so, offs, cigar, info, pairs, sam = run.result[:7]
    sel = run.last["select"]
    assert sel["counts"][:, 0].max() > P.SELECT_LANE_MAX             # the wide read
    pb = run.last["pair_batch"]
    R = records.shape[0]
    combos = [len(PU.candidates(pb, 2 * k, R, pb["klass"].shape[0])) * len(PU.candidates(pb, 2 * k + 1, R, pb["klass"].shape[0]))
              for k in range(len(pairs))]
    wide = int(np.argmax(combos))
    assert combos[wide] > P.PAIR_LANE_MAX and wide in b.pairs_of("tandem") and pairs[wide, 6] > P.PAIR_LANE_MAX      # the wide pair
    texts = CG.cigar_strings(offs, cigar)
    for letter in "SIDX":
        assert sum(letter in t for t in texts) >= 2, letter
    split = b.pairs_of("chimeric") + b.pairs_of("boundary")          # the mates that two contigs share
    assert (records[:, 2] == 1).sum() >= 2 and all(int(records[j, 0]) // 2 in split for j in np.flatnonzero(records[:, 2] == 1))
    assert any("N" in s for s in b.strings())
    # rescue: the planted diverged mates become proper, the unreachable ones stay without a record
    proper0, proper = plain.result[5][:, 2] & 1, pairs[:, 2] & 1
    for k in b.pairs_of("diverged"):
        assert not proper0[k] and proper[k] and np.diff(plain.result[1])[2 * k + 1] == 0 and np.diff(so)[2 * k + 1] == 1
    assert proper.sum() == proper0.sum() + len(b.pairs_of("diverged")) and not (proper0 & ~proper).any()
    windows = run.result[7][0]
    for k in b.pairs_of("unreachable"):
        assert np.diff(so)[2 * k + 1] == 0 and not proper[k] and (windows[4 * k + 2:4 * k + 4, 1] > windows[4 * k + 2:4 * k + 4, 0]).any()
    for r, t in enumerate(b.truth):
        if t.contig < 0 or t.label == "short_mate" and r % 2:
            assert so[r + 1] == so[r], (r, t)
    # an overhang is clipped, never aligned across the boundary; check_sam holds every record inside its contig
    for k in b.pairs_of("overhang"):
        j = int(so[2 * k + 1])
        assert "40S" in texts[j] and records[j, 5] - 1 + records[j, 6] <= np.diff(P.TABLE)[records[j, 4]]
    for k in b.pairs_of("boundary"):                                 # the reference itself across a and b: 60 bases on either side
        rows = records[so[2 * k + 1]:so[2 * k + 2]]
        assert rows[:, 2].tolist() == [0, 1] and rows[:, 4].tolist() == [0, 1] and rows[:, 6].tolist() == [60, 60]
        assert rows[0, 5] - 1 + 60 == P.TABLE[1] and rows[1, 5] == 1
    print("hard:", dict(widest_read=int(sel["counts"][:, 0].max()), widest_pair=combos[wide], concordant=int(pairs[wide, 6]),
                        **{x: sum(x in t for t in texts) for x in "SIDX"}, supplementary=int((records[:, 2] == 1).sum()),
                        proper_first=int(proper0.sum()), proper_rescue=int(proper.sum()), unmapped=int((np.diff(so) == 0).sum())))


def test_the_library_batch_holds_its_scenarios():
    """Counts on the host result: 48 pairs, mate 0 forward in 24; 38 proper after the first pass, 48 after rescue with and without
    the estimate (all 9 diverged mates found); the estimate is FR from 28 samples with mean 373 and window [0, 861], around the
    simulated inserts of 250 to 500."""
    T, b = P.batch("library")
    assert sum(b.truth[2 * k].strand == 0 for k in range(len(b.truth) // 2)) == len(b.truth) // 4
    diverged = b.pairs_of("diverged")
    assert len(diverged) >= len(b.truth) // 2 // 5
    plain, rescue, est = (P.host_run("library", s) for s in ("plain", "rescue", "estimate"))
    for run in (rescue, est):
        proper0, proper = plain.result[5][:, 2] & 1, run.result[5][:, 2] & 1
        for k in diverged:
            assert not proper0[k] and proper[k], k
        assert proper.sum() >= proper0.sum() + len(diverged)
    e = est.result[-1]
    lo, hi = b.insert_range
    assert e.estimated and e.orient == P.ORIENT["fr"] and lo <= e.isize_mean <= hi and e.isize_min <= lo and hi <= e.isize_max
    assert e.stats[0][0] >= 25 and e == est.est
    texts = CG.cigar_strings(est.result[2], est.result[3])
    for letter in "IDX":
        assert sum(letter in t for t in texts) >= 10, letter
    print("library:", dict(proper_first=int((plain.result[5][:, 2] & 1).sum()), proper_rescue=int((rescue.result[5][:, 2] & 1).sum()),
                           proper_estimate=int((est.result[5][:, 2] & 1).sum()), diverged=len(diverged), estimate=e[:5],
                           samples=e.stats[0][0]))


def _recovered(run, r, t):
    records, so = run.result[0], run.result[1]
    if so[r + 1] == so[r]:
        return False
    j = int(so[r])                                                   # the read's primary record comes first
    lo = int(records[j, 5]) - 1
    here = records[j, 2] == 0 and records[j, 4] == t.contig and records[j, 3] == t.strand
    return here and lo < t.end and t.start < lo + int(records[j, 6])


@pytest.mark.parametrize("name, option_set", RUNS)
def test_truth_recovery(name, option_set):
    """Every recoverable mate is recovered: its primary record is on the true contig and strand and overlaps the true interval.
    Recoverable by construction: an exact run of at least minimum_length bases between two simulated edits and no overlap with
    the planted repeats; with rescue also the diverged mates planted inside a window.  library: of 96 mates 11 are left out with
    rescue (10 touch a planted repeat, 1 kept no run of 19 bases between its edits) and 20 without it (the 9 diverged ones more);
    hard: of 84 mates 22 with rescue (6 in the repeats, 8 random or empty, 2 short, 2 across the boundary, 4 unreachable) and 24
    without (the 2 diverged ones more)."""
    T, b = P.batch(name)
    run = P.host_run(name, option_set)
    rescue = option_set != "plain"
    recoverable = [r for r, t in enumerate(b.truth) if t.recoverable or (rescue and t.rescuable)]
    missed = [(r, b.truth[r]) for r in recoverable if not _recovered(run, r, b.truth[r])]
    assert not missed, missed[:4]
    left_out = len(b.truth) - len(recoverable)
    print(name, option_set, "mates", len(b.truth), "not recoverable", left_out)
    if name == "library":
        assert 4 * left_out <= len(b.truth)


# ------------------------------------------------------------------ the checker can fail
def _lines(text, line_offsets):
    raw = bytes(text)
    return [raw[a:b] for a, b in zip(line_offsets[:-1], line_offsets[1:])]


def _join(lines):
    off = np.zeros(len(lines) + 1, np.int64)
    off[1:] = np.cumsum([len(x) for x in lines])
    return b"".join(lines), off


def _set(line, column, edit):
    cols = line[:-1].split(b"\t")
    cols[column] = edit(cols[column])
    return b"\t".join(cols) + b"\n"


def _tag(line, key):
    return next(k for k, c in enumerate(line[:-1].split(b"\t")) if k >= 11 and c.startswith(key))


def _bump(value):
    head, number = value.rsplit(b":", 1) if b":" in value else (None, value)
    out = b"%d" % (int(number) + 1)
    return out if head is None else head + b":" + out


CORRUPTIONS = {
    "tlen_sign": (lambda c: int(c[8]) != 0 and not int(c[1]) & 0x900, lambda ln: _set(ln, 8, lambda v: b"%d" % -int(v))),
    "md_letter": (lambda c: any(x.startswith(b"MD:Z:") and re.search(rb"\d[ACGT]\d", x) for x in c[11:]),
                  lambda ln: _set(ln, _tag(ln, b"MD"), lambda v: re.sub(rb"(\d)([ACGT])(\d)", lambda m: m.group(1) + b"ACGT"[
                      (b"ACGT".index(m.group(2)) + 1) % 4:][:1] + m.group(3), v, count=1))),
    "nm": (lambda c: not int(c[1]) & 4, lambda ln: _set(ln, _tag(ln, b"NM"), _bump)),
    "as": (lambda c: not int(c[1]) & 4, lambda ln: _set(ln, _tag(ln, b"AS"), _bump)),
    "first_last": (lambda c: True, lambda ln: _set(ln, 1, lambda v: b"%d" % (int(v) ^ 0xC0))),
    "pnext": (lambda c: not int(c[1]) & 0xC, lambda ln: _set(ln, 7, _bump)),
    "cigar_length": (lambda c: not int(c[1]) & 4,
                     lambda ln: _set(ln, 5, lambda v: re.sub(rb"^\d+", lambda m: b"%d" % (int(m.group()) + 1), v))),
    "mapq": (lambda c: not int(c[1]) & 4, lambda ln: _set(ln, 4, lambda v: b"61")),
    "mc": (lambda c: any(x.startswith(b"MC:Z:") for x in c[11:]), lambda ln: _set(ln, _tag(ln, b"MC"), lambda v: v + b"1=")),
    "mq": (lambda c: any(x.startswith(b"MQ:i:") for x in c[11:]), lambda ln: _set(ln, _tag(ln, b"MQ"), _bump)),
    "across_the_boundary": (lambda c: c[2] == b"a" and c[5] == b"140=" and not int(c[1]) & 4, lambda ln: _set(ln, 3, lambda v: b"3200")),
}


@pytest.mark.parametrize("what", sorted(CORRUPTIONS))
def test_the_checker_can_fail(what):
    """One field of one line of the host text corrupted per rule: check_sam must raise on each, and on every line the
    corruption applies to when it is made there alone (the first, a middle and the last such line are tried)."""
    T, b = P.batch("hard")
    run = P.host_run("hard", "rescue")
    text, line_offsets, _ = _text("hard", "rescue")
    lines = _lines(text, line_offsets)

    def check(text, offsets):
        return P.check_sam(text, offsets, T, P.TABLE, P.CONTIG_NAMES, b.reads(), b.names, run.align_params, quals=_quals(b))
    assert check(*_join(lines)) == len(lines)                        # put together again unchanged, the text passes
    applies, edit = CORRUPTIONS[what]
    at = [k for k, ln in enumerate(lines) if applies(ln[:-1].split(b"\t"))]
    assert at, what
    for k in sorted({at[0], at[len(at) // 2], at[-1]}):
        bad = list(lines)
        bad[k] = edit(lines[k])
        assert bad[k] != lines[k], (what, lines[k])
        with pytest.raises(AssertionError):
            check(*_join(bad))
