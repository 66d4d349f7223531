"""Batches wide enough for the batch-level loops of genie_chain_mems, genie_align_chains and genie_chain_cigars to go round more
than twice (tests/test_wide_map_host.py, tests/test_wide_map_gpu.py), and their expected results.  G is the number of waves of
a full grid: 16 per CU (4 blocks of 4 waves).

The brute forces of tests/align_util.py and tests/cigar_util.py cost milliseconds per chain, so the wide align / CIGAR batch is
drawn from T templates (T prime): a template is one strand-read with 0 to 3 chains (with S == 2: one read, the chains on one
of its strands).  The brute force runs once, on the batch of the T templates, and the wide expectation is put together from its
per-chain pieces: aln rows as they are; per chain the ops, info (column 0 set to the wide chain index) and direction need;
offsets, flags 8 and totals recomputed as running sums.  Nothing here comes from the library under test."""
import numpy as np

import align_util as AU
import chain_util as CH
import cigar_util as CU

N_REF = 1 << 14
TABLE = np.asarray([0, 3000, 9000, N_REF], np.int64)
PRM = AU.Params(1, 4, 6, 1, 40, 400, 5)      # 81 diagonals (2 chunks) when B == A, 481 (8 chunks) when |B - A| = 400
N_TEMPLATES = 251
SCAN = 1024                                  # kScanBlock: the one-block loops
EXT = (0, 1, 5, 64, 65, 130)
EXT_P = (0.25, 0.2, 0.25, 0.1, 0.1, 0.1)
KINDS = ("single", "equal", "wide_del", "wide_ins", "closed_a", "closed_b", "multi", "trivial", "equal", "multi", "single", "closed_a",
         "equal", "multi", "trivial", "closed_b")


def reference():
    return np.random.default_rng(7).integers(0, 4, N_REF).astype(np.uint8)


def grid_waves(n_cus):
    return 16 * n_cus


# ------------------------------------------------------------------ templates
def chain(rng, T, spec, left, right, lo=0, hi=None, rate=0.1, overlap=0.0, dup=0.0, t0=None):
    """A strand-read with one chain inside the reference window [lo, hi): AU.synth_chain, then some members made longer so that
    they overlap the next one (trimmed; the read is given the reference's bases there), and some rows put in that start where
    the next member starts in the reference (skipped)."""
    hi = len(T) if hi is None else hi
    span = sum(l + B for l, A, B in spec[:-1]) + spec[-1][0]
    if t0 is None:
        t0 = int(rng.integers(lo + left + 45, max(lo + left + 46, hi - span - right - 45)))
    Q, rows = AU.synth_chain(rng, T, t0, spec, left, right, rate)
    out = []
    for k, (s, e, pos) in enumerate(rows):
        if k + 1 < len(rows) and rng.random() < overlap:
            e = min(e + int(rng.integers(1, 6)), rows[k + 1][1] - 1, len(Q))
            upto = min(e, rows[k + 1][0])                            # what is left of it after trimming is a true match, so that
            Q[s:upto] = T[pos - 1:pos - 1 + upto - s]                # CU.check_chain holds on the result
        if k and rng.random() < dup and s - 1 > rows[k - 1][0]:
            out.append((s - 1, min(s + 2, len(Q)), pos))
        out.append((s, e, pos))
    return Q, out


def _one_chain(rng, T, kind, lo, hi, near, outer=(True, True)):
    """(Q, rows) of one chain of the given kind; near: next to the window's start, so that the left extension meets it; outer:
    whether its left / right end is an end of the strand-read (between two chains of a read the ends stay short: the brute
    force runs every extension over the rest of the read)."""
    m = lambda: int(rng.integers(6, 13))      # noqa: E731
    left, right = (int(rng.choice(EXT, p=EXT_P)) if o else int(rng.choice(EXT[:3])) for o in outer)
    overlap = dup = 0.0
    if kind == "single":
        spec = [(m(), 0, 0)]
    elif kind == "trivial":                                          # the whole read is the member: need 0
        spec, left, right = [(m() + 20, 0, 0)], 0, 0
    elif kind == "equal":
        A = int(rng.integers(1, 31))
        spec = [(m(), A, A), (m(), 0, 0)]
    elif kind == "wide_del":
        A = int(rng.integers(1, 7))
        spec = [(m(), A, A + int(rng.integers(392, 401))), (m(), 0, 0)]
    elif kind == "wide_ins":
        B = int(rng.integers(1, 7))
        spec = [(m(), B + int(rng.integers(392, 401)), B), (m(), 0, 0)]
    elif kind == "closed_a":
        spec = [(m(), 0, int(rng.integers(1, 21))), (m(), 0, 0)]
    elif kind == "closed_b":
        spec = [(m(), int(rng.integers(1, 21)), 0), (m(), 0, 0)]
    elif kind == "skip":                                             # |B - A| > max_indel behind the first member
        A = int(rng.integers(0, 5))
        spec = [(m(), A, A + int(rng.integers(401, 420))), (m(), 2, 3), (m(), 0, 0)]
    else:
        assert kind == "multi"
        spec = [(m(), int(rng.integers(0, 9)), int(rng.integers(0, 9))) for _ in range(int(rng.integers(3, 6)))]
        overlap, dup = 0.4, 0.3
    Q, rows = chain(rng, T, spec, left, right, lo, hi, rate=float(rng.choice((0.1, 0.25))), overlap=overlap, dup=dup,
                     t0=lo + 3 if near else None)
    if kind in ("equal", "multi") and rng.random() < 0.3:            # breaks (code 4) in gaps and extensions, not in members
        free = [q for q in range(len(Q)) if not any(s <= q < e for s, e, _ in rows)]
        if free:
            Q = Q.copy()
            Q[rng.choice(free, min(2, len(free)), replace=False)] = 4
    return Q, rows


def templates(T, table, seed, count=N_TEMPLATES):
    """count strand-reads (Q, [(rows, contig), ...]) with 0 to 3 chains; about 1 chain in 40 is skipped by the aligner.  The
    chains of one strand-read lie one behind the other in the read."""
    rng = np.random.default_rng(seed)
    out, n_chain = [], 0
    for t in range(count):
        n = int(rng.choice(4, p=(0.1, 0.45, 0.3, 0.15)))
        if n == 0:
            out.append((rng.integers(0, 4, int(rng.integers(20, 60))).astype(np.uint8), []))
            continue
        Qs, chs, shift = [], [], 0
        for k in range(n):
            kind = "skip" if n_chain % 40 == 17 else KINDS[n_chain % len(KINDS)]
            if kind == "wide_ins" and k:                             # 400 bases of the read: alone in the next template
                break
            n_chain += 1
            g = 0 if table is None else int(rng.integers(0, len(table) - 1))
            lo, hi = (0, len(T)) if table is None else (int(table[g]), int(table[g + 1]))
            Q, rows = _one_chain(rng, T, kind, lo, hi, near=table is not None and rng.random() < 0.3, outer=(k == 0, k == n - 1))
            chs.append(([(s + shift, e + shift, pos) for s, e, pos in rows], g))
            Qs.append(Q)
            shift += len(Q)
            if kind == "wide_ins":
                break
        out.append((np.concatenate(Qs), chs))
    return out


def _units(tmpl, t, S):
    """The units of template t: one with S == 1; with S == 2 the two strands of its read, the chains on strand t % 2."""
    Q, chs = tmpl[t]
    if S == 1:
        return [(Q, chs)]
    return [(AU.revcomp(Q), []), (Q, chs)] if t % 2 else [(Q, chs), (AU.revcomp(Q), [])]


def template_batch(tmpl, S):
    return AU.make_batch([u for t in range(len(tmpl)) for u in _units(tmpl, t, S)], S)


# ------------------------------------------------------------------ the draw
def draw(seed, n_templates, counts, min_chains, min_slots, apart):
    """Template ids, one per slot (a unit, or a read with S == 2), until there are more than min_slots slots and they hold more
    than min_chains chains; slots i and i + d hold different templates for every d in `apart`."""
    rng = np.random.default_rng(seed)
    out, chains = [], 0
    while chains <= min_chains or len(out) <= min_slots:
        i = len(out)
        banned = {out[i - d] for d in apart if i - d >= 0}
        t = int(rng.integers(0, n_templates))
        while t in banned:
            t = int(rng.integers(0, n_templates))
        out.append(t)
        chains += int(counts[t])
    return np.asarray(out, np.int64)


class Wide:
    """A wide batch: b the batch dict of AU.make_batch, slots the template of every slot, tb the batch of the templates,
    tchain the template chain behind every chain of b."""

    def __init__(self, tmpl, S, table, slots, tb=None):
        self.tmpl, self.S, self.table, self.slots = tmpl, S, table, np.asarray(slots, np.int64)
        self.tb = template_batch(tmpl, S) if tb is None else tb
        per = np.add.reduceat(np.diff(self.tb["chain_offsets"]), np.arange(0, S * len(tmpl), S))      # chains per template
        first = self.tb["chain_offsets"][::S][:-1]
        self.per, self.first = per.astype(np.int64), np.asarray(first, np.int64)
        self.b = AU.make_batch([u for t in self.slots.tolist() for u in _units(tmpl, t, S)], S)
        n = self.per[self.slots]
        start = np.repeat(self.first[self.slots], n)
        inside = np.arange(int(n.sum())) - np.repeat(np.cumsum(n) - n, n)
        self.tchain = start + inside
        assert self.tchain.size == int(self.b["chain_offsets"][-1])

    def cut(self, lo, hi):
        """The batch of the slots [lo, hi) alone."""
        return Wide(self.tmpl, self.S, self.table, self.slots[lo:hi], self.tb)


def wide_batch(tmpl, S, table, seed, G):
    """More than 2 G + 300 units and more than 2.5 G + 300 chains (one chain in six needs no direction storage or is skipped,
    and more than 2 G should need some); units u, u + G, u + 2 G and u + 1024 hold different templates (with S == 2 the reads do)."""
    tb = template_batch(tmpl, S)
    per = np.add.reduceat(np.diff(tb["chain_offsets"]), np.arange(0, S * len(tmpl), S))
    apart = sorted({G // S, 2 * G // S, SCAN // S})
    return Wide(tmpl, S, table, draw(seed, len(tmpl), per, 2 * G + G // 2 + 300, (2 * G + 300) // S, apart), tb)


# ------------------------------------------------------------------ the brute force on the templates, once
def template_expectation(w, prm, T, table="own", cigars=True):
    """AU.expected and CU.expected on the batch of the templates -> dict(aln, ties, ops [per chain], info, need, cigars: CU.expected's own dict)."""
    table = w.table if isinstance(table, str) else table
    aln, _, ties = AU.expected(w.tb, prm, T, table)
    te = {"aln": aln, "ties": ties}
    if cigars:
        cg = CU.expected(w.tb, prm, T, aln, table)
        te["ops"] = [cg["cigar"][cg["offsets"][k]:cg["offsets"][k + 1]] for k in range(aln.shape[0])]
        te["info"], te["need"], te["cigars"] = cg["info"], cg["need"], cg
    return te


def wide_aln(w, te, cap=None):
    """What genie_align_chains returns for the wide batch -> (aln int32 [C, 8], totals int64 [2])."""
    aln = te["aln"][w.tchain]
    if cap is not None:
        aln = aln[:cap]
    skipped = int(((aln[:, 5] & 4) != 0).sum())
    return aln, np.asarray([aln.shape[0] - skipped, skipped], np.int64)


def wide_cigars(w, te, sel=None, cap_ops=None, dir_bytes=None):
    """What genie_chain_cigars returns for the wide batch and the selection -> the dict CU.expected makes."""
    C_ = w.tchain.size
    sel = np.arange(C_, dtype=np.int64) if sel is None else np.asarray(sel, np.int64)
    good = (sel >= 0) & (sel < C_)
    tc = w.tchain[np.where(good, sel, 0)]
    info = te["info"][tc].astype(np.int64)
    info[~good] = [0, CU.BAD, 0, 0, 0, 0, 0, 0]
    info[:, 0] = sel.astype(np.int32)                                # the low 32 bits, as the call writes them
    need = np.where(good, te["need"][tc], 0).astype(np.int64)
    ops = [te["ops"][t] if g else te["ops"][0][:0] for t, g in zip(tc.tolist(), good.tolist())]
    if dir_bytes is not None:
        for k in np.flatnonzero(np.cumsum(need) > dir_bytes).tolist():
            info[k, 1:] = [info[k, 1] | CU.NO_ROOM, 0, 0, 0, 0, 0, 0]
            ops[k] = ops[k][:0]
    assert all(len(o) == 0 for o, f in zip(ops, info[:, 1].tolist()) if f)
    offsets = np.zeros(sel.size + 1, np.int64)
    offsets[1:] = np.cumsum([len(o) for o in ops])
    cigar = np.concatenate(ops + [np.zeros(0, np.uint32)]).astype(np.uint32)
    flagged = int((info[:, 1] != 0).sum())
    return {"offsets": offsets, "cigar": cigar if cap_ops is None else cigar[:cap_ops], "info": info.astype(np.int32).reshape(-1, 8),
            "need": need, "totals": np.asarray([sel.size - flagged, flagged, int(need.sum())], np.int64)}


def wide_selection(seed, C_, n=3 * SCAN + 5, needy=None, at=()):
    """n entries: random chains with repeats, reversed stretches, and bad indices (negative, C, 2^40 and beyond) in rounds 1, 2
    and 4 of a scan of 1024; needy: chains to draw from for the positions `at`."""
    rng = np.random.default_rng(seed)
    sel = rng.integers(0, C_, n).astype(np.int64)
    for lo in (100, 1500, 2450):                                     # reversed stretches, one of them across a round's end
        sel[lo:lo + 600] = np.arange(lo + 5000, lo + 4400, -1) % C_
    sel[300:310] = sel[290:300]                                      # repeats next to each other, and far apart
    sel[2040:2056] = sel[7:23]
    bad = {5: -1, 700: C_, 1000: 2**40, 1100: -2**40, 1300: 2**40 + 3, 2000: C_ + 7, 3073: 2**40, 3075: -5}
    for k, v in bad.items():
        sel[k] = v
    for k in at:
        assert k not in bad
        sel[k] = int(needy[int(rng.integers(0, len(needy)))])
    return sel, sorted(bad)


# ------------------------------------------------------------------ genie_chain_mems: light units with heavy ones between
TABLE_CHAINS = np.asarray([0, 9000, 9000, 30000, 30011, 1 << 16], np.int64)
HEAVY = (65, 130, 513, 700, 1500)


def chain_units(seed, G, extra=300):
    """(offsets, rows, sizes, heavy) of U = 2 G + extra units of 0 to 6 rows, one in 8 empty, and 30 heavy ones placed so that
    u, u + G, u + 2 G are (heavy, light, heavy) for some u and (light, heavy, light) for others."""
    rng = np.random.default_rng(seed)
    U = 2 * G + extra
    sizes = np.where(rng.random(U) < 0.125, 0, rng.integers(1, 7, U))
    heavy = {}
    for k in range(10):                                              # (heavy, light, heavy) at 10 columns, (light, heavy, light) at 10
        u = 3 + 29 * k
        heavy[u], heavy[u + 2 * G] = HEAVY[k % 5], HEAVY[(k + 2) % 5]
        heavy[G + u + 13] = HEAVY[(k + 1) % 5]
    for u, n in heavy.items():
        sizes[u] = n
    offs, rows = CH.synth_batch(rng, sizes, 1 << 16)
    return offs, rows, sizes, sorted(heavy)
