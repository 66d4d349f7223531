"""GPU: SMEM.map_pairs and SMEM.sam_text against the composed host pipeline of tests/pipeline_util.py on its two simulated
batches -- noisy FR pairs, and the hard cases: repeats, overhangs, chimeras, indels, N runs, overlapping, RF, same-strand,
two-contig and distant pairs, random, short and empty mates, diverged mates inside and outside a rescue window.  Stage by stage
through the public methods, each fed the device's previous result, so that a failure names the first stage that differs; the
whole call, every tensor of its tuple exactly equal; the text, byte for byte and through check_sam; the four forms a batch may
be given in; and the run without a contig table.  The host runs are computed once per batch and option set and shared with
tests/test_pipeline_host.py, which checks them on their own."""
import numpy as np
import pytest

import isize_util as IU
import pipeline_util as P

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    import genie_smem_amd as g

    class Env:
        pass
    e = Env()
    e.g, e.mapped = g, {}
    e.T = P.batch("hard")[0]
    m = g.ExactMatch("pipeline_simulated.fa")
    m.set_reference("".join("ACGT"[c] for c in e.T))
    e.sm = g.SMEM(m, 4)
    e.rs = g.ReferenceSet([x.decode() for x in P.CONTIG_NAMES], P.TABLE, e.T)
    return e


def _np(t):
    import torch
    return (t.view(torch.int32) if t.dtype == torch.uint32 else t).cpu().numpy()


def _same(stage, name, got, want):
    """dtype, shape and every element; a uint32 tensor is compared as the int32 of the same bits."""
    got = _np(got) if hasattr(got, "cpu") else np.asarray(got)
    want = np.asarray(want)
    if want.dtype == np.uint32:
        want = want.view(np.int32)
    assert got.dtype == want.dtype and got.shape == want.shape, (stage, name, got.dtype, want.dtype, got.shape, want.shape)
    bad = np.argwhere(got != want)
    assert bad.size == 0, (stage, name, len(bad), bad[:4].tolist(), got[tuple(bad[0])[:1]].tolist(), want[tuple(bad[0])[:1]].tolist())


def _kwargs(b, option_set):
    """map_pairs' keyword arguments: host_pipeline's, the chain options flat."""
    opts = P.map_options(b, option_set)
    opts.update(opts.pop("chain_options", {}))
    return opts


def _mapped(env, name, option_set):
    """SMEM.map_pairs on a batch given as CSR codes, with the contig table: launched once per option set and shared."""
    if (name, option_set) not in env.mapped:
        b = P.batch(name)[1]
        csr = (b.bases, b.read_offsets)
        env.mapped[name, option_set] = env.sm.map_pairs(csr, b.options["minimum_length"], env.rs, **_kwargs(b, option_set))
    return env.mapped[name, option_set]


def _same_result(stage, got, want):
    assert len(got) == len(want), (stage, len(got), len(want))
    names = "records sel_offsets cigar_offsets cigar info pairs sam".split()
    import torch
    assert got[3].dtype == torch.uint32
    for name, x, y in zip(names, got[:7], want[:7]):
        _same(stage, name, x, y)
    rest_got, rest_want = list(got[7:]), list(want[7:])
    if rest_want and isinstance(rest_want[0], tuple) and len(rest_want[0]) == 3 and not hasattr(rest_want[0], "orient"):
        for name, x, y in zip(("windows", "status", "totals"), rest_got.pop(0), rest_want.pop(0)):
            _same(stage, name, x, y)
    assert len(rest_got) == len(rest_want) <= 1
    if rest_want:
        assert isinstance(rest_got[0], type(rest_want[0])) and rest_got[0] == rest_want[0], (stage, "InsertSize", rest_got[0], rest_want[0])


def _four(env, b, csr, mems, host, tag, kw, popts, before_pairing=None):
    """chain_mems, align_chains, select_alignments and pair_alignments on device MEM rows against one pass of the host run."""
    sm, rs = env.sm, env.rs
    chains = sm.chain_mems(mems[0], mems[1], rs, by_score=False, **kw.get("chain_options", {}))
    for name, x, y in zip(("offsets", "chains", "anchor_chain", "anchor_pred", "anchor_score"), chains[:5], (host["chains"][k] for k in (
            "offsets", "chains", "anchor_chain", "anchor_pred", "anchor_score"))):
        _same(tag + "chain_mems", name, x, y)
    assert chains[5] == host["chains"]["totals"][1], (tag + "chain_mems", "dropped")
    aln, counts = sm.align_chains(csr, mems[0], mems[1], chains, rs, True, kw["split_breaks"], **kw.get("align_options", {}))
    _same(tag + "align_chains", "aln", aln, host["aln"])
    assert list(counts) == host["aln_totals"].tolist(), (tag + "align_chains", "totals")
    sel = sm.select_alignments(csr[1], chains[0], chains[1], aln, rs, True, **kw.get("select_options", {}))
    keys = ("offsets", "sel", "records", "klass", "counts", "totals")
    for name, x, key in zip(("sel_offsets", "sel", "records", "klass", "read_counts", "totals"), sel, keys):
        _same(tag + "select_alignments", name, x, host["select"][key])
    if before_pairing is not None:
        before_pairing(sel)
    pairs = sm.pair_alignments(sel[0], sel[2], sel[3], **popts)
    for name, x, key in zip(("pairs", "sam", "totals"), pairs, ("pairs", "sam", "totals")):
        _same(tag + "pair_alignments", name, x, host["pair"][key])
    return chains, aln, sel, pairs


@pytest.mark.parametrize("name, option_set", [("hard", "rescue"), ("library", "estimate")])
def test_stage_by_stage(env, name, option_set):
    g, sm, rs = env.g, env.sm, env.rs
    T, b = P.batch(name)
    host = P.host_run(name, option_set)
    kw = P.map_options(b, option_set)
    csr = (b.bases, b.read_offsets)
    m, split = b.options["minimum_length"], kw["split_breaks"]
    mems = sm.find_mems_contigs(rs, csr, m, True, split, 0)
    for what, x, y in zip(("offsets", "rows", "status"), mems[:3], host.first["mems"][:3]):
        _same("find_mems_contigs", what, x, y)
    assert int(mems[3]) == host.first["mems"][3]
    popts = {}

    def estimate(sel):
        """Between the first selection and the first pairing, where map_pairs reads the statistics; a batch that asks for no
        estimate checks the call all the same."""
        stats, samples, totals = sm.insert_size_stats(sel[0], sel[2], samples=True)
        want = IU.expected(host.first["pair_batch"], IU.DEFAULTS)
        for what, x in (("stats", stats), ("samples", samples), ("totals", totals)):
            _same("insert_size_stats", what, x, want[what])
        if host.est is not None:
            est = g.index.insert_size_options(stats.cpu(), {})
            assert est == host.est, ("insert_size_options", est, host.est)
            popts.update(orient=est.orient, isize_min=est.isize_min, isize_max=est.isize_max, isize_mean=est.isize_mean)
    chains, aln, sel, pairs = _four(env, b, csr, mems, host.first, "first pass: ", kw, popts, estimate)
    where = {k: popts[k] for k in ("orient", "isize_max") if k in popts}
    windows, planned = sm.rescue_windows(csr[1], sel[0], sel[2], pairs[0], rs, min_anchor_score=P.RESCUE_MIN_ANCHOR, **where)
    _same("rescue_windows", "windows", windows, host.windows)
    _same("rescue_windows", "totals", planned, host.planned)
    assert host.second is not None and int(planned[0]) > 0
    wm = sm.window_mems(csr, windows, P.RESCUE_MIN_LEN, mems[0], mems[1], True, split)
    for what, x, y in zip(("offsets", "rows", "status", "totals"), wm, host.window_mems):
        _same("window_mems", what, x, y)
    chains, aln, sel, pairs = _four(env, b, csr, wm, host.second, "second pass: ", kw, popts)
    cig = sm.chain_cigars(csr, wm[0], wm[1], chains, aln, sel[1], rs, True, split)
    for what, x, key in zip(("cigar_offsets", "cigar", "info"), cig, ("offsets", "cigar", "info")):
        _same("chain_cigars", what, x, host.cigars[key])
    result = (sel[2], sel[0], cig[0], cig[1], cig[2], pairs[0], pairs[1])
    text = sm.sam_text(result, csr, b.names, quals=b.quals, contigs=rs, tags=P.ALL_TAGS)
    want = P.host_sam_text(host.result, T, P.TABLE, csr, b.names, P.CONTIG_NAMES, b.quals, P.ALL_TAGS)
    for what, x, y in zip(("text", "line_offsets", "totals"), text, want):
        _same("sam_text", what, x, y)


WHOLE = [(n, s) for n in ("library", "hard") for s in ("plain", "rescue", "estimate")] + [("hard", "any")]


@pytest.mark.parametrize("name, option_set", WHOLE)
def test_the_whole(env, name, option_set):
    _same_result(f"map_pairs({name}, {option_set})", _mapped(env, name, option_set), P.host_run(name, option_set).result)


def _quals(b):
    return [bytes(b.quals[b.read_offsets[r]:b.read_offsets[r + 1]]) for r in range(len(b.truth))]


@pytest.mark.parametrize("name, option_set", [("hard", "rescue"), ("library", "estimate")])
def test_text(env, name, option_set):
    g, sm, rs = env.g, env.sm, env.rs
    T, b = P.batch(name)
    host = P.host_run(name, option_set)
    csr = (b.bases, b.read_offsets)
    out = _mapped(env, name, option_set)
    quals = _quals(b)
    cases = ((3, True, True), (3, False, True), (P.ALL_TAGS, True, True), (P.ALL_TAGS, False, True), (P.ALL_TAGS, True, False))
    for tags, with_quals, seq in cases:
        got = sm.sam_text(out, csr, b.names, quals=b.quals if with_quals else None, contigs=rs, tags=tags, seq=seq)
        want = P.host_sam_text(host.result, T, P.TABLE, csr, b.names, P.CONTIG_NAMES, b.quals if with_quals else None, tags, seq)
        for what, x, y in zip(("text", "line_offsets", "totals"), got, want):
            _same(f"sam_text(tags={tags}, quals={with_quals}, seq={seq})", what, x, y)
        lines = P.check_sam(_np(got[0]), _np(got[1]), T, P.TABLE, P.CONTIG_NAMES, b.reads(), b.names, host.align_params, tags=tags, seq=seq,
                            quals=quals if with_quals and seq else None)
        assert lines == int(got[2][0])
        if tags == 3 and with_quals:                                 # sam_lines writes these columns and these two tags
            helper = g.sam_lines(out[0], out[6], out[4], out[2], out[3], [x.decode() for x in b.names], rs.names, b.strings(),
                                 [q.decode() for q in quals])
            assert bytes(_np(got[0])).decode() == "".join(ln + "\n" for ln in helper)


def test_entry_forms(env):
    """The hard batch as strings, as a (reads1, reads2) tuple of lists, as FASTQ text and as CSR codes: the same bytes."""
    g, sm, rs = env.g, env.sm, env.rs
    T, b = P.batch("hard")
    host = P.host_run("hard", "rescue")
    kw = _kwargs(b, "rescue")
    m = b.options["minimum_length"]
    strings, quals = b.strings(), _quals(b)
    records = enumerate(zip(b.names, strings, quals))
    fastq = b"".join(b"@%s mate/%d\n%s\n+\n%s\n" % (n, r % 2 + 1, s.encode(), q) for r, (n, s, q) in records)
    bases, read_offsets, consumed = g.text_reads.reads_from_text(fastq, "fastq")
    assert consumed == len(fastq)
    _same("reads_from_text", "bases", bases, b.bases)
    _same("reads_from_text", "read_offsets", read_offsets, b.read_offsets)
    names, name_offsets, qs = g.text_reads.fastq_fields(fastq, read_offsets)
    forms = {"strings": strings, "tuple": (strings[0::2], strings[1::2]), "fastq": (bases, read_offsets), "csr": (b.bases, b.read_offsets)}
    texts = {}
    for form, reads in forms.items():
        out = _mapped(env, "hard", "rescue") if form == "csr" else sm.map_pairs(reads, m, rs, **kw)
        _same_result(f"map_pairs({form})", out, host.result)
        given = {"strings": strings, "tuple": strings, "fastq": (bases, read_offsets), "csr": (b.bases, b.read_offsets)}[form]
        name_arg, qual_arg = (b.names, quals) if form in ("strings", "tuple") else (b.names, b.quals)
        if form == "fastq":
            name_arg, qual_arg = (names, name_offsets), qs
        texts[form] = bytes(_np(sm.sam_text(out, given, name_arg, quals=qual_arg, contigs=rs, tags=P.ALL_TAGS)[0]))
    want = P.host_sam_text(host.result, T, P.TABLE, (b.bases, b.read_offsets), b.names, P.CONTIG_NAMES, b.quals, P.ALL_TAGS)[0]
    for form, text in texts.items():
        assert text == bytes(want), form


@pytest.mark.parametrize("option_set", ["plain", "estimate"])
def test_without_a_contig_table(env, option_set):
    T, b = P.batch("library")
    host = P.host_run("library", option_set, table=False)
    csr = (b.bases, b.read_offsets)
    out = env.sm.map_pairs(csr, b.options["minimum_length"], None, **_kwargs(b, option_set))
    _same_result(f"map_pairs(library, {option_set}, no table)", out, host.result)
    got = env.sm.sam_text(out, csr, b.names, quals=b.quals, tags=P.ALL_TAGS)
    want = P.host_sam_text(host.result, T, None, csr, b.names, [b"ref"], b.quals, P.ALL_TAGS)
    for what, x, y in zip(("text", "line_offsets", "totals"), got, want):
        _same("sam_text without a table", what, x, y)
    P.check_sam(_np(got[0]), _np(got[1]), T, None, [b"ref"], b.reads(), b.names, host.align_params, quals=_quals(b))
