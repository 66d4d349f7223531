"""SMEM -- drop-in for the reference's SMEM class (reference SMEM/SMEM.py:8).

Per-query methods keep the reference's names, arguments and return shapes:
    get_SMEMS(query, minimum_length)   BWA-SMEM   (SMEM.py:456)
    get_smems_lut(query)               LUT-SMEM   (SMEM.py:20)
    get_smems_rmi(query)               RMI-SMEM   (SMEM.py:206)
each returning the insertion-ordered dict {substring: (lo, hi)}.  They are thin views over the
batched entry points
    find_smems_bwa / find_smems_lut / find_smems_rmi (reads) -> (offsets, smems[S,4], status)
which run one wavefront per read on the GPU (genie_find_smems).  The single-step helpers
(get_suffix_index, forward_extension, backward_extension, get_SMEM_at_index, check_sequential)
are provided with the reference's semantics on top of the batched interval search.
"""
import random

import numpy as np
import torch

from . import _native as N
from .exact_match import ExactMatch
from .lut import LUT
from .rmi_lut import RMI_LUT
from .text_reads import reads_from_text


class SMEM:

    def __init__(self, matcher: ExactMatch, lut_size: int = None):
        self.matcher = matcher
        self.lut = LUT(self.matcher)
        if lut_size is None:
            self.lut.load_lut()                 # SMEM.py:11-12 (FileNotFoundError if never saved)
        else:
            self.lut.generate_lut(lut_size)
        self.rmi_lut = None

    # ------------------------------------------------------------------ batched entry points
    @staticmethod
    def _encode_batch(reads, encode):
        """list[str] -> (uint8 [N, max(width, 1)] codes, zero-padded; int32 lens, or None when every read has the same
        length; width: the longest read's length, 0 for no reads)."""
        enc = [encode(r) for r in reads]
        lens = np.asarray([len(e) for e in enc], np.int32)
        width = int(lens.max()) if len(enc) else 0
        mat = np.zeros((len(enc), max(width, 1)), np.uint8)
        for i, e in enumerate(enc):
            mat[i, :len(e)] = e
        ragged = len(enc) > 0 and int(lens.min()) != width
        return mat, (lens if ragged else None), width

    def _reads_codes(self, reads):
        """list[str] | ndarray -> (uint8 [N, width] numpy codes, int32 lens or None)."""
        if isinstance(reads, np.ndarray):
            return np.ascontiguousarray(reads, np.uint8), None
        mat, lens, _ = self._encode_batch(reads, self.matcher.encode)
        return mat, lens

    def _reads_tensor(self, reads):
        """list[str] | ndarray | tensor -> (uint8 [N, stride] on the device, lens or None)."""
        ix_dev = torch.device(self.matcher.device)
        if isinstance(reads, torch.Tensor):
            return reads, None
        if isinstance(reads, np.ndarray):
            return torch.as_tensor(np.ascontiguousarray(reads, np.uint8)).to(ix_dev), None
        mat, lens, _ = self._encode_batch(reads, self.matcher.encode)
        return torch.as_tensor(mat).to(ix_dev), (torch.as_tensor(lens).to(ix_dev) if lens is not None else None)

    def _mode_index(self, mode):
        if mode == "rmi":
            if self.rmi_lut is None:
                self.rmi_lut = RMI_LUT.load("rmi_file.npz", matcher=self.matcher)     # cf. SMEM.py:207
            return self.rmi_lut._index()
        return self.matcher.index(self.lut.lut_size)

    def _find(self, mode, reads, lens, min_len):
        ix = self._mode_index(mode)
        if not isinstance(reads, torch.Tensor):
            # host inputs: 2-bit packed over the host link, 8-byte rows back (genie_find_smems_packed); results on the host
            codes, l2 = self._reads_codes(reads)
            if codes.shape[1] <= 255:
                ln = lens if lens is not None else l2
                off, rows, st = ix.find_smems_host(mode, codes, ln, min_len)
                return torch.as_tensor(off), torch.as_tensor(rows), torch.as_tensor(st)
        t, l2 = self._reads_tensor(reads)
        return ix.find_smems(mode, t, lens if lens is not None else l2, min_len)

    def find_smems_bwa(self, reads, minimum_length=1, lens=None):
        return self._find("bwa", reads, lens, minimum_length)

    def find_smems_split(self, reads, minimum_length=1, lens=None):
        """get_SMEMS over reads that may hold ambiguous bases (N): every symbol outside the reference's alphabet, and every
        base the reference lacks, is a break, and a read's SMEMs are those of the runs between its breaks (start / end in
        the whole read).  reads: list[str] (encoded with ExactMatch.encode_lenient), or numpy / torch uint8 codes (any code
        > 3 is a break).  Host inputs travel as uint8 codes (the 2-bit packed host path cannot carry a break); results come
        back on the device.  -> (offsets, smems[S, 4], status) like find_smems_bwa."""
        ix = self.matcher.index(self.lut.lut_size)
        if isinstance(reads, (torch.Tensor, np.ndarray)):
            return ix.find_smems_split(reads, lens, minimum_length)
        mat, ln, width = self._encode_batch(reads, self.matcher.encode_lenient)
        if lens is None:
            lens = ln
        return ix.find_smems_split(mat if width else mat[:, :0], lens, minimum_length)

    def find_smems_both(self, reads, mode="lut", minimum_length=1, lens=None):
        """SMEMs of both strands of every read in one call (genie_find_smems_both).  reads: list[str], or numpy / torch uint8
        codes.  -> (offsets int64[2N+1], smems[S, 4], status int32[2N]) on the device: strand-read 2i is read i, 2i + 1 its
        reverse complement, whose rows are those get_SMEMS / get_smems_lut / get_smems_rmi give for that reverse complement
        (start / end in it; forward coordinates L - end, L - start).  Host inputs travel as uint8 codes."""
        ix = self._mode_index(mode)
        t, l2 = self._reads_tensor(reads)
        return ix.find_smems_both(mode, t, lens if lens is not None else l2, minimum_length)

    def find_smems_long(self, reads, minimum_length=1, mode="bwa", both_strands=False, split_breaks=False):
        """SMEMs of reads of any length (genie_find_smems_long).  reads: list[str], or (bases, read_offsets) -- uint8 codes
        back to back and int64[N+1] offsets, numpy or torch.  -> (offsets, smems[S, 4], status) like find_smems_bwa.
        both_strands: 2N strand-reads as find_smems_both (2i read i, 2i + 1 its reverse complement).  split_breaks (mode
        "bwa"): breaks cut the reads as find_smems_split; strings are then encoded with ExactMatch.encode_lenient."""
        ix = self.matcher.index(self.lut.lut_size)
        bases, read_offsets = self._csr_reads(reads, split_breaks)
        return ix.find_smems_long(mode, bases, read_offsets, minimum_length, both_strands=both_strands, split_breaks=split_breaks)

    def find_smems_text(self, data, fmt="lines", mode="bwa", minimum_length=1, both_strands=False, split_breaks=True,
                        fold_case=False):
        """SMEMs of the reads in a text: every line a read (fmt "lines"), four-line FASTQ records (fmt "fastq") or FASTA
        records with wrapped sequences (fmt "fasta").  data: bytes-like, numpy uint8 or torch uint8, on the host or the
        device.  The text is cut into reads and translated on the device (text_reads.reads_from_text with
        ExactMatch.byte_codes(fold_case): the codes encode_lenient gives), then searched as
        find_smems_long((bases, read_offsets), ...) with the same options.  -> (offsets, smems[S, 4], status)."""
        return self._find_text(data, fmt, False, mode, minimum_length, both_strands, split_breaks, fold_case)[:3]

    def _find_text(self, data, fmt, partial, mode, minimum_length, both_strands, split_breaks, fold_case):
        """find_smems_text on one chunk -> (offsets, smems, status, reads, consumed bytes)."""
        ix = self.matcher.index(self.lut.lut_size)
        bases, read_offsets, consumed = reads_from_text(data, fmt, self.matcher.byte_codes(fold_case), partial, ix.device)
        res = ix.find_smems_long(mode, bases, read_offsets, minimum_length, both_strands=both_strands, split_breaks=split_breaks)
        return res + (read_offsets.numel() - 1, consumed)

    def match_stats(self, reads, intervals=True, both_strands=False, split_breaks=False):
        """Matching statistics of every position of every read (genie_match_stats): the batched forward_extension.  reads:
        list[str], or (bases, read_offsets) as find_smems_long takes them.  -> (ms int32[S*total], lohi int32[S*total, 2] or
        None with intervals=False, status int32[S*N]) on the device: position p of strand-read S*i + s is element
        S*read_offsets[i] + s*L_i + p, ms the length of the longest match that starts there and lohi its interval, so that
        forward_extension(q, p)[1] == q[p:p + ms] and its interval is lohi.  split_breaks: breaks are covered by no match
        and flag no read; strings are then encoded with ExactMatch.encode_lenient."""
        ix = self.matcher.index(self.lut.lut_size)
        bases, read_offsets = self._csr_reads(reads, split_breaks)
        return ix.match_stats(bases, read_offsets, intervals, both_strands, split_breaks)

    def find_mems(self, reads, minimum_length, both_strands=False, split_breaks=False, max_occ=0):
        """Every maximal exact match of at least minimum_length bases, with its reference position (genie_find_mems).
        reads: list[str], or (bases, read_offsets) as match_stats takes them.  -> (offsets int64[S*N+1], mems int32[R, 4] =
        (start, end, pos, row), status int32[S*N], skipped) on the device: bases [start, end) of the strand-read equal the
        reference from the 1-based position pos on, and neither side extends; rows of a strand-read by (start, row).
        max_occ > 0 skips positions whose first minimum_length bases occur more often than that (`skipped` counts them).
        split_breaks: breaks end a match and flag no read; strings are then encoded with ExactMatch.encode_lenient."""
        ix = self.matcher.index(self.lut.lut_size)
        bases, read_offsets = self._csr_reads(reads, split_breaks)
        return ix.find_mems(bases, read_offsets, minimum_length, both_strands, split_breaks, max_occ)

    def find_mems_contigs(self, contigs, reads, minimum_length, both_strands=False, split_breaks=False, max_occ=0):
        """find_mems on a reference of several sequences (genie_find_mems_contigs): contigs is the ReferenceSet whose
        concatenation this matcher's reference is.  reads and the four results as find_mems; every row lies inside one
        contig (GenieIndex.find_mems_contigs), pos is 1-based in the concatenation (contigs.coords names it)."""
        ix = self.matcher.index(self.lut.lut_size)
        bases, read_offsets = self._csr_reads(reads, split_breaks)
        return ix.find_mems_contigs(contigs, bases, read_offsets, minimum_length, both_strands, split_breaks, max_occ)

    def chain_mems(self, offsets, rows, contigs=None, **chain_options):
        """The rows of find_mems / find_mems_contigs chained per strand-read (genie_chain_mems) -> (chain_offsets, chains
        int32[C, 8] = (q_begin, q_end, r_begin, r_end, score, n_anchors, contig, last), anchor_chain, anchor_pred,
        anchor_score, dropped): GenieIndex.chain_mems, which documents the options (max_dist, bandwidth, gap_cost, max_pred,
        min_score, by_score) and their defaults."""
        return self.matcher.index(self.lut.lut_size).chain_mems(offsets, rows, contigs, **chain_options)

    def find_chains(self, reads, minimum_length, contigs=None, both_strands=False, split_breaks=False, max_occ=0, **chain_options):
        """find_mems (find_mems_contigs with a ReferenceSet) followed by chain_mems on its rows -> (mems, chains): the two
        calls' results as they return them.  Candidate mapping locations of every strand-read: chains[:, 2:4] in the
        concatenation's 1-based coordinates, chains[:, 6] the contig, the strand the unit's parity with both_strands."""
        if contigs is None:
            mems = self.find_mems(reads, minimum_length, both_strands, split_breaks, max_occ)
        else:
            mems = self.find_mems_contigs(contigs, reads, minimum_length, both_strands, split_breaks, max_occ)
        return mems, self.chain_mems(mems[0], mems[1], contigs, **chain_options)

    def align_chains(self, reads, offsets, rows, chains_result, contigs=None, both_strands=False, split_breaks=False, **align_options):
        """Every chain of chain_mems aligned (genie_align_chains) -> (aln int32[C, 8] = (score, q_begin, q_end, r_begin,
        r_end, flags, n_used, matched), (aligned, skipped)): GenieIndex.align_chains, which documents the options (match,
        mismatch, gap_open, gap_extend, band, max_indel, end_bonus) and their defaults.  reads as find_mems took them, with
        the same split_breaks (it decides how strings are encoded, nothing else); chains_result: chain_mems' result with
        by_score=False."""
        ix = self.matcher.index(self.lut.lut_size)
        return ix.align_chains(self._csr_reads(reads, split_breaks), offsets, rows, chains_result, contigs, both_strands, **align_options)

    def find_alignments(self, reads, minimum_length, contigs=None, both_strands=False, split_breaks=False, max_occ=0, align_options=None,
                        **chain_options):
        """find_chains followed by align_chains -> (mems, chains, aln): the first two as find_chains returns them, aln int32[C, 8]
        parallel to the chain rows.  With by_score=True the chains of a unit come by (score descending, last ascending), as
        chain_mems orders them, and aln follows the same order.  align_options: a dict of align_chains' options."""
        by_score = bool(chain_options.pop("by_score", False))
        csr = self._csr_reads(reads, split_breaks)
        mems, chains = self.find_chains(csr, minimum_length, contigs, both_strands, split_breaks, max_occ, by_score=False, **chain_options)
        aln, _ = self.align_chains(csr, mems[0], mems[1], chains, contigs, both_strands, split_breaks, **(align_options or {}))
        if by_score and chains[1].shape[0]:
            ix = self.matcher.index(self.lut.lut_size)
            order = ix._chains_by_score(mems[0], chains[0], chains[1], chains[2])
            chains = (chains[0], chains[1][order]) + tuple(chains[2:])
            aln = aln[order]
        return mems, chains, aln

    def chain_cigars(self, reads, offsets, rows, chains_result, aln, select=None, contigs=None, both_strands=False, split_breaks=False,
                     **cigar_options):
        """The CIGAR of selected chains (genie_chain_cigars) -> (cigar_offsets, cigar uint32[ops], info int32[n_sel, 8] =
        (chain, flags, n_ops, nm, n_eq, n_x, ins_bases, del_bases)): GenieIndex.chain_cigars, which documents `select`, the
        options (align_chains' scoring options, which must be those aln was made with, ops_hint, dir_bytes_hint) and their
        defaults.  reads, split_breaks and chains_result as align_chains took them; aln: its first result."""
        ix = self.matcher.index(self.lut.lut_size)
        return ix.chain_cigars(self._csr_reads(reads, split_breaks), offsets, rows, chains_result, aln, select, contigs, both_strands,
                               **cigar_options)

    def map_reads(self, reads, minimum_length, contigs=None, both_strands=True, split_breaks=False, max_occ=0, align_options=None,
                  **chain_options):
        """One mapping per read: find_alignments, then per read the non-skipped chain of the highest alignment score over its
        strand-reads (a tie goes to the smaller global chain index), then chain_cigars on that selection -> (hits int32[N, 6] =
        (chain, strand, contig, offset, score, nm), cigar_offsets int64[N+1], cigar uint32[ops]) on the device.  chain is the
        global chain index (the row of find_alignments' chains and aln), strand 1 the reverse complement, offset the 1-based
        start of the alignment inside its contig (in the concatenation, and contig 0, without `contigs`); the CIGAR is in
        strand-read order, as SAM has it.  A read without a chain gets (-1, 0, -1, 0, 0, 0) and an empty CIGAR."""
        import torch
        ix = self.matcher.index(self.lut.lut_size)
        csr = self._csr_reads(reads, split_breaks)
        opts = dict(align_options or {})
        mems, chains, aln = self.find_alignments(csr, minimum_length, contigs, both_strands, split_breaks, max_occ, opts, by_score=False,
                                                 **chain_options)
        S = 2 if both_strands else 1
        U, kept = mems[0].numel() - 1, chains[1].shape[0]
        n_reads = U // S
        dev = aln.device
        hits = torch.zeros((n_reads, 6), dtype=torch.int32, device=dev)
        hits[:, 0] = -1
        hits[:, 2] = -1
        if kept == 0 or n_reads == 0:
            return hits, torch.zeros(n_reads + 1, dtype=torch.int64, device=dev), torch.zeros(0, dtype=torch.int32, device=dev).view(torch.uint32)
        unit = torch.repeat_interleave(torch.arange(U, device=dev), chains[0][1:] - chains[0][:-1])
        read = unit // S
        live = (aln[:, 5] & 4) == 0
        # the best score of every read, then the smallest chain index that has it
        score = torch.where(live, aln[:, 0].long(), torch.full((kept,), -(1 << 40), dtype=torch.int64, device=dev))
        best = torch.full((n_reads,), -(1 << 40), dtype=torch.int64, device=dev).scatter_reduce(0, read, score, "amax")
        index = torch.arange(kept, device=dev)
        cand = torch.where(live & (score == best[read]), index, torch.full_like(index, kept))
        pick = torch.full((n_reads,), kept, dtype=torch.int64, device=dev).scatter_reduce(0, read, cand, "amin")
        has = pick < kept
        sel = pick[has]
        offs, cigar, info = ix.chain_cigars(csr, mems[0], mems[1], chains, aln, sel, contigs, both_strands, **opts)
        got = aln[sel]
        hits[has, 0] = sel.to(torch.int32)
        hits[has, 1] = (unit[sel] % S).to(torch.int32)
        if contigs is not None:
            hits[has, 2:4] = ix.contig_coords(contigs, got[:, 3].contiguous())
        else:
            hits[has, 2] = 0
            hits[has, 3] = got[:, 3]
        hits[has, 4] = got[:, 0]
        hits[has, 5] = info[:, 3]
        counts = torch.zeros(n_reads, dtype=torch.int64, device=dev)
        counts[has] = offs[1:] - offs[:-1]
        cigar_offsets = torch.zeros(n_reads + 1, dtype=torch.int64, device=dev)
        cigar_offsets[1:] = torch.cumsum(counts, 0)
        return hits, cigar_offsets, cigar

    def select_alignments(self, read_offsets, chain_offsets, chains, aln, contigs=None, both_strands=False, **select_options):
        """The alignments of every read (genie_select_alignments) -> (sel_offsets, sel, records int32[n, 12] = (read, chain, kind,
        strand, contig, offset, r_span, q_begin, q_end, score, sub, mapq), klass, read_counts, totals):
        GenieIndex.select_alignments, which documents the options (mask_level, pri_ratio, max_secondary, min_score, mapq_full)
        and their defaults."""
        ix = self.matcher.index(self.lut.lut_size)
        return ix.select_alignments(read_offsets, chain_offsets, chains, aln, contigs, both_strands, **select_options)

    def map_records(self, reads, minimum_length, contigs=None, both_strands=True, split_breaks=False, max_occ=0, align_options=None,
                    select_options=None, **chain_options):
        """Every alignment of every read: find_alignments, select_alignments on its rows, chain_cigars on that selection ->
        (records int32[n, 12], sel_offsets int64[N+1], cigar_offsets int64[n+1], cigar uint32[ops], info int32[n, 8]) on the
        device, records, CIGARs and info parallel: read i's alignments are the rows sel_offsets[i] .. sel_offsets[i+1], its
        primary first, then its supplementary ones, then its secondaries.  records as select_alignments returns them (kind 0
        primary, 1 supplementary, 2 secondary; q_begin / q_end in forward read coordinates); the CIGAR is in strand-read
        order, as SAM has it; paf_lines turns the lot into text.  align_options, select_options: dicts of align_chains' and
        select_alignments' options."""
        ix = self.matcher.index(self.lut.lut_size)
        csr = self._csr_reads(reads, split_breaks)
        opts = dict(align_options or {})
        mems, chains, aln = self.find_alignments(csr, minimum_length, contigs, both_strands, split_breaks, max_occ, opts, by_score=False,
                                                 **chain_options)
        sel_offsets, sel, records = ix.select_alignments(csr[1], chains[0], chains[1], aln, contigs, both_strands, **(select_options or {}))[:3]
        offs, cigar, info = ix.chain_cigars(csr, mems[0], mems[1], chains, aln, sel, contigs, both_strands, **opts)
        return records, sel_offsets, offs, cigar, info

    def pair_alignments(self, sel_offsets, records, klass, **pair_options):
        """The alignments of paired-end reads (genie_pair_alignments) -> (pairs int32[P, 8] = (rec0, rec1, flags, pair_score,
        sub_score, isize, n_concordant, type), sam int32[R, 4] = (flag, mapq, mate_record, tlen), totals):
        GenieIndex.pair_alignments, which documents the options (orient, isize_min, isize_max, isize_mean, pen_slope, pen_max,
        pen_unpaired, mapq_boost) and their defaults.  Reads 2k and 2k + 1 are the mates of pair k."""
        ix = self.matcher.index(self.lut.lut_size)
        return ix.pair_alignments(sel_offsets, records, klass, **pair_options)

    def insert_size_stats(self, sel_offsets, records, **options):
        """The insert-size distribution of a paired batch, estimated from the batch (genie_insert_size_stats) -> (stats
        int64[3, 12], samples int32[P, 2] or None, totals int64[4]): GenieIndex.insert_size_stats, which documents the options
        (min_mapq, max_span, min_samples, samples) and their defaults; index.insert_size_options turns stats into
        pair_alignments' options."""
        ix = self.matcher.index(self.lut.lut_size)
        return ix.insert_size_stats(sel_offsets, records, **options)

    def rescue_windows(self, read_offsets, sel_offsets, records, pairs, contigs=None, **rescue_options):
        """Where to seed a mate again next to its partner (genie_rescue_windows) -> (windows int32[2N, 2], totals):
        GenieIndex.rescue_windows, which documents the options (orient, isize_max, min_anchor_score) and their defaults."""
        ix = self.matcher.index(self.lut.lut_size)
        return ix.rescue_windows(read_offsets, sel_offsets, records, pairs, contigs, **rescue_options)

    def window_mems(self, reads, windows, minimum_length, offsets=None, rows=None, both_strands=False, split_breaks=False):
        """The MEMs of every strand-read against its own window of the reference, merged into the rows of find_mems*
        (genie_window_mems) -> (offsets, mems int32[R, 4], status, totals): GenieIndex.window_mems.  reads as find_mems takes
        them; windows int32[U, 2] = (wb, we), one per strand-read; offsets / rows: find_mems*' first two results, or None."""
        ix = self.matcher.index(self.lut.lut_size)
        bases, read_offsets = self._csr_reads(reads, split_breaks)
        return ix.window_mems(bases, read_offsets, windows, minimum_length, offsets, rows, both_strands, split_breaks)

    def map_pairs(self, reads, minimum_length, contigs=None, both_strands=True, split_breaks=False, max_occ=0, align_options=None,
                  select_options=None, pair_options=None, rescue=False, rescue_options=None, insert_size=None, **chain_options):
        """Every alignment of every mate, paired: map_records on the interleaved batch, then pair_alignments on its records ->
        (records, sel_offsets, cigar_offsets, cigar, info, pairs, sam): map_records' five results, then pairs int32[P, 8] and
        sam int32[n, 4] parallel to records; sam_lines turns the lot into text.  reads: an interleaved batch (reads 2k and
        2k + 1 are mates) in any form map_records takes, or a tuple (reads1, reads2) of two batches of equally many reads,
        each in such a form, which text_reads.interleave_reads makes one.  pair_options: a dict of pair_alignments' options.
        rescue=True (it needs both_strands) seeds the mates of pairs that are not proper again, next to their partner: after
        the first pairing rescue_windows names the windows; where there is one, window_mems adds each window's MEMs of at
        least rescue_options["min_len"] bases (12) to the rows of the first pass, and chaining, alignment, selection and pairing
        run once more over the union, with the same options.  rescue_options: a dict of min_len, min_anchor_score (40) and
        the orient and isize_max of rescue_windows (default: those of pair_options).  An eighth result then follows the
        seven: (windows int32[2N, 2], status int32[2N], totals int64[3]) as rescue_windows and window_mems return them, status
        and totals zero where no unit had a window.
        insert_size: None, and orient, isize_min, isize_max and isize_mean are pair_options' (or the defaults).  "estimate", or
        a dict of insert_size_stats' options (min_mapq, max_span, min_samples): the statistics of the records of the first
        selection are read to the host (36 numbers: the one added host read) and index.insert_size_options turns them into
        those four options of every pairing, before and after rescue, and into rescue's orient and isize_max unless
        rescue_options names them; the values given in pair_options are the fallback where no type has samples enough.  An
        index.InsertSize of an earlier call is applied as it is, without estimating: estimate on the first chunk of a file,
        reuse on the others.  In both cases the InsertSize used follows as the last result."""
        import torch
        from .index import InsertSize, insert_size_options
        from .text_reads import interleave_reads
        ix = self.matcher.index(self.lut.lut_size)
        if isinstance(reads, tuple) and len(reads) == 2 and all(isinstance(r, (list, tuple)) for r in reads):
            ix._need_device()
            one, two = (self._csr_reads(r, split_breaks) for r in reads)
            reads = interleave_reads((ix._as_dev(one[0], torch.uint8), ix._as_dev(one[1], torch.int64)), two)
        csr = self._csr_reads(reads, split_breaks)
        opts = dict(align_options or {})
        mems, chains, aln = self.find_alignments(csr, minimum_length, contigs, both_strands, split_breaks, max_occ, opts, by_score=False,
                                                 **chain_options)
        sel_offsets, sel, records, klass = ix.select_alignments(csr[1], chains[0], chains[1], aln, contigs, both_strands,
                                                                **(select_options or {}))[:4]
        popts, ropts, used = dict(pair_options or {}), dict(rescue_options or {}), ()
        if insert_size is not None:
            if isinstance(insert_size, InsertSize):
                est = insert_size
            elif insert_size == "estimate" or isinstance(insert_size, dict):
                stats = ix.insert_size_stats(sel_offsets, records, **(insert_size if isinstance(insert_size, dict) else {}))[0]
                est = insert_size_options(stats.cpu(), popts)        # the added host read
            else:
                raise ValueError('insert_size must be None, "estimate", a dict of insert_size_stats\' options or an InsertSize')
            popts.update(orient=est.orient, isize_min=est.isize_min, isize_max=est.isize_max, isize_mean=est.isize_mean)
            used = (est,)
        if not rescue:
            offs, cigar, info = ix.chain_cigars(csr, mems[0], mems[1], chains, aln, sel, contigs, both_strands, **opts)
            pairs, sam, _ = ix.pair_alignments(sel_offsets, records, klass, **popts)
            return (records, sel_offsets, offs, cigar, info, pairs, sam) + used
        if not both_strands:
            raise ValueError("rescue needs both_strands: a mate is sought on the strand its partner implies")
        min_len, min_anchor = int(ropts.pop("min_len", 12)), int(ropts.pop("min_anchor_score", 40))
        where = {key: ropts.pop(key) if key in ropts else popts[key] for key in ("orient", "isize_max") if key in ropts or key in popts}
        if ropts:
            raise TypeError(f"unknown rescue option {sorted(ropts)[0]!r}")
        pairs, sam, _ = ix.pair_alignments(sel_offsets, records, klass, **popts)
        windows, planned = ix.rescue_windows(csr[1], sel_offsets, records, pairs, contigs, min_anchor_score=min_anchor, **where)
        status = torch.zeros(windows.shape[0], dtype=torch.int32, device=windows.device)
        totals = torch.zeros(3, dtype=torch.int64, device=windows.device)
        if int(planned[0].item()) > 0:                               # the one host read: is there anything to rescue?
            offsets, rows, status, totals = ix.window_mems(csr[0], csr[1], windows, min_len, mems[0], mems[1], both_strands, split_breaks)
            chains = self.chain_mems(offsets, rows, contigs, by_score=False, **chain_options)
            mems = (offsets, rows)
            aln, _ = self.align_chains(csr, offsets, rows, chains, contigs, both_strands, split_breaks, **opts)
            sel_offsets, sel, records, klass = ix.select_alignments(csr[1], chains[0], chains[1], aln, contigs, both_strands,
                                                                    **(select_options or {}))[:4]
            pairs, sam, _ = ix.pair_alignments(sel_offsets, records, klass, **popts)
        offs, cigar, info = ix.chain_cigars(csr, mems[0], mems[1], chains, aln, sel, contigs, both_strands, **opts)
        return (records, sel_offsets, offs, cigar, info, pairs, sam, (windows, status, totals)) + used

    def sam_text(self, result, reads, names, contig_names=None, quals=None, contigs=None, tags=N.SAM_NM | N.SAM_AS, seq=True):
        """The SAM records of a mapped batch as text on the device (genie_sam_text) -> (text uint8[bytes], line_offsets
        int64[n_lines + 1], totals int64[3] = (lines, bytes, unmapped lines)): GenieIndex.sam_text.  result: the tuple of
        map_pairs (7 to 9 results; only the first five and the seventh are used) or of map_records (5 results: single-end mode).  reads: the batch as that call took it,
        interleaved; strings are encoded with ExactMatch.encode_lenient whatever split_breaks that call had, so a symbol
        outside the alphabet is written N.  names: one per read, a list of str or bytes or the (bytes, offsets) of index.names_csr or
        text_reads.fastq_fields; contig_names likewise, by default contigs.names, "ref" without contigs.  quals: None (`*`),
        a list of str or bytes with one entry per read, or uint8 parallel to the bases (fastq_fields).  tags: a mask of
        _native.SAM_NM (1), SAM_AS (2), SAM_MD (4), SAM_MC (8), SAM_MQ (16); seq=False writes `*` for SEQ and QUAL."""
        return self._sam_bytes("sam_text", result, reads, names, contig_names, quals, contigs, tags, seq)

    def bam_records(self, result, reads, names, contig_names=None, quals=None, contigs=None, tags=N.SAM_NM | N.SAM_AS, seq=True):
        """The same batch as uncompressed BAM alignment records on the device (genie_bam_records) -> (data uint8[bytes],
        record_offsets int64[n + 1], totals int64[3] = (records, bytes, unmapped records)): GenieIndex.bam_records.  The
        arguments and their forms are sam_text's; one record per line of sam_text, in its order."""
        return self._sam_bytes("bam_records", result, reads, names, contig_names, quals, contigs, tags, seq)

    def _sam_bytes(self, method, result, reads, names, contig_names, quals, contigs, tags, seq):
        """sam_text and bam_records: the input forms they share, then GenieIndex's method of that name."""
        from .index import names_csr
        ix = self.matcher.index(self.lut.lut_size)
        if len(result) not in (5, 7, 8, 9):
            raise ValueError("result must be what map_pairs (7 to 9 results) or map_records (5 results) returned")
        records, sel_offsets, cigar_offsets, cigar, info = result[:5]
        sam = result[6] if len(result) > 5 else None
        bases, read_offsets = self._csr_reads(reads, True)       # strings as the split_breaks calls took them: N, code 4, is written N
        if contig_names is None:
            contig_names = contigs.names if contigs is not None else ["ref"]
        csr = lambda x: x if isinstance(x, tuple) else names_csr(x)      # noqa: E731
        if isinstance(quals, (list, tuple)):
            quals = names_csr(quals)[0]
        return getattr(ix, method)(bases, read_offsets, sel_offsets, records, sam, info, cigar_offsets, cigar, *csr(names), *csr(contig_names),
                                   quals=quals, contigs=contigs, tags=tags, seq=seq)

    def write_sam(self, path, result, reads, names, contig_names=None, contig_lengths=None, **options):
        """A SAM file: the header lines of index.sam_header, then the text of sam_text(result, reads, names, contig_names,
        **options) in one copy from the device -> totals.  contig_lengths default to those of options["contigs"], or the
        reference's length without contigs; contig_names here are a list."""
        from .index import sam_header
        contigs = options.get("contigs")
        if contig_names is None:
            contig_names = contigs.names if contigs is not None else ["ref"]
        if contig_lengths is None:
            contig_lengths = np.diff(contigs.offsets) if contigs is not None else [self.matcher.index(self.lut.lut_size).n]
        text, _, totals = self.sam_text(result, reads, names, contig_names, **options)
        with open(path, "wb") as f:
            f.write(("\n".join(sam_header(contig_names, contig_lengths)) + "\n").encode())
            f.write(text.cpu().numpy().tobytes())
        return totals

    def write_bam(self, path, result, reads, names, contig_names=None, contig_lengths=None, level=1, **options):
        """A BAM file: index.bam_header, then the records of bam_records(result, reads, names, contig_names, **options) in one
        copy from the device, the two compressed as by index.bgzf_compress at `level` and written block by block -> totals.
        Names and lengths default as in write_sam.  The records are in the order of the reads (unsorted, grouped by query), as
        the header says."""
        from .index import bam_header, bgzf_blocks
        contigs = options.get("contigs")
        if contig_names is None:
            contig_names = contigs.names if contigs is not None else ["ref"]
        if contig_lengths is None:
            contig_lengths = np.diff(contigs.offsets) if contigs is not None else [self.matcher.index(self.lut.lut_size).n]
        data, _, totals = self.bam_records(result, reads, names, contig_names, **options)
        with open(path, "wb") as f:
            for block in bgzf_blocks([bam_header(contig_names, contig_lengths), data.cpu().numpy()], level):
                f.write(block)
        return totals

    def locate_contigs(self, contigs, rows):
        """SMEM rows (start, end, lo, hi) of any find_smems* call -> (hit_offsets, hits int32[T, 2] = (contig, 1-based
        offset), dropped): GenieIndex.locate_contigs.  The rows stay SMEMs of the concatenation; occurrences that bridge two
        sequences are dropped."""
        return self.matcher.index(self.lut.lut_size).locate_contigs(contigs, rows)

    def _csr_reads(self, reads, split_breaks):
        """list[str] or (bases, read_offsets) -> (bases, read_offsets), strings encoded as match_stats encodes them."""
        if isinstance(reads, tuple):
            return reads
        encode = self.matcher.encode_lenient if split_breaks else self.matcher.encode
        enc = [encode(r) for r in reads]
        read_offsets = np.zeros(len(enc) + 1, np.int64)
        read_offsets[1:] = np.cumsum([len(e) for e in enc]) if enc else []
        return (np.concatenate(enc).astype(np.uint8) if enc else np.zeros(0, np.uint8)), read_offsets

    def match_stats_contigs(self, contigs, reads, intervals=True, both_strands=False, split_breaks=False):
        """match_stats that is exact with respect to a reference of several sequences (genie_match_stats_contigs): contigs is
        the ReferenceSet whose concatenation this matcher's reference is.  reads as match_stats.  -> (ms, lohi, status,
        clipped): ms the longest match from each position that lies inside ONE contig, lohi its interval in the concatenation,
        clipped the number of positions where that is shorter than match_stats's answer."""
        bases, read_offsets = self._csr_reads(reads, split_breaks)
        return self.matcher.index(self.lut.lut_size).match_stats_contigs(contigs, bases, read_offsets, intervals, both_strands,
                                                                         split_breaks)

    def find_smems_contigs(self, contigs, reads, minimum_length=1, mode="bwa", both_strands=False, split_breaks=False):
        """find_smems_long whose rows are the SMEMs with respect to the SET of sequences (genie_find_smems_contigs): no row
        relies on a match that bridges two contigs, so every row has a hit in locate_contigs.  reads and options as
        find_smems_long.  -> (offsets, smems[S, 4], status, clipped)."""
        bases, read_offsets = self._csr_reads(reads, split_breaks)
        return self.matcher.index(self.lut.lut_size).find_smems_contigs(contigs, mode, bases, read_offsets, minimum_length,
                                                                        both_strands=both_strands, split_breaks=split_breaks)

    def match_stats_min_occ(self, reads, min_occ, intervals=True, both_strands=False, split_breaks=False):
        """match_stats of what occurs at least min_occ times in the reference (genie_match_stats_min_occ).  reads as
        match_stats.  -> (ms, lohi, status, shortened): ms the longest match from each position whose interval lohi has at
        least min_occ rows, shortened the number of positions where that is shorter than match_stats's answer."""
        bases, read_offsets = self._csr_reads(reads, split_breaks)
        return self.matcher.index(self.lut.lut_size).match_stats_min_occ(bases, read_offsets, min_occ, intervals, both_strands,
                                                                         split_breaks)

    def find_smems_min_occ(self, reads, min_occ, minimum_length=1, mode="bwa", both_strands=False, split_breaks=False,
                           rows_hint=None):
        """find_smems_long under a minimum occurrence count, BWA-MEM's min_intv (genie_find_smems_min_occ): the matches of
        at least min_occ occurrences that no other such match contains.  reads and options as find_smems_long.
        -> (offsets, smems[S, 4], status, shortened)."""
        bases, read_offsets = self._csr_reads(reads, split_breaks)
        return self.matcher.index(self.lut.lut_size).find_smems_min_occ(mode, bases, read_offsets, min_occ, minimum_length,
                                                                        rows_hint=rows_hint, both_strands=both_strands,
                                                                        split_breaks=split_breaks)

    def match_stats_text(self, data, fmt="lines", intervals=True, both_strands=False, split_breaks=True, fold_case=False):
        """match_stats of the reads in a text (find_smems_text's formats and translation) -> (ms, lohi, status,
        read_offsets): read_offsets int64[N+1] on the device, to index the flat arrays with."""
        ix = self.matcher.index(self.lut.lut_size)
        bases, read_offsets, _ = reads_from_text(data, fmt, self.matcher.byte_codes(fold_case), False, ix.device)
        return ix.match_stats(bases, read_offsets, intervals, both_strands, split_breaks) + (read_offsets,)

    def iter_text_smems(self, path, fmt, chunk_bytes=64 << 20, mode="bwa", minimum_length=1, both_strands=False, split_breaks=True,
                        fold_case=False):
        """find_smems_text over a file of any size, a chunk at a time: yields (offsets, smems, status) of the reads (records)
        that are complete in each chunk of about chunk_bytes bytes; the unfinished one at a chunk's end is carried into the
        next chunk.  A chunk that holds no complete read grows by another chunk_bytes until it does (or the file ends), and
        is parsed again from its start each time it grows: one record much larger than chunk_bytes (a chromosome in a
        FASTA file) is re-parsed once per growth step, so choose chunk_bytes above the largest record.  The concatenated
        reads are those of find_smems_text on the whole file."""
        chunk_bytes = max(int(chunk_bytes), 1)
        opts = (mode, minimum_length, both_strands, split_breaks, fold_case)
        with open(path, "rb") as fh:
            carry = b""
            while True:
                fresh = fh.read(chunk_bytes)
                last = len(fresh) < chunk_bytes                     # a short read of a regular file: its end
                buf = carry + fresh
                if last:
                    if buf:
                        yield self._find_text(buf, fmt, False, *opts)[:3]
                    return
                offsets, smems, status, n_reads, consumed = self._find_text(buf, fmt, True, *opts)
                carry = buf[consumed:]                              # no complete record: everything, and the chunk grows
                if n_reads:
                    yield offsets, smems, status

    def iter_fastq_smems(self, path, chunk_bytes=64 << 20, mode="bwa", minimum_length=1, both_strands=False, split_breaks=True,
                         fold_case=False):
        """iter_text_smems over a FASTQ file (four-line records)."""
        return self.iter_text_smems(path, "fastq", chunk_bytes, mode, minimum_length, both_strands, split_breaks, fold_case)

    def iter_fasta_smems(self, path, chunk_bytes=64 << 20, mode="bwa", minimum_length=1, both_strands=False, split_breaks=True,
                         fold_case=False):
        """iter_text_smems over a FASTA file ('>' header lines, sequences wrapped over any number of lines)."""
        return self.iter_text_smems(path, "fasta", chunk_bytes, mode, minimum_length, both_strands, split_breaks, fold_case)

    def find_smems_lut(self, reads, lens=None):
        return self._find("lut", reads, lens, 1)

    def find_smems_rmi(self, reads, lens=None):
        return self._find("rmi", reads, lens, 1)

    # ------------------------------------------------------------------ reference API (per query)
    def _one(self, mode, query, min_len=1):
        codes = self.matcher.encode(query)                    # KeyError for an unknown base
        if len(codes) == 0:
            if mode == "bwa":
                return {}
            raise KeyError("")                                # SMEM.py:39 on an empty query
        if len(codes) > N.MAX_READ_LEN:                       # past the fixed-stride path's limit: the long-read path
            ix = self.matcher.index(self.lut.lut_size)
            offsets, smems, status = ix.find_smems_long(mode, codes, np.asarray([0, len(codes)], np.int64), min_len)
        else:
            offsets, smems, status = self._find(mode, codes.reshape(1, -1), None, min_len)
        st = int(status[0].item())
        if st == N.READ_ABSENT_BASE:
            raise KeyError("")            # reference: forward_match[0][""] (SMEM.py:39) / runaway loop
        if st == N.READ_TOO_SHORT:
            raise ValueError("query shorter than the LUT key size (the reference mis-encodes it, SMEM.py:26-28)")
        if st != N.READ_OK:
            raise RuntimeError(f"genie_find_smems: read status {st}")
        out = {}
        for s, e, lo, hi in smems.cpu().numpy().tolist():
            out[query[s:e]] = (lo, hi)
        return out

    def get_suffix_index(self, query):
        return self.matcher.exact_match_back_prop(query)

    def get_smems_lut(self, query):
        return self._one("lut", query)

    def get_smems_rmi(self, query):
        return self._one("rmi", query)

    def get_SMEMS(self, query, minimum_length):
        return self._one("bwa", query, minimum_length)

    @staticmethod
    def check_sequential(list1, list2):
        """SMEM.py:196-202."""
        s2 = set(list2)
        return any(item1 + 1 in s2 for item1 in list1)

    def forward_extension(self, query, start_index, largest="", suffix_tuple=None):
        """SMEM.py:425-443: ({every matching string: interval}, longest).  All prefixes are
        searched in ONE batched device call instead of one backward search per step."""
        forward_matches = {}
        if suffix_tuple is not None:
            forward_matches[largest] = suffix_tuple
        pats = [largest + query[start_index:i] for i in range(start_index + 1, len(query) + 1)]
        if not pats:
            return forward_matches, largest
        res = self.matcher.exact_match_batch(pats)
        longest = largest
        for p, (lo, hi) in zip(pats, res.tolist()):
            if lo < 0:
                return forward_matches, p[:-1]
            forward_matches[p] = (lo, hi)
            longest = p
        return forward_matches, longest

    def backward_extension(self, query, start_index, forward_matches):
        """SMEM.py:389-423."""
        largest, suffix_of_largest, end_index = "", None, -1
        largest_forward = ""
        keys = list(forward_matches)
        pats, owner = [], []
        for key in keys:
            for i in range(start_index - 1, -1, -1):
                pats.append(query[i:start_index] + key)
                owner.append(key)
        res = self.matcher.exact_match_batch(pats).tolist() if pats else []
        pos = 0
        for key in keys:
            if len(key) > len(largest_forward):
                largest_forward = key
            broken = False
            for i in range(start_index - 1, -1, -1):
                lo, hi = res[pos]
                cur = pats[pos]
                pos += 1
                if broken:
                    continue
                if lo < 0:
                    broken = True
                    continue
                if len(cur) > len(largest):
                    largest, suffix_of_largest, end_index = cur, (lo, hi), start_index + len(key)
        if len(largest_forward) > len(largest):
            largest = largest_forward
            suffix_of_largest = forward_matches[largest_forward]
            end_index = start_index + len(largest_forward)
        return largest, suffix_of_largest, end_index

    def get_SMEM_at_index(self, query, start_index):
        """SMEM.py:469-484."""
        forward_extension = self.forward_extension(query, start_index)
        largest_backward = self.backward_extension(query, start_index, forward_extension[0])
        if len(forward_extension[1]) > len(largest_backward[0]):
            return [forward_extension[1], forward_extension[0][forward_extension[1]],
                    len(forward_extension[1]) + start_index]
        return [largest_backward[0], largest_backward[1], largest_backward[2]]


def create_random_query(query_size):
    """SMEM.py:489-493."""
    return "".join(random.choice(["A", "G", "C", "T"]) for _ in range(query_size))


def create_query_from_ref(ref_seq, query_size):
    """SMEM.py:496-505."""
    ref_size = len(ref_seq)
    query = ""
    while len(query) < query_size:
        position = random.randint(0, ref_size)
        size = random.randint(1, 30)
        if size + position > ref_size:
            continue
        query += ref_seq[position: position + size]
    return query[:query_size]
