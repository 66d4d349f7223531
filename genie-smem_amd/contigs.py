"""ReferenceSet: a reference of several sequences (chromosomes, scaffolds, plasmids) as the library takes it -- the
concatenation of their base codes, the contig table (int64 offsets, the convention of a read batch's read_offsets) and
the records' names.  One GenieIndex is built over the concatenation; find_mems_contigs, locate_contigs and contig_coords
take the ReferenceSet next to it and answer per sequence (include/genie_smem.h, "A reference of SEVERAL sequences")."""
import ctypes as C

import numpy as np
import torch

from . import _native as N
from .index import GenieIndex, _ptr, _stream
from .text_reads import record_names, reads_from_text

_CODE = {"A": 0, "C": 1, "G": 2, "T": 3}
_LETTER_CODE = np.full(256, 4, np.uint8)                   # A C G T in either case -> 0 1 2 3, every other byte a break
for _ch, _code in _CODE.items():
    _LETTER_CODE[ord(_ch)] = _LETTER_CODE[ord(_ch.lower())] = _code


def _check_ambiguous(ambiguous):
    if ambiguous not in ("error", "cut"):
        raise ValueError(f"ambiguous must be 'error' or 'cut', got {ambiguous!r}")


def cut_segments(codes, record_offsets):
    """The cut of genie_reference_segments in numpy, on the host: codes uint8 (a code > 3 is a break), record_offsets int64
    [records + 1] -> (bases, seg_offsets, seg_record, seg_origin): the kept codes back to back, the kept codes in front of
    every segment (one more value: their number), each segment's record and the 0-based offset of its first base in it."""
    codes = np.ascontiguousarray(codes, np.uint8).reshape(-1)
    off = np.ascontiguousarray(record_offsets, np.int64)
    if off.ndim != 1 or off.size < 2 or off[0] != 0 or off[-1] != codes.size or (np.diff(off) < 0).any():
        raise ValueError("record_offsets must start at 0, never decrease and end at the number of codes")
    keep = codes <= 3
    start = keep.copy()
    start[1:] &= ~keep[:-1]                                # the base in front is a break ...
    at = off[off < codes.size]
    start[at] |= keep[at]                                  # ... or a record starts here
    first = np.flatnonzero(start).astype(np.int64)
    before = np.cumsum(keep, dtype=np.int64) - keep        # kept codes in front of every position
    seg_offsets = np.append(before[first], np.int64(keep.sum())).astype(np.int64)
    seg_record = (np.searchsorted(off, first, side="right") - 1).astype(np.int32)
    return codes[keep], seg_offsets, seg_record, first - off[seg_record]


def reference_segments(codes, record_offsets=None, device="cuda"):
    """genie_reference_segments on the device: codes uint8 (host or device; a code > 3 is a break), record_offsets int64
    [records + 1] or None (one record) -> (bases uint8 [n_kept], seg_offsets int64 [n_seg + 1], seg_record int32 [n_seg],
    seg_origin int64 [n_seg], longest segment): four tensors on `device` and a count.  Two native calls: one sizes the
    outputs, one fills them.  A table that does not start at 0, decreases or does not end at len(codes) is a ValueError."""
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError("reference_segments runs on an MI355X only (no CPU fallback); device is " + str(device))
    if device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    if not isinstance(codes, torch.Tensor):
        codes = torch.as_tensor(np.ascontiguousarray(codes, np.uint8))
    codes = codes.to(device=device, dtype=torch.uint8).contiguous().view(-1)
    n_records = 1
    if record_offsets is not None:
        if not isinstance(record_offsets, torch.Tensor):
            record_offsets = torch.as_tensor(np.ascontiguousarray(record_offsets, np.int64))
        record_offsets = record_offsets.to(device=device, dtype=torch.int64).contiguous().view(-1)
        n_records = record_offsets.numel() - 1
    lib = N.lib()
    n_given = codes.numel()
    tmp_bytes = int(lib.genie_reference_segments_tmp_bytes(n_given, n_records))
    if tmp_bytes < 0:
        raise N.GenieError(tmp_bytes, "genie_reference_segments_tmp_bytes")
    tmp = torch.empty(max(tmp_bytes, 256), dtype=torch.uint8, device=device)
    out4 = (C.c_int64 * 4)()
    ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None and t.numel() else C.c_void_p(0)      # noqa: E731

    def call(bases, seg_offsets, seg_record, seg_origin, cap_bases, cap_segs):
        with torch.cuda.device(device):
            rc = lib.genie_reference_segments(ptr(codes), n_given, ptr(record_offsets), n_records, ptr(bases), cap_bases,
                                              ptr(seg_offsets), ptr(seg_record), ptr(seg_origin), cap_segs, out4, ptr(tmp), tmp_bytes,
                                              _stream(device))
        if rc == -1 and out4[3]:
            raise ValueError(f"record_offsets is no table of {n_given} codes (genie_contigs_validate's conditions: mask {out4[3]})")
        N.check(rc, "genie_reference_segments")

    call(None, None, None, None, 0, 0)
    n_seg, n_kept, longest = int(out4[0]), int(out4[1]), int(out4[2])
    bases = torch.empty(max(n_kept, 1), dtype=torch.uint8, device=device)        # a pointer even for nothing
    seg_offsets = torch.empty(n_seg + 1, dtype=torch.int64, device=device)
    seg_record = torch.empty(max(n_seg, 1), dtype=torch.int32, device=device)
    seg_origin = torch.empty(max(n_seg, 1), dtype=torch.int64, device=device)
    call(bases, seg_offsets, seg_record, seg_origin, n_kept, n_seg)
    return bases[:n_kept], seg_offsets, seg_record[:n_seg], seg_origin[:n_seg], longest


class ReferenceSet:
    def __init__(self, names, offsets, codes):
        """names: list[str]; offsets: int64 numpy [len(names) + 1]; codes: uint8 base codes 0..3 of the concatenation, a
        numpy array (host) or a torch tensor (device)."""
        self.names = list(names)
        self.offsets = np.ascontiguousarray(offsets, np.int64)
        self.codes = codes
        self._dev = {}
        self.index = None               # the GenieIndex build_index made last
        if self.offsets.ndim != 1 or self.offsets.size != len(self.names) + 1 or self.offsets.size < 2:
            raise ValueError("a ReferenceSet needs at least one record and one offset more than names")

    def __len__(self):
        return len(self.names)

    @property
    def n(self):
        return int(self.offsets[-1])

    @classmethod
    def from_sequences(cls, sequences, names=None, ambiguous="error"):
        """list[str] of A/C/G/T (either case; a record may be empty), on the host.  names default to "0", "1", ...
        ambiguous: "error" refuses any other letter; "cut" takes every other letter (N, IUPAC codes) as a break and returns
        a SegmentedReferenceSet, cut here in numpy."""
        _check_ambiguous(ambiguous)
        sequences = list(sequences)
        names = [str(i) for i in range(len(sequences))] if names is None else [str(x) for x in names]
        if len(names) != len(sequences):
            raise ValueError("one name per sequence")
        if not sequences:
            raise ValueError("a ReferenceSet needs at least one record")
        if ambiguous == "cut":
            given = np.concatenate([_LETTER_CODE[np.frombuffer(seq.encode("latin-1", "replace"), np.uint8)] for seq in sequences])
            record_offsets = np.zeros(len(sequences) + 1, np.int64)
            record_offsets[1:] = np.cumsum([len(seq) for seq in sequences])
            return SegmentedReferenceSet(names, record_offsets, *cut_segments(given, record_offsets))
        parts = []
        for name, seq in zip(names, sequences):
            try:
                parts.append(np.fromiter((_CODE[ch] for ch in seq.upper()), np.uint8, len(seq)))
            except KeyError as e:
                raise ValueError(f"reference record {name!r} holds {e.args[0]!r}: only A, C, G and T are supported") from None
        offsets = np.zeros(len(parts) + 1, np.int64)
        offsets[1:] = np.cumsum([p.size for p in parts])
        return cls(names, offsets, np.concatenate(parts).astype(np.uint8))

    @classmethod
    def from_fasta(cls, data, device="cuda", ambiguous="error"):
        """A multi-FASTA text (bytes-like or numpy uint8 on the host), cut and translated on the device
        (text_reads.reads_from_text): the codes stay there, for build_index to build from where they lie.  ambiguous:
        "error" refuses a letter other than A, C, G and T; "cut" takes it as a break and returns a SegmentedReferenceSet,
        squeezed and cut on the device (reference_segments)."""
        _check_ambiguous(ambiguous)
        bases, offsets, _, starts = reads_from_text(data, "fasta", _LETTER_CODE, False, device, return_starts=True)
        if offsets.numel() < 2:
            raise ValueError("the FASTA text holds no record")
        names = [x.decode("ascii", "replace") for x in record_names(data, starts)]
        host = offsets.cpu().numpy()
        if ambiguous == "cut":
            kept, seg_offsets, seg_record, seg_origin, _ = reference_segments(bases, offsets, bases.device)
            self = SegmentedReferenceSet(names, host, kept, seg_offsets.cpu().numpy(), seg_record.cpu().numpy(), seg_origin.cpu().numpy())
            self._dev[seg_offsets.device] = seg_offsets
            self._dev_segments[seg_offsets.device] = (seg_record, seg_origin)
            return self
        bad = torch.nonzero(bases > 3)
        if bad.numel():
            at = int(bad[0].item())
            rec = int(np.searchsorted(host, at, side="right")) - 1
            raise ValueError(f"reference record {names[rec]!r} holds a base other than A, C, G and T (base {at - int(host[rec]) + 1})")
        self = cls(names, host, bases)
        self._dev[offsets.device] = offsets
        return self

    def device_offsets(self, device):
        """The table on `device` (uploaded once)."""
        device = torch.device(device)
        if device not in self._dev:
            self._dev[device] = torch.as_tensor(self.offsets).to(device)
        return self._dev[device]

    def build_index(self, K, dir_bits=7, table_bits=0, table_format="auto", device="cuda"):
        """The GenieIndex of the concatenation, on the device: built there when the codes lie there (from_fasta), else by
        the host builder and uploaded.  The table is then checked against it (genie_contigs_validate)."""
        if isinstance(self.codes, torch.Tensor) and self.codes.device.type == "cuda":
            ix = GenieIndex.build_on_device(self.codes, K, dir_bits, table_bits, table_format, device=self.codes.device)
        else:
            codes = self.codes.cpu().numpy() if isinstance(self.codes, torch.Tensor) else self.codes
            ix = GenieIndex.build(codes, K, dir_bits, table_bits=table_bits, table_format=table_format).to(device)
        off = self.device_offsets(ix.device)
        with torch.cuda.device(ix.device):
            N.check(N.lib().genie_contigs_validate(ix._h, _ptr(off), off.numel() - 1, _stream(ix.device)), "genie_contigs_validate")
        self.index = ix
        return ix

    def coords(self, pos, stride=1, index=None):
        """1-based concatenation positions (MEM rows' pos column, a locate result) -> int32 [count, 2] (contig, 1-based
        offset inside it) on the device: GenieIndex.contig_coords on `index`, by default the one build_index made."""
        ix = self.index if index is None else index
        if ix is None:
            raise RuntimeError("ReferenceSet.coords needs an index: call build_index first or pass index=")
        return ix.contig_coords(self, pos, stride)

    def name_of(self, contig):
        return self.names[int(contig)]


class SegmentedReferenceSet(ReferenceSet):
    """A reference with ambiguous bases (ReferenceSet.from_sequences / from_fasta with ambiguous="cut"): every letter other
    than A, C, G and T is a break, the breaks are removed and the reference is cut at them and at the record boundaries
    into SEGMENTS (include/genie_smem.h, "A reference with AMBIGUOUS BASES").  `codes` is the squeezed concatenation and
    `offsets` the SEGMENT table, so build_index and every *_contigs method of GenieIndex and SMEM take the object as it is
    and answer per segment; coords and hit_coords then name positions in the records as they were given, breaks counted.
    names, record_offsets: the given records; seg_record, seg_origin: every segment's record and the 0-based offset of its
    first base inside it (numpy, host)."""

    def __init__(self, names, record_offsets, codes, seg_offsets, seg_record, seg_origin):
        self.names = list(names)
        self.record_offsets = np.ascontiguousarray(record_offsets, np.int64)
        self.offsets = np.ascontiguousarray(seg_offsets, np.int64)
        self.seg_record = np.ascontiguousarray(seg_record, np.int32)
        self.seg_origin = np.ascontiguousarray(seg_origin, np.int64)
        self.codes = codes
        self._dev = {}
        self._dev_segments = {}
        self.index = None
        if self.record_offsets.ndim != 1 or self.record_offsets.size != len(self.names) + 1 or self.record_offsets.size < 2:
            raise ValueError("a ReferenceSet needs at least one record and one offset more than names")
        if self.offsets.size != self.seg_record.size + 1 or self.seg_origin.size != self.seg_record.size:
            raise ValueError("a segment table needs one offset more than segments")
        if self.n_segments == 0:
            raise ValueError("the reference holds no A, C, G or T at all")

    @property
    def n_segments(self):
        return int(self.seg_record.size)

    @property
    def n_given(self):
        return int(self.record_offsets[-1])

    def device_segments(self, device):
        """(seg_record, seg_origin) on `device` (uploaded once)."""
        device = torch.device(device)
        if device not in self._dev_segments:
            self._dev_segments[device] = (torch.as_tensor(self.seg_record).to(device), torch.as_tensor(self.seg_origin).to(device))
        return self._dev_segments[device]

    def _index(self, index, what):
        ix = self.index if index is None else index
        if ix is None:
            raise RuntimeError(f"SegmentedReferenceSet.{what} needs an index: call build_index first or pass index=")
        return ix

    def coords(self, pos, stride=1, index=None):
        """1-based positions in the squeezed concatenation (MEM rows' pos column, a locate result) -> int64 [count, 2]
        (record, 1-based offset inside the given record, breaks counted) on the device: GenieIndex.segment_coords on
        `index`, by default the one build_index made."""
        return self._index(index, "coords").segment_coords(self, pos, "positions", stride)

    def hit_coords(self, hits, index=None):
        """locate_contigs hits [T, 2] (segment, 1-based offset inside it) -> int64 [T, 2] as coords gives them."""
        return self._index(index, "hit_coords").segment_coords(self, hits, "hits")
