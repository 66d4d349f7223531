"""ReferenceSet: a reference of several sequences (chromosomes, scaffolds, plasmids) as the library takes it -- the
concatenation of their base codes, the contig table (int64 offsets, the convention of a read batch's read_offsets) and
the records' names.  One GenieIndex is built over the concatenation; find_mems_contigs, locate_contigs and contig_coords
take the ReferenceSet next to it and answer per sequence (include/genie_smem.h, "A reference of SEVERAL sequences")."""
import numpy as np
import torch

from . import _native as N
from .index import GenieIndex, _ptr, _stream
from .text_reads import record_names, reads_from_text

_CODE = {"A": 0, "C": 1, "G": 2, "T": 3}


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
    def from_sequences(cls, sequences, names=None):
        """list[str] of A/C/G/T (either case; a record may be empty), on the host.  names default to "0", "1", ..."""
        sequences = list(sequences)
        names = [str(i) for i in range(len(sequences))] if names is None else [str(x) for x in names]
        if len(names) != len(sequences):
            raise ValueError("one name per sequence")
        if not sequences:
            raise ValueError("a ReferenceSet needs at least one record")
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
    def from_fasta(cls, data, device="cuda"):
        """A multi-FASTA text (bytes-like or numpy uint8 on the host), cut and translated on the device
        (text_reads.reads_from_text): the codes stay there, for build_index to build from where they lie."""
        table = np.full(256, 4, np.uint8)
        for ch, code in _CODE.items():
            table[ord(ch)] = table[ord(ch.lower())] = code
        bases, offsets, _, starts = reads_from_text(data, "fasta", table, False, device, return_starts=True)
        if offsets.numel() < 2:
            raise ValueError("the FASTA text holds no record")
        names = [x.decode("ascii", "replace") for x in record_names(data, starts)]
        host = offsets.cpu().numpy()
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
