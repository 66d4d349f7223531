"""The raw ctypes calls of genie_reads_from_text, genie_reads_from_fasta and genie_reference_segments, which share one shape,
name(d_input, input_bytes, *middle, d_bases, cap_bases, *d_items, cap_items, out, d_tmp, tmp_bytes, stream), and one protocol:
the sizing call (no outputs) reports n_items = out[0] and n_bases = out[1], the full call fills buffers of those sizes.
text_util, fasta_util and segment_util bind a Call each and keep their models and their cases."""
import ctypes as C

import numpy as np

ITEM_FILL = -7                  # what the item arrays hold before the call
SPARE = 8                       # elements behind every output that the call is not told of


def _vp(address):
    return C.c_void_p(address) if address else None


def same(got, want, names):
    """A driver's (status, out, *arrays) against the model's: status and out always, the arrays when the model's status is 0."""
    assert got[:2] == want[:2], (got[:2], want[:2])
    for g, w, name in zip(got[2:], want[2:], names if want[0] == 0 else ()):
        assert np.array_equal(g, w), name
    return want


class Call:
    """items: (dtype name, elements beyond cap_items that the call owns) of each item array; null_cap: the sizing call's capacities."""

    def __init__(self, name, items, nout, null_cap=0):
        self.name, self.items, self.nout, self.null_cap = name, tuple(items), nout, null_cap

    def tmp_bytes(self, lib, input_bytes, count):
        return int(getattr(lib, self.name + "_tmp_bytes")(input_bytes, count))

    def raw(self, lib, input_ptr, input_bytes, middle, bases_ptr, cap_bases, item_ptrs, cap_items, tmp_ptr, tmp_len, stream=None):
        """One call on raw addresses (0: NULL) -> (status, out as a list)."""
        out = (C.c_int64 * self.nout)(*[-99] * self.nout)
        rc = getattr(lib, self.name)(_vp(input_ptr), input_bytes, *middle, _vp(bases_ptr), cap_bases, *map(_vp, item_ptrs), cap_items,
                                     out, _vp(tmp_ptr), tmp_len, _vp(stream))
        return rc, list(out)

    def run(self, lib, data, middle, tmp_bytes, cap_bases=None, cap_items=None, sizing=False, lead=0, fill=0xA5, spare=SPARE):
        """The sizing call (unless both capacities are given), then the full call, on the current torch stream: the input `lead`
        bytes behind a 16-byte boundary, the scratch (tmp_bytes(cap_items) bytes) and the outputs filled first, the outputs `spare`
        elements longer than the call is told (None: told what the sizing call reported) -> (status, out) of the sizing call with
        sizing=True, else (status, out, bases, [item arrays]), the arrays whole.  Asserts that the two calls agree on every word of
        out (on the status too, with no capacity given) and that the slack behind every output keeps its fill."""
        import torch
        data = np.frombuffer(bytes(data), np.uint8) if isinstance(data, (bytes, bytearray)) else np.asarray(data, np.uint8)
        n = data.size
        whole = torch.zeros(n + 16, dtype=torch.uint8, device="cuda")
        whole[lead:lead + n].copy_(torch.from_numpy(data.copy()))
        ptr = whole.data_ptr() + lead if n else 0

        def call(cap_bases, cap_items, bases, arrays):
            tb = int(tmp_bytes(max(cap_items, 0)))
            assert tb > 0 and tb % 256 == 0
            tmp = torch.full((tb,), fill, dtype=torch.uint8, device="cuda")
            return self.raw(lib, ptr, n, middle, bases, cap_bases, arrays, cap_items, tmp.data_ptr(), tb, torch.cuda.current_stream().cuda_stream)

        given = (cap_bases is not None) + (cap_items is not None)
        size = None if given == 2 and not sizing else call(self.null_cap, self.null_cap, 0, [0] * len(self.items))
        if sizing:
            return size
        cap_items = size[1][0] if cap_items is None else cap_items
        cap_bases = size[1][1] if cap_bases is None else cap_bases
        bases = torch.full((cap_bases + spare,), fill, dtype=torch.uint8, device="cuda")
        arrays = [torch.full((cap_items + own + spare,), ITEM_FILL, dtype=getattr(torch, dt), device="cuda") for dt, own in self.items]
        rc, out = call(cap_bases, cap_items, bases.data_ptr(), [a.data_ptr() for a in arrays])     # it waits for the stream itself
        assert size is None or (out == size[1] and (rc == size[0] or given)), "the sizing call and the full call disagree"
        b, arrays = bases.cpu().numpy(), [a.cpu().numpy() for a in arrays]
        assert (b[min(max(out[1], 0), cap_bases):] == fill).all(), "written past the bases"
        for a, (_, own) in zip(arrays, self.items):
            assert (a[min(max(out[0], 0), cap_items) + own:] == ITEM_FILL).all(), "written past the outputs"
        return rc, out, b, arrays
