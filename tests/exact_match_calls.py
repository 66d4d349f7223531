"""Raw ctypes calls of genie_exact_match for the GPU tests: on torch buffers of exactly the declared sizes, and on the guarded
buffers of tests/guarded.py the way tests/contract_calls.py makes the other calls."""
import ctypes as C

import numpy as np

BOTH = 1


def call(lib, ix, flags, bases, offs, max_len=None, total=None, counts=True, status=True, fill=-7, want_rc=0):
    """One raw call: the workspace exactly what its size function returns, every output filled with `fill` first ->
    (lohi, counts or None, status or None) as numpy; None when want_rc is an error.  total: total_bases, by default the
    size of `bases`."""
    import torch
    bases, offs = np.asarray(bases, np.uint8), np.asarray(offs, np.int64)
    n = offs.size - 1
    total = int(bases.size) if total is None else total
    strands = 2 if flags & BOTH else 1
    if max_len is None:
        max_len = int(np.diff(offs).max()) if n else 0
    b = torch.as_tensor(bases if bases.size else np.zeros(1, np.uint8)).cuda()
    of = torch.as_tensor(offs).cuda()
    ws_bytes = lib.genie_exact_match_workspace_bytes(n, total, max_len, flags)
    assert ws_bytes >= 0 and ws_bytes % 256 == 0
    assert ws_bytes <= lib.genie_match_stats_workspace_bytes(n, total, max_len, flags)
    ws = torch.empty(max(ws_bytes, 1), dtype=torch.uint8, device="cuda")
    lohi = torch.full((strands * n, 2), fill, dtype=torch.int32, device="cuda")
    cnt = torch.full((strands * n,), fill, dtype=torch.int32, device="cuda") if counts else None
    st = torch.full((strands * n,), fill, dtype=torch.int32, device="cuda") if status else None
    p = lambda t: C.c_void_p(t.data_ptr() if t is not None and t.numel() else 0)      # noqa: E731
    rc_ = lib.genie_exact_match(ix._h, flags, p(b) if total else C.c_void_p(0), p(of), n, total, max_len, p(lohi), p(cnt), p(st),
                                p(ws), ws_bytes, C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert rc_ == want_rc, rc_
    if rc_:
        return None
    return lohi.cpu().numpy(), (cnt.cpu().numpy() if counts else None), (st.cpu().numpy() if status else None)


def guarded_call(lib, ix, a, s, flags, pats, lead=0, tail=0, counts=True, status=True):
    """The call on guarded buffers: inputs frozen, every output and the workspace cut from the arena `a` with exactly the
    declared bytes and the weakest alignment the header allows (d_lohi 8 but not 16, d_counts / d_status 4 but not 8, the
    workspace 256 but not 512), ONE call on stream `s` without synchronising -> a contract_calls.Call.  The workspace
    holds the arena's poison."""
    import contract_calls as CC
    import exact_match_util as EM
    from guarded import as_numpy
    bases, offs = EM.csr(pats, lead, tail, fill=3)
    n, total = len(pats), int(bases.size)
    strands = 2 if flags & BOTH else 1
    max_len = max([len(p) for p in pats] + [0])
    p = CC._inp(a, "bases", bases)
    po = CC._inp(a, "pat_offsets", offs, 8)
    lohi = a.alloc("lohi", strands * n * 8, 8)
    cnt = a.alloc("counts", strands * n * 4, 4) if counts else None
    st = a.alloc("status", strands * n * 4, 4) if status else None
    need = lib.genie_exact_match_workspace_bytes(n, total, max_len, flags)
    w, wb = CC._workspace(a, need, None)
    rc_ = lib.genie_exact_match(ix._h, flags, CC._vp(p), CC._vp(po), n, total, max_len, CC._vp(a.addr("lohi")),
                                CC._vp(a.addr("counts") if counts else 0), CC._vp(a.addr("status") if status else 0), CC._vp(w), wb,
                                CC._vp(s))

    def collect():
        res = {"lohi": as_numpy(lohi, np.int32, (strands * n, 2))}
        if counts:
            res["counts"] = as_numpy(cnt, np.int32)
        if status:
            res["status"] = as_numpy(st, np.int32)
        return res
    return CC.Call("exact_match", rc_, collect)
