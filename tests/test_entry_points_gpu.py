"""GPU tests of the GenieIndex batch plumbing shared by the SMEM entry points (run with -m gpu on an MI355X): the checks of
the [N, stride] batch and its lengths, the results of empty batches (N = 0) and of empty reads (stride 0) -- shapes, dtypes,
device and offsets -- and the rerun with the exact size when the first row capacity is too small."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    import genie_smem_amd as g
    from genie_smem_amd import synth
    codes = synth.synth_ref(20_000, 20_000)
    ix = g.GenieIndex.build(codes, 11).to("cuda")
    return g, ix, codes


def _like(ix, t, shape, dtype):
    assert tuple(t.shape) == tuple(shape) and t.dtype == dtype and t.device == ix.device, (t.shape, t.dtype, t.device)


# each batch method, called on reads (and lengths) only
_CALLS = {
    "sa_interval": lambda ix, r, l: ix.sa_interval(r, l),
    "find_smems_slots": lambda ix, r, l: ix.find_smems_slots("bwa", r, l),
    "find_smems": lambda ix, r, l: ix.find_smems("bwa", r, l),
    "find_smems_both": lambda ix, r, l: ix.find_smems_both("bwa", r, l),
    "find_smems_split": lambda ix, r, l: ix.find_smems_split(r, l),
}


@pytest.mark.parametrize("name", list(_CALLS))
def test_batch_checks(env, name):
    _, ix, _ = env
    call = _CALLS[name]
    what = "pat" if name == "sa_interval" else "read"
    reads = np.zeros((4, 20), np.uint8)
    with pytest.raises(ValueError, match=f"{what}s must be \\[N, stride\\]"):
        call(ix, np.zeros(20, np.uint8), None)
    with pytest.raises(ValueError, match=f"{'pattern' if what == 'pat' else 'read'} length outside \\[0, stride\\]"):
        call(ix, reads, np.asarray([20, 21, 3, 0], np.int32))
    with pytest.raises(ValueError, match="length outside"):
        call(ix, reads, np.asarray([20, -1, 3, 0], np.int32))


def test_empty_batches(env):
    import torch
    _, ix, _ = env
    i32, i64 = torch.int32, torch.int64
    for stride in (0, 150):
        none = np.zeros((0, stride), np.uint8)
        _like(ix, ix.sa_interval(none), (0, 2), i32)
        c, s, st = ix.find_smems_slots("bwa", none)
        _like(ix, c, (0,), i32), _like(ix, s, (0, max(stride, 1), 4), i32), _like(ix, st, (0,), i32)
        for off, sm, st in (ix.find_smems("bwa", none), ix.find_smems_both("lut", none), ix.find_smems_split(none)):
            _like(ix, off, (1,), i64), _like(ix, sm, (0, 4), i32), _like(ix, st, (0,), i32)
            assert off.cpu().tolist() == [0]
    off, sm, st = ix.find_smems_long("bwa", np.zeros(0, np.uint8), np.zeros(1, np.int64))
    _like(ix, off, (1,), i64), _like(ix, sm, (0, 4), i32), _like(ix, st, (0,), i32)
    assert off.cpu().tolist() == [0]
    for rb in (6, 8):
        c8, s8, r8, esc = ix.find_smems_packed("lut", np.zeros((0, 40), np.uint8), 150, row_bytes=rb)
        _like(ix, c8, (0,), torch.uint8), _like(ix, s8, (0,), torch.uint8)
        _like(ix, r8, (0, rb), torch.uint8), _like(ix, esc, (0, 2), i64)


def test_empty_reads(env):
    """Three reads of no bases (stride 0): no rows, status 0 (BWA mode), an empty pattern's interval is the whole array."""
    import torch
    g, ix, _ = env
    i32, i64 = torch.int32, torch.int64
    three = np.zeros((3, 0), np.uint8)
    lohi = ix.sa_interval(three)
    _like(ix, lohi, (3, 2), i32)
    assert lohi.cpu().tolist() == [[0, ix.n]] * 3
    c, s, st = ix.find_smems_slots("bwa", three)
    _like(ix, c, (3,), i32), _like(ix, s, (3, 1, 4), i32), _like(ix, st, (3,), i32)
    assert c.cpu().tolist() == [0] * 3 and st.cpu().tolist() == [0] * 3
    for n, (off, sm, st) in ((3, ix.find_smems("bwa", three)), (6, ix.find_smems_both("bwa", three)),
                             (3, ix.find_smems_split(three))):
        _like(ix, off, (n + 1,), i64), _like(ix, sm, (0, 4), i32), _like(ix, st, (n,), i32)
        assert off.cpu().tolist() == [0] * (n + 1) and st.cpu().tolist() == [0] * n
    off, sm, st = ix.find_smems_long("bwa", np.zeros(0, np.uint8), np.zeros(4, np.int64))
    _like(ix, off, (4,), i64), _like(ix, sm, (0, 4), i32), _like(ix, st, (3,), i32)
    assert off.cpu().tolist() == [0] * 4 and st.cpu().tolist() == [0] * 3
    # packed reads of no bytes: the reads pointer of an empty tensor is null, which the C ABI refuses
    with pytest.raises(g._native.GenieError) as e:
        ix.find_smems_packed("bwa", three, 0)
    assert e.value.status == -1


def test_rows_hint_one_equals_no_hint(env):
    import torch
    from genie_smem_amd import synth
    _, ix, codes = env
    reads = synth.reads_from_ref(codes, 60, 150, 3)
    lens = np.random.default_rng(4).integers(0, 151, 60).astype(np.int32)
    split = reads.copy()
    split[::7, 40] = 4                                          # a break in every seventh read
    for call in (lambda **k: ix.find_smems("lut", reads, **k), lambda **k: ix.find_smems("bwa", reads, lens, 5, **k),
                 lambda **k: ix.find_smems_split(split, **k), lambda **k: ix.find_smems_split(split, lens, 3, **k)):
        want, got = call(), call(rows_hint=1)
        assert int(want[0][-1]) > 1
        for x, y in zip(want, got):
            assert x.dtype == y.dtype and x.shape == y.shape and x.device == y.device
            assert torch.equal(x, y)
