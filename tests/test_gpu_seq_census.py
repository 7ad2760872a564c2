"""The sequence census on the device (csrc/seq_census.hip) through its raw entry point, against the tests' own model
(tests/seq_census_model.py) on the designed streams of tests/seq_census_design.py.  Every size derives from the kernel's
tile: rows of every length around it at every alignment, runs of N on, at and across tile borders, hundreds of short rows
in one tile, windows of several sizes cut inside runs, stream positions past 2^33, rows that must stay untouched, every
byte value, tables that are out of order."""
import ctypes as C

import numpy as np
import pytest

from besst_amd import _lib, seqreport
from tests import seq_census_design as D
from tests import seq_census_model as M

pytestmark = pytest.mark.gpu

NAMES = ['all_byte_values', 'all_n_and_neighbours', 'lengths_and_alignments', 'many_short_rows', 'runs_at_tile_borders']
_DESIGNS, _WANT = {}, {}


def tile():
    """besst_dev_seq_census_tile_bytes(): every size below derives from it (asked at run time: the library is loaded
    behind torch, as everywhere in the package)"""
    import torch  # noqa: F401
    return int(_lib.load().besst_dev_seq_census_tile_bytes())


def design(name):
    if not _DESIGNS:
        _DESIGNS.update((d['name'], d) for d in D.all_designs(tile()))
        assert sorted(_DESIGNS) == NAMES
    return _DESIGNS[name]


def want_of(name, min_gap=1):
    """the model's partial table of a design, computed once"""
    if (name, min_gap) not in _WANT:
        d = design(name)
        _WANT[name, min_gap] = M.table(d['stream'], d['seq_off'], d['seq_len'], min_gap)
    return _WANT[name, min_gap]


def device_census(stream, seq_off, seq_len, cuts, min_gap=1, origin=0, lead=0, acc=None, window_cap=None):
    """besst_dev_seq_census over windows [cuts[k], cuts[k + 1]) of ``stream``, which begins at stream position ``origin``
    and lies ``lead`` bytes behind a 16-byte aligned address -> (acc rows, status words)"""
    import torch
    lib, dev = _lib.load(), torch.device('cuda', 0)
    n = len(stream)
    room = torch.zeros((lead + n + 15) // 16 * 16 + 16, dtype=torch.uint8, device=dev)        # whole groups are readable
    assert room.data_ptr() % 16 == 0
    if n:
        room[lead:lead + n] = torch.from_numpy(np.frombuffer(bytes(stream), dtype=np.uint8).copy()).to(dev)
    off = torch.tensor(list(seq_off), dtype=torch.int64, device=dev)
    length = torch.tensor(list(seq_len), dtype=torch.int64, device=dev)
    rows = len(seq_off)
    start = np.zeros((rows, 16), dtype=np.int64) if acc is None else np.asarray(acc, dtype=np.int64).reshape(rows, 16)
    d_acc = torch.from_numpy(start.copy()).to(dev) if rows else torch.zeros((1, 16), dtype=torch.int64, device=dev)
    status = torch.full((2,), -1, dtype=torch.int64, device=dev)
    cap = max([b - a for a, b in zip(cuts[:-1], cuts[1:])] + [1]) if window_cap is None else window_cap
    ws = torch.empty(lib.besst_dev_seq_census_workspace_bytes(cap, rows), dtype=torch.uint8, device=dev)
    stream_h = torch.cuda.current_stream(dev).cuda_stream
    p = C.c_void_p
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        _lib.check(lib.besst_dev_seq_census(p(stream_h), p(room.data_ptr() + lead + lo), origin + lo, hi - lo, rows,
                                            p(off.data_ptr()) if rows else None, p(length.data_ptr()) if rows else None, min_gap,
                                            p(ws.data_ptr()), p(d_acc.data_ptr()), p(status.data_ptr())), 'besst_dev_seq_census')
    torch.cuda.synchronize(dev)
    return d_acc.cpu().numpy()[:rows].tolist(), status.cpu().numpy().tolist()


def test_the_tile_size_is_what_the_header_says():
    T = tile()
    assert T == 8192 and T % 1024 == 0
    assert _lib.load().besst_dev_seq_census_workspace_bytes(3 * T, 7) >= 4 * 2 * 16 * 8


@pytest.mark.parametrize('name', NAMES)
def test_one_call_equals_the_model(name):
    d = design(name)
    for lead in (0, 5):
        got, status = device_census(d['stream'], d['seq_off'], d['seq_len'], [0, len(d['stream'])], lead=lead)
        assert status == [-1, -1]
        assert got == want_of(name), (name, lead)


@pytest.mark.parametrize('name', NAMES)
def test_windows_of_several_sizes_equal_one_call(name):
    d = design(name)
    n = len(d['stream'])
    T = tile()
    for window in (T // 2, T, 3 * T + 16):
        cuts = list(range(0, n, window)) + [n]
        got, status = device_census(d['stream'], d['seq_off'], d['seq_len'], cuts)
        assert status == [-1, -1]
        assert got == want_of(name), (name, window)


def test_window_cuts_inside_runs_and_min_gap():
    d, T = design('runs_at_tile_borders'), tile()
    n = len(d['stream'])
    # inside the run that ends a tile, one byte into the run that is a whole tile, in the middle of the three-tile run, twice
    cuts = [0, T - 3, 3 * T + 1, 5 * T + 7, 6 * T, 7 * T + 2, n]
    assert all(M.CLASS[d['stream'][c]] == M.N and M.CLASS[d['stream'][c - 1]] == M.N for c in cuts[1:-1])
    for min_gap in (1, 6, T, T + 1, 10 ** 6):
        got, _ = device_census(d['stream'], d['seq_off'], d['seq_len'], cuts, min_gap)
        assert got == want_of('runs_at_tile_borders', min_gap), min_gap
        assert got == device_census(d['stream'], d['seq_off'], d['seq_len'], [0, n], min_gap)[0]
    final = M.finalise(want_of('runs_at_tile_borders', T)[0], T)
    assert final[M.GAPS] == 2 and final[M.RUNS] == 5 and final[M.LONGEST] == 2 * T + 6


def test_runs_do_not_join_across_rows():
    d, T = design('all_n_and_neighbours'), tile()
    got, _ = device_census(d['stream'], d['seq_off'], d['seq_len'], [0, len(d['stream'])])
    assert got == want_of('all_n_and_neighbours')
    assert got[0][M.PRE] == got[0][M.SUF] == got[0][M.LEN] == 3 * T + 5 and got[0][M.RUNS] == 0
    assert got[1][M.PRE] == 4 and got[1][M.SUF] == 3 and got[2][M.PRE] == 1 and got[3][M.PRE] == 20


@pytest.mark.parametrize('name', ['all_n_and_neighbours', 'lengths_and_alignments', 'many_short_rows'])
def test_stream_positions_past_2_33(name):
    d = design(name)
    origin, T = (1 << 33) + 5, tile()
    off, length = D.shifted(d, origin)
    n = len(d['stream'])
    got, status = device_census(d['stream'], off, length, [0, n // 3, min(n, n // 3 + T + 1), n], origin=origin)
    assert status == [-1, -1]
    assert got == want_of(name)


def test_a_window_inside_rows_and_rows_outside_it_stay_bit_for_bit():
    rng, T = np.random.default_rng(7), tile()
    stream = bytes(rng.choice(np.frombuffer(b'ACGTNNNacgtn*R', dtype=np.uint8), 6 * T))
    off, length = [10, T // 2, 2 * T + 3, 5 * T, 6 * T - 4], [100, T, 2 * T, 100, 4]
    lo, hi = T, 3 * T + 9                                        # begins inside row 1, ends inside row 2
    sentinel = (np.arange(5 * 16, dtype=np.int64).reshape(5, 16) * 1000003 + 17) * np.array([[-1], [1], [1], [-1], [1]])
    before = np.zeros((5, 16), dtype=np.int64)
    for i in (0, 3, 4):
        before[i] = sentinel[i]
    got, status = device_census(stream[lo:hi], off, length, [0, hi - lo], origin=lo, acc=before)
    assert status == [-1, -1]
    for i in (0, 3, 4):                                          # entirely outside the window
        assert got[i] == before[i].tolist()
    assert got[1] == M.partial(stream[lo:T // 2 + T]) and got[2] == M.partial(stream[2 * T + 3:hi])
    # the rest of the stream as further windows: merged as the right-hand neighbour
    first, _ = device_census(stream[:lo], off, length, [0, lo])
    acc = np.asarray(first, dtype=np.int64)
    second, _ = device_census(stream[lo:hi], off, length, [0, hi - lo], origin=lo, acc=acc)
    third, _ = device_census(stream[hi:], off, length, [0, len(stream) - hi], origin=hi, acc=np.asarray(second, dtype=np.int64))
    assert third == M.table(stream, off, length)


def test_every_byte_value_in_rows_of_its_own():
    stream = b''.join(bytes([b]) * 5 + b'N' for b in range(256))
    off, length = [6 * b for b in range(256)], [5] * 256
    got, _ = device_census(stream, off, length, [0, len(stream)], lead=3)
    assert got == M.table(stream, off, length)
    for b in range(256):
        assert got[b][M.CLASS[b]] == 5 and got[b][M.LOWER] == (5 if 0x61 <= b <= 0x7A else 0)


def test_tables_out_of_order_are_a_status_and_raise_in_python():
    import torch
    stream = b'ACGTNNNNACGTNNNN' * 8
    for off, length, bad in (([0, 40, 20, 60], [10, 10, 10, 10], 2), ([0, 5, 30], [10, 10, 10], 1),
                             ([0, 20, 40, 39], [10, 10, 10, 1], 3)):
        _, status = device_census(stream, off, length, [0, len(stream)])
        assert status[0] == bad, (off, status)
        with pytest.raises(ValueError, match='row %d' % bad):
            seqreport.check_table(off, length)
        dev = torch.device('cuda', 0)
        run = seqreport.CensusRun(torch, dev, np.asarray(off), np.asarray(length), len(stream))
        buf = torch.from_numpy(np.frombuffer(stream, dtype=np.uint8).copy()).to(dev)
        run.add(buf.data_ptr(), 0, len(stream))
        with pytest.raises(_lib.BesstDeviceError, match='row %d' % bad):
            run.words()
    _, status = device_census(stream, [0, 10, 10, 30], [10, 0, 20, 0], [0, len(stream)])
    assert status == [-1, -1]                                    # rows of length 0 between neighbours that touch


def test_nothing_to_do_is_a_clean_no_op():
    before = np.arange(32, dtype=np.int64).reshape(2, 16)
    got, status = device_census(b'', [0, 5], [5, 5], [0, 0], acc=before)
    assert got == before.tolist() and status == [-1, -1]
    got, status = device_census(b'ACGTN' * 10, [], [], [0, 50])
    assert got == [] and status == [-1, -1]
    lib = _lib.load()
    assert lib.besst_dev_seq_census(None, None, 0, 0, 0, None, None, 1, None, None, None) == 0
    assert lib.besst_dev_seq_census(None, None, 0, 16, 2, None, None, 1, None, None, None) != 0
    assert 'null' in _lib.last_error()
