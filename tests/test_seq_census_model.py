"""No GPU: the census rule, the designs, the host entry point and the summary statistics.

The merge law is held against ``itertools.groupby`` on random strings; every designed stream is shown to contain the
borders it names; ``besst_host_seq_census`` (the kernels' core header on the host) is called through ctypes and held
against the tests' model; ``AssemblyStats`` against the model's Nx and against ``CreateGraph.CalculateStats``."""
import ctypes as C
import io
import random

import numpy as np
import pytest

from besst_amd import CreateGraph, _lib, seqreport
from tests import seq_census_design as D
from tests import seq_census_model as M

T = 1024                                  # the host entry knows no tile; the designs only scale with it


def host_census(stream, seq_off, seq_len, cuts, min_gap=1, origin=0, acc=None):
    """besst_host_seq_census over windows [cuts[k], cuts[k + 1]) of ``stream`` (which begins at stream position ``origin``)"""
    lib = _lib.load()
    off, length = np.asarray(seq_off, dtype=np.int64), np.asarray(seq_len, dtype=np.int64)
    acc = np.zeros((len(off), 16), dtype=np.int64) if acc is None else np.array(acc, dtype=np.int64)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        window = np.frombuffer(bytes(stream[lo:hi]) or b'\0', dtype=np.uint8)
        status = lib.besst_host_seq_census(p(window), origin + lo, hi - lo, len(off), p(off), p(length), min_gap, p(acc))
        assert status == 0, _lib.last_error()
    return acc.tolist()


@pytest.mark.parametrize('min_gap', [1, 2, 3, 10 ** 6])
def test_merge_law_on_random_strings(min_gap):
    rng = random.Random(min_gap)
    for _ in range(1500):
        n = rng.randrange(0, 24)
        data = bytes(rng.choice(b'NNAg') for _ in range(n))
        cuts = sorted(rng.randrange(0, n + 1) for _ in range(rng.randrange(0, 5)))
        parts = [M.partial(data[a:b], min_gap) for a, b in zip([0] + cuts, cuts + [n])]
        while len(parts) > 1:                                    # any association order
            k = rng.randrange(len(parts) - 1)
            parts[k:k + 2] = [M.merge(parts[k], parts[k + 1], min_gap)]
        assert parts[0] == M.partial(data, min_gap), (data, cuts)
        assert M.finalise(parts[0], min_gap) == M.whole(data, min_gap), (data, cuts)


@pytest.mark.parametrize('design', D.all_designs(T), ids=lambda d: d['name'])
def test_every_design_contains_the_borders_it_names(design):
    assert design['borders']
    for border in design['borders']:
        assert D.has_border(design, border, T), (design['name'], border)
    off, length = design['seq_off'], design['seq_len']
    assert all(o2 >= o1 + n1 for o1, n1, o2 in zip(off[:-1], length[:-1], off[1:]))
    assert off[-1] + length[-1] <= len(design['stream'])


@pytest.mark.parametrize('design', D.all_designs(T), ids=lambda d: d['name'])
def test_host_entry_equals_the_model_on_every_design(design):
    stream, off, length = design['stream'], design['seq_off'], design['seq_len']
    n = len(stream)
    want = M.table(stream, off, length)
    assert host_census(stream, off, length, [0, n]) == want
    for window in (T // 2, T, 3 * T + 16):
        cuts = list(range(0, n, window)) + [n]
        assert host_census(stream, off, length, cuts) == want == M.windowed(stream, off, length, cuts)
    # 64-bit stream positions, and min_gap
    origin = (1 << 33) + 5
    shifted_off, _ = D.shifted(design, origin)
    assert host_census(stream, shifted_off, length, [0, n // 3, n], 3, origin) == M.table(stream, off, length, 3)


def test_host_entry_on_all_256_byte_values():
    for b in range(256):
        data = bytes([b]) * 3 + b'A'
        got = host_census(data, [0], [4], [0, 2, 4])[0]
        assert got == M.partial(data), b
        assert got[M.CLASS[b]] >= 3 and got[M.LOWER] == (3 if 0x61 <= b <= 0x7A else 0)


def test_windows_at_every_cut_across_a_run():
    data = b'ACGTACGTAC' + b'N' * 7 + b'acgtn' + b'N' * 6 + b'GATTACAGATTA'        # 40 bytes
    assert len(data) == 40
    off, length = [0, 12, 30], [12, 18, 10]                      # the first run straddles rows 0 and 1
    want = M.table(data, off, length)
    for cut in range(0, 41):
        for second in (cut, min(40, cut + 3), 40):
            cuts = [0, cut, second, 40]
            assert host_census(data, off, length, cuts) == want, cuts
            assert M.windowed(data, off, length, cuts) == want, cuts


def test_rows_without_bytes_in_the_window_are_not_touched():
    acc = np.arange(3 * 16, dtype=np.int64).reshape(3, 16) + 1000
    got = host_census(b'ACGTNNNNAC', [100, 104, 200], [4, 6, 5], [4, 10], origin=100, acc=acc)
    assert got[0] == acc[0].tolist() and got[2] == acc[2].tolist()
    assert got[1] == M.merge(acc[1].tolist(), M.partial(b'NNNNAC'))
    lib = _lib.load()
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    bad_off, bad_len = np.array([0, 10, 5], dtype=np.int64), np.array([3, 3, 3], dtype=np.int64)
    buf, out = np.zeros(16, dtype=np.uint8), np.zeros((3, 16), dtype=np.int64)
    assert lib.besst_host_seq_census(p(buf), 0, 16, 3, p(bad_off), p(bad_len), 1, p(out)) != 0
    assert 'row 2' in _lib.last_error()
    with pytest.raises(ValueError, match='row 2'):
        seqreport.check_table(bad_off, bad_len)


def census_of(lengths):
    words = np.zeros((len(lengths), 16), dtype=np.int64)
    words[:, M.LEN] = lengths
    return seqreport.SequenceCensus(['s%d' % k for k in range(len(lengths))], words)


def test_nx_lx_ties_and_borders():
    for lengths in ([50, 30, 20], [5, 5, 5, 5], [9, 1], [7], [10, 10, 10, 10, 10, 10, 10, 10, 10, 10], [3, 3, 2, 1, 1]):
        stats = seqreport.AssemblyStats(census_of(lengths))
        for x in (0, 1, 50, 60, 90, 100):
            assert stats.nx(x) == M.nx(lengths, x), (lengths, x)
            assert stats.lx(x) == M.lx(lengths, x), (lengths, x)
    ties = seqreport.AssemblyStats(census_of([50, 30, 20]))     # the running sum equals the threshold exactly
    assert (ties.nx(50), ties.lx(50)) == (50, 1)
    assert (seqreport.AssemblyStats(census_of([40, 50, 10])).nx(90), seqreport.AssemblyStats(census_of([40, 50, 10])).lx(90)) == (40, 2)
    one = seqreport.AssemblyStats(census_of([7]))
    assert (one.N50, one.L50, one.N90, one.L90, one.min, one.max, one.total) == (7, 1, 7, 1, 7, 7, 7)
    equal = seqreport.AssemblyStats(census_of([5] * 4))
    assert (equal.nx(50), equal.lx(50), equal.nx(90), equal.lx(90)) == (5, 2, 5, 4)


def test_nx_lx_without_sequences():
    empty = seqreport.AssemblyStats(census_of([]))
    assert empty.nx(50) is None and empty.lx(50) == 0
    assert (empty.n, empty.total, empty.N50, empty.L50, empty.gc) == (0, 0, None, 0, None)
    assert M.nx([], 50) is None and M.lx([], 50) == 0
    assert seqreport.reference_n60([]) is None


def test_nx50_equals_calculate_stats():
    rng = random.Random(50)

    class Param(object):
        pass

    for _ in range(200):
        lengths = [rng.randrange(1, 40) for _ in range(rng.randrange(1, 30))]
        param = Param()
        param.tot_assembly_length = sum(lengths)
        n50, l50 = CreateGraph.CalculateStats(sorted(lengths, reverse=True), [], param, io.StringIO())
        stats = seqreport.AssemblyStats(census_of(lengths))
        assert (stats.nx(50), stats.lx(50)) == (n50, l50), lengths


def test_reference_n60_keeps_the_float_expression():
    for lengths in ([50, 30, 20], [60, 40], [6, 4], [3, 3, 3, 1], [7]):
        desc = sorted(lengths, reverse=True)
        stop, running, want = sum(desc) / (100 / 60.0), 0, None
        for v in desc:
            running += v
            if running >= stop:
                want = v
                break
        assert seqreport.reference_n60(lengths) == want
    assert seqreport.reference_n60([60, 40]) == 60


def test_tsv_round_trip(tmp_path):
    data = [b'ACGTNNNNacgtRYx*NN', b'NNNN', b'', b'--', b'GGCC' + b'N' * 12 + b'AT']
    words = np.asarray([M.partial(d, 3) for d in data], dtype=np.int64)
    census = seqreport.SequenceCensus(['one', 'two', 'two', 'odd name|x', 'five'], words, min_gap=3)
    assert not census.final and census.finalised().words.tolist() == [M.whole(d, 3) for d in data]
    path = str(tmp_path / 'report.tsv')
    census.write(path)
    back = seqreport.SequenceCensus.read(path)
    assert back.final and back.min_gap == 3 and back.names == census.names
    assert back.words.tolist() == census.finalised().words.tolist()
    back.write(str(tmp_path / 'again.tsv'))
    assert open(path).read() == open(str(tmp_path / 'again.tsv')).read()
    lines = open(path).read().splitlines()
    assert lines[1].split('\t') == list(seqreport.COLUMNS)
    gc = [line.split('\t')[10] for line in lines[2:]]
    assert gc[0] == '%.6f' % (4 / 8.0) and gc[1] == '' and gc[2] == '' and gc[3] == ''
    assert census.gaps.tolist() == words[:, M.GAPS].tolist() and back.longest_gap.tolist() == [4, 4, 0, 0, 12]
