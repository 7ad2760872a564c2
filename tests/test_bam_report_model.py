"""No GPU: the BAM report's model (tests/bam_report_model.py) against numbers counted by hand and against the sixteen census
rules written out a second time; besst_amd.report's files, sums and orientation note; the C ABI's argument errors."""
import ctypes as C
import os

import numpy as np
import pytest

from besst_amd import _lib, bamio, report
from tests import bam_report_model as M

HERE = os.path.dirname(os.path.abspath(__file__))


def as_report(cols, n_refs, bins=64, **kw):
    return report.LibraryReport(M.words(cols, n_refs, bins), n_refs, bins, **kw)


@pytest.mark.parametrize('name', ['handmade_a.bam', 'handmade_b.bam'])
def test_model_on_the_hand_assembled_files(name):
    """The fifteen records of tests/golden/bam/handmade_bam.json, counted by hand from their flags: all QC-pass; records 9
    and 15 unmapped (15 unplaced, 9 placed on ctgB); read 2 of a pair on one reference: records 2 and 7 (reverse, mate
    forward, tlen -400 / -1800: innie) and 13 (opposite strands, tlen 0: other)."""
    batch = bamio.read_bam(os.path.join(HERE, 'golden', 'bam', name), threads=1)
    m = M.model(batch, 3, isize_bins=1000)
    want = dict(zip(M.ROWS, (15, 15, 0, 0, 0, 0, 13, 13, 15, 9, 6, 9, 13, 0, 6, 6)))
    assert {lab: int(m['census'][r, 0]) for r, lab in enumerate(M.ROWS)} == want
    assert not m['census'][:, 1].any()
    assert (m['unplaced'], m['tid_out_of_range']) == (1, 0)
    assert m['mapped'].tolist() == [4, 6, 3] and m['placed_unmapped'].tolist() == [0, 1, 0]
    assert {int(v): int(m['mapq'][v]) for v in np.flatnonzero(m['mapq'])} == {0: 1, 10: 1, 11: 1, 37: 1, 60: 9}
    assert {int(v): int(m['qlen'][v]) for v in np.flatnonzero(m['qlen'])} == {0: 1, 30: 1, 80: 2, 90: 1, 100: 8}
    assert m['pairs'].tolist() == [2, 0, 0, 1]
    assert np.flatnonzero(m['innie']).tolist() == [400, 1000] and m['innie'][[400, 1000]].tolist() == [1, 1]   # 1800: overflow
    assert not m['outie'].any() and not m['tandem'].any()
    assert m['digest'] == M.digest_py(M.columns_of(batch)) == M.digest_np(M.columns_of(batch))
    # the first record's h, from the formula by hand: tid 0, mtid 0, pos 100, mpos 400, tlen 400, flag 99, qlen 100, mapq 60
    a, b, c = 0, 100 | 400 << 32, 400 | 99 << 32 | 100 << 48
    sm = M.splitmix64
    assert M.record_hash(0, 0, 100, 400, 400, 99, 60, 100) == sm(sm(sm(sm(a) ^ b) ^ c) ^ 60)
    assert sm(0) == 0xe220a8397b1dcdaf                        # splitmix64's first output for seed 0, as published


def census_by_loop(cols):
    """The sixteen rules of the issue as a straight loop over the records."""
    t = [[0, 0] for _ in range(16)]
    for tid, mtid, flag, mapq in zip(cols['tid'].tolist(), cols['mtid'].tolist(), cols['flag'].tolist(), cols['mapq'].tolist()):
        q = 1 if flag & 0x200 else 0
        t[0][q] += 1
        if not flag & 0x4:
            t[6][q] += 1
        if flag & 0x400:
            t[4][q] += 1
        if flag & 0x100:
            t[2][q] += 1
            continue
        if flag & 0x800:
            t[3][q] += 1
            continue
        t[1][q] += 1
        if not flag & 0x4:
            t[7][q] += 1
        if flag & 0x400:
            t[5][q] += 1
        if not flag & 0x1:
            continue
        t[8][q] += 1
        if flag & 0x40:
            t[9][q] += 1
        if flag & 0x80:
            t[10][q] += 1
        if flag & 0x2 and not flag & 0x4:
            t[11][q] += 1
        if flag & 0x8 and not flag & 0x4:
            t[13][q] += 1
        if not flag & 0x4 and not flag & 0x8:
            t[12][q] += 1
            if tid != mtid:
                t[14][q] += 1
                if mapq >= 5:
                    t[15][q] += 1
    return t


@pytest.mark.parametrize('n_refs,shuffled', [(3, None), (3, 5), (1, None)])
def test_flag_truth_table(n_refs, shuffled):
    cols = M.flag_table(n_refs, shuffled)
    assert len(set(zip(cols['flag'].tolist(), (cols['tid'] == cols['mtid']).tolist(), (cols['tid'] < 0).tolist(),
                       (cols['mtid'] < 0).tolist()))) == 4 * 4096
    m = M.model(cols, n_refs, 64)
    assert m['census'].tolist() == census_by_loop(cols)
    assert m['census'][:, 1].sum() > 0 and m['pairs'].min() > 0 and m['census'].min() > 0
    # every record is in exactly one of: a reference's two counts, unplaced, out of range
    assert m['mapped'].sum() + m['placed_unmapped'].sum() + m['unplaced'] + m['tid_out_of_range'] == 4 * 4096
    assert m['digest'] == M.digest_py(cols)
    assert M.model(M.flag_table(n_refs, 9), n_refs, 64)['digest'] == m['digest']         # (order independent)


def test_write_read_round_trip(tmp_path):
    cols = M.flag_table(3)
    rep = as_report(cols, 3, 300, references=['a', 'b b', 'c'], lengths=[10, 20, 30])
    rep.write(str(tmp_path))
    assert sorted(os.listdir(str(tmp_path))) == sorted(report.FILES)
    back = report.LibraryReport.read(str(tmp_path))
    assert back == rep and back.references == ['a', 'b b', 'c'] and back.lengths == [10, 20, 30]
    top = [l.rstrip('\n').split('\t') for l in open(str(tmp_path / 'bam_report.tsv'))]
    assert top[0] == ['label', 'pass', 'fail'] and [r[0] for r in top[1:17]] == list(M.ROWS)
    assert top[-2][0] == 'digest_sum' and int(top[-2][1], 16) == M.digest_py(cols)[0]
    idx = [l.rstrip('\n').split('\t') for l in open(str(tmp_path / 'idxstats.tsv'))]
    assert idx[-1] == ['*', '0', '0', str(rep.unplaced)] and idx[2][:2] == ['b b', '20']
    ins = [l.rstrip('\n').split('\t') for l in open(str(tmp_path / 'insert_sizes.tsv'))]
    assert ins[-1][0] == '>=300' and all(any(int(x) for x in r[1:]) for r in ins[1:-1])
    for fname in ('mapq_hist.tsv', 'qlen_hist.tsv'):
        assert all(int(l.split('\t')[1]) > 0 for l in list(open(str(tmp_path / fname)))[1:])
    # an empty report too
    empty = report.LibraryReport(np.zeros(report.report_words(0, 1), np.uint64), 0, 1)
    empty.write(str(tmp_path / 'e'))
    assert report.LibraryReport.read(str(tmp_path / 'e')) == empty


def test_add_over_every_cut_of_a_stream():
    cols = {k: v[5000:5300] for k, v in M.flag_table(3, shuffled=3).items()}
    whole = as_report(cols, 3)
    assert whole.n_records == 300 and whole.digest == M.digest_py(cols)
    for cut in range(301):
        a = as_report({k: v[:cut] for k, v in cols.items()}, 3)
        b = as_report({k: v[cut:] for k, v in cols.items()}, 3)
        assert a + b == whole, cut
    with pytest.raises(ValueError):
        whole + as_report(cols, 4)


def pairs_report(innie, outie):
    w = np.zeros(report.report_words(1, 1), np.uint64)
    w[report.PAIRS], w[report.PAIRS + 1] = innie, outie
    return report.LibraryReport(w, 1, 1)


def test_orientation_note_borders():
    for named, mine in (('fr', 0), ('rf', 1)):
        def rep(share, total):
            counts = [total - share, total - share]
            counts[mine] = share
            return pairs_report(*counts)
        assert report.orientation_note(rep(99, 1000), named) is not None           # 9.9 % of 1000
        assert report.orientation_note(rep(100, 1000), named) is None              # 10 %
        assert report.orientation_note(rep(0, 999), named) is None                 # under 1000 pairs
        assert report.orientation_note(rep(0, 1000), named) is not None
        assert report.orientation_note(rep(9999, 100000), named) is not None and report.orientation_note(rep(10000, 100000), named) is None
        note = report.orientation_note(rep(99, 1000), named)
        assert '-orientation %s' % named in note and ('rf' if named == 'fr' else 'fr') in note
        other = 'rf' if named == 'fr' else 'fr'
        assert report.orientation_note(rep(99, 1000), other) is None               # the other class holds 90.1 %
    with pytest.raises(ValueError):
        report.orientation_note(pairs_report(1, 1), 'ff')


def test_length_mismatches():
    assert report.length_mismatches(['a', 'b', 'c'], [10, 20, 30], {'a': 10, 'b': 21, 'd': 5}) == [('b', 20, 21)]


def test_report_words_and_argument_errors_need_no_gpu():
    lib = _lib.load()
    assert lib.besst_dev_library_report_words(3, 32768) == report.report_words(3, 32768) == M.n_words(3, 32768)
    assert lib.besst_dev_library_report_words(0, 1) == M.n_words(0, 1)
    for bad in ((3, 0), (3, (1 << 20) + 1), (-1, 10), (1 << 31, 10)):
        assert lib.besst_dev_library_report_words(*bad) == 0
        with pytest.raises(ValueError):
            report.report_words(*bad)
    words = M.n_words(3, 16)
    out = np.zeros(words, np.uint64)
    col = np.zeros(4, np.int32)
    p = col.ctypes.data

    def args(**kw):
        a = dict(tid=p, mtid=p, pos=p, mpos=p, tlen=p, flag=p, mapq=p, qlen=p, tid_bits=None, n_records=4, n_refs=3,
                 isize_bins=16, out_words=words)
        a.update(kw)
        return _lib.ReportArgs(**a)
    call = lambda a, o=out: lib.besst_dev_library_report(None, C.byref(a) if a is not None else None,
                                                         _lib.ptr(o) if o is not None else None)
    assert call(None) == 1 and 'null' in _lib.last_error()
    assert call(args(), None) == 1 and 'null' in _lib.last_error()
    for col_name in M.COLUMNS:
        assert call(args(**{col_name: None})) == 1 and 'null column' in _lib.last_error()
    assert call(args(isize_bins=0)) == 1 and 'isize_bins' in _lib.last_error()
    assert call(args(isize_bins=(1 << 20) + 1)) == 1 and 'isize_bins' in _lib.last_error()
    assert call(args(out_words=words - 1)) == 1 and 'too short' in _lib.last_error()
    assert call(args(n_records=-1)) == 1 and call(args(n_refs=-1)) == 1 and call(args(n_records=1 << 32)) == 1
    assert lib.besst_ctx_library_report(None, 16, _lib.ptr(out), words) == 1 and 'null' in _lib.last_error()
