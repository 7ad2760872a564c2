"""CPU checks of the scaffold output stage: the fixture captured from the reference, the plain-Python and numpy models of
tests/output_util.py against it, and the host side of besst_amd.GenerateOutput (layout, piece table, WriteToF, the
library's complement table, the CLI's refusals).  The kernels themselves: tests/test_gpu_scaffold_output.py."""
import ctypes as C

import numpy as np
import pytest

from besst_amd import GenerateOutput as GO
from besst_amd import _lib
from tests import output_util as OU

DOC = OU.load_golden()
CASES = {c['name']: c for c in DOC['cases']}
UID = DOC['unique_id']


def test_fixture_loads_and_covers_what_it_should():
    assert len(CASES) == len(DOC['cases']) >= 15
    assert {c['K'] for c in DOC['cases']} >= {0, 1, 64, 200}
    assert any(isinstance(c['sigma'], float) and c['sigma'] != int(c['sigma']) for c in DOC['cases'])
    assert any(c['sigma'] == 0 for c in DOC['cases'])
    merges = [int(l.split()[1]) for c in DOC['cases'] for l in c['expect']['merging']]
    assert {20, 21, 63, 64, 199, 200} <= set(merges) and min(merges) == 20 and max(merges) == 200
    errors = {c['expect']['key_error'] for c in DOC['cases']}
    assert {'u', 'x', 'U', None} <= errors
    assert CASES['forward_U']['expect']['key_error'] is None and CASES['forward_x']['expect']['key_error'] is None
    lengths = {len(t[4]) for c in DOC['cases'] for s in c['F'] for t in s}
    assert {1, 2} <= lengths
    assert any(len(s) == 1 for c in DOC['cases'] for s in c['F'])


def test_complement_tables_agree():
    """the fixture's rev_nuc, the model's table and the table compiled into the library are one table"""
    assert DOC['rev_nuc'] == OU.complement_table()
    lib = _lib.load()
    table = C.string_at(lib.besst_host_complement_table(), 256)
    assert list(table) == DOC['rev_nuc']


@pytest.mark.parametrize('name', sorted(CASES))
def test_model_reproduces_the_reference(name):
    case = CASES[name]
    got = OU.model_output(OU.case_F(case), case['K'], case['sigma'], UID)
    want = case['expect']
    for key in ('key_error', 'merging', 'fasta', 'agp', 'gff'):
        assert got[key] == want[key], key


def _layout(case):
    F = OU.case_F(case)
    flat = [t for scaf in OU.ordered(F) for t in scaf]
    pool, off, length = GO.pack_sequences([t[4] for t in flat])
    lay = GO.ScaffoldLayout(F, OU.Param(case['K'], case['sigma']), UID, off, length)
    return F, flat, pool, off, length, lay


def _model_overlaps(F, K):
    """raw overlap of every junction in output order, None where a reversal fails"""
    out = []
    for scaf in OU.ordered(F):
        for a, b in zip(scaf[:-1], scaf[1:]):
            try:
                out.append(OU.window_overlap(a, b, K))
            except KeyError:
                out.append(None)
    return out


@pytest.mark.parametrize('name', sorted(n for n, c in CASES.items() if c['expect']['key_error'] is None))
def test_piece_table_matches_the_model(name):
    case = CASES[name]
    F, flat, pool, off, length, lay = _layout(case)
    every = _model_overlaps(F, case['K'])
    junction = np.flatnonzero(~lay.first) - np.cumsum(lay.first)[~lay.first]      # junction ordinal of each non-first contig
    cand_junction = {int(c): int(j) for c, j in zip(np.flatnonzero(~lay.first), junction)}
    overlaps = [every[cand_junction[int(c)]] for c in lay.cand]
    tab = lay.pieces(overlaps)
    want = case['expect']['fasta'].encode()
    assert tab['total'] == len(want) == int(tab['out_off'][-1])
    assert tab['out_off'][0] == 0 and (np.diff(tab['out_off']) == tab['len']).all()
    assert len(tab['mode']) == 2 * len(flat) + len(F) <= 4 * len(flat)
    assert OU.apply_pieces(tab, pool) == want
    assert ['merging %d bp here' % n for _, n in tab['merges']] == case['expect']['merging']
    # candidates: exactly the junctions with gap <= 2 sigma
    gaps = [b[2] - (a[2] + a[3]) for scaf in OU.ordered(F) for a, b in zip(scaf[:-1], scaf[1:])]
    assert [cand_junction[int(c)] for c in lay.cand] == [j for j, g in enumerate(gaps) if g <= 2 * case['sigma']]


@pytest.mark.parametrize('name', ['mixed', 'overlaps_K200', 'short_K5', 'gaps_sigma12.7'])
def test_numpy_model_matches_the_string_model(name):
    case = CASES[name]
    F, flat, pool, off, length, lay = _layout(case)
    scaffolds, overlaps, row = [], {}, 0
    for k, scaf in enumerate(OU.ordered(F)):
        rows = []
        for i, t in enumerate(scaf):
            rows.append((row, t[1], t[2], t[3]))
            if i:
                overlaps[(k, i - 1)] = OU.window_overlap(scaf[i - 1], t, case['K'])
            row += 1
        scaffolds.append(rows)
    got = OU.numpy_fasta(scaffolds, pool, off, length, overlaps, case['sigma'], UID)
    assert got.tobytes() == case['expect']['fasta'].encode()


class _Contig(object):
    def __init__(self, name, direction, position, length, sequence):
        self.name, self.direction, self.position, self.length, self.sequence = name, direction, position, length, sequence


def test_write_to_f_tuples(capsys):
    objs = [_Contig('a', True, 0, 4, 'ACGT'), _Contig('b', False, -3, 2, 'GG')]
    F = GO.WriteToF([], {}, objs)
    F = GO.WriteToF(F, {}, objs[:1])
    assert F == [[('a', True, 0, 4, 'ACGT'), ('b', False, -3, 2, 'GG')], [('a', True, 0, 4, 'ACGT')]]
    assert capsys.readouterr().out == 'Write to F: Position is negative! -3 b False\n'


def test_pack_sequences_and_limits():
    pool, off, length = GO.pack_sequences(['ACgt', '', b'NNn', None, 'x'])
    assert pool.tobytes() == b'ACgtNNnx' and off.tolist() == [0, 4, 4, 7, 7] and length.tolist() == [4, 0, 3, 0, 1]
    assert off.dtype == np.int64 and length.dtype == np.int32 and pool.dtype == np.uint8
    with pytest.raises(ValueError):
        GO.pack_sequences(['ACé'])
    with pytest.raises(ValueError):
        GO.pack_sequences([b'AC\xe9'])
    F = [[('a', True, 0, 4, 'ACGT')]]
    for K in (-1, GO.MAX_CONTIG_OVERLAP_LIMIT + 1):
        with pytest.raises(ValueError):
            GO.ScaffoldLayout(F, OU.Param(K, 1.0), UID, [0], [4])
    GO.ScaffoldLayout(F, OU.Param(GO.MAX_CONTIG_OVERLAP_LIMIT, 1.0), UID, [0], [4])


def test_argument_errors_of_the_new_entry_points_need_no_gpu():
    lib = _lib.load()
    err = (C.c_uint64 * 2)()
    assert lib.besst_host_seq_overlaps(0, None, 0, 0, None, None, 1, None, None, None, 4097, None, err) == 1
    assert 'max_overlap' in _lib.last_error()
    assert lib.besst_host_seq_overlaps(0, None, 0, 0, None, None, 1, None, None, None, -1, None, err) == 1
    assert lib.besst_host_seq_overlaps(0, None, 0, 0, None, None, 0, None, None, None, 200, None, err) == 0
    assert lib.besst_host_emit_scaffolds(0, None, 0, None, 0, 0, None, None, None, None, 5, 3, None, err) == 1
    assert 'range' in _lib.last_error()
    assert lib.besst_host_emit_scaffolds(0, None, 0, None, 0, 0, None, None, None, None, 0, 0, None, err) == 0
    # a table whose out_off is not the prefix sum of len, and a piece outside its pool
    src, ln, mode = np.zeros(1, np.int64), np.array([4], np.int64), np.zeros(1, np.uint8)
    pool, out = np.frombuffer(b'ACGT', np.uint8), np.zeros(16, np.uint8)
    p = _lib.ptr
    assert lib.besst_host_emit_scaffolds(0, p(pool), 4, None, 0, 1, p(src), p(ln), p(mode), p(np.array([0, 5], np.int64)),
                                         0, 4, p(out), err) == 1
    assert 'prefix sum' in _lib.last_error()
    assert lib.besst_host_emit_scaffolds(0, p(pool), 3, None, 0, 1, p(src), p(ln), p(mode), p(np.array([0, 4], np.int64)),
                                         0, 4, p(out), err) == 1
    assert 'outside' in _lib.last_error()


def test_cli_scaffolds_needs_y_and_scoring(tmp_path):
    from besst_amd import cli
    base = ['-c', str(tmp_path / 'none.fa'), '-f', str(tmp_path / 'none.bam'), '-orientation', 'fr', '-o', str(tmp_path)]
    for extra, word in ((['--scaffolds'], 'path search'), (['--scaffolds', '-y', '--no_score'], '--no_score'),
                        (['--scaffolds', '-y', '-max_contig_overlap', '5000'], 'max_contig_overlap')):
        with pytest.raises(SystemExit) as exc:
            cli.main(base + extra)
        assert exc.value.code not in (0, None) and word in str(exc.value.code)
    assert not (tmp_path / 'BESST_output').exists()
    args = cli.build_parser().parse_args(base)
    assert args.max_contig_overlap == 200 and args.scaffolds is False
