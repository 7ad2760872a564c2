"""GPU: the side-stream form of the fused record loop as a software pipeline, launched in two parts.

The full blocks of a stream run the lean form of fused_wave_kernel - a loop unrolled by two whose buffers alternate, with
the round's contig rows issued behind the round before - and the stream's partial last block runs the general form with a
block offset.  What can go wrong is at the borders of that structure: the split between the two launches (no full block,
no tail, a chain that reaches across), the number of rounds of a block against the unroll factor and against the 64
sub-tiles, the `tid` double buffer where the contig changes, and the `mtid` path of a table with absent contigs.

Every case runs the third form writing keys and grouping runs and compares edge table, coverage and counters with
oracle/py_oracle.record_loop, with the C oracle, and with the same call without the side stream (BESST_CAND_STREAM=0: in
the process, and once for all streams in a child process started with it).  The generators assert on the CPU that a
stream has the property it is named for (tests/test_side_loop_pipeline_design.py runs them without a GPU)."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import record_design as D
from tests import test_candidate_stream as M
from tests import test_gpu_candidate_stream as S
from tests import test_gpu_record_borders as T
from tests.record_design import BLOCK, SUB, N_CONTIGS

pytestmark = pytest.mark.gpu

UNROLL = 2                                                   # the loop's unroll factor (classify.hip: `it += 2`)
SUBS = BLOCK // SUB
A, B = D.LARGE[0], D.LARGE[1]
ABSENT = D.rows_of('absent')
RD1, RD2, UN = S.RD1, S.RD2, S.UN


def present_table():
    """D.TABLE with a small contig on a scaffold of its own in the place of every absent row: every contig of the header is
    in the table (the loop's all_present path; the scaffold ids r + 1 of those rows are free in D.TABLE)."""
    t = {k: list(v) for k, v in D.TABLE.items()}
    for r in ABSENT:
        assert r + 1 not in D.TABLE['scaf']
        t['cls'][r], t['scaf'][r], t['slen'][r], t['cpos'][r], t['clen'][r], t['cdir'][r] = D.CLS_SMALL, r + 1, 300, 0, 300, True
    assert D.CLS_ABSENT not in t['cls'] and max(t['scaf']) == max(D.TABLE['scaf'])
    return t


TABLES = {'absent': D.TABLE, 'present': present_table()}
assert D.CLS_ABSENT in TABLES['absent']['cls']


def entry_counts(rec):
    """Entries of the side stream per block, and the rounds of 64 they make."""
    off = M.compact(rec, N_CONTIGS)['offsets'].astype(np.int64)
    counts = np.diff(off)
    return counts.tolist(), (-(-counts // 64)).tolist()


def _scatter(b, blk, count):
    step = max(1, BLOCK // max(count, 1))
    at = [blk * BLOCK + (j * step + (7 if count < BLOCK else 0)) % BLOCK for j in range(count)]
    assert len(set(at)) == count
    for i in at:
        S._link(b, i)


# ---- the split launch --------------------------------------------------------------------------------------------------
SPLIT_LENGTHS = [BLOCK - 1, BLOCK, BLOCK + 1, 2 * BLOCK - 1, 3 * BLOCK + SUB]


def stream_split(n):
    """n records: n // BLOCK full blocks for the lean launch (none at BLOCK - 1), n % BLOCK records for the general one (none
    at BLOCK); links and fishy records all along, so both launches emit and the chain runs through every border."""
    s = S.stream_lengths(n)
    rec = s.records
    assert len(rec['tid']) == n
    counts, _ = entry_counts(rec)
    assert len(counts) == -(-n // BLOCK) and all(c > 0 for c in counts[:n // BLOCK])
    if n % BLOCK > 3:
        assert counts[-1] > 0
    return D.Stream('pipe_split_%d' % n, rec, s.lib, {})


def stream_border_chain():
    """The last record of the last lean block that reaches CreateEdge and the first one of the tail block are the same
    observation of the same pair: the tail block's head finds its predecessor across the border of the two launches and is
    dropped as its duplicate; a third copy behind it is dropped inside the general form."""
    n = BLOCK + 40
    b = D.Builder(n, D.make_lib(detect_duplicate=True), filler_rows=[A])
    for i in range(5, BLOCK - 200, 97):
        S._link(b, i)
    for i in (BLOCK - 2, BLOCK + 1, BLOCK + 9):
        b.link(i, A, D.LARGE[12], 100, 120)
    S._link(b, BLOCK + 20)
    rec = b.records()
    rp = D.replay(rec, D.TABLE, b.lib)
    c = D.census(rec, b.lib, rp)
    assert c.heads == [5, BLOCK + 1] and c.dropped_heads == [BLOCK + 1]
    assert rp.reach[BLOCK - 2] and not rp.reach[BLOCK - 1] and not rp.reach[BLOCK]
    assert rp.emit[BLOCK - 2] and not rp.emit[BLOCK + 9] and rp.emit[BLOCK + 20]
    return D.Stream('pipe_border_chain', rec, b.lib, {})


# ---- rounds per block ---------------------------------------------------------------------------------------------------
# no round, one entry, one short of a round, a round, one more; 64 k entries for both residues of k modulo the unroll factor
# below the 64 sub-tiles ...
COUNTS_FEW = [0, 1, 63, 64, 65, 64 * 2, 64 * 3, 0, 65]
# ... rounds equal to the sub-tiles and one to either side, both residues above them, every record in the set, and two
# neighbours with very different counts
COUNTS_MANY = [64 * SUBS - 1, 64 * SUBS, 64 * SUBS + 1, 64 * (SUBS + 2), 64 * (SUBS + 3), BLOCK, 1]
assert UNROLL == 2 and {c // 64 % UNROLL for c in (128, 192)} == {0, 1} == {c // 64 % UNROLL for c in COUNTS_MANY[3:5]}


def stream_counts(which):
    counts = {'few': COUNTS_FEW, 'many': COUNTS_MANY}[which]
    n = len(counts) * BLOCK + 5
    b = D.Builder(n, D.make_lib(), filler_rows=[A])
    for blk, count in enumerate(counts):
        _scatter(b, blk, count)
    S._link(b, n - 2)
    rec = b.records()
    got, rounds = entry_counts(rec)
    assert got == counts + [1]
    if which == 'many':
        assert rounds[:6] == [SUBS, SUBS, SUBS + 1, SUBS + 2, SUBS + 3, BLOCK // 64]
    else:
        assert rounds[:7] == [0, 1, 1, 1, 2, 2, 3]
    return D.Stream('pipe_counts_' + which, rec, b.lib, {})


# ---- contig changes ------------------------------------------------------------------------------------------------------
# per block: the offsets of the records that lie on another contig than the record before them
CHANGES = [
    [],                                                      # none
    [1],                                                     # the block's second record
    [100],                                                   # in the first sub-tile
    [63 * SUB + 17],                                         # in the last
    [10 * SUB + 5, 11 * SUB + 250],                          # in two consecutive sub-tiles
    [s * SUB + (s * 37 + 3) % SUB for s in range(SUBS)],     # in every sub-tile
    [],
]


def stream_changes():
    n = len(CHANGES) * BLOCK + 3 * SUB + 9
    b = D.Builder(n, D.make_lib(), filler_rows=[A])
    rows = [A, B, D.LARGE[2], D.LARGE[3]]
    cuts = sorted(blk * BLOCK + o for blk, offs in enumerate(CHANGES) for o in offs) + [len(CHANGES) * BLOCK + SUB + 3]
    for k, lo in enumerate(cuts):
        hi = cuts[k + 1] if k + 1 < len(cuts) else n
        b.tid[lo:hi] = rows[(k + 1) % len(rows)]
        b.mtid[lo:hi] = rows[(k + 1) % len(rows)]
    for i in range(3, n, 41):
        S._link(b, i)
    for i in range(17, n, 1201):
        b.fishy(i, int(b.tid[i]), D.LARGE[40 + i % 5])
    rec = b.records()
    run = np.flatnonzero(rec['tid'][1:] != rec['tid'][:-1]) + 1
    assert run.tolist() == cuts
    for blk, offs in enumerate(CHANGES):
        mine = run[(run >= blk * BLOCK) & (run < (blk + 1) * BLOCK)] - blk * BLOCK
        assert sorted(set((mine // SUB).tolist())) == sorted(set(o // SUB for o in offs))
    assert sorted(set(o // SUB for o in CHANGES[5])) == list(range(SUBS)) and CHANGES[4][1] // SUB == CHANGES[4][0] // SUB + 1
    return D.Stream('pipe_changes', rec, b.lib, {})


# ---- the `mtid` path ------------------------------------------------------------------------------------------------------
def stream_mates():
    """In the pipeline's first two sub-tiles, in an even and an odd one, in the last one of a full block and in the tail
    block: a set record on a row that is absent in D.TABLE, a set record with its mate there, a mate-elsewhere record
    outside the set with its mate there (mapq 0, below min_mapq, above), one whose own contig is that row, tid -1 inside and
    outside the set, and an `mtid` that is no reference of the header."""
    n = 2 * BLOCK + SUB + 5
    b = D.Builder(n, D.make_lib(min_mapq=11), filler_rows=[A, B])
    X, Y = ABSENT[0], ABSENT[1]
    bases = [3, SUB + 9, 6 * SUB + 1, 7 * SUB + 100, 63 * SUB + 150, BLOCK + 2 * SUB + 77, 2 * BLOCK - 12, 2 * BLOCK + 30]
    outside = []
    for base in bases:
        i = base
        for mapq in (0, 5, 60):
            own = int(b.tid[i])
            b.raw(i, X, B, RD2, mapq=mapq, qlen=71)
            b.raw(i + 1, own, X, RD2, mapq=mapq, qlen=72)
            b.raw(i + 2, own, Y, RD1, mapq=mapq, qlen=73); outside.append(i + 2)
            b.raw(i + 3, own, D.LARGE[7], RD1, mapq=mapq, qlen=74); outside.append(i + 3)
            b.raw(i + 4, X, X, RD1, mapq=mapq, qlen=75)
            b.raw(i + 5, own, N_CONTIGS + 3, RD1, mapq=mapq, qlen=76)
            b.raw(i + 6, -1, B, RD2, mapq=mapq, qlen=77)
            b.raw(i + 7, -1, -1, RD1 | UN, mapq=mapq, qlen=78)
            b.raw(i + 8, own, -1, RD1, mapq=mapq, qlen=79)
            i += 9
    for i in range(8 * SUB + 1, n, 389):
        if int(b.tid[i]) == int(b.mtid[i]):
            S._link(b, i)
    rec = b.records()
    model = M.compact(rec, N_CONTIGS)
    in_set = np.unpackbits(model['set_bits'], bitorder='little')[:n].astype(bool)
    assert not in_set[outside].any() and (rec['tid'][outside] != rec['mtid'][outside]).all()
    assert in_set[[base + 5 for base in bases]].all() and in_set[[base + 6 for base in bases]].all()
    assert not in_set[[base + 7 for base in bases]].any()
    assert {(base % BLOCK) // SUB for base in bases if base < 2 * BLOCK} >= {0, 1, 6, 7, SUBS - 1} and bases[-1] >= 2 * BLOCK
    return D.Stream('pipe_mates', rec, b.lib, {})


STREAMS = dict([('split_%d' % n, (lambda n=n: stream_split(n))) for n in SPLIT_LENGTHS],
               border_chain=stream_border_chain, counts_few=lambda: stream_counts('few'),
               counts_many=lambda: stream_counts('many'), changes=stream_changes, mates=stream_mates)
# (the table with every contig present: the streams that touch the rows it changes, and one of each other kind)
CASES = [(k, 'absent') for k in sorted(STREAMS)] + [(k, 'present') for k in ('mates', 'changes', 'counts_few', 'split_%d' % (BLOCK + 1))]

_MADE, _ORACLE, _BUILDERS = {}, {}, {}


def made(key):
    if key not in _MADE:
        _MADE[key] = STREAMS[key]()
    return _MADE[key]


def oracle(key, tab):
    """(stream, batch, C oracle's workload, py oracle's result) of a stream on a table, computed once."""
    if (key, tab) not in _ORACLE:
        from oracle import py_oracle as O
        s = made(key)
        rec, _, p = D.as_oracle_inputs(s)
        wl = dict(table=D.table_columns(TABLES[tab]), lib=s.lib, node_bits=D.NODE_BITS)
        _ORACLE[(key, tab)] = (s, D.as_batch(s), wl, O.record_loop(rec, TABLES[tab], p))
    return _ORACLE[(key, tab)]


def check(key, tab, table, aligned, ctr):
    from tests import gpu_util as DU
    from tests.test_gpu_fullsize import assert_table_equals_c_oracle
    s, batch, wl, loop = oracle(key, tab)
    DU.assert_matches_oracle(table, aligned, ctr, loop, N_CONTIGS)
    assert (ctr.n_reach, ctr.n_tuples) == (loop.n_reach, sum(r.n + r.fishy for r in loop.edges.values()))
    assert_table_equals_c_oracle(table, aligned, ctr, batch, wl)


def builder(tab, grouping, n):
    """Writing keys: a builder of the stream's own size; grouping runs: one of 4.3 M tuples per table, kept."""
    import torch
    from besst_amd import pipeline
    dev = torch.device('cuda', 0)
    if not grouping:
        gb = pipeline.DeviceGraphBuilder(dev, N_CONTIGS, D.NODE_BITS, D.make_lib(), n, n)
        gb.set_contigs(**D.table_columns(TABLES[tab]))
        return gb
    if tab not in _BUILDERS:
        cap_n = max(len(COUNTS_FEW), len(COUNTS_MANY), len(CHANGES) + 1) * BLOCK + BLOCK
        gb = pipeline.DeviceGraphBuilder(dev, N_CONTIGS, D.NODE_BITS, D.make_lib(), cap_n, T.CAP)
        gb.set_contigs(**D.table_columns(TABLES[tab]))
        _BUILDERS[tab] = gb
    return _BUILDERS[tab]


def steps(gb, s, batch, side, setenv, delenv):
    """Two steps with (side) or without the side stream -> the columns S._columns compares, the presort description, form."""
    from besst_amd import pipeline
    setenv('BESST_RECORD_PATH', '1')
    for k in ('BESST_MATE_BITS', 'BESST_TID_BITS'):
        delenv(k)
    if side:
        delenv('BESST_CAND_STREAM')
    else:
        setenv('BESST_CAND_STREAM', '0')
    T.set_library(gb, s.lib)
    gb.sort_flags = 0
    rec = pipeline.DeviceRecords(batch, gb.device)
    for _ in range(2):
        gb.step(rec)
    table = gb.fetch_table()
    spec = gb._args.get('presort')
    return table, gb.aligned.cpu().numpy().copy(), gb.read_counters(), (spec[0] if spec and spec[1] else None), S._form()


@pytest.mark.parametrize('form', ['writing keys', 'grouping runs'])
@pytest.mark.parametrize('key,tab', CASES)
def test_pipelined_loop_against_both_oracles_and_the_second_form(key, tab, form, monkeypatch):
    s, batch, _, _ = oracle(key, tab)
    grouping = form == 'grouping runs'
    gb = builder(tab, grouping, len(batch))
    got = []
    for side in (True, False):
        table, aligned, ctr, spec, ran = steps(gb, s, batch, side, monkeypatch.setenv,
                                               lambda k: monkeypatch.delenv(k, raising=False))
        assert gb.params.record_path == 1 and ran == (3 if side else 2) and bool(gb.params.cand_stream) == side
        if grouping:
            assert spec is not None and spec.segmented == 1 and spec.in_record_loop == 3 and gb.sort_flags == 0
        check(key, tab, table, aligned, ctr)
        got.append(S._columns(table, aligned, ctr))
    for x, y in zip(*got):
        assert np.array_equal(x, y)


_CHILD = r'''
import os, sys
sys.path.insert(0, %(repo)r)
import numpy as np
from tests import test_gpu_side_loop_pipeline as P
from tests import test_gpu_candidate_stream as S
out = {}
for key, tab in P.CASES:
    s = P.made(key)
    batch = P.D.as_batch(s)
    for grouping in (False, True):
        gb = P.builder(tab, grouping, len(batch))
        table, aligned, ctr, spec, ran = P.steps(gb, s, batch, False, os.environ.__setitem__, lambda k: os.environ.pop(k, None))
        assert ran == 2 and not gb.params.cand_stream
        for j, col in enumerate(S._columns(table, aligned, ctr)):
            out['%%s|%%s|%%d|%%d' %% (key, tab, grouping, j)] = col
np.savez(%(path)r, **out)
print('FORM 2 SAVED', len(out))
'''


def test_equal_to_a_process_started_with_the_stream_switched_off(tmp_path, monkeypatch):
    """Every case once more against a fresh process whose environment has BESST_CAND_STREAM=0 from its start (the
    library's own switch, read once per process): the second form's columns come back in a file and equal the third's."""
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    path = str(tmp_path / 'form2.npz')
    env = dict(os.environ, BESST_CAND_STREAM='0', BESST_RECORD_PATH='1')
    for k in ('BESST_MATE_BITS', 'BESST_TID_BITS', 'BESST_STITCH_SPAN'):
        env.pop(k, None)
    out = subprocess.run([sys.executable, '-c', _CHILD % dict(repo=repo, path=path)], env=env, capture_output=True, text=True,
                         timeout=600)
    assert 'FORM 2 SAVED' in out.stdout, (out.stdout[-2000:], out.stderr[-3000:])
    want = np.load(path)
    for key, tab in CASES:
        s, batch, _, _ = oracle(key, tab) if (key, tab) in _ORACLE else (made(key), D.as_batch(made(key)), None, None)
        for grouping in (False, True):
            gb = builder(tab, grouping, len(batch))
            table, aligned, ctr, _, ran = steps(gb, s, batch, True, monkeypatch.setenv,
                                                lambda k: monkeypatch.delenv(k, raising=False))
            assert ran == 3
            for j, col in enumerate(S._columns(table, aligned, ctr)):
                assert np.array_equal(col, want['%s|%s|%d|%d' % (key, tab, grouping, j)]), (key, tab, grouping, j)
