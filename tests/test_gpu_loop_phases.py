"""GPU: the lean side-stream loop in two phases, and the running coverage sum it carries through both.

A block of the lean form runs phase 1 - a round paired with a sub-tile, unrolled by two - while rounds remain, rounded up to a
whole pair, and phase 2 - the streaming half alone - over the sub-tiles that are left; the last round of phase 1 is finished
at the top of phase 2, or behind phase 1 where no sub-tile is left.  The coverage of the sub-tiles that lie on one contig is
a running (contig, sum) of the wave, written with one atomic when the contig changes or the block ends - in whichever phase
that happens.  What can go wrong is at the borders of the two: the number of rounds against the pair and against the 64
sub-tiles, the `tid` buffer and the running contig across the hand-over, the `mtid` path inside phase 2, coverage credited in
one phase and taken back in the other, the chain's state behind the last round - and, for the sum, where it is flushed, what a
mixed sub-tile leaves of it, how large it grows, and a running contig that is no row of the table.

Streams are 2 * BLOCK + SUB + 5 records long: two lean blocks that differ and a block for the general form.  Every case runs
the side-stream form writing keys and grouping runs, on the designed table (absent contigs) and on the one with every contig
present, with BESST_LOOP_SPEC unset and =0 (the specialised and the generic lean instance), and compares edge table, coverage
and counters with oracle/py_oracle.record_loop and with the C oracle; the two instances must agree column by column.  The
generators assert on the CPU that a stream has the property it is named for, and state the rounds of every block and the
positions of its run bits (tests/test_loop_phases_design.py runs them without a GPU)."""
import numpy as np
import pytest

from tests import record_design as D
from tests import test_candidate_stream as M
from tests import test_gpu_candidate_stream as S
from tests import test_gpu_side_loop_pipeline as P
from tests.record_design import BLOCK, SUB, N_CONTIGS

pytestmark = pytest.mark.gpu

N = 2 * BLOCK + SUB + 5
SUBS = BLOCK // SUB
A, B, C3, C4 = D.LARGE[0], D.LARGE[1], D.LARGE[2], D.LARGE[3]
X, Y = P.ABSENT[0], P.ABSENT[1]
RD1, RD2 = S.RD1, S.RD2
LIB = D.make_lib(min_mapq=11)


def phase1_end(rounds):
    """The first iteration of phase 2: the rounds, rounded up to a whole unrolled pair (classify.hip: phase 1's `iters`)."""
    return (rounds + P.UNROLL - 1) // P.UNROLL * P.UNROLL


def facts(rec, lib=LIB):
    """What the CPU twin holds a stream's claims against: the rounds of every block by the side stream's set rule
    (tests/test_candidate_stream.py), the rounds D.census counts from the evaluable records, the positions of the run bits
    (records on another contig than the record before them), and the entry number of every record of the set in its block."""
    model = M.compact(rec, N_CONTIGS)
    in_set = np.unpackbits(model['set_bits'], bitorder='little')[:len(rec['tid'])].astype(bool)
    _, rounds = P.entry_counts(rec)
    rp = D.replay(rec, D.TABLE, lib)
    c = D.census(rec, lib, rp)
    entry = np.full(len(in_set), -1, np.int64)
    for lo in range(0, len(in_set), BLOCK):
        idx = lo + np.flatnonzero(in_set[lo:lo + BLOCK])
        entry[idx] = np.arange(len(idx))
    runs = (np.flatnonzero(rec['tid'][1:] != rec['tid'][:-1]) + 1).tolist()
    return dict(rounds=rounds, census_rounds=[len(r) for r in c.rounds], runs=runs, in_set=in_set, entry=entry, replay=rp, census=c)


def _segments(b, cuts, rows):
    """The contig changes at every index of `cuts` (ascending), cycling through `rows`; the stream begins on rows[0]."""
    edges = [0] + list(cuts) + [b.n]
    for k in range(len(edges) - 1):
        b.tid[edges[k]:edges[k + 1]] = rows[k % len(rows)]
        b.mtid[edges[k]:edges[k + 1]] = rows[k % len(rows)]


def _links(b, at):
    for i in at:
        assert int(b.tid[i]) == int(b.mtid[i]), i           # (a filler so far)
        S._link(b, int(i))


def _done(name, b, claims):
    """The stream, with its claims held against the facts: rounds per block and run bits as stated."""
    rec = b.records()
    f = facts(rec, b.lib)
    assert f['rounds'] == claims['rounds'], (name, f['rounds'])
    assert f['runs'] == claims['runs'], (name, f['runs'][:8])
    if claims.get('all_evaluable', True):                    # every entry is a candidate the census counts, too
        assert f['census_rounds'] == claims['rounds'], (name, f['census_rounds'])
    return D.Stream('phases_' + name, rec, b.lib, claims), f


# ---- the rounds of the first lean block ----------------------------------------------------------------------------------------
ROUNDS = [0, 1, 2, 3, 63, 64, 65, 256]
OTHER_ROUNDS = 5                                             # the second lean block's, in every stream of this kind


def entries_for(rounds):
    """The fewest entries that make `rounds` rounds - the last round holds one -, every record of the block for 256."""
    return BLOCK if rounds == BLOCK // 64 else (0 if rounds == 0 else 64 * (rounds - 1) + 1)


def stream_rounds(rounds):
    """Block 0 has `rounds` rounds: phase 2 only; the rounded-up pair, then 62 streaming iterations; even and odd hand-over;
    one phase-2 iteration pair, none, rounds that outlast the sub-tiles; every record in the set.  Block 1 has five.  The
    contig changes every 1000 records, so run bits fall into both phases."""
    b = D.Builder(N, LIB, filler_rows=[A, B])
    P._scatter(b, 0, entries_for(rounds))
    P._scatter(b, 1, entries_for(OTHER_ROUNDS))
    S._link(b, N - 2)
    runs = list(range(1000, N, 1000))
    s, f = _done('rounds_%d' % rounds, b, dict(rounds=[rounds, OTHER_ROUNDS, 1], runs=runs))
    assert rounds != OTHER_ROUNDS and SUBS == 64
    assert (phase1_end(rounds) < SUBS) == (rounds <= 62) and (phase1_end(rounds) == SUBS) == (rounds in (63, 64))
    if rounds == 256:
        assert f['in_set'][:BLOCK].all()
    return s


# ---- a contig change at the hand-over ----------------------------------------------------------------------------------------
HANDOVER_ROUNDS = [6, 5]                                     # block 0 even, block 1 odd: phase 2 begins at iteration 6 in both


def stream_handover_change(d):
    """A run bit in sub-tile n_rounds + d of both lean blocks, d = -1, 0, +1: the sub-tile of phase 1's last round, the first
    one behind the rounds, the one behind that.  With six rounds they are the last iteration of phase 1 and the first two of
    phase 2; with five, the two iterations of phase 1's rounded-up pair and the first of phase 2."""
    b = D.Builder(N, LIB, filler_rows=[A])
    cuts = [blk * BLOCK + (r + d) * SUB + 77 for blk, r in enumerate(HANDOVER_ROUNDS)] + [2 * BLOCK + SUB + 1]
    _segments(b, cuts, [A, B, C3, C4])
    for blk, r in enumerate(HANDOVER_ROUNDS):
        count = entries_for(r) + 20
        _links(b, [blk * BLOCK + 3 + j * (BLOCK // count) for j in range(count)])
    S._link(b, N - 2)
    s, f = _done('handover_%+d' % d, b, dict(rounds=HANDOVER_ROUNDS + [1], runs=cuts))
    assert [phase1_end(r) for r in HANDOVER_ROUNDS] == [6, 6]
    assert [(c % BLOCK) // SUB - r for c, r in zip(cuts, HANDOVER_ROUNDS)] == [d, d]
    return s


# ---- absent contigs inside phase 2 ---------------------------------------------------------------------------------------------
def stream_absent_in_phase2():
    """Block 0 has two rounds, block 1 three: in the first pair of phase 2, in an even and an odd iteration of its loop and in
    the block's last sub-tile stand mate-elsewhere records OUTSIDE the set whose mate lies on an absent row of the designed table
    (mapq 0, below min_mapq and above it: counted non-unique or not, credited and taken back or not), one with both contigs
    present, and one whose own contig is the absent row."""
    b = D.Builder(N, LIB, filler_rows=[A, B])
    _links(b, [3 + 5 * j for j in range(100)])                              # 100 entries in the first two sub-tiles
    _links(b, [BLOCK + 3 + 5 * j for j in range(150)])                      # 150 in the first three
    S._link(b, N - 2)
    subs = {0: [2, 3, 10, 11, SUBS - 1], 1: [4, 5, 20, 21, SUBS - 1]}
    outside, on_absent = [], []
    for blk, where in subs.items():
        for st in where:
            i = blk * BLOCK + st * SUB + 31
            for mapq in (0, LIB['min_mapq'] - 1, 60):
                own = int(b.tid[i])
                b.raw(i, own, Y, RD1, mapq=mapq, qlen=73)
                b.raw(i + 1, own, D.LARGE[7], RD1, mapq=mapq, qlen=74)
                b.raw(i + 2, X, own, RD1, mapq=mapq, qlen=75)
                outside += [i, i + 1, i + 2]
                on_absent.append(i + 2)
                i += 5
    # the run bits: the filler's contig changes every 1000 records, and a record whose own contig is the absent row differs
    # from the record before it, as does the one behind it
    runs = sorted(set(range(1000, N, 1000)) | set(on_absent) | {i + 1 for i in on_absent})
    s, f = _done('absent_in_phase2', b, dict(rounds=[2, 3, 1], runs=runs, all_evaluable=True))
    assert len(on_absent) == 30 and len(runs) == len(range(1000, N, 1000)) + 60
    assert not f['in_set'][outside].any() and (s.records['tid'][outside] != s.records['mtid'][outside]).all()
    for i in outside:
        assert (i % BLOCK) // SUB >= phase1_end(f['rounds'][i // BLOCK])
    assert {(i % BLOCK) // SUB % 2 for i in outside} == {0, 1}
    return s


# ---- coverage credited in one phase, taken back in the other --------------------------------------------------------------------
def stream_takeback():
    """Entries whose coverage the streaming half credits on their mapq and their round takes back: the mate is no reference of
    the header, or lies on an absent row.  Block 0, three rounds: such entries in sub-tiles 40 and 63 - streamed in phase 2, but
    members of round 2, which phase 1 finishes.  Block 1, two rounds, all entries in the first two sub-tiles: such entries in
    round 1 - streamed in phase 1, finished at the top of phase 2."""
    b = D.Builder(N, LIB, filler_rows=[A])
    back = []

    def group(i):
        for mapq in (0, LIB['min_mapq'] - 1, 60):
            b.raw(i, A, N_CONTIGS + 3, RD1, mapq=mapq, qlen=76)
            b.raw(i + 1, A, X, RD2, mapq=mapq, qlen=72)
            back.extend([i, i + 1])
            i += 3
    _links(b, [3 + 7 * j for j in range(130)])                              # rounds 0, 1 and the first of round 2
    group(40 * SUB + 9)
    group(63 * SUB + 200)
    _links(b, [BLOCK + 2 + 4 * j for j in range(70)])                       # round 0 and the first of round 1
    group(BLOCK + SUB + 100)
    group(BLOCK + SUB + 200)
    S._link(b, N - 2)
    s, f = _done('takeback', b, dict(rounds=[3, 2, 1], runs=[], all_evaluable=False))
    assert f['in_set'][back].all()
    for i in back:
        blk, st, rnd = i // BLOCK, (i % BLOCK) // SUB, int(f['entry'][i]) // 64
        end = phase1_end(f['rounds'][blk])
        if blk == 0:
            assert st >= end and rnd == 2 and rnd + 1 < end                 # finished by iteration 3 of phase 1
        else:
            assert st < end and rnd == 1 and rnd + 1 == end                 # finished at the top of phase 2
    rp = f['replay']
    assert not rp.reach[back].any()
    return s


# ---- the chain across the hand-over --------------------------------------------------------------------------------------------
def stream_chain():
    """The last record of a lean block that reaches CreateEdge is a member of the block's final round - finished at the top of
    phase 2 in block 0 (four rounds), inside phase 1's rounded-up pair in block 1 (three) - and the first reaching record of
    the next block observes the same: the next block's head is dropped as its duplicate, and a third copy behind it."""
    b = D.Builder(N, LIB, filler_rows=[A])
    _links(b, [5 + 9 * j for j in range(64 * 3 + 10)])
    _links(b, [BLOCK + 40 + 9 * j for j in range(64 * 2 + 10)])
    last = {}
    for k, at in enumerate((BLOCK, 2 * BLOCK)):
        # (the last link of the block sits in its first sub-tiles' reach of the chain, the block's later sub-tiles stream
        # in phase 2 with the chain's state at rest)
        first = at - BLOCK + 9 * 64 * 4 + 11
        for i in (first, at + 1, at + 9):
            b.link(i, A, D.LARGE[12 + k], 100 + k, 120 + k)
        last[at] = first
    S._link(b, N - 2)
    s, f = _done('chain', b, dict(rounds=[4, 3, 1], runs=[]))
    rp, c = f['replay'], f['census']
    for at, first in last.items():
        blk = at // BLOCK - 1
        assert rp.emit[first] and not rp.reach[first + 1:at + 1].any() and rp.dup[at + 1] and rp.dup[at + 9]
        assert int(f['entry'][first]) // 64 == f['rounds'][blk] - 1 and (first % BLOCK) // SUB < SUBS - 1
    assert c.heads[1:] == [BLOCK + 1, 2 * BLOCK + 1] and c.dropped_heads == [BLOCK + 1, 2 * BLOCK + 1]
    return s


# ---- the running sum: where it is flushed, what it is carried across, how large it grows ---------------------------------------
def stream_one_contig():
    """No run bit anywhere: every sub-tile of a block is credited to one contig and the sum is reduced at the block's end only;
    the next block goes on with the same contig, so two waves add to one counter."""
    b = D.Builder(N, LIB, filler_rows=[A])
    _links(b, [100, 5000, BLOCK + 7, 2 * BLOCK + 9])
    s, f = _done('one_contig', b, dict(rounds=[1, 1, 1], runs=[]))
    assert (s.records['tid'] == A).all()
    return s


def stream_flushes():
    """Block 0: the contig changes in every sub-tile - 64 flushes.  Block 1: it changes on the block's first record and in its
    last sub-tile, and nowhere between."""
    b = D.Builder(N, LIB, filler_rows=[A])
    cuts = [s * SUB + (s * 37 + 3) % SUB for s in range(SUBS)] + [BLOCK, BLOCK + 63 * SUB + 17]
    _segments(b, cuts, [A, B, C3, C4])
    _links(b, [50 + 301 * j for j in range(40)] + [BLOCK + 9 + 700 * j for j in range(20)] + [N - 2])
    s, f = _done('flushes', b, dict(rounds=[1, 1, 1], runs=cuts))
    assert sorted({c // SUB for c in cuts[:SUBS]}) == list(range(SUBS)) and all(c % SUB for c in cuts[:SUBS])
    return s


def stream_mixed():
    """A sub-tile with two contig borders, each inside a lane's four records, between two sub-tiles that lie wholly on the contig
    the mixed one begins and ends with: its coverage goes out in atomics of its own while the running sum of the surrounding
    contig is carried across it.  In phase 1 and in phase 2 of both lean blocks."""
    b = D.Builder(N, LIB, filler_rows=[A])
    cuts = []
    for blk, subs in ((0, (1, 20)), (1, (0, 41))):
        for st in subs:
            lo = blk * BLOCK + st * SUB
            cuts += [lo + 4 * 10 + 2, lo + 4 * 30 + 1]
    _segments(b, cuts, [A, B])
    _links(b, [3 + 3 * j for j in range(70)] + [BLOCK + 600 + 3 * j for j in range(70)] + [N - 2])
    s, f = _done('mixed', b, dict(rounds=[2, 2, 1], runs=cuts))
    tid = s.records['tid']
    for c in cuts:
        assert c % 4 != 0 and tid[c // 4 * 4] != tid[c // 4 * 4 + 3]        # the border lies inside a lane's four
    for lo in sorted({c // SUB * SUB for c in cuts}):
        st = (lo % BLOCK) // SUB
        assert tid[lo] == tid[lo + SUB - 1] == A and (tid[lo + SUB:lo + 2 * SUB] == A).all()
        assert st == 0 or (tid[lo - SUB:lo] == A).all()
    assert {((c % BLOCK) // SUB) >= phase1_end(2) for c in cuts} == {False, True}
    return s


def stream_largest_sum():
    """Block 0: 16 384 covered records of qlen 65 535 on one contig - a lane adds 64 x 4 x 65 535 and the wave's running sum
    reaches 1.07 x 10^9, the largest it can be."""
    b = D.Builder(N, LIB, filler_rows=[A])
    _links(b, [100, 9000, BLOCK + 7, N - 2])
    b.qlen[:BLOCK] = 65535
    s, f = _done('largest_sum', b, dict(rounds=[1, 1, 1], runs=[]))
    rec = s.records
    assert (rec['qlen'][:BLOCK] == 65535).all() and (rec['mapq'][:BLOCK] >= LIB['min_mapq']).all()
    assert SUBS * 4 * 65535 < 2 ** 24 and BLOCK * 65535 == 1073725440 < 2 ** 31
    assert f['replay'].aligned[A] >= BLOCK * 65535
    return s


def stream_mapq_borders():
    """mapq one below min_mapq (no coverage), at min_mapq and 0 (coverage), with a qlen of their own, on both sides of a contig
    change: in phase 1 and in phase 2 of both lean blocks."""
    b = D.Builder(N, LIB, filler_rows=[A])
    cuts = [2 * SUB + 100, 30 * SUB + 6, BLOCK + 1 * SUB + 250, BLOCK + 50 * SUB + 129]
    _segments(b, cuts, [A, B, C3, C4])
    _links(b, [1000 + 5 * j for j in range(130)] + [BLOCK + 1000 + 5 * j for j in range(130)] + [N - 2])
    mq = LIB['min_mapq']
    for c in cuts:
        for k, mapq in enumerate((mq - 1, mq, 0)):
            for i, q in ((c - 3 + k, 200 + k), (c + k, 300 + k)):
                assert int(b.tid[i]) == int(b.mtid[i])
                b.mapq[i], b.qlen[i] = mapq, q
    s, f = _done('mapq_borders', b, dict(rounds=[3, 3, 1], runs=cuts))
    assert [((c % BLOCK) // SUB) >= phase1_end(3) for c in cuts] == [False, True, False, True]
    return s


def stream_outside_table():
    """The running contig at a flush is no row of the table: whole sub-tiles of records on contig id N_CONTIGS + 5 and on -1
    (their mate on the same id: coverage candidates and nothing else), followed by a contig change inside the block, and once
    up to the block's end, where the flush is the block's last."""
    b = D.Builder(N, LIB, filler_rows=[A])
    cuts = [3 * SUB, 6 * SUB + 40, 20 * SUB + 1, 23 * SUB, BLOCK + 62 * SUB - 5, 2 * BLOCK]
    _segments(b, cuts, [A, N_CONTIGS + 5, B, -1, C3, N_CONTIGS + 5, C4])
    _links(b, [7 + 5 * j for j in range(70)] + [BLOCK + 3, N - 2])
    s, f = _done('outside_table', b, dict(rounds=[2, 1, 1], runs=cuts))
    tid = s.records['tid']
    assert (tid[2 * BLOCK - 2 * SUB:2 * BLOCK] == N_CONTIGS + 5).all() and tid[2 * BLOCK] == C4
    assert (tid[3 * SUB:6 * SUB] == N_CONTIGS + 5).all() and (tid[21 * SUB:23 * SUB] == -1).all()
    off_table = (tid < 0) | (tid >= N_CONTIGS)
    assert off_table.sum() >= 7 * SUB and not f['in_set'][off_table].any() and (s.records['mtid'][tid < 0] == -1).all()
    return s


STREAMS = dict([('rounds_%d' % r, (lambda r=r: stream_rounds(r))) for r in ROUNDS] +
               [('handover_%+d' % d, (lambda d=d: stream_handover_change(d))) for d in (-1, 0, 1)],
               absent_in_phase2=stream_absent_in_phase2, takeback=stream_takeback, chain=stream_chain,
               one_contig=stream_one_contig, flushes=stream_flushes, mixed=stream_mixed, largest_sum=stream_largest_sum,
               mapq_borders=stream_mapq_borders, outside_table=stream_outside_table)
CASES = [(k, tab) for k in sorted(STREAMS) for tab in ('absent', 'present')]

_MADE, _ORACLE = {}, {}


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
        wl = dict(table=D.table_columns(P.TABLES[tab]), lib=s.lib, node_bits=D.NODE_BITS)
        _ORACLE[(key, tab)] = (s, D.as_batch(s), wl, O.record_loop(rec, P.TABLES[tab], p))
    return _ORACLE[(key, tab)]


def check(key, tab, table, aligned, ctr):
    from tests import gpu_util as DU
    from tests.test_gpu_fullsize import assert_table_equals_c_oracle
    s, batch, wl, loop = oracle(key, tab)
    DU.assert_matches_oracle(table, aligned, ctr, loop, N_CONTIGS)
    assert (ctr.n_reach, ctr.n_tuples) == (loop.n_reach, sum(r.n + r.fishy for r in loop.edges.values()))
    assert_table_equals_c_oracle(table, aligned, ctr, batch, wl)


@pytest.mark.parametrize('form', ['writing keys', 'grouping runs'])
@pytest.mark.parametrize('key,tab', CASES)
def test_two_phase_loop_against_both_oracles(key, tab, form, monkeypatch):
    s, batch, _, _ = oracle(key, tab)
    assert len(batch) == N
    grouping = form == 'grouping runs'
    gb = P.builder(tab, grouping, len(batch))
    got = []
    for switch in (None, '0'):                               # the specialised lean instance, then the generic one
        if switch is None:
            monkeypatch.delenv('BESST_LOOP_SPEC', raising=False)
        else:
            monkeypatch.setenv('BESST_LOOP_SPEC', switch)
        table, aligned, ctr, spec, ran = P.steps(gb, s, batch, True, monkeypatch.setenv,
                                                 lambda k: monkeypatch.delenv(k, raising=False))
        assert gb.params.record_path == 1 and ran == 3 and gb.params.cand_stream
        if grouping:
            assert spec is not None and spec.segmented == 1 and spec.in_record_loop == 3 and gb.sort_flags == 0
        check(key, tab, table, aligned, ctr)
        got.append(S._columns(table, aligned, ctr))
    for x, y in zip(*got):
        assert np.array_equal(x, y)
