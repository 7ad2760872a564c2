"""The candidate side stream of the resident record layout, stated in numpy (no GPU): the set rule - which records get an
entry - and the compaction - set plane, entry offsets per 16 384-record block, entry columns in record order.  The device
maker is held against this statement in tests/test_gpu_candidate_stream.py.

What the rule has to guarantee to the record loop's third form: every record the reference's loop body evaluates beyond
its coverage line - a link candidate (oracle/py_oracle.record_loop past its `continue` of CreateGraph.py:169) or a fishy
read (:141) - has an entry, and every mate-elsewhere record WITHOUT an entry has its `mtid` inside the header, so that the
streaming half may credit its coverage and count it non-unique without reading `mtid`."""
import numpy as np
import pytest

from tests import golden_util as GU
from tests import record_design as D

BLOCK = 16384
F_UNMAPPED, F_READ1, F_READ2 = 0x4, 0x40, 0x80
LENGTHS = [0, 1, 7, 8, 9, 16383, 16384, 16385, 2 * 16384 + 5]


def in_set(tid, mtid, flag, n_refs):
    tid, mtid, flag = np.asarray(tid, np.int64), np.asarray(mtid, np.int64), np.asarray(flag, np.int64)
    read2_mapped = ((flag & F_READ2) != 0) & ((flag & F_UNMAPPED) == 0)
    quirk = ((flag & F_UNMAPPED) != 0) & ((flag & F_READ1) != 0)
    outside = (mtid < 0) | (mtid >= n_refs)                  # (uint32) mtid >= n_refs
    return (tid != mtid) & (read2_mapped | quirk | outside)


def compact(rec, n_refs):
    """rec: the seven columns -> dict(set_bits, offsets, n_entries, tid, mtid, pos, mpos, flag_qlen, mapq)."""
    n = len(rec['tid'])
    s = in_set(rec['tid'], rec['mtid'], rec['flag'], n_refs)
    nblocks = (n + BLOCK - 1) // BLOCK
    counts = np.add.reduceat(s.astype(np.int64), np.arange(0, n, BLOCK)) if n else np.zeros(0, np.int64)
    offsets = np.r_[0, np.cumsum(counts)].astype(np.uint32)
    assert len(offsets) == nblocks + 1
    out = dict(set_bits=np.packbits(s, bitorder='little'), offsets=offsets, n_entries=int(s.sum()))
    for k in ('tid', 'mtid', 'pos', 'mpos'):
        out[k] = np.asarray(rec[k], np.int32)[s]
    out['flag_qlen'] = (np.asarray(rec['flag']).astype(np.uint32) | (np.asarray(rec['qlen']).astype(np.uint32) << 16))[s]
    out['mapq'] = np.asarray(rec['mapq'], np.uint8)[s]
    return out


def random_records(n, n_refs, seed, share=0.25):
    """Sorted-ish `tid`, a share of mates elsewhere (some outside the header), every flag combination the rule reads."""
    rng = np.random.default_rng(seed)
    tid = np.sort(rng.integers(-1, n_refs + 1, n)).astype(np.int32)
    mtid = np.where(rng.random(n) < 1 - share, tid, rng.integers(-2, n_refs + 3, n)).astype(np.int32)
    flag = (1 | rng.choice([F_READ1, F_READ2], n) | np.where(rng.random(n) < 0.2, F_UNMAPPED, 0) |
            rng.choice([0, 0x10, 0x20, 0x30], n)).astype(np.uint16)
    return dict(tid=tid, mtid=mtid, pos=rng.integers(0, 1 << 30, n).astype(np.int32),
                mpos=rng.integers(0, 1 << 30, n).astype(np.int32), flag=flag,
                mapq=rng.choice([0, 5, 10, 11, 60, 255], n).astype(np.uint8),
                qlen=rng.integers(0, 65536, n).astype(np.uint16))


def _loop_reads(rec, n_refs, min_mapq, cls=None, scaf=None):
    """(link, fishy) masks: the records py_oracle.record_loop takes past line 499 / into the branch of line 485.  Without a
    table: every contig present, every pair of contigs on two scaffolds (the widest either can be)."""
    tid, mtid = np.asarray(rec['tid'], np.int64), np.asarray(rec['mtid'], np.int64)
    flag, mapq = np.asarray(rec['flag'], np.int64), np.asarray(rec['mapq'], np.int64)
    ok = (tid >= 0) & (tid < n_refs) & (mtid >= 0) & (mtid < n_refs)
    t, m = np.where(ok, tid, 0), np.where(ok, mtid, 0)
    other_scaffold = t != m
    if cls is not None:
        cls, scaf = np.asarray(cls), np.asarray(scaf)
        ok &= (cls[t] != 0) & (cls[m] != 0)
        other_scaffold = scaf[t] != scaf[m]
    fishy = ok & ((flag & F_UNMAPPED) != 0) & ((flag & F_READ1) != 0) & other_scaffold
    link = ok & (tid != mtid) & ((flag & F_READ2) != 0) & ((flag & F_UNMAPPED) == 0) & (mapq >= min_mapq)
    return link, fishy


def _assert_rule_serves_the_loop(rec, n_refs, min_mapq, cls=None, scaf=None):
    s = in_set(rec['tid'], rec['mtid'], rec['flag'], n_refs)
    link, fishy = _loop_reads(rec, n_refs, min_mapq, cls, scaf)
    assert not np.any(link & ~s), 'a link candidate without an entry'
    assert not np.any(fishy & ~s), 'a fishy read without an entry'
    rest = (np.asarray(rec['tid']) != np.asarray(rec['mtid'])) & ~s
    m = np.asarray(rec['mtid'], np.int64)[rest]
    assert np.all((m >= 0) & (m < n_refs)), 'a mate-elsewhere record outside the set with its mate outside the header'
    return s, link, fishy


@pytest.mark.parametrize('name', D.STREAM_NAMES)
def test_set_holds_what_the_loop_evaluates_designed_streams(name):
    st = D.all_streams()[name]
    s, link, fishy = _assert_rule_serves_the_loop(st.records, D.N_CONTIGS, st.lib['min_mapq'], D.TABLE['cls'], D.TABLE['scaf'])
    # the same without the table's help (absent contigs, contigs of one scaffold: the rule may not lean on either)
    _assert_rule_serves_the_loop(st.records, D.N_CONTIGS, 0)
    assert s.sum() >= (link | fishy).sum()


@pytest.mark.parametrize('name', GU.scenario_names())
def test_set_holds_what_the_loop_evaluates_golden_inputs(name):
    doc, batch = GU.load(name)
    rec = {k: getattr(batch, k) for k in ('tid', 'mtid', 'pos', 'mpos', 'flag', 'mapq', 'qlen')}
    for min_mapq in (0, 11):
        _assert_rule_serves_the_loop(rec, len(batch.references), min_mapq)


def test_rule_takes_each_clause_alone():
    n_refs = 10
    rd1, rd2, un = 1 | F_READ1, 1 | F_READ2, F_UNMAPPED
    cases = [  # tid, mtid, flag, in the set
        (3, 3, rd2, False), (3, 3, rd1 | un, False),         # mate on the same reference: never
        (3, 4, rd2, True), (3, 4, rd2 | un, False),          # read 2: mapped only
        (3, 4, rd1 | un, True), (3, 4, rd1, False),          # read 1: the unmapped quirk only ...
        (3, -1, rd1, True), (3, 10, rd1, True), (3, 9, rd1, False),   # ... or a mate outside the header
        (-1, 4, rd2, True), (-1, 4, rd1, False), (-1, -1, rd2, False), (12, 11, rd1, True),
    ]
    for tid, mtid, flag, want in cases:
        assert bool(in_set([tid], [mtid], [flag], n_refs)[0]) == want, (tid, mtid, flag)


@pytest.mark.parametrize('n', LENGTHS)
def test_compaction_on_ragged_lengths(n):
    n_refs = 40
    rec = random_records(n, n_refs, seed=n + 1)
    c = compact(rec, n_refs)
    s = in_set(rec['tid'], rec['mtid'], rec['flag'], n_refs)
    assert len(c['set_bits']) == (n + 7) // 8
    assert np.array_equal(np.unpackbits(c['set_bits'], bitorder='little')[:n].astype(bool), s)
    assert not np.unpackbits(c['set_bits'], bitorder='little')[n:].any()      # bits behind the last record
    off = c['offsets'].astype(np.int64)
    assert off[0] == 0 and off[-1] == c['n_entries'] == s.sum() and np.all(np.diff(off) >= 0) and np.all(np.diff(off) <= BLOCK)
    where = np.flatnonzero(s)
    for b in range(len(off) - 1):                            # block b owns exactly its own records' entries, in record order
        mine = where[off[b]:off[b + 1]]
        assert np.all(mine // BLOCK == b)
    for k in ('tid', 'mtid', 'pos', 'mpos', 'mapq'):
        assert np.array_equal(c[k], rec[k][where])
    assert np.array_equal(c['flag_qlen'] & 0xffff, rec['flag'][where]) and np.array_equal(c['flag_qlen'] >> 16, rec['qlen'][where])
    if n >= 9:
        assert 0 < c['n_entries'] < n


# ---- the same claim made by the oracle itself: its loop over the set records alone finds what it finds over all of them ----------
def _loop_summary(loop):
    # (first_idx is a record's place in the stream it was read from: the one field that has to differ)
    edges = [(k, [(a, getattr(r, a)) for a in r.__slots__ if a != 'first_idx']) for k, r in loop.edges.items()]
    return (edges, loop.count, loop.non_unique_for_scaf, loop.nr_of_duplicates, loop.too_long, loop.fishy_reads, loop.n_reach,
            loop.prev)


def _assert_oracle_needs_only_the_set(rec, table, p, n_refs):
    """oracle/py_oracle.record_loop on every record and on the set records only: every record it takes past its line 499, or
    into the fishy branch of line 485, is a set record iff both runs give the same edge rows (every observation, in order),
    chain state and counters; a record outside the set may only add coverage and the non-unique tally."""
    from oracle import py_oracle as O
    s = in_set(rec['tid'], rec['mtid'], rec['flag'], n_refs)
    full = O.record_loop({k: list(v) for k, v in rec.items()}, table, p)
    only = O.record_loop({k: [x for x, keep in zip(v, s) if keep] for k, v in rec.items()}, table, p)
    assert _loop_summary(only) == _loop_summary(full)
    assert only.non_unique <= full.non_unique and all(a <= b for a, b in zip(only.aligned, full.aligned))


@pytest.mark.parametrize('name', D.STREAM_NAMES)
def test_oracle_over_the_set_records_alone_designed_streams(name):
    rec, table, p = D.as_oracle_inputs(D.all_streams()[name])
    _assert_oracle_needs_only_the_set(rec, table, p, D.N_CONTIGS)


@pytest.mark.parametrize('name', GU.scenario_names())
def test_oracle_over_the_set_records_alone_golden_inputs(name):
    from tests.test_gpu_graph_build import _oracle_inputs
    doc, batch = GU.load(name)
    p, rec, tab = _oracle_inputs(doc, batch)
    rec = {k: rec[k] for k in ('tid', 'mtid', 'pos', 'mpos', 'flag', 'mapq', 'qlen')}
    _assert_oracle_needs_only_the_set(rec, tab, p, len(batch.references))
