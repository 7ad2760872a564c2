"""GPU: the candidate side stream (besst_dev_candidate_offsets / besst_dev_candidate_stream, besst_lib_params.cand_stream)
and the third form of the fused record loop that reads it.

The maker is held against the numpy statement of tests/test_candidate_stream.py: set plane, offsets, entry columns.  The
loop is held against oracle/py_oracle.record_loop and the C oracle's tuple stream (test_gpu_record_borders.check: integers,
equality) and against the form with the two bit planes alone: edge table, coverage and counters equal.  Which form ran is
read from besst_dev_record_loop_form()."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import golden_util as GU
from tests import record_design as D
from tests import test_candidate_stream as M
from tests import test_gpu_record_borders as T
from tests import test_gpu_tid_bits as TB
from tests.record_design import BLOCK, SUB, N_CONTIGS

pytestmark = pytest.mark.gpu

assert BLOCK == M.BLOCK
LARGE = D.LARGE
A, B = LARGE[0], LARGE[1]
ABSENT = D.rows_of('absent')
RD1, RD2, UN = 1 | D.F_READ1, 1 | D.F_READ2 | D.F_MREVERSE, D.F_UNMAPPED


# ---- the maker ---------------------------------------------------------------------------------------------------------
def device_stream(rec, n_refs, with_bits=False):
    """The maker's output as numpy, in the shape of M.compact(); buffers are pre-filled so that an unwritten byte shows."""
    import torch
    from besst_amd import _lib
    lib = _lib.load()
    dev = torch.device('cuda', 0)
    n = len(rec['tid'])
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a.view(np.int16) if a.dtype == np.uint16 else a)).to(dev)
    d = {k: (up(v) if n else torch.zeros(4, dtype=torch.int32, device=dev)) for k, v in rec.items()}
    p = lambda t: C.c_void_p(t.data_ptr())
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    nbytes = int(lib.besst_dev_mate_bits_bytes(n))
    set_bits, mate, runs = (torch.full((nbytes,), 0xAA, dtype=torch.uint8, device=dev) for _ in range(3))
    offsets = torch.full((int(lib.besst_dev_candidate_offsets_bytes(n)) // 4,), -7, dtype=torch.int32, device=dev)
    _lib.check(lib.besst_dev_candidate_offsets(stream, n, n_refs, p(d['tid']), p(d['mtid']), p(d['flag']), p(set_bits),
                                               p(offsets), p(mate) if with_bits else None, p(runs) if with_bits else None),
               'dev_candidate_offsets')
    nblocks = (n + BLOCK - 1) // BLOCK
    off = offsets.cpu().numpy().view(np.uint32)[:nblocks + 1]
    n_entries = int(off[-1])
    size = int(lib.besst_dev_candidate_stream_bytes(n_entries))
    assert size >= 21 * (n_entries + 1)
    entries = torch.full((size,), 0x55, dtype=torch.uint8, device=dev)
    desc = _lib.CandStream()
    _lib.check(lib.besst_dev_candidate_stream(stream, n, n_refs, p(d['tid']), p(d['mtid']), p(d['pos']), p(d['mpos']),
                                              p(d['flag']), p(d['mapq']), p(d['qlen']), p(set_bits), p(offsets), n_entries,
                                              p(entries), size, C.byref(desc)), 'dev_candidate_stream')
    torch.cuda.synchronize()
    assert (desc.n_refs, desc.n_records, desc.n_entries) == (n_refs, n, n_entries)
    assert desc.offsets == offsets.data_ptr() and desc.set_bits == set_bits.data_ptr()
    raw = entries.cpu().numpy()
    base = entries.data_ptr()

    def col(addr, dtype):
        w = np.dtype(dtype).itemsize
        assert 0 <= addr - base and addr - base + (n_entries + 1) * w <= size and (addr - base) % w == 0
        return raw[addr - base:addr - base + n_entries * w].view(dtype).copy()
    k = (n + 7) // 8
    out = dict(set_bits=set_bits.cpu().numpy()[:k], offsets=off.copy(), n_entries=n_entries,
               tid=col(desc.tid, np.int32), mtid=col(desc.mtid, np.int32), pos=col(desc.pos, np.int32),
               mpos=col(desc.mpos, np.int32), flag_qlen=col(desc.flag_qlen, np.uint32), mapq=col(desc.mapq, np.uint8))
    if with_bits:
        out['mate_bits'], out['tid_bits'] = mate.cpu().numpy()[:k], runs.cpu().numpy()[:k]
    return out


def assert_same_stream(got, want):
    assert got['n_entries'] == want['n_entries']
    for k in ('set_bits', 'offsets', 'tid', 'mtid', 'pos', 'mpos', 'flag_qlen', 'mapq'):
        assert np.array_equal(got[k], want[k]), k


@pytest.mark.parametrize('n', M.LENGTHS)
def test_maker_on_ragged_lengths(n):
    n_refs = 40
    rec = M.random_records(n, n_refs, seed=n + 1)
    got = device_stream(rec, n_refs, with_bits=True)
    assert_same_stream(got, M.compact(rec, n_refs))          # (set_bits to its last byte: the bits behind the last record are 0)
    assert np.array_equal(got['mate_bits'], np.packbits(rec['tid'] != rec['mtid'], bitorder='little'))
    want_runs = np.packbits(np.r_[True, rec['tid'][1:] != rec['tid'][:-1]], bitorder='little') if n else np.zeros(0, np.uint8)
    assert np.array_equal(got['tid_bits'], want_runs)
    assert_same_stream(device_stream(rec, n_refs), M.compact(rec, n_refs))    # the planes left alone


def test_maker_no_record_in_the_set():
    rec = M.random_records(2 * BLOCK + 5, 40, seed=3)
    rec['mtid'] = rec['tid'].copy()
    got = device_stream(rec, 40)
    assert got['n_entries'] == 0 and not got['offsets'].any() and not got['set_bits'].any()


def test_maker_every_record_in_the_set():
    rec = M.random_records(BLOCK, 40, seed=4)
    rec['tid'][:] = 3
    rec['mtid'][:] = 5
    rec['flag'][:] = RD2
    got = device_stream(rec, 40)
    assert got['n_entries'] == BLOCK and got['offsets'].tolist() == [0, BLOCK] and np.all(got['set_bits'] == 0xff)
    assert_same_stream(got, M.compact(rec, 40))


def test_maker_mate_outside_the_header_on_mapped_read1():
    n, n_refs = BLOCK + 9, 40
    rec = M.random_records(n, n_refs, seed=5, share=0.0)
    rec['mtid'] = rec['tid'].copy()
    rec['tid'] = np.clip(rec['tid'], 0, n_refs - 1)
    rec['mtid'] = rec['tid'].copy()
    rec['flag'][:] = RD1
    where = {7: -1, 8: n_refs, 100: n_refs + 5, BLOCK - 1: -1, BLOCK: n_refs, BLOCK + 8: 2 ** 31 - 1}
    inside = {9: (int(rec['tid'][9]) + 1) % n_refs}          # a mapped read 1 with its mate elsewhere INSIDE the header: no entry
    for i, m in list(where.items()) + list(inside.items()):
        rec['mtid'][i] = m
    got = device_stream(rec, n_refs)
    assert np.flatnonzero(np.unpackbits(got['set_bits'], bitorder='little')).tolist() == sorted(where)
    assert_same_stream(got, M.compact(rec, n_refs))


# ---- the third form of the loop ---------------------------------------------------------------------------------------------
def _form():
    from besst_amd import _lib
    return int(_lib.load().besst_dev_record_loop_form())


def _steps(gb, name, side, monkeypatch, n_refs_of_stream=None):
    """Two steps on the builder with (side) or without the side stream -> table, coverage, counters, presort, form."""
    from besst_amd import pipeline
    monkeypatch.setenv('BESST_RECORD_PATH', '1')
    for k in ('BESST_MATE_BITS', 'BESST_TID_BITS'):
        monkeypatch.delenv(k, raising=False)
    if side:
        monkeypatch.delenv('BESST_CAND_STREAM', raising=False)
    else:
        monkeypatch.setenv('BESST_CAND_STREAM', '0')         # (pipeline.DeviceRecords hands no stream over)
    s, batch, _, _ = T.oracle(name)
    T.set_library(gb, s.lib)
    gb.sort_flags = 0
    rec = pipeline.DeviceRecords(batch, gb.device, n_refs=n_refs_of_stream)
    for _ in range(2):
        gb.step(rec)
    table = gb.fetch_table()
    spec = gb._args.get('presort')
    return table, gb.aligned.cpu().numpy().copy(), gb.read_counters(), (spec[0] if spec and spec[1] else None), _form()


def _columns(table, aligned, ctr):
    return (table.key.copy(), table.n.copy(), table.sum_obs.copy(), table.sum_obs_sq.copy(), table.obs_lo.copy(),
            table.obs_hi.copy(), table.mask.copy(), aligned, np.array([getattr(ctr, f) for f, _ in ctr._fields_]))


def both_forms(name, gb, monkeypatch, grouping=False, expect_over=False):
    """Form 3 and form 2 on one builder: each equals both oracles, and they equal each other."""
    got = []
    for side in (True, False):
        table, aligned, ctr, spec, form = _steps(gb, name, side, monkeypatch)
        assert gb.params.record_path == 1 and form == (3 if side else 2) and bool(gb.params.cand_stream) == side
        if grouping and not expect_over:
            assert spec is not None and spec.segmented == 1 and spec.in_record_loop == 3 and gb.sort_flags == 0
        T.check(name, table, aligned, ctr)
        got.append(_columns(table, aligned, ctr))
    for x, y in zip(*got):
        assert np.array_equal(x, y)


@pytest.fixture(scope='module')
def runs_builder():
    yield T.make_large_builder()


@pytest.mark.parametrize('name', D.STREAM_NAMES)
def test_designed_streams_writing_keys(name, monkeypatch):
    both_forms(name, T.small_builder(name), monkeypatch)


@pytest.mark.parametrize('name', D.STREAM_NAMES)
def test_designed_streams_grouping_runs(name, runs_builder, monkeypatch):
    both_forms(name, runs_builder, monkeypatch, grouping=True, expect_over=bool(T.oracle(name)[0].claims.get('over')))


def _link(b, i, k=0, **kw):
    row = int(b.tid[i])
    b.link(i, row, LARGE[10 + (i + k) % 20], *D.distinct_obs(i), **kw)


ENTRY_COUNTS = [0, 63, 64, 65, BLOCK]


def stream_entry_counts():
    """Blocks of 0, 63, 64, 65 and 16 384 entries - no round, one short of a round, a round, a round and one, 256 rounds
    behind 64 sub-tiles - and five records on the element-wise path behind them."""
    n = len(ENTRY_COUNTS) * BLOCK + 5
    b = D.Builder(n, D.make_lib(), filler_rows=[A])
    for blk, count in enumerate(ENTRY_COUNTS):
        step = max(1, BLOCK // max(count, 1))
        at = [blk * BLOCK + (j * step + (7 if count < BLOCK else 0)) % BLOCK for j in range(count)]
        assert len(set(at)) == count
        for i in at:
            _link(b, i)
    _link(b, n - 2)
    rec = b.records()
    off = M.compact(rec, N_CONTIGS)['offsets']
    assert np.diff(off.astype(np.int64)).tolist() == ENTRY_COUNTS + [1]
    return D.Stream('cand_entry_counts', rec, b.lib, {})


def stream_absent_contigs():
    """The table has absent contigs (all_present false).  An absent contig as the `tid` of a set record, as its `mtid`, and as
    the `mtid` of a mate-elsewhere record outside the set with mapq 0, below min_mapq and above it: what each does to the
    non-unique tally and to the coverage - credited by the streaming half, taken back where a contig is absent."""
    n = 2 * BLOCK + 5
    b = D.Builder(n, D.make_lib(min_mapq=11), filler_rows=[A, B])
    X, Y = ABSENT[0], ABSENT[1]
    def put(i, tid, mtid, flag, **kw):
        if i < n:
            b.raw(i, int(b.tid[i]) if tid is None else tid, int(b.tid[i]) if mtid is None else mtid, flag, **kw)
    i = 3 * SUB
    for mapq in (0, 5, 60):                                  # a sub-tile of a full block, then on into the next ones
        for rep in range(3):
            put(i, X, B, RD2, mapq=mapq, qlen=71); i += 1            # set record on an absent contig
            put(i, None, X, RD2, mapq=mapq, qlen=72); i += 1         # set record, mate on an absent contig
            put(i, None, Y, RD1, mapq=mapq, qlen=73); i += 1         # outside the set, mate on an absent contig
            put(i, None, LARGE[7], RD1, mapq=mapq, qlen=74); i += 1  # outside the set, both present
            put(i, X, None, RD1, mapq=mapq, qlen=75); i += 1         # outside the set, ITS contig absent
            put(i, None, N_CONTIGS + 3, RD1, mapq=mapq, qlen=76); i += 1   # in the set by the last clause only
            put(i, None, -1, RD1, mapq=mapq, qlen=77); i += 1
            i += 97
        i = {0: BLOCK + 5 * SUB, 5: 2 * BLOCK - 11}.get(mapq, i)     # ... another block, and across into the last block
    for mapq, i in ((0, 2 * BLOCK + 1), (60, 2 * BLOCK + 2)):
        put(i, None, Y, RD1, mapq=mapq, qlen=78)
    for i in range(7 * SUB + 1, 2 * BLOCK, 389):
        if int(b.tid[i]) == int(b.mtid[i]):
            _link(b, i)
    return D.Stream('cand_absent', b.records(), b.lib, {})


def stream_tid_minus_one():
    """Records with tid -1: in the set with a mate inside the header (read 2) and by the last clause, and outside the set."""
    n = 2 * BLOCK + 5
    b = D.Builder(n, D.make_lib(), filler_rows=[A])
    for base in (2 * SUB + 3, BLOCK + SUB + 1, 2 * BLOCK + 1):
        b.raw(base, -1, B, RD2, mapq=60, qlen=81)
        b.raw(base + 1, -1, B, RD1, mapq=0, qlen=82)
        b.raw(base + 2, -1, N_CONTIGS, RD1, mapq=0, qlen=83)
        b.raw(base + 3, -1, -1, RD1 | UN, mapq=0, qlen=84)
        if base + 5 < n:
            _link(b, base + 5)
    return D.Stream('cand_tid_minus_one', b.records(), b.lib, {})


def stream_low_mapq():
    """Set records whose mapq fails the link test (0 and below min_mapq): entries that only count, between links."""
    n = 2 * BLOCK + 5
    b = D.Builder(n, D.make_lib(min_mapq=11), filler_rows=[A])
    for j, i in enumerate(range(5, n, 41)):
        if j % 3 == 2:
            _link(b, i)
        else:
            _link(b, i, mapq=(0, 10)[j % 3])
    return D.Stream('cand_low_mapq', b.records(), b.lib, {})


def stream_lengths(n):
    b = D.Builder(n, D.make_lib(), filler_rows=[A, B])
    for i in range(3, n, 29):
        _link(b, i)
    for i in range(11, n, 977):
        b.fishy(i, int(b.tid[i]), LARGE[40 + i % 5])
    return D.Stream('cand_len_%d' % n, b.records(), b.lib, {})


OWN = dict(entry_counts=stream_entry_counts, absent=stream_absent_contigs, tid_minus_one=stream_tid_minus_one,
           low_mapq=stream_low_mapq, short=lambda: stream_lengths(BLOCK - 100), two_blocks_less_one=lambda: stream_lengths(2 * BLOCK - 1))


@pytest.mark.parametrize('form', ['writing keys', 'grouping runs'])
@pytest.mark.parametrize('stream', sorted(OWN))
def test_third_form_at_its_own_borders(stream, form, runs_builder, monkeypatch):
    name = TB.register(OWN[stream]())
    gb = runs_builder if form == 'grouping runs' else T.small_builder(name)
    both_forms(name, gb, monkeypatch, grouping=form == 'grouping runs')


def test_stream_made_for_another_header_is_not_honoured(monkeypatch):
    """A stream of n_refs != the call's n_contigs: the loop runs with the two bit planes, same result."""
    from besst_amd import pipeline
    name = TB.register(stream_lengths(2 * BLOCK - 1))
    gb = T.small_builder(name)
    monkeypatch.setenv('BESST_RECORD_PATH', '1')
    for k in ('BESST_MATE_BITS', 'BESST_TID_BITS', 'BESST_CAND_STREAM'):
        monkeypatch.delenv(k, raising=False)
    s, batch, _, _ = T.oracle(name)
    T.set_library(gb, s.lib)
    rec = pipeline.DeviceRecords(batch, gb.device, n_refs=N_CONTIGS - 1)
    assert rec._cand is not None and rec._cand[0].n_refs == N_CONTIGS - 1
    monkeypatch.setattr(rec, 'candidate_stream', lambda n_refs: C.addressof(rec._cand[0]))   # (the builder would remake it)
    for _ in range(2):
        gb.step(rec)
    assert bool(gb.params.cand_stream) and _form() == 2
    T.check(name, gb.fetch_table(), gb.aligned.cpu().numpy(), gb.read_counters())
    monkeypatch.undo()
    monkeypatch.setenv('BESST_RECORD_PATH', '1')
    rec = pipeline.DeviceRecords(batch, gb.device, n_refs=N_CONTIGS)      # made with the bits, in one pass
    assert rec._cand is not None and rec.mate_bits is not None and rec.tid_bits is not None
    for _ in range(2):
        gb.step(rec)
    assert _form() == 3
    T.check(name, gb.fetch_table(), gb.aligned.cpu().numpy(), gb.read_counters())


_CHILD = r'''
import sys
sys.path.insert(0, %(repo)r)
import ctypes as C
from besst_amd import _lib, pipeline
from tests import test_gpu_record_borders as T
from tests import test_gpu_tid_bits as TB
from tests import test_gpu_candidate_stream as S
name = TB.register(S.stream_lengths(2 * S.BLOCK - 1))
gb = T.small_builder(name)
s, batch, _, _ = T.oracle(name)
rec = pipeline.DeviceRecords(batch, gb.device)
assert rec.candidate_stream(S.N_CONTIGS) is None and rec.cand_stream_bytes == 0
rec._make_stream(S.N_CONTIGS, with_bits=False)               # handed over all the same: the library's own switch decides
rec.candidate_stream = lambda n_refs: C.addressof(rec._cand[0])
for _ in range(2):
    gb.step(rec)
assert bool(gb.params.cand_stream) and _lib.load().besst_dev_record_loop_form() == 2
T.check(name, gb.fetch_table(), gb.aligned.cpu().numpy(), gb.read_counters())
print('FORM 2 EQUAL')
'''


def test_switched_off_in_a_child_process():
    """BESST_CAND_STREAM=0 in the environment of a fresh process: no stream is made, and one handed over all the same is
    not honoured."""
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, BESST_CAND_STREAM='0', BESST_RECORD_PATH='1')
    for k in ('BESST_MATE_BITS', 'BESST_TID_BITS', 'BESST_STITCH_SPAN'):
        env.pop(k, None)
    out = subprocess.run([sys.executable, '-c', _CHILD % dict(repo=repo)], env=env, capture_output=True, text=True, timeout=300)
    assert 'FORM 2 EQUAL' in out.stdout, (out.stdout[-2000:], out.stderr[-3000:])


def test_resident_builder_every_contig_present(monkeypatch):
    """DeviceGraphBuilder.step() - what the benchmark times - on a dense library whose table holds every contig (the loop's
    all_present path): the table with the side stream equals the table without it and the C oracle's."""
    import torch
    from besst_amd import pipeline, workload
    from tests.test_gpu_fullsize import assert_table_equals_c_oracle
    for k in ('BESST_MATE_BITS', 'BESST_TID_BITS', 'BESST_RECORD_PATH'):
        monkeypatch.delenv(k, raising=False)
    dev = torch.device('cuda', 0)
    wl = workload.make_device(dev, 'C3', 0, pairs=1_000_000, nc=4000)
    tables = []
    for side in (True, False):
        if side:
            monkeypatch.delenv('BESST_CAND_STREAM', raising=False)
        else:
            monkeypatch.setenv('BESST_CAND_STREAM', '0')
        rec = pipeline.DeviceRecords.from_columns(wl['cols'])
        gb = pipeline.DeviceGraphBuilder(dev, wl['asm'].nc, wl['node_bits'], wl['lib'], rec.n, rec.n)
        gb.set_contigs(**wl['table'])
        for _ in range(2):
            gb.step(rec)
        assert gb.params.record_path == 1 and _form() == (3 if side else 2)
        assert (rec.cand_stream_bytes > 0) == side
        table, ctr = gb.fetch_table(), gb.read_counters()
        assert_table_equals_c_oracle(table, gb.aligned.cpu().numpy(), ctr, wl['batch'], wl)
        tables.append(_columns(table, gb.aligned.cpu().numpy().copy(), ctr))
    for a, b in zip(*tables):
        assert np.array_equal(a, b)


# ---- the context layer: the stream is extended at a build for what was pushed since the last one --------------------------------
def _context(monkeypatch):
    from besst_amd import device
    monkeypatch.setenv('BESST_RECORD_PATH', '1')
    for k in ('BESST_MATE_BITS', 'BESST_TID_BITS', 'BESST_CAND_STREAM'):
        monkeypatch.delenv(k, raising=False)
    return device.GraphContext(0)


def _set_library(ctx, lib):
    ctx.set_library(lib['read_len'], lib['ins_size_threshold'], lib['min_mapq'], lib['orientation'], lib['detect_duplicate'],
                    lib['extend_paths'], lib['no_score'])


def stream_with_far_mates(n):
    """stream_lengths(n) + mapped read 1 records whose mate lies on one of the table's last eight contigs: outside the set
    for this table, inside it (last clause) for a header that is eight references shorter."""
    s = stream_lengths(n)
    rec = {k: v.copy() for k, v in s.records.items()}
    for j, i in enumerate(range(17, n, 1201)):
        rec['mtid'][i], rec['flag'][i], rec['mapq'][i] = N_CONTIGS - 2 - (j % 2) * 2, RD1, (0, 60)[j % 2]
    return D.Stream('cand_far_%d' % n, rec, s.lib, {})


PUSHES = {
    # cuts inside a block and on a block border; the buffers of the first build hold the later ones: pure extension
    'extended': [0, 2 * BLOCK - 3000, 2 * BLOCK, 2 * BLOCK + 2500],
    # every build outgrows what the one before allocated: the stream is made anew each time
    'regrown': [0, 5001, 2 * BLOCK, 3 * BLOCK + 77],
}


@pytest.mark.parametrize('how', sorted(PUSHES))
def test_context_extends_the_stream_over_pushes_and_builds(how, monkeypatch):
    """push - build - push - build - push - build: every build equals the oracle on the records pushed so far (what one push
    of them gives), through the third form."""
    cuts = PUSHES[how]
    names = [TB.register(stream_with_far_mates(c)) for c in cuts[1:]]
    s, batch, wl, _ = T.oracle(names[-1])
    with _context(monkeypatch) as ctx:
        ctx.set_contigs(**wl['table'])
        _set_library(ctx, s.lib)
        for name, lo, hi in zip(names, cuts[:-1], cuts[1:]):
            ctx.push_records(batch.slice(lo, hi))
            for _ in range(2):                               # (the second build finds the stream as the first left it)
                T.check(name, *ctx.build_graph())
                assert _form() == 3


def test_context_pushed_in_three_parts_equals_one_push(monkeypatch):
    cuts = PUSHES['extended']
    name = TB.register(stream_with_far_mates(cuts[-1]))
    s, batch, wl, _ = T.oracle(name)
    got = []
    for parts in (cuts, [0, cuts[-1]]):
        with _context(monkeypatch) as ctx:
            ctx.set_contigs(**wl['table'])
            _set_library(ctx, s.lib)
            for lo, hi in zip(parts[:-1], parts[1:]):
                ctx.push_records(batch.slice(lo, hi))
            table, aligned, ctr = ctx.build_graph()
            assert _form() == 3
            T.check(name, table, aligned, ctr)
            got.append(_columns(table, aligned, ctr))
    for x, y in zip(*got):
        assert np.array_equal(x, y)


def test_context_makes_the_stream_anew_for_another_contig_count(monkeypatch):
    """A build with a table eight contigs shorter leaves a stream whose set holds the records with a mate on those eight; the
    build with the full table may not read it."""
    name = TB.register(stream_with_far_mates(2 * BLOCK + 2500))
    s, batch, wl, _ = T.oracle(name)
    short = {k: v[:N_CONTIGS - 8] for k, v in wl['table'].items()}
    with _context(monkeypatch) as ctx:
        ctx.set_contigs(**short)
        _set_library(ctx, s.lib)
        ctx.push_records(batch)
        ctx.build_graph()
        assert _form() == 3
        ctx.set_contigs(**wl['table'])
        T.check(name, *ctx.build_graph())
        assert _form() == 3


# ---- the golden inputs (streams captured from the reference's own runs, 24 k - 60 k records: full blocks + a last one) ------------
@pytest.mark.parametrize('name', GU.scenario_names())
def test_golden_inputs_third_form_against_both_oracles_and_second_form(name, monkeypatch):
    """Every golden scenario through the context layer with the fused loop forced: with the side stream (form 3) and with
    BESST_CAND_STREAM=0 (form 2) - each equal to py_oracle.record_loop and to the C oracle's tuple stream and aggregation,
    and the two equal to each other: edge table, coverage, counters."""
    from oracle import py_oracle as O
    from tests import gpu_util as DU
    from tests.test_gpu_fullsize import assert_table_equals_c_oracle
    from tests.test_gpu_graph_build import _oracle_inputs
    monkeypatch.setenv('BESST_RECORD_PATH', '1')
    for k in ('BESST_MATE_BITS', 'BESST_TID_BITS'):
        monkeypatch.delenv(k, raising=False)
    doc, batch = GU.load(name)
    assert len(batch) > BLOCK                                # (at least one block takes its rounds from the stream)
    p, rec, tab = _oracle_inputs(doc, batch)
    loop = O.record_loop(rec, tab, p)
    lib = dict(read_len=p.read_len, ins_size_threshold=p.ins_size_threshold, min_mapq=p.min_mapq, orientation=p.orientation,
               detect_duplicate=p.detect_duplicate, extend_paths=p.extend_paths, no_score=p.no_score)
    got = []
    for side in (True, False):
        if side:
            monkeypatch.delenv('BESST_CAND_STREAM', raising=False)
        else:
            monkeypatch.setenv('BESST_CAND_STREAM', '0')
        table, aligned, ctr = DU.device_build(batch, tab, p, chunks=3 if side else 1)
        assert _form() == (3 if side else 2)
        DU.assert_matches_oracle(table, aligned, ctr, loop, len(batch.references))
        assert_table_equals_c_oracle(table, aligned, ctr, batch,
                                     dict(table=DU.table_columns(tab), lib=lib, node_bits=table.node_bits))
        got.append(_columns(table, aligned, ctr))
    for x, y in zip(*got):
        assert np.array_equal(x, y)
