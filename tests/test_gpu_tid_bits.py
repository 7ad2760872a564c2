"""GPU: the run bits of the resident record layout (besst_dev_record_bits, besst_lib_params.tid_bits) - one bit per record,
set where the record lies on another reference than the record before it.  With them the fused loop reads `tid` only in
the 256-record sub-tiles that hold such a record and carries the contig (cur_tid) over the others.

Checked here: the plane itself on ragged lengths beside the mate plane; the context's incremental planes when a push
begins inside a byte, on the same contig as the resident record before it and on another; the fused loop, writing keys and
grouping runs, on streams designed for the borders of the new logic (tests/record_design.Builder); and the builder path the
benchmark times.  The oracle is taken through test_gpu_record_borders.check - py_oracle.record_loop and the C oracle's tuple
stream, integers, equality -, and every device result with the plane equals the one with BESST_TID_BITS=0."""
import ctypes as C

import numpy as np
import pytest

from tests import record_design as D
from tests import test_gpu_record_borders as T
from tests.record_design import BLOCK, SUB, TABLE, N_CONTIGS

pytestmark = pytest.mark.gpu

N = 3 * BLOCK + 5            # three full blocks on the pipelined path + the element-wise last block
LARGE = D.LARGE
A, B, C3 = LARGE[0], LARGE[1], LARGE[2]
assert len({TABLE['scaf'][r] for r in (A, B, C3)}) == 3


def _run(b, lo, hi, row, mtid=None):
    b.tid[lo:hi] = row
    b.mtid[lo:hi] = row if mtid is None else mtid


def _link(b, i, k=0):
    """Record i: an accepted link from the contig the record lies on to another large one."""
    row = int(b.tid[i])
    other = LARGE[10 + (i + k) % 20]
    b.link(i, row, other, *D.distinct_obs(i))


def stream_one_contig():
    """(a) one contig over all blocks: no run bit but the stream's first, cur_tid of every block from the prologue load; the
    candidates' ring `tid` comes from cur_tid."""
    b = D.Builder(N, D.make_lib(), filler_rows=[A])
    for i in range(SUB + 3, N, 97):
        _link(b, i)
    for i in range(2 * SUB + 1, N, 1501):
        b.fishy(i, A, LARGE[40 + i % 5])
    for i in range(3 * SUB + 2, N, 2003):
        b.idle(i, A, B)
    assert np.all(b.tid == A)
    return D.Stream('tidbits_one_contig', b.records(), b.lib, dict(changes=[0]))


CHANGES = [3 * SUB, 5 * SUB + SUB - 1, 8 * SUB + 4 * 17 + 1, BLOCK - 1, BLOCK, BLOCK + 10 * SUB + 4 * 5 + 1, 2 * BLOCK - 1,
           2 * BLOCK + 7 * SUB, 3 * BLOCK - 1, 3 * BLOCK + 2]


def stream_changes():
    """(b) the contig changes at a sub-tile's first record, at its last, inside a lane's four, at a block's last record and
    at a block's first - each in a sub-tile of its own, the sub-tiles between them without a bit; at 2 BLOCK - 1 and not at
    2 BLOCK: block 2's cur_tid is the contig of block 1's last record only."""
    b = D.Builder(N, D.make_lib(), filler_rows=[A])
    assert len({c // SUB for c in CHANGES}) == len(CHANGES)
    for j, (lo, hi) in enumerate(zip(CHANGES, CHANGES[1:] + [N])):
        _run(b, lo, hi, LARGE[1 + j % 3])
    for j, c in enumerate(CHANGES):
        if c + 1 < N:
            _link(b, c + 1)                                  # the record right after the change
        if j % 2:
            _link(b, c, 1)                                   # the changed record itself
    for i in range(9 * SUB + 5, N, 611):                     # and candidates in sub-tiles without a bit
        if i not in b.wanted:
            _link(b, i)
    tid = b.tid
    assert sorted(np.flatnonzero(tid[1:] != tid[:-1]) + 1) == CHANGES
    return D.Stream('tidbits_changes', b.records(), b.lib, dict(changes=CHANGES))


def stream_every_record():
    """(c) every record on another contig than the one before: unsorted, every sub-tile loads."""
    b = D.Builder(N, D.make_lib(), filler_rows=[A])
    rows = np.asarray(LARGE[:7], np.int32)
    b.tid[:] = rows[np.arange(N) % 7]
    b.mtid[:] = b.tid
    for i in range(5, N, 53):
        _link(b, i)
    assert np.all(b.tid[1:] != b.tid[:-1])
    return D.Stream('tidbits_every_record', b.records(), b.lib, {})


def stream_out_of_range():
    """(d) runs of tid -1 and of ids beyond the table that span whole sub-tiles (one of them a block border): cur_tid is
    out of range, no coverage, a candidate among them is not evaluated - then an in-range run."""
    b = D.Builder(N, D.make_lib(), filler_rows=[A])
    un = 1 | D.F_UNMAPPED | D.F_READ1
    for i in range(2 * SUB + 9, 6 * SUB):
        b.raw(i, -1, -1, un, mapq=0)
    for i in range(6 * SUB, 9 * SUB + 7):
        b.raw(i, N_CONTIGS + 1, N_CONTIGS + 1, 1 | D.F_READ1, mapq=60)
    for i in range(BLOCK - 2 * SUB, BLOCK + 3 * SUB):
        b.raw(i, -1, -1, un, mapq=0)
    for i in range(2 * BLOCK - SUB - 1, 2 * BLOCK + 2 * SUB + 2):
        b.raw(i, N_CONTIGS + 7, N_CONTIGS + 7, 1 | D.F_READ1, mapq=60)
    rd2 = 1 | D.F_READ2 | D.F_MREVERSE
    for i in (4 * SUB + 5, BLOCK + SUB + 1):                 # candidates whose own contig is -1 / beyond the table
        b.raw(i, -1, B, rd2, mapq=60, qlen=77)
    for i in (7 * SUB + 6, 2 * BLOCK + SUB + 3):
        b.raw(i, int(b.tid[i]), C3, rd2, mapq=60, qlen=78)
    for i in (9 * SUB + 7, 9 * SUB + 8, 10 * SUB + 1, BLOCK + 3 * SUB, BLOCK + 4 * SUB + 2, 2 * BLOCK + 2 * SUB + 2,
              2 * BLOCK + 4 * SUB):                          # the in-range run behind each
        _link(b, i)
    return D.Stream('tidbits_out_of_range', b.records(), b.lib, {})


def stream_aba():
    """(e) two changes inside one sub-tile that return to the first contig: cur_tid behind it is the first contig again."""
    b = D.Builder(N, D.make_lib(), filler_rows=[A])
    for base in (4 * SUB, BLOCK + 20 * SUB, 2 * BLOCK + 63 * SUB):
        _run(b, base + 40, base + 90, B)
        _link(b, base + 39)
        _link(b, base + 41)
        _link(b, base + 90)
        if base + SUB + 3 < N:
            _link(b, base + SUB + 3)                         # in the next sub-tile: no bit there
    _run(b, 9 * SUB + 4 * 63, 9 * SUB + 4 * 63 + 3, C3)      # inside lane 63's four, back at its last record
    _link(b, 9 * SUB + 4 * 63 + 3)
    _link(b, 10 * SUB + 7)
    return D.Stream('tidbits_aba', b.records(), b.lib, {})


X = 5 * SUB + 131            # where the incremental stream changes its contig: inside a byte, inside a sub-tile


def stream_incremental(n):
    b = D.Builder(2 * BLOCK + 5, D.make_lib(), filler_rows=[A])
    _run(b, X, b.n, B)
    for i in (X - 2, X + 3, X + SUB + 9, BLOCK + 77):
        _link(b, i)
    return D.Stream('tidbits_incremental_%d' % n, b.records(n), b.lib, {})


STREAMS = dict(one_contig=stream_one_contig, changes=stream_changes, every_record=stream_every_record,
               out_of_range=stream_out_of_range, aba=stream_aba)


def register(s):
    """The stream under its name in test_gpu_record_borders' oracle cache: its check() then serves this stream too."""
    if s.name not in T._ORACLE:
        from oracle import py_oracle as O
        rec, table, p = D.as_oracle_inputs(s)
        wl = dict(table=D.table_columns(), lib=s.lib, node_bits=D.NODE_BITS)
        T._ORACLE[s.name] = (s, D.as_batch(s), wl, O.record_loop(rec, table, p))
    return s.name


def _planes(n, tid, mtid):
    import torch
    from besst_amd import _lib
    lib = _lib.load()
    dev = torch.device('cuda', 0)
    d_tid, d_mtid = torch.from_numpy(tid).to(dev), torch.from_numpy(mtid).to(dev)
    nbytes = int(lib.besst_dev_mate_bits_bytes(n))
    assert nbytes >= (n + 7) // 8
    mate, runs, old = (torch.full((nbytes,), 0xAA, dtype=torch.uint8, device=dev) for _ in range(3))
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    p = lambda t: C.c_void_p(t.data_ptr())
    _lib.check(lib.besst_dev_record_bits(stream, n, p(d_tid), p(d_mtid), p(mate), p(runs)), 'dev_record_bits')
    _lib.check(lib.besst_dev_mate_bits(stream, n, p(d_tid), p(d_mtid), p(old)), 'dev_mate_bits')
    k = (n + 7) // 8
    return mate.cpu().numpy()[:k], runs.cpu().numpy()[:k], old.cpu().numpy()[:k]


@pytest.mark.parametrize('kind', ['sorted', 'random'])
@pytest.mark.parametrize('n', [1, 7, 8, 9, 4095, 16384 + 3, 100_001])
def test_both_planes_packed(n, kind):
    rng = np.random.default_rng(n)
    tid = rng.integers(-1, 50, n).astype(np.int32)
    if kind == 'sorted':
        tid = np.sort(tid)
    mtid = np.where(rng.random(n) < 0.7, tid, rng.integers(-1, 50, n)).astype(np.int32)
    mate, runs, old = _planes(n, tid, mtid)
    want = np.packbits(np.r_[True, tid[1:] != tid[:-1]], bitorder='little')
    assert np.array_equal(runs, want)                        # (bits behind the last record: 0)
    assert np.array_equal(mate, old)
    assert np.array_equal(mate, np.packbits(tid != mtid, bitorder='little'))


@pytest.mark.parametrize('border', ['other contig', 'same contig'])
def test_context_extends_both_planes_over_pushes_and_builds(border, monkeypatch):
    """push - build - push - build on one context; the second push begins inside a byte of the planes and inside a sub-tile
    that holds no other change: its first bit compares with the resident record before it."""
    from besst_amd import device
    monkeypatch.setenv('BESST_RECORD_PATH', '1')
    monkeypatch.delenv('BESST_MATE_BITS', raising=False)
    monkeypatch.delenv('BESST_TID_BITS', raising=False)
    cut = X if border == 'other contig' else X + 2
    whole = stream_incremental(2 * BLOCK + 5)
    tid = whole.records['tid']
    assert cut % 8 != 0 and (tid[cut] != tid[cut - 1]) == (border == 'other contig')
    names = [register(stream_incremental(cut)), register(whole)]
    s, batch, wl, _ = T.oracle(names[1])
    lib = s.lib
    with device.GraphContext(0) as ctx:
        ctx.set_contigs(**wl['table'])
        ctx.set_library(lib['read_len'], lib['ins_size_threshold'], lib['min_mapq'], lib['orientation'], lib['detect_duplicate'],
                        lib['extend_paths'], lib['no_score'])
        ctx.push_records(batch.slice(0, cut))
        T.check(names[0], *ctx.build_graph())
        ctx.push_records(batch.slice(cut, len(batch)))
        T.check(names[1], *ctx.build_graph())


def _two_steps(gb, name, tid_bits, monkeypatch):
    from besst_amd import pipeline
    if tid_bits:
        monkeypatch.delenv('BESST_TID_BITS', raising=False)
    else:
        monkeypatch.setenv('BESST_TID_BITS', '0')
    s, batch, _, _ = T.oracle(name)
    T.set_library(gb, s.lib)
    gb.sort_flags = 0
    rec = pipeline.DeviceRecords(batch, gb.device)
    assert rec.mate_bits is not None and (rec.tid_bits is not None) == tid_bits
    for _ in range(2):
        gb.step(rec)
    table = gb.fetch_table()
    spec = gb._args.get('presort')
    return table, gb.aligned.cpu().numpy().copy(), gb.read_counters(), (spec[0] if spec and spec[1] else None)


@pytest.fixture(scope='module')
def runs_builder():
    """One builder of 4.3 M tuples for the module: stage 2 takes its run-grouped form, the loop groups the runs."""
    import torch
    from besst_amd import pipeline
    gb = pipeline.DeviceGraphBuilder(torch.device('cuda', 0), N_CONTIGS, D.NODE_BITS, D.make_lib(), N, T.CAP)
    gb.set_contigs(**D.table_columns())
    yield gb


@pytest.mark.parametrize('form', ['writing keys', 'grouping runs'])
@pytest.mark.parametrize('stream', sorted(STREAMS))
def test_fused_loop_at_the_borders_of_the_run_bits(stream, form, runs_builder, monkeypatch):
    monkeypatch.setenv('BESST_RECORD_PATH', '1')
    monkeypatch.delenv('BESST_MATE_BITS', raising=False)
    name = register(STREAMS[stream]())
    assert len(T.oracle(name)[1]) == N
    got = []
    for tid_bits in (True, False):
        gb = runs_builder if form == 'grouping runs' else T.small_builder(name)
        table, aligned, ctr, spec = _two_steps(gb, name, tid_bits, monkeypatch)
        assert gb.params.record_path == 1 and bool(gb.params.tid_bits) == tid_bits
        if form == 'grouping runs':
            assert spec is not None and spec.segmented == 1 and spec.in_record_loop == 3 and gb.sort_flags == 0
        T.check(name, table, aligned, ctr)
        got.append((table.key.copy(), table.n.copy(), table.sum_obs.copy(), table.sum_obs_sq.copy(), table.obs_lo.copy(),
                    aligned, np.array([getattr(ctr, f) for f, _ in ctr._fields_])))
    for x, y in zip(*got):
        assert np.array_equal(x, y)


def test_resident_builder_same_table_with_and_without_run_bits(monkeypatch):
    """DeviceGraphBuilder.step() - what the benchmark times - on a dense library (fused loop, runs named in the loop): the
    edge table with the run bits equals the table without them and the C oracle's."""
    import torch
    from besst_amd import pipeline, workload
    from tests.test_gpu_fullsize import assert_table_equals_c_oracle
    monkeypatch.delenv('BESST_MATE_BITS', raising=False)
    monkeypatch.delenv('BESST_RECORD_PATH', raising=False)
    dev = torch.device('cuda', 0)
    wl = workload.make_device(dev, 'C3', 0, pairs=2_000_000, nc=4000)
    tables = []
    for bits in ('1', '0'):
        monkeypatch.setenv('BESST_TID_BITS', bits)
        rec = pipeline.DeviceRecords.from_columns(wl['cols'])
        assert rec.mate_bits is not None and (rec.tid_bits is not None) == (bits == '1')
        gb = pipeline.DeviceGraphBuilder(dev, wl['asm'].nc, wl['node_bits'], wl['lib'], rec.n, rec.n)
        gb.set_contigs(**wl['table'])
        for _ in range(2):
            gb.step(rec)
        assert gb.params.record_path == 1 and bool(gb.params.tid_bits) == (bits == '1')
        table, ctr = gb.fetch_table(), gb.read_counters()
        assert_table_equals_c_oracle(table, gb.aligned.cpu().numpy(), ctr, wl['batch'], wl)
        tables.append((table.key.copy(), table.n.copy(), table.sum_obs.copy(), table.obs_lo.copy(), gb.aligned.cpu().numpy().copy()))
    for a, b in zip(*tables):
        assert np.array_equal(a, b)
