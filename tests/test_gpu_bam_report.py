"""GPU: the BAM report (csrc/report.hip) == tests/bam_report_model.py on every word - through the dev layer on caller-owned
columns at every alignment, through the context (pushed parts, a BAM file by either ingest), under two and three gloo ranks,
and through the command line.  The shapes are the smallest at which the kernel can go wrong: around the four-record groups,
the 512-thread step and the workgroup's piece, one stream of several pieces per workgroup of a full grid; every histogram
with all records in one bin and with every lane in another; |tlen| at the borders of the bins."""
import os

import numpy as np
import pytest

from tests import bam_report_model as M
from tests import golden_util as GU

pytestmark = pytest.mark.gpu

INT32_MAX, INT32_MIN = 2 ** 31 - 1, -2 ** 31
DTYPES = dict(tid=np.int32, mtid=np.int32, pos=np.int32, mpos=np.int32, tlen=np.int32, flag=np.uint16, mapq=np.uint8,
              qlen=np.uint16)


# ---- streams -------------------------------------------------------------------------------------------------------------
def stream(n, n_refs=37, seed=1, sort=True):
    """Records as an aligner leaves them, roughly: coordinate order with the unplaced at the end, most pairs on one
    reference, a palette of flags with every census bit, mapq and qlen mostly on one value each, |tlen| around 400 with a few
    far out - and some reference ids outside the header."""
    rng = np.random.default_rng(seed)
    tid = rng.integers(0, n_refs, n)
    tid[rng.random(n) < 0.03] = -1
    tid[rng.random(n) < 0.01] = n_refs + 2
    if sort:
        tid = tid[np.argsort(np.where(tid < 0, 1 << 40, tid), kind='stable')]             # (the unplaced sort last)
    mtid = np.where(rng.random(n) < 0.8, tid, rng.integers(-1, n_refs + 1, n))
    palette = np.array([99, 147, 83, 163, 97, 145, 65, 129, 113, 177, 73, 137, 69, 133, 77, 141, 0, 16, 4,
                        99 | 0x400, 147 | 0x400, 99 | 0x200, 147 | 0x200, 0x100 | 16, 0x800, 0x900 | 1, 0x81, 0xb1])
    flag = palette[rng.integers(0, len(palette), n)]
    tlen = np.rint(rng.normal(0, 400, n)).astype(np.int64)
    far = rng.random(n) < 0.02
    tlen[far] = rng.integers(-70000, 70000, int(far.sum()))
    mapq = np.where(rng.random(n) < 0.7, 60, rng.integers(0, 256, n))
    qlen = np.where(rng.random(n) < 0.9, 100, rng.integers(0, 65536, n))
    cols = dict(tid=tid, mtid=mtid, pos=rng.integers(-1, 1 << 30, n), mpos=rng.integers(-1, 1 << 30, n), tlen=tlen,
                flag=flag, mapq=mapq, qlen=qlen)
    return {k: np.ascontiguousarray(v.astype(DTYPES[k])) for k, v in cols.items()}


def constant(n, **values):
    base = dict(tid=0, mtid=0, pos=10, mpos=20, tlen=-300, flag=147, mapq=60, qlen=100)
    base.update(values)
    return {k: np.full(n, base[k], dtype=DTYPES[k]) for k in DTYPES}


def with_columns(cols, **over):
    out = dict(cols)
    for k, v in over.items():
        out[k] = np.ascontiguousarray(np.asarray(v).astype(DTYPES[k]))
    return out


def take(cols, order):
    return {k: np.ascontiguousarray(v[order]) for k, v in cols.items()}


# ---- the dev layer -------------------------------------------------------------------------------------------------------
class _Rec(object):
    pass


def dev_words(cols, n_refs, bins=64, offsets=0, hint=False, twice=False):
    """besst_dev_library_report on torch-owned columns whose first record lies `offsets` records (one number, or one per
    column) behind a 256-byte aligned address."""
    import torch
    from besst_amd import report
    dev = torch.device('cuda', 0)
    n = len(cols['tid'])
    offs = dict(zip(M.COLUMNS, offsets)) if isinstance(offsets, (tuple, list)) else {k: offsets for k in M.COLUMNS}
    rec = _Rec()
    rec.n = n
    keep = []
    for k in M.COLUMNS:
        a = cols[k]
        a = a.view(np.int16) if a.dtype == np.uint16 else a
        buf = torch.zeros(n + offs[k] + 8, dtype=torch.from_numpy(a[:0]).dtype, device=dev)
        buf[offs[k]:offs[k] + n] = torch.from_numpy(a).to(dev)
        keep.append(buf)
        setattr(rec, k, buf[offs[k]:offs[k] + n])
    bits = None
    if hint:
        runs = np.packbits(np.r_[True, cols['tid'][1:] != cols['tid'][:-1]], bitorder='little') if n else np.zeros(1, np.uint8)
        bits = torch.from_numpy(runs).to(dev)
    got = report.dev_report_tensor(rec, n_refs, bins, tid_bits=bits)
    out = got.cpu().numpy().view(np.uint64).copy()
    if twice:
        again = report.dev_report_tensor(rec, n_refs, bins, tid_bits=bits).cpu().numpy().view(np.uint64)
        assert np.array_equal(out, again), 'two runs of one call differ'
    return out


def assert_words(got, want, what=''):
    if not np.array_equal(got, want):
        at = np.flatnonzero(got != want)
        raise AssertionError('%s: %d words differ, first at %s: got %s, model %s' % (
            what, at.size, at[:8].tolist(), got[at[:8]].tolist(), want[at[:8]].tolist()))


LENGTHS = [0, 1, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1023, 1025, 16383, 16384, 16385, 3 * 16384 + 7]


@pytest.mark.parametrize('n', LENGTHS)
def test_lengths(n):
    cols = stream(n, seed=n + 1)
    assert_words(dev_words(cols, 37, twice=True), M.words(cols, 37, 64), 'n=%d' % n)


def test_several_pieces_per_workgroup_of_a_full_grid():
    """2^22 + 5 records: more 512-thread steps than a grid of two workgroups per CU has workgroups, so every workgroup
    walks a piece of several steps; the peeled records lie behind 2^22."""
    n = (1 << 22) + 5
    cols = stream(n, n_refs=1000, seed=3)
    got = dev_words(cols, 1000, 32768, offsets=3, twice=True)
    assert_words(got, M.words(cols, 1000, 32768), 'n=2^22+5')


@pytest.mark.parametrize('offsets', [0, 1, 2, 3, (0, 1, 2, 3, 0, 1, 2, 3), (3, 3, 3, 3, 3, 2, 3, 1), (1, 0, 0, 0, 0, 0, 0, 0)])
@pytest.mark.parametrize('n', [2, 7, 1029])
def test_alignment(offsets, n):
    """A slice of a stream: every column starts the same number of records behind an aligned address (the peeled head makes
    the rest aligned); and columns that cannot all be aligned by one head (those are read element by element)."""
    cols = stream(n, seed=11)
    assert_words(dev_words(cols, 37, offsets=offsets), M.words(cols, 37, 64), 'offsets=%r' % (offsets,))


@pytest.mark.parametrize('n_refs', [3, 1])
@pytest.mark.parametrize('shuffled', [None, 4])
def test_flag_truth_table(n_refs, shuffled):
    cols = M.flag_table(n_refs, shuffled)
    assert_words(dev_words(cols, n_refs), M.words(cols, n_refs, 64), 'flag table')


def test_reference_ids_at_the_borders():
    n_refs = 5
    ids = [-1, 0, n_refs - 1, n_refs, INT32_MAX, INT32_MIN, -2]
    tid = np.repeat(ids, len(ids) * 4)
    mtid = np.tile(np.repeat(ids, 4), len(ids))
    flag = np.tile([0x81, 0x91, 0x85, 0x41], len(ids) ** 2)
    cols = with_columns(constant(len(tid)), tid=tid, mtid=mtid, flag=flag)
    m = M.model(cols, n_refs)
    assert m['tid_out_of_range'] == 2 * 28 and m['unplaced'] == 3 * 28 and m['pairs'].sum() > 0
    assert_words(dev_words(cols, n_refs), M.words(cols, n_refs, 64), 'border ids')


def test_more_references_than_records():
    cols = stream(50, n_refs=100000, seed=5)
    assert_words(dev_words(cols, 100000), M.words(cols, 100000, 64), 'n_refs=100000')
    assert_words(dev_words(stream(0), 100000), M.words(stream(0), 100000, 64), 'no record')


# ---- contention and spread ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', [64, 5000])
def test_every_record_identical(n):
    for values in (dict(), dict(qlen=65535, mapq=255, tlen=-40000), dict(flag=0x81, tlen=7), dict(tid=-1, mtid=-1, flag=77)):
        cols = constant(n, **values)
        assert_words(dev_words(cols, 2, 32768), M.words(cols, 2, 32768), 'constant %r' % (values,))


def test_every_record_on_another_reference():
    n = 3000
    for order in (np.arange(n), np.random.default_rng(1).permutation(n)):
        cols = with_columns(constant(n), tid=order, mtid=order, flag=np.where(order % 3 == 0, 0x95, 0x91))
        assert_words(dev_words(cols, n), M.words(cols, n, 64), 'one reference per record')


@pytest.mark.parametrize('distinct', [1, 2, 63, 64])
def test_distinct_values_in_one_wave(distinct):
    """64 consecutive records (and a lane's four: 256) with 1, 2, 63 and 64 distinct tid / qlen values, short and long
    reads, in runs and interleaved."""
    for n in (64, 256, 1024):
        k = np.arange(n)
        for which in (k % distinct, k * distinct // n, (k // 4) % distinct):
            cols = with_columns(constant(n), tid=which, mtid=which, qlen=which * 1000 + 5, flag=np.where(k % 5 == 0, 0x95, 0x91))
            assert_words(dev_words(cols, 64), M.words(cols, 64, 64), 'distinct=%d n=%d' % (distinct, n))


def test_mapq_and_qlen_values():
    cols = with_columns(constant(256), mapq=np.arange(256))
    assert_words(dev_words(cols, 1), M.words(cols, 1, 64), 'mapq 0..255')
    q = np.tile([0, 1, 1023, 1024, 65534, 65535], 50)
    cols = with_columns(constant(len(q)), qlen=q)
    assert M.model(cols, 1)['qlen'][[0, 1, 1023, 1024, 65534, 65535]].tolist() == [50] * 6
    assert_words(dev_words(cols, 1), M.words(cols, 1, 64), 'qlen borders')


@pytest.mark.parametrize('bins', [1, 2, 8192, 32768, 1 << 20])
def test_tlen_at_the_borders_of_the_bins(bins):
    """0, +-1, +-(bins - 1), +-bins, +-(bins + 1), INT32_MAX, INT32_MIN, and the same around the 8192 bins a workgroup
    keeps on chip, in every class: reverse / forward read 2 with the mate on the other strand or on the same."""
    values = sorted(set([0, 1, -1, bins - 1, 1 - bins, bins, -bins, bins + 1, -bins - 1, INT32_MAX, INT32_MIN,
                         8191, -8191, 8192, -8192, 8193]))
    flags = [0x81 | 0x10, 0x81 | 0x20, 0x81, 0x81 | 0x30]
    tlen = np.repeat(values, len(flags) * 3)
    flag = np.tile(np.repeat(flags, 3), len(values))
    cols = with_columns(constant(len(tlen)), tlen=tlen, flag=flag)
    m = M.model(cols, 1, bins)
    assert m['pairs'].min() > 0 and m['innie'][bins] > 0 and m['outie'][bins] > 0 and m['tandem'][bins] > 0
    assert_words(dev_words(cols, 1, bins), M.words(cols, 1, bins), 'bins=%d' % bins)


# ---- order, hint, determinism -------------------------------------------------------------------------------------------
def test_order_and_hint():
    """One stream coordinate-sorted, name-sorted (mates side by side, references at random) and reversed: three equal
    reports, each with and without the run-bit plane as a hint, and equal to the model."""
    n = 20000
    cols = stream(n, n_refs=300, seed=21)
    want = M.words(cols, 300, 4096)
    rng = np.random.default_rng(2)
    by_name = (rng.permutation(n // 2)[:, None] * 2 + np.arange(2)[None, :]).reshape(-1)
    for what, order in (('coordinate', np.arange(n)), ('name', by_name), ('reversed', np.arange(n)[::-1])):
        part = take(cols, order)
        for hint in (False, True):
            assert_words(dev_words(part, 300, 4096, hint=hint, twice=True), want, '%s hint=%s' % (what, hint))


# ---- the context layer ----------------------------------------------------------------------------------------------------
def batch_of(cols, n_refs):
    from besst_amd.records import RecordBatch
    return RecordBatch(['c%d' % i for i in range(n_refs)], [5000 + i for i in range(n_refs)], **cols)


def new_context(n_refs):
    from besst_amd import device
    ctx = device.GraphContext(0)
    zeros = np.zeros(n_refs, dtype=np.int32)
    ctx.set_contigs(scaf_id=zeros, scaf_len=zeros, ctg_pos=zeros, ctg_len=zeros, direction=zeros, cls=zeros)
    return ctx


def test_records_pushed_in_three_ragged_parts():
    n, n_refs = 10007, 37
    cols = stream(n, n_refs, seed=31)
    batch = batch_of(cols, n_refs)
    with new_context(n_refs) as ctx:
        assert_words(ctx.library_report(64).words, M.words(stream(0), n_refs, 64), 'empty context')
        at = 0
        for cut in (1, 4098, n):
            ctx.push_records(batch.slice(at, cut))
            at = cut
            before = ctx.layout_state()
            rep = ctx.library_report(64)
            assert ctx.layout_state() == before
            assert_words(rep.words, M.words(take(cols, np.arange(cut)), n_refs, 64), 'first %d records' % cut)
        assert rep.n_records == n and (rep.n_refs, rep.isize_bins) == (n_refs, 64)
        assert ctx.library_report().isize_bins == 32768


@pytest.fixture(scope='module')
def golden_file(tmp_path_factory):
    from tests import bam_writer
    doc, batch = GU.load('fr_infer')
    path = str(tmp_path_factory.mktemp('bam_report') / 'fr_infer.bam')
    bam_writer.write_bam(path, batch, block_bytes=20000, align_records=False)
    return path, doc, batch


@pytest.mark.parametrize('mode', ['device', 'host'])
def test_open_bam_report(golden_file, mode, monkeypatch):
    """A BAM file through open_bam(...).report() == the model on read_bam's columns, by the device ingest and by the host's;
    the layout the ingest left is the same before and after."""
    from besst_amd import bamio
    path, doc, batch = golden_file
    monkeypatch.setenv('BESST_INGEST', mode)
    host = bamio.read_bam(path, threads=2)
    n_refs = len(host.references)
    bam = bamio.open_bam(path, threads=2)
    try:
        assert type(bam).__name__ == 'ResidentBam' and bam.ingest.on_device == (1 if mode == 'device' else 0)
        before = bam.layout_state()
        rep = bam.report(4096)
        assert bam.layout_state() == before
        assert_words(rep.words, M.words(host, n_refs, 4096), mode)
        assert rep.references == list(host.references) and rep.lengths == [int(x) for x in host.lengths]
        assert rep.n_records == len(batch) and rep.digest == M.digest_py(M.columns_of(host))
        assert rep.pair_classes.tolist() == [14212, 0, 0, 0]
    finally:
        bam.close()


@pytest.mark.parametrize('env', [dict(BESST_RECORD_PATH='1'), dict(BESST_RECORD_PATH='1', BESST_CAND_STREAM='0'),
                                 dict(BESST_RECORD_PATH='0')], ids=['side_stream', 'fused', 'two_pass'])
def test_a_build_after_a_report_is_the_build_without_one(golden_file, env, monkeypatch):
    """Edge table, coverage and counters of the first build, and the layout state after it, with a report between ingest
    and build and without one - in the loop forms the file reaches."""
    from besst_amd import bamio
    from tests import gpu_util as DU
    from tests.test_gpu_candidate_stream import _columns, _form
    from tests.test_gpu_graph_build import _oracle_inputs
    path, doc, batch = golden_file
    for k in ('BESST_MATE_BITS', 'BESST_TID_BITS', 'BESST_CAND_STREAM', 'BESST_INGEST_LAYOUT', 'BESST_RECORD_PATH'):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    p, _rec, tab = _oracle_inputs(doc, batch)
    results = []
    for with_report in (False, True):
        bam = bamio.ResidentBam(path, threads=2, mode='device', chunk_blocks=64)
        try:
            if with_report:
                before = bam.layout_state()
                assert bam.report().n_records == len(batch)
                assert bam.layout_state() == before
            bam.ctx.set_contigs(**DU.table_columns(tab))
            bam.ctx.set_library(p.read_len, p.ins_size_threshold, p.min_mapq, p.orientation, p.detect_duplicate, p.extend_paths,
                                p.no_score)
            out = _columns(*bam.ctx.build_graph())
            results.append((out, bam.layout_state(), _form()))
        finally:
            bam.close()
    (a, state_a, form_a), (b, state_b, form_b) = results
    assert form_a == form_b and state_a == state_b
    assert len(a[0]) > 10 and len(a) == len(b)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)


# ---- sharded --------------------------------------------------------------------------------------------------------------
def _rank(rank, world, port, path, out):
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    import torch
    import torch.distributed as dist
    from besst_amd import bamio, sharded
    torch.cuda.set_device(0)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    sharded.enable()
    try:
        os.environ['BESST_SHARDED'] = '0'
        one = bamio.open_bam(path, threads=2, chunk_blocks=64)
        assert type(one).__name__ == 'ResidentBam'
        single = one.report(4096)
        one.close()
        os.environ['BESST_SHARDED'] = '1'
        many = bamio.open_bam(path, threads=2, chunk_blocks=64)
        assert type(many).__name__ == 'ShardedBam' and sum(many.head.slice_records) == single.n_records
        got = many.report(4096)
        many.close()
        host = bamio.read_bam(path, threads=2)
        assert_words(single.words, M.words(host, len(host.references), 4096), 'single process')
        assert_words(got.words, single.words, 'rank %d of %d' % (rank, world))
        assert got.references == single.references and got.lengths == single.lengths
        out.put((rank, got.n_records, len(many.slice)))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize('world', [2, 3])
def test_sharded_report_on_every_rank(world, golden_file):
    """Two and three gloo ranks on the one GPU, each with its slice of the file: every rank's report == the single-process
    report of the same file == the model."""
    import torch.multiprocessing as mp
    from tests.test_sharded_dropin_cpu import _free_port
    path, doc, batch = golden_file
    ctx = mp.get_context('spawn')
    out = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_rank, args=(r, world, port, path, out)) for r in range(world)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(900)
        if p.is_alive():
            p.kill()
        assert p.exitcode == 0
    got = sorted(out.get(timeout=5) for _ in range(world))
    assert [g[0] for g in got] == list(range(world)) and all(g[1] == len(batch) for g in got)
    assert sum(g[2] for g in got) == len(batch) and sum(1 for g in got if g[2]) > 1          # (more than one slice holds records)


# ---- the command line -------------------------------------------------------------------------------------------------------
def _tree(out):
    files = {}
    for base, _dirs, names in os.walk(out):
        for name in names:
            with open(os.path.join(base, name), 'rb') as fh:
                files[os.path.relpath(os.path.join(base, name), out)] = fh.read()
    return files


def _untimed(stats):
    import re
    return [l for l in stats.decode().split('\n') if not re.search(r'\btime\b|elapsed', l, re.I)]     # (wall times)


@pytest.fixture(scope='module')
def cli_inputs(tmp_path_factory):
    from tests import bam_writer
    d = tmp_path_factory.mktemp('bam_report_cli')
    doc, batch = GU.load('fr_infer')
    doc2, batch2 = GU.load('rf_contam')
    bams = [str(d / 'lib1.bam'), str(d / 'lib2.bam')]
    bam_writer.write_bam(bams[0], batch, block_bytes=20000, align_records=False)
    bam_writer.write_bam(bams[1], batch2, block_bytes=30000, align_records=True)
    lens = dict(zip(batch.references, batch.lengths))
    fastas = []
    for name, longer in (('contigs.fa', ()), ('other.fa', doc['fasta_names'][3:15])):
        fastas.append(str(d / name))
        with open(fastas[-1], 'w') as fh:
            for n in doc['fasta_names']:
                fh.write('>%s\n%s\n' % (n, 'A' * (lens[n] + (1 if n in longer else 0))))
    return d, fastas, bams, (batch, batch2)


def test_cli_bam_report(cli_inputs, capsys):
    """--bam_report on a two-library run: the files of both passes parse back to the model's numbers, the census stands in
    Statistics.txt, no note is printed; without the flag the output directory is the same, byte for byte, less the report's
    files and lines (and the times)."""
    from besst_amd import bamio, cli, report
    d, fastas, bams, batches = cli_inputs
    argv = ['-c', fastas[0], '-f'] + bams + ['-orientation', 'fr', 'rf']
    assert cli.main(argv + ['-o', str(d / 'plain')]) == 0
    capsys.readouterr()
    assert cli.main(argv + ['-o', str(d / 'report'), '--bam_report']) == 0
    assert 'NOTE' not in capsys.readouterr().err
    plain, rep = _tree(str(d / 'plain' / 'BESST_output')), _tree(str(d / 'report' / 'BESST_output'))
    mine = set(os.path.join('pass%d' % n, f) for n in (1, 2) for f in report.FILES)
    assert set(rep) - set(plain) == mine and set(plain) <= set(rep)
    assert not any('report' in k or 'idxstats' in k or '_hist' in k or 'insert_sizes' in k for k in plain)
    for k in plain:
        if k != 'Statistics.txt':
            assert plain[k] == rep[k], k
    stats = _untimed(rep['Statistics.txt'])
    census = []
    for n, (bam, batch) in enumerate(zip(bams, batches)):
        host = bamio.read_bam(bam, threads=2)
        got = report.LibraryReport.read(str(d / 'report' / 'BESST_output' / ('pass%d' % (n + 1))))
        assert_words(got.words, M.words(host, len(host.references), 32768), 'pass %d' % (n + 1))
        assert got.references == list(host.references) and got.lengths == [int(x) for x in host.lengths]
        m = M.model(host, len(host.references))
        census += ['%d + %d %s' % (m['census'][r, 0], m['census'][r, 1], lab) for r, lab in enumerate(M.ROWS)]
    before = [l for l in _untimed(plain['Statistics.txt']) if l]
    assert [l for l in stats if l in set(census)] == census and not set(census) & set(before)
    assert [l for l in stats if l and l not in set(census) and not l.startswith('BAM report of ')] == before
    assert b'BAM report' not in plain['Statistics.txt'] and b'NOTE' not in rep['Statistics.txt']


def test_cli_notes(cli_inputs, capsys):
    """An fr library named rf, and a contig file in which twelve contigs are one base longer than the header says: both
    notes go to stderr and to Statistics.txt, and the run goes on to write its edge tables.  (-m and -s are given, as the
    reference's own message asks: without them a library named the wrong way round ends in get_metrics - "To few valid
    read alignments" - behind the note.)"""
    import re
    from besst_amd import cli
    d, fastas, bams, batches = cli_inputs
    capsys.readouterr()
    assert cli.main(['-c', fastas[1], '-f', bams[0], '-orientation', 'rf', '-m', '480', '-s', '55', '-o',
                     str(d / 'notes'), '--bam_report']) == 0
    err = capsys.readouterr().err
    stats = open(str(d / 'notes' / 'BESST_output' / 'Statistics.txt')).read()
    for text in (err, stats):
        assert 'named -orientation rf, but only 0 of the 14212 pairs' in text
        assert 'NOTE: 12 contig(s) have another length' in text
        names = re.findall(r'(\S+) \(\d+, header \d+\)', text.split('another contig file?): ')[1].split('\n')[0])
        doc, batch = GU.load('fr_infer')
        longer = [n for n in batch.references if n in doc['fasta_names'][3:15]]
        assert len(longer) == 12 and names == longer[:10]
    assert os.path.exists(str(d / 'notes' / 'BESST_output' / 'pass1' / 'edges_G.tsv'))
