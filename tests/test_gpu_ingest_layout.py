"""GPU: what a device ingest leaves beside the record columns - the mate-elsewhere and run planes and the candidate side
stream (set plane, offsets per 16 384-record block, entry columns), written while the chunks are decoded.

Two references, both applied to the columns the ingest left (ctx.fetch_records()): the numpy statement of the layout in
tests/test_candidate_stream.py, and the device makers (besst_dev_candidate_offsets / besst_dev_candidate_stream with both
planes).  Everything is compared with ==.  That the first build launches no maker is read from
besst_ctx_layout_state's launch counter; that its results do not change, from the same file read with
BESST_INGEST_LAYOUT=0 in the same process."""
import os
import struct

import numpy as np
import pytest

from tests import test_candidate_stream as M
from tests import test_gpu_candidate_stream as S
from tests.bam_writer import write_bam

pytestmark = pytest.mark.gpu

BLOCK = M.BLOCK
N_REFS = 300
N = 40000
F_PAIRED, F_UNMAPPED, F_REVERSE, F_READ1, F_READ2 = 0x1, 0x4, 0x10, 0x40, 0x80


# ---- the records ------------------------------------------------------------------------------------------------------
def library(n=N, seed=1, n_refs=N_REFS, share=0.3, qlen=(20, 40), first_tid=None, last_tid=None, names=None):
    """Coordinate-sorted records on a few hundred short contigs.  `share` of them have the mate elsewhere: mapped read 2
    (in the set), mapped read 1 with the mate inside the header (mate elsewhere, NOT in the set), unmapped read 1 (in it),
    mapped read 1 with mtid -1 or >= n_refs (in it)."""
    from besst_amd.records import RecordBatch
    rng = np.random.default_rng(seed)
    tid = np.sort(rng.integers(0, n_refs, n)).astype(np.int32)
    if first_tid is not None and n:
        tid[:3] = first_tid
    if last_tid is not None and n:
        tid[-3:] = last_tid
    kind = np.where(rng.random(n) < share, rng.integers(1, 6, n), 0)
    other = ((tid.astype(np.int64) + rng.integers(1, n_refs, n)) % n_refs).astype(np.int32)
    mtid = np.where(kind == 0, tid, other).astype(np.int32)
    flag = np.full(n, F_PAIRED | F_READ1, dtype=np.int64)
    flag[kind == 1] = F_PAIRED | F_READ2                                 # mapped read 2, mate elsewhere
    flag[kind == 2] = F_PAIRED | F_READ1                                 # mapped read 1, mate elsewhere inside the header
    flag[kind == 3] = F_PAIRED | F_READ1 | F_UNMAPPED                    # the unmapped-read-1 quirk
    mtid[kind == 4] = -1                                                 # mapped read 1, mate outside the header
    mtid[kind == 5] = n_refs + (np.arange(n)[kind == 5] % 3)
    flag[(kind == 0) & (rng.random(n) < 0.5)] = F_PAIRED | F_READ2       # read 2 with its mate on the same contig: not in the set
    flag |= np.where(rng.random(n) < 0.5, F_REVERSE, 0)
    q = rng.integers(qlen[0], qlen[1], n) if not callable(qlen) else qlen(n, rng)
    pos = rng.integers(0, 4000, n)
    refs = names or ['c%d' % i for i in range(n_refs)]
    return RecordBatch(refs, [5000] * n_refs, tid, mtid, pos, rng.integers(0, 4000, n), rng.integers(-500, 500, n),
                       flag.astype(np.uint16), rng.choice([0, 5, 11, 40, 60], n).astype(np.uint8), q.astype(np.uint16))


def clause_counts(rec, n_refs):
    t, m, f = rec['tid'].astype(np.int64), rec['mtid'].astype(np.int64), rec['flag'].astype(np.int64)
    away = t != m
    read2 = away & ((f & F_READ2) != 0) & ((f & F_UNMAPPED) == 0)
    quirk = away & ((f & F_UNMAPPED) != 0) & ((f & F_READ1) != 0)
    outside = away & ((f & F_READ1) != 0) & ((f & F_UNMAPPED) == 0) & ((m < 0) | (m >= n_refs))
    outside_set = away & ~M.in_set(t, m, f, n_refs)
    return int(read2.sum()), int(quirk.sum()), int(outside.sum()), int(outside_set.sum())


_FILES = {}


@pytest.fixture(scope='module')
def files(tmp_path_factory):
    """name -> path of a file written once for the module."""
    root = tmp_path_factory.mktemp('ingest_layout')

    def get(name, batch_of, **kw):
        if name not in _FILES:
            path = str(root / (name + '.bam'))
            batch = batch_of()
            write_bam(path, batch, **kw)
            _FILES[name] = (path, batch)
        return _FILES[name]
    return get


# ---- ingest, references --------------------------------------------------------------------------------------------------
def fresh_env(monkeypatch):
    monkeypatch.setenv('BESST_RECORD_PATH', '1')
    for k in ('BESST_MATE_BITS', 'BESST_TID_BITS', 'BESST_CAND_STREAM', 'BESST_INGEST_LAYOUT', 'BESST_INGEST_ENTRY_ROOM'):
        monkeypatch.delenv(k, raising=False)


def new_context(n_refs=N_REFS):
    from besst_amd import device
    ctx = device.GraphContext(0)
    zeros = np.zeros(n_refs, dtype=np.int32)
    ctx.set_contigs(scaf_id=zeros, scaf_len=zeros, ctg_pos=zeros, ctg_len=zeros, direction=zeros, cls=zeros)
    return ctx


def push_file(ctx, path, **kw):
    from besst_amd import _lib, bamio
    lib = _lib.load()
    handle, _, _ = bamio._open(lib, path, 2)
    try:
        stats = ctx.push_bam(handle, **kw)[0]
    finally:
        lib.besst_bam_close(handle)
    return stats


def planes_of(rec):
    n = len(rec['tid'])
    mate = np.packbits(rec['tid'] != rec['mtid'], bitorder='little')
    runs = np.packbits(np.r_[True, rec['tid'][1:] != rec['tid'][:-1]], bitorder='little') if n else np.zeros(0, np.uint8)
    return mate, runs


def assert_planes(ctx, rec):
    got = ctx.fetch_layout()
    mate, runs = planes_of(rec)
    assert np.array_equal(got['mate_bits'], mate), 'mate_bits'
    assert np.array_equal(got['tid_bits'], runs), 'tid_bits'
    return got


def assert_layout(ctx, n_refs=N_REFS, makers=True):
    """Planes and stream of the context == the numpy model and == the device makers, both on the columns it holds."""
    st = ctx.layout_state()
    n = st['n_records']
    assert st['bits_upto'] == n and st['tid_bits_upto'] == n and st['cs_upto'] == n, st
    rec = ctx.fetch_records()
    want = M.compact(rec, n_refs)
    assert (st['n_entries'], st['n_refs']) == (want['n_entries'], n_refs), st
    assert st['entry_capacity'] >= st['n_entries'] + 1 and st['entry_capacity'] % 64 == 0, st
    got = assert_planes(ctx, rec)
    S.assert_same_stream(got, want)
    if makers:
        dev = S.device_stream(rec, n_refs, with_bits=True)
        S.assert_same_stream(got, dev)
        assert np.array_equal(got['mate_bits'], dev['mate_bits']) and np.array_equal(got['tid_bits'], dev['tid_bits'])
    return rec, st


def real_table(n_refs=N_REFS):
    ids = np.arange(1, n_refs + 1, dtype=np.int32)
    full = np.full(n_refs, 5000, dtype=np.int32)
    return dict(scaf_id=ids, scaf_len=full, ctg_pos=np.zeros(n_refs, np.int32), ctg_len=full,
                direction=np.ones(n_refs, np.uint8), cls=np.ones(n_refs, np.uint8))


def build(ctx, table=None):
    ctx.set_contigs(**(table or real_table()))
    ctx.set_library(30.0, 3000.0, 11, 'fr', True, True, False)
    table, aligned, ctr = ctx.build_graph()
    return S._columns(table, aligned, ctr)


def assert_same_results(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)


def reference_results(path, monkeypatch, **kw):
    """The same file with the feature switched off, in this process: the build makes planes and stream from the columns."""
    monkeypatch.setenv('BESST_INGEST_LAYOUT', '0')
    with new_context() as ctx:
        push_file(ctx, path, mode='device', **kw)
        st = ctx.layout_state()
        assert (st['bits_upto'], st['tid_bits_upto'], st['cs_upto'], st['maker_launches']) == (0, 0, 0, 0), st
        out = build(ctx)
        assert ctx.layout_state()['maker_launches'] == 3 and S._form() == 3
    monkeypatch.delenv('BESST_INGEST_LAYOUT')
    return out


# ---- state and results -----------------------------------------------------------------------------------------------------
def test_first_build_finds_nothing_to_make(files, monkeypatch):
    """After the ingest, before any build: the three watermarks stand at n_records, no maker has been launched; the build
    with the fused loop launches none, runs the side-stream form, and gives what the switched-off ingest gives."""
    from besst_amd import bamio
    fresh_env(monkeypatch)
    path, batch = files('htslib_3000', library, block_bytes=3000, align_records=True)
    bam = bamio.ResidentBam(path, threads=2, mode='device', chunk_blocks=64)
    try:
        st = bam.layout_state()
        assert st['n_records'] == len(batch) == N
        assert (st['bits_upto'], st['tid_bits_upto'], st['cs_upto']) == (N, N, N), st
        assert st['maker_launches'] == 0
        rec, _ = assert_layout(bam.ctx)
        read2, quirk, outside, outside_set = clause_counts(rec, N_REFS)
        assert min(read2, quirk, outside, outside_set) > 500              # every clause, and mates elsewhere outside the set
        assert len(np.unique(rec['tid'])) > 200 and N > 2 * BLOCK
        got = build(bam.ctx)
        st = bam.layout_state()
        assert st['maker_launches'] == 0 and S._form() == 3, st
        assert (st['bits_upto'], st['tid_bits_upto'], st['cs_upto']) == (N, N, N), st
        assert_same_results(got, build(bam.ctx))                          # (a second build finds the same)
        assert bam.layout_state()['maker_launches'] == 0
    finally:
        bam.close()
    assert_same_results(got, reference_results(path, monkeypatch, chunk_blocks=64))


# ---- block layouts ---------------------------------------------------------------------------------------------------------
LAYOUTS = {
    # htslib's layout: every block begins with a record; many chunks, seams at odd record indices
    'htslib_700': (dict(block_bytes=700, align_records=True), 64),
    'htslib_3000': (dict(block_bytes=3000, align_records=True), 64),
    # records straddle blocks: a chunk's unfinished record travels as the next chunk's block 0; with 90-byte blocks many
    # blocks hold no record start, and the records in front of the two 16 384-record borders are long ones, so that such
    # blocks lie right in front of both borders (asserted below).  64 blocks a chunk is the smallest the ingest takes.
    'straddle_5000': (dict(block_bytes=5000, align_records=False), 64),
    'straddle_90': (dict(block_bytes=90, align_records=False), 64),
}


def long_before_the_borders():
    b = library()
    b.qlen[[BLOCK - 1, 2 * BLOCK - 1]] = 400
    return b


def record_starts(batch):
    """Offset of every record in the uncompressed BAM stream that tests.bam_writer.write_bam writes for `batch`."""
    header = 12 + len(b'@HD\tVN:1.0\tSO:coordinate\n') + sum(9 + len(r) for r in batch.references)
    q = batch.qlen.astype(np.int64)
    names = np.array([len('r%d' % i) + 1 for i in range(len(batch))])
    sizes = 4 + 32 + names + 4 * (q > 0) + (q + 1) // 2 + q
    return header + np.r_[0, np.cumsum(sizes)[:-1]]


@pytest.mark.parametrize('name', sorted(LAYOUTS))
def test_layouts(name, files, monkeypatch):
    fresh_env(monkeypatch)
    kw, chunk_blocks = LAYOUTS[name]
    path, batch = files(name, long_before_the_borders if name == 'straddle_90' else library, **kw)
    if name == 'straddle_90':
        starts = record_starts(batch)
        assert starts[-1] < os.path.getsize(path) * 50
        holds_a_start = np.zeros(starts[-1] // 90 + 1, dtype=bool)
        holds_a_start[starts // 90] = True
        assert (~holds_a_start).sum() > 1000                 # blocks no record begins in, everywhere ...
        for border in (BLOCK, 2 * BLOCK):                    # ... and at least three in a row right in front of each border's block
            at = starts[border] // 90
            assert not holds_a_start[at - 3:at].any()
    with new_context() as ctx:
        stats = push_file(ctx, path, mode='device', chunk_blocks=chunk_blocks)
        assert stats.on_device == 1 and stats.records == N and stats.chunks > 8
        assert ctx.layout_state()['maker_launches'] == 0
        rec, _ = assert_layout(ctx)
        for c in ('tid', 'mtid', 'flag', 'qlen'):
            assert np.array_equal(rec[c], getattr(batch, c)), c


def test_a_block_begins_on_a_multiple_of_32(files, monkeypatch):
    """Records of one size in htslib's layout (behind record 10 000, where the names 'r<i>' stop growing): every block holds
    the same number of records.  With 33 a block, the blocks' first records run through every position of a plane word,
    its first bit included - a block that begins exactly on a multiple of 32; with 32 every block begins at the same
    position, and every word is shared by the same two blocks."""
    fresh_env(monkeypatch)
    for per_block in (32, 33):
        one_size = lambda: library(n=2 * BLOCK + 100, seed=5, qlen=(30, 31))
        # a record: 4 + 32 + 7 (name) + 4 (one CIGAR op) + 15 + 30 = 92 bytes
        path, batch = files('same_%d' % per_block, one_size, block_bytes=per_block * 92 + 40, align_records=True)
        with new_context() as ctx:
            push_file(ctx, path, mode='device', chunk_blocks=64)
            assert_layout(ctx)


@pytest.mark.parametrize('n', [50, BLOCK, BLOCK + 1])
def test_short_files_and_the_block_border(n, files, monkeypatch):
    fresh_env(monkeypatch)
    path, _ = files('n_%d' % n, lambda: library(n=n, seed=n), block_bytes=3000, align_records=True)
    with new_context() as ctx:
        assert push_file(ctx, path, mode='device', chunk_blocks=64).records == n
        _, st = assert_layout(ctx)
        assert ctx.fetch_layout()['offsets'].shape[0] == (n + BLOCK - 1) // BLOCK + 1


def test_no_record_and_every_record_in_the_set(files, monkeypatch):
    fresh_env(monkeypatch)

    def none():
        b = library(n=BLOCK + 700, seed=8)
        b.mtid[:] = b.tid
        return b

    def every():
        b = library(n=BLOCK + 700, seed=9)
        b.mtid[:] = (b.tid + 1) % N_REFS
        b.flag[:] = F_PAIRED | F_READ2
        return b
    for name, make, count in (('none', none, 0), ('every', every, BLOCK + 700)):
        path, _ = files('set_' + name, make, block_bytes=5000, align_records=False)
        with new_context() as ctx:
            push_file(ctx, path, mode='device', chunk_blocks=64)
            _, st = assert_layout(ctx)
            assert st['n_entries'] == count


# ---- seams: a contig change exactly at a chunk's / a block's first record, and none there ------------------------------------
def test_run_bits_at_chunk_and_block_seams(files, monkeypatch):
    """Records of 88 to 91 bytes, 8 per block, 64 blocks per chunk at most: block b begins with record 8 b (behind the
    header's block), chunks begin at multiples of 8.  Over the first 2392 records a contig change lies ON every block's
    first record in one file - so on the first record of every chunk that begins there - and on no block's first record in
    the other (every run begins at 8 k + 3); the ingest's own chunk count says that there were seams to settle."""
    fresh_env(monkeypatch)
    n = 6000

    def at_seams(shift):
        def make():
            b = library(n=n, seed=11, qlen=(30, 31))
            b.tid[:] = np.minimum((np.arange(n) + 8 - shift) // 8, N_REFS - 1)       # runs of 8 records = one block's
            return b
        return make
    for shift in (0, 3):
        path, batch = files('seam_%d' % shift, at_seams(shift), block_bytes=8 * 92 + 40, align_records=True)
        with new_context() as ctx:
            stats = push_file(ctx, path, mode='device', chunk_blocks=64)
            assert stats.chunks >= 8
            rec, _ = assert_layout(ctx)
            starts = np.flatnonzero(np.r_[True, rec['tid'][1:] != rec['tid'][:-1]])
            assert len(starts) > 100 and np.all(starts[1:] % 8 == shift)


# ---- pushes ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('continues', [True, False])
def test_two_files_into_one_context(continues, files, monkeypatch):
    """The first file ends inside a 16 384-record block and inside a plane byte; the second file's first record continues
    the first file's last contig, or begins another."""
    fresh_env(monkeypatch)
    n1, n2 = BLOCK + 3003, BLOCK + 1501
    assert n1 % BLOCK and n1 % 8
    p1, _ = files('first', lambda: library(n=n1, seed=21, last_tid=N_REFS - 1), block_bytes=3000, align_records=True)
    p2, _ = files('second_%d' % continues, lambda: library(n=n2, seed=22, first_tid=N_REFS - 1 if continues else 0),
                  block_bytes=5000, align_records=False)
    with new_context() as ctx:
        push_file(ctx, p1, mode='device', chunk_blocks=64)
        assert_layout(ctx, makers=False)
        push_file(ctx, p2, mode='device', chunk_blocks=64)
        rec, st = assert_layout(ctx)
        assert st['n_records'] == n1 + n2 and st['maker_launches'] == 0
        assert (rec['tid'][n1] == rec['tid'][n1 - 1]) == continues
        got = build(ctx)
        assert ctx.layout_state()['maker_launches'] == 0 and S._form() == 3
    monkeypatch.setenv('BESST_INGEST_LAYOUT', '0')
    with new_context() as ctx:
        push_file(ctx, p1, mode='device', chunk_blocks=64)
        push_file(ctx, p2, mode='device', chunk_blocks=64)
        assert_same_results(got, build(ctx))


@pytest.mark.parametrize('second', ['host', 'records'])
def test_host_push_behind_a_device_push(second, files, monkeypatch):
    """The host forms leave the watermarks where they are: the build extends planes and stream from there (its launch
    counter rises) and gives what one push of everything gives."""
    fresh_env(monkeypatch)
    n1, n2 = BLOCK + 3003, 5000
    p1, b1 = files('first', lambda: library(n=n1, seed=21, last_tid=N_REFS - 1), block_bytes=3000, align_records=True)
    p2, b2 = files('tail_host', lambda: library(n=n2, seed=23), block_bytes=3000, align_records=True)
    with new_context() as ctx:
        push_file(ctx, p1, mode='device', chunk_blocks=64)
        if second == 'host':
            assert push_file(ctx, p2, mode='host').on_device == 0
        else:
            ctx.push_records(b2)
        st = ctx.layout_state()
        assert st['n_records'] == n1 + n2 and (st['bits_upto'], st['tid_bits_upto'], st['cs_upto']) == (n1, n1, n1), st
        got = build(ctx)
        st = ctx.layout_state()
        assert st['maker_launches'] == 3 and S._form() == 3, st
        assert_layout(ctx)
    with new_context() as ctx:
        from besst_amd.records import RecordBatch
        ctx.push_records(RecordBatch.concatenate([b1, b2]))
        assert_same_results(got, build(ctx))


# ---- growth, overflow, failure ---------------------------------------------------------------------------------------------------
def test_columns_grow_under_the_ingest(files, monkeypatch):
    """The first fifth of the file holds long reads: the record reservation made from the first chunk is too small, the
    columns grow under the ingest, and planes, offsets and entry columns move with them.  The entry columns start with
    room for ROOM entries (the knob) and can only have more after being carved anew where the columns grew."""
    fresh_env(monkeypatch)
    room = 12000
    def long_then_short():
        b = library(qlen=lambda n, rng: np.where(np.arange(n) < n // 5, 600, 25), seed=31)
        for col, v in (('pos', 7), ('mpos', 9), ('tlen', 0), ('mapq', 60)):     # the short records deflate to a fraction of the long
            getattr(b, col)[N // 5:] = v                                      # ones' bytes: far more records per byte than the first chunk saw
        return b
    path, _ = files('long_then_short', long_then_short, block_bytes=3000, align_records=True)
    monkeypatch.setenv('BESST_INGEST_ENTRY_ROOM', str(room))
    with new_context() as ctx:
        push_file(ctx, path, mode='device', chunk_blocks=64)
        _, st = assert_layout(ctx)
        assert st['n_entries'] < room                                      # (the first carving would have held them all)
        assert st['entry_capacity'] > (room + 1 + 63) // 64 * 64, st


def test_entries_that_do_not_fit(files, monkeypatch):
    """Room for a few hundred entries: cs_upto stays where it was - the only case in which it may lie below n_records -,
    the planes are handed over, the build makes the stream (two launches) and gives the same results."""
    fresh_env(monkeypatch)
    path, _ = files('htslib_3000', library, block_bytes=3000, align_records=True)
    monkeypatch.setenv('BESST_INGEST_ENTRY_ROOM', '300')
    with new_context() as ctx:
        push_file(ctx, path, mode='device', chunk_blocks=256)
        st = ctx.layout_state()
        assert (st['bits_upto'], st['tid_bits_upto'], st['cs_upto'], st['maker_launches']) == (N, N, 0, 0), st
        assert_planes(ctx, ctx.fetch_records())
        got = build(ctx)
        st = ctx.layout_state()
        assert st['maker_launches'] == 2 and st['cs_upto'] == N and S._form() == 3, st
        assert_layout(ctx)
    monkeypatch.delenv('BESST_INGEST_ENTRY_ROOM')
    assert_same_results(got, reference_results(path, monkeypatch, chunk_blocks=256))


def test_entries_that_do_not_fit_behind_a_resident_stream(files, monkeypatch):
    """The same on a context that holds a valid stream whose last record lies inside a 16 384-record block: the resident
    stream stays exactly what it was - its last offset too, which the second file's records had written over."""
    fresh_env(monkeypatch)
    n1 = BLOCK + 3003
    p1, b1 = files('first', lambda: library(n=n1, seed=21, last_tid=N_REFS - 1), block_bytes=3000, align_records=True)
    p2, _ = files('htslib_3000', library, block_bytes=3000, align_records=True)
    with new_context() as ctx:
        push_file(ctx, p1, mode='device', chunk_blocks=64)
        before = ctx.fetch_layout()
        entries = ctx.layout_state()['n_entries']
        monkeypatch.setenv('BESST_INGEST_ENTRY_ROOM', '300')
        push_file(ctx, p2, mode='device', chunk_blocks=64)
        st = ctx.layout_state()
        assert (st['n_records'], st['bits_upto'], st['tid_bits_upto'], st['cs_upto'], st['n_entries']) == (n1 + N, n1 + N, n1 + N, n1, entries), st
        after = ctx.fetch_layout()
        S.assert_same_stream(after, before)
        S.assert_same_stream(after, M.compact({k: v[:n1] for k, v in ctx.fetch_records().items()}, N_REFS))
        assert_planes(ctx, ctx.fetch_records())
        got = build(ctx)
        assert ctx.layout_state()['maker_launches'] == 2 and S._form() == 3
        assert_layout(ctx)
    monkeypatch.setenv('BESST_INGEST_LAYOUT', '0')
    with new_context() as ctx:
        push_file(ctx, p1, mode='device', chunk_blocks=64)
        push_file(ctx, p2, mode='device', chunk_blocks=64)
        assert_same_results(got, build(ctx))


def bgzf_blocks(raw):
    out, at = [], 0
    while at < len(raw):
        size = struct.unpack_from('<H', raw, at + 16)[0] + 1
        out.append((at, size))
        at += size
    return out


def test_a_damaged_block_leaves_nothing_behind(files, tmp_path, monkeypatch):
    """One payload byte of a late block is damaged: the call fails as it does today, the state does not move, and a good
    file pushed afterwards gets exact planes - the bits the failed call had ORed in behind the watermark are gone."""
    from besst_amd import _lib
    fresh_env(monkeypatch)
    p1, _ = files('first', lambda: library(n=BLOCK + 3003, seed=21, last_tid=N_REFS - 1), block_bytes=3000, align_records=True)
    good, _ = files('htslib_3000', library, block_bytes=3000, align_records=True)
    raw = bytearray(open(good, 'rb').read())
    blocks = bgzf_blocks(raw)
    at, size = blocks[len(blocks) * 3 // 4]
    raw[at + 18 + (size - 26) // 2] ^= 0x5a
    bad = str(tmp_path / 'damaged.bam')
    with open(bad, 'wb') as fh:
        fh.write(raw)
    with new_context() as ctx:
        push_file(ctx, p1, mode='device', chunk_blocks=64)
        before = ctx.layout_state()
        with pytest.raises(_lib.BesstDeviceError):
            push_file(ctx, bad, mode='device', chunk_blocks=64)
        assert ctx.layout_state() == before
        assert_layout(ctx, makers=False)
        push_file(ctx, good, mode='device', chunk_blocks=64)
        _, st = assert_layout(ctx)
        assert st['n_records'] == before['n_records'] + N and st['maker_launches'] == 0


# ---- another header, slices ---------------------------------------------------------------------------------------------------
def test_a_table_of_another_size_makes_the_stream_anew(files, monkeypatch):
    """The ingest's stream is made for the file's reference count; a contig table with eight rows fewer makes the build drop
    it and make its own - equal to what the switched-off ingest and the same table give."""
    fresh_env(monkeypatch)
    def low_tids():
        b = library(seed=41)
        b.tid[:] = np.minimum(b.tid, N_REFS - 9)             # every record lies on a contig of the shorter table; mates need not
        return b
    path, _ = files('low_tids', low_tids, block_bytes=3000, align_records=True)
    short = {k: v[:N_REFS - 8] for k, v in real_table().items()}
    with new_context() as ctx:
        push_file(ctx, path, mode='device', chunk_blocks=64)
        got = build(ctx, short)
        st = ctx.layout_state()
        assert st['maker_launches'] == 2 and st['n_refs'] == N_REFS - 8 and S._form() == 3, st
        assert_layout(ctx, n_refs=N_REFS - 8)
    monkeypatch.setenv('BESST_INGEST_LAYOUT', '0')
    with new_context() as ctx:
        push_file(ctx, path, mode='device', chunk_blocks=64)
        assert_same_results(got, build(ctx, short))


def test_a_header_of_another_size_against_the_oracle(files, monkeypatch):
    """As tests/test_gpu_candidate_stream.py::test_context_makes_the_stream_anew_for_another_contig_count, from a file: the
    file's header names eight references more than the contig table has rows, so the ingest's stream - made for the
    header's count - is dropped by the build, which makes its own; edge table, coverage and counters equal both oracles'."""
    from besst_amd.records import RecordBatch
    from tests import test_gpu_record_borders as T
    from tests import test_gpu_tid_bits as TB
    from tests.record_design import N_CONTIGS
    fresh_env(monkeypatch)
    name = TB.register(S.stream_with_far_mates(2 * BLOCK + 2500))
    s, batch, wl, _ = T.oracle(name)
    assert len(batch.references) == N_CONTIGS

    def wider_header():
        cols = {k: getattr(batch, k) for k in ('tid', 'mtid', 'pos', 'mpos', 'tlen', 'flag', 'mapq', 'qlen')}
        return RecordBatch(list(batch.references) + ['extra%d' % i for i in range(8)], list(batch.lengths) + [1000] * 8, **cols)
    path, _ = files('wider_header', wider_header, block_bytes=3000, align_records=True)
    with new_context(N_CONTIGS + 8) as ctx:
        push_file(ctx, path, mode='device', chunk_blocks=64)
        rec, st = assert_layout(ctx, n_refs=N_CONTIGS + 8, makers=False)
        for c in ('tid', 'mtid', 'pos', 'mpos', 'tlen', 'flag', 'mapq', 'qlen'):
            assert np.array_equal(rec[c], getattr(batch, c)), c
        ctx.set_contigs(**wl['table'])
        S._set_library(ctx, s.lib)
        T.check(name, *ctx.build_graph())
        st = ctx.layout_state()
        assert st['maker_launches'] == 2 and st['n_refs'] == N_CONTIGS and S._form() == 3, st


@pytest.mark.parametrize('world', [2, 3])
def test_slices_of_a_straddling_file(world, files, monkeypatch):
    from besst_amd import distributed
    fresh_env(monkeypatch)
    path, batch = files('straddle_5000', library, block_bytes=5000, align_records=False)
    slices, _ = distributed.ingest_all_slices(path, world, device_index=0, threads=2, chunk_blocks=64)
    try:
        assert sum(len(b) for b, _ in slices) == N
        for bam, _ in slices:
            assert len(bam) > 0 and bam.layout_state()['maker_launches'] == 0
            assert_layout(bam.ctx)
    finally:
        for bam, _ in slices:
            bam.close()
