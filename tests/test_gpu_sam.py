"""GPU: SAM text parsed on the device (csrc/sam.hip, bamio.ResidentSam) == the tests' own decoder (tests/sam_model.py), and
== the BAM of the same records.  The shapes are the smallest at which the passes can go wrong: the hand-written fixture in
every container, the designed border file of tests/sam_design.py at the smallest and the largest tile, chunks of 4 KiB, a
reference table of 70 000 names, every error class in the middle of a file."""
import gzip
import json
import os
import warnings

import numpy as np
import pytest

from tests import bgzf_writer, sam_design, sam_model

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
SAM = os.path.join(HERE, 'golden', 'sam', 'handmade.sam')
BAM = os.path.join(HERE, 'golden', 'bam', 'handmade_a.bam')
JSON = os.path.join(HERE, 'golden', 'bam', 'handmade_bam.json')
COLS = ('tid', 'mtid', 'pos', 'mpos', 'tlen', 'flag', 'mapq', 'qlen')


def put(tmp_path, name, data):
    path = str(tmp_path / name)
    with open(path, 'wb') as fh:
        fh.write(data)
    return path


def assert_is_model(sam, model, what=''):
    """the resident columns and the head arrays of an open ResidentSam against the model's decode of the same bytes"""
    n = len(model['tid'])
    assert len(sam) == n and sam.ingest.records == n and sam.ingest.on_device == 1, what
    got = sam.ctx.fetch_records()
    for k in COLS:
        assert np.array_equal(got[k], model[k]), (what, k, np.flatnonzero(got[k] != model[k])[:5])
    k = min(n, 1000)
    assert np.array_equal(sam.rlen, model['rlen'][:k]) and np.array_equal(sam.alen, model['alen'][:k]), what
    assert np.array_equal(sam.qlen, model['qlen'][:k]), what
    assert sam.references == model['references'] and list(sam.lengths) == model['lengths'], what


# ---- 4. the hand-written fixture, in every container ------------------------------------------------------------------------
@pytest.fixture(scope='module')
def handmade():
    from besst_amd import bamio
    with open(SAM, 'rb') as fh:
        data = fh.read()
    with open(JSON) as fh:
        doc = json.load(fh)
    bam = bamio.ResidentBam(BAM, mode='device')
    ref = dict(cols=bam.ctx.fetch_records(), rlen=bam.rlen.copy(), alen=bam.alen.copy(), qlen=bam.qlen.copy(),
               words=bam.report().words.copy(), references=list(bam.references), lengths=list(bam.lengths))
    bam.close()
    return data, doc, ref


FORMS = ['plain', 'crlf', 'no_final_newline', 'bgzf', 'bgzf_small_blocks', 'gzip', 'gzip_on_gpu']


@pytest.mark.parametrize('form', FORMS)
def test_handmade_sam_is_the_handmade_bam(handmade, form, tmp_path):
    from besst_amd import bamio
    data, doc, ref = handmade
    kw = {}
    if form == 'crlf':
        data = data.replace(b'\n', b'\r\n')
    elif form == 'no_final_newline':
        data = data[:-1]
    elif form == 'bgzf':
        data = bgzf_writer.bgzf(data)
    elif form == 'bgzf_small_blocks':
        data = bgzf_writer.bgzf(data, payload=97, empty_at=(0, 3))       # the header and every record straddle blocks
    elif form in ('gzip', 'gzip_on_gpu'):
        data = gzip.compress(data)
        kw = dict(gzip_on_gpu=form == 'gzip_on_gpu')
    path = put(tmp_path, 'handmade.' + form, data)
    assert bamio.reader_class(path) is bamio.ResidentSam
    sam = bamio.open_bam(path, **kw)
    try:
        assert isinstance(sam, bamio.ResidentSam) and len(sam) == 15
        got = sam.ctx.fetch_records()
        for i, want in enumerate(doc['records']):
            for k in COLS:
                assert int(got[k][i]) == want[k], (want['name'], k)
            assert (int(sam.rlen[i]), int(sam.alen[i]), int(sam.qlen[i])) == (want['rlen'], want['alen'], want['qlen']), want['name']
        for k in COLS:
            assert np.array_equal(got[k], ref['cols'][k]) and got[k].dtype == ref['cols'][k].dtype, k
        assert np.array_equal(sam.rlen, ref['rlen']) and np.array_equal(sam.alen, ref['alen']) and np.array_equal(sam.qlen, ref['qlen'])
        assert sam.references == ref['references'] and list(sam.lengths) == ref['lengths']
        assert np.array_equal(sam.report().words, ref['words'])          # every word, the digest included
        st = sam.layout_state()
        assert (st['n_records'], st['bits_upto'], st['tid_bits_upto'], st['cs_upto']) == (15, 0, 0, 0)
        want_path = dict(bgzf='device', bgzf_small_blocks='device', gzip='host', gzip_on_gpu='device_gzip').get(form)
        assert sam.inflate == want_path, (form, sam.inflate, sam.inflate_stats)
    finally:
        sam.close()


# ---- 5. tile borders ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def border():
    data, head = sam_design.border_file(tile=1024, long_lines=True)
    sam_design.cases_present(data, head, tile=1024, long_lines=True)
    return data, sam_model.decode(data)


@pytest.mark.parametrize('tile', [1024, 65536, None])
def test_tile_borders(border, tile, tmp_path):
    from besst_amd import bamio
    data, model = border
    assert model['saturated'] == 1 and len(model['tid']) == 1200
    path = put(tmp_path, 'border.sam', data)
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter('always')
        sam = bamio.ResidentSam(path, tile_bytes=tile)
    try:
        assert_is_model(sam, model, 'tile %s' % tile)
        assert sam.ingest.chunks == 1 and sam.ingest.bytes_h2d == len(data) - model['header_bytes']
        assert [str(w.message) for w in caught if '65535' in str(w.message)] == [
            '%s: 1 record(s) align more than 65535 query bases; their qlen is stored as 65535' % path]
    finally:
        sam.close()


def test_tile_borders_in_a_bgzf_file(border, tmp_path):
    """the same text behind a header whose length is no multiple of 16: the records are moved down over it"""
    from besst_amd import bamio
    data, model = border
    assert model['header_bytes'] % 16
    path = put(tmp_path, 'border.sam.gz', bgzf_writer.bgzf(data))
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        sam = bamio.ResidentSam(path, tile_bytes=1024)
    try:
        assert_is_model(sam, model)
        assert sam.inflate == 'device' and sam.ingest.inflated_bytes == len(data)
    finally:
        sam.close()


# ---- 6. chunk borders ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def chunked():
    data, head = sam_design.border_file(tile=1024, chunk=4096, long_lines=False)
    plan = sam_design.cases_present(data, head, tile=1024, chunk=4096, long_lines=False)
    return data, sam_model.decode(data), plan


def test_chunk_borders(chunked, tmp_path):
    from besst_amd import bamio
    data, model, plan = chunked
    offsets = np.asarray(model['offsets']) - model['header_bytes']
    assert sum(1 for at, _, _ in plan if at <= offsets[999]) > 60        # the head arrays fill across that many chunks
    path = put(tmp_path, 'chunks.sam', data)
    one = bamio.ResidentSam(path, tile_bytes=1024)
    try:
        assert_is_model(one, model, 'one chunk')
        whole = one.ctx.fetch_records()
        assert one.ingest.chunks == 1
    finally:
        one.close()
    many = bamio.ResidentSam(path, chunk_bytes=4096, tile_bytes=1024)
    try:
        assert many.ingest.chunks == len(plan) and len(plan) > 100
        assert many.ingest.bytes_h2d == sum(n for _, n, _ in plan) == len(data) - model['header_bytes']
        assert_is_model(many, model, 'chunks of 4096')
        got = many.ctx.fetch_records()
        for k in COLS:
            assert np.array_equal(got[k], whole[k]), k
    finally:
        many.close()


def test_a_line_longer_than_the_chunk(border, tmp_path):
    from besst_amd import bamio
    data, model = border
    path = put(tmp_path, 'border.sam', data)
    first_long = next(at for at, nxt in zip(model['offsets'], model['offsets'][1:] + [len(data)]) if nxt - at > 4096)
    with pytest.raises(bamio.SamError) as err:
        bamio.ResidentSam(path, chunk_bytes=4096, tile_bytes=1024)
    assert err.value.offset - model['header_bytes'] >= 0
    # the offset is the line's first byte, counted in the file
    assert err.value.offset == first_long and 'chunk_bytes' in str(err.value)


# ---- 7. the reference table on the device ------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def big_table():
    names, absent = sam_design.reference_names(70000)
    rng = np.random.RandomState(11)
    head = ''.join('@SQ\tSN:%s\tLN:%d\n' % (n, 1000 + i % 977) for i, n in enumerate(names))
    special = [names.index(x) for x in ('ctg1', 'ctg10', 'ctg100', 'scaffold_0000A', 'scaffold_0000B', 'c', 'N' * 200,
                                        'N' * 199 + 'M', 'ctg')]
    lines = []
    for i in range(5000):
        tid = -1 if i % 11 == 5 else (special[i % len(special)] if i % 7 == 0 else int(rng.randint(0, len(names))))
        pick = i % 5
        rnext = '=' if pick == 0 else ('*' if pick == 1 else names[special[(i // 5) % len(special)] if pick == 2 else
                                                                  int(rng.randint(0, len(names)))])
        lines.append('r%d\t%d\t%s\t%d\t%d\t50M\t%s\t%d\t%d\t*\t*' % (i, i % 4096, '*' if tid < 0 else names[tid], i + 1, i % 61,
                                                                     rnext, 2 * i + 1, i - 2500))
    return head, lines, absent


def test_reference_lookup(big_table, tmp_path):
    from besst_amd import bamio
    head, lines, _ = big_table
    data = (head + '\n'.join(lines) + '\n').encode()
    model = sam_model.decode(data)
    assert len(set(model['tid'].tolist())) > 3000 and (model['tid'] == -1).any() and (model['mtid'] == -1).any()
    sam = bamio.ResidentSam(put(tmp_path, 'table.sam', data), tile_bytes=1024)
    try:
        assert_is_model(sam, model)
    finally:
        sam.close()


def test_unknown_names_and_the_smallest_offset(big_table, tmp_path):
    from besst_amd import bamio
    head, lines, absent = big_table
    bad = list(lines)
    f = bad[4100].split('\t')
    f[6] = absent[0]                                             # RNEXT unknown, far behind ...
    bad[4100] = '\t'.join(f)
    f = bad[1234].split('\t')
    f[2] = absent[3]                                             # ... an RNAME that is a present name's prefix
    bad[1234] = '\t'.join(f)
    data = (head + '\n'.join(bad) + '\n').encode()
    with pytest.raises(sam_model.SamModelError) as want:
        sam_model.decode(data)
    assert want.value.code == 9
    with pytest.raises(bamio.SamError) as err:
        bamio.ResidentSam(put(tmp_path, 'unknown.sam', data), tile_bytes=1024)
    assert (err.value.offset, err.value.line, err.value.reason) == (want.value.offset, want.value.line, bamio.SAM_REASONS[9])
    assert data[err.value.offset:].startswith(b'r1234\t')
    # in chunks the first bad line still wins: the chunk that holds it is the first to fail
    with pytest.raises(bamio.SamError) as err:
        bamio.ResidentSam(put(tmp_path, 'unknown.sam', data), tile_bytes=1024, chunk_bytes=8192)
    assert (err.value.offset, err.value.line) == (want.value.offset, want.value.line)


# ---- 8. every error class, in the middle of a file ---------------------------------------------------------------------------
@pytest.mark.parametrize('case', sam_design.ERROR_LINES, ids=lambda c: c[0])
def test_error_in_the_middle_of_a_file(case, tmp_path):
    from besst_amd import bamio
    _, bad, code = case
    good = [sam_design.GOOD_LINE.replace('read', 'read%d' % i, 1) for i in range(300)]
    lines = good[:150] + [bad] + good[150:250] + [bad] + good[250:]
    data = sam_design.header_bytes() + ('\n'.join(lines) + '\n').encode()
    with pytest.raises(sam_model.SamModelError) as want:
        sam_model.decode(data)
    assert want.value.code == code
    path = put(tmp_path, 'bad.sam', data)
    with pytest.raises(bamio.SamError) as err:
        bamio.ResidentSam(path, tile_bytes=1024)
    assert (err.value.offset, err.value.line, err.value.reason) == (want.value.offset, want.value.line, bamio.SAM_REASONS[code])
    assert isinstance(err.value, ValueError) and str(want.value.offset) in str(err.value)
    # the same through a compressed file: the offset counts the inflated text and the message says so
    with pytest.raises(bamio.SamError) as err:
        bamio.ResidentSam(put(tmp_path, 'bad.sam.gz', bgzf_writer.bgzf(data)), tile_bytes=1024)
    assert (err.value.offset, err.value.line) == (want.value.offset, want.value.line) and 'inflated' in str(err.value)
    # a second, good file opens in the same process
    ok = bamio.ResidentSam(put(tmp_path, 'good.sam', sam_design.header_bytes() + ('\n'.join(good) + '\n').encode()), tile_bytes=1024)
    try:
        assert len(ok) == 300
    finally:
        ok.close()


def short_lines_case():
    """Good lines, then three lines that cannot be read and lie inside ONE 16-byte lane slice - 'short\\tline', an empty
    line, 'ab' -, then good lines again -> (bytes, offset of the first bad line).  A record that can be read is 21 bytes at
    least, so a line inside one slice is always such a line; that the three are where they are said to be is asserted
    from the offsets."""
    front = ('\n'.join(sam_design.GOOD_LINE for _ in range(48)) + '\n').encode()
    bad = b'short\tline\n' + b'\n' + b'ab\n'
    assert len(front) % 16 == 0 and len(bad) <= 16
    data = front + bad + front
    at = len(front)
    starts = [at, at + 11, at + 12]
    for a, text in zip(starts, (b'short\tline\n', b'\n', b'ab\n')):
        assert data[a:a + len(text)] == text and data[a - 1:a] == b'\n'
        assert a // 16 == (a + len(text) - 1) // 16 == at // 16          # begins and ends inside the one slice
    return data, at


def test_a_failed_chunk_leaves_the_context_without_its_records(tmp_path):
    """the C ABI below ResidentSam: a chunk with a bad line is not appended, clear_records leaves nothing behind, and the
    context takes a good chunk afterwards.  The bad lines are short_lines_case's: three line starts in one lane slice."""
    import torch
    from besst_amd import _lib, device
    lib = _lib.load()
    good = ('\n'.join(sam_design.GOOD_LINE for _ in range(40)) + '\n').encode()
    bad, bad_at = short_lines_case()
    ctx = device.GraphContext(0)
    try:
        blob = np.frombuffer(b'ctg1', dtype=np.uint8)
        _lib.check(lib.besst_ctx_set_sam_references(ctx._ctx, _lib.ptr(blob), _lib.ptr(np.array([0, 4], dtype=np.int64)), 1), 'refs')
        head = [np.zeros(8, dtype=np.int32), np.zeros(8, dtype=np.int32), np.zeros(8, dtype=np.uint16)]

        def push(data, file_offset):
            text = torch.zeros(len(data) + 64, dtype=torch.uint8, device='cuda')
            text[:len(data)] = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
            torch.cuda.synchronize()
            info = np.zeros(4, dtype=np.int64)
            _lib.check(lib.besst_ctx_push_sam_text(ctx._ctx, None, text.data_ptr(), len(data), file_offset, 1024, 8, _lib.ptr(head[0]),
                                                   _lib.ptr(head[1]), _lib.ptr(head[2]), _lib.ptr(info)), 'push')
            return info.tolist()
        assert push(good, 0) == [40, 0, -1, 0]
        assert ctx.layout_state()['n_records'] == 40
        # 48 + 3 + 48 lines, every one with its own row; 'short\tline' (fewer than eleven fields) comes first
        assert push(bad, 1000) == [99, 0, 1000 + bad_at, 1]
        assert ctx.layout_state()['n_records'] == 40
        # the empty line alone in front of the others: its own offset and reason
        assert push(bad[:bad_at] + b'\n' + bad[bad_at:], 0) == [100, 0, bad_at, 2]
        ctx.clear_records()
        assert ctx.layout_state()['n_records'] == 0
        assert push(good, 0) == [40, 0, -1, 0]
        got = ctx.fetch_records()
        assert got['pos'].tolist() == [100] * 40 and got['tid'].tolist() == [0] * 40 and got['mtid'].tolist() == [0] * 40
        assert head[0].tolist() == [4] * 8 and head[1].tolist() == [100] * 8 and head[2].tolist() == [4] * 8
    finally:
        ctx.close()


def test_short_lines_through_the_reader(tmp_path):
    from besst_amd import bamio
    body, bad_at = short_lines_case()
    head = sam_design.header_bytes()
    with pytest.raises(bamio.SamError) as err:
        bamio.ResidentSam(put(tmp_path, 'short.sam', head + body), tile_bytes=1024)
    assert (err.value.offset, err.value.line, err.value.reason) == (len(head) + bad_at, head.count(b'\n') + 49, bamio.SAM_REASONS[1])


def test_columns_grow_once_when_the_text_is_announced():
    """besst_ctx_sam_expect_text: ten chunks of one announced text leave the columns where the first chunk put them;
    without the announcement they double, a few times"""
    import ctypes as C
    import torch
    from besst_amd import _lib, device
    lib = _lib.load()
    good = ('\n'.join(sam_design.GOOD_LINE for _ in range(400)) + '\n').encode()
    text = torch.zeros(len(good) + 64, dtype=torch.uint8, device='cuda')
    text[:len(good)] = torch.frombuffer(bytearray(good), dtype=torch.uint8).cuda()
    torch.cuda.synchronize()
    for announced, most in ((10 * len(good), 0), (0, 5)):      # (doubling: 400 -> 4000 records in four or five steps)
        ctx = device.GraphContext(0)
        try:
            blob = np.frombuffer(b'ctg1', dtype=np.uint8)
            _lib.check(lib.besst_ctx_set_sam_references(ctx._ctx, _lib.ptr(blob), _lib.ptr(np.array([0, 4], dtype=np.int64)), 1), 'refs')
            _lib.check(lib.besst_ctx_sam_expect_text(ctx._ctx, announced), 'expect')
            info, seen = np.zeros(4, dtype=np.int64), []
            for k in range(10):
                _lib.check(lib.besst_ctx_push_sam_text(ctx._ctx, None, text.data_ptr(), len(good), k * len(good), 1024, 0, None, None,
                                                       None, _lib.ptr(info)), 'push')
                assert info.tolist() == [400, 0, -1, 0]
                n, ptrs = C.c_int64(0), np.zeros(8, dtype=np.uint64)
                _lib.check(lib.besst_ctx_record_pointers(ctx._ctx, C.byref(n), _lib.ptr(ptrs)), 'pointers')
                assert n.value == 400 * (k + 1)
                seen.append(tuple(ptrs.tolist()))
            moves = sum(1 for a, b in zip(seen, seen[1:]) if a != b)
            assert moves <= most, (announced, moves)
            got = ctx.fetch_records()
            assert got['pos'].tolist() == [100] * 4000 and got['flag'].tolist() == [99] * 4000
        finally:
            ctx.close()


def test_damaged_compressed_data_names_the_compressed_offset(tmp_path):
    from besst_amd import bamio
    with open(SAM, 'rb') as fh:
        data = bgzf_writer.bgzf(fh.read(), payload=700)
    bad, at = bgzf_writer.damaged(data, 2, 'crc')
    assert at > 0
    with pytest.raises(bamio.SamError) as err:
        bamio.ResidentSam(put(tmp_path, 'damaged.sam.gz', bad))
    assert (err.value.offset, err.value.reason, err.value.line) == (at, 'compressed data', None)
    assert 'compressed SAM file' in str(err.value) and 'FASTA' not in str(err.value) and 'not of the inflated text' in str(err.value)
