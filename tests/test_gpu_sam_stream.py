"""GPU: a compressed SAM streamed chunk by chunk (bamio.ResidentSam: BGZF inflated and cut on the device, other gzip by zlib on
the host) == the tests' own decoder (tests/sam_model.py), round for round what tests/sam_stream_model.py predicts; the line
cutter (besst_dev_sam_lines) == the model's on its borders and on 3 MiB of sparse newlines; a file of more than 4 GiB of text;
and the text is not resident."""
import ctypes as C
import gzip
import os

import numpy as np
import pytest

from tests import bam_report_model, bgzf_writer, sam_design, sam_model, sam_stream_design, sam_stream_model
from tests.bgzf_util import EOF

pytestmark = pytest.mark.gpu

COLS = ('tid', 'mtid', 'pos', 'mpos', 'tlen', 'flag', 'mapq', 'qlen')
CHUNK, TILE = sam_stream_design.CHUNK, sam_stream_design.TILE


def put(tmp_path, name, data):
    path = str(tmp_path / name)
    with open(path, 'wb') as fh:
        fh.write(data)
    return path


def assert_is_model(sam, model, words=None, what=''):
    n = len(model['tid'])
    assert len(sam) == n and sam.ingest.records == n and sam.ingest.on_device == 1, what
    got = sam.ctx.fetch_records()
    for k in COLS:
        assert np.array_equal(got[k], model[k]), (what, k, np.flatnonzero(got[k] != model[k])[:5])
    k = min(n, 1000)
    assert np.array_equal(sam.rlen, model['rlen'][:k]) and np.array_equal(sam.alen, model['alen'][:k]), what
    assert np.array_equal(sam.qlen, model['qlen'][:k]), what
    assert sam.references == model['references'] and list(sam.lengths) == model['lengths'], what
    if words is not None:
        assert np.array_equal(sam.report().words, words), what


# ---- 1. the line cutter ------------------------------------------------------------------------------------------------------
def dev_cut(text, n, want, upto):
    """besst_dev_sam_lines over the first n bytes of ``text`` (the bytes behind n are on the device too) -> out"""
    import torch
    from besst_amd import _lib
    lib = _lib.load()
    room = (len(text) + 15) // 16 * 16 + 16
    buf = torch.full((room,), 0xff, dtype=torch.uint8, device='cuda')
    if text:
        buf[:len(text)] = torch.frombuffer(bytearray(text), dtype=torch.uint8).cuda()
    out = torch.full((4,), 7, dtype=torch.int64, device='cuda')
    torch.cuda.synchronize()
    _lib.check(lib.besst_dev_sam_lines(None, C.c_void_p(buf.data_ptr()), n, want, upto, C.c_void_p(out.data_ptr())), 'sam_lines')
    torch.cuda.synchronize()
    return out.cpu().tolist()


def test_the_cutter_on_its_borders():
    for name, text, queries in sam_stream_design.cutter_cases():
        for n, want, upto in queries:
            assert dev_cut(text, n, want, upto) == sam_stream_model.cutter(text[:n], bool(want), upto), (name, n, want, upto)


def test_the_cutter_on_three_mib_of_sparse_newlines():
    rng = np.random.RandomState(11)
    n = (3 << 20) + 5                                            # more than one wave's run of rounds, no multiple of 16
    raw = rng.randint(32, 127, size=n).astype(np.uint8)
    raw[raw == 64] = 65
    where = np.sort(rng.choice(n, size=40, replace=False))
    raw[where] = 10
    raw[0] = 64
    raw[where[:25] + 1] = 64                                     # 25 header lines, then a record line
    text = raw.tobytes()
    for want, upto in ((1, 0), (1, int(where[30]) + 1), (0, n), (1, n // 2)):
        assert dev_cut(text, n, want, upto) == sam_stream_model.cutter(text, bool(want), upto), (want, upto)
    head = text[:int(where[20]) + 1]                             # header lines alone, the last one whole / cut
    assert dev_cut(text, len(head), 1, 0) == sam_stream_model.cutter(head, True, 0) == [len(head), len(head), 0, 0]
    assert dev_cut(text, len(head) - 1, 1, 0) == sam_stream_model.cutter(head[:-1], True, 0)
    from besst_amd import _lib
    lib = _lib.load()
    assert lib.besst_dev_sam_lines(None, C.c_void_p(16), 1 << 32, 0, 0, C.c_void_p(16)) == 1      # refused without a launch
    assert lib.besst_dev_sam_lines(None, C.c_void_p(8), 16, 0, 0, C.c_void_p(16)) == 1
    assert lib.besst_dev_sam_lines(None, C.c_void_p(16), 16, 0, 17, C.c_void_p(16)) == 1


# ---- 2. the designed files, round for round ------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def designed():
    cases = sam_stream_design.designed_files()
    plans = sam_stream_design.census(cases)
    models = {}
    for case in cases:
        if 'too_long' not in case and case['text'] not in models:
            model = sam_model.decode(case['text'])
            models[case['text']] = (model, bam_report_model.words(model, len(model['references'])))
    return {case['name']: (case, plans[case['name']], models.get(case['text'])) for case in cases}


NAMES = ['borders_97', 'borders_700', 'borders_65280', 'hand_cut', 'long_header_700', 'no_final_newline_700', 'header_only_97',
         'header_only_no_newline_700', 'line_too_long_65280']


@pytest.mark.parametrize('name', NAMES)
def test_designed_file(designed, name, tmp_path):
    from besst_amd import bamio
    assert sorted(designed) == sorted(NAMES)
    case, plan, ref = designed[name]
    path = put(tmp_path, name + '.sam.gz', case['data'])
    if 'too_long' in case:
        with pytest.raises(bamio.SamError) as err:
            bamio.ResidentSam(path, chunk_bytes=CHUNK, tile_bytes=TILE)
        assert (err.value.offset, err.value.reason, err.value.line) == (case['too_long'], 'line longer than a chunk', None)
        assert 'chunk_bytes' in str(err.value)
        return
    model, words = ref
    sam = bamio.ResidentSam(path, chunk_bytes=CHUNK, tile_bytes=TILE)
    try:
        assert_is_model(sam, model, words, name)
        assert sam.inflate == 'device' and sam.ingest.inflated_bytes == len(case['text'])
        assert sam.ingest.chunks == len(plan.pushes) and sam.ingest.bytes_h2d == len(case['data'])
        assert sam.inflate_stats['rounds'] == len(plan.rounds) and sam.inflate_stats['host_from'] is None
        if case.get('header_only'):
            assert len(sam) == 0 and sam.ingest.chunks == 0
        else:
            assert sam.ingest.chunks > 1                         # (one push of the whole text before the reader streamed)
    finally:
        sam.close()


def test_blocks_the_device_kernel_refuses_are_inflated_on_the_host(designed, tmp_path, monkeypatch):
    """reasons 1..8 of the first bad block: the round's blocks go through zlib and land where the device put them.  The
    device takes every block zlib writes, so the first round's answer is made to say that it refused block 0."""
    from besst_amd import bamio
    case, plan, (model, words) = designed['borders_700']
    real, calls = bamio.ResidentSam._cut, []

    def cut(self, *args):
        got = real(self, *args)
        calls.append(1)
        if len(calls) == 1:
            got[4] = (0 << 8) | 3
        return got
    monkeypatch.setattr(bamio.ResidentSam, '_cut', cut)
    sam = bamio.ResidentSam(put(tmp_path, 'refused.sam.gz', case['data']), chunk_bytes=CHUNK, tile_bytes=TILE)
    try:
        assert_is_model(sam, model, words)
        assert sam.inflate_stats['host_rounds'] == 1 and sam.ingest.chunks == len(plan.pushes)
    finally:
        sam.close()


# ---- 3. other gzip: streamed on the host -----------------------------------------------------------------------------------------
@pytest.mark.parametrize('form', ['one_member', 'three_members'])
def test_gzip_is_streamed_on_the_host(designed, form, tmp_path):
    from besst_amd import bamio
    case, _, (model, words) = designed['borders_700']
    text = case['text']
    if form == 'one_member':
        data = gzip.compress(text)
    else:
        a, b = len(text) // 3 + 5, 2 * len(text) // 3 + 1        # (the members end in the middle of lines)
        data = gzip.compress(text[:a]) + gzip.compress(text[a:b]) + gzip.compress(text[b:])
    path = put(tmp_path, form + '.sam.gz', data)
    sam = bamio.ResidentSam(path, chunk_bytes=CHUNK, tile_bytes=TILE)
    try:
        assert_is_model(sam, model, words, form)
        assert sam.inflate == 'host' and sam.ingest.chunks > 1 and sam.ingest.inflated_bytes == len(text)
        plain = sam_design.chunk_plan(len(text) - model['header_bytes'],
                                      [at - model['header_bytes'] for at in model['offsets'][1:]] + [len(text) - model['header_bytes']],
                                      CHUNK)
        assert sam.ingest.chunks == len(plain)                   # the plain reader's chunks
    finally:
        sam.close()
    sam = bamio.ResidentSam(path, chunk_bytes=CHUNK, tile_bytes=TILE, gzip_on_gpu=True)
    try:
        assert_is_model(sam, model, words, form + ' on the device')
        assert sam.inflate == 'device_gzip', sam.inflate_stats
    finally:
        sam.close()


def test_a_gzip_member_behind_a_bgzf_chain(designed, tmp_path):
    from besst_amd import bamio
    case, _, (model, words) = designed['borders_700']
    text = case['text']
    for cut in (len(text) // 2 + 3, 100):                        # in the middle of a record line; inside the header
        front = b''.join(bgzf_writer.blocks_of(text[:cut], payload=700, level=1))
        data = front + gzip.compress(text[cut:])
        sam = bamio.ResidentSam(put(tmp_path, 'chain_%d.sam.gz' % cut, data), chunk_bytes=CHUNK, tile_bytes=TILE)
        try:
            assert_is_model(sam, model, words, 'cut at %d' % cut)
            assert sam.inflate == 'device' and sam.inflate_stats['host_from'] == len(front)
            assert sam.ingest.inflated_bytes == len(text)
        finally:
            sam.close()


# ---- 4. errors -------------------------------------------------------------------------------------------------------------------
def error_text(bad):
    good = [sam_design.GOOD_LINE.replace('read', 'read%d' % i, 1) for i in range(300)]
    lines = good[:200] + [bad] + good[200:250] + [bad] + good[250:]
    return sam_design.header_bytes() + ('\n'.join(lines) + '\n').encode()


@pytest.mark.parametrize('case', sam_design.ERROR_LINES, ids=lambda c: c[0])
def test_error_behind_the_third_round(case, tmp_path):
    from besst_amd import bamio
    _, bad, code = case
    text = error_text(bad)
    with pytest.raises(sam_model.SamModelError) as want:
        sam_model.decode(text)
    assert want.value.code == code
    isizes = [min(700, len(text) - at) for at in range(0, len(text), 700)] + [0]
    third = sam_stream_model.rounds(isizes, text, CHUNK).rounds[2]
    assert want.value.offset >= third['text_at'] + third['held']
    with pytest.raises(bamio.SamError) as err:
        bamio.ResidentSam(put(tmp_path, 'bad.sam.gz', bgzf_writer.bgzf(text, payload=700, level=1)), chunk_bytes=CHUNK, tile_bytes=TILE)
    assert (err.value.offset, err.value.line, err.value.reason) == (want.value.offset, want.value.line, bamio.SAM_REASONS[code])
    assert 'inflated' in str(err.value)
    with pytest.raises(bamio.SamError) as err:                   # and through the host's stream
        bamio.ResidentSam(put(tmp_path, 'bad.gz', gzip.compress(text)), chunk_bytes=CHUNK, tile_bytes=TILE)
    assert (err.value.offset, err.value.line, err.value.reason) == (want.value.offset, want.value.line, bamio.SAM_REASONS[code])


@pytest.mark.parametrize('how', ['payload', 'crc', 'isize+', 'isize-', 'cut'])
def test_damage_in_the_fourth_round(designed, how, tmp_path):
    from besst_amd import bamio
    case, plan, _ = designed['borders_700']
    fourth = plan.rounds[3]
    k = fourth['first_block'] + 1
    assert fourth['n_blocks'] > 2 and case['isizes'][k] == 700
    bad, at = bgzf_writer.damaged(case['data'], k, how)
    assert at == bgzf_writer.offsets(case['data'])[k] > 0
    with pytest.raises(bamio.SamError) as err:
        bamio.ResidentSam(put(tmp_path, 'damaged.sam.gz', bad), chunk_bytes=CHUNK, tile_bytes=TILE)
    assert (err.value.offset, err.value.reason, err.value.line) == (at, 'compressed data', None), str(err.value)
    assert 'compressed SAM file' in str(err.value) and 'not of the inflated text' in str(err.value)


# ---- 5. more than 4 GiB of text --------------------------------------------------------------------------------------------------
LONG = 4000


def long_line(i):
    return ('long%d\t99\tctg1\t%d\t60\t%dM\t=\t%d\t%d\t%s\t%s\n' % (i, 1 + i, LONG, 401 + i, 400 + LONG, 'ACGT' * (LONG // 4),
                                                                 'I' * LONG)).encode()


def repeated_file(path, n_blocks, last, seq=None):
    """header in a block of its own, one block of eight long lines written n_blocks times, ``last`` in a last block"""
    if seq is None:
        piece = b''.join(long_line(i) for i in range(8))
    else:
        piece = b''.join(long_line(i).replace(b'ACGT' * (LONG // 4), s) for i, s in enumerate(seq))
    assert len(piece) <= 65280
    one = bgzf_writer.block(piece, level=6)
    head = sam_design.header_bytes()
    with open(path, 'wb') as fh:
        fh.write(bgzf_writer.block(head, level=1))
        for at in range(0, n_blocks, 1024):
            fh.write(one * min(1024, n_blocks - at))
        if last:
            fh.write(bgzf_writer.block(last, level=1))
        fh.write(EOF)
    return head, piece


@pytest.mark.parametrize('bad', [True, False], ids=['a_bad_line', 'good'])
def test_more_than_four_gib_of_text(bad, tmp_path):
    """the file the whole-text reader refused (MemoryError): the error's offset and line number need all 64 bits"""
    from besst_amd import bamio
    piece_bytes = sum(len(long_line(i)) for i in range(8))
    n_blocks = -(-((1 << 32) + (1 << 26)) // piece_bytes)
    good = [sam_design.GOOD_LINE.replace('read', 'tail%d' % i, 1) + '\n' for i in range(4)]
    lines = good[:3] + ([sam_design.GOOD_LINE.replace('\t60\t', '\t256\t') + '\n'] if bad else []) + good[3:]
    path = str(tmp_path / 'huge.sam.gz')
    head, piece = repeated_file(path, n_blocks, ''.join(lines).encode())
    assert os.path.getsize(path) < 100 << 20
    body = n_blocks * len(piece)
    assert body > (1 << 32) + (1 << 26)
    if bad:
        with pytest.raises(bamio.SamError) as err:
            bamio.ResidentSam(path)
        at = len(head) + body + sum(len(l) for l in lines[:3])
        line = head.count(b'\n') + 8 * n_blocks + 4
        assert at > 1 << 32
        assert (err.value.offset, err.value.line, err.value.reason) == (at, line, bamio.SAM_REASONS[6]), str(err.value)
        return
    sam = bamio.ResidentSam(path)
    try:
        n = 8 * n_blocks + 4
        assert len(sam) == n and sam.inflate == 'device' and sam.ingest.chunks > 64
        assert sam.ingest.inflated_bytes == len(head) + body + sum(len(l) for l in lines)
        got = sam.ctx.fetch_records()
        first = sam_model.decode(head + piece)
        tail = sam_model.decode(head + ''.join(lines).encode())
        for k in COLS:
            assert np.array_equal(got[k][:8], first[k]) and np.array_equal(got[k][n - 12:n - 4], first[k]), k
            assert np.array_equal(got[k][n - 4:], tail[k]), k
        assert int(got['qlen'][0]) == LONG and np.array_equal(sam.rlen[:8], first['rlen'])
    finally:
        sam.close()


# ---- 6. the text is not resident ---------------------------------------------------------------------------------------------------
def test_the_text_is_not_resident(tmp_path):
    """a condition, not a measurement: the peak of the device memory the reader asks for is that of its buffers, whatever
    the file's size - files of T and 4 T text, T = 64 chunks of 1 MiB, differ by less than a chunk"""
    import torch
    from besst_amd import bamio
    chunk = 1 << 20
    rng = np.random.RandomState(5)
    seq = [bytes(rng.choice(np.frombuffer(b'ACGT', dtype=np.uint8), size=LONG)) for _ in range(8)]
    piece_bytes = sum(len(long_line(i)) for i in range(8))
    peaks, counts = [], []
    for k in (1, 4):
        n_blocks = -(-k * 64 * chunk // piece_bytes)
        path = str(tmp_path / ('text_%d.sam.gz' % k))
        repeated_file(path, n_blocks, b'', seq)
        assert os.path.getsize(path) > 4 * chunk                 # (the compressed windows are full-sized for both)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        sam = bamio.ResidentSam(path, chunk_bytes=chunk)
        try:
            peaks.append(torch.cuda.max_memory_allocated() - base)
            counts.append(len(sam))
            assert len(sam) == 8 * n_blocks and sam.ingest.chunks >= n_blocks * piece_bytes // (chunk + 65536) > 48 * k
            assert sam.ingest.inflated_bytes == n_blocks * piece_bytes + len(sam_design.header_bytes())
        finally:
            sam.close()
    assert counts[1] > 3 * counts[0]
    assert peaks[0] > 2 * chunk and abs(peaks[1] - peaks[0]) < chunk, peaks
