"""A gzip or BGZF contig FASTA, the parts that need no GPU: the library's walk of a BGZF chain and its window scan
(besst_bgzf_walk, besst_bgzf_scan_chunk) against tests/bgzf_writer.py's walk of the same bytes; the walk's C++ as a
stand-alone program; the argument checks of the device inflate's entry points; the host inflate's member offsets; and the
command line's Python reader (cli.read_fasta) on the fixture of the reference's reader, compressed both ways."""
import ctypes as C
import gzip
import os
import shutil
import subprocess
import types

import numpy as np
import pytest

from besst_amd import GenerateOutput as GO
from besst_amd import _lib
from tests import bgzf_writer as BW
from tests import fasta_util as FU
from tests.bgzf_util import EOF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TEXT = b'>c1 x\n' + b'ACGTTGCA' * 90 + b'\n>c2\n' + b'GATTACA' * 55 + b'\n'
BIG = b'>big\n' + np.frombuffer(b'ACGT', dtype=np.uint8)[np.random.default_rng(3).integers(0, 4, 40000)].tobytes() + b'\n'


def lib_walk(data, max_blocks=-1):
    lib = _lib.load()
    buf = np.frombuffer(bytes(data), dtype=np.uint8)
    n, inflated, end = C.c_int64(-1), C.c_int64(-1), C.c_size_t(12345)
    assert lib.besst_bgzf_walk(_lib.ptr(buf) if len(data) else None, len(data), max_blocks, C.byref(n), C.byref(inflated),
                               C.byref(end)) == 0
    return n.value, inflated.value, end.value


def lib_scan(data, start=0, more_follows=False, max_blocks=1000, dst0=0):
    """-> ([(src_off, src_len, dst, dst_len, crc)], compressed bytes taken, inflated bytes) or None (an error)"""
    lib = _lib.load()
    buf = np.frombuffer(bytes(data), dtype=np.uint8)
    desc = np.full((max(1, max_blocks), 6), 0xEEEEEEEE, dtype=np.uint32)
    n, comp, inflated = C.c_int64(-1), C.c_size_t(0), C.c_int64(-1)
    rc = lib.besst_bgzf_scan_chunk(_lib.ptr(buf) if len(data) else None, len(data), start, 1 if more_follows else 0, max_blocks,
                                   dst0, _lib.ptr(desc), C.byref(n), C.byref(comp), C.byref(inflated))
    if rc:
        assert rc == 1 and (n.value, inflated.value) == (-1, -1)     # (the counts are not written)
        return None
    assert (desc[n.value:] == 0xEEEEEEEE).all()
    rows = [(int(d[0]), int(d[1]), int(d[2]) | (int(d[3]) << 32), int(d[4]), int(d[5])) for d in desc[:n.value]]
    return rows, comp.value, inflated.value


def model_scan(data, start=0, more_follows=False, max_blocks=1000, dst0=0):
    blocks, end, error = BW.walk(bytes(data)[start:], more_follows)
    if error and len(blocks) < max_blocks:
        return None
    rows, dst = [], dst0
    for at, size, p_at, p_len, isize, crc in blocks[:max_blocks]:
        rows.append((start + p_at, p_len, dst, isize, crc))
        dst += isize
        end = at + size
    if not blocks:
        end = 0
    return rows, end if rows else 0, dst - dst0


LAYOUTS = {
    'plain': BW.bgzf(TEXT, 300),
    'one block': BW.bgzf(TEXT),
    'no eof block': BW.bgzf(TEXT, 300, eof=False),
    'empty first': BW.bgzf(TEXT, 300, empty_at=(0,)),
    'empty in the middle': BW.bgzf(TEXT, 300, empty_at=(2, 3)),
    'empty last, twice': BW.bgzf(TEXT, 300, empty_at=(-1,)),
    'a second subfield': BW.bgzf(TEXT, 300, extra=BW.subfield()),
    'two more subfields': BW.bgzf(TEXT, 300, extra=BW.subfield(b'AB', b'') + BW.subfield(b'CD', b'0123456789')),
    'stored': BW.bgzf(TEXT, 300, level=0),
    'payload 1': BW.bgzf(TEXT[:70], 1),
    'eof blocks only': EOF * 3,
}


@pytest.mark.parametrize('what', sorted(LAYOUTS))
def test_walk_and_scan_of_whole_files(what):
    data = LAYOUTS[what]
    blocks, end, error = BW.walk(data)
    assert not error and end == len(data)
    text = b'' if what == 'eof blocks only' else TEXT[:70] if what == 'payload 1' else TEXT
    assert BW.host_inflate(data) == (text, None)                 # the input is what it is meant to be
    assert lib_walk(data) == (len(blocks), len(text), len(data))
    for k in range(len(blocks) + 1):
        at = blocks[k][0] if k < len(blocks) else len(data)
        assert lib_walk(data, k)[::2] == (k, at)
    assert lib_scan(data) == model_scan(data) == ([(b[2], b[3], sum(x[4] for x in blocks[:i]), b[4], b[5])
                                                   for i, b in enumerate(blocks)], len(data), len(text))
    # from a block in the middle, a few blocks, to a place past 2^32: offsets count from the window's first byte
    if len(blocks) > 4:
        start, dst0 = blocks[2][0], (1 << 32) - 100
        got = lib_scan(data, start, False, 2, dst0)
        assert got == model_scan(data, start, False, 2, dst0)
        assert got[0][0][0] == blocks[2][2] and got[0][0][2] == dst0 and got[1] == blocks[4][0] - start


def test_a_window_that_ends_anywhere():
    """every cut of a file: inside a header, inside a payload, inside a trailer, exactly on a boundary"""
    data = BW.bgzf(TEXT, 300, extra=BW.subfield(), empty_at=(1,))
    bounds = BW.offsets(data) + [len(data)]
    assert len(bounds) > 5
    for n in range(len(data) + 1):
        window = data[:n]
        whole = max(b for b in bounds if b <= n)
        got = lib_scan(window, 0, True)
        assert got == model_scan(window, 0, True), n
        assert got[1] == whole and len(got[0]) == bounds.index(whole)
        strict = lib_scan(window, 0, False)
        assert (strict is None) == (n not in bounds) and strict == model_scan(window, 0, False), n
        assert lib_walk(window)[2] == whole
    assert lib_scan(data, bounds[2], True, 0) == ([], 0, 0)
    assert lib_scan(data, len(data), True) == ([], 0, 0)


def malformed():
    good = BW.block(TEXT[:200], extra=BW.subfield())
    out = {}
    for name, at, value in (('magic 0', 0, 30), ('magic 1', 1, 138), ('method', 2, 7), ('no FEXTRA', 3, 0), ('XLEN < 6', 10, 5),
                            ('BC not first (B)', 12, 88), ('BC not first (C)', 13, 88), ('length of BC', 14, 3),
                            ('length of BC, high byte', 15, 1), ('XLEN beyond the block', 11, 1),
                            ('ISIZE > 65536', len(good) - 2, 2)):
        bad = bytearray(good)
        bad[at] = value
        out[name] = bytes(bad)
    out['BSIZE < header'] = good[:16] + b'\x10\0' + good[18:]
    out['BSIZE beyond the end'] = good[:16] + b'\xff\xff' + good[18:]
    out['a plain gzip member'] = gzip.compress(TEXT[:200])
    out['zero bytes'] = bytes(40)
    return good, out


def test_every_malformed_header_is_rejected():
    good, cases = malformed()
    assert lib_scan(good + good) == model_scan(good + good) and len(lib_scan(good + good)[0]) == 2
    for name, bad in sorted(cases.items()):
        for data in (bad, good + bad + good):
            assert BW.walk(data)[2], name
            assert lib_scan(data) is None and model_scan(data) is None, name
            assert lib_walk(data) == ((0, 0, 0) if data is bad else (1, 200, len(good))), name
        if name != 'BSIZE beyond the end':                       # (with more to come that one is a block cut by the window)
            assert lib_scan(good + bad, 0, True) is None, name
        # blocks in front of the bad one are still handed out when the scan is told to stop there
        assert lib_scan(good + bad, 0, False, 1) == model_scan(good + bad, 0, False, 1), name


def test_entry_points_refuse_bad_arguments_without_a_gpu():
    lib = _lib.load()
    p = C.c_void_p
    n, comp, inflated, end = C.c_int64(0), C.c_size_t(0), C.c_int64(0), C.c_size_t(0)
    buf = np.zeros(64, dtype=np.uint8)
    assert lib.besst_bgzf_walk(_lib.ptr(buf), 64, -1, None, C.byref(inflated), C.byref(end)) == 1
    assert lib.besst_bgzf_scan_chunk(_lib.ptr(buf), 64, 65, 0, 4, 0, _lib.ptr(buf), C.byref(n), C.byref(comp), C.byref(inflated)) == 1
    assert lib.besst_bgzf_scan_chunk(_lib.ptr(buf), 64, 0, 0, -1, 0, _lib.ptr(buf), C.byref(n), C.byref(comp), C.byref(inflated)) == 1
    assert lib.besst_bgzf_scan_chunk(_lib.ptr(buf), 64, 0, 0, 4, 0, None, C.byref(n), C.byref(comp), C.byref(inflated)) == 1
    ws = lib.besst_dev_bgzf_inflate_workspace_bytes
    assert ws(-1, 0) == 0 and ws(1, -1) == 0 and ws(1, 65537) == 0 and ws((1 << 24) + 1, 0) == 0
    assert ws(0, 0) > 0 and ws(1, 65536) >= 4 * 65536 + 4
    assert ws(4096, 4096 * 65536) >= 4 * 4096 * 65536 + 4 * 4096
    assert ws(4096, 4096 * 65280) < ws(4096, 4096 * 65536) < (4 * 4096 * 65536) * 1.01 + (1 << 23)
    need = ws(4, 1000)
    fake = 1 << 20                                               # (never dereferenced: every call ends at its argument check)
    call = lib.besst_dev_bgzf_inflate
    for args in ((None, p(fake), p(fake), 4, 0, 1000, p(fake), p(fake), need, None),
                 (None, None, p(fake), 4, 0, 1000, p(fake), p(fake), need, p(fake)),
                 (None, p(fake), None, 4, 0, 1000, p(fake), p(fake), need, p(fake)),
                 (None, p(fake), p(fake), 4, 0, 1000, None, p(fake), need, p(fake)),
                 (None, p(fake), p(fake), 4, 0, 1000, p(fake), None, need, p(fake)),
                 (None, p(fake), p(fake), -1, 0, 1000, p(fake), p(fake), need, p(fake)),
                 (None, p(fake), p(fake), 4, -1, 1000, p(fake), p(fake), need, p(fake)),
                 (None, p(fake), p(fake), 4, 0, 4 * 65536 + 1, p(fake), p(fake), 1 << 30, p(fake)),
                 (None, p(fake), p(fake), 4, 0, 1000, p(fake), p(fake), need - 1, p(fake)),
                 (None, p(fake + 2), p(fake), 4, 0, 1000, p(fake), p(fake), need, p(fake))):
        assert call(*args) == 1, args
        assert 'dev_bgzf_inflate' in _lib.last_error()


def _host_compiler():
    for name in (os.environ.get('CXX'), 'c++', 'g++', 'clang++', '/opt/rocm/llvm/bin/clang++'):
        path = shutil.which(name) if name else None
        if path:
            return path
    raise AssertionError('no host C++ compiler found (set CXX)')


def test_bgzf_walk_program(tmp_path):
    exe = str(tmp_path / 'bgzf_walk_test')
    src = os.path.join(ROOT, 'tests', 'cpp', 'bgzf_walk_test.cpp')
    built = subprocess.run([_host_compiler(), '-std=c++17', '-O1', '-Wall', '-Wextra', src, '-o', exe], capture_output=True, text=True)
    assert built.returncode == 0 and not built.stderr.strip(), built.stderr      # (a warning fails it too)
    ran = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert ran.returncode == 0, ran.stdout + ran.stderr


# ---- the host inflate: pieces and the offset of the member at fault ----------------------------------------------------------
def members(data, piece):
    import io
    try:
        return b''.join(GO._gzip_members(io.BytesIO(data), piece)), None
    except GO.FastaError as exc:
        return None, exc.offset


def test_host_inflate_names_the_member_at_fault():
    big = BIG
    files = {
        'gzip': gzip.compress(big),
        'two members': gzip.compress(big[:5000]) + gzip.compress(big[5000:]),
        'bgzf then gzip': BW.bgzf(big[:7000], 1000) + gzip.compress(big[7000:]),
        'bgzf': BW.bgzf(big, 4096),
        'empty members': gzip.compress(b'') + BW.bgzf(big, 4096, empty_at=(0, 2, -1)) + gzip.compress(b''),
    }
    for name, data in files.items():
        assert BW.host_inflate(data) == (big, None), name
        for piece in (1, 7, 1000, 1 << 20):
            if piece == 1 and len(data) > 20000:
                continue
            assert members(data, piece) == (big, None), (name, piece)
    data = files['bgzf']
    n = len(BW.offsets(data))
    for k in (0, n // 2, n - 2):
        for how in ('payload', 'crc', 'isize+', 'isize-', 'cut'):
            bad, at = BW.damaged(data, k, how)
            assert BW.host_inflate(bad) == (None, at), (k, how)
            for piece in (7, 1 << 20):
                assert members(bad, piece) == (None, at), (k, how, piece)
    for tail in (b'0123456789', b'\x1f\x8b', b'\0'):
        assert BW.host_inflate(data + tail) == (None, len(data))
        assert members(data + tail, 1000) == (None, len(data)), tail
    two = files['two members']
    second = len(gzip.compress(big[:5000]))
    assert second > 1000 and len(two) - second > 1000
    assert members(two[:-1], 1000) == (None, second) and members(BW.flip(two, second + 500), 1000) == (None, second)
    assert members(BW.flip(two, 500), 1000) == (None, 0)


# ---- cli.read_fasta ------------------------------------------------------------------------------------------------------
def read_outcome(path):
    from besst_amd import cli
    try:
        return list(cli.read_fasta(path).items())
    except Exception as exc:                                     # the reference's reader fails the way Python does
        return type(exc)


def test_read_fasta_on_the_fixture_compressed_both_ways(tmp_path):
    golden = FU.load_golden()
    assert len(golden['cases']) == 49
    outcomes = set()
    for k, case in enumerate(golden['cases']):
        data = case['data']
        forms = {'plain.fa': data, 'gzip.fa.gz': gzip.compress(data), 'bgzf.fa.gz': BW.bgzf(data, 61, level=1 + k % 9),
                 'named_plain.fa': BW.bgzf(data, 4096)}        # (the name does not matter)
        got = {}
        for name, content in forms.items():
            if name != 'plain.fa':
                assert BW.host_inflate(content) == (data, None)
            path = str(tmp_path / name)
            with open(path, 'wb') as fh:
                fh.write(content)
            got[name] = read_outcome(path)
        assert got['gzip.fa.gz'] == got['bgzf.fa.gz'] == got['named_plain.fa'] == got['plain.fa'], case['name']
        outcomes.add(got['plain.fa'] if isinstance(got['plain.fa'], type) else dict)
    assert dict in outcomes and len(outcomes) >= 2               # texts that are read and texts that are refused


def test_read_fasta_leaves_a_plain_file_that_looks_compressed_to_gzip(tmp_path):
    """the first bytes decide: two bytes of gzip magic in front of anything else is a damaged gzip file, not a FASTA"""
    from besst_amd import cli
    path = str(tmp_path / 'x.fa')
    with open(path, 'wb') as fh:
        fh.write(b'\x1f\x8b>c\nACGT\n')
    with pytest.raises(OSError):
        cli.read_fasta(path)


# ---- the command line on stand-ins ---------------------------------------------------------------------------------------
class _NoStore(object):
    def __init__(self, names, sequences, device=0):
        pass

    def close(self):
        pass


@pytest.mark.parametrize('form', ['bgzf', 'gzip'])
def test_cli_run_on_stand_ins_reads_a_compressed_fasta(form, monkeypatch, tmp_path):
    from besst_amd import MakeScaffolds as MS
    from besst_amd import bamio, cli, session
    from tests import fake_device
    from tests import flow_util as FLOW
    monkeypatch.setattr(session.device, 'GraphContext', fake_device.FakeGraphContext)
    monkeypatch.setattr(MS, 'chain_arrays', fake_device.fake_chain_arrays)
    monkeypatch.setattr(MS, 'linearize_arrays', fake_device.fake_linearize_arrays)
    monkeypatch.setattr(GO, 'PrintOutput', fake_device.fake_print_output)
    monkeypatch.setattr(GO, 'time', types.SimpleNamespace(time=lambda: float(FLOW.UNIQUE_ID)))
    doc = FLOW.load_doc('flow_a')
    asm, libs = FLOW.load_inputs()
    plain = FLOW.write_fasta(str(tmp_path / 'plain.fa'), FLOW.contig_sequences(asm))
    with open(plain, 'rb') as fh:
        text = fh.read()
    fasta = str(tmp_path / 'contigs.fa.gz')
    with open(fasta, 'wb') as fh:
        fh.write(BW.bgzf(text, 65280, level=1) if form == 'bgzf' else gzip.compress(text, 1))
    os.remove(plain)
    opened = {'lib%d.bam' % (k + 1): FLOW.RecordBatch(b.references, b.lengths, **{c: getattr(b, c) for c in FLOW.COLS})
              for k, b in enumerate(libs)}
    for batch in opened.values():
        batch.close = lambda: None
    monkeypatch.setattr(bamio, 'open_bam', lambda path, threads=None: opened[path])
    monkeypatch.setattr(GO, 'SequenceStore', _NoStore)
    argv, per_lib = FLOW.cli_args(doc['scenario'], fasta, sorted(opened), str(tmp_path))
    args = cli.build_parser().parse_args(argv)
    for dest, values in per_lib.items():
        setattr(args, dest, values)
    assert cli._run(args, 0) == 0
    FLOW.assert_files_equal_fixture(str(tmp_path / 'BESST_output'), doc, 'flow_a, %s' % form)
