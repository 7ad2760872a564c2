"""SequenceStore.from_fasta on a gzip or BGZF contig FASTA: BGZF is inflated on the device, block by block at its place in
the text (GenerateOutput._upload_bgzf_file, besst_dev_bgzf_inflate), any other gzip file by zlib on the host
(_upload_gzip_host); then the same parser.  The yardstick is the parser on the plain bytes (GenerateOutput.parse_fasta_text,
itself held to the reference's reader by tests/test_gpu_fasta_reader.py); the files come from tests/bgzf_writer.py and are
checked with zlib alone before the device sees them.

Which path a case takes is asserted through ``store.inflate``: 'device' for every BGZF layout, 'host' for the fall-backs.
A damaged block reaches FastaError either way - through the device's CRC-32 / ISIZE check, or, where the kernel's status
refuses the DEFLATE data, through the host fall-back's zlib - with the same compressed offset."""
import gc
import gzip
import os
import socket
import subprocess
import sys
import types

import numpy as np
import pytest

from besst_amd import GenerateOutput as GO
from tests import bgzf_util as BU
from tests import bgzf_writer as BW
from tests import fasta_util as FU
from tests import flow_util as FLOW

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAD = GO.EMIT_PAD
TILES = (1024, None)
PAYLOADS = (1, 7, 61, 4096, 65280, 65536)


def device_text(data):
    import torch
    t = torch.zeros(len(data) + PAD, dtype=torch.uint8, device='cuda')
    if data:
        t[:len(data)] = torch.frombuffer(bytearray(data), dtype=torch.uint8)
    return t


def plain_parse(data, tile=None):
    """the parser on the plain bytes -> dict(names, offsets, lengths, pool) as Python values, or ('error', offset)"""
    try:
        out = GO.parse_fasta_text(device_text(data), len(data), tile)
    except GO.FastaError as exc:
        return ('error', exc.offset)
    n = out['pool_bytes']
    blob, at = out['names'].cpu().numpy().tobytes().decode('ascii'), out['name_off'].cpu().tolist()
    return dict(names=[blob[a:b] for a, b in zip(at[:-1], at[1:])], offsets=out['ctg_off'].cpu().tolist(),
                lengths=out['ctg_len'].cpu().tolist(), pool=out['pool'][PAD:PAD + n].cpu().numpy().tobytes())


def file_parse(path, tile=None, **kw):
    """from_fasta on a file -> (the same dict or ('error', offset), store.inflate)"""
    try:
        store = GO.SequenceStore.from_fasta(path, tile_bytes=tile, **kw)
    except GO.FastaError as exc:
        return ('error', exc.offset), None
    with store:
        n = store.pool_bytes
        assert store._pool[:PAD].count_nonzero().item() == 0 and store._pool[PAD + n:].count_nonzero().item() == 0
        return dict(names=list(store.names), offsets=store.offsets.tolist(), lengths=store.lengths.tolist(),
                    pool=store._pool[PAD:PAD + n].cpu().numpy().tobytes()), store.inflate


def write(path, data):
    with open(str(path), 'wb') as fh:
        fh.write(data)
    return str(path)


def acgt(n, seed):
    return np.frombuffer(b'ACGT', dtype=np.uint8)[np.random.default_rng(seed).integers(0, 4, n)].tobytes()


def fasta_text(n, seed=1, line=70):
    """about n bytes of contigs in lines of ``line`` bases"""
    rng = np.random.default_rng(seed)
    parts, have, k = [], 0, 0
    while have < n:
        k += 1
        seq = acgt(int(rng.integers(1, 4000)), seed * 1000 + k)
        new = b'>contig_%d len=%d\n' % (k, len(seq)) + b'\n'.join(seq[a:a + line] for a in range(0, len(seq), line)) + b'\n'
        parts.append(new)
        have += len(new)
    return b''.join(parts)


# ---- 1. the fixture of the reference's reader, in blocks of every size ----------------------------------------------------------
@pytest.fixture(scope='module')
def fixture_files():
    """[(case name, plain bytes, {payload: BGZF bytes})], every file checked with zlib"""
    out = []
    for k, case in enumerate(FU.load_golden()['cases']):
        files = {}
        for payload in PAYLOADS:
            files[payload] = BW.bgzf(case['data'], payload, level=(1, 6, 9)[k % 3])
            assert BW.host_inflate(files[payload]) == (case['data'], None)
        out.append((case['name'], case['data'], files))
    assert len(out) == 49
    return out


@pytest.mark.parametrize('tile', TILES)
def test_fixture_cases_in_blocks_of_every_size(fixture_files, tile, tmp_path):
    errors = 0
    for name, data, files in fixture_files:
        want = plain_parse(data, tile)
        errors += isinstance(want, tuple)
        for payload, content in files.items():
            got, inflate = file_parse(write(tmp_path / 'case.fa.gz', content), tile)
            assert got == want, (name, payload)
            assert inflate == (None if isinstance(want, tuple) else 'device'), (name, payload)
    assert errors >= 5                                           # texts the parser refuses, at the same inflated offset
    with pytest.raises(GO.FastaError, match='inflated text'):
        bad = [data for name, data, _ in fixture_files if name == 'non_ascii_byte'][0]
        GO.SequenceStore.from_fasta(write(tmp_path / 'bad.gz', BW.bgzf(bad, 7)), tile_bytes=tile)


def test_a_plain_file_is_read_as_before(fixture_files, tmp_path, monkeypatch):
    monkeypatch.setattr(GO, '_upload_gzip_file', None)           # not called for a file without the magic, whatever its name
    for name, data, _ in fixture_files:
        got, inflate = file_parse(write(tmp_path / 'plain.fa.gz', data))
        assert got == plain_parse(data) and inflate is None, name


# ---- 2. layouts --------------------------------------------------------------------------------------------------------------
TEXT = fasta_text(150000, seed=2)


def libdeflate_file(text, payload, level):
    from tests import libdeflate_util as LD
    return b''.join(BW.block(text[at:at + payload], deflate=LD.deflate(text[at:at + payload], level))
                    for at in range(0, len(text), payload)) + BU.EOF


def layouts():
    out = {
        'empty blocks first, in the middle and last': (BW.bgzf(TEXT, 9000, empty_at=(0, 1, 7, 8, -1)), TEXT),
        'no EOF block': (BW.bgzf(TEXT, 65280, eof=False), TEXT),
        'level 0 (stored)': (BW.bgzf(TEXT, 65280, level=0), TEXT),
        'level 1': (BW.bgzf(TEXT, 65280, level=1), TEXT),
        'level 6, blocks of 65536': (BW.bgzf(TEXT, 65536, level=6), TEXT),
        'level 9': (BW.bgzf(TEXT, 30011, level=9), TEXT),
        'a second extra subfield': (BW.bgzf(TEXT, 20000, extra=BW.subfield(b'XY', b'0123456')), TEXT),
        'EOF blocks only': (BU.EOF * 3, b''),
        'one EOF block': (BU.EOF, b''),
    }
    return out


@pytest.mark.parametrize('what', sorted(layouts()))
def test_layouts(what, tmp_path):
    content, text = layouts()[what]
    assert BW.host_inflate(content) == (text, None)
    got, inflate = file_parse(write(tmp_path / 'x.fa.gz', content))
    assert got == plain_parse(text) and inflate == 'device'
    if not text:                                                 # what the empty plain file gives
        assert got == file_parse(write(tmp_path / 'empty.fa', b''))[0] and got['pool'] == b''


def test_blocks_from_libdeflate(tmp_path):
    from tests import libdeflate_util as LD
    if not LD.available():
        pytest.skip('no libdeflate in this image')
    want = plain_parse(TEXT)
    for level, payload in ((1, 65280), (6, 65280), (12, 40000)):
        content = libdeflate_file(TEXT, payload, level)
        assert BW.host_inflate(content) == (TEXT, None)
        assert file_parse(write(tmp_path / 'ld.fa.gz', content)) == (want, 'device'), level


def test_the_package_s_own_bgzf_files(tmp_path):
    """bgzf_compress's output, and a file the shape --final_fasta --bgzf_outputs leaves: a stream whose EOF block is cut off,
    a second stream behind it, one EOF block at the end"""
    repeats = fasta_text(30000, seed=9)
    for content, text in ((GO.bgzf_compress(TEXT), TEXT), (GO.bgzf_compress(TEXT, block_payload=4096), TEXT),
                          (GO.bgzf_compress(TEXT, eof=False) + GO.bgzf_compress(repeats), TEXT + repeats)):
        assert BW.host_inflate(content) == (text, None) and content.count(BU.EOF) >= 1 and content.endswith(BU.EOF)
        assert file_parse(write(tmp_path / 'own.fa.gz', content)) == (plain_parse(text), 'device')


# ---- 3. the borders of the pipeline ---------------------------------------------------------------------------------------------
def test_windows_and_launches_cut_anywhere(tmp_path, monkeypatch):
    """10 MB in blocks of 1 KiB, windows of 64 KiB + 1 (they end inside headers and payloads; every window carries a cut
    block into the next) and 64 blocks per launch (a launch boundary inside every window)"""
    import torch
    text = BU.scaffold_text(10_000_000, seed=4)
    content = BW.bgzf(text, 1024, level=1)
    sizes = {b[1] for b in BW.walk(content)[0]}
    assert gzip.decompress(content) == text and len(content) > 40 * 65537 and max(sizes) < 2000
    monkeypatch.setattr(GO, 'UPLOAD_CHUNK', 65536 + 1)
    calls, lib = [], GO._lib.load()
    real = lib.besst_dev_bgzf_inflate
    want = GO.parse_fasta_text(device_text(text), len(text))
    path = write(tmp_path / 'big.fa.gz', content)
    with monkeypatch.context() as mp:                            # (blocks, first block, inflated bytes of every launch)
        mp.setattr(lib, 'besst_dev_bgzf_inflate', lambda *a: calls.append((a[3], a[4], a[5])) or real(*a))
        text_dev, n = GO._upload_bgzf_file(torch, torch.device('cuda', 0), path, *GO.bgzf_walk(path)[:2], blocks_per_launch=64)
    assert n == len(text) and torch.equal(text_dev[:n].cpu(), torch.frombuffer(bytearray(text), dtype=torch.uint8))
    assert text_dev[n:].count_nonzero().item() == 0
    del text_dev
    n_blocks = len(BW.walk(content)[0])
    assert sum(c[0] for c in calls) == n_blocks and [c[1] for c in calls] == np.cumsum([0] + [c[0] for c in calls[:-1]]).tolist()
    assert max(c[0] for c in calls) == 64 and sum(1 for c in calls if c[0] < 64) >= 30   # launches cut by 64, and by the windows' ends
    assert sum(c[2] for c in calls) == len(text)
    with GO.SequenceStore.from_fasta(path, blocks_per_launch=64) as store:
        assert store.inflate == 'device' and store.pool_bytes == want['pool_bytes']
        assert torch.equal(store._pool, want['pool']) and torch.equal(store._off, want['ctg_off'])
        assert torch.equal(store._len, want['ctg_len']) and torch.equal(store._names, want['names'])
        assert torch.equal(store._name_off, want['name_off'])


# ---- 4. a text of more than 2^32 bytes --------------------------------------------------------------------------------------------
def test_past_four_gigabytes(tmp_path):
    """One block of 65280 'A', some 65800 times, and five header blocks placed as tests/test_gpu_fasta_reader.py places its
    headers - one of them across inflated offset 2^32: a file of a few MB, a text of 4.3 GB."""
    import torch
    full = BW.block(b'A' * 65280)
    assert len(full) < 200
    n = (1 << 32) + 2 * 16384 + 123
    breaks = [1400000007, 2800000011, (1 << 32) - 2, n - 50]      # the '\n' in front of every later header
    parts, at, n_blocks = [BW.block(b'>a\n')], 3, 1
    for stop, name in zip(breaks + [n], b'bcde' + b'\0'):
        k, rest = divmod(stop - at, 65280)
        parts.append(full * k)
        if rest:
            parts.append(BW.block(b'A' * rest))
        n_blocks += k + bool(rest)
        at = stop
        if stop != n:
            parts.append(BW.block(b'\n>' + bytes([name]) + b'\n'))
            at, n_blocks = at + 4, n_blocks + 1
    content = b''.join(parts) + BU.EOF
    assert len(content) < 16 << 20 and n_blocks > 65800
    path = write(tmp_path / 'long.fa.gz', content)
    assert GO.bgzf_walk(path) == (n_blocks + 1, n, len(content), len(content))
    starts = [3] + [b + 4 for b in breaks]
    lengths = [e - s for s, e in zip(starts, breaks + [n])]
    offsets = [0] + np.cumsum(lengths)[:-1].tolist()
    assert max(lengths) < 1 << 31 and breaks[2] < 1 << 32 < breaks[2] + 4
    with GO.SequenceStore.from_fasta(path, tile_bytes=16384) as store:
        assert store.inflate == 'device' and store.names == ['a', 'b', 'c', 'd', 'e']
        assert store.pool_bytes == sum(lengths) == n - 3 - 4 * len(breaks)
        assert store.lengths.tolist() == lengths and store.offsets.tolist() == offsets
        assert not bool((store._pool[PAD:PAD + store.pool_bytes] != 65).any())


# ---- 5. damaged files ---------------------------------------------------------------------------------------------------------------
PER_LAUNCH = 8
DAMAGE_TEXT = fasta_text(40000, seed=5)


@pytest.fixture(scope='module')
def damage_file():
    content = BW.bgzf(DAMAGE_TEXT, 1024, level=6)
    blocks = BW.walk(content)[0]
    assert len(blocks) > 3 * PER_LAUNCH and blocks[-1][4] == 0 and blocks[-2][4] > 0
    return content, {'first': 0, 'second launch': PER_LAUNCH + PER_LAUNCH // 2, 'last': len(blocks) - 2}


def raises_at(path, at):
    import torch
    gc.collect()
    before = torch.cuda.memory_allocated()
    with pytest.raises(GO.FastaError) as err:
        GO.SequenceStore.from_fasta(path, blocks_per_launch=PER_LAUNCH)
    assert err.value.offset == at and ('byte %d' % at) in str(err.value)
    del err
    gc.collect()
    assert torch.cuda.memory_allocated() <= before               # no store, no text left behind


@pytest.mark.parametrize('where', ['first', 'second launch', 'last'])
@pytest.mark.parametrize('how', ['payload', 'crc', 'isize+', 'isize-', 'cut'])
def test_a_damaged_block_is_named_by_its_compressed_offset(damage_file, how, where, tmp_path):
    content, places = damage_file
    bad, at = BW.damaged(content, places[where], how)
    assert at == BW.offsets(content)[places[where]] and (at > 0) == (where != 'first')
    assert BW.host_inflate(bad) == (None, at)                    # zlib fails there too
    raises_at(write(tmp_path / 'bad.fa.gz', bad), at)


def test_bytes_behind_the_last_block(damage_file, tmp_path):
    content, _ = damage_file
    bad = content + b'0123456789'
    assert BW.host_inflate(bad) == (None, len(content))
    raises_at(write(tmp_path / 'bad.fa.gz', bad), len(content))
    # and the damaged files do not spoil the next good one
    assert file_parse(write(tmp_path / 'good.fa.gz', content), blocks_per_launch=PER_LAUNCH) == (plain_parse(DAMAGE_TEXT), 'device')


def test_a_stored_block_s_flipped_byte_is_the_device_s_crc_mismatch(tmp_path, monkeypatch):
    """level 0: the flipped byte is a flipped base - every block inflates, the CRC-32 kernel is what finds it"""
    monkeypatch.setattr(GO, '_upload_gzip_host', None)           # (the host fall-back is not asked)
    content = BW.bgzf(DAMAGE_TEXT, 1024, level=0)
    for k in (0, PER_LAUNCH + 3, len(BW.walk(content)[0]) - 2):
        bad, at = BW.damaged(content, k, 'payload')
        assert BW.host_inflate(bad) == (None, at)
        with pytest.raises(GO.FastaError, match='CRC-32') as err:
            GO.SequenceStore.from_fasta(write(tmp_path / 'bad.fa.gz', bad), blocks_per_launch=PER_LAUNCH)
        assert err.value.offset == at
        bad, at = BW.damaged(content, k, 'isize+')
        with pytest.raises(GO.FastaError) as err:
            GO.SequenceStore.from_fasta(write(tmp_path / 'bad.fa.gz', bad), blocks_per_launch=PER_LAUNCH)
        assert err.value.offset == at


# ---- 6. the host fall-back ----------------------------------------------------------------------------------------------------------
def test_other_gzip_files_are_inflated_on_the_host(tmp_path, monkeypatch):
    want = plain_parse(TEXT)
    cut = len(TEXT) // 3
    files = {
        'gzip': gzip.compress(TEXT),
        'two members': gzip.compress(TEXT[:cut], 1) + gzip.compress(TEXT[cut:], 9),
        'a BGZF chain, then a plain member': BW.bgzf(TEXT[:cut], 4096) + gzip.compress(TEXT[cut:]),
        'a plain member, then a BGZF chain': gzip.compress(TEXT[:cut]) + BW.bgzf(TEXT[cut:], 4096),
    }
    monkeypatch.setattr(GO, 'UPLOAD_CHUNK', 40000)               # several uploads per file, a piece cut by a buffer's end
    for name, content in files.items():
        assert BW.host_inflate(content) == (TEXT, None)
        assert file_parse(write(tmp_path / 'x.fa.gz', content)) == (want, 'host'), name
    for name, data, _ in [(c['name'], c['data'], None) for c in FU.load_golden()['cases']]:
        got = file_parse(write(tmp_path / 'case.fa.gz', gzip.compress(data)))
        want_case = plain_parse(data)
        assert got == (want_case, None if isinstance(want_case, tuple) else 'host'), name


def test_a_block_the_kernel_refuses_sends_the_file_to_the_host(tmp_path, monkeypatch):
    content = BW.bgzf(TEXT, 4096)
    path = write(tmp_path / 'x.fa.gz', content)
    want = plain_parse(TEXT)
    assert file_parse(path) == (want, 'device')
    seen, real = [], GO._first_bad

    def refused(word):
        seen.append(real(word))
        return (3, 5)                                            # block 3: a code the kernel does not take
    monkeypatch.setattr(GO, '_first_bad', refused)
    assert file_parse(path) == (want, 'host') and seen == [None]


# ---- 7. the command line, and the file the package writes ------------------------------------------------------------------------
def read(path):
    with open(path, 'rb') as fh:
        return fh.read()


def tree(out):
    """every file under BESST_output but Statistics.txt (it holds times) -> {relative path: bytes}"""
    files = {}
    for dirpath, _dirs, fnames in os.walk(out):
        for fname in fnames:
            if fname != 'Statistics.txt':
                files[os.path.relpath(os.path.join(dirpath, fname), out)] = read(os.path.join(dirpath, fname))
    return files


@pytest.fixture(scope='module')
def inputs(tmp_path_factory):
    """contigs.fa, contigs.fa.gz (BGZF) and lib1..3.bam of the flow fixture's inputs, written once"""
    from tests import bam_writer
    asm, libs = FLOW.load_inputs()
    d = tmp_path_factory.mktemp('gz_inputs')
    fasta = FLOW.write_fasta(str(d / 'contigs.fa'), FLOW.contig_sequences(asm))
    packed = write(d / 'contigs.fa.gz', BW.bgzf(read(fasta), 65280, level=6))
    assert gzip.decompress(read(packed)) == read(fasta)
    bams = []
    for k, batch in enumerate(libs):
        bams.append(str(d / ('lib%d.bam' % (k + 1))))
        bam_writer.write_bam(bams[-1], batch, block_bytes=50000 + 7000 * k, align_records=bool(k % 2))
    return fasta, packed, bams


def run_cli(fasta, bams, out, extra):
    from besst_amd import cli
    doc = FLOW.load_doc('flow_a')
    argv, per_lib = FLOW.cli_args(doc['scenario'], fasta, bams, out)
    assert not per_lib
    assert cli.main(argv + extra) == 0
    return os.path.join(out, 'BESST_output')


@pytest.fixture(scope='module')
def plain_run(inputs, tmp_path_factory):
    """scenario A from the plain FASTA, with -filter_contigs too: what every compressed-input run must leave"""
    d = tmp_path_factory.mktemp('gz_plain')
    threshold = sorted(int(x) for x in FLOW.load_inputs()[0]['lengths'])[20] + 1
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(GO, 'time', types.SimpleNamespace(time=lambda: float(FLOW.UNIQUE_ID)))
        out = tree(run_cli(inputs[0], inputs[2], str(d / 'all'), ['--fasta_on_gpu']))
        filtered = tree(run_cli(inputs[0], inputs[2], str(d / 'filtered'), ['--fasta_on_gpu', '-filter_contigs', str(threshold)]))
    assert any(k.endswith('Scaffolds-pass3.fa') for k in out) and out != filtered
    return out, filtered, threshold


@pytest.mark.parametrize('extra', [['--fasta_on_gpu'], []], ids=['fasta_on_gpu', 'python_reader'])
def test_cli_reads_the_compressed_fasta(extra, inputs, plain_run, tmp_path, monkeypatch):
    monkeypatch.setattr(GO, 'time', types.SimpleNamespace(time=lambda: float(FLOW.UNIQUE_ID)))
    out = run_cli(inputs[1], inputs[2], str(tmp_path / 'all'), extra)
    FLOW.assert_files_equal_fixture(out, FLOW.load_doc('flow_a'), 'flow_a from contigs.fa.gz')
    assert tree(out) == plain_run[0]
    out = run_cli(inputs[1], inputs[2], str(tmp_path / 'filtered'), extra + ['-filter_contigs', str(plain_run[2])])
    assert tree(out) == plain_run[1]


@pytest.mark.parametrize('extra', [['--fasta_on_gpu'], []], ids=['fasta_on_gpu', 'python_reader'])
def test_cli_two_ranks_read_the_compressed_fasta(extra, inputs, tmp_path):
    doc = FLOW.load_doc('flow_a')
    argv, per_lib = FLOW.cli_args(doc['scenario'], inputs[1], inputs[2], str(tmp_path))
    assert not per_lib
    with socket.socket() as s:
        s.bind(('127.0.0.1', 0))
        port = s.getsockname()[1]
    env = dict(os.environ, BESST_DIST_BACKEND='gloo', HSA_ENABLE_IPC_MODE_LEGACY='0')
    cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', '2', '--master-addr', '127.0.0.1',
           '--master-port', str(port), '-m', 'besst_amd.cli'] + argv + extra
    done = subprocess.run(cmd, cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    assert done.returncode == 0, done.stdout.decode()[-3000:]
    FLOW.assert_files_equal_fixture(str(tmp_path / 'BESST_output'), doc, 'flow_a from contigs.fa.gz, two ranks', uid=True)


def test_round_trip_of_a_pass_s_own_output(inputs, plain_run, tmp_path, monkeypatch):
    """Scaffolds-pass1.fa.gz of a --scaffolds --bgzf_outputs run, read back, against the .fa of the same pass without the
    switch"""
    import torch
    monkeypatch.setattr(GO, 'time', types.SimpleNamespace(time=lambda: float(FLOW.UNIQUE_ID)))
    monkeypatch.setattr(GO, 'BGZF_BLOCK_PAYLOAD', 4096)
    monkeypatch.setattr(GO, 'CHUNK_BYTES', 5 * 4096 + 9)
    out = run_cli(inputs[0], inputs[2], str(tmp_path / 'bgzf'), ['--fasta_on_gpu', '--bgzf_outputs'])
    packed = os.path.join(out, 'pass1', 'Scaffolds-pass1.fa.gz')
    plain = write(tmp_path / 'Scaffolds-pass1.fa', plain_run[0][os.path.join('pass1', 'Scaffolds-pass1.fa')])
    assert gzip.decompress(read(packed)) == read(plain) and len(BW.walk(read(packed))[0]) > 20
    with GO.SequenceStore.from_fasta(packed) as got, GO.SequenceStore.from_fasta(plain) as want:
        assert (got.inflate, want.inflate) == ('device', None)
        assert got.names == want.names and got.index == want.index and got.pool_bytes == want.pool_bytes
        assert torch.equal(got._pool, want._pool) and torch.equal(got._off, want._off) and torch.equal(got._len, want._len)
