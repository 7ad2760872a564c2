"""SequenceStore.from_fasta(gzip_on_gpu=True) on plain gzip members: the device's parallel inflate (csrc/gzip_stream.hip,
DESIGN.md section 11.2) against the parser on the plain bytes, and against the model of the scheme
(tests/gzip_stream_model.py) - the same numbers of chunks, candidates and live chunks, exactly.  The streams are the designed
ones of tests/gzip_stream_design.py (tests/test_gzip_stream_model.py asserts on the CPU that each holds its border).
Damaged files must reach the host path's FastaError, word for word what ``gzip_on_gpu=False`` raises, with the device's
reason in ``inflate_stats``."""
import gc
import gzip
import os
import struct
import types
import zlib

import numpy as np
import pytest

from besst_amd import GenerateOutput as GO
from tests import bgzf_writer as BW
from tests import fasta_util as FU
from tests import flow_util as FLOW
from tests import gzip_stream_design as D
from tests import gzip_stream_model as M

pytestmark = pytest.mark.gpu

PAD = GO.EMIT_PAD
NAMES = sorted(D.streams())


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
    """from_fasta on a file -> (the same dict or ('error', offset), store.inflate, store.inflate_stats)"""
    try:
        store = GO.SequenceStore.from_fasta(path, tile_bytes=tile, **kw)
    except GO.FastaError as exc:
        return ('error', exc.offset), None, exc.inflate_stats
    with store:
        n = store.pool_bytes
        assert store._pool[:PAD].count_nonzero().item() == 0 and store._pool[PAD + n:].count_nonzero().item() == 0
        return dict(names=list(store.names), offsets=store.offsets.tolist(), lengths=store.lengths.tolist(),
                    pool=store._pool[PAD:PAD + n].cpu().numpy().tobytes()), store.inflate, store.inflate_stats


def write(path, data):
    with open(str(path), 'wb') as fh:
        fh.write(data)
    return str(path)


def counts(stats):
    return {k: stats[k] for k in ('chunks', 'candidates', 'live', 'text_bytes', 'status')}


# ---- 1. the designed streams at every chunk size -------------------------------------------------------------------------------
@pytest.mark.parametrize('name', NAMES)
def test_designed_streams(name, tmp_path):
    raw, text = D.streams()[name]
    path = write(tmp_path / 'x.fa.gz', M.gzip_member(raw, text))
    want = plain_parse(text)
    for chunk in D.CHUNKS:
        model = D.modelled(name, chunk)
        got, inflate, stats = file_parse(path, gzip_on_gpu=True, gzip_chunk_bytes=chunk)
        # (the stitched text holds DEFLATE data: the parser refuses it at the same byte, and the store is not made)
        assert inflate == (None if isinstance(want, tuple) else 'device_gzip') and got == want, chunk
        assert counts(stats) == dict(chunks=model['chunks'], candidates=model['candidates'], live=model['live'],
                                     text_bytes=len(text), status='ok'), chunk
        if name.startswith('mem1_') and chunk <= 1024:
            assert stats['live'] >= 10                           # (a single-chunk run does not pass for the parallel one)


@pytest.mark.parametrize('name', NAMES)
def test_designed_streams_text(name, tmp_path):
    """the inflated text itself, byte for byte, whether or not it is a FASTA file"""
    import torch
    raw, text = D.streams()[name]
    path = write(tmp_path / 'x.fa.gz', M.gzip_member(raw, text))
    for chunk in (256, 1024):
        stats = {}
        out, n = GO._upload_gzip_device(torch, torch.device('cuda', 0), path, chunk, stats)
        assert n == len(text) and stats['status'] == 'ok' and out.shape[0] == n + PAD
        assert out[:n].cpu().numpy().tobytes() == text and out[n:].count_nonzero().item() == 0, chunk


def test_header_fields_and_the_default_chunk(tmp_path):
    for name, (member, text, head) in D.header_variants().items():
        got, inflate, stats = file_parse(write(tmp_path / 'h.fa.gz', member), gzip_on_gpu=True, gzip_chunk_bytes=512)
        model = D.modelled('mem1_level6', 512)
        assert (got, inflate) == (plain_parse(text), 'device_gzip'), name
        assert (stats['chunks'], stats['candidates'], stats['live']) == (model['chunks'], model['candidates'], model['live']), name
    text = D.fasta_text(400000, seed=31)
    got, inflate, stats = file_parse(write(tmp_path / 'd.fa.gz', gzip.compress(text, 6)), gzip_on_gpu=True)
    assert (got, inflate, stats['status']) == (plain_parse(text), 'device_gzip', 'ok')
    assert stats['chunks'] == -(-(len(gzip.compress(text, 6)) - 18) // GO.GZIP_CHUNK_BYTES) >= 2 and stats['text_bytes'] == len(text)


# ---- 2. the fixture of the reference's reader ------------------------------------------------------------------------------------
@pytest.mark.parametrize('tile', (1024, None))
def test_fixture_cases_under_gzip(tile, tmp_path):
    cases = FU.load_golden()['cases']
    assert len(cases) == 49
    errors = 0
    for k, case in enumerate(cases):
        want = plain_parse(case['data'], tile)
        errors += isinstance(want, tuple)
        path = write(tmp_path / 'case.fa.gz', gzip.compress(case['data'], (1, 6, 9)[k % 3]))
        got, inflate, stats = file_parse(path, tile, gzip_on_gpu=True, gzip_chunk_bytes=(256, None)[k % 2])
        assert got == want, case['name']                         # (a parser error: the same inflated offset)
        assert stats['status'] == 'ok' and stats['text_bytes'] == len(case['data']), case['name']
        assert inflate == (None if isinstance(want, tuple) else 'device_gzip'), case['name']
    assert errors >= 5
    bad = [c['data'] for c in cases if c['name'] == 'non_ascii_byte'][0]
    with pytest.raises(GO.FastaError, match='inflated text'):
        GO.SequenceStore.from_fasta(write(tmp_path / 'bad.gz', gzip.compress(bad)), tile_bytes=tile, gzip_on_gpu=True)


# ---- 3. damage ---------------------------------------------------------------------------------------------------------------------
DAMAGE_CHUNK = 1024


def damaged_files():
    raw, text = D.streams()['mem1_level6']
    good = M.gzip_member(raw, text)
    chain = D.modelled('mem1_level6', DAMAGE_CHUNK)['chain']
    assert len(chain) >= 10

    def flipped(link):
        at = 10 + (link[1] + link[2]) // 16                      # a byte in the middle of the live chunk's bits
        return good[:at] + bytes([good[at] ^ 0x10]) + good[at + 1:]
    crc, isize = struct.unpack('<II', good[-8:])
    return good, text, {
        'first live chunk': flipped(chain[0]), 'a middle live chunk': flipped(chain[len(chain) // 2]),
        'last live chunk': flipped(chain[-1]), 'crc': good[:-8] + struct.pack('<II', crc ^ 0x8000, isize),
        'isize': good[:-8] + struct.pack('<II', crc, isize + 1), 'cut': good[:10 + len(raw) // 2]}


@pytest.mark.parametrize('how', ['first live chunk', 'a middle live chunk', 'last live chunk', 'crc', 'isize', 'cut'])
def test_damage_reaches_the_host_s_error(how, tmp_path):
    import torch
    good, text, files = damaged_files()
    path = write(tmp_path / 'bad.fa.gz', files[how])
    with pytest.raises(GO.FastaError) as host:
        GO.SequenceStore.from_fasta(path)
    gc.collect()
    before = torch.cuda.memory_allocated()
    with pytest.raises(GO.FastaError) as dev:
        GO.SequenceStore.from_fasta(path, gzip_on_gpu=True, gzip_chunk_bytes=DAMAGE_CHUNK)
    assert (str(dev.value), dev.value.offset) == (str(host.value), host.value.offset) and dev.value.offset == 0
    status = dev.value.inflate_stats['status']
    assert status in GO.GZIP_STATUS[1:] and host.value.inflate_stats['status'] is None
    if how in ('crc', 'isize'):
        assert status == how
    del dev, host
    gc.collect()
    assert torch.cuda.memory_allocated() <= before               # no store, no text, no workspace left behind
    # and a good file right after is the device's again
    got, inflate, stats = file_parse(write(tmp_path / 'good.fa.gz', good), gzip_on_gpu=True, gzip_chunk_bytes=DAMAGE_CHUNK)
    assert (got, inflate, stats['status']) == (plain_parse(text), 'device_gzip', 'ok')


def test_several_members_and_bytes_behind_the_member(tmp_path):
    text = D.streams()['mem8'][1]
    cut = len(text) // 3
    want = plain_parse(text)
    for name, content in {'two members': gzip.compress(text[:cut], 1) + gzip.compress(text[cut:], 9),
                          'a plain member, then a BGZF chain': gzip.compress(text[:cut]) + BW.bgzf(text[cut:], 4096)}.items():
        got, inflate, stats = file_parse(write(tmp_path / 'm.fa.gz', content), gzip_on_gpu=True, gzip_chunk_bytes=1024)
        assert got == want and inflate in ('device_gzip', 'host'), name
        assert stats['status'] == ('ok' if inflate == 'device_gzip' else 'trailing_bytes'), name
    path = write(tmp_path / 'tail.fa.gz', gzip.compress(text) + b'0123456789')
    with pytest.raises(GO.FastaError) as host:
        GO.SequenceStore.from_fasta(path)
    with pytest.raises(GO.FastaError) as dev:
        GO.SequenceStore.from_fasta(path, gzip_on_gpu=True)
    assert (str(dev.value), dev.value.offset) == (str(host.value), host.value.offset)


# ---- 4. a text of more than 2^32 bytes ---------------------------------------------------------------------------------------------
def unit(data):
    """``data`` as DEFLATE blocks that end on a byte boundary and need nothing in front of them but more of the same byte"""
    c = zlib.compressobj(6, zlib.DEFLATED, -15)
    return c.compress(data) + c.flush(zlib.Z_SYNC_FLUSH)


def test_past_four_gigabytes(tmp_path):
    """The text tests/test_gpu_bgzf_fasta_input.py builds - 4.3 GB of 'A' under five headers, one of them across inflated
    offset 2^32 - as ONE gzip member of a few MB: byte-aligned units of 65 280 'A' (a dynamic block each, ~100 bytes),
    repeated.  Chunks of 4 KiB hold ~40 units: no wave makes more than a few MB, and the chunks' places pass 2^32."""
    full = unit(b'A' * 65280)
    assert len(full) < 200 and zlib.decompress(full * 3 + b'\x03\x00', -15) == b'A' * (3 * 65280)
    n = (1 << 32) + 2 * 16384 + 123
    breaks = [1400000007, 2800000011, (1 << 32) - 2, n - 50]      # the '\n' in front of every later header
    parts, at, crc = [unit(b'>a\n')], 3, zlib.crc32(b'>a\n')
    piece = b'A' * (65280 * 256)
    for stop, name in zip(breaks + [n], b'bcde' + b'\0'):
        k, rest = divmod(stop - at, 65280)
        parts.append(full * k)
        if rest:
            parts.append(unit(b'A' * rest))
        left = stop - at
        while left:
            take = min(left, len(piece))
            crc = zlib.crc32(piece[:take], crc)
            left -= take
        at = stop
        if stop != n:
            header = b'\n>' + bytes([name]) + b'\n'
            parts.append(unit(header))
            crc, at = zlib.crc32(header, crc), at + 4
    raw = b''.join(parts) + b'\x03\x00'
    content = b'\x1f\x8b\x08\0\0\0\0\0\0\x03' + raw + struct.pack('<II', crc, n & 0xffffffff)
    assert len(content) < 16 << 20
    path = write(tmp_path / 'long.fa.gz', content)
    starts = [3] + [b + 4 for b in breaks]
    lengths = [e - s for s, e in zip(starts, breaks + [n])]
    offsets = [0] + np.cumsum(lengths)[:-1].tolist()
    assert max(lengths) < 1 << 31 and breaks[2] < 1 << 32 < breaks[2] + 4
    with GO.SequenceStore.from_fasta(path, tile_bytes=16384, gzip_on_gpu=True, gzip_chunk_bytes=4096) as store:
        assert store.inflate == 'device_gzip' and store.names == ['a', 'b', 'c', 'd', 'e']
        stats = store.inflate_stats
        assert stats['status'] == 'ok' and stats['text_bytes'] == n and stats['live'] > 1000
        assert stats['live'] >= 0.9 * stats['chunks']            # every wave makes about n / live bytes: ~3 MB
        assert store.pool_bytes == sum(lengths) == n - 3 - 4 * len(breaks)
        assert store.lengths.tolist() == lengths and store.offsets.tolist() == offsets
        assert not bool((store._pool[PAD:PAD + store.pool_bytes] != 65).any())


# ---- 5. the flag on other files, and the command line --------------------------------------------------------------------------------
def test_the_flag_changes_nothing_for_bgzf_and_plain_files(tmp_path, monkeypatch):
    text = D.streams()['mem8'][1]
    want = plain_parse(text)
    bgzf = write(tmp_path / 'b.fa.gz', BW.bgzf(text, 4096))
    plain = write(tmp_path / 'p.fa', text)
    zipped = write(tmp_path / 'z.fa.gz', gzip.compress(text))
    assert file_parse(zipped)[:2] == (want, 'host')              # the default stays the host
    monkeypatch.setattr(GO, '_upload_gzip_device', None)         # never asked for these
    for kw in ({}, {'gzip_on_gpu': True}, {'gzip_on_gpu': True, 'gzip_chunk_bytes': 256}):
        assert file_parse(bgzf, **kw)[:2] == (want, 'device'), kw
        assert file_parse(plain, **kw)[:2] == (want, None), kw
        assert file_parse(bgzf, **kw)[2]['status'] is None


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


def run_cli(fasta, bams, out, extra):
    from besst_amd import cli
    doc = FLOW.load_doc('flow_a')
    argv, per_lib = FLOW.cli_args(doc['scenario'], fasta, bams, out)
    assert not per_lib
    assert cli.main(argv + extra) == 0
    return os.path.join(out, 'BESST_output')


def test_cli_reads_the_gzip_fasta_on_the_gpu(tmp_path, monkeypatch):
    """scenario A from contigs.fa.gz (plain gzip) with --fasta_on_gpu --gzip_on_gpu: the files of the run from contigs.fa"""
    from tests import bam_writer
    asm, libs = FLOW.load_inputs()
    fasta = FLOW.write_fasta(str(tmp_path / 'contigs.fa'), FLOW.contig_sequences(asm))
    packed = write(tmp_path / 'contigs.fa.gz', gzip.compress(read(fasta), 6))
    bams = []
    for k, batch in enumerate(libs):
        bams.append(str(tmp_path / ('lib%d.bam' % (k + 1))))
        bam_writer.write_bam(bams[-1], batch, block_bytes=50000 + 7000 * k, align_records=bool(k % 2))
    monkeypatch.setattr(GO, 'time', types.SimpleNamespace(time=lambda: float(FLOW.UNIQUE_ID)))
    want = tree(run_cli(fasta, bams, str(tmp_path / 'plain'), ['--fasta_on_gpu']))
    seen, real = [], GO._upload_gzip_device

    def spy(*args):
        got = real(*args)
        seen.append((got is not None, args[4]['status']))
        return got
    monkeypatch.setattr(GO, '_upload_gzip_device', spy)
    out = run_cli(packed, bams, str(tmp_path / 'gz'), ['--fasta_on_gpu', '--gzip_on_gpu'])
    assert seen == [(True, 'ok')]
    FLOW.assert_files_equal_fixture(out, FLOW.load_doc('flow_a'), 'flow_a from contigs.fa.gz on the GPU')
    assert tree(out) == want and any(k.endswith('Scaffolds-pass3.fa') for k in want)
