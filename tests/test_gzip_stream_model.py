"""CPU checks of the parallel gzip inflate: the model (tests/gzip_stream_model.py) against zlib on
every designed stream at every chunk size; a census that the border each stream was designed for is really in it; the
host-compiled steps of the kernels (besst_amd/csrc/gzip_stream_core.h) run by tests/cpp/gzip_stream_core_test.cpp against
zlib; and what needs no GPU of the entry points, the header parse and the command line."""
import ctypes as C
import gzip
import os
import shutil
import subprocess
import zlib

import pytest

from besst_amd import GenerateOutput as GO
from besst_amd import _lib
from tests import gzip_stream_design as D
from tests import gzip_stream_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = sorted(D.streams())


@pytest.mark.parametrize('name', NAMES)
def test_the_model_is_zlib(name):
    raw, text = D.streams()[name]
    assert zlib.decompress(raw, -15) == text
    got, blocks = M.inflate(D.stream_model(name))
    assert got == text and blocks[-1][1] <= 8 * len(raw) and sum(b[4] for b in blocks) == len(text)
    for chunk in D.CHUNKS:
        r = D.modelled(name, chunk)
        assert r['text'] == text, chunk
        assert r['chunks'] == max(1, -(-len(raw) // chunk)) and r['live'] <= r['candidates'] + 1 <= r['chunks']
        places = [link[4] for link in r['chain']]
        assert places == sorted(places) and places[0] == 0 and places[-1] + r['chain'][-1][3] == len(text)


def census(name, chunk):
    """what the model sees of a stream at a chunk size"""
    raw, text = D.streams()[name]
    s, r = D.stream_model(name), D.modelled(name, chunk)
    blocks = M.inflate(s)[1]
    starts = {b[0]: b for b in blocks}
    cands = [8 * chunk * j + c for j, c in enumerate(r['cands']) if j and c is not None]
    live_starts = {link[1] for link in r['chain']}
    before = {b[1]: b[2] for b in blocks}                        # end bit -> type of the block that ends there
    return dict(blocks=blocks, types=[b[2] for b in blocks], cands=cands, false=[c for c in cands if c not in starts],
                dropped=[c for c in cands if c not in live_starts], live=r['live'], chunks=r['chunks'],
                without=sum(c is None for c in r['cands']), live_bytes=[link[3] for link in r['chain']],
                starts_per_chunk=[sum(1 for b in starts if b // (8 * chunk) == j) for j in range(r['chunks'])],
                live_behind=[before.get(link[1]) for link in r['chain'][1:]],
                landings=[link[2] for link in r['chain']], chain=r['chain'],
                distances=[t[1] for b in blocks for t in s.block(b[0])[3] if not isinstance(t, int)],
                lengths=[t[0] for b in blocks for t in s.block(b[0])[3] if not isinstance(t, int)])


def test_census_small_blocks():
    """memLevel 1: blocks of a few hundred bytes - several starts in every chunk, every live chunk far below 32 KiB (windows
    inherited many times in a row), no false candidate, every chunk live (but a last one that holds no start)"""
    for level in (1, 6, 9):
        for chunk in (512, 1024):
            c = census('mem1_level%d' % level, chunk)
            assert min(c['starts_per_chunk'][:-1]) >= 2 and max(c['live_bytes']) < 8192
            assert c['false'] == [] and c['live'] >= c['chunks'] - 1 and c['live'] >= 25
            assert c['live'] >= 10


def test_census_one_long_block():
    c = census('mem8', 1024)
    assert len(c['blocks']) == 1 and c['chunks'] >= 20 and c['without'] == c['chunks'] - 1 and c['live'] == 1
    assert c['live_bytes'] == [len(D.streams()['mem8'][1])]


def test_census_stitched():
    assert sorted(set(census('stitched', 1024)['types'])) == [0, 1, 2]
    for chunk in (256, 512, 1024):
        c = census('stitched', chunk)
        assert len(c['false']) >= 1 and len(c['dropped']) >= len(c['false'])     # headers inside the stored block's payload
        assert 0 in c['live_behind'] and 2 in c['live_behind']                   # a landing behind a stored block
        assert c['live'] < len(c['cands']) + 1


def test_census_repeats():
    z = census('repeat_zlib', 1024)
    assert max(z['distances']) > 32000 and max(z['distances']) <= 32506 and max(z['lengths']) == 258
    m = census('repeat_zlib_mem1', 512)
    far = [d for d in m['distances'] if d >= 32000]
    assert len(far) >= 3 * 8 and m['live'] >= 50 and max(m['live_bytes']) < 8192      # matches across dozens of live chunks
    if D.LD.available():
        for level in (1, 6, 12):
            c = census('repeat_libdeflate%d' % level, 1024)
            assert max(c['distances']) >= 32500 and c['live'] >= 2, level
    # distance 32 768 itself (zlib stops at 32 506): a hand-made match, read from in front of its live chunk
    for chunk in (256, 512, 1024):
        c = census('distance_32768', chunk)
        assert c['distances'][-1] == 32768 == max(c['distances']) and c['lengths'][-1] == 258
        assert c['live'] >= 3 and c['live_bytes'][-1] < 1000 and c['chain'][-1][5][-1] == c['blocks'][-1][0]


def test_census_flushes():
    for name, empty_type in (('sync_flush', 0), ('partial_flush', 1)):
        c = census(name, 1024)
        empties = [b for b in c['blocks'] if b[4] == 0]
        assert len(empties) >= 100 and {b[2] for b in empties} == {empty_type}
        assert c['live'] >= 10 and empty_type in c['live_behind']              # landings behind empty stored / fixed blocks
    # a landing that is no candidate: the final block's end
    c = census('sync_flush', 1024)
    assert c['landings'][-1] not in c['cands']


def test_census_empty_member():
    raw, text = D.streams()['empty']
    assert text == b'' and D.modelled('empty', 65536)['live'] == 1 and len(raw) == 2


def _host_compiler():
    for name in (os.environ.get('CXX'), 'c++', 'g++', 'clang++', '/opt/rocm/llvm/bin/clang++'):
        path = shutil.which(name) if name else None
        if path:
            return path
    raise AssertionError('no host C++ compiler found (set CXX)')


def test_gzip_stream_core_program(tmp_path):
    exe = str(tmp_path / 'gzip_stream_core_test')
    src = os.path.join(ROOT, 'tests', 'cpp', 'gzip_stream_core_test.cpp')
    built = subprocess.run([_host_compiler(), '-std=c++17', '-O1', '-Wall', '-Wextra', src, '-lz', '-o', exe], capture_output=True,
                           text=True)
    assert built.returncode == 0 and not built.stderr.strip(), built.stderr      # (a warning fails it too)
    ran = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert ran.returncode == 0, (ran.stdout + ran.stderr)[-3000:]


def test_entry_points_check_their_arguments_without_a_gpu():
    lib = _lib.load()
    ws = lib.besst_dev_gzip_plan_workspace_bytes
    assert ws(1 << 20, 10, 65536) > 0 and ws(1 << 20, 10, 256) > ws(1 << 20, 10, 65536)
    for chunk in (0, 255, 264, 128, (1 << 24) + 16, -16):
        assert ws(1 << 20, 10, chunk) == 0, chunk
    assert ws(17, 10, 256) == 0 and ws(18, 10, 256) > 0 and ws(100, -1, 256) == 0 and ws((1 << 35) + 1, 10, 65536) == 0
    assert lib.besst_dev_gzip_inflate_workspace_bytes(1000, 1) >= 2000
    assert lib.besst_dev_gzip_inflate_workspace_bytes(1000, 0) == 0 and lib.besst_dev_gzip_inflate_workspace_bytes(-1, 1) == 0
    p = C.c_void_p
    buf = (C.c_uint64 * 64)()
    at = C.addressof(buf)
    assert lib.besst_dev_gzip_plan(None, None, 100, 10, 256, 0, p(at), 1 << 20, p(at)) == 1 and 'null' in _lib.last_error()
    assert lib.besst_dev_gzip_plan(None, p(at), 100, 10, 250, 0, p(at), 1 << 20, p(at)) == 1 and 'range' in _lib.last_error()
    assert lib.besst_dev_gzip_plan(None, p(at), 100, 10, 256, 0, p(at), 16, p(at)) == 1 and 'small' in _lib.last_error()
    assert lib.besst_dev_gzip_plan(None, p(at + 2), 100, 10, 256, 0, p(at), 1 << 20, p(at)) == 1 and 'misaligned' in _lib.last_error()
    assert lib.besst_dev_gzip_inflate(None, p(at), 100, 10, 256, 0, None, 1, 50, p(at), p(at), 1 << 20, p(at)) == 1
    assert 'null' in _lib.last_error()
    assert lib.besst_dev_gzip_inflate(None, p(at), 100, 10, 256, 0, p(at), 2, 50, p(at), p(at), 1 << 20, p(at)) == 1
    assert 'n_live' in _lib.last_error()                         # more live chunks than chunks
    assert lib.besst_dev_gzip_inflate(None, p(at), 100, 10, 256, 0, p(at), 1, 50, p(at), p(at), 16, p(at)) == 1
    assert 'small' in _lib.last_error()
    with pytest.raises(ValueError, match='gzip_chunk_bytes'):
        GO.SequenceStore.from_fasta(os.devnull, gzip_on_gpu=True, gzip_chunk_bytes=1000)


def test_header_parse_against_gzip():
    for name, (member, text, head) in D.header_variants().items():
        assert gzip.decompress(member) == text, name
        assert GO.gzip_header_bytes(member[:GO.GZIP_HEADER_ROOM]) == head, name
        assert zlib.decompress(member[head:-8], -15) == text, name
        for cut in (1, 5, 9, head - 1):
            assert GO.gzip_header_bytes(member[:cut]) is None, (name, cut)
    plain = gzip.compress(b'>a\nACGT\n')
    assert GO.gzip_header_bytes(plain) == 10
    assert GO.gzip_header_bytes(b'\x1f\x8b\x07' + plain[3:]) is None          # CM
    assert GO.gzip_header_bytes(plain[:3] + b'\x20' + plain[4:]) is None      # a reserved flag bit
    assert GO.gzip_header_bytes(b'>a\nACGT\nACGT\n') is None


def test_cli_refuses_gzip_on_gpu_without_fasta_on_gpu(tmp_path):
    from besst_amd import cli
    argv = ['-c', 'contigs.fa.gz', '-f', 'lib.bam', '-orientation', 'fr', '-o', str(tmp_path), '--gzip_on_gpu']
    with pytest.raises(SystemExit) as err:
        cli.main(argv)
    assert '--gzip_on_gpu needs --fasta_on_gpu' in str(err.value.code)
