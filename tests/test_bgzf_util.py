"""CPU checks around the BGZF compressor (csrc/bgzf_deflate.hip): the validator the GPU tests rely on bites
(tests/bgzf_util.py), the bound's arithmetic, the argument errors of besst_dev_bgzf_deflate (returned without a GPU), the
new symbols in header, library and ctypes table, and the command line's refusal of --bgzf_outputs without --scaffolds."""
import ctypes as C
import gzip
import os
import re
import struct
import zlib

import numpy as np
import pytest

from besst_amd import Parameter, _lib, cli
from besst_amd import GenerateOutput as GO
from tests import bam_writer
from tests import bgzf_util as BU

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ['besst_bgzf_deflate_device', 'besst_dev_bgzf_deflate', 'besst_dev_bgzf_deflate_bound',
       'besst_dev_bgzf_deflate_workspace_bytes']
TEXT = BU.scaffold_text(3 * 4096 + 100, seed=5)


def test_constants():
    assert BU.EOF == GO.BGZF_EOF and len(BU.EOF) == 28
    assert gzip.decompress(BU.EOF) == b''
    assert GO.BGZF_BLOCK_PAYLOAD == BU.BLOCK_PAYLOAD == 0xff00


@pytest.mark.parametrize('payload', [16, 4096, 65280])
def test_validator_accepts_zlib_files(payload):
    for raw in (b'', b'x', TEXT[:payload], TEXT[:payload + 1], TEXT):
        data = BU.zlib_file(raw, payload)
        got, sizes = BU.validate(data, payload)
        assert got == raw == gzip.decompress(data)
        assert len(sizes) == -(-len(raw) // payload) and sum(sizes) + 28 == len(data)
        assert BU.yardstick(raw, payload) == len(data) - 28
    assert BU.validate(BU.zlib_file(TEXT, 4096, eof=False), 4096, eof=False)[0] == TEXT


def test_validator_accepts_a_bam_writer_file(tmp_path):
    from besst_amd.records import RecordBatch
    n = 3000
    z = np.zeros(n, dtype=np.int32)
    batch = RecordBatch(tid=z, mtid=z, pos=np.arange(n, dtype=np.int32), mpos=z, tlen=z, flag=np.zeros(n, np.uint16),
                        mapq=np.zeros(n, np.uint8), qlen=np.full(n, 50, np.uint16), references=['c1'], lengths=[100000])
    path = str(tmp_path / 'a.bam')
    bam_writer.write_bam(path, batch, block_bytes=60000)
    with open(path, 'rb') as fh:
        data = fh.read()
    raw, sizes = BU.validate(data, 60000)
    assert raw[:4] == b'BAM\x01' and len(sizes) >= 2 and raw == gzip.decompress(data)


def _blocks(payload=4096):
    return [BU.zlib_block(TEXT[at:at + payload]) for at in range(0, len(TEXT), payload)]


def test_validator_rejects_what_a_reader_would():
    blocks = _blocks()
    good = b''.join(blocks) + BU.EOF
    assert BU.validate(good, 4096)[0] == TEXT

    def broken(k, change):
        b = bytearray(blocks[k])
        change(b)
        return b''.join(blocks[:k]) + bytes(b) + b''.join(blocks[k + 1:]) + BU.EOF

    def flip_crc(b):
        b[-8] ^= 1

    def isize(b):
        b[-4:] = struct.pack('<I', struct.unpack('<I', bytes(b[-4:]))[0] + 1)

    with pytest.raises(BU.BgzfError, match='CRC'):
        BU.validate(broken(1, flip_crc), 4096)
    with pytest.raises(BU.BgzfError, match='ISIZE'):
        BU.validate(broken(2, isize), 4096)
    # BSIZE one too large (a byte of padding in front of the trailer) and one too small
    b = blocks[1]
    for delta, pad in ((1, b'\0'), (-1, b'')):
        wrong = b[:16] + struct.pack('<H', len(b) - 1 + delta) + b[18:-8] + pad + b[-8:]
        with pytest.raises(BU.BgzfError):
            BU.validate(blocks[0] + wrong + b''.join(blocks[2:]) + BU.EOF, 4096)
    with pytest.raises(BU.BgzfError, match='EOF'):
        BU.validate(b''.join(blocks), 4096)
    with pytest.raises(BU.BgzfError, match='EOF'):
        BU.validate(good + BU.EOF, 4096)
    with pytest.raises(BU.BgzfError, match='EOF'):
        BU.validate(blocks[0] + BU.EOF + b''.join(blocks[1:]) + BU.EOF, 4096)
    with pytest.raises(BU.BgzfError, match='carries'):
        BU.validate(blocks[0] + blocks[-1] + blocks[1] + BU.EOF, 4096)
    with pytest.raises(BU.BgzfError, match='header'):
        BU.validate(b'\x1f\x8b\x08\x00' + good[4:], 4096)


def test_validator_rejects_a_match_in_front_of_the_block():
    first, second = TEXT[:4096], TEXT[2048:4096] + TEXT[:2048]
    comp = zlib.compressobj(6, zlib.DEFLATED, -15, 8, zlib.Z_DEFAULT_STRATEGY, first)        # the block before as dictionary
    body = comp.compress(second) + comp.flush()
    assert zlib.decompressobj(-15, first).decompress(body) == second
    block = BU.HEADER + struct.pack('<H', len(body) + 25) + body + struct.pack('<II', zlib.crc32(second) & 0xffffffff, len(second))
    with pytest.raises(BU.BgzfError, match='on its own'):
        BU.validate(BU.zlib_block(first) + block + BU.EOF, 4096)


# ---- the library without a GPU ---------------------------------------------------------------------------------------------
def test_bound_arithmetic():
    lib = _lib.load()
    bound = lib.besst_dev_bgzf_deflate_bound
    assert bound(0, 65280, 0) == 0 and bound(0, 65280, 1) == 28
    assert bound(1, 65280, 0) == 32 and bound(1, 65280, 1) == 60
    assert bound(65280, 65280, 0) == 65280 + 31 and bound(65281, 65280, 0) == 65281 + 62
    assert bound(1000, 16, 1) == 1000 + 31 * 63 + 28
    n = (1 << 40) + 3
    assert bound(n, 65280, 1) == n + 31 * -(-n // 65280) + 28
    for bad in (0, -1, 65281, 1 << 20):
        assert bound(100, bad, 1) == 0 and lib.besst_dev_bgzf_deflate_workspace_bytes(100, bad) == 0
    assert bound(-1, 65280, 1) == 0
    # a slot of 64 KiB per block, and room for sizes and offsets
    ws = lib.besst_dev_bgzf_deflate_workspace_bytes
    assert ws(3 * 65280 + 1, 65280) >= 4 * 65536 + 4 * 4 + 5 * 8
    assert ws(100, 16) >= 7 * 65536


def test_argument_errors_do_not_need_a_gpu():
    lib = _lib.load()
    fake = C.c_void_p(4096)                                      # never dereferenced: every call below is refused first
    n, payload = 100000, 65280
    ws = lib.besst_dev_bgzf_deflate_workspace_bytes(n, payload)
    cap = lib.besst_dev_bgzf_deflate_bound(n, payload, 1)

    def call(src=fake, n=n, payload=payload, workspace=fake, ws_bytes=ws, out=fake, out_cap=cap, out_bytes=fake):
        return lib.besst_dev_bgzf_deflate(None, src, n, payload, 1, workspace, ws_bytes, out, out_cap, out_bytes, None)

    for kwargs, word in ((dict(src=None), 'null'), (dict(workspace=None), 'null'), (dict(out=None), 'null'),
                         (dict(out_bytes=None), 'null'), (dict(payload=0), 'block_payload'), (dict(payload=65281), 'block_payload'),
                         (dict(payload=-5), 'block_payload'), (dict(ws_bytes=ws - 1), 'workspace'), (dict(out_cap=cap - 1), 'output'),
                         (dict(n=-1), 'negative')):
        assert call(**kwargs) == 1, kwargs
        assert word in _lib.last_error(), (kwargs, _lib.last_error())
    size = C.c_size_t(0)
    buf = np.zeros(64, dtype=np.uint8)
    assert lib.besst_bgzf_deflate_device(0, _lib.ptr(buf), 64, 0, 1, _lib.ptr(buf), 64, C.byref(size)) == 1
    assert lib.besst_bgzf_deflate_device(0, _lib.ptr(buf), 64, 65280, 1, _lib.ptr(buf), 64, C.byref(size)) == 1      # 64 + 31 + 28 needed
    assert 'output' in _lib.last_error()
    with pytest.raises(ValueError):
        GO.bgzf_compress(b'abc', block_payload=70000)


def test_new_symbols_in_header_library_and_table():
    text = open(os.path.join(REPO, 'include', 'besst_amd.h')).read()
    code = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    lib = _lib.load()
    for name in NEW:
        assert re.search(r'\b%s\s*\(' % name, code), name
        assert hasattr(lib, name) and name in _lib.exported_symbols()
    assert re.search(r'#define\s+BESST_BGZF_BLOCK_PAYLOAD\s+65280\b', text)
    assert lib.besst_abi_version() == 3


def test_the_switch_and_the_command_line():
    assert Parameter.parameter().outputs_bgzf is False
    base = ['-c', 'c.fa', '-f', 'a.bam', '-orientation', 'fr']
    assert cli.build_parser().parse_args(base).bgzf_outputs is False
    assert cli.build_parser().parse_args(base + ['--bgzf_outputs']).bgzf_outputs is True
    with pytest.raises(SystemExit) as exc:
        cli.main(base + ['--bgzf_outputs'])
    assert '--scaffolds' in str(exc.value)
