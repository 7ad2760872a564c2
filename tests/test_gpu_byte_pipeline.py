"""GenerateOutput.write_chunks alone: the pipeline every device-produced file goes through, without the emit kernels.  The
source fills its ranges with a pattern by torch ops on the stream it is given; block payload and chunk size are shrunk so
that 2305 bytes are four chunks and both slots of the buffers are used twice."""
import gzip
import io

import pytest

from besst_amd import GenerateOutput as GO
from tests import bgzf_util as BU

pytestmark = pytest.mark.gpu

PAYLOAD = 256
CHUNK = 3 * PAYLOAD + 100                                        # deflated: chunks of three blocks (768 bytes)
TOTALS = (0, 1, 767, 768, 769, 1536, 2305)


@pytest.fixture(autouse=True)
def small_blocks(monkeypatch):
    monkeypatch.setattr(GO, 'BGZF_BLOCK_PAYLOAD', PAYLOAD)
    monkeypatch.setattr(GO, 'CHUNK_BYTES', CHUNK)


def pattern(begin, end):
    return bytes((i * 131) % 251 for i in range(begin, end))


class PatternSource(object):
    """byte i of the file is (i * 131) % 251"""

    def __init__(self, total):
        import torch
        self.torch, self.dev, self.total = torch, torch.device('cuda', 0), total
        self.ranges, self.checks = [], 0

    def emit(self, begin, end, out, stream):
        torch = self.torch
        self.ranges.append((begin, end))
        with torch.cuda.stream(stream):
            out[:end - begin] = ((torch.arange(begin, end, device=self.dev) * 131) % 251).to(torch.uint8)

    def check(self):
        self.torch.cuda.synchronize(self.dev)
        self.checks += 1


def run(total, deflate, step, path=None):
    """-> the bytes write_chunks wrote into a BytesIO (``path``: into that file), after the checks every run has to pass"""
    src = PatternSource(total)
    if path is None:
        fh = io.BytesIO()
        spent = GO.write_chunks(src, fh, GO.CHUNK_BYTES, deflate)
        data = fh.getvalue()
    else:
        spent = GO.write_file(src, str(path), GO.CHUNK_BYTES, deflate)
        with open(str(path), 'rb') as fh:
            data = fh.read()
    assert src.checks == 1
    assert all(end > begin for begin, end in src.ranges)
    assert src.ranges == [(b, min(total, b + step)) for b in range(0, total, step)]
    assert spent['file_bytes'] == len(data)
    assert sorted(spent) == ['bgzf_kernels', 'd2h', 'emit_kernels', 'file_bytes', 'file_write']
    return data


@pytest.mark.parametrize('total', TOTALS)
def test_plain(total, tmp_path):
    want = pattern(0, total)
    assert run(total, False, CHUNK) == want
    assert run(total, False, CHUNK, tmp_path / 'plain.bin') == want


@pytest.mark.parametrize('total', TOTALS)
def test_deflated(total, tmp_path):
    want = pattern(0, total)
    data = run(total, True, 3 * PAYLOAD)
    text, sizes = BU.validate(data, PAYLOAD)
    assert text == want and len(sizes) == -(-total // PAYLOAD)
    assert gzip.decompress(data) == want
    assert data == GO.bgzf_compress(want, block_payload=PAYLOAD)
    if total == 0:
        assert data == GO.bgzf_compress(b'')
    assert run(total, True, 3 * PAYLOAD, tmp_path / 'deflated.bin') == data
