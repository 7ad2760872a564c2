"""The BGZF compressor on the device (csrc/bgzf_deflate.hip) through its host hook, besst_bgzf_deflate_device: every file
it writes goes through the validator of tests/bgzf_util.py (each block inflated ALONE by zlib, BSIZE, CRC-32, ISIZE, full
blocks, one EOF block), through gzip.decompress, and back through this project's own inflate in both its forms; a second
call gives the same bytes; a block is at most payload + 31 bytes; and nucleotide text of a full block or more is no larger
than zlib level 1 makes the same blocks."""
import gzip
import random

import numpy as np
import pytest

from besst_amd import GenerateOutput as GO
from besst_amd import bamio
from tests import bgzf_util as BU

pytestmark = pytest.mark.gpu

FULL = 65280
SMALL = (16, 255, 256, 257, 4096)
ACGT = np.frombuffer(b'ACGT', dtype=np.uint8)


def acgt(n, seed):
    return ACGT[np.random.default_rng(seed).integers(0, 4, n)].tobytes()


def lane_span(payload):
    """bytes per lane of a full block (csrc/bgzf_deflate_core.h: span_of)"""
    return (-(-payload // 256) + 3) // 4 * 4


def check(raw, payload, monkeypatch, nucleotide=False, stored=None):
    raw = bytes(raw)
    data = GO.bgzf_compress(raw, block_payload=payload)
    got, sizes = BU.validate(data, payload)
    assert got == raw
    assert gzip.decompress(data) == raw
    n_blocks = -(-len(raw) // payload)
    assert len(sizes) == n_blocks
    for k, size in enumerate(sizes):
        assert size <= min(payload, len(raw) - k * payload) + 31, (k, size)
    if stored is not None:
        assert [s == min(payload, len(raw) - k * payload) + 31 for k, s in enumerate(sizes)] == [stored] * n_blocks
    assert GO.bgzf_compress(raw, block_payload=payload) == data, 'a second call gave other bytes'
    assert GO.bgzf_compress(raw, block_payload=payload, eof=False) == data[:-28]
    for form in ('second', 'first'):
        if form == 'first':
            monkeypatch.setenv('BESST_INFLATE', '1')
        else:
            monkeypatch.delenv('BESST_INFLATE', raising=False)
        assert bamio.inflate_bgzf_device(data, out_cap=len(raw) + 64) == raw, form
    monkeypatch.delenv('BESST_INFLATE', raising=False)
    if nucleotide and payload == FULL and len(raw) >= FULL:
        size, bar = len(data) - 28, BU.yardstick(raw, payload)
        print('payload of %d bytes: %d bytes, zlib level 1 %d' % (len(raw), size, bar))
        assert size <= bar
    return data


def test_nothing():
    assert GO.bgzf_compress(b'') == BU.EOF
    assert GO.bgzf_compress(b'', eof=False) == b''
    assert GO.bgzf_compress(b'', block_payload=16) == BU.EOF


@pytest.mark.parametrize('payload', (FULL,) + SMALL)
def test_lengths_around_nothing_and_around_a_block(payload, monkeypatch):
    text = acgt(2 * payload + 1, payload)
    for n in (1, 2, 3, 4, 5, payload - 1, payload, payload + 1, 2 * payload, 2 * payload + 1):
        check(text[:n], payload, monkeypatch, nucleotide=True)
        check(b'N' * n, payload, monkeypatch)                                    # one distinct byte (a whole block of it)
        check(bytes(bytearray(b'AN'[(i // 3) & 1] for i in range(n))), payload, monkeypatch)      # two


RUNS = list(range(2, 7)) + list(range(257, 264)) + list(range(515, 521))


@pytest.mark.parametrize('mode', ['starts', 'ends', 'straddles'])
@pytest.mark.parametrize('payload', SMALL + (FULL,))
def test_runs_on_the_borders_of_blocks_and_lane_spans(payload, mode, monkeypatch):
    """every run length, placed so that it starts exactly at / ends exactly at / lies across every border - of blocks and
    of the kernel's lane spans -, and the same one byte to either side"""
    span = lane_span(payload)
    borders = [payload, 2 * payload, span, 2 * span, payload + span, 2 * payload + 3 * span]
    n = 3 * payload + 1200
    for run in RUNS:
        back = {'starts': 0, 'ends': run, 'straddles': run // 2}[mode]
        for shift in (0, -1, 1):
            text = bytearray(acgt(n, run))
            for border in borders:
                begin = border + shift - back
                if begin >= 0:
                    text[begin:begin + run] = b'N' * run
            text = bytes(text[:n])
            if shift == 0 and mode == 'starts':
                assert all(text[b:b + run] == b'N' * run for b in borders)
            if shift == 0 and mode == 'ends':
                assert all(text[b - run:b] == b'N' * run for b in borders if b >= run)
            check(text, payload, monkeypatch, nucleotide=True)


def test_scaffold_text_and_random_acgt(monkeypatch):
    check(acgt(3 * FULL + 77, 3), FULL, monkeypatch, nucleotide=True)
    text = BU.scaffold_text(1 << 20, seed=2)
    assert b'>scaffold_' in text and b'NNNN' in text and b'n' in text
    check(text, FULL, monkeypatch, nucleotide=True)
    for payload in SMALL:
        check(text[:5 * payload + 3], payload, monkeypatch)


@pytest.mark.parametrize('payload', (FULL,) + SMALL)
def test_random_bytes_are_stored(payload, monkeypatch):
    raw = np.random.default_rng(9).integers(0, 256, 70000 if payload == FULL else 4 * payload, dtype=np.uint8).tobytes()
    check(raw, payload, monkeypatch, stored=True if payload >= 255 else None)      # (16 random bytes may repeat one)


def test_fibonacci_counts_force_the_length_limit(monkeypatch):
    counts, a, b = [], 1, 1
    for _ in range(22):                                          # the unlimited Huffman tree of these is 21 deep
        counts.append(a)
        a, b = b, a + b
    symbols = b''.join(bytes([65 + k]) * c for k, c in enumerate(counts))
    assert len(symbols) <= FULL
    check(symbols, FULL, monkeypatch)                            # sorted: runs
    shuffled = bytearray(symbols)
    random.Random(4).shuffle(shuffled)
    data = check(bytes(shuffled), FULL, monkeypatch)
    assert len(data) < len(symbols) // 2                         # (not stored: the limited code was used)


def seeded_payload(k):
    rng = np.random.default_rng(1000 + k)
    alphabet = int(rng.integers(1, 257))
    payload = ((FULL,) + SMALL)[k % 6]
    n = int(rng.integers(1, 3 * payload + 1))
    shape = k % 4
    if shape == 0:
        p = np.ones(alphabet)
    elif shape == 1:
        p = 0.5 ** np.arange(alphabet)
    elif shape == 2:
        p = 1.0 / np.arange(1, alphabet + 1)
    else:
        p = 0.618 ** np.arange(alphabet)                         # Fibonacci-like counts: the deepest trees
    p = np.maximum(p, 1e-300)
    symbols = rng.permutation(256)[:alphabet].astype(np.uint8)
    return symbols[rng.choice(alphabet, size=n, p=p / p.sum())].tobytes(), payload


@pytest.mark.parametrize('group', range(6))
def test_seeded_payloads(group, monkeypatch):
    """300 payloads: alphabets of 1..256 symbols; uniform, geometric, Zipf and Fibonacci-like frequencies; up to 3 blocks"""
    for k in range(50 * group, 50 * group + 50):
        raw, payload = seeded_payload(k)
        check(raw, payload, monkeypatch)


def test_64_mib_of_scaffold_text(monkeypatch):
    """several thousand blocks in one call: the offsets are 64-bit, the grid is large"""
    raw = BU.scaffold_text(64 << 20, seed=3)
    data = GO.bgzf_compress(raw)
    got, sizes = BU.validate(data)
    assert got == raw and len(sizes) == -(-len(raw) // FULL) > 1000
    assert max(sizes) <= FULL + 31
    assert GO.bgzf_compress(raw) == data
    for form in ('second', 'first'):
        if form == 'first':
            monkeypatch.setenv('BESST_INFLATE', '1')
        assert bamio.inflate_bgzf_device(data, out_cap=len(raw) + 64) == raw, form
    size, bar = len(data) - 28, BU.yardstick(raw)
    print('64 MiB: %d bytes, zlib level 1 %d' % (size, bar))
    assert size <= bar
