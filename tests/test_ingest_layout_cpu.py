"""No GPU: the entry points that report what a device ingest left beside the record columns (besst_ctx_layout_state /
besst_ctx_fetch_layout) are bound and answer argument errors, and the per-lane rules of the ingest's layout step
(besst_amd/csrc/ingest_layout_core.h) - run on the host by tests/cpp/ingest_layout_core_test.cpp, lane after lane, the way
the kernels use them - give the planes, the offsets and the entry order of the numpy statement in
tests/test_candidate_stream.py.  The cases put a 16 384-record border inside a BGZF block, on a block's first record, on a
chunk's first record and inside a stretch of blocks no record begins in; records resident before the call end inside a
plane byte and inside a block."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import test_candidate_stream as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BLOCK = M.BLOCK


def test_entry_points_are_bound():
    from besst_amd import _lib
    lib = _lib.load()
    for name in ('besst_ctx_layout_state', 'besst_ctx_fetch_layout'):
        assert name in _lib._SIGNATURES and getattr(lib, name) is not None


def test_null_context_is_an_argument_error():
    from besst_amd import _lib
    lib = _lib.load()
    out = np.zeros(8, dtype=np.int64)
    assert lib.besst_ctx_layout_state(None, _lib.ptr(out)) == 1
    assert 'layout_state' in _lib.last_error()
    assert lib.besst_ctx_fetch_layout(None, *([None] * 10)) == 1
    assert 'fetch_layout' in _lib.last_error()


def _host_compiler():
    for name in (os.environ.get('CXX'), 'c++', 'g++', 'clang++', '/opt/rocm/llvm/bin/clang++'):
        path = shutil.which(name) if name else None
        if path:
            return path
    raise AssertionError('no host C++ compiler found (set CXX)')


@pytest.fixture(scope='module')
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp('layout_core') / 'ingest_layout_core_test')
    src = os.path.join(ROOT, 'tests', 'cpp', 'ingest_layout_core_test.cpp')
    built = subprocess.run([_host_compiler(), '-std=c++17', '-O1', '-g', '-Wall', '-Wextra', '-fsanitize=address,undefined',
                            '-fno-sanitize-recover=undefined', src, '-o', exe], capture_output=True, text=True)
    assert built.returncode == 0 and not built.stderr.strip(), built.stderr      # (a warning fails it too)
    return exe


def _counts(total, sizes):
    """Block counts that add up to `total`, cycling through `sizes`."""
    out, left, k = [], total, 0
    while left > 0:
        c = min(left, sizes[k % len(sizes)])
        out.append(c)
        left -= c
        k += 1
    return out


def _cases():
    # (name, resident records, block counts, first block of every chunk)
    inside = _counts(2 * BLOCK + 777, [300])                 # 16384 = 54 * 300 + 184: inside a block
    yield 'border_inside_a_block', 0, inside, list(range(0, len(inside), 7))
    first = _counts(2 * BLOCK + 100, [256])                  # every border is a block's first record, chunks of 9 blocks: no seam there
    yield 'border_on_a_blocks_first_record', 0, first, list(range(0, len(first), 9))
    seam = _counts(2 * BLOCK + 100, [256])                   # chunks of 64 blocks = 16384 records: every border is a chunk's first record
    yield 'border_on_a_chunk_seam', 0, seam, list(range(0, len(seam), 64))
    holes = []
    for c in _counts(BLOCK, [100]) + _counts(BLOCK + 50, [100]):
        holes += [c, 0, 0]                                   # two blocks without a record start behind every block,
    at = len(_counts(BLOCK, [100])) * 3                      # the border's block behind such a stretch - and first in its chunk
    yield 'border_behind_blocks_without_a_start', 0, holes, sorted({0, 5, at - 2, at + 7})
    late = _counts(BLOCK + 5000, [31, 1, 64, 33, 0, 2048, 500])
    yield 'resident_records_end_inside_a_byte', BLOCK - 3000 - 5, late, list(range(0, len(late), 4))
    yield 'resident_records_end_on_a_border', BLOCK, _counts(BLOCK + 1, [777]), [0, 1, 2]
    yield 'fewer_than_64_records', 0, [7, 0, 30, 1], [0, 2]


@pytest.mark.parametrize('case', list(_cases()), ids=lambda c: c[0])
def test_core_against_the_numpy_model(case, program, tmp_path):
    name, n_res, counts, chunks = case
    n_new = int(sum(counts))
    total, n_refs = n_res + n_new, 40
    rec = M.random_records(total, n_refs, seed=len(name) + n_res)
    want = M.compact(rec, n_refs)
    mate = np.packbits(rec['tid'] != rec['mtid'], bitorder='little')
    runs = np.packbits(np.r_[True, rec['tid'][1:] != rec['tid'][:-1]], bitorder='little')
    path = str(tmp_path / (name + '.case'))
    with open(path, 'wb') as fh:
        np.array([n_res, n_new, n_refs, len(counts), len(chunks)], dtype=np.int64).tofile(fh)
        np.array(counts, dtype=np.uint32).tofile(fh)
        np.array(chunks, dtype=np.uint32).tofile(fh)
        rec['tid'].astype(np.int32).tofile(fh)
        rec['mtid'].astype(np.int32).tofile(fh)
        rec['flag'].astype(np.uint32).tofile(fh)
        for plane in (mate, runs, want['set_bits']):
            assert plane.shape[0] == (total + 7) // 8
            plane.tofile(fh)
        want['offsets'].astype(np.uint32).tofile(fh)
    ran = subprocess.run([program, path], capture_output=True, text=True, timeout=120)
    assert ran.returncode == 0, (ran.stdout + ran.stderr)[-3000:]
    assert ran.stdout.startswith('ok: %d + %d records' % (n_res, n_new))
