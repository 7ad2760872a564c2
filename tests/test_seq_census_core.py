"""No GPU: the census record and its merge rule (besst_amd/csrc/seq_census_core.h) run on the host by
tests/cpp/seq_census_core_test.cpp - built with the host compiler under AddressSanitizer and UBSan, warnings fail - against
the tests' own model (tests/seq_census_model.py): the class of every byte value, every designed stream walked in windows
of several sizes, and a table that is out of order."""
import os
import shutil
import subprocess

import pytest

from tests import seq_census_design as D
from tests import seq_census_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = 1024                                  # the rule knows no tile: a small one keeps the model's byte loops short


def _host_compiler():
    for name in (os.environ.get('CXX'), 'c++', 'g++', 'clang++', '/opt/rocm/llvm/bin/clang++'):
        path = shutil.which(name) if name else None
        if path:
            return path
    raise AssertionError('no host C++ compiler found (set CXX)')


@pytest.fixture(scope='module')
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp('seq_census_core') / 'seq_census_core_test')
    src = os.path.join(ROOT, 'tests', 'cpp', 'seq_census_core_test.cpp')
    built = subprocess.run([_host_compiler(), '-std=c++17', '-O1', '-g', '-Wall', '-Wextra', '-fsanitize=address,undefined',
                            '-fno-sanitize-recover=undefined', src, '-o', exe], capture_output=True, text=True)
    assert built.returncode == 0 and not built.stderr.strip(), built.stderr      # (a warning fails it too)
    return exe


def run(program, tmp_path, stream, seq_off, seq_len, min_gap, window):
    """-> (partial rows, finalised rows, first row out of order)"""
    paths = [str(tmp_path / 'stream.bin'), str(tmp_path / 'table.txt')]
    with open(paths[0], 'wb') as fh:
        fh.write(stream)
    with open(paths[1], 'w') as fh:
        fh.write(''.join('%d %d\n' % row for row in zip(seq_off, seq_len)))
    ran = subprocess.run([program] + paths + [str(min_gap), str(window)], capture_output=True, text=True, timeout=120)
    assert ran.returncode == 0, (ran.stdout + ran.stderr)[-3000:]
    part, final, order = [], [], None
    for line in ran.stdout.splitlines():
        f = line.split()
        if f[0] == 'order':
            order = int(f[1])
        else:
            (part if f[0] == 'part' else final).append([int(v) for v in f[2:]])
    return part, final, order


def test_the_class_of_every_byte_value(program):
    ran = subprocess.run([program, 'classes'], capture_output=True, text=True, timeout=60)
    assert ran.returncode == 0, ran.stderr[-3000:]
    got = [tuple(int(v) for v in line.split()[1:]) for line in ran.stdout.splitlines()]
    assert got == [(b, M.CLASS[b], int(0x61 <= b <= 0x7A)) for b in range(256)]
    assert sum(1 for b in range(256) if M.CLASS[b] != M.OTHER) == 31          # 5 x 2 + 10 x 2 + X


@pytest.mark.parametrize('design', D.all_designs(T), ids=lambda d: d['name'])
def test_designs_in_windows(program, tmp_path, design):
    stream, off, length = design['stream'], design['seq_off'], design['seq_len']
    for min_gap, window in ((1, len(stream) + 1), (1, 1), (2, 7), (3, T), (10 ** 6, T // 2 + 3)):
        part, final, order = run(program, tmp_path, stream, off, length, min_gap, window)
        assert order == -1
        assert part == M.table(stream, off, length, min_gap), (design['name'], min_gap, window)
        assert final == [M.whole(stream[o:o + n], min_gap) for o, n in zip(off, length)]


def test_a_table_out_of_order_is_named(program, tmp_path):
    for off, length, want in (([0, 10, 5], [3, 3, 3], 2), ([0, 4], [5, 1], 1), ([0, 5, 5], [5, 0, 2], -1), ([0, 3], [-1, 2], 0)):
        _, _, order = run(program, tmp_path, b'ACGTNACGTNACGTN', off, length, 1, 4)
        assert order == want
