"""No GPU: the per-record rules of the SAM reader (besst_amd/csrc/sam_core.h) run on the host by
tests/cpp/sam_core_test.cpp - built with the host compiler under AddressSanitizer and UBSan, warnings fail - against the
tests' own decoder (tests/sam_model.py): every handmade line, every error class, numbers at their limits, qlen
saturation, and the reference table with 70 000 names."""
import os
import shutil
import subprocess

import pytest

from tests import sam_design, sam_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAM = os.path.join(ROOT, 'tests', 'golden', 'sam', 'handmade.sam')


def _host_compiler():
    for name in (os.environ.get('CXX'), 'c++', 'g++', 'clang++', '/opt/rocm/llvm/bin/clang++'):
        path = shutil.which(name) if name else None
        if path:
            return path
    raise AssertionError('no host C++ compiler found (set CXX)')


@pytest.fixture(scope='module')
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp('sam_core') / 'sam_core_test')
    src = os.path.join(ROOT, 'tests', 'cpp', 'sam_core_test.cpp')
    built = subprocess.run([_host_compiler(), '-std=c++17', '-O1', '-g', '-Wall', '-Wextra', '-fsanitize=address,undefined',
                            '-fno-sanitize-recover=undefined', src, '-o', exe], capture_output=True, text=True)
    assert built.returncode == 0 and not built.stderr.strip(), built.stderr      # (a warning fails it too)
    return exe


def run(program, tmp_path, names, body, queries=None):
    """-> (the program's record lines, its query rows)"""
    paths = [str(tmp_path / 'names.txt'), str(tmp_path / 'records.sam')]
    with open(paths[0], 'wb') as fh:
        fh.write('\n'.join(names).encode())
    with open(paths[1], 'wb') as fh:
        fh.write(body)
    if queries is not None:
        paths.append(str(tmp_path / 'queries.txt'))
        with open(paths[2], 'wb') as fh:
            fh.write('\n'.join(queries).encode())
    ran = subprocess.run([program] + paths, capture_output=True, text=True, timeout=120)
    assert ran.returncode == 0, (ran.stdout + ran.stderr)[-3000:]
    out = ran.stdout.splitlines()
    assert out[0].startswith('table %d ' % len(names)), out[0]
    return [l for l in out[1:] if not l.startswith('row ')], [int(l.split()[1]) for l in out[1:] if l.startswith('row ')]


def expected(names, body):
    """what the program must print for every line of ``body``, from the model"""
    row_of = {n.encode(): i for i, n in enumerate(names)}
    want = []
    for at, line in sam_model.lines_of(body):
        got = sam_model.decode_record(line, row_of)
        if isinstance(got, int):
            want.append('%d err %d' % (at, got))
        else:
            v, sat = got
            want.append('%d ok %d %d %d %d %d %d %d %d %d %d %d' % (at, v['tid'], v['mtid'], v['pos'], v['mpos'], v['tlen'], v['flag'],
                                                                   v['mapq'], v['qlen'], v['rlen'], v['alen'], int(sat)))
    return want


def test_every_handmade_line(program, tmp_path):
    with open(SAM, 'rb') as fh:
        data = fh.read()
    model = sam_model.decode(data)
    body = data[model['header_bytes']:]
    for form in (body, body.replace(b'\n', b'\r\n'), body[:-1]):
        got, _ = run(program, tmp_path, model['references'], form)
        assert got == expected(model['references'], form)
        assert len(got) == 15 and all(' ok ' in l for l in got)


def test_error_classes_limits_and_saturation(program, tmp_path):
    lines = [l for _, l, _ in sam_design.ERROR_LINES] + [l for _, l, _ in sam_design.LIMIT_LINES]
    body = '\n'.join(lines).encode()                             # (no final newline: the last line ends with the file)
    got, _ = run(program, tmp_path, sam_design.REFS, body)
    want = expected(sam_design.REFS, body)
    assert got == want
    n_err = len(sam_design.ERROR_LINES)
    for (name, _, code), line in zip(sam_design.ERROR_LINES, got):
        assert line.endswith(' err %d' % code), (name, line)
    for (name, _, readable), line in zip(sam_design.LIMIT_LINES, got[n_err:]):
        assert (' ok ' in line) == readable, (name, line)
    by_name = dict(zip((n for n, _, _ in sam_design.LIMIT_LINES), got[n_err:]))
    assert by_name['qlen_saturates'].split()[9:] == ['65535', '0', '70000', '1']       # qlen rlen alen saturated
    assert by_name['qlen_65535'].split()[9:] == ['65535', '0', '65535', '0']
    assert by_name['qlen_65536'].split()[9:] == ['65535', '0', '65536', '1']
    assert by_name['clips_only'].split()[9] == '0'               # 4 - 3 - 2 < 0: floored
    assert by_name['tlen_int32_min'].split()[6] == '-2147483648'
    assert by_name['pos_0'].split()[4] == '-1'


def test_reference_table_of_70000_names(program, tmp_path):
    names, absent = sam_design.reference_names(70000)
    probe = ['ctg1', 'ctg10', 'ctg100', 'scaffold_0000A', 'scaffold_0000B', 'c', 'N' * 200, 'N' * 199 + 'M', 'ctg', 'ctg69993']
    body = '\n'.join(sam_design.GOOD_LINE.replace('ctg1', n, 1).replace('=', m, 1)
                     for n, m in zip(probe + absent[:2], probe[::-1] + ['=', absent[2]])).encode() + b'\n'
    got, rows = run(program, tmp_path, names, body, queries=names[::7] + absent + probe)
    assert got == expected(names, body)
    assert got[-2].endswith(' err 9') and got[-1].endswith(' err 9')
    index = {n: i for i, n in enumerate(names)}
    assert rows == [index.get(q, -1) for q in names[::7] + absent + probe]
    assert rows[len(names[::7]):len(names[::7]) + len(absent)] == [-1] * len(absent)


def test_a_repeated_name_is_reported(program, tmp_path):
    paths = [str(tmp_path / 'names.txt'), str(tmp_path / 'records.sam')]
    with open(paths[0], 'wb') as fh:
        fh.write(b'a\nb\nab\nb')
    open(paths[1], 'wb').close()
    ran = subprocess.run([program] + paths, capture_output=True, text=True, timeout=60)
    assert ran.returncode == 0 and ran.stdout.strip() == 'duplicate 3'
