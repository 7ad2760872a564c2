"""No GPU: the streamed SAM reader's model and designed files (tests/sam_stream_model.py, tests/sam_stream_design.py) and the
line cutter's sequential rule (besst_amd/csrc/sam_lines_core.h), run lane after lane by tests/cpp/sam_lines_core_test.cpp -
built with the host compiler under AddressSanitizer and UBSan, warnings fail - against the model's cutter."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import bgzf_writer, sam_model, sam_stream_design, sam_stream_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _host_compiler():
    for name in (os.environ.get('CXX'), 'c++', 'g++', 'clang++', '/opt/rocm/llvm/bin/clang++'):
        path = shutil.which(name) if name else None
        if path:
            return path
    raise AssertionError('no host C++ compiler found (set CXX)')


@pytest.fixture(scope='module')
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp('sam_lines_core') / 'sam_lines_core_test')
    src = os.path.join(ROOT, 'tests', 'cpp', 'sam_lines_core_test.cpp')
    built = subprocess.run([_host_compiler(), '-std=c++17', '-O1', '-g', '-Wall', '-Wextra', '-fsanitize=address,undefined',
                            '-fno-sanitize-recover=undefined', src, '-o', exe], capture_output=True, text=True)
    assert built.returncode == 0 and not built.stderr.strip(), built.stderr      # (a warning fails it too)
    return exe


@pytest.fixture(scope='module')
def cases():
    return sam_stream_design.designed_files()


def test_the_model_cutter_on_plain_cases():
    cut = sam_stream_model.cutter
    assert cut(b'') == [0, -1, 0, 0] and cut(b'', True) == [0, -1, 0, 0]
    assert cut(b'@a\n@b\n', True) == [6, 6, 0, 0] and cut(b'@a\n@b', True) == [3, -1, 0, 0]
    assert cut(b'@a\nr1\nr2', True, 4) == [6, 3, 1, 0] and cut(b'r1\n', True, 3) == [3, 0, 1, 0]
    assert cut(b'@a\n\n@b\n', True) == [7, 3, 0, 0]            # an empty line is no header line
    assert cut(b'@a\nr1\n', False) == [6, -1, 0, 0]


def test_the_core_lane_after_lane_is_the_model(program, tmp_path):
    for name, text, queries in sam_stream_design.cutter_cases():
        path = str(tmp_path / (name + '.bin'))
        with open(path, 'wb') as fh:
            fh.write(text)
        args = [str(v) for q in queries for v in q]
        ran = subprocess.run([program, path] + args, capture_output=True, text=True, timeout=120)
        assert ran.returncode == 0, (name, (ran.stdout + ran.stderr)[-3000:])
        got = [[int(v) for v in line.split()] for line in ran.stdout.splitlines()]
        want = [sam_stream_model.cutter(text[:n], bool(w), upto) for n, w, upto in queries]
        assert got == want, (name, [(q, g, w) for q, g, w in zip(queries, got, want) if g != w][:5])


def test_the_core_on_a_designed_text_at_every_round(program, cases, tmp_path):
    """the buffers the reader hands the cutter for the hand-cut file: every round's bytes, header rounds with the header's
    end asked for"""
    case = next(c for c in cases if c['name'] == 'hand_cut')
    plan = sam_stream_model.rounds(case['isizes'], case['text'], sam_stream_design.CHUNK)
    for k, r in enumerate(plan.rounds):
        buf = case['text'][r['text_at']:r['text_at'] + r['held']]
        path = str(tmp_path / ('round%d.bin' % k))
        with open(path, 'wb') as fh:
            fh.write(buf)
        want_header = 1 if r['kind'] == 'header' else 0
        ran = subprocess.run([program, path, str(len(buf)), str(want_header), str(len(buf) // 2)], capture_output=True, text=True,
                             timeout=120)
        assert ran.returncode == 0, (ran.stdout + ran.stderr)[-3000:]
        assert [int(v) for v in ran.stdout.split()] == sam_stream_model.cutter(buf, bool(want_header), len(buf) // 2)


def test_every_border_case_is_in_the_designed_files(cases):
    plans = sam_stream_design.census(cases)
    for case in cases:
        blocks, end, bad = bgzf_writer.walk(case['data'])
        assert not bad and end == len(case['data']) and [b[4] for b in blocks] == case['isizes'], case['name']
        assert bgzf_writer.host_inflate(case['data'])[0] == case['text']
        plan = plans[case['name']]
        if isinstance(plan, sam_stream_model.LineTooLong):
            continue
        if not case.get('header_only'):
            assert len(plan.pushes) > 1, case['name']
            model = sam_model.decode(case['text'])
            assert plan.header_bytes == model['header_bytes'], case['name']
            # every push begins at a line start and - but for the last - ends at a line end
            starts = set(model['offsets'])
            assert all(at in starts for at, _ in plan.pushes), case['name']
            assert all(case['text'][at + n - 1:at + n] == b'\n' for at, n in plan.pushes[:-1]), case['name']
        for r in plan.rounds:
            assert r['held'] < sam_stream_design.CHUNK + 65536 and (r['n_blocks'] > 0 or r['carry_in'] >= sam_stream_design.CHUNK)


def test_the_model_follows_the_pinned_rule_on_a_small_example():
    # chunk 10: blocks of 4 bytes; the header '@h\n' ends inside the first round, the records start the next buffer
    text = b'@h\nab\ncdefgh\nij\nk'
    isizes = [4, 4, 4, 4, 1, 0]
    plan = sam_stream_model.rounds(isizes, text, 10)
    assert [(r['kind'], r['carry_in'], r['held'], r['take'], r['carry_out'], r['n_blocks']) for r in plan.rounds] == [
        ('header', 0, 12, 3, 9, 3), ('records', 9, 13, 13, 0, 1), ('records', 0, 1, 1, 0, 2)]
    assert plan.pushes == [(3, 13), (16, 1)] and plan.header_bytes == 3
    with pytest.raises(sam_stream_model.LineTooLong) as err:
        sam_stream_model.rounds([4] * 5, b'ab\n' + b'x' * 17, 10)
    assert err.value.offset == 3
    assert np.sum(isizes) == len(text)
