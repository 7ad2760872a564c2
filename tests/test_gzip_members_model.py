"""CPU checks of the parallel inflate of a gzip file of several members: the model
(tests/gzip_members_model.py) against ``gzip.decompress`` and the host path's reader on the designed files
(tests/gzip_members_design.py) at every chunk size, a census that each file holds its border, the host-compiled steps of
the kernels (besst_amd/csrc/gzip_stream_core.h) run by tests/cpp/gzip_members_core_test.cpp against zlib on the same files -
their numbers must be the model's -, once more under the address and undefined-behaviour sanitizers, and the new entry points'
argument checks."""
import ctypes as C
import gzip
import io
import os
import re
import shutil
import struct
import subprocess

import pytest

from besst_amd import GenerateOutput as GO
from besst_amd import _lib
from tests import gzip_members_design as G
from tests import gzip_members_model as MM
from tests import gzip_stream_design as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = sorted(G.files())


def host_text(data):
    return b''.join(GO._gzip_members(io.BytesIO(data)))


@pytest.mark.parametrize('name', NAMES)
def test_model_against_zlib(name):
    data, text, _fasta = G.files()[name]
    assert gzip.decompress(data) == text == host_text(data)
    members = None
    for chunk in G.CHUNKS:
        res = G.modelled(name, chunk)
        assert res['status'] == 'ok' and res['text'] == text, chunk
        assert res['member_candidates'] >= res['members'] - 1 >= 1, chunk
        assert res['live'] >= res['members'] and res['bad_member'] is None
        table = res['member_table']
        assert [m['at'] for m in table] == sorted(m['at'] for m in table) and table[0]['at'] == 0
        assert sum(m['bytes'] for m in table) == len(text) and table[-1]['trailer'] + 8 == len(data)
        members = members or [(m['at'], m['bytes']) for m in table]
        assert members == [(m['at'], m['bytes']) for m in table]            # the members do not depend on the chunk size
        assert res['chunks'] == max(1, -(-(len(data) - 8 - table[0]['data']) // chunk))


def test_census():
    """every file holds the border it was built for"""
    many = G.file_model('plain_then_bgzf_256')
    assert G.modelled('plain_then_bgzf_256', 65536)['members'] == 326 and G.modelled('plain_then_bgzf_4096', 1024)['members'] == 23
    c = many.census(65536)
    assert c['result']['chunks'] == 1 and c['result']['live'] == 326 > c['result']['chunks']     # more live segments than chunks
    assert list(c['starts_per_chunk'].values()) == [325]                      # all of them begin in one chunk
    c = many.census(1024)
    assert max(c['starts_per_chunk'].values()) >= 7 and c['result']['live'] > c['result']['chunks']
    # a dropped false candidate of each kind: in a header, in a stored block's payload, in Huffman-coded data
    assert [len(v) for v in G.file_model('fextra_holds_member').census(1024)['dropped'].values()] == [1]
    assert list(G.file_model('fextra_holds_member').census(1024)['dropped']) == ['header']
    assert len(G.file_model('fname_flagged_false_start').census(1024)['dropped']['header']) == 1
    assert G.file_model('fname_false_start').census(1024)['dropped'] == {}     # ('x' as FLG has reserved bits: never a candidate)
    stored = G.file_model('stored_holds_member').census(1024)
    assert len(stored['dropped']['stored']) == 2 and stored['result']['members'] == 2
    codes = G.file_model('magic_in_codes').census(1024)
    assert len(codes['dropped']['codes']) == 1 and codes['result']['members'] == 3
    for name in NAMES:                                                        # and nothing is dropped anywhere else
        if name not in ('fextra_holds_member', 'fname_flagged_false_start', 'stored_holds_member', 'magic_in_codes'):
            assert G.file_model(name).census(256)['dropped'] == {}, name
    # a member border on, one byte in front of and one byte behind a chunk border of every size; a header across one
    for chunk in G.CHUNKS:
        assert 0 in G.file_model('border_on').census(chunk)['border_offsets']
        assert chunk - 1 in G.file_model('border_before').census(chunk)['border_offsets']
        assert 1 in G.file_model('border_behind').census(chunk)['border_offsets']
        for name in ('border_before', 'border_straddled'):
            assert any(m['at'] == 10 + G.BORDER + (-1 if name == 'border_before' else -5)
                       for m in G.file_model(name).census(chunk)['straddled']), (name, chunk)
    # empty members at the front, doubled in the middle, at the end, and alone
    for name, sizes in (('empty_front', 0), ('empty_end', -1)):
        assert G.modelled(name, 1024)['member_table'][sizes]['bytes'] == 0
    middle = [m['bytes'] for m in G.modelled('empty_middle', 1024)['member_table']]
    assert middle[1:3] == [0, 0] and middle[0] and middle[3]
    assert [m['bytes'] for m in G.modelled('empty_only', 256)['member_table']] == [0, 0, 0]
    # first blocks: dynamic, stored, fixed, dynamic
    fm = G.file_model('first_blocks')
    kinds = [fm.s.block(8 * (m['data'] - fm.data_off))[2] for m in G.modelled('first_blocks', 1024)['member_table']]
    assert kinds == [2, 0, 1, 2]


def test_reach():
    """a match may reach its member's first byte and not one further - and the input tells the two rules apart"""
    data, text, _ = G.files()['reach_ok']
    assert text[-259:] == b'A' * 259
    for chunk in G.CHUNKS:
        table = G.modelled('reach_ok', chunk)['member_table']
        assert table[1]['bytes'] == 259 and G.modelled('reach_ok', chunk)['status'] == 'ok'
    bad, at = G.reach_bad()
    assert at == 33781
    with pytest.raises(GO.FastaError, match='invalid distance too far back') as err:
        host_text(bad)
    assert err.value.offset == at
    fm = MM.FileModel(bad)
    for chunk in G.CHUNKS:
        res = fm.inflate(chunk)
        assert (res['status'], res['members']) == ('bad_distance', 2), chunk
        whole = fm.inflate(chunk, whole_text_rule=True)                       # the rule of a one-member decoder takes the file
        assert whole['status'] == 'ok' and whole['text'][-258:] == whole['text'][-259:-258] * 258, chunk


@pytest.mark.parametrize('how', G.DAMAGE)
def test_damage_in_the_model(how):
    data, status, at = G.damaged()[how]
    with pytest.raises(GO.FastaError) as err:
        host_text(data)
    assert err.value.offset == at
    for chunk in G.CHUNKS:
        res = MM.FileModel(data).inflate(chunk)
        assert res['status'] != 'ok' and (status is None or res['status'] == status), chunk
        assert res['bad_member_offset'] == at, chunk


def test_capacity_in_the_model():
    fm = G.file_model('plain_then_bgzf_256')
    n = len(fm.marks)
    assert n == 325 and fm.inflate(1024, member_cap=n)['status'] == 'ok'
    assert fm.inflate(1024, member_cap=n - 2)['status'] == 'too_many_members'
    assert GO.gzip_member_capacity(1 << 20) == 4096 + 4096 and n < GO.gzip_member_capacity(len(fm.data))


def test_header_parse_is_the_package_s():
    for name, (member, _text, head) in D.header_variants().items():
        assert MM.member_data_offset(member, 0) == head == GO.gzip_header_bytes(member[:GO.GZIP_HEADER_ROOM]), name
        assert MM.member_data_offset(b'junk' + member, 4) == 4 + head
        assert MM.member_data_offset(member[:head + 7], 0) is None             # no room for the trailer
    long_name = b'\x1f\x8b\x08\x08\0\0\0\0\0\x03' + b'n' * MM.HEADER_FIELD_LIMIT + b'\0' + b'\x03\0' + b'\0' * 8
    assert MM.member_data_offset(long_name, 0) is None
    assert MM.member_data_offset(long_name[:10] + long_name[11:], 0) == 10 + MM.HEADER_FIELD_LIMIT


def _host_compiler():
    for name in (os.environ.get('CXX'), 'c++', 'g++', 'clang++', '/opt/rocm/llvm/bin/clang++'):
        path = shutil.which(name) if name else None
        if path:
            return path
    raise AssertionError('no host C++ compiler found (set CXX)')


def _files_binary(path):
    bad, _at = G.reach_bad()
    with open(path, 'wb') as fh:
        for name, data in ([(n, G.files()[n][0]) for n in NAMES] + [('reach_bad', bad)] +
                           [(how, G.damaged()[how][0]) for how in G.DAMAGE]):
            fh.write(name.encode('ascii').ljust(64, b'\0') + struct.pack('<Q', len(data)) + data)
    return path


LINE = re.compile(r'^(\S+)\s+chunk\s+(\d+): status\s+(\d+)\s+(\d+) chunks\s+(\d+) candidates\s+(\d+) live\s+(\d+) members\s+(\d+) member')


def test_gzip_members_core_program(tmp_path):
    exe = str(tmp_path / 'gzip_members_core_test')
    src = os.path.join(ROOT, 'tests', 'cpp', 'gzip_members_core_test.cpp')
    built = subprocess.run([_host_compiler(), '-std=c++17', '-O1', '-Wall', '-Wextra', src, '-lz', '-o', exe], capture_output=True,
                           text=True)
    assert built.returncode == 0 and not built.stderr.strip(), built.stderr      # (a warning fails it too)
    ran = subprocess.run([exe, _files_binary(str(tmp_path / 'files.bin'))], capture_output=True, text=True, timeout=300)
    assert ran.returncode == 0, (ran.stdout + ran.stderr)[-3000:]
    seen = set()
    for line in ran.stdout.splitlines():
        got = LINE.match(line)
        assert got, line
        name, (chunk, status, chunks, cands, live, members, marks) = got.group(1), map(int, got.groups()[1:])
        seen.add(name)
        if name in G.files():                                    # the numbers of the host-compiled steps are the model's
            model = G.modelled(name, chunk)
            assert (status, chunks, cands, live, members, marks) == (0, model['chunks'], model['candidates'], model['live'],
                                                                     model['members'], model['member_candidates']), line
        elif name == 'reach_bad':
            assert GO.GZIP_STATUS[status] == 'bad_distance', line
        elif G.damaged()[name][1] is not None:
            assert GO.GZIP_STATUS[status] == G.damaged()[name][1], line
    assert seen == set(NAMES) | {'reach_bad'} | set(G.DAMAGE)


def test_gzip_members_core_program_under_sanitizers(tmp_path):
    exe = str(tmp_path / 'gzip_members_core_test_san')
    src = os.path.join(ROOT, 'tests', 'cpp', 'gzip_members_core_test.cpp')
    built = subprocess.run([_host_compiler(), '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
                            src, '-lz', '-o', exe], capture_output=True, text=True)
    if built.returncode != 0:
        pytest.skip('the host compiler does not link the sanitizers: ' + built.stderr[-300:])
    ran = subprocess.run([exe, _files_binary(str(tmp_path / 'files.bin'))], capture_output=True, text=True, timeout=600)
    assert ran.returncode == 0, (ran.stdout + ran.stderr)[-3000:]


def test_abi_names_and_argument_checks():
    lib = _lib.load()
    names = ['besst_dev_gzip_members_plan_workspace_bytes', 'besst_dev_gzip_members_plan',
             'besst_dev_gzip_members_inflate_workspace_bytes', 'besst_dev_gzip_members_inflate']
    with open(os.path.join(ROOT, 'include', 'besst_amd.h')) as fh:
        header = fh.read()
    for name in names:
        assert name in _lib.exported_symbols() and getattr(lib, name) and re.search(r'\b%s\(' % name, header), name
    assert '#define BESST_GZIP_TOO_MANY_MEMBERS %d\n' % GO.GZIP_STATUS.index('too_many_members') in header
    assert '#define BESST_GZIP_MEMBER_INFO_WORDS %d\n' % GO.GZIP_MEMBER_INFO_WORDS in header
    assert '#define BESST_GZIP_INFO_MEMBERS %d\n' % GO.GZIP_INFO_MEMBERS in header
    assert '#define BESST_GZIP_INFO_BAD_MEMBER %d\n' % GO.GZIP_INFO_BAD_MEMBER in header
    ws = lib.besst_dev_gzip_members_plan_workspace_bytes
    assert ws(1 << 20, 10, 65536, 0) > 0 and ws(1 << 20, 10, 65536, 4096) > ws(1 << 20, 10, 65536, 0)
    assert ws(1 << 20, 10, 65536, 0) >= lib.besst_dev_gzip_plan_workspace_bytes(1 << 20, 10, 65536)
    assert ws(1 << 20, 10, 250, 16) == 0 and ws(1 << 20, 10, 256, -1) == 0 and ws(17, 10, 256, 16) == 0
    iws = lib.besst_dev_gzip_members_inflate_workspace_bytes
    assert iws(1000, 1, 1) >= 2000 and iws(1000, 5000, 5000) > iws(1000, 5000, 1) > iws(1000, 1, 1)
    assert iws(1000, 0, 1) == 0 and iws(1000, 1, 0) == 0 and iws(1000, 1, 2) == 0 and iws(-1, 1, 1) == 0
    p = C.c_void_p
    buf = (C.c_uint64 * 64)()
    at = C.addressof(buf)
    plan, inflate = lib.besst_dev_gzip_members_plan, lib.besst_dev_gzip_members_inflate
    assert plan(None, None, 100, 10, 256, 4, 0, p(at), 1 << 20, p(at)) == 1 and 'null' in _lib.last_error()
    assert plan(None, p(at), 100, 10, 250, 4, 0, p(at), 1 << 20, p(at)) == 1 and 'range' in _lib.last_error()
    assert plan(None, p(at), 100, 10, 256, -4, 0, p(at), 1 << 20, p(at)) == 1 and 'range' in _lib.last_error()
    assert plan(None, p(at), 100, 10, 256, 4, 0, p(at), 16, p(at)) == 1 and 'small' in _lib.last_error()
    assert plan(None, p(at + 2), 100, 10, 256, 4, 0, p(at), 1 << 20, p(at)) == 1 and 'misaligned' in _lib.last_error()
    assert inflate(None, p(at), 100, 10, 256, 4, 0, None, 1, 1, 50, p(at), p(at), 1 << 20, p(at)) == 1 and 'null' in _lib.last_error()
    assert inflate(None, p(at), 100, 10, 256, 4, 0, p(at), 6, 1, 50, p(at), p(at), 1 << 20, p(at)) == 1
    assert 'n_live' in _lib.last_error()                         # more segments than chunks and member candidates together
    assert inflate(None, p(at), 100, 10, 256, 4, 0, p(at), 5, 1, 50, p(at), p(at), 16, p(at)) == 1 and 'small' in _lib.last_error()
