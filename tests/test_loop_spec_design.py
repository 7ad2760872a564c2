"""CPU: the streams of tests/test_gpu_loop_spec.py have the properties they are named for.  Every generator asserts its own
design - the case-A, case-B and quirk records of every block, the acceptance borders by the replay, the duplicate chain across
both block borders by the replay and the census - so making a stream is the test; here they are made without a GPU, and the
host rule the file restates is held against the source's."""
import re

import pytest

from tests import record_design as D
from tests import test_gpu_loop_spec as L


@pytest.mark.parametrize('key', sorted(L.STREAMS))
def test_stream_has_its_property(key):
    s = L.made(key)
    assert all(len(v) == L.N for v in s.records.values()) and s.name.startswith('spec_')
    assert L.N == 2 * D.BLOCK + D.SUB + 5 and L.N // D.BLOCK == 2 and L.N % D.BLOCK > D.SUB


def test_cases_cover_both_forms_both_tables_and_every_way_out():
    assert {k for k, _ in L.CASES} == set(L.STREAMS)
    assert {(k, t) for k, t in L.CASES if k.startswith('mix_')} == {('mix_' + o, t) for o in ('fr', 'rf') for t in ('absent', 'present')}
    out = {k: L.made(k).lib for k in L.STREAMS if k.startswith('out_')}
    assert len(out) == 6 and not any(L.takes_specialised_form(lib) for lib in out.values())
    assert sorted(lib['read_len'] for lib in out.values() if lib['read_len'] != 100) == [0.5, 99.999, 99.999]
    for flag, value in (('extend_paths', False), ('no_score', True), ('detect_duplicate', False)):
        assert sum(lib[flag] == value for lib in out.values()) == 1
    spec = [L.made(k).lib for k in L.STREAMS if not k.startswith('out_')]
    assert all(L.takes_specialised_form(lib) for lib in spec) and {lib['orientation'] for lib in spec} == {'fr', 'rf'}


def test_host_rule_is_the_source_s():
    src = open(D.CSRC + '/classify.hip').read()
    rule = re.search(r'const bool spec = (.*?);', src, re.S).group(1)
    for term in ('getenv("BESST_LOOP_SPEC")', ):
        assert term in src
    for term in ('a.read_len_int >= 0', 'a.extend_paths != 0', 'a.no_score == 0', 'a.detect_dup != 0'):
        assert term in rule
    assert 'a.rf != 0 ? kSpecRf : kSpecFr' in src
    api = open(D.CSRC + '/api.hip').read()
    assert 'a.read_len_int = (p->read_len >= 0.0 && p->read_len < 2147483648.0 && p->read_len == floor(p->read_len))' in api
