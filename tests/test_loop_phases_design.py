"""CPU: the streams of tests/test_gpu_loop_phases.py have the properties they are named for.  Every generator asserts its own
design - the rounds of every block by the side stream's set rule and by D.census, the positions of the run bits, which phase a
record's sub-tile and its round fall into - so making a stream is the test; here they are made without a GPU, their claims are
stated once more against the facts, and the structure the file restates is held against the source's."""
import re

import pytest

from tests import record_design as D
from tests import test_gpu_loop_phases as L
from tests import test_gpu_loop_spec as LS
from tests.record_design import BLOCK, SUB


@pytest.mark.parametrize('key', sorted(L.STREAMS))
def test_stream_has_its_property(key):
    s = L.made(key)
    assert all(len(v) == L.N for v in s.records.values()) and s.name.startswith('phases_')
    assert L.N == 2 * BLOCK + SUB + 5 and L.N // BLOCK == 2 and L.N % BLOCK > SUB
    f = L.facts(s.records, s.lib)
    assert f['rounds'] == s.claims['rounds'] and len(f['rounds']) == 3
    assert f['runs'] == s.claims['runs']
    if s.claims.get('all_evaluable', True):
        assert [len(r) for r in f['census'].rounds] == s.claims['rounds']
    rec = s.records
    assert all(rec['tid'][i] != rec['tid'][i - 1] for i in f['runs'])
    if key.startswith('rounds_'):
        assert f['rounds'][1] == L.OTHER_ROUNDS != f['rounds'][0]           # the second lean block differs


def test_cases_cover_the_borders_the_two_phases_have():
    assert L.ROUNDS == [0, 1, 2, 3, 63, 64, 65, 256] and L.SUBS == 64 and L.P.UNROLL == 2
    assert [L.phase1_end(r) for r in L.ROUNDS] == [0, 2, 2, 4, 64, 64, 66, 256]
    assert {L.made('rounds_%d' % r).claims['rounds'][0] for r in L.ROUNDS} == set(L.ROUNDS)
    assert {k for k, _ in L.CASES} == set(L.STREAMS) and {t for _, t in L.CASES} == {'absent', 'present'}
    assert len(L.CASES) == 2 * len(L.STREAMS)
    for d in (-1, 0, 1):
        s = L.made('handover_%+d' % d)
        assert [(c % BLOCK) // SUB for c in s.claims['runs'][:2]] == [r + d for r in L.HANDOVER_ROUNDS]
    assert len(L.made('flushes').claims['runs']) == L.SUBS + 2 and L.made('one_contig').claims['runs'] == []
    assert D.CLS_ABSENT in L.P.TABLES['absent']['cls'] and D.CLS_ABSENT not in L.P.TABLES['present']['cls']
    assert LS.takes_specialised_form(L.LIB)                  # BESST_LOOP_SPEC unset: the specialised instance runs


def test_phase_two_streams_only():
    """The loop over the sub-tiles behind the last round calls the streaming half and nothing of a round: no entry loads, no
    row gathers, no pending round."""
    src = open(D.CSRC + '/classify.hip').read()
    lean = src[src.index('if constexpr (kLean) {'):src.index('} else if (kBits != 3 && block_base')]
    loops = [m.start() for m in re.finditer(r'for \(', lean)]
    bodies = []
    for at in loops:
        open_at = lean.index('{', at)
        depth, k = 0, open_at
        while True:
            depth += {'{': 1, '}': -1}.get(lean[k], 0)
            if depth == 0:
                break
            k += 1
        bodies.append(lean[open_at:k + 1])
    streaming = [b for b in bodies if b.count('stream(') == 2 and 'load_q(' in b]
    assert len(streaming) == 2                               # phase 1's loop and phase 2's
    only = [b for b in streaming if not any(w in b for w in ('rows(', 'load_e(', 'round_finish(', 'pend'))]
    assert len(only) == 1
