"""GPU: the lean side-stream loop with the library's constants compiled in.

launch_classify_scan takes a specialised instance of fused_wave_kernel<kRuns, 3, true> - one for `fr`, one for `rf` - when
the library's read_len is a whole number and extend_paths, no_score and detect_duplicate have BESST's defaults, and the
generic lean form otherwise (or for every library under BESST_LOOP_SPEC=0).  What can go wrong is what the constants touch:
the integer form of PosDirCalculator and the strand inversion of `rf`, the acceptance borders behind it, the double call of a
case-A pair, case B, the BWA quirk's sides, the duplicate chain - and the host rule itself, which must leave the
specialisation for every library that differs in ONE of its five conditions.

Streams are 2 * BLOCK + SUB + 5 records long: two lean blocks, a chain across their border, and a block for the general
form.  Every case runs the side-stream form writing keys and grouping runs and compares edge table, coverage and counters
with oracle/py_oracle.record_loop, with the C oracle, and with the same call under BESST_LOOP_SPEC=0 in the same process
(the switch is read at every call).  What the cases cannot see is WHICH instance ran: the library exports nothing that tells, so
a host rule that always chose the generic form would pass them all.  `takes_specialised_form` restates the rule and
tests/test_loop_spec_design.py holds the restatement against the source text; that is the limit without a change of the ABI.
The generators assert on the CPU that a stream has the property it is named for
(tests/test_loop_spec_design.py runs them without a GPU)."""
import math

import numpy as np
import pytest

from tests import record_design as D
from tests import test_gpu_candidate_stream as S
from tests import test_gpu_side_loop_pipeline as P
from tests.record_design import BLOCK, SUB

pytestmark = pytest.mark.gpu

N = 2 * BLOCK + SUB + 5
A, B = D.LARGE[0], D.LARGE[1]
CLS = np.asarray(D.TABLE['cls'])
SCAF = np.asarray(D.TABLE['scaf'])
COLS = ('tid', 'mtid', 'pos', 'mpos', 'flag', 'mapq', 'qlen')

SPEC_LIBS = {'fr': D.make_lib('fr', read_len=100), 'rf': D.make_lib('rf', read_len=100)}
# every way out of the specialisation, one condition at a time
WAYS_OUT = {
    'read_len_99.999': D.make_lib(read_len=99.999),
    'read_len_0.5': D.make_lib(read_len=0.5),
    'extend_paths_off': D.make_lib(extend_paths=False),
    'no_score_on': D.make_lib(no_score=True),
    'detect_duplicate_off': D.make_lib(detect_duplicate=False),
}


def takes_specialised_form(lib):
    """The host rule of launch_classify_scan, restated: read_len a whole number in [0, 2^31) (api.hip's read_len_int >= 0)
    and the three flags at BESST's defaults."""
    rl = lib['read_len']
    whole = 0 <= rl < 2 ** 31 and rl == math.floor(rl)
    return bool(whole and lib['extend_paths'] and not lib['no_score'] and lib['detect_duplicate'])


assert all(takes_specialised_form(lib) for lib in SPEC_LIBS.values())
assert not any(takes_specialised_form(lib) for lib in WAYS_OUT.values())
assert all(sum(lib[k] != SPEC_LIBS['fr'][k] for k in lib) == 1 for lib in WAYS_OUT.values())


def _kinds(rec, rp):
    """Per record: a case-A pair (two large contigs on different scaffolds), a case-B pair (the other reaching ones)."""
    tid, mtid = np.asarray(rec['tid']).astype(np.int64), np.asarray(rec['mtid']).astype(np.int64)
    ok = rp.reach
    t, m = np.where(ok, tid, 0), np.where(ok, mtid, 0)
    case_a = ok & (CLS[t] == D.CLS_LARGE) & (CLS[m] == D.CLS_LARGE) & (SCAF[t] != SCAF[m])
    return case_a, ok & ~case_a


def _per_block(mask):
    return [bool(mask[lo:lo + BLOCK].any()) for lo in range(0, N, BLOCK)]


def _assert_count_is_calls(lib, rec, rp):
    """Nothing but the designed duplicates: every emitted case-A record was counted twice where the library scores and
    extends paths (the double call for G and G'), every other emitted record once."""
    case_a, _ = _kinds(rec, rp)
    twice = lib['extend_paths'] and not lib['no_score']
    assert rp.counters[0] == int((rp.emit & case_a).sum()) * (2 if twice else 1) + int((rp.emit & ~case_a).sum())


# ---- a stream of everything: the two specialised forms on both tables, and every way out ---------------------------------------
def stream_mix(name, lib):
    """Case-A links, case-B links of both kinds, BWA-quirk records and mates on absent rows all along the three blocks; the
    last reaching record of a block and the first of the next observe the same, across the border of the two lean blocks and
    across the border of the two launches."""
    b = D.Builder(N, lib, filler_rows=[A, B])
    for i in range(3, N, 41):
        S._link(b, i)                                        # large / large
    for i in range(11, N, 97):
        b.link(i, int(b.tid[i]), D.SMALL[i % 20], *D.distinct_obs(i), reverse=bool(i & 2), mreverse=not (i & 4))
    for i in range(29, N, 211):
        b.link(i, D.SMALL[3 + i % 5], D.SMALL[10 + i % 7], *D.distinct_obs(i), reverse=not (i & 2))
    for i in range(17, N, 301):
        b.fishy(i, int(b.tid[i]), D.LARGE[40 + i % 5], reverse=bool(i & 1), mreverse=bool(i & 2))
    for i in range(23, N, 1999):
        b.raw(i, int(b.tid[i]), P.ABSENT[i % 3], S.RD2, mapq=60)
    chain = {}
    for k, at in enumerate((BLOCK, 2 * BLOCK)):
        for i in (at - 2, at + 1, at + 9):
            b.link(i, int(b.tid[i]), D.LARGE[12 + k], 100 + k, 120 + k)
        chain[at] = (at - 2, at + 1, at + 9)
    rec = b.records()
    rp = D.replay(rec, D.TABLE, lib)
    c = D.census(rec, lib, rp)
    case_a, case_b = _kinds(rec, rp)
    detect = bool(lib['detect_duplicate'])
    assert _per_block(case_a) == [True] * 3 and _per_block(rp.fishy) == [True] * 3
    assert _per_block(case_b) == [bool(lib['extend_paths'])] * 3
    for at, (first, second, third) in chain.items():
        assert rp.emit[first] and not rp.dup[first] and rp.dup[second] and rp.dup[third]
        assert not rp.reach[first + 1:second].any() and not rp.reach[second + 1:third].any()
        assert bool(rp.emit[second]) == bool(rp.emit[third]) == (not detect)
    assert c.heads[1:] == [BLOCK + 1, 2 * BLOCK + 1] and c.dropped_heads == ([BLOCK + 1, 2 * BLOCK + 1] if detect else [])
    assert int(rp.dup.sum()) == 4
    if detect:
        _assert_count_is_calls(lib, rec, rp)
    masks = {t[5] for t in rp.tuples if not t[2]}
    want_a = D.MASK_GP if lib['no_score'] else (D.MASK_G | (D.MASK_GP if lib['extend_paths'] else 0))
    assert masks == ({want_a, D.MASK_GP} if lib['extend_paths'] else {want_a})
    return D.Stream('spec_' + name, rec, lib, {})


# ---- the acceptance borders ----------------------------------------------------------------------------------------------------
def stream_accept(orientation, run_lib=None):
    """record_design's acceptance stream placed for the whole-number library of one orientation - every pair of {-1, 0, 25,
    26}, sums one below, at and one above the threshold, through all sixteen pairs of calculator branches - laid across the
    border of the two lean blocks, and its border pairs once more in the block of the general form.  run_lib: the same
    coordinates under another read length (the fp64 branches)."""
    lib = SPEC_LIBS[orientation]
    src = D.acceptance_stream('accept', lib)
    length = len(src.records['tid'])
    off = BLOCK - length // 2
    b = D.Builder(N, lib, filler_rows=[A])
    for k in COLS:
        getattr(b, k)[off:off + length] = src.records[k]
    T = src.claims['threshold']
    tail = [(25, 26), (26, 25), (26, 26), (26, T - 27), (26, T - 26), (T - 300, 300), (-1, -1), (0, 30)]
    for j, (o1, o2) in enumerate(tail):
        b.link(2 * BLOCK + 10 + 8 * j, A, D.LARGE[30 + j], o1, o2, reverse=bool(j & 1), mreverse=not (j & 2))
    rec = b.records()
    rp = D.replay(rec, D.TABLE, lib)
    wanted = {i + off: o for i, o in src.claims['observations'].items()}
    wanted.update(b.wanted)
    assert len(src.claims['branches']) == 16 and min(wanted) < BLOCK <= max(i for i in wanted if i < 2 * BLOCK)
    assert sum(1 for i in wanted if i >= 2 * BLOCK) == len(tail)
    for i, (o1, o2) in wanted.items():
        assert rp.reach[i] and (rp.o1[i], rp.o2[i]) == (o1, o2)
        assert bool(rp.accept[i]) == (o1 > 25 and o2 > 25 and o1 + o2 < T)
    seen = set(wanted.values())
    assert {(25, 26), (26, 25), (26, 26), (26, T - 27), (26, T - 26)} <= seen
    assert int(rp.reach.sum()) == len(wanted) and 0 < int(rp.accept.sum()) < len(wanted)
    if run_lib is None:
        return D.Stream('spec_accept_' + orientation, rec, lib, {})
    other = D.replay(rec, D.TABLE, run_lib)
    assert (other.o1 != rp.o1).any() and (other.accept != rp.accept).any()      # the read length is in the observations
    return D.Stream('spec_accept_same_coordinates', rec, run_lib, {})


# ---- the duplicate chain -------------------------------------------------------------------------------------------------------
def stream_chain(orientation):
    """Reaching records with equal observations on different node pairs, detect_duplicate on: neighbours, a chain of three,
    behind a predecessor that is not accepted, across the border of the two lean blocks and across the border of the two
    launches; equal obs1 alone is none, and (-1, -1) meets the initial prev_obs and the second call's."""
    lib = SPEC_LIBS[orientation]
    b = D.Builder(N, lib, filler_rows=[A])
    serial = [0]

    def same(at, o=None):
        serial[0] += 1
        o = o or D.distinct_obs(7 * serial[0])
        for j, i in enumerate(at):
            b.link(i, A, D.LARGE[20 + (3 * serial[0] + j) % 30], o[0], o[1])

    b.link(2, A, D.LARGE[40], -1, -1)                        # the stream's first reaching record: the initial prev_obs
    same((40, 44))
    same((120, 125, 131))
    same((160, 166), o=(10, 400))                            # reaches, is not accepted, is the predecessor all the same
    b.link(280, A, D.LARGE[45], 77, 200)
    b.link(284, A, D.LARGE[46], 77, 201)                     # equal obs1 only
    b.link(300, A, D.LARGE[47], -1, -1)                      # the second call's prev_obs is (-1, -1)
    same((2 * SUB - 1, 2 * SUB))
    same((BLOCK - 1, BLOCK))
    same((BLOCK + 700,))
    same((2 * BLOCK - 1, 2 * BLOCK))
    same((2 * BLOCK + 100,))
    rec = b.records()
    rp = D.replay(rec, D.TABLE, lib)
    c = D.census(rec, lib, rp)
    assert sorted(np.flatnonzero(rp.dup).tolist()) == [2, 44, 125, 131, 166, 2 * SUB, BLOCK, 2 * BLOCK]
    assert rp.counters[3] == 9 and not rp.emit[rp.dup].any()     # (with the second call of record 300)
    assert c.heads == [2, BLOCK, 2 * BLOCK] and c.dropped_heads == [BLOCK, 2 * BLOCK]
    assert rp.reach[160] and not rp.accept[160] and rp.emit[280] and rp.emit[284] and not rp.emit[300]
    return D.Stream('spec_chain_' + orientation, rec, lib, {})


# ---- case A, case B, the quirk -------------------------------------------------------------------------------------------------
PAIR_BASES = [5, SUB + 3, 31 * SUB + 200, BLOCK - 17, BLOCK + 300, 2 * BLOCK - 11, 2 * BLOCK + 40]


def stream_pairs(orientation):
    """Both contig directions of large / large (case A: the double call), large / small and small / small (case B) through all
    four strand pairs, and a BWA-quirk record of each, in groups: in the first two sub-tiles, inside a block, across both
    block borders and in the block of the general form."""
    lib = SPEC_LIBS[orientation]
    kinds = [p for p in D.rule_pairs() if p[0] in ('large/large', 'large/small', 'small/small')]
    assert len(kinds) == 6
    b = D.Builder(N, lib, filler_rows=[A, B])
    links, quirks = [], []
    for base in PAIR_BASES:
        i = base
        for q, (_, t, m) in enumerate(kinds):
            for strands in range(4):
                b.link(i, t, m, *D.distinct_obs(i), reverse=bool(strands & 1), mreverse=bool(strands & 2))
                links.append(i)
                i += 1
            b.fishy(i, t, m, reverse=bool(q & 1), mreverse=bool(q & 2))
            quirks.append(i)
            i += 1
    assert i <= N and len(set(links + quirks)) == len(PAIR_BASES) * 30
    rec = b.records()
    rp = D.replay(rec, D.TABLE, lib)
    case_a, case_b = _kinds(rec, rp)
    assert rp.reach[links].all() and rp.emit[links].all() and not rp.dup.any() and int(rp.reach.sum()) == len(links)
    assert rp.fishy[quirks].all() and int(rp.fishy.sum()) == len(quirks)
    assert int(case_a.sum()) == len(links) // 3 and int(case_b.sum()) == 2 * len(links) // 3
    assert _per_block(case_a) == _per_block(case_b) == _per_block(rp.fishy) == [True] * 3
    _assert_count_is_calls(lib, rec, rp)
    assert rp.counters[0] == 2 * int(case_a.sum()) + int(case_b.sum())
    assert {t[5] for t in rp.tuples if not t[2]} == {D.MASK_G | D.MASK_GP, D.MASK_GP}
    sides = {(k >> 1) & 1 for k in rp.key[quirks].tolist()} | {(k >> (1 + D.NODE_BITS)) & 1 for k in rp.key[quirks].tolist()}
    assert sides == {0, 1}                                   # both sides of a scaffold among the quirk tuples' nodes
    return D.Stream('spec_pairs_' + orientation, rec, lib, {})


STREAMS = {}
for _o in ('fr', 'rf'):
    STREAMS['mix_' + _o] = (lambda o=_o: stream_mix(o, SPEC_LIBS[o]))
    STREAMS['accept_' + _o] = (lambda o=_o: stream_accept(o))
    STREAMS['chain_' + _o] = (lambda o=_o: stream_chain(o))
    STREAMS['pairs_' + _o] = (lambda o=_o: stream_pairs(o))
for _k in WAYS_OUT:
    STREAMS['out_' + _k] = (lambda k=_k: stream_mix(k, WAYS_OUT[k]))
STREAMS['out_same_coordinates'] = lambda: stream_accept('fr', dict(SPEC_LIBS['fr'], read_len=99.999))

# both specialised forms on both tables; everything else on the designed table
CASES = [('mix_' + o, tab) for o in ('fr', 'rf') for tab in ('absent', 'present')] + \
        [(k, 'absent') for k in sorted(STREAMS) if not k.startswith('mix_')]

_MADE, _ORACLE = {}, {}


def made(key):
    if key not in _MADE:
        _MADE[key] = STREAMS[key]()
    return _MADE[key]


def oracle(key, tab):
    """(stream, batch, C oracle's workload, py oracle's result) of a stream on a table, computed once."""
    if (key, tab) not in _ORACLE:
        from oracle import py_oracle as O
        s = made(key)
        rec, _, p = D.as_oracle_inputs(s)
        wl = dict(table=D.table_columns(P.TABLES[tab]), lib=s.lib, node_bits=D.NODE_BITS)
        _ORACLE[(key, tab)] = (s, D.as_batch(s), wl, O.record_loop(rec, P.TABLES[tab], p))
    return _ORACLE[(key, tab)]


def check(key, tab, table, aligned, ctr):
    from tests import gpu_util as DU
    from tests.test_gpu_fullsize import assert_table_equals_c_oracle
    s, batch, wl, loop = oracle(key, tab)
    DU.assert_matches_oracle(table, aligned, ctr, loop, D.N_CONTIGS)
    assert (ctr.n_reach, ctr.n_tuples) == (loop.n_reach, sum(r.n + r.fishy for r in loop.edges.values()))
    assert_table_equals_c_oracle(table, aligned, ctr, batch, wl)


@pytest.mark.parametrize('form', ['writing keys', 'grouping runs'])
@pytest.mark.parametrize('key,tab', CASES)
def test_specialised_loop_against_both_oracles_and_the_generic_form(key, tab, form, monkeypatch):
    s, batch, _, _ = oracle(key, tab)
    assert len(batch) == N and takes_specialised_form(s.lib) == (not key.startswith('out_'))
    grouping = form == 'grouping runs'
    gb = P.builder(tab, grouping, len(batch))
    got = []
    for switch in (None, '0'):                               # the host's choice, then the generic lean form for every library
        if switch is None:
            monkeypatch.delenv('BESST_LOOP_SPEC', raising=False)
        else:
            monkeypatch.setenv('BESST_LOOP_SPEC', switch)
        table, aligned, ctr, spec, ran = P.steps(gb, s, batch, True, monkeypatch.setenv,
                                                 lambda k: monkeypatch.delenv(k, raising=False))
        assert gb.params.record_path == 1 and ran == 3 and gb.params.cand_stream
        if grouping:
            assert spec is not None and spec.segmented == 1 and spec.in_record_loop == 3 and gb.sort_flags == 0
        check(key, tab, table, aligned, ctr)
        got.append(S._columns(table, aligned, ctr))
    for x, y in zip(*got):
        assert np.array_equal(x, y)
