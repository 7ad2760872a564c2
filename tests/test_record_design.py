"""The designed record streams (tests/record_design.py) checked without a GPU: the sequential restatement of the loop body
equals both oracles on every stream; every stream holds the cases it was designed for, where the census of the kernels'
structures says they must be (the ring one short of full, the chunk counts, the heads the stitch drops, the round and
sub-tile positions of the duplicate pairs, the observations the coordinates were solved for); and every named wrong variant
of a rule changes what its stream expects - which is why a kernel with that rule wrong would fail the GPU tests."""
import math

import numpy as np
import pytest

from oracle import c_oracle as CO
from oracle import py_oracle as O
from tests import record_design as D

K, BLOCK, SUB, GROUP = D.K, D.BLOCK, D.SUB, D.GROUP
_RESULTS = {}


def results(name):
    """(stream, Replay, Census, py oracle's LoopResult) of a designed stream, computed once per session."""
    if name not in _RESULTS:
        s = D.all_streams()[name]
        rp = D.replay(s.records, D.TABLE, s.lib)
        rec, table, p = D.as_oracle_inputs(s)
        res = O.LoopResult(D.N_CONTIGS)
        res.tuples = []
        loop = O.record_loop(rec, table, p, res)
        _RESULTS[name] = (s, rp, D.census(s.records, s.lib, rp), loop)
    return _RESULTS[name]


def test_constants_are_read_from_the_sources():
    assert set(K) == {'kClsTile', 'kGroup', 'kStreamTile', 'kFwSub', 'kFwRing', 'kOrdRound', 'kRlChunkTuples', 'kRlCloseRuns',
                      'kRlSlots', 'kRlMaxChunks', 'kStitchSpan'}
    assert all(isinstance(v, int) and v > 0 for v in K.values())
    # what the designs rely on: a ring of a sub-tile and an unfinished round, sub-tiles and groups that tile a block,
    # run names of a byte, several blocks per stitch span
    assert K['kFwRing'] == K['kFwSub'] + 64 and K['kClsTile'] % K['kFwSub'] == 0 and K['kClsTile'] % K['kGroup'] == 0
    assert K['kRlSlots'] >= 2 * K['kRlCloseRuns'] - 1 and K['kRlSlots'] < 256 and K['kStitchSpan'] > 8
    assert sorted(D.all_streams()) == sorted(D.STREAM_NAMES)


def test_table_holds_every_kind_of_contig():
    t = D.TABLE
    assert max(t['scaf']) >= 2048 and 2 * D.NODE_BITS + 1 >= 25          # stage 2 takes the hand-over from 25-bit keys on
    for kind in ('large', 'small'):
        assert D.rows_of(kind, True) and D.rows_of(kind, False)
    assert D.rows_of('absent') and all(t['cls'][r] == D.CLS_ABSENT for r in D.rows_of('absent'))
    for a, b in zip(D.rows_of('pair0') + D.rows_of('spair0'), D.rows_of('pair1') + D.rows_of('spair1')):
        assert t['scaf'][a] == t['scaf'][b] and t['cpos'][a] == 0 and t['cpos'][b] == t['clen'][a] + D.PAIR_GAP
        assert t['slen'][a] == t['slen'][b] == t['cpos'][b] + t['clen'][b] and t['cdir'][a] and not t['cdir'][b]
    singles = [r for r in range(D.N_CONTIGS) if r % 8 < 5]
    assert len({t['scaf'][r] for r in singles}) == len(singles)


@pytest.mark.parametrize('read_len', [100, 100.38, 99.999, 0.5])
@pytest.mark.parametrize('orientation', ['fr', 'rf'])
def test_place_inverts_both_calculators(orientation, read_len):
    lib = D.make_lib(orientation, read_len)
    branches = set()
    rows = [D.rows_of('large', True)[3], D.rows_of('large', False)[3], D.rows_of('pair0')[2], D.rows_of('pair1')[2],
            D.rows_of('small', False)[1]]
    for row in rows:
        for reverse in (False, True):
            branches.add(D.branch_of(lib, row, reverse))
            for obs in (-1, 0, 25, 26, 399, 400, 5000):
                pos = D.place(row, reverse, obs, lib)
                t = D.TABLE
                got = O.posdir(orientation, t['cdir'][row], not reverse, t['cpos'][row], pos, t['slen'][row], t['clen'][row], read_len)
                assert got[0] == obs, (row, reverse, obs, pos)
    assert branches == {0, 1, 2, 3}


@pytest.mark.parametrize('name', D.STREAM_NAMES)
def test_replay_equals_both_oracles(name):
    s, rp, _, loop = results(name)
    assert rp.counters[:6] == [loop.count, loop.non_unique, loop.non_unique_for_scaf, loop.nr_of_duplicates, loop.too_long,
                               loop.fishy_reads]
    assert rp.aligned == loop.aligned and rp.prev == loop.prev and rp.n_reach == loop.n_reach
    assert rp.tuples == loop.tuples                                       # every tuple, in stream order
    # rows and the order of the observations inside them
    rows = {}
    for i in np.nonzero(rp.emit | rp.fishy)[0]:
        rows.setdefault(int(rp.key[i]), []).append(int(i))
    want = {}
    for (u, v), r in loop.edges.items():
        if r.n:
            want[((u << D.NODE_BITS) | v) << 1] = (r.n, r.first_idx, [a + b for a, b in zip(r.obs_u, r.obs_v)])
        if r.fishy:
            want[(((u << D.NODE_BITS) | v) << 1) | 1] = (r.fishy, None, None)
    assert set(rows) == set(want)
    for key, members in rows.items():
        n, first, sums = want[key]
        assert len(members) == n
        if first is not None:
            assert members[0] == first and [int(rp.o1[i] + rp.o2[i]) for i in members] == sums
    # the C oracle: the same stream as packed keys and payload words
    keys, payload, aligned, ctr = CO.record_loop(D.as_batch(s), D.table_columns(), s.lib, D.NODE_BITS)
    assert ctr.tolist() == rp.counters and aligned.tolist() == rp.aligned
    t = np.array(rp.tuples, dtype=np.uint64).reshape(-1, 6)
    assert np.array_equal(keys, (((t[:, 0] << np.uint64(D.NODE_BITS)) | t[:, 1]) << np.uint64(1)) | t[:, 2])
    assert np.array_equal(payload, t[:, 3] | ((t[:, 4] | (t[:, 5] << np.uint64(30))) << np.uint64(32)))


@pytest.mark.parametrize('name', D.STREAM_NAMES)
def test_placed_records_observe_what_they_were_placed_for(name):
    s, rp, _, _ = results(name)
    for i, (o1, o2) in s.claims.get('observations', {}).items():
        assert rp.reach[i] and (rp.o1[i], rp.o2[i]) == (o1, o2), (name, i)


def test_rules_streams_hold_the_product_under_every_switch():
    libs = D.RULE_LIBS
    for field in ('orientation', 'read_len', 'min_mapq', 'detect_duplicate', 'extend_paths', 'no_score'):
        assert len({lib[field] for lib in libs}) == 2, field
    assert any(lib['min_mapq'] == 0 and lib['extend_paths'] and not lib['no_score'] for lib in libs)
    kinds = {'large/large', 'large/small', 'small/small', '*/absent', 'absent/*', 'two contigs of a scaffold', 'same contig',
             'tid -1', 'tid beyond', 'mtid -1', 'mtid beyond'}
    for k, lib in enumerate(libs):
        s, rp, cs, loop = results('rules%d' % k)
        assert set(s.claims['pair_kinds']) == kinds and s.claims['product'] == 64 * 4 * 2 * len(kinds)
        rec = s.records
        n = s.claims['product']
        assert len(rec['tid']) == 2 * n
        # product order, then the same records shuffled
        first = sorted(zip(*(rec[c][:n].tolist() for c in ('tid', 'mtid', 'pos', 'mpos', 'flag', 'mapq', 'qlen'))))
        second = sorted(zip(*(rec[c][n:].tolist() for c in ('tid', 'mtid', 'pos', 'mpos', 'flag', 'mapq', 'qlen'))))
        assert first == second and rec['flag'][:n].tolist() != rec['flag'][n:].tolist()
        assert {int(f) >> 2 & 63 for f in rec['flag'][:n]} == set(range(64))
        assert set(rec['mapq'].tolist()) == {0, max(lib['min_mapq'] - 1, 0), lib['min_mapq'], 255}
        assert rp.n_reach > 0 and rp.counters[5] > 0 and rp.counters[1] > 0
        if lib['min_mapq'] == 0:
            assert rp.counters[2] > 0                        # a mapq 0 record reached CreateEdge
        else:
            assert rp.counters[2] == 0


@pytest.mark.parametrize('name', ['accept_whole', 'accept_fractional', 'accept_half'])
def test_acceptance_borders(name):
    s, rp, _, _ = results(name)
    T = s.claims['threshold']
    assert T == math.ceil(s.lib['ins_size_threshold'])
    assert len(s.claims['branches']) == 16                   # both calculators' four branches at both ends
    seen = set()
    for i, (o1, o2) in s.claims['observations'].items():
        assert bool(rp.accept[i]) == (o1 > 25 and o2 > 25 and o1 + o2 < T), (i, o1, o2)
        seen.add((o1, o2))
    assert {(a, b) for a in (-1, 0, 25, 26) for b in (-1, 0, 25, 26)} <= seen
    assert {T - 1, T, T + 1} <= {a + b for a, b in seen if a == 26} and {T - 1, T, T + 1} <= {a + b for a, b in seen if a == 300}


def test_same_coordinates_through_the_float_branches():
    """The coordinates solved for read_len 100, read with 99.999: the two branches that add read_len truncate to one less,
    the other two stay."""
    whole, _, _, _ = results('accept_whole')
    s, rp, _, _ = results('accept_same_coordinates')
    assert all(np.array_equal(whole.records[c], s.records[c]) for c in whole.records)
    changed = 0
    for i, (o1, o2) in whole.claims['observations'].items():
        b1 = D.branch_of(s.lib, s.records['tid'][i], bool(s.records['flag'][i] & D.F_REVERSE))
        b2 = D.branch_of(s.lib, s.records['mtid'][i], bool(s.records['flag'][i] & D.F_MREVERSE))
        want = (o1 - (1 if b1 >= 2 and o1 > 0 else 0), o2 - (1 if b2 >= 2 and o2 > 0 else 0))
        assert (rp.o1[i], rp.o2[i]) == want, (i, b1, b2)
        changed += want != (o1, o2)
    assert changed > 100


@pytest.mark.parametrize('name', ['chain_detect', 'chain_count'])
def test_chain_pairs_sit_on_their_borders(name):
    s, rp, cs, _ = results(name)
    pairs = s.claims['pairs']
    for label, members in pairs.items():
        assert all(rp.reach[i] for i in members), label
        if len(members) > 1 and label != 'equal obs1 only':
            o = {(int(rp.o1[i]), int(rp.o2[i])) for i in members}
            assert len(o) == 1 and len({int(rp.key[i]) for i in members}) == len(members), label
            assert all(rp.dup[i] for i in members[1:]), label
            between = np.nonzero(rp.reach[members[0] + 1:members[1]])[0]
            assert len(between) == 0, label
    first = int(np.nonzero(rp.reach)[0][0])
    assert pairs['first reaching record against the initial prev_obs'] == (first,) and rp.dup[first]
    assert (rp.o1[first], rp.o2[first]) == (-1, -1)
    i = pairs['(-1, -1) under the double call'][0]
    assert (rp.o1[i], rp.o2[i]) == (-1, -1) and not rp.dup[i] and s.lib['extend_paths'] and not s.lib['no_score']
    a, b = pairs['equal obs1 only']
    assert rp.o1[a] == rp.o1[b] and rp.o2[a] != rp.o2[b] and not rp.dup[b]
    a, b = pairs['next lane']
    assert a // 4 + 1 == b // 4 and a // 256 == b // 256
    a, b = pairs['inside a lane']
    assert a // 4 == b // 4
    a, b = pairs['sub-tile border']
    assert a % SUB == SUB - 1 and b == a + 1
    a, b = pairs['round border']                             # the block's 64th and 65th evaluable candidate
    assert cs.evaluable[a] and cs.evaluable[b] and int(cs.evaluable[:a].sum()) == 63 and int(cs.evaluable[:b].sum()) == 64
    assert (cs.round_of[a], cs.round_of[b]) == (0, 1)
    a, b = pairs['predecessor reaches but is not accepted']
    assert not rp.accept[a] and not rp.accept[b]
    a, b = pairs['fishy record between']
    assert rp.fishy[a + 1:b].sum() == 1
    a, b = pairs['small contig, one call']
    assert D.TABLE['cls'][s.records['mtid'][a]] == D.CLS_SMALL
    a, b = pairs['block border']
    assert (a, b) == (BLOCK - 1, BLOCK) and cs.heads[1] == BLOCK
    assert int((rp.accept | rp.fishy)[BLOCK:2 * BLOCK].sum()) == 1           # the head is its block's only tuple
    a, b = pairs['one block without a reaching record between']
    assert b // BLOCK - a // BLOCK == 2 and cs.heads[b // BLOCK] == b
    a, b = pairs['three blocks without a reaching record between']
    assert b // BLOCK - a // BLOCK == 4 and cs.heads[b // BLOCK] == b
    assert [blk for blk, h in enumerate(cs.heads) if h < 0] == s.claims['empty_blocks']
    assert cs.dropped_heads == s.claims['dropped_heads']
    if s.lib['detect_duplicate']:
        assert len(cs.dropped_heads) == 3
        # spans of one and of two blocks: dropped heads whose predecessor lies in another span, and (two) one in the head's own
        last_reach = {h: int(np.nonzero(rp.reach[:h])[0][-1]) // BLOCK for h in cs.dropped_heads}
        for span in (1, 2):
            same = [h for h, p in last_reach.items() if p // span == (h // BLOCK) // span]
            assert len(same) == (0 if span == 1 else 1) and len(last_reach) - len(same) >= 2
    # the heads call CreateEdge twice
    assert all(D.TABLE['cls'][s.records[c][h]] == D.CLS_LARGE for h in s.claims['dropped_heads'] for c in ('tid', 'mtid'))


def test_ring_streams_fill_the_ring_to_one_short():
    lengths = []
    for n in D.RING_LENGTHS:
        s, rp, cs, _ = results('ring_n%d' % n)
        lengths.append(len(s.records['tid']))
        assert cs.ring_peak == s.claims['ring_peak'] == K['kFwRing'] - 1
        assert cs.sub_counts[0][:len(D.RING_SUBS)].tolist() == D.RING_SUBS
        assert {0, 1, 63, 64, 65, 127, 128, 129, 255, 256} <= set(cs.sub_counts[0].tolist())
        peak = np.argwhere(cs.queue_before + cs.sub_counts == K['kFwRing'] - 1)
        assert len(peak) and all(cs.queue_before[b][st] == 63 and cs.sub_counts[b][st] == SUB for b, st in peak)
        assert cs.head_wraps and cs.sub_counts[0][-1] == SUB               # the queue's head wraps; a full last sub-tile
        assert rp.reach[BLOCK:2 * BLOCK].all() and rp.emit[BLOCK:2 * BLOCK].all()
        assert sum(cs.rounds[1]) == BLOCK and set(cs.rounds[1]) == {64}
    assert lengths == D.RING_LENGTHS
    assert {n % 4 for n in lengths} == {0, 1, 2, 3}
    assert {2 * BLOCK, 2 * BLOCK + 1, 2 * BLOCK + SUB - 1, 2 * BLOCK + SUB, 2 * BLOCK + SUB + 1} <= set(lengths)


@pytest.mark.parametrize('name', ['runs', 'runs_over'])
def test_runs_streams_close_their_chunks_where_designed(name):
    s, rp, cs, _ = results(name)
    c = s.claims
    assert cs.chunk_sizes[c['chunk_512_block']][:2] == [K['kRlChunkTuples'], K['kRlChunkTuples'] - 1]
    keys = cs.chunk_keys[c['table_127_block']][0]
    assert len(keys) == K['kRlSlots'] - 1                    # 63 open runs + a round of 64 new keys
    hashes = sorted(D.slot_hash(k) for k in keys)
    top = hashes[-1]
    assert hashes.count(top) >= 8 and top + hashes.count(top) > K['kRlSlots']   # probing runs from the last slots into slot 0
    assert len({D.slot_hash(k) for k in keys}) < len(keys)
    # a link key and the fishy key of the same node pair in one chunk; a run of one tuple among longer ones
    both = [ks for ks in cs.chunk_keys[c['fishy_pair_block']] if any(k & 1 and (k ^ 1) in ks for k in ks)]
    assert both
    blk = c['fishy_pair_block']
    members = np.nonzero((rp.emit | rp.fishy)[blk * BLOCK:(blk + 1) * BLOCK])[0] + blk * BLOCK
    tail = [int(rp.key[i]) for i in members if i >= blk * BLOCK + 192]
    counts = {k: tail.count(k) for k in set(tail)}
    assert 1 in counts.values() and max(counts.values()) > 20
    assert cs.chunks[c['chunks_block']] == c['chunks'] == K['kRlMaxChunks'] + (1 if c['over'] else 0)
    assert max(cs.chunks) == c['chunks']
    assert all(len(ks) == K['kRlCloseRuns'] for ks in cs.chunk_keys[c['chunks_block']])     # each closed by its 64th run
    assert rp.counters[3] == 0                               # no duplicates: every chunk border is where the design put it


@pytest.mark.parametrize('name', ['groups', 'groups_short'])
def test_groups_streams_hold_their_candidate_counts(name):
    s, rp, cs, _ = results(name)
    want = s.claims['block_candidates']
    assert cs.block_candidates[:len(want)].tolist() == want
    assert {0, 1, K['kOrdRound'] - 1, K['kOrdRound'], K['kOrdRound'] + 1, 1023, 1024, 1025, 2049, BLOCK} <= set(want)
    assert cs.ord_rounds[:len(want)] == [-(-c // K['kOrdRound']) for c in want]
    assert {0, 1, GROUP - 1, GROUP} <= set(cs.group_counts[3].tolist())
    blk = s.claims['last_group_only_block']
    assert cs.group_counts[blk][:-1].sum() == 0 and cs.group_counts[blk][-1] > 0
    n = len(s.records['tid'])
    assert n % K['kStreamTile'] in (1, K['kStreamTile'] - 1) and n % GROUP != 0
    assert rp.n_reach > 0 and rp.counters[5] > 0 and rp.counters[1] > 0


def test_coverage_stream():
    s, rp, cs, _ = results('coverage')
    c = s.claims
    tid = s.records['tid']
    wave, lane, inside = c['changes']
    assert wave % 256 == 0 and lane % 4 == 0 and lane % 256 and inside % 4 == 2
    assert all(tid[i - 1] != tid[i] for i in c['changes'])
    assert c['big_sum'] <= rp.aligned[c['big_contig']] < 1 << 31 and c['big_sum'] > (1 << 31) - (1 << 16)
    assert len(set(tid[BLOCK:3 * BLOCK].tolist())) == 1 and (s.records['qlen'][BLOCK:3 * BLOCK] == 65535).all()
    one_each = tid[4 * SUB:4 * SUB + 600]
    assert len(set(one_each.tolist())) == 600
    assert (tid == -1).sum() >= 300 and (tid >= D.N_CONTIGS).sum() >= 300
    absent = set(D.rows_of('absent'))
    mt = s.records['mtid']
    assert any(t in absent and m not in absent and t != m for t, m in zip(tid.tolist(), mt.tolist()))
    assert any(m in absent and t not in absent and t != m for t, m in zip(tid.tolist(), mt.tolist()))
    q = s.records['mapq']
    assert ((q > 0) & (q < s.lib['min_mapq'])).sum() >= 200 and (q == 0).sum() >= 20


@pytest.mark.parametrize('mutation', D.MUTATIONS)
def test_every_wrong_rule_changes_what_its_stream_expects(mutation):
    """No deliberately wrong kernel is built: the restated loop with one rule wrong gives other counters, coverage or tuples
    on the stream designed for that rule, so a kernel with that rule wrong cannot equal the oracle there."""
    s, rp, _, _ = results(D.MUTATION_TARGETS[mutation])
    wrong = D.replay(s.records, D.TABLE, s.lib, mutate=mutation)
    assert (wrong.counters, wrong.aligned, wrong.tuples) != (rp.counters, rp.aligned, rp.tuples)
