"""The designs of tests/exchange_design.py checked without a GPU: every named case is really in its inputs (the census),
the model's owner hash is the library's, its partition and unpack are what tests/dist_util.OracleBackend does where that
stand-in applies (no heads, no rider), its head replay - cut at every record that reaches CreateEdge - composes the
slice-local runs of oracle.py_oracle.record_loop into the whole stream's run, and every named wrong model changes the
expectation of the design that is there to catch it.  tests/test_gpu_exchange_borders.py then holds the kernels against
the same model."""
import numpy as np
import pytest

from tests import exchange_design as XD

DESIGNS = XD.all_designs()


def test_the_knobs_are_the_sources():
    """The form constants come from the sources; the capacities on the two switches follow them."""
    k = XD.source_knobs()
    assert XD.SMALL_TILE == k['THREADS'] * k['SMALL_ITEMS'] and XD.SORT_TILE == k['THREADS'] * k['SORT_ITEMS']
    assert XD.SMALL_TILE < XD.SORT_TILE, 'the small tile is no longer smaller than the sort tile: the form designs are void'
    assert XD.SCAN_FREE_CAP < XD.SMALL_TILE_CAP, \
        'BESST_SCAN_FREE_MAX_BLOCKS small tiles now reach beyond BESST_MSD_MAX_BLOCKS sort tiles: the row-scanned small-tile form is gone'
    assert [XD.form_of(c)[0] for c in (XD.SCAN_FREE_CAP, XD.SCAN_FREE_CAP + 1, XD.SMALL_TILE_CAP, XD.SMALL_TILE_CAP + 1)] == \
        [XD.FORMS[0], XD.FORMS[1], XD.FORMS[1], XD.FORMS[2]]


@pytest.mark.parametrize('name', list(DESIGNS))
def test_census_confirms_the_design(name):
    ex = DESIGNS[name]
    c = XD.census(ex)
    assert ex.claims, 'a design without a claim'
    for text, holds in ex.claims:
        print('%s: %s' % (name, text))
        assert holds(c), '%s: not in the inputs - %s' % (name, text)
    for s, src in enumerate(ex.sources):
        assert len(src.keys) >= src.cap and len(src.payload) >= src.cap
        assert (src.rider is None) == (ex.sources[0].rider is None)
        assert src.rider is None or len(src.rider) == len(ex.sources[0].rider)
        n = min(src.n_reported, src.cap)
        assert n == 0 or int(src.keys[:n].max()).bit_length() <= 2 * ex.node_bits + 1
    assert ex.pair_cap > 0 and ex.pair_cap % 2 == 0
    if ex.round_trip:
        assert not ex.speculative and not any(XD.census(ex, s).truncated for s in range(ex.world))


def test_every_form_has_a_design_on_each_side_of_its_switches():
    caps = {}
    for name, ex in DESIGNS.items():
        for s in ex.sources:
            caps.setdefault(XD.form_of(s.cap)[0], set()).add(s.cap)
    assert set(caps) == set(XD.FORMS)
    assert XD.SCAN_FREE_CAP in caps[XD.FORMS[0]] and XD.SCAN_FREE_CAP + 1 in caps[XD.FORMS[1]]
    assert XD.SMALL_TILE_CAP in caps[XD.FORMS[1]] and XD.SMALL_TILE_CAP + 1 in caps[XD.FORMS[2]]
    full = [ex for ex in DESIGNS.values() if XD.census(ex).n in (XD.SCAN_FREE_CAP, XD.SCAN_FREE_CAP + 1)]
    assert len(full) == 2, 'the capacities on the first switch also run full'
    assert {ex.world for ex in DESIGNS.values()} >= {1, 2, 3, 8, 64, 255, 256}
    assert {XD.census(ex).n for n, ex in DESIGNS.items() if n.startswith('sizes_n_')} >= set(XD.SIZES)


def test_overflow_sits_on_each_side_of_pair_capacity():
    seen = set()
    for name, ex in DESIGNS.items():
        if name.startswith('overflow_'):
            c = XD.census(ex)
            seen.add((ex.pair_cap, int(c.totals[1]) - ex.pair_cap))
    for pc in (2, 64, XD.SMALL_TILE + 2):
        assert {(pc, -1), (pc, 0), (pc, 1)} <= seen, pc
    assert (64, 64) in seen


def test_owner_is_the_library_hash():
    """owner() against besst_owner_of_scaffold over 0 .. 2^20 and a sample above 2^27 (the library loads without a GPU)."""
    from besst_amd import _lib
    lib = _lib.load()
    f = lib.besst_owner_of_scaffold
    ids = np.arange(1 << 20, dtype=np.uint64)
    for world in (3, 256):
        want = XD.owners_of_keys(ids << np.uint64(2 + 16), 16, world).tolist()
        for s in range(1 << 20):
            if f(s, world) != want[s]:
                raise AssertionError('scaffold %d, world %d: library %d, model %d' % (s, world, f(s, world), want[s]))
    sample = list(range(0, 1 << 20, 997)) + [(1 << 27) + 12_345 * j for j in range(2000)] + [(1 << 32) - 1, (1 << 31), (1 << 31) - 1]
    for world in (1, 2, 3, 8, 64, 255, 256):
        for s in sample:
            assert f(s, world) == XD.owner(s, world), (s, world)
    nb = 29
    k = (np.array(sample[-2003:-3], dtype=np.uint64) * np.uint64(2) + np.uint64(1)) << np.uint64(nb + 1)
    assert XD.owners_of_keys(k, nb, 255).tolist() == [XD.owner(s, 255) for s in sample[-2003:-3]]


def _oracle_backend(ex, s, rank):
    """tests/dist_util.OracleBackend around the tuples of source s (its partition and unpack need nothing else)."""
    from besst_amd import _lib
    from tests import dist_util as DU
    src = ex.sources[s]
    n, nb = min(src.n_reported, src.cap), ex.node_bits
    b = object.__new__(DU.OracleBackend)
    b.lib, b.nb, b.rank, b.world, b.pair_cap = _lib.load(), nb, rank, ex.world, ex.pair_cap
    b.region = 64 + ex.pair_cap * 20
    b.overflow = False
    res = type('Res', (), {})()
    k, pl = src.keys[:n].tolist(), src.payload[:n].tolist()
    res.tuples = [(key >> (1 + nb), (key >> 1) & ((1 << nb) - 1), key & 1, p & 0xffffffff, (p >> 32) & 0x3fffffff, p >> 62)
                  for key, p in zip(k, pl)]
    b.res = res
    return b


PLAIN = [n for n, ex in DESIGNS.items() if not ex.speculative and XD.rider_bytes_of(ex) == 0]


@pytest.mark.parametrize('name', PLAIN)
def test_model_is_the_oracle_backend_where_that_applies(name):
    """No heads, no rider - every world and every capacity (the stand-in takes the first n tuples): the send buffer (the
    defined bytes; the stand-in starts from zeros, the model from the canary) and what the receivers unpack (worlds 255
    and 256: the design's sample of ranks)."""
    import torch
    ex = DESIGNS[name]
    parts = XD.model_partitions(ex)
    sends = []
    for s in range(ex.world):
        got = _oracle_backend(ex, s, s).partition().numpy()
        a, b = XD.render(parts[s], ex.pair_cap, 0, 0xA5), XD.render(parts[s], ex.pair_cap, 0, 0x5A)
        defined = a == b
        assert np.array_equal(got[defined], a[defined]), 'source %d' % s
        assert not got[~defined].any()
        sends.append(got)
    region = XD.stride_bytes(ex.pair_cap, 0)
    for r in XD.ranks_of(ex):
        b = _oracle_backend(ex, 0, r)
        b.unpack(torch.from_numpy(np.concatenate([sends[s][r * region:(r + 1) * region] for s in range(ex.world)])))
        want = XD.model_unpack(ex, r, parts)
        assert [t[0] for t in b.recv] == want.keys.tolist()
        assert [t[1] for t in b.recv] == want.payload.tolist()
        assert [t[2] for t in b.recv] == want.gidx.tolist()
        assert bool(b.overflow) == want.overflow and len(b.recv) == want.n_out


# ---- the head replay against the oracle ------------------------------------------------------------------------------------
COUNTERS = ('count', 'non_unique', 'non_unique_for_scaf', 'nr_of_duplicates', 'too_long', 'fishy_reads')


def _run(rec, lo, hi, table, p, res=None):
    from oracle import py_oracle as O
    if res is None:
        res = O.LoopResult(len(table['cls']))
        res.tuples = []
    O.record_loop({k: v[lo:hi] for k, v in rec.items()}, table, p, res=res)
    return res


def _words(res):
    return [getattr(res, k) for k in COUNTERS] + [len(res.tuples), res.n_reach]


def _describe(rec, table, p):
    """Per record, from the oracle alone: does it reach CreateEdge, and if so (obs1, obs2, flags) - the record run on its own
    WITHOUT detect_duplicate, so that the number of calls is count + too_long."""
    from oracle import py_oracle as O
    import copy
    q = copy.copy(p)
    q.detect_duplicate = False
    res = O.LoopResult(len(table['cls']))
    res.tuples = []
    out = {}
    for i in range(len(rec['tid'])):
        before = (res.n_reach, res.count, res.too_long, res.non_unique_for_scaf)
        res.prev = (-7, -7)
        O.record_loop({k: v[i:i + 1] for k, v in rec.items()}, table, q, res=res)
        if res.n_reach != before[0]:
            c, l, m = res.count - before[1], res.too_long - before[2], res.non_unique_for_scaf - before[3]
            out[i] = (res.prev[0], res.prev[1], (1 if c else 0) | (2 if c + l == 2 else 0) | (4 if m else 0) | (8 if c else 0))
    return out


def _slices_as_exchange(rec, table, p, cuts, heads, cache, node_bits):
    """The slices [cuts[j], cuts[j + 1]) as sources of an exchange: their tuples from the slice-local oracle run, their
    descriptions from it and from `heads`; -> (Exchange, the slices' counters without their heads' own calls)."""
    world = len(cuts) - 1
    sources, words = [], []
    for j in range(world):
        lo, hi = cuts[j], cuts[j + 1]
        if (lo, hi) not in cache:
            res = _run(rec, lo, hi, table, p)
            reaching = [i for i in heads if lo <= i < hi]     # (heads: every reaching record of the stream, ascending)
            info = XD._info()
            w = _words(res)
            if reaching:
                h = reaching[0]
                alone = _run(rec, h, h + 1, table, p)         # the head's own calls against (-1, -1), as the slice-local run made them
                before = _run(rec, lo, h, table, p)           # the tuples in front of the head's: fishy ones
                assert before.n_reach == 0 and alone.n_reach == 1
                o1, o2, flags = heads[h]
                assert bool(flags & 8) == (len(alone.tuples) == 1)
                info = XD._info(1, res.prev, 1, (o1, o2), flags, len(before.tuples) if flags & 8 else -1)
                for k in (0, 2, 3, 4):
                    w[k] -= _words(alone)[k]
            t = res.tuples
            keys = np.array([(((u << node_bits) | v) << 1) | f for u, v, f, _, _, _ in t], dtype=np.uint64)
            payload = np.array([ou | ((ov | (mask << 30)) << 32) for _, _, _, ou, ov, mask in t], dtype=np.uint64)
            cache[(lo, hi)] = (XD.Source(keys, payload, len(t), len(t), None, info), w)
        sources.append(cache[(lo, hi)][0])
        words.append(cache[(lo, hi)][1])
    ex = XD.Exchange('slices', world, 1 << 20, node_bits, sources, True, bool(p.detect_duplicate), None, [], False, False)
    return ex, words


REPLAY_STREAMS = ['chain_detect', 'chain_count'] + ['rules%d' % k for k in range(6)]


@pytest.mark.parametrize('stream', REPLAY_STREAMS)
def test_head_replay_composes_slice_local_oracle_runs(stream):
    """The stream cut at EVERY record that reaches CreateEdge, into two slices (the cut) and three (the cut and the next
    reaching record; for the last one, the one before): the slice-local oracle runs, the model's partition of their
    tuples and its unpack on every rank - head replay, dropped tuples, shifted emit indexes, counter corrections - must
    give the whole stream's oracle counters, tuples and emit indexes."""
    from tests import record_design as RD
    s = RD.chain_stream(stream == 'chain_detect') if stream.startswith('chain') else RD.rules_stream(int(stream[-1]))
    rec, table, p = RD.as_oracle_inputs(s)
    n = len(rec['tid'])
    whole = _run(rec, 0, n, table, p)
    want_words = _words(whole)
    nb = RD.NODE_BITS
    want_keys = [(((u << nb) | v) << 1) | f for u, v, f, _, _, _ in whole.tuples]
    want_payload = [ou | ((ov | (mask << 30)) << 32) for _, _, _, ou, ov, mask in whole.tuples]
    heads = _describe(rec, table, p)
    reaching = sorted(heads)
    assert len(reaching) == whole.n_reach and len(reaching) >= 20
    cache = {}
    dropped = 0
    for k, c in enumerate(reaching):
        other = reaching[k + 1] if k + 1 < len(reaching) else reaching[k - 1]
        for cuts in ([0, c, n], [0] + sorted((c, other)) + [n]):
            ex, words = _slices_as_exchange(rec, table, p, cuts, heads, cache, nb)
            parts = XD.model_partitions(ex)
            got, corr = [], None
            for r in range(ex.world):
                u = XD.model_unpack(ex, r, parts)
                assert not u.overflow
                assert corr is None or corr == u.corrections, 'the ranks disagree on the corrections'
                corr = u.corrections
                assert set(XD.owners_of_keys(u.keys, nb, ex.world).tolist()) <= {r}
                got += list(zip(u.gidx.tolist(), u.keys.tolist(), u.payload.tolist()))
            got.sort()
            dropped += -corr[6]
            assert [g[0] for g in got] == list(range(len(want_keys))), (stream, cuts)
            assert [g[1] for g in got] == want_keys and [g[2] for g in got] == want_payload, (stream, cuts)
            total = [sum(w[j] for w in words) + corr[j] for j in range(8)]
            assert total == want_words, (stream, cuts, total, want_words)
    if p.detect_duplicate and whole.nr_of_duplicates:
        assert dropped > 0, 'no cut put a slice head on a duplicate'
    print('%s: %d cuts, %d heads dropped at their owners' % (stream, len(reaching), dropped))


# ---- the wrong models -----------------------------------------------------------------------------------------------------------
def _expectation(ex, wrong=None):
    parts = XD.model_partitions(ex, wrong)
    images = [XD.render(p, ex.pair_cap, XD.rider_bytes_of(ex)) for p in parts]
    ups = [XD.model_unpack(ex, r, parts, wrong) for r in XD.ranks_of(ex)]
    return images, ups


def _same(a, b):
    if any(not np.array_equal(x, y) for x, y in zip(a[0], b[0])):
        return False
    for x, y in zip(a[1], b[1]):
        for f in x._fields:
            if not np.array_equal(np.asarray(getattr(x, f)), np.asarray(getattr(y, f))):
                return False
    return True


def test_there_are_twelve_wrong_models():
    assert len(XD.WRONG_MODELS) >= 12
    assert all(case in DESIGNS for _, case in XD.WRONG_MODELS.values())


@pytest.mark.parametrize('wrong', list(XD.WRONG_MODELS))
def test_wrong_model_changes_its_named_case(wrong):
    what, case = XD.WRONG_MODELS[wrong]
    print('%s (%s) is told apart by %s' % (wrong, what, case))
    ex = DESIGNS[case]
    assert not _same(_expectation(ex), _expectation(ex, wrong)), '%s expects the same of %s as the model' % (wrong, case)


def test_shift_at_ge_drop_is_no_wrong_model():
    """`idx >= drop` instead of `idx > drop`: the same output on every design and every rank, because no receiver ever holds
    the tuple whose idx IS the drop (see exchange_design.EQUIVALENT_MODELS)."""
    for name, ex in DESIGNS.items():
        if ex.speculative:
            assert _same(_expectation(ex), _expectation(ex, 'shift_ge_drop')), name
