"""The multi-GPU exchange at its borders: besst_dev_partition and besst_dev_unpack called directly on the designs of
tests/exchange_design.py (what each one holds, and why, is checked without a GPU in tests/test_exchange_design.py), the
reduction on the receiver's global emit indexes behind them, the heads of real slices through distributed.HipBackend,
and stage 2 in every form with a first_map.

  partition    the send buffer of every source == the model byte for byte: headers, the written prefix of the three
               columns, the rider, and the canary everywhere else - in every form, size, world and overflow design
  unpack       the receive buffers assembled by the tensor shuffle of tests/test_gpu_distributed_sim.py; keys, payload and
               gidx up to n_out (and the canary behind them), n_out, the overflow flag, the rider sums or `counters`,
               all_slice_info == the model on every rank (worlds 255 and 256: the five ranks the design names)
  round trip   untruncated designs: partition -> shuffle -> unpack -> besst_dev_reduce with gidx as first_map; the union of
               the owners' rows == oracle.c_oracle.edge_rows of the whole stream, owners disjoint and complete - on every
               rank of every world, 255 and 256 included
  heads        record_design's chain and rules streams cut so that a slice head lies in the slice's first block, behind one
               and behind three blocks without a reaching record, on a duplicate, on a double call with mapq 0, on a record
               that is not accepted, with a slice in the middle that reaches nothing; the heads behind empty blocks also
               with BESST_STITCH_SPAN 1 and 2, so that the head lies in another stitch span than the slice's first block:
               rows, counters and coverage == the single-process oracle
  mapped       every stream of tests/test_gpu_sort_classes.py with a first_map: strictly increasing with irregular steps,
               and the same beginning at 0xF0000000 (indexes at and above 2^31)

Everything is an integer: equality, no tolerance.  Every call is made twice on the same buffers."""
import ctypes as C
import types

import numpy as np
import pytest

from tests import exchange_design as XD
from tests import sort_design as SD

pytestmark = pytest.mark.gpu

DESIGNS = XD.all_designs()
OUT_CANARY = -0x5A5A5A5A5A5A5A5B                              # what the unpack outputs hold before a call
COUNTER_BASE = [1000 + 7 * k for k in range(8)]
_MODEL, _SENDS = {}, {}


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _stream(dev):
    import torch
    return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _i64(a, dev):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).to(dev)


def model(name):
    """(the model's regions, its send buffer images) of the design used last: one design is kept at a time."""
    if name not in _MODEL:
        ex = DESIGNS[name]
        parts = XD.model_partitions(ex)
        _MODEL.clear()
        _MODEL[name] = (parts, [XD.render(p, ex.pair_cap, XD.rider_bytes_of(ex)) for p in parts])
    return _MODEL[name]


def partition_on_gpu(name):
    """Every source's send buffer after the first and after the second call (host copies).  Only the design used last is
    kept (world 256 alone is 256 sources x 2 images x 256 regions): a test that comes back to a design partitions again."""
    if name in _SENDS:
        return _SENDS[name]
    import torch
    from besst_amd import _lib
    lib = _lib.load()
    ex = DESIGNS[name]
    dev = torch.device('cuda', 0)
    rider_bytes = XD.rider_bytes_of(ex)
    stride = XD.stride_bytes(ex.pair_cap, rider_bytes)
    assert stride == lib.besst_dev_exchange_stride_bytes(ex.pair_cap, rider_bytes)
    out = []
    for src in ex.sources:
        assert len(src.keys) >= src.cap and len(src.payload) >= src.cap      # the kernels read up to the capacity
        keys, payload = _i64(src.keys, dev), _i64(src.payload, dev)
        cnt = torch.tensor([src.n_reported], dtype=torch.int32, device=dev)
        rider = _i64(src.rider, dev) if rider_bytes else None
        info = torch.from_numpy(src.slice_info).to(dev) if src.slice_info is not None else None
        ws = torch.empty(lib.besst_dev_reduce_workspace_bytes(max(src.cap, 1)), dtype=torch.uint8, device=dev)
        send = torch.full((ex.world * stride,), XD.CANARY, dtype=torch.uint8, device=dev)
        images = []
        for _ in range(2):                                   # the second call starts from the first one's leftovers
            _lib.check(lib.besst_dev_partition(_stream(dev), src.cap, _p(cnt), ex.node_bits, ex.world, _p(keys), _p(payload),
                                               ex.pair_cap, _p(send), _p(ws), ws.numel(), _p(rider), rider_bytes, _p(info)),
                       'partition')
            torch.cuda.synchronize()
            images.append(send.cpu().numpy().copy())
        out.append(images)
        del keys, payload, ws, send
    _SENDS.clear()
    _SENDS[name] = out
    return out


def assert_partitions(name):
    _, want = model(name)
    for s, images in enumerate(partition_on_gpu(name)):
        for call, got in enumerate(images):
            if not np.array_equal(got, want[s]):
                at = int(np.nonzero(got != want[s])[0][0])
                stride = len(got) // DESIGNS[name].world
                raise AssertionError('%s: source %d, call %d: the send buffer differs from the model at byte %d (region %d, '
                                     'offset %d): %d, want %d' % (name, s, call, at, at // stride, at % stride, got[at], want[s][at]))


@pytest.mark.parametrize('name', list(DESIGNS))
def test_partition_equals_the_model(name):
    assert_partitions(name)


def unpack_on_gpu(name, rank):
    """-> dict of host arrays after the second call (the first call's are compared with them before it returns)."""
    import torch
    from besst_amd import _lib
    lib = _lib.load()
    ex = DESIGNS[name]
    dev = torch.device('cuda', 0)
    rider_bytes = XD.rider_bytes_of(ex)
    stride = XD.stride_bytes(ex.pair_cap, rider_bytes)
    sends = partition_on_gpu(name)
    recv = torch.from_numpy(np.concatenate([sends[s][1][rank * stride:(rank + 1) * stride] for s in range(ex.world)])).to(dev)
    slots = ex.world * ex.pair_cap
    keys = torch.full((slots,), OUT_CANARY, dtype=torch.int64, device=dev)
    payload = torch.full((slots,), OUT_CANARY, dtype=torch.int64, device=dev)
    gidx = torch.full((slots,), -0x5A5A5A5B, dtype=torch.int32, device=dev)
    flags = torch.zeros(2, dtype=torch.int32, device=dev)
    rider_sum = torch.full((rider_bytes // 8,), OUT_CANARY, dtype=torch.int64, device=dev) if rider_bytes else None
    all_info = torch.full((ex.world * 8,), -77, dtype=torch.int32, device=dev) if ex.speculative and not ex.null_all_info else None
    counters = torch.tensor(COUNTER_BASE, dtype=torch.int64, device=dev) if ex.speculative else None
    results = []
    for _ in range(2):
        flags.zero_()                                        # (as the builder's reset does before every step)
        if counters is not None:
            counters.copy_(torch.tensor(COUNTER_BASE, dtype=torch.int64))
        _lib.check(lib.besst_dev_unpack(_stream(dev), ex.world, ex.pair_cap, _p(recv), _p(keys), _p(payload), _p(gidx),
                                        C.c_void_p(flags.data_ptr()), C.c_void_p(flags.data_ptr() + 4), _p(rider_sum),
                                        rider_bytes, 1 if ex.speculative else 0, rank, 1 if ex.detect and ex.speculative else 0,
                                        _p(all_info), _p(counters)), 'unpack')
        torch.cuda.synchronize()
        h = lambda t: None if t is None else t.cpu().numpy().copy()
        results.append(dict(keys=h(keys), payload=h(payload), gidx=h(gidx), flags=h(flags), rider_sum=h(rider_sum),
                            all_info=h(all_info), counters=h(counters)))
    for k in results[0]:
        assert np.array_equal(results[0][k], results[1][k]), '%s: rank %d: %s differs between the two calls' % (name, rank, k)
    return results[1]


def assert_unpacked(name, rank, got):
    ex = DESIGNS[name]
    parts, _ = model(name)
    want = XD.model_unpack(ex, rank, parts)
    n = want.n_out
    where = '%s: rank %d: ' % (name, rank)
    assert got['flags'].tolist() == [n, 1 if want.overflow else 0], where + 'n_out, overflow'
    assert np.array_equal(got['keys'][:n].view(np.uint64), want.keys), where + 'keys'
    assert np.array_equal(got['payload'][:n].view(np.uint64), want.payload), where + 'payload'
    assert np.array_equal(got['gidx'][:n].view(np.uint32), want.gidx), where + 'gidx'
    assert (got['keys'][n:] == OUT_CANARY).all() and (got['payload'][n:] == OUT_CANARY).all() and \
        (got['gidx'][n:] == -0x5A5A5A5B).all(), where + 'something was written behind n_out'
    if want.rider_sum is not None:
        assert np.array_equal(got['rider_sum'].view(np.uint64), want.rider_sum), where + 'rider sums'
    if ex.speculative:
        base = COUNTER_BASE if want.rider_sum is not None else [(b + c) % (1 << 64) for b, c in zip(COUNTER_BASE, want.corrections)]
        assert got['counters'].view(np.uint64).tolist() == base, where + 'counters'
        if not ex.null_all_info:
            assert np.array_equal(got['all_info'].reshape(ex.world, 8), want.all_slice_info), where + 'all_slice_info'
    return want


@pytest.mark.parametrize('name', list(DESIGNS))
def test_unpack_equals_the_model(name):
    assert_partitions(name)                                  # (no receive buffer is built from a send buffer that is off)
    for rank in XD.ranks_of(DESIGNS[name]):
        assert_unpacked(name, rank, unpack_on_gpu(name, rank))


ROUND_TRIPS = [n for n, ex in DESIGNS.items() if ex.round_trip]


@pytest.mark.parametrize('name', ROUND_TRIPS)
def test_round_trip_gives_the_whole_streams_edge_table(name):
    """partition -> shuffle -> unpack -> besst_dev_reduce (first_map = gidx) on EVERY rank of the world - 255 and 256
    too, where owner 255 is also the digit of the lanes behind n."""
    from oracle import c_oracle as CO
    from tests.test_gpu_runs import run_reduce
    ex = DESIGNS[name]
    assert_partitions(name)
    keys, payload = XD.whole_stream(ex)
    want = CO.edge_rows(keys, payload)
    cols = {k: [] for k in ('key', 'n', 'sum_obs', 'sum_obs_sq', 'first_idx', 'mask')}
    obs = {}
    for rank in range(ex.world):
        got = unpack_on_gpu(name, rank)
        n = int(got['flags'][0])
        assert not got['flags'][1]
        if n == 0:
            continue
        k, pl, g = got['keys'][:n].view(np.uint64), got['payload'][:n].view(np.uint64), got['gidx'][:n].view(np.uint32)
        assert set(XD.owners_of_keys(k, ex.node_bits, ex.world).tolist()) == {rank}
        gb, r = run_reduce(k.copy(), pl.copy(), ex.node_bits, cap=max(n, 1024), first_map=g.copy())
        get = lambda t, m, dt: t[:m].cpu().numpy().view(dt)
        row_key = get(gb.row_key, r, np.uint64)
        cols['key'].append(row_key)
        cols['n'].append(get(gb.row_n, r, np.uint32).astype(np.int64))
        cols['sum_obs'].append(get(gb.row_sum, r, np.int64))
        cols['sum_obs_sq'].append(get(gb.row_sum_sq, r, np.int64))
        cols['first_idx'].append(get(gb.row_first, r, np.uint32).astype(np.int64))
        cols['mask'].append(get(gb.row_mask, r, np.uint32).astype(np.int64))
        off = get(gb.row_offset, r, np.uint32).astype(np.int64)
        lo, hi = get(gb.obs_lo, n, np.int32), get(gb.obs_hi, n, np.int32)
        for j in range(r):
            obs[int(row_key[j])] = (lo[off[j]:off[j] + cols['n'][-1][j]].tolist(), hi[off[j]:off[j] + cols['n'][-1][j]].tolist())
    if not len(keys):
        assert not cols['key']
        return
    key = np.concatenate(cols['key'])
    order = np.argsort(key, kind='stable')
    assert np.array_equal(key[order], want['key']), 'the owners\' rows are not the whole stream\'s, each once'
    for c in ('n', 'sum_obs', 'sum_obs_sq', 'first_idx', 'mask'):
        assert np.array_equal(np.concatenate(cols[c])[order], want[c]), c
    for j, kk in enumerate(want['key'].tolist()):
        a, b = int(want['offset'][j]), int(want['offset'][j] + want['n'][j])
        assert obs[kk] == (want['obs_lo'][a:b].tolist(), want['obs_hi'][a:b].tolist()), 'observations of row %d' % j


def test_errors_return_before_any_launch():
    """World 0 and 257, an odd and a zero pair_capacity, a rider of 12 bytes, a rider of 8 bytes or a rank outside the world
    with speculative heads: a non-zero status, a message, and every buffer as it was."""
    import torch
    from besst_amd import _lib
    lib = _lib.load()
    dev = torch.device('cuda', 0)
    world, pair_cap, n = 3, 8, 20
    keys = _i64(XD.make_keys(np.arange(n) % world, world, 16), dev)
    payload = _i64(np.arange(n, dtype=np.uint64), dev)
    cnt = torch.tensor([n], dtype=torch.int32, device=dev)
    ws = torch.empty(lib.besst_dev_reduce_workspace_bytes(n), dtype=torch.uint8, device=dev)
    send = torch.full((world * XD.stride_bytes(pair_cap, 64) + 4096,), XD.CANARY, dtype=torch.uint8, device=dev)
    rider = torch.zeros(8, dtype=torch.int64, device=dev)
    outs = [torch.full((world * pair_cap + 64,), OUT_CANARY, dtype=torch.int64, device=dev) for _ in range(4)]
    small = [torch.full((64,), -77, dtype=torch.int32, device=dev) for _ in range(3)]
    for what, stage, change in XD.ERROR_CASES:
        a = dict(world=world, pair_cap=pair_cap, rider_bytes=0, speculative=0, rank=0)
        a.update(change)
        if stage == 'partition':
            rc = lib.besst_dev_partition(_stream(dev), n, _p(cnt), 16, a['world'], _p(keys), _p(payload), a['pair_cap'], _p(send),
                                         _p(ws), ws.numel(), _p(rider), a['rider_bytes'], None)
        else:
            rc = lib.besst_dev_unpack(_stream(dev), a['world'], a['pair_cap'], _p(send), _p(outs[0]), _p(outs[1]), _p(small[0]),
                                      C.c_void_p(small[1].data_ptr()), C.c_void_p(small[1].data_ptr() + 4), _p(outs[2]),
                                      a['rider_bytes'], a['speculative'], a['rank'], 1, _p(small[2]), _p(outs[3]))
        assert rc != 0, '%s (%s) was accepted' % (what, stage)
        message = _lib.last_error()
        assert stage in message, '%s: the message does not name the stage: %r' % (what, message)
        torch.cuda.synchronize()
        assert bool((send == XD.CANARY).all()), what
        assert all(bool((t == OUT_CANARY).all()) for t in outs) and all(bool((t == -77).all()) for t in small), what


# ---- the heads of real slices ----------------------------------------------------------------------------------------------
def _rules_cut():
    """In rules1 (min_mapq 0, the double call): the first record behind the stream's first quarter that reaches CreateEdge
    with mapq 0 on two large contigs of different scaffolds."""
    from tests import record_design as D
    s = D.rules_stream(1)
    rp = D.replay(s.records, D.TABLE, s.lib)
    rec = s.records
    for i in range(len(rec['tid']) // 4, len(rec['tid'])):
        if rp.reach[i] and rec['mapq'][i] == 0 and D.TABLE['cls'][rec['tid'][i]] == D.CLS_LARGE and \
                D.TABLE['cls'][rec['mtid'][i]] == D.CLS_LARGE:
            return i
    raise AssertionError('rules1 holds no such record')


def _head_cases():
    from tests import record_design as D
    B = D.BLOCK
    cases = []
    for stream in ('chain_detect', 'chain_count'):
        cases += [(stream, [44], 'the head is a duplicate, in the slice\'s first block'),
                  (stream, [166], 'the head is a duplicate that is not accepted'),
                  (stream, [160, 2 * B], 'a head that is not accepted; a head behind one block without a reaching record'),
                  (stream, [1300, 16000, 4 * B], 'a middle slice that reaches nothing; a head behind three such blocks')]
    cases = [c + (None,) for c in cases]
    # BESST_STITCH_SPAN 1 and 2 (blocks per stitch span): the slice head then lies in another span than the slice's first block
    cases += [c[:3] + (span,) for c in cases if 'behind' in c[2] for span in ('1', '2')]
    cases.append(('rules1', [None, None], 'the head is a double call with mapq 0', None))
    return cases


@pytest.mark.parametrize('stream,cuts,what,span', _head_cases())
def test_slice_heads_end_to_end(stream, cuts, what, span, monkeypatch):
    """The record loop feeds the headers (classify_emit_speculative); rows, counters and coverage against the single-process
    oracle, as tests/test_gpu_distributed_sim.test_slice_boundary_right_before_a_duplicate compares them."""
    if span is None:
        monkeypatch.delenv('BESST_STITCH_SPAN', raising=False)
    else:
        monkeypatch.setenv('BESST_STITCH_SPAN', span)
    import torch
    from besst_amd import distributed
    from tests import dist_util as DU
    from tests import record_design as D
    s = D.all_streams()[stream]
    batch = D.as_batch(s)
    n = len(batch)
    if cuts[0] is None:
        c = _rules_cut()
        cuts = [c, c + (n - c) // 2]
    rp = D.replay(s.records, D.TABLE, s.lib)
    bounds = [0] + cuts + [n]
    world = len(bounds) - 1
    if 'middle slice' in what:
        assert not rp.reach[bounds[1]:bounds[2]].any()
    if 'three such blocks' in what:
        head = bounds[-2] + int(np.nonzero(rp.reach[bounds[-2]:])[0][0])
        assert head // D.BLOCK - bounds[-2] // D.BLOCK == 3 and bounds[-2] % D.BLOCK == 0
    if 'behind one block' in what:
        head = bounds[2] + int(np.nonzero(rp.reach[bounds[2]:])[0][0])
        assert (head - bounds[2]) // D.BLOCK == 1
    if 'duplicate' in what:
        assert rp.reach[cuts[0]] and rp.dup[cuts[0]]
    if 'not accepted' in what:
        assert rp.reach[cuts[0]] and not rp.accept[cuts[0]]
    if 'mapq 0' in what:
        assert rp.reach[cuts[0]] and s.records['mapq'][cuts[0]] == 0 and s.lib['extend_paths'] and not s.lib['no_score']
    wl = dict(asm=types.SimpleNamespace(nc=D.N_CONTIGS), node_bits=D.NODE_BITS, lib=s.lib, table=D.table_columns())
    want_rows, want = DU.expected_rows(batch, wl['table'], wl['lib'], wl['node_bits'])
    dev = torch.device('cuda', 0)
    backends = []
    for r in range(world):
        sub = dict(wl)
        sub['batch'] = batch.take(slice(bounds[r], bounds[r + 1]))
        backends.append(distributed.HipBackend(dev, sub, r, world, 4096))
    for _ in range(2):
        sends = []
        for b in backends:
            b.reset()
            b.classify_scan()
            b.classify_emit_speculative()
            sends.append(b.partition().clone())
        region = backends[0].region
        for r, b in enumerate(backends):
            b.unpack(torch.cat([sends[q][r * region:(r + 1) * region] for q in range(world)]))
            b.reduce()
        torch.cuda.synchronize()
    assert backends[0].sums_ride_exchange
    assert not any(b.overflowed() for b in backends)
    words = [want.count, want.non_unique, want.non_unique_for_scaf, want.nr_of_duplicates, want.too_long, want.fishy_reads,
             len(want.tuples), want.n_reach]
    merged = {}
    for b in backends:
        assert b.counter_words.cpu().tolist() == words
        assert b.aligned.cpu().tolist() == want.aligned
        rows = DU.rows_from_table(b.local_table())
        for k in rows:
            if k & 1:
                rows[k]['lo'] = [0] * rows[k]['n']
                rows[k]['hi'] = [0] * rows[k]['n']
        assert not set(rows) & set(merged)
        merged.update(rows)
    for k, r in want_rows.items():
        if k & 1:
            r['s'] = r['s2'] = 0
    assert merged == want_rows
    assert sum(int(b.flags.cpu()[0]) for b in backends) == len(want.tuples)


# ---- the mapped reduce in every form ---------------------------------------------------------------------------------------------
NO_RUNS = 1                                                  # pipeline.REDUCE_NO_RUNS (asserted below)
ZERO_CENSUS = [0] * 7


def first_maps(n):
    """Two global emit indexes for n tuples: strictly increasing with irregular steps, and the same beginning at 0xF0000000."""
    steps = np.random.default_rng(n).integers(1, 4, n).astype(np.int64)
    base = np.cumsum(steps) - steps + 7
    high = base - 7 + 0xF0000000
    assert n == 0 or (int(high[-1]) < 1 << 32 and (np.diff(base) > 0).all() and int(high[0]) >= 1 << 31)
    return [base.astype(np.uint32), high.astype(np.uint32)]


def reduce_mapped_and_check(keys, payload, key_bits, key_base, cap, flags, want_census):
    from besst_amd import pipeline
    from tests.test_gpu_runs import assert_rows, run_reduce
    assert pipeline.REDUCE_NO_RUNS == NO_RUNS
    node_bits = max(1, min(29, (key_bits - 1) // 2))
    for first_map in first_maps(len(keys)):
        gb, n_rows = run_reduce(keys, payload, node_bits, cap=cap, first_map=first_map, flags=flags, key_bits=key_bits,
                                key_base=key_base)
        assert gb.sort_flags == flags, 'read_sizes() repeated the call in another form'
        got = gb.reduce_census(cap or len(keys))
        assert got == list(want_census), SD.explain_census(got, want_census)
        assert_rows(gb, n_rows, keys, payload, first_map=first_map)
        del gb


@pytest.mark.parametrize('key_bits,big', [(25, False), (30, False), (37, False), (41, False), (37, True)])
def test_mapped_chained_scan_buckets(key_bits, big):
    """Chained scan + buckets: the wave kernel, its digit passes, the workgroup kernel in LDS and in global memory."""
    key_base = (3 << 45) + 12_345 if key_bits in (30, 41) else 0
    _, keys, payload = SD.chained_stream(key_bits, key_base=key_base, big=big)
    want = SD.chained_census(SD.predict_chained(keys, key_bits, key_base))
    assert all(want[1 + c] > 0 for c in (SD.WAVE, SD.WAVE_DIGIT, SD.WG_LDS, SD.WG_GLOBAL))
    reduce_mapped_and_check(keys, payload, key_bits, key_base, SD.LARGE_CAPACITY, NO_RUNS, want)


@pytest.mark.parametrize('n', [0, 1, 100])
def test_mapped_chained_scan_buckets_on_nearly_empty_streams(n):
    key_bits = 37
    keys, payload = SD.tiny_stream(n, key_bits)
    want = SD.chained_census(SD.predict_chained(keys, key_bits))
    assert want[1] >= (1 << 16) - n
    reduce_mapped_and_check(keys, payload, key_bits, 0, SD.LARGE_CAPACITY, NO_RUNS, want)


@pytest.mark.parametrize('key_bits,one_more,big', [(20, False, False), (20, True, False), (45, False, False), (45, True, False),
                                                   (20, True, True)])
def test_mapped_chained_scan_tile_reduction(key_bits, one_more, big):
    keys, payload = SD.tile_stream(key_bits, one_more=one_more, big=big)
    reduce_mapped_and_check(keys, payload, key_bits, 0, SD.LARGE_CAPACITY, NO_RUNS, [SD.FORM_CHAINED_TILES] + ZERO_CENSUS)


@pytest.mark.parametrize('key_bits,cap_factor,big', [(9, 1, False), (15, 1, False), (31, 1, False), (41, 1, False),
                                                     (31, 3, False), (31, 1, True)])
def test_mapped_msd_partition_buckets(key_bits, cap_factor, big):
    key_base = 77 << 40 if key_bits == 31 else 0
    _, keys, payload = SD.msd_stream(key_bits, key_base=key_base, big=big)
    want = SD.msd_census(SD.predict_msd(keys, key_bits, key_base))
    reduce_mapped_and_check(keys, payload, key_bits, key_base, cap_factor * len(keys), 0, want)


@pytest.mark.parametrize('one_chunk,big', [(False, False), (True, False), (False, True)])
def test_mapped_run_grouped_chunks(one_chunk, big):
    key_bits = 37
    keys, payload, _ = SD.runs_stream(key_bits, exactly_one_chunk=one_chunk, big=big)
    reduce_mapped_and_check(keys, payload, key_bits, 0, SD.LARGE_CAPACITY, 0, [SD.FORM_RUNS] + ZERO_CENSUS)
