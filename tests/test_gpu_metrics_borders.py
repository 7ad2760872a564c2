"""The library-metrics pass (csrc/metrics.hip: metrics_stage / tiles / place, the count-only form, value_hist_kernel, and the
host chunk loop of besst_ctx_metrics_sample) at its cut-offs and tile borders: the designed streams of
tests/metrics_design.py - tests/test_metrics_design.py shows without a GPU that every named case is in them and that the
model is the C oracle's statement - through the kernels, every comparison integer equality."""
import time

import numpy as np
import pytest
import torch

from besst_amd import device, pipeline
from oracle import c_oracle as CO
from tests import metrics_design as MD
from tests.dist_util import OracleMetricsBackend

pytestmark = pytest.mark.gpu

CAP = MD.CAP
_kept = {}


def _stream(name):
    if name not in _kept:
        _kept[name] = dict(dense=MD.dense_stream, small=MD.small_sparse_stream, large=MD.large_sparse_stream,
                           values=MD.value_stream, count=MD.count_stream)[name]()
    return _kept[name]


def _sampler(batch):
    """The records on the device, once per (stream, orientation) of the module."""
    dev = torch.device('cuda', 0)
    s = pipeline.DeviceMetricsSampler(dev, pipeline.DeviceRecords(batch, dev), MD.N_CONTIGS)
    s.set_top(MD.TOP_MASK)
    return s


def _first_difference(got, want):
    at = np.nonzero(got != want)[0]
    i = int(at[0])
    return '%d entries differ, the first at %s[%d]: %d, expected %d' % (len(at), 'isize' if i < CAP else 'contam', i % CAP,
                                                                       got[i], want[i])


@pytest.mark.parametrize('orientation', ['fr', 'rf'])
@pytest.mark.parametrize('name', ['dense', 'small', 'large', 'values'])
def test_sampling_form_on_every_named_case(name, orientation):
    s = _stream(name)
    sampler = _sampler(s.batch(orientation))
    model = s.model(orientation)
    assert len(s.cases) >= 6
    for case in s.cases:
        label = '%s / %s / %s' % (s.name, orientation, case.name)
        before = torch.tensor(case.before, dtype=torch.int64)
        want, want_state = model.emit(before, orientation, case.min_mapq, case.read_len, case.want_isize)
        got, state = sampler.emit(before.to(sampler.device), orientation, case.min_mapq, case.read_len, case.want_isize)
        got, state, want_state = got.cpu(), state.cpu().tolist(), want_state.tolist()
        # the whole buffer: the samples at their places and nothing anywhere else
        assert torch.equal(got, want), '%s: %s' % (label, _first_difference(got.numpy(), want.numpy()))
        assert state[3:6] == want_state[3:6], label
        a0, b0, _ = case.before
        live = (case.want_isize and a0 < CAP) or b0 < CAP
        if live or case.want_isize:
            assert [min(state[j], CAP) for j in (0, 1)] == [min(want_state[j], CAP) for j in (0, 1)], label
        if live:                                                # a call that begins with a live list counts exactly
            assert state[0:3] == want_state[0:3], label
        else:
            # both lists full - one that is not asked for counts as full -: the records are not looked at (metrics.hip,
            # launch_metrics' contract), so an unwanted A's count below the cap stays where it was
            assert state[0:3] == list(case.before), label
        assert state[6:8] == [0, 0], label


@pytest.mark.parametrize('n', [1, 3, 4, 5, 1023, 1024, 1025])
@pytest.mark.parametrize('name', ['dense', 'small'])
def test_count_only_form_sizes(name, n):
    # (the sparse stream from two records in front of tile 63's first top record: the third record of the slice counts)
    start = 0 if name == 'dense' else 63 * MD.TILE + MD.WAVE_RECORDS - 2
    for orientation in ('fr', 'rf'):
        part = _stream(name).batch(orientation).slice(start, start + n)
        want = OracleMetricsBackend(part, MD.TOP_MASK).count(orientation, MD.MIN_MAPQ, MD.READ_LEN)
        got = _sampler(part).count(orientation, MD.MIN_MAPQ, MD.READ_LEN).cpu()
        assert got.tolist() == want.tolist(), (name, n, orientation)
        if name == 'dense':
            assert want.tolist() == [(n + 2) // 3, n, (n + 1) // 3]
        elif n >= 3:
            assert want[1] >= 1


def test_count_only_form_second_turn_of_the_scan():
    s = _stream('count')
    assert -(-s.n // MD.SUB) > MD.COUNT_TURN
    for orientation in ('fr', 'rf'):
        sampler = _sampler(s.batch(orientation))
        want = s.model(orientation).count(orientation, MD.MIN_MAPQ, MD.READ_LEN)
        assert sampler.count(orientation, MD.MIN_MAPQ, MD.READ_LEN).cpu().tolist() == want.tolist()
        assert int(sampler.state[5]) == 0 and min(want.tolist()) > 0


@pytest.mark.parametrize('orientation', ['fr', 'rf'])
def test_host_chunk_loop_second_chunk(orientation):
    """besst_ctx_metrics_sample's loop (api.hip): 16 Mi records with 300 top records, then a dense tail - the second chunk is
    sized from that rate, B is cut in it and A fills exactly, on a later record.  Against the C oracle.
    (On an MI355X the call takes 0.4 - 0.5 ms and the test, with its 18 M generated records, half a second.)"""
    s = MD.chunk_loop_stream()
    b_cut, a_cut = MD.chunk_loop_present(s)
    batch = s.batch(orientation)
    nc = MD.N_CONTIGS
    one = np.ones(nc, np.int32)
    with device.GraphContext(0) as ctx:
        ctx.set_contigs(scaf_id=np.arange(1, nc + 1, dtype=np.int32), scaf_len=one * 1000, ctg_pos=one * 0, ctg_len=one * 1000,
                        direction=one.astype(np.uint8), cls=one.astype(np.uint8))
        ctx.push_records(batch)
        t0 = time.perf_counter()
        isize, contam, counts = ctx.metrics_sample(MD.TOP_MASK, orientation, MD.MIN_MAPQ, MD.READ_LEN, True)
        print('metrics_sample over %d records in two chunks: %.2f ms' % (s.n, 1e3 * (time.perf_counter() - t0)))
        isize, contam = isize.copy(), contam.copy()
    w_isize, w_contam, w = CO.metrics_sample(batch, MD.TOP_MASK, orientation, MD.MIN_MAPQ, MD.READ_LEN, True)
    assert [counts.n_isize, counts.n_contam, counts.counter_total, counts.sample_counter] == w.tolist()
    assert counts.n_isize == CAP and counts.sample_counter == CAP
    assert counts.records_scanned == s.n                        # the second chunk was read
    assert np.array_equal(isize, w_isize) and isize[-1] == a_cut + 1
    assert np.array_equal(contam, w_contam) and contam[-1] <= b_cut + 1


def _histogram_inputs():
    rng = np.random.default_rng(20255)
    lo, hi = np.iinfo(np.int32).min, np.iinfo(np.int32).max
    for n_bins in (1, 2, 4097):
        edge = np.array([-1, 0, n_bins - 1, n_bins, lo, hi, n_bins + 1, -n_bins], np.int32)
        for n in (0, 1, 255, 256, 257, 100_003):
            v = rng.integers(-3, n_bins + 3, n).astype(np.int32)
            k = min(n, len(edge))
            v[:k] = edge[:k]
            if n > 1:
                v[-1] = n_bins - 1
            yield n_bins, v
        yield n_bins, np.full(100_003, n_bins - 1, np.int32)    # every value equal: one counter takes every add
        yield n_bins, np.full(257, n_bins, np.int32)            # ... and every value just outside
        yield n_bins, np.array([0], np.int32)


def test_value_histogram_edges():
    with device.GraphContext(0) as ctx:
        for n_bins, v in _histogram_inputs():
            ok = (v >= 0) & (v < n_bins)
            want = np.bincount(v[ok], minlength=n_bins)
            hist, overflow = ctx.value_histogram(v, n_bins)
            assert hist.shape == (n_bins,) and np.array_equal(hist, want), (n_bins, len(v))
            assert overflow == int((~ok).sum()), (n_bins, len(v))
            assert int(hist.sum()) + overflow == len(v)
