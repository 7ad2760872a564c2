"""The designed streams of tests/metrics_design.py hold every case they name, a handful of subtly wrong models each differ
from the right one on some named case, and the model the GPU tests hold the kernels against
(tests/dist_util.OracleMetricsBackend continuing a scan from `before`) says what the C oracle says about the same records
behind a prefix that qualifies exactly `before` times.  No GPU: this is what keeps tests/test_gpu_metrics_borders.py from
quietly testing something else than it names."""
import numpy as np
import pytest
import torch

from besst_amd.records import RecordBatch
from oracle import c_oracle as CO
from tests import metrics_design as MD

CAP = MD.CAP
_streams = {}


def stream(name):
    if name not in _streams:
        _streams[name] = dict(dense=MD.dense_stream, small=MD.small_sparse_stream, large=MD.large_sparse_stream,
                              values=MD.value_stream)[name]()
    return _streams[name]


def test_constants_mirror_the_source():
    for name, value in MD.source_constants().items():
        assert getattr(MD, name) == value, name
    assert MD.TILE == 4096 and MD.SUB == 1024 and MD.WAVE_RECORDS == 256
    assert [MD.tiles_per_wave(nt) for nt in (1, 66, 1024, 1025, 2048, 16384)] == [64, 64, 64, 128, 128, 1024]
    assert MD.where(0) == (0, 0, 0, 0, 0) and MD.where(4095) == (0, 3, 3, 63, 3) and MD.where(4096 + 1024 + 256 + 5) == (1, 1, 1, 1, 1)


@pytest.mark.parametrize('orientation', ['fr', 'rf'])
@pytest.mark.parametrize('name', ['dense', 'small', 'large', 'values'])
def test_cases_are_present(name, orientation):
    s = stream(name)
    # (the large stream: the two statements of the model are compared on every fourth case - 0.2 s each at 4 M records)
    found = MD.cases_present(s, orientation, agree_every=4 if name == 'large' else 1)
    assert len(found) == len(s.cases)
    if name == 'large':
        assert s.n == 1024 * 4096 + 5 and MD.tiles_per_wave(-(-s.n // MD.TILE)) == 128
    if name == 'small':
        assert s.n == 65 * 4096 + 5


def test_count_stream_needs_a_second_turn():
    s = MD.count_stream()
    assert s.n == 1_048_576 + 1025 and -(-s.n // MD.SUB) > MD.COUNT_TURN
    top = s.kind != MD.NON_TOP
    assert top[:MD.COUNT_TURN * MD.SUB].any() and top[MD.COUNT_TURN * MD.SUB:].any()     # both turns count something


@pytest.mark.parametrize('orientation', ['fr', 'rf'])
def test_every_mutant_is_told_apart(orientation):
    kills = MD.mutant_kills([stream('dense'), stream('small')], orientation)
    assert set(kills) == set(MD.mutants()) and all(kills.values())
    # the two tile-granular mutants die only where a tile ends at, or one past, exactly 1,000,000
    assert all('last' in k or 'k=4096' in k or 'k=8192' in k or 'k=12293' in k
               for k in kills['inside_tile_left_to_the_straddle_path'])


def _prefix(before, orientation):
    """Records that qualify exactly (a0, b0, d0) times: d0 D records first (inside B's cut-off whatever b0 is), a0 A
    records, plain mapped top records for the rest of b0.  Their values lie above every value of a designed stream."""
    a0, b0, d0 = before
    kind = np.concatenate([np.full(d0, MD.K_D, np.int8), np.full(a0, MD.K_A, np.int8),
                           np.full(b0 - a0 - d0, MD.K_PLAIN, np.int8)])
    b = MD.make_batch(kind, orientation)
    b.tlen[:] = np.where(b.tlen < 0, b.tlen - 5_000_000, b.tlen + 5_000_000)
    return b


def _pin(s, case, orientation):
    a0, b0, d0 = case.before
    assert d0 <= CAP
    sl = s.batch(orientation)
    whole = RecordBatch.concatenate([_prefix(case.before, orientation), sl]) if b0 else sl
    isize, contam, counts = CO.metrics_sample(whole, s.top, orientation, case.min_mapq, case.read_len, case.want_isize)
    samples, state = s.model(orientation).emit(torch.tensor(case.before), orientation, case.min_mapq, case.read_len,
                                               case.want_isize)
    samples, state = samples.numpy(), [int(x) for x in state]
    a_in = min(a0, CAP) if case.want_isize else 0
    n_isize = min(state[0], CAP) if case.want_isize else 0
    n_contam = d0 + state[4]
    assert counts.tolist() == [n_isize, n_contam, min(b0, CAP) + state[3], min(state[1], CAP)], case.name
    assert state[5] == len(sl)
    assert np.array_equal(isize[a_in:], samples[a_in:n_isize]), case.name
    assert not samples[:a_in].any() and not samples[n_isize:CAP].any(), case.name
    assert (isize[:a_in] > 5_000_000).all()
    assert np.array_equal(contam[d0:], samples[CAP + d0:CAP + n_contam]), case.name
    assert not samples[CAP:CAP + d0].any() and not samples[CAP + n_contam:].any(), case.name


@pytest.mark.parametrize('orientation', ['fr', 'rf'])
@pytest.mark.parametrize('name', ['dense', 'small', 'values'])
def test_model_continuing_a_scan_is_the_c_oracle_behind_a_prefix(name, orientation):
    s = stream(name)
    pinned = 0
    for case in s.cases:
        if case.consistent:                                     # (the others start from counts no stream produces)
            _pin(s, case, orientation)
            pinned += 1
    assert pinned >= len(s.cases) - 2
