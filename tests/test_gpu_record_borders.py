"""The record loop at its structural and rule borders: every designed stream of tests/record_design.py (what each one holds,
and why, is checked without a GPU in tests/test_record_design.py) through every form of the loop that can serve it -

  two-pass            stream_kernel + ordered_kernel (BESST_RECORD_PATH=0), with the mate-bit column and without
  fused, keys         fused_wave_kernel<false, .> behind a builder whose tuple capacity is the record count
  fused, runs         fused_wave_kernel<true, .> behind a builder of 4.3 M tuples: the loop groups the runs (in_record_loop 3)
  fused, digits       the same builder with BESST_REDUCE_NO_RUNS: the loop writes keys and counts the sort's digits (1)
  BESST_LOOP_RUNS=0   keys in the block segments, rg_group_kernel finds the runs (2): one child process for all streams
  context             device.GraphContext, the chain and ring streams pushed in three parts that cut a lane's four records and
                      a sub-tile

- each against oracle/py_oracle.record_loop (gpu_util.assert_matches_oracle) and against the C oracle's tuple stream and its
aggregation (assert_table_equals_c_oracle: rows, offsets, first_idx, masks, every observation in order).  Everything is an
integer: equality, no tolerance.  Every builder runs two steps; the second starts from what the first left."""
import os
import subprocess
import sys

import pytest

from tests import record_design as D

pytestmark = pytest.mark.gpu

CAP = 4_300_000          # a tuple capacity beyond 4 M: stage 2 takes its run-grouped form, the loop groups the runs
_ORACLE = {}


def oracle(name):
    """(stream, RecordBatch, {table, lib, node_bits}, py oracle's LoopResult), computed once per session."""
    if name not in _ORACLE:
        from oracle import py_oracle as O
        s = D.all_streams()[name]
        rec, table, p = D.as_oracle_inputs(s)
        wl = dict(table=D.table_columns(), lib=s.lib, node_bits=D.NODE_BITS)
        _ORACLE[name] = (s, D.as_batch(s), wl, O.record_loop(rec, table, p))
    return _ORACLE[name]


def check(name, table, aligned, ctr):
    from tests import gpu_util as DU
    from tests.test_gpu_fullsize import assert_table_equals_c_oracle
    s, batch, wl, loop = oracle(name)
    DU.assert_matches_oracle(table, aligned, ctr, loop, D.N_CONTIGS)
    assert (ctr.n_reach, ctr.n_tuples) == (loop.n_reach, sum(r.n + r.fishy for r in loop.edges.values()))
    assert_table_equals_c_oracle(table, aligned, ctr, batch, wl)


def set_library(gb, lib):
    """The builder's library constants (the struct its marshalled argument lists point to), changed in place."""
    p = gb.params
    p.read_len, p.ins_size_threshold, p.min_mapq = float(lib['read_len']), float(lib['ins_size_threshold']), int(lib['min_mapq'])
    p.orientation = {'fr': 0, 'rf': 1}[lib['orientation']]
    p.detect_duplicate, p.extend_paths, p.no_score = (int(bool(lib[k])) for k in ('detect_duplicate', 'extend_paths', 'no_score'))


def run_builder(gb, name, flags=0):
    """Two steps of the stream on the builder -> (table, coverage, counters, presort description or None)."""
    from besst_amd import pipeline
    s, batch, _, _ = oracle(name)
    set_library(gb, s.lib)
    gb.sort_flags = flags
    rec = pipeline.DeviceRecords(batch, gb.device)
    for _ in range(2):
        gb.step(rec)
    table = gb.fetch_table()
    spec = gb._args.get('presort')
    return table, gb.aligned.cpu().numpy(), gb.read_counters(), (spec[0] if spec and spec[1] else None)


def small_builder(name):
    import torch
    from besst_amd import pipeline
    s, batch, _, _ = oracle(name)
    dev = torch.device('cuda', 0)
    gb = pipeline.DeviceGraphBuilder(dev, D.N_CONTIGS, D.NODE_BITS, s.lib, len(batch), len(batch))
    gb.set_contigs(**D.table_columns())
    return gb


def make_large_builder():
    import torch
    from besst_amd import pipeline
    dev = torch.device('cuda', 0)
    n = max(len(s.records['tid']) for s in D.all_streams().values())
    gb = pipeline.DeviceGraphBuilder(dev, D.N_CONTIGS, D.NODE_BITS, D.make_lib(), n, CAP)
    gb.set_contigs(**D.table_columns())
    return gb


@pytest.fixture(scope='module')
def large_builder():
    """One builder of 4.3 M tuples for the module; a test sets its library constants and flags."""
    yield make_large_builder()


@pytest.mark.parametrize('bits', ['1', '0'])
@pytest.mark.parametrize('path', ['0', '1'])
@pytest.mark.parametrize('name', D.STREAM_NAMES)
def test_two_pass_and_fused_loop_writing_keys(name, path, bits, monkeypatch):
    monkeypatch.setenv('BESST_RECORD_PATH', path)
    monkeypatch.setenv('BESST_MATE_BITS', bits)
    gb = small_builder(name)
    table, aligned, ctr, _ = run_builder(gb, name)
    assert gb.params.record_path == int(path)
    check(name, table, aligned, ctr)


@pytest.mark.parametrize('bits', ['1', '0'])
@pytest.mark.parametrize('name', D.STREAM_NAMES)
def test_fused_loop_grouping_runs(name, bits, large_builder, monkeypatch):
    """The loop names the runs itself - unless a block closes more chunks than its tables hold: then stage 2 reports the
    overflow, the pass is repeated with BESST_REDUCE_NO_RUNS, and the table is exact all the same."""
    from besst_amd import pipeline
    monkeypatch.setenv('BESST_RECORD_PATH', '1')
    monkeypatch.setenv('BESST_MATE_BITS', bits)
    table, aligned, ctr, spec = run_builder(large_builder, name)
    assert spec is not None and spec.segmented == 1, 'stage 2 should take the hand-over from the record loop'
    if oracle(name)[0].claims.get('over'):
        assert large_builder.sort_flags == pipeline.REDUCE_NO_RUNS and spec.in_record_loop == 1
    else:
        assert large_builder.sort_flags == 0 and spec.in_record_loop == 3
    check(name, table, aligned, ctr)


@pytest.mark.parametrize('name', D.STREAM_NAMES)
def test_fused_loop_counting_digits(name, large_builder, monkeypatch):
    from besst_amd import pipeline
    monkeypatch.setenv('BESST_RECORD_PATH', '1')
    monkeypatch.delenv('BESST_MATE_BITS', raising=False)
    table, aligned, ctr, spec = run_builder(large_builder, name, flags=pipeline.REDUCE_NO_RUNS)
    assert spec is not None and spec.in_record_loop == 1 and large_builder.sort_flags == pipeline.REDUCE_NO_RUNS
    check(name, table, aligned, ctr)


@pytest.mark.parametrize('span', ['1', '2'])
@pytest.mark.parametrize('form', ['two-pass', 'fused keys', 'fused runs'])
@pytest.mark.parametrize('name', ['chain_detect', 'chain_count'])
def test_chain_streams_across_span_borders(name, form, span, large_builder, monkeypatch):
    """BESST_STITCH_SPAN 1 and 2: the dropped heads' predecessors lie in other spans (and, with 2, one in the head's own)."""
    monkeypatch.setenv('BESST_STITCH_SPAN', span)
    monkeypatch.setenv('BESST_RECORD_PATH', '0' if form == 'two-pass' else '1')
    monkeypatch.delenv('BESST_MATE_BITS', raising=False)
    gb = large_builder if form == 'fused runs' else small_builder(name)
    table, aligned, ctr, spec = run_builder(gb, name)
    if form == 'fused runs':
        assert spec is not None and spec.in_record_loop == 3 and gb.sort_flags == 0
    check(name, table, aligned, ctr)


CONTEXT_STREAMS = ['chain_detect', 'chain_count'] + ['ring_n%d' % n for n in D.RING_LENGTHS]


@pytest.mark.parametrize('path', ['0', '1'])
@pytest.mark.parametrize('name', CONTEXT_STREAMS)
def test_context_layer_pushed_in_three_parts(name, path, monkeypatch):
    from besst_amd import device
    monkeypatch.setenv('BESST_RECORD_PATH', path)
    monkeypatch.delenv('BESST_MATE_BITS', raising=False)
    s, batch, wl, _ = oracle(name)
    n = len(batch)
    cuts = [0, (n // 3) // 4 * 4 + 1, (2 * n // 3) // D.SUB * D.SUB + 130, n]   # inside a lane's four records; inside a sub-tile
    assert cuts[1] % 4 == 1 and cuts[2] % D.SUB == 130 and cuts[1] < cuts[2] < n
    lib = s.lib
    with device.GraphContext(0) as ctx:
        ctx.set_contigs(**wl['table'])
        ctx.set_library(lib['read_len'], lib['ins_size_threshold'], lib['min_mapq'], lib['orientation'], lib['detect_duplicate'],
                        lib['extend_paths'], lib['no_score'])
        for lo, hi in zip(cuts[:-1], cuts[1:]):
            ctx.push_records(batch.slice(lo, hi))
        for _ in range(2):
            table, aligned, ctr = ctx.build_graph()
            check(name, table, aligned, ctr)


_CHILD = r'''
import sys
sys.path.insert(0, %(repo)r)
from tests import record_design as D
from tests import test_gpu_record_borders as T
gb = T.make_large_builder()
for name in D.STREAM_NAMES:
    table, aligned, ctr, spec = T.run_builder(gb, name)
    assert spec is not None and spec.in_record_loop == 2 and gb.sort_flags == 0, (name, spec and spec.in_record_loop, gb.sort_flags)
    T.check(name, table, aligned, ctr)
print('ALL EQUAL')
'''


def test_every_stream_with_the_grouping_kernel():
    """BESST_LOOP_RUNS=0 (read once per process, hence a fresh child): the loop leaves keys in the block segments and
    rg_group_kernel finds the runs - every stream, the one with a chunk too many included (nothing overflows here)."""
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, BESST_LOOP_RUNS='0', BESST_RECORD_PATH='1')
    env.pop('BESST_MATE_BITS', None)
    env.pop('BESST_STITCH_SPAN', None)
    out = subprocess.run([sys.executable, '-c', _CHILD % dict(repo=repo)], env=env, capture_output=True, text=True, timeout=600)
    assert 'ALL EQUAL' in out.stdout, (out.stdout[-2000:], out.stderr[-3000:])
