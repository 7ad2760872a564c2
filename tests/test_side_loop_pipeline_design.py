"""CPU: the streams of tests/test_gpu_side_loop_pipeline.py have the properties they are named for.  Every generator asserts
its own design - lengths against the block size, entries and rounds per block by the numpy statement of the side stream,
run bits per sub-tile by counting, the chain across the launch border by the replay and the census - so making a stream is
the test; here they are made without a GPU, and the table with every contig present is held against the designed one."""
import numpy as np
import pytest

from tests import record_design as D
from tests import test_gpu_side_loop_pipeline as P


@pytest.mark.parametrize('key', sorted(P.STREAMS))
def test_stream_has_its_property(key):
    s = P.made(key)
    n = len(s.records['tid'])
    assert all(len(v) == n for v in s.records.values()) and s.name.startswith('pipe_')


def test_cases_cover_both_tables_and_every_stream():
    assert {k for k, _ in P.CASES} == set(P.STREAMS) and {t for _, t in P.CASES} == {'absent', 'present'}
    assert sorted(n % D.BLOCK for n in P.SPLIT_LENGTHS) == [0, 1, D.SUB, D.BLOCK - 1, D.BLOCK - 1]
    assert min(P.SPLIT_LENGTHS) // D.BLOCK == 0


def test_present_table_differs_in_the_absent_rows_only():
    a, p = P.TABLES['absent'], P.TABLES['present']
    rows = [r for r in range(D.N_CONTIGS) if any(a[k][r] != p[k][r] for k in a)]
    assert rows == list(P.ABSENT) and len(set(p['scaf'][r] for r in rows)) == len(rows)
    assert not set(p['scaf'][r] for r in rows) & set(a['scaf'])


def test_unroll_factor_is_the_source_s():
    src = open(D.CSRC + '/classify.hip').read()
    assert 'for (int it = 0; it < iters; it += %d)' % P.UNROLL in src
