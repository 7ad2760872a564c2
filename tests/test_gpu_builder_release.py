"""GPU: a DeviceGraphBuilder that is dropped frees its device buffers at once.

reduce() keeps a closure that repeats the stage-2 call (self._redo).  Bound to the builder it made every builder that had
run a step a reference cycle: its buffers - 1.2 GB for a builder of 4.3 M tuples - stayed allocated until some later garbage
collection, and whatever measured the allocator in between (tests/test_gpu_two_ranks.py's memory budget) saw them go."""
import gc
import weakref

import pytest

from tests import record_design as D
from tests import test_gpu_record_borders as T

pytestmark = pytest.mark.gpu


def stream():
    """One full block and a few records: large / large links all along, so that both stages run and emit."""
    lib = D.make_lib()
    b = D.Builder(D.BLOCK + 40, lib, filler_rows=[D.LARGE[0]])
    for i in range(5, b.n, 97):
        b.link(i, D.LARGE[0], D.LARGE[10 + i % 20], *D.distinct_obs(i))
    rec = b.records()
    assert D.replay(rec, D.TABLE, lib).emit.sum() > 100
    return D.Stream('release', rec, lib, {})


@pytest.mark.parametrize('grouping', [False, True], ids=['writing keys', 'grouping runs'])
def test_dropped_builder_is_freed_without_a_collection(grouping, monkeypatch):
    import torch
    from besst_amd import pipeline
    s = stream()
    batch = D.as_batch(s)
    dev = torch.device('cuda', 0)
    gc.collect()
    was_enabled = gc.isenabled()
    gc.disable()
    try:
        before = torch.cuda.memory_allocated(dev)
        gb = pipeline.DeviceGraphBuilder(dev, D.N_CONTIGS, D.NODE_BITS, s.lib, len(batch), T.CAP if grouping else len(batch))
        gb.set_contigs(**D.table_columns())
        monkeypatch.setenv('BESST_RECORD_PATH', '1')
        T.set_library(gb, s.lib)
        gb.sort_flags = 0
        rec = pipeline.DeviceRecords(batch, dev)
        for _ in range(2):
            gb.step(rec)
        table = gb.fetch_table()
        assert len(table.key) == 20                          # (one edge per mate contig: LARGE[10 .. 29])
        with_builder = torch.cuda.memory_allocated(dev)
        own = sum(t.numel() * t.element_size() for t in (gb.ws1, gb.ws2, gb.keys, gb.payload))     # nobody else holds these
        assert 0 < own <= with_builder - before
        ref = weakref.ref(gb)
        del gb, table, rec
        assert ref() is None
        assert torch.cuda.memory_allocated(dev) <= with_builder - own
    finally:
        if was_enabled:
            gc.enable()
