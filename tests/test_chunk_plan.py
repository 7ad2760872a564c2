"""GenerateOutput.chunk_plan: where the one pipeline of the device-produced files (write_chunks) cuts a file into chunks.
Pure Python; the pipeline itself runs in tests/test_gpu_byte_pipeline.py."""
import pytest

from besst_amd import GenerateOutput as GO

PAYLOAD = 256
STEP = 3 * PAYLOAD
TOTALS = (0, 1, 767, 768, 769, 1536, 2305)


@pytest.fixture(autouse=True)
def small_blocks(monkeypatch):
    monkeypatch.setattr(GO, 'BGZF_BLOCK_PAYLOAD', PAYLOAD)


@pytest.mark.parametrize('deflate', [False, True])
@pytest.mark.parametrize('total', TOTALS)
def test_plan_tiles_the_file(total, deflate):
    plan = GO.chunk_plan(total, STEP, deflate)
    if total == 0:
        assert plan == ([(0, 0, True)] if deflate else [])         # the empty chunk carries the EOF block
        return
    assert len(plan) == -(-total // STEP)
    assert plan[0][0] == 0 and plan[-1][1] == total
    assert [p[0] for p in plan[1:]] == [p[1] for p in plan[:-1]]    # each begins where the one before ended
    assert all(end > begin for begin, end, _last in plan)
    assert [last for _b, _e, last in plan] == [False] * (len(plan) - 1) + [True]
    assert all(end - begin == STEP for begin, end, _last in plan[:-1])
    if deflate:
        assert all((end - begin) % PAYLOAD == 0 for begin, end, _last in plan[:-1])


def test_deflate_chunks_are_whole_blocks_within_the_chunk_size():
    assert GO.bgzf_chunk(STEP + 100) == STEP and GO.bgzf_chunk(1) == PAYLOAD
    for total in TOTALS:
        assert GO.chunk_plan(total, STEP + 100, True) == GO.chunk_plan(total, STEP, True)
    assert GO.chunk_plan(600, 1, True) == [(0, 256, False), (256, 512, False), (512, 600, True)]


def test_plain_chunks_are_cut_at_the_size_asked_for():
    assert GO.chunk_plan(3, 1, False) == [(0, 1, False), (1, 2, False), (2, 3, True)]
    assert GO.chunk_plan(15, 7, False) == [(0, 7, False), (7, 14, False), (14, 15, True)]
    assert GO.chunk_plan(STEP, STEP + 100, False) == [(0, STEP, True)]
